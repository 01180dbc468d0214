// fr_cluster_math.h -- the arithmetic of DBSCAN and of the target selection of global_planning (fr_cluster.hip), host/device-neutral:
// the kernels and the g++ harness (tests/harness/fr_cluster_harness.cpp) compile these same functions, so a brute-force CPU run over
// them states the kernels' results bit for bit.
//
// The statement is the middle of the reference's global_planning (models/SLAM/gaussian.py:1216-1276): the Gaussians of a height
// band, torch.quantile of their scores, sklearn.cluster.DBSCAN on those above it, the cluster with the highest score.
// Everything is binary32, one rounding per written operation (the build has -ffp-contract=off; the two fmaf below are written,
// not contracted), and every operand order is the one written here.
//
// The labelling rule (it gives sklearn's labels_):
//   * a point is CORE when at least min_samples points lie within eps of it, itself included, the test being frk_inside (<=);
//   * clusters are the connected components of the core points under "within eps";
//   * clusters are numbered 0, 1, ... by ascending lowest original index of their core points;
//   * a point that is not core takes the lowest cluster number among the core points within eps of it, or -1 (noise);
//   * a point with a non-finite coordinate is noise and nobody's neighbour.
#ifndef FR_CLUSTER_MATH_H_INCLUDED
#define FR_CLUSTER_MATH_H_INCLUDED

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define FRK_HD __host__ __device__ __forceinline__
#else
#define FRK_HD inline
#endif

#define FRK_CELL_BITS 10
#define FRK_CELLS 1024                /* cells per axis of the search grid */
#define FRK_NO_CODE 0xFFFFFFFFu       /* the cell code of a point with a non-finite coordinate: behind every 30-bit code */
#define FRK_SIDE_FACTOR 1.125f        /* smallest cell side over eps: see frk_cell */

FRK_HD uint32_t frk_bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
FRK_HD float frk_float(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }

// finite: the exponent field is not all ones (no libm call, the same test on both sides)
FRK_HD bool frk_finite(float v) { return (frk_bits(v) & 0x7f800000u) != 0x7f800000u; }
FRK_HD bool frk_finite3(float x, float y, float z) { return frk_finite(x) && frk_finite(y) && frk_finite(z); }

// eps is usable when eps * eps is a normal number: below that the squares of differences larger than eps underflow to "inside"
FRK_HD float frk_eps2(float eps) { return eps * eps; }
FRK_HD bool frk_eps_ok(float eps) { const float e2 = eps * eps; return eps > 0.0f && frk_finite(e2) && e2 >= 1.17549435e-38f; }

FRK_HD float frk_dist2(float px, float py, float pz, float qx, float qy, float qz)
{
	const float dx = px - qx, dy = py - qy, dz = pz - qz;
	return (dx * dx + dy * dy) + dz * dz;
}
FRK_HD bool frk_inside(float d2, float eps2) { return d2 <= eps2; }

// ---- the search grid ----------------------------------------------------------------------------------------------------------------
// Per axis: side = max(eps * FRK_SIDE_FACTOR, extent / FRK_CELLS), cell = floor((p - lo) / side) clamped to [0, FRK_CELLS - 1].
// Guarantee: two finite points that frk_inside accepts differ by at most ONE cell on every axis, so a point's neighbours lie in the
// 27 cells around its own.  Proof.  frk_inside gives fl(dx * dx) <= eps2, so |p - q| <= eps (1 + 2^-22) on the axis (three roundings;
// frk_eps_ok keeps the squares away from underflow).  u = (p - lo) / side has two roundings: u = u_true (1 + d), |d| < 2^-22.9, and
// u_true <= extent / side <= FRK_CELLS (1 + 2^-23), so |u - u_true| < 2^-12.8.  side >= 1.125 eps (1 - 2^-24), so u_true(p) and
// u_true(q) differ by less than 0.8889 + 2^-21 and the computed values by less than 0.8889 + 2^-11.7 < 1: their floors differ by at
// most 1, and the clamp is monotone.  (With a side equal to eps the difference could reach 1 + 2^-11.8: two cells apart.)
// A cloud wider than FRK_CELLS sides gets larger cells on that axis alone: slower, never wrong.  An extent that overflows gives
// side = inf and u = 0 or NaN, both cell 0.
FRK_HD float frk_side(float lo, float hi, float eps)
{
	const float smin = eps * FRK_SIDE_FACTOR;
	const float s = (hi - lo) / (float)FRK_CELLS;
	return s > smin ? s : smin;                              // (no finite point: lo = +inf, hi = -inf, s = -inf)
}
FRK_HD uint32_t frk_cell(float p, float lo, float side)
{
	float u = (p - lo) / side;
	u = u > 0.0f ? u : 0.0f;                                 // (NaN goes to 0 as well)
	u = u < (float)(FRK_CELLS - 1) ? u : (float)(FRK_CELLS - 1);
	return (uint32_t)u;
}
// x fastest: the cells (cx - 1 .. cx + 1, cy, cz) are one contiguous run of the points sorted by code
FRK_HD uint32_t frk_code(uint32_t cx, uint32_t cy, uint32_t cz) { return (cz << (2 * FRK_CELL_BITS)) | (cy << FRK_CELL_BITS) | cx; }
FRK_HD uint32_t frk_point_code(float x, float y, float z, const float* lo, const float* side)
{
	return frk_code(frk_cell(x, lo[0], side[0]), frk_cell(y, lo[1], side[1]), frk_cell(z, lo[2], side[2]));
}

// ---- the band, the quantile and the winner -----------------------------------------------------------------------------------------

// gaussian.py:1221: lower_y <= y <= upper_y (a NaN height is outside)
FRK_HD bool frk_in_band(float y, float lower_y, float upper_y) { return y >= lower_y && y <= upper_y; }

// unsigned order = float order; -0 is +0 (they are equal to a sort); NaNs sort to the two ends
FRK_HD uint32_t frk_enc(float f)
{
	uint32_t u = frk_bits(f);
	if (u == 0x80000000u) u = 0u;
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
FRK_HD float frk_dec(uint32_t e) { return frk_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e); }

// torch.quantile(x, q), interpolation "linear", on n values: rank = fl(q * fl(n - 1)); the two order statistics floor(rank) and
// ceil(rank) (0-based, ascending), weight = rank - floor(rank) (exact)
FRK_HD void frk_quantile_rank(float q, uint32_t n, uint32_t* below, uint32_t* above, float* weight)
{
	const float rank = q * (float)(n - 1u);
	const float fl = floorf(rank), ce = ceilf(rank);
	uint32_t b = (uint32_t)fl, a = (uint32_t)ce;
	if (b > n - 1u) b = n - 1u;                               // (n - 1 beyond 2^24 may round up)
	if (a > n - 1u) a = n - 1u;
	*below = b; *above = a; *weight = rank - fl;
}
// torch's lerp, as its kernels evaluate it: one fused multiply-add from the nearer end.  This form equals torch.quantile on the CPU
// bit for bit for every n in 1..4096 (tests/test_cluster_cpu.py); a + w * (b - a) with two roundings does not (n = 7, 18, 90, ...).
FRK_HD float frk_lerp(float a, float b, float w)
{
	const float diff = b - a;
	return w < 0.5f ? fmaf(w, diff, a) : fmaf(w - 1.0f, diff, b);
}

// gaussian.py:1227: strictly above the threshold
FRK_HD bool frk_above(float score, float threshold) { return score > threshold; }

// gaussian.py:1247-1257: the loop starts from max_score = -1 and takes a cluster on strict >, so the lowest label wins a tie and a
// cluster whose best score is not above -1 never wins; then -1 stays, which selects the NOISE points at 1266-1267
#define FRK_START_SCORE (-1.0f)
FRK_HD bool frk_beats(float cluster_score, float max_score) { return cluster_score > max_score; }

#endif
