// fr_cloud_math.h -- the arithmetic of the nearest-point search over a cloud index (fr_cloud.hip), host/device-neutral: the kernels
// and the g++ harness (tests/harness/fr_cloud_harness.cpp) compile these same functions, so a brute-force CPU run over them states
// the kernels' results bit for bit.
//
// The statement is "distance from each point of cloud A to the nearest point of cloud B", which the reference takes from a KD-tree in
// accuracy_comp_ratio_from_pcl (scripts/eval_3d_reconstruction.py:84-125) and novelty_mask_from_pcd_nn (test_utils.py:503-578).
// Everything is binary32, one rounding per written operation (the build has -ffp-contract=off and an IEEE sqrt), and every operand
// order is the one written here.
#ifndef FR_CLOUD_MATH_H_INCLUDED
#define FR_CLOUD_MATH_H_INCLUDED

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define FRC_HD __host__ __device__ __forceinline__
#else
#define FRC_HD inline
#endif

#define FRC_BLOCK 256                 /* queries per partial sum of the statistics (a workgroup of the reduction) */
#define FRC_NO_CODE 0xFFFFFFFFu       /* the Morton word of a point with a non-finite coordinate: behind every 30-bit code */

FRC_HD uint32_t frc_bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }

// finite: the exponent field is not all ones (no libm call, the same test on both sides)
FRC_HD bool frc_finite(float v) { return (frc_bits(v) & 0x7f800000u) != 0x7f800000u; }
FRC_HD bool frc_finite3(float x, float y, float z) { return frc_finite(x) && frc_finite(y) && frc_finite(z); }

// the squared distance from query q to target t
FRC_HD float frc_dist2(float qx, float qy, float qz, float tx, float ty, float tz)
{
	const float dx = qx - tx, dy = qy - ty, dz = qz - tz;
	return (dx * dx + dy * dy) + dz * dz;
}

// A lower bound of frc_dist2(q, t) over every t inside the box [lo, hi], AS COMPUTED: per axis the difference to the nearer face
// where q is outside the slab, 0 inside it, then the same squares and the same two sums in the same order.  q - t is rounded
// monotonically in t, so |fl(q - t)| >= |fl(q - face)| for t beyond the face; squares and sums of non-negative terms are monotone
// under rounding too.  A box no point was put into has lo = +inf, hi = -inf: its bound is +inf.
FRC_HD float frc_box_dist2(float qx, float qy, float qz, const float* lo, const float* hi)
{
	const float dx = qx < lo[0] ? qx - lo[0] : (qx > hi[0] ? qx - hi[0] : 0.0f);
	const float dy = qy < lo[1] ? qy - lo[1] : (qy > hi[1] ? qy - hi[1] : 0.0f);
	const float dz = qz < lo[2] ? qz - lo[2] : (qz > hi[2] ? qz - hi[2] : 0.0f);
	return (dx * dx + dy * dy) + dz * dz;
}

// candidate (d2, idx) against the best so far: smaller distance, or the same distance at a lower original index
FRC_HD bool frc_better(float d2, int32_t idx, float best_d2, int32_t best_idx)
{
	return d2 < best_d2 || (d2 == best_d2 && (uint32_t)idx < (uint32_t)best_idx);
}

FRC_HD float frc_distance(float d2) { return sqrtf(d2); }

// The seeded ("fold") search: a running squared distance against a candidate.  min over a union of target sets = min of the minima,
// exactly: both are values of frc_dist2 (never -0, never NaN for finite operands), and the smaller of two floats is one of them.
// Equal values keep the seed's bits; a candidate replaces the seed only when it is strictly smaller, so no index is kept and the
// box tests of a fold may prune strictly (frc_fold_may_improve).
FRC_HD float frc_fold(float seed_d2, float d2) { return d2 < seed_d2 ? d2 : seed_d2; }
FRC_HD bool frc_fold_may_improve(float bound_d2, float best_d2) { return bound_d2 < best_d2; }

FRC_HD uint32_t frc_spread10(uint32_t x)
{
	x = (x | (x << 16)) & 0x030000FFu;
	x = (x | (x << 8)) & 0x0300F00Fu;
	x = (x | (x << 4)) & 0x030C30C3u;
	x = (x | (x << 2)) & 0x09249249u;
	return x;
}

// the 30-bit Morton code of a finite point in the frame [lo, hi] of the index's finite targets; a point outside the frame is
// clamped onto it (a query need not lie among the targets).  The code only orders work: no result depends on it.
FRC_HD uint32_t frc_morton(float x, float y, float z, const float* lo, const float* hi)
{
	const float p[3] = {x, y, z};
	uint32_t code = 0;
	for (int a = 0; a < 3; a++)
	{
		const float ext = hi[a] - lo[a];
		float u = ext > 0.0f ? (p[a] - lo[a]) / ext : 0.0f;
		u = u > 0.0f ? u : 0.0f;                          // (a NaN from inf / inf goes to 0 as well)
		u = u < 1.0f ? u : 1.0f;
		code |= frc_spread10((uint32_t)(u * 1023.0f)) << a;
	}
	return code;
}

// test_utils.py:531: a pixel has a depth when it is finite and positive
FRC_HD bool frc_depth_valid(float d) { return frc_finite(d) && d > 0.0f; }

// tester_gaussians_navigation.py:515, (object_mask_bw > 0) & (depth > 0): with a mask a pixel is a query only where its mask byte
// is not 0 and it has a depth; a masked-out pixel is a pixel without a depth in every respect
FRC_HD bool frc_sample_is_query(float d, int has_mask, uint8_t mask_byte) { return (!has_mask || mask_byte != 0) && frc_depth_valid(d); }

// test_utils.py:544-550: the pixel (u, v) at depth d through kinv [9] into the camera frame, the camera z negated for a camera that
// looks along -Z, then through c2w [12] (the top three rows of a row-major 4 x 4) into the world
FRC_HD void frc_back_project(int u, int v, float d, const float* kinv, const float* c2w, int flip_z, float* p)
{
	const float fu = (float)u, fv = (float)v;
	const float rx = (kinv[0] * fu + kinv[1] * fv) + kinv[2];
	const float ry = (kinv[3] * fu + kinv[4] * fv) + kinv[5];
	const float rz = (kinv[6] * fu + kinv[7] * fv) + kinv[8];
	const float X = rx * d, Y = ry * d;
	float Z = rz * d;
	if (flip_z) Z = -Z;
	for (int r = 0; r < 3; r++) p[r] = ((c2w[4 * r + 0] * X + c2w[4 * r + 1] * Y) + c2w[4 * r + 2] * Z) + c2w[4 * r + 3];
}

// eval_3d_reconstruction.py:104: within the threshold (strict);  test_utils.py:559: novel beyond it (strict)
FRC_HD bool frc_flag_near(float d, float th) { return d < th; }
FRC_HD bool frc_flag_novel(float d, float th) { return d > th; }

// The sum of the distances, in binary64 and in one fixed order (no atomics).  A partial is the sum over FRC_BLOCK consecutive
// queries in caller order (those left out add +0.0): per 64 of them the butterfly v[l] += v[l ^ o], o = 32 .. 1 -- addition
// commutes, so every lane holds the same bits --, then the four results from left to right.  The total takes the partials
// strided: slot t = p[t] + p[t + FRC_BLOCK] + ..., then the same block sum over the slots.
FRC_HD double frc_sum64(double* v)                   // v[64] is used up
{
	for (int o = 32; o > 0; o >>= 1)
		for (int l = 0; l < o; l++) v[l] = v[l] + v[l + o];
	return v[0];
}
FRC_HD double frc_sum_block(const double* v)          // v[FRC_BLOCK]
{
	double w[4];
	for (int k = 0; k < 4; k++)
	{
		double t[64];
		for (int l = 0; l < 64; l++) t[l] = v[64 * k + l];
		w[k] = frc_sum64(t);
	}
	return ((w[0] + w[1]) + w[2]) + w[3];
}

#endif
