// fr_cloud.hip -- nearest-point search of one cloud against a persistent index over another (gfx950).
//
// What the reference does on the host with a KD-tree it rebuilds on every call: accuracy_comp_ratio_from_pcl
// (scripts/eval_3d_reconstruction.py:84-125: three trees, three queries) and novelty_mask_from_pcd_nn (test_utils.py:503-578: a
// tree over the unchanging environment cloud, every frame).  Here the index is built once and outlives the call:
//
//   fr_cloud_index_build   k_cloud_minmax   bounding box and count of the FINITE targets (fr_block.h's frb_minmax3_finite, then
//                                           integer atomics on encoded floats)
//                          k_cloud_tkeys    Morton code << 32 | original index; a non-finite target gets FRC_NO_CODE and sorts last
//                          fr_sort_keys64   the 64-bit key sort of the Morton sort (fisher_rast.hip)
//                          k_cloud_gather   the sorted coordinates
//                          k_cloud_boxes    AABBs of 1024-point boxes and of 64-point sub-boxes over the finite prefix
//                          k_cloud_supers   AABBs of 16 boxes each: with two levels the linear scan of the boxes was up to 70 % of the
//                                           search at 2M targets (profiles/cloud_nn_bench.txt), so the scan is over these
//   fr_cloud_query         k_cloud_qkeys    "points": the queries' codes in the index's frame (clamped), sorted, so that the 64
//                                           queries of a wave are neighbours in space; "depth": a wave takes an 8 x 8 block of the
//                                           sample grid instead, and nothing is sorted
//                          k_cloud_search   wave-cooperative exact search, as k_knn_search: each lane's best is seeded from the
//                                           targets around its own key, then super-boxes -> boxes -> sub-boxes -> points are opened when ANY live
//                                           lane can still improve or tie there (pruning is non-strict: the lowest original index
//                                           among equal distances is part of the result); loop counters, bounds and candidates
//                                           are wave-uniform
//                                           <0, 1> is the FOLD of a running evaluation (cfg->seed_d2): best starts at the caller's
//                                           running squared distance and is written back, pruning is STRICT (no index, so no ties),
//                                           and a lane that the frame of all targets cannot improve is dead before the first load.
//                                           "depth" also takes a pixel mask, the near flag rule and writes the samples' points
//                                           (NaN rows where there is no query: a ready target cloud for fr_cloud_index_build)
//                          k_cloud_partials / k_cloud_total   the statistics, in caller order and one fixed order of sums
//                                           (fr_cloud_math.h: frc_sum_block): binary64 partials per 256 queries, no float atomics
//
// Nothing is allocated, nothing is read back, no environment variable is read; every launch and memset is on the caller's stream.
// The arithmetic is in fr_cloud_math.h, which tests/harness/fr_cloud_harness.cpp compiles with g++ for the bit-exact statement.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fr_internal.h"
#include "fr_block.h"
#include "fr_cloud_math.h"

#define FRC_THREADS 256
static_assert(FRC_THREADS == FRB_THREADS, "fr_block.h is written for 256 threads");
#define FRC_BOX 1024
#define FRC_SUB 64
#define FRC_SUPER 16                  // boxes per super-box: the level above the 1024-point boxes (16384 points)
#define FRC_SEED 2                   // targets tested on each side of a query's place among the sorted keys
#define FRC_MAX_GRID 2048

// the head of an index: the frame of the finite targets and their number, written by the build, read by every query
struct FrcHead
{
	float lo[3], hi[3];
	uint32_t nf;                      // finite targets: the sorted prefix the boxes cover
};

struct FrcIndexLayout { size_t head, keys, sorted, boxes, sboxes, supers, total; };
static FrcIndexLayout frc_index_layout(int64_t N)
{
	FrcIndexLayout L;
	size_t o = 0;
	L.head = o; o = fr_align256(o + sizeof(FrcHead));
	L.keys = o; o = fr_align256(o + (size_t)N * 8);
	L.sorted = o; o = fr_align256(o + (size_t)N * 12);
	L.boxes = o; o = fr_align256(o + (size_t)((N + FRC_BOX - 1) / FRC_BOX) * 24);
	L.sboxes = o; o = fr_align256(o + (size_t)((N + FRC_SUB - 1) / FRC_SUB) * 24);
	L.supers = o; o = fr_align256(o + (size_t)((N + FRC_SUPER * FRC_BOX - 1) / (FRC_SUPER * FRC_BOX)) * 24);
	L.total = o;
	return L;
}

struct FrcQueryLayout { size_t qkeys, dist, partials, total; };
static int64_t frc_blocks(int64_t M) { return (M + FRC_BLOCK - 1) / FRC_BLOCK; }
static FrcQueryLayout frc_query_layout(int64_t M)
{
	FrcQueryLayout L;
	size_t o = 0;
	L.qkeys = o; o = fr_align256(o + (size_t)M * 8);
	L.dist = o; o = fr_align256(o + (size_t)M * 4);
	L.partials = o; o = fr_align256(o + (size_t)frc_blocks(M) * 32 + 32);
	L.total = o;
	return L;
}

__device__ __forceinline__ uint32_t frc_enc(float f)
{
	const uint32_t u = frc_bits(f);
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float frc_dec(uint32_t e)
{
	return __uint_as_float((e & 0x80000000u) ? (e & 0x7fffffffu) : ~e);
}
__device__ __forceinline__ bool frc_any(bool p) { return __ballot(p) != 0ull; }

// ---- build ------------------------------------------------------------------------------------------------------------------------

// acc[0..2] = min, acc[3..5] = max of the finite targets (encoded so that unsigned order is float order), acc[6] = their number
__global__ __launch_bounds__(FRC_THREADS) void k_cloud_minmax(int N, const float* __restrict__ pts, uint32_t* __restrict__ acc)
{
	__shared__ float s_lo[3][4], s_hi[3][4];
	__shared__ uint32_t s_cnt[4];
	frb_minmax3_finite(pts, N, [](float x, float y, float z) { return frc_finite3(x, y, z); }, s_lo, s_hi, s_cnt);
	// one set of integer atomics per workgroup: their result does not depend on the order of arrival
	if (threadIdx.x < 3)
	{
		const int a = threadIdx.x;
		atomicMin(&acc[a], frc_enc(frb_min4(s_lo[a])));
		atomicMax(&acc[3 + a], frc_enc(frb_max4(s_hi[a])));
	}
	if (threadIdx.x == 3) atomicAdd(&acc[6], s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
}

// the head of the index from the accumulators (N = 0 launches this alone: an index with no target)
__global__ void k_cloud_head(const uint32_t* __restrict__ acc, FrcHead* __restrict__ head)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	for (int a = 0; a < 3; a++) { head->lo[a] = frc_dec(acc[a]); head->hi[a] = frc_dec(acc[3 + a]); }
	head->nf = acc[6];
}

__global__ __launch_bounds__(FRC_THREADS) void k_cloud_tkeys(int N, const float* __restrict__ pts, const uint32_t* __restrict__ acc,
                                                             uint64_t* __restrict__ keys)
{
	const int i = blockIdx.x * FRC_THREADS + threadIdx.x;
	if (i >= N) return;
	float lo[3], hi[3];
	for (int a = 0; a < 3; a++) { lo[a] = frc_dec(acc[a]); hi[a] = frc_dec(acc[3 + a]); }
	const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
	const uint32_t code = frc_finite3(x, y, z) ? frc_morton(x, y, z, lo, hi) : FRC_NO_CODE;
	keys[i] = ((uint64_t)code << 32) | (uint32_t)i;
}

__global__ __launch_bounds__(FRC_THREADS) void k_cloud_gather(int N, const float* __restrict__ pts, const uint64_t* __restrict__ keys,
                                                              float* __restrict__ sorted)
{
	const int t = blockIdx.x * FRC_THREADS + threadIdx.x;
	if (t >= N) return;
	const uint32_t i = (uint32_t)keys[t];
	sorted[3 * (size_t)t] = pts[3 * (size_t)i]; sorted[3 * (size_t)t + 1] = pts[3 * (size_t)i + 1]; sorted[3 * (size_t)t + 2] = pts[3 * (size_t)i + 2];
}

// A workgroup of four waves takes one 1024-point box, wave w its 64-point sub-boxes w, w + 4, ...; the box is the union of its
// sub-boxes.  Only the finite prefix [0, nf) is boxed: the search never reads a box or sub-box beyond it.
__global__ __launch_bounds__(FRC_THREADS) void k_cloud_boxes(const FrcHead* __restrict__ head, const float* __restrict__ sorted,
                                                             float* __restrict__ boxes, float* __restrict__ sboxes)
{
	__shared__ float red[6][4];
	const int nf = (int)head->nf;
	const int b = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	float blo[3] = { INFINITY, INFINITY, INFINITY }, bhi[3] = { -INFINITY, -INFINITY, -INFINITY };
	for (int k = w; k < FRC_BOX / FRC_SUB; k += 4)
	{
		const int sb = b * (FRC_BOX / FRC_SUB) + k;
		if (sb * FRC_SUB >= nf) break;
		const int t = sb * FRC_SUB + lane;
		float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
		if (t < nf)
		{
#pragma unroll
			for (int a = 0; a < 3; a++) { lo[a] = sorted[3 * (size_t)t + a]; hi[a] = lo[a]; }
		}
#pragma unroll
		for (int a = 0; a < 3; a++)
		{
#pragma unroll
			for (int o = 32; o > 0; o >>= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64)); }
			blo[a] = fminf(blo[a], lo[a]); bhi[a] = fmaxf(bhi[a], hi[a]);
		}
		if (lane == 0)
		{
#pragma unroll
			for (int a = 0; a < 3; a++) { sboxes[6 * (size_t)sb + a] = lo[a]; sboxes[6 * (size_t)sb + 3 + a] = hi[a]; }
		}
	}
	if (lane == 0)
	{
#pragma unroll
		for (int a = 0; a < 3; a++) { red[a][w] = blo[a]; red[3 + a][w] = bhi[a]; }
	}
	__syncthreads();
	if (threadIdx.x < 6 && b * FRC_BOX < nf)
	{
		const int a = threadIdx.x;
		float r = red[a][0];
		for (int k = 1; k < 4; k++) r = a < 3 ? fminf(r, red[a][k]) : fmaxf(r, red[a][k]);
		boxes[6 * (size_t)b + a] = r;
	}
}

// the super-boxes: one wave per FRC_SUPER consecutive boxes, lane l < FRC_SUPER their box l
__global__ __launch_bounds__(FRC_THREADS) void k_cloud_supers(const FrcHead* __restrict__ head, const float* __restrict__ boxes,
                                                              float* __restrict__ supers)
{
	const int nb = ((int)head->nf + FRC_BOX - 1) / FRC_BOX;
	const int sp = (int)((blockIdx.x * FRC_THREADS + threadIdx.x) >> 6), lane = threadIdx.x & 63;
	if (sp * FRC_SUPER >= nb) return;
	const int b = sp * FRC_SUPER + lane;
	float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
	if (lane < FRC_SUPER && b < nb)
	{
#pragma unroll
		for (int a = 0; a < 3; a++) { lo[a] = boxes[6 * (size_t)b + a]; hi[a] = boxes[6 * (size_t)b + 3 + a]; }
	}
#pragma unroll
	for (int a = 0; a < 3; a++)
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) { lo[a] = fminf(lo[a], __shfl_xor(lo[a], o, 64)); hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o, 64)); }
	if (lane == 0)
	{
#pragma unroll
		for (int a = 0; a < 3; a++) { supers[6 * (size_t)sp + a] = lo[a]; supers[6 * (size_t)sp + 3 + a] = hi[a]; }
	}
}

// ---- query ------------------------------------------------------------------------------------------------------------------------

struct FrcQuery
{
	int M;                            // queries ("depth": Hs * Ws)
	int H, W, stride, Hs, Ws, flip_z;
	float dist_th;
	const float* queries;
	const float* depth;
	const float* kinv;
	const float* c2w;
	const FrcHead* head;
	const uint64_t* tkeys;
	const float* sorted;
	const float* boxes;
	const float* sboxes;
	const float* supers;
	uint64_t* qkeys;
	float* dist;                      // out_dist, or the workspace's copy when only the statistics want it (null: not written)
	int32_t* out_idx;
	uint8_t* out_flag;
	float* seed_d2;                   // "points": the running squared distances of a fold, read and written by the query's own lane
	const uint8_t* mask;              // "depth": [H,W] or null
	float* out_points;                // "depth": [Hs Ws, 3] or null
	int flag_near;                    // "depth": the flag is d < dist_th instead of d > dist_th
};

__global__ __launch_bounds__(FRC_THREADS) void k_cloud_qkeys(FrcQuery p)
{
	const int i = blockIdx.x * FRC_THREADS + threadIdx.x;
	if (i >= p.M) return;
	const float x = p.queries[3 * (size_t)i], y = p.queries[3 * (size_t)i + 1], z = p.queries[3 * (size_t)i + 2];
	const uint32_t code = frc_finite3(x, y, z) ? frc_morton(x, y, z, p.head->lo, p.head->hi) : FRC_NO_CODE;
	p.qkeys[i] = ((uint64_t)code << 32) | (uint32_t)i;
}

// the query of sample (sx, sy) of the depth image: false where the pixel is masked out, has no depth or its point is not finite
__device__ __forceinline__ bool frc_depth_query(const FrcQuery& p, int sx, int sy, float* q)
{
	const int u = sx * p.stride, v = sy * p.stride;
	const size_t px = (size_t)v * p.W + u;
	const float d = p.depth[px];
	if (!frc_sample_is_query(d, p.mask != nullptr, p.mask ? p.mask[px] : (uint8_t)1)) return false;
	frc_back_project(u, v, d, p.kinv, p.c2w, p.flip_z, q);
	return frc_finite3(q[0], q[1], q[2]);
}

__device__ __forceinline__ bool frc_depth_flag(const FrcQuery& p, float d)
{
	return p.flag_near ? frc_flag_near(d, p.dist_th) : frc_flag_novel(d, p.dist_th);
}

// FOLD ("points" with seed_d2): a lane's best starts at its seed, no index is kept, and every test is strict -- a box is opened
// only when a live lane can IMPROVE there (frc_fold_may_improve), since a tie changes nothing.  A lane whose seed is not above
// its bound to the frame of all finite targets is dead from the start; a wave of dead lanes writes its outputs and leaves.
template <int DEPTH, int FOLD>
__global__ __launch_bounds__(FRC_THREADS) void k_cloud_search(FrcQuery p)
{
	static_assert(!(DEPTH && FOLD), "a fold takes its queries from points");
	const int lane = threadIdx.x & 63;
	const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (FRC_THREADS / 64) + (threadIdx.x >> 6)));
	bool inrange, ok;
	int m = 0;
	uint32_t code = 0;
	float q[3] = { 0.f, 0.f, 0.f };
	if (DEPTH)
	{
		const int tx = (p.Ws + 7) >> 3, ty = (p.Hs + 7) >> 3;
		if (wave >= tx * ty) return;
		const int sx = (wave % tx) * 8 + (lane & 7), sy = (wave / tx) * 8 + (lane >> 3);
		inrange = sx < p.Ws && sy < p.Hs;
		ok = false;
		if (inrange)
		{
			m = sy * p.Ws + sx;
			ok = frc_depth_query(p, sx, sy, q);
			if (p.out_points)
			{
				float* o = p.out_points + 3 * (size_t)m;
				o[0] = ok ? q[0] : NAN; o[1] = ok ? q[1] : NAN; o[2] = ok ? q[2] : NAN;
			}
		}
		if (ok) code = frc_morton(q[0], q[1], q[2], p.head->lo, p.head->hi);
		else q[0] = q[1] = q[2] = 0.f;
	}
	else
	{
		if (wave * 64 >= p.M) return;
		const int t = wave * 64 + lane;
		inrange = t < p.M;
		ok = false;
		if (inrange)
		{
			const uint64_t key = p.qkeys[t];
			m = (int)(uint32_t)key;
			code = (uint32_t)(key >> 32);
			ok = code != FRC_NO_CODE;
			if (ok) { q[0] = p.queries[3 * (size_t)m]; q[1] = p.queries[3 * (size_t)m + 1]; q[2] = p.queries[3 * (size_t)m + 2]; }
		}
	}
	const int nf = __builtin_amdgcn_readfirstlane((int)p.head->nf);
	float best = INFINITY;
	int32_t bidx = -1;
	bool live = ok;                   // the lane has a query; FOLD: and the query can still improve
	if (FOLD)
	{
		if (ok) best = p.seed_d2[m];
		live = ok && nf > 0 && frc_fold_may_improve(frc_box_dist2(q[0], q[1], q[2], p.head->lo, p.head->hi), best);
	}
	if (live && nf > 0)
	{
		// the lane's own place among the sorted target keys (first key of its code or beyond), and FRC_SEED targets on each side
		const uint64_t want = (uint64_t)code << 32;
		int a = 0, b = nf;
		while (a < b)
		{
			const int mid = (a + b) >> 1;
			if (p.tkeys[mid] < want) a = mid + 1; else b = mid;
		}
		const int s0 = max(0, a - FRC_SEED), s1 = min(nf - 1, a + FRC_SEED);
		for (int s = s0; s <= s1; s++)
		{
			const float d2 = frc_dist2(q[0], q[1], q[2], p.sorted[3 * (size_t)s], p.sorted[3 * (size_t)s + 1], p.sorted[3 * (size_t)s + 2]);
			if (FOLD) best = frc_fold(best, d2);
			else
			{
				const int32_t idx = (int32_t)(uint32_t)p.tkeys[s];
				if (frc_better(d2, idx, best, bidx)) { best = d2; bidx = idx; }
			}
		}
	}
	const int nb = (nf + FRC_BOX - 1) / FRC_BOX, nsb = (nf + FRC_SUB - 1) / FRC_SUB;
	const int nsp = (!FOLD || frc_any(live)) ? (nb + FRC_SUPER - 1) / FRC_SUPER : 0;          // (a fold's wave of dead lanes scans nothing)
	for (int sp = 0; sp < nsp; sp++)
	{
		const float* px = p.supers + 6 * (size_t)sp;
		const float d0 = frc_box_dist2(q[0], q[1], q[2], px, px + 3);
		// skipped only when no lane can improve OR TIE there; a fold: when no live lane can improve
		if (!frc_any(live && (FOLD ? frc_fold_may_improve(d0, best) : !(d0 > best)))) continue;
		const int b1 = min(nb, (sp + 1) * FRC_SUPER);
		for (int b = sp * FRC_SUPER; b < b1; b++)
		{
			const float* bx = p.boxes + 6 * (size_t)b;
			const float d1 = frc_box_dist2(q[0], q[1], q[2], bx, bx + 3);
			if (!frc_any(live && (FOLD ? frc_fold_may_improve(d1, best) : !(d1 > best)))) continue;
			const int sb1 = min(nsb, (b + 1) * (FRC_BOX / FRC_SUB));
			for (int sb = b * (FRC_BOX / FRC_SUB); sb < sb1; sb++)
			{
				const float* sx = p.sboxes + 6 * (size_t)sb;
				const float d2b = frc_box_dist2(q[0], q[1], q[2], sx, sx + 3);
				if (!frc_any(live && (FOLD ? frc_fold_may_improve(d2b, best) : !(d2b > best)))) continue;
				const int end = min(nf, (sb + 1) * FRC_SUB);
				for (int s = sb * FRC_SUB; s < end; s++)
				{
					const float d2 = frc_dist2(q[0], q[1], q[2], p.sorted[3 * (size_t)s], p.sorted[3 * (size_t)s + 1], p.sorted[3 * (size_t)s + 2]);
					if (FOLD) best = frc_fold(best, d2);
					else
					{
						const int32_t idx = (int32_t)(uint32_t)p.tkeys[s];
						if (frc_better(d2, idx, best, bidx)) { best = d2; bidx = idx; }
					}
				}
			}
		}
	}
	if (!inrange) return;
	if (FOLD)
	{
		// the query's own lane is the only one that touches its seed: no atomics; a query that is not finite leaves it alone
		if (ok) p.seed_d2[m] = best;
		const float d = ok ? frc_distance(best) : INFINITY;
		if (p.dist) p.dist[m] = d;
		if (p.out_flag) p.out_flag[m] = (uint8_t)(ok && frc_flag_near(d, p.dist_th));
		return;
	}
	const bool found = ok && bidx >= 0;
	const float d = found ? frc_distance(best) : INFINITY;
	if (p.dist) p.dist[m] = d;
	if (p.out_idx) p.out_idx[m] = found ? bidx : -1;
	if (p.out_flag) p.out_flag[m] = (uint8_t)(ok && (DEPTH ? frc_depth_flag(p, d) : frc_flag_near(d, p.dist_th)));
}

struct FrcPartial { double sum; unsigned long long valid, flagged, skipped; };

// the partial of each FRC_BLOCK consecutive queries in CALLER order (frc_sum_block): a query that was skipped adds +0.0
template <int DEPTH>
__global__ __launch_bounds__(FRC_THREADS) void k_cloud_partials(FrcQuery p, int nblk, FrcPartial* __restrict__ partials)
{
	__shared__ double s_sum[4];
	__shared__ uint32_t s_cnt[3][4];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x)
	{
		const int m = blk * FRC_BLOCK + (int)threadIdx.x;
		bool inrange = m < p.M, ok = false;
		if (inrange)
		{
			if (DEPTH)
			{
				float q[3];
				ok = frc_depth_query(p, m % p.Ws, m / p.Ws, q);
			}
			else ok = frc_finite3(p.queries[3 * (size_t)m], p.queries[3 * (size_t)m + 1], p.queries[3 * (size_t)m + 2]);
		}
		const float d = ok ? p.dist[m] : 0.0f;
		const bool flag = ok && (DEPTH ? frc_depth_flag(p, d) : frc_flag_near(d, p.dist_th));
		double v = ok ? (double)d : 0.0;
#pragma unroll
		for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
		const uint32_t c_ok = (uint32_t)__popcll(__ballot(ok)), c_flag = (uint32_t)__popcll(__ballot(flag));
		const uint32_t c_skip = (uint32_t)__popcll(__ballot(inrange && !ok));
		if (lane == 0) { s_sum[w] = v; s_cnt[0][w] = c_ok; s_cnt[1][w] = c_flag; s_cnt[2][w] = c_skip; }
		__syncthreads();
		if (threadIdx.x == 0)
		{
			FrcPartial r;
			r.sum = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
			r.valid = s_cnt[0][0] + s_cnt[0][1] + s_cnt[0][2] + s_cnt[0][3];
			r.flagged = s_cnt[1][0] + s_cnt[1][1] + s_cnt[1][2] + s_cnt[1][3];
			r.skipped = s_cnt[2][0] + s_cnt[2][1] + s_cnt[2][2] + s_cnt[2][3];
			partials[blk] = r;
		}
		__syncthreads();
	}
}

// one workgroup: slot t = +0.0 + p[t] + p[t + FRC_BLOCK] + ..., then the block sum over the slots; the counts are integers
__global__ __launch_bounds__(FRC_THREADS) void k_cloud_total(int nblk, const FrcPartial* __restrict__ partials, unsigned long long* __restrict__ out_stats)
{
	__shared__ double s_sum[4];
	__shared__ unsigned long long s_cnt[3][4];
	const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
	double v = 0.0;
	unsigned long long c[3] = { 0ull, 0ull, 0ull };
	for (int j = threadIdx.x; j < nblk; j += FRC_THREADS)
	{
		v = v + partials[j].sum;
		c[0] += partials[j].valid; c[1] += partials[j].flagged; c[2] += partials[j].skipped;
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
	{
		v = v + __shfl_xor(v, o, 64);
#pragma unroll
		for (int k = 0; k < 3; k++) c[k] += __shfl_xor(c[k], o, 64);
	}
	if (lane == 0) { s_sum[w] = v; for (int k = 0; k < 3; k++) s_cnt[k][w] = c[k]; }
	__syncthreads();
	if (threadIdx.x == 0)
	{
		const double total = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
		out_stats[0] = (unsigned long long)__double_as_longlong(total);
		for (int k = 0; k < 3; k++) out_stats[1 + k] = s_cnt[k][0] + s_cnt[k][1] + s_cnt[k][2] + s_cnt[k][3];
	}
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------


extern "C" size_t fr_cloud_index_bytes(int32_t N)
{
	if (N < 0 || N > FR_CLOUD_MAX_POINTS) return 0;
	return frc_index_layout(N).total;
}

extern "C" size_t fr_cloud_index_workspace_bytes(int32_t N)
{
	if (N < 0 || N > FR_CLOUD_MAX_POINTS) return 0;
	return 256;                                                // the build's accumulators: the sort works in place in the index
}

extern "C" size_t fr_cloud_query_workspace_bytes(int32_t M)
{
	if (M < 0 || M > FR_CLOUD_MAX_POINTS) return 0;
	return frc_query_layout(M).total;
}

extern "C" int fr_cloud_index_build(int32_t N, const float* points, void* index, size_t index_bytes, void* workspace, size_t workspace_bytes,
                                    fr_stream_t stream)
{
	if (N < 0 || N > FR_CLOUD_MAX_POINTS) return fr_fail(FR_EINVAL, "fr_cloud_index_build: N outside [0, FR_CLOUD_MAX_POINTS]");
	if (!index || !workspace || (N > 0 && !points)) return fr_fail(FR_EINVAL, "fr_cloud_index_build: null pointer");
	if (!fr_aligned(points, 4) || !fr_aligned(index, 8) || !fr_aligned(workspace, 8))
		return fr_fail(FR_EINVAL, "fr_cloud_index_build: misaligned pointer (points 4, index and workspace 8 bytes)");
	const FrcIndexLayout L = frc_index_layout(N);
	if (index_bytes < L.total) return fr_fail(FR_EINVAL, "fr_cloud_index_build: index smaller than fr_cloud_index_bytes()");
	if (workspace_bytes < fr_cloud_index_workspace_bytes(N)) return fr_fail(FR_EINVAL, "fr_cloud_index_build: workspace smaller than fr_cloud_index_workspace_bytes()");
	hipStream_t s = (hipStream_t)stream;
	char* ix = (char*)index;
	uint32_t* acc = (uint32_t*)workspace;
	FrcHead* head = (FrcHead*)(ix + L.head);
	uint64_t* keys = (uint64_t*)(ix + L.keys);
	float* sorted = (float*)(ix + L.sorted);
	int rc;
	(void)hipMemsetAsync(acc, 0xFF, 12, s);
	(void)hipMemsetAsync(acc + 3, 0x00, 20, s);
	if (N > 0)
	{
		const int nblk = (N + FRC_THREADS - 1) / FRC_THREADS;
		hipLaunchKernelGGL(k_cloud_minmax, dim3(nblk < FRC_MAX_GRID ? nblk : FRC_MAX_GRID), dim3(FRC_THREADS), 0, s, N, points, acc);
		if ((rc = fr_check_launch("k_cloud_minmax"))) return rc;
		hipLaunchKernelGGL(k_cloud_head, dim3(1), dim3(64), 0, s, (const uint32_t*)acc, head);
		hipLaunchKernelGGL(k_cloud_tkeys, dim3(nblk), dim3(FRC_THREADS), 0, s, N, points, (const uint32_t*)acc, keys);
		if ((rc = fr_check_launch("k_cloud_tkeys"))) return rc;
		if ((rc = fr_sort_keys64(keys, (uint32_t)N, stream))) return rc;
		hipLaunchKernelGGL(k_cloud_gather, dim3(nblk), dim3(FRC_THREADS), 0, s, N, points, (const uint64_t*)keys, sorted);
		if ((rc = fr_check_launch("k_cloud_gather"))) return rc;
		hipLaunchKernelGGL(k_cloud_boxes, dim3((N + FRC_BOX - 1) / FRC_BOX), dim3(FRC_THREADS), 0, s, (const FrcHead*)head, (const float*)sorted,
		                   (float*)(ix + L.boxes), (float*)(ix + L.sboxes));
		if ((rc = fr_check_launch("k_cloud_boxes"))) return rc;
		const int nsp = (N + FRC_SUPER * FRC_BOX - 1) / (FRC_SUPER * FRC_BOX);
		hipLaunchKernelGGL(k_cloud_supers, dim3((nsp * 64 + FRC_THREADS - 1) / FRC_THREADS), dim3(FRC_THREADS), 0, s, (const FrcHead*)head,
		                   (const float*)(ix + L.boxes), (float*)(ix + L.supers));
		return fr_check_launch("k_cloud_supers");
	}
	hipLaunchKernelGGL(k_cloud_head, dim3(1), dim3(64), 0, s, (const uint32_t*)acc, head);
	return fr_check_launch("k_cloud_head");
}

extern "C" int fr_cloud_query(const void* index, size_t index_bytes, int32_t N, const fr_cloud_query_cfg* cfg, void* workspace,
                              size_t workspace_bytes, fr_stream_t stream)
{
	if (N < 0 || N > FR_CLOUD_MAX_POINTS) return fr_fail(FR_EINVAL, "fr_cloud_query: N outside [0, FR_CLOUD_MAX_POINTS]");
	if (!index || !cfg || !workspace) return fr_fail(FR_EINVAL, "fr_cloud_query: null pointer");
	const FrcIndexLayout L = frc_index_layout(N);
	if (index_bytes < L.total) return fr_fail(FR_EINVAL, "fr_cloud_query: index smaller than fr_cloud_index_bytes()");
	const bool depth = cfg->source == FR_CLOUD_SOURCE_DEPTH;
	if (!depth && cfg->source != FR_CLOUD_SOURCE_POINTS) return fr_fail(FR_EINVAL, "fr_cloud_query: source is neither FR_CLOUD_SOURCE_POINTS nor FR_CLOUD_SOURCE_DEPTH");
	FrcQuery p = {};
	int64_t M;
	if (depth)
	{
		if (cfg->H <= 0 || cfg->W <= 0 || cfg->stride <= 0) return fr_fail(FR_EINVAL, "fr_cloud_query: H, W and stride must be positive");
		if ((int64_t)cfg->H * cfg->W > FR_CLOUD_MAX_POINTS) return fr_fail(FR_EINVAL, "fr_cloud_query: H W beyond FR_CLOUD_MAX_POINTS");
		if (!cfg->depth || !cfg->kinv || !cfg->c2w) return fr_fail(FR_EINVAL, "fr_cloud_query: null depth, kinv or c2w");
		if (!fr_aligned(cfg->depth, 4) || !fr_aligned(cfg->kinv, 4) || !fr_aligned(cfg->c2w, 4))
			return fr_fail(FR_EINVAL, "fr_cloud_query: misaligned depth, kinv or c2w");
		p.H = cfg->H; p.W = cfg->W; p.stride = cfg->stride; p.flip_z = cfg->flip_z != 0;
		p.Hs = (cfg->H + cfg->stride - 1) / cfg->stride; p.Ws = (cfg->W + cfg->stride - 1) / cfg->stride;
		M = (int64_t)p.Hs * p.Ws;
		if (cfg->seed_d2) return fr_fail(FR_EINVAL, "fr_cloud_query: seed_d2 goes with FR_CLOUD_SOURCE_POINTS only");
		if (!fr_aligned(cfg->out_points, 4)) return fr_fail(FR_EINVAL, "fr_cloud_query: misaligned out_points (4 bytes)");
		p.mask = cfg->mask; p.out_points = cfg->out_points; p.flag_near = cfg->flag_near != 0;
	}
	else
	{
		M = cfg->M;
		if (M < 0 || M > FR_CLOUD_MAX_POINTS) return fr_fail(FR_EINVAL, "fr_cloud_query: M outside [0, FR_CLOUD_MAX_POINTS]");
		if (M > 0 && !cfg->queries) return fr_fail(FR_EINVAL, "fr_cloud_query: null queries");
		if (!fr_aligned(cfg->queries, 4)) return fr_fail(FR_EINVAL, "fr_cloud_query: misaligned queries");
		if (cfg->mask || cfg->out_points) return fr_fail(FR_EINVAL, "fr_cloud_query: mask and out_points go with FR_CLOUD_SOURCE_DEPTH only");
		if (cfg->seed_d2 && cfg->out_idx) return fr_fail(FR_EINVAL, "fr_cloud_query: out_idx must be null with seed_d2 (the union it would index is gone)");
		if (!fr_aligned(cfg->seed_d2, 4)) return fr_fail(FR_EINVAL, "fr_cloud_query: misaligned seed_d2 (4 bytes)");
		p.seed_d2 = cfg->seed_d2;
	}
	if (!fr_aligned(index, 8) || !fr_aligned(workspace, 8) || !fr_aligned(cfg->out_dist, 4) || !fr_aligned(cfg->out_idx, 4) ||
	    !fr_aligned(cfg->out_stats, 8))
		return fr_fail(FR_EINVAL, "fr_cloud_query: misaligned pointer (index, workspace and out_stats 8, out_dist and out_idx 4 bytes)");
	const FrcQueryLayout Q = frc_query_layout(M);
	if (workspace_bytes < Q.total) return fr_fail(FR_EINVAL, "fr_cloud_query: workspace smaller than fr_cloud_query_workspace_bytes()");
	hipStream_t s = (hipStream_t)stream;
	const char* ix = (const char*)index;
	char* ws = (char*)workspace;
	p.M = (int)M;
	p.dist_th = cfg->dist_th;
	p.queries = cfg->queries; p.depth = cfg->depth; p.kinv = cfg->kinv; p.c2w = cfg->c2w;
	p.head = (const FrcHead*)(ix + L.head);
	p.tkeys = (const uint64_t*)(ix + L.keys);
	p.sorted = (const float*)(ix + L.sorted);
	p.boxes = (const float*)(ix + L.boxes);
	p.sboxes = (const float*)(ix + L.sboxes);
	p.supers = (const float*)(ix + L.supers);
	p.qkeys = (uint64_t*)(ws + Q.qkeys);
	p.dist = cfg->out_dist ? cfg->out_dist : (cfg->out_stats ? (float*)(ws + Q.dist) : nullptr);
	p.out_idx = cfg->out_idx; p.out_flag = cfg->out_flag;
	int rc;
	if (M > 0 && (p.dist || p.out_idx || p.out_flag || p.seed_d2 || p.out_points))
	{
		if (depth)
		{
			const int waves = ((p.Ws + 7) / 8) * ((p.Hs + 7) / 8);
			hipLaunchKernelGGL((k_cloud_search<1, 0>), dim3((waves + 3) / 4), dim3(FRC_THREADS), 0, s, p);
		}
		else
		{
			const int nblk = (int)((M + FRC_THREADS - 1) / FRC_THREADS);
			hipLaunchKernelGGL(k_cloud_qkeys, dim3(nblk), dim3(FRC_THREADS), 0, s, p);
			if ((rc = fr_check_launch("k_cloud_qkeys"))) return rc;
			if ((rc = fr_sort_keys64(p.qkeys, (uint32_t)M, stream))) return rc;
			if (p.seed_d2) hipLaunchKernelGGL((k_cloud_search<0, 1>), dim3(nblk), dim3(FRC_THREADS), 0, s, p);
			else hipLaunchKernelGGL((k_cloud_search<0, 0>), dim3(nblk), dim3(FRC_THREADS), 0, s, p);
		}
		if ((rc = fr_check_launch("k_cloud_search"))) return rc;
	}
	if (cfg->out_stats)
	{
		const int nblk = (int)frc_blocks(M);
		FrcPartial* partials = (FrcPartial*)(ws + Q.partials);
		if (nblk > 0)
		{
			const int grid = nblk < FRC_MAX_GRID ? nblk : FRC_MAX_GRID;
			if (depth) hipLaunchKernelGGL(k_cloud_partials<1>, dim3(grid), dim3(FRC_THREADS), 0, s, p, nblk, partials);
			else hipLaunchKernelGGL(k_cloud_partials<0>, dim3(grid), dim3(FRC_THREADS), 0, s, p, nblk, partials);
			if ((rc = fr_check_launch("k_cloud_partials"))) return rc;
		}
		hipLaunchKernelGGL(k_cloud_total, dim3(1), dim3(FRC_THREADS), 0, s, nblk, (const FrcPartial*)partials, (unsigned long long*)cfg->out_stats);
		return fr_check_launch("k_cloud_total");
	}
	return FR_OK;
}
