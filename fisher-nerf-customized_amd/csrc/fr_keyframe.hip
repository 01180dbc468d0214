// fr_keyframe.hip -- the keyframe overlap of libfisher_rast.so (gfx950, wave64): fr_keyframe_valid_pixels / fr_keyframe_overlap.
//
// The reference picks the mapping window with a torch chain (models/SLAM/utils/keyframe_selection.py:10-37, 40-134): a torch.where
// and a unique() over the drawn points (a host synchronisation each), a torch.inverse, about fifteen small launches per keyframe in
// a Python loop, and a Python sort over 0-dim device tensors.  Here, whatever the number of keyframes:
//
//   k_kf_count                one thread per pixel: depth > 0 (& mask != 0), counted per workgroup by ballot / popcount.
//   k_kf_scan                 one workgroup: exclusive scan of the per-workgroup counts, the total into status[0].
//   k_kf_scatter              same geometry as k_kf_count: pixel p goes to slot offset[workgroup] + waves before + lanes before, so the
//                             list ascends -- the order torch.where gives.
//   k_kf_points               one thread per drawn point: the pixel behind the draw (range-checked, never read through when out of
//                             range), its back-projection (c2w is inverted from w2c once per workgroup) and its three keys.
//   k_kf_pairs                one thread per drawn point against every other, the keys tiled through LDS 256 at a time: invalid when
//                             another point or (0,0,0) has the same keys.  Per-workgroup counts of the valid points and of the
//                             out-of-range draws by ballot / popcount.  No atomics, no sort.
//   k_kf_status               one wave: the per-workgroup counts (at most FR_KEYFRAME_MAX_POINTS / 256 of them) added in order.
//   k_kf_overlap              grid (point chunk, keyframe; grid-stride over the keyframes): projection of every valid point into the
//                             keyframe, the keyframe's mask where it has one, valid & inside counted by ballot / popcount and
//                             added to out_counts[k] with one integer atomic per workgroup.
//
// Workgroups never wait for each other: what one launch hands to the next goes through the kernel boundary.  The ballot count / rank
// of k_kf_count / k_kf_scatter and the scan of the counts are the workgroup primitives of fr_block.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "fr_internal.h"
#include "fr_block.h"
#include "fr_keyframe_math.h"

#define FRK_THREADS 256
static_assert(FRK_THREADS == FRB_THREADS, "fr_block.h is written for 256 threads");
#define FRK_CHUNK_ITEMS 4                                  // points per thread of an overlap workgroup
#define FRK_MAX_WG (FR_KEYFRAME_MAX_POINTS / FRK_THREADS)  // workgroups of k_kf_points / k_kf_pairs at the most
#define FRK_NAN_BITS 0x7fc00000u                           // the keys of an out-of-range draw: a NaN equals nothing
#define FRK_FLAG_VALID 1
#define FRK_FLAG_OUT_OF_RANGE 2                            // left by k_kf_points for k_kf_pairs, which overwrites it

__device__ __forceinline__ bool frk_pixel_valid(const float* __restrict__ depth, const uint8_t* __restrict__ mask, uint32_t p, uint32_t n)
{
	return p < n && depth[p] > 0.0f && (!mask || mask[p] != 0);
}

__global__ __launch_bounds__(FRK_THREADS) void k_kf_count(const float* __restrict__ depth, const uint8_t* __restrict__ mask, uint32_t n,
                                                          uint32_t* __restrict__ counts)
{
	__shared__ uint32_t s_wave[4];
	const bool sel = frk_pixel_valid(depth, mask, blockIdx.x * (uint32_t)FRK_THREADS + threadIdx.x, n);
	const uint32_t count = frb_count256(sel, s_wave);
	if (threadIdx.x == 0) counts[blockIdx.x] = count;
}

__global__ __launch_bounds__(FRK_THREADS) void k_kf_scan(const uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets, int nwg,
                                                         int32_t* __restrict__ status)
{
	__shared__ uint32_t s_wave[4];
	const uint32_t total = frb_scan_counts(counts, offsets, nwg, s_wave);
	if (threadIdx.x == 0) { status[0] = (int32_t)total; status[1] = 0; status[2] = 0; status[3] = 0; }
}

__global__ __launch_bounds__(FRK_THREADS) void k_kf_scatter(const float* __restrict__ depth, const uint8_t* __restrict__ mask, uint32_t n,
                                                            const uint32_t* __restrict__ offsets, int32_t* __restrict__ idx)
{
	__shared__ uint32_t s_wave[4];
	const uint32_t p = blockIdx.x * (uint32_t)FRK_THREADS + threadIdx.x;
	const bool sel = frk_pixel_valid(depth, mask, p, n);
	const uint32_t before = frb_rank256(sel, s_wave);        // (a barrier: in front of the return)
	if (!sel) return;
	const uint32_t slot = offsets[blockIdx.x] + before;
	if (slot < n) idx[slot] = (int32_t)p;                  // always: at most n pixels are selected
}

struct FrkArgs {
	const float* depth;          // [H,W]
	const int32_t* valid_idx;    // [n_valid_idx], or null: a draw is a pixel
	const int64_t* draws;        // [n]
	const float* intr;           // [3,3]
	const float* w2c;            // [4,4]
	const float* kf_w2c;         // [K,16]
	const uint64_t* masks;       // [K] addresses of byte masks [H,W], or null
	int H, W, n, K, edge;
	int64_t limit;               // draws are valid below this
	int64_t hw;
	float* pts;                  // workspace [n,3]
	float* keys;                 // workspace [n,3]
	uint8_t* flags;              // workspace [n]: FRK_FLAG_*
	uint32_t* wg_counts;         // workspace [2][FRK_MAX_WG]: valid points, out-of-range draws per workgroup of k_kf_pairs
	int32_t* out_counts;
	uint8_t* out_valid;
	float* out_pts;
	int32_t* status;
};

__global__ __launch_bounds__(FRK_THREADS) void k_kf_points(FrkArgs a)
{
	__shared__ float s_m[12], s_k[4];
	const int tid = threadIdx.x;
	if (tid == 0)
	{
		fri_invert_affine(a.w2c, s_m);
		s_k[0] = a.intr[0]; s_k[1] = a.intr[4]; s_k[2] = a.intr[2]; s_k[3] = a.intr[5];
	}
	__syncthreads();
	const int i = blockIdx.x * FRK_THREADS + tid;
	if (i >= a.n) return;
	const int64_t d = a.draws[i];
	int64_t pix = -1;
	if (d >= 0 && d < a.limit) pix = a.valid_idx ? (int64_t)a.valid_idx[d] : d;
	float p[3] = {0.0f, 0.0f, 0.0f}, k[3];
	const bool in_range = pix >= 0 && pix < a.hw;
	a.flags[i] = in_range ? 0 : FRK_FLAG_OUT_OF_RANGE;
	if (in_range)
	{
		const int y = (int)(pix / a.W), x = (int)(pix - (int64_t)y * a.W);
		fri_back_project(x, y, a.depth[pix], s_k[0], s_k[1], s_k[2], s_k[3], s_m, p);
		frk_keys(p, k);
	}
	else
		k[0] = k[1] = k[2] = fri_float(FRK_NAN_BITS);
	for (int c = 0; c < 3; c++)
	{
		a.pts[3 * i + c] = p[c];
		a.keys[3 * i + c] = k[c];
		if (a.out_pts) a.out_pts[3 * i + c] = p[c];
	}
}

__global__ __launch_bounds__(FRK_THREADS) void k_kf_pairs(FrkArgs a)
{
	__shared__ float s_keys[3 * FRK_THREADS];
	__shared__ uint32_t s_wave[8];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int i = blockIdx.x * FRK_THREADS + tid;
	float k[3] = {0.0f, 0.0f, 0.0f};
	if (i < a.n) { k[0] = a.keys[3 * i]; k[1] = a.keys[3 * i + 1]; k[2] = a.keys[3 * i + 2]; }
	const bool oor = i < a.n && a.flags[i] == FRK_FLAG_OUT_OF_RANGE;
	bool dup = frk_origin_key(k);
	for (int base = 0; base < a.n; base += FRK_THREADS)
	{
		const int j = base + tid;
		__syncthreads();
		for (int c = 0; c < 3; c++) s_keys[3 * tid + c] = j < a.n ? a.keys[3 * j + c] : fri_float(FRK_NAN_BITS);
		__syncthreads();
		const int m = min(FRK_THREADS, a.n - base);
		for (int t = 0; t < m; t++)
			if (base + t != i) dup |= frk_same_key(k, &s_keys[3 * t]);
	}
	const bool valid = i < a.n && !oor && !dup;
	if (i < a.n)
	{
		a.flags[i] = valid ? FRK_FLAG_VALID : 0;
		if (a.out_valid) a.out_valid[i] = valid ? 1 : 0;
	}
	const unsigned long long bv = __ballot(valid), bo = __ballot(oor);
	if (lane == 0) { s_wave[wave] = (uint32_t)__popcll(bv); s_wave[4 + wave] = (uint32_t)__popcll(bo); }
	__syncthreads();
	if (tid == 0)
	{
		a.wg_counts[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
		a.wg_counts[FRK_MAX_WG + blockIdx.x] = ((s_wave[4] + s_wave[5]) + s_wave[6]) + s_wave[7];
	}
}

__global__ __launch_bounds__(64) void k_kf_status(const uint32_t* __restrict__ wg_counts, int nwg, int32_t* __restrict__ status)
{
	if (threadIdx.x != 0) return;
	uint32_t v = 0u, o = 0u;
	for (int w = 0; w < nwg; w++) { v += wg_counts[w]; o += wg_counts[FRK_MAX_WG + w]; }
	status[0] = (int32_t)v; status[1] = (int32_t)o; status[2] = 0; status[3] = 0;
}

__global__ __launch_bounds__(FRK_THREADS) void k_kf_overlap(FrkArgs a)
{
	__shared__ float s_w[12], s_k[9];
	__shared__ uint32_t s_wave[4];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	if (tid < 9) s_k[tid] = a.intr[tid];
	// this workgroup's points stay in registers over the keyframes
	float p[FRK_CHUNK_ITEMS][3];
	bool ok[FRK_CHUNK_ITEMS];
#pragma unroll
	for (int q = 0; q < FRK_CHUNK_ITEMS; q++)
	{
		const int i = (blockIdx.x * FRK_CHUNK_ITEMS + q) * FRK_THREADS + tid;
		ok[q] = i < a.n && a.flags[i] == FRK_FLAG_VALID;
		for (int c = 0; c < 3; c++) p[q][c] = ok[q] ? a.pts[3 * i + c] : 0.0f;
	}
	for (int kf = blockIdx.y; kf < a.K; kf += gridDim.y)
	{
		__syncthreads();
		if (tid < 12) s_w[tid] = a.kf_w2c[(size_t)kf * 16 + tid];
		__syncthreads();
		const uint8_t* mask = a.masks ? (const uint8_t*)(uintptr_t)a.masks[kf] : nullptr;
		uint32_t mine = 0u;
#pragma unroll
		for (int q = 0; q < FRK_CHUNK_ITEMS; q++)
		{
			bool in = false;
			if (ok[q])
			{
				float u, v;
				in = frk_project_inside(s_w, s_k, p[q], a.H, a.W, a.edge, &u, &v);
				if (in && mask) in = frk_mask_hit(mask, a.H, a.W, u, v);
			}
			mine += (uint32_t)__popcll(__ballot(in));        // the same number in every lane of the wave
		}
		if (lane == 0) s_wave[wave] = mine;
		__syncthreads();
		if (tid == 0)
		{
			const uint32_t total = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
			if (total) atomicAdd(&a.out_counts[kf], (int32_t)total);
		}
	}
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

static int frk_pixel_wgs(int32_t H, int32_t W) { return (int)(((int64_t)H * W + FRK_THREADS - 1) / FRK_THREADS); }

extern "C" size_t fr_keyframe_valid_pixels_workspace_bytes(int32_t H, int32_t W)
{
	if (!fr_image_ok(H, W)) return 0;
	return 2 * (size_t)frk_pixel_wgs(H, W) * sizeof(uint32_t);
}

struct FrkLayout { size_t pts, keys, counts, flags, total; };

static FrkLayout frk_layout(int32_t n)
{
	FrkLayout l;
	l.pts = 0;
	l.keys = l.pts + (size_t)n * 3 * sizeof(float);
	l.counts = l.keys + (size_t)n * 3 * sizeof(float);
	l.flags = l.counts + 2 * (size_t)FRK_MAX_WG * sizeof(uint32_t);
	l.total = (l.flags + (size_t)n + 15) & ~(size_t)15;
	return l;
}

extern "C" size_t fr_keyframe_overlap_workspace_bytes(int32_t n)
{
	if (n < 1 || n > FR_KEYFRAME_MAX_POINTS) return 0;
	return frk_layout(n).total;
}

extern "C" int fr_keyframe_valid_pixels(int32_t H, int32_t W, const float* depth, const uint8_t* mask, int32_t* idx_out, int32_t* status,
                                        void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	if (!fr_image_ok(H, W)) return fr_fail(FR_EINVAL, "fr_keyframe_valid_pixels: bad argument (H, W; H W at most 2^30)");
	if (!depth || !idx_out || !status) return fr_fail(FR_EINVAL, "fr_keyframe_valid_pixels: null pointer (depth, idx_out, status)");
	if ((uintptr_t)depth % 4 || (uintptr_t)idx_out % 4 || (uintptr_t)status % 4)
		return fr_fail(FR_EINVAL, "fr_keyframe_valid_pixels: bad argument (depth, idx_out, status must be 4-byte aligned)");
	const int nwg = frk_pixel_wgs(H, W);
	if (!workspace || workspace_bytes < 2 * (size_t)nwg * sizeof(uint32_t))
		return fr_fail(FR_EINVAL, "fr_keyframe_valid_pixels: workspace too small (fr_keyframe_valid_pixels_workspace_bytes)");
	if ((uintptr_t)workspace % 8) return fr_fail(FR_EINVAL, "fr_keyframe_valid_pixels: bad argument (workspace must be 8-byte aligned)");
	uint32_t* counts = (uint32_t*)workspace;
	uint32_t* offsets = counts + nwg;
	const uint32_t n = (uint32_t)((int64_t)H * W);
	hipStream_t s = (hipStream_t)stream;
	const dim3 block(FRK_THREADS), grid(nwg);
	int rc;
	hipLaunchKernelGGL(k_kf_count, grid, block, 0, s, depth, mask, n, counts);
	if ((rc = fr_check_launch("k_kf_count"))) return rc;
	hipLaunchKernelGGL(k_kf_scan, dim3(1), block, 0, s, (const uint32_t*)counts, offsets, nwg, status);
	if ((rc = fr_check_launch("k_kf_scan"))) return rc;
	hipLaunchKernelGGL(k_kf_scatter, grid, block, 0, s, depth, mask, n, (const uint32_t*)offsets, idx_out);
	return fr_check_launch("k_kf_scatter");
}

extern "C" int fr_keyframe_overlap(const fr_keyframe_cfg* cfg, const float* depth, const int32_t* valid_idx, const int64_t* draws,
                                   const float* kf_w2c, const uint64_t* kf_mask_table, int32_t* out_counts, uint8_t* out_valid, float* out_pts,
                                   int32_t* status, void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	if (!cfg) return fr_fail(FR_EINVAL, "fr_keyframe_overlap: null cfg");
	if (!fr_image_ok(cfg->H, cfg->W)) return fr_fail(FR_EINVAL, "fr_keyframe_overlap: bad argument (cfg: H, W; H W at most 2^30)");
	if (cfg->n < 1 || cfg->n > FR_KEYFRAME_MAX_POINTS) return fr_fail(FR_EINVAL, "fr_keyframe_overlap: bad argument (cfg->n is 1 .. FR_KEYFRAME_MAX_POINTS)");
	if (cfg->K < 0 || cfg->edge < 0) return fr_fail(FR_EINVAL, "fr_keyframe_overlap: bad argument (cfg: K, edge must not be negative)");
	if (valid_idx && cfg->n_valid_idx < 0) return fr_fail(FR_EINVAL, "fr_keyframe_overlap: bad argument (cfg->n_valid_idx)");
	if (!depth || !draws || !status || !cfg->intrinsics || !cfg->w2c)
		return fr_fail(FR_EINVAL, "fr_keyframe_overlap: null pointer (depth, draws, status, cfg->intrinsics, cfg->w2c)");
	if (cfg->K > 0 && (!kf_w2c || !out_counts)) return fr_fail(FR_EINVAL, "fr_keyframe_overlap: null pointer (kf_w2c, out_counts with K > 0)");
	if ((uintptr_t)depth % 4 || (uintptr_t)cfg->intrinsics % 4 || (uintptr_t)cfg->w2c % 4 || (uintptr_t)kf_w2c % 4 || (uintptr_t)out_pts % 4 ||
	    (uintptr_t)valid_idx % 4 || (uintptr_t)out_counts % 4 || (uintptr_t)status % 4)
		return fr_fail(FR_EINVAL, "fr_keyframe_overlap: bad argument (float and int32 pointers must be 4-byte aligned)");
	if ((uintptr_t)draws % 8 || (uintptr_t)kf_mask_table % 8)
		return fr_fail(FR_EINVAL, "fr_keyframe_overlap: bad argument (draws and kf_mask_table must be 8-byte aligned)");
	const FrkLayout l = frk_layout(cfg->n);
	if (!workspace || workspace_bytes < l.total) return fr_fail(FR_EINVAL, "fr_keyframe_overlap: workspace too small (fr_keyframe_overlap_workspace_bytes)");
	if ((uintptr_t)workspace % 8) return fr_fail(FR_EINVAL, "fr_keyframe_overlap: bad argument (workspace must be 8-byte aligned)");

	char* ws = (char*)workspace;
	FrkArgs a;
	a.depth = depth; a.valid_idx = valid_idx; a.draws = draws; a.intr = cfg->intrinsics; a.w2c = cfg->w2c;
	a.kf_w2c = kf_w2c; a.masks = kf_mask_table;
	a.H = cfg->H; a.W = cfg->W; a.n = cfg->n; a.K = cfg->K; a.edge = cfg->edge;
	a.hw = (int64_t)cfg->H * cfg->W;
	a.limit = valid_idx ? (int64_t)cfg->n_valid_idx : a.hw;
	a.pts = (float*)(ws + l.pts); a.keys = (float*)(ws + l.keys); a.flags = (uint8_t*)(ws + l.flags);
	a.wg_counts = (uint32_t*)(ws + l.counts);
	a.out_counts = out_counts; a.out_valid = out_valid; a.out_pts = out_pts; a.status = status;
	hipStream_t s = (hipStream_t)stream;
	const dim3 block(FRK_THREADS);
	const int nwg = (cfg->n + FRK_THREADS - 1) / FRK_THREADS;
	int rc;
	hipLaunchKernelGGL(k_kf_points, dim3(nwg), block, 0, s, a);
	if ((rc = fr_check_launch("k_kf_points"))) return rc;
	hipLaunchKernelGGL(k_kf_pairs, dim3(nwg), block, 0, s, a);
	if ((rc = fr_check_launch("k_kf_pairs"))) return rc;
	hipLaunchKernelGGL(k_kf_status, dim3(1), dim3(64), 0, s, (const uint32_t*)a.wg_counts, nwg, status);
	if ((rc = fr_check_launch("k_kf_status"))) return rc;
	if (cfg->K == 0) return FR_OK;
	if (hipMemsetAsync(out_counts, 0, (size_t)cfg->K * sizeof(int32_t), s) != hipSuccess) return fr_fail(FR_ELAUNCH, "fr_keyframe_overlap: hipMemsetAsync failed");
	const int per = FRK_THREADS * FRK_CHUNK_ITEMS;
	const dim3 grid((cfg->n + per - 1) / per, cfg->K < 4096 ? cfg->K : 4096);
	hipLaunchKernelGGL(k_kf_overlap, grid, block, 0, s, a);
	return fr_check_launch("k_kf_overlap");
}
