// fr_ingest.hip -- the frame ingest of libfisher_rast.so (gfx950, wave64): fr_frame_ingest_select / fr_frame_ingest_emit.
//
// The reference grows the map from an RGB-D frame with a torch chain (models/SLAM/gaussian.py:320-414 over 75-143 and 299-318): a
// full sort for the median of the depth error, a max_pool2d, two boolean indexings and a `sum() > 0` (a host synchronisation
// each), a torch.inverse and about a dozen H W sized temporaries.  Here:
//
//   k_ingest_hist<PASS> x 4   the exact lower median of the H W depth errors (element (n - 1) / 2 of the sorted values) by a radix
//                             select on the bit patterns, most significant byte first.  The errors are never negative, so unsigned
//                             order is float order.  A workgroup counts 2048 pixels into an integer LDS histogram and flushes it with
//                             integer atomics; pass p first walks the histograms of the passes before it to the prefix they fixed
//                             (every workgroup does, it is 256 numbers a pass).  Pass 0 counts the NaNs, which are left out of every
//                             histogram: one NaN makes the median NaN.  Integer sums only: no dependence on the launch geometry.
//   k_ingest_mask             walks the four histograms to the median, then one thread per cell of the H/d x W/d grid: the
//                             non-presence predicate (fr_ingest_math.h; ANDed with the caller's bytes where given: the
//                             object mask of gaussian_object.py:447-460) or the caller's byte mask alone, OR-ed over the cell's d x d pixels
//                             (max_pool2d of a 0/1 image), stored as a byte, and counted per workgroup by ballot / popcount.
//   k_ingest_scan             one workgroup: exclusive scan of the per-workgroup counts, the total into status[0].
//   k_ingest_scatter          same geometry as k_ingest_mask: cell g goes to slot offset[workgroup] + waves before + lanes before,
//                             so the list ascends -- the order boolean indexing gives.
//   k_ingest_emit             one thread per selected cell: back-projection of the cell's top-left pixel, colour bits, (1,0,0,0), 0,
//                             log scale; c2w is inverted from w2c once per workgroup.
//
// Workgroups never wait for each other: what one launch hands to the next goes through the kernel boundary.  The radix select, the
// ballot count / rank and the scan of the counts are the workgroup primitives of fr_block.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "fr_internal.h"
#include "fr_block.h"
#include "fr_ingest_math.h"

#define FRI_THREADS 256
static_assert(FRI_THREADS == FRB_THREADS, "fr_block.h is written for 256 threads");
#define FRI_HIST_ITEMS 8                                   // pixels per thread of a histogram workgroup
#define FRI_HIST_BYTES (4 * 256 * sizeof(uint32_t))       // the four histograms; the NaN count sits behind them
#define FRI_HEAD_BYTES (FRI_HIST_BYTES + 64)

struct FriArgs {
	const float* depth_sil;      // [3,H,W]: channel 0 depth, channel 1 silhouette (FR_INGEST_NONPRESENCE)
	const float* gt;             // [1,H,W]
	const uint8_t* mask_in;      // [H,W] bytes: the mask itself (FR_INGEST_MASK), or one ANDed into the predicate (FR_INGEST_NONPRESENCE; may be null)
	int H, W, d, Gw, G, mode;
	uint32_t n;                  // H W
	float sil_thres, ratio;
	uint32_t* hist;              // [4][256], then the NaN count
	uint8_t* pooled;             // [G]
	uint32_t* counts;            // [workgroups of G]
	uint32_t* offsets;
	int32_t* idx;                // [G]
	int32_t* status;
};

// the prefix that the first `passes` histograms fix for the lower median, element (n - 1) / 2 of the sorted errors
__device__ __forceinline__ uint32_t fri_prefix(const FriArgs& a, int passes, uint32_t* s_wave, uint32_t* s_out)
{
	uint32_t k = (a.n - 1u) / 2u, inside;
	return frb_select_prefix(a.hist, passes, k, inside, s_wave, s_out);
}

template <int PASS>
__global__ __launch_bounds__(FRI_THREADS) void k_ingest_hist(FriArgs a)
{
	__shared__ uint32_t s_hist[256], s_wave[4], s_out[3];
	const int tid = threadIdx.x;
	s_hist[tid] = 0u;
	const uint32_t prefix = fri_prefix(a, PASS, s_wave, s_out);
	__syncthreads();
	uint32_t nans = 0u;
	const uint32_t base = blockIdx.x * (uint32_t)(FRI_THREADS * FRI_HIST_ITEMS);
#pragma unroll
	for (int i = 0; i < FRI_HIST_ITEMS; i++)
	{
		const uint32_t p = base + (uint32_t)(i * FRI_THREADS + tid);
		if (p >= a.n) continue;
		const float e = fri_depth_error(a.gt[p], a.depth_sil[p]);
		if (e != e) { nans++; continue; }
		frb_select_count<PASS>(s_hist, fri_bits(e), prefix);
	}
	__syncthreads();
	frb_select_flush<PASS>(a.hist, s_hist);
	if (PASS == 0 && nans) atomicAdd(&a.hist[4 * 256], nans);
}

__global__ __launch_bounds__(FRI_THREADS) void k_ingest_mask(FriArgs a)
{
	__shared__ uint32_t s_wave[4], s_out[3];
	const int tid = threadIdx.x;
	uint32_t med = 0u, has_nan = 0u;
	float thr = 0.0f;
	if (a.mode == FR_INGEST_NONPRESENCE)
	{
		med = fri_prefix(a, 4, s_wave, s_out);
		has_nan = a.hist[4 * 256] != 0u;
		if (has_nan) med = FRI_NAN_BITS;
		thr = fri_threshold(a.ratio, fri_float(med));
	}
	const int g = blockIdx.x * FRI_THREADS + tid;
	bool sel = false;
	if (g < a.G)
	{
		const int gy = g / a.Gw, gx = g - gy * a.Gw;
		for (int dy = 0; dy < a.d; dy++)
			for (int dx = 0; dx < a.d; dx++)
			{
				const size_t p = (size_t)(gy * a.d + dy) * a.W + (gx * a.d + dx);
				if (a.mode == FR_INGEST_MASK) sel |= a.mask_in[p] != 0;
				else sel |= fri_non_presence(a.depth_sil[(size_t)a.n + p], a.depth_sil[p], a.gt[p], thr, a.sil_thres) && (!a.mask_in || a.mask_in[p] != 0);
			}
		a.pooled[g] = sel ? 1 : 0;
	}
	const uint32_t count = frb_count256(sel, s_wave);
	if (tid == 0)
	{
		a.counts[blockIdx.x] = count;
		if (blockIdx.x == 0) { a.status[1] = (int32_t)has_nan; a.status[2] = 0; a.status[3] = 0; a.status[4] = (int32_t)med; }
	}
}

__global__ __launch_bounds__(FRI_THREADS) void k_ingest_scan(const uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets, int nwg,
                                                             int32_t* __restrict__ status)
{
	__shared__ uint32_t s_wave[4];
	const uint32_t total = frb_scan_counts(counts, offsets, nwg, s_wave);
	if (threadIdx.x == 0) status[0] = (int32_t)total;
}

__global__ __launch_bounds__(FRI_THREADS) void k_ingest_scatter(FriArgs a)
{
	__shared__ uint32_t s_wave[4];
	const int g = blockIdx.x * FRI_THREADS + threadIdx.x;
	const bool sel = g < a.G && a.pooled[g] != 0;
	const uint32_t before = frb_rank256(sel, s_wave);        // (a barrier: in front of the return)
	if (!sel) return;
	const uint32_t slot = a.offsets[blockIdx.x] + before;
	if (slot < (uint32_t)a.G) a.idx[slot] = g;            // always: at most G cells are selected
}

struct FriEmitArgs {
	const float* color;          // [3,H,W]
	const float* gt;             // [1,H,W]
	const float* w2c;            // [4,4] row-major, or null: camera frame
	const float* intr;           // [3,3] row-major
	const int32_t* idx;          // ascending cells, or null: all of them
	int count, H, W, d, Gw, scale_cols, means_stride, colors_stride;
	long long row_offset;
	float *means, *rgb, *rot, *opac, *logs, *msd;
};

__global__ __launch_bounds__(FRI_THREADS) void k_ingest_emit(FriEmitArgs a)
{
	__shared__ float s_m[12], s_k[4];
	const int tid = threadIdx.x;
	if (tid == 0)
	{
		if (a.w2c) fri_invert_affine(a.w2c, s_m);
		s_k[0] = a.intr[0]; s_k[1] = a.intr[4]; s_k[2] = a.intr[2]; s_k[3] = a.intr[5];
	}
	__syncthreads();
	const int i = blockIdx.x * FRI_THREADS + tid;
	if (i >= a.count) return;
	const int g = a.idx ? a.idx[i] : i;
	const int gy = g / a.Gw, gx = g - gy * a.Gw;
	const int x = gx * a.d, y = gy * a.d;
	if (x >= a.W || y >= a.H || g < 0) return;             // never with a list that fr_frame_ingest_select wrote
	const size_t p = (size_t)y * a.W + x, hw = (size_t)a.H * a.W;
	const float z = a.gt[p];
	const size_t row = (size_t)(a.row_offset + i);
	if (a.means)
	{
		float pt[3];
		fri_back_project(x, y, z, s_k[0], s_k[1], s_k[2], s_k[3], a.w2c ? s_m : nullptr, pt);
		float* o = a.means + row * a.means_stride;
		o[0] = pt[0]; o[1] = pt[1]; o[2] = pt[2];
	}
	if (a.rgb)
	{
		float* o = a.rgb + row * a.colors_stride;
		o[0] = a.color[p]; o[1] = a.color[hw + p]; o[2] = a.color[2 * hw + p];
	}
	if (a.rot) { float* o = a.rot + row * 4; o[0] = 1.0f; o[1] = 0.0f; o[2] = 0.0f; o[3] = 0.0f; }
	if (a.opac) a.opac[row] = 0.0f;
	if (a.logs || a.msd)
	{
		const float m = fri_mean3_sq_dist(a.d, z, s_k[0], s_k[1]);
		if (a.msd) a.msd[row] = m;
		if (a.logs)
		{
			const float l = fri_log_scale(m);
			for (int c = 0; c < a.scale_cols; c++) a.logs[row * a.scale_cols + c] = l;
		}
	}
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

struct FriLayout { size_t idx, pooled, counts, offsets, total; int G, Gw, nwg; };

static bool fri_shape_ok(int32_t H, int32_t W, int32_t d)
{
	if (H <= 0 || W <= 0 || d <= 0) return false;
	if ((int64_t)H * W > ((int64_t)1 << 30)) return false;
	return H % d == 0 && W % d == 0;
}

static FriLayout fri_layout(int32_t H, int32_t W, int32_t d)
{
	FriLayout l;
	l.Gw = W / d;
	l.G = (H / d) * l.Gw;
	l.nwg = (l.G + FRI_THREADS - 1) / FRI_THREADS;
	l.idx = FR_INGEST_WS_INDEX_OFFSET;
	l.pooled = l.idx + (size_t)l.G * sizeof(int32_t);
	l.counts = (l.pooled + (size_t)l.G + 15) & ~(size_t)15;
	l.offsets = l.counts + (size_t)l.nwg * sizeof(uint32_t);
	l.total = l.offsets + (size_t)l.nwg * sizeof(uint32_t);
	return l;
}

extern "C" size_t fr_frame_ingest_workspace_bytes(int32_t H, int32_t W, int32_t downsample)
{
	static_assert(FRI_HEAD_BYTES <= FR_INGEST_WS_INDEX_OFFSET, "the histograms must fit in front of the index list");
	if (!fri_shape_ok(H, W, downsample)) return 0;
	return fri_layout(H, W, downsample).total;
}

extern "C" int fr_frame_ingest_select(const fr_frame_ingest_cfg* cfg, const float* depth_sil, const float* gt_depth, const uint8_t* mask_in,
                                      int32_t* status, void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	if (!cfg) return fr_fail(FR_EINVAL, "fr_frame_ingest_select: null cfg");
	if (cfg->H <= 0 || cfg->W <= 0 || cfg->downsample <= 0 || (int64_t)cfg->H * cfg->W > ((int64_t)1 << 30))
		return fr_fail(FR_EINVAL, "fr_frame_ingest_select: bad argument (cfg: H, W, downsample; H W at most 2^30)");
	if (cfg->H % cfg->downsample || cfg->W % cfg->downsample)
		return fr_fail(FR_EINVAL, "fr_frame_ingest_select: bad argument (downsample must divide H and W)");
	if (cfg->mode != FR_INGEST_NONPRESENCE && cfg->mode != FR_INGEST_MASK)
		return fr_fail(FR_EINVAL, "fr_frame_ingest_select: bad argument (cfg->mode)");
	if (cfg->mode == FR_INGEST_NONPRESENCE && (!depth_sil || !gt_depth))
		return fr_fail(FR_EINVAL, "fr_frame_ingest_select: null pointer (depth_sil, gt_depth in FR_INGEST_NONPRESENCE)");
	if (cfg->mode == FR_INGEST_MASK && !mask_in) return fr_fail(FR_EINVAL, "fr_frame_ingest_select: null pointer (mask_in in FR_INGEST_MASK)");
	if (!status) return fr_fail(FR_EINVAL, "fr_frame_ingest_select: null pointer (status)");
	const FriLayout l = fri_layout(cfg->H, cfg->W, cfg->downsample);
	if (!workspace || workspace_bytes < l.total) return fr_fail(FR_ENOSPACE, "fr_frame_ingest_select: workspace too small (fr_frame_ingest_workspace_bytes)");
	if ((uintptr_t)workspace % 8) return fr_fail(FR_EINVAL, "fr_frame_ingest_select: bad argument (workspace must be 8-byte aligned)");

	char* ws = (char*)workspace;
	FriArgs a;
	a.depth_sil = depth_sil; a.gt = gt_depth; a.mask_in = mask_in;
	a.H = cfg->H; a.W = cfg->W; a.d = cfg->downsample; a.Gw = l.Gw; a.G = l.G; a.mode = cfg->mode;
	a.n = (uint32_t)((int64_t)cfg->H * cfg->W);
	a.sil_thres = cfg->sil_thres; a.ratio = cfg->depth_error_ratio;
	a.hist = (uint32_t*)ws; a.pooled = (uint8_t*)(ws + l.pooled);
	a.counts = (uint32_t*)(ws + l.counts); a.offsets = (uint32_t*)(ws + l.offsets);
	a.idx = (int32_t*)(ws + l.idx); a.status = status;
	hipStream_t s = (hipStream_t)stream;
	const dim3 block(FRI_THREADS), grid(l.nwg);
	int rc;
	if (cfg->mode == FR_INGEST_NONPRESENCE)
	{
		if (hipMemsetAsync(ws, 0, FRI_HEAD_BYTES, s) != hipSuccess) return fr_fail(FR_ELAUNCH, "fr_frame_ingest_select: hipMemsetAsync failed");
		const uint32_t per = FRI_THREADS * FRI_HIST_ITEMS;
		const dim3 hgrid((a.n + per - 1) / per);
		hipLaunchKernelGGL(k_ingest_hist<0>, hgrid, block, 0, s, a);
		hipLaunchKernelGGL(k_ingest_hist<1>, hgrid, block, 0, s, a);
		hipLaunchKernelGGL(k_ingest_hist<2>, hgrid, block, 0, s, a);
		hipLaunchKernelGGL(k_ingest_hist<3>, hgrid, block, 0, s, a);
		if ((rc = fr_check_launch("k_ingest_hist"))) return rc;
	}
	hipLaunchKernelGGL(k_ingest_mask, grid, block, 0, s, a);
	if ((rc = fr_check_launch("k_ingest_mask"))) return rc;
	hipLaunchKernelGGL(k_ingest_scan, dim3(1), block, 0, s, (const uint32_t*)a.counts, a.offsets, l.nwg, status);
	if ((rc = fr_check_launch("k_ingest_scan"))) return rc;
	hipLaunchKernelGGL(k_ingest_scatter, grid, block, 0, s, a);
	return fr_check_launch("k_ingest_scatter");
}

extern "C" int fr_frame_ingest_emit(const fr_frame_ingest_cfg* cfg, const float* color, const float* gt_depth, const float* w2c,
                                    const void* workspace, int32_t count, int64_t row_offset,
                                    float* means3D, float* rgb_colors, float* unnorm_rotations, float* logit_opacities,
                                    float* log_scales, float* mean3_sq_dist, fr_stream_t stream)
{
	if (!cfg) return fr_fail(FR_EINVAL, "fr_frame_ingest_emit: null cfg");
	if (!fri_shape_ok(cfg->H, cfg->W, cfg->downsample))
		return fr_fail(FR_EINVAL, "fr_frame_ingest_emit: bad argument (cfg: H, W, downsample, which must divide H and W)");
	const FriLayout l = fri_layout(cfg->H, cfg->W, cfg->downsample);
	if (count < 0 || count > l.G || row_offset < 0) return fr_fail(FR_EINVAL, "fr_frame_ingest_emit: bad argument (count, row_offset)");
	if (!workspace && count != l.G && count != 0)
		return fr_fail(FR_EINVAL, "fr_frame_ingest_emit: bad argument (without an index list count must be every grid point)");
	if (cfg->scale_cols != 1 && cfg->scale_cols != 3) return fr_fail(FR_EINVAL, "fr_frame_ingest_emit: bad argument (cfg->scale_cols is 1 or 3)");
	if (cfg->means_stride < 3 || cfg->colors_stride < 3) return fr_fail(FR_EINVAL, "fr_frame_ingest_emit: bad argument (cfg: means_stride, colors_stride at least 3)");
	if (!color || !gt_depth || !cfg->intrinsics) return fr_fail(FR_EINVAL, "fr_frame_ingest_emit: null pointer (color, gt_depth, cfg->intrinsics)");
	if (cfg->transform_pts && !w2c) return fr_fail(FR_EINVAL, "fr_frame_ingest_emit: null pointer (w2c with cfg->transform_pts)");
	if (count == 0) return FR_OK;
	FriEmitArgs a;
	a.color = color; a.gt = gt_depth; a.w2c = cfg->transform_pts ? w2c : nullptr; a.intr = cfg->intrinsics;
	a.idx = workspace ? (const int32_t*)((const char*)workspace + l.idx) : nullptr;
	a.count = count; a.H = cfg->H; a.W = cfg->W; a.d = cfg->downsample; a.Gw = l.Gw;
	a.scale_cols = cfg->scale_cols; a.means_stride = cfg->means_stride; a.colors_stride = cfg->colors_stride;
	a.row_offset = row_offset;
	a.means = means3D; a.rgb = rgb_colors; a.rot = unnorm_rotations; a.opac = logit_opacities; a.logs = log_scales; a.msd = mean3_sq_dist;
	hipLaunchKernelGGL(k_ingest_emit, dim3((count + FRI_THREADS - 1) / FRI_THREADS), dim3(FRI_THREADS), 0, (hipStream_t)stream, a);
	return fr_check_launch("k_ingest_emit");
}
