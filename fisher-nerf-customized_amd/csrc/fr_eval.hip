// fr_eval.hip -- the render-quality evaluation of libfisher_rast.so (gfx950, wave64): fr_view_metrics / fr_view_metrics_summary.
//
// The reference scores a rendered view against its ground truth with calc_psnr, a depth mean, `ssim` (five grouped 11 x 11 conv2d
// calls and about twenty element-wise kernels) and four `.item()` reads, one pose at a time
// (tester_gaussians_navigation.py:1450-1491; models/SLAM/utils/eval_helpers.py:230-257 for a training frame).  Here a batch of V
// views is three launches and no synchronisation:
//
//   k_view_metrics_tiles<U8, MASKED>   grid (tiles, views) x 256 threads, a 16 x 16 pixel tile per workgroup with fr_loss.hip's
//                                      tiling and passes (fr_ssim_tile.h).  The workgroup does the three channels of its tile one after the other: render and
//                                      target go to LDS with a halo of 5 (zero padded; the render clamped, both times the mask),
//                                      the horizontal 11-tap pass fills 26 rows x 16 columns x 5 moments, the vertical pass gives
//                                      every lane its pixel's moments and frl_ssim_pixel its SSIM term; a tile with a window that
//                                      is black in one image runs the two passes again over the raw moments for those pixels
//                                      (fr_eval_math.h: fre_window_is_dark).  A byte target's pixel
//                                      and the mask are read ONCE, into one packed word per halo pixel, before the channel loop.
//                                      (x - y)^2 per channel, the SSIM terms and the depth terms of the lane's pixel are summed per
//                                      workgroup in fp64 and stored as plain partials [V][7][T].
//   k_view_metrics_rows                one workgroup per view: a wave per quantity adds that quantity's T partials in a fixed order
//                                      in fp64; thread 0 finalises the row in fp64 (fre_finalise_row) and rounds it once.
//   k_view_metrics_summary             one workgroup: the rows are staged through LDS 256 at a time and added by thread 0 in index
//                                      order under the reference's keep rule (fre_summary_add).
//
// No atomics: the same call gives the same bits.  The arithmetic is csrc/fr_eval_math.h over csrc/fr_loss_math.h, which the CPU
// harness compiles too.  LDS: 5.4 KB (two 26 x 26 float tiles) + 2.7 KB (the packed words) + 8.3 KB (26 x 16 x 5) + 0.5 KB (wave sums, vote).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "fr_internal.h"
#include "fr_block.h"
#include "fr_ssim_tile.h"
#include "fr_eval_math.h"

static_assert(FRS_THREADS == FRB_THREADS, "fr_block.h is written for 256 threads");
#define FRE_IN_IMAGE 0x80000000u                 // packed word: bytes 0..2 = the target's bytes, bit 24 = mask, bit 31 = in the image
#define FRE_MASK_BIT 0x01000000u

struct FrEvalArgs {
	const float* render;         // [V] x [3,H,W], view stride render_vs
	const float* depth;          // [V] x [H,W], view stride depth_vs, or null
	const void* gt;              // float [V][3][H][W] or bytes [V][H][W][gt_channels]
	const float* gt_depth;       // [V] x [H,W], view stride gt_depth_vs, or null
	const uint8_t* mask;         // [V][H][W] or null
	long long render_vs, depth_vs, gt_depth_vs;
	int H, W, gx, T;             // tiles per row, tiles per view
	int gt_channels, clamp, valid_only;
	double* partials;            // [V][FRE_SUMS][T]
};

template <bool U8, bool MASKED>
__global__ __launch_bounds__(FRS_THREADS) void k_view_metrics_tiles(FrEvalArgs a)
{
	__shared__ float s_x[FRS_EXT * FRS_EXT], s_y[FRS_EXT * FRS_EXT];
	__shared__ uint32_t s_pix[FRS_EXT * FRS_EXT];
	__shared__ float s_h[5][FRS_EXT * FRS_TILE];
	__shared__ double s_red[FRE_SUMS][FRS_THREADS / 64];
	const int tid = threadIdx.x, v = blockIdx.y;
	const int tile = blockIdx.x, tx = tile % a.gx, ty = tile / a.gx;
	const int lx = tid % FRS_TILE, ly = tid / FRS_TILE;
	const int px = tx * FRS_TILE + lx, py = ty * FRS_TILE + ly;
	const bool inside = px < a.W && py < a.H;
	const size_t hw = (size_t)a.H * a.W;
	const float* render = a.render + (size_t)v * a.render_vs;

	// what is read once per halo pixel: whether it lies in the image, its mask bit, a byte target's three bytes
	for (int i = tid; i < FRS_EXT * FRS_EXT; i += FRS_THREADS)
	{
		const int gy = ty * FRS_TILE - FRL_RADIUS + i / FRS_EXT, gx = tx * FRS_TILE - FRL_RADIUS + i % FRS_EXT;
		uint32_t w = 0;
		if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W)
		{
			const size_t o = (size_t)gy * a.W + gx;
			w = FRE_IN_IMAGE;
			if (!MASKED || a.mask[(size_t)v * hw + o]) w |= FRE_MASK_BIT;
			if (U8)
			{
				const uint8_t* p = (const uint8_t*)a.gt + ((size_t)v * hw + o) * a.gt_channels;
				w |= (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
			}
		}
		s_pix[i] = w;
	}

	double sums[FRE_SUMS];
#pragma unroll
	for (int k = 0; k < FRE_SUMS; k++) sums[k] = 0.0;

	for (int c = 0; c < 3; c++)
	{
		__syncthreads();                  // s_pix is written; the previous channel's tiles and moments have been read
		for (int i = tid; i < FRS_EXT * FRS_EXT; i += FRS_THREADS)
		{
			const uint32_t w = s_pix[i];
			float xv = 0.0f, yv = 0.0f;
			if (w & FRE_IN_IMAGE)
			{
				const int gy = ty * FRS_TILE - FRL_RADIUS + i / FRS_EXT, gx = tx * FRS_TILE - FRL_RADIUS + i % FRS_EXT;
				const size_t oc = (size_t)c * hw + (size_t)gy * a.W + gx;
				const float m = (w & FRE_MASK_BIT) ? 1.0f : 0.0f;
				xv = fre_render(render[oc], a.clamp, m, MASKED);
				const float t = U8 ? fre_byte((uint8_t)(w >> (8 * c))) : ((const float*)a.gt)[(size_t)v * 3 * hw + oc];
				yv = fre_target(t, m, MASKED);
			}
			s_x[i] = xv; s_y[i] = yv;
		}
		__syncthreads();
		frs_rows<frl_conv11_moments>(s_x, s_y, s_h);
		__syncthreads();
		float mo[5];
		frs_columns(s_h, lx, ly, mo);
		float dmu, d11, d12;
		float ssim = frl_ssim_pixel(mo[0], mo[1], mo[2], mo[3], mo[4], dmu, d11, d12);
		// a window black in one image (fr_eval_math.h): the raw moments, in a second pass through s_h that a tile without such a
		// pixel skips.  The vote is a barrier: every lane has read its moments by then.
		const bool dark = inside && fre_window_is_dark(mo[0], mo[1]);
		if (__syncthreads_or(dark))
		{
			frs_rows<fre_conv11_raw_moments>(s_x, s_y, s_h);
			__syncthreads();
			if (dark)
			{
				frs_columns(s_h, lx, ly, mo);
				ssim = fre_ssim_pixel_raw(mo[0], mo[1], mo[2], mo[3], mo[4]);
			}
		}
		if (inside)
		{
			const int o = (ly + FRL_RADIUS) * FRS_EXT + lx + FRL_RADIUS;
			const double sq = (double)fre_sq_diff(s_x[o], s_y[o]);
			if (c == 0) sums[FRE_S_MSE] = sq; else if (c == 1) sums[FRE_S_MSE + 1] = sq; else sums[FRE_S_MSE + 2] = sq;
			sums[FRE_S_SSIM] += (double)ssim;
		}
	}

	if (a.depth && inside)
	{
		const size_t o = (size_t)py * a.W + px;
		const float g = a.gt_depth[(size_t)v * a.gt_depth_vs + o];
		if (fre_depth_counts(g, a.valid_only))
		{
			const float m = (s_pix[(ly + FRL_RADIUS) * FRS_EXT + lx + FRL_RADIUS] & FRE_MASK_BIT) ? 1.0f : 0.0f;
			const float dd = fre_depth_diff(a.depth[(size_t)v * a.depth_vs + o], g, m, MASKED);
			sums[FRE_S_DL1] = (double)fabsf(dd);
			sums[FRE_S_DSQ] = (double)(dd * dd);
			sums[FRE_S_DCNT] = 1.0;
		}
	}

	frb_sum256<FRE_SUMS>(sums, s_red);
	if (tid < FRE_SUMS) a.partials[((size_t)v * FRE_SUMS + tid) * a.T + tile] = frb_sum4(s_red[tid]);
}

// A quantity's T partials are added by one wave: lane l adds partials l, l + 64, .. in index order, then the lanes in a fixed tree.
__global__ __launch_bounds__(FRS_THREADS) void k_view_metrics_rows(const double* __restrict__ partials, int T, double hw, int has_depth,
                                                                   float* __restrict__ rows)
{
	__shared__ double s_sum[FRE_SUMS];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, v = blockIdx.x;
	for (int q = wave; q < FRE_SUMS; q += FRS_THREADS / 64)
	{
		const double s = frb_row_sum(partials + ((size_t)v * FRE_SUMS + q) * T, T);
		if (lane == 0) s_sum[q] = s;
	}
	__syncthreads();
	if (tid != 0) return;
	double s[FRE_SUMS];
	for (int q = 0; q < FRE_SUMS; q++) s[q] = s_sum[q];
	float row[FRE_ROW];
	fre_finalise_row(s, hw, has_depth, row);
	for (int k = 0; k < FRE_ROW; k++) rows[(size_t)v * FRE_ROW + k] = row[k];
}

__global__ __launch_bounds__(FRS_THREADS) void k_view_metrics_summary(const float* __restrict__ rows, int V, float* __restrict__ summary)
{
	__shared__ float s_rows[FRS_THREADS][4];
	const int tid = threadIdx.x;
	double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
	for (int v0 = 0; v0 < V; v0 += FRS_THREADS)
	{
		const int n = V - v0 < FRS_THREADS ? V - v0 : FRS_THREADS;
		__syncthreads();
		if (tid < n)
			for (int k = 0; k < 4; k++) s_rows[tid][k] = rows[(size_t)(v0 + tid) * FRE_ROW + k];
		__syncthreads();
		if (tid == 0)
			for (int i = 0; i < n; i++)
			{
				float row[FRE_ROW];
				for (int k = 0; k < 4; k++) row[k] = s_rows[i][k];
				fre_summary_add(acc, row);
			}
	}
	if (tid != 0) return;
	float out[FRE_ROW];
	fre_summary_finish(acc, V, out);
	for (int k = 0; k < FRE_ROW; k++) summary[k] = out[k];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

static int fre_tiles(int n) { return (n + FRS_TILE - 1) / FRS_TILE; }

static bool fre_dims_ok(int32_t V, int32_t H, int32_t W)
{
	// the views ride on the grid's y; H W within 2^30 keeps every tile count and every in-view offset far inside 32 bits
	return V >= 1 && V <= 65535 && fr_image_ok(H, W);
}

extern "C" size_t fr_view_metrics_workspace_bytes(int32_t V, int32_t H, int32_t W)
{
	if (!fre_dims_ok(V, H, W)) return 0;
	return (size_t)V * FRE_SUMS * fre_tiles(H) * fre_tiles(W) * sizeof(double);       // the per-workgroup partials [V][7][T]
}

extern "C" int fr_view_metrics_summary(const float* rows, int32_t V, float* summary, fr_stream_t stream)
{
	if (!rows || !summary) return fr_fail(FR_EINVAL, "fr_view_metrics_summary: null pointer (rows, summary)");
	if (V < 1) return fr_fail(FR_EINVAL, "fr_view_metrics_summary: bad argument (V >= 1)");
	hipLaunchKernelGGL(k_view_metrics_summary, dim3(1), dim3(FRS_THREADS), 0, (hipStream_t)stream, rows, V, summary);
	return fr_check_launch("k_view_metrics_summary");
}

extern "C" int fr_view_metrics(const fr_view_metrics_cfg* cfg, const float* render, const float* depth, const void* gt_rgb,
                               const float* gt_depth, const uint8_t* mask, float* rows, float* summary,
                               void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	if (!cfg) return fr_fail(FR_EINVAL, "fr_view_metrics: null pointer (cfg)");
	if (!fre_dims_ok(cfg->V, cfg->H, cfg->W))
		return fr_fail(FR_EINVAL, "fr_view_metrics: bad argument (cfg: 1 <= V <= 65535, H >= 1, W >= 1, H W <= 2^30)");
	if (cfg->gt_layout != FR_EVAL_GT_F32_CHW && cfg->gt_layout != FR_EVAL_GT_U8_HWC)
		return fr_fail(FR_EINVAL, "fr_view_metrics: bad argument (cfg->gt_layout: FR_EVAL_GT_F32_CHW or FR_EVAL_GT_U8_HWC)");
	if (cfg->gt_layout == FR_EVAL_GT_U8_HWC && cfg->gt_channels != 3 && cfg->gt_channels != 4)
		return fr_fail(FR_EINVAL, "fr_view_metrics: bad argument (cfg->gt_channels: 3 or 4 for a byte target)");
	if ((cfg->clamp_render != 0 && cfg->clamp_render != 1) || (cfg->depth_valid_only != 0 && cfg->depth_valid_only != 1))
		return fr_fail(FR_EINVAL, "fr_view_metrics: bad argument (cfg->clamp_render and cfg->depth_valid_only: 0 or 1)");
	if (!render || !gt_rgb || !rows || !summary) return fr_fail(FR_EINVAL, "fr_view_metrics: null pointer (render, gt_rgb, rows, summary)");
	if ((depth != nullptr) != (gt_depth != nullptr))
		return fr_fail(FR_EINVAL, "fr_view_metrics: bad argument (depth and gt_depth go together: both or neither)");
	const int64_t hw = (int64_t)cfg->H * cfg->W;
	if (cfg->render_view_stride < 3 * hw)
		return fr_fail(FR_EINVAL, "fr_view_metrics: bad argument (cfg->render_view_stride below 3 H W)");
	if (depth && (cfg->depth_view_stride < hw || cfg->gt_depth_view_stride < hw))
		return fr_fail(FR_EINVAL, "fr_view_metrics: bad argument (cfg->depth_view_stride / gt_depth_view_stride below H W)");
	if (!workspace || workspace_bytes < fr_view_metrics_workspace_bytes(cfg->V, cfg->H, cfg->W))
		return fr_fail(FR_EINVAL, "fr_view_metrics: workspace null or too small (fr_view_metrics_workspace_bytes)");
	if ((uintptr_t)workspace % sizeof(double)) return fr_fail(FR_EINVAL, "fr_view_metrics: bad argument (workspace must be 8-byte aligned)");

	FrEvalArgs a;
	a.render = render; a.depth = depth; a.gt = gt_rgb; a.gt_depth = gt_depth; a.mask = mask;
	a.render_vs = cfg->render_view_stride; a.depth_vs = cfg->depth_view_stride; a.gt_depth_vs = cfg->gt_depth_view_stride;
	a.H = cfg->H; a.W = cfg->W; a.gx = fre_tiles(cfg->W); a.T = a.gx * fre_tiles(cfg->H);
	a.gt_channels = cfg->gt_channels; a.clamp = cfg->clamp_render; a.valid_only = cfg->depth_valid_only;
	a.partials = (double*)workspace;
	hipStream_t s = (hipStream_t)stream;
	const dim3 grid(a.T, cfg->V), block(FRS_THREADS);
	if (cfg->gt_layout == FR_EVAL_GT_U8_HWC)
	{
		if (mask) hipLaunchKernelGGL((k_view_metrics_tiles<true, true>), grid, block, 0, s, a);
		else hipLaunchKernelGGL((k_view_metrics_tiles<true, false>), grid, block, 0, s, a);
	}
	else
	{
		if (mask) hipLaunchKernelGGL((k_view_metrics_tiles<false, true>), grid, block, 0, s, a);
		else hipLaunchKernelGGL((k_view_metrics_tiles<false, false>), grid, block, 0, s, a);
	}
	int rc;
	if ((rc = fr_check_launch("k_view_metrics_tiles"))) return rc;
	hipLaunchKernelGGL(k_view_metrics_rows, dim3(cfg->V), block, 0, s, (const double*)workspace, a.T, (double)hw, depth ? 1 : 0, rows);
	if ((rc = fr_check_launch("k_view_metrics_rows"))) return rc;
	hipLaunchKernelGGL(k_view_metrics_summary, dim3(1), block, 0, s, (const float*)rows, (int)cfg->V, summary);
	return fr_check_launch("k_view_metrics_summary");
}
