// fr_loss.hip -- the training step's image loss of libfisher_rast.so (gfx950, wave64): fr_image_loss_forward / _backward.
//
// The reference forms w_l1 * L1 + w_ssim * (1 - SSIM) between a render and its target with five grouped 11 x 11 conv2d calls,
// about twenty element-wise kernels, the same again in autograd, and boolean-mask indexing that synchronises the host
// (models/SLAM/utils/slam_helpers.py:23-77, slam_external.py:77-193).  Here that is three launches and no synchronisation:
//
//   k_image_loss_tiles<SSIM, MASKED>     grid (tiles, channels) x 256 threads, a 16 x 16 pixel tile per workgroup (768 workgroups at
//                                        3 x 256 x 256).  Render and target go to LDS with a halo of 5 (zero padded; with a mask both
//                                        are multiplied by it first), a horizontal 11-tap pass fills 26 rows x 16 columns x 5
//                                        moments (taken about 0.5: fr_loss_math.h), a vertical pass gives every lane its pixel's
//                                        moments, then the SSIM term and the three partials the backward needs.  |x - y|, the SSIM term and the mask count are summed
//                                        per workgroup in fp64 and stored as plain partials.
//   k_image_loss_reduce                  one workgroup: a wave per (quantity, channel) row adds that row's partials in a fixed order
//                                        in fp64; thread 0 adds the channels in index order and writes the loss.
//   k_image_loss_backward<SSIM, MASKED>  same tiling: the adjoint of the symmetric, zero-padded window is the same separable pass
//                                        over the three saved partial maps.  The upstream gradient is read from device memory.
//
// No atomics: the same call gives the same bits.  The arithmetic is csrc/fr_loss_math.h, which the CPU harness compiles too; the tile
// geometry and the two passes of the forward are csrc/fr_ssim_tile.h (shared with fr_eval.hip), the fp64 sums fr_block.h's.
// LDS: 5.4 KB (two 26 x 26 tiles) + 8.3 KB (26 x 16 x 5) forward, 8.1 KB + 5 KB backward.  At 3 x 256 x 256 the three kernels move
// ~6 MB: launch latency, not bandwidth, is what a call costs.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "fr_internal.h"
#include "fr_block.h"
#include "fr_ssim_tile.h"

static_assert(FRS_THREADS == FRB_THREADS, "fr_block.h is written for 256 threads");

struct FrLossArgs {
	const float* x;              // [C,H,W] render
	const float* y;              // [C,H,W] target
	const uint8_t* mask;         // [C,H,W] or [1,H,W] bytes (0 / 1), or null
	long long mask_cstride;      // H W or 0
	int C, H, W, gx, T;          // tiles per row, tiles per channel
	int weights_map;             // the mask weights the SSIM map (calc_ssim_masked) instead of multiplying the images
	float* ssim_map;             // [C,H,W] or null
	float* saved;                // [3,C,H,W] partial maps (SSIM only)
	double* partials;            // [3][C][T]: SSIM sum, L1 sum, count
};

// x, y of pixel (py, px) of channel c as the loss sees them (zero outside the image; times the mask where it multiplies the images)
template <bool MASKED>
__device__ __forceinline__ void frl_load(const FrLossArgs& a, int c, int py, int px, float& xv, float& yv, float& m)
{
	xv = 0.0f; yv = 0.0f; m = 0.0f;
	if (py < 0 || py >= a.H || px < 0 || px >= a.W) return;
	const size_t o = (size_t)py * a.W + px, oc = (size_t)c * a.H * a.W + o;
	xv = a.x[oc]; yv = a.y[oc]; m = 1.0f;
	if (MASKED)
	{
		m = a.mask[(size_t)c * a.mask_cstride + o] ? 1.0f : 0.0f;
		if (!a.weights_map) { xv = xv * m; yv = yv * m; }
	}
}

template <bool SSIM, bool MASKED>
__global__ __launch_bounds__(FRS_THREADS) void k_image_loss_tiles(FrLossArgs a)
{
	__shared__ float s_x[SSIM ? FRS_EXT * FRS_EXT : 1], s_y[SSIM ? FRS_EXT * FRS_EXT : 1];
	__shared__ float s_h[SSIM ? 5 : 1][SSIM ? FRS_EXT * FRS_TILE : 1];
	__shared__ double s_red[3][FRS_THREADS / 64];
	const int tid = threadIdx.x, c = blockIdx.y;
	const int tile = blockIdx.x, tx = tile % a.gx, ty = tile / a.gx;
	const int lx = tid % FRS_TILE, ly = tid / FRS_TILE;
	const int px = tx * FRS_TILE + lx, py = ty * FRS_TILE + ly;
	const bool inside = px < a.W && py < a.H;
	float xv, yv, m;
	double v[3] = {0.0, 0.0, 0.0};                            // SSIM term, |x - y|, mask count
	if constexpr (SSIM)
	{
		for (int i = tid; i < FRS_EXT * FRS_EXT; i += FRS_THREADS)
		{
			const int r = i / FRS_EXT, q = i % FRS_EXT;
			float mm;
			frl_load<MASKED>(a, c, ty * FRS_TILE - FRL_RADIUS + r, tx * FRS_TILE - FRL_RADIUS + q, s_x[i], s_y[i], mm);
		}
		__syncthreads();
		frs_rows<frl_conv11_moments>(s_x, s_y, s_h);
		__syncthreads();
		float mo[5];
		frs_columns(s_h, lx, ly, mo);
		float dmu, d11, d12;
		float ssim = frl_ssim_pixel(mo[0], mo[1], mo[2], mo[3], mo[4], dmu, d11, d12);
		xv = s_x[(ly + FRL_RADIUS) * FRS_EXT + lx + FRL_RADIUS];
		yv = s_y[(ly + FRL_RADIUS) * FRS_EXT + lx + FRL_RADIUS];
		m = 1.0f;
		if (MASKED && inside) m = a.mask[(size_t)c * a.mask_cstride + (size_t)py * a.W + px] ? 1.0f : 0.0f;
		if (inside)
		{
			const size_t n = (size_t)a.C * a.H * a.W, o = ((size_t)c * a.H + py) * a.W + px;
			if (MASKED && a.weights_map && m == 0.0f) { ssim = 0.0f; dmu = 0.0f; d11 = 0.0f; d12 = 0.0f; }
			if (a.ssim_map) a.ssim_map[o] = ssim;
			a.saved[o] = dmu; a.saved[n + o] = d11; a.saved[2 * n + o] = d12;
			v[0] = (double)ssim;
		}
	}
	else
		frl_load<MASKED>(a, c, py, px, xv, yv, m);
	if (inside && m != 0.0f) { v[1] = (double)fabsf(xv - yv); v[2] = 1.0; }
	frb_sum256<3>(v, s_red);
	if (tid < 3) a.partials[((size_t)tid * a.C + c) * a.T + tile] = frb_sum4(s_red[tid]);
}

// out[4] = {loss, L1 term, SSIM mean, count}; out_channel[C] = the channels' SSIM sums / (H W); tail = the two factors of the backward.
// A row of T partials is added by one wave: lane l adds partials l, l + 64, .. in index order, then the lanes are added in a fixed tree.
__global__ __launch_bounds__(FRS_THREADS) void k_image_loss_reduce(const double* __restrict__ partials, int C, int T, long long HW,
                                                                   float w_l1, float w_ssim, int denom_mode, int weights_map,
                                                                   float* __restrict__ out, float* __restrict__ out_channel,
                                                                   float* __restrict__ tail, double* __restrict__ rows)
{
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	for (int r = wave; r < 3 * C; r += FRS_THREADS / 64)
	{
		const double s = frb_row_sum(partials + (size_t)r * T, T);
		if (lane == 0) rows[r] = s;
	}
	__syncthreads();
	if (out_channel)
		for (int c = tid; c < C; c += FRS_THREADS) out_channel[c] = (float)(rows[c] / (double)HW);
	if (tid != 0) return;
	double q[3];
	for (int k = 0; k < 3; k++)
	{
		double s = 0.0;
		for (int c = 0; c < C; c++) s += rows[k * C + c];
		q[k] = s;
	}
	const double n = (double)C * (double)HW;
	const double denom = denom_mode == FR_LOSS_L1_SUM ? 1.0 : (denom_mode == FR_LOSS_L1_MEAN ? n : q[2]);
	const double norm = weights_map ? (q[2] > (double)C ? q[2] : (double)C) : n;
	const double l1 = q[1] / denom;                      // an empty mask: 0 / 0 = NaN, torch's mean of nothing
	const double ssim = q[0] / norm;
	double loss = 0.0;
	if (w_l1 != 0.0f) loss += (double)w_l1 * l1;
	if (w_ssim != 0.0f) loss += (double)w_ssim * (1.0 - ssim);
	out[0] = (float)loss; out[1] = (float)l1; out[2] = (float)ssim; out[3] = (float)q[2];
	tail[0] = (float)((double)w_l1 / denom); tail[1] = (float)((double)w_ssim / norm); tail[2] = 0.0f; tail[3] = 0.0f;
}

template <bool SSIM, bool MASKED>
__global__ __launch_bounds__(FRS_THREADS) void k_image_loss_backward(FrLossArgs a, const float* __restrict__ tail,
                                                                     const float* __restrict__ upstream, float* __restrict__ dL_dx)
{
	__shared__ float s_p[SSIM ? 3 : 1][SSIM ? FRS_EXT * FRS_EXT : 1];
	__shared__ float s_h[SSIM ? 3 : 1][SSIM ? FRS_EXT * FRS_TILE : 1];
	const int tid = threadIdx.x, c = blockIdx.y;
	const int tile = blockIdx.x, tx = tile % a.gx, ty = tile / a.gx;
	const int lx = tid % FRS_TILE, ly = tid / FRS_TILE;
	const int px = tx * FRS_TILE + lx, py = ty * FRS_TILE + ly;
	float D[3] = {0.0f, 0.0f, 0.0f};
	if (SSIM)
	{
		const size_t n = (size_t)a.C * a.H * a.W;
		for (int i = tid; i < FRS_EXT * FRS_EXT; i += FRS_THREADS)
		{
			const int gy = ty * FRS_TILE - FRL_RADIUS + i / FRS_EXT, gx = tx * FRS_TILE - FRL_RADIUS + i % FRS_EXT;
			const bool in = gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
			const size_t o = in ? ((size_t)c * a.H + gy) * a.W + gx : 0;
#pragma unroll
			for (int k = 0; k < 3; k++) s_p[k][i] = in ? a.saved[k * n + o] : 0.0f;
		}
		__syncthreads();
		for (int i = tid; i < FRS_EXT * FRS_TILE; i += FRS_THREADS)
		{
			const int r = i / FRS_TILE, q = i % FRS_TILE;
#pragma unroll
			for (int k = 0; k < 3; k++) s_h[k][i] = frl_conv11(&s_p[k][r * FRS_EXT + q], 1);
		}
		__syncthreads();
#pragma unroll
		for (int k = 0; k < 3; k++) D[k] = frl_conv11(&s_h[k][ly * FRS_TILE + lx], FRS_TILE);
	}
	if (px >= a.W || py >= a.H) return;
	float xv, yv, m;
	frl_load<MASKED>(a, c, py, px, xv, yv, m);
	const float up = upstream[0];
	float g = frl_pixel_grad(up * tail[0], -(up * tail[1]), xv, yv, D[0], D[1], D[2], SSIM);
	if (MASKED && !a.weights_map && m == 0.0f) g = 0.0f;      // selected, not multiplied: an empty mask gives zeros, not NaN
	dL_dx[((size_t)c * a.H + py) * a.W + px] = g;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

static bool frl_cfg_ok(const fr_image_loss_cfg* cfg)
{
	if (!cfg || cfg->C <= 0 || cfg->H <= 0 || cfg->W <= 0 || cfg->C > 65535) return false;
	if ((int64_t)cfg->C * cfg->H * cfg->W > ((int64_t)1 << 30)) return false;
	if (cfg->l1_denom != FR_LOSS_L1_SUM && cfg->l1_denom != FR_LOSS_L1_MEAN && cfg->l1_denom != FR_LOSS_L1_MASKED_MEAN) return false;
	if (cfg->mask_channels != 0 && cfg->mask_channels != 1 && cfg->mask_channels != cfg->C) return false;
	if (cfg->mask_weights_ssim_map != 0 && cfg->mask_weights_ssim_map != 1) return false;
	return true;
}

static int frl_tiles(int n) { return (n + FRS_TILE - 1) / FRS_TILE; }

extern "C" size_t fr_image_loss_workspace_bytes(int32_t C, int32_t H, int32_t W)
{
	if (C <= 0 || H <= 0 || W <= 0 || C > 65535) return 0;
	// the per-workgroup partials [3][C][T] and the per-row sums [3][C]
	return ((size_t)3 * C * frl_tiles(H) * frl_tiles(W) + (size_t)3 * C) * sizeof(double);
}

static FrLossArgs frl_args(const fr_image_loss_cfg* cfg, const float* img, const float* gt, const uint8_t* mask)
{
	FrLossArgs a;
	a.x = img; a.y = gt; a.mask = mask;
	a.mask_cstride = cfg->mask_channels > 1 ? (long long)cfg->H * cfg->W : 0;
	a.C = cfg->C; a.H = cfg->H; a.W = cfg->W;
	a.gx = frl_tiles(cfg->W); a.T = a.gx * frl_tiles(cfg->H);
	a.weights_map = cfg->mask_weights_ssim_map;
	a.ssim_map = nullptr; a.saved = nullptr; a.partials = nullptr;
	return a;
}

extern "C" int fr_image_loss_forward(const fr_image_loss_cfg* cfg, const float* img, const float* gt, const uint8_t* mask,
                                     float* out4, float* out_channel_ssim, float* out_ssim_map, float* saved,
                                     void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	if (!frl_cfg_ok(cfg)) return fr_fail(FR_EINVAL, "fr_image_loss_forward: bad argument (cfg: C, H, W, l1_denom, mask_channels)");
	if (!img || !gt || !out4 || !saved) return fr_fail(FR_EINVAL, "fr_image_loss_forward: null pointer (img, gt, out4, saved)");
	if ((mask != nullptr) != (cfg->mask_channels != 0))
		return fr_fail(FR_EINVAL, "fr_image_loss_forward: bad argument (mask and cfg->mask_channels must go together)");
	if (!mask && (cfg->l1_denom == FR_LOSS_L1_MASKED_MEAN || cfg->mask_weights_ssim_map))
		return fr_fail(FR_EINVAL, "fr_image_loss_forward: bad argument (a masked mean or a weighted SSIM map needs a mask)");
	const bool ssim = cfg->w_ssim != 0.0f;
	if (!ssim && (out_ssim_map || out_channel_ssim || cfg->mask_weights_ssim_map))
		return fr_fail(FR_EINVAL, "fr_image_loss_forward: bad argument (SSIM outputs asked with w_ssim == 0)");
	if (!workspace || workspace_bytes < fr_image_loss_workspace_bytes(cfg->C, cfg->H, cfg->W))
		return fr_fail(FR_ENOSPACE, "fr_image_loss_forward: workspace too small (fr_image_loss_workspace_bytes)");
	if ((uintptr_t)workspace % sizeof(double)) return fr_fail(FR_EINVAL, "fr_image_loss_forward: bad argument (workspace must be 8-byte aligned)");

	FrLossArgs a = frl_args(cfg, img, gt, mask);
	a.ssim_map = out_ssim_map; a.saved = saved; a.partials = (double*)workspace;
	hipStream_t s = (hipStream_t)stream;
	const dim3 grid(a.T, a.C), block(FRS_THREADS);
	if (ssim)
	{
		if (mask) hipLaunchKernelGGL((k_image_loss_tiles<true, true>), grid, block, 0, s, a);
		else hipLaunchKernelGGL((k_image_loss_tiles<true, false>), grid, block, 0, s, a);
	}
	else
	{
		if (mask) hipLaunchKernelGGL((k_image_loss_tiles<false, true>), grid, block, 0, s, a);
		else hipLaunchKernelGGL((k_image_loss_tiles<false, false>), grid, block, 0, s, a);
	}
	int rc;
	if ((rc = fr_check_launch("k_image_loss_tiles"))) return rc;
	const size_t n = (size_t)cfg->C * cfg->H * cfg->W;
	hipLaunchKernelGGL(k_image_loss_reduce, dim3(1), block, 0, s, (const double*)workspace, a.C, a.T, (long long)cfg->H * cfg->W,
	                   cfg->w_l1, cfg->w_ssim, cfg->l1_denom, cfg->mask_weights_ssim_map, out4, out_channel_ssim,
	                   saved + (ssim ? 3 * n : 0), (double*)workspace + (size_t)3 * a.C * a.T);
	return fr_check_launch("k_image_loss_reduce");
}

extern "C" int fr_image_loss_backward(const fr_image_loss_cfg* cfg, const float* img, const float* gt, const uint8_t* mask,
                                      const float* saved, const float* upstream, float* dL_dimg, fr_stream_t stream)
{
	if (!frl_cfg_ok(cfg)) return fr_fail(FR_EINVAL, "fr_image_loss_backward: bad argument (cfg: C, H, W, l1_denom, mask_channels)");
	if (!img || !gt || !saved || !upstream || !dL_dimg)
		return fr_fail(FR_EINVAL, "fr_image_loss_backward: null pointer (img, gt, saved, upstream, dL_dimg)");
	if ((mask != nullptr) != (cfg->mask_channels != 0))
		return fr_fail(FR_EINVAL, "fr_image_loss_backward: bad argument (mask and cfg->mask_channels must go together)");
	if (!mask && (cfg->l1_denom == FR_LOSS_L1_MASKED_MEAN || cfg->mask_weights_ssim_map))
		return fr_fail(FR_EINVAL, "fr_image_loss_backward: bad argument (a masked mean or a weighted SSIM map needs a mask)");
	const bool ssim = cfg->w_ssim != 0.0f;
	FrLossArgs a = frl_args(cfg, img, gt, mask);
	a.saved = const_cast<float*>(saved);
	const float* tail = saved + (ssim ? (size_t)3 * cfg->C * cfg->H * cfg->W : 0);
	hipStream_t s = (hipStream_t)stream;
	const dim3 grid(a.T, a.C), block(FRS_THREADS);
	if (ssim)
	{
		if (mask) hipLaunchKernelGGL((k_image_loss_backward<true, true>), grid, block, 0, s, a, tail, upstream, dL_dimg);
		else hipLaunchKernelGGL((k_image_loss_backward<true, false>), grid, block, 0, s, a, tail, upstream, dL_dimg);
	}
	else
	{
		if (mask) hipLaunchKernelGGL((k_image_loss_backward<false, true>), grid, block, 0, s, a, tail, upstream, dL_dimg);
		else hipLaunchKernelGGL((k_image_loss_backward<false, false>), grid, block, 0, s, a, tail, upstream, dL_dimg);
	}
	return fr_check_launch("k_image_loss_backward");
}
