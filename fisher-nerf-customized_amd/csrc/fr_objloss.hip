// fr_objloss.hip -- the object-aware training step of libfisher_rast.so (gfx950, wave64): fr_loss_mask, fr_bg_penalty_forward /
// _backward, fr_outside_mask.
//
// Between the render and the loss terms the reference's get_loss builds its pixel mask with a chain of comparisons, isnan calls and
// ANDs -- with ignore_outlier_depth_loss a full sort for the median as well -- and the object class adds two masked means with their
// autograd (models/SLAM/gaussian_object.py:213-275); around it get_gaussians_outside_mask projects the map into the object mask with
// two nonzero calls and four .item() reads (models/SLAM/utils/slam_external.py:270-343).  Here:
//
//   k_objloss_hist<PASS> x 4   with reject_outliers only: the exact lower median of the H W depth errors by a radix select on the bit
//                              patterns, most significant byte first -- the radix select of fr_block.h, which the frame ingest
//                              (fr_ingest.hip) uses too.  Integer histograms in LDS, flushed with integer atomics; NaNs are counted
//                              apart and make the median NaN.  Integer sums only: no dependence on the launch geometry.
//   k_objloss_mask             one thread per pixel: walks the histograms to the median (with reject_outliers), the predicate of
//                              fr_objloss_math.h, the byte, and the kept / background counts by ballot and one integer atomic a
//                              workgroup.  Without reject_outliers this is the call's only launch.
//   k_bg_penalty_partials      1024 pixels a workgroup: |im| bg over the three channels, clamp(sil) bg and bg itself, summed per
//                              thread, wave and workgroup in fp64 in a fixed order and stored as plain partials.
//   k_bg_penalty_reduce        one workgroup: a wave per quantity adds its partials in a fixed order; thread 0 writes out4 and the
//                              two denominators the backward divides by.
//   k_bg_penalty_backward      one thread per pixel writes the three channels of dL_dim and of dL_ddepth_sil (0 and 2: zeros).
//   k_outside_mask             1024 Gaussians a workgroup: projection, mask lookup, the byte; counts, NaN flags and the extreme log
//                              scales of both sets as integer keys, reduced by shuffles and LDS to eight words a workgroup.
//   k_outside_finish           one workgroup reduces those words and writes the status; exp is taken of the four extremes only.
//
// No float atomics and no float adds across threads but the fp64 sums in their fixed order: the same call gives the same bits.
// Nothing is read back to the host.  The arithmetic is csrc/fr_objloss_math.h, which the CPU harness compiles too; the select, the
// fp64 workgroup sum (frb_sum256) and the one-wave row sum (frb_row_sum) are fr_block.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "fr_internal.h"
#include "fr_block.h"
#include "fr_objloss_math.h"

#define FRO_THREADS 256
static_assert(FRO_THREADS == FRB_THREADS, "fr_block.h is written for 256 threads");
#define FRO_HIST_ITEMS 8                                   // pixels per thread of a histogram workgroup
#define FRO_HIST_BYTES (4 * 256 * sizeof(uint32_t))       // the four histograms; the NaN count sits behind them
#define FRO_HEAD_BYTES (FRO_HIST_BYTES + 64)
#define FRO_SUM_ITEMS 4                                    // pixels per thread of a penalty workgroup, Gaussians per thread of an outside-mask one

struct FroMaskArgs {
	const float* depth_sil;      // [3,H,W]
	const float* gt;             // [1,H,W]
	const uint8_t* obj;          // [H,W] or null
	uint32_t n;                  // H W
	int reject, presence;
	float sil_thres, ratio;
	uint32_t* hist;              // [4][256], then the NaN count (reject only)
	uint8_t* mask;               // [H,W]
	int32_t* status;
};

// the prefix that the first `passes` histograms fix for the lower median, element (n - 1) / 2 of the sorted errors
__device__ __forceinline__ uint32_t fro_prefix(const FroMaskArgs& a, int passes, uint32_t* s_wave, uint32_t* s_out)
{
	uint32_t k = (a.n - 1u) / 2u, inside;
	return frb_select_prefix(a.hist, passes, k, inside, s_wave, s_out);
}

template <int PASS>
__global__ __launch_bounds__(FRO_THREADS) void k_objloss_hist(FroMaskArgs a)
{
	__shared__ uint32_t s_hist[256], s_wave[4], s_out[3];
	const int tid = threadIdx.x;
	s_hist[tid] = 0u;
	const uint32_t prefix = fro_prefix(a, PASS, s_wave, s_out);
	__syncthreads();
	uint32_t nans = 0u;
	const uint32_t base = blockIdx.x * (uint32_t)(FRO_THREADS * FRO_HIST_ITEMS);
#pragma unroll
	for (int i = 0; i < FRO_HIST_ITEMS; i++)
	{
		const uint32_t p = base + (uint32_t)(i * FRO_THREADS + tid);
		if (p >= a.n) continue;
		const float e = fro_depth_error(a.gt[p], a.depth_sil[p]);
		if (e != e) { nans++; continue; }
		frb_select_count<PASS>(s_hist, fro_bits(e), prefix);
	}
	__syncthreads();
	frb_select_flush<PASS>(a.hist, s_hist);
	if (PASS == 0 && nans) atomicAdd(&a.hist[4 * 256], nans);
}

__global__ __launch_bounds__(FRO_THREADS) void k_objloss_mask(FroMaskArgs a)
{
	__shared__ uint32_t s_wave[4], s_out[3], s_bg[4];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	uint32_t med = 0u, has_nan = 0u;
	float thr = 0.0f;
	if (a.reject)
	{
		med = fro_prefix(a, 4, s_wave, s_out);
		has_nan = a.hist[4 * 256] != 0u;
		if (has_nan) med = FRO_NAN_BITS;
		thr = fro_threshold(a.ratio, fro_float(med));
	}
	const uint32_t p = blockIdx.x * (uint32_t)FRO_THREADS + (uint32_t)tid;
	bool keep = false, bg = false;
	if (p < a.n)
	{
		const uint8_t o = a.obj ? a.obj[p] : (uint8_t)1;
		keep = fro_keep(a.depth_sil[p], a.depth_sil[(size_t)a.n + p], a.depth_sil[2 * (size_t)a.n + p], a.gt[p], a.reject != 0, thr,
		                a.presence != 0, a.sil_thres, a.obj != nullptr, o);
		bg = a.obj != nullptr && o == 0;
		a.mask[p] = keep ? 1 : 0;
	}
	const unsigned long long kept = __ballot(keep), back = __ballot(bg);
	if (lane == 0) { s_wave[wave] = (uint32_t)__popcll(kept); s_bg[wave] = (uint32_t)__popcll(back); }
	__syncthreads();
	if (tid == 0)
	{
		const uint32_t nk = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3], nb = ((s_bg[0] + s_bg[1]) + s_bg[2]) + s_bg[3];
		if (nk) atomicAdd(&a.status[0], (int32_t)nk);         // integer sums: the status was zeroed in front of the launch
		if (nb) atomicAdd(&a.status[2], (int32_t)nb);
		if (blockIdx.x == 0) { a.status[1] = (int32_t)has_nan; a.status[3] = 0; a.status[4] = (int32_t)med; }
	}
}

// ---- background penalties --------------------------------------------------------------------------------------------------------

struct FroPenaltyArgs {
	const float* im;             // [3,H,W]
	const float* depth_sil;      // [3,H,W]: channel 1 is read
	const uint8_t* obj;          // [H,W]
	uint32_t n;                  // H W
	int T;                       // workgroups of the partial pass
	float lambda_rgb, lambda_alpha;
};

__global__ __launch_bounds__(FRO_THREADS) void k_bg_penalty_partials(FroPenaltyArgs a, double* __restrict__ partials)
{
	__shared__ double s_red[3][FRO_THREADS / 64];
	const int tid = threadIdx.x;
	double v[3] = {0.0, 0.0, 0.0};
	const uint32_t base = blockIdx.x * (uint32_t)(FRO_THREADS * FRO_SUM_ITEMS);
#pragma unroll
	for (int i = 0; i < FRO_SUM_ITEMS; i++)
	{
		const uint32_t p = base + (uint32_t)(i * FRO_THREADS + tid);
		if (p >= a.n) continue;
		const float bg = fro_background(a.obj[p]);
		for (int c = 0; c < 3; c++) v[0] += (double)fro_rgb_term(a.im[(size_t)c * a.n + p], bg);
		v[1] += (double)fro_alpha_term(a.depth_sil[(size_t)a.n + p], bg);
		v[2] += (double)bg;
	}
	frb_sum256<3>(v, s_red);
	if (tid < 3) partials[(size_t)tid * a.T + blockIdx.x] = frb_sum4(s_red[tid]);
}

// A row of T partials is added by one wave: lane l adds partials l, l + 64, .. in index order, then the lanes are added in a fixed tree.
__global__ __launch_bounds__(FRO_THREADS) void k_bg_penalty_reduce(const double* __restrict__ partials, int T, float lambda_rgb, float lambda_alpha,
                                                                   float* __restrict__ out4, float* __restrict__ saved2)
{
	__shared__ double s_rows[3];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	if (wave < 3)
	{
		const double s = frb_row_sum(partials + (size_t)wave * T, T);
		if (lane == 0) s_rows[wave] = s;
	}
	__syncthreads();
	if (tid == 0) fro_penalty_finish(s_rows[0], s_rows[1], s_rows[2], lambda_rgb, lambda_alpha, out4, saved2);
}

__global__ __launch_bounds__(FRO_THREADS) void k_bg_penalty_backward(FroPenaltyArgs a, const float* __restrict__ saved2, const float* __restrict__ upstream,
                                                                     float* __restrict__ dL_dim, float* __restrict__ dL_dds)
{
	const uint32_t p = blockIdx.x * (uint32_t)FRO_THREADS + threadIdx.x;
	if (p >= a.n) return;
	const float up = upstream[0];
	const float f_rgb = fro_grad_factor(up, a.lambda_rgb, saved2[0]), f_alpha = fro_grad_factor(up, a.lambda_alpha, saved2[1]);
	const float bg = fro_background(a.obj[p]);
	for (int c = 0; c < 3; c++) dL_dim[(size_t)c * a.n + p] = fro_rgb_grad(f_rgb, bg, a.im[(size_t)c * a.n + p]);
	dL_dds[p] = 0.0f;
	dL_dds[(size_t)a.n + p] = fro_alpha_grad(f_alpha, bg, a.depth_sil[(size_t)a.n + p]);
	dL_dds[2 * (size_t)a.n + p] = 0.0f;
}

// ---- outside mask ----------------------------------------------------------------------------------------------------------------

struct FroOutsideArgs {
	const float* means;          // [P,3]
	const float* logs;           // [P,cols]
	const float* w2c;            // [4,4]
	const float* intr;           // [3,3]
	const uint8_t* obj;          // [H,W]
	int P, cols, H, W;
	uint8_t* outside;            // [P]
	uint32_t* parts;             // [workgroups][8]
};

// the eight words of a set pair: counts and NaN counts are added, the keys of the extreme log scales take min / max
__device__ __forceinline__ uint32_t fro_join(int j, uint32_t a, uint32_t b)
{
	return j < 4 ? a + b : ((j & 1) ? (a > b ? a : b) : (a < b ? a : b));
}

// v[8] over the workgroup (shuffles, then the four waves through LDS); valid in thread 0
__device__ __forceinline__ void fro_reduce8(uint32_t* v, uint32_t (*s_red)[FRO_THREADS / 64])
{
	const int tid = threadIdx.x;
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
#pragma unroll
		for (int j = 0; j < 8; j++) v[j] = fro_join(j, v[j], (uint32_t)__shfl_down(v[j], o, 64));
	if ((tid & 63) == 0)
		for (int j = 0; j < 8; j++) s_red[j][tid >> 6] = v[j];
	__syncthreads();
	if (tid == 0)
		for (int j = 0; j < 8; j++) v[j] = fro_join(j, fro_join(j, fro_join(j, s_red[j][0], s_red[j][1]), s_red[j][2]), s_red[j][3]);
}

__device__ __forceinline__ void fro_empty8(uint32_t* v)
{
	v[0] = 0u; v[1] = 0u; v[2] = 0u; v[3] = 0u;
	v[4] = 0xffffffffu; v[5] = 0u; v[6] = 0xffffffffu; v[7] = 0u;
}

__global__ __launch_bounds__(FRO_THREADS) void k_outside_mask(FroOutsideArgs a)
{
	__shared__ float s_m[16], s_k[9];
	__shared__ uint32_t s_red[8][FRO_THREADS / 64];
	const int tid = threadIdx.x;
	if (tid < 16) s_m[tid] = a.w2c[tid];
	if (tid >= 64 && tid < 73) s_k[tid - 64] = a.intr[tid - 64];
	__syncthreads();
	uint32_t v[8];
	fro_empty8(v);
	const long long base = (long long)blockIdx.x * (FRO_THREADS * FRO_SUM_ITEMS);
#pragma unroll
	for (int k = 0; k < FRO_SUM_ITEMS; k++)
	{
		const long long i = base + k * FRO_THREADS + tid;
		if (i >= a.P) continue;
		int iu, iv;
		const float* m = a.means + 3 * (size_t)i;
		const bool in_img = fro_project(s_m, s_k, m[0], m[1], m[2], a.W, a.H, iu, iv);
		const bool inside = in_img && a.obj[(size_t)iv * a.W + iu] != 0;       // (iu, iv) is clamped to the image
		a.outside[i] = inside ? 0 : 1;
		const float ls = fro_row_log_scale(a.logs + (size_t)i * a.cols, a.cols);
		const int s = inside ? 0 : 1;
		v[s] += 1u;
		if (ls != ls) v[2 + s] += 1u;
		else
		{
			const uint32_t key = fro_order_key(ls);
			v[4 + 2 * s] = key < v[4 + 2 * s] ? key : v[4 + 2 * s];
			v[5 + 2 * s] = key > v[5 + 2 * s] ? key : v[5 + 2 * s];
		}
	}
	fro_reduce8(v, s_red);
	if (tid == 0)
		for (int j = 0; j < 8; j++) a.parts[(size_t)blockIdx.x * 8 + j] = v[j];
}

__global__ __launch_bounds__(FRO_THREADS) void k_outside_finish(const uint32_t* __restrict__ parts, int nwg, int32_t* __restrict__ status)
{
	__shared__ uint32_t s_red[8][FRO_THREADS / 64];
	uint32_t v[8];
	fro_empty8(v);
	for (int w = threadIdx.x; w < nwg; w += FRO_THREADS)
		for (int j = 0; j < 8; j++) v[j] = fro_join(j, v[j], parts[(size_t)w * 8 + j]);
	fro_reduce8(v, s_red);
	if (threadIdx.x != 0) return;
	uint32_t r[4];
	fro_range_bits(v[0], v[2], v[4], v[5], &r[0], &r[1]);
	fro_range_bits(v[1], v[3], v[6], v[7], &r[2], &r[3]);
	status[0] = (int32_t)v[0]; status[1] = (int32_t)v[1];
	for (int j = 0; j < 4; j++) status[2 + j] = (int32_t)r[j];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

extern "C" size_t fr_loss_mask_workspace_bytes(int32_t H, int32_t W)
{
	return fr_image_ok(H, W) ? (size_t)FRO_HEAD_BYTES : 0;
}

extern "C" int fr_loss_mask(const fr_loss_mask_cfg* cfg, const float* depth_sil, const float* gt_depth, const uint8_t* obj_mask,
                            uint8_t* mask, int32_t* status, void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	if (!cfg) return fr_fail(FR_EINVAL, "fr_loss_mask: null cfg");
	if (!fr_image_ok(cfg->H, cfg->W)) return fr_fail(FR_EINVAL, "fr_loss_mask: bad argument (cfg: H, W; H W at most 2^30)");
	if (!depth_sil || !gt_depth || !mask || !status) return fr_fail(FR_EINVAL, "fr_loss_mask: null pointer (depth_sil, gt_depth, mask, status)");
	if (cfg->reject_outliers)
	{
		if (!workspace || workspace_bytes < FRO_HEAD_BYTES) return fr_fail(FR_ENOSPACE, "fr_loss_mask: workspace too small (fr_loss_mask_workspace_bytes)");
		if ((uintptr_t)workspace % 8) return fr_fail(FR_EINVAL, "fr_loss_mask: bad argument (workspace must be 8-byte aligned)");
	}
	FroMaskArgs a;
	a.depth_sil = depth_sil; a.gt = gt_depth; a.obj = obj_mask;
	a.n = (uint32_t)((int64_t)cfg->H * cfg->W);
	a.reject = cfg->reject_outliers != 0; a.presence = cfg->need_presence != 0;
	a.sil_thres = cfg->sil_thres; a.ratio = cfg->outlier_ratio;
	a.hist = (uint32_t*)workspace; a.mask = mask; a.status = status;
	hipStream_t s = (hipStream_t)stream;
	const dim3 block(FRO_THREADS);
	if (hipMemsetAsync(status, 0, FR_LOSS_MASK_STATUS_WORDS * sizeof(int32_t), s) != hipSuccess)
		return fr_fail(FR_ELAUNCH, "fr_loss_mask: hipMemsetAsync failed");
	int rc;
	if (a.reject)
	{
		if (hipMemsetAsync(workspace, 0, FRO_HEAD_BYTES, s) != hipSuccess) return fr_fail(FR_ELAUNCH, "fr_loss_mask: hipMemsetAsync failed");
		const uint32_t per = FRO_THREADS * FRO_HIST_ITEMS;
		const dim3 hgrid((a.n + per - 1) / per);
		hipLaunchKernelGGL(k_objloss_hist<0>, hgrid, block, 0, s, a);
		hipLaunchKernelGGL(k_objloss_hist<1>, hgrid, block, 0, s, a);
		hipLaunchKernelGGL(k_objloss_hist<2>, hgrid, block, 0, s, a);
		hipLaunchKernelGGL(k_objloss_hist<3>, hgrid, block, 0, s, a);
		if ((rc = fr_check_launch("k_objloss_hist"))) return rc;
	}
	hipLaunchKernelGGL(k_objloss_mask, dim3((a.n + FRO_THREADS - 1) / FRO_THREADS), block, 0, s, a);
	return fr_check_launch("k_objloss_mask");
}

static int fro_penalty_tiles(int32_t H, int32_t W)
{
	const int64_t n = (int64_t)H * W, per = FRO_THREADS * FRO_SUM_ITEMS;
	return (int)((n + per - 1) / per);
}

extern "C" size_t fr_bg_penalty_workspace_bytes(int32_t H, int32_t W)
{
	return fr_image_ok(H, W) ? (size_t)3 * fro_penalty_tiles(H, W) * sizeof(double) : 0;
}

static FroPenaltyArgs fro_penalty_args(int32_t H, int32_t W, float lambda_rgb, float lambda_alpha, const float* im, const float* depth_sil,
                                       const uint8_t* obj)
{
	FroPenaltyArgs a;
	a.im = im; a.depth_sil = depth_sil; a.obj = obj;
	a.n = (uint32_t)((int64_t)H * W); a.T = fro_penalty_tiles(H, W);
	a.lambda_rgb = lambda_rgb; a.lambda_alpha = lambda_alpha;
	return a;
}

extern "C" int fr_bg_penalty_forward(int32_t H, int32_t W, float lambda_rgb, float lambda_alpha, const float* im, const float* depth_sil,
                                     const uint8_t* obj_mask, float* out4, float* saved2, void* workspace, size_t workspace_bytes,
                                     fr_stream_t stream)
{
	if (!fr_image_ok(H, W)) return fr_fail(FR_EINVAL, "fr_bg_penalty_forward: bad argument (H, W; H W at most 2^30)");
	if (!im || !depth_sil || !obj_mask || !out4 || !saved2)
		return fr_fail(FR_EINVAL, "fr_bg_penalty_forward: null pointer (im, depth_sil, obj_mask, out4, saved2)");
	if (!workspace || workspace_bytes < fr_bg_penalty_workspace_bytes(H, W))
		return fr_fail(FR_ENOSPACE, "fr_bg_penalty_forward: workspace too small (fr_bg_penalty_workspace_bytes)");
	if ((uintptr_t)workspace % sizeof(double)) return fr_fail(FR_EINVAL, "fr_bg_penalty_forward: bad argument (workspace must be 8-byte aligned)");
	const FroPenaltyArgs a = fro_penalty_args(H, W, lambda_rgb, lambda_alpha, im, depth_sil, obj_mask);
	hipStream_t s = (hipStream_t)stream;
	hipLaunchKernelGGL(k_bg_penalty_partials, dim3(a.T), dim3(FRO_THREADS), 0, s, a, (double*)workspace);
	int rc;
	if ((rc = fr_check_launch("k_bg_penalty_partials"))) return rc;
	hipLaunchKernelGGL(k_bg_penalty_reduce, dim3(1), dim3(FRO_THREADS), 0, s, (const double*)workspace, a.T, lambda_rgb, lambda_alpha, out4, saved2);
	return fr_check_launch("k_bg_penalty_reduce");
}

extern "C" int fr_bg_penalty_backward(int32_t H, int32_t W, float lambda_rgb, float lambda_alpha, const float* im, const float* depth_sil,
                                      const uint8_t* obj_mask, const float* saved2, const float* upstream, float* dL_dim,
                                      float* dL_ddepth_sil, fr_stream_t stream)
{
	if (!fr_image_ok(H, W)) return fr_fail(FR_EINVAL, "fr_bg_penalty_backward: bad argument (H, W; H W at most 2^30)");
	if (!im || !depth_sil || !obj_mask || !saved2 || !upstream || !dL_dim || !dL_ddepth_sil)
		return fr_fail(FR_EINVAL, "fr_bg_penalty_backward: null pointer (im, depth_sil, obj_mask, saved2, upstream, dL_dim, dL_ddepth_sil)");
	const FroPenaltyArgs a = fro_penalty_args(H, W, lambda_rgb, lambda_alpha, im, depth_sil, obj_mask);
	hipLaunchKernelGGL(k_bg_penalty_backward, dim3((a.n + FRO_THREADS - 1) / FRO_THREADS), dim3(FRO_THREADS), 0, (hipStream_t)stream, a, saved2,
	                   upstream, dL_dim, dL_ddepth_sil);
	return fr_check_launch("k_bg_penalty_backward");
}

static int fro_outside_groups(int32_t P) { return (int)(((int64_t)P + FRO_THREADS * FRO_SUM_ITEMS - 1) / (FRO_THREADS * FRO_SUM_ITEMS)); }

extern "C" size_t fr_outside_mask_workspace_bytes(int32_t P)
{
	if (P < 0) return 0;
	const size_t words = (size_t)8 * fro_outside_groups(P);
	return (words > 8 ? words : 8) * sizeof(uint32_t);
}

extern "C" int fr_outside_mask(int32_t P, int32_t scale_cols, const float* means3D, const float* log_scales, const float* w2c,
                               const float* intrinsics, const uint8_t* obj_mask, int32_t H, int32_t W, uint8_t* outside, int32_t* status,
                               void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	if (P < 0 || (scale_cols != 1 && scale_cols != 3)) return fr_fail(FR_EINVAL, "fr_outside_mask: bad argument (P, scale_cols is 1 or 3)");
	if (!fr_image_ok(H, W)) return fr_fail(FR_EINVAL, "fr_outside_mask: bad argument (H, W; H W at most 2^30)");
	if (!w2c || !intrinsics || !obj_mask || !status) return fr_fail(FR_EINVAL, "fr_outside_mask: null pointer (w2c, intrinsics, obj_mask, status)");
	if (P > 0 && (!means3D || !log_scales || !outside)) return fr_fail(FR_EINVAL, "fr_outside_mask: null pointer (means3D, log_scales, outside)");
	if (!workspace || workspace_bytes < fr_outside_mask_workspace_bytes(P))
		return fr_fail(FR_ENOSPACE, "fr_outside_mask: workspace too small (fr_outside_mask_workspace_bytes)");
	if ((uintptr_t)workspace % 8) return fr_fail(FR_EINVAL, "fr_outside_mask: bad argument (workspace must be 8-byte aligned)");
	FroOutsideArgs a;
	a.means = means3D; a.logs = log_scales; a.w2c = w2c; a.intr = intrinsics; a.obj = obj_mask;
	a.P = P; a.cols = scale_cols; a.H = H; a.W = W;
	a.outside = outside; a.parts = (uint32_t*)workspace;
	hipStream_t s = (hipStream_t)stream;
	const int nwg = fro_outside_groups(P);
	int rc;
	if (nwg > 0)
	{
		hipLaunchKernelGGL(k_outside_mask, dim3(nwg), dim3(FRO_THREADS), 0, s, a);
		if ((rc = fr_check_launch("k_outside_mask"))) return rc;
	}
	hipLaunchKernelGGL(k_outside_finish, dim3(1), dim3(FRO_THREADS), 0, s, (const uint32_t*)workspace, nwg, status);
	return fr_check_launch("k_outside_finish");
}
