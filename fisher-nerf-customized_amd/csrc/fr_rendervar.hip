// fr_rendervar.hip -- the fused render-variable build of libfisher_rast.so (gfx950, wave64): fr_rendervar_forward /
// fr_rendervar_backward.
//
// The stretch between `params` and the rasteriser of a tracking / mapping iteration is, in the reference, a chain of torch
// element-wise ops (transform_to_frame, get_depth_and_silhouette, transformed_params2rendervar: models/SLAM/utils/slam_helpers.py)
// that autograd then runs backwards -- in tracking with a reduction over all Gaussians down to seven numbers.  Here:
//
//   k_rendervar_forward    one launch, grid-stride over the rows with a capped grid.  Thread 0 of every workgroup computes the
//                          frame's pose (two normalisations, build_rotation) into LDS; a thread does a row: the camera-frame
//                          point, the (z, 1, z^2) features, the normalised rotation, the opacity, the scales -- whatever is asked for.
//   k_rendervar_backward   one launch, the same shape.  A row's forward is recomputed from the inputs (nothing is saved), its
//                          gradients written.  With a camera gradient every thread also keeps the twelve sums dR = sum G (x) m,
//                          dt = sum G over its rows; they are reduced in the wave by shuffles, across the workgroup's waves
//                          through LDS in wave order, and stored as the workgroup's row of the workspace.
//   k_rendervar_camera     one workgroup: adds the rows in the same fixed order, runs frv_pose_backward, writes the [4,T] / [3,T]
//                          gradients whole (zero outside the frame).
//
// No atomics and no election of a last workgroup: the camera gradient has the same bits on every call.  Rows are 12 or 16 bytes and
// only 4-byte alignment is assumed, so a row moves as 4-byte words.  fr_rendervar_math.h is the arithmetic.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "fr_internal.h"
#include "fr_rendervar_math.h"

#define FRV_THREADS 256
#define FRV_MAX_GRID 2048            // streaming kernels: about 8 workgroups per CU, the rest is grid-strided
#define FRV_SUMS 12                  // dR[9], dt[3]
#define FRV_WAVES (FRV_THREADS / 64)

static unsigned frv_grid(int32_t P)
{
	const unsigned blocks = ((unsigned)P + FRV_THREADS - 1) / FRV_THREADS;
	return blocks < FRV_MAX_GRID ? blocks : FRV_MAX_GRID;
}

// the pose of frame time_idx (and row 2 of first_frame_w2c) into LDS, by thread 0; every thread returns with them readable
__device__ __forceinline__ void frv_stage_pose(const fr_rendervar_cfg& c, frv_pose* pose, float* w)
{
	if (threadIdx.x == 0)
	{
		if (c.cam_unnorm_rots && c.cam_trans)
		{
			float cq[4], ct[3];
			for (int k = 0; k < 4; k++) cq[k] = c.cam_unnorm_rots[(size_t)k * c.n_frames + c.time_idx];
			for (int k = 0; k < 3; k++) ct[k] = c.cam_trans[(size_t)k * c.n_frames + c.time_idx];
			frv_pose_forward(cq, ct, *pose);
		}
		for (int k = 0; k < 4; k++) w[k] = c.first_frame_w2c ? c.first_frame_w2c[8 + k] : 0.0f;
	}
	__syncthreads();
}

__global__ __launch_bounds__(FRV_THREADS) void k_rendervar_forward(fr_rendervar_cfg c)
{
	__shared__ frv_pose s_pose;
	__shared__ float s_w[4];
	frv_stage_pose(c, &s_pose, s_w);
	if (c.rel_w2c && blockIdx.x == 0 && threadIdx.x == 0)
	{
		float m[16];
		frv_pose_matrix(s_pose, m);
		for (int k = 0; k < 16; k++) c.rel_w2c[k] = m[k];
	}
	const frv_pose pose = s_pose;
	const float w[4] = {s_w[0], s_w[1], s_w[2], s_w[3]};
	const size_t P = (size_t)c.P, stride = (size_t)gridDim.x * FRV_THREADS;
	for (size_t i = (size_t)blockIdx.x * FRV_THREADS + threadIdx.x; i < P; i += stride)
	{
		if (c.pts || c.feats)
		{
			const float m[3] = {c.means3D[3 * i], c.means3D[3 * i + 1], c.means3D[3 * i + 2]};
			float pts[3];
			frv_point(pose, m, pts);
			if (c.pts) { c.pts[3 * i] = pts[0]; c.pts[3 * i + 1] = pts[1]; c.pts[3 * i + 2] = pts[2]; }
			if (c.feats)
			{
				const float zc = frv_depth(w, pts);
				c.feats[3 * i] = zc; c.feats[3 * i + 1] = 1.0f; c.feats[3 * i + 2] = zc * zc;
			}
		}
		if (c.rotations)
		{
			const float q[4] = {c.unnorm_rotations[4 * i], c.unnorm_rotations[4 * i + 1], c.unnorm_rotations[4 * i + 2], c.unnorm_rotations[4 * i + 3]};
			float rot[4];
			frv_normalize4(q, rot);
			for (int k = 0; k < 4; k++) c.rotations[4 * i + k] = rot[k];
		}
		if (c.opacities) c.opacities[i] = frv_sigmoid(c.logit_opacities[i]);
		if (c.scales)
		{
			if (c.scale_cols == 1)
			{
				const float s = fr_expf(c.log_scales[i]);
				c.scales[3 * i] = s; c.scales[3 * i + 1] = s; c.scales[3 * i + 2] = s;
			}
			else
				for (int k = 0; k < 3; k++) c.scales[3 * i + k] = fr_expf(c.log_scales[3 * i + k]);
		}
	}
}

// v[0..11] summed over the workgroup in a fixed order: the wave by shuffles (a halving tree), the waves in wave order through LDS.
// Threads 0 .. 11 return the sum of their column (the others garbage).
__device__ __forceinline__ float frv_block_sums(float* v, float (*s_part)[FRV_SUMS])
{
	for (int k = 0; k < FRV_SUMS; k++)
		for (int off = 32; off > 0; off >>= 1) v[k] = v[k] + __shfl_down(v[k], off, 64);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (lane == 0)
		for (int k = 0; k < FRV_SUMS; k++) s_part[wave][k] = v[k];
	__syncthreads();
	float total = 0.0f;
	if (threadIdx.x < FRV_SUMS)
	{
		total = s_part[0][threadIdx.x];
		for (int wv = 1; wv < FRV_WAVES; wv++) total = total + s_part[wv][threadIdx.x];
	}
	return total;
}

// partials [gridDim.x][FRV_SUMS]: null without a camera gradient
__global__ __launch_bounds__(FRV_THREADS) void k_rendervar_backward(fr_rendervar_cfg c, float* partials)
{
	__shared__ frv_pose s_pose;
	__shared__ float s_w[4];
	__shared__ float s_part[FRV_WAVES][FRV_SUMS];
	frv_stage_pose(c, &s_pose, s_w);
	const frv_pose pose = s_pose;
	const float w[4] = {s_w[0], s_w[1], s_w[2], s_w[3]};
	const bool point_path = c.g_means3D || partials;
	float acc[FRV_SUMS];
	for (int k = 0; k < FRV_SUMS; k++) acc[k] = 0.0f;
	const size_t P = (size_t)c.P, stride = (size_t)gridDim.x * FRV_THREADS;
	for (size_t i = (size_t)blockIdx.x * FRV_THREADS + threadIdx.x; i < P; i += stride)
	{
		if (point_path)
		{
			const float m[3] = {c.means3D[3 * i], c.means3D[3 * i + 1], c.means3D[3 * i + 2]};
			float gp[3], gf[3], G[3], zc = 0.0f;
			if (c.g_pts) { gp[0] = c.g_pts[3 * i]; gp[1] = c.g_pts[3 * i + 1]; gp[2] = c.g_pts[3 * i + 2]; }
			if (c.g_feats)
			{
				float pts[3];
				frv_point(pose, m, pts);
				zc = frv_depth(w, pts);
				gf[0] = c.g_feats[3 * i]; gf[1] = c.g_feats[3 * i + 1]; gf[2] = c.g_feats[3 * i + 2];
			}
			frv_point_grad(c.g_pts ? gp : nullptr, c.g_feats ? gf : nullptr, w, zc, G);
			if (c.g_means3D)
			{
				float g[3];
				frv_means_grad(pose, G, g);
				c.g_means3D[3 * i] = g[0]; c.g_means3D[3 * i + 1] = g[1]; c.g_means3D[3 * i + 2] = g[2];
			}
			if (partials)
			{
				for (int a = 0; a < 3; a++)
				{
					for (int b = 0; b < 3; b++) acc[3 * a + b] = acc[3 * a + b] + G[a] * m[b];
					acc[9 + a] = acc[9 + a] + G[a];
				}
			}
		}
		if (c.g_unnorm_rotations)
		{
			float out[4] = {0.0f, 0.0f, 0.0f, 0.0f};           // a null incoming gradient is a zero gradient
			if (c.g_rotations)
			{
				float q[4], g[4];
				for (int k = 0; k < 4; k++) { q[k] = c.unnorm_rotations[4 * i + k]; g[k] = c.g_rotations[4 * i + k]; }
				frv_normalize4_grad(q, g, out);
			}
			for (int k = 0; k < 4; k++) c.g_unnorm_rotations[4 * i + k] = out[k];
		}
		if (c.g_logit_opacities) c.g_logit_opacities[i] = c.g_opacities ? frv_sigmoid_grad(c.g_opacities[i], frv_sigmoid(c.logit_opacities[i])) : 0.0f;
		if (c.g_log_scales)
		{
			if (!c.g_scales)
				for (int k = 0; k < c.scale_cols; k++) c.g_log_scales[(size_t)c.scale_cols * i + k] = 0.0f;
			else if (c.scale_cols == 1)
			{
				const float s = fr_expf(c.log_scales[i]);
				c.g_log_scales[i] = (c.g_scales[3 * i] * s + c.g_scales[3 * i + 1] * s) + c.g_scales[3 * i + 2] * s;
			}
			else
				for (int k = 0; k < 3; k++) c.g_log_scales[3 * i + k] = c.g_scales[3 * i + k] * fr_expf(c.log_scales[3 * i + k]);
		}
	}
	if (partials)                       // uniform over the launch
	{
		const float total = frv_block_sums(acc, s_part);
		if (threadIdx.x < FRV_SUMS) partials[(size_t)blockIdx.x * FRV_SUMS + threadIdx.x] = total;
	}
}

// one workgroup: the rows of partials added in a fixed order, the pose's way back, the [4,T] / [3,T] gradients written whole
__global__ __launch_bounds__(FRV_THREADS) void k_rendervar_camera(fr_rendervar_cfg c, const float* partials, int32_t rows)
{
	__shared__ frv_pose s_pose;
	__shared__ float s_w[4];
	__shared__ float s_part[FRV_WAVES][FRV_SUMS];
	__shared__ float s_sum[FRV_SUMS];
	__shared__ float s_out[7];
	frv_stage_pose(c, &s_pose, s_w);
	float acc[FRV_SUMS];
	for (int k = 0; k < FRV_SUMS; k++) acc[k] = 0.0f;
	for (int32_t r = threadIdx.x; r < rows; r += FRV_THREADS)
		for (int k = 0; k < FRV_SUMS; k++) acc[k] = acc[k] + partials[(size_t)r * FRV_SUMS + k];
	const float total = frv_block_sums(acc, s_part);
	if (threadIdx.x < FRV_SUMS) s_sum[threadIdx.x] = total;
	__syncthreads();
	if (threadIdx.x == 0)
	{
		float dR[9], dt[3], g_cq[4], g_ct[3];
		for (int k = 0; k < 9; k++) dR[k] = s_sum[k];
		for (int k = 0; k < 3; k++) dt[k] = s_sum[9 + k];
		frv_pose_backward(s_pose, dR, dt, g_cq, g_ct);
		for (int k = 0; k < 4; k++) s_out[k] = g_cq[k];
		for (int k = 0; k < 3; k++) s_out[4 + k] = g_ct[k];
	}
	__syncthreads();
	const int32_t T = c.n_frames;
	if (c.g_cam_unnorm_rots)
		for (int32_t e = threadIdx.x; e < 4 * T; e += FRV_THREADS) c.g_cam_unnorm_rots[e] = (e % T == c.time_idx) ? s_out[e / T] : 0.0f;
	if (c.g_cam_trans)
		for (int32_t e = threadIdx.x; e < 3 * T; e += FRV_THREADS) c.g_cam_trans[e] = (e % T == c.time_idx) ? s_out[4 + e / T] : 0.0f;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

static int frv_check_common(const fr_rendervar_cfg* c, const char* who, bool need_pose, bool need_w2c)
{
	static thread_local char msg[160];
	const char* why = nullptr;
	if (!c) why = "null pointer (cfg)";
	else if (c->P < 0) why = "bad argument (P is negative)";
	else if (c->scale_cols != 1 && c->scale_cols != 3) why = "bad argument (scale_cols is 1 or 3)";
	else if (need_pose && (c->n_frames <= 0 || c->n_frames > (1 << 26) || c->time_idx < 0 || c->time_idx >= c->n_frames)) why = "bad argument (time_idx is outside [0, n_frames))";
	else if (need_pose && (!c->cam_unnorm_rots || !c->cam_trans)) why = "null pointer (cam_unnorm_rots, cam_trans)";
	else if (need_w2c && !c->first_frame_w2c) why = "null pointer (first_frame_w2c)";
	else
	{
		const void* all[] = {c->cam_unnorm_rots, c->cam_trans, c->first_frame_w2c, c->means3D, c->unnorm_rotations, c->logit_opacities, c->log_scales,
		                     c->pts, c->feats, c->rotations, c->opacities, c->scales, c->rel_w2c, c->g_pts, c->g_feats, c->g_rotations, c->g_opacities,
		                     c->g_scales, c->g_means3D, c->g_unnorm_rotations, c->g_logit_opacities, c->g_log_scales, c->g_cam_unnorm_rots, c->g_cam_trans};
		uintptr_t bits = 0;
		for (const void* p : all) bits |= (uintptr_t)p;
		if (bits % 4) why = "bad argument (pointers must be 4-byte aligned)";
	}
	if (!why) return FR_OK;
	snprintf(msg, sizeof(msg), "%s: %s", who, why);
	return fr_fail(FR_EINVAL, msg);
}

extern "C" size_t fr_rendervar_workspace_bytes(int32_t P)
{
	return P > 0 ? (size_t)frv_grid(P) * FRV_SUMS * sizeof(float) : 0;
}

extern "C" int fr_rendervar_forward(const fr_rendervar_cfg* c, fr_stream_t stream)
{
	const bool point_path = c && (c->pts || c->feats);
	const int rc = frv_check_common(c, "fr_rendervar_forward", point_path || (c && c->rel_w2c), c && c->feats);
	if (rc != FR_OK) return rc;
	if (c->P > 0)
	{
		if (point_path && !c->means3D) return fr_fail(FR_EINVAL, "fr_rendervar_forward: null pointer (means3D)");
		if (c->rotations && !c->unnorm_rotations) return fr_fail(FR_EINVAL, "fr_rendervar_forward: null pointer (unnorm_rotations)");
		if (c->opacities && !c->logit_opacities) return fr_fail(FR_EINVAL, "fr_rendervar_forward: null pointer (logit_opacities)");
		if (c->scales && !c->log_scales) return fr_fail(FR_EINVAL, "fr_rendervar_forward: null pointer (log_scales)");
	}
	const bool rows = c->P > 0 && (point_path || c->rotations || c->opacities || c->scales);
	if (!rows && !c->rel_w2c) return FR_OK;
	const dim3 grid(rows ? frv_grid(c->P) : 1);
	hipLaunchKernelGGL(k_rendervar_forward, grid, dim3(FRV_THREADS), 0, (hipStream_t)stream, *c);
	return fr_check_launch("k_rendervar_forward");
}

extern "C" int fr_rendervar_backward(const fr_rendervar_cfg* c, void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	const bool camera = c && (c->g_cam_unnorm_rots || c->g_cam_trans);
	const bool point_path = c && (c->g_means3D || camera);
	const int rc = frv_check_common(c, "fr_rendervar_backward", point_path, c && point_path && c->g_feats);
	if (rc != FR_OK) return rc;
	if (c->P > 0)
	{
		if (point_path && !c->means3D) return fr_fail(FR_EINVAL, "fr_rendervar_backward: null pointer (means3D)");
		if (c->g_unnorm_rotations && c->g_rotations && !c->unnorm_rotations) return fr_fail(FR_EINVAL, "fr_rendervar_backward: null pointer (unnorm_rotations)");
		if (c->g_logit_opacities && c->g_opacities && !c->logit_opacities) return fr_fail(FR_EINVAL, "fr_rendervar_backward: null pointer (logit_opacities)");
		if (c->g_log_scales && c->g_scales && !c->log_scales) return fr_fail(FR_EINVAL, "fr_rendervar_backward: null pointer (log_scales)");
	}
	if (camera && c->P > 0)
	{
		if (workspace_bytes < fr_rendervar_workspace_bytes(c->P)) return fr_fail(FR_ENOSPACE, "fr_rendervar_backward: the workspace is smaller than fr_rendervar_workspace_bytes(P)");
		if (!workspace || (uintptr_t)workspace % 4) return fr_fail(FR_EINVAL, "fr_rendervar_backward: null pointer (workspace)");
	}
	if (c->P == 0)
	{
		// no row, nothing to launch: the camera gradients are zero
		if (c->g_cam_unnorm_rots && hipMemsetAsync(c->g_cam_unnorm_rots, 0, (size_t)4 * c->n_frames * sizeof(float), (hipStream_t)stream) != hipSuccess)
			return fr_fail(FR_ELAUNCH, "fr_rendervar_backward: hipMemsetAsync failed");
		if (c->g_cam_trans && hipMemsetAsync(c->g_cam_trans, 0, (size_t)3 * c->n_frames * sizeof(float), (hipStream_t)stream) != hipSuccess)
			return fr_fail(FR_ELAUNCH, "fr_rendervar_backward: hipMemsetAsync failed");
		return FR_OK;
	}
	if (!point_path && !c->g_unnorm_rotations && !c->g_logit_opacities && !c->g_log_scales) return FR_OK;
	const unsigned blocks = frv_grid(c->P);
	hipLaunchKernelGGL(k_rendervar_backward, dim3(blocks), dim3(FRV_THREADS), 0, (hipStream_t)stream, *c, camera ? (float*)workspace : (float*)nullptr);
	int launched = fr_check_launch("k_rendervar_backward");
	if (launched != FR_OK || !camera) return launched;
	hipLaunchKernelGGL(k_rendervar_camera, dim3(1), dim3(FRV_THREADS), 0, (hipStream_t)stream, *c, (const float*)workspace, (int32_t)blocks);
	return fr_check_launch("k_rendervar_camera");
}
