// fr_rendervar_math.h -- the arithmetic of the fused render-variable build (fr_rendervar.hip), host/device-neutral: the kernels and
// the g++ harness (tests/harness/fr_rendervar_harness.cpp) compile these same functions, so a CPU run states the kernels' per-Gaussian
// results bit for bit.
//
// The statement is the stretch between `params` and the rasteriser of one tracking / mapping iteration: transform_to_frame
// (models/SLAM/utils/slam_helpers.py:282-317 over build_rotation, slam_external.py:25-42), get_depth_and_silhouette and
// transformed_params2rendervar (slam_helpers.py:178-188, 235-252, 268-279), forward and backward.  Everything is binary32, one
// rounding per written operation (the build has -ffp-contract=off and an IEEE divide / sqrt), every operand order is the one written
// here, and the only contraction is inside fr_expf (fr_math.h).  torch's matmul and vector_norm leave their operand order open: its
// last bits are not reproduced and are not meant to be.
//
// NaN and infinity travel as they do in the torch chain: the norm clamp lets a NaN norm through (torch's clamp_min does), a zero
// camera quaternion gives a NaN pose (the second normalisation is 0 / 0), exp overflows to infinity.
#ifndef FR_RENDERVAR_MATH_H_INCLUDED
#define FR_RENDERVAR_MATH_H_INCLUDED

#include "fr_math.h"

#define FRV_NORM_EPS 1e-12f            // F.normalize's eps

// max(n, eps) as torch's clamp_min has it: a NaN norm stays NaN
FR_HD float frv_clamp_norm(float n) { return n < FRV_NORM_EPS ? FRV_NORM_EPS : n; }

FR_HD float frv_norm4(const float* v) { return sqrtf(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3]); }

FR_HD float frv_dot4(const float* a, const float* b) { return ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3]; }

// The frame's pose: a = cq / max(|cq|, eps) (F.normalize), q = a / |a| (build_rotation normalises again), R the nine entries of
// build_rotation as written there, row-major.  n1, d1, n2 are kept for the way back.
struct frv_pose { float a[4], q[4], n1, d1, n2, R[9], t[3]; };

FR_HD void frv_pose_forward(const float* cq, const float* ct, frv_pose& p)
{
	p.n1 = frv_norm4(cq);
	p.d1 = frv_clamp_norm(p.n1);
	for (int k = 0; k < 4; k++) p.a[k] = cq[k] / p.d1;
	p.n2 = frv_norm4(p.a);
	for (int k = 0; k < 4; k++) p.q[k] = p.a[k] / p.n2;
	const float r = p.q[0], x = p.q[1], y = p.q[2], z = p.q[3];
	p.R[0] = 1.0f - 2.0f * (y * y + z * z);
	p.R[1] = 2.0f * (x * y - r * z);
	p.R[2] = 2.0f * (x * z + r * y);
	p.R[3] = 2.0f * (x * y + r * z);
	p.R[4] = 1.0f - 2.0f * (x * x + z * z);
	p.R[5] = 2.0f * (y * z - r * x);
	p.R[6] = 2.0f * (x * z - r * y);
	p.R[7] = 2.0f * (y * z + r * x);
	p.R[8] = 1.0f - 2.0f * (x * x + y * y);
	for (int k = 0; k < 3; k++) p.t[k] = ct[k];
}

// rel_w2c [4,4] row-major: eye(4) with R and t set
FR_HD void frv_pose_matrix(const frv_pose& p, float* m)
{
	for (int i = 0; i < 3; i++)
	{
		for (int j = 0; j < 3; j++) m[4 * i + j] = p.R[3 * i + j];
		m[4 * i + 3] = p.t[i];
	}
	m[12] = 0.0f; m[13] = 0.0f; m[14] = 0.0f; m[15] = 1.0f;
}

// pts = R m + t
FR_HD void frv_point(const frv_pose& p, const float* m, float* pts)
{
	for (int i = 0; i < 3; i++) pts[i] = ((p.R[3 * i] * m[0] + p.R[3 * i + 1] * m[1]) + p.R[3 * i + 2] * m[2]) + p.t[i];
}

// the depth in the first frame: w = row 2 of first_frame_w2c
FR_HD float frv_depth(const float* w, const float* pts) { return ((w[0] * pts[0] + w[1] * pts[1]) + w[2] * pts[2]) + w[3]; }

// rot = q / max(|q|, eps); returns the norm
FR_HD float frv_normalize4(const float* q, float* rot)
{
	const float n = frv_norm4(q), d = frv_clamp_norm(n);
	for (int k = 0; k < 4; k++) rot[k] = q[k] / d;
	return n;
}

FR_HD float frv_sigmoid(float logit) { return 1.0f / (1.0f + fr_expf(-logit)); }

// ---- the way back ----------------------------------------------------------------------------------------------------------------

// G = g_pts + w[0:3] (g_feats0 + 2 zc g_feats2); a null pointer is a part that is absent (not a zero that is added)
FR_HD void frv_point_grad(const float* g_pts, const float* g_feats, const float* w, float zc, float* G)
{
	if (g_feats)
	{
		const float s = g_feats[0] + (2.0f * zc) * g_feats[2];
		for (int j = 0; j < 3; j++) G[j] = g_pts ? g_pts[j] + w[j] * s : w[j] * s;
	}
	else
		for (int j = 0; j < 3; j++) G[j] = g_pts ? g_pts[j] : 0.0f;
}

// g_means = R^T G
FR_HD void frv_means_grad(const frv_pose& p, const float* G, float* g)
{
	for (int j = 0; j < 3; j++) g[j] = (p.R[j] * G[0] + p.R[3 + j] * G[1]) + p.R[6 + j] * G[2];
}

// F.normalize's gradient: (g - rot (rot . g)) / |q|, and g / eps where the norm is below the clamp
FR_HD void frv_normalize4_grad(const float* q, const float* g, float* out)
{
	float rot[4];
	const float n = frv_normalize4(q, rot), d = frv_clamp_norm(n);
	if (n < FRV_NORM_EPS)
	{
		for (int k = 0; k < 4; k++) out[k] = g[k] / d;
		return;
	}
	const float dot = frv_dot4(rot, g);
	for (int k = 0; k < 4; k++) out[k] = (g[k] - rot[k] * dot) / d;
}

FR_HD float frv_sigmoid_grad(float g, float opac) { return (g * opac) * (1.0f - opac); }

// The camera's tail: dR[9] = sum G (x) m (row-major, the gradient of R), dt[3] = sum G  ->  the gradients of the frame's unnormalised
// quaternion and translation, through build_rotation's entries and both normalisations.
FR_HD void frv_pose_backward(const frv_pose& p, const float* dR, const float* dt, float* g_cq, float* g_ct)
{
	const float r = p.q[0], x = p.q[1], y = p.q[2], z = p.q[3];
	float dq[4], da[4];
	dq[0] = 2.0f * ((x * (dR[7] - dR[5]) + y * (dR[2] - dR[6])) + z * (dR[3] - dR[1]));
	dq[1] = 2.0f * (((y * (dR[1] + dR[3]) + z * (dR[2] + dR[6])) + r * (dR[7] - dR[5])) - (2.0f * x) * (dR[4] + dR[8]));
	dq[2] = 2.0f * (((x * (dR[1] + dR[3]) + z * (dR[5] + dR[7])) + r * (dR[2] - dR[6])) - (2.0f * y) * (dR[0] + dR[8]));
	dq[3] = 2.0f * (((x * (dR[2] + dR[6]) + y * (dR[5] + dR[7])) + r * (dR[3] - dR[1])) - (2.0f * z) * (dR[0] + dR[4]));
	const float dotq = frv_dot4(p.q, dq);
	for (int k = 0; k < 4; k++) da[k] = (dq[k] - p.q[k] * dotq) / p.n2;
	if (p.n1 < FRV_NORM_EPS)
		for (int k = 0; k < 4; k++) g_cq[k] = da[k] / p.d1;
	else
	{
		const float dota = frv_dot4(p.a, da);
		for (int k = 0; k < 4; k++) g_cq[k] = (da[k] - p.a[k] * dota) / p.d1;
	}
	for (int k = 0; k < 3; k++) g_ct[k] = dt[k];
}

#endif
