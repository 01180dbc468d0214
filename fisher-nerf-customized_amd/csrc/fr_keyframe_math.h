// fr_keyframe_math.h -- the arithmetic of the keyframe overlap (fr_keyframe.hip), host/device-neutral: the kernels and the g++ harness
// (tests/harness/fr_keyframe_harness.cpp) compile these same functions, so a CPU run states the kernels' results bit for bit.
//
// The statement is the reference's get_pointcloud / keyframe_selection_overlap (models/SLAM/utils/keyframe_selection.py:10-37,
// 40-134).  Everything is binary32, one rounding per written operation (the build has -ffp-contract=off and an IEEE divide), and
// every operand order is the one written here.  The back-projection and the affine inverse are the frame ingest's
// (fri_back_project, fri_invert_affine): (col - cx) / fx * z, then the rows of the inverse of w2c.
//
// Non-finite inputs: this header is the statement.  No parity with torch is claimed for them.
#ifndef FR_KEYFRAME_MATH_H_INCLUDED
#define FR_KEYFRAME_MATH_H_INCLUDED

#include "fr_ingest_math.h"

#define FRK_HD FRI_HD

// keyframe_selection.py:28: |round(p, decimals=4)|, per coordinate.  nearbyintf rounds halves to even, as torch.round does
// (the rounding mode is never changed); the scaling by 1e4 and back are one multiplication and one division.
FRK_HD float frk_key(float p) { return fabsf(nearbyintf(p * 1e4f) / 1e4f); }

FRK_HD void frk_keys(const float* p, float* k) { k[0] = frk_key(p[0]); k[1] = frk_key(p[1]); k[2] = frk_key(p[2]); }

// two points are the same to the reference's unique() when their three keys are equal as floats -- so (x, y, z) and (-x, y, z) are
FRK_HD bool frk_same_key(const float* a, const float* b) { return (a[0] == b[0]) & (a[1] == b[1]) & (a[2] == b[2]); }

// keyframe_selection.py:29: the row of zeros that is appended before unique() -- a point whose keys are all 0 is never alone
FRK_HD bool frk_origin_key(const float* k) { return (k[0] == 0.0f) & (k[1] == 0.0f) & (k[2] == 0.0f); }

// keyframe_selection.py:80-94: the world point p in the camera of a keyframe (w = est_w2c, row-major 4 x 4, rows 0..2 used), through the
// full 3 x 3 intrinsics, divided by z + 1e-5; inside the image by more than `edge` pixels and in front of the camera.  (u, v) are
// returned for the mask look-up.
FRK_HD bool frk_project_inside(const float* w, const float* intr, const float* p, int H, int W, int edge, float* u, float* v)
{
	float c[3], q[3];
	for (int r = 0; r < 3; r++) c[r] = ((w[4 * r + 0] * p[0] + w[4 * r + 1] * p[1]) + w[4 * r + 2] * p[2]) + w[4 * r + 3];
	for (int r = 0; r < 3; r++) q[r] = (intr[3 * r + 0] * c[0] + intr[3 * r + 1] * c[1]) + intr[3 * r + 2] * c[2];
	const float z = q[2] + 1e-5f;
	*u = q[0] / z;
	*v = q[1] / z;
	return (*u < (float)(W - edge)) & (*u > (float)edge) & (*v < (float)(H - edge)) & (*v > (float)edge) & (z > 0.0f);
}

// keyframe_selection.py:112-114: mask[clamp(round(v), 0, H - 1)][clamp(round(u), 0, W - 1)] != 0, for a point that is inside (u and v are
// finite and within [edge, W - edge] x [edge, H - edge] there; the clamp is taken in floats, before the conversion, all the same)
FRK_HD bool frk_mask_hit(const uint8_t* mask, int H, int W, float u, float v)
{
	const float ru = fminf(fmaxf(nearbyintf(u), 0.0f), (float)(W - 1)), rv = fminf(fmaxf(nearbyintf(v), 0.0f), (float)(H - 1));
	return mask[(size_t)(int)rv * (size_t)W + (size_t)(int)ru] != 0;
}

#endif
