// fr_ingest_math.h -- the arithmetic of the frame ingest (fr_ingest.hip), host/device-neutral: the kernels and the g++ harness
// (tests/harness/fr_ingest_harness.cpp) compile these same functions, so a CPU run states the kernels' results bit for bit
// (all but logf, which is the platform's).
//
// The statement is the reference's add_new_gaussians / get_pointcloud / initialize_new_params
// (models/SLAM/gaussian.py:320-414, 75-143, 299-318).  Everything is binary32, one rounding per written operation (the build has
// -ffp-contract=off and an IEEE divide / sqrt), and every operand order is the one written here.
#ifndef FR_INGEST_MATH_H_INCLUDED
#define FR_INGEST_MATH_H_INCLUDED

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define FRI_HD __host__ __device__ __forceinline__
#else
#define FRI_HD inline
#endif

#define FRI_NAN_BITS 0x7fc00000u      /* the median of a frame that holds a NaN, whatever the NaN's own bits were */

FRI_HD uint32_t fri_bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
FRI_HD float fri_float(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }

// |gt - render| where a depth was measured, 0 elsewhere (gaussian.py:334).  The product is taken literally: an infinite or NaN
// difference times 0 is NaN, as torch's is.  Never negative, so the order of the bit patterns is the order of the values.
FRI_HD float fri_depth_error(float gt, float render)
{
	return fabsf(gt - render) * (gt > 0.0f ? 1.0f : 0.0f);
}

// gaussian.py:330-342: no silhouette here, or a surface in front of what the map renders by more than thr = ratio * median;
// and a depth worth a point at all.
FRI_HD bool fri_non_presence(float sil, float render, float gt, float thr, float sil_thres)
{
	const float err = fri_depth_error(gt, render);
	bool np = (sil < sil_thres) | ((render > gt) & (err > thr));
	np &= gt > 0.01f;
	return np;
}

FRI_HD float fri_threshold(float ratio, float median) { return ratio * median; }

// c2w [3][4] from the top 3 x 4 of w2c (row-major 4 x 4): the adjugate of the 3 x 3 over its determinant, then -A^-1 t.
// A general affine inverse -- the reference calls torch.inverse on whatever it was handed (gaussian.py:105).
FRI_HD void fri_invert_affine(const float* w, float* m)
{
	const float a00 = w[0], a01 = w[1], a02 = w[2], t0 = w[3];
	const float a10 = w[4], a11 = w[5], a12 = w[6], t1 = w[7];
	const float a20 = w[8], a21 = w[9], a22 = w[10], t2 = w[11];
	const float c00 = a11 * a22 - a12 * a21, c01 = a02 * a21 - a01 * a22, c02 = a01 * a12 - a02 * a11;
	const float c10 = a12 * a20 - a10 * a22, c11 = a00 * a22 - a02 * a20, c12 = a02 * a10 - a00 * a12;
	const float c20 = a10 * a21 - a11 * a20, c21 = a01 * a20 - a00 * a21, c22 = a00 * a11 - a01 * a10;
	const float det = (a00 * c00 + a01 * c10) + a02 * c20;
	const float i[9] = {c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det};
	for (int r = 0; r < 3; r++)
	{
		m[4 * r + 0] = i[3 * r + 0]; m[4 * r + 1] = i[3 * r + 1]; m[4 * r + 2] = i[3 * r + 2];
		m[4 * r + 3] = -((i[3 * r + 0] * t0 + i[3 * r + 1] * t1) + i[3 * r + 2] * t2);
	}
}

// gaussian.py:93-108: the pixel (x, y) at depth z in the camera frame, then in the world (m = c2w [3][4]; null: stays in the camera frame)
FRI_HD void fri_back_project(int x, int y, float z, float fx, float fy, float cx, float cy, const float* m, float* p)
{
	const float xx = ((float)x - cx) / fx, yy = ((float)y - cy) / fy;
	const float X = xx * z, Y = yy * z;
	if (!m) { p[0] = X; p[1] = Y; p[2] = z; return; }
	for (int r = 0; r < 3; r++) p[r] = ((m[4 * r + 0] * X + m[4 * r + 1] * Y) + m[4 * r + 2] * z) + m[4 * r + 3];
}

// gaussian.py:114-115: the projective radius of a pixel of a frame taken at one in `downsample`, squared
FRI_HD float fri_mean3_sq_dist(int downsample, float z, float fx, float fy)
{
	const float s = ((float)downsample * z) / ((fx + fy) / 2.0f);
	return s * s;
}

// gaussian.py:309
FRI_HD float fri_log_scale(float mean3_sq_dist) { return logf(sqrtf(mean3_sq_dist)); }

#endif
