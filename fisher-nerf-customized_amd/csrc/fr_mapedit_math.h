// fr_mapedit_math.h -- the arithmetic of the map edit (fr_mapedit.hip), host/device-neutral: the kernel and the g++ harness
// (tests/harness/fr_mapedit_harness.cpp) compile these same functions, so a CPU run states the kernel's results bit for bit
// (all but logf, which is the platform's).
//
// The statement is the split child of the reference's densify (models/SLAM/utils/slam_external.py:427-435) over its
// build_rotation (25-42).  Everything is binary32, one rounding per written operation (the build has -ffp-contract=off and an IEEE
// divide / sqrt), and every operand order is the one written here.  The normal samples z are an input.
#ifndef FR_MAPEDIT_MATH_H_INCLUDED
#define FR_MAPEDIT_MATH_H_INCLUDED

#include "fr_math.h"

#if defined(__HIPCC__)
#define FRM_HD __host__ __device__ __forceinline__
#else
#define FRM_HD static inline
#endif

// slam_external.py:25-42: R [9] row-major from the unnormalised quaternion q = (r, x, y, z)
FRM_HD void frm_build_rotation(const float* q, float* R)
{
	const float norm = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
	const float r = q[0] / norm, x = q[1] / norm, y = q[2] / norm, z = q[3] / norm;
	R[0] = 1.0f - 2.0f * (y * y + z * z);
	R[1] = 2.0f * (x * y - r * z);
	R[2] = 2.0f * (x * z + r * y);
	R[3] = 2.0f * (x * y + r * z);
	R[4] = 1.0f - 2.0f * (x * x + z * z);
	R[5] = 2.0f * (y * z - r * x);
	R[6] = 2.0f * (x * z - r * y);
	R[7] = 2.0f * (y * z + r * x);
	R[8] = 1.0f - 2.0f * (x * x + y * y);
}

// slam_external.py:435: the reference divides by the Python double 0.8 * n, which torch rounds once to binary32
FRM_HD float frm_split_divisor(int n_into) { return (float)(0.8 * (double)n_into); }

// One child of a split Gaussian, in place: q [4] its copied rotation, logs [cols] its copied log scales (cols is 1 or 3), z [3] its
// normal sample, mean [3] its copied mean.  slam_external.py:430-435: std = exp(log_scales), broadcast over the three axes when
// isotropic; mean += R (z std); log_scale = log(exp(log_scale) / (0.8 n)).
FRM_HD void frm_split_child(const float* q, float* logs, int cols, const float* z, float divisor, float* mean)
{
	float R[9], s[3];
	frm_build_rotation(q, R);
	for (int c = 0; c < 3; c++) s[c] = z[c] * fr_expf(logs[c < cols - 1 ? c : cols - 1]);
	for (int r = 0; r < 3; r++)
	{
		const float offset = (R[3 * r + 0] * s[0] + R[3 * r + 1] * s[1]) + R[3 * r + 2] * s[2];
		mean[r] = mean[r] + offset;
	}
	for (int c = 0; c < cols; c++) logs[c] = logf(fr_expf(logs[c]) / divisor);
}

#endif
