// fr_goal_math.h -- goal selection of the object round, host/device neutral: compiled into csrc/fr_goal.hip and, with g++, into
// tests/harness/fr_goal_harness.cpp.  It restates what AstarPlanner.build_object_frontiers (planning/astar.py:686-734) and
// generate_candidate_adv_object(mode="sorted") (1471-1588) compute per point and per pose:
//
//   frg_bin          discretize_coords (datasets/util/map_utils.py:106-125), the rule of fr_occ_cells_of: floor((v - c) / cell) +
//                    (dim - 1) / 2.0, truncated, clamped to the grid -- a Gaussian outside the map counts in the border cell.  A
//                    non-finite coordinate has no cell (frg_finite): the reference's cast is undefined there.
//   frg_cell_world   a cell's world position as build_frontiers / build_object_frontiers give it: (cell - dim // 2) * cell_size +
//                    map_center, in binary64, rounded once.
//   frg_n_angles, frg_linspace, frg_angle, frg_radius
//                    the two tables of the sorted grid.  n_theta = max(1, round(2 pi / deg2rad(step))) comes from the caller, who
//                    takes it on the host as the reference does; the angles are the first max(1, n_theta - 1) points of
//                    linspace(0, 2 pi, n_theta) -- the reference drops the closing angle, so 15 degrees give 23 angles, not 24;
//                    the radii are linspace(min_range, radius, bins), or
//                    sqrt(min^2 + linspace(0, 1, bins) (max^2 - min^2)) with sqrt_area and more than one bin.  Every entry is taken
//                    in binary64 (start + i * step, the last point the end itself, as np.linspace) and rounded once to binary32.
//   frg_uniform, frg_yaw_rotation
//                    the counter-based generator and the yaw rotation of the ring kernel (fisher_occ.hip: occ_uniform,
//                    occ_yaw_rotation), restated so that both kernels draw the same centres and build the same orientation.
#ifndef FR_GOAL_MATH_H_INCLUDED
#define FR_GOAL_MATH_H_INCLUDED
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FRG_HD __host__ __device__ __forceinline__
#else
#define FRG_HD static inline
#endif

#define FRG_TWO_PI 6.283185307179586476925286766559
#define FRG_PI_F 3.14159274101257324f                     // torch.pi as float32

FRG_HD int frg_finite(float v) { return v - v == 0.0f; }

FRG_HD int frg_bin(float x, float c, float cell, int dim)
{
	const float b = floorf((x - c) / cell) + (float)(dim - 1) / 2.0f;
	if (!(b > 0.0f)) return 0;
	if (b >= (float)(dim - 1)) return dim - 1;
	return (int)b;
}

FRG_HD float frg_cell_world(int cell, int dim, float cell_size, float center)
{
	return (float)((double)(cell - dim / 2) * (double)cell_size + (double)center);
}

// point i of np.linspace(lo, hi, n)
FRG_HD double frg_linspace(double lo, double hi, int n, int i)
{
	if (n <= 1) return lo;
	if (i == n - 1) return hi;
	const double step = (hi - lo) / (double)(n - 1);
	return lo + (double)i * step;
}

FRG_HD int frg_n_angles(int n_theta) { return n_theta - 1 > 1 ? n_theta - 1 : 1; }

FRG_HD float frg_angle(int n_theta, int j) { return (float)frg_linspace(0.0, FRG_TWO_PI, n_theta, j); }

FRG_HD float frg_radius(float min_range, float radius, int bins, int sqrt_area, int i)
{
	if (sqrt_area && bins > 1)
	{
		const double lo = (double)min_range * (double)min_range, hi = (double)radius * (double)radius;
		return (float)sqrt(lo + frg_linspace(0.0, 1.0, bins, i) * (hi - lo));
	}
	return (float)frg_linspace((double)min_range, (double)radius, bins, i);
}

// the ring kernel's generator: x = seed + 0x9E3779B9 (4 k + j + 1), a 32-bit finaliser, u = (x >> 8) / 2^24 in [0, 1)
FRG_HD float frg_uniform(uint32_t seed, uint32_t k, uint32_t j)
{
	uint32_t x = seed + 0x9E3779B9u * (4u * k + j + 1u);
	x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
	return (float)(x >> 8) * (1.0f / 16777216.0f);
}

// the index of pose k's centre among n (> 0) centres, drawn with replacement
FRG_HD int frg_center_index(uint32_t seed, uint32_t k, int n)
{
	const int ci = (int)(frg_uniform(seed, k, 2) * (float)n);
	return ci > n - 1 ? n - 1 : ci;
}

// rotation about y from the quaternion (qr, 0, qy, 0) as build_rotation does it, columns scaled by s0..s2, into rows 0..2 of a 4x4
FRG_HD void frg_yaw_rotation(float qr, float qy, float* m, float s0, float s1, float s2)
{
	const float norm = sqrtf(qr * qr + qy * qy);
	const float r = qr / norm, y = qy / norm;
	const float d = 1.0f - 2.0f * (y * y), o = 2.0f * (r * y);
	m[0] = d * s0;  m[1] = 0.0f * s1; m[2] = o * s2;
	m[4] = 0.0f * s0; m[5] = 1.0f * s1; m[6] = 0.0f * s2;
	m[8] = -o * s0; m[9] = 0.0f * s1; m[10] = d * s2;
}

// pose k of the sorted grid around the centre (cx, cz): entry k mod (bins * angles), the ring index the slow one
FRG_HD void frg_grid_pose(int k, int n_theta, int bins, int sqrt_area, float min_range, float radius, float cx, float cz, float cam_height,
                          float* m)
{
	const int angles = frg_n_angles(n_theta);
	const int e = k % (bins * angles);
	const float r = frg_radius(min_range, radius, bins, sqrt_area, e / angles);
	const float theta = frg_angle(n_theta, e % angles);
	const float phi = theta + FRG_PI_F;
	frg_yaw_rotation(cosf(phi / 2.0f), sinf(phi / 2.0f), m, -1.0f, -1.0f, 1.0f);      // astar.py:1579-1580: columns 0 and 1 negated
	m[3] = cx + r * sinf(theta); m[7] = cam_height; m[11] = cz + r * cosf(theta);
	m[12] = 0.f; m[13] = 0.f; m[14] = 0.f; m[15] = 1.f;
}
#endif
