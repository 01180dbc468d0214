// fr_action_math.h -- the agent's actions and the waypoint follower that turns a grid path into an action list, host/device neutral:
// compiled into csrc/fr_action.hip and, with g++, into tests/harness/fr_action_harness.cpp.  Binary64 throughout, as the reference's
// NumPy is.  It restates compute_next_campos (models/SLAM/utils/slam_external.py:44-65) and the second half of NavTester.action_planning
// (tester_gaussians_navigation.py:2246-2330), quirks kept; what differs from the reference is said in INTEGRATION.md section 4b.2.
//
//   pose         a camera-to-world matrix, double [16] row-major, taken to be rigid: its inverse is written in closed form.
//   actions      1 forward by `step` along the camera's +z; 2 / 3 yaw by -/+ turn_angle degrees (right-multiplication by the
//                y-rotation); anything else leaves the pose alone.
//   cells        a path point is (x, z) = (col, row); its world position is that of its centre (+ 0.5), by
//                convert_to_world: (coord - grid_dim / 2) * cell_size + map_center, grid_dim / 2 a true division.
//   convert_to_map   int((c - center) / cell_size + grid_dim // 2), truncating towards zero as Python's int() does (here saturated
//                at the ends of int32, where Python would go on).
//   sine, cosine and the threshold radians(turn_angle) are taken once on the host (fra_make_cfg) and handed to the device, so both
//   sides turn by the very same matrix.
#ifndef FR_ACTION_MATH_H_INCLUDED
#define FR_ACTION_MATH_H_INCLUDED
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FRA_HD __host__ __device__ __forceinline__
#else
#define FRA_HD static inline
#endif

#define FRA_MAX_QUEUE 128                   // the longest action list a call makes (fisher_occ.h: FR_ACTION_MAX_QUEUE)
#define FRA_PI 3.14159265358979323846

typedef struct fra_cfg {
	int32_t grid_w, grid_h;                 // grid_dim[0], grid_dim[1]
	double cell_size;
	double center_x, center_z;              // map_center: the binary32 values, promoted
	double step;                            // forward_step_size
	double turn_angle;                      // degrees
	double sin_a, cos_a;                    // of deg2rad(turn_angle)
	double turn_rad;                        // radians(turn_angle), the follower's threshold
	double cam_height;
	int32_t queue;                          // planning_queue_size
} fra_cfg;

static inline fra_cfg fra_make_cfg(int grid_w, int grid_h, double cell_size, float center_x, float center_z, double step, double turn_angle,
                                   double cam_height, int queue)
{
	fra_cfg c;
	c.grid_w = grid_w; c.grid_h = grid_h;
	c.cell_size = cell_size;
	c.center_x = (double)center_x; c.center_z = (double)center_z;
	c.step = step;
	c.turn_angle = turn_angle;
	const double a = turn_angle * (FRA_PI / 180.0);      // np.deg2rad / np.radians: x * (pi / 180)
	c.sin_a = sin(a); c.cos_a = cos(a);
	c.turn_rad = a;
	c.cam_height = cam_height;
	c.queue = queue;
	return c;
}

// one action applied to T in place (compute_next_campos)
FRA_HD void fra_apply(const fra_cfg* c, double* T, int action)
{
	if (action == 1)
	{
		T[3] = T[3] + T[2] * c->step;
		T[7] = T[7] + T[6] * c->step;
		T[11] = T[11] + T[10] * c->step;
	}
	else if (action == 2 || action == 3)
	{
		const double s = action == 2 ? -c->sin_a : c->sin_a, co = c->cos_a;
		for (int i = 0; i < 3; i++)
		{
			const double r0 = T[4 * i], r2 = T[4 * i + 2];
			T[4 * i] = r0 * co + r2 * (-s);
			T[4 * i + 2] = r0 * s + r2 * co;
		}
	}
}

// the inverse of a rigid T: [R^T | -R^T t]
FRA_HD void fra_rigid_inverse(const double* T, double* W)
{
	for (int i = 0; i < 3; i++)
	{
		for (int j = 0; j < 3; j++) W[4 * i + j] = T[4 * j + i];
		W[4 * i + 3] = -(T[i] * T[3] + T[4 + i] * T[7] + T[8 + i] * T[11]);
	}
	W[12] = 0.0; W[13] = 0.0; W[14] = 0.0; W[15] = 1.0;
}

FRA_HD double fra_to_world(double coord, int dim, double cell, double center) { return (coord - (double)dim / 2.0) * cell + center; }

FRA_HD int32_t fra_to_map(double v, int dim, double cell, double center)
{
	const double b = (v - center) / cell + (double)(dim / 2);
	if (!(b > -2147483648.0)) return INT32_MIN;          // also NaN
	if (b >= 2147483647.0) return INT32_MAX;
	return (int32_t)b;                                     // truncates towards zero
}

// a // b of NumPy's float64 (npy_divmod) for a >= 0, b > 0
FRA_HD double fra_floor_divide(double a, double b)
{
	const double mod = fmod(a, b);
	const double div = (a - mod) / b;
	double fl = floor(div);
	if (div - fl > 0.5) fl += 1.0;
	return fl;
}

FRA_HD double fra_yaw_deg(double m02, double m22) { return atan2(m02, m22) * (180.0 / FRA_PI); }

// what a call writes for the pose after an action; any pointer may be null
FRA_HD void fra_emit(const fra_cfg* c, const double* T, float* w2c, double* xz, int32_t* cell)
{
	if (w2c)
	{
		double W[16];
		fra_rigid_inverse(T, W);
		for (int i = 0; i < 16; i++) w2c[i] = (float)W[i];
	}
	if (xz) { xz[0] = T[3]; xz[1] = T[11]; }
	if (cell)
	{
		cell[0] = fra_to_map(T[3], c->grid_w, c->cell_size, c->center_x);
		cell[1] = fra_to_map(T[11], c->grid_h, c->cell_size, c->center_z);
	}
}

// the stage goal's position relative to the pose, x and z: rows 0 and 2 of inv(T) @ (gx, T.y, gz, 1) -- the goal is at the pose's
// height, so the y term is exactly zero
FRA_HD void fra_relative(const double* T, double gx, double gz, double* rx, double* rz)
{
	const double dx = gx - T[3], dz = gz - T[11];
	*rx = T[0] * dx + T[8] * dz;
	*rz = T[2] * dx + T[10] * dz;
}

// The waypoint follower for one goal.  path: int32 [len][2] = (x, z), len >= 1; finish = the goal's cell (row, col), used only by a
// path of one point, which gets it appended AS IT IS -- row-col into an x-z list -- like the reference; goal_c2w float [16];
// agent: the agent's pose.  Writes actions[k], w2c[k][16], xz[k][2], cells[k][2] for k < the count it returns (<= c->queue).
FRA_HD int fra_follow(const fra_cfg* c, const int32_t* path, int len, int finish_row, int finish_col, const float* goal_c2w, const double* agent,
                      uint8_t* actions, float* w2c, double* xz, int32_t* cells)
{
	double T[16];
	for (int i = 0; i < 16; i++) T[i] = agent[i];
	T[7] = c->cam_height;
	const int npts = len == 1 ? 2 : len;
	int stage = 1;
	int px = len == 1 ? finish_row : path[2], pz = len == 1 ? finish_col : path[3];
	double gx = fra_to_world((double)px + 0.5, c->grid_w, c->cell_size, c->center_x);
	double gz = fra_to_world((double)pz + 0.5, c->grid_h, c->cell_size, c->center_z);
	int k = 0;
	while (k < c->queue)
	{
		double rx, rz;
		fra_relative(T, gx, gz, &rx, &rz);
		if (sqrt(rx * rx + rz * rz) < c->step)
		{
			stage++;
			if (stage == npts)
			{
				double angle = fra_yaw_deg((double)goal_c2w[2], (double)goal_c2w[10]) - fra_yaw_deg(T[2], T[10]);
				if (fabs(angle) > 180.0) angle = angle > 0.0 ? angle - 360.0 : angle + 360.0;
				const double turns = fra_floor_divide(fabs(angle), c->turn_angle);
				const int action = angle > 0.0 ? 2 : 3;
				for (double t = 0.0; t < turns && k < c->queue; t += 1.0, k++)
				{
					fra_apply(c, T, action);
					actions[k] = (uint8_t)action;
					fra_emit(c, T, w2c ? w2c + 16 * (size_t)k : nullptr, xz ? xz + 2 * (size_t)k : nullptr, cells ? cells + 2 * (size_t)k : nullptr);
				}
				break;
			}
			px = path[2 * stage]; pz = path[2 * stage + 1];
			gx = fra_to_world((double)px + 0.5, c->grid_w, c->cell_size, c->center_x);
			gz = fra_to_world((double)pz + 0.5, c->grid_h, c->cell_size, c->center_z);
			fra_relative(T, gx, gz, &rx, &rz);
		}
		const double angle = atan2(rx, rz);
		const int action = angle > c->turn_rad ? 3 : (angle < -c->turn_rad ? 2 : 1);
		fra_apply(c, T, action);
		actions[k] = (uint8_t)action;
		fra_emit(c, T, w2c ? w2c + 16 * (size_t)k : nullptr, xz ? xz + 2 * (size_t)k : nullptr, cells ? cells + 2 * (size_t)k : nullptr);
		k++;
	}
	return k;
}

// the roll-out alone: n actions from `start` (as it is: no height is set here)
FRA_HD void fra_rollout(const fra_cfg* c, const double* start, const uint8_t* actions, int n, float* w2c, double* c2w)
{
	double T[16];
	for (int i = 0; i < 16; i++) T[i] = start[i];
	for (int k = 0; k < n; k++)
	{
		fra_apply(c, T, (int)actions[k]);
		fra_emit(c, T, w2c ? w2c + 16 * (size_t)k : nullptr, nullptr, nullptr);
		if (c2w) for (int i = 0; i < 16; i++) c2w[16 * (size_t)k + i] = T[i];
	}
}

// 1 when goals g and h produced the same list
FRA_HD int fra_same_list(const uint8_t* a, int na, const uint8_t* b, int nb)
{
	if (na != nb) return 0;
	for (int k = 0; k < na; k++) if (a[k] != b[k]) return 0;
	return 1;
}
#endif
