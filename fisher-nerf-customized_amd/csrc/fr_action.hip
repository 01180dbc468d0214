// fr_action.hip -- action planning of libfisher_rast.so (gfx950, wave64): fr_plan_actions / fr_rollout_actions.
//
// The reference turns every goal's grid path into the agent's action list in a host loop (tester_gaussians_navigation.py:2246-2330):
// per step a 4 x 4 inverse, a compute_next_campos and an atan2, then a duplicate-list filter; the path evaluation rolls the same
// actions out again and inverts every pose (1684-1687).  Here (arithmetic: fr_action_math.h, binary64):
//
//   k_action_follow           one wave per goal.  Lane 0 runs the waypoint follower, which is sequential -- each decision reads the pose
//                             the previous action left -- and writes the action, the pose's inverse (rounded once to binary32), its
//                             x-z and its cell after every action.  The wave then fills what lies behind the list: zeros.
//   k_action_keep             a second launch, after every list exists: one wave per goal, its lanes share the search for an equal
//                             list among the earlier goals that have a path.  No workgroup waits for another.
//   k_action_rollout          one thread per list: the roll-out alone.
//
// Sine and cosine of the turn are taken on the host and travel in the kernel arguments with the agent's pose (fra_cfg).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fr_internal.h"
#include "../../include/fisher_occ.h"
#include "fr_action_math.h"

static_assert(FRA_MAX_QUEUE == FR_ACTION_MAX_QUEUE, "fisher_occ.h and fr_action_math.h disagree on the queue cap");

#define FRA_WAVE 64

struct ActionPose { double m[16]; };

__global__ __launch_bounds__(FRA_WAVE) void k_action_follow(fra_cfg c, ActionPose agent, const int32_t* __restrict__ paths, int max_len,
                                                           const int32_t* __restrict__ lengths, const int32_t* __restrict__ goals,
                                                           const float* __restrict__ goals_c2w, uint8_t* __restrict__ actions,
                                                           int32_t* __restrict__ n_actions, float* __restrict__ w2c, double* __restrict__ c2w_xz,
                                                           int32_t* __restrict__ map_xz)
{
	const int g = blockIdx.x, lane = threadIdx.x;
	const size_t Q = (size_t)c.queue;
	uint8_t* act = actions + (size_t)g * Q;
	float* w = w2c + (size_t)g * Q * 16;
	double* xz = c2w_xz + (size_t)g * Q * 2;
	int32_t* cells = map_xz + (size_t)g * Q * 2;
	__shared__ int s_n;
	if (lane == 0)
	{
		int len = lengths[g];
		if (len > max_len) len = max_len;                  // never read past a goal's block of `paths`
		int n = -1;
		if (len > 0)
			n = fra_follow(&c, paths + (size_t)g * max_len * 2, len, goals[2 * g], goals[2 * g + 1], goals_c2w + (size_t)g * 16, agent.m, act, w, xz, cells);
		n_actions[g] = n;
		s_n = n < 0 ? 0 : n;
	}
	__syncthreads();
	const size_t n = (size_t)s_n;
	for (size_t k = n + lane; k < Q; k += FRA_WAVE) act[k] = 0;
	for (size_t k = n * 16 + lane; k < Q * 16; k += FRA_WAVE) w[k] = 0.f;
	for (size_t k = n * 2 + lane; k < Q * 2; k += FRA_WAVE) { xz[k] = 0.0; cells[k] = 0; }
}

__global__ __launch_bounds__(FRA_WAVE) void k_action_keep(int Q, const uint8_t* __restrict__ actions, const int32_t* __restrict__ n_actions,
                                                         uint8_t* __restrict__ keep)
{
	const int g = blockIdx.x, lane = threadIdx.x;
	const int n = n_actions[g];
	int same = 0;
	if (n >= 0)
		for (int h = lane; h < g && !same; h += FRA_WAVE)
			same = fra_same_list(actions + (size_t)g * Q, n, actions + (size_t)h * Q, n_actions[h]);
	same = __syncthreads_or(same);
	if (lane == 0) keep[g] = (uint8_t)(n >= 0 && !same);
}

__global__ __launch_bounds__(FRA_WAVE) void k_action_rollout(fra_cfg c, ActionPose start, int G, const uint8_t* __restrict__ actions,
                                                            const int32_t* __restrict__ n_actions, float* __restrict__ w2c, double* __restrict__ c2w)
{
	const int g = blockIdx.x * FRA_WAVE + threadIdx.x;
	if (g >= G) return;
	const size_t Q = (size_t)c.queue;
	int n = n_actions[g];
	n = n < 0 ? 0 : (n > c.queue ? c.queue : n);
	float* w = w2c + (size_t)g * Q * 16;
	double* t = c2w ? c2w + (size_t)g * Q * 16 : nullptr;
	fra_rollout(&c, start.m, actions + (size_t)g * Q, n, w, t);
	for (size_t k = (size_t)n * 16; k < Q * 16; k++)
	{
		w[k] = 0.f;
		if (t) t[k] = 0.0;
	}
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

static bool action_finite(double v) { return v == v && v - v == 0.0; }

extern "C" int fr_plan_actions(const fr_occ_cfg* cfg, const int32_t* paths, int32_t max_len, const int32_t* lengths, const int32_t* goals,
                               const float* goals_c2w, int32_t n_goals, const double* agent_c2w, double cam_height, double forward_step_size,
                               double turn_angle, int32_t queue_size, double cell_size, uint8_t* actions, int32_t* n_actions, uint8_t* keep,
                               float* w2c, double* c2w_xz, int32_t* map_xz, fr_stream_t stream)
{
	if (!cfg || cfg->grid_w <= 0 || cfg->grid_h <= 0) return fr_fail(FR_EINVAL, "fr_plan_actions: bad fr_occ_cfg");
	if (n_goals < 0 || max_len < 1) return fr_fail(FR_EINVAL, "fr_plan_actions: bad argument (n_goals must not be negative, max_len at least 1)");
	if (queue_size < 1 || queue_size > FR_ACTION_MAX_QUEUE) return fr_fail(FR_EINVAL, "fr_plan_actions: bad argument (queue_size must be 1 .. FR_ACTION_MAX_QUEUE)");
	if (!(cell_size > 0.0) || !(forward_step_size > 0.0) || !(turn_angle > 0.0) || !action_finite(cell_size) || !action_finite(forward_step_size) ||
	    !action_finite(turn_angle) || !action_finite(cam_height))
		return fr_fail(FR_EINVAL, "fr_plan_actions: bad argument (cell_size, forward_step_size, turn_angle must be positive and finite, cam_height finite)");
	if (!agent_c2w) return fr_fail(FR_EINVAL, "fr_plan_actions: null pointer (agent_c2w)");
	for (int i = 0; i < 16; i++)
		if (!action_finite(agent_c2w[i])) return fr_fail(FR_EINVAL, "fr_plan_actions: bad argument (agent_c2w is not finite)");
	if (n_goals == 0) return FR_OK;
	if (!paths || !lengths || !goals || !goals_c2w || !actions || !n_actions || !keep || !w2c || !c2w_xz || !map_xz)
		return fr_fail(FR_EINVAL, "fr_plan_actions: null pointer (paths, lengths, goals, goals_c2w, actions, n_actions, keep, w2c, c2w_xz, map_xz)");
	if ((uintptr_t)paths % 4 || (uintptr_t)lengths % 4 || (uintptr_t)goals % 4 || (uintptr_t)goals_c2w % 4 || (uintptr_t)n_actions % 4 ||
	    (uintptr_t)w2c % 4 || (uintptr_t)map_xz % 4 || (uintptr_t)c2w_xz % 8)
		return fr_fail(FR_EINVAL, "fr_plan_actions: bad argument (c2w_xz must be 8-byte, the other word arrays 4-byte aligned)");
	const fra_cfg c = fra_make_cfg(cfg->grid_w, cfg->grid_h, cell_size, cfg->center_x, cfg->center_z, forward_step_size, turn_angle, cam_height, queue_size);
	ActionPose agent;
	for (int i = 0; i < 16; i++) agent.m[i] = agent_c2w[i];
	hipStream_t s = (hipStream_t)stream;
	hipLaunchKernelGGL(k_action_follow, dim3(n_goals), dim3(FRA_WAVE), 0, s, c, agent, paths, max_len, lengths, goals, goals_c2w, actions, n_actions,
	                   w2c, c2w_xz, map_xz);
	int rc;
	if ((rc = fr_check_launch("k_action_follow"))) return rc;
	hipLaunchKernelGGL(k_action_keep, dim3(n_goals), dim3(FRA_WAVE), 0, s, queue_size, (const uint8_t*)actions, (const int32_t*)n_actions, keep);
	return fr_check_launch("k_action_keep");
}

extern "C" int fr_rollout_actions(const double* start_c2w, const uint8_t* actions, const int32_t* n_actions, int32_t n_lists, int32_t queue_size,
                                  double forward_step_size, double turn_angle, float* w2c, double* c2w, fr_stream_t stream)
{
	if (n_lists < 0) return fr_fail(FR_EINVAL, "fr_rollout_actions: bad argument (n_lists must not be negative)");
	if (queue_size < 1 || queue_size > FR_ACTION_MAX_QUEUE) return fr_fail(FR_EINVAL, "fr_rollout_actions: bad argument (queue_size must be 1 .. FR_ACTION_MAX_QUEUE)");
	if (!action_finite(forward_step_size) || !action_finite(turn_angle))
		return fr_fail(FR_EINVAL, "fr_rollout_actions: bad argument (forward_step_size, turn_angle must be finite)");
	if (!start_c2w) return fr_fail(FR_EINVAL, "fr_rollout_actions: null pointer (start_c2w)");
	for (int i = 0; i < 16; i++)
		if (!action_finite(start_c2w[i])) return fr_fail(FR_EINVAL, "fr_rollout_actions: bad argument (start_c2w is not finite)");
	if (n_lists == 0) return FR_OK;
	if (!actions || !n_actions || !w2c) return fr_fail(FR_EINVAL, "fr_rollout_actions: null pointer (actions, n_actions, w2c)");
	if ((uintptr_t)n_actions % 4 || (uintptr_t)w2c % 4 || (uintptr_t)c2w % 8)
		return fr_fail(FR_EINVAL, "fr_rollout_actions: bad argument (n_actions, w2c must be 4-byte, c2w 8-byte aligned)");
	const fra_cfg c = fra_make_cfg(1, 1, 1.0, 0.f, 0.f, forward_step_size, turn_angle, 0.0, queue_size);
	ActionPose start;
	for (int i = 0; i < 16; i++) start.m[i] = start_c2w[i];
	hipLaunchKernelGGL(k_action_rollout, dim3((n_lists + FRA_WAVE - 1) / FRA_WAVE), dim3(FRA_WAVE), 0, (hipStream_t)stream, c, start, n_lists, actions,
	                   n_actions, w2c, c2w);
	return fr_check_launch("k_action_rollout");
}
