// fr_action_object.hip -- the follower of the object round in libfisher_rast.so (gfx950, wave64): fr_plan_actions_object.
//
// NavTester.action_planning_object_adv (tester_gaussians_navigation.py:2403-2496) prunes every goal's grid path near the goal and walks
// it in a host loop of up to 200 actions with three to five 4 x 4 inverses per step.  Here (arithmetic: fr_action_object_math.h on
// fr_action_math.h, binary64):
//
//   k_action_object_follow    one wave per goal.  The wave prunes its path together: the lanes test 64 points at a time, a ballot and a
//                             count of the set bits below the lane give each surviving point its slot, the chunk's base carried from
//                             chunk to chunk -- the order of the path is kept.  Lane 0 then runs the follower, which is sequential,
//                             and the wave fills what lies behind the list and behind the pruned path: zeros.
//   k_action_object_keep      a second launch, after every list exists: one wave per goal, its lanes share the search for an equal list
//                             among the earlier goals.  A list without an action is dropped, unlike fr_plan_actions'.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fr_internal.h"
#include "../../include/fisher_occ.h"
#include "fr_action_object_math.h"

static_assert(FRA_OBJECT_MAX == FR_ACTION_OBJECT_MAX, "fisher_occ.h and fr_action_object_math.h disagree on the cap");

#define FAO_WAVE 64

struct ActionObjectPose { double m[16]; };

__global__ __launch_bounds__(FAO_WAVE) void k_action_object_follow(fra_cfg c, ActionObjectPose agent, const int32_t* __restrict__ paths, int max_len,
                                                                  const int32_t* __restrict__ lengths, const int32_t* __restrict__ goals,
                                                                  const float* __restrict__ goals_c2w, uint8_t* __restrict__ actions,
                                                                  int32_t* __restrict__ n_actions, float* __restrict__ w2c, double* __restrict__ c2w_xz,
                                                                  int32_t* __restrict__ map_xz, int32_t* pruned_all, int32_t* __restrict__ pruned_len)
{
	const int g = blockIdx.x, lane = threadIdx.x;
	const size_t Q = FRA_OBJECT_MAX, room = (size_t)max_len + 1;
	uint8_t* act = actions + (size_t)g * Q;
	float* w = w2c + (size_t)g * Q * 16;
	double* xz = c2w_xz + (size_t)g * Q * 2;
	int32_t* cells = map_xz + (size_t)g * Q * 2;
	int32_t* pruned = pruned_all + (size_t)g * room * 2;
	const int32_t* path = paths + (size_t)g * max_len * 2;
	const float* goal = goals_c2w + (size_t)g * 16;
	__shared__ int s_n, s_kept;
	int len = lengths[g];
	if (len > max_len) len = max_len;                      // never read past a goal's block of `paths`
	int kept = 0;
	if (len > 0)
	{
		const int np = fao_padded_len(len), fr = goals[2 * g], fc = goals[2 * g + 1];
		const double gx = (double)goal[3], gz = (double)goal[11], h = agent.m[7];
		for (int base = 0; base < np; base += FAO_WAVE)    // np is the same in every lane: the ballots are whole
		{
			const int i = base + lane;
			int32_t px = 0, pz = 0;
			bool stays = false;
			if (i < np)
			{
				fao_point(path, len, fr, fc, i, &px, &pz);
				stays = fao_stays(&c, px, pz, gx, gz, h) != 0;
			}
			const unsigned long long b = __ballot(stays);
			if (stays)
			{
				const size_t slot = (size_t)kept + (size_t)__popcll(b & ((1ull << lane) - 1ull));      // <= i: inside the goal's block
				pruned[2 * slot] = px; pruned[2 * slot + 1] = pz;
			}
			kept += (int)__popcll(b);
		}
	}
	__syncthreads();                                       // the pruned path is in memory before lane 0 reads it
	if (lane == 0)
	{
		int n = -1;
		if (len > 0)
		{
			kept = fao_prune_fixup(path, len, goals[2 * g], goals[2 * g + 1], pruned, kept);
			n = fao_follow_pruned(&c, pruned, kept, goal, agent.m, act, w, xz, cells, nullptr);
		}
		n_actions[g] = n;
		pruned_len[g] = kept;
		s_n = n < 0 ? 0 : n;
		s_kept = kept;
	}
	__syncthreads();
	const size_t n = (size_t)s_n;
	for (size_t k = n + lane; k < Q; k += FAO_WAVE) act[k] = 0;
	for (size_t k = n * 16 + lane; k < Q * 16; k += FAO_WAVE) w[k] = 0.f;
	for (size_t k = n * 2 + lane; k < Q * 2; k += FAO_WAVE) { xz[k] = 0.0; cells[k] = 0; }
	for (size_t k = (size_t)s_kept * 2 + lane; k < room * 2; k += FAO_WAVE) pruned[k] = 0;
}

__global__ __launch_bounds__(FAO_WAVE) void k_action_object_keep(const uint8_t* __restrict__ actions, const int32_t* __restrict__ n_actions,
                                                                uint8_t* __restrict__ keep)
{
	const int g = blockIdx.x, lane = threadIdx.x;
	const int n = n_actions[g];
	int same = 0;
	if (n > 0)
		for (int h = lane; h < g && !same; h += FAO_WAVE)
			same = fra_same_list(actions + (size_t)g * FRA_OBJECT_MAX, n, actions + (size_t)h * FRA_OBJECT_MAX, n_actions[h]);
	same = __syncthreads_or(same);
	if (lane == 0) keep[g] = (uint8_t)(n > 0 && !same);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

static bool fao_finite(double v) { return v == v && v - v == 0.0; }

extern "C" int fr_plan_actions_object(const fr_occ_cfg* cfg, const int32_t* paths, int32_t max_len, const int32_t* lengths, const int32_t* goals,
                                      const float* goals_c2w, int32_t n_goals, const double* agent_c2w, double cam_height, double forward_step_size,
                                      double turn_angle, double cell_size, uint8_t* actions, int32_t* n_actions, uint8_t* keep, float* w2c,
                                      double* c2w_xz, int32_t* map_xz, int32_t* pruned, int32_t* pruned_len, fr_stream_t stream)
{
	if (!cfg || cfg->grid_w <= 0 || cfg->grid_h <= 0) return fr_fail(FR_EINVAL, "fr_plan_actions_object: bad fr_occ_cfg");
	if (n_goals < 0 || max_len < 1) return fr_fail(FR_EINVAL, "fr_plan_actions_object: bad argument (n_goals must not be negative, max_len at least 1)");
	if (!(cell_size > 0.0) || !(forward_step_size > 0.0) || !(turn_angle > 0.0) || !fao_finite(cell_size) || !fao_finite(forward_step_size) ||
	    !fao_finite(turn_angle) || !fao_finite(cam_height))
		return fr_fail(FR_EINVAL, "fr_plan_actions_object: bad argument (cell_size, forward_step_size, turn_angle must be positive and finite, cam_height finite)");
	if (!agent_c2w) return fr_fail(FR_EINVAL, "fr_plan_actions_object: null pointer (agent_c2w)");
	for (int i = 0; i < 16; i++)
		if (!fao_finite(agent_c2w[i])) return fr_fail(FR_EINVAL, "fr_plan_actions_object: bad argument (agent_c2w is not finite)");
	if (n_goals == 0) return FR_OK;
	if (!paths || !lengths || !goals || !goals_c2w || !actions || !n_actions || !keep || !w2c || !c2w_xz || !map_xz || !pruned || !pruned_len)
		return fr_fail(FR_EINVAL, "fr_plan_actions_object: null pointer (paths, lengths, goals, goals_c2w, actions, n_actions, keep, w2c, c2w_xz, map_xz, pruned, pruned_len)");
	if (!fr_aligned(paths, 4) || !fr_aligned(lengths, 4) || !fr_aligned(goals, 4) || !fr_aligned(goals_c2w, 4) || !fr_aligned(n_actions, 4) ||
	    !fr_aligned(w2c, 4) || !fr_aligned(map_xz, 4) || !fr_aligned(pruned, 4) || !fr_aligned(pruned_len, 4) || !fr_aligned(c2w_xz, 8))
		return fr_fail(FR_EINVAL, "fr_plan_actions_object: bad argument (c2w_xz must be 8-byte, the other word arrays 4-byte aligned)");
	const fra_cfg c = fra_make_cfg(cfg->grid_w, cfg->grid_h, cell_size, cfg->center_x, cfg->center_z, forward_step_size, turn_angle, cam_height, FRA_OBJECT_MAX);
	ActionObjectPose agent;
	for (int i = 0; i < 16; i++) agent.m[i] = agent_c2w[i];
	hipStream_t s = (hipStream_t)stream;
	hipLaunchKernelGGL(k_action_object_follow, dim3(n_goals), dim3(FAO_WAVE), 0, s, c, agent, paths, max_len, lengths, goals, goals_c2w, actions, n_actions,
	                   w2c, c2w_xz, map_xz, pruned, pruned_len);
	int rc;
	if ((rc = fr_check_launch("k_action_object_follow"))) return rc;
	hipLaunchKernelGGL(k_action_object_keep, dim3(n_goals), dim3(FAO_WAVE), 0, s, (const uint8_t*)actions, (const int32_t*)n_actions, keep);
	return fr_check_launch("k_action_object_keep");
}
