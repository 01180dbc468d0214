// fr_action_object_math.h -- the follower of the object round, host/device neutral: compiled into csrc/fr_action_object.hip and, with
// g++, into tests/harness/fr_goal_harness.cpp.  Binary64 throughout.  It restates the loop of NavTester.action_planning_object_adv
// (tester_gaussians_navigation.py:2403-2496) on fr_action_math.h's pose arithmetic, quirks kept:
//
//   padding    a path of one point gets `finish` = (row, col) appended AS IT IS -- row-col into an x-z list -- when it differs
//              element-wise from the point, else the point again (2395-2401).
//   pruning    a waypoint stays when d_goal > 2 step, d_goal = ||(wx - gx, h - gz)||: (wx, wz) the waypoint's cell centre, (gx, gz)
//              the goal's position, h the AGENT's own height agent_c2w[1][3] (not cam_height).  The reference builds [wx, wz, h, 1]
//              and indexes [0, 2] against [gx, h, gz, 1][[0, 2]] (2405-2408), so the waypoint's z never enters.  Nothing left: the
//              path becomes [first, last]; fewer than 2 points left: `finish` is appended (2411-2415).
//   goal yaw   np.arctan2 of two binary32 scalars, a binary32 value: the binary64 atan2 rounded once.  The pose's own yaw and
//              dyaw = atan2(sin d, cos d) are binary64.
//   per step   (1) d_final < 2.5 step and |dyaw| <= radians(turn): stop.  (2) d_final < 2.5 step: turn, 2 when dyaw > 0, else 3.
//              (3) the stage goal within `step`: with a next waypoint, jump to the final position (stage = last) when
//              ||rel_final|| - ||rel_next|| < 0.25 step, else take it; without one the final position becomes the stage goal; no
//              action is spent.  (4) steer: 3 if atan2(rx, rz) > turn, 2 if < -turn, else 1.
//   the cap    FRA_OBJECT_MAX = 200 actions, the reference's SAFETY_CAP; the planning queue does not cut these lists.
//   the bound  the free advances of (3) are bounded by the path's length (once the final position is the stage goal, (1) or (2) come
//              first); the loop still ends after len + 2 of them in a row and says so.
#ifndef FR_ACTION_OBJECT_MATH_H_INCLUDED
#define FR_ACTION_OBJECT_MATH_H_INCLUDED
#include "fr_action_math.h"

#define FRA_OBJECT_MAX 200                  // fisher_occ.h: FR_ACTION_OBJECT_MAX

// points of the padded path: a path of one point counts two
FRA_HD int fao_padded_len(int len) { return len == 1 ? 2 : len; }

// point i of the padded path (x, z)
FRA_HD void fao_point(const int32_t* path, int len, int finish_row, int finish_col, int i, int32_t* px, int32_t* pz)
{
	if (len == 1 && i == 1)
	{
		const int same = path[0] == finish_row && path[1] == finish_col;
		*px = same ? path[0] : finish_row;
		*pz = same ? path[1] : finish_col;
		return;
	}
	*px = path[2 * i]; *pz = path[2 * i + 1];
}

// does the waypoint (px, pz) survive the pruning?  h: the agent's own height
FRA_HD int fao_stays(const fra_cfg* c, int32_t px, int32_t pz, double gx, double gz, double h)
{
	const double wx = fra_to_world((double)px + 0.5, c->grid_w, c->cell_size, c->center_x);
	(void)pz;                                                     // [wx, wz, h, 1][[0, 2]] = (wx, h): the waypoint's z is not read
	const double dx = wx - gx, dz = h - gz;
	return sqrt(dx * dx + dz * dz) > 2.0 * c->step;
}

// the pruning of one path, in order: pruned[.][2] gets the survivors, the count is returned (before fao_prune_fixup)
FRA_HD int fao_prune(const fra_cfg* c, const int32_t* path, int len, int finish_row, int finish_col, double gx, double gz, double h, int32_t* pruned)
{
	const int np = fao_padded_len(len);
	int kept = 0;
	for (int i = 0; i < np; i++)
	{
		int32_t px, pz;
		fao_point(path, len, finish_row, finish_col, i, &px, &pz);
		if (fao_stays(c, px, pz, gx, gz, h)) { pruned[2 * kept] = px; pruned[2 * kept + 1] = pz; kept++; }
	}
	return kept;
}

// what the reference does with a pruned path of fewer than 2 points; returns the final count (>= 2)
FRA_HD int fao_prune_fixup(const int32_t* path, int len, int finish_row, int finish_col, int32_t* pruned, int kept)
{
	if (kept == 0)
	{
		fao_point(path, len, finish_row, finish_col, 0, &pruned[0], &pruned[1]);
		fao_point(path, len, finish_row, finish_col, fao_padded_len(len) - 1, &pruned[2], &pruned[3]);
		kept = 2;
	}
	if (kept < 2)
	{
		pruned[2 * kept] = finish_row; pruned[2 * kept + 1] = finish_col;
		kept++;
	}
	return kept;
}

// The follower on a pruned path of plen >= 2 points.  Writes actions[k], w2c[k][16], xz[k][2], cells[k][2] for k < the count it
// returns (<= FRA_OBJECT_MAX); *bound_hit (or null) is set when the defensive bound ended the loop.
FRA_HD int fao_follow_pruned(const fra_cfg* c, const int32_t* pruned, int plen, const float* goal_c2w, const double* agent,
                             uint8_t* actions, float* w2c, double* xz, int32_t* cells, int* bound_hit)
{
	double T[16];
	for (int i = 0; i < 16; i++) T[i] = agent[i];
	T[7] = c->cam_height;
	const double fx = (double)goal_c2w[3], fz = (double)goal_c2w[11];
	const double yaw_goal = (double)(float)atan2((double)goal_c2w[2], (double)goal_c2w[10]);
	const double pos_tol = 2.5 * c->step, skip_margin = 0.25 * c->step;
	int stage = 1;
	double gx = fra_to_world((double)pruned[2] + 0.5, c->grid_w, c->cell_size, c->center_x);
	double gz = fra_to_world((double)pruned[3] + 0.5, c->grid_h, c->cell_size, c->center_z);
	int k = 0, free_run = 0;
	if (bound_hit) *bound_hit = 0;
	while (k < FRA_OBJECT_MAX)
	{
		double rx, rz;
		fra_relative(T, fx, fz, &rx, &rz);
		const double d_final = sqrt(rx * rx + rz * rz);
		const double d = yaw_goal - atan2(T[2], T[10]);
		const double dyaw = atan2(sin(d), cos(d));
		int action;
		if (d_final < pos_tol)
		{
			if (fabs(dyaw) <= c->turn_rad) break;
			action = dyaw > 0.0 ? 2 : 3;
		}
		else
		{
			fra_relative(T, gx, gz, &rx, &rz);
			if (sqrt(rx * rx + rz * rz) < c->step)
			{
				if (stage + 1 < plen)
				{
					const double nx = fra_to_world((double)pruned[2 * (stage + 1)] + 0.5, c->grid_w, c->cell_size, c->center_x);
					const double nz = fra_to_world((double)pruned[2 * (stage + 1) + 1] + 0.5, c->grid_h, c->cell_size, c->center_z);
					double qx, qz;
					fra_relative(T, nx, nz, &qx, &qz);
					if (d_final - sqrt(qx * qx + qz * qz) < skip_margin) { gx = fx; gz = fz; stage = plen - 1; }
					else { stage++; gx = nx; gz = nz; }
				}
				else { gx = fx; gz = fz; }
				if (++free_run > plen + 2)
				{
					if (bound_hit) *bound_hit = 1;
					break;
				}
				continue;
			}
			const double angle = atan2(rx, rz);
			action = angle > c->turn_rad ? 3 : (angle < -c->turn_rad ? 2 : 1);
		}
		free_run = 0;
		fra_apply(c, T, action);
		actions[k] = (uint8_t)action;
		fra_emit(c, T, w2c ? w2c + 16 * (size_t)k : nullptr, xz ? xz + 2 * (size_t)k : nullptr, cells ? cells + 2 * (size_t)k : nullptr);
		k++;
	}
	return k;
}

// One goal from its path to its list: pruned int32 [fao_padded_len(len) .. at most len + 1][2] and *pruned_len are written too.
FRA_HD int fra_follow_object(const fra_cfg* c, const int32_t* path, int len, int finish_row, int finish_col, const float* goal_c2w, const double* agent,
                             int32_t* pruned, int32_t* pruned_len, uint8_t* actions, float* w2c, double* xz, int32_t* cells, int* bound_hit)
{
	int kept = fao_prune(c, path, len, finish_row, finish_col, (double)goal_c2w[3], (double)goal_c2w[11], agent[7], pruned);
	kept = fao_prune_fixup(path, len, finish_row, finish_col, pruned, kept);
	*pruned_len = kept;
	return fao_follow_pruned(c, pruned, kept, goal_c2w, agent, actions, w2c, xz, cells, bound_hit);
}
#endif
