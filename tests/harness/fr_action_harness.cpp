// fr_action_harness.cpp -- csrc/fr_action_math.h on the CPU: the calls of fr_plan_actions / fr_rollout_actions with plain loops in the
// kernels' place, same buffers, same zeros behind a list.  tests/action_cases.py loads it as a shared library; with
// -DFRA_HARNESS_MAIN it is a stand-alone program (the one to put under -fsanitize=address,undefined) that plans a few goals on
// exactly sized buffers and prints a checksum.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../fisher-nerf-customized_amd/csrc/fr_action_math.h"

extern "C" {

int fra_h_max_queue() { return FRA_MAX_QUEUE; }

void fra_h_plan(int grid_w, int grid_h, double cell, float cx, float cz, const int32_t* paths, int max_len, const int32_t* lengths,
                const int32_t* goals, const float* goals_c2w, int G, const double* agent, double cam_height, double step, double turn, int Q,
                uint8_t* actions, int32_t* n_actions, uint8_t* keep, float* w2c, double* c2w_xz, int32_t* map_xz)
{
	const fra_cfg c = fra_make_cfg(grid_w, grid_h, cell, cx, cz, step, turn, cam_height, Q);
	for (int g = 0; g < G; g++)
	{
		uint8_t* act = actions + (size_t)g * Q;
		float* w = w2c + (size_t)g * Q * 16;
		double* xz = c2w_xz + (size_t)g * Q * 2;
		int32_t* cells = map_xz + (size_t)g * Q * 2;
		int len = lengths[g] > max_len ? max_len : lengths[g];
		int n = -1;
		if (len > 0) n = fra_follow(&c, paths + (size_t)g * max_len * 2, len, goals[2 * g], goals[2 * g + 1], goals_c2w + (size_t)g * 16, agent, act, w, xz, cells);
		n_actions[g] = n;
		const size_t k0 = n < 0 ? 0 : (size_t)n;
		for (size_t k = k0; k < (size_t)Q; k++) act[k] = 0;
		for (size_t k = k0 * 16; k < (size_t)Q * 16; k++) w[k] = 0.f;
		for (size_t k = k0 * 2; k < (size_t)Q * 2; k++) { xz[k] = 0.0; cells[k] = 0; }
	}
	for (int g = 0; g < G; g++)
	{
		int same = 0;
		for (int h = 0; h < g && !same && n_actions[g] >= 0; h++)
			same = fra_same_list(actions + (size_t)g * Q, n_actions[g], actions + (size_t)h * Q, n_actions[h]);
		keep[g] = (uint8_t)(n_actions[g] >= 0 && !same);
	}
}

void fra_h_rollout(const double* start, const uint8_t* actions, const int32_t* n_actions, int G, int Q, double step, double turn, float* w2c, double* c2w)
{
	const fra_cfg c = fra_make_cfg(1, 1, 1.0, 0.f, 0.f, step, turn, 0.0, Q);
	for (int g = 0; g < G; g++)
	{
		int n = n_actions[g] < 0 ? 0 : (n_actions[g] > Q ? Q : n_actions[g]);
		float* w = w2c + (size_t)g * Q * 16;
		double* t = c2w ? c2w + (size_t)g * Q * 16 : nullptr;
		fra_rollout(&c, start, actions + (size_t)g * Q, n, w, t);
		for (size_t k = (size_t)n * 16; k < (size_t)Q * 16; k++)
		{
			w[k] = 0.f;
			if (t) t[k] = 0.0;
		}
	}
}

}  // extern "C"

#ifdef FRA_HARNESS_MAIN
int main()
{
	// an odd grid with its centre off the origin; goals: an L-path, a path of one point, no path, a path too long for the queue, the first again
	const int W = 67, H = 70, max_len = 5;
	const double cell = 0.05, step = 0.065, turn = 10.0, cam_height = 0.4;
	const float cx = 0.3f, cz = -0.2f;
	const int32_t one_path[5][2] = {{20, 20}, {20, 30}, {35, 30}, {35, 31}, {36, 31}};
	unsigned long long sum = 0;
	for (int Q : {1, 7, 30, FRA_MAX_QUEUE})
	{
		const int G = 5;
		std::vector<int32_t> paths((size_t)G * max_len * 2), lengths = {3, 1, 0, 5, 3}, goals = {30, 35, 21, 20, 5, 5, 31, 36, 30, 35};
		for (int g = 0; g < G; g++) memcpy(&paths[(size_t)g * max_len * 2], one_path, sizeof(one_path));
		std::vector<float> goals_c2w((size_t)G * 16, 0.f);
		for (int g = 0; g < G; g++)
		{
			float* m = &goals_c2w[(size_t)g * 16];
			const double a = 0.7 * (g % 4) - 2.9;
			m[0] = (float)cos(a); m[2] = (float)sin(a); m[5] = 1.f; m[8] = -(float)sin(a); m[10] = (float)cos(a); m[15] = 1.f;
		}
		double agent[16] = {0};
		const double yaw = 2.6;
		agent[0] = cos(yaw); agent[2] = sin(yaw); agent[5] = 1.0; agent[8] = -sin(yaw); agent[10] = cos(yaw); agent[15] = 1.0;
		agent[3] = fra_to_world(20.4, W, cell, cx); agent[7] = 1.3; agent[11] = fra_to_world(20.6, H, cell, cz);
		std::vector<uint8_t> actions((size_t)G * Q), keep(G);
		std::vector<int32_t> n_actions(G), map_xz((size_t)G * Q * 2);
		std::vector<float> w2c((size_t)G * Q * 16), w2c_again((size_t)G * Q * 16);
		std::vector<double> xz((size_t)G * Q * 2), c2w((size_t)G * Q * 16);
		fra_h_plan(W, H, cell, cx, cz, paths.data(), max_len, lengths.data(), goals.data(), goals_c2w.data(), G, agent, cam_height, step, turn, Q,
		           actions.data(), n_actions.data(), keep.data(), w2c.data(), xz.data(), map_xz.data());
		double start[16];
		memcpy(start, agent, sizeof(start));
		start[7] = cam_height;
		fra_h_rollout(start, actions.data(), n_actions.data(), G, Q, step, turn, w2c_again.data(), c2w.data());
		if (memcmp(w2c.data(), w2c_again.data(), w2c.size() * sizeof(float)) != 0) { printf("the roll-out differs from the plan at Q = %d\n", Q); return 1; }
		if (n_actions[2] != -1 || keep[2] != 0 || keep[4] != 0 || keep[0] != 1) { printf("unexpected keep / n_actions at Q = %d\n", Q); return 1; }
		for (int g = 0; g < G; g++)
		{
			sum = sum * 1000003ull + (unsigned long long)(n_actions[g] + 1) * 7 + keep[g];
			for (int k = 0; k < Q; k++) sum = sum * 31 + actions[(size_t)g * Q + k] + (unsigned)map_xz[((size_t)g * Q + k) * 2];
		}
	}
	printf("checksum %llu\n", sum);
	return 0;
}
#endif
