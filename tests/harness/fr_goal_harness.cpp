// fr_goal_harness.cpp -- csrc/fr_action_object_math.h and csrc/fr_goal_math.h on the CPU: the calls of fr_plan_actions_object,
// fr_occ_object_cells and fr_occ_grid_candidates with plain loops in the kernels' place, same buffers, same zeros behind a list.
// tests/goal_cases.py loads it as a shared library; with -DFRG_HARNESS_MAIN it is a stand-alone program (the one to put under
// -fsanitize=address,undefined) that runs a few goals and clouds on exactly sized buffers and prints a checksum.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../../fisher-nerf-customized_amd/csrc/fr_action_object_math.h"
#include "../../fisher-nerf-customized_amd/csrc/fr_goal_math.h"

extern "C" {

int frg_h_object_max() { return FRA_OBJECT_MAX; }

// bound_hit: int32 [G], 1 where the defensive bound on free stage advances ended a loop
void frg_h_plan_object(int grid_w, int grid_h, double cell, float cx, float cz, const int32_t* paths, int max_len, const int32_t* lengths,
                       const int32_t* goals, const float* goals_c2w, int G, const double* agent, double cam_height, double step, double turn,
                       uint8_t* actions, int32_t* n_actions, uint8_t* keep, float* w2c, double* c2w_xz, int32_t* map_xz, int32_t* pruned,
                       int32_t* pruned_len, int32_t* bound_hit)
{
	const size_t Q = FRA_OBJECT_MAX, room = (size_t)max_len + 1;
	const fra_cfg c = fra_make_cfg(grid_w, grid_h, cell, cx, cz, step, turn, cam_height, FRA_OBJECT_MAX);
	for (int g = 0; g < G; g++)
	{
		uint8_t* act = actions + (size_t)g * Q;
		float* w = w2c + (size_t)g * Q * 16;
		double* xz = c2w_xz + (size_t)g * Q * 2;
		int32_t* cells = map_xz + (size_t)g * Q * 2;
		int32_t* pr = pruned + (size_t)g * room * 2;
		int len = lengths[g] > max_len ? max_len : lengths[g];
		int n = -1, hit = 0;
		int32_t kept = 0;
		if (len > 0)
			n = fra_follow_object(&c, paths + (size_t)g * max_len * 2, len, goals[2 * g], goals[2 * g + 1], goals_c2w + (size_t)g * 16, agent, pr, &kept,
			                      act, w, xz, cells, &hit);
		n_actions[g] = n;
		pruned_len[g] = kept;
		bound_hit[g] = hit;
		const size_t k0 = n < 0 ? 0 : (size_t)n;
		for (size_t k = k0; k < Q; k++) act[k] = 0;
		for (size_t k = k0 * 16; k < Q * 16; k++) w[k] = 0.f;
		for (size_t k = k0 * 2; k < Q * 2; k++) { xz[k] = 0.0; cells[k] = 0; }
		for (size_t k = (size_t)kept * 2; k < room * 2; k++) pr[k] = 0;
	}
	for (int g = 0; g < G; g++)
	{
		int same = 0;
		for (int h = 0; h < g && !same && n_actions[g] > 0; h++)
			same = fra_same_list(actions + (size_t)g * Q, n_actions[g], actions + (size_t)h * Q, n_actions[h]);
		keep[g] = (uint8_t)(n_actions[g] > 0 && !same);
	}
}

void frg_h_object_cells(int grid_w, int grid_h, float cell, float cx, float cz, const float* points, int n, int min_count, int32_t* cells,
                        int max_cells, int32_t* counts)
{
	std::vector<uint32_t> hist((size_t)grid_w * grid_h, 0u);
	int32_t binned = 0;
	for (int i = 0; i < n; i++)
	{
		const float x = points[3 * (size_t)i], z = points[3 * (size_t)i + 2];
		if (!frg_finite(x) || !frg_finite(z)) continue;
		hist[(size_t)frg_bin(z, cz, cell, grid_h) * grid_w + frg_bin(x, cx, cell, grid_w)]++;
		binned++;
	}
	int32_t found = 0;
	for (size_t i = 0; i < hist.size(); i++)
	{
		if (hist[i] <= (uint32_t)min_count) continue;
		if (found < max_cells) { cells[2 * (size_t)found] = (int32_t)(i % grid_w); cells[2 * (size_t)found + 1] = (int32_t)(i / grid_w); }
		found++;
	}
	counts[0] = found; counts[1] = binned;
}

// angles float [max(1, n_theta - 1)], radii float [bins]
void frg_h_tables(int n_theta, int bins, int sqrt_area, float min_range, float radius, float* angles, float* radii)
{
	for (int j = 0; j < frg_n_angles(n_theta); j++) angles[j] = frg_angle(n_theta, j);
	for (int i = 0; i < bins; i++) radii[i] = frg_radius(min_range, radius, bins, sqrt_area, i);
}

// the poses of fr_occ_grid_candidates around float centres, with the host's sinf / cosf
void frg_h_grid(const float* centers, int n_centers, int K, float min_range, float radius, int n_theta, int bins, int sqrt_area, float cam_height,
                uint32_t seed, float* c2w)
{
	for (int k = 0; k < K; k++)
	{
		const int ci = frg_center_index(seed, (uint32_t)k, n_centers);
		frg_grid_pose(k, n_theta, bins, sqrt_area, min_range, radius, centers[2 * (size_t)ci], centers[2 * (size_t)ci + 1], cam_height, c2w + 16 * (size_t)k);
	}
}

}  // extern "C"

#ifdef FRG_HARNESS_MAIN
int main()
{
	unsigned long long sum = 0;
	// an odd grid with its centre off the origin; goals: an L-path, a path of one point, no path, a long straight path, the first again
	const int W = 67, H = 70;
	const double cell = 0.05, cam_height = 0.4;
	const float cx = 0.3f, cz = -0.2f;
	for (int max_len : {5, 130})
	{
		const int G = 5;
		std::vector<int32_t> paths((size_t)G * max_len * 2, -7777), lengths = {3, 1, 0, max_len, 3}, goals = {30, 35, 21, 20, 5, 5, 31, 36, 30, 35};
		const int32_t ell[3][2] = {{20, 20}, {20, 30}, {35, 30}};
		for (int g : {0, 1, 4}) memcpy(&paths[(size_t)g * max_len * 2], ell, sizeof(ell));
		for (int i = 0; i < max_len; i++) { paths[((size_t)3 * max_len + i) * 2] = 20 + i / 3; paths[((size_t)3 * max_len + i) * 2 + 1] = 20 + i / 4; }
		std::vector<float> goals_c2w((size_t)G * 16, 0.f);
		for (int g = 0; g < G; g++)
		{
			float* m = &goals_c2w[(size_t)g * 16];
			const double a = 0.7 * (g % 4) - 2.9;
			m[0] = (float)cos(a); m[2] = (float)sin(a); m[5] = 1.f; m[8] = -(float)sin(a); m[10] = (float)cos(a); m[15] = 1.f;
			m[3] = (float)fra_to_world(goals[2 * g + 1] + 0.5, W, cell, cx); m[7] = 0.9f; m[11] = (float)fra_to_world(goals[2 * g] + 0.5, H, cell, cz);
		}
		double agent[16] = {0};
		const double yaw = 2.6;
		agent[0] = cos(yaw); agent[2] = sin(yaw); agent[5] = 1.0; agent[8] = -sin(yaw); agent[10] = cos(yaw); agent[15] = 1.0;
		agent[3] = fra_to_world(20.4, W, cell, cx); agent[7] = 1.3; agent[11] = fra_to_world(20.6, H, cell, cz);
		for (double step : {0.065, 0.25})
		{
			const size_t Q = FRA_OBJECT_MAX;
			std::vector<uint8_t> actions((size_t)G * Q), keep(G);
			std::vector<int32_t> n_actions(G), map_xz((size_t)G * Q * 2), pruned((size_t)G * (max_len + 1) * 2), pruned_len(G), hit(G);
			std::vector<float> w2c((size_t)G * Q * 16);
			std::vector<double> xz((size_t)G * Q * 2);
			frg_h_plan_object(W, H, cell, cx, cz, paths.data(), max_len, lengths.data(), goals.data(), goals_c2w.data(), G, agent, cam_height, step, 10.0,
			                  actions.data(), n_actions.data(), keep.data(), w2c.data(), xz.data(), map_xz.data(), pruned.data(), pruned_len.data(), hit.data());
			if (n_actions[2] != -1 || keep[2] != 0 || keep[4] != 0 || pruned_len[2] != 0) { printf("unexpected keep / n_actions\n"); return 1; }
			for (int g = 0; g < G; g++)
			{
				if (hit[g]) { printf("the defensive bound was reached at goal %d\n", g); return 1; }
				sum = sum * 1000003ull + (unsigned long long)(n_actions[g] + 1) * 7 + keep[g] + (unsigned)pruned_len[g] * 13;
				for (size_t k = 0; k < Q; k++) sum = sum * 31 + actions[(size_t)g * Q + k] + (unsigned)map_xz[((size_t)g * Q + k) * 2];
			}
		}
	}
	// a cloud with points outside the map and rows that are not finite, on exactly sized buffers; then the grid around its cells' float centres
	{
		const int n = 500, max_cells = 3;
		std::vector<float> pts((size_t)n * 3);
		for (int i = 0; i < n; i++) { pts[3 * (size_t)i] = cx + 0.011f * (float)(i % 17) - 0.05f; pts[3 * (size_t)i + 1] = 0.1f; pts[3 * (size_t)i + 2] = cz + 0.3f * (float)(i % 5); }
		pts[0] = NAN; pts[5] = INFINITY; pts[6] = 1e30f; pts[11] = -1e30f;
		std::vector<int32_t> cells((size_t)max_cells * 2), counts(2);
		frg_h_object_cells(W, H, (float)cell, cx, cz, pts.data(), n, 3, cells.data(), max_cells, counts.data());
		if (counts[1] != n - 2 || counts[0] < max_cells) { printf("unexpected counts %d %d\n", counts[0], counts[1]); return 1; }
		std::vector<float> centers((size_t)max_cells * 2);
		for (int i = 0; i < max_cells; i++)
		{
			centers[2 * (size_t)i] = frg_cell_world(cells[2 * (size_t)i], W, (float)cell, cx);
			centers[2 * (size_t)i + 1] = frg_cell_world(cells[2 * (size_t)i + 1], H, (float)cell, cz);
		}
		for (int n_theta : {1, 2, 24})
			for (int bins : {1, 6})
			{
				const int K = 139;
				std::vector<float> angles(frg_n_angles(n_theta)), radii(bins), c2w((size_t)K * 16);
				frg_h_tables(n_theta, bins, bins > 1, 0.2f, 1.5f, angles.data(), radii.data());
				frg_h_grid(centers.data(), max_cells, K, 0.2f, 1.5f, n_theta, bins, bins > 1, (float)cam_height, 77u, c2w.data());
				sum = sum * 31 + (unsigned long long)(angles.back() * 1000.f) + (unsigned long long)(radii.back() * 1000.f) + (c2w[(size_t)(K - 1) * 16 + 15] == 1.f);
			}
		sum = sum * 31 + (unsigned)counts[0];
	}
	printf("checksum %llu\n", sum);
	return 0;
}
#endif
