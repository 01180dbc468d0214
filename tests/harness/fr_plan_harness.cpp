// g++ build of csrc/fr_plan_math.h with plain drivers: the planning grid, the capped L1 transform, a Dijkstra over the move table and
// the path read-out.  tests/plan_cases.py loads it as a shared library; with -DFRP_HARNESS_MAIN it is a stand-alone program (the
// one to put under -fsanitize=address,undefined) that plans on a small serpentine and prints a checksum.
#include <stdint.h>
#include <stdio.h>
#include <queue>
#include <utility>
#include <vector>
#include "../../fisher-nerf-customized_amd/csrc/fr_plan_math.h"

extern "C" {

void frp_h_grid(int H, int W, const float* occ_map, const float* pts, int n, float cell, float cx, float cz, float cam_height, int sy, int sx,
                uint8_t* occ_plan, int32_t* status)
{
	const size_t cells = (size_t)H * W;
	std::vector<uint32_t> hist(cells, 0u);
	std::vector<uint8_t> raw(cells, 0);
	int32_t binned = 0;
	for (int i = 0; i < n; i++)
	{
		if (!frp_in_band(pts[3 * (size_t)i + 1], cam_height)) continue;
		const int col = frp_bin(pts[3 * (size_t)i], cx, cell, W), row = frp_bin(pts[3 * (size_t)i + 2], cz, cell, H);
		if (col < 0 || row < 0) continue;
		hist[(size_t)row * W + col]++;
		binned++;
	}
	for (size_t i = 0; i < cells; i++)
	{
		const float a = occ_map[i], b = occ_map[cells + i], c = occ_map[2 * cells + i];
		raw[i] = ((b > a && !(c > b)) || hist[i] > (uint32_t)FRP_GAUSSIAN_MIN) ? 1 : 0;
	}
	int32_t ring = 0;
	for (int y = 0; y < H; y++)
		for (int x = 0; x < W; x++)
		{
			uint8_t r = 0;
			for (int yy = y - 1; yy <= y + 1; yy++)
				for (int xx = x - 1; xx <= x + 1; xx++)
					if (yy >= 0 && yy < H && xx >= 0 && xx < W && raw[(size_t)yy * W + xx]) r = 1;
			const int ady = y > sy ? y - sy : sy - y, adx = x > sx ? x - sx : sx - x;
			if (ady == 0 && adx == 0) r = 0;
			else if (ady <= 1 && adx <= 1 && r) ring++;
			occ_plan[(size_t)y * W + x] = r;
		}
	status[0] = ring; status[1] = binned; status[2] = 0; status[3] = 0;
}

void frp_h_tiers(int H, int W, const uint8_t* free_space, uint8_t* tiers)
{
	for (int y = 0; y < H; y++)
		for (int x = 0; x < W; x++)
		{
			int d = FRP_DIST_CAP;
			for (int yy = y - (FRP_DIST_CAP - 1); yy <= y + (FRP_DIST_CAP - 1); yy++)
			{
				if (yy < 0 || yy >= H) continue;
				const int ry = yy > y ? yy - y : y - yy;
				for (int xx = x - (FRP_DIST_CAP - 1 - ry); xx <= x + (FRP_DIST_CAP - 1 - ry); xx++)
				{
					if (xx < 0 || xx >= W || free_space[(size_t)yy * W + xx]) continue;
					const int v = ry + (xx > x ? xx - x : x - xx);
					d = v < d ? v : d;
				}
			}
			tiers[(size_t)y * W + x] = frp_tier_byte(free_space[(size_t)y * W + x] != 0, d);
		}
}

// plain Dijkstra in push form; returns 1 when the start is in free space
int frp_h_field(int H, int W, const uint8_t* tiers, int sy, int sx, uint64_t* field)
{
	const size_t cells = (size_t)H * W;
	for (size_t i = 0; i < cells; i++) field[i] = FRP_UNREACHED;
	const uint32_t s = (uint32_t)((size_t)sy * W + sx);
	if (!(tiers[s] & 1)) return 0;
	typedef std::pair<uint32_t, uint32_t> Item;                    // (cost bits, cell)
	std::priority_queue<Item, std::vector<Item>, std::greater<Item>> heap;
	std::vector<uint8_t> done(cells, 0);
	field[s] = (uint64_t)s;
	heap.push(Item(0u, s));
	while (!heap.empty())
	{
		const Item it = heap.top();
		heap.pop();
		const uint32_t u = it.second;
		if (done[u] || it.first != (uint32_t)(field[u] >> 32)) continue;
		done[u] = 1;
		const int uy = (int)(u / (uint32_t)W), ux = (int)(u % (uint32_t)W);
		for (int m = 0; m < FRP_MOVES; m++)
		{
			const uint8_t b = frp_weight_byte(tiers, H, W, uy, ux, m);
			if (b == FRP_NO_MOVE) continue;
			int dy, dx;
			frp_move(m, &dy, &dx);
			const uint32_t v = (uint32_t)((size_t)(uy + dy) * W + (ux + dx));
			const uint64_t cand = frp_relax(field[u], u, m, b);
			if (cand < field[v])
			{
				const bool cheaper = (uint32_t)(cand >> 32) != (uint32_t)(field[v] >> 32);
				field[v] = cand;
				if (cheaper) heap.push(Item((uint32_t)(cand >> 32), v));
			}
		}
	}
	return 1;
}

static int frp_h_blocked(int H, int W, const uint8_t* occ, int ay, int ax, int by, int bx)
{
	const int y0 = (ay < by ? ay : by) - 4, y1 = (ay < by ? by : ay) + 4, x0 = (ax < bx ? ax : bx) - 4, x1 = (ax < bx ? bx : ax) + 4;
	for (int y = y0; y <= y1; y++)
		for (int x = x0; x <= x1; x++)
			if (y >= 0 && y < H && x >= 0 && x < W && occ[(size_t)y * W + x] && frp_in_band_of_segment(ay, ax, by, bx, y, x)) return 1;
	return 0;
}

void frp_h_paths(int H, int W, const uint64_t* field, const uint8_t* occ_plan, int sy, int sx, const int32_t* goals, int G, int shortcut,
                 int32_t* paths, int max_len, int32_t* lengths)
{
	const int64_t cells = (int64_t)H * W, start = (int64_t)sy * W + sx;
	for (int g = 0; g < G; g++)
	{
		int32_t* out = paths + (size_t)g * max_len * 2;
		const int64_t end = frp_end_cell(field, occ_plan, H, W, sy, sx, goals[2 * g], goals[2 * g + 1]);
		std::vector<int64_t> chain;
		if (end >= 0)
		{
			int64_t cur = end;
			chain.push_back(cur);
			while (cur != start && (int64_t)chain.size() <= cells)
			{
				cur = (int64_t)(field[cur] & 0xFFFFFFFFull);
				chain.push_back(cur);
			}
			if ((int64_t)chain.size() > cells) chain.clear();
		}
		std::vector<std::pair<int, int>> p;                         // (x, z), start first
		for (size_t k = chain.size(); k-- > 0;) p.push_back(std::make_pair((int)(chain[k] % W), (int)(chain[k] / W)));
		// the path as walked has to fit (it is shortcut in place); a two-point path grows to three under the shortcut
		if ((int64_t)((shortcut && p.size() == 2) ? 3 : p.size()) > max_len) { lengths[g] = -1; continue; }
		if (shortcut && p.size() >= 2)
		{
			std::vector<std::pair<int, int>> sc;
			sc.push_back(p[0]); sc.push_back(p[1]);
			size_t path_idx = 1;
			for (size_t i = 2; i + 1 < p.size(); i++)
			{
				if (!frp_h_blocked(H, W, occ_plan, sc[path_idx - 1].second, sc[path_idx - 1].first, p[i].second, p[i].first)) sc[path_idx] = p[i];
				else { sc.push_back(p[i]); path_idx++; }
			}
			sc.push_back(p.back());
			p = sc;
		}
		lengths[g] = (int32_t)p.size();
		for (size_t k = 0; k < p.size(); k++) { out[2 * k] = p[k].first; out[2 * k + 1] = p[k].second; }
	}
}

}  // extern "C"

#ifdef FRP_HARNESS_MAIN
int main()
{
	const int H = 70, W = 67;
	std::vector<float> occ_map(3 * (size_t)H * W, 0.f);
	std::vector<uint8_t> free_space((size_t)H * W, 1), occ_plan((size_t)H * W), tiers((size_t)H * W);
	for (int y = 0; y < H; y++)
		for (int x = 0; x < W; x++)
		{
			const bool wall = y % 12 == 8 && ((y / 12) % 2 ? x >= 9 : x < W - 9);
			occ_map[(wall ? 1 : 2) * (size_t)H * W + (size_t)y * W + x] = wall ? 1.f : 2.f;
			free_space[(size_t)y * W + x] = wall ? 0 : 1;
		}
	std::vector<float> pts;
	for (int i = 0; i < 60; i++) { pts.push_back(0.26f); pts.push_back(0.2f); pts.push_back(-1.23f); }
	pts.push_back(1e9f); pts.push_back(0.2f); pts.push_back(0.f);
	int32_t status[4];
	frp_h_grid(H, W, occ_map.data(), pts.data(), (int)pts.size() / 3, 0.05f, 0.f, 0.f, 0.5f, 2, 3, occ_plan.data(), status);
	frp_h_tiers(H, W, free_space.data(), tiers.data());
	std::vector<uint64_t> field((size_t)H * W);
	const int in_free = frp_h_field(H, W, tiers.data(), 2, 3, field.data());
	const int32_t goals[] = {66, 60, 2, 4, 8, 8, 69, 0, -1, 5, 30, 30};
	const int G = 6, max_len = H * W + 1;
	std::vector<int32_t> paths((size_t)G * max_len * 2), lengths(G);
	uint64_t sum = 0;
	for (int shortcut = 0; shortcut < 2; shortcut++)
	{
		frp_h_paths(H, W, field.data(), occ_plan.data(), 2, 3, goals, G, shortcut, paths.data(), max_len, lengths.data());
		for (int g = 0; g < G; g++) sum = sum * 31 + (uint64_t)(lengths[g] + 7);
	}
	for (size_t i = 0; i < field.size(); i++) sum = sum * 1099511628211ull + field[i];
	printf("in_free %d ring %d binned %d lengths %d %d %d %d %d %d checksum %016llx\n", in_free, status[0], status[1], lengths[0], lengths[1], lengths[2],
	       lengths[3], lengths[4], lengths[5], (unsigned long long)sum);
	return in_free && lengths[0] > 2 ? 0 : 1;
}
#endif
