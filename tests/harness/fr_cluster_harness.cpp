// g++ build of csrc/fr_cluster_math.h: a brute-force DBSCAN and target selection over the SAME functions the kernels compile, so that
// what they return states the kernels' results bit for bit (tests/test_cluster_cpu.py, tests/test_gpu_cluster.py).  Every pair is
// tested (no grid), components are merged serially.  With -DFRK_HARNESS_MAIN it is a stand-alone program (for a sanitizer run).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../fisher-nerf-customized_amd/csrc/fr_cluster_math.h"

static int find_root(std::vector<int>& parent, int x)
{
	while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
	return x;
}

static int dbscan(int n, const float* pts, float eps, int min_samples, int32_t* labels)
{
	const float eps2 = frk_eps2(eps);
	std::vector<char> ok(n), core(n, 0);
	for (int i = 0; i < n; i++) ok[i] = frk_finite3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
	auto inside = [&](int i, int j) {
		return frk_inside(frk_dist2(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], pts[3 * j], pts[3 * j + 1], pts[3 * j + 2]), eps2);
	};
	for (int i = 0; i < n; i++)
	{
		if (!ok[i]) continue;
		int cnt = 0;
		for (int j = 0; j < n; j++) if (ok[j] && inside(i, j)) cnt++;
		core[i] = cnt >= min_samples;
	}
	std::vector<int> parent(n);
	for (int i = 0; i < n; i++) parent[i] = i;
	for (int i = 0; i < n; i++)
	{
		if (!core[i]) continue;
		for (int j = i + 1; j < n; j++)
		{
			if (!core[j] || !inside(i, j)) continue;
			const int a = find_root(parent, i), b = find_root(parent, j);
			if (a != b) parent[a > b ? a : b] = a > b ? b : a;          // the lower index stays the root
		}
	}
	std::vector<int> number(n, -1);
	int clusters = 0;
	for (int i = 0; i < n; i++) if (core[i] && find_root(parent, i) == i) number[i] = clusters++;     // ascending lowest core index
	for (int i = 0; i < n; i++) labels[i] = core[i] ? number[find_root(parent, i)] : -1;
	for (int i = 0; i < n; i++)
	{
		if (core[i] || !ok[i]) continue;
		int best = INT32_MAX;
		for (int j = 0; j < n; j++) if (core[j] && inside(i, j) && labels[j] < best) best = labels[j];
		if (best != INT32_MAX) labels[i] = best;
	}
	return clusters;
}

// the frame of the finite points and the sides; returns the number of finite points
static int grid_of(int n, const float* pts, float eps, float* lo, float* side)
{
	float hi[3] = { -INFINITY, -INFINITY, -INFINITY };
	lo[0] = lo[1] = lo[2] = INFINITY;
	int nf = 0;
	for (int i = 0; i < n; i++)
	{
		if (!frk_finite3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2])) continue;
		for (int a = 0; a < 3; a++) { lo[a] = fminf(lo[a], pts[3 * i + a]); hi[a] = fmaxf(hi[a], pts[3 * i + a]); }
		nf++;
	}
	for (int a = 0; a < 3; a++) side[a] = frk_side(lo[a], hi[a], eps);
	return nf;
}

extern "C" {

int frk_h_eps_ok(float eps) { return frk_eps_ok(eps) ? 1 : 0; }
float frk_h_dist2(const float* p, const float* q) { return frk_dist2(p[0], p[1], p[2], q[0], q[1], q[2]); }
int frk_h_inside(const float* p, const float* q, float eps) { return frk_inside(frk_dist2(p[0], p[1], p[2], q[0], q[1], q[2]), frk_eps2(eps)) ? 1 : 0; }
float frk_h_side(float lo, float hi, float eps) { return frk_side(lo, hi, eps); }
uint32_t frk_h_cell(float p, float lo, float side) { return frk_cell(p, lo, side); }

// the cell of every point on every axis in the cloud's own grid (cells [n,3]; FRK_NO_CODE rows for a non-finite point), the sides
void frk_h_cells(int n, const float* pts, float eps, uint32_t* cells, float* sides)
{
	float lo[3];
	grid_of(n, pts, eps, lo, sides);
	for (int i = 0; i < n; i++)
		for (int a = 0; a < 3; a++)
			cells[3 * i + a] = frk_finite3(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]) ? frk_cell(pts[3 * i + a], lo[a], sides[a]) : FRK_NO_CODE;
}

// status as fr_dbscan writes it: {clusters, finite points, three sides (float bits), 0, 0, 0}
void frk_h_dbscan(int n, const float* pts, float eps, int min_samples, int32_t* labels, int32_t* status)
{
	float lo[3], side[3];
	for (int k = 0; k < 8; k++) status[k] = 0;
	if (n == 0) return;
	status[0] = dbscan(n, pts, eps, min_samples, labels);
	status[1] = grid_of(n, pts, eps, lo, side);
	for (int a = 0; a < 3; a++) status[2 + a] = (int32_t)frk_bits(side[a]);
}

void frk_h_quantile_rank(float q, uint32_t n, uint32_t* out2, float* weight) { frk_quantile_rank(q, n, out2, out2 + 1, weight); }
float frk_h_lerp(float a, float b, float w) { return frk_lerp(a, b, w); }

// torch.quantile(x, q) of n values in any order (no NaN among them)
float frk_h_quantile(uint32_t n, const float* x, float q)
{
	std::vector<uint32_t> e(n);
	for (uint32_t i = 0; i < n; i++) e[i] = frk_enc(x[i]);
	std::sort(e.begin(), e.end());
	uint32_t below, above;
	float w;
	frk_quantile_rank(q, n, &below, &above, &w);
	return frk_lerp(frk_dec(e[below]), frk_dec(e[above]), w);
}

// gaussian.py:1247-1257 over the scores and labels of the points above the threshold
int frk_h_winner(int n, const float* scores, const int32_t* labels)
{
	int clusters = 0;
	for (int j = 0; j < n; j++) clusters = std::max(clusters, labels[j] + 1);
	int max_label = -1;
	float max_score = FRK_START_SCORE;
	for (int c = 0; c < clusters; c++)
	{
		bool any = false;
		uint32_t best = 0;
		for (int j = 0; j < n; j++) if (labels[j] == c) { best = any ? std::max(best, frk_enc(scores[j])) : frk_enc(scores[j]); any = true; }
		if (any && frk_beats(frk_dec(best), max_score)) { max_label = c; max_score = frk_dec(best); }
	}
	return max_label;
}

// fr_target_select, every output as the library lays it out (lists hold their first n_* entries); status: 16 int32
void frk_h_target_select(int P, const float* means, const float* scores, float lower_y, float upper_y, float q, float eps, int min_samples,
                         int32_t* band_idx, int32_t* above_idx, int32_t* labels, int32_t* sel_idx, float* threshold, int32_t* status)
{
	for (int k = 0; k < 16; k++) status[k] = 0;
	int nb = 0, argmax = -1, nan = 0;
	std::vector<float> bs;
	for (int i = 0; i < P; i++)
	{
		if (!frk_in_band(means[3 * i + 1], lower_y, upper_y)) continue;
		band_idx[nb++] = i;
		bs.push_back(scores[i]);
		if (scores[i] != scores[i]) nan = 1;
		if (argmax < 0 || frk_enc(scores[i]) > frk_enc(scores[argmax])) argmax = i;
	}
	*threshold = nb ? frk_h_quantile((uint32_t)nb, bs.data(), q) : NAN;
	int na = 0;
	std::vector<float> pts, as;
	for (int j = 0; j < nb; j++)
	{
		if (!frk_above(frk_dec(frk_enc(bs[j])), *threshold)) continue;
		const int row = band_idx[j];
		above_idx[na++] = row;
		as.push_back(bs[j]);
		for (int a = 0; a < 3; a++) pts.push_back(means[3 * row + a]);
	}
	float lo[3], side[3];
	const int clusters = na ? dbscan(na, pts.data(), eps, min_samples, labels) : 0;
	const int nf = grid_of(na, pts.data(), eps, lo, side);
	const int max_label = frk_h_winner(na, as.data(), labels);
	int ns = 0;
	for (int j = 0; j < na; j++) if (labels[j] == max_label) sel_idx[ns++] = above_idx[j];
	status[0] = nb; status[1] = na; status[2] = clusters; status[3] = max_label; status[4] = ns; status[5] = argmax;
	for (int a = 0; a < 3; a++) status[6 + a] = P > 0 ? (int32_t)frk_bits(side[a]) : 0;      // (P = 0: no DBSCAN is launched)
	status[9] = nan; status[10] = (int32_t)frk_bits(*threshold); status[11] = nf;
}

}

#ifdef FRK_HARNESS_MAIN
int main()
{
	const int n = 600;
	std::vector<float> pts(3 * n), scores(n);
	uint32_t s = 12345u;
	auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
	for (int i = 0; i < n; i++)
	{
		const float c = (float)(i % 3);
		pts[3 * i] = c + 0.2f * rnd(); pts[3 * i + 1] = 0.4f * rnd(); pts[3 * i + 2] = -c + 0.2f * rnd();
		scores[i] = rnd();
	}
	pts[3 * 7] = NAN;
	std::vector<int32_t> labels(n), band(n), above(n), lab2(n), sel(n);
	int32_t st[16];
	frk_h_dbscan(n, pts.data(), 0.1f, 5, labels.data(), st);
	float thr;
	frk_h_target_select(n, pts.data(), scores.data(), 0.1f, 0.3f, 0.8f, 0.1f, 5, band.data(), above.data(), lab2.data(), sel.data(), &thr, st);
	std::vector<uint32_t> cells(3 * n);
	float sides[3];
	frk_h_cells(n, pts.data(), 0.1f, cells.data(), sides);
	printf("clusters %d band %d above %d selected %d threshold %.9g\n", st[2], st[0], st[1], st[4], thr);
	return 0;
}
#endif
