// g++ build of the POp-GS block stage's arithmetic (csrc/fr_popgs_block_math.h) for CPU-side checks: the per-pair term, the
// factorisation and the prior block are the header's, the same functions k_pb_score / k_pb_prior of csrc/fr_popgs_block.hip compile;
// the loops over poses and prior rows are written here, in plain index order.  Also the layout of fr_raster_cfg and fr_raster_ext
// as a C++ compiler sees them and the workspace macro, for the ctypes mirrors in fisher_rast/_lib.py.
// -DFRPB_HARNESS_MAIN: a program of its own (for the sanitizer run of tests/test_popgs_block_cpu.py).
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cmath>
#include <vector>
#include "../../include/fisher_rast.h"
#include "../../fisher-nerf-customized_amd/csrc/fr_popgs_block_math.h"

#define FRPBH_SWITCH(d, CALL) \
	switch (d) { case 3: CALL(3) break; case 4: CALL(4) break; case 6: CALL(6) break; case 7: CALL(7) break; case 8: CALL(8) break; \
	             case 10: CALL(10) break; case 11: CALL(11) break; default: return -1; }

extern "C" {

int frpbh_dim(int o, int r, int s) { return frpb_dim(o, r, s); }
void frpbh_cols(int o, int r, int s, int* out) { for (int c = 0; c < frpb_dim(o, r, s); c++) out[c] = frpb_col(c, o, r, s); }

// A [d, d] binary64 (lower triangle read): pivots[d], trace(A^-1) and sum log|pi| from the header's factor.  Returns the header's
// flag (1: a non-positive pivot), -1 for a d the stage does not have.
int frpbh_factor(int d, const double* A, double* pivots, double* trace_inv, double* logabs)
{
	double t[FRPB_TRI(11)];
	for (int i = 0; i < d; i++) for (int j = 0; j <= i; j++) t[i * (i + 1) / 2 + j] = A[i * d + j];
	int bad = 0;
#define FRPBH_CALL(D) { bad = frpb_ldlt<D>(t); for (int j = 0; j < D; j++) pivots[j] = t[j * (j + 1) / 2 + j]; *logabs = frpb_logabs<D>(t); *trace_inv = frpb_trace_inv<D>(t); }
	FRPBH_SWITCH(d, FRPBH_CALL)
#undef FRPBH_CALL
	return bad;
}

// the term of one pair (frpb_pair_term); returns the number of factorisations with a non-positive pivot, -1 for a bad d
int frpbh_pair(int o, int r, int s, const float* rows, long long k_stride, int K, const float* prior, double lam, int criterion, double* term)
{
	int cols[11], bad = 0;
	const int d = frpb_dim(o, r, s);
	frpbh_cols(o, r, s, cols);
#define FRPBH_CALL(D) { *term = frpb_pair_term<D>(rows, k_stride, K, cols, prior, lam, criterion, bad); }
	FRPBH_SWITCH(d, FRPBH_CALL)
#undef FRPBH_CALL
	return bad;
}

// one keyframe's binary32 block added to (first: stored into) the lower triangle acc[d (d + 1) / 2]
int frpbh_prior_add(int o, int r, int s, const float* rows, long long k_stride, int K, int first, float* acc)
{
	int cols[11];
	const int d = frpb_dim(o, r, s);
	frpbh_cols(o, r, s, cols);
#define FRPBH_CALL(D) { frpb_prior_add<D>(rows, k_stride, K, cols, first != 0, acc); }
	FRPBH_SWITCH(d, FRPBH_CALL)
#undef FRPBH_CALL
	return 0;
}

// The SCORE mode on the CPU: rows [poses K, P, 11], vis [poses, P], prior [n, d, d], idx [n]; a pose's terms are added in the order
// of the prior rows.  status as the stage's.
int frpbh_scores(int o, int r, int s, int P, int poses, int K, int n, const float* rows, const uint8_t* vis, const float* prior,
                 const int32_t* idx, double lam, int criterion, double* scores, int32_t* matched, int32_t* status)
{
	const int d = frpb_dim(o, r, s);
	const long long stride = 11ll * P;
	status[0] = status[1] = status[2] = status[3] = 0;
	for (int p = 0; p < poses; p++)
	{
		double sum = 0.0;
		int m = 0;
		for (int q = 0; q < n; q++)
		{
			const int32_t i = idx[q];
			if (i < 0 || i >= P) { if (p == 0) status[3]++; continue; }
			if (!vis[(size_t)p * P + i]) continue;
			double term = 0.0;
			const int bad = frpbh_pair(o, r, s, rows + (long long)p * K * stride + 11ll * i, stride, K, prior + (size_t)q * d * d, lam, criterion, &term);
			if (bad < 0) return -1;
			sum += term; m++; status[2] += bad;
		}
		scores[p] = m ? sum : -INFINITY;
		matched[p] = m;
		status[0] += m;
	}
	return 0;
}

unsigned long long frpbh_ws_bytes(long long P, long long poses) { return (unsigned long long)FR_POPGS_BLOCK_WS_BYTES(P, poses); }

// out[0..2] = FR_EXT_POPGS_BLOCK, FR_POPGS_BLOCK_MAX_WG, the three modes packed as VISIBLE + 10 SCORE + 100 PRIOR
void frpbh_constants(long long* out)
{
	out[0] = FR_EXT_POPGS_BLOCK; out[1] = FR_POPGS_BLOCK_MAX_WG;
	out[2] = FR_POPGS_BLOCK_VISIBLE + 10 * FR_POPGS_BLOCK_SCORE + 100 * FR_POPGS_BLOCK_PRIOR;
}

// out[0] = sizeof(fr_raster_cfg), out[1..14] its field offsets in declaration order; out[15] = sizeof(fr_raster_ext), out[16..31] its
// field offsets in declaration order.  Returns the number of values written.
int frpbh_layout(long long* out)
{
	int n = 0;
	out[n++] = (long long)sizeof(fr_raster_cfg);
#define O(f) out[n++] = (long long)offsetof(fr_raster_cfg, f);
	O(P) O(image_height) O(image_width) O(tanfovx) O(tanfovy) O(scale_modifier) O(sh_degree) O(sh_coeffs) O(prefiltered) O(bg) O(viewmatrix)
	O(projmatrix) O(campos) O(ext)
#undef O
	out[n++] = (long long)sizeof(fr_raster_ext);
#define O(f) out[n++] = (long long)offsetof(fr_raster_ext, f);
	O(kind) O(mode) O(K) O(use_opacity) O(use_rot) O(use_scale) O(criterion) O(n) O(lam) O(vis_in) O(out_vis) O(out_vis_count) O(prior_blocks)
	O(prior_idx) O(out_scores) O(out_matched)
#undef O
	return n;
}

}

#ifdef FRPB_HARNESS_MAIN
// every flag combination, K = 1 .. 3, both criteria over a small synthetic batch with exactly-sized buffers (the sanitizer's red zones
// stand round them): an index out of range, an unsorted list, a pose without a match
int main()
{
	uint32_t seed = 12345u;
	auto rnd = [&seed]() { seed = seed * 1664525u + 1013904223u; return (float)((seed >> 8) & 0xffff) / 32768.0f - 1.0f; };
	for (int flags = 0; flags < 8; flags++)
	{
		const int o = flags & 1, r = (flags >> 1) & 1, s = (flags >> 2) & 1, d = frpb_dim(o, r, s);
		for (int K = 1; K <= 3; K++)
		{
			const int P = 37, poses = 3, n = 29;
			std::vector<float> rows((size_t)poses * K * P * 11), prior((size_t)n * d * d);
			std::vector<uint8_t> vis((size_t)poses * P);
			std::vector<int32_t> idx(n);
			for (auto& v : rows) v = rnd();
			for (int q = 0; q < n; q++)
			{
				std::vector<float> m((size_t)d * d);
				for (auto& v : m) v = rnd();
				for (int i = 0; i < d; i++) for (int j = 0; j < d; j++)
				{
					float acc = i == j ? 0.01f : 0.0f;
					for (int k = 0; k < d; k++) acc += m[i * d + k] * m[j * d + k];
					prior[(size_t)q * d * d + i * d + j] = acc;
				}
				idx[q] = (q * 7) % P;
			}
			idx[5] = P; idx[6] = -1;
			for (int p = 0; p < poses; p++) for (int i = 0; i < P; i++) vis[(size_t)p * P + i] = p == 2 ? 0 : (uint8_t)((i + p) % 3 != 0);
			for (int criterion = 0; criterion < 2; criterion++)
			{
				std::vector<double> scores(poses);
				std::vector<int32_t> matched(poses);
				int32_t status[4];
				if (frpbh_scores(o, r, s, P, poses, K, n, rows.data(), vis.data(), prior.data(), idx.data(), 1e-6, criterion, scores.data(), matched.data(), status)) return 1;
				if (status[3] != 2 || status[2] != 0 || matched[2] != 0 || !(scores[2] < 0 && std::isinf(scores[2])) || !std::isfinite(scores[0])) { printf("bad result d = %d K = %d\n", d, K); return 1; }
			}
			std::vector<float> acc((size_t)d * (d + 1) / 2);
			frpbh_prior_add(o, r, s, rows.data(), 11ll * P, K, 1, acc.data());
			frpbh_prior_add(o, r, s, rows.data() + 11 * (P - 1), 11ll * P, K, 0, acc.data());
			std::vector<double> A((size_t)d * d), piv(d);
			for (int i = 0; i < d; i++) for (int j = 0; j < d; j++) A[i * d + j] = (double)prior[i * d + j];
			double tr, la;
			if (frpbh_factor(d, A.data(), piv.data(), &tr, &la) != 0 || !(tr > 0)) { printf("bad factor d = %d\n", d); return 1; }
		}
	}
	long long lay[40];
	if (frpbh_layout(lay) != 32 || frpbh_ws_bytes(1100, 3) == 0) return 1;
	printf("ok\n");
	return 0;
}
#endif
