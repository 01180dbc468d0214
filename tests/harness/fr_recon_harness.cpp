// g++ build of what the running reconstruction metrics add to csrc/fr_cloud_math.h -- the fold of a seed and a candidate, the
// "is this sample a query" predicate with a mask, the back-projection of one pixel -- and the layout of fr_cloud_query_cfg as a
// C++ compiler lays the public header's struct out (held against ctypes in tests/test_recon_stream_cpu.py).
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include "../../include/fisher_rast.h"
#include "../../fisher-nerf-customized_amd/csrc/fr_cloud_math.h"

extern "C" {

float frc_r_fold(float seed_d2, float d2) { return frc_fold(seed_d2, d2); }
int frc_r_fold_may_improve(float bound_d2, float best_d2) { return frc_fold_may_improve(bound_d2, best_d2); }
int frc_r_sample_is_query(float d, int has_mask, int mask_byte) { return frc_sample_is_query(d, has_mask, (uint8_t)mask_byte); }

// the fold of a whole frame, brute force: seeds [M] in and out against targets [N,3], as the kernel states it
void frc_r_fold_cloud(int N, const float* targets, int M, const float* queries, float* seed_d2)
{
	for (int m = 0; m < M; m++)
	{
		const float* q = queries + 3 * (size_t)m;
		if (!frc_finite3(q[0], q[1], q[2])) continue;
		for (int i = 0; i < N; i++)
		{
			const float* t = targets + 3 * (size_t)i;
			if (frc_finite3(t[0], t[1], t[2])) seed_d2[m] = frc_fold(seed_d2[m], frc_dist2(q[0], q[1], q[2], t[0], t[1], t[2]));
		}
	}
}

// out_points of the depth source: [Hs Ws, 3], three NaNs where the sample is no query; valid [Hs Ws] bytes
void frc_r_depth_points(int H, int W, int stride, int flip_z, const float* depth, const uint8_t* mask, const float* kinv, const float* c2w,
                        float* points, uint8_t* valid)
{
	const int Hs = (H + stride - 1) / stride, Ws = (W + stride - 1) / stride;
	for (int sy = 0; sy < Hs; sy++)
		for (int sx = 0; sx < Ws; sx++)
		{
			const int m = sy * Ws + sx, u = sx * stride, v = sy * stride;
			const size_t px = (size_t)v * W + u;
			float q[3] = {0.f, 0.f, 0.f};
			bool ok = frc_sample_is_query(depth[px], mask != nullptr, mask ? mask[px] : (uint8_t)1);
			if (ok)
			{
				frc_back_project(u, v, depth[px], kinv, c2w, flip_z, q);
				ok = frc_finite3(q[0], q[1], q[2]);
			}
			valid[m] = ok;
			for (int a = 0; a < 3; a++) points[3 * (size_t)m + a] = ok ? q[a] : NAN;
		}
}

// sizeof(fr_cloud_query_cfg), then the offset of every field in declaration order; returns the number of values written
int frc_r_cfg_layout(size_t* out)
{
	int n = 0;
	out[n++] = sizeof(fr_cloud_query_cfg);
#define FIELD(f) out[n++] = offsetof(fr_cloud_query_cfg, f)
	FIELD(source); FIELD(M); FIELD(H); FIELD(W); FIELD(stride); FIELD(flip_z); FIELD(dist_th);
	FIELD(queries); FIELD(depth); FIELD(kinv); FIELD(c2w); FIELD(out_dist); FIELD(out_idx); FIELD(out_flag); FIELD(out_stats);
	FIELD(seed_d2); FIELD(mask); FIELD(flag_near); FIELD(out_points);
#undef FIELD
	return n;
}

}
