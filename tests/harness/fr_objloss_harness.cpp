// g++ build of the object-aware training step's arithmetic (csrc/fr_objloss_math.h) for CPU-side checks: the per-element functions
// are the header's, the same ones the kernels compile.  The median (a partial sort of the bit patterns) and the min / max of the
// outside mask are plain loops -- what the radix select and the shuffle / LDS reductions of csrc/fr_objloss.hip have to reproduce;
// the fp64 sums of the penalties are added in the kernels' own order (threads, shuffle tree, waves, partials), so that they compare
// bit for bit.
#include <algorithm>
#include <cstdint>
#include <vector>
#include "../../fisher-nerf-customized_amd/csrc/fr_objloss_math.h"

namespace {

const int THREADS = 256, ITEMS = 4;           // FRO_THREADS, FRO_SUM_ITEMS of csrc/fr_objloss.hip

// lane 0 of a wave after `for (o = 32; o > 0; o >>= 1) v += shfl_down(v, o)`
double wave_tree(double* v)
{
	for (int o = 32; o > 0; o >>= 1)
		for (int l = 0; l < o; l++) v[l] += v[l + o];
	return v[0];
}

}

extern "C" {

// mask [H W] bytes, status [5] = {kept, median is NaN, background pixels, 0, median bits}; obj null: no object mask
void fro_loss_mask(int H, int W, float sil_thres, int reject, float ratio, int presence, const float* depth_sil, const float* gt,
                   const uint8_t* obj, uint8_t* mask, int32_t* status)
{
	const size_t n = (size_t)H * W;
	uint32_t med = 0u;
	int has_nan = 0;
	float thr = 0.0f;
	if (reject)
	{
		std::vector<uint32_t> bits;
		bits.reserve(n);
		for (size_t p = 0; p < n; p++)
		{
			const float e = fro_depth_error(gt[p], depth_sil[p]);
			if (e != e) has_nan = 1;
			else bits.push_back(fro_bits(e));
		}
		if (has_nan) med = FRO_NAN_BITS;
		else
		{
			std::nth_element(bits.begin(), bits.begin() + (n - 1) / 2, bits.end());
			med = bits[(n - 1) / 2];
		}
		thr = fro_threshold(ratio, fro_float(med));
	}
	int32_t kept = 0, back = 0;
	for (size_t p = 0; p < n; p++)
	{
		const uint8_t o = obj ? obj[p] : (uint8_t)1;
		const bool keep = fro_keep(depth_sil[p], depth_sil[n + p], depth_sil[2 * n + p], gt[p], reject != 0, thr, presence != 0, sil_thres,
		                           obj != nullptr, o);
		mask[p] = keep ? 1 : 0;
		kept += keep ? 1 : 0;
		back += (obj && o == 0) ? 1 : 0;
	}
	status[0] = kept; status[1] = has_nan; status[2] = back; status[3] = 0; status[4] = (int32_t)med;
}

// out4, saved2 as fr_bg_penalty_forward writes them
void fro_penalty_forward(int H, int W, float lambda_rgb, float lambda_alpha, const float* im, const float* depth_sil, const uint8_t* obj,
                         float* out4, float* saved2)
{
	const size_t n = (size_t)H * W;
	const int T = (int)((n + THREADS * ITEMS - 1) / (THREADS * ITEMS));
	std::vector<double> partials((size_t)3 * T);
	for (int wg = 0; wg < T; wg++)
	{
		double v[3][THREADS];
		for (int tid = 0; tid < THREADS; tid++)
		{
			double a[3] = {0.0, 0.0, 0.0};
			for (int i = 0; i < ITEMS; i++)
			{
				const size_t p = (size_t)wg * THREADS * ITEMS + (size_t)i * THREADS + tid;
				if (p >= n) continue;
				const float bg = fro_background(obj[p]);
				for (int c = 0; c < 3; c++) a[0] += (double)fro_rgb_term(im[c * n + p], bg);
				a[1] += (double)fro_alpha_term(depth_sil[n + p], bg);
				a[2] += (double)bg;
			}
			for (int q = 0; q < 3; q++) v[q][tid] = a[q];
		}
		for (int q = 0; q < 3; q++)
		{
			double w[4];
			for (int k = 0; k < 4; k++) w[k] = wave_tree(&v[q][64 * k]);
			partials[(size_t)q * T + wg] = ((w[0] + w[1]) + w[2]) + w[3];
		}
	}
	double rows[3];
	for (int q = 0; q < 3; q++)
	{
		double lanes[64];
		for (int l = 0; l < 64; l++)
		{
			double s = 0.0;
			for (int t = l; t < T; t += 64) s += partials[(size_t)q * T + t];
			lanes[l] = s;
		}
		rows[q] = wave_tree(lanes);
	}
	fro_penalty_finish(rows[0], rows[1], rows[2], lambda_rgb, lambda_alpha, out4, saved2);
}

// dL_dim [3,H,W], dL_dds [3,H,W] as fr_bg_penalty_backward writes them
void fro_penalty_backward(int H, int W, float lambda_rgb, float lambda_alpha, const float* im, const float* depth_sil, const uint8_t* obj,
                          const float* saved2, float upstream, float* dL_dim, float* dL_dds)
{
	const size_t n = (size_t)H * W;
	const float f_rgb = fro_grad_factor(upstream, lambda_rgb, saved2[0]), f_alpha = fro_grad_factor(upstream, lambda_alpha, saved2[1]);
	for (size_t p = 0; p < n; p++)
	{
		const float bg = fro_background(obj[p]);
		for (int c = 0; c < 3; c++) dL_dim[c * n + p] = fro_rgb_grad(f_rgb, bg, im[c * n + p]);
		dL_dds[p] = 0.0f;
		dL_dds[n + p] = fro_alpha_grad(f_alpha, bg, depth_sil[n + p]);
		dL_dds[2 * n + p] = 0.0f;
	}
}

// outside [P] bytes, status [6] as fr_outside_mask writes them
void fro_outside_mask(int P, int cols, const float* means, const float* logs, const float* w2c, const float* intr, const uint8_t* obj,
                      int H, int W, uint8_t* outside, int32_t* status)
{
	uint32_t cnt[2] = {0u, 0u}, nan[2] = {0u, 0u}, kmin[2] = {0xffffffffu, 0xffffffffu}, kmax[2] = {0u, 0u};
	for (int i = 0; i < P; i++)
	{
		int iu, iv;
		const bool in_img = fro_project(w2c, intr, means[3 * (size_t)i], means[3 * (size_t)i + 1], means[3 * (size_t)i + 2], W, H, iu, iv);
		const bool inside = in_img && obj[(size_t)iv * W + iu] != 0;
		outside[i] = inside ? 0 : 1;
		const int s = inside ? 0 : 1;
		const float ls = fro_row_log_scale(logs + (size_t)i * cols, cols);
		cnt[s]++;
		if (ls != ls) nan[s]++;
		else
		{
			const uint32_t key = fro_order_key(ls);
			kmin[s] = std::min(kmin[s], key);
			kmax[s] = std::max(kmax[s], key);
		}
	}
	uint32_t r[4];
	fro_range_bits(cnt[0], nan[0], kmin[0], kmax[0], &r[0], &r[1]);
	fro_range_bits(cnt[1], nan[1], kmin[1], kmax[1], &r[2], &r[3]);
	status[0] = (int32_t)cnt[0]; status[1] = (int32_t)cnt[1];
	for (int j = 0; j < 4; j++) status[2 + j] = (int32_t)r[j];
}

}
