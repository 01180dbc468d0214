// tests/harness/fr_eval_harness.cpp -- TEST ONLY.
// Compiles the host/device-neutral arithmetic of fisher-nerf-customized_amd/csrc/fr_eval_math.h (over fr_loss_math.h) with g++ and
// runs it over whole views the way csrc/fr_eval.hip runs it over tiles: the same functions on the same operands, so the per-pixel
// values are the kernels' bit for bit; the sums are plain fp64 sums in index order (the kernels add per-tile partials: that order
// is the one freedom between the two).  Never loaded by the product.
#include <cmath>
#include <cstdint>
#include <vector>
#include "../../fisher-nerf-customized_amd/csrc/fr_eval_math.h"

namespace {

struct View {
	int H, W, u8, channels, clamp;
	const float* render; const void* gt; const uint8_t* mask;          // of this view
	// x, y of channel c as the metrics see them (zero outside the image)
	void load(int c, int py, int px, float& xv, float& yv) const
	{
		xv = 0.0f; yv = 0.0f;
		if (py < 0 || py >= H || px < 0 || px >= W) return;
		const size_t o = (size_t)py * W + px;
		const float m = (!mask || mask[o]) ? 1.0f : 0.0f;
		xv = fre_render(render[(size_t)c * H * W + o], clamp, m, mask != nullptr);
		const float t = u8 ? fre_byte(((const uint8_t*)gt)[o * channels + c]) : ((const float*)gt)[(size_t)c * H * W + o];
		yv = fre_target(t, m, mask != nullptr);
	}
};

}

extern "C" {

void fre_byte_table(float out[256])
{
	for (int b = 0; b < 256; b++) out[b] = fre_byte((uint8_t)b);
}

float fre_clamp_of(float v) { return fre_clamp01(v); }

void fre_summary(const float* rows, int V, float* summary)
{
	double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
	for (int v = 0; v < V; v++) fre_summary_add(acc, rows + (size_t)v * FRE_ROW);
	fre_summary_finish(acc, V, summary);
}

// rows [V][8], summary [8]; strides in elements as fr_view_metrics_cfg has them; depth / gt_depth both null or both given
int fre_view_metrics(int V, int H, int W, int u8, int channels, int clamp, int valid_only,
                     const float* render, long long render_vs, const float* depth, long long depth_vs, const void* gt,
                     const float* gt_depth, long long gt_depth_vs, const uint8_t* mask, float* rows, float* summary)
{
	const size_t hw = (size_t)H * W;
	const float zeros[FRL_WINDOW] = { 0.0f };
	float padrow[5];
	frl_conv11_moments(zeros, zeros, 1, padrow);       // the moments are taken about 0.5: a row of padding is not a row of zeros
	float padraw[5] = { 0.0f, 0.0f, 0.0f, 0.0f, 0.0f };  // the raw moments of a row of padding are zeros
	std::vector<float> hrows(5 * hw), hraw(5 * hw);
	for (int v = 0; v < V; v++)
	{
		const View im = { H, W, u8, channels, clamp, render + (size_t)v * render_vs,
		                  u8 ? (const void*)((const uint8_t*)gt + (size_t)v * hw * channels) : (const void*)((const float*)gt + (size_t)v * 3 * hw),
		                  mask ? mask + (size_t)v * hw : nullptr };
		double s[FRE_SUMS] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
		for (int c = 0; c < 3; c++)
		{
			for (int r = 0; r < H; r++)
				for (int px = 0; px < W; px++)
				{
					float wx[FRL_WINDOW], wy[FRL_WINDOW], h[5];
					for (int k = 0; k < FRL_WINDOW; k++) im.load(c, r, px - FRL_RADIUS + k, wx[k], wy[k]);
					frl_conv11_moments(wx, wy, 1, h);
					for (int k = 0; k < 5; k++) hrows[((size_t)k * H + r) * W + px] = h[k];
					fre_conv11_raw_moments(wx, wy, 1, h);
					for (int k = 0; k < 5; k++) hraw[((size_t)k * H + r) * W + px] = h[k];
				}
			for (int py = 0; py < H; py++)
				for (int px = 0; px < W; px++)
				{
					float mo[5], dmu, d11, d12, xv, yv;
					for (int k = 0; k < 5; k++)
					{
						float col[FRL_WINDOW];
						for (int j = 0; j < FRL_WINDOW; j++)
						{
							const int r = py - FRL_RADIUS + j;
							col[j] = (r < 0 || r >= H) ? padrow[k] : hrows[((size_t)k * H + r) * W + px];
						}
						mo[k] = frl_conv11(col, 1);
					}
					float ssim = frl_ssim_pixel(mo[0], mo[1], mo[2], mo[3], mo[4], dmu, d11, d12);
					if (fre_window_is_dark(mo[0], mo[1]))
					{
						for (int k = 0; k < 5; k++)
						{
							float col[FRL_WINDOW];
							for (int j = 0; j < FRL_WINDOW; j++)
							{
								const int r = py - FRL_RADIUS + j;
								col[j] = (r < 0 || r >= H) ? padraw[k] : hraw[((size_t)k * H + r) * W + px];
							}
							mo[k] = frl_conv11(col, 1);
						}
						ssim = fre_ssim_pixel_raw(mo[0], mo[1], mo[2], mo[3], mo[4]);
					}
					s[FRE_S_SSIM] += (double)ssim;
					im.load(c, py, px, xv, yv);
					s[FRE_S_MSE + c] += (double)fre_sq_diff(xv, yv);
				}
		}
		if (depth)
			for (size_t o = 0; o < hw; o++)
			{
				const float g = gt_depth[(size_t)v * gt_depth_vs + o];
				if (!fre_depth_counts(g, valid_only)) continue;
				const float m = (!mask || mask[(size_t)v * hw + o]) ? 1.0f : 0.0f;
				const float dd = fre_depth_diff(depth[(size_t)v * depth_vs + o], g, m, mask != nullptr);
				s[FRE_S_DL1] += (double)std::fabs(dd);
				s[FRE_S_DSQ] += (double)(dd * dd);
				s[FRE_S_DCNT] += 1.0;
			}
		fre_finalise_row(s, (double)hw, depth != nullptr, rows + (size_t)v * FRE_ROW);
	}
	fre_summary(rows, V, summary);
	return 0;
}

}
