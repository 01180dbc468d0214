// tests/harness/fr_loss_harness.cpp -- TEST ONLY.
// Compiles the host/device-neutral arithmetic of fisher-nerf-customized_amd/csrc/fr_loss_math.h with g++ and runs it over whole
// images the way csrc/fr_loss.hip runs it over tiles (the same functions on the same operands, so the per-pixel results are the
// kernels' bit for bit); the sums are plain fp64 sums in index order.  Never loaded by the product.
#include <cmath>
#include <cstdint>
#include <vector>
#include "../../fisher-nerf-customized_amd/csrc/fr_loss_math.h"

namespace {

struct Img {
	int C, H, W;
	const float* x; const float* y; const uint8_t* mask; int mask_channels; int weights_map;
	// x, y as the loss sees them: zero outside the image, times the mask where it multiplies the images
	void load(int c, int py, int px, float& xv, float& yv, float& m) const
	{
		xv = 0.0f; yv = 0.0f; m = 0.0f;
		if (py < 0 || py >= H || px < 0 || px >= W) return;
		const size_t o = (size_t)py * W + px, oc = (size_t)c * H * W + o;
		xv = x[oc]; yv = y[oc]; m = 1.0f;
		if (mask)
		{
			m = mask[(mask_channels > 1 ? (size_t)c * H * W : 0) + o] ? 1.0f : 0.0f;
			if (!weights_map) { xv = xv * m; yv = yv * m; }
		}
	}
};

// the separable window over `n_maps` maps of one channel: horizontal pass for every row, then vertical; a row outside the image is
// `padrow` (what the horizontal pass gives on a row of padding), or 0 where there is none
void window(int H, int W, int n_maps, const std::vector<float>& hrows, int py, int px, float* out, const float* padrow = nullptr)
{
	for (int k = 0; k < n_maps; k++)
	{
		float col[FRL_WINDOW];
		for (int j = 0; j < FRL_WINDOW; j++)
		{
			const int r = py - FRL_RADIUS + j;
			col[j] = (r < 0 || r >= H) ? (padrow ? padrow[k] : 0.0f) : hrows[((size_t)k * H + r) * W + px];
		}
		out[k] = frl_conv11(col, 1);
	}
}

}

extern "C" {

void frl_taps(float out[FRL_WINDOW])
{
	for (int k = 0; k < FRL_WINDOW; k++) out[k] = frl_tap(k);
}

float frl_sign_of(float d) { return frl_sign(d); }

// out[4] = {loss, L1 term, SSIM mean, count} in fp64; ssim_map [C,H,W] and channel_ssim [C] may be null;
// saved: (w_ssim != 0 ? 3 C H W : 0) + 4 floats, as fr_image_loss_forward lays them out
int frl_forward(int C, int H, int W, float w_l1, float w_ssim, int denom_mode, int mask_channels, int weights_map,
                const float* x, const float* y, const uint8_t* mask, double* out, double* channel_ssim, float* ssim_map, float* saved)
{
	const Img im = { C, H, W, x, y, mask_channels ? mask : nullptr, mask_channels, weights_map };
	const bool ssim = w_ssim != 0.0f;
	const size_t n = (size_t)C * H * W;
	double q_ssim = 0.0, q_l1 = 0.0, q_cnt = 0.0;
	std::vector<float> hrows((size_t)5 * H * W);
	const float zeros[FRL_WINDOW] = { 0.0f };
	float padrow[5];
	frl_conv11_moments(zeros, zeros, 1, padrow);       // the moments are taken about 0.5: a row of padding is not a row of zeros
	for (int c = 0; c < C; c++)
	{
		if (ssim)
			for (int r = 0; r < H; r++)
				for (int px = 0; px < W; px++)
				{
					float wx[FRL_WINDOW], wy[FRL_WINDOW], m, h[5];
					for (int k = 0; k < FRL_WINDOW; k++) im.load(c, r, px - FRL_RADIUS + k, wx[k], wy[k], m);
					frl_conv11_moments(wx, wy, 1, h);
					for (int k = 0; k < 5; k++) hrows[((size_t)k * H + r) * W + px] = h[k];
				}
		double c_ssim = 0.0;
		for (int py = 0; py < H; py++)
			for (int px = 0; px < W; px++)
			{
				float xv, yv, m;
				im.load(c, py, px, xv, yv, m);
				const size_t o = ((size_t)c * H + py) * W + px;
				if (ssim)
				{
					float mo[5], dmu, d11, d12;
					window(H, W, 5, hrows, py, px, mo, padrow);
					float s = frl_ssim_pixel(mo[0], mo[1], mo[2], mo[3], mo[4], dmu, d11, d12);
					if (im.mask && weights_map && m == 0.0f) { s = 0.0f; dmu = 0.0f; d11 = 0.0f; d12 = 0.0f; }
					if (ssim_map) ssim_map[o] = s;
					saved[o] = dmu; saved[n + o] = d11; saved[2 * n + o] = d12;
					c_ssim += (double)s;
				}
				if (m != 0.0f) { q_l1 += (double)std::fabs(xv - yv); q_cnt += 1.0; }
			}
		if (channel_ssim) channel_ssim[c] = c_ssim / ((double)H * W);
		q_ssim += c_ssim;
	}
	const double nn = (double)n;
	const double denom = denom_mode == 0 ? 1.0 : (denom_mode == 1 ? nn : q_cnt);
	const double norm = weights_map ? (q_cnt > (double)C ? q_cnt : (double)C) : nn;
	const double l1 = q_l1 / denom, sm = q_ssim / norm;
	double loss = 0.0;
	if (w_l1 != 0.0f) loss += (double)w_l1 * l1;
	if (w_ssim != 0.0f) loss += (double)w_ssim * (1.0 - sm);
	out[0] = loss; out[1] = l1; out[2] = sm; out[3] = q_cnt;
	float* tail = saved + (ssim ? 3 * n : 0);
	tail[0] = (float)((double)w_l1 / denom); tail[1] = (float)((double)w_ssim / norm); tail[2] = 0.0f; tail[3] = 0.0f;
	return 0;
}

int frl_backward(int C, int H, int W, float w_ssim, int mask_channels, int weights_map,
                 const float* x, const float* y, const uint8_t* mask, const float* saved, float upstream, float* dL_dx)
{
	const Img im = { C, H, W, x, y, mask_channels ? mask : nullptr, mask_channels, weights_map };
	const bool ssim = w_ssim != 0.0f;
	const size_t n = (size_t)C * H * W;
	const float* tail = saved + (ssim ? 3 * n : 0);
	std::vector<float> hrows((size_t)3 * H * W);
	for (int c = 0; c < C; c++)
	{
		if (ssim)
			for (int k = 0; k < 3; k++)
				for (int r = 0; r < H; r++)
					for (int px = 0; px < W; px++)
					{
						float w[FRL_WINDOW];
						for (int j = 0; j < FRL_WINDOW; j++)
						{
							const int q = px - FRL_RADIUS + j;
							w[j] = (q < 0 || q >= W) ? 0.0f : saved[k * n + ((size_t)c * H + r) * W + q];
						}
						hrows[((size_t)k * H + r) * W + px] = frl_conv11(w, 1);
					}
		for (int py = 0; py < H; py++)
			for (int px = 0; px < W; px++)
			{
				float D[3] = { 0.0f, 0.0f, 0.0f }, xv, yv, m;
				if (ssim) window(H, W, 3, hrows, py, px, D);
				im.load(c, py, px, xv, yv, m);
				float g = frl_pixel_grad(upstream * tail[0], -(upstream * tail[1]), xv, yv, D[0], D[1], D[2], ssim);
				if (im.mask && !weights_map && m == 0.0f) g = 0.0f;
				dL_dx[((size_t)c * H + py) * W + px] = g;
			}
	}
	return 0;
}

}
