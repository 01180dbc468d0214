// fr_eval_math.h -- the arithmetic of the render-quality evaluation (fr_eval.hip), host/device-neutral: the kernels and the g++
// harness (tests/harness/fr_eval_harness.cpp) compile these same functions, so a CPU run states the kernels' per-pixel results
// bit for bit and their sums up to the order of a binary64 addition.
//
// The statement is the reference's evaluation of a rendered view against its ground truth
// (tester_gaussians_navigation.py:1450-1491, models/SLAM/utils/eval_helpers.py:230-257):
//   colour   color.clamp_(0, 1);  rgb_gt = rgb[:, :, :3] / 255;  with a presence mask both images are multiplied by it
//   PSNR     calc_psnr(color, rgb_gt).mean(): per channel 20 log10(1 / sqrt(mean((x - y)^2))), then the mean of the three
//   SSIM     the mean of the SSIM map (fr_loss_math.h: frl_conv11_moments, frl_conv11, frl_ssim_pixel, unchanged; a window that is
//            black in one image takes the raw-moment statement instead: fre_window_is_dark below)
//   depth    mean |d - d_gt| over all pixels, or the sum where d_gt > 0 over their count; with a mask the difference is multiplied
// Per pixel everything is binary32, one rounding per written operation (the build has -ffp-contract=off and an IEEE divide);
// every sum is binary64 and a row is finalised in binary64 before its one rounding to float.
//
// The reference's own "RMSE" (eval_helpers.py:242-251) takes the square root of EACH square and sums those, which is its L1 again;
// depth_rmse here is sqrt(sum (d - d_gt)^2 / denominator), what the name says.
#ifndef FR_EVAL_MATH_H_INCLUDED
#define FR_EVAL_MATH_H_INCLUDED

#include <math.h>
#include <stdint.h>
#include "fr_loss_math.h"

#define FRE_HD FRL_HD

#define FRE_ROW 8            /* {psnr, ssim, depth_l1, depth_rmse, mse_r, mse_g, mse_b, depth_count} */
#define FRE_SUMS 7           /* a view's binary64 sums: (x - y)^2 per channel, the SSIM map, |dd|, dd^2, the depth count */
#define FRE_S_MSE 0
#define FRE_S_SSIM 3
#define FRE_S_DL1 4
#define FRE_S_DSQ 5
#define FRE_S_DCNT 6

// torch.clamp(v, 0, 1): a NaN stays a NaN (fminf / fmaxf would return the bound)
FRE_HD float fre_clamp01(float v)
{
	return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
}

// a byte of Habitat's rgb as `rgb / 255` gives it in binary32: the correctly rounded quotient
FRE_HD float fre_byte(uint8_t b)
{
	return (float)b / 255.0f;
}

// the render and the target as the metrics see them: clamp first (the render only), then the mask (m = 0 or 1) on both
FRE_HD float fre_render(float v, int clamp, float m, int masked)
{
	if (clamp) v = fre_clamp01(v);
	return masked ? v * m : v;
}

FRE_HD float fre_target(float v, float m, int masked)
{
	return masked ? v * m : v;
}

// Where fr_loss_math.h's pivot does not serve.  Its moments about 0.5 carry an ABSOLUTE error of ~2^-25 in each mean and in each
// centred second moment whatever the window holds.  Over a window that is black in one image (an all-black Habitat frame, a masked
// region) the exact mu is ~0, 2 mu1 mu2 + c1 is c1 = 1e-4, and that absolute error becomes a relative 1e-5 .. 1e-4 of the term (measured:
// 19 times the tolerance rule's bound), while the reference's raw moments are bounded by the small mean and are exact to ~1e-9.
// So a pixel whose window mean of EITHER image is below 2^-5 takes the reference's own statement in raw moments (pivot 0), and
// every other pixel fr_loss_math.h's, bit for bit.  The zero-padded corner of a mid-grey image has a window mean of ~0.15: ordinary
// images never come here.  A NaN mean is not below the threshold.
#define FRE_DARK_MEAN 0x1p-5f

FRE_HD bool fre_window_is_dark(float M1, float M2)
{
	const float mu1 = M1 + FRL_AS, mu2 = M2 + FRL_AS;
	return mu1 < FRE_DARK_MEAN || mu2 < FRE_DARK_MEAN;
}

// the horizontal pass of the raw moments over one row window: the filtered rows x, y, x x, y y, x y
FRE_HD void fre_conv11_raw_moments(const float* x, const float* y, int stride, float out[5])
{
	float xx[FRL_WINDOW], yy[FRL_WINDOW], xy[FRL_WINDOW];
	for (int k = 0; k < FRL_WINDOW; k++)
	{
		const float a = x[k * stride], b = y[k * stride];
		xx[k] = a * a; yy[k] = b * b; xy[k] = a * b;
	}
	out[0] = frl_conv11(x, stride);
	out[1] = frl_conv11(y, stride);
	out[2] = frl_conv11(xx, 1);
	out[3] = frl_conv11(yy, 1);
	out[4] = frl_conv11(xy, 1);
}

// one pixel's SSIM term from the raw window moments, as slam_external.py:104-115 writes it
FRE_HD float fre_ssim_pixel_raw(float mu1, float mu2, float E11, float E22, float E12)
{
	const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
	const float s1 = E11 - mu1_sq, s2 = E22 - mu2_sq, s12 = E12 - mu1_mu2;
	return ((2.0f * mu1_mu2 + FRL_C1) * (2.0f * s12 + FRL_C2)) / (((mu1_sq + mu2_sq) + FRL_C1) * ((s1 + s2) + FRL_C2));
}

// (x - y) ** 2 of calc_psnr / calc_mse
FRE_HD float fre_sq_diff(float x, float y)
{
	const float d = x - y;
	return d * d;
}

// (depth - depth_gt) [* mask]; |.| and its square are taken of this value
FRE_HD float fre_depth_diff(float d, float g, float m, int masked)
{
	const float dd = d - g;
	return masked ? dd * m : dd;
}

// whether a pixel enters the depth sums: every pixel, or those with a measured depth (valid_depth_mask = depth_gt > 0)
FRE_HD bool fre_depth_counts(float g, int valid_only)
{
	return !valid_only || g > 0.0f;
}

FRE_HD float fre_nan()
{
	return __builtin_nanf("");
}

// One view's row from its sums.  hw = H W.  Without depth the three depth entries and the count are NaN.
// valid-only with no valid pixel: 0 / 0 = NaN, as torch's sum() / sum() gives.
FRE_HD void fre_finalise_row(const double s[FRE_SUMS], double hw, int has_depth, float row[FRE_ROW])
{
	double psnr = 0.0;
	for (int c = 0; c < 3; c++)
	{
		const double mse = s[FRE_S_MSE + c] / hw;
		psnr += 20.0 * log10(1.0 / sqrt(mse));
		row[4 + c] = (float)mse;
	}
	row[0] = (float)(psnr / 3.0);
	row[1] = (float)(s[FRE_S_SSIM] / (3.0 * hw));
	if (has_depth)
	{
		const double n = s[FRE_S_DCNT];
		row[2] = (float)(s[FRE_S_DL1] / n);
		row[3] = (float)sqrt(s[FRE_S_DSQ] / n);
		row[7] = (float)n;
	}
	else
	{
		row[2] = fre_nan(); row[3] = fre_nan(); row[7] = fre_nan();
	}
}

// The keep rule of eval_navigation (tester_gaussians_navigation.py:1484): a view is left out when torch.isinf(psnr); a NaN stays in.
FRE_HD bool fre_kept(float psnr)
{
	return !(psnr == INFINITY || psnr == -INFINITY);
}

// the running sums of the summary: acc = {kept, psnr, ssim, depth_l1, depth_rmse}, one row added at a time in index order
FRE_HD void fre_summary_add(double acc[5], const float row[FRE_ROW])
{
	if (!fre_kept(row[0])) return;
	acc[0] += 1.0;
	for (int k = 0; k < 4; k++) acc[1 + k] += (double)row[k];
}

// summary = {views kept, mean psnr, mean ssim, mean depth_l1, mean depth_rmse, 0, 0, V}; no view kept: 0 / 0 = NaN
FRE_HD void fre_summary_finish(const double acc[5], int V, float out[FRE_ROW])
{
	out[0] = (float)acc[0];
	for (int k = 0; k < 4; k++) out[1 + k] = (float)(acc[1 + k] / acc[0]);
	out[5] = 0.0f; out[6] = 0.0f; out[7] = (float)V;
}

#endif
