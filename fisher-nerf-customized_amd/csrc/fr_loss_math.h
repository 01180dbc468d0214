// fr_loss_math.h -- the arithmetic of the fused image loss (fr_loss.hip), host/device-neutral: the kernels and the g++ harness
// (tests/harness/fr_loss_harness.cpp) compile these same functions, so a CPU run states the kernels' results bit for bit.
//
// The statement is the reference's `_ssim` (models/SLAM/utils/slam_external.py:100-120) with its 11 x 11 window applied as the
// two 11-tap passes it is the outer product of: horizontal first, then vertical, taps added in ascending order, zero padding,
// and with the window moments taken about 0.5 (below).
// Everything is binary32, one rounding per written operation (the build has -ffp-contract=off and an IEEE divide).
#ifndef FR_LOSS_MATH_H_INCLUDED
#define FR_LOSS_MATH_H_INCLUDED

#if defined(__HIPCC__)
#define FRL_HD __host__ __device__ __forceinline__
#else
#define FRL_HD inline
#endif

#define FRL_WINDOW 11
#define FRL_RADIUS 5

// gaussian(11, 1.5) of the reference (slam_external.py:77-79) as it comes out in binary32: 6 distinct values, g[k] = G|k - 5|
#define FRL_G0 0x1.106560p-2f      /* 0.26601171 (centre) */
#define FRL_G1 0x1.b43c3ep-3f      /* 0.21300553 */
#define FRL_G2 0x1.bff0fep-4f      /* 0.10936069 */
#define FRL_G3 0x1.26eb18p-5f      /* 0.03600077 */
#define FRL_G4 0x1.f1fe02p-8f      /* 0.00759876 */
#define FRL_G5 0x1.0d956cp-10f     /* 0.00102838 */

#define FRL_C1 1.0e-4f             /* 0.01 ^ 2 */
#define FRL_C2 9.0e-4f             /* 0.03 ^ 2 */

FRL_HD float frl_tap(int k)
{
	switch (k < FRL_RADIUS ? FRL_RADIUS - k : k - FRL_RADIUS)
	{
	case 0: return FRL_G0;
	case 1: return FRL_G1;
	case 2: return FRL_G2;
	case 3: return FRL_G3;
	case 4: return FRL_G4;
	default: return FRL_G5;
	}
}

// one 11-tap pass over a[0], a[stride], ..: ((g0 a0 + g1 a1) + g2 a2) + .. + g10 a10 -- all 11 taps, always
FRL_HD float frl_conv11(const float* a, int stride)
{
	float s = FRL_G5 * a[0] + FRL_G4 * a[stride];
	s = s + FRL_G3 * a[2 * stride];
	s = s + FRL_G2 * a[3 * stride];
	s = s + FRL_G1 * a[4 * stride];
	s = s + FRL_G0 * a[5 * stride];
	s = s + FRL_G1 * a[6 * stride];
	s = s + FRL_G2 * a[7 * stride];
	s = s + FRL_G3 * a[8 * stride];
	s = s + FRL_G4 * a[9 * stride];
	s = s + FRL_G5 * a[10 * stride];
	return s;
}

// The window moments are taken ABOUT 0.5, the middle of a colour's range: the filtered quantities are x~ = x - 0.5, y~ = y - 0.5,
// x~ x~, y~ y~, x~ y~ (padding: x = 0, so x~ = -0.5 there).  In exact arithmetic this changes nothing -- with S = (sum of the taps)^2,
// the weight of a whole window, mu = M + 0.5 S and E[x y] - mu1 mu2 = (E12 - M1 M2) + 0.5 (1 - S)(M1 + M2) + 0.25 S (1 - S) -- but
// in binary32 the raw second moments of a colour near 0.75 carry an absolute error of ~1e-7, which sigma^2 + c2 ~ 1e-3 turns into a
// relative 1e-4 of the term and of its gradient; about 0.5 the second moments are nine times smaller and so is that error.
// S is a property of the 11 literals above (S - 1 = -6.24e-8); the three constants below are 0.5 S, 0.5 (1 - S), 0.25 S (1 - S),
// formed exactly from the taps and rounded once.
#define FRL_MID 0.5f
#define FRL_AS 0x1.fffffep-2f       /* 0.49999997 */
#define FRL_AK1 0x1.0cp-25f         /* 3.1199306e-08 */
#define FRL_A2K2 0x1.0bfffep-26f    /* 1.5599651e-08 */

// the horizontal pass of the forward over one row window x[0..10], y[0..10] (zero outside the image): the five filtered rows
// x~, y~, x~ x~, y~ y~, x~ y~ (the products are formed in binary32 first, as `img1 * img1` is)
FRL_HD void frl_conv11_moments(const float* x, const float* y, int stride, float out[5])
{
	float xc[FRL_WINDOW], yc[FRL_WINDOW], xx[FRL_WINDOW], yy[FRL_WINDOW], xy[FRL_WINDOW];
	for (int k = 0; k < FRL_WINDOW; k++)
	{
		const float a = x[k * stride] - FRL_MID, b = y[k * stride] - FRL_MID;
		xc[k] = a; yc[k] = b;
		xx[k] = a * a; yy[k] = b * b; xy[k] = a * b;
	}
	out[0] = frl_conv11(xc, 1);
	out[1] = frl_conv11(yc, 1);
	out[2] = frl_conv11(xx, 1);
	out[3] = frl_conv11(yy, 1);
	out[4] = frl_conv11(xy, 1);
}

// One pixel's SSIM term m from the five window moments about 0.5 (M1 = E[x~], M2 = E[y~], E11 = E[x~ x~], E22, E12) and the three
// partials the backward needs, with M1, E11, E12 as the independent variables (x enters through these three only):
//   mu = M + 0.5 S,  s1 = (E11 - M1^2) + (2 k M1 + q),  s12 = (E12 - M1 M2) + (k (M1 + M2) + q),  k = 0.5 (1 - S), q = 0.25 S (1 - S)
//   m   = (A1 A2) / (B1 B2),  A1 = 2 mu1 mu2 + c1,  A2 = 2 s12 + c2,  B1 = mu1^2 + mu2^2 + c1,  B2 = s1 + s2 + c2
//   d11 = dm/dE11 = -m / B2
//   d12 = dm/dE12 = 2 (A1 / B1) / B2
//   dM  = dm/dM1 (total) = 2 (mu2 (A2 / B2) - mu1 m) / B1 + (d11 2 (k - M1) + d12 (k - M2))
// The partials are written so that render == target gives d12 = -2 d11 and dM = 0 EXACTLY (then A1 = B1, A2 = B2 and m = 1 bit
// for bit), i.e. a gradient of exactly 0 where the exact gradient is 0, instead of the rounding noise of three large terms.
FRL_HD float frl_ssim_pixel(float M1, float M2, float E11, float E22, float E12, float& dM, float& d11, float& d12)
{
	const float mu1 = M1 + FRL_AS, mu2 = M2 + FRL_AS;
	const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
	const float s1 = (E11 - M1 * M1) + ((2.0f * FRL_AK1) * M1 + FRL_A2K2);
	const float s2 = (E22 - M2 * M2) + ((2.0f * FRL_AK1) * M2 + FRL_A2K2);
	const float s12 = (E12 - M1 * M2) + (FRL_AK1 * (M1 + M2) + FRL_A2K2);
	const float A1 = 2.0f * mu1_mu2 + FRL_C1;
	const float A2 = 2.0f * s12 + FRL_C2;
	const float B1 = (mu1_sq + mu2_sq) + FRL_C1;
	const float B2 = (s1 + s2) + FRL_C2;
	const float m = (A1 * A2) / (B1 * B2);
	d11 = -(m / B2);
	d12 = (2.0f * (A1 / B1)) / B2;
	const float t1 = FRL_AK1 - M1, t2 = FRL_AK1 - M2;
	dM = (2.0f * (mu2 * (A2 / B2) - mu1 * m)) / B1 + (d11 * (2.0f * t1) + d12 * t2);
	return m;
}

// torch's sign for abs': sign(0) = 0
FRL_HD float frl_sign(float d)
{
	return d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
}

// dL/dx at one pixel: `gl1` = upstream * w_l1 / denominator, `s` = -(upstream * w_ssim / normaliser), D* = the window sums of the
// three saved partial maps at this pixel, (x, y) the (masked) render and target (the SSIM part takes them about 0.5, as the moments are)
FRL_HD float frl_pixel_grad(float gl1, float s, float x, float y, float DM, float D11, float D12, bool ssim)
{
	float g = gl1 * frl_sign(x - y);
	if (ssim) g = g + s * ((DM + (2.0f * (x - FRL_MID)) * D11) + (y - FRL_MID) * D12);
	return g;
}

#endif
