// fr_objloss_math.h -- the arithmetic of the object-aware training step (fr_objloss.hip), host/device-neutral: the kernels and the
// g++ harness (tests/harness/fr_objloss_harness.cpp) compile these same functions, so a CPU run states the kernels' results bit for
// bit.
//
// The statement is the reference's get_loss of the object class (models/SLAM/gaussian_object.py:213-275) and its
// get_gaussians_outside_mask (models/SLAM/utils/slam_external.py:270-343).  Everything per element is binary32, one rounding per
// written operation (the build has -ffp-contract=off and an IEEE divide), and every operand order is the one written here.
#ifndef FR_OBJLOSS_MATH_H_INCLUDED
#define FR_OBJLOSS_MATH_H_INCLUDED

#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define FRO_HD __host__ __device__ __forceinline__
#else
#define FRO_HD inline
#endif

#define FRO_NAN_BITS 0x7fc00000u      /* a NaN median or scale range, whatever the NaN's own bits were */

FRO_HD uint32_t fro_bits(float v) { uint32_t u; memcpy(&u, &v, 4); return u; }
FRO_HD float fro_float(uint32_t u) { float v; memcpy(&v, &u, 4); return v; }

// ---- the loss pixel mask (gaussian_object.py:213-248) ----------------------------------------------------------------------------

// |gt - render| where a depth was measured, 0 elsewhere (225).  The product is taken literally: an infinite or NaN difference times
// 0 is NaN, as torch's is.  Never negative, so the order of the bit patterns is the order of the values.
FRO_HD float fro_depth_error(float gt, float render)
{
	return fabsf(gt - render) * (gt > 0.0f ? 1.0f : 0.0f);
}

FRO_HD float fro_threshold(float ratio, float median) { return ratio * median; }

// one pixel of the mask; thr = fro_threshold(outlier_ratio, median) is read with reject_outliers only, sil_thres with need_presence
FRO_HD bool fro_keep(float render, float sil, float render_sq, float gt, bool reject_outliers, float thr, bool need_presence,
                     float sil_thres, bool has_obj, uint8_t obj)
{
	bool keep = gt > 0.0f;
	if (reject_outliers) keep &= fro_depth_error(gt, render) < thr;
	const float sq = render * render;
	const float var = render_sq - sq;                      // two roundings: inf - inf is NaN
	keep &= !(render != render) & !(var != var);
	if (need_presence) keep &= sil > sil_thres;
	if (has_obj) keep &= obj != 0;
	return keep;
}

// ---- the background penalties (gaussian_object.py:263-275) -----------------------------------------------------------------------

FRO_HD float fro_background(uint8_t obj) { return obj == 0 ? 1.0f : 0.0f; }

// torch's clamp(min=0, max=1): a NaN stays, an infinity goes to its end
FRO_HD float fro_clamp01(float v) { return v != v ? v : (v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v)); }

FRO_HD float fro_rgb_term(float im, float bg) { return fabsf(im) * bg; }
FRO_HD float fro_alpha_term(float sil, float bg) { return fro_clamp01(sil) * bg; }

// out4 = {lambda_rgb L_rgb + lambda_alpha L_alpha, L_rgb, L_alpha, n}, saved2 = the two denominators, from the fp64 sums
FRO_HD void fro_penalty_finish(double s_rgb, double s_alpha, double n, float lambda_rgb, float lambda_alpha, float* out4, float* saved2)
{
	const double d_rgb = 3.0 * n > 1.0 ? 3.0 * n : 1.0, d_alpha = n > 1.0 ? n : 1.0;
	const float l_rgb = (float)(s_rgb / d_rgb), l_alpha = (float)(s_alpha / d_alpha);
	const float a = lambda_rgb * l_rgb, b = lambda_alpha * l_alpha;
	out4[0] = a + b; out4[1] = l_rgb; out4[2] = l_alpha; out4[3] = (float)n;
	saved2[0] = (float)d_rgb; saved2[1] = (float)d_alpha;
}

// the factor of a penalty's gradient: (upstream lambda) / denominator, autograd's order (mul, then div)
FRO_HD float fro_grad_factor(float upstream, float lambda, float denom)
{
	const float g = upstream * lambda;
	return g / denom;
}

// abs': sgn(im), 0 at +-0 and at NaN; the products as autograd takes them (times the mask, then times the sign)
FRO_HD float fro_rgb_grad(float factor, float bg, float im)
{
	const float s = im > 0.0f ? 1.0f : (im < 0.0f ? -1.0f : 0.0f);
	const float g = factor * bg;
	return g * s;
}

// clamp': the gradient where 0 <= sil <= 1 (both ends included), 0 elsewhere and at NaN -- selected, not multiplied
FRO_HD float fro_alpha_grad(float factor, float bg, float sil)
{
	const float g = factor * bg;
	return (sil >= 0.0f && sil <= 1.0f) ? g : 0.0f;
}

// ---- the outside mask (slam_external.py:290-315) ---------------------------------------------------------------------------------

// w2c [4,4] and k [3,3] row-major.  Returns whether the Gaussian projects into the image; (iu, iv) is then the pixel that the
// reference looks up: round half to even (torch.round), clamped to the image.
FRO_HD bool fro_project(const float* w2c, const float* k, float x, float y, float z, int W, int H, int& iu, int& iv)
{
	const float X = ((w2c[0] * x + w2c[1] * y) + w2c[2] * z) + w2c[3];
	const float Y = ((w2c[4] * x + w2c[5] * y) + w2c[6] * z) + w2c[7];
	const float Z = ((w2c[8] * x + w2c[9] * y) + w2c[10] * z) + w2c[11];
	const float p0 = (k[0] * X + k[1] * Y) + k[2] * Z;
	const float p1 = (k[3] * X + k[4] * Y) + k[5] * Z;
	const float p2 = (k[6] * X + k[7] * Y) + k[8] * Z;
	const float den = p2 != p2 ? p2 : (p2 < 1e-6f ? 1e-6f : p2);       // clamp_min(1e-6): a NaN stays
	const float u = p0 / den, v = p1 / den;
	const bool in_img = (Z > 0.0f) & (u >= 0.0f) & (u < (float)W) & (v >= 0.0f) & (v < (float)H);
	iu = 0; iv = 0;
	if (in_img)
	{
		const float ru = rintf(u), rv = rintf(v);                     // u < W <= 2^30: the conversions are exact
		iu = (int)ru; iv = (int)rv;
		iu = iu < 0 ? 0 : (iu > W - 1 ? W - 1 : iu);
		iv = iv < 0 ? 0 : (iv > H - 1 ? H - 1 : iv);
	}
	return in_img;
}

// max_k log_scales[k] of a row, NaN as soon as one entry is NaN: exp is increasing, so the largest scale is the exp of this
FRO_HD float fro_row_log_scale(const float* ls, int cols)
{
	float m = ls[0];
	for (int c = 1; c < cols; c++)
	{
		const float v = ls[c];
		m = (m != m || v != v) ? fro_float(FRO_NAN_BITS) : (v > m ? v : m);
	}
	return m;
}

// An order-preserving integer key of a float that is not NaN (-0 below +0): min / max of floats as min / max of unsigned integers
FRO_HD uint32_t fro_order_key(float v) { const uint32_t u = fro_bits(v); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
FRO_HD float fro_order_value(uint32_t key) { return fro_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key); }

// exp of an extreme log scale, correctly rounded to binary32 through binary64 (the same bits from every libm whose binary64 exp is
// good to an ulp, but for a result within that ulp of a binary32 rounding boundary: one value in ~2^28)
FRO_HD float fro_scale(float log_scale) { return (float)exp((double)log_scale); }

// the four range words of the status from a set's count, NaN flag and the keys of its extreme log scales
FRO_HD void fro_range_bits(uint32_t count, uint32_t has_nan, uint32_t key_min, uint32_t key_max, uint32_t* lo, uint32_t* hi)
{
	if (count == 0u || has_nan) { *lo = FRO_NAN_BITS; *hi = FRO_NAN_BITS; return; }
	*lo = fro_bits(fro_scale(fro_order_value(key_min)));
	*hi = fro_bits(fro_scale(fro_order_value(key_max)));
}

#endif
