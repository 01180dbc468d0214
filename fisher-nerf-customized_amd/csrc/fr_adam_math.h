// fr_adam_math.h -- the arithmetic of the fused Adam step (fr_adam.hip), host/device-neutral: the kernel and the g++ harness
// (tests/harness/fr_adam_harness.cpp) compile this same function, so a CPU run states the kernel's results bit for bit, binary32
// denormals included.
//
// The statement is one element of torch.optim.Adam's non-capturable single-tensor step (torch/optim/adam.py: lerp_, mul_ /
// addcmul_, sqrt / div / add_, addcdiv_) with amsgrad, maximize and weight decay off.  Everything is binary32, one rounding per
// written operation (the build has -ffp-contract=off and an IEEE divide / sqrt), only + - x / sqrt, and every operand order is the one
// written here.  torch's own kernels contract inside lerp / addcmul / addcdiv, differently on the CPU and on the GPU: its last
// bits are not reproduced and are not meant to be.
#ifndef FR_ADAM_MATH_H_INCLUDED
#define FR_ADAM_MATH_H_INCLUDED

#include <math.h>

#if defined(__HIPCC__)
#define FRA_HD __host__ __device__ __forceinline__
#else
#define FRA_HD static inline
#endif

// An array's coefficients, each a Python double of torch/optim/adam.py rounded once to binary32 by the caller:
//   w1 = 1 - beta1, beta2, c2 = 1 - beta2, bc2_sqrt = (1 - beta2^t)^0.5, eps, neg_step_size = -lr / (1 - beta1^t)
struct fra_coeffs { float w1, beta2, c2, bc2_sqrt, eps, neg_step_size; };

// (p, g, m, v) -> (p', m', v').  lr == 0 goes through the same arithmetic, p + (-0) x: a non-finite gradient reaches a frozen
// parameter as it does in torch.
FRA_HD void fra_adam(float& p, float g, float& m, float& v, const fra_coeffs& c)
{
	const float d = g - m;
	// ATen's lerp rule: the form that is exact at the end the weight is nearer to
	const float m1 = fabsf(c.w1) < 0.5f ? m + c.w1 * d : g - d * (1.0f - c.w1);
	const float v1 = v * c.beta2 + (c.c2 * g) * g;
	const float den = sqrtf(v1) / c.bc2_sqrt + c.eps;
	p = p + c.neg_step_size * (m1 / den);
	m = m1;
	v = v1;
}

#endif
