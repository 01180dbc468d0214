// fr_popgs.hip -- the POp-GS diagonal criteria of libfisher_rast.so (gfx950, wave64): fr_popgs_diag_criterion.
//
// The reference scores a pose with the diagonal estimator in a chain of torch ops over [11 P] vectors
// (models/SLAM/gaussian_object.py:1705-1719, tester_gaussians_navigation.py:2147-2178): square the K probe rows, average,
// add the prior and lambda, clamp, reciprocal (T-opt) or two logarithms (D-opt), sum, then prior + estimate for the next
// step of the path.  Here that is ONE streaming pass per batch of views:
//
//   k_popgs_criterion   grid (blocks per view, V) x 256 threads.  A thread takes 4 consecutive entries at a time (one 16-byte
//                       load per probe row and one for the prior; four dword loads each where the view's base is not 16-byte
//                       aligned, i.e. E % 4 != 0), forms the entry's term in fp32, adds it to an fp64 sum of its own, and
//                       writes prior + J back where the view accumulates.  Wave reduction, then ONE fp64 partial per workgroup.
//   k_popgs_reduce      one thread per view adds the view's partials in index order, applies the sign and the vis_count rule.
//
// No atomics: the same call gives the same bits.  The number of workgroups per view depends on E alone and both load forms
// visit the entries in the same order, so a view's score does not depend on the batch it is in, nor on alignment.
// HBM-bound: 4 (K + 1) bytes read and 0 or 4 written per entry against ~25 (T-opt) / ~60 (D-opt) lane instructions.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "fr_internal.h"
#include "fr_block.h"
#include "fr_math.h"

#define POPGS_THREADS 256
static_assert(POPGS_THREADS == FRB_THREADS, "fr_block.h is written for 256 threads");
#define POPGS_MAX_BLOCKS_PER_VIEW 96     // 21 paths x 96 = 2016 workgroups: one resident set of 256 CUs x 8

// workgroups per view: a function of E alone (see above)
static int popgs_blocks(int64_t E)
{
	const int64_t units = (E + 3) / 4;
	const int64_t nb = (units + POPGS_THREADS - 1) / POPGS_THREADS;
	return (int)(nb < POPGS_MAX_BLOCKS_PER_VIEW ? nb : POPGS_MAX_BLOCKS_PER_VIEW);
}

struct PopgsArgs {
	const float* rows;           // [V][K][E]
	const float* prior_in;       // [E] or [V][E]
	float* prior_out;            // [V][E] or null; may alias prior_in
	const uint8_t* accumulate;   // [V] or null
	double* partials;            // [V][gridDim.x]
	long long E, prior_stride;
	int K;
	float lam, clamp;
};

// (one entry's term: popgs_term of fr_math.h, which the CPU harness compiles too)
template <bool VEC>
__device__ __forceinline__ float4 popgs_load4(const float* base, long long e, long long E)
{
	if (VEC) return *reinterpret_cast<const float4*>(base + e);
	float4 r;
	r.x = base[e];
	r.y = e + 1 < E ? base[e + 1] : 0.0f;
	r.z = e + 2 < E ? base[e + 2] : 0.0f;
	r.w = e + 3 < E ? base[e + 3] : 0.0f;
	return r;
}

template <bool DOPT, bool VEC>
__global__ __launch_bounds__(POPGS_THREADS) void k_popgs_criterion(PopgsArgs a)
{
	const int v = blockIdx.y, tid = threadIdx.x;
	const int K = a.K;
	const long long E = a.E;
	const float* rows = a.rows + (size_t)v * (size_t)K * (size_t)E;
	const float* pin = a.prior_in + (size_t)v * (size_t)a.prior_stride;
	float* pout = (a.prior_out && a.accumulate && a.accumulate[v]) ? a.prior_out + (size_t)v * (size_t)E : nullptr;
	const bool pow2 = (K & (K - 1)) == 0;
	const float kdiv = pow2 ? 1.0f / (float)K : (float)K;
	const long long units = (E + 3) / 4;
	double sum = 0.0;
	for (long long u = (long long)blockIdx.x * POPGS_THREADS + tid; u < units; u += (long long)gridDim.x * POPGS_THREADS)
	{
		const long long e = 4 * u;
		const float4 p = popgs_load4<VEC>(pin, e, E);
		float4 ss = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		// (a copy of this loop unrolled for K = 4 with its loads in front was measured and bought nothing: HBM binds the pass)
		for (int k = 0; k < K; k++)
		{
			const float4 x = popgs_load4<VEC>(rows + (size_t)k * (size_t)E, e, E);
			ss.x = fmaf(x.x, x.x, ss.x); ss.y = fmaf(x.y, x.y, ss.y);
			ss.z = fmaf(x.z, x.z, ss.z); ss.w = fmaf(x.w, x.w, ss.w);
		}
		float4 J;
		const float t0 = popgs_term<DOPT>(ss.x, kdiv, pow2, p.x, a.lam, a.clamp, J.x);
		const float t1 = popgs_term<DOPT>(ss.y, kdiv, pow2, p.y, a.lam, a.clamp, J.y);
		const float t2 = popgs_term<DOPT>(ss.z, kdiv, pow2, p.z, a.lam, a.clamp, J.z);
		const float t3 = popgs_term<DOPT>(ss.w, kdiv, pow2, p.w, a.lam, a.clamp, J.w);
		const bool full = VEC || e + 3 < E;               // the last unit of a view may hold 1 .. 3 entries
		sum += (double)t0;
		if (full || e + 1 < E) sum += (double)t1;
		if (full || e + 2 < E) sum += (double)t2;
		if (full) sum += (double)t3;
		if (pout)
		{
			if (VEC) *reinterpret_cast<float4*>(pout + e) = make_float4(p.x + J.x, p.y + J.y, p.z + J.z, p.w + J.w);
			else
			{
				pout[e] = p.x + J.x;
				if (e + 1 < E) pout[e + 1] = p.y + J.y;
				if (e + 2 < E) pout[e + 2] = p.z + J.z;
				if (e + 3 < E) pout[e + 3] = p.w + J.w;
			}
		}
	}
	__shared__ double s_red[1][POPGS_THREADS / 64];
	frb_sum256<1>(&sum, s_red);
	if (tid == 0) a.partials[(size_t)v * gridDim.x + blockIdx.x] = frb_sum4(s_red[0]);
}

// scores[v] = -/+ the view's partials added in index order; exactly 0.0 for a view that sees nothing (tester 2162-2163)
__global__ __launch_bounds__(64) void k_popgs_reduce(const double* __restrict__ partials, int nb, int V, int dopt,
                                                     const int* __restrict__ vis_count, double* __restrict__ scores)
{
	const int v = blockIdx.x * 64 + threadIdx.x;
	if (v >= V) return;
	double s = 0.0;
	for (int b = 0; b < nb; b++) s += partials[(size_t)v * nb + b];
	if (vis_count && vis_count[v] == 0) s = 0.0;
	else if (!dopt) s = -s;
	scores[v] = s;
}

extern "C" size_t fr_popgs_diag_criterion_workspace_bytes(int32_t V, int64_t E)
{
	if (V <= 0 || E <= 0) return 0;
	return (size_t)V * (size_t)popgs_blocks(E) * sizeof(double);
}

extern "C" int fr_popgs_diag_criterion(int32_t V, int32_t K, int64_t E, const float* rows, const float* prior_in,
                                       int64_t prior_in_view_stride, float* prior_out, const uint8_t* accumulate,
                                       const int32_t* vis_count, float lam, int32_t criterion, double* scores,
                                       void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	if (V <= 0 || K <= 0 || E <= 0) return fr_fail(FR_EINVAL, "fr_popgs_diag_criterion: bad argument (V, K, E must be positive)");
	if (V > 65535) return fr_fail(FR_EINVAL, "fr_popgs_diag_criterion: bad argument (more than 65535 views)");
	if (!rows || !prior_in || !scores) return fr_fail(FR_EINVAL, "fr_popgs_diag_criterion: null pointer (rows, prior_in, scores)");
	if (criterion != FR_POPGS_TOPT && criterion != FR_POPGS_DOPT) return fr_fail(FR_EINVAL, "fr_popgs_diag_criterion: unknown criterion");
	if (prior_in_view_stride != 0 && prior_in_view_stride != E)
		return fr_fail(FR_EINVAL, "fr_popgs_diag_criterion: bad argument (prior_in_view_stride must be 0 or E)");
	if (!(lam >= 0.0f)) return fr_fail(FR_EINVAL, "fr_popgs_diag_criterion: bad argument (lam must be >= 0)");
	if (prior_out && accumulate)
	{
		// in place is fine view by view; anything else that overlaps would let one view read what another has written
		const size_t n_in = prior_in_view_stride ? (size_t)V * (size_t)E : (size_t)E;
		const bool same = prior_out == prior_in && (prior_in_view_stride == E || V == 1);
		if (!same && fr_overlap(prior_in, n_in * sizeof(float), prior_out, (size_t)V * (size_t)E * sizeof(float)))
			return fr_fail(FR_EINVAL, "fr_popgs_diag_criterion: bad argument (prior_out overlaps prior_in without being the same [V, E] block)");
		if (fr_overlap(rows, (size_t)V * (size_t)K * (size_t)E * sizeof(float), prior_out, (size_t)V * (size_t)E * sizeof(float)))
			return fr_fail(FR_EINVAL, "fr_popgs_diag_criterion: bad argument (prior_out overlaps rows)");
	}
	const int nb = popgs_blocks(E);
	if (!workspace || workspace_bytes < (size_t)V * (size_t)nb * sizeof(double))
		return fr_fail(FR_ENOSPACE, "fr_popgs_diag_criterion: workspace too small (fr_popgs_diag_criterion_workspace_bytes)");
	if ((uintptr_t)workspace % sizeof(double) || (uintptr_t)scores % sizeof(double))
		return fr_fail(FR_EINVAL, "fr_popgs_diag_criterion: bad argument (workspace and scores must be 8-byte aligned)");

	PopgsArgs a;
	a.rows = rows; a.prior_in = prior_in; a.prior_out = prior_out; a.accumulate = accumulate;
	a.partials = (double*)workspace;
	a.E = E; a.prior_stride = prior_in_view_stride; a.K = K;
	a.lam = lam; a.clamp = FR_POPGS_CLAMP;
	const bool vec = E % 4 == 0 && (uintptr_t)rows % 16 == 0 && (uintptr_t)prior_in % 16 == 0 && (uintptr_t)prior_out % 16 == 0;
	const bool dopt = criterion == FR_POPGS_DOPT;
	hipStream_t s = (hipStream_t)stream;
	const dim3 grid(nb, V), block(POPGS_THREADS);
	if (dopt)
	{
		if (vec) hipLaunchKernelGGL((k_popgs_criterion<true, true>), grid, block, 0, s, a);
		else hipLaunchKernelGGL((k_popgs_criterion<true, false>), grid, block, 0, s, a);
	}
	else
	{
		if (vec) hipLaunchKernelGGL((k_popgs_criterion<false, true>), grid, block, 0, s, a);
		else hipLaunchKernelGGL((k_popgs_criterion<false, false>), grid, block, 0, s, a);
	}
	int rc;
	if ((rc = fr_check_launch("k_popgs_criterion"))) return rc;
	hipLaunchKernelGGL(k_popgs_reduce, dim3((V + 63) / 64), dim3(64), 0, s, (const double*)workspace, nb, V, dopt ? 1 : 0, vis_count, scores);
	return fr_check_launch("k_popgs_reduce");
}
