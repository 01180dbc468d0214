// fr_popgs_block_math.h -- the per-Gaussian arithmetic of the POp-GS block stage (fr_popgs_block.hip), host/device neutral (FR_HD):
// tests/harness/fr_popgs_block_harness.cpp compiles the same functions with g++.
//
// A block is d x d, d = 3 + use_opacity + 4 use_rot + 3 use_scale, over the columns [0,1,2 | 3 | 7..10 | 4..6] of a scorer row
// (_ROW_BLOCKS / _POPGS_BLOCK_ORDER of models/SLAM/gaussian_object.py).  A symmetric block lives as its lower triangle, packed by
// rows: entry (i, j), j <= i, at i (i + 1) / 2 + j.  D is a template parameter and every loop below has constant bounds: unrolled,
// nothing is indexed at run time and a triangle stays in registers (66 binary64 at D = 11).
//
// Built with -ffp-contract=off like every unit: a product is rounded before it is added, except where fmaf is written out (the
// binary32 prior block, which follows torch's batched matrix product: one fused multiply-add per probe).
#pragma once
#include "fr_math.h"

#define FRPB_ROW 11                   // columns of a scorer row
#define FRPB_TRI(D) ((D) * ((D) + 1) / 2)

FR_HD int frpb_dim(int use_opacity, int use_rot, int use_scale) { return 3 + (use_opacity ? 1 : 0) + (use_rot ? 4 : 0) + (use_scale ? 3 : 0); }

// the row column of block column c, c < frpb_dim(..)
FR_HD int frpb_col(int c, int use_opacity, int use_rot, int use_scale)
{
	if (c < 3) return c;
	c -= 3;
	if (use_opacity) { if (c == 0) return 3; c--; }
	if (use_rot) { if (c < 4) return 7 + c; c -= 4; }
	(void)use_scale;
	return 4 + c;
}

// t += g g^T (lower triangle)
template <int D, typename T>
FR_HD void frpb_gram_add(T* t, const T* g)
{
#pragma unroll
	for (int i = 0; i < D; i++)
	{
#pragma unroll
		for (int j = 0; j <= i; j++) t[i * (i + 1) / 2 + j] += g[i] * g[j];
	}
}

// Unpivoted L D L^T in place: on return the diagonal holds the pivots, below it the unit lower factor.  Returns 1 when a pivot is not
// positive (zero, negative or NaN), else 0.  Right-looking: column j is scaled by its pivot and the trailing triangle is updated.
template <int D>
FR_HD int frpb_ldlt(double* t)
{
	int bad = 0;
#pragma unroll
	for (int j = 0; j < D; j++)
	{
		const double piv = t[j * (j + 1) / 2 + j];
		if (!(piv > 0.0)) bad = 1;
		double l[D];
#pragma unroll
		for (int i = j + 1; i < D; i++) l[i] = t[i * (i + 1) / 2 + j] / piv;
#pragma unroll
		for (int i = j + 1; i < D; i++)
		{
#pragma unroll
			for (int k = j + 1; k <= i; k++) t[i * (i + 1) / 2 + k] -= l[i] * t[k * (k + 1) / 2 + j];
		}
#pragma unroll
		for (int i = j + 1; i < D; i++) t[i * (i + 1) / 2 + j] = l[i];
	}
	return bad;
}

// sum_j log|pi_j| of a factor, j ascending (slogdet's logabsdet)
template <int D>
FR_HD double frpb_logabs(const double* t)
{
	double s = 0.0;
#pragma unroll
	for (int j = 0; j < D; j++) s += log(fabs(t[j * (j + 1) / 2 + j]));
	return s;
}

// trace(A^-1) of a factor: A^-1 = M^T diag(1 / pi) M with M = L^-1 (unit lower), so the trace is sum_k (sum_j M_kj^2) / pi_k.  The
// factor's lower part is overwritten by M, column by column: M_ij = -(L_ij + sum_{j < k < i} L_ik M_kj).
template <int D>
FR_HD double frpb_trace_inv(double* t)
{
#pragma unroll
	for (int j = 0; j < D; j++)
	{
#pragma unroll
		for (int i = j + 1; i < D; i++)
		{
			double s = t[i * (i + 1) / 2 + j];
#pragma unroll
			for (int k = j + 1; k < i; k++) s += t[i * (i + 1) / 2 + k] * t[k * (k + 1) / 2 + j];
			t[i * (i + 1) / 2 + j] = -s;
		}
	}
	double tr = 0.0;
#pragma unroll
	for (int k = 0; k < D; k++)
	{
		double s = 1.0;
#pragma unroll
		for (int j = 0; j < k; j++) s += t[k * (k + 1) / 2 + j] * t[k * (k + 1) / 2 + j];
		tr += s / t[k * (k + 1) / 2 + k];
	}
	return tr;
}

// A0 = lower triangle of a binary32 d x d block + lam I, in binary64
template <int D>
FR_HD void frpb_prior_tri(const float* prior, double lam, double* t)
{
#pragma unroll
	for (int i = 0; i < D; i++)
	{
#pragma unroll
		for (int j = 0; j <= i; j++) t[i * (i + 1) / 2 + j] = (double)prior[i * D + j] + (i == j ? lam : 0.0);
	}
}

// The term of one (pose, prior row) pair.  rows: the Gaussian's row of the pose's first probe, k_stride elements to the next probe's;
// cols[D] the row columns of the block; prior [D, D] binary32.  criterion 0: - trace(A1^-1); 1: sum log|pi(A1)| - sum log|pi(A0)|.
// bad is raised by the factorisations that meet a non-positive pivot (A1; A0 too under criterion 1).
template <int D>
FR_HD double frpb_pair_term(const float* rows, long long k_stride, int K, const int* cols, const float* prior, double lam, int criterion, int& bad)
{
	double t[FRPB_TRI(D)];
	double log0 = 0.0;
	if (criterion != 0)
	{
		frpb_prior_tri<D>(prior, lam, t);
		bad += frpb_ldlt<D>(t);
		log0 = frpb_logabs<D>(t);
	}
#pragma unroll
	for (int e = 0; e < FRPB_TRI(D); e++) t[e] = 0.0;
	for (int k = 0; k < K; k++)
	{
		double g[D];
#pragma unroll
		for (int c = 0; c < D; c++) g[c] = (double)rows[(long long)k * k_stride + cols[c]];
		frpb_gram_add<D, double>(t, g);
	}
	const double dK = (double)K;
#pragma unroll
	for (int i = 0; i < D; i++)
	{
#pragma unroll
		for (int j = 0; j <= i; j++)
		{
			const int e = i * (i + 1) / 2 + j;
			t[e] = ((double)prior[i * D + j] + (i == j ? lam : 0.0)) + t[e] / dK;
		}
	}
	bad += frpb_ldlt<D>(t);
	if (criterion == 0) return -frpb_trace_inv<D>(t);
	return frpb_logabs<D>(t) - log0;
}

// One keyframe's binary32 block of one Gaussian, (sum_k g_a g_b) / K, added to acc (lower triangle); first: acc is not read, the block
// is stored (the reference starts from a copy of the first keyframe's blocks).  The sum over the probes is the chain the reference's
// einsum runs on gfx950 (a batched matrix product): b = fma(g_a, g_b, b) from 0 with k ascending, so the first product is rounded and
// every further one is added with ONE rounding.  Following that chain is what keeps the stage within the reference's bits (measured on
// MI355X: bit-equal to torch.einsum('kvi,kvj->vij') at K = 1 and K = 2): the keyframes are then added by the same binary32 additions on
// the same operands.
template <int D>
FR_HD void frpb_prior_add(const float* rows, long long k_stride, int K, const int* cols, bool first, float* acc)
{
	float b[FRPB_TRI(D)];
#pragma unroll
	for (int e = 0; e < FRPB_TRI(D); e++) b[e] = 0.0f;
	for (int k = 0; k < K; k++)
	{
		float g[D];
#pragma unroll
		for (int c = 0; c < D; c++) g[c] = rows[(long long)k * k_stride + cols[c]];
#pragma unroll
		for (int i = 0; i < D; i++)
		{
#pragma unroll
			for (int j = 0; j <= i; j++) b[i * (i + 1) / 2 + j] = fmaf(g[i], g[j], b[i * (i + 1) / 2 + j]);
		}
	}
	const float fK = (float)K;
#pragma unroll
	for (int e = 0; e < FRPB_TRI(D); e++) acc[e] = first ? b[e] / fK : acc[e] + b[e] / fK;
}

// the seven block sizes the three flags can give
#define FRPB_FOR_EACH_D(X) X(3) X(4) X(6) X(7) X(8) X(10) X(11)
