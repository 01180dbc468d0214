// fr_adam.hip -- the fused Adam step of libfisher_rast.so (gfx950, wave64): fr_adam_step.
//
// The reference's get_optimizer (models/SLAM/gaussian.py:1458-1469) builds a torch.optim.Adam of seven groups of one tensor each;
// torch steps its groups one after the other, a chain of about a dozen element-wise launches per group, each streaming the whole
// array.  Adam is one read of (p, g, m, v) and one write of (p, m, v) per element, so here:
//
//   k_adam_step   one launch for a table of up to 16 arrays.  Every array is cut into chunks of FRA_CHUNK elements; the prefix of
//                 chunks per array travels beside the table in the kernel arguments.  A workgroup finds the array of its chunk by
//                 a uniform search over the prefix, does the chunk -- a 16-byte load of each of p, g, m, v per thread and a store
//                 of p, m, v when all four pointers are 16-byte aligned, scalar words otherwise and for the n % 4 tail -- and
//                 strides on by the grid.  fr_adam_math.h is the arithmetic.
//
// No LDS, no atomics, no workspace, no host read; an element is touched by one thread, so the result does not depend on the
// launch geometry.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include "fr_internal.h"
#include "fr_adam_math.h"

#define FRA_THREADS 256
#define FRA_CHUNK 1024                // elements per chunk: one float4 per thread
#define FRA_MAX_GRID 2048             // a streaming kernel: about 8 workgroups per CU, the rest is grid-strided

struct FraArray {
	float* p; const float* g; float* m; float* v;
	unsigned long long n;
	fra_coeffs c;
	int32_t fresh, vec;          // vec: all four pointers are 16-byte aligned
};

struct FraArgs {
	FraArray t[FR_ADAM_MAX_ARRAYS];
	unsigned long long first[FR_ADAM_MAX_ARRAYS + 1];     // first[a]: chunks before array a; first[n_arrays]: all chunks
	int32_t n_arrays;
};

__global__ __launch_bounds__(FRA_THREADS) void k_adam_step(FraArgs a)
{
	const unsigned long long chunks = a.first[a.n_arrays];
	for (unsigned long long chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x)
	{
		int k = 0;
		while (k + 1 < a.n_arrays && chunk >= a.first[k + 1]) k++;        // uniform: at most 16 entries (empty arrays are passed over)
		const FraArray t = a.t[k];
		const unsigned long long base = (chunk - a.first[k]) * FRA_CHUNK;
		const unsigned long long left = t.n - base;
		const uint32_t count = left < FRA_CHUNK ? (uint32_t)left : FRA_CHUNK;
		uint32_t done = 0;
		if (t.vec)
		{
			done = count & ~3u;
			const uint32_t i = threadIdx.x * 4;
			if (i < done)
			{
				float4 p = *(const float4*)(t.p + base + i);
				const float4 g = *(const float4*)(t.g + base + i);
				float4 m = make_float4(0.0f, 0.0f, 0.0f, 0.0f), v = m;
				if (!t.fresh)
				{
					m = *(const float4*)(t.m + base + i);
					v = *(const float4*)(t.v + base + i);
				}
				fra_adam(p.x, g.x, m.x, v.x, t.c);
				fra_adam(p.y, g.y, m.y, v.y, t.c);
				fra_adam(p.z, g.z, m.z, v.z, t.c);
				fra_adam(p.w, g.w, m.w, v.w, t.c);
				*(float4*)(t.p + base + i) = p;
				*(float4*)(t.m + base + i) = m;
				*(float4*)(t.v + base + i) = v;
			}
		}
		for (uint32_t i = done + threadIdx.x; i < count; i += FRA_THREADS)
		{
			float p = t.p[base + i], m = 0.0f, v = 0.0f;
			const float g = t.g[base + i];
			if (!t.fresh) { m = t.m[base + i]; v = t.v[base + i]; }
			fra_adam(p, g, m, v, t.c);
			t.p[base + i] = p;
			t.m[base + i] = m;
			t.v[base + i] = v;
		}
	}
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

extern "C" int fr_adam_step(const fr_adam_array* table, int32_t n_arrays, fr_stream_t stream)
{
	if (n_arrays < 0 || n_arrays > FR_ADAM_MAX_ARRAYS) return fr_fail(FR_EINVAL, "fr_adam_step: bad argument (n_arrays is 0 .. FR_ADAM_MAX_ARRAYS)");
	if (n_arrays && !table) return fr_fail(FR_EINVAL, "fr_adam_step: null pointer (table)");
	for (int i = 0; i < n_arrays; i++)
	{
		const fr_adam_array& t = table[i];
		if (t.n < 0) return fr_fail(FR_EINVAL, "fr_adam_step: bad argument (n is negative)");
		if (t.n > ((int64_t)1 << 60)) return fr_fail(FR_EINVAL, "fr_adam_step: bad argument (n is more than 2^60)");
		if (t.n && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)) return fr_fail(FR_EINVAL, "fr_adam_step: null pointer (param, grad, exp_avg, exp_avg_sq)");
		if (t.n && ((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq) % 4)
			return fr_fail(FR_EINVAL, "fr_adam_step: bad argument (pointers must be 4-byte aligned)");
		if (t.fresh != 0 && t.fresh != 1) return fr_fail(FR_EINVAL, "fr_adam_step: bad argument (fresh is 0 or 1)");
	}
	// a range that is written (param and both moments) overlaps no other range of the table; gradients are only read
	for (int i = 0; i < n_arrays; i++)
	{
		const void* written[3] = {table[i].param, table[i].exp_avg, table[i].exp_avg_sq};
		for (int w = 0; w < 3; w++)
			for (int j = 0; j < n_arrays; j++)
			{
				const void* other[4] = {table[j].param, table[j].exp_avg, table[j].exp_avg_sq, table[j].grad};
				for (int o = 0; o < 4; o++)
					if (!(j == i && o == w) && fr_overlap(written[w], (size_t)table[i].n * 4, other[o], (size_t)table[j].n * 4))
						return fr_fail(FR_EINVAL, "fr_adam_step: bad argument (a param, exp_avg or exp_avg_sq range overlaps another range of the table)");
			}
	}
	FraArgs a;
	memset(&a, 0, sizeof(a));                // entries past n_arrays: n == 0, never looked at
	unsigned long long chunks = 0;
	for (int i = 0; i < FR_ADAM_MAX_ARRAYS; i++)
	{
		FraArray& d = a.t[i];
		a.first[i] = chunks;
		if (i >= n_arrays) continue;
		const fr_adam_array& t = table[i];
		d.p = t.param; d.g = t.grad; d.m = t.exp_avg; d.v = t.exp_avg_sq;
		d.n = (unsigned long long)t.n;
		d.c.w1 = t.w1; d.c.beta2 = t.beta2; d.c.c2 = t.c2; d.c.bc2_sqrt = t.bc2_sqrt; d.c.eps = t.eps; d.c.neg_step_size = t.neg_step_size;
		d.fresh = t.fresh;
		d.vec = (((uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq) % 16) == 0;
		chunks += (d.n + FRA_CHUNK - 1) / FRA_CHUNK;
	}
	a.first[FR_ADAM_MAX_ARRAYS] = chunks;
	a.n_arrays = n_arrays;
	if (chunks == 0) return FR_OK;
	const dim3 grid((unsigned)(chunks < FRA_MAX_GRID ? chunks : FRA_MAX_GRID));
	hipLaunchKernelGGL(k_adam_step, grid, dim3(FRA_THREADS), 0, (hipStream_t)stream, a);
	return fr_check_launch("k_adam_step");
}
