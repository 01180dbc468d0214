// g++ build of the fused Adam step's arithmetic (csrc/fr_adam_math.h) for CPU-side checks: the per-element function is the header's,
// the same one k_adam_step of csrc/fr_adam.hip compiles; the loop over an array is written here.  Also the layout of fr_adam_array as
// a C++ compiler sees it, for the ctypes mirror in fisher_rast/_lib.py.
#include <cstddef>
#include <cstdint>
#include "../../include/fisher_rast.h"
#include "../../fisher-nerf-customized_amd/csrc/fr_adam_math.h"

extern "C" {

// in place on p, m, v [n]; fresh: m and v are not read (taken as zero), only written
void fra_step(long long n, float* p, const float* g, float* m, float* v, float w1, float beta2, float c2, float bc2_sqrt, float eps,
              float neg_step_size, int fresh)
{
	const fra_coeffs c = {w1, beta2, c2, bc2_sqrt, eps, neg_step_size};
	for (long long i = 0; i < n; i++)
	{
		float pp = p[i], mm = fresh ? 0.0f : m[i], vv = fresh ? 0.0f : v[i];
		fra_adam(pp, g[i], mm, vv, c);
		p[i] = pp; m[i] = mm; v[i] = vv;
	}
}

int fra_max_arrays() { return FR_ADAM_MAX_ARRAYS; }

// out[0] = sizeof(fr_adam_array), out[1..12] = the offsets of its fields in declaration order
void fra_layout(long long* out)
{
	out[0] = (long long)sizeof(fr_adam_array);
	out[1] = offsetof(fr_adam_array, param); out[2] = offsetof(fr_adam_array, grad); out[3] = offsetof(fr_adam_array, exp_avg);
	out[4] = offsetof(fr_adam_array, exp_avg_sq); out[5] = offsetof(fr_adam_array, n); out[6] = offsetof(fr_adam_array, w1);
	out[7] = offsetof(fr_adam_array, beta2); out[8] = offsetof(fr_adam_array, c2); out[9] = offsetof(fr_adam_array, bc2_sqrt);
	out[10] = offsetof(fr_adam_array, eps); out[11] = offsetof(fr_adam_array, neg_step_size); out[12] = offsetof(fr_adam_array, fresh);
}

}
