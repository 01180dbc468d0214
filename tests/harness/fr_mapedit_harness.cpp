// g++ build of the map edit's arithmetic (csrc/fr_mapedit_math.h) for CPU-side checks: the per-child function is the header's, the
// same one k_edit_split of csrc/fr_mapedit.hip compiles; the loops over the children are written here.
#include <cstdint>
#include "../../fisher-nerf-customized_amd/csrc/fr_mapedit_math.h"

extern "C" {

// R [n,9] row-major from q [n,4]
void frm_rotations(int n, const float* q, float* R)
{
	for (int i = 0; i < n; i++) frm_build_rotation(q + 4 * i, R + 9 * i);
}

float frm_divisor(int n_into) { return frm_split_divisor(n_into); }

// in place on `children` = n_into n_split rows: means [*,3], logs [*,cols] (cols 1 or 3); rot [*,4], z [*,3]
void frm_split(int children, int n_into, int cols, const float* z, float* means, const float* rot, float* logs)
{
	const float divisor = frm_split_divisor(n_into);
	for (int i = 0; i < children; i++) frm_split_child(rot + 4 * i, logs + (size_t)cols * i, cols, z + 3 * i, divisor, means + 3 * i);
}

}
