// fr_mapedit.hip -- the map edit of libfisher_rast.so (gfx950, wave64): fr_map_edit_plan / fr_map_edit_apply /
// fr_map_edit_split_children.
//
// The reference applies a prune or densify mask with a torch chain (models/SLAM/utils/slam_external.py:218-262, 411-463): about 20
// boolean indexings per remove_points (a nonzero with a host synchronisation and a gather each) over the parameters, both Adam moments
// of each and the per-Gaussian statistics, two rounds of about 15 cats per densify, a build_rotation and a bmm.  A row's destination
// depends on the masks alone, so here:
//
//   k_edit_count     one thread per source row: the three byte masks (keep, clone, split), counted per workgroup by ballot / popcount.
//   k_edit_scan      one workgroup: exclusive scans of the three lists of per-workgroup counts, the totals into status[0..2].
//   k_edit_scatter   same geometry as k_edit_count: row i goes to slot offset[workgroup] + waves before + lanes before of each list
//                    it belongs to, so every list ascends -- the order boolean indexing gives.
//   k_edit_apply     one launch for a table of up to 32 arrays (blockIdx.y picks the array): a thread per destination word, so the
//                    stores are coalesced and the loads contiguous within a row.  Destination rows are [kept | clones | children,
//                    copy-major], the order of cat((v[keep], v[clone], v[split].repeat(n, 1))).  Words are moved as bits.
//   k_edit_split     one thread per child: fr_mapedit_math.h on the child's copied rotation, log scales and mean, in place.
//
// Integer sums only: no dependence on the launch geometry.  Workgroups never wait for each other: what one launch hands to the next
// goes through the kernel boundary.  k_edit_scan is three calls of fr_block.h's frb_scan_counts; k_edit_count and k_edit_scatter
// keep their own ballots, three predicates behind ONE barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "fr_internal.h"
#include "fr_block.h"
#include "fr_mapedit_math.h"

#define FRM_THREADS 256
static_assert(FRM_THREADS == FRB_THREADS, "fr_block.h is written for 256 threads");
#define FRM_APPLY_MAX_GRID 4096       // workgroups per array of the apply launch; the rest is grid-strided

struct FrmPlanArgs {
	const uint8_t* mask[3];      // keep (null: every row), clone, split (null: no row)
	int P, nwg;
	uint32_t* counts;            // [3][nwg]
	uint32_t* offsets;           // [3][nwg]
	int32_t* idx[3];             // [P] each
	int32_t* status;
};

__device__ __forceinline__ bool frm_selected(const FrmPlanArgs& a, int k, int i)
{
	if (i >= a.P) return false;
	return a.mask[k] ? a.mask[k][i] != 0 : k == 0;
}

__global__ __launch_bounds__(FRM_THREADS) void k_edit_count(FrmPlanArgs a)
{
	__shared__ uint32_t s_wave[3][4];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int i = blockIdx.x * FRM_THREADS + tid;
#pragma unroll
	for (int k = 0; k < 3; k++)
	{
		const unsigned long long ballot = __ballot(frm_selected(a, k, i));
		if (lane == 0) s_wave[k][wave] = (uint32_t)__popcll(ballot);
	}
	__syncthreads();
	if (tid < 3) a.counts[tid * a.nwg + blockIdx.x] = ((s_wave[tid][0] + s_wave[tid][1]) + s_wave[tid][2]) + s_wave[tid][3];
}

__global__ __launch_bounds__(FRM_THREADS) void k_edit_scan(const uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets, int nwg,
                                                           int32_t* __restrict__ status)
{
	__shared__ uint32_t s_wave[4];
	const int tid = threadIdx.x;
	for (int k = 0; k < 3; k++)
	{
		const uint32_t total = frb_scan_counts(counts + k * nwg, offsets + k * nwg, nwg, s_wave);
		if (tid == 0) status[k] = (int32_t)total;
	}
	if (tid == 0) status[3] = 0;
}

__global__ __launch_bounds__(FRM_THREADS) void k_edit_scatter(FrmPlanArgs a)
{
	__shared__ uint32_t s_wave[3][4];
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int i = blockIdx.x * FRM_THREADS + tid;
	bool sel[3];
	unsigned long long ballot[3];
#pragma unroll
	for (int k = 0; k < 3; k++)
	{
		sel[k] = frm_selected(a, k, i);
		ballot[k] = __ballot(sel[k]);
		if (lane == 0) s_wave[k][wave] = (uint32_t)__popcll(ballot[k]);
	}
	__syncthreads();
#pragma unroll
	for (int k = 0; k < 3; k++)
	{
		if (!sel[k]) continue;
		uint32_t slot = a.offsets[k * a.nwg + blockIdx.x] + (uint32_t)__popcll(ballot[k] & ((1ull << lane) - 1ull));
		for (int w = 0; w < wave; w++) slot += s_wave[k][w];
		if (slot < (uint32_t)a.P) a.idx[k][slot] = i;          // always: at most P rows are selected
	}
}

struct FrmArray { const uint32_t* src; uint32_t* dst; int32_t cols, appended; };

struct FrmApplyArgs {
	FrmArray t[FR_EDIT_MAX_ARRAYS];
	const int32_t* idx[3];
	uint32_t P, n_keep, n_clone, n_split;
	unsigned long long rows;     // n_keep + n_clone + n_into n_split
};

// w = row * cols + c, c < cols; the divisions by the usual widths are by constants
__device__ __forceinline__ void frm_row_of(unsigned long long w, uint32_t cols, unsigned long long& row, uint32_t& c)
{
	switch (cols)
	{
	case 1: row = w; break;
	case 3: row = w / 3ull; break;
	case 4: row = w >> 2; break;
	case 16: row = w >> 4; break;
	default: row = w / (unsigned long long)cols; break;
	}
	c = (uint32_t)(w - row * cols);
}

__global__ __launch_bounds__(FRM_THREADS) void k_edit_apply(FrmApplyArgs a)
{
	const FrmArray t = a.t[blockIdx.y];
	const uint32_t cols = (uint32_t)t.cols;
	const unsigned long long words = a.rows * cols, stride = (unsigned long long)gridDim.x * FRM_THREADS;
	const unsigned long long first_clone = a.n_keep, first_child = (unsigned long long)a.n_keep + a.n_clone;
	for (unsigned long long w = (unsigned long long)blockIdx.x * FRM_THREADS + threadIdx.x; w < words; w += stride)
	{
		unsigned long long row64;
		uint32_t c;
		frm_row_of(w, cols, row64, c);
		const uint32_t row = (uint32_t)row64;                     // at most 2^31 - 1 rows (checked by the host)
		if (row >= first_clone && t.appended == FR_EDIT_ZERO) { t.dst[w] = 0u; continue; }
		int32_t s;
		if (row < first_clone) s = a.idx[0][row];
		else if (row < first_child) s = a.idx[1][row - first_clone];
		else s = a.idx[2][(row - first_child) % a.n_split];       // n_split > 0 here: there are child rows
		if ((uint32_t)s >= a.P) continue;                         // never with lists that fr_map_edit_plan wrote for these counts
		t.dst[w] = t.src[(unsigned long long)(uint32_t)s * cols + c];
	}
}

__global__ __launch_bounds__(FRM_THREADS) void k_edit_split(long long children, int cols, float divisor, const float* __restrict__ z,
                                                            float* __restrict__ means, const float* __restrict__ rot, float* __restrict__ logs)
{
	const long long i = (long long)blockIdx.x * FRM_THREADS + threadIdx.x;
	if (i >= children) return;
	float q[4], l[3], zz[3], m[3];
	for (int c = 0; c < 4; c++) q[c] = rot[4 * i + c];
	for (int c = 0; c < 3; c++) { zz[c] = z[3 * i + c]; m[c] = means[3 * i + c]; }
	for (int c = 0; c < cols; c++) l[c] = logs[(long long)cols * i + c];
	frm_split_child(q, l, cols, zz, divisor, m);
	for (int c = 0; c < 3; c++) means[3 * i + c] = m[c];
	for (int c = 0; c < cols; c++) logs[(long long)cols * i + c] = l[c];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

struct FrmLayout { size_t idx[3], counts, offsets, total; int nwg; };

static FrmLayout frm_layout(int32_t P)
{
	FrmLayout l;
	const size_t list = FR_EDIT_WS_LIST_STRIDE(P);
	l.nwg = (int)(((int64_t)P + FRM_THREADS - 1) / FRM_THREADS);
	for (int k = 0; k < 3; k++) l.idx[k] = (size_t)k * list;
	l.counts = 3 * list;
	l.offsets = l.counts + 3 * (size_t)l.nwg * sizeof(uint32_t);
	l.total = l.offsets + 3 * (size_t)l.nwg * sizeof(uint32_t);
	return l;
}

extern "C" size_t fr_map_edit_workspace_bytes(int32_t P)
{
	if (P < 0) return 0;
	return frm_layout(P).total;
}

extern "C" int fr_map_edit_plan(int32_t P, const uint8_t* keep, const uint8_t* clone, const uint8_t* split, int32_t* status,
                                void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	if (P < 0) return fr_fail(FR_EINVAL, "fr_map_edit_plan: bad argument (P)");
	if (!status) return fr_fail(FR_EINVAL, "fr_map_edit_plan: null pointer (status)");
	hipStream_t s = (hipStream_t)stream;
	if (P == 0)
	{
		if (hipMemsetAsync(status, 0, FR_EDIT_STATUS_WORDS * sizeof(int32_t), s) != hipSuccess) return fr_fail(FR_ELAUNCH, "fr_map_edit_plan: hipMemsetAsync failed");
		return FR_OK;
	}
	const FrmLayout l = frm_layout(P);
	if (!workspace || workspace_bytes < l.total) return fr_fail(FR_ENOSPACE, "fr_map_edit_plan: workspace too small (fr_map_edit_workspace_bytes)");
	if ((uintptr_t)workspace % 8) return fr_fail(FR_EINVAL, "fr_map_edit_plan: bad argument (workspace must be 8-byte aligned)");
	char* ws = (char*)workspace;
	FrmPlanArgs a;
	a.mask[0] = keep; a.mask[1] = clone; a.mask[2] = split;
	a.P = P; a.nwg = l.nwg;
	a.counts = (uint32_t*)(ws + l.counts); a.offsets = (uint32_t*)(ws + l.offsets);
	for (int k = 0; k < 3; k++) a.idx[k] = (int32_t*)(ws + l.idx[k]);
	a.status = status;
	const dim3 block(FRM_THREADS), grid(l.nwg);
	int rc;
	hipLaunchKernelGGL(k_edit_count, grid, block, 0, s, a);
	if ((rc = fr_check_launch("k_edit_count"))) return rc;
	hipLaunchKernelGGL(k_edit_scan, dim3(1), block, 0, s, (const uint32_t*)a.counts, a.offsets, l.nwg, status);
	if ((rc = fr_check_launch("k_edit_scan"))) return rc;
	hipLaunchKernelGGL(k_edit_scatter, grid, block, 0, s, a);
	return fr_check_launch("k_edit_scatter");
}

extern "C" int fr_map_edit_apply(const fr_map_edit_array* table, int32_t n_arrays, int32_t P, int32_t n_keep, int32_t n_clone, int32_t n_split,
                                 int32_t n_into, const void* workspace, fr_stream_t stream)
{
	if (n_arrays < 0 || n_arrays > FR_EDIT_MAX_ARRAYS) return fr_fail(FR_EINVAL, "fr_map_edit_apply: bad argument (n_arrays is at most FR_EDIT_MAX_ARRAYS)");
	if (n_arrays && !table) return fr_fail(FR_EINVAL, "fr_map_edit_apply: null pointer (table)");
	if (P < 0 || n_keep < 0 || n_clone < 0 || n_split < 0 || n_keep > P || n_clone > P || n_split > P)
		return fr_fail(FR_EINVAL, "fr_map_edit_apply: bad argument (P; n_keep, n_clone, n_split in 0 .. P)");
	if (n_into < 1) return fr_fail(FR_EINVAL, "fr_map_edit_apply: bad argument (n_into is at least 1)");
	const uint64_t rows = (uint64_t)n_keep + (uint64_t)n_clone + (uint64_t)n_into * (uint64_t)n_split;
	if (rows > ((uint64_t)1 << 31) - 1) return fr_fail(FR_EINVAL, "fr_map_edit_apply: bad argument (more than 2^31 - 1 destination rows)");
	for (int i = 0; i < n_arrays; i++)
	{
		const fr_map_edit_array& t = table[i];
		if (t.cols < 1 || t.cols > FR_EDIT_MAX_COLS) return fr_fail(FR_EINVAL, "fr_map_edit_apply: bad argument (cols in 1 .. FR_EDIT_MAX_COLS)");
		if (t.appended != FR_EDIT_COPY && t.appended != FR_EDIT_ZERO) return fr_fail(FR_EINVAL, "fr_map_edit_apply: bad argument (appended is FR_EDIT_COPY or FR_EDIT_ZERO)");
		if ((!t.src && P) || (!t.dst && rows)) return fr_fail(FR_EINVAL, "fr_map_edit_apply: null pointer (table src, dst)");
		if (((uintptr_t)t.src | (uintptr_t)t.dst) % 4) return fr_fail(FR_EINVAL, "fr_map_edit_apply: bad argument (src and dst must be 4-byte aligned)");
		if (t.src && t.src == t.dst) return fr_fail(FR_EINVAL, "fr_map_edit_apply: bad argument (src == dst: the edit is not in place)");
	}
	// no destination may overlap a source or another destination
	for (int i = 0; i < n_arrays; i++)
	{
		const size_t nd = (size_t)rows * table[i].cols * 4;
		for (int j = 0; j < n_arrays; j++)
		{
			if (fr_overlap(table[i].dst, nd, table[j].src, (size_t)P * table[j].cols * 4))
				return fr_fail(FR_EINVAL, "fr_map_edit_apply: bad argument (a destination overlaps a source)");
			if (j != i && fr_overlap(table[i].dst, nd, table[j].dst, (size_t)rows * table[j].cols * 4))
				return fr_fail(FR_EINVAL, "fr_map_edit_apply: bad argument (two destinations overlap)");
		}
	}
	if (rows == 0 || n_arrays == 0) return FR_OK;
	if (!workspace) return fr_fail(FR_EINVAL, "fr_map_edit_apply: null pointer (workspace)");
	const FrmLayout l = frm_layout(P);
	FrmApplyArgs a;
	int max_cols = 1;
	for (int i = 0; i < FR_EDIT_MAX_ARRAYS; i++)
	{
		const fr_map_edit_array& t = table[i < n_arrays ? i : 0];
		a.t[i].src = (const uint32_t*)t.src; a.t[i].dst = (uint32_t*)t.dst; a.t[i].cols = t.cols; a.t[i].appended = t.appended;
		if (i < n_arrays && t.cols > max_cols) max_cols = t.cols;
	}
	for (int k = 0; k < 3; k++) a.idx[k] = (const int32_t*)((const char*)workspace + l.idx[k]);
	a.P = (uint32_t)P; a.n_keep = (uint32_t)n_keep; a.n_clone = (uint32_t)n_clone; a.n_split = (uint32_t)n_split;
	a.rows = rows;
	const uint64_t wgs = (rows * (uint64_t)max_cols + FRM_THREADS - 1) / FRM_THREADS;
	const dim3 grid((unsigned)(wgs < FRM_APPLY_MAX_GRID ? wgs : FRM_APPLY_MAX_GRID), (unsigned)n_arrays);
	hipLaunchKernelGGL(k_edit_apply, grid, dim3(FRM_THREADS), 0, (hipStream_t)stream, a);
	return fr_check_launch("k_edit_apply");
}

extern "C" int fr_map_edit_split_children(int32_t n_split, int32_t n_into, int32_t scale_cols, const float* z, float* means,
                                          const float* unnorm_rotations, float* log_scales, fr_stream_t stream)
{
	if (n_split < 0 || n_into < 1) return fr_fail(FR_EINVAL, "fr_map_edit_split_children: bad argument (n_split, n_into)");
	if (scale_cols != 1 && scale_cols != 3) return fr_fail(FR_EINVAL, "fr_map_edit_split_children: bad argument (scale_cols is 1 or 3)");
	const int64_t children = (int64_t)n_split * n_into;
	if (children > ((int64_t)1 << 31) - 1) return fr_fail(FR_EINVAL, "fr_map_edit_split_children: bad argument (more than 2^31 - 1 children)");
	if (children == 0) return FR_OK;
	if (!z || !means || !unnorm_rotations || !log_scales) return fr_fail(FR_EINVAL, "fr_map_edit_split_children: null pointer (z, means, unnorm_rotations, log_scales)");
	hipLaunchKernelGGL(k_edit_split, dim3((unsigned)((children + FRM_THREADS - 1) / FRM_THREADS)), dim3(FRM_THREADS), 0, (hipStream_t)stream,
	                   (long long)children, (int)scale_cols, frm_split_divisor(n_into), z, means, unnorm_rotations, log_scales);
	return fr_check_launch("k_edit_split");
}
