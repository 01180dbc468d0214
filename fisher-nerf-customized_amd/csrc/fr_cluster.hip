// fr_cluster.hip -- DBSCAN and the target selection of global_planning on the device (gfx950, wave64): fr_dbscan / fr_target_select.
//
// What the reference does on the host in the middle of global_planning (models/SLAM/gaussian.py:1216-1276): boolean indexing for a
// height band, torch.quantile of the band's scores (a full sort for two values), three more boolean indexings, a copy to the host,
// sklearn.cluster.DBSCAN and a Python loop over the labels.  Here, with the arithmetic and the labelling rule of fr_cluster_math.h:
//
//   DBSCAN    k_cluster_minmax     bounding box and count of the FINITE points (integer atomics on encoded floats)
//             k_cluster_keys       cell code << 32 | original index (x fastest; a non-finite point sorts last); labels = -1, parent = self
//             fr_sort_keys64       the 64-bit key sort (fisher_rast.hip)
//             k_cluster_gather     sorted (x, y, z, code) as one 16-byte row
//             k_cluster_core       lane per sorted point: neighbours counted up to min_samples over the 9 rows of 3 cells around it,
//                                  each row one binary search and one contiguous run -- the lanes of a wave are neighbours in space
//             k_cluster_union      core-core pairs (each once): the higher root is hooked under the lower with atomicMin, so a
//                                  component's root is its lowest-index core point
//             k_cluster_flatten    every core point's root; roots counted per workgroup
//             k_cluster_scan / k_cluster_rank    a root's number = roots before it in ORIGINAL index order: sklearn's numbering
//             k_cluster_label      core points take their root's number
//             k_cluster_border     the others take the lowest number among their core neighbours
//   select    k_cluster_count<M> / k_cluster_scan / k_cluster_scatter<M>   ordered compaction, three times: the band (with the
//                                  NaN flag and the lowest-index argmax of its scores), score > threshold, label == max_label
//             k_cluster_hist<PASS> x 4, k_cluster_next, k_cluster_threshold   the order statistic floor(rank) by radix select over the
//                                  encoded band scores, the one after it (the same value, or the smallest value above it), frk_lerp
//             k_cluster_cmax / k_cluster_winner   per-cluster maximum (integer atomicMax on encoded scores), the reference's loop
//
// Counts that a later kernel needs stay on the device (the status block): grids are sized for the capacity and threads beyond the
// count return.  Workgroups never wait for each other: what one launch hands to the next goes through the kernel boundary.  Nothing
// is allocated, nothing is read back, no environment variable is read, no float atomics; every launch and memset is on the caller's stream.
// The scan, the ballot count / rank, the radix select and the min / max / count of the finite points are fr_block.h's; the order key
// frk_enc (-0 taken as +0) and the xor trees of the key maxima are this unit's own.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fr_internal.h"
#include "fr_block.h"
#include "fr_cluster_math.h"

#define FRK_THREADS 256
static_assert(FRK_THREADS == FRB_THREADS, "fr_block.h is written for 256 threads");
#define FRK_MAX_GRID 2048
#define FRK_HIST_ITEMS 8                                   // scores per thread of a histogram workgroup

// status words of fr_target_select (include/fisher_rast.h)
enum { ST_BAND = 0, ST_ABOVE, ST_CLUSTERS, ST_MAXLABEL, ST_SELECTED, ST_ARGMAX, ST_SIDE, ST_NAN = 9, ST_THRESHOLD, ST_FINITE };

static int frk_blocks(int64_t n) { return (int)((n + FRK_THREADS - 1) / FRK_THREADS); }

// ---- DBSCAN -------------------------------------------------------------------------------------------------------------------------

struct FrkDb
{
	int cap;                          // capacity: what the grids, the sort and the workspace are sized for
	int n_host;                       // number of points when n_dev is null
	const int32_t* n_dev;             // or a count on the device (fr_target_select: n_above), clamped to [0, cap]
	const float* pts;                 // [n,3]
	float eps, eps2;
	int min_samples;
	int32_t* labels;                  // [n]
	int32_t *st_clusters, *st_finite, *st_side;      // where the status words go
	uint32_t* acc;                    // min[3], max[3] (encoded), finite count
	uint64_t* keys;                   // [cap]
	float4* sorted;                   // [cap]: x, y, z, code bits of the finite points in key order
	int32_t* parent;                  // [cap] by original index
	int32_t* comp;                    // [cap] root of a core point, -1 otherwise
	int32_t* rank;                    // [cap] number of a root
	uint8_t* core;                    // [cap] by sorted position
	uint8_t* coreo;                   // [cap] by original index
	uint32_t* counts;                 // [workgroups of cap]
	uint32_t* offsets;
};

struct FrkDbLayout { size_t acc, keys, sorted, parent, comp, rank, core, coreo, counts, offsets, total; };
static FrkDbLayout frk_db_layout(int64_t cap)
{
	FrkDbLayout L;
	size_t o = 0;
	const size_t nwg = (size_t)frk_blocks(cap);
	L.acc = o; o = fr_align256(o + 64);
	L.keys = o; o = fr_align256(o + (size_t)cap * 8);
	L.sorted = o; o = fr_align256(o + (size_t)cap * 16);
	L.parent = o; o = fr_align256(o + (size_t)cap * 4);
	L.comp = o; o = fr_align256(o + (size_t)cap * 4);
	L.rank = o; o = fr_align256(o + (size_t)cap * 4);
	L.core = o; o = fr_align256(o + (size_t)cap);
	L.coreo = o; o = fr_align256(o + (size_t)cap);
	L.counts = o; o = fr_align256(o + nwg * 4);
	L.offsets = o; o = fr_align256(o + nwg * 4);
	L.total = o;
	return L;
}

__device__ __forceinline__ int frk_n(const FrkDb& a)
{
	if (!a.n_dev) return a.n_host;
	const int n = *a.n_dev;
	return n < 0 ? 0 : (n > a.cap ? a.cap : n);
}

// the frame of the finite points and the cell sides, from the accumulators (frk_enc: unsigned order is float order)
__device__ __forceinline__ void frk_grid(const FrkDb& a, float* lo, float* side)
{
#pragma unroll
	for (int k = 0; k < 3; k++)
	{
		lo[k] = frk_dec(a.acc[k]);
		side[k] = frk_side(lo[k], frk_dec(a.acc[3 + k]), a.eps);
	}
}

// acc[0..2] = min, acc[3..5] = max of the finite points (encoded so that unsigned order is float order), acc[6] = their number
__global__ __launch_bounds__(FRK_THREADS) void k_cluster_minmax(FrkDb a)
{
	__shared__ float s_lo[3][4], s_hi[3][4];
	__shared__ uint32_t s_cnt[4];
	frb_minmax3_finite(a.pts, frk_n(a), [](float x, float y, float z) { return frk_finite3(x, y, z); }, s_lo, s_hi, s_cnt);
	// one set of integer atomics per workgroup: their result does not depend on the order of arrival
	if (threadIdx.x < 3)
	{
		const int k = threadIdx.x;
		atomicMin(&a.acc[k], frk_enc(frb_min4(s_lo[k])));
		atomicMax(&a.acc[3 + k], frk_enc(frb_max4(s_hi[k])));
	}
	if (threadIdx.x == 3) atomicAdd(&a.acc[6], s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
}

// one thread per slot of the capacity: slots beyond the count get the last key of all, so the sort leaves them behind
__global__ __launch_bounds__(FRK_THREADS) void k_cluster_keys(FrkDb a)
{
	const int i = blockIdx.x * FRK_THREADS + threadIdx.x;
	if (i >= a.cap) return;
	const int n = frk_n(a);
	float lo[3], side[3];
	frk_grid(a, lo, side);
	if (i == 0)
	{
		*a.st_finite = (int32_t)a.acc[6];
		for (int k = 0; k < 3; k++) a.st_side[k] = (int32_t)frk_bits(side[k]);
	}
	uint32_t code = FRK_NO_CODE;
	if (i < n)
	{
		const float x = a.pts[3 * (size_t)i], y = a.pts[3 * (size_t)i + 1], z = a.pts[3 * (size_t)i + 2];
		if (frk_finite3(x, y, z)) code = frk_point_code(x, y, z, lo, side);
		a.labels[i] = -1;
		a.parent[i] = i;
		a.coreo[i] = 0;
	}
	a.keys[i] = ((uint64_t)code << 32) | (uint32_t)i;
}

__global__ __launch_bounds__(FRK_THREADS) void k_cluster_gather(FrkDb a)
{
	const int t = blockIdx.x * FRK_THREADS + threadIdx.x;
	if (t >= (int)a.acc[6]) return;                          // the finite prefix of the sorted keys
	const uint64_t key = a.keys[t];
	const uint32_t i = (uint32_t)key;
	a.sorted[t] = make_float4(a.pts[3 * (size_t)i], a.pts[3 * (size_t)i + 1], a.pts[3 * (size_t)i + 2], __uint_as_float((uint32_t)(key >> 32)));
}

// f(t, row) for every sorted position t in the 27 cells around `code`; f returns true to stop.  Per (y, z) row of cells the three
// x-neighbours are one run of the sorted points: a binary search for its first point, then a walk to the first code beyond it.
template <typename F>
__device__ __forceinline__ void frk_neighbours(const FrkDb& a, int nf, uint32_t code, F&& f)
{
	const int cx = (int)(code & (FRK_CELLS - 1)), cy = (int)((code >> FRK_CELL_BITS) & (FRK_CELLS - 1)), cz = (int)(code >> (2 * FRK_CELL_BITS));
	const uint32_t x0 = (uint32_t)(cx > 0 ? cx - 1 : 0), x1 = (uint32_t)(cx < FRK_CELLS - 1 ? cx + 1 : FRK_CELLS - 1);
	for (int z = cz - 1; z <= cz + 1; z++)
	{
		if (z < 0 || z >= FRK_CELLS) continue;
		for (int y = cy - 1; y <= cy + 1; y++)
		{
			if (y < 0 || y >= FRK_CELLS) continue;
			const uint32_t c0 = frk_code(x0, (uint32_t)y, (uint32_t)z), c1 = frk_code(x1, (uint32_t)y, (uint32_t)z);
			int b0 = 0, b1 = nf;
			while (b0 < b1)
			{
				const int mid = (b0 + b1) >> 1;
				if (__float_as_uint(a.sorted[mid].w) < c0) b0 = mid + 1; else b1 = mid;
			}
			for (int t = b0; t < nf; t++)
			{
				const float4 r = a.sorted[t];
				if (__float_as_uint(r.w) > c1) break;
				if (f(t, r)) return;
			}
		}
	}
}

__global__ __launch_bounds__(FRK_THREADS) void k_cluster_core(FrkDb a)
{
	const int s = blockIdx.x * FRK_THREADS + threadIdx.x;
	const int nf = (int)a.acc[6];
	if (s >= nf) return;
	const float4 p = a.sorted[s];
	int cnt = 0;
	const int want = a.min_samples;
	const float eps2 = a.eps2;
	frk_neighbours(a, nf, __float_as_uint(p.w), [&](int, const float4& r) {
		if (frk_inside(frk_dist2(p.x, p.y, p.z, r.x, r.y, r.z), eps2)) cnt++;        // (itself included)
		return cnt >= want;
	});
	const uint8_t c = cnt >= want ? 1 : 0;
	a.core[s] = c;
	a.coreo[(uint32_t)a.keys[s]] = c;
}

// the root of x: parents only ever decrease, and a value read late is still an ancestor.  The loads go past this CU's L1, which
// another CU's atomics do not refresh within a launch.
__device__ __forceinline__ int frk_find(int32_t* parent, int x)
{
	int p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	while (p != x) { x = p; p = __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
	return x;
}
__device__ __forceinline__ void frk_union(int32_t* parent, int a, int b)
{
	for (;;)
	{
		a = frk_find(parent, a); b = frk_find(parent, b);
		if (a == b) return;
		if (a < b) { const int t = a; a = b; b = t; }      // a is the larger root: hang it under b
		const int old = atomicMin(&parent[a], b);
		if (old == a) return;
		a = old;                                            // somebody re-rooted a meanwhile: merge that tree with b
	}
}

__global__ __launch_bounds__(FRK_THREADS) void k_cluster_union(FrkDb a)
{
	const int s = blockIdx.x * FRK_THREADS + threadIdx.x;
	const int nf = (int)a.acc[6];
	if (s >= nf || !a.core[s]) return;
	const float4 p = a.sorted[s];
	const int i = (int)(uint32_t)a.keys[s];
	const float eps2 = a.eps2;
	frk_neighbours(a, nf, __float_as_uint(p.w), [&](int t, const float4& r) {
		if (t > s && a.core[t] && frk_inside(frk_dist2(p.x, p.y, p.z, r.x, r.y, r.z), eps2))    // each pair once
			frk_union(a.parent, i, (int)(uint32_t)a.keys[t]);
		return false;
	});
}

__global__ __launch_bounds__(FRK_THREADS) void k_cluster_flatten(FrkDb a)
{
	__shared__ uint32_t s_wave[4];
	const int i = blockIdx.x * FRK_THREADS + threadIdx.x;
	const int n = frk_n(a);
	bool root = false;
	if (i < n)
	{
		int r = -1;
		if (a.coreo[i])
		{
			r = i;
			int p = a.parent[r];
			while (p != r) { r = p; p = a.parent[r]; }
		}
		a.comp[i] = r;
		root = r == i;
	}
	const uint32_t c = frb_count256(root, s_wave);
	if (threadIdx.x == 0) a.counts[blockIdx.x] = c;
}

// one workgroup: exclusive scan of the per-workgroup counts, the total into *out_total
__global__ __launch_bounds__(FRK_THREADS) void k_cluster_scan(const uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets, int nwg,
                                                              int32_t* __restrict__ out_total)
{
	__shared__ uint32_t s_wave[4];
	const uint32_t total = frb_scan_counts(counts, offsets, nwg, s_wave);
	if (threadIdx.x == 0) *out_total = (int32_t)total;
}

__global__ __launch_bounds__(FRK_THREADS) void k_cluster_rank(FrkDb a)
{
	__shared__ uint32_t s_wave[4];
	const int i = blockIdx.x * FRK_THREADS + threadIdx.x;
	const bool root = i < frk_n(a) && a.comp[i] == i;
	const uint32_t before = frb_rank256(root, s_wave);
	if (root) a.rank[i] = (int32_t)(a.offsets[blockIdx.x] + before);
}

__global__ __launch_bounds__(FRK_THREADS) void k_cluster_label(FrkDb a)
{
	const int i = blockIdx.x * FRK_THREADS + threadIdx.x;
	if (i >= frk_n(a)) return;
	const int r = a.comp[i];
	if (r >= 0) a.labels[i] = a.rank[r];
}

__global__ __launch_bounds__(FRK_THREADS) void k_cluster_border(FrkDb a)
{
	const int s = blockIdx.x * FRK_THREADS + threadIdx.x;
	const int nf = (int)a.acc[6];
	if (s >= nf || a.core[s]) return;
	const float4 p = a.sorted[s];
	const float eps2 = a.eps2;
	int best = INT32_MAX;
	frk_neighbours(a, nf, __float_as_uint(p.w), [&](int t, const float4& r) {
		if (a.core[t] && frk_inside(frk_dist2(p.x, p.y, p.z, r.x, r.y, r.z), eps2))
		{
			const int l = a.labels[(uint32_t)a.keys[t]];      // a core point's label: written by the launch before this one
			best = l < best ? l : best;
		}
		return false;
	});
	if (best != INT32_MAX) a.labels[(uint32_t)a.keys[s]] = best;
}

static FrkDb frk_db_args(int cap, int n_host, const int32_t* n_dev, const float* pts, float eps, int min_samples, int32_t* labels,
                         int32_t* st_clusters, int32_t* st_finite, int32_t* st_side, char* ws)
{
	const FrkDbLayout L = frk_db_layout(cap);
	FrkDb a;
	a.cap = cap; a.n_host = n_host; a.n_dev = n_dev; a.pts = pts;
	a.eps = eps; a.eps2 = frk_eps2(eps); a.min_samples = min_samples;
	a.labels = labels; a.st_clusters = st_clusters; a.st_finite = st_finite; a.st_side = st_side;
	a.acc = (uint32_t*)(ws + L.acc); a.keys = (uint64_t*)(ws + L.keys); a.sorted = (float4*)(ws + L.sorted);
	a.parent = (int32_t*)(ws + L.parent); a.comp = (int32_t*)(ws + L.comp); a.rank = (int32_t*)(ws + L.rank);
	a.core = (uint8_t*)(ws + L.core); a.coreo = (uint8_t*)(ws + L.coreo);
	a.counts = (uint32_t*)(ws + L.counts); a.offsets = (uint32_t*)(ws + L.offsets);
	return a;
}

// the launches of one DBSCAN over a.cap > 0 slots
static int frk_dbscan_launch(const FrkDb& a, hipStream_t s)
{
	int rc;
	const int nblk = frk_blocks(a.cap);
	const dim3 block(FRK_THREADS), grid(nblk);
	if (hipMemsetAsync(a.acc, 0xFF, 12, s) != hipSuccess || hipMemsetAsync(a.acc + 3, 0x00, 20, s) != hipSuccess)
		return fr_fail(FR_ELAUNCH, "fr_dbscan: hipMemsetAsync failed");
	hipLaunchKernelGGL(k_cluster_minmax, dim3(nblk < FRK_MAX_GRID ? nblk : FRK_MAX_GRID), block, 0, s, a);
	if ((rc = fr_check_launch("k_cluster_minmax"))) return rc;
	hipLaunchKernelGGL(k_cluster_keys, grid, block, 0, s, a);
	if ((rc = fr_check_launch("k_cluster_keys"))) return rc;
	if ((rc = fr_sort_keys64(a.keys, (uint32_t)a.cap, (fr_stream_t)s))) return rc;
	hipLaunchKernelGGL(k_cluster_gather, grid, block, 0, s, a);
	if ((rc = fr_check_launch("k_cluster_gather"))) return rc;
	hipLaunchKernelGGL(k_cluster_core, grid, block, 0, s, a);
	if ((rc = fr_check_launch("k_cluster_core"))) return rc;
	hipLaunchKernelGGL(k_cluster_union, grid, block, 0, s, a);
	if ((rc = fr_check_launch("k_cluster_union"))) return rc;
	hipLaunchKernelGGL(k_cluster_flatten, grid, block, 0, s, a);
	if ((rc = fr_check_launch("k_cluster_flatten"))) return rc;
	hipLaunchKernelGGL(k_cluster_scan, dim3(1), block, 0, s, (const uint32_t*)a.counts, a.offsets, nblk, a.st_clusters);
	if ((rc = fr_check_launch("k_cluster_scan"))) return rc;
	hipLaunchKernelGGL(k_cluster_rank, grid, block, 0, s, a);
	if ((rc = fr_check_launch("k_cluster_rank"))) return rc;
	hipLaunchKernelGGL(k_cluster_label, grid, block, 0, s, a);
	if ((rc = fr_check_launch("k_cluster_label"))) return rc;
	hipLaunchKernelGGL(k_cluster_border, grid, block, 0, s, a);
	return fr_check_launch("k_cluster_border");
}

// ---- target selection ---------------------------------------------------------------------------------------------------------------

struct FrkSel
{
	int P;
	const float* means;               // [P,3]
	const float* scores;              // [P]
	float lower_y, upper_y, q;
	int32_t *band_idx, *above_idx, *labels, *sel_idx;
	float* threshold;
	int32_t* status;
	uint32_t* hist;                   // [4][256]
	unsigned long long* argmax;       // encoded score << 32 | ~row
	uint32_t* next;                   // smallest encoded band score above the lower order statistic
	uint32_t* bscore;                 // [P] encoded scores of the band rows, in band order
	uint32_t* ascore;                 // [P] likewise of the rows above the threshold
	float* pts;                       // [P,3] their centres: the cloud DBSCAN runs on
	uint32_t* cmax;                   // [P] encoded maximum score per cluster
	uint32_t* counts;
	uint32_t* offsets;
};

#define FRK_HEAD_BYTES 8192           /* the four histograms, argmax and next: cleared at the start of a call */
struct FrkSelLayout { size_t head, bscore, ascore, pts, cmax, counts, offsets, db, total; };
static FrkSelLayout frk_sel_layout(int64_t P)
{
	FrkSelLayout L;
	size_t o = 0;
	const size_t nwg = (size_t)frk_blocks(P);
	L.head = o; o = fr_align256(o + FRK_HEAD_BYTES);
	L.bscore = o; o = fr_align256(o + (size_t)P * 4);
	L.ascore = o; o = fr_align256(o + (size_t)P * 4);
	L.pts = o; o = fr_align256(o + (size_t)P * 12);
	L.cmax = o; o = fr_align256(o + (size_t)P * 4);
	L.counts = o; o = fr_align256(o + nwg * 4);
	L.offsets = o; o = fr_align256(o + nwg * 4);
	L.db = o; o = o + frk_db_layout(P).total;
	L.total = o;
	return L;
}

// the three compactions.  0: rows of the map inside the band;  1: band entries above the threshold;  2: entries above the
// threshold whose label is max_label
template <int MODE>
__device__ __forceinline__ bool frk_selected(const FrkSel& a, int j)
{
	if (MODE == 0) return j < a.P && frk_in_band(a.means[3 * (size_t)j + 1], a.lower_y, a.upper_y);
	if (MODE == 1) return j < a.status[ST_BAND] && frk_above(frk_dec(a.bscore[j]), *a.threshold);
	return j < a.status[ST_ABOVE] && a.labels[j] == a.status[ST_MAXLABEL];
}

template <int MODE>
__global__ __launch_bounds__(FRK_THREADS) void k_cluster_count(FrkSel a)
{
	__shared__ uint32_t s_wave[4];
	const int j = blockIdx.x * FRK_THREADS + threadIdx.x;
	const bool sel = frk_selected<MODE>(a, j);
	if (MODE == 0)
	{
		// the NaN flag and the lowest row that attains the band's highest score: integer atomics, one per wave
		unsigned long long key = 0ull;
		bool nan = false;
		if (sel)
		{
			const float sc = a.scores[j];
			nan = sc != sc;
			key = ((unsigned long long)frk_enc(sc) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)j);
		}
#pragma unroll
		for (int o = 32; o > 0; o >>= 1)
		{
			const unsigned long long other = __shfl_xor(key, o, 64);
			key = other > key ? other : key;
		}
		if ((threadIdx.x & 63) == 0 && key) atomicMax(a.argmax, key);
		if (__ballot(nan) && (threadIdx.x & 63) == 0) atomicOr((unsigned int*)&a.status[ST_NAN], 1u);
	}
	const uint32_t c = frb_count256(sel, s_wave);
	if (threadIdx.x == 0) a.counts[blockIdx.x] = c;
}

template <int MODE>
__global__ __launch_bounds__(FRK_THREADS) void k_cluster_scatter(FrkSel a)
{
	__shared__ uint32_t s_wave[4];
	const int j = blockIdx.x * FRK_THREADS + threadIdx.x;
	const bool sel = frk_selected<MODE>(a, j);
	const uint32_t slot = a.offsets[blockIdx.x] + frb_rank256(sel, s_wave);
	if (!sel || slot >= (uint32_t)a.P) return;                // (always inside: at most P rows are selected)
	if (MODE == 0)
	{
		a.band_idx[slot] = j;
		a.bscore[slot] = frk_enc(a.scores[j]);
	}
	else if (MODE == 1)
	{
		const int row = a.band_idx[j];
		a.above_idx[slot] = row;
		a.ascore[slot] = a.bscore[j];
		a.pts[3 * (size_t)slot] = a.means[3 * (size_t)row];
		a.pts[3 * (size_t)slot + 1] = a.means[3 * (size_t)row + 1];
		a.pts[3 * (size_t)slot + 2] = a.means[3 * (size_t)row + 2];
	}
	else a.sel_idx[slot] = a.above_idx[j];
}

template <int PASS>
__global__ __launch_bounds__(FRK_THREADS) void k_cluster_hist(FrkSel a)
{
	__shared__ uint32_t s_hist[256], s_wave[4], s_out[3];
	const int tid = threadIdx.x;
	const uint32_t n = (uint32_t)a.status[ST_BAND];
	const uint32_t base = blockIdx.x * (uint32_t)(FRK_THREADS * FRK_HIST_ITEMS);
	if (base >= n) return;                                     // (the whole workgroup)
	s_hist[tid] = 0u;
	uint32_t below, above, k, inside = 0u;
	float w;
	frk_quantile_rank(a.q, n, &below, &above, &w);
	k = below;
	const uint32_t prefix = frb_select_prefix(a.hist, PASS, k, inside, s_wave, s_out);
	__syncthreads();
#pragma unroll
	for (int i = 0; i < FRK_HIST_ITEMS; i++)
	{
		const uint32_t j = base + (uint32_t)(i * FRK_THREADS + tid);
		if (j >= n) continue;
		frb_select_count<PASS>(s_hist, a.bscore[j], prefix);
	}
	__syncthreads();
	frb_select_flush<PASS>(a.hist, s_hist);
}

// the smallest encoded band score above the lower order statistic (left at 0xFFFFFFFF when there is none)
__global__ __launch_bounds__(FRK_THREADS) void k_cluster_next(FrkSel a)
{
	__shared__ uint32_t s_wave[4], s_out[3];
	const uint32_t n = (uint32_t)a.status[ST_BAND];
	const uint32_t base = blockIdx.x * (uint32_t)(FRK_THREADS * FRK_HIST_ITEMS);
	if (base >= n) return;
	uint32_t below, above, k, inside = 0u;
	float w;
	frk_quantile_rank(a.q, n, &below, &above, &w);
	k = below;
	const uint32_t v = frb_select_prefix(a.hist, 4, k, inside, s_wave, s_out);
	uint32_t best = 0xFFFFFFFFu;
#pragma unroll
	for (int i = 0; i < FRK_HIST_ITEMS; i++)
	{
		const uint32_t j = base + (uint32_t)(i * FRK_THREADS + threadIdx.x);
		if (j >= n) continue;
		const uint32_t u = a.bscore[j];
		if (u > v && u < best) best = u;
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
	{
		const uint32_t other = __shfl_xor(best, o, 64);
		best = other < best ? other : best;
	}
	if ((threadIdx.x & 63) == 0 && best != 0xFFFFFFFFu) atomicMin(a.next, best);
}

// one workgroup: the two order statistics and the threshold; the argmax row
__global__ __launch_bounds__(FRK_THREADS) void k_cluster_threshold(FrkSel a)
{
	__shared__ uint32_t s_wave[4], s_out[3];
	const uint32_t n = (uint32_t)a.status[ST_BAND];
	float thr = NAN;                                           // an empty band: torch.quantile raises, the caller does too
	if (n > 0u)
	{
		uint32_t below, above, k, inside = 0u;
		float w;
		frk_quantile_rank(a.q, n, &below, &above, &w);
		k = below;
		const uint32_t v = frb_select_prefix(a.hist, 4, k, inside, s_wave, s_out);
		// `inside` values equal v, this one being number k of them: the next order statistic is v again unless this is the last
		const uint32_t v_above = (above == below || k + 1u < inside) ? v : *a.next;
		thr = frk_lerp(frk_dec(v), frk_dec(v_above), w);
	}
	if (threadIdx.x == 0)
	{
		*a.threshold = thr;
		a.status[ST_THRESHOLD] = (int32_t)frk_bits(thr);
		a.status[ST_ARGMAX] = n > 0u ? (int32_t)(0xFFFFFFFFu - (uint32_t)(*a.argmax & 0xFFFFFFFFull)) : -1;
	}
}

__global__ __launch_bounds__(FRK_THREADS) void k_cluster_cmax(FrkSel a)
{
	const int j = blockIdx.x * FRK_THREADS + threadIdx.x;
	if (j >= a.status[ST_ABOVE]) return;
	const int l = a.labels[j];
	if (l >= 0 && l < a.P) atomicMax(&a.cmax[l], a.ascore[j]);
}

// one workgroup: gaussian.py:1247-1257.  The highest cluster maximum, the lowest label among equals; it wins only above -1.
__global__ __launch_bounds__(FRK_THREADS) void k_cluster_winner(FrkSel a)
{
	__shared__ unsigned long long s_key[4];
	const int nc = a.status[ST_CLUSTERS];
	unsigned long long key = 0ull;
	for (int c = threadIdx.x; c < nc; c += FRK_THREADS)
	{
		const unsigned long long k = ((unsigned long long)a.cmax[c] << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)c);
		key = k > key ? k : key;
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
	{
		const unsigned long long other = __shfl_xor(key, o, 64);
		key = other > key ? other : key;
	}
	if ((threadIdx.x & 63) == 0) s_key[threadIdx.x >> 6] = key;
	__syncthreads();
	if (threadIdx.x == 0)
	{
		for (int w = 1; w < 4; w++) key = s_key[w] > key ? s_key[w] : key;
		int label = -1;
		if (nc > 0 && frk_beats(frk_dec((uint32_t)(key >> 32)), FRK_START_SCORE)) label = (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull));
		a.status[ST_MAXLABEL] = label;
	}
}

// ---- C ABI ------------------------------------------------------------------------------------------------------------------------

extern "C" size_t fr_dbscan_workspace_bytes(int32_t N)
{
	if (N < 0 || N > FR_CLUSTER_MAX_POINTS) return 0;
	return frk_db_layout(N).total;
}

extern "C" size_t fr_target_select_workspace_bytes(int32_t P)
{
	if (P < 0 || P > FR_CLUSTER_MAX_POINTS) return 0;
	return frk_sel_layout(P).total;
}

extern "C" int fr_dbscan(int32_t N, const float* points, float eps, int32_t min_samples, int32_t* labels, int32_t* status,
                         void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	if (N < 0 || N > FR_CLUSTER_MAX_POINTS) return fr_fail(FR_EINVAL, "fr_dbscan: N outside [0, FR_CLUSTER_MAX_POINTS]");
	if (!frk_eps_ok(eps)) return fr_fail(FR_EINVAL, "fr_dbscan: eps must be positive with a normal, finite square");
	if (min_samples < 1) return fr_fail(FR_EINVAL, "fr_dbscan: min_samples must be at least 1");
	if (!status || !workspace || (N > 0 && (!points || !labels))) return fr_fail(FR_EINVAL, "fr_dbscan: null pointer");
	if (!fr_aligned(points, 4) || !fr_aligned(labels, 4) || !fr_aligned(status, 4) || !fr_aligned(workspace, 8))
		return fr_fail(FR_EINVAL, "fr_dbscan: misaligned pointer (points, labels and status 4, workspace 8 bytes)");
	if (workspace_bytes < frk_db_layout(N).total) return fr_fail(FR_EINVAL, "fr_dbscan: workspace smaller than fr_dbscan_workspace_bytes()");
	hipStream_t s = (hipStream_t)stream;
	if (hipMemsetAsync(status, 0, FR_DBSCAN_STATUS_WORDS * sizeof(int32_t), s) != hipSuccess) return fr_fail(FR_ELAUNCH, "fr_dbscan: hipMemsetAsync failed");
	if (N == 0) return FR_OK;
	const FrkDb a = frk_db_args(N, N, nullptr, points, eps, min_samples, labels, status, status + 1, status + 2, (char*)workspace);
	return frk_dbscan_launch(a, s);
}

extern "C" int fr_target_select(int32_t P, const float* means3D, const float* scores, float lower_y, float upper_y, float q, float eps,
                                int32_t min_samples, int32_t* out_band_idx, int32_t* out_above_idx, int32_t* out_labels,
                                int32_t* out_selected_idx, float* out_threshold, int32_t* status, void* workspace, size_t workspace_bytes,
                                fr_stream_t stream)
{
	if (P < 0 || P > FR_CLUSTER_MAX_POINTS) return fr_fail(FR_EINVAL, "fr_target_select: P outside [0, FR_CLUSTER_MAX_POINTS]");
	if (!frk_eps_ok(eps)) return fr_fail(FR_EINVAL, "fr_target_select: eps must be positive with a normal, finite square");
	if (min_samples < 1) return fr_fail(FR_EINVAL, "fr_target_select: min_samples must be at least 1");
	if (!(q >= 0.0f && q <= 1.0f)) return fr_fail(FR_EINVAL, "fr_target_select: q outside [0, 1]");
	if (!status || !workspace || !out_threshold) return fr_fail(FR_EINVAL, "fr_target_select: null pointer (status, workspace, out_threshold)");
	if (P > 0 && (!means3D || !scores || !out_band_idx || !out_above_idx || !out_labels || !out_selected_idx))
		return fr_fail(FR_EINVAL, "fr_target_select: null pointer");
	if (!fr_aligned(means3D, 4) || !fr_aligned(scores, 4) || !fr_aligned(out_band_idx, 4) || !fr_aligned(out_above_idx, 4) ||
	    !fr_aligned(out_labels, 4) || !fr_aligned(out_selected_idx, 4) || !fr_aligned(out_threshold, 4) || !fr_aligned(status, 4) ||
	    !fr_aligned(workspace, 8))
		return fr_fail(FR_EINVAL, "fr_target_select: misaligned pointer (workspace 8, everything else 4 bytes)");
	const FrkSelLayout L = frk_sel_layout(P);
	if (workspace_bytes < L.total) return fr_fail(FR_EINVAL, "fr_target_select: workspace smaller than fr_target_select_workspace_bytes()");
	hipStream_t s = (hipStream_t)stream;
	char* ws = (char*)workspace;
	FrkSel a;
	a.P = P; a.means = means3D; a.scores = scores; a.lower_y = lower_y; a.upper_y = upper_y; a.q = q;
	a.band_idx = out_band_idx; a.above_idx = out_above_idx; a.labels = out_labels; a.sel_idx = out_selected_idx;
	a.threshold = out_threshold; a.status = status;
	a.hist = (uint32_t*)(ws + L.head);
	a.argmax = (unsigned long long*)(ws + L.head + 4096);
	a.next = (uint32_t*)(ws + L.head + 4096 + 8);
	a.bscore = (uint32_t*)(ws + L.bscore); a.ascore = (uint32_t*)(ws + L.ascore); a.pts = (float*)(ws + L.pts);
	a.cmax = (uint32_t*)(ws + L.cmax); a.counts = (uint32_t*)(ws + L.counts); a.offsets = (uint32_t*)(ws + L.offsets);
	if (hipMemsetAsync(status, 0, FR_TARGET_STATUS_WORDS * sizeof(int32_t), s) != hipSuccess ||
	    hipMemsetAsync(ws + L.head, 0, FRK_HEAD_BYTES, s) != hipSuccess || hipMemsetAsync(a.next, 0xFF, 4, s) != hipSuccess)
		return fr_fail(FR_ELAUNCH, "fr_target_select: hipMemsetAsync failed");
	int rc;
	const int nblk = frk_blocks(P);
	const dim3 block(FRK_THREADS), grid(nblk), one(1);
	if (P > 0)
	{
		const dim3 hgrid((P + FRK_THREADS * FRK_HIST_ITEMS - 1) / (FRK_THREADS * FRK_HIST_ITEMS));
		hipLaunchKernelGGL(k_cluster_count<0>, grid, block, 0, s, a);
		hipLaunchKernelGGL(k_cluster_scan, one, block, 0, s, (const uint32_t*)a.counts, a.offsets, nblk, status + ST_BAND);
		hipLaunchKernelGGL(k_cluster_scatter<0>, grid, block, 0, s, a);
		if ((rc = fr_check_launch("k_cluster_scatter<0>"))) return rc;
		hipLaunchKernelGGL(k_cluster_hist<0>, hgrid, block, 0, s, a);
		hipLaunchKernelGGL(k_cluster_hist<1>, hgrid, block, 0, s, a);
		hipLaunchKernelGGL(k_cluster_hist<2>, hgrid, block, 0, s, a);
		hipLaunchKernelGGL(k_cluster_hist<3>, hgrid, block, 0, s, a);
		hipLaunchKernelGGL(k_cluster_next, hgrid, block, 0, s, a);
		if ((rc = fr_check_launch("k_cluster_next"))) return rc;
	}
	hipLaunchKernelGGL(k_cluster_threshold, one, block, 0, s, a);
	if ((rc = fr_check_launch("k_cluster_threshold"))) return rc;
	if (P == 0)
	{
		hipLaunchKernelGGL(k_cluster_winner, one, block, 0, s, a);
		return fr_check_launch("k_cluster_winner");
	}
	hipLaunchKernelGGL(k_cluster_count<1>, grid, block, 0, s, a);
	hipLaunchKernelGGL(k_cluster_scan, one, block, 0, s, (const uint32_t*)a.counts, a.offsets, nblk, status + ST_ABOVE);
	hipLaunchKernelGGL(k_cluster_scatter<1>, grid, block, 0, s, a);
	if ((rc = fr_check_launch("k_cluster_scatter<1>"))) return rc;
	const FrkDb d = frk_db_args(P, 0, status + ST_ABOVE, a.pts, eps, min_samples, out_labels, status + ST_CLUSTERS, status + ST_FINITE,
	                            status + ST_SIDE, ws + L.db);
	if ((rc = frk_dbscan_launch(d, s))) return rc;
	if (hipMemsetAsync(a.cmax, 0, (size_t)P * 4, s) != hipSuccess) return fr_fail(FR_ELAUNCH, "fr_target_select: hipMemsetAsync failed");
	hipLaunchKernelGGL(k_cluster_cmax, grid, block, 0, s, a);
	hipLaunchKernelGGL(k_cluster_winner, one, block, 0, s, a);
	if ((rc = fr_check_launch("k_cluster_winner"))) return rc;
	hipLaunchKernelGGL(k_cluster_count<2>, grid, block, 0, s, a);
	hipLaunchKernelGGL(k_cluster_scan, one, block, 0, s, (const uint32_t*)a.counts, a.offsets, nblk, status + ST_SELECTED);
	hipLaunchKernelGGL(k_cluster_scatter<2>, grid, block, 0, s, a);
	return fr_check_launch("k_cluster_scatter<2>");
}
