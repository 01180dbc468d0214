// fr_goal.hip -- goal selection of the object round in libfisher_rast.so (gfx950, wave64): fr_occ_object_cells /
// fr_occ_grid_candidates (include/fisher_occ.h; arithmetic: fr_goal_math.h).
//
// The reference's build_object_frontiers (planning/astar.py:686-734) runs a torch.unique(dim=0, return_counts=True) over every object
// Gaussian's cell -- a sort of the whole cloud -- copies the unique cells down and paints and reads back a host mask to get them in
// np.where order; generate_candidate_adv_object(mode="sorted") (1471-1588) builds its grid of rings and angles with a dozen torch ops.
//
//   fr_occ_object_cells     k_goal_hist (one thread per Gaussian, an integer atomic into its cell: exact, whatever the order)
//                           -> k_goal_count / k_goal_scan / k_goal_scatter (the ordered compaction of the cells with more than
//                           min_count Gaussians on fr_block.h's scan: raster order is np.where order)
//   fr_occ_grid_candidates  one kernel: the eroded-free-space count, then a pose per thread -- grid entry, centre draw, pose, keep flag.
//                           The centres may be the cells fr_occ_object_cells left on the device, their count read there.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "fr_internal.h"
#include "../../include/fisher_occ.h"
#include "fr_block.h"
#include "fr_goal_math.h"

#define FRG_THREADS 256
static_assert(FRG_THREADS == FRB_THREADS, "fr_block.h is written for 256 threads");

struct GoalGeom {
	int gw, gh;
	float cell, cx, cz;
};

static GoalGeom goal_geom(const fr_occ_cfg* c)
{
	GoalGeom g;
	g.gw = c->grid_w; g.gh = c->grid_h; g.cell = c->cell_size; g.cx = c->center_x; g.cz = c->center_z;
	return g;
}

__global__ __launch_bounds__(FRG_THREADS) void k_goal_hist(GoalGeom g, const float* __restrict__ points, int n, uint32_t* __restrict__ hist,
                                                           uint32_t* __restrict__ binned)
{
	const size_t i = (size_t)blockIdx.x * FRG_THREADS + threadIdx.x;
	bool ok = false;
	if (i < (size_t)n)
	{
		const float x = points[3 * i], z = points[3 * i + 2];
		ok = frg_finite(x) && frg_finite(z);
		if (ok) atomicAdd(&hist[(size_t)frg_bin(z, g.cz, g.cell, g.gh) * g.gw + frg_bin(x, g.cx, g.cell, g.gw)], 1u);
	}
	const unsigned long long b = __ballot(ok);
	if ((threadIdx.x & 63) == 0 && b) atomicAdd(binned, (uint32_t)__popcll(b));
}

__device__ __forceinline__ bool goal_cell_selected(const uint32_t* __restrict__ hist, uint32_t i, uint32_t n, uint32_t min_count)
{
	return i < n && hist[i] > min_count;
}

__global__ __launch_bounds__(FRG_THREADS) void k_goal_count(const uint32_t* __restrict__ hist, uint32_t n, uint32_t min_count,
                                                            uint32_t* __restrict__ counts)
{
	__shared__ uint32_t s_wave[4];
	const bool sel = goal_cell_selected(hist, blockIdx.x * (uint32_t)FRG_THREADS + threadIdx.x, n, min_count);
	const uint32_t count = frb_count256(sel, s_wave);
	if (threadIdx.x == 0) counts[blockIdx.x] = count;
}

__global__ __launch_bounds__(FRG_THREADS) void k_goal_scan(const uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets, int nwg,
                                                           const uint32_t* __restrict__ binned, int32_t* __restrict__ out_counts)
{
	__shared__ uint32_t s_wave[4];
	const uint32_t total = frb_scan_counts(counts, offsets, nwg, s_wave);
	if (threadIdx.x == 0) { out_counts[0] = (int32_t)total; out_counts[1] = (int32_t)*binned; }
}

__global__ __launch_bounds__(FRG_THREADS) void k_goal_scatter(const uint32_t* __restrict__ hist, uint32_t n, uint32_t min_count, int gw,
                                                              const uint32_t* __restrict__ offsets, int32_t* __restrict__ cells, uint32_t max_cells)
{
	__shared__ uint32_t s_wave[4];
	const uint32_t i = blockIdx.x * (uint32_t)FRG_THREADS + threadIdx.x;
	const bool sel = goal_cell_selected(hist, i, n, min_count);
	const uint32_t before = frb_rank256(sel, s_wave);        // (a barrier: in front of the return)
	if (!sel) return;
	const uint32_t slot = offsets[blockIdx.x] + before;
	if (slot < max_cells) { cells[2 * (size_t)slot] = (int32_t)(i % (uint32_t)gw); cells[2 * (size_t)slot + 1] = (int32_t)(i / (uint32_t)gw); }
}

struct GridArgs {
	GoalGeom g;
	const float* centers;        // [n_centers][2] = (x, z), or null: the centres are cells
	const int32_t* cells;        // [n_centers][2] = (col, row)
	const int32_t* n_cells_dev;  // how many of `cells` are there (clamped to n_centers)
	int n_centers, K, n_theta, bins, sqrt_area, min_free;
	float min_range, radius, cam_height;
	uint32_t seed;
	const uint8_t* eroded;
};

__global__ __launch_bounds__(1024) void k_goal_grid_candidates(GridArgs a, float* __restrict__ c2w, uint8_t* __restrict__ keep)
{
	__shared__ unsigned long long s_free;
	const int tid = threadIdx.x;
	const GoalGeom g = a.g;
	if (tid == 0) s_free = 0ull;
	__syncthreads();
	if (a.eroded)
	{
		// astar.py:1389: the filter applies only when the eroded free space has more than `min_free` cells
		unsigned long long c = 0;
		const size_t n = (size_t)g.gw * g.gh;
		for (size_t i = tid; i < n; i += 1024) c += a.eroded[i] ? 1ull : 0ull;
		if (c) atomicAdd(&s_free, c);
	}
	__syncthreads();
	const bool filter = a.eroded != nullptr && s_free > (unsigned long long)a.min_free;
	int n_centers = a.n_centers;
	if (!a.centers)
	{
		const int on_device = *a.n_cells_dev;
		n_centers = on_device < n_centers ? (on_device < 0 ? 0 : on_device) : n_centers;
	}
	for (int k = tid; k < a.K; k += 1024)
	{
		float* m = c2w + 16 * (size_t)k;
		if (n_centers == 0)
		{
			// no cell to stand around: a zero matrix that is not kept
			for (int i = 0; i < 16; i++) m[i] = 0.f;
			if (keep) keep[k] = 0;
			continue;
		}
		const int ci = frg_center_index(a.seed, (uint32_t)k, n_centers);
		float cx, cz;
		if (a.centers) { cx = a.centers[2 * (size_t)ci]; cz = a.centers[2 * (size_t)ci + 1]; }
		else
		{
			cx = frg_cell_world(a.cells[2 * (size_t)ci], g.gw, g.cell, g.cx);
			cz = frg_cell_world(a.cells[2 * (size_t)ci + 1], g.gh, g.cell, g.cz);
		}
		frg_grid_pose(k, a.n_theta, a.bins, a.sqrt_area, a.min_range, a.radius, cx, cz, a.cam_height, m);
		if (keep)
		{
			uint8_t kp = 1;
			if (filter)
			{
				// astar.py:1392-1398: (x - map_center) / cell_size + grid_dim // 2, .long() (truncation), eroded[row, col]
				const float fc = (m[3] - g.cx) / g.cell + (float)(g.gw / 2), fr = (m[11] - g.cz) / g.cell + (float)(g.gh / 2);
				kp = 0;
				if (fc > -1.0f && fc < (float)g.gw && fr > -1.0f && fr < (float)g.gh)
				{
					const int col = (int)fc, row = (int)fr;
					if (col >= 0 && col < g.gw && row >= 0 && row < g.gh) kp = a.eroded[(size_t)row * g.gw + col] ? 1 : 0;
				}
			}
			keep[k] = kp;
		}
	}
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

static bool goal_finite(float v) { return v - v == 0.0f; }

static int goal_validate(const fr_occ_cfg* c, const char* msg)
{
	if (!c || c->grid_w <= 0 || c->grid_h <= 0 || !(c->cell_size > 0.f) || !goal_finite(c->cell_size) || !goal_finite(c->center_x) ||
	    !goal_finite(c->center_z) || (long long)c->grid_w * c->grid_h > (1ll << 30))
		return fr_fail(FR_EINVAL, msg);
	return FR_OK;
}

extern "C" int fr_occ_object_cells(const fr_occ_cfg* cfg, const float* points, int32_t n_points, int32_t min_count, int32_t* cells,
                                   int32_t max_cells, int32_t* counts, void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	int rc = goal_validate(cfg, "fr_occ_object_cells: bad fr_occ_cfg");
	if (rc) return rc;
	if (n_points < 0 || min_count < 0 || max_cells < 0) return fr_fail(FR_EINVAL, "fr_occ_object_cells: bad argument (n_points, min_count, max_cells must not be negative)");
	if (!counts || (n_points > 0 && !points) || (max_cells > 0 && !cells) || !workspace)
		return fr_fail(FR_EINVAL, "fr_occ_object_cells: null pointer (points, cells, counts, workspace)");
	if (!fr_aligned(points, 4) || !fr_aligned(cells, 4) || !fr_aligned(counts, 4) || !fr_aligned(workspace, 16))
		return fr_fail(FR_EINVAL, "fr_occ_object_cells: bad argument (points, cells, counts must be 4-byte, workspace 16-byte aligned)");
	const size_t n = (size_t)cfg->grid_w * cfg->grid_h;
	const int nwg = (int)((n + FRG_THREADS - 1) / FRG_THREADS);
	const size_t o_counts = fr_align256(n * 4), o_offsets = o_counts + fr_align256((size_t)nwg * 4), o_binned = o_offsets + fr_align256((size_t)nwg * 4);
	const size_t need = o_binned + 256;
	if (need > fr_occ_workspace_bytes(cfg) || workspace_bytes < fr_occ_workspace_bytes(cfg))
		return fr_fail(FR_ENOSPACE, "fr_occ_object_cells: workspace smaller than fr_occ_workspace_bytes()");
	hipStream_t s = (hipStream_t)stream;
	char* ws = (char*)workspace;
	uint32_t* hist = (uint32_t*)ws;
	uint32_t* wg_counts = (uint32_t*)(ws + o_counts);
	uint32_t* wg_offsets = (uint32_t*)(ws + o_offsets);
	uint32_t* binned = (uint32_t*)(ws + o_binned);
	if (hipMemsetAsync(hist, 0, n * 4, s) != hipSuccess || hipMemsetAsync(binned, 0, 4, s) != hipSuccess)
		return fr_fail(FR_ELAUNCH, "fr_occ_object_cells: hipMemsetAsync failed");
	const GoalGeom g = goal_geom(cfg);
	if (n_points > 0)
	{
		hipLaunchKernelGGL(k_goal_hist, dim3((unsigned)(((size_t)n_points + FRG_THREADS - 1) / FRG_THREADS)), dim3(FRG_THREADS), 0, s, g, points, n_points,
		                   hist, binned);
		if ((rc = fr_check_launch("k_goal_hist"))) return rc;
	}
	hipLaunchKernelGGL(k_goal_count, dim3(nwg), dim3(FRG_THREADS), 0, s, (const uint32_t*)hist, (uint32_t)n, (uint32_t)min_count, wg_counts);
	if ((rc = fr_check_launch("k_goal_count"))) return rc;
	hipLaunchKernelGGL(k_goal_scan, dim3(1), dim3(FRG_THREADS), 0, s, (const uint32_t*)wg_counts, wg_offsets, nwg, (const uint32_t*)binned, counts);
	if ((rc = fr_check_launch("k_goal_scan"))) return rc;
	hipLaunchKernelGGL(k_goal_scatter, dim3(nwg), dim3(FRG_THREADS), 0, s, (const uint32_t*)hist, (uint32_t)n, (uint32_t)min_count, g.gw,
	                   (const uint32_t*)wg_offsets, cells, (uint32_t)max_cells);
	return fr_check_launch("k_goal_scatter");
}

extern "C" int fr_occ_grid_candidates(const fr_occ_cfg* cfg, const float* centers, int32_t n_centers, const int32_t* cells, const int32_t* n_cells_dev,
                                      int32_t K, float min_range, float radius, int32_t n_theta, int32_t radial_bins, int32_t sqrt_area,
                                      float cam_height, uint32_t seed, const uint8_t* eroded_free, int32_t min_free, float* c2w, uint8_t* keep,
                                      fr_stream_t stream)
{
	int rc = goal_validate(cfg, "fr_occ_grid_candidates: bad fr_occ_cfg");
	if (rc) return rc;
	if (K < 0 || n_centers < 0) return fr_fail(FR_EINVAL, "fr_occ_grid_candidates: bad argument (K, n_centers must not be negative)");
	if (n_theta < 1 || radial_bins < 1 || (long long)radial_bins * frg_n_angles(n_theta) > (1ll << 30))
		return fr_fail(FR_EINVAL, "fr_occ_grid_candidates: bad argument (n_theta, radial_bins at least 1, the grid at most 2^30 entries)");
	if (!goal_finite(min_range) || !goal_finite(radius) || !goal_finite(cam_height) || min_range < 0.f || radius < 0.f)
		return fr_fail(FR_EINVAL, "fr_occ_grid_candidates: bad argument (min_range, radius must be finite and not negative, cam_height finite)");
	if (K == 0) return FR_OK;
	if (!c2w) return fr_fail(FR_EINVAL, "fr_occ_grid_candidates: null pointer (c2w)");
	if ((centers != nullptr) == (cells != nullptr)) return fr_fail(FR_EINVAL, "fr_occ_grid_candidates: bad argument (give centers or cells, one of them)");
	if (centers && n_centers == 0) return fr_fail(FR_EINVAL, "fr_occ_grid_candidates: bad argument (no centres)");
	if (cells && !n_cells_dev) return fr_fail(FR_EINVAL, "fr_occ_grid_candidates: null pointer (n_cells_dev)");
	if (!fr_aligned(centers, 4) || !fr_aligned(cells, 4) || !fr_aligned(n_cells_dev, 4) || !fr_aligned(c2w, 4))
		return fr_fail(FR_EINVAL, "fr_occ_grid_candidates: bad argument (centers, cells, n_cells_dev, c2w must be 4-byte aligned)");
	GridArgs a;
	a.g = goal_geom(cfg);
	a.centers = centers; a.cells = cells; a.n_cells_dev = n_cells_dev;
	a.n_centers = n_centers; a.K = K; a.n_theta = n_theta; a.bins = radial_bins; a.sqrt_area = sqrt_area ? 1 : 0; a.min_free = min_free;
	a.min_range = min_range; a.radius = radius; a.cam_height = cam_height;
	a.seed = seed;
	a.eroded = eroded_free;
	hipLaunchKernelGGL(k_goal_grid_candidates, dim3(1), dim3(1024), 0, (hipStream_t)stream, a, c2w, keep);
	return fr_check_launch("k_goal_grid_candidates");
}
