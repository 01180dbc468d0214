// fr_plan.hip -- the path planner of libfisher_rast.so (gfx950, wave64): fr_plan_grid / fr_plan_tiers / fr_plan_field / fr_plan_paths.
//
// The reference plans with a host best-first search per goal (planning/astar.py:449-538, 1591-1777).  Its product -- a path from one
// start to each of some twenty goals under one cost model -- is a single-source shortest-path field, which is what is built here
// (cost model: fr_plan_math.h):
//
//   k_plan_hist               one thread per Gaussian: the height band, the cell, one integer atomic into the histogram.
//   k_plan_occ                one thread per cell: arg-max label == 1, or more than 50 Gaussians.
//   k_plan_dilate             one thread per cell: 3 x 3 dilation (cells outside do not count), the start cleared; the threads of the
//                             start's eight neighbours count the occupied ones into status[0].
//   k_plan_tiers              one workgroup per 32 x 32 cells: the free bytes with a 20-cell halo into LDS, the capped L1 transform as a
//                             row pass and a column pass through LDS, one tier byte per cell.
//   k_plan_weights            one thread per cell: the weight bytes of its 16 INCOMING moves, 16 bytes per cell.
//   k_plan_seed               one thread: the start's word, its tile marked dirty.
//   k_plan_round              one workgroup per 64 x 64 tile, in pull form: a clean tile returns at once; a dirty one loads its words
//                             with a 3-cell halo into LDS, sweeps  g(v) = min over the incoming moves  (Jacobi: every thread computes
//                             from LDS, barrier, writes, barrier) until a sweep changes nothing, writes back the words that fell and
//                             marks the neighbours whose halo they lie in dirty for the next round.  A tile writes its own cells only.
//                             A neighbour may load a halo word while it is rewritten: every word moves as one aligned 64-bit access,
//                             either value is an upper bound, and the values only fall -- the fixed point is the same.
//   k_plan_paths              one workgroup per goal: the goal rule and the walk over the parents by one thread, the shortcut loop with
//                             each segment's band test spread over the threads.
//
// The host launches rounds and reads one device word every FRP_CHECK_EVERY rounds; it stops when a whole round changed nothing and
// gives up with FR_ENOSPACE past fr_plan_round_cap().  Workgroups never wait for each other.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "fr_internal.h"
#include "../../include/fisher_occ.h"
#include "fr_plan_math.h"

#define FRP_THREADS 256
#define FRP_TILE FR_PLAN_TILE
#define FRP_HALO 3
#define FRP_SPAN (FRP_TILE + 2 * FRP_HALO)
#define FRP_ROUND_THREADS 1024
#define FRP_ROWS_PER_PASS (FRP_ROUND_THREADS / FRP_TILE)           // 16
#define FRP_CELLS (FRP_TILE / FRP_ROWS_PER_PASS)                   // 4 cells per thread
#define FRP_MAX_SWEEPS 8192
#define FRP_CHECK_EVERY 8
#define FRP_TT 32                                                  // tile of the distance transform
#define FRP_TH (FRP_DIST_CAP - 1)                                  // its halo: 20
#define FRP_TS (FRP_TT + 2 * FRP_TH)                               // 72

struct PlanGeom {
	int gw, gh;
	float cell, cx, cz;
};

static PlanGeom plan_geom(const fr_occ_cfg* c)
{
	PlanGeom g;
	g.gw = c->grid_w; g.gh = c->grid_h; g.cell = c->cell_size; g.cx = c->center_x; g.cz = c->center_z;
	return g;
}

__global__ __launch_bounds__(FRP_THREADS) void k_plan_hist(PlanGeom g, const float* __restrict__ pts, int n, float cam_height,
                                                          uint32_t* __restrict__ hist, int32_t* __restrict__ status)
{
	const int i = blockIdx.x * FRP_THREADS + threadIdx.x;
	bool binned = false;
	if (i < n)
	{
		const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
		if (frp_in_band(y, cam_height))
		{
			const int col = frp_bin(x, g.cx, g.cell, g.gw), row = frp_bin(z, g.cz, g.cell, g.gh);
			if (col >= 0 && row >= 0)
			{
				atomicAdd(&hist[(size_t)row * g.gw + col], 1u);
				binned = true;
			}
		}
	}
	const unsigned long long bal = __ballot(binned);
	if ((threadIdx.x & 63) == 0 && bal) atomicAdd(&status[1], (int32_t)__popcll(bal));
}

// arg-max over the three layers (first maximum wins) == 1, or more than 50 Gaussians
__global__ __launch_bounds__(FRP_THREADS) void k_plan_occ(PlanGeom g, const float* __restrict__ occ_map, const uint32_t* __restrict__ hist,
                                                         uint8_t* __restrict__ out)
{
	const int i = blockIdx.x * FRP_THREADS + threadIdx.x;
	const size_t cells = (size_t)g.gw * g.gh;
	if ((size_t)i >= cells) return;
	const float a = occ_map[i], b = occ_map[cells + i], c = occ_map[2 * cells + i];
	bool occ = b > a && !(c > b);
	if (hist && hist[i] > (uint32_t)FRP_GAUSSIAN_MIN) occ = true;
	out[i] = occ ? 1 : 0;
}

__global__ __launch_bounds__(FRP_THREADS) void k_plan_dilate(PlanGeom g, const uint8_t* __restrict__ src, int sy, int sx,
                                                            uint8_t* __restrict__ occ_plan, int32_t* __restrict__ status)
{
	const int i = blockIdx.x * FRP_THREADS + threadIdx.x;
	if (i >= g.gw * g.gh) return;
	const int x = i % g.gw, y = i / g.gw;
	uint8_t r = 0;
	for (int yy = y - 1; yy <= y + 1; yy++)
	{
		if (yy < 0 || yy >= g.gh) continue;
		for (int xx = x - 1; xx <= x + 1; xx++)
			if (xx >= 0 && xx < g.gw && src[(size_t)yy * g.gw + xx]) r = 1;
	}
	const int ady = y > sy ? y - sy : sy - y, adx = x > sx ? x - sx : sx - x;
	if (ady == 0 && adx == 0) r = 0;
	else if (ady <= 1 && adx <= 1 && r) atomicAdd(&status[0], 1);
	occ_plan[i] = r;
}

// capped L1 distance to the nearest non-free cell inside the grid: a row pass and a column pass through LDS
__global__ __launch_bounds__(FRP_THREADS) void k_plan_tiers(int H, int W, const uint8_t* __restrict__ free_space, uint8_t* __restrict__ tiers)
{
	__shared__ uint8_t s_free[FRP_TS * FRP_TS];              // 1 = free or outside the grid (no obstacle)
	__shared__ uint8_t s_row[FRP_TS * FRP_TT];               // distance along the row, capped
	const int tid = threadIdx.x;
	const int x0 = blockIdx.x * FRP_TT, y0 = blockIdx.y * FRP_TT;
	for (int i = tid; i < FRP_TS * FRP_TS; i += FRP_THREADS)
	{
		const int ly = i / FRP_TS, lx = i % FRP_TS, y = y0 + ly - FRP_TH, x = x0 + lx - FRP_TH;
		uint8_t f = 1;
		if (y >= 0 && y < H && x >= 0 && x < W) f = free_space[(size_t)y * W + x] ? 1 : 0;
		s_free[i] = f;
	}
	__syncthreads();
	for (int i = tid; i < FRP_TS * FRP_TT; i += FRP_THREADS)
	{
		const int ly = i / FRP_TT, lx = i % FRP_TT + FRP_TH;
		int d = FRP_DIST_CAP;
		for (int o = 0; o <= FRP_TH; o++)
			if (!s_free[ly * FRP_TS + lx - o] || !s_free[ly * FRP_TS + lx + o]) { d = o; break; }
		s_row[i] = (uint8_t)d;
	}
	__syncthreads();
	for (int i = tid; i < FRP_TT * FRP_TT; i += FRP_THREADS)
	{
		const int ty = i / FRP_TT, tx = i % FRP_TT, y = y0 + ty, x = x0 + tx;
		if (y >= H || x >= W) continue;
		const int ly = ty + FRP_TH;
		int d = FRP_DIST_CAP;
		for (int o = -FRP_TH; o <= FRP_TH; o++)
		{
			const int v = (int)s_row[(ly + o) * FRP_TT + tx] + (o < 0 ? -o : o);
			d = v < d ? v : d;
		}
		tiers[(size_t)y * W + x] = frp_tier_byte(s_free[ly * FRP_TS + tx + FRP_TH], d);
	}
}

// byte m of cell v: the weight byte of move m LEAVING v - move(m), which arrives in v
__global__ __launch_bounds__(FRP_THREADS) void k_plan_weights(int H, int W, const uint8_t* __restrict__ tiers, uint4* __restrict__ wtab)
{
	const int i = blockIdx.x * FRP_THREADS + threadIdx.x;
	if (i >= H * W) return;
	const int x = i % W, y = i / W;
	uint32_t w[4] = {0u, 0u, 0u, 0u};
	for (int m = 0; m < FRP_MOVES; m++)
	{
		int dy, dx;
		frp_move(m, &dy, &dx);
		const int uy = y - dy, ux = x - dx;
		uint32_t b = FRP_NO_MOVE;
		if ((tiers[i] & 1) && uy >= 0 && uy < H && ux >= 0 && ux < W) b = frp_weight_byte(tiers, H, W, uy, ux, m);
		w[m >> 2] |= b << (8 * (m & 3));
	}
	wtab[i] = make_uint4(w[0], w[1], w[2], w[3]);
}

__global__ void k_plan_seed(int W, const uint8_t* __restrict__ tiers, int sy, int sx, int tiles_x, uint64_t* __restrict__ field,
                            int* __restrict__ dirty, int32_t* __restrict__ status)
{
	if (threadIdx.x != 0 || blockIdx.x != 0) return;
	const size_t s = (size_t)sy * W + sx;
	const bool in_free = tiers[s] & 1;
	if (in_free)
	{
		field[s] = (uint64_t)s;                                // cost +0.0, its own parent
		dirty[(sy / FRP_TILE) * tiles_x + sx / FRP_TILE] = 1;
	}
	status[2] = in_free ? 1 : 0;
	status[3] = 0;
}

__device__ __forceinline__ uint64_t frp_load_word(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void frp_store_word(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(FRP_ROUND_THREADS) void k_plan_round(int H, int W, int tiles_x, int tiles_y, const uint4* __restrict__ wtab,
                                                                  uint64_t* field, int* dirty_now, int* dirty_next, int round,
                                                                  int32_t* status)
{
	__shared__ uint64_t s_g[FRP_SPAN * FRP_SPAN];
	__shared__ int s_flag, s_sides;
	const int tid = threadIdx.x;
	const int tile = blockIdx.x, tile_x = tile % tiles_x, tile_y = tile / tiles_x;
	const int x0 = tile_x * FRP_TILE, y0 = tile_y * FRP_TILE;
	if (tid == 0)
	{
		s_flag = dirty_now[tile];
		s_sides = 0;
		if (s_flag) dirty_now[tile] = 0;                       // nobody else touches this round's flag of this tile
	}
	__syncthreads();
	if (!s_flag) return;

	for (int i = tid; i < FRP_SPAN * FRP_SPAN; i += FRP_ROUND_THREADS)
	{
		const int y = y0 + i / FRP_SPAN - FRP_HALO, x = x0 + i % FRP_SPAN - FRP_HALO;
		uint64_t w = FRP_UNREACHED;
		if (y >= 0 && y < H && x >= 0 && x < W) w = frp_load_word(&field[(size_t)y * W + x]);
		s_g[i] = w;
	}
	const int lx = tid % FRP_TILE, ly0 = tid / FRP_TILE, x = x0 + lx;
	uint64_t wb_lo[FRP_CELLS], wb_hi[FRP_CELLS];               // weight bytes of the moves 0-7 and 8-15 arriving in each of the thread's cells
	bool inside[FRP_CELLS];
#pragma unroll
	for (int k = 0; k < FRP_CELLS; k++)
	{
		const int y = y0 + ly0 + FRP_ROWS_PER_PASS * k;
		inside[k] = y < H && x < W;
		uint4 q = make_uint4(~0u, ~0u, ~0u, ~0u);
		if (inside[k]) q = wtab[(size_t)y * W + x];
		wb_lo[k] = ((uint64_t)q.y << 32) | q.x;
		wb_hi[k] = ((uint64_t)q.w << 32) | q.z;
	}
	__syncthreads();
	uint64_t orig[FRP_CELLS], cur[FRP_CELLS], next[FRP_CELLS];
#pragma unroll
	for (int k = 0; k < FRP_CELLS; k++)
		orig[k] = cur[k] = s_g[(ly0 + FRP_ROWS_PER_PASS * k + FRP_HALO) * FRP_SPAN + lx + FRP_HALO];

	int sweep = 0;
	for (; sweep < FRP_MAX_SWEEPS; sweep++)
	{
#pragma unroll
		for (int k = 0; k < FRP_CELLS; k++) next[k] = cur[k];
		// the move is the outer loop and is not unrolled: four LDS words in flight, not sixty-four
#pragma unroll 1
		for (int m = 0; m < FRP_MOVES; m++)
		{
			int dy, dx;
			frp_move(m, &dy, &dx);
			const int shift = 8 * (m & 7);
#pragma unroll
			for (int k = 0; k < FRP_CELLS; k++)
			{
				const uint8_t b = (uint8_t)((m < 8 ? wb_lo[k] : wb_hi[k]) >> shift);
				if (b == FRP_NO_MOVE) continue;                    // also every move of a cell outside the grid
				const int ly = ly0 + FRP_ROWS_PER_PASS * k;
				const uint64_t from = s_g[(ly - dy + FRP_HALO) * FRP_SPAN + lx - dx + FRP_HALO];
				const uint64_t cand = frp_relax(from, (uint32_t)((y0 + ly - dy) * W + (x - dx)), m, b);
				next[k] = cand < next[k] ? cand : next[k];
			}
		}
		int changed = 0;
#pragma unroll
		for (int k = 0; k < FRP_CELLS; k++) changed |= next[k] < cur[k];
		if (!__syncthreads_or(changed)) break;                 // every thread has read what it needs of this sweep's state
#pragma unroll
		for (int k = 0; k < FRP_CELLS; k++)
			if (next[k] < cur[k])
			{
				cur[k] = next[k];
				s_g[(ly0 + FRP_ROWS_PER_PASS * k + FRP_HALO) * FRP_SPAN + lx + FRP_HALO] = cur[k];
			}
		__syncthreads();
	}

	int sides = 0;
#pragma unroll
	for (int k = 0; k < FRP_CELLS; k++)
		if (inside[k] && cur[k] != orig[k])
		{
			const int ly = ly0 + FRP_ROWS_PER_PASS * k;
			frp_store_word(&field[(size_t)(y0 + ly) * W + x], cur[k]);
			sides |= 16 | (ly < FRP_HALO ? 1 : 0) | (ly >= FRP_TILE - FRP_HALO ? 2 : 0) | (lx < FRP_HALO ? 4 : 0) | (lx >= FRP_TILE - FRP_HALO ? 8 : 0);
		}
	if (sides) atomicOr(&s_sides, sides);
	__syncthreads();
	if (tid != 0) return;
	sides = s_sides;
	if (sweep == FRP_MAX_SWEEPS) { dirty_next[tile] = 1; sides |= 16; }        // not settled: once more
	if (!sides) return;
	atomicMax(&status[3], round + 1);
	for (int ny = -1; ny <= 1; ny++)
		for (int nx = -1; nx <= 1; nx++)
		{
			if (!ny && !nx) continue;
			if ((ny < 0 && !(sides & 1)) || (ny > 0 && !(sides & 2)) || (nx < 0 && !(sides & 4)) || (nx > 0 && !(sides & 8))) continue;
			const int ty = tile_y + ny, tx = tile_x + nx;
			if (ty < 0 || ty >= tiles_y || tx < 0 || tx >= tiles_x) continue;
			dirty_next[ty * tiles_x + tx] = 1;
		}
}

// 1 when an occupied cell of occ_plan lies in the band of the segment (ay, ax) - (by, bx); the candidates (a strip of 14 cells
// across the major axis, 4 more cells at either end: a superset of the band) are spread over the workgroup's threads
__device__ __forceinline__ int frp_segment_blocked(const uint8_t* __restrict__ occ, int H, int W, int ay, int ax, int by, int bx, int tid, int nthreads)
{
	const int ady = by > ay ? by - ay : ay - by, adx = bx > ax ? bx - ax : ax - bx;
	const bool along_x = adx >= ady;
	// (p, q): major and minor coordinates
	const int ap = along_x ? ax : ay, aq = along_x ? ay : ax, bp = along_x ? bx : by, bq = along_x ? by : bx;
	const int lo = ap < bp ? ap : bp, hi = ap < bp ? bp : ap;
	const int items = (hi - lo + 9) * 14;
	int blocked = 0;
	for (int i = tid; i < items && !blocked; i += nthreads)
	{
		const int p = lo - 4 + i / 14;
		const int pc = p < lo ? lo : (p > hi ? hi : p);
		int qc = aq;
		if (bp != ap)
		{
			const int num = (pc - ap) * (bq - aq), den = bp - ap;
			int fl = num / den;
			if ((num % den != 0) && ((num < 0) != (den < 0))) fl--;
			qc = aq + fl;
		}
		const int q = qc - 6 + i % 14;
		const int y = along_x ? q : p, x = along_x ? p : q;
		if (y < 0 || y >= H || x < 0 || x >= W) continue;
		if (occ[(size_t)y * W + x] && frp_in_band_of_segment(ay, ax, by, bx, y, x)) blocked = 1;
	}
	return blocked;
}

__global__ __launch_bounds__(FRP_THREADS) void k_plan_paths(int H, int W, const uint64_t* __restrict__ field, const uint8_t* __restrict__ occ_plan,
                                                           int sy, int sx, const int32_t* __restrict__ goals, int shortcut,
                                                           int32_t* paths, int max_len, int32_t* __restrict__ lengths)
{
	__shared__ int s_n;
	const int tid = threadIdx.x, g = blockIdx.x;
	int32_t* out = paths + (size_t)g * max_len * 2;
	if (tid == 0)
	{
		const int64_t cells = (int64_t)H * W, start = (int64_t)sy * W + sx;
		const int64_t end = frp_end_cell(field, occ_plan, H, W, sy, sx, goals[2 * g], goals[2 * g + 1]);
		int64_t n = 0;
		if (end >= 0)
		{
			int64_t cur = end;
			n = 1;
			while (cur != start && n <= cells)
			{
				const uint64_t w = field[cur];
				const int64_t parent = (int64_t)(w & 0xFFFFFFFFull);
				if (w == FRP_UNREACHED || parent >= cells) { n = cells + 1; break; }
				cur = parent;
				n++;
			}
			if (n > cells) n = 0;                                   // not a tree over the start: no path
		}
		const int64_t need = (shortcut && n == 2) ? 3 : n;
		if (need > max_len) n = -1;
		else if (n > 0)
		{
			int64_t cur = end;
			for (int64_t k = n - 1; k >= 0; k--)
			{
				out[2 * k] = (int32_t)(cur % W);
				out[2 * k + 1] = (int32_t)(cur / W);
				cur = (int64_t)(field[cur] & 0xFFFFFFFFull);
			}
		}
		s_n = (int)n;
	}
	__syncthreads();
	const int n = s_n;
	if (n <= 0 || !shortcut)
	{
		if (tid == 0) lengths[g] = n;
		return;
	}
	// astar.py:1755-1770 as written: the list starts as the first two points; a point that can be seen from the one before the
	// list's last replaces the last, any other is appended; the last point is appended at the end (twice on a two-point path)
	int path_idx = 1;
	for (int i = 2; i < n - 1; i++)
	{
		const int ax = out[2 * (path_idx - 1)], ay = out[2 * (path_idx - 1) + 1], bx = out[2 * i], by = out[2 * i + 1];
		const int blocked = __syncthreads_or(frp_segment_blocked(occ_plan, H, W, ay, ax, by, bx, tid, FRP_THREADS));
		if (blocked) path_idx++;
		if (tid == 0) { out[2 * path_idx] = bx; out[2 * path_idx + 1] = by; }
		__syncthreads();
	}
	if (tid == 0)
	{
		const int lx = out[2 * (n - 1)], ly = out[2 * (n - 1) + 1];
		out[2 * (path_idx + 1)] = lx; out[2 * (path_idx + 1) + 1] = ly;
		lengths[g] = path_idx + 2;
	}
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

struct PlanLayout { size_t hist, tmp, wtab, dirty, total; int tiles_x, tiles_y; };


static PlanLayout plan_layout(const fr_occ_cfg* c)
{
	PlanLayout L;
	const size_t n = (size_t)c->grid_w * c->grid_h;
	L.tiles_x = (c->grid_w + FRP_TILE - 1) / FRP_TILE;
	L.tiles_y = (c->grid_h + FRP_TILE - 1) / FRP_TILE;
	size_t o = 0;
	L.wtab = o; o = fr_align256(o + n * 16);
	L.hist = o; o = fr_align256(o + n * 4);
	L.tmp = o; o = fr_align256(o + n);
	L.dirty = o; o = fr_align256(o + 2 * (size_t)L.tiles_x * L.tiles_y * 4);
	L.total = o;
	return L;
}

static bool plan_cfg_ok(const fr_occ_cfg* c)
{
	return c && c->grid_w > 0 && c->grid_h > 0 && c->cell_size > 0.f && (long long)c->grid_w * c->grid_h <= (1ll << 30);
}

static inline dim3 plan_grid(size_t n) { return dim3((unsigned)((n + FRP_THREADS - 1) / FRP_THREADS)); }

extern "C" size_t fr_plan_workspace_bytes(const fr_occ_cfg* cfg)
{
	if (!plan_cfg_ok(cfg)) return 0;
	return plan_layout(cfg).total;
}

extern "C" int32_t fr_plan_round_cap(const fr_occ_cfg* cfg)
{
	if (!plan_cfg_ok(cfg)) return 0;
	const PlanLayout L = plan_layout(cfg);
	return 32 * L.tiles_x * L.tiles_y + 64;
}

static bool plan_cell_ok(const fr_occ_cfg* c, int32_t row, int32_t col) { return row >= 0 && row < c->grid_h && col >= 0 && col < c->grid_w; }

extern "C" int fr_plan_grid(const fr_occ_cfg* cfg, const float* occ_map, const float* points, int32_t n_points, float cam_height,
                            int32_t start_row, int32_t start_col, uint8_t* occ_plan, int32_t* status,
                            void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	if (!plan_cfg_ok(cfg)) return fr_fail(FR_EINVAL, "fr_plan_grid: bad fr_occ_cfg");
	if (!occ_map || !occ_plan || !status || n_points < 0) return fr_fail(FR_EINVAL, "fr_plan_grid: bad argument (occ_map, occ_plan, status, n_points)");
	if (!plan_cell_ok(cfg, start_row, start_col)) return fr_fail(FR_EINVAL, "fr_plan_grid: bad argument (the start cell is outside the grid)");
	if ((uintptr_t)occ_map % 4 || (uintptr_t)points % 4 || (uintptr_t)status % 4)
		return fr_fail(FR_EINVAL, "fr_plan_grid: bad argument (occ_map, points, status must be 4-byte aligned)");
	const PlanLayout L = plan_layout(cfg);
	if (!workspace || workspace_bytes < L.total) return fr_fail(FR_ENOSPACE, "fr_plan_grid: workspace smaller than fr_plan_workspace_bytes()");
	if ((uintptr_t)workspace % 16) return fr_fail(FR_EINVAL, "fr_plan_grid: bad argument (workspace must be 16-byte aligned)");
	hipStream_t s = (hipStream_t)stream;
	char* ws = (char*)workspace;
	const PlanGeom g = plan_geom(cfg);
	const size_t n = (size_t)g.gw * g.gh;
	uint32_t* hist = (uint32_t*)(ws + L.hist);
	uint8_t* tmp = (uint8_t*)(ws + L.tmp);
	if (hipMemsetAsync(status, 0, FR_PLAN_STATUS_WORDS * sizeof(int32_t), s) != hipSuccess) return fr_fail(FR_ELAUNCH, "fr_plan_grid: hipMemsetAsync failed");
	const bool with_pts = points != nullptr && n_points > 0;
	int rc;
	if (with_pts)
	{
		if (hipMemsetAsync(hist, 0, n * 4, s) != hipSuccess) return fr_fail(FR_ELAUNCH, "fr_plan_grid: hipMemsetAsync failed");
		hipLaunchKernelGGL(k_plan_hist, plan_grid((size_t)n_points), dim3(FRP_THREADS), 0, s, g, points, n_points, cam_height, hist, status);
		if ((rc = fr_check_launch("k_plan_hist"))) return rc;
	}
	hipLaunchKernelGGL(k_plan_occ, plan_grid(n), dim3(FRP_THREADS), 0, s, g, occ_map, with_pts ? (const uint32_t*)hist : (const uint32_t*)nullptr, tmp);
	if ((rc = fr_check_launch("k_plan_occ"))) return rc;
	hipLaunchKernelGGL(k_plan_dilate, plan_grid(n), dim3(FRP_THREADS), 0, s, g, (const uint8_t*)tmp, start_row, start_col, occ_plan, status);
	return fr_check_launch("k_plan_dilate");
}

extern "C" int fr_plan_tiers(const fr_occ_cfg* cfg, const uint8_t* free_space, uint8_t* tiers, fr_stream_t stream)
{
	if (!plan_cfg_ok(cfg)) return fr_fail(FR_EINVAL, "fr_plan_tiers: bad fr_occ_cfg");
	if (!free_space || !tiers) return fr_fail(FR_EINVAL, "fr_plan_tiers: null pointer (free_space, tiers)");
	const dim3 grid((cfg->grid_w + FRP_TT - 1) / FRP_TT, (cfg->grid_h + FRP_TT - 1) / FRP_TT);
	hipLaunchKernelGGL(k_plan_tiers, grid, dim3(FRP_THREADS), 0, (hipStream_t)stream, cfg->grid_h, cfg->grid_w, free_space, tiers);
	return fr_check_launch("k_plan_tiers");
}

extern "C" int fr_plan_field(const fr_occ_cfg* cfg, const uint8_t* tiers, int32_t start_row, int32_t start_col, uint64_t* field,
                             int32_t* status, int32_t* host_counts, void* workspace, size_t workspace_bytes, fr_stream_t stream)
{
	if (!plan_cfg_ok(cfg)) return fr_fail(FR_EINVAL, "fr_plan_field: bad fr_occ_cfg");
	if (!tiers || !field || !status) return fr_fail(FR_EINVAL, "fr_plan_field: null pointer (tiers, field, status)");
	if (!plan_cell_ok(cfg, start_row, start_col)) return fr_fail(FR_EINVAL, "fr_plan_field: bad argument (the start cell is outside the grid)");
	if ((uintptr_t)field % 8 || (uintptr_t)status % 4) return fr_fail(FR_EINVAL, "fr_plan_field: bad argument (field must be 8-byte, status 4-byte aligned)");
	const PlanLayout L = plan_layout(cfg);
	if (!workspace || workspace_bytes < L.total) return fr_fail(FR_ENOSPACE, "fr_plan_field: workspace smaller than fr_plan_workspace_bytes()");
	if ((uintptr_t)workspace % 16) return fr_fail(FR_EINVAL, "fr_plan_field: bad argument (workspace must be 16-byte aligned)");
	hipStream_t s = (hipStream_t)stream;
	char* ws = (char*)workspace;
	const int H = cfg->grid_h, W = cfg->grid_w, tiles = L.tiles_x * L.tiles_y;
	const size_t n = (size_t)H * W;
	uint4* wtab = (uint4*)(ws + L.wtab);
	int* dirty = (int*)(ws + L.dirty);
	if (host_counts) host_counts[0] = host_counts[1] = 0;
	if (hipMemsetAsync(field, 0xFF, n * 8, s) != hipSuccess || hipMemsetAsync(dirty, 0, 2 * (size_t)tiles * 4, s) != hipSuccess)
		return fr_fail(FR_ELAUNCH, "fr_plan_field: hipMemsetAsync failed");
	int rc;
	hipLaunchKernelGGL(k_plan_weights, plan_grid(n), dim3(FRP_THREADS), 0, s, H, W, tiers, wtab);
	if ((rc = fr_check_launch("k_plan_weights"))) return rc;
	hipLaunchKernelGGL(k_plan_seed, dim3(1), dim3(64), 0, s, W, tiers, start_row, start_col, L.tiles_x, field, dirty, status);
	if ((rc = fr_check_launch("k_plan_seed"))) return rc;
	const int cap = fr_plan_round_cap(cfg);
	int rounds = 0, reads = 0;
	for (;;)
	{
		for (int k = 0; k < FRP_CHECK_EVERY; k++, rounds++)
		{
			hipLaunchKernelGGL(k_plan_round, dim3(tiles), dim3(FRP_ROUND_THREADS), 0, s, H, W, L.tiles_x, L.tiles_y, (const uint4*)wtab, field,
			                   dirty + (rounds & 1) * tiles, dirty + ((rounds + 1) & 1) * tiles, rounds, status);
			if ((rc = fr_check_launch("k_plan_round"))) return rc;
		}
		int32_t last = 0;
		if (hipMemcpyAsync(&last, status + 3, sizeof(last), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
			return fr_fail(FR_ELAUNCH, "fr_plan_field: reading the convergence word failed");
		reads++;
		if (host_counts) { host_counts[0] = rounds; host_counts[1] = reads; }
		if (last < rounds) return FR_OK;                           // the last round launched changed nothing: nothing is dirty
		if (rounds >= cap) return fr_fail(FR_ENOSPACE, "fr_plan_field: the field did not settle within fr_plan_round_cap() rounds");
	}
}

extern "C" int fr_plan_paths(const fr_occ_cfg* cfg, const uint64_t* field, const uint8_t* occ_plan, int32_t start_row, int32_t start_col,
                             const int32_t* goals, int32_t n_goals, int32_t shortcut, int32_t* paths, int32_t max_len, int32_t* lengths,
                             fr_stream_t stream)
{
	if (!plan_cfg_ok(cfg)) return fr_fail(FR_EINVAL, "fr_plan_paths: bad fr_occ_cfg");
	if (n_goals < 0 || max_len < 0) return fr_fail(FR_EINVAL, "fr_plan_paths: bad argument (n_goals, max_len must not be negative)");
	if (!plan_cell_ok(cfg, start_row, start_col)) return fr_fail(FR_EINVAL, "fr_plan_paths: bad argument (the start cell is outside the grid)");
	if (n_goals == 0) return FR_OK;
	if (!field || !occ_plan || !goals || !lengths || (max_len > 0 && !paths))
		return fr_fail(FR_EINVAL, "fr_plan_paths: null pointer (field, occ_plan, goals, lengths, paths)");
	if ((uintptr_t)field % 8 || (uintptr_t)goals % 4 || (uintptr_t)paths % 4 || (uintptr_t)lengths % 4)
		return fr_fail(FR_EINVAL, "fr_plan_paths: bad argument (field must be 8-byte, goals, paths, lengths 4-byte aligned)");
	hipLaunchKernelGGL(k_plan_paths, dim3(n_goals), dim3(FRP_THREADS), 0, (hipStream_t)stream, cfg->grid_h, cfg->grid_w, field, occ_plan,
	                   start_row, start_col, goals, shortcut ? 1 : 0, paths, max_len, lengths);
	return fr_check_launch("k_plan_paths");
}
