// fr_plan_math.h -- the path planner's cost model, host/device neutral: compiled into csrc/fr_plan.hip and, with g++, into
// tests/harness/fr_plan_harness.cpp.  It restates the model of the reference's AstarPlanner.planning (planning/astar.py:1591-1777),
// quirks kept; what differs from the reference's search is said in INTEGRATION.md section 4b.
//
//   cells        (row, col) = (y, x); the raster index of a cell is y * W + x.
//   tier byte    0 where the cell is not in free_space, else 1 | tier << 1 with tier = 3, 2, 1, 0 for an L1 distance to the
//                nearest non-free cell of <= 5, <= 10, <= 20, more (astar.py:1709-1712): the cell costs 4 * tier.
//   move         one of 16 displacements with three path cells each (astar.py:1641-1682); the corridor is those three cells and
//                their two copies shifted by +-1 in x for the table's rows 0-8, by +-1 in y for rows 9-15 (astar.py:1684-1687: by
//                table index, not by geometry).  A move exists when its nine cells are inside the grid and free; it weighs
//                fl32(L + C), L = |displacement| as a binary32 constant, C the nine cells' costs.
//   weight byte  C / 4 (0 .. 27) of one move, FRP_NO_MOVE where the move does not exist.
//   field word   (bits of the binary32 cost) << 32 | raster index of the parent; all ones where the cell is not reached.  Costs are
//                not negative, so their bits order as they do: the smaller word is the cheaper cost, then the smaller parent.
#ifndef FR_PLAN_MATH_H_INCLUDED
#define FR_PLAN_MATH_H_INCLUDED
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FRP_HD __host__ __device__ __forceinline__
#else
#define FRP_HD static inline
#endif

#define FRP_MOVES 16
#define FRP_DIST_CAP 21                     // the transform only has to tell <= 5, <= 10, <= 20 and more apart
#define FRP_GAUSSIAN_MIN 50                 // a cell is occupied when it holds MORE than this many Gaussians of the height band
#define FRP_NO_MOVE 0xFFu
#define FRP_UNREACHED 0xFFFFFFFFFFFFFFFFull
#define FRP_BAND_HALF2 49                   // (2 * 3.5)^2: cv2.line's thickness 7 as a band of half-width 3.5

// displacement (dy, dx) of move m
FRP_HD void frp_move(int m, int* dy, int* dx)
{
	constexpr int8_t T[FRP_MOVES][2] = {{-3, 0}, {-3, 1}, {-3, 3}, {-1, 3}, {0, 3}, {3, 0}, {3, 1}, {3, 3}, {1, 3},
	                                    {-3, -1}, {-3, -3}, {-1, -3}, {0, -3}, {3, -1}, {3, -3}, {1, -3}};
	*dy = T[m][0]; *dx = T[m][1];
}

// corridor cell c (0 .. 8) of move m, relative to the cell the move leaves: c % 3 picks the path cell, c / 3 the copy
// (0 the path itself, 1 shifted by +1, 2 shifted by -1; along x for m < 9, along y otherwise)
FRP_HD void frp_corridor(int m, int c, int* dy, int* dx)
{
	constexpr int8_t P[FRP_MOVES][3][2] = {
		{{-1, 0}, {-2, 0}, {-3, 0}},   {{-1, 0}, {-2, 1}, {-3, 1}},    {{-1, 1}, {-2, 2}, {-3, 3}},    {{0, 1}, {-1, 2}, {-1, 3}},
		{{0, 1}, {0, 2}, {0, 3}},      {{1, 0}, {2, 0}, {3, 0}},       {{1, 0}, {2, 1}, {3, 1}},       {{1, 1}, {2, 2}, {3, 3}},
		{{0, 1}, {1, 2}, {1, 3}},      {{-1, 0}, {-2, -1}, {-3, -1}},  {{-1, -1}, {-2, -2}, {-3, -3}}, {{0, -1}, {-1, -2}, {-1, -3}},
		{{0, -1}, {0, -2}, {0, -3}},   {{1, 0}, {2, -1}, {3, -1}},     {{1, -1}, {2, -2}, {3, -3}},    {{0, -1}, {1, -2}, {1, -3}}};
	const int k = c % 3, copy = c / 3;
	const int shift = copy == 0 ? 0 : (copy == 1 ? 1 : -1);
	*dy = P[m][k][0] + (m < 9 ? 0 : shift);
	*dx = P[m][k][1] + (m < 9 ? shift : 0);
}

// |displacement| of move m as the binary32 constant: 3, sqrt(10) or sqrt(18)
FRP_HD float frp_move_length(int m)
{
	int dy, dx;
	frp_move(m, &dy, &dx);
	const int q = dy * dy + dx * dx;
	return q == 9 ? 3.0f : (q == 10 ? 3.16227766016837933f : 4.24264068711928515f);
}

FRP_HD uint8_t frp_tier_byte(int free, int dist)
{
	if (!free) return 0;
	const int tier = dist <= 5 ? 3 : (dist <= 10 ? 2 : (dist <= 20 ? 1 : 0));
	return (uint8_t)(1 | (tier << 1));
}

// weight byte of move m leaving (y, x); tiers: [H][W] tier bytes
FRP_HD uint8_t frp_weight_byte(const uint8_t* tiers, int H, int W, int y, int x, int m)
{
	int sum = 0;
	for (int c = 0; c < 9; c++)
	{
		int dy, dx;
		frp_corridor(m, c, &dy, &dx);
		const int yy = y + dy, xx = x + dx;
		if (yy < 0 || yy >= H || xx < 0 || xx >= W) return FRP_NO_MOVE;
		const uint8_t t = tiers[(size_t)yy * W + xx];
		if (!(t & 1)) return FRP_NO_MOVE;
		sum += t >> 1;
	}
	return (uint8_t)sum;
}

FRP_HD float frp_weight(int m, uint8_t weight_byte) { return frp_move_length(m) + (float)(4 * (int)weight_byte); }

FRP_HD uint32_t frp_float_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
FRP_HD float frp_bits_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

// the word a cell gets from its predecessor (word `from`, raster index `from_index`) over move m
FRP_HD uint64_t frp_relax(uint64_t from, uint32_t from_index, int m, uint8_t weight_byte)
{
	if (from == FRP_UNREACHED || weight_byte == FRP_NO_MOVE) return FRP_UNREACHED;
	const float g = frp_bits_float((uint32_t)(from >> 32)) + frp_weight(m, weight_byte);
	return ((uint64_t)frp_float_bits(g) << 32) | from_index;
}

// the planning grid's rule for a Gaussian (fr_occ_cells_of's, datasets/util/map_utils.py:106-125, without the clamp): the cell
// along one axis, or -1 where the point lies outside the grid
FRP_HD int frp_bin(float x, float c, float cell, int dim)
{
	const float b = floorf((x - c) / cell) + (float)(dim - 1) / 2.0f;
	if (!(b > -1.0f && b < (float)dim)) return -1;
	return (int)b;
}

FRP_HD int frp_in_band(float y, float cam_height) { return y >= cam_height - 1.0f && y <= cam_height; }

// 1 when the centre of cell (py, px) lies within 3.5 cells of the segment between the centres of (ay, ax) and (by, bx)
FRP_HD int frp_in_band_of_segment(int ay, int ax, int by, int bx, int py, int px)
{
	const int64_t aby = by - ay, abx = bx - ax, apy = py - ay, apx = px - ax;
	const int64_t ab2 = aby * aby + abx * abx, ap2 = apy * apy + apx * apx, dot = apy * aby + apx * abx;
	if (dot <= 0) return 4 * ap2 <= FRP_BAND_HALF2;
	if (dot >= ab2)
	{
		const int64_t bpy = py - by, bpx = px - bx;
		return 4 * (bpy * bpy + bpx * bpx) <= FRP_BAND_HALF2;
	}
	return 4 * (ap2 * ab2 - dot * dot) <= FRP_BAND_HALF2 * ab2;
}

// the goal rule (astar.py:1594, 1634, 1732-1747): the end cell's raster index, or -1 for an empty path
FRP_HD int64_t frp_end_cell(const uint64_t* field, const uint8_t* occ_plan, int H, int W, int start_y, int start_x, int gy, int gx)
{
	if (gy < 0 || gy >= H || gx < 0 || gx >= W) return -1;
	if (occ_plan[(size_t)gy * W + gx]) return -1;
	int64_t best = -1;
	uint32_t best_bits = 0;
	for (int y = gy - 1; y <= gy + 1; y++)
		for (int x = gx - 1; x <= gx + 1; x++)
		{
			if (y < 0 || y >= H || x < 0 || x >= W) continue;
			const uint64_t w = field[(size_t)y * W + x];
			if (w == FRP_UNREACHED) continue;
			const uint32_t bits = (uint32_t)(w >> 32);
			if (best < 0 || bits < best_bits) { best = (int64_t)y * W + x; best_bits = bits; }
		}
	if (best == (int64_t)start_y * W + start_x) return -1;
	return best;
}
#endif
