// fr_sortnet.h -- the plan of the register-resident key sort (fisher_rast.hip: fr_sort_wave_segment / fr_sort_wg_segment),
// host/device-neutral: the kernels and the g++ harness (tests/harness/fr_sortnet_harness.cpp) compile these same comparator
// lists, level conditions, partner rules and dispatch tables, so a CPU run over a host model of the lanes checks what the
// kernels execute.  Only the exchanges themselves (DPP / permlane / LDS in the kernels, index arithmetic in the harness) differ.
//
// A wave holds a RUN of 64 K keys, element (lane l, register r) = l K + r, K any of 1 .. 8 (16 in the long-list tiers):
//
//   level 0      every lane sorts its own K keys                                            FrSnSort<K>
//   level M      (1 .. 6) merges the sorted blocks of 2^(M-1) lanes into blocks of 2^M lanes:
//                  flip           (l, r) <-> (l ^ (2^M - 1), K - 1 - r); the lower lane of a pair keeps the minimum.  The two halves
//                                 of a block are equally long for any K, which is all the flip needs: afterwards every key of the
//                                 lower half is <= every key of the upper, and both halves are bitonic.  For odd K the middle
//                                 register pairs with itself in the mirror lane.
//                  half-cleaners  (l, r) <-> (l ^ 2^t, r), t = M - 2 .. 0: a bitonic sequence of 2^(t+1) K keys into two of 2^t K
//                                 (equally long again, down to one lane)
//                  clean-up       a lane is left with a bitonic sequence of its K keys (in the cyclic sense: a rotation
//                                 of rise-then-fall) and sorts it                                  FrSnClean<K>
//   A level is skipped when the blocks it would merge already hold all n keys (fr_sn_wave_level): the keys at and beyond n are
//   +inf, so they are at the end from level 0 on.
//
// Four (or sixteen) waves join their runs through LDS the same way, a run taking a lane's place: levels SW = 1 .. log2 NW,
//   flip (w, l, r) <-> (w ^ (2^SW - 1), 63 - l, K - 1 - r), half-cleaners w ^ 2^t, then the half-cleaners of lane strides 32 .. 1
//   and the clean-up inside every run.
//
// For K a power of two the in-lane steps are the stages of the same flip network on the lane's registers (FrSnSort: stages 2, 4,
// .. K; FrSnClean: strides K/2 .. 1), which is what the kernels' power-of-two instantiations have always run.  For the other K
// they are fixed comparator lists: FrSnSort an optimal sorting network (3 / 9 / 12 / 16 comparators for 3 / 5 / 6 / 7 keys),
// FrSnClean the shortest list found (breadth-first over the sets of reachable zero-one inputs) that sorts every cyclically bitonic
// sequence: 3 / 8 / 9 / 12 comparators.  The harness checks each list exhaustively by the zero-one principle.
#ifndef FR_SORTNET_H_INCLUDED
#define FR_SORTNET_H_INCLUDED

#include <stdint.h>

#if defined(__HIPCC__)
#define FRSN_HD __host__ __device__ __forceinline__
#else
#define FRSN_HD inline
#endif

#define FR_SN_LANES 64
#define FR_SN_LANE_LEVELS 6          // log2 FR_SN_LANES

struct FrSnCmp { unsigned char a, b; };          // compare-exchange of registers a < b: the minimum to a

FRSN_HD constexpr bool fr_sn_pow2(int K) { return (K & (K - 1)) == 0; }

// ---- level 0: a lane's K keys, any order -> ascending
template <int K> struct FrSnSort;
#define FR_SN_LIST(NAME, K_, N_, ...) \
	template <> struct NAME<K_> { static constexpr int N = N_; \
		static FRSN_HD constexpr FrSnCmp at(int i) { constexpr FrSnCmp c[N_ ? N_ : 1] = {__VA_ARGS__}; return c[i]; } };
FR_SN_LIST(FrSnSort, 1, 0, {0, 0})
FR_SN_LIST(FrSnSort, 2, 1, {0, 1})
FR_SN_LIST(FrSnSort, 3, 3, {0, 2}, {0, 1}, {1, 2})
FR_SN_LIST(FrSnSort, 4, 6, {0, 1}, {2, 3}, {0, 3}, {1, 2}, {0, 1}, {2, 3})
FR_SN_LIST(FrSnSort, 5, 9, {0, 3}, {1, 4}, {0, 2}, {1, 3}, {0, 1}, {2, 4}, {1, 2}, {3, 4}, {2, 3})
FR_SN_LIST(FrSnSort, 6, 12, {0, 5}, {1, 3}, {2, 4}, {1, 2}, {3, 4}, {0, 3}, {2, 5}, {0, 1}, {2, 3}, {4, 5}, {1, 2}, {3, 4})
FR_SN_LIST(FrSnSort, 7, 16, {0, 6}, {2, 3}, {4, 5}, {0, 2}, {1, 4}, {3, 6}, {0, 1}, {2, 5}, {3, 4}, {1, 2}, {4, 6}, {2, 3}, {4, 5},
           {1, 2}, {3, 4}, {5, 6})
FR_SN_LIST(FrSnSort, 8, 24, {0, 1}, {2, 3}, {4, 5}, {6, 7}, {0, 3}, {1, 2}, {4, 7}, {5, 6}, {0, 1}, {2, 3}, {4, 5}, {6, 7},
           {0, 7}, {1, 6}, {2, 5}, {3, 4}, {0, 2}, {1, 3}, {4, 6}, {5, 7}, {0, 1}, {2, 3}, {4, 5}, {6, 7})

// ---- after a merge level: a lane's K keys, cyclically bitonic -> ascending
template <int K> struct FrSnClean;
FR_SN_LIST(FrSnClean, 1, 0, {0, 0})
FR_SN_LIST(FrSnClean, 2, 1, {0, 1})
FR_SN_LIST(FrSnClean, 3, 3, {0, 1}, {0, 2}, {1, 2})
FR_SN_LIST(FrSnClean, 4, 4, {0, 2}, {1, 3}, {0, 1}, {2, 3})
FR_SN_LIST(FrSnClean, 5, 8, {0, 1}, {0, 2}, {0, 3}, {0, 4}, {1, 3}, {2, 4}, {1, 2}, {3, 4})
FR_SN_LIST(FrSnClean, 6, 9, {0, 2}, {0, 4}, {1, 3}, {1, 5}, {0, 1}, {2, 4}, {3, 5}, {2, 3}, {4, 5})
FR_SN_LIST(FrSnClean, 7, 12, {0, 1}, {0, 4}, {2, 6}, {3, 5}, {1, 5}, {2, 3}, {4, 6}, {1, 3}, {0, 2}, {1, 2}, {3, 4}, {5, 6})
FR_SN_LIST(FrSnClean, 8, 12, {0, 4}, {1, 5}, {2, 6}, {3, 7}, {0, 2}, {1, 3}, {4, 6}, {5, 7}, {0, 1}, {2, 3}, {4, 5}, {6, 7})
#undef FR_SN_LIST

// ---- which levels a run of n keys needs
// level M of a wave (1 .. 6) merges blocks of 2^(M-1) lanes: needed while one such block does not hold all n keys
FRSN_HD constexpr bool fr_sn_wave_level(int K, int M, uint32_t n) { return ((uint32_t)K << (M - 1)) < n; }
// level SW of a workgroup (1 .. log2 NW) merges blocks of 2^(SW-1) runs
FRSN_HD constexpr bool fr_sn_wg_level(int K, int SW, uint32_t n) { return ((uint32_t)(FR_SN_LANES * K) << (SW - 1)) < n; }

// ---- partners.  `unit`: the lane inside a wave, or the wave inside a workgroup.
FRSN_HD constexpr int fr_sn_flip_unit(int unit, int M) { return unit ^ ((1 << M) - 1); }
FRSN_HD constexpr int fr_sn_flip_reg(int K, int r) { return K - 1 - r; }
FRSN_HD constexpr bool fr_sn_flip_keepmin(int unit, int M) { return (unit & (1 << (M - 1))) == 0; }
FRSN_HD constexpr int fr_sn_xor_unit(int unit, int t) { return unit ^ (1 << t); }
FRSN_HD constexpr bool fr_sn_xor_keepmin(int unit, int t) { return (unit & (1 << t)) == 0; }

// ---- dispatch: keys per lane for a list or part of n keys (the smallest instantiated K that holds it)
// Bit K of a mask: K keys per lane is instantiated (8 always is).  The defaults are what measured (profiles/NOTES.md round 7); a build
// with -DFR_SN_WAVE_KS=... / -DFR_SN_WG4_KS=... leaves some out for an A/B (a K that is not dispatched to is not compiled).
#ifndef FR_SN_WAVE_KS
#define FR_SN_WAVE_KS 0x1FE          // one wave: 1 .. 8
#endif
#ifndef FR_SN_WG4_KS
#define FR_SN_WG4_KS 0x1F8           // four waves: 3 .. 8
#endif
FRSN_HD constexpr bool fr_sn_has(int mask, int K) { return ((mask >> K) & 1) != 0; }
FRSN_HD constexpr int fr_sn_pick_k(int mask, uint32_t n, uint32_t per_k)
{
	for (int K = 1; K < 8; K++)
		if (fr_sn_has(mask, K) && n <= per_k * (uint32_t)K) return K;
	return 8;
}
// one wave, 2 <= n <= 512
FRSN_HD constexpr int fr_sn_wave_k(uint32_t n) { return fr_sn_pick_k(FR_SN_WAVE_KS, n, FR_SN_LANES); }
// four waves, 513 <= n <= 2048
FRSN_HD constexpr int fr_sn_wg4_k(uint32_t n) { return fr_sn_pick_k(FR_SN_WG4_KS, n, 4 * FR_SN_LANES); }

#endif
