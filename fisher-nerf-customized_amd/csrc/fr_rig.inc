// fr_rig.inc -- the experiment rig of fisher_rast.hip.  Always included; without one of the macros below every hook here expands to
// nothing, and the product build reads no environment variable.
//
//   -DFR_AB         host switches and knobs, read once per process from the environment (tools/build_variant.sh, ab.sh, ab_env.sh):
//                   FR_DEBUG_MODE
//                      1  k_fisher_tile_v2 stops after its first pass         7  every sort tier on the caller's stream (no fork)
//                      9  the second-generation two-pass kernels instead of k_fisher_tile_v3 / _v4 / _v3h
//                     15  early frustum test of the front end off            19  dense records instead of compact ones
//                     22  k_fisher_tile_v2 instead of k_fisher_tile_v3g      27  views in index order, not dealt over the XCDs by weight
//                     32  no list partitioning in the sort stage             33  never the chunked backward
//                   FR_GV / FR_VC (Gaussians per thread / views per workgroup of the multi-view front end), FR_GROUPS, FR_TILE_PRIO,
//                   FR_PART_MIN, FR_SPLIT_BLOCKS, FR_PART_BLOCKS: see where they are read.
//   -DFR_LOOPSTATS  (implies FR_AB) loop-trip counters and s_memtime shares of the scoring tile kernels; FR_LOOPSTATS_MODE selects the
//                   one a tile returns in place of its score (tools/loopstats.py; the numbers are listed at FrLoopStats::walk_result).
//   -DFR_ABLATE     (implies FR_AB) FR_ABLATE_MODE leaves parts of product kernels out (tools/fe_ablate.py): 28 / 29 in the out_H and
//                   point walks, 30..37 in the front end (every mode from 30 up also raises the overflow flag).
//   -DFR_FWD_STATS  counters of k_render_forward_walk in place of the depth of a wave's first eight pixels (tools/fwd_walk_stats.py).
// The three mode variables are separate on purpose: the numbers of one rig mean nothing to the others.
#if defined(FR_ABLATE) || defined(FR_LOOPSTATS)
#ifndef FR_AB
#define FR_AB
#endif
#endif

#ifdef FR_AB
#define FR_AB_ONLY(x) x
static int fr_env_int(const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; }
static int fr_debug_mode() { static const int mode = fr_env_int("FR_DEBUG_MODE"); return mode; }
#else
#define FR_AB_ONLY(x)
static constexpr int fr_debug_mode() { return 0; }
#endif

#ifdef FR_ABLATE
#define FR_ABL(x) x
#define FR_ABL_OR(x, y) x
static int fr_ablate_mode() { static const int mode = fr_env_int("FR_ABLATE_MODE"); return mode; }
#else
#define FR_ABL(x)
#define FR_ABL_OR(x, y) y
#endif

// ---- loop statistics: FR_STATS_DECLARE once per kernel, FR_STATS(counting statement), FR_STATS_START / FR_STATS_STAMP(ts | tc | tw)
// around a phase, FR_STATS_RESULT at the end
#ifdef FR_LOOPSTATS
static int fr_loopstats_mode() { static const int mode = fr_env_int("FR_LOOPSTATS_MODE"); return mode; }
__device__ __forceinline__ float wave_sum(float v);
__device__ __forceinline__ int wave_max_i(int v);
struct FrLoopStats {
	int cand = 0, chunks = 0, steps = 0, hits = 0, wsteps = 0, cs = 0, empty = 0, p1any = 0, p1con = 0;
	long long t0 = 0, ts = 0, tc = 0, tw = 0;     // s_memtime: start of the running phase; sums of the key stream / chunk set-up / walk
	__device__ __forceinline__ void start() { t0 = (long long)__builtin_amdgcn_s_memtime(); }
	__device__ __forceinline__ void stamp(long long& acc) { const long long t = (long long)__builtin_amdgcn_s_memtime(); acc += t - t0; t0 = t; }
	// a chunk's walk costs the wave as many iterations as its busiest lane took steps
	__device__ __forceinline__ void end_chunk() { wsteps += wave_max_i(cs); cs = 0; }
	// k_fisher_tile_v3 / _v4, per wave (the tile's score is the sum over its four waves):
	//   2 candidates   3 chunks   4 wave-level walk iterations   5 contributing pairs   6 lane-level walk steps   7 steps of the busiest lane
	//   10 / 11 / 12 s_memtime ticks (/ 64) in the key stream / the chunk set-up / the walk
	//   13 keys streamed before the wave's 64 pixels were finished   14 the tile's keys   15 candidates parked with an empty footprint mask
	__device__ __forceinline__ float walk_result(int mode, uint32_t base, uint32_t n) const
	{
		if (mode == 15) return (float)empty;
		if (mode == 13) return (float)(base < n ? base : n);
		if (mode == 14) return (float)n;
		if (mode >= 10) return (float)((mode == 10 ? ts : mode == 11 ? tc : tw) >> 6);
		return mode == 2 ? (float)cand : mode == 3 ? (float)chunks : mode == 4 ? (float)wsteps
		     : mode == 5 ? wave_sum((float)hits) : mode == 7 ? (float)wave_max_i(steps) : wave_sum((float)steps);
	}
	// k_fisher_tile_v2, per wave: 2 first-pass candidates, 3 chunks, 4 walk steps, 5 contributing pairs, 7 / 8 first-pass candidates
	// that pass the pair test on some pixel / contribute to one; else the length of the wave's list
	__device__ __forceinline__ float two_pass_result(int mode, int wcnt) const
	{
		return mode == 2 ? (float)cand : mode == 3 ? (float)chunks : mode == 4 ? (float)steps : mode == 5 ? (float)hits
		     : mode == 7 ? (float)p1any : mode == 8 ? (float)p1con : (float)wcnt;
	}
};
#define FR_STATS(x) x
#define FR_STATS_DECLARE FrLoopStats ls;
#define FR_STATS_START ls.start();
#define FR_STATS_STAMP(acc) ls.stamp(ls.acc);
#define FR_STATS_RESULT(ws, base, n) if (f.stat_mode >= 2) ws = ls.walk_result(f.stat_mode, base, n);
#define FR_STATS_RESULT_V2(ws, wcnt) if (f.stat_mode >= 2) ws = ls.two_pass_result(f.stat_mode, wcnt);
#else
#define FR_STATS(x)
#define FR_STATS_DECLARE
#define FR_STATS_START
#define FR_STATS_STAMP(acc)
#define FR_STATS_RESULT(ws, base, n)
#define FR_STATS_RESULT_V2(ws, wcnt)
#endif

// the rig's fields of FrFisherArgs, filled where the host builds one
#define FR_RIG_ARGS(f) FR_AB_ONLY(f.debug_mode = fr_debug_mode();) FR_STATS(f.stat_mode = fr_loopstats_mode();) FR_ABL(f.ablate = fr_ablate_mode();)

// ---- forward-walk probes: FR_FWD_DECLARE, FR_FWD(statement), FR_FWD_STAMP(stream | setup | walk)
#ifdef FR_FWD_STATS
struct FrFwdStats {
	long long t0, stream = 0, setup = 0, walk = 0;
	uint32_t chunks = 0, steps = 0, windows = 0;
	__device__ __forceinline__ FrFwdStats() { t0 = (long long)__builtin_amdgcn_s_memtime(); }
	__device__ __forceinline__ void stamp(long long& acc) { const long long t = (long long)__builtin_amdgcn_s_memtime(); acc += t - t0; t0 = t; }
	// one more chunk; its walk takes as many steps as the busiest lane has candidates
	__device__ __forceinline__ void chunk(unsigned long long mask)
	{
		chunks++;
		uint32_t pc = (uint32_t)__popcll(mask);
		for (int o = 32; o > 0; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)pc, o, 64); pc = t > pc ? t : pc; }
		steps += pc;
	}
	// what lane 0..7 writes in place of its pixel's depth
	__device__ __forceinline__ float result(int lane, uint32_t n) const
	{
		const float vals[8] = { (float)(stream >> 6), (float)(setup >> 6), (float)(walk >> 6), (float)chunks, (float)steps, (float)windows, (float)n, 0.f };
		return vals[lane];
	}
};
#define FR_FWD(x) x
#define FR_FWD_DECLARE FrFwdStats fs;
#define FR_FWD_STAMP(acc) fs.stamp(fs.acc);
#else
#define FR_FWD(x)
#define FR_FWD_DECLARE
#define FR_FWD_STAMP(acc)
#endif
