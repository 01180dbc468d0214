// fr_block.h -- workgroup primitives shared by the .hip units of libfisher_rast.so (device only; gfx950, wave64).
//
// Everything here is written for a workgroup of FRB_THREADS = 256 threads, four waves of 64, and every thread of the workgroup
// must call a helper that has a barrier in it (each says so): the call sits in front of any divergent return of its kernel.
// Integer helpers give results that do not depend on the launch geometry; the fp64 sums add in one fixed order (lanes by a
// __shfl_down tree, 32 down to 1, then the four waves in index order), so the same call gives the same bits.
#ifndef FR_BLOCK_H_INCLUDED
#define FR_BLOCK_H_INCLUDED
#include <hip/hip_runtime.h>
#include <stdint.h>

#define FRB_THREADS 256
#define FRB_WAVES (FRB_THREADS / 64)

// ---- scan, count, rank ------------------------------------------------------------------------------------------------------------

// inclusive scan of one value per thread over the 256 threads of the workgroup; s_wave[4] is scratch (free again on return).
// Two barriers.
__device__ __forceinline__ uint32_t frb_scan256(uint32_t c, uint32_t* s_wave, uint32_t& total)
{
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	uint32_t incl = c;
#pragma unroll
	for (int o = 1; o < 64; o <<= 1)
	{
		const uint32_t v = __shfl_up(incl, o, 64);
		if (lane >= o) incl += v;
	}
	if (lane == 63) s_wave[wave] = incl;
	__syncthreads();
	uint32_t base = 0;
	for (int w = 0; w < wave; w++) base += s_wave[w];
	total = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
	__syncthreads();
	return incl + base;
}

// number of set predicates in the workgroup, for every thread (s_wave[4] is scratch, in use until the next barrier).  One barrier.
__device__ __forceinline__ uint32_t frb_count256(bool sel, uint32_t* s_wave)
{
	const unsigned long long ballot = __ballot(sel);
	if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = (uint32_t)__popcll(ballot);
	__syncthreads();
	return ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

// number of set predicates in front of this thread in the workgroup: the slot of an ordered compaction.  One barrier.
__device__ __forceinline__ uint32_t frb_rank256(bool sel, uint32_t* s_wave)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const unsigned long long ballot = __ballot(sel);
	if (lane == 0) s_wave[wave] = (uint32_t)__popcll(ballot);
	__syncthreads();
	uint32_t before = (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
	for (int w = 0; w < wave; w++) before += s_wave[w];
	return before;
}

// one workgroup: offsets[] = exclusive scan of counts[0 .. nwg), in rounds of 256 with a carry; returns the total.  Barriers:
// the whole workgroup calls it, with the same nwg.
__device__ __forceinline__ uint32_t frb_scan_counts(const uint32_t* counts, uint32_t* offsets, int nwg, uint32_t* s_wave)
{
	const int tid = threadIdx.x;
	uint32_t carry = 0u;
	for (int base = 0; base < nwg; base += FRB_THREADS)
	{
		const int i = base + tid;
		const uint32_t c = i < nwg ? counts[i] : 0u;
		uint32_t total;
		const uint32_t incl = frb_scan256(c, s_wave, total);
		if (i < nwg) offsets[i] = carry + (incl - c);
		carry += total;
	}
	return carry;
}

// ---- radix select -----------------------------------------------------------------------------------------------------------------
// The order statistic of rank k among 32-bit keys whose unsigned order is the wanted order, most significant byte first: pass p
// counts byte 3 - p of the keys that share the prefix the passes before it fixed, into hist[p][256].  Integer sums only.

// the bucket of histogram h that holds rank k, for every thread; k becomes the rank inside that bucket and `inside` the number of
// values in it.  s_wave[4], s_out[3] are scratch.  Barriers.
__device__ __forceinline__ uint32_t frb_select_pick(const uint32_t* __restrict__ h, uint32_t& k, uint32_t& inside, uint32_t* s_wave, uint32_t* s_out)
{
	const int tid = threadIdx.x;
	const uint32_t c = h[tid];
	uint32_t total;
	const uint32_t incl = frb_scan256(c, s_wave, total);
	if (tid == 0) { s_out[0] = 255u; s_out[1] = 0u; s_out[2] = 0u; }      // rank k lies past the counted values: the result is not used
	__syncthreads();
	if (incl > k && incl - c <= k) { s_out[0] = (uint32_t)tid; s_out[1] = k - (incl - c); s_out[2] = c; }
	__syncthreads();
	const uint32_t bucket = s_out[0];
	k = s_out[1];
	inside = s_out[2];
	__syncthreads();
	return bucket;
}

// the prefix that the first `passes` histograms fix for rank k; k becomes the rank left inside it, `inside` the values that share it
__device__ __forceinline__ uint32_t frb_select_prefix(const uint32_t* hist, int passes, uint32_t& k, uint32_t& inside, uint32_t* s_wave, uint32_t* s_out)
{
	uint32_t prefix = 0u;
	for (int p = 0; p < passes; p++) prefix = (prefix << 8) | frb_select_pick(hist + 256 * p, k, inside, s_wave, s_out);
	return prefix;
}

// pass PASS counts key u into the workgroup's LDS histogram when u has the prefix of the passes before
template <int PASS>
__device__ __forceinline__ void frb_select_count(uint32_t* s_hist, uint32_t u, uint32_t prefix)
{
	constexpr int shift = 24 - 8 * PASS;
	if (PASS == 0 || (u >> ((shift + 8) & 31)) == prefix) atomicAdd(&s_hist[(u >> shift) & 255u], 1u);
}

// the workgroup's LDS histogram added to histogram PASS in memory (the caller has put a barrier after the last frb_select_count)
template <int PASS>
__device__ __forceinline__ void frb_select_flush(uint32_t* hist, const uint32_t* s_hist)
{
	const int tid = threadIdx.x;
	if (s_hist[tid]) atomicAdd(&hist[256 * PASS + tid], s_hist[tid]);
}

// ---- fp64 sums in a fixed order ---------------------------------------------------------------------------------------------------

// v[0 .. N) of every thread summed over the workgroup: on return (behind the barrier in here) s_red[j][0 .. 4) holds the four wave
// sums of v[j], which frb_sum4 adds.  v is left with the wave's sums in lane 0 of each wave.
template <int N>
__device__ __forceinline__ void frb_sum256(double* v, double (*s_red)[FRB_WAVES])
{
	const int tid = threadIdx.x;
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
	{
#pragma unroll
		for (int j = 0; j < N; j++) v[j] += __shfl_down(v[j], o, 64);
	}
	if ((tid & 63) == 0)
	{
#pragma unroll
		for (int j = 0; j < N; j++) s_red[j][tid >> 6] = v[j];
	}
	__syncthreads();
}
__device__ __forceinline__ double frb_sum4(const double* r) { return ((r[0] + r[1]) + r[2]) + r[3]; }

// one wave adds row[0 .. T): lane l adds l, l + 64, .. in index order, then the lanes are added in the tree; the sum is in lane 0.
// No barrier: a wave may call it alone.
__device__ __forceinline__ double frb_row_sum(const double* row, int T)
{
	double s = 0.0;
	for (int t = (int)(threadIdx.x & 63); t < T; t += 64) s += row[t];
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
	return s;
}

// ---- the frame of a cloud ---------------------------------------------------------------------------------------------------------

// min / max / count of the finite points among pts[0 .. n) (grid-strided), by lane, wave (an xor tree: min, max and integer adds do
// not depend on the order) and workgroup: on return (behind the barrier in here) s_lo[k][w], s_hi[k][w], s_cnt[w] hold wave w's
// values of axis k.  finite3(x, y, z) is the unit's own test (its *_math.h): a non-finite point must not widen the frame.  The
// caller encodes and issues its own atomics.
template <typename F>
__device__ __forceinline__ void frb_minmax3_finite(const float* __restrict__ pts, int n, F finite3, float (*s_lo)[FRB_WAVES],
                                                   float (*s_hi)[FRB_WAVES], uint32_t* s_cnt)
{
	float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
	uint32_t cnt = 0;
	for (int i = blockIdx.x * FRB_THREADS + threadIdx.x; i < n; i += gridDim.x * FRB_THREADS)
	{
		const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
		if (!finite3(x, y, z)) continue;
		lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
		lo[1] = fminf(lo[1], y); hi[1] = fmaxf(hi[1], y);
		lo[2] = fminf(lo[2], z); hi[2] = fmaxf(hi[2], z);
		cnt++;
	}
#pragma unroll
	for (int o = 32; o > 0; o >>= 1)
	{
#pragma unroll
		for (int k = 0; k < 3; k++) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], o, 64)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], o, 64)); }
		cnt += __shfl_xor(cnt, o, 64);
	}
	if ((threadIdx.x & 63) == 0)
	{
		for (int k = 0; k < 3; k++) { s_lo[k][threadIdx.x >> 6] = lo[k]; s_hi[k][threadIdx.x >> 6] = hi[k]; }
		s_cnt[threadIdx.x >> 6] = cnt;
	}
	__syncthreads();
}
__device__ __forceinline__ float frb_min4(const float* r) { return fminf(fminf(r[0], r[1]), fminf(r[2], r[3])); }
__device__ __forceinline__ float frb_max4(const float* r) { return fmaxf(fmaxf(r[0], r[1]), fmaxf(r[2], r[3])); }

#endif
