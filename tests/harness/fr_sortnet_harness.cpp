// g++ build of the register-resident key sort's plan (csrc/fr_sortnet.h) for CPU-side checks: the comparator lists, the level
// conditions, the partner rules and the dispatch tables are the header's, the same ones fr_sort_wave_segment / fr_sort_wg_segment of
// csrc/fisher_rast.hip compile; the lanes are an array here and the exchanges index arithmetic.
// With -DFR_SORTNET_MAIN the file is a program of its own (for a sanitizer build: g++ -fsanitize=address,undefined).
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../fisher-nerf-customized_amd/csrc/fr_sortnet.h"

namespace {

constexpr int LANES = FR_SN_LANES;

inline void cx(uint64_t& lo, uint64_t& hi) { if (lo > hi) std::swap(lo, hi); }
// fr_take of the kernels
inline uint64_t take(uint64_t mine, uint64_t other, bool keepmin) { return ((other < mine) == keepmin) ? other : mine; }

template <class L, int K> void lane_net(uint64_t* key)
{
	for (int i = 0; i < L::N; i++) { const FrSnCmp c = L::at(i); cx(key[c.a], key[c.b]); }
}

// NW runs of LANES x K keys, key[(w * LANES + l) * K + r] = element (w, l, r) = position w 64 K + l K + r
template <int K> struct Model
{
	int NW;
	std::vector<uint64_t> key, tmp;
	uint64_t& at(int w, int l, int r) { return key[(size_t)((w * LANES + l) * K + r)]; }
	uint64_t& nx(int w, int l, int r) { return tmp[(size_t)((w * LANES + l) * K + r)]; }

	void clean() { for (int u = 0; u < NW * LANES; u++) lane_net<FrSnClean<K>, K>(&key[(size_t)u * K]); }
	void lane_xor(int t)
	{
		for (int w = 0; w < NW; w++) for (int l = 0; l < LANES; l++) for (int r = 0; r < K; r++)
			nx(w, l, r) = take(at(w, l, r), at(w, fr_sn_xor_unit(l, t), r), fr_sn_xor_keepmin(l, t));
		key.swap(tmp);
	}
	void wave_levels(uint32_t n)
	{
		for (int u = 0; u < NW * LANES; u++) lane_net<FrSnSort<K>, K>(&key[(size_t)u * K]);
		for (int M = 1; M <= FR_SN_LANE_LEVELS; M++)
		{
			if (!fr_sn_wave_level(K, M, n)) continue;
			for (int w = 0; w < NW; w++) for (int l = 0; l < LANES; l++) for (int r = 0; r < K; r++)
				nx(w, l, r) = take(at(w, l, r), at(w, fr_sn_flip_unit(l, M), fr_sn_flip_reg(K, r)), fr_sn_flip_keepmin(l, M));
			key.swap(tmp);
			for (int t = M - 2; t >= 0; t--) lane_xor(t);
			clean();
		}
	}
	void wg_levels(uint32_t n)
	{
		int LW = 0;
		while ((1 << LW) < NW) LW++;
		for (int SW = 1; SW <= LW; SW++)
		{
			if (!fr_sn_wg_level(K, SW, n)) continue;
			for (int w = 0; w < NW; w++) for (int l = 0; l < LANES; l++) for (int r = 0; r < K; r++)
				nx(w, l, r) = take(at(w, l, r), at(fr_sn_flip_unit(w, SW), LANES - 1 - l, fr_sn_flip_reg(K, r)), fr_sn_flip_keepmin(w, SW));
			key.swap(tmp);
			for (int t = SW - 2; t >= 0; t--)
			{
				for (int w = 0; w < NW; w++) for (int l = 0; l < LANES; l++) for (int r = 0; r < K; r++)
					nx(w, l, r) = take(at(w, l, r), at(fr_sn_xor_unit(w, t), l, r), fr_sn_xor_keepmin(w, t));
				key.swap(tmp);
			}
			for (int t = FR_SN_LANE_LEVELS - 1; t >= 0; t--) lane_xor(t);
			clean();
		}
	}
	// what fr_sort_wave_segment (NW = 1) / fr_sort_wg_segment (NW = 4, 16) do to n keys of a segment
	void sort(uint64_t* gk, uint32_t n, int nw)
	{
		NW = nw;
		const size_t cap = (size_t)NW * LANES * K;
		key.assign(cap, ~0ull); tmp.assign(cap, ~0ull);
		for (size_t i = 0; i < cap && i < n; i++) key[i] = gk[i];
		wave_levels(n);
		wg_levels(n);
		for (size_t i = 0; i < cap && i < n; i++) gk[i] = key[i];
	}
};

template <int K> int list_failures(int which)
{
	int bad = 0;
	if (which == 0)
	{
		for (unsigned v = 0; v < (1u << K); v++)
		{
			uint64_t key[K];
			for (int r = 0; r < K; r++) key[r] = (v >> r) & 1u;
			lane_net<FrSnSort<K>, K>(key);
			bad += !std::is_sorted(key, key + K);
		}
		return bad;
	}
	// every cyclically bitonic zero-one sequence: one run of ones, of any length, starting anywhere, wrapping round
	for (int start = 0; start < K; start++)
		for (int len = 0; len <= K; len++)
		{
			uint64_t key[K];
			for (int r = 0; r < K; r++) key[r] = 0;
			for (int i = 0; i < len; i++) key[(start + i) % K] = 1;
			lane_net<FrSnClean<K>, K>(key);
			bad += !std::is_sorted(key, key + K);
		}
	return bad;
}

template <int K> int run_k(int nw, uint64_t* keys, uint32_t n)
{
	std::vector<uint64_t> want(keys, keys + n);
	std::sort(want.begin(), want.end());
	Model<K> m;
	m.sort(keys, n, nw);
	int bad = 0;
	for (uint32_t i = 0; i < n; i++) bad += keys[i] != want[i];
	return bad;
}

}

#define FRSN_BY_K(K, CALL) \
	switch (K) { case 1: { constexpr int KK = 1; return CALL; } case 2: { constexpr int KK = 2; return CALL; } case 3: { constexpr int KK = 3; return CALL; } \
	             case 4: { constexpr int KK = 4; return CALL; } case 5: { constexpr int KK = 5; return CALL; } case 6: { constexpr int KK = 6; return CALL; } \
	             case 7: { constexpr int KK = 7; return CALL; } case 8: { constexpr int KK = 8; return CALL; } default: return -1; }

extern "C" {

// comparators in a list (which: 0 FrSnSort, 1 FrSnClean)
int frsn_list_len(int K, int which) { FRSN_BY_K(K, (which == 0 ? FrSnSort<KK>::N : FrSnClean<KK>::N)) }
// inputs the list leaves unsorted: all 2^K zero-one inputs (FrSnSort), all cyclically bitonic zero-one inputs (FrSnClean)
int frsn_list_failures(int K, int which) { FRSN_BY_K(K, list_failures<KK>(which)) }
// n <= nw * 64 * K keys sorted in place by the plan; returns the positions that differ from std::sort
int frsn_sort_run(int K, int nw, uint64_t* keys, uint32_t n) { FRSN_BY_K(K, run_k<KK>(nw, keys, n)) }
int frsn_wave_k(uint32_t n) { return fr_sn_wave_k(n); }
int frsn_wg4_k(uint32_t n) { return fr_sn_wg4_k(n); }
int frsn_wave_ks() { return FR_SN_WAVE_KS; }
int frsn_wg4_ks() { return FR_SN_WG4_KS; }

}

#ifdef FR_SORTNET_MAIN
int main()
{
	int bad = 0;
	uint64_t s = 0x9E3779B97F4A7C15ull;
	auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
	for (int K = 1; K <= 8; K++)
	{
		bad += frsn_list_failures(K, 0) + frsn_list_failures(K, 1);
		for (int nw = 1; nw <= 4; nw *= 4)
			for (int trial = 0; trial < 40; trial++)
			{
				const uint32_t cap = (uint32_t)(nw * 64 * K), n = trial == 0 ? cap : 2u + (uint32_t)(rnd() % (cap - 1u));
				std::vector<uint64_t> k(n);
				for (auto& x : k) x = trial % 3 == 1 ? rnd() % 7 : rnd();
				bad += frsn_sort_run(K, nw, k.data(), n);
			}
	}
	printf("fr_sortnet: %d failures\n", bad);
	return bad != 0;
}
#endif
