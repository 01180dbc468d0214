// g++ build of the keyframe overlap's arithmetic (csrc/fr_keyframe_math.h, over csrc/fr_ingest_math.h) for CPU-side checks: the
// per-point functions are the headers', the same ones the kernels compile; the compaction, the all-pairs duplicate filter and the
// counts are written here as plain loops -- what the ballot counts, the scan, the LDS tiles and the integer atomics of
// csrc/fr_keyframe.hip have to reproduce.
#include <cstdint>
#include <vector>
#include "../../fisher-nerf-customized_amd/csrc/fr_keyframe_math.h"

extern "C" {

// idx [H W] (count entries written): ascending flat indices of depth > 0 (& mask != 0); status [4] = {count, 0, 0, 0}
void frk_valid_pixels(int H, int W, const float* depth, const uint8_t* mask, int32_t* idx, int32_t* status)
{
	int32_t count = 0;
	for (int64_t p = 0; p < (int64_t)H * W; p++)
		if (depth[p] > 0.0f && (!mask || mask[p] != 0)) idx[count++] = (int32_t)p;
	status[0] = count; status[1] = 0; status[2] = 0; status[3] = 0;
}

float frk_key_of(float p) { return frk_key(p); }

// masks: K host addresses of byte masks [H,W] (0: none), or null.  counts [K], valid [n], pts [n,3], status [4] = {valid points,
// out-of-range draws, 0, 0}; uv [K,n,2] (may be null): the projections, for the margins of the tests
void frk_overlap(int H, int W, int n, int K, int edge, int n_valid_idx, const float* intr, const float* w2c, const float* depth,
                 const int32_t* valid_idx, const int64_t* draws, const float* kf_w2c, const uint64_t* masks,
                 int32_t* counts, uint8_t* valid, float* pts, int32_t* status, float* uv)
{
	float m[12];
	fri_invert_affine(w2c, m);
	const int64_t hw = (int64_t)H * W, limit = valid_idx ? (int64_t)n_valid_idx : hw;
	std::vector<float> keys(3 * (size_t)n);
	std::vector<uint8_t> oor(n);
	int32_t n_oor = 0, n_valid = 0;
	for (int i = 0; i < n; i++)
	{
		const int64_t d = draws[i];
		int64_t pix = -1;
		if (d >= 0 && d < limit) pix = valid_idx ? (int64_t)valid_idx[d] : d;
		oor[i] = !(pix >= 0 && pix < hw);
		pts[3 * i] = pts[3 * i + 1] = pts[3 * i + 2] = 0.0f;
		if (oor[i]) { n_oor++; continue; }
		fri_back_project((int)(pix % W), (int)(pix / W), depth[pix], intr[0], intr[4], intr[2], intr[5], m, pts + 3 * i);
		frk_keys(pts + 3 * i, &keys[3 * i]);
	}
	for (int i = 0; i < n; i++)
	{
		bool dup = oor[i] || frk_origin_key(&keys[3 * i]);
		for (int j = 0; j < n && !dup; j++)
			if (j != i && !oor[j]) dup = frk_same_key(&keys[3 * i], &keys[3 * j]);
		valid[i] = dup ? 0 : 1;
		n_valid += valid[i];
	}
	status[0] = n_valid; status[1] = n_oor; status[2] = 0; status[3] = 0;
	for (int k = 0; k < K; k++)
	{
		const uint8_t* mask = masks ? (const uint8_t*)(uintptr_t)masks[k] : nullptr;
		int32_t c = 0;
		for (int i = 0; i < n; i++)
		{
			float u = 0.0f, v = 0.0f;
			bool in = false;
			if (valid[i])
			{
				in = frk_project_inside(kf_w2c + 16 * (size_t)k, intr, pts + 3 * i, H, W, edge, &u, &v);
				if (in && mask) in = frk_mask_hit(mask, H, W, u, v);
			}
			if (uv) { uv[2 * ((size_t)k * n + i)] = u; uv[2 * ((size_t)k * n + i) + 1] = v; }
			c += in ? 1 : 0;
		}
		counts[k] = c;
	}
}

}
