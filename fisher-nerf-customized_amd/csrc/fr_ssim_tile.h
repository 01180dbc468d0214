// fr_ssim_tile.h -- the tiling of the 11 x 11 SSIM window that fr_loss.hip and fr_eval.hip share (device only).
//
// A workgroup of 256 threads takes a 16 x 16 pixel tile.  The two images of the tile lie in LDS with a halo of 5 as s_x, s_y
// [FRS_EXT][FRS_EXT] (each kernel loads them its own way); the horizontal 11-tap pass fills s_h, 5 moments x 26 rows x 16 columns,
// and the vertical pass gives every lane the five moments of its pixel.  The arithmetic is fr_loss_math.h's.
#ifndef FR_SSIM_TILE_H_INCLUDED
#define FR_SSIM_TILE_H_INCLUDED
#include "fr_loss_math.h"

#define FRS_TILE 16
#define FRS_EXT (FRS_TILE + 2 * FRL_RADIUS)      // 26
#define FRS_THREADS (FRS_TILE * FRS_TILE)

// the horizontal pass: MOMENTS (frl_conv11_moments, or another with its signature) over every row window of the tile.  The caller
// puts a barrier in front (s_x, s_y written; s_h free) and one behind.
template <void (*MOMENTS)(const float*, const float*, int, float*)>
__device__ __forceinline__ void frs_rows(const float* s_x, const float* s_y, float (*s_h)[FRS_EXT * FRS_TILE])
{
	for (int i = threadIdx.x; i < FRS_EXT * FRS_TILE; i += FRS_THREADS)
	{
		const int r = i / FRS_TILE, q = i % FRS_TILE;
		float h[5];
		MOMENTS(&s_x[r * FRS_EXT + q], &s_y[r * FRS_EXT + q], 1, h);
#pragma unroll
		for (int k = 0; k < 5; k++) s_h[k][i] = h[k];
	}
}

// the vertical pass: the five moments of pixel (lx, ly) of the tile
__device__ __forceinline__ void frs_columns(const float (*s_h)[FRS_EXT * FRS_TILE], int lx, int ly, float mo[5])
{
#pragma unroll
	for (int k = 0; k < 5; k++) mo[k] = frl_conv11(&s_h[k][ly * FRS_TILE + lx], FRS_TILE);
}

#endif
