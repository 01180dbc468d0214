// fr_internal.h -- shared between the translation units of libfisher_rast.so (not part of the C ABI).
#ifndef FR_INTERNAL_H_INCLUDED
#define FR_INTERNAL_H_INCLUDED
#include "../../include/fisher_rast.h"

// records the message for fr_last_error() (thread-local) and returns `code`
__attribute__((visibility("hidden"))) int fr_fail(int code, const char* msg);
// FR_OK, or FR_ELAUNCH with hipGetErrorString of the pending launch error
__attribute__((visibility("hidden"))) int fr_check_launch(const char* what);
// ascending sort of n 64-bit device keys in place on `stream` (fisher_rast.hip: the bitonic network of the Morton sort); n = 0 is fine
__attribute__((visibility("hidden"))) int fr_sort_keys64(uint64_t* keys, uint32_t n, fr_stream_t stream);
// fr_fisher_views with cfg->ext set (non-null): the POp-GS block stage over probe rows (fr_popgs_block.hip; contract in fisher_rast.h)
__attribute__((visibility("hidden"))) int fr_popgs_block_stage(const fr_raster_cfg* cfg, const fr_gaussians* g, const fr_fisher_cfg* fc, void* workspace,
                                                               size_t workspace_bytes, int32_t* status, fr_stream_t stream);

// ---- argument checks and workspace layout of the entry points (host) ----------------------------------------------------------------
// workspace sections begin on 256 bytes
static inline size_t fr_align256(size_t x) { return (x + 255) & ~(size_t)255; }
// p on a multiple of a, a power of two (a null pointer is aligned)
static inline bool fr_aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
// do the byte ranges [a, a + na) and [b, b + nb) share a byte?  An empty range overlaps nothing.
static inline bool fr_overlap(const void* a, size_t na, const void* b, size_t nb)
{
	const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
	return na && nb && a0 < b0 + nb && b0 < a0 + na;
}
// an image the pixel kernels index with 32 bits: H, W positive and H W at most 2^30
static inline bool fr_image_ok(int32_t H, int32_t W) { return H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 30); }
#endif
