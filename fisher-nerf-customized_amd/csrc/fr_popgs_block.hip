// fr_popgs_block.hip -- the POp-GS block stage of libfisher_rast.so (gfx950, wave64).  No export: fr_fisher_views hands over to
// fr_popgs_block_stage when its fr_raster_cfg carries an extension (fr_raster_ext, include/fisher_rast.h, where the contract is).
//
// The reference scores a pose from per-Gaussian d x d blocks with one more render (radius > 0), an einsum, two isin, batched LAPACK
// on binary32 blocks and a host read, per pose (models/SLAM/gaussian_object.py:2111-2176, 1572-1585, 1660-1732).  Here:
//
//   k_pb_visible   one thread per (pose, Gaussian): the single-view rasteriser's projection (fr_cov3d, fr_preprocess_one) on the
//                  camera-frame mean, radius > 0 as a byte; the workgroup's count by ballot.
//   k_pb_scan      one workgroup per pose: exclusive scan of the workgroup counts (frb_scan_counts), the pose's total.
//   k_pb_scatter   k_pb_visible's geometry: the ordered compaction (frb_rank256) of a pose's visible indices -- PRIOR only.
//   k_pb_prior<D>  one thread per prior row: the keyframes' binary32 blocks at their r-th visible Gaussian, added in keyframe order.
//   k_pb_score<D>  a thread per (pose, prior row), rows in steps of the grid: the pair's term in binary64 (fr_popgs_block_math.h:
//                  Gram matrix, two unpivoted L D L^T in registers, the trace of the inverse or the log pivots), summed per thread,
//                  per workgroup (frb_sum256), one partial per workgroup.  Most pairs are not visible and leave at once.
//   k_pb_finish    one workgroup: a pose's partials in index order, -inf for a pose without a pair, the status word.
//
// D is a template parameter (seven instantiations): the triangles are registers, nothing spills.  No atomics; the partial sums have
// one order, which depends on n alone.  Workgroups never wait for each other.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "fr_internal.h"
#include "fr_block.h"
#include "fr_popgs_block_math.h"

#define FRPB_THREADS 256
static_assert(FRPB_THREADS == FRB_THREADS, "fr_block.h is written for 256 threads");

struct FrpbPartial { double sum; int32_t matched, bad, skipped, pad0; int64_t pad1; };
static_assert(sizeof(FrpbPartial) == 32, "FR_POPGS_BLOCK_WS_BYTES counts 32 bytes per partial");

struct FrpbGeom {
	const float* means; const float* scales; const float* rots; const float* w2c; const float* view; const float* proj;
	int P, K, W, H;
	float tanfovx, tanfovy, focal_x, focal_y, mod;
	uint32_t gx, gy;
	uint8_t* vis;            // [poses, P] workspace
	uint8_t* out_vis;        // [poses, P] or null
	uint32_t* counts;        // [poses, nwg]
	int nwg;
};

__device__ __forceinline__ bool frpb_visible(const FrpbGeom& a, int p, int i)
{
	const float* w = a.w2c + 16 * ((size_t)p * a.K);
	float wm[12], vm[16], pm[16];
#pragma unroll
	for (int k = 0; k < 12; k++) wm[k] = w[k];
#pragma unroll
	for (int k = 0; k < 16; k++) { vm[k] = a.view[k]; pm[k] = a.proj[k]; }
	const fr_f3 pw = { a.means[3 * (size_t)i], a.means[3 * (size_t)i + 1], a.means[3 * (size_t)i + 2] };
	const fr_f3 po = fr_world_to_cam(pw, wm);
	const fr_f3 pv = fr_xform4x3(po, vm);
	if (pv.z <= 0.001f) return false;          // the first test of fr_preprocess_one, before the covariance is built
	const fr_f3 sc = { a.scales[3 * (size_t)i], a.scales[3 * (size_t)i + 1], a.scales[3 * (size_t)i + 2] };
	const fr_f4 q = { a.rots[4 * (size_t)i], a.rots[4 * (size_t)i + 1], a.rots[4 * (size_t)i + 2], a.rots[4 * (size_t)i + 3] };
	float c3[6];
	fr_cov3d(sc, a.mod, q, c3);
	const fr_splat s = fr_preprocess_one(po, c3, vm, pm, a.W, a.H, a.tanfovx, a.tanfovy, a.focal_x, a.focal_y, a.gx, a.gy);
	return s.radius > 0;
}

__global__ __launch_bounds__(FRPB_THREADS) void k_pb_visible(FrpbGeom a)
{
	__shared__ uint32_t s_wave[4];
	const int p = blockIdx.y, i = blockIdx.x * FRPB_THREADS + threadIdx.x;
	const bool vis = i < a.P && frpb_visible(a, p, i);
	if (i < a.P)
	{
		a.vis[(size_t)p * a.P + i] = vis ? 1 : 0;
		if (a.out_vis) a.out_vis[(size_t)p * a.P + i] = vis ? 1 : 0;
	}
	const uint32_t c = frb_count256(vis, s_wave);
	if (threadIdx.x == 0) a.counts[(size_t)p * a.nwg + blockIdx.x] = c;
}

__global__ __launch_bounds__(FRPB_THREADS) void k_pb_scan(const uint32_t* __restrict__ counts, uint32_t* __restrict__ offsets, int nwg,
                                                          uint32_t* __restrict__ totals, int32_t* __restrict__ out_vis_count)
{
	__shared__ uint32_t s_wave[4];
	const int p = blockIdx.x;
	const uint32_t total = frb_scan_counts(counts + (size_t)p * nwg, offsets + (size_t)p * nwg, nwg, s_wave);
	if (threadIdx.x == 0)
	{
		totals[p] = total;
		if (out_vis_count) out_vis_count[p] = (int32_t)total;
	}
}

__global__ __launch_bounds__(FRPB_THREADS) void k_pb_scatter(const uint8_t* __restrict__ vis, const uint32_t* __restrict__ offsets, int P, int nwg,
                                                             int32_t* __restrict__ lists)
{
	__shared__ uint32_t s_wave[4];
	const int p = blockIdx.y, i = blockIdx.x * FRPB_THREADS + threadIdx.x;
	const bool sel = i < P && vis[(size_t)p * P + i] != 0;
	const uint32_t slot = offsets[(size_t)p * nwg + blockIdx.x] + frb_rank256(sel, s_wave);
	if (sel && slot < (uint32_t)P) lists[(size_t)p * P + slot] = i;          // always: at most P are visible
}

struct FrpbRows {
	const float* rows;       // [poses K, P, 11]
	long long view_stride;   // 11 P
	int P, K, poses, n;
	int use_opacity, use_rot, use_scale;
};

template <int D>
__global__ __launch_bounds__(FRPB_THREADS) void k_pb_prior(FrpbRows a, const uint32_t* __restrict__ totals, const int32_t* __restrict__ lists,
                                                           float* __restrict__ out_blocks, int32_t* __restrict__ out_idx, int32_t* __restrict__ status)
{
	uint32_t nmin = totals[0];
	for (int f = 1; f < a.poses; f++) nmin = totals[f] < nmin ? totals[f] : nmin;
	const long long r = (long long)blockIdx.x * FRPB_THREADS + threadIdx.x;
	if (r == 0) { status[0] = (int32_t)nmin; status[1] = 0; status[2] = 0; status[3] = 0; }
	if (r >= (long long)nmin || r >= (long long)a.n) return;
	int cols[D];
#pragma unroll
	for (int c = 0; c < D; c++) cols[c] = frpb_col(c, a.use_opacity, a.use_rot, a.use_scale);
	float acc[FRPB_TRI(D)];
#pragma unroll
	for (int e = 0; e < FRPB_TRI(D); e++) acc[e] = 0.0f;
	bool first = true;
	for (int f = 0; f < a.poses; f++)
	{
		const int32_t i = lists[(size_t)f * a.P + r];
		if ((uint32_t)i >= (uint32_t)a.P) continue;          // never with lists that k_pb_scatter wrote for these counts
		frpb_prior_add<D>(a.rows + (long long)f * a.K * a.view_stride + (long long)i * FRPB_ROW, a.view_stride, a.K, cols, first, acc);
		first = false;
	}
	float* out = out_blocks + r * (D * D);
#pragma unroll
	for (int i = 0; i < D; i++)
	{
#pragma unroll
		for (int j = 0; j <= i; j++) { out[i * D + j] = acc[i * (i + 1) / 2 + j]; out[j * D + i] = acc[i * (i + 1) / 2 + j]; }
	}
	out_idx[r] = lists[r];
}

// the sum of one int per thread over the workgroup, for every thread.  Two barriers.
__device__ __forceinline__ int frpb_isum256(int v, int* s_w)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
	if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
	__syncthreads();
	const int r = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
	__syncthreads();
	return r;
}

template <int D>
__global__ __launch_bounds__(FRPB_THREADS) void k_pb_score(FrpbRows a, const uint8_t* __restrict__ vis, const float* __restrict__ prior,
                                                           const int32_t* __restrict__ idx, double lam, int criterion, FrpbPartial* __restrict__ part)
{
	__shared__ double s_red[1][FRB_WAVES];
	__shared__ int s_w[4];
	const int p = blockIdx.y;
	int cols[D];
#pragma unroll
	for (int c = 0; c < D; c++) cols[c] = frpb_col(c, a.use_opacity, a.use_rot, a.use_scale);
	double sum[1] = { 0.0 };
	int matched = 0, bad = 0, skipped = 0;
	const float* rows = a.rows + (long long)p * a.K * a.view_stride;
	const uint8_t* v = vis + (size_t)p * a.P;
	for (long long r = (long long)blockIdx.x * FRPB_THREADS + threadIdx.x; r < a.n; r += (long long)gridDim.x * FRPB_THREADS)
	{
		const int32_t i = idx[r];
		if ((uint32_t)i >= (uint32_t)a.P) { skipped++; continue; }
		if (!v[i]) continue;
		sum[0] += frpb_pair_term<D>(rows + (long long)i * FRPB_ROW, a.view_stride, a.K, cols, prior + r * (D * D), lam, criterion, bad);
		matched++;
	}
	frb_sum256<1>(sum, s_red);
	matched = frpb_isum256(matched, s_w);
	bad = frpb_isum256(bad, s_w);
	skipped = frpb_isum256(skipped, s_w);
	if (threadIdx.x == 0)
	{
		FrpbPartial o;
		o.sum = frb_sum4(s_red[0]); o.matched = matched; o.bad = bad; o.skipped = skipped; o.pad0 = 0; o.pad1 = 0;
		part[(size_t)p * gridDim.x + blockIdx.x] = o;
	}
}

__global__ __launch_bounds__(FRPB_THREADS) void k_pb_finish(const FrpbPartial* __restrict__ part, int nwg, int poses, double* __restrict__ out_scores,
                                                            int32_t* __restrict__ out_matched, int32_t* __restrict__ status)
{
	__shared__ int s_w[4];
	int matched = 0, bad = 0, skipped = 0;
	for (int p = threadIdx.x; p < poses; p += FRPB_THREADS)
	{
		double s = 0.0;
		int m = 0;
		for (int w = 0; w < nwg; w++)
		{
			const FrpbPartial q = part[(size_t)p * nwg + w];
			s += q.sum; m += q.matched; bad += q.bad;
			if (p == 0) skipped += q.skipped;          // every pose walks the same prior rows
		}
		out_scores[p] = m ? s : -INFINITY;
		out_matched[p] = m;
		matched += m;
	}
	matched = frpb_isum256(matched, s_w);
	bad = frpb_isum256(bad, s_w);
	skipped = frpb_isum256(skipped, s_w);
	if (threadIdx.x == 0) { status[0] = matched; status[1] = 0; status[2] = bad; status[3] = skipped; }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------

struct FrpbLayout { size_t vis, lists, counts, offsets, totals, partials, total; int nwg; };

static FrpbLayout frpb_layout(int32_t P, int32_t poses)
{
	FrpbLayout l;
	const size_t pp = (size_t)poses * (size_t)P;
	l.nwg = (int)FR_POPGS_BLOCK_WGS(P);
	l.vis = 0;
	l.lists = l.vis + FR_POPGS_BLOCK_ALIGN(pp);
	l.counts = l.lists + FR_POPGS_BLOCK_ALIGN(pp * 4);
	l.offsets = l.counts + FR_POPGS_BLOCK_ALIGN((size_t)poses * l.nwg * 4);
	l.totals = l.offsets + FR_POPGS_BLOCK_ALIGN((size_t)poses * l.nwg * 4);
	l.partials = l.totals + FR_POPGS_BLOCK_ALIGN((size_t)poses * 4);
	l.total = l.partials + FR_POPGS_BLOCK_ALIGN((size_t)poses * FR_POPGS_BLOCK_MAX_WG * sizeof(FrpbPartial));
	return l;
}

#define FRPB_WHO "fr_fisher_views (POp-GS block stage): "

int fr_popgs_block_stage(const fr_raster_cfg* cfg, const fr_gaussians* g, const fr_fisher_cfg* fc, void* workspace, size_t workspace_bytes,
                         int32_t* status, fr_stream_t stream)
{
	const fr_raster_ext* x = cfg->ext;
	if (x->kind != FR_EXT_POPGS_BLOCK) return fr_fail(FR_EINVAL, FRPB_WHO "unknown extension kind (FR_EXT_POPGS_BLOCK is the only one)");
	if (!fc || !status) return fr_fail(FR_EINVAL, FRPB_WHO "null pointer (cfg_f, status)");
	const int mode = x->mode;
	if (mode != FR_POPGS_BLOCK_VISIBLE && mode != FR_POPGS_BLOCK_SCORE && mode != FR_POPGS_BLOCK_PRIOR)
		return fr_fail(FR_EINVAL, FRPB_WHO "bad argument (mode is FR_POPGS_BLOCK_VISIBLE, _SCORE or _PRIOR)");
	if (x->K < 1 || fc->n_views < 1 || fc->n_views % x->K) return fr_fail(FR_EINVAL, FRPB_WHO "bad argument (K at least 1, n_views a positive multiple of K)");
	const int P = cfg->P, K = x->K, poses = fc->n_views / K;
	if (P < 1) return fr_fail(FR_EINVAL, FRPB_WHO "bad argument (P is at least 1)");
	if (poses > 65535) return fr_fail(FR_EINVAL, FRPB_WHO "bad argument (at most 65535 poses a call)");
	if (fc->columns != FRPB_ROW) return fr_fail(FR_EINVAL, FRPB_WHO "columns must be 11");
	if (fc->dL_dpix != 0.0f || fc->H_inv || fc->H_inv_view_stride || fc->out_scores || fc->out_vis_count || fc->out_num_rendered || fc->dL_dpix_image ||
	    fc->dL_image_view_stride || fc->tile_capacity || fc->poses_are_c2w || fc->reuse_static || fc->order || fc->view_is_identity)
		return fr_fail(FR_EINVAL, FRPB_WHO "bad fisher cfg (only n_views, w2c, columns, out_H and out_H_view_stride are read: every other field must be zero or null)");
	if ((x->use_opacity | x->use_rot | x->use_scale) & ~1) return fr_fail(FR_EINVAL, FRPB_WHO "bad argument (use_opacity, use_rot, use_scale are 0 or 1)");
	if (g && g->cov3D_precomp) return fr_fail(FR_EINVAL, FRPB_WHO "cov3D_precomp is not supported");
	const bool need_rows = mode != FR_POPGS_BLOCK_VISIBLE;
	if (need_rows && !fc->out_H) return fr_fail(FR_EINVAL, FRPB_WHO "null pointer (out_H: the probe rows)");
	if (fc->out_H ? fc->out_H_view_stride != (int64_t)FRPB_ROW * P : (fc->out_H_view_stride != 0 && fc->out_H_view_stride != (int64_t)FRPB_ROW * P))
		return fr_fail(FR_EINVAL, FRPB_WHO "bad argument (out_H_view_stride is 11 P)");
	if (mode != FR_POPGS_BLOCK_SCORE && x->vis_in) return fr_fail(FR_EINVAL, FRPB_WHO "bad argument (vis_in is read by FR_POPGS_BLOCK_SCORE alone)");
	if (mode == FR_POPGS_BLOCK_VISIBLE && !x->out_vis && !x->out_vis_count) return fr_fail(FR_EINVAL, FRPB_WHO "nothing to compute (no out_vis and no out_vis_count)");
	if (need_rows)
	{
		if (x->n < 1) return fr_fail(FR_EINVAL, FRPB_WHO "bad argument (n is at least 1)");
		if (!x->prior_blocks || !x->prior_idx) return fr_fail(FR_EINVAL, FRPB_WHO "null pointer (prior_blocks, prior_idx)");
	}
	if (mode == FR_POPGS_BLOCK_SCORE)
	{
		if (x->criterion != FR_POPGS_TOPT && x->criterion != FR_POPGS_DOPT) return fr_fail(FR_EINVAL, FRPB_WHO "bad argument (criterion is FR_POPGS_TOPT or FR_POPGS_DOPT)");
		if (!(x->lam >= 0.0) || !(x->lam < INFINITY)) return fr_fail(FR_EINVAL, FRPB_WHO "bad argument (lam is finite and not negative)");
		if (!x->out_scores || !x->out_matched) return fr_fail(FR_EINVAL, FRPB_WHO "null pointer (out_scores, out_matched)");
		if (x->vis_in && (x->out_vis || x->out_vis_count)) return fr_fail(FR_EINVAL, FRPB_WHO "bad argument (out_vis / out_vis_count with vis_in: no visibility is computed)");
	}
	const bool geometry = !(mode == FR_POPGS_BLOCK_SCORE && x->vis_in);
	if (geometry)
	{
		if (!g || !g->means3D || !g->scales || !g->rotations) return fr_fail(FR_EINVAL, FRPB_WHO "null pointer (means3D, scales, rotations)");
		if (!fc->w2c || !cfg->viewmatrix || !cfg->projmatrix) return fr_fail(FR_EINVAL, FRPB_WHO "null pointer (w2c, viewmatrix, projmatrix)");
		if (!fr_image_ok(cfg->image_height, cfg->image_width) || !(cfg->tanfovx > 0.f) || !(cfg->tanfovy > 0.f))
			return fr_fail(FR_EINVAL, FRPB_WHO "bad argument (image size, tanfovx, tanfovy)");
	}
	const FrpbLayout l = frpb_layout(P, poses);
	if (!workspace || workspace_bytes < l.total) return fr_fail(FR_ENOSPACE, FRPB_WHO "workspace smaller than FR_POPGS_BLOCK_WS_BYTES(P, poses)");
	if (!fr_aligned(workspace, 8) || !fr_aligned(x->out_scores, 8)) return fr_fail(FR_EINVAL, FRPB_WHO "bad argument (workspace and out_scores must be 8-byte aligned)");

	hipStream_t s = (hipStream_t)stream;
	char* ws = (char*)workspace;
	const dim3 block(FRPB_THREADS);
	int rc;
	uint32_t* totals = (uint32_t*)(ws + l.totals);
	uint32_t* offsets = (uint32_t*)(ws + l.offsets);
	const uint8_t* vis = x->vis_in;
	if (geometry)
	{
		FrpbGeom a;
		a.means = g->means3D; a.scales = g->scales; a.rots = g->rotations; a.w2c = fc->w2c; a.view = cfg->viewmatrix; a.proj = cfg->projmatrix;
		a.P = P; a.K = K; a.W = cfg->image_width; a.H = cfg->image_height;
		a.tanfovx = cfg->tanfovx; a.tanfovy = cfg->tanfovy;
		a.focal_y = a.H / (2.0f * cfg->tanfovy);          // as fr_fill_params (rasterizer_impl.cu:222-223)
		a.focal_x = a.W / (2.0f * cfg->tanfovx);
		a.mod = cfg->scale_modifier;
		a.gx = (uint32_t)((a.W + 15) / 16); a.gy = (uint32_t)((a.H + 15) / 16);
		a.vis = (uint8_t*)(ws + l.vis); a.out_vis = x->out_vis;
		a.counts = (uint32_t*)(ws + l.counts); a.nwg = l.nwg;
		hipLaunchKernelGGL(k_pb_visible, dim3((unsigned)l.nwg, (unsigned)poses), block, 0, s, a);
		if ((rc = fr_check_launch("k_pb_visible"))) return rc;
		hipLaunchKernelGGL(k_pb_scan, dim3((unsigned)poses), block, 0, s, (const uint32_t*)a.counts, offsets, l.nwg, totals, x->out_vis_count);
		if ((rc = fr_check_launch("k_pb_scan"))) return rc;
		vis = a.vis;
	}
	if (mode == FR_POPGS_BLOCK_VISIBLE)
	{
		if (hipMemsetAsync(status, 0, 4 * sizeof(int32_t), s) != hipSuccess) return fr_fail(FR_ELAUNCH, FRPB_WHO "hipMemsetAsync failed");
		return FR_OK;
	}
	FrpbRows r;
	r.rows = fc->out_H; r.view_stride = (long long)fc->out_H_view_stride;
	r.P = P; r.K = K; r.poses = poses; r.n = x->n;
	r.use_opacity = x->use_opacity; r.use_rot = x->use_rot; r.use_scale = x->use_scale;
	const int d = frpb_dim(x->use_opacity, x->use_rot, x->use_scale);
	if (mode == FR_POPGS_BLOCK_PRIOR)
	{
		int32_t* lists = (int32_t*)(ws + l.lists);
		hipLaunchKernelGGL(k_pb_scatter, dim3((unsigned)l.nwg, (unsigned)poses), block, 0, s, vis, (const uint32_t*)offsets, P, l.nwg, lists);
		if ((rc = fr_check_launch("k_pb_scatter"))) return rc;
		const int rows_max = x->n < P ? x->n : P;
		const dim3 grid((unsigned)((rows_max + FRPB_THREADS - 1) / FRPB_THREADS));
		switch (d)
		{
#define FRPB_CASE(D) case D: hipLaunchKernelGGL(k_pb_prior<D>, grid, block, 0, s, r, (const uint32_t*)totals, (const int32_t*)lists, x->prior_blocks, x->prior_idx, status); break;
		FRPB_FOR_EACH_D(FRPB_CASE)
#undef FRPB_CASE
		default: return fr_fail(FR_EINVAL, FRPB_WHO "bad block size");
		}
		return fr_check_launch("k_pb_prior");
	}
	FrpbPartial* part = (FrpbPartial*)(ws + l.partials);
	const int64_t want = ((int64_t)x->n + FRPB_THREADS - 1) / FRPB_THREADS;
	const int nwg = (int)(want < FR_POPGS_BLOCK_MAX_WG ? want : FR_POPGS_BLOCK_MAX_WG);
	const dim3 grid((unsigned)nwg, (unsigned)poses);
	switch (d)
	{
#define FRPB_CASE(D) case D: hipLaunchKernelGGL(k_pb_score<D>, grid, block, 0, s, r, vis, (const float*)x->prior_blocks, (const int32_t*)x->prior_idx, x->lam, (int)x->criterion, part); break;
	FRPB_FOR_EACH_D(FRPB_CASE)
#undef FRPB_CASE
	default: return fr_fail(FR_EINVAL, FRPB_WHO "bad block size");
	}
	if ((rc = fr_check_launch("k_pb_score"))) return rc;
	hipLaunchKernelGGL(k_pb_finish, dim3(1), block, 0, s, (const FrpbPartial*)part, nwg, poses, x->out_scores, x->out_matched, status);
	return fr_check_launch("k_pb_finish");
}
