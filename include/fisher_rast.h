/*
 * fisher_rast.h -- C ABI of libfisher_rast.so (MI355X / gfx950).
 *
 * Drop-in boundary for ONE hot path of davidea97/Fisher-Nerf-customized: the differentiable
 * 3D-Gaussian-splat rasteriser with the FisherRF `grad_power` backward, the per-candidate-view
 * Fisher-information scorer built on it, and simple-knn's distCUDA2.
 *
 * Every entry point
 *   - takes plain device pointers and sizes (no torch types), plus an explicit HIP stream;
 *   - never allocates device memory, never synchronises the device, never throws.  The forward / scorer pipelines
 *     fork onto two internal side streams (sort tier, scorer records) and join back onto the caller's stream; those
 *     two streams and four timing-disabled events are created once per host thread and device, by fr_init() or
 *     lazily by the first call that needs them (fr_profile_enable(1) additionally records two events per launch);
 *   - returns 0 on success or an FR_E* code; fr_last_error() gives the message (thread-local).
 *
 * Reference interfaces replaced (paths relative to the reference tree,
 * RAST = thirdparty/diff-gaussian-rasterization-modified):
 *   fr_mark_visible      <- markVisible                    RAST/rasterize_points.cu:198-217,
 *                                                          RAST/cuda_rasterizer/rasterizer_impl.cu:141-153
 *   fr_forward           <- RasterizeGaussiansCUDA         RAST/rasterize_points.cu:35-115
 *                           -> Rasterizer::forward         RAST/cuda_rasterizer/rasterizer_impl.cu:198-339
 *   fr_backward          <- RasterizeGaussiansBackwardCUDA RAST/rasterize_points.cu:117-196
 *                           -> Rasterizer::backward        RAST/cuda_rasterizer/rasterizer_impl.cu:343-434
 *   fr_forward_features, fr_backward_pair <- the second Renderer call of get_loss, models/SLAM/gaussian.py:203-211
 *   fr_fisher_views      <- the Python loop GaussianSLAM.pose_eval / compute_H_train / compute_Hessian
 *                           models/SLAM/gaussian.py:1338-1375, 1503-1570 and
 *                           models/SLAM/gaussian_object.py:1541-1551, 1591-1617, 1940-2045
 *                           (V x [forward + backward(power=2) + cat + sum]) as one batched call
 *   fr_fisher_pose_views <- the pose_H of compute_Hessian(return_pose=True) that the path objective uses
 *                           (tester_gaussians_navigation.py:1689-1701; a placeholder eye(6) in the reference)
 *   fr_render_views      <- the render_at_pose(c2w) calls inside the candidate loops of pose_eval_popgs / pose_eval_popgs_blocks
 *                           (models/SLAM/gaussian_object.py:1640, 1668; the image dump of pose_eval, 1606-1607): render_at_pose
 *                           (models/SLAM/gaussian.py:555-579) for V poses -- V x [transform + two rasteriser forwards] as one batched call
 *   fr_fisher_point_views <- the candidate scan of GaussianSLAM.global_planning (models/SLAM/gaussian.py:1285-1325: pointScores per
 *                           candidate, the running max_points_score that prune_invisible reads) as one batched call
 *   fr_popgs_diag_criterion <- the T-opt / D-opt criterion and prior update inside path_evaluation_popgs
 *                           (tester_gaussians_navigation.py:2147-2178, models/SLAM/gaussian_object.py:1705-1719)
 *   fr_densify_stats / fr_densify_masks / fr_prune_mask <- the statistics of get_loss / densify / prune_gaussians
 *                           models/SLAM/gaussian.py:289-291, models/SLAM/utils/slam_external.py:196-200, 345-465
 *   fr_image_loss_forward / fr_image_loss_backward <- calc_loss / calc_loss_mask / calc_ssim / calc_ssim_masked,
 *                           models/SLAM/utils/slam_helpers.py:23-77, models/SLAM/utils/slam_external.py:77-193
 *   fr_frame_ingest_select / fr_frame_ingest_emit <- add_new_gaussians / get_pointcloud / initialize_new_params,
 *                           models/SLAM/gaussian.py:320-414, 75-143, 299-318
 *   fr_loss_mask / fr_bg_penalty_forward / fr_bg_penalty_backward / fr_outside_mask <- the pixel mask and the object lines of get_loss,
 *                           models/SLAM/gaussian.py:212-233, models/SLAM/gaussian_object.py:213-275, and get_gaussians_outside_mask,
 *                           models/SLAM/utils/slam_external.py:270-343
 *   fr_map_edit_plan / fr_map_edit_apply / fr_map_edit_split_children <- remove_points / cat_params_to_optimizer and the split
 *                           children of densify, models/SLAM/utils/slam_external.py:218-262, 411-463 over 25-42
 *   fr_adam_step         <- optimizer.step() of the torch.optim.Adam that get_optimizer builds (seven groups of one tensor),
 *                           models/SLAM/gaussian.py:1458-1469, models/SLAM/gaussian_object.py:1815-1826
 *   fr_keyframe_valid_pixels / fr_keyframe_overlap <- the device work of keyframe_selection_overlap / get_pointcloud,
 *                           models/SLAM/utils/keyframe_selection.py:40-134, 10-37
 *   fr_rendervar_forward / fr_rendervar_backward <- transform_to_frame, get_depth_and_silhouette, transformed_params2rendervar and
 *                           their autograd, models/SLAM/utils/slam_helpers.py:178-188, 235-252, 268-317 over slam_external.py:25-42
 *   fr_knn_dist2         <- simple_knn._C.distCUDA2 (thirdparty/simple-knn, un-vendored submodule)
 *   fr_cloud_index_build / fr_cloud_query <- the KD-tree searches of accuracy_comp_ratio_from_pcl, scripts/eval_3d_reconstruction.py:84-125,
 *                           and novelty_mask_from_pcd_nn, test_utils.py:503-578
 *
 * The pybind module `_C` of the reference (RAST/ext.cpp:14-18) is re-created in Python on top of
 * this ABI by fisher-nerf-customized_amd/diff_gaussian_rasterization/_C.py; see INTEGRATION.md.
 */
#ifndef FISHER_RAST_H_INCLUDED
#define FISHER_RAST_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FR_VERSION 100

enum {
	FR_OK = 0,
	FR_EINVAL = 1,      /* bad argument (null pointer, negative size, unsupported combination) */
	FR_ELAUNCH = 2,     /* HIP runtime error at launch; message has hipGetErrorString */
	FR_ENOSPACE = 3     /* workspace too small (host-visible sizes only) */
};

/* device-side status word written by the kernels (int32[4] = {num_rendered_total, overflow, max_tile_count, reserved}) */
#define FR_STATUS_WORDS 4

typedef void* fr_stream_t; /* hipStream_t */

/* Camera / raster settings: GaussianRasterizationSettings, RAST/diff_gaussian_rasterization/__init__.py:140-151.
 * bg / viewmatrix / projmatrix / campos stay DEVICE pointers, as in the reference (they are CUDA tensors there);
 * viewmatrix and projmatrix are the 16 floats of the transposed tensors, i.e. column-major matrices. */
struct fr_raster_ext;
typedef struct fr_raster_cfg {
	int32_t P;
	int32_t image_height;
	int32_t image_width;
	float tanfovx;
	float tanfovy;
	float scale_modifier;
	int32_t sh_degree;   /* D */
	int32_t sh_coeffs;   /* M = shs.size(1), 0 when colours are precomputed */
	int32_t prefiltered; /* auxiliary.h:156-160: with it set, a point culled by the near plane is an error -- the reference traps the
	                        device; fr_forward raises status[3] instead and the Python layer throws the reference's message */
	const float* bg;
	const float* viewmatrix;
	const float* projmatrix;
	const float* campos;
	const struct fr_raster_ext* ext; /* null: every entry point is what it was before this field existed, bit for bit.  Only
	                                    fr_fisher_views reads it (the POp-GS block stage, below its declaration); every other
	                                    entry point ignores the field */
} fr_raster_cfg;

/* Gaussian inputs; a null pointer stands for the reference's empty tensor. */
typedef struct fr_gaussians {
	const float* means3D;        /* [P,3] */
	const float* colors_precomp; /* [P,3] or null */
	const float* shs;            /* [P,M,3] or null */
	const float* opacities;      /* [P] (or [P,1]) */
	const float* scales;         /* [P,3] or null */
	const float* rotations;      /* [P,4] or null */
	const float* cov3D_precomp;  /* [P,6] or null */
} fr_gaussians;

int fr_version(void);
const char* fr_last_error(void);
/* Hash of the kernel / header sources this library was compiled from (stamped by __graft_entry__.build();
 * "unstamped" for a hand build).  The Python loader refuses a library whose id does not match the sources beside it. */
const char* fr_build_id(void);
/* Optional: creates the calling thread's side streams and events for the current device now instead of on first use. */
int fr_init(void);

/* ---- single-view rasteriser (the reference's _C.rasterize_gaussians / _backward / mark_visible) ---- */

/* Bytes of the three opaque work buffers (geomBuffer, binningBuffer, imgBuffer of the reference).
 * out[0] geometry (P), out[1] binning (max_rendered tile instances), out[2] image (W,H). */
int fr_workspace_bytes(int32_t P, int32_t W, int32_t H, int64_t max_rendered, size_t out[3]);

/* Byte offsets of the named sections inside the three buffers (for tests / debuggers).
 * geom:    [0] splat f32[P,8] = {mean2D.x, mean2D.y, conic.x, conic.y, conic.z, opacity, depth, pad} (valid where radii > 0),
 *          [1] cov3D f32[P,6], [2] rgb f32[P,3], [3] clamped u8[P,3]
 * image:   [4] tile_count u32[T], [5] tile_offset u32[T], [6] tile_fill u32[T], [7] final_T f32[HW],
 *          [8] n_contrib u32[HW], [9] status i32[4]
 * binning: [10] keys u64[R]  (sorted per tile: (depth_bits << 32) | gaussian_index) */
int fr_workspace_layout(int32_t P, int32_t W, int32_t H, int64_t max_rendered, size_t offsets[11]);

int fr_mark_visible(int32_t P, const float* means3D, const float* viewmatrix, const float* projmatrix,
                    uint8_t* present, fr_stream_t stream);

/* Forward.  binning_capacity = number of tile instances binning_ws can hold.  status (device int32[4]) receives
 * {num_rendered, overflow, longest tile list, prefiltered violated}; when num_rendered > binning_capacity nothing is rendered, overflow = 1 and the caller
 * re-runs with a larger buffer (the reference instead synchronises on num_rendered before sizing the buffer,
 * rasterizer_impl.cu:282-286).  out_color [3,H,W], out_depth [1,H,W], radii [P]. */
int fr_forward(const fr_raster_cfg* cfg, const fr_gaussians* g,
               void* geom_ws, void* binning_ws, int64_t binning_capacity, void* image_ws,
               float* out_color, float* out_depth, int32_t* radii, int32_t* status, fr_stream_t stream);

/* Backward.  All nine gradient buffers are overwritten (zero-filled first, rasterize_points.cu:151-159).
 * dL_dmeans2D [P,3], dL_dcolors [P,3], dL_dopacity [P,1], dL_dmeans3D [P,3], dL_dcov3D [P,6], dL_dsh [P,M,3]
 * (may be null when M == 0), dL_dscales [P,3], dL_drotations [P,4], dL_dconic [P,2,2].
 * power is the reference's `backward_power` (1 = gradients, 2 = squared per-pixel gradients). */
int fr_backward(const fr_raster_cfg* cfg, const fr_gaussians* g, const int32_t* radii,
                const void* geom_ws, const void* binning_ws, const void* image_ws,
                const float* dL_dout_color, int32_t power,
                float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D,
                float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations, float* dL_dconic,
                fr_stream_t stream);

/* fr_backward with a scratch buffer the power-2 backward may use: fr_backward_scratch_bytes(P, W, H, power, num_rendered) bytes,
 * num_rendered = what fr_forward reported for this image (status[0]); 0 = no use for one (other powers; more than 16384 tiles or 4 GiB).
 * (Power 1, the training backward, takes the same scratch and the same route for its nine per-candidate sums.)
 * fr_backward's power-2 pass is one workgroup per tile -- one 256 x 256 view is 256 workgroups on 256 CUs, the longest tile list sets
 * the time of the literal `backward_power=2` loop (models/SLAM/gaussian.py:1548-1549) -- and its per-candidate LDS accumulators
 * serialise under splats that cover a strip; given the scratch, the backward is cut into chunks of at most 64
 * candidates of one 16 x 4 pixel strip that run as independent pieces of work (a cheap pass leaves each chunk's effect on a pixel's
 * back-to-front state, a prefix pass the state in front of every chunk).  The same pairs contribute; a pixel's state at the start of a
 * chunk differs from the single pass's by rounding only (a few 1e-7 relative).  scratch == NULL or too small: fr_backward's single pass.
 * num_rendered below what the forward reported (a scratch laid out for too few tile instances): the kernels notice and leave every
 * gradient zero. */
size_t fr_backward_scratch_bytes(int32_t P, int32_t W, int32_t H, int32_t power, int64_t num_rendered);
int fr_backward_ws(const fr_raster_cfg* cfg, const fr_gaussians* g, const int32_t* radii,
                   const void* geom_ws, const void* binning_ws, const void* image_ws,
                   const float* dL_dout_color, int32_t power,
                   float* dL_dmeans2D, float* dL_dcolors, float* dL_dopacity, float* dL_dmeans3D,
                   float* dL_dcov3D, float* dL_dsh, float* dL_dscales, float* dL_drotations, float* dL_dconic,
                   int64_t num_rendered, void* scratch, size_t scratch_bytes, fr_stream_t stream);

/* ---- second feature image on the same geometry (training step) ------------------------
 * The reference's get_loss renders twice with identical means / scales / rotations / opacities / camera and different
 * colours: RGB, then (depth, 1, depth^2) for depth + silhouette (models/SLAM/gaussian.py:199-211,
 * slam_helpers.py:268-279) -- two full rasteriser forwards and two full backwards.
 * fr_forward_features composites another [P,3] feature array over what fr_forward just projected, binned and sorted
 * (same cfg and workspaces; no preprocess, no sort).  fr_backward_pair is the backward of both images in one call
 * (grad_power 1): one tile pass per image, the per-Gaussian Jacobian chain once.  dL_dmeans2D receives the colour image's
 * screen-space gradient only -- the statistic the densifier reads (gaussian.py:207) -- dL_dmeans2D_features the other
 * image's; every other output is the sum over both images, except dL_dcolors / dL_dfeatures. */
/* fr_forward with a second feature array composited in the same pass: out_features [3,H,W] */
int fr_forward_pair(const fr_raster_cfg* cfg, const fr_gaussians* g, const float* features,
                    void* geom_ws, void* binning_ws, int64_t binning_capacity, void* image_ws,
                    float* out_color, float* out_features, float* out_depth, int32_t* radii, int32_t* status,
                    fr_stream_t stream);
int fr_forward_features(const fr_raster_cfg* cfg, const float* features,
                        const void* geom_ws, const void* binning_ws, void* image_ws,
                        float* out_features, fr_stream_t stream);
int fr_backward_pair(const fr_raster_cfg* cfg, const fr_gaussians* g, const int32_t* radii,
                     const void* geom_ws, const void* binning_ws, const void* image_ws,
                     const float* dL_dout_color, const float* features, const float* dL_dout_features,
                     float* dL_dmeans2D, float* dL_dmeans2D_features, float* dL_dcolors, float* dL_dfeatures,
                     float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dscales,
                     float* dL_drotations, float* dL_dconic, fr_stream_t stream);

/* fr_backward_pair with the scratch buffer of the chunked form (fr_backward_ws, above; six colour channels in the per-chunk state):
 * fr_backward_pair_scratch_bytes(P, W, H, num_rendered) bytes, num_rendered = what the forward of this image reported. */
size_t fr_backward_pair_scratch_bytes(int32_t P, int32_t W, int32_t H, int64_t num_rendered);
int fr_backward_pair_ws(const fr_raster_cfg* cfg, const fr_gaussians* g, const int32_t* radii,
                        const void* geom_ws, const void* binning_ws, const void* image_ws,
                        const float* dL_dout_color, const float* features, const float* dL_dout_features,
                        float* dL_dmeans2D, float* dL_dmeans2D_features, float* dL_dcolors, float* dL_dfeatures,
                        float* dL_dopacity, float* dL_dmeans3D, float* dL_dcov3D, float* dL_dscales,
                        float* dL_drotations, float* dL_dconic,
                        int64_t num_rendered, void* scratch, size_t scratch_bytes, fr_stream_t stream);

/* ---- fused multi-view Fisher scorer -------------------------------------------------------------- */

typedef struct fr_fisher_cfg {
	int32_t n_views;
	int32_t columns;            /* 4 = [mean_cam xyz | opacity] (gaussian.py:1555-1556);
	                               11 = + [scale xyz | rot rxyz] (gaussian_object.py:2022-2027) */
	float dL_dpix;              /* constant upstream gradient of every pixel/channel (reference: 1e-3) */
	const float* w2c;           /* device [n_views,16], row-major 4x4 world->camera (rel_w2c) */
	const float* H_inv;         /* device [P,columns] weights, or null */
	int64_t H_inv_view_stride;  /* elements between consecutive views' H_inv blocks (0 = one block shared) */
	float* out_scores;          /* device [n_views]: sum(cur_H * H_inv) per view, or null */
	float* out_H;               /* device [.., P, columns], ACCUMULATED into (caller zero-fills), or null */
	int64_t out_H_view_stride;  /* elements between views' blocks in out_H (0 = all views sum into one block) */
	int32_t* out_vis_count;     /* device [n_views]: #Gaussians with radius > 0, or null */
	int32_t* out_num_rendered;  /* device [n_views]: tile instances per view, or null */
	const float* dL_dpix_image; /* device [n_views,3,H,W] or null: per view an upstream-gradient image instead of the constant
	                               dL_dpix -- the `im.backward(gradient=z)` probes of estimate_diag_JtJ_simple /
	                               estimate_block_JtJ (gaussian_object.py:2088-2098, 2158-2170).  out_H mode only. */
	int64_t dL_image_view_stride; /* elements between views' images (0 = one image shared by all views) */
	int32_t tile_capacity;      /* 0: the keys of all (view, tile) lists are packed into max_rendered slots (count, scan, scatter).
	                               > 0: every (view, tile) owns a fixed segment of tile_capacity keys, which the projection kernel
	                               fills itself -- no scan dependency and no scatter kernel; needs n_views * tiles * tile_capacity
	                               <= max_rendered (and < 2^32).  A tile with more instances than that: overflow, status[3] = 1. */
	int32_t poses_are_c2w;      /* 1: `w2c` holds camera-to-world poses; the library inverts them (one small kernel) */
	int32_t reuse_static;       /* 1: THIS workspace still holds the per-Gaussian static records the call would build -- the previous
	                               fr_fisher_views call on it (ordered before this one on the stream) had the same Gaussians, the same
	                               shared H_inv rows (or none / per-view ones), the same columns, order, n_views and max_rendered -- so
	                               the packing kernel is skipped.  A planner scores hundreds of pose batches against one map and one
	                               H_inv (tester_gaussians_navigation.py:1684-1705); the caller vouches for the sameness. */
	const uint32_t* order;      /* device [P] or null: a permutation of 0..P-1 -- the order in which the Gaussians are laid out and
	                               processed inside the call (fr_spatial_order: Morton order of the means).  Purely a layout
	                               hint: every input and output keeps the caller's indexing (H_inv rows, out_H rows), the contributor
	                               sets and their depth order are unchanged.  With a spatially coherent order a projection workgroup's
	                               256 Gaussians are neighbours in space: whole groups fall outside a view and are skipped by one bounding
	                               test, a workgroup's keys land in a handful of tiles, a tile's records sit side by side in memory.
	                               (Splats of EQUAL depth in one tile are ordered by their place in `order`; fr_spatial_order is stable
	                               -- equal means keep the caller's order -- so duplicated Gaussians composite as in the reference.)
	                               Ignored by the fall-back kernels (H_inv and out_H in one launch, images beyond 4096 tiles). */
	int32_t view_is_identity;   /* 1: the caller vouches that cfg->viewmatrix is the identity (the scorer's camera: gaussian.py:343), and
	                               the score-only front end with fixed key segments leaves the view products out (bit-identical
	                               projections).  The kernel checks the matrix: any other raises the overflow flag -- nothing is scored --
	                               and bit 1 of status[3] (value 2).  0: the general path. */
} fr_fisher_cfg;

/* Morton (Z-curve, 10 bits per axis over the bounding box of the means) order of P points: order_out[k] = index of the k-th point
 * along the curve; points with equal codes keep their index order (a stable sort).  The reference has no counterpart: it processes
 * the Gaussians in the order of the parameter tensors (models/SLAM/gaussian.py:1529-1543).  Once per map, not per call. */
size_t fr_spatial_order_workspace_bytes(int32_t P);
int fr_spatial_order(int32_t P, const float* means3D, uint32_t* order_out, void* workspace, size_t workspace_bytes, fr_stream_t stream);

size_t fr_fisher_workspace_bytes(int32_t P, int32_t W, int32_t H, int32_t n_views, int64_t max_rendered, int32_t columns);
/* Byte offsets of the named sections inside the scorer's workspace (for tests / debuggers):
 * [0] tile_count u32[V,T], [1] tile_offset u32[V,T], [2] keys u64[R] (sorted per (view, tile) from tile_offset on: (depth_bits << 32) |
 *     record slot with packed lists, (depth_bits << 32) | slot << 4 | strips of the tile reached with fixed segments -- tile_capacity),
 * [3] dense {recA, recB} records [V,P] x 32 B -- only the single-view front end (images beyond 4096 tiles) fills them; the default
 *     path leaves this section unused -- [4] the scorer's records: COMPACT [V][PV] records, PV = projection workgroups x their
 *     Gaussians (>= P), one per visible (view, Gaussian) at slot = workgroup * its Gaussians + rank among the workgroup's visible
 *     splats of the view: 80 B (score form with fixed key segments: {x, y, k3, log2 o} {-cx/2, -cy, -cz/2, r+g+b} + 12 polynomial
 *     coefficients), 96 B (score form with packed lists, A-form of the 4-column out_H kernel), 112 / 208 B (general out_H form, 4 / 11
 *     columns), 48 B (render form of fr_render_views); dense [V,P] x 64 B with the single-view front end,
 * [5] tile_scores f32[V,T], [6] status i32[4], [7] visible-list lengths u32[V, blocks] */
int fr_fisher_workspace_layout(int32_t P, int32_t W, int32_t H, int32_t n_views, int64_t max_rendered, int32_t columns,
                               size_t offsets[8]);
/* Byte offset of the PART LIST in the same workspace (fixed key segments; appended behind every section above): u32 [0] = number
 * of parts of the last call (of its first view group), [16 ..] pairs {key offset relative to section [2], count}: the ranges of
 * 2 .. 512 keys that the long lists (2049 .. tile_capacity / 2 - 64 keys) were cut into, each sorted by one wave; up to 64 per
 * (view, tile).  A view group after the first has its own {count, pad[15], pairs} at u32 index first_view * tiles * 128 + 16 * group. */
int fr_fisher_part_list_offset(int32_t P, int32_t W, int32_t H, int32_t n_views, int64_t max_rendered, int32_t columns, size_t* offset);

/* Scores n_views candidate poses in one batched launch sequence.  g->means3D are WORLD positions; each view's
 * camera-frame means are computed in-kernel from cfg_f->w2c and then rendered through cfg->viewmatrix/projmatrix
 * exactly as the reference does (gaussian.py:1523-1548; its camera has viewmatrix = I).
 * status (device int32[4]) receives {total tile instances, overflow, largest tile list, tile_capacity exceeded}; on overflow
 * (total > max_rendered, or a tile list longer than cfg_f->tile_capacity) no score is written and nothing is accumulated. */
int fr_fisher_views(const fr_raster_cfg* cfg, const fr_gaussians* g, const fr_fisher_cfg* cfg_f,
                    void* workspace, size_t workspace_bytes, int64_t max_rendered,
                    int32_t* status, fr_stream_t stream);

/* ---- camera-pose Fisher information of candidate views ---------------------------------------------
 * The reference's path objective adds path_pose_weight * log det(pose_H) per step (tester_gaussians_navigation.py:1689-1701,
 * 1925-1946); its compute_Hessian(return_pose=True) returns eye(6) there, a placeholder.  This is the quantity that name promises:
 * each view is rendered as fr_fisher_views renders it (camera-frame means m_i = rel_w2c x_i, viewmatrix = I; rotations, scales,
 * opacities and colours do not move with the pose), the pose is perturbed on the left, m_i(xi) = exp(xi^) m_i with xi = (rho, phi),
 * translation first, so dm_i/dxi = [I | -[m_i]x], and with g_{p,i} pixel p's share of dL/dm_i for the constant upstream gradient
 * dL_dpix on every channel (the mean2D and the cov2D-through-J(t) paths of the reference's backward, limx / limy clamp included)
 *     j_p = sum_i [ g_{p,i} ; m_i x g_{p,i} ]        pose_H = sum_p j_p j_p^T     (6 x 6, symmetric positive semi-definite)
 * Contributor sets and cut-offs are the forward's.  One front-to-back walk per (view, tile) writes plain per-tile partials, which are
 * summed in a fixed order in double: the same call gives bit-identical results, and a view's result does not depend on the batch.
 * fr_fisher_cfg fields used: n_views, dL_dpix, w2c, poses_are_c2w, out_vis_count, out_num_rendered, tile_capacity, order (columns is
 * ignored: the pose Fisher does not depend on it).  H_inv / out_scores, out_H, dL_dpix_image and reuse_static are rejected (FR_EINVAL),
 * and so are images beyond 4096 tiles; every check is made before any device work.
 * out_pose_H: device float [n_views, 6, 6], both triangles written.  status as fr_fisher_views; on overflow nothing is written. */
size_t fr_fisher_pose_workspace_bytes(int32_t P, int32_t W, int32_t H, int32_t n_views, int64_t max_rendered);
/* offsets [0..7] as fr_fisher_workspace_layout(.., columns = 4) (the records are the 112-byte pose form: the 4-column general out_H
 * record with the camera-frame mean in the place of the colour), [8] the per-tile partials f64 [n_views, tiles, 21] */
int fr_fisher_pose_workspace_layout(int32_t P, int32_t W, int32_t H, int32_t n_views, int64_t max_rendered, size_t offsets[9]);
int fr_fisher_pose_views(const fr_raster_cfg* cfg, const fr_gaussians* g, const fr_fisher_cfg* cfg_f, float* out_pose_H,
                         void* workspace, size_t workspace_bytes, int64_t max_rendered, int32_t* status, fr_stream_t stream);

/* ---- batched render of candidate views: RGB, depth / silhouette, median depth, final transmittance -------------------
 * View v is exactly what fr_forward / fr_forward_pair produce for means3D = m with the camera of cfg, where
 *     m_i = ((w0 x + w1 y) + w2 z) + w3   per row of w2c[v], in binary32 without fused multiply-add
 * and the second feature array is (m_i.z, 1, m_i.z * m_i.z): get_depth_and_silhouette with the identity first_frame_w2c
 * (models/SLAM/utils/slam_helpers.py:268-279).  Contributor rules forward.cu:338-366; out = C + T * bg on all six channels.
 * Bit for bit: the front end writes one 48-byte record per visible (view, Gaussian) -- {x, y, ext, opacity} {conic.x, conic.y,
 * conic.z, depth} {r, g, b, m.z}, the single-view rasteriser's values (`ext`, the conservative half extents, only culls) -- and the
 * tile kernel composites from them with the single-view kernel's pair arithmetic.  A view's images do not depend on the batch.
 *   out_color    [V,3,H,W]                              or null
 *   out_features [V,3,H,W] composited (z, 1, z*z)       or null
 *   out_depth    [V,1,H,W] median depth (default 15.0)  or null
 *   out_final_T  [V,H,W]                                or null      (at least one of the four)
 * fr_fisher_cfg fields used: n_views, w2c, poses_are_c2w, out_vis_count (Gaussians with radius > 0), out_num_rendered (the
 * reference's rectangle count), tile_capacity, order.  H_inv / out_scores, out_H, dL_dpix_image, reuse_static, SH colours
 * (colors_precomp is required), cov3D_precomp, four null outputs and images beyond 4096 tiles are rejected (FR_EINVAL); every
 * check is made before any device work.  status as fr_fisher_views; on overflow nothing is written (no output byte changes).
 * No device allocation, no host synchronisation, no atomics on the images.
 * fr_render_views_workspace_bytes is a host-only query (0 for a bad argument or an image beyond 4096 tiles); the layout's offsets
 * [0..7] are those of fr_fisher_workspace_layout(.., columns = 4), [4] holding the compact [V][PV] x 48 B render records. */
size_t fr_render_views_workspace_bytes(int32_t P, int32_t W, int32_t H, int32_t n_views, int64_t max_rendered);
int fr_render_views_workspace_layout(int32_t P, int32_t W, int32_t H, int32_t n_views, int64_t max_rendered, size_t offsets[8]);
int fr_render_views(const fr_raster_cfg* cfg, const fr_gaussians* g, const fr_fisher_cfg* cfg_f,
                    float* out_color, float* out_features, float* out_depth, float* out_final_T,
                    void* workspace, size_t workspace_bytes, int64_t max_rendered, int32_t* status, fr_stream_t stream);

/* ---- per-Gaussian view scores and their running maximum ---------------------------------------------------------------
 * The candidate scan of GaussianSLAM.global_planning (models/SLAM/gaussian.py:1285-1325, the same loop in gaussian_object.py) asks
 * "which Gaussians does view v inform, and by how much?": pointScores = sum(cur_H * H_train_inv, dim=1) per candidate, a running
 * max_points_score over the candidates, prune_invisible on that maximum.  With cur_H[v] what fr_fisher_views accumulates into a
 * per-view out_H (the dL_dpix^2 factor included):
 *     point[v, i] = sum_c cur_H[v, i, c] * H_inv[(v,) i, c]
 * One number per (view, Gaussian): the tile kernel keeps ONE accumulator per candidate whatever `columns` is (the pair's contracted
 * factor comes from the score records of fr_fisher_views), and no [V, P, columns] tensor exists anywhere.
 *   out_point_scores [V, P] or null: every element is written; a Gaussian that contributes nothing in view v gets 0.0
 *   out_point_max    [P] or null:    out_point_max[i] <- max(out_point_max[i], max_v point[v, i]).  The CALLER initialises it (the
 *                    reference starts from zeros) with non-negative values, so calls over chunks of views compose, and ranks through
 *                    all_reduce(MAX).  The maximum is taken on the bit patterns (unsigned atomic max): exact, independent of the order;
 *                    with both outputs given, out_point_max == max(initial, max over v of out_point_scores) of the same call bit for bit.
 *   at least one of the two.
 * fr_fisher_cfg fields used: n_views, columns (4 or 11), dL_dpix, w2c, poses_are_c2w, H_inv (required), H_inv_view_stride (0 = one
 * block shared, else one per view), out_scores (optional: the view's score sum_i point[v, i], summed from per-tile partials in a fixed
 * order in double -- the same bits from call to call, and independent of the batch), out_vis_count, out_num_rendered, tile_capacity,
 * order.  out_H, dL_dpix_image, reuse_static, a null H_inv, two null outputs and images beyond 4096 tiles are rejected (FR_EINVAL);
 * every check is made before any device work.
 * point[v, i] itself is a sum of global float atomics, one per (16 x 4 pixel strip, Gaussian): their arrival order is not fixed, so two
 * calls may differ in its last bits.  out_scores and the max identity above do not depend on that order.
 * status as fr_fisher_views; on overflow no output byte changes.  No device allocation, no host synchronisation.
 * fr_fisher_point_workspace_bytes is a host-only query (0 for a bad argument or an image beyond 4096 tiles); the layout's offsets
 * [0..7] are those of fr_fisher_workspace_layout, [8] the per-slot accumulators f32 [n_views, PV] (PV as there). */
size_t fr_fisher_point_workspace_bytes(int32_t P, int32_t W, int32_t H, int32_t n_views, int64_t max_rendered, int32_t columns);
int fr_fisher_point_workspace_layout(int32_t P, int32_t W, int32_t H, int32_t n_views, int64_t max_rendered, int32_t columns,
                                     size_t offsets[9]);
int fr_fisher_point_views(const fr_raster_cfg* cfg, const fr_gaussians* g, const fr_fisher_cfg* cfg_f,
                          float* out_point_scores, float* out_point_max,
                          void* workspace, size_t workspace_bytes, int64_t max_rendered, int32_t* status, fr_stream_t stream);

/* ---- POp-GS diagonal criteria over probe rows ("T-opt/D-opt variants") ---------------------
 * The reference scores a pose from the diagonal estimator with a chain of torch ops over [11 P] vectors and, along a path, folds
 * the estimate into the path's prior (models/SLAM/gaussian_object.py:1705-1719, tester_gaussians_navigation.py:2147-2178).
 * One call does that for V views in one streaming pass.  Per entry e of view v
 *     J      = (sum_k rows[v,k,e]^2) / K                                      fp32
 *     prior  = prior_in[v,e] + lam ;  post = prior + J
 *     T-opt:  scores[v] = - sum_e 1 / max(post, 1e-12)
 *     D-opt:  scores[v] =   sum_e [ log max(post, 1e-12) - log max(prior, 1e-12) ]
 * Every term is formed in fp32 without cancellation -- the D-opt term is log1p(J / prior) where nothing is clamped and exactly 0
 * where J == 0, never the difference of two rounded logarithms -- and the terms are added in fp64: per thread, per wave, one partial per
 * workgroup into `workspace`, then a view's partials in index order.  No atomics: the same call gives the same bits, and a view's
 * score does not depend on the other views of the batch (the workgroups per view depend on E alone).
 *   rows        [V, K, E] the probe rows as fr_fisher_views wrote them (out_H per view under dL_dpix_image), E = P * columns entries
 *               per view.  The criteria are sums over all entries, so any layout will do that prior and rows share.
 *   prior_in    [E] with prior_in_view_stride = 0 (every view against the same prior: the first round of a path evaluation), or
 *               [V, E] with prior_in_view_stride = E
 *   prior_out   [V, E] or null; accumulate [V] bytes or null (= no view accumulates).  Where accumulate[v] != 0,
 *               prior_out[v,e] = prior_in[v,e] + J (fp32; the reference's H_train_path + cur_diag, lam not included); the other views'
 *               blocks are not touched.  prior_out may BE prior_in (same pointer, stride E); any other overlap is rejected.
 *   vis_count   [V] or null: a view with vis_count[v] == 0 scores exactly 0.0 (tester 2162-2163); its prior still accumulates
 *   scores      [V] fp64
 *   workspace   fr_popgs_diag_criterion_workspace_bytes(V, E) bytes (host-only query; 0 for a bad argument), 8-byte aligned
 * 16-byte loads and stores when E % 4 == 0 and the pointers are 16-byte aligned, dword ones otherwise; the result is the same. */
enum { FR_POPGS_TOPT = 0, FR_POPGS_DOPT = 1 };
#define FR_POPGS_CLAMP 1e-12f
size_t fr_popgs_diag_criterion_workspace_bytes(int32_t V, int64_t E);
int fr_popgs_diag_criterion(int32_t V, int32_t K, int64_t E, const float* rows, const float* prior_in, int64_t prior_in_view_stride,
                            float* prior_out, const uint8_t* accumulate, const int32_t* vis_count, float lam, int32_t criterion,
                            double* scores, void* workspace, size_t workspace_bytes, fr_stream_t stream);

/* ---- POp-GS block criteria over probe rows: an extension of fr_raster_cfg, no export of its own -------------------------
 * The reference scores a pose from the block estimator per pose: one more render for `radius > 0`, an einsum to [Nv,d,d], two isin,
 * batched LAPACK on binary32 blocks of condition ~ |J| / lam, one float read back (models/SLAM/gaussian_object.py:2111-2176, 1572-1585,
 * 1660-1732).  With cfg->ext set, fr_fisher_views IS A DIFFERENT CALL THAT RENDERS NOTHING: the block stage over probe rows the caller
 * already has (what fr_fisher_views wrote into out_H per view under dL_dpix_image).  It branches before any other validation.
 *
 * What the stage reads from the ordinary arguments:
 *   cfg        P (at least 1), image size, tanfovx / tanfovy, scale_modifier, viewmatrix, projmatrix (the last six only where a
 *              visibility is computed), ext
 *   g          means3D, scales, rotations where a visibility is computed (else g may be null); a non-null cov3D_precomp: FR_EINVAL
 *   cfg_f      n_views = poses * K; w2c [n_views,16] -- pose p is read from view p K (the caller repeats it per probe); columns = 11;
 *              out_H = the rows [n_views, P, 11], an INPUT here; out_H_view_stride = 11 P.  Every other field zero / null, else FR_EINVAL
 *   workspace  FR_POPGS_BLOCK_WS_BYTES(P, poses) bytes, 8-byte aligned (smaller: FR_ENOSPACE)
 *   max_rendered  ignored
 *   status     device int32[4] = {PRIOR: n; SCORE: pairs matched over all poses; VISIBLE: 0,
 *                                 0,
 *                                 SCORE: factorisations that met a non-positive pivot (A1 of a pair; A0 too under D-opt),
 *                                 SCORE: prior rows skipped for an index outside [0, P)}
 * d = 3 + use_opacity + 4 use_rot + 3 use_scale; a block's columns are the row's columns [0,1,2 | 3 | 7..10 | 4..6] (mean, opacity,
 * rot, scale: the reference's order), those present.
 *
 * FR_POPGS_BLOCK_VISIBLE  out_vis[p,i] = 1 where Gaussian i has radius > 0 in pose p, else 0; out_vis_count[p] = their number (what
 *     out_vis_count of a rendering call reports).  Camera-frame mean ((w0 x + w1 y) + w2 z) + w3 per row of the pose, unfused, then the
 *     single-view rasteriser's own projection: the mask is its `radii > 0`, bit for bit.  The rows may be null.
 * FR_POPGS_BLOCK_SCORE    visibility from vis_in where given (no geometry is read), else computed as above (and written to out_vis /
 *     out_vis_count where given).  For pose p and prior row r with i = prior_idx[r] visible in p, all in binary64:
 *         G_k = the d selected columns of row (p K + k, i);  J = (sum_k G_k G_k^T) / K, k ascending
 *         A0 = lower triangle of prior_blocks[r] + lam I;  A1 = A0 + J;  both factorised as an unpivoted L D L^T with pivots pi
 *         T-opt term: - trace(A1^-1), from the factor;  D-opt term: sum log|pi(A1)| - sum log|pi(A0)|  (exactly 0.0 when every G_k is
 *         zero: the two factorisations are then the same operations).  A non-positive pivot is counted, the value still formed from |pi|.
 *     out_scores[p] = the sum over r in a fixed order: per thread (r ascending in steps of the grid), the workgroup's 256 threads, one
 *     partial per workgroup, a pose's partials in index order; the workgroups per pose depend on n alone.  No atomics: the same call
 *     gives the same bits, and a pose's score does not depend on its batch.  out_matched[p] = the pairs; a pose with none scores -inf.
 *     prior_idx need not be sorted; an index outside [0, P) skips the row (never dereferenced) and is counted.
 * FR_POPGS_BLOCK_PRIOR    compute_H_train_blocks, the reference's truncation kept (gaussian_object.py:1577-1584): views are keyframes x K.
 *     Each keyframe's visible Gaussians are listed ascending; n = the smallest count; prior_idx[r] = the first keyframe's r-th visible
 *     index; prior_blocks[r] = sum over the keyframes, in order, of that keyframe's block at ITS r-th visible Gaussian (by position, not
 *     by index), a block = binary32 (sum_k g_a g_b) / K as fma(g_a, g_b, b) from 0 with k ascending -- the chain of the reference's einsum --,
 *     all d x d entries written.  ext->n is the capacity of
 *     the two outputs: rows r < min(n, ext->n) are written; status[0] = n is the call's one host read.
 * No device allocation, no host synchronisation.  poses at most 65535. */
enum { FR_EXT_POPGS_BLOCK = 1 };
enum { FR_POPGS_BLOCK_VISIBLE = 0, FR_POPGS_BLOCK_SCORE = 1, FR_POPGS_BLOCK_PRIOR = 2 };
#define FR_POPGS_BLOCK_MAX_WG 256      /* workgroups (partials) per pose of the SCORE pass: min(this, ceil(n / 256)) */
#define FR_POPGS_BLOCK_ALIGN(x) ((((size_t)(x)) + 255) & ~(size_t)255)
#define FR_POPGS_BLOCK_WGS(P) ((((size_t)(P)) + 255) / 256)
/* sections, each on 256 bytes: visibility u8[poses,P], visible lists i32[poses,P], counts and offsets u32[poses, ceil(P/256)] each,
 * list lengths u32[poses], partials 32 B x [poses, FR_POPGS_BLOCK_MAX_WG] */
#define FR_POPGS_BLOCK_WS_BYTES(P, poses) \
	(FR_POPGS_BLOCK_ALIGN((size_t)(poses) * (size_t)(P)) + FR_POPGS_BLOCK_ALIGN((size_t)(poses) * (size_t)(P) * 4) + \
	 2 * FR_POPGS_BLOCK_ALIGN((size_t)(poses) * FR_POPGS_BLOCK_WGS(P) * 4) + FR_POPGS_BLOCK_ALIGN((size_t)(poses) * 4) + \
	 FR_POPGS_BLOCK_ALIGN((size_t)(poses) * FR_POPGS_BLOCK_MAX_WG * 32))
typedef struct fr_raster_ext {
	int32_t kind;                 /* FR_EXT_POPGS_BLOCK; anything else: FR_EINVAL */
	int32_t mode;                 /* FR_POPGS_BLOCK_VISIBLE / _SCORE / _PRIOR */
	int32_t K;                    /* probes per pose */
	int32_t use_opacity, use_rot, use_scale;   /* 0 or 1 each */
	int32_t criterion;            /* SCORE: FR_POPGS_TOPT / FR_POPGS_DOPT */
	int32_t n;                    /* SCORE: prior rows; PRIOR: capacity of prior_blocks / prior_idx in rows */
	double lam;                   /* SCORE */
	const uint8_t* vis_in;        /* SCORE: device [poses,P] bytes or null */
	uint8_t* out_vis;             /* device [poses,P] bytes or null (VISIBLE: this or out_vis_count) */
	int32_t* out_vis_count;       /* device [poses] or null */
	float* prior_blocks;          /* device [n,d,d] binary32: SCORE reads it, PRIOR writes it */
	int32_t* prior_idx;           /* device [n]: SCORE reads it, PRIOR writes it */
	double* out_scores;           /* SCORE: device [poses] binary64 */
	int32_t* out_matched;         /* SCORE: device [poses] */
} fr_raster_ext;

/* ---- densification / pruning statistics of the training step ---------------------------
 * One pass over the Gaussians each, in place of the torch-op chains of models/SLAM/gaussian.py:289-291 and
 * models/SLAM/utils/slam_external.py:196-200, 345-465.  All arrays are device float32 [P] unless noted. */

/* After a render (+ backward): seen[i] = radii[i] > 0 (uint8, may be null); where seen: max_2D_radius = max(radius, max_2D_radius)
 * (may be null) and -- when grad_means2D ([P,3], the colour render's means2D.grad) is given -- means2D_gradient_accum += |grad.xy|,
 * denom += 1 (accumulate_mean2d_gradient). */
int fr_densify_stats(int32_t P, const int32_t* radii, const float* grad_means2D, float* max_2D_radius,
                     float* means2D_gradient_accum, float* denom, uint8_t* seen, fr_stream_t stream);

/* densify(): grads = accum / denom with NaN -> 0; to_clone = grads >= grad_thresh AND max_k exp(log_scales) <= clone_max_scale;
 * to_split = max_k exp(log_scales) > split_min_scale (the reference applies no gradient test to the split).
 * log_scales: [P, scale_cols], scale_cols 1 (isotropic) or 3.  Masks: uint8 [P]. */
int fr_densify_masks(int32_t P, const float* means2D_gradient_accum, const float* denom, const float* log_scales,
                     int32_t scale_cols, float grad_thresh, float clone_max_scale, float split_min_scale,
                     uint8_t* to_clone, uint8_t* to_split, fr_stream_t stream);

/* prune_gaussians() / the removal pass of densify(): to_remove = sigmoid(logit_opacities) < opacity_thresh
 * OR (big_thresh >= 0 AND max_k exp(log_scales) > big_thresh).  uint8 [P]. */
int fr_prune_mask(int32_t P, const float* logit_opacities, const float* log_scales, int32_t scale_cols,
                  float opacity_thresh, float big_thresh, uint8_t* to_remove, fr_stream_t stream);

/* ---- fused image loss of the training step: L1 + SSIM, forward and backward ------------------------------------------
 * In place of calc_loss / calc_loss_mask / calc_ssim / calc_ssim_masked (models/SLAM/utils/slam_helpers.py:23-77,
 * slam_external.py:77-193): per term two launches forward and one backward, no host synchronisation, no atomics (the same call
 * gives the same bits).  The 11 x 11 window (gaussian(11, 1.5); no other size) is applied as its two 11-tap passes, zero padded.
 *   loss = w_l1 * (sum |img - gt| / denominator) + w_ssim * (1 - sum ssim_map / normaliser)       (a term whose weight is 0 is left out)
 *   denominator: 1 (FR_LOSS_L1_SUM), C H W (FR_LOSS_L1_MEAN) or the number of mask bytes set (FR_LOSS_L1_MASKED_MEAN; an empty mask
 *                gives NaN, as torch's mean of nothing does);   normaliser: C H W
 * mask: device bytes (0 / 1), [C,H,W] (mask_channels = C) or [1,H,W] shared by the channels (mask_channels = 1), or null
 * (mask_channels = 0).  It selects the pixels of the L1 sum, and both images are multiplied by it before the SSIM (calc_loss_mask).
 * With mask_weights_ssim_map = 1 it does neither: it weights the SSIM map instead, and the normaliser is max(bytes set, C) -- for a
 * [1,H,W] mask the mean over the channels, weighted by the mask with clamp_min(1) on its count (calc_ssim_masked).
 * w_ssim == 0 is the L1-only form (depth term, tracking terms): no SSIM pass, and the SSIM outputs must be null. */
enum { FR_LOSS_L1_SUM = 0, FR_LOSS_L1_MEAN = 1, FR_LOSS_L1_MASKED_MEAN = 2 };
typedef struct {
	int32_t C, H, W;
	float w_l1, w_ssim;
	int32_t l1_denom;                 /* FR_LOSS_L1_* */
	int32_t mask_channels;            /* 0 (no mask), 1 or C */
	int32_t mask_weights_ssim_map;    /* 0 / 1, see above */
} fr_image_loss_cfg;

/* Host-only query (0 for a bad argument): the fp64 per-workgroup partials and their per-channel sums. */
size_t fr_image_loss_workspace_bytes(int32_t C, int32_t H, int32_t W);
/* out4 = {loss, L1 term (sum / denominator), SSIM mean, mask bytes set (C H W without a mask)}; out_channel_ssim [C] (or null):
 * the channels' SSIM means; out_ssim_map [C,H,W] (or null): the per-pixel map.  saved: (w_ssim != 0 ? 3 C H W : 0) + 4 floats that
 * fr_image_loss_backward reads -- the three partial maps of the SSIM term w.r.t. the window moments of img (mean, E[x x], E[x y], taken about 0.5) and the two factors w_l1 / denominator,
 * w_ssim / normaliser.  workspace: fr_image_loss_workspace_bytes, 8-byte aligned. */
int fr_image_loss_forward(const fr_image_loss_cfg* cfg, const float* img, const float* gt, const uint8_t* mask,
                          float* out4, float* out_channel_ssim, float* out_ssim_map, float* saved,
                          void* workspace, size_t workspace_bytes, fr_stream_t stream);
/* dL_dimg [C,H,W] = upstream[0] * d loss / d img, every element written once; exactly 0 where the mask is 0 (also under an empty
 * mask).  upstream: DEVICE float (autograd's 0-dim gradient), read by the kernel.  cfg, img, gt, mask, saved as in the forward. */
int fr_image_loss_backward(const fr_image_loss_cfg* cfg, const float* img, const float* gt, const uint8_t* mask,
                           const float* saved, const float* upstream, float* dL_dimg, fr_stream_t stream);

/* ---- frame ingest: new Gaussians from an RGB-D frame ------------------------------------------------------------------
 * In place of add_new_gaussians / get_pointcloud / initialize_new_params (models/SLAM/gaussian.py:320-414, 75-143, 299-318): which
 * cells of the H/d x W/d grid of a frame become Gaussians, as an ascending index list, and their parameter rows.  Two calls, since
 * the row count has to reach the host once to size the new tensors; no other host read, no atomics on floats (the same call
 * gives the same bits), nothing allocated inside.
 *   FR_INGEST_NONPRESENCE: a pixel is selected when the map does not explain it --
 *       err = |gt - render| * (gt > 0);  np = (sil < sil_thres) | ((render > gt) & (err > depth_error_ratio * median(err)));
 *       np &= mask_in (where one is given: the obj_mask_2d of models/SLAM/gaussian_object.py:447-460);  np &= gt > 0.01
 *     with the exact lower median of the H W errors (element (n - 1) / 2 of the sorted values; NaN as soon as one error is NaN,
 *     which switches the depth term off everywhere), found by a radix select.
 *   FR_INGEST_MASK: the caller's bytes [H,W] (non-zero = selected).
 * A cell is selected when any pixel of its d x d block is (max_pool2d); depth and colour of its row are those of the block's
 * TOP-LEFT pixel (x, y) = (gx d, gy d), as in the reference, so a selected block whose top-left depth is 0 gives a point at the
 * camera centre with log scale -inf.  downsample must divide H and W (FR_EINVAL otherwise: the reference's own shapes disagree then).
 * intrinsics ([3,3]) and w2c ([4,4]) are DEVICE float32, row-major, read by the kernels. */
enum { FR_INGEST_NONPRESENCE = 0, FR_INGEST_MASK = 1 };
#define FR_INGEST_STATUS_WORDS 5
#define FR_INGEST_WS_INDEX_OFFSET 8192   /* byte offset of the int32 index list in the workspace; the pooled mask, one byte per cell, follows it at + 4 (H/d)(W/d) */
typedef struct {
	int32_t H, W, downsample;
	int32_t mode;                     /* FR_INGEST_*  (select) */
	float sil_thres;                  /* select, FR_INGEST_NONPRESENCE */
	float depth_error_ratio;          /* select, FR_INGEST_NONPRESENCE: densify_dict["depth_error_ratio"] */
	int32_t transform_pts;            /* emit: 1 = world points through the inverse of w2c, 0 = camera-frame points */
	int32_t scale_cols;               /* emit: columns of log_scales, 1 (isotropic) or 3 */
	int32_t means_stride;             /* emit: floats between rows of means3D (3; 6 writes into an [N,6] xyz+rgb cloud) */
	int32_t colors_stride;            /* emit: the same for rgb_colors */
	const float* intrinsics;          /* emit: device [3,3] */
} fr_frame_ingest_cfg;

/* Host-only query (0 for a bad argument, a downsample that does not divide H and W included). */
size_t fr_frame_ingest_workspace_bytes(int32_t H, int32_t W, int32_t downsample);
/* depth_sil: [3,H,W], channel 0 the rendered depth, channel 1 the silhouette; gt_depth: [1,H,W] (both FR_INGEST_NONPRESENCE only);
 * mask_in: bytes [H,W] -- the mask itself in FR_INGEST_MASK; in FR_INGEST_NONPRESENCE optional (null: none), ANDed into the predicate.  status: FR_INGEST_STATUS_WORDS device int32 = {count, median is NaN, 0, 0, the
 * median's bits (0x7fc00000 when NaN; 0 in FR_INGEST_MASK)}.  The index list (count ascending row-major cell indices) is left in
 * the workspace (fr_frame_ingest_workspace_bytes, 8-byte aligned) for the emit call. */
int fr_frame_ingest_select(const fr_frame_ingest_cfg* cfg, const float* depth_sil, const float* gt_depth, const uint8_t* mask_in,
                           int32_t* status, void* workspace, size_t workspace_bytes, fr_stream_t stream);
/* One row per selected cell, written to rows [row_offset, row_offset + count) of every destination that is not null: means3D
 * [*,3] the back-projected point ((m0 X + m1 Y) + m2 Z) + m3 per row of c2w = the affine inverse of w2c; rgb_colors [*,3] the
 * pixel's colour, bits copied; unnorm_rotations [*,4] = (1,0,0,0); logit_opacities [*,1] = 0; log_scales [*,scale_cols] =
 * log(sqrt(mean3_sq_dist)); mean3_sq_dist [*] = (d z / ((fx + fy) / 2))^2.  color: [3,H,W]; count: status[0] as the host read it.
 * workspace null with count == (H/d)(W/d): every cell (mask=None), no select call needed.  count == 0 launches and writes nothing. */
int fr_frame_ingest_emit(const fr_frame_ingest_cfg* cfg, const float* color, const float* gt_depth, const float* w2c,
                         const void* workspace, int32_t count, int64_t row_offset,
                         float* means3D, float* rgb_colors, float* unnorm_rotations, float* logit_opacities,
                         float* log_scales, float* mean3_sq_dist, fr_stream_t stream);

/* ---- object-aware training step: loss pixel mask, background penalties, outside mask -----------------------------------
 * In place of the stretch between the render and the loss terms of get_loss (models/SLAM/gaussian.py:212-233 and, with the object
 * lines, models/SLAM/gaussian_object.py:213-275) and of get_gaussians_outside_mask (models/SLAM/utils/slam_external.py:270-343).
 * Nothing is read back to the host and nothing is allocated inside; integer sums and fp64 sums in a fixed order only (the same
 * call gives the same bits).  Object masks are device bytes [H,W], non-zero = object.
 *
 * fr_loss_mask -- the pixels that enter the loss, exactly the reference's:
 *       keep = gt > 0
 *       reject_outliers:  err = |gt - d| * (gt > 0);  keep &= err < outlier_ratio * median(err)      (strict; the product in binary32)
 *       keep &= !isnan(d) & !isnan(d2 - d * d)                                                      (two roundings: inf - inf is NaN)
 *       need_presence:    keep &= sil > sil_thres                                                   (strict, binary32)
 *       obj_mask:         keep &= obj != 0
 *   with the exact lower median of the H W errors (element (n - 1) / 2 of the sorted values; NaN as soon as one error is NaN,
 *   torch.median's rule), found by a radix select: four histogram launches in front of the mask launch.  Without reject_outliers
 *   the call is one launch and takes no workspace. */
#define FR_LOSS_MASK_STATUS_WORDS 5
typedef struct {
	int32_t H, W;
	float sil_thres;                  /* read with need_presence */
	int32_t reject_outliers;          /* 0 / 1: ignore_outlier_depth_loss */
	float outlier_ratio;              /* read with reject_outliers: the reference's 10 */
	int32_t need_presence;            /* 0 / 1: tracking and use_sil_for_loss */
} fr_loss_mask_cfg;

/* Host-only query (0 for a bad argument): the histograms of the radix select. */
size_t fr_loss_mask_workspace_bytes(int32_t H, int32_t W);
/* depth_sil: [3,H,W] rendered depth, silhouette, depth^2; gt_depth: [1,H,W]; obj_mask: bytes [H,W] or null (none).  mask: bytes
 * [H,W], 0 or 1, every element written once (a torch bool view of it costs nothing).  status: FR_LOSS_MASK_STATUS_WORDS device
 * int32 = {pixels kept, median is NaN, background pixels (obj_mask == 0; 0 without one), 0, the median's bits (0x7fc00000 when
 * NaN; 0 without reject_outliers)}.  workspace (fr_loss_mask_workspace_bytes, 8-byte aligned): with reject_outliers only, may be
 * null otherwise. */
int fr_loss_mask(const fr_loss_mask_cfg* cfg, const float* depth_sil, const float* gt_depth, const uint8_t* obj_mask,
                 uint8_t* mask, int32_t* status, void* workspace, size_t workspace_bytes, fr_stream_t stream);

/* fr_bg_penalty_forward / _backward -- the two background penalties of gaussian_object.py:263-275.  With bg = (obj_mask == 0) and
 * n = count(bg):   L_rgb = sum_{c,p} (|im| * bg) / max(3 n, 1),   L_alpha = sum_p (clamp(sil, 0, 1) * bg) / max(n, 1),
 * the products in binary32 as the reference takes them (a non-finite im anywhere makes L_rgb NaN, a NaN silhouette L_alpha; an
 * infinite one clamps to 1), the sums in fp64: per-workgroup partials added in a fixed order, as fr_image_loss_forward does.
 * im: [3,H,W]; depth_sil: [3,H,W], channel 1 is read.  Two launches forward, one backward. */
size_t fr_bg_penalty_workspace_bytes(int32_t H, int32_t W);
/* out4 = {fl(lambda_rgb L_rgb) + fl(lambda_alpha L_alpha), L_rgb, L_alpha, n}; saved2: the two denominators, which
 * fr_bg_penalty_backward reads.  workspace: fr_bg_penalty_workspace_bytes, 8-byte aligned. */
int fr_bg_penalty_forward(int32_t H, int32_t W, float lambda_rgb, float lambda_alpha, const float* im, const float* depth_sil,
                          const uint8_t* obj_mask, float* out4, float* saved2, void* workspace, size_t workspace_bytes,
                          fr_stream_t stream);
/* dL_dim [3,H,W] = fl(fl(up lambda_rgb) / max(3 n, 1)) * bg * sign(im), sign(+-0) = sign(NaN) = 0; dL_ddepth_sil [3,H,W]: channel 1 =
 * fl(fl(up lambda_alpha) / max(n, 1)) * bg where 0 <= sil <= 1 (both ends included; 0 elsewhere and at NaN), channels 0 and 2 exact
 * zeros.  These are torch autograd's own values, bit for bit; every element is written once.  upstream: DEVICE float (autograd's
 * 0-dim gradient), read by the kernel. */
int fr_bg_penalty_backward(int32_t H, int32_t W, float lambda_rgb, float lambda_alpha, const float* im, const float* depth_sil,
                           const uint8_t* obj_mask, const float* saved2, const float* upstream, float* dL_dim,
                           float* dL_ddepth_sil, fr_stream_t stream);

/* fr_outside_mask -- which Gaussians do not project into the object mask (slam_external.py:290-315).  Per Gaussian: the camera
 * point ((r0 x + r1 y) + r2 z) + t per row of w2c, the homogeneous pixel (k_i0 X + k_i1 Y) + k_i2 Z, u = p0 / max(p2, 1e-6), v
 * likewise; in_img = Z > 0 & 0 <= u < W & 0 <= v < H; the pixel looked up is (clamp(rint(u), 0, W - 1), clamp(rint(v), 0, H - 1)),
 * round half to even; outside = !(in_img & obj_mask[iv, iu]).  means3D: [P,3]; log_scales: [P,scale_cols], 1 or 3; w2c ([4,4]) and
 * intrinsics ([3,3]): DEVICE float32, row-major.  outside: bytes [P], 0 or 1.  status: FR_OUTSIDE_STATUS_WORDS device int32 =
 * {in_count, out_count, the bits of min and of max over the inside Gaussians of max_k exp(log_scales), the same two over the outside
 * ones}; a range over an empty set or over a set that holds a NaN scale is NaN (0x7fc00000).  Minima and maxima are taken on integer
 * keys of the log scales and exp of the four extremes alone, through binary64.  Two launches; P = 0 is fine (one). */
#define FR_OUTSIDE_STATUS_WORDS 6
size_t fr_outside_mask_workspace_bytes(int32_t P);
int fr_outside_mask(int32_t P, int32_t scale_cols, const float* means3D, const float* log_scales, const float* w2c,
                    const float* intrinsics, const uint8_t* obj_mask, int32_t H, int32_t W, uint8_t* outside, int32_t* status,
                    void* workspace, size_t workspace_bytes, fr_stream_t stream);

/* ---- map edit: a prune or densify mask applied to the map, its Adam state and its statistics --------------------------
 * In place of remove_points / cat_params_to_optimizer and the clone / split of densify (models/SLAM/utils/slam_external.py:218-262,
 * 411-463): a row's destination depends on the masks alone, so one ordered compaction of the masks (plan) and one gather over a
 * table of arrays (apply) do the work of the reference's boolean indexings and cats, with one host read of the three counts between
 * them to size the new tensors.  Nothing is allocated inside; integer sums only (the same call gives the same lists). */
enum { FR_EDIT_COPY = 0, FR_EDIT_ZERO = 1 };
#define FR_EDIT_STATUS_WORDS 4
#define FR_EDIT_MAX_ARRAYS 32
#define FR_EDIT_MAX_COLS 16
/* the ascending int32 list k (0 kept rows, 1 cloned rows, 2 split rows) begins at byte k * FR_EDIT_WS_LIST_STRIDE(P) of the workspace */
#define FR_EDIT_WS_LIST_STRIDE(P) ((((size_t)(P)) * 4 + 15) & ~(size_t)15)
typedef struct {
	const void* src;                  /* device [P, cols] 4-byte words */
	void* dst;                        /* device [n_keep + n_clone + n_into n_split, cols]; overlaps no source and no other destination */
	int32_t cols;                     /* 1 .. FR_EDIT_MAX_COLS */
	int32_t appended;                 /* FR_EDIT_COPY: clones and children carry their source row (parameters);
	                                     FR_EDIT_ZERO: the appended rows are zero (Adam moments, timestep) */
} fr_map_edit_array;

/* Host-only query (0 for a negative P). */
size_t fr_map_edit_workspace_bytes(int32_t P);
/* keep, clone, split: byte masks over the P source rows (non-zero = selected); any may be null -- a null keep keeps every row, a
 * null clone / split selects none.  Leaves the three ascending index lists in the workspace (fr_map_edit_workspace_bytes, 8-byte
 * aligned; FR_ENOSPACE when short) and status = {n_keep, n_clone, n_split, 0} (FR_EDIT_STATUS_WORDS device int32).  Three launches:
 * count, a one-workgroup scan, scatter.  P == 0 launches nothing and writes zeros to status. */
int fr_map_edit_plan(int32_t P, const uint8_t* keep, const uint8_t* clone, const uint8_t* split, int32_t* status,
                     void* workspace, size_t workspace_bytes, fr_stream_t stream);
/* One launch for the whole table (HOST array of n_arrays <= FR_EDIT_MAX_ARRAYS entries, passed in the kernel arguments).  Rows are
 * copied as bits.  The destination's rows are: the kept rows in ascending source order; the clones in ascending source order; the
 * children copy-major (every split row for copy 0, then for copy 1, ... n_into copies) -- the order of
 * cat((v[keep], v[to_clone], v[to_split].repeat(n_into, 1))).  n_keep, n_clone, n_split: the status as the host read it; the
 * workspace is the one the plan call wrote for this P.  FR_EINVAL for src == dst, a destination that overlaps a source or another
 * destination, cols outside 1 .. FR_EDIT_MAX_COLS or more than FR_EDIT_MAX_ARRAYS arrays.  A destination of zero rows launches nothing. */
int fr_map_edit_apply(const fr_map_edit_array* table, int32_t n_arrays, int32_t P, int32_t n_keep, int32_t n_clone, int32_t n_split,
                      int32_t n_into, const void* workspace, fr_stream_t stream);
/* The split children of densify, in place on the n_into n_split child rows of the destination (pointers already offset to the first
 * child): reads each child's copied unnorm_rotations [*,4] and log_scales [*,scale_cols] (1 or 3) and its normal sample z [*,3], and
 * writes means += R (z exp(log_scales)), log_scales = log(exp(log_scales) / (0.8 n_into)) -- csrc/fr_mapedit_math.h. */
int fr_map_edit_split_children(int32_t n_split, int32_t n_into, int32_t scale_cols, const float* z, float* means,
                               const float* unnorm_rotations, float* log_scales, fr_stream_t stream);

/* ---- fused Adam step: one launch over a table of parameter arrays ------------------------------------------------------
 * In place of optimizer.step() of the reference's torch.optim.Adam (amsgrad, maximize and weight decay off): per element, in binary32
 * and in this operand order (csrc/fr_adam_math.h; no contraction, IEEE divide and sqrt, so a g++ build of that header gives the same bits)
 *   m' = |w1| < 0.5 ? m + w1 (g - m) : g - (g - m)(1 - w1);   v' = v beta2 + (c2 g) g;   p' = p + neg_step_size (m' / (sqrt(v') / bc2_sqrt + eps))
 * The caller computes the coefficients as torch/optim/adam.py does, in doubles, and rounds each once: w1 = 1 - beta1, c2 = 1 - beta2,
 * bc2_sqrt = (1 - beta2^t)^0.5, neg_step_size = -lr / (1 - beta1^t).  lr == 0 goes through the same arithmetic. */
#define FR_ADAM_MAX_ARRAYS 16
typedef struct {
	float* param; const float* grad; float* exp_avg; float* exp_avg_sq;   /* device, n floats each, 4-byte aligned */
	int64_t n;
	float w1, beta2, c2, bc2_sqrt, eps, neg_step_size;
	int32_t fresh;    /* 1: first step of this array -- exp_avg / exp_avg_sq are NOT read (taken as zero), only written */
} fr_adam_array;
/* One launch for the whole table (HOST array of n_arrays <= FR_ADAM_MAX_ARRAYS entries, passed in the kernel arguments); no
 * workspace, no atomics, no host read.  An array whose four pointers are 16-byte aligned moves as 16-byte words, any other as 4-byte
 * words.  Nothing is launched when every n is 0.  FR_EINVAL for a null pointer with n > 0, n < 0, fresh outside 0 / 1, n_arrays outside
 * 0 .. FR_ADAM_MAX_ARRAYS, or a param, exp_avg or exp_avg_sq range that overlaps any other range of the table (gradients, which are
 * only read, may share memory with each other). */
int fr_adam_step(const fr_adam_array* table, int32_t n_arrays, fr_stream_t stream);

/* ---- fused render-variable build: frame transform and activations ---------------------------------------------------------
 * Everything between `params` and the rasteriser of a tracking / mapping iteration, one launch forward and one backward (two with a
 * camera gradient), in binary32 and in the operand order of csrc/fr_rendervar_math.h:
 *   q = normalize(normalize(cq)),  R = build_rotation(q),  pts = R m + ct,  zc = w2c[2,:3] . pts + w2c[2,3],  feats = (zc, 1, zc^2),
 *   rotations = q_g / max(|q_g|, 1e-12),  opacities = 1 / (1 + exp(-logit)),  scales = exp(log_scales) (one column broadcast to three)
 * All pointers are device pointers, 4-byte aligned (rows of 12 bytes: nothing more is assumed).  The camera arrays are the
 * reference's [1,4,T] / [1,3,T] tensors themselves: element c of frame time_idx is base[c * n_frames + time_idx].
 * Every output and every incoming gradient is nullable: a null output is a part that is not computed, a null incoming gradient is
 * not read and counts as zero (an output gradient that depends on it alone is then written as zeros). */
typedef struct {
	int32_t P, scale_cols;                 /* scale_cols: 1 (isotropic, broadcast to three) or 3 */
	int32_t time_idx, n_frames;
	const float* cam_unnorm_rots;          /* [4, n_frames] */
	const float* cam_trans;                /* [3, n_frames] */
	const float* first_frame_w2c;          /* [4,4] row-major; needed for feats / g_feats only */
	const float* means3D;                  /* [P,3] */
	const float* unnorm_rotations;         /* [P,4] */
	const float* logit_opacities;          /* [P,1] */
	const float* log_scales;               /* [P,scale_cols] */
	/* forward outputs */
	float* pts;                            /* [P,3] */
	float* feats;                          /* [P,3] */
	float* rotations;                      /* [P,4] */
	float* opacities;                      /* [P,1] */
	float* scales;                         /* [P,3] */
	float* rel_w2c;                        /* [4,4] row-major: the frame's pose as a matrix */
	/* backward: incoming gradients of the five outputs */
	const float* g_pts; const float* g_feats; const float* g_rotations; const float* g_opacities; const float* g_scales;
	/* backward outputs */
	float* g_means3D;                      /* [P,3] */
	float* g_unnorm_rotations;             /* [P,4] */
	float* g_logit_opacities;              /* [P,1] */
	float* g_log_scales;                   /* [P,scale_cols] */
	float* g_cam_unnorm_rots;              /* [4, n_frames]: written whole, zero outside time_idx */
	float* g_cam_trans;                    /* [3, n_frames]: written whole, zero outside time_idx */
} fr_rendervar_cfg;
/* bytes of the backward's workspace when a camera gradient is asked for: one row of twelve partial sums per workgroup */
size_t fr_rendervar_workspace_bytes(int32_t P);
/* One launch.  Reads the inputs an asked-for output needs (FR_EINVAL when one of them is null), writes the non-null outputs. */
int fr_rendervar_forward(const fr_rendervar_cfg* cfg, fr_stream_t stream);
/* One launch for the non-null per-Gaussian gradients; with g_cam_unnorm_rots or g_cam_trans set, the same launch leaves one row of
 * partial sums per workgroup in the workspace (plain stores, no atomics) and a second, one-workgroup launch adds the rows in a fixed
 * order and runs the pose's way back: the same bits on every call.  The workspace is the caller's (needed only with a camera
 * gradient); nothing is allocated, read back or synchronised.  P == 0 launches nothing: the camera gradients are set to zero.
 * FR_EINVAL for P < 0, scale_cols not 1 or 3, time_idx outside [0, n_frames), a null input that an asked-for gradient needs; FR_ENOSPACE for a workspace
 * that is too small. */
int fr_rendervar_backward(const fr_rendervar_cfg* cfg, void* workspace, size_t workspace_bytes, fr_stream_t stream);

/* ---- keyframe overlap: which keyframes see the current frame -----------------------------------------------------------
 * In place of the device work of keyframe_selection_overlap / get_pointcloud (models/SLAM/utils/keyframe_selection.py:10-37, 40-134):
 * the list of pixels with a measured depth, then -- for n of them the caller drew -- their world points, which of those the
 * reference's duplicate filter keeps, and how many of the kept ones each of K keyframes sees.  Two calls, with the one host read of
 * the pixel count between them (the draw needs it); arithmetic in csrc/fr_keyframe_math.h.  Nothing allocated, no host read inside,
 * integer sums only (the same call gives the same numbers whatever the launch geometry).
 *   key(c)  = |nearbyint(c * 1e4) / 1e4| per coordinate;  a point is INVALID when its three keys equal those of any other drawn
 *             point or (0,0,0): both copies of a pixel drawn twice go, and so do mirror images (x,y,z) / (-x,y,z) -- the reference's
 *             unique() / isin() filter, kept as it is.
 *   inside  = (u < W - edge) & (u > edge) & (v < H - edge) & (v > edge) & (z > 0), with (u, v) = p2.xy / z, z = p2.z + 1e-5,
 *             p2 = K (est_w2c p), and, where a keyframe has a mask, mask[clamp(nearbyint(v))][clamp(nearbyint(u))] != 0. */
#define FR_KEYFRAME_STATUS_WORDS 4
#define FR_KEYFRAME_MAX_POINTS 4096      /* the most points one overlap call takes (the reference draws 1600) */
typedef struct {
	int32_t H, W;                     /* the frame; H W at most 2^30 */
	int32_t n;                        /* drawn points, 1 .. FR_KEYFRAME_MAX_POINTS */
	int32_t K;                        /* keyframes, 0 or more */
	int32_t edge;                     /* margin in pixels, 0 or more (the reference uses 20) */
	int32_t n_valid_idx;              /* entries of valid_idx (the first call's count as the host read it); ignored without valid_idx */
	const float* intrinsics;          /* device [3,3] row-major */
	const float* w2c;                 /* device [4,4] row-major: the current frame */
} fr_keyframe_cfg;

/* Host-only queries (0 for a bad argument). */
size_t fr_keyframe_valid_pixels_workspace_bytes(int32_t H, int32_t W);
size_t fr_keyframe_overlap_workspace_bytes(int32_t n);
/* idx_out [H W] int32: the ascending flat indices of depth > 0 (& mask != 0 where mask, bytes [H,W], is not null) -- the row-major
 * order torch.where gives; status: FR_KEYFRAME_STATUS_WORDS device int32 = {count, 0, 0, 0}.  Three launches: per-workgroup counts by
 * ballot / popcount, a one-workgroup scan, a scatter; workgroups never wait for each other.  workspace: 8-byte aligned; FR_EINVAL
 * when it is short, as for a null pointer, a bad size or a misaligned depth / idx_out / status. */
int fr_keyframe_valid_pixels(int32_t H, int32_t W, const float* depth, const uint8_t* mask, int32_t* idx_out, int32_t* status,
                             void* workspace, size_t workspace_bytes, fr_stream_t stream);
/* Point i is the back-projection of pixel valid_idx[draws[i]] (valid_idx null: of pixel draws[i]) of depth [H,W] through the inverse
 * of cfg->w2c.  draws: int64 [n].  kf_w2c: [K,16] row-major est_w2c of the keyframes.  kf_mask_table: device uint64 [K] of addresses of
 * byte masks [H,W] (0: that keyframe has none), or null: no keyframe has one.  out_counts [K] int32: valid & inside points per
 * keyframe.  out_valid [n] bytes and out_pts [n,3] (every drawn point, kept or not; zeros for an out-of-range draw) may be null.
 * status = {valid points, out-of-range draws, 0, 0}: a draw outside [0, n_valid_idx) (or [0, H W) without valid_idx) or a valid_idx
 * entry outside [0, H W) makes its point invalid and is counted; nothing is read through it.  K == 0 writes status, out_valid and
 * out_pts only.  FR_EINVAL for a null required pointer, sizes outside the limits above, a float pointer not 4-byte or an int64 /
 * table pointer not 8-byte aligned, and a short workspace (fr_keyframe_overlap_workspace_bytes, 8-byte aligned). */
int fr_keyframe_overlap(const fr_keyframe_cfg* cfg, const float* depth, const int32_t* valid_idx, const int64_t* draws,
                        const float* kf_w2c, const uint64_t* kf_mask_table, int32_t* out_counts, uint8_t* out_valid, float* out_pts,
                        int32_t* status, void* workspace, size_t workspace_bytes, fr_stream_t stream);

/* ---- simple-knn ---------------------------------------------------------------------------------- */

size_t fr_knn_workspace_bytes(int32_t P);
/* out[i] = mean of the squared distances from points[i] to its 3 nearest other points. */
int fr_knn_dist2(int32_t P, const float* points, float* out, void* workspace, size_t workspace_bytes,
                 fr_stream_t stream);

/* ---- nearest point of another cloud: reconstruction metrics and the novelty mask -----------------------------------------
 * "Distance from each point of cloud A to the nearest point of cloud B", which the reference takes from a KD-tree it rebuilds on
 * every call: accuracy_comp_ratio_from_pcl (scripts/eval_3d_reconstruction.py:84-125) and novelty_mask_from_pcd_nn
 * (test_utils.py:503-578).  Here the index over B is built once, is the caller's memory and outlives the call; any number of
 * queries run against it.  Arithmetic in csrc/fr_cloud_math.h: exact search, binary32, one rounding per written operation --
 *   d2 = (dx*dx + dy*dy) + dz*dz with dx = q.x - t.x,   d = sqrtf(d2);
 * out_dist[i] is the minimum of that expression over all finite targets, bit for bit, and out_idx[i] the LOWEST original target
 * index that attains it.  A target with a non-finite coordinate is never the nearest and does not widen the index's frame.  A query
 * with a non-finite coordinate (in depth mode: a pixel without a depth, or whose point is not finite) gets +inf / -1 / flag 0, is
 * left out of the sums and is counted.  N = 0 or no finite target: every distance +inf, every index -1.
 * Nothing is allocated, nothing is read back, no environment variable is read; every launch is on `stream` (capturable).
 * Limits: N, M and H W at most FR_CLOUD_MAX_POINTS. */
#define FR_CLOUD_MAX_POINTS (1 << 27)
#define FR_CLOUD_STATS_WORDS 4           /* 8-byte words: {sum of distances (binary64), valid queries, flagged, skipped}, the last three uint64 */
#define FR_CLOUD_SOURCE_POINTS 0
#define FR_CLOUD_SOURCE_DEPTH 1
typedef struct {
	int32_t source;                   /* FR_CLOUD_SOURCE_POINTS: queries [M,3];  FR_CLOUD_SOURCE_DEPTH: the pixels of a depth image */
	int32_t M;                        /* "points": number of queries, 0 or more.  "depth": ignored, M = Hs Ws */
	int32_t H, W, stride;             /* "depth": the image and the sample grid u = 0, stride, ... < W, v likewise: Hs = ceil(H / stride), Ws = ceil(W / stride) */
	int32_t flip_z;                   /* "depth": negate the camera z (a camera that looks along -Z) */
	float dist_th;                    /* flag = d < dist_th in "points" mode, d > dist_th (novel; 0 at a skipped pixel) in "depth" mode; both strict */
	const float* queries;             /* device [M,3] */
	const float* depth;               /* device [H,W]; a pixel is valid when its depth is finite and > 0 */
	const float* kinv;                /* device [9] row-major: point = c2w (kinv (u, v, 1) d, 1) */
	const float* c2w;                 /* device [12] row-major: the top three rows of the camera-to-world matrix */
	float* out_dist;                  /* [M] or null */
	int32_t* out_idx;                 /* [M] or null */
	uint8_t* out_flag;                /* [M] bytes or null */
	void* out_stats;                  /* FR_CLOUD_STATS_WORDS 8-byte words or null; the same call gives the same bytes: per-256-query binary64
	                                     partials in caller order, added in one fixed order (frc_sum_block), integer counts, no float atomics */
	/* Optional, for a running evaluation that folds one frame after another into the search; all zero or null is the call above, bit for bit. */
	float* seed_d2;                   /* "points": [M] in and out, or null.  A FOLD: query m starts from best = seed_d2[m], a SQUARED distance
	                                     (d2 above), and the smaller of the seed and the minimum over the finite targets is written back;
	                                     out_dist[m] = sqrtf of it, out_flag and the statistics are taken from it -- what a search against the
	                                     union of everything folded so far would give, exactly (a minimum over a union is the minimum of the
	                                     minima).  A query with a non-finite coordinate leaves its seed untouched and is counted as skipped.
	                                     Seeds are +inf or values an earlier fold wrote; they are NOT inspected.  out_idx must be null (the
	                                     union is gone); FR_EINVAL otherwise, in "depth" mode, or when not 4-byte aligned */
	const uint8_t* mask;              /* "depth": device [H,W] bytes or null.  A pixel is a query only where its byte is not 0 AND its depth is
	                                     valid; a masked-out pixel is a pixel without a depth in every respect.  FR_EINVAL in "points" mode */
	int32_t flag_near;                /* "depth": non-zero makes out_flag and `flagged` d < dist_th (strict) instead of d > dist_th */
	float* out_points;                /* "depth": [Hs Ws, 3] or null: the point of every sample in sample order, three NaNs where the sample is
	                                     no query -- fr_cloud_index_build sorts such rows last and ignores them, so this is a target cloud
	                                     as it stands.  4-byte aligned; FR_EINVAL when not, or in "points" mode */
} fr_cloud_query_cfg;

/* Host-only queries, non-decreasing in their argument (0 for an argument outside the limits). */
size_t fr_cloud_index_bytes(int32_t N);
size_t fr_cloud_index_workspace_bytes(int32_t N);
size_t fr_cloud_query_workspace_bytes(int32_t M);
/* The index over points [N,3]: Morton keys of the finite targets in their own bounding box, the 64-bit key sort, the sorted
 * coordinates and original indices, AABBs of 64-point sub-boxes, 1024-point boxes and super-boxes of 16 boxes.  The workspace is scratch of the build only.
 * FR_EINVAL for N outside the limits, a null pointer (points may be null when N = 0), points not 4-byte or index / workspace not
 * 8-byte aligned, a short index or workspace. */
int fr_cloud_index_build(int32_t N, const float* points, void* index, size_t index_bytes, void* workspace, size_t workspace_bytes,
                         fr_stream_t stream);
/* Any subset of the outputs of cfg against an index built over N points.  M = 0 writes the statistics only (zeros).
 * FR_EINVAL for a null index, cfg or workspace, a null source pointer, an unknown source, non-positive H / W / stride, sizes outside the
 * limits, a misaligned pointer (index, workspace, out_stats 8 bytes; floats and out_idx 4), a short index or workspace
 * (fr_cloud_query_workspace_bytes(M), in depth mode of Hs Ws; the optional fields need no more), an optional field with the wrong
 * source or misaligned (see the struct). */
int fr_cloud_query(const void* index, size_t index_bytes, int32_t N, const fr_cloud_query_cfg* cfg, void* workspace,
                   size_t workspace_bytes, fr_stream_t stream);

/* ---- DBSCAN and the target selection of global_planning ---------------------------------------------------------------------
 * The middle of the reference's global_planning (models/SLAM/gaussian.py:1216-1276; the same lines at gaussian_object.py:1419-1479):
 * the Gaussians of a height band, torch.quantile of their scores, sklearn.cluster.DBSCAN(eps, min_samples) on the host over those
 * above it, a Python loop for the cluster with the highest score.  Arithmetic and the labelling rule in csrc/fr_cluster_math.h:
 * binary32, one rounding per written operation, d2 = (dx*dx + dy*dy) + dz*dz, a neighbour when d2 <= eps*eps (itself included);
 * core = at least min_samples neighbours; clusters = connected components of the core points, numbered by ascending lowest
 * original index of their core points; a point that is not core takes the lowest cluster number among its core neighbours, else
 * -1.  These are sklearn's labels_ wherever no pair lies within rounding of eps.  A point with a non-finite coordinate is noise
 * and nobody's neighbour (sklearn raises).  Integer atomics only: the same call gives the same bytes.
 * Nothing is allocated, nothing is read back, no environment variable is read; every launch and memset is on `stream`.
 * The search grid has 1024 cells per axis of side max(1.125 eps, extent / 1024), per axis: a cloud wider than that (115 m at
 * eps = 0.1) gets larger cells on that axis, which is slower and never wrong; status reports the three sides. */
#define FR_CLUSTER_MAX_POINTS (1 << 26)
#define FR_DBSCAN_STATUS_WORDS 8         /* int32: {clusters, finite points, side x, side y, side z (float bits), 0, 0, 0} */
#define FR_TARGET_STATUS_WORDS 16        /* int32: {n_band, n_above, n_clusters, max_label, n_selected, argmax, side x, side y, side z
                                            (float bits), nan flag, threshold (float bits), finite points among those above, 0...} */
/* Host-only queries, non-decreasing in their argument (0 for an argument outside [0, FR_CLUSTER_MAX_POINTS]). */
size_t fr_dbscan_workspace_bytes(int32_t N);
size_t fr_target_select_workspace_bytes(int32_t P);
/* labels [N] int32 of points [N,3].  status: FR_DBSCAN_STATUS_WORDS int32 on the device.  FR_EINVAL for N outside the limits, an eps
 * whose square is not a normal binary32 number, min_samples < 1, a null pointer (points and labels may be null when N = 0), a
 * pointer not 4-byte (workspace: 8-byte) aligned, a short workspace. */
int fr_dbscan(int32_t N, const float* points, float eps, int32_t min_samples, int32_t* labels, int32_t* status,
              void* workspace, size_t workspace_bytes, fr_stream_t stream);
/* One call for gaussian.py:1221-1267 over means3D [P,3] and scores [P]; every output stays on the device, each list ascending:
 *   out_band_idx [P]      the rows with lower_y <= y <= upper_y (points_index_range), n_band of them;
 *   out_threshold [1]     torch.quantile(scores[band], q): the order statistics floor and ceil of fl(q * fl(n_band - 1)) by radix
 *                         select, joined by frk_lerp (NaN when the band is empty);
 *   out_above_idx [P]     the band rows with score > threshold (points_index), n_above of them;
 *   out_labels [P]        the DBSCAN labels of those rows, in the order of out_above_idx;
 *   out_selected_idx [P]  the rows of out_above_idx whose label is max_label (selected_points_index), n_selected of them.
 * max_label follows the reference's loop: from max_score = -1 a cluster wins on strict >, so the lowest label wins a tie; when no
 * cluster qualifies it stays -1, which selects the NOISE rows, as `labels == max_count_label` does there.  status
 * (FR_TARGET_STATUS_WORDS int32 on the device, the one thing a caller reads): the counts, max_label, the lowest row that attains
 * the band's highest score (-1 for an empty band: the reference's `else` branch at 1274), the cell sides, and a flag that is 1
 * when a band score is NaN -- the threshold is then not torch's, and the caller takes another route.
 * Only the first n_* entries of a list are written.  FR_EINVAL as fr_dbscan, and for q outside [0, 1]. */
int fr_target_select(int32_t P, const float* means3D, const float* scores, float lower_y, float upper_y, float q, float eps,
                     int32_t min_samples, int32_t* out_band_idx, int32_t* out_above_idx, int32_t* out_labels,
                     int32_t* out_selected_idx, float* out_threshold, int32_t* status, void* workspace, size_t workspace_bytes,
                     fr_stream_t stream);

/* ---- render-quality evaluation: PSNR, SSIM and depth error per view ------------------------------------------------------------
 * What NavTester.eval_navigation computes per rendered pose (tester_gaussians_navigation.py:1450-1491: color.clamp_(0, 1),
 * calc_psnr(color, rgb_gt).mean(), mean |depth - depth_gt|, ssim(color, rgb_gt), the `torch.isinf(psnr)` skip) and report_progress
 * per training frame (models/SLAM/utils/eval_helpers.py:230-257), for a batch of V views in three launches.  Arithmetic in
 * csrc/fr_eval_math.h over csrc/fr_loss_math.h (the SSIM map is the image loss's, bit for bit, except where a window's mean is below
 * 2^-5 in either image: there the reference's raw moments, which the loss's moments about 0.5 cannot match): per pixel binary32, one rounding
 * per written operation; every sum binary64 -- per-workgroup partials stored plainly and added in a fixed order, a row finalised in
 * binary64 and rounded once.  No atomics: the same call gives the same bits.  Device pointers, explicit stream, nothing allocated,
 * nothing read back.
 *   rows[v]  = {psnr, ssim, depth_l1, depth_rmse, mse_r, mse_g, mse_b, depth_count}
 *              psnr = the mean over the three channels of 20 log10(1 / sqrt(mse_c)); ssim = the mean of the SSIM map over 3 H W;
 *              depth_l1 = sum |dd| / depth_count, depth_rmse = sqrt(sum dd^2 / depth_count), dd = (depth - gt_depth) [* mask] in
 *              binary32.  The reference's own "RMSE" (eval_helpers.py:242-251) takes sqrt of EACH square and so equals its L1;
 *              that is not reproduced under this name.  depth_count = H W, or with depth_valid_only the pixels with gt_depth > 0
 *              (none: 0 / 0 = NaN, as torch gives).  Without depth the three depth entries are NaN.
 *   summary  = {views kept, mean psnr, mean ssim, mean depth_l1, mean depth_rmse, 0, 0, V}: the means over the views the reference
 *              keeps, added in index order in binary64.  A view whose psnr is infinite (render == target in a channel; an empty
 *              mask) is left out of every mean; a NaN psnr is not and makes the means NaN; no view kept: NaN.
 * With a mask (0 / 1 bytes) the clamped render and the target are multiplied by it before PSNR and SSIM, and the depth difference
 * as well.  The clamp keeps a NaN a NaN, as torch.clamp does. */
#define FR_EVAL_ROW 8
enum { FR_EVAL_GT_F32_CHW = 0,    /* gt_rgb: float [V][3][H][W]                                                        */
       FR_EVAL_GT_U8_HWC  = 1 };  /* gt_rgb: uint8 [V][H][W][gt_channels], channels 0..2 used, value / 255 (Habitat)   */
typedef struct {
	int32_t V, H, W;                  /* 1 <= V <= 65535, H W <= 2^30 */
	int32_t gt_layout, gt_channels;   /* gt_channels: 3 or 4, U8_HWC only                                             */
	int32_t clamp_render;             /* 1: render clamped to [0,1] first (eval_navigation's color.clamp_)            */
	int32_t depth_valid_only;         /* 0: depth error averaged over all H W pixels (eval_navigation);               */
	                                  /* 1: summed where gt_depth > 0, divided by their count (report_progress)       */
	int64_t render_view_stride, depth_view_stride, gt_depth_view_stride;   /* in elements; >= 3 H W, H W, H W: a view's image is
	                                     contiguous, the views need not be (the depth of fr_render_views is channel 0 of [V,3,H,W]) */
} fr_view_metrics_cfg;
/* Host only; 0 for an argument outside the limits. */
size_t fr_view_metrics_workspace_bytes(int32_t V, int32_t H, int32_t W);
/* rows [V][FR_EVAL_ROW] and summary [FR_EVAL_ROW] of a batch.  depth and gt_depth may both be null (colour only); mask [V][H][W]
 * or null.  FR_EINVAL for a null cfg, render, gt_rgb, rows or summary, V / H / W outside the limits, an unknown layout, gt_channels
 * other than 3 or 4 for a byte target, a flag that is not 0 or 1, only one of depth / gt_depth, a view stride below its image,
 * a null, short or not 8-byte aligned workspace. */
int fr_view_metrics(const fr_view_metrics_cfg* cfg, const float* render, const float* depth, const void* gt_rgb,
                    const float* gt_depth, const uint8_t* mask /* [V][H][W] 0/1 or null */,
                    float* rows /* [V][FR_EVAL_ROW] */, float* summary /* [FR_EVAL_ROW] */,
                    void* workspace, size_t workspace_bytes, fr_stream_t stream);
/* The summary alone over rows [V][FR_EVAL_ROW] that several fr_view_metrics calls filled slice by slice (an evaluation in chunks):
 * one launch.  FR_EINVAL for a null pointer or V < 1. */
int fr_view_metrics_summary(const float* rows, int32_t V, float* summary, fr_stream_t stream);

/* ---- measurement hooks (not part of the reference surface) ------------------------------------------ */

/* When enabled, every fr_fisher_views call records a pair of HIP events around its dominant kernel
 * (k_fisher_tile_v4 / _v3 in the score-only mode, k_fisher_tile_v3h / _v3g / _v2 otherwise) on the stream the kernel is launched on.  Enabling or disabling clears the record. */
int fr_profile_enable(int on);
/* Waits for the recorded events and writes up to max_n per-launch durations in milliseconds; returns the count
 * (or -1 on a HIP error).  This is the only entry point that blocks. */
int fr_profile_fetch(float* ms, int max_n);

#ifdef __cplusplus
}
#endif
#endif /* FISHER_RAST_H_INCLUDED */
