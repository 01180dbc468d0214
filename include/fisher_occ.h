/*
 * fisher_occ.h -- C ABI of the planner-side kernels in libfisher_rast.so (MI355X / gfx950): the occupancy-map update
 * and the frontier extraction that sit either side of view scoring in a planning round.
 *
 * Reference interfaces replaced (paths relative to the reference tree):
 *   fr_occ_update        <- AstarPlanner.update_occ_map           planning/astar.py:202-301
 *                           (11 depth samples per pixel, torch.unique count binning into a 3 x H x W grid,
 *                            one cv2.line per occupied cell -- a Python loop on the host -- and the normalised add)
 *   fr_occ_freespace     <- AstarPlanner.build_connected_freespace planning/astar.py:401-447
 *                           (arg-max label, Gaussian blocking with count > 25, 3x3 opening, largest 8-connected component)
 *   fr_occ_frontiers     <- AstarPlanner.build_frontiers           planning/astar.py:540-683
 *                           (dilate - free AND unknown, dilate, components, min area 10, largest / combined / closest)
 *   fr_occ_erode         <- cv2.erode(free_space, np.ones((k, k)))  planning/astar.py:805, 1388
 *   fr_occ_cells_of      <- datasets/util/map_utils.py:106-125 discretize_coords
 *   fr_occ_ring_candidates <- AstarPlanner.generate_candidate / generate_candidate_object planning/astar.py:1383-1430, 1432-1469
 *                           fused with the free-space filter of the candidate loop planning/astar.py:1387-1401
 *   fr_occ_free_candidates <- AstarPlanner.sample_random_candidate   planning/astar.py:782-837
 *   fr_occ_object_cells  <- AstarPlanner.build_object_frontiers    planning/astar.py:686-734
 *                           (torch.unique(dim=0, return_counts=True) over every object Gaussian's cell, count > 3, a host mask
 *                            painted and read back with np.where)
 *   fr_occ_grid_candidates <- AstarPlanner.generate_candidate_adv_object(mode="sorted") planning/astar.py:1471-1588
 *                           (the ordered grid of rings and angles), fused with the free-space filter planning/astar.py:1387-1401
 *   fr_plan_actions_object <- NavTester.action_planning_object_adv   tester_gaussians_navigation.py:2403-2496
 *                           (waypoint pruning near the goal, orientation-only mode, waypoint skipping, up to 200 actions)
 *
 * Conventions are fisher_rast.h's: device pointers unless noted, explicit stream, no allocation, no device
 * synchronisation, 0 or an FR_E* code, message through fr_last_error().
 * occ_map is the planner's float32 [3][grid_h][grid_w] tensor (0 unknown, 1 occupied, 2 free), updated in place.
 */
#ifndef FISHER_OCC_H_INCLUDED
#define FISHER_OCC_H_INCLUDED

#include "fisher_rast.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fr_occ_cfg {
	int32_t grid_w, grid_h;            /* grid_dim[0], grid_dim[1]                      (astar.py:74, 86) */
	float cell_size;                   /* metres per cell                                                  */
	float center_x, center_z;          /* map_center                                     (astar.py:80, 90) */
	float height_lower, height_upper;  /* floor / ceiling filter on world y              (astar.py:265, 284) */
	float far_distance;                /* pcd_far_distance                               (astar.py:247)    */
} fr_occ_cfg;

/* frontier selection (AstarPlanner.frontier_select_method) */
enum { FR_OCC_LARGEST = 0, FR_OCC_COMBINED = 1, FR_OCC_CLOSEST = 2 };

/* bytes of scratch for any of the calls below on this grid */
size_t fr_occ_workspace_bytes(const fr_occ_cfg* cfg);

/* update_occ_map.  depth: [H][W] float32 (device).  intr = {fx, fy, cx, cy} and c2w (row-major 4x4) are HOST arrays;
 * sample_fracs (HOST, n_samples <= 32): the fractions of the depth sampled along each ray, the last one being the depth
 * point itself (the reference: linspace(1e-3, 0.95, 11) with the last set to 1).  cam_col / cam_row: the camera's cell
 * (astar.py:211-213, computed by the caller exactly as the reference does on the host).  The 3 x 3 block round it is
 * marked with the rules of the reference's slice [cam-1 : cam+2]: clipped past the last row / column, empty when the
 * camera is in row 0 or column 0 (the slice then starts at -1, which counts from the end). */
int fr_occ_update(const fr_occ_cfg* cfg, const float* depth, int32_t W, int32_t H, int32_t downsample,
                  const float intr[4], const float c2w[16], const float* sample_fracs, int32_t n_samples,
                  int32_t cam_col, int32_t cam_row, float* occ_map,
                  void* workspace, size_t workspace_bytes, fr_stream_t stream);

/* build_connected_freespace.  points: [n_points][3] world-frame Gaussian means or null.  free_space: uint8 [grid_h][grid_w] out. */
int fr_occ_freespace(const fr_occ_cfg* cfg, const float* occ_map, const float* points, int32_t n_points,
                     uint8_t* free_space, void* workspace, size_t workspace_bytes, fr_stream_t stream);

/* build_frontiers after build_connected_freespace.  Outputs (device):
 *   frontier   uint8 [grid_h][grid_w]   boundary AND unknown, before the dilation             (self.frontier)
 *   target     uint8 [grid_h][grid_w]   the selected component                                 (self.target_frontier)
 *   cells      int32 [max_cells][2]     its (col, row) cells in raster order                   (np.where order)
 *   counts     int32 [4]                {frontier cells before dilation, components over min_area, cells of target, root cell of target or -1}
 * cam_row / cam_col: self.cam_pos. */
int fr_occ_frontiers(const fr_occ_cfg* cfg, const float* occ_map, const uint8_t* free_space,
                     int32_t cam_row, int32_t cam_col, int32_t method, int32_t min_area,
                     uint8_t* frontier, uint8_t* target, int32_t* cells, int32_t max_cells, int32_t* counts,
                     void* workspace, size_t workspace_bytes, fr_stream_t stream);

/* cv2.erode(src, ones(k, k)) with cv2's defaults: anchor (k/2, k/2), cells outside the map do not constrain. */
int fr_occ_erode(const fr_occ_cfg* cfg, const uint8_t* src, uint8_t* dst, int32_t ksize, fr_stream_t stream);

/* discretize_coords for n (x, z) pairs taken from xyz[n][3] (columns 0 and 2): cells[n][2] = (col, row), int32 */
int fr_occ_cells_of(const fr_occ_cfg* cfg, const float* xyz, int32_t n, int32_t* cells, fr_stream_t stream);

/* Candidate poses on a ring around centres drawn (with replacement) from `centers` [n_centers][2] = (x, z):
 * position = centre + r (sin t, 0, cos t) at height cam_height, t = 2 pi u0, r = min_range + u1 (radius - min_range),
 * centre index = floor(u2 n_centers); orientation = yaw (t + pi) with columns 0 and 1 negated (astar.py:1406-1423).
 * The uniforms come from a counter-based generator keyed by (seed, k): see occ_uniform in fisher_occ.hip, restated in
 * oracle/occupancy_frontier.py.  c2w: [K][16] row-major, out.  keep: [K] uint8 out or null -- 1 where the pose's cell lies in
 * `eroded_free` (uint8 [grid_h][grid_w], or null = keep all); as in the reference the filter only applies when more
 * than `min_free` cells of eroded_free are set (astar.py:1389: 40). */
int fr_occ_ring_candidates(const fr_occ_cfg* cfg, const float* centers, int32_t n_centers, int32_t K,
                           float min_range, float radius, float cam_height, uint32_t seed,
                           const uint8_t* eroded_free, int32_t min_free, float* c2w, uint8_t* keep, fr_stream_t stream);

/* Uniformly placed poses in the (already eroded) free space: the free cells in raster order, a quarter as many draws with
 * replacement, position at the cell centre and height agent_y, uniform yaw with columns 1 and 2 negated (astar.py:805-835).
 * c2w: [max_out][16] out; counts: device int32[2] = {free cells, poses written}. */
int fr_occ_free_candidates(const fr_occ_cfg* cfg, const uint8_t* eroded_free, float agent_y, uint32_t seed,
                           float* c2w, int32_t max_out, int32_t* counts, void* workspace, size_t workspace_bytes,
                           fr_stream_t stream);

/* build_object_frontiers (astar.py:686-734): the map cells that hold more than min_count (the reference: 3) of the Gaussians
 * points [n_points][3], as (col, row) in raster order -- np.where order.  A point's cell is fr_occ_cells_of's: discretize_coords,
 * clamped to the grid, so a Gaussian outside the map counts in the border cell, as in the reference.  A point whose x or z is not
 * finite is NOT binned (the reference's cast is undefined there).  Integer atomics: the answer does not depend on the order.
 *   cells   int32 [max_cells][2] out; with more cells than max_cells nothing is written past it
 *   counts  int32 [2] (device) = {cells with count > min_count -- the true number, also beyond max_cells --, points binned}
 * n_points = 0 is legal (points may be null) and gives {0, 0}.  Workspace: fr_occ_workspace_bytes(), 16-byte aligned. */
int fr_occ_object_cells(const fr_occ_cfg* cfg, const float* points, int32_t n_points, int32_t min_count, int32_t* cells,
                        int32_t max_cells, int32_t* counts, void* workspace, size_t workspace_bytes, fr_stream_t stream);

/* generate_candidate_adv_object(mode="sorted") (astar.py:1514-1588): K poses on an ordered grid of rings and angles.
 *   n_theta      max(1, round(2 pi / deg2rad(theta_step_deg))), taken by the caller on the host as the reference does.  The angles
 *                are the first max(1, n_theta - 1) points of linspace(0, 2 pi, n_theta): the reference drops the closing angle, so
 *                a step of 15 degrees gives 23 angles, not 24.
 *   radial_bins  the radii are linspace(min_range, radius, radial_bins), or sqrt(linspace(min_range^2, radius^2)) with sqrt_area
 *                != 0 and more than one bin.  Both tables are taken in binary64 and rounded once to binary32.
 * Pose k takes grid entry k mod (radial_bins * angles), the ring index the slow one (meshgrid(indexing='ij'), then slice or
 * repeat); its centre is drawn with replacement by fr_occ_ring_candidates' generator (index = floor(u2 n), keyed by (seed, k));
 * position = centre + r (sin t, 0, cos t) at height cam_height, orientation = yaw (t + pi) with columns 0 and 1 negated; keep is
 * fr_occ_ring_candidates' eroded-free-space rule (keep may be null).  The centres come from ONE of
 *   centers      float32 [n_centers][2] = (x, z), n_centers > 0, or
 *   cells        int32 [n_centers][2] = (col, row) as fr_occ_object_cells leaves them, of which min(*n_cells_dev, n_centers) are
 *                there (n_cells_dev: device int32, e.g. fr_occ_object_cells' counts; n_centers: the rows `cells` has room for):
 *                object cells -> candidates -> filter run back to back without a host read.  A cell's world position is
 *                (cell - grid_dim // 2) * cell_size + map_center, as build_frontiers gives it.  With no cell on the device every
 *                pose is a zero matrix with keep 0.
 * c2w: float32 [K][16] row-major, out.  K = 0 returns FR_OK without a launch. */
int fr_occ_grid_candidates(const fr_occ_cfg* cfg, const float* centers, int32_t n_centers, const int32_t* cells, const int32_t* n_cells_dev,
                           int32_t K, float min_range, float radius, int32_t n_theta, int32_t radial_bins, int32_t sqrt_area,
                           float cam_height, uint32_t seed, const uint8_t* eroded_free, int32_t min_free, float* c2w, uint8_t* keep,
                           fr_stream_t stream);

/* ---- path planning: one cost field from the start, paths to all goals ------------------------------------------------------
 * Replaces AstarPlanner.setup_start + planning (planning/astar.py:449-538, 1591-1777): the reference runs a best-first search
 * per goal on the host; these calls build the single-source shortest-path field of the same cost model (csrc/fr_plan_math.h)
 * on the device and read every goal's path off it.  Cells are (row, col); a cell's raster index is row * grid_w + col.
 *
 *   fr_plan_grid    occ_plan uint8 [grid_h][grid_w] = the reference's occ_map_np: arg-max label == 1, plus the cells holding more
 *                   than 50 of the Gaussians `points` [n_points][3] (or null) with cam_height - 1 <= y <= cam_height (cells by the
 *                   rule of fr_occ_cells_of; Gaussians outside the grid are ignored), dilated 3 x 3, the start cleared.
 *                   status int32 [FR_PLAN_STATUS_WORDS] (device) = {occupied cells among the start's 8 neighbours in the dilated
 *                   map, Gaussians binned, 0, 0}; fr_plan_field then sets words 2 and 3.
 *   fr_plan_tiers   tiers uint8 [grid_h][grid_w] from free_space (fr_occ_freespace's output): 0 where not free, else
 *                   1 | tier << 1, tier = 3, 2, 1, 0 for an L1 distance to the nearest non-free cell of <= 5, <= 10, <= 20, more.
 *   fr_plan_field   field uint64 [grid_h][grid_w]: (bits of the binary32 cost) << 32 | raster index of the parent, all ones where
 *                   the start does not reach.  status[2] = 1 when the start is in free space, status[3] = the number of rounds
 *                   that changed something.  The call launches rounds over FR_PLAN_TILE-square tiles and READS ONE DEVICE WORD
 *                   every few rounds (it synchronises the stream); past fr_plan_round_cap() rounds it returns FR_ENOSPACE.
 *                   host_counts: HOST int32 [2] or null = {rounds launched, convergence reads}.
 *   fr_plan_paths   goals int32 [n_goals][2] = (row, col).  paths int32 [n_goals][max_len][2] = (x, z) = (col, row) from the start
 *                   to the end cell; lengths int32 [n_goals]: 0 = no path (goal occupied in occ_plan or outside the grid, nothing
 *                   reached within Chebyshev distance 1 of it, or the end cell is the start), -1 = the path as walked, before
 *                   any shortcut, is longer than max_len (repeat with a larger one; grid_w * grid_h + 1 always suffices).  shortcut != 0 runs the reference's shortcut loop,
 *                   a segment being clear when no occupied cell's centre lies within 3.5 cells of it.
 * Workspace: fr_plan_workspace_bytes(), 16-byte aligned, shared by fr_plan_grid and fr_plan_field (not kept between calls). */
#define FR_PLAN_STATUS_WORDS 4
#define FR_PLAN_TILE 64

size_t fr_plan_workspace_bytes(const fr_occ_cfg* cfg);
int32_t fr_plan_round_cap(const fr_occ_cfg* cfg);

int fr_plan_grid(const fr_occ_cfg* cfg, const float* occ_map, const float* points, int32_t n_points, float cam_height,
                 int32_t start_row, int32_t start_col, uint8_t* occ_plan, int32_t* status,
                 void* workspace, size_t workspace_bytes, fr_stream_t stream);

int fr_plan_tiers(const fr_occ_cfg* cfg, const uint8_t* free_space, uint8_t* tiers, fr_stream_t stream);

int fr_plan_field(const fr_occ_cfg* cfg, const uint8_t* tiers, int32_t start_row, int32_t start_col, uint64_t* field,
                  int32_t* status, int32_t* host_counts, void* workspace, size_t workspace_bytes, fr_stream_t stream);

int fr_plan_paths(const fr_occ_cfg* cfg, const uint64_t* field, const uint8_t* occ_plan, int32_t start_row, int32_t start_col,
                  const int32_t* goals, int32_t n_goals, int32_t shortcut, int32_t* paths, int32_t max_len, int32_t* lengths,
                  fr_stream_t stream);

/* ---- action planning: every goal's path to the agent's action list, and the poses along it -----------------------------------
 * Replaces the second half of NavTester.action_planning (tester_gaussians_navigation.py:2246-2330): the waypoint follower that
 * walks a grid path with the agent's three actions (1 forward by forward_step_size along the camera's +z, 2 / 3 yaw by -/+
 * turn_angle degrees), the final re-orientation towards the goal pose, the duplicate-list filter -- and the roll-out and inversion
 * of the poses that the path evaluation repeats on the host (1684-1687).  Binary64 arithmetic (csrc/fr_action_math.h), quirks kept.
 *
 *   fr_plan_actions     paths int32 [n_goals][max_len][2] and lengths int32 [n_goals] as fr_plan_paths leaves them; goals int32
 *                       [n_goals][2] = (row, col), read only for a path of one point, which gets it appended as the reference does;
 *                       goals_c2w float32 [n_goals][16] row-major; agent_c2w: HOST double [16], taken to be rigid, its height
 *                       replaced by cam_height.  cell_size is the planner's own binary64 value (cfg's binary32 one is not read here:
 *                       the reference converts cells with the Python float); the map centre is cfg's, promoted.  Outputs (device):
 *                         actions   uint8 [n_goals][queue_size]
 *                         n_actions int32 [n_goals]                    -1 where lengths[g] <= 0: the goal has no path
 *                         keep      uint8 [n_goals]                    1 where the goal has a path and no earlier goal with a path
 *                                                                      produced the same list (an empty list is a list)
 *                         w2c       float32 [n_goals][queue_size][16]  the inverse of the pose after each action, rounded once
 *                         c2w_xz    float64 [n_goals][queue_size][2]   the pose's x and z after each action
 *                         map_xz    int32 [n_goals][queue_size][2]     their cell, int((v - centre) / cell_size + grid_dim // 2)
 *                       Entries past n_actions[g] are written as zeros.  The entries with action 1 are the reference's world_path /
 *                       map_path.  Two launches: the lists, then the duplicate search.
 *   fr_rollout_actions  the roll-out alone, for lists from elsewhere: start_c2w HOST double [16] (used as it is), actions uint8
 *                       [n_lists][queue_size], n_actions int32 [n_lists] (negative counts as 0); w2c float32 [n_lists][queue_size][16],
 *                       c2w float64 [n_lists][queue_size][16] or null, zeros past a list's end.  Given fr_plan_actions' lists and its
 *                       start, w2c comes out bit for bit the same.
 * queue_size: 1 .. FR_ACTION_MAX_QUEUE, else FR_EINVAL.  n_goals / n_lists = 0 returns FR_OK without a launch. */
#define FR_ACTION_MAX_QUEUE 128

int fr_plan_actions(const fr_occ_cfg* cfg, const int32_t* paths, int32_t max_len, const int32_t* lengths, const int32_t* goals,
                    const float* goals_c2w, int32_t n_goals, const double* agent_c2w, double cam_height, double forward_step_size,
                    double turn_angle, int32_t queue_size, double cell_size, uint8_t* actions, int32_t* n_actions, uint8_t* keep,
                    float* w2c, double* c2w_xz, int32_t* map_xz, fr_stream_t stream);

int fr_rollout_actions(const double* start_c2w, const uint8_t* actions, const int32_t* n_actions, int32_t n_lists, int32_t queue_size,
                       double forward_step_size, double turn_angle, float* w2c, double* c2w, fr_stream_t stream);

/* ---- the object round's follower ---------------------------------------------------------------------------------------------
 * Replaces the loop of NavTester.action_planning_object_adv (tester_gaussians_navigation.py:2403-2496): per goal the path is padded
 * (a path of one point), pruned near the goal, and walked with early stop, orientation-only mode near the goal and waypoint
 * skipping, for up to FR_ACTION_OBJECT_MAX actions (the reference's SAFETY_CAP; the planning queue does not cut these lists).
 * Binary64 arithmetic (csrc/fr_action_object_math.h, which states every rule), quirks kept.  Inputs as fr_plan_actions'; the
 * pruning measures against the agent's own height agent_c2w[1][3], the walk starts at cam_height.  Outputs (device):
 *   actions    uint8 [n_goals][200]           n_actions  int32 [n_goals], -1 where lengths[g] <= 0: the goal has no path
 *   keep       uint8 [n_goals]                1 where the list is not empty and no earlier goal made the same list (an empty list
 *                                             is dropped, unlike fr_plan_actions')
 *   w2c        float32 [n_goals][200][16]     c2w_xz  float64 [n_goals][200][2]     map_xz  int32 [n_goals][200][2]
 *   pruned     int32 [n_goals][max_len + 1][2] the pruned path (x, z), what the reference returns as paths_arr
 *   pruned_len int32 [n_goals]                its points: at least 2 with a path, 0 without
 * Zeros past every list and every pruned path.  Two launches; n_goals = 0 returns FR_OK without one. */
#define FR_ACTION_OBJECT_MAX 200

int fr_plan_actions_object(const fr_occ_cfg* cfg, const int32_t* paths, int32_t max_len, const int32_t* lengths, const int32_t* goals,
                           const float* goals_c2w, int32_t n_goals, const double* agent_c2w, double cam_height, double forward_step_size,
                           double turn_angle, double cell_size, uint8_t* actions, int32_t* n_actions, uint8_t* keep, float* w2c,
                           double* c2w_xz, int32_t* map_xz, int32_t* pruned, int32_t* pruned_len, fr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
