"""`AstarPlanner`'s occupancy-map and frontier operators on MI355X (reference: planning/astar.py).

In scope (same names, arguments and return conventions as the reference):
    init (66-103)                      update_occ_map (202-301)        build_connected_freespace (401-447)
    build_frontiers (540-683)          generate_candidate (1406-1430)  generate_candidate_object (1432-1469)
    the free-space filter of the candidate loop (1383-1401)            sample_random_candidate (782-837)
    setup_start + planning (449-538, 1591-1777): `PathPlanOps`, one cost field from the start, paths to all goals
    `PathPlanOps.plan_actions`: the loop of NavTester.action_planning (tester_gaussians_navigation.py:2231-2330), every goal's path
    and action list and the poses along it from two calls and one host read (`ActionPlan`)
    `PathPlanOps.plan_actions_object`: the loop of NavTester.action_planning_object_adv (2385-2496), up to 200 actions (`ObjectActionPlan`)
    `GoalSelectOps`: global_planning (843-1000), build_object_frontiers (686-734), generate_candidate_adv_object (1471-1588),
    global_object_planning (1151-1346), built from the stages above
Visualisation, the RRT planner and the VLM frontier selection are NOT rebuilt: they are reference Python that stays as it
is.  `OccupancyOps.install(cls)` / `PathPlanOps.install(cls)` / `GoalSelectOps.install(cls)` graft the methods onto the reference class;
`AstarPlanner` below is the same operator surface as a standalone object for tests and benchmarks.

What changes underneath: the reference bins the depth samples with torch ops and then walks every occupied cell in a
Python loop on the host (one `cv2.line` each, astar.py:291-297), and runs `cv2` morphology / connected components on the
CPU after copying the map down.  Here the whole step is a handful of HIP kernels on the resident map
(fisher_occ.h: fr_occ_update / fr_occ_freespace / fr_occ_frontiers); the only host traffic is the selected frontier's cells.
Candidate poses come from one kernel each (fr_occ_ring_candidates: centre pick, ring sample, pose, eroded-free-space
test; fr_occ_free_candidates: uniform poses in the free space) driven by a counter-based generator, so a call is
reproducible from its seed and has a NumPy restatement in oracle/occupancy_frontier.py to test against.
"""
import ctypes
import math

import numpy as np
import torch

from fisher_rast import _lib

_METHODS = {"largest": 0, "combined": 1, "closest": 2}


class OccupancyOps:
    """Mixin with the accelerated occupancy / frontier methods.  Needs the attributes AstarPlanner.__init__ sets:
    device, cell_size, height_lower, height_upper, pcd_far_distance, frontier_select_method, K, radius, min_range.

    One planner, one stream at a time: every method runs on the torch stream that is current when it is called, and the resident
    map and the workspaces (`_occ_ws`, `_occ_cells`, `_plan_ws`, `_free_space_dev`) belong to the object, not to a stream.  Calls
    made on different streams must be ordered by the caller, as two writers of `occ_map` would be."""

    # -- internals -----------------------------------------------------------------------------------------------
    def _occ_cfg(self):
        mc = self.map_center
        if isinstance(mc, torch.Tensor):
            # the host copy is kept until the tensor is replaced or written: one device read, not one per call
            held = getattr(self, "_occ_mc_held", None)
            if held is None or held[0] is not mc or held[1] != mc._version:
                held = self._occ_mc_held = (mc, mc._version, mc.detach().cpu().numpy())
            mc = held[2]
        else:
            mc = np.asarray(mc)
        return _lib.OccCfg(int(self.grid_dim[0]), int(self.grid_dim[1]), float(self.cell_size), float(np.float32(mc[0])),
                           float(np.float32(mc[1])), float(self.height_lower), float(self.height_upper), float(self.pcd_far_distance))

    def _occ_workspace(self, cfg):
        lib = _lib.load()
        need = lib.fr_occ_workspace_bytes(ctypes.byref(cfg))
        ws = getattr(self, "_occ_ws", None)
        if ws is None or ws.numel() < need or ws.device != self.occ_map.device:
            ws = torch.empty((need,), dtype=torch.uint8, device=self.occ_map.device)
            self._occ_ws = ws
        return ws, need

    @staticmethod
    def _stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    # -- astar.py:66-103 ---------------------------------------------------------------------------------------------
    def _cell_of(self, x, z):
        """(col, row) of a world position: int((v - centre) / cell + dim // 2), the planner's own rule (astar.py:93-94, 211-212)."""
        mc = self._map_center_np
        return (int((x - mc[0]) / self.cell_size + self.grid_dim[0] // 2), int((z - mc[1]) / self.cell_size + self.grid_dim[1] // 2))

    def init(self, pose, intrinsic, scene_bounds=None):
        """Fresh map: 768 x 768 cells centred on the first pose, or the scene's x-z extent at the fixed cell size; every cell
        unknown (layer 0 = 1) except the 3 x 3 block under the camera, which is free (layer 2 = 2)."""
        T = pose.detach().cpu().numpy() if isinstance(pose, torch.Tensor) else np.asarray(pose)
        self.intrinsics = intrinsic
        self.cam_height = float(T[1, 3])
        self.frame_idx = 0
        if scene_bounds is None:
            self.grid_dim = np.array([768, 768])
            centre = T[[0, 2], 3]
        else:
            self.scene_bounds = scene_bounds
            lo, hi = (np.asarray(b) for b in scene_bounds)
            extent = (hi - lo)[[0, 2]] / self.cell_size
            self.grid_dim = np.array([int(extent[0] + 1), int(extent[1] + 1)])
            centre = (hi[[0, 2]] + lo[[0, 2]]) / 2
        self._map_center_np = np.asarray(centre)
        self.map_center = torch.from_numpy(self._map_center_np).to(self.device)
        gw, gh = int(self.grid_dim[0]), int(self.grid_dim[1])
        occ = torch.zeros((3, gh, gw), device=self.device)
        occ[0].fill_(1.)
        col, row = self._cell_of(T[0, 3], T[2, 3])
        self.cam_pos = np.array([row, col])
        occ[2, row - 1:row + 2, col - 1:col + 2] = 2.
        self.occ_map = occ

    # -- astar.py:202-301 --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update_occ_map(self, depth, c2w, t, downsample=1):
        """ Update Occulision map based on depth observation """
        lib = _lib.load()
        self.frame_idx = t
        c2w_h = c2w.detach().float().cpu() if isinstance(c2w, torch.Tensor) else torch.as_tensor(np.asarray(c2w)).float()
        mc = self.map_center.detach().cpu()
        cam_x, cam_z = c2w_h[0, 3], c2w_h[2, 3]
        cam_pos_x = int((cam_x - mc[0]) / self.cell_size + self.grid_dim[0] // 2)
        cam_pos_z = int((cam_z - mc[1]) / self.cell_size + self.grid_dim[1] // 2)
        self.cam_pos = np.array([cam_pos_z, cam_pos_x])
        if isinstance(depth, np.ndarray):
            depth = torch.from_numpy(depth)
        depth = depth.to(self.device).float().contiguous()
        width, height = depth.shape[2], depth.shape[1]
        K = self.intrinsics
        intr = (ctypes.c_float * 4)(float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]))
        c2w_a = (ctypes.c_float * 16)(*[float(v) for v in c2w_h.reshape(-1)])
        fr = torch.linspace(1e-3, 0.95, 11).clamp_(min=0.)
        fr[-1] = 1.
        fracs = (ctypes.c_float * 11)(*[float(v) for v in fr])
        cfg = self._occ_cfg()
        ws, need = self._occ_workspace(cfg)
        _lib.check(lib.fr_occ_update(ctypes.byref(cfg), depth.data_ptr(), width, height, int(downsample), ctypes.byref(intr),
                                     ctypes.byref(c2w_a), fracs, 11, cam_pos_x, cam_pos_z, self.occ_map.data_ptr(),
                                     ws.data_ptr(), need, self._stream()), "fr_occ_update")

    # -- astar.py:401-447 --------------------------------------------------------------------------------------------
    def build_connected_freespace(self, gaussian_points=None, as_tensor=False):
        """ find the connected free space to the robot: (H, W) uint8, 1 - free, 0 - occupied
        (np.ndarray like the reference, or the resident tensor with as_tensor=True) """
        lib = _lib.load()
        cfg = self._occ_cfg()
        ws, need = self._occ_workspace(cfg)
        free = torch.empty((int(self.grid_dim[1]), int(self.grid_dim[0])), dtype=torch.uint8, device=self.occ_map.device)
        pts, n = None, 0
        if gaussian_points is not None:
            pts_t = gaussian_points.detach().to(self.occ_map.device).float().contiguous()
            pts, n = pts_t.data_ptr(), int(pts_t.shape[0])
        _lib.check(lib.fr_occ_freespace(ctypes.byref(cfg), self.occ_map.data_ptr(), pts, n, free.data_ptr(), ws.data_ptr(), need,
                                        self._stream()), "fr_occ_freespace")
        self._free_space_dev = free
        return free if as_tensor else free.cpu().numpy()

    # -- astar.py:540-683 --------------------------------------------------------------------------------------------
    def build_frontiers(self, gaussian_points=None):
        """ Return frontiers in pixel space  """
        lib = _lib.load()
        free_dev = self.build_connected_freespace(gaussian_points, as_tensor=True)
        cfg = self._occ_cfg()
        ws, need = self._occ_workspace(cfg)
        gh, gw = int(self.grid_dim[1]), int(self.grid_dim[0])
        dev = self.occ_map.device
        frontier = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
        target = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
        max_cells = gh * gw
        cells = getattr(self, "_occ_cells", None)
        if cells is None or cells.shape[0] < max_cells or cells.device != dev:
            cells = torch.empty((max_cells, 2), dtype=torch.int32, device=dev)
            self._occ_cells = cells
        counts = torch.zeros((4,), dtype=torch.int32, device=dev)
        method = self.frontier_select_method
        if method not in _METHODS:
            raise ValueError(f"frontier_select_method {method!r} is not one of {sorted(_METHODS)} (the VLM selection stays reference Python)")
        _lib.check(lib.fr_occ_frontiers(ctypes.byref(cfg), self.occ_map.data_ptr(), free_dev.data_ptr(), int(self.cam_pos[0]),
                                        int(self.cam_pos[1]), _METHODS[method], 10, frontier.data_ptr(), target.data_ptr(),
                                        cells.data_ptr(), max_cells, counts.data_ptr(), ws.data_ptr(), need, self._stream()),
                   "fr_occ_frontiers")
        n_frontier, n_comp, n_target, _ = [int(v) for v in counts.cpu()]          # the one host sync of the step
        free_space = free_dev.cpu().numpy()
        self.frontier = frontier.cpu().numpy()
        if n_frontier == 0:
            self.target_frontier = None
            return None, free_space
        if n_comp == 0 or n_target == 0:
            return None, free_space
        if method == "largest":
            self.selection = 0
        self.target_frontier = target.cpu().numpy()
        map_center = self.map_center.cpu().numpy()
        select_pixels = cells[:n_target].cpu().numpy().astype(np.int64)              # (col, row) in np.where order
        select_pixels = (select_pixels - np.array([[self.grid_dim[0] // 2, self.grid_dim[1] // 2]])) * self.cell_size + map_center[None, :]
        if gaussian_points is not None:
            return select_pixels, free_space
        return self._fbe_point(select_pixels), free_space

    def _fbe_point(self, select_xy, min_thresh=0.5):
        """Frontier-based exploration target (astar.py:655-679): the selected cell nearest to `self.cam_pos` among those at
        least min_thresh away, else a point half a unit from it along the fixed 5 pi / 4 direction.  The reference measures
        the distance between the cells' WORLD coordinates and cam_pos, which holds GRID indices (row, col); kept as it is."""
        agent = np.asarray(self.cam_pos, dtype=np.float64)
        dist = np.sqrt(((select_xy - agent[None, :]) ** 2).sum(axis=1))
        far_enough = dist >= min_thresh
        if far_enough.any():
            pick = int(np.argmin(np.where(far_enough, dist, np.inf)))
            return select_xy[pick:pick + 1]
        ang = math.pi * 5 / 4
        return agent[None, :] - 0.5 * np.array([[math.cos(ang), math.sin(ang)]])

    # -- astar.py:1406-1430, 1432-1469 -------------------------------------------------------------------------------
    def _next_seed(self):
        """One 32-bit seed per call: from `self.candidate_seed` (an int, incremented) when set, else from torch's global CPU
        generator -- so `torch.manual_seed` makes a planning round reproducible, as it does for the reference's torch.rand."""
        fixed = getattr(self, "candidate_seed", None)
        if fixed is not None:
            self.candidate_seed = (int(fixed) + 1) & 0xFFFFFFFF
            return int(fixed) & 0xFFFFFFFF
        return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())

    def _ring_candidates(self, center_point, K, min_range, radius, eroded=None, min_free=40, seed=None):
        """K poses around the (x, z) rows of center_point (fr_occ_ring_candidates): ([K,4,4] c2w, [K] bool keep)."""
        lib = _lib.load()
        dev = self.occ_map.device
        centers = center_point.detach().to(dev).float()[:, :2].contiguous()
        c2w = torch.empty((int(K), 4, 4), dtype=torch.float32, device=dev)
        keep = torch.empty((int(K),), dtype=torch.uint8, device=dev)
        cfg = self._occ_cfg()
        seed = self._next_seed() if seed is None else int(seed) & 0xFFFFFFFF
        self.last_candidate_seed = seed
        _lib.check(lib.fr_occ_ring_candidates(ctypes.byref(cfg), centers.data_ptr(), int(centers.shape[0]), int(K), float(min_range),
                                              float(radius), float(self.cam_height), seed,
                                              None if eroded is None else eroded.data_ptr(), int(min_free), c2w.data_ptr(),
                                              keep.data_ptr(), self._stream()), "fr_occ_ring_candidates")
        return c2w, keep.bool()

    def generate_candidate(self, center_point: torch.Tensor, expansion=1, seed=None):
        """ sample camera poses from the center point (K, 4, 4) """
        return self._ring_candidates(center_point, self.K, self.min_range, self.radius * expansion, seed=seed)[0]

    def generate_candidate_object(self, center_point: torch.Tensor, expansion=1, seed=None):
        """ the object-centric ring: K_object poses between min_range_object and radius_object * expansion """
        return self._ring_candidates(center_point, self.K_object, self.min_range_object, self.radius_object * expansion, seed=seed)[0]

    def generate_candidate_in_freespace(self, center_point, free_space=None, expansion=1, ksize=10, min_free=40, seed=None):
        """generate_candidate + the free-space filter of the candidate loop (astar.py:1383-1401) in ONE launch: the poses
        whose cell lies in the free space eroded by a ksize x ksize box (all of them when that has no more than min_free cells)."""
        eroded = self._eroded_free(free_space, ksize)
        c2w, keep = self._ring_candidates(center_point, self.K, self.min_range, self.radius * expansion, eroded, min_free, seed)
        return c2w[keep]

    # -- astar.py:782-837 --------------------------------------------------------------------------------------------
    def sample_random_candidate(self, agent_pos, free_space, sample_range=1., sample_size: int = 100, seed=None):
        """ Randomly placed poses in the free space eroded by 11 x 11 (a quarter as many as it has cells), at the agent's height.
        sample_range / sample_size are accepted and unused, as in the reference. """
        lib = _lib.load()
        dev = self.occ_map.device
        eroded = self._eroded_free(free_space, 11)
        cfg = self._occ_cfg()
        ws, need = self._occ_workspace(cfg)
        max_out = (int(self.grid_dim[0]) * int(self.grid_dim[1])) // 4
        out = torch.empty((max_out, 4, 4), dtype=torch.float32, device=dev)
        counts = torch.zeros((2,), dtype=torch.int32, device=dev)
        seed = self._next_seed() if seed is None else int(seed) & 0xFFFFFFFF
        self.last_candidate_seed = seed
        y = float(agent_pos[1])
        _lib.check(lib.fr_occ_free_candidates(ctypes.byref(cfg), eroded.data_ptr(), y, seed, out.data_ptr(), max_out,
                                              counts.data_ptr(), ws.data_ptr(), need, self._stream()), "fr_occ_free_candidates")
        return out[:int(counts[1].item())]

    def _eroded_free(self, free_space, ksize):
        lib = _lib.load()
        dev = self.occ_map.device
        if free_space is None:
            free_dev = self._free_space_dev
        else:
            free_dev = (free_space if isinstance(free_space, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(free_space))).to(dev).to(torch.uint8).contiguous()
        eroded = torch.empty_like(free_dev)
        cfg = self._occ_cfg()
        _lib.check(lib.fr_occ_erode(ctypes.byref(cfg), free_dev.data_ptr(), eroded.data_ptr(), int(ksize), self._stream()), "fr_occ_erode")
        return eroded

    # -- astar.py:1387-1401: keep the candidates whose cell lies in the free space eroded by a 10 x 10 box ------------
    def filter_candidates_in_freespace(self, candidate_pose, free_space=None, ksize=10, min_free=40):
        """The filter alone, for poses that did not come from generate_candidate_in_freespace."""
        dev = self.occ_map.device
        eroded = self._eroded_free(free_space, ksize)
        if int(eroded.sum()) <= min_free:
            return candidate_pose
        mc = self.map_center.to(dev)
        col = ((candidate_pose[:, 0, 3] - mc[0]) / self.cell_size + self.grid_dim[0] // 2).long()
        row = ((candidate_pose[:, 2, 3] - mc[1]) / self.cell_size + self.grid_dim[1] // 2).long()
        return candidate_pose[eroded[row, col].bool()]

    def cells_of(self, xyz):
        """discretize_coords (datasets/util/map_utils.py:106-125) of the x / z columns of an [n, 3] tensor -> int32 [n, 2] (col, row)."""
        lib = _lib.load()
        xyz = xyz.detach().to(self.occ_map.device).float().contiguous()
        out = torch.empty((xyz.shape[0], 2), dtype=torch.int32, device=xyz.device)
        cfg = self._occ_cfg()
        _lib.check(lib.fr_occ_cells_of(ctypes.byref(cfg), xyz.data_ptr(), int(xyz.shape[0]), out.data_ptr(), self._stream()), "fr_occ_cells_of")
        return out

    @classmethod
    def install(cls, planner_cls):
        """Graft the accelerated methods onto the reference's AstarPlanner class."""
        for name in ("update_occ_map", "build_connected_freespace", "build_frontiers", "_fbe_point", "generate_candidate",
                     "generate_candidate_object", "generate_candidate_in_freespace", "sample_random_candidate", "_ring_candidates",
                     "_next_seed", "_eroded_free", "filter_candidates_in_freespace", "cells_of", "_occ_cfg", "_occ_workspace", "_stream"):
            setattr(planner_cls, name, cls.__dict__[name])
        return planner_cls


class ActionPlan:
    """What `PathPlanOps.plan_actions` returns.  Per goal, in goal order (G goals, Q = queue_size):
        paths       the grid paths as plan_paths gives them      n_actions  int32 [G], -1 without a path
        keep        uint8 [G]: has a path, and no earlier goal with a path has the same action list
        actions     uint8 [G, Q]      map_xz  int32 [G, Q, 2]    c2w_xz  float64 [G, Q, 2]   (zeros behind a list)
        w2c         DEVICE float32 [G, Q, 4, 4]: the inverse of the pose after each action; `kept_w2c()` gathers the kept rows there
    and of the kept goals only, as the reference's lists:
        kept_index, valid_global_points, path_actions, paths_arr (a path of one point has the goal cell appended, as the
        reference leaves it), world_path / map_path (the `action == 1` entries: tester 1707-1711)
    `triple()` is action_planning's return value; `reads` the host reads the call made."""

    def __init__(self, goal_c2ws, paths, n_actions, keep, actions, map_xz, c2w_xz, w2c, finishes, reads):
        self.paths, self.n_actions, self.keep, self.actions, self.map_xz, self.c2w_xz, self.w2c, self.reads = \
            paths, n_actions, keep, actions, map_xz, c2w_xz, w2c, reads
        self.kept_index = [int(k) for k in np.nonzero(keep)[0]]
        self.valid_global_points = [goal_c2ws[k] for k in self.kept_index]
        self.path_actions = [[int(a) for a in actions[k, :n_actions[k]]] for k in self.kept_index]
        self.paths_arr = [np.concatenate([paths[k], finishes[k][None, :]], axis=0) if len(paths[k]) == 1 else paths[k] for k in self.kept_index]
        fwd = [np.nonzero(actions[k, :n_actions[k]] == 1)[0] for k in self.kept_index]
        self.world_path = [[c2w_xz[k, j].copy() for j in f] for k, f in zip(self.kept_index, fwd)]
        self.map_path = [[map_xz[k, j].astype(np.int64) for j in f] for k, f in zip(self.kept_index, fwd)]

    def triple(self):
        return self.valid_global_points, self.path_actions, self.paths_arr

    def kept_w2c(self, rows=None):
        """w2c of the kept goals (or of `rows`, positions in the kept lists), gathered on the device: [n, Q, 4, 4]"""
        idx = self.kept_index if rows is None else [self.kept_index[r] for r in rows]
        return self.w2c[torch.as_tensor(idx, dtype=torch.long, device=self.w2c.device)]


class ObjectActionPlan(ActionPlan):
    """What `PathPlanOps.plan_actions_object` returns: an ActionPlan with Q = 200 whose `keep` drops a list without an action, and
    whose `paths_arr` are the PRUNED paths (int32 [M, 2]), as action_planning_object_adv returns them; `pruned` holds every goal's
    (an empty array without a path)."""

    def __init__(self, goal_c2ws, paths, pruned, n_actions, keep, actions, map_xz, c2w_xz, w2c, finishes, reads):
        super().__init__(goal_c2ws, [np.zeros((0, 2), np.int64)] * len(paths), n_actions, keep, actions, map_xz, c2w_xz, w2c, finishes, reads)
        self.paths, self.pruned = paths, pruned
        self.paths_arr = [pruned[k] for k in self.kept_index]


class PathPlanOps:
    """Mixin with the action-planning stage: `setup_start` + `planning` (astar.py:449-538, 1591-1777) and the batched `plan_paths`.

    The reference searches best-first on the host, once per goal.  Here `setup_start` builds ONE cost field from the start on the
    device (fisher_occ.h: fr_plan_grid, fr_occ_freespace, fr_plan_tiers, fr_plan_field) and every goal's path is read off it
    (fr_plan_paths): the minimum of the reference's own cost, distance + collision, with no expansion cap -- never above what the
    reference's search pays for the same cell.  Needs OccupancyOps' internals and the attributes
    occ_map, cam_height, grid_dim; `shortcut_path` defaults to True.  The reference's `planning_direction` array is not maintained
    (`plan_field()` gives cost and parent), and no PNG is written."""

    PLAN_MAX_LEN = 1024            # path points per goal of the first fr_plan_paths call; a longer path repeats the call

    @staticmethod
    def _localization_error(cls):
        """the LocalizationError of the module that defines `cls` (defined there when the module has none)"""
        import sys
        mod = sys.modules.get(cls.__module__)
        err = getattr(mod, "LocalizationError", None)
        if err is None:
            err = type("LocalizationError", (Exception,), {"__module__": cls.__module__})
            if mod is not None:
                mod.LocalizationError = err
        return err

    def _plan_cell(self, cell):
        return int(cell[0]), int(cell[1])

    # -- astar.py:449-538 --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def setup_start(self, start, gaussian_points=None, frame_idx=0):
        """ Setup the start point for the planner: the planning grid, the free space, and the cost field from `start` = (row, col).
            This function should be called before the planning """
        lib = _lib.load()
        dev = self.occ_map.device
        cfg = self._occ_cfg()
        gh, gw = int(self.grid_dim[1]), int(self.grid_dim[0])
        need = lib.fr_plan_workspace_bytes(ctypes.byref(cfg))
        ws = getattr(self, "_plan_ws", None)
        if ws is None or ws.numel() < need or ws.device != dev:
            ws = torch.empty((need,), dtype=torch.uint8, device=dev)
            self._plan_ws = ws
        sy, sx = self._plan_cell(start)
        pts, n = None, 0
        if gaussian_points is not None:
            pts_t = gaussian_points.detach().to(dev).float().contiguous()
            pts, n = pts_t.data_ptr(), int(pts_t.shape[0])
        occ_plan = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
        tiers = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
        field = torch.empty((gh, gw), dtype=torch.int64, device=dev)
        status = torch.empty((_lib.FR_PLAN_STATUS_WORDS,), dtype=torch.int32, device=dev)
        _lib.check(lib.fr_plan_grid(ctypes.byref(cfg), self.occ_map.data_ptr(), pts, n, float(self.cam_height), sy, sx, occ_plan.data_ptr(),
                                    status.data_ptr(), ws.data_ptr(), need, self._stream()), "fr_plan_grid")
        free = self.build_connected_freespace(gaussian_points, as_tensor=True)
        _lib.check(lib.fr_plan_tiers(ctypes.byref(cfg), free.data_ptr(), tiers.data_ptr(), self._stream()), "fr_plan_tiers")
        counts = (ctypes.c_int32 * 2)()
        _lib.check(lib.fr_plan_field(ctypes.byref(cfg), tiers.data_ptr(), sy, sx, field.data_ptr(), status.data_ptr(), ctypes.byref(counts),
                                     ws.data_ptr(), need, self._stream()), "fr_plan_field")
        self.start = start
        self._plan = dict(cfg=cfg, start=(sy, sx), occ_plan=occ_plan, free=free, tiers=tiers, field=field)
        self._plan_np = {}
        st = self._plan_read(status)                               # the one host read of the step beyond the convergence checks
        self.plan_stats = dict(ring=int(st[0]), gaussians_binned=int(st[1]), start_in_free_space=bool(st[2]), rounds=int(st[3]),
                               rounds_launched=int(counts[0]), convergence_reads=int(counts[1]))
        if st[0] >= 8:
            raise self._localization_error(type(self))("The start point is not in free space")

    @staticmethod
    def _plan_read(t):
        """every device-to-host copy of the stage goes through here"""
        return t.cpu().numpy()

    @property
    def occ_map_np(self):
        """the planning grid (uint8 [H, W]), copied down on first access"""
        if "occ" not in self._plan_np:
            self._plan_np["occ"] = self._plan_read(self._plan["occ_plan"])
        return self._plan_np["occ"]

    @occ_map_np.setter
    def occ_map_np(self, value):
        self.__dict__.setdefault("_plan_np", {})["occ"] = value

    @property
    def free_space_np(self):
        if "free" not in self._plan_np:
            self._plan_np["free"] = self._plan_read(self._plan["free"])
        return self._plan_np["free"]

    @free_space_np.setter
    def free_space_np(self, value):
        self.__dict__.setdefault("_plan_np", {})["free"] = value

    # -- astar.py:1591-1777 ------------------------------------------------------------------------------------------
    def plan_paths(self, goals):
        """[G, 2] goals (row, col) -> a list of G paths, each an (M, 2) int array in x-z order or np.array([]): one kernel call and
        one host read (a path longer than PLAN_MAX_LEN points repeats both once with room for any path)."""
        lib = _lib.load()
        plan = self._plan
        dev = plan["field"].device
        g = torch.as_tensor(np.asarray(goals, dtype=np.int64).reshape(-1, 2)).to(torch.int32)
        G = int(g.shape[0])
        if G == 0:
            return []
        g = g.to(dev).contiguous()
        shortcut = 1 if getattr(self, "shortcut_path", True) else 0
        max_len = int(self.PLAN_MAX_LEN)
        while True:
            out = torch.empty((G * (2 * max_len + 1),), dtype=torch.int32, device=dev)       # the lengths, then the paths: one copy down
            lengths, paths = out[:G], out[G:]
            _lib.check(lib.fr_plan_paths(ctypes.byref(plan["cfg"]), plan["field"].data_ptr(), plan["occ_plan"].data_ptr(), plan["start"][0],
                                         plan["start"][1], g.data_ptr(), G, shortcut, paths.data_ptr(), max_len, lengths.data_ptr(),
                                         self._stream()), "fr_plan_paths")
            host = self._plan_read(out)
            lens, pts = host[:G], host[G:].reshape(G, max_len, 2)
            if (lens >= 0).all():
                break
            max_len = int(self.grid_dim[0]) * int(self.grid_dim[1]) + 1
        return [pts[k, :lens[k]].astype(np.int64) if lens[k] > 0 else np.array([]) for k in range(G)]

    def planning(self, goal):
        """ the path to one goal (row, col): (M, 2) int array in x-z order, or np.array([]) """
        return self.plan_paths([self._plan_cell(goal)])[0]

    # -- astar.py:1372-1381 ------------------------------------------------------------------------------------------
    def _map_center_host(self):
        """map_center on the host, in its own dtype: the copy _occ_cfg holds until the tensor is replaced or written (no read per call)"""
        if isinstance(self.map_center, torch.Tensor):
            self._occ_cfg()
            return self._occ_mc_held[2]
        return np.asarray(self.map_center)

    def _plan_to_map(self, coord):
        """convert_to_map (astar.py:1372-1376) on the held copy of the map centre"""
        map_center = self._map_center_host()
        cam_pos_x = int((coord[0] - map_center[0]) / self.cell_size + self.grid_dim[0] // 2)
        cam_pos_z = int((coord[1] - map_center[1]) / self.cell_size + self.grid_dim[1] // 2)
        return np.array([cam_pos_x, cam_pos_z])

    def convert_to_map(self, coord):
        return self._plan_to_map(coord)

    def convert_to_world(self, coord):
        map_center = self._map_center_host()
        return (coord - np.asarray(self.grid_dim) / 2) * self.cell_size + map_center

    def _action_inputs(self, goal_c2ws, agent_c2w):
        """(the agent's pose float64 [4, 4], the goal poses [G, 4, 4], their cells int64 [G, 2] = (row, col)) as the tester makes them:
        convert_to_map(...)[[1, 0]], the goal's height replaced by the agent's; the agent must stand on the cost field's start cell"""
        plan = self._plan
        agent = np.array(agent_c2w.detach().cpu().numpy() if isinstance(agent_c2w, torch.Tensor) else agent_c2w)
        if agent.shape != (4, 4):
            raise ValueError(f"agent_c2w must be 4 x 4, got {agent.shape}")
        goal_np = goal_c2ws.detach().cpu().numpy() if isinstance(goal_c2ws, torch.Tensor) else np.asarray(goal_c2ws)
        goal_np = goal_np.reshape(-1, 4, 4) if goal_np.size else np.zeros((0, 4, 4), np.float32)
        current_agent_pos = agent[:3, 3]
        start = self._plan_to_map(current_agent_pos[[0, 2]])[[1, 0]]
        if self._plan_cell(start) != plan["start"]:
            raise ValueError(f"the agent stands on cell {self._plan_cell(start)}, the cost field was set up from {plan['start']}: run setup_start first")
        G = int(goal_np.shape[0])
        finishes = np.zeros((G, 2), np.int64)
        for k, pose_np in enumerate(goal_np):
            pos_np = pose_np[:3, 3].copy()
            pos_np[1] = current_agent_pos[1]
            finishes[k] = self._plan_to_map(pos_np[[0, 2]])[[1, 0]]
        return agent, goal_np, finishes

    # -- tester_gaussians_navigation.py:2227-2330 --------------------------------------------------------------------
    @torch.no_grad()
    def plan_actions(self, goal_c2ws, agent_c2w, *, forward_step_size, turn_angle, queue_size, cam_height=None):
        """The loop of NavTester.action_planning after `setup_start`: [G, 4, 4] goal poses and the agent's pose -> an ActionPlan.
        Goals and start become cells on the host as the tester makes them (convert_to_map(...)[[1, 0]], the goal's height replaced by the
        agent's); fr_plan_paths and fr_plan_actions run back to back on the device; ONE host read brings lengths, paths, action
        counts, keep flags, actions, cells and x-z positions over (a path longer than PLAN_MAX_LEN points repeats the calls and the
        read once, as plan_paths does).  The poses' inverses stay on the device (ActionPlan.w2c)."""
        lib = _lib.load()
        plan = self._plan
        dev = plan["field"].device
        Q = int(queue_size)
        if not 1 <= Q <= _lib.FR_ACTION_MAX_QUEUE:
            raise ValueError(f"queue_size must be 1 .. {_lib.FR_ACTION_MAX_QUEUE}, got {queue_size}")
        if not (float(forward_step_size) > 0 and float(turn_angle) > 0):
            raise ValueError("forward_step_size and turn_angle must be positive")
        agent, goal_np, finishes = self._action_inputs(goal_c2ws, agent_c2w)
        G = int(goal_np.shape[0])
        height = float(self.cam_height if cam_height is None else cam_height)
        if G == 0:
            return ActionPlan(goal_np, [], np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros((0, Q), np.uint8), np.zeros((0, Q, 2), np.int32),
                              np.zeros((0, Q, 2)), torch.zeros((0, Q, 4, 4), dtype=torch.float32, device=dev), finishes, reads=0)
        if np.abs(finishes).max() >= 2 ** 31:
            raise ValueError("a goal lies too far outside the map for a 32-bit cell")
        g = torch.from_numpy(finishes.astype(np.int32)).to(dev)
        poses = torch.from_numpy(np.ascontiguousarray(goal_np, np.float32).reshape(G, 16)).to(dev)
        agent_a = (ctypes.c_double * 16)(*[float(v) for v in agent.reshape(-1)])
        w2c = torch.empty((G, Q, 4, 4), dtype=torch.float32, device=dev)
        shortcut = 1 if getattr(self, "shortcut_path", True) else 0
        max_len = int(self.PLAN_MAX_LEN)
        reads = 0
        while True:
            # one buffer, one copy down: [c2w_xz f64 | lengths, paths, n_actions, map_xz i32 | keep, actions u8], each part 8-byte aligned
            sizes = (16 * G * Q, 4 * G, 8 * G * max_len, 4 * G, 8 * G * Q, G, G * Q)
            offs = np.concatenate([[0], np.cumsum([(s + 7) & ~7 for s in sizes])])
            out = torch.empty((int(offs[-1]),), dtype=torch.uint8, device=dev)
            part = [out[int(o):int(o) + s] for o, s in zip(offs[:-1], sizes)]
            ptr = [p.data_ptr() for p in part]
            _lib.check(lib.fr_plan_paths(ctypes.byref(plan["cfg"]), plan["field"].data_ptr(), plan["occ_plan"].data_ptr(), plan["start"][0],
                                         plan["start"][1], g.data_ptr(), G, shortcut, ptr[2], max_len, ptr[1], self._stream()), "fr_plan_paths")
            _lib.check(lib.fr_plan_actions(ctypes.byref(plan["cfg"]), ptr[2], max_len, ptr[1], g.data_ptr(), poses.data_ptr(), G, agent_a, height,
                                           float(forward_step_size), float(turn_angle), Q, float(self.cell_size), ptr[6], ptr[3], ptr[5],
                                           w2c.data_ptr(), ptr[0], ptr[4], self._stream()), "fr_plan_actions")
            host = self._plan_read(out)
            reads += 1
            h = [host[int(o):int(o) + s] for o, s in zip(offs[:-1], sizes)]
            lens = h[1].view(np.int32)
            if (lens >= 0).all():
                break
            max_len = int(self.grid_dim[0]) * int(self.grid_dim[1]) + 1
        pts = h[2].view(np.int32).reshape(G, max_len, 2)
        paths = [pts[k, :lens[k]].astype(np.int64) if lens[k] > 0 else np.array([]) for k in range(G)]
        return ActionPlan(goal_np, paths, h[3].view(np.int32).copy(), h[5].copy(), h[6].reshape(G, Q).copy(), h[4].view(np.int32).reshape(G, Q, 2).copy(),
                          h[0].view(np.float64).reshape(G, Q, 2).copy(), w2c, finishes, reads=reads)

    # -- tester_gaussians_navigation.py:2385-2496 --------------------------------------------------------------------
    @torch.no_grad()
    def plan_actions_object(self, goal_c2ws, agent_c2w, *, forward_step_size, turn_angle, cam_height=None):
        """The loop of NavTester.action_planning_object_adv after `setup_start`: [G, 4, 4] goal poses and the agent's pose -> an
        ObjectActionPlan (Q = FR_ACTION_OBJECT_MAX = 200; the planning queue does not cut these lists).  fr_plan_paths and
        fr_plan_actions_object run back to back on the device; ONE host read brings lengths, paths, pruned paths, action counts, keep
        flags, actions, cells and x-z positions over (a path longer than PLAN_MAX_LEN points repeats the calls and the read once, as
        plan_actions does).  The poses' inverses stay on the device (ObjectActionPlan.w2c)."""
        lib = _lib.load()
        plan = self._plan
        dev = plan["field"].device
        Q = _lib.FR_ACTION_OBJECT_MAX
        if not (float(forward_step_size) > 0 and float(turn_angle) > 0):
            raise ValueError("forward_step_size and turn_angle must be positive")
        agent, goal_np, finishes = self._action_inputs(goal_c2ws, agent_c2w)
        G = int(goal_np.shape[0])
        height = float(self.cam_height if cam_height is None else cam_height)
        if G == 0:
            return ObjectActionPlan(goal_np, [], [], np.zeros(0, np.int32), np.zeros(0, np.uint8), np.zeros((0, Q), np.uint8), np.zeros((0, Q, 2), np.int32),
                                    np.zeros((0, Q, 2)), torch.zeros((0, Q, 4, 4), dtype=torch.float32, device=dev), finishes, reads=0)
        if np.abs(finishes).max() >= 2 ** 31:
            raise ValueError("a goal lies too far outside the map for a 32-bit cell")
        g = torch.from_numpy(finishes.astype(np.int32)).to(dev)
        poses = torch.from_numpy(np.ascontiguousarray(goal_np, np.float32).reshape(G, 16)).to(dev)
        agent_a = (ctypes.c_double * 16)(*[float(v) for v in agent.reshape(-1)])
        w2c = torch.empty((G, Q, 4, 4), dtype=torch.float32, device=dev)
        shortcut = 1 if getattr(self, "shortcut_path", True) else 0
        max_len = int(self.PLAN_MAX_LEN)
        reads = 0
        while True:
            # one buffer, one copy down: [c2w_xz f64 | lengths, paths, n_actions, map_xz, pruned, pruned_len i32 | keep, actions u8], each part 8-byte aligned
            sizes = (16 * G * Q, 4 * G, 8 * G * max_len, 4 * G, 8 * G * Q, 8 * G * (max_len + 1), 4 * G, G, G * Q)
            offs = np.concatenate([[0], np.cumsum([(s + 7) & ~7 for s in sizes])])
            out = torch.empty((int(offs[-1]),), dtype=torch.uint8, device=dev)
            ptr = [out[int(o):int(o) + s].data_ptr() for o, s in zip(offs[:-1], sizes)]
            _lib.check(lib.fr_plan_paths(ctypes.byref(plan["cfg"]), plan["field"].data_ptr(), plan["occ_plan"].data_ptr(), plan["start"][0],
                                         plan["start"][1], g.data_ptr(), G, shortcut, ptr[2], max_len, ptr[1], self._stream()), "fr_plan_paths")
            _lib.check(lib.fr_plan_actions_object(ctypes.byref(plan["cfg"]), ptr[2], max_len, ptr[1], g.data_ptr(), poses.data_ptr(), G, agent_a, height,
                                                  float(forward_step_size), float(turn_angle), float(self.cell_size), ptr[8], ptr[3], ptr[7],
                                                  w2c.data_ptr(), ptr[0], ptr[4], ptr[5], ptr[6], self._stream()), "fr_plan_actions_object")
            host = self._plan_read(out)
            reads += 1
            h = [host[int(o):int(o) + s] for o, s in zip(offs[:-1], sizes)]
            lens = h[1].view(np.int32)
            if (lens >= 0).all():
                break
            max_len = int(self.grid_dim[0]) * int(self.grid_dim[1]) + 1
        pts = h[2].view(np.int32).reshape(G, max_len, 2)
        paths = [pts[k, :lens[k]].astype(np.int64) if lens[k] > 0 else np.array([]) for k in range(G)]
        pruned_len = h[6].view(np.int32)
        pr = h[5].view(np.int32).reshape(G, max_len + 1, 2)
        pruned = [pr[k, :pruned_len[k]].copy() if pruned_len[k] > 0 else np.zeros((0, 2), np.int32) for k in range(G)]
        return ObjectActionPlan(goal_np, paths, pruned, h[3].view(np.int32).copy(), h[7].copy(), h[8].reshape(G, Q).copy(),
                                h[4].view(np.int32).reshape(G, Q, 2).copy(), h[0].view(np.float64).reshape(G, Q, 2).copy(), w2c, finishes, reads=reads)

    def plan_field(self):
        """(cost float32 [H, W], -1 where the start does not reach; parent int32 [H, W, 2] = (row, col), -1 there)"""
        words = self._plan_read(self._plan["field"]).view(np.uint64)
        reached = words != np.uint64(_lib.FR_PLAN_UNREACHED)
        cost = np.where(reached, (words >> np.uint64(32)).astype(np.uint32).view(np.float32), np.float32(-1))
        idx = (words & np.uint64(0xFFFFFFFF)).astype(np.int64)
        gw = int(self.grid_dim[0])
        parent = np.where(reached[..., None], np.stack([idx // gw, idx % gw], axis=-1), -1).astype(np.int32)
        return cost, parent

    @classmethod
    def install(cls, planner_cls):
        """Graft the planning stage onto the reference's AstarPlanner class (after OccupancyOps.install, whose internals it uses)."""
        for name in ("setup_start", "planning", "plan_paths", "plan_actions", "plan_actions_object", "_action_inputs", "plan_field", "_plan_cell", "_plan_to_map", "_map_center_host", "_plan_read", "_localization_error",
                     "occ_map_np", "free_space_np", "PLAN_MAX_LEN"):
            setattr(planner_cls, name, cls.__dict__[name])
        for name in ("convert_to_map", "convert_to_world"):                     # the reference class has its own
            if not hasattr(planner_cls, name):
                setattr(planner_cls, name, cls.__dict__[name])
        cls._localization_error(planner_cls)
        return planner_cls


class GoalSelectOps:
    """Mixin with goal selection: `global_planning` (astar.py:843-1000) and the object round's `build_object_frontiers` (686-734),
    `generate_candidate_adv_object` (1471-1588) and `global_object_planning` (1151-1346), built from the library's stages.  Needs
    OccupancyOps' methods and, beyond its attributes, K_object, radius_object, min_range_object, centering, add_random_gaussians.

    What differs from the reference: `visualize` is accepted and writes NOTHING -- no PNG; cv2 and
    matplotlib are not imported.  The "vlm" frontier method raises, as build_frontiers does.  The candidates' draws come from the
    counter-based generator (`candidate_seed` / torch.manual_seed), not from torch.rand / torch.randint.  The widening loop
    `while len(candidate_pose) == 0` ends with an error after MAX_WIDENINGS rounds instead of spinning for ever."""

    TOPK = 20                      # astar.py:992, 1338
    MAX_WIDENINGS = 64             # the radius has grown by 1.5 ** 64 by then
    GAUSSIAN_PER_GRID = 200        # astar.py:1353

    # -- astar.py:686-734 ----------------------------------------------------------------------------------------------
    def build_object_frontiers(self, gaussian_points, use_convex_hull=True):
        """The centres (world x-z, float64 [N, 2], np.where order) of the map cells that hold more than 3 of the object's Gaussians,
        or None.  One launch chain (fr_occ_object_cells) in place of torch.unique over the cloud; the cells and their count also stay
        on the device (`_object_cells_dev`) for generate_candidate_adv_object.  A Gaussian with a non-finite x or z is not counted.
        use_convex_hull is accepted and unused, as in the reference."""
        self._object_cells_dev = None
        if gaussian_points is None or gaussian_points.numel() == 0:
            return None
        lib = _lib.load()
        dev = self.occ_map.device
        pts = gaussian_points.detach().to(dev).float().contiguous()
        cfg = self._occ_cfg()
        ws, need = self._occ_workspace(cfg)
        gw, gh = int(self.grid_dim[0]), int(self.grid_dim[1])
        max_cells = gw * gh
        cells = torch.empty((max_cells, 2), dtype=torch.int32, device=dev)
        counts = torch.empty((2,), dtype=torch.int32, device=dev)
        _lib.check(lib.fr_occ_object_cells(ctypes.byref(cfg), pts.data_ptr(), int(pts.shape[0]), 3, cells.data_ptr(), max_cells, counts.data_ptr(),
                                           ws.data_ptr(), need, self._stream()), "fr_occ_object_cells")
        n = int(counts.cpu()[0])
        if n == 0:
            return None
        self._object_cells_dev = (cells, counts, n)
        map_center = self.map_center.cpu().numpy() if torch.is_tensor(self.map_center) else np.asarray(self.map_center)
        select_pixels = cells[:n].cpu().numpy().astype(np.int64)                    # (col, row) in np.where order
        return (select_pixels - np.array([[gw // 2, gh // 2]])) * float(self.cell_size) + map_center[None, :]

    # -- astar.py:1471-1588 ----------------------------------------------------------------------------------------------
    @staticmethod
    def _n_theta(theta_step_deg):
        """max(1, round(2 pi / deg2rad(step))) as the reference takes it: in binary32, round half to even"""
        step_rad = np.deg2rad(np.float32(theta_step_deg))
        if not (np.isfinite(step_rad) and step_rad > 0):
            raise ValueError(f"theta_step_deg must be positive and finite, got {theta_step_deg}")
        return max(1, int(np.round(np.float32(2 * math.pi) / step_rad)))

    def _grid_candidates(self, center_point, expansion=1, theta_step_deg=15.0, radial_bins=6, radial_spacing="linear", eroded=None, min_free=40,
                         seed=None, cells_dev=None):
        """K_object poses on the ordered grid of rings and angles (fr_occ_grid_candidates): ([K, 4, 4] c2w, [K] bool keep).  The
        centres are the (x, z) rows of center_point, or -- cells_dev = (cells, counts, n) of build_object_frontiers -- the object
        cells on the device, with no host copy in between."""
        lib = _lib.load()
        dev = self.occ_map.device
        K = int(self.K_object)
        c2w = torch.empty((K, 4, 4), dtype=torch.float32, device=dev)
        keep = torch.empty((K,), dtype=torch.uint8, device=dev)
        cfg = self._occ_cfg()
        seed = self._next_seed() if seed is None else int(seed) & 0xFFFFFFFF
        self.last_candidate_seed = seed
        if cells_dev is not None:
            centers, n_centers, cells, n_dev = None, int(cells_dev[0].shape[0]), cells_dev[0].data_ptr(), cells_dev[1].data_ptr()
        else:
            held = center_point.detach().to(dev).float()[:, :2].contiguous()
            centers, n_centers, cells, n_dev = held.data_ptr(), int(held.shape[0]), None, None
        _lib.check(lib.fr_occ_grid_candidates(ctypes.byref(cfg), centers, n_centers, cells, n_dev, K, float(self.min_range_object),
                                              float(self.radius_object * expansion), self._n_theta(theta_step_deg), max(1, int(radial_bins)),
                                              1 if radial_spacing == "sqrt_area" else 0, float(self.cam_height), seed,
                                              None if eroded is None else eroded.data_ptr(), int(min_free), c2w.data_ptr(), keep.data_ptr(),
                                              self._stream()), "fr_occ_grid_candidates")
        return c2w, keep.bool()

    def generate_candidate_adv_object(self, center_point: torch.Tensor, expansion: float = 1, mode: str = "random", theta_step_deg: float = 15.0,
                                      radial_bins: int = 6, radial_spacing: str = "linear", seed=None):
        """ Sample camera poses around the (one or more) center points: (K_object, 4, 4).
        mode="random": the random ring (fr_occ_ring_candidates); mode="sorted": the ordered grid (fr_occ_grid_candidates) """
        if mode.lower() == "random":
            return self._ring_candidates(center_point, self.K_object, self.min_range_object, self.radius_object * expansion, seed=seed)[0]
        if mode.lower() == "sorted":
            return self._grid_candidates(center_point, expansion, theta_step_deg, radial_bins, radial_spacing, seed=seed)[0]
        raise ValueError("mode must be 'random' or 'sorted'")

    # -- astar.py:839-841, 1348-1370 ---------------------------------------------------------------------------------------
    def pose_eval(self, poses, *args):
        return torch.ones((poses.shape[0],)), poses

    def generate_random_gaussians(self, candidate_pos):
        """ Generate Random Gaussians from candidate positions: the reference's distribution, drawn by torch on the device """
        if candidate_pos is None:
            return None
        dev = self.occ_map.device
        position = torch.as_tensor(np.asarray(candidate_pos)).float().to(dev)
        n, per = position.shape[0], self.GAUSSIAN_PER_GRID
        xz_offset = torch.rand((1, per, 2), device=dev) * self.cell_size
        y_offset = (self.cam_height - 1.0) + torch.rand((n, per, 1), device=dev)
        new_p3t = torch.cat([position[:, None, :] + xz_offset, y_offset], dim=-1).reshape(-1, 3)[:, [0, 2, 1]]          # x-y-z order
        m = new_p3t.shape[0]
        new_rotations = torch.zeros((m, 4), device=dev)
        new_rotations[:, 0] = 1.
        return dict(means3D=new_p3t, scales=torch.rand((m, 3), device=dev).clamp_(min=1e-3) * self.cell_size * 0.05, rotations=new_rotations,
                    opacity=torch.rand((m, 1), device=dev).clamp_(min=1e-3), shs=torch.rand((m, 1, 3), device=dev))

    # -- the shared second half of global_planning / global_object_planning ----------------------------------------------------
    def _select_goals(self, candidate_pos, use_frontier, sample, agent_pose, free_space, expansion, evaluate):
        """candidate centres -> poses in the eroded free space (widening by x 1.5 while none is left), the random poses when there is no
        frontier, the evaluation, the top 20.  sample(centres, expansion, eroded) -> (c2w, keep): the filter rides in the launch."""
        dev = self.occ_map.device
        candidate_pose = []
        if candidate_pos is not None:
            if isinstance(candidate_pos, np.ndarray):
                candidate_pos = torch.from_numpy(candidate_pos).to(dev)
            if getattr(self, "centering", False):
                candidate_pos = torch.mean(candidate_pos, dim=0, keepdim=True)
            eroded = self._eroded_free(None, 10)                     # the free space build_frontiers just left on the device
            widenings = 0
            while len(candidate_pose) == 0:
                if widenings == self.MAX_WIDENINGS:
                    raise RuntimeError(f"no candidate pose in the free space after {widenings} widenings of the sampling radius")
                c2w, keep = sample(candidate_pos, expansion, eroded)
                candidate_pose = c2w[keep]
                expansion *= 1.5
                widenings += 1
            self.last_widenings = widenings
        if not use_frontier:
            random_pose = self.sample_random_candidate(agent_pose, free_space, sample_range=2 * expansion, sample_size=int(400 * expansion))
            candidate_pose = random_pose if len(candidate_pose) == 0 else torch.cat([candidate_pose, random_pose], dim=0)
        scores, poses = evaluate(candidate_pose)
        sort_index = torch.argsort(scores, descending=True)
        poses = poses[sort_index[:self.TOPK].to(poses.device)]
        scores = scores[sort_index[:self.TOPK]]
        self.previous_candidates = poses
        return poses, scores, candidate_pos

    # -- astar.py:843-1000 -----------------------------------------------------------------------------------------------
    def global_planning(self, pose_evaluation_fn=None, gaussian_points=None, goal_proposal_fn=None, expansion=1, visualize=True, agent_pose=None,
                        last_goal=None, slam=None):
        """ Global Planning for next target goal: (poses [<= 20, 4, 4], scores, random_gaussian_params), or (None, None, None) in frontier
        mode without a frontier.  visualize writes nothing; last_goal and slam are accepted and unused (the VLM frontier raises). """
        if self.frontier_select_method == "vlm":
            raise ValueError("frontier_select_method 'vlm' is not rebuilt (the VLM selection stays reference Python)")
        candidate_pos, free_space = self.build_frontiers(gaussian_points)
        use_frontier = candidate_pos is not None
        if pose_evaluation_fn is None and not use_frontier:
            return None, None, None
        random_gaussian_params = self.generate_random_gaussians(candidate_pos) if getattr(self, "add_random_gaussians", False) else None
        if candidate_pos is None and goal_proposal_fn is not None:
            candidate_pos = goal_proposal_fn(self.K, self.cam_height)

        def sample(centres, expansion, eroded):
            return self._ring_candidates(centres, self.K, self.min_range, self.radius * expansion, eroded, 40)

        def evaluate(candidate_pose):
            return self.pose_eval(candidate_pose) if pose_evaluation_fn is None else pose_evaluation_fn(candidate_pose, random_gaussian_params)

        poses, scores, _ = self._select_goals(candidate_pos, use_frontier, sample, agent_pose, free_space, expansion, evaluate)
        return poses, scores, random_gaussian_params

    # -- astar.py:1151-1346 ----------------------------------------------------------------------------------------------
    def global_object_planning(self, pose_evaluation_fn=None, gaussian_points=None, gaussian_points_scene=None, goal_proposal_fn=None, expansion=1,
                               visualize=True, agent_pose=None, criterion=None):
        """ Global Planning for next target goal around the object: (poses [<= 20, 4, 4], scores, None, the candidate centres), or
        (None, None, None) in frontier mode without object cells.  The third value is None whatever add_random_gaussians says: the
        reference makes the random Gaussians and discards them (astar.py:1182), and so does this.  Without centering the object cells
        go from fr_occ_object_cells to fr_occ_grid_candidates on the device. """
        if self.frontier_select_method == "vlm":
            raise ValueError("frontier_select_method 'vlm' is not rebuilt (the VLM selection stays reference Python)")
        _, free_space = self.build_frontiers(gaussian_points_scene)
        candidate_obj_pos = self.build_object_frontiers(gaussian_points)
        use_frontier = candidate_obj_pos is not None
        if pose_evaluation_fn is None and not use_frontier:
            return None, None, None
        if getattr(self, "add_random_gaussians", False):
            self.generate_random_gaussians(candidate_obj_pos)
        random_gaussian_params = None
        cells_dev = self._object_cells_dev if use_frontier and not getattr(self, "centering", False) else None
        if candidate_obj_pos is None and goal_proposal_fn is not None:
            candidate_obj_pos = goal_proposal_fn(self.K_object, self.cam_height)

        def sample(centres, expansion, eroded):
            return self._grid_candidates(centres, expansion, eroded=eroded, min_free=40, cells_dev=cells_dev)

        def evaluate(candidate_pose):
            if pose_evaluation_fn is None:
                return self.pose_eval(candidate_pose)
            return pose_evaluation_fn(candidate_pose, random_gaussian_params, criterion=criterion)

        poses, scores, candidate_obj_pos = self._select_goals(candidate_obj_pos, use_frontier, sample, agent_pose, free_space, expansion, evaluate)
        return poses, scores, random_gaussian_params, candidate_obj_pos

    @classmethod
    def install(cls, planner_cls):
        """Graft goal selection onto the reference's AstarPlanner class (after OccupancyOps.install, whose methods it uses)."""
        for name in ("build_object_frontiers", "generate_candidate_adv_object", "global_planning", "global_object_planning", "generate_random_gaussians",
                     "_grid_candidates", "_n_theta", "_select_goals", "TOPK", "MAX_WIDENINGS", "GAUSSIAN_PER_GRID"):
            setattr(planner_cls, name, cls.__dict__[name])
        if not hasattr(planner_cls, "pose_eval"):
            planner_cls.pose_eval = cls.__dict__["pose_eval"]
        return planner_cls


class LocalizationError(Exception):
    """raised by setup_start when all 8 neighbours of the start are occupied in the dilated map (astar.py:481-482)"""


class AstarPlanner(OccupancyOps, PathPlanOps, GoalSelectOps):
    """Standalone object with the reference constructor's configuration keys (astar.py:23-60)."""

    def __init__(self, slam_config=None, eval_dir=None, device=torch.device("cuda:0"), **kw):
        cfg = slam_config or {}
        ex, pol = cfg.get("explore", {}), cfg.get("policy", {})
        self.device = torch.device(device)
        self.cell_size = kw.get("cell_size", ex.get("cell_size", 0.05))
        self.height_upper = kw.get("height_upper", pol.get("height_upper", 0.6))
        self.height_lower = kw.get("height_lower", pol.get("height_lower", -0.6))
        self.K = kw.get("sample_view_num", ex.get("sample_view_num", 64))
        self.radius = kw.get("sample_range", ex.get("sample_range", 1.0))
        self.min_range = kw.get("min_range", ex.get("min_range", 0.2))
        self.K_object = kw.get("sample_view_num_object", ex.get("sample_view_num_object", self.K))
        self.radius_object = kw.get("sample_range_object", ex.get("sample_range_object", self.radius))
        self.min_range_object = kw.get("min_range_object", ex.get("min_range_object", self.min_range))
        self.frontier_select_method = kw.get("frontier_select_method", ex.get("frontier_select_method", "combined"))
        self.pcd_far_distance = kw.get("pcd_far_distance", pol.get("pcd_far_distance", 10.0))
        self.eval_dir = eval_dir
        self.cam_pos = None
        self.frame_idx = 0
        self.shortcut_path = kw.get("shortcut_path", ex.get("shortcut_path", True))
        self.centering = kw.get("centering", ex.get("centering", False))
        self.add_random_gaussians = kw.get("add_random_gaussians", ex.get("add_random_gaussians", False))
        self.previous_candidates = None
