"""Cases of the running reconstruction metrics (CloudIndex.fold, the masked depth source, ReconTracker): how a target cloud of
tests/cloud_cases.py is cut into frames, an object scene seen from a ring of cameras, the reference's chain for a frame's points in
NumPy float64 (tester_gaussians_navigation.py:511-529 and 1221), and the g++ harness over csrc/fr_cloud_math.h and the public header
(tests/harness/fr_recon_harness.cpp).  The families, the SciPy float64 statement and the qualification rule are cloud_cases'."""
import ctypes
import functools

import numpy as np

import cloud_cases as cc
import harness_build

F = np.float32
FOLD_FAMILIES = ("uniform", "clusters", "surface", "nonfinite")
FOLD_N = (1, 64, 65, 1025, 5000)
FOLD_K = (1, 2, 5)
FOLD_M = (1, 64, 65, 257, 1000)
CFG_FIELDS = ("source", "M", "H", "W", "stride", "flip_z", "dist_th", "queries", "depth", "kinv", "c2w", "out_dist", "out_idx", "out_flag",
              "out_stats", "seed_d2", "mask", "flag_near", "out_points")
NEW_FIELDS = CFG_FIELDS[CFG_FIELDS.index("out_stats") + 1:]


# ---- the harness ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def build_harness():
    h = ctypes.CDLL(harness_build.shared("fr_recon_harness"))
    vp, f32, ci = ctypes.c_void_p, ctypes.c_float, ctypes.c_int
    h.frc_r_fold.argtypes, h.frc_r_fold.restype = [f32, f32], f32
    h.frc_r_fold_may_improve.argtypes, h.frc_r_fold_may_improve.restype = [f32, f32], ci
    h.frc_r_sample_is_query.argtypes, h.frc_r_sample_is_query.restype = [f32, ci, ci], ci
    h.frc_r_fold_cloud.argtypes, h.frc_r_fold_cloud.restype = [ci, vp, ci, vp, vp], None
    h.frc_r_depth_points.argtypes, h.frc_r_depth_points.restype = [ci] * 4 + [vp] * 6, None
    h.frc_r_cfg_layout.argtypes, h.frc_r_cfg_layout.restype = [vp], ci
    return h


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def cfg_layout(h):
    """(sizeof, {field: offset}) of fr_cloud_query_cfg as g++ lays the header's struct out"""
    out = np.zeros(64, np.uintp)
    n = h.frc_r_cfg_layout(_p(out))
    assert n == 1 + len(CFG_FIELDS)
    return int(out[0]), {f: int(o) for f, o in zip(CFG_FIELDS, out[1:n])}


def harness_fold(h, targets, queries, seed_d2):
    """the seeds after folding `targets` in (a copy)"""
    t, q = np.ascontiguousarray(targets, F).reshape(-1, 3), np.ascontiguousarray(queries, F).reshape(-1, 3)
    s = np.array(seed_d2, F)
    h.frc_r_fold_cloud(t.shape[0], _p(t), q.shape[0], _p(q), _p(s))
    return s


def harness_points(h, depth, mask, kinv, c2w, stride=1, flip_z=False):
    """out_points of the depth source: (points [Hs Ws, 3] with NaN rows, valid [Hs Ws] bool)"""
    H, W = depth.shape
    Hs, Ws = (H + stride - 1) // stride, (W + stride - 1) // stride
    depth, kinv, c2w = np.ascontiguousarray(depth, F), np.ascontiguousarray(kinv, F), np.ascontiguousarray(np.asarray(c2w)[:3, :4], F)
    mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    pts, valid = np.empty((Hs * Ws, 3), F), np.empty(Hs * Ws, np.uint8)
    h.frc_r_depth_points(H, W, stride, int(flip_z), _p(depth), _p(mask), _p(kinv), _p(c2w), _p(pts), _p(valid))
    return pts, valid.astype(bool)


# ---- a target cloud cut into frames ---------------------------------------------------------------------------------------------------

def cut(t, k):
    """`t` [N,3] as k frames whose concatenation is a permutation of t.  k = 2: two halves (N = 1 leaves one of them empty).
    k = 5: one frame is empty and, where t has non-finite rows, one frame holds those and nothing else; the finite rows go to the
    other frames in unequal parts."""
    t = np.ascontiguousarray(t, F)
    if k == 1:
        return [t]
    if k == 2:
        return [t[:len(t) // 2], t[len(t) // 2:]]
    assert k == 5
    bad = ~np.isfinite(t).all(1)
    if bad.any():
        good = t[~bad]
        a, b = len(good) // 7, len(good) // 2
        return [good[:a], t[:0], t[bad], good[a:b], good[b:]]
    a, b, c = len(t) // 7, len(t) // 3, (2 * len(t)) // 3
    return [t[:a], t[:0], t[a:b], t[b:c], t[c:]]


# ---- an object seen from a ring of cameras --------------------------------------------------------------------------------------------

OBJ_RADIUS = 0.5
HABITAT_TRANSFORM = np.diag([1.0, -1.0, -1.0, 1.0])              # tester_gaussians_navigation.py:86-91


def _look_at(eye, target):
    """camera-to-world of a camera at `eye` that looks along its +Z at `target` (x right, y down)"""
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, y, z, eye
    return c2w


def make_scene(n_gt, n_frames=5, H=48, W=64, seed=0):
    """A sphere of radius 0.5 m that stands at `object_pose` in the world; the ground truth is n_gt points of its surface in the
    evaluation frame (eval_transform applied to the object frame, as the reference's gt_obj_3d_rotated).  Every frame: a camera
    on a ring 1.6 to 2.2 m from the object, the depth of the sphere with +-3 mm of noise in front of a wall at 3 m, the object
    mask (the sphere's pixels, a rim of wall pixels the mask wrongly includes, a few of its pixels wrongly left out), and pixels
    without a depth inside and outside the mask.  dict(gt [n_gt,3] float32, frames: list of dict(depth, mask, intrinsics,
    camera_pose, object_pose)), eval_transform."""
    rng = np.random.default_rng([n_gt, n_frames, H, W, seed])
    v = rng.normal(size=(n_gt, 3))
    obj_pts = OBJ_RADIUS * v / np.linalg.norm(v, axis=1, keepdims=True)
    object_pose = cc._rigid(rng)
    gt = (np.c_[obj_pts, np.ones(n_gt)] @ HABITAT_TRANSFORM.T)[:, :3]
    centre = object_pose[:3, 3]
    fx = 60.0
    K = np.array([[fx, 0, W / 2 - 0.5], [0, fx, H / 2 - 0.5], [0, 0, 1]])
    vv, uu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    frames = []
    for f in range(n_frames):
        ang = 2 * np.pi * f / n_frames + rng.uniform(-0.2, 0.2)
        eye = centre + rng.uniform(1.6, 2.2) * np.array([np.cos(ang), rng.uniform(-0.3, 0.3), np.sin(ang)])
        camera_pose = _look_at(eye, centre + rng.uniform(-0.1, 0.1, 3))
        rays = np.stack([(uu - K[0, 2]) / fx, (vv - K[1, 2]) / fx, np.ones((H, W))], -1)          # z = 1: the ray parameter is the depth
        rw = rays @ camera_pose[:3, :3].T
        oc = eye - centre
        a, b, c = (rw * rw).sum(-1), 2 * (rw @ oc), oc @ oc - OBJ_RADIUS ** 2
        disc = b * b - 4 * a * c
        hit = disc > 0
        depth = np.full((H, W), 3.0)
        depth[hit] = ((-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a))[hit] + rng.uniform(-0.003, 0.003, int(hit.sum()))
        mask = hit.copy()
        mask[:, 1:] |= hit[:, :-1]                                  # a rim of wall pixels on one side
        mask &= rng.uniform(size=(H, W)) > 0.03                     # a few object pixels left out
        n_bad = H * W // 12
        depth.reshape(-1)[rng.integers(0, H * W, n_bad)] = np.array([0.0, -1.0, np.inf, np.nan])[rng.integers(0, 4, n_bad)]
        frames.append(dict(depth=depth.astype(F), mask=mask.astype(np.uint8) * 255, intrinsics=K.astype(F), camera_pose=camera_pose,
                           object_pose=object_pose))
    return dict(gt=gt.astype(F), frames=frames, eval_transform=HABITAT_TRANSFORM, seed=seed)


def frame_transform(scene, frame):
    """(kinv [3,3], cam_to_eval [4,4]) float32: eval_transform inv(object_pose) camera_pose composed in binary64, rounded once"""
    T = scene["eval_transform"] @ np.linalg.inv(frame["object_pose"]) @ frame["camera_pose"]
    return np.linalg.inv(frame["intrinsics"].astype(np.float64)).astype(F), T.astype(F)


def np_reference_points(scene, frame):
    """the reference's chain in float64: store_filtered_obj_pointcloud's points_obj (tester_gaussians_navigation.py:511-529) through
    apply_transform_to_pointcloud(..., habitat_transform) (1221), in the reference's pixel order (np.where: row-major).  A depth
    of +inf passes the reference's `depth > 0` and gives it a point that is not finite; the product leaves such a pixel out
    (frc_depth_valid), and so does this statement."""
    K, depth = frame["intrinsics"].astype(np.float64), frame["depth"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        valid = (frame["mask"] > 0) & (depth > 0) & np.isfinite(depth)
    ys, xs = np.where(valid)
    zs = depth[ys, xs]
    cam = np.stack([(xs - K[0, 2]) * zs / K[0, 0], (ys - K[1, 2]) * zs / K[1, 1], zs, np.ones_like(zs)], 1)
    world = (frame["camera_pose"] @ cam.T).T
    obj = (np.linalg.inv(frame["object_pose"]) @ world.T).T
    return (scene["eval_transform"] @ obj.T).T[:, :3], valid


def scene_points(h, scene, upto=None):
    """the finite points of the first `upto` frames as the product makes them (the harness's frc_back_project), concatenated"""
    out = [np.zeros((0, 3), F)]
    for fr in scene["frames"][:upto]:
        kinv, T = frame_transform(scene, fr)
        pts, valid = harness_points(h, fr["depth"], fr["mask"], kinv, T)
        out.append(pts[valid])
    return np.concatenate(out)


def qualifying_scene(h, n_gt, thresholds=cc.THRESHOLDS, **kw):
    """the first seed whose scene qualifies (cloud_cases.qualifies_points, both directions, after every frame) within MAX_SEEDS"""
    for seed in range(cc.MAX_SEEDS):
        s = make_scene(n_gt, seed=seed, **kw)
        if all(cc.qualifies_points(s["gt"], scene_points(h, s, k), thresholds) and cc.qualifies_points(scene_points(h, s, k), s["gt"], thresholds)
               for k in range(1, len(s["frames"]) + 1)):
            return s
    raise AssertionError(f"no qualifying seed for the object scene with {n_gt} ground-truth points")
