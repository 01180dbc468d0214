"""Shared camera cases for the tests: cameras that are NOT the unit camera of scenes.intrinsics (fx = W/2, fy = H/2, centred
principal point, hence tanfovx == tanfovy == 1), with scale modifiers other than 1 and a visible background.

A case is (name, W, H, K, scale_modifier, bg, view_w2c).  The three cameras of the real workloads, and a fourth for the early bound:
  narrow_wide  200 x 120, fx = 220, fy = 37.5: tanfov 0.4545 / 1.6, centred; both image sizes ragged in 16
  offcentre    160 x 96,  K = [[70, 0, 95], [0, 85, 30], [0, 0, 1]]: anisotropic, principal point far from the centre
  replica8     150 x 85,  fx = fy = 75, cx = 74.4375, cy = 41.9375: Replica's 1200 x 680 / fx = fy = 600 camera at one eighth
  tall         32 x 640,  fx = 40, fy = 160 (tanfov 0.4 / 2.0), centred: fy >> fx AND tanfovy >> tanfovx, the one combination in
               which the y terms carry the projection kernel's early radius bound (with the three cameras above a bound that takes
               x's clamp or x's focal length for y is still a valid bound, so no output can show it)
RASTER_CASES carry the yaw / translation pose of test_gpu_rasterizer_parity._pose as their view (the single-view rasteriser),
BATCHED_CASES the identity or the small rotation of test_gpu_view_identity.py (the view-batched entry points, whose poses arrive
as w2c beside the camera).

The scene builders spread the means over about 1.6 x the case's own frustum, per axis: visible splats then fall on both sides of
the 1.3 tanfov clamp of forward.cu:80-84 on both axes and straddle all four image borders (tests/test_camera_cases_cpu.py proves
it with the oracle alone)."""
from typing import NamedTuple

import numpy as np

BG = np.array([0.2, 0.5, 0.1], np.float32)
# the scenes of tests/test_gpu_cameras.py, whose properties tests/test_camera_cases_cpu.py proves: Gaussians, seed, mean scale
P_RASTER, SEED_RASTER = 4000, 1
P_BATCHED, SEED_BATCHED = 5000, 3
SCALE = 0.08
SCALE_BATCHED = 0.12
P_POSE = 300                      # pose_fisher_ref costs one backward per pixel group on the CPU: at most 500


class Case(NamedTuple):
    name: str
    W: int
    H: int
    K: tuple
    scale_modifier: float
    bg: np.ndarray
    view_w2c: np.ndarray

    @property
    def tanfov(self):
        return self.W / (2.0 * self.K[0][0]), self.H / (2.0 * self.K[1][1])


def pose(yaw=0.3, t=(0.2, -0.1, 0.3)):
    """test_gpu_rasterizer_parity._pose"""
    w2c = np.eye(4, dtype=np.float32)
    c, s = np.cos(yaw), np.sin(yaw)
    w2c[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    w2c[:3, 3] = t
    return w2c


def small_rotation():
    """the camera of test_gpu_view_identity.py::test_non_identity_camera_matches_oracle"""
    c, s = np.cos(0.08), np.sin(0.08)
    return np.array([[c, 0, s, 0.05], [0, 1, 0, -0.03], [-s, 0, c, 0.02], [0, 0, 0, 1]], np.float32)


CAMERAS = {
    "narrow_wide": (200, 120, ((220.0, 0.0, 100.0), (0.0, 37.5, 60.0), (0.0, 0.0, 1.0))),
    "offcentre": (160, 96, ((70.0, 0.0, 95.0), (0.0, 85.0, 30.0), (0.0, 0.0, 1.0))),
    "replica8": (150, 85, ((75.0, 0.0, 74.4375), (0.0, 75.0, 41.9375), (0.0, 0.0, 1.0))),
    "tall": (32, 640, ((40.0, 0.0, 16.0), (0.0, 160.0, 320.0), (0.0, 0.0, 1.0))),
}


def case(camera, mod, view, bg=BG, tag=None):
    W, H, K = CAMERAS[camera]
    name = f"{camera}-m{mod:g}" + (f"-{tag}" if tag else "")
    return Case(name, W, H, K, float(mod), np.asarray(bg, np.float32), np.asarray(view, np.float32))


def scaled(c, W, H):
    """The same camera at another image size: K scaled per axis (still anisotropic and off-centre)."""
    sx, sy = W / c.W, H / c.H
    K = ((c.K[0][0] * sx, 0.0, c.K[0][2] * sx), (0.0, c.K[1][1] * sy, c.K[1][2] * sy), (0.0, 0.0, 1.0))
    return c._replace(name=f"{c.name}-{W}x{H}", W=W, H=H, K=K)


# every camera with every modifier once over the two lists; the background is set everywhere but in one case of each list
RASTER_CASES = [case("narrow_wide", 1.7, pose()), case("offcentre", 0.4, pose(-0.2)), case("replica8", 1.0, pose(0.3, (0.1, 0.1, 0.2))),
                case("offcentre", 1.7, pose(0.15, (-0.2, 0.05, 0.1)), bg=np.zeros(3))]
BATCHED_CASES = [case("narrow_wide", 0.4, np.eye(4)), case("offcentre", 1.7, np.eye(4)), case("replica8", 1.7, np.eye(4), bg=np.zeros(3)),
                 case("offcentre", 1.0, small_rotation(), tag="rot"), case("narrow_wide", 1.7, small_rotation(), tag="rot"),
                 case("tall", 1.0, np.eye(4))]


# raster cases whose scene holds a tile list longer than 256, the shortest segment the chunked backward cuts lists into (the fourth,
# offcentre-m0.4, has small splats and a longest list of 133: there the chunked kernels run on lists of one segment)
CHUNKED_CASES = ["narrow_wide-m1.7", "replica8-m1", "offcentre-m1.7"]


# the pose Fisher test: 48 x 32 variants of an identity-view and a rotated case (its reference costs one backward per pixel group)
POSE_CASES = [scaled(BATCHED_CASES[1], 48, 32), scaled(BATCHED_CASES[4], 48, 32)]


# the fused pair test.  Every tile adds its partial sum of a Gaussian's screen-space gradients with a binary32 atomic add, in an order
# that differs from run to run, and the test's rule (test_fused_rgb_depth_silhouette_pair's: 1e-4, 1e-6 of the tensor's maximum) leaves
# little room for that: with depths from 0.3, where 96 splats of narrow_wide are wider than 64 px and collect a sum from each of the
# 104 tiles, two runs of the SAME separate backward differed by up to 0.67 of the rule in dL_dcov3D, and the comparison failed in
# one run of two.  Depths of 1 to 3 keep all but a handful of radii under 64 px (a visible splat behind narrow_wide's x clamp needs
# 30 px) and still leave more than 20 visible splats behind each clamp; the two blobs put more than 600 faint splats into tiles of
# the left and the top edge, so that the chunked backward cuts lists under these cameras.
PAIR_CASES = [case("offcentre", 0.4, pose()), case("narrow_wide", 0.4, pose())]
P_PAIR, SCALE_PAIR, Z_PAIR = 5000, 0.1, (1.0, 3.0)


def pair_scene(c):
    return frustum_scene(c, P_PAIR, SEED_RASTER, zmin=Z_PAIR[0], zmax=Z_PAIR[1], scale=SCALE_PAIR, clusters=2)


def by_name(cases):
    return {c.name: c for c in cases}


def ids(cases):
    return [c.name for c in cases]


def oracle_camera(oracle, c, view=None):
    """oracle.Camera of a case (modifier and background set); `view` overrides the case's own"""
    cam = oracle.setup_camera(c.W, c.H, c.K, c.view_w2c if view is None else view)
    return cam._replace(scale_modifier=c.scale_modifier, bg=c.bg.copy())


def device_camera(c, dev, view=None):
    """GaussianRasterizationSettings of a case on `dev`"""
    import torch
    from models.SLAM.utils.recon_helpers import setup_camera
    cam = setup_camera(c.W, c.H, c.K, c.view_w2c if view is None else view, device=dev)
    return cam._replace(scale_modifier=c.scale_modifier, bg=torch.from_numpy(c.bg.copy()).to(dev))


def frustum_window(c, factor=1.6):
    """(centre_x, half_x, centre_y, half_y) of x/z, y/z: the image's own window [-cx / fx, (W - cx) / fx] widened by `factor`"""
    fx, fy, cx, cy = c.K[0][0], c.K[1][1], c.K[0][2], c.K[1][2]
    return (0.5 * c.W - cx) / fx, factor * c.W / (2 * fx), (0.5 * c.H - cy) / fy, factor * c.H / (2 * fy)


def frustum_scene(c, P, seed, zmin=0.3, zmax=6.0, scale=0.05, opacity_mean=1.0, factor=1.6, first_w2c=None, clusters=0):
    """scenes.random_scene with the means uniform over `factor` x the case's frustum (in the frame of the case's view applied behind
    `first_w2c`, the identity by default), then taken back to world coordinates: what the case's camera sees (from the first pose)
    is the spread scene.
    clusters (0, 1 or 2): the last 600 splats each form a tight blob (radius 0.005 at depth 3, about one cell of the 1024^3 Z-curve
    grid; modified scales around 0.006) whose centre projects onto the image's left edge (the top edge for the second).  600 neighbours hold at least
    one whole round of 256 along a Z-curve, so the projection kernel's group test decides about a round that straddles the border on
    its two tight sides, with a bound small enough that a principal point or a view rotation left out of it shows."""
    from scenes import random_scene
    sc = random_scene(P, seed, zmin=zmin, zmax=zmax, spread=1.0, scale=scale, opacity_mean=opacity_mean)
    rng = np.random.default_rng(seed + 7919)
    z = sc["means3D"][:, 2].astype(np.float64)
    x0, hx, y0, hy = frustum_window(c, factor)
    m = np.stack([(x0 + rng.uniform(-hx, hx, P)) * z, (y0 + rng.uniform(-hy, hy, P)) * z, z], 1)
    fx, fy, cx, cy = c.K[0][0], c.K[1][1], c.K[0][2], c.K[1][2]
    for k in range(clusters):
        n, zc = 600, 3.0
        centre = np.array([(-0.5 - cx) / fx * zc, (0.5 * c.H - cy) / fy * zc, zc]) if k == 0 else \
            np.array([(0.5 * c.W - cx) / fx * zc, (-0.5 - cy) / fy * zc, zc])
        d = rng.normal(size=(n, 3))
        d *= (0.005 * rng.uniform(0, 1, (n, 1)) ** (1 / 3)) / np.linalg.norm(d, axis=1, keepdims=True)
        sl = slice(P - (k + 1) * n, P - k * n)
        m[sl] = centre + d
        sc["scales"][sl] *= np.float32(0.006 / (scale * c.scale_modifier))
        sc["opacities"][sl] *= np.float32(0.1)              # 600 splats on a few pixels: faint, so that the whole stack contributes
    full = c.view_w2c.astype(np.float64) @ (np.eye(4) if first_w2c is None else np.asarray(first_w2c, np.float64))
    inv = np.linalg.inv(full)
    sc["means3D"] = np.ascontiguousarray((m @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32))
    return sc


def batched_scene(c):
    """the world the view-batched GPU tests score under case c, with frustum_poses(c)"""
    return frustum_scene(c, P_BATCHED, SEED_BATCHED, scale=SCALE_BATCHED, first_w2c=frustum_poses(c, 1)[0], clusters=2)


def pose_scene(c):
    """the world of the pose Fisher test under a POSE_CASES case"""
    return frustum_scene(c, P_POSE, 11, zmin=0.5, zmax=3.0, scale=0.06, first_w2c=frustum_poses(c, 1)[0])


def pose_views(c):
    """its two views: the small motions among frustum_poses"""
    return frustum_poses(c, 4)[[0, 3]]


def raster_scene(c):
    """the scene the single-view GPU tests render under case c"""
    return frustum_scene(c, P_RASTER, SEED_RASTER, scale=SCALE)


def frustum_poses(c, V=3, zmax=6.0, factor=1.6):
    """[V,4,4] w2c for the view-batched entry points on a frustum_scene world: pose 0 a small yaw / translation
    (test_gpu_pose_fisher._yaw(1)), pose 1 in a far corner of the cloud looking back into it, pose 2 outside the cloud, beside it (as
    test_gpu_spatial_order.py::test_group_test_never_drops_a_survivor places two of its poses) and turned 1.3 half fields of view off
    it, so that most of the cloud lies beyond one side of the frustum -- there the early bound removes most splats and the group test
    whole rounds; the rest further small motions."""
    x0, hx, y0, hy = frustum_window(c, factor)

    def look(yaw, pos):
        c2w = np.eye(4)
        cs, sn = np.cos(yaw), np.sin(yaw)
        c2w[:3, :3] = np.array([[cs, 0, sn], [0, 1, 0], [-sn, 0, cs]])
        c2w[:3, 3] = pos
        return np.linalg.inv(c2w)
    corner = np.array([(x0 + 0.9 * hx) * zmax, (y0 + 0.5 * hy) * zmax, zmax])
    out = [pose(0.06, (0.04, -0.02, 0.03)).astype(np.float64),
           look(np.arctan2(-corner[0], -corner[2]) + 0.4, corner),        # towards the apex of the cloud, turned 0.4 rad off it
           look(-np.pi / 2 + 1.3 * np.arctan(0.5 * c.W / c.K[0][0]), ((x0 + hx) * zmax + 4.0, y0 * 3.0, 3.0))]
    for k in range(3, V):
        out.append(pose(-0.05 * k, (0.03 * k, 0.02 * k, -0.04 * k)).astype(np.float64))
    return np.stack(out[:V]).astype(np.float32)


# ---- what a scene exercises, from the oracle's forward alone ----------------------------------------------------------------
def clamp_counts(oracle, cam, means_cam, fwd):
    """(visible with |tx/tz| > 1.3 tanfovx, visible with |ty/tz| > 1.3 tanfovy): t = the view matrix applied to the means the
    forward was given (forward.cu:80-84)"""
    w2c = np.asarray(cam.viewmatrix, np.float32).reshape(4, 4).T
    t = oracle.transform_points(w2c, means_cam).astype(np.float64)
    vis = fwd["radii"] > 0
    with np.errstate(all="ignore"):
        cx = np.abs(t[:, 0] / t[:, 2]) > 1.3 * cam.tanfovx
        cy = np.abs(t[:, 1] / t[:, 2]) > 1.3 * cam.tanfovy
    return int((vis & cx).sum()), int((vis & cy).sum())


def border_counts(cam, fwd):
    """visible splats whose tile rectangle (auxiliary.h:46-58, getRect) touches the left, right, top, bottom border"""
    W, H = cam.image_width, cam.image_height
    gx, gy = (W + 15) // 16, (H + 15) // 16
    vis = fwd["radii"] > 0
    r = fwd["radii"][vis].astype(np.float32)
    p = fwd["means2D"][vis].astype(np.float32)
    # visible = the rectangle is not empty; it reaches the first / last tile column or row AND the radius crosses the image's edge
    x0 = np.clip(((p[:, 0] - r) / np.float32(16)).astype(np.int64), 0, gx)
    x1 = np.clip(((p[:, 0] + r + np.float32(15)) / np.float32(16)).astype(np.int64), 0, gx)
    y0 = np.clip(((p[:, 1] - r) / np.float32(16)).astype(np.int64), 0, gy)
    y1 = np.clip(((p[:, 1] + r + np.float32(15)) / np.float32(16)).astype(np.int64), 0, gy)
    return (int(((x0 == 0) & (p[:, 0] - r < 0)).sum()), int(((x1 == gx) & (p[:, 0] + r > W - 1)).sum()),
            int(((y0 == 0) & (p[:, 1] - r < 0)).sum()), int(((y1 == gy) & (p[:, 1] + r > H - 1)).sum()))
