"""CPU: the two conservative culls of the view-batched projection kernel (csrc/fisher_rast.hip, k_preprocess_views / _c), restated
in NumPy and held against the oracle's own radii.

  * the early frustum bound of phase A (per Gaussian): whenever the bound puts a splat outside the tile grid, the oracle (the
    restatement of forward.cu:155-256) must have given it radius 0 -- on needle-shaped splats with non-unit quaternions placed
    around the image edges, on the benchmark scene family, and under the cameras of tests/cameras.py (anisotropic focal lengths,
    off-centre principal point, a view matrix that is not the identity, scale modifiers other than 1);
  * the group test (per round of 256 Z-curve neighbours and view): four linear side inequalities and `behind` on the round's
    bounding sphere -- no round may be skipped while the oracle sees one of its splats.

Both are restated from the projection matrix, the view matrix and its norm factor `wn`, as the kernel reads them."""
import ctypes

import numpy as np
import pytest

import cameras as C
from scenes import intrinsics

f32 = np.float32


def _mats(cam):
    """(vm, pm): the 16 floats of the view and the projection matrix as the kernel indexes them (column-major)"""
    return np.asarray(cam.viewmatrix, f32).reshape(16), np.asarray(cam.projmatrix, f32).reshape(16)


def _wn(vm):
    """|W|_2^2 <= |W|_1 |W|_inf of the view matrix's 3 x 3"""
    a = np.abs(vm)
    c = max(a[0] + a[1] + a[2], a[4] + a[5] + a[6], a[8] + a[9] + a[10])
    r = max(a[0] + a[4] + a[8], a[1] + a[5] + a[9], a[2] + a[6] + a[10])
    return f32(c) * f32(r)


def _focal2(cam, vm):
    fx, fy = f32(cam.image_width / (f32(2.0) * f32(cam.tanfovx))), f32(cam.image_height / (f32(2.0) * f32(cam.tanfovy)))
    wn = _wn(vm)
    return f32(1.02) * wn * fx * fx, f32(1.02) * wn * fy * fy


def _bound_says_outside(po, tr, cam):
    """The kernel's arithmetic (float32) on the means `po` the camera's matrices are applied to (a view's camera-frame means) and
    the traces of the 3D covariances: lambda1 <= kc / z^2 * trace(cov3D) + 0.7, radius <= 3 sqrt(.) + 2, the pixel of the centre
    from the projection matrix."""
    W, H = cam.image_width, cam.image_height
    vm, pm = _mats(cam)
    x, y, z = (np.asarray(po)[:, k].astype(f32) for k in range(3))
    tr = np.asarray(tr, f32)
    lx, ly = f32(1.3) * f32(cam.tanfovx), f32(1.3) * f32(cam.tanfovy)
    fx2, fy2 = _focal2(cam, vm)
    with np.errstate(all="ignore"):
        vx = vm[0] * x + vm[4] * y + vm[8] * z + vm[12]
        vy = vm[1] * x + vm[5] * y + vm[9] * z + vm[13]
        vz = vm[2] * x + vm[6] * y + vm[10] * z + vm[14]
        hx = pm[0] * x + pm[4] * y + pm[8] * z + pm[12]
        hy = pm[1] * x + pm[5] * y + pm[9] * z + pm[13]
        hw = pm[3] * x + pm[7] * y + pm[11] * z + pm[15]
        p_w = f32(1.0) / (hw + f32(0.0000001))
        px, py = ((hx * p_w + f32(1.0)) * f32(W) - f32(1.0)) * f32(0.5), ((hy * p_w + f32(1.0)) * f32(H) - f32(1.0)) * f32(0.5)
        iz = f32(1.0) / vz
        jx = np.minimum(np.abs(vx * iz) * f32(1.001), lx)
        jy = np.minimum(np.abs(vy * iz) * f32(1.001), ly)
        kc = fx2 * (f32(1.0) + jx * jx) + fy2 * (f32(1.0) + jy * jy)
        rb = f32(3.0) * np.sqrt(kc * tr * (iz * iz) + f32(0.7)) + f32(2.0)
        gx, gy = (W + 15) // 16, (H + 15) // 16
        out = (px + rb < 0) | (px - rb > gx * 16 + 16) | (py + rb < 0) | (py - rb > gy * 16 + 16)
    return out & (vz > 0.001)


def _group_test_skips(means, tr, w2c, cam):
    """The group test on rounds of 256 consecutive rows of `means` (world coordinates, already in processing order), for the view
    w2c [4,4]: True where the kernel skips the round.  Box of the means and largest trace per round (k_pack_static), sphere
    (c, R) taken to the view's frame, then the four sides and `behind` as linear forms of the centre with |grad| R to spare."""
    W, H = cam.image_width, cam.image_height
    vm, pm = _mats(cam)
    means, tr, m = np.asarray(means, f32), np.asarray(tr, f32), np.asarray(w2c, f32)
    lx, ly = f32(1.3) * f32(cam.tanfovx), f32(1.3) * f32(cam.tanfovy)
    fx2, fy2 = _focal2(cam, vm)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    xmax, ymax = f32(gx * 16 + 16), f32(gy * 16 + 16)
    wrow = abs(pm[3] - vm[2]) + abs(pm[7] - vm[6]) + abs(pm[11] - vm[10]) + abs(pm[15] - vm[14])
    wmag = abs(vm[2]) + abs(vm[6]) + abs(vm[10]) + abs(vm[14])
    n = (means.shape[0] + 255) // 256
    skips = np.zeros(n, bool)
    if not wrow <= f32(1e-6) * wmag:            # not a pinhole projection (clip w != view z): no group test
        return skips
    G = m[:3, :3].T.astype(f32) @ m[:3, :3].astype(f32)
    g = np.abs(G)
    rscale = np.sqrt(f32(max(G[0, 0] + g[0, 1] + g[0, 2], g[0, 1] + G[1, 1] + g[1, 2], g[0, 2] + g[1, 2] + G[2, 2]))) * f32(1.00001)
    kcm = fx2 * (f32(1.0) + lx * lx) + fy2 * (f32(1.0) + ly * ly)
    c0 = f32(6.0)
    Wf, Hf = f32(W), f32(H)
    zn = np.sqrt(vm[2] * vm[2] + vm[6] * vm[6] + vm[10] * vm[10])
    for r in range(n):
        blk, t = means[256 * r:256 * r + 256], tr[256 * r:256 * r + 256]
        if not (np.isfinite(blk).all() and np.isfinite(t).all()):
            continue                             # a NaN bound compares false everywhere: the round is kept
        lo, hi = blk.min(0), blk.max(0)
        cw = f32(0.5) * (lo + hi)
        e = hi - cw
        R = (f32(1.01) * np.sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) + f32(1e-6)) * rscale
        c = np.array([((m[k, 0] * cw[0] + m[k, 1] * cw[1]) + m[k, 2] * cw[2]) + m[k, 3] for k in range(3)], f32)
        a2 = f32(2.0) * f32(1.01) * f32(3.0) * np.sqrt(kcm * t.max())
        zc = vm[2] * c[0] + vm[6] * c[1] + vm[10] * c[2] + vm[14]

        def side(sx, sy, sz, sw, kz, add):
            Ax, Ay, Az = sx + kz * vm[2], sy + kz * vm[6], sz + kz * vm[10]
            Lc = Ax * c[0] + Ay * c[1] + Az * c[2] + (sw + kz * vm[14]) + add
            return Lc + np.sqrt(Ax * Ax + Ay * Ay + Az * Az) * R < 0
        left = side(Wf * pm[0], Wf * pm[4], Wf * pm[8], Wf * pm[12], Wf - f32(1.0) + f32(2.0) * c0, a2)
        right = side(-Wf * pm[0], -Wf * pm[4], -Wf * pm[8], -Wf * pm[12], -(Wf - f32(1.0) - f32(2.0) * xmax - f32(2.0) * c0), a2)
        top = side(Hf * pm[1], Hf * pm[5], Hf * pm[9], Hf * pm[13], Hf - f32(1.0) + f32(2.0) * c0, a2)
        bottom = side(-Hf * pm[1], -Hf * pm[5], -Hf * pm[9], -Hf * pm[13], -(Hf - f32(1.0) - f32(2.0) * ymax - f32(2.0) * c0), a2)
        behind = zc + zn * R <= f32(0.001)
        skips[r] = bool(left or right or top or bottom or behind)
    return skips


def _traces(harness, scales, mod, rots):
    """trace of every Gaussian's 3D covariance as k_pack_static forms it (fr_cov3d of csrc/fr_math.h with the scale modifier) --
    the oracle computes a covariance for visible splats only"""
    P = scales.shape[0]
    cov = np.zeros((P, 6), f32)
    s, r = np.ascontiguousarray(scales, f32), np.ascontiguousarray(rots, f32)
    harness.h_cov3d(ctypes.c_int(P), s.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.c_float(mod),
                    r.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), cov.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    return (cov[:, 0] + cov[:, 3] + cov[:, 5]).astype(f32)


@pytest.mark.parametrize("which", ["border", "room"])
def test_bound_never_drops_a_visible_splat(oracle, which):
    if which == "border":
        from test_gpu_scorer_adversarial import border_scene
        W, H, sc, _ = border_scene()
        K = intrinsics(W, H)
        means, scales, rots, opac, col = sc["means3D"], sc["scales"], sc["rotations"], sc["opacities"], sc["colors"]
    else:
        from fisher_rast import synthetic
        W, H = 160, 112
        K = np.asarray(synthetic.intrinsics(W, H), np.float64)
        act = {k: v.numpy() for k, v in synthetic.activate(synthetic.room_shell(20000, seed=5)).items()}
        w2c = synthetic.invert_rigid(synthetic.candidate_poses(1, seed=5))[0].numpy()
        means = oracle.transform_points(w2c, act["means3D"])
        scales, rots, opac, col = act["scales"], act["rotations"], act["opacities"], act["rgb_colors"]
    cam = oracle.setup_camera(W, H, K, np.eye(4))
    fwd = oracle.rasterize_forward(cam, means, opac, colors_precomp=col, scales=scales, rotations=rots)
    cov3D = fwd["cov3D"]
    outside = _bound_says_outside(np.asarray(means, np.float32), cov3D[:, 0] + cov3D[:, 3] + cov3D[:, 5], cam)
    visible = fwd["radii"] > 0
    assert not (outside & visible).any(), int((outside & visible).sum())
    # ... and on an ordinary scene it is worth having: it removes most of the splats that are in front of the camera but not
    # visible (`border` is built to sit where it cannot)
    front = np.asarray(means)[:, 2] > 0.001
    if which == "room":
        assert outside.sum() > 0.5 * (front & ~visible).sum(), (int(outside.sum()), int((front & ~visible).sum()))


@pytest.mark.parametrize("name", C.ids(C.BATCHED_CASES))
def test_bound_and_group_test_under_the_camera_cases(oracle, harness, name):
    """The scenes and poses the GPU tests score (tests/test_gpu_cameras.py): per view, the early bound never puts a visible splat
    outside and the group test never skips a round of 256 Z-curve neighbours the oracle sees a splat of; the bound does remove
    splats in front of the camera, so the assertion is not empty."""
    from test_gpu_spatial_order import _morton_np
    c = C.by_name(C.BATCHED_CASES)[name]
    sc = C.batched_scene(c)
    cam = C.oracle_camera(oracle, c)
    tr = _traces(harness, sc["scales"], c.scale_modifier, sc["rotations"])
    order = np.argsort(_morton_np(sc["means3D"]), kind="stable")
    removed = 0
    for w in C.frustum_poses(c, 3):
        m = oracle.transform_points(w, sc["means3D"])
        fwd = oracle.rasterize_forward(cam, m, sc["opacities"], colors_precomp=sc["colors"], scales=sc["scales"], rotations=sc["rotations"])
        visible = fwd["radii"] > 0
        outside = _bound_says_outside(m, tr, cam)
        assert not (outside & visible).any(), int((outside & visible).sum())
        removed += int(outside.sum())
        skips = _group_test_skips(sc["means3D"][order], tr[order], w, cam)
        seen = np.add.reduceat(visible[order].astype(np.int64), np.arange(0, len(order), 256)) > 0
        assert not (skips & seen).any(), np.nonzero(skips & seen)[0]
        # a skipped round holds no survivor of the per-Gaussian test either (the kernel's own claim)
        keep = ~outside & (m[:, 2] == m[:, 2])
        vm, _ = _mats(cam)
        vz = vm[2] * m[:, 0] + vm[6] * m[:, 1] + vm[10] * m[:, 2] + vm[14]
        keep &= vz > 0.001
        kept = np.add.reduceat(keep[order].astype(np.int64), np.arange(0, len(order), 256)) > 0
        assert not (skips & kept).any(), np.nonzero(skips & kept)[0]
    assert removed > 0


def test_the_group_test_decides_something(oracle, harness):
    """... and both tests do decide on these scenes, so the assertions above are not empty: from the pose beside the cloud the early
    bound puts more than 1500 of the 5000 splats outside under every case, and the group test skips at least two of the 20 rounds
    under five of the six (under `tall`, whose frustum is 2 x 2 tanfovy high, no round's bounding ball clears a side)."""
    from test_gpu_spatial_order import _morton_np
    deciding = []
    for c in C.BATCHED_CASES:
        sc = C.batched_scene(c)
        cam = C.oracle_camera(oracle, c)
        tr = _traces(harness, sc["scales"], c.scale_modifier, sc["rotations"])
        order = np.argsort(_morton_np(sc["means3D"]), kind="stable")
        w = C.frustum_poses(c, 3)[2]
        assert _bound_says_outside(oracle.transform_points(w, sc["means3D"]), tr, cam).sum() > 1500, c.name
        if _group_test_skips(sc["means3D"][order], tr[order], w, cam).sum() >= 2:
            deciding.append(c.name)
    assert len(deciding) >= 5, deciding
