"""CPU: the scenes of tests/test_gpu_cameras.py exercise what they claim -- proved with the oracle alone, so that a GPU test which
passes has passed on visible splats on both sides of the 1.3 tanfov clamp of forward.cu:80-84 (on each axis), on splats that cross
each of the four image borders, on tile lists the chunked backward cuts, and (power 2) on Gaussians whose reference chain is itself
well conditioned in binary32 (the arbiter condition of test_gpu_rasterizer_parity.py::test_backward_parity)."""
import numpy as np
import pytest

import cameras as C

NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")


def _forward(oracle, cam, sc, means=None):
    return oracle.rasterize_forward(cam, sc["means3D"] if means is None else means, sc["opacities"], colors_precomp=sc["colors"],
                                    scales=sc["scales"], rotations=sc["rotations"])


def _check_coverage(oracle, cam, means, fwd, what):
    cx, cy = C.clamp_counts(oracle, cam, means, fwd)
    assert cx >= 20 and cy >= 20, (what, "visible and clamped in x / y", cx, cy)
    # ... and the clamp does not hold everywhere: most visible splats are on its inside
    assert cx + cy < 0.5 * int((fwd["radii"] > 0).sum()), (what, cx, cy)
    borders = C.border_counts(cam, fwd)
    assert min(borders) >= 20, (what, "visible across the left / right / top / bottom border", borders)


@pytest.mark.parametrize("name", C.ids(C.RASTER_CASES))
def test_raster_scenes(oracle, name):
    c = C.by_name(C.RASTER_CASES)[name]
    cam = C.oracle_camera(oracle, c)
    sc = C.raster_scene(c)
    fwd = _forward(oracle, cam, sc)
    _check_coverage(oracle, cam, sc["means3D"], fwd, name)
    # three of the four scenes hold lists the chunked backward cuts; offcentre-m0.4 (small splats, longest list 133) runs the chunked
    # kernels on lists of a single segment
    longest = int((fwd["ranges"][:, 1].astype(np.int64) - fwd["ranges"][:, 0]).max())
    assert (longest > 256) == (name in C.CHUNKED_CASES), (name, longest)
    # the arbiter condition: fewer than 2 % of the Gaussians are off by more than 2e-5 in the reference's own binary32 chain
    dL = np.full((3, c.H, c.W), 1e-3, np.float32)
    gw = oracle.rasterize_backward(cam, fwd, dL, 2)
    w64 = oracle.rasterize_forward(cam, sc["means3D"], sc["opacities"], colors_precomp=sc["colors"], scales=sc["scales"],
                                   rotations=sc["rotations"], decisions=fwd)
    ga = oracle.rasterize_backward(cam, w64, dL, 2)
    for n in NAMES:
        o, a = gw[n].astype(np.float64).reshape(gw[n].shape[0], -1), ga[n].reshape(gw[n].shape[0], -1)
        big = np.abs(a) > 1e-7 * np.abs(a).max()
        r = np.where(big, np.abs(o - a) / np.maximum(np.abs(a), 1e-300), 0.0).max(axis=1)
        assert (r > 2e-5).mean() < 0.02, (name, n, float((r > 2e-5).mean()), float(r.max()))


@pytest.mark.parametrize("name", C.ids(C.BATCHED_CASES))
def test_batched_scenes(oracle, name):
    """pose 0 sees the spread scene (both clamps, four borders); the corner pose and the outside pose see part of it, with the
    background showing; and over the three views fewer than 2 % of the (view, Gaussian) pairs are off by more than 2e-5 in the
    reference's own binary32 chain (the condition of test_gpu_point_scores.py::test_point_scores_against_the_oracle)"""
    from test_gpu_scorer_adversarial import _entry_tolerance
    c = C.by_name(C.BATCHED_CASES)[name]
    cam = C.oracle_camera(oracle, c)
    sc = C.batched_scene(c)
    P = sc["means3D"].shape[0]
    clear, wide = False, {4: 0, 11: 0}
    for v, w in enumerate(C.frustum_poses(c, 3)):
        m = oracle.transform_points(w, sc["means3D"])
        fwd = _forward(oracle, cam, sc, m)
        n_vis = int((fwd["radii"] > 0).sum())
        assert 0 < n_vis < P, (name, v, n_vis)
        clear = clear or bool((fwd["final_T"] > 0.5).any())
        for columns in (4, 11):
            o, a, _ = oracle.compute_hessian(cam, w, sc["means3D"], sc["colors"], sc["rotations"], sc["opacities"], sc["scales"],
                                             columns=columns, arbiter=True)
            wide[columns] += int((_entry_tolerance(o, a, columns)[1] > 2e-5).sum())
        if v == 0:
            _check_coverage(oracle, cam, m, fwd, name)
            # the two blobs on the left and the top edge are (partly) visible: the group test must keep their rounds
            assert (fwd["radii"][P - 600:] > 0).sum() > 100 and (fwd["radii"][P - 1200:P - 600] > 0).sum() > 100
    assert clear and max(wide.values()) <= 0.02 * 3 * P, (clear, wide)


@pytest.mark.parametrize("name", C.ids(C.PAIR_CASES))
def test_pair_scenes(oracle, name):
    """the scenes of the fused pair test: the same clamp and border bounds, and lists the chunked pair backward cuts (the two blobs:
    tiles of the left and of the top edge hold more than 600 splats each)"""
    c = C.by_name(C.PAIR_CASES)[name]
    cam, sc = C.oracle_camera(oracle, c), C.pair_scene(c)
    fwd = _forward(oracle, cam, sc)
    _check_coverage(oracle, cam, sc["means3D"], fwd, name)
    length = fwd["ranges"][:, 1].astype(np.int64) - fwd["ranges"][:, 0]
    assert (length > 600).sum() >= 2 and (fwd["radii"] > 0).sum() > 500, np.sort(length)[-4:]
    # ... and hardly a splat covers the whole image (see PAIR_CASES: the order of the tiles' atomic adds is not the test's subject)
    assert (fwd["radii"] > 64).sum() <= 4, int((fwd["radii"] > 64).sum())


@pytest.mark.parametrize("name", C.ids(C.POSE_CASES))
def test_pose_scenes(oracle, name):
    """the 48 x 32 variants the pose Fisher test uses: still anisotropic / off-centre, and in each of its views the same clamp and
    border bounds"""
    c = C.by_name(C.POSE_CASES)[name]
    assert c.tanfov[0] != c.tanfov[1] and (c.W, c.H) == (48, 32)
    cam = C.oracle_camera(oracle, c)
    sc = C.pose_scene(c)
    assert sc["means3D"].shape[0] <= 500
    for v, w in enumerate(C.pose_views(c)):
        m = oracle.transform_points(w, sc["means3D"])
        _check_coverage(oracle, cam, m, _forward(oracle, cam, sc, m), (name, v))
