"""-m gpu: the one chunk-and-redo driver of FisherScorer under its four callers (run, pose_fisher, render_views, point_scores).
Five views, at most two per launch, and buffers far too small at the start: the first launch (three views) overflows, the buffers
grow, the chunk shrinks to two views -- the caller's per-view slices are taken again -- and is redone; then two more launches.
What comes out is, bit for bit, what one launch of a scorer that never overflowed gives.

The per-Gaussian sums of point_scores are the exception the library documents: every (view, Gaussian) entry is a sum of one float
atomic add per tile the splat reaches, in whatever order the tiles finish, and a tile's term is itself a sum of double atomics in
LDS rounded to float.  The terms are non-negative and there are at most T = 12 of them (64 x 48 pixels): a term may round either
way (one ulp, 2^-23 of it), each of the two orders of the T terms loses at most (T - 1) 2^-24 of the entry -- two results differ by
at most 2 T 2^-24 of the entry.  Whether the bits agreed is printed."""
import numpy as np
import pytest
import torch

from scenes import random_scene, intrinsics

pytestmark = pytest.mark.gpu

W, H, P, V = 64, 48, 2000, 5
TILES = ((W + 15) // 16) * ((H + 15) // 16)
ATOMIC_ORDER = 2.0 * TILES * 2.0 ** -24


def _yaw(k):
    yaw, t = 0.06 * k, np.array([0.04 * k, -0.02 * k, 0.03 * k], np.float32)
    c, s = np.cos(yaw), np.sin(yaw)
    d = np.eye(4, dtype=np.float32)
    d[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    d[:3, 3] = t
    return d


@pytest.fixture(scope="module")
def scene(gpu):
    from models.SLAM.utils.recon_helpers import setup_camera
    sc = random_scene(P, 5, zmin=1.0, spread=0.8)
    cam = setup_camera(W, H, intrinsics(W, H), np.eye(4), device=gpu)
    t = [torch.from_numpy(np.ascontiguousarray(sc[k])).to(gpu) for k in ("means3D", "colors", "rotations", "opacities", "scales")]
    w2c = torch.from_numpy(np.stack([_yaw(k) for k in range(V)])).to(gpu)
    g = torch.Generator().manual_seed(3)
    return dict(cam=cam, t=t, w2c=w2c, H_inv=(torch.rand((P, 4), generator=g) * 3.0 + 0.05).to(gpu),
                H_inv_v=(torch.rand((V, P, 4), generator=g) * 3.0 + 0.05).to(gpu), whole={})


CALLS = {   # entry -> (the driver under test, the *_launch method it goes through)
    "run": (lambda s, sc: sc.run(s["w2c"], H_inv=s["H_inv_v"], H_inv_per_view=True), "launch"),
    "pose": (lambda s, sc: dict(pose_H=sc.pose_fisher(s["w2c"])), "pose_launch"),
    "render": (lambda s, sc: sc.render_views(s["w2c"]), "render_launch"),
    "point": (lambda s, sc: sc.point_scores(s["w2c"], s["H_inv_v"], H_inv_per_view=True), "point_launch"),
}
SUMS_OF_ATOMICS = ("point_scores", "point_max")


def _whole(scene, entry):
    """one launch of a scorer with room for everything, computed once per entry point and left as it is"""
    from fisher_rast.ops import FisherScorer
    if entry not in scene["whole"]:
        sc = FisherScorer(scene["cam"], *scene["t"])
        assert sc.max_views_per_launch() >= V
        scene["whole"][entry] = {k: v.clone() for k, v in CALLS[entry][0](scene, sc).items() if v is not None}
    return scene["whole"][entry]


@pytest.mark.parametrize("mode", ["segments", "key_buffer"])
@pytest.mark.parametrize("entry", sorted(CALLS))
def test_chunk_boundary_and_overflow_redo_give_the_bits_of_one_launch(scene, gpu, monkeypatch, entry, mode):
    from fisher_rast.ops import FisherScorer
    want = _whole(scene, entry)
    # fixed segments shorter than the longest tile list, or packed lists in a key buffer too small
    sc = FisherScorer(scene["cam"], *scene["t"], tile_capacity=16 if mode == "segments" else 0)
    sc.per_view_capacity = 64
    # three views per launch until the buffers have grown, two from then on: the overflowed chunk comes back shorter
    monkeypatch.setattr(FisherScorer, "max_views_per_launch", lambda self: 3 if self.per_view_capacity == 64 else 2)
    call, launch_name = CALLS[entry]
    real, launches = getattr(FisherScorer, launch_name), []
    monkeypatch.setattr(FisherScorer, launch_name, lambda self, w, *a, **k: (launches.append(int(w.shape[0])), real(self, w, *a, **k))[1])
    got = call(scene, sc)
    monkeypatch.undo()
    assert launches == [3, 2, 2, 1], launches
    assert sc.per_view_capacity > 64 and (mode == "key_buffer" or sc.tile_capacity == 0 or sc.tile_capacity > 16)
    assert set(k for k, v in got.items() if v is not None) == set(want)
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and g.dtype == w.dtype, k
        same = torch.equal(g.view(torch.int32), w.view(torch.int32))
        if k in SUMS_OF_ATOMICS:
            print(f"[{entry} {mode}] {k}: bits {'equal' if same else 'differ (order of the float atomics)'}")
            assert bool(((g.double() - w.double()).abs() <= ATOMIC_ORDER * w.double()).all()) and float(w.max()) > 0, k
        else:
            assert same, (entry, mode, k)
