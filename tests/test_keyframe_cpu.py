"""The keyframe overlap on the CPU: the arithmetic (csrc/fr_keyframe_math.h, compiled with g++ in tests/harness/fr_keyframe_harness.cpp)
bit for bit against the binary32 NumPy restatement of tests/keyframe_cases.py on every family; against the reference-order torch
chain and the outputs of the reference's own functions (tests/golden/reference_keyframe.npz) on the cases that qualify -- every
decision clear of its threshold in binary64 by about 40 times the binary32 evaluation error, since torch's matmul does not promise
our summation order; the drop-in (models/SLAM/utils/keyframe_selection.py) over the harness against the torch chain under the same
seeds; the install; the ABI's rejections, which need no device."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

import keyframe_cases as kc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_keyframe.npz")


@pytest.fixture(scope="module")
def kf_harness():
    return kc.build_harness()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_key_is_torch_round_to_four_decimals(kf_harness):
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(-10, 10, 20000), rng.integers(-99999, 99999, 20000) / 1e4 + 5e-5, [0.0, -0.0, 4.99e-5, 5.01e-5]]).astype(np.float32)
    want = torch.abs(torch.round(_t(x), decimals=4)).numpy()
    got = np.array([kf_harness.frk_key_of(float(v)) for v in x], np.float32)
    assert np.array_equal(_bits(got), _bits(want))


def test_the_duplicate_filter_keeps_the_reference_quirk(kf_harness):
    """[[1,2,3],[1,2,3],[-1,2,3],[0,0,0],[5,5,5]]: unique / isin mark the first four -- both copies, the mirror image and the origin"""
    pts = torch.tensor([[1.0, 2, 3], [1, 2, 3], [-1, 2, 3], [0, 0, 0], [5, 5, 5]])
    keys = torch.abs(torch.round(pts, decimals=4))
    _, inv, counts = torch.cat([keys, torch.zeros((1, 3))]).unique(dim=0, return_inverse=True, return_counts=True)
    assert torch.isin(inv, torch.where(counts.gt(1))[0])[:5].tolist() == [True, True, True, True, False]
    # the same through the harness: a 1 x 5 frame under fx = 1, cx = 0.5 and the identity pose back-projects to (-1.5,0,3), (1.5,0,3) --
    # mirror images --, (4.5,0,3), the camera origin (no depth) and (17.5,0,5)
    c = dict(H=1, W=5, K=np.eye(3, dtype=np.float32), w2c=np.eye(4, dtype=np.float32), kf_w2c=np.zeros((0, 4, 4), np.float32), kf_masks=[],
             edge=0, depth=np.array([[[3.0, 3.0, 3.0, 0.0, 5.0]]], np.float32), draws=np.arange(5), valid_idx=None)
    c["K"][0, 2] = 0.5
    got = kc.harness_overlap(kf_harness, c, valid_idx=None)
    assert got["pts"][0].tolist() == [-1.5, 0.0, 3.0] and got["pts"][1].tolist() == [1.5, 0.0, 3.0]
    assert got["valid"].tolist() == [0, 0, 1, 0, 1] and got["status"].tolist() == [2, 0, 0, 0]
    # a pixel drawn twice loses both copies
    got = kc.harness_overlap(kf_harness, c, valid_idx=None, draws=np.array([2, 4, 2]))
    assert got["valid"].tolist() == [0, 1, 0]


@pytest.mark.parametrize("family", kc.FAMILIES)
def test_harness_equals_the_binary32_restatement(kf_harness, family):
    """every family, two seeds, with the index list and with pixels drawn directly: integers and flags equal, points bit for bit"""
    for seed in (0, 1):
        c = kc.make_case(family, seed)
        idx, status = kc.harness_valid_pixels(kf_harness, c["depth"], c["curr_mask"])
        assert np.array_equal(idx, c["valid_idx"]) and np.array_equal(idx, kc.np_valid_pixels(c)) and status.tolist() == [len(idx), 0, 0, 0]
        routes = [("case", None)]
        if len(idx):
            routes.append((None, c["valid_idx"][c["draws"]].astype(np.int64)))
        for vi, draws in routes:
            got, want = kc.harness_overlap(kf_harness, c, valid_idx=vi, draws=draws), kc.np_overlap(c, np.float32, valid_idx=vi, draws=draws)
            assert np.array_equal(got["counts"], want["counts"]), family
            assert np.array_equal(got["valid"].astype(bool), want["valid"]) and np.array_equal(_bits(got["pts"]), _bits(want["pts"]))
            assert got["status"].tolist() == [want["n_valid"], want["n_oor"], 0, 0]
            assert np.array_equal(_bits(got["uv"][:, want["valid"]]), _bits(want["uv"][:, want["valid"]]))


def test_the_adversarial_families_sit_on_their_decisions(kf_harness):
    c = kc.make_case("wall")
    r = kc.harness_overlap(kf_harness, c)
    pix = c["valid_idx"][c["draws"]]
    once = np.array([np.sum(pix == p) == 1 for p in pix])
    assert (once & (r["valid"] == 0)).any(), "no mirror pair among the draws"          # drawn once, and still dropped
    c = kc.make_case("dup-draws")
    assert 0 < kc.harness_overlap(kf_harness, c)["status"][0] < len(c["draws"])
    c = kc.make_case("all-invalid")
    r = kc.harness_overlap(kf_harness, c)
    assert r["status"].tolist() == [0, 0, 0, 0] and not r["counts"].any() and not r["valid"].any()
    c = kc.make_case("zero-depth-in-mask")
    assert 12 * c["W"] + 15 not in c["valid_idx"] and len(c["valid_idx"]) == 198
    c = kc.make_case("curr-mask-empty")
    assert len(c["valid_idx"]) == 0
    for family in ("edges", "masks-absent-edge0"):
        c = kc.make_case(family)
        only = kc.harness_overlap(kf_harness, c, draws=c["draws"][:10])          # the ten pixels on and next to the thresholds
        e, H, W = c["edge"], c["H"], c["W"]
        u, v = only["uv"][0, :, 0], only["uv"][0, :, 1]
        pix = c["valid_idx"][c["draws"][:10]]
        assert np.array_equal(u, (pix % W).astype(np.float32)) and np.array_equal(v, (pix // W).astype(np.float32))       # exact projections
        strictly = (u < W - e) & (u > e) & (v < H - e) & (v > e)
        assert (u == e).any() and (v == e).any() and 0 < strictly.sum() < 10
        assert e == 0 or ((u == W - e).any() and (v == H - e).any())             # no pixel lies on W itself
        # a point on a threshold is outside, the one next to it inside
        assert only["valid"].all() and only["counts"][0] == strictly.sum()


@pytest.mark.parametrize("family", kc.QUALIFYING)
def test_harness_against_the_torch_chain_on_qualifying_cases(kf_harness, family):
    c = kc.qualifying_case(family)
    got = kc.harness_overlap(kf_harness, c)
    rec = {}
    torch.manual_seed(c["seed"])
    np.random.seed(0)
    kc.torch_chain(_t(c["depth"]), _t(c["w2c"]), _t(c["K"]), kc.keyframe_list(c), 2, None if c["curr_mask"] is None else _t(c["curr_mask"]),
                   pixels=len(c["draws"]), edge=c["edge"], record=rec)
    assert np.array_equal(rec["draws"].numpy(), c["draws"])
    assert np.array_equal(rec["valid"].numpy(), got["valid"].astype(bool)) and rec["pts"].shape[0] == got["status"][0] > 0
    assert np.allclose(rec["pts"].numpy(), got["pts"][got["valid"].astype(bool)], rtol=0, atol=1e-5)
    want = np.array(rec["percent"], np.float32)
    assert np.array_equal(got["counts"].astype(np.float32) / np.float32(got["status"][0]), want), (got["counts"], want)
    assert (got["counts"] > 0).any()
    # the binary64 restatement decides alike
    r64 = kc.np_overlap(c, np.float64)
    assert np.array_equal(r64["counts"], got["counts"]) and np.array_equal(r64["valid"], got["valid"].astype(bool))


def _drop_in(kf_harness):
    from models.SLAM.utils.keyframe_selection import KeyframeSelection
    return KeyframeSelection(kc.HarnessBackend(kf_harness))


@pytest.mark.parametrize("family", kc.QUALIFYING)
def test_drop_in_selects_what_the_torch_chain_selects(kf_harness, family):
    """the product's host logic over the kernels' arithmetic, at the product's own margin of 20 pixels: identical lists for k below
    and above the number of overlapping keyframes, and the random streams left where the chain leaves them"""
    sel = _drop_in(kf_harness)
    c = None
    for seed in range(kc.MAX_SEEDS):
        cand = kc.make_case(family, seed, 96, 128, n=24 if family.startswith("masks") else 64, K=5)
        cand["edge"] = 20
        if kc.qualifies(cand):
            c = cand
            break
    assert c is not None, family
    depth, w2c, K = _t(c["depth"]), _t(c["w2c"]), _t(c["K"])
    mask = None if c["curr_mask"] is None else _t(c["curr_mask"])
    kfs = kc.keyframe_list(c)
    overlapping = int((kc.harness_overlap(kf_harness, c)["counts"] > 0).sum())
    assert overlapping >= 2
    for k in (1, overlapping - 1, overlapping, overlapping + 3):
        torch.manual_seed(c["seed"]); np.random.seed(7)
        want = kc.torch_chain(depth, w2c, K, kfs, k, mask, pixels=len(c["draws"]))
        after = (torch.rand(1).item(), np.random.rand())
        torch.manual_seed(c["seed"]); np.random.seed(7)
        got = sel.keyframe_selection_overlap(depth, w2c, K, kfs, k, mask, pixels=len(c["draws"]))
        assert got == want and len(got) == min(k, overlapping) and all(type(a) is type(b) for a, b in zip(got, want))
        assert after == (torch.rand(1).item(), np.random.rand())
    assert sel.backend.calls == ["valid_pixels", "overlap"] * 4


def test_drop_in_corner_returns(kf_harness):
    sel = _drop_in(kf_harness)
    c = kc.make_case("curr-mask-empty")
    state = torch.random.get_rng_state()
    assert sel.keyframe_selection_overlap(_t(c["depth"]), _t(c["w2c"]), _t(c["K"]), kc.keyframe_list(c), 3, _t(c["curr_mask"])) == []
    assert torch.equal(state, torch.random.get_rng_state()) and sel.backend.calls == ["valid_pixels"]          # returned before any draw
    # nothing survives the filter -- two pixels, the same one drawn twice: 0 / 0 is NaN and selects nothing
    c = kc.make_case("generic", H=96, W=128)
    two = np.zeros_like(c["depth"])
    two[0, 40, 50], two[0, 41, 50] = 2.0, 2.5
    seed = next(s for s in range(64) if len(set(torch.manual_seed(s) and torch.randint(2, (2,)).tolist())) == 1)
    torch.manual_seed(seed)
    assert sel.keyframe_selection_overlap(_t(two), _t(c["w2c"]), _t(c["K"]), kc.keyframe_list(c), 3, pixels=2) == []
    assert sel.last["n_valid"] == 0 and not sel.last["counts"].any()
    # no keyframes: nothing to select
    assert sel.keyframe_selection_overlap(_t(c["depth"]), _t(c["w2c"]), _t(c["K"]), [], 3) == []
    # get_pointcloud: the kept points of the sampled pixels, as the chain's
    rc = torch.tensor([[10, 12], [10, 12], [20, 30], [5, 6]])
    got = sel.get_pointcloud(_t(c["depth"]), _t(c["K"]), _t(c["w2c"]), rc)
    want = kc.torch_pointcloud(_t(c["depth"]), _t(c["K"]), _t(c["w2c"]), rc)
    assert got.shape == want.shape == (2, 3) and torch.allclose(got, want, rtol=0, atol=1e-5)


def test_keyframe_masks_keys_and_resize():
    from models.SLAM.utils.keyframe_selection import _keyframe_masks
    a, b = torch.zeros(4, 6, dtype=torch.bool), torch.ones(2, 3)
    a[1, 2] = True
    out = _keyframe_masks([{"obj_mask_2d": a, "mask": b}, {"mask": b}, {}, {"obj_mask_2d": None, "mask": a.float()}], 4, 6)
    assert out[0] is not None and torch.equal(out[0], a) and out[1].shape == (4, 6) and bool(out[1].all()) and out[2] is None
    assert out[3].dtype == torch.bool and torch.equal(out[3], a)


def test_reference_pin(kf_harness):
    """the drop-in's counts, kept points and selected ids against what the reference's own functions returned
    (tests/golden/make_reference_keyframe_vectors.py) on three qualifying cases"""
    z = np.load(GOLDEN)
    names = [str(k) for k in z["cases"]]
    assert len(names) == 3
    sel = _drop_in(kf_harness)
    for name in names:
        family, seed, H, W = name.split("/")
        c = kc.make_case(family, int(seed), int(H), int(W), n=24 if family.startswith("masks") else 64, K=5)
        c["edge"] = 20
        assert kc.qualifies(c), name
        torch.manual_seed(c["seed"]); np.random.seed(11)
        got = sel.keyframe_selection_overlap(_t(c["depth"]), _t(c["w2c"]), _t(c["K"]), kc.keyframe_list(c), int(z[name + "/k"]),
                                             None if c["curr_mask"] is None else _t(c["curr_mask"]), pixels=len(c["draws"]))
        pts, percent = z[name + "/pts"], z[name + "/percent_inside"]
        assert sel.last["n_valid"] == pts.shape[0] > 0
        assert np.array_equal(sel.last["counts"].astype(np.float32) / np.float32(sel.last["n_valid"]), percent.astype(np.float32))
        assert [int(i) for i in got] == [int(i) for i in z[name + "/selected"]] and len(got) > 0
        r = kc.harness_overlap(kf_harness, c)
        assert np.allclose(r["pts"][r["valid"].astype(bool)], pts, rtol=0, atol=1e-5)
        gp = sel.get_pointcloud(_t(c["depth"]), _t(c["K"]), _t(c["w2c"]), _t(z[name + "/sampled_indices"]))
        assert np.allclose(gp.numpy(), z[name + "/get_pointcloud"], rtol=0, atol=1e-5)


def test_install_replaces_the_one_name():
    from models.SLAM import gaussian as G
    from models.SLAM.utils import keyframe_selection as ks
    mod = types.ModuleType("fake_ref_gaussian_keyframes")
    keep = object()
    mod.keyframe_selection_overlap = keep
    mod.get_pointcloud = keep
    sys.modules[mod.__name__] = mod
    try:
        cls = type("RefSLAM", (), {"__module__": mod.__name__})
        attrs = set(vars(cls))
        before = dict(vars(mod))
        assert G.KeyframeSelectOps.install(cls) is cls
        changed = {k for k, v in vars(mod).items() if before.get(k, None) is not v}
        assert changed == {"keyframe_selection_overlap"} and mod.keyframe_selection_overlap == ks.keyframe_selection_overlap
        assert set(vars(cls)) == attrs
        del mod.keyframe_selection_overlap
        with pytest.raises(ValueError, match="keyframe_selection_overlap"):
            G.KeyframeSelectOps.install(cls)
    finally:
        del sys.modules[mod.__name__]
    # opt-in: the package's own classes are left alone
    assert not hasattr(G, "keyframe_selection_overlap")


def test_abi_rejections_need_no_device():
    import __graft_entry__ as g
    g.build()
    from fisher_rast import _lib
    lib = _lib.load()
    assert _lib.FR_KEYFRAME_MAX_POINTS >= 4096
    assert lib.fr_keyframe_overlap_workspace_bytes(0) == 0 and lib.fr_keyframe_overlap_workspace_bytes(_lib.FR_KEYFRAME_MAX_POINTS + 1) == 0
    assert lib.fr_keyframe_overlap_workspace_bytes(1) > 0 and lib.fr_keyframe_overlap_workspace_bytes(_lib.FR_KEYFRAME_MAX_POINTS) >= 25 * 4096
    assert lib.fr_keyframe_valid_pixels_workspace_bytes(0, 4) == 0 and lib.fr_keyframe_valid_pixels_workspace_bytes(1 << 16, 1 << 15) == 0
    assert lib.fr_keyframe_valid_pixels_workspace_bytes(48, 64) >= 2 * 4 * 12
    # addresses that are never dereferenced: every call below is refused on the host
    A = 1 << 20
    big = 1 << 30

    def overlap(cfg=None, depth=A, valid_idx=A, draws=A, kf=A, table=None, counts=A, valid=None, pts=None, status=A, ws=A, nws=big, **kw):
        f = dict(H=48, W=64, n=16, K=2, edge=20, n_valid_idx=100, intrinsics=A, w2c=A)
        f.update(kw)
        cfg = _lib.KeyframeCfg(*(f[k] for k in ("H", "W", "n", "K", "edge", "n_valid_idx", "intrinsics", "w2c")))
        return lib.fr_keyframe_overlap(ctypes.byref(cfg), depth, valid_idx, draws, kf, table, counts, valid, pts, status, ws, nws, None)

    assert lib.fr_keyframe_overlap(None, A, A, A, A, None, A, None, None, A, A, big, None) == _lib.FR_EINVAL
    for bad in (dict(depth=None), dict(draws=None), dict(status=None), dict(intrinsics=None), dict(w2c=None), dict(kf=None), dict(counts=None),
                dict(ws=None), dict(n=0), dict(n=_lib.FR_KEYFRAME_MAX_POINTS + 1), dict(K=-1), dict(edge=-1), dict(H=0), dict(W=-3),
                dict(n_valid_idx=-1), dict(nws=int(lib.fr_keyframe_overlap_workspace_bytes(16)) - 1), dict(nws=0),
                dict(depth=A + 2), dict(pts=A + 1), dict(kf=A + 3), dict(intrinsics=A + 2), dict(w2c=A + 1), dict(draws=A + 4),
                dict(table=A + 4), dict(ws=A + 4), dict(valid_idx=A + 2), dict(counts=A + 1), dict(status=A + 2)):
        assert overlap(**bad) == _lib.FR_EINVAL, bad
        assert b"fr_keyframe_overlap" in lib.fr_last_error()

    def pixels(H=48, W=64, depth=A, mask=None, idx=A, status=A, ws=A, nws=big):
        return lib.fr_keyframe_valid_pixels(H, W, depth, mask, idx, status, ws, nws, None)

    for bad in (dict(depth=None), dict(idx=None), dict(status=None), dict(ws=None), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15),
                dict(nws=int(lib.fr_keyframe_valid_pixels_workspace_bytes(48, 64)) - 1), dict(depth=A + 1), dict(idx=A + 2), dict(status=A + 3),
                dict(ws=A + 4)):
        assert pixels(**bad) == _lib.FR_EINVAL, bad
        assert b"fr_keyframe_valid_pixels" in lib.fr_last_error()
    assert lib.fr_version() == 100


def test_sources_and_exports():
    from fisher_rast import _lib
    assert os.path.join(_lib._CSRC, "fr_keyframe.hip") in _lib.UNITS and os.path.join(_lib._CSRC, "fr_keyframe_math.h") in _lib.SOURCES
    for name in ("fr_keyframe_valid_pixels_workspace_bytes", "fr_keyframe_overlap_workspace_bytes", "fr_keyframe_valid_pixels", "fr_keyframe_overlap"):
        assert name in _lib.EXPORTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "fisher-nerf-customized_amd", "csrc", "fr_keyframe_math.h")).read()
    assert '#include "fr_ingest_math.h"' in header and "void fri_invert_affine" not in header and "void fri_back_project" not in header
