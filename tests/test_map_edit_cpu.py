"""The map edit on the CPU: the split child's arithmetic (csrc/fr_mapedit_math.h, compiled with g++ in
tests/harness/fr_mapedit_harness.cpp) bit for bit against the binary32 NumPy restatement of tests/map_edit_cases.py (all but logf),
the child log scales and means by their rules against the same chain in binary64, and the product's own bookkeeping Python
(models/SLAM/utils/slam_external.MapEdit) over a NumPy backend against what the reference's remove_points / cat_params_to_optimizer /
prune_gaussians / densify gave (tests/golden/reference_map_edit.npz)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

import map_edit_cases as mc


@pytest.fixture(scope="module")
def edit_harness():
    return mc.build_harness()


@pytest.fixture(scope="module")
def gold():
    return mc.load_golden()


def _children(cols):
    z, means, rot, logs = mc.sweep()
    return z, means, rot, np.ascontiguousarray(logs[:, :cols])


@pytest.mark.parametrize("cols", [3, 1])
@pytest.mark.parametrize("n_into", [2, 3])
def test_harness_equals_the_numpy_restatement_bit_for_bit(edit_harness, oracle, cols, n_into):
    z, means, rot, logs = _children(cols)
    assert np.array_equal(mc.bits(mc.harness_rotations(edit_harness, rot)), mc.bits(mc.np_rotation(rot)))
    assert mc.bits(np.array(edit_harness.frm_divisor(n_into), mc.F)) == mc.bits(np.array(0.8 * n_into, mc.F))
    want_means, arg32 = mc.np_split(oracle.expf, z, means, rot, logs, n_into)
    got_means, got_logs = means.copy(), logs.copy()
    mc.harness_split(edit_harness, n_into, z, got_means, rot, got_logs)
    assert np.array_equal(mc.bits(got_means), mc.bits(want_means))
    # logf is the platform's: within the rule of the binary64 log of its own binary32 argument
    assert mc.log_scale_ok(got_logs, np.log(arg32.astype(np.float64)))


@pytest.mark.parametrize("cols", [3, 1])
@pytest.mark.parametrize("n_into", [2, 3])
def test_child_log_scales_by_the_rule(edit_harness, cols, n_into):
    z, means, rot, logs = _children(cols)
    got = logs.copy()
    mc.harness_split(edit_harness, n_into, z, means.copy(), rot, got)
    want64 = np.log(np.exp(logs.astype(np.float64)) / np.float64(mc.F(0.8 * n_into)))
    assert mc.log_scale_ok(got, want64)
    # an infinite or zero scale: exp gives 0 / inf, the log -inf / inf, exactly
    edge = np.array([[-200.0] * cols, [100.0] * cols], mc.F)
    m = np.zeros((2, 3), mc.F)
    mc.harness_split(edit_harness, n_into, np.zeros((2, 3), mc.F), m, np.array([[1, 0, 0, 0]] * 2, mc.F), edge)
    assert np.all(np.isneginf(edge[0])) and np.all(np.isposinf(edge[1]))
    assert mc.log_scale_ok(edge, np.array([[-np.inf] * cols, [np.inf] * cols]))


def test_child_means_by_the_k_rule(edit_harness):
    """quaternion norms from 1e-3 to 50, scales from 0.003 to 0.3, anisotropic and isotropic; prints the K needed"""
    worst = 0.0
    for cols in (3, 1):
        z, means, rot, logs = _children(cols)
        got = means.copy()
        mc.harness_split(edit_harness, 2, z, got, rot, logs.copy())
        zs = z.astype(np.float64) * (np.exp(logs.astype(np.float64)) * np.ones((1, 3)))
        m64 = means.astype(np.float64)
        want = m64 + np.einsum("nij,nj->ni", mc.rotation64(rot.astype(np.float64)), zs)
        worst = max(worst, mc.k_need(got, want, np.abs(m64) + np.abs(zs).sum(1, keepdims=True)))
    print(f"child means against the binary64 chain: K needed {worst:.2f}, K used {mc.K_CHILD}")
    assert worst <= mc.K_CHILD <= 16
    # K used is twice the K needed, and the figure on record (map_edit_cases.K_NEEDED_CPU) is the one measured here
    assert mc.K_CHILD == min(16.0, round(2 * mc.K_NEEDED_CPU, 1)) and abs(worst - mc.K_NEEDED_CPU) <= 0.05, (worst, mc.K_NEEDED_CPU)
    design = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "DESIGN.md")).read()
    assert f"child means: **K needed, measured on the CPU over quaternion norms from 1e-3 to 50 and scales from 0.003 to 0.3: {mc.K_NEEDED_CPU}" in design


def _edit(edit_harness, st):
    from models.SLAM.utils import slam_external as se
    backend = mc.NumpyBackend(edit_harness, st["z"])
    return se.MapEdit(backend), backend


@pytest.mark.parametrize("case", list(mc.CASES))
def test_bookkeeping_over_the_numpy_backend_against_the_reference(edit_harness, oracle, gold, case):
    st = mc.state_of(case, gold)
    edit, backend = _edit(edit_harness, st)
    snap, params, variables, opt, before = mc.run_case(case, edit, st, "cpu")
    mc.check_bookkeeping(params, variables, opt, before)
    want = mc.golden_of(gold, case)
    mc.compare_with_golden(case, st, snap, want)
    # the lengths, quirk included: seen / means2D keep the old length
    assert int(snap["len/seen"]) == mc.P_GOLDEN == int(snap["len/means2D"])
    # pass count: one plan and one apply per prune, two of each per densify
    fn = mc.CASES[case]["fn"]
    expect = {"remove_points": 1, "cat": 0, "densify": 2, "prune": 0 if case == "prune/off-beat-reset" else 1}[fn]
    assert backend.plans == expect == backend.applies


def test_the_golden_file_covers_what_it_should(gold):
    """rows on the thresholds in the inputs; kept rows, clones and children in every densify result; state and no state"""
    for cols in (3, 1):
        st = {k[len(f"state{cols}/"):]: v for k, v in gold.items() if k.startswith(f"state{cols}/")}
        ls, lo = st["p/log_scales"], st["p/logit_opacities"]
        assert ls.shape == (mc.P_GOLDEN, cols)
        assert (ls == mc.F(np.log(0.05))).any() and (ls == np.nextafter(mc.F(np.log(0.05)), mc.F(1))).any() and (ls == mc.F(np.log(0.1))).any()
        assert (lo == mc.F(np.log(0.005 / 0.995))).any() and (lo == np.nextafter(mc.F(np.log(0.005 / 0.995)), mc.F(-10))).any()
    for case, c in mc.CASES.items():
        w = mc.golden_of(gold, case)
        assert ("m/means3D" in w) == (c["optimizer"] and c["state"]) and "m/" + mc.STATELESS not in w
        assert ("var/timestep" in w) == c["timestep"]
        if c["fn"] == "densify":
            ci = w["child_index"]
            n_child = int((ci >= 0).sum())
            assert 0 < n_child < ci.size - 5 and w["p/log_scales"].shape[1] == c["cols"]
            assert ci.size == w["var/timestep"].size == w["var/denom"].size and not w["var/denom"].any()


def test_thresholds_do_not_cross_and_install_is_opt_in():
    from models.SLAM.utils import slam_external as se
    from models.SLAM.gaussian import MapEditOps
    assert se.CLONE_MAX_SCALE == 0.05 == se.SPLIT_MIN_SCALE
    mod = types.ModuleType("fake_reference_module")
    marks = {n: object() for n in MapEditOps.EDIT_NAMES}
    outside = lambda params, curr_data, obj_mask_2d: None
    mod.__dict__.update(marks, get_gaussians_outside_mask=outside)
    cls = type("Target", (), {"__module__": mod.__name__})
    sys.modules[mod.__name__] = mod
    try:
        assert all(getattr(mod, n) is marks[n] for n in marks)                  # nothing installed by default
        assert MapEditOps.install(cls) is cls
        for n in MapEditOps.EDIT_NAMES:
            assert getattr(mod, n) is not marks[n] and getattr(mod, n).__self__.outside_mask_fn is outside
        empty = types.ModuleType("fake_empty_module")
        sys.modules[empty.__name__] = empty
        with pytest.raises(ValueError):
            MapEditOps.install(type("Other", (), {"__module__": empty.__name__}))
    finally:
        sys.modules.pop(mod.__name__, None)
        sys.modules.pop("fake_empty_module", None)


def test_object_mask_branch_ors_the_outside_mask(edit_harness, oracle, gold):
    """prune_gaussians with obj_mask_2d: the module's outside mask, ANDed with `active` and the optional size cut, is OR-ed in"""
    from models.SLAM.utils import slam_external as se
    st = mc.state_of("prune/before-stop", gold)
    outside = np.zeros(mc.P_GOLDEN, bool)
    outside[10:30] = True
    seen_args = []

    def outside_fn(params, curr_data, obj_mask_2d):
        seen_args.append((curr_data, obj_mask_2d))
        return torch.from_numpy(outside), {}

    edit = se.MapEdit(mc.NumpyBackend(edit_harness), outside_mask_fn=outside_fn)
    params, variables, opt = mc.build_inputs(st, "cpu")
    cfg = dict(mc.PRUNE, outside_opacity_thresh=0.3, outside_max_scale=0.02)
    params, variables = edit.prune_gaussians(params, variables, opt, 20, cfg, None, "data", "mask")
    assert seen_args == [("data", "mask")]
    from oracle import densify_stats as ods
    lo, ls = st["p/logit_opacities"], st["p/log_scales"]
    alpha = torch.sigmoid(torch.from_numpy(lo)).squeeze(-1).numpy()
    big = torch.exp(torch.from_numpy(ls)).max(dim=1).values.numpy() >= 0.02
    rm = ods.prune_mask(lo, ls, 0.005, None) | (outside & (alpha >= 0.3) & big)
    assert 0 < (rm & ~ods.prune_mask(lo, ls, 0.005, None)).sum()
    assert np.array_equal(mc.bits(params["means3D"].detach().numpy()), mc.bits(st["p/means3D"][~rm]))
    with pytest.raises(ValueError):
        se.MapEdit(mc.NumpyBackend(edit_harness)).prune_gaussians(*mc.build_inputs(st, "cpu"), 20, cfg, None, "data", "mask")
