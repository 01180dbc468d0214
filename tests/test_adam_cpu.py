"""The fused Adam step on the CPU: the arithmetic (csrc/fr_adam_math.h, compiled with g++ in tests/harness/fr_adam_harness.cpp) bit
for bit against the binary32 NumPy restatement of tests/adam_cases.py and stage by stage against binary64; twenty steps of
fisher_rast.optim.FusedAdam over that harness against torch.optim.Adam in float64, with torch's own float32 Adam as the yardstick;
FusedAdam's bookkeeping (state layout, skipped parameters, state_dict round trips, skip_frozen, the fallbacks); the graft
OptimizerOps.install; the ABI of fr_adam_step."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adam_cases as ac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def adam_harness():
    return ac.build_harness()


@pytest.fixture(scope="module")
def swept():
    return ac.sweep()


# ---- 1. the harness against the NumPy restatement -------------------------------------------------------------------------------

@pytest.mark.parametrize("cset", ac.COEFF_SETS, ids=lambda c: f"lr{c[0]}-b{c[1][0]}-eps{c[2]}-t{c[3]}")
def test_harness_equals_the_numpy_restatement_bit_for_bit(adam_harness, swept, cset):
    p, g, m, v = swept
    c = ac.coeffs(*cset)
    got = ac.harness_stepped(adam_harness, p, g, m, v, c)
    want = ac.np_step(p, g, m, v, c)
    for name, a, b in zip("pmv", got, want):
        assert ac.same_bits_or_both_nan(a, b), name
    # what the sweep is there for: NaN results (from NaN / inf gradients), an overflowed second moment, denormal results, both signs of zero
    assert np.isnan(got[0]).any() and np.isinf(got[2]).any() and ((got[2] > 0) & (got[2] < np.finfo(ac.F).tiny)).any()
    # fresh: the moments are not read
    junk = np.full_like(m, np.nan)
    fresh = ac.harness_stepped(adam_harness, p, g, junk, junk, c, fresh=True)
    zeros = ac.harness_stepped(adam_harness, p, g, np.zeros_like(m), np.zeros_like(v), c)
    for a, b in zip(fresh, zeros):
        assert ac.same_bits_or_both_nan(a, b)


def test_a_frozen_parameter_moves_only_by_a_non_finite_gradient(adam_harness, swept):
    """lr == 0 goes through the same arithmetic, p + (-0) x: finite gradients leave p's bits, NaN / inf gradients poison it as in torch"""
    p, g, m, v = swept
    c = ac.coeffs(0.0, (0.9, 0.999), 1e-8, 3)
    p1, m1, v1 = ac.harness_stepped(adam_harness, p, g, m, v, c)
    bad = ~np.isfinite(g)
    assert bad.any() and np.isnan(p1[bad]).all()
    ok = np.isfinite(g) & np.isfinite(v1)
    assert np.array_equal(ac.bits(p1[ok]), ac.bits(p[ok])) and not np.array_equal(ac.bits(m1[ok]), ac.bits(m[ok]))


# ---- 2. the stage rules against binary64 ------------------------------------------------------------------------------------------

def test_stages_by_the_k_rule(adam_harness, swept):
    """every coefficient set over the sweep's finite gradients (denormals, 1e19 .. 1e21 and v == 0 with eps 1e-15 among them);
    prints the K needed per stage"""
    p, g, m, v = swept
    fin = np.isfinite(g)
    p, g, m, v = p[fin], g[fin], m[fin], v[fin]
    worst = {"m": 0.0, "v": 0.0, "p": 0.0}
    for cset in ac.COEFF_SETS:
        c = ac.coeffs(*cset)
        p1, m1, v1 = ac.harness_stepped(adam_harness, p, g, m, v, c)
        want = ac.stage64(p, g, m, v, m1, v1, c)
        for stage, got in (("m", m1), ("v", v1), ("p", p1)):
            worst[stage] = max(worst[stage], ac.k_need(got, *want[stage]))
    need = max(worst.values())
    print(f"Adam stages against binary64: K needed m' {worst['m']:.2f}, v' {worst['v']:.2f}, p' {worst['p']:.2f}; K used {ac.K_ADAM}")
    assert need <= ac.K_ADAM <= 16
    # K used is twice the K needed, and the figure on record (adam_cases.K_NEEDED_CPU) is the one measured here
    assert ac.K_ADAM == min(16.0, round(2 * ac.K_NEEDED_CPU, 1)) and abs(need - ac.K_NEEDED_CPU) <= 0.05, (need, ac.K_NEEDED_CPU)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert f"Adam stages: **K needed, measured on the CPU over the value sweep: {ac.K_NEEDED_CPU}" in design


# ---- 3. twenty steps against torch in float64 ---------------------------------------------------------------------------------------

def _run(mode, make, dtype, steps=20):
    """{name: final parameter as float64 numpy} after `steps` steps of the optimizer `make(groups, kwargs)` builds"""
    params = {k: torch.nn.Parameter(torch.from_numpy(v.copy()).to(dtype)) for k, v in ac.init_params().items()}
    opt = make(*ac.reference_groups(params, mode))
    for t in range(steps):
        for k, v in params.items():
            v.grad = torch.from_numpy(ac.gradient(k, t)).to(dtype) if ac.has_gradient(mode, k) else None
        opt.step()
    return {k: v.detach().double().numpy() for k, v in params.items()}, opt


@pytest.mark.parametrize("mode", ["mapping", "tracking"])
def test_twenty_steps_against_torch_in_float64(adam_harness, mode):
    from fisher_rast.optim import FusedAdam
    want, _ = _run(mode, lambda g, kw: torch.optim.Adam(g, **kw), torch.float64)
    theirs, _ = _run(mode, lambda g, kw: torch.optim.Adam(g, **kw), torch.float32)
    backend = ac.HarnessBackend(adam_harness)
    ours, opt = _run(mode, lambda g, kw: FusedAdam(g, backend=backend, **kw), torch.float32)
    assert backend.calls == 20 and set(backend.arrays) == {7 if mode == "tracking" else 5}, "a step fell back to torch"
    start = ac.init_params()
    moved = max(float(np.abs(want[k] - start[k]).max()) for k in want)
    dev_ours = max(float(np.abs(ours[k] - want[k]).max()) for k in want)
    dev_torch = max(float(np.abs(theirs[k] - want[k]).max()) for k in want)
    print(f"{mode}: 20 steps, largest update {moved:.3g}; max |float32 - float64|: ours {dev_ours:.3g}, torch's own {dev_torch:.3g}, "
          f"ratio {dev_ours / dev_torch:.2f}")
    assert moved > 1e-3 and dev_torch > 0
    assert dev_ours <= 2 * dev_torch
    for k in want:
        if ac.LRS[mode][k] == 0:                            # a frozen array keeps its bits (finite gradients), stepped or not
            assert np.array_equal(ours[k], start[k].astype(np.float64)), k


# ---- 4. bookkeeping on the harness backend ------------------------------------------------------------------------------------------

def _pair(adam_harness, mode="mapping", n=257, **extra):
    """(params, FusedAdam over the harness, backend) and (params, torch.optim.Adam) on equal float32 values"""
    from fisher_rast.optim import FusedAdam
    init = ac.init_params(n)
    mk = lambda: {k: torch.nn.Parameter(torch.from_numpy(v.copy())) for k, v in init.items()}
    pa, pb = mk(), mk()
    backend = ac.HarnessBackend(adam_harness)
    ga, kw = ac.reference_groups(pa, mode)
    gb, _ = ac.reference_groups(pb, mode)
    return (pa, FusedAdam(ga, backend=backend, **kw, **extra), backend), (pb, torch.optim.Adam(gb, **kw))


def _set_grads(params, mode, t, n=257):
    for k, v in params.items():
        v.grad = torch.from_numpy(ac.gradient(k, t, n)) if ac.has_gradient(mode, k) else None


def test_state_is_torchs_own_layout(adam_harness):
    (pa, fused, backend), (pb, plain) = _pair(adam_harness)
    for t in range(3):
        _set_grads(pa, "mapping", t)
        _set_grads(pb, "mapping", t)
        fused.step()
        plain.step()
    for k in ac.MAP_KEYS + ac.CAM_KEYS:
        sa, sb = fused.state.get(pa[k], None), plain.state.get(pb[k], None)
        if k in ac.CAM_KEYS:                                   # grad is None: no state, no count, as torch has it
            assert not sa and not sb and pa[k] not in fused.state
            assert torch.equal(pa[k], pb[k])
            continue
        assert set(sa) == set(sb) == {"step", "exp_avg", "exp_avg_sq"}
        assert sa["step"].device.type == "cpu" and sa["step"].dtype == sb["step"].dtype and sa["step"].shape == sb["step"].shape == ()
        assert float(sa["step"]) == float(sb["step"]) == 3.0
        assert sa["exp_avg"].shape == pa[k].shape == sa["exp_avg_sq"].shape and sa["exp_avg"].dtype == torch.float32
        assert torch.allclose(pa[k], pb[k], rtol=0, atol=1e-5)                   # how close is test_twenty_steps_against_torch_in_float64's matter
    assert backend.calls == 3 and backend.arrays == [5, 5, 5]
    # a closure is evaluated once, with gradients enabled, and its loss returned
    seen = []

    def closure():
        seen.append(torch.is_grad_enabled())
        return torch.tensor(4.5)

    assert float(fused.step(closure)) == 4.5 and seen == [True] and backend.calls == 4


def _check_next_step_by_rule(p0, g, m0, v0, c, p1, m1, v1, who):
    """a step from the shared binary32 state (p0, m0, v0): every stage of the result within the K rule of its binary64 evaluation"""
    want = ac.stage64(p0, g, m0, v0, m1, v1, c)
    for stage, got in (("m", m1), ("v", v1), ("p", p1)):
        need = ac.k_need(got, *want[stage])
        assert need <= ac.K_ADAM, (who, stage, need)


def test_state_dict_round_trips_through_a_plain_adam(adam_harness):
    from fisher_rast.optim import FusedAdam
    (pa, fused, backend), (pb, plain) = _pair(adam_harness)
    for t in range(2):
        _set_grads(pa, "mapping", t)
        fused.step()
    with torch.no_grad():
        for k in pa:
            pb[k].copy_(pa[k])
    plain.load_state_dict(copy.deepcopy(fused.state_dict()))          # load_state_dict keeps the tensors it is handed
    # ... and back, into a third optimizer
    pc = {k: torch.nn.Parameter(v.detach().clone()) for k, v in pa.items()}
    gc, kw = ac.reference_groups(pc, "mapping")
    back = FusedAdam(gc, backend=backend, **kw)
    back.load_state_dict(copy.deepcopy(plain.state_dict()))
    before = {k: (pa[k].detach().numpy().copy(), fused.state[pa[k]]["exp_avg"].numpy().copy(), fused.state[pa[k]]["exp_avg_sq"].numpy().copy())
              for k in ac.MAP_KEYS}
    for params in (pa, pb, pc):
        _set_grads(params, "mapping", 2)
    calls = backend.calls
    fused.step(); plain.step(); back.step()
    assert backend.calls == calls + 2
    for k in ac.MAP_KEYS:
        c = ac.coeffs(ac.LRS["mapping"][k], (0.9, 0.999), 1e-15, 3)
        g = ac.gradient(k, 2, 257)
        for who, params, opt in (("fused", pa, fused), ("plain", pb, plain), ("back", pc, back)):
            s = opt.state[params[k]]
            assert float(s["step"]) == 3.0
            _check_next_step_by_rule(*before[k][:1], g, *before[k][1:], c, params[k].detach().numpy(), s["exp_avg"].numpy(), s["exp_avg_sq"].numpy(), (who, k))
        assert np.array_equal(ac.bits(pa[k].detach().numpy()), ac.bits(pc[k].detach().numpy())), k      # the same arithmetic on the same state


def test_skip_frozen_leaves_lr0_groups_without_state(adam_harness):
    (pa, fused, backend), (pb, plain) = _pair(adam_harness, mode="tracking", skip_frozen=True)
    (pc, full, backend_c), _ = _pair(adam_harness, mode="tracking")
    poison = ac.gradient("means3D", 0, 257)
    poison[3] = np.nan
    for t in range(2):
        for params in (pa, pc):
            _set_grads(params, "tracking", t)
            params["means3D"].grad = torch.from_numpy(poison.copy())
        fused.step()
        full.step()
    assert backend.arrays == [2, 2] and backend_c.arrays == [7, 7]
    for k in ac.MAP_KEYS:                                      # lr == 0: no state, no count, and the NaN gradient does not arrive
        assert pa[k] not in fused.state and bool(torch.isfinite(pa[k]).all())
        assert float(full.state[pc[k]]["step"]) == 2.0
    assert bool(torch.isnan(pc["means3D"][3])) and int(torch.isnan(pc["means3D"]).sum()) == 1      # without the option it does, as in torch
    for k in ac.CAM_KEYS:
        assert float(fused.state[pa[k]]["step"]) == 2.0
        assert torch.equal(pa[k], pc[k])


def _fallback_case(adam_harness, what):
    """two optimizers on equal values, outside the fused subset by `what`: (FusedAdam, its params, backend, plain Adam, its params)"""
    from fisher_rast.optim import FusedAdam
    rng = np.random.default_rng(21)
    dtype = torch.float64 if what == "float64" else torch.float32
    a0, b0 = rng.normal(size=(33, 4)), rng.normal(size=(33, 4))
    kw = dict(lr=0.01)
    if what == "amsgrad":
        kw["amsgrad"] = True
    if what == "weight_decay":
        kw["weight_decay"] = 0.1

    def make(cls, **extra):
        x = torch.from_numpy(a0.copy()).to(dtype)
        y = torch.from_numpy(b0.copy()).to(torch.float32)
        if what == "non-contiguous":
            x = x.t()                                          # a transposed leaf: dense, not contiguous
        params = [torch.nn.Parameter(x), torch.nn.Parameter(y)]
        return params, cls([dict(params=[params[0]], name="a"), dict(params=[params[1]], name="b", lr=0.002)], **kw, **extra)

    backend = ac.HarnessBackend(adam_harness)
    pa, fused = make(FusedAdam, backend=backend)
    pb, plain = make(torch.optim.Adam)
    return fused, pa, backend, plain, pb


@pytest.mark.parametrize("what", ["amsgrad", "weight_decay", "float64", "non-contiguous"])
def test_outside_the_fused_subset_the_step_is_torchs(adam_harness, what):
    fused, pa, backend, plain, pb = _fallback_case(adam_harness, what)
    assert not pa[0].is_contiguous() if what == "non-contiguous" else pa[0].is_contiguous()
    rng = np.random.default_rng(22)
    for t in range(3):
        grads = [rng.normal(size=tuple(p.shape)) for p in pa]
        for params in (pa, pb):
            for p, g in zip(params, grads):
                p.grad = torch.from_numpy(g.copy()).to(p.dtype)
        fused.step()
        plain.step()
    assert backend.calls == 0, "the fused backend ran outside its subset"
    for p, q in zip(pa, pb):                                   # it is super().step(): bit for bit
        assert torch.equal(p, q)
        sa, sb = fused.state[p], plain.state[q]
        assert set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_install_replaces_get_optimizer_and_is_opt_in(adam_harness):
    from fisher_rast.optim import FusedAdam
    from models.SLAM.gaussian import FisherOps, GaussianSLAM, OptimizerOps

    class Stub:
        def __init__(self):
            self.config = ac.CONFIG
            self.params = {k: torch.nn.Parameter(torch.from_numpy(v.copy())) for k, v in ac.init_params(5).items()}

    assert not hasattr(Stub, "get_optimizer") and not hasattr(GaussianSLAM, "get_optimizer") and not hasattr(FisherOps, "get_optimizer")
    assert OptimizerOps.install(Stub) is Stub
    s = Stub()
    for tracking in (True, False):
        mode = "tracking" if tracking else "mapping"
        opt = s.get_optimizer(tracking)
        groups, kw = ac.reference_groups(s.params, mode)
        want = torch.optim.Adam(groups, **kw)
        assert isinstance(opt, FusedAdam) and isinstance(opt, torch.optim.Adam) and opt.skip_frozen is False
        assert len(opt.param_groups) == len(want.param_groups) == 7
        for a, b in zip(opt.param_groups, want.param_groups):
            assert a["name"] == b["name"] and a["lr"] == b["lr"] == ac.LRS[mode][a["name"]] and a["params"][0] is b["params"][0] is s.params[a["name"]]
            assert set(a) == set(b) and all(a[k] == b[k] for k in a if k != "params")
            assert a["eps"] == (1e-8 if tracking else 1e-15) and a["betas"] == (0.9, 0.999)
    assert opt.defaults == want.defaults and opt.defaults["lr"] == 0.0
    OptimizerOps.install(Stub, skip_frozen=True)
    assert Stub().get_optimizer(True).skip_frozen is True
    # the graft's optimizer steps like any FusedAdam
    opt = s.get_optimizer(False)
    opt.backend = ac.HarnessBackend(adam_harness)
    for k, v in s.params.items():
        v.grad = torch.ones_like(v) if k in ac.MAP_KEYS else None
    before = s.params["means3D"].detach().clone()
    opt.step()
    assert opt.backend.arrays == [5] and torch.allclose(s.params["means3D"], before - 0.001, rtol=0, atol=1e-6)


# ---- 5. the ABI -----------------------------------------------------------------------------------------------------------------------

def test_abi_is_declared_exported_and_mirrored(adam_harness):
    import __graft_entry__ as g
    g.build()
    from fisher_rast import _lib
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "fisher_rast.h")).read()
    assert re.search(r"\bint\s+fr_adam_step\s*\(\s*const\s+fr_adam_array\s*\*\s*table\s*,\s*int32_t\s+n_arrays\s*,\s*fr_stream_t\s+stream\s*\)\s*;", hdr)
    assert "fr_adam_step" in _lib.EXPORTS and hasattr(lib, "fr_adam_step")
    assert lib.fr_adam_step.restype is ctypes.c_int and len(lib.fr_adam_step.argtypes) == 3
    assert os.path.join(_lib._CSRC, "fr_adam.hip") in _lib.UNITS and os.path.join(_lib._CSRC, "fr_adam_math.h") in _lib.SOURCES
    assert _lib.FR_ADAM_MAX_ARRAYS == adam_harness.fra_max_arrays() == 16 and re.search(r"#define\s+FR_ADAM_MAX_ARRAYS\s+16\b", hdr)
    out = (ctypes.c_longlong * 13)()
    adam_harness.fra_layout(ctypes.addressof(out))
    names = [n for n, _ in _lib.AdamArray._fields_]
    assert names == ["param", "grad", "exp_avg", "exp_avg_sq", "n", "w1", "beta2", "c2", "bc2_sqrt", "eps", "neg_step_size", "fresh"]
    assert ctypes.sizeof(_lib.AdamArray) == out[0]
    assert [getattr(_lib.AdamArray, n).offset for n in names] == list(out[1:])
    # host-side argument checks need no device: nothing is launched for an empty table or for arrays of no element
    assert lib.fr_adam_step(None, 0, None) == 0
    A = _lib.AdamArray
    ok = (1.0, 0.999, 0.001, 1.0, 1e-8, -0.001)
    one = lambda *a: (A * 1)(A(*a))
    assert lib.fr_adam_step(one(None, None, None, None, 0, *ok, 0), 1, None) == 0
    assert lib.fr_adam_step(one(None, None, None, None, -1, *ok, 0), 1, None) == _lib.FR_EINVAL and b"negative" in lib.fr_last_error()
    assert lib.fr_adam_step(one(256, None, 512, 768, 4, *ok, 0), 1, None) == _lib.FR_EINVAL and b"null pointer" in lib.fr_last_error()
    assert lib.fr_adam_step(one(256, 1024, 512, 520, 4, *ok, 0), 1, None) == _lib.FR_EINVAL and b"overlaps" in lib.fr_last_error()
    assert lib.fr_adam_step((A * 17)(), 17, None) == _lib.FR_EINVAL and b"FR_ADAM_MAX_ARRAYS" in lib.fr_last_error()
    assert lib.fr_adam_step(None, -1, None) == _lib.FR_EINVAL
