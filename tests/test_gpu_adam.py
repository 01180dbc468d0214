"""-m gpu: the fused Adam step (fr_adam_step, csrc/fr_adam.hip) and what is written on it (fisher_rast/optim.FusedAdam,
OptimizerOps of models/SLAM/gaussian.py).

Through the C ABI on guarded buffers against the g++ build of the same header (tests/harness/fr_adam_harness.cpp), bit for bit and
NaN-ness for NaNs: one array at every size around a vector, a wave, a chunk and the grid cap, every pointer misaligned in turn,
`fresh`, a table with the map's shapes in one launch, the refusals.  Then FusedAdam on the device against the same sequence on the
harness backend, a map edit between a backward and a step included, and one mapping iteration through the drop-in rasteriser with
the grafted get_optimizer."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adam_cases as ac
import map_edit_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                    # words in front of and behind every buffer (256 bytes: the data keep the allocation's 16-byte alignment)
GUARD_BITS = 0x5A5A5A5A


def _kernel_constant(name):
    src = open(os.path.join(ROOT, "fisher-nerf-customized_amd", "csrc", "fr_adam.hip")).read()
    return int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1))


CHUNK = _kernel_constant("FRA_CHUNK")           # elements a workgroup does at a time
MAX_GRID = _kernel_constant("FRA_MAX_GRID")     # the grid cap: with more chunks than this a workgroup takes a second one
# a vector, a wave, a chunk (CHUNK - 1, CHUNK, CHUNK + 1) and, last, one chunk and a tail more than the capped grid does in one round
SIZES = [0, 1, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, MAX_GRID * CHUNK + CHUNK + 5]


@pytest.fixture(scope="module")
def adam_harness():
    return ac.build_harness()


class _Guarded:
    """a device buffer of n 32-bit words with GUARD words of the guard pattern on both sides; `shift` (0 .. 3 words) misaligns it"""

    def __init__(self, n, dev, init=None, shift=0):
        self.buf = torch.full((n + 2 * GUARD + 4,), GUARD_BITS, dtype=torch.int32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.n, self.o = n, GUARD + shift
        if init is not None:
            self.buf[self.o:self.o + n] = torch.from_numpy(np.ascontiguousarray(init).reshape(-1).view(np.int32)).to(dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.o

    def get(self):
        return self.buf[self.o:self.o + self.n].cpu().numpy().view(np.float32)

    def intact(self):
        return bool((self.buf[:self.o] == GUARD_BITS).all()) and bool((self.buf[self.o + self.n:] == GUARD_BITS).all())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _inputs(n, seed=0):
    """(p, g, m, v) float32 [n] from the CPU sweep, its special gradients (+-0, denormals, 1e19 .. 1e21, NaN, +-inf) first"""
    p, g, m, v = ac.sweep()
    k = ac.SPECIAL_G.size * 3
    order = np.concatenate([np.arange(p.size - k, p.size), np.roll(np.arange(p.size - k), 97 * seed)])
    return tuple(np.resize(a[order], n).astype(ac.F) for a in (p, g, m, v))


def _call(dev, arrays, n_arrays=None):
    """fr_adam_step over `arrays` = [dict(p, g, m, v, c, fresh=False, shift=(0, 0, 0, 0))]: (return code, the guarded buffers per array)"""
    from fisher_rast import _lib
    lib = _lib.load()
    held, entries = [], []
    for a in arrays:
        shift = a.get("shift", (0, 0, 0, 0))
        bufs = [_Guarded(a["p"].size, dev, a[k], s) for k, s in zip("pgmv", shift)]
        held.append(bufs)
        entries.append(_lib.AdamArray(*(b.ptr for b in bufs), a["p"].size, *(float(ac.F(x)) for x in a["c"]), int(a.get("fresh", False))))
    rc = lib.fr_adam_step((_lib.AdamArray * max(len(entries), 1))(*entries), len(entries) if n_arrays is None else n_arrays, _stream(dev))
    torch.cuda.synchronize()
    return rc, held


def _check_against_harness(adam_harness, a, bufs, what):
    want = ac.harness_stepped(adam_harness, a["p"], a["g"], a["m"], a["v"], a["c"], a.get("fresh", False))
    assert all(b.intact() for b in bufs), (what, "a guard word was written")
    assert np.array_equal(ac.bits(bufs[1].get()), ac.bits(a["g"])), (what, "grad was written")
    for name, b, w in zip("pmv", (bufs[0], bufs[2], bufs[3]), want):
        assert ac.same_bits_or_both_nan(b.get(), w), (what, name)


# ---- 6. one array through the C ABI -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", SIZES)
def test_one_array_equals_the_harness_bit_for_bit(gpu, adam_harness, n):
    p, g, m, v = _inputs(n, seed=n % 7)
    for cset in (ac.COEFF_SETS[SIZES.index(n) % len(ac.COEFF_SETS)], ac.COEFF_SETS[3]):
        a = dict(p=p, g=g, m=m, v=v, c=ac.coeffs(*cset))
        rc, held = _call(gpu, [a])
        assert rc == 0
        _check_against_harness(adam_harness, a, held[0], (n, cset))


def test_every_pointer_misaligned_in_turn(gpu, adam_harness):
    """an array with any pointer off a 16-byte boundary takes the 4-byte path: the same bits, no word outside"""
    n = CHUNK + 5
    p, g, m, v = _inputs(n, seed=3)
    for which in range(4):
        for words in (1, 2, 3):                                # 4, 8 and 12 bytes
            shift = tuple(words if k == which else 0 for k in range(4))
            a = dict(p=p, g=g, m=m, v=v, c=ac.coeffs(*ac.COEFF_SETS[(which * 3 + words) % len(ac.COEFF_SETS)]), shift=shift)
            rc, held = _call(gpu, [a])
            assert rc == 0 and held[0][which].ptr % 16 == 4 * words
            _check_against_harness(adam_harness, a, held[0], shift)


# ---- 7. fresh ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", [(0, 0, 0, 0), (0, 0, 1, 0)])
def test_fresh_does_not_read_the_moments(gpu, adam_harness, shift):
    n = 2 * CHUNK + 7
    p, g, _, _ = _inputs(n, seed=5)
    nan_bits = np.full(n, 0x7FC00000, np.uint32).view(ac.F)
    c = ac.coeffs(0.01, (0.9, 0.999), 1e-15, 1)
    fresh = dict(p=p, g=g, m=nan_bits, v=nan_bits, c=c, fresh=True, shift=shift)
    zeros = dict(p=p, g=g, m=np.zeros(n, ac.F), v=np.zeros(n, ac.F), c=c, shift=shift)
    rc1, h1 = _call(gpu, [fresh])
    rc2, h2 = _call(gpu, [zeros])
    assert rc1 == 0 == rc2 and all(b.intact() for b in h1[0] + h2[0])
    for k in (0, 2, 3):
        assert ac.same_bits_or_both_nan(h1[0][k].get(), h2[0][k].get())
    _check_against_harness(adam_harness, zeros, h1[0][:1] + h2[0][1:2] + h1[0][2:], "fresh against the harness on zeros")


# ---- 8. a table with the map's shapes ------------------------------------------------------------------------------------------------

P_MAP = 257
MAP_SHAPES = [(P_MAP, 3), (P_MAP, 3), (P_MAP, 4), (P_MAP, 1), (P_MAP, 1), (P_MAP, 3), (1, 4, 5), (1, 3, 5), (0, 3)]


def _map_table():
    arrays = []
    for i, shape in enumerate(MAP_SHAPES):
        p, g, m, v = _inputs(int(np.prod(shape)), seed=i)
        cset = list(ac.COEFF_SETS[i % len(ac.COEFF_SETS)])
        cset[0] = 0.0 if i == 2 else 0.001 * (i + 1)           # an lr of its own, one array frozen
        arrays.append(dict(p=p, g=g, m=m, v=v, c=ac.coeffs(*cset), fresh=(i == 4)))
    return arrays


def test_a_table_with_the_maps_shapes_in_one_launch(gpu, adam_harness):
    arrays = _map_table()
    bystander = _Guarded(P_MAP * 3, gpu, _inputs(P_MAP * 3, seed=9)[0])           # an array that is not in the table
    rc, held = _call(gpu, arrays)
    assert rc == 0
    for i, (a, bufs) in enumerate(zip(arrays, held)):
        _check_against_harness(adam_harness, a, bufs, MAP_SHAPES[i])
    assert bystander.intact() and np.array_equal(ac.bits(bystander.get()), ac.bits(_inputs(P_MAP * 3, seed=9)[0]))
    frozen = arrays[2]
    ok = np.isfinite(frozen["g"]) & np.isfinite(held[2][3].get())
    assert np.array_equal(ac.bits(held[2][0].get())[ok], ac.bits(frozen["p"])[ok])


def test_refusals_write_nothing_and_leave_the_library_usable(gpu, adam_harness):
    from fisher_rast import _lib
    lib = _lib.load()
    A = _lib.AdamArray
    n = 300
    p, g, m, v = _inputs(n, seed=2)
    c = tuple(float(ac.F(x)) for x in ac.coeffs(0.01, (0.9, 0.999), 1e-8, 2))
    big = _Guarded(8 * n, gpu, np.resize(p, 8 * n))
    before = big.buf.clone()
    at = lambda k: big.ptr + 4 * n * k

    def call(entries, count=None):
        rc = lib.fr_adam_step((A * len(entries))(*entries), len(entries) if count is None else count, _stream(gpu))
        torch.cuda.synchronize()
        return rc

    good = A(at(0), at(1), at(2), at(3), n, *c, 0)
    other = A(at(4), at(5), at(6), at(7), n, *c, 0)
    assert call([good] * 17) == _lib.FR_EINVAL and b"FR_ADAM_MAX_ARRAYS" in lib.fr_last_error()            # 17 entries
    assert call([good], count=-1) == _lib.FR_EINVAL
    assert call([good, A(at(4), at(5), at(6), at(3) + 4 * (n - 1), n, *c, 0)]) == _lib.FR_EINVAL and b"overlaps" in lib.fr_last_error()
    assert call([good, good]) == _lib.FR_EINVAL                                                             # the same array twice
    assert call([A(at(0), at(1), at(0), at(3), n, *c, 0)]) == _lib.FR_EINVAL                                # exp_avg is param
    assert call([good, A(at(4), at(2), at(6), at(7), n, *c, 0)]) == _lib.FR_EINVAL                          # a gradient that another entry writes
    assert call([A(at(0), None, at(2), at(3), n, *c, 0)]) == _lib.FR_EINVAL and b"null pointer" in lib.fr_last_error()
    assert call([A(at(0), at(1), at(2), at(3), -1, *c, 0)]) == _lib.FR_EINVAL
    assert call([A(at(0), at(1), at(2), at(3), n, *c, 2)]) == _lib.FR_EINVAL                                # fresh is 0 or 1
    assert torch.equal(big.buf, before), "a refused call wrote"
    # two entries may share a gradient (it is only read); arrays of no element and null pointers with n == 0 launch nothing
    assert call([A(None, None, None, None, 0, *c, 0)]) == 0 and call([]) == 0 and torch.equal(big.buf, before)
    shared = A(at(4), at(1), at(6), at(7), n, *c, 0)
    assert call([good, shared]) == 0 and big.intact()
    words = big.get().reshape(8, n)
    base = np.resize(p, 8 * n).reshape(8, n)
    for rows in ((0, 2, 3), (4, 6, 7)):
        want = ac.harness_stepped(adam_harness, base[rows[0]], base[1], base[rows[1]], base[rows[2]], ac.coeffs(0.01, (0.9, 0.999), 1e-8, 2))
        for r, w in zip(rows, want):
            assert ac.same_bits_or_both_nan(words[r], w)
    assert np.array_equal(ac.bits(words[[1, 5]]), ac.bits(base[[1, 5]]))


def test_nineteen_arrays_through_fused_adam_take_two_launches(gpu, adam_harness):
    from fisher_rast import optim
    launches = []

    class Backend(optim.HipAdamBackend):
        @staticmethod
        def step(entries):
            launches.append(-(-len(entries) // 16))
            return optim.HipAdamBackend.step(entries)

    rng = np.random.default_rng(19)
    init = [rng.normal(size=(11 + 37 * i,)).astype(ac.F) for i in range(19)]
    grads = [[(rng.normal(size=a.shape) * 10.0 ** (i % 5 - 2)).astype(ac.F) for i, a in enumerate(init)] for _ in range(3)]

    def run(dev, backend):
        params = [torch.nn.Parameter(torch.from_numpy(a.copy()).to(dev)) for a in init]
        opt = optim.FusedAdam([dict(params=[p], lr=1e-3 * (i + 1)) for i, p in enumerate(params)], backend=backend)
        for step in grads:
            for p, g in zip(params, step):
                p.grad = torch.from_numpy(g.copy()).to(dev)
            opt.step()
        return [p.detach().cpu().numpy() for p in params] + [opt.state[p][k].cpu().numpy() for p in params for k in ("exp_avg", "exp_avg_sq")]

    got = run(gpu, Backend())
    torch.cuda.synchronize()
    want = run("cpu", ac.HarnessBackend(adam_harness))
    assert launches == [2, 2, 2]
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(ac.bits(a), ac.bits(b)), i


# ---- 9. FusedAdam on the device ---------------------------------------------------------------------------------------------------------

def _gradient(key, t, shape):
    rng = np.random.default_rng([(ac.MAP_KEYS + ac.CAM_KEYS).index(key), t, 7])
    g = rng.normal(size=shape) * 10.0 ** rng.uniform(-3, 1)
    g.reshape(-1)[::7] = 0.0
    return g.astype(ac.F)


DENSIFY_AT, PRUNE_AT = 5, 11


def _sequence(mode, dev, st, edit, backend, steps=20, sync_check=False):
    """`steps` steps of FusedAdam in the reference's configuration `mode`; a densify between the backward and the step of iteration
    DENSIFY_AT and a prune_gaussians at PRUNE_AT.  Returns (params, optimizer, what the edits left)."""
    from fisher_rast.optim import FusedAdam
    params, variables, _ = mc.build_inputs(st, dev, optimizer=False)
    groups, kw = ac.reference_groups(params, mode)
    opt = FusedAdam(groups, backend=backend, **kw)
    info = {}
    for t in range(steps):
        for k, v in params.items():
            v.grad = torch.from_numpy(_gradient(k, t, tuple(v.shape))).to(dev) if ac.has_gradient(mode, k) else None
        if t == DENSIFY_AT:
            rows = params["means3D"].shape[0]
            params, variables = edit.densify(params, variables, opt, 20, dict(mc.DENSIFY, removal_opacity_threshold=0.0))     # its second stage removes no row
            info["densified"] = (rows, params["means3D"].shape[0])
            info["after_densify"] = {k: params[k].detach().cpu().numpy().copy() for k in ac.MAP_KEYS}
        if t == PRUNE_AT:
            rows = params["means3D"].shape[0]
            params, variables = edit.prune_gaussians(params, variables, opt, 20, dict(mc.PRUNE, removal_opacity_threshold=0.4))
            info["pruned"] = (rows, params["means3D"].shape[0])
        if t in (DENSIFY_AT, PRUNE_AT):
            # the edit replaced the map's parameters: they have no gradient, so this step passes them over, as torch's does
            assert all(params[k].grad is None for k in ac.MAP_KEYS)
            counts = {k: float(opt.state[params[k]]["step"]) for k in ac.MAP_KEYS if params[k] in opt.state}
        if sync_check and t in (0, 3) and hasattr(torch.cuda, "set_sync_debug_mode"):
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                opt.step()                                     # raises on a device -> host read or a synchronising call
            finally:
                torch.cuda.set_sync_debug_mode("default")
        else:
            opt.step()
        if t in (DENSIFY_AT, PRUNE_AT):
            assert counts == {k: float(opt.state[params[k]]["step"]) for k in ac.MAP_KEYS if params[k] in opt.state}, "a skipped array was counted"
        if t == DENSIFY_AT:
            info["moments_after_densify"] = {k: opt.state[params[k]]["exp_avg"].cpu().numpy().copy() for k in ac.MAP_KEYS if params[k] in opt.state}
    return params, opt, info


def _device_edit(st):
    from models.SLAM.utils import slam_external as se

    class Backend(se.HipMapEditBackend):
        def __init__(self):
            self.plans = []

        def plan(self, *a, **k):
            out = super().plan(*a, **k)
            self.plans.append(out[0])
            return out

        def randn(self, rows, like, generator=None):
            return torch.from_numpy(np.ascontiguousarray(st["z"][:rows])).to(like.device)

    backend = Backend()
    return se.MapEdit(backend), backend


@pytest.mark.parametrize("mode", ["mapping", "tracking"])
def test_fused_adam_on_the_device_equals_the_harness_backend(gpu, adam_harness, oracle, mode):
    """Both sides run the product's own MapEdit (kernels here, the NumPy backend there).  The split children's log scales go through
    the platform's logf, which the two sides need not round alike, so the CPU side takes the device's child log
    scales -- held to the rule for them first -- and every later step is compared bit for bit on equal inputs."""
    from fisher_rast import optim
    from models.SLAM.utils import slam_external as se
    st = mc.make_state(P_MAP, 3, 31)
    edit_d, eb = _device_edit(st)

    class CpuEdit(se.MapEdit):
        """after the densify, the log scales are the device's: equal but for the children's, which lie within the rule for them"""
        device_log_scales = None

        def densify(self, params, variables, optimizer, *a, **k):
            params, variables = super().densify(params, variables, optimizer, *a, **k)
            got, dev = params["log_scales"].detach().numpy(), self.device_log_scales
            assert got.shape == dev.shape
            assert np.all(np.abs(got.astype(np.float64) - dev) <= 2 * np.spacing(np.abs(got)) + 2.0 ** -23), "log scales beyond the logf rule"
            with torch.no_grad():
                params["log_scales"].copy_(torch.from_numpy(dev))
            return params, variables

    p_d, opt_d, info_d = _sequence(mode, gpu, st, edit_d, optim.HipAdamBackend(), sync_check=True)
    torch.cuda.synchronize()
    edit_c = CpuEdit(mc.NumpyBackend(mc.build_harness(), st["z"]))
    edit_c.device_log_scales = info_d["after_densify"]["log_scales"]
    p_c, opt_c, info_c = _sequence(mode, "cpu", st, edit_c, ac.HarnessBackend(adam_harness))
    # the edits happened, with clones and children, and removed rows
    stage1 = eb.plans[0]
    assert stage1.n_clone > 0 and stage1.n_split > 0 and info_d["densified"] == info_c["densified"] and info_d["densified"][1] != P_MAP
    assert info_d["pruned"] == info_c["pruned"] and info_d["pruned"][1] < info_d["pruned"][0]
    for k in ac.MAP_KEYS:
        if k != "log_scales":
            assert np.array_equal(ac.bits(info_d["after_densify"][k]), ac.bits(info_c["after_densify"][k])), k
    # the appended moment rows start at zero, and the step that followed the edit left them there (no gradient: skipped)
    assert info_d["densified"][1] == stage1.rows and set(info_d["moments_after_densify"]) == set(ac.MAP_KEYS)
    for k, m in info_d["moments_after_densify"].items():
        assert m.shape[0] == stage1.rows and not m[stage1.n_keep:].any() and m[:stage1.n_keep].any(), k
    for k in ac.MAP_KEYS + ac.CAM_KEYS:
        a, b = p_d[k].detach().cpu().numpy(), p_c[k].detach().numpy()
        assert a.shape == b.shape and np.array_equal(ac.bits(a), ac.bits(b)), k
        sa, sb = opt_d.state.get(p_d[k], None), opt_c.state.get(p_c[k], None)
        assert bool(sa) == bool(sb) == ac.has_gradient(mode, k), k
        if sa:
            want_steps = 20.0 if k in ac.CAM_KEYS else 18.0             # the two steps that followed an edit passed the map over
            assert float(sa["step"]) == float(sb["step"]) == want_steps and sa["step"].device.type == "cpu", k
            for key in ("exp_avg", "exp_avg_sq"):
                assert sa[key].is_cuda and np.array_equal(ac.bits(sa[key].cpu().numpy()), ac.bits(sb[key].numpy())), (k, key)


# ---- 10. the graft in one mapping iteration ---------------------------------------------------------------------------------------------

def test_install_in_a_mapping_iteration_with_the_drop_in_rasteriser(gpu):
    """render -> loss -> backward -> optimizer.step() three times with the grafted get_optimizer: the loss falls.  The gradients of
    such an iteration depend on the parameters (and on the order of the rasteriser's atomic sums), so the comparison with the torch
    optimizer is made on the gradients the torch run saw: FusedAdam, fed those, against torch.optim.Adam in float64 fed the same,
    within twice the deviation of the torch run itself (the rule of test_twenty_steps_against_torch_in_float64)."""
    from fisher_rast import optim, synthetic
    from models.SLAM.gaussian import OptimizerOps
    from models.SLAM.utils.recon_helpers import setup_camera
    from models.SLAM.utils.slam_helpers import render_rgb_depth_sil
    P, W, H = 5000, 64, 64
    init = {k: v.contiguous() for k, v in synthetic.room_shell(P, seed=9).items()}
    init["cam_unnorm_rots"] = torch.tensor([[[1.0], [0.0], [0.0], [0.0]]])
    init["cam_trans"] = torch.zeros((1, 3, 1))
    cam = setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4), device=gpu)
    w2c = synthetic.invert_rigid(synthetic.candidate_poses(1, seed=10))[0].to(gpu)

    class Slam:
        """the reference's attributes and its get_optimizer"""

        def __init__(self, dtype=torch.float32):
            self.config = ac.CONFIG
            self.params = {k: torch.nn.Parameter(v.to(gpu, dtype).requires_grad_(True)) for k, v in init.items()}

        def get_optimizer(self, tracking):
            groups, kw = ac.reference_groups(self.params, "tracking" if tracking else "mapping")
            return torch.optim.Adam(groups, **kw)

    class Grafted(Slam):
        pass

    assert OptimizerOps.install(Grafted) is Grafted and Slam.get_optimizer is not Grafted.get_optimizer

    def loss_of(params):
        pts = params['means3D']
        tp = (w2c @ torch.cat((pts, torch.ones_like(pts[:, :1])), 1).T).T[:, :3]
        im, radius, depth_sil, rv = render_rgb_depth_sil(params, cam, w2c, tp)
        return (im - 0.3).abs().sum() + 0.5 * (depth_sil[0] - 2.0).abs().sum()

    def iterate(slam, record):
        opt = slam.get_optimizer(False)
        losses = []
        for it in range(3):
            opt.zero_grad(set_to_none=True)
            loss = loss_of(slam.params)
            loss.backward()
            losses.append(float(loss.detach()))
            record.append({k: None if v.grad is None else v.grad.detach().clone() for k, v in slam.params.items()})
            opt.step()
        losses.append(float(loss_of(slam.params).detach()))            # the render keeps means2D's gradient: not under no_grad
        return opt, losses

    def replay(slam, grads):
        opt = slam.get_optimizer(False)
        for step in grads:
            for k, v in slam.params.items():
                v.grad = None if step[k] is None else step[k].to(v.dtype).clone()
            opt.step()
        return opt

    seen, grafted_seen = [], []
    plain = Slam()
    iterate(plain, seen)
    assert all(step[k] is not None for step in seen for k in ac.MAP_KEYS) and all(step[k] is None for step in seen for k in ac.CAM_KEYS)
    grafted = Grafted()
    opt, losses = iterate(grafted, grafted_seen)
    assert isinstance(opt, optim.FusedAdam) and isinstance(opt.backend, optim.HipAdamBackend)
    print("loss before and after three fused steps:", losses)
    assert losses[-1] < losses[0]
    for k in ac.MAP_KEYS:
        s = opt.state[grafted.params[k]]
        assert float(s["step"]) == 3.0 and s["exp_avg"].is_cuda and bool(torch.isfinite(grafted.params[k]).all()), k
    assert all(grafted.params[k] not in opt.state for k in ac.CAM_KEYS)
    ours, exact = Grafted(), Slam(torch.float64)
    assert isinstance(replay(ours, seen), optim.FusedAdam)
    replay(exact, seen)
    torch.cuda.synchronize()
    dev_ours = max(float((ours.params[k].detach().double() - exact.params[k].detach()).abs().max()) for k in ac.MAP_KEYS)
    dev_torch = max(float((plain.params[k].detach().double() - exact.params[k].detach()).abs().max()) for k in ac.MAP_KEYS)
    moved = max(float((exact.params[k].detach() - init[k].to(gpu).double()).abs().max()) for k in ac.MAP_KEYS)
    print(f"three mapping steps, largest update {moved:.3g}; max |float32 - float64|: ours {dev_ours:.3g}, the torch run's {dev_torch:.3g}")
    assert moved > 1e-3 and dev_torch > 0
    assert dev_ours <= 2 * dev_torch
