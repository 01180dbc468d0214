"""-m gpu: the fused render-variable build (fr_rendervar_forward / fr_rendervar_backward, csrc/fr_rendervar.hip) and what is written on
it (fisher_rast/rendervar.FrameRenderVars, frame_render_vars of models/SLAM/utils/slam_helpers.py, make_get_loss(fused_rendervar=True)).

Through the C ABI on guarded buffers against the g++ build of the same header (tests/harness/fr_rendervar_harness.cpp): the forward
and the per-Gaussian backward bit for bit and NaN for NaN, the seven camera gradients within the sums' allowance at that P carried
through the tail, and the same bits on a second call -- at every size around a wave, a workgroup and the grid cap, every per-row
pointer misaligned in turn, every nullable pointer null in turn, three frames with NaN in the others, the special rows.  Then
FrameRenderVars on the device against the binary64 chain with torch's own float32 chain beside it, without a host synchronisation,
and one get_loss through the drop-in rasteriser with the flag on and off."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import rendervar_cases as rc
from gpu_util import assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64                    # words in front of and behind every buffer
GUARD_BITS = 0x5A5A5A5A


def _kernel_constant(name):
    src = open(os.path.join(ROOT, "fisher-nerf-customized_amd", "csrc", "fr_rendervar.hip")).read()
    return int(re.search(rf"#define\s+{name}\s+(\d+)", src).group(1))


THREADS = _kernel_constant("FRV_THREADS")       # rows a workgroup does at a time
MAX_GRID = _kernel_constant("FRV_MAX_GRID")     # the grid cap: with more rows than THREADS * MAX_GRID a thread takes a second one
# around a wave, around a workgroup and, last, one workgroup and a tail more than the capped grid does in one round
SIZES = [0, 1, 3, 63, 64, 65, THREADS - 1, THREADS, THREADS + 1, MAX_GRID * THREADS + THREADS + 5]

INPUTS = rc.PARAMS + ("first_frame_w2c",)
FORWARD_OUT = rc.OUTPUTS + ("rel_w2c",)
PER_ROW = ("means3D", "unnorm_rotations", "logit_opacities", "log_scales") + rc.OUTPUTS + rc.UPSTREAM + rc.GRADS[:4]
# an incoming gradient that is null counts as zero: the gradient it alone feeds is written as zeros
FEEDS = {"g_rotations": "g_unnorm_rotations", "g_opacities": "g_logit_opacities", "g_scales": "g_log_scales"}


@pytest.fixture(scope="module")
def rv_harness():
    return rc.build_harness()


class _Guarded:
    """a device buffer of n 32-bit words with GUARD words of the guard pattern on both sides; `shift` (0 .. 3 words) misaligns it.
    Without `init` the data words hold the guard pattern too."""

    def __init__(self, n, dev, init=None, shift=0):
        self.buf = torch.full((n + 2 * GUARD + 4,), GUARD_BITS, dtype=torch.int32, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.n, self.o = n, GUARD + shift
        if init is not None:
            self.buf[self.o:self.o + n] = torch.from_numpy(np.ascontiguousarray(init).reshape(-1).view(np.int32)).to(dev)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * self.o

    def get(self, shape=None):
        a = self.buf[self.o:self.o + self.n].cpu().numpy().view(np.float32)
        return a if shape is None else a.reshape(shape)

    def intact(self):
        return bool((self.buf[:self.o] == GUARD_BITS).all()) and bool((self.buf[self.o + self.n:] == GUARD_BITS).all())

    def untouched(self):
        return bool((self.buf == GUARD_BITS).all())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _shapes(P, cols, frames):
    return {"pts": (P, 3), "feats": (P, 3), "rotations": (P, 4), "opacities": (P, 1), "scales": (P, 3), "rel_w2c": (4, 4),
            "g_means3D": (P, 3), "g_unnorm_rotations": (P, 4), "g_logit_opacities": (P, 1), "g_log_scales": (P, cols),
            "g_cam_unnorm_rots": (1, 4, frames), "g_cam_trans": (1, 3, frames)}


def _skipped(skip, gaussians_grad, camera_grad):
    skip = set(skip)
    if not gaussians_grad:
        skip.add("g_means3D")
    if not camera_grad:
        skip |= {"g_cam_unnorm_rots", "g_cam_trans"}
    return skip


def _device_run(dev, inp, t, gaussians_grad=True, camera_grad=True, skip=(), shift=None, twice=False):
    """fr_rendervar_forward then fr_rendervar_backward on guarded copies of `inp`: ({name: array} of what was written, the buffers).
    Names in `skip` are passed as null pointers (their buffers exist and must stay untouched); `shift` = {name: words}."""
    from fisher_rast import _lib
    lib = _lib.load()
    P, cols, frames = inp["means3D"].shape[0], inp["log_scales"].shape[1], inp["cam_trans"].shape[2]
    shift = shift or {}
    skip = _skipped(skip, gaussians_grad, camera_grad)
    shapes = _shapes(P, cols, frames)
    bufs = {k: _Guarded(inp[k].size, dev, inp[k], shift.get(k, 0)) for k in INPUTS + rc.UPSTREAM}
    bufs.update({k: _Guarded(int(np.prod(s)), dev, None, shift.get(k, 0)) for k, s in shapes.items()})
    nws = int(lib.fr_rendervar_workspace_bytes(P))
    ws = _Guarded(nws // 4, dev)
    ptr = lambda names: {k: bufs[k].ptr for k in names if k not in skip}
    dims = dict(P=P, scale_cols=cols, time_idx=t, n_frames=frames)
    fwd = _lib.RenderVarCfg(**dims, **ptr(INPUTS + FORWARD_OUT))
    bwd = _lib.RenderVarCfg(**dims, **ptr(INPUTS + rc.UPSTREAM + rc.GRADS))
    assert lib.fr_rendervar_forward(ctypes.byref(fwd), _stream(dev)) == 0, lib.fr_last_error()
    assert lib.fr_rendervar_backward(ctypes.byref(bwd), ws.ptr, nws, _stream(dev)) == 0, lib.fr_last_error()
    torch.cuda.synchronize()
    got = {k: bufs[k].get(shapes[k]) for k in shapes if k not in skip}
    if twice:                                              # the same bits on every call, the camera's sums included
        first = {k: bufs[k].buf.clone() for k in shapes}
        ws.buf.fill_(GUARD_BITS)
        assert lib.fr_rendervar_forward(ctypes.byref(fwd), _stream(dev)) == 0 and lib.fr_rendervar_backward(ctypes.byref(bwd), ws.ptr, nws, _stream(dev)) == 0
        torch.cuda.synchronize()
        assert all(torch.equal(first[k], bufs[k].buf) for k in shapes), "a second call gave other bits"
    # every guard intact, the inputs as they were, what was not asked for not written
    assert ws.intact() and all(b.intact() for b in bufs.values()), [k for k, b in bufs.items() if not b.intact()]
    for k in INPUTS + rc.UPSTREAM:
        assert np.array_equal(rc.bits(bufs[k].get()), rc.bits(inp[k]).reshape(-1)), k
    assert all(bufs[k].untouched() for k in shapes if k in skip), [k for k in shapes if k in skip and not bufs[k].untouched()]
    return got, skip


def _check_against_harness(rv_harness, inp, t, got, skip, gaussians_grad=True, camera_grad=True, what=None):
    P = inp["means3D"].shape[0]
    want = rc.harness_run(rv_harness, inp, t, gaussians_grad, camera_grad, skip=skip)
    assert set(got) == set(want) - {"G", "sums"}, (what, set(got) ^ set(want))
    for k, g in got.items():
        if k not in ("g_cam_unnorm_rots", "g_cam_trans"):
            assert rc.same_bits_or_both_nan(g, want[k]), (what, k)
    present = [k for k in ("g_cam_unnorm_rots", "g_cam_trans") if k in got]
    if present:
        others = [f for f in range(inp["cam_trans"].shape[2]) if f != t]
        assert not any(rc.bits(got[k])[0][:, others].any() for k in present), what
        sel = np.concatenate([np.arange(4) if k == "g_cam_unnorm_rots" else np.arange(4, 7) for k in present])
        seven = np.concatenate([got[k][0, :, t] for k in present]).astype(np.float64)
        if P == 0:
            assert not rc.bits(seven.astype(rc.F)).any()
        elif np.isfinite(want["sums"]).all() and np.isfinite(inp["cam_unnorm_rots"][0, :, t]).all() and inp["cam_unnorm_rots"][0, :, t].any():
            w7, bound = rc.camera_bound(inp, t, want, P)
            print(f"{what}: camera gradients, largest deviation / bound {float((np.abs(seven - w7[sel]) / bound[sel]).max()):.3f}")
            assert (np.abs(seven - w7[sel]) <= bound[sel]).all(), (what, seven, w7[sel], bound[sel])
        else:
            h7 = np.concatenate([want[k][0, :, t] for k in present])
            assert np.array_equal(np.isnan(seven), np.isnan(h7)), what


# ---- 1. sizes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", SIZES)
def test_kernels_equal_the_harness(gpu, rv_harness, P):
    cols = 1 if SIZES.index(P) % 2 else 3
    for (gg, cg), c in (((True, True), 3), ((True, False), cols), ((False, True), cols)):
        inp = rc.make_inputs(P, c, seed=1)
        got, skip = _device_run(gpu, inp, 1, gg, cg, twice=True)
        _check_against_harness(rv_harness, inp, 1, got, skip, gg, cg, what=(P, c, gg, cg))


# ---- 2. pointers ------------------------------------------------------------------------------------------------------------------------

def test_every_per_row_pointer_misaligned_in_turn(gpu, rv_harness):
    """rows of 4, 12 and 16 bytes at any 4-byte address: the same bits, no word outside"""
    P = THREADS + 1                                            # (a size whose sums have their figure on record)
    for i, name in enumerate(PER_ROW):
        for words in (1, 2, 3):                                # 4, 8 and 12 bytes
            cols = 1 if (i + words) % 2 else 3
            inp = rc.make_inputs(P, cols, seed=2)
            got, skip = _device_run(gpu, inp, 3, shift={name: words})
            _check_against_harness(rv_harness, inp, 3, got, skip, what=(name, words, cols))


def test_all_pointers_misaligned_by_every_shift(gpu, rv_harness):
    P = 2000
    for words in (1, 2, 3):
        inp = rc.make_inputs(P, 3, seed=3)
        got, skip = _device_run(gpu, inp, 0, shift={name: words for name in PER_ROW})
        _check_against_harness(rv_harness, inp, 0, got, skip, what=words)


def test_every_nullable_pointer_null_in_turn(gpu, rv_harness):
    """a null output or incoming gradient is a part that is not computed / not read: the rest has the harness's bits, and the buffer
    behind the null pointer is not written"""
    P = THREADS + 1
    inp = rc.make_inputs(P, 3, seed=4)
    for name in FORWARD_OUT + rc.UPSTREAM + rc.GRADS:
        got, skip = _device_run(gpu, inp, 2, skip=(name,))
        assert name not in got
        if name in FEEDS:
            assert not rc.bits(got[FEEDS[name]]).any(), name
        _check_against_harness(rv_harness, inp, 2, got, skip, camera_grad="g_cam_unnorm_rots" in got or "g_cam_trans" in got, what=name)
    # a plain transform_to_frame: the points alone
    got, skip = _device_run(gpu, inp, 2, skip=[k for k in FORWARD_OUT + rc.UPSTREAM + rc.GRADS if k != "pts"])
    assert set(got) == {"pts"}
    assert rc.same_bits_or_both_nan(got["pts"], rc.harness_run(rv_harness, inp, 2)["pts"])


# ---- 3. frames and special rows ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("t", [0, 2, 4])
def test_only_the_addressed_frame_is_read(gpu, rv_harness, t):
    inp = rc.make_inputs(THREADS - 1, 1, seed=5)
    for k in ("cam_unnorm_rots", "cam_trans"):
        keep = inp[k][0, :, t].copy()
        inp[k][:] = np.nan
        inp[k][0, :, t] = keep
    got, skip = _device_run(gpu, inp, t)
    assert all(np.isfinite(v).all() for v in got.values())
    _check_against_harness(rv_harness, inp, t, got, skip, what=t)


@pytest.mark.parametrize("cols", [1, 3])
def test_special_rows_do_not_fault_and_equal_the_harness(gpu, rv_harness, cols):
    inp = rc.special_inputs(cols)
    for gg, cg in ((True, False), (False, True)):
        got, skip = _device_run(gpu, inp, 1, gg, cg)
        _check_against_harness(rv_harness, inp, 1, got, skip, gg, cg, what=("special", cols, gg, cg))
    assert np.isposinf(got["scales"][3, 0]) and got["opacities"][2, 0] == 0.0 and np.isnan(got["pts"][5]).all()
    zero = rc.make_inputs(70, cols, seed=6)
    zero["cam_unnorm_rots"][0, :, 1] = 0.0                     # a NaN pose, as in the reference
    got, skip = _device_run(gpu, zero, 1)
    _check_against_harness(rv_harness, zero, 1, got, skip, what="zero camera quaternion")
    assert np.isnan(got["pts"]).all() and np.isnan(got["g_cam_unnorm_rots"][0, :, 1]).all() and np.isfinite(got["rotations"]).all()
    nan_w2c = rc.make_inputs(70, cols, seed=6)
    nan_w2c["first_frame_w2c"][2, 1] = np.nan                  # the row the depth features are taken with
    got, skip = _device_run(gpu, nan_w2c, 1)
    _check_against_harness(rv_harness, nan_w2c, 1, got, skip, what="NaN in first_frame_w2c")
    assert np.isnan(got["feats"][:, [0, 2]]).all() and np.isfinite(got["pts"]).all() and np.isnan(got["g_means3D"]).all()


def test_refusals_write_nothing(gpu):
    from fisher_rast import _lib
    lib = _lib.load()
    inp = rc.make_inputs(40, 3, seed=7)
    bufs = {k: _Guarded(inp[k].size, gpu, inp[k]) for k in INPUTS + rc.UPSTREAM}
    bufs.update({k: _Guarded(int(np.prod(s)), gpu) for k, s in _shapes(40, 3, 5).items()})
    ws = _Guarded(12, gpu)
    full = dict(P=40, scale_cols=3, time_idx=1, n_frames=5, **{k: b.ptr for k, b in bufs.items()})

    def both(**kw):
        cfg = _lib.RenderVarCfg(**{**full, **kw})
        return (lib.fr_rendervar_forward(ctypes.byref(cfg), _stream(gpu)), lib.fr_rendervar_backward(ctypes.byref(cfg), ws.ptr, 48, _stream(gpu)))

    E = _lib.FR_EINVAL
    assert both(P=-1) == (E, E) and both(scale_cols=2) == (E, E) and both(time_idx=5) == (E, E) and both(time_idx=-1) == (E, E)
    assert both(means3D=None) == (E, E) and both(cam_unnorm_rots=None) == (E, E) and both(first_frame_w2c=None) == (E, E)
    assert both(log_scales=None) == (E, E)
    cfg = _lib.RenderVarCfg(**full)
    assert lib.fr_rendervar_backward(ctypes.byref(cfg), ws.ptr, 47, _stream(gpu)) == _lib.FR_ENOSPACE
    assert lib.fr_rendervar_backward(ctypes.byref(cfg), None, 48, _stream(gpu)) == E
    torch.cuda.synchronize()
    assert all(b.untouched() for k, b in bufs.items() if k not in INPUTS + rc.UPSTREAM) and ws.untouched()
    # ... and the library is usable afterwards
    assert both() == (0, 0)
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs.values()) and not bufs["pts"].untouched()


# ---- 4. FrameRenderVars on the device ---------------------------------------------------------------------------------------------------

def _device_leaves(inp, dev):
    return {k: torch.from_numpy(inp[k].copy()).to(dev).requires_grad_(True) for k in rc.PARAMS}


def _apply(p, inp, dev, t, gg, cg):
    from fisher_rast.rendervar import FrameRenderVars
    return FrameRenderVars.apply(p["means3D"], p["unnorm_rotations"], p["logit_opacities"], p["log_scales"], p["cam_unnorm_rots"], p["cam_trans"],
                                 t, torch.from_numpy(inp["first_frame_w2c"]).to(dev), gg, cg)


@pytest.mark.parametrize("mode", ["mapping", "tracking"])
@pytest.mark.parametrize("cols", [1, 3])
def test_frame_render_vars_on_the_device_by_the_stage_rule(gpu, rv_harness, mode, cols):
    P, t = 1000, 2
    gg, cg = mode == "mapping", mode == "tracking"
    inp = rc.make_inputs(P, cols, seed=21)
    p = _device_leaves(inp, gpu)
    outs = _apply(p, inp, gpu, t, gg, cg)
    up = [torch.from_numpy(inp[g]).to(gpu) for g in rc.UPSTREAM]
    torch.autograd.backward(outs, up)
    torch.cuda.synchronize()
    got = {name: o.detach().cpu().numpy() for name, o in zip(rc.OUTPUTS, outs)}
    got.update({"g_" + k: v.grad.cpu().numpy() for k, v in p.items() if v.grad is not None})
    assert ("g_means3D" in got) == gg and ("g_cam_unnorm_rots" in got) == cg and ("g_cam_trans" in got) == cg
    assert {"g_unnorm_rotations", "g_logit_opacities", "g_log_scales"} <= set(got)
    host = rc.harness_run(rv_harness, inp, t, gg, cg)
    vals = {**got, "rel_w2c": host["rel_w2c"], "G": host["G"]}
    need = {s: rc.k_need(*tr) for s, tr in rc.stages(inp, t, vals).items() if s not in ("sums", "tail", "pose")}
    print(f"{mode}, {cols} scale column(s): K needed on the device " + ", ".join(f"{s} {k:.2f}" for s, k in sorted(need.items())))
    for s, k in need.items():
        assert k <= rc.allowed(s), (s, k, rc.allowed(s))
    if cg:
        assert got["g_cam_unnorm_rots"].shape == (1, 4, rc.T_FRAMES) and got["g_cam_trans"].shape == (1, 3, rc.T_FRAMES)
        seven = np.concatenate([got["g_cam_unnorm_rots"][0, :, t], got["g_cam_trans"][0, :, t]]).astype(np.float64)
        w7, bound = rc.camera_bound(inp, t, host, P)
        assert (np.abs(seven - w7) <= bound).all(), (seven, w7, bound)
        assert not got["g_cam_unnorm_rots"][0, :, [0, 1, 3, 4]].any() and not got["g_cam_trans"][0, :, [0, 1, 3, 4]].any()
    # the binary64 chain, with torch's own float32 chain on the device beside ours
    exact = rc.torch_chain(inp, t, gg, cg)
    theirs = rc.torch_chain(inp, t, gg, cg, dtype=torch.float32, device=gpu)
    for k in sorted(got):
        e = exact[k].numpy()
        scale = max(float(np.abs(e).max()), 1e-30)
        ours_dev, torch_dev = float(np.abs(got[k] - e).max()) / scale, float(np.abs(theirs[k].cpu().double().numpy() - e).max()) / scale
        print(f"  {k}: max |float32 - float64| / max |float64|: ours {ours_dev:.2e}, torch's own {torch_dev:.2e}")
        assert ours_dev <= 1e-5, k


def test_forward_and_backward_without_a_host_synchronisation(gpu):
    inp = rc.make_inputs(3000, 1, seed=22)
    for gg, cg in ((True, False), (False, True)):
        p = _device_leaves(inp, gpu)
        up = [torch.from_numpy(inp[g]).to(gpu) for g in rc.UPSTREAM]
        torch.autograd.backward(_apply(p, inp, gpu, 1, gg, cg), up)            # the workspace and the allocator's pools exist now
        for v in p.values():
            v.grad = None
        w2c = torch.from_numpy(inp["first_frame_w2c"]).to(gpu)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            from fisher_rast.rendervar import FrameRenderVars
            outs = FrameRenderVars.apply(p["means3D"], p["unnorm_rotations"], p["logit_opacities"], p["log_scales"], p["cam_unnorm_rots"],
                                         p["cam_trans"], 1, w2c, gg, cg)
            torch.autograd.backward(outs, up)                     # raises on a device -> host read or a synchronising call
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        assert all(bool(torch.isfinite(v.grad).all()) for v in p.values() if v.grad is not None)
        assert (p["means3D"].grad is not None) == gg and (p["cam_trans"].grad is not None) == cg


# ---- 5. one full get_loss ---------------------------------------------------------------------------------------------------------------

def _quaternion_of(R):
    """(w, x, y, z) of a rotation matrix in the convention of rc.t_rotation, from the largest of the four components (a half turn has r = 0)"""
    d = np.array([1 + R[0, 0] + R[1, 1] + R[2, 2], 1 + R[0, 0] - R[1, 1] - R[2, 2], 1 - R[0, 0] + R[1, 1] - R[2, 2], 1 - R[0, 0] - R[1, 1] + R[2, 2]])
    k = int(np.argmax(d))
    s = 2 * np.sqrt(d[k])                                   # four times the component k
    q = [np.array([s / 4, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s]),
         np.array([(R[2, 1] - R[1, 2]) / s, s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s]),
         np.array([(R[0, 2] - R[2, 0]) / s, (R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s]),
         np.array([(R[1, 0] - R[0, 1]) / s, (R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4])][k]
    back = rc.t_rotation(torch.from_numpy(q)[None])[0].numpy()
    assert np.abs(back - R).max() < 1e-6, (R, back)
    return q


@pytest.mark.parametrize("mode", ["mapping", "tracking"])
def test_get_loss_with_the_flag_on_against_off(gpu, rv_harness, monkeypatch, mode):
    """make_get_loss through the drop-in rasteriser at 64 x 64 and P = 2000.  The losses of the two routes agree; the gradients that
    reached the fused route's render variables from the shared rasteriser, taken through the stages' binary64 evaluation, give every
    parameter gradient of the fused route within its allowance; means2D's gradient is there in both."""
    from fisher_rast import synthetic
    import models.SLAM.gaussian as G
    from models.SLAM.utils import slam_helpers as sh
    from models.SLAM.utils.recon_helpers import setup_camera
    P, W, H, t = 2000, 64, 64, 1
    tracking = mode == "tracking"
    base = {k: v.contiguous() for k, v in synthetic.room_shell(P, seed=12).items()}
    pose = synthetic.invert_rigid(synthetic.candidate_poses(1, seed=13))[0].double().numpy()
    rots = np.tile(np.array([1.0, 0, 0, 0])[None, :, None], (1, 1, 3))
    rots[0, :, t] = 1.7 * _quaternion_of(pose[:3, :3])                 # unnormalised, as the optimiser leaves it
    trans = np.zeros((1, 3, 3))
    trans[0, :, t] = pose[:3, 3]
    base["cam_unnorm_rots"], base["cam_trans"] = torch.from_numpy(rots).float(), torch.from_numpy(trans).float()
    cam = setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4), device=gpu)
    first = rc.random_rigid(np.random.default_rng(5))
    first[:3, :3] = 0.9 * np.eye(3) + 0.1 * first[:3, :3]                # depth along a direction near the camera's own axis
    g = torch.Generator().manual_seed(3)
    curr = dict(cam=cam, w2c=torch.from_numpy(first).float().to(gpu), im=torch.rand((3, H, W), generator=g).to(gpu),
                depth=(torch.rand((1, H, W), generator=g) * 4 + 0.5).to(gpu))

    def transform_to_frame(params, time_idx, gaussians_grad, camera_grad):          # the reference's, restated
        cq, ct = params['cam_unnorm_rots'][..., time_idx], params['cam_trans'][..., time_idx]
        if not camera_grad:
            cq, ct = cq.detach(), ct.detach()
        return rc.t_points(rc.t_pose(cq, ct), params['means3D'] if gaussians_grad else params['means3D'].detach())

    kept = {}
    plain = sh.frame_render_vars

    def keeping(*a, **k):
        rendervar, feats = plain(*a, **k)
        kept.update(pts=rendervar['means3D'], feats=feats, rotations=rendervar['rotations'], opacities=rendervar['opacities'], scales=rendervar['scales'])
        for v in kept.values():
            if v.requires_grad:
                v.retain_grad()
        return rendervar, feats

    monkeypatch.setattr(G, "frame_render_vars", keeping)
    weights = dict(im=0.5, depth=1.0)
    result = {}
    for flag in (True, False):
        params = {k: v.clone().to(gpu).requires_grad_(True) for k, v in base.items()}
        variables = dict(max_2D_radius=torch.zeros(P, device=gpu), means2D_gradient_accum=torch.zeros(P, device=gpu), denom=torch.zeros(P, device=gpu))
        loss, variables, _ = G.make_get_loss(transform_to_frame, sh.calc_loss, fused_rendervar=flag)(
            params, curr, variables, t, weights, True, 0.5, True, False, tracking=tracking, mapping=not tracking)
        loss.backward()
        torch.cuda.synchronize()
        assert variables['means2D'].grad is not None and variables['means2D'].grad.shape == (P, 3) and float(variables['means2D'].grad.abs().sum()) > 0
        assert int(variables['seen'].sum()) > 10
        result[flag] = (float(loss.detach()), {k: None if v.grad is None else v.grad.cpu().numpy() for k, v in params.items()})
    assert kept, "the fused route was not taken"
    (loss_on, grads_on), (loss_off, grads_off) = result[True], result[False]
    print(f"{mode}: loss with the flag on {loss_on!r}, off {loss_off!r}")
    assert abs(loss_on - loss_off) <= 2e-4 * abs(loss_off)
    wanted = ("cam_unnorm_rots", "cam_trans") if tracking else ("means3D",)
    for k in rc.PARAMS:
        has = k in wanted or k in ("unnorm_rotations", "logit_opacities", "log_scales")
        assert (grads_on[k] is not None) == has == (grads_off[k] is not None), k
        if has:
            scale = float(np.abs(grads_off[k]).max())
            tol = 2e-4 * np.abs(grads_off[k]) + 2e-6 * scale
            print(f"  d/d{k}: max |on - off| / max |off| {float(np.abs(grads_on[k] - grads_off[k]).max()) / scale:.2e}, "
                  f"largest |on - off| / tolerance {float((np.abs(grads_on[k] - grads_off[k]) / tol).max()):.3f}")
            # the two routes hand the rasteriser render variables that differ in their last bits: the project's tolerance for the
            # gradients of two such get_loss routes (tests/test_gpu_densify_stats.py, tests/test_gpu_image_loss.py)
            assert_close(grads_on[k], grads_off[k], 2e-4, f"get_loss d/d{k}, fused_rendervar on against off", atol_frac=2e-6)
    assert grads_on["rgb_colors"] is not None
    # the fused route's gradients from the gradients the rasteriser handed it, stage by stage
    inp = {k: base[k].numpy() for k in rc.PARAMS}
    inp["first_frame_w2c"] = first.astype(rc.F)
    for name in rc.OUTPUTS:
        assert kept[name].grad is not None, name
        inp["g_" + name] = kept[name].grad.cpu().numpy()
    host = rc.harness_run(rv_harness, inp, t, not tracking, tracking)
    vals = {name: kept[name].detach().cpu().numpy() for name in rc.OUTPUTS}
    vals.update({"g_" + k: v for k, v in grads_on.items() if v is not None and k in rc.PARAMS}, rel_w2c=host["rel_w2c"], G=host["G"])
    need = {s: rc.k_need(*tr) for s, tr in rc.stages(inp, t, vals).items() if s not in ("sums", "tail", "pose")}
    print(f"  K needed: " + ", ".join(f"{s} {k:.2f}" for s, k in sorted(need.items())))
    for s, k in need.items():
        assert k <= rc.allowed(s), (s, k, rc.allowed(s))
    if tracking:
        rc.K_TORCH_SUMS_AT[P]                                 # the sums' figure at this P is on record
        seven = np.concatenate([grads_on["cam_unnorm_rots"][0, :, t], grads_on["cam_trans"][0, :, t]]).astype(np.float64)
        w7, bound = rc.camera_bound(inp, t, host, P)
        assert (np.abs(seven - w7) <= bound).all(), (seven, w7, bound)
        assert not grads_on["cam_unnorm_rots"][0, :, [0, 2]].any()
