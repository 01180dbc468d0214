"""Stream-order harness: one entry point of the Python layer, driven so that ONLY stream order can give the right answer.

Every case has two input sets of identical shapes and dtypes, `real` and `decoy` (another seed of the same builder: valid data, every
index in range), and a `call(ctx, buffers) -> {name: tensor}`.  `run_case`:

  1. reference runs on the default stream, each followed by a device synchronise: want = call(real), want_decoy = call(decoy); the
     two must differ on every compared output (bit-exact outputs: not equal; toleranced outputs: by 100 x the tolerance of step 3);
  2. the work buffers hold `decoy`, settled.  On a torch.cuda.Stream s (`caller_stream`: one of the fresh streams that was seen to
     run beside the default stream, see there): a blocker (torch.cuda._sleep), an event `gate`, the
     work buffers overwritten in place with `real` (tensor.copy_: version counters move), the call, a clone of every output, and
     s.synchronize() -- never a device-wide synchronise between the call and the clones;
  3. the clones against `want`: bit for bit where the suite already compares bit for bit (forward images, keys, scores, knn, the
     harness-backed kernels), by the rule of the entry point's existing parity test where float atomics accumulate (quoted per case);
  4. validity: gate.query() is False immediately before the call (the blocker was still running, so the buffers still held `decoy`
     when the call was enqueued), and for the entry points the suite runs under set_sync_debug_mode("error") also immediately after.
     A failed guard FAILS the case ("blocker too short"); it never passes or skips.

A launch, memset or copy on another stream than the caller's reads `decoy` (or writes an output before the caller's stream fills
it); a side-stream launch in front of its wait does the same; a join that is missing lets the clones run ahead of the side stream.

`run_case(..., null_stream=patch)` is the committed mutation check: `patch` makes the layer's stream helper return the null stream,
the default stream is synchronised before the clones are enqueued, and the clones must then equal `want_decoy` exactly.

Blocker length.  torch.cuda._sleep cycles are calibrated to milliseconds once per session with two timing events
(`cycles_per_ms`).  Host-side enqueue times (first copy_ to the return of the call) measured on an MI355X box, the larger of two
runs, milliseconds:
    backward power 1 0.28, power 2 chunked 0.31, power 2 single pass 0.24, pair backward 0.31, mark_visible 0.08,
    scorer launch (H_inv, packed) 0.16, launch (out_H, 11 columns) 0.15, pose_launch 0.13, render_launch 0.12, point_launch 0.15,
    single-view front end 0.15, knn 0.10, spatial order 0.10, image loss forward + backward 0.10, fused adam 0.08,
    rendervar forward + backward 0.14, keyframe pixels + overlap 0.19, frame ingest select + emit 0.31, map edit apply + split 0.13,
    densify statistics + masks + prune 0.11, POp-GS criterion 0.09, occupancy update + free space + candidates 0.26
The slowest is 0.31 ms, ten times that 3.1 ms: the floor applies, BLOCKER_MS = 20 (the cap would be 250).  rasterize_forward, the
map edit's plan and setup_start / plan_paths read a status word or a result (the reference's own host synchronisations), so those
cases wait for the blocker inside the call (20.2 to 20.6 ms): their figure is the blocker's, not the host's, and is left out of
the maximum.  One torch.cuda._sleep cycle was 0.417 ns there (2.40e6 cycles per ms).
"""
import ctypes
import time
from typing import Callable, NamedTuple, Optional

import numpy as np

BLOCKER_MS = 20.0
BLOCKER_CAP_MS = 250.0

ENQUEUE_MS = {}                     # case name -> host milliseconds of the last stream-ordered run (reported by the tests)
_CYCLES_PER_MS = {}


class Case(NamedTuple):
    name: str
    make: Callable                  # make(which) -> {name: np.ndarray}; which = 0 real, 1 decoy
    call: Callable                  # call(ctx, buffers) -> {name: tensor}; "_status" (optional): status[1] must be 0
    exact: tuple = ()               # outputs compared bit for bit
    close: dict = {}                # output -> (rtol, atol_frac): |got - want| <= rtol |want| + atol_frac max|want| (gpu_util.assert_close)
    close_from: str = ""            # the existing parity test the numbers in `close` are taken from
    bounds: dict = {}               # index input -> (lo, hi): every element in [lo, hi)
    same: tuple = ()                # inputs kept equal between real and decoy (small host-like values, fixed parameters)
    setup: Optional[Callable] = None      # setup(buffers, dev) -> ctx, once per buffer set (a scorer over the buffers, ...)
    prepare: Optional[Callable] = None    # prepare(buffers, dev) -> {name: tensor or host value}: inputs the device derives (a forward's buffers)
    sync_free: bool = False         # the suite runs this entry point under set_sync_debug_mode("error")


# ---- the harness ----------------------------------------------------------------------------------------------------------------------

def cycles_per_ms(dev):
    """torch.cuda._sleep cycles per millisecond, measured once per session and device with two timing events"""
    import torch
    key = str(dev)
    if key not in _CYCLES_PER_MS:
        torch.cuda.synchronize(dev)
        best = None
        for cycles in (1_000_000, 20_000_000, 20_000_000):              # the first call warms the kernel up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cycles)
            e1.record()
            e1.synchronize()
            best = cycles / max(e0.elapsed_time(e1), 1e-3)
        _CYCLES_PER_MS[key] = best
    return _CYCLES_PER_MS[key]


_CALLER_STREAM = {}


def caller_stream(dev):
    """A torch.cuda.Stream that is known to run BESIDE the default stream, found once per session among fresh ones.  The runtime
    deals streams over a few hardware queues (four by default), and a queue runs its packets in order: on a stream that shares
    the null stream's queue, a kernel launched on the null stream by mistake queues up behind the blocker and the copies like a
    correct one, and the harness could not tell (seen on an MI355X box: the image-loss control came back with the real result).
    The probe: a 5 ms blocker on the candidate, one small kernel on the default stream, the default stream synchronised -- the
    candidate is taken if its blocker is still running then."""
    import torch
    key = str(dev)
    if key not in _CALLER_STREAM:
        probe = torch.zeros((64,), device=dev)
        cycles = int(5 * cycles_per_ms(dev))
        torch.cuda.synchronize(dev)
        for _ in range(16):
            s = torch.cuda.Stream(dev)
            with torch.cuda.stream(s):
                torch.cuda._sleep(cycles)
                gate = torch.cuda.Event()
                gate.record(s)
            with torch.cuda.stream(torch.cuda.default_stream(dev)):
                probe.add_(1.0)
            torch.cuda.default_stream(dev).synchronize()
            beside = not gate.query()
            s.synchronize()
            if beside:
                _CALLER_STREAM[key] = s
                break
        assert key in _CALLER_STREAM, "none of 16 fresh streams runs beside the default stream: a launch on the null stream could not be told from a correct one"
    return _CALLER_STREAM[key]


def upload(arrays, dev):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in arrays.items()}


def _tensors(d):
    import torch
    return {k: v for k, v in d.items() if isinstance(v, torch.Tensor)}


def _pristine(case, which, dev):
    import torch
    b = upload(case.make(which), dev)
    torch.cuda.synchronize(dev)
    if case.prepare is not None:
        b.update(case.prepare(b, dev))
        torch.cuda.synchronize(dev)
    return b


def _fill(work, src):
    for k, v in _tensors(src).items():
        work[k].copy_(v)


def _outputs(out):
    return {k: v for k, v in out.items() if v is not None and not k.startswith("_")}


def _same_bits(a, b):
    a, b = a.detach().cpu().contiguous().numpy(), b.detach().cpu().contiguous().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def mismatches(case, got, want):
    """the compared outputs of `got` that are not `want` (names with a figure): empty when the run gave the reference"""
    bad = []
    for k in case.exact:
        if not _same_bits(got[k], want[k]):
            bad.append(f"{k}: bits differ")
    for k, (rtol, atol_frac) in case.close.items():
        g, w = got[k].detach().cpu().double().numpy(), want[k].detach().cpu().double().numpy()
        tol = rtol * np.abs(w) + atol_frac * np.abs(w).max()
        over = np.abs(g - w) > tol
        if g.shape != w.shape or over.any() or not np.isfinite(g).all():
            bad.append(f"{k}: {int(over.sum())} of {w.size} outside {rtol:g} |want| + {atol_frac:g} max|want|, worst |err| "
                       f"{float(np.abs(g - w).max()):.3e} of max|want| {float(np.abs(w).max()):.3e}")
    return bad


def assert_distinct(case, want, want_decoy):
    """step 1: without this the case proves nothing"""
    for k in case.exact:
        assert not _same_bits(want[k], want_decoy[k]), f"{case.name}: real and decoy give the same {k}"
    for k, (rtol, atol_frac) in case.close.items():
        w, d = want[k].detach().cpu().double().numpy(), want_decoy[k].detach().cpu().double().numpy()
        tol = (rtol + atol_frac) * np.abs(w).max()                       # the largest deviation step 3 lets through
        gap = float(np.abs(w - d).max())
        assert tol > 0 and gap >= 100.0 * tol, f"{case.name}: real and decoy differ by {gap:.3e} on {k}, under 100 x the tolerance {tol:.3e}"


class Reference(NamedTuple):
    work: dict
    ctx: object
    real: dict
    decoy: dict
    want: dict
    want_decoy: dict


def reference(case, dev):
    """steps 1: both reference runs on the default stream; leaves the work buffers holding `decoy`, settled"""
    import torch
    real, decoy = _pristine(case, 0, dev), _pristine(case, 1, dev)
    for k, v in real.items():
        if isinstance(v, torch.Tensor):
            assert v.shape == decoy[k].shape and v.dtype == decoy[k].dtype, (case.name, k)
        else:
            assert v == decoy[k], f"{case.name}: host value {k} differs between real and decoy ({v} / {decoy[k]})"
    work = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in real.items()}
    ctx = case.setup(work, dev) if case.setup is not None else None
    runs = []
    for src in (real, decoy):
        _fill(work, src)
        out = case.call(ctx, work)
        torch.cuda.synchronize(dev)
        if out.get("_status") is not None:
            assert int(out["_status"].cpu()[1]) == 0, f"{case.name}: the key buffer overflowed in a reference run"
        runs.append({k: v.clone() for k, v in _outputs(out).items()})
    _fill(work, decoy)                                                    # (calls that write their inputs: decoy as it was)
    torch.cuda.synchronize(dev)
    names = set(case.exact) | set(case.close)
    assert names and names <= set(runs[0]), (case.name, names - set(runs[0]))
    assert_distinct(case, runs[0], runs[1])
    return Reference(work, ctx, real, decoy, runs[0], runs[1])


class Pending(NamedTuple):
    case: Case
    stream: object
    clones: dict
    status: object
    guards: tuple                   # (blocker_ms or 0, gate done before the call, gate done after it, is `after` binding, enqueue ms)


def enqueue(case, ref, dev, stream=None, blocker_ms=BLOCKER_MS, null_stream=False):
    """step 2 without its last line: blocker, gate, the buffers overwritten with `real`, the call and the clones, all enqueued on the
    stream; nothing is waited for.  blocker_ms = 0: no blocker and no guard (a caller that is not held back)."""
    import torch
    work = ref.work
    s = stream if stream is not None else caller_stream(dev)
    cycles = int(min(blocker_ms, BLOCKER_CAP_MS) * cycles_per_ms(dev))
    with torch.cuda.stream(s):
        gate = torch.cuda.Event()
        if cycles:
            torch.cuda._sleep(cycles)
        gate.record(s)
        t0 = time.perf_counter()
        _fill(work, ref.real)
        before = gate.query()
        out = case.call(ref.ctx, work)
        t1 = time.perf_counter()
        after = gate.query()
        if null_stream:
            torch.cuda.default_stream(dev).synchronize()                 # what ran on the null stream has run; the copies on s have not
            after = gate.query()
        clones = {k: v.clone() for k, v in _outputs(out).items()}
        status = out["_status"].clone() if (out.get("_status") is not None and not null_stream) else None
    return Pending(case, s, clones, status, (blocker_ms if cycles else 0, before, after, case.sync_free or null_stream, (t1 - t0) * 1e3))


def finish(p):
    """the last line of step 2, s.synchronize() -- the stream alone -- and the guards of step 4: returns the clones"""
    p.stream.synchronize()
    blocker_ms, before, after, binding, ms = p.guards
    ENQUEUE_MS[p.case.name] = ms
    if blocker_ms:
        assert not before, f"{p.case.name}: the blocker of {blocker_ms} ms was too short: it had ended before the call was enqueued"
        assert not (binding and after), (f"{p.case.name}: the blocker of {blocker_ms} ms was too short: it had ended when the call "
                                         f"returned (enqueue took {ms:.2f} ms)")
    if p.status is not None:
        assert int(p.status.cpu()[1]) == 0, f"{p.case.name}: the key buffer overflowed"
    return p.clones


def stream_run(case, ref, dev, stream=None, blocker_ms=BLOCKER_MS, null_stream=False):
    return finish(enqueue(case, ref, dev, stream, blocker_ms, null_stream))


def run_case(case, dev, blocker_ms=BLOCKER_MS):
    """the whole procedure for one case; raises AssertionError with the outputs that missed"""
    ref = reference(case, dev)
    got = stream_run(case, ref, dev, blocker_ms=blocker_ms)
    bad = mismatches(case, got, ref.want)
    assert not bad, f"{case.name}: the stream-ordered run does not give the default-stream result: {bad}"
    return ref, got


def null_stream_of(dev):
    import torch
    return ctypes.c_void_p(torch.cuda.default_stream(dev).cuda_stream)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------

F = np.float32
SORT_W, SORT_H = 32, 16              # the image of tests/test_gpu_sort_sizes.py: two tiles, every Gaussian of a scene in tile 0 or 1


def _camera(W, H, dev="cpu"):
    from fisher_rast.synthetic import intrinsics
    from models.SLAM.utils.recon_helpers import setup_camera
    return setup_camera(W, H, intrinsics(W, H), np.eye(4), device=dev)


def _camera_arrays(W, H):
    cam = _camera(W, H)
    return dict(bg=np.array([0.2, 0.5, 0.1], F), view=cam.viewmatrix.numpy().reshape(16).astype(F),
                proj=cam.projmatrix.numpy().reshape(16).astype(F), campos=cam.campos.numpy().astype(F))


CAMERA_NAMES = ("bg", "view", "proj", "campos")


def _sort_scene(n, which, features=False, dL=False):
    """the scene builder of tests/test_gpu_sort_sizes.py: n Gaussians in tile 0 (and n // 3 in tile 1), tied depths"""
    from test_gpu_sort_sizes import _scene
    W, H, sc = _scene(n, 1000 + n + 7919 * which)
    P = sc["means3D"].shape[0]
    rng = np.random.default_rng([n, which, 31])
    d = dict(means3D=sc["means3D"], colors=sc["colors"], opacity=sc["opacities"], scales=sc["scales"], rotations=sc["rotations"],
             **_camera_arrays(W, H))
    if features:
        d["features"] = rng.uniform(0, 1, (P, 3)).astype(F)
    if dL:
        d["dL"] = rng.normal(size=(3, H, W)).astype(F)
        if features:
            d["dLf"] = rng.normal(size=(3, H, W)).astype(F)
    return d


def _forward(b, features=False):
    import torch
    from fisher_rast import ops
    cam = _camera(SORT_W, SORT_H)
    empty = torch.Tensor([])
    return ops.rasterize_forward(b["bg"], b["means3D"], b["colors"], b["opacity"], b["scales"], b["rotations"], 1.0, empty, b["view"],
                                 b["proj"], cam.tanfovx, cam.tanfovy, SORT_H, SORT_W, empty, 0, b["campos"], False,
                                 features=b["features"] if features else None)


def _forward_case(n, features=False):
    def call(ctx, b):
        r = _forward(b, features)
        assert r[0] == n + n // 3, (r[0], n)
        out = dict(color=r[1], depth=r[6], keys=r[4][:8 * r[0]])
        if features:
            out["feature_image"] = r[7]
        return out
    # (n = 1500 faint Gaussians do not bring any pixel to the median's half transmittance: the depth image is the same for both sets)
    return Case(name=f"forward{'_pair' if features else ''}_n{n}", make=lambda which: _sort_scene(n, which, features), call=call,
                exact=("color", "keys") + (("depth",) if n >= 5000 else ()) + (("feature_image",) if features else ()),
                same=CAMERA_NAMES + ("opacity", "scales", "rotations"))


def _prepare_forward(features):
    def prepare(b, dev):
        r = _forward(b, features)
        return dict(radii=r[2], geom=r[3], binning=r[4], img=r[5], R=int(r[0]))
    return prepare


GRADS = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")


def _backward_case(n, power, segmented):
    def call(ctx, b):
        import torch
        from fisher_rast import ops
        cam = _camera(SORT_W, SORT_H)
        empty = torch.Tensor([])
        outs = ops.rasterize_backward(b["bg"], b["means3D"], b["radii"], b["colors"], b["scales"], b["rotations"], 1.0, empty, b["view"],
                                      b["proj"], cam.tanfovx, cam.tanfovy, b["dL"], empty, 0, b["campos"], b["geom"], b["R"], b["binning"],
                                      b["img"], power, segmented=segmented)
        return dict(zip(GRADS, outs))
    rule = (1e-4, 2e-5)
    return Case(name=f"backward_p{power}{'' if segmented else '_single_pass'}_n{n}", make=lambda which: _sort_scene(n, which, dL=True),
                call=call, prepare=_prepare_forward(False),
                close={k: rule for k in ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D")},
                close_from="test_gpu_rasterizer_parity.py::test_backward_parity (1e-4, atol_frac 2e-5)",
                same=CAMERA_NAMES + ("opacity", "scales", "rotations"))


PAIR_GRADS = ("dL_dmeans2D", "dL_dmeans2D_features", "dL_dcolors", "dL_dfeatures", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D",
              "dL_dscales", "dL_drotations")


def _backward_pair_case(n):
    def call(ctx, b):
        import torch
        from fisher_rast import ops
        cam = _camera(SORT_W, SORT_H)
        empty = torch.Tensor([])
        outs = ops.rasterize_backward_pair(b["bg"], b["means3D"], b["radii"], b["colors"], b["features"], b["scales"], b["rotations"], 1.0,
                                           empty, b["view"], b["proj"], cam.tanfovx, cam.tanfovy, b["dL"], b["dLf"], b["campos"],
                                           b["geom"], b["binning"], b["img"], num_rendered=b["R"])
        return dict(zip(PAIR_GRADS, outs))
    rule = (1e-4, 1e-6)
    return Case(name=f"backward_pair_n{n}", make=lambda which: _sort_scene(n, which, features=True, dL=True), call=call,
                prepare=_prepare_forward(True),
                close={k: rule for k in ("dL_dmeans2D", "dL_dmeans2D_features", "dL_dcolors", "dL_dfeatures", "dL_dopacity", "dL_dmeans3D")},
                close_from="test_gpu_rasterizer_parity.py::test_fused_rgb_depth_silhouette_pair (1e-4, atol_frac 1e-6)",
                same=CAMERA_NAMES + ("opacity", "scales", "rotations"))


def _mark_visible_case():
    def make(which):
        rng = np.random.default_rng([5, which])
        cam = _camera_arrays(SORT_W, SORT_H)
        means = np.stack([rng.uniform(-4, 4, 3001), rng.uniform(-3, 3, 3001), rng.uniform(-1, 5, 3001)], 1).astype(F)
        return dict(means3D=means, view=cam["view"], proj=cam["proj"])

    def call(ctx, b):
        from fisher_rast import ops
        import torch
        return dict(present=ops.mark_visible(b["means3D"], b["view"], b["proj"]).view(torch.uint8))
    return Case(name="mark_visible", make=make, call=call, exact=("present",), same=("view", "proj"))


# -- the scorer: the sort-sizes scene under 8 poses near the identity ----------------------------------------------------------------------

N_SCORER, V_SCORER = 5000, 8


def _near_identity(V, which, step=0.004):
    rng = np.random.default_rng([V, which, 77])
    w = np.tile(np.eye(4, dtype=F), (V, 1, 1))
    w[:, :3, 3] = rng.uniform(-step, step, (V, 3)).astype(F)
    return w


def _scorer_scene(which, columns, n=N_SCORER, V=V_SCORER):
    sc = _sort_scene(n, which)
    P = sc["means3D"].shape[0]
    rng = np.random.default_rng([n, which, columns])
    return dict(means3D=sc["means3D"], colors=sc["colors"], rotations=sc["rotations"], opacity=sc["opacity"], scales=sc["scales"],
                w2c=_near_identity(V, which), H_inv=(rng.uniform(0.05, 2.05, (P, columns))).astype(F))


def _scorer_setup(columns, W=SORT_W, H=SORT_H, **kw):
    def setup(b, dev):
        from fisher_rast.ops import FisherScorer
        return FisherScorer(_camera(W, H, dev), b["means3D"], b["colors"], b["rotations"], b["opacity"], b["scales"], columns=columns, **kw)
    return setup


SCORER_SAME = ("rotations", "opacity", "scales")


def _scorer_cases():
    import functools

    def launch_hinv(sc, b):
        r = sc.launch(b["w2c"], H_inv=b["H_inv"])
        return dict(scores=r["scores"], _status=r["status"])

    def launch_outh(sc, b):
        import torch
        out = torch.zeros((sc.P, sc.columns), device=sc.dev)
        r = sc.launch(b["w2c"], out_H=out)
        return dict(out_H=out, _status=r["status"])

    def pose(sc, b):
        r = sc.pose_launch(b["w2c"])
        return dict(pose_H=r["pose_H"], _status=r["status"])

    def render(sc, b):
        r = sc.render_launch(b["w2c"])
        return dict(render=r["render"], depth_sil=r["depth_sil"], median_depth=r["median_depth"], final_T=r["final_T"], _status=r["status"])

    def point(sc, b):
        r = sc.point_launch(b["w2c"], b["H_inv"])
        return dict(scores=r["scores"], point_scores=r["point_scores"], _status=r["status"])

    mk = lambda c: functools.partial(_scorer_scene, columns=c)
    return [
        # packed lists with V >= 8: the multi-view configuration that forks the 1024-thread sort tier onto side stream [0] (want_fork)
        Case(name="scorer_launch_hinv_packed", make=mk(4), call=launch_hinv, setup=_scorer_setup(4, tile_capacity=0), exact=("scores",),
             same=SCORER_SAME, sync_free=True),
        Case(name="scorer_launch_outH_11", make=mk(11), call=launch_outh, setup=_scorer_setup(11), close={"out_H": (1e-4, 1e-7)},
             close_from="test_gpu_fisher_parity.py::test_per_view_hessian_and_scores (1e-4, atol_frac 1e-7)", same=SCORER_SAME, sync_free=True),
        Case(name="scorer_pose_launch", make=mk(4), call=pose, setup=_scorer_setup(4), exact=("pose_H",), same=SCORER_SAME, sync_free=True),
        Case(name="scorer_render_launch", make=mk(4), call=render, setup=_scorer_setup(4),
             exact=("render", "depth_sil", "median_depth", "final_T"), same=SCORER_SAME, sync_free=True),
        Case(name="scorer_point_launch", make=mk(4), call=point, setup=_scorer_setup(4), exact=("scores",),
             close={"point_scores": (1e-4, 1e-7)},
             close_from="test_gpu_point_scores.py::test_point_scores_against_the_oracle (the flat part of its rule: 1e-4 |want| + 1e-7 max|want|)",
             same=SCORER_SAME, sync_free=True),
    ]


SV_P, SV_W, SV_H, SV_V = 3000, 1040, 1040, 2


def _single_view_front_end_case():
    """65 x 65 tiles: beyond 4096 tiles fr_fisher_views takes the single-view front end, whose k_fisher_records runs on side stream [1]
    beside the sorts (fr_bin_pipeline, `plan && !multi`): tests/test_gpu_outh_variants.py reaches it the same way"""
    def make(which):
        from fisher_rast import synthetic
        act = synthetic.activate(synthetic.room_shell(SV_P, seed=8 + which))
        rng = np.random.default_rng([which, 65])
        w2c = np.ascontiguousarray(synthetic.invert_rigid(synthetic.candidate_poses(SV_V, seed=8 + which)).numpy(), F)
        return dict(means3D=act["means3D"].numpy(), colors=act["rgb_colors"].numpy(), rotations=act["rotations"].numpy(),
                    opacity=act["opacities"].numpy(), scales=act["scales"].numpy(), w2c=w2c,
                    H_inv=rng.uniform(0.05, 2.05, (SV_P, 4)).astype(F))

    def call(sc, b):
        assert sc.tiles == 65 * 65
        r = sc.launch(b["w2c"], H_inv=b["H_inv"])
        return dict(scores=r["scores"], _status=r["status"])
    return Case(name="scorer_single_view_front_end", make=make, call=call, setup=_scorer_setup(4, SV_W, SV_H), exact=("scores",),
                sync_free=True)


# -- knn and the spatial order: one key past an LDS chunk of the bitonic network -----------------------------------------------------------

P_KNN = 2049


def _points(which):
    rng = np.random.default_rng([P_KNN, which])
    return dict(points=rng.uniform(-2, 2, (P_KNN, 3)).astype(F))


def _knn_case():
    def call(ctx, b):
        from simple_knn._C import distCUDA2
        return dict(dist2=distCUDA2(b["points"]))
    return Case(name="knn_dist2", make=_points, call=call, exact=("dist2",))


def _spatial_order_case():
    def call(ctx, b):
        from fisher_rast import ops
        return dict(order=ops.spatial_order_of(b["points"]))
    return Case(name="spatial_order", make=_points, call=call, exact=("order",))


# -- one case each from the tables of the other families -------------------------------------------------------------------------------------

LOSS_SHAPE = (3, 17, 33)


def _image_loss_case():
    def make(which):
        import loss_cases as lc
        x, y, m1, _ = lc.make_case(LOSS_SHAPE, ("noise", "smooth")[which], "half")
        rng = np.random.default_rng([which, 3])
        return dict(img=x, gt=y, mask=m1.astype(np.uint8), upstream=rng.uniform(0.5, 1.5, 1).astype(F))

    def call(ctx, b):
        from fisher_rast import image_loss as il
        out4, chan, smap, saved, cfg, m = il.forward_raw(b["img"], b["gt"], b["mask"], 0.8, 0.2, il.FR_LOSS_L1_MASKED_MEAN, want_map=True,
                                                         want_channels=True)
        grad = il.backward_raw(b["img"], b["gt"], m, saved, cfg, b["upstream"])
        return dict(out4=out4, channel_ssim=chan, ssim_map=smap, grad=grad)
    return Case(name="image_loss", make=make, call=call, exact=("out4", "channel_ssim", "ssim_map", "grad"), sync_free=True)


ADAM_SIZES = (4099, 3, 1024)


def _adam_case():
    def make(which):
        rng = np.random.default_rng([which, 11])
        d = {}
        for i, n in enumerate(ADAM_SIZES):
            d[f"p{i}"], d[f"g{i}"] = rng.normal(size=n).astype(F), rng.normal(size=n).astype(F)
            d[f"m{i}"], d[f"v{i}"] = (0.1 * rng.normal(size=n)).astype(F), (0.01 * rng.uniform(size=n)).astype(F)
        return d

    def call(ctx, b):
        import adam_cases as ac
        from fisher_rast.optim import HipAdamBackend
        entries = [(b[f"p{i}"], b[f"g{i}"], b[f"m{i}"], b[f"v{i}"], ac.coeffs(0.01 * (i + 1), (0.9, 0.999), 1e-8, 3), False)
                   for i in range(len(ADAM_SIZES))]
        HipAdamBackend.step(entries)
        return {k: b[k] for k in b if k[0] in "pmv"}
    names = tuple(f"{c}{i}" for i in range(len(ADAM_SIZES)) for c in "pmv")
    return Case(name="fused_adam", make=make, call=call, exact=names, sync_free=True)


RV_P = 257


def _rendervar_case():
    import rendervar_cases as rc

    def make(which):
        return rc.make_inputs(RV_P, 3, seed=20 + which)

    def call(ctx, b):
        import torch
        from fisher_rast import ops
        dev = b["means3D"].device
        inputs = {k: b[k] for k in rc.PARAMS + ("first_frame_w2c",)}
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        out = dict(pts=new(RV_P, 3), feats=new(RV_P, 3), rotations=new(RV_P, 4), opacities=new(RV_P, 1), scales=new(RV_P, 3))
        ops.rendervar_forward(RV_P, 3, 2, rc.T_FRAMES, {**inputs, **out})
        grads = dict(g_means3D=new(RV_P, 3), g_unnorm_rotations=new(RV_P, 4), g_logit_opacities=new(RV_P, 1), g_log_scales=new(RV_P, 3),
                     g_cam_unnorm_rots=new(1, 4, rc.T_FRAMES), g_cam_trans=new(1, 3, rc.T_FRAMES))
        ops.rendervar_backward(RV_P, 3, 2, rc.T_FRAMES, {**inputs, **{k: b[k] for k in rc.UPSTREAM}, **grads})
        return {**out, **grads}
    return Case(name="rendervar", make=make, call=call, exact=rc.OUTPUTS + rc.GRADS, sync_free=True)


KF_N_VALID = 2048                    # the prefix of the valid-pixel list the draws index: below both cases' counts


def _keyframe_case():
    import keyframe_cases as kc

    def make(which):
        c = kc.make_case("masks-present", seed=which, n=16)
        assert c["valid_idx"].size >= KF_N_VALID
        rng = np.random.default_rng([which, 41])
        d = dict(depth=c["depth"], K=c["K"], w2c=c["w2c"], kf_w2c=c["kf_w2c"], draws=rng.integers(0, KF_N_VALID, 48).astype(np.int64))
        for k, m in enumerate(c["kf_masks"]):
            d[f"kf_mask{k}"] = m.astype(np.uint8)
        return d

    def call(ctx, b):
        from fisher_rast import ops
        idx, status = ops.keyframe_valid_pixels(b["depth"])
        masks = [b[f"kf_mask{k}"] for k in range(b["kf_w2c"].shape[0])]
        # (n_valid_idx is the count as the host read it: a fixed prefix here, so that nothing is read back between the two calls)
        r = ops.keyframe_overlap(b["depth"], b["K"], b["w2c"], b["draws"], b["kf_w2c"], valid_idx=idx, n_valid_idx=KF_N_VALID,
                                 kf_masks=masks, edge=4, want_pts=True)
        return dict(idx_head=idx[:KF_N_VALID], n_valid=status[:1], counts=r["counts"], valid=r["valid"], pts=r["pts"])
    return Case(name="keyframe", make=make, call=call, exact=("idx_head", "n_valid", "counts", "pts"), bounds={"draws": (0, KF_N_VALID)},
                same=("K", "w2c"), sync_free=True)


INGEST_SHAPE = (48, 64, 4)           # H, W, downsample
INGEST_ROWS = 40                     # rows emitted: below the number of cells either input set selects (checked where the inputs are made)


def _ingest_inputs(which):
    """the "half" case of tests/ingest_cases.py; the decoy is the same frame mirrored left to right under the table's other camera,
    with the silhouette also open over its left quarter (another count, another median)"""
    import ingest_cases as ic
    c = ic.make_case("half", INGEST_SHAPE, which_camera=which)
    if which:
        for k in ("depth_sil", "gt", "color"):
            c[k] = np.ascontiguousarray(c[k][..., ::-1])
        c["depth_sil"][1, :, :INGEST_SHAPE[1] // 4] = 0.0
    assert ic.np_select(c)["count"] >= INGEST_ROWS
    return c


def _ingest_case():
    def make(which):
        c = _ingest_inputs(which)
        return dict(depth_sil=c["depth_sil"], gt=c["gt"], color=c["color"], K=c["K"], w2c=c["w2c"])

    def call(ctx, b):
        import torch
        import ingest_cases as ic
        from fisher_rast import ops
        ratio = _ingest_inputs(0)["ratio"]
        status, ws = ops.frame_ingest_select(b["depth_sil"], b["gt"], downsample=INGEST_SHAPE[2], sil_thres=ic.SIL_THRES, depth_error_ratio=ratio)
        new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=b["gt"].device)
        out = dict(means3D=new(INGEST_ROWS, 3), rgb_colors=new(INGEST_ROWS, 3), unnorm_rotations=new(INGEST_ROWS, 4),
                   logit_opacities=new(INGEST_ROWS, 1), log_scales=new(INGEST_ROWS, 3), mean3_sq_dist=new(INGEST_ROWS))
        # (the count is the host's read of status[0] in the product; a fixed prefix here, so that nothing is read back in between)
        ops.frame_ingest_emit(b["color"], b["gt"], b["K"], b["w2c"], ws, INGEST_ROWS, downsample=INGEST_SHAPE[2], **out)
        return dict(status=status, means3D=out["means3D"], rgb_colors=out["rgb_colors"], log_scales=out["log_scales"],
                    mean3_sq_dist=out["mean3_sq_dist"])
    return Case(name="frame_ingest", make=make, call=call, exact=("status", "means3D", "rgb_colors", "log_scales", "mean3_sq_dist"),
                same=("K",), sync_free=True)


# -- map edit: plan (one host read inside), apply and split children -----------------------------------------------------------------------

EDIT_P, EDIT_SPLIT, EDIT_CLONE, EDIT_INTO = 300, 40, 60, 2


def _edit_inputs(which):
    """every row is plain, cloned or split; both input sets have the same number of each (the plan's counts are host values), at other rows"""
    rng = np.random.default_rng([which, 67])
    role = rng.permutation(np.repeat([0, 1, 2], [EDIT_P - EDIT_SPLIT - EDIT_CLONE, EDIT_CLONE, EDIT_SPLIT]))
    return dict(keep=(role != 2).astype(np.uint8), clone=(role == 1).astype(np.uint8), split=(role == 2).astype(np.uint8),
                means3D=rng.normal(size=(EDIT_P, 3)).astype(F), unnorm_rotations=rng.normal(size=(EDIT_P, 4)).astype(F),
                log_scales=(rng.normal(size=(EDIT_P, 3)) - 3).astype(F), exp_avg=rng.normal(size=(EDIT_P, 3)).astype(F),
                z=rng.normal(size=(EDIT_INTO * EDIT_SPLIT, 3)).astype(F))


def _edit_plan(b, dev):
    from models.SLAM.utils.slam_external import HipMapEditBackend
    plan, _ = HipMapEditBackend().plan(EDIT_P, b["keep"], b["clone"], b["split"], EDIT_INTO, dev)
    assert (plan.n_keep, plan.n_clone, plan.n_split) == (EDIT_P - EDIT_SPLIT, EDIT_CLONE, EDIT_SPLIT)
    return plan


def _edit_apply(plan, b):
    from fisher_rast import _lib
    from models.SLAM.utils.slam_external import HipMapEditBackend
    be = HipMapEditBackend()
    means, rots, logs, m = be.apply(plan, [(b["means3D"], _lib.FR_EDIT_COPY), (b["unnorm_rotations"], _lib.FR_EDIT_COPY),
                                           (b["log_scales"], _lib.FR_EDIT_COPY), (b["exp_avg"], _lib.FR_EDIT_ZERO)])
    be.split_children(plan, b["z"], means, rots, logs)
    return dict(means3D=means, unnorm_rotations=rots, log_scales=logs, exp_avg=m)


EDIT_OUT = ("means3D", "unnorm_rotations", "log_scales", "exp_avg")


def _map_edit_cases():
    def whole(ctx, b):
        return _edit_apply(_edit_plan(b, b["means3D"].device), b)      # the plan's host read waits for the stream in the middle of the call

    def prepare(b, dev):
        return dict(handle=_edit_plan(b, dev).handle)

    def apply_only(ctx, b):
        from models.SLAM.utils.slam_external import MapEditPlan
        return _edit_apply(MapEditPlan(EDIT_P, EDIT_P - EDIT_SPLIT, EDIT_CLONE, EDIT_SPLIT, EDIT_INTO, b["handle"]), b)
    return [Case(name="map_edit_plan_apply_split", make=_edit_inputs, call=whole, exact=EDIT_OUT),
            # the plan made beforehand, its index lists an input like any other: apply and split children behind the blocker
            Case(name="map_edit_apply_split", make=_edit_inputs, call=apply_only, prepare=prepare, exact=EDIT_OUT)]


# -- densify statistics, densify masks, prune mask -------------------------------------------------------------------------------------------

DENSIFY_P = 1027


def _densify_case():
    def make(which):
        rng = np.random.default_rng([which, 71])
        P = DENSIFY_P
        return dict(radii=(rng.integers(0, 40, P) * (rng.uniform(size=P) < 0.7)).astype(np.int32), grad=rng.normal(size=(P, 3)).astype(F),
                    max_2D_radius=rng.uniform(0, 30, P).astype(F), means2D_gradient_accum=rng.uniform(0, 2, P).astype(F),
                    denom=rng.integers(1, 6, P).astype(F), logit_opacities=(3 * rng.normal(size=(P, 1))).astype(F),
                    log_scales=(rng.normal(size=(P, 3)) - 3).astype(F))

    def call(ctx, b):
        import types
        import torch
        from models.SLAM.utils import slam_external as se
        variables = dict(means2D=types.SimpleNamespace(grad=b["grad"]), means2D_gradient_accum=b["means2D_gradient_accum"], denom=b["denom"],
                         max_2D_radius=b["max_2D_radius"])
        se.accumulate_mean2d_gradient(variables, radius=b["radii"])
        to_clone, to_split = se.densify_masks(b, variables, 0.2)
        to_remove = se.prune_mask(b, 0.005, 0.1)
        u8 = lambda t: t.view(torch.uint8)
        return dict(means2D_gradient_accum=b["means2D_gradient_accum"], denom=b["denom"], max_2D_radius=b["max_2D_radius"],
                    seen=u8(variables["seen"]), to_clone=u8(to_clone), to_split=u8(to_split), to_remove=u8(to_remove))
    return Case(name="densify_stats_masks_prune", make=make, call=call, bounds={"radii": (0, 40)},
                exact=("means2D_gradient_accum", "denom", "max_2D_radius", "seen", "to_clone", "to_split", "to_remove"))


# -- occupancy and planning through planning/astar.py ---------------------------------------------------------------------------------------

OCC_DEPTH_HW = (24, 32)


def _planner(c, dev):
    """tests/test_gpu_path_plan.py's planner over a case of tests/plan_cases.py; the map centre is held on the host, so that no method
    reads it back from the device in front of its launches"""
    import torch
    from planning.astar import AstarPlanner
    p = AstarPlanner(device=dev)
    p.grid_dim = np.array([c["W"], c["H"]])
    p._map_center_np = np.asarray(c["center"], np.float64)
    p.map_center = torch.from_numpy(p._map_center_np)
    p.cell_size, p.cam_height = c["cell"], c["cam_height"]
    p.intrinsics = np.array([[28.0, 0, 16.0], [0, 28.0, 12.0], [0, 0, 1]], F)
    return p


def _plan_map(which):
    import plan_cases as pc
    return pc.make_case(("door-3", "door-9")[which])


def _occupancy_case():
    def make(which):
        rng = np.random.default_rng([which, 73])
        return dict(occ_map=_plan_map(which)["occ_map"], depth=rng.uniform(0.3, 1.5, (1,) + OCC_DEPTH_HW).astype(F),
                    centre=rng.uniform(-0.3, 0.3, (1, 2)).astype(F))

    def setup(b, dev):
        p = _planner(_plan_map(0), dev)
        p.occ_map = b["occ_map"]
        return p

    def call(p, b):
        import torch
        p.update_occ_map(b["depth"], np.eye(4, dtype=F), 1)
        free = p.build_connected_freespace(as_tensor=True)
        eroded = p._eroded_free(None, 3)
        c2w, keep = p._ring_candidates(b["centre"], 16, p.min_range, p.radius, eroded, 40, seed=5)
        return dict(occ_map=b["occ_map"], free=free, eroded=eroded, c2w=c2w, keep=keep.view(torch.uint8))
    return Case(name="occupancy_update_freespace_candidates", make=make, call=call, setup=setup, exact=("occ_map", "free", "eroded", "c2w"))


def _path_plan_case():
    def make(which):
        return dict(occ_map=_plan_map(which)["occ_map"])

    def setup(b, dev):
        p = _planner(_plan_map(0), dev)
        p.occ_map = b["occ_map"]
        return p

    def call(p, b):
        import torch
        c = _plan_map(0)                                                  # (start and goals are the same in both maps)
        p.setup_start(np.array(c["start"]))
        paths = p.plan_paths(c["goals"])
        flat = np.concatenate([np.asarray(q, np.int64).reshape(-1) for q in paths] + [np.array([len(q) for q in paths], np.int64)])
        plan = p._plan
        return dict(occ_plan=plan["occ_plan"], free=plan["free"], tiers=plan["tiers"], field=plan["field"], paths=torch.from_numpy(flat))
    return Case(name="path_plan_grid_field_paths", make=make, call=call, setup=setup, exact=("occ_plan", "free", "field", "paths"))


POPGS_V, POPGS_K, POPGS_E = 5, 3, 1027


def _popgs_case():
    def make(which):
        rng = np.random.default_rng([which, 53])
        return dict(rows=rng.normal(size=(POPGS_V, POPGS_K, POPGS_E)).astype(F), prior=rng.uniform(0.5, 2.0, (POPGS_V, POPGS_E)).astype(F),
                    vis=rng.integers(1, 100, POPGS_V).astype(np.int32), accumulate=np.array([1, 0, 1, 1, 0], np.uint8))

    def call(ctx, b):
        import torch
        from fisher_rast import ops
        out = torch.zeros((POPGS_V, POPGS_E), dtype=torch.float32, device=b["rows"].device)
        s = ops.popgs_diag_criterion(b["rows"], b["prior"], 1e-6, "dopt", prior_out=out, accumulate=b["accumulate"], vis_count=b["vis"])
        return dict(scores=s, prior_out=out)
    return Case(name="popgs_criterion", make=make, call=call, exact=("scores", "prior_out"), bounds={"vis": (1, 100)}, same=("accumulate",))


_TABLE = None


def cases():
    global _TABLE
    if _TABLE is None:
        n = N_SCORER
        _TABLE = [
            _forward_case(n), _forward_case(1500), _forward_case(n, features=True),
            _backward_case(n, 1, True), _backward_case(n, 2, True), _backward_case(n, 2, False), _backward_pair_case(n),
            _mark_visible_case(), *_scorer_cases(), _single_view_front_end_case(), _knn_case(), _spatial_order_case(),
            _image_loss_case(), _adam_case(), _rendervar_case(), _keyframe_case(), _ingest_case(), *_map_edit_cases(), _densify_case(), _popgs_case(),
            _occupancy_case(), _path_plan_case(),
        ]
    return _TABLE


def by_name(name):
    return next(c for c in cases() if c.name == name)


def names():
    return [c.name for c in cases()]
