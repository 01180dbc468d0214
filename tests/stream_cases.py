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

Coverage.  Every case lists in `covers` the C entry points its call drives.  tests/test_stream_cases_cpu.py holds the union of the
lists against the exports that take a stream (every export of fisher_rast._lib.EXPORTS whose declaration has an fr_stream_t), so an
entry point added without a case fails there; test_stream_order wraps those exports of the loaded library in a recorder for the
stream-ordered run and holds each list against what was called, so a list cannot claim more, or less, than the call does.

Memsets.  A hipMemsetAsync that clears an accumulator, a histogram or a status word on another stream than the caller's runs EARLY,
while the blocker holds the kernels back: on a workspace that nothing has touched since the reference runs it clears what it should,
only too soon, and the result is right.  A case with `repeat` therefore makes the call twice behind the blocker and compares the
second: the second call's early memset then runs before the first call's kernels have dirtied the workspace (the one kept per index
or per stream, or the block that the caching allocator hands out again), and the second call's kernels find it dirty.
What is shown and what is not: tests/test_gpu_streams.py holds the mechanism against a torch stand-in with a workspace of its own whose
clear goes to the null stream -- nothing patches a real unit's memset, so no test proves that a unit's second call meets a dirty
workspace.  For DBSCAN, the loss mask and the cloud search (fresh torch.empty blocks per call, a fresh index per call) that rests on
the caching allocator handing the freed block of the first call to the second, which is its usual behaviour and a supposition
here; the view metrics, the background penalty, the roll-out and the grid candidates issue no memset at all, `repeat` there only
makes a second call re-use what the first left.  `repeat` narrows the gap for the units that clear with memsets; it does not close it.

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
and of the cases added with the `covers` column (a `repeat` case: both calls):
    forward_features 0.30, fr_backward through the C ABI 0.20, fr_backward_pair 0.24,
    cloud build + search 0.17 (twice), cloud build + query_depth 0.21 (twice), dbscan_raw 0.13 (twice),
    view metrics + summary float 0.13 (twice), uint8 0.10 (twice), loss mask one launch 0.09 (twice), five launches 0.11 (twice),
    background penalty forward + backward through autograd 0.52 (twice), roll-out 0.07 (twice), grid candidates from device centres 0.09 (twice)
The slowest is 0.52 ms, ten times that 5.2 ms: the floor applies, BLOCKER_MS = 20 (the cap would be 250).  rasterize_forward, the
map edit's plan and setup_start / plan_paths read a status word or a result (the reference's own host synchronisations), so those
cases wait for the blocker inside the call (20.2 to 20.6 ms): their figure is the blocker's, not the host's, and is left out of
the maximum.  The same holds for build_frontiers + sample_random_candidate (20.5), select_target (20.4), get_gaussians_outside_mask
(20.3), setup_start + plan_actions (21.3), + plan_actions_object (21.4) and build_object_frontiers + grid candidates (20.5).
One torch.cuda._sleep cycle was 0.417 ns there (2.40e6 cycles per ms).
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
    sync_free: bool = False         # nothing is read back inside the call (the suite runs the entry point under set_sync_debug_mode("error"), or
                                    # its layer documents no host read): the call must return while the blocker is still running
    covers: tuple = ()              # the C entry points (names of fisher_rast._lib.EXPORTS) that `call` drives: all of them, and no other
    images: tuple = ()              # uint8 inputs that hold image bytes (0 .. 255), not a mask or a flag
    repeat: bool = False            # the stream-ordered run makes the call twice back to back and compares the second (a call that reads nothing
                                    # back and writes none of its inputs): see "Memsets" in the module's docstring


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
        if case.repeat:
            case.call(ref.ctx, work)                                     # dropped: its workspaces and outputs go back to the allocator, dirty
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


def declared_exports(with_return=False):
    """{name: parameter list} of every function that include/fisher_rast.h and include/fisher_occ.h declare, comments taken out;
    with_return: {name: (return type, parameter list)}"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    found = {}
    for header in ("fisher_rast.h", "fisher_occ.h"):
        with open(os.path.join(root, "include", header)) as f:
            text = f.read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        for m in re.finditer(r"([A-Za-z_][\w \t*]*?)\s*\b(fr_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", text):
            found[m.group(2)] = (" ".join(m.group(1).split()), m.group(3)) if with_return else m.group(3)
    return found


def stream_exports():
    """the exports that take a stream: those whose declaration has an fr_stream_t parameter (tests/test_stream_cases_cpu.py holds the
    declarations against fisher_rast._lib.EXPORTS and the others against a list written out by name)"""
    return tuple(n for n, params in declared_exports().items() if "fr_stream_t" in params)


class recorded_calls:
    """`with recorded_calls() as called:` -- every stream-taking export of the loaded library is wrapped for the length of the block
    (an attribute set on the CDLL object shadows the function the Python layers look up at every call); `called` is the set of the
    names that were called.  The wrappers come off on exit."""

    def __enter__(self):
        from fisher_rast import _lib
        self.lib, self.called, self.saved = _lib.load(), set(), {}
        for name in stream_exports():
            fn = getattr(self.lib, name)
            self.saved[name] = fn

            def wrapper(*args, _fn=fn, _name=name):
                self.called.add(_name)
                return _fn(*args)
            setattr(self.lib, name, wrapper)
        return self.called

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.lib, name, fn)
        return False


def run_case(case, dev, blocker_ms=BLOCKER_MS, check_covers=False):
    """the whole procedure for one case; raises AssertionError with the outputs that missed.  check_covers: the stream-ordered run
    called every entry point of `case.covers` and no other stream-taking export."""
    ref = reference(case, dev)
    with recorded_calls() as called:
        got = stream_run(case, ref, dev, blocker_ms=blocker_ms)
    bad = mismatches(case, got, ref.want)
    assert not bad, f"{case.name}: the stream-ordered run does not give the default-stream result: {bad}"
    if check_covers:
        assert called == set(case.covers), (f"{case.name}: covers lists {sorted(set(case.covers) - called)} that the call did not drive, "
                                            f"and leaves out {sorted(called - set(case.covers))} that it did")
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
                same=CAMERA_NAMES + ("opacity", "scales", "rotations"), covers=("fr_forward_pair" if features else "fr_forward",))


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
                same=CAMERA_NAMES + ("opacity", "scales", "rotations"), covers=("fr_backward_ws",))


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
                same=CAMERA_NAMES + ("opacity", "scales", "rotations"), covers=("fr_backward_pair_ws",))


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
    return Case(name="mark_visible", make=make, call=call, exact=("present",), same=("view", "proj"), covers=("fr_mark_visible",))


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
             same=SCORER_SAME, sync_free=True, covers=("fr_fisher_views",)),
        Case(name="scorer_launch_outH_11", make=mk(11), call=launch_outh, setup=_scorer_setup(11), close={"out_H": (1e-4, 1e-7)},
             close_from="test_gpu_fisher_parity.py::test_per_view_hessian_and_scores (1e-4, atol_frac 1e-7)", same=SCORER_SAME, sync_free=True,
             covers=("fr_fisher_views",)),
        Case(name="scorer_pose_launch", make=mk(4), call=pose, setup=_scorer_setup(4), exact=("pose_H",), same=SCORER_SAME, sync_free=True,
             covers=("fr_fisher_pose_views",)),
        Case(name="scorer_render_launch", make=mk(4), call=render, setup=_scorer_setup(4),
             exact=("render", "depth_sil", "median_depth", "final_T"), same=SCORER_SAME, sync_free=True, covers=("fr_render_views",)),
        Case(name="scorer_point_launch", make=mk(4), call=point, setup=_scorer_setup(4), exact=("scores",),
             close={"point_scores": (1e-4, 1e-7)},
             close_from="test_gpu_point_scores.py::test_point_scores_against_the_oracle (the flat part of its rule: 1e-4 |want| + 1e-7 max|want|)",
             same=SCORER_SAME, sync_free=True, covers=("fr_fisher_point_views",)),
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
                sync_free=True, covers=("fr_fisher_views",))


# -- knn and the spatial order: one key past an LDS chunk of the bitonic network -----------------------------------------------------------

P_KNN = 2049


def _points(which):
    rng = np.random.default_rng([P_KNN, which])
    return dict(points=rng.uniform(-2, 2, (P_KNN, 3)).astype(F))


def _knn_case():
    def call(ctx, b):
        from simple_knn._C import distCUDA2
        return dict(dist2=distCUDA2(b["points"]))
    return Case(name="knn_dist2", make=_points, call=call, exact=("dist2",), covers=("fr_knn_dist2",))


def _spatial_order_case():
    def call(ctx, b):
        from fisher_rast import ops
        return dict(order=ops.spatial_order_of(b["points"]))
    return Case(name="spatial_order", make=_points, call=call, exact=("order",), covers=("fr_spatial_order",))


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
    return Case(name="image_loss", make=make, call=call, exact=("out4", "channel_ssim", "ssim_map", "grad"), sync_free=True,
                covers=("fr_image_loss_forward", "fr_image_loss_backward"))


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
    return Case(name="fused_adam", make=make, call=call, exact=names, sync_free=True, covers=("fr_adam_step",))


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
    return Case(name="rendervar", make=make, call=call, exact=rc.OUTPUTS + rc.GRADS, sync_free=True,
                covers=("fr_rendervar_forward", "fr_rendervar_backward"))


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
                same=("K", "w2c"), sync_free=True, covers=("fr_keyframe_valid_pixels", "fr_keyframe_overlap"))


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
                same=("K",), sync_free=True, covers=("fr_frame_ingest_select", "fr_frame_ingest_emit"))


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
    return [Case(name="map_edit_plan_apply_split", make=_edit_inputs, call=whole, exact=EDIT_OUT,
                 covers=("fr_map_edit_plan", "fr_map_edit_apply", "fr_map_edit_split_children")),
            # the plan made beforehand, its index lists an input like any other: apply and split children behind the blocker
            Case(name="map_edit_apply_split", make=_edit_inputs, call=apply_only, prepare=prepare, exact=EDIT_OUT,
                 covers=("fr_map_edit_apply", "fr_map_edit_split_children"))]


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
                exact=("means2D_gradient_accum", "denom", "max_2D_radius", "seen", "to_clone", "to_split", "to_remove"),
                covers=("fr_densify_stats", "fr_densify_masks", "fr_prune_mask"))


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
    return Case(name="occupancy_update_freespace_candidates", make=make, call=call, setup=setup, exact=("occ_map", "free", "eroded", "c2w"),
                covers=("fr_occ_update", "fr_occ_freespace", "fr_occ_erode", "fr_occ_ring_candidates"))


PLAN_COVERS = ("fr_plan_grid", "fr_occ_freespace", "fr_plan_tiers", "fr_plan_field", "fr_plan_paths")      # setup_start + plan_paths


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
    return Case(name="path_plan_grid_field_paths", make=make, call=call, setup=setup, exact=("occ_plan", "free", "field", "paths"),
                covers=PLAN_COVERS)


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
    return Case(name="popgs_criterion", make=make, call=call, exact=("scores", "prior_out"), bounds={"vis": (1, 100)}, same=("accumulate",),
                covers=("fr_popgs_diag_criterion",))


# -- entry points from before the table had a `covers` column, found by the completeness check ---------------------------------------------

def _forward_features_case(n):
    """fr_forward_features over the geometry a forward binned beforehand (the buffers are inputs like any other)"""
    def call(ctx, b):
        from fisher_rast import ops
        cam = _camera(SORT_W, SORT_H)
        P = int(b["means3D"].shape[0])
        args = (P, SORT_H, SORT_W, cam.tanfovx, cam.tanfovy, 1.0, b["bg"], b["view"], b["proj"], b["campos"])
        return dict(feature_image=ops.rasterize_forward_features(b["features"], args, b["geom"], b["binning"], b["img"]))
    return Case(name=f"forward_features_n{n}", make=lambda which: _sort_scene(n, which, features=True), call=call, prepare=_prepare_forward(False),
                exact=("feature_image",), same=CAMERA_NAMES + ("opacity", "scales", "rotations"), covers=("fr_forward_features",))


def _backward_abi_case(n, power):
    """fr_backward, the entry point without a scratch buffer, through the C ABI (no Python layer calls it): the arguments of
    ops.rasterize_backward, the same outputs by the same rule"""
    def call(ctx, b):
        import torch
        from fisher_rast import _lib, ops
        dev = b["means3D"].device
        cam = _camera(SORT_W, SORT_H)
        P = int(b["means3D"].shape[0])
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        out = dict(dL_dmeans2D=new(P, 3), dL_dcolors=new(P, 3), dL_dopacity=new(P, 1), dL_dmeans3D=new(P, 3), dL_dcov3D=new(P, 6),
                   dL_dscales=new(P, 3), dL_drotations=new(P, 4), dL_dconic=new(P, 2, 2))
        cfg = ops._raster_cfg(P, SORT_H, SORT_W, cam.tanfovx, cam.tanfovy, 1.0, 0, 0, False, b["bg"], b["view"], b["proj"], b["campos"])
        g = ops._gaussians(b["means3D"], b["colors"], None, None, b["scales"], b["rotations"], None)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().fr_backward(ctypes.byref(cfg), ctypes.byref(g), b["radii"].data_ptr(), b["geom"].data_ptr(),
                                               b["binning"].data_ptr(), b["img"].data_ptr(), b["dL"].data_ptr(), power,
                                               *(out[k].data_ptr() for k in ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D")),
                                               None, out["dL_dscales"].data_ptr(), out["dL_drotations"].data_ptr(), out["dL_dconic"].data_ptr(),
                                               ops._stream(dev)), "fr_backward")
        return out
    rule = (1e-4, 2e-5)
    return Case(name=f"backward_abi_p{power}_n{n}", make=lambda which: _sort_scene(n, which, dL=True), call=call, prepare=_prepare_forward(False),
                close={k: rule for k in ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D")},
                close_from="test_gpu_rasterizer_parity.py::test_backward_parity (1e-4, atol_frac 2e-5)",
                same=CAMERA_NAMES + ("opacity", "scales", "rotations"), covers=("fr_backward",))


def _backward_pair_abi_case(n):
    """fr_backward_pair, likewise: the arguments of ops.rasterize_backward_pair without the scratch buffer"""
    def call(ctx, b):
        import torch
        from fisher_rast import _lib, ops
        dev = b["means3D"].device
        cam = _camera(SORT_W, SORT_H)
        P = int(b["means3D"].shape[0])
        new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)
        shapes = dict(dL_dmeans2D=(P, 3), dL_dmeans2D_features=(P, 3), dL_dcolors=(P, 3), dL_dfeatures=(P, 3), dL_dopacity=(P, 1), dL_dmeans3D=(P, 3),
                      dL_dcov3D=(P, 6), dL_dscales=(P, 3), dL_drotations=(P, 4), dL_dconic=(P, 2, 2))
        out = {k: new(*s) for k, s in shapes.items()}
        cfg = ops._raster_cfg(P, SORT_H, SORT_W, cam.tanfovx, cam.tanfovy, 1.0, 0, 0, False, b["bg"], b["view"], b["proj"], b["campos"])
        g = ops._gaussians(b["means3D"], b["colors"], None, None, b["scales"], b["rotations"], None)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().fr_backward_pair(ctypes.byref(cfg), ctypes.byref(g), b["radii"].data_ptr(), b["geom"].data_ptr(),
                                                    b["binning"].data_ptr(), b["img"].data_ptr(), b["dL"].data_ptr(), b["features"].data_ptr(),
                                                    b["dLf"].data_ptr(), *(out[k].data_ptr() for k in shapes), ops._stream(dev)), "fr_backward_pair")
        return out
    rule = (1e-4, 1e-6)
    return Case(name=f"backward_pair_abi_n{n}", make=lambda which: _sort_scene(n, which, features=True, dL=True), call=call,
                prepare=_prepare_forward(True),
                close={k: rule for k in ("dL_dmeans2D", "dL_dmeans2D_features", "dL_dcolors", "dL_dfeatures", "dL_dopacity", "dL_dmeans3D")},
                close_from="test_gpu_rasterizer_parity.py::test_fused_rgb_depth_silhouette_pair (1e-4, atol_frac 1e-6)",
                same=CAMERA_NAMES + ("opacity", "scales", "rotations"), covers=("fr_backward_pair",))


FRONTIER_XYZ = 1027


def _frontier_map(which):
    """the door map with a block of unknown cells on its far side: the right-hand columns (real) or the bottom rows of the right-hand
    room (decoy), so that the free space has a frontier"""
    occ = _plan_map(which)["occ_map"].copy()
    block = (slice(None), slice(44, None)) if which == 0 else (slice(36, None), slice(27, None))
    occ[0][block], occ[1][block], occ[2][block] = 1.0, 0.0, 0.0
    return occ


def _frontier_case():
    """build_frontiers (free space, fr_occ_frontiers, host reads), sample_random_candidate on the free space it left (erode,
    fr_occ_free_candidates, a host read) and cells_of (fr_occ_cells_of)"""
    def make(which):
        rng = np.random.default_rng([which, 79])
        return dict(occ_map=_frontier_map(which), xyz=rng.uniform(-1.6, 1.6, (FRONTIER_XYZ, 3)).astype(F))

    def setup(b, dev):
        p = _planner(_plan_map(0), dev)
        p.occ_map = b["occ_map"]
        p.cam_pos = np.array(_plan_map(0)["start"])
        p.frontier_select_method = "largest"
        return p

    def call(p, b):
        import torch
        # an out-of-range point (far above the height window) makes build_frontiers return the whole cell list, not the one FBE pick
        probe = torch.tensor([[0.0, 100.0, 0.0]], device=b["occ_map"].device)
        pts, free = p.build_frontiers(probe)
        assert pts is not None and len(pts) >= 10, "the map has no frontier: the case proves nothing"
        poses = p.sample_random_candidate(np.array([0.0, 0.4, 0.0]), None, seed=41)
        cells = p.cells_of(b["xyz"])
        return dict(frontier=torch.from_numpy(p.frontier), target=torch.from_numpy(p.target_frontier), selected=torch.from_numpy(pts),
                    free=torch.from_numpy(free), poses=poses, cells=cells)
    return Case(name="occupancy_frontiers_free_candidates_cells", make=make, call=call, setup=setup,
                exact=("frontier", "target", "selected", "free", "poses", "cells"),
                covers=("fr_occ_freespace", "fr_occ_frontiers", "fr_occ_erode", "fr_occ_free_candidates", "fr_occ_cells_of"))


# -- nearest point of another cloud (fisher_rast/cloud.py) ---------------------------------------------------------------------------------

CLOUD_N, CLOUD_M = 1500, 700         # two 1024-point boxes, a ragged last 64-point sub-box (1500 = 23 * 64 + 28)
CLOUD_DEPTH_HW, CLOUD_DEPTH_STRIDE = (24, 32), 2


def _cloud_points_case():
    def make(which):
        import cloud_cases as cc
        t, q = cc.make_case("clusters", CLOUD_N, CLOUD_M, seed=which)
        return dict(points=t, queries=q)

    def call(ctx, b):
        from fisher_rast.cloud import CloudIndex
        return CloudIndex(b["points"]).search(b["queries"], 0.05, dist=True, index=True, flag=True, stats=True)      # the build is on the stream too
    return Case(name="cloud_build_search", make=make, call=call, exact=("dist", "index", "flag", "stats"), sync_free=True, repeat=True,
                covers=("fr_cloud_index_build", "fr_cloud_query"))


def _cloud_depth_case():
    def make(which):
        import cloud_cases as cc
        c = cc.make_depth_case(*CLOUD_DEPTH_HW, "object", "-Z", seed=which)
        depth = np.where(np.isfinite(c["depth"]), c["depth"], F(0.0)).astype(F)        # (the table's inputs are finite: inf and NaN pixels become "no depth")
        return dict(env=c["env"], depth=depth, kinv=np.ascontiguousarray(cc.depth_kinv(c), F), c2w=c["c2w"])

    def call(ctx, b):
        from fisher_rast.cloud import CloudIndex
        mask, stats, dist = CloudIndex(b["env"]).query_depth(b["depth"], b["kinv"], b["c2w"], stride=CLOUD_DEPTH_STRIDE, flip_z=True, dist_th=0.05,
                                                            want_dist=True)
        return dict(mask=mask, stats=stats, dist=dist)
    return Case(name="cloud_query_depth", make=make, call=call, exact=("mask", "stats", "dist"), same=("kinv",), sync_free=True, repeat=True,
                covers=("fr_cloud_index_build", "fr_cloud_query"))


# -- DBSCAN and the target selection (fisher_rast/cluster.py) -------------------------------------------------------------------------------

CLUSTER_N = 1500
SELECT_BAND = (-0.6, 0.6)            # wider than cluster_cases' band: more than 256 of the 1500 rows lie in it (held in test_stream_cases_cpu.py)


def _dbscan_case():
    def make(which):
        import cluster_cases as cl
        return dict(points=cl.make_case("blobs", CLUSTER_N, seed=which))

    def call(ctx, b):
        import cluster_cases as cl
        from fisher_rast import cluster
        labels, status = cluster.dbscan_raw(b["points"], cl.EPS, cl.MIN_SAMPLES)
        return dict(labels=labels, status=status)
    return Case(name="dbscan_raw", make=make, call=call, exact=("labels", "status"), sync_free=True, repeat=True, covers=("fr_dbscan",))


def _select_inputs(which):
    import cluster_cases as cl
    means, scores = cl.make_select_case(CLUSTER_N, seed=which)
    return dict(means3D=means, scores=scores)


def _select_target_case():
    def call(ctx, b):
        import torch
        import cluster_cases as cl
        from fisher_rast import cluster
        r = cluster.select_target(b["means3D"], b["scores"], SELECT_BAND[0], SELECT_BAND[1], cl.Q, cl.EPS, cl.MIN_SAMPLES)        # one host read inside
        assert not r.nan_scores
        return dict(band=r.points_index_range, above=r.points_index, labels=r.labels, selected=r.selected_points_index, threshold=r.threshold.reshape(1),
                    counts=torch.tensor([r.n_band, r.n_above, r.n_clusters, r.max_label, r.n_selected, r.argmax], dtype=torch.int64))
    return Case(name="select_target", make=_select_inputs, call=call, exact=("band", "above", "labels", "selected", "threshold", "counts"),
                covers=("fr_target_select",))


# -- render-quality evaluation (ops.view_metrics) ----------------------------------------------------------------------------------------------

EVAL_SHAPE = (3, 24, 40)             # the 11-tap SSIM window fits


EVAL_FAMILIES = (("noise", "smooth", "step"), ("smooth", "out_of_range", "noise"))      # per view: real, decoy


def _eval_batch(which):
    """Three views of eval_cases' families with a half mask and a garbage fourth byte.  The decoy is other content, not the real set
    rearranged: other families per view, every view, mask and alpha from other seeds (a mirrored or permuted batch would give the same
    sums, hence the same rows up to rounding).  tests/test_stream_cases_cpu.py holds every column of every row apart."""
    import eval_cases as ec
    V, H, W = EVAL_SHAPE
    views = [ec.make_view((H, W), family, v + 10 * which) for v, family in enumerate(EVAL_FAMILIES[which])]
    rng = np.random.default_rng([which, 107])
    gt_u8 = np.stack([t[1] for t in views])
    alpha = rng.integers(0, 256, (V, H, W, 1), dtype=np.uint8)
    d = dict(render=np.stack([t[0] for t in views]), gt_f32=ec.u8_to_f32(gt_u8), gt_u8x4=np.concatenate((gt_u8, alpha), axis=-1),
             depth=np.stack([t[2] for t in views]), gt_depth=np.stack([t[3] for t in views]),
             mask=(rng.uniform(size=(V, H, W)) < 0.5).astype(np.uint8))
    return {k: np.ascontiguousarray(v) for k, v in d.items()}


def _view_metrics_cases():
    def make_f32(which):
        d = _eval_batch(which)
        return {k: d[k] for k in ("render", "gt_f32", "depth", "gt_depth", "mask")}

    def make_u8(which):
        d = _eval_batch(which)
        return {k: d[k] for k in ("render", "gt_u8x4")}

    def call_f32(ctx, b):
        from fisher_rast import ops
        # (depth_valid_only: the depth count of a row is then the view's number of measured pixels, not H W for every view)
        r = ops.view_metrics(b["render"], b["gt_f32"], b["depth"], b["gt_depth"], b["mask"], depth_valid_only=True)
        return dict(rows=r["rows"], summary=r["summary"], summary_of_rows=ops.view_metrics_summary(r["rows"]))

    def call_u8(ctx, b):
        from fisher_rast import ops
        r = ops.view_metrics(b["render"], b["gt_u8x4"])
        return dict(rows=r["rows"], summary=r["summary"], summary_of_rows=ops.view_metrics_summary(r["rows"]))
    covers = ("fr_view_metrics", "fr_view_metrics_summary")
    out = ("rows", "summary", "summary_of_rows")
    return [Case(name="view_metrics_f32_depth_mask", make=make_f32, call=call_f32, exact=out, sync_free=True, repeat=True, covers=covers),
            Case(name="view_metrics_u8x4", make=make_u8, call=call_u8, exact=out, sync_free=True, repeat=True, covers=covers, images=("gt_u8x4",))]


# -- the object-aware training step (fisher_rast/object_loss.py, slam_external.get_gaussians_outside_mask) ------------------------------------

OBJLOSS_SHAPE = (24, 32)
OUTSIDE_P, OUTSIDE_MASK = 2000, (48, 64)


def _loss_mask_case(reject):
    """loss_pixel_mask with the object mask ANDed in: one launch, or -- reject_outliers -- five, the radix-select median between them"""
    def make(which):
        import objloss_cases as oc
        ds, gt = oc.make_mask_case(OBJLOSS_SHAPE, ("neg_zero_gt", "mostly_unmeasured")[which])
        return dict(depth_sil=ds, gt_depth=gt, obj=oc.make_obj(OBJLOSS_SHAPE, "half", seed=which))

    def call(ctx, b):
        import torch
        import objloss_cases as oc
        from fisher_rast import object_loss
        depth, mask = object_loss.loss_pixel_mask(b["depth_sil"], b["gt_depth"], oc.SIL_THRES, reject, True, b["obj"])
        return dict(mask=mask.view(torch.uint8))
    return Case(name=f"loss_mask{'_reject_outliers' if reject else ''}", make=make, call=call, exact=("mask",), sync_free=True, repeat=True,
                covers=("fr_loss_mask",))


def _bg_penalty_case():
    def make(which):
        import objloss_cases as oc
        im, ds, obj = oc.make_penalty_case(OBJLOSS_SHAPE, ("plain", "sil_edges")[which], "half")
        return dict(im=im, depth_sil=ds, obj=obj, upstream=np.array([(0.37, 1.9)[which]], F))

    def call(ctx, b):
        import torch
        import objloss_cases as oc
        from fisher_rast import object_loss
        im, ds = b["im"].detach().requires_grad_(True), b["depth_sil"].detach().requires_grad_(True)          # leaves over the work buffers
        penalty = object_loss.background_penalty(im, ds, b["obj"], oc.LAMBDA, oc.LAMBDA)
        g_im, g_ds = torch.autograd.grad(penalty, (im, ds), grad_outputs=b["upstream"].reshape(()))
        return dict(penalty=penalty.detach().reshape(1), g_im=g_im, g_depth_sil=g_ds)
    return Case(name="background_penalty", make=make, call=call, exact=("penalty", "g_im", "g_depth_sil"), same=("obj",), sync_free=True, repeat=True,
                covers=("fr_bg_penalty_forward", "fr_bg_penalty_backward"))


def _outside_mask_case():
    def make(which):
        import objloss_cases as oc
        c = oc.make_outside_case(OUTSIDE_P, OUTSIDE_MASK, 3, "general", seed=which)
        p = oc.trajectory_params(c)
        return dict(means3D=c["means"], log_scales=c["logs"], cam_unnorm_rots=p["cam_unnorm_rots"].numpy(), cam_trans=p["cam_trans"].numpy(),
                    K=c["K"], obj=c["obj"])

    def call(ctx, b):
        import torch
        from models.SLAM.utils import slam_external as se
        params = {k: b[k] for k in ("means3D", "log_scales", "cam_unnorm_rots", "cam_trans")}
        outside, stats = se.get_gaussians_outside_mask(params, dict(id=1, intrinsics=b["K"]), b["obj"])       # one host read inside
        ranges = torch.tensor([stats[k] for k in ("inside_scale_min", "inside_scale_max", "outside_scale_min", "outside_scale_max")], dtype=torch.float64)
        return dict(outside=outside.view(torch.uint8), idx_in=stats["idx_in"], idx_out=stats["idx_out"], ranges=ranges)
    return Case(name="outside_mask", make=make, call=call, exact=("outside", "idx_in", "idx_out", "ranges"), same=("K", "cam_trans"),
                covers=("fr_outside_mask",))


# -- action planning and the roll-out (planning/astar.py: plan_actions, plan_actions_object; fr_rollout_actions) ---------------------------

ACTION_STEP = dict(forward_step_size=0.065, turn_angle=10.)
ACTION_QUEUE = 30
ROLLOUT_LISTS = 70


def _action_poses(c, pose_of):
    """(the agent's pose on the start cell, the goal poses [G, 4, 4] float32 in the middle of the map's goal cells): host values, the same
    for both door maps.  A cell (row, col) has its middle at ((col, row) - grid_dim // 2 + 0.5) * cell + centre (convert_to_map)."""
    rng = np.random.default_rng(83)
    half = np.array([c["W"] // 2, c["H"] // 2])
    world = lambda row, col: (np.array([col, row]) - half + 0.5) * c["cell"] + np.asarray(c["center"])
    x, z = world(*c["start"])
    agent = pose_of(0.3, x, c["cam_height"], z)
    goals = np.zeros((len(c["goals"]), 4, 4), np.float32)
    for g, (row, col) in enumerate(c["goals"]):
        x, z = world(row, col)
        goals[g] = pose_of(rng.uniform(-np.pi, np.pi), x, rng.uniform(0.2, 1.5), z, np.float32)
    return agent, goals


def _plan_tensors(plan):
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    return dict(n_actions=t(plan.n_actions), keep=t(plan.keep), actions=t(plan.actions), cells=t(plan.map_xz), xz=t(plan.c2w_xz), w2c=plan.w2c)


PLAN_OUT = ("n_actions", "keep", "actions", "cells", "xz", "w2c")


def _plan_actions_cases():
    def make(which):
        return dict(occ_map=_plan_map(which)["occ_map"])

    def setup(b, dev):
        p = _planner(_plan_map(0), dev)
        p.occ_map = b["occ_map"]
        return p

    def call(p, b):
        import action_cases as ac
        c = _plan_map(0)
        agent, goals = _action_poses(c, ac.yaw_pose)
        p.setup_start(np.array(c["start"]))
        return _plan_tensors(p.plan_actions(goals, agent, queue_size=ACTION_QUEUE, **ACTION_STEP))

    def call_object(p, b):
        import torch
        import goal_cases as gc
        c = _plan_map(0)
        agent, goals = _action_poses(c, gc.cam_pose)
        p.setup_start(np.array(c["start"]))
        plan = p.plan_actions_object(goals, agent, **ACTION_STEP)
        flat = np.concatenate([np.asarray(q, np.int64).reshape(-1) for q in plan.pruned] + [np.array([len(q) for q in plan.pruned], np.int64)])
        return dict(pruned=torch.from_numpy(flat), **_plan_tensors(plan))
    return [Case(name="plan_actions", make=make, call=call, setup=setup, exact=PLAN_OUT, covers=PLAN_COVERS + ("fr_plan_actions",)),
            Case(name="plan_actions_object", make=make, call=call_object, setup=setup, exact=PLAN_OUT + ("pruned",),
                 covers=PLAN_COVERS + ("fr_plan_actions_object",))]


def _rollout_case():
    """fr_rollout_actions through the C ABI (fisher_rast.path_eval.rollout_device takes host lists only): the action lists and their
    lengths are device buffers"""
    def make(which):
        rng = np.random.default_rng([which, 89])
        return dict(actions=rng.integers(1, 4, (ROLLOUT_LISTS, ACTION_QUEUE)).astype(np.uint8),
                    lengths=rng.integers(0, ACTION_QUEUE + 1, ROLLOUT_LISTS).astype(np.int32))

    def call(ctx, b):
        import torch
        import action_cases as ac
        from fisher_rast import _lib
        dev = b["actions"].device
        w2c = torch.empty((ROLLOUT_LISTS, ACTION_QUEUE, 4, 4), dtype=torch.float32, device=dev)
        c2w = torch.empty((ROLLOUT_LISTS, ACTION_QUEUE, 4, 4), dtype=torch.float64, device=dev)
        start = (ctypes.c_double * 16)(*[float(v) for v in ac.yaw_pose(0.3, 0.1, 0.5, -0.2).reshape(-1)])
        with torch.cuda.device(dev):
            _lib.check(_lib.load().fr_rollout_actions(start, b["actions"].data_ptr(), b["lengths"].data_ptr(), ROLLOUT_LISTS, ACTION_QUEUE,
                                                      ACTION_STEP["forward_step_size"], ACTION_STEP["turn_angle"], w2c.data_ptr(), c2w.data_ptr(),
                                                      ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "fr_rollout_actions")
        return dict(w2c=w2c, c2w=c2w)
    return Case(name="rollout_actions", make=make, call=call, exact=("w2c", "c2w"), bounds={"actions": (1, 4), "lengths": (0, ACTION_QUEUE + 1)},
                sync_free=True, repeat=True, covers=("fr_rollout_actions",))


# -- goal selection of the object round (planning/astar.py: build_object_frontiers, _grid_candidates) ------------------------------------------

OBJECT_BLOCK = 24                    # the object's Gaussians fall into a block of 24 x 24 cells
OBJECT_COUNTS = (3, 4, 5, 6, 4, 5)   # per cell, in equal shares: a sixth of the cells has exactly 3 (not "more than 3"), 480 cells have more
GRID_CENTRES = 300


def object_points(which):
    """[N, 3] object Gaussians and the (col, row) of the cells that hold more than 3 of them: a block of cells of the 52 x 46 map, each
    with 3 to 6 points near its middle (the same total for both input sets)"""
    c = _plan_map(0)
    rng = np.random.default_rng([which, 97])
    col0, row0 = ((10, 10), (22, 14))[which]
    cols, rows = np.meshgrid(np.arange(col0, col0 + OBJECT_BLOCK), np.arange(row0, row0 + OBJECT_BLOCK))
    cells = np.stack([cols.ravel(), rows.ravel()], axis=1)
    counts = rng.permutation(np.resize(np.array(OBJECT_COUNTS), len(cells)))
    rep = np.repeat(cells, counts, axis=0)
    mid = (rep - (np.array([c["W"], c["H"]]) - 1) // 2 + 0.5) * c["cell"] + np.asarray(c["center"])        # fr_occ_object_cells' own rule
    xz = mid + rng.uniform(-0.015, 0.015, mid.shape)
    pts = np.stack([xz[:, 0], rng.uniform(-0.3, 0.3, len(xz)), xz[:, 1]], axis=1).astype(F)
    return pts[rng.permutation(len(pts))], cells[counts > 3]


def _goal_planner(b, dev):
    p = _planner(_plan_map(0), dev)
    p.occ_map = b["occ_map"]
    p.K_object, p.radius_object, p.min_range_object = 138, 0.9, 0.3
    return p


def _object_goal_cases():
    def make(which):
        c = _plan_map(which)
        return dict(occ_map=c["occ_map"], free=c["free"], points=object_points(which)[0])

    def call(p, b):
        import torch
        centres = p.build_object_frontiers(b["points"])                  # reads the number of cells back
        eroded = p._eroded_free(b["free"], 3)
        c2w, keep = p._grid_candidates(None, 1, eroded=eroded, min_free=40, seed=11, cells_dev=p._object_cells_dev)
        return dict(centres=torch.from_numpy(centres), eroded=eroded, c2w=c2w, keep=keep.view(torch.uint8))

    def make_single(which):
        rng = np.random.default_rng([which, 101])
        eroded = _plan_map(which)["free"].copy()
        eroded[:, :4 + 3 * which] = 0
        return dict(occ_map=_plan_map(which)["occ_map"], centres=rng.uniform(-0.8, 0.8, (GRID_CENTRES, 2)).astype(F), eroded=eroded)

    def call_single(p, b):
        import torch
        c2w, keep = p._grid_candidates(b["centres"], 1, eroded=b["eroded"], min_free=40, seed=11)
        return dict(c2w=c2w, keep=keep.view(torch.uint8))
    return [Case(name="object_cells_grid_candidates", make=make, call=call, setup=_goal_planner, exact=("centres", "eroded", "c2w", "keep"),
                 covers=("fr_occ_object_cells", "fr_occ_erode", "fr_occ_grid_candidates")),
            Case(name="grid_candidates_device_centres", make=make_single, call=call_single, setup=_goal_planner, exact=("c2w", "keep"),
                 sync_free=True, repeat=True,
                 covers=("fr_occ_grid_candidates",))]


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
            _forward_features_case(n), _backward_abi_case(n, 1), _backward_pair_abi_case(n), _frontier_case(),
            _cloud_points_case(), _cloud_depth_case(), _dbscan_case(), _select_target_case(), *_view_metrics_cases(),
            _loss_mask_case(False), _loss_mask_case(True), _bg_penalty_case(), _outside_mask_case(),
            *_plan_actions_cases(), _rollout_case(), *_object_goal_cases(),
        ]
    return _TABLE


def by_name(name):
    return next(c for c in cases() if c.name == name)


def names():
    return [c.name for c in cases()]
