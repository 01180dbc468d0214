"""-m gpu: every entry point on a non-default stream, in stream order (tests/stream_cases.py has the procedure and the cases).

  a. every case of the table through the harness: behind a blocker on a fresh stream the work buffers are overwritten with the real
     inputs, the call is made, its outputs are cloned on the stream, and only the stream is waited for; a recorder on the loaded
     library holds the case's `covers` against the entry points the call did drive;
  b. the mutation check: with the layer's stream helper patched to return the null stream the harness must report a mismatch and
     recover exactly the decoy's result -- one case per helper (ops, image_loss, cluster, cloud, object_loss, the planner's); and
     a stand-in whose clear goes to the null stream, which only the repeated call of a `repeat` case notices;
  c. two caller streams on one host thread, which share the thread's side streams and events; two cloud indexes, one per stream;
  d. two host threads with a stream each (side streams, error text and CU count are thread-local in the library);
  e. graph capture and replay of the scorer's launch (packed lists, 8 views: the fork / join is inside the capture) and render_launch,
     replayed on inputs changed in place;
  f. the keyframe and the view-metrics workspaces are per stream;
  g. the roll-out helper hands the library the stream that is current."""
import threading

import numpy as np
import pytest
import torch

import stream_cases as sc

pytestmark = pytest.mark.gpu


# ---- a. every family in stream order ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.names())
def test_stream_order(gpu, name):
    case = sc.by_name(name)
    sc.run_case(case, gpu, check_covers=True)
    print(f"[{name}] enqueue {sc.ENQUEUE_MS[name]:.3f} ms, blocker {sc.BLOCKER_MS} ms ({sc.cycles_per_ms(gpu):.0f} cycles per ms)")


# ---- b. negative control ------------------------------------------------------------------------------------------------------------------

# (case, where its layer's `_stream` lives: a module, or module:class for the planner's static method).  Each case is one stage with
# no host read inside: after a read the second stage would run on the real inputs, and the result would be neither set's.
NULL_STREAM_CONTROLS = [("knn_dist2", "fisher_rast.ops"), ("image_loss", "fisher_rast.image_loss"), ("dbscan_raw", "fisher_rast.cluster"),
                        ("cloud_build_search", "fisher_rast.cloud"), ("loss_mask_reject_outliers", "fisher_rast.object_loss"),
                        ("view_metrics_f32_depth_mask", "fisher_rast.ops"), ("grid_candidates_device_centres", "planning.astar:AstarPlanner")]


@pytest.mark.parametrize("name,where", NULL_STREAM_CONTROLS)
def test_null_stream_execution_is_detected(gpu, monkeypatch, name, where):
    """the layer's stream helper returns the null stream: the kernels run at once, on the decoy that the buffers still hold"""
    import importlib
    case = sc.by_name(name)
    ref = sc.reference(case, gpu)
    module, _, cls = where.partition(":")
    if cls:
        monkeypatch.setattr(getattr(importlib.import_module(module), cls), "_stream", staticmethod(lambda: sc.null_stream_of(gpu)))
    else:
        monkeypatch.setattr(importlib.import_module(module), "_stream", lambda dev: sc.null_stream_of(gpu))
    got = sc.stream_run(case, ref, gpu, null_stream=True)
    monkeypatch.undo()
    assert sc.mismatches(case, got, ref.want), f"{name}: execution on the null stream went unnoticed"
    assert not sc.mismatches(case, got, ref.want_decoy), sc.mismatches(case, got, ref.want_decoy)
    # ... and the unpatched layer, same buffers (they hold `real` now: filled with decoy again first), gives the reference
    sc._fill(ref.work, ref.decoy)
    torch.cuda.synchronize()
    assert not sc.mismatches(case, sc.stream_run(case, ref, gpu), ref.want)


def test_a_clear_on_the_null_stream_is_detected_by_the_repeated_call(gpu):
    """A stand-in for an entry point with a workspace kept between calls: clear it, accumulate into it.  With the clear on the null
    stream one call behind the blocker still gives the right answer (the clear only runs too soon) -- which is why the cases of the
    units that clear their accumulators with hipMemsetAsync have `repeat`: of two calls back to back the second finds the workspace
    dirty, and the harness reports it.  This holds the mechanism on a stand-in only: no real unit's memset is moved here (see
    "Memsets" in tests/stream_cases.py for what that leaves open)."""
    held = {}

    def make(which):
        return dict(x=np.random.default_rng([which, 103]).normal(size=4099).astype(np.float32))

    def call_clearing_on(stream_of):
        def call(ctx, b):
            acc = held.setdefault("acc", torch.empty_like(b["x"]))
            with torch.cuda.stream(stream_of(b["x"].device)):
                acc.zero_()
            acc.add_(b["x"])
            return dict(sum=acc.clone())
        return call
    good = sc.Case(name="stand_in_clear_accumulate", make=make, call=call_clearing_on(torch.cuda.current_stream), exact=("sum",), sync_free=True, repeat=True)
    bad = good._replace(call=call_clearing_on(torch.cuda.default_stream))
    sc.run_case(good, gpu)
    sc.run_case(bad._replace(repeat=False), gpu)                          # one call: the early clear goes unnoticed
    with pytest.raises(AssertionError, match="does not give the default-stream result"):
        sc.run_case(bad, gpu)


# ---- c. two caller streams, one host thread -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("second", ["forward_n5000", "scorer_launch_hinv_packed"])
def test_two_caller_streams_share_the_side_streams(gpu, second):
    """A (scorer launch, packed lists, 8 views: forks onto side stream [0]) on s1 behind a blocker, B on s2 without one, enqueued
    while A is still held back: both go through the same thread-local side streams and fork / join events.  Nothing is asserted
    about which finishes first."""
    a_case, b_case = sc.by_name("scorer_launch_hinv_packed"), sc.by_name(second)
    ref_a, ref_b = sc.reference(a_case, gpu), sc.reference(b_case, gpu)
    s1, s2 = sc.caller_stream(gpu), torch.cuda.Stream(gpu)
    for _ in range(32):
        if s2.cuda_stream != s1.cuda_stream:
            break
        s2 = torch.cuda.Stream(gpu)
    assert s2.cuda_stream != s1.cuda_stream
    pa = sc.enqueue(a_case, ref_a, gpu, stream=s1)
    pb = sc.enqueue(b_case, ref_b, gpu, stream=s2, blocker_ms=0)
    got_b, got_a = sc.finish(pb), sc.finish(pa)
    assert not sc.mismatches(a_case, got_a, ref_a.want), sc.mismatches(a_case, got_a, ref_a.want)
    assert not sc.mismatches(b_case, got_b, ref_b.want), sc.mismatches(b_case, got_b, ref_b.want)


def test_two_cloud_indexes_one_per_stream(gpu):
    """an index is built and searched on s1 behind a blocker, another on s2 meanwhile (one index stays on one stream, as CloudIndex
    documents; two indexes share nothing): each gives its serial result"""
    case = sc.by_name("cloud_build_search")
    ref_a, ref_b = sc.reference(case, gpu), sc.reference(case, gpu)
    s1, s2 = sc.caller_stream(gpu), torch.cuda.Stream(gpu)
    for _ in range(32):
        if s2.cuda_stream != s1.cuda_stream:
            break
        s2 = torch.cuda.Stream(gpu)
    assert s2.cuda_stream != s1.cuda_stream
    pa = sc.enqueue(case, ref_a, gpu, stream=s1)
    pb = sc.enqueue(case, ref_b, gpu, stream=s2, blocker_ms=0)
    got_b, got_a = sc.finish(pb), sc.finish(pa)
    assert not sc.mismatches(case, got_a, ref_a.want), sc.mismatches(case, got_a, ref_a.want)
    assert not sc.mismatches(case, got_b, ref_b.want), sc.mismatches(case, got_b, ref_b.want)


# ---- d. two host threads, one stream each ---------------------------------------------------------------------------------------------------

THREAD_CASES = ("forward_n5000", "backward_p1_n5000", "scorer_launch_hinv_packed", "knn_dist2")
THREAD_CASES_NEWER = ("dbscan_raw", "view_metrics_f32_depth_mask", "loss_mask_reject_outliers")


def test_two_host_threads_with_a_stream_each(gpu):
    """each thread: forward, backward, scorer launch and knn, three times over, on its own stream with its own buffers; the results
    are the serial ones"""
    _two_threads(gpu, THREAD_CASES)


def test_two_host_threads_with_a_stream_each_newer_units(gpu):
    """the same with DBSCAN (a fresh workspace per call), the view metrics (a workspace per stream) and the five-launch loss mask"""
    _two_threads(gpu, THREAD_CASES_NEWER)


def _two_threads(gpu, names):
    """thread 0 runs every case's real set, thread 1 its decoy set (the roles swapped: the decoy is what it writes into its buffers and
    what it must get), so that a workspace shared between the two streams by mistake would be written with different values"""
    refs = [{n: sc.reference(sc.by_name(n), gpu) for n in names} for _ in range(2)]
    refs[1] = {n: r._replace(real=r.decoy, decoy=r.real, want=r.want_decoy, want_decoy=r.want) for n, r in refs[1].items()}
    sc.cycles_per_ms(gpu)
    torch.cuda.synchronize()
    errors = [[], []]

    def work(t):
        try:
            torch.cuda.set_device(gpu)
            s = torch.cuda.Stream(gpu)
            for rep in range(3):
                for n in names:
                    case, ref = sc.by_name(n), refs[t][n]
                    got = sc.stream_run(case, ref, gpu, stream=s, blocker_ms=0)
                    bad = sc.mismatches(case, got, ref.want)
                    if bad:
                        errors[t].append((n, rep, bad))
        except Exception as e:                                          # noqa: BLE001 -- reported by the main thread
            errors[t].append(repr(e))

    threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join(timeout=120)
    assert not any(th.is_alive() for th in threads), "a thread did not finish"
    assert errors == [[], []], errors


# ---- e. graph capture and replay ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,changed", [("scorer_launch_hinv_packed", ("w2c", "H_inv")), ("scorer_render_launch", ("w2c",))])
def test_graph_capture_and_replay_on_changed_inputs(gpu, name, changed):
    """captured with the decoy's poses (and H_inv), replayed after they were overwritten in place with the real ones: the replay must
    read them again, through the captured fork onto the side stream and back.  The map stays as it is between capture and replay, and
    `map_changed()` in front of the capture puts the packing of the static records (H_inv rows included) into the graph."""
    case = sc.by_name(name)
    ref = sc.reference(case, gpu)                                         # the work buffers hold the decoy
    scorer, work = ref.ctx, ref.work
    cur = torch.cuda.current_stream(gpu)
    side = torch.cuda.Stream(gpu)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        for _ in range(3):
            case.call(scorer, work)
    cur.wait_stream(side)
    torch.cuda.synchronize()
    scorer.map_changed()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = case.call(scorer, work)
    for k in changed:
        work[k].copy_(ref.real[k])
    g.replay()
    torch.cuda.synchronize()
    assert int(out["_status"].cpu()[1]) == 0
    got = {k: v.clone() for k, v in sc._outputs(out).items()}
    eager = case.call(scorer, work)
    torch.cuda.synchronize()
    bad = sc.mismatches(case, got, sc._outputs(eager))
    assert not bad, bad
    # the replay did read the new values: on the captured ones it would have given the decoy's result
    assert sc.mismatches(case, got, ref.want_decoy)


# ---- f. per-stream workspaces ---------------------------------------------------------------------------------------------------------------

def test_keyframe_workspaces_are_per_stream(gpu):
    from fisher_rast import _lib, ops
    lib = _lib.load()
    n_overlap, n_pixels = int(lib.fr_keyframe_overlap_workspace_bytes(48)), int(lib.fr_keyframe_valid_pixels_workspace_bytes(48, 64))
    s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    assert s1.cuda_stream != s2.cuda_stream
    got = {}
    for tag, s in (("a", s1), ("b", s2), ("a2", s1)):
        with torch.cuda.stream(s):
            got[tag] = (ops._keyframe_workspace("overlap", (48,), gpu, n_overlap), ops._keyframe_workspace("pixels", (48, 64), gpu, n_pixels))
    for i in range(2):
        assert got["a"][i] is got["a2"][i], "one stream must get its workspace back"
        assert got["a"][i].data_ptr() != got["b"][i].data_ptr(), "two streams must not share a workspace"


def test_view_metrics_workspaces_are_per_stream(gpu):
    from fisher_rast import _lib, ops
    nbytes = int(_lib.load().fr_view_metrics_workspace_bytes(3, 24, 40))
    s1, s2 = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
    assert s1.cuda_stream != s2.cuda_stream
    got = {}
    for tag, s in (("a", s1), ("b", s2), ("a2", s1)):
        with torch.cuda.stream(s):
            got[tag] = ops._view_metrics_workspace(gpu, nbytes)
    assert got["a"] is got["a2"], "one stream must get its workspace back"
    assert got["a"].data_ptr() != got["b"].data_ptr(), "two streams must not share a workspace"


# ---- g. the roll-out helper's own stream choice -----------------------------------------------------------------------------------------------

def test_rollout_helper_passes_the_current_stream(gpu, monkeypatch):
    from fisher_rast import _lib
    from fisher_rast.path_eval import rollout_device
    lib = _lib.load()
    real, seen = lib.fr_rollout_actions, []
    monkeypatch.setattr(lib, "fr_rollout_actions", lambda *a: (seen.append(a[-1].value or 0), real(*a))[1])
    s = sc.caller_stream(gpu)
    with torch.cuda.stream(s):
        w2c, lengths = rollout_device(np.eye(4), [[1, 2, 1], [3]], 0.065, 10., device=gpu)
    s.synchronize()
    assert seen == [s.cuda_stream] and s.cuda_stream != torch.cuda.default_stream(gpu).cuda_stream
    assert lengths == [3, 1] and bool(w2c[0, :3].abs().sum() > 0) and not bool(w2c[1, 1:].any())
