"""-m gpu: every entry point on a non-default stream, in stream order (tests/stream_cases.py has the procedure and the cases).

  a. every case of the table through the harness: behind a blocker on a fresh stream the work buffers are overwritten with the real
     inputs, the call is made, its outputs are cloned on the stream, and only the stream is waited for;
  b. the mutation check: with the layer's stream helper patched to return the null stream the harness must report a mismatch and
     recover exactly the decoy's result (knn through ops._stream, the image loss through image_loss._stream);
  c. two caller streams on one host thread, which share the thread's side streams and events;
  d. two host threads with a stream each (side streams, error text and CU count are thread-local in the library);
  e. graph capture and replay of the scorer's launch (packed lists, 8 views: the fork / join is inside the capture) and render_launch,
     replayed on inputs changed in place;
  f. the keyframe workspaces are per stream."""
import threading

import pytest
import torch

import stream_cases as sc

pytestmark = pytest.mark.gpu


# ---- a. every family in stream order ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sc.names())
def test_stream_order(gpu, name):
    case = sc.by_name(name)
    sc.run_case(case, gpu)
    print(f"[{name}] enqueue {sc.ENQUEUE_MS[name]:.3f} ms, blocker {sc.BLOCKER_MS} ms ({sc.cycles_per_ms(gpu):.0f} cycles per ms)")


# ---- b. negative control ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,module", [("knn_dist2", "fisher_rast.ops"), ("image_loss", "fisher_rast.image_loss")])
def test_null_stream_execution_is_detected(gpu, monkeypatch, name, module):
    """the layer's stream helper returns the null stream: the kernels run at once, on the decoy that the buffers still hold"""
    import importlib
    case = sc.by_name(name)
    ref = sc.reference(case, gpu)
    monkeypatch.setattr(importlib.import_module(module), "_stream", lambda dev: sc.null_stream_of(gpu))
    got = sc.stream_run(case, ref, gpu, null_stream=True)
    monkeypatch.undo()
    assert sc.mismatches(case, got, ref.want), f"{name}: execution on the null stream went unnoticed"
    assert not sc.mismatches(case, got, ref.want_decoy), sc.mismatches(case, got, ref.want_decoy)
    # ... and the unpatched layer, same buffers (they hold `real` now: filled with decoy again first), gives the reference
    sc._fill(ref.work, ref.decoy)
    torch.cuda.synchronize()
    assert not sc.mismatches(case, sc.stream_run(case, ref, gpu), ref.want)


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


# ---- d. two host threads, one stream each ---------------------------------------------------------------------------------------------------

THREAD_CASES = ("forward_n5000", "backward_p1_n5000", "scorer_launch_hinv_packed", "knn_dist2")


def test_two_host_threads_with_a_stream_each(gpu):
    """each thread: forward, backward, scorer launch and knn, three times over, on its own stream with its own buffers; the results
    are the serial ones"""
    refs = [{n: sc.reference(sc.by_name(n), gpu) for n in THREAD_CASES} for _ in range(2)]
    sc.cycles_per_ms(gpu)
    torch.cuda.synchronize()
    errors = [[], []]

    def work(t):
        try:
            torch.cuda.set_device(gpu)
            s = torch.cuda.Stream(gpu)
            for rep in range(3):
                for n in THREAD_CASES:
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
