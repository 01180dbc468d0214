"""fr_popgs_diag_criterion on synthetic rows (tests/popgs_cases.py): every tail length, views shorter than a unit, a wave and a
workgroup, the edge of the workgroup cap, K that is no power of two, the dword load path chosen by alignment, k_popgs_reduce beyond
its first block, the clamped-prior and far-quotient branches of the D-opt term, and guard words around everything the call writes.
tests/test_gpu_popgs_path.py runs the kernel on real probe rows only: V = 5, K in {1, 4}, E % 4 in {0, 3}, aligned allocations."""
import numpy as np
import pytest
import torch

import popgs_cases as pc

pytestmark = pytest.mark.gpu

FILL = -7.0
_worst = {}                      # family -> [worst relative score error, worst prior error in 2^-24], over the whole module


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for fam, (rel, ulp) in sorted(_worst.items()):
        print(f"\npopgs synthetic, family {fam}: worst relative score error {rel:.2e}, worst prior error {ulp:.2f} x 2^-24")


def _note(family, rel, ulp):
    w = _worst.setdefault(family, [0.0, 0.0])
    w[0], w[1] = max(w[0], rel), max(w[1], ulp)


def _carve(a, gpu, off=0):
    """`a` on the device in a 1-D slice that starts `off` floats past a 16-byte boundary (a 1-D slice stays contiguous)."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 8, dtype=torch.from_numpy(a).dtype, device=gpu)
    assert buf.data_ptr() % 16 == 0
    t = buf[off:off + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() == buf.data_ptr() + off * a.itemsize
    return t


def _call(gpu, rows, prior, lam, crit, acc, vis=None, offs=(0, 0, 0)):
    """One call on fresh device copies, rows / prior_in / prior_out `offs` floats past a 16-byte boundary.  Returns the scores and
    the whole prior_out (prefilled with FILL) as NumPy, after checking that prior_in was only read."""
    from fisher_rast import ops
    V, K, E = rows.shape
    d_rows, d_prior = _carve(rows, gpu, offs[0]), _carve(prior, gpu, offs[1])
    out = _carve(np.full((V, E), FILL, dtype=np.float32), gpu, offs[2])
    d_acc = torch.tensor(acc, dtype=torch.uint8, device=gpu)
    d_vis = None if vis is None else torch.tensor(vis, dtype=torch.int32, device=gpu)
    scores = torch.full((V,), float("nan"), dtype=torch.float64, device=gpu)       # a score that is never written stays NaN
    got = ops.popgs_diag_criterion(d_rows, d_prior, lam, crit, prior_out=out, accumulate=d_acc, vis_count=d_vis, scores=scores)
    got = got.cpu().numpy()
    assert np.all(np.isfinite(got)), (crit, lam, got)
    assert np.array_equal(d_prior.cpu().numpy(), prior) and np.array_equal(d_rows.cpu().numpy(), rows)
    return got, out.cpu().numpy()


def _check_call(gpu, family, rows, prior, lam, crit, acc, label):
    """Scores and written priors against the restatement at the bounds of test_kernel_matches_float64_restatement; the blocks of
    the views that do not accumulate keep their fill value."""
    K = rows.shape[1]
    got, out = _call(gpu, rows, prior, lam, crit, acc)
    assert np.all(got <= 0) if crit == "topt" else np.all(got >= 0)
    written = [v for v, a in enumerate(acc) if a]
    rel, ulp = pc.check(got, out, rows, prior, lam, crit, K, views=written, label=label)
    for v, a in enumerate(acc):
        if not a:
            assert np.all(out[v] == np.float32(FILL)), (label, v)
    _note(family, rel, ulp)
    return rel, ulp


LENGTHS = [1, 2, 3, 4, 5, 6, 7, 1021, 1022, 1023, 1024, 1025, 1026, 1027, 98304, 98305, 98306, 98307, 98308, 300001]


@pytest.mark.parametrize("E", LENGTHS)
@pytest.mark.parametrize("family,K", [("wide", 3), ("far", 4)])
def test_lengths(gpu, family, K, E):
    """Tails of 0 .. 3 entries below one unit, around one workgroup (1024 entries), around the last length with one unit per thread
    (96 workgroups x 256 threads x 4 = 98304) and well into the grid-stride loop."""
    worst = (0.0, 0.0)
    for per_view in (False, True):
        rows, prior = pc.FAMILIES[family](3, K, E, seed=11, per_view=per_view)
        for crit in ("topt", "dopt"):
            for lam in (0.0, 1e-6):
                r = _check_call(gpu, family, rows, prior, lam, crit, [1, 0, 1], (family, E, K, per_view, crit, lam))
                worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print(f"\n{family} K={K} E={E}: worst relative score error {worst[0]:.2e}, worst prior error {worst[1]:.2f} x 2^-24")


@pytest.mark.parametrize("E", [1026, 4096])
@pytest.mark.parametrize("K", [1, 2, 3, 5, 7, 8])
@pytest.mark.parametrize("family", ["wide", "far"])
def test_probe_counts(gpu, family, K, E):
    """J = ss * (1 / K) for a power of two, ss / K otherwise, on the dword (E = 1026) and the 16-byte (E = 4096) load path."""
    worst = (0.0, 0.0)
    for per_view in (False, True):
        rows, prior = pc.FAMILIES[family](3, K, E, seed=12, per_view=per_view)
        for crit in ("topt", "dopt"):
            for lam in (0.0, 1e-6):
                r = _check_call(gpu, family, rows, prior, lam, crit, [1, 0, 1], (family, E, K, per_view, crit, lam))
                worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print(f"\n{family} K={K} E={E}: worst relative score error {worst[0]:.2e}, worst prior error {worst[1]:.2f} x 2^-24")


@pytest.mark.parametrize("V", [1, 64, 65, 130])
def test_view_counts(gpu, V):
    """k_popgs_reduce takes 64 views per block: V on either side of one block and into a third.  Views 0, 63, 64 and V - 1 see
    nothing and score exactly 0.0 (and still accumulate); every view scores the same bits alone as inside the batch."""
    from fisher_rast import ops
    E, K, lam = 1027, 2, 1e-6
    rows, prior = pc.wide(V, K, E, seed=13, per_view=True)
    blind = sorted({v for v in (0, 63, 64, V - 1) if v < V})
    vis = np.full(V, 5, dtype=np.int32)
    vis[blind] = 0
    d_rows, d_prior, d_vis = _carve(rows, gpu), _carve(prior, gpu), torch.from_numpy(vis).to(gpu)
    for crit in ("topt", "dopt"):
        got, out = _call(gpu, rows, prior, lam, crit, [1] * V, vis=vis)
        want, _ = pc.restate(rows, prior, lam, crit)
        assert np.all(got[blind] == 0.0)
        seen = vis > 0
        assert np.all(want[seen] != 0) and np.all(np.abs(got - want)[seen] <= 1e-5 * np.abs(want)[seen]), (V, crit, got, want)
        want0 = want.copy()
        want0[blind] = 0.0
        assert np.array_equal(got == 0.0, want0 == 0.0)
        pc.check(want, out, rows, prior, lam, crit, K, label=(V, crit))         # the written priors (the scores are held above)
        alone = np.empty(V)
        for v in range(V):
            alone[v] = ops.popgs_diag_criterion(d_rows[v:v + 1], d_prior[v:v + 1], lam, crit, vis_count=d_vis[v:v + 1]).item()
        assert np.array_equal(alone, got), (V, crit, np.nonzero(alone != got)[0])


@pytest.mark.parametrize("E", [1024, 98308])
def test_alignment_changes_no_bit(gpu, E):
    """E % 4 == 0 with rows, prior_in or prior_out 1, 2 or 3 floats past a 16-byte boundary takes the dword loads: the same bits as
    the 16-byte path of the aligned call (fr_popgs.hip: "a view's score does not depend on [...] alignment")."""
    V, K, lam = 3, 3, 1e-6
    rows, prior = pc.wide(V, K, E, seed=14, per_view=True)
    shifts = [tuple(s if i == t else 0 for i in range(3)) for t in range(3) for s in (1, 2, 3)] + [(1, 2, 3), (3, 3, 3)]
    for crit in ("topt", "dopt"):
        s0, o0 = _call(gpu, rows, prior, lam, crit, [1, 0, 1])
        pc.check(s0, o0, rows, prior, lam, crit, K, views=[0, 2], label=(E, crit))
        for offs in shifts:
            s, o = _call(gpu, rows, prior, lam, crit, [1, 0, 1], offs=offs)
            assert np.array_equal(s, s0), (E, crit, offs, s, s0)
            assert np.array_equal(o, o0), (E, crit, offs, int((o != o0).sum()))


GUARD, PATTERN = 64, 0xA5


def _guarded(nbytes, dtype, gpu, shift=0):
    """(whole uint8 buffer of PATTERN, the tensor of `nbytes` bytes in it with GUARD + shift bytes before and >= GUARD after)."""
    start = GUARD + shift
    buf = torch.full((start + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[start:start + nbytes].view(dtype), start


def _guards_intact(buf, start, nbytes):
    b = buf.cpu().numpy()
    return np.all(b[:start] == PATTERN) and np.all(b[start + nbytes:] == PATTERN)


@pytest.mark.parametrize("inplace", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("E,shift", [(1, 0), (2, 0), (3, 0), (5, 0), (1025, 0), (1026, 0), (1027, 0), (4, 0), (1024, 0), (4, 4), (1024, 4)])
def test_guard_words(gpu, E, shift, inplace):
    """prior_out, scores and a workspace of exactly fr_popgs_diag_criterion_workspace_bytes, each between 64 bytes of a sentinel
    pattern: every sentinel byte survives the call, and so does the block of the view that does not accumulate.  E % 4 == 0 runs on
    the 16-byte path (shift 0) and, with prior_out 4 bytes further on, on the dword path."""
    from fisher_rast import _lib, ops
    V, K, lam = 3, 3, 1e-6
    rows, prior = pc.wide(V, K, E, seed=15, per_view=True)
    acc = [1, 0, 1]
    need = int(_lib.load().fr_popgs_diag_criterion_workspace_bytes(V, E))
    assert need == V * min((((E + 3) // 4) + 255) // 256, 96) * 8
    for crit in ("topt", "dopt"):
        d_rows = _carve(rows, gpu)
        pbuf, pout, pstart = _guarded(4 * V * E, torch.float32, gpu, shift)
        sbuf, scores, sstart = _guarded(8 * V, torch.float64, gpu)
        wbuf, ws, wstart = _guarded(need, torch.float64, gpu)
        pout = pout.view(V, E)
        if inplace:
            pout.copy_(torch.from_numpy(prior))
            d_prior = pout
        else:
            pout.fill_(FILL)
            d_prior = _carve(prior, gpu)
        got = ops.popgs_diag_criterion(d_rows, d_prior, lam, crit, prior_out=pout, accumulate=torch.tensor(acc, dtype=torch.uint8, device=gpu),
                                       scores=scores, workspace=ws)
        assert got.data_ptr() == scores.data_ptr()
        assert _guards_intact(pbuf, pstart, 4 * V * E), ("prior_out", E, shift, crit)
        assert _guards_intact(sbuf, sstart, 8 * V), ("scores", E, shift, crit)
        assert _guards_intact(wbuf, wstart, need), ("workspace", E, shift, crit)
        out = pout.cpu().numpy()
        pc.check(got.cpu().numpy(), out, rows, prior, lam, crit, K, views=[0, 2], label=(E, shift, crit, inplace))
        assert np.array_equal(out[1], prior[1] if inplace else np.full(E, FILL, dtype=np.float32))


def test_branches(gpu):
    """The far-quotient branch (family far, lam = 0: d / base >= 3e38, two logarithms) and the clamped-prior branch (family wide,
    lam = 0) of the D-opt term, populated by construction and not by what a render leaves; a view of zero rows scores D-opt 0.0."""
    E = 4099
    for family, K, branch, least in (("far", 4, "far", 0.3), ("wide", 3, "clamped", 0.2)):
        for per_view in (False, True):
            rows, prior = pc.FAMILIES[family](3, K, E, seed=16, per_view=per_view)
            rows[1] = 0.0                                   # J == 0 everywhere: "J == 0 gives exactly 0"
            shares = pc.emulate(rows, prior, 0.0, "dopt")[2]
            assert shares[branch] >= least * 2 / 3, shares  # two of the three views carry the family's rows
            assert pc.emulate(rows[[0, 2]], prior if prior.ndim == 1 else prior[[0, 2]], 0.0, "dopt")[2][branch] >= least
            for lam in (0.0, 1e-6):
                got, _ = _call(gpu, rows, prior, lam, "dopt", [1, 1, 1])
                assert np.all(np.isfinite(got)) and np.all(got >= 0) and got[1] == 0.0, (family, lam, got)
                rel, ulp = _check_call(gpu, family, rows, prior, lam, "dopt", [1, 0, 1], (family, per_view, lam))
                print(f"\n{family} per_view={per_view} lam={lam:g}: shares {shares}, D-opt {got}, worst relative error {rel:.2e}")
                got, _ = _call(gpu, rows, prior, lam, "topt", [0, 0, 0])
                assert np.all(np.isfinite(got)) and np.all(got <= 0)
                _check_call(gpu, family, rows, prior, lam, "topt", [1, 0, 1], (family, per_view, lam))


@pytest.mark.parametrize("E", [1024, 1027])
def test_in_place_with_a_shared_prior(gpu, E):
    """V = 1: the shared prior (view stride 0) may be its own output; the result is the out-of-place one."""
    from fisher_rast import ops
    K, lam = 3, 1e-6
    rows, prior = pc.wide(1, K, E, seed=17)
    assert prior.shape == (E,)
    for crit in ("topt", "dopt"):
        s0, o0 = _call(gpu, rows, prior, lam, crit, [1])
        pc.check(s0, o0, rows, prior, lam, crit, K, label=(E, crit))
        d_rows, d_prior = _carve(rows, gpu), _carve(prior, gpu)
        s = ops.popgs_diag_criterion(d_rows, d_prior, lam, crit, prior_out=d_prior, accumulate=torch.ones(1, dtype=torch.uint8, device=gpu))
        assert np.array_equal(s.cpu().numpy(), s0) and np.array_equal(d_prior.cpu().numpy(), o0[0])
