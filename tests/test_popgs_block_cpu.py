"""The POp-GS block stage without a GPU (fr_raster_cfg.ext of fr_fisher_views; csrc/fr_popgs_block.hip): the header's arithmetic
(csrc/fr_popgs_block_math.h, compiled with g++ in tests/harness/fr_popgs_block_harness.cpp) against the binary64 NumPy restatement of
tests/popgs_block_cases.py within the derived bound, on exactly the cases the GPU test runs; the ctypes mirrors against the header's
layout; the argument checks of the call, every one made before any device work; the harness under the address and UB sanitizers."""
import ctypes
import os
import re

import numpy as np
import pytest

import popgs_block_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def h():
    return pc.build_harness()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from fisher_rast import _lib
    return _lib.load()


# ---- 1. the arithmetic ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flags", pc.FLAG_SETS, ids=pc.flag_id)
def test_factor_and_terms_against_numpy(h, flags):
    """the header's L D L^T: pivots, trace(A^-1) and sum log|pi| of SPD blocks and of indefinite ones whose pivots stay apart from 0"""
    cols = pc.columns(**flags)
    d = len(cols)
    assert h.frpbh_dim(*pc._orf(flags)) == d
    got_cols = (ctypes.c_int * d)()
    h.frpbh_cols(*pc._orf(flags), got_cols)
    assert list(got_cols) == cols
    rng = np.random.default_rng(7 + d)
    blocks = [(pc.sym_lower(b.astype(np.float64)) + 1e-6 * np.eye(d), False) for b in pc.spd_blocks(rng, 12, d, 2)]
    blocks += [(pc.sym_lower(pc.indefinite_block(rng, d).astype(np.float64)), True) for _ in range(6)]
    for A, indefinite in blocks:
        kappa = float(np.linalg.cond(A))
        assert kappa <= pc.KAPPA_MAX
        flag, piv, tr, la = pc.harness_factor(h, A)
        want_piv = pc.np_pivots(A)
        assert flag == int((want_piv <= 0).any()) == int(indefinite)
        if indefinite:
            assert np.abs(want_piv).min() >= 0.1 and (want_piv < 0).any() and (want_piv > 0).any()
        assert np.allclose(piv, want_piv, rtol=1e-9 * max(1.0, kappa * 1e-6), atol=0)
        want_tr = float(np.trace(np.linalg.inv(A)))
        sign, want_la = np.linalg.slogdet(A)
        assert sign == np.prod(np.sign(piv))
        assert abs(tr - want_tr) <= 8 * (d + 1) * pc.U * kappa * max(abs(want_tr), np.abs(np.linalg.eigvalsh(np.linalg.inv(A))).sum())
        assert abs(la - want_la) <= 8 * d * (d + 1) * pc.U * kappa


def test_the_two_d7_blocks_take_different_columns(h):
    """the header's column list (frpb_col through the harness) for every flag set: the reference's order, and d = 7 twice"""
    def header_cols(**f):
        d = h.frpbh_dim(*pc._orf(f))
        out = (ctypes.c_int * d)()
        h.frpbh_cols(*pc._orf(f), out)
        return list(out)
    assert header_cols(use_opacity=True, use_rot=False, use_scale=True) == [0, 1, 2, 3, 4, 5, 6]
    assert header_cols(use_opacity=False, use_rot=True, use_scale=False) == [0, 1, 2, 7, 8, 9, 10]
    assert header_cols(use_opacity=True, use_rot=True, use_scale=True) == [0, 1, 2, 3, 7, 8, 9, 10, 4, 5, 6]
    assert sorted(len(header_cols(**f)) for f in pc.FLAG_SETS) == [3, 4, 6, 7, 7, 8, 10, 11]
    from models.SLAM.gaussian_object import ObjectFisherOps
    for f in pc.FLAG_SETS:
        assert header_cols(**f) == pc.columns(**f) == ObjectFisherOps._block_columns(f["use_rot"], f["use_scale"], f["use_opacity"])


@pytest.mark.parametrize("name,kw", pc.SCORE_CASES, ids=[c[0] for c in pc.SCORE_CASES])
@pytest.mark.parametrize("criterion", [pc.TOPT, pc.DOPT], ids=["topt", "dopt"])
def test_harness_scores_lie_within_the_bound(h, name, kw, criterion):
    """the cases of tests/test_gpu_popgs_block.py, through g++: already within the bound the kernels are held to"""
    case = pc.make_case(**kw)
    want = pc.restate(case, criterion)
    scores, matched, status = pc.harness_scores(h, case, criterion)
    assert np.array_equal(matched, want["matched"]) and status[0] == want["matched"].sum() and status[2] == 0 and status[3] == 0
    pc.check_scores(scores, want, name)


@pytest.mark.parametrize("flags", pc.FLAG_SETS, ids=pc.flag_id)
def test_zero_rows_give_a_dopt_term_of_exactly_zero(h, flags):
    case = pc.make_case(5, 64, 2, 3, 40, flags)
    case["rows"][:] = 0.0
    case["rows"][1, :, :] = -0.0
    scores, matched, _ = pc.harness_scores(h, case, pc.DOPT)
    assert matched.sum() > 0 and all(s == 0.0 for s in scores)
    t, _, _ = pc.harness_scores(h, case, pc.TOPT)
    assert all(np.isfinite(t)) and all(t < 0)


def test_an_indefinite_prior_is_counted_and_scored_from_absolute_pivots(h):
    case = pc.make_case(9, 50, 2, 2, 20, pc.FULL)
    rng = np.random.default_rng(3)
    case["prior"][4] = pc.indefinite_block(rng, 11)
    case["rows"][:, case["idx"][4], :] *= 1e-3
    case["vis"][:, case["idx"][4]] = 1
    for criterion in (pc.TOPT, pc.DOPT):
        want = pc.restate(case, criterion)
        scores, matched, status = pc.harness_scores(h, case, criterion)
        assert status[2] == (2 if criterion == pc.TOPT else 4)           # two poses: A1 each, and A0 too under D-opt
        pc.check_scores(scores, want, "indefinite")


def test_indices_out_of_range_are_skipped_and_counted_and_a_pose_without_a_match_scores_minus_inf(h):
    case = pc.make_case(11, 80, 3, 2, 30, pc.FULL)
    case["idx"][7], case["idx"][19] = 80, -1
    case["vis"][2, :] = 0
    want = pc.restate(case, pc.TOPT)
    scores, matched, status = pc.harness_scores(h, case, pc.TOPT)
    assert want["skipped"] == 2 and status[3] == 2 and matched[2] == 0 and scores[2] == -np.inf
    pc.check_scores(scores, want, "skipped")


@pytest.mark.parametrize("K", [1, 2, 3])
def test_prior_block_is_binary32_in_the_stated_order(h, K):
    """(sum_k g_a g_b) / K as b = fma(g_a, g_b, b) from 0, k ascending (the chain of torch's einsum on the device: one rounding per
    probe); the first keyframe is stored, the next ones added"""
    rng = np.random.default_rng(K)
    for flags in pc.FLAG_SETS:
        cols = pc.columns(**flags)
        d = len(cols)
        rows = rng.uniform(-2, 2, (2, K, 11)).astype(np.float32)
        acc = np.full(d * (d + 1) // 2, np.nan, np.float32)
        want = None
        for f in range(2):
            assert h.frpbh_prior_add(*pc._orf(flags), rows[f].ctypes.data, 11, K, int(f == 0), acc.ctypes.data) == 0
            G = rows[f][:, cols]
            b = np.zeros((d, d), np.float32)
            for k in range(K):
                for i in range(d):
                    for j in range(i + 1):
                        b[i, j] = pc.fma32(G[k, i], G[k, j], b[i, j])
            b = b / np.float32(K)
            want = b if want is None else want + b
        got = np.zeros((d, d), np.float32)
        got[np.tril_indices(d)] = acc
        assert np.array_equal(got[np.tril_indices(d)], want[np.tril_indices(d)])
        if K > 1 and d == 11:                                             # the chain is not the sum of rounded products: the test can tell
            u = np.zeros((d, d), np.float32)
            for k in range(K):
                u = u + np.outer(rows[1][k][cols], rows[1][k][cols]).astype(np.float32)
            f = np.zeros((d, d), np.float32)
            for k in range(K):
                for i in range(d):
                    for j in range(i + 1):
                        f[i, j] = pc.fma32(rows[1][k][cols][i], rows[1][k][cols][j], f[i, j])
            assert not np.array_equal(np.tril(u), np.tril(f))


# ---- 2. the ABI ---------------------------------------------------------------------------------------------------------------------------

def test_ctypes_mirrors_equal_the_headers_layout(h):
    from fisher_rast import _lib
    out = (ctypes.c_longlong * 40)()
    assert h.frpbh_layout(out) == 32
    cfg_names = [n for n, _ in _lib.RasterCfg._fields_]
    assert cfg_names == ["P", "image_height", "image_width", "tanfovx", "tanfovy", "scale_modifier", "sh_degree", "sh_coeffs", "prefiltered",
                         "bg", "viewmatrix", "projmatrix", "campos", "ext"]
    assert ctypes.sizeof(_lib.RasterCfg) == out[0] and [getattr(_lib.RasterCfg, n).offset for n in cfg_names] == list(out[1:15])
    ext_names = [n for n, _ in _lib.RasterExt._fields_]
    assert ext_names == ["kind", "mode", "K", "use_opacity", "use_rot", "use_scale", "criterion", "n", "lam", "vis_in", "out_vis", "out_vis_count",
                         "prior_blocks", "prior_idx", "out_scores", "out_matched"]
    assert ctypes.sizeof(_lib.RasterExt) == out[15] and [getattr(_lib.RasterExt, n).offset for n in ext_names] == list(out[16:32])
    c = (ctypes.c_longlong * 3)()
    h.frpbh_constants(c)
    assert c[0] == _lib.FR_EXT_POPGS_BLOCK == 1 and c[1] == _lib.FR_POPGS_BLOCK_MAX_WG
    assert c[2] == _lib.FR_POPGS_BLOCK_VISIBLE + 10 * _lib.FR_POPGS_BLOCK_SCORE + 100 * _lib.FR_POPGS_BLOCK_PRIOR
    assert ctypes.sizeof(_lib.FisherCfg) == 128
    # a fresh cfg carries no extension
    assert not _lib.RasterCfg().ext


def test_workspace_macro_equals_the_lib_function(h):
    from fisher_rast import _lib
    for P, poses in [(1, 1), (255, 1), (256, 3), (257, 64), (1100, 3), (500000, 64), (3000000, 700)]:
        assert _lib.popgs_block_workspace_bytes(P, poses) == h.frpbh_ws_bytes(P, poses), (P, poses)
    assert _lib.popgs_block_workspace_bytes(1100, 3) % 256 == 0


def test_the_header_declares_no_new_export():
    from fisher_rast import _lib
    hdr = open(os.path.join(ROOT, "include", "fisher_rast.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert not [n for n in re.findall(r"\b(fr_[a-z0-9_]+)\s*\(", code) if "block" in n]
    assert "fr_raster_ext" in code and "FR_POPGS_BLOCK_WS_BYTES" in code
    assert os.path.join(_lib._CSRC, "fr_popgs_block.hip") in _lib.UNITS and os.path.join(_lib._CSRC, "fr_popgs_block_math.h") in _lib.SOURCES


# ---- 3. the argument checks (no GPU: every rejection is made before any device work) ---------------------------------------------------

def _args(mode, P=10, poses=2, K=3):
    """a well-formed call of the block stage up to the pointers (host addresses that no check dereferences)"""
    from fisher_rast import _lib
    buf = ctypes.create_string_buffer(64)
    addr = ctypes.cast(buf, ctypes.c_void_p)
    cfg, g, fc, ext = _lib.RasterCfg(), _lib.Gaussians(), _lib.FisherCfg(), _lib.RasterExt()
    cfg.P, cfg.image_width, cfg.image_height, cfg.tanfovx, cfg.tanfovy, cfg.scale_modifier = P, 64, 48, 0.5, 0.5, 1.0
    cfg.viewmatrix = cfg.projmatrix = addr
    g.means3D = g.scales = g.rotations = addr
    fc.n_views, fc.columns, fc.w2c, fc.out_H, fc.out_H_view_stride = poses * K, 11, addr, addr, 11 * P
    ext.kind, ext.mode, ext.K, ext.use_opacity, ext.use_rot, ext.use_scale = _lib.FR_EXT_POPGS_BLOCK, mode, K, 1, 1, 1
    ext.n, ext.lam, ext.criterion = 5, 1e-6, _lib.FR_POPGS_TOPT
    if mode == _lib.FR_POPGS_BLOCK_VISIBLE:
        ext.out_vis = addr
    else:
        ext.prior_blocks = ext.prior_idx = addr
    if mode == _lib.FR_POPGS_BLOCK_SCORE:
        ext.out_scores = ext.out_matched = addr
    cfg.ext = ctypes.pointer(ext)
    return dict(cfg=cfg, g=g, fc=fc, ext=ext, addr=addr, buf=buf)


def _call(lib, a, ws_bytes=0, status=True, g=True):
    return lib.fr_fisher_views(ctypes.byref(a["cfg"]), ctypes.byref(a["g"]) if g else None, ctypes.byref(a["fc"]), a["addr"], ws_bytes, 0,
                               a["addr"] if status else None, None)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["visible", "score", "prior"])
def test_a_well_formed_call_reaches_the_workspace_check(lib, mode):
    a = _args(mode)
    assert _call(lib, a) == 3                                            # FR_ENOSPACE: every argument check passed
    msg = lib.fr_last_error().decode()
    assert "block stage" in msg and "FR_POPGS_BLOCK_WS_BYTES" in msg
    from fisher_rast import _lib
    assert _call(lib, a, _lib.popgs_block_workspace_bytes(10, 2) - 1) == 3


def test_the_block_stage_rejects_what_it_does_not_take(lib):
    from fisher_rast import _lib
    VIS, SCORE, PRIOR = _lib.FR_POPGS_BLOCK_VISIBLE, _lib.FR_POPGS_BLOCK_SCORE, _lib.FR_POPGS_BLOCK_PRIOR

    def rejected(mode, word, **change):
        a = _args(mode)
        for k, v in change.items():
            where, name = k.split("__")
            setattr(a[where], name, v(a) if callable(v) else v)
        assert _call(lib, a) == 1, change                                 # FR_EINVAL, not FR_ENOSPACE
        msg = lib.fr_last_error().decode()
        assert "block stage" in msg and word in msg, (change, msg)

    rejected(SCORE, "kind", ext__kind=2)
    rejected(SCORE, "kind", ext__kind=0)
    rejected(SCORE, "mode", ext__mode=3)
    rejected(SCORE, "multiple of K", ext__K=4)                            # 6 views, K = 4
    rejected(SCORE, "multiple of K", ext__K=0)
    rejected(SCORE, "multiple of K", fc__n_views=0)
    rejected(SCORE, "columns", fc__columns=4)
    rejected(SCORE, "every other field", fc__H_inv=lambda a: a["addr"])
    rejected(SCORE, "every other field", fc__poses_are_c2w=1)
    rejected(SCORE, "every other field", fc__dL_dpix=1e-3)
    rejected(SCORE, "every other field", fc__out_vis_count=lambda a: a["addr"].value)
    rejected(SCORE, "every other field", fc__tile_capacity=1024)
    rejected(SCORE, "rows", fc__out_H=None)
    rejected(PRIOR, "rows", fc__out_H=None)
    rejected(SCORE, "out_H_view_stride", fc__out_H_view_stride=0)
    rejected(SCORE, "n is at least 1", ext__n=0)
    rejected(PRIOR, "n is at least 1", ext__n=-3)
    rejected(SCORE, "prior_blocks", ext__prior_blocks=None)
    rejected(SCORE, "out_scores", ext__out_matched=None)
    rejected(SCORE, "criterion", ext__criterion=2)
    rejected(SCORE, "lam", ext__lam=float("nan"))
    rejected(SCORE, "lam", ext__lam=-1.0)
    rejected(SCORE, "use_opacity", ext__use_rot=2)
    rejected(SCORE, "cov3D_precomp", g__cov3D_precomp=lambda a: a["addr"])
    rejected(SCORE, "means3D", g__scales=None)
    rejected(SCORE, "w2c", fc__w2c=None)
    rejected(SCORE, "image size", cfg__image_width=0)
    rejected(SCORE, "P is at least 1", cfg__P=0)
    rejected(VIS, "nothing to compute", ext__out_vis=None)
    rejected(VIS, "vis_in", ext__vis_in=lambda a: a["addr"])
    rejected(PRIOR, "vis_in", ext__vis_in=lambda a: a["addr"])
    # null status, null fisher cfg
    a = _args(SCORE)
    assert _call(lib, a, status=False) == 1
    assert lib.fr_fisher_views(ctypes.byref(a["cfg"]), ctypes.byref(a["g"]), None, a["addr"], 0, 0, a["addr"], None) == 1
    # VISIBLE takes null rows; SCORE with vis_in reads no geometry: g may be null
    a = _args(VIS)
    a["fc"].out_H, a["fc"].out_H_view_stride = None, 0
    assert _call(lib, a) == 3
    a = _args(SCORE)
    a["ext"].vis_in = a["addr"]
    a["cfg"].viewmatrix = a["cfg"].projmatrix = None
    assert _call(lib, a, g=False) == 3
    a = _args(SCORE)
    assert _call(lib, a, g=False) == 1 and b"means3D" in lib.fr_last_error()
    # a misaligned workspace
    a = _args(SCORE)
    big = _lib.popgs_block_workspace_bytes(10, 2)
    assert lib.fr_fisher_views(ctypes.byref(a["cfg"]), ctypes.byref(a["g"]), ctypes.byref(a["fc"]), a["addr"].value + 4, big, 0, a["addr"], None) == 1
    assert b"aligned" in lib.fr_last_error()


def test_without_an_extension_the_call_is_todays(lib):
    """ext = NULL reaches the messages fr_fisher_views has always given for these arguments"""
    a = _args(1)
    a["cfg"].ext = None
    assert _call(lib, a) == 1
    msg = lib.fr_last_error().decode()
    assert "fr_fisher_views" in msg and "block stage" not in msg
    a["cfg"].bg = a["addr"]
    a["g"].colors_precomp = a["g"].opacities = a["addr"]
    a["fc"].dL_dpix = 1e-3
    assert _call(lib, a) == 3 and b"fr_fisher_workspace_bytes" in lib.fr_last_error()            # the rendering call's workspace check


# ---- 4. the harness under the sanitizers --------------------------------------------------------------------------------------------------

def test_harness_runs_clean_under_asan_and_ubsan(tmp_path):
    """a stand-alone program (its own main): nothing is preloaded into Python"""
    import harness_build
    r = harness_build.sanitized_program("fr_popgs_block_harness", "FRPB_HARNESS_MAIN", tmp_path)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
