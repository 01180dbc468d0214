"""CPU: the per-Gaussian view score entry point (fr_fisher_point_views) is declared, exported and bound; its workspace queries are
host-only and the per-slot accumulators lie inside the workspace; its argument checks reject what it does not support before any
device work; PointScoreOps grafts exactly its surface; and the polynomial pair factor of the score record -- which the per-Gaussian
sums inherit splat by splat, with no averaging over a view -- is within the project's entry rule of the exact value on every sampled
needle-shaped splat of `border`."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest

from scenes import intrinsics
from test_gpu_scorer_adversarial import border_scene, _views, K_DEV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fr_fisher_point_views", "fr_fisher_point_workspace_bytes", "fr_fisher_point_workspace_layout")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from fisher_rast import _lib
    return _lib.load()


def test_point_symbols_declared_and_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fisher_rast.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fr_[a-z0-9_]+)\s*\(", hdr))
    from fisher_rast import _lib
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.fr_fisher_point_views.restype is ctypes.c_int and len(lib.fr_fisher_point_views.argtypes) == 10
    assert lib.fr_fisher_point_workspace_bytes.restype is ctypes.c_size_t and len(lib.fr_fisher_point_workspace_layout.argtypes) == 7
    assert lib.fr_version() == 100
    from fisher_rast._lib import FisherCfg
    assert ctypes.sizeof(FisherCfg) == 128                     # fr_fisher_cfg keeps its layout


@pytest.mark.parametrize("columns", [4, 11])
def test_point_workspace_queries_are_host_only(lib, columns):
    P, W, H, V, R = 500000, 256, 256, 64, 64 * 500000
    n = int(lib.fr_fisher_point_workspace_bytes(P, W, H, V, R, columns))
    base = int(lib.fr_fisher_workspace_bytes(P, W, H, V, R, columns))
    off = (ctypes.c_size_t * 9)()
    assert lib.fr_fisher_point_workspace_layout(P, W, H, V, R, columns, off) == 0
    o = [int(x) for x in off]
    ref = (ctypes.c_size_t * 8)()
    assert lib.fr_fisher_workspace_layout(P, W, H, V, R, columns, ref) == 0
    assert o[:8] == [int(x) for x in ref] and all(x % 256 == 0 for x in o)
    # [8]: one float per (view, slot), PV >= P slots per view, behind every section of the scorer's workspace and inside this one
    assert o[8] == base and n >= o[8] + V * P * 4 and n - o[8] <= V * (P + 256 * 32) * 4 + 256
    assert int(lib.fr_fisher_point_workspace_bytes(10, 0, 256, 1, 1, 4)) == 0
    assert int(lib.fr_fisher_point_workspace_bytes(10, 16, 16, 0, 1, 4)) == 0
    assert int(lib.fr_fisher_point_workspace_bytes(10, 16, 16, 1, 1, 5)) == 0
    assert int(lib.fr_fisher_point_workspace_bytes(10, 16 * 65, 16 * 64, 1, 1, 4)) == 0       # 4160 tiles
    assert int(lib.fr_fisher_point_workspace_bytes(0, 16, 16, 1, 0, 4)) > 0
    assert lib.fr_fisher_point_workspace_layout(-1, 16, 16, 1, 1, 4, off) == 1
    assert b"fr_fisher_point_workspace_layout" in lib.fr_last_error()


def _args(W=64, H=48, P=10):
    """a well-formed call up to the pointers (host addresses that no check dereferences: every rejection below happens first)"""
    from fisher_rast._lib import RasterCfg, Gaussians, FisherCfg
    buf = ctypes.create_string_buffer(64)
    addr = ctypes.cast(buf, ctypes.c_void_p)
    cfg, g, fc = RasterCfg(), Gaussians(), FisherCfg()
    cfg.P, cfg.image_width, cfg.image_height = P, W, H
    cfg.bg = cfg.viewmatrix = cfg.projmatrix = addr
    g.means3D = g.colors_precomp = g.opacities = g.scales = g.rotations = addr
    fc.n_views, fc.columns, fc.dL_dpix, fc.w2c, fc.H_inv = 1, 4, 1e-3, addr, addr
    return cfg, g, fc, addr, buf


def _call(lib, cfg, g, fc, addr, out=True, best=True):
    return lib.fr_fisher_point_views(ctypes.byref(cfg), ctypes.byref(g), ctypes.byref(fc), addr if out else None, addr if best else None,
                                     None, 0, 0, addr, None)


def test_point_abi_accepts_a_well_formed_call_as_far_as_the_workspace(lib):
    cfg, g, fc, addr, _buf = _args()
    assert _call(lib, cfg, g, fc, addr) == 3 and b"workspace" in lib.fr_last_error()           # FR_ENOSPACE: every check passed
    assert _call(lib, cfg, g, fc, addr, out=False) == 3 and _call(lib, cfg, g, fc, addr, best=False) == 3
    fc.columns = 11
    assert _call(lib, cfg, g, fc, addr) == 3


@pytest.mark.parametrize("field", ["out_H", "dL_dpix_image", "reuse_static"])
def test_point_abi_rejects_unsupported_fields(lib, field):
    cfg, g, fc, addr, _buf = _args()
    setattr(fc, field, 1 if field == "reuse_static" else addr)
    assert _call(lib, cfg, g, fc, addr) == 1                   # FR_EINVAL, not FR_ENOSPACE: no workspace was even looked at
    msg = lib.fr_last_error().decode()
    assert "fr_fisher_point_views" in msg and field.split("_")[0] in msg


def test_point_abi_rejects_missing_weights_outputs_and_large_images(lib):
    cfg, g, fc, addr, _buf = _args()
    fc.H_inv = None
    assert _call(lib, cfg, g, fc, addr) == 1 and b"H_inv" in lib.fr_last_error()
    cfg, g, fc, addr, _buf = _args()
    assert _call(lib, cfg, g, fc, addr, out=False, best=False) == 1 and b"no output" in lib.fr_last_error()
    cfg, g, fc, addr, _buf = _args(W=16 * 65, H=16 * 64)        # 4160 tiles
    assert _call(lib, cfg, g, fc, addr) == 1 and b"4096 tiles" in lib.fr_last_error()
    cfg, g, fc, addr, _buf = _args(W=16 * 64, H=16 * 64)        # 4096 tiles: accepted as far as the workspace check
    assert _call(lib, cfg, g, fc, addr) == 3
    cfg, g, fc, addr, _buf = _args()
    fc.columns = 7
    assert _call(lib, cfg, g, fc, addr) == 1 and b"columns" in lib.fr_last_error()
    cfg, g, fc, addr, _buf = _args()
    fc.n_views = 0
    assert _call(lib, cfg, g, fc, addr) == 1
    cfg, g, fc, addr, _buf = _args()
    fc.tile_capacity = -1
    assert _call(lib, cfg, g, fc, addr) == 1
    cfg, g, fc, addr, _buf = _args()
    fc.tile_capacity = 1024                                     # 12 tiles x 1024 keys do not fit max_rendered = 0
    assert _call(lib, cfg, g, fc, addr) == 1 and b"tile_capacity" in lib.fr_last_error()
    cfg, g, fc, addr, _buf = _args()
    assert lib.fr_fisher_point_views(ctypes.byref(cfg), ctypes.byref(g), ctypes.byref(fc), addr, addr, None, 0, 0, None, None) == 1   # null status


def test_point_score_ops_install_grafts_exactly_its_surface():
    from models.SLAM.gaussian import PointScoreOps, GaussianSLAM, FisherOps
    from models.SLAM.gaussian_object import GaussianObjectSLAM, ObjectFisherOps

    class Target:
        pass
    before = set(vars(Target))
    assert PointScoreOps.install(Target) is Target
    assert set(vars(Target)) - before == {"pose_eval_points"}
    assert Target.pose_eval_points is PointScoreOps.pose_eval_points
    assert GaussianSLAM.pose_eval_points is PointScoreOps.pose_eval_points and GaussianObjectSLAM.pose_eval_points is PointScoreOps.pose_eval_points
    assert GaussianSLAM.FISHER_COLUMNS == 4 and GaussianObjectSLAM.FISHER_COLUMNS == 11
    assert GaussianSLAM.pose_eval is FisherOps.pose_eval                      # pose_eval itself is untouched

    # the tuples of FisherOps.install / ObjectFisherOps.install (which the signature test enumerates) do not carry the new name
    def grafted(cls):
        src = open(os.path.join(ROOT, "fisher-nerf-customized_amd", *cls.__module__.split(".")) + ".py").read()
        node = next(n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.ClassDef) and n.name == cls.__name__)
        inst = next(n for n in node.body if isinstance(n, ast.FunctionDef) and n.name == "install")
        return [e.value for f in ast.walk(inst) if isinstance(f, ast.For) and isinstance(f.iter, ast.Tuple) for e in f.iter.elts
                if isinstance(e, ast.Constant)]
    assert grafted(PointScoreOps) == ["pose_eval_points"]
    for cls in (FisherOps, ObjectFisherOps):
        assert "pose_eval_points" not in grafted(cls)


def test_sharded_point_score_max_keeps_its_default_route():
    import inspect
    from fisher_rast import distributed as D
    sig = inspect.signature(D.sharded_point_score_max)
    assert sig.parameters["fused"].default is False and list(sig.parameters)[:5] == ["scorer", "w2c_all", "H_inv", "group", "chunk"]


def test_polynomial_pair_factor_per_splat_on_border(oracle, harness):
    """tests/test_arbiter_cpu.py::test_scorer_record_is_as_well_conditioned_as_the_reference_chain, splat by splat: a view's score
    averages the record's error over thousands of splats, a per-Gaussian score does not.  The pair factor F = sum_c H_inv[c] leaf_c^2 /
    w^2 of the score record (fr_scorer_poly_g, evaluated as the walk does) against the exact value (arbiter build of the reference's
    per-pair chain), weighted by G^2 over three rings of the footprint, for every sampled visible splat of `border` (view 2, random
    11-column weights): no splat may exceed the entry rule 1e-4 + K_DEV e_ref, e_ref = what the reference's own binary32 chain loses on
    that splat."""
    cf, cd = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_double)
    pf = lambda x: x.ctypes.data_as(cf)
    pd = lambda x: x.ctypes.data_as(cd)
    L32, L64 = oracle.lib(), oracle.lib64()
    W, H, sc, w2c = border_scene()
    cam = oracle.setup_camera(W, H, intrinsics(W, H), np.eye(4))
    w2cs = _views(w2c, 3)
    pts = oracle.transform_points(w2cs[2], sc["means3D"])
    kw = dict(colors_precomp=sc["colors"], scales=sc["scales"], rotations=sc["rotations"])
    fwd = oracle.rasterize_forward(cam, pts, sc["opacities"], **kw)
    fwd64 = oracle.rasterize_forward(cam, oracle.transform_points(w2cs[2], sc["means3D"], arbiter=True), sc["opacities"], decisions=fwd, **kw)
    rng = np.random.default_rng(0)
    hv = rng.uniform(0.5, 10, 11).astype(np.float32)
    view = np.ascontiguousarray(cam.viewmatrix, np.float32); proj = np.ascontiguousarray(cam.projmatrix, np.float32)
    view64, proj64 = view.astype(np.float64), proj.astype(np.float64)
    powers = np.repeat([0.5, 2.0, 4.0], 16)
    G2 = np.exp(-2 * powers)
    rows = []
    for i in np.nonzero(fwd["radii"] > 0)[0][::3]:
        con = np.ascontiguousarray(fwd64["conic_opacity"][i])
        ev, evec = np.linalg.eigh(np.array([[con[0], con[1]], [con[1], con[2]]]))
        if ev.min() <= 0:
            continue
        th = np.tile(np.linspace(0, 2 * np.pi, 16, endpoint=False), 3)
        d = (evec @ (np.sqrt(2 * powers) * np.stack([np.cos(th), np.sin(th)]) / np.sqrt(ev)[:, None])).T
        n = len(d)
        dx, dy = np.ascontiguousarray(d[:, 0], np.float32), np.ascontiguousarray(d[:, 1], np.float32)
        og, od, c3 = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(3, np.float32)
        mean, cov = np.ascontiguousarray(pts[i], np.float32), np.ascontiguousarray(fwd["cov3D"][i], np.float32)
        s, r = np.ascontiguousarray(sc["scales"][i], np.float32), np.ascontiguousarray(sc["rotations"][i], np.float32)
        harness.h_scorer_pair_factor(ctypes.c_int(11), pf(mean), pf(cov), pf(s), ctypes.c_float(1.0), pf(r), pf(view), pf(proj),
                                     ctypes.c_int(W), ctypes.c_int(H), ctypes.c_float(cam.tanfovx), ctypes.c_float(cam.tanfovy),
                                     pf(hv), ctypes.c_float(sc["opacities"][i]), ctypes.c_int(n), pf(dx), pf(dy), pf(og), pf(od), pf(c3))
        F64, F32 = np.zeros(n), np.zeros(n)
        m64, cov64 = np.ascontiguousarray(fwd64["inputs"]["means3D"][i]), np.ascontiguousarray(fwd64["cov3D"][i])
        s64, r64 = s.astype(np.float64), r.astype(np.float64)
        co32 = np.ascontiguousarray(fwd["conic_opacity"][i], np.float32)
        out, outf = np.zeros(11), np.zeros(11, np.float32)
        for k in range(n):
            L64.orc_pair_leaves(pd(m64), pd(cov64), pd(s64), ctypes.c_double(1.0), pd(r64), pd(view64), pd(proj64), ctypes.c_int(W), ctypes.c_int(H),
                                ctypes.c_double(cam.tanfovx), ctypes.c_double(cam.tanfovy), pd(con), ctypes.c_double(float(dx[k])),
                                ctypes.c_double(float(dy[k])), ctypes.c_double(1.0), pd(out))
            F64[k] = (hv.astype(np.float64) * out ** 2).sum()
            L32.orc_pair_leaves(pf(mean), pf(cov), pf(s), ctypes.c_float(1.0), pf(r), pf(view), pf(proj), ctypes.c_int(W), ctypes.c_int(H),
                                ctypes.c_float(cam.tanfovx), ctypes.c_float(cam.tanfovy), pf(co32), ctypes.c_float(float(dx[k])),
                                ctypes.c_float(float(dy[k])), ctypes.c_float(1.0), pf(outf))
            F32[k] = (hv.astype(np.float64) * outf.astype(np.float64) ** 2).sum()
        den = (G2 * F64).sum()
        rows.append((den, abs((G2 * (og - F64)).sum()), abs((G2 * (F32 - F64)).sum())))
    rows = np.array(rows)
    assert len(rows) > 400
    e_poly, e_ref = rows[:, 1] / rows[:, 0], rows[:, 2] / rows[:, 0]
    over = e_poly > 1e-4
    k_needed = float(((e_poly[over] - 1e-4) / np.maximum(e_ref[over], 1e-300)).max()) if over.any() else 0.0
    print(f"[border, view 2, {len(rows)} splats] polynomial pair factor: worst {e_poly.max():.2e}, reference chain: worst {e_ref.max():.2e}, "
          f"splats above 1e-4: {int(over.sum())} / {int((e_ref > 1e-4).sum())}, K needed {k_needed:.2f} of K_DEV {K_DEV[11]}")
    assert (e_poly <= 1e-4 + K_DEV[11] * e_ref).all(), (float(e_poly.max()), k_needed)
