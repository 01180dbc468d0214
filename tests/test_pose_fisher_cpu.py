"""CPU: the camera-pose Fisher entry point (fr_fisher_pose_views) is declared, exported and bound; its workspace queries are host-only;
its argument checks reject what it does not support before any device work; and the definition the GPU tests pin -- the oracle-built
reference of tests/pose_fisher_ref.py -- is the derivative it claims to be (central differences of the arbiter's render)."""
import ctypes
import os
import re

import numpy as np
import pytest

from scenes import random_scene, intrinsics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("fr_fisher_pose_views", "fr_fisher_pose_workspace_bytes", "fr_fisher_pose_workspace_layout")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from fisher_rast import _lib
    return _lib.load()


def test_pose_symbols_declared_and_exported(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fisher_rast.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(fr_[a-z0-9_]+)\s*\(", hdr))
    from fisher_rast import _lib
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.fr_fisher_pose_views.restype is ctypes.c_int and len(lib.fr_fisher_pose_views.argtypes) == 9
    assert lib.fr_version() == 100


def test_pose_workspace_queries_are_host_only(lib):
    P, W, H, V, R = 500000, 256, 256, 64, 64 * 500000
    n = int(lib.fr_fisher_pose_workspace_bytes(P, W, H, V, R))
    base = int(lib.fr_fisher_workspace_bytes(P, W, H, V, R, 4))
    assert n >= base + V * 256 * 21 * 8
    off = (ctypes.c_size_t * 9)()
    assert lib.fr_fisher_pose_workspace_layout(P, W, H, V, R, off) == 0
    o = [int(x) for x in off]
    ref = (ctypes.c_size_t * 8)()
    assert lib.fr_fisher_workspace_layout(P, W, H, V, R, 4, ref) == 0
    assert o[:8] == [int(x) for x in ref] and o[8] == base and all(x % 256 == 0 for x in o)
    assert int(lib.fr_fisher_pose_workspace_bytes(10, 0, 256, 1, 1)) == 0
    assert int(lib.fr_fisher_pose_workspace_bytes(10, 16, 16, 0, 1)) == 0
    assert lib.fr_fisher_pose_workspace_layout(-1, 16, 16, 1, 1, off) == 1
    assert b"fr_fisher_pose_workspace_layout" in lib.fr_last_error()


def _args(W=64, H=48, P=10):
    """a well-formed call up to the pointers (host addresses that no check dereferences: every rejection below happens first)"""
    from fisher_rast._lib import RasterCfg, Gaussians, FisherCfg
    buf = ctypes.create_string_buffer(64)
    addr = ctypes.cast(buf, ctypes.c_void_p)
    cfg, g, fc = RasterCfg(), Gaussians(), FisherCfg()
    cfg.P, cfg.image_width, cfg.image_height = P, W, H
    cfg.bg = cfg.viewmatrix = cfg.projmatrix = addr
    g.means3D = g.colors_precomp = g.opacities = g.scales = g.rotations = addr
    fc.n_views, fc.columns, fc.dL_dpix, fc.w2c = 1, 4, 1e-3, addr
    return cfg, g, fc, addr, buf


def _call(lib, cfg, g, fc, addr):
    return lib.fr_fisher_pose_views(ctypes.byref(cfg), ctypes.byref(g), ctypes.byref(fc), addr, None, 0, 0, addr, None)


@pytest.mark.parametrize("field", ["H_inv", "out_H", "dL_dpix_image", "reuse_static"])
def test_pose_abi_rejects_unsupported_fields(lib, field):
    cfg, g, fc, addr, _buf = _args()
    setattr(fc, field, 1 if field == "reuse_static" else addr)
    assert _call(lib, cfg, g, fc, addr) == 1                   # FR_EINVAL, not FR_ENOSPACE: no workspace was even looked at
    msg = lib.fr_last_error().decode()
    assert "fr_fisher_pose_views" in msg and field.split("_")[0] in msg


def test_pose_abi_rejects_large_images_and_bad_arguments(lib):
    cfg, g, fc, addr, _buf = _args(W=16 * 65, H=16 * 64)        # 4160 tiles
    assert _call(lib, cfg, g, fc, addr) == 1 and b"4096 tiles" in lib.fr_last_error()
    cfg, g, fc, addr, _buf = _args(W=16 * 64, H=16 * 64)        # 4096 tiles: accepted as far as the workspace check
    assert _call(lib, cfg, g, fc, addr) == 3 and b"workspace" in lib.fr_last_error()
    cfg, g, fc, addr, _buf = _args()
    assert lib.fr_fisher_pose_views(ctypes.byref(cfg), ctypes.byref(g), ctypes.byref(fc), None, None, 0, 0, addr, None) == 1
    fc.n_views = 0
    assert _call(lib, cfg, g, fc, addr) == 1
    cfg, g, fc, addr, _buf = _args()
    fc.tile_capacity = -1
    assert _call(lib, cfg, g, fc, addr) == 1
    cfg, g, fc, addr, _buf = _args()
    g.scales = g.rotations = None
    g.cov3D_precomp = addr
    assert _call(lib, cfg, g, fc, addr) == 1 and b"scales" in lib.fr_last_error()


def test_reference_pose_hessian_is_the_pose_derivative(oracle):
    """The reference (one-hot backward -> g_{p,i} -> j_p) against central differences of the arbiter's rendered sum_ch dL C under
    exp(+-eps xi_k) on the camera-frame means, decisions held fixed; a non-zero background, so the T_final bg term is in it."""
    import pose_fisher_ref as pf
    W, H = 32, 24
    sc = random_scene(60, 5, scale=0.08)
    cam = oracle.setup_camera(W, H, intrinsics(W, H), np.eye(4))._replace(bg=np.array([0.2, 0.5, 0.1], np.float32))
    for w2c in (np.eye(4, dtype=np.float32), np.array([[0.995, 0, 0.0998, 0.05], [0, 1, 0, -0.02], [-0.0998, 0, 0.995, 0.1], [0, 0, 0, 1]], np.float32)):
        H64, JJ, jp = pf.pose_hessian_ref(cam, w2c, sc)
        jf = pf.finite_difference_j(cam, w2c, sc)
        Hf = jf.reshape(-1, 6).T @ jf.reshape(-1, 6)
        assert np.abs(jp).max() > 0
        assert np.abs(jp - jf).max() <= 1e-6 * np.abs(jf).max(), np.abs(jp - jf).max()
        assert np.abs(H64 - Hf).max() <= 1e-6 * np.abs(Hf).max()
        assert np.allclose(H64, H64.T, rtol=0, atol=1e-12 * np.abs(H64).max())
        assert np.linalg.eigvalsh(H64).min() > 0                 # six independent directions on this scene
        assert (JJ >= np.abs(H64) * (1 - 1e-12)).all()          # |sum_p j_a j_b| <= sum_p J+_a J+_b


def test_pose_log_det_convention():
    import torch
    from fisher_rast.path_eval import pose_log_det
    A = torch.eye(6).repeat(3, 1, 1) * 2.0
    A[1, 0, 0] = 0.0
    A[2, 0, 0] = -1.0
    got = pose_log_det(A)
    assert np.isclose(got[0], 6 * np.log(2.0)) and got[1] == -np.inf and got[2] == -np.inf
    assert np.isclose(pose_log_det(A, 1.0)[1], np.log(1.0) + 5 * np.log(3.0))
