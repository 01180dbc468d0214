"""CPU-only: the C-ABI library loads and exports every symbol include/fisher_rast.h declares (no compute calls without
a GPU), host-side argument validation, the drop-in module's error behaviour, the synthetic generators."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from fisher_rast import _lib
    return _lib.load()


def test_header_symbols_exported(lib):
    declared = set()
    for h in ("fisher_rast.h", "fisher_occ.h"):
        hdr = open(os.path.join(ROOT, "include", h)).read()
        hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
        declared |= set(re.findall(r"\b(fr_[a-z0-9_]+)\s*\(", hdr))
    assert {"fr_occ_update", "fr_occ_freespace", "fr_occ_frontiers", "fr_occ_erode", "fr_occ_cells_of", "fr_occ_workspace_bytes"} <= declared
    assert {"fr_forward", "fr_backward", "fr_fisher_views", "fr_mark_visible", "fr_knn_dist2", "fr_version",
            "fr_last_error", "fr_workspace_bytes", "fr_workspace_layout", "fr_fisher_workspace_bytes",
            "fr_knn_workspace_bytes"} <= declared
    for name in declared:
        assert hasattr(lib, name), name
    from fisher_rast import _lib
    assert set(_lib.EXPORTS) == declared
    assert lib.fr_version() == 100


def test_workspace_queries_are_host_only(lib):
    out = (ctypes.c_size_t * 3)()
    assert lib.fr_workspace_bytes(500000, 256, 256, 1 << 20, out) == 0
    geom, binning, img = int(out[0]), int(out[1]), int(out[2])
    assert geom >= 500000 * (32 + 24 + 12 + 3) and binning >= (1 << 20) * 8 and img >= 256 * 256 * 8
    off = (ctypes.c_size_t * 11)()
    assert lib.fr_workspace_layout(1000, 64, 48, 10, off) == 0
    o = [int(x) for x in off]
    assert o[0] == 0 and all(x % 256 == 0 for x in o) and o[1] > o[0] and o[8] > o[7] and o[10] == 0
    assert lib.fr_workspace_bytes(-1, 256, 256, 0, out) == 1          # FR_EINVAL
    assert b"bad argument" in lib.fr_last_error()
    n = int(lib.fr_fisher_workspace_bytes(500000, 256, 256, 64, 64 * 500000, 4))
    assert n >= 64 * 500000 * (4 + 32) + 64 * 500000 * 8
    assert int(lib.fr_fisher_workspace_bytes(500000, 256, 256, 64, 64 * 500000, 11)) > n
    assert int(lib.fr_fisher_workspace_bytes(10, 0, 256, 1, 1, 4)) == 0 and int(lib.fr_fisher_workspace_bytes(10, 16, 16, 1, 1, 5)) == 0
    assert int(lib.fr_knn_workspace_bytes(1000)) >= 1000 * 20


def test_occupancy_queries_and_validation_without_gpu(lib):
    from fisher_rast._lib import OccCfg
    cfg = OccCfg(768, 768, 0.05, 0.0, 0.0, -0.6, 0.6, 10.0)
    n = int(lib.fr_occ_workspace_bytes(ctypes.byref(cfg)))
    assert n >= 768 * 768 * (8 + 1 + 1 + 1 + 1 + 4 + 4 + 8)
    bad = OccCfg(768, -1, 0.05, 0.0, 0.0, -0.6, 0.6, 10.0)
    assert int(lib.fr_occ_workspace_bytes(ctypes.byref(bad))) == 0
    assert lib.fr_occ_update(ctypes.byref(cfg), None, 64, 64, 1, None, None, None, 11, 0, 0, None, None, 0, None) == 1
    assert b"fr_occ_update" in lib.fr_last_error()
    assert lib.fr_occ_freespace(ctypes.byref(cfg), 8, None, 0, 8, None, 0, None) == 3            # FR_ENOSPACE
    assert lib.fr_occ_frontiers(ctypes.byref(cfg), 8, 8, 0, 0, 7, 10, 8, 8, 8, 0, 8, None, 0, None) == 1
    assert lib.fr_occ_cells_of(ctypes.byref(cfg), None, 0, None, None) == 0                       # empty input is fine


def test_pair_entry_points_validate_without_gpu(lib):
    from fisher_rast._lib import RasterCfg, Gaussians
    cfg, g = RasterCfg(), Gaussians()
    cfg.P, cfg.image_width, cfg.image_height = 10, 32, 32
    assert lib.fr_forward_pair(ctypes.byref(cfg), ctypes.byref(g), None, None, None, 0, None, None, None, None, None, None, None) == 1
    assert b"fr_forward_pair" in lib.fr_last_error()
    assert lib.fr_forward_features(ctypes.byref(cfg), None, None, None, None, None, None) == 1
    assert b"fr_forward_features" in lib.fr_last_error()
    args = [ctypes.byref(cfg), ctypes.byref(g)] + [None] * 18
    assert lib.fr_backward_pair(*args) == 1


def test_argument_validation_without_gpu(lib):
    from fisher_rast._lib import RasterCfg, Gaussians, FisherCfg
    cfg, g, fc = RasterCfg(), Gaussians(), FisherCfg()
    cfg.P, cfg.image_width, cfg.image_height = 10, 32, 32
    rc = lib.fr_forward(ctypes.byref(cfg), ctypes.byref(g), None, None, 0, None, None, None, None, None, None)
    assert rc == 1 and b"fr_forward" in lib.fr_last_error()
    rc = lib.fr_fisher_views(ctypes.byref(cfg), ctypes.byref(g), ctypes.byref(fc), None, 0, 0, None, None)
    assert rc == 1
    rc = lib.fr_forward(None, None, None, None, 0, None, None, None, None, None, None)
    assert rc == 1 and b"null" in lib.fr_last_error()
    assert lib.fr_knn_dist2(-5, None, None, None, 0, None) == 1


BATCHED = {   # entry point -> (output pointers between the fisher cfg and the workspace, fr_fisher_cfg fields it needs besides w2c)
    "fr_fisher_views": (0, ("H_inv", "out_scores")),
    "fr_fisher_pose_views": (1, ()),
    "fr_render_views": (4, ()),
    "fr_fisher_point_views": (2, ("H_inv",)),
}


@pytest.mark.parametrize("name", sorted(BATCHED))
def test_batched_entry_points_share_their_argument_checks(lib, name):
    """The checks the four view-batched entry points share, each under the caller's own name and before any device work: host
    addresses that nothing dereferences stand in for device memory.  Where fr_fisher_views differs, the difference is recorded."""
    from fisher_rast._lib import RasterCfg, Gaussians, FisherCfg
    n_out, needs = BATCHED[name]
    buf = ctypes.create_string_buffer(64)
    addr = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL, ENOSPACE, ROOMY = 1, 3, 1 << 40
    views = name == "fr_fisher_views"

    def call(edit=None, fc_null=False, status=addr, ws=None, ws_bytes=0, max_rendered=0):
        cfg, g, fc = RasterCfg(), Gaussians(), FisherCfg()
        cfg.P, cfg.image_width, cfg.image_height = 10, 64, 48                      # 12 tiles
        cfg.bg = cfg.viewmatrix = cfg.projmatrix = addr
        g.means3D = g.colors_precomp = g.opacities = g.scales = g.rotations = addr
        fc.n_views, fc.columns, fc.dL_dpix, fc.w2c = 1, 4, 1e-3, addr
        for f in needs:
            setattr(fc, f, addr)
        if edit:
            edit(fc)
        rc = getattr(lib, name)(ctypes.byref(cfg), ctypes.byref(g), None if fc_null else ctypes.byref(fc), *([addr] * n_out),
                                ws, ws_bytes, max_rendered, status, None)
        return rc, lib.fr_last_error()

    def rejected(**kw):
        rc, msg = call(**kw)
        assert rc == EINVAL and msg.startswith(name.encode() + b":"), (kw, rc, msg)
        return msg

    rejected(fc_null=True)
    rejected(edit=lambda fc: setattr(fc, "n_views", 0))
    rejected(edit=lambda fc: setattr(fc, "w2c", None))
    rejected(status=None)
    # (a workspace that would do: fr_fisher_views looks at tile_capacity behind its workspace check, the others before it)
    assert b"tile_capacity" in rejected(edit=lambda fc: setattr(fc, "tile_capacity", -1), ws=addr, ws_bytes=ROOMY)
    assert b"exceeds max_rendered" in rejected(edit=lambda fc: setattr(fc, "tile_capacity", 1024), ws=addr, ws_bytes=ROOMY, max_rendered=12 * 1024 - 1)
    rc, msg = call(edit=lambda fc: setattr(fc, "tile_capacity", 1024), max_rendered=12 * 1024)
    assert rc == ENOSPACE and msg.startswith(name.encode() + b":") and b"workspace" in msg       # well-formed, as far as the workspace
    assert call()[0] == ENOSPACE
    # fr_fisher_views as it is: tile_capacity only behind the workspace check, and no check of max_rendered of its own
    assert call(edit=lambda fc: setattr(fc, "tile_capacity", -1))[0] == (ENOSPACE if views else EINVAL)
    rc, msg = call(max_rendered=-1)
    assert rc == (ENOSPACE if views else EINVAL) and (views or b"max_rendered" in msg)


def test_chunk_and_redo_driver_host_logic():
    """FisherScorer._chunks on a stand-in scorer (no device): five views, three per launch until the buffers have grown and two from
    then on.  The overflowed chunk is redone shorter, the growth follows the status word, bit 0 of status[3] alone grows the
    segments, bit 1 raises, and no views means no launch."""
    from fisher_rast.ops import FisherScorer
    from fisher_rast._lib import FisherRastError

    def stand_in(tile_capacity):
        sc = FisherScorer.__new__(FisherScorer)
        sc.tiles, sc.tile_capacity, sc.per_view_capacity = 12, tile_capacity, 64
        sc.max_views_per_launch = lambda: 3 if sc.per_view_capacity == 64 else 2
        return sc

    for tile_capacity, st3 in ((16, 1), (0, 0)):
        sc, calls = stand_in(tile_capacity), []

        def launch(v0, v1):
            calls.append((v0, v1))
            st = [9000, 1, 700, st3] if sc.per_view_capacity == 64 else [9000, 0, 700, 0]
            return dict(status=torch.tensor(st, dtype=torch.int32), views=(v0, v1))
        assert [r["views"] for r in sc._chunks(5, launch)] == [(0, 2), (2, 4), (4, 5)]
        assert calls == [(0, 3), (0, 2), (2, 4), (4, 5)]
        assert sc.per_view_capacity == int(9000 * 1.25 / 3) + 4096 and sc.tile_capacity == (1024 if st3 else 0)
    with pytest.raises(FisherRastError, match="view_is_identity"):
        list(stand_in(16)._chunks(5, lambda v0, v1: dict(status=torch.tensor([0, 1, 0, 2], dtype=torch.int32))))
    assert list(stand_in(0)._chunks(0, None)) == []


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under the product package may reference it."""
    pkg = os.path.join(ROOT, "fisher-nerf-customized_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(d, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), (d, f)
                assert "liboracle" not in txt and "fisher_oracle" not in txt.replace("oracle/fisher_oracle.c", ""), (d, f)


def test_product_library_is_not_the_experiment_rig(lib):
    """The library build() produces reads NO environment variable (no getenv import) and holds only kernels a default call can reach:
    the A/B generations (rolling-window walk, 8 x 8 pixel blocks, the 25-leaf two-pass kernel, round 1's compositing and sort
    forms, the parking projection kernels) are retired from the source as well; what is left of the rig (csrc/fr_rig.inc: host
    switches, loop statistics, ablations) exists in -DFR_AB builds only (tools/build_variant.sh -> tools/_build/)."""
    import subprocess
    import sys
    from fisher_rast import _lib
    so = _lib.SO_PATH
    undefined = subprocess.run(["nm", "-D", "--undefined-only", so], capture_output=True, text=True, check=True).stdout
    assert "getenv" not in undefined, "the product library must not read the environment"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj
    names = set()
    for co in codeobj._code_objects(open(so, "rb").read()):
        names |= set(codeobj._functions(co))
    assert any("k_fisher_tile_v4" in n for n in names)            # the dominant kernel is there
    for banned in ("k_fisher_tile_v3w", "k_fisher_tile_v3ILi8ELi8E", "k_fisher_tile_v3ILi16ELi4ELb1E", "k_fisher_tile_v2ILi25E", "k_pack_staticILi25E", "k_render_forwardILi",
                   "k_backward_lin_tileILb0E", "k_backward_lin_walkILb1E", "k_preprocess_viewsILi4E", "k_preprocess_viewsILin4E",
                   "k_preprocess_viewsILi11E"):
        assert not any(banned in n for n in names), banned
    src = open(os.path.join(ROOT, "fisher-nerf-customized_amd", "csrc", "fisher_rast.hip")).read()
    outside = re.sub(r"#ifdef FR_AB\b.*?#e(?:ndif|lse)", "", src, flags=re.S)
    assert "getenv" not in outside and "getenv" not in open(os.path.join(ROOT, "fisher-nerf-customized_amd", "csrc", "fisher_occ.hip")).read()
    # the rig's header (always included) reads the environment inside `#ifdef FR_AB` only
    rig = open(os.path.join(ROOT, "fisher-nerf-customized_amd", "csrc", "fr_rig.inc")).read()
    assert "getenv" in rig and "getenv" not in re.sub(r"#ifdef FR_AB\b.*?#e(?:ndif|lse)", "", rig, flags=re.S)
    # the kernels carry single-line hooks of the rig, never a preprocessor block of it ...
    assert not re.search(r"#\s*(?:ifdef|ifndef|if\s+defined|if\s+!\s*defined|elif)\b[^\n]*\bFR_(?:LOOPSTATS|ABLATE|FWD_STATS)\b", src)
    # ... and the generations that only a rig switch selected are gone from the source, not just from the binary
    for retired in (r"k_fisher_tile_v3w", r"k_fisher_tile_v3<\s*8", r"k_fisher_tile_v3<\s*16,\s*4,\s*true", r"k_fisher_tile_v2<\s*25", r"k_pack_static<\s*25",
                    r"k_render_forward\b(?!_walk)", r"k_backward_lin_tile<\s*false", r"k_backward_lin_walk<\s*true", r"k_preprocess_views<\s*-?(?:4|11|RC)\b",
                    r"legacy_sort"):
        assert not re.search(retired, src), retired
    for py in ("ops.py", "_lib.py", "distributed.py", "path_eval.py"):
        txt = open(os.path.join(ROOT, "fisher-nerf-customized_amd", "fisher_rast", py)).read()
        for var in ("FR_DEBUG_MODE", "FR_STREAMS", "FR_TILE_CAPACITY", "FR_GROUPS", "FR_GV", "FR_VC"):
            assert var not in txt, (py, var)


def test_missing_library_fails_loudly(monkeypatch, lib):
    from fisher_rast import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "SO_PATH", "/nonexistent/libfisher_rast.so")
    with pytest.raises(_lib.FisherRastError, match="no CPU fallback"):
        _lib.load()


def test_rasterizer_front_end_errors():
    """GaussianRasterizer.forward argument rules (reference __init__.py:174-178) fire before any device work."""
    from diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizationSettings
    rs = GaussianRasterizationSettings(32, 32, 1.0, 1.0, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False)
    assert rs._fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix",
                          "projmatrix", "sh_degree", "campos", "prefiltered")
    r = GaussianRasterizer(rs, backward_power=2)
    assert r.backward_power == 2 and GaussianRasterizer(rs).backward_power == 1
    m = torch.zeros((5, 3))
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(means3D=m, means2D=m, opacities=m[:, :1], scales=m, rotations=torch.zeros((5, 4)))
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(means3D=m, means2D=m, opacities=m[:, :1], shs=torch.zeros((5, 1, 3)), colors_precomp=m, scales=m, rotations=torch.zeros((5, 4)))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=m, means2D=m, opacities=m[:, :1], colors_precomp=m, scales=m)
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=m, means2D=m, opacities=m[:, :1], colors_precomp=m, scales=m, rotations=torch.zeros((5, 4)), cov3D_precomp=torch.zeros((5, 6)))
    # CPU tensors reach the op layer, which refuses: there is no CPU path
    from fisher_rast import FisherRastError
    with pytest.raises(FisherRastError, match="no CPU path"):
        r(means3D=m, means2D=m, opacities=m[:, :1], colors_precomp=m, scales=m, rotations=torch.zeros((5, 4)))


def test_synthetic_generators_are_seeded():
    from fisher_rast import synthetic
    a, b = synthetic.room_shell(2000, 7), synthetic.room_shell(2000, 7)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert set(a) == {"means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales"}
    assert a["means3D"].shape == (2000, 3) and a["log_scales"].shape == (2000, 3)
    s = torch.exp(a["log_scales"])
    assert float(s.min()) >= 0.001 and float(s.max()) <= 0.1 * 1.6
    m = a["means3D"]
    assert float(m[:, 0].abs().max()) <= 5.1 and float(m[:, 1].abs().max()) <= 1.35
    on_face = ((m.abs() - torch.tensor([5.0, 1.25, 5.0])).abs() < 0.06).any(1).float().mean()
    assert 0.8 < float(on_face) < 0.95
    c2w = synthetic.candidate_poses(16, 3)
    R = c2w[:, :3, :3]
    assert torch.allclose(R @ R.transpose(1, 2), torch.eye(3).expand(16, 3, 3), atol=1e-6)
    assert torch.allclose(torch.linalg.det(R), torch.ones(16), atol=1e-6)      # two negated columns keep det = +1
    assert float(c2w[:, 1, 3].abs().max()) == 0.0
    w2c = synthetic.invert_rigid(c2w)
    assert torch.allclose(w2c @ c2w, torch.eye(4).expand(16, 4, 4), atol=1e-5)
    act = synthetic.activate(a)
    assert torch.allclose(act["rotations"].norm(dim=1), torch.ones(2000), atol=1e-6)


def test_setup_camera_matches_oracle_restatement(oracle):
    from models.SLAM.utils.recon_helpers import setup_camera
    from fisher_rast import synthetic
    w2c = np.eye(4, dtype=np.float32)
    w2c[:3, 3] = [0.3, -0.2, 1.0]
    K = synthetic.intrinsics(256, 256)
    cam = setup_camera(256, 256, K, w2c, device="cpu")
    o = oracle.setup_camera(256, 256, K, w2c)
    assert cam.viewmatrix.shape == (1, 4, 4) and cam.projmatrix.shape == (1, 4, 4)
    assert np.allclose(cam.viewmatrix.reshape(-1).numpy(), o.viewmatrix) and np.allclose(cam.projmatrix.reshape(-1).numpy(), o.projmatrix, atol=1e-6)
    assert cam.tanfovx == 1.0 and cam.sh_degree == 0 and not cam.prefiltered
    # identity camera at 256x256: p_hom.w = z and pixel = 128 x/z + 127.5
    pm = setup_camera(256, 256, K, np.eye(4), device="cpu").projmatrix.reshape(-1).numpy()
    assert np.allclose(pm[[0, 5, 11]], [1, 1, 1]) and np.allclose(pm[[3, 7, 15]], [0, 0, 0])


def test_install_grafts_methods_onto_reference_like_classes():
    """INTEGRATION.md sections 4 / 4b: `install` puts the accelerated methods on classes that merely look like the reference's."""
    from models.SLAM.gaussian import FisherOps
    from models.SLAM.gaussian_object import ObjectFisherOps
    from planning.astar import OccupancyOps

    class RefSLAM:
        pass

    class RefObjectSLAM:
        def topt_score_from_diags(self, *a, **k):
            return 1

    class RefPlanner:
        pass

    FisherOps.install(RefSLAM)
    assert RefSLAM.FISHER_COLUMNS == 4 and all(callable(getattr(RefSLAM, n)) for n in ("compute_Hessian", "compute_H_train", "pose_eval", "path_scores"))
    ObjectFisherOps.install(RefObjectSLAM)
    assert RefObjectSLAM.FISHER_COLUMNS == 11 and callable(RefObjectSLAM._flat_diag)
    assert all(callable(getattr(RefObjectSLAM, n)) for n in ("pose_eval", "estimate_diag_JtJ_simple", "estimate_block_JtJ", "pose_eval_popgs", "pose_eval_popgs_blocks"))
    assert RefObjectSLAM().topt_score_from_diags() == 1                       # the reference's own helpers are left alone
    OccupancyOps.install(RefPlanner)
    assert all(callable(getattr(RefPlanner, n)) for n in ("update_occ_map", "build_connected_freespace", "build_frontiers", "generate_candidate",
                                                                   "generate_candidate_object", "generate_candidate_in_freespace", "sample_random_candidate"))


def test_get_loss_graft_is_opt_in_and_the_pixel_mask_follows_the_reference_rule():
    """`install` leaves the module-level get_loss of the module it patches alone unless asked (patch_get_loss=True); the loss
    mask (`_loss_pixel_mask`) equals the rule of the reference's get_loss (gaussian.py:212-233), restated here step by step."""
    import types
    import sys
    from models.SLAM import gaussian as G
    mod = types.ModuleType("fake_ref_gaussian")
    mod.get_loss = lambda *a, **k: "reference"
    mod.transform_to_frame = lambda *a, **k: None
    mod.calc_loss = lambda *a, **k: {}
    sys.modules[mod.__name__] = mod
    try:
        cls = type("RefSLAM", (), {"__module__": mod.__name__})
        G.FisherOps.install(cls)
        assert mod.get_loss() == "reference"
        G.FisherOps.install(cls, patch_get_loss=True)
        assert mod.get_loss.__name__ == "get_loss" and mod.get_loss.__module__ == G.__name__
    finally:
        del sys.modules[mod.__name__]
    g = torch.Generator().manual_seed(4)
    Hh, Ww = 24, 32
    gt = torch.rand((1, Hh, Ww), generator=g) * 4
    gt[0, :3] = 0                                              # unmeasured rows
    ds = torch.rand((3, Hh, Ww), generator=g) * 4
    ds[0] = gt[0] + 0.05 * torch.randn((Hh, Ww), generator=g)
    ds[0, 10, 10] += 9.0                                       # an outlier
    ds[0, 5, 5] = float("nan")
    ds[2, 6, 6] = float("nan")
    for outl in (False, True):
        for pres in (False, True):
            depth, mask = G._loss_pixel_mask(ds, gt, 0.5, outl, pres)
            d = ds[0].unsqueeze(0)
            unc = ds[2].unsqueeze(0) - d ** 2
            nanm = (~torch.isnan(d)) & (~torch.isnan(unc))
            if outl:
                err = torch.abs(gt - d) * (gt > 0)
                m = (err < 10 * err.median()) & (gt > 0)
            else:
                m = gt > 0
            m = m & nanm
            if pres:
                m = m & (ds[1] > 0.5)
            assert mask.shape == (1, Hh, Ww) and mask.dtype == torch.bool and torch.equal(mask, m)
            assert torch.equal(torch.nan_to_num(depth), torch.nan_to_num(d))
            assert not bool(mask[0, 5, 5]) and not bool(mask[0, 6, 6]) and not bool(mask[0, 0, 0])
            assert bool(mask[0, 10, 10]) == (not outl and (not pres or bool(ds[1, 10, 10] > 0.5)))
