#!/usr/bin/env python3
"""Golden vectors produced by RUNNING the reference's frame ingest on the CPU: `add_new_gaussians` down to its call of
`get_pointcloud` (models/SLAM/gaussian.py:320-355) and `get_pointcloud` itself (75-143), imported from a reference checkout with
stand-ins for what cannot run here -- `Tensor.cuda()` returns the tensor, the modules that do not import (open3d, habitat_sim,
wandb, the CUDA rasteriser, ...) are empty stubs, and the render is the case's own depth / silhouette image.  Outputs only; no
reference source is copied.  The inputs are not stored: tests/ingest_cases.py regenerates them from seeds.  Run from the repo root:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reference_ingest_vectors.py <reference tree>

reference_ingest.npz holds, for each of the three cases "<family>/<H>/<W>/<d>" listed in `cases`:
    <case>/mask            bool [H W]     the non-presence mask add_new_gaussians handed to get_pointcloud
    <case>/point_cld       float32 [N,6]  what get_pointcloud returned for it (binary32, the reference's own arithmetic)
    <case>/mean3_sq_dist   float32 [N]
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ingest_cases as ic                                                              # noqa: E402

CASES = [("half", (5, 7, 1)), ("inf", (4, 6, 2)), ("half", (48, 64, 4))]


class _Stub(types.ModuleType):
    """a module that has every attribute, each one a callable stub again"""
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return _Stub(f"{self.__name__}.{name}")

    def __call__(self, *a, **k):
        return self


def _import_with_stubs(name):
    """import `name`; every module that is missing on the way becomes a stub, one at a time"""
    import importlib
    for _ in range(100):
        try:
            return importlib.import_module(name)
        except ModuleNotFoundError as e:
            print("stub for", e.name)
            parts = e.name.split(".")
            for i in range(1, len(parts) + 1):
                sys.modules.setdefault(".".join(parts[:i]), _Stub(".".join(parts[:i])))
            for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
                del sys.modules[k]                     # a half-imported reference package would hide the retry
    raise SystemExit(f"could not import {name}")


class _Stop(Exception):
    pass


def main(ref_root):
    sys.path.insert(0, ref_root)
    torch.Tensor.cuda = lambda self, *a, **k: self
    ref = _import_with_stubs("models.SLAM.gaussian")                                   # the reference's module
    real_get_pointcloud = ref.get_pointcloud
    out = {"cases": np.array(["/".join([f] + [str(v) for v in s]) for f, s in CASES])}
    for (family, shape), name in zip(CASES, out["cases"]):
        c = ic.make_case(family, shape)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        seen = {}

        def recording_get_pointcloud(color, depth, intrinsics, w2c, **kw):
            seen["mask"] = kw["mask"].clone()
            seen["out"] = real_get_pointcloud(color, depth, intrinsics, w2c, **kw)
            raise _Stop()

        # the render and the camera are the case's; everything between them and get_pointcloud is the reference's
        ref.transform_to_frame = lambda *a, **k: None
        ref.transformed_params2depthplussilhouette = lambda *a, **k: {}
        ref.Renderer = lambda raster_settings: (lambda **kw: (t(c["depth_sil"]), None, None))
        ref.build_rotation = lambda q: t(c["w2c"][:3, :3])[None]
        ref.get_pointcloud = recording_get_pointcloud
        params = dict(cam_unnorm_rots=torch.tensor([[1.0, 0, 0, 0]])[..., None], cam_trans=t(c["w2c"][:3, 3])[None, :, None],
                      means3D=torch.zeros((1, 3)))
        curr = dict(w2c=torch.eye(4), cam=None, depth=t(c["gt"]), im=t(c["color"]), intrinsics=t(c["K"]))
        try:
            ref.add_new_gaussians(dict(isotropic=False), params, {}, curr, ic.SIL_THRES, 0, "projective",
                                  dict(depth_error_ratio=c["ratio"]), add_rand_gaussians=False, downsample_pcd=c["d"])
            raise SystemExit(f"{name}: the reference selected nothing")
        except _Stop:
            pass
        cld, msd = seen["out"]
        assert cld.dtype == torch.float32 and msd.dtype == torch.float32
        out[f"{name}/mask"] = seen["mask"].numpy().astype(bool)
        out[f"{name}/point_cld"] = cld.numpy()
        out[f"{name}/mean3_sq_dist"] = msd.numpy()
        print(name, "rows", cld.shape[0])
    np.savez_compressed(os.path.join(HERE, "reference_ingest.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
