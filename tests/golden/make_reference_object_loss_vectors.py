#!/usr/bin/env python3
"""Golden vectors produced by RUNNING the reference's object-aware training step on the CPU: `get_loss` of
models/SLAM/gaussian_object.py (188-336) and `get_gaussians_outside_mask` of models/SLAM/utils/slam_external.py (270-343), imported
from a reference checkout with stand-ins for what cannot run here -- `Tensor.cuda()` returns the tensor, a tensor asked for on
'cuda' is made on the CPU (build_rotation's hard-coded device), the modules that do not import (open3d, habitat_sim, wandb, the CUDA
rasteriser, ...) are empty stubs, and the module's `Renderer`, `transform_to_frame` and the two `transformed_params2*` names return
the case's own `im` / `depth_sil` as leaves that require a gradient, so that `loss.backward()` yields the reference's d loss / d im
and d loss / d depth_sil.  Everything between the render and the loss -- the pixel mask, the object lines, calc_loss /
calc_loss_mask with their SSIM -- is the reference's.  Outputs only; no reference source is copied.  The inputs are not stored:
tests/objloss_cases.py regenerates them from seeds.  Run from the repo root:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reference_object_loss_vectors.py <reference tree>

reference_object_loss.npz holds, for each get_loss run "loss/<case>/<tracking|mapping>" (the three cases of GOLDEN_LOSS_CASES):
    <run>/weighted      float32 [3]      the weighted losses im, depth and their sum
    <run>/mask          bool [H,W]       the pixel mask calc_loss / calc_loss_mask was handed
    <run>/d_im          float32 [3,H,W]  d loss / d im
    <run>/d_depth_sil   float32 [3,H,W]  d loss / d depth_sil
    <run>/weighted64, d_im64, d_depth_sil64   the same from a run on the same inputs in binary64 (it must select the same pixels)
and for each outside-mask case "outside/<case>" (GOLDEN_OUTSIDE_CASES):
    <case>/outside      bool [P]
    <case>/counts       int64 [3]        in_count, out_count, total
    <case>/ranges       float32 [4]      inside_scale_min / max, outside_scale_min / max
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import objloss_cases as oc                                                             # noqa: E402


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


def _on_the_cpu(fn):
    def wrapped(*a, **k):
        if str(k.get("device", "")).startswith("cuda"):
            k.pop("device")
        return fn(*a, **k)
    return wrapped


def main(ref_root):
    sys.path.insert(0, ref_root)
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.zeros, torch.eye = _on_the_cpu(torch.zeros), _on_the_cpu(torch.eye)
    ref = _import_with_stubs("models.SLAM.gaussian_object")                            # the reference's module
    ext = sys.modules["models.SLAM.utils.slam_external"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    out = {}
    for i in range(len(oc.GOLDEN_LOSS_CASES)):
        c = oc.make_golden_loss_case(i)
        for mode, dtype in ((m, d) for m in ("tracking", "mapping") for d in (torch.float32, torch.float64)):
            im, ds = t(c["im"]).to(dtype).requires_grad_(True), t(c["depth_sil"]).to(dtype).requires_grad_(True)
            P = 7
            seen = {}

            def recording(real):
                def calc(curr_data, im_, depth_, mask, color_mask, *flags):
                    seen["mask"] = mask.detach().clone()
                    return real(curr_data, im_, depth_, mask, color_mask, *flags)
                return calc

            ref.transform_to_frame = lambda *a, **k: None
            ref.transformed_params2rendervar = lambda *a, **k: dict(means2D=torch.zeros((P, 3), requires_grad=True), which="im")
            ref.transformed_params2depthplussilhouette = lambda *a, **k: dict(which="depth_sil")
            ref.Renderer = lambda raster_settings: (lambda which, **kw: (im, torch.arange(P) % 3, None) if which == "im" else (ds, None, None))
            real_calc_loss, real_calc_loss_mask = ref.calc_loss, ref.calc_loss_mask
            ref.calc_loss, ref.calc_loss_mask = recording(real_calc_loss), recording(real_calc_loss_mask)
            curr = dict(cam=None, w2c=torch.eye(4), im=t(c["gt_im"]).to(dtype), depth=t(c["gt"]).to(dtype), obj_mask_2d=t(c["obj"]).bool())
            variables = dict(max_2D_radius=torch.zeros(P))
            try:
                loss, _, weighted = ref.get_loss({}, curr, variables, 0, oc.GOLDEN_WEIGHTS, True, oc.SIL_THRES, True, c["ignore"],
                                                 tracking=mode == "tracking", mapping=mode == "mapping")
            finally:
                ref.calc_loss, ref.calc_loss_mask = real_calc_loss, real_calc_loss_mask
            loss.backward()
            run, tag = f"loss/{i}/{mode}", "" if dtype == torch.float32 else "64"
            out[f"{run}/weighted{tag}"] = np.array([float(weighted[k].detach()) for k in ("im", "depth", "loss")], np.float32 if not tag else np.float64)
            if tag:
                assert np.array_equal(out[f"{run}/mask"], seen["mask"][0].numpy().astype(bool)), "the binary64 run selects other pixels"
            out[f"{run}/mask"] = seen["mask"][0].numpy().astype(bool)
            out[f"{run}/d_im{tag}"] = im.grad.numpy()
            out[f"{run}/d_depth_sil{tag}"] = ds.grad.numpy()
            print(run, dtype, out[f"{run}/weighted{tag}"], "mask", int(out[f"{run}/mask"].sum()))
    for i in range(len(oc.GOLDEN_OUTSIDE_CASES)):
        c = oc.make_golden_outside_case(i)
        params = oc.trajectory_params(c, t=oc.GOLDEN_FRAME)
        outside, stats = ext.get_gaussians_outside_mask(params, dict(id=oc.GOLDEN_FRAME, intrinsics=t(c["K"])), t(c["obj"]).bool())
        name = f"outside/{i}"
        out[f"{name}/outside"] = outside.numpy().astype(bool)
        out[f"{name}/counts"] = np.array([stats["in_count"], stats["out_count"], stats["total"]], np.int64)
        out[f"{name}/ranges"] = np.array([stats[k] for k in ("inside_scale_min", "inside_scale_max", "outside_scale_min", "outside_scale_max")], np.float32)
        assert int(stats["idx_in"].numel()) == stats["in_count"] and int(stats["idx_out"].numel()) == stats["out_count"]
        print(name, out[f"{name}/counts"], out[f"{name}/ranges"])
    np.savez_compressed(os.path.join(HERE, "reference_object_loss.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1])
