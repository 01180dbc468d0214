#!/usr/bin/env python3
"""Golden vectors produced by RUNNING the reference's metric functions on the CPU (imported from the reference tree in the build
container only): `calc_psnr` and `calc_ssim` (models/SLAM/utils/slam_external.py:72-120), which import with numpy + torch alone --
in binary32 AND in binary64 (the same functions on double tensors).  Results only; no reference source is copied.  The inputs are
not stored: tests/eval_cases.py regenerates them from seeds.  Run from the repo root:
    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree> python tests/golden/make_reference_eval_vectors.py

The tester's `ssim` (tester_gaussians_navigation.py:1481) is `models/utils.ssim`; its body is the same statement as `calc_ssim`
(the same window, the same five convolutions, the same map), but its module imports `cv2`, which the build container does not
have, so `calc_ssim` is what is run.  What the tester does around the two functions is restated here, one torch expression each:
    color.clamp_(0, 1)                                           tester_gaussians_navigation.py:1451
    rgb_gt = rgb[:, :, :3].permute(2, 0, 1) / 255                :1454
    psnr = calc_psnr(color, rgb_gt).mean()                       :1473
    depth_mae = torch.mean(torch.abs(depth - depth_gt))          :1474
    (the keep rule `torch.isinf(psnr)` of :1484 is applied by the tests to these values)
and of report_progress (models/SLAM/utils/eval_helpers.py:236, 245-247) the masked forms
    calc_psnr(im * mask, gt * mask).mean()
    (torch.abs((depth - depth_gt) * mask) * valid).sum() / valid.sum(),  valid = depth_gt > 0
The "rmse" entries are sqrt(sum(((depth - depth_gt) * mask) ** 2 [* valid]) / count): the library's definition, not
report_progress's (which takes sqrt of each square and so repeats its L1).

reference_eval.npz holds
    keys       str [N]          "<V>x<H>x<W>/<rot>/<mask kind>/<clamp|raw>" (eval_cases.key)
    offsets    int64 [N + 1]    the views of case i are values[offsets[i]:offsets[i + 1]]
    values     float64 [.,2,6]  per view, in binary32 and in binary64: psnr, ssim, l1_all, rmse_all, l1_valid, rmse_valid
"""
import os
import sys

import numpy as np
import torch

from models.SLAM.utils.slam_external import calc_psnr, calc_ssim      # reference

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import eval_cases as ec                                                # noqa: E402


def run_view(render, gt_u8, depth, gt_depth, mask, clamp, dtype):
    color = torch.tensor(render, dtype=dtype)
    if clamp:
        color.clamp_(min=0., max=1.)
    rgb_gt = torch.tensor(gt_u8)[:, :, :3].permute(2, 0, 1) / 255
    assert rgb_gt.dtype == torch.float32
    rgb_gt = rgb_gt.to(dtype)
    d, g = torch.tensor(depth, dtype=dtype)[None], torch.tensor(gt_depth, dtype=dtype)[None]
    if mask is not None:
        m = torch.tensor(mask.astype(bool))[None]
        color, rgb_gt = color * m, rgb_gt * m
        diff = (d - g) * m
    else:
        diff = d - g
    with torch.no_grad():
        psnr = calc_psnr(color, rgb_gt).mean()
        ssim = calc_ssim(color, rgb_gt)
        valid = g > 0
        l1_all = torch.mean(torch.abs(diff))
        rmse_all = torch.sqrt(torch.mean(diff ** 2))
        l1_valid = (torch.abs(diff) * valid).sum() / valid.sum()
        rmse_valid = torch.sqrt(((diff ** 2) * valid).sum() / valid.sum())
    return [float(t) for t in (psnr, ssim, l1_all, rmse_all, l1_valid, rmse_valid)]


keys, values, offsets = [], [], [0]
for shape, rot, kind, clamp in ec.all_cases():
    b = ec.make_batch(shape, rot, kind)
    for v in range(shape[0]):
        m = None if b["mask"] is None else b["mask"][v]
        values.append([run_view(b["render"][v], b["gt_u8"][v], b["depth"][v], b["gt_depth"][v], m, clamp, dt)
                       for dt in (torch.float32, torch.float64)])
    keys.append(ec.key(shape, rot, kind, clamp))
    offsets.append(len(values))
out = os.path.join(HERE, "reference_eval.npz")
np.savez_compressed(out, keys=np.array(keys), offsets=np.array(offsets, np.int64), values=np.array(values, np.float64))
print("written", out, os.path.getsize(out), "bytes,", len(keys), "cases,", len(values), "views")
