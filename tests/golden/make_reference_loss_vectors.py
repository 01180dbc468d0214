#!/usr/bin/env python3
"""Golden vectors produced by RUNNING the reference's loss functions on the CPU (imported from the reference tree in the build
container only): `gaussian`, `calc_ssim`, `calc_ssim_masked` (models/SLAM/utils/slam_external.py:77-193) and `calc_loss`,
`calc_loss_mask` (models/SLAM/utils/slam_helpers.py:23-77), which import with numpy + torch alone -- in binary32 AND in binary64
(the same functions on double tensors), with their autograd gradients w.r.t. the render.  Inputs and outputs only; no reference
source is copied.  The inputs are not stored: tests/loss_cases.py regenerates them from seeds.  Run from the repo root:
    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<reference tree> python tests/golden/make_reference_loss_vectors.py

reference_loss.npz holds
    taps_bits  uint32 [11]    gaussian(11, 1.5) in binary32
    keys       str [N]        "<C>x<H>x<W>/<family>/<mask kind>/<term>" (loss_cases.key)
    values     float64 [N,3]  the term in binary32, in binary64, and max |gradient32 - gradient64|
    grad64     float32        the binary64 gradients rounded to binary32, one after the other (offsets [N + 1])
To stay under 200 KB the gradient of the two SSIM-only terms (calc_ssim, calc_ssim_masked) is kept for the two smaller colour
shapes only; at 3x17x33 those terms keep their values and their binary32 deviation, the tests take the binary64 gradient from
loss_cases.loss64 (which the kept gradients pin to 1e-12), and the same kernels' gradient is in the fixture through map_im / mapmask_im.
"""
import os
import sys

import numpy as np
import torch

from models.SLAM.utils.slam_external import calc_ssim, calc_ssim_masked, gaussian      # reference
from models.SLAM.utils.slam_helpers import calc_loss, calc_loss_mask                   # reference

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import loss_cases as lc                                                                # noqa: E402


def run_term(name, x, y, m1, mc, dtype):
    """(value, gradient w.r.t. the render) of one term from the reference's own functions"""
    xr = torch.tensor(x, dtype=dtype, requires_grad=True)
    yt = torch.tensor(y, dtype=dtype)
    m1t, mct = torch.tensor(m1), torch.tensor(mc)
    C, H, W = x.shape
    dummy3, dummy1 = torch.zeros((3, H, W), dtype=dtype), torch.zeros((1, H, W), dtype=dtype)
    if name == "ssim":
        v = calc_ssim(xr, yt)
    elif name == "ssim_masked":
        v = calc_ssim_masked(xr, yt, m1t)
    elif name == "map_im":
        v = calc_loss(dict(im=yt, depth=dummy1), xr, dummy1, m1t, mct, False, False, False, False)["im"]
    elif name == "trk_im":
        v = calc_loss(dict(im=yt, depth=dummy1), xr, dummy1, m1t, mct, False, False, False, True)["im"]
    elif name == "trk_im_masked":
        v = calc_loss(dict(im=yt, depth=dummy1), xr, dummy1, m1t, mct, False, True, False, True)["im"]
    elif name == "mapmask_im":
        v = calc_loss_mask(dict(im=yt, depth=dummy1), xr, dummy1, m1t, mct, False, False, False, False)["im"]
    elif name == "map_depth":
        v = calc_loss(dict(im=dummy3, depth=yt), dummy3, xr, m1t, m1t.repeat(3, 1, 1), True, False, False, False)["depth"]
    elif name == "trk_depth":
        v = calc_loss(dict(im=dummy3, depth=yt), dummy3, xr, m1t, m1t.repeat(3, 1, 1), True, False, False, True)["depth"]
    else:
        raise ValueError(name)
    g, = torch.autograd.grad(v, xr, allow_unused=True)
    g = torch.zeros_like(xr) if g is None else g
    return float(v.detach()), g.detach().numpy()


taps = gaussian(11, 1.5).numpy()
assert taps.dtype == np.float32
keys, values, grads, offsets = [], [], [], [0]
for shape, family, kind in lc.all_cases():
    x, y, m1, mc = lc.make_case(shape, family, kind)
    for term in lc.terms_for(shape[0], kind):
        v32, g32 = run_term(term.name, x, y, m1, mc, torch.float32)
        v64, g64 = run_term(term.name, x, y, m1, mc, torch.float64)
        keys.append(lc.key(shape, family, kind, term.name))
        values.append([v32, v64, float(np.abs(g32.astype(np.float64) - g64).max())])
        keep = not (term.out == "ssim" and x.size > 1100)
        grads.append(g64.astype(np.float32).reshape(-1) if keep else np.zeros(0, np.float32))
        offsets.append(offsets[-1] + grads[-1].size)
out = os.path.join(HERE, "reference_loss.npz")
np.savez_compressed(out, taps_bits=taps.view(np.uint32), keys=np.array(keys), values=np.array(values, np.float64),
                    grad64=np.concatenate(grads), offsets=np.array(offsets, np.int64))
print("written", out, os.path.getsize(out), "bytes,", len(keys), "terms")
