#!/usr/bin/env python3
"""Golden vectors produced by RUNNING the reference's two nearest-point functions on the CPU: `accuracy_comp_ratio_from_pcl`
(scripts/eval_3d_reconstruction.py) and `novelty_mask_from_pcd_nn` (test_utils.py).  Their files import open3d / trimesh / cv2 and
load meshes at top level, so each function is taken out of its file by `ast` and compiled alone, with the names it uses (np, torch,
KDTree, cKDTree) supplied and an empty stand-in for `cv2`, which the path does not call.  Outputs only; no reference source is
copied.  The inputs are not stored: tests/cloud_cases.py regenerates them from seeds.  Run from the repo root:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reference_cloud_vectors.py <reference tree>

reference_cloud.npz holds
    points_cases             "<family>/<N>/<M>/<seed>"; targets are the ground truth, queries the reconstruction
    <case>/<th>/forward      float64 [3]  (acc, comp, ratio) of f(gt, rec, th)
    <case>/<th>/swapped      float64 [3]  of f(rec, gt, th), as the tester calls it the second time
    depth_cases              "<H>/<W>/<kind>/<z_forward>/<stride>/<seed>"
    <case>/mask              uint8        what the function returned (shape [Hs,Ws], or [H,W] when it gave up)
    sig/<function>           JSON         [[parameter, default or null, has default], ...]
"""
import ast
import inspect
import json
import os
import sys
import types

import numpy as np
import torch
from scipy.spatial import KDTree, cKDTree

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "fisher-nerf-customized_amd"))
import cloud_cases as cc                                                               # noqa: E402


def extract(path, name):
    tree = ast.parse(open(path).read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    ns = dict(np=np, torch=torch, KDTree=KDTree, cKDTree=cKDTree)
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns[name]


def signature(fn):
    return json.dumps([[p.name, None if p.default is inspect.Parameter.empty else p.default, p.default is not inspect.Parameter.empty]
                       for p in inspect.signature(fn).parameters.values()])


def main(ref_root):
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    metrics = extract(os.path.join(ref_root, "scripts", "eval_3d_reconstruction.py"), "accuracy_comp_ratio_from_pcl")
    novelty = extract(os.path.join(ref_root, "test_utils.py"), "novelty_mask_from_pcd_nn")
    out = {"sig/accuracy_comp_ratio_from_pcl": np.array(signature(metrics)), "sig/novelty_mask_from_pcd_nn": np.array(signature(novelty))}
    names = []
    for family, N, M in cc.GOLDEN_POINTS:
        gt, rec, seed = cc.qualifying_case(family, N, M)
        assert cc.qualifies_points(rec, gt)                      # the swapped call's distances too
        name = f"{family}/{N}/{M}/{seed}"
        names.append(name)
        for th in cc.THRESHOLDS:
            out[f"{name}/{th}/forward"] = np.array(metrics(gt, rec, th), np.float64)
            out[f"{name}/{th}/swapped"] = np.array(metrics(rec, gt, th), np.float64)
            print(name, th, out[f"{name}/{th}/forward"], out[f"{name}/{th}/swapped"])
    dnames = []
    for H, W, kind, z_forward, stride in cc.GOLDEN_DEPTH:
        c = cc.qualifying_depth_case(H, W, kind, z_forward)
        name = f"{H}/{W}/{kind}/{z_forward}/{stride}/{c['seed']}"
        dnames.append(name)
        mask = novelty(torch.from_numpy(c["env"]), c["depth"], torch.from_numpy(c["inv_K"]), torch.from_numpy(c["c2w"]), (H, W),
                       z_forward=z_forward, stride=stride)
        assert mask.dtype == np.uint8
        out[f"{name}/mask"] = mask
        print(name, mask.shape, int(mask.sum()))
    np.savez_compressed(os.path.join(HERE, "reference_cloud.npz"), points_cases=np.array(names), depth_cases=np.array(dnames), **out)


if __name__ == "__main__":
    main(sys.argv[1])
