#!/usr/bin/env python3
"""Golden vectors produced by RUNNING the reference's map edit on the CPU: `remove_points`, `cat_params_to_optimizer`,
`prune_gaussians` and `densify` of models/SLAM/utils/slam_external.py, loaded from a reference checkout by file path, with stand-ins
for what cannot run here -- `torch.zeros(..., device="cuda")` allocates on the CPU, and `torch.normal(mean, std)` returns
mean + z std with the case's recorded z, so the normal samples are an input.  Data only; no reference source is copied.  Run from
the repo root:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reference_map_edit_vectors.py <reference tree>

reference_map_edit.npz (read it with map_edit_cases.load_golden: every group is one packed blob and its layout) holds the inputs, "state3/<key>" and "state1/<key>" for every key of map_edit_cases.make_state with 3 and
with 1 column of log_scales (parameters, Adam moments, statistics, the gradient of means2D, the normal samples z), and for each case of map_edit_cases.CASES, "<case>/<key>" for every key of map_edit_cases.snapshot
(parameters, Adam moments and step, statistics, the lengths of `seen` and `means2D`) after the call, and for the densify cases
    <case>/child_index   int32 [rows]   which child (its row of z) a row of the final map is, -1 for the rows that are none
    <case>/child_src     int32 [rows]   the original row it was split from, -1
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import map_edit_cases as mc                                                            # noqa: E402


def main(ref_root):
    spec = importlib.util.spec_from_file_location("reference_slam_external", os.path.join(ref_root, "models", "SLAM", "utils", "slam_external.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)                                                       # the reference's module
    real_zeros, real_remove = torch.zeros, ref.remove_points
    torch.zeros = lambda *a, **k: real_zeros(*a, **{n: v for n, v in k.items() if n != "device"})
    out = {"cases": np.array(list(mc.CASES))}
    for case, c in mc.CASES.items():
        st = mc.state_of(case)
        for k, v in st.items():
            out[f"state{c['cols']}/{k}"] = v
        masks = []

        def recording_remove_points(to_remove, *a, **k):
            masks.append(to_remove.clone().numpy())
            return real_remove(to_remove, *a, **k)

        ref.remove_points = recording_remove_points
        torch.normal = lambda mean, std: mean + torch.from_numpy(st["z"][:std.shape[0]]) * std
        snap, params, variables, opt, before = mc.run_case(case, ref, st, "cpu")
        mc.check_bookkeeping(params, variables, opt, before)                           # the reference's own bookkeeping passes the checks
        for k, v in snap.items():
            out[f"{case}/{k}"] = v
        if c["fn"] == "densify":
            # rows after the first removal: [originals that were not split, clones, children]; the second removal thins them
            P, n = mc.P_GOLDEN, c["cfg"]["num_to_split_into"]
            first, second = masks
            to_split = first[:P]
            assert not first[P:].any() and to_split.any(), case
            n_split = int(to_split.sum())
            n_other = first.size - P - n * n_split + (P - n_split)                     # originals kept + clones
            assert n_other > P - n_split, f"{case}: nothing was cloned"
            child1 = np.concatenate([np.full(n_other, -1), np.arange(n * n_split)])
            ci = child1[~second].astype(np.int32)
            assert (ci >= 0).any() and second.any() and ci.size == snap["p/means3D"].shape[0], case
            out[f"{case}/child_index"] = ci
            out[f"{case}/child_src"] = np.where(ci >= 0, np.flatnonzero(to_split)[np.maximum(ci, 0) % n_split], -1).astype(np.int32)
        print(case, "rows", mc.P_GOLDEN, "->", snap["p/means3D"].shape[0], [int(m.sum()) for m in masks], [m.size for m in masks])
    # one blob and one layout string per group (the two input states and the cases)
    groups = {}
    for k, v in out.items():
        if k != "cases":
            g = k.split("/")[0] if k.startswith("state") else "/".join(k.split("/")[:2])
            groups.setdefault(g, {})[k[len(g) + 1:]] = v
    packed = {"groups": np.array(list(groups))}
    for g, arrays in groups.items():
        packed[f"{g}:data"], layout = mc.pack(arrays)
        packed[f"{g}:layout"] = np.array(layout)
    np.savez_compressed(os.path.join(HERE, "reference_map_edit.npz"), **packed)


if __name__ == "__main__":
    main(sys.argv[1])
