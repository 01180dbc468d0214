#!/usr/bin/env python3
"""Golden vectors produced by RUNNING the reference's keyframe selection on the CPU: `keyframe_selection_overlap` and
`get_pointcloud` of models/SLAM/utils/keyframe_selection.py, imported from a reference checkout with `Tensor.cuda()` returning the
tensor.  Outputs only; no reference source is copied.  The inputs are not stored: tests/keyframe_cases.py regenerates them from
seeds, and `torch.randint` is checked to hand the reference the case's own draws.  Run from the repo root:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_reference_keyframe_vectors.py <reference tree>

reference_keyframe.npz holds, for each of the three qualifying cases "<family>/<seed>/<H>/<W>" listed in `cases` (five keyframes,
the reference's margin of 20 pixels):
    <case>/k                 int            the k the selection was asked for
    <case>/pts               float32 [M,3]  the points that survived get_pointcloud's filter inside the selection
    <case>/percent_inside    float32 [K]    per keyframe, as handed to sorted()
    <case>/selected          int64 [<=k]    the returned ids, under np.random.seed(11)
    <case>/sampled_indices   int64 [n,2]    the (row, col) pixels the selection sampled
    <case>/get_pointcloud    float32 [M,3]  get_pointcloud called on its own with them
"""
import builtins
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import keyframe_cases as kc                                                            # noqa: E402

FAMILIES = ["generic", "masks-mixed", "curr-mask"]
H, W, NK, K_ASKED = 96, 128, 5, 3


def main(ref_root):
    torch.Tensor.cuda = lambda self, *a, **k: self
    spec = importlib.util.spec_from_file_location("ref_keyframe_selection", os.path.join(ref_root, "models", "SLAM", "utils", "keyframe_selection.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    real_get_pointcloud, real_randint = ref.get_pointcloud, torch.randint
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    names, out = [], {}
    for family in FAMILIES:
        c = None
        for seed in range(kc.MAX_SEEDS):
            cand = kc.make_case(family, seed, H, W, n=24 if family.startswith("masks") else 64, K=NK)
            cand["edge"] = 20
            if kc.qualifies(cand):
                c = cand
                break
        assert c is not None, family
        name = f"{family}/{c['seed']}/{H}/{W}"
        seen = {}

        def recording_get_pointcloud(depth, intrinsics, w2c, sampled_indices):
            seen["sampled"] = sampled_indices.clone()
            seen["pts"] = real_get_pointcloud(depth, intrinsics, w2c, sampled_indices)
            return seen["pts"]

        def recording_sorted(items, **kw):
            items = list(items)
            seen["percent"] = [float(i["percent_inside"]) for i in items]
            return builtins.sorted(items, **kw)

        def checked_randint(*a, **kw):
            d = real_randint(*a, **kw)
            assert np.array_equal(d.numpy(), c["draws"]), "the reference did not draw the case's pixels"
            return d

        ref.get_pointcloud, ref.sorted, torch.randint = recording_get_pointcloud, recording_sorted, checked_randint
        try:
            torch.manual_seed(c["seed"])
            np.random.seed(11)
            selected = ref.keyframe_selection_overlap(t(c["depth"]), t(c["w2c"]), t(c["K"]), kc.keyframe_list(c), K_ASKED,
                                                      None if c["curr_mask"] is None else t(c["curr_mask"]), pixels=len(c["draws"]))
        finally:
            ref.get_pointcloud, torch.randint = real_get_pointcloud, real_randint
            del ref.sorted
        assert len(selected) > 0 and seen["pts"].dtype == torch.float32
        names.append(name)
        out[f"{name}/k"] = np.int64(K_ASKED)
        out[f"{name}/pts"] = seen["pts"].numpy()
        out[f"{name}/percent_inside"] = np.array(seen["percent"], np.float32)
        out[f"{name}/selected"] = np.array(selected, np.int64)
        out[f"{name}/sampled_indices"] = seen["sampled"].numpy().astype(np.int64)
        out[f"{name}/get_pointcloud"] = real_get_pointcloud(t(c["depth"]), t(c["K"]), t(c["w2c"]), seen["sampled"]).numpy()
        print(name, "points", seen["pts"].shape[0], "percent", seen["percent"], "selected", selected)
    np.savez_compressed(os.path.join(HERE, "reference_keyframe.npz"), cases=np.array(names), **out)


if __name__ == "__main__":
    main(sys.argv[1])
