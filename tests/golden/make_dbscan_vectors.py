"""Writes tests/golden/dbscan_cases.npz: sklearn.cluster.DBSCAN's labels_ for the qualifying cases of tests/cluster_cases.py
(GOLDEN: family, N, eps, min_samples), so that a machine without scikit-learn can compare against them.  The clouds themselves are
regenerated from (family, N, seed); only the seed that qualified, the parameters and the int16 labels are stored.

    python tests/golden/make_dbscan_vectors.py          (needs scikit-learn; the file was written with 1.7.2)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import cluster_cases as kc  # noqa: E402


def main():
    import sklearn
    from sklearn.cluster import DBSCAN
    out = {"sklearn_version": np.array(sklearn.__version__)}
    names = []
    for family, N, eps, min_samples in kc.GOLDEN:
        pts, seed = kc.qualifying_case(family, N, eps)
        ok = np.isfinite(pts).all(1)                               # sklearn raises on a non-finite row: those rows are noise here
        labels = np.full(N, -1, np.int64)
        labels[ok] = DBSCAN(eps=eps, min_samples=min_samples).fit(pts[ok]).labels_       # float32 rows, as gaussian.py:1239-1241 feeds it
        assert labels.max() < 2 ** 15 and N <= 5000
        name = f"{family}/{N}/{eps:g}/{min_samples}"
        names.append(name)
        out[name + "/seed"] = np.array(seed, np.int32)
        out[name + "/labels"] = labels.astype(np.int16)
    out["cases"] = np.array(names)
    path = os.path.join(HERE, "dbscan_cases.npz")
    np.savez_compressed(path, **out)
    print(f"{len(names)} cases, {os.path.getsize(path)} bytes -> {path}")


if __name__ == "__main__":
    main()
