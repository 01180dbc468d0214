"""DBSCAN and the target selection of global_planning on the device (fr_dbscan / fr_target_select, include/fisher_rast.h; arithmetic and
the labelling rule in csrc/fr_cluster_math.h).

  * `dbscan_labels(points, eps, min_samples)` -- sklearn.cluster.DBSCAN(eps, min_samples).fit(points).labels_ as an int32 device
    tensor; nothing is read back.
  * `select_target(means3D, score_points, lower_y, upper_y, q, eps, min_samples)` -- the middle of the reference's global_planning
    (models/SLAM/gaussian.py:1221-1267): height band, torch.quantile, `score > threshold`, DBSCAN, the cluster with the highest
    score, in one library call and ONE host read (the status block).

Distances are binary32 (float64 inputs are rounded to float32 on entry; the reference's clouds are float32 already), so a label can
differ from sklearn's only where a pair of points lies within rounding of eps.  A point with a non-finite coordinate is noise.
Everything runs on torch's current stream and allocates through torch only.
"""
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib
from ._lib import FisherRastError
from .ops import _ptr, _stream


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _f32_on_device(x, shape_tail, name, dev=None):
    """torch or NumPy, on either device, as contiguous float32 on the GPU (host values through pinned memory, non-blocking)"""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    t = t.detach()
    if tuple(t.shape[1:]) != shape_tail or t.dim() != 1 + len(shape_tail):
        raise FisherRastError(f"{name} must be [n{''.join(',%d' % d for d in shape_tail)}], got {tuple(t.shape)}")
    if t.is_cuda:
        return t.float().contiguous() if dev is None else t.to(dev).float().contiguous()
    dev = dev or _device()
    t = t.float().contiguous()
    return t.pin_memory().to(dev, non_blocking=True) if t.numel() else torch.empty(t.shape, dtype=torch.float32, device=dev)


def _check_params(eps, min_samples):
    eps, min_samples = float(eps), int(min_samples)
    if not eps > 0.0:
        raise FisherRastError(f"eps must be positive, got {eps}")
    if min_samples < 1:
        raise FisherRastError(f"min_samples must be at least 1, got {min_samples}")
    return eps, min_samples


def _workspace(nbytes, dev):
    return torch.empty(((int(nbytes) + 7) // 8,), dtype=torch.int64, device=dev)


def dbscan_raw(points, eps=0.1, min_samples=5):
    """(labels int32 [N], status int32 [FR_DBSCAN_STATUS_WORDS]) on the device of `points` (float32 [N,3] CUDA tensor); status =
    {clusters, finite points, the three cell sides as float bits, ...}.  No host synchronisation."""
    eps, min_samples = _check_params(eps, min_samples)
    lib = _lib.load()
    N, dev = int(points.shape[0]), points.device
    need = int(lib.fr_dbscan_workspace_bytes(N))
    if N and need == 0:
        raise FisherRastError(f"dbscan_labels: {N} points, beyond FR_CLUSTER_MAX_POINTS")
    labels = torch.empty((N,), dtype=torch.int32, device=dev)
    status = torch.empty((_lib.FR_DBSCAN_STATUS_WORDS,), dtype=torch.int32, device=dev)
    ws = _workspace(max(need, 8), dev)
    with torch.cuda.device(dev):
        _lib.check(lib.fr_dbscan(N, _ptr(points) if N else None, eps, min_samples, _ptr(labels) if N else None, _ptr(status), _ptr(ws),
                                 ws.numel() * 8, _stream(dev)), "fr_dbscan")
    return labels, status


def dbscan_labels(points, eps=0.1, min_samples=5):
    """sklearn.cluster.DBSCAN(eps=eps, min_samples=min_samples).fit(points).labels_ as int32 [N] on the device.  `points` [N,3] may
    be torch or NumPy, on either device; it is rounded to float32."""
    return dbscan_raw(_f32_on_device(points, (3,), "points"), eps, min_samples)[0]


class TargetSelection(NamedTuple):
    """What gaussian.py:1221-1267 computes, the tensors on the device and the counts on the host."""
    points_index_range: torch.Tensor          # int32 [n_band]: the rows of the map inside the height band, ascending
    points_index: torch.Tensor                # int32 [n_above]: those with score > threshold
    labels: torch.Tensor                      # int32 [n_above]: their DBSCAN labels
    selected_points_index: torch.Tensor       # int32 [n_selected]: those of them labelled max_label
    threshold: torch.Tensor                   # float32 []: torch.quantile(scores[band], q)
    n_band: int
    n_above: int
    n_clusters: int
    max_label: int                            # -1 when no cluster qualified: the selected rows are then the NOISE rows (the reference's quirk)
    n_selected: int
    argmax: int                               # the lowest row that attains the band's highest score (the reference's `else` branch)
    cell_sides: tuple                         # the DBSCAN grid's cell side per axis: above 1.125 eps where the cloud is wider than 1024 cells
    nan_scores: bool                          # a band score was NaN: this result came by the torch route


def _torch_route(means3D, scores, lower_y, upper_y, q):
    """the reference's own lines for a band with a NaN score: the threshold is NaN, nothing is above it, argmax is the NaN's row"""
    sign = torch.bitwise_and(means3D[:, 1] >= lower_y, means3D[:, 1] <= upper_y)
    band = torch.where(sign)[0]
    sel = scores[sign]
    threshold = torch.quantile(sel, q)
    above = band[sel > threshold].to(torch.int32)
    empty = torch.empty((0,), dtype=torch.int32, device=means3D.device)
    return TargetSelection(band.to(torch.int32), above, torch.full_like(above, -1), empty, threshold, int(band.numel()), int(above.numel()), 0, -1, 0,
                           int(band[torch.argmax(sel)]), (float("nan"),) * 3, True)


def select_target(means3D, score_points, lower_y, upper_y, q=0.8, eps=0.1, min_samples=5) -> TargetSelection:
    """The target selection of global_planning over means3D [P,3] and score_points [P] (torch or NumPy, on either device; rounded
    to float32).  Raises RuntimeError for an empty band, as torch.quantile does on an empty tensor.  One host read."""
    eps, min_samples = _check_params(eps, min_samples)
    if not 0.0 <= float(q) <= 1.0:
        raise FisherRastError(f"q must lie in [0, 1], got {q}")
    means = _f32_on_device(means3D, (3,), "means3D")
    scores = _f32_on_device(score_points, (), "score_points", means.device)
    P, dev = int(means.shape[0]), means.device
    if int(scores.shape[0]) != P:
        raise FisherRastError(f"score_points has {int(scores.shape[0])} entries for {P} Gaussians")
    lib = _lib.load()
    need = int(lib.fr_target_select_workspace_bytes(P))
    if P and need == 0:
        raise FisherRastError(f"select_target: {P} Gaussians, beyond FR_CLUSTER_MAX_POINTS")
    lists = torch.empty((4, max(P, 1)), dtype=torch.int32, device=dev)                 # band, above, labels, selected
    words = _lib.FR_TARGET_STATUS_WORDS
    head = torch.empty((words + 1,), dtype=torch.int32, device=dev)                    # the status block, then the threshold
    status, threshold = head[:words], head[words:].view(torch.float32)
    ws = _workspace(max(need, 8), dev)
    with torch.cuda.device(dev):
        _lib.check(lib.fr_target_select(P, _ptr(means) if P else None, _ptr(scores) if P else None, float(lower_y), float(upper_y), float(q),
                                        eps, min_samples, _ptr(lists[0]), _ptr(lists[1]), _ptr(lists[2]), _ptr(lists[3]), _ptr(threshold),
                                        _ptr(status), _ptr(ws), ws.numel() * 8, _stream(dev)), "fr_target_select")
    host = status.cpu().numpy()                                                        # the one host read
    n_band, n_above, n_clusters, max_label, n_selected, argmax = (int(v) for v in host[:6])
    if n_band == 0:
        raise RuntimeError("select_target: no Gaussian lies in the height band (quantile() input tensor must be non-empty)")
    if int(host[9]):
        return _torch_route(means, scores, float(lower_y), float(upper_y), float(q))
    sides = tuple(float(v) for v in host[6:9].copy().view(np.float32))
    return TargetSelection(lists[0, :n_band], lists[1, :n_above], lists[2, :n_above], lists[3, :n_selected], threshold[0], n_band, n_above,
                           n_clusters, max_label, n_selected, argmax, sides, False)
