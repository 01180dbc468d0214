"""Nearest point of another cloud on the device: reconstruction metrics and the novelty mask (fr_cloud_index_build / fr_cloud_query,
include/fisher_rast.h; arithmetic in csrc/fr_cloud_math.h).

  * `CloudIndex(points)` -- the index over one cloud, built once; `.query`, `.stats`, `.query_depth` run other points against it
    with no host synchronisation.
  * `reconstruction_metrics(gt, rec, dist_th)` -- accuracy, completion, completion ratio and their swapped counterparts from two
    directed searches and one host read (the reference builds six KD-trees for them: accuracy_comp_ratio_from_pcl called twice,
    tester_gaussians_navigation.py:1223-1224).
  * `accuracy_comp_ratio_from_pcl`, `novelty_mask_from_pcd_nn` -- drop-ins with the reference's names, parameter order and defaults
    (scripts/eval_3d_reconstruction.py:84-125, test_utils.py:503-578); `CloudEvalOps.install(module)` puts them in place of the
    names a module imported.

The search is binary32 and exact: float64 inputs are rounded to float32 on entry (the reference's clouds are float32 already).
"""
import ctypes
import struct

import numpy as np
import torch

from . import _lib
from ._lib import FisherRastError, CloudQueryCfg
from .ops import _ptr, _small_f32, _stream

MIN_NOVEL_PX = 20                     # test_utils.py:574


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _cloud_f32(x, dev=None):
    """a cloud [n,3] (NumPy or torch, on either device) as contiguous float32 on `dev`, without a host synchronisation: host values
    are staged in pinned memory and sent with a non-blocking copy (see ops._small_f32)"""
    t = x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
    t = t.detach()
    if t.dim() != 2 or t.shape[1] != 3:
        raise FisherRastError(f"a cloud must be [n,3], got {tuple(t.shape)}")
    if t.is_cuda:
        return t.to(dev or t.device).float().contiguous()
    t = t.float().contiguous()
    return t.pin_memory().to(dev or _device(), non_blocking=True) if t.numel() else torch.empty((0, 3), dtype=torch.float32, device=dev or _device())


def decode_stats(words):
    """the FR_CLOUD_STATS_WORDS 8-byte words, read on the host: dict(sum float, valid, flagged, skipped ints)"""
    w = [int(v) for v in np.asarray(words).reshape(-1)[:_lib.FR_CLOUD_STATS_WORDS]]
    return dict(sum=struct.unpack("<d", struct.pack("<q", w[0]))[0], valid=w[1], flagged=w[2], skipped=w[3])


def _mean(s):
    return s["sum"] / s["valid"] if s["valid"] else float("nan")


def _share(s):
    return s["flagged"] / s["valid"] if s["valid"] else float("nan")


def metrics_from_stats(rec_to_gt, gt_to_rec):
    """the five numbers from the decoded statistics of the two directed searches: `rec_to_gt` the reconstructed points against the
    index over the ground truth, `gt_to_rec` the other way round.  acc = mean distance rec -> gt, comp = mean distance gt -> rec,
    ratio = share of gt within dist_th of rec, iratio = share of rec within dist_th of gt (the ratio of the call with swapped
    arguments), fpr = 1 - iratio."""
    iratio = _share(rec_to_gt)
    return dict(acc=_mean(rec_to_gt), comp=_mean(gt_to_rec), ratio=_share(gt_to_rec), iratio=iratio, fpr=1.0 - iratio)


class CloudIndex:
    """The persistent index over `points` (float32 CUDA tensor [N,3], N may be 0; the tensor is kept and must not be written
    afterwards).  Holds the index and one grow-only query workspace, so calls on one index follow each other on one stream.  No method reads anything back."""

    def __init__(self, points):
        if not isinstance(points, torch.Tensor) or not points.is_cuda:
            raise FisherRastError("CloudIndex: points must live on a HIP device; fisher_rast has no CPU path")
        if points.dim() != 2 or points.shape[1] != 3 or points.dtype != torch.float32:
            raise FisherRastError(f"CloudIndex: points must be float32 [N,3], got {points.dtype} {tuple(points.shape)}")
        if points.shape[0] > _lib.FR_CLOUD_MAX_POINTS:
            raise FisherRastError(f"CloudIndex: {points.shape[0]} points, beyond FR_CLOUD_MAX_POINTS")
        points = points.detach().contiguous()
        lib = _lib.load()
        self.points = points                                    # kept: the queries when this cloud is searched against another
        self.device, self.N = points.device, int(points.shape[0])
        self.index_bytes = int(lib.fr_cloud_index_bytes(self.N))
        self.index = torch.empty((self.index_bytes // 8,), dtype=torch.int64, device=self.device)
        scratch = torch.empty((int(lib.fr_cloud_index_workspace_bytes(self.N)) // 8,), dtype=torch.int64, device=self.device)
        self._ws = None
        with torch.cuda.device(self.device):
            _lib.check(lib.fr_cloud_index_build(self.N, _ptr(points) if self.N else None, _ptr(self.index), self.index_bytes, _ptr(scratch),
                                                scratch.numel() * 8, _stream(self.device)), "fr_cloud_index_build")

    def _workspace(self, M):
        need = int(_lib.load().fr_cloud_query_workspace_bytes(M))
        if need == 0:
            raise FisherRastError(f"CloudIndex: {M} queries, beyond FR_CLOUD_MAX_POINTS")
        if self._ws is None or self._ws.numel() * 8 < need:
            self._ws = torch.empty(((need + 7) // 8,), dtype=torch.int64, device=self.device)
        return self._ws

    def _run(self, cfg, M):
        ws = self._workspace(M)
        with torch.cuda.device(self.device):
            _lib.check(_lib.load().fr_cloud_query(_ptr(self.index), self.index_bytes, self.N, ctypes.byref(cfg), _ptr(ws), ws.numel() * 8,
                                                  _stream(self.device)), "fr_cloud_query")

    def _queries(self, q):
        if not isinstance(q, torch.Tensor) or q.device != self.device or q.dtype != torch.float32 or q.dim() != 2 or q.shape[1] != 3:
            raise FisherRastError("CloudIndex: queries must be a float32 [M,3] tensor on the device of the index")
        return q.detach().contiguous()

    def _new(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    def search(self, q, dist_th=0.0, *, dist=True, index=False, flag=False, stats=False):
        """any subset of the outputs of one search of q [M,3]: dict(dist float32 [M], index int32 [M], flag uint8 [M] = d < dist_th,
        stats int64 [FR_CLOUD_STATS_WORDS] -- see decode_stats), the ones not asked for None"""
        q = self._queries(q)
        M = int(q.shape[0])
        out = dict(dist=self._new((M,), torch.float32) if dist else None, index=self._new((M,), torch.int32) if index else None,
                   flag=self._new((M,), torch.uint8) if flag else None,
                   stats=self._new((_lib.FR_CLOUD_STATS_WORDS,), torch.int64) if stats else None)
        cfg = CloudQueryCfg(source=_lib.FR_CLOUD_SOURCE_POINTS, M=M, dist_th=float(dist_th), queries=q.data_ptr() if M else None,
                            out_dist=out["dist"].data_ptr() if dist and M else None, out_idx=out["index"].data_ptr() if index and M else None,
                            out_flag=out["flag"].data_ptr() if flag and M else None, out_stats=out["stats"].data_ptr() if stats else None)
        self._run(cfg, M)
        return out

    def query(self, q, return_index=False):
        """distance from every row of q to its nearest finite target (float32 [M]; +inf where there is none or the row is not
        finite); with return_index also the lowest original index that attains it (int32 [M], -1 likewise)"""
        r = self.search(q, index=return_index)
        return (r["dist"], r["index"]) if return_index else r["dist"]

    def stats(self, q, dist_th):
        """device int64 [FR_CLOUD_STATS_WORDS]: {sum of distances (binary64 bits), finite queries, those with d < dist_th, skipped};
        decode_stats reads them on the host"""
        return self.search(q, dist_th, dist=False, stats=True)["stats"]

    def query_depth(self, depth, kinv, c2w, stride=1, flip_z=False, dist_th=0.05, want_dist=False):
        """the novelty rule on the sample grid of a depth image (float32 [H,W] on the device): (mask uint8 [Hs,Ws] -- 1 where the
        pixel's world point lies farther than dist_th from every target, 0 elsewhere and at a pixel without a depth --, stats as in
        `stats`, with `flagged` the novel pixels), and the distances float32 [Hs,Ws] behind them with want_dist.  kinv [3,3] and c2w
        (at least [3,4]) may live anywhere."""
        mask, stats, dist, _ = self._depth(depth, kinv, c2w, stride, flip_z, dist_th, want_dist)
        return (mask, stats, dist) if want_dist else (mask, stats)

    def _depth(self, depth, kinv, c2w, stride, flip_z, dist_th, want_dist=False):
        if not isinstance(depth, torch.Tensor) or depth.device != self.device or depth.dtype != torch.float32 or depth.dim() != 2:
            raise FisherRastError("CloudIndex.query_depth: depth must be a float32 [H,W] tensor on the device of the index")
        depth = depth.detach().contiguous()
        H, W, stride = int(depth.shape[0]), int(depth.shape[1]), int(stride)
        if H <= 0 or W <= 0 or stride <= 0:
            raise FisherRastError(f"CloudIndex.query_depth: H, W and stride must be positive, got {H}, {W}, {stride}")
        Hs, Ws = (H + stride - 1) // stride, (W + stride - 1) // stride
        M = Hs * Ws
        kinv, c2w = _small_f32(kinv, self.device, 3, 3, "kinv"), _small_f32(c2w, self.device, 3, 4, "c2w")
        words = (M + 7) // 8
        packed = self._new((words + _lib.FR_CLOUD_STATS_WORDS,), torch.int64)          # the mask bytes, then the statistics
        mask, stats = packed.view(torch.uint8)[:M].view(Hs, Ws), packed[words:]
        dist = self._new((Hs, Ws), torch.float32) if want_dist else None
        cfg = CloudQueryCfg(source=_lib.FR_CLOUD_SOURCE_DEPTH, H=H, W=W, stride=stride, flip_z=int(bool(flip_z)), dist_th=float(dist_th),
                            depth=depth.data_ptr(), kinv=kinv.data_ptr(), c2w=c2w.data_ptr(), out_dist=dist.data_ptr() if want_dist else None,
                            out_flag=mask.data_ptr(), out_stats=stats.data_ptr())
        self._run(cfg, M)
        return mask, stats, dist, packed


def _as_index(x, dev=None):
    return x if isinstance(x, CloudIndex) else CloudIndex(_cloud_f32(x, dev))


def reconstruction_metrics(gt, rec, dist_th=0.05):
    """dict(acc, comp, ratio, iratio, fpr) of a reconstructed cloud against the ground truth (see metrics_from_stats).  Either
    argument may be a CloudIndex built earlier (the ground truth of a run never changes): an index keeps its points, which are
    the queries of the other search.  Two directed searches, one host read."""
    dev = gt.device if isinstance(gt, CloudIndex) else (rec.device if isinstance(rec, CloudIndex) else None)
    gt_ix = _as_index(gt, dev)
    rec_ix = _as_index(rec, gt_ix.device)
    both = torch.stack([gt_ix.stats(rec_ix.points, dist_th), rec_ix.stats(gt_ix.points, dist_th)]).cpu().numpy()          # the one host read
    return metrics_from_stats(decode_stats(both[0]), decode_stats(both[1]))


def accuracy_comp_ratio_from_pcl(gt_points, rec_points, dist_th=0.05):
    """drop-in for scripts/eval_3d_reconstruction.py:84-125: (accuracy, completion, completion ratio)"""
    m = reconstruction_metrics(gt_points, rec_points, dist_th)
    return m["acc"], m["comp"], m["ratio"]


def novelty_kinv(inv_K_t, dtype=torch.float32):
    """test_utils.py:541-542, on the host as the reference takes it: inv(inv(inv_K)[:3,:3])"""
    K_t = torch.linalg.inv(inv_K_t.detach().to(device="cpu", dtype=dtype))[:3, :3]
    return torch.linalg.inv(K_t)


def novelty_mask_from_host(mask_sub, stats, H, W):
    """the reference's returns from the sub-sampled mask and the decoded statistics (test_utils.py:533-535, 573-578): an all-zero
    mask of the FULL shape when no pixel is valid or fewer than MIN_NOVEL_PX are novel"""
    if stats["valid"] == 0 or stats["flagged"] < MIN_NOVEL_PX:
        return np.zeros((H, W), dtype=np.uint8)
    return mask_sub


def novelty_mask_from_pcd_nn(env_pcd_xyz, depth_np, inv_K_t, c2w_t, img_hw, z_forward="-Z", dist_thresh_m=0.05, stride=1, frame_id=0):
    """drop-in for test_utils.py:503-578: uint8 NumPy mask [Hs,Ws] holding 1 where the observed point is farther than dist_thresh_m
    from the environment cloud.  env_pcd_xyz may be a CloudIndex, so that the index over the unchanging environment is built once
    per run instead of once per frame.  One host read."""
    H, W = int(img_hw[0]), int(img_hw[1])
    index = _as_index(env_pcd_xyz, c2w_t.device if isinstance(c2w_t, torch.Tensor) and c2w_t.is_cuda else None)
    dtype = c2w_t.dtype if isinstance(c2w_t, torch.Tensor) else torch.float32
    d = torch.as_tensor(np.asarray(depth_np)) if not isinstance(depth_np, torch.Tensor) else depth_np
    if tuple(d.shape) != (H, W):
        raise FisherRastError(f"novelty_mask_from_pcd_nn: depth is {tuple(d.shape)}, img_hw says {(H, W)}")
    d = d.detach().to(dtype).float().contiguous()
    depth = d.to(index.device) if d.is_cuda else d.pin_memory().to(index.device, non_blocking=True)
    kinv = novelty_kinv(inv_K_t if isinstance(inv_K_t, torch.Tensor) else torch.as_tensor(inv_K_t), dtype).float()
    c2w = c2w_t if isinstance(c2w_t, torch.Tensor) else torch.as_tensor(c2w_t, dtype=torch.float32)
    mask, _, _, packed = index._depth(depth, kinv, c2w.detach(), stride, z_forward in ("-Z", "-z"), dist_thresh_m)
    host = packed.cpu().numpy()                                                                            # the one host read
    M = mask.numel()
    stats = decode_stats(host[(M + 7) // 8:])
    return novelty_mask_from_host(host.view(np.uint8)[:M].reshape(tuple(mask.shape)).copy(), stats, H, W)


class CloudEvalOps:
    """The evaluation searches for the reference's driver: `install(module)` replaces the module-level names
    `accuracy_comp_ratio_from_pcl` and `novelty_mask_from_pcd_nn` -- those of the two the module has -- in the module that imported
    them (tester_gaussians_navigation.py looks them up there at every evaluation and, in known_env_mode, every frame).  Opt-in:
    nothing is installed by default."""

    NAMES = ("accuracy_comp_ratio_from_pcl", "novelty_mask_from_pcd_nn")

    @classmethod
    def install(cls, module):
        here = globals()
        found = [n for n in cls.NAMES if hasattr(module, n)]
        if not found:
            raise ValueError(f"CloudEvalOps.install: {getattr(module, '__name__', module)} defines neither of {', '.join(cls.NAMES)}")
        for n in found:
            setattr(module, n, here[n])
        return module
