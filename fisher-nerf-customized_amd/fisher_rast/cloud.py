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
  * `ReconTracker(gt, dist_th)` -- the same five numbers carried forward frame by frame (`add_frame`, `add_points`, `metrics`), at
    a cost per frame that does not depend on the frames before it: `CloudIndex.fold` is the seeded search behind it, and
    `query_depth(mask=, near=, want_points=)` the masked depth source.  `ReconStreamOps.install(tester_cls)` puts it in place of
    the reference's per-step store_filtered_obj_pointcloud / evaluate_3d_object_reconstruction; `object_recon_row` and
    `append_recon_row` are the YAML bookkeeping of the latter as pure functions.

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

    def __init__(self, points, *, storage=None):
        """storage: a dict the caller keeps between indices that replace one another (ReconTracker's frame index): its "index" and
        "scratch" tensors are used when they are large enough and replaced by larger ones when not, so that a run of builds
        allocates only while the clouds grow.  An index built into a storage is valid until the next one is."""
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
        storage = {} if storage is None else storage
        self.index = storage["index"] = self._grown(storage.get("index"), self.index_bytes)
        scratch = storage["scratch"] = self._grown(storage.get("scratch"), int(lib.fr_cloud_index_workspace_bytes(self.N)))
        self._ws = storage.get("workspace")
        self._storage = storage
        with torch.cuda.device(self.device):
            _lib.check(lib.fr_cloud_index_build(self.N, _ptr(points) if self.N else None, _ptr(self.index), self.index_bytes, _ptr(scratch),
                                                scratch.numel() * 8, _stream(self.device)), "fr_cloud_index_build")

    def _workspace(self, M):
        need = int(_lib.load().fr_cloud_query_workspace_bytes(M))
        if need == 0:
            raise FisherRastError(f"CloudIndex: {M} queries, beyond FR_CLOUD_MAX_POINTS")
        self._ws = self._storage["workspace"] = self._grown(self._ws, need)
        return self._ws

    def _grown(self, t, nbytes):
        if t is None or t.device != self.device or t.numel() * 8 < nbytes:
            t = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=self.device)
        return t

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

    def fold(self, q, seed_d2, dist_th=0.0, *, dist=False, flag=False, stats=False):
        """the seeded search: seed_d2 (float32 [M] on the device of the index; +inf, or what an earlier fold left) holds a running
        SQUARED distance per row of q and is updated in place to the smaller of itself and the squared distance to the nearest
        finite target of this index.  dist, flag and stats are taken from the folded value: after folding the indices of several
        clouds they are those of one search against the clouds' union, bit for bit.  A non-finite row of q keeps its seed and is
        counted as skipped.  Returns dict(dist, flag, stats), the ones not asked for None."""
        q = self._queries(q)
        M = int(q.shape[0])
        if (not isinstance(seed_d2, torch.Tensor) or seed_d2.device != self.device or seed_d2.dtype != torch.float32 or tuple(seed_d2.shape) != (M,)
                or not seed_d2.is_contiguous()):
            raise FisherRastError(f"CloudIndex.fold: seed_d2 must be a contiguous float32 [{M}] tensor on the device of the index")
        out = dict(dist=self._new((M,), torch.float32) if dist else None, flag=self._new((M,), torch.uint8) if flag else None,
                   stats=self._new((_lib.FR_CLOUD_STATS_WORDS,), torch.int64) if stats else None)
        cfg = CloudQueryCfg(source=_lib.FR_CLOUD_SOURCE_POINTS, M=M, dist_th=float(dist_th), queries=q.data_ptr() if M else None,
                            out_dist=out["dist"].data_ptr() if dist and M else None, out_flag=out["flag"].data_ptr() if flag and M else None,
                            out_stats=out["stats"].data_ptr() if stats else None, seed_d2=seed_d2.data_ptr() if M else None)
        self._run(cfg, M)
        return out

    def query_depth(self, depth, kinv, c2w, stride=1, flip_z=False, dist_th=0.05, want_dist=False, mask=None, near=False, want_points=False):
        """the novelty rule on the sample grid of a depth image (float32 [H,W] on the device): (mask uint8 [Hs,Ws] -- 1 where the
        pixel's world point lies farther than dist_th from every target, 0 elsewhere and at a pixel without a depth --, stats as in
        `stats`, with `flagged` the novel pixels), and the distances float32 [Hs,Ws] behind them with want_dist.  kinv [3,3] and c2w
        (at least [3,4]) may live anywhere.
        mask ([H,W] on the device; uint8 or bool, anything else is taken as mask > 0): only the pixels where it is set are
        queries, the others behave as pixels without a depth.  near: the returned mask and `flagged` mark d < dist_th instead.
        want_points: the samples' points float32 [Hs Ws, 3] are returned last, NaN rows where a sample is no query -- a cloud
        CloudIndex takes as it is."""
        flags, stats, dist, _, points = self._depth(depth, kinv, c2w, stride, flip_z, dist_th, want_dist, mask, near, want_points)
        return (flags, stats) + ((dist,) if want_dist else ()) + ((points,) if want_points else ())

    def _depth(self, depth, kinv, c2w, stride, flip_z, dist_th, want_dist=False, pixel_mask=None, near=False, want_points=False):
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
        points = self._new((M, 3), torch.float32) if want_points else None
        if pixel_mask is not None:
            if not isinstance(pixel_mask, torch.Tensor) or pixel_mask.device != self.device or tuple(pixel_mask.shape) != (H, W):
                raise FisherRastError(f"CloudIndex.query_depth: mask must be a [{H},{W}] tensor on the device of the index")
            pixel_mask = pixel_mask.detach()
            if pixel_mask.dtype != torch.uint8:
                pixel_mask = (pixel_mask if pixel_mask.dtype == torch.bool else pixel_mask > 0).view(torch.uint8)
            pixel_mask = pixel_mask.contiguous()
        cfg = CloudQueryCfg(source=_lib.FR_CLOUD_SOURCE_DEPTH, H=H, W=W, stride=stride, flip_z=int(bool(flip_z)), dist_th=float(dist_th),
                            depth=depth.data_ptr(), kinv=kinv.data_ptr(), c2w=c2w.data_ptr(), out_dist=dist.data_ptr() if want_dist else None,
                            out_flag=mask.data_ptr(), out_stats=stats.data_ptr(), mask=None if pixel_mask is None else pixel_mask.data_ptr(),
                            flag_near=int(bool(near)), out_points=points.data_ptr() if want_points else None)
        self._run(cfg, M)
        return mask, stats, dist, packed, points


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
    mask, _, _, packed, _ = index._depth(depth, kinv, c2w.detach(), stride, z_forward in ("-Z", "-z"), dist_thresh_m)
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


# ---- running reconstruction metrics --------------------------------------------------------------------------------------------------

class ReconTracker:
    """The five numbers of `reconstruction_metrics` carried forward frame by frame, at a cost per frame that does not depend on
    how many frames came before (the reference re-reads and re-indexes the whole accumulated cloud at every navigation step,
    tester_gaussians_navigation.py:508-550, 1212-1229).

      * completion side (comp, ratio): `best_d2`, the squared distance of every ground-truth point to the nearest reconstructed
        point so far; a frame is folded in by `CloudIndex.fold` (min over a union = min of the minima, exactly);
      * accuracy side (acc, iratio, fpr): a binary64 sum and integer counts over the reconstructed points, a frame's share of which
        never changes; they are added up on the device.

    `gt`: a cloud or a CloudIndex, indexed once.  `add_frame` and `add_points` read nothing back; `metrics()` reads once.
    keep_points: the frames' points are also kept, and `cloud()` returns the finite ones (for a caller that still writes the PLY).
    One query workspace and one frame-index buffer are kept and only grown.  A minimum cannot be undone: `reset()` is the only way
    to take a frame out again."""

    def __init__(self, gt, dist_th=0.05, keep_points=False):
        self.gt = _as_index(gt)
        self.device, self.dist_th, self.keep_points = self.gt.device, float(dist_th), bool(keep_points)
        self._frame = {}                                        # the storage of the frame index: index, scratch, query workspace
        self._empty = CloudIndex(torch.empty((0, 3), dtype=torch.float32, device=self.device))
        self.best_d2 = torch.empty((self.gt.N,), dtype=torch.float32, device=self.device)
        self.running = torch.empty((_lib.FR_CLOUD_STATS_WORDS,), dtype=torch.int64, device=self.device)   # {sum (binary64 bits), valid, near, skipped}
        self.reset()

    def reset(self):
        self.best_d2.fill_(float("inf"))
        self.running.zero_()
        self._chunks, self._cloud = [], torch.empty((0, 3), dtype=torch.float32, device=self.device)
        self.frames = 0

    def _fold(self, stats, points):
        self.running[:1].view(torch.float64).add_(stats[:1].view(torch.float64))
        self.running[1:].add_(stats[1:])
        CloudIndex(points, storage=self._frame).fold(self.gt.points, self.best_d2)
        if self.keep_points:
            self._chunks.append(points)
        self.frames += 1

    def add_frame(self, depth, kinv, cam_to_eval, mask=None, stride=1):
        """one depth frame (float32 [H,W] on the device; mask [H,W] or None): its masked pixels with a depth, back-projected
        through kinv [3,3] and cam_to_eval (the top [3,4] of camera -> the frame of the ground truth, composed by the caller; the
        camera looks along +Z), are searched against the ground truth and folded into the running state.  Three library calls, no
        host synchronisation."""
        _, stats, points = self.gt.query_depth(depth, kinv, cam_to_eval, stride=stride, dist_th=self.dist_th, mask=mask, near=True,
                                               want_points=True)
        self._fold(stats, points)

    def add_points(self, points):
        """the same for a cloud [n,3] that does not come from a depth image (non-finite rows are left out)"""
        points = _cloud_f32(points, self.device)
        self._fold(self.gt.stats(points, self.dist_th), points)

    def metrics(self):
        """dict(acc, comp, ratio, iratio, fpr) as reconstruction_metrics(gt, everything added so far) gives them, and n_rec, the
        number of reconstructed points behind them.  One statistics pass over best_d2 (a fold against an index without a target
        changes nothing and sums in the plain query's fixed order), one host read."""
        comp = self._empty.fold(self.gt.points, self.best_d2, self.dist_th, stats=True)["stats"]
        both = torch.stack([self.running, comp]).cpu().numpy()                                                   # the one host read
        rec_to_gt = decode_stats(both[0])
        return dict(metrics_from_stats(rec_to_gt, decode_stats(both[1])), n_rec=rec_to_gt["valid"])

    def cloud(self):
        """the finite points added so far, float32 [n,3] on the device (keep_points=True).  Compacts what was added since the last
        call, which reads a count back."""
        if not self.keep_points:
            raise FisherRastError("ReconTracker.cloud: the tracker was made with keep_points=False")
        if self._chunks:
            new = torch.cat(self._chunks)
            self._cloud = torch.cat([self._cloud, new[torch.isfinite(new).all(1)]])
            self._chunks = []
        return self._cloud


RECON_ROW_KEYS = ("step", "acc_distance_m", "comp_distance_m", "completeness_ratio", "fpr", "est_pcl_path")


def object_recon_row(step, metrics, est_path):
    """the row tester_gaussians_navigation.py:1237-1245 writes per evaluation: the reference's keys and its x 100 scaling; before
    any point was reconstructed its values for "no cloud file yet" (1228: all 0)"""
    if metrics.get("n_rec", 1) == 0:
        acc = comp = ratio = fpr = 0.0
    else:
        acc, comp, ratio, fpr = metrics["acc"], metrics["comp"], metrics["ratio"], metrics["fpr"]
    return {"step": int(step), "acc_distance_m": float(acc * 100), "comp_distance_m": float(comp * 100), "completeness_ratio": float(ratio * 100),
            "fpr": float(fpr * 100), "est_pcl_path": str(est_path)}


def new_recon_data(dist_th, policy_name="unknown", scene_id="unknown"):
    """the empty document of tester_gaussians_navigation.py:1249-1259"""
    return {"experiment": {"policy_name": policy_name, "scene_id": scene_id}, "settings": {"distance_threshold_m": float(dist_th)},
            "steps": [], "summary": {}}


def append_recon_row(data, row):
    """tester_gaussians_navigation.py:1261-1288 as a pure function of the document: the row appended, the rows sorted by step, the
    trapezoid AUC of the completeness percentage over the steps raw and normalised -- by max_steps * 100 when the settings carry
    max_steps, else by (last - first) * 100 --, the summary keys, and the normalised AUC written into the row.  Returns data."""
    data["steps"].append(row)
    data["steps"] = sorted(data["steps"], key=lambda r: r["step"])
    xs = [float(r["step"]) for r in data["steps"]]
    ys = [float(r["completeness_ratio"]) for r in data["steps"]]
    max_steps = int(data.get("settings", {}).get("max_steps", 0) or 0)
    auc_raw = float(sum((x1 - x0) * (y0 + y1) / 2.0 for x0, x1, y0, y1 in zip(xs, xs[1:], ys, ys[1:])))
    denom = max_steps * 100.0 if max_steps else ((xs[-1] - xs[0]) * 100.0 if len(xs) >= 2 else 1.0)
    auc_norm = float(auc_raw / denom) if denom > 0 else 0.0
    summary = data.setdefault("summary", {})
    summary["auc_completeness_percent_vs_steps_raw"] = auc_raw
    summary["auc_completeness_normalized_0_1"] = auc_norm
    summary["last_step"] = int(data["steps"][-1]["step"])
    summary["last_completeness_percent"] = float(data["steps"][-1]["completeness_ratio"])
    row["auc_until_now_normalized"] = auc_norm
    return data


def _host64(x):
    return (x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)).astype(np.float64)


class ReconStreamOps:
    """The reference's per-step object evaluation on a ReconTracker: `install(tester_cls, ...)` replaces
    `store_filtered_obj_pointcloud` and `evaluate_3d_object_reconstruction` (tester_gaussians_navigation.py:508-550, 1212-1289) on
    the class it is given.  The tracker is made at the first call from the instance's ground-truth cloud (`gt_attr`) and kept on
    the instance as `recon_tracker`.  No PLY is written or read and open3d is not imported.  Opt-in, beside CloudEvalOps."""

    HABITAT_TRANSFORM = ((1.0, 0.0, 0.0, 0.0), (0.0, -1.0, 0.0, 0.0), (0.0, 0.0, -1.0, 0.0), (0.0, 0.0, 0.0, 1.0))
    NAMES = ("store_filtered_obj_pointcloud", "evaluate_3d_object_reconstruction")

    @classmethod
    def install(cls, tester_cls, gt_attr="gt_obj_3d_rotated", eval_transform=HABITAT_TRANSFORM, dist_th=0.01):
        missing = [n for n in cls.NAMES if not hasattr(tester_cls, n)]
        if missing:
            raise ValueError(f"ReconStreamOps.install: {getattr(tester_cls, '__name__', tester_cls)} has no {', '.join(missing)}")
        T_eval = np.asarray(eval_transform, np.float64).reshape(4, 4)

        def tracker(self):
            if getattr(self, "recon_tracker", None) is None:
                self.recon_tracker = ReconTracker(_cloud_f32(getattr(self, gt_attr)), dist_th)
            return self.recon_tracker

        def store_filtered_obj_pointcloud(self, rgb, depth, intrinsics, object_mask_bw, camera_pose, object_pose, step=None):
            tr = tracker(self)
            on_host = not (isinstance(depth, torch.Tensor) and depth.is_cuda) and not (isinstance(object_mask_bw, torch.Tensor) and object_mask_bw.is_cuda)
            if on_host and not ((_host64(object_mask_bw) > 0) & (_host64(depth) > 0)).any():
                return None                                     # the reference's early return; device inputs are not read back for it
            # eval_transform inv(object_pose) camera_pose, composed once in binary64 and rounded to binary32
            cam_to_eval = T_eval @ np.linalg.inv(_host64(object_pose)) @ _host64(camera_pose)
            kinv = np.linalg.inv(_host64(intrinsics)[:3, :3])
            stage = lambda a, dt: a.to(tr.device, dt) if isinstance(a, torch.Tensor) and a.is_cuda else \
                torch.as_tensor(np.ascontiguousarray(a)).to(dt).pin_memory().to(tr.device, non_blocking=True)
            m = object_mask_bw if isinstance(object_mask_bw, torch.Tensor) else np.asarray(object_mask_bw)
            tr.add_frame(stage(depth, torch.float32), torch.from_numpy(kinv).float(), torch.from_numpy(cam_to_eval).float(),
                         mask=stage(m > 0, torch.uint8))
            self.recon_last_step = step
            return None

        def evaluate_3d_object_reconstruction(self, step=0):
            import os
            m = tracker(self).metrics()
            row = object_recon_row(step, m, f"recon_tracker:{tracker(self).frames}_frames")
            print(f"[eval] step={step} | ACC={row['acc_distance_m']:.2f} cm | COMP={row['comp_distance_m']:.2f} cm | "
                  f"Completeness={row['completeness_ratio']:.2f}% | FPR={row['fpr']:.2f}%")
            root = getattr(self, "policy_eval_dir", None)
            if root and os.path.isdir(root):
                import yaml
                path = os.path.join(root, "metrics", "object_recon_metrics.yaml")
                os.makedirs(os.path.dirname(path), exist_ok=True)
                data = None
                if os.path.exists(path):
                    with open(path) as f:
                        data = yaml.safe_load(f)
                data = data or new_recon_data(dist_th, getattr(self, "policy_name", "unknown"), getattr(self, "scene_id", "unknown"))
                append_recon_row(data, row)
                with open(path, "w") as f:
                    yaml.safe_dump(data, f, sort_keys=False)
            return m

        tester_cls.store_filtered_obj_pointcloud = store_filtered_obj_pointcloud
        tester_cls.evaluate_3d_object_reconstruction = evaluate_3d_object_reconstruction
        return tester_cls
