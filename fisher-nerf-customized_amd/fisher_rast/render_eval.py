"""Render-quality evaluation of a map: what NavTester.eval_navigation reports per run (tester_gaussians_navigation.py:1397-1491),
PSNR, SSIM and the depth error of ~2000 rendered poses against Habitat's images, from the batched render (fr_render_views) and the
batched metrics (fr_view_metrics) -- a chunk of poses is one render call and one metrics call, and the whole evaluation reads the
host once.

    ev = evaluate_views(slam, c2ws, rgb_gt, depth_gt)          # rgb_gt: uint8 [V,H,W,3|4] as Habitat gives it, or float [V,3,H,W]
    ev.mean["psnr"], ev.mean["ssim"], ev.mean["depth_mae"]     # the tester's test/psnr, test/ssim, test/depth_mae

What differs from the reference's loop: the sums are binary64 in a fixed order (the same call gives the same bits); LPIPS is not
computed -- `on_chunk` hands the clamped images to the caller for it; the depth is the camera-frame z of the pose, which is
`render_at_pose`'s while `first_frame_w2c` is the identity (RenderOps.render_at_poses says the same)."""
import torch

from . import ops
from ._lib import FR_EVAL_ROW, FisherRastError


class ViewEvaluation:
    """The result of `evaluate_views`: per view `psnr`, `ssim`, `depth_mae`, `depth_rmse` (CPU float32 [V]; the depth entries NaN
    without a ground-truth depth) and `kept` (bool [V]: not left out by the reference's `torch.isinf(psnr)` rule); `mean`, the means over
    the kept views under the names the tester logs; `summary`, the library's 8 floats on the host; `rows`, the [V,8] device tensor."""

    def __init__(self, rows, rows_host, summary_host):
        self.rows = rows
        self.psnr, self.ssim = rows_host[:, 0].clone(), rows_host[:, 1].clone()
        self.depth_mae, self.depth_rmse = rows_host[:, 2].clone(), rows_host[:, 3].clone()
        self.kept = ~torch.isinf(self.psnr)
        self.summary = summary_host
        self.n_kept = int(summary_host[0])
        self.mean = {"psnr": float(summary_host[1]), "ssim": float(summary_host[2]), "depth_mae": float(summary_host[3]),
                     "depth_rmse": float(summary_host[4])}


def _scorer_and_poses(slam_or_scorer, c2ws):
    if isinstance(slam_or_scorer, ops.FisherScorer):
        if not isinstance(c2ws, torch.Tensor):
            raise ValueError("evaluate_views: with a FisherScorer the poses must be a [V,4,4] tensor")
        return slam_or_scorer, c2ws.reshape(-1, 4, 4).to(slam_or_scorer.dev).float()
    if not (hasattr(slam_or_scorer, "_scorer") and hasattr(slam_or_scorer, "_stack_poses")):
        raise ValueError("evaluate_views: needs a FisherScorer or a SLAM object with FisherOps installed")
    return slam_or_scorer._scorer(), slam_or_scorer._stack_poses(c2ws)


def _chunk_of(t, v0, v1, dev):
    """views [v0, v1) of a ground-truth tensor on the device (a host tensor goes over chunk by chunk)"""
    if t is None:
        return None
    c = t[v0:v1]
    return c if c.device == dev else c.to(dev, non_blocking=True)


def evaluate_views(slam_or_scorer, c2ws, gt_rgb, gt_depth=None, chunk=64, on_chunk=None):
    """Render V camera-to-world poses `chunk` at a time and score each chunk against its ground truth into its slice of one [V,8]
    tensor; the summary runs once over all rows and ONE host read brings rows, summary and the renders' status words over.
    gt_rgb: float32 [V,3,H,W] or uint8 [V,H,W,3|4]; gt_depth: float32 [V,1,H,W] / [V,H,W] or None; either may live on the host.
    Never more than one chunk of images is held.  `on_chunk(v0, v1, render, depth)` receives the chunk's clamped colour [n,3,H,W] and
    its depth [n,1,H,W] (a view of the render's buffer: copy what is to be kept) -- the place for the caller's own LPIPS or image
    dump; with it, and for images beyond 4096 tiles, the render goes through `FisherScorer.render_views`, which reads one status
    word per chunk.  Returns a ViewEvaluation."""
    scorer, poses = _scorer_and_poses(slam_or_scorer, c2ws)
    dev = scorer.dev
    V = int(poses.shape[0])
    if V < 1:
        raise ValueError("evaluate_views: no pose given")
    if int(gt_rgb.shape[0]) != V or (gt_depth is not None and int(gt_depth.shape[0]) != V):
        raise ValueError(f"evaluate_views: {V} poses, but ground truth for {int(gt_rgb.shape[0])}"
                         + ("" if gt_depth is None else f" / {int(gt_depth.shape[0])}") + " views")
    chunk = max(1, int(chunk))
    checked = on_chunk is not None or scorer.tiles > 4096
    if not checked:
        chunk = min(chunk, scorer.max_views_per_launch())
    rows = torch.empty((V, FR_EVAL_ROW), dtype=torch.float32, device=dev)
    scratch = torch.empty((FR_EVAL_ROW,), dtype=torch.float32, device=dev)       # a chunk's own summary: not used
    spans = [(v0, min(V, v0 + chunk)) for v0 in range(0, V, chunk)]
    statuses = []

    def score(v0, v1, render, depth_sil):
        depth = depth_sil[:, 0:1]
        if on_chunk is not None:
            render.clamp_(0.0, 1.0)
            on_chunk(v0, v1, render, depth)
        ops.view_metrics(render, _chunk_of(gt_rgb, v0, v1, dev), depth if gt_depth is not None else None, _chunk_of(gt_depth, v0, v1, dev),
                         clamp=True, out={"rows": rows[v0:v1], "summary": scratch})

    def checked_render(v0, v1):
        r = scorer.render_views(poses[v0:v1], poses_are_c2w=True, depth=False, final_T=False)
        score(v0, v1, r["render"], r["depth_sil"])

    for v0, v1 in spans:
        if checked:
            checked_render(v0, v1)
            continue
        r = scorer.render_launch(poses[v0:v1], poses_are_c2w=True, depth=False, final_T=False)
        statuses.append(r["status"])
        score(v0, v1, r["render"], r["depth_sil"])
    summary = ops.view_metrics_summary(rows)

    def read():                                                        # the one host read
        parts = [rows.reshape(-1).view(torch.int32), summary.view(torch.int32)] + statuses
        return torch.cat(parts).cpu()
    host = read()
    if statuses:
        st = host[(V + 1) * FR_EVAL_ROW:].reshape(-1, 4)
        redo = [i for i in range(len(spans)) if int(st[i, 1]) != 0]
        if redo:
            # a chunk's key buffer overflowed: nothing of it was rendered.  Redone through render_views, which grows the buffers.
            if any(int(st[i, 3]) & 2 for i in redo):
                raise FisherRastError("evaluate_views: the camera's view matrix is not the identity the scorer was promised")
            statuses = []
            for i in redo:
                checked_render(*spans[i])
            summary = ops.view_metrics_summary(rows)
            host = read()
    n = V * FR_EVAL_ROW
    return ViewEvaluation(rows, host[:n].view(torch.float32).reshape(V, FR_EVAL_ROW), host[n:n + FR_EVAL_ROW].view(torch.float32))
