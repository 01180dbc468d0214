"""The fused render-variable build (fr_rendervar_forward / fr_rendervar_backward, include/fisher_rast.h) as a torch autograd
function: everything between `params` and the rasteriser of a tracking / mapping iteration -- the frame transform of the means, the
(z, 1, z^2) depth / silhouette features, the normalised rotations, the opacities and the scales -- in one launch forward and one
backward (two with a camera gradient), without a host synchronisation.

`FrameRenderVars` is what models/SLAM/utils/slam_helpers.py (frame_render_vars, transform_to_frame) is written on.  Inputs the
kernels cannot take raise `RenderVarUnsupported` before anything is launched; there is no torch fallback in here."""
import torch

from fisher_rast import ops as _ops
from fisher_rast.ops import RenderVarUnsupported   # noqa: F401


class HipRenderVarBackend:
    """the kernels of csrc/fr_rendervar.hip on device tensors"""

    @staticmethod
    def check(tensors, time_idx):
        return _ops.rendervar_check(tensors, time_idx, need_cuda=True)

    forward = staticmethod(_ops.rendervar_forward)
    backward = staticmethod(_ops.rendervar_backward)


def default_backend():
    return HipRenderVarBackend


_INPUT_NAMES = ("means3D", "unnorm_rotations", "logit_opacities", "log_scales", "cam_unnorm_rots", "cam_trans")


class FrameRenderVars(torch.autograd.Function):
    """(pts [P,3], feats [P,3], rotations [P,4], opacities [P,1], scales [P,3]) of frame `time_idx`.

    `gaussians_grad` / `camera_grad` have transform_to_frame's meaning: means3D takes a gradient only with the first, the camera arrays
    only with the second (returned whole, [1,4,T] / [1,3,T], zero outside `time_idx`); the other three parameters take theirs whenever
    they require one.  An input given as None leaves out what is built from it: without `first_frame_w2c` there are no feats, without
    `unnorm_rotations` no rotations, and so on (the drop-in transform_to_frame asks for pts alone)."""

    @staticmethod
    def forward(ctx, means3D, unnorm_rotations, logit_opacities, log_scales, cam_unnorm_rots, cam_trans, time_idx, first_frame_w2c,
                gaussians_grad, camera_grad, backend=None):
        backend = backend or default_backend()
        time_idx = int(time_idx)
        inputs = dict(zip(_INPUT_NAMES, (means3D, unnorm_rotations, logit_opacities, log_scales, cam_unnorm_rots, cam_trans)))
        inputs = {k: (None if v is None else v.detach()) for k, v in inputs.items()}
        inputs["first_frame_w2c"] = None if first_frame_w2c is None else first_frame_w2c.detach()
        if means3D is None or cam_unnorm_rots is None or cam_trans is None:
            raise RenderVarUnsupported("rendervar: means3D and the camera arrays are required")
        P, scale_cols, n_frames = backend.check(inputs, time_idx)
        new = lambda cols: means3D.new_empty((P, cols))
        out = {
            "pts": new(3),
            "feats": new(3) if first_frame_w2c is not None else None,
            "rotations": new(4) if unnorm_rotations is not None else None,
            "opacities": new(1) if logit_opacities is not None else None,
            "scales": new(3) if log_scales is not None else None,
        }
        backend.forward(P, scale_cols, time_idx, n_frames, {**inputs, **out})
        need = ctx.needs_input_grad
        ctx.want = {
            "g_means3D": bool(gaussians_grad) and need[0],
            "g_unnorm_rotations": unnorm_rotations is not None and need[1],
            "g_logit_opacities": logit_opacities is not None and need[2],
            "g_log_scales": log_scales is not None and need[3],
            "g_cam_unnorm_rots": bool(camera_grad) and need[4],
            "g_cam_trans": bool(camera_grad) and need[5],
        }
        ctx.backend, ctx.dims = backend, (P, scale_cols, time_idx, n_frames)
        ctx.save_for_backward(means3D, unnorm_rotations, logit_opacities, log_scales, cam_unnorm_rots, cam_trans, first_frame_w2c)
        if not (ctx.want["g_means3D"] or ctx.want["g_cam_unnorm_rots"] or ctx.want["g_cam_trans"]):
            ctx.mark_non_differentiable(*(t for t in (out["pts"], out["feats"]) if t is not None))
        ctx.set_materialize_grads(False)
        return out["pts"], out["feats"], out["rotations"], out["opacities"], out["scales"]

    @staticmethod
    def backward(ctx, g_pts, g_feats, g_rotations, g_opacities, g_scales):
        P, scale_cols, time_idx, n_frames = ctx.dims
        inputs = dict(zip(_INPUT_NAMES + ("first_frame_w2c",), (None if t is None else t.detach() for t in ctx.saved_tensors)))
        want = ctx.want
        like = inputs["means3D"]

        def incoming(g):
            if g is None:
                return None
            return g if (g.dtype == torch.float32 and g.is_contiguous()) else g.float().contiguous()

        grads = {"g_pts": incoming(g_pts), "g_feats": incoming(g_feats), "g_rotations": incoming(g_rotations),
                 "g_opacities": incoming(g_opacities), "g_scales": incoming(g_scales)}
        outs = {
            "g_means3D": like.new_empty((P, 3)) if want["g_means3D"] else None,
            "g_cam_unnorm_rots": like.new_empty((1, 4, n_frames)) if want["g_cam_unnorm_rots"] else None,
            "g_cam_trans": like.new_empty((1, 3, n_frames)) if want["g_cam_trans"] else None,
        }
        # a parameter whose output took no gradient has a zero gradient: nothing to launch for it
        for name, src, g in (("g_unnorm_rotations", "unnorm_rotations", "g_rotations"), ("g_logit_opacities", "logit_opacities", "g_opacities"),
                             ("g_log_scales", "log_scales", "g_scales")):
            outs[name] = torch.empty_like(inputs[src]) if (want[name] and grads[g] is not None) else None
        if any(t is not None for t in outs.values()):
            ctx.backend.backward(P, scale_cols, time_idx, n_frames, {**inputs, **grads, **outs})
        return (outs["g_means3D"], outs["g_unnorm_rotations"], outs["g_logit_opacities"], outs["g_log_scales"],
                outs["g_cam_unnorm_rots"], outs["g_cam_trans"], None, None, None, None, None)
