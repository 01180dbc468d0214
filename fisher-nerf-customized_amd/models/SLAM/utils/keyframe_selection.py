"""Keyframe selection by overlap: which keyframes see the points of the current frame (the reference's
models/SLAM/utils/keyframe_selection.py, same names, arguments and return values), on fr_keyframe_valid_pixels / fr_keyframe_overlap
(include/fisher_rast.h, arithmetic in csrc/fr_keyframe_math.h).

The reference loops over the keyframes in Python, about fifteen small launches each, after a torch.where, a unique() and a
torch.inverse, and sorts 0-dim device tensors on the host (a synchronisation per comparison).  Here one call lists the pixels with a
measured depth, the host reads their count (the draw needs it), a second call back-projects the drawn pixels, applies the
reference's duplicate filter and counts the points every keyframe sees, and the host reads the counts: two host reads and a number of
launches that does not depend on the number of keyframes.  The random streams are consumed as the reference consumes them
(torch.randint on the CPU generator, np.random.permutation), so a seeded run selects the same keyframes."""
import numpy as np
import torch
import torch.nn.functional as F

from fisher_rast import ops as _ops

EDGE = 20          # pixels a projection has to stay away from the image border


class HipKeyframeBackend:
    """the two library calls (fisher_rast.ops.keyframe_valid_pixels / keyframe_overlap); there is no other backend in the package --
    the CPU tests put the g++ build of the same arithmetic behind the same two methods"""

    valid_pixels = staticmethod(_ops.keyframe_valid_pixels)
    overlap = staticmethod(_ops.keyframe_overlap)


def _depth_plane(depth):
    d = depth if depth.dtype == torch.float32 else depth.float()
    return d.contiguous()


def _keyframe_masks(keyframe_list, H, W):
    """per keyframe its object mask ('obj_mask_2d', else the older key 'mask') at the frame's resolution, or None"""
    masks = []
    for kf in keyframe_list:
        m = kf.get('obj_mask_2d', None)
        if m is None:
            m = kf.get('mask', None)
        if m is not None:
            m = m.bool()
            if tuple(m.shape[-2:]) != (H, W):
                m = F.interpolate(m[None, None].float(), size=(H, W), mode='nearest')[0, 0].bool()
        masks.append(m)
    return masks


class KeyframeSelection:
    """get_pointcloud and keyframe_selection_overlap over a backend's two calls; `last` keeps what the latest selection read from
    the device (counts per keyframe, kept points, out-of-range draws) for tests and benchmarks"""

    def __init__(self, backend):
        self.backend = backend
        self.last = None

    def get_pointcloud(self, depth, intrinsics, w2c, sampled_indices):
        """World points [M,3] of the pixels `sampled_indices` [n,2] = (row, col) of depth [1,H,W], without the ones the reference's
        filter drops: a point whose coordinates, rounded to four decimals and taken absolute, equal those of another sampled point
        or (0,0,0).  Selecting the kept rows is the one host synchronisation."""
        depth = _depth_plane(depth)
        W = int(depth.shape[-1])
        idx = sampled_indices.to(depth.device).long()
        out = self.backend.overlap(depth, intrinsics, w2c, idx[:, 0] * W + idx[:, 1], torch.empty((0, 4, 4)), edge=0, want_pts=True)
        return out["pts"][out["valid"].bool()]

    def keyframe_selection_overlap(self, gt_depth, w2c, intrinsics, keyframe_list, k, curr_mask=None, pixels=1600):
        """Ids (positions in `keyframe_list`) of up to k keyframes that see the current frame: `pixels` pixels are drawn, with
        replacement, among those with gt_depth > 0 (and inside curr_mask where given), back-projected through the inverse of w2c
        and projected into every keyframe's `est_w2c`; a keyframe overlaps when at least one point falls inside its image by more
        than EDGE pixels, in front of its camera and, where it carries an object mask, on the mask.  The result is a random k of
        the overlapping keyframes (a permutation of the list sorted by overlap, cut at k), as in the reference."""
        depth = _depth_plane(gt_depth)
        H, W = int(depth.shape[-2]), int(depth.shape[-1])
        valid_idx, status = self.backend.valid_pixels(depth, curr_mask)
        n_pixels = int(status[0])                                           # host read 1: the draw needs the count
        if n_pixels == 0:
            return []
        draws = torch.randint(n_pixels, (min(pixels, n_pixels),))
        K = len(keyframe_list)
        dev = depth.device
        kf_w2c = torch.stack([kf['est_w2c'].to(dev).float() for kf in keyframe_list]) if K else torch.empty((0, 4, 4))
        out = self.backend.overlap(depth, intrinsics, w2c, draws, kf_w2c, valid_idx=valid_idx, n_valid_idx=n_pixels,
                                   kf_masks=_keyframe_masks(keyframe_list, H, W), edge=EDGE, want_valid=False)
        host = torch.cat((out["counts"], out["status"])).cpu().numpy()     # host read 2: the counts and the number of kept points
        self.last = dict(counts=host[:K].copy(), n_valid=int(host[K]), out_of_range=int(host[K + 1]))
        with np.errstate(invalid="ignore", divide="ignore"):
            percent = host[:K].astype(np.float32) / np.float32(host[K])     # 0 / 0 is NaN: nothing kept, nothing selected
        order = sorted(range(K), key=lambda i: percent[i], reverse=True)    # stable: ties keep keyframe order
        selected = [i for i in order if percent[i] > 0.0]
        return list(np.random.permutation(np.array(selected))[:k])


_hip = KeyframeSelection(HipKeyframeBackend())
get_pointcloud = _hip.get_pointcloud
keyframe_selection_overlap = _hip.keyframe_selection_overlap
