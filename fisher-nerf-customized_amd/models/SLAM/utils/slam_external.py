"""Densification / pruning statistics of the training step (models/SLAM/utils/slam_external.py:196-200, 345-465 and the tail of
get_loss, models/SLAM/gaussian.py:289-291) on MI355X: each torch-op chain of the reference is one kernel pass over the
Gaussians (fr_densify_stats / fr_densify_masks / fr_prune_mask, include/fisher_rast.h).

`calc_ssim` / `calc_ssim_masked` (slam_external.py:89-120, 144-193) are the fused image-loss kernels (fr_image_loss_forward /
fr_image_loss_backward through fisher_rast/image_loss.py): one forward launch pair, one backward launch, no host synchronisation.
`calc_mse` / `calc_psnr` (slam_external.py:68-74) take a float32 [3,H,W] pair on the device through fr_view_metrics.
`get_gaussians_outside_mask` (slam_external.py:270-343) is fr_outside_mask through fisher_rast/object_loss.py: two launches and one host read.

What the reference then DOES with a mask -- cloning / splitting the parameter tensors, rebuilding the Adam state
(cat_params_to_optimizer, remove_points, slam_external.py:203-262) and the bodies of prune_gaussians / densify (345-463) -- is the map
edit: `remove_points`, `cat_params_to_optimizer`, `update_params_and_optimizer`, `prune_gaussians` and `densify` below, call-compatible
with the reference's.  A row's destination depends on the masks alone, so one ordered compaction of the masks (fr_map_edit_plan), one
host read of the three counts and one gather over a table of every parameter, both Adam moments of each and the per-Gaussian
statistics (fr_map_edit_apply) replace the reference's ~20 boolean indexings per remove_points and ~15 cats per
cat_params_to_optimizer; the split children are written by fr_map_edit_split_children (csrc/fr_mapedit_math.h).  The bookkeeping
around those calls (`MapEdit`) takes the plan / apply steps from a backend object, `HipMapEditBackend` on the device, so the tests
run the very same Python on the CPU with a NumPy backend.
"""
import ctypes

import torch

from fisher_rast import _lib
from fisher_rast import image_loss as _il


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _f32(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def update_seen_and_radius(variables, radius):
    """The tail of get_loss (gaussian.py:289-291): variables['seen'] = radius > 0 and, where seen,
    max_2D_radius = max(radius, max_2D_radius) -- in place."""
    dev = radius.device
    P = int(radius.shape[0])
    radii = radius if (radius.dtype == torch.int32 and radius.is_contiguous()) else radius.to(torch.int32).contiguous()
    seen = torch.empty((P,), dtype=torch.bool, device=dev)
    mr = variables['max_2D_radius']
    assert mr.dtype == torch.float32 and mr.is_contiguous()
    with torch.cuda.device(dev):
        _lib.check(_lib.load().fr_densify_stats(P, radii.data_ptr(), None, mr.data_ptr(), None, None, seen.data_ptr(), _stream(dev)),
                   "fr_densify_stats")
    variables['seen'] = seen
    return variables


def accumulate_mean2d_gradient(variables, radius=None):
    """slam_external.py:196-200: means2D_gradient_accum[seen] += |means2D.grad[seen, :2]|, denom[seen] += 1 -- in place.
    With `radius` (the colour render's radii) the visibility comes from it and max_2D_radius / seen are updated in the same
    pass (the tail of get_loss); without, variables['seen'] is used as the reference does."""
    grad = _f32(variables['means2D'].grad)
    dev = grad.device
    P = int(grad.shape[0])
    acc, den = variables['means2D_gradient_accum'], variables['denom']
    assert acc.dtype == den.dtype == torch.float32 and acc.is_contiguous() and den.is_contiguous()
    lib = _lib.load()
    with torch.cuda.device(dev):
        if radius is not None:
            radii = radius if (radius.dtype == torch.int32 and radius.is_contiguous()) else radius.to(torch.int32).contiguous()
            seen = torch.empty((P,), dtype=torch.bool, device=dev)
            _lib.check(lib.fr_densify_stats(P, radii.data_ptr(), grad.data_ptr(), variables['max_2D_radius'].data_ptr(), acc.data_ptr(),
                                            den.data_ptr(), seen.data_ptr(), _stream(dev)), "fr_densify_stats")
            variables['seen'] = seen
        else:
            radii = variables['seen'].to(torch.int32)             # 1 where seen: max_2D_radius is not touched on this route
            _lib.check(lib.fr_densify_stats(P, radii.data_ptr(), grad.data_ptr(), None, acc.data_ptr(), den.data_ptr(), None, _stream(dev)),
                       "fr_densify_stats")
    return variables


def densify_masks(params, variables, grad_thresh, clone_max_scale=0.05, split_min_scale=0.05):
    """(to_clone, to_split) of densify() (slam_external.py:419-433) as bool tensors.  NOTE the reference evaluates to_split AFTER
    the clones were appended; a clone has max scale <= clone_max_scale, so with the default thresholds the mask over the
    grown array is this mask followed by False for every clone."""
    ls = _f32(params['log_scales'])
    dev = ls.device
    P, cols = int(ls.shape[0]), int(ls.shape[1]) if ls.dim() == 2 else 1
    to_clone = torch.empty((P,), dtype=torch.bool, device=dev)
    to_split = torch.empty((P,), dtype=torch.bool, device=dev)
    acc, den = _f32(variables['means2D_gradient_accum']), _f32(variables['denom'])
    with torch.cuda.device(dev):
        _lib.check(_lib.load().fr_densify_masks(P, acc.data_ptr(), den.data_ptr(), ls.data_ptr(), cols, float(grad_thresh),
                                                float(clone_max_scale), float(split_min_scale), to_clone.data_ptr(), to_split.data_ptr(),
                                                _stream(dev)), "fr_densify_masks")
    return to_clone, to_split


def prune_mask(params, opacity_thresh, big_thresh=None):
    """to_remove of prune_gaussians() / of the removal pass of densify() (slam_external.py:354, 394-396, 452-457):
    sigmoid(logit_opacities) < opacity_thresh, OR-ed with max scale > big_thresh when big_thresh is given
    (0.1 in prune_gaussians, 0.1 * scene_radius in densify)."""
    lo, ls = _f32(params['logit_opacities']).reshape(-1), _f32(params['log_scales'])
    dev = lo.device
    P, cols = int(lo.shape[0]), int(ls.shape[1]) if ls.dim() == 2 else 1
    out = torch.empty((P,), dtype=torch.bool, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().fr_prune_mask(P, lo.data_ptr(), ls.data_ptr(), cols, float(opacity_thresh),
                                             -1.0 if big_thresh is None else float(big_thresh), out.data_ptr(), _stream(dev)), "fr_prune_mask")
    return out


def _check_window(window_size):
    if window_size != 11:
        raise NotImplementedError(f"calc_ssim: only window_size == 11 is built (the reference passes no other), got {window_size}")


def calc_ssim(img1, img2, window_size=11, size_average=True):
    """slam_external.py:89-120: the mean SSIM of img1 against img2 ([C,H,W] or [B,C,H,W]; a batch folds into the channels), or
    with size_average=False the per-batch means [B], from the per-channel sums.  Differentiable w.r.t. img1 (with
    size_average=False for a single image only; img2 must not require a gradient)."""
    _check_window(window_size)
    if size_average:
        return _il.image_loss(img1, img2, None, 0.0, -1.0, _il.FR_LOSS_L1_SUM, which=_il.OUT_SSIM)[0]
    B = int(img1.shape[0]) if img1.dim() == 4 else 1
    if B == 1:
        return _il.image_loss(img1, img2, None, 0.0, -1.0, _il.FR_LOSS_L1_SUM, which=_il.OUT_SSIM)[0].reshape(1)
    if img1.requires_grad and torch.is_grad_enabled():
        raise NotImplementedError("calc_ssim(size_average=False): the gradient of a batch's per-image means is not built")
    chan = _il.image_loss(img1.detach(), img2, None, 0.0, -1.0, _il.FR_LOSS_L1_SUM, which=_il.OUT_SSIM, want_channels=True)[1]
    return chan.reshape(B, -1).mean(1)


def calc_ssim_masked(img1, img2, mask, window_size=11):
    """slam_external.py:144-193: the SSIM map's mean over the channels, weighted by `mask` ([1,H,W] or [H,W], 0 / 1) with
    clamp_min(1) on its count.  img1, img2: [C,H,W] (or [1,C,H,W]).  Differentiable w.r.t. img1."""
    _check_window(window_size)
    if img1.dim() == 4:
        if img1.shape[0] != 1:
            raise NotImplementedError("calc_ssim_masked: one image at a time (the reference's callers pass [3,H,W])")
        img1, img2 = img1[0], img2[0]
    H, W = int(img1.shape[-2]), int(img1.shape[-1])
    return _il.image_loss(img1, img2, mask.reshape(1, H, W), 0.0, -1.0, _il.FR_LOSS_L1_SUM, weights_map=True, which=_il.OUT_SSIM)[0]


def _on_kernel(img1, img2):
    """a float32 [3,H,W] pair on one HIP device that asks for no gradient: what fr_view_metrics takes as one view"""
    return (isinstance(img1, torch.Tensor) and isinstance(img2, torch.Tensor) and img1.is_cuda and img1.device == img2.device
            and img1.dtype == img2.dtype == torch.float32 and img1.dim() == 3 and img1.shape[0] == 3 and img1.shape == img2.shape
            and img1.numel() > 0 and not (torch.is_grad_enabled() and (img1.requires_grad or img2.requires_grad)))


def calc_mse(img1, img2):
    """slam_external.py:68-69: the mean squared difference per channel, [C,1].  A float32 [3,H,W] pair on a HIP device is one
    fr_view_metrics call (binary64 sums in a fixed order, rounded once); anything else takes the torch expression."""
    if _on_kernel(img1, img2):
        from fisher_rast.ops import view_metrics
        return view_metrics(img1.contiguous().unsqueeze(0), img2.contiguous().unsqueeze(0), clamp=False)["rows"][0, 4:7].reshape(3, 1)
    return torch.square(img1 - img2).reshape(img1.shape[0], -1).mean(dim=1, keepdim=True)


def calc_psnr(img1, img2):
    """slam_external.py:72-74: 20 log10(1 / sqrt(mse)) per channel, [C,1]; +inf where the channels are equal."""
    return 20 * torch.log10(1.0 / torch.sqrt(calc_mse(img1, img2)))


def get_gaussians_outside_mask(params, curr_data, obj_mask_2d, with_indices=True):
    """slam_external.py:270-343, same arguments and return: (outside_mask bool [N], stats) for the frame `curr_data['id']` of the
    camera trajectory in `params` -- the Gaussians that do not project into `obj_mask_2d` (those outside the image or behind the
    camera included), the counts and the ranges of the largest scale inside and outside.  Two launches (fr_outside_mask) and ONE host
    read, of the status block, in place of the reference's two nonzero calls and four .item() reads; `idx_in` / `idx_out` are taken
    from the byte masks after the read, with the counts it brought (no further synchronisation).  `with_indices=False` (not in the
    reference's signature; none of its callers reads the lists) leaves them out of `stats`."""
    from fisher_rast import object_loss as _ol
    from models.SLAM.gaussian import frame_w2c              # (that module imports this one)
    outside, status = _ol.outside_mask(params, frame_w2c(params, curr_data['id']), curr_data['intrinsics'], obj_mask_2d)
    st = status.cpu()                                        # the one host read
    counts, ranges = st[:2].tolist(), st[2:].view(torch.float32).tolist()
    stats = {
        'in_count': int(counts[0]),
        'out_count': int(counts[1]),
        'total': int(outside.shape[0]),
        'inside_scale_min': ranges[0],
        'inside_scale_max': ranges[1],
        'outside_scale_min': ranges[2],
        'outside_scale_max': ranges[3],
    }
    if with_indices:
        inside = torch.logical_not(outside)
        if hasattr(torch, "nonzero_static"):
            stats['idx_in'] = torch.nonzero_static(inside, size=stats['in_count']).squeeze(1)
            stats['idx_out'] = torch.nonzero_static(outside, size=stats['out_count']).squeeze(1)
        else:
            stats['idx_in'] = torch.nonzero(inside, as_tuple=False).squeeze(1)
            stats['idx_out'] = torch.nonzero(outside, as_tuple=False).squeeze(1)
    return outside, stats


# ---- the map edit: a prune or densify mask applied to the map, its Adam state and its statistics ---------------------------------

_CAM_KEYS = ('cam_unnorm_rots', 'cam_trans')
_STAT_KEYS = ('means2D_gradient_accum', 'denom', 'max_2D_radius')
# densify's scale thresholds (slam_external.py:419, 427), hard-coded there.  The reference evaluates to_split AFTER the clones were
# appended; a clone has max scale <= CLONE_MAX_SCALE, so while CLONE_MAX_SCALE <= SPLIT_MIN_SCALE no clone is ever split and masks
# over the original rows state the whole edit.  They must not cross: with CLONE_MAX_SCALE > SPLIT_MIN_SCALE a row could be cloned
# and both it and its clone split, which a plan over the original rows cannot express.
CLONE_MAX_SCALE = 0.05
SPLIT_MIN_SCALE = 0.05
assert CLONE_MAX_SCALE <= SPLIT_MIN_SCALE


class MapEditPlan:
    """Where every source row goes: the counts as the host read them, and the backend's handle on the three index lists."""

    def __init__(self, P, n_keep, n_clone, n_split, n_into, handle):
        self.P, self.n_keep, self.n_clone, self.n_split, self.n_into, self.handle = int(P), int(n_keep), int(n_clone), int(n_split), int(n_into), handle

    @property
    def rows(self):
        return self.n_keep + self.n_clone + self.n_into * self.n_split

    @property
    def first_child(self):
        return self.n_keep + self.n_clone


class HipMapEditBackend:
    """The device side of the map edit: the mask kernels, fr_map_edit_plan with its one host read, fr_map_edit_apply over a table
    of tensors and fr_map_edit_split_children, on the current torch stream."""

    prune_mask = staticmethod(prune_mask)
    accumulate = staticmethod(accumulate_mean2d_gradient)

    @staticmethod
    def densify_masks(params, variables, grad_thresh):
        return densify_masks(params, variables, grad_thresh, CLONE_MAX_SCALE, SPLIT_MIN_SCALE)

    @staticmethod
    def _mask_ptr(m, P):
        if m is None:
            return None, None
        m = m.reshape(-1)
        if m.dtype not in (torch.bool, torch.uint8) or not m.is_contiguous():
            m = (m != 0).contiguous()
        assert m.shape[0] == P, f"a mask of {m.shape[0]} rows for a map of {P}"
        return m, m.data_ptr()

    def plan(self, P, keep, clone, split, n_into, device, read_with=None):
        """(MapEditPlan, read_with on the host).  keep / clone / split: bool or byte tensors [P] or None.  `read_with`: a float32
        scalar on the device comes over in the same host read as the counts (another tensor costs a read of its own)."""
        lib = _lib.load()
        if not hasattr(lib, "fr_map_edit_plan"):
            raise _lib.FisherRastError("libfisher_rast.so has no fr_map_edit_plan: rebuild it")
        nws = int(lib.fr_map_edit_workspace_bytes(P))
        ws = torch.empty((max(nws, 8),), dtype=torch.uint8, device=device)
        status = torch.empty((_lib.FR_EDIT_STATUS_WORDS,), dtype=torch.int32, device=device)
        held = [self._mask_ptr(m, P) for m in (keep, clone, split)]
        with torch.cuda.device(device):
            _lib.check(lib.fr_map_edit_plan(P, held[0][1], held[1][1], held[2][1], status.data_ptr(), ws.data_ptr(), nws, _stream(device)),
                       "fr_map_edit_plan")
        extra = read_with
        if torch.is_tensor(read_with) and read_with.is_cuda and read_with.dtype == torch.float32 and read_with.numel() == 1:
            both = torch.cat((status, read_with.detach().reshape(1).view(torch.int32))).cpu()               # the one host read
            st, extra = both[:4].tolist(), both[4:].view(torch.float32)[0]
        else:
            st = status.cpu().tolist()                                                                       # the one host read
            if torch.is_tensor(read_with):
                extra = read_with.detach().cpu()
        return MapEditPlan(P, st[0], st[1], st[2], n_into, ws), extra

    def apply(self, plan, table):
        """table: [(tensor [P, ...], FR_EDIT_COPY or FR_EDIT_ZERO), ...] -> the edited tensors, [plan.rows, ...] each"""
        lib = _lib.load()
        entries, out, held = [], [], []
        for src, mode in table:
            src = src.detach()
            if not src.is_contiguous():
                src = src.contiguous()
            assert src.shape[0] == plan.P, f"a tensor of {src.shape[0]} rows in an edit of {plan.P}"
            row_bytes = src.element_size()
            for d in src.shape[1:]:
                row_bytes *= int(d)
            if row_bytes % 4 or not 1 <= row_bytes // 4 <= _lib.FR_EDIT_MAX_COLS:
                raise NotImplementedError(f"map edit: rows of {row_bytes} bytes (1 to {_lib.FR_EDIT_MAX_COLS} 4-byte words are built)")
            dst = torch.empty((plan.rows,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
            entries.append(_lib.MapEditArray(src.data_ptr(), dst.data_ptr(), row_bytes // 4, mode))
            held.append(src)
            out.append(dst)
        if entries:
            dev = out[0].device
            with torch.cuda.device(dev):
                for i in range(0, len(entries), _lib.FR_EDIT_MAX_ARRAYS):
                    chunk = entries[i:i + _lib.FR_EDIT_MAX_ARRAYS]
                    _lib.check(lib.fr_map_edit_apply((_lib.MapEditArray * len(chunk))(*chunk), len(chunk), plan.P, plan.n_keep, plan.n_clone,
                                                     plan.n_split, plan.n_into, plan.handle.data_ptr(), _stream(dev)), "fr_map_edit_apply")
        return out

    @staticmethod
    def randn(rows, like, generator=None):
        return torch.randn((rows, 3), dtype=torch.float32, device=like.device, generator=generator)

    def split_children(self, plan, z, means, rots, logs):
        """in place on rows [plan.first_child:] of the edited means3D / log_scales"""
        if plan.n_split == 0:
            return
        c = plan.first_child
        cols = int(logs.shape[1]) if logs.dim() == 2 else 1
        z = _f32(z)
        assert means.dtype == rots.dtype == logs.dtype == torch.float32 and z.shape[0] == plan.n_into * plan.n_split
        with torch.cuda.device(means.device):
            _lib.check(_lib.load().fr_map_edit_split_children(plan.n_split, plan.n_into, cols, z.data_ptr(), means[c:].data_ptr(), rots[c:].data_ptr(),
                                                              logs[c:].data_ptr(), _stream(means.device)), "fr_map_edit_split_children")


class MapEdit:
    """remove_points / cat_params_to_optimizer / update_params_and_optimizer / prune_gaussians / densify of the reference
    (slam_external.py:203-262, 345-463) over a backend that plans and applies an edit.  `outside_mask_fn`: the
    get_gaussians_outside_mask of the caller's module, for the object-aware branch of prune_gaussians."""

    def __init__(self, backend, outside_mask_fn=None):
        self.backend = backend
        self.outside_mask_fn = outside_mask_fn

    # -- the bookkeeping: one table, one apply -------------------------------------------------------------------------------------

    @staticmethod
    def _group(optimizer, name):
        return [g for g in optimizer.param_groups if g['name'] == name][0]

    def _edit(self, plan, params, variables, optimizer, zero_stats, z=None):
        """Applies `plan` to every map parameter, to both Adam moments of each that has state, and to the statistics: carried
        (remove_points) or, with zero_stats, replaced by zeros of the new length (densify).  `timestep` is carried, zeros appended."""
        COPY, ZERO = _lib.FR_EDIT_COPY, _lib.FR_EDIT_ZERO
        keys = [k for k in params.keys() if k not in _CAM_KEYS]
        table, slots = [], []
        for k in keys:
            if optimizer is not None:
                group = self._group(optimizer, k)
                old = group['params'][0]
                state = optimizer.state.get(old, None)
            else:
                group, old, state = None, params[k], None
            table.append((old, COPY))
            if state is not None:
                table.append((state['exp_avg'], ZERO))
                table.append((state['exp_avg_sq'], ZERO))
            slots.append((k, group, old, state))
        stat_keys = [] if zero_stats else list(_STAT_KEYS)
        if zero_stats or 'timestep' in variables.keys():
            stat_keys.append('timestep')
        for k in stat_keys:
            table.append((variables[k], ZERO))
        edited = iter(self.backend.apply(plan, table))
        new = {}
        for k, group, old, state in slots:
            new[k] = (next(edited), next(edited), next(edited)) if state is not None else (next(edited),)
        if z is not None:
            self.backend.split_children(plan, z, new['means3D'][0], new['unnorm_rotations'][0], new['log_scales'][0])
        for k, group, old, state in slots:
            if optimizer is None:
                params[k] = new[k][0]
                continue
            if state is not None:
                state['exp_avg'], state['exp_avg_sq'] = new[k][1], new[k][2]
                del optimizer.state[old]
            group['params'][0] = torch.nn.Parameter(new[k][0].requires_grad_(True))
            if state is not None:
                optimizer.state[group['params'][0]] = state
            params[k] = group['params'][0]
        for k in stat_keys:
            variables[k] = next(edited)
        if zero_stats:
            like = variables['timestep']
            for k in _STAT_KEYS:
                variables[k] = torch.zeros((plan.rows,), dtype=torch.float32, device=like.device)
        # `seen` / `means2D` keep their old length, as in the reference (which notes this "implicit bug" itself)
        return params, variables

    @staticmethod
    def _rows(params):
        return int(next(v for k, v in params.items() if k not in _CAM_KEYS).shape[0])

    @staticmethod
    def _device(params):
        return next(v for k, v in params.items() if k not in _CAM_KEYS).device

    # -- the reference's functions --------------------------------------------------------------------------------------------------

    def remove_points(self, to_remove, params, variables, optimizer=None):
        P = self._rows(params)
        plan, _ = self.backend.plan(P, torch.logical_not(to_remove.reshape(-1)), None, None, 1, self._device(params))
        return self._edit(plan, params, variables, optimizer, zero_stats=False)

    @staticmethod
    def cat_params_to_optimizer(new_params, params, optimizer):
        for k, v in new_params.items():
            group = MapEdit._group(optimizer, k)
            old = group['params'][0]
            state = optimizer.state.get(old, None)
            if state is not None:
                state['exp_avg'] = torch.cat((state['exp_avg'], torch.zeros_like(v)), dim=0)
                state['exp_avg_sq'] = torch.cat((state['exp_avg_sq'], torch.zeros_like(v)), dim=0)
                del optimizer.state[old]
            group['params'][0] = torch.nn.Parameter(torch.cat((old, v), dim=0).requires_grad_(True))
            if state is not None:
                optimizer.state[group['params'][0]] = state
            params[k] = group['params'][0]
        return params

    @staticmethod
    def update_params_and_optimizer(new_params, params, optimizer):
        for k, v in new_params.items():
            group = MapEdit._group(optimizer, k)
            old = group['params'][0]
            state = optimizer.state.get(old, None)
            state['exp_avg'] = torch.zeros_like(v)              # a group without state fails here, as in the reference
            state['exp_avg_sq'] = torch.zeros_like(v)
            del optimizer.state[old]
            group['params'][0] = torch.nn.Parameter(v.requires_grad_(True))
            optimizer.state[group['params'][0]] = state
            params[k] = group['params'][0]
        return params

    def _reset_opacities(self, params, optimizer):
        x = torch.ones_like(params['logit_opacities']) * 0.01
        return self.update_params_and_optimizer({'logit_opacities': torch.log(x / (1 - x))}, params, optimizer)

    def prune_gaussians(self, params, variables, optimizer, iter, prune_dict, scene_bound=None, curr_data=None, obj_mask_2d=None):
        """One plan, one host read, one apply.  The object-aware branch (obj_mask_2d given) ORs the Gaussians that project outside
        the mask, are active (opacity >= outside_opacity_thresh) and, where asked, at least outside_max_scale big into the mask;
        the reference's progress prints are not made."""
        if iter <= prune_dict['stop_after']:
            if (iter >= prune_dict['start_after']) and (iter % prune_dict['prune_every'] == 0):
                if iter == prune_dict['stop_after']:
                    remove_threshold = prune_dict['final_removal_opacity_threshold']
                else:
                    remove_threshold = prune_dict['removal_opacity_threshold']
                big = 0.1 if iter >= prune_dict['remove_big_after'] else None
                to_remove = self.backend.prune_mask(params, remove_threshold, big)
                if obj_mask_2d is not None:
                    if self.outside_mask_fn is None:
                        raise ValueError("prune_gaussians: obj_mask_2d needs the module's get_gaussians_outside_mask (MapEditOps.install passes it)")
                    active = torch.sigmoid(params['logit_opacities']).squeeze(-1) >= prune_dict.get('outside_opacity_thresh', 0.01)
                    outside_active = self.outside_mask_fn(params, curr_data, obj_mask_2d)[0] & active
                    if 'outside_max_scale' in prune_dict:
                        outside_active = outside_active & (torch.exp(params['log_scales']).max(dim=1).values >= prune_dict['outside_max_scale'])
                    to_remove = torch.logical_or(to_remove, outside_active.reshape(-1))
                params, variables = self.remove_points(to_remove, params, variables, optimizer)
            if iter > 0 and iter % prune_dict['reset_opacities_every'] == 0 and prune_dict['reset_opacities']:
                params = self._reset_opacities(params, optimizer)
        return params, variables

    def densify(self, params, variables, optimizer, iter, densify_dict, generator=None):
        """Two stages of plan, host read and apply.  Stage 1 writes [rows that are not split, clones, n children of every split row]
        directly -- keep = not to_split, then to_clone, then to_split x n -- which is what the reference reaches by appending the
        clones, appending the children and removing the split rows (masks over the original rows suffice: see CLONE_MAX_SCALE).  The
        children's normal samples are drawn on the device (`generator`: for tests).  Stage 2 removes by opacity and size."""
        if iter <= densify_dict['stop_after']:
            variables = self.backend.accumulate(variables)
            grad_thresh = densify_dict['grad_thresh']
            if (iter >= densify_dict['start_after']) and (iter % densify_dict['densify_every'] == 0):
                to_clone, to_split = self.backend.densify_masks(params, variables, grad_thresh)
                n = densify_dict['num_to_split_into']
                if iter == densify_dict['stop_after']:
                    remove_threshold = densify_dict['final_removal_opacity_threshold']
                else:
                    remove_threshold = densify_dict['removal_opacity_threshold']
                remove_big = iter >= densify_dict['remove_big_after']
                plan, radius = self.backend.plan(self._rows(params), torch.logical_not(to_split), to_clone, to_split, n, self._device(params),
                                                 read_with=variables['scene_radius'] if remove_big else None)
                z = self.backend.randn(n * plan.n_split, params['means3D'], generator)
                params, variables = self._edit(plan, params, variables, optimizer, zero_stats=True, z=z)
                # 0.1 * scene_radius as the reference forms it: in the tensor's precision when it is one, a Python double otherwise
                big = None if not remove_big else float(0.1 * radius)
                to_remove = self.backend.prune_mask(params, remove_threshold, big)
                params, variables = self.remove_points(to_remove, params, variables, optimizer)
            if iter > 0 and iter % densify_dict['reset_opacities_every'] == 0 and densify_dict['reset_opacities']:
                params = self._reset_opacities(params, optimizer)
        return params, variables


_HIP_EDIT = MapEdit(HipMapEditBackend())
remove_points = _HIP_EDIT.remove_points
cat_params_to_optimizer = MapEdit.cat_params_to_optimizer
update_params_and_optimizer = MapEdit.update_params_and_optimizer
prune_gaussians = _HIP_EDIT.prune_gaussians
densify = _HIP_EDIT.densify
