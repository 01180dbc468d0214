"""FusedAdam: torch.optim.Adam whose step is one launch of fr_adam_step (csrc/fr_adam.hip) over the table of every parameter that
has a gradient, over all groups -- the reference builds its optimizer as seven groups of one tensor each, which torch steps one
after the other as a chain of about a dozen element-wise launches per group.

The state is torch's own: state[p] = {'step': CPU float tensor, 'exp_avg', 'exp_avg_sq'}, so the map edit
(models/SLAM/utils/slam_external.MapEdit), state_dict() / load_state_dict() and a plain torch.optim.Adam keep working on it.

Observable differences from torch.optim.Adam:
  * the arithmetic is csrc/fr_adam_math.h: binary32, a fixed operand order, no contraction.  torch's own kernels contract inside
    lerp / addcmul / addcdiv (differently on the CPU and on the GPU), so the last bits differ from torch's;
  * `skip_frozen=True` (off by default) leaves the parameters of groups with lr == 0 out of the step: they get no state, their step
    is not counted, and a non-finite gradient no longer reaches them (torch adds -0 x NaN to a frozen parameter);
  * anything outside the fused subset sends the whole step to torch.optim.Adam.step: amsgrad, maximize, weight decay, capturable,
    differentiable, fused, an lr or beta that is a tensor, a parameter or gradient that is not a dense contiguous float32 tensor
    on the backend's one device.
"""
import ctypes

import torch

from . import _lib

try:
    from torch.optim.optimizer import _get_scalar_dtype
except ImportError:                                          # an older torch: the step count is a float32 tensor there
    def _get_scalar_dtype():
        return torch.float32


class HipAdamBackend:
    """fr_adam_step on the current torch stream of the tensors' device, one launch per FR_ADAM_MAX_ARRAYS entries"""

    @staticmethod
    def accepts(t):
        return t.is_cuda

    @staticmethod
    def step(entries):
        """entries: [(param, grad, exp_avg, exp_avg_sq, (w1, beta2, c2, bc2_sqrt, eps, neg_step_size), fresh), ...]"""
        lib = _lib.load()
        if not hasattr(lib, "fr_adam_step"):
            raise _lib.FisherRastError("libfisher_rast.so has no fr_adam_step: rebuild it")
        dev = entries[0][0].device
        table = [_lib.AdamArray(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), *c, int(fresh)) for p, g, m, v, c, fresh in entries]
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            for i in range(0, len(table), _lib.FR_ADAM_MAX_ARRAYS):
                chunk = table[i:i + _lib.FR_ADAM_MAX_ARRAYS]
                _lib.check(lib.fr_adam_step((_lib.AdamArray * len(chunk))(*chunk), len(chunk), stream), "fr_adam_step")


class FusedAdam(torch.optim.Adam):
    """torch.optim.Adam's constructor plus `skip_frozen` and `backend` (default: the HIP library; a test passes a CPU backend over
    the g++ build of csrc/fr_adam_math.h)."""

    def __init__(self, params, *args, skip_frozen=False, backend=None, **kwargs):
        super().__init__(params, *args, **kwargs)
        self.skip_frozen = bool(skip_frozen)
        self.backend = backend if backend is not None else HipAdamBackend()

    def _fused_subset(self):
        """the (group, parameter) pairs of this step, or None when something is outside the fused subset"""
        work, device = [], None
        for group in self.param_groups:
            if (group["amsgrad"] or group["maximize"] or group["weight_decay"] != 0 or group["capturable"] or group["differentiable"]
                    or group["fused"] or not isinstance(group["lr"], (int, float)) or not all(isinstance(b, (int, float)) for b in group["betas"])):
                return None
            for p in group["params"]:
                g = p.grad
                if g is None:
                    continue
                for t in (p, g):
                    if t.dtype != torch.float32 or t.layout != torch.strided or not t.is_contiguous() or not self.backend.accepts(t):
                        return None
                    if device is None:
                        device = t.device
                    if t.device != device:
                        return None
                state = self.state.get(p, None)
                if state and not (torch.is_tensor(state.get("step")) and state["step"].device.type == "cpu"
                                  and all(torch.is_tensor(state.get(k)) and state[k].dtype == torch.float32 and state[k].is_contiguous()
                                          and state[k].device == device and state[k].shape == p.shape for k in ("exp_avg", "exp_avg_sq"))):
                    return None
                if not (self.skip_frozen and group["lr"] == 0):
                    work.append((group, p))
        return work

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = self._fused_subset()
        if work is None:
            fallback = torch.optim.Adam.step
            if getattr(fallback, "hooked", False):           # this step's own wrapper runs the step hooks: not twice
                fallback = fallback.__wrapped__
            fallback(self)
            return loss
        entries = []
        for group, p in work:
            state = self.state[p]
            fresh = len(state) == 0
            if fresh:
                state["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())
                state["exp_avg"] = torch.empty_like(p, memory_format=torch.preserve_format)        # written, not read, by the first step
                state["exp_avg_sq"] = torch.empty_like(p, memory_format=torch.preserve_format)
            state["step"] += 1
            # torch/optim/adam.py, the non-capturable branch: Python doubles, each rounded once to binary32 on the way into the table
            step = state["step"].item()
            beta1, beta2 = group["betas"]
            bias_correction1 = 1 - beta1 ** step
            bias_correction2 = 1 - beta2 ** step
            step_size = group["lr"] / bias_correction1
            bias_correction2_sqrt = bias_correction2 ** 0.5
            coeffs = (1 - beta1, beta2, 1 - beta2, bias_correction2_sqrt, group["eps"], -step_size)
            entries.append((p, p.grad, state["exp_avg"], state["exp_avg_sq"], coeffs, fresh))
        if entries:
            self.backend.step(entries)
        return loss
