"""The optimizer step of a Hier-SLAM iteration on our own kernels (include/hsr_optim.h); an opt-in drop-in for the reference's
torch.optim.Adam (scripts/hierslam.py:411-417, :1757) and its best-pose bookkeeping (:1814-1816, :1855-1860, :1892-1894).

    Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, ...)   torch.optim.Adam with step() as ONE launch per device (up to
                                                               HSR_ADAM_MAX_TENSORS tensors per launch) instead of seven foreach
                                                               passes; bit-identical to torch's default foreach path
    TrackingCandidate(params, time_idx)                        the tracking loop's best (loss, pose) kept on the device: update(loss)
                                                               and restore(params) never wait on the host

Adam keeps torch's non-fused state layout (state['step'] a CPU fp32 scalar tensor, exp_avg, exp_avg_sq), so slam_external's prune /
densify re-keying works unchanged and state_dict() moves freely between this class and torch.optim.Adam.  A tensor takes the kernel
when it is dense fp32 on a HIP device with param, grad and both moments of identical strides and param / grad not overlapping, in a
group with plain-number lr / betas / eps, weight_decay == 0 and amsgrad, maximize, capturable, differentiable, fused and decoupled
weight decay off (and foreach not explicitly False).  Every other tensor goes through torch's own functional adam() with its
group's settings, in the same step().
"""
import numbers

import torch
from torch.optim.adam import adam as _torch_adam
from torch.optim.optimizer import _get_scalar_dtype

from diff_gaussian_rasterization import _abi

_lib = _abi.lib
_AdamTensor = _abi.hsr_adam_tensor


def _dense(t):
    """non-overlapping and dense: the numel elements fill one contiguous span of memory, in some order of the dimensions"""
    if t.numel() == 0:
        return True
    expect = 1
    for st, sz in sorted((st, sz) for sz, st in zip(t.shape, t.stride()) if sz != 1):
        if st != expect:
            return False
        expect *= sz
    return True


def _group_takes_kernel(group):
    beta1, beta2 = group["betas"]
    plain = all(isinstance(x, numbers.Real) and not isinstance(x, bool) for x in (group["lr"], beta1, beta2, group["eps"]))
    return (plain and group["weight_decay"] == 0 and not group["amsgrad"] and not group["maximize"] and not group["capturable"]
            and not group["differentiable"] and not group.get("fused") and not group.get("decoupled_weight_decay", False)
            and group.get("foreach") is not False)


def _tensor_takes_kernel(p, grad):
    if not (p.is_cuda and p.dtype == torch.float32 and grad.dtype == torch.float32 and grad.device == p.device
            and not grad.is_sparse and p.layout == torch.strided and grad.layout == torch.strided):
        return False
    if p.stride() != grad.stride() or not _dense(p):
        return False
    n = p.numel() * 4
    a, b = p.data_ptr(), grad.data_ptr()
    return n == 0 or a + n <= b or b + n <= a


class Adam(torch.optim.Adam):
    """torch.optim.Adam whose step() runs hsr_adam_step for every eligible tensor (module docstring).  Same constructor, param_groups
    and state.  After each step, `last_fused_tensors` / `last_fused_numel` say how many tensors / elements took the kernel."""

    last_fused_tensors = 0
    last_fused_numel = 0

    def _torch_step(self, group, params):
        """torch.optim.Adam.step for `params` (a subset of group['params']) with the group's settings"""
        sub = dict(group)
        sub["params"] = params
        p_, g_, m_, v_, vmax_, steps_ = [], [], [], [], [], []
        has_complex = self._init_group(sub, p_, g_, m_, v_, vmax_, steps_)
        beta1, beta2 = group["betas"]
        _torch_adam(p_, g_, m_, v_, vmax_, steps_, amsgrad=group["amsgrad"], has_complex=has_complex, beta1=beta1, beta2=beta2,
                    lr=group["lr"], weight_decay=group["weight_decay"], eps=group["eps"], maximize=group["maximize"],
                    foreach=group["foreach"], capturable=group["capturable"], differentiable=group["differentiable"],
                    fused=group["fused"], grad_scale=getattr(self, "grad_scale", None), found_inf=getattr(self, "found_inf", None),
                    decoupled_weight_decay=group["decoupled_weight_decay"])

    @torch.no_grad()
    def step(self, closure=None):
        self._cuda_graph_capture_health_check()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        tables = {}        # device -> [_AdamTensor]; the tensors are kept alive by the state and the params until the launch
        fused_numel = 0
        for group in self.param_groups:
            kernel_group = _group_takes_kernel(group)
            rest = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
                if not (kernel_group and _tensor_takes_kernel(p, p.grad)):
                    rest.append(p)
                    continue
                state = self.state[p]
                if len(state) == 0:   # torch's lazy initialisation (non-fused, non-capturable: the step lives on the CPU)
                    state["step"] = torch.tensor(0.0, dtype=_get_scalar_dtype())
                    state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                m, v = state["exp_avg"], state["exp_avg_sq"]
                if not all(t.dtype == torch.float32 and t.device == p.device and t.stride() == p.stride() for t in (m, v)) \
                        or state["step"].is_cuda:
                    rest.append(p)   # state from elsewhere (a loaded state_dict of another layout): torch handles it
                    continue
                state["step"] += 1
                step = state["step"].item()   # CPU tensor: no device synchronisation
                beta1, beta2 = group["betas"]
                lr = group["lr"]
                # torch's foreach path (torch/optim/adam.py, _multi_tensor_adam, capturable=False), in double, cast to float by ctypes
                bc1 = 1 - beta1 ** step
                bc2 = 1 - beta2 ** step
                tables.setdefault(p.device, []).append(_AdamTensor(
                    p.data_ptr(), p.grad.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), (lr / bc1) * -1, bc2 ** 0.5,
                    group["eps"], 1 - beta1, beta2, 1 - beta2))
                fused_numel += p.numel()
            if rest:
                self._torch_step(group, rest)
        for dev, entries in tables.items():
            arr = (_AdamTensor * len(entries))(*entries)
            _abi.call(_lib.hsr_adam_step, "hsr_adam_step", dev, len(entries), arr)
        self.last_fused_tensors = sum(len(e) for e in tables.values())
        self.last_fused_numel = fused_numel
        return loss


class TrackingCandidate:
    """The best camera pose of one tracking frame, kept on the device (scripts/hierslam.py:1814-1816, :1855-1860, :1892-1894).

        cand = TrackingCandidate(params, time_idx)     clones column time_idx of cam_unnorm_rots / cam_trans; best loss 1e20
        cand.update(loss)                              after optimizer.step(): if loss < best, keep loss and the post-step pose
        cand.restore(params)                           after the loop: write the kept pose back into column time_idx

    update() reads params['cam_unnorm_rots'] / ['cam_trans'] from the dict given to the constructor at the time of the call.  Both
    calls run on the current stream and never read a device value on the host.  A NaN loss keeps the old candidate."""

    def __init__(self, params, time_idx):
        rots, trans = params["cam_unnorm_rots"], params["cam_trans"]
        for name, t, rows in (("cam_unnorm_rots", rots, 4), ("cam_trans", trans, 3)):
            if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 3 and tuple(t.shape[:2]) == (1, rows) and t.is_contiguous()):
                raise RuntimeError("TrackingCandidate: %s must be a contiguous fp32 [1,%d,T] tensor on a HIP device (got %s %s on %s)"
                                   % (name, rows, t.dtype, tuple(t.shape), t.device))
        if not 0 <= time_idx < rots.shape[2] or trans.shape[2] != rots.shape[2]:
            raise RuntimeError("TrackingCandidate: time_idx %d outside [0, %d)" % (time_idx, rots.shape[2]))
        self._params = params
        self.time_idx = int(time_idx)
        self.cam_unnorm_rot = rots[..., time_idx].detach().clone()
        self.cam_tran = trans[..., time_idx].detach().clone()
        self.best_loss = torch.full((), 1e20, dtype=torch.float32, device=rots.device)

    def update(self, loss):
        rots, trans = self._params["cam_unnorm_rots"], self._params["cam_trans"]
        loss = loss.detach()
        if not (loss.numel() == 1 and loss.dtype == torch.float32 and loss.device == self.best_loss.device):
            raise RuntimeError("TrackingCandidate.update: the loss must be one fp32 value on %s (got %s %s on %s)"
                               % (self.best_loss.device, loss.dtype, tuple(loss.shape), loss.device))
        if not (rots.is_contiguous() and trans.is_contiguous() and rots.device == loss.device and trans.device == loss.device):
            raise RuntimeError("TrackingCandidate.update: cam_unnorm_rots / cam_trans must stay contiguous on %s" % loss.device)
        _abi.call(_lib.hsr_track_keep_best, "hsr_track_keep_best", loss.device, rots.shape[2], self.time_idx, loss.data_ptr(),
                  self.best_loss.data_ptr(), rots.data_ptr(), trans.data_ptr(), self.cam_unnorm_rot.data_ptr(), self.cam_tran.data_ptr())

    @torch.no_grad()
    def restore(self, params):
        params["cam_unnorm_rots"][..., self.time_idx] = self.cam_unnorm_rot
        params["cam_trans"][..., self.time_idx] = self.cam_tran
