"""
Optimizer step on the device in one launch.

`Adam` is a drop-in for the reference's `torch.optim.Adam(net.parameters(), lr)` (exp.py:89): same
constructor arguments, same `param_groups` (so `ReduceLROnPlateau`, exp.py:91-98, drives `lr` unchanged),
same `state_dict()` layout (`step`, `exp_avg`, `exp_avg_sq` per parameter) — a checkpoint of one loads into
the other.  The arithmetic is torch's default Adam path operation by operation (csrc/optim.hip); `step`
needs no host round trip.  amsgrad / maximize / capturable variants are not part of the reference's use and
raise.

`Adam(..., max_grad_norm=c)` clips the gradients by their global 2-norm inside that step (csrc/gradclip.hip): one
norm over the gradients of all parameter groups, accumulated in double in a fixed order on the device, the
coefficient min(c / (norm + 1e-6), 1) folded into the Adam kernel's read of the gradient (which is never rewritten),
and a step whose norm is not finite skipped on the device.  `clip_grad_norm_` is the standalone form for callers that
keep another optimizer.
"""
import ctypes
import math
import numbers

import torch

from ._capi import check, lib
from .functional import _stream, status_word


def _check_max_norm(value, what):
    """A positive number or +inf, as a float; anything else is a ValueError."""
    if isinstance(value, bool) or not isinstance(value, numbers.Real) or not value > 0:  # (NaN > 0 is False)
        raise ValueError(f"{what}: a positive number or float('inf'), got {value!r}")
    return float(value)


def _tables(tensors):
    """(array of device pointers, array of element counts) of a list of contiguous tensors (None: NULL, 0)."""
    n = len(tensors)
    return ((ctypes.c_void_p * max(n, 1))(*[None if t is None or t.numel() == 0 else t.data_ptr() for t in tensors]),
            (ctypes.c_int64 * max(n, 1))(*[0 if t is None else t.numel() for t in tensors]))


def _grad_norm(grads, max_norm, clip, ws, tensor_norms=None, skip=None):
    """sparch_grad_norm on a list of contiguous fp32 device tensors."""
    a_g, a_n = _tables(grads)
    check(lib.sparch_grad_norm(len(grads), a_g, a_n, float(max_norm), ws.data_ptr() if ws.numel() else None,
                               ws.numel() * 8, clip.data_ptr(), None if tensor_norms is None else tensor_norms.data_ptr(),
                               None if skip is None else skip.data_ptr(), _stream()), "sparch_grad_norm")


def _ws_doubles(numels):
    n = len(numels)
    return (int(lib.sparch_grad_norm_ws_bytes(n, (ctypes.c_int64 * max(n, 1))(*numels))) + 7) // 8


def _norm_of(clip):
    """Word 0 of a clip state as a 0-d fp32 tensor (a view: no copy, no sync)."""
    return clip[:1].view(torch.float32)[0]


def clip_grad_norm_(parameters, max_norm, tensor_norms=False):
    """torch.nn.utils.clip_grad_norm_ (2-norm) for fp32 gradients on the GPU, without a host round trip: the norm is
    accumulated in double in a fixed order (the same gradients give the same bits on every call and every replica) and
    the gradients are scaled in place by min(max_norm / (norm + 1e-6), 1).  Returns the norm as a 0-d device tensor;
    with tensor_norms=True also each gradient's own norm, in the order of `parameters` (those without a gradient left
    out).  Unlike torch, a NaN or inf norm leaves the gradients UNTOUCHED (torch multiplies all of them by NaN): the
    caller sees it in the returned norm.  max_norm may be float('inf'): measure only."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    max_norm = _check_max_norm(max_norm, "clip_grad_norm_: max_norm")
    grads = [p.grad for p in parameters if p.grad is not None]
    for g in grads:
        if g.dtype != torch.float32 or not g.is_cuda or g.is_sparse or not g.is_contiguous():
            raise RuntimeError("sparch_amd.optim.clip_grad_norm_: contiguous float32 dense gradients on the GPU only")
    dev = grads[0].device if grads else torch.device("cuda")
    clip = torch.zeros(8, dtype=torch.int32, device=dev)
    ws = torch.empty(_ws_doubles([g.numel() for g in grads]), dtype=torch.float64, device=dev)
    per = torch.empty(len(grads), dtype=torch.float32, device=dev) if tensor_norms else None
    _grad_norm(grads, max_norm, clip, ws, per)
    a_g, a_n = _tables(grads)
    check(lib.sparch_scale_grads(len(grads), a_g, a_n, clip.data_ptr(), _stream()), "sparch_scale_grads")
    return (_norm_of(clip), per) if tensor_norms else _norm_of(clip)


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False,
                 max_grad_norm=None):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if amsgrad:
            raise NotImplementedError("sparch_amd.optim.Adam: amsgrad is not implemented (the reference does not use it)")
        # None: no clipping, the same C calls as ever.  A positive number or inf (measure, and skip non-finite steps,
        # without scaling): ONE global norm per step() over all groups, every launch through sparch_adam_step_clip.
        self.max_grad_norm = None if max_grad_norm is None else _check_max_norm(max_grad_norm, "Invalid max_grad_norm")
        self._clip = None           # {"state": 8 words, "ws": doubles}: made once, the workspace grown with the parameters
        self._clip_taken_back = 0   # how much of state[3] sync_skipped() has passed to take_back()
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False))
        # Steps the device skipped after a persistent kernel's timeout (status word raised: sparch_adam_step is a
        # no-op and counts itself in status[1]) are taken back from the bias-correction counters when the host
        # reads the word, so that "a skipped step is a no-op" also holds for t in 1 - beta^t.
        import weakref

        from . import functional as _Fn
        ref = weakref.ref(self)

        def _on_timeout(info, ref=ref):
            opt = ref()
            if opt is None:
                _Fn._timeout_listeners.remove(_on_timeout)
            else:
                opt.take_back(info["skipped_steps"])
        _Fn._timeout_listeners.append(_on_timeout)

    def take_back(self, n):
        """Undo the step-counter advance of `n` optimizer steps that were no-ops on the device."""
        if n <= 0:
            return
        for group in self.param_groups:
            for p in group["params"]:
                st = self.state.get(p)
                if st and "step" in st:
                    st["step"] -= min(float(n), float(st["step"]))
        g = getattr(self, "_g", None)
        if g is not None:
            g["t"].sub_(float(n)).clamp_(min=0.0)

    def _clip_buffers(self, numels, dev):
        """The clip state and a workspace for gradients of these sizes.  Everything per-step lives in them, on the
        device; nothing is allocated once they fit, so a captured step replays on the same memory."""
        need = _ws_doubles(numels)
        if self._clip is None:
            self._clip = {"state": torch.zeros(8, dtype=torch.int32, device=dev),
                          "ws": torch.empty(need, dtype=torch.float64, device=dev)}
        elif self._clip["ws"].numel() < need:
            self._clip["ws"] = torch.empty(need, dtype=torch.float64, device=dev)
        return self._clip

    def _clip_norm(self, ps):
        """ONE norm over the gradients of `ps` (all groups' parameters that have one); returns the clip state."""
        c = self._clip_buffers([p.numel() for p in ps], ps[0].device)
        _grad_norm([self._grad(p) for p in ps], self.max_grad_norm, c["state"], c["ws"], skip=status_word(ps[0].device))
        return c["state"]

    @staticmethod
    def _grad(p):
        return p.grad if p.grad.is_contiguous() else p.grad.contiguous()

    @staticmethod
    def _check_param(p):
        if p.dtype != torch.float32 or not p.is_cuda or p.grad.is_sparse:
            raise RuntimeError("sparch_amd.optim.Adam: float32 dense parameters on the GPU only")

    def clip_stats(self):
        """The clip state read back (one sync): the last step's norm, coefficient and non-finite flag, and since the
        optimizer was made (or reset_clip_stats()) the finite steps, how many of them were clipped, the steps skipped
        for a non-finite norm and the largest finite norm."""
        if self.max_grad_norm is None:
            raise RuntimeError("sparch_amd.optim.Adam.clip_stats: the optimizer was made without max_grad_norm")
        if self._clip is None:
            return dict(norm=0.0, coef=1.0, nonfinite=False, skipped=0, steps=0, clipped=0, max_norm=0.0)
        w = self._clip["state"].cpu()
        f = w.view(torch.float32)
        return dict(norm=float(f[0]), coef=float(f[1]), nonfinite=bool(w[2]), skipped=int(w[3]), steps=int(w[4]),
                    clipped=int(w[5]), max_norm=float(f[6]))

    def reset_clip_stats(self):
        """Zero the counters (after sync_skipped(): steps it has not seen yet would be forgotten)."""
        if self._clip is not None:
            self.sync_skipped()
            self._clip["state"].zero_()
            self._clip_taken_back = 0

    def sync_skipped(self):
        """One host read: the steps the device skipped for a non-finite gradient norm since the last call are taken
        back from the bias-correction counters (take_back, as after a kernel timeout).  Returns their number."""
        if self._clip is None:
            return 0
        skipped = int(self._clip["state"][3])
        n, self._clip_taken_back = skipped - self._clip_taken_back, skipped
        self.take_back(n)
        return n

    def enable_graph_mode(self):
        """Keep the per-step factors (lr / (1 - beta1^t), sqrt(1 - beta2^t)) in DEVICE memory, computed by a few
        captured torch ops from a device step counter, so that `step()` can be part of a HIP graph (kernel
        arguments are frozen at capture time).  The arithmetic is the same double-precision formula the host
        path evaluates; `lr` is read from a device scalar that `step()` refreshes whenever the scheduler changed
        the group's value.  One parameter group stepping together (the reference's use)."""
        if len(self.param_groups) != 1:
            raise NotImplementedError("sparch_amd.optim.Adam graph mode: one parameter group")
        group = self.param_groups[0]
        dev = group["params"][0].device
        t0 = 0.0
        for p in group["params"]:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            t0 = float(st["step"])
        self._g = {"t": torch.full((), t0, dtype=torch.float64, device=dev),
                   "lr": torch.full((), float(group["lr"]), dtype=torch.float64, device=dev),
                   "lr_host": float(group["lr"]),
                   "scalars": torch.zeros(2, dtype=torch.float32, device=dev)}
        if self.max_grad_norm is not None:  # made now, for every parameter: nothing is allocated inside a capture
            self._clip_buffers([p.numel() for p in group["params"]], dev)

    def sync_lr(self):
        """Graph mode, outside the captured region: push a learning rate changed by the scheduler."""
        g = getattr(self, "_g", None)
        if g is not None and float(self.param_groups[0]["lr"]) != g["lr_host"]:
            g["lr_host"] = float(self.param_groups[0]["lr"])
            g["lr"].fill_(g["lr_host"])

    def note_replay(self):
        """Graph mode: a replay advanced the device step counter; keep the host-side `step` entries in step."""
        for p in self.param_groups[0]["params"]:
            if p in self.state:
                self.state[p]["step"] += 1

    @torch.no_grad()
    def step(self, closure=None):
        if getattr(self, "_g", None) is not None:
            return self._step_graph_mode()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        clip = None
        if self.max_grad_norm is not None:
            every = [p for group in self.param_groups for p in group["params"] if p.grad is not None]
            for p in every:
                self._check_param(p)
            if every:
                clip = self._clip_norm(every)
        for group in self.param_groups:
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            beta1, beta2 = group["betas"]
            steps = set()
            for p in ps:
                self._check_param(p)
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)  # host scalar, as torch.optim.Adam keeps it
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                steps.add(float(st["step"]))
            # parameters that joined at different times step separately (never the case in the reference's use)
            for t in sorted(steps):
                sel = [p for p in ps if float(self.state[p]["step"]) == t]
                bc1 = 1.0 - beta1 ** t
                bc2 = 1.0 - beta2 ** t
                self._launch(sel, group["lr"] / bc1, beta1, beta2, math.sqrt(bc2), group["eps"], group["weight_decay"],
                             clip=clip)
        return loss

    def _step_graph_mode(self):
        group, g = self.param_groups[0], self._g
        ps = [p for p in group["params"] if p.grad is not None]
        beta1, beta2 = group["betas"]
        check(lib.sparch_adam_scalars(g["t"].data_ptr(), g["lr"].data_ptr(), float(beta1), float(beta2),
                                      g["scalars"].data_ptr(), _stream()), "sparch_adam_scalars")
        if not torch.cuda.is_current_stream_capturing():
            self.note_replay()
        clip = self._clip_norm(ps) if self.max_grad_norm is not None and ps else None
        self._launch(ps, 0.0, beta1, beta2, 1.0, group["eps"], group["weight_decay"], scalars=g["scalars"], clip=clip)
        return None

    def _launch(self, ps, step_size, beta1, beta2, bc2_sqrt, eps, weight_decay, scalars=None, clip=None):
        n = len(ps)
        arr = ctypes.c_void_p * n
        grads = [self._grad(p) for p in ps]
        for p in ps:
            if not p.is_contiguous():
                raise RuntimeError("sparch_amd.optim.Adam: parameters must be contiguous")
        a_p = arr(*[p.data_ptr() for p in ps])
        a_g = arr(*[g.data_ptr() for g in grads])
        a_m = arr(*[self.state[p]["exp_avg"].data_ptr() for p in ps])
        a_v = arr(*[self.state[p]["exp_avg_sq"].data_ptr() for p in ps])
        a_n = (ctypes.c_int64 * n)(*[p.numel() for p in ps])
        # guarded by the recurrent kernels' status word: after an in-kernel timeout (invalid gradients) the
        # step is a no-op on the device until check_status() has reported it and cleared the word
        skip = status_word(ps[0].device)
        if clip is not None:
            check(lib.sparch_adam_step_clip(n, a_p, a_g, a_m, a_v, a_n, float(step_size), float(beta1), float(beta2),
                                            float(bc2_sqrt), float(eps), float(weight_decay),
                                            scalars.data_ptr() if scalars is not None else None, skip.data_ptr(),
                                            clip.data_ptr(), _stream()), "sparch_adam_step_clip")
            return
        check(lib.sparch_adam_step(n, a_p, a_g, a_m, a_v, a_n, float(step_size), float(beta1), float(beta2),
                                   float(bc2_sqrt), float(eps), float(weight_decay),
                                   scalars.data_ptr() if scalars is not None else None, skip.data_ptr(), _stream()),
              "sparch_adam_step")
