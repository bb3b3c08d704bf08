"""
Host orchestration of the HIP hot path: one torch.autograd.Function per layer type.

Each Function replaces the eager op chain of a reference layer's forward
(snns.py:249-280 / 386-417 / 521-552 / 663-694 for the spiking layers, 793-806 for the
readout) and the autograd tape replay behind `loss.backward()` (exp.py:376) with a fixed
sequence of libsparch_hip.so calls on the current HIP stream.  PyTorch here only owns
device memory, the stream and the autograd graph edges between layers.

No CPU fallback: CPU tensors raise.
"""
import ctypes
import os
import typing

import torch

from . import _capi
from ._capi import KIND, check, lib, ptr

# Dense GEMMs: "split6" = exact 6-term bf16 split on the bf16 MFMA (default), "fp32" = fp32-input MFMA.
DENSE_GEMM = os.environ.get("SPARCH_DENSE_GEMM", "split6")

# The gradient of a BatchNorm'd projection may leave the BatchNorm pass as its three exact bf16 planes (made once) so
# that the dX / dW products read planes instead of re-splitting the fp32 tensor in every workgroup that stages a tile
# of it; results are bit-identical either way.  Measured (round 3, A/B in one call): at the headline shape the
# products do not get faster for it (dX 0.69 -> 0.67 ms, dW unchanged: conversion VALU is NOT what bounds them) and
# the pass writes half as much again (0.125 -> 0.165 ms): 6.58 -> 6.63 ms per step.  For a BIDIRECTIONAL layer the
# same pass also adds the two directions' gradients (no separate sparch_add_halves pass): cfg5 76.1 -> 74.7 ms.
# Hence "auto" = bidirectional layers only; SPARCH_DX_PLANES=1 / 0 forces it on / off.
USE_DX_PLANES = {"1": True, "0": False}.get(os.environ.get("SPARCH_DX_PLANES", "auto"), "auto")

# Saved states (u, w) of the spiking layers in bf16 instead of fp32 (SPARCH_SAVE_DTYPE=bf16; BASELINE configs[4]
# is the long-sequence bf16 case: at T=1000 the fp32 saves are 4.2 GB per layer and direction pair).  Every
# discrete decision of the backward pass stays exactly the fp32 one (csrc/common.h save_u16), so spikes, dWx, dW
# and dV do not change; dalpha / dbeta / da see the 2^-9 rounding of u and w: stated tolerance 2e-2 of max-abs
# against the fp32 path (tests/test_hip_parity.py::test_bf16_saved_states_*).  Off by default.
SAVE_BF16 = os.environ.get("SPARCH_SAVE_DTYPE", "fp32").lower() == "bf16"

# Operand precision of every matrix product (include/sparch_hip.h sparch_set_operand_precision): "fp32" = exact
# bf16 splits of fp32 operands (default, fp32 results), "bf16" = operands rounded once to bf16, fp32
# accumulation, fp32 states / statistics / parameter updates (BASELINE configs[4]; SPARCH_COMPUTE_DTYPE=bf16 or
# run_exp.py --compute_dtype bf16).  Stated tolerance against the fp32 path: tests/test_hip_parity.py
# ::test_bf16_operand_mode_*.
COMPUTE_DTYPES = {"fp32": 0, "bf16": 1}


_precision = 0  # what this module passes as the `precision` argument of every matrix-product call (the C library
#                keeps no such state since ABI v5: include/sparch_hip.h)


def set_compute_dtype(name):
    """Select the operand precision this module asks of the library's matrix products; returns the previous
    setting's name."""
    global _precision
    name = {"float32": "fp32", "f32": "fp32", "bfloat16": "bf16"}.get(str(name).lower(), str(name).lower())
    if name not in COMPUTE_DTYPES:
        raise ValueError(f"compute dtype must be one of {sorted(COMPUTE_DTYPES)}, got {name!r}")
    prev = compute_dtype()
    _precision = COMPUTE_DTYPES[name]
    return prev


def compute_dtype():
    return "bf16" if _precision == 1 else "fp32"


def _prec():
    return _precision


if os.environ.get("SPARCH_COMPUTE_DTYPE"):
    set_compute_dtype(os.environ["SPARCH_COMPUTE_DTYPE"])

SEED_IN_MEMORY = 1 << 63  # include/sparch_hip.h SPARCH_SEED_IN_MEMORY: the seed argument carries a device address

BN_MOMENTUM = 0.05  # snns.py:240
# SyncBN for data-parallel runs (off by default = standard DDP semantics: per-rank statistics).
# {"group": process group or None, "world": n}: BatchNorm then normalises with the statistics of the GLOBAL
# batch — forward: every rank's per-tile (sum x, sum x^2) partials are all-gathered and finished in one pass
# (same fp64 reduction as the single-device path, so world ranks x B/world rows reproduce one device with B
# rows up to summation order); backward: (sum dy, sum dy*xhat) are all-reduced for dx, the affine
# parameters' own gradients stay local sums (the gradient all-reduce averages them like every other one).
SYNC_BN = None
NORM_EPS = 1e-5
# BatchNorm over at most this many rows takes its statistics from exact column sums of the projection
# (sparch_bn_colstat_exact) instead of the GEMM epilogue's fp32 partials, whose E[x^2] - mean^2 loses
# log2((mean^2 + var) / var) bits: the baselines' readout normalises softmax sums over the batch alone, where that
# ratio reaches 3e4.  Above it the second read of the projection would cost what the epilogue saves.
BN_EXACT_ROWS = 1024

ALPHA_LIM = (0.8187307530779818, 0.9607894391523232)  # exp(-1/5), exp(-1/25)   snns.py:229
BETA_LIM = (0.9672161004820059, 0.9917012926388759)  # exp(-1/30), exp(-1/120)  snns.py:357
A_LIM = (-1.0, 1.0)  # snns.py:358
B_LIM = (0.0, 2.0)  # snns.py:359

_status = {}

# Objects with pre_persistent() / post_persistent(), called right before / right behind every persistent recurrent
# launch (kernels whose workgroups wait for each other and need the whole GPU): sparch_amd.dp's "window" policy
# keeps its collectives out of those kernels' way with them.
persistent_hooks = []


class _persistent_launch:
    """with _persistent_launch(): <enqueue one persistent kernel>"""

    def __enter__(self):
        for h in persistent_hooks:
            h.pre_persistent()

    def __exit__(self, *exc):
        if exc[0] is None:
            for h in persistent_hooks:
                h.post_persistent()
        return False



class KernelTimer:
    """Optional HIP-event timing of named C-ABI calls on the current stream (bench.py uses it for
    the roofline object).  Disabled by default: zero overhead on the training path."""

    def __init__(self):
        self.enabled = False
        self.pending = []   # (name, start_event, end_event)
        self.totals = {}    # name -> [count, total_ms]

    def start(self, name):
        if not self.enabled:
            return None
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        return (name, a, b)

    def stop(self, tok):
        if tok is not None:
            tok[2].record()
            self.pending.append(tok)

    def collect(self):
        torch.cuda.synchronize()
        for name, a, b in self.pending:
            c = self.totals.setdefault(name, [0, 0.0])
            c[0] += 1
            c[1] += a.elapsed_time(b)
        self.pending = []
        return self.totals

    def reset(self):
        self.pending, self.totals = [], {}


timer = KernelTimer()


def _require_device(t, what):
    if not t.is_cuda:
        raise RuntimeError(
            f"sparch_amd: {what} is on '{t.device}'. The MI355X path has no CPU fallback; "
            "move the model and inputs to a HIP device (.to('cuda'))."
        )


def _stream():
    return torch.cuda.current_stream().cuda_stream


def status_word(device):
    """Per-device uint32 raised by a recurrent kernel whose in-kernel wait timed out."""
    key = torch.device(device).index or 0
    if key not in _status:
        _status[key] = torch.zeros(4, dtype=torch.int32, device=device)
    return _status[key]


_TIMEOUT_TEXT = (
    "recurrent cell kernel: in-kernel wait timed out (SPARCH_ETIMEOUT).  The persistent kernels need one "
    "workgroup per CU resident at the same time; if the GPU is shared with another process (or partitioned) "
    "they cannot all become resident.  The results of the affected step are invalid (the optimizer step and "
    "the BatchNorm running statistics skip themselves on the device while the status word is raised).")
_degraded = set()  # device indices whose recurrent kernels now run one launch per time step


STATUS_KERNELS = {0: "?", 1: "rec_fwd (RLIF / RadLIF forward)", 2: "rec_bwd (RLIF / RadLIF backward)",
                  3: "ann_rec forward (RNN)", 4: "ann_rec backward (RNN)", 5: "ligru forward", 6: "ligru backward",
                  7: "gru forward", 8: "gru backward"}  # include/sparch_hip.h SPARCH_STATUS_*
last_timeout = None   # details of the most recent timeout poll_status() saw: dict(kernel, step, skipped_steps)
_timeout_listeners = []  # callables(info) — e.g. the optimizer takes its step counter back by info["skipped_steps"]


def poll_status(device="cuda"):
    """Synchronising read of the persistent-kernel status word (4 x uint32: raised, optimizer steps skipped since,
    kernel id, time step); clears it.  True = a wait timed out; the details are left in `last_timeout` and handed
    to the registered listeners."""
    global last_timeout
    w = status_word(device)
    vals = w.tolist()
    if vals[0] != 0:
        w.zero_()
        step = vals[3] & 0xFFFFFFFF
        last_timeout = {"kernel": STATUS_KERNELS.get(vals[2], f"kernel id {vals[2]}"),
                        "step": None if step == 0xFFFFFFFF else step, "skipped_steps": int(vals[1]),
                        "device": str(w.device)}
        for fn in list(_timeout_listeners):
            fn(last_timeout)
        return True
    return False


def describe_timeout():
    """One line about the most recent timeout (which kernel, which time step, how many optimizer steps were skipped)."""
    if last_timeout is None:
        return "no timeout recorded"
    t = last_timeout
    import os as _os
    rank = _os.environ.get("RANK")
    return (f"{'rank ' + rank + ', ' if rank is not None else ''}{t['device']}: {t['kernel']} gave up"
            f"{'' if t['step'] is None else ' at time step ' + str(t['step'])}; "
            f"{t['skipped_steps']} optimizer step(s) were skipped on the device since")


def degrade(device="cuda"):
    """From now on this process runs the recurrent cells with one launch per time step on `device` (nothing
    waits inside a launch, any CU share works).  New launches only — the process is never re-executed."""
    _degraded.add(torch.device(device).index or 0)


def check_status(device="cuda", on_timeout="raise"):
    """Synchronising check of the persistent-kernel status word (call at a sync point).
    on_timeout = "raise": SparchHipError.  "degrade": switch this process to one launch per time step
    (see `degrade`) and return True, so that a trainer can log the lost step and carry on."""
    if not poll_status(device):
        return False
    if on_timeout == "degrade":
        degrade(device)
        return True
    raise _capi.SparchHipError(_TIMEOUT_TEXT + "  [" + describe_timeout() + "]  Set SPARCH_REC_STEPS_PER_LAUNCH=1 "
                               "(one launch per time step, no waiting inside) to run on a shared GPU.")


def rec_steps_per_launch(T):
    """Time steps per persistent launch of the recurrent cell kernels (default: whole sequence; 1 after a
    timeout put the current device into degraded mode)."""
    v = os.environ.get("SPARCH_REC_STEPS_PER_LAUNCH", "")
    if v:
        return int(v)
    if _degraded and torch.cuda.is_available() and torch.cuda.current_device() in _degraded:
        return 1
    return T


# Hidden sizes above this take the step path of the recurrent cells (the persistent kernels keep a (H x 32)
# slice of V in registers, which stops fitting at H > 1024); SPARCH_REC_STEP_PATH=1 forces it at any size (tests).
REC_PERSISTENT_MAX_H = 1024


def rec_step_path(H):
    return H > REC_PERSISTENT_MAX_H or os.environ.get("SPARCH_REC_STEP_PATH", "0") == "1"


def ligru_persistent_ok(H):
    """The LiGRU persistent kernels (gatedcell.hip) take hidden sizes that are multiples of 32 up to 1024;
    SPARCH_LIGRU_PERSISTENT=0 forces the launch-per-step path (comparison in tests)."""
    return H % 32 == 0 and H <= 1024 and os.environ.get("SPARCH_LIGRU_PERSISTENT", "1") != "0"


def gru_persistent_ok(H):
    """The GRU persistent kernels (gatedcell.hip): hidden sizes that are multiples of 32 up to 1024 whose H / 16
    workgroups per row tile fit the GPU at once (two hand-offs inside a step: no per-step degenerate form, so a
    device in degraded mode takes the launch-per-step path); SPARCH_GRU_PERSISTENT=0 forces that path."""
    if H % 32 != 0 or H > 1024 or os.environ.get("SPARCH_GRU_PERSISTENT", "1") == "0":
        return False
    if _degraded and torch.cuda.is_available() and torch.cuda.current_device() in _degraded:
        return False
    return H // 16 <= lib.sparch_device_cus()


def _f32c(t):
    return t.contiguous().float() if (t.dtype != torch.float32 or not t.is_contiguous()) else t


# ----------------------------------------------------------------------------- primitives
def flag_bf16_exact(x):
    """Device uint32: 1 iff every element of x is exactly representable in bf16 (no host sync)."""
    flag = torch.empty(4, dtype=torch.int32, device=x.device)
    check(lib.sparch_flag_bf16_exact(x.numel(), ptr(x), ptr(flag), _stream()), "sparch_flag_bf16_exact")
    return flag


def plane_bf16_exact(x2):
    """(plane, flag) of a (M, K) fp32 network input: the bf16 plane of x (rows padded to a multiple of 8 elements,
    zeros behind column K) and the device flag "every element is bf16-exact", made in ONE pass — the first
    layer's GEMMs then read the plane (2 bytes per element) when the flag is 1 and x itself otherwise."""
    M, K = x2.shape
    ldp = (K + 7) // 8 * 8
    plane = torch.empty(M, ldp, dtype=torch.bfloat16, device=x2.device)
    flag = torch.empty(4, dtype=torch.int32, device=x2.device)
    check(lib.sparch_plane_bf16_exact(M, K, ptr(x2), x2.stride(0), ptr(plane), ldp, ptr(flag), _stream()),
          "sparch_plane_bf16_exact")
    return plane, flag


_flag_one = {}


def input_from_counts(counts):
    """A batch of binned spike counts as (B,T,K) uint8 ON THE DEVICE -> the network input for SNN.forward: a
    (B,T,K) fp32 PLACEHOLDER (no values are written) carrying the bf16 plane the first layer's GEMMs read, made by
    one pass over the bytes (`sparch_expand_counts_u8`).  The reference uploads the dense float batch every step
    (exp.py:355-356: 179 MB at the headline shape against 45 MB of bytes); counts up to 255 are exact in both
    uint8 and bf16, so the plane — and everything computed from it — is the one `plane_bf16_exact` makes from the
    float batch."""
    _require_device(counts, "counts")
    if counts.dtype != torch.uint8 or counts.ndim != 3:
        raise ValueError("input_from_counts: a (B,T,K) uint8 tensor of spike counts")
    counts = counts.contiguous()
    B, T, K = counts.shape
    M, ldp = B * T, (K + 7) // 8 * 8
    plane = torch.empty(M, ldp, dtype=torch.bfloat16, device=counts.device)
    check(lib.sparch_expand_counts_u8(M, K, ptr(counts), ptr(plane), ldp, None, 0, _stream()), "sparch_expand_counts_u8")
    key = str(counts.device)
    one = _flag_one.get(key)
    if one is None:
        one = _flag_one[key] = torch.ones(4, dtype=torch.int32, device=counts.device)
    x = spike_placeholder(B, T, K, counts.device)
    x = x.view(B, T, K)  # a tensor object of its own for the tag (same one-element storage)
    x._sparch_input_plane = (tuple(x.shape), plane, one)
    return x


def input_from_plane(plane, B, T, K):
    """The network input `input_from_counts` returns, for a bf16 count plane (B*T, ldp) that is already on the device
    (zeros behind column K, counts <= 255: the spike encoders' output): the (B,T,K) placeholder tagged with the plane
    and the flag "exact"."""
    _require_device(plane, "plane")
    if plane.dtype != torch.bfloat16 or plane.ndim != 2 or plane.shape[0] != B * T or plane.shape[1] < K or \
            plane.shape[1] % 8 or not plane.is_contiguous():
        raise ValueError("input_from_plane: a contiguous (B*T, ldp) bf16 plane with ldp % 8 == 0 and ldp >= K")
    key = str(plane.device)
    one = _flag_one.get(key)
    if one is None:
        one = _flag_one[key] = torch.ones(4, dtype=torch.int32, device=plane.device)
    x = spike_placeholder(B, T, K, plane.device).view(B, T, K)
    x._sparch_input_plane = (tuple(x.shape), plane, one)
    return x


def input_plane_of(x):
    """(plane, flag) if x is an input made by `input_from_counts`, else None."""
    tag = getattr(x, "_sparch_input_plane", None)
    if tag is None or tag[0] != tuple(x.shape):
        return None
    return tag[1], tag[2]


def time_slice(x, t0, t1):
    """Steps [t0, t1) of a network input (B,T,K) as an input of its own: a contiguous copy, or — for an input made by
    `input_from_counts` — a placeholder that carries the same rows of the bf16 plane (chunks of a stateful run)."""
    tag = input_plane_of(x)
    if tag is None:
        return x[:, t0:t1].contiguous()
    B, T, K = x.shape
    plane, flag = tag
    part = plane.view(B, T, plane.shape[-1])[:, t0:t1].contiguous().view(-1, plane.shape[-1])
    xs = spike_placeholder(B, t1 - t0, K, x.device).view(B, t1 - t0, K)
    xs._sparch_input_plane = (tuple(xs.shape), part, flag)
    return xs


def split_planes(W):
    """The three exact bf16 planes of a weight matrix, (3, *W.shape) bf16 (W = p0 + p1 + p2 exactly, the
    truncation split the GEMM kernels otherwise redo in every workgroup that stages a tile of W); None where
    the pre-split kernels do not apply (a layout they do not take)."""
    if W.dtype != torch.float32 or not W.is_contiguous() or W.numel() % 8 or W.shape[-1] % 8:
        return None
    planes = torch.empty((3,) + tuple(W.shape), dtype=torch.bfloat16, device=W.device)
    check(lib.sparch_split3(W.numel(), ptr(W), ptr(planes), _stream()), "sparch_split3")
    return planes


def gemm_nt(A, B, bias=None, colstat=False, spike_scale=None, a_exact_flag=None, a16=None, b_planes=None,
            a_plane=None):
    """A (M,K) @ B (N,K)^T (+bias) -> (M,N); optional BatchNorm column-stat partials.
    spike_scale = c: A's entries are 0 or c (a spike train) -> exact bf16-split MFMA path;
    a16: the same spikes as a (M,K) bf16 0/1 plane (read instead of A);
    b_planes: split_planes(B) (same result; the kernel copies the planes instead of converting B)."""
    M, K = A.shape
    N = B.shape[0]
    C = torch.empty(M, N, dtype=torch.float32, device=A.device)
    ws = None
    if colstat:
        ws = torch.empty(2 * ((M + 127) // 128) * N, dtype=torch.float32, device=A.device)
    if spike_scale is not None and a16 is not None and b_planes is not None:
        tok = timer.start(f"gemm_spike_nt[{M}x{N}x{K}]")
        check(lib.sparch_gemm_spike16_nt_wp(M, N, K, ptr(a16), a16.stride(0), float(spike_scale), ptr(B),
                                            ptr(b_planes), B.stride(0), ptr(C), N, ptr(bias), ptr(ws), _stream(), _prec()),
              "sparch_gemm_spike16_nt_wp")
    elif spike_scale is not None and a16 is not None:
        tok = timer.start(f"gemm_spike_nt[{M}x{N}x{K}]")
        check(lib.sparch_gemm_spike16_nt(M, N, K, ptr(a16), a16.stride(0), float(spike_scale), ptr(B), B.stride(0),
                                         ptr(C), N, ptr(bias), ptr(ws), _stream(), _prec()), "sparch_gemm_spike16_nt")
    elif spike_scale is not None:
        tok = timer.start(f"gemm_spike_nt[{M}x{N}x{K}]")
        check(lib.sparch_gemm_spike_nt(M, N, K, ptr(A), A.stride(0), float(spike_scale), ptr(B), B.stride(0),
                                       ptr(C), N, ptr(bias), ptr(ws), _stream(), _prec()), "sparch_gemm_spike_nt")
    elif a_exact_flag is not None and a_plane is not None and DENSE_GEMM == "split6":
        tok = timer.start(f"gemm_auto_nt[{M}x{N}x{K}]")  # a_plane: plane_bf16_exact(A)[0], read when the flag is 1
        check(lib.sparch_gemm_auto16_nt(M, N, K, ptr(A), A.stride(0) or K, ptr(a_plane), a_plane.stride(0), ptr(B),
                                        B.stride(0), ptr(C), N, ptr(bias), ptr(ws), ptr(a_exact_flag), _stream(), _prec()),
              "sparch_gemm_auto16_nt")
    elif a_exact_flag is not None and DENSE_GEMM == "split6":
        tok = timer.start(f"gemm_auto_nt[{M}x{N}x{K}]")
        check(lib.sparch_gemm_auto_nt(M, N, K, ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(C), N, ptr(bias),
                                      ptr(ws), ptr(a_exact_flag), _stream(), _prec()), "sparch_gemm_auto_nt")
    else:
        split6 = DENSE_GEMM == "split6"  # (the fp32-input MFMA kernels of gemm.hip have one precision)
        fn = lib.sparch_gemm6_nt if split6 else lib.sparch_gemm_nt
        tok = timer.start(f"gemm_nt[{M}x{N}x{K}]")
        check(fn(M, N, K, ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(C), N, ptr(bias), ptr(ws), _stream(),
                 *((_prec(),) if split6 else ())), "sparch_gemm_nt")
    timer.stop(tok)
    return C, ws


def gemm_nn(A, B, b_planes=None):
    """A (M,K) @ B (K,N) -> (M,N).  b_planes: split_planes(B)."""
    M, K = A.shape
    N = B.shape[1]
    C = torch.empty(M, N, dtype=torch.float32, device=A.device)
    tok = timer.start(f"gemm_nn[{M}x{N}x{K}]")
    if b_planes is not None and DENSE_GEMM == "split6":
        check(lib.sparch_gemm6_nn_wp(M, N, K, ptr(A), A.stride(0), ptr(B), ptr(b_planes), B.stride(0), ptr(C), N,
                                     _stream(), _prec()), "sparch_gemm6_nn_wp")
    else:
        split6 = DENSE_GEMM == "split6"
        fn = lib.sparch_gemm6_nn if split6 else lib.sparch_gemm_nn
        check(fn(M, N, K, ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(C), N, _stream(), *((_prec(),) if split6 else ())),
              "sparch_gemm_nn")
    timer.stop(tok)
    return C


def _tn_workspace(device, M, N, K, split6=True):
    """(workspace, its byte count as the entry point is told it) for the K-range slabs of a TN product."""
    nbytes = (lib.sparch_gemm_spike_tn_workspace_bytes(M, N, K, _prec()) if split6
              else lib.sparch_gemm_tn_workspace_bytes(M, N, K))
    return torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=device), nbytes


def gemm_tn(A, B, zero_diag=False, spike_side=None, spike_scale=1.0, out=None, b_exact_flag=None, spike16=False,
            b_plane=None):
    """A (K,M)^T @ B (K,N) -> (M,N); contraction over the long leading axis.
    spike_side 0/1: A / B is a spike tensor (entries 0 or spike_scale) -> exact bf16-split MFMA path;
    spike16: that operand is given as a bf16 0/1 plane (torch.bfloat16).
    out: accumulate into this (M,N) tensor instead of allocating."""
    K, M = A.shape
    N = B.shape[1]
    accumulate = out is not None
    C = out if accumulate else torch.empty(M, N, dtype=torch.float32, device=A.device)
    if spike16 and spike_side is None:
        raise RuntimeError("internal: a bf16 spike plane needs the spike GEMM path")
    if spike_side is not None and spike16:
        ws, nbytes = _tn_workspace(A.device, M, N, K)
        tok = timer.start(f"gemm_spike_tn[{M}x{N}x{K}]")
        check(lib.sparch_gemm_spike16_tn(M, N, K, ptr(A), A.stride(0), ptr(B), B.stride(0), int(spike_side),
                                         float(spike_scale), ptr(C), C.stride(0), int(zero_diag), int(accumulate),
                                         ptr(ws), nbytes, _stream(), _prec()), "sparch_gemm_spike16_tn")
    elif spike_side is not None:
        ws, nbytes = _tn_workspace(A.device, M, N, K)
        tok = timer.start(f"gemm_spike_tn[{M}x{N}x{K}]")
        check(lib.sparch_gemm_spike_tn(M, N, K, ptr(A), A.stride(0), ptr(B), B.stride(0), int(spike_side),
                                       float(spike_scale), ptr(C), C.stride(0), int(zero_diag), int(accumulate),
                                       ptr(ws), nbytes, _stream(), _prec()), "sparch_gemm_spike_tn")
    elif b_exact_flag is not None and b_plane is not None and DENSE_GEMM == "split6":
        ws, nbytes = _tn_workspace(A.device, M, (N + 7) // 8 * 8, K)  # slabs at the plane's padded width
        tok = timer.start(f"gemm_auto_tn[{M}x{N}x{K}]")
        check(lib.sparch_gemm_auto16_tn(M, N, K, ptr(A), A.stride(0), ptr(B), B.stride(0) or N, ptr(b_plane),
                                        b_plane.stride(0), ptr(C), C.stride(0), int(zero_diag), int(accumulate),
                                        ptr(b_exact_flag), ptr(ws), nbytes, _stream(), _prec()), "sparch_gemm_auto16_tn")
    elif b_exact_flag is not None and DENSE_GEMM == "split6":
        ws, nbytes = _tn_workspace(A.device, M, N, K)
        tok = timer.start(f"gemm_auto_tn[{M}x{N}x{K}]")
        check(lib.sparch_gemm_auto_tn(M, N, K, ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(C), C.stride(0),
                                      int(zero_diag), int(accumulate), ptr(b_exact_flag), ptr(ws), nbytes,
                                      _stream(), _prec()), "sparch_gemm_auto_tn")
    else:
        split6 = DENSE_GEMM == "split6"
        ws, nbytes = _tn_workspace(A.device, M, N, K, split6)
        fn = lib.sparch_gemm6_tn if split6 else lib.sparch_gemm_tn
        tok = timer.start(f"gemm_tn[{M}x{N}x{K}]")
        check(fn(M, N, K, ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(C), C.stride(0), int(zero_diag),
                 int(accumulate), ptr(ws), nbytes, _stream(), *((_prec(),) if split6 else ())), "sparch_gemm_tn")
    timer.stop(tok)
    return C


def _colsum(x2d):
    M, H = x2d.shape
    out = torch.empty(H, dtype=torch.float32, device=x2d.device)
    nbytes = lib.sparch_bn_bwd_workspace_bytes(M, H)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=x2d.device)
    check(lib.sparch_colsum(M, H, ptr(x2d), ptr(out), ptr(ws), nbytes, _stream()), "sparch_colsum")
    return out


def _finish_param_grads(ws, rows, H, raws, lims):
    """ws (n,rows,H) partials -> list of (H,) grads gated by the clamp range (torch.clamp backward)."""
    import ctypes

    n = len(raws)
    outs = [torch.empty(H, dtype=torch.float32, device=ws.device) for _ in range(n)]
    raw_arr = (ctypes.c_void_p * n)(*[(r.data_ptr() if r is not None else None) for r in raws])  # None: no clamp gate
    out_arr = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    lim_arr = (ctypes.c_float * (2 * n))(*[v for lo_hi in lims for v in lo_hi])
    check(lib.sparch_colsum_clamped(n, rows, H, ptr(ws), raw_arr, lim_arr, out_arr, _stream()),
          "sparch_colsum_clamped")
    return outs


class _Norm:
    """Forward/backward of the normalisation on the (M,H) projection.  BatchNorm is folded into
    (scale, shift) consumed by the cell kernel; LayerNorm materialises the normalised tensor."""

    @staticmethod
    def forward(mode, Wx_raw, colstat, weight, bias, running_mean, running_var, training, dup, nbt=None, ln_width=None,
                n_valid=None):
        """nbt: BatchNorm's num_batches_tracked (int64 device tensor) — incremented by the finalize kernel itself,
        under the status-word guard, instead of by a separate host-side `+= 1` (None: the caller keeps doing that).
        ln_width: LayerNorm's width when the layer runs zero-padded to more columns (None: all H columns).
        n_valid: ragged batch — BatchNorm's sample count is the number of valid rows (the padded rows of Wx_raw are
        exactly zero and have added nothing to the column sums); None: all M rows."""
        M, H = Wx_raw.shape
        dev = Wx_raw.device
        if mode == "batchnorm":
            scale = torch.empty(H, dtype=torch.float32, device=dev)
            shift = torch.empty(H, dtype=torch.float32, device=dev)
            mean = torch.empty(H, dtype=torch.float32, device=dev)
            invstd = torch.empty(H, dtype=torch.float32, device=dev)
            n_tiles, rows = (M + 127) // 128, (M if n_valid is None else n_valid)
            if training and M <= BN_EXACT_ROWS and Wx_raw.is_contiguous():
                colstat, n_tiles = torch.empty(2 * 3 * H, dtype=torch.float32, device=dev), 3
                check(lib.sparch_bn_colstat_exact(M, H, ptr(Wx_raw), ptr(colstat), _stream()), "sparch_bn_colstat_exact")
            if training and SYNC_BN is not None and SYNC_BN["world"] > 1:
                import torch.distributed as dist

                world = SYNC_BN["world"]
                parts = [torch.empty_like(colstat) for _ in range(world)]
                dist.all_gather(parts, colstat, group=SYNC_BN["group"])
                colstat = torch.stack([q.view(2, n_tiles, H) for q in parts], dim=1).reshape(-1)  # (2, world*tiles, H)
                n_tiles, rows = n_tiles * world, M * world
            if training and rows * dup < 2:  # nn.BatchNorm1d's own refusal (the unbiased variance divides by n - 1)
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {(M, H)}")
            check(lib.sparch_bn_finalize(H, rows, n_tiles, dup, ptr(colstat), ptr(weight), ptr(bias),
                                         ptr(running_mean), ptr(running_var), BN_MOMENTUM, NORM_EPS,
                                         int(training), ptr(scale), ptr(shift), ptr(mean), ptr(invstd),
                                         ptr(status_word(dev)), ptr(nbt), _stream()), "sparch_bn_finalize")
            return Wx_raw, scale, shift, (mean, invstd)
        if mode == "layernorm":
            y = torch.empty_like(Wx_raw)
            mu = torch.empty(M, dtype=torch.float32, device=dev)
            rstd = torch.empty(M, dtype=torch.float32, device=dev)
            check(lib.sparch_layernorm_fwd(M, H, ln_width or H, ptr(Wx_raw), ptr(weight), ptr(bias), NORM_EPS, ptr(y),
                                           ptr(mu), ptr(rstd), _stream()), "sparch_layernorm_fwd")
            return y, None, None, (mu, rstd)
        return Wx_raw, None, None, None

    @staticmethod
    def backward(mode, dy, Wx_raw, weight, saved, training, sums=None, planes=False, dy2=None, keep_fp32=True,
                 ln_width=None, n_valid=None):
        """dy (M,H) grad wrt the normalised projection -> (dx_raw, dweight, dbias). May overwrite dy.
        sums = (dbeta, dgamma) when the cell's backward kernel already produced BatchNorm's column sums.
        planes=True (batchnorm, H % 8 == 0): returns (dx_raw or None, dweight, dbias, dx_planes) with dx_planes the
        (3, M, H) bf16 planes of dx_raw; keep_fp32=False skips the fp32 tensor (dx_raw is None).  dy2: the second
        direction's gradient of a bidirectional layer, added in the same pass (dy + dy2).  n_valid: ragged batch —
        BatchNorm's two means are over the valid rows (dy is zero on the padded ones, so the column sums are right as
        they come; the apply kernels divide by M, so the sums go in scaled by M / n_valid)."""
        M, H = dy.shape
        dev = dy.device
        if mode == "batchnorm":
            mean, invstd = saved  # batch statistics (train) or running statistics (eval)
            if sums is not None:
                dbeta, dgamma = sums
            else:
                dgamma = torch.empty(H, dtype=torch.float32, device=dev)
                dbeta = torch.empty(H, dtype=torch.float32, device=dev)
                nbytes = lib.sparch_bn_bwd_workspace_bytes(M, H)
                ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
                check(lib.sparch_bn_bwd_reduce(M, H, ptr(dy), ptr(Wx_raw), ptr(mean), ptr(invstd), ptr(dgamma),
                                               ptr(dbeta), ptr(ws), nbytes, _stream()), "sparch_bn_bwd_reduce")
            if training and SYNC_BN is not None and SYNC_BN["world"] > 1:
                import torch.distributed as dist

                red = torch.stack([dgamma, dbeta])
                dist.all_reduce(red, op=dist.ReduceOp.SUM, group=SYNC_BN["group"])
                red.mul_(1.0 / SYNC_BN["world"])  # the apply kernel divides by the LOCAL row count
                cg, cb = red[0], red[1]
            elif training:
                cg, cb = dgamma, dbeta
                if n_valid is not None and n_valid != M:
                    cg, cb = dgamma * (M / n_valid), dbeta * (M / n_valid)
            else:  # fixed statistics: dx = dy * gamma * invstd, i.e. the batch-coupling terms vanish
                cg = torch.zeros(H, dtype=torch.float32, device=dev)
                cb = cg
            if planes:
                dxp = torch.empty(3, M, H, dtype=torch.bfloat16, device=dev)
                dx_out = dy if keep_fp32 else None
                tok = timer.start(f"bn_bwd_apply_planes[{M}x{H}]")
                check(lib.sparch_bn_bwd_apply_planes(M, H, ptr(dy), ptr(dy2), ptr(Wx_raw), ptr(mean), ptr(invstd),
                                                     ptr(weight), ptr(cg), ptr(cb), ptr(dxp), ptr(dx_out), _stream()),
                      "sparch_bn_bwd_apply_planes")
                timer.stop(tok)
                return dx_out, dgamma, dbeta, dxp
            check(lib.sparch_bn_bwd_apply(M, H, ptr(dy), ptr(Wx_raw), ptr(mean), ptr(invstd), ptr(weight),
                                          ptr(cg), ptr(cb), ptr(dy), _stream()), "sparch_bn_bwd_apply")
            return dy, dgamma, dbeta
        if mode == "layernorm":
            mu, rstd = saved
            dgamma = torch.empty(H, dtype=torch.float32, device=dev)
            dbeta = torch.empty(H, dtype=torch.float32, device=dev)
            dx = torch.empty_like(dy)
            nbytes = lib.sparch_bn_bwd_workspace_bytes(M, H)
            ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
            check(lib.sparch_layernorm_bwd(M, H, ln_width or H, ptr(dy), ptr(Wx_raw), ptr(mu), ptr(rstd), ptr(weight),
                                           ptr(dx), ptr(dgamma), ptr(dbeta), ptr(ws), nbytes, _stream()),
                  "sparch_layernorm_bwd")
            return dx, dgamma, dbeta
        return dy, None, None


# ----------------------------------------------------------------------------- the projection of a layer
class _LayerInput(typing.NamedTuple):
    """How a layer's GEMMs read its (M,K) input: x2 itself (scale, x16, flag, plane all None); a spike train of ours
    with entries 0 or `scale`, read through its bf16 0/1 plane x16 (x2 may then be a placeholder without values);
    or a network input whose bf16 `plane` is read when the device `flag` says every value is bf16-exact, x2 otherwise.
    The forward product and the weight gradient take the same description, so they cannot disagree."""
    x2: torch.Tensor
    scale: typing.Optional[float] = None
    x16: typing.Optional[torch.Tensor] = None
    flag: typing.Optional[torch.Tensor] = None
    plane: typing.Optional[torch.Tensor] = None

    def project(self, W, Wb, colstat, b_planes=None):
        """x W^T (+ Wb) -> ((M,H), BatchNorm column-stat partials or None)."""
        return gemm_nt(self.x2, W, Wb, colstat=colstat, spike_scale=self.scale, a_exact_flag=self.flag, a16=self.x16,
                       b_planes=b_planes, a_plane=self.plane)

    def weight_grad(self, dx_raw):
        """dx_raw^T x -> (H,K)."""
        if self.scale is None:
            return gemm_tn(dx_raw, self.x2, b_exact_flag=self.flag, b_plane=self.plane)
        if self.x16 is None:
            return gemm_tn(dx_raw, self.x2, spike_side=1, spike_scale=self.scale)
        return gemm_tn(dx_raw, self.x16, spike_side=1, spike_scale=self.scale, spike16=True)


def _layer_input(cfg, x, gated=True):
    """The _LayerInput of x (B,T,K) under cfg's in_spike_scale / in_spike16 (x came out of a spiking layer of ours)
    and in_plane (x was made by input_from_counts).  gated: for any other input let the device decide whether it is
    bf16-exact (binned spike counts are) — one pass that also makes the plane the GEMMs then read."""
    B, T, K = x.shape
    scale, x16, tag = cfg.get("in_spike_scale"), cfg.get("in_spike16"), cfg.get("in_plane") if gated else None
    if scale is not None and x16 is not None:
        return _LayerInput(x.view(B * T, K), scale, x16.view(B * T, K))  # (x may be a placeholder: never touch it)
    if tag is not None:
        return _LayerInput(x.view(B * T, K), None, None, tag[1], tag[0])
    x2 = _f32c(x).view(B * T, K)
    if scale is not None or not gated:
        return _LayerInput(x2, scale)
    if DENSE_GEMM == "split6":
        plane, flag = plane_bf16_exact(x2)
        return _LayerInput(x2, None, None, flag, plane)
    return _LayerInput(x2, None, None, flag_bf16_exact(x2))


def _project(inp, W, Wb, nw, nb, cfg, dup, ln_width=None, n_valid=None):
    """norm(x W^T + Wb) of a layer -> (Wx_in, scale, shift, nsaved, Wx_raw): what the cell reads (BatchNorm stays
    folded into scale / shift), what _Norm.backward needs, and the raw projection where backward needs it (else
    None).  dup: how many directions share the rows (BatchNorm's sample count); n_valid: the rows that count in it
    (SeqLayout.n_valid; None: all)."""
    norm, training = cfg["normalization"], cfg["training"]
    Wx_raw, colstat = inp.project(W, Wb, colstat=(norm == "batchnorm" and training))
    Wx_in, scale, shift, nsaved = _Norm.forward(norm, Wx_raw, colstat, nw, nb, cfg.get("running_mean"),
                                                cfg.get("running_var"), training, dup,
                                                nbt=cfg.get("num_batches_tracked"), ln_width=ln_width,
                                                n_valid=n_valid)
    return Wx_in, scale, shift, nsaved, Wx_raw if norm in ("batchnorm", "layernorm") else None


def _use_dx_planes(inp, norm, dirs, M, K, H):
    """dx as bf16 planes (made once by the BatchNorm pass) for the dW and dX products: a hidden layer fed by a spike
    plane, exact mode, shapes the pipelined plane kernels take (whole tiles, 32-deep K tiles)."""
    return ((USE_DX_PLANES is True or (USE_DX_PLANES == "auto" and dirs == 2))
            and norm == "batchnorm" and inp.x16 is not None and DENSE_GEMM == "split6"
            and _precision == 0 and H % 32 == 0 and K % 32 == 0 and H >= 256 and K >= 256 and M >= 256
            and M % 32 == 0)


def _project_backward(inp, W, nw, cfg, nsaved, Wx_raw, dy, dirs=1, *, need_dx, need_bias, sums=None, ln_width=None,
                      w_planes=None, dx_planes=False, raw_dx=False, n_valid=None):
    """Backward of _project.  dy: the gradient of the normalised projection, (M,H) or the (B*dirs,T,H) halves of
    `dirs` directions that share the projection rows (snns.py:252-254); may be overwritten.  sums: BatchNorm's column
    sums where the cell's backward kernel made them.  w_planes: split_planes(W) for the dx product.  dx_planes: the
    layer may take the plane kernels (_use_dx_planes decides).  n_valid: as _project's.  Returns (dx (M,K) or None, dW,
    dWb or None, dnw, dnb); raw_dx: the first entry is dx_raw (M,H) instead — the caller forms dx itself."""
    norm = cfg["normalization"]
    H, K = W.shape
    M = dy.numel() // (H * dirs)
    dxp = None
    if dx_planes and _use_dx_planes(inp, norm, dirs, M, K, H) and (not need_dx or w_planes is not None):
        B = dy.shape[0] // dirs
        dy2 = dy[B:].view(M, H) if dirs == 2 else None  # second direction: added by the same pass
        dx_raw, dnw, dnb, dxp = _Norm.backward(norm, dy[:B].view(M, H), Wx_raw, nw, nsaved, cfg["training"], sums=sums,
                                               planes=True, dy2=dy2, keep_fp32=need_bias, n_valid=n_valid)
        nbytes = lib.sparch_gemm_spike_tn_workspace_bytes(H, K, M, _prec())
        ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=W.device)
        dW = torch.empty(H, K, dtype=torch.float32, device=W.device)
        tok = timer.start(f"gemm_spike_tn[{H}x{K}x{M}]")
        check(lib.sparch_gemm_spike16_tn_ap(H, K, M, ptr(dx_raw), ptr(dxp), H, ptr(inp.x16), inp.x16.stride(0),
                                            float(inp.scale), ptr(dW), K, 0, 0, ptr(ws), nbytes, _stream(), _prec()),
              "sparch_gemm_spike16_tn_ap")
        timer.stop(tok)
    else:
        if dirs == 2:
            halves, dy = dy, torch.empty(dy.shape[0] // 2, dy.shape[1], H, dtype=torch.float32, device=W.device)
            check(lib.sparch_add_halves(M * H, ptr(halves), ptr(dy), _stream()), "sparch_add_halves")
        dx_raw, dnw, dnb = _Norm.backward(norm, dy.view(M, H), Wx_raw, nw, nsaved, cfg["training"], sums=sums,
                                          ln_width=ln_width, n_valid=n_valid)
        dW = inp.weight_grad(dx_raw)
    dWb = _colsum(dx_raw) if need_bias else None
    if raw_dx:
        return dx_raw, dW, dWb, dnw, dnb
    dx = None
    if need_dx and dxp is not None:
        dx = torch.empty(M, K, dtype=torch.float32, device=W.device)
        tok = timer.start(f"gemm_nn[{M}x{K}x{H}]")
        check(lib.sparch_gemm6_nn_pp(M, K, H, ptr(dx_raw), ptr(dxp), H, ptr(W), ptr(w_planes), K, ptr(dx), K, _stream(),
                                     _prec()), "sparch_gemm6_nn_pp")
        timer.stop(tok)
    elif need_dx:
        dx = gemm_nn(dx_raw, W, b_planes=w_planes)
    return dx, dW, dWb, dnw, dnb


# ----------------------------------------------------------------------------- cells (given Wx)
_placeholder_zero = {}  # one element per device (a fresh torch.zeros(1) per layer and step was a fill kernel each)


def spike_placeholder(B, T, F, device):
    """(B,T,F) fp32 stand-in for a spike tensor whose only consumer reads its bf16 plane: one element of storage,
    expanded — autograd needs the edge's shape and dtype, nobody reads the values."""
    key = str(device)
    z = _placeholder_zero.get(key)
    if z is None:
        z = _placeholder_zero[key] = torch.zeros(1, dtype=torch.float32, device=device)
    return z.expand(B, T, F)


def _persistent(label, entry, lead, nbytes, dev, L, *tail, sg=None):
    """One persistent recurrent launch (a kernel whose workgroups wait for each other): `entry`(*lead, channel buffer
    of `nbytes`, its size, status word, L time steps per launch, [*sg: surrogate id and scale of an `_sg` entry,]
    stream, *tail) inside `_persistent_launch()`, timed under `label` (None: not timed)."""
    chan = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)  # (ceil: the byte count need not be a multiple of 8)
    tok = timer.start(label) if label is not None else None
    with _persistent_launch():
        check(getattr(lib, entry)(*lead, ptr(chan), nbytes, ptr(status_word(dev)), L, *(sg or ()), _stream(), *tail), entry)
    timer.stop(tok)


def _vpack(H, V, flags, vmask=None):
    """V (H,H) packed into the MFMA fragments of the persistent kernels (flags: 1 = transposed, 2 = dense, i.e. no
    zeroed diagonal); vmask: also write the masked fp32 copy there."""
    vpack = torch.empty(lib.sparch_vpack_bytes(H) // 4, dtype=torch.float32, device=V.device)
    check(lib.sparch_vpack(H, ptr(V), flags, ptr(vpack), ptr(vmask), _stream(), _prec()), "sparch_vpack")
    return vpack


SURROGATES = {"boxcar": 0, "triangle": 1, "fast_sigmoid": 2, "atan": 3}  # SPARCH_SURROGATE_*


def surrogate_args(surrogate):
    """None or ("name", scale) -> None for the reference's box-car, else (SPARCH_SURROGATE_* id, scale) of a smooth
    form (the forward pass is the same under every surrogate; the smooth ones run the `_sg` backward entry points)."""
    if surrogate is None or surrogate[0] == "boxcar":
        return None
    name, scale = surrogate
    if name not in SURROGATES:
        raise ValueError(f"unknown surrogate {name!r}: one of {sorted(SURROGATES)}")
    return SURROGATES[name], float(scale)


class PackPlan(typing.NamedTuple):
    """A packed ragged batch (snns.prepare_packing; DESIGN.md section 6, "Packed ragged batches"): the sequences sorted
    by length, descending and stable.  order / lengths / offsets / inverse are int32 views of ONE device buffer: sequence j
    is batch row order[j], has lengths[j] steps and owns packed rows [offsets[j], offsets[j] + lengths[j]); offsets has
    batch + 1 entries and offsets[batch] = n; inverse[order[j]] = j.  t_max is the longest length, T the padded tensors'
    time axis.  host: (order, lengths, offsets) as numpy arrays."""
    order: torch.Tensor
    lengths: torch.Tensor
    offsets: torch.Tensor
    inverse: torch.Tensor
    n: int
    t_max: int
    batch: int
    T: int
    host: tuple

    def args(self):
        """(lengths, offsets, n_valid) as the `_pk` entry points take them."""
        return ptr(self.lengths), ptr(self.offsets), int(self.n)


class SeqLayout(typing.NamedTuple):
    """How the time axis of a batch lies in memory, and the only place that knows how the three layouts differ:
    dense (B,T,.) tensors, the same with `lengths` = (device int32 (B,), their sum) masking every row's padded steps
    (the `_len` entry points), or `pack`, a PackPlan: (1,n,.) tensors of the valid steps only (the `_pk` ones).  Built
    once per layer pass (of_cfg) or per call of a public wrapper (its lengths= / pack= keywords).  For a bidirectional
    layer on a ragged batch `doubled` is the layout of its 2B sequences — every clip and, behind the batch, the clip
    read backwards — and fwd / rev say where the two copies of a packed sequence start there (BidirPlan)."""
    lengths: typing.Optional[tuple] = None
    pack: typing.Optional[PackPlan] = None
    doubled: typing.Optional["SeqLayout"] = None
    fwd: typing.Optional[torch.Tensor] = None
    rev: typing.Optional[torch.Tensor] = None

    @classmethod
    def of(cls, lengths=None, pack=None):
        """The layout of the lengths= / pack= keywords of the public wrappers (a dense batch: one shared record)."""
        return _DENSE if lengths is None and pack is None else cls(lengths, pack)

    @classmethod
    def of_cfg(cls, cfg):
        """The layout a layer Function's cfg describes: cfg["lengths"] or cfg["pack"], and for dirs == 2 the doubled
        batch's cfg["lengths2"] (snns.double_lengths) or cfg["pack2"] (a BidirPlan).  The bidir_* movers alone also
        take a cfg without dirs."""
        lengths, pack, two = cfg.get("lengths"), cfg.get("pack"), cfg.get("dirs") == 2
        if lengths is None and pack is None:
            return _DENSE
        if pack is not None:
            plan2 = cfg["pack2"] if two else cfg.get("pack2")
            return cls(None, pack) if plan2 is None else cls(None, pack, cls(None, plan2.plan), plan2.fwd, plan2.rev)
        return cls(lengths, None, cls(cfg["lengths2"]) if two and lengths is not None else None)

    @property
    def suffix(self):
        """What the layout appends to an entry point's name."""
        return "_pk" if self.pack is not None else "" if self.lengths is None else "_len"

    def index(self, B, T):
        """The kernels' (sequences, steps) for tensors whose leading shape is (B, T)."""
        return (B, T) if self.pack is None else (self.pack.batch, self.pack.t_max)

    @property
    def ragged_steps(self):
        """The steps that exist in a ragged batch; 0 for a dense one (what the `_red` entries take)."""
        return int(self.pack.n) if self.pack is not None else 0 if self.lengths is None else int(self.lengths[1])

    def n_valid(self, B, T):
        """The steps that exist in tensors of leading shape (B, T): the firing rate's and BatchNorm's denominator."""
        return self.ragged_steps or B * T

    @property
    def tail(self):
        """The arguments the cell and readout entries take for the layout: (), (lengths, n_valid) or (lengths,
        offsets, n_valid)."""
        if self.pack is not None:
            return self.pack.args()
        return () if self.lengths is None else (ptr(self.lengths[0]), int(self.lengths[1]))

    @property
    def ptrs(self):
        """(lengths, offsets) as the entries with one form for all layouts take them (delay, synapse, `_red`): NULL for
        what the layout does not have."""
        if self.pack is not None:
            return ptr(self.pack.lengths), ptr(self.pack.offsets)
        return (None if self.lengths is None else ptr(self.lengths[0])), None

    def space(self, B, T):
        """(sequences, steps, lengths, offsets): the index space of the delay and synapse kernels for (B,T,.) tensors —
        packed ones are (1,n,.), and the shift or the filter stays inside each sequence's rows."""
        if self.pack is not None and (B, T) != (1, self.pack.n):
            raise ValueError(f"sparch_amd: a packed delay input must be (1, {self.pack.n}, K), got ({B}, {T}, K)")
        return (*self.index(B, T), *self.ptrs)

    @property
    def map_tail(self):
        """The arguments behind the tensors of the sparch_bidir_* entries."""
        return self.tail if self.pack is None else (*self.ptrs, ptr(self.fwd), ptr(self.rev), int(self.pack.n))

    def scaled(self, B, T, num, den=1):
        """The leading shape of a tensor with num / den times the sequences of one whose leading shape is (B, T)."""
        return (1, T * num // den) if self.pack is not None else (B * num // den, T)

    def first_steps(self, t, rows, flipped=False):
        """t (B',T,H), or packed (1,n,H) -> (rows,H): the first step of the sequences `rows` (a slice; packed: of all
        of them), which for a dense direction that runs backwards in time (flipped) is the last."""
        if self.pack is not None:
            return t.view(-1, t.shape[-1]).index_select(0, self.pack.offsets[:self.pack.batch])
        return t[rows, t.shape[1] - 1 if flipped else 0, :]


_DENSE = SeqLayout()


def _pack_call(entry, src, dst, plan, C):
    check(getattr(lib, entry)(plan.batch, plan.T, C, src.element_size(), ptr(src), ptr(dst), ptr(plan.order),
                              ptr(plan.lengths), ptr(plan.offsets), int(plan.n), _stream()), entry)


def pack_rows(x, plan):
    """x (batch, T, C), elements of 1, 2 or 4 bytes -> (n, C): every sequence's own steps, in the plan's order."""
    _require_device(x, "input")
    x = x.contiguous()
    B, T, C = x.shape
    if (B, T) != (plan.batch, plan.T) or x.element_size() not in (1, 2, 4):
        raise ValueError(f"pack_rows: a ({plan.batch}, {plan.T}, C) tensor of 1-, 2- or 4-byte elements (got "
                         f"{tuple(x.shape)}, {x.dtype})")
    out = torch.empty(plan.n, C, dtype=x.dtype, device=x.device)
    tok = timer.start("pack_rows")
    _pack_call("sparch_pack_rows", x, out, plan, C)
    timer.stop(tok)
    return out


def unpack_rows(xp, plan):
    """xp (n, C) -> (batch, T, C) in the caller's row order, exactly 0 on every row's steps t >= its length."""
    _require_device(xp, "input")
    xp = xp.contiguous()
    if xp.ndim != 2 or xp.shape[0] != plan.n or xp.element_size() not in (1, 2, 4):
        raise ValueError(f"unpack_rows: a ({plan.n}, C) tensor of 1-, 2- or 4-byte elements (got {tuple(xp.shape)}, {xp.dtype})")
    out = torch.empty(plan.batch, plan.T, xp.shape[1], dtype=xp.dtype, device=xp.device)
    tok = timer.start("unpack_rows")
    _pack_call("sparch_unpack_rows", xp, out, plan, xp.shape[1])
    timer.stop(tok)
    return out


class PackRowsFn(torch.autograd.Function):
    """pack_rows with its gradient: unpack_rows (zero on the padding)."""

    @staticmethod
    def forward(ctx, x, plan):
        ctx.plan = plan
        return pack_rows(x, plan)

    @staticmethod
    def backward(ctx, g):
        return unpack_rows(_f32c(g), ctx.plan), None


class UnpackRowsFn(torch.autograd.Function):
    """unpack_rows with its gradient: pack_rows (what arrives on the padding is dropped)."""

    @staticmethod
    def forward(ctx, xp, plan):
        ctx.plan = plan
        return unpack_rows(xp, plan)

    @staticmethod
    def backward(ctx, g):
        return pack_rows(_f32c(g), ctx.plan), None


# ----------------------------------------------------------------------------- axonal delays
MAX_DELAY_CAP = 255  # the largest max_delay the kernels take (csrc/delay.hip)


def check_max_delay(max_delay, zero_ok=False):
    """max_delay as SNN and the delay kernels take it: an integer in [1, 255] ([0, 255] with zero_ok) -> int."""
    lo = 0 if zero_ok else 1
    if isinstance(max_delay, bool) or not isinstance(max_delay, int) or not lo <= max_delay <= MAX_DELAY_CAP:
        raise ValueError(f"sparch_amd: max_delay must be an integer in [{lo}, {MAX_DELAY_CAP}] (got {max_delay!r})")
    return max_delay


def _delay_rows(x, what):
    """x (B,T,K), 2- or 4-byte elements -> (x, row stride in elements) with unit stride along K and the rows of all
    batch entries one stride apart (a column slice of a wider buffer is read where it lies, anything else is copied)."""
    if x.ndim != 3 or x.element_size() not in (2, 4):
        raise ValueError(f"{what}: a (B,T,K) tensor of 2- or 4-byte elements (got {tuple(x.shape)}, {x.dtype})")
    B, T, K = x.shape
    if T > 1:
        ld = x.stride(1)
        ok = B == 1 or x.stride(0) == T * ld
    else:
        ld = x.stride(0) if B > 1 else K
        ok = True
    if not (ok and ld >= K and (K == 1 or x.stride(2) == 1)):
        x, ld = x.contiguous(), K
    return x, ld


def _check_delays(delay, K, device, what):
    """The delay parameter as the kernels read it: K contiguous fp32 values on the tensors' device."""
    delay = _f32c(delay)
    if delay.numel() != K or delay.device != device:
        raise ValueError(f"{what}: {K} delays on {device} (got {tuple(delay.shape)} on {delay.device})")
    return delay


def delay_forward(x, delay, max_delay, lengths=None, pack=None, out=None):
    """y[b,t,i] = x[b, t - d_i, i] for d_i <= t < len_b, else 0, with d_i = rint(clamp(delay_i, 0, max_delay)) taken on
    the device (`sparch_delay_fwd`).  x (B,T,K): any 2- or 4-byte dtype (the bf16 spike plane, fp32), moved as raw
    bytes.  out: a tensor to write (same dtype; every row that exists is written), else a fresh contiguous one."""
    _require_device(x, "input")
    D = check_max_delay(max_delay)
    x, ldx = _delay_rows(x, "delay_forward")
    B, T, K = x.shape
    delay = _check_delays(delay, K, x.device, "delay_forward")
    y = torch.empty(B, T, K, dtype=x.dtype, device=x.device) if out is None else out
    if y.dtype != x.dtype or tuple(y.shape) != (B, T, K):
        raise ValueError("delay_forward: out must have the input's shape and dtype")
    y_rows, ldy = _delay_rows(y, "delay_forward")
    if y_rows is not y:
        raise ValueError("delay_forward: out must have unit stride along K and one row stride")
    Bk, Tk, len_ptr, off_ptr = SeqLayout.of(lengths, pack).space(B, T)
    tok = timer.start("delay_fwd")
    check(lib.sparch_delay_fwd(Bk, Tk, K, x.element_size(), D, ptr(delay), ptr(x), ldx, ptr(y), ldy, len_ptr, off_ptr,
                               _stream()), "sparch_delay_fwd")
    timer.stop(tok)
    return y


def delay_backward(g_y, delay, max_delay, x=None, x_scale=1.0, lengths=None, pack=None, need_gx=True, need_gdelay=True):
    """The two gradients of delay_forward (`sparch_delay_bwd`) -> (g_x or None, g_delay or None), both fp32.
    g_x[b,t,i] = g_y[b, t + d_i, i] for t + d_i < len_b, else 0.  g_delay: the finite difference of the delayed input
    (SLAYER's rule), gate_i * sum g_y[b,t,i] * x_scale * (x[b,t-d_i-1,i] - x[b,t-d_i,i]); x is the forward's input, fp32
    or its bf16 plane; summed in a fixed order (two runs give the same bits)."""
    _require_device(g_y, "gradient")
    D = check_max_delay(max_delay)
    g_y, ldg = _delay_rows(_f32c(g_y), "delay_backward")
    B, T, K = g_y.shape
    delay = _check_delays(delay, K, g_y.device, "delay_backward")
    Bk, Tk, len_ptr, off_ptr = SeqLayout.of(lengths, pack).space(B, T)
    g_x = torch.empty(B, T, K, dtype=torch.float32, device=g_y.device) if need_gx else None
    g_delay = ws = None
    nbytes, esize, ldx = 0, 4, K
    if need_gdelay:
        if x is None or tuple(x.shape) != (B, T, K):
            raise ValueError("delay_backward: the delay's gradient needs the forward's input, in the gradient's shape")
        if x.dtype not in (torch.float32, torch.bfloat16):
            x = x.float()
        x, ldx = _delay_rows(x, "delay_backward")
        esize = x.element_size()
        g_delay = torch.empty(K, dtype=torch.float32, device=g_y.device)
        nbytes = lib.sparch_delay_bwd_workspace_bytes(Bk, Tk, K)
        ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=g_y.device)
    if not need_gx and not need_gdelay:
        return None, None
    tok = timer.start("delay_bwd")
    check(lib.sparch_delay_bwd(Bk, Tk, K, esize, D, ptr(delay), ptr(g_y), ldg, ptr(x) if need_gdelay else None, ldx,
                               float(x_scale), ptr(g_x), K, ptr(g_delay), ptr(ws), nbytes, len_ptr, off_ptr, _stream()),
          "sparch_delay_bwd")
    timer.stop(tok)
    return g_x, g_delay


def delay_stream(x, delay, max_delay, hist, out=None):
    """The delay on a chunk x (B,Tc,K) of a stream (`sparch_delay_stream`): hist (B,max_delay,K), same dtype,
    contiguous, holds the last max_delay input steps and is advanced in place."""
    _require_device(x, "input")
    D = check_max_delay(max_delay)
    x, ldx = _delay_rows(x, "delay_stream")
    B, Tc, K = x.shape
    if tuple(hist.shape) != (B, D, K) or hist.dtype != x.dtype or not hist.is_contiguous() or hist.device != x.device:
        raise ValueError(f"delay_stream: hist must be a contiguous ({B}, {D}, {K}) {x.dtype} tensor on {x.device}")
    y = torch.empty(B, Tc, K, dtype=x.dtype, device=x.device) if out is None else out
    y_rows, ldy = _delay_rows(y, "delay_stream")
    if y_rows is not y or y.dtype != x.dtype or tuple(y.shape) != (B, Tc, K):
        raise ValueError("delay_stream: out must have the input's shape and dtype, unit stride along K")
    delay = _check_delays(delay, K, x.device, "delay_stream")
    check(lib.sparch_delay_stream(B, Tc, K, x.element_size(), D, ptr(delay), ptr(x), ldx, ptr(y), ldy, ptr(hist),
                                  _stream()), "sparch_delay_stream")
    return y


class DelayFn(torch.autograd.Function):
    """x (B,T,K), delay (K,) -> (y, y_plane): the layer input shifted by its per-feature delays (DESIGN.md section 6,
    "Axonal delays"), on the representation the layer's GEMMs read.  cfg: max_delay; lengths / pack as the layers take
    them; plane: None — x itself is gathered and y_plane is None — or the (B,T,K) bf16 plane that carries x's values
    (a spike train of ours, an input made by input_from_counts): the plane is gathered into y_plane ((B*T, ld_plane)
    with zeros behind column K, ld_plane default K) and y is a placeholder without values, as x may be; scale: x = plane
    * scale (the delay's gradient reads the plane)."""

    @staticmethod
    def forward(ctx, x, delay, cfg):
        _require_device(x, "input")
        _require_device(delay, "delay")
        B, T, K = x.shape
        D, plane, lay = cfg["max_delay"], cfg.get("plane"), SeqLayout.of_cfg(cfg)
        lengths, pack = lay.lengths, lay.pack
        if plane is None:
            src = x if x.element_size() in (2, 4) else x.float()
            src = src.contiguous() if src.stride(2) != 1 else src
            y, y16 = delay_forward(src, delay, D, lengths, pack), None
        else:
            ld = int(cfg.get("ld_plane", K))
            store = (torch.empty if ld == K else torch.zeros)(B * T, ld, dtype=plane.dtype, device=plane.device)
            delay_forward(plane, delay, D, lengths, pack, out=store.view(B, T, ld)[:, :, :K])
            src, y, y16 = plane, spike_placeholder(B, T, K, x.device), store
            ctx.mark_non_differentiable(y16)
        ctx.cfg, ctx.lay = cfg, lay
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(delay, src if ctx.needs_input_grad[1] else None)
        return y, y16

    @staticmethod
    def backward(ctx, g_y, _g16=None):
        if g_y is None:
            return None, None, None
        cfg = ctx.cfg
        delay, src = ctx.saved_tensors
        g_x, g_delay = delay_backward(g_y, delay, cfg["max_delay"], src, float(cfg.get("scale") or 1.0),
                                      ctx.lay.lengths, ctx.lay.pack, need_gx=ctx.needs_input_grad[0],
                                      need_gdelay=ctx.needs_input_grad[1])
        return g_x, g_delay, None


# ----------------------------------------------------------------------------- synaptic currents
def check_synapse(synapse):
    """synapse as SNN and the synapse kernels take it: None, or (lo, hi) with 0 <= lo <= hi < 1 -> None or two floats."""
    if synapse is None:
        return None
    try:
        lo, hi = synapse
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"sparch_amd: synapse must be None or a pair (lo, hi) of numbers (got {synapse!r})") from None
    if not 0.0 <= lo <= hi < 1.0:
        raise ValueError(f"sparch_amd: synapse limits must satisfy 0 <= lo <= hi < 1 (got {synapse!r})")
    return lo, hi


def _limits(limits):
    if limits is None:
        raise ValueError("sparch_amd: the synapse kernels need their limits (lo, hi)")
    return check_synapse(limits)


def _synapse_cols(t, H, device, what, name):
    """An (H,) per-column operand of the synapse kernels (None stays None): contiguous fp32 on the tensors' device."""
    if t is None:
        return None
    t = _f32c(t)
    if t.numel() != H or t.device != device:
        raise ValueError(f"{what}: {name} must hold {H} values on {device} (got {tuple(t.shape)} on {t.device})")
    return t


def _synapse_state(t, rows, H, device, what, name):
    if t is None:
        return None
    if tuple(t.shape) != (rows, H) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != device:
        raise ValueError(f"{what}: {name} must be a contiguous ({rows}, {H}) fp32 tensor on {device}")
    return t


def _synapse_out(out, B, T, H, device, what):
    """(the tensor a synapse kernel writes, its row stride): `out` where given and usable as it lies, else a fresh one."""
    if out is None:
        return torch.empty(B, T, H, dtype=torch.float32, device=device), H
    if tuple(out.shape) != (B, T, H) or out.dtype != torch.float32 or out.device != device:
        raise ValueError(f"{what}: out must be a ({B}, {T}, {H}) fp32 tensor on {device}")
    rows, ld = _delay_rows(out, what)
    if rows is not out:
        raise ValueError(f"{what}: out must have unit stride along H and one row stride")
    return out, ld


def synapse_forward(Wx, gamma, limits, bias=None, scale=None, shift=None, i0=None, lengths=None, pack=None,
                    want_final=False, i_T=None, out=None):
    """i[b,t,h] = g_h i[b,t-1,h] + (1 - g_h) z[b,t,h] for t < len_b, with g = clamp(gamma, *limits) taken on the device
    and z the cell's input as the cell forms it from (Wx, bias, scale, shift) (`sparch_synapse_fwd`; DESIGN.md section
    6, "Synaptic currents").  Wx (B,T,H) fp32, or packed (1,n,H) with pack; i0 (rows,H) or None (zeros).  Returns i, and
    with want_final (or an i_T to write, which may be i0) the pair (i, i_T): every row's state after its last step.
    out: an fp32 tensor of Wx's shape to write (unit stride along H, one row stride; every row that exists is written),
    else a fresh contiguous one."""
    lo, hi = _limits(limits)
    _require_device(Wx, "input")
    Wx, ldwx = _delay_rows(Wx if Wx.dtype == torch.float32 else Wx.float(), "synapse_forward")
    B, T, H = Wx.shape
    dev = Wx.device
    Bk, Tk, len_ptr, off_ptr = SeqLayout.of(lengths, pack).space(B, T)
    gamma = _synapse_cols(gamma, H, dev, "synapse_forward", "gamma")
    bias, scale, shift = (_synapse_cols(t, H, dev, "synapse_forward", n)
                          for t, n in ((bias, "bias"), (scale, "scale"), (shift, "shift")))
    i0 = _synapse_state(i0, Bk, H, dev, "synapse_forward", "i0")
    if i_T is None and want_final:
        i_T = torch.empty(Bk, H, dtype=torch.float32, device=dev)
    i_T = _synapse_state(i_T, Bk, H, dev, "synapse_forward", "i_T")
    i_out, ldi = _synapse_out(out, B, T, H, dev, "synapse_forward")
    tok = timer.start("synapse_fwd")
    check(lib.sparch_synapse_fwd(Bk, Tk, H, ptr(Wx), ldwx, ptr(bias), ptr(scale), ptr(shift), ptr(gamma), lo, hi,
                                 ptr(i0), ptr(i_out), ldi, ptr(i_T), len_ptr, off_ptr, _stream()), "sparch_synapse_fwd")
    timer.stop(tok)
    return (i_out, i_T) if i_T is not None else i_out


def synapse_backward(g_i, i, gamma, limits, i0=None, lengths=None, pack=None, need_gz=True, need_ggamma=True, out=None,
                     bn=None):
    """The two gradients of synapse_forward (`sparch_synapse_bwd`) -> (g_z or None, g_gamma or None), both fp32.  i is
    the forward's result, i0 the forward's.  g_z is exactly 0 on padded steps, whatever g_i holds there; g_gamma is
    summed in a fixed order (two runs give the same bits) and is 0 where gamma lies outside its limits.  out: a tensor
    for g_z, as synapse_forward's.
    bn = (Wx_raw, mean, invstd) of the layer's BatchNorm: a third result, (sum g_z, sum g_z xhat) per column — BatchNorm
    backward's column sums, accumulated by the same kernel in the cell backward kernels' order and finished as theirs."""
    lo, hi = _limits(limits)
    _require_device(g_i, "gradient")
    if not need_gz and not need_ggamma:
        return None, None
    g_i, ldg = _delay_rows(g_i if g_i.dtype == torch.float32 else g_i.float(), "synapse_backward")
    B, T, H = g_i.shape
    dev = g_i.device
    Bk, Tk, len_ptr, off_ptr = SeqLayout.of(lengths, pack).space(B, T)
    gamma = _synapse_cols(gamma, H, dev, "synapse_backward", "gamma")
    i0 = _synapse_state(i0, Bk, H, dev, "synapse_backward", "i0")
    g_z, ldgz = _synapse_out(out, B, T, H, dev, "synapse_backward") if need_gz else (None, H)
    g_gamma = ws = None
    nbytes, ldi = 0, H
    if need_ggamma:
        if i is None or tuple(i.shape) != (B, T, H):
            raise ValueError("synapse_backward: gamma's gradient needs the forward's result, in the gradient's shape")
        i, ldi = _delay_rows(i if i.dtype == torch.float32 else i.float(), "synapse_backward")
        g_gamma = torch.empty(H, dtype=torch.float32, device=dev)
        nbytes = lib.sparch_synapse_bwd_workspace_bytes(Bk, Tk, H)
        ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=dev)
    bn_x = bn_mean = bn_invstd = bn_ws = None
    if bn is not None:
        bn_x, bn_mean, bn_invstd = bn
        if not need_gz or bn_x.numel() != B * T * H or not bn_x.is_contiguous() or bn_x.dtype != torch.float32:
            raise ValueError("synapse_backward: bn needs g_z and the contiguous fp32 projection in the gradient's shape")
        bn_ws = torch.empty(2, Bk, H, dtype=torch.float32, device=dev)
    tok = timer.start("synapse_bwd")
    check(lib.sparch_synapse_bwd(Bk, Tk, H, ptr(g_i), ldg, ptr(i) if need_ggamma else None, ldi, ptr(i0), ptr(gamma),
                                 lo, hi, ptr(g_z), ldgz, ptr(g_gamma), ptr(ws), nbytes, ptr(bn_x), H, ptr(bn_mean),
                                 ptr(bn_invstd), ptr(bn_ws), len_ptr, off_ptr, _stream()), "sparch_synapse_bwd")
    timer.stop(tok)
    if bn is not None:
        return g_z, g_gamma, tuple(_finish_param_grads(bn_ws, Bk, H, [None, None], [(0.0, 0.0)] * 2))
    return g_z, g_gamma


def synapse_stream(Wx, gamma, limits, state, bias=None, scale=None, shift=None):
    """The synapse on a chunk Wx (B,Tc,H) of a stream: state (B,H) fp32, contiguous, is the current after the last step
    seen (zeros at the start of a stream) and is advanced in place; the same call as synapse_forward, so a stream cut
    into chunks gives the whole sequence's bits."""
    if state is None:
        raise ValueError("synapse_stream: the carried state is required")
    return synapse_forward(Wx, gamma, limits, bias, scale, shift, i0=state, i_T=state)[0]


def _check_packed(pack, dirs, recurrent, H):
    """What the `_pk` kernels do not take."""
    if pack is None:
        return
    if recurrent and rec_step_path(H):
        raise ValueError(f"sparch_amd: pack=True with a recurrent hidden size above 1024 (got {H}) is not supported "
                         "(the per-step recurrent path takes no packed batches)")
    if recurrent and rec_steps_per_launch(2) < 2:
        raise ValueError("sparch_amd: pack=True in the degraded step mode (one recurrent launch per time step) is not "
                         "supported: the packed recurrent kernels run whole sequences only")
    if recurrent and isinstance(pack, PackPlan) and rec_steps_per_launch(pack.t_max) < pack.t_max:
        raise ValueError(f"sparch_amd: pack=True with chunked recurrent launches (SPARCH_REC_STEPS_PER_LAUNCH="
                         f"{rec_steps_per_launch(pack.t_max)} for sequences of up to {pack.t_max} steps) is not supported: "
                         "the packed recurrent kernels run whole sequences only")


def _check_ragged(lengths, dirs, recurrent, H):
    """What the `_len` kernels do not take."""
    if lengths is None:
        return
    if recurrent and rec_step_path(H):
        raise ValueError(f"sparch_amd: lengths with a recurrent hidden size above 1024 (got {H}) is not supported "
                         "(the per-step recurrent path takes no lengths)")


def _check_one_direction(dirs, lengths, pack):
    """The `_len` / `_pk` cell kernels run one direction: a bidirectional layer reaches them through SpikingLayerFn, which
    runs them on 2B sequences between bidir_split and bidir_join ("Bidirectional ragged batches")."""
    if dirs != 1 and (lengths is not None or pack is not None):
        raise ValueError("sparch_amd: cell_forward / cell_backward with lengths or pack take dirs=1 (a bidirectional "
                         "layer runs them on the doubled batch: SpikingLayerFn)")


# ----------------------------------------------------------------------------- bidirectional layers on ragged batches
class BidirPlan(typing.NamedTuple):
    """The doubled batch of a bidirectional layer on a packed ragged batch (snns.prepare_bidir_packing): `plan` is the
    PackPlan of the 2B sequences — batch row b is clip b, row B + b clip b read backwards — and fwd / rev (B,) int32, in
    the single plan's sorted order, the first row of sequence j's forward and reversed copy in the doubled packed
    tensor.  All views of one device buffer."""
    plan: PackPlan
    fwd: torch.Tensor
    rev: torch.Tensor


def _bidir_call(stem, lay, single, *args):
    """One sparch_bidir_* mover under its timer label: `stem` + the layout's suffix, on the kernels' index space of the
    single tensor (leading shape `single`), `args` between that and the layout's map arguments."""
    entry = stem + lay.suffix
    tok = timer.start(stem[len("sparch_"):])
    check(getattr(lib, entry)(*lay.index(*single), *args, *lay.map_tail, _stream()), entry)
    timer.stop(tok)


def bidir_split(x, cfg):
    """x (B,T,C), or packed (1,n,C), elements of 1, 2 or 4 bytes -> (2B,T,C) / (1,2n,C): the batch and, behind it, every
    clip read backwards inside its own length; zeros on the tails.  cfg: a layer's cfg, or its SeqLayout."""
    lay = cfg if isinstance(cfg, SeqLayout) else SeqLayout.of_cfg(cfg)
    x = x.contiguous()
    C = x.shape[2]
    out = torch.empty(*lay.scaled(*x.shape[:2], 2), C, dtype=x.dtype, device=x.device)
    _bidir_call("sparch_bidir_split", lay, x.shape[:2], C, x.element_size(), ptr(x), ptr(out))
    return out


def bidir_split_backward(g, cfg):
    """The adjoint of bidir_split on fp32: g (2B,T,C) / (1,2n,C) -> (B,T,C) / (1,n,C), exactly 0 on the tails."""
    lay = cfg if isinstance(cfg, SeqLayout) else SeqLayout.of_cfg(cfg)
    g = _f32c(g)
    C = g.shape[2]
    single = lay.scaled(*g.shape[:2], 1, 2)
    out = torch.empty(*single, C, dtype=torch.float32, device=g.device)
    _bidir_call("sparch_bidir_split_bwd", lay, single, C, ptr(g), ptr(out))
    return out


def bidir_join(s16, cfg, scale=1.0, want_fp32=True):
    """s16 (2B,T,H) / (1,2n,H), the bf16 0/1 plane of the doubled batch -> (s (B,T,2H) fp32 = plane * scale or None,
    the plane (B,T,2H), count (2H,) int32 of the spikes per output column): forward columns first, the reverse
    direction back in the clip's own time order, zeros on the tails."""
    lay = cfg if isinstance(cfg, SeqLayout) else SeqLayout.of_cfg(cfg)
    H = s16.shape[2]
    single = lay.scaled(*s16.shape[:2], 1, 2)
    y16 = torch.empty(*single, 2 * H, dtype=torch.bfloat16, device=s16.device)
    y32 = torch.empty(*single, 2 * H, dtype=torch.float32, device=s16.device) if want_fp32 else None
    count = torch.zeros(2 * H, dtype=torch.int32, device=s16.device)
    _bidir_call("sparch_bidir_join", lay, single, H, ptr(s16), ptr(y16), ptr(y32), float(scale), ptr(count))
    return y32, y16, count


def bidir_join_backward(g, g_rate, rate_scale, cfg):
    """The adjoint of bidir_join: g (B,T,2H) / (1,n,2H) fp32 -> (2B,T,H) / (1,2n,H), with g_rate[column] * rate_scale (the
    firing rate's gradient; g_rate None: nothing) added on the valid steps and exactly 0 on the tails."""
    lay = cfg if isinstance(cfg, SeqLayout) else SeqLayout.of_cfg(cfg)
    g = _f32c(g)
    H = g.shape[2] // 2
    out = torch.empty(*lay.scaled(*g.shape[:2], 2), H, dtype=torch.float32, device=g.device)
    _bidir_call("sparch_bidir_join_bwd", lay, g.shape[:2], H, ptr(g), ptr(g_rate), float(rate_scale), ptr(out))
    return out


def check_stateful(kind=None, H=0, *, dirs=1, lengths=None, pack=None, per_step=None, readout=None, T=None):
    """The refusals of stateful training (`state` / `return_state`), each before any kernel.
    kind=None: the readout layer."""
    if dirs != 1:
        raise ValueError("sparch_amd: state / return_state with bidirectional=True is not supported (a carried state "
                         "is causal: the reverse direction would start where the stream has not arrived yet)")
    if pack is not None:  # (in front of lengths: a packed batch always comes with them)
        raise ValueError("sparch_amd: state / return_state with pack is not supported (the packed kernels have no "
                         "stateful form)")
    if lengths is not None:
        raise ValueError("sparch_amd: state / return_state with lengths is not supported (the kernels with lengths "
                         "have no stateful form)")
    if per_step is not None:
        raise ValueError("sparch_amd: state / return_state with per_step is not supported (the per-step readout has "
                         "no stateful form)")
    if readout_mode(readout) != 0:
        raise ValueError(f"sparch_amd: state / return_state with readout={readout!r} is not supported (chunks add up "
                         "under the softmax-sum only)")
    if SAVE_BF16:
        raise ValueError("sparch_amd: state / return_state with SPARCH_SAVE_DTYPE=bf16 is not supported (the final "
                         "state is read from the fp32 saves)")
    if _prec() != 0:
        raise ValueError("sparch_amd: state / return_state in the bf16 operand mode is not supported")
    if kind is not None and KIND[kind] & 2:
        if rec_step_path(H):
            raise ValueError(f"sparch_amd: state / return_state with a recurrent hidden size above 1024 (got {H}) is not "
                             "supported (the per-step recurrent path has no stateful form)")
        L = rec_steps_per_launch(T if T is not None else 1 << 30)
        if L < (T if T is not None else 2):
            raise ValueError("sparch_amd: state / return_state in the degraded or chunked recurrent launch modes "
                             f"({L} steps per launch) is not supported (the stateful recurrent backward runs whole "
                             "sequences only)")


class _ColPad:
    """The zero-padding of a recurrent width H to the next multiple of 4, H4 (cell_forward says why): pad / cut work on
    the last axis, which holds `groups` blocks of H (H4) columns; None stays None."""

    def __init__(self, H):
        self.H, self.H4 = H, (H + 3) // 4 * 4

    def pad(self, t, groups=1):
        if t is None:
            return None
        lead = t.shape[:-1]
        return torch.nn.functional.pad(t.reshape(*lead, groups, self.H), (0, self.H4 - self.H)).reshape(*lead, groups * self.H4)

    def cut(self, t, groups=1):
        if t is None:
            return None
        lead = t.shape[:-1]
        return t.reshape(*lead, groups, self.H4)[..., :self.H].reshape(*lead, groups * self.H).contiguous()

    def pad_params(self, p):
        """The cell's parameters: V (H,H) grows on both axes."""
        d = self.H4 - self.H
        return {n: (torch.nn.functional.pad(v, (0, d, 0, d)) if n == "V" else self.pad(v)) for n, v in p.items()}

    def cut_params(self, grads):
        return {n: (v[:self.H, :self.H].contiguous() if n == "V" else self.cut(v)) for n, v in grads.items()}


def cell_forward(kind, Wx, scale, shift, p, u0, w0, s0, *, B, dirs, theta, p_drop, seed, steps_per_launch=None,
                 want_s_out=True, want_saves=True, surrogate=None, lengths=None, pack=None):
    """Run one spiking cell over the whole sequence on the device.

    Wx (B,T,H) raw projection (+ optional per-column scale/shift); u0/w0/s0 (B*dirs,H).
    Returns (s_out (B,T,H*dirs), count (H*dirs) int32, saved, s16) where saved feeds cell_backward and s16 is
    s_out != 0 as a bf16 plane.  want_s_out=False (round 3): the fp32 tensor is not written — s_out is
    None — for a layer whose output only feeds the next layer's spike GEMMs
    (the reference materialises it because its next op is a dense nn.Linear, snns.py:261; here it was 4 of the
    14 bytes a recurrent forward step stores per element).  want_saves=False (LIF / adLIF, nothing will be
    differentiated — validation and test forwards, exp.py:405-518): u / w are not saved either (8 of an adLIF step's
    14 bytes); `saved` is then (None, None).  surrogate: with a smooth form the saves stay fp32 whatever
    SPARCH_SAVE_DTYPE says — a bf16 save keeps the box-car's three decisions, not the u a smooth gate reads.
    lengths: None, or (device int32 (B,), their sum) of a ragged batch — the `_len` entry points then zero the output
    spikes of every row's padded steps and leave them out of `count`.
    pack: None, or a PackPlan — Wx is then the packed (1, n, H) projection, B = 1, u0 / w0 / s0 hold the plan's `batch`
    rows in its sorted order, and every (B,T,.) result above is (1, n, .): the `_pk` entry points."""
    _, T, H = Wx.shape
    Bp = B * dirs
    dev = Wx.device
    k = KIND[kind]
    adaptive, recurrent = bool(k & 1), bool(k & 2)
    lay = SeqLayout.of(lengths, pack)
    _check_one_direction(dirs, lengths, pack)
    _check_ragged(lengths, dirs, recurrent, H)
    _check_packed(pack, dirs, recurrent, H)
    if recurrent and H % 4 != 0:
        # The recurrent kernels own 4 columns per thread.  Any other width (the reference takes any nb_hiddens,
        # snns.py:608-661) runs zero-padded to the next multiple of 4: a padded neuron has no input, no
        # recurrent weights and u0 = 0, so it never spikes and feeds nothing; outputs are sliced back.
        cols = _ColPad(H)
        s_p, count_p, saved_p, s16_p = cell_forward(kind, cols.pad(Wx), cols.pad(scale), cols.pad(shift), cols.pad_params(p),
                                                    cols.pad(u0), cols.pad(w0), cols.pad(s0), B=B, dirs=dirs, theta=theta,
                                                    p_drop=p_drop, seed=seed, steps_per_launch=steps_per_launch,
                                                    want_s_out=want_s_out, surrogate=surrogate, lengths=lengths, pack=pack)
        return cols.cut(s_p, dirs), cols.cut(count_p, dirs), saved_p, cols.cut(s16_p, dirs)
    # the same spikes as a bf16 0/1 plane for the GEMMs of the next layer (rows must stay 16-byte aligned)
    s16 = torch.empty(B, T, H * dirs, dtype=torch.bfloat16, device=dev)
    s_out = torch.empty(B, T, H * dirs, dtype=torch.float32, device=dev) if want_s_out else None
    steps = lambda T_: steps_per_launch if steps_per_launch is not None else rec_steps_per_launch(T_)  # noqa: E731
    # bf16 saves: the recurrent kernels take them for whole-sequence launches only (a chunked forward resumes
    # from the saved state, which must then be exact)
    save16 = SAVE_BF16 and H % 4 == 0 and (not recurrent or (steps(T) >= T and not rec_step_path(H)))
    if surrogate_args(surrogate) is not None:
        save16 = False
    sdt = torch.bfloat16 if save16 else torch.float32
    want_saves = want_saves or recurrent  # (the recurrent kernels always save)
    u_save = torch.empty(Bp, T, H, dtype=sdt, device=dev) if want_saves else None
    w_save = torch.empty(Bp, T, H, dtype=sdt, device=dev) if (adaptive and want_saves) else None
    count = torch.zeros(H * dirs, dtype=torch.int32, device=dev)
    if recurrent and rec_step_path(H):
        # One launch per time step, the recurrent product s_{t-1} @ V between the steps on the exact
        # spike GEMM (3 bf16 planes of V, fp32 accumulate): same arithmetic as the persistent kernel.
        vmask = torch.empty(H, H, dtype=torch.float32, device=dev)
        check(lib.sparch_vmask(H, ptr(p["V"]), ptr(vmask), _stream()), "sparch_vmask")
        vmask_t = vmask.t().contiguous()              # (H_out, H_in): the NT operand
        rec = gemm_nn(s0, vmask)                      # t = 0: s0 is uniform noise, not binary
        s_step = torch.empty(Bp, H, dtype=torch.bfloat16, device=dev)
        tok = timer.start(f"rec_cell_fwd_steps[{kind}]")
        for t in range(T):
            if t > 0:
                rec, _ = gemm_nt(s_step, vmask_t, spike_scale=1.0, a16=s_step)
            check(lib.sparch_rec_cell_step_fwd(k, B, dirs, T, H, t, ptr(Wx), ptr(scale), ptr(shift),
                                               ptr(p["alpha"]), ptr(p.get("beta")), ptr(p.get("a")),
                                               ptr(p.get("b")), ptr(rec), ptr(u0), ptr(w0), ptr(s0), theta,
                                               p_drop, seed, ptr(s_out), ptr(s16), ptr(u_save), ptr(w_save),
                                               ptr(count), ptr(s_step), _stream()), "sparch_rec_cell_step_fwd")
        timer.stop(tok)
        return s_out, count, (u_save, w_save), s16
    # both families: the kernels' sequences and steps and the drive in front, the states and results behind
    Bk, Tk = lay.index(B, T)
    lead = (k, Bk, dirs, Tk, H, ptr(Wx), ptr(scale), ptr(shift), ptr(p["alpha"]), ptr(p.get("beta")), ptr(p.get("a")),
            ptr(p.get("b")))
    rest = (ptr(u0), ptr(w0), ptr(s0), theta, p_drop, seed, ptr(s_out), ptr(s16), ptr(u_save), ptr(w_save), int(save16),
            ptr(count), *lay.tail)
    if not recurrent:
        entry = "sparch_cell_fwd" + lay.suffix
        tok = timer.start(f"cell_fwd[{kind}]")
        check(getattr(lib, entry)(*lead, *rest, _stream()), entry)
        timer.stop(tok)
        return s_out, count, (u_save, w_save), s16
    # forward fragments, backward fragments (kept for cell_backward) and the masked copy: one launch
    vpack = torch.empty(lib.sparch_vpack_bytes(H) // 4, dtype=torch.float32, device=dev)
    vpack_t = torch.empty_like(vpack)
    vmask = torch.empty(H, H, dtype=torch.float32, device=dev)
    check(lib.sparch_vpack_both(H, ptr(p["V"]), ptr(vpack), ptr(vpack_t), ptr(vmask), _stream(), _prec()), "sparch_vpack_both")
    # t = 0 drive: s0 is uniform noise, not binary (snns.py:559/702): a (B', H, H) dense product, split-K so
    # that its 16 output tiles become a full grid (38 -> ~15 us at B' = 256, H = 1024)
    rec0 = _gemm_small(s0, vmask, nn=True)
    _persistent(f"rec_cell_fwd[{kind}]", "sparch_rec_cell_fwd" + lay.suffix, (*lead, ptr(vpack), ptr(rec0), *rest),
                lib.sparch_rec_chan_bytes(Bk * dirs, Tk, H), dev, steps(Tk), _prec())
    return s_out, count, (u_save, w_save, vpack_t), s16


def cell_backward(kind, g_out, g_rate, p, u0, w0, s0, saved, *, B, dirs, T, H, theta, p_drop, seed,
                  steps_per_launch=None, bn=None, surrogate=None, lengths=None, pack=None, state_grads=None,
                  want_state_grads=False):
    """Reverse-time pass.  Returns dWx (B*dirs,T,H) [virtual rows, original time index],
    param grads dict (alpha[,beta,a,b][,V]) — plus, with bn = (Wx_raw (B,T,H), mean, invstd), the entry
    "bn_sums" = (dbeta, dgamma): BatchNorm backward's column sums, accumulated by the same kernel.
    surrogate: None or ("name", scale).  None / "boxcar" issue the calls they always did; a smooth form issues the
    `_sg` entry points with (id, scale) in front of the stream (timer labels unchanged).
    lengths: as in cell_forward — the `_len` entry points (one per family, any surrogate) take the incoming gradient of
    a row's padded steps as zero, whatever g_out holds there; dWx is exactly 0 on them.
    pack: as in cell_forward (B = 1, T = n: g_out, dWx and bn's projection are the packed (1, n, .) tensors).
    state_grads / want_state_grads (stateful training): state_grads = (g_uT, g_wT, g_sT), each
    (B,H) or None, is the gradient arriving on the chunk's final state (u_T, w_T, s_T = 1[u_T > theta]);
    want_state_grads=True adds the entry "state" = (g_u0, g_w0, g_s0), the gradient of the initial state (g_w0 None
    without adaptation).  Either issues sparch_cell_bwd_st (timer label unchanged); neither: the calls above."""
    sg = surrogate_args(surrogate)
    Bp = B * dirs
    dev = g_out.device
    k = KIND[kind]
    adaptive, recurrent = bool(k & 1), bool(k & 2)
    lay = SeqLayout.of(lengths, pack)
    stateful = want_state_grads or (state_grads is not None and any(g is not None for g in state_grads))
    if stateful:
        check_stateful(kind, H, dirs=dirs, lengths=lengths, pack=pack,
                       T=T if steps_per_launch is None or steps_per_launch >= T else None)
        if steps_per_launch is not None and steps_per_launch < T and recurrent:
            raise ValueError("sparch_amd: state / return_state in the degraded or chunked recurrent launch modes is not "
                             "supported (the stateful recurrent backward runs whole sequences only)")
        if saved[0].dtype != torch.float32:
            raise ValueError("sparch_amd: stateful training needs fp32 saves (SPARCH_SAVE_DTYPE=bf16 is not supported)")
    _check_one_direction(dirs, lengths, pack)
    _check_ragged(lengths, dirs, recurrent, H)
    _check_packed(pack, dirs, recurrent, H)
    u_save, w_save = saved[0], saved[1]
    if recurrent and u_save.shape[-1] != H:  # forward ran zero-padded to a multiple of 4 columns (see cell_forward)
        cols = _ColPad(H)
        st_kw = {}
        if stateful:  # (the padding's state is zero and stays zero: its incoming gradient is zero, its outgoing one cut off)
            st_kw = {"state_grads": tuple(cols.pad(g) for g in (state_grads or (None, None, None))),
                     "want_state_grads": want_state_grads}
        dWx_p, gp = cell_backward(kind, cols.pad(g_out, dirs), cols.pad(g_rate, dirs), cols.pad_params(p), cols.pad(u0),
                                  cols.pad(w0), cols.pad(s0), saved, B=B, dirs=dirs, T=T, H=cols.H4, theta=theta,
                                  p_drop=p_drop, seed=seed, steps_per_launch=steps_per_launch, bn=None,
                                  surrogate=surrogate, lengths=lengths, pack=pack, **st_kw)
        state_p = gp.pop("state", None)
        grads = cols.cut_params(gp)
        if state_p is not None:
            grads["state"] = tuple(cols.cut(g) for g in state_p)
        return cols.cut(dWx_p), grads
    vpack_fwd_made = saved[2] if len(saved) > 2 else None  # backward fragments of V packed by cell_forward
    save16 = u_save.dtype == torch.bfloat16
    dWx = torch.empty(Bp, T, H, dtype=torch.float32, device=dev)
    n_base = 6 if recurrent else 4
    Bk, Tk = lay.index(B, T)  # (the kernels' B and T; the partial sums are per sequence)
    rows = Bk * dirs
    ws = torch.empty(n_base + (2 if bn is not None else 0), rows, H, dtype=torch.float32, device=dev)
    bn_x, bn_mean, bn_invstd = bn if bn is not None else (None, None, None)
    grads = {}
    # which backward entry of either family, and what it takes behind the layout's arguments: the stateful form the
    # surrogate and the two state gradients, a ragged layout the surrogate (one entry for all of them), dense the
    # box-car's entry nothing and the smooth ones' `_sg` theirs
    sg_any = sg if sg is not None else (SURROGATES["boxcar"], 0.0)
    if stateful:
        g_in = [None if g is None else _f32c(g) for g in (state_grads or (None, None, None))]
        g_0 = [torch.empty(rows, H, dtype=torch.float32, device=dev) if (want_state_grads and (i != 1 or adaptive))
               else None for i in range(3)]
        variant, extra = "_st", (*sg_any, *(ptr(g) for g in g_in), *(ptr(g) for g in g_0))
    elif lay.suffix:
        variant, extra = lay.suffix, sg_any
    else:
        variant, extra = ("", ()) if sg is None else ("_sg", sg)
    lead = (k, Bk, dirs, Tk, H, ptr(g_out), ptr(g_rate), ptr(u_save), ptr(w_save), int(save16), ptr(p["alpha"]),
            ptr(p.get("beta")), ptr(p.get("a")), ptr(p.get("b")))
    rest = (ptr(u0), ptr(w0), ptr(s0), theta, p_drop, seed, ptr(dWx))
    bn_ptrs = (ptr(bn_x), ptr(bn_mean), ptr(bn_invstd))
    if not recurrent:
        entry = "sparch_cell_bwd" + variant
        tok = timer.start(f"cell_bwd[{kind}]")
        check(getattr(lib, entry)(*lead, *rest, ptr(ws), *bn_ptrs, *lay.tail, *extra, _stream()), entry)
        timer.stop(tok)
    else:
        V = p["V"]
        s_prev = torch.empty(dWx.shape, dtype=torch.bfloat16, device=dev)  # bf16 0/1 plane
        if rec_step_path(H):
            # reverse-time steps with dWx_{t+1} @ V^T between them (exact six-term split GEMM)
            vmask = torch.empty(H, H, dtype=torch.float32, device=dev)
            check(lib.sparch_vmask(H, ptr(V), ptr(vmask), _stream()), "sparch_vmask")
            dwx_step = torch.empty(Bp, H, dtype=torch.float32, device=dev)
            rec = None
            entry = "sparch_rec_cell_step_bwd" + ("" if sg is None else "_sg")
            tok = timer.start(f"rec_cell_bwd_steps[{kind}]")
            for t in range(T - 1, -1, -1):
                if t + 1 < T:
                    rec, _ = gemm_nt(dwx_step, vmask)     # rec[b,i] = sum_j dWx[b,j] Vm[i,j]
                check(getattr(lib, entry)(k, B, dirs, T, H, t, ptr(g_out), ptr(g_rate), ptr(u_save), ptr(w_save),
                                          ptr(p["alpha"]), ptr(p.get("beta")), ptr(p.get("a")), ptr(p.get("b")), ptr(rec),
                                          *rest, ptr(s_prev), ptr(ws), *bn_ptrs, ptr(dwx_step), *(sg or ()), _stream()),
                      entry)
            timer.stop(tok)
        else:
            vpack_t = vpack_fwd_made if vpack_fwd_made is not None else _vpack(H, V, 1)
            _persistent(f"rec_cell_bwd[{kind}]", "sparch_rec_cell_bwd" + variant,
                        (*lead, ptr(vpack_t), *rest, ptr(s_prev), ptr(ws), *bn_ptrs, *lay.tail),
                        lib.sparch_rec_chan_bytes(rows, Tk, H), dev,
                        steps_per_launch if steps_per_launch is not None else rec_steps_per_launch(Tk), _prec(),
                        sg=extra)
            if want_state_grads:
                # g_s0's third term, (dWx_1) Vm^T: one (B' x H)(H x H) product on the first step's dWx (the kernel wrote
                # the two pointwise terms)
                vmask = torch.empty(H, H, dtype=torch.float32, device=dev)
                check(lib.sparch_vmask(H, ptr(V), ptr(vmask), _stream()), "sparch_vmask")
                rec1, _ = gemm_nt(dWx[:, 0, :].contiguous(), vmask)  # rec1[b,i] = sum_j dWx_1[b,j] Vm[i,j]
                g_0[2] = g_0[2] + rec1
        # dV = sum_t s_{t-1}^T (1-alpha) du_t with the diagonal zeroed (mask at snns.py:566/712):
        # binary rows t >= 1 on the exact bf16-split path, plus the t = 0 term with the non-binary s0
        # (cell step 0 sits at original time 0 for the forward direction, T-1 for the flipped one)
        dV = gemm_tn(s_prev.view(-1, H), dWx.view(-1, H), zero_diag=True, spike_side=0, spike16=True)
        for dd in range(dirs):  # s_prev rows of cell step 0 are zero: add the s0 term
            r0 = slice(dd * Bk, (dd + 1) * Bk)
            gemm_tn(s0[r0], lay.first_steps(dWx, r0, flipped=bool(dd)), zero_diag=True, out=dV)
        grads["V"] = dV
    if want_state_grads:
        grads["state"] = tuple(g_0)
    names = ["alpha"] + (["beta", "a", "b"] if adaptive else [])
    lims = [ALPHA_LIM] + ([BETA_LIM, A_LIM, B_LIM] if adaptive else [])
    if bn is None:
        outs = _finish_param_grads(ws, rows, H, [p[n] for n in names], lims)
    else:
        # one launch for the parameter planes and the two BatchNorm planes behind them (no clamp gate there; the
        # planes in between, if any, are summed too and dropped)
        n_all = n_base + 2
        outs = _finish_param_grads(ws, rows, H, [p[n] for n in names] + [None] * (n_all - len(names)),
                                   lims + [(0.0, 0.0)] * (n_all - len(names)))
        grads["bn_sums"] = (outs[n_base], outs[n_base + 1])
    grads.update(dict(zip(names, outs)))
    return dWx, grads


# ----------------------------------------------------------------------------- layer Functions
def _check_synapse_layer(cfg, gamma, lay):
    """What a layer with a synapse does not take, before any kernel."""
    check_synapse(cfg["synapse"])
    if gamma is None:
        raise ValueError("sparch_amd: a layer with a synapse needs its parameter gamma")
    if cfg.get("stateful"):
        raise ValueError("sparch_amd: state / return_state with a synapse is not supported (the carried state has no "
                         "synaptic current yet)")
    if cfg["dirs"] == 2 and lay.pack is not None:
        raise ValueError("sparch_amd: pack=True with bidirectional=True and a synapse is not supported")
    if cfg["dirs"] == 2 and lay.lengths is None:
        raise ValueError("sparch_amd: a bidirectional layer with a synapse runs on the doubled batch: it needs lengths "
                         "(snns synthesises lengths = T)")


class SpikingLayerFn(torch.autograd.Function):
    """x (B,T,K) -> (s (B,T,H*dirs), firing_rate (H*dirs)) for LIF / adLIF / RLIF / RadLIF."""

    @staticmethod
    def forward(ctx, cfg, x, W, Wb, nw, nb, alpha, beta, a, b, V, u0, w0, s0, gamma=None):
        _require_device(x, "input")
        _require_device(W, "layer parameters")
        kind, dirs, theta, p_drop, seed = cfg["kind"], cfg["dirs"], cfg["theta"], cfg["p_drop"], cfg["seed"]
        # synaptic currents: cfg["synapse"] = (lo, hi) puts the filter between the projection and
        # the cell, which then reads the current i with no scale and no shift; absent: every call below is what it was
        syn = cfg.get("synapse")
        ctx.has_gamma = gamma is not None
        # the layout of the time axis; a bidirectional layer on a ragged one runs its cell on the doubled batch
        lay = SeqLayout.of_cfg(cfg)
        two, fp32_out = lay.doubled is not None, cfg.get("fp32_out", True)
        cell_lay = lay.doubled if two else lay
        if syn is not None:
            _check_synapse_layer(cfg, gamma, lay)
        inp = _layer_input(cfg, x)
        B, T, K = x.shape
        H = W.shape[0]
        # the weights' bf16 planes, split once here for backward's dx GEMM (775 -> 732 us).  The projection itself
        # converts W on the fly: every workgroup streams all of W, and 4 MB of fp32 stay resident in the XCD's 4 MB
        # L2 where 6 MB of planes do not (0.42 against 0.61 GB of L2 misses per launch, 1.8 % faster)
        ctx.w_planes = split_planes(W) if (ctx.needs_input_grad[1] and K % 32 == 0 and H >= 128) else None
        Wx_in, scale, shift, nsaved, Wx_raw = _project(inp, W, Wb, nw, nb, cfg, dirs,
                                                       n_valid=lay.n_valid(B, T))  # snns.py:261, 264-266
        p = {"alpha": alpha, "beta": beta, "a": a, "b": b, "V": V}
        p = {k_: v for k_, v in p.items() if v is not None}
        if cfg.get("states_ready") is not None:  # initial states uploaded on a side stream (snns._rand_batch)
            cfg["states_ready"]()
        inv_keep = 1.0 / (1.0 - p_drop)
        drive = Wx_in.view(B, T, H)
        if two:
            # both directions as 2B sequences of the one-direction `_len` / `_pk` kernels: the normalised drive is
            # split (the projection and BatchNorm's statistics ran once, on B rows, as on the padded path), the
            # spikes are joined and counted per direction
            drive = bidir_split(drive, lay)
        if syn is not None:  # the cell reads the current, no scale, no shift; each direction filtered in its own order
            drive = ctx.syn_i = synapse_forward(drive, gamma, syn, scale=scale, shift=shift, lengths=cell_lay.lengths,
                                                pack=cell_lay.pack)
            scale = shift = None
        s_out, count, saved, s16 = cell_forward(kind, drive, scale, shift, p, u0, w0, s0, B=drive.shape[0],
                                                dirs=1 if two else dirs, theta=theta, p_drop=p_drop, seed=seed,
                                                want_s_out=fp32_out and not two,
                                                want_saves=any(ctx.needs_input_grad) or bool(cfg.get("stateful")),
                                                surrogate=cfg.get("surrogate"), lengths=cell_lay.lengths,
                                                pack=cell_lay.pack)
        if two:
            s_out, s16, count = bidir_join(s16, lay, scale=inv_keep, want_fp32=fp32_out)
        if s_out is None:
            s_out = spike_placeholder(B, T, H * dirs, x.device)
        # snns.py:174 on post-dropout spikes, ragged: the mean over valid steps (int32 * float -> fp32, one kernel)
        rate = count * (inv_keep / float(lay.n_valid(B, T)))
        ctx.cfg, ctx.inp, ctx.lay = cfg, inp, lay
        ctx.shape = (B, T, K, H)
        ctx.nsaved = nsaved
        ctx.cell_saved = saved
        ctx.set_materialize_grads(False)  # no zero tensors for unused outputs (s16 is as large as s in bf16)
        ctx.save_for_backward(inp.x2, W, nw, alpha, beta, a, b, V, u0, w0, s0, Wx_raw, *([gamma] if syn is not None else []))
        ctx.mark_non_differentiable(s16)
        if cfg.get("stateful"):
            # the final state: with fp32 saves the last saved step IS u_T / w_T, and s_T = 1[u_T > theta] is the raw
            # spike, before dropout (how the kernels themselves resume); outputs of this node, so that a gradient on
            # them reaches backward() as g_uT / g_wT / g_sT
            # (a recurrent width that runs zero-padded saves the padded width: the state goes out unpadded)
            u_T = saved[0][:, T - 1, :H].contiguous()
            w_T = saved[1][:, T - 1, :H].contiguous() if saved[1] is not None else None
            s_T = (u_T > theta).to(torch.float32)
            return s_out, rate, s16, u_T, w_T, s_T
        return s_out, rate, s16

    @staticmethod
    def backward(ctx, g_s, g_rate, _g_s16=None, g_uT=None, g_wT=None, g_sT=None):
        cfg = ctx.cfg
        kind, norm, dirs = cfg["kind"], cfg["normalization"], cfg["dirs"]
        B, T, K, H = ctx.shape
        x2, W, nw, alpha, beta, a, b, V, u0, w0, s0, Wx_raw, *gamma = ctx.saved_tensors
        dev = x2.device
        if g_s is None:
            g_s = torch.zeros(B, T, H * dirs, dtype=torch.float32, device=dev)
        g_s = _f32c(g_s)
        if g_rate is not None:
            g_rate = _f32c(g_rate)
        p = {"alpha": alpha, "beta": beta, "a": a, "b": b, "V": V}
        p = {k_: v for k_, v in p.items() if v is not None}
        syn, lay = cfg.get("synapse"), ctx.lay
        two = lay.doubled is not None
        cell_lay = lay.doubled if two else lay
        n_valid = lay.n_valid(B, T)
        # BatchNorm backward's column sums (dbeta, dgamma): out of the cell's backward kernel; with a synapse out of the
        # filter's adjoint instead (they are sums over g_z, not over the current's gradient), made where the cell's
        # kernel would have (one direction, whole 4-column pieces) in that kernel's order — at gamma = 0 the layer's
        # gradients are the bits of the layer without a synapse; on the doubled batch, which has 2B rows of a
        # projection that has B, _project_backward's own pass forms them
        bn = (Wx_raw, ctx.nsaved[0], ctx.nsaved[1]) if (norm == "batchnorm" and H % 4 == 0 and not two) else None
        st_kw = {}
        if cfg.get("stateful"):  # (absent otherwise: the calls and their arguments are then what they always were)
            st_kw = {"state_grads": (g_uT, g_wT, g_sT), "want_state_grads": any(ctx.needs_input_grad[11:14])}
        if two:
            # the forward's movements, reversed: the gather (with the rate's gradient, each direction's own count over
            # the valid steps), the one-direction cell backward on the doubled batch, and below the two directions'
            # dWx summed in the clip's own time order
            g_s, g_rate = bidir_join_backward(g_s, g_rate, 1.0 / float(n_valid), lay), None
        g, pg = cell_backward(kind, g_s, g_rate, p, u0, w0, s0, ctx.cell_saved, B=g_s.shape[0], dirs=1 if two else dirs,
                              T=g_s.shape[1], H=H, theta=cfg["theta"], p_drop=cfg["p_drop"], seed=cfg["seed"],
                              bn=None if syn is not None else bn, surrogate=cfg.get("surrogate"), lengths=cell_lay.lengths,
                              pack=cell_lay.pack, **st_kw)
        sums, g_gm = pg.get("bn_sums"), None
        if syn is not None:
            g, g_gm, *sums = synapse_backward(g, ctx.syn_i, gamma[0], syn, need_ggamma=ctx.needs_input_grad[14], bn=bn,
                                              lengths=cell_lay.lengths, pack=cell_lay.pack)
            sums = sums[0] if sums else None
        ctx.cell_saved = ctx.syn_i = None
        if two:
            g = bidir_split_backward(g, lay)
        dx, dW, dWb, dnw, dnb = _project_backward(ctx.inp, W, nw, cfg, ctx.nsaved, Wx_raw, g, 1 if two else dirs,
                                                  need_dx=ctx.needs_input_grad[1], need_bias=ctx.needs_input_grad[3],
                                                  sums=sums, w_planes=ctx.w_planes, dx_planes=True, n_valid=n_valid)
        dx = None if dx is None else dx.view(B, T, K)
        ctx.w_planes = ctx.inp = None
        g_u0, g_w0, g_s0 = pg.get("state", (None, None, None))
        need = ctx.needs_input_grad
        return (None, dx, dW, dWb, dnw, dnb, pg.get("alpha"), pg.get("beta"), pg.get("a"), pg.get("b"),
                pg.get("V"), g_u0 if need[11] else None, g_w0 if need[12] else None, g_s0 if need[13] else None,
                *((g_gm,) if ctx.has_gamma else ()))  # (one more gradient exactly when gamma was passed)


SEQ_MODES = {"prob": 0, "sum": 1}  # per-step readout: SPARCH_SEQ_PROB / SPARCH_SEQ_SUM


def seq_mode(per_step):
    """per_step (None, "prob" or "sum") -> None or the C ABI's seq_mode."""
    if per_step is None:
        return None
    if not isinstance(per_step, str) or per_step not in SEQ_MODES:
        raise ValueError(f"sparch_amd: per_step must be None, 'prob' or 'sum' (got {per_step!r})")
    return SEQ_MODES[per_step]


# selectable readout ("Selectable readout"): SPARCH_RED_*
READOUT_MODES = {"softmax_sum": 0, "softmax_mean": 1, "u_max": 2, "u_mean": 3, "u_last": 4}


def readout_mode(readout):
    """readout (None or a name of READOUT_MODES) -> the C ABI's `red`; None is the default, "softmax_sum"."""
    if readout is None:
        return 0
    if not isinstance(readout, str) or readout not in READOUT_MODES:
        raise ValueError(f"sparch_amd: readout must be one of {', '.join(READOUT_MODES)} (got {readout!r})")
    return READOUT_MODES[readout]


def _check_per_step(pack):
    if pack is not None:
        raise ValueError("sparch_amd: the per-step readout has no packed form (per_step with pack)")


def _readout_variant(lay, red, mode, red_arg=None, state=None):
    """Which of the readout's entry points a pass runs, forward and backward alike: (the suffix behind
    sparch_readout_fwd / sparch_readout_bwd, the arguments behind the plain ones).  state: the stateful backward's
    (g_uT, g_u0) pointers; red: a reduction other than the softmax-sum (one entry for every layout) with red_arg, the
    tensor of u_max's steps; mode: the per-step form (its seq tensor and mode sit further in front, with the caller)."""
    if state is not None:
        return "_st", state
    if red != 0:
        return "_red", (red, ptr(red_arg), *lay.ptrs, lay.ragged_steps)
    if mode is not None:
        _check_per_step(lay.pack)
        return "_seq" + lay.suffix, lay.tail
    return lay.suffix, lay.tail


class ReadoutLayerFn(torch.autograd.Function):
    """x (B,T,K) -> out (B,C): softmax-sum readout (snns.py:793-825), or with cfg["readout"] another reduction over
    time (READOUT_MODES; the default issues exactly the calls it always did).

    With cfg["per_step"] ("prob" / "sum"; DESIGN.md section 6, "Per-step readout") -> (out, seq): seq (B,T,C) is
    softmax(u_t), or the running sum of `out` after every step; its gradient reaches the kernel as g_seq."""

    @staticmethod
    def forward(ctx, cfg, x, W, Wb, nw, nb, alpha, u0):
        _require_device(x, "input")
        _require_device(W, "layer parameters")
        B, T, K = x.shape
        C = W.shape[0]
        if C > 256:
            raise ValueError(f"sparch_amd: the readout kernels handle at most 256 classes (got {C})")
        inp = _layer_input(cfg, x, gated=False)
        lay = SeqLayout.of_cfg(cfg)  # (packed: x is the (1, n, K) batch, out and u0 hold the plan's sorted rows)
        Wx_in, scale, shift, nsaved, Wx_raw = _project(inp, W, Wb, nw, nb, cfg, 1,
                                                       n_valid=lay.n_valid(B, T))  # snns.py:796, 799-801
        Bk, Tk = lay.index(B, T)
        out = torch.empty(Bk, C, dtype=torch.float32, device=x.device)
        u_save = torch.empty(B, T, C, dtype=torch.float32, device=x.device)
        mode = seq_mode(cfg.get("per_step"))
        red = readout_mode(cfg.get("readout"))
        if red != 0 and mode is not None:
            raise ValueError("sparch_amd: per_step needs the default readout (softmax_sum)")
        ctx.red_arg = None
        if red == READOUT_MODES["u_max"]:  # the step of each maximum: the backward reads it
            ctx.red_arg = torch.empty(Bk, C, dtype=torch.int32, device=x.device)
        variant, extra = _readout_variant(lay, red, mode, ctx.red_arg)
        seq_args = ()
        if mode is not None:
            seq = torch.empty(B, T, C, dtype=torch.float32, device=x.device)  # (every element is written: no clear)
            seq_args = (ptr(seq), mode)
            ctx.set_materialize_grads(False)  # a loss on one of the two outputs: no zero tensor for the other
        entry = "sparch_readout_fwd" + variant
        check(getattr(lib, entry)(Bk, Tk, C, ptr(Wx_in), ptr(scale), ptr(shift), ptr(alpha), ptr(u0), ptr(out),
                                  ptr(u_save), *seq_args, *extra, _stream()), entry)
        ctx.cfg, ctx.inp, ctx.lay = cfg, inp, lay
        ctx.shape = (B, T, K, C)
        ctx.nsaved = nsaved
        ctx.save_for_backward(inp.x2, W, nw, alpha, u0, u_save, Wx_raw)
        if cfg.get("stateful"):  # (out, u_T): the final membrane is the last saved step; its gradient comes back as g_uT
            if variant:
                raise ValueError("sparch_amd: the stateful readout is the plain softmax-sum's")
            ctx.set_materialize_grads(False)
            return out, u_save[:, T - 1].contiguous()
        return out if mode is None else (out, seq)

    @staticmethod
    def backward(ctx, g_out, g_seq=None):
        cfg, lay = ctx.cfg, ctx.lay
        norm = cfg["normalization"]
        B, T, K, C = ctx.shape
        x2, W, nw, alpha, u0, u_save, Wx_raw = ctx.saved_tensors
        dev = x2.device
        state, g_u0 = None, None
        mode = seq_mode(cfg.get("per_step"))
        if g_seq is None:
            mode = None  # nothing came back through seq: the plain kernels
        dWx = torch.empty(B, T, C, dtype=torch.float32, device=dev)
        fuse = norm == "batchnorm"
        Bk, Tk = lay.index(B, T)  # (the kernels' B and T: packed, the sequences and the longest of them)
        if cfg.get("stateful"):  # the second output was u_T, not seq
            g_uT, mode = (None if g_seq is None else _f32c(g_seq)), None
            if ctx.needs_input_grad[7]:
                g_u0 = torch.empty(Bk, C, dtype=torch.float32, device=dev)
            state = (ptr(g_uT), ptr(g_u0))
        if g_out is None and mode is None:
            g_out = torch.zeros(B, C, dtype=torch.float32, device=dev)
        g_out = None if g_out is None else _f32c(g_out)
        ws = torch.empty(3 if fuse else 1, Bk, C, dtype=torch.float32, device=dev)
        variant, extra = _readout_variant(lay, readout_mode(cfg.get("readout")), mode, ctx.red_arg, state)
        seq_args = () if mode is None else (ptr(_f32c(g_seq)), mode)
        entry = "sparch_readout_bwd" + variant
        check(getattr(lib, entry)(Bk, Tk, C, ptr(g_out), *seq_args, ptr(Wx_raw) if fuse else None,
                                  ptr(ctx.nsaved[0]) if fuse else None, ptr(ctx.nsaved[1]) if fuse else None, ptr(u_save),
                                  ptr(alpha), ptr(u0), ptr(dWx), ptr(ws), *extra, _stream()), entry)
        if fuse:  # dalpha and BatchNorm's two column sums: one launch
            dalpha, s1, s2 = _finish_param_grads(ws, Bk, C, [alpha, None, None], [ALPHA_LIM, (0.0, 0.0), (0.0, 0.0)])
            sums = (s1, s2)
        else:
            (dalpha,) = _finish_param_grads(ws, Bk, C, [alpha], [ALPHA_LIM])
            sums = None
        dx, dW, dWb, dnw, dnb = _project_backward(ctx.inp, W, nw, cfg, ctx.nsaved, Wx_raw, dWx.view(B * T, C),
                                                  need_dx=ctx.needs_input_grad[1], need_bias=ctx.needs_input_grad[3],
                                                  sums=sums, n_valid=lay.n_valid(B, T))
        dx = None if dx is None else dx.view(*ctx.shape[:3])
        ctx.inp = None
        return None, dx, dW, dWb, dnw, dnb, dalpha, g_u0


class SpikingCellFn(torch.autograd.Function):
    """A cell in isolation: Wx (B',T,H) already projected/normalised -> spikes (B',T,H).
    Mirrors the reference's `_lif_cell`/`_adlif_cell`/`_rlif_cell`/`_radlif_cell` methods."""

    @staticmethod
    def forward(ctx, kind, theta, Wx, alpha, beta, a, b, V, u0, w0, s0, steps_per_launch=None, surrogate=None):
        _require_device(Wx, "Wx")
        Wx = _f32c(Wx)
        Bp, T, H = Wx.shape
        p = {k_: v for k_, v in dict(alpha=alpha, beta=beta, a=a, b=b, V=V).items() if v is not None}
        s, _, saved, _ = cell_forward(kind, Wx, None, None, p, u0, w0, s0, B=Bp, dirs=1, theta=theta, p_drop=0.0,
                                      seed=0, steps_per_launch=steps_per_launch, want_saves=any(ctx.needs_input_grad),
                                      surrogate=surrogate)
        ctx.kind, ctx.theta, ctx.dims, ctx.cell_saved, ctx.spl = kind, theta, (Bp, T, H), saved, steps_per_launch
        ctx.surrogate = surrogate
        ctx.save_for_backward(alpha, beta, a, b, V, u0, w0, s0)
        return s

    @staticmethod
    def backward(ctx, g_s):
        alpha, beta, a, b, V, u0, w0, s0 = ctx.saved_tensors
        Bp, T, H = ctx.dims
        p = {k_: v for k_, v in dict(alpha=alpha, beta=beta, a=a, b=b, V=V).items() if v is not None}
        dWx, pg = cell_backward(ctx.kind, _f32c(g_s), None, p, u0, w0, s0, ctx.cell_saved, B=Bp, dirs=1, T=T,
                                H=H, theta=ctx.theta, p_drop=0.0, seed=0, steps_per_launch=ctx.spl,
                                surrogate=ctx.surrogate)
        return (None, None, dWx, pg.get("alpha"), pg.get("beta"), pg.get("a"), pg.get("b"), pg.get("V"),
                None, None, None, None, None)


class ReadoutCellFn(torch.autograd.Function):
    """The readout cell in isolation (reference `_readout_cell`, snns.py:808-825); readout: a name of READOUT_MODES."""

    @staticmethod
    def forward(ctx, Wx, alpha, u0, readout=None):
        red = readout_mode(readout)
        _require_device(Wx, "Wx")
        Wx = _f32c(Wx)
        B, T, C = Wx.shape
        if C > 256:
            raise ValueError(f"sparch_amd: the readout kernels handle at most 256 classes (got {C})")
        out = torch.empty(B, C, dtype=torch.float32, device=Wx.device)
        u_save = torch.empty(B, T, C, dtype=torch.float32, device=Wx.device)
        ctx.red, ctx.red_arg = red, None
        if red == READOUT_MODES["u_max"]:
            ctx.red_arg = torch.empty(B, C, dtype=torch.int32, device=Wx.device)
        variant, extra = _readout_variant(_DENSE, red, None, ctx.red_arg)
        check(getattr(lib, "sparch_readout_fwd" + variant)(B, T, C, ptr(Wx), None, None, ptr(alpha), ptr(u0), ptr(out),
                                                           ptr(u_save), *extra, _stream()), "sparch_readout_fwd" + variant)
        ctx.dims = (B, T, C)
        ctx.save_for_backward(alpha, u0, u_save)
        return out

    @staticmethod
    def backward(ctx, g_out):
        alpha, u0, u_save = ctx.saved_tensors
        B, T, C = ctx.dims
        dWx = torch.empty(B, T, C, dtype=torch.float32, device=g_out.device)
        ws = torch.empty(1, B, C, dtype=torch.float32, device=g_out.device)
        variant, extra = _readout_variant(_DENSE, ctx.red, None, ctx.red_arg)
        check(getattr(lib, "sparch_readout_bwd" + variant)(B, T, C, ptr(_f32c(g_out)), None, None, None, ptr(u_save),
                                                           ptr(alpha), ptr(u0), ptr(dWx), ptr(ws), *extra, _stream()),
              "sparch_readout_bwd" + variant)
        (dalpha,) = _finish_param_grads(ws, B, C, [alpha], [ALPHA_LIM])
        return dWx, dalpha, None, None


class CrossEntropyFn(torch.autograd.Function):
    """nn.CrossEntropyLoss()(output, y) of the train step (exp.py:100, 362; mean reduction) with its gradient, in
    one launch (`sparch_ce_loss`): eager torch runs seven small kernels for it per step."""

    @staticmethod
    def forward(ctx, logits, labels):
        _require_device(logits, "logits")
        _require_device(labels, "labels")
        logits = _f32c(logits)
        B, C = logits.shape
        loss = torch.empty(1, dtype=torch.float32, device=logits.device)
        dlogits = torch.empty_like(logits)
        check(lib.sparch_ce_loss(B, C, ptr(logits), ptr(labels.contiguous()), ptr(loss), ptr(dlogits), _stream()),
              "sparch_ce_loss")
        ctx.save_for_backward(dlogits)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None


def cross_entropy(logits, labels):
    """Mean cross-entropy of (B,C) logits against int64 class labels on the device (see CrossEntropyFn)."""
    if labels.dtype != torch.int64 or logits.ndim != 2:
        return torch.nn.functional.cross_entropy(logits, labels)
    return CrossEntropyFn.apply(logits, labels)


class CrossEntropyLoss(torch.nn.Module):
    """Drop-in for the reference's `nn.CrossEntropyLoss()` (exp.py:100) on the HIP path."""

    def forward(self, output, target):
        return cross_entropy(output, target)


def fbank(wave, num_mel_bins=40):
    """Kaldi-style log-mel filterbank of (clips, samples) fp32 audio on the device
    (replaces torchaudio.compliance.kaldi.fbank at nonspiking_datasets.py:96,194)."""
    _require_device(wave, "waveform")
    wave = _f32c(wave)
    if wave.ndim == 1:
        wave = wave[None]
    n_clips, n_samples = wave.shape
    frames = lib.sparch_fbank_frames(n_samples)
    out = torch.empty(n_clips, frames, num_mel_bins, dtype=torch.float32, device=wave.device)
    tok = timer.start(f"fbank[{n_clips}x{n_samples}]")
    check(lib.sparch_fbank_fwd(n_clips, n_samples, num_mel_bins, ptr(wave), ptr(out), _stream()),
          "sparch_fbank_fwd")
    timer.stop(tok)
    return out


def fbank_padded(wave, lengths, num_mel_bins=40):
    """Log-mel features of clips of different lengths, padded as the reference's HD / SC collate pads them
    (kaldi.fbank per clip, then pad_sequence: nonspiking_datasets.py:96-111, 194-209).

    wave: (B, ld) device tensor, fp32 in [-1, 1] or int16 PCM (scaled by 2^-15 in the kernel; the same bits as the
    fp32 path on pcm / 32768); clip i is wave[i, :lengths[i]].  lengths: B host ints or a tensor (samples).
    Returns (feats (B, T_max, num_mel_bins) fp32 on the device, frames (B,) int64 on the host): clip i's frames
    t < frames[i] are fbank(wave[i, :lengths[i]]) bit for bit, the later ones exactly 0; T_max = frames.max().
    Raises ValueError when a length exceeds ld or when no clip reaches one frame (400 samples)."""
    _require_device(wave, "waveform")
    if wave.ndim != 2:
        raise ValueError(f"fbank_padded: wave must be (clips, samples), got shape {tuple(wave.shape)}")
    if wave.dtype == torch.int16:
        in_dtype, wave = 1, wave.contiguous()
    else:
        in_dtype, wave = 0, _f32c(wave)
    n_clips, ld = wave.shape
    lens = torch.as_tensor(lengths).detach().to("cpu", torch.int64).reshape(-1)
    if lens.numel() != n_clips:
        raise ValueError(f"fbank_padded: {lens.numel()} lengths for {n_clips} clips")
    if n_clips and int(lens.max()) > ld:
        raise ValueError(f"fbank_padded: a clip length {int(lens.max())} exceeds the row length {ld}")
    # sparch_fbank_frames over the batch (400-sample frames every 160 samples); the library's own count of the
    # longest clip is T_max, and the two must agree
    n = lens.clamp(min=0)
    frames = torch.where(n < 400, torch.zeros_like(n), 1 + torch.div(n - 400, 160, rounding_mode="floor"))
    n_frames = lib.sparch_fbank_frames(int(n.max())) if n_clips else 0
    if n_clips and int(frames.max()) != n_frames:
        raise RuntimeError(f"fbank_padded: frame count {int(frames.max())} differs from the library's {n_frames}")
    if n_frames == 0:
        raise ValueError("fbank_padded: no clip is long enough for one frame (400 samples)")
    # from pinned memory without blocking the host: the caching host allocator does not hand the block out again
    # before the copy has completed
    lens_dev = lens.to(torch.int32).pin_memory().to(wave.device, non_blocking=True)
    out = torch.empty(n_clips, n_frames, num_mel_bins, dtype=torch.float32, device=wave.device)
    tok = timer.start(f"fbank_padded[{n_clips}x{ld}]")
    check(lib.sparch_fbank_padded_fwd(n_clips, ld, ptr(lens_dev), n_frames, num_mel_bins, in_dtype, ptr(wave),
                                      ptr(out), _stream()), "sparch_fbank_padded_fwd")
    timer.stop(tok)
    return out, frames


AUGM_FIELDS = 9  # SPARCH_AUGM_FIELDS


def _augm_table(params, n_clips, sample_rate, what):
    """The (n_clips, AUGM_FIELDS) table of draws as a contiguous host fp32 tensor, or ValueError for an entry out of
    range (shared by `augment_padded` and `AudioStore.gather_augment`)."""
    table = torch.as_tensor(params).detach().to("cpu", torch.float32).contiguous()
    if tuple(table.shape) != (n_clips, AUGM_FIELDS):
        raise ValueError(f"{what}: params must be ({n_clips}, {AUGM_FIELDS}), got {tuple(table.shape)}")
    flags, u, ratio, rds = table[:, :4], table[:, 4], table[:, 5], table[:, 6:]
    if not bool(((flags == 0) | (flags == 1)).all()):
        raise ValueError(f"{what}: stage flags must be 0 or 1")
    # u in [0, 1): random.random() rounded to fp32, which rounds up to 1.0 for the last 2^-25 of the range
    if not bool(((u >= 0) & (u <= 1)).all()):
        raise ValueError(f"{what}: the noise uniform must lie in [0, 1)")
    if not bool(torch.isfinite(ratio).all()):
        raise ValueError(f"{what}: the gain ratio must be finite")
    if not bool(((rds >= 0) & (rds <= 100)).all()):
        raise ValueError(f"{what}: reverberance, HF damping and room scale must lie in [0, 100]")
    if not 8000 <= int(sample_rate) <= 48000:
        raise ValueError(f"{what}: sample rate {sample_rate} outside 8000-48000 Hz")
    return table


def augment_padded(wave, lengths, params, noise_seed, min_snr, max_snr, sample_rate=16000):
    """Waveform augmentation of padded clips on the device (sparch_augment_padded): the reference's training-split
    transforms (torchaudio_augmentations' PolarityInversion, Noise, Gain and sox's reverb, nonspiking_datasets.py:71-78,
    170-177), restated (DESIGN.md §4 "augment", parity unpinned), with the per-clip decisions and values drawn on the
    host (`dataloaders.augment.draw_augmentation`).

    wave: (B, ld) device tensor, fp32 or int16 PCM (scaled by 2^-15); clip i is wave[i, :lengths[i]].  lengths: B host
    ints or a tensor (a negative length counts as 0).  params: (B, AUGM_FIELDS) host table, per clip the polarity,
    noise, gain and reverb flags (0 / 1), the noise uniform u, the gain ratio, reverberance, HF damping and room scale
    in [0, 100].  noise_seed: key of the noise stream; min_snr / max_snr: the Noise bounds; sample_rate: what sox is
    told (the reference passes 16000 for every clip).
    Returns a fresh fp32 (B, ld) device tensor: row i holds the augmented clip in [:lengths[i]] and is not written
    after it.  Raises ValueError for a length past ld or a table entry out of range."""
    _require_device(wave, "waveform")
    if wave.ndim != 2:
        raise ValueError(f"augment_padded: wave must be (clips, samples), got shape {tuple(wave.shape)}")
    if wave.dtype == torch.int16:
        in_dtype, wave = 1, wave.contiguous()
    else:
        in_dtype, wave = 0, _f32c(wave)
    n_clips, ld = wave.shape
    lens = torch.as_tensor(lengths).detach().to("cpu", torch.int64).reshape(-1)
    if lens.numel() != n_clips:
        raise ValueError(f"augment_padded: {lens.numel()} lengths for {n_clips} clips")
    if n_clips and int(lens.max()) > ld:
        raise ValueError(f"augment_padded: a clip length {int(lens.max())} exceeds the row length {ld}")
    table = _augm_table(params, n_clips, sample_rate, "augment_padded")
    dev = wave.device
    # from pinned memory without blocking the host (the caching host allocator keeps the blocks until the copies
    # are done)
    lens_dev = lens.to(torch.int32).pin_memory().to(dev, non_blocking=True)
    table_dev = table.pin_memory().to(dev, non_blocking=True)
    out = torch.empty(n_clips, ld, dtype=torch.float32, device=dev)
    tok = timer.start(f"augment_padded[{n_clips}x{ld}]")
    check(lib.sparch_augment_padded(n_clips, ld, ptr(lens_dev), in_dtype, ptr(wave), ptr(table_dev), float(min_snr),
                                    float(max_snr), int(noise_seed) & (2 ** 64 - 1), int(sample_rate), ptr(out),
                                    _stream()), "sparch_augment_padded")
    timer.stop(tok)
    return out


FLAC_CLIP_FIELDS = 13  # SPARCH_FLAC_CLIP_FIELDS
FLAC_REASONS = {1: "inconsistent clip table entry", 2: "no valid frame header where the previous frame ended",
                3: "invalid subframe or residual coding", 4: "truncated: a frame runs past the end of the file",
                5: "frame CRC-16 mismatch", 6: "the frames do not add up to the STREAMINFO sample count"}


def flac_pack(streams, infos, rows, n_rows, ld, int16):
    """Host half of `flac_decode_padded`: (pinned uint8 tensor of the streams, each at a 4-aligned offset; clip
    table (n, FLAC_CLIP_FIELDS) int64; slot count; scratch int32 count), checked against an (n_rows, ld) output."""
    import numpy as np

    n = len(streams)
    if n == 0 or len(infos) != n or len(rows) != n:
        raise ValueError("flac_decode_padded: one descriptor and one row per stream, at least one stream")
    sizes = [len(s) for s in streams]
    begins = np.zeros(n + 1, np.int64)
    begins[1:] = np.cumsum([(z + 3) & ~3 for z in sizes])
    table = np.zeros((n, FLAC_CLIP_FIELDS), np.int64)
    slot_base = scratch_base = 0
    for k, (info, row) in enumerate(zip(infos, rows)):
        if info is None or not 0 <= row < n_rows or info.total_samples > ld:
            raise ValueError(f"flac_decode_padded: stream {k}: no descriptor, row {row} outside {n_rows} rows, or "
                             f"{getattr(info, 'total_samples', '?')} samples exceed the row length {ld}")
        if int16 and info.bps != 16:
            raise ValueError(f"flac_decode_padded: stream {k} has {info.bps}-bit samples; int16 rows take 16 bits")
        slots = -(-info.total_samples // info.min_block)                  # frames <= ceil(total / min block)
        scratch = slots * info.max_block if info.channels == 2 else 0
        table[k] = (begins[k], begins[k] + sizes[k], begins[k] + info.first_frame, info.total_samples, row,
                    info.sample_rate, info.channels, info.bps, info.min_block, info.max_block, slot_base, slots,
                    scratch_base)
        slot_base += slots
        scratch_base += scratch
    host = torch.empty(int(begins[-1]), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    buf = host.numpy()
    for k, s in enumerate(streams):
        buf[begins[k]:begins[k] + sizes[k]] = np.frombuffer(s, np.uint8)
        buf[begins[k] + sizes[k]:begins[k + 1]] = 0
    return host, table, slot_base, scratch_base


def flac_decode_padded(streams, infos, wave, rows=None):
    """Decode FLAC streams on the device into rows of `wave` (sparch_flac_decode_padded).

    streams: file contents (bytes); infos: their `dataloaders.audio.parse_flac` descriptors; wave: (R, ld) device
    tensor, fp32 (x * 2^-(bps-1)) or int16 (16-bit streams only); rows: the row of each stream (default 0, 1, ...).
    Channel 0 of stream k fills wave[rows[k], :total_samples]; nothing else of `wave` is written.  The file bytes go
    up in one pinned copy.  Returns the device error record (2,) int64 without synchronising: read it with
    `flac_error_message` once the stream has reached it."""
    _require_device(wave, "waveform")
    if wave.ndim != 2 or not wave.is_contiguous() or wave.dtype not in (torch.float32, torch.int16):
        raise ValueError("flac_decode_padded: wave must be a contiguous (rows, samples) fp32 or int16 tensor")
    n_rows, ld = wave.shape
    rows = list(range(len(streams))) if rows is None else [int(r) for r in rows]
    int16 = wave.dtype == torch.int16
    host, table, n_slots, n_scratch = flac_pack(streams, infos, rows, n_rows, ld, int16)
    dev = wave.device
    # from pinned memory without blocking the host (the caching host allocator keeps both blocks until the copies
    # are done)
    bytes_d = host.to(dev, non_blocking=True)
    table_d = torch.from_numpy(table).pin_memory().to(dev, non_blocking=True)
    ws_bytes = lib.sparch_flac_workspace_bytes(n_slots, n_scratch)
    if ws_bytes == 0:
        raise ValueError(f"flac_decode_padded: workspace of {n_slots} frame slots out of range")
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    err = torch.empty(2, dtype=torch.int64, device=dev)
    tok = timer.start(f"flac_decode_padded[{len(streams)}x{ld}]")
    check(lib.sparch_flac_decode_padded(len(streams), ptr(table_d), ptr(bytes_d), host.numel(), n_slots, n_scratch,
                                        n_rows, ld, 1 if int16 else 0, ptr(wave), ptr(err), ptr(ws), ws_bytes,
                                        _stream()), "sparch_flac_decode_padded")
    timer.stop(tok)
    return err


def flac_error_message(record, names):
    """Text of a `flac_decode_padded` error record (a host copy) naming the failing file of `names` (the streams in
    the order they were passed), or None when every stream decoded."""
    count, key = (int(v) for v in record)
    if count == 0:
        return None
    key &= (1 << 64) - 1
    clip, frame, reason = key >> 32, (key >> 8) & 0xFFFFFF, key & 0xFF
    msg = f"{names[clip]}: FLAC frame {frame}: {FLAC_REASONS.get(reason, f'reason {reason}')}"
    return msg + (f" ({count - 1} more file(s) of the batch failed)" if count > 1 else "")


def bin_events(times, units, nb_steps=100, nb_units=700, max_time=1.4, device="cuda"):
    """Batch of event lists -> dense (B, nb_steps, nb_units) float32 spike counts on the device, as the
    reference's SpikingDataset.__getitem__ builds them per sample on the CPU (spiking_datasets.py:66-78).
    times / units: sequences (one entry per sample) of 1-D arrays or tensors.  Returns (x, n_dropped) where
    n_dropped is a device int32 tensor counting events the reference would have rejected."""
    import numpy as np

    lens = [len(t) for t in times]
    if len(lens) == 0 or len(units) != len(lens):
        raise ValueError("bin_events: times and units must be non-empty sequences of equal length")
    offs = torch.zeros(len(lens) + 1, dtype=torch.int64)
    offs[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int64), 0)
    n = int(offs[-1])
    t_all = torch.from_numpy(np.concatenate([np.asarray(t, np.float32).ravel() for t in times]).astype(np.float32)) \
        if n else torch.zeros(0, dtype=torch.float32)
    u_all = torch.from_numpy(np.concatenate([np.asarray(u).ravel() for u in units]).astype(np.int32)) \
        if n else torch.zeros(0, dtype=torch.int32)
    dev = torch.device(device)
    t_d, u_d, o_d = t_all.to(dev), u_all.to(dev), offs.to(dev)
    out = torch.empty(len(lens), nb_steps, nb_units, dtype=torch.float32, device=dev)
    dropped = torch.empty(4, dtype=torch.int32, device=dev)
    check(lib.sparch_bin_events(n, ptr(t_d) if n else None, ptr(u_d) if n else None, ptr(o_d), len(lens), nb_steps,
                                nb_units, float(max_time), ptr(out), ptr(dropped), _stream()), "sparch_bin_events")
    return out, dropped[:1]


# ----------------------------------------------------------------------------- resident SHD / SSC events
EVENT_PACK_KEYS = ("times", "units", "offsets", "labels")
_UNIT_DROPPED = 0xFFFF  # stored for a unit that is negative or does not fit 16 bits: still counted as dropped


def event_arrays_from_mapping(h5):
    """The contents of an SHD / SSC file — any mapping with ["spikes"]["times"], ["spikes"]["units"] (one
    variable-length row per sample) and ["labels"], an open h5py file included — as the four flat arrays of an
    event store: times (float16 or float32 as the source had them; anything else, float64 included, rounded to
    float32 as SpikingDataset.__getitem__ does), units (uint16, 0xFFFF for a unit that is negative or does not
    fit), offsets (int64, n + 1), labels (int64, n)."""
    import numpy as np

    labels = np.array(h5["labels"], dtype=np.int64).ravel()
    rows_t, rows_u = h5["spikes"]["times"], h5["spikes"]["units"]
    n = len(labels)
    ts = [np.asarray(rows_t[i]).ravel() for i in range(n)]
    us = [np.asarray(rows_u[i]).ravel() for i in range(n)]
    lens = np.array([len(t) for t in ts], dtype=np.int64)
    if any(len(u) != m for u, m in zip(us, lens)):
        raise ValueError("event store: a sample has different numbers of times and units")
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    keep16 = n > 0 and all(t.dtype == np.float16 for t in ts)
    tdt = np.float16 if keep16 else np.float32
    times = np.concatenate([t.astype(tdt, copy=False) for t in ts]) if n and offsets[-1] else np.zeros(0, tdt)
    u = np.concatenate([x.astype(np.int64, copy=False) for x in us]) if n and offsets[-1] else np.zeros(0, np.int64)
    units = np.where((u < 0) | (u >= _UNIT_DROPPED), _UNIT_DROPPED, u).astype(np.uint16)
    return {"times": times, "units": units, "offsets": offsets, "labels": labels}


def check_event_arrays(a, what="event store"):
    """ValueError unless the four arrays agree (host-side; the kernel trusts the offsets)."""
    import numpy as np

    for k in EVENT_PACK_KEYS:
        if k not in a:
            raise ValueError(f"{what}: array '{k}' is missing")
    t, u, o, y = (np.asarray(a[k]) for k in EVENT_PACK_KEYS)
    if t.dtype not in (np.float16, np.float32) or u.dtype != np.uint16 or o.dtype != np.int64 or y.dtype != np.int64:
        raise ValueError(f"{what}: dtypes must be float16/float32, uint16, int64, int64; got "
                         f"{t.dtype}, {u.dtype}, {o.dtype}, {y.dtype}")
    if t.ndim != 1 or u.ndim != 1 or o.ndim != 1 or y.ndim != 1:
        raise ValueError(f"{what}: the arrays must be one-dimensional")
    if len(y) == 0:
        raise ValueError(f"{what}: no samples")
    if len(o) != len(y) + 1:
        raise ValueError(f"{what}: {len(y)} labels need {len(y) + 1} offsets, found {len(o)}")
    if o[0] != 0 or np.any(np.diff(o) < 0):
        raise ValueError(f"{what}: offsets must start at 0 and never decrease")
    if len(t) != len(u) or int(o[-1]) != len(t):
        raise ValueError(f"{what}: the last offset ({int(o[-1])}) is not the number of events "
                         f"({len(t)} times, {len(u)} units)")
    return {"times": t, "units": u, "offsets": o, "labels": y}


def save_event_pack(path, arrays):
    """Write the pack file of a split: an uncompressed np.savez of times, units, offsets, labels."""
    import numpy as np

    a = check_event_arrays(arrays, what=str(path))
    with open(path, "wb") as f:  # a file object: np.savez would append ".npz" to a name
        np.savez(f, **a)


def load_event_pack(path):
    import numpy as np

    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in EVENT_PACK_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: not an event pack (no {', '.join(missing)})")
        return check_event_arrays({k: z[k] for k in EVENT_PACK_KEYS}, what=str(path))


def _samples_sorted(times, offsets):
    """True iff the times of every sample are non-decreasing (NaN counts as unsorted)."""
    import numpy as np

    if len(times) < 2:
        return True
    ok = times[1:] >= times[:-1]
    starts = offsets[1:-1]                       # pairs (s - 1, s) that straddle two samples do not count
    starts = starts[(starts > 0) & (starts < len(times))]
    ok[starts - 1] = True
    return bool(ok.all())


def _require_room(need, free, what, kind="event", env="SPARCH_EVENTS"):
    if need > free:
        raise RuntimeError(f"{what}: the {kind} store needs {need / 2**20:.1f} MiB on the device, only "
                           f"{free / 2**20:.1f} MiB are free; train without {env}=resident")


class EventStore:
    """All events of one SHD / SSC split on the device, uploaded once; `batch(idx)` then builds a batch from a device
    list of sample indices in one launch (`sparch_events_gather_bin`).

    Built from the four flat arrays (`event_arrays_from_mapping`, `load_event_pack`), or through `from_mapping` /
    `from_pack`.  `prepare(nb_steps)` bins the whole store once on the device and keeps the largest count of any
    (sample, bin, unit): up to 255 the store serves the bf16 plane layer 1 reads, wrapped as `input_from_counts`
    wraps it; above, dense fp32 as the per-sample loader does.  The decision is taken once, on the host."""

    def __init__(self, arrays, device="cuda", nb_units=700, max_time=1.4):
        import numpy as np

        a = check_event_arrays(arrays)
        if not 0 < nb_units <= 65535:
            raise ValueError(f"EventStore: nb_units {nb_units} outside 1..65535 (units are stored in 16 bits)")
        self.device = torch.device(device)
        _require_device(torch.empty(0, device=self.device), "EventStore")
        self.nb_units, self.max_time = int(nb_units), float(max_time)
        self.n_samples, self.n_events = len(a["labels"]), len(a["times"])
        self.sorted = _samples_sorted(a["times"], a["offsets"])
        self.nbytes = sum(int(v.nbytes) for v in a.values())
        _require_room(self.nbytes, torch.cuda.mem_get_info(self.device)[0], "EventStore")
        # an empty store array still needs an address for the kernel's argument check
        pad = {k: (v if len(v) else np.zeros(1, v.dtype)) for k, v in a.items()}
        self.times = torch.from_numpy(pad["times"]).to(self.device)
        self.units = torch.from_numpy(pad["units"].view("int16")).to(self.device)  # bits; torch has no uint16 maths
        self.offsets = torch.from_numpy(pad["offsets"]).to(self.device)
        self.labels = torch.from_numpy(pad["labels"]).to(self.device)
        self.times_dtype = 1 if a["times"].dtype.itemsize == 2 else 0
        self._max_count = {}    # nb_steps -> largest bin count of the store
        self._dropped = {}      # nb_steps -> events dropped over the whole store

    @classmethod
    def from_mapping(cls, h5, **kw):
        return cls(event_arrays_from_mapping(h5), **kw)

    @classmethod
    def from_pack(cls, path, **kw):
        return cls(load_event_pack(path), **kw)

    def __len__(self):
        return self.n_samples

    def upload_augmentation(self, table):
        """A host augmentation table ((n, 8): `dataloaders.event_augment`) checked and copied to the store's device in
        one copy; row slices of the result are what `gather(..., augment=(rows, seed))` takes without another check.
        ValueError for a table the kernel's contract does not allow."""
        from .dataloaders.event_augment import check_event_augmentation

        if isinstance(table, torch.Tensor):
            table = table.detach().cpu().numpy()
        return torch.from_numpy(check_event_augmentation(table)).to(self.device)

    def _augment_rows(self, augment, B):
        """(device (B, 8) fp32 rows, seed) of a gather's `augment` argument.  A host table (numpy array, list, CPU
        tensor) is validated and uploaded; a device tensor is one `upload_augmentation` has checked."""
        from .dataloaders.event_augment import EVAUG_FIELDS

        try:
            table, seed = augment
            seed = int(seed)
        except (TypeError, ValueError):
            raise ValueError("EventStore: augment must be a pair (table, seed)") from None
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f"EventStore: augmentation seed {seed} outside 0..2^64-1")
        if not (isinstance(table, torch.Tensor) and table.is_cuda):
            table = self.upload_augmentation(table)
        if (table.dtype != torch.float32 or tuple(table.shape) != (B, EVAUG_FIELDS) or not table.is_contiguous()):
            raise ValueError(f"EventStore: the augmentation table must be contiguous float32 of shape ({B}, "
                             f"{EVAUG_FIELDS}), found {table.dtype} {tuple(table.shape)}")
        return table, seed

    def _launch(self, idx, nb_steps, plane=None, dense=None, counts=None, y=None, n_dropped=None, augment=None):
        B = idx.numel()
        ws, ws_bytes = None, 0
        if n_dropped is not None:
            ws_bytes = lib.sparch_events_gather_bin_workspace_bytes(B, nb_steps, self.nb_units)
            ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=self.device)
        args = (ptr(self.times), self.times_dtype, ptr(self.units), ptr(self.offsets), ptr(self.labels),
                self.n_samples, ptr(idx), B, nb_steps, self.nb_units, self.max_time, int(self.sorted), ptr(plane),
                ptr(dense), ptr(counts), ptr(y), ptr(n_dropped), ptr(ws), ws_bytes)
        if augment is None:
            tok = timer.start(f"events_gather_bin[{B}x{nb_steps}x{self.nb_units}]")
            check(lib.sparch_events_gather_bin(*args, _stream()), "sparch_events_gather_bin")
        else:
            tok = timer.start(f"events_gather_bin_aug[{B}x{nb_steps}x{self.nb_units}]")
            check(lib.sparch_events_gather_bin_aug(*args, ptr(augment[0]), augment[1], _stream()),
                  "sparch_events_gather_bin_aug")
        timer.stop(tok)

    def gather(self, idx, nb_steps, plane=False, dense=False, counts=False, dropped=False, augment=None):
        """Raw outputs of the kernel for the device int64 index list `idx`: a dict with 'y' and whichever of
        'plane' ((B * nb_steps, ldp) bf16), 'dense' ((B, nb_steps, K) fp32), 'counts' ((B, nb_steps, K) uint8,
        saturating) and 'n_dropped' (device int32, 1 element) were asked for.  augment = (table, seed): row b of
        the (B, 8) table transforms the events of batch row b inside the kernel (`sparch_events_gather_bin_aug`;
        `dataloaders.event_augment` draws such tables); a host table is validated here, before anything is
        launched (ValueError)."""
        _require_device(idx, "idx")
        if idx.dtype != torch.int64 or idx.ndim != 1 or idx.numel() == 0 or not idx.is_contiguous():
            raise ValueError("EventStore.gather: idx must be a non-empty contiguous 1-D int64 tensor")
        if not (plane or dense or counts):
            raise ValueError("EventStore.gather: ask for at least one of plane, dense, counts")
        B, K, dev = idx.numel(), self.nb_units, self.device
        if augment is not None:
            augment = self._augment_rows(augment, B)
        out = {"y": torch.empty(B, dtype=torch.int64, device=dev)}
        if plane:
            out["plane"] = torch.empty(B * nb_steps, (K + 7) // 8 * 8, dtype=torch.bfloat16, device=dev)
        if dense:
            out["dense"] = torch.empty(B, nb_steps, K, dtype=torch.float32, device=dev)
        if counts:
            out["counts"] = torch.empty(B, nb_steps, K, dtype=torch.uint8, device=dev)
        if dropped:
            out["n_dropped"] = torch.empty(4, dtype=torch.int32, device=dev)
        self._launch(idx, nb_steps, out.get("plane"), out.get("dense"), out.get("counts"), out["y"],
                     out.get("n_dropped"), augment)
        if dropped:
            out["n_dropped"] = out["n_dropped"][:1]
        return out

    def prepare(self, nb_steps, chunk=256):
        """Largest bin count over the whole store at nb_steps (found on the device, one read-back), cached."""
        if nb_steps not in self._max_count:
            top = torch.zeros((), dtype=torch.float32, device=self.device)
            lost = torch.zeros(1, dtype=torch.int64, device=self.device)
            for a in range(0, self.n_samples, chunk):
                idx = torch.arange(a, min(a + chunk, self.n_samples), dtype=torch.int64, device=self.device)
                got = self.gather(idx, nb_steps, dense=True, dropped=True)
                top = torch.maximum(top, got["dense"].max())
                lost += got["n_dropped"]
            self._max_count[nb_steps] = int(top.item())
            self._dropped[nb_steps] = int(lost.item())
        return self._max_count[nb_steps]

    def dropped(self, nb_steps):
        """Events of the whole store that the binning rejects (t < 0, t >= max_time, unit out of range)."""
        self.prepare(nb_steps)
        return self._dropped[nb_steps]

    def serves_plane(self, nb_steps, augment_scale=None):
        # the conditions under which layer 1 would read the plane of an fp32 batch (SpikingLayerFn.forward)
        if augment_scale is None:
            return DENSE_GEMM == "split6" and self.prepare(nb_steps) <= 255
        # augmented batches: time compression merges bins, so the store's largest count is no bound any more.  A bin
        # of t' = a * t + c covers at most ceil(1 / a) + 1 bins of t, a >= 1 - augment_scale, one more for the edges
        from .dataloaders.event_augment import plane_count_factor

        return DENSE_GEMM == "split6" and self.prepare(nb_steps) * plane_count_factor(augment_scale) <= 255

    def batch(self, idx, nb_steps, values=False, augment=None, augment_scale=None):
        """(x, y) on the device for the index list: x is the layer-1 input — the tagged placeholder of
        `input_from_counts` when the store serves the plane, dense fp32 (B, nb_steps, K) otherwise or when
        `values` asks for a tensor whose elements can be read (non-spiking networks).  augment: as `gather` takes
        it; `augment_scale` < 1 is then a bound of the table's time compression, a >= 1 - augment_scale (None: read
        from the table), which decides whether the counts still fit the plane."""
        if augment is not None:
            augment = self._augment_rows(augment, idx.numel())      # validated (and uploaded) before anything else
            if augment_scale is None:   # one read-back; a loader passes the bound of its spec instead
                augment_scale = max(0.0, 1.0 - float(augment[0][:, 1].min()))
        if not values and self.serves_plane(nb_steps, augment_scale if augment is not None else None):
            got = self.gather(idx, nb_steps, plane=True, augment=augment)
            B = idx.numel()
            key = str(self.device)
            one = _flag_one.get(key)
            if one is None:
                one = _flag_one[key] = torch.ones(4, dtype=torch.int32, device=self.device)
            x = spike_placeholder(B, nb_steps, self.nb_units, self.device).view(B, nb_steps, self.nb_units)
            x._sparch_input_plane = (tuple(x.shape), got["plane"], one)
            return x, got["y"]
        got = self.gather(idx, nb_steps, dense=True, augment=augment)
        return got["dense"], got["y"]


# ----------------------------------------------------------------------------- resident HD / SC audio
AUDIO_PACK_KEYS = ("samples", "starts", "lengths", "labels")
AUDIO_FLAC_CHUNK = 256  # FLAC clips decoded per launch while the arrays of a split are built


def check_audio_arrays(a, what="audio store"):
    """ValueError unless the four arrays of an audio store agree (host-side; the kernels trust them): samples int16
    or float32, starts int64, lengths int32, labels int64, one entry per clip in the last three; every clip
    [start, start + length) lies inside samples, and no two clips overlap."""
    import numpy as np

    for k in AUDIO_PACK_KEYS:
        if k not in a:
            raise ValueError(f"{what}: array '{k}' is missing")
    x, s, n, y = (np.asarray(a[k]) for k in AUDIO_PACK_KEYS)
    if x.dtype not in (np.int16, np.float32) or s.dtype != np.int64 or n.dtype != np.int32 or y.dtype != np.int64:
        raise ValueError(f"{what}: dtypes must be int16/float32, int64, int32, int64; got "
                         f"{x.dtype}, {s.dtype}, {n.dtype}, {y.dtype}")
    if x.ndim != 1 or s.ndim != 1 or n.ndim != 1 or y.ndim != 1:
        raise ValueError(f"{what}: the arrays must be one-dimensional")
    if len(y) == 0:
        raise ValueError(f"{what}: no clips")
    if not len(s) == len(n) == len(y):
        raise ValueError(f"{what}: starts, lengths and labels must have one length, found {len(s)}, {len(n)}, "
                         f"{len(y)}")
    if np.any(s < 0):
        raise ValueError(f"{what}: clip {int(np.argmax(s < 0))} has a negative start")
    if np.any(n < 0):
        raise ValueError(f"{what}: clip {int(np.argmax(n < 0))} has a negative length")
    end = s + n
    if np.any(end > len(x)):
        i = int(np.argmax(end > len(x)))
        raise ValueError(f"{what}: clip {i} ends at sample {int(end[i])}, past the end of samples ({len(x)})")
    live = np.flatnonzero(n > 0)                         # an empty clip overlaps nothing
    live = live[np.argsort(s[live], kind="stable")]
    clash = end[live][:-1] > s[live][1:]
    if np.any(clash):
        k = int(np.argmax(clash))
        raise ValueError(f"{what}: clips {int(live[k])} and {int(live[k + 1])} overlap")
    return {"samples": x, "starts": s, "lengths": n, "labels": y}


def save_audio_pack(path, arrays):
    """Write the pack file of a split: an uncompressed np.savez of samples, starts, lengths, labels."""
    import numpy as np

    a = check_audio_arrays(arrays, what=str(path))
    with open(path, "wb") as f:  # a file object: np.savez would append ".npz" to a name
        np.savez(f, **a)


def load_audio_pack(path):
    import numpy as np

    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in AUDIO_PACK_KEYS if k not in z.files]
        if missing:
            raise ValueError(f"{path}: not an audio pack (no {', '.join(missing)})")
        return check_audio_arrays({k: z[k] for k in AUDIO_PACK_KEYS}, what=str(path))


def audio_arrays_from_files(file_list, targets, device="cuda", sample_rate=16000, chunk=AUDIO_FLAC_CHUNK):
    """The clips `file_list` with labels `targets` as the four flat host arrays of an audio store, clip after clip
    without gaps (the kernels load single samples: nothing to align).  samples is int16 PCM when every clip is
    16-bit mono, else float32 in [-1, 1] for the whole split, each clip converted as the file loader's collate
    converts it (`dataloaders.audio`: int16 / 2^15, FLAC x * 2^-(bps-1)).  WAV clips are read on the host; FLAC clips
    are decoded on `device`, `chunk` clips per launch (`flac_decode_padded`), every chunk's error record and every
    mono clip's STREAMINFO MD5 checked (FlacError naming the file).  A tree with FLAC clips needs a device: this
    build decodes FLAC nowhere else (RuntimeError naming the first such file when none is visible).  Warns once when
    a clip's sample rate is not `sample_rate` (nothing is resampled).  The files are read twice (lengths and sample
    format first, samples second), so the host holds the flat array and one clip or FLAC chunk, not the split twice."""
    import logging

    import numpy as np

    from .dataloaders.audio import FlacError, FlacStream, flac_md5_ok, read_clip

    if len(file_list) != len(targets):
        raise ValueError(f"audio store: {len(file_list)} files, {len(targets)} labels")
    # two passes over the files, so that the host never holds more than the flat array and one clip (or one chunk of
    # FLAC files): the first finds every clip's length and whether the split is 16-bit mono throughout
    n = len(file_list)
    lengths, flac, pcm16, warned = np.zeros(n, np.int32), [], True, False
    for i, path in enumerate(file_list):
        clip, rate = read_clip(path)
        if rate != sample_rate and not warned:
            warned = True
            logging.getLogger(__name__).warning(
                f"{path}: sample rate {rate} Hz; the features assume {sample_rate} Hz and nothing is resampled (as "
                "in the reference). Warned once per dataset.")
        if isinstance(clip, FlacStream):
            flac.append(i)
            lengths[i] = clip.info.total_samples
            pcm16 = pcm16 and clip.info.bps == 16 and clip.info.channels == 1
        else:
            lengths[i] = len(clip)
            pcm16 = pcm16 and clip.dtype == np.int16
    if flac and (device is None or not torch.cuda.is_available()):
        raise RuntimeError(f"{file_list[flac[0]]}: FLAC clips are decoded on the device (this build has no host "
                           "FLAC decoder) and no HIP device is visible; build the audio store or its pack where "
                           "one is")
    starts = np.zeros(n, np.int64)
    np.cumsum(lengths[:-1], dtype=np.int64, out=starts[1:])
    samples = np.empty(int(lengths.sum(dtype=np.int64)), np.int16 if pcm16 else np.float32)

    def reread(i):
        clip, _ = read_clip(file_list[i])
        m = clip.info.total_samples if isinstance(clip, FlacStream) else len(clip)
        if m != lengths[i] or isinstance(clip, FlacStream) != (i in is_flac):
            raise ValueError(f"{file_list[i]}: the file changed while the audio store was built")
        return clip

    is_flac = set(flac)
    for i in range(n):
        if i not in is_flac:
            c = reread(i)
            samples[starts[i]:starts[i] + lengths[i]] = (
                c if pcm16 or c.dtype == np.float32 else c.astype(np.float32) / np.float32(2 ** 15))
    for at in range(0, len(flac), chunk):  # (a FLAC stream this build decodes has at least one sample: ld >= 1)
        part = flac[at:at + chunk]
        streams = [reread(i) for i in part]
        wave = torch.empty(len(part), int(lengths[part].max()), dtype=torch.int16 if pcm16 else torch.float32,
                           device=device)
        err = flac_decode_padded([c.data for c in streams], [c.info for c in streams], wave)
        msg = flac_error_message(err.cpu(), [c.path for c in streams])  # load time: synchronous anyway
        if msg:
            raise FlacError(msg)
        rows = wave.cpu().numpy()
        for row, i, c in zip(rows, part, streams):
            x = row[:lengths[i]]
            if c.info.channels == 1 and not flac_md5_ok(x, c.info):
                raise FlacError(f"{c.path}: decoded samples do not match the STREAMINFO MD5")
            samples[starts[i]:starts[i] + lengths[i]] = x
    return {"samples": samples, "starts": starts, "lengths": lengths, "labels": np.asarray(targets, np.int64)}


class AudioStore:
    """All clips of one HD / SC split on the device, uploaded once; `batch(idx, idx_host)` then builds the padded
    log-mel batch of the file loader's collate from a device list of clip indices: one launch
    (`sparch_audio_gather_fbank`), or two for an augmented split (`sparch_audio_gather_augment`, then
    `sparch_fbank_padded_fwd`).  The lengths stay on the host too: T_max and the frame counts of a batch are computed
    there, so a batch costs no synchronisation and no device-to-host read.

    Built from the four flat arrays (`audio_arrays_from_files`, `load_audio_pack`), or through `from_files` /
    `from_pack`; `source` says which, for the log."""

    def __init__(self, arrays, device="cuda", source="arrays"):
        import numpy as np

        a = check_audio_arrays(arrays)
        self.device = torch.device(device)
        _require_device(torch.empty(0, device=self.device), "AudioStore")
        self.n_clips, self.n_samples = len(a["labels"]), len(a["samples"])
        self.int16 = a["samples"].dtype == np.int16
        self.dtype = 1 if self.int16 else 0  # the kernels' `dtype` / `in_dtype`
        self.source = source
        self.nbytes = sum(int(v.nbytes) for v in a.values())
        _require_room(self.nbytes, torch.cuda.mem_get_info(self.device)[0], "AudioStore", "audio", "SPARCH_AUDIO")
        # an empty sample array still needs an address for the kernels' argument check
        x = a["samples"] if self.n_samples else np.zeros(1, a["samples"].dtype)
        self.samples = torch.from_numpy(x).to(self.device)
        self.starts = torch.from_numpy(a["starts"]).to(self.device)
        self.lengths = torch.from_numpy(a["lengths"]).to(self.device)
        self.labels = torch.from_numpy(a["labels"]).to(self.device)
        self.lengths_host = torch.from_numpy(a["lengths"].astype(np.int64))

    @classmethod
    def from_files(cls, file_list, targets, device="cuda", **kw):
        return cls(audio_arrays_from_files(file_list, targets, device=device, **kw), device=device, source="files")

    @classmethod
    def from_pack(cls, path, device="cuda"):
        return cls(load_audio_pack(path), device=device, source="pack")

    def __len__(self):
        return self.n_clips

    def _idx(self, idx, what):
        _require_device(idx, "idx")
        if idx.dtype != torch.int64 or idx.ndim != 1 or idx.numel() == 0 or not idx.is_contiguous():
            raise ValueError(f"AudioStore.{what}: idx must be a non-empty contiguous 1-D int64 tensor")
        return idx.numel()

    def gather_fbank(self, idx, n_frames, num_mel_bins=40):
        """(feats (B, n_frames, num_mel_bins) fp32, y (B,) int64) on the device for the device int64 index list
        `idx`: row b holds the frames of clip idx[b] as `fbank_padded` gives them, then exact zeros; an index outside
        the store gives a zero row and label -1."""
        B = self._idx(idx, "gather_fbank")
        out = torch.empty(B, n_frames, num_mel_bins, dtype=torch.float32, device=self.device)
        y = torch.empty(B, dtype=torch.int64, device=self.device)
        tok = timer.start(f"audio_gather_fbank[{B}x{n_frames}]")
        check(lib.sparch_audio_gather_fbank(ptr(self.samples), self.dtype, ptr(self.starts), ptr(self.lengths),
                                            ptr(self.labels), self.n_clips, ptr(idx), B, n_frames, num_mel_bins,
                                            ptr(out), ptr(y), _stream()), "sparch_audio_gather_fbank")
        timer.stop(tok)
        return out, y

    def gather_augment(self, idx, ld, params, noise_seed, min_snr, max_snr, sample_rate=16000):
        """(rows (B, ld) fp32, lengths (B,) int32, y (B,) int64) on the device: row b holds clip idx[b] (its first
        ld samples) augmented as `augment_padded` augments row b of a batch of those clips, same table, same seed; it
        is not written behind the clip.  params: the (B, AUGM_FIELDS) host table of `draw_augmentation`."""
        B = self._idx(idx, "gather_augment")
        table = _augm_table(params, B, sample_rate, "AudioStore.gather_augment")
        if not 0 < int(ld) <= 2 ** 31 - 1:
            raise ValueError(f"AudioStore.gather_augment: row length {ld} out of range")
        # from pinned memory without blocking the host (the caching host allocator keeps the block until the copy
        # is done)
        table_dev = table.pin_memory().to(self.device, non_blocking=True)
        out = torch.empty(B, ld, dtype=torch.float32, device=self.device)
        lens = torch.empty(B, dtype=torch.int32, device=self.device)
        y = torch.empty(B, dtype=torch.int64, device=self.device)
        tok = timer.start(f"audio_gather_augment[{B}x{ld}]")
        check(lib.sparch_audio_gather_augment(ptr(self.samples), self.dtype, ptr(self.starts), ptr(self.lengths),
                                              ptr(self.labels), self.n_clips, ptr(idx), B, ld, ptr(table_dev),
                                              float(min_snr), float(max_snr), int(noise_seed) & (2 ** 64 - 1),
                                              int(sample_rate), ptr(out), ptr(lens), ptr(y), _stream()),
              "sparch_audio_gather_augment")
        timer.stop(tok)
        return out, lens, y

    def batch(self, idx, idx_host, augment=None, num_mel_bins=40, sample_rate=16000):
        """(xs (B, T_max, num_mel_bins) on the device, xlens (B,) host int64 frame counts, ys (B,) on the device): the
        batch the file loader's collate makes of the clips `idx_host` (host int64; `idx` is the same list on the
        device).  augment: None, or (params, noise_seed, min_snr, max_snr) of `draw_augmentation`.  Raises the
        ValueError of `fbank_padded` when no clip of the batch reaches one frame."""
        n = self.lengths_host[idx_host]
        frames = torch.where(n < 400, torch.zeros_like(n), 1 + torch.div(n - 400, 160, rounding_mode="floor"))
        n_frames = int(frames.max())
        if n_frames == 0:
            raise ValueError("fbank_padded: no clip is long enough for one frame (400 samples)")
        if augment is None:
            xs, ys = self.gather_fbank(idx, n_frames, num_mel_bins)
            return xs, frames, ys
        params, noise_seed, min_snr, max_snr = augment
        B, ld = idx.numel(), int(n.max())
        rows, lens, ys = self.gather_augment(idx, ld, params, noise_seed, min_snr, max_snr, sample_rate)
        xs = torch.empty(B, n_frames, num_mel_bins, dtype=torch.float32, device=self.device)
        tok = timer.start(f"fbank_padded[{B}x{ld}]")
        check(lib.sparch_fbank_padded_fwd(B, ld, ptr(lens), n_frames, num_mel_bins, 0, ptr(rows), ptr(xs), _stream()),
              "sparch_fbank_padded_fwd")
        timer.stop(tok)
        return xs, frames, ys


# ----------------------------------------------------------------------------- f-4: non-spiking baselines
ACT_KIND = {"sigmoid": 0, "relu": 1, "tanh": 2}


class MLPLayerFn(torch.autograd.Function):
    """x (B,T,K) -> dropout(act(norm(W x))) (B,T,H): MLPLayer.forward, anns.py:210-227."""

    @staticmethod
    def forward(ctx, cfg, x, W, Wb, nw, nb):
        _require_device(x, "input")
        _require_device(W, "layer parameters")
        B, T, K = x.shape
        H = W.shape[0]
        if H % 4 != 0:
            raise ValueError("sparch_amd: MLP layers need hidden_size % 4 == 0")
        M = B * T
        inp = _LayerInput(_f32c(x).view(M, K))
        Wx_in, scale, shift, nsaved, Wx_raw = _project(inp, W, Wb, nw, nb, cfg, 1, cfg.get("ln_width"))  # anns.py:218-223
        y = torch.empty(B, T, H, dtype=torch.float32, device=x.device)
        check(lib.sparch_act_fwd(ACT_KIND[cfg["act"]], M * H, H, ptr(Wx_in), ptr(scale), ptr(shift),
                                 cfg["p_drop"], cfg["seed"], ptr(y), _stream()), "sparch_act_fwd")  # 226
        ctx.cfg, ctx.shape, ctx.nsaved = cfg, (B, T, K, H), nsaved
        ctx.save_for_backward(inp.x2, W, nw, Wx_raw, Wx_in if cfg["normalization"] != "batchnorm" else None, scale,
                              shift)
        return y

    @staticmethod
    def backward(ctx, g_y):
        cfg = ctx.cfg
        B, T, K, H = ctx.shape
        x2, W, nw, Wx_raw, Wx_in, scale, shift = ctx.saved_tensors
        M = B * T
        z = Wx_in if Wx_in is not None else Wx_raw
        dz = torch.empty(M, H, dtype=torch.float32, device=x2.device)
        check(lib.sparch_act_bwd(ACT_KIND[cfg["act"]], M * H, H, ptr(z), ptr(scale), ptr(shift), ptr(_f32c(g_y)),
                                 cfg["p_drop"], cfg["seed"], ptr(dz), _stream()), "sparch_act_bwd")
        dx, dW, dWb, dnw, dnb = _project_backward(_LayerInput(x2), W, nw, cfg, ctx.nsaved, Wx_raw, dz,
                                                  need_dx=ctx.needs_input_grad[1], need_bias=ctx.needs_input_grad[3],
                                                  ln_width=cfg.get("ln_width"))
        return None, None if dx is None else dx.view(B, T, K), dW, dWb, dnw, dnb


class ReadoutANNFn(torch.autograd.Function):
    """x (B,T,K) -> norm(W sum_t softmax(x_t)) (B,C): ReadoutLayerANN.forward, anns.py:644-665."""

    @staticmethod
    def forward(ctx, cfg, x, W, Wb, nw, nb):
        _require_device(x, "input")
        _require_device(W, "layer parameters")
        x = _f32c(x)
        B, T, K = x.shape
        C = W.shape[0]
        if K % 4 != 0 or K > 4096:
            raise ValueError("sparch_amd: ANN readout needs input features % 4 == 0 and <= 4096")
        y = torch.empty(B, K, dtype=torch.float32, device=x.device)
        check(lib.sparch_softmax_sum_fwd(B, T, K, ptr(x), ptr(y), _stream()), "sparch_softmax_sum_fwd")  # 658-663
        Wy_in, scale, shift, nsaved, Wy_raw = _project(_LayerInput(y), W, Wb, nw, nb, cfg, 1)           # 650, 653-654
        out = Wy_in if scale is None else Wy_in * scale + shift  # (B,C): tiny
        ctx.cfg, ctx.shape, ctx.nsaved = cfg, (B, T, K, C), nsaved
        ctx.save_for_backward(x, y, W, nw, Wy_raw, scale)
        return out

    @staticmethod
    def backward(ctx, g_out):
        cfg = ctx.cfg
        B, T, K, _ = ctx.shape
        x, y, W, nw, Wy_raw, _ = ctx.saved_tensors
        dz = _f32c(g_out).clone()
        gy, dW, dWb, dnw, dnb = _project_backward(_LayerInput(y), W, nw, cfg, ctx.nsaved, Wy_raw, dz,
                                                  need_dx=ctx.needs_input_grad[1], need_bias=ctx.needs_input_grad[3])
        dx = None
        if gy is not None:  # (B,K)
            dx = torch.empty(B, T, K, dtype=torch.float32, device=x.device)
            check(lib.sparch_softmax_sum_bwd(B, T, K, ptr(x), ptr(gy), ptr(dx), _stream()), "sparch_softmax_sum_bwd")
        return None, dx, dW, dWb, dnw, dnb


class RNNLayerFn(torch.autograd.Function):
    """x (B,T,K) -> dropout(y) (B,T,H*dirs) with y_t = act(norm(W x)_t + y_{t-1} V^T): RNNLayer.forward,
    anns.py:295-339.  The flipped copy of a bidirectional layer is never materialised (as for the spiking
    layers: W(x.flip(1)) = W(x).flip(1), BatchNorm over B'T rows = over BT rows)."""

    @staticmethod
    def forward(ctx, cfg, x, W, Wb, nw, nb, V):
        _require_device(x, "input")
        _require_device(W, "layer parameters")
        dirs = cfg["dirs"]
        B, T, K = x.shape
        H = W.shape[0]
        if H % 4 != 0:
            raise ValueError("sparch_amd: recurrent layers need hidden_size % 4 == 0")
        dev = x.device
        inp = _LayerInput(_f32c(x).view(B * T, K))
        Wx_in, scale, shift, nsaved, Wx_raw = _project(inp, W, Wb, nw, nb, cfg, dirs, cfg.get("ln_width"))  # anns.py:306-311
        Bp = B * dirs
        y_out = torch.empty(B, T, H * dirs, dtype=torch.float32, device=dev)
        y_state = torch.empty(Bp, T, H, dtype=torch.float32, device=dev)
        if rec_step_path(H):  # one launch per step, y_{t-1} V^T between the steps (exact six-term split GEMM)
            y_step = torch.empty(Bp, H, dtype=torch.float32, device=dev)
            rec = None
            tok = timer.start("ann_rec_fwd_steps[RNN]")
            for t in range(T):
                if t > 0:
                    rec, _ = gemm_nt(y_step, V)
                check(lib.sparch_ann_rec_step_fwd(ACT_KIND[cfg["act"]], B, dirs, T, H, t, ptr(Wx_in), ptr(scale),
                                                  ptr(shift), ptr(rec), cfg["p_drop"], cfg["seed"], ptr(y_out),
                                                  ptr(y_state), ptr(y_step), _stream()), "sparch_ann_rec_step_fwd")
            timer.stop(tok)
        else:
            vpack = _vpack(H, V, 1 | 2)  # y V^T, dense
            _persistent("ann_rec_fwd[RNN]", "sparch_ann_rec_fwd",
                        (ACT_KIND[cfg["act"]], B, dirs, T, H, ptr(Wx_in), ptr(scale), ptr(shift), ptr(vpack),
                         cfg["p_drop"], cfg["seed"], ptr(y_out), ptr(y_state)),
                        lib.sparch_rec_chan_bytes(Bp, T, H), dev, rec_steps_per_launch(T))
        ctx.cfg, ctx.shape, ctx.nsaved = cfg, (B, T, K, H), nsaved
        ctx.save_for_backward(inp.x2, W, nw, V, y_state, Wx_raw)
        return y_out

    @staticmethod
    def backward(ctx, g_y):
        cfg = ctx.cfg
        dirs = cfg["dirs"]
        B, T, K, H = ctx.shape
        x2, W, nw, V, y_state, Wx_raw = ctx.saved_tensors
        Bp = B * dirs
        dev = x2.device
        dpre = torch.empty(Bp, T, H, dtype=torch.float32, device=dev)
        y_prev = torch.empty(Bp, T, H, dtype=torch.float32, device=dev)
        g_y = _f32c(g_y)
        if rec_step_path(H):
            dpre_step = torch.empty(Bp, H, dtype=torch.float32, device=dev)
            rec = None
            tok = timer.start("ann_rec_bwd_steps[RNN]")
            for s_ in range(T):
                if s_ > 0:
                    rec = gemm_nn(dpre_step, V)           # dpre_{t+1} V
                check(lib.sparch_ann_rec_step_bwd(ACT_KIND[cfg["act"]], B, dirs, T, H, s_, ptr(g_y), ptr(y_state),
                                                  ptr(rec), cfg["p_drop"], cfg["seed"], ptr(dpre), ptr(y_prev),
                                                  ptr(dpre_step), _stream()), "sparch_ann_rec_step_bwd")
            timer.stop(tok)
        else:
            vpack = _vpack(H, V, 0 | 2)  # dpre V, dense
            _persistent("ann_rec_bwd[RNN]", "sparch_ann_rec_bwd",
                        (ACT_KIND[cfg["act"]], B, dirs, T, H, ptr(g_y), ptr(y_state), ptr(vpack), cfg["p_drop"],
                         cfg["seed"], ptr(dpre), ptr(y_prev)),
                        lib.sparch_rec_chan_bytes(Bp, T, H), dev, rec_steps_per_launch(T))
        # dV[i][j] = sum over rows and steps of dpre[.,i] * y_{t-1}[.,j]   (V(y) = y V^T, anns.py:336)
        dV = gemm_tn(dpre.view(Bp * T, H), y_prev.view(Bp * T, H))
        dx, dW, dWb, dnw, dnb = _project_backward(_LayerInput(x2), W, nw, cfg, ctx.nsaved, Wx_raw, dpre, dirs,
                                                  need_dx=ctx.needs_input_grad[1], need_bias=ctx.needs_input_grad[3],
                                                  ln_width=cfg.get("ln_width"))  # (anns.py:298-300: shared rows)
        return None, None if dx is None else dx.view(B, T, K), dW, dWb, dnw, dnb, dV


def _gemm_small(A, B, nn):
    """Per-step recurrent product of the gated baselines: A (M,K) @ B^T (nn=False, B (N,K)) or @ B (nn=True,
    B (K,N)) with M*N small and K long -> split-K form (fills the GPU instead of 16 workgroups)."""
    M, K = A.shape
    N = B.shape[1] if nn else B.shape[0]
    C = torch.empty(M, N, dtype=torch.float32, device=A.device)
    nbytes = lib.sparch_gemm6_splitk_workspace_bytes(M, N, K, _prec())
    ws = torch.empty(max(nbytes, 16) // 4, dtype=torch.float32, device=A.device)
    fn = lib.sparch_gemm6_nn_splitk if nn else lib.sparch_gemm6_nt_splitk
    check(fn(M, N, K, ptr(A), A.stride(0), ptr(B), B.stride(0), ptr(C), N, ptr(ws), nbytes, _stream(), _prec()),
          "sparch_gemm6_splitk")
    return C


def _gate_step(mode, B, dirs, T, H, t, ins, outs, p_drop, seed):
    """One launch of sparch_gate_step; ins / outs: dicts slot name -> tensor (missing = NULL)."""
    in_names = ["Wx", "sc", "sh", "Wzx", "scz", "shz", "Wrx", "scr", "shr", "rec", "g_out", "carry_mv", "carry_dir", "dry"]
    out_names = ["y_state", "z_save", "r_save", "c_save", "ry", "y_out", "carry_dir_out", "dgate", "dcp", "dz_all",
                 "dr_all", "dc_all", "yprev_all", "ry_all"]
    arr = ctypes.c_void_p * 14
    a_in = arr(*[(ins[n].data_ptr() if ins.get(n) is not None else None) for n in in_names])
    a_out = arr(*[(outs[n].data_ptr() if outs.get(n) is not None else None) for n in out_names])
    check(lib.sparch_gate_step(mode, B, dirs, T, H, t, a_in, a_out, p_drop, seed, _stream()), "sparch_gate_step")


class GatedLayerFn(torch.autograd.Function):
    """LiGRU / GRU baseline layers (anns.py:412-462, 540-595): x (B,T,K) -> dropout(y) (B,T,H*dirs).
    Launch-per-step this round: per time step the recurrent products run on the exact-split GEMMs and the
    gate arithmetic in `sparch_gate_step`; projections, normalisation and all weight gradients are whole-
    sequence GEMMs as for the other layers.  mats = ("c", "z") for LiGRU, ("c", "z", "r") for GRU; the tensor
    arguments come in groups (W, Wb, norm weight, norm bias, V) per matrix in that order."""

    @staticmethod
    def forward(ctx, cfg, x, *params):
        _require_device(x, "input")
        kind, dirs = cfg["kind"], cfg["dirs"]
        mats = ("c", "z", "r") if kind == "GRU" else ("c", "z")
        P = {m: dict(zip(("W", "Wb", "nw", "nb", "V"), params[5 * i:5 * i + 5])) for i, m in enumerate(mats)}
        B, T, K = x.shape
        H = P["c"]["W"].shape[0]
        if H % 4 != 0:
            raise ValueError("sparch_amd: recurrent layers need hidden_size % 4 == 0")
        Bp, dev = B * dirs, x.device
        inp = _LayerInput(_f32c(x).view(B * T, K))
        proj = {}
        for m in mats:
            rm, rv = cfg["running"][m]
            z_in, sc, sh, nsaved, raw = _project(inp, P[m]["W"], P[m]["Wb"], P[m]["nw"], P[m]["nb"],
                                                 dict(cfg, running_mean=rm, running_var=rv), dirs, cfg.get("ln_width"))
            proj[m] = dict(raw=raw, z_in=z_in, sc=sc, sh=sh, nsaved=nsaved)
        Vgate = torch.cat([P["z"]["V"], P["r"]["V"] if kind == "GRU" else P["c"]["V"]], dim=0).contiguous()  # (2H,H)
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        y_state, z_save, c_save = new(Bp, T, H), new(Bp, T, H), new(Bp, T, H)
        r_save = new(Bp, T, H) if kind == "GRU" else None
        ry = new(Bp, H) if kind == "GRU" else None
        y_out = new(B, T, H * dirs)
        ins = {"Wx": proj["c"]["z_in"], "sc": proj["c"]["sc"], "sh": proj["c"]["sh"],
               "Wzx": proj["z"]["z_in"], "scz": proj["z"]["sc"], "shz": proj["z"]["sh"]}
        if kind == "GRU":
            ins.update(Wrx=proj["r"]["z_in"], scr=proj["r"]["sc"], shr=proj["r"]["sh"])
        outs = {"y_state": y_state, "z_save": z_save, "r_save": r_save, "c_save": c_save, "ry": ry, "y_out": y_out}
        p_drop, seed = cfg["p_drop"], cfg["seed"]
        persistent = kind == "LiGRU" and ligru_persistent_ok(H)
        ctx.gru_persistent = kind == "GRU" and gru_persistent_ok(H)
        if ctx.gru_persistent:
            # both hand-offs of a step inside one persistent launch per row-tile group (gatedcell.hip)
            vg = torch.empty(lib.sparch_gru_vpack_bytes(H, 0, 0) // 4, dtype=torch.float32, device=dev)
            vc = torch.empty(lib.sparch_gru_vpack_bytes(H, 0, 1) // 4, dtype=torch.float32, device=dev)
            check(lib.sparch_gru_vpack(H, ptr(P["z"]["V"]), ptr(P["r"]["V"]), ptr(P["c"]["V"]), 0, ptr(vg), ptr(vc),
                                       _stream(), _prec()), "sparch_gru_vpack")
            _persistent("gru_fwd", "sparch_gru_fwd",
                        (B, dirs, T, H, ptr(proj["c"]["z_in"]), ptr(proj["c"]["sc"]), ptr(proj["c"]["sh"]),
                         ptr(proj["z"]["z_in"]), ptr(proj["z"]["sc"]), ptr(proj["z"]["sh"]), ptr(proj["r"]["z_in"]),
                         ptr(proj["r"]["sc"]), ptr(proj["r"]["sh"]), ptr(vg), ptr(vc), p_drop, seed, ptr(y_out),
                         ptr(y_state), ptr(z_save), ptr(r_save), ptr(c_save)),
                        lib.sparch_gru_chan_bytes(Bp, H), dev, rec_steps_per_launch(T))
        elif persistent:
            # the whole time loop in one persistent launch per row-tile group (gatedcell.hip)
            vp = torch.empty(lib.sparch_ligru_vpack_bytes(H, 0) // 4, dtype=torch.float32, device=dev)
            check(lib.sparch_ligru_vpack(H, ptr(P["z"]["V"]), ptr(P["c"]["V"]), 0, ptr(vp), _stream(), _prec()), "sparch_ligru_vpack")
            _persistent("ligru_fwd", "sparch_ligru_fwd",
                        (B, dirs, T, H, ptr(proj["c"]["z_in"]), ptr(proj["c"]["sc"]), ptr(proj["c"]["sh"]),
                         ptr(proj["z"]["z_in"]), ptr(proj["z"]["sc"]), ptr(proj["z"]["sh"]), ptr(vp), p_drop, seed,
                         ptr(y_out), ptr(y_state), ptr(z_save), ptr(c_save)),
                        lib.sparch_ligru_chan_bytes(Bp, H), dev, rec_steps_per_launch(T))
        else:
            tok = timer.start(f"gated_fwd[{kind}]")
            for t in range(T):
                rec = _gemm_small(y_state[:, t - 1, :], Vgate, nn=False) if t > 0 else None   # y_{t-1} [Vz;V]^T  (anns.py:457-458)
                if kind == "LiGRU":
                    _gate_step(0, B, dirs, T, H, t, dict(ins, rec=rec), outs, p_drop, seed)
                else:
                    _gate_step(1, B, dirs, T, H, t, dict(ins, rec=rec), outs, p_drop, seed)
                    recc = _gemm_small(ry, P["c"]["V"], nn=False) if t > 0 else None       # (r y_{t-1}) V^T  (anns.py:591)
                    _gate_step(2, B, dirs, T, H, t, dict(ins, rec=recc), outs, p_drop, seed)
            timer.stop(tok)
        ctx.cfg, ctx.shape, ctx.mats = cfg, (B, T, K, H), mats
        ctx.nsaved = {m: proj[m]["nsaved"] for m in mats}
        ctx.needs_b = {m: P[m]["Wb"] is not None for m in mats}
        saved = [inp.x2, y_state, z_save, c_save, r_save, Vgate]
        for m in mats:
            saved += [P[m]["W"], P[m]["nw"], P[m]["V"], proj[m]["raw"]]
        ctx.save_for_backward(*saved)
        return y_out

    @staticmethod
    def backward(ctx, g_y):
        cfg, mats = ctx.cfg, ctx.mats
        kind, dirs = cfg["kind"], cfg["dirs"]
        B, T, K, H = ctx.shape
        sv = ctx.saved_tensors
        x2, y_state, z_save, c_save, r_save, Vgate = sv[:6]
        Pm = {m: dict(zip(("W", "nw", "V", "raw"), sv[6 + 4 * i:10 + 4 * i])) for i, m in enumerate(mats)}
        Bp, dev = B * dirs, x2.device
        new = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        d_all = {"z": new(Bp, T, H), "c": new(Bp, T, H)}
        yprev_all = new(Bp, T, H)
        ry_all = new(Bp, T, H) if kind == "GRU" else None
        if kind == "GRU":
            d_all["r"] = new(Bp, T, H)
        dgate, dcp = new(Bp, 2 * H), (new(Bp, H) if kind == "GRU" else None)
        cdir = [new(Bp, H), new(Bp, H)]
        ins = {"g_out": _f32c(g_y)}
        outs = {"y_state": y_state, "z_save": z_save, "r_save": r_save, "c_save": c_save, "dgate": dgate, "dcp": dcp,
                "dz_all": d_all["z"], "dc_all": d_all["c"], "dr_all": d_all.get("r"), "yprev_all": yprev_all,
                "ry_all": ry_all}
        p_drop, seed = cfg["p_drop"], cfg["seed"]
        if kind == "GRU" and ctx.gru_persistent and gru_persistent_ok(H):
            vg = torch.empty(lib.sparch_gru_vpack_bytes(H, 1, 0) // 4, dtype=torch.float32, device=dev)
            vc = torch.empty(lib.sparch_gru_vpack_bytes(H, 1, 1) // 4, dtype=torch.float32, device=dev)
            check(lib.sparch_gru_vpack(H, ptr(Pm["z"]["V"]), ptr(Pm["r"]["V"]), ptr(Pm["c"]["V"]), 1, ptr(vg), ptr(vc),
                                       _stream(), _prec()), "sparch_gru_vpack")
            carry = new(Bp, H)
            _persistent("gru_bwd", "sparch_gru_bwd",
                        (B, dirs, T, H, ptr(_f32c(g_y)), ptr(y_state), ptr(z_save), ptr(r_save), ptr(c_save), ptr(vg),
                         ptr(vc), p_drop, seed, ptr(d_all["z"]), ptr(d_all["r"]), ptr(d_all["c"]), ptr(yprev_all),
                         ptr(ry_all), ptr(carry)),
                        lib.sparch_gru_chan_bytes(Bp, H), dev, rec_steps_per_launch(T))
        elif kind == "LiGRU" and ligru_persistent_ok(H):
            vpb = torch.empty(lib.sparch_ligru_vpack_bytes(H, 1) // 4, dtype=torch.float32, device=dev)
            check(lib.sparch_ligru_vpack(H, ptr(Pm["z"]["V"]), ptr(Pm["c"]["V"]), 1, ptr(vpb), _stream(), _prec()), "sparch_ligru_vpack")
            carry = new(Bp, H)
            _persistent("ligru_bwd", "sparch_ligru_bwd",
                        (B, dirs, T, H, ptr(_f32c(g_y)), ptr(y_state), ptr(z_save), ptr(c_save), ptr(vpb), p_drop, seed,
                         ptr(d_all["z"]), ptr(d_all["c"]), ptr(yprev_all), ptr(carry)),
                        lib.sparch_ligru_chan_bytes(Bp, H), dev, rec_steps_per_launch(T))
        else:
            carry_mv = carry_dir = None
            tok = timer.start(f"gated_bwd[{kind}]")
            for t in range(T - 1, -1, -1):
                o = dict(outs, carry_dir_out=cdir[t & 1])
                i = dict(ins, carry_mv=carry_mv, carry_dir=carry_dir)
                if kind == "LiGRU":
                    _gate_step(3, B, dirs, T, H, t, i, o, p_drop, seed)
                else:
                    _gate_step(4, B, dirs, T, H, t, i, o, p_drop, seed)
                    dry = _gemm_small(dcp, Pm["c"]["V"], nn=True)        # gradient of r * y_{t-1}
                    _gate_step(5, B, dirs, T, H, t, {"dry": dry}, o, p_drop, seed)
                if t > 0:
                    carry_mv = _gemm_small(dgate, Vgate, nn=True)        # [dz_pre | d*_pre] [Vz; V*]
                    carry_dir = cdir[t & 1]
            timer.stop(tok)
        flat = lambda a: a.view(Bp * T, H)  # noqa: E731
        dV = {"z": gemm_tn(flat(d_all["z"]), flat(yprev_all))}
        if kind == "GRU":
            dV["r"] = gemm_tn(flat(d_all["r"]), flat(yprev_all))
            dV["c"] = gemm_tn(flat(d_all["c"]), flat(ry_all))
        else:
            dV["c"] = gemm_tn(flat(d_all["c"]), flat(yprev_all))
        grads, dx_raws, inp = {}, [], _LayerInput(x2)
        for m in mats:  # per gate matrix; dx below is one product over the concatenated dx_raw
            dx_raw, dW, dWb, dnw, dnb = _project_backward(inp, Pm[m]["W"], Pm[m]["nw"], cfg, ctx.nsaved[m], Pm[m]["raw"],
                                                          d_all[m], dirs, need_dx=False, need_bias=ctx.needs_b[m],
                                                          ln_width=cfg.get("ln_width"), raw_dx=True)
            dx_raws.append(dx_raw)
            grads[m] = (dW, dWb, dnw, dnb, dV[m])
        dx = None
        if ctx.needs_input_grad[1]:
            dx = gemm_nn(torch.cat(dx_raws, dim=1), torch.cat([Pm[m]["W"] for m in mats], dim=0)).view(B, T, K)
        out = [None, dx]
        for m in mats:
            out += list(grads[m])
        return tuple(out)
