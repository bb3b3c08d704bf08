"""
The readout kernels (readout_fwd_kernel / readout_bwd_kernel of sparch_amd/csrc/cell.hip) against the fp64 restatement
of tests/spiking_numpy.py (readout_forward / readout_backward) at the edges of their staging sweeps and time chunks.

The forward stages a chunk in sweeps of 256 x 36 = 9216 elements, the backward in sweeps of 256 x 18 = 4608; both cut
the sequence into chunks of min(256, LDS floats / row stride) steps.  Shapes (B, T, C), each plain (ReadoutCellFn) and
with the forward's folded affine plus the backward's BatchNorm sums (the library calls exactly as ReadoutLayerFn makes
them, on a given projection):

    (3, 1, 5)      one step
    (2, 133, 35)   4655 elements: a second backward sweep of 47
    (2, 250, 37)   9250 elements: a second forward sweep of 34, three backward sweeps
    (3, 300, 64)   chunks 256 + 44; a last wave with classes exactly full
    (3, 270, 65)   a second wave that owns one class
    (2, 123, 256)  forward chunks 61 / 61 / 1, backward 50 / 50 / 23
    (2, 513, 1)    row stride 3, chunks 256 / 256 / 1
    (2, 40, 2)     even C

  forward   u_save and out against the FREE-RUNNING fp64 restatement: the recurrence is linear, there is no
            discontinuity.
  backward  dWx, the alpha gradient (class 0 below, class 1 above the clamp range where C >= 3: exactly 0) and the two
            BatchNorm sums on the kernel's own u_save.

Bound: 4 x the worst of two fp32 runs of the restatement (softmax denominator, dot and the sums over the batch rows
ascending, descending) against fp64, and at most 1e-5 of the reference tensor's max-abs.  tests/test_spiking_numpy_host.py
shows that it resolves an ignored u0, a dot over C - 1 classes and a ragged sweep's last element read as 0.
Condition: the softmax rows are not degenerate — the largest probability of a row has median < 0.9 (asserted where
C >= 2: one class has probability 1 by definition, and there dWx and dalpha are identically 0).
"""
import functools

import numpy as np
import pytest
import torch

from tests import spiking_numpy as sn
from tests.kit import DEV, F32, F64, D, N, record, within
from tests.kit import Fn as _Fn

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=2)
def case(B, T, C):
    c = sn.readout_case(B, T, C)
    c["dev"] = {k: D(c[k]) for k in ("Wx", "u0", "alpha", "g_out", "scale", "shift")}
    c["dev"]["bn"] = tuple(D(v) for v in c["bn"])
    return c


def kernel(c, affine):
    """Forward and backward on the device.  Returns u_save, out and the backward's tensors as numpy arrays."""
    from sparch_amd._capi import check, lib, ptr
    Fn, d = _Fn(), c["dev"]
    B, T, C = c["B"], c["T"], c["C"]
    if not affine:
        Wx, alpha = d["Wx"].clone().requires_grad_(True), d["alpha"].clone().requires_grad_(True)
        out = Fn.ReadoutCellFn.apply(Wx, alpha, d["u0"])
        u_save = out.grad_fn.saved_tensors[2]
        out.backward(d["g_out"])
        got = {"u_save": u_save, "out": out, "dWx": Wx.grad, "alpha": alpha.grad}
    else:                                                   # ReadoutLayerFn's calls, on a given raw projection
        Wx_raw, mean, invstd = d["bn"]
        out = torch.empty(B, C, dtype=torch.float32, device=DEV)
        u_save = torch.empty(B, T, C, dtype=torch.float32, device=DEV)
        check(lib.sparch_readout_fwd(B, T, C, ptr(Wx_raw), ptr(d["scale"]), ptr(d["shift"]), ptr(d["alpha"]), ptr(d["u0"]),
                                     ptr(out), ptr(u_save), Fn._stream()), "sparch_readout_fwd")
        dWx = torch.empty(B, T, C, dtype=torch.float32, device=DEV)
        ws = torch.empty(3, B, C, dtype=torch.float32, device=DEV)
        check(lib.sparch_readout_bwd(B, T, C, ptr(d["g_out"]), ptr(Wx_raw), ptr(mean), ptr(invstd), ptr(u_save),
                                     ptr(d["alpha"]), ptr(d["u0"]), ptr(dWx), ptr(ws), Fn._stream()), "sparch_readout_bwd")
        dalpha, s1, s2 = Fn._finish_param_grads(ws, B, C, [d["alpha"], None, None],
                                                [Fn.ALPHA_LIM, (0.0, 0.0), (0.0, 0.0)])
        got = {"u_save": u_save, "out": out, "dWx": dWx, "alpha": dalpha, "bn_dy": s1, "bn_dyx": s2}
    Fn.check_status()
    torch.cuda.synchronize()
    return {k: N(v) for k, v in got.items()}


@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine_bn"])
@pytest.mark.parametrize("B,T,C", sn.READOUT_SHAPES, ids=lambda v: str(v))
def test_readout_forward_and_backward(B, T, C, affine, record_property):
    c = case(B, T, C)
    got = kernel(c, affine)
    x, scale, shift = (c["bn"][0], c["scale"], c["shift"]) if affine else (c["Wx"], None, None)

    def fw(dt, order):
        u, out = sn.readout_forward(dt, x, scale, shift, c["alpha"], c["u0"], order)
        return {"u_save": u, "out": out}

    ref = fw(F64, None)
    e = np.exp(ref["u_save"] - ref["u_save"].max(-1, keepdims=True))
    if C >= 2:
        top = float(np.median((e / e.sum(-1, keepdims=True)).max(-1)))
        assert top < 0.9, f"degenerate softmax rows: the median largest probability is {top:.3f}"
    assert abs(ref["out"].sum() - B * T) <= 1e-9 * B * T
    names = ("u_save", "out")
    bound = sn.capped(sn.bound_of([fw(F32, "asc"), fw(F32, "desc")], ref, names), ref, names)
    worst = [within(got[k], ref[k], bound[k], k) for k in names]

    us = got["u_save"]
    bn = c["bn"] if affine else None

    def bw(dt, order):
        return sn.readout_backward(dt, c["g_out"], us, c["alpha"], c["u0"], bn=bn, class_order=order)

    refb = bw(F64, None)
    names = sn.READOUT_BWD_TENSORS[affine]
    boundb = sn.capped(sn.bound_of([bw(F32, "asc"), bw(F32, "desc")], refb, names), refb, names)
    worst += [within(got[k], refb[k], boundb[k], k) for k in names]
    if C >= 3:
        assert got["alpha"][0] == 0 and got["alpha"][1] == 0 and np.abs(got["alpha"][2:]).max() > 0
    if C == 1:
        assert not got["dWx"].any() and not got["alpha"].any()
    else:
        assert np.abs(got["dWx"]).max() > 0
    record(record_property, *worst)


def test_readout_stream_in_chunks_continues_one_sum():
    """(3, 300, 64) with the affine: sparch_readout_stream_fwd, as StreamingSNN calls it, in chunks of 100 / 156 / 44
    equals the whole-sequence out and final u bit for bit — the accumulator continues one sequential sum."""
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    B, T, C = 3, 300, 64
    c = case(B, T, C)
    d = c["dev"]
    Wx = d["bn"][0]
    out_w = torch.empty(B, C, dtype=torch.float32, device=DEV)
    u_save = torch.empty(B, T, C, dtype=torch.float32, device=DEV)
    check(lib.sparch_readout_fwd(B, T, C, ptr(Wx), ptr(d["scale"]), ptr(d["shift"]), ptr(d["alpha"]), ptr(d["u0"]),
                                 ptr(out_w), ptr(u_save), Fn._stream()), "sparch_readout_fwd")
    u, out, t0 = d["u0"].clone(), torch.zeros(B, C, dtype=torch.float32, device=DEV), 0
    for n in (100, 156, 44):
        Wc = Wx[:, t0:t0 + n].contiguous()
        check(lib.sparch_readout_stream_fwd(B, n, C, ptr(Wc), ptr(d["scale"]), ptr(d["shift"]), ptr(d["alpha"]), ptr(u),
                                            ptr(out), Fn._stream()), "sparch_readout_stream_fwd")
        t0 += n
    Fn.check_status()
    torch.cuda.synchronize()
    assert t0 == T and torch.equal(out, out_w) and torch.equal(u, u_save[:, -1])
    assert abs(float(out_w.double().sum()) - B * T) <= 1e-4 * B * T
