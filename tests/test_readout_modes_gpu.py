"""
The selectable readout on the GPU: readout_fwd_kernel / readout_bwd_kernel with a trailing RoRed<M> (sparch_amd/csrc/cell.hip),
at the C ABI (sparch_readout_fwd_red / _bwd_red / _stream_fwd_red) and through ReadoutCellFn / ReadoutLayerFn / SNN.

Shapes (B, T, C) of tests/spiking_numpy.py READOUT_SHAPES, each plain (ReadoutCellFn) and with the forward's folded affine
plus the backward's BatchNorm sums (the library calls as ReadoutLayerFn makes them, on a given projection):
    (3, 1, 5) one step; (2, 133, 35); (3, 300, 64) forward chunks 256 + 44; (3, 270, 65) a second wave that owns one class;
    (2, 123, 256) forward chunks 61 / 61 / 1; (2, 513, 1).

  u_save     against the FREE-RUNNING fp64 restatement (tests/readout_modes_numpy.py); bound of
             tests/test_readout_kernels_fp64_gpu.py: 4 x the worse of the restatement's two fp32 runs, at most 1e-5 of max-abs.
  exact      on the kernel's own u_save: u_max out == its max over the row's steps and arg == the first argmax; u_last
             out == u_save[b, T_b - 1]; softmax_mean out == the softmax_sum out / float32(T_b); all bit for bit.  u_mean
             against fp64 with the bound above.
  backward   dWx, dalpha and the two BatchNorm sums against the fp64 restatement on the kernel's own u_save and arg, same
             bound; dWx exactly 0 behind every row's end.
  mode 0     through the new entry points == the existing ones bit for bit.
  lengths    B = 6, T = 300, lengths {1, 2, 256, 257, T - 1, T}, masked and packed: against the restatement, and against
             each other bit for bit.
  streaming  (3, 300, 64) in chunks 100 / 156 / 44 == the whole sequence bit for bit, at the C ABI and through
             StreamingSNN with a rows= reset in the middle and a get_state / set_state round trip.
  networks   [64, 64, 20], B = 6, T = 23, lengths [23, 1, 9, 17, 2, 22]: a row is its clip run alone, packed == masked,
             readout="softmax_sum" == no argument, one training step per mode, a run_exp.py epoch under SPARCH_READOUT.

Where the maxima lie (checked with the restatement, asserted below so that a change of a case cannot lose it): in every
plain case several classes have their maximum at step 0; in (3, 300, 64) 22 of 192 have it at steps >= 256 (the second
chunk); in (3, 270, 65) two have it at the last step; fp32 and fp64 agree on every argument.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import snn_oracle as orc
from tests import ragged_oracle as rag
from tests import readout_modes_numpy as rm
from tests import spiking_numpy as sn
from tests import stream_cases as sc
from tests.kit import DEV, F32, F64, D, N, record, same_bits, within
from tests.kit import Fn as _Fn
from tests.kit import sp  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 1, 5), (2, 133, 35), (3, 300, 64), (3, 270, 65), (2, 123, 256), (2, 513, 1)]
assert all(s in sn.READOUT_SHAPES for s in SHAPES)
RED = {m: i for i, m in enumerate(rm.MODES)}
NAN = float("nan")


@functools.lru_cache(maxsize=2)
def case(B, T, C):
    c = sn.readout_case(B, T, C)
    c["dev"] = {k: D(c[k]) for k in ("Wx", "u0", "alpha", "g_out", "scale", "shift")}
    c["dev"]["bn"] = tuple(D(v) for v in c["bn"])
    return c


@functools.lru_cache(maxsize=4)
def free_running(B, T, C, affine):
    """The free-running restatement of u_save (fp64, and the two fp32 runs of the bound) and the fp64 arguments."""
    c = case(B, T, C)
    x, scale, shift = (c["bn"][0], c["scale"], c["shift"]) if affine else (c["Wx"], None, None)
    ref = rm.forward(F64, x, scale, shift, c["alpha"], c["u0"], "u_max")
    r32 = rm.forward(F32, x, scale, shift, c["alpha"], c["u0"], "u_max")
    assert np.array_equal(ref["arg"], r32["arg"])               # no near-tie: fp32 and fp64 agree on every argument
    return ref, r32


def bound_of(runs32, ref, names):
    """The bound of tests/test_readout_kernels_fp64_gpu.py: 4 x the worse of the restatement's fp32 runs, CAPPED at 1e-5 of
    the reference's max-abs — where the fp32 restatement's own error comes near the cap (u_mean's BatchNorm sums: dWx has
    one sign along a row, and a sequential fp32 sum of 513 such terms is 2.7e-6 of its value off) the cap is the bound."""
    b = sn.bound_of(runs32, ref, names)
    return {k: min(b[k], sn.BOUND_CAP * float(np.abs(ref[k]).max())) for k in names}


def dev_lengths(lens):
    return torch.tensor(np.asarray(lens), dtype=torch.int32, device=DEV), int(np.sum(lens))


def red_calls(red, x, scale, shift, alpha, u0, g_out, bn, dims, L=None, plan=None, n_rows=None):
    """sparch_readout_fwd_red and sparch_readout_bwd_red as ReadoutLayerFn makes them.  dims (B, T, C): the kernels' B and T.
    The padded layout holds (B, T, C) tensors, the packed one (n_rows, C).  Everything the kernels need not write is NaN."""
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    B, T, C = dims
    tail = (plan.args() if plan is not None else (ptr(L[0]), None, L[1]) if L is not None else (None, None, 0))
    shape = (B, T, C) if plan is None else (n_rows, C)
    out = torch.full((B, C), NAN, dtype=torch.float32, device=DEV)
    u_save = torch.full(shape, NAN, dtype=torch.float32, device=DEV)
    arg = torch.full((B, C), -7, dtype=torch.int32, device=DEV)
    check(lib.sparch_readout_fwd_red(B, T, C, ptr(x), ptr(scale), ptr(shift), ptr(alpha), ptr(u0), ptr(out), ptr(u_save),
                                     red, ptr(arg), *tail, Fn._stream()), "sparch_readout_fwd_red")
    dWx = torch.full(shape, NAN, dtype=torch.float32, device=DEV)
    ws = torch.full((3 if bn else 1, B, C), NAN, dtype=torch.float32, device=DEV)
    bnp = [ptr(v) for v in bn] if bn else [None, None, None]
    check(lib.sparch_readout_bwd_red(B, T, C, ptr(g_out), *bnp, ptr(u_save), ptr(alpha), ptr(u0), ptr(dWx), ptr(ws),
                                     red, ptr(arg), *tail, Fn._stream()), "sparch_readout_bwd_red")
    Fn.check_status()
    return {"out": out, "u_save": u_save, "arg": arg, "dWx": dWx, "ws": ws}


def finish(ws, alpha, B, C):
    """dalpha and, with three planes, the two BatchNorm sums, as ReadoutLayerFn finishes them."""
    Fn = _Fn()
    if ws.shape[0] == 3:
        dalpha, s1, s2 = Fn._finish_param_grads(ws, B, C, [alpha, None, None], [Fn.ALPHA_LIM, (0.0, 0.0), (0.0, 0.0)])
        return {"alpha": N(dalpha), "bn_dy": N(s1), "bn_dyx": N(s2)}
    return {"alpha": N(Fn._finish_param_grads(ws, B, C, [alpha], [Fn.ALPHA_LIM])[0])}


def existing_calls(x, scale, shift, alpha, u0, g_out, bn, dims, L=None, plan=None, n_rows=None):
    """The softmax-sum's own entry points (plain, `_len`, `_pk`), the same way."""
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    B, T, C = dims
    suffix, tail = (("_pk", plan.args()) if plan is not None else ("_len", (ptr(L[0]), L[1])) if L is not None else ("", ()))
    shape = (B, T, C) if plan is None else (n_rows, C)
    out = torch.full((B, C), NAN, dtype=torch.float32, device=DEV)
    u_save = torch.full(shape, NAN, dtype=torch.float32, device=DEV)
    check(getattr(lib, "sparch_readout_fwd" + suffix)(B, T, C, ptr(x), ptr(scale), ptr(shift), ptr(alpha), ptr(u0), ptr(out),
                                                       ptr(u_save), *tail, Fn._stream()), "sparch_readout_fwd" + suffix)
    dWx = torch.full(shape, NAN, dtype=torch.float32, device=DEV)
    ws = torch.full((3 if bn else 1, B, C), NAN, dtype=torch.float32, device=DEV)
    bnp = [ptr(v) for v in bn] if bn else [None, None, None]
    check(getattr(lib, "sparch_readout_bwd" + suffix)(B, T, C, ptr(g_out), *bnp, ptr(u_save), ptr(alpha), ptr(u0), ptr(dWx),
                                                       ptr(ws), *tail, Fn._stream()), "sparch_readout_bwd" + suffix)
    Fn.check_status()
    return {"out": out, "u_save": u_save, "dWx": dWx, "ws": ws}


def check_exact_relations(mode, out, u_save, arg, lens, softmax_sum_out):
    """The bit-for-bit relations between out / arg and the kernel's own u_save (numpy arrays, padded layout)."""
    B, T, C = u_save.shape
    for b in range(B):
        n = int(lens[b])
        if mode == "u_max":
            assert same_bits(out[b], u_save[b, :n].max(0)), b
            assert arg.dtype == np.int32 and np.array_equal(arg[b], u_save[b, :n].argmax(0)), b
        elif mode == "u_last":
            assert same_bits(out[b], u_save[b, n - 1]), b
        elif mode == "softmax_mean":
            assert same_bits(out[b], softmax_sum_out[b] / F32(n)), b
        elif mode == "softmax_sum":
            assert same_bits(out[b], softmax_sum_out[b]), b


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("mode", rm.MODES)
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine_bn"])
@pytest.mark.parametrize("B,T,C", SHAPES, ids=lambda v: str(v))
def test_readout_modes_forward_and_backward(B, T, C, affine, mode, record_property):
    c = case(B, T, C)
    d = c["dev"]
    Fn = _Fn()
    ref_u, r32_u = free_running(B, T, C, affine)
    if not affine:                                              # where the maxima lie (module docstring)
        a = ref_u["arg"]
        assert (a == 0).sum() >= 1
        if (B, T, C) == (3, 300, 64):
            assert (a >= 256).sum() == 22 and a.size == 192
        if (B, T, C) == (3, 270, 65):
            assert (a == T - 1).sum() == 2
    x_host, scale_h, shift_h = (c["bn"][0], c["scale"], c["shift"]) if affine else (c["Wx"], None, None)
    bn_host = c["bn"] if affine else None
    if affine:
        args = (d["bn"][0], d["scale"], d["shift"], d["alpha"], d["u0"], d["g_out"], d["bn"], (B, T, C))
        r = red_calls(RED[mode], *args)
        got = {k: N(r[k]) for k in ("out", "u_save", "arg", "dWx")}
        got.update(finish(r["ws"], d["alpha"], B, C))
        plain = existing_calls(*args)
        sum_out = N(plain["out"])
        if mode == "softmax_sum":                               # mode 0 through the new entries: the existing entries' bits
            for k in ("out", "u_save", "dWx", "ws"):
                assert same_bits(r[k], plain[k]), k
            assert (got["arg"] == -7).all()                     # arg is not touched
    else:
        Wx, alpha = d["Wx"].clone().requires_grad_(True), d["alpha"].clone().requires_grad_(True)
        out = Fn.ReadoutCellFn.apply(Wx, alpha, d["u0"], mode)
        u_save, arg = out.grad_fn.saved_tensors[2], out.grad_fn.red_arg
        out.backward(d["g_out"])
        Fn.check_status()
        got = {"out": N(out), "u_save": N(u_save), "arg": N(arg), "dWx": N(Wx.grad), "alpha": N(alpha.grad)}
        sum_out = N(Fn.ReadoutCellFn.apply(d["Wx"], d["alpha"], d["u0"]))
        if mode == "softmax_sum":
            r = red_calls(0, d["Wx"], None, None, d["alpha"], d["u0"], d["g_out"], None, (B, T, C))
            assert same_bits(r["out"], out.detach()) and same_bits(r["u_save"], u_save) and same_bits(r["dWx"], Wx.grad)
    assert (got["arg"] is None) == (mode != "u_max" and not affine)

    # u_save: free-running, fp64
    names = ("u_save",)
    bound = bound_of([r32_u, r32_u], ref_u, names)
    worst = [within(got["u_save"], ref_u["u_save"], bound["u_save"], "u_save")]
    check_exact_relations(mode, got["out"], got["u_save"], got["arg"], [T] * B, sum_out)
    if mode == "u_mean":
        def fw(dt):
            return rm.forward(dt, x_host, scale_h, shift_h, c["alpha"], c["u0"], mode)
        ref = fw(F64)
        b_out = bound_of([fw(F32), fw(F32)], ref, ("out",))
        worst.append(within(got["out"], ref["out"], b_out["out"], "out"))

    # backward on the kernel's own u_save and arg
    def bw(dt, order):
        return rm.backward(dt, c["g_out"], mode, got["u_save"], c["alpha"], c["u0"], bn=bn_host, arg=got["arg"],
                           class_order=order)
    refb = bw(F64, None)
    names = sn.READOUT_BWD_TENSORS[affine]
    boundb = bound_of([bw(F32, "asc"), bw(F32, "desc")], refb, names)
    worst += [within(got[k], refb[k], boundb[k], k) for k in names]
    if C >= 3:
        assert got["alpha"][0] == 0 and got["alpha"][1] == 0
    if mode.startswith("u_") or C > 1:
        assert np.abs(got["dWx"]).max() > 0 and np.abs(got["alpha"]).max() > 0
    record(record_property, *worst)


# ------------------------------------------------------------------------------------------------ lengths, masked and packed
LEN_B, LEN_T, LEN_C = 6, 300, 35
LENS = [257, 1, 300, 2, 256, 299]           # {1, 2, 256, 257, T - 1, T}


@pytest.mark.parametrize("mode", rm.MODES)
def test_readout_modes_with_lengths_masked_and_packed(mode, record_property):
    from sparch_amd.snns import prepare_packing
    Fn = _Fn()
    B, T, C = LEN_B, LEN_T, LEN_C
    c = case(B, T, C)
    d = c["dev"]
    lens = np.asarray(LENS, np.int64)
    assert sorted(LENS) == [1, 2, 256, 257, T - 1, T]
    L = dev_lengths(lens)
    m = rm.valid(lens, B, T)[:, :, None]
    args = (d["bn"][0], d["scale"], d["shift"], d["alpha"], d["u0"], d["g_out"], d["bn"])
    r = red_calls(RED[mode], *args, (B, T, C), L=L)
    got = {k: N(r[k]) for k in ("out", "u_save", "arg", "dWx", "ws")}
    got.update(finish(r["ws"], d["alpha"], B, C))
    # behind a row's length: u_save not written, dWx exactly 0; nothing else is NaN
    assert np.isnan(got["u_save"][np.broadcast_to(~m, got["u_save"].shape)]).all()
    assert not np.isnan(got["u_save"][np.broadcast_to(m, got["u_save"].shape)]).any()
    assert not (got["dWx"] * ~m).any() and not np.isnan(got["dWx"]).any()
    tail = got["dWx"][np.broadcast_to(~m, got["dWx"].shape)]
    assert same_bits(tail, np.zeros_like(tail))                             # +0, not -0
    assert not np.isnan(got["out"]).any() and not np.isnan(got["ws"]).any()
    plain = existing_calls(*args, (B, T, C), L=L)
    check_exact_relations(mode, got["out"], got["u_save"], got["arg"], lens, N(plain["out"]))
    if mode == "softmax_sum":
        for k in ("out", "u_save", "dWx", "ws"):
            assert same_bits(r[k], plain[k]), k

    # against the restatement
    def fw(dt, order):
        return rm.forward(dt, c["bn"][0], c["scale"], c["shift"], c["alpha"], c["u0"], mode, lens, order)

    def bw(dt, order):
        return rm.backward(dt, c["g_out"], mode, got["u_save"], c["alpha"], c["u0"], bn=c["bn"], lengths=lens,
                           arg=got["arg"], class_order=order)
    ref, r32 = fw(F64, None), [fw(F32, "asc"), fw(F32, "desc")]
    if mode == "u_max":
        assert np.array_equal(ref["arg"], r32[0]["arg"]) and np.array_equal(got["arg"], ref["arg"])
    bound = bound_of(r32, ref, ("out",))
    worst = [within(got["out"], ref["out"], bound["out"], "out")]
    ub = sn.bound_of([{"u_save": np.where(m, q["u_save"], 0)} for q in r32], {"u_save": np.where(m, ref["u_save"], 0)},
                     ("u_save",))["u_save"]
    worst.append(within(np.where(m, got["u_save"], 0), np.where(m, ref["u_save"], 0), ub, "u_save"))
    refb = bw(F64, None)
    names = sn.READOUT_BWD_TENSORS[True]
    boundb = bound_of([bw(F32, "asc"), bw(F32, "desc")], refb, names)
    worst += [within(got[k], refb[k], boundb[k], k) for k in names]

    # packed, sorted as prepare_packing does: the same bits
    plan = prepare_packing(torch.tensor(LENS), B, T, torch.device(DEV))
    order = plan.order.long()
    assert N(plan.lengths).tolist() == sorted(LENS, reverse=True) and plan.t_max == T and plan.n == int(lens.sum())
    xp = Fn.pack_rows(d["bn"][0], plan)
    pargs = (xp, d["scale"], d["shift"], d["alpha"], d["u0"].index_select(0, order), d["g_out"].index_select(0, order),
             (xp, d["bn"][1], d["bn"][2]))
    p = red_calls(RED[mode], *pargs, (B, T, C), plan=plan, n_rows=plan.n)
    assert same_bits(p["out"], r["out"].index_select(0, order))
    assert same_bits(p["ws"], r["ws"].index_select(1, order))
    if mode == "u_max":
        assert same_bits(p["arg"], r["arg"].index_select(0, order))       # the step inside the row's own sequence
    assert same_bits(Fn.unpack_rows(p["dWx"], plan), r["dWx"])
    assert same_bits(p["u_save"], Fn.pack_rows(r["u_save"], plan))
    if mode == "softmax_sum":
        pp = existing_calls(*pargs, (B, T, C), plan=plan, n_rows=plan.n)
        for k in ("out", "u_save", "dWx", "ws"):
            assert same_bits(p[k], pp[k]), k
    Fn.check_status()
    record(record_property, *worst)


# ------------------------------------------------------------------------------------------------ streaming
@pytest.mark.parametrize("mode", rm.MODES)
def test_stream_kernel_in_chunks_equals_the_whole_sequence(mode):
    """(3, 300, 64) with the affine: sparch_readout_stream_fwd_red in chunks of 100 / 156 / 44, the accumulator carried in
    `out` (from -inf for u_max), the mean modes divided by the step count behind it."""
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    B, T, C = 3, 300, 64
    d = case(B, T, C)["dev"]
    Wx = d["bn"][0]
    whole = red_calls(RED[mode], Wx, d["scale"], d["shift"], d["alpha"], d["u0"], d["g_out"], None, (B, T, C))
    u = d["u0"].clone()
    out = torch.full((B, C), float("-inf") if mode == "u_max" else 0.0, dtype=torch.float32, device=DEV)
    t0 = 0
    for n in (100, 156, 44):
        Wc = Wx[:, t0:t0 + n].contiguous()
        check(lib.sparch_readout_stream_fwd_red(B, n, C, ptr(Wc), ptr(d["scale"]), ptr(d["shift"]), ptr(d["alpha"]), ptr(u),
                                                ptr(out), RED[mode], Fn._stream()), "sparch_readout_stream_fwd_red")
        t0 += n
    Fn.check_status()
    if mode in rm.MEAN_MODES:
        out = out / torch.full((B, 1), float(T), dtype=torch.float32, device=DEV)
    assert t0 == T and same_bits(out, whole["out"]) and same_bits(u, whole["u_save"][:, -1])


def flat_states(init, rows=slice(None)):
    return [st[k][rows] for st in init for k in ("u0", "w0", "s0") if k in st]


@pytest.mark.parametrize("mode", rm.MODES)
def test_streaming_snn_follows_the_mode(sp, mode):
    """A dyadic LIF network with 64 classes, (3, 300): chunks 100 / 156 / 44 == net(x) bit for bit; row 1 restarted behind
    the first chunk (reset(rows=[1])) ends as its last 200 steps run alone; get_state -> set_state continues bit for bit."""
    B, T, K, sizes = 3, 300, 40, [64, 64]
    net, init = sc.dyadic_net(sp, "LIF", B, K, sizes, "batchnorm", 5)
    net.readout = net.snn[-1].readout = mode
    x = (torch.rand(B, T, K, generator=torch.Generator().manual_seed(2)) < 0.3).float().to(DEV)
    whole, _, _ = sc.whole_forward(net, x, flat_states(init))
    st = sp.StreamingSNN(net, B)
    st.reset(states=init)
    outs, t0 = [], 0
    for n in (100, 156, 44):
        outs.append(st.step(x[:, t0:t0 + n]))
        t0 += n
    assert same_bits(outs[-1], whole)
    # a restart of row 1 in the middle, and a second stream continued from a saved state
    st.reset(states=init)
    st.step(x[:, :100])
    st.reset(states=[{k: v[1:2] for k, v in s.items()} for s in init], rows=[1])
    st.step(x[:, 100:256])
    saved = st.get_state()
    assert ("steps" in saved[-1]) == (mode in rm.MEAN_MODES)
    last = st.step(x[:, 256:])
    alone, _, _ = sc.whole_forward(net, x[1:2, 100:].contiguous(), flat_states(init, slice(1, 2)))
    assert same_bits(last[1:2], alone) and same_bits(last[[0, 2]], whole[[0, 2]])
    st2 = sp.StreamingSNN(net, B)
    st2.reset(states=init)
    st2.set_state(saved)
    assert same_bits(st2.step(x[:, 256:]), last)
    _Fn().check_status()


# ------------------------------------------------------------------------------------------------ whole networks
SIZES, NB, NT, NC = [64, 64, 20], 6, 23, 40
NET_LENGTHS = [23, 1, 9, 17, 2, 22]


def make_net(sp, kind, seed=3, **kw):
    """tests/test_ragged_gpu.py's network: dyadic weights, a positive drive, a live BatchNorm affine."""
    torch.manual_seed(seed)
    net = sp.SNN((NB, None, NC), SIZES, neuron_type=kind, dropout=0.0, normalization="batchnorm", **kw)
    with torch.no_grad():
        for lay in net.snn:
            lay.W.weight.copy_(torch.round((lay.W.weight * 4 + 0.25) * 64) / 64)
            if hasattr(lay, "V"):
                lay.V.weight.copy_(torch.round(lay.V.weight * 64) / 64)
            lay.norm.weight.copy_(torch.round((torch.rand_like(lay.norm.weight) + 1.0) * 16) / 16)
            lay.norm.bias.copy_(torch.round((torch.rand_like(lay.norm.bias) * 0.5 + 0.25) * 16) / 16)
    return net


def net_inputs(kind, seed=11):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(NB, NT, NC, generator=g) < 0.3).float()
    x = x * rag.valid_mask(NET_LENGTHS, NT)[:, :, None]
    y = torch.randint(0, SIZES[-1], (NB,), generator=g)
    torch.manual_seed(seed + 1)
    init = orc.draw_init_states(NB, SIZES, kind)
    init = [{k: torch.floor(v * 16) / 16 for k, v in st.items()} for st in init]
    return x, y, init


class injected_states:
    """The initial states of `init` (row range `rows`) handed to the network's draws, in the reference's order."""

    def __init__(self, init, rows=slice(None)):
        self.order = flat_states(init, rows)

    def __enter__(self):
        from sparch_amd import snns as snn_mod
        it = iter(self.order)
        self.mod, self.old = snn_mod, snn_mod._rand_to
        snn_mod._rand_to = lambda rows, cols, device: next(it).to(device)

    def __exit__(self, *exc):
        self.mod._rand_to = self.old


@pytest.mark.parametrize("mode", rm.MODES)
@pytest.mark.parametrize("kind", ["LIF", "RadLIF"])
def test_a_row_is_its_clip_run_alone_and_packed_is_masked(sp, kind, mode):
    net = make_net(sp, kind, readout=mode).to(DEV).eval()
    x, _, init = net_inputs(kind)
    with torch.no_grad():
        with injected_states(init):
            out, _ = net(x.to(DEV), lengths=torch.tensor(NET_LENGTHS))
        for b, n in enumerate(NET_LENGTHS):
            with injected_states(init, slice(b, b + 1)):
                alone, _ = net(x[b:b + 1, :n].contiguous().to(DEV))
            assert same_bits(out[b:b + 1], alone), (b, n)
        with injected_states(init):
            packed, _ = net(x.to(DEV), lengths=torch.tensor(NET_LENGTHS), pack=True)
    assert same_bits(packed, out)
    _Fn().check_status()


def train_step(net, x, y, init, **kw):
    net.zero_grad(set_to_none=True)
    with injected_states(init):
        out, rates = net(x.to(DEV), **kw)
        loss = orc.train_step_loss(out, rates, y.to(DEV), use_regularizers=True)
        loss.backward()
    _Fn().check_status()
    return out.detach().clone(), {k: v.grad.detach().clone() for k, v in net.named_parameters()}


@pytest.mark.parametrize("kw", [{}, {"lengths": NET_LENGTHS}, {"lengths": NET_LENGTHS, "pack": True}], ids=["full", "masked", "packed"])
def test_the_named_default_is_the_default_bit_for_bit(sp, kw):
    x, y, init = net_inputs("RadLIF")
    kw = {k: (torch.tensor(v) if k == "lengths" else v) for k, v in kw.items()}
    a_out, a_grad = train_step(make_net(sp, "RadLIF").to(DEV).train(), x, y, init, **kw)
    b_out, b_grad = train_step(make_net(sp, "RadLIF", readout="softmax_sum").to(DEV).train(), x, y, init, **kw)
    assert same_bits(a_out, b_out) and set(a_grad) == set(b_grad)
    for k in a_grad:
        assert same_bits(a_grad[k], b_grad[k]), k


@pytest.mark.parametrize("kw", [{}, {"lengths": NET_LENGTHS}, {"lengths": NET_LENGTHS, "pack": True}], ids=["full", "masked", "packed"])
@pytest.mark.parametrize("mode", rm.MODES)
def test_one_training_step_per_mode(sp, mode, kw):
    x, y, init = net_inputs("RadLIF")
    kw = {k: (torch.tensor(v) if k == "lengths" else v) for k, v in kw.items()}
    out, grads = train_step(make_net(sp, "RadLIF", readout=mode).to(DEV).train(), x, y, init, **kw)
    assert torch.isfinite(out).all()
    for k, g in grads.items():
        assert torch.isfinite(g).all() and bool(g.any()), k


def test_run_exp_under_sparch_readout(tmp_path):
    exp = tmp_path / "exp"
    env = dict(os.environ, SPARCH_READOUT="u_max")
    for k in ("SPARCH_LENGTHS", "SPARCH_PER_STEP_LOSS"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_exp.py"), "--model_type", "RadLIF", "--nb_layers", "3",
                        "--nb_hiddens", "64", "--dataset_name", "shd", "--batch_size", "8", "--nb_epochs", "1",
                        "--synthetic", "1", "--synthetic_batches", "3", "--save_best", "0", "--log_tofile", "1",
                        "--new_exp_folder", str(exp)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    log = (exp / "log" / "exp.log").read_text()
    assert "readout=u_max" in log
    values = [float(v) for v in re.findall(r"Epoch \d+: train loss=(\S+)", log)]
    assert len(values) == 1 and np.isfinite(values).all(), values
    assert "nan" not in log.lower()
