"""
GPU: the per-step readout — sparch_readout_fwd_seq / sparch_readout_bwd_seq, their `_len` forms, SNN.forward(x, per_step=...)
and SPARCH_PER_STEP_LOSS ("Per-step readout").

Shapes: B = 3; C in {1, 35, 70, 256} (one partial wave, two waves, the cap; row strides 3, 37, 71, 257).  Per C two
sequence lengths, both taken from the kernels' own chunk sizing (sparch_readout_chunk_steps, what the launchers pass as
`rows`): "long" — the smallest T above twice the largest of the forward's, the per-step backward's and the plain
backward's chunk at which every one of the three ends in a partial chunk whose length is no multiple of 8 (so every
kernel runs at least three chunks, whole groups of 8 steps and a step-by-step tail) — and "short", T = 5.  Lengths: 1, T,
the forward's chunk and one past it, the per-step backward's chunk and one past it.

 1. forward identity   out and u_save of the `_seq` forms are the plain forms' bits; "sum": seq at a row's last step is
                       out; "prob": a sequential fp32 sum of seq over t is out.
 2. streaming identity on the dyadic fixtures net(x, per_step="sum") row t is what StreamingSNN.step returns after step
                       t; on real-valued data sparch_readout_fwd_seq row t is sparch_readout_stream_fwd's accumulator
                       after t + 1 one-step calls on the same Wx.
 3. backward identities  g_seq = 0 gives the plain backward; "prob" with the same row h at every step is the plain
                       backward on fp32(g_out + h); "sum" is "prob" fed with the sequential fp32 reverse running sum.
 4. accuracy           seq, out, u_save, dWx, dalpha and the two BatchNorm sums against the fp64 restatement
                       (tests/readout_seq_numpy.py), held to the bound of tests/test_readout_kernels_fp64_gpu.py: 4 x the
                       worst of two fp32 runs of the restatement (class sums ascending / descending) against fp64, at most
                       spiking_numpy.BOUND_CAP = 1e-5 of the reference's max-abs (sn.bound_of, sn.capped).  The running sums
                       ("sum" mode: seq itself, and S_t inside the backward) are taken by the restatement's fp32 runs in the
                       kernel's order, so their T u growth is in the bound by construction and needs no bar of its own.
 5. ragged             seq is +0 at t >= len on a NaN-filled buffer; NaNs in g_seq on the padding change no bit; every
                       row is the clip run alone at B = 1, T = len, forward and backward.
 6. module level       SNN.forward(x, per_step="sum") with a per-step loss against the oracle with a per-step head, on a
                       RadLIF and an adLIF network with BatchNorm from tests/network_cases.py, to the bound rule of
                       tests/test_network_fuzz_gpu.py; run_exp.py with SPARCH_PER_STEP_LOSS in a child process.
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
from tests import network_cases as nc
from tests import ragged_oracle as rag
from tests import readout_seq_numpy as rs
from tests import spiking_numpy as sn
from tests.golden_io import snn_case
from tests.kit import DEV, F32, F64, D, N, nan_, ptr, record, same_bits, sp, within  # noqa: F401  (sp: a fixture)
from tests.kit import Fn as _Fn
from tests.spiking_cases import build_snn

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 3
CLASSES = (1, 35, 70, 256)
SHAPES = [(C, kind) for C in CLASSES for kind in ("long", "short")]
MODE = {"prob": 0, "sum": 1}
BIG = 1 << 20


def chunk(C, bwd, seq):
    """The steps per chunk of a long sequence: what the launcher passes as `rows`."""
    from sparch_amd._capi import lib
    r = lib.sparch_readout_chunk_steps(BIG, C, bwd, seq)
    assert r > 0
    return r


def steps_of(C, kind):
    if kind == "short":
        return 5
    rows = (chunk(C, 0, 1), chunk(C, 1, 1), chunk(C, 1, 0))
    T = 2 * max(rows) + 1
    while any((T % r) % 8 == 0 for r in rows):
        T += 1
    assert all(T > 2 * r and (T % r) % 8 for r in rows)
    return T


def length_sets(C, kind):
    T = steps_of(C, kind)
    if kind == "short":
        return [[1, T, 3]]
    rf, rb = chunk(C, 0, 1), chunk(C, 1, 1)
    return [[1, T, rf], [rf + 1, rb, rb + 1]]


@functools.lru_cache(maxsize=None)
def case(C, kind):
    """tests/spiking_numpy.py readout_case (real-valued Wx, the affine, BatchNorm's operands) plus g_seq ~ N(0,1)."""
    T = steps_of(C, kind)
    c = sn.readout_case(B, T, C)
    c["g_seq"] = np.random.default_rng(77 + 1000 * C + T).standard_normal((B, T, C)).astype(F32)
    c["dev"] = {k: D(c[k]) for k in ("u0", "alpha", "g_out", "g_seq", "scale", "shift")}
    c["dev"]["Wx"], c["dev"]["mean"], c["dev"]["invstd"] = (D(v) for v in c["bn"])   # the raw projection and its statistics
    return c


def _lens(lengths):
    return (None, 0) if lengths is None else (torch.tensor(lengths, dtype=torch.int32, device=DEV), int(sum(lengths)))


def run_fwd(d, mode=None, lengths=None, rows=slice(None), steps=None):
    """One forward launch on rows `rows`, steps [:steps] of the case: (out, u_save, seq).  u_save starts as zeros (the
    ragged forms do not write behind a row's end), seq as NaNs."""
    from sparch_amd._capi import check, lib
    Wx = d["Wx"][rows, :steps].contiguous()
    u0 = d["u0"][rows].contiguous()
    b, T, C = Wx.shape
    out = nan_(b, C)
    u_save = torch.zeros(b, T, C, dtype=torch.float32, device=DEV)
    seq = None if mode is None else nan_(b, T, C)
    lens, n = _lens(lengths)
    lead = (b, T, C, ptr(Wx), ptr(d["scale"]), ptr(d["shift"]), ptr(d["alpha"]), ptr(u0), ptr(out), ptr(u_save))
    tail = () if lengths is None else (ptr(lens), n)
    stream = _Fn()._stream()
    if mode is None:
        name = "sparch_readout_fwd" if lengths is None else "sparch_readout_fwd_len"
        check(getattr(lib, name)(*lead, *tail, stream), name)
    else:
        name = "sparch_readout_fwd_seq" if lengths is None else "sparch_readout_fwd_seq_len"
        check(getattr(lib, name)(*lead, ptr(seq), MODE[mode], *tail, stream), name)
    return out, u_save, seq


def run_bwd(d, u_save, g_out, g_seq=None, mode=None, lengths=None, rows=slice(None), steps=None):
    """One backward launch: (dWx, ws (3,b,C)), both NaN-filled beforehand."""
    from sparch_amd._capi import check, lib
    Wx = d["Wx"][rows, :steps].contiguous()
    u0 = d["u0"][rows].contiguous()
    b, T, C = Wx.shape
    dWx, ws = nan_(b, T, C), nan_(3, b, C)
    lens, n = _lens(lengths)
    per_step = () if mode is None else (ptr(g_seq), MODE[mode])
    lead = (b, T, C, ptr(g_out), *per_step, ptr(Wx), ptr(d["mean"]), ptr(d["invstd"]), ptr(u_save), ptr(d["alpha"]), ptr(u0),
            ptr(dWx), ptr(ws))
    tail = () if lengths is None else (ptr(lens), n)
    name = "sparch_readout_bwd" + ("" if mode is None else "_seq") + ("" if lengths is None else "_len")
    check(getattr(lib, name)(*lead, *tail, _Fn()._stream()), name)
    return dWx, ws


def done():
    _Fn().check_status()
    torch.cuda.synchronize()


def time_sum(seq):
    """The sequential fp32 sum over t of a (b,T,C) array."""
    acc = np.zeros((seq.shape[0], seq.shape[2]), F32)
    for t in range(seq.shape[1]):
        acc = acc + seq[:, t]
    return acc


def ids(v):
    return str(v)


# ------------------------------------------------------------------------------------------------ 1. forward identity
@pytest.mark.parametrize("C,kind", SHAPES, ids=ids)
def test_forward_identity(C, kind):
    d, T = case(C, kind)["dev"], steps_of(C, kind)
    for lengths in [None] + length_sets(C, kind):
        out_p, us_p, _ = run_fwd(d, None, lengths)
        last = [T - 1] * B if lengths is None else [n - 1 for n in lengths]
        for mode in rs.MODES:
            out, us, seq = run_fwd(d, mode, lengths)
            done()
            assert same_bits(out, out_p) and same_bits(us, us_p), (mode, lengths)
            assert not torch.isnan(seq).any() and float(out.sum()) > 0
            if mode == "sum":
                assert same_bits(torch.stack([seq[b, last[b]] for b in range(B)]), out), (mode, lengths)
            else:
                assert same_bits(time_sum(N(seq)), N(out)), (mode, lengths)
            if lengths is not None:     # exactly +0 behind every row's end, on the NaN-filled buffer
                for b, n in enumerate(lengths):
                    assert not seq[b, n:].view(torch.int32).any(), (mode, lengths, b)
                    assert bool((seq[b, :n] > 0).all())


# ------------------------------------------------------------------------------------------------ 2. streaming identity
@pytest.mark.parametrize("name", ["dyadic_RadLIF_none", "dyadic_RLIF_none_bias"])
def test_running_sum_is_the_stream_step_by_step(sp, name):
    cfg, x, y, params, init, z = snn_case(name)
    net = build_snn(sp, cfg, params).eval()
    x = x.to(DEV)
    with torch.no_grad(), nc.injected_states({"init": init}):
        out, rates, seq = net(x, per_step="sum")
    st = sp.StreamingSNN(net, cfg["B"])
    st.reset(states=init)
    assert seq.shape == (cfg["B"], cfg["T"], out.shape[1])
    for t in range(cfg["T"]):
        got = st.step(x[:, t:t + 1])
        assert same_bits(got, seq[:, t]), t
    done()
    assert same_bits(seq[:, -1], out)
    assert np.abs(N(out) - z["out"]).max() <= 2e-5 * cfg["T"]


def test_running_sum_is_the_stream_kernel_on_real_valued_data():
    """The readout kernel alone: the same arithmetic in the same order."""
    from sparch_amd._capi import check, lib
    C = 35
    d, T = case(C, "long")["dev"], steps_of(C, "long")
    out, us, seq = run_fwd(d, "sum")
    u, acc = d["u0"].clone(), torch.zeros(B, C, dtype=torch.float32, device=DEV)
    rows = []
    for t in range(T):
        Wc = d["Wx"][:, t:t + 1].contiguous()
        check(lib.sparch_readout_stream_fwd(B, 1, C, ptr(Wc), ptr(d["scale"]), ptr(d["shift"]), ptr(d["alpha"]), ptr(u),
                                            ptr(acc), _Fn()._stream()), "sparch_readout_stream_fwd")
        rows.append(acc.clone())
    done()
    assert same_bits(torch.stack(rows, dim=1), seq) and same_bits(acc, out) and same_bits(u, us[:, -1])


# ------------------------------------------------------------------------------------------------ 3. backward identities
@pytest.mark.parametrize("C,kind", SHAPES, ids=ids)
def test_backward_identities(C, kind):
    c = case(C, kind)
    d, T = c["dev"], steps_of(C, kind)
    zero = torch.zeros(B, T, C, dtype=torch.float32, device=DEV)
    h = D(np.random.default_rng(5 + C).standard_normal((B, C)).astype(F32))
    for lengths in [None] + length_sets(C, kind):
        _, us, _ = run_fwd(d, None, lengths)
        plain = run_bwd(d, us, d["g_out"], lengths=lengths)
        plain_h = run_bwd(d, us, d["g_out"] + h, lengths=lengths)
        S = D(rs.reverse_running_sum(c["g_seq"], F32, lengths))
        by_sum = run_bwd(d, us, d["g_out"], d["g_seq"], "sum", lengths)
        by_prob = run_bwd(d, us, d["g_out"], S, "prob", lengths)
        none = run_bwd(d, us, None, d["g_seq"], "sum", lengths)
        zeros = run_bwd(d, us, torch.zeros_like(d["g_out"]), d["g_seq"], "sum", lengths)
        done()
        for mode in rs.MODES:
            got = run_bwd(d, us, d["g_out"], zero, mode, lengths)
            assert all(same_bits(a, b) for a, b in zip(got, plain)), ("g_seq = 0", mode, lengths)
        got = run_bwd(d, us, d["g_out"], h[:, None, :].expand(B, T, C).contiguous(), "prob", lengths)
        done()
        assert all(same_bits(a, b) for a, b in zip(got, plain_h)), ("the same row at every step", lengths)
        assert all(same_bits(a, b) for a, b in zip(by_sum, by_prob)), ("sum against prob on S", lengths)
        assert all(same_bits(a, b) for a, b in zip(none, zeros)), ("g_out = NULL", lengths)
        assert not torch.isnan(by_sum[0]).any() and not torch.isnan(by_sum[1]).any()
        if C > 1:
            assert float(by_sum[0].abs().max()) > 0 and not same_bits(by_sum[0], plain[0])


# ------------------------------------------------------------------------------------------------ 4. accuracy
@pytest.mark.parametrize("mode", rs.MODES)
@pytest.mark.parametrize("C,kind", SHAPES, ids=ids)
def test_against_the_fp64_restatement(C, kind, mode, record_property):
    c = case(C, kind)
    d = c["dev"]
    Fn = _Fn()
    out, us, seq = run_fwd(d, mode)
    dWx, ws = run_bwd(d, us, d["g_out"], d["g_seq"], mode)
    dalpha, s1, s2 = Fn._finish_param_grads(ws, B, C, [d["alpha"], None, None], [Fn.ALPHA_LIM, (0.0, 0.0), (0.0, 0.0)])
    done()
    got = {"u_save": N(us), "out": N(out), "seq": N(seq), "dWx": N(dWx), "alpha": N(dalpha), "bn_dy": N(s1), "bn_dyx": N(s2)}
    x = c["bn"][0]

    def fw(dt, order):
        return rs.forward(dt, x, c["scale"], c["shift"], c["alpha"], c["u0"], mode, class_order=order)

    ref = fw(F64, None)
    if C >= 2:
        top = float(np.median(rs.forward(F64, x, c["scale"], c["shift"], c["alpha"], c["u0"], "prob")["seq"].max(-1)))
        assert top < 0.9, f"degenerate softmax rows: the median largest probability is {top:.3f}"
    names = ("u_save", "out", "seq")
    bound = sn.capped(sn.bound_of([fw(F32, "asc"), fw(F32, "desc")], ref, names), ref, names)
    worst = [within(got[k], ref[k], bound[k], k) for k in names]

    def bw(dt, order):
        return rs.backward(dt, c["g_out"], c["g_seq"], mode, got["u_save"], c["alpha"], c["u0"], bn=c["bn"], class_order=order)

    refb = bw(F64, None)
    names = sn.READOUT_BWD_TENSORS[True]
    boundb = sn.capped(sn.bound_of([bw(F32, "asc"), bw(F32, "desc")], refb, names), refb, names)
    worst += [within(got[k], refb[k], boundb[k], k) for k in names]
    if C >= 3:
        assert got["alpha"][0] == 0 and got["alpha"][1] == 0 and np.abs(got["alpha"][2:]).max() > 0
    if C == 1:
        assert not got["dWx"].any() and not got["alpha"].any()
    else:
        assert np.abs(got["dWx"]).max() > 0
    record(record_property, *worst)


# ------------------------------------------------------------------------------------------------ 5. ragged
@pytest.mark.parametrize("mode", rs.MODES)
@pytest.mark.parametrize("C,kind", SHAPES, ids=ids)
def test_ragged_rows_are_the_clips_run_alone(C, kind, mode):
    c = case(C, kind)
    d, T = c["dev"], steps_of(C, kind)
    for lengths in length_sets(C, kind):
        out, us, seq = run_fwd(d, mode, lengths)
        dWx, ws = run_bwd(d, us, d["g_out"], d["g_seq"], mode, lengths)
        poisoned = d["g_seq"].clone()
        for b, n in enumerate(lengths):
            poisoned[b, n:] = float("nan")
        dWx_p, ws_p = run_bwd(d, us, d["g_out"], poisoned, mode, lengths)
        done()
        assert same_bits(dWx_p, dWx) and same_bits(ws_p, ws), lengths
        assert not torch.isnan(dWx).any() and not torch.isnan(ws).any()
        for b, n in enumerate(lengths):
            assert not dWx[b, n:].view(torch.int32).any() and not seq[b, n:].view(torch.int32).any()
            one = slice(b, b + 1)
            out1, us1, seq1 = run_fwd(d, mode, None, one, n)
            g1 = d["g_seq"][one, :n].contiguous()
            dWx1, ws1 = run_bwd(d, us1, d["g_out"][one].contiguous(), g1, mode, None, one, n)
            done()
            assert same_bits(out1, out[one]) and same_bits(us1, us[one, :n]) and same_bits(seq1, seq[one, :n]), (lengths, b)
            assert same_bits(dWx1, dWx[one, :n]) and same_bits(ws1, ws[:, one]), (lengths, b)


# ------------------------------------------------------------------------------------------------ 6. module level
PER_STEP_W, PER_STEP_T0 = 0.5, 1
NETWORKS = (59, 69)         # tests/network_cases.py: RadLIF and adLIF with BatchNorm and a readout layer, train mode; 69 ragged


def _loss(cfg, out, rates, seq, y, gout):
    from sparch_amd import exp
    lengths = None if cfg["lengths"] is None else torch.tensor(cfg["lengths"])
    return nc.loss_of(cfg, out, rates, y, gout) + PER_STEP_W * exp.per_step_nll(seq, y, lengths, PER_STEP_T0)


def oracle_with_head(i, dtype):
    """nc.oracle_run with a per-step head: orc.readout_cell also hands back its running sum (rows padded with zeros
    behind a clip's end, as the ragged oracle runs the readout clip by clip)."""
    c = nc.case(i)
    cfg = c["cfg"]

    def cast(t):
        return t.to(dtype) if t.is_floating_point() else t

    p = {k: cast(v).clone().requires_grad_(v.is_floating_point() and "running" not in k)
         for k, v in c["params"].items() if "num_batches" not in k}
    init = [{k: cast(v) for k, v in st.items()} for st in c["init"]]
    heads = []

    def cell(Wx, alpha_raw, u0):
        alpha = torch.clamp(alpha_raw, min=orc.ALPHA_LIM[0], max=orc.ALPHA_LIM[1])
        u, out, rows = u0, torch.zeros(Wx.shape[0], Wx.shape[2], dtype=Wx.dtype), []
        for t in range(Wx.shape[1]):
            u = alpha * u + (1 - alpha) * Wx[:, t, :]
            out = out + torch.softmax(u, dim=1)
            rows.append(out)
        heads.append(torch.nn.functional.pad(torch.stack(rows, dim=1), (0, 0, 0, cfg["T"] - Wx.shape[1])))
        return out

    def step(dd):
        if cfg["surrogate"]:
            from sparch_amd.snns import SpikeFunctionSurrogate
            return SpikeFunctionSurrogate.apply(dd, *cfg["surrogate"])
        return nc._Step.apply(dd)

    kw = dict(neuron_type=cfg["kind"], num_layers=len(cfg["sizes"]), init_states=init, normalization=cfg["normalization"],
              training=cfg["training"], theta=cfg["threshold"], stats={}, drop_masks=None)
    assert c["masks"] is None
    old = orc.spike, orc.readout_cell
    orc.spike, orc.readout_cell = step, cell
    try:
        if cfg["lengths"] is None:
            out, rates = orc.snn_forward(cast(c["x"]), p, bidirectional=cfg["bidirectional"], use_readout_layer=True, **kw)
        else:
            out, rates = rag.snn_forward(cast(c["x"]), cfg["lengths"], p, **kw)
    finally:
        orc.spike, orc.readout_cell = old
    seq = torch.cat(heads, dim=0)
    loss = _loss(cfg, out, rates, seq, c["y"], cast(c["gout"]))
    loss.backward()
    return dict(out=out.detach(), seq=seq.detach(), loss=loss.detach(), **{k: v.grad for k, v in p.items() if v.requires_grad})


@pytest.mark.parametrize("i", NETWORKS, ids=[nc.label(nc.draw(i)) for i in NETWORKS])
def test_network_with_a_per_step_loss_against_the_oracle(sp, i, record_property):
    """The bound rule of tests/network_cases.py bounds(): 4 x max(|fp32 oracle - fp64 oracle| of this run, r_role x
    max-abs), r_role the pooled relative fp32 error of the parameter role (nc.role_errors; seq takes out's), each asserted
    under the whole-network bars 5e-4 / 1e-4 / 1e-5."""
    Fn = _Fn()
    c = nc.case(i)
    cfg = c["cfg"]
    assert cfg["normalization"] == "batchnorm" and cfg["training"] and cfg["dropout"] == 0.0
    net, _ = nc.build(sp, cfg)
    net = net.to(DEV).train()
    x = c["x"].to(DEV)
    kw = {} if cfg["lengths"] is None else {"lengths": torch.tensor(cfg["lengths"])}
    with nc.injected_states(c):
        out, rates, seq = net(x, per_step="sum", **kw)
        loss = _loss(cfg, out, rates, seq, c["y"].to(DEV), c["gout"].to(DEV))
        loss.backward()
    done()
    got = dict(out=N(out), seq=N(seq), loss=N(loss), **{k: N(v.grad) for k, v in net.named_parameters()})
    r64, r32 = oracle_with_head(i, torch.float64), oracle_with_head(i, torch.float32)
    assert set(got) == set(r64)
    pool, worst = nc.role_errors(), []
    for k in sorted(r64):
        if nc.residue(cfg, k):
            continue
        role = "out" if k == "seq" else nc.role_of(k)
        top = max(1.0, nc.maxabs(r64[k])) if k == "loss" else nc.maxabs(r64[k])
        bound = 4.0 * max(nc.maxabs(r32[k].double() - r64[k]), pool[role] * top)
        cap = nc.OUT_CAP if role == "out" else nc.LOSS_CAP if role == "loss" else nc.GRAD_CAP
        assert bound <= cap * top * (1 + 1e-9), (k, bound, cap * top)
        worst.append(within(got[k], r64[k].numpy(), bound, k))
    if cfg["lengths"] is not None:
        for b, n in enumerate(cfg["lengths"]):
            assert not seq[b, n:].any() and same_bits(seq[b, n - 1], out[b].detach())
    else:
        assert same_bits(seq[:, -1], out.detach())
    record(record_property, *worst)


def test_run_exp_with_a_per_step_loss(tmp_path):
    exp = tmp_path / "exp"
    env = dict(os.environ, SPARCH_PER_STEP_LOSS="0.5:10")
    env.pop("SPARCH_LENGTHS", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_exp.py"), "--model_type", "RadLIF", "--nb_layers", "3",
                        "--nb_hiddens", "64", "--dataset_name", "shd", "--batch_size", "8", "--nb_epochs", "2",
                        "--synthetic", "1", "--synthetic_batches", "3", "--save_best", "0", "--log_tofile", "1",
                        "--new_exp_folder", str(exp)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    log = (exp / "log" / "exp.log").read_text()
    for pattern in (r"Epoch \d+: train loss=(\S+)", r"Epoch \d+: train per-step loss=(\S+)",
                    r"Epoch \d+: valid mean decision step=(\S+)"):
        values = [float(v) for v in re.findall(pattern, log)]
        assert len(values) == 2 and np.isfinite(values).all(), (pattern, values)
    steps = [float(v) for v in re.findall(r"mean decision step=(\S+)", log)]
    assert all(0 <= v <= 100 for v in steps)            # (--seq_len: 100 steps by default)
    assert "nan" not in log.lower()
