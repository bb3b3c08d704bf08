"""
GPU: stateful training — SNN.forward(x, state=st, return_state=True), sparch_cell_bwd_st, sparch_rec_cell_bwd_st,
sparch_readout_bwd_st ("Stateful training"), for all four kinds.

The invariant: feeding x in chunks, each chunk started from the state the previous one returned, is the whole-sequence
forward started from the first chunk's state — spikes and final state bit for bit, the summed output and (with the
states kept in the graph) every gradient within fp32 reassociation.  References: the whole-sequence run on the device,
tests/stateful_oracle.py on the CPU.  Bars: GRAD_CAP / OUT_CAP of the reference tensor's max-abs (tests/network_cases.py:
the project's whole-network bars; the chunked run reassociates the same sums the oracle comparison already allows for).

Shapes are the smallest that cross the kernels' edges: B 3 and 33, T = 24 in chunks [24], [1] * 24, [7, 7, 7, 3] and
[5, 1, 13, 2, 3], H 10 (not a multiple of 4), 36 and 128, classes 5 and 35; one case at H = 1024, B = 33; and, at the cell
level, B = 512 x H = 1024, the smallest size at which the launch rule takes four neurons per thread.
"""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import snn_oracle as orc
from tests import dropout_numpy as dn
from tests import stateful_oracle as so
from tests.kit import DEV, record, within
from tests.kit import Fn as _Fn
from tests.kit import sp  # noqa: F401  (a fixture)
from tests.network_cases import GRAD_CAP, OUT_CAP
from tests.stream_cases import dyadic_net
from tests.surrogate_numpy import TEST_SCALE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, C = 24, 20
CHUNKINGS = {"whole": [24], "ones": [1] * 24, "sevens": [7, 7, 7, 3], "uneven": [5, 1, 13, 2, 3]}
CASES = [("LIF", 3, (10, 36, 5)), ("adLIF", 3, (10, 36, 5)), ("LIF", 33, (36, 128, 35)), ("adLIF", 33, (128, 10, 35)),
         ("RLIF", 3, (10, 36, 5)), ("RadLIF", 3, (10, 36, 5)), ("RLIF", 33, (128, 10, 35)), ("RadLIF", 33, (36, 128, 35))]
SOME = [CASES[1], CASES[2], CASES[5], CASES[6]]      # (one case per kind, both batch sizes, every width)
case_id = lambda c: f"{c[0]}-B{c[1]}-" + "x".join(map(str, c[2]))  # noqa: E731
NORMS = [("none", True), ("layernorm", True), ("batchnorm", False)]
norm_id = lambda n: f"{n[0]}-{'train' if n[1] else 'eval'}"  # noqa: E731


def make(sp, kind, B, sizes, norm, training, seed=11, real=False, surrogate=None, dropout=0.0):  # noqa: F811
    net, init = dyadic_net(sp, kind, B, C, list(sizes), norm, seed)
    g = torch.Generator().manual_seed(seed + 5)
    with torch.no_grad():
        for lay in net.snn[:-1]:
            if norm == "none":  # nothing rescales the drive: a positive offset on the 2^-6 grid carries its mean to ~2
                fan = lay.W.weight.shape[1]
                lay.W.weight.add_(max(1, round(64 * 2.0 / (0.3 * fan))) / 64)
        for lay in net.snn:
            if real:  # real-valued weights: off every grid
                lay.W.weight.add_((torch.rand(lay.W.weight.shape, generator=g) * 1e-2).to(DEV))
            if norm == "layernorm":  # a drive that reaches the threshold
                lay.norm.weight.fill_(2.0)
                lay.norm.bias.fill_(1.0)
    hidden = list(net.snn)[:-1]
    for k, lay in enumerate(hidden):
        if surrogate is not None:
            lay.surrogate, lay.surrogate_scale = surrogate
        if dropout:
            lay.dropout = dropout
            lay._dropout_seed = lambda device, seed=1234 + 7919 * k: seed
    net.train(training)
    x = (torch.rand(B, T, C, generator=g) < 0.3).float()
    gout = torch.round(torch.randn(B, sizes[-1], generator=g) * 8) / 8           # a dyadic cotangent
    state = [{k[0]: v for k, v in st.items()} for st in init]
    return net, x, gout, state


def on_device(state, grad=False):
    return [{k: v.to(DEV).clone().requires_grad_(grad) for k, v in st.items()} for st in state]


class tapped:
    """Records every hidden layer's output spikes, call by call, around forward_with_rate (the layers still hand each
    other placeholders and bf16 planes)."""

    def __init__(self, net):
        self.net, self.rec = net, {}

    def __enter__(self):
        from sparch_amd import snns as snn_mod
        self.layers = list(self.net.snn)[:-1] if self.net.use_readout_layer else list(self.net.snn)
        for k, lay in enumerate(self.layers):
            def wrapped(inp, orig=lay.forward_with_rate, k=k, **kw):
                res = orig(inp, **kw)
                self.rec.setdefault(k, []).append(snn_mod.materialize_spikes(res[0]).detach().float())
                return res
            lay.forward_with_rate = wrapped
        return self

    def __exit__(self, *exc):
        for lay in self.layers:
            del lay.forward_with_rate

    def spikes(self):
        return [torch.cat(self.rec[k], dim=1) for k in sorted(self.rec)]


def chained(net, x, chunks, state, detach=False):
    """(sum of out, the chunks' rates, the last state, per-layer spikes) of x fed in `chunks` from `state`."""
    from sparch_amd.snns import detach_state
    total, rates, t0 = None, [], 0
    with tapped(net) as tap:
        for n in chunks:
            out, r, state = net(x[:, t0:t0 + n], state=state, return_state=True)
            if detach:
                state = detach_state(state)
            total = out if total is None else total + out
            rates.append(r)
            t0 += n
    _Fn().check_status()
    return total, rates, state, tap.spikes()


def state_form(final, seed=3):
    """A fixed random linear form of a state (dyadic coefficients), on the state's device."""
    g = torch.Generator().manual_seed(seed)
    coef = [{k: (torch.round(torch.randn(v.shape, generator=g) * 4) / 4) for k, v in sorted(st.items())} for st in final]
    return sum((st[k] * c[k].to(st[k].device)).sum() for st, c in zip(final, coef) for k in c)


def loss_of(out, rates, chunks, final, gout, form="all", rates_term=True):
    """form: "all" — a cotangent on the summed output, the firing rates and a linear form of the final state;
    "state" — the final state only (out unused); "out" — the output and the rates only."""
    if form == "state":
        return state_form(final)
    loss = (out * gout.to(out.device)).sum()
    if rates_term:  # the whole sequence's firing rates: the chunks' means weighted by their steps
        loss = loss + sum(r.sum() * (n / T) for r, n in zip(rates, chunks))
    return loss + state_form(final) if form == "all" else loss


def device_grads(net, x, chunks, state0, gout, form="all", rates_term=True):
    net.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(True)
    st = on_device(state0, grad=True)
    out, rates, final, spikes = chained(net, xd, chunks, st)
    loss_of(out, rates, chunks, final, gout, form, rates_term).backward()
    _Fn().check_status()
    grads = {k: v.grad.detach().cpu() for k, v in net.named_parameters() if v.grad is not None}
    grads["x"] = xd.grad.cpu()
    for i, d in enumerate(st):
        for k, v in d.items():
            grads[f"state{i}.{k}"] = None if v.grad is None else v.grad.cpu()
    return out.detach().cpu(), [s.cpu() for s in spikes], grads, [{k: v.detach().cpu() for k, v in d.items()} for d in final]


def oracle_grads(net, kind, x, chunks, state0, gout, norm, training, form="all", masks=None, surrogate=None):
    p = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point() and "running" not in k)
         for k, v in net.state_dict().items() if "num_batches" not in k}
    xo = x.clone().requires_grad_(True)
    st = [{k: v.clone().requires_grad_(True) for k, v in d.items()} for d in state0]
    old = orc.spike
    if surrogate is not None:
        from sparch_amd.snns import SpikeFunctionSurrogate
        orc.spike = lambda d: SpikeFunctionSurrogate.apply(d, *surrogate)
    try:
        out, rates, final, spikes = so.chained(xo, chunks, p, st, neuron_type=kind, num_layers=len(net.snn),
                                               normalization=norm, training=training, drop_masks=masks)
    finally:
        orc.spike = old
    loss_of(out, rates, chunks, final, gout, form).backward()
    grads = {k: v.grad for k, v in p.items() if v.requires_grad and v.grad is not None}
    grads["x"] = xo.grad
    for i, d in enumerate(st):
        for k, v in d.items():
            grads[f"state{i}.{k}"] = v.grad
    return out.detach(), [s.detach() for s in spikes], grads, [{k: v.detach() for k, v in d.items()} for d in final]


def compare_grads(got, ref, what):
    assert set(got) == set(ref), (sorted(set(got) ^ set(ref)), what)
    worst = 0.0
    for k, r in ref.items():
        if r is None:
            assert got[k] is None, k
            continue
        m = float(r.abs().max())
        assert m > 0, f"{what}: the reference gradient of {k} is all zero"
        assert tuple(got[k].shape) == tuple(r.shape), k
        if k.endswith("V.weight"):      # the recurrent weights' diagonal takes no part: its gradient is exactly 0
            assert not got[k].diagonal().any(), k
        worst = max(worst, within(got[k].numpy(), r.numpy(), GRAD_CAP * m, f"{what} {k}"))
    return worst


# ---------------------------------------------------------------------------------------------- 1. forward equality
# (real-valued weights for LIF / adLIF only: no product order is involved there; the recurrent layers' boundary product
# s_T Vm is exact on the dyadic networks, in any order)
FORWARD = [(c, r) for c in CASES for r in (False, True) if not (r and orc.RECURRENT[c[0]])]


@pytest.mark.parametrize("norm", NORMS, ids=norm_id)
@pytest.mark.parametrize("case,real", FORWARD, ids=lambda v: case_id(v) if isinstance(v, tuple) else ("realw" if v else "dyadic"))
def test_chained_forward_is_the_whole_sequence_bit_for_bit(sp, case, norm, real):  # noqa: F811
    kind, B, sizes = case
    net, x, gout, state0 = make(sp, kind, B, sizes, *norm, real=real)
    xd = x.to(DEV)
    with torch.no_grad():
        out_w, _, final_w, spikes_w = chained(net, xd, CHUNKINGS["whole"], on_device(state0))
        assert all(float(s.sum()) > 0 for s in spikes_w)
        for name in ("ones", "sevens", "uneven"):
            out_c, _, final_c, spikes_c = chained(net, xd, CHUNKINGS[name], on_device(state0))
            for a, b in zip(spikes_c, spikes_w):
                assert torch.equal(a, b), name
            for a, b in zip(final_c, final_w):
                assert set(a) == set(b)
                for k in a:
                    assert a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (name, k)
            within(out_c.cpu().numpy(), out_w.cpu().numpy(), OUT_CAP * float(out_w.abs().max()), f"out {name}")
        # the returned state is what the streaming class carries after the same chunks, and it takes it back
        net.eval()      # (no dropout, and BatchNorm only in eval: the stream computes what the forward above did)
        st = sp.StreamingSNN(net, B)
        st.reset(states=on_device(state0))
        t0 = 0
        for n in CHUNKINGS["uneven"]:
            st.step(xd[:, t0:t0 + n])
            t0 += n
        for a, b in zip(st.get_state(), final_c):
            for k in b:
                assert torch.equal(a[k], b[k]), k
        st.reset(states=final_c)
        carried = [{k: v for k, v in d.items() if k in ("u", "w", "s")} for d in st.get_state()]
        nxt, _, _ = net(xd[:, :3], state=carried, return_state=True)
        ref, _, _ = net(xd[:, :3], state=final_c, return_state=True)
        assert torch.equal(nxt, ref)


def test_state_none_draws_as_always_and_return_state_false_returns_as_always(sp):  # noqa: F811
    net, x, gout, state0 = make(sp, "adLIF", 3, (10, 36, 5), "none", True)
    xd = x.to(DEV)
    with torch.no_grad():
        torch.manual_seed(5)
        out_a, rates_a = net(xd)
        torch.manual_seed(5)
        out_b, rates_b, final = net(xd, return_state=True)
        after = torch.rand(1)
        torch.manual_seed(5)
        net(xd)
        assert torch.equal(after, torch.rand(1))                  # the same number of draws from the host generator
        assert torch.equal(out_a, out_b) and torch.equal(rates_a, rates_b)
        torch.manual_seed(5)
        res = net(xd, state=on_device(state0))
        first = torch.rand(1)
        torch.manual_seed(5)
        assert len(res) == 2 and torch.equal(first, torch.rand(1))      # with a state given nothing was drawn
        assert [sorted(d) for d in final] == [["s", "u", "w"], ["s", "u", "w"], ["u"]]


# ---------------------------------------------------------------------------------------------- 2. gradient chain
@pytest.mark.parametrize("norm", NORMS, ids=norm_id)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_gradients_cross_the_chunk_boundaries(sp, case, norm, record_property):  # noqa: F811
    kind, B, sizes = case
    net, x, gout, state0 = make(sp, kind, B, sizes, *norm)
    out_o, spikes_o, grads_o, final_o = oracle_grads(net, kind, x, CHUNKINGS["whole"], state0, gout, *norm)
    out_w, spikes_w, grads_w, final_w = device_grads(net, x, CHUNKINGS["whole"], state0, gout)
    for a, b in zip(spikes_w, spikes_o):
        assert torch.equal(a, b)
    worst = [compare_grads(grads_w, grads_o, "whole vs oracle")]
    for name in ("ones", "sevens", "uneven"):
        out_c, spikes_c, grads_c, final_c = device_grads(net, x, CHUNKINGS[name], state0, gout)
        worst.append(compare_grads(grads_c, grads_w, f"{name} vs whole"))
        worst.append(compare_grads(grads_c, grads_o, f"{name} vs oracle"))
        worst.append(within(out_c.numpy(), out_o.numpy(), OUT_CAP * float(out_o.abs().max()), f"out {name}"))
        for i, d in enumerate(final_c):     # unpadded, whatever the width
            assert all(v.shape == (B, sizes[i]) for v in d.values())
    record(record_property, *worst)


@pytest.mark.parametrize("name", ["triangle"])
@pytest.mark.parametrize("case", SOME, ids=case_id)
def test_gradients_cross_the_chunk_boundaries_with_a_smooth_surrogate(sp, case, name, record_property):  # noqa: F811
    kind, B, sizes = case
    sg = (name, TEST_SCALE[name])
    net, x, gout, state0 = make(sp, kind, B, sizes, "none", True, surrogate=sg)
    _, _, grads_o, _ = oracle_grads(net, kind, x, CHUNKINGS["whole"], state0, gout, "none", True, surrogate=sg)
    worst = []
    for chunks in ("whole", "uneven", "ones"):
        _, _, grads_c, _ = device_grads(net, x, CHUNKINGS[chunks], state0, gout)
        worst.append(compare_grads(grads_c, grads_o, f"{chunks} vs oracle"))
    record(record_property, *worst)


@pytest.mark.parametrize("name", ["sevens", "uneven", "ones"])
@pytest.mark.parametrize("kind", ["LIF", "adLIF"])
def test_dwx_of_the_chained_run_is_the_whole_sequence_runs_bit_for_bit(sp, kind, name, monkeypatch):  # noqa: F811
    """On a dyadic network with a dyadic cotangent, dWx of both hidden layers, every chunking.

    A chunk boundary hands over the ROUNDED sums g_sT = -alpha du + b dw and g_uT = alpha du + a dw, and fp32 addition
    does not reassociate (alpha, a, b and with them du, dw are not dyadic, whatever the weights are).  The stateful
    kernels therefore form exactly these two sums first at EVERY step and add them to the incoming gradient and to the
    gate: a boundary then rounds as an inner step does.  (With the plain kernels' order, (gs - alpha du) + b dw, the
    adLIF cases differed by 2e-10 .. 3e-8 of max-abs.)  The rate term of the loss is left out here: its weight n / T is
    not dyadic."""
    F_ = _Fn()
    net, x, gout, state0 = make(sp, kind, 3, (10, 36, 5), "none", True)
    calls, orig = [], F_.cell_backward

    def recording(*a, **kw):
        dWx, grads = orig(*a, **kw)
        calls.append(dWx.detach().clone())
        return dWx, grads

    monkeypatch.setattr(F_, "cell_backward", recording)

    def dwx_of(chunks):
        calls.clear()
        device_grads(net, x, chunks, state0, gout, rates_term=False)    # (n / T is not dyadic)
        per_layer = {}
        for d in calls:                       # the backward walks the chunks last to first
            per_layer.setdefault(d.shape[-1], []).insert(0, d)
        return {h: torch.cat(v, dim=1) for h, v in per_layer.items()}

    whole = dwx_of(CHUNKINGS["whole"])
    got = dwx_of(CHUNKINGS[name])
    assert set(got) == set(whole) == {10, 36}
    diff = {h: float((got[h] - whole[h]).abs().max()) / float(whole[h].abs().max()) for h in whole}
    for h in whole:
        print(f"  {kind} {name} H={h}: max |dWx - whole| / max |whole| = {diff[h]:.3e}")
    assert all(torch.equal(got[h], whole[h]) for h in whole), (kind, name, diff)


# ---------------------------------------------------------------------------------------------- 3. state gradients alone
@pytest.mark.parametrize("norm", NORMS[:2], ids=norm_id)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_state_gradients_alone_and_output_gradients_alone(sp, case, norm, record_property):  # noqa: F811
    kind, B, sizes = case
    net, x, gout, state0 = make(sp, kind, B, sizes, *norm)
    worst = []
    for form in ("state", "out"):     # a loss on the returned state only (out unused); a loss on out only
        _, _, grads_o, _ = oracle_grads(net, kind, x, [T], state0, gout, *norm, form=form)
        _, _, grads_d, _ = device_grads(net, x, [T], state0, gout, form=form)
        worst.append(compare_grads(grads_d, grads_o, f"{form} only"))
    record(record_property, *worst)


@pytest.mark.parametrize("case", SOME, ids=case_id)
def test_spike_state_gradient_enters_behind_the_dropout_scale(sp, case, record_property):  # noqa: F811
    """g_sT alone, dropout 0.25: the oracle runs with the kernels' own mask (tests/dropout_numpy.py).  A kernel that
    scaled g_sT by the dropout factor would zero a quarter of it and scale the rest by 4/3."""
    kind, B, sizes = case
    net, x, gout, state0 = make(sp, kind, B, sizes, "none", True, dropout=0.25)
    # (a recurrent layer runs at its width padded to a multiple of 4, and its mask is indexed there)
    pad = (lambda H: (H + 3) // 4 * 4) if orc.RECURRENT[kind] else (lambda H: H)
    masks = [torch.from_numpy(dn.keep_mask_padded(1234 + 7919 * k, B, T, 1, H, pad(H), 0.25)) for k, H in enumerate(sizes[:-1])]

    def spike_form(final):
        g = torch.Generator().manual_seed(9)
        return sum((st["s"] * (torch.round(torch.randn(st["s"].shape, generator=g) * 4) / 4).to(st["s"].device)).sum()
                   for st in final[:-1])

    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in net.state_dict().items()}
    so_state = [{k: v.clone().requires_grad_(True) for k, v in d.items()} for d in state0]
    xo = x.clone().requires_grad_(True)
    _, _, final_o, spikes_o = so.chained(xo, [T], p, so_state, neuron_type=kind, num_layers=3, normalization="none",
                                         training=True, drop_masks=masks)
    spike_form(final_o).backward()
    net.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(True)
    st = on_device(state0, grad=True)
    _, _, final_d, spikes_d = chained(net, xd, [T], st)
    for a, b in zip(spikes_d, spikes_o):
        assert torch.equal(a.cpu(), b.detach())             # the same mask on both sides
    spike_form(final_d).backward()
    _Fn().check_status()
    got = {k: v.grad.cpu() for k, v in net.named_parameters() if v.grad is not None}
    ref = {k: v.grad for k, v in p.items() if v.grad is not None and k in got}
    got["x"], ref["x"] = xd.grad.cpu(), xo.grad
    for i, (d, o) in enumerate(zip(st[:-1], so_state[:-1])):
        for k in d:
            got[f"state{i}.{k}"], ref[f"state{i}.{k}"] = d[k].grad.cpu(), o[k].grad
    ref = {k: v for k, v in ref.items() if float(v.abs().max()) > 0}
    record(record_property, compare_grads({k: got[k] for k in ref}, ref, "g_sT alone, dropout"))
    assert any(k.startswith("state0") for k in ref) and "snn.0.W.weight" in ref


# ---------------------------------------------------------------------------------------------- 4. BatchNorm, train mode
@pytest.mark.parametrize("case", SOME, ids=case_id)
def test_batchnorm_in_train_mode_takes_each_chunk_as_its_batch(sp, case, record_property):  # noqa: F811
    kind, B, sizes = case
    net, x, gout, state0 = make(sp, kind, B, sizes, "batchnorm", True)
    chunks = [13, 11]
    p = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point() and "running" not in k)
         for k, v in net.state_dict().items() if "num_batches" not in k}
    st = [{k: v.clone().requires_grad_(True) for k, v in d.items()} for d in state0]
    xo = x.clone().requires_grad_(True)
    cur, t0, total, rates = st, 0, 0, []
    for n in chunks:           # the oracle chunk by chunk: every chunk's statistics are its own B * n rows
        stats = {}
        out, r, cur = so.snn_forward(xo[:, t0:t0 + n], p, neuron_type=kind, num_layers=3, state=cur,
                                     normalization="batchnorm", training=True, stats=stats)
        for k, v in stats.items():
            p[k] = v
        total, t0 = total + out, t0 + n
        rates.append(r)
    loss_of(total, rates, chunks, cur, gout).backward()
    grads_o = {k: v.grad for k, v in p.items() if v.requires_grad}
    grads_o["x"] = xo.grad
    for i, d in enumerate(st):
        for k, v in d.items():
            grads_o[f"state{i}.{k}"] = v.grad
    out_d, _, grads_d, final_d = device_grads(net, x, chunks, state0, gout)
    worst = [compare_grads(grads_d, grads_o, "batchnorm train"),
             within(out_d.numpy(), total.detach().numpy(), OUT_CAP * float(total.detach().abs().max()), "out")]
    for k, v in net.state_dict().items():
        if "running" in k:
            worst.append(within(v.cpu().numpy(), p[k].numpy(), OUT_CAP * float(p[k].abs().max()), k))
        if "num_batches" in k:
            assert int(v) == 2
    record(record_property, *worst)


# ---------------------------------------------------------------------------------------------- 5. detach
def test_detached_state_is_truncated_bptt(sp):  # noqa: F811
    from sparch_amd.snns import detach_state
    net, x, gout, state0 = make(sp, "adLIF", 3, (10, 36, 5), "none", True)
    xd = x.to(DEV)
    st0 = on_device(state0, grad=True)
    out1, r1, st1 = net(xd[:, :13], state=st0, return_state=True)
    cut = detach_state(st1)
    assert all(not v.requires_grad for d in cut for v in d.values())
    net.zero_grad(set_to_none=True)
    out2, r2, st2 = net(xd[:, 13:], state=cut, return_state=True)
    loss_of(out2, [r2], [11], st2, gout).backward()
    _Fn().check_status()
    assert all(v.grad is None for d in st0 for v in d.values())          # nothing crossed the boundary
    got = {k: v.grad.clone() for k, v in net.named_parameters()}
    # the second chunk alone, from the same values
    net.zero_grad(set_to_none=True)
    out3, r3, st3 = net(xd[:, 13:], state=[{k: v.clone() for k, v in d.items()} for d in cut], return_state=True)
    loss_of(out3, [r3], [11], st3, gout).backward()
    for k, v in net.named_parameters():
        assert torch.equal(got[k], v.grad), k
    # and the first chunk's graph is still whole: its own backward runs and reaches the first state
    (out1 * gout.to(DEV)).sum().backward()
    assert all(v.grad is not None for d in st0 for v in d.values())


# ---------------------------------------------------------------------------------------------- the wide kernels
@pytest.mark.parametrize("kind", ["LIF", "adLIF", "RLIF", "RadLIF"])
def test_wide_network_h1024(sp, kind, record_property):  # noqa: F811
    """H = 1024, B = 33: the recurrent kinds' full-width grid (two row tiles x 32 workgroups)."""
    net, x, gout, state0 = make(sp, kind, 33, (1024, 1024, 35), "none", True)
    _, spikes_o, grads_o, _ = oracle_grads(net, kind, x, [T], state0, gout, "none", True)
    _, spikes_c, grads_c, _ = device_grads(net, x, CHUNKINGS["uneven"], state0, gout)
    for a, b in zip(spikes_c, spikes_o):
        assert torch.equal(a, b)
    record(record_property, compare_grads(grads_c, grads_o, "H=1024 uneven vs oracle"))


@pytest.mark.parametrize("bn", [False, True], ids=["plain", "bnsums"])
@pytest.mark.parametrize("surrogate", [None, ("triangle", TEST_SCALE["triangle"])], ids=["boxcar", "triangle"])
@pytest.mark.parametrize("kind", ["LIF", "adLIF"])
def test_cell_backward_st_four_neurons_per_thread(sp, kind, surrogate, bn, record_property):  # noqa: F811
    """functional.cell_backward(state_grads=, want_state_grads=) at B x H = 512 x 1024, where the launch rule gives a
    thread four neurons (VEC = 4), against the oracle cell's autograd; with dropout, and with BatchNorm's sums folded in."""
    F_ = _Fn()
    B, H, Tc, p_drop, seed = 512, 1024, 6, 0.25, 4242
    g = torch.Generator().manual_seed(21)
    p = {"alpha": torch.rand(H, generator=g) * 0.16 + 0.8}
    if kind == "adLIF":
        p.update(beta=torch.rand(H, generator=g) * 0.03 + 0.965, a=torch.rand(H, generator=g) * 2.2 - 1.1,
                 b=torch.rand(H, generator=g) * 2.2 - 0.1)
    Wx = torch.rand(B, Tc, H, generator=g) * 3
    u0, w0, s0 = (torch.rand(B, H, generator=g) for _ in range(3))
    if kind != "adLIF":
        w0 = None
    g_out = torch.randn(B, Tc, H, generator=g)
    g_T = [torch.randn(B, H, generator=g) for _ in range(3)]
    mask = torch.from_numpy(dn.keep_mask(seed, (B, Tc, H), p_drop))
    # the oracle
    leaves = [t.clone().requires_grad_(True) for t in (u0, w0, s0) if t is not None]
    lu, lw, ls = (leaves[0], leaves[1], leaves[2]) if w0 is not None else (leaves[0], None, leaves[1])
    po = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    Wo = Wx.clone().requires_grad_(True)
    old = orc.spike
    if surrogate is not None:
        from sparch_amd.snns import SpikeFunctionSurrogate
        orc.spike = lambda d: SpikeFunctionSurrogate.apply(d, *surrogate)
    try:
        s, fin = so.spiking_cell(kind, Wo, po, lu, lw, ls)
    finally:
        orc.spike = old
    loss = (s * mask * g_out).sum() + (fin["u"] * g_T[0]).sum() + (fin["s"] * g_T[2]).sum()
    if lw is not None:
        loss = loss + (fin["w"] * g_T[1]).sum()
    loss.backward()
    # the device
    pd = {k: v.to(DEV) for k, v in p.items()}
    ud, wd, sd = (None if t is None else t.to(DEV) for t in (u0, w0, s0))
    s_out, count, saved, s16 = F_.cell_forward(kind, Wx.to(DEV), None, None, pd, ud, wd, sd, B=B, dirs=1, theta=1.0,
                                               p_drop=p_drop, seed=seed)
    assert torch.equal(s_out.cpu(), (s * mask).detach())
    assert torch.equal(saved[0][:, -1].cpu(), fin["u"].detach())
    bn_arg = None
    if bn:
        bn_arg = (Wx.to(DEV), torch.zeros(H, device=DEV), torch.ones(H, device=DEV))
    dWx, grads = F_.cell_backward(kind, g_out.to(DEV), None, pd, ud, wd, sd, saved, B=B, dirs=1, T=Tc, H=H, theta=1.0,
                                  p_drop=p_drop, seed=seed, bn=bn_arg, surrogate=surrogate,
                                  state_grads=tuple(t.to(DEV) if (i != 1 or lw is not None) else None for i, t in enumerate(g_T)),
                                  want_state_grads=True)
    F_.check_status()
    bar = lambda r: GRAD_CAP * float(r.abs().max())  # noqa: E731
    worst = [within(dWx.cpu().numpy(), Wo.grad.numpy(), bar(Wo.grad), "dWx")]
    for name, leaf, got in (("g_u0", lu, grads["state"][0]), ("g_w0", lw, grads["state"][1]), ("g_s0", ls, grads["state"][2])):
        if leaf is None:
            assert got is None
            continue
        worst.append(within(got.cpu().numpy(), leaf.grad.numpy(), bar(leaf.grad), name))
    for k in po:
        worst.append(within(grads[k].cpu().numpy(), po[k].grad.numpy(), bar(po[k].grad), k))
    if bn:      # mean 0, invstd 1: the sums of dWx and of dWx * x
        dbeta, dgamma = grads["bn_sums"]
        ref_b, ref_g = Wo.grad.sum(dim=(0, 1)), (Wo.grad * Wx).sum(dim=(0, 1))
        worst.append(within(dbeta.cpu().numpy(), ref_b.numpy(), bar(ref_b), "bn dbeta"))
        worst.append(within(dgamma.cpu().numpy(), ref_g.numpy(), bar(ref_g), "bn dgamma"))
    record(record_property, *worst)


# ---------------------------------------------------------------------------------------------- 7. SPARCH_TBPTT
def test_run_exp_with_sparch_tbptt(tmp_path):
    """run_exp.py with SPARCH_TBPTT=8 on synthetic SHD-shaped data, in a child process: one epoch of two batches of T = 20
    steps ends with a finite loss after ceil(20 / 8) optimizer steps per batch."""
    exp, seq_len = tmp_path / "exp", 20
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPARCH_")}
    env["SPARCH_TBPTT"] = "8"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_exp.py"), "--model_type", "adLIF", "--dataset_name", "shd",
                        "--synthetic", "1", "--synthetic_batches", "2", "--seq_len", str(seq_len), "--nb_epochs", "1",
                        "--nb_layers", "3", "--nb_hiddens", "64", "--batch_size", "8", "--log_tofile", "1",
                        "--new_exp_folder", str(exp)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    log = (exp / "log" / "exp.log").read_text()
    loss = [float(v) for v in re.findall(r"Epoch 1: train loss=(\S+)", log)]
    assert len(loss) == 1 and np.isfinite(loss[0])
    steps = [int(v) for v in re.findall(r"optimizer steps=(\d+)", log)]
    assert steps == [2 * math.ceil(seq_len / 8)]
    assert "Test acc=" in log and "nan" not in log.lower()
