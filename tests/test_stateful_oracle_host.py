"""The stateful-training oracle (tests/stateful_oracle.py) against the reference-faithful oracle and against autograd:
no GPU.  What it pins:

  * started from the same states, the helper's spikes and `out` are oracle.snn_oracle.snn_forward's bit for bit;
  * chained through any chunking, the sum of `out` and every gradient (parameters, input, first state) are the
    whole-sequence run's within fp32 reassociation (GRAD_CAP of the tensor's max-abs, tests/network_cases.py);
  * the closed forms that turn the reverse pass's last carries into the initial state's gradient equal autograd's.
"""
import math

import pytest
import torch

from oracle import snn_oracle as orc
from tests import stateful_oracle as so
from tests.network_cases import GRAD_CAP, OUT_CAP

KINDS = ("LIF", "adLIF", "RLIF", "RadLIF")
T = 24
CHUNKINGS = {"whole": [24], "ones": [1] * 24, "sevens": [7, 7, 7, 3], "uneven": [5, 1, 13, 2, 3]}


def make_case(kind, B=3, C=20, sizes=(10, 36, 5), normalization="none", seed=0, use_bias=False):
    """Parameters under the reference's state_dict keys, a 0/1 input, a cotangent and a first state."""
    g = torch.Generator().manual_seed(1000 + seed)
    p, fan = {}, C
    for k, H in enumerate(sizes):
        pre, hidden = f"snn.{k}.", k < len(sizes) - 1
        p[pre + "W.weight"] = (torch.rand(H, fan, generator=g) * 2 - 1) / math.sqrt(fan) * 4 + (0.25 if k == 0 else 0.1)
        if use_bias:
            p[pre + "W.bias"] = torch.rand(H, generator=g) * 0.2
        p[pre + "alpha"] = torch.rand(H, generator=g) * 0.2 + 0.78  # (a few below the clamp range)
        if hidden and orc.ADAPTIVE[kind]:
            p[pre + "beta"] = torch.rand(H, generator=g) * 0.04 + 0.96
            p[pre + "a"] = torch.rand(H, generator=g) * 2.2 - 1.1
            p[pre + "b"] = torch.rand(H, generator=g) * 2.2 - 0.1
        if hidden and orc.RECURRENT[kind]:
            p[pre + "V.weight"] = torch.nn.init.orthogonal_(torch.empty(H, H), generator=g) * 0.5
        if normalization in ("batchnorm", "layernorm"):
            p[pre + "norm.weight"] = torch.rand(H, generator=g) + 1.0
            p[pre + "norm.bias"] = torch.rand(H, generator=g) * 0.5 + 0.5
        if normalization == "batchnorm":
            p[pre + "norm.running_mean"] = torch.rand(H, generator=g) * 0.2
            p[pre + "norm.running_var"] = torch.rand(H, generator=g) * 0.5 + 0.5
        fan = H
    x = (torch.rand(B, T, C, generator=g) < 0.3).float()
    gout = torch.randn(B, sizes[-1], generator=g)
    state = []
    for k, H in enumerate(sizes):
        if k == len(sizes) - 1:
            state.append({"u": torch.rand(B, H, generator=g)})
        else:
            st = {"u": torch.rand(B, H, generator=g)}
            if orc.ADAPTIVE[kind]:
                st["w"] = torch.rand(B, H, generator=g)
            st["s"] = torch.rand(B, H, generator=g)
            state.append(st)
    return p, x, gout, state


def leaves(p, x, state):
    p = {k: v.clone().requires_grad_("running" not in k) for k, v in p.items()}
    x = x.clone().requires_grad_(True)
    state = [{k: v.clone().requires_grad_(True) for k, v in st.items()} for st in state]
    return p, x, state


def run(kind, chunks, p, x, gout, state, normalization="none", training=True):
    p, x, state = leaves(p, x, state)
    out, rates, final, spikes = so.chained(x, chunks, p, state, neuron_type=kind, num_layers=3,
                                           normalization=normalization, training=training)
    # the loss: a cotangent on the summed output, the whole sequence's firing rates (the chunks' means weighted by their
    # steps), and the state the sequence ended in
    loss = ((out * gout).sum() + sum(r.sum() * (n / T) for r, n in zip(rates, chunks))
            + sum((v * 0.25).sum() for st in final for v in st.values()))
    loss.backward()
    grads = {k: v.grad for k, v in p.items() if v.requires_grad}
    grads["x"] = x.grad
    for i, st in enumerate(state):
        for k, v in st.items():
            grads[f"state{i}.{k}"] = v.grad
    return out.detach(), [s.detach() for s in spikes], grads, [{k: v.detach() for k, v in st.items()} for st in final]


@pytest.mark.parametrize("normalization", ["none", "batchnorm", "layernorm"])
@pytest.mark.parametrize("kind", KINDS)
def test_whole_sequence_equals_the_reference_oracle_bit_for_bit(kind, normalization):
    p, x, gout, state = make_case(kind, normalization=normalization)
    spikes, stats, stats_ref, spikes_ref = [], {}, {}, []
    out, rates, final = so.snn_forward(x, p, neuron_type=kind, num_layers=3, state=state, normalization=normalization,
                                       stats=stats, spikes_out=spikes)
    init = [{k + "0": v for k, v in st.items()} for st in state]
    out_ref, rates_ref = orc.snn_forward(x, p, neuron_type=kind, num_layers=3, init_states=init,
                                         normalization=normalization, stats=stats_ref, spikes_out=spikes_ref)
    assert sum(float(s.sum()) for s in spikes) > 0
    for s, r in zip(spikes, spikes_ref):
        assert torch.equal(s, r)
    assert torch.equal(out, out_ref) and torch.equal(rates, rates_ref)
    for k in stats_ref:
        assert torch.equal(stats[k], stats_ref[k])
    # the final state: the last spike of every hidden layer, and shapes as the first state's
    for st, s, first in zip(final, spikes, state):
        assert torch.equal(st["s"], s[:, -1])
        assert {k: v.shape for k, v in st.items()} == {k: v.shape for k, v in first.items()}


@pytest.mark.parametrize("normalization,training", [("none", True), ("layernorm", True), ("batchnorm", False)])
@pytest.mark.parametrize("name", [n for n in CHUNKINGS if n != "whole"])
@pytest.mark.parametrize("kind", KINDS)
def test_chained_chunks_equal_the_whole_sequence(kind, name, normalization, training):
    case = make_case(kind, normalization=normalization)
    out_w, spikes_w, grads_w, final_w = run(kind, CHUNKINGS["whole"], *case, normalization=normalization, training=training)
    out_c, spikes_c, grads_c, final_c = run(kind, CHUNKINGS[name], *case, normalization=normalization, training=training)
    for a, b in zip(spikes_c, spikes_w):
        assert torch.equal(a, b)
    for a, b in zip(final_c[:-1], final_w[:-1]):      # the hidden states: no sum is split, bit-equal
        for k in a:
            assert torch.equal(a[k], b[k])
    assert float((out_c - out_w).abs().max()) <= OUT_CAP * float(out_w.abs().max())
    assert set(grads_c) == set(grads_w)
    for k, ref in grads_w.items():
        assert ref is not None and float(ref.abs().max()) > 0, k
        assert float((grads_c[k] - ref).abs().max()) <= GRAD_CAP * float(ref.abs().max()), k


@pytest.mark.parametrize("kind", KINDS)
def test_closed_form_state_gradients_equal_autograd(kind):
    B, H = 3, 12
    g = torch.Generator().manual_seed(7)
    p = {"alpha": torch.rand(H, generator=g) * 0.14 + 0.82}
    if orc.ADAPTIVE[kind]:
        p.update(beta=torch.rand(H, generator=g) * 0.02 + 0.97, a=torch.rand(H, generator=g) * 2 - 1,
                 b=torch.rand(H, generator=g) * 2)
    if orc.RECURRENT[kind]:
        p["V"] = torch.nn.init.orthogonal_(torch.empty(H, H), generator=g)
    Wx = torch.rand(B, T, H, generator=g) * 3
    u0, w0, s0 = (torch.rand(B, H, generator=g).requires_grad_(True) for _ in range(3))
    # the first step on its own: its final state holds u_1, w_1 and s_1 = spike(u_1), so their .grad are the TOTAL
    # gradients du_1, dw_1 of the recurrences
    s_first, st1 = so.spiking_cell(kind, Wx[:, :1], p, u0, w0, s0)
    s_rest, st_T = so.spiking_cell(kind, Wx[:, 1:], p, st1["u"], st1.get("w"), st1["s"])
    for v in st1.values():
        v.retain_grad()
    cot = torch.randn(B, T, H, generator=g)
    loss = (torch.cat([s_first, s_rest], dim=1) * cot).sum() + sum((v * 0.5).sum() for v in st_T.values())
    loss.backward()
    assert float(s_rest.detach().sum()) > 0
    du1 = st1["u"].grad
    dw1 = st1["w"].grad if orc.ADAPTIVE[kind] else None
    g_u0, g_w0, g_s0 = so.closed_form_state_grads(kind, p, du1, dw1)
    # three products and two sums of fp32 numbers against autograd's own order: a few ulp of the largest term
    for got, ref, what in ((g_u0, u0.grad, "u0"), (g_s0, s0.grad, "s0")) + (((g_w0, w0.grad, "w0"),) if dw1 is not None else ()):
        assert float(ref.abs().max()) > 0, what
        assert float((got - ref).abs().max()) <= 1e-6 * float(ref.abs().max()), what
    if dw1 is None:
        assert g_w0 is None and w0.grad is None
