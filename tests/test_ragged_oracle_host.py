"""
tests/ragged_oracle.py pinned against the reference-faithful oracle (oracle.snn_oracle.snn_forward) where the two must
agree:
  * all lengths == T: the same network, outputs, rates, gradients and running statistics;
  * normalisation none / layernorm: row b and its share of every gradient equal snn_forward on x[b:b+1, :L_b];
  * B = 1, L < T with BatchNorm: snn_forward on the truncated clip, running statistics included.
Spikes are compared exactly; everything else to fp32 rounding (the bars of tests/test_oracle_golden.py's network cases:
outputs rtol 2e-5 / atol 2e-6, gradients rtol 2e-4 / atol 2e-6, running statistics rtol 1e-5 / atol 1e-6).
"""
import numpy as np
import pytest
import torch

from oracle import snn_oracle as orc
from tests import ragged_oracle as rag

KINDS = ["LIF", "adLIF", "RLIF", "RadLIF"]
SIZES = [12, 8, 5]
B, T, C = 4, 9, 7
LENGTHS = [9, 1, 4, 6]


def make_params(kind, normalization, seed, bias=False):
    g = torch.Generator().manual_seed(seed)
    p = {}
    fan = C
    for i, H in enumerate(SIZES):
        pre = f"snn.{i}."
        p[pre + "W.weight"] = torch.randn(H, fan, generator=g) * 0.6 + 0.5  # (a positive drive: every layer spikes)
        if bias:
            p[pre + "W.bias"] = torch.randn(H, generator=g) * 0.1
        p[pre + "alpha"] = torch.rand(H, generator=g) * 0.2 + 0.78
        last = i == len(SIZES) - 1
        if not last and orc.ADAPTIVE[kind]:
            p[pre + "beta"] = torch.rand(H, generator=g) * 0.05 + 0.95
            p[pre + "a"] = torch.rand(H, generator=g) * 1.6 - 0.8
            p[pre + "b"] = torch.rand(H, generator=g) * 1.5
        if not last and orc.RECURRENT[kind]:
            p[pre + "V.weight"] = torch.randn(H, H, generator=g) * 0.3
        if normalization in ("batchnorm", "layernorm"):
            p[pre + "norm.weight"] = torch.rand(H, generator=g) + 1.5
            p[pre + "norm.bias"] = torch.randn(H, generator=g) * 0.2 + 0.6
        if normalization == "batchnorm":
            p[pre + "norm.running_mean"] = torch.randn(H, generator=g) * 0.1
            p[pre + "norm.running_var"] = torch.rand(H, generator=g) + 0.5
        fan = H
    x = torch.randn(B, T, C, generator=g) + 1.5
    gout = torch.randn(B, SIZES[-1], generator=g)
    grate = torch.randn(sum(SIZES[:-1]), generator=g)
    torch.manual_seed(seed + 1)
    init = orc.draw_init_states(B, SIZES, kind)
    return p, x, gout, grate, init


def leaves(p):
    return {k: v.clone().requires_grad_("running" not in k) for k, v in p.items()}


def close(a, b, rtol, atol, what):
    np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=rtol, atol=atol, err_msg=what)


@pytest.mark.parametrize("normalization", ["batchnorm", "layernorm", "none"])
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("kind", KINDS)
def test_full_lengths_equal_the_reference_oracle(kind, normalization, training):
    p, x, gout, grate, init = make_params(kind, normalization, 11, bias=normalization != "batchnorm")
    pa, pb = leaves(p), leaves(p)
    sa, sb, spa, spb = {}, {}, [], []
    out_a, rates_a = rag.snn_forward(x, [T] * B, pa, neuron_type=kind, num_layers=3, init_states=init,
                                     normalization=normalization, training=training, stats=sa, spikes_out=spa)
    out_b, rates_b = orc.snn_forward(x, pb, neuron_type=kind, num_layers=3, init_states=init,
                                     normalization=normalization, training=training, stats=sb, spikes_out=spb)
    for a, b in zip(spa, spb):
        assert torch.equal(a, b)
    assert float(rates_b.detach()[SIZES[0]:].sum()) > 0  # (the second layer spikes too)
    close(out_a, out_b, 2e-5, 2e-6, "out")
    close(rates_a, rates_b, 1e-6, 1e-7, "rates")
    ((out_a * gout).sum() + (rates_a * grate).sum()).backward()
    ((out_b * gout).sum() + (rates_b * grate).sum()).backward()
    for k in pa:
        if pa[k].requires_grad:
            close(pa[k].grad, pb[k].grad, 2e-4, 2e-6, k)
    assert sa.keys() == sb.keys()
    for k in sa:
        close(sa[k], sb[k], 1e-5, 1e-6, k)


@pytest.mark.parametrize("normalization", ["layernorm", "none"])
@pytest.mark.parametrize("kind", KINDS)
def test_each_row_is_its_clip_run_alone(kind, normalization):
    """Without batch statistics the rows do not see each other: row b's output, its spikes and its share of every
    gradient are those of snn_forward on the truncated clip (a bias is on: it reaches the padded rows)."""
    p, x, gout, grate, init = make_params(kind, normalization, 23, bias=True)
    mask = rag.valid_mask(LENGTHS, T)
    x = x * mask[:, :, None]
    pa = leaves(p)
    spa = []
    out_a, rates_a = rag.snn_forward(x, LENGTHS, pa, neuron_type=kind, num_layers=3, init_states=init,
                                     normalization=normalization, training=True, spikes_out=spa)
    N = sum(LENGTHS)
    ((out_a * gout).sum() + (rates_a * grate).sum()).backward()
    pb = leaves(p)
    count = torch.zeros_like(rates_a)
    for b, L in enumerate(LENGTHS):
        init_b = [{k: v[b:b + 1] for k, v in st.items()} for st in init]
        spb = []
        out_b, rates_b = orc.snn_forward(x[b:b + 1, :L], pb, neuron_type=kind, num_layers=3, init_states=init_b,
                                         normalization=normalization, training=True, spikes_out=spb)
        for a, s in zip(spa, spb):
            assert torch.equal(a[b:b + 1, :L], s)
            assert not a[b, L:].any()
        close(out_a[b:b + 1], out_b, 2e-5, 2e-6, f"out[{b}]")
        count = count + rates_b.detach() * L
        # the rate of the ragged batch is sum_b L_b rate_b / N: the same weights on the gradient
        ((out_b * gout[b:b + 1]).sum() + (rates_b * grate).sum() * (L / N)).backward()
    assert float(count[SIZES[0]:].sum()) > 0
    close(rates_a, count / N, 1e-5, 1e-7, "rates")
    for k in pa:
        close(pa[k].grad, pb[k].grad, 2e-4, 2e-6, k)


@pytest.mark.parametrize("kind", KINDS)
def test_one_short_clip_with_batchnorm_equals_the_truncated_clip(kind):
    p, x, gout, grate, init = make_params(kind, "batchnorm", 37)
    L = 5
    init1 = [{k: v[:1] for k, v in st.items()} for st in init]
    x1 = x[:1] * rag.valid_mask([L], T)[:, :, None]
    pa, pb = leaves(p), leaves(p)
    sa, sb = {}, {}
    out_a, rates_a = rag.snn_forward(x1, [L], pa, neuron_type=kind, num_layers=3, init_states=init1,
                                     normalization="batchnorm", training=True, stats=sa)
    out_b, rates_b = orc.snn_forward(x1[:, :L], pb, neuron_type=kind, num_layers=3, init_states=init1,
                                     normalization="batchnorm", training=True, stats=sb)
    close(out_a, out_b, 2e-5, 2e-6, "out")
    close(rates_a, rates_b, 1e-6, 1e-7, "rates")
    ((out_a * gout[:1]).sum() + (rates_a * grate).sum()).backward()
    ((out_b * gout[:1]).sum() + (rates_b * grate).sum()).backward()
    for k in pa:
        if pa[k].requires_grad:
            close(pa[k].grad, pb[k].grad, 2e-4, 2e-6, k)
    assert sa.keys() == sb.keys() and sa
    for k in sa:
        close(sa[k], sb[k], 1e-5, 1e-6, k)
