"""
tests/bidir_ragged_oracle.py pinned against the reference-faithful oracle (oracle.snn_oracle.snn_forward with
bidirectional=True) where the two must agree, in fp64 to 1e-12, with eval-mode normalisation or none (batch statistics
couple the rows; the statistics themselves are pinned by the all-lengths-equal case in train mode):
  pin 1  all lengths == T: the same network — outputs, spikes, rates, input and parameter gradients;
  pin 2  ragged lengths: row b equals snn_forward(x[b:b+1, :L_b], bidirectional=True) with the state rows b and B + b —
         outputs, spikes, the rates (the rows' counts summed), input and parameter gradients (the rows' shares summed).
"""
import numpy as np
import pytest
import torch

from oracle import snn_oracle as orc
from tests import bidir_cases as bc
from tests import bidir_ragged_oracle as bro
from tests import ragged_oracle as rag

KINDS = ["LIF", "adLIF", "RLIF", "RadLIF"]
SIZES = [12, 8, 5]
B, T, C = 4, 9, 7
LENGTHS = [9, 1, 4, 6]
F64 = torch.float64


def make_params(kind, normalization, seed, bias=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g, dtype=F64)      # noqa: E731
    n = lambda *s: torch.randn(*s, generator=g, dtype=F64)     # noqa: E731
    p = {}
    fan = C
    for i, H in enumerate(SIZES):
        pre = f"snn.{i}."
        last = i == len(SIZES) - 1
        p[pre + "W.weight"] = n(H, fan) * 0.6 + 0.5  # (a positive drive: every layer spikes)
        if bias:
            p[pre + "W.bias"] = n(H) * 0.1
        p[pre + "alpha"] = r(H) * 0.2 + 0.78
        if not last and orc.ADAPTIVE[kind]:
            p[pre + "beta"] = r(H) * 0.05 + 0.95
            p[pre + "a"] = r(H) * 1.6 - 0.8
            p[pre + "b"] = r(H) * 1.5
        if not last and orc.RECURRENT[kind]:
            p[pre + "V.weight"] = n(H, H) * 0.3
        if normalization in ("batchnorm", "layernorm"):
            p[pre + "norm.weight"] = r(H) + 1.5
            p[pre + "norm.bias"] = n(H) * 0.2 + 0.6
        if normalization == "batchnorm":
            p[pre + "norm.running_mean"] = n(H) * 0.1 + (4.0, 1.0, 0.0)[i]   # (near the drive's own mean)
            p[pre + "norm.running_var"] = r(H) + 0.5
        fan = H if last else 2 * H
    x = n(B, T, C) + 1.5
    gout = n(B, SIZES[-1])
    grate = n(2 * sum(SIZES[:-1]))
    torch.manual_seed(seed + 1)
    init = [{k: v.to(F64) for k, v in st.items()} for st in orc.draw_init_states(B, SIZES, kind, bidirectional=True)]
    return p, x, gout, grate, init


@pytest.fixture(autouse=True)
def fp64_spikes():
    """Both oracles run in fp64 here: their spike function keeps the dtype for the length of a test."""
    with bro.own_dtype_spikes():
        yield


def leaves(p):
    return {k: v.clone().requires_grad_("running" not in k) for k, v in p.items()}


def close(a, b, what):
    np.testing.assert_allclose(a.detach().numpy(), b.detach().numpy(), rtol=1e-12, atol=1e-12, err_msg=what)


CASES = [("batchnorm", False), ("layernorm", False), ("none", False), ("none", True), ("layernorm", True)]


@pytest.mark.parametrize("normalization,training", CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_full_lengths_equal_the_reference_oracle(kind, normalization, training):
    p, x, gout, grate, init = make_params(kind, normalization, 11, bias=normalization != "batchnorm")
    pa, pb = leaves(p), leaves(p)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    spa, spb = [], []
    out_a, rates_a = bro.snn_forward(xa, [T] * B, pa, neuron_type=kind, num_layers=3, init_states=init,
                                     normalization=normalization, training=training, spikes_out=spa)
    out_b, rates_b = orc.snn_forward(xb, pb, neuron_type=kind, num_layers=3, init_states=init, bidirectional=True,
                                     normalization=normalization, training=training, spikes_out=spb)
    for a, b in zip(spa, spb):
        assert torch.equal(a, b)
    H0, H1 = SIZES[0], SIZES[1]
    for lo, hi in ((0, H0), (H0, 2 * H0), (2 * H0, 2 * H0 + H1), (2 * H0 + H1, 2 * H0 + 2 * H1)):
        assert float(rates_b.detach()[lo:hi].sum()) > 0  # (both directions of both layers spike)
    close(out_a, out_b, "out")
    close(rates_a, rates_b, "rates")
    ((out_a * gout).sum() + (rates_a * grate).sum()).backward()
    ((out_b * gout).sum() + (rates_b * grate).sum()).backward()
    close(xa.grad, xb.grad, "x")
    assert float(xa.grad.abs().max()) > 0
    for k in pa:
        if pa[k].requires_grad:
            close(pa[k].grad, pb[k].grad, k)


def test_full_lengths_in_train_mode_give_the_reference_batch_statistics():
    """BatchNorm in train mode, every length == T: the running statistics (the unbiased variance over 2 B T samples) and
    the outputs of the reference's batch-concatenated form."""
    p, x, gout, grate, init = make_params("adLIF", "batchnorm", 13)
    sa, sb = {}, {}
    out_a, rates_a = bro.snn_forward(x, [T] * B, p, neuron_type="adLIF", num_layers=3, init_states=init,
                                     normalization="batchnorm", training=True, stats=sa)
    out_b, rates_b = orc.snn_forward(x, p, neuron_type="adLIF", num_layers=3, init_states=init, bidirectional=True,
                                     normalization="batchnorm", training=True, stats=sb)
    close(out_a, out_b, "out")
    close(rates_a, rates_b, "rates")
    assert sa.keys() == sb.keys() and len(sa) == 6
    for k in sa:
        close(sa[k], sb[k], k)


@pytest.mark.parametrize("normalization,training", CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_each_row_is_its_clip_run_alone(kind, normalization, training):
    p, x, gout, grate, init = make_params(kind, normalization, 23, bias=normalization != "batchnorm")
    mask = rag.valid_mask(LENGTHS, T)
    x = x * mask[:, :, None]
    pa = leaves(p)
    xa = x.clone().requires_grad_(True)
    spa = []
    out_a, rates_a = bro.snn_forward(xa, LENGTHS, pa, neuron_type=kind, num_layers=3, init_states=init,
                                     normalization=normalization, training=training, spikes_out=spa)
    N = sum(LENGTHS)
    ((out_a * gout).sum() + (rates_a * grate).sum()).backward()
    pb = leaves(p)
    count = torch.zeros_like(rates_a)
    for b, L in enumerate(LENGTHS):
        xb = x[b:b + 1, :L].clone().requires_grad_(True)
        spb = []
        out_b, rates_b = orc.snn_forward(xb, pb, neuron_type=kind, num_layers=3, init_states=bro.rows_of(init, b, B),
                                         bidirectional=True, normalization=normalization, training=training,
                                         spikes_out=spb)
        for a, s in zip(spa, spb):
            assert torch.equal(a[b:b + 1, :L], s)
            assert not a[b, L:].any()
        close(out_a[b:b + 1], out_b, f"out[{b}]")
        count = count + rates_b.detach() * L
        # the rate of the ragged batch is sum_b L_b rate_b / N: the same weights on the gradient
        ((out_b * gout[b:b + 1]).sum() + (rates_b * grate).sum() * (L / N)).backward()
        close(xa.grad[b:b + 1, :L], xb.grad, f"x[{b}]")
        assert not xa.grad[b, L:].any()
    H0 = SIZES[0]
    assert float(count[:H0].sum()) > 0 and float(count[H0:2 * H0].sum()) > 0 and float(count[2 * H0:].sum()) > 0
    close(rates_a, count / N, "rates")
    for k in pa:
        if pa[k].requires_grad:
            close(pa[k].grad, pb[k].grad, k)


def test_flip_in_length():
    x = torch.arange(2 * 4 * 3, dtype=F64).reshape(2, 4, 3) + 1
    y = bro.flip_in_length(x, [4, 2])
    assert torch.equal(y[0], x[0].flip(0))
    assert torch.equal(y[1, :2], x[1, :2].flip(0)) and not y[1, 2:].any()
    assert torch.equal(bro.flip_in_length(y, [4, 2]), x * rag.valid_mask([4, 2], 4)[:, :, None])


# ------------------------------------------------------------------------------------------------ the GPU tests' data seed
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("normalization", bc.NORMS)
@pytest.mark.parametrize("kind", bc.KINDS)
def test_the_data_seed_keeps_its_margin(kind, normalization, training):
    """The condition of the count equality in tests/test_bidir_ragged_gpu.py, recomputed for every one of its 24 cases:
    the oracle's fp32 and fp64 runs agree on every spike, and every valid u - theta is MARGIN_RATIO times further from 0
    than its own fp32-versus-fp64 difference (tests/bidir_cases.py says why the margin is relative)."""
    import sparch_amd
    net = bc.make_net(sparch_amd, kind, normalization)
    params = {k: v.clone() for k, v in net.state_dict().items()}
    x, y, init = bc.net_inputs(kind)
    *_, s32, d32 = bc.oracle_step(kind, normalization, training, params, x, y, init)
    *_, s64, d64 = bc.oracle_step(kind, normalization, training, params, x, y, init, torch.float64)
    assert all(torch.equal(a.double(), b) for a, b in zip(s32, s64))
    ratio = float((d64.abs() / (d32.double() - d64).abs().clamp_min(1e-300)).min())
    print(f"  smallest |u - theta| {float(d64.abs().min()):.3e}, smallest ratio to its fp32 error {ratio:.1f}")
    assert ratio >= bc.MARGIN_RATIO, ratio
