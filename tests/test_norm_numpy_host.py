"""
Host tests of tests/norm_numpy.py (no GPU needed): each fp64 restatement of a G2 kernel against torch fp64 on the
CPU — torch.native_batch_norm / batch_norm, layer_norm, autograd for the backward formulas, torch.clamp's backward
for the gate — at rtol 1e-12.  Sums whose terms cancel (a gradient, a normalised value near 0) are held to 1e-12 of
the largest element of the array instead of their own size: an fp64 sum is not better than that in either library.
The GPU tests (tests/test_norm_kernels_gpu.py) then lean on a reference that has been checked here.
"""
import numpy as np
import pytest
import torch

from tests import norm_numpy as nn_

RTOL = 1e-12


def close(got, ref, what="", scale=0.0):
    """scale: the size of the terms where the whole array is a difference that cancels (dx of a one-column row)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=RTOL * max(float(np.abs(ref).max()), scale), err_msg=what)


def _bn_case(M, H, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, H, generator=g, dtype=torch.float64) * (torch.rand(H, generator=g, dtype=torch.float64) + 0.5) \
        + torch.randn(H, generator=g, dtype=torch.float64)
    gamma = torch.rand(H, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(H, generator=g, dtype=torch.float64)
    rm = torch.randn(H, generator=g, dtype=torch.float64)
    rv = torch.rand(H, generator=g, dtype=torch.float64) + 0.5
    return x, gamma, beta, rm, rv


@pytest.mark.parametrize("M,H", [(2, 1), (37, 5), (300, 17), (1000, 33)])
@pytest.mark.parametrize("dup", [1, 2])
def test_bn_finalize_from_partials_is_torch_batch_norm(M, H, dup):
    """dup = 2: every row seen twice (a bidirectional layer) — the batch of 2M rows torch gets is [x; x]."""
    x, gamma, beta, rm, rv = _bn_case(M, H, 100 * M + H)
    s, ss = nn_.tile_partials(x.numpy())
    assert s.shape == ((M + 127) // 128, H)
    r = nn_.bn_finalize(s, ss, M, dup, gamma.numpy(), beta.numpy(), rm.numpy(), rv.numpy())
    xx = torch.cat([x] * dup)
    trm, trv = rm.clone(), rv.clone()
    y, save_mean, save_invstd = torch.native_batch_norm(xx, gamma, beta, trm, trv, True, nn_.BN_MOMENTUM, nn_.NORM_EPS)
    close(r["mean"], save_mean.numpy(), "mean")
    close(r["invstd"], save_invstd.numpy(), "invstd")
    close(r["var"], xx.var(0, unbiased=False).numpy(), "biased var")
    close(r["unbiased"], xx.var(0, unbiased=True).numpy(), "unbiased var, n = dup * M")
    close(r["running_mean"], trm.numpy(), "running_mean")
    close(r["running_var"], trv.numpy(), "running_var")
    close(x.numpy() * r["scale"] + r["shift"], y[:M].numpy(), "x * scale + shift")
    y2 = torch.nn.functional.batch_norm(xx, rm.clone(), rv.clone(), gamma, beta, True, nn_.BN_MOMENTUM, nn_.NORM_EPS)
    close(x.numpy() * r["scale"] + r["shift"], y2[:M].numpy(), "functional.batch_norm")


def test_bn_finalize_clamps_a_negative_variance():
    r = nn_.bn_finalize([[2.0]], [[3.9]], 1, 2, [1.0], [0.0], [0.0], [1.0])   # ss/M - mu^2 = 3.9 - 4
    assert r["var"][0] == 0.0 and r["unbiased"][0] == 0.0
    assert r["invstd"][0] == 1.0 / np.sqrt(nn_.NORM_EPS)


def test_bn_eval_is_torch_batch_norm_in_eval_mode():
    x, gamma, beta, rm, rv = _bn_case(41, 9, 3)
    r = nn_.bn_eval(gamma.numpy(), beta.numpy(), rm.numpy(), rv.numpy())
    trm, trv = rm.clone(), rv.clone()
    y = torch.nn.functional.batch_norm(x, trm, trv, gamma, beta, False, nn_.BN_MOMENTUM, nn_.NORM_EPS)
    assert torch.equal(trm, rm) and torch.equal(trv, rv)
    close(x.numpy() * r["scale"] + r["shift"], y.numpy())
    close(r["invstd"], (1.0 / torch.sqrt(rv + nn_.NORM_EPS)).numpy())


@pytest.mark.parametrize("M,H", [(2, 3), (5, 1), (300, 17)])
def test_bn_backward_is_autograd_of_batch_norm(M, H):
    x, gamma, beta, rm, rv = _bn_case(M, H, 7 * M + H)
    g = torch.Generator().manual_seed(M)
    dy = torch.randn(x.shape, generator=g, dtype=torch.float64)
    xa, ga, ba = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = torch.nn.functional.batch_norm(xa, None, None, ga, ba, True, nn_.BN_MOMENTUM, nn_.NORM_EPS)
    (y * dy).sum().backward()
    mean = x.mean(0).numpy()
    invstd = (1.0 / torch.sqrt(x.var(0, unbiased=False) + nn_.NORM_EPS)).numpy()
    dgamma, dbeta = nn_.bn_bwd_reduce(dy.numpy(), x.numpy(), mean, invstd)
    close(dgamma, ga.grad.numpy(), "dgamma")
    close(dbeta, ba.grad.numpy(), "dbeta")
    close(nn_.bn_bwd_apply(dy.numpy(), x.numpy(), mean, invstd, gamma.numpy(), dgamma, dbeta), xa.grad.numpy(), "dx")
    t1, t0 = nn_.bn_bwd_terms(dy.numpy(), x.numpy(), mean, invstd)
    assert (t1 >= np.abs(dgamma) - 1e-9).all() and (t0 >= np.abs(dbeta) - 1e-9).all()
    # eval mode (fixed statistics): the batch-coupling terms vanish, which the library states as dgamma = dbeta = 0
    xe = x.clone().requires_grad_(True)
    ye = torch.nn.functional.batch_norm(xe, rm.clone(), rv.clone(), gamma, beta, False, nn_.BN_MOMENTUM, nn_.NORM_EPS)
    (ye * dy).sum().backward()
    inv_e = (1.0 / torch.sqrt(rv + nn_.NORM_EPS)).numpy()
    zero = np.zeros(H)
    close(nn_.bn_bwd_apply(dy.numpy(), x.numpy(), rm.numpy(), inv_e, gamma.numpy(), zero, zero), xe.grad.numpy(), "eval dx")


LN_SHAPES = [(1, 1, 1), (3, 7, 7), (4, 64, 64), (5, 65, 65), (9, 8, 5), (6, 128, 100), (257, 264, 260)]


def _ln_case(M, H, Hn, seed):
    g = torch.Generator().manual_seed(seed)
    s = torch.exp(torch.randn(M, 1, generator=g, dtype=torch.float64))
    o = s * torch.tensor([0.0, 1.0, 10.0, 100.0, -100.0], dtype=torch.float64)[torch.arange(M) % 5].view(M, 1)
    x = torch.randn(M, H, generator=g, dtype=torch.float64) * s + o
    gamma = torch.rand(H, generator=g, dtype=torch.float64) + 0.5
    beta = torch.randn(H, generator=g, dtype=torch.float64)
    x[:, Hn:] = 0
    gamma[Hn:] = 0
    dy = torch.randn(M, H, generator=g, dtype=torch.float64)
    return x, gamma, beta, dy


@pytest.mark.parametrize("M,H,Hn", LN_SHAPES)
def test_layernorm_forward_and_backward_are_torch_layer_norm(M, H, Hn):
    x, gamma, beta, dy = _ln_case(M, H, Hn, 11 * M + H)
    xa = x[:, :Hn].clone().requires_grad_(True)
    ga, ba = gamma[:Hn].clone().requires_grad_(True), beta[:Hn].clone().requires_grad_(True)
    yt = torch.nn.functional.layer_norm(xa, (Hn,), ga, ba, nn_.NORM_EPS)
    (yt * dy[:, :Hn]).sum().backward()
    y, mu, rstd = nn_.layernorm_fwd(x.numpy(), gamma.numpy(), beta.numpy(), Hn)
    close(y[:, :Hn], yt.detach().numpy(), "y")
    assert not y[:, Hn:].any()
    close(mu, x[:, :Hn].mean(1).numpy(), "mu")
    close(rstd, (1.0 / torch.sqrt(x[:, :Hn].var(1, unbiased=False) + nn_.NORM_EPS)).numpy(), "rstd")
    dx, dgamma, dbeta = nn_.layernorm_bwd(dy.numpy(), x.numpy(), mu, rstd, gamma.numpy(), Hn)
    close(dx[:, :Hn], xa.grad.numpy(), "dx", scale=float((rstd[:, None] * np.abs(dy.numpy())).max()))
    assert not dx[:, Hn:].any()
    close(dgamma[:Hn], ga.grad.numpy(), "dgamma", scale=float(np.abs(dy.numpy()).sum(0).max()))   # (|xhat| ~ 1)
    close(dbeta[:Hn], ba.grad.numpy(), "dbeta")
    assert np.isfinite(dgamma).all() and np.isfinite(dbeta).all()
    t1, t0 = nn_.layernorm_bwd_terms(dy.numpy(), x.numpy(), mu, rstd)
    assert (t1 >= np.abs(dgamma) - 1e-9).all() and (t0 >= np.abs(dbeta) - 1e-9).all()


def test_layernorm_of_a_constant_row_is_beta():
    x = np.full((2, 6), 3.0)
    y, mu, rstd = nn_.layernorm_fwd(x, np.arange(1.0, 7.0), np.arange(6.0) / 4, 6)
    assert (y == np.arange(6.0) / 4).all() and (mu == 3.0).all() and (rstd == 1.0 / np.sqrt(nn_.NORM_EPS)).all()


@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-1.0, 1.0), (0.36787944, 0.96)])
def test_clamp_gate_is_torch_clamps_backward(lo, hi):
    raw = nn_.edge_values(lo, hi)
    lo, hi = float(np.float32(lo)), float(np.float32(hi))
    p = torch.from_numpy(raw.astype(np.float64)).requires_grad_(True)
    w = torch.arange(1.0, raw.size + 1.0, dtype=torch.float64)
    (torch.clamp(p, lo, hi) * w).sum().backward()
    gate = nn_.clamp_gate(raw, lo, hi)
    assert gate.tolist() == [1, 1, 1, 0, 0, 0, 1, 1]
    np.testing.assert_array_equal(gate * w.numpy(), p.grad.numpy())
    ws = np.stack([np.outer(np.ones(3), w.numpy()), np.outer(np.arange(3.0), w.numpy())])    # (2, 3, H)
    out = nn_.colsum_clamped(ws, [raw, None], [(lo, hi), (lo, hi)])
    np.testing.assert_array_equal(out[0], 3 * p.grad.numpy())
    np.testing.assert_array_equal(out[1], 3 * w.numpy())
    np.testing.assert_array_equal(nn_.colsum_clamped(ws, [raw, raw], None)[0], 3 * w.numpy())
    np.testing.assert_array_equal(nn_.colsum_clamped(ws, None, [(lo, hi)] * 2)[0], 3 * w.numpy())


def test_split3_planes_are_the_exact_truncation_split():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(5, 16, generator=g) * torch.exp(4 * torch.randn(5, 16, generator=g))).numpy()
    x[0, :3] = [0.0, -0.0, 1.0]
    p = nn_.split3_planes(x)
    assert p.dtype == np.uint16 and p.shape == (3, 5, 16)
    f = nn_.planes_to_f32(p)
    np.testing.assert_array_equal((f[0] + f[1]) + f[2], x)
    np.testing.assert_array_equal(p[0], (x.view(np.uint32) >> 16).astype(np.uint16))
