"""
Host tests of tests/head_numpy.py (no GPU needed).

1. Every fp64 reference against torch float64 on the CPU at rtol 1e-12: torch.optim.Adam(foreach=False) over several
   steps with and without weight decay, F.cross_entropy with autograd, torch.sigmoid / relu / tanh with autograd, the
   `y += softmax(x_t)` loop with autograd.  Results that are differences which cancel (a gradient row that sums to
   zero) are held to 1e-12 of the largest element instead of their own size.
2. The fp32 restatements on EVERY input set tests/test_head_kernels_gpu.py uses: each stays within a quarter of its
   bound (so the constants of head_numpy cannot be loose: they are four times the restatement's worst ratio, and the
   other three quarters are the device's margin), and the input sets hold what the GPU tests rely on.
"""
import numpy as np
import pytest
import torch

from tests import head_numpy as hn
from tests.dropout_numpy import keep_mask

RTOL = 1e-12


def close(got, ref, what="", scale=0.0):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=RTOL * max(float(np.abs(ref).max()), scale), err_msg=what)


def quarter(got, ref, bound, what, floor=hn.TINY):
    """|restatement - reference| <= a quarter of the bound's rounding part c u mag, everywhere; `floor`, the part of
    the bound that stands for fp32's underflow, is no rounding error and is not quartered."""
    err = np.maximum(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) - floor, 0.0)
    bound = np.broadcast_to(np.asarray(bound, np.float64) - floor, err.shape)
    bad = err > 0.25 * bound
    assert not bad.any(), f"{what}: {float((err[bad] / bound[bad]).max())} of the bound"


# ====================================================================================================== 1. torch fp64
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("eps", [1e-8, 1e-3])
def test_adam_reference_is_torch_adam_in_float64(weight_decay, eps):
    lr, betas, n = 1e-2, (0.9, 0.999), 600
    p0, _, _, _ = hn.adam_inputs(n, 1, weight_decay, 5)
    pt = torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, foreach=False)
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t in range(1, 8):
        _, g, _, _ = hn.adam_inputs(n, 2, weight_decay, 100 + t)
        g = g.astype(np.float64) * (10.0 ** (t - 4))
        if t == 4:
            lr *= 0.7
            opt.param_groups[0]["lr"] = lr
        _, step_size, bc2_sqrt = hn.adam_scalars_ref(t - 1, lr, *betas)
        s = dict(step_size=step_size, bc2_sqrt=bc2_sqrt, beta1=betas[0], beta2=betas[1], w1=1.0 - betas[0],
                 w2=1.0 - betas[1], eps=eps, weight_decay=weight_decay)
        p, m, v = hn.adam_step_ref(p, g, m, v, s)
        pt.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[pt]
        assert float(st["step"]) == t
        close(p, pt.detach().numpy(), f"p after step {t}")
        close(m, st["exp_avg"].numpy(), f"m after step {t}")
        close(v, st["exp_avg_sq"].numpy(), f"v after step {t}")


def test_adam_scalars_reference():
    for t in (0, 1, 999, 99999):
        t1, step_size, bc2_sqrt = hn.adam_scalars_ref(t, 7e-3, 0.9, 0.999)
        assert t1 == t + 1
        assert step_size == 7e-3 / (1.0 - 0.9 ** (t + 1)) and bc2_sqrt == (1.0 - 0.999 ** (t + 1)) ** 0.5
    s = hn.adam_scalars32(1)
    assert s["step_size"] == np.float32(1e-2 / (1 - 0.9)) and s["w1"] == np.float32(1.0) - np.float32(0.9)
    assert all(isinstance(x, np.float32) for x in s.values())


@pytest.mark.parametrize("B,C", [(1, 1), (1, 2), (255, 7), (64, 1000)])
@pytest.mark.parametrize("family", hn.CE_FAMILIES)
def test_cross_entropy_reference_is_torch_cross_entropy(B, C, family):
    y = hn.ce_labels(B, C, 1)[-1]
    x = hn.ce_logits(B, C, family, y, 2)
    r = hn.ce_ref(x, y)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    rows = torch.nn.functional.cross_entropy(xt, torch.from_numpy(y), reduction="none")
    # the reference's divisor is fp32(1 / B), the kernel's: undo it for torch's exact mean
    loss = rows.sum() * r["inv_b"]
    loss.backward()
    close(r["rows"], rows.detach().numpy(), "rows", scale=float(np.abs(x).max()))
    close(r["loss"], float(loss.detach()), "loss", scale=float(np.abs(x).max()))
    close(r["dlogits"], xt.grad.numpy(), "dlogits", scale=r["inv_b"])
    np.testing.assert_allclose(float(loss.detach()), float(torch.nn.functional.cross_entropy(xt, torch.from_numpy(y)).detach()), rtol=1e-7)


def test_cross_entropy_reference_ignores_a_label_out_of_range():
    """The contract of include/sparch_hip.h: such a row adds nothing, its gradient row is zero, the divisor stays B —
    torch's ignore_index gives the same numerators and divides by the rows it counted."""
    B, C = 9, 5
    y = hn.ce_labels(B, C, 3)[0]
    x = hn.ce_logits(B, C, "randn3", y, 4)
    bad = y.copy()
    bad[2], bad[5] = -100, C
    r, good = hn.ce_ref(x, bad), hn.ce_ref(x, y)
    keep = np.ones(B, bool)
    keep[[2, 5]] = False
    assert not r["dlogits"][~keep].any() and not r["rows"][~keep].any()
    assert (r["dlogits"][keep] == good["dlogits"][keep]).all() and (r["rows"][keep] == good["rows"][keep]).all()
    np.testing.assert_allclose(r["loss"], good["rows"][keep].sum() * good["inv_b"], rtol=1e-13)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    yt = torch.from_numpy(np.where(keep, y, -100))
    lt = torch.nn.functional.cross_entropy(xt, yt, ignore_index=-100)
    lt.backward()
    scale = keep.sum() * r["inv_b"]                          # (rows counted) / B
    close(r["loss"], float(lt.detach()) * scale, "loss")
    close(r["dlogits"], xt.grad.numpy() * scale, "dlogits")
    b = hn.ce_bound(x, bad)
    assert not b["dlogits"][~keep].any()                     # zero rows are exact


@pytest.mark.parametrize("kind", list(hn.ACT_KINDS))
@pytest.mark.parametrize("family", hn.ACT_FAMILIES)
@pytest.mark.parametrize("affine", [True, False])
def test_activation_reference_is_torch_autograd(kind, family, affine):
    M, H = 37, 52
    z, sc, sh, dy = hn.act_inputs(M, H, family, affine, 6)
    mask = keep_mask(99, (M, H), 0.25)
    f = {"sigmoid": torch.sigmoid, "relu": torch.relu, "tanh": torch.tanh}[kind]
    zt = torch.from_numpy(z.astype(np.float64))
    v = zt if not affine else zt * torch.from_numpy(sc.astype(np.float64)) + torch.from_numpy(sh.astype(np.float64))
    v = v.clone().requires_grad_(True)
    k = torch.from_numpy(mask.astype(np.float64))
    yt = f(v) * k
    yt.backward(torch.from_numpy(dy.astype(np.float64)))
    y, dz = hn.act_ref(kind, z, sc, sh, dy, mask)
    close(y, yt.detach().numpy(), "y")
    # 1 - a: relative to 1 where the activation is saturated (fp64 rounds a, then subtracts, in both libraries)
    close(dz, v.grad.numpy(), "dz", scale=1e-3 * float(np.abs(dy).max()) if kind != "relu" else 0.0)
    y0, dz0 = hn.act_ref(kind, z, sc, sh, dy, None)
    assert (y == y0 * mask).all() and (dz == (dy.astype(np.float64) * mask) * hn._dact64(kind, hn._act64(kind, hn.act_preact_ref(z, sc, sh)))).all()
    if family == "saturated":
        a = hn._act64(kind, hn.act_preact_ref(z, sc, sh))
        assert np.isfinite(a).all() and (np.abs(hn.act_preact_ref(z, sc, sh)) >= 19.9).all()
    if family == "zeros":
        v32 = z if not affine else (z.astype(np.float64) * sc + sh).astype(np.float32)
        assert (v32 == 0).sum() >= 100 and np.signbit(v32[v32 == 0]).any() == (not affine)


def test_activation_reference_propagates_nan_as_torch_does():
    z = np.array([[np.nan, np.inf, -np.inf, 1.0]], dtype=np.float32)
    dy = np.ones((1, 4), dtype=np.float32)
    for kind, f in (("sigmoid", torch.sigmoid), ("relu", torch.relu), ("tanh", torch.tanh)):
        v = torch.from_numpy(z.copy()).requires_grad_(True)
        out = f(v)
        out.backward(torch.from_numpy(dy))
        with np.errstate(invalid="ignore"):
            y, _ = hn.act_ref(kind, z, None, None, dy)
            y32, _ = hn.act_f32(kind, z, None, None, dy)
        assert (np.isnan(y) == np.isnan(out.detach().numpy())).all(), kind
        assert (np.isnan(y32) == np.isnan(out.detach().numpy())).all(), kind
        assert np.isnan(y[0, 0])


@pytest.mark.parametrize("B,T,K", [(1, 1, 4), (3, 17, 48), (2, 5, 1028)])
@pytest.mark.parametrize("family", hn.SS_FAMILIES)
def test_softmax_sum_reference_is_the_torch_loop(B, T, K, family):
    x, g = hn.ss_inputs(B, T, K, family, 8)
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    out = 0
    for t in range(T):
        out = out + torch.softmax(xt[:, t, :], dim=-1)
    out.backward(torch.from_numpy(g.astype(np.float64)))
    ro, rdx = hn.ss_ref(x, g)
    close(ro, out.detach().numpy(), "out")
    close(rdx, xt.grad.numpy(), "dx", scale=float(np.abs(g).max()))


# ============================================================================== 2. restatements, bounds, input sets
@pytest.mark.parametrize("t,weight_decay,eps", list(hn.adam_cases()))
def test_adam_restatement_within_a_quarter_of_the_bound(t, weight_decay, eps):
    (p, g, m, v), tensors = hn.adam_table(t, weight_decay)
    assert [a.size for a in tensors[0]] == list(hn.ADAM_SIZES)
    s = hn.adam_scalars32(t, eps=eps, weight_decay=weight_decay)
    for name, a, b, bd in zip("pmv", hn.adam_step_f32(p, g, m, v, s), hn.adam_step_ref(p, g, m, v, s),
                              hn.adam_bound(p, g, m, v, s)):
        quarter(a, b, bd, f"Adam {name}' at t={t} wd={weight_decay} eps={eps}")
    # what the GPU test relies on
    assert (v == 0).any() and (g == 0).any() and ((np.abs(g) < eps) & (g != 0)).any()
    scales = np.asarray(hn.ADAM_GRAD_SCALES)[np.arange(g.size) % 5]
    for sc in hn.ADAM_GRAD_SCALES:
        gs = np.abs(g[(scales == sc) & (np.arange(g.size) % 7 != 3)])
        assert np.median(gs) > 0.1 * sc and np.median(gs) < 10 * sc
    assert ((m == 0).all() and (v == 0).all()) == (t == 1)
    if weight_decay:
        g1 = g.astype(np.float64) + p.astype(np.float64) * float(s["weight_decay"])
        few_bits = np.abs(g1) < 2.0 ** -16 * np.abs(g)
        assert few_bits.sum() >= 1000 and (g1[few_bits] != 0).all()


def test_cross_entropy_restatement_within_a_quarter_of_the_bound():
    seen = set()
    for B, C, fam, x, y in hn.ce_cases():
        r, f, b = hn.ce_ref(x, y), hn.ce_f32(x, y), hn.ce_bound(x, y)
        what = f"ce ({B},{C}) {fam}"
        quarter(f["rows"], r["rows"], b["rows"], what + " rows")
        quarter(f["loss"], r["loss"], b["loss"], what + " loss")
        quarter(f["dlogits"], r["dlogits"], b["dlogits"], what + " dlogits")
        assert r["ok"].all()
        seen.add((B, C, fam))
        labels = set(np.concatenate(hn.ce_labels(B, C, 100 * B + C)).tolist())
        assert 0 in labels and C - 1 in labels
        if fam == "randn100" and C >= 35:
            assert (np.exp(x.astype(np.float32) - x.max(1, keepdims=True)) == 0).mean() > 0.5     # most underflow
    assert len(seen) == len(hn.CE_SHAPES) * len(hn.CE_FAMILIES)


@pytest.mark.parametrize("kind", list(hn.ACT_KINDS))
def test_activation_restatement_within_a_quarter_of_the_bound(kind):
    n = 0
    for k, M, H, fam, affine, z, sc, sh, dy in hn.act_cases():
        if k != kind:
            continue
        for p_drop, seed in (hn.ACT_DROPS if M * H < (1 << 20) else hn.ACT_DROPS[1:2]):
            mask = keep_mask(seed, (M, H), p_drop) if p_drop else None
            (y, dz), (ry, rdz) = hn.act_f32(kind, z, sc, sh, dy, mask), hn.act_ref(kind, z, sc, sh, dy, mask)
            by, bdz = hn.act_bound(kind, z, sc, sh, dy, mask)
            what = f"{kind} ({M},{H}) {fam} affine={affine} p={p_drop}"
            fy, fdz = hn.act_floor(dy, mask)
            quarter(y, ry, by, what + " y", fy)
            quarter(dz, rdz, bdz, what + " dz", fdz)
            if mask is not None and M * H >= 1000:
                r0 = hn.act_f32(kind, z, sc, sh, dy, None)[0]           # the undropped forward value, in fp32
                assert ((mask != 0) & (r0 != 0)).sum() >= 100 and ((mask == 0) & (r0 != 0)).sum() >= 100, what
            n += 1
    assert n >= 3 * 3 * 2 * 3 + 2


def test_softmax_sum_restatement_within_a_quarter_of_the_bound():
    for B, T, K, fam, x, g in hn.ss_cases():
        (o, dx), (ro, rdx), (bo, bdx) = hn.ss_f32(x, g), hn.ss_ref(x, g), hn.ss_bound(x, g)
        quarter(o, ro, bo, f"softmax_sum ({B},{T},{K}) {fam} out")
        quarter(dx, rdx, bdx, f"softmax_sum ({B},{T},{K}) {fam} dx")
        # the sums the GPU test checks hold for the reference itself
        assert (np.abs(ro.sum(1) - T) <= bo.sum(1)).all() and (np.abs(rdx.sum(2)) <= bdx.sum(2)).all()


def test_adam_constants_are_four_times_the_restatements_worst_ratio():
    """The rule the constants follow, spelled out for Adam's three: ceil(4 x the restatement's worst ratio) is the
    constant in force (`python -m tests.head_numpy` prints the ratios of every operation; the quarter tests above
    hold all of them from above)."""
    import math
    w = {}

    def put(k, val):
        w[k] = max(w.get(k, 0.0), val)
    for t, wd, eps in hn.adam_cases():
        (p, g, m, v), _ = hn.adam_table(t, wd)
        s = hn.adam_scalars32(t, eps=eps, weight_decay=wd)
        for name, a, b, mag in zip(("P", "M", "V"), hn.adam_step_f32(p, g, m, v, s), hn.adam_step_ref(p, g, m, v, s),
                                   hn.adam_mags(p, g, m, v, s)):
            put(name, hn.worst(a, b, mag))
    assert (math.ceil(4 * w["P"]), math.ceil(4 * w["M"]), math.ceil(4 * w["V"])) == (hn.C_ADAM_P, hn.C_ADAM_M, hn.C_ADAM_V)
