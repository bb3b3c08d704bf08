"""
GPU tests of the two inputs of the hand-written backward kernels that no other test compares with a reference:
the dropout mask a backward REGENERATES from (seed, output element index), and the gradient through the firing
rates (`g_rate`).  Reference: the CPU oracle's autograd (oracle/snn_oracle.py, pinned to the reference by
tests/test_oracle_golden.py) with the mask restated in numpy (tests/dropout_numpy.py) applied as a constant.

How dropout parity is established: the mask is a pure function of (seed, index), so the numpy restatement is
pinned to the kernels through what a forward shows — in every test here that uses it, the HIP output must equal
`raw * mask` EXACTLY (raw: the oracle's undropped output, or in the pinning tests the same kernel's own
p_drop = 0 output; dropout does not feed back into a cell).  A spike that did not fire still carries surrogate
gradient, so the mask at non-fired elements matters in the backward and shows in no forward output: that part is
held by the gradient comparisons with the oracle, which multiplies by the full mask.

Bars (none new): dyadic V makes raw spikes bit-equal, so spikes are compared exactly, `count` with
(s_out > 0).sum((0, 1)) exactly, rates to rtol 1e-5, dWx and every parameter gradient within 2e-4 of the
tensor's max-abs (tests/test_hip_parity.py, "Stated tolerances"), dV's diagonal exactly zero; bf16 saved states
and the bf16 operand mode keep the bars their own tests state (2e-2).  BatchNorm's column sums: derived bound,
see `_check_bn_sums`.  The g_rate identity (part 3) is bit-for-bit.
"""
import numpy as np
import pytest
import torch

from oracle import snn_oracle as orc
from tests import dropout_numpy as dn
from tests.kit import DEV, SEED, bf16_mode, relmax  # noqa: F401  (bf16_mode: a fixture)
from tests.kit import Fn as _Fn

pytestmark = pytest.mark.gpu

ADAPTIVE, RECURRENT = orc.ADAPTIVE, orc.RECURRENT


# ---------------------------------------------------------------------------------------------- helpers
def _case(kind, B, T, H, dirs, seed):
    """The `dyadic_cell_case` recipe of tests/spiking_cases.py (V on a 2^-6 grid, binary s0: every partial sum of
    s @ V is exact in fp32, so raw spikes cannot depend on summation order) for a layer with `dirs` directions:
    Wx (B,T,H), states (B*dirs,H), upstream gradients g_s (B,T,dirs*H) and g_r (dirs*H).  g_r has every unit
    non-zero and is O(B*T), so that the rate term g_r / (B*T) is as large as g_s and a wrong scale, offset or a
    missing dropout factor on it moves the gradients by O(1) of their size, not by 1 / (B*T)."""
    g = torch.Generator().manual_seed(seed)
    Bp, F = B * dirs, H * dirs
    V = torch.randint(-24, 25, (H, H), generator=g).float() / 64.0
    Wx = torch.randn(B, T, H, generator=g) * 1.5 + 0.4
    p = {"alpha": torch.rand(H, generator=g) * 0.2 + 0.78}
    if RECURRENT[kind]:
        p["V"] = V
    if ADAPTIVE[kind]:
        p.update(beta=torch.rand(H, generator=g) * 0.05 + 0.95, a=torch.rand(H, generator=g) * 2.4 - 1.2,
                 b=torch.rand(H, generator=g) * 2.4 - 0.2)
    u0 = torch.rand(Bp, H, generator=g)
    w0 = torch.rand(Bp, H, generator=g) if ADAPTIVE[kind] else None
    s0 = (torch.rand(Bp, H, generator=g) < 0.3).float()
    g_s = torch.randn(B, T, F, generator=g)
    sign = (torch.rand(F, generator=g) < 0.5).float() * 2 - 1
    g_r = sign * (torch.rand(F, generator=g) * 0.5 + 0.25) * float(B * T)
    return dict(kind=kind, B=B, T=T, H=H, dirs=dirs, Wx=Wx, p=p, u0=u0, w0=w0, s0=s0, g_s=g_s, g_r=g_r)


def _mask(c, p_drop, seed):
    """The kernels' mask for this case as a CPU tensor (ones without dropout).  The element index is the one of the
    tensor the kernel writes: a recurrent cell whose width is not a multiple of 4 runs zero-padded to the next one
    (functional.cell_forward), so its mask is the padded tensor's, sliced."""
    B, T, H, dirs = c["B"], c["T"], c["H"], c["dirs"]
    if p_drop == 0.0:
        return torch.ones(B, T, dirs * H)
    Hp = (H + 3) // 4 * 4 if RECURRENT[c["kind"]] else H
    return torch.from_numpy(dn.keep_mask_padded(seed, B, T, dirs, H, Hp, p_drop))


def _glue(s, dirs):
    """snns.py:272-275: un-flip the second direction's rows and stack them on the features."""
    if dirs == 1:
        return s
    s_f, s_b = s.chunk(2, dim=0)
    return torch.cat([s_f, s_b.flip(1)], dim=2)


def _oracle(c, mask):
    """Oracle forward with the explicit flip / cat glue, constant mask, and autograd through
    loss = (s * g_s).sum() + (rate * g_r).sum().  Returns raw spikes, dropped spikes, rate, dWx (both directions'
    halves added: they share the projection rows) and the parameter gradients."""
    kind, dirs = c["kind"], c["dirs"]
    Wx = c["Wx"].clone().requires_grad_(True)
    p = {k: v.clone().requires_grad_(True) for k, v in c["p"].items()}
    Wcat = torch.cat([Wx, Wx.flip(1)], dim=0) if dirs == 2 else Wx
    raw = _glue(orc.spiking_cell(kind, Wcat, p, c["u0"], c["w0"], c["s0"]), dirs)
    s_ref = raw * mask
    rate = s_ref.mean(dim=(0, 1))
    loss = (s_ref * c["g_s"]).sum() + (rate * c["g_r"]).sum()
    loss.backward()
    assert float(raw.detach().sum()) > 0
    assert bool(torch.isfinite(Wx.grad).all()), "oracle dWx not finite"
    for k, v in p.items():
        assert bool(torch.isfinite(v.grad).all()), ("oracle gradient not finite", k)
    return raw.detach(), s_ref.detach(), rate.detach(), Wx.grad, {k: v.grad for k, v in p.items()}


def _hip(c, p_drop, seed, spl=None, bn=None, use_rate=True, backward=True, g_s=None):
    """functional.cell_forward / cell_backward on the case.  Returns a dict of CPU tensors."""
    Fn = _Fn()
    kind, B, T, H, dirs = c["kind"], c["B"], c["T"], c["H"], c["dirs"]
    pd = {k: v.to(DEV) for k, v in c["p"].items()}
    Wxd, u0, s0 = c["Wx"].to(DEV), c["u0"].to(DEV), c["s0"].to(DEV)
    w0 = None if c["w0"] is None else c["w0"].to(DEV)
    s_out, count, saved, s16 = Fn.cell_forward(kind, Wxd, None, None, pd, u0, w0, s0, B=B, dirs=dirs, theta=1.0,
                                               p_drop=p_drop, seed=seed, steps_per_launch=spl)
    Fn.check_status()
    r = {"s": s_out.cpu(), "count": count.cpu(), "s16": None if s16 is None else s16.float().cpu()}
    if backward:
        bn_d = None if bn is None else tuple(t.to(DEV) for t in bn)
        g_out = (c["g_s"] if g_s is None else g_s).to(DEV)
        dWx, pg = Fn.cell_backward(kind, g_out, c["g_r"].to(DEV) if use_rate else None, pd, u0, w0, s0, saved,
                                   B=B, dirs=dirs, T=T, H=H, theta=1.0, p_drop=p_drop, seed=seed,
                                   steps_per_launch=spl, bn=bn_d)
        Fn.check_status()
        r["dWx_rows"] = dWx.cpu()
        r["dWx"] = (dWx[:B] + dWx[B:]).cpu() if dirs == 2 else dWx.cpu()
        r["bn_sums"] = tuple(t.cpu() for t in pg.pop("bn_sums")) if "bn_sums" in pg else None
        r["grads"] = {k: v.cpu() for k, v in pg.items()}
    return r


def _check_forward(c, r, s_ref, rate_ref, p_drop, tag):
    """HIP output == raw * mask at every element (so in particular wherever the undropped output is non-zero: the
    numpy mask is pinned there; and nothing fires where the oracle is silent), bf16 plane, count, rate."""
    assert tuple(r["s"].shape) == tuple(s_ref.shape), tag
    assert torch.equal(r["s"], s_ref), (tag, float((r["s"] != s_ref).float().mean()))
    if r["s16"] is not None:
        assert torch.equal(r["s16"], (r["s"] != 0).float()), tag
    np.testing.assert_array_equal(r["count"].numpy(), (r["s"] > 0).sum(dim=(0, 1)).numpy(), err_msg=str(tag))
    # the layer's rate (functional.SpikingLayerFn.forward): count * inv_keep / (B*T)
    rate = r["count"].float() * (float(dn.inv_keep(p_drop)) / float(c["B"] * c["T"]))
    np.testing.assert_allclose(rate.numpy(), rate_ref.numpy(), rtol=1e-5, atol=0, err_msg=str(tag))


def _check_grads(r, dwx_ref, g_ref, tag, tol=2e-4, tol_neuron=None):
    assert bool(torch.isfinite(r["dWx"]).all()), tag
    e = relmax(r["dWx"].numpy(), dwx_ref.numpy())
    assert e <= tol, (tag, "dWx", e)
    assert set(r["grads"]) == set(g_ref), tag
    for k in g_ref:
        assert tuple(r["grads"][k].shape) == tuple(g_ref[k].shape), (tag, k)
        e = relmax(r["grads"][k].numpy(), g_ref[k].numpy())
        assert e <= (tol if (k == "V" or tol_neuron is None) else tol_neuron), (tag, k, e)
    if "V" in g_ref:
        assert float(torch.diag(r["grads"]["V"]).abs().max()) == 0.0, tag


def _run_and_check(c, p_drop, spl=None, seed=SEED, tag=None):
    tag = tag or (c["kind"], c["B"], c["T"], c["H"], c["dirs"], p_drop, spl)
    mask = _mask(c, p_drop, seed)
    raw, s_ref, rate_ref, dwx_ref, g_ref = _oracle(c, mask)
    for L in (spl if isinstance(spl, (tuple, list)) else (spl,)):
        r = _hip(c, p_drop, seed, spl=L)
        _check_forward(c, r, s_ref, rate_ref, p_drop, (tag, L))
        _check_grads(r, dwx_ref, g_ref, (tag, L))
    return raw, mask


# ---------------------------------------------------------------- part 2: cell level against oracle autograd
@pytest.mark.parametrize("p_drop", [0.0, 0.25])
@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("kind,B,T,H", [("LIF", 5, 17, 64), ("adLIF", 5, 17, 64), ("LIF", 33, 9, 128),
                                        ("adLIF", 33, 9, 128)])
def test_scan_cells_backward_with_dropout_and_rate_gradient(kind, B, T, H, dirs, p_drop):
    """cell.hip (LIF / adLIF): forward mask, regenerated backward mask (flipped time for the second direction,
    d*H + h feature offset) and g_rate (indexed d*H + h, scaled 1/(B*T), times the dropout factor) against the
    oracle's autograd."""
    _run_and_check(_case(kind, B, T, H, dirs, 100 + B + H + dirs), p_drop)


@pytest.mark.parametrize("dirs", [1, 2])
def test_scan_cells_around_the_prefetch_ring_depths_with_dropout_and_rate_gradient(dirs):
    """The sequence lengths of test_scan_kernels_around_the_prefetch_ring_depths (both sides of every ring depth,
    the tail without refills, cell step 0 inside the tail; one and four neurons per thread) with p_drop = 0.25 and
    g_rate: the mask index of a step taken from a ring slot must be that step's."""
    bad = []
    # (17 rows where that test has 3: with 3 x 5 neurons some of these short sequences never fire in the oracle)
    cases = [(17, T, 5) for T in (6, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49)]
    cases += [(512 // dirs, T, 1024) for T in (7, 8, 9, 17)]
    for kind in ("adLIF", "LIF"):
        for B, T, H in cases:
            try:
                _run_and_check(_case(kind, B, T, H, dirs, 11 * T + B), 0.25)
            except AssertionError as e:  # collect: one report for the whole grid
                bad.append((kind, B, T, H, str(e)[:200]))
    assert not bad, bad[:6]


@pytest.mark.parametrize("p_drop", [0.0, 0.25])
@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("kind", ["RLIF", "RadLIF"])
@pytest.mark.parametrize("B,T,H", [(5, 33, 64), (40, 21, 132), (48, 40, 1024)])
def test_persistent_recurrent_cells_backward_with_dropout_and_rate_gradient(kind, B, T, H, dirs, p_drop):
    """reccell.hip, whole-sequence launch, chunks of 7 steps (the mask index after a chunk boundary) and one launch
    per step: every launch form against the same oracle run."""
    _run_and_check(_case(kind, B, T, H, dirs, 200 + B + H + dirs), p_drop, spl=(None, 7, 1))


@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("kind,H", [("RLIF", 66), ("RadLIF", 130), ("RadLIF", 7)])
def test_padded_width_backward_with_dropout_and_rate_gradient(kind, H, dirs):
    """Widths that run zero-padded to a multiple of 4 (shapes of test_recurrent_cell_any_hidden_size): the mask index
    is the padded tensor's, g_rate is padded per direction (`gr_p` in functional.cell_backward)."""
    _run_and_check(_case(kind, 9, 14, H, dirs, 40 + H + dirs), 0.25, spl=(None, 1))


@pytest.mark.parametrize("dirs", [1, 2])
def test_step_path_backward_with_dropout_and_rate_gradient(dirs):
    """H = 1028 > 1024: one launch per time step with the recurrent product between the steps
    (sparch_rec_cell_step_fwd / _bwd)."""
    _run_and_check(_case("RadLIF", 9, 14, 1028, dirs, 77 + dirs), 0.25)


def _check_bn_sums(c, r, bn, tag):
    """The BatchNorm column sums the cell backward folds in, against fp64 sums formed from the kernel's OWN dWx:
    dbeta[h] = sum dWx[b', t, h], dgamma[h] = sum dWx[b', t, h] * xhat[b, t, h] over both directions' rows (dWx is
    stored at the original time index, as bn_x is).  Derived bar: a row accumulates its T terms one after the
    other in fp32 (recursive summation: (T - 1) * 2^-24 * sum|term|), a term carries up to three roundings (x - mean,
    * invstd, * dWx), the rows then meet in fp64 and the result is cast once:
    |err| <= (T + 4) * 2^-24 * sum|term| per column, sum|term| formed in fp64 too."""
    B, T, dirs = c["B"], c["T"], c["dirs"]
    x, mean, invstd = (t.double() for t in bn)
    xhat = (x - mean) * invstd                                   # (B, T, H)
    d = r["dWx_rows"].double().view(dirs, B, T, -1)
    bound = (T + 4) * 2.0 ** -24
    dbeta, dgamma = (t.double() for t in r["bn_sums"])
    for got, terms, name in ((dbeta, d, "dbeta"), (dgamma, d * xhat, "dgamma")):
        ref, mag = terms.sum(dim=(0, 1, 2)), terms.abs().sum(dim=(0, 1, 2))
        assert float(mag.min()) > 0
        worst = float(((got - ref).abs() / mag).max())
        print(f"{tag} {name}: worst |err| / sum|term| = {worst:.2e} (bound {bound:.2e})")
        assert bool(((got - ref).abs() <= bound * mag).all()), (tag, name, worst, bound)


@pytest.mark.parametrize("kind,B,T,H", [("adLIF", 33, 9, 128), ("RadLIF", 40, 21, 132)])
def test_batchnorm_sums_folded_into_the_cell_backward(kind, B, T, H):
    """`bn=` of cell_backward with two directions, dropout and g_rate: gradients against the oracle as above, and the
    returned column sums against fp64 sums of the kernel's own dWx."""
    c = _case(kind, B, T, H, 2, 300 + H)
    mask = _mask(c, 0.25, SEED)
    raw, s_ref, rate_ref, dwx_ref, g_ref = _oracle(c, mask)
    flat = c["Wx"].reshape(B * T, H)
    mean = flat.mean(0)
    invstd = 1.0 / torch.sqrt(flat.var(0, unbiased=False) + 1e-5)
    bn = (c["Wx"], mean, invstd)
    r = _hip(c, 0.25, SEED, bn=bn)
    _check_forward(c, r, s_ref, rate_ref, 0.25, kind)
    _check_grads(r, dwx_ref, g_ref, kind)
    assert r["bn_sums"] is not None
    _check_bn_sums(c, r, bn, kind)


@pytest.mark.parametrize("kind,B,T,H,dirs", [("adLIF", 6, 40, 64, 2), ("RadLIF", 40, 50, 256, 2),
                                             ("RLIF", 5, 33, 64, 1)])  # (shapes of the test whose bars these are)
def test_bf16_saved_states_with_dropout_and_rate_gradient(kind, B, T, H, dirs, monkeypatch):
    """SPARCH_SAVE_DTYPE=bf16 with dropout and g_rate, bars of test_bf16_saved_states_keep_every_discrete_decision:
    against the fp32-saved run dWx and dV identical bit for bit and the neuron parameters within 2e-2 of max-abs;
    hence against the oracle dWx / dV at 2e-4 and the neuron parameters at 2e-2."""
    Fn = _Fn()
    c = _case(kind, B, T, H, dirs, 400 + H)
    mask = _mask(c, 0.25, SEED)
    raw, s_ref, rate_ref, dwx_ref, g_ref = _oracle(c, mask)
    r32 = _hip(c, 0.25, SEED)
    monkeypatch.setattr(Fn, "SAVE_BF16", True)
    r16 = _hip(c, 0.25, SEED)
    _check_forward(c, r16, s_ref, rate_ref, 0.25, kind)
    assert torch.equal(r16["dWx_rows"], r32["dWx_rows"])
    for k in g_ref:
        if k == "V":
            assert torch.equal(r16["grads"][k], r32["grads"][k])
        else:
            assert relmax(r16["grads"][k].numpy(), r32["grads"][k].numpy()) <= 2e-2, k
    _check_grads(r16, dwx_ref, g_ref, kind, tol=2e-4, tol_neuron=2e-2)


@pytest.mark.parametrize("kind,B,T,H,dirs,spl", [("RadLIF", 40, 21, 132, 2, None), ("RLIF", 5, 33, 64, 1, 1)])
def test_bf16_operand_mode_with_dropout_and_rate_gradient(kind, B, T, H, dirs, spl, bf16_mode):
    """The bf16 operand mode (dWx rounded to bf16 once per recurrent product; V is bf16-exact here, so the forward
    stays bit-exact): 2e-2 of max-abs, as test_bf16_operand_mode_recurrent_cell."""
    c = _case(kind, B, T, H, dirs, 500 + H)
    mask = _mask(c, 0.25, SEED)
    raw, s_ref, rate_ref, dwx_ref, g_ref = _oracle(c, mask)
    r = _hip(c, 0.25, SEED, spl=spl)
    _check_forward(c, r, s_ref, rate_ref, 0.25, kind)
    _check_grads(r, dwx_ref, g_ref, kind, tol=2e-2)


# ---------------------------------------------------------------- pinning the numpy mask to every forward family
@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("family,kind,B,T,H,spl", [
    ("scan", "LIF", 48, 40, 1024, None), ("scan", "adLIF", 48, 40, 1024, None),
    ("persistent whole-sequence", "RadLIF", 48, 40, 1024, None), ("persistent chunked", "RLIF", 48, 40, 1024, 7),
    ("persistent one launch per step", "RadLIF", 48, 40, 1024, 1), ("step path", "RadLIF", 9, 14, 1028, None),
    ("padded width", "RadLIF", 48, 40, 130, None)])
def test_numpy_mask_is_the_kernels_mask(family, kind, B, T, H, spl, dirs):
    """One test per forward family: raw = the same kernel's own p_drop = 0 output (dropout does not feed back into
    the cell, so the raw spikes are the same bits); with p_drop = 0.25 the output must be raw * mask at every
    element, where at least 1000 fired elements are kept and at least 1000 are dropped."""
    c = _case(kind, B, T, H, dirs, 600 + H + dirs)
    raw = _hip(c, 0.0, 0, spl=spl, backward=False)["s"]
    assert set(torch.unique(raw).tolist()) == {0.0, 1.0}
    for seed in (SEED, 3):
        got = _hip(c, 0.25, seed, spl=spl, backward=False)
        mask = _mask(c, 0.25, seed)
        fired = raw > 0
        kept, dropped = int((fired & (mask > 0)).sum()), int((fired & (mask == 0)).sum())
        assert kept >= 1000 and dropped >= 1000, (family, kept, dropped)
        assert torch.equal(got["s"][fired], (raw * mask)[fired]), family
        assert torch.equal(got["s"], raw * mask), family
        np.testing.assert_array_equal(got["count"].numpy(), (got["s"] > 0).sum(dim=(0, 1)).numpy())


# ---------------------------------------------------------------- part 3: an identity that needs no tolerance
def _device_case(kind, B, T, H, dirs, seed):
    """As `_case`, drawn on the device (no oracle runs at these sizes)."""
    g = torch.Generator(DEV).manual_seed(seed)
    kw = dict(generator=g, device=DEV)
    Bp, F = B * dirs, H * dirs
    p = {"alpha": torch.rand(H, **kw) * 0.2 + 0.78}
    if RECURRENT[kind]:
        p["V"] = torch.randint(-24, 25, (H, H), **kw).float() / 64.0
    if ADAPTIVE[kind]:
        p.update(beta=torch.rand(H, **kw) * 0.05 + 0.95, a=torch.rand(H, **kw) * 2.4 - 1.2,
                 b=torch.rand(H, **kw) * 2.4 - 0.2)
    sign = (torch.rand(F, **kw) < 0.5).float() * 2 - 1
    return dict(kind=kind, B=B, T=T, H=H, dirs=dirs, Wx=torch.randn(B, T, H, **kw) * 1.5 + 0.4, p=p,
                u0=torch.rand(Bp, H, **kw), w0=torch.rand(Bp, H, **kw) if ADAPTIVE[kind] else None,
                s0=(torch.rand(Bp, H, **kw) < 0.3).float(), g_s=torch.randn(B, T, F, **kw),
                g_r=sign * (torch.rand(F, **kw) * 0.5 + 0.25) * float(B * T))


@pytest.mark.parametrize("kind,B,dirs,T,H,spl,compute,save16", [
    ("RadLIF", 256, 1, 250, 1024, None, "fp32", False),   # the headline launch, Bp = 256
    ("RadLIF", 256, 2, 250, 1024, None, "fp32", False),   # Bp = 512: two directions
    ("RadLIF", 256, 2, 250, 1024, None, "bf16", False),   # ... in the bf16 operand mode
    ("RLIF", 256, 1, 250, 1024, None, "fp32", True),      # bf16 saved states
    ("RadLIF", 128, 2, 250, 1024, None, "bf16", True),
    ("RadLIF", 144, 2, 4, 1024, 2, "fp32", False),        # Bp = 288: several row-tile groups, chunked launches
    ("RLIF", 260, 2, 3, 1024, 1, "fp32", False),          # Bp = 520, one launch per step
    ("RadLIF", 35, 2, 6, 1000, 3, "fp32", False),
    ("RadLIF", 9, 2, 14, 1028, None, "fp32", False),      # step path
    ("RLIF", 9, 2, 14, 130, None, "fp32", False),         # padded width
    ("adLIF", 128, 2, 100, 512, None, "fp32", False),     # scan kernels, four neurons per thread
    ("adLIF", 128, 2, 100, 512, None, "fp32", True),
    ("LIF", 3, 2, 17, 5, None, "fp32", False)])           # one neuron per thread
def test_rate_gradient_equals_its_share_added_to_the_output_gradient(kind, B, dirs, T, H, spl, compute, save16,
                                                                     request, monkeypatch):
    """For fixed saved states the backward is a function of g_out + g_rate / (B*T) only.  The kernels form
    gr = g_rate[f] * (1.0f / ((float)B * (float)T)) and (g + gr) * k, and the library is built with
    -ffp-contract=off: cell_backward(g_out, g_rate) must equal cell_backward(g_out + g_rate * fp32(1/(B*T)), None)
    BIT FOR BIT in dWx and every parameter gradient (the torch side takes the same two fp32 roundings).  Run where
    the oracle is too slow to go; p_drop = 0.1.  A wrong scale (Bp for B), a wrong second-direction offset or a
    rate gradient that skips the dropout factor breaks the equality at almost every element."""
    Fn = _Fn()
    if compute == "bf16":
        request.getfixturevalue("bf16_mode")
    monkeypatch.setattr(Fn, "SAVE_BF16", save16)
    c = _device_case(kind, B, T, H, dirs, 700 + B + T)
    p_drop = 0.1
    s_out, count, saved, _ = Fn.cell_forward(kind, c["Wx"], None, None, c["p"], c["u0"], c["w0"], c["s0"], B=B,
                                             dirs=dirs, theta=1.0, p_drop=p_drop, seed=SEED, steps_per_launch=spl)
    Fn.check_status()
    assert int(count.sum()) > 0
    assert (saved[0].dtype == torch.bfloat16) == (save16 and spl is None and H % 4 == 0 and H <= 1024)
    kw = dict(B=B, dirs=dirs, T=T, H=H, theta=1.0, p_drop=p_drop, seed=SEED, steps_per_launch=spl)
    dwx_a, g_a = Fn.cell_backward(kind, c["g_s"], c["g_r"], c["p"], c["u0"], c["w0"], c["s0"], saved, **kw)
    Fn.check_status()
    scale = float(np.float32(1.0) / (np.float32(B) * np.float32(T)))  # an fp32 value, held exactly by the double
    g_sum = c["g_s"] + (c["g_r"] * scale).view(1, 1, -1)
    dwx_b, g_b = Fn.cell_backward(kind, g_sum, None, c["p"], c["u0"], c["w0"], c["s0"], saved, **kw)
    Fn.check_status()
    dwx_0, _ = Fn.cell_backward(kind, c["g_s"], None, c["p"], c["u0"], c["w0"], c["s0"], saved, **kw)
    Fn.check_status()
    assert bool(torch.isfinite(dwx_a).all())
    assert not torch.equal(dwx_a, dwx_0), "g_rate had no effect"
    assert torch.equal(dwx_a, dwx_b), float((dwx_a != dwx_b).float().mean())
    assert set(g_a) == set(g_b)
    for k in g_a:
        assert torch.equal(g_a[k], g_b[k]), (k, float((g_a[k] - g_b[k]).abs().max()))


# ---------------------------------------------------------------- part 6: the non-spiking baselines
@pytest.mark.parametrize("kind,bidir,norm,H,env", [
    ("MLP", False, "batchnorm", 64, {}),
    ("MLP", False, "layernorm", 30, {}),                                  # runs at the padded width 32
    ("RNN", True, "batchnorm", 64, {}),                                   # persistent dense recurrent kernel
    ("RNN", False, "none", 64, {"SPARCH_REC_STEP_PATH": "1"}),            # one launch per step
    ("RNN", True, "layernorm", 30, {}),
    ("LiGRU", False, "batchnorm", 64, {}),                                # persistent kernels (gatedcell.hip)
    ("LiGRU", True, "layernorm", 64, {"SPARCH_LIGRU_PERSISTENT": "0"}),   # launch per step (annstep.hip)
    ("GRU", True, "batchnorm", 64, {}),
    ("GRU", False, "none", 64, {"SPARCH_GRU_PERSISTENT": "0"}),
    ("GRU", True, "none", 64, {"SPARCH_REC_STEPS_PER_LAUNCH": "5"})])     # persistent kernels, chunked launches
def test_baseline_layers_with_dropout_vs_oracle(kind, bidir, norm, H, env, monkeypatch):
    """MLP / RNN / LiGRU / GRU layers with dropout = 0.3 against ann_oracle.hidden_layer(...) * mask (mask from
    tests/dropout_numpy.py, the layer's seed fixed), bars of test_gated_baseline_layers_vs_oracle: output 5e-5,
    gradients 2e-4 of each tensor's largest entry.  The output is non-zero almost everywhere, so the mask is pinned
    at every element: the zero pattern of the HIP output must be the mask's wherever the oracle's undropped output
    is not itself tiny.  Dropout acts on the layer's output only (the recurrent state stays undropped), and the
    backward regenerates the mask per element — flipped time for the second direction."""
    from oracle import ann_oracle as ao
    from sparch_amd import anns

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    B, T, C, p_drop = 10, 19, 36, 0.3
    dirs = 2 if bidir else 1
    torch.manual_seed(23)
    layer = getattr(anns, kind + "Layer")(C, H, B, dropout=p_drop, normalization=norm, use_bias=True, bidirectional=bidir)
    with torch.no_grad():
        for n in ("norm", "normz", "normr"):
            if hasattr(layer, n) and norm != "none":
                getattr(layer, n).weight.uniform_(0.7, 1.3)
                getattr(layer, n).bias.uniform_(-0.2, 0.2)
    g = torch.Generator().manual_seed(24)
    x = torch.randn(B, T, C, generator=g)
    gy = torch.randn(B, T, H * dirs, generator=g)
    p = {"ann.0." + k: v.detach().clone().requires_grad_(v.dtype.is_floating_point and "running" not in k)
         for k, v in layer.state_dict().items() if "num_batches" not in k}
    mask = torch.from_numpy(dn.keep_mask_padded(SEED, B, T, dirs, H, (H + 3) // 4 * 4, p_drop))
    xr = x.clone().requires_grad_(True)
    raw = ao.hidden_layer(kind, xr, p, "ann.0", norm, bidir, training=True, running=None)
    ref = raw * mask
    (ref * gy).sum().backward()
    layer = layer.to(DEV).train()
    monkeypatch.setattr(layer, "_dropout_seed", lambda device: SEED, raising=False)
    xd = x.to(DEV).requires_grad_(True)
    y = layer(xd)
    (y * gy.to(DEV)).sum().backward()
    _Fn().check_status()
    y_c = y.detach().cpu()
    clear = raw.detach().abs() > 1e-3 * float(raw.detach().abs().max())
    assert float(clear.float().mean()) > 0.5 and int((clear & (mask == 0)).sum()) >= 1000
    assert torch.equal((y_c != 0)[clear], (mask != 0)[clear]), "the kernel's mask is not the restated one"
    assert bool((y_c[mask == 0] == 0).all())
    assert relmax(y_c.numpy(), ref.detach().numpy()) <= 5e-5
    assert relmax(xd.grad.cpu().numpy(), xr.grad.numpy()) <= 2e-4
    wmax = float(layer.W.weight.grad.abs().max())
    for k, v in layer.named_parameters():
        r = p["ann.0." + k].grad.numpy()
        if k.endswith(".bias") and k[0] == "W" and norm != "none":  # removed by the normalisation: exactly zero in real arithmetic
            assert np.abs(v.grad.cpu().numpy() - r).max() <= 1e-4 * wmax, k
            continue
        assert relmax(v.grad.cpu().numpy(), r) <= 2e-4, k


# ---------------------------------------------------------------- part 4: whole networks, dropout 0.5 + regulariser
def _layer_seeds(n_hidden):
    return [SEED + 7919 * i for i in range(n_hidden)]


def _network_masks(cfg, seeds, p_drop):
    """One mask per hidden layer, at the width the layer's kernels run at (recurrent widths pad to multiples of 4)."""
    dirs = 2 if cfg["bidirectional"] else 1
    rec = RECURRENT[cfg["neuron_type"]]
    return [torch.from_numpy(dn.keep_mask_padded(seed, cfg["B"], cfg["T"], dirs, H, (H + 3) // 4 * 4 if rec else H, p_drop))
            for seed, H in zip(seeds, cfg["layer_sizes"][:-1])]


def _split_threshold(rates, n):
    """fmin = fmax = the midpoint between two adjacent distinct values of the ORACLE's rates whose share of units
    above it is closest to 1/4: both hinge branches of the regulariser are then live.  Asserted on the oracle alone:
    >= 20 % of the units above, >= 20 % below, no unit closer to the threshold than 1 / (4 * n), n = B*T (HIP and
    oracle rates differ by fp32 rounding only, adjacent rate values by at least 1 / n)."""
    r = rates.detach().double().numpy()
    vals = np.unique(r)
    mids = (vals[:-1] + vals[1:]) / 2
    share = np.array([(r > m).mean() for m in mids])
    thr = float(mids[int(np.argmin(np.abs(share - 0.25)))])
    above, below, nearest = float((r > thr).mean()), float((r < thr).mean()), float(np.abs(r - thr).min())
    assert above >= 0.2 and below >= 0.2, (above, below)
    assert nearest >= 1.0 / (4 * n), (nearest, 1.0 / (4 * n))
    return thr


def _network_oracle(cfg, x, y, params, init, masks, thresholds):
    """Live oracle step with the masks and the regulariser.  thresholds: 'split' (see _split_threshold) or
    'default' (0.01 / 0.5, as the command line uses them)."""
    po = {k: v.clone().requires_grad_(v.dtype == torch.float32 and "running" not in k) for k, v in params.items()}
    spikes = []
    out, rates = orc.snn_forward(x, po, neuron_type=cfg["neuron_type"], num_layers=len(cfg["layer_sizes"]),
                                 init_states=init, normalization=cfg["normalization"],
                                 bidirectional=cfg["bidirectional"], training=True, stats={}, drop_masks=masks,
                                 spikes_out=spikes)
    if thresholds == "split":
        thr = _split_threshold(rates, cfg["B"] * cfg["T"])
        loss_kw = dict(use_regularizers=True, reg_fmin=thr, reg_fmax=thr)
    else:
        loss_kw = dict(use_regularizers=True)
    loss = orc.train_step_loss(out, rates, y, **loss_kw)
    loss.backward()
    for k, v in po.items():
        if v.requires_grad:
            assert bool(torch.isfinite(v.grad).all()), ("oracle gradient not finite", k)
    return po, [s.detach() for s in spikes], out.detach(), rates.detach(), loss.detach(), loss_kw


@pytest.mark.parametrize("thresholds", ["split", "default"])
@pytest.mark.parametrize("name", ["dyadic_RadLIF_none", "dyadic_RLIF_none_bias", "dyadic_RadLIF_bidir_none",
                                  "dyadic_RadLIF_bn"])
def test_dyadic_networks_with_dropout_and_regulariser_vs_oracle(name, thresholds, monkeypatch):
    """The four dyadic fixtures' networks with dropout = 0.5 and the firing-rate regulariser in the loss, against the
    live oracle (the fixtures were recorded without either; tests/test_oracle_golden.py pins the oracle to the
    reference, regulariser included).  The kept scale is exactly 2.0, so the next layer's projection sums stay exact
    and every layer's (dropped) spikes must equal the oracle's bit for bit.  Bars of
    test_snn_dyadic_network_bit_equal_spikes_and_gradients: output 2e-5 * T, loss 1e-5 relative, every parameter
    gradient 2e-4 of its max-abs, V.weight's gradient diagonal zero.  With batchnorm, bit-equality is observed, not
    guaranteed (the last bit of the batch variance depends on summation order), as that test's docstring says."""
    import sparch_amd
    from tests.golden_io import snn_case
    from tests.spiking_cases import run_dyadic as _run_dyadic

    cfg, x, y, params, init, z = snn_case(name)
    seeds = _layer_seeds(len(cfg["layer_sizes"]) - 1)
    masks = _network_masks(cfg, seeds, 0.5)
    po, spikes_o, out_o, rates_o, loss_o, loss_kw = _network_oracle(cfg, x, y, params, init, masks, thresholds)
    cfg, z, rec, out, loss, net = _run_dyadic(sparch_amd, name, monkeypatch, dropout=0.5, seeds=seeds, loss_kw=loss_kw)
    assert sorted(rec) == list(range(len(spikes_o)))
    for k in sorted(rec):
        got = rec[k].cpu()
        assert float(spikes_o[k].sum()) > 0 and set(torch.unique(spikes_o[k]).tolist()) == {0.0, 2.0}
        assert torch.equal(got, spikes_o[k]), (k, float((got != spikes_o[k]).float().mean()))
    T = cfg["T"]
    assert float((out.detach().cpu() - out_o).abs().max()) <= 2e-5 * T
    assert abs(float(loss.detach()) - float(loss_o)) <= 1e-5 * max(1.0, abs(float(loss_o)))
    for k, v in net.named_parameters():
        e = relmax(v.grad.cpu().numpy(), po[k].grad.numpy())
        assert e <= 2e-4, (k, e)
        if k.endswith("V.weight"):
            assert float(torch.diag(v.grad).abs().max()) == 0.0


def _odd_width_network(sp):
    """The bidirectional RadLIF [130, 66, 20] network of test_snn_with_hidden_sizes_not_multiples_of_four."""
    B, T, C, sizes = 6, 20, 44, [130, 66, 20]
    cfg = dict(B=B, T=T, C=C, layer_sizes=sizes, neuron_type="RadLIF", normalization="none", bidirectional=True)
    torch.manual_seed(11)
    net = sp.SNN((B, None, C), sizes, neuron_type="RadLIF", dropout=0.5, normalization="none", bidirectional=True)
    with torch.no_grad():
        for lay in net.snn:
            lay.W.weight.copy_(torch.round(lay.W.weight * 4 * 64) / 64)
            if hasattr(lay, "V"):
                lay.V.weight.copy_(torch.round(lay.V.weight * 64) / 64)
    params = {k: v.clone() for k, v in net.state_dict().items()}
    g = torch.Generator().manual_seed(5)
    x = (torch.rand(B, T, C, generator=g) < 0.3).float()
    y = torch.randint(0, sizes[-1], (B,), generator=g)
    torch.manual_seed(7)
    init = orc.draw_init_states(B, sizes, "RadLIF", bidirectional=True)
    init = [{k: torch.floor(v * 16) / 16 for k, v in st.items()} for st in init]
    return cfg, net, params, x, y, init


def test_odd_width_bidirectional_network_with_dropout_and_regulariser_vs_oracle(monkeypatch):
    """Widths 130 and 66 (both run padded to a multiple of 4, per direction) with two directions, dropout = 0.5 and
    the regulariser (split threshold): the mask index is the padded tensor's in both layers.  Bars of
    test_snn_with_hidden_sizes_not_multiples_of_four: per-neuron spike counts equal, loss 1e-5, gradients 2e-4."""
    import sparch_amd
    from sparch_amd import snns as snn_mod

    cfg, net, params, x, y, init = _odd_width_network(sparch_amd)
    seeds = _layer_seeds(2)
    masks = _network_masks(cfg, seeds, 0.5)
    po, spikes_o, out_o, rates_o, loss_o, loss_kw = _network_oracle(cfg, x, y, params, init, masks, "split")
    order = iter([st[k] for st in init for k in ("u0", "w0", "s0") if k in st])
    monkeypatch.setattr(snn_mod, "_rand_to", lambda rows, cols, device: next(order).to(device))
    for lay, seed in zip(list(net.snn)[:-1], seeds):
        lay._dropout_seed = lambda device, seed=seed: seed
    net = net.to(DEV).train()
    out, rates = net(x.to(DEV))
    loss = orc.train_step_loss(out, rates, y.to(DEV), **loss_kw)
    loss.backward()
    _Fn().check_status()
    n = cfg["B"] * cfg["T"]
    assert float(rates_o.sum()) > 0
    assert torch.equal(torch.round(rates.detach().cpu() * n).long(), torch.round(rates_o * n).long())
    assert abs(float(loss.detach()) - float(loss_o)) <= 1e-5 * max(1.0, abs(float(loss_o)))
    for k, v in net.named_parameters():
        assert relmax(v.grad.cpu().numpy(), po[k].grad.numpy()) <= 2e-4, k


# ---------------------------------------------------------------- part 5: the captured step
@pytest.mark.parametrize("kind,compute", [("adLIF", "fp32"), ("RadLIF", "fp32"), ("RadLIF", "bf16")])
def test_graphed_train_step_with_dropout_and_regulariser_matches_eager_steps(kind, compute, request):
    """test_graphed_train_step_matches_eager_steps with what it leaves out: dropout = 0.2 and the firing-rate
    regulariser as `extra_loss`.  In graph mode a layer's seed is a device word advanced inside the captured body, so
    the eager twin's `_dropout_seed` hands out the values read from the graphed step's `_seeds` after each replay:
    same kernels, same masks, and the bars of that test hold unchanged (losses rtol 2e-4 while the trajectories
    coincide, adLIF parameters after 5 steps 2e-4).  The thresholds (0.01 / 0.05) are fixed numbers for which both
    hinge branches are live on the first step (asserted on the eager twin's rates)."""
    import sparch_amd as sp
    from sparch_amd.graph import GraphedTrainStep
    from sparch_amd.optim import Adam

    if compute == "bf16":  # the operand mode is read when a launch is enqueued: captured with the graph
        request.getfixturevalue("bf16_mode")
    B, T, C, sizes = 16, 25, 40, [64, 64, 20]
    fmin, fmax, steps = 0.01, 0.05, 5
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(B, T, C, generator=g) < 0.2).float().to(DEV)
    y = torch.randint(0, sizes[-1], (B,), generator=g).to(DEV)

    def make():
        torch.manual_seed(11)
        net = sp.SNN((B, None, C), sizes, neuron_type=kind, dropout=0.2).to(DEV).train()
        return net, Adam(net.parameters(), 1e-2)

    def regulariser(out, rates):  # exp.py:369-372
        return 0.5 * (torch.relu(fmin - rates).sum() + torch.relu(rates - fmax).sum())

    loss_fn = torch.nn.CrossEntropyLoss()
    net_c, opt_c = make()
    torch.manual_seed(77)
    gs = GraphedTrainStep(net_c, opt_c, loss_fn, x, y, extra_loss=regulariser, warmup=0)
    losses_g, seeds = [], []
    for _ in range(steps):
        losses_g.append(float(gs.step()))
        seeds.append([int(v) for v in gs._seeds.cpu().tolist()])  # the words this replay's kernels read
    _Fn().check_status()
    assert all(seeds[k + 1][i] == seeds[k][i] + 1 for k in range(steps - 1) for i in range(len(seeds[0])))
    assert len(set(seeds[0][:-1])) == len(seeds[0]) - 1  # every hidden layer its own seed
    # eager twin (see test_graphed_train_step_matches_eager_steps for the two discarded draws)
    net_d, opt_d = make()
    torch.manual_seed(77)
    net_d.draw_states(B, torch.device(DEV))
    net_d.draw_states(B, torch.device(DEV))
    step = {"k": 0}
    for i, lay in enumerate(net_d.snn):
        lay._dropout_seed = lambda device, i=i: seeds[step["k"]][i]
    losses_d = []
    for k in range(steps):
        step["k"] = k
        opt_d.zero_grad(set_to_none=True)
        out, rates = net_d(x)
        if k == 0:
            r = rates.detach()
            quiet, burst = float((r < fmin).float().mean()), float((r > fmax).float().mean())
            print(f"{kind}: share of units below fmin {quiet:.3f}, above fmax {burst:.3f}")
            assert quiet > 0 and burst > 0, (quiet, burst)
        loss = loss_fn(out, y)
        loss = loss + regulariser(out, rates)
        loss.backward()
        opt_d.step()
        losses_d.append(float(loss.detach()))
    _Fn().check_status()
    assert float(opt_c.state[next(iter(net_c.parameters()))]["step"]) == steps
    n_cmp = steps if kind == "adLIF" else 2
    np.testing.assert_allclose(losses_g[:n_cmp], losses_d[:n_cmp], rtol=2e-4)
    if kind == "adLIF":
        for (k, pa), pb in zip(net_d.named_parameters(), net_c.parameters()):
            assert relmax(pb.detach().cpu().numpy(), pa.detach().cpu().numpy()) <= 2e-4, k
    gs.close()
