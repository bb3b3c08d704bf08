"""
tests/spiking_numpy.py — the reference and yardstick of tests/test_rec_cell_real_V_gpu.py — pinned on the CPU:

  * its fp32 free-running forward equals oracle.bptt_numpy.cell_forward bit for bit (u, w, spikes), all four kinds;
  * its fp64 backward on its own fp64 saves equals torch autograd of oracle.snn_oracle.spiking_cell in float64 to
    1e-12 of each tensor's max-abs: all four kinds, one and two directions, with scale / shift and the firing-rate
    gradient;
  * the teacher-forced form fed the restatement's own saves reproduces them exactly;
  * SHARPNESS of the GPU file's bound.  For every drive-regime case of that file, with the restatement's fp32 saves
    standing in for the kernel's, the bound (4 x the worst fp32-restatement error, k blocks ascending and descending,
    against fp64) is computed exactly as the GPU file computes it, and a reference run with a MUTATED recurrent product
    must leave it behind:
        V without plane 2 of the truncation split (split3)       u_save error >= 3 x bound
        ... in the first quarter of k only                                    >  1 x bound
        dWx Vm^T without the cross term t3 * hi                  dWx error    >  1 x bound
    and, beyond what was asked for, with the NEAREST-EVEN split the pack kernels of reccell.hip really make (its third
    plane has a quarter of the truncation split's root mean square and no common sign — the weaker, honest mutant):
        V without plane 2 (lo) of split3_rne                     u_save error >= 2 x bound
        ... in the first quarter of k only                                    >  1 x bound
    A kernel that stays within the bound and loses lo is then at least 2 - 1 bounds off: the GPU test must fail.
    Measured here, error / bound (record_property keeps them per case), RLIF | RadLIF:
        H               plane 2        quarter k      lo (rne)       quarter k (rne)   t3 * hi
        96              16.2 |  9.9    6.0 | 5.6      2.78 | 2.24    1.61 | 1.36       7.8 |  5.5
        132             14.3 |  9.7    8.7 | 5.0      3.41 | 2.65    1.74 | 1.38       7.7 |  6.7
        384             13.2 | 13.6    4.0 | 6.3      2.29 | 2.83    1.26 | 1.50      18.3 |  7.8
        1024             9.9 | 11.5    6.2 | 6.3      2.55 | 2.65    1.45 | 1.51      17.0 | 13.3
        132, 2 dirs      9.7 | 11.8    7.8 | 4.7      2.14 | 4.75    1.34 | 1.70       9.6 |  5.3
    Every mutant is resolved at every H of the GPU file; a nearest-even lo plane lost in a quarter of k is resolved with
    the least room (1.26 .. 1.74 bounds: a kernel that is itself more than a quarter of a bound off could hide it).
    The bound is made of the rounding of u itself — half an ulp of the largest |u| of the tensor — which is why the
    drive regime keeps |u| within a few units (spiking_numpy.make_inputs).
  * for tests/test_scan_kernels_fp64_gpu.py and tests/test_readout_kernels_fp64_gpu.py (second half of this file):
    backward(keep=) against float64 autograd with the mask as a constant; the readout restatement against float64
    autograd of oracle.snn_oracle.readout_cell, affine and BatchNorm sums included; save_u16 in numpy on 10^6 values;
    the TIE regression — LIF (33, 2, 9, 7944) holds one saved potential whose u - theta <= -0.5 in fp32 and not in
    fp64, and with the box-car edges taken in the run's dtype bound_of('dWx') was 0.27 for a tensor of max-abs 0.45
    (any kernel would have passed); taken in the save's own type it is 4e-7 of max-abs; and the sharpness of the two
    files' bounds.  Measured here, mutant error / bound, smallest over the cases:
        scan     rate term over B dirs T 2.1e5   keep not on the rate term 8.6e4   step 0 reads u_save[0] 8.5e5
                 xhat without its mean in the last column 2.0e4 (the column's share of a 7944-wide sum)
        readout  u0 ignored 9.3e5   dot over C - 1 classes 1.8e3   ragged sweep's last element as 0 2.9e3
"""
import numpy as np
import pytest
import torch

from oracle import bptt_numpy as bn
from oracle import snn_oracle as orc
from tests import spiking_numpy as sn
from tests.kit import F32, F64, SEED


def _args(c):
    return (c["Wx"], c["scale"], c["shift"], c["p"], c["u0"], c["w0"], c["s0"])


def _geo(c):
    return {"B": c["B"], "dirs": c["dirs"], "theta": c["theta"]}


@pytest.mark.parametrize("kind", sn.KINDS)
def test_fp32_forward_equals_bptt_numpy_bit_for_bit(kind):
    for regime in ("drive", "init"):
        c = sn.make_inputs(kind, 7, 1, 14, 40, 11, regime)
        got = sn.forward(kind, F32, *_args(c), **_geo(c))
        S, U, W = bn.cell_forward(kind, c["Wx"], c["p"], c["u0"], c["w0"], c["s0"], c["theta"])
        assert 0 < S.mean() < 0.7
        for a, b in ((got["s"], S), (got["u_save"], U)) + (((got["w_save"], W),) if W is not None else ()):
            assert a.dtype == F32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(got["count"], S.sum((0, 1)).astype(np.int64))


class _Boxcar64(orc._Boxcar):
    """The oracle's surrogate with a forward that keeps the input's dtype (its own returns float32, which a float64
    matmul refuses); the backward is the oracle's."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return (x > 0).to(x.dtype)


@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("kind", sn.KINDS)
def test_fp64_backward_equals_autograd_of_the_oracle(kind, dirs, monkeypatch):
    monkeypatch.setattr(orc, "spike", _Boxcar64.apply)
    for k in ("alpha", "beta", "a", "b"):          # the kernels' float32 limits (the oracle's are the doubles)
        monkeypatch.setattr(orc, k.upper() + "_LIM", tuple(float(v) for v in sn.LIMS[k]))
    B, T, H = 5, 9, 24
    c = sn.make_inputs(kind, B, dirs, T, H, 100 + dirs, "drive", affine_in=True)
    c["p"]["alpha"][:2] = (0.5, 0.99)                       # outside the clamp range: gated gradients
    if sn.ADAPTIVE[kind]:
        c["p"]["a"][2], c["p"]["b"][3], c["p"]["beta"][4] = 1.5, -0.1, 0.999
    fwd = sn.forward(kind, F64, *_args(c), **_geo(c))
    got = sn.backward(kind, F64, c["g_out"], c["g_rate"], fwd["u_save"], fwd["w_save"], c["p"], c["u0"], c["w0"], c["s0"],
                      **_geo(c))

    t64 = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=F64))  # noqa: E731
    xv = t64(sn.affine(c["Wx"], c["scale"], c["shift"], dirs, F64)).requires_grad_(True)
    p = {k: t64(v).requires_grad_(True) for k, v in c["p"].items()}
    s = orc.spiking_cell(kind, xv, p, t64(c["u0"]), t64(c["w0"]), t64(c["s0"]), c["theta"])
    assert np.array_equal(s.detach().numpy(), fwd["s"]) and 0.01 < fwd["s"].mean() < 0.7
    o = s if dirs == 1 else torch.cat([s[:B], s[B:].flip(1)], dim=2)
    assert np.array_equal(o.detach().numpy(), fwd["s_out"])
    loss = (o * t64(c["g_out"])).sum() + (o.sum((0, 1)) / (B * T) * t64(c["g_rate"])).sum()
    loss.backward()

    def close(a, ref, what):
        ref = ref.numpy()
        assert np.abs(a - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), what

    close(got["dWx"], torch.from_numpy(sn.to_original(xv.grad.numpy(), B, dirs)), "dWx")
    for k in p:
        close(got[k], p[k].grad, k)
        if k != "V":
            assert np.array_equal(got[k], got["ws_" + k].sum(0) * sn.inside(c["p"][k], sn.LIMS[k]))
    assert got["alpha"][0] == 0 and got["alpha"][1] == 0 and np.abs(got["alpha"][2:]).min() > 0
    if "V" in got:
        assert np.all(np.diag(got["V"]) == 0)


@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("kind", sn.KINDS)
def test_teacher_forced_on_own_saves_reproduces_them(kind, dirs):
    c = sn.make_inputs(kind, 6, dirs, 10, 72, 5, "drive", affine_in=(dirs == 2))
    for dt in (F32, F64):
        for ko in (None, "desc"):
            free = sn.forward(kind, dt, *_args(c), k_order=ko, **_geo(c))
            tf = sn.teacher_forced_forward(kind, dt, *_args(c), free["u_save"], free["w_save"], k_order=ko, **_geo(c))
            for k in ("u_save", "w_save", "s", "s_out", "count"):
                assert (free[k] is None and tf[k] is None) or np.array_equal(free[k], tf[k]), (k, dt, ko)


def test_splits_are_exact():
    x = (np.random.default_rng(0).standard_normal((64, 96)) * 0.5).astype(F32)
    for parts in (sn.split3(x), sn.split3_rne(x)):
        assert np.array_equal((parts[0].astype(F64) + parts[1]) + parts[2], x.astype(F64))
        assert all(np.array_equal(sn.bf16_round(q), q) for q in parts) and np.abs(parts[2]).max() > 0
    assert np.abs(sn.split3_rne(x)[2]).max() <= 2.0 ** -17 * np.abs(x).max()
    q = sn.V_without_plane2(x, 0.25)
    assert np.array_equal(q[16:], x[16:]) and np.array_equal(q[:16], sn.V_without_plane2(x)[:16]) and (q[:16] != x[:16]).any()


def _err(a, ref):
    return float(np.abs(a.astype(F64) - ref).max())


@pytest.mark.parametrize("kind,B,dirs,T,H", sn.REC_SHAPES + sn.BIDIR_SHAPES,
                         ids=lambda v: str(v))
def test_bound_of_the_gpu_file_resolves_the_mutants(kind, B, dirs, T, H, record_property):
    c = sn.make_inputs(kind, B, dirs, T, H, sn.case_seed(kind, B, dirs, T, H), "drive", affine_in=(dirs == 2))
    geo = _geo(c)
    saves = sn.forward(kind, F32, *_args(c), k_order="asc", **geo)          # stands in for the kernel's saves
    us, ws = saves["u_save"], saves["w_save"]
    assert 0.05 <= saves["s"].mean() <= 0.7

    def tf(dt, ko, p=None):
        a = list(_args(c))
        if p is not None:
            a[3] = p
        return sn.teacher_forced_forward(kind, dt, *a, us, ws, k_order=ko, **geo)

    ref = tf(F64, None)
    bound = sn.bound_of([tf(F32, "asc"), tf(F32, "desc")], ref, sn.FWD_TENSORS[sn.ADAPTIVE[kind]])

    def mutant(frac, split):
        V = sn.V_without_plane2(c["p"]["V"], frac, split)
        return _err(tf(F64, None, dict(c["p"], V=V))["u_save"], ref["u_save"]) / bound["u_save"]

    f_all, f_quarter, f_all_rne, f_quarter_rne = mutant(1, "trunc"), mutant(0.25, "trunc"), mutant(1, "rne"), mutant(0.25, "rne")

    def bw(dt, ko, **kw):
        return sn.backward(kind, dt, c["g_out"], None, us, ws, c["p"], c["u0"], c["w0"], c["s0"], k_order=ko, **geo, **kw)

    refb = bw(F64, None)
    boundb = sn.bound_of([bw(F32, "asc"), bw(F32, "desc")], refb, ("dWx",))
    f_t3 = _err(bw(F64, None, rec_product=sn.rec_bwd_without_t3_hi)["dWx"], refb["dWx"]) / boundb["dWx"]
    for k, v in (("plane2", f_all), ("quarter_k", f_quarter), ("plane2_rne", f_all_rne), ("quarter_k_rne", f_quarter_rne),
                 ("t3_hi", f_t3)):
        record_property(k + "_over_bound", round(v, 2))
    print(f"{kind} H={H} dirs={dirs} spikes {saves['s'].mean():.3f}: plane 2 {f_all:.1f} (rne {f_all_rne:.2f}), quarter k "
          f"{f_quarter:.1f} (rne {f_quarter_rne:.2f}), t3*hi {f_t3:.1f} x bound")
    assert f_all >= 3.0, f_all
    assert f_quarter > 1.0, f_quarter
    assert f_t3 > 1.0, f_t3
    assert f_all_rne >= 2.0, f_all_rne
    assert f_quarter_rne > 1.0, f_quarter_rne


# ============================================================== the scan (LIF / adLIF) and readout kernels' restatement
# tests/test_scan_kernels_fp64_gpu.py and tests/test_readout_kernels_fp64_gpu.py rest on the pieces pinned here: the
# dropout multiplier of backward(), the readout restatement, save_u16 in numpy, the decisions taken in the save's own
# type (the tie regression) and the sharpness of the two files' bounds.


@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("kind", ["LIF", "adLIF"])
def test_fp64_backward_with_keep_equals_autograd_of_the_oracle(kind, dirs, monkeypatch):
    """The dropout multiplier as a constant of the graph: loss = <s keep, g_out> + <sum(s keep) / (B T), g_rate>."""
    from tests.dropout_numpy import keep_mask
    monkeypatch.setattr(orc, "spike", _Boxcar64.apply)
    for k in ("alpha", "beta", "a", "b"):
        monkeypatch.setattr(orc, k.upper() + "_LIM", tuple(float(v) for v in sn.LIMS[k]))
    B, T, H = 5, 9, 24
    c = sn.make_inputs(kind, B, dirs, T, H, 200 + dirs, "drive", affine_in=True)
    c["g_rate"] = c["g_rate"] * F32(B * T)
    c["p"]["alpha"][:2] = (0.5, 0.99)
    keep = keep_mask(SEED, (B, T, H * dirs), 0.25)
    assert set(np.unique(keep)) == {F32(0), F32(1) / F32(0.75)}
    fwd = sn.forward(kind, F64, *_args(c), **_geo(c))
    got = sn.backward(kind, F64, c["g_out"], c["g_rate"], fwd["u_save"], fwd["w_save"], c["p"], c["u0"], c["w0"], c["s0"],
                      keep=keep, **_geo(c))
    ordered = sn.backward(kind, F64, c["g_out"], c["g_rate"], fwd["u_save"], fwd["w_save"], c["p"], c["u0"], c["w0"],
                          c["s0"], keep=keep, row_order="desc", **_geo(c))

    t64 = lambda a: None if a is None else torch.from_numpy(np.asarray(a, dtype=F64))  # noqa: E731
    xv = t64(sn.affine(c["Wx"], c["scale"], c["shift"], dirs, F64)).requires_grad_(True)
    p = {k: t64(v).requires_grad_(True) for k, v in c["p"].items()}
    s = orc.spiking_cell(kind, xv, p, t64(c["u0"]), t64(c["w0"]), t64(c["s0"]), c["theta"])
    o = (s if dirs == 1 else torch.cat([s[:B], s[B:].flip(1)], dim=2)) * t64(keep)
    assert 0.01 < fwd["s"].mean() < 0.7
    ((o * t64(c["g_out"])).sum() + (o.sum((0, 1)) / (B * T) * t64(c["g_rate"])).sum()).backward()

    def close(a, ref, what):
        assert np.abs(a - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), what

    close(got["dWx"], sn.to_original(xv.grad.numpy(), B, dirs), "dWx")
    for k in p:
        close(got[k], p[k].grad.numpy(), k)
        close(ordered[k], p[k].grad.numpy(), k + " (rows descending)")
    assert got["alpha"][0] == 0 and got["alpha"][1] == 0 and np.abs(got["alpha"][2:]).min() > 0


@pytest.mark.parametrize("with_bn", [False, True], ids=["plain", "affine_bn"])
def test_fp64_readout_restatement_equals_autograd_of_the_oracle(with_bn, monkeypatch):
    """out, dWx and the alpha gradient (two alphas outside the clamp range, one on each side: gated); with the affine,
    the BN sums are the gradients of shift and scale of an explicit xhat * scale + shift."""
    monkeypatch.setattr(orc, "ALPHA_LIM", tuple(float(v) for v in sn.LIMS["alpha"]))
    c = sn.readout_case(4, 23, 11)
    assert c["alpha"][0] < sn.LIMS["alpha"][0] and c["alpha"][1] > sn.LIMS["alpha"][1]
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=F64))  # noqa: E731
    alpha = t64(c["alpha"]).requires_grad_(True)
    if with_bn:
        x_raw, mean, invstd = c["bn"]
        weight, bias = c["scale"].astype(F64), c["shift"].astype(F64)
        scale = (invstd.astype(F64) * weight).astype(F32)         # the fold, rounded to the fp32 the kernel is handed
        shift = (bias - mean.astype(F64) * scale.astype(F64)).astype(F32)
        # the explicit form of that same affine map: xhat * w + b with w = scale / invstd, b = shift + mean * scale
        w = (t64(scale) / t64(invstd)).requires_grad_(True)
        b = (t64(shift) + t64(mean) * t64(scale)).requires_grad_(True)
        x = ((t64(x_raw) - t64(mean)) * t64(invstd) * w + b)
        x.retain_grad()
        fwd_args, bn = (x_raw, scale, shift), c["bn"]
    else:
        x = t64(c["Wx"]).requires_grad_(True)
        fwd_args, bn = (c["Wx"], None, None), None
    out = orc.readout_cell(x, alpha, t64(c["u0"]))
    (out * t64(c["g_out"])).sum().backward()

    def close(a, ref, what):
        ref = ref.detach().numpy()
        assert a.shape == ref.shape and np.abs(a - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), what

    for order in (None, "asc", "desc"):
        u_save, got_out = sn.readout_forward(F64, *fwd_args, c["alpha"], c["u0"], class_order=order)
        close(got_out, out, "out")
        got = sn.readout_backward(F64, c["g_out"], u_save, c["alpha"], c["u0"], bn=bn, class_order=order)
        close(got["dWx"], x.grad, "dWx")
        close(got["alpha"], alpha.grad, "alpha")
        assert got["alpha"][0] == 0 and got["alpha"][1] == 0 and np.abs(got["alpha"][2:]).min() > 0
        assert np.array_equal(got["alpha"][2:], sn.ordered_sum(got["ws_alpha"], 0, order)[2:])
        if with_bn:
            close(got["bn_dy"], b.grad, "bn_dy")
            close(got["bn_dyx"], w.grad, "bn_dyx")
    assert np.abs(out.detach().numpy().sum() - 4 * 23) < 1e-9


def test_save_u16_keeps_every_decision_and_stays_within_one_ulp():
    """10^6 values that include exact ties and values within one bf16 ulp of theta and theta +- 0.5."""
    rng = np.random.default_rng(16)
    for theta in (F32(0.25), F32(1.0)):
        edges = np.array([theta, theta - F32(0.5), theta + F32(0.5)], dtype=F32)
        ulp = F32(2.0 ** -7)                                      # above a bf16 ulp of every |value| < 2 here
        near = (edges[rng.integers(0, 3, 600000)] + rng.uniform(-1, 1, 600000).astype(F32) * ulp).astype(F32)
        steps = np.nextafter(np.repeat(edges, 2), np.tile(np.array([-np.inf, np.inf], dtype=F32), 3)).astype(F32)
        wide = (rng.standard_normal(400000 - 12) * 1.5).astype(F32)
        u = np.concatenate([near, wide, edges, steps, np.array([0.0, -0.0, 1e-30], dtype=F32)])
        assert u.size == 10 ** 6
        b = sn.save_u16(u, theta)
        v = sn.bf16_to_f32(b)
        assert np.array_equal(sn.decisions_of(v, theta), sn.decisions_of(u, theta))
        plain = sn.bf16_words(u)
        assert np.array_equal(sn.bf16_to_f32(plain), sn.bf16_round(u))          # the rounding itself, against torch's
        moved = b != plain
        assert 100 < moved.sum() < u.size // 2                                    # the step back is taken, and not always
        one_ulp = np.maximum(np.abs(sn.bf16_to_f32(b + np.uint16(1)) - v), np.abs(v - sn.bf16_to_f32(b - np.uint16(1))))
        ok = (b & np.uint16(0x7FFF)) != 0
        assert np.all(np.abs(v.astype(F64) - u)[ok] <= one_ulp[ok].astype(F64))
        assert np.all(np.abs(v.astype(F64) - u)[~ok] <= 2.0 ** -126)
        assert np.all((sn.decisions_of(sn.bf16_to_f32(plain), theta) != sn.decisions_of(u, theta))[moved])


def _scan_runs(c, us, ws, keep, **kw):
    kind = c["kind"]

    def bw(dt, ro, **more):
        return sn.flat(sn.backward(kind, dt, c["g_out"], c["g_rate"], us, ws, c["p"], c["u0"], c["w0"], c["s0"], bn=c["bn"],
                                   keep=keep, row_order=ro, **_geo(c), **kw, **more))
    return bw


def test_a_tie_on_a_boxcar_edge_does_not_widen_the_bound():
    """LIF (33, 2, 9, 7944): one of 4 718 736 saved potentials has u - theta <= -0.5 in fp32 and not in fp64.  Taken
    from U - theta in the run's dtype the edge differs between the fp32 and fp64 runs and bound_of('dWx') was 0.27 for
    a tensor whose max-abs is 0.45; taken in the save's own type, as the kernels take it, the bound is rounding."""
    kind, B, dirs, T, H = "LIF", 33, 2, 9, 7944
    c = sn.make_inputs(kind, B, dirs, T, H, sn.case_seed(kind, B, dirs, T, H), "drive", affine_in=True)
    us = sn.forward(kind, F32, *_args(c), **_geo(c))["u_save"]
    x32, x64 = us - F32(c["theta"]), us.astype(F64) - c["theta"]
    ties = int(((x32 <= F32(-0.5)) != (x64 <= -0.5)).sum() + ((x32 > F32(0.5)) != (x64 > 0.5)).sum())
    assert ties >= 1, "the case holds no tie: it no longer shows what it is here for"

    def bw(dt):
        return sn.backward(kind, dt, c["g_out"], c["g_rate"], us, None, c["p"], c["u0"], None, c["s0"], **_geo(c))

    ref = bw(F64)
    bound = sn.bound_of([bw(F32)], ref, ("dWx",))["dWx"]
    assert bound <= 1e-5 * np.abs(ref["dWx"]).max(), (bound, float(np.abs(ref["dWx"]).max()), ties)


@pytest.mark.parametrize("kind,B,dirs,T,H", sn.SCAN_SHAPES, ids=lambda v: str(v))
def test_bound_of_the_scan_file_resolves_the_mutants(kind, B, dirs, T, H, record_property):
    """Every drive case of tests/test_scan_kernels_fp64_gpu.py in its fullest variant (BN sums, dropout, g_rate), the
    fp32 restatement's saves standing in for the kernel's: each mutated fp64 backward leaves the bound of its tensor
    behind by >= 10 x.  (One direction: the rate term's mutant is the identity and is not run.)"""
    c = sn.scan_case(kind, B, dirs, T, H)
    f = sn.forward(kind, F32, *_args(c), **_geo(c))
    us, ws = f["u_save"], f["w_save"]
    keep = sn.scan_keep(c, SEED)
    sn.scan_conditions(c, us, keep)
    bw = _scan_runs(c, us, ws, keep)
    ref = bw(F64, None)
    names = sn.bwd_tensors(kind, True)
    bound = sn.capped(sn.bound_of([bw(F32, "asc"), bw(F32, "desc")], ref, names), ref, names)
    mutants = {"rate_over_dirs": "dWx", "keep_not_on_rate": "dWx", "step0_reads_u_save": "alpha",
               "xhat_without_mean_last_column": "bn_dyx"}
    assert set(mutants) == set(sn.SCAN_MUTANTS)
    for m, k in mutants.items():
        if m == "rate_over_dirs" and dirs == 1:
            continue
        ratio = _err(bw(F64, None, mutant=m)[k], ref[k]) / bound[k]
        record_property(m + "_over_bound", round(ratio, 1))
        print(f"{kind} ({B},{dirs},{T},{H}) {m}: {k} {ratio:.3g} x bound")
        assert ratio >= 10.0, (m, k, ratio)


@pytest.mark.parametrize("B,T,C", sn.READOUT_SHAPES, ids=lambda v: str(v))
def test_bound_of_the_readout_file_resolves_the_mutants(B, T, C, record_property):
    """Every shape of tests/test_readout_kernels_fp64_gpu.py with BN sums, on the fp32 restatement's u_save.  C = 1:
    the softmax is the constant 1 and dWx, dalpha are identically 0 — only the dot's mutant changes anything there."""
    c = sn.readout_case(B, T, C)
    us = sn.readout_forward(F32, c["bn"][0], c["scale"], c["shift"], c["alpha"], c["u0"], "asc")[0]

    def bw(dt, order, **kw):
        return sn.readout_backward(dt, c["g_out"], us, c["alpha"], c["u0"], bn=c["bn"], class_order=order, **kw)

    ref = bw(F64, None)
    names = sn.READOUT_BWD_TENSORS[True]
    bound = sn.capped(sn.bound_of([bw(F32, "asc"), bw(F32, "desc")], ref, names), ref, names)
    mutants = {"u0_ignored": "alpha", "dot_without_last_class": "dWx", "ragged_sweep_tail_zero": "dWx"}
    assert set(mutants) == set(sn.READOUT_MUTANTS)
    for m, k in mutants.items():
        if C == 1 and m != "dot_without_last_class":
            continue
        err = _err(bw(F64, None, mutant=m)[k], ref[k])
        ratio = err / bound[k] if bound[k] > 0 else float("inf") if err > 0 else 0.0
        record_property(m + "_over_bound", round(min(ratio, 1e12), 1))
        print(f"readout ({B},{T},{C}) {m}: {k} {ratio:.3g} x bound")
        assert ratio >= 10.0, (m, k, ratio)
