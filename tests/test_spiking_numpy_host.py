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
"""
import numpy as np
import pytest
import torch

from oracle import bptt_numpy as bn
from oracle import snn_oracle as orc
from tests import spiking_numpy as sn

F32, F64 = np.float32, np.float64


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
