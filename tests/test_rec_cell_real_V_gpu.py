"""
The recurrent spiking kernels (rec_fwd_kernel / rec_bwd_kernel of sparch_amd/csrc/reccell.hip, their launch-per-step forms
and the V pack kernels) with a REAL-VALUED V, against the fp64 restatement tests/spiking_numpy.py, called through
functional.cell_forward / cell_backward.

The bit-exact tests of this suite draw V from 49 dyadic values whose second and third bf16 planes are zero; the
real-valued ones accept any spike flip near the threshold.  Neither sees plane 2 of V, a wave that skips k-groups of it,
or a small cross term of the backward product.  Here nothing is exempted, because nothing free-runs in the reference:

  forward   one free-running launch of the kernel.  Its raw spikes (fp32 tensor, bf16 plane, spike_count) must equal
            u_save > theta on the kernel's OWN saved u, exactly, at the un-flipped time index and feature block.  Its
            u_save[t] / w_save[t] are compared with the restatement's step from the kernel's own state of t - 1
            (teacher-forced: u_save[t-1], w_save[t-1], s_{t-1} = u_save[t-1] > theta; u0 / w0 / real-valued s0 at t = 0).
            Non-vacuity: 5 .. 70 % spikes, and every k-group of every row tile carries a spike at some consumed step.
  backward  the kernel on its own forward saves and a random g_out (g_rate in the bidirectional cases): dWx and the
            gradients of alpha, beta, a, b, V against the restatement's reverse pass on the same saves — linear in g
            given the saves, no discontinuity; the diagonal of dV exactly 0.

Bound (never taken from the code under test): per output tensor, 4 x the worst max-abs error of two fp32 runs of the
restatement (k blocks of 32 ascending, descending) against its fp64 run on the same inputs — the rule of
tests/test_gated_kernels_gpu.py, applied by tests/kit.within.  tests/test_spiking_numpy_host.py shows on the CPU that, for every drive-regime case
here, losing plane 2 of V, a quarter of it, or the t3 * hi term of the backward leaves that bound behind.  Each test
records its worst fraction of the bound (record_property "worst_fraction_of_bound"; DESIGN.md has the figures measured
on an MI355X).

Inputs (spiking_numpy.make_inputs): "drive" — V ~ N(0, 0.5^2), every significand bit live, theta 0.25: the recurrent
term dominates u; "init" — V orthogonal, theta 1.  Shapes: Bp = 33 (two row tiles, the second with one row), T = 6 (the
backward's depth-4 ring wraps), H = 96 / 132 / 384 / 1024 = the kernel shapes kgw 1 / 2 (partial last column tile) /
4 / 8.  Launch forms: whole sequence at every H; chunks of 1 and 4 steps, the bf16 operand mode (V rounded once in the
reference; the dense products read the kernel's own rounded dWx, see spiking_numpy) at H = 132 and 1024; two
directions (B = 17, with scale / shift and g_rate) and the launch-per-step path at H = 132.  (No test of this suite
selects the 64-column workgroups by SPARCH_REC_CW, so none does here.)  The non-recurrent kinds run their backward
through the same restatement and rule at (33, 17, 100), with and without the folded BatchNorm sums.
"""
import numpy as np
import pytest
import torch

from tests import spiking_numpy as sn
from tests.kit import F32, F64, D, N, bf16_mode, record, within  # noqa: F401  (bf16_mode: a fixture)
from tests.kit import Fn as _Fn
from tests.spiking_cases import collect
from tests.spiking_cases import rec_case as case
from tests.spiking_cases import rec_forward as kernel_forward

pytestmark = pytest.mark.gpu


def check_forward(c, spl, operand, record_property):
    """Returns the worst fraction of the bound."""
    kind, B, dirs, T, H, theta = c["kind"], c["B"], c["dirs"], c["T"], c["H"], c["theta"]
    s_out, count, saved, s16 = kernel_forward(c, spl)
    us, ws = N(saved[0]), N(saved[1])
    assert saved[0].dtype == torch.float32 and us.shape == (c["Bp"], T, H) and not np.isnan(us).any()
    # raw spikes: the decision on the kernel's own u, in the kernel's arithmetic, at the output layout
    S = ((us - F32(theta)) > 0).astype(F32)                            # (Bp,T,H), cell time order
    want = sn.out_layout(S, B, dirs)
    assert np.array_equal(N(s_out), want), float((N(s_out) != want).mean())
    if s16 is not None:
        assert s16.dtype == torch.bfloat16 and np.array_equal(N(s16, torch.float32), want)
    assert np.array_equal(N(count).astype(np.int64), want.sum((0, 1)).astype(np.int64))
    # non-vacuity
    frac = float(S.mean())
    assert 0.05 <= frac <= 0.7, frac
    n_rt, n_kg = -(-c["Bp"] // 32), -(-H // 32)
    for rt in range(n_rt):
        for kg in range(n_kg):
            assert S[32 * rt:32 * rt + 32, :T - 1, 32 * kg:32 * kg + 32].any(), ("silent k-group", rt, kg)
    # saved state against the teacher-forced restatement
    args = (c["Wx"], c["scale"], c["shift"], c["p"], c["u0"], c["w0"], c["s0"], us, ws)

    def tf(dt, ko):
        return sn.teacher_forced_forward(kind, dt, *args, B=B, dirs=dirs, theta=theta, k_order=ko, operand=operand)

    ref = tf(F64, None)
    names = sn.FWD_TENSORS[sn.ADAPTIVE[kind]]
    bound = sn.bound_of([tf(F32, "asc"), tf(F32, "desc")], ref, names)
    got = {"u_save": us, "w_save": ws}
    record_property("spike_fraction", round(frac, 3))
    return max(within(got[k], ref[k], bound[k], k) for k in names)


def check_backward(c, spl, operand, with_rate=False, bn=None):
    """Returns the worst fraction of the bound."""
    Fn, d = _Fn(), c["dev"]
    kind, B, dirs, T, H, theta = c["kind"], c["B"], c["dirs"], c["T"], c["H"], c["theta"]
    _, _, saved, _ = kernel_forward(c, spl)
    us, ws = N(saved[0]), N(saved[1])
    x = us - F32(theta)
    if sn.RECURRENT[kind]:
        assert 0.05 <= float((x > 0).mean()) <= 0.7
    assert (x > 0).any() and 0.05 <= float(((x > -0.5) & (x <= 0.5)).mean()) <= 0.95       # spikes; the box-car open and shut
    g_rate = d["g_rate"] if with_rate else None
    bn_dev = None if bn is None else tuple(D(v) for v in bn)
    dWx, grads = Fn.cell_backward(kind, d["g_out"], g_rate, d["p"], d["u0"], d["w0"], d["s0"], saved, B=B, dirs=dirs, T=T,
                                  H=H, theta=theta, p_drop=0.0, seed=0, steps_per_launch=spl, bn=bn_dev)
    Fn.check_status()
    torch.cuda.synchronize()
    got = collect(dWx, grads, bn is not None)
    # (bf16 operand mode: the dense products of the reference read the kernel's own dWx, rounded as the kernel rounds it)
    rec_operand = got["dWx"] if operand is not None else None

    def bw(dt, ko):
        return sn.flat(sn.backward(kind, dt, c["g_out"], c["g_rate"] if with_rate else None, us, ws, c["p"], c["u0"], c["w0"],
                                   c["s0"], B=B, dirs=dirs, theta=theta, k_order=ko, operand=operand,
                                   rec_operand=rec_operand, bn=bn))

    ref = bw(F64, None)
    names = sn.bwd_tensors(kind, bn is not None)
    assert set(names) == set(got), (names, sorted(got))
    bound = sn.bound_of([bw(F32, "asc"), bw(F32, "desc")], ref, names)
    worst = max(within(got[k], ref[k], bound[k], k) for k in names)
    if "V" in got:
        assert np.all(np.diag(got["V"]) == 0) and np.abs(got["V"]).max() > 0
    return worst


# ------------------------------------------------------------------------------------------------ recurrent kinds
WHOLE = [(k, B, dirs, T, H, regime) for regime in ("drive", "init") for (k, B, dirs, T, H) in sn.REC_SHAPES]
CHUNKED = [(k, 33, 1, 6, H, spl) for H in (132, 1024) for k in ("RLIF", "RadLIF") for spl in (1, 4)]
BF16 = [(k, 33, 1, 6, H) for H in (132, 1024) for k in ("RLIF", "RadLIF")]


@pytest.mark.parametrize("kind,B,dirs,T,H,regime", WHOLE)
def test_forward_whole_sequence(kind, B, dirs, T, H, regime, record_property):
    record(record_property, check_forward(case(kind, B, dirs, T, H, regime), None, None, record_property))


@pytest.mark.parametrize("kind,B,dirs,T,H,regime", WHOLE)
def test_backward_whole_sequence(kind, B, dirs, T, H, regime, record_property):
    record(record_property, check_backward(case(kind, B, dirs, T, H, regime), None, None))


@pytest.mark.parametrize("kind,B,dirs,T,H,spl", CHUNKED)
def test_forward_and_backward_in_chunks_of_steps(kind, B, dirs, T, H, spl, record_property):
    c = case(kind, B, dirs, T, H, "drive")
    record(record_property, check_forward(c, spl, None, record_property), check_backward(c, spl, None))


@pytest.mark.parametrize("kind,B,dirs,T,H", sn.BIDIR_SHAPES)
def test_two_directions_with_scale_shift_and_rate_gradient(kind, B, dirs, T, H, record_property):
    c = case(kind, B, dirs, T, H, "drive")
    record(record_property, check_forward(c, None, None, record_property), check_backward(c, None, None, with_rate=True))


@pytest.mark.parametrize("kind", ["RLIF", "RadLIF"])
def test_launch_per_step_path(kind, monkeypatch, record_property):
    monkeypatch.setenv("SPARCH_REC_STEP_PATH", "1")
    assert _Fn().rec_step_path(132)
    c = case(kind, 33, 1, 6, 132, "drive")
    record(record_property, check_forward(c, None, None, record_property), check_backward(c, None, None, with_rate=True))


@pytest.mark.parametrize("kind,B,dirs,T,H", BF16)
def test_bf16_operand_mode(kind, B, dirs, T, H, bf16_mode, record_property):
    assert bf16_mode.compute_dtype() == "bf16"
    c = case(kind, B, dirs, T, H, "drive")
    record(record_property, check_forward(c, None, sn.bf16_round, record_property), check_backward(c, None, sn.bf16_round))


# ------------------------------------------------------------------------------------------------ non-recurrent kinds
@pytest.mark.parametrize("with_bn", [False, True], ids=["plain", "bn_sums"])
@pytest.mark.parametrize("kind", ["LIF", "adLIF"])
def test_nonrecurrent_backward(kind, with_bn, record_property):
    """(Bp, T, H) = (33, 17, 100): T on both sides of the scan kernels' ring depths.  The forward of these kinds is
    bit-exact against the oracle elsewhere; here the backward on the kernel's own saves, with the firing-rate gradient."""
    B, T, H = 33, 17, 100
    c = case(kind, B, 1, T, H, "drive")
    bn = None
    if with_bn:
        rng = np.random.default_rng(7)
        bn = ((c["Wx"] * 0.8 + 0.3).astype(F32), rng.uniform(0.2, 0.6, H).astype(F32), rng.uniform(0.5, 1.5, H).astype(F32))
    record(record_property, check_backward(c, None, None, with_rate=True, bn=bn))
