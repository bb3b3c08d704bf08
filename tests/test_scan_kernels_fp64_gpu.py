"""
The LIF / adLIF scan kernels (cell_fwd_pipe_kernel / cell_bwd_pipe_kernel of sparch_amd/csrc/cell.hip) against the fp64
restatement tests/spiking_numpy.py on real-valued data, through functional.cell_forward / cell_backward, in every
instantiation the dispatcher can take: kind {LIF, adLIF} x neurons per thread {4, 1} x saves {fp32, bf16} x folded
BatchNorm sums {off, on} x dropout {off, on} — the 32 backward kernels, each once — and the ring depths' edges.

  forward   one launch per variant on one set of inputs.  Raw spikes (fp32 tensor, bf16 plane, spike_count) equal
            [u_save - theta > 0] on the kernel's OWN fp32 u_save times the numpy keep mask (tests/dropout_numpy.py),
            exactly; u_save / w_save against the teacher-forced restatement (every step from the kernel's own state of
            the step before: nothing free-runs, so no spike flip is exempted).  want_s_out=False, want_saves=False and
            bf16 saves give the same plane and counts bit for bit; the bf16 u_save words equal spiking_numpy.save_u16 of
            the fp32 run's u_save exactly, the w_save words its round-to-nearest-even.
  backward  the kernel on its own saves (bf16 saves upcast exactly), g_out, g_rate (scaled by B T: as large as g_out),
            BatchNorm operands and the dropout mask: dWx, the gradients of alpha, beta, a, b and the two BatchNorm sums
            against the restatement's reverse pass on the same saves.  Clamped-out parameters (neuron 0 below, neuron 1
            above the range) get exactly 0.

Bound (never taken from the code under test): per tensor 4 x the worst max-abs error of the fp32 restatement (sums over
the rows ascending, descending) against its fp64 run on the same inputs, the rule of tests/test_gated_kernels_gpu.py;
and every bound is at most 1e-5 of its reference tensor's max-abs (spiking_numpy.capped), so that a tie on a box-car edge
between the fp32 and fp64 runs — which made the bound 0.27 of a 0.45 tensor before the restatement took its decisions in
the save's own type — cannot hide a failure.  tests/test_spiking_numpy_host.py shows that the bound resolves a rate term
scaled by 1/(B dirs T), a keep factor missing from the rate term, a cell step 0 that reads u_save[0] for u0 and an xhat
without its mean by four orders of magnitude.

Conditions (spiking_numpy.scan_conditions, on the fp32 restatement's free-running saves — not the kernel's): 2 .. 50 %
spikes, the box-car open on 5 .. 95 %, and with dropout kept and dropped elements among the non-fired ones inside the
box-car, 0.75 +- 0.02 kept.  A seed that breaks one gets another through spiking_numpy.SCAN_SALT; the conditions stay.

Shapes (spiking_numpy): V4 (33, 2, 7944) = 524 304 neurons, 1986 threads per row: waves straddle rows; V1BIG
(33, 2, 7940), just under the threshold at nearly the same size; V1 (33, 2, 100); V1ODD (33, 1, 99).  T = 9 at V4 (ring
depth 8: one main trip and a one-step tail that is cell step 0), T = 17 at V1 (depths 16 / 15 / 15 / 12); the sweeps run
T on both sides of every depth on the fullest variant.  The stream entry sparch_cell_stream_fwd runs at (33, 15888),
four neurons per thread, through StreamingSNN's own call.
"""
import numpy as np
import pytest
import torch

from tests import spiking_numpy as sn
from tests.kit import DEV, F32, F64, SEED, D, N, record, within, words
from tests.kit import Fn as _Fn
from tests.spiking_cases import collect
from tests.spiking_cases import scan_case_of as case_of
from tests.spiking_cases import scan_forward as kernel_forward

pytestmark = pytest.mark.gpu

P_DROP = sn.P_DROP


def check_forward(c, p_drop):
    """Returns the worst fraction of the bound."""
    kind, B, dirs, T, H, theta = c["kind"], c["B"], c["dirs"], c["T"], c["H"], c["theta"]
    adaptive = sn.ADAPTIVE[kind]
    s_out, count, saved, s16 = kernel_forward(c, p_drop)
    us, ws = N(saved[0]), N(saved[1])
    assert saved[0].dtype == torch.float32 and us.shape == (c["Bp"], T, H) and not np.isnan(us).any()
    # spikes: the decision on the kernel's own u, in the kernel's arithmetic, times the mask, at the output layout
    S = ((us - F32(theta)) > 0).astype(F32)
    want = sn.out_layout(S, B, dirs) * (c["keep"] if p_drop else F32(1))
    plane = (want != 0).astype(F32)
    cnt = plane.sum((0, 1)).astype(np.int64)
    assert 0.02 <= S.mean() <= 0.5 and (p_drop == 0 or 0 < cnt.sum() < S.sum())
    assert np.array_equal(N(s_out), want), float((N(s_out) != want).mean())
    assert s16.dtype == torch.bfloat16 and np.array_equal(N(s16, torch.float32), plane)
    assert np.array_equal(N(count).astype(np.int64), cnt)
    # the saved states against the teacher-forced restatement
    args = (c["Wx"], c["scale"], c["shift"], c["p"], c["u0"], c["w0"], c["s0"], us, ws)
    tf = lambda dt: sn.teacher_forced_forward(kind, dt, *args, B=B, dirs=dirs, theta=theta)  # noqa: E731
    ref = tf(F64)
    names = sn.FWD_TENSORS[adaptive]
    bound = sn.capped(sn.bound_of([tf(F32)], ref, names), ref, names)
    worst = max(within({"u_save": us, "w_save": ws}[k], ref[k], bound[k], k) for k in names)
    # the other output selections and save types: the same plane and counts, bit for bit
    for kw in ({"want_s_out": False}, {"want_saves": False}) + (({"save16": True},) if H % 4 == 0 else ()):
        s2, count2, saved2, s16_2 = kernel_forward(c, p_drop, **kw)
        assert torch.equal(s16_2, s16) and torch.equal(count2, count), kw
        if "want_s_out" in kw:
            assert s2 is None and torch.equal(saved2[0], saved[0])
        elif "want_saves" in kw:
            assert saved2[0] is None and saved2[1] is None and torch.equal(s2, s_out)
        else:
            assert saved2[0].dtype == torch.bfloat16 and torch.equal(s2, s_out)
            got_u, want_u = words(saved2[0]), sn.save_u16(us, theta)
            assert np.array_equal(got_u, want_u), int((got_u != want_u).sum())
            assert (want_u != sn.bf16_words(us)).any() or H < 1000, "no saved potential took the step back"
            if adaptive:
                assert saved2[1].dtype == torch.bfloat16 and np.array_equal(words(saved2[1]), sn.bf16_words(ws))
    return worst


def check_backward(c, save16, with_bn, p_drop):
    """Returns the worst fraction of the bound."""
    Fn, d = _Fn(), c["dev"]
    kind, B, dirs, T, H, theta = c["kind"], c["B"], c["dirs"], c["T"], c["H"], c["theta"]
    _, _, saved, _ = kernel_forward(c, p_drop, save16)
    assert saved[0].dtype == (torch.bfloat16 if save16 else torch.float32)
    us, ws = N(saved[0], torch.float32), N(saved[1], torch.float32)        # (bf16 -> fp32 is exact)
    x = us - F32(theta)
    assert 0.02 <= (x > 0).mean() <= 0.5 and 0.05 <= ((x > F32(-0.5)) & (x <= F32(0.5))).mean() <= 0.95
    dWx, grads = Fn.cell_backward(kind, d["g_out"], d["g_rate"], d["p"], d["u0"], d["w0"], d["s0"], saved, B=B, dirs=dirs,
                                  T=T, H=H, theta=theta, p_drop=p_drop, seed=SEED, bn=d["bn"] if with_bn else None)
    Fn.check_status()
    torch.cuda.synchronize()
    got = collect(dWx, grads, with_bn)

    def bw(dt, ro):
        return sn.flat(sn.backward(kind, dt, c["g_out"], c["g_rate"], us, ws, c["p"], c["u0"], c["w0"], c["s0"], B=B,
                                   dirs=dirs, theta=theta, bn=c["bn"] if with_bn else None,
                                   keep=c["keep"] if p_drop else None, row_order=ro))

    ref = bw(F64, None)
    names = sn.bwd_tensors(kind, with_bn)
    assert set(names) == set(got), (names, sorted(got))
    bound = sn.capped(sn.bound_of([bw(F32, "asc"), bw(F32, "desc")], ref, names), ref, names)
    worst = max(within(got[k], ref[k], bound[k], k) for k in names)
    for k in c["p"]:                                                       # neuron 0 below, neuron 1 above the clamp range
        assert got[k][0] == 0 and got[k][1] == 0 and np.abs(got[k][2:]).max() > 0, k
    return worst


FORWARD = [(g, p) for g in ("V4", "V1") for p in (0.0, P_DROP)] + [("V1big", P_DROP), ("V1odd", P_DROP)]


@pytest.mark.parametrize("geom,p_drop", FORWARD)
@pytest.mark.parametrize("kind", sn.SCAN_KINDS)
def test_forward(kind, geom, p_drop, record_property):
    record(record_property, check_forward(case_of(kind, geom), p_drop))


@pytest.mark.parametrize("p_drop", [0.0, P_DROP], ids=["nodrop", "drop"])
@pytest.mark.parametrize("with_bn", [False, True], ids=["plain", "bn_sums"])
@pytest.mark.parametrize("save16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("geom", ["V4", "V1"])
@pytest.mark.parametrize("kind", sn.SCAN_KINDS)
def test_backward_every_instantiation(kind, geom, save16, with_bn, p_drop, record_property):
    record(record_property, check_backward(case_of(kind, geom), save16, with_bn, p_drop))


@pytest.mark.parametrize("geom", ["V1big", "V1odd"])
@pytest.mark.parametrize("kind", sn.SCAN_KINDS)
def test_backward_under_the_threshold_and_at_an_odd_width(kind, geom, record_property):
    record(record_property, check_backward(case_of(kind, geom), False, True, P_DROP))


RING = [("V4", T) for T in (1, 8, 9, 16)] + [("V1", T) for T in (1, 12, 13, 15, 16, 17, 25)]


@pytest.mark.parametrize("geom,T", RING)
@pytest.mark.parametrize("kind", sn.SCAN_KINDS)
def test_backward_around_the_ring_depths(kind, geom, T, record_property):
    """The fullest variant (BN sums, dropout, g_rate) with T below, at and above every depth of the register ring."""
    record(record_property, check_backward(case_of(kind, geom, T), False, True, P_DROP))


@pytest.mark.parametrize("kind", sn.SCAN_KINDS)
def test_stream_entry_four_neurons_per_thread(kind):
    """sparch_cell_stream_fwd at (33, 15888), as StreamingSNN launches it: chunks of 1, 4 and 1 steps on one carried
    state equal the whole-sequence cell_forward plane, counts and end state, bit for bit."""
    import sparch_amd as sp
    Fn = _Fn()
    B, H, K, chunks = 33, 15888, 4, (1, 4, 1)
    T = sum(chunks)
    assert B * H >= 524288 and H % 4 == 0
    c = sn.scan_case(kind, B, 1, T, H)
    torch.manual_seed(1)
    net = sp.SNN((B, None, K), [H], neuron_type=kind, threshold=c["theta"], dropout=0.0, normalization="batchnorm",
                 use_readout_layer=False)
    lay = net.snn[0]
    rng = np.random.default_rng(3)
    with torch.no_grad():
        for k, v in c["p"].items():
            getattr(lay, k).copy_(torch.from_numpy(v))
        lay.norm.weight.copy_(torch.from_numpy(rng.uniform(0.7, 1.3, H).astype(F32)))
        lay.norm.bias.copy_(torch.from_numpy(rng.uniform(-0.2, 0.2, H).astype(F32)))
        lay.norm.running_mean.copy_(torch.from_numpy(rng.uniform(-0.1, 0.1, H).astype(F32)))
        lay.norm.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, H).astype(F32)))
    st = sp.StreamingSNN(net.to(DEV).eval(), B)
    state = {"u": torch.from_numpy(c["u0"]), "s": torch.from_numpy(c["s0"])}
    if c["w0"] is not None:
        state["w"] = torch.from_numpy(c["w0"])
    st.set_state([state])
    L = st._layers[0]
    assert not L.recurrent and L.Hs == H and L.scale is not None
    Wx = D(c["Wx"])
    whole, count, saved, plane = Fn.cell_forward(kind, Wx, L.scale, L.shift, L.p, D(c["u0"]), D(c["w0"]), D(c["s0"]), B=B,
                                                 dirs=1, theta=c["theta"], p_drop=0.0, seed=0)
    assert saved[0].dtype == torch.float32 and 0.02 <= float(whole.mean()) <= 0.5
    got, got16, t0 = [], [], 0
    for n in chunks:
        s, s16 = st._cell(L, Wx[:, t0:t0 + n].reshape(B * n, H).contiguous(), n, True)
        got.append(s)
        got16.append(s16)
        t0 += n
    Fn.check_status()
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(got, 1), whole) and torch.equal(torch.cat(got16, 1), plane)
    assert torch.equal(L.count, count)
    assert torch.equal(L.u, saved[0][:, -1]) and torch.equal(L.s, whole[:, -1])
    if sn.ADAPTIVE[kind]:
        assert torch.equal(L.w, saved[1][:, -1])
