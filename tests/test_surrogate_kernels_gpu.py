"""
The backward kernels with a smooth surrogate gradient (cell_bwd_pipe_sg_kernel of sparch_amd/csrc/cell.hip,
rec_bwd_sg_kernel of reccell.hip in its persistent and its launch-per-step form) against the fp64 restatement
tests/surrogate_numpy.py, through functional.cell_forward / cell_backward — built as check_backward of
tests/test_scan_kernels_fp64_gpu.py and tests/test_rec_cell_real_V_gpu.py build theirs: the kernel runs on its own
forward saves, the restatement on the same saves.  The forward pass does not depend on the surrogate.

Scales: triangle 2.0, fast_sigmoid 5.0, atan 2.5 (surrogate_numpy.TEST_SCALE).

Bound (never taken from the code under test): per tensor spiking_numpy.bound_of — 4 x the worst max-abs error of two
fp32 runs of the restatement (rows, respectively k blocks, ascending and descending) against its fp64 run on the same
inputs — and every bound is held under spiking_numpy.capped (at most 1e-5 of the reference tensor's max-abs).
tests/test_surrogate_host.py shows that it resolves an ignored scale, a lost abs(), the box-car in the smooth gate's
place and a dropped square by more than four orders of magnitude.  Each test records its worst fraction of the bound.

Conditions: spiking_numpy.scan_conditions (2 .. 50 % spikes, the box-car — the triangle's support at scale 2 — open on
5 .. 95 %, kept and dropped elements with dropout) for the scan cases, 5 .. 70 % spikes and the same open share for the
recurrent ones, on the fp32 restatement's free run and again on the kernel's own saves.

Cases.  Scan: spiking_numpy.SCAN_SHAPES, {LIF, adLIF} x neurons per thread {4, 1} x folded BatchNorm sums x dropout
x the three forms, fp32 saves; SAVE_BF16 with a smooth form keeps fp32 saves.  Recurrent, persistent: REC_SHAPES whole
sequence in the drive regime (every form at H 132 and 1024, one per other shape), chunks of 1 and 4 steps and the bf16
operand mode at H 132 and 1024, two directions with scale / shift and g_rate; dV's diagonal exactly 0.  The
launch-per-step path at (33, 1, 6, 132).  Every form's dWx differs from the box-car kernel's and from the other forms'
by more than 1000 x the bound.  An SNN trains: same forward bit for bit, other gradients, finite Adam steps, run_exp.py.
"""
import functools
import logging

import numpy as np
import pytest
import torch

from tests import spiking_numpy as sn
from tests import surrogate_numpy as sg
from tests.kit import DEV, F32, F64, SEED, N, bf16_mode, record, within  # noqa: F401  (bf16_mode: a fixture)
from tests.kit import Fn as _Fn
from tests.spiking_cases import GEOM, collect, rec_case, scan_forward
from tests.spiking_cases import scan_case_of as case_of

pytestmark = pytest.mark.gpu

P_DROP = sn.P_DROP
FORMS = [(name, sg.TEST_SCALE[name]) for name in sg.SMOOTH]
form_id = lambda f: f[0] if isinstance(f, tuple) else None  # noqa: E731


def held(got, kind, with_bn, bw):
    """bw(dtype, order) is the restatement on the case; the rule of the module docstring.  Returns (worst fraction of
    the bound, the bounds, the fp64 reference)."""
    ref = bw(F64, None)
    names = sn.bwd_tensors(kind, with_bn)
    assert set(names) == set(got), (names, sorted(got))
    bound = sn.capped(sn.bound_of([bw(F32, "asc"), bw(F32, "desc")], ref, names), ref, names)
    return max(within(got[k], ref[k], bound[k], k) for k in names), bound, ref


# ------------------------------------------------------------------------------------------------ scan kernels
@functools.lru_cache(maxsize=2)
def scan_saves(kind, geom, p_drop):
    """The forward kernel's saves of a scan case: made once, shared by the forms (the forward has no surrogate)."""
    c = case_of(kind, geom)
    _, _, saved, _ = scan_forward(c, p_drop, surrogate=FORMS[0])
    assert saved[0].dtype == torch.float32
    sn.scan_conditions(c, N(saved[0]), c["keep"] if p_drop else None)      # on the kernel's own saves too
    return saved, N(saved[0]), N(saved[1])


def scan_kernel(c, saved, with_bn, p_drop, form):
    Fn, d = _Fn(), c["dev"]
    dWx, grads = Fn.cell_backward(c["kind"], d["g_out"], d["g_rate"], d["p"], d["u0"], d["w0"], d["s0"], saved, B=c["B"],
                                  dirs=c["dirs"], T=c["T"], H=c["H"], theta=c["theta"], p_drop=p_drop, seed=SEED,
                                  bn=d["bn"] if with_bn else None, surrogate=form)
    Fn.check_status()
    torch.cuda.synchronize()
    return collect(dWx, grads, with_bn)


def scan_restated(c, us, ws, with_bn, p_drop, form):
    def bw(dt, ro):
        return sn.flat(sg.backward(c["kind"], dt, c["g_out"], c["g_rate"], us, ws, c["p"], c["u0"], c["w0"], c["s0"],
                                   B=c["B"], dirs=c["dirs"], surrogate=form, theta=c["theta"],
                                   bn=c["bn"] if with_bn else None, keep=c["keep"] if p_drop else None, row_order=ro))
    return bw


def check_scan(kind, geom, with_bn, p_drop, form):
    c = case_of(kind, geom)                                 # (its conditions hold on the restatement's free run)
    saved, us, ws = scan_saves(kind, geom, p_drop)
    got = scan_kernel(c, saved, with_bn, p_drop, form)
    worst, _, _ = held(got, kind, with_bn, scan_restated(c, us, ws, with_bn, p_drop, form))
    for k in c["p"]:                                        # neuron 0 below, neuron 1 above the clamp range
        assert got[k][0] == 0 and got[k][1] == 0 and np.abs(got[k][2:]).max() > 0, k
    return worst


@pytest.mark.parametrize("form", FORMS, ids=form_id)
@pytest.mark.parametrize("p_drop", [0.0, P_DROP], ids=["nodrop", "drop"])
@pytest.mark.parametrize("with_bn", [False, True], ids=["plain", "bn_sums"])
@pytest.mark.parametrize("geom", ["V4", "V1"])
@pytest.mark.parametrize("kind", sn.SCAN_KINDS)
def test_scan_backward_every_instantiation(kind, geom, with_bn, p_drop, form, record_property):
    assert set(GEOM) == {"V4", "V1", "V1big", "V1odd"}
    record(record_property, check_scan(kind, geom, with_bn, p_drop, form))


@pytest.mark.parametrize("form", FORMS, ids=form_id)
@pytest.mark.parametrize("geom", ["V1big", "V1odd"])
@pytest.mark.parametrize("kind", sn.SCAN_KINDS)
def test_scan_backward_under_the_threshold_and_at_an_odd_width(kind, geom, form, record_property):
    record(record_property, check_scan(kind, geom, True, P_DROP, form))


def test_bf16_saves_are_not_taken_with_a_smooth_surrogate():
    Fn = _Fn()
    c = case_of("adLIF", "V1")
    _, _, boxed, _ = scan_forward(c, 0.0, save16=True)
    _, _, smooth, _ = scan_forward(c, 0.0, save16=True, surrogate=FORMS[1])
    _, _, plain, _ = scan_forward(c, 0.0)
    assert boxed[0].dtype == boxed[1].dtype == torch.bfloat16
    assert smooth[0].dtype == smooth[1].dtype == torch.float32
    assert torch.equal(smooth[0], plain[0]) and torch.equal(smooth[1], plain[1])
    assert not Fn.SAVE_BF16
    # and the entry point itself refuses the combination
    d = c["dev"]
    with pytest.raises(ValueError, match="sparch_cell_bwd_sg"):
        Fn.cell_backward(c["kind"], d["g_out"], d["g_rate"], d["p"], d["u0"], d["w0"], d["s0"], boxed, B=c["B"],
                         dirs=c["dirs"], T=c["T"], H=c["H"], theta=c["theta"], p_drop=0.0, seed=0, surrogate=FORMS[1])
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ recurrent kernels
def rec_forward(c, spl):
    Fn, d = _Fn(), c["dev"]
    assert not Fn.SAVE_BF16
    _, _, saved, _ = Fn.cell_forward(c["kind"], d["Wx"], d["scale"], d["shift"], d["p"], d["u0"], d["w0"], d["s0"], B=c["B"],
                                     dirs=c["dirs"], theta=c["theta"], p_drop=0.0, seed=0, steps_per_launch=spl,
                                     surrogate=FORMS[0])
    Fn.check_status()
    torch.cuda.synchronize()
    return saved


def rec_conditions(c, u_save):
    x = np.asarray(u_save, dtype=F32) - F32(c["theta"])
    spikes, box = float((x > 0).mean()), float(((x > F32(-0.5)) & (x <= F32(0.5))).mean())
    assert 0.05 <= spikes <= 0.7, ("spike fraction", spikes)
    assert 0.05 <= box <= 0.95, ("box-car open share", box)


def rec_kernel(c, saved, spl, form, with_rate):
    Fn, d = _Fn(), c["dev"]
    dWx, grads = Fn.cell_backward(c["kind"], d["g_out"], d["g_rate"] if with_rate else None, d["p"], d["u0"], d["w0"],
                                  d["s0"], saved, B=c["B"], dirs=c["dirs"], T=c["T"], H=c["H"], theta=c["theta"],
                                  p_drop=0.0, seed=0, steps_per_launch=spl, surrogate=form)
    Fn.check_status()
    torch.cuda.synchronize()
    return collect(dWx, grads, False)


def rec_restated(c, us, ws, form, with_rate, operand, rec_operand):
    def bw(dt, ko):
        return sn.flat(sg.backward(c["kind"], dt, c["g_out"], c["g_rate"] if with_rate else None, us, ws, c["p"], c["u0"],
                                   c["w0"], c["s0"], B=c["B"], dirs=c["dirs"], surrogate=form, theta=c["theta"],
                                   k_order=ko, operand=operand, rec_operand=rec_operand))
    return bw


def check_rec(c, spl, form, operand=None, with_rate=False):
    """Returns the worst fraction of the bound."""
    free = sn.forward(c["kind"], F32, c["Wx"], c["scale"], c["shift"], c["p"], c["u0"], c["w0"], c["s0"], B=c["B"],
                      dirs=c["dirs"], theta=c["theta"], operand=operand)
    rec_conditions(c, free["u_save"])
    saved = rec_forward(c, spl)
    us, ws = N(saved[0]), N(saved[1])
    rec_conditions(c, us)
    got = rec_kernel(c, saved, spl, form, with_rate)
    # (bf16 operand mode: the dense products of the reference read the kernel's own dWx, rounded as the kernel rounds it)
    rec_operand = got["dWx"] if operand is not None else None
    worst, _, _ = held(got, c["kind"], False, rec_restated(c, us, ws, form, with_rate, operand, rec_operand))
    assert np.all(np.diag(got["V"]) == 0) and np.abs(got["V"]).max() > 0
    return worst


# every form at H 132 and 1024, one form (rotating) at H 96 and 384
WHOLE = [(shape, FORMS[i % 3]) for i, shape in enumerate(s for s in sn.REC_SHAPES if s[4] in (96, 384))] \
    + [(shape, form) for shape in sn.REC_SHAPES if shape[4] in (132, 1024) for form in FORMS]
CHUNKED = [((k, 33, 1, 6, H), spl, FORMS[i % 3])
           for i, (H, k, spl) in enumerate((H, k, spl) for H in (132, 1024) for k in ("RLIF", "RadLIF") for spl in (1, 4))]
BF16 = [((k, 33, 1, 6, H), FORMS[(i + 1) % 3]) for i, (H, k) in enumerate((H, k) for H in (132, 1024) for k in ("RLIF", "RadLIF"))]
shape_id = lambda v: "-".join(map(str, v)) if isinstance(v, tuple) and len(v) == 5 else form_id(v)  # noqa: E731


@pytest.mark.parametrize("shape,form", WHOLE, ids=shape_id)
def test_recurrent_backward_whole_sequence(shape, form, record_property):
    record(record_property, check_rec(rec_case(*shape, "drive"), None, form))


@pytest.mark.parametrize("shape,spl,form", CHUNKED, ids=shape_id)
def test_recurrent_backward_in_chunks_of_steps(shape, spl, form, record_property):
    assert {f for _, _, f in CHUNKED} == set(FORMS)
    record(record_property, check_rec(rec_case(*shape, "drive"), spl, form))


@pytest.mark.parametrize("form", FORMS[:2], ids=form_id)
@pytest.mark.parametrize("shape", sn.BIDIR_SHAPES, ids=shape_id)
def test_recurrent_backward_two_directions_with_scale_shift_and_rate_gradient(shape, form, record_property):
    record(record_property, check_rec(rec_case(*shape, "drive"), None, form, with_rate=True))


@pytest.mark.parametrize("shape,form", BF16, ids=shape_id)
def test_recurrent_backward_bf16_operand_mode(shape, form, bf16_mode, record_property):  # noqa: F811
    assert bf16_mode.compute_dtype() == "bf16" and {f for _, f in BF16} == set(FORMS)
    record(record_property, check_rec(rec_case(*shape, "drive"), None, form, operand=sn.bf16_round))


@pytest.mark.parametrize("kind,form", [("RLIF", FORMS[2]), ("RadLIF", FORMS[1])], ids=form_id)
def test_launch_per_step_path(kind, form, monkeypatch, record_property):
    monkeypatch.setenv("SPARCH_REC_STEP_PATH", "1")
    assert _Fn().rec_step_path(132)
    record(record_property, check_rec(rec_case(kind, 33, 1, 6, 132, "drive"), None, form, with_rate=True))


# ------------------------------------------------------------------------------------------------ telling them apart
def apart(dwx, bounds):
    """dwx: {name: dWx of the kernel under that surrogate, on the same saves}; every pair differs by more than 1000 x
    the (larger) bound.  Returns the smallest ratio."""
    names = list(dwx)
    smallest = float("inf")
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            ratio = float(np.abs(dwx[a].astype(F64) - dwx[b]).max()) / max(bounds.get(a, 0.0), bounds.get(b, 0.0))
            print(f"  {a} vs {b}: {ratio:.3g} x the bound")
            assert ratio > 1000, (a, b, ratio)
            smallest = min(smallest, ratio)
    return smallest


def test_scan_kernel_tells_the_surrogates_apart(record_property):
    kind, geom = "adLIF", "V1"
    c = case_of(kind, geom)
    saved, us, ws = scan_saves(kind, geom, 0.0)
    dwx, bounds = {"boxcar": scan_kernel(c, saved, False, 0.0, None)["dWx"]}, {}
    assert np.array_equal(dwx["boxcar"], scan_kernel(c, saved, False, 0.0, ("boxcar", None))["dWx"])
    for form in FORMS:
        got = scan_kernel(c, saved, False, 0.0, form)
        _, bound, _ = held(got, kind, False, scan_restated(c, us, ws, False, 0.0, form))
        dwx[form[0]], bounds[form[0]] = got["dWx"], bound["dWx"]
    record_property("smallest_difference_over_bound", round(apart(dwx, bounds), 1))


def test_recurrent_kernel_tells_the_surrogates_apart(record_property):
    c = rec_case("RadLIF", 33, 1, 6, 132, "drive")
    saved = rec_forward(c, None)
    us, ws = N(saved[0]), N(saved[1])
    dwx, bounds = {"boxcar": rec_kernel(c, saved, None, None, False)["dWx"]}, {}
    for form in FORMS:
        got = rec_kernel(c, saved, None, form, False)
        _, bound, _ = held(got, c["kind"], False, rec_restated(c, us, ws, form, False, None, None))
        dwx[form[0]], bounds[form[0]] = got["dWx"], bound["dWx"]
    record_property("smallest_difference_over_bound", round(apart(dwx, bounds), 1))


# ------------------------------------------------------------------------------------------------ network level
B_NET, T_NET, K_NET, H_NET, C_NET = 8, 12, 40, 64, 10


def network(**kw):
    import sparch_amd as sp
    torch.manual_seed(11)
    # (threshold 0.1: at the default 1.0 these twelve steps of a normalised projection leave 0.8 % spikes)
    return sp.SNN((B_NET, None, K_NET), [H_NET, H_NET, C_NET], neuron_type="RadLIF", threshold=0.1, dropout=0.1,
                  normalization="batchnorm", **kw).to(DEV).train()


def one_step(net):
    """Forward and backward of a fixed batch with fixed initial-state draws: (out, rates, {name: grad})."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B_NET, T_NET, K_NET, generator=g).to(DEV)
    y = torch.randint(0, C_NET, (B_NET,), generator=g).to(DEV)
    torch.manual_seed(7)
    out, rates = net(x)
    loss = torch.nn.functional.cross_entropy(out, y) + rates.sum()
    net.zero_grad()
    loss.backward()
    _Fn().check_status()
    torch.cuda.synchronize()
    return out.detach().clone(), rates.detach().clone(), {k: p.grad.detach().clone() for k, p in net.named_parameters()}


@functools.lru_cache(maxsize=1)
def boxcar_step():
    return one_step(network())


def test_network_explicit_boxcar_is_the_default_network():
    out, rates, grads = one_step(network(surrogate="boxcar"))
    out0, rates0, grads0 = boxcar_step()
    assert 0.01 < float(rates0.mean()) < 0.9
    assert torch.equal(out, out0) and torch.equal(rates, rates0) and set(grads) == set(grads0)
    for k in grads0:
        assert torch.equal(grads[k], grads0[k]), k


@pytest.mark.parametrize("name", sg.SMOOTH)
def test_network_with_a_smooth_surrogate(name):
    import sparch_amd as sp
    net = network(surrogate=name)
    assert net.snn[0]._surrogate() == (name, sg.DEFAULT_SCALE[name])
    out, rates, grads = one_step(net)
    out0, rates0, grads0 = boxcar_step()
    assert torch.equal(out, out0) and torch.equal(rates, rates0)            # the forward does not change
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert not torch.equal(grads["snn.0.W.weight"], grads0["snn.0.W.weight"])
    assert float(grads["snn.0.W.weight"].abs().max()) > 0
    opt = sp.optim.Adam(net.parameters(), 1e-3)
    g = torch.Generator().manual_seed(6)
    for _ in range(3):
        x = torch.randn(B_NET, T_NET, K_NET, generator=g).to(DEV)
        y = torch.randint(0, C_NET, (B_NET,), generator=g).to(DEV)
        out, rates = net(x)
        loss = torch.nn.functional.cross_entropy(out, y)
        opt.zero_grad()
        loss.backward()
        opt.step()
        assert bool(torch.isfinite(loss.detach()))
    _Fn().check_status()
    assert all(bool(torch.isfinite(p).all()) for p in net.parameters())


def test_run_exp_reads_sparch_surrogate(tmp_path, monkeypatch, caplog):
    import run_exp
    monkeypatch.setenv("SPARCH_SURROGATE", "atan:2.5")
    caplog.set_level(logging.INFO)
    torch.manual_seed(3)
    run_exp.main(["--model_type", "RLIF", "--nb_layers", "3", "--nb_hiddens", "64", "--dataset_name", "shd",
                  "--batch_size", "8", "--nb_epochs", "1", "--synthetic", "1", "--synthetic_batches", "2", "--save_best",
                  "0", "--new_exp_folder", str(tmp_path / "exp_sg")])
    text = "\n".join(r.getMessage() for r in caplog.records)
    assert "Surrogate gradient: atan, scale 2.5 (SPARCH_SURROGATE)" in text
    assert "surrogate=atan, surrogate_scale=2.5" in text and "Epoch 1: train loss=" in text
    caplog.clear()
    run_exp.main(["--model_type", "MLP", "--nb_layers", "3", "--nb_hiddens", "64", "--dataset_name", "shd",
                  "--batch_size", "8", "--nb_epochs", "1", "--synthetic", "1", "--synthetic_batches", "2", "--save_best",
                  "0", "--new_exp_folder", str(tmp_path / "exp_mlp")])
    assert "SPARCH_SURROGATE is ignored: MLP has no spike function" in "\n".join(r.getMessage() for r in caplog.records)
