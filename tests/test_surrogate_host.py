"""
The selectable surrogate gradient, without a GPU:

  * tests/surrogate_numpy.py (the reverse pass with the gate as a parameter) equals spiking_numpy.backward bit for bit in
    fp32 with the box-car, and in float64 matches torch autograd of a plain-torch step loop through
    snns.SpikeFunctionSurrogate at 1e-10 of each tensor's max-abs: four kinds x three smooth forms at (Bp, T, H) = (5, 6, 12);
  * sharpness of the bound tests/test_surrogate_kernels_gpu.py holds the kernels to (4 x the worst error of two fp32
    runs of the restatement against its fp64 run): a scale that is ignored, abs(x) replaced by x (atan: x shifted by
    0.125), the box-car in place of the smooth gate and a dropped square each leave it behind by at least 1000 x on dWx
    and on alpha (the triangle has no square to drop);
  * SNN / layer constructors, SPARCH_SURROGATE parsing, refusals, defaults (the three scales at which the gate's area is
    the box-car's), pickling, the reference's checkpoint;
  * the three `_sg` entry points' refusals (the style of tests/test_rec_entry_validation_host.py), ABI version 5;
  * with the recording stand-in of tools/layer_call_trace.py: a layer with ("fast_sigmoid", 5.0) issues the `_sg`
    backward with (2, 5.0) and otherwise the box-car's calls; the committed trace is unchanged.
"""
import io
import math
import os
import pickle

import numpy as np
import pytest
import torch

from tests import spiking_numpy as sn
from tests import surrogate_numpy as sg
from tests.entry_probes import KIND, MIS, NAN, RLIF, WS, Entry, P, T, head, ptrs
from tests.kit import EALIGN, EINVAL, EWORKSPACE, F32, F64
from tools.layer_call_trace import traced


# ------------------------------------------------------------------------------------------------ the restatement
def free_saves(c):
    f = sn.forward(c["kind"], F32, c["Wx"], c["scale"], c["shift"], c["p"], c["u0"], c["w0"], c["s0"], B=c["B"],
                   dirs=c["dirs"], theta=c["theta"])
    return f["u_save"], f["w_save"]


def scan_inputs(kind, B, dirs, T_, H):
    c = sn.scan_case(kind, B, dirs, T_, H)
    c["keep"] = None
    return c


def rec_inputs(kind, B, dirs, T_, H):
    c = sn.make_inputs(kind, B, dirs, T_, H, sn.case_seed(kind, B, dirs, T_, H), "drive")
    c["bn"] = c["keep"] = None
    return c


def run(mod, c, dtype, saves, **kw):
    return sn.flat(mod.backward(c["kind"], dtype, c["g_out"], c["g_rate"], saves[0], saves[1], c["p"], c["u0"], c["w0"],
                                c["s0"], B=c["B"], dirs=c["dirs"], theta=c["theta"], bn=c["bn"], **kw))


@pytest.mark.parametrize("make,shape", [(scan_inputs, ("adLIF", 33, 2, 17, 100)), (rec_inputs, ("RadLIF", 33, 1, 6, 132))],
                         ids=["scan", "recurrent"])
def test_boxcar_restatement_is_spiking_numpy_bit_for_bit(make, shape):
    c = make(*shape)
    saves = free_saves(c)
    for order in ({"row_order": "asc"}, {"row_order": "desc", "k_order": "desc"}):
        a, b = run(sn, c, F32, saves, **order), run(sg, c, F32, saves, surrogate=("boxcar", None), **order)
        assert set(a) == set(b)
        for k in a:
            if k != "bn_sums":
                assert a[k].dtype == b[k].dtype == F32 and np.array_equal(a[k], b[k]), k


def torch_reference(c, name, scale):
    """A plain-torch float64 step loop of the cell (spiking_numpy's forward relations) through SpikeFunctionSurrogate;
    returns the saves it made and the autograd gradients of sum(s_out g_out) + sum(rate g_rate)."""
    from sparch_amd.snns import SpikeFunctionSurrogate
    kind, Bp, T_, H, theta = c["kind"], c["Bp"], c["T"], c["H"], c["theta"]
    adaptive, recurrent = sn.ADAPTIVE[kind], sn.RECURRENT[kind]
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=F64))  # noqa: E731
    raw = {k: t64(v).requires_grad_(True) for k, v in c["p"].items()}
    lim = lambda k: torch.clamp(raw[k], float(sn.LIMS[k][0]), float(sn.LIMS[k][1]))  # noqa: E731
    alpha = lim("alpha")
    beta, a, b = (lim("beta"), lim("a"), lim("b")) if adaptive else (None, None, None)
    Vm = raw["V"] * (1 - torch.eye(H, dtype=torch.float64)) if recurrent else None
    Wx = t64(c["Wx"]).requires_grad_(True)
    u, s = t64(c["u0"]), t64(c["s0"])
    w = t64(c["w0"]) if adaptive else None
    U, W, S = [], [], []
    for t in range(T_):
        drive = Wx[:, t]
        if adaptive:
            w = (beta * w + a * u) + b * s
        if recurrent:
            drive = drive + s @ Vm
        if adaptive:
            drive = drive - w
        u = alpha * (u - s) + (1 - alpha) * drive
        s = SpikeFunctionSurrogate.apply(u - theta, name, scale)
        U.append(u)
        W.append(w)
        S.append(s)
    s_out = torch.stack(S, 1)
    loss = (s_out * t64(c["g_out"])).sum() + (s_out.mean((0, 1)) * t64(c["g_rate"])).sum()
    loss.backward()
    got = {"dWx": Wx.grad.numpy()}
    got.update({k: v.grad.numpy() for k, v in raw.items()})
    us = torch.stack(U, 1).detach().numpy()
    ws = torch.stack(W, 1).detach().numpy() if adaptive else None
    assert 0.02 <= float(s_out.detach().mean()) <= 0.9
    return (us, ws), got


@pytest.mark.parametrize("name", sg.SMOOTH)
@pytest.mark.parametrize("kind", sn.KINDS)
def test_restatement_is_torch_autograd_in_float64(kind, name):
    c = sn.make_inputs(kind, 5, 1, 6, 12, 77 + len(kind), "drive")
    c["bn"] = None
    scale = sg.TEST_SCALE[name]
    saves, want = torch_reference(c, name, scale)
    got = run(sg, c, F64, saves, surrogate=(name, scale))
    for k in sn.bwd_tensors(kind):
        top = np.abs(want[k]).max()
        assert top > 0 and np.abs(got[k] - want[k]).max() <= 1e-10 * top, (k, float(np.abs(got[k] - want[k]).max() / top))


def test_spike_function_surrogate_is_generic_in_dtype_and_boxcar_is_the_old_function():
    from sparch_amd.snns import SpikeFunctionBoxcar, SpikeFunctionSurrogate
    x = torch.tensor([-0.75, -0.5, -0.25, 0.0, 0.25, 0.5, 0.75])
    g = torch.arange(1.0, 8.0)
    for dt in (torch.float32, torch.float64):
        for name in sg.SMOOTH:
            k = sg.TEST_SCALE[name]
            xv = x.to(dt).clone().requires_grad_(True)
            s = SpikeFunctionSurrogate.apply(xv, name, k)
            assert s.dtype == dt and torch.equal(s, (x > 0).to(dt))
            s.backward(g.to(dt))
            want = sg.gate(name, k, g.to(dt).numpy(), x.to(dt).numpy())
            assert xv.grad.dtype == dt and np.array_equal(xv.grad.numpy(), want), (name, dt)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    SpikeFunctionSurrogate.apply(xa, "boxcar", None).backward(g)
    SpikeFunctionBoxcar.apply(xb).backward(g)
    assert torch.equal(xa.grad, xb.grad) and torch.equal(xa.grad, torch.tensor([0.0, 0, 3, 4, 5, 6, 0]))
    nan = torch.tensor([float("nan")], requires_grad=True)
    for name in sg.SMOOTH:                      # plain multiplications: a NaN x propagates
        nan.grad = None
        SpikeFunctionSurrogate.apply(nan, name, 1.0).backward(torch.ones(1))
        assert torch.isnan(nan.grad).all(), name


def test_areas_and_default_scales():
    from sparch_amd import snns
    x = np.linspace(-200, 200, 1_600_001)
    for name in sg.SMOOTH:
        k = sg.DEFAULT_SCALE[name]
        assert snns.SURROGATE_DEFAULT_SCALE[name] == k and snns.resolve_surrogate(name) == (name, k)
        assert sg.AREA[name](k) == pytest.approx(1.0, abs=1e-15)
        for kk in (k, sg.TEST_SCALE[name]):
            y = sg.gate(name, kk, np.ones_like(x), x)
            assert y.max() == 1.0 and y[x == 0] == 1.0
            area = float(((y[1:] + y[:-1]) * 0.5 * np.diff(x)).sum())
            # what lies beyond +-200, analytically: 2 / (k (1 + 200 k)) and 2 (pi / 2 - atan(200 k)) / k
            tail = {"triangle": 0.0, "fast_sigmoid": 2 / (kk * (1 + kk * 200)),
                    "atan": 2 * (math.pi / 2 - math.atan(200 * kk)) / kk}[name]
            assert area + tail == pytest.approx(sg.AREA[name](kk), rel=1e-6), (name, kk)


SHARP = [("LIF", 33, 1, 17, 99), ("adLIF", 33, 2, 17, 100), ("RLIF", 33, 1, 6, 96), ("RadLIF", 33, 1, 6, 132)]


@pytest.mark.parametrize("shape", SHARP, ids=lambda s: s[0])
def test_the_bound_resolves_every_mutated_gate(shape):
    c = (rec_inputs if sn.RECURRENT[shape[0]] else scan_inputs)(*shape)
    saves = free_saves(c)
    smallest = float("inf")
    for name in sg.SMOOTH:
        s = (name, sg.TEST_SCALE[name])
        ref = run(sg, c, F64, saves, surrogate=s)
        runs32 = [run(sg, c, F32, saves, surrogate=s, row_order="asc", k_order="asc"),
                  run(sg, c, F32, saves, surrogate=s, row_order="desc", k_order="desc")]
        bound = sn.capped(sn.bound_of(runs32, ref, ("dWx", "alpha")), ref, ("dWx", "alpha"))
        for m in sg.mutants_of(name):
            mut = run(sg, c, F64, saves, surrogate=s, mutant=m)
            for k in ("dWx", "alpha"):
                ratio = float(np.abs(mut[k] - ref[k]).max()) / bound[k]
                smallest = min(smallest, ratio)
                assert ratio >= 1000, (name, m, k, ratio)
    print(f"  smallest mutant error / bound: {smallest:.3g}")


# ------------------------------------------------------------------------------------------------ the Python surface
def test_constructors_defaults_and_refusals():
    import sparch_amd as sp
    from sparch_amd import snns
    net = sp.SNN((4, None, 12), [8, 8, 3], neuron_type="RadLIF")
    assert (net.surrogate, net.surrogate_scale) == ("boxcar", None) and "surrogate" not in repr(net)
    assert all(l._surrogate() is None and l.spike_fct == snns.SpikeFunctionBoxcar.apply for l in net.snn[:-1])
    for name, k in (("triangle", 1.0), ("fast_sigmoid", 2.0), ("atan", math.pi)):
        net = sp.SNN((4, None, 12), [8, 8, 3], neuron_type="adLIF", surrogate=name)
        assert (net.surrogate, net.surrogate_scale) == (name, k)
        for l in net.snn[:-1]:
            assert (l.surrogate, l.surrogate_scale) == (name, k) and l._surrogate() == (name, k)
            x = torch.tensor([0.1], dtype=torch.float64, requires_grad=True)
            l.spike_fct(x).backward(torch.ones(1, dtype=torch.float64))
            assert x.grad.numpy() == sg.gate(name, k, np.ones(1), np.array([0.1]))
        assert f"surrogate={name}" in repr(net) and not hasattr(net.snn[-1], "surrogate")
    net = sp.SNN((4, None, 12), [8, 3], neuron_type="LIF", surrogate="fast_sigmoid", surrogate_scale=5)
    assert net.snn[0]._surrogate() == ("fast_sigmoid", 5.0) and "surrogate_scale=5" in repr(net.snn[0])
    for cls in (sp.LIFLayer, sp.adLIFLayer, sp.RLIFLayer, sp.RadLIFLayer):
        assert cls(12, 8, 4, surrogate="atan", surrogate_scale=2.5)._surrogate() == ("atan", 2.5)
        assert cls(12, 8, 4)._surrogate() is None
    for bad in (dict(surrogate="sigmoid"), dict(surrogate="triangle", surrogate_scale=0.0),
                dict(surrogate="atan", surrogate_scale=-1.0), dict(surrogate="atan", surrogate_scale=float("nan")),
                dict(surrogate="atan", surrogate_scale=float("inf")), dict(surrogate="boxcar", surrogate_scale=1.0)):
        for make in (lambda kw: sp.SNN((4, None, 12), [8, 3], **kw), lambda kw: sp.RLIFLayer(12, 8, 4, **kw)):
            with pytest.raises(ValueError, match="boxcar, triangle, fast_sigmoid, atan"):
                make(bad)


def test_sparch_surrogate_parsing():
    from sparch_amd.snns import parse_surrogate
    assert parse_surrogate("fast_sigmoid:5") == ("fast_sigmoid", 5.0)
    assert parse_surrogate(" atan : 2.5 ") == ("atan", 2.5)
    assert parse_surrogate("triangle") == ("triangle", 1.0) and parse_surrogate("atan") == ("atan", math.pi)
    assert parse_surrogate("boxcar") == ("boxcar", None)
    for bad in ("sigmoid", "atan:", "atan:fast", "atan:0", "atan:-2", "atan:nan", "boxcar:1", ":2", "atan:1:2"):
        with pytest.raises(ValueError):
            parse_surrogate(bad)


def test_experiment_refuses_a_malformed_value_before_anything_else(monkeypatch, tmp_path):
    """Experiment parses SPARCH_SURROGATE first: no folder is made, no device or data is asked for."""
    import argparse

    from sparch_amd.exp import Experiment
    monkeypatch.setenv("SPARCH_SURROGATE", "atan:fast")
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="SPARCH_SURROGATE|malformed surrogate"):
        Experiment(argparse.Namespace(model_type="RLIF"))
    assert not os.listdir(tmp_path)


def test_pickle_round_trip_and_older_checkpoints():
    import sparch_amd as sp
    from tests.golden_io import GOLDEN
    net = sp.SNN((4, None, 12), [8, 8, 3], neuron_type="RadLIF", surrogate="fast_sigmoid", surrogate_scale=5.0)
    buf = io.BytesIO()
    torch.save(net, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert (back.surrogate, back.surrogate_scale) == ("fast_sigmoid", 5.0)
    assert all(l._surrogate() == ("fast_sigmoid", 5.0) for l in back.snn[:-1]) and repr(back) == repr(net)
    assert pickle.loads(pickle.dumps(net.snn[0]))._surrogate() == ("fast_sigmoid", 5.0)
    # the reference's own pickle, and ours from before the setting existed: no such attributes, read as box-car
    ref = torch.load(os.path.join(GOLDEN, "ref_checkpoint_RadLIF.pth"), weights_only=False)
    assert not hasattr(ref, "surrogate") and all(not hasattr(l, "surrogate") for l in ref.snn)
    assert all(l._surrogate() is None for l in ref.snn[:-1]) and "surrogate" not in repr(ref)
    old = sp.RLIFLayer(12, 8, 4)
    del old.surrogate, old.surrogate_scale
    assert old._surrogate() is None and "surrogate" not in repr(old)


# ------------------------------------------------------------------------------------------------ the C ABI
SG = [("surrogate", 2), ("surrogate_scale", 5.0)]
LIF_K, ADLIF_K = 0, 1
CELL_SG = Entry("sparch_cell_bwd_sg", head(("kind", ADLIF_K)) + ptrs("g_out g_rate u_save w_save", "g_rate") + [("save_bf16", 0)]
                + ptrs("alpha beta a b u0 w0 s0") + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)]
                + ptrs("dWx dparam_ws bn_x bn_mean bn_invstd", "bn_x bn_mean bn_invstd") + SG + [("stream", None)])
REC_SG = Entry("sparch_rec_cell_bwd_sg", head(KIND) + ptrs("g_out g_rate u_save w_save", "g_rate") + [("save_bf16", 0)]
               + ptrs("alpha beta a b vpack_t u0 w0 s0") + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)]
               + ptrs("dWx s_prev16 dparam_ws bn_x bn_mean bn_invstd", "bn_x bn_mean bn_invstd") + WS[:-1] + SG
               + [("stream", None), ("precision", 0)])
STEP_SG = Entry("sparch_rec_cell_step_bwd_sg", head(KIND, "t")
                + ptrs("g_out g_rate u_save w_save alpha beta a b rec u0 w0 s0", "g_rate")
                + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)]
                + ptrs("dWx s_prev16 dparam_ws bn_x bn_mean bn_invstd dwx_step", "bn_x bn_mean bn_invstd") + SG
                + [("stream", None)])
SG_ENTRIES = (CELL_SG, REC_SG, STEP_SG)
ids = lambda e: e.name  # noqa: E731


def test_abi_is_additive():
    from sparch_amd._capi import PROTOTYPES, lib
    assert lib.sparch_abi_version() == 5
    for e, sibling in zip(SG_ENTRIES, ("sparch_cell_bwd", "sparch_rec_cell_bwd", "sparch_rec_cell_step_bwd")):
        assert len(e.args) == len(PROTOTYPES[e.name][1]) == len(PROTOTYPES[sibling][1]) + 2, e.name
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sparch_hip.h")) as f:
        header = f.read()
    for name, v in (("BOXCAR", 0), ("TRIANGLE", 1), ("FAST_SIGMOID", 2), ("ATAN", 3)):
        assert f"#define SPARCH_SURROGATE_{name} {v}\n" in header and sg.IDS[name.lower()] == v
    for e in SG_ENTRIES:
        assert f"int {e.name}(" in header


@pytest.mark.parametrize("e", SG_ENTRIES, ids=ids)
def test_sg_entries_refuse_before_any_device_work(e):
    """Nothing here reaches a launch: the persistent entry ends at its workspace check (chan = NULL), the other two are
    only ever called with something broken."""
    for bad in (-1, 4, 7):
        assert e(surrogate=bad) == EINVAL, bad
    for sid in (1, 2, 3):
        for k in (0.0, -1.0, NAN, float("inf"), -float("inf")):
            assert e(surrogate=sid, surrogate_scale=k) == EINVAL, (sid, k)
    if any(k == "save_bf16" for k, _ in e.args):
        for sid in (1, 2, 3):
            assert e(surrogate=sid, save_bf16=1) == EINVAL, sid
    # the surrogate is checked first: in front of the alignment check, like every other SPARCH_EINVAL
    assert e(surrogate=9, g_out=MIS) == EINVAL and e(surrogate=2, surrogate_scale=0.0, g_out=MIS) == EINVAL
    # the sibling's own refusals still hold behind it, with a smooth form and with the box-car (any scale: ignored)
    for over in (dict(), dict(surrogate=0, surrogate_scale=NAN), dict(surrogate=0, surrogate_scale=-3.0)):
        assert e(B=0, **over) == EINVAL and e(g_out=None, **over) == EINVAL and e(p_drop=1.0, **over) == EINVAL
        assert e(g_out=MIS, **over) == EALIGN and e(dWx=MIS, **over) == EALIGN
        assert e(bn_x=P, **over) == EINVAL
    assert e(kind=7) == EINVAL and e(kind=(RLIF if e is CELL_SG else LIF_K)) == EINVAL
    if e is REC_SG:
        for over in (dict(), dict(surrogate=0, surrogate_scale=0.0), dict(surrogate=0, save_bf16=1), dict(surrogate=3)):
            assert e(**over) == EWORKSPACE, over         # a valid call up to its workspace: chan is NULL
        assert e(precision=7) == EINVAL
    if e is STEP_SG:
        assert e(t=0, rec=None) == EINVAL and e(t=T) == EINVAL and e(t=-1) == EINVAL


# ------------------------------------------------------------------------------------------------ the calls issued
def layer_case(kind, sgate, **kw):
    def run(lct):
        with lct._env(**kw.get("env", {})):         # (the tracer clears the switches around the cases: set inside)
            x, xcfg = lct._input("dense", 4, 3, 32, True)
            s, rate, _ = lct._spiking(x, dict(xcfg, **({} if sgate is None else {"surrogate": sgate})), kind, "batchnorm",
                                      kw.get("dirs", 1), 128)
            lct._backward(s, rate)
    return run


def cell_case(kind, sgate):
    def run(lct):
        from sparch_amd import functional as Fn
        adaptive, rec = kind in ("adLIF", "RadLIF"), kind in ("RLIF", "RadLIF")
        beta, a, b = (lct._p(8), lct._p(8), lct._p(8)) if adaptive else (None, None, None)
        s = Fn.SpikingCellFn.apply(kind, 1.0, lct._p(4, 3, 8), lct._p(8), beta, a, b, lct._p(8, 8) if rec else None,
                                   torch.zeros(4, 8), torch.zeros(4, 8) if adaptive else None, torch.zeros(4, 8), None, sgate)
        lct._backward(s)
    return run


def only_the_backward_differs(box, smooth, entry):
    """Every line equal but the backward entry: there `entry`_sg with (2, 5.0) in front of the stream.  Returns how
    many such lines there were."""
    assert len(box) == len(smooth)
    n = 0
    for a, b in zip(box, smooth):
        if a.startswith(entry + "("):
            head_, tail = a[len(entry):].rsplit(", NULL", 1)        # the stream is the last NULL of the line
            assert b == f"{entry}_sg{head_}, 2, 5.0, NULL{tail}", (a, b)
            n += 1
        else:
            assert a == b
    assert not any("_sg(" in ln for ln in box)
    return n


SMOOTH_CFG = ("fast_sigmoid", 5.0)


@pytest.mark.parametrize("via", ["layer", "cell"])
def test_a_smooth_layer_issues_the_sg_backward_and_nothing_else_changes(via):
    case_ = layer_case if via == "layer" else cell_case
    for kind, entry in (("adLIF", "sparch_cell_bwd"), ("RadLIF", "sparch_rec_cell_bwd")):
        box = traced(case_(kind, None))
        assert traced(case_(kind, ("boxcar", None))) == box
        assert only_the_backward_differs(box, traced(case_(kind, SMOOTH_CFG)), entry) == 1
    step = dict(dirs=2, env={"SPARCH_REC_STEP_PATH": "1"})  # the launch-per-step path: one call per step
    box = traced(layer_case("RadLIF", None, **step))
    assert only_the_backward_differs(box, traced(layer_case("RadLIF", SMOOTH_CFG, **step)), "sparch_rec_cell_step_bwd") == 3


def test_a_smooth_layer_keeps_fp32_saves():
    from tools import layer_call_trace as lct

    def run_with(sgate):
        def run(l):
            with l._attr("SAVE_BF16", True):
                layer_case("adLIF", sgate)(l)
        return run

    box, smooth = traced(run_with(None)), traced(run_with(SMOOTH_CFG))
    fwd = lambda lines: next(ln for ln in lines if ln.startswith("sparch_cell_fwd("))  # noqa: E731
    assert fwd(box).count("bf16[4,3,128]") == 3         # the spike plane, u_save, w_save
    assert fwd(smooth).count("bf16[4,3,128]") == 1      # the spike plane only: the saves are fp32
    bwd = next(ln for ln in smooth if ln.startswith("sparch_cell_bwd_sg("))
    assert ", 2, 5.0, NULL)" in bwd and lct.DTYPE[torch.float32] == "f32"
