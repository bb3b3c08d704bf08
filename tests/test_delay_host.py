"""
Axonal delays (SNN(max_delay=...), functional.DelayFn, the `sparch_delay_*` entry points, SPARCH_DELAYS) without a GPU:
  * the three entry points are declared, bound and refuse bad arguments before any device work;
  * the module: same seed => every other parameter is bit-equal with and without delays, max_delay=0 registers
    nothing, the constructor's refusals, which layers get a `delay`, fixed delays;
  * the calls a delayed network issues (driven on CPU tensors against the recording stand-in of
    tools/layer_call_trace.py): one gather per delayed layer on the representation the GEMMs read, the first layer's dX
    product only with learnable delays, and the backward's call;
  * SPARCH_DELAYS parsing and Experiment's refusals; the streaming and stateful refusals;
  * without delays the committed layer call trace is unchanged.
"""
import argparse
import os
import re

import pytest
import torch

from tests.entry_probes import Entry, P, ptrs
from tests.kit import EINVAL, EWORKSPACE
from tools.layer_call_trace import calls as _calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = [("B", 2), ("T", 3), ("K", 8)]
FWD = Entry("sparch_delay_fwd", SHAPE + [("elem_size", 2), ("max_delay", 4)] + ptrs("delay x") + [("ldx", 8)] + ptrs("y")
            + [("ldy", 8), ("lengths", None), ("offsets", None), ("stream", None)])
BWD = Entry("sparch_delay_bwd", SHAPE + [("x_elem_size", 4), ("max_delay", 4)] + ptrs("delay g_y") + [("ldg", 8)] + ptrs("x")
            + [("ldx", 8), ("x_scale", 1.0)] + ptrs("g_x") + [("ldgx", 8)] + ptrs("g_delay ws")
            + [("ws_bytes", 0), ("lengths", None), ("offsets", None), ("stream", None)])
STREAM = Entry("sparch_delay_stream", [("B", 2), ("Tc", 3), ("K", 8), ("elem_size", 4), ("max_delay", 4)] + ptrs("delay x")
               + [("ldx", 8)] + ptrs("y") + [("ldy", 8)] + ptrs("hist") + [("stream", None)])


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_and_bound():
    from sparch_amd._capi import PROTOTYPES, lib
    assert lib.sparch_abi_version() == 5
    with open(os.path.join(ROOT, "include", "sparch_hip.h")) as f:
        header = f.read()
    for e in (FWD, BWD, STREAM):
        decl = re.search(r"\bint " + e.name + r"\(([^;]*)\);", header)
        assert decl, e.name
        params = [q.strip() for q in decl.group(1).replace("\n", " ").split(",")]
        assert len(params) == len(e.args) == len(PROTOTYPES[e.name][1]), e.name
        assert [q.split()[-1].lstrip("*") for q in params] == [k for k, _ in e.args], e.name
        assert hasattr(lib, e.name)
    assert os.path.exists(os.path.join(ROOT, "sparch_amd", "csrc", "delay.hip"))


def test_workspace_query():
    from sparch_amd._capi import lib
    q = lib.sparch_delay_bwd_workspace_bytes
    assert q(0, 3, 8) == 0 and q(2, 0, 8) == 0 and q(2, 3, 0) == 0 and q(-1, 3, 8) == 0
    assert q(2, 3, 8) == 8 * 4                      # one slab of K floats for a handful of rows
    assert q(3, 12, 36) == 2 * 36 * 4               # 36 rows: slabs of 32 rows
    assert q(256, 250, 1024) == 128 * 1024 * 4      # never more than 128 slabs
    assert q(1 << 15, 1 << 15, 4) == 128 * 4 * 4    # 2^30 rows: 64-bit row counts
    assert q((1 << 31) - 1, (1 << 31) - 1, 1) == 128 * 4            # 2^62 rows: the slab's row count is 64-bit too


@pytest.mark.parametrize("e", [FWD, BWD, STREAM], ids=lambda e: e.name)
def test_delay_entries_refuse_before_any_device_work(e):
    """Nothing here reaches a launch: every call has something broken."""
    time = "Tc" if e is STREAM else "T"
    for k in ("B", time, "K"):
        assert e(**{k: 0}) == EINVAL and e(**{k: -3}) == EINVAL, k
    for d in (0, -1, 256, 1 << 20):
        assert e(max_delay=d) == EINVAL, d
    assert e(delay=None) == EINVAL
    size = "x_elem_size" if e is BWD else "elem_size"
    for s in (0, 1, 3, 8):
        assert e(**{size: s}) == EINVAL, s
    for ld in ("ldx", "ldg", "ldgx", "ldy"):
        if any(k == ld for k, _ in e.args):
            assert e(**{ld: 7}) == EINVAL, ld
    if e is not STREAM:
        assert e(offsets=P) == EINVAL                                   # an offset without lengths
    if e is FWD:
        assert e(x=None) == EINVAL and e(y=None) == EINVAL
    if e is STREAM:
        assert e(x=None) == EINVAL and e(y=None) == EINVAL and e(hist=None) == EINVAL
    if e is BWD:
        assert e(g_y=None) == EINVAL and e(g_x=None, g_delay=None) == EINVAL
        assert e(x=None) == EINVAL and e(ws=None) == EINVAL             # the delay's gradient needs x and a workspace
        assert e() == EWORKSPACE and e(ws_bytes=8 * 4 - 1) == EWORKSPACE  # a valid call up to its workspace
        assert e(offsets=P, lengths=P, ws_bytes=0) == EWORKSPACE          # (offsets with lengths pass the argument check)


# ------------------------------------------------------------------------------------------------ the module
def _net(kind="adLIF", sizes=(8, 8, 5), **kw):
    import sparch_amd
    return sparch_amd.SNN((3, None, 6), list(sizes), neuron_type=kind, **kw)


@pytest.mark.parametrize("kind", ["LIF", "adLIF", "RLIF", "RadLIF"])
@pytest.mark.parametrize("kw", [dict(max_delay=3), dict(max_delay=7, delay_init="uniform"),
                                dict(max_delay=2, delay_init="uniform", delay_layers="hidden", learn_delays=False)],
                         ids=["zero", "uniform", "uniform-hidden-fixed"])
def test_every_other_parameter_is_bit_equal_under_one_seed(kind, kw):
    from tests.kit import same_bits
    torch.manual_seed(5)
    plain = _net(kind, bidirectional=(kind == "RLIF"))
    torch.manual_seed(5)
    delayed = _net(kind, bidirectional=(kind == "RLIF"), **kw)
    a, b = plain.state_dict(), delayed.state_dict()
    assert list(a) == [k for k in b if not k.endswith(".delay")]
    for k, v in a.items():
        assert same_bits(v, b[k]), k
    first = 1 if kw.get("delay_layers") == "hidden" else 0
    assert [k for k in b if k.endswith(".delay")] == [f"snn.{i}.delay" for i in range(first, 3)]
    for i, layer in enumerate(delayed.snn):
        if i < first:
            assert not hasattr(layer, "delay") and getattr(layer, "max_delay", 0) == 0
            continue
        d = layer.delay
        assert isinstance(d, torch.nn.Parameter) and d.dtype == torch.float32 and d.shape == (layer.input_size,)
        assert d.requires_grad == kw.get("learn_delays", True) and layer.max_delay == kw["max_delay"]
        if kw.get("delay_init") == "uniform":
            v = d.detach()
            assert float(v.min()) >= 0 and float(v.max()) <= kw["max_delay"] and v.unique().numel() > 1
        else:
            assert not d.detach().any()
    assert sorted(delayed.delay_steps()) == list(range(first, 3))
    assert "max_delay" in repr(delayed) and "max_delay" not in repr(plain)


def test_max_delay_zero_registers_nothing():
    torch.manual_seed(1)
    plain = _net()
    torch.manual_seed(1)
    off = _net(max_delay=0, delay_init="uniform", learn_delays=False, delay_layers="hidden")
    assert list(plain.state_dict()) == list(off.state_dict())
    assert [n for n, _ in off.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert off.delay_steps() == {} and not any(hasattr(layer, "delay") for layer in off.snn)
    assert torch.equal(torch.rand(3), (torch.manual_seed(1), _net(), torch.rand(3))[2])    # and draws nothing
    # a reference-shaped checkpoint loads into it, and the other way round
    off.load_state_dict(plain.state_dict())
    with pytest.raises(RuntimeError, match="delay"):
        _net(max_delay=2).load_state_dict(plain.state_dict())


def test_constructor_refusals():
    for bad in (-1, 256, 2.0, "3", True, None):
        with pytest.raises(ValueError, match="max_delay"):
            _net(max_delay=bad)
    with pytest.raises(ValueError, match="delay_init"):
        _net(max_delay=2, delay_init="normal")
    with pytest.raises(ValueError, match="delay_layers"):
        _net(max_delay=2, delay_layers="first")
    _net(max_delay=255)
    from sparch_amd import functional as Fn
    for bad in (0, 256, 1.5):
        with pytest.raises(ValueError, match="max_delay"):
            Fn.check_max_delay(bad)


def test_a_host_tensor_is_refused_not_delayed_on_the_cpu():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _net(max_delay=2)(torch.zeros(3, 4, 6))
    from sparch_amd import functional as Fn
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.delay_forward(torch.zeros(3, 4, 6), torch.zeros(6), 2)


# ------------------------------------------------------------------------------------------------ the calls issued
def _traced(kind="LIF", source="dense", train=True, **kw):
    """The C-ABI calls of one forward (and backward) of a two-hidden-layer network, as text lines."""
    from tools import layer_call_trace as lct
    from sparch_amd import functional as Fn, snns
    B, T, K, H, C = 4, 3, 32, 128, 5
    grads = {}

    def run(lct):
        torch.manual_seed(0)
        net = snns.SNN((B, None, K), [H, H, C], neuron_type=kind, **kw)
        net.train(train)
        x = (Fn.input_from_counts(torch.zeros(B, T, K, dtype=torch.uint8)) if source == "counts"
             else torch.zeros(B, T, K))
        rates = []
        for i, layer in enumerate(net.snn):
            if i == net.num_layers - 1:
                x = layer(x, u0=torch.zeros(B, C))
            else:
                states = (torch.zeros(B, H), torch.zeros(B, H) if kind in ("adLIF", "RadLIF") else None, torch.zeros(B, H))
                x, r = layer.forward_with_rate(x, states=states, fp32_out=False)
                rates.append(r)
        if train:
            lct._backward(x, *rates)
            grads.update({n: p.grad for n, p in net.named_parameters()})

    return lct.traced(run)[1:], grads


def test_without_delays_the_calls_are_what_they_were():
    plain, _ = _traced()
    off, _ = _traced(max_delay=0)
    assert plain == off and not any("delay" in ln for ln in plain)
    from tools import layer_call_trace as lct
    assert lct.difference(lct.trace()) == []


@pytest.mark.parametrize("source", ["dense", "counts"])
def test_a_delayed_network_gathers_once_per_layer_on_what_the_gemms_read(source):
    plain, _ = _traced(source=source)
    lines, grads = _traced(source=source, max_delay=3)
    fwd, bwd = _calls(lines, "sparch_delay_fwd"), _calls(lines, "sparch_delay_bwd")
    assert len(fwd) == 3 and len(bwd) == 3
    # layer 0: the fp32 batch itself, or the bf16 plane of the spike counts; layers 1, 2: the bf16 spike plane
    sizes = [a.split("(")[1].split(", ")[:5] for a in fwd]
    assert sizes[0] == ["4", "3", "32", "4" if source == "dense" else "2", "3"]
    assert sizes[1] == sizes[2] == ["4", "3", "128", "2", "3"]
    assert all(", NULL, NULL, NULL)" in a for a in fwd)                 # dense: no lengths, no offsets
    # the backward: layer 0 gives the delay's gradient only (the batch has none), the others g_x as well
    first = next(b for b in bwd if b.startswith("sparch_delay_bwd(4, 3, 32,"))
    assert ", NULL, 32, f32[32]#" in first                               # g_x NULL, g_delay (K,)
    for b in bwd:
        if b is not first:
            assert "f32[4,3,128]#" in b and "f32[128]#" in b and "bf16[" in b
    # every delay has a gradient, and every other call of the plain network is still issued, in order
    assert all(g is not None for n, g in grads.items() if n.endswith("delay")) and len(grads) > 3
    kept = [ln for ln in lines if "delay" not in ln]
    names = lambda ls: [ln.split("(")[0] for ln in ls if "(" in ln and not ln.startswith("q")]  # noqa: E731
    extra = [n for n in names(kept) if n not in names(plain)]
    assert not extra, extra
    it = iter(names(kept))
    assert all(n in it for n in names(plain)), "a call of the plain network is missing or out of order"


def test_the_first_layers_dx_product_runs_only_with_learnable_delays():
    def dx_products(lines):   # products with M = B T = 12 rows and N = K = 32 columns: dX of layer 0
        return [ln for ln in lines if re.match(r"sparch_gemm\w*_nn\w*\(12, 32, 128,", ln)]
    plain, _ = _traced()
    assert dx_products(plain) == []
    learn, _ = _traced(max_delay=3)
    assert len(dx_products(learn)) == 1
    for kw in (dict(max_delay=3, learn_delays=False), dict(max_delay=3, delay_layers="hidden")):
        lines, grads = _traced(**kw)
        assert dx_products(lines) == [], kw
    fixed, grads = _traced(max_delay=3, learn_delays=False)
    assert len(_calls(fixed, "sparch_delay_fwd")) == 3
    bwd = _calls(fixed, "sparch_delay_bwd")
    assert len(bwd) == 2 and all(b.endswith(", NULL, NULL, 0, NULL, NULL, NULL)") for b in bwd)   # g_x only: no g_delay, no ws
    assert all(g is None for n, g in grads.items() if n.endswith("delay"))
    hidden, _ = _traced(max_delay=3, delay_layers="hidden")
    assert len(_calls(hidden, "sparch_delay_fwd")) == 2


def test_eval_issues_the_gather_and_no_backward():
    lines, _ = _traced(train=False, max_delay=2)
    assert len(_calls(lines, "sparch_delay_fwd")) == 3 and not _calls(lines, "sparch_delay_bwd")


def test_lengths_and_pack_reach_the_kernels():
    from tools import layer_call_trace as lct
    from sparch_amd import snns
    rec = lct._Recorder()
    with lct._tracing(rec):
        rec.new_case("case")
        net = snns.SNN((3, None, 32), [128, 5], neuron_type="LIF", max_delay=2).train()
        lens = snns.prepare_lengths([4, 1, 2], 3, 4, "cpu")
        s, r = net.snn[0].forward_with_rate(torch.zeros(3, 4, 32), states=(torch.zeros(3, 128), None, torch.zeros(3, 128)),
                                            fp32_out=False, lengths=lens)
        net.snn[1](s, u0=torch.zeros(3, 5), lengths=lens)
        plan = snns.prepare_packing([4, 1, 2], 3, 4, "cpu")
        s, r = net.snn[0].forward_with_rate(torch.zeros(1, 7, 32), states=(torch.zeros(3, 128), None, torch.zeros(3, 128)),
                                            fp32_out=False, pack=plan)
        net.snn[1](s, u0=torch.zeros(3, 5), pack=plan)
    fwd = _calls(rec.lines, "sparch_delay_fwd")
    assert len(fwd) == 4
    for a in fwd[:2]:
        assert a.startswith("sparch_delay_fwd(3, 4, ") and a.endswith(", i32[3]#" + a.split("i32[3]#")[1]) and "NULL, NULL)" in a
    for a in fwd[2:]:                                                     # packed: 3 sequences, the longest has 4 steps
        assert a.startswith("sparch_delay_fwd(3, 4, ") and "i32[3]/" not in a and "i32[4]" in a and "NULL, NULL)" not in a


# ------------------------------------------------------------------------------------------------ refusals
def test_stateful_training_refuses_delays():
    x = torch.zeros(3, 4, 6)
    net = _net(max_delay=2)
    for kw in (dict(return_state=True), dict(state=[{}, {}, {}]), dict(state=[{}, {}, {}], return_state=True)):
        with pytest.raises(ValueError, match="axonal delays"):
            net(x, **kw)
    with pytest.raises(ValueError, match="axonal delays"):
        net.snn[0].forward_with_rate(x, return_state=True)
    with pytest.raises(ValueError, match="axonal delays"):
        net.snn[-1](torch.zeros(3, 4, 8), return_state=True)
    with pytest.raises(ValueError, match="axonal delays"):                # only the readout is delayed: refused as well
        hidden = _net(sizes=(8, 5), max_delay=2, delay_layers="hidden")
        hidden(x, return_state=True)


def test_streaming_refusals_and_state():
    from sparch_amd import streaming
    net = _net(max_delay=2).eval()
    for kw, match in ((dict(fused=True), "fused"), (dict(fused=True, sparse=True), "sparse"), (dict(graph=True), "graph")):
        with pytest.raises(ValueError, match=match):
            streaming.StreamingSNN(net, 3, **kw)
    streaming.StreamingSNN(net, 3)
    streaming.StreamingSNN(_net().eval(), 3, fused=True, sparse=True)      # (without delays nothing changes)


def test_streaming_state_gains_hist_only_with_delays():
    from tools import layer_call_trace as lct
    from sparch_amd import snns, streaming
    B, Tc, K, H, C = 4, 3, 32, 128, 5
    states = [(torch.zeros(B, H), None, torch.zeros(B, H)) for _ in range(2)] + [torch.zeros(B, C)]
    rec = lct._Recorder()
    with lct._tracing(rec):
        rec.new_case("case")
        for D in (0, 2):
            net = snns.SNN((B, None, K), [H, H, C], neuron_type="LIF", max_delay=D, delay_layers="hidden").eval()
            st = streaming.StreamingSNN(net, B)
            st.reset(states=states)
            st.step(torch.zeros(B, Tc, K))
            st.step(torch.zeros(B, 1, K, dtype=torch.uint8))
            state = st.get_state()
            if D == 0:
                assert all("hist" not in s for s in state)
                continue
            assert "hist" not in state[0] and state[1]["hist"].shape == (B, D, H) and state[2]["hist"].shape == (B, D, H)
            assert state[1]["hist"].dtype == torch.bfloat16
            st._layers[1].hist.fill_(1.0)
            st.reset(states=[tuple(None if t is None else t[:2] for t in s) if isinstance(s, tuple) else s[:2]
                             for s in states], rows=[1, 3])
            assert st._layers[1].hist[:, :, 0].float().sum(1).tolist() == [2.0, 0.0, 2.0, 0.0]
            st.set_state(state)
            assert not st._layers[1].hist.any()
    calls = _calls(rec.lines, "sparch_delay_stream")
    assert len(calls) == 4 and calls[0].startswith("sparch_delay_stream(4, 3, 128, 2, 2,")
    assert calls[2].startswith("sparch_delay_stream(4, 1, 128, 2, 2,")
    assert not _calls(rec.lines, "sparch_delay_fwd")


# ------------------------------------------------------------------------------------------------ the GPU file's cases
def test_the_network_cases_fire_inside_the_window_in_the_cpu_restatement():
    """tests/delay_cases.py: the committed data seeds are the ones the fp64 restatement picks, and with them every hidden
    layer fires inside the window, with zero delays and with the test's delays — before anything runs on a GPU."""
    import sparch_amd as sp
    from tests import delay_cases as dc
    for (kind, sizes, bidir), seed in dc.SEEDS.items():
        assert dc.pick_seed(sp, kind, sizes, bidir) == seed, (kind, sizes, bidir)
        net = dc.make_net(sp, kind, sizes, bidir, max_delay=dc.ND)
        x, _, init = dc.net_inputs(kind, sizes, bidir, seed)
        for delays in (None, dc.net_delays(net)):
            rates = dc.cpu_rates(net, kind, x, init, delays, bidir)
            assert len(rates) == 2 and dc.in_window(rates, dc.PICK_WINDOW), (kind, sizes, bidir, rates)
    for kind in dc.KINDS:                                                   # the ragged cases of the GPU file
        net = dc.make_net(sp, kind, max_delay=dc.ND)
        x, _, init = dc.net_inputs(kind, seed=dc.seed_of(kind))
        rates = dc.cpu_rates_ragged(net, kind, x, init, dc.net_delays(net), dc.NET_LENGTHS)
        assert dc.in_window(rates, dc.PICK_WINDOW), (kind, rates)
    assert set(k[0] for k in dc.SEEDS) == set(dc.KINDS)
    assert any(sizes[0] % 4 for kind, sizes, _ in dc.SEEDS if kind in ("RLIF", "RadLIF"))


def test_the_kernel_cases_hold_every_class_of_delay():
    from tests import delay_cases as dc
    from tests import delay_numpy as dn
    for K in dc.WIDTHS:
        for D in dc.CAPS:
            x, g, th = dc.kernel_data(K, D)
            d, gate = dn.steps(th, D), dn.gate(th, D)
            assert d[0] == 0 and (th < 0).any() and (th > D).any() and (gate == 0).any() and (gate == 1).any()
            if D >= 4:
                assert th[1] == 2.5 and d[1] == 2 and th[2] == 3.5 and d[2] == 4
            if D > dc.T:
                assert (d >= dc.T).any()                                    # whole columns come out zero
            _, mag = dn.backward_theta(g, x, th, D)
            assert (mag[d < dc.T - 1] > 0).all(), (K, D)                    # the delay's gradient has something to sum
    x, g, th = dc.big_kernel_data()
    d = dn.steps(th, dc.BIG_D)
    assert dc.BIG_T > 2 * 64 and dc.BIG_T > 64 + dc.BIG_D and set(d) == set(range(dc.BIG_D + 1))
    assert (dn.backward_theta(g, x, th, dc.BIG_D)[1] > 0).all()


# ------------------------------------------------------------------------------------------------ SPARCH_DELAYS
def test_sparch_delays_parsing():
    from sparch_amd import exp
    assert exp.parse_delays(None) is None and exp.parse_delays("") is None and exp.parse_delays("  ") is None
    base = {"max_delay": 4, "delay_init": "zero", "learn_delays": True, "delay_layers": "all"}
    assert exp.parse_delays("4") == base and exp.parse_delays(" 4 ") == base and exp.parse_delays("4:zero") == base
    assert exp.parse_delays("4:uniform") == dict(base, delay_init="uniform")
    assert exp.parse_delays("25:fixed") == dict(base, max_delay=25, learn_delays=False)
    assert exp.parse_delays("255:uniform:fixed:hidden") == {"max_delay": 255, "delay_init": "uniform",
                                                            "learn_delays": False, "delay_layers": "hidden"}
    assert exp.parse_delays("4:hidden:uniform") == dict(base, delay_init="uniform", delay_layers="hidden")
    for bad in ("0", "-1", "256", "4.0", "four", "uniform", "4:", "4:normal", "4:zero:uniform", "4:fixed:fixed",
                "4:hidden:hidden", "4:uniform:uniform", ":4", "4,uniform", "1e2"):
        with pytest.raises(ValueError, match="SPARCH_DELAYS"):
            exp.parse_delays(bad)


def test_experiment_refuses_delay_combinations_before_anything_else(monkeypatch, tmp_path):
    from sparch_amd import exp

    def args(**kw):
        base = dict(model_type="adLIF", sync_bn=False, use_pretrained_model=False, bidirectional=False,
                    compute_dtype="fp32", new_exp_folder=str(tmp_path / "never"))
        base.update(kw)
        return argparse.Namespace(**base)

    for name in ("SPARCH_LENGTHS", "SPARCH_PER_STEP_LOSS", "SPARCH_READOUT", "SPARCH_SURROGATE", "SPARCH_CLIP_GRAD",
                 "SPARCH_TBPTT"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SPARCH_DELAYS", "many")
    with pytest.raises(ValueError, match="SPARCH_DELAYS"):
        exp.Experiment(args())
    monkeypatch.setenv("SPARCH_DELAYS", "4:uniform")
    for model in ("MLP", "RNN", "LiGRU", "GRU"):
        with pytest.raises(ValueError, match="SPARCH_DELAYS needs a spiking model"):
            exp.Experiment(args(model_type=model))
    monkeypatch.setenv("SPARCH_TBPTT", "8")
    with pytest.raises(ValueError, match="SPARCH_DELAYS with SPARCH_TBPTT"):
        exp.Experiment(args())
    assert not (tmp_path / "never").exists()
