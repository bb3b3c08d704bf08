"""
Synaptic currents (SNN(synapse=...), the `sparch_synapse_*` entry points, SPARCH_SYNAPSE) without a GPU:
  * the entry points are declared, bound and refuse bad arguments before any device work; the ABI version stays 5;
  * the module: same seed => every other parameter is bit-equal with and without a synapse, synapse=None registers
    nothing (the state_dict keys are the reference's), which layers get a `gamma`, its init ranges, fixed synapses,
    extra_repr, the constructor's refusals;
  * the calls a network with a synapse issues (driven on CPU tensors against the recording stand-in of
    tools/layer_call_trace.py): one filter per layer between the projection and the cell, which then gets no scale and
    no shift; the backward's call; lengths and pack reach the kernels; a bidirectional layer runs on the doubled batch;
  * every refusal: stateful training, a captured step, pack with bidirectional, the streaming classes' fused, sparse
    and captured steps; SPARCH_SYNAPSE parsing and Experiment's refusals;
  * without a synapse the committed layer call trace is unchanged.
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
SHAPE = [("B", 2), ("T", 3), ("H", 8)]
FWD = Entry("sparch_synapse_fwd", SHAPE + ptrs("Wx") + [("ldwx", 8)] + ptrs("bias scale shift gamma")
            + [("lo", 0.0), ("hi", 0.9)] + ptrs("i0 i_out") + [("ldi", 8)] + ptrs("i_T")
            + [("lengths", None), ("offsets", None), ("stream", None)])
BWD = Entry("sparch_synapse_bwd", SHAPE + ptrs("g_i") + [("ldg", 8)] + ptrs("i") + [("ldi", 8)] + ptrs("i0 gamma")
            + [("lo", 0.0), ("hi", 0.9)] + ptrs("g_z") + [("ldgz", 8)] + ptrs("g_gamma ws")
            + [("ws_bytes", 0), ("bn_x", None), ("ldbn", 8), ("bn_mean", None), ("bn_invstd", None), ("bn_ws", None),
               ("lengths", None), ("offsets", None), ("stream", None)])


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_and_bound():
    from sparch_amd._capi import PROTOTYPES, lib
    assert lib.sparch_abi_version() == 5
    with open(os.path.join(ROOT, "include", "sparch_hip.h")) as f:
        header = f.read()
    for e in (FWD, BWD):
        decl = re.search(r"\bint " + e.name + r"\(([^;]*)\);", header)
        assert decl, e.name
        params = [q.strip() for q in decl.group(1).replace("\n", " ").split(",")]
        assert len(params) == len(e.args) == len(PROTOTYPES[e.name][1]), e.name
        assert [q.split()[-1].lstrip("*") for q in params] == [k for k, _ in e.args], e.name
        assert hasattr(lib, e.name)
    assert os.path.exists(os.path.join(ROOT, "sparch_amd", "csrc", "synapse.hip"))


def test_workspace_query():
    from sparch_amd._capi import lib
    q = lib.sparch_synapse_bwd_workspace_bytes
    assert q(0, 3, 8) == 0 and q(2, 0, 8) == 0 and q(2, 3, 0) == 0 and q(-1, 3, 8) == 0
    assert q(2, 3, 8) == 2 * 8 * 4 and q(256, 250, 1024) == 256 * 1024 * 4      # one slab of H floats per sequence
    assert q(1 << 20, 1, 1 << 12) == (1 << 34)                                 # 64-bit sizes


@pytest.mark.parametrize("e", [FWD, BWD], ids=lambda e: e.name)
def test_synapse_entries_refuse_before_any_device_work(e):
    """Nothing here reaches a launch: every call has something broken."""
    for k in ("B", "T", "H"):
        assert e(**{k: 0}) == EINVAL and e(**{k: -3}) == EINVAL, k
    for lo, hi in ((-0.1, 0.5), (0.6, 0.5), (0.0, 1.0), (0.0, 1.5), (float("nan"), 0.5), (0.0, float("nan"))):
        assert e(lo=lo, hi=hi) == EINVAL, (lo, hi)
    assert e(gamma=None) == EINVAL
    for ld in ("ldwx", "ldi", "ldg", "ldgz"):
        if any(k == ld for k, _ in e.args):
            assert e(**{ld: 7}) == EINVAL, ld
    assert e(offsets=P) == EINVAL                                       # an offset without lengths
    if e is FWD:
        assert e(Wx=None) == EINVAL and e(i_out=None) == EINVAL
    else:
        assert e(g_i=None) == EINVAL and e(g_z=None, g_gamma=None) == EINVAL
        assert e(i=None) == EINVAL and e(ws=None) == EINVAL             # gamma's gradient needs i and a workspace
        assert e() == EWORKSPACE and e(ws_bytes=2 * 8 * 4 - 1) == EWORKSPACE    # a valid call up to its workspace
        assert e(offsets=P, lengths=P, ws_bytes=0) == EWORKSPACE        # (offsets with lengths pass the argument check)
        bn = dict(bn_x=P, bn_mean=P, bn_invstd=P, bn_ws=P)              # BatchNorm's sums need all four, g_z and a stride
        assert e(**bn) == EWORKSPACE
        for k in ("bn_mean", "bn_invstd", "bn_ws", "g_z"):
            assert e(**dict(bn, **{k: None})) == EINVAL, k
        assert e(ldbn=7, **bn) == EINVAL


# ------------------------------------------------------------------------------------------------ the module
def _net(kind="adLIF", sizes=(8, 8, 5), **kw):
    import sparch_amd
    return sparch_amd.SNN((3, None, 6), list(sizes), neuron_type=kind, **kw)


@pytest.mark.parametrize("kind", ["LIF", "adLIF", "RLIF", "RadLIF"])
@pytest.mark.parametrize("kw", [dict(synapse=(0.0, 0.9)), dict(synapse=(0.5, 0.8), syn_init="lo", max_delay=2),
                                dict(synapse=(0.2, 0.2), synapse_layers="hidden", learn_synapse=False)],
                         ids=["uniform", "lo-delays", "hidden-fixed"])
def test_every_other_parameter_is_bit_equal_under_one_seed(kind, kw):
    other = {k: v for k, v in kw.items() if k == "max_delay"}
    torch.manual_seed(11)
    plain = _net(kind, **other)
    torch.manual_seed(11)
    syn = _net(kind, **kw)
    ref = plain.state_dict()
    got = syn.state_dict()
    extra = sorted(set(got) - set(ref))
    layers = [1] if kw.get("synapse_layers") == "hidden" else [0, 1]
    assert extra == [f"snn.{i}.gamma" for i in layers] and not set(ref) - set(got)
    for k, v in ref.items():
        assert torch.equal(got[k], v), k
    lo, hi = kw["synapse"]
    for i in layers:
        g = syn.snn[i].gamma
        assert g.shape == (8,) and g.requires_grad == kw.get("learn_synapse", True) and syn.snn[i].synapse == (lo, hi)
        assert bool(((g >= lo) & (g <= hi)).all())
        if kw.get("syn_init") == "lo" or lo == hi:
            assert bool((g == lo).all())
        else:
            assert len(set(g.tolist())) == 8
    assert not hasattr(syn.snn[-1], "gamma") and getattr(syn.snn[-1], "synapse", None) is None
    assert f"synapse=({lo:g}, {hi:g})" in repr(syn) and "synapse" not in repr(plain)
    assert sorted(syn.synapse_gammas()) == layers


def test_synapse_none_registers_nothing():
    import sparch_amd
    net = _net(synapse=None)
    assert net.synapse is None and not any("gamma" in k for k in net.state_dict())
    assert all(getattr(lay, "synapse", None) is None for lay in net.snn) and net.synapse_gammas() == {}
    ref = sparch_amd.SNN((3, None, 6), [8, 8, 5], neuron_type="adLIF")
    assert list(net.state_dict()) == list(ref.state_dict())
    # without a readout layer every layer is a hidden spiking layer
    assert sorted(_net(use_readout_layer=False, synapse=(0.0, 0.5)).synapse_gammas()) == [0, 1, 2]


def test_constructor_refusals():
    for bad in ((-0.1, 0.5), (0.6, 0.5), (0.0, 1.0), (0.5,), "0:0.9", 0.5, (0.0, float("nan")), ("a", "b")):
        with pytest.raises(ValueError, match="synapse"):
            _net(synapse=bad)
    with pytest.raises(ValueError, match="syn_init"):
        _net(synapse=(0.0, 0.9), syn_init="zero")
    with pytest.raises(ValueError, match="synapse_layers"):
        _net(synapse=(0.0, 0.9), synapse_layers="first")


def test_a_host_tensor_is_refused_not_filtered_on_the_cpu():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _net(synapse=(0.0, 0.9))(torch.zeros(3, 4, 6))
    from sparch_amd import functional as Fn
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.synapse_forward(torch.zeros(3, 4, 6), torch.zeros(6), (0.0, 0.9))
    with pytest.raises(ValueError, match="synapse"):
        Fn.synapse_forward(torch.zeros(3, 4, 6), torch.zeros(6), (0.0, 1.0))


# ------------------------------------------------------------------------------------------------ the calls issued
def _traced(kind="LIF", train=True, norm="batchnorm", bidirectional=False, lengths=None, **kw):
    """The C-ABI calls of one forward (and backward) of a two-hidden-layer network, as text lines."""
    from tools import layer_call_trace as lct
    from sparch_amd import snns
    B, T, K, H, C = 4, 3, 32, 128, 5
    dirs = 2 if bidirectional else 1
    grads = {}

    def run(lct):
        torch.manual_seed(0)
        net = snns.SNN((B, None, K), [H, H, C], neuron_type=kind, normalization=norm, bidirectional=bidirectional, **kw)
        net.train(train)
        x = torch.zeros(B, T, K)
        rates = []
        fw = {} if lengths is None else {"lengths": (torch.tensor(lengths, dtype=torch.int32), sum(lengths))}
        for i, layer in enumerate(net.snn):
            if i == net.num_layers - 1:
                x = layer(x, u0=torch.zeros(B, C), **fw)
            else:
                rows = B * dirs
                states = (torch.zeros(rows, H), torch.zeros(rows, H) if kind in ("adLIF", "RadLIF") else None,
                          torch.zeros(rows, H))
                x, r = layer.forward_with_rate(x, states=states, fp32_out=False, **fw)
                rates.append(r)
        if train:
            lct._backward(x, *rates)
            grads.update({n: p.grad for n, p in net.named_parameters()})

    return lct.traced(run)[1:], grads


def _index(lines, name):
    return [k for k, ln in enumerate(lines) if ln.startswith(name + "(")]


def test_without_a_synapse_the_calls_are_what_they_were():
    plain, _ = _traced()
    off, _ = _traced(synapse=None)
    assert plain == off and not any("synapse" in ln for ln in plain)
    from tools import layer_call_trace as lct
    assert lct.difference(lct.trace()) == []


@pytest.mark.parametrize("kind", ["LIF", "RadLIF"])
def test_a_network_with_a_synapse_filters_once_per_layer_between_projection_and_cell(kind):
    plain, _ = _traced(kind)
    lines, grads = _traced(kind, synapse=(0.0, 0.9))
    fwd, bwd = _calls(lines, "sparch_synapse_fwd"), _calls(lines, "sparch_synapse_bwd")
    assert len(fwd) == 2 and len(bwd) == 2 and all(ln.startswith("sparch_synapse_fwd(4, 3, 128,") for ln in fwd)
    cell = "sparch_rec_cell_fwd" if kind == "RadLIF" else "sparch_cell_fwd"
    at_f, at_c = _index(lines, "sparch_synapse_fwd"), _index(lines, cell)
    assert len(at_c) == 2 and all(f < c for f, c in zip(at_f, at_c)) and at_c[0] < at_f[1]
    # BatchNorm's column sums leave the cell's backward for the filter's (they are sums over g_z): no reduction pass more
    assert len(_calls(lines, "sparch_bn_bwd_reduce")) == len(_calls(plain, "sparch_bn_bwd_reduce"))
    assert len(_calls(lines, "sparch_colsum_clamped")) == len(_calls(plain, "sparch_colsum_clamped")) + 2
    for i in range(2):
        g = grads[f"snn.{i}.gamma"]
        assert g is not None and g.shape == (128,)
    fixed, fgrads = _traced(kind, synapse=(0.0, 0.9), learn_synapse=False)
    assert len(_calls(fixed, "sparch_synapse_bwd")) == 2 and all(fgrads[f"snn.{i}.gamma"] is None for i in range(2))
    hidden, _ = _traced(kind, synapse=(0.0, 0.9), synapse_layers="hidden")
    assert len(_calls(hidden, "sparch_synapse_fwd")) == 1
    ev, _ = _traced(kind, train=False, synapse=(0.0, 0.9))
    assert len(_calls(ev, "sparch_synapse_fwd")) == 2 and not _calls(ev, "sparch_synapse_bwd")


def test_lengths_and_two_directions_reach_the_kernels():
    lines, _ = _traced(synapse=(0.0, 0.9), lengths=[3, 1, 2, 3])
    assert len(_calls(lines, "sparch_synapse_fwd")) == 2 and len(_calls(lines, "sparch_cell_fwd_len")) == 2
    assert len(_calls(lines, "sparch_cell_bwd_len")) == 2
    # both directions: the doubled batch of the ragged route, with lengths synthesised where none are given
    for lengths in (None, [3, 1, 2, 3]):
        two, _ = _traced(synapse=(0.0, 0.9), bidirectional=True, lengths=lengths)
        fwd = _calls(two, "sparch_synapse_fwd")
        assert len(fwd) == 2 and all(ln.startswith("sparch_synapse_fwd(8, 3, 128,") for ln in fwd)
        assert len(_calls(two, "sparch_bidir_split_len")) == 2 and len(_calls(two, "sparch_cell_fwd_len")) == 2
        assert len(_calls(two, "sparch_synapse_bwd")) == 2


# ------------------------------------------------------------------------------------------------ refusals
def test_stateful_training_and_packing_refusals():
    x = torch.zeros(3, 4, 6)
    net = _net(synapse=(0.0, 0.9))
    for kw in (dict(return_state=True), dict(state=[{}, {}, {}]), dict(state=[{}, {}, {}], return_state=True)):
        with pytest.raises(ValueError, match="with a synapse"):
            net(x, **kw)
    with pytest.raises(ValueError, match="with a synapse"):
        net.snn[0].forward_with_rate(x, return_state=True)
    two = _net(synapse=(0.0, 0.9), bidirectional=True)
    with pytest.raises(ValueError, match="pack=True with bidirectional=True and a synapse"):
        two(x, lengths=torch.tensor([4, 2, 1]), pack=True)
    from sparch_amd import graph

    class Untouched:                                                    # the refusal comes before graph mode is switched on
        def enable_graph_mode(self):
            raise AssertionError("the optimizer was switched to graph mode")

    with pytest.raises(ValueError, match="captured step"):
        graph.GraphedTrainStep(net, Untouched(), None, x, torch.zeros(3, dtype=torch.long))
    assert not hasattr(net.snn[0], "_seed_word") and getattr(net, "_static_states", None) is None
    net._static_states = object()                                       # (and SNN.forward refuses inside one as well)
    with pytest.raises(ValueError, match="captured step"):
        net(x)
    wide = _net("RLIF", sizes=(1028, 5), synapse=(0.0, 0.9), bidirectional=True)
    with pytest.raises(ValueError, match="recurrent hidden size above 1024"):   # before the projection, in the caller's terms
        wide(x)
    with pytest.raises(ValueError, match="recurrent hidden size above 1024"):
        wide.snn[0].forward_with_rate(x)


def test_streaming_refusals():
    from sparch_amd import streaming
    net = _net(synapse=(0.0, 0.9)).eval()
    for kw, match in ((dict(fused=True), "fused"), (dict(fused=True, sparse=True), "sparse"), (dict(graph=True), "graph")):
        with pytest.raises(ValueError, match=match):
            streaming.StreamingSNN(net, 3, **kw)
    streaming.StreamingSNN(net, 3)
    streaming.StreamingSNN(_net().eval(), 3, fused=True, sparse=True)      # (without a synapse nothing changes)


def test_streaming_state_gains_i_only_with_a_synapse():
    from tools import layer_call_trace as lct
    from sparch_amd import snns, streaming
    B, Tc, K, H, C = 4, 3, 32, 128, 5
    states = [(torch.zeros(B, H), None, torch.zeros(B, H)) for _ in range(2)] + [torch.zeros(B, C)]
    rec = lct._Recorder()
    with lct._tracing(rec):
        rec.new_case("case")
        for syn in (None, (0.0, 0.9)):
            net = snns.SNN((B, None, K), [H, H, C], neuron_type="LIF", synapse=syn, synapse_layers="hidden").eval()
            st = streaming.StreamingSNN(net, B)
            st.reset(states=states)
            st.step(torch.zeros(B, Tc, K))
            st.step(torch.zeros(B, 1, K))
            state = st.get_state()
            if syn is None:
                assert all("i" not in s for s in state)
                continue
            assert "i" not in state[0] and state[1]["i"].shape == (B, H) and "i" not in state[2]
            st._layers[1].i.fill_(1.0)
            st.reset(states=[tuple(None if t is None else t[:2] for t in s) if isinstance(s, tuple) else s[:2]
                             for s in states], rows=[1, 3])
            assert st._layers[1].i[:, 0].tolist() == [1.0, 0.0, 1.0, 0.0]
            st.set_state(state)
            assert not st._layers[1].i.any()
    calls = _calls(rec.lines, "sparch_synapse_fwd")
    assert len(calls) == 2 and calls[0].startswith("sparch_synapse_fwd(4, 3, 128,")
    assert calls[1].startswith("sparch_synapse_fwd(4, 1, 128,")


# ------------------------------------------------------------------------------------------------ SPARCH_SYNAPSE
def test_sparch_synapse_parsing():
    from sparch_amd import exp
    assert exp.parse_synapse(None) is None and exp.parse_synapse("") is None and exp.parse_synapse("  ") is None
    base = {"synapse": (0.0, 0.9), "syn_init": "uniform", "learn_synapse": True, "synapse_layers": "all"}
    assert exp.parse_synapse("0:0.9") == base and exp.parse_synapse(" 0 : 0.9 ") == base
    assert exp.parse_synapse("0:0.9:uniform") == base
    assert exp.parse_synapse("0:0.9:lo") == dict(base, syn_init="lo")
    assert exp.parse_synapse("0.5:0.5:fixed") == dict(base, synapse=(0.5, 0.5), learn_synapse=False)
    assert exp.parse_synapse("0.1:0.95:lo:fixed:hidden") == {"synapse": (0.1, 0.95), "syn_init": "lo",
                                                             "learn_synapse": False, "synapse_layers": "hidden"}
    assert exp.parse_synapse("0:0.9:hidden:lo") == dict(base, syn_init="lo", synapse_layers="hidden")
    for bad in ("0", "0.9", "0:1", "0:1.5", "-0.1:0.5", "0.6:0.5", "a:b", "0:0.9:", "0:0.9:zero", "0:0.9:lo:uniform",
                "0:0.9:fixed:fixed", "0:0.9:hidden:hidden", ":0.9", "0,0.9", "nan:0.5", "0:nan"):
        with pytest.raises(ValueError, match="SPARCH_SYNAPSE"):
            exp.parse_synapse(bad)


def test_experiment_refuses_synapse_combinations_before_anything_else(monkeypatch, tmp_path):
    from sparch_amd import exp

    def args(**kw):
        base = dict(model_type="adLIF", sync_bn=False, use_pretrained_model=False, bidirectional=False,
                    compute_dtype="fp32", new_exp_folder=str(tmp_path / "never"))
        base.update(kw)
        return argparse.Namespace(**base)

    for name in ("SPARCH_LENGTHS", "SPARCH_PER_STEP_LOSS", "SPARCH_READOUT", "SPARCH_SURROGATE", "SPARCH_CLIP_GRAD",
                 "SPARCH_TBPTT", "SPARCH_DELAYS"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SPARCH_SYNAPSE", "slow")
    with pytest.raises(ValueError, match="SPARCH_SYNAPSE"):
        exp.Experiment(args())
    monkeypatch.setenv("SPARCH_SYNAPSE", "0:0.9")
    for model in ("MLP", "RNN", "LiGRU", "GRU"):
        with pytest.raises(ValueError, match="SPARCH_SYNAPSE needs a spiking model"):
            exp.Experiment(args(model_type=model))
    monkeypatch.setenv("SPARCH_LENGTHS", "pack")
    with pytest.raises(ValueError, match="SPARCH_LENGTHS=pack with --bidirectional"):   # (refused with or without a synapse)
        exp.Experiment(args(bidirectional=True))
    with pytest.raises(ValueError, match="SPARCH_SYNAPSE with --bidirectional and SPARCH_LENGTHS=pack"):
        exp.Experiment(args(bidirectional=True, use_pretrained_model=True))
    monkeypatch.delenv("SPARCH_LENGTHS")
    monkeypatch.setenv("SPARCH_TBPTT", "8")
    with pytest.raises(ValueError, match="SPARCH_SYNAPSE with SPARCH_TBPTT"):
        exp.Experiment(args())
    assert not (tmp_path / "never").exists()
