"""
Stateful training (SNN.forward(x, state=..., return_state=True), the `_st` entry points) without a GPU:
  * every refusal of DESIGN.md section 7 is a ValueError before any kernel (the C binding is replaced by one that fails
    on any call);
  * the `_st` entry points return SPARCH_EINVAL before any device work for what they do not take;
  * SPARCH_TBPTT parsing and its refusals; detach_state; the default path's committed layer call trace is unchanged;
  * the ABI is additive and prototypes = header.
"""
import argparse
import os
import re

import pytest
import torch

from tests.entry_probes import KIND, MIS, WS, Entry, P, T, head, ptrs
from tests.kit import EALIGN, EINVAL, EWORKSPACE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SG = [("surrogate", 0), ("surrogate_scale", 0.0)]
ST = ptrs("g_uT g_wT g_sT g_u0 g_w0 g_s0")
CELL_ST = Entry("sparch_cell_bwd_st", head(("kind", 1)) + ptrs("g_out g_rate u_save w_save", "g_rate") + [("save_bf16", 0)]
                + ptrs("alpha beta a b u0 w0 s0") + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)]
                + ptrs("dWx dparam_ws bn_x bn_mean bn_invstd", "bn_x bn_mean bn_invstd") + SG + ST + [("stream", None)])
RO_ST = Entry("sparch_readout_bwd_st", [("B", 2), ("T", T), ("C", 5)]
              + ptrs("g_out bn_x bn_mean bn_invstd u_save alpha u0 dWx dalpha_ws", "bn_x bn_mean bn_invstd")
              + ptrs("g_uT g_u0") + [("stream", None)])
REC_ST = Entry("sparch_rec_cell_bwd_st", head(KIND) + ptrs("g_out g_rate u_save w_save", "g_rate") + [("save_bf16", 0)]
               + ptrs("alpha beta a b vpack_t u0 w0 s0") + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)]
               + ptrs("dWx s_prev16 dparam_ws bn_x bn_mean bn_invstd", "bn_x bn_mean bn_invstd") + WS[:-1] + SG + ST
               + [("stream", None), ("precision", 0)])


# ------------------------------------------------------------------------------------------------ the C ABI
def test_rec_st_entry_refuses_before_any_device_work():
    """Nothing here reaches a launch: a valid call ends at its workspace check (chan = NULL)."""
    from sparch_amd._capi import PROTOTYPES
    e = REC_ST
    assert len(e.args) == len(PROTOTYPES[e.name][1]) == len(PROTOTYPES["sparch_rec_cell_bwd_sg"][1]) + 6
    assert e() == EWORKSPACE
    assert e(steps_per_launch=T - 1) == EINVAL and e(steps_per_launch=1) == EINVAL and e(steps_per_launch=T + 5) == EWORKSPACE
    assert e(dirs=2) == EINVAL and e(dirs=0) == EINVAL
    assert e(save_bf16=1) == EINVAL
    assert e(precision=1) == EINVAL and e(precision=7) == EINVAL           # the bf16 operand mode
    assert e(H=1028) == EINVAL and e(H=2048) == EINVAL and e(H=10) == EINVAL
    assert e(surrogate=9) == EINVAL and e(surrogate=2, surrogate_scale=0.0) == EINVAL
    assert e(kind=0) == EINVAL and e(kind=1) == EINVAL                     # LIF / adLIF have their own entry point
    for k in ("g_out", "u_save", "alpha", "vpack_t", "u0", "s0", "dWx", "s_prev16", "dparam_ws", "status", "beta", "a", "b",
              "w0", "w_save"):
        assert e(**{k: None}) == EINVAL, k
    assert e(kind=2, beta=None, a=None, b=None, w0=None, w_save=None) == EWORKSPACE     # RLIF reads none of them
    assert e(B=0) == EINVAL and e(T=0) == EINVAL and e(bn_x=P) == EINVAL
    assert e(steps_per_launch=1, g_uT=MIS) == EINVAL and e(B=0, g_s0=MIS) == EINVAL    # in front of the alignment check
    for k in ("g_out", "g_uT", "g_wT", "g_sT", "g_u0", "g_w0", "g_s0"):
        assert e(**{k: MIS}) == EALIGN, k


def test_abi_is_additive_and_prototypes_are_the_header():
    from sparch_amd._capi import PROTOTYPES, lib
    assert lib.sparch_abi_version() == 5
    with open(os.path.join(ROOT, "include", "sparch_hip.h")) as f:
        header = f.read()
    for e, sibling, extra in ((CELL_ST, "sparch_cell_bwd_sg", 6), (RO_ST, "sparch_readout_bwd", 2)):
        assert len(e.args) == len(PROTOTYPES[e.name][1]) == len(PROTOTYPES[sibling][1]) + extra, e.name
        assert PROTOTYPES[e.name][1][:len(PROTOTYPES[sibling][1]) - 1] == PROTOTYPES[sibling][1][:-1]
        decl = re.search(r"\bint " + e.name + r"\(([^;]*)\);", header)
        assert decl, e.name
        params = [q.strip() for q in decl.group(1).replace("\n", " ").split(",")]
        assert len(params) == len(e.args), e.name
        assert "const float* g_uT" in params and "float* g_u0" in params and params[-1] == "void* stream"
        assert hasattr(lib, e.name)
    declared = set(re.findall(r"\b(sparch_\w+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(PROTOTYPES)


def test_cell_st_entry_refuses_before_any_device_work():
    """Nothing here reaches a launch: the entry is only ever called with something broken."""
    e = CELL_ST
    assert e(dirs=2) == EINVAL and e(dirs=0) == EINVAL
    assert e(save_bf16=1) == EINVAL
    assert e(surrogate=9) == EINVAL and e(surrogate=-1) == EINVAL
    assert e(surrogate=2, surrogate_scale=0.0) == EINVAL and e(surrogate=1, surrogate_scale=float("nan")) == EINVAL
    assert e(kind=2) == EINVAL and e(kind=3) == EINVAL           # the recurrent kinds have their own entry points
    for k in ("g_out", "u_save", "alpha", "u0", "s0", "dWx", "dparam_ws", "beta", "a", "b", "w0", "w_save"):
        assert e(**{k: None}) == EINVAL, k
    assert e(B=0) == EINVAL and e(T=0) == EINVAL and e(H=0) == EINVAL
    assert e(p_drop=1.0) == EINVAL and e(p_drop=-0.1) == EINVAL
    assert e(bn_x=P) == EINVAL                                     # the raw projection without its statistics
    # these refusals stand in front of the alignment check, like every other SPARCH_EINVAL
    assert e(dirs=2, g_out=MIS) == EINVAL and e(save_bf16=1, g_uT=MIS) == EINVAL
    for k in ("g_out", "g_uT", "g_wT", "g_sT", "g_u0", "g_w0", "g_s0"):
        assert e(**{k: MIS}) == EALIGN, k


def test_readout_st_entry_refuses_before_any_device_work():
    e = RO_ST
    for k in ("g_out", "u_save", "alpha", "u0", "dWx", "dalpha_ws"):
        assert e(**{k: None}) == EINVAL, k
    assert e(B=0) == EINVAL and e(T=0) == EINVAL and e(C=0) == EINVAL and e(C=257) == EINVAL
    assert e(bn_x=P) == EINVAL


# ------------------------------------------------------------------------------------------------ Python refusals
class _NoCalls:
    """In the place of the C binding: any entry point that is looked up fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the C library was called ({name}) before the refusal")


def _net(kw=None, kind="LIF", sizes=(8, 8, 5)):
    import sparch_amd
    return sparch_amd.SNN((3, None, 6), list(sizes), neuron_type=kind, **(kw or {}))


X = torch.zeros(3, 4, 6)


def _state(net, batch=3):
    st = []
    for lay in net.snn:
        d = {"u": torch.zeros(batch, lay.hidden_size)}
        if getattr(lay, "kind", None) in ("adLIF", "RadLIF"):
            d["w"] = torch.zeros(batch, lay.hidden_size)
        if hasattr(lay, "kind"):
            d["s"] = torch.zeros(batch, lay.hidden_size)
        st.append(d)
    return st


def test_every_python_refusal_is_a_value_error_before_any_kernel(monkeypatch):
    from sparch_amd import functional as Fn
    from sparch_amd import snns
    monkeypatch.setattr(Fn, "lib", _NoCalls())
    both = (dict(return_state=True), None)      # return_state alone, and a state given (filled in per network below)

    def refused(net, match, **kw):
        for form in both:
            args = dict(form) if form is not None else dict(state=_state(net))
            with pytest.raises(ValueError, match=match):
                net(X, **args, **kw)

    refused(_net(dict(bidirectional=True)), "bidirectional")
    refused(_net(), "lengths", lengths=torch.tensor([4, 1, 2]))
    refused(_net(), "pack", lengths=torch.tensor([4, 1, 2]), pack=True)
    refused(_net(), "per_step", per_step="sum")
    for readout in ("softmax_mean", "u_max", "u_mean", "u_last"):
        refused(_net(dict(readout=readout)), "readout")
    for kind in ("RLIF", "RadLIF"):             # recurrent layers: above 1024 units, and the degraded / chunked launch modes
        refused(_net(kind=kind, sizes=(8, 1028, 5)), "above 1024")
        monkeypatch.setenv("SPARCH_REC_STEP_PATH", "1")
        refused(_net(kind=kind), "above 1024")
        monkeypatch.delenv("SPARCH_REC_STEP_PATH")
        for steps in ("1", "3"):                # one launch per step (what a timeout degrades to), and chunks of 3 of T = 4
            monkeypatch.setenv("SPARCH_REC_STEPS_PER_LAUNCH", steps)
            refused(_net(kind=kind), "degraded or chunked")
        monkeypatch.setenv("SPARCH_REC_STEPS_PER_LAUNCH", "4")      # whole sequences: accepted (the device check stops it)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _net(kind=kind)(X, return_state=True)
        monkeypatch.delenv("SPARCH_REC_STEPS_PER_LAUNCH")
    _net(kind="LIF", sizes=(8, 1028, 5))        # (a non-recurrent layer of that width has no per-step path)
    monkeypatch.setattr(Fn, "SAVE_BF16", True)
    refused(_net(), "SPARCH_SAVE_DTYPE")
    monkeypatch.setattr(Fn, "SAVE_BF16", False)
    prev = Fn.set_compute_dtype("bf16")
    try:
        refused(_net(), "bf16 operand mode")
    finally:
        Fn.set_compute_dtype(prev)
    net = _net()
    net._static_states = object()       # (what GraphedTrainStep sets for the life of its captured step)
    refused(net, "captured step")
    del net._static_states
    # the state itself
    net = _net(kind="adLIF")
    good = _state(net)
    for bad, match in ((good[:2], "entries"), ([dict(good[0], u=torch.zeros(2, 8))] + good[1:], "expected"),
                       ([{"u": good[0]["u"], "s": good[0]["s"]}] + good[1:], "'w'"),
                       ([dict(good[0], s=torch.zeros(3, 8, dtype=torch.float64))] + good[1:], "float32")):
        with pytest.raises(ValueError, match=match):
            net(X, state=bad)
    # the layers' own forms
    with pytest.raises(ValueError, match="lengths"):
        net.snn[0].forward_with_rate(X, lengths=(torch.tensor([4, 1, 2], dtype=torch.int32), 7), return_state=True)
    with pytest.raises(ValueError, match="per_step"):
        net.snn[-1](torch.zeros(3, 4, 8), per_step="sum", return_state=True)
    # accepted: nothing above stands in the way of use_readout_layer=False with return_state=True, or of the plain
    # network — the device check is what stops a host tensor
    monkeypatch.undo()
    for n in (_net(dict(use_readout_layer=False), sizes=(8, 8)), _net()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            n(X, return_state=True)
    assert snns.detach_state is not None


def test_detach_state_cuts_every_tensor_out_of_the_graph():
    from sparch_amd.snns import detach_state
    w = torch.ones(2, 3, requires_grad=True)
    st = [{"u": w * 2, "w": w * 3, "s": w * 4}, {"u": w * 5}]
    cut = detach_state(st)
    assert [sorted(d) for d in cut] == [sorted(d) for d in st]
    for a, b in zip(cut, st):
        for k in a:
            assert not a[k].requires_grad and a[k].grad_fn is None and torch.equal(a[k], b[k])
            assert a[k].data_ptr() == b[k].data_ptr()           # no copy


def test_sparch_tbptt_parsing():
    from sparch_amd import exp
    assert exp.parse_tbptt(None) is None and exp.parse_tbptt("") is None and exp.parse_tbptt("  ") is None
    assert exp.parse_tbptt("1") == 1 and exp.parse_tbptt("8") == 8 and exp.parse_tbptt(" 250 ") == 250
    for bad in ("0", "-3", "8.0", "eight", "1e2", "8:2", "inf"):
        with pytest.raises(ValueError, match="SPARCH_TBPTT"):
            exp.parse_tbptt(bad)


def test_experiment_refuses_tbptt_combinations_before_anything_else(monkeypatch, tmp_path):
    from sparch_amd import exp

    def args(**kw):
        base = dict(model_type="adLIF", sync_bn=False, use_pretrained_model=False, bidirectional=False,
                    compute_dtype="fp32", new_exp_folder=str(tmp_path / "never"))
        base.update(kw)
        return argparse.Namespace(**base)

    for name in ("SPARCH_LENGTHS", "SPARCH_PER_STEP_LOSS", "SPARCH_READOUT", "SPARCH_SURROGATE", "SPARCH_CLIP_GRAD"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SPARCH_TBPTT", "zero")
    with pytest.raises(ValueError, match="SPARCH_TBPTT"):
        exp.Experiment(args())
    monkeypatch.setenv("SPARCH_TBPTT", "8")
    for kw, match in ((dict(bidirectional=True), "--bidirectional"), (dict(sync_bn=True), "--sync_bn"),
                      (dict(model_type="MLP"), "spiking model"), (dict(model_type="GRU"), "spiking model"),
                      (dict(compute_dtype="bf16"), "bf16")):
        with pytest.raises(ValueError, match=match):
            exp.Experiment(args(**kw))
    for name, value in (("SPARCH_LENGTHS", "mask"), ("SPARCH_LENGTHS", "pack"), ("SPARCH_PER_STEP_LOSS", "0.5"),
                        ("SPARCH_READOUT", "u_max")):
        monkeypatch.setenv(name, value)
        with pytest.raises(ValueError, match=f"SPARCH_TBPTT with {name}"):
            exp.Experiment(args())
        monkeypatch.delenv(name)
    assert not (tmp_path / "never").exists()


# ------------------------------------------------------------------------------------------------ the calls issued
def test_a_stateful_layer_issues_the_st_entries_call_for_call():
    """The stateful layer issues the plain forward and, in the plain backward's place, the `_st` entry point."""
    from tools import layer_call_trace as lct

    import sparch_amd

    def traced(stateful):
        def run(lct):
            torch.manual_seed(0)
            lay = sparch_amd.adLIFLayer(32, 128, 4)
            ro = sparch_amd.ReadoutLayer(128, 5, 4)
            x = torch.zeros(4, 3, 32)
            states = tuple(torch.zeros(4, 128, requires_grad=stateful) for _ in range(3))
            s, rate, *st = lay.forward_with_rate(x, states=states, **({"return_state": True} if stateful else {}))
            out, *st_ro = ro(s, u0=torch.zeros(4, 5, requires_grad=stateful), **({"return_state": True} if stateful else {}))
            loss = out.sum() + rate.sum()
            if stateful:
                loss = loss + sum(v.sum() for v in st[0].values()) + st_ro[0]["u"].sum()
            loss.backward()
            if stateful:
                assert all(t.grad is not None and t.grad.shape == (4, 128) for t in states)
        return [ln.split("(")[0] for ln in lct.traced(run)]

    plain, st = traced(False), traced(True)
    swap = {"sparch_cell_bwd_st": "sparch_cell_bwd", "sparch_readout_bwd_st": "sparch_readout_bwd"}
    assert "sparch_cell_bwd" in plain and "sparch_readout_bwd" in plain and not any(n.endswith("_st") for n in plain)
    assert "sparch_cell_bwd_st" in st and "sparch_readout_bwd_st" in st
    assert "sparch_cell_bwd" not in st and "sparch_readout_bwd" not in st
    assert [swap.get(n, n) for n in st] == plain
