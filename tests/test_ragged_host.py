"""
Ragged batches (SNN.forward(x, lengths), the `_len` entry points) without a GPU:
  * every refusal of DESIGN.md section 7, at the Python level and at the C ABI (SPARCH_EINVAL before any device work);
  * lengths=None leaves the committed layer call trace unchanged, lengths given issues the `_len` entry points with the
    lengths, their sum and (backward) the surrogate, and BatchNorm's count becomes the number of valid rows;
  * SPARCH_LENGTHS parsing; the ABI is additive and prototypes = header.
"""
import os
import re

import pytest
import torch

from tests.entry_probes import KIND, MIS, WS, Entry, P, T, head, ptrs
from tests.kit import EALIGN, EINVAL, EWORKSPACE
from tools.layer_call_trace import traced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEN = [("lengths", P), ("n_valid", 5)]
SG = [("surrogate", 0), ("surrogate_scale", 0.0)]
CELL_FWD = Entry("sparch_cell_fwd_len", head(("kind", 1)) + ptrs("Wx scale shift alpha beta a b u0 w0 s0", "scale shift")
                 + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)] + ptrs("s_out s16_out u_save w_save", "s16_out")
                 + [("save_bf16", 0), ("spike_count", None)] + LEN + [("stream", None)])
CELL_BWD = Entry("sparch_cell_bwd_len", head(("kind", 1)) + ptrs("g_out g_rate u_save w_save", "g_rate") + [("save_bf16", 0)]
                 + ptrs("alpha beta a b u0 w0 s0") + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)]
                 + ptrs("dWx dparam_ws bn_x bn_mean bn_invstd", "bn_x bn_mean bn_invstd") + LEN + SG + [("stream", None)])
REC_FWD = Entry("sparch_rec_cell_fwd_len", head(KIND) + ptrs("Wx scale shift alpha beta a b vpack rec0 u0 w0 s0", "scale shift")
                + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)] + ptrs("s_out s16_out u_save w_save", "s16_out")
                + [("save_bf16", 0), ("spike_count", None)] + LEN + WS + [("precision", 0)])
REC_BWD = Entry("sparch_rec_cell_bwd_len", head(KIND) + ptrs("g_out g_rate u_save w_save", "g_rate") + [("save_bf16", 0)]
                + ptrs("alpha beta a b vpack_t u0 w0 s0") + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)]
                + ptrs("dWx s_prev16 dparam_ws bn_x bn_mean bn_invstd", "bn_x bn_mean bn_invstd") + LEN + WS[:-1] + SG
                + [("stream", None), ("precision", 0)])
RO_FWD = Entry("sparch_readout_fwd_len", [("B", 2), ("T", T), ("C", 5)] + ptrs("Wx scale shift alpha u0 out u_save", "scale shift")
               + LEN + [("stream", None)])
RO_BWD = Entry("sparch_readout_bwd_len", [("B", 2), ("T", T), ("C", 5)]
               + ptrs("g_out bn_x bn_mean bn_invstd u_save alpha u0 dWx dalpha_ws", "bn_x bn_mean bn_invstd") + LEN
               + [("stream", None)])
ENTRIES = (CELL_FWD, CELL_BWD, REC_FWD, REC_BWD, RO_FWD, RO_BWD)
SIBLING = {CELL_FWD: ("sparch_cell_fwd", 2), CELL_BWD: ("sparch_cell_bwd", 4), REC_FWD: ("sparch_rec_cell_fwd", 2),
           REC_BWD: ("sparch_rec_cell_bwd", 4), RO_FWD: ("sparch_readout_fwd", 2), RO_BWD: ("sparch_readout_bwd", 2)}
ids = lambda e: e.name  # noqa: E731


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_is_additive_and_prototypes_are_the_header():
    from sparch_amd._capi import PROTOTYPES, lib
    assert lib.sparch_abi_version() == 5
    with open(os.path.join(ROOT, "include", "sparch_hip.h")) as f:
        header = f.read()
    for e in ENTRIES:
        sibling, extra = SIBLING[e]
        assert len(e.args) == len(PROTOTYPES[e.name][1]) == len(PROTOTYPES[sibling][1]) + extra, e.name
        decl = re.search(r"\bint " + e.name + r"\(([^;]*)\);", header)
        assert decl, e.name
        params = [q.strip() for q in decl.group(1).replace("\n", " ").split(",")]
        assert len(params) == len(e.args), e.name
        assert "const int* lengths" in params and "long long n_valid" in params
        assert params.index("long long n_valid") == params.index("const int* lengths") + 1
        assert hasattr(lib, e.name)
    declared = set(re.findall(r"\b(sparch_\w+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(PROTOTYPES)


@pytest.mark.parametrize("e", ENTRIES, ids=ids)
def test_len_entries_refuse_before_any_device_work(e):
    """Nothing here reaches a launch: the persistent entries end at their workspace check (chan = NULL), the others are
    only ever called with something broken."""
    assert e(lengths=None) == EINVAL
    for n in (0, -1, -(1 << 40)):
        assert e(n_valid=n) == EINVAL, n
    if any(k == "dirs" for k, _ in e.args):
        assert e(dirs=2) == EINVAL and e(dirs=0) == EINVAL
        first = next(k for k, v in e.args if v == P)
        # the ragged checks come first: in front of the alignment check, like every other SPARCH_EINVAL
        assert e(lengths=None, **{first: MIS}) == EINVAL and e(dirs=2, **{first: MIS}) == EINVAL
        assert e(**{first: MIS}) == EALIGN
    # the sibling's own refusals still hold behind them
    assert e(B=0) == EINVAL and e(T=0) == EINVAL and e(alpha=None) == EINVAL
    if e in (REC_FWD, REC_BWD):
        assert e() == EWORKSPACE and e(n_valid=1 << 40) == EWORKSPACE    # a valid call up to its workspace: chan is NULL
        assert e(precision=7) == EINVAL and e(H=2048) == EINVAL
    if e in (CELL_BWD, REC_BWD):
        assert e(surrogate=9) == EINVAL and e(surrogate=2, surrogate_scale=0.0) == EINVAL
        assert e(surrogate=2, surrogate_scale=5.0, save_bf16=1) == EINVAL
    if e is REC_FWD:
        assert e(save_bf16=1, steps_per_launch=1) == EINVAL


# ------------------------------------------------------------------------------------------------ Python refusals
def _net(sp_kw=None, kind="LIF", sizes=(8, 8, 5)):
    import sparch_amd
    return sparch_amd.SNN((3, None, 6), list(sizes), neuron_type=kind, **(sp_kw or {}))


X, LENS = torch.zeros(3, 4, 6), torch.tensor([4, 1, 2])


def test_every_python_refusal_is_a_value_error(monkeypatch):
    from sparch_amd import functional as Fn
    from sparch_amd import snns
    with pytest.raises(ValueError, match="bidirectional"):
        _net(dict(bidirectional=True))(X, lengths=LENS)
    with pytest.raises(ValueError, match="above 1024"):
        _net(kind="RLIF", sizes=(8, 1028, 5))(X, lengths=LENS)
    _net(kind="LIF", sizes=(8, 1028, 5))  # (a non-recurrent layer of that width has no per-step path)
    with pytest.raises(ValueError, match="use_bias"):
        _net(dict(use_bias=True, normalization="batchnorm"))(X, lengths=LENS)
    monkeypatch.setattr(Fn, "SYNC_BN", {"group": None, "world": 2})
    with pytest.raises(ValueError, match="sync_bn"):
        _net()(X, lengths=LENS)
    monkeypatch.setattr(Fn, "SYNC_BN", None)
    net = _net()
    net._static_states = object()       # (what GraphedTrainStep sets for the life of its captured step)
    with pytest.raises(ValueError, match="captured step"):
        net(X, lengths=LENS)
    del net._static_states
    # the lengths themselves
    for bad in (torch.tensor([4, 0, 2]), torch.tensor([5, 1, 2]), torch.tensor([4, 1]), torch.tensor([4.0, 1.0, 2.0]),
                torch.tensor([[4, 1, 2]])):
        with pytest.raises(ValueError, match="lengths"):
            net(X, lengths=bad)
    with pytest.raises(ValueError, match="prepare_lengths"):
        net.snn[0].forward_with_rate(X, lengths=LENS)
    # with bias under LayerNorm or no normalisation nothing is refused: the device check is what stops a host tensor
    for norm in ("layernorm", "none"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _net(dict(use_bias=True, normalization=norm))(X, lengths=LENS)
    lens_dev, n = snns.prepare_lengths([4, 1, 2], 3, 4, "cpu")
    assert lens_dev.dtype == torch.int32 and lens_dev.tolist() == [4, 1, 2] and n == 7


def test_baselines_and_streams_refuse_lengths():
    import sparch_amd
    from sparch_amd import streaming, streaming_ann
    from sparch_amd.anns import ANN
    ann = ANN((3, None, 6), [8, 5], ann_type="MLP")
    with pytest.raises(ValueError, match="non-spiking"):
        ann(X, lengths=LENS)
    for cls in (streaming.StreamingSNN, streaming_ann.StreamingANN):
        with pytest.raises(ValueError, match="streaming"):
            cls.step(object.__new__(cls), X, lengths=LENS)


def test_sparch_lengths_parsing(monkeypatch):
    from sparch_amd import exp
    assert exp.parse_lengths_mode(None) is False and exp.parse_lengths_mode("") is False
    assert exp.parse_lengths_mode("mask") is True
    for bad in ("1", "Mask", "mask ", "on", "truncate"):
        with pytest.raises(ValueError, match="SPARCH_LENGTHS"):
            exp.parse_lengths_mode(bad)


def test_experiment_refuses_a_bad_value_before_anything_else(monkeypatch, tmp_path):
    """A malformed SPARCH_LENGTHS, mask with --sync_bn and mask with a baseline model end the run before folders, data
    or device are touched."""
    from sparch_amd import exp
    import argparse

    def args(**kw):
        return argparse.Namespace(model_type="LIF", sync_bn=False, use_pretrained_model=False,
                                  new_exp_folder=str(tmp_path / "never"), **kw)
    monkeypatch.setenv("SPARCH_LENGTHS", "yes")
    with pytest.raises(ValueError, match="SPARCH_LENGTHS"):
        exp.Experiment(args())
    monkeypatch.setenv("SPARCH_LENGTHS", "mask")
    with pytest.raises(ValueError, match="sync_bn"):
        exp.Experiment(argparse.Namespace(**dict(vars(args()), sync_bn=True)))
    with pytest.raises(ValueError, match="spiking model"):
        exp.Experiment(argparse.Namespace(**dict(vars(args()), model_type="MLP")))
    assert not (tmp_path / "never").exists()


# ------------------------------------------------------------------------------------------------ the calls issued
def layer_case(kind, lengths, norm="batchnorm"):
    def run(lct):
        x, xcfg = lct._input("dense", 4, 3, 32, True)
        cfg = dict(xcfg, **({} if lengths is None else {"lengths": lengths}))
        s, rate, _ = lct._spiking(x, cfg, kind, norm, 1, 128)
        lct._backward(s, rate)
    return run


@pytest.mark.parametrize("kind,fwd,bwd", [("adLIF", "sparch_cell_fwd", "sparch_cell_bwd"),
                                          ("RadLIF", "sparch_rec_cell_fwd", "sparch_rec_cell_bwd")])
def test_a_layer_with_lengths_issues_the_len_entries(kind, fwd, bwd):
    lengths = (torch.tensor([3, 1, 2, 3], dtype=torch.int32), 9)
    plain, ragged = traced(layer_case(kind, None)), traced(layer_case(kind, lengths))
    assert len(plain) == len(ragged)         # call for call: only the entries and their arguments differ
    names = lambda lines: [ln.split("(")[0] for ln in lines]  # noqa: E731
    assert not any(n.endswith("_len") for n in names(plain))
    assert fwd in names(plain) and bwd in names(plain)
    assert fwd + "_len" in names(ragged) and bwd + "_len" in names(ragged)
    assert fwd not in names(ragged) and bwd not in names(ragged)
    f = next(ln for ln in ragged if ln.startswith(fwd + "_len("))
    b = next(ln for ln in ragged if ln.startswith(bwd + "_len("))
    assert "i32[4]" in f and ", 9, " in f and "i32[4]" in b and ", 9, " in b
    assert ", 0, 0.0, NULL" in b             # the box-car, in front of the stream
    # BatchNorm's count: the valid rows instead of all 12
    fin_p = next(ln for ln in plain if ln.startswith("sparch_bn_finalize("))
    fin_r = next(ln for ln in ragged if ln.startswith("sparch_bn_finalize("))
    assert fin_p.startswith("sparch_bn_finalize(128, 12, ") and fin_r.startswith("sparch_bn_finalize(128, 9, ")
