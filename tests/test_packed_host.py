"""
Packed ragged batches (SNN.forward(x, lengths, pack=True), the `_pk` entry points) without a GPU:
  * every `_pk` entry is declared in the header, bound in _capi.PROTOTYPES and refuses before any device work;
  * snns.prepare_packing: stable descending order, exclusive prefix sum, N, the refusals of prepare_lengths;
  * the numpy restatement of pack / unpack (tests/packed_numpy.py) round-trips and pins layout and tail zeros;
  * SPARCH_LENGTHS parsing and every Python refusal of DESIGN.md section 7;
  * without pack=True the committed layer call trace is unchanged.
"""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from tests import packed_numpy as pn
from tests.entry_probes import KIND, MIS, WS, Entry, P, T, head, ptrs
from tests.kit import EALIGN, EINVAL, EWORKSPACE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PK = [("lengths", P), ("offsets", P), ("n_valid", 5)]
SG = [("surrogate", 0), ("surrogate_scale", 0.0)]
CELL_FWD = Entry("sparch_cell_fwd_pk", head(("kind", 1)) + ptrs("Wx scale shift alpha beta a b u0 w0 s0", "scale shift")
                 + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)] + ptrs("s_out s16_out u_save w_save", "s16_out")
                 + [("save_bf16", 0), ("spike_count", None)] + PK + [("stream", None)])
CELL_BWD = Entry("sparch_cell_bwd_pk", head(("kind", 1)) + ptrs("g_out g_rate u_save w_save", "g_rate") + [("save_bf16", 0)]
                 + ptrs("alpha beta a b u0 w0 s0") + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)]
                 + ptrs("dWx dparam_ws bn_x bn_mean bn_invstd", "bn_x bn_mean bn_invstd") + PK + SG + [("stream", None)])
REC_FWD = Entry("sparch_rec_cell_fwd_pk", head(KIND) + ptrs("Wx scale shift alpha beta a b vpack rec0 u0 w0 s0", "scale shift")
                + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)] + ptrs("s_out s16_out u_save w_save", "s16_out")
                + [("save_bf16", 0), ("spike_count", None)] + PK + WS + [("precision", 0)])
REC_BWD = Entry("sparch_rec_cell_bwd_pk", head(KIND) + ptrs("g_out g_rate u_save w_save", "g_rate") + [("save_bf16", 0)]
                + ptrs("alpha beta a b vpack_t u0 w0 s0") + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)]
                + ptrs("dWx s_prev16 dparam_ws bn_x bn_mean bn_invstd", "bn_x bn_mean bn_invstd") + PK + WS[:-1] + SG
                + [("stream", None), ("precision", 0)])
RO_FWD = Entry("sparch_readout_fwd_pk", [("B", 2), ("T", T), ("C", 5)] + ptrs("Wx scale shift alpha u0 out u_save", "scale shift")
               + PK + [("stream", None)])
RO_BWD = Entry("sparch_readout_bwd_pk", [("B", 2), ("T", T), ("C", 5)]
               + ptrs("g_out bn_x bn_mean bn_invstd u_save alpha u0 dWx dalpha_ws", "bn_x bn_mean bn_invstd") + PK
               + [("stream", None)])
ROWS = [("B", 2), ("T", T), ("C", 8), ("elem_size", 4)] + ptrs("src dst order lengths offsets") + [("n_valid", 5), ("stream", None)]
PACK, UNPACK = Entry("sparch_pack_rows", ROWS), Entry("sparch_unpack_rows", ROWS)
ENTRIES = (CELL_FWD, CELL_BWD, REC_FWD, REC_BWD, RO_FWD, RO_BWD)
SIBLING = {CELL_FWD: "sparch_cell_fwd_len", CELL_BWD: "sparch_cell_bwd_len", REC_FWD: "sparch_rec_cell_fwd_len",
           REC_BWD: "sparch_rec_cell_bwd_len", RO_FWD: "sparch_readout_fwd_len", RO_BWD: "sparch_readout_bwd_len"}
ids = lambda e: e.name  # noqa: E731


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_is_additive_and_prototypes_are_the_header():
    from sparch_amd._capi import PROTOTYPES, lib
    assert lib.sparch_abi_version() == 5
    with open(os.path.join(ROOT, "include", "sparch_hip.h")) as f:
        header = f.read()
    for e in ENTRIES + (PACK, UNPACK):
        decl = re.search(r"\bint " + e.name + r"\(([^;]*)\);", header)
        assert decl, e.name
        params = [q.strip() for q in decl.group(1).replace("\n", " ").split(",")]
        assert len(params) == len(e.args) == len(PROTOTYPES[e.name][1]), e.name
        assert "const int* lengths" in params and "long long n_valid" in params
        assert params.index("const int* offsets") == params.index("const int* lengths") + 1
        assert params.index("long long n_valid") == params.index("const int* offsets") + 1
        assert hasattr(lib, e.name)
    for e in ENTRIES:  # the `_len` form's argument list with the offsets behind the lengths
        len_params = PROTOTYPES[SIBLING[e]][1]
        pk_params = PROTOTYPES[e.name][1]
        at = [k for k, _ in e.args].index("offsets")
        assert pk_params[:at] + pk_params[at + 1:] == len_params, e.name
    declared = set(re.findall(r"\b(sparch_\w+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(PROTOTYPES)


@pytest.mark.parametrize("e", ENTRIES, ids=ids)
def test_pk_entries_refuse_before_any_device_work(e):
    """Nothing here reaches a launch: every call has something broken."""
    assert e(lengths=None) == EINVAL and e(offsets=None) == EINVAL
    for n in (0, -1, -(1 << 40)):
        assert e(n_valid=n) == EINVAL, n
    if any(k == "dirs" for k, _ in e.args):
        assert e(dirs=2) == EINVAL and e(dirs=0) == EINVAL
        first = next(k for k, v in e.args if v == P)
        # the packed checks come first: in front of the alignment check, like every other SPARCH_EINVAL
        assert e(lengths=None, **{first: MIS}) == EINVAL and e(offsets=None, **{first: MIS}) == EINVAL
        assert e(dirs=2, **{first: MIS}) == EINVAL
        assert e(**{first: MIS}) == EALIGN
    # the sibling's own refusals still hold behind them
    assert e(B=0) == EINVAL and e(T=0) == EINVAL and e(alpha=None) == EINVAL
    if e in (REC_FWD, REC_BWD):
        assert e() == EWORKSPACE and e(n_valid=1 << 40) == EWORKSPACE    # a valid call up to its workspace: chan is NULL
        assert e(precision=7) == EINVAL and e(H=2048) == EINVAL
        assert e(steps_per_launch=T - 1) == EINVAL and e(steps_per_launch=1) == EINVAL       # whole sequences only
    if e in (CELL_BWD, REC_BWD):
        assert e(surrogate=9) == EINVAL and e(surrogate=2, surrogate_scale=0.0) == EINVAL
        assert e(surrogate=2, surrogate_scale=5.0, save_bf16=1) == EINVAL
    if e in (RO_FWD, RO_BWD):
        assert e(C=257) == EINVAL and e(u0=None) == EINVAL
    if e is CELL_FWD:
        assert e(kind=2) == EINVAL and e(p_drop=1.0) == EINVAL and e(s_out=None) == EINVAL   # (s16_out is NULL too)


@pytest.mark.parametrize("e", [PACK, UNPACK], ids=ids)
def test_row_movers_refuse_before_any_device_work(e):
    for k in ("src", "dst", "order", "lengths", "offsets"):
        assert e(**{k: None}) == EINVAL, k
    for size in (0, 3, 8):
        assert e(elem_size=size) == EINVAL, size
    assert e(B=0) == EINVAL and e(T=0) == EINVAL and e(C=0) == EINVAL
    assert e(n_valid=0) == EINVAL and e(n_valid=2 * T + 1) == EINVAL     # more rows than the padded tensor has


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("lengths,T_", [([4, 7, 4, 1, 7, 4], 7), ([3], 5), ([2, 2, 2], 2), ([1, 2, 3, 4], 9)])
def test_prepare_packing(lengths, T_):
    from sparch_amd import snns
    plan = snns.prepare_packing(lengths, len(lengths), T_, "cpu")
    order, lens, offsets, n = pn.plan_of(lengths)
    assert plan.order.dtype == plan.lengths.dtype == plan.offsets.dtype == torch.int32
    assert plan.order.tolist() == order.tolist()
    assert plan.lengths.tolist() == lens.tolist() == sorted(lengths, reverse=True)
    assert plan.offsets.tolist() == offsets.tolist() and plan.offsets.tolist()[0] == 0
    assert plan.n == n == sum(lengths) == plan.offsets.tolist()[-1]
    assert plan.t_max == max(lengths) and plan.batch == len(lengths) and plan.T == T_
    # stable: equal lengths keep the batch order
    for j in range(len(lengths) - 1):
        assert lens[j] > lens[j + 1] or order[j] < order[j + 1]
    assert plan.inverse[plan.order.long()].tolist() == list(range(len(lengths)))
    # one buffer: the four views are consecutive pieces of one allocation
    base = plan.order.data_ptr()
    assert plan.lengths.data_ptr() == base + 4 * len(lengths) and plan.offsets.data_ptr() == base + 8 * len(lengths)
    for k, h in enumerate(plan.host):
        assert h.tolist() == (plan.order, plan.lengths, plan.offsets)[k].tolist()
    # a tensor of lengths, int64 or int32, gives the same plan
    for dt in (torch.int64, torch.int32):
        again = snns.prepare_packing(torch.tensor(lengths, dtype=dt), len(lengths), T_, "cpu")
        assert again.order.tolist() == plan.order.tolist() and again.n == plan.n


def test_prepare_packing_refuses_what_prepare_lengths_refuses():
    from sparch_amd import snns
    for bad in (torch.tensor([4, 0, 2]), torch.tensor([5, 1, 2]), torch.tensor([4, 1]), torch.tensor([4.0, 1.0, 2.0]),
                torch.tensor([[4, 1, 2]]), torch.tensor([True, True, False])):
        with pytest.raises(ValueError) as a:
            snns.prepare_lengths(bad, 3, 4, "cpu")
        with pytest.raises(ValueError) as b:
            snns.prepare_packing(bad, 3, 4, "cpu")
        assert str(a.value) == str(b.value) and "lengths" in str(b.value)


# ------------------------------------------------------------------------------------------------ pack / unpack restated
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16, np.float32])
def test_the_restatement_round_trips_and_pins_the_layout(dtype):
    lengths, T_, C = [23, 1, 9, 17, 2, 22], 23, 5
    rng = np.random.default_rng(3)
    x = rng.integers(1, 200, (len(lengths), T_, C)).astype(dtype)        # (no zeros: a zero is a tail)
    xp = pn.pack(x, lengths)
    order, lens, offsets, n = pn.plan_of(lengths)
    assert order.tolist() == [0, 5, 3, 2, 4, 1] and lens.tolist() == [23, 22, 17, 9, 2, 1]
    assert offsets.tolist() == [0, 23, 45, 62, 71, 73, 74] and n == 74 and xp.shape == (74, C) and xp.dtype == dtype
    # the layout: sequence j's step t at row offsets[j] + t; the first and last row of every sequence
    for j, b in enumerate(order):
        assert np.array_equal(xp[offsets[j]], x[b, 0]) and np.array_equal(xp[offsets[j + 1] - 1], x[b, lens[j] - 1])
    back = pn.unpack(xp, lengths, T_)
    m = pn.valid_mask(lengths, T_)
    assert back.shape == x.shape and back.dtype == dtype
    assert np.array_equal(back[m], x[m]) and not back[~m].any() and (back[m] != 0).all()
    assert np.array_equal(pn.pack(back, lengths), xp)
    idx = pn.packed_index(lengths, T_, C)
    assert np.array_equal(np.sort(idx[m].ravel()), np.arange(n * C)) and (idx[~m] == -1).all()
    assert np.array_equal(xp.ravel()[idx[m].ravel()], x[m].ravel())


# ------------------------------------------------------------------------------------------------ mode parsing, refusals
def test_sparch_lengths_parsing():
    from sparch_amd import exp
    assert exp.parse_lengths_mode(None) is False and exp.parse_lengths_mode("") is False
    assert exp.parse_lengths_mode("mask") is True
    assert exp.parse_lengths_mode("pack") == "pack"
    for bad in ("1", "Pack", "pack ", "packed", "on", "mask,pack"):
        with pytest.raises(ValueError, match="SPARCH_LENGTHS"):
            exp.parse_lengths_mode(bad)


def test_experiment_refuses_before_anything_else(monkeypatch, tmp_path):
    from sparch_amd import exp

    def args(**kw):
        base = dict(model_type="LIF", sync_bn=False, use_pretrained_model=False, bidirectional=False,
                    new_exp_folder=str(tmp_path / "never"))
        return argparse.Namespace(**dict(base, **kw))
    monkeypatch.setenv("SPARCH_LENGTHS", "pack")
    with pytest.raises(ValueError, match="sync_bn"):
        exp.Experiment(args(sync_bn=True))
    with pytest.raises(ValueError, match="spiking model"):
        exp.Experiment(args(model_type="MLP"))
    with pytest.raises(ValueError, match="bidirectional"):
        exp.Experiment(args(bidirectional=True))
    with pytest.raises(ValueError, match="above 1024"):
        exp.Experiment(args(model_type="RadLIF", nb_hiddens=2048))
    monkeypatch.setenv("SPARCH_REC_STEPS_PER_LAUNCH", "1")
    with pytest.raises(ValueError, match="step mode"):
        exp.Experiment(args(model_type="RLIF", nb_hiddens=64))
    monkeypatch.delenv("SPARCH_REC_STEPS_PER_LAUNCH")
    assert not (tmp_path / "never").exists()


def _net(sp_kw=None, kind="LIF", sizes=(8, 8, 5)):
    import sparch_amd
    return sparch_amd.SNN((3, None, 6), list(sizes), neuron_type=kind, **(sp_kw or {}))


X, LENS = torch.zeros(3, 4, 6), torch.tensor([4, 1, 2])


def test_every_python_refusal_is_a_value_error(monkeypatch):
    from sparch_amd import functional as Fn
    with pytest.raises(ValueError, match="needs lengths"):
        _net()(X, pack=True)
    with pytest.raises(ValueError, match="bidirectional"):
        _net(dict(bidirectional=True))(X, lengths=LENS, pack=True)
    with pytest.raises(ValueError, match="above 1024"):
        _net(kind="RLIF", sizes=(8, 1028, 5))(X, lengths=LENS, pack=True)
    _net(kind="LIF", sizes=(8, 1028, 5))  # (a non-recurrent layer of that width has no per-step path)
    monkeypatch.setenv("SPARCH_REC_STEPS_PER_LAUNCH", "1")
    with pytest.raises(ValueError, match="step mode"):
        _net(kind="RadLIF")(X, lengths=LENS, pack=True)
    monkeypatch.setenv("SPARCH_REC_STEPS_PER_LAUNCH", "3")      # chunks shorter than the longest sequence (4 steps)
    with pytest.raises(ValueError, match="chunked recurrent launches"):
        _net(kind="RadLIF")(X, lengths=LENS, pack=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # (LIF layers have no launches to chunk)
        _net(kind="LIF")(X, lengths=LENS, pack=True)
    monkeypatch.delenv("SPARCH_REC_STEPS_PER_LAUNCH")
    monkeypatch.setattr(Fn, "_degraded", {0})       # (what a timeout leaves behind on device 0)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    with pytest.raises(ValueError, match="step mode"):
        _net(kind="RLIF")(X, lengths=LENS, pack=True)
    monkeypatch.undo()
    monkeypatch.setattr(Fn, "SYNC_BN", {"group": None, "world": 2})
    with pytest.raises(ValueError, match="sync_bn"):
        _net()(X, lengths=LENS, pack=True)
    monkeypatch.setattr(Fn, "SYNC_BN", None)
    net = _net()
    net._static_states = object()       # (what GraphedTrainStep sets for the life of its captured step)
    with pytest.raises(ValueError, match="captured step"):
        net(X, lengths=LENS, pack=True)
    del net._static_states
    for bad in (torch.tensor([4, 0, 2]), torch.tensor([5, 1, 2]), torch.tensor([4, 1]), torch.tensor([4.0, 1.0, 2.0])):
        with pytest.raises(ValueError, match="lengths"):
            net(X, lengths=bad, pack=True)
    with pytest.raises(ValueError, match="prepare_packing"):
        net.snn[0].forward_with_rate(X, pack=LENS)
    # BatchNorm with a bias is NOT refused here (there is no padded row for the bias to fill): the device check is
    # what stops a host tensor, as under LayerNorm and without normalisation
    for norm in ("batchnorm", "layernorm", "none"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _net(dict(use_bias=True, normalization=norm))(X, lengths=LENS, pack=True)


def test_baselines_and_streams_refuse_packed_batches():
    from sparch_amd import streaming, streaming_ann
    from sparch_amd.anns import ANN
    ann = ANN((3, None, 6), [8, 5], ann_type="MLP")
    for kw in (dict(lengths=LENS, pack=True), dict(pack=True)):
        with pytest.raises(ValueError, match="non-spiking"):
            ann(X, **kw)
        for cls in (streaming.StreamingSNN, streaming_ann.StreamingANN):
            with pytest.raises(ValueError, match="streaming"):
                cls.step(object.__new__(cls), X, **kw)
