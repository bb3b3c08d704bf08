"""
Bidirectional layers on ragged batches without a GPU:
  * the eight sparch_bidir_* entries are declared in the header, bound in _capi.PROTOTYPES (the ABI version stays) and
    refuse — SPARCH_EINVAL in front of SPARCH_EALIGN — before any device work (nothing here reaches a launch);
  * snns.prepare_bidir_packing: the doubled batch's plan meets prepare_packing's invariants, and fwd / rev point at the two
    copies of every sequence (against tests/bidir_numpy.doubled_plan);
  * the numpy restatement itself: split / join and their adjoints are adjoint pairs, padded and packed agree;
  * lengths / pack with bidirectional=True pass every Python refusal but the one that stops a host tensor, and the
    refusals that stay are ValueErrors before the first kernel;
  * without lengths the committed layer call trace is unchanged.
"""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from tests import bidir_numpy as bn
from tests import packed_numpy as pn
from tests.entry_probes import Entry, P
from tests.kit import EALIGN, EINVAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B_, T_ = 2, 3
ODD2, ODD4 = 17, 18          # misaligned for a 2-byte / a 4-byte element (18 is aligned for a 2-byte one)
LEN = [("lengths", P), ("n_valid", 5), ("stream", None)]
PK = [("lengths", P), ("offsets", P), ("fwd", P), ("rev", P), ("n_valid", 5), ("stream", None)]


def entries(name, mid, width="C"):
    shape = [("B", B_), ("T", T_), (width, 8)]
    return Entry(f"sparch_bidir_{name}_len", shape + mid + LEN), Entry(f"sparch_bidir_{name}_pk", shape + mid + PK)


SPLIT = entries("split", [("elem_size", 4), ("src", P), ("dst", P)])
SPLIT_BWD = entries("split_bwd", [("g", P), ("g_src", P)])
JOIN = entries("join", [("s16", P), ("y16", P), ("y32", None), ("scale", 1.0), ("spike_count", P)], "H")
JOIN_BWD = entries("join_bwd", [("g", P), ("g_rate", None), ("rate_scale", 0.2), ("g2", P)], "H")
ALL = SPLIT + SPLIT_BWD + JOIN + JOIN_BWD
REQUIRED = {"split": ("src", "dst"), "split_bwd": ("g", "g_src"), "join": ("s16", "y16", "spike_count"),
            "join_bwd": ("g", "g2")}
ids = lambda e: e.name  # noqa: E731


def family(e):
    return e.name[len("sparch_bidir_"):].rsplit("_", 1)[0]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_is_additive_and_prototypes_are_the_header():
    from sparch_amd._capi import PROTOTYPES, lib
    assert lib.sparch_abi_version() == 5
    with open(os.path.join(ROOT, "include", "sparch_hip.h")) as f:
        header = f.read()
    for e in ALL:
        decl = re.search(r"\bint " + e.name + r"\(([^;]*)\);", header)
        assert decl, e.name
        params = [q.strip() for q in decl.group(1).replace("\n", " ").split(",")]
        assert len(params) == len(e.args) == len(PROTOTYPES[e.name][1]), e.name
        assert [q.split()[-1].lstrip("*") for q in params] == [k for k, _ in e.args], e.name
        assert hasattr(lib, e.name)
    for a, b in (SPLIT, SPLIT_BWD, JOIN, JOIN_BWD):   # the `_pk` form: offsets, fwd, rev behind the lengths
        at = [k for k, _ in b.args].index("offsets")
        pk = PROTOTYPES[b.name][1]
        assert pk[:at] + pk[at + 3:] == PROTOTYPES[a.name][1]
    declared = set(re.findall(r"\b(sparch_\w+)\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S)))
    assert declared == set(PROTOTYPES)


@pytest.mark.parametrize("e", ALL, ids=ids)
def test_entries_refuse_before_any_device_work(e):
    """Every call has something broken: nothing is launched (the pointers are small integers)."""
    names = [k for k, _ in e.args]
    need = REQUIRED[family(e)] + ("lengths",) + (("offsets", "fwd", "rev") if e.name.endswith("_pk") else ())
    for k in need:
        assert e(**{k: None}) == EINVAL, k
    for n in (0, -1, -(1 << 40), B_ * T_ + 1):
        assert e(n_valid=n) == EINVAL, n
    width = "C" if "C" in names else "H"
    assert e(B=0) == EINVAL and e(T=0) == EINVAL and e(**{width: 0}) == EINVAL and e(B=-3) == EINVAL
    if "elem_size" in names:
        for size in (0, 3, 8, -1):
            assert e(elem_size=size) == EINVAL, size
    # alignment to the element, checked behind every SPARCH_EINVAL
    first = need[0]
    odd = ODD2 if family(e) == "join" else ODD4
    assert e(**{first: odd}) == EALIGN
    assert e(**{first: odd, "lengths": None}) == EINVAL and e(**{first: odd, "n_valid": 0}) == EINVAL
    assert e(**{first: odd, "T": 0}) == EINVAL
    if "elem_size" in names:
        assert e(**{first: odd, "elem_size": 3}) == EINVAL
        assert e(src=ODD2, elem_size=2) == EALIGN and e(dst=ODD4, elem_size=4) == EALIGN
    if family(e) == "join":
        assert e(y32=ODD4) == EALIGN and e(spike_count=ODD4) == EALIGN and e(y16=ODD2) == EALIGN
    if family(e) == "join_bwd":
        assert e(g_rate=ODD4) == EALIGN and e(g2=ODD4) == EALIGN
    if family(e) == "split_bwd":
        assert e(g_src=ODD4) == EALIGN


# ------------------------------------------------------------------------------------------------ the doubled plan
PLANS = [([4, 7, 4, 1, 7, 4], 7), ([3], 5), ([2, 2, 2], 2), ([1, 2, 3, 4], 9), ([23, 1, 9, 17, 2, 22], 23)]


@pytest.mark.parametrize("lengths,T", PLANS)
def test_the_doubled_plan_meets_prepare_packings_invariants(lengths, T):
    from sparch_amd import functional as Fn
    from sparch_amd import snns
    B = len(lengths)
    plan = snns.prepare_packing(lengths, B, T, "cpu")
    two = snns.prepare_bidir_packing(plan, "cpu")
    assert isinstance(two, Fn.BidirPlan) and isinstance(two.plan, Fn.PackPlan)
    p2 = two.plan
    # what prepare_packing itself gives for the 2B sequences — batch row b is clip b, row B + b its reversed copy
    want = snns.prepare_packing(list(lengths) + list(lengths), 2 * B, T, "cpu")
    for name in ("order", "lengths", "offsets", "inverse"):
        assert getattr(p2, name).dtype == torch.int32
        assert getattr(p2, name).tolist() == getattr(want, name).tolist(), name
    assert (p2.n, p2.t_max, p2.batch, p2.T) == (2 * plan.n, plan.t_max, 2 * B, T) == (want.n, want.t_max, want.batch, want.T)
    # the invariants, spelled out: descending and stable, an exclusive prefix sum, the inverse permutation
    order, lens, offsets = p2.order.tolist(), p2.lengths.tolist(), p2.offsets.tolist()
    assert sorted(order) == list(range(2 * B))
    for j in range(2 * B - 1):
        assert lens[j] > lens[j + 1] or (lens[j] == lens[j + 1] and order[j] < order[j + 1])
    assert offsets[0] == 0 and offsets[-1] == p2.n and all(offsets[j + 1] - offsets[j] == lens[j] for j in range(2 * B))
    assert p2.inverse[p2.order.long()].tolist() == list(range(2 * B))
    for k, h in enumerate(p2.host):
        assert h.tolist() == (p2.order, p2.lengths, p2.offsets)[k].tolist()
    # fwd / rev: where sequence j of the single plan and its reversed copy start in the doubled packed tensor
    order2, lens2, offsets2, inverse2, fwd, rev = bn.doubled_plan(lengths)
    assert order == order2.tolist() and offsets == offsets2.tolist()
    assert two.fwd.dtype == two.rev.dtype == torch.int32
    assert two.fwd.tolist() == fwd.tolist() and two.rev.tolist() == rev.tolist()
    for j, b in enumerate(plan.order.tolist()):
        assert offsets[order.index(b)] == int(two.fwd[j]) and offsets[order.index(B + b)] == int(two.rev[j])
    # one buffer: consecutive pieces of one allocation
    base = p2.order.data_ptr()
    assert p2.lengths.data_ptr() == base + 8 * B and p2.offsets.data_ptr() == base + 16 * B
    assert two.fwd.data_ptr() == base + 4 * (8 * B + 1) and two.rev.data_ptr() == two.fwd.data_ptr() + 4 * B


# ------------------------------------------------------------------------------------------------ the restatement
def test_the_restatement_is_consistent():
    lengths, T, C = [23, 1, 9, 17, 2, 22], 23, 5
    B = len(lengths)
    rng = np.random.default_rng(5)
    x = rng.integers(1, 200, (B, T, C)).astype(np.float32)
    m = pn.valid_mask(lengths, T)
    x2 = bn.split(x, lengths)
    assert x2.shape == (2 * B, T, C) and not x2[np.concatenate([~m, ~m])].any()
    assert np.array_equal(x2[:B][m], x[m]) and np.array_equal(x2[B, :, 0], x[0, ::-1, 0]) and x2[B + 1, 0, 0] == x[1, 0, 0]
    assert np.array_equal(x2[B + 2, :9], x[2, 8::-1])
    # join undoes split on both halves
    y = bn.join(x2, lengths)
    assert np.array_equal(y[..., :C][m], x[m]) and np.array_equal(y[..., C:][m], x[m]) and not y[~m].any()
    # adjoint pairs: <split x, g> = <x, split_bwd g> and <join s, g> = <s, join_bwd g> on the valid steps
    g2 = rng.integers(-9, 9, (2 * B, T, C)).astype(np.float32)
    xm = x * m[:, :, None]
    assert float((bn.split(xm, lengths) * g2).sum()) == float((xm * bn.split_bwd(g2, lengths)).sum())
    s2 = x2
    gy = rng.integers(-9, 9, (B, T, 2 * C)).astype(np.float32)
    assert float((bn.join(s2, lengths) * gy).sum()) == float((s2 * bn.join_bwd(gy, None, 0.0, lengths)).sum())
    # the rate term: a constant per column on the valid steps of the direction's rows
    gr = rng.integers(1, 9, 2 * C).astype(np.float32)
    d = bn.join_bwd(gy, gr, 0.5, lengths) - bn.join_bwd(gy, None, 0.0, lengths)
    m2 = np.concatenate([m, m])
    assert np.array_equal(d[:B][m], np.broadcast_to(gr[:C] * 0.5, d[:B][m].shape))
    assert np.array_equal(d[B:][m], np.broadcast_to(gr[C:] * 0.5, d[B:][m].shape)) and not d[~m2].any()
    # packed: every doubled row is written exactly once, forward and reverse rows where the plan says
    order2, lens2, offsets2, inverse2, fwd, rev = bn.doubled_plan(lengths)
    xp2 = bn.pack2(x2, lengths)
    xp = pn.pack(x, lengths)
    order, lens, offsets, n = pn.plan_of(lengths)
    assert xp2.shape == (2 * n, C)
    for j in range(B):
        L = int(lens[j])
        assert np.array_equal(xp2[fwd[j]:fwd[j] + L], xp[offsets[j]:offsets[j] + L])
        assert np.array_equal(xp2[rev[j]:rev[j] + L], xp[offsets[j]:offsets[j] + L][::-1])


# ------------------------------------------------------------------------------------------------ Python refusals
def _net(sp_kw=None, kind="LIF", sizes=(8, 8, 5)):
    import sparch_amd
    return sparch_amd.SNN((3, None, 6), list(sizes), neuron_type=kind, **dict(dict(bidirectional=True), **(sp_kw or {})))


X, LENS = torch.zeros(3, 4, 6), torch.tensor([4, 1, 2])
MODES = [dict(lengths=LENS), dict(lengths=LENS, pack=True)]


@pytest.mark.parametrize("mode", MODES, ids=["mask", "pack"])
@pytest.mark.parametrize("kind", ["LIF", "adLIF", "RLIF", "RadLIF"])
def test_bidirectional_layers_take_lengths(kind, mode, monkeypatch):
    """No refusal of the combination is left.  What stops a HOST tensor is a refusal of its own, a ValueError that names
    the device; with that one check answered the call goes on to the layers, where the library's device check ("no CPU
    fallback") ends it: every Python refusal has been passed."""
    from sparch_amd import snns
    for norm in ("batchnorm", "layernorm", "none"):
        with pytest.raises(ValueError, match="bidirectional=True takes an input on the HIP device"):
            _net(dict(normalization=norm), kind=kind)(X, **mode)
    monkeypatch.setattr(snns, "_check_bidir_input", lambda net, x, what: None)
    for norm in ("batchnorm", "layernorm", "none"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _net(dict(normalization=norm), kind=kind)(X, **mode)
    if not mode.get("pack"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _net(kind=kind)(X, per_step="sum", **mode)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _net(dict(readout="u_max"), kind=kind)(X, **mode)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _net(dict(max_delay=3), kind=kind)(X, **mode)


@pytest.mark.parametrize("mode", MODES, ids=["mask", "pack"])
def test_the_refusals_that_stay_are_value_errors(mode, monkeypatch):
    from sparch_amd import functional as Fn
    st = [{"u": torch.zeros(3, 8), "s": torch.zeros(3, 8)}, {"u": torch.zeros(3, 8), "s": torch.zeros(3, 8)},
          {"u": torch.zeros(3, 5)}]
    for kw in (dict(state=st), dict(return_state=True)):            # a carried state is causal
        with pytest.raises(ValueError, match="bidirectional"):
            _net()(X, **mode, **kw)
        with pytest.raises(ValueError, match="bidirectional"):
            _net()(X, **kw)
    net = _net()
    net._static_states = object()       # (what GraphedTrainStep sets for the life of its captured step)
    with pytest.raises(ValueError, match="captured step"):
        net(X, **mode)
    monkeypatch.setattr(Fn, "SYNC_BN", {"group": None, "world": 2})
    with pytest.raises(ValueError, match="sync_bn"):
        _net()(X, **mode)
    monkeypatch.setattr(Fn, "SYNC_BN", None)
    with pytest.raises(ValueError, match="above 1024"):
        _net(kind="RadLIF", sizes=(8, 1028, 5))(X, **mode)
    if mode.get("pack"):
        with pytest.raises(ValueError, match="per_step"):
            _net()(X, per_step="sum", **mode)
        monkeypatch.setenv("SPARCH_REC_STEPS_PER_LAUNCH", "1")
        with pytest.raises(ValueError, match="step mode"):
            _net(kind="RadLIF")(X, **mode)
        monkeypatch.setenv("SPARCH_REC_STEPS_PER_LAUNCH", "3")      # chunks shorter than the longest sequence (4 steps)
        with pytest.raises(ValueError, match="chunked recurrent launches"):
            _net(kind="RLIF")(X, **mode)
        monkeypatch.delenv("SPARCH_REC_STEPS_PER_LAUNCH")
    else:
        with pytest.raises(ValueError, match="use_bias"):
            _net(dict(use_bias=True, normalization="batchnorm"))(X, **mode)
    # the layer alone, and the cell functions: they run one direction
    with pytest.raises(ValueError, match="prepare_"):
        _net().snn[0].forward_with_rate(X, **({"pack": LENS} if mode.get("pack") else {"lengths": LENS}))
    zeros = torch.zeros(6, 4, 8)
    with pytest.raises(ValueError, match="dirs=1"):
        Fn.cell_forward("LIF", zeros, None, None, {}, None, None, None, B=3, dirs=2, theta=1.0, p_drop=0.0, seed=0,
                        lengths=(LENS.int(), 7))
    with pytest.raises(ValueError, match="dirs=1"):
        Fn.cell_backward("LIF", zeros, None, {}, None, None, None, (zeros, None), B=3, dirs=2, T=4, H=8, theta=1.0,
                         p_drop=0.0, seed=0, lengths=(LENS.int(), 7))


def test_baselines_and_streams_still_refuse(monkeypatch, tmp_path):
    from sparch_amd import exp, streaming, streaming_ann
    from sparch_amd.anns import ANN
    ann = ANN((3, None, 6), [8, 5], ann_type="RNN", bidirectional=True)
    for kw in MODES:
        with pytest.raises(ValueError, match="non-spiking"):
            ann(X, **kw)
        for cls in (streaming.StreamingSNN, streaming_ann.StreamingANN):
            with pytest.raises(ValueError, match="streaming"):
                cls.step(object.__new__(cls), X, **kw)
    with pytest.raises(ValueError, match="not causal"):
        streaming.StreamingSNN(_net(), 3)

    def args(**kw):
        base = dict(model_type="LIF", sync_bn=False, use_pretrained_model=False, bidirectional=True,
                    new_exp_folder=str(tmp_path / "never"))
        return argparse.Namespace(**dict(base, **kw))
    for mode in ("mask", "pack"):                                    # the refusals in front of the model still hold
        monkeypatch.setenv("SPARCH_LENGTHS", mode)
        with pytest.raises(ValueError, match="sync_bn"):
            exp.Experiment(args(sync_bn=True))
        with pytest.raises(ValueError, match="spiking model"):
            exp.Experiment(args(model_type="RNN"))
    # the command line: SPARCH_LENGTHS=pack with --bidirectional stays refused there; =mask is not
    # refused — the constructor goes on to the arguments it needs next, of which this bare namespace has none
    with pytest.raises(ValueError, match="bidirectional"):
        exp.Experiment(args())
    assert not (tmp_path / "never").exists()
    monkeypatch.setenv("SPARCH_LENGTHS", "mask")
    with pytest.raises(AttributeError) as err:
        exp.Experiment(args())
    assert "bidirectional" not in str(err.value)
