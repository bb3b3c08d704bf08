"""
The selectable readout (SNN(readout=...), the `_red` entry points, SPARCH_READOUT) without a GPU:
  * the host restatement (tests/readout_modes_numpy.py) against torch autograd on a torch fp64 forward of the same
    formulas, every mode, with and without lengths; mode 0 of it is tests/spiking_numpy.py's arrays exactly;
  * the C ABI: the `_red` entry points refuse with SPARCH_EINVAL before any device work, the ABI is additive;
  * the Python refusals, each a ValueError before a kernel; the default leaves the committed layer call trace unchanged;
  * SPARCH_READOUT parsing and the refusals of Experiment;
  * a network pickled before the attribute existed behaves as the default.
"""
import argparse
import os
import pickle
import re

import numpy as np
import pytest
import torch

from tests import readout_modes_numpy as rm
from tests import spiking_numpy as sn
from tests.entry_probes import Entry, P, T, ptrs
from tests.kit import EINVAL, F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [("B", 2), ("T", T), ("C", 5)]
TAIL = [("red", 2), ("arg", P), ("lengths", P), ("offsets", P), ("n_valid", 5), ("stream", None)]
FWD = Entry("sparch_readout_fwd_red", DIMS + ptrs("Wx scale shift alpha u0 out u_save", "scale shift") + TAIL)
BWD = Entry("sparch_readout_bwd_red",
            DIMS + ptrs("g_out bn_x bn_mean bn_invstd u_save alpha u0 dWx dalpha_ws", "bn_x bn_mean bn_invstd") + TAIL)
STREAM = Entry("sparch_readout_stream_fwd_red",
               DIMS + ptrs("Wx scale shift alpha u out", "scale shift") + [("red", 2), ("stream", None)])
ENTRIES = (FWD, BWD)
SIBLING = {FWD: "sparch_readout_fwd_pk", BWD: "sparch_readout_bwd_pk", STREAM: "sparch_readout_stream_fwd"}


# ------------------------------------------------------------------------------------------------ the restatement
def _case(B, T_, C, seed):
    rng = np.random.default_rng(seed)
    c = dict(Wx=(1.5 * rng.standard_normal((B, T_, C))), alpha=rng.uniform(0.83, 0.95, C).astype(F32),
             u0=rng.uniform(0, 1, (B, C)), g_out=rng.standard_normal((B, C)))
    if C >= 3:
        c["alpha"][0], c["alpha"][1] = 0.5, 1.2        # outside the clamp range: a zero gradient
    return c


@pytest.mark.parametrize("lengths", [None, [9, 4]], ids=["full", "ragged"])
@pytest.mark.parametrize("mode", rm.MODES)
def test_restatement_against_autograd_fp64(mode, lengths):
    B, T_, C = 2, 9, 5
    c = _case(B, T_, C, 11)
    Wx = torch.tensor(c["Wx"], dtype=torch.float64, requires_grad=True)
    alpha = torch.tensor(c["alpha"], dtype=torch.float64, requires_grad=True)
    out = rm.torch_forward(Wx, alpha, torch.tensor(c["u0"]), mode, lengths)
    (out * torch.tensor(c["g_out"])).sum().backward()
    f = rm.forward(F64, c["Wx"], None, None, c["alpha"], c["u0"], mode, lengths)
    np.testing.assert_allclose(f["out"], out.detach().numpy(), rtol=1e-13, atol=0)
    m = rm.valid(lengths, B, T_)
    arg = f.get("arg")
    if mode == "u_max":
        assert arg.dtype == np.int32 and (arg < rm.steps_of(lengths, B, T_)[:, None]).all()
    if lengths is not None:
        f["u_save"][~m] = np.nan                            # the saved state behind a row's end is never looked at
    b = rm.backward(F64, c["g_out"], mode, f["u_save"], c["alpha"], c["u0"], lengths=lengths, arg=arg)
    scale = np.abs(Wx.grad.numpy()).max()
    assert np.abs(b["dWx"] - Wx.grad.numpy()).max() <= 1e-10 * scale
    assert np.abs(b["alpha"] - alpha.grad.numpy()).max() <= 1e-10 * np.abs(alpha.grad.numpy()).max()
    assert b["alpha"][0] == 0 and b["alpha"][1] == 0 and np.abs(b["alpha"][2:]).min() > 0
    assert not b["dWx"][~m].any()
    if mode == "u_max":                                     # arg None: taken from u_save — the same thing
        b2 = rm.backward(F64, c["g_out"], mode, np.where(m[:, :, None], f["u_save"], 0), c["alpha"], c["u0"], lengths=lengths)
        assert np.array_equal(b2["dWx"], b["dWx"])


@pytest.mark.parametrize("dtype", [F32, F64], ids=["fp32", "fp64"])
def test_mode_zero_is_spiking_numpy_exactly(dtype):
    B, T_, C = 2, 9, 5
    c = _case(B, T_, C, 3)
    bn = (0.8 * c["Wx"] + 0.3, np.full(C, 0.4), np.full(C, 1.25))
    for order in (None, "asc", "desc"):
        u, out = sn.readout_forward(dtype, c["Wx"], None, None, c["alpha"], c["u0"], order)
        f = rm.forward(dtype, c["Wx"], None, None, c["alpha"], c["u0"], "softmax_sum", class_order=order)
        assert f["u_save"].dtype == dtype and np.array_equal(f["u_save"], u) and np.array_equal(f["out"], out)
        want = sn.readout_backward(dtype, c["g_out"], u, c["alpha"], c["u0"], bn=bn, class_order=order)
        got = rm.backward(dtype, c["g_out"], "softmax_sum", u, c["alpha"], c["u0"], bn=bn, class_order=order)
        assert set(got) == set(want) and all(np.array_equal(got[k], want[k]) for k in want)
    # with every length == T the general path gives the same numbers (a sequential sum against numpy's: to rounding)
    full = [T_] * B
    f = rm.forward(dtype, c["Wx"], None, None, c["alpha"], c["u0"], "softmax_sum", lengths=full, class_order="asc")
    _, out = sn.readout_forward(dtype, c["Wx"], None, None, c["alpha"], c["u0"], "asc")
    assert np.array_equal(f["out"], out)
    got = rm.backward(dtype, c["g_out"], "softmax_sum", f["u_save"], c["alpha"], c["u0"], bn=bn, lengths=full, class_order="asc")
    want = sn.readout_backward(dtype, c["g_out"], f["u_save"], c["alpha"], c["u0"], bn=bn, class_order="asc")
    assert all(np.array_equal(got[k], want[k]) for k in want)


def test_restatement_relations_in_fp32():
    """What the kernels are held to bit for bit holds in the sequential-fp32 restatement too; ties go to the earliest."""
    B, T_, C = 2, 13, 4
    c = {k: v.astype(F32) for k, v in _case(B, T_, C, 5).items()}
    lens = [13, 6]
    f = {m: rm.forward(F32, c["Wx"], None, None, c["alpha"], c["u0"], m, lens) for m in rm.MODES}
    n = np.asarray(lens, F32)[:, None]
    assert np.array_equal(f["softmax_mean"]["out"], f["softmax_sum"]["out"] / n)
    U = f["u_max"]["u_save"]
    for b, nb in enumerate(lens):
        assert np.array_equal(f["u_max"]["out"][b], U[b, :nb].max(0)) and np.array_equal(f["u_last"]["out"][b], U[b, nb - 1])
    U2 = U.copy()
    U2[0, 7, 1] = U2[0, 2, 1] = U2[0].max() + 1            # a tie: the earliest step wins
    assert rm.first_argmax(U2, lens)[0, 1] == 2
    assert rm.first_argmax(U2, [2, 6])[0, 1] < 2            # ... among the row's own steps


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_is_additive_and_prototypes_are_the_header():
    from sparch_amd._capi import PROTOTYPES, lib
    assert lib.sparch_abi_version() == 5
    with open(os.path.join(ROOT, "include", "sparch_hip.h")) as f:
        header = f.read()
    for e, more in ((FWD, 2), (BWD, 2), (STREAM, 1)):
        assert len(e.args) == len(PROTOTYPES[e.name][1]) == len(PROTOTYPES[SIBLING[e]][1]) + more, e.name
        decl = re.search(r"\bint " + e.name + r"\(([^;]*)\);", header)
        assert decl, e.name
        params = [q.strip() for q in decl.group(1).replace("\n", " ").split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == [k for k, _ in e.args], e.name
        assert hasattr(lib, e.name)
    names = ("SOFTMAX_SUM", "SOFTMAX_MEAN", "U_MAX", "U_MEAN", "U_LAST")
    for i, name in enumerate(names):
        assert re.search(rf"#define SPARCH_RED_{name} {i}\n", header), name
    from sparch_amd import functional as Fn
    assert Fn.READOUT_MODES == {n.lower(): i for i, n in enumerate(names)} and tuple(Fn.READOUT_MODES) == rm.MODES


@pytest.mark.parametrize("e", ENTRIES, ids=lambda e: e.name)
def test_red_entries_refuse_before_any_device_work(e):
    """Nothing here reaches a launch: every call has something broken."""
    for red in (-1, 5, 99):
        assert e(red=red) == EINVAL, red
    assert e(red=2, arg=None) == EINVAL                                  # u_max without arg
    assert e(offsets=P, lengths=None) == EINVAL                          # offsets without lengths
    for n in (0, -1, -(1 << 40)):
        assert e(n_valid=n) == EINVAL and e(n_valid=n, offsets=None) == EINVAL, n
    assert e(C=257) == EINVAL
    # every one of them also with every other mode and layout; mode 0 takes the existing entry points' refusals
    for red in range(5):
        for lay in ({}, {"offsets": None}, {"offsets": None, "lengths": None}):
            assert e(red=red, C=257, **lay) == EINVAL and e(red=red, C=0, **lay) == EINVAL
            assert e(red=red, B=0, **lay) == EINVAL and e(red=red, T=0, **lay) == EINVAL
            assert e(red=red, alpha=None, **lay) == EINVAL and e(red=red, u0=None, **lay) == EINVAL
            if e is FWD:
                assert e(red=red, Wx=None, **lay) == EINVAL and e(red=red, out=None, **lay) == EINVAL
                assert e(red=red, scale=P, **lay) == EINVAL                                  # scale without shift
            else:
                assert e(red=red, g_out=None, **lay) == EINVAL and e(red=red, dWx=None, **lay) == EINVAL
                assert e(red=red, dalpha_ws=None, **lay) == EINVAL and e(red=red, u_save=None, **lay) == EINVAL
                assert e(red=red, bn_x=P, **lay) == EINVAL                                   # bn_x without its statistics


def test_stream_entry_refuses_before_any_device_work():
    e = STREAM
    for red in (-1, 5):
        assert e(red=red) == EINVAL
    for red in range(5):
        assert e(red=red, C=257) == EINVAL and e(red=red, C=0) == EINVAL and e(red=red, B=0) == EINVAL
        assert e(red=red, T=0) == EINVAL and e(red=red, Wx=None) == EINVAL and e(red=red, alpha=None) == EINVAL
        assert e(red=red, u=None) == EINVAL and e(red=red, out=None) == EINVAL and e(red=red, scale=P) == EINVAL


# ------------------------------------------------------------------------------------------------ Python
def _net(**kw):
    import sparch_amd
    return sparch_amd.SNN((3, None, 6), [8, 8, 5], neuron_type="LIF", **kw)


X, LENS = torch.zeros(3, 4, 6), torch.tensor([4, 1, 2])
NEW_MODES = rm.MODES[1:]


def test_every_python_refusal_is_a_value_error():
    import sparch_amd
    from sparch_amd import functional as Fn
    for bad in ("max", "U_MAX", "softmax", 1, True, ""):
        with pytest.raises(ValueError, match="readout"):
            _net(readout=bad)
        with pytest.raises(ValueError, match="readout"):
            sparch_amd.snns.ReadoutLayer(6, 5, 3, readout=bad)
        with pytest.raises(ValueError, match="readout"):
            Fn.ReadoutCellFn.apply(torch.zeros(2, 3, 5), torch.zeros(5), torch.zeros(2, 5), bad)
    for mode in NEW_MODES:
        net = _net(readout=mode).eval()
        for per_step in ("prob", "sum"):
            with pytest.raises(ValueError, match="per_step with readout"):
                net(X, per_step=per_step)
            with pytest.raises(ValueError, match="per_step with readout"):
                net(X, lengths=LENS, per_step=per_step)
            with pytest.raises(ValueError, match="per_step with readout"):
                net.snn[-1](X, per_step=per_step)
        for kw in ({"fused": True}, {"fused": True, "sparse": True}):
            with pytest.raises(ValueError, match="fused=True does not take readout"):
                sparch_amd.StreamingSNN(net, 3, **kw)
        # nothing else is refused: the device check is what stops a host tensor
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            net(X)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            net(X, lengths=LENS)
        assert f"readout={mode}" in repr(net) and f"readout={mode}" in repr(net.snn[-1])
    assert "readout" not in repr(_net()) and "readout" not in repr(_net(readout="softmax_sum"))
    assert Fn.readout_mode(None) == 0 and [Fn.readout_mode(m) for m in rm.MODES] == [0, 1, 2, 3, 4]


def test_a_network_pickled_without_the_attribute_is_the_default():
    """What torch.save(net) wrote before the argument existed: no `readout` in any __dict__."""
    net = _net().eval()
    del net.__dict__["readout"], net.snn[-1].__dict__["readout"]
    old = pickle.loads(pickle.dumps(net))
    assert not hasattr(old, "readout") and not hasattr(old.snn[-1], "readout")
    assert "readout" not in repr(old)
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # every refusal passed: it reaches the device check
        old(X, per_step="sum")
    import sparch_amd
    assert sparch_amd.StreamingSNN._readout_name(old) == "softmax_sum"
    sparch_amd.StreamingSNN(old, 3, fused=True)                    # not refused


# ------------------------------------------------------------------------------------------------ SPARCH_READOUT
def test_sparch_readout_parsing():
    from sparch_amd import exp
    assert exp.parse_readout(None) is None and exp.parse_readout("") is None and exp.parse_readout("  ") is None
    for m in rm.MODES:
        assert exp.parse_readout(m) == m and exp.parse_readout(f" {m} ") == m
    for bad in ("max", "U_MAX", "u_max:1", "softmax", "0", "u_max,u_mean"):
        with pytest.raises(ValueError, match="SPARCH_READOUT"):
            exp.parse_readout(bad)


def test_experiment_refuses_before_anything_else(monkeypatch, tmp_path):
    from sparch_amd import exp

    def args(**kw):
        return argparse.Namespace(**dict(dict(model_type="LIF", sync_bn=False, use_pretrained_model=False,
                                              new_exp_folder=str(tmp_path / "never")), **kw))
    for k in ("SPARCH_LENGTHS", "SPARCH_PER_STEP_LOSS", "SPARCH_SURROGATE", "SPARCH_CLIP_GRAD"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SPARCH_READOUT", "max")
    with pytest.raises(ValueError, match="SPARCH_READOUT"):
        exp.Experiment(args())
    monkeypatch.setenv("SPARCH_READOUT", "u_max")
    with pytest.raises(ValueError, match="SPARCH_READOUT needs a spiking model"):
        exp.Experiment(args(model_type="MLP"))
    monkeypatch.setenv("SPARCH_PER_STEP_LOSS", "0.5:10")
    with pytest.raises(ValueError, match="SPARCH_READOUT=u_max with SPARCH_PER_STEP_LOSS"):
        exp.Experiment(args())
    assert not (tmp_path / "never").exists()
