"""
The per-step readout (SNN.forward(x, per_step=...), the `_seq` entry points, SPARCH_PER_STEP_LOSS) without a GPU:
  * the host restatement (tests/readout_seq_numpy.py) against torch autograd in fp64, both modes, with and without
    lengths, and against the oracle's own readout where the two must agree;
  * the C ABI: the `_seq` entry points refuse with SPARCH_EINVAL before any device work, the ABI is additive;
  * the Python refusals; per_step=None leaves the committed layer call trace unchanged;
  * SPARCH_PER_STEP_LOSS parsing, the per-step loss and the decision-step metric on hand-made tensors.
"""
import argparse
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import readout_seq_numpy as rs
from tests.entry_probes import Entry, P, T, ptrs
from tests.kit import EINVAL, F32, F64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIMS = [("B", 2), ("T", T), ("C", 5)]
LEN = [("lengths", P), ("n_valid", 5)]
FWD_ARGS = DIMS + ptrs("Wx scale shift alpha u0 out u_save seq", "scale shift") + [("seq_mode", 1)]
BWD_ARGS = (DIMS + ptrs("g_out g_seq") + [("seq_mode", 1)]
            + ptrs("bn_x bn_mean bn_invstd u_save alpha u0 dWx dalpha_ws", "bn_x bn_mean bn_invstd"))
FWD = Entry("sparch_readout_fwd_seq", FWD_ARGS + [("stream", None)])
BWD = Entry("sparch_readout_bwd_seq", BWD_ARGS + [("stream", None)])
FWD_LEN = Entry("sparch_readout_fwd_seq_len", FWD_ARGS + LEN + [("stream", None)])
BWD_LEN = Entry("sparch_readout_bwd_seq_len", BWD_ARGS + LEN + [("stream", None)])
ENTRIES = (FWD, BWD, FWD_LEN, BWD_LEN)
SIBLING = {FWD: "sparch_readout_fwd", BWD: "sparch_readout_bwd", FWD_LEN: "sparch_readout_fwd_len",
           BWD_LEN: "sparch_readout_bwd_len"}


# ------------------------------------------------------------------------------------------------ the restatement
def _case(B, T_, C, seed):
    rng = np.random.default_rng(seed)
    c = dict(Wx=(1.5 * rng.standard_normal((B, T_, C))), alpha=rng.uniform(0.83, 0.95, C).astype(F32),
             u0=rng.uniform(0, 1, (B, C)), g_out=rng.standard_normal((B, C)), g_seq=rng.standard_normal((B, T_, C)))
    if C >= 3:
        c["alpha"][0], c["alpha"][1] = 0.5, 1.2        # outside the clamp range: a zero gradient
    return c


@pytest.mark.parametrize("lengths", [None, [9, 1, 4]], ids=["full", "ragged"])
@pytest.mark.parametrize("mode", rs.MODES)
def test_restatement_against_autograd_fp64(mode, lengths):
    B, T_, C = 3, 9, 5
    c = _case(B, T_, C, 11)
    Wx = torch.tensor(c["Wx"], dtype=torch.float64, requires_grad=True)
    alpha = torch.tensor(c["alpha"], dtype=torch.float64, requires_grad=True)
    out, seq = rs.torch_forward(Wx, alpha, torch.tensor(c["u0"]), mode, lengths)
    g_seq = c["g_seq"].copy()
    (out * torch.tensor(c["g_out"])).sum().add((seq * torch.tensor(g_seq)).sum()).backward()
    f = rs.forward(F64, c["Wx"], None, None, c["alpha"], c["u0"], mode, lengths)
    np.testing.assert_allclose(f["out"], out.detach().numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(f["seq"], seq.detach().numpy(), rtol=1e-13, atol=1e-15)
    if lengths is not None:
        m = rs._valid(lengths, B, T_)
        assert not f["seq"][~m].any() and f["seq"][m].all()
        g_seq[~m] = np.nan                                  # the padding's gradient is never looked at
        f["u_save"][~m] = np.nan                            # nor is the saved state behind a row's end
    b = rs.backward(F64, c["g_out"], g_seq, mode, f["u_save"], c["alpha"], c["u0"], lengths=lengths)
    np.testing.assert_allclose(b["dWx"], Wx.grad.numpy(), rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(b["alpha"], alpha.grad.numpy(), rtol=1e-10, atol=1e-14)
    assert b["alpha"][0] == 0 and b["alpha"][1] == 0 and np.abs(b["alpha"][2:]).min() > 0
    if lengths is not None:
        assert not b["dWx"][~m].any()
    # g_out = None counts as 0
    b0 = rs.backward(F64, None, g_seq, mode, f["u_save"], c["alpha"], c["u0"], lengths=lengths)
    bz = rs.backward(F64, np.zeros((B, C)), g_seq, mode, f["u_save"], c["alpha"], c["u0"], lengths=lengths)
    assert np.array_equal(b0["dWx"], bz["dWx"])


def test_restatement_identities_in_fp32():
    """What the kernels are held to bit for bit holds in the sequential-fp32 restatement too."""
    B, T_, C = 2, 13, 4
    c = {k: v.astype(F32) for k, v in _case(B, T_, C, 5).items()}
    fs = rs.forward(F32, c["Wx"], None, None, c["alpha"], c["u0"], "sum")
    fp = rs.forward(F32, c["Wx"], None, None, c["alpha"], c["u0"], "prob")
    assert fs["seq"].dtype == F32 and np.array_equal(fs["seq"][:, -1], fs["out"]) and np.array_equal(fs["out"], fp["out"])
    acc = np.zeros((B, C), F32)
    for t in range(T_):
        acc = acc + fp["seq"][:, t]
        assert np.array_equal(acc, fs["seq"][:, t])
    S = rs.reverse_running_sum(c["g_seq"], F32)
    a = rs.backward(F32, c["g_out"], c["g_seq"], "sum", fs["u_save"], c["alpha"], c["u0"])
    b = rs.backward(F32, c["g_out"], S, "prob", fs["u_save"], c["alpha"], c["u0"])
    assert all(np.array_equal(a[k], b[k]) for k in a)
    h = c["g_seq"][:, 0]
    a = rs.backward(F32, c["g_out"], np.repeat(h[:, None], T_, 1), "prob", fs["u_save"], c["alpha"], c["u0"])
    b = rs.backward(F32, c["g_out"] + h, np.zeros_like(c["g_seq"]), "prob", fs["u_save"], c["alpha"], c["u0"])
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_restatement_against_the_oracle():
    assert rs.check_against_oracle() <= 5e-6


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_is_additive_and_prototypes_are_the_header():
    from sparch_amd._capi import PROTOTYPES, lib
    assert lib.sparch_abi_version() == 5
    with open(os.path.join(ROOT, "include", "sparch_hip.h")) as f:
        header = f.read()
    for e in ENTRIES:
        assert len(e.args) == len(PROTOTYPES[e.name][1]) == len(PROTOTYPES[SIBLING[e]][1]) + 2, e.name
        decl = re.search(r"\bint " + e.name + r"\(([^;]*)\);", header)
        assert decl, e.name
        params = [q.strip() for q in decl.group(1).replace("\n", " ").split(",")]
        assert [p.split()[-1].lstrip("*") for p in params] == [k for k, _ in e.args], e.name
        assert hasattr(lib, e.name)
    assert re.search(r"#define SPARCH_SEQ_PROB 0\n#define SPARCH_SEQ_SUM 1\n", header)


@pytest.mark.parametrize("e", ENTRIES, ids=lambda e: e.name)
def test_seq_entries_refuse_before_any_device_work(e):
    """Nothing here reaches a launch: every call has something broken."""
    per_step = "seq" if "fwd" in e.name else "g_seq"
    assert e(**{per_step: None}) == EINVAL
    for mode in (-1, 2, 7):
        assert e(seq_mode=mode) == EINVAL, mode
    assert e(C=257) == EINVAL and e(C=0) == EINVAL and e(B=0) == EINVAL and e(T=0) == EINVAL
    assert e(alpha=None) == EINVAL and e(u0=None) == EINVAL and e(u_save=None if "bwd" in e.name else P, C=257) == EINVAL
    if "fwd" in e.name:
        assert e(Wx=None) == EINVAL and e(out=None) == EINVAL and e(scale=P) == EINVAL      # scale without shift
    else:
        assert e(dWx=None) == EINVAL and e(dalpha_ws=None) == EINVAL and e(u_save=None) == EINVAL
        assert e(bn_x=P) == EINVAL                                                             # bn_x without its statistics
        assert e(g_out=None, g_seq=None) == EINVAL      # (g_out alone may be NULL: a valid call, made on the GPU only)
    if e in (FWD_LEN, BWD_LEN):
        assert e(lengths=None) == EINVAL
        for n in (0, -1, -(1 << 40)):
            assert e(n_valid=n) == EINVAL, n


def test_chunk_steps_is_the_launchers_sizing():
    """sparch_readout_chunk_steps: min(T, 256, LDS floats / row stride), the row stride odd and above C; the per-step
    backward holds four chunk images where the plain one holds three."""
    from sparch_amd._capi import lib
    rows = lib.sparch_readout_chunk_steps
    assert rows(1000, 35, 0, 0) == rows(1000, 35, 0, 1) == 256 and rows(7, 35, 1, 1) == 7
    assert rows(1000, 256, 0, 0) == 15872 // 257 == 61
    assert rows(1000, 256, 1, 0) == (39168 // 3) // 257 == 50 and rows(1000, 256, 1, 1) == (39168 // 4) // 257 == 38
    assert rows(1000, 70, 1, 1) == (39168 // 4) // 71 == 137 and rows(1000, 70, 1, 0) == 183
    assert rows(0, 5, 0, 0) == 0 and rows(5, 0, 0, 0) == 0 and rows(5, 257, 1, 1) == 0


# ------------------------------------------------------------------------------------------------ Python refusals
def _net(**kw):
    import sparch_amd
    return sparch_amd.SNN((3, None, 6), [8, 8, 5], neuron_type="LIF", **kw)


X, LENS = torch.zeros(3, 4, 6), torch.tensor([4, 1, 2])


def test_every_python_refusal_is_a_value_error():
    from sparch_amd import functional as Fn
    for bad in ("mean", "SUM", 1, True, ""):
        with pytest.raises(ValueError, match="per_step"):
            _net()(X, per_step=bad)
        with pytest.raises(ValueError, match="per_step"):
            _net().snn[-1](X, per_step=bad)
    for mode in rs.MODES:
        with pytest.raises(ValueError, match="pack"):
            _net()(X, lengths=LENS, pack=True, per_step=mode)
        with pytest.raises(ValueError, match="pack"):
            _net().snn[-1](X, pack=object(), per_step=mode)
        with pytest.raises(ValueError, match="readout layer"):
            _net(use_readout_layer=False)(X, per_step=mode)
        # nothing else is refused: the device check is what stops a host tensor
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _net()(X, per_step=mode)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            _net()(X, lengths=LENS, per_step=mode)
    assert Fn.seq_mode(None) is None and Fn.seq_mode("prob") == 0 and Fn.seq_mode("sum") == 1


# ------------------------------------------------------------------------------------------------ SPARCH_PER_STEP_LOSS
def test_sparch_per_step_loss_parsing():
    from sparch_amd import exp
    assert exp.parse_per_step_loss(None) is None and exp.parse_per_step_loss("") is None
    assert exp.parse_per_step_loss("0.5") == (0.5, 0) and exp.parse_per_step_loss("0.5:10") == (0.5, 10)
    assert exp.parse_per_step_loss("2:0") == (2.0, 0) and exp.parse_per_step_loss(" 1e-1:3 ") == (0.1, 3)
    for bad in ("x", "0", "-1", "nan", "inf", "0.5:", "0.5:-1", "0.5:1.5", "0.5:a", ":3", "0.5:1:2"):
        with pytest.raises(ValueError, match="SPARCH_PER_STEP_LOSS"):
            exp.parse_per_step_loss(bad)


def test_experiment_refuses_before_anything_else(monkeypatch, tmp_path):
    from sparch_amd import exp

    def args(**kw):
        return argparse.Namespace(**dict(dict(model_type="LIF", sync_bn=False, use_pretrained_model=False,
                                              new_exp_folder=str(tmp_path / "never")), **kw))
    monkeypatch.delenv("SPARCH_LENGTHS", raising=False)
    monkeypatch.setenv("SPARCH_PER_STEP_LOSS", "half")
    with pytest.raises(ValueError, match="SPARCH_PER_STEP_LOSS"):
        exp.Experiment(args())
    monkeypatch.setenv("SPARCH_PER_STEP_LOSS", "0.5:10")
    with pytest.raises(ValueError, match="SPARCH_PER_STEP_LOSS needs a spiking model"):
        exp.Experiment(args(model_type="MLP"))
    monkeypatch.setenv("SPARCH_LENGTHS", "pack")
    with pytest.raises(ValueError, match="SPARCH_PER_STEP_LOSS with SPARCH_LENGTHS=pack"):
        exp.Experiment(args())
    assert not (tmp_path / "never").exists()


# seq_sum (2, 5, 3): clip 0, label 2 — argmax 0, 2, 1, 2, 2: right from step 3 on; clip 1, label 0 — argmax 0, 0, 1, (0, 0)
HAND = torch.tensor([[[.5, .2, .3], [.6, .5, .9], [.9, 1.2, .9], [1., 1.3, 1.7], [1.2, 1.4, 2.4]],
                     [[.8, .1, .1], [1.5, .3, .2], [1.6, 1.9, .5], [2.6, 1., .4], [3.6, 1., .4]]])
HAND_Y = torch.tensor([2, 0])


def test_decision_step_on_a_hand_made_tensor():
    from sparch_amd import exp
    assert exp.decision_steps(HAND, HAND_Y).tolist() == [3, 3]
    assert exp.decision_steps(HAND, HAND_Y, torch.tensor([5, 3])).tolist() == [3, 3]   # clip 1 never settles: its length
    assert exp.decision_steps(HAND, HAND_Y, torch.tensor([3, 2])).tolist() == [3, 0]   # clip 0 too; clip 1 right at once
    assert exp.decision_steps(HAND, HAND_Y, torch.tensor([2, 1])).tolist() == [1, 0]
    assert exp.decision_steps(HAND, torch.tensor([1, 1])).tolist() == [5, 5]


def test_per_step_loss_on_a_hand_made_tensor():
    from sparch_amd import exp
    at = [[.3, .9, .9, 1.7, 2.4], [.8, 1.5, 1.6, 2.6, 3.6]]

    def want(pairs):
        return sum(-math.log(at[b][t] / (t + 1)) for b, t in pairs) / len(pairs)
    full = [(b, t) for b in range(2) for t in range(5)]
    assert float(exp.per_step_nll(HAND, HAND_Y)) == pytest.approx(want(full), rel=1e-6)
    assert float(exp.per_step_nll(HAND, HAND_Y, None, 3)) == pytest.approx(want([p for p in full if p[1] >= 3]), rel=1e-6)
    lens = torch.tensor([4, 2])
    pairs = [(0, 1), (0, 2), (0, 3), (1, 1)]
    assert float(exp.per_step_nll(HAND, HAND_Y, lens, 1)) == pytest.approx(want(pairs), rel=1e-6)
    assert float(exp.per_step_nll(HAND, HAND_Y, lens, 4)) == 0.0
    # the padding's values are never looked at, and no gradient goes there
    seq = HAND.clone()
    seq[0, 4:], seq[1, 2:] = 0.0, 0.0
    seq.requires_grad_(True)
    loss = exp.per_step_nll(seq, HAND_Y, lens, 1)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(want(pairs), rel=1e-6) and torch.isfinite(seq.grad).all()
    assert not seq.grad[0, 4:].any() and not seq.grad[1, 2:].any() and not seq.grad[:, 0].any()
