"""CPU: what streaming the non-spiking baselines (sparch_amd/streaming_ann.py, csrc/streamann.hip) rests on and what
it refuses, without a device.

* the restatement tests/stream_ann_numpy.py, stepped in fp64 over the unidirectional ANN fixtures (parameters
  param.*, running statistics after.*), equals the real reference's own eval-mode output `out_eval` within the bar
  tests/test_oracle_golden.py holds oracle.ann_oracle to (rtol 2e-5, atol 2e-6);
* a step needs the carried state and nothing else: chunkings [1, 7, 1, ...] are bit-equal to chunks of 1;
* the constructor's refusals come before any device use, and StreamingSNN keeps refusing a baseline;
* the two entry points validate their arguments and return their codes without launching.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import stream_ann_numpy as sn
from tests.golden_io import load
from tests.kit import EALIGN, EINVAL

FIXTURES = ["ann_MLP_bn", "ann_RNN_bn", "ann_LiGRU_bn", "ann_GRU_bn", "ann_MLP_ln_bias_noreadout"]


def _chunks(T):
    cuts, pattern, i = [], [1, 7], 0
    while sum(cuts) < T:
        cuts.append(min(pattern[i % 2], T - sum(cuts)))
        i += 1
    return cuts


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_stepped_in_fp64_equals_the_reference_eval_output(name):
    z = load(name)
    cfg, layers = sn.network(z)
    x = z["x"].astype(np.float64)
    state = sn.zero_state(layers, cfg["B"])
    out = None
    outs = []
    for t in range(cfg["T"]):
        out = sn.stream(layers, state, x[:, t:t + 1])
        outs.append(out)
    got = out if cfg["use_readout_layer"] else np.concatenate(outs, axis=1)
    np.testing.assert_allclose(got, z["out_eval"], rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_in_chunks_is_bit_equal_to_chunks_of_one(name, dtype):
    z = load(name)
    cfg, layers = sn.network(z)
    x = z["x"].astype(dtype)
    T = cfg["T"]
    cuts = _chunks(T)
    assert cuts[:3] == [1, 7, 1] and sum(cuts) == T

    def run(cs):
        state, t0, outs = sn.zero_state(layers, cfg["B"], dtype), 0, []
        for n in cs:
            outs.append(sn.stream(layers, state, x[:, t0:t0 + n], dtype))
            t0 += n
        return (outs[-1] if cfg["use_readout_layer"] else np.concatenate(outs, axis=1)), state

    a, sa = run([1] * T)
    b, sb = run(cuts)
    assert a.dtype == dtype and np.array_equal(a, b)
    assert all(np.array_equal(p, q) for p, q in zip(sa, sb))


def test_constructor_refusals_come_before_any_device_use():
    import sparch_amd
    from sparch_amd import anns
    from sparch_amd import functional as Fn

    torch.manual_seed(3)
    snn = sparch_amd.SNN((4, None, 12), [16, 16, 5], neuron_type="RadLIF").eval()
    with pytest.raises(ValueError, match="StreamingSNN"):
        sparch_amd.StreamingANN(snn, 4)
    bidir = anns.ANN((4, None, 12), [16, 16, 5], ann_type="GRU", bidirectional=True).eval()
    with pytest.raises(ValueError, match="not causal"):
        sparch_amd.StreamingANN(bidir, 4)
    net = anns.ANN((4, None, 12), [16, 16, 5], ann_type="LiGRU")
    assert net.training
    with pytest.raises(ValueError, match="training mode"):
        sparch_amd.StreamingANN(net, 4)
    net.eval()
    prev = Fn.set_compute_dtype("bf16")
    try:
        with pytest.raises(ValueError, match="bf16"):
            sparch_amd.StreamingANN(net, 4)
    finally:
        Fn.set_compute_dtype(prev)
    st = sparch_amd.StreamingANN(net, 4, graph=True)      # CPU parameters: fine until the first use
    assert st.steps_seen == 0 and st.batch_size == 4 and st.row_steps.tolist() == [0, 0, 0, 0]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.reset()
    for kind in ("MLP", "RNN", "LiGRU", "GRU"):            # StreamingSNN keeps refusing the baselines
        with pytest.raises(ValueError):
            sparch_amd.StreamingSNN(anns.ANN((4, None, 12), [16, 5], ann_type=kind).eval(), 4)


P = 16    # any non-NULL, 16-byte aligned value: nothing is dereferenced before the checks
Q = 32    # another one
ODD = 20  # non-NULL, not 16-byte aligned
MLP, RNN, LIGRU, GRU = 0, 1, 2, 3


def _arr(*slots):
    return (ctypes.c_void_p * 3)(*slots)


def step(cell=RNN, phase=0, act=0, B=2, K=8, H=8, ld=8, x=P, ldx=8, W=(P, P, P), bias=None, scale=None, shift=None,
         pre=None, V=(P, P, P), y_in=P, y_out=Q, z=48, ry=64):
    from sparch_amd._capi import lib
    a = lambda v: None if v is None else _arr(*v)  # noqa: E731
    return lib.sparch_ann_stream_step(cell, phase, act, B, K, H, ld, x, ldx, a(W), a(bias), a(scale), a(shift), a(pre),
                                      a(V), y_in, y_out, z, ry, None)


def test_step_entry_point_validates_without_launching():
    N3 = (None, None, None)
    # unknown cell, phase, activation
    assert step(cell=4) == EINVAL and step(cell=-1) == EINVAL
    assert step(cell=RNN, phase=1) == EINVAL and step(cell=MLP, phase=2) == EINVAL and step(cell=LIGRU, phase=1) == EINVAL
    assert step(cell=GRU, phase=0) == EINVAL and step(cell=GRU, phase=3) == EINVAL
    assert step(cell=RNN, act=3) == EINVAL and step(cell=MLP, act=-1) == EINVAL
    # sizes and strides
    for kw in ({"B": 0}, {"K": 0}, {"H": 0}, {"B": -3}, {"ld": 7}, {"ldx": 7}):
        assert step(**kw) == EINVAL, kw
    # a missing operand of the cell
    assert step(W=None) == EINVAL and step(W=(None, P, P)) == EINVAL            # slot 0 is the RNN's
    assert step(V=None) == EINVAL and step(V=(None, P, P)) == EINVAL
    assert step(y_in=None) == EINVAL and step(y_out=None) == EINVAL
    assert step(cell=LIGRU, W=(P, None, P)) == EINVAL and step(cell=LIGRU, V=(P, None, P)) == EINVAL
    assert step(cell=GRU, phase=1, W=(P, P, None)) == EINVAL and step(cell=GRU, phase=1, V=(P, None, P)) == EINVAL
    assert step(cell=GRU, phase=1, z=None) == EINVAL and step(cell=GRU, phase=1, ry=None) == EINVAL
    assert step(cell=GRU, phase=2, W=(None, P, P)) == EINVAL and step(cell=GRU, phase=2, z=None) == EINVAL
    assert step(cell=GRU, phase=2, ry=None) == EINVAL and step(cell=GRU, phase=2, y_out=None) == EINVAL
    assert step(x=None) == EINVAL and step(x=None, pre=(None, P, P)) == EINVAL   # no x: the projection must be given
    # scale without shift (and the reverse)
    assert step(scale=(P, None, None)) == EINVAL and step(shift=(P, None, None)) == EINVAL
    assert step(cell=LIGRU, scale=(P, P, None), shift=(P, None, None)) == EINVAL
    # aliased state in and out where every workgroup reads all of the input
    assert step(y_out=P) == EINVAL and step(cell=LIGRU, y_out=P) == EINVAL
    assert step(cell=GRU, phase=1, z=P) == EINVAL and step(cell=GRU, phase=1, ry=P) == EINVAL
    assert step(cell=GRU, phase=1, z=64, ry=64) == EINVAL
    assert step(cell=GRU, phase=2, y_out=64) == EINVAL and step(cell=GRU, phase=2, y_out=48) == EINVAL
    # more than 65535 row tiles of 16
    assert step(B=65535 * 16 + 1) == EINVAL
    # every SPARCH_EINVAL comes before SPARCH_EALIGN
    assert step(W=(ODD, P, P), ld=7) == EINVAL and step(y_in=ODD, y_out=ODD) == EINVAL
    # alignment of a weight or state base
    assert step(W=(ODD, P, P)) == EALIGN and step(V=(ODD, P, P)) == EALIGN
    assert step(y_in=ODD) == EALIGN and step(y_out=ODD) == EALIGN
    assert step(cell=LIGRU, W=(P, ODD, P)) == EALIGN and step(cell=LIGRU, V=(P, ODD, P)) == EALIGN
    assert step(cell=GRU, phase=1, z=ODD) == EALIGN and step(cell=GRU, phase=2, ry=ODD) == EALIGN
    # slots the launch does not read are not looked at
    assert step(cell=MLP, W=(ODD, P, P), V=N3, y_in=None) == EALIGN                 # valid up to the alignment
    assert step(cell=LIGRU, W=(P, P, None), V=(P, P, ODD), y_out=ODD) == EALIGN     # slot 2 is not the LiGRU's


def readout(B=2, K=8, C=5, y=P, ldy=8, acc=P, W=P, bias=None, norm=0, p0=None, p1=None, out=P):
    from sparch_amd._capi import lib
    return lib.sparch_ann_stream_readout(B, K, C, y, ldy, acc, W, bias, norm, p0, p1, 1e-5, out, None)


def test_readout_entry_point_validates_without_launching():
    from sparch_amd._capi import lib
    for kw in ({"B": 0}, {"K": 0}, {"C": 0}, {"K": 4097, "ldy": 4097}, {"C": 257}, {"ldy": 7}, {"y": None}, {"acc": None},
               {"W": None}, {"out": None}, {"norm": 3}, {"norm": -1}, {"norm": 1}, {"norm": 1, "p0": P},
               {"norm": 2, "p1": P}):
        assert readout(**kw) == EINVAL, kw
    assert readout(W=ODD, C=257) == EINVAL                     # EINVAL before EALIGN
    assert readout(W=ODD) == EALIGN and readout(acc=ODD) == EALIGN
    assert readout(W=ODD, norm=2, p0=P, p1=P) == EALIGN
    assert lib.sparch_abi_version() == 5                       # additive: the ABI version stays
