"""
Spike encoders (sparch_amd.encoders, `sparch_spike_encode`, SPARCH_ENCODE) without a GPU:
  * the two entry points are declared, bound and exported; the widths; every refusal of the entry point returns its
    code before any device work;
  * `parse_encode` accepts and rejects what it should; the encoder's constructor, range and seed sequence;
  * a CPU tensor and a tensor that wants a gradient are refused; `functional.input_from_plane` checks its plane;
  * Experiment's SPARCH_ENCODE refusals.
"""
import argparse
import os
import re

import pytest
import torch

from tests.entry_probes import MIS, Entry, P, ptrs
from tests.kit import EINVAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EALIGN = -2
RATE, IF, DELTA = 0, 1, 2
ENC = Entry("sparch_spike_encode", [("code", IF), ("B", 2), ("T", 3), ("K", 5)] + ptrs("x lo scale state")
            + [("fresh", 1), ("t0", 0), ("seed", 0), ("lengths", None), ("plane", P), ("ldp", 16), ("counts", P), ("dense", P),
               ("totals", None), ("stream", None)])


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entries_are_declared_bound_and_exported():
    from sparch_amd._capi import PROTOTYPES, lib
    assert lib.sparch_abi_version() == 5                                    # additive: the ABI version stays
    with open(os.path.join(ROOT, "include", "sparch_hip.h")) as f:
        header = f.read()
    decl = re.search(r"\bint sparch_spike_encode\(([^;]*)\);", header)
    params = [q.strip() for q in decl.group(1).replace("\n", " ").split(",")]
    assert len(params) == len(ENC.args) == len(PROTOTYPES["sparch_spike_encode"][1])
    assert [q.split()[-1].lstrip("*") for q in params] == [k for k, _ in ENC.args]
    assert re.search(r"\bint sparch_spike_encode_width\(int code, int K\);", header)
    assert hasattr(lib, "sparch_spike_encode") and hasattr(lib, "sparch_spike_encode_width")
    assert os.path.exists(os.path.join(ROOT, "sparch_amd", "csrc", "encode.hip"))
    from sparch_amd import encoders
    depth = int(re.search(r"#define SPARCH_ENCODE_PREFETCH (\d+)", header).group(1))
    assert encoders.PREFETCH_DEPTH == depth >= 2
    for name, code in (("RATE", RATE), ("IF", IF), ("DELTA", DELTA)):
        assert re.search(rf"#define SPARCH_ENCODE_{name} {code}\b", header)
        assert encoders.CODES[name.lower()] == code


def test_widths():
    from sparch_amd._capi import lib
    w = lib.sparch_spike_encode_width
    assert w(RATE, 40) == 40 and w(IF, 40) == 40 and w(DELTA, 40) == 80 and w(DELTA, 1) == 2
    assert w(3, 40) == 0 and w(-1, 40) == 0 and w(IF, 0) == 0 and w(DELTA, -4) == 0
    assert w(DELTA, 1 << 30) == 0                                           # 2 K does not fit an int


def test_the_entry_refuses_before_any_device_work():
    """Nothing here reaches a launch: every call has something broken (the pointers are not memory)."""
    for code in (-1, 3, 99):
        assert ENC(code=code) == EINVAL, code
    for code in (RATE, IF, DELTA):
        for k in ("B", "T", "K"):
            assert ENC(code=code, **{k: 0}) == EINVAL and ENC(code=code, **{k: -2}) == EINVAL, (code, k)
        for p in ("x", "lo", "scale"):
            assert ENC(code=code, **{p: None}) == EINVAL, (code, p)
        assert ENC(code=code, plane=None, counts=None, dense=None) == EINVAL
        assert ENC(code=code, t0=-1) == EINVAL
        assert ENC(code=code, ldp=12) == EINVAL and ENC(code=code, ldp=4) == EINVAL       # ldp % 8, ldp < K'
        assert ENC(code=code, plane=MIS) == EALIGN
        assert ENC(code=code, plane=MIS, ldp=12) == EINVAL                                 # the arguments come first
    assert ENC(code=IF, state=None) == EINVAL and ENC(code=DELTA, state=None) == EINVAL
    assert ENC(code=DELTA, ldp=8) == EINVAL                                 # K' = 10 > 8
    assert ENC(code=IF, K=65536, ldp=65536) == EINVAL                       # K' > 65535
    assert ENC(code=DELTA, K=32768, ldp=65536) == EINVAL
    assert ENC(code=DELTA, K=1 << 30, ldp=8) == EINVAL
    # (ldp is checked without a plane too: it is part of the call's shape)
    assert ENC(code=IF, plane=None, ldp=3) == EINVAL


# ------------------------------------------------------------------------------------------------ parse_encode
def test_parse_encode_accepts():
    from sparch_amd import parse_encode
    assert parse_encode(None) is None and parse_encode("") is None and parse_encode("   ") is None
    assert parse_encode("rate") == {"code": "rate"} and parse_encode(" if ") == {"code": "if"}
    assert parse_encode("if:gain=0.5,lo=-16,hi=8") == {"code": "if", "gain": 0.5, "lo": -16.0, "hi": 8.0}
    assert parse_encode("rate: hi = 8 , lo=-16,seed=7") == {"code": "rate", "hi": 8.0, "lo": -16.0, "seed": 7}
    assert parse_encode("delta:delta=1.5") == {"code": "delta", "delta": 1.5}
    assert parse_encode("delta:seed=3") == {"code": "delta", "seed": 3}
    assert parse_encode("if:gain=1e-1") == {"code": "if", "gain": 0.1}


@pytest.mark.parametrize("bad", ["latency", "IF", "if:", "if:gain", "if:gain=", "if:gain=x", "if:gain=0", "if:gain=-1",
                                 "if:delta=1", "delta:gain=2", "delta:lo=0", "delta:delta=0", "delta:delta=-2",
                                 "if:lo=3,hi=3", "if:lo=4,hi=3", "if:hi=-1", "if:gain=1,gain=2", "rate:seed=-1",
                                 "rate:seed=1.5", "if:gain=inf", "if:lo=nan", "if,gain=1", "if:gain=1;lo=0", ":gain=1",
                                 "if:gain=1,", "rate:p=0.5"])
def test_parse_encode_rejects(bad):
    from sparch_amd import parse_encode
    with pytest.raises(ValueError, match="SPARCH_ENCODE"):
        parse_encode(bad)


# ------------------------------------------------------------------------------------------------ the module
def test_encoder_parameters():
    import numpy as np
    from sparch_amd import SpikeEncoder
    e = SpikeEncoder("if", 4, lo=-16, hi=8, gain=0.5)
    assert e.out_features == 4 and e.lo.tolist() == [-16.0] * 4
    assert e.scale.dtype == torch.float32 and e.scale.tolist() == [float(np.float32(0.5) / np.float32(24.0))] * 4
    e = SpikeEncoder("rate", 3, lo=[0, 1, 2], hi=torch.tensor([1.0, 3.0, 6.0]))
    assert e.scale.tolist() == [1.0, 0.5, 0.25] and e.out_features == 3
    d = SpikeEncoder("delta", 40, delta=1.5)
    assert d.out_features == 80 and not d.lo.any() and d.scale.tolist() == [float(np.float32(1) / np.float32(1.5))] * 40
    assert SpikeEncoder.from_spec("if:gain=0.5,lo=-16,hi=8", 4).scale.tolist() == SpikeEncoder("if", 4, -16, 8, 0.5).scale.tolist()
    assert SpikeEncoder.from_spec({"code": "delta", "delta": 2.0}, 5).out_features == 10
    for bad in (dict(code="latency", num_features=4), dict(code="if", num_features=0), dict(code="if", num_features=2.5),
                dict(code="if", num_features=4, lo=1, hi=1), dict(code="if", num_features=4, lo=[0, 0], hi=1),
                dict(code="if", num_features=4, gain=0), dict(code="if", num_features=4, delta=1.0),
                dict(code="delta", num_features=4, lo=0.0), dict(code="delta", num_features=4, gain=2.0),
                dict(code="delta", num_features=4, delta=0.0), dict(code="delta", num_features=40000),
                dict(code="if", num_features=4, hi=float("inf"))):
        with pytest.raises(ValueError, match="SpikeEncoder"):
            SpikeEncoder(**bad)
    with pytest.raises(ValueError, match="delta"):
        d.set_range(0, 1)


def test_seed_sequence_is_host_side_and_repeats():
    from sparch_amd import SpikeEncoder
    a, b = SpikeEncoder("rate", 4, seed=5), SpikeEncoder("rate", 4, seed=5)
    sa = [a.next_seed() for _ in range(4)]
    assert sa == [b.next_seed() for _ in range(4)] and len(set(sa)) == 4 and a.calls == 4
    assert all(0 <= s < 1 << 63 for s in sa)
    assert SpikeEncoder("rate", 4, seed=6).next_seed() != sa[0]
    torch.manual_seed(1234)
    assert SpikeEncoder("rate", 4).base_seed == 1234


def test_host_tensors_and_gradients_are_refused():
    from sparch_amd import SpikeEncoder, StreamingSpikeEncoder
    from sparch_amd import functional as Fn
    e = SpikeEncoder("if", 6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        e.encode(torch.zeros(2, 3, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        StreamingSpikeEncoder(e, 2).push(torch.zeros(2, 3, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        e.calibrate(torch.zeros(2, 3, 6))
    for bad in (torch.zeros(2, 3, 5), torch.zeros(2, 6), torch.zeros(2, 3, 6, dtype=torch.int32)):
        with pytest.raises(ValueError, match="SpikeEncoder"):
            e.encode(bad)
    with pytest.raises(ValueError, match="StreamingSpikeEncoder"):
        StreamingSpikeEncoder("if", 2)
    with pytest.raises(ValueError, match="whole batch"):
        StreamingSpikeEncoder(SpikeEncoder("delta", 6), 2).reset(rows=[0])
    assert StreamingSpikeEncoder(e, 2).push(torch.zeros(2, 0, 6)) is None      # no frame became complete: nothing to do
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fn.input_from_plane(torch.zeros(6, 8, dtype=torch.bfloat16), 2, 3, 6)


# ------------------------------------------------------------------------------------------------ SPARCH_ENCODE
def _args(tmp_path, **kw):
    base = dict(model_type="LIF", sync_bn=False, use_pretrained_model=False, bidirectional=False, compute_dtype="fp32",
                dataset_name="sc", new_exp_folder=str(tmp_path / "never"))
    base.update(kw)
    return argparse.Namespace(**base)


def test_experiment_refuses_before_anything_else(monkeypatch, tmp_path):
    from sparch_amd import exp
    for name in ("SPARCH_LENGTHS", "SPARCH_PER_STEP_LOSS", "SPARCH_READOUT", "SPARCH_SURROGATE", "SPARCH_CLIP_GRAD",
                 "SPARCH_TBPTT", "SPARCH_DELAYS"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv("SPARCH_ENCODE", "latency")
    with pytest.raises(ValueError, match="SPARCH_ENCODE"):
        exp.Experiment(_args(tmp_path))
    monkeypatch.setenv("SPARCH_ENCODE", "if:gain=0.5,lo=-16,hi=8")
    for name in ("shd", "ssc"):
        with pytest.raises(ValueError, match="already spikes"):
            exp.Experiment(_args(tmp_path, dataset_name=name))
    for model in ("MLP", "RNN", "LiGRU", "GRU"):
        with pytest.raises(ValueError, match="SPARCH_ENCODE needs a spiking model"):
            exp.Experiment(_args(tmp_path, model_type=model))
    assert not (tmp_path / "never").exists()


def test_a_model_of_another_input_width_is_refused():
    import sparch_amd
    from sparch_amd import anns, exp
    enc = sparch_amd.SpikeEncoder("delta", 40)
    exp.check_encode_model(sparch_amd.SNN((2, None, 80), [8, 5], neuron_type="LIF"), enc)
    with pytest.raises(ValueError, match="80 input features, the model's first layer takes 40"):
        exp.check_encode_model(sparch_amd.SNN((2, None, 40), [8, 5], neuron_type="LIF"), enc)
    with pytest.raises(ValueError, match="needs a spiking model"):
        exp.check_encode_model(anns.ANN((2, None, 80), [8, 5], ann_type="MLP"), enc)
