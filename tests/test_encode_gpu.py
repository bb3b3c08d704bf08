"""
The spike encoders on the device (csrc/encode.hip through `sparch_spike_encode`, sparch_amd.encoders; DESIGN.md section
6, "Spike encoders") against the float32 restatement tests/encode_numpy.py.  The library is built without fused
multiply-adds and every code is a handful of fp32 operations per element, so everything is compared BIT FOR BIT: the
byte counts, the fp32 tensor, the bf16 plane with its pad columns (filled with ones before the call), the totals and the
final state.

Shapes (B,T,K): (1,1,1), (3,7,5), (2,9,8) and (4,T,40) with T in {1, D-1, D, D+1, 2D+3}, D the scan kernels' prefetch
depth; K' = 5 and 10 leave pad columns, and one plane is a whole group of 8 wider than it needs to be.  Lengths
[1, 2, T-1, T]; a carried state; a step count past 2^32 for the rate code's 64-bit index; every subset of the outputs;
chunks [1, 3, rest] through StreamingSpikeEncoder; saturation and non-finite features.  End to end: the network on the
encoder's tagged input equals the network on the same spikes as a dense tensor (out, rates, every gradient), a
StreamingSNN takes a tagged chunk, and run_exp.py trains under SPARCH_ENCODE.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import encode_numpy as en
from tests import network_cases as nc
from tests.kit import DEV, F32, D, N, bits, ptr, same_bits
from tests.kit import sp  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEPTH = 8                                   # SPARCH_ENCODE_PREFETCH (tests/test_encode_host.py holds it to the header)
CODES = {"rate": en.RATE, "if": en.IF, "delta": en.DELTA}
SHAPES = [(1, 1, 1), (3, 7, 5), (2, 9, 8)] + [(4, T, 40) for T in (1, DEPTH - 1, DEPTH, DEPTH + 1, 2 * DEPTH + 3)]
SHAPES += [(2, 3, 12),          # K % 4 == 0 with a last column group that is not full: quads and single loads in one row
           (300, 2, 40)]        # more rows than one workgroup of the flat pass holds, more than one workgroup of a scan
SEED = 0x0123456789ABCDEF


def features(B, T, K, seed):
    """Features that cross both clamps of every code: mostly in [-1, 3], every 11th element large."""
    rng = np.random.default_rng([seed, B, T, K])
    x = rng.uniform(-1.0, 3.0, (B, T, K)).astype(F32)
    flat = x.reshape(-1)
    flat[::11] *= F32(40.0)
    return x


def params(code, K, seed=3):
    rng = np.random.default_rng([seed, K])
    lo = rng.uniform(-0.5, 0.5, K).astype(F32)
    top = {en.RATE: 0.4, en.IF: 1.3, en.DELTA: 2.1}[code]
    return lo, rng.uniform(0.5 * top, top, K).astype(F32)


def run_entry(code, x, lo, scale, state=None, lengths=None, seed=SEED, t0=0, ldp=None, want=("plane", "counts", "dense")):
    """One call of the entry point: {counts, dense, plane (uint16 words), totals, state} as host arrays."""
    from sparch_amd._capi import check, lib
    B, T, K = x.shape
    KW = en.width(code, K)
    ldp = (KW + 7) // 8 * 8 if ldp is None else ldp
    xd, lod, scd = D(x), D(lo), D(scale)
    fresh = state is None
    st = None if code == en.RATE else (torch.full((B, K), float("nan"), device=DEV) if fresh else D(state))
    plane = torch.full((B * T, ldp), 1.0, dtype=torch.bfloat16, device=DEV) if "plane" in want else None
    counts = torch.full((B, T, KW), 77, dtype=torch.uint8, device=DEV) if "counts" in want else None
    dense = torch.full((B, T, KW), float("nan"), device=DEV) if "dense" in want else None
    totals = torch.full((KW,), 5, dtype=torch.int32, device=DEV)
    lens = None if lengths is None else D(np.asarray(lengths, np.int32))
    check(lib.sparch_spike_encode(code, B, T, K, ptr(xd), ptr(lod), ptr(scd), ptr(st), int(fresh), t0, seed, ptr(lens),
                                  ptr(plane), ldp, ptr(counts), ptr(dense), ptr(totals),
                                  torch.cuda.current_stream().cuda_stream), "sparch_spike_encode")
    return dict(counts=N(counts), dense=N(dense), plane=None if plane is None else bits(plane), state=N(st),
                totals=N(totals).astype(np.int64) - 5)


def check_against(code, got, x, lo, scale, state=None, lengths=None, seed=SEED, t0=0, ldp=None):
    ref, ref_state = en.encode(code, x, lo, scale, state=state, lengths=lengths, seed=seed, t0=t0)
    dense, plane, totals = en.outputs(ref, ldp)
    if got["counts"] is not None:
        assert got["counts"].dtype == np.uint8 and np.array_equal(got["counts"], ref)
    if got["dense"] is not None:
        assert same_bits(got["dense"], dense)
    if got["plane"] is not None:
        assert got["plane"].shape == plane.shape and np.array_equal(got["plane"], plane)    # the pad columns too
    assert np.array_equal(got["totals"], totals.astype(np.int64))
    if code != en.RATE:
        assert same_bits(got["state"], ref_state)
    return ref


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("code", list(CODES), ids=str)
def test_entry_equals_the_restatement(code, shape):
    c = CODES[code]
    B, T, K = shape
    x = features(B, T, K, 1)
    lo, scale = params(c, K)
    ref = check_against(c, run_entry(c, x, lo, scale), x, lo, scale)
    if B * T * K >= 35 and not (c == en.DELTA and T == 1):
        assert ref.any() and (ref == 0).any()
    # a carried state and a step count: the next chunk of a stream (the rate code's index past 2^32)
    state = None if c == en.RATE else np.random.default_rng(5).uniform(0, 1, (B, K)).astype(F32)
    t0 = (1 << 40) + 3
    check_against(c, run_entry(c, x, lo, scale, state=state, t0=t0), x, lo, scale, state=state, t0=t0)


@pytest.mark.parametrize("K", [2056, 1001], ids=["own-slots", "shared-slots"])
def test_rate_rows_past_one_sweep_and_wide_inputs(K):
    """The flat pass runs about 2^18 threads, 2^18 / (ldp / 8) row lanes: 1100 rows of 2056 columns and 2200 rows of
    1001 take a second sweep; from 256 column groups on (K > 2040) a workgroup's threads add their own totals."""
    B, T = 2, 550 if K > 2040 else 1100
    assert B * T > (1 << 18) // ((K + 7) // 8)
    x = features(B, T, K, 13)
    lo, scale = params(en.RATE, K)
    ref = check_against(en.RATE, run_entry(en.RATE, x, lo, scale, t0=7), x, lo, scale, t0=7)
    assert ref.any()


@pytest.mark.parametrize("code", list(CODES), ids=str)
def test_lengths_mask_the_emission_and_freeze_the_state(code):
    c = CODES[code]
    B, T, K = 4, 2 * DEPTH + 3, 40
    x = features(B, T, K, 2)
    lo, scale = params(c, K)
    lengths = [1, 2, T - 1, T]
    ref = check_against(c, run_entry(c, x, lo, scale, lengths=lengths), x, lo, scale, lengths=lengths)
    assert ref[3].any() and not ref[0, 1:].any() and not ref[2, T - 1:].any()
    B, T, K = 4, 4, 5                                                      # T itself among the lengths, K' = 5 / 10
    x = features(B, T, K, 3)
    lo, scale = params(c, K)
    lengths = [1, 2, T - 1, T]
    check_against(c, run_entry(c, x, lo, scale, lengths=lengths), x, lo, scale, lengths=lengths)


@pytest.mark.parametrize("want", [("plane",), ("counts",), ("dense",), ("plane", "dense"), ("counts", "dense"),
                                  ("plane", "counts")], ids="+".join)
@pytest.mark.parametrize("code", list(CODES), ids=str)
def test_every_subset_of_the_outputs(code, want):
    c = CODES[code]
    x = features(3, 7, 5, 4)
    lo, scale = params(c, 5)
    got = run_entry(c, x, lo, scale, want=want)
    assert [k for k in ("plane", "counts", "dense") if got[k] is not None] == list(want)
    check_against(c, got, x, lo, scale)


@pytest.mark.parametrize("code", list(CODES), ids=str)
def test_a_plane_wider_than_it_needs_to_be_has_zero_pad(code):
    c = CODES[code]
    B, T, K = 2, 9, 5
    ldp = (en.width(c, K) + 7) // 8 * 8 + 8
    x = features(B, T, K, 6)
    lo, scale = params(c, K)
    got = run_entry(c, x, lo, scale, ldp=ldp)
    check_against(c, got, x, lo, scale, ldp=ldp)
    assert got["plane"].shape == (B * T, ldp) and not got["plane"][:, en.width(c, K):].any()


def test_saturation():
    F = F32
    x = np.zeros((1, 6, 2), F)
    x[0, :, 0] = [0, 300, 300, 300, -10, -10]                              # feature 0: a jump of 300, then one of -310
    x[0, :, 1] = [1000, np.inf, 0.5, 0.5, 0.25, 0.25]
    lo, scale = np.zeros(2, F), np.ones(2, F)
    d = check_against(en.DELTA, run_entry(en.DELTA, x, lo, scale), x, lo, scale)
    assert d[0, :, 0].tolist() == [0, 255, 45, 0, 0, 0] and d[0, :, 2].tolist() == [0, 0, 0, 0, 255, 55]
    i = check_against(en.IF, run_entry(en.IF, x, lo, scale), x, lo, scale)
    assert i[0, :, 1].tolist() == [255, 255, 0, 1, 0, 0] and i[0, :, 0].tolist() == [0, 255, 255, 255, 0, 0]
    r = check_against(en.RATE, run_entry(en.RATE, x, lo, scale), x, lo, scale)
    assert r[0, :, 0].tolist() == [0, 1, 1, 1, 0, 0]                        # p = 0 and p = 1 are certain


@pytest.mark.parametrize("code", list(CODES), ids=str)
def test_non_finite_features(code):
    c = CODES[code]
    B, T, K = 2, DEPTH + 3, 5
    x = features(B, T, K, 7)
    x[0, 0, 0], x[0, 3, 1], x[1, 4] = np.nan, np.inf, [np.nan, np.inf, -np.inf, np.nan, 1.0]
    x[1, 0, 2], x[0, T - 1, 3] = -np.inf, np.nan
    lo, scale = params(c, K)
    ref = check_against(c, run_entry(c, x, lo, scale), x, lo, scale)
    if c == en.DELTA:
        assert not ref[1, 4, :4].any() and not ref[1, 4, K:K + 4].any()


# ------------------------------------------------------------------------------------------------ the module
@pytest.mark.parametrize("code", list(CODES), ids=str)
def test_encoder_outputs_and_totals(sp, code):
    from sparch_amd import functional as Fn
    c = CODES[code]
    B, T, K = 3, 7, 5
    x = features(B, T, K, 8)
    enc = sp.SpikeEncoder(code, K, delta=0.75) if code == "delta" else sp.SpikeEncoder(code, K, lo=-0.5, hi=2.5, gain=1.25)
    lo, scale = enc.lo.numpy(), enc.scale.numpy()
    ref, _ = en.encode(c, x, lo, scale, seed=41)
    dense, plane, totals = en.outputs(ref)
    xd = D(x)
    counts = enc.encode(xd, out="counts", seed=41)
    assert counts.dtype == torch.uint8 and np.array_equal(N(counts), ref)
    assert same_bits(N(enc.encode(xd, out="dense", seed=41)), dense)
    tagged = enc.encode(xd, seed=41)
    assert tuple(tagged.shape) == (B, T, enc.out_features) and tagged.dtype == torch.float32
    got_plane, flag = Fn.input_plane_of(tagged)
    assert np.array_equal(bits(got_plane), plane) and N(flag).tolist() == [1, 1, 1, 1]
    assert np.array_equal(bits(Fn.input_plane_of(Fn.input_from_counts(counts))[0]), plane)   # what input_from_counts makes
    assert enc.totals().tolist() == (3 * totals.astype(np.int64)).tolist() and not enc.totals().any()
    lengths = [7, 1, 4]
    ref_l, _ = en.encode(c, x, lo, scale, lengths=lengths, seed=41)
    assert np.array_equal(N(enc.encode(xd, lengths=lengths, out="counts", seed=41)), ref_l)
    assert np.array_equal(N(enc.encode(xd, lengths=torch.tensor(lengths, device=DEV), out="counts", seed=41)), ref_l)
    with pytest.raises(ValueError, match="no gradient"):
        enc.encode(xd.clone().requires_grad_(True))
    if code == "rate":                                                     # without a seed: the encoder's own sequence
        twin = sp.SpikeEncoder(code, K, lo=-0.5, hi=2.5, gain=1.25, seed=enc.base_seed)
        twin.calls = enc.calls
        a, b, c2 = enc.encode(xd, out="counts"), twin.encode(xd, out="counts"), enc.encode(xd, out="counts")
        assert torch.equal(a, b) and not torch.equal(a, c2)


@pytest.mark.parametrize("code", list(CODES), ids=str)
def test_chunks_equal_the_whole_sequence(sp, code):
    from sparch_amd import functional as Fn
    c = CODES[code]
    B, T, K = 4, 2 * DEPTH + 3, 40
    x = features(B, T, K, 9)
    enc = sp.SpikeEncoder(code, K, delta=0.6) if code == "delta" else sp.SpikeEncoder(code, K, lo=-0.25, hi=3.0)
    xd = D(x)
    whole = enc.encode(xd, out="counts", seed=99)
    assert np.array_equal(N(whole), en.encode(c, x, enc.lo.numpy(), enc.scale.numpy(), seed=99)[0])
    whole_plane = bits(Fn.input_plane_of(enc.encode(xd, seed=99))[0]).reshape(B, T, -1)
    stream = sp.StreamingSpikeEncoder(enc, B, seed=99)
    for rounds in range(2):                                                # (the second round: after a reset)
        parts, planes, at = [], [], 0
        for n in (1, 3, T - 4):
            chunk = xd[:, at:at + n]
            if rounds == 0:
                parts.append(stream.push(chunk, out="counts"))
            else:
                tagged = stream.push(chunk)
                planes.append(bits(Fn.input_plane_of(tagged)[0]).reshape(B, n, -1))
            at += n
        assert stream.t0 == T
        if rounds == 0:
            assert torch.equal(torch.cat(parts, dim=1), whole)
            if code != "rate":
                ref_state = en.encode(c, x, enc.lo.numpy(), enc.scale.numpy())[1]
                assert same_bits(N(stream.state), ref_state)
        else:
            assert np.array_equal(np.concatenate(planes, axis=1), whole_plane)
        stream.reset(seed=99)


def test_calibrate_sets_the_range_from_the_valid_steps(sp):
    B, T, K = 3, 6, 4
    x = features(B, T, K, 10)
    x[1, 2, 0] = np.nan
    x[:, :, 3] = 2.0
    lengths = [6, 2, 4]
    enc = sp.SpikeEncoder("if", K).calibrate(D(x), lengths=lengths)
    ok = (np.arange(T)[None, :] < np.asarray(lengths)[:, None])[:, :, None] & np.isfinite(x)
    lo = np.where(ok, x, np.inf).min((0, 1))
    hi = np.where(ok, x, -np.inf).max((0, 1))
    assert enc.lo.numpy().tolist() == lo.tolist()
    assert enc.hi.numpy()[:3].tolist() == hi[:3].tolist() and enc.hi[3] == 3.0   # a feature that does not move: lo + 1
    assert same_bits(enc.scale.numpy(), (F32(1.0) / (enc.hi.numpy() - enc.lo.numpy())).astype(F32))


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("index", [76, 63], ids=lambda i: nc.label(nc.draw(i)))
def test_network_on_the_tagged_input_equals_the_dense_spikes(sp, index):
    """The smallest LIF and RadLIF cases of tests/network_cases.py, their input replaced by encoded features: both
    arms read the same exact bf16 plane, so out, the rates and every parameter gradient are equal."""
    from sparch_amd import functional as Fn
    c = nc.case(index)
    cfg = c["cfg"]
    assert cfg["kind"] == {76: "LIF", 63: "RadLIF"}[index]
    B, T, C = cfg["B"], cfg["T"], cfg["C"]
    enc = sp.SpikeEncoder("if", C, lo=-0.5, hi=1.5)
    xd = D(features(B, T, C, 11))
    net, _ = nc.build(sp, cfg)
    net = net.to(DEV).train(cfg["training"])
    res = []
    for out in ("input", "dense"):
        x = enc.encode(xd, out=out)
        assert (Fn.input_plane_of(x) is not None) == (out == "input")
        net.zero_grad(set_to_none=True)
        with nc.injected_states(c):
            o, rates = net(x)
            loss = nc.loss_of(cfg, o, rates, None if c["y"] is None else c["y"].to(DEV),
                              None if c["gout"] is None else c["gout"].to(DEV))
            loss.backward()
        Fn.check_status()
        res.append((o.detach().clone(), rates.detach().clone(),
                    {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}))
    (o1, r1, g1), (o2, r2, g2) = res
    assert bool(torch.isfinite(o1).all()) and bool(r1.any())
    assert torch.equal(o1, o2) and torch.equal(r1, r2)
    assert list(g1) == list(g2) and len(g1) >= 2 and "snn.0.W.weight" in g1
    for name in g1:
        assert torch.equal(g1[name], g2[name]), name
    assert bool(g1["snn.0.W.weight"].any())


def test_streaming_snn_takes_a_tagged_chunk(sp):
    B, T, K = 3, 6, 8
    torch.manual_seed(3)
    net = sp.SNN((B, None, K), [16, 16, 5], neuron_type="adLIF", normalization="batchnorm").to(DEV).eval()
    enc = sp.SpikeEncoder("if", K, lo=-0.5, hi=1.0)
    xd = D(features(B, T, K, 12))
    outs = []
    for tagged in (True, False):
        torch.manual_seed(4)
        stream = sp.StreamingSNN(net, B)
        stream.reset()
        se = sp.StreamingSpikeEncoder(enc, B)
        got = [stream.step(se.push(xd[:, a:b], out="input" if tagged else "counts")) for a, b in ((0, 1), (1, 4), (4, 6))]
        outs.append(got[-1].clone())
        assert stream.steps_seen == T
    assert bool(torch.isfinite(outs[0]).all()) and bool(outs[0].any()) and torch.equal(outs[0], outs[1])


def test_run_exp_trains_with_sparch_encode(tmp_path):
    """run_exp.py --dataset_name sc --synthetic 1 under SPARCH_ENCODE=if:..., in a child process: a finite loss, and
    every epoch logs the input spike density."""
    exp = tmp_path / "exp"
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPARCH_")}
    env["SPARCH_ENCODE"] = "if:gain=0.5,lo=-16,hi=8"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "run_exp.py"), "--model_type", "adLIF", "--dataset_name", "sc",
                          "--synthetic", "1", "--synthetic_batches", "2", "--nb_epochs", "1", "--nb_layers", "3",
                          "--nb_hiddens", "32", "--batch_size", "8", "--log_tofile", "1", "--save_best", "0",
                          "--new_exp_folder", str(exp)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    text = (exp / "log" / "exp.log").read_text()
    assert "Input features are encoded as spikes on the device" in text and "(SPARCH_ENCODE)" in text
    lines = [ln for ln in text.splitlines() if "input spike density=" in ln]
    assert any(ln.startswith("Epoch 1: train input spike density=") for ln in lines)
    assert any(ln.startswith("Epoch 1: valid input spike density=") for ln in lines)
    density = float(lines[0].split("density=")[1].split()[0])
    assert 0.0 < density < 255.0
    losses = [float(ln.split("train loss=")[1]) for ln in text.splitlines() if "train loss=" in ln]
    assert len(losses) == 1 and all(np.isfinite(v) for v in losses) and "nan" not in text.lower()
