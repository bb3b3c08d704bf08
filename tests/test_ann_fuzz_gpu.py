"""
Whole non-spiking baseline networks (MLP / RNN / LiGRU / GRU stacks, with and without ReadoutLayerANN) drawn at random
(tests/ann_cases.py), on the HIP path against the oracle in float64 (tests/ann_net_oracle.py).  The cell kernels are
held to fp64 at the C ABI and single layers to the fp32 oracle elsewhere; what exists only when the layers are composed
is checked here: running statistics copied back from behind a padded width, eval mode, per-layer dropout masks across
stacked layers, the (B, T, dirs, H + extra) slice of a padded bidirectional layer feeding the next layer's K, the
readout's -1e30 feature padding and its gradient into the layer below, LayerNorm over the true width under all three
gates, networks without a readout, 4-D input, the input's gradient, num_batches_tracked, and the same network on the
persistent, chunked and launch-per-step paths.

Every case was kept by a rule that looks at the oracle alone (ann_cases.verdict).  Against the fp64 run:

  out, loss, every parameter gradient, the input's gradient   within ann_cases.bounds(i): 4 x max(|fp32 oracle - fp64
             oracle| of the case, r_role x max-abs), asserted there to lie under 5e-4 / 1e-4 / 1e-5
  W*.bias under train-mode BatchNorm   zero in real arithmetic: finite and at most 1e-4 x max|W.weight.grad| of its layer
  V*.weight (and the GRU's reset gate) over a single step   exactly zero
  running statistics after a training step   rtol 1e-4 / atol 1e-6, every gate's; num_batches_tracked advanced by one
  dropout    every hidden layer's output (a forward hook) is zero exactly where the restated mask is, and non-zero
             wherever the mask keeps an element whose undropped oracle value exceeds 1e-3 of the layer's max-abs
  eval       the forward under torch.no_grad() and the one that saves for a backward give the same bits; the running
             statistics and the counters keep their bits and receive no gradient
  chunk      bit-equal to the same case on the default path (the carry between launches of 3 steps)
  step       the same bounds (another summation order: not bit-equal)
  stream     eval, one-direction cases with T > 1 through StreamingANN in chunks [1, T - 1]: out within bounds(i)["out"]

functional.check_status() follows every forward and backward (ann_cases.device_run).
"""
import numpy as np
import pytest
import torch

from tests import ann_cases as ac
from tests.kit import DEV, N, record, same_bits, within
from tests.kit import sp  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

CASES = list(ac.KEPT) + list(ac.FIXED)
EVAL_CASES = [i for i in ac.KEPT if not ac.draw(i)["training"]]
CHUNK_CASES = [i for i in ac.KEPT if ac.draw(i)["path"] == "chunk"]
STREAM_CASES = [i for i in EVAL_CASES if not ac.draw(i)["bidirectional"] and ac.draw(i)["T"] > 1]


def ids(cases):
    return [ac.label(ac.draw(i)) for i in cases]


def set_path(monkeypatch, cfg, path=None):
    env = ac.PATH_ENV[path or cfg["path"]]
    env = env.get(cfg["kind"], env) if (path or cfg["path"]) == "step" else env
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def gradients(d):
    got = {k: v.grad for k, v in d["net"].named_parameters()}
    assert all(g is not None for g in got.values()), [k for k, g in got.items() if g is None]
    return dict(got, x=d["x"].grad)


def check_against_oracle(i, d, worst):
    """out, loss and every gradient of a device run against the fp64 oracle; the worst fraction of a bound per role
    goes into `worst`."""
    c = ac.case(i)
    cfg = c["cfg"]
    r64, _ = ac.runs(i)
    bound, ref = ac.bounds(i), ac.compared(r64)
    got = dict(out=N(d["out"]), loss=N(d["loss"]), **{k: N(v) for k, v in gradients(d).items()})
    assert set(got) == set(ref)
    for k in sorted(bound):
        f = within(got[k], ref[k].numpy(), bound[k], k)
        worst[ac.role_of(k)] = max(worst.get(ac.role_of(k), 0.0), f)
    for k in sorted(set(ref) - set(bound)):
        assert np.isfinite(got[k]).all(), k
        if ac.structural_zero(cfg, k):
            assert not got[k].any(), (k, "a single step leaves this gradient exactly zero")
        else:
            assert ac.residue(cfg, k)
            top = float(np.abs(got[k[:-len("bias")] + "weight"]).max())
            assert np.abs(got[k]).max() <= 1e-4 * top, (k, float(np.abs(got[k]).max()), top)


def check_statistics(i, d):
    """After a training step under BatchNorm: every running statistic, every gate's, and every counter; otherwise the
    statistics and counters keep their bits."""
    c = ac.case(i)
    cfg = c["cfg"]
    r64, _ = ac.runs(i)
    state, buffers = d["net"].state_dict(), dict(d["net"].named_buffers())
    tracked = [k for k in c["params"] if k.endswith("num_batches_tracked")]
    assert (len(r64["stats"]) > 0) == (cfg["normalization"] == "batchnorm") == (len(tracked) > 0)
    assert len(r64["stats"]) == 2 * len(tracked)
    for k, v in r64["stats"].items():
        assert buffers[k].grad is None and not buffers[k].requires_grad and buffers[k].grad_fn is None, k
        if cfg["training"]:
            np.testing.assert_allclose(N(state[k]), v.numpy(), rtol=1e-4, atol=1e-6, err_msg=k)
        else:
            assert same_bits(state[k].cpu(), c["params"][k]), k
    for k in tracked:
        assert int(state[k]) == int(c["params"][k]) + int(cfg["training"]), k


def check_dropout(i, d):
    c = ac.case(i)
    r64, _ = ac.runs(i)
    assert len(d["hidden"]) == len(r64["hidden"]) == len(c["masks"])
    for k, (got, raw, mask) in enumerate(zip(d["hidden"], r64["hidden"], c["masks"])):
        got = got.cpu()
        assert got.shape == raw.shape == mask.shape
        assert bool((got[mask == 0] == 0).all()), f"layer {k}: an element the mask drops is not zero"
        clear = (raw.abs() > 1e-3 * ac.maxabs(raw)) & (mask != 0)
        assert int(clear.sum()) > 0 and int((mask == 0).sum()) > 0
        assert bool((got[clear] != 0).all()), f"layer {k}: an element the mask keeps is zero"


@pytest.mark.parametrize("i", CASES, ids=ids(CASES))
def test_network_vs_oracle(sp, i, monkeypatch, record_property):
    c = ac.case(i)
    cfg = c["cfg"]
    set_path(monkeypatch, cfg)
    d = ac.device_run(sp, c)
    worst = {}
    check_against_oracle(i, d, worst)
    check_statistics(i, d)
    if cfg["dropout"] > 0:
        check_dropout(i, d)
    print("  worst fraction of the bound per role: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    for k, v in worst.items():
        record_property("fraction_" + k, round(v, 3))
    record(record_property, *worst.values())


@pytest.mark.parametrize("i", CHUNK_CASES, ids=ids(CHUNK_CASES))
def test_chunked_launches_give_the_bits_of_one_launch(sp, i, monkeypatch, record_property):
    """The carry between persistent launches of 3 steps: out, loss, every gradient, the hidden outputs and the running
    statistics equal those of the default path bit for bit."""
    c = ac.case(i)
    with monkeypatch.context() as mp:
        set_path(mp, c["cfg"], "chunk")
        a = ac.device_run(sp, c)
    with monkeypatch.context() as mp:
        set_path(mp, c["cfg"], "default")
        b = ac.device_run(sp, c)
    assert same_bits(a["out"].detach(), b["out"].detach()) and same_bits(a["loss"].detach(), b["loss"].detach())
    ga, gb = gradients(a), gradients(b)
    for k in ga:
        assert same_bits(ga[k], gb[k]), k
    for k, (u, v) in enumerate(zip(a["hidden"], b["hidden"])):
        assert same_bits(u, v), f"hidden layer {k}"
    sa, sb = a["net"].state_dict(), b["net"].state_dict()
    for k in sa:
        assert same_bits(sa[k], sb[k]), k
    record(record_property, 0.0)


@pytest.mark.parametrize("i", EVAL_CASES, ids=ids(EVAL_CASES))
def test_eval_forward_is_the_no_grad_forward(sp, i, monkeypatch, record_property):
    """Eval mode: the forward under torch.no_grad() gives the bits of the forward that saves for a backward, within
    bounds(i)["out"] of the oracle, and leaves the running statistics and counters alone."""
    c = ac.case(i)
    set_path(monkeypatch, c["cfg"])
    a = ac.device_run(sp, c, backward=False)
    b = ac.device_run(sp, c, grad=False)
    assert a["out"].requires_grad and not b["out"].requires_grad
    assert same_bits(a["out"].detach(), b["out"])
    for k, (u, v) in enumerate(zip(a["hidden"], b["hidden"])):
        assert same_bits(u, v), f"hidden layer {k}"
    f = within(N(b["out"]), ac.runs(i)[0]["out"].numpy(), ac.bounds(i)["out"], "out under no_grad")
    check_statistics(i, a)
    check_statistics(i, b)
    record(record_property, f)


@pytest.mark.parametrize("i", STREAM_CASES, ids=ids(STREAM_CASES))
def test_eval_network_streamed_in_two_chunks(sp, i, record_property):
    """StreamingANN fed the clip in chunks [1, T - 1] (the calls of tests/test_stream_ann_gpu.py): the readout's last
    output, or all outputs without one, within bounds(i)["out"] of the whole-sequence oracle."""
    from sparch_amd import functional as Fn
    c = ac.case(i)
    cfg = c["cfg"]
    net, _ = ac.build(sp, cfg)
    st = sp.StreamingANN(net.to(DEV).eval(), cfg["B"])
    st.reset()
    x = c["x"].to(DEV)
    outs = [st.step(x[:, :1]).clone(), st.step(x[:, 1:]).clone()]
    Fn.check_status()
    assert st.steps_seen == cfg["T"]
    got = outs[-1] if cfg["use_readout_layer"] else torch.cat(outs, dim=1)
    f = within(N(got), ac.runs(i)[0]["out"].numpy(), ac.bounds(i)["out"], "streamed out")
    record(record_property, f)
