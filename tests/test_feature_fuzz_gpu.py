"""
Whole spiking networks over the feature matrix — layout (dense, `lengths`, `pack=True`) x axonal delays x synaptic
currents x readout mode / per-step readout, on top of kind, normalisation, directions, dropout and surrogate — drawn by
tests/feature_cases.py, through the public SNN.forward on the HIP path against ONE composed oracle in float64
(tests/feature_oracle.py).  Each feature's own file checks it alone, mostly against the package itself (a delayed layer
against the layer on a shifted input, pack against lengths, a row against its clip); here two and more are on together
against a reference that shares no code with the package, so an error in a joint of the layer host code
(functional.SeqLayout, snns._layout_cfg: the placeholder and bf16 plane through DelayFn into a projection, the filter
between the normalisation and the cell on a doubled batch, BatchNorm's sums inside the synapse backward, lengths2 /
pack2, the rate gradient under dropout) fails a case.

Every case was kept by tests/network_cases.py's rule on the oracle alone (feature_cases.verdict), and every pair of
feature values that is not refused occurs in a kept case (tests/test_feature_fuzz_host.py).  So:

  spikes     every hidden layer's train, after dropout, equals the fp64 oracle's element for element, zero on padding;
  rates      to 1e-6 of the largest;
  out, seq, loss, every parameter gradient (delay and gamma among them)   within 4 x max(|fp32 oracle - fp64 oracle| of
             the case, r_role x max-abs); every bound asserted under the project's bars 5e-4 / 1e-4 / 1e-5 (seq: out's);
  W.bias under train-mode BatchNorm   as tests/test_network_fuzz_gpu.py treats it: out of the relative comparison, finite
             and below 1e-3 of that layer's norm.bias gradient;
  exact      V.weight's gradient has a zero diagonal; the input gradient is 0 on padding; delay's gradient is exactly 0
             where its clamp is active and absent with learn_delays=False; gamma's is exactly 0 where it is clamped and
             absent with learn_synapse=False; running statistics to rtol 1e-4 / atol 1e-6, the counter advanced by one.
"""
import numpy as np
import pytest
import torch

from tests import feature_cases as fc
from tests import ragged_oracle as rag
from tests.kit import N, bf16_mode, record, relmax, within  # noqa: F401  (bf16_mode: a fixture)
from tests.kit import sp  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

CASES = list(fc.KEPT) + [fc.WIDE, fc.DX_PLANES]
BF16_CASES = fc.bf16_cases()
BOTH_LAYOUTS = [i for i in fc.KEPT if fc.other_layout(fc.draw(i)) is not None]


def ids(cases):
    return [fc.label(fc.draw(i)) for i in cases]


def check_spikes(cfg, d, r64):
    assert sorted(d["spikes"]) == list(range(len(r64["spikes"])))
    for k, want in enumerate(r64["spikes"]):
        got, want = N(d["spikes"][k]), want.float().numpy()
        assert got.shape == want.shape
        if not np.array_equal(got, want):
            at = tuple(int(v) for v in np.argwhere(got != want)[0])
            raise AssertionError(f"layer {k}: {int((got != want).sum())} of {want.size} spikes differ from the "
                                 f"oracle's, the first at (b, t, h) = {at}: {got[at]} against {want[at]}")
        if cfg["lengths"] is not None:
            assert not (got * ~rag.valid_mask(cfg["lengths"], cfg["T"]).numpy()[:, :, None]).any(), k


def device_grads(cfg, d):
    """{key: gradient} of the parameters that learn; the fixed ones (learn_delays / learn_synapse False) have none."""
    got = {}
    for k, v in d["net"].named_parameters():
        if fc.learnable(cfg, k):
            assert v.grad is not None, k
            got[k] = N(v.grad)
        else:
            assert not v.requires_grad and v.grad is None, k
    return got


def check_residue_and_exact(c, cfg, d, r64, grads):
    """What is exact, and W.bias under train-mode BatchNorm."""
    for k, g in grads.items():
        assert np.isfinite(g).all(), k
        if k.endswith("V.weight"):
            assert not np.diag(g).any() and np.abs(g).max() > 0, k
        if fc.residue(cfg, k):
            top = fc.maxabs(r64["grads"][k[:-len("W.bias")] + "norm.bias"])
            assert np.abs(g).max() <= 1e-3 * top, (k, float(np.abs(g).max()), top)
        if k.endswith("delay"):
            raw = c["params"][k].numpy()
            outside = (raw < 0) | (raw > cfg["max_delay"])
            assert outside.any() and not g[outside].any(), k
        if k.endswith("gamma"):
            raw = c["params"][k].numpy()
            outside = (raw < np.float32(fc.SYN_LIMITS[0])) | (raw > np.float32(fc.SYN_LIMITS[1]))
            assert outside.any() and not g[outside].any(), k
    if cfg["lengths"] is not None and d["x"].requires_grad:
        g = N(d["x"].grad)
        m = rag.valid_mask(cfg["lengths"], cfg["T"]).numpy()[:, :, None]
        assert np.isfinite(g).all() and not (g * ~m).any() and np.abs(g).max() > 0


def watched_run(sp, c, monkeypatch, decisions):
    """device_run with functional._use_dx_planes recording what it is asked and what it answers."""
    from sparch_amd import functional as Fn
    real = Fn._use_dx_planes

    def watched(inp, norm, dirs, M, K, H):
        took = real(inp, norm, dirs, M, K, H)
        decisions.append(((norm, M, K, H, inp.x16 is not None), bool(took)))
        return took

    monkeypatch.setattr(Fn, "_use_dx_planes", watched)
    return fc.device_run(sp, c)


def compare(i, d, record_property):
    """The whole comparison of one fp32 run of case i with the fp64 oracle (module docstring)."""
    c = fc.case(i)
    cfg = c["cfg"]
    r64, _ = fc.runs(i)
    check_spikes(cfg, d, r64)
    assert relmax(N(d["rates"]), r64["rates"].numpy()) <= 1e-6
    bound = fc.bounds(i)
    grads = device_grads(cfg, d)
    got = dict(out=N(d["out"]), loss=N(d["loss"]), **grads)
    if cfg["per_step"]:
        got["seq"] = N(d["seq"])
    ref = fc.compared(r64)
    assert set(got) == set(ref), sorted(set(got) ^ set(ref))
    worst = {}
    for k in sorted(bound):
        f = within(got[k], ref[k].numpy(), bound[k], k)
        worst[fc.role_of(k)] = max(worst.get(fc.role_of(k), 0.0), f)
    check_residue_and_exact(c, cfg, d, r64, grads)
    if cfg["normalization"] == "batchnorm" and cfg["training"]:
        state = d["net"].state_dict()
        assert r64["stats"]
        for k, v in r64["stats"].items():
            np.testing.assert_allclose(N(state[k]), v.numpy(), rtol=1e-4, atol=1e-6, err_msg=k)
            tracked = k.rsplit(".", 1)[0] + ".num_batches_tracked"
            assert int(state[tracked]) == int(c["params"][tracked]) + 1, tracked
    print("  worst fraction of the bound per role: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))
    for k, v in worst.items():
        record_property("fraction_" + k, round(v, 3))
    record(record_property, *worst.values())


DX_SHAPE = ("batchnorm", 256, 256, 256, True)       # the second layer of the DX_PLANES case: whole tiles, a spike plane


@pytest.mark.parametrize("i", CASES, ids=ids(CASES))
def test_features_vs_oracle(sp, i, record_property, monkeypatch):
    decisions = []
    d = watched_run(sp, fc.case(i), monkeypatch, decisions)
    if i == fc.DX_PLANES:
        # The delayed, spike-fed, bidirectional layer under lengths reaches functional._use_dx_planes with shapes the
        # plane kernels take.  On the doubled-batch route the projection's backward runs as one direction, so the
        # default ("auto": two directions only) answers no here; the test below switches the planes on.
        from sparch_amd import functional as Fn
        assert Fn.DENSE_GEMM == "split6" and Fn.compute_dtype() == "fp32"
        assert [took for shape, took in decisions if shape == DX_SHAPE] == [Fn.USE_DX_PLANES is True], decisions
    compare(i, d, record_property)


def test_dx_planes_under_lengths_with_delays_and_two_directions(sp, record_property, monkeypatch):
    """The DX_PLANES case with functional.USE_DX_PLANES on (SPARCH_DX_PLANES=1): BatchNorm's backward writes dx as bf16
    planes with the column sums scaled for the valid rows, and the dW and dX products of the spike-fed layer read them —
    behind a delay gather, on a ragged bidirectional batch.  Held to the same oracle and bounds."""
    from sparch_amd import functional as Fn
    monkeypatch.setattr(Fn, "USE_DX_PLANES", True)
    decisions = []
    d = watched_run(sp, fc.case(fc.DX_PLANES), monkeypatch, decisions)
    assert (DX_SHAPE, True) in decisions, decisions
    compare(fc.DX_PLANES, d, record_property)


@pytest.mark.parametrize("i", BF16_CASES, ids=ids(BF16_CASES))
def test_features_vs_oracle_bf16_operands(sp, i, bf16_mode):
    """The bf16 operand mode on the kept cases whose operands are bf16-exact (grid weights, a 0/1 or count input, the
    box-car): the spike trains still equal the oracle's; gradients to the mode's 2e-2 of max-abs, the neuron parameters
    (gamma among them) to five times that, as tests/test_network_fuzz_gpu.py holds them."""
    c = fc.case(i)
    cfg = c["cfg"]
    d = fc.device_run(sp, c)
    r64, _ = fc.runs(i)
    check_spikes(cfg, d, r64)
    assert relmax(N(d["rates"]), r64["rates"].numpy()) <= 1e-6
    grads = device_grads(cfg, d)
    for k, g in grads.items():
        if fc.residue(cfg, k):
            continue
        e = relmax(g, r64["grads"][k].numpy())
        assert e <= 2e-2 * (5.0 if k.split(".")[-1] in ("alpha", "beta", "a", "b", "gamma") else 1.0), (k, e)
    check_residue_and_exact(c, cfg, d, r64, grads)


@pytest.mark.parametrize("i", BOTH_LAYOUTS, ids=ids(BOTH_LAYOUTS))
def test_masked_and_packed_give_equal_bits_in_eval_mode(sp, i):
    """Every kept ragged case that both layouts accept, in eval mode: `lengths` and `pack=True` give the same bits for
    out, rates and every hidden layer's spikes — with delays, synapses, two directions and every readout mode, where
    tests/test_packed_gpu.py holds it for networks with none of them."""
    c = fc.case(i)
    a = fc.device_run(sp, c, grad=False, training=False, dropout=0.0, layout="lengths")
    b = fc.device_run(sp, c, grad=False, training=False, dropout=0.0, layout="pack")
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["rates"], b["rates"])
    assert sorted(a["spikes"]) == sorted(b["spikes"])
    for k in a["spikes"]:
        assert torch.equal(a["spikes"][k].cpu(), b["spikes"][k].cpu()), k
