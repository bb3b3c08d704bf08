"""
Whole spiking networks with BatchNorm / LayerNorm / no normalisation, drawn at random (tests/network_cases.py), on the
HIP path against the oracle in float64.  What joins the kernels into a layer is Python host code full of
value-changing branches — odd widths (BatchNorm's sums from their own kernel, the padded recurrent path), two
directions, a bias, eval mode, ragged batches, placeholders between the layers, the three descriptions of an input —
and only a whole network runs them.

Every case was kept by a rule that looks at the oracle alone (network_cases.verdict): its spike trains are decided (the
fp32 and the fp64 run agree and the smallest |u - theta| is 8 x their largest difference), every layer fires at a rate
in [0.02, 0.7], no gradient is identically zero and every fp32 gradient is within 1e-4 of the fp64 one.  So:

  spikes     every hidden layer's train, after dropout, equals the fp64 oracle's element for element;
  rates      to 1e-6 of the largest;
  out, loss, every parameter gradient   within 4 x max(|fp32 oracle - fp64 oracle| of the case, r_role x max-abs), r_role
             the worst relative fp32 error of that parameter role over all kept cases; every bound is asserted (in
             network_cases.bounds) to lie under the project's whole-network bars, 5e-4 / 1e-4 / 1e-5;
  W.bias under train-mode BatchNorm   is zero in real arithmetic and rounding residue on both sides.  An absolute bound
             from the oracle's column sums of |dx| is not robust (dx is itself a difference of three terms, so its error
             is not relative to it); as in the baselines' fuzz the entry is left out of the relative comparison and held
             finite and below 1e-3 of that layer's norm.bias gradient;
  exact      V.weight's gradient has a zero diagonal; with lengths the input gradient is 0 on the padding; train-mode
             BatchNorm's running statistics to rtol 1e-4 / atol 1e-6 and its counter advanced by one.
"""
import numpy as np
import pytest
import torch

from tests import network_cases as nc
from tests import ragged_oracle as rag
from tests.kit import N, bf16_mode, record, relmax, within  # noqa: F401  (bf16_mode: a fixture)
from tests.kit import sp  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

CASES = list(nc.KEPT) + [nc.PLANES]
EVAL_CASES = [i for i in nc.KEPT if not nc.draw(i)["training"]]


def ids(cases):
    return [nc.label(nc.draw(i)) for i in cases]


def check_spikes(d, r64, what=""):
    assert sorted(d["spikes"]) == list(range(len(r64["spikes"])))
    for k, want in enumerate(r64["spikes"]):
        got, want = N(d["spikes"][k]), want.float().numpy()
        assert got.shape == want.shape
        if not np.array_equal(got, want):
            at = tuple(int(v) for v in np.argwhere(got != want)[0])
            raise AssertionError(f"{what}layer {k}: {int((got != want).sum())} of {want.size} spikes differ from the "
                                 f"oracle's, the first at (b, t, h) = {at}: {got[at]} against {want[at]}")


def check_residue_and_exact(c, d, r64):
    """What is exact, and W.bias under train-mode BatchNorm."""
    cfg, net = c["cfg"], d["net"]
    for k, v in net.named_parameters():
        g = N(v.grad)
        assert np.isfinite(g).all(), k
        if k.endswith("V.weight"):
            assert not np.diag(g).any() and np.abs(g).max() > 0, k
        if nc.residue(cfg, k):
            top = nc.maxabs(r64["grads"][k[:-len("W.bias")] + "norm.bias"])
            assert np.abs(g).max() <= 1e-3 * top, (k, float(np.abs(g).max()), top)
    if cfg["lengths"] is not None and d["x"].requires_grad:
        g = N(d["x"].grad)
        m = rag.valid_mask(cfg["lengths"], cfg["T"]).numpy()[:, :, None]
        assert np.isfinite(g).all() and not (g * ~m).any() and np.abs(g).max() > 0


@pytest.mark.parametrize("i", CASES, ids=ids(CASES))
def test_network_vs_oracle(sp, i, record_property):
    c = nc.case(i)
    cfg = c["cfg"]
    d = nc.device_run(sp, c)
    r64, _ = nc.runs(i)
    if i == nc.PLANES:      # the case is there for this branch
        from sparch_amd import functional as Fn
        assert Fn.USE_DX_PLANES in (True, "auto") and Fn.DENSE_GEMM == "split6" and Fn.compute_dtype() == "fp32"
    check_spikes(d, r64)
    assert relmax(N(d["rates"]), r64["rates"].numpy()) <= 1e-6
    bound = nc.bounds(i)
    got = dict(out=N(d["out"]), loss=N(d["loss"]), **{k: N(v.grad) for k, v in d["net"].named_parameters()})
    assert set(got) == set(nc.compared(r64))
    ref = nc.compared(r64)
    worst = {}
    for k in sorted(bound):
        f = within(got[k], ref[k].numpy(), bound[k], k)
        worst[nc.role_of(k)] = max(worst.get(nc.role_of(k), 0.0), f)
    check_residue_and_exact(c, d, r64)
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


BF16_CASES = nc.bf16_cases()


@pytest.mark.parametrize("i", BF16_CASES, ids=ids(BF16_CASES))
def test_network_vs_oracle_bf16_operands(sp, i, bf16_mode):
    """The bf16 operand mode on the cases whose operands are bf16-exact (grid weights, a 0/1 or count input, the
    box-car): the spike trains still equal the oracle's; gradients to the mode's 2e-2 of max-abs, the neuron parameters
    to five times that, as test_snn_random_configurations_vs_oracle holds them."""
    c = nc.case(i)
    d = nc.device_run(sp, c)
    r64, _ = nc.runs(i)
    check_spikes(d, r64)
    assert relmax(N(d["rates"]), r64["rates"].numpy()) <= 1e-6
    for k, v in d["net"].named_parameters():
        if nc.residue(c["cfg"], k):
            continue
        e = relmax(N(v.grad), r64["grads"][k].numpy())
        assert e <= 2e-2 * (5.0 if k.split(".")[-1] in ("alpha", "beta", "a", "b") else 1.0), (k, e)
    check_residue_and_exact(c, d, r64)


@pytest.mark.parametrize("i", EVAL_CASES, ids=ids(EVAL_CASES))
def test_eval_forward_is_the_no_save_forward(sp, i):
    """Eval mode: the forward under torch.no_grad() — the kernels' no-save and placeholder instantiations — gives the
    bits of the forward that saves for a backward."""
    c = nc.case(i)
    a = nc.device_run(sp, c, backward=False)
    b = nc.device_run(sp, c, grad=False)
    assert a["out"].requires_grad and not b["out"].requires_grad
    assert torch.equal(a["out"].detach(), b["out"]) and torch.equal(a["rates"].detach(), b["rates"])
    for k in a["spikes"]:
        assert torch.equal(a["spikes"][k], b["spikes"][k]), k
