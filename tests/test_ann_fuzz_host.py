"""
The whole-network fuzz of the non-spiking baselines (tests/ann_cases.py) on the CPU, with no package involved:

  the oracle   tests/ann_net_oracle.py gives the bits of oracle/ann_oracle.py in fp32 without masks, reproduces the six
               reference fixtures tests/golden/ann_*.npz at the bars of tests/test_oracle_golden.py, is unchanged by
               masks of ones, and its bidirectional rows are the clip and its flip through one-direction layers;
  the list     KEPT is what the keep rule gives (re-derived with the slack band of network_cases.verdict), at least 0.85
               of the indices tried are kept, every kind keeps at least 12, every required pair of axis values is covered
               or refused with a reason, and every bound lies under the project's whole-network bars;
  the bound    six wrong networks, each an edit of the oracle's expressions made here, leave the acceptance of
               tests/test_ann_fuzz_gpu.py on at least one kept case.
"""
import collections
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ann_oracle as ao
from tests import ann_cases as ac
from tests import ann_net_oracle as ano
from tests import network_cases as nc
from tests.golden_io import load

ALL = list(ac.KEPT) + list(ac.FIXED)


# ------------------------------------------------------------------------------------------------ the oracle is the oracle
def fp32_parameters(c):
    return {k: v.clone().requires_grad_("running" not in k) for k, v in c["params"].items() if "num_batches" not in k}


def test_fp32_without_masks_is_the_existing_oracle_bit_for_bit():
    """ann_oracle.ann_forward takes 3-D input and no masks: every kept and fixed case with its masks left out and its
    input flattened, train mode as drawn, running=None."""
    for i in ALL:
        c = ac.case(i)
        cfg = c["cfg"]
        x = c["x"].flatten(2)
        got = ano.ann_forward(ac.oracle_cfg(cfg), fp32_parameters(c), c["x"], training=cfg["training"], running=None)
        want = ao.ann_forward(ac.oracle_cfg(cfg), fp32_parameters(c), x, training=cfg["training"], running=None)
        assert got.dtype == torch.float32 and torch.equal(got, want), ac.label(cfg)


FIXTURES = ["ann_MLP_bn", "ann_MLP_ln_bias_noreadout", "ann_RNN_bn", "ann_RNN_bidir", "ann_LiGRU_bn", "ann_GRU_bn"]


@pytest.fixture
def one_thread():
    """The fixtures were written by the reference on one thread, and tests/test_oracle_golden.py compares on one."""
    n = torch.get_num_threads()
    torch.set_num_threads(1)
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("name", FIXTURES)
def test_the_reference_fixtures(name, one_thread):
    """The bars of tests/test_oracle_golden.py test_ann_oracle_matches_reference_fixture."""
    z = load(name)
    cfg = json.loads(str(z["cfg"]))
    p = {k[len("param."):]: torch.tensor(z[k]).requires_grad_(z[k].dtype.kind == "f" and "running" not in k)
         for k in z if k.startswith("param.") and "num_batches" not in k}
    x, y = torch.tensor(z["x"]), torch.tensor(z["y"])
    running = {k: v.detach().clone() for k, v in p.items() if "running" in k}
    out = ano.ann_forward(cfg, p, x, training=True, running=running)
    np.testing.assert_allclose(out.detach().numpy(), z["out"], rtol=2e-5, atol=2e-6)
    loss = F.cross_entropy(out, y) if cfg["use_readout_layer"] else (out * out).mean()
    np.testing.assert_allclose(float(loss.detach()), float(z["loss"]), rtol=1e-5)
    loss.backward()
    seen = 0
    for k in z:
        if k.startswith("grad."):
            np.testing.assert_allclose(p[k[len("grad."):]].grad.numpy(), z[k], rtol=2e-4, atol=2e-6, err_msg=k)
            seen += 1
        if k.startswith("after."):
            np.testing.assert_allclose(running[k[len("after."):]].numpy(), z[k], rtol=1e-5, atol=1e-6, err_msg=k)
    assert seen
    with torch.no_grad():
        out_e = ano.ann_forward(cfg, p, x, training=False, running=running)
    np.testing.assert_allclose(out_e.numpy(), z["out_eval"], rtol=2e-5, atol=2e-6)


def test_masks_of_ones_change_nothing():
    cases = [i for i in ALL if ac.draw(i)["dropout"] > 0]
    assert len(cases) >= 6
    for i in cases:
        c = ac.case(i)
        for dtype in (torch.float32, torch.float64):
            a = ac.oracle_run(c, dtype, masks=None)
            b = ac.oracle_run(c, dtype, masks=[torch.ones_like(m) for m in c["masks"]])
            for k, v in ac.compared(a).items():
                assert torch.equal(v, ac.compared(b)[k]), (ac.label(c["cfg"]), k)
            assert all(torch.equal(v, b["stats"][k]) for k, v in a["stats"].items())


def test_bidirectional_rows_are_the_clip_and_its_flip_through_one_direction_layers():
    """Layer by layer in fp64, on the hidden outputs the oracle recorded: a bidirectional layer's output is
    cat(f(h), flip(f(flip(h)))) with f the same layer run in one direction.  BatchNorm in train mode takes its statistics
    over both directions' rows at once, so those cases are left to the fixture ann_RNN_bidir."""
    cases = [i for i in ALL if ac.draw(i)["bidirectional"]
             and not (ac.draw(i)["normalization"] == "batchnorm" and ac.draw(i)["training"])]
    assert len(cases) >= 6 and {ac.draw(i)["kind"] for i in cases} == {"RNN", "LiGRU", "GRU"}
    for i in cases:
        c = ac.case(i)
        cfg = c["cfg"]
        p = {k: v.double() for k, v in c["params"].items() if v.is_floating_point()}
        running = {k: v for k, v in p.items() if "running" in k} or None
        hidden = ac.runs(i)[0]["hidden"]
        h = c["x"].double().flatten(2)
        for k, want in enumerate(hidden):
            def one(v, k=k):
                return ano.hidden_layer(cfg["kind"], v, p, f"ann.{k}", cfg["normalization"], False, cfg["training"],
                                        running)
            got = torch.cat([one(h), one(h.flip(1)).flip(1)], dim=2)
            assert got.shape == want.shape and ac.maxabs(got - want) <= 1e-12 * ac.maxabs(want), (ac.label(cfg), k)
            h = want if c["masks"] is None else want * c["masks"][k].double()


# ------------------------------------------------------------------------------------------------ the list and its conditions
def test_the_constants_are_the_projects():
    assert (ac.MARGIN, ac.GRAD_RTOL, ac.OUT_RTOL, ac.LOSS_RTOL) == (nc.MARGIN, nc.GRAD_RTOL, nc.OUT_RTOL, nc.LOSS_RTOL)
    assert (ac.GRAD_CAP, ac.OUT_CAP, ac.LOSS_CAP) == (nc.GRAD_CAP, nc.OUT_CAP, nc.LOSS_CAP) == (5e-4, 1e-4, 1e-5)
    assert ac.MARGIN == 8 and ac.N_KEPT == 64


def test_draw_is_a_pure_function_of_the_index():
    for i in (0, 5, 63, ac.FILL_BASE + 17, *ac.FIXED):
        assert ac.draw(i) == ac.draw(i)
    assert ac.draw(3) != ac.draw(7)
    for i in range(200):
        cfg = ac.draw(i)
        assert cfg["kind"] == ac.KINDS[i % 4] and not (cfg["kind"] == "MLP" and cfg["bidirectional"])
        assert cfg["dropout"] == 0.0 or cfg["training"]
        assert ac.refusal(ac.axis_values(cfg).values()) is None
    wide, tile = ac.draw(ac.RNN_WIDE), ac.draw(ac.GRU_TILE)
    assert (wide["kind"], wide["sizes"], wide["B"], wide["T"]) == ("RNN", [1028, 20], 4, 4)
    assert (tile["kind"], tile["sizes"], tile["B"], tile["T"], tile["bidirectional"], tile["dropout"]) == \
        ("GRU", [96, 64, 35], 17, 7, True, 0.25)


def test_kept_is_what_the_rule_gives_and_the_conditions_hold():
    """The literal is re-derived with a band (network_cases.verdict says why): every index tried that passes the rule
    tightened by 2 must be in KEPT, none that fails the rule relaxed by 2 may be."""
    kept, tried = list(ac.KEPT), ac.tried_indices()
    random = [i for i in kept if i < ac.FILL_BASE]
    assert len(random) == ac.N_KEPT and len(kept) == len(set(kept)) and kept == sorted(kept)
    derived = ac.derive_kept()
    print(f"  the rule as it stands gives {'KEPT' if tuple(derived[0]) == ac.KEPT else 'another list'} here")
    for i in tried:
        if ac.verdict(i, 2.0)[0]:
            assert i in kept, (i, "passes the tightened rule")
        if not ac.verdict(i, 0.5)[0]:
            assert i not in kept, (i, ac.verdict(i, 0.5)[1])
    rejected = {i: ac.verdict(i)[1] for i in tried if i not in kept}
    share = len(kept) / len(tried)
    print(f"  {len(kept)} of {len(tried)} indices tried are kept ({share:.3f})")
    for i, why in rejected.items():
        print(f"    {ac.label(ac.draw(i))}: {why}")
    assert share >= 0.85
    kinds = collections.Counter(ac.draw(i)["kind"] for i in kept)
    print("  " + ", ".join(f"{k} {kinds[k]}" for k in ac.KINDS))
    assert all(kinds[k] >= 12 for k in ac.KINDS)
    # coverage: every pair of axis values is in a kept case or refused with a reason
    covered, refused, missing = ac.coverage(kept)
    assert not missing, missing
    assert len(covered) + len(refused) == len(ac.required_pairs()) and not covered & refused
    assert refused == {("kind=MLP", "dirs=2"), ("train=False", f"dropout={ac.P_DROP}")}
    for i in kept:          # a fill case is there for a pair that the cases before it left uncovered, and has it
        if i >= ac.FILL_BASE:
            pair = ac.required_pairs()[(i - ac.FILL_BASE) // ac.FILL_TRIES]
            assert pair in ac.pairs_of(ac.draw(i)) and pair not in ac.coverage([j for j in kept if j < i])[0]
    tally = collections.Counter(v for i in kept for v in ac.axis_values(ac.draw(i)).values())
    print("  " + ", ".join(f"{k} {tally[k]}" for k in sorted(tally)))
    for name, values in (("B", ac.BATCHES), ("T", ac.STEPS), ("C", ac.CHANNELS)):
        assert {ac.draw(i)[name] for i in kept} == set(values)
    assert {h for i in kept for h in ac.hidden_sizes(ac.draw(i))} == set(ac.WIDTHS)
    assert {ac.draw(i)["sizes"][-1] for i in kept if ac.draw(i)["use_readout_layer"]} == set(ac.CLASSES)
    # the two fixed cases are held to the same rule, with the margin of the band
    for i in ac.FIXED:
        assert ac.verdict(i, 2.0)[0], (i, ac.verdict(i, 2.0))
    for i in ALL:           # every bound lies under the project's bars (asserted inside)
        ac.bounds(i)
    print("  r_role: " + ", ".join(f"{k} {v:.2e}" for k, v in ac.role_errors().items()))


def test_the_fp32_oracle_is_inside_every_bound():
    for i in ALL:
        r64, r32 = ac.runs(i)
        wrong = dict(r32, out=r32["out"].double(), loss=r32["loss"].double(),
                     grads={k: v.double() for k, v in r32["grads"].items()},
                     stats={k: v.double() for k, v in r32["stats"].items()})
        assert factor_outside(i, wrong) <= 1.0, ac.label(ac.draw(i))


# ------------------------------------------------------------------------------------------------ what the bound resolves
class _Functional:
    """torch.nn.functional with some functions replaced: what oracle.ann_oracle sees as F."""

    def __init__(self, **replaced):
        self.__dict__.update(replaced)

    def __getattr__(self, name):
        return getattr(F, name)


def _rows_of(mask, cfg):
    """A layer's (B, T, dirs * H) mask in the cell's own layout: (dirs * B, T, H), the second direction in its own time."""
    if not cfg["bidirectional"]:
        return mask
    fwd, bwd = mask.chunk(2, dim=2)
    return torch.cat([fwd, bwd.flip(1)], dim=0)


class _DropUnscaledBackward(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, mask):
        ctx.save_for_backward(mask)
        return y * mask

    @staticmethod
    def backward(ctx, g):
        (mask,) = ctx.saved_tensors
        return g * (mask != 0).to(g.dtype), None


def _bn_biased_running_var(x, rm, rv, w, b, training, momentum, eps):
    if not training or rv is None:
        return F.batch_norm(x, rm, rv, w, b, training, momentum, eps)
    y = F.batch_norm(x, rm, rv.clone(), w, b, training, momentum, eps)
    rv.copy_((1 - momentum) * rv + momentum * x.detach().var(0, unbiased=False))
    return y


def _softmax_with_weighted_padding(x, dim=-1):
    K = x.shape[-1]
    return F.softmax(F.pad(x, (0, -K % 4)), dim=dim)[..., :K]


def wrong_run(name, i, mp):
    """The fp64 oracle run of case i with one edit."""
    c = ac.case(i)
    cfg = c["cfg"]
    masks = None if c["masks"] is None else [m.double() for m in c["masks"]]
    if name == "a mask indexed at the unpadded width":
        return ac.oracle_run(c, torch.float64, masks=ac.drop_masks(cfg, padded=False))
    if name == "a mask applied to the recurrent state":
        mp.setattr(ano, "carry", lambda yt, t, layer: yt * _rows_of(masks[layer], cfg)[:, t])
    elif name == "1 / (1 - p) missing from one layer's backward":
        mp.setattr(ano, "drop", lambda y, m, layer: _DropUnscaledBackward.apply(y, m) if layer == 0 else y * m)
    elif name == "running variance biased instead of unbiased":
        mp.setattr(ao, "F", _Functional(batch_norm=_bn_biased_running_var))
    elif name == "LayerNorm statistics over the padded width":
        left = [ac.n_hidden(cfg) * len(ano.GATES[cfg["kind"]])]     # the hidden layers' calls come first; not the readout's

        def layer_norm(x, shape, w, b, eps):
            left[0] -= 1
            if left[0] < 0:
                return F.layer_norm(x, shape, w, b, eps)
            H = shape[0]
            return F.layer_norm(F.pad(x, (0, -H % 4)), (H + -H % 4,), None, None, eps)[:, :H] * w + b
        mp.setattr(ao, "F", _Functional(layer_norm=layer_norm))
    elif name == "the readout's padded features given weight":
        mp.setattr(ao, "F", _Functional(softmax=_softmax_with_weighted_padding))
    else:
        raise KeyError(name)
    return ac.oracle_run(c, torch.float64)


def _padded(cfg):
    return any(h % 4 for h in ac.hidden_sizes(cfg))


WRONG = {
    "a mask indexed at the unpadded width": lambda cfg: cfg["dropout"] > 0 and _padded(cfg),
    "a mask applied to the recurrent state": lambda cfg: cfg["dropout"] > 0 and cfg["kind"] != "MLP" and cfg["T"] > 1,
    "1 / (1 - p) missing from one layer's backward": lambda cfg: cfg["dropout"] > 0,
    "running variance biased instead of unbiased": lambda cfg: cfg["normalization"] == "batchnorm" and cfg["training"],
    "LayerNorm statistics over the padded width": lambda cfg: cfg["normalization"] == "layernorm" and _padded(cfg),
    "the readout's padded features given weight":
        lambda cfg: cfg["use_readout_layer"] and (cfg["sizes"][-2] * (2 if cfg["bidirectional"] else 1)) % 4 != 0,
}


def factor_outside(i, wrong):
    """By how much a run leaves the GPU test's acceptance: the largest error over its bound among out, loss and the
    gradients (ann_cases.bounds) and, after a training step, the running statistics (rtol 1e-4 / atol 1e-6)."""
    ref = ac.runs(i)[0]
    bound = ac.bounds(i)
    a, b = ac.compared(ref), ac.compared(wrong)
    worst = max(ac.maxabs(b[k] - a[k]) / bound[k] for k in bound)
    if ac.case(i)["cfg"]["training"]:
        for k, v in ref["stats"].items():
            worst = max(worst, float(((wrong["stats"][k] - v).abs() / (1e-6 + 1e-4 * v.abs())).max()))
    return worst


@pytest.mark.parametrize("name", list(WRONG))
def test_the_bound_resolves_a_wrong_network(name, monkeypatch, record_property):
    """Each edit breaks a bound of at least one kept case; the factors of all cases that have the feature are printed."""
    cases = [i for i in ALL if WRONG[name](ac.draw(i))]
    assert len(cases) >= 3, cases
    factors = {}
    for i in cases:
        with monkeypatch.context() as mp:
            factors[i] = factor_outside(i, wrong_run(name, i, mp))
    broken = [i for i, f in factors.items() if f > 1.0]
    print(f"  {name}: {len(broken)} of {len(cases)} cases with the feature leave a bound; factors from "
          f"{min(factors.values()):.3g} to {max(factors.values()):.3g}")
    record_property("smallest_factor", min(factors.values()))
    record_property("largest_factor", max(factors.values()))
    assert broken, factors
    assert ano.carry(1.0, 0, 0) == 1.0 and ao.F is F       # the edits are undone
