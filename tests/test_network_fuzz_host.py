"""
The whole-network fuzz of tests/network_cases.py on the CPU: the list of kept cases is what the keep rule gives and obeys
its caps; the oracle run with the recording, dtype-keeping spike is the oracle; and the bound the GPU test applies
(network_cases.bounds, from the oracle alone) resolves eight wrong networks — each an edit of the oracle's torch
expressions made here — by a factor of at least 100 on at least three kept cases that have the feature.
"""
import collections

import pytest
import torch
import torch.nn.functional as F

from oracle import snn_oracle as orc
from tests import network_cases as nc
from tests import ragged_oracle as rag


# ------------------------------------------------------------------------------------------------ the list and its caps
def test_kept_is_what_the_rule_gives_and_the_caps_hold():
    """The literal is re-derived with a band (network_cases.verdict says why): every draw up to the last kept one that
    passes the rule tightened by 2 must be in KEPT, none that fails the rule relaxed by 2 may be.  The caps are the
    literal's."""
    kept, draws = list(nc.KEPT), nc.KEPT[-1] + 1
    assert len(kept) == nc.N_KEPT == len(set(kept)) and kept == sorted(kept)
    verdicts = {i: nc.verdict(i) for i in range(draws)}
    same = [i for i in verdicts if verdicts[i][0]] == kept
    print(f"  the rule as it stands gives {'KEPT' if same else 'another list'} here")
    for i in range(draws):
        if nc.verdict(i, 2.0)[0]:
            assert i in kept, (i, "passes the tightened rule")
        if not nc.verdict(i, 0.5)[0]:
            assert i not in kept, (i, nc.verdict(i, 0.5)[1])
    rejected = {i: verdicts[i][1] for i in range(draws) if i not in kept}
    print(f"  {len(rejected)} of {draws} draws rejected")
    for i, why in rejected.items():
        print(f"    {nc.label(nc.draw(i))}: {why}")
    assert 4 * len(rejected) <= draws
    tally = collections.Counter(v for i in kept for v in nc.axis_values(nc.draw(i)))
    print("  " + ", ".join(f"{k} {tally[k]}" for k in sorted(tally)))
    expected = {f"kind={k}" for k in nc.KINDS} | {f"norm={k}" for k in nc.NORMS} | {f"input={k}" for k in nc.INPUTS}
    expected |= {f"{a}={v}" for a in ("bias", "readout", "train", "real_weights", "regulariser", "lengths", "smooth")
                 for v in (True, False)}
    expected |= {"dirs=1", "dirs=2", "threshold=1.0", "threshold=0.75", "dropout=0.0", f"dropout={nc.P_DROP}"}
    assert set(tally) == expected
    assert min(tally.values()) >= 6, tally
    for name, values in (("B", nc.BATCHES), ("T", nc.STEPS), ("C", nc.CHANNELS)):
        assert {nc.draw(i)[name] for i in kept} == set(values)
    assert {h for i in kept for h in nc.draw(i)["sizes"]} >= set(nc.WIDTHS) | set(nc.CLASSES)
    print("  the planes case:", nc.verdict(nc.PLANES), nc.verdict(nc.PLANES, 4.0))
    assert nc.verdict(nc.PLANES, 0.5)[0], nc.verdict(nc.PLANES, 0.5)
    assert len(nc.bf16_cases()) == 16 and len([i for i in kept if not nc.draw(i)["training"]]) >= 6
    for i in list(kept) + [nc.PLANES]:          # every bound lies under the project's bars (asserted inside)
        nc.bounds(i)
    print("  r_role: " + ", ".join(f"{k} {v:.2e}" for k, v in nc.role_errors().items()))


def test_draw_is_a_pure_function_of_the_index():
    for i in (0, 5, 63, nc.PLANES):
        assert nc.draw(i) == nc.draw(i)
    assert nc.draw(3) != nc.draw(4)
    eligible = [i for i in range(200) if not nc.draw(i)["bidirectional"] and nc.draw(i)["use_readout_layer"]
                and not (nc.draw(i)["normalization"] == "batchnorm" and nc.draw(i)["use_bias"])]
    ragged = [i for i in range(200) if nc.draw(i)["lengths"] is not None]
    assert set(ragged) <= set(eligible)
    for i in ragged:
        cfg = nc.draw(i)
        assert len(cfg["lengths"]) == cfg["B"] and {1, cfg["T"]} <= set(cfg["lengths"])
        x = nc.case(i)["x"] if i in nc.KEPT else None
        if x is not None:
            assert not (x * ~rag.valid_mask(cfg["lengths"], cfg["T"])[:, :, None]).any()


# ------------------------------------------------------------------------------------------------ the oracle is the oracle
def plain_cases():
    """Three kept cases with the box-car and no lengths, one per normalisation."""
    found = {}
    for i in nc.KEPT:
        cfg = nc.draw(i)
        if cfg["surrogate"] is None and cfg["lengths"] is None:
            found.setdefault(cfg["normalization"], i)
    assert len(found) == 3
    return sorted(found.values())


@pytest.mark.parametrize("i", plain_cases())
def test_the_recording_spike_changes_nothing_in_fp32(i):
    """oracle_run in fp32 against the oracle as it stands (its own spike, nothing replaced): out, rates, spike trains,
    loss, every gradient and the running statistics bit for bit."""
    c = nc.case(i)
    cfg = c["cfg"]
    got = nc.oracle_run(c, torch.float32)
    p = {k: v.clone().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in c["params"].items()
         if "num_batches" not in k}
    spikes, stats = [], {}
    out, rates = orc.snn_forward(c["x"], p, neuron_type=cfg["kind"], num_layers=len(cfg["sizes"]), init_states=c["init"],
                                 normalization=cfg["normalization"], bidirectional=cfg["bidirectional"],
                                 use_readout_layer=cfg["use_readout_layer"], training=cfg["training"],
                                 theta=cfg["threshold"], stats=stats, drop_masks=c["masks"], spikes_out=spikes)
    loss = nc.loss_of(cfg, out, rates, c["y"], c["gout"])
    loss.backward()
    assert torch.equal(got["out"], out.detach()) and torch.equal(got["rates"], rates.detach())
    assert torch.equal(got["loss"], loss.detach())
    assert all(torch.equal(a, b.detach()) for a, b in zip(got["spikes"], spikes)) and len(spikes) == len(got["spikes"])
    assert set(got["grads"]) == {k for k, v in p.items() if v.requires_grad}
    for k, v in got["grads"].items():
        assert torch.equal(v, p[k].grad), k
    assert set(got["stats"]) == set(stats) and all(torch.equal(got["stats"][k], stats[k]) for k in stats)
    # and the recorded differences are the spikes' own
    for d, s in zip(got["diffs"], got["spikes"]):
        rows = d.shape[0]
        fired = (d > 0).float()
        if cfg["bidirectional"]:
            fired = torch.cat([fired[:rows // 2], fired[rows // 2:].flip(1)], dim=2)
        assert torch.equal(fired, (s != 0).float()) or c["masks"] is not None


def test_the_ragged_oracle_with_full_lengths_is_the_plain_one():
    i = next(i for i in nc.KEPT if nc.draw(i)["lengths"] is None and not nc.draw(i)["bidirectional"]
             and nc.draw(i)["use_readout_layer"] and nc.draw(i)["normalization"] == "batchnorm"
             and nc.draw(i)["training"])
    c = nc.case(i)
    cfg = c["cfg"]
    plain = nc.oracle_run(c, torch.float64)
    full = nc.oracle_run(dict(c, cfg=dict(cfg, lengths=[cfg["T"]] * cfg["B"])), torch.float64)
    assert all(torch.equal(a, b) for a, b in zip(plain["spikes"], full["spikes"]))
    for k, a in nc.compared(plain).items():
        b = nc.compared(full)[k]
        assert nc.maxabs(a - b) <= 1e-12 * nc.maxabs(a), k
    assert nc.maxabs(plain["rates"] - full["rates"]) <= 1e-15
    for k, v in plain["stats"].items():
        assert nc.maxabs(v - full["stats"][k]) <= 1e-12, k


# ------------------------------------------------------------------------------------------------ what the bound resolves
class _Functional:
    """torch.nn.functional with some functions replaced: what oracle.snn_oracle and tests.ragged_oracle see as F."""

    def __init__(self, **replaced):
        self.__dict__.update(replaced)

    def __getattr__(self, name):
        return getattr(F, name)


def _bn_with_running_statistics(x, rm, rv, w, b, training, momentum, eps):
    return F.batch_norm(x, rm, rv, w, b, False, momentum, eps)


def _bn_biased_running_var(x, rm, rv, w, b, training, momentum, eps):
    y = F.batch_norm(x, rm, rv.clone(), w, b, training, momentum, eps)
    if training:
        rv.copy_((1 - momentum) * rv + momentum * x.detach().var(0, unbiased=False))
    return y


class _EvalCoupled(torch.autograd.Function):
    """Eval-mode BatchNorm whose backward keeps train mode's two batch-coupling terms."""

    @staticmethod
    def forward(ctx, x, rm, rv, w, b, eps):
        invstd = 1.0 / torch.sqrt(rv + eps)
        xhat = (x - rm) * invstd
        ctx.save_for_backward(xhat, invstd, w)
        return xhat * w + b

    @staticmethod
    def backward(ctx, g):
        xhat, invstd, w = ctx.saved_tensors
        dxhat = g * w
        dx = invstd * (dxhat - dxhat.mean(0) - xhat * (dxhat * xhat).mean(0))
        return dx, None, None, (g * xhat).sum(0), g.sum(0), None


def _bn_eval_coupled(x, rm, rv, w, b, training, momentum, eps):
    return F.batch_norm(x, rm, rv, w, b, training, momentum, eps) if training else _EvalCoupled.apply(x, rm, rv, w, b, eps)


def _second_direction_dropped(kind, Wx, p, u0, w0, s0, theta=1.0, cell=orc.spiking_cell):
    half = Wx.shape[0] // 2
    return cell(kind, torch.cat([Wx[:half], Wx[half:].detach()], dim=0), p, u0, w0, s0, theta)


class _BiasFromDy:
    """W.bias receives the column sum of the normalised projection's gradient instead of the raw projection's."""

    def __init__(self):
        self.bias = None

    def linear(self, x, W, b=None):
        self.bias = b
        return F.linear(x, W, None if b is None else b.detach())

    def layer_norm(self, x, shape, w, b, eps):
        y = F.layer_norm(x, shape, w, b, eps)
        return y if self.bias is None else y + (self.bias - self.bias.detach())


def _ln_over_the_padded_width(x, shape, w, b, eps):
    H = shape[0]
    Hp = (H + 3) // 4 * 4
    return F.layer_norm(F.pad(x, (0, Hp - H)), (Hp,), None, None, eps)[:, :H] * w + b


def _patches(name):
    """(replacements of F's functions, replacement of orc.spiking_cell or None) of a wrong network."""
    if name == "train BatchNorm normalises with the running statistics":
        return dict(batch_norm=_bn_with_running_statistics), None
    if name == "running_var updated with the biased variance":
        return dict(batch_norm=_bn_biased_running_var), None
    if name == "eval BatchNorm backward keeps the batch-coupling terms":
        return dict(batch_norm=_bn_eval_coupled), None
    if name == "second direction's gradient not added into the projection":
        return {}, _second_direction_dropped
    if name == "W.bias under LayerNorm from the column sum of dy":
        m = _BiasFromDy()
        return dict(linear=m.linear, layer_norm=m.layer_norm), None
    if name == "LayerNorm over the width rounded up to a multiple of 4":
        return dict(layer_norm=_ln_over_the_padded_width), None
    raise KeyError(name)


def _rate_term_over_all_steps(cfg):
    """The gradient through the rates scaled by 1 / (B T) where 1 / N is meant; the values stay."""
    k = sum(cfg["lengths"]) / float(cfg["B"] * cfg["T"])
    return lambda rates: rates.detach() + (rates - rates.detach()) * k


WRONG = {
    "train BatchNorm normalises with the running statistics":
        lambda cfg: cfg["normalization"] == "batchnorm" and cfg["training"],
    "running_var updated with the biased variance":
        lambda cfg: cfg["normalization"] == "batchnorm" and cfg["training"],
    "eval BatchNorm backward keeps the batch-coupling terms":
        lambda cfg: cfg["normalization"] == "batchnorm" and not cfg["training"],
    "second direction's gradient not added into the projection": lambda cfg: cfg["bidirectional"],
    "rate term scaled by 1 / (B T) where N is meant":
        lambda cfg: cfg["lengths"] is not None and cfg["regulariser"] and sum(cfg["lengths"]) < cfg["B"] * cfg["T"],
    "W.bias under LayerNorm from the column sum of dy":
        lambda cfg: cfg["normalization"] == "layernorm" and cfg["use_bias"],
    "LayerNorm over the width rounded up to a multiple of 4":
        lambda cfg: cfg["normalization"] == "layernorm" and any(h % 4 for h in cfg["sizes"]),
    "dropout's 1 / (1 - p) missing from the rates": lambda cfg: cfg["dropout"] > 0,
}


def factor_outside(i, wrong):
    """By how much the wrong run leaves the GPU test's acceptance: the largest error over its bound among out, loss and
    the gradients (network_cases.bounds), the rates (1e-6 of the largest) and the running statistics (rtol 1e-4 / atol
    1e-6); infinite if a spike differs."""
    ref = nc.runs(i)[0]
    if any(not torch.equal(a, b) for a, b in zip(ref["spikes"], wrong["spikes"])):
        return float("inf")
    bound = nc.bounds(i)
    a, b = nc.compared(ref), nc.compared(wrong)
    worst = max(nc.maxabs(b[k] - a[k]) / bound[k] for k in bound)
    worst = max(worst, nc.maxabs(wrong["rates"] - ref["rates"]) / (1e-6 * nc.maxabs(ref["rates"])))
    if nc.case(i)["cfg"]["training"]:
        for k, v in ref["stats"].items():
            worst = max(worst, float(((wrong["stats"][k] - v).abs() / (1e-6 + 1e-4 * v.abs())).max()))
    return worst


@pytest.mark.parametrize("name", list(WRONG))
def test_the_bound_resolves_a_wrong_network(name, monkeypatch, record_property):
    cases = [i for i in nc.KEPT if WRONG[name](nc.draw(i))]
    assert len(cases) >= 3, cases
    factors = {}
    for i in cases:
        c = nc.case(i)
        cfg = c["cfg"]
        with monkeypatch.context() as mp:
            edit = None
            if name.startswith("rate term"):
                edit = _rate_term_over_all_steps(cfg)
            elif name.startswith("dropout's"):
                edit = lambda rates, keep=1.0 - cfg["dropout"]: rates * keep  # noqa: E731
            else:
                fns, cell = _patches(name)
                if fns:
                    mp.setattr(orc, "F", _Functional(**fns))
                    mp.setattr(rag, "F", _Functional(**fns))
                if cell is not None:
                    mp.setattr(orc, "spiking_cell", cell)
            wrong = nc.oracle_run(c, torch.float64, rates_edit=edit)
        factors[i] = factor_outside(i, wrong)
    resolved = sorted(f for f in factors.values() if f >= 100.0)
    print(f"  {name}: {len(resolved)} of {len(cases)} cases with the feature resolved at a factor >= 100; "
          f"smallest factor over all of them {min(factors.values()):.3g}, over the resolved ones "
          f"{resolved[0] if resolved else float('nan'):.3g}")
    record_property("smallest_factor", min(factors.values()))
    assert len(resolved) >= 3, factors


def test_the_unedited_run_is_inside_every_bound():
    """The yardstick of the test above at zero: the fp32 oracle against the fp64 one stays inside it."""
    for i in nc.KEPT[:16]:
        assert factor_outside(i, dict(nc.runs(i)[1], out=nc.runs(i)[1]["out"].double(),
                                      loss=nc.runs(i)[1]["loss"].double(),
                                      rates=nc.runs(i)[1]["rates"].double(),
                                      spikes=[s.double() for s in nc.runs(i)[1]["spikes"]],
                                      grads={k: v.double() for k, v in nc.runs(i)[1]["grads"].items()},
                                      stats={k: v.double() for k, v in nc.runs(i)[1]["stats"].items()})) <= 1.0
