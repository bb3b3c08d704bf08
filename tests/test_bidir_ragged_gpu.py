"""
Bidirectional layers on ragged batches on the GPU (SNN(bidirectional=True).forward(x, lengths[, pack=True]); DESIGN.md
section 6, "Bidirectional ragged batches").  Every test here is a ValueError without the feature ("lengths with
bidirectional=True is not supported").

The small recipe of tests/test_ragged_gpu.py: sizes [64, 64, 20], 6 clips of up to 23 steps and 40 features with the
lengths [23, 1, 9, 17, 2, 22] (a full clip, a one-step clip, a crossed tile), dyadic weights, injected initial states on a
2^-4 grid — 12 rows per hidden layer, row 6 + b the reverse direction of clip b.

  the invariant   eval, bit for bit: row b is the clip run alone through the EXISTING bidirectional path.
  all lengths T   eval: out, rates and every hidden layer's spikes are the plain bidirectional forward's bits; after one
                  train step the BatchNorm running statistics agree to rtol 1e-4 / atol 1e-6.
  the oracle      tests/bidir_ragged_oracle.py with the bars of test_whole_network_vs_ragged_oracle, unchanged: per-neuron
                  spike counts equal, out to 1e-4, rates to 1e-6, gradients to 5e-4 of max-abs (2e-2 in the bf16 operand
                  mode), running statistics rtol 1e-4 / atol 1e-6.  tests/bidir_cases.py says how the data seed was picked.
  pack=True       the masked mode's bits in eval mode and its input gradient to 5e-4, as tests/test_packed_gpu.py holds the
                  one-direction packed path to the masked one.
  dropout, per_step, readout, delays, input_from_counts, the command line (SPARCH_LENGTHS=mask): one case each.
"""
import numpy as np
import pytest
import torch

from oracle import snn_oracle as orc
from tests import bidir_ragged_oracle as bro
from tests import packed_numpy as pn
from tests.bidir_cases import KINDS, LENGTHS, NB, NC, NORMS, NT, SIZES, make_net, net_inputs, oracle_step  # noqa: F401
from tests.kit import DEV, SEED, N, bf16_mode, relmax  # noqa: F401  (bf16_mode: a fixture)
from tests.kit import Fn as _Fn
from tests.kit import sp  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu
class injected:
    """`init` handed to the network's draws in the reference's order; b: the rows of clip b run alone (b and NB + b)."""

    def __init__(self, init, b=None):
        init = init if b is None else bro.rows_of(init, b, NB)
        self.order = [st[k] for st in init for k in ("u0", "w0", "s0") if k in st]

    def __enter__(self):
        from sparch_amd import snns as snn_mod
        it = iter(self.order)
        self.mod, self.old = snn_mod, snn_mod._rand_to
        snn_mod._rand_to = lambda rows, cols, device: next(it).to(device)

    def __exit__(self, *exc):
        self.mod._rand_to = self.old


def mask3():
    return torch.from_numpy(pn.valid_mask(LENGTHS, NT))[:, :, None]


# ------------------------------------------------------------------------------------------------ the invariant
@pytest.mark.parametrize("normalization", NORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_a_row_is_its_clip_run_alone_bit_for_bit(sp, kind, normalization):
    """Eval mode, dyadic data: net(x, lengths)[0][b] equals net(x[b:b+1, :L_b])[0] through the existing bidirectional path
    with the state rows b and NB + b; another row's content or length does not change row b's bits."""
    net = make_net(sp, kind, normalization).to(DEV).eval()
    x, _, init = net_inputs(kind)
    with torch.no_grad():
        with injected(init):
            out, rates = net(x.to(DEV), lengths=torch.tensor(LENGTHS))
        for b, n in enumerate(LENGTHS):
            with injected(init, b):
                alone, _ = net(x[b:b + 1, :n].contiguous().to(DEV))
            assert torch.equal(out[b:b + 1], alone), (b, n)
        x2, lens2 = x.clone(), list(LENGTHS)
        x2[0] = (torch.rand(NT, NC) < 0.5).float()            # row 0: other content, row 3: another length
        lens2[3] = 5
        x2 = x2 * torch.from_numpy(pn.valid_mask(lens2, NT))[:, :, None]
        with injected(init):
            out2, _ = net(x2.to(DEV), lengths=torch.tensor(lens2))
    keep = [1, 2, 4, 5]
    assert torch.equal(out2[keep], out[keep])
    assert not torch.equal(out2[0], out[0]) and not torch.equal(out2[3], out[3])
    H = SIZES[0]
    assert all(float(rates[lo:lo + H].sum()) > 0 for lo in range(0, 4 * H, H))      # both directions of both layers fire
    _Fn().check_status()


@pytest.mark.parametrize("normalization", NORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_all_lengths_equal_T_are_the_plain_forward_bits(sp, kind, normalization):
    """Eval, dyadic: out, rates and — layer by layer — the hidden spikes."""
    from sparch_amd import snns
    net = make_net(sp, kind, normalization).to(DEV).eval()
    full = [NT] * NB
    x, _, init = net_inputs(kind, lengths=full)
    with torch.no_grad():
        with injected(init):
            a, ra = net(x.to(DEV))
        with injected(init):
            b, rb = net(x.to(DEV), lengths=torch.tensor(full))
        assert torch.equal(a, b) and torch.equal(ra, rb)
        L = snns.prepare_lengths(full, NB, NT, DEV)
        xa = xb = x.to(DEV)
        for i in range(2):
            st = tuple(None if k not in init[i] else init[i][k].to(DEV) for k in ("u0", "w0", "s0"))
            xa, r1 = net.snn[i].forward_with_rate(xa, states=st)
            xb, r2 = net.snn[i].forward_with_rate(xb, states=st, lengths=L)
            assert tuple(xb.shape) == (NB, NT, 2 * SIZES[i]) and torch.equal(xa, xb) and torch.equal(r1, r2), i
            assert float(xb[..., :SIZES[i]].sum()) > 0 and float(xb[..., SIZES[i]:].sum()) > 0
    _Fn().check_status()


@pytest.mark.parametrize("kind", KINDS)
def test_all_lengths_equal_T_one_train_step_gives_the_plain_running_statistics(sp, kind):
    full = [NT] * NB
    x, y, init = net_inputs(kind, lengths=full)
    got = []
    for kw in ({}, {"lengths": torch.tensor(full)}):
        net = make_net(sp, kind, "batchnorm").to(DEV).train()
        with injected(init):
            out, rates = net(x.to(DEV), **kw)
            orc.train_step_loss(out, rates, y.to(DEV), use_regularizers=True).backward()
        got.append(({k: N(v) for k, v in net.state_dict().items() if "running" in k or "num_batches" in k},
                    {k: N(v.grad) for k, v in net.named_parameters()}, N(out)))
    (sa, ga, oa), (sb, gb, ob) = got
    assert len(sa) == 9
    for k in sa:
        np.testing.assert_allclose(sb[k], sa[k], rtol=1e-4, atol=1e-6, err_msg=k)
    assert relmax(ob, oa) <= 1e-4
    for k in ga:                                 # and the plain path's gradients, at the bar of the oracle comparison
        assert relmax(gb[k], ga[k]) <= 5e-4, k
    _Fn().check_status()


# ------------------------------------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("normalization", NORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_whole_network_vs_bidir_ragged_oracle(sp, kind, normalization, training, compute, request):
    if compute == "bf16":
        request.getfixturevalue("bf16_mode")
    tol_g = 5e-4 if compute == "fp32" else 2e-2
    net = make_net(sp, kind, normalization)
    params = {k: v.clone() for k, v in net.state_dict().items()}
    x, y, init = net_inputs(kind)
    net = net.to(DEV).train(training)
    with injected(init):
        out, rates = net(x.to(DEV), lengths=torch.tensor(LENGTHS))
        loss = orc.train_step_loss(out, rates, y.to(DEV), use_regularizers=True)
        loss.backward()
        _Fn().check_status()
    po, out_o, rates_o, loss_o, stats, _, diffs = oracle_step(kind, normalization, training, params, x, y, init)
    n_valid = sum(LENGTHS)
    counts, counts_o = torch.round(rates.detach().cpu() * n_valid).long(), torch.round(rates_o.detach() * n_valid).long()
    H = SIZES[0]
    assert all(int(counts_o[lo:lo + H].sum()) > 0 for lo in range(0, 4 * H, H))     # both directions of both layers
    print(f"  smallest |u - theta| of the oracle {float(diffs.abs().min()):.3e}")
    assert torch.equal(counts, counts_o), "per-neuron spike counts differ from the oracle"
    eo = relmax(N(out), out_o.detach().numpy())
    print(f"  out {eo:.3e}  loss {float(loss.detach()):.6f} / {float(loss_o.detach()):.6f}")
    assert eo <= 1e-4
    assert abs(float(loss.detach()) - float(loss_o.detach())) <= 1e-5 * max(1.0, abs(float(loss_o.detach())))
    er = relmax(N(rates), rates_o.detach().numpy())
    print(f"  rates {er:.3e}")
    assert er <= 1e-6
    for k, v in net.named_parameters():
        e = relmax(N(v.grad), po[k].grad.numpy())
        print(f"  {k}: {e:.3e}")
        assert e <= tol_g, (k, e)
    for k, v in stats.items():
        np.testing.assert_allclose(N(net.state_dict()[k]), v.numpy(), rtol=1e-4, atol=1e-6, err_msg=k)


def test_the_input_gradient_is_zero_on_the_padding_and_non_zero_inside(sp):
    net = make_net(sp, "adLIF", "batchnorm").to(DEV).train()
    x, y, init = net_inputs("adLIF")
    xd = x.to(DEV).requires_grad_(True)
    with injected(init):
        out, rates = net(xd, lengths=torch.tensor(LENGTHS, device=DEV))    # (lengths on the device work too)
        orc.train_step_loss(out, rates, y.to(DEV), use_regularizers=True).backward()
    g = N(xd.grad)
    m = pn.valid_mask(LENGTHS, NT)
    assert not g[~m].any() and not np.isnan(g).any()
    assert all(np.abs(g[b, :n]).max() > 0 for b, n in enumerate(LENGTHS))
    _Fn().check_status()


# ------------------------------------------------------------------------------------------------ pack=True
@pytest.mark.parametrize("normalization", NORMS)
@pytest.mark.parametrize("kind", KINDS)
def test_pack_gives_the_masked_modes_results(sp, kind, normalization):
    """Eval, dyadic: out and rates are the masked mode's bits (and so every row is its clip run alone)."""
    net = make_net(sp, kind, normalization).to(DEV).eval()
    x, _, init = net_inputs(kind)
    with torch.no_grad():
        with injected(init):
            out, rates = net(x.to(DEV), lengths=torch.tensor(LENGTHS), pack=True)
        with injected(init):
            out_m, rates_m = net(x.to(DEV), lengths=torch.tensor(LENGTHS))
    assert torch.equal(out, out_m) and torch.equal(rates, rates_m)
    assert float(rates.sum()) > 0
    _Fn().check_status()


@pytest.mark.parametrize("kind", ["adLIF", "RadLIF"])
def test_pack_gives_the_masked_modes_gradients(sp, kind):
    """Train mode with BatchNorm: the input gradient is zero on the padding and the masked mode's to 5e-4, and so is every
    parameter gradient."""
    x, y, init = net_inputs(kind)
    res = []
    for kw in (dict(pack=True), dict()):
        net = make_net(sp, kind, "batchnorm").to(DEV).train()
        xd = x.to(DEV).requires_grad_(True)
        with injected(init):
            out, rates = net(xd, lengths=torch.tensor(LENGTHS), **kw)
            orc.train_step_loss(out, rates, y.to(DEV), use_regularizers=True).backward()
        res.append((N(xd.grad), {k: N(v.grad) for k, v in net.named_parameters()}, N(out), N(rates)))
    (g, pg, out, rates), (g_m, pg_m, out_m, rates_m) = res
    m = pn.valid_mask(LENGTHS, NT)
    assert g.shape == tuple(x.shape) and not g[~m].any() and np.abs(g).max() > 0 and not np.isnan(g).any()
    assert relmax(g, g_m) <= 5e-4
    assert relmax(out, out_m) <= 1e-4 and relmax(rates, rates_m) <= 1e-6
    for k in pg:
        assert relmax(pg[k], pg_m[k]) <= 5e-4, k
    _Fn().check_status()


# ------------------------------------------------------------------------------------------------ dropout
@pytest.mark.parametrize("pack", [False, True], ids=["mask", "pack"])
@pytest.mark.parametrize("kind", ["adLIF", "RadLIF"])
def test_dropout_on(sp, kind, pack):
    """Tails are zero, values are in {0, 1 / keep}, and each direction's rate is its column sums over sum(L)."""
    net = make_net(sp, kind, "batchnorm", dropout=0.25, use_readout_layer=False).to(DEV).train()
    for i, lay in enumerate(net.snn):
        lay._dropout_seed = lambda device, i=i: SEED + i
    x, _, _ = net_inputs(kind)
    with torch.no_grad():
        s, rates = net(x.to(DEV), lengths=torch.tensor(LENGTHS), pack=pack)
    H = SIZES[-1]
    assert tuple(s.shape) == (NB, NT, 2 * H)
    m = mask3().to(DEV)
    assert not (s * ~m).any() and float(s[..., :H].sum()) > 0 and float(s[..., H:].sum()) > 0
    assert set(np.unique(N(s)).tolist()) == {0.0, float(np.float32(1.0) / np.float32(0.75))}
    np.testing.assert_allclose(N(rates)[-2 * H:], N(s.sum((0, 1)) / sum(LENGTHS)), rtol=1e-6)
    kept = float((s != 0).float().sum() / max(1.0, float(sum(LENGTHS) * 2 * H)))
    assert kept > 0.01
    _Fn().check_status()


@pytest.mark.parametrize("pack", [False, True], ids=["mask", "pack"])
@pytest.mark.parametrize("kind", ["adLIF", "RadLIF"])
def test_rate_gradient_under_dropout(sp, kind, pack):
    """Backward with dropout on.  rate[c] is the column sum of the layer's output over sum(L) (test_dropout_on), so a loss
    on the rates and the same loss written on the spikes, sum_c w[c] * s[:, :, c].sum() / sum(L), have the same gradient:
    the first travels as g_rate through bidir_join_backward (g_rate / sum(L) added on the valid steps, the cell kernel then
    multiplies by the mask and 1 / keep), the second as g_s.  The two incoming gradients differ by one fp32 rounding per
    element (w * (1 / n) against w / n: 6e-8 relative); the parameter gradients are linear in them, and BatchNorm's
    backward subtracts means, so the bound leaves two orders of magnitude for cancellation: 1e-5 of max-abs.  A second
    factor 1 / keep on the rate term would be an error of 33 %."""
    net = make_net(sp, kind, "batchnorm", dropout=0.25, use_readout_layer=False).to(DEV).train()
    for i, lay in enumerate(net.snn):
        lay._dropout_seed = lambda device, i=i: SEED + i
    x, _, init = net_inputs(kind)
    init = init[:2] + [dict(init[1])]            # (three hidden layers here: the third's states, 2 NB rows of 20)
    init[2] = {k: v[:, :SIZES[2]].contiguous() for k, v in init[2].items()}
    w = torch.linspace(-1.0, 2.0, 2 * sum(SIZES)).to(DEV)
    n = float(sum(LENGTHS))
    grads = []
    for on_rates in (True, False):
        net.zero_grad()
        with injected(init):
            s, rates = net(x.to(DEV), lengths=torch.tensor(LENGTHS), pack=pack)
        H = SIZES[-1]
        if on_rates:
            loss = (rates[-2 * H:] * w[-2 * H:]).sum()
        else:
            loss = (s.sum((0, 1)) / n * w[-2 * H:]).sum()
        loss.backward()
        grads.append({k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None})
    ga, gb = grads
    assert set(ga) == set(gb) and any("snn.0." in k for k in ga)
    for k in ga:
        assert float(ga[k].abs().max()) > 0, k
        assert relmax(N(ga[k]), N(gb[k])) <= 1e-5, k
    _Fn().check_status()


# ------------------------------------------------------------------------------------------------ composition
def rows_alone_equal(net, x, init, run, pick):
    """pick(run(net, x, lengths))[b] equals pick(run(net, x[b:b+1, :L_b], None)) for every clip, bit for bit."""
    with torch.no_grad():
        with injected(init):
            whole = pick(run(net, x.to(DEV), torch.tensor(LENGTHS)))
        for b, n in enumerate(LENGTHS):
            with injected(init, b):
                alone = pick(run(net, x[b:b + 1, :n].contiguous().to(DEV), None))
            got = whole[b:b + 1, :n] if whole.ndim == 3 else whole[b:b + 1]
            assert torch.equal(got, alone), (b, n)
            if whole.ndim == 3:
                assert not whole[b, n:].any()
    return whole


def test_per_step_readout_composes(sp):
    net = make_net(sp, "adLIF", "batchnorm").to(DEV).eval()
    x, _, init = net_inputs("adLIF")
    run = lambda net, x, L: net(x, per_step="sum") if L is None else net(x, lengths=L, per_step="sum")  # noqa: E731
    seq = rows_alone_equal(net, x, init, run, lambda r: r[2])
    out = rows_alone_equal(net, x, init, run, lambda r: r[0])
    for b, n in enumerate(LENGTHS):
        assert torch.equal(seq[b, n - 1], out[b])
    _Fn().check_status()


def test_selectable_readout_composes(sp):
    net = make_net(sp, "RLIF", "layernorm", readout="u_max").to(DEV).eval()
    x, _, init = net_inputs("RLIF")
    run = lambda net, x, L: net(x) if L is None else net(x, lengths=L)  # noqa: E731
    out = rows_alone_equal(net, x, init, run, lambda r: r[0])
    with torch.no_grad(), injected(init):
        packed, _ = net(x.to(DEV), lengths=torch.tensor(LENGTHS), pack=True)
    assert torch.equal(packed, out)
    _Fn().check_status()


def test_delays_compose(sp):
    """Delays act on the layer's input in forward time, before the split, as on the padded path."""
    net = make_net(sp, "adLIF", "none", max_delay=3, delay_init="uniform").to(DEV).eval()
    assert all(int(d.max()) > 0 for d in net.delay_steps().values())
    x, _, init = net_inputs("adLIF")
    run = lambda net, x, L: net(x) if L is None else net(x, lengths=L)  # noqa: E731
    out = rows_alone_equal(net, x, init, run, lambda r: r[0])
    with torch.no_grad(), injected(init):
        packed, _ = net(x.to(DEV), lengths=torch.tensor(LENGTHS), pack=True)
    assert torch.equal(packed, out)
    _Fn().check_status()


@pytest.mark.parametrize("pack", [False, True], ids=["mask", "pack"])
def test_input_from_counts_composes(sp, pack):
    """A uint8 batch travels as its bf16 plane: the projection reads it on NB rows, and what is split is the drive — the
    results are the fp32 input's bits, and backward works."""
    Fn = _Fn()
    x, y, init = net_inputs("adLIF")
    res = []
    for as_counts in (False, True):
        xin = Fn.input_from_counts(x.to(torch.uint8).to(DEV)) if as_counts else x.to(DEV)
        assert (Fn.input_plane_of(xin) is not None) == as_counts
        mine = make_net(sp, "adLIF", "batchnorm").to(DEV).train()
        with injected(init):
            out, rates = mine(xin, lengths=torch.tensor(LENGTHS), pack=pack)
            orc.train_step_loss(out, rates, y.to(DEV), use_regularizers=True).backward()
        res.append((out.detach(), rates.detach(), {k: v.grad.clone() for k, v in mine.named_parameters()}))
    (oa, ra, ga), (ob, rb, gb) = res
    assert torch.equal(oa, ob) and torch.equal(ra, rb)
    for k in ga:
        assert relmax(N(gb[k]), N(ga[k])) <= 5e-4, k
    Fn.check_status()


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_hd_bidirectional_with_lengths(tmp_path, monkeypatch):
    """SPARCH_LENGTHS=mask run_exp.py --bidirectional 1 --dataset_name hd on a tiny folder of unequal clips: two training
    steps, every batch goes to the network with its own unequal lengths, and the loss is finite.  (SPARCH_LENGTHS=pack
    with --bidirectional stays refused at the command line: DESIGN.md section 7; `net(x, lengths, pack=True)` is covered
    above.)"""
    import run_exp
    import sparch_amd
    from sparch_amd import exp
    from tests.audio_trees import make_hd_tree
    root = str(tmp_path / "hd")
    make_hd_tree(root, n_train=8, n_test=4, lengths=(16000, 6400, 11200, 9000))
    monkeypatch.setenv("SPARCH_LENGTHS", "mask")
    seen = []
    forward = sparch_amd.SNN.forward
    loss_call = exp.Fn.CrossEntropyLoss.forward

    def spy(self, x, lengths=None, pack=False):
        seen.append((None if lengths is None else [int(v) for v in lengths], pack))
        assert self.bidirectional and getattr(self, "_static_states", None) is None      # eager
        return forward(self, x, lengths=lengths, pack=pack)

    losses = []

    def loss_spy(self, output, target):
        v = loss_call(self, output, target)
        losses.append(float(v))
        return v

    monkeypatch.setattr(sparch_amd.SNN, "forward", spy)
    monkeypatch.setattr(exp.Fn.CrossEntropyLoss, "forward", loss_spy)
    torch.manual_seed(5)
    run_exp.main(["--model_type", "RadLIF", "--nb_layers", "3", "--nb_hiddens", "64", "--dataset_name", "hd",
                  "--bidirectional", "1", "--data_folder", root, "--batch_size", "4", "--nb_epochs", "1", "--save_best", "0",
                  "--new_exp_folder", str(tmp_path / "exp")])
    assert len(seen) >= 3 and all(v is not None and not pk for v, pk in seen)
    assert all(len(set(v)) > 1 for v, _ in seen[:2]), seen[:2]       # unequal clips in a batch
    assert len(losses) >= 3 and all(np.isfinite(v) for v in losses), losses
