"""
The feature fuzz of tests/feature_cases.py on the CPU.  The composed oracle (tests/feature_oracle.py) is held, in fp64,

  * bit for bit to the three oracles it extends, with every new feature off (oracle.snn_oracle.snn_forward,
    tests/ragged_oracle.snn_forward, tests/bidir_ragged_oracle.snn_forward), outputs and gradients;
  * with one new feature on, to that feature's numpy restatement (tests/delay_numpy.py, tests/synapse_numpy.py,
    tests/readout_modes_numpy.py, tests/readout_seq_numpy.py);
  * to the network without the feature at the neutral values gamma = 0 and delay = 0;
  * to the package's documented contract on its own masking: in eval mode row b of a batch is clip b run alone, for a
    case with delays, a synapse and two directions together.

Then the list: KEPT is what the keep rule gives (re-derived with the slack band of tests/test_network_fuzz_host.py),
every required pair of axis values is refused or covered by a kept case, at least half of the indices tried are kept,
every bound lies under the project's bars.  Every entry of REFUSED raises its ValueError before any entry point is
called, and every kept case — so every pair that is not refused — constructs and runs forward and backward against the
recording stand-in of tools/layer_call_trace.py.  Last, what the bound resolves: one delay moved by one step and the
filter's (1 - g) factor dropped, each an edit made here, leave the GPU test's acceptance by a factor of at least 100.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import snn_oracle as orc
from tests import bidir_ragged_oracle as bro
from tests import delay_numpy as dn
from tests import feature_cases as fc
from tests import feature_oracle as fo
from tests import ragged_oracle as rag
from tests import readout_modes_numpy as rmn
from tests import readout_seq_numpy as rsq
from tests import synapse_numpy as sy
from tests.kit import F64

F64T = torch.float64


def config(kind="RadLIF", norm="batchnorm", bidir=False, lengths=None, layout=None, B=3, T=9, C=8, sizes=(10, 12, 5),
           **kw):
    """A configuration made by hand: every new feature off unless kw switches it on."""
    cfg = dict(index=None, kind=kind, B=B, T=T, C=C, sizes=list(sizes), normalization=norm, bidirectional=bidir,
               use_bias=norm != "batchnorm", training=True, threshold=1.0, input="binary", real_weights=True, dropout=0.0,
               regulariser=True, surrogate=None, layout=layout or ("dense" if lengths is None else "lengths"),
               lengths=lengths, delay="off", max_delay=3, delay_layers="all", synapse="off", synapse_layers="all",
               output="softmax_sum")
    cfg.update(kw)
    return fc._finish(cfg)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ the oracle is the oracles
EXISTING = [(kind, norm, bidir, ragged, drop)
            for kind, norm in (("LIF", "batchnorm"), ("adLIF", "layernorm"), ("RLIF", "none"), ("RadLIF", "batchnorm"))
            for bidir in (False, True) for ragged in (False, True)
            for drop in ((0.0,) if (bidir and ragged) else (0.0, fc.P_DROP))]     # (no host mask on the doubled batch)


@pytest.mark.parametrize("kind,norm,bidir,ragged,drop", EXISTING)
def test_with_every_new_feature_off_it_is_the_existing_oracle_bit_for_bit(kind, norm, bidir, ragged, drop):
    """fp64 (the spike keeps its input's dtype on both sides): out, rates, spikes, loss, every gradient and the running
    statistics of oracle.snn_oracle.snn_forward — with lengths tests/ragged_oracle's, with two directions and lengths
    tests/bidir_ragged_oracle's — equal the composed oracle's, bit for bit."""
    L = [9, 1, 4] if ragged else None
    cfg = config(kind, norm, bidir, L, dropout=drop)
    c = fc.case_of(cfg, 11)
    got = fc.oracle_run(c, F64T)
    p = {k: v.double().clone().requires_grad_(v.is_floating_point() and "running" not in k)
         for k, v in c["params"].items() if "num_batches" not in k}
    init = [{k: v.double() for k, v in st.items()} for st in c["init"]]
    masks = None if c["masks"] is None else [m.double() for m in c["masks"]]
    spikes, stats = [], {}
    kw = dict(neuron_type=kind, num_layers=3, init_states=init, normalization=norm, training=True, theta=1.0, stats=stats,
              drop_masks=masks, spikes_out=spikes)
    with bro.own_dtype_spikes():
        if not ragged:
            out, rates = orc.snn_forward(c["x"].double(), p, bidirectional=bidir, use_readout_layer=True, **kw)
        elif not bidir:
            out, rates = rag.snn_forward(c["x"].double(), L, p, **kw)
        else:
            out, rates = bro.snn_forward(c["x"].double(), L, p, **kw)
    loss = fc.loss_of(cfg, out, rates, c["y"], c["gout"].double())
    loss.backward()
    assert same(got["out"], out.detach()) and same(got["rates"], rates.detach()) and same(got["loss"], loss.detach())
    assert len(spikes) == len(got["spikes"]) == 2 and all(same(a, b.detach()) for a, b in zip(got["spikes"], spikes))
    assert set(got["grads"]) == set(p) - {k for k in p if "running" in k}
    for k, v in got["grads"].items():
        assert same(v, p[k].grad), k
    assert set(got["stats"]) == set(stats) and all(same(got["stats"][k], stats[k]) for k in stats)
    assert bool(got["spikes"][1].any()) and (norm != "batchnorm" or stats)


# ------------------------------------------------------------------------------------------------ each feature alone
@pytest.mark.parametrize("lengths", [None, [9, 1, 4]], ids=["dense", "lengths"])
@pytest.mark.parametrize("D", fc.MAX_DELAYS)
def test_delays_are_the_numpy_restatement(D, lengths):
    """The wrapped Function: y, g_x and (fp64) g_theta are tests/delay_numpy.py's arrays; the sum the other dtypes take
    equals backward_theta to fp64 rounding in fp64 and to the rounding of an fp32 sum in fp32; and a layer with delays is
    the layer without them on the restatement's shifted input."""
    g = torch.Generator().manual_seed(D)
    B, T, K = 3, 9, 8
    x = ((torch.rand(B, T, K, generator=g) < 0.4).double() * torch.rand(B, T, K, generator=g).double())
    if lengths is not None:
        x = x * rag.valid_mask(lengths, T)[:, :, None]
    theta = torch.rand(K, generator=g) * (D + 1.0) - 0.5
    theta[:5] = torch.tensor([0.0, 2.5, 3.5, -0.75, D + 0.5])
    cot = torch.randn(B, T, K, generator=g).double()
    xr, th = x.clone().requires_grad_(True), theta.double().requires_grad_(True)
    y = fo.Delay.apply(xr, th, D, lengths)
    (y * cot).sum().backward()
    assert np.array_equal(y.detach().numpy(), dn.forward(x.numpy(), theta.numpy(), D, lengths))
    assert np.array_equal(xr.grad.numpy(), dn.backward_x(cot.numpy(), theta.numpy(), D, lengths))
    want, mag = dn.backward_theta(cot.numpy(), x.numpy(), theta.numpy(), D, lengths)
    assert np.array_equal(th.grad.numpy(), want) and np.abs(want).max() > 0
    outside = (theta.numpy() < 0) | (theta.numpy() > D)
    assert outside.any() and not want[outside].any()
    other = fo.finite_difference(cot, x, theta.numpy(), D, lengths).numpy()
    assert np.abs(other - want).max() <= 1e-14 * mag.max()
    x32, th32 = x.float().requires_grad_(True), theta.clone().requires_grad_(True)
    (fo.Delay.apply(x32, th32, D, lengths) * cot.float()).sum().backward()
    want32, mag32 = dn.backward_theta(cot.float().numpy(), x.float().numpy(), theta.numpy(), D, lengths)
    assert th32.grad.dtype == torch.float32 and np.abs(th32.grad.numpy() - want32).max() <= B * T * 2.0 ** -23 * mag32.max()
    # a delayed layer against the layer on the shifted input
    cfg = config("adLIF", "layernorm", False, lengths, delay="all", max_delay=D)
    c = fc.case_of(cfg, 5)
    p = {k: v.double() for k, v in c["params"].items() if "num_batches" not in k}
    init = {k: v.double() for k, v in c["init"][0].items()}
    kw = dict(normalization="layernorm", bidirectional=False, training=True)
    with bro.own_dtype_spikes():
        a = fo.hidden_layer("adLIF", c["x"].double(), lengths, p, "snn.0.", init, max_delay=D, **kw)
        plain = {k: v for k, v in p.items() if not k.endswith("delay")}
        shifted = torch.from_numpy(dn.forward(c["x"].double().numpy(), c["params"]["snn.0.delay"].numpy(), D, lengths))
        b = fo.hidden_layer("adLIF", shifted, lengths, plain, "snn.0.", init, **kw)
    assert same(a, b) and bool(a.any())
    assert not np.array_equal(shifted.numpy(), c["x"].double().numpy())


@pytest.mark.parametrize("bidir", [False, True], ids=["1dir", "2dir"])
@pytest.mark.parametrize("lengths", [None, [9, 1, 4]], ids=["dense", "lengths"])
def test_the_synapse_is_the_numpy_restatement(lengths, bidir):
    """The cell's input of a layer with a synapse is tests/synapse_numpy.forward of the same layer's input without one
    (on the doubled batch for two directions, the valid steps with lengths), and gamma's gradient through the filter is
    the restatement's, from its definition."""
    lo, hi = fc.SYN_LIMITS
    cfg = config("LIF", "batchnorm", bidir, lengths, synapse="all")
    c = fc.case_of(cfg, 7)
    p = {k: v.double() for k, v in c["params"].items() if "num_batches" not in k}
    init = {k: v.double() for k, v in c["init"][0].items()}
    kw = dict(normalization="batchnorm", bidirectional=bidir, training=True)
    with_syn, without = [], []
    with bro.own_dtype_spikes():
        fo.hidden_layer("LIF", c["x"].double(), lengths, p, "snn.0.", init, synapse=fc.SYN_LIMITS_F32, pre_cell=with_syn,
                        **kw)
        fo.hidden_layer("LIF", c["x"].double(), lengths, {k: v for k, v in p.items() if not k.endswith("gamma")}, "snn.0.",
                        init, pre_cell=without, **kw)
    gamma = c["params"]["snn.0.gamma"].numpy()
    assert (gamma < lo).any() and (gamma > hi).any()
    L2 = None if lengths is None else lengths * (2 if bidir else 1)
    want, _ = sy.forward(without[0].numpy(), gamma, lo, hi, lengths=L2, dtype=F64)
    m = fc.valid_rows(cfg).numpy()
    assert with_syn[0].shape == want.shape == (3 * (2 if bidir else 1), 9, 10)
    assert np.abs(np.where(m, with_syn[0].numpy() - want, 0.0)).max() <= 1e-14 * np.abs(want).max()
    assert np.abs(with_syn[0].numpy() - without[0].numpy()).max() > 0.1
    # gamma's gradient
    z = without[0].clone().requires_grad_(True)
    gm = torch.from_numpy(gamma).double().requires_grad_(True)
    cot = torch.randn(z.shape, generator=torch.Generator().manual_seed(3)).double() * torch.from_numpy(m).double()
    (fo.synapse_filter(z, gm, fc.SYN_LIMITS_F32) * cot).sum().backward()
    want_g = sy.backward_gamma_direct(cot.numpy(), without[0].numpy(), gamma, lo, hi, lengths=L2)
    assert np.abs(gm.grad.numpy() - want_g).max() <= 1e-12 * np.abs(want_g).max() and np.abs(want_g).max() > 0
    assert not gm.grad.numpy()[(gamma < np.float32(lo)) | (gamma > np.float32(hi))].any()
    want_z = sy.backward_z(cot.numpy(), gamma, lo, hi, lengths=L2, dtype=F64)
    assert np.abs(np.where(m, z.grad.numpy() - want_z, 0.0)).max() <= 1e-13 * np.abs(want_z).max()


def _readout_inputs(lengths):
    cfg = config("LIF", "none", False, lengths, sizes=(10, 5))
    c = fc.case_of(cfg, 9)
    c["params"]["snn.1.alpha"][:2] = torch.tensor([0.5, 1.2])      # below and above the clamp range
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(3, 9, 10, generator=g) < 0.3).double()
    p = {k: v.double() for k, v in c["params"].items()}
    Wx = F.linear(x, p["snn.1.W.weight"], p["snn.1.W.bias"]).numpy()
    return x, p, c["init"][1]["u0"].double(), Wx, c["params"]["snn.1.alpha"].numpy()


@pytest.mark.parametrize("lengths", [None, [9, 1, 4]], ids=["dense", "lengths"])
@pytest.mark.parametrize("mode", rmn.MODES)
def test_the_readout_modes_are_the_numpy_restatement(mode, lengths):
    x, p, u0, Wx, alpha = _readout_inputs(lengths)
    kw = dict(normalization="none", training=True)
    got = fo.readout_layer(x, lengths, p, "snn.1.", u0, readout=mode, **kw)
    want = rmn.forward(F64, Wx, None, None, alpha, u0.numpy(), mode, lengths)["out"]
    lo, hi = orc.ALPHA_LIM
    assert (alpha < lo).any() or (alpha > hi).any()
    if mode == "softmax_sum":
        # the default has two forms: the existing oracles' cell, which clamps alpha at the limits in double, and the
        # restatement's torch form, which clamps at the fp32 limits as the restatement does (2e-8 apart)
        forced = fo.readout_layer(x, lengths, p, "snn.1.", u0, readout=mode, force_modes=True, **kw)
        assert np.abs(forced.numpy() - want).max() <= 1e-13 * np.abs(want).max()
        assert np.abs(got.numpy() - want).max() <= 1e-7 * np.abs(want).max()
    else:
        assert np.abs(got.numpy() - want).max() <= 1e-13 * np.abs(want).max()
        default = fo.readout_layer(x, lengths, p, "snn.1.", u0, **kw)
        assert np.abs(default.numpy() - got.numpy()).max() > 1e-2


@pytest.mark.parametrize("lengths", [None, [9, 1, 4]], ids=["dense", "lengths"])
@pytest.mark.parametrize("mode", rsq.MODES)
def test_the_per_step_readout_is_the_numpy_restatement(mode, lengths):
    x, p, u0, Wx, alpha = _readout_inputs(lengths)
    out, seq = fo.readout_layer(x, lengths, p, "snn.1.", u0, normalization="none", training=True, per_step=mode)
    want = rsq.forward(F64, Wx, None, None, alpha, u0.numpy(), mode, lengths)
    assert np.abs(out.numpy() - want["out"]).max() <= 1e-13 and np.abs(seq.numpy() - want["seq"]).max() <= 1e-13
    assert seq.shape == (3, 9, 5) and (lengths is None or not seq[1, 1:].any())
    default = fo.readout_layer(x, lengths, p, "snn.1.", u0, normalization="none", training=True)
    assert np.abs(out.numpy() - default.numpy()).max() <= 1e-7


# ------------------------------------------------------------------------------------------------ neutral values
@pytest.mark.parametrize("bidir,lengths", [(False, None), (True, None), (False, [9, 1, 4]), (True, [9, 1, 4])])
def test_gamma_0_and_delay_0_give_the_network_without_the_feature(bidir, lengths):
    """fp64: out, rates, loss and the spikes bit for bit, the shared gradients to 1e-13 of their max-abs."""
    on = config("RadLIF", "batchnorm", bidir, lengths, delay="all", synapse="all")
    off = config("RadLIF", "batchnorm", bidir, lengths)
    c = fc.case_of(on, 13)
    for k in c["params"]:
        if k.endswith(("delay", "gamma")):
            c["params"][k] = torch.zeros_like(c["params"][k])
    plain = dict(c, cfg=off, params={k: v for k, v in c["params"].items() if not k.endswith(("delay", "gamma"))})
    a, b = fc.oracle_run(c, F64T), fc.oracle_run(plain, F64T)
    assert same(a["out"], b["out"]) and same(a["rates"], b["rates"]) and same(a["loss"], b["loss"])
    assert all(same(s, t) for s, t in zip(a["spikes"], b["spikes"])) and bool(a["spikes"][1].any())
    assert set(a["grads"]) - set(b["grads"]) == {f"snn.{k}.delay" for k in range(3)} | {f"snn.{k}.gamma" for k in range(2)}
    for k, v in b["grads"].items():     # (autograd adds two directions' terms in another order with the nodes between)
        assert fc.maxabs(a["grads"][k] - v) <= 1e-13 * fc.maxabs(v), k
    assert all(bool(a["grads"][k].any()) for k in a["grads"] if k.endswith(("delay", "gamma")))


# ------------------------------------------------------------------------------------------------ a row is its clip alone
@pytest.mark.parametrize("norm", fc.NORMS)
def test_in_eval_mode_a_row_is_its_clip_run_alone(norm):
    """Delays, a synapse and two directions together, lengths [9, 1, 4]: every row of out, seq and the hidden spikes is
    what the clip gives on its own through the DENSE branch of the oracle (no lengths), with the initial-state rows b and
    B + b; the spikes behind the clip's end are zero."""
    L = [9, 1, 4]
    cfg = config("RadLIF", norm, True, L, delay="all", synapse="all", output="sum", training=False, use_bias=False)
    c = fc.case_of(cfg, 17)
    whole = fc.oracle_run(c, F64T, backward=False)
    assert bool(whole["spikes"][1].any())
    for b, n in enumerate(L):
        clip = dict(c, cfg=dict(cfg, B=1, T=n, lengths=None, layout="dense"), x=c["x"][b:b + 1, :n],
                    init=bro.rows_of(c["init"], b, 3))
        alone = fc.oracle_run(clip, F64T, backward=False)
        assert fc.maxabs(alone["out"] - whole["out"][b:b + 1]) <= 1e-12
        assert fc.maxabs(alone["seq"] - whole["seq"][b:b + 1, :n]) <= 1e-12 and not whole["seq"][b, n:].any()
        for s, t in zip(alone["spikes"], whole["spikes"]):
            assert same(s, t[b:b + 1, :n]) and not t[b, n:].any()


# ------------------------------------------------------------------------------------------------ the list
def test_kept_is_what_the_rule_gives_and_every_pair_is_covered():
    kept = list(fc.KEPT)
    assert len(kept) == len(set(kept)) and 64 <= len(kept) <= 96
    derived, tried, rejected = fc.derive_kept()
    print(f"  the rule as it stands gives {'KEPT' if derived == kept else 'another list'} here")
    tried = fc.tried_indices()
    for i in tried:
        if fc.verdict(i, 2.0)[0]:
            assert i in kept, (i, "passes the tightened rule")
        if not fc.verdict(i, 0.5)[0]:
            assert i not in kept, (i, fc.verdict(i, 0.5)[1])
    # fill indices are there for a pair that the indices before them leave uncovered
    for n, i in enumerate(kept):
        if i >= fc.FILL_BASE:
            pair = fc.required_pairs()[(i - fc.FILL_BASE) // fc.FILL_TRIES]
            assert pair in fc.coverage(kept[:n])[2] and pair in fc.pairs_of(fc.draw(i)), (i, pair)
    # coverage: every required pair is refused or occurs in a kept case
    covered, refused, missing = fc.coverage(kept)
    print(f"  {len(fc.required_pairs())} pairs: {len(covered)} covered, {len(refused)} refused, {len(missing)} missing")
    assert not missing, missing
    assert not covered & refused and len(covered) + len(refused) == len(fc.required_pairs())
    # keep rate
    share = len(kept) / len(tried)
    print(f"  kept {len(kept)} of {len(tried)} indices tried ({share:.2f})")
    for i in tried:
        if i not in kept:
            print(f"    {fc.label(fc.draw(i))}: {fc.verdict(i)[1]}")
    assert 2 * len(kept) >= len(tried)
    # the axes beside the pairs, and the shapes
    cfgs = [fc.draw(i) for i in kept]
    assert {c["max_delay"] for c in cfgs} >= set(fc.MAX_DELAYS) and {c["input"] for c in cfgs} == set(fc.INPUTS)
    assert {c["training"] for c in cfgs} == {True, False} and {c["use_bias"] for c in cfgs} == {True, False}
    assert {c["real_weights"] for c in cfgs} == {True, False} and {c["regulariser"] for c in cfgs} == {True, False}
    for name, values in (("B", fc.BATCHES), ("T", fc.STEPS), ("C", fc.CHANNELS)):
        assert {c[name] for c in cfgs} == set(values)
    assert {h for c in cfgs for h in c["sizes"]} >= set(fc.WIDTHS) | set(fc.CLASSES)
    for c in cfgs:
        if c["lengths"] is not None:
            assert len(c["lengths"]) == c["B"] and {1, c["T"]} <= set(c["lengths"])
            assert not (fc.case(c["index"])["x"] * ~rag.valid_mask(c["lengths"], c["T"])[:, :, None]).any()
        assert fc.refusal(fc.axis_values(c).values()) is None
    # the two fixed cases (their data seeds were picked at 4 x the rule; the fp32 run's error moves with the CPU and its
    # thread count, tests/network_cases.py verdict); every bound lies under the project's bars (asserted inside)
    for i in (fc.WIDE, fc.DX_PLANES):
        print(f"  fixed case {i}:", fc.verdict(i), fc.verdict(i, 4.0))
        assert fc.verdict(i, 0.5)[0], (i, fc.verdict(i, 0.5))
    assert fc.draw(fc.WIDE)["sizes"][0] == 264
    d = fc.draw(fc.DX_PLANES)
    assert d["bidirectional"] and d["layout"] == "lengths" and d["delay"] == "all" and {1, 8} <= set(d["lengths"])
    for i in kept + [fc.WIDE, fc.DX_PLANES]:
        fc.bounds(i)
    print("  r_role: " + ", ".join(f"{k} {v:.2e}" for k, v in fc.role_errors().items()))
    assert all(v > 0 for v in fc.role_errors().values())
    assert len(fc.bf16_cases()) >= 8 and len([i for i in kept if fc.other_layout(fc.draw(i))]) >= 16


def test_draw_is_a_pure_function_of_the_index():
    for i in (0, 5, 95, fc.FILL_BASE + 7, fc.WIDE, fc.DX_PLANES):
        assert fc.draw(i) == fc.draw(i)
    assert fc.draw(3) != fc.draw(4)
    for n, pair in enumerate(fc.required_pairs()):
        if fc.refusal(pair) is None and n % 7 == 0:
            for attempt in range(fc.FILL_TRIES):
                assert pair in fc.pairs_of(fc.draw(fc.fill_index(pair, attempt)))
    for i in range(200):        # no draw is refused, and dropout stays off where no host mask exists
        cfg = fc.draw(i)
        assert fc.refusal(fc.axis_values(cfg).values()) is None
        if cfg["dropout"] > 0:
            assert cfg["training"] and (not cfg["bidirectional"] or (cfg["layout"] == "dense" and cfg["synapse"] == "off"))


# ------------------------------------------------------------------------------------------------ refusals, reachability
def _traced(run):
    """The launching calls `run` issues against the recording stand-in (queries and timer labels left out)."""
    from tools import layer_call_trace as lct
    rec = lct._Recorder()
    with lct._tracing(rec):
        rec.new_case("case")
        try:
            run()
        finally:
            lines = [ln for ln in rec.lines[1:] if ln.startswith("sparch_")]
    return lines


def _refused_config(combo):
    """A configuration that holds the axis values of a REFUSED entry and, beside them, nothing that is refused."""
    a = dict(v.split("=") for v in combo)
    cfg = config(a.get("kind", "LIF"), a.get("norm", "layernorm"), a.get("dirs", "1") == "2", [9, 1, 4],
                 layout=a.get("layout", "lengths"), delay=a.get("delay", "off"), synapse=a.get("synapse", "off"),
                 output=a.get("output", "softmax_sum"), use_bias=a.get("bias", "False") == "True")
    assert set(combo) <= set(fc.axis_values(cfg).values())
    return cfg


@pytest.mark.parametrize("combo", list(fc.REFUSED), ids=["+".join(c) for c in fc.REFUSED])
def test_every_refused_combination_raises_before_any_entry_point(combo):
    import sparch_amd as sp
    cfg = _refused_config(combo)
    seen = []

    def run():
        net = sp.SNN((cfg["B"], None, cfg["C"]), cfg["sizes"], **fc.net_kwargs(cfg))
        try:
            with pytest.raises(ValueError, match=fc.REFUSED[combo].replace("(", r"\(")):
                net(torch.zeros(cfg["B"], cfg["T"], cfg["C"]), **fc.forward_kwargs(cfg))
        finally:
            seen.append(True)

    assert _traced(run) == [] and seen
    # and each entry is needed: with one of its values changed the call goes through
    for k, v in enumerate(combo):
        axis, value = v.split("=")
        other = {"layout": "dense", "output": "softmax_sum", "norm": "layernorm", "bias": "False", "dirs": "1",
                 "synapse": "off"}[axis]
        relaxed = tuple(f"{axis}={other}" if n == k else w for n, w in enumerate(combo))
        ok = _refused_config(relaxed)
        if ok["layout"] == "dense":
            ok = dict(ok, lengths=None)
        net = [None]

        def run_ok():
            net[0] = sp.SNN((ok["B"], None, ok["C"]), ok["sizes"], **fc.net_kwargs(ok))
            net[0](torch.zeros(ok["B"], ok["T"], ok["C"]), **fc.forward_kwargs(ok))

        assert fc.refusal(relaxed) is None and _traced(run_ok), relaxed


@pytest.mark.parametrize("kw,words", [(dict(readout="u_max"), "per_step with readout="),
                                      (dict(use_readout_layer=False), "per_step needs a readout layer")])
def test_the_refusals_inside_the_output_axis(kw, words):
    """per_step with another readout mode or without a readout layer: two values of ONE axis, so not in REFUSED."""
    import sparch_amd as sp

    def run():
        net = sp.SNN((3, None, 8), [10, 5], neuron_type="LIF", **kw)
        with pytest.raises(ValueError, match=words):
            net(torch.zeros(3, 9, 8), per_step="prob")

    assert _traced(run) == []


def test_every_kept_case_constructs_and_traces():
    """Reachability: every kept case — and with them every pair of axis values that is not refused (the coverage
    condition) — builds with the case's parameters and runs forward and backward on CPU tensors against the recording
    stand-in, with the calls its features stand for."""
    import sparch_amd as sp
    from tools import layer_call_trace as lct
    for i in list(fc.KEPT) + [fc.WIDE, fc.DX_PLANES]:
        c = fc.case(i)
        cfg = c["cfg"]

        def run():
            net, _ = fc.build(sp, cfg)
            net.train(cfg["training"])
            res = net(c["x"].clone(), **fc.forward_kwargs(cfg))
            assert len(res) == (3 if cfg["per_step"] else 2)
            if cfg["training"]:
                lct._backward(*res)

        lines = _traced(run)
        label = fc.label(cfg)
        layers = len(cfg["sizes"])
        n_delay = sum(fc.has_delay(cfg, k) for k in range(layers))
        n_syn = sum(fc.has_synapse(cfg, k) for k in range(layers))
        assert len(lct.calls(lines, "sparch_delay_fwd")) == n_delay, label
        assert len([ln for ln in lines if ln.startswith("sparch_synapse_fwd")]) == n_syn, label
        assert bool([ln for ln in lines if ln.startswith("sparch_pack_rows")]) == (cfg["layout"] == "pack"), label
        ragged_two = cfg["bidirectional"] and (cfg["layout"] != "dense" or cfg["synapse"] != "off")
        assert bool([ln for ln in lines if ln.startswith("sparch_bidir_")]) == ragged_two, label


# ------------------------------------------------------------------------------------------------ what the bound resolves
def factor_outside(i, wrong):
    """By how much a wrong run leaves the GPU test's acceptance (tests/test_network_fuzz_host.py factor_outside):
    infinite if a spike differs."""
    ref = fc.runs(i)[0]
    if any(not torch.equal(a, b) for a, b in zip(ref["spikes"], wrong["spikes"])):
        return float("inf")
    bound = fc.bounds(i)
    a, b = fc.compared(ref), fc.compared(wrong)
    worst = max(fc.maxabs(b[k] - a[k]) / bound[k] for k in bound)
    return max(worst, fc.maxabs(wrong["rates"] - ref["rates"]) / (1e-6 * fc.maxabs(ref["rates"])))


def _both_learnable():
    cases = [i for i in fc.KEPT if fc.draw(i)["learn_delays"] and fc.draw(i)["learn_synapse"] and fc.draw(i)["training"]]
    assert len(cases) >= 2
    return cases


def test_the_unedited_fp32_run_is_inside_every_bound():
    for i in _both_learnable():
        r32 = fc.runs(i)[1]
        as64 = dict(r32, out=r32["out"].double(), loss=r32["loss"].double(), rates=r32["rates"].double(),
                    seq=None if r32["seq"] is None else r32["seq"].double(), spikes=[s.double() for s in r32["spikes"]],
                    grads={k: v.double() for k, v in r32["grads"].items()})
        assert factor_outside(i, as64) <= 1.0


def test_the_bound_sees_a_delay_moved_by_one_step():
    """One in-range delay of every delayed layer moved to the neighbouring step."""
    factors = {}
    for i in _both_learnable():
        c = fc.case(i)
        D = c["cfg"]["max_delay"]
        params = dict(c["params"])
        for k, v in params.items():
            if k.endswith("delay"):
                d = dn.steps(v.numpy(), D)
                j = int(np.argmax((v.numpy() >= 0) & (v.numpy() <= D) & (np.arange(len(d)) >= 5)))
                v = v.clone()
                v[j] = float(d[j] + 1 if d[j] < D else d[j] - 1)
                params[k] = v
        factors[i] = factor_outside(i, fc.oracle_run(dict(c, params=params), F64T))
    print("  factors:", factors)
    assert sum(f >= 100.0 for f in factors.values()) >= 2, factors


def test_the_bound_sees_the_filter_without_its_1_minus_g(monkeypatch):
    def wrong_filter(z, gamma, limits):
        g = torch.clamp(gamma, min=limits[0], max=limits[1])
        cur, out = torch.zeros_like(z[:, 0]), []
        for t in range(z.shape[1]):
            cur = g * cur + z[:, t]
            out.append(cur)
        return torch.stack(out, dim=1)

    monkeypatch.setattr(fo, "synapse_filter", wrong_filter)
    factors = {i: factor_outside(i, fc.oracle_run(fc.case(i), F64T)) for i in _both_learnable()}
    print("  factors:", factors)
    assert sum(f >= 100.0 for f in factors.values()) >= 2, factors
