"""
Synaptic currents on the device ("Synaptic currents"), against tests/synapse_numpy.py and the
layer-level oracle of tests/synapse_cases.py.

Kernels (sparch_synapse_fwd / _bwd through functional.synapse_forward / synapse_backward / synapse_stream): B = 3, T = 9,
H in {5, 8, 36} and H = 264 (66 four-column pieces per sequence: the 64-lane workgroups are cut inside a row and across
sequences); dense, lengths = [9, 1, 4] and packed through snns.prepare_packing; with and without bias / scale / shift;
limits (0, 0.9) and (0.25, 0.875) with gamma columns 0, lo, hi, below lo, above hi; a row stride that keeps the 16-byte
pieces and one that does not; BatchNorm's column sums (`bn=`) against their fp32 restatement, learnable and fixed.  i, i_T and g_z are bit-equal to the fp32 restatement of the kernels' expression tree;
every valid element is written (NaN-poisoned outputs), g_i on padded steps is never read (NaN there).  g_gamma is
within the bound derived in tests/synapse_numpy.py of the fp64 value, bit-equal across two runs, exactly 0 where the
gate is 0.  The stream form in chunks of 1, 2 and 5 steps equals the whole-sequence call bit for bit.  (Time is not cut
into segments: there is no segment length to straddle.)

Networks (tests/synapse_cases.py: all four kinds, 8 -> 12 -> 12 -> 5 and a recurrent width of 10, B = 3, T = 12,
BatchNorm, LayerNorm and none, bidirectional with and without lengths, a smooth surrogate, one case with max_delay; data
seeds picked on the host by the keep rule of tests/network_cases.py): gamma = 0 under limits (0, 0.9) is the network
without a synapse, bit for bit, for one direction and for both directions called with lengths; both directions called
without lengths: bit-equal in eval mode, a training step to the bars of tests/test_bidir_ragged_gpu.py; with gamma in (0.3, 0.9) the spikes equal the oracle's exactly and out, loss and every
parameter gradient, gamma's included, lie within OUT_CAP / LOSS_CAP / GRAD_CAP of tests/network_cases.py; with lengths
each clip run alone is its row of the batch; pack=True equals lengths (eval bit-equal, train to GRAD_CAP); a
StreamingSNN fed in chunks reproduces the whole-sequence spikes and its "i" round-trips; one Adam step moves gamma and
leaves it alone under learn_synapse=False; run_exp.py trains two epochs under SPARCH_SYNAPSE=0:0.9.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import packed_numpy as pn
from tests import synapse_cases as sc
from tests import synapse_numpy as syn
from tests.kit import DEV, F32, F64, N, relmax, same_bits, within
from tests.kit import Fn as _Fn
from tests.kit import sp  # noqa: F401  (a fixture)
from tests.network_cases import GRAD_CAP, LOSS_CAP, OUT_CAP, RATE_WINDOW
from tests.stream_cases import run_stream, whole_forward

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T = sc.B, sc.T
ALL_WIDTHS = sc.WIDTHS + (sc.WIDE_H,)


def plan_of(lengths, T_):
    from sparch_amd import snns
    return snns.prepare_packing(torch.as_tensor(np.asarray(lengths)), len(lengths), T_, DEV)


def dev_lengths(lengths):
    return torch.from_numpy(np.asarray(lengths).astype(np.int32)).to(DEV), int(np.sum(lengths))


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, F32)).to(DEV)


def poison(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def reference(d, gamma, lim, lengths):
    """The fp32 restatement (z, i, i_T, g_z) and the fp64 one (z, i) of one kernel case."""
    z32 = syn.drive(d["Wx"], d["bias"], d["scale"], d["shift"], F32)
    i32, iT32 = syn.forward(z32, gamma, *lim, d["i0"], lengths, F32)
    gz32 = syn.backward_z(d["g"], gamma, *lim, lengths, F32)
    z64 = syn.drive(d["Wx"], d["bias"], d["scale"], d["shift"], F64)
    i64, _ = syn.forward(z64, gamma, *lim, d["i0"], lengths, F64)
    return z32, i32, iT32, gz32, z64, i64


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("layout", ["dense", "lengths", "packed"])
@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("lim", sc.LIMITS, ids=["0-0.9", "0.25-0.875"])
@pytest.mark.parametrize("H", ALL_WIDTHS)
def test_kernels_against_the_restatements(H, lim, affine, layout):
    Fn = _Fn()
    d, gamma = sc.kernel_data(H, affine), sc.gammas(H, *lim)
    assert gamma[0] == 0 and gamma[1] == F32(lim[0]) and gamma[2] == F32(lim[1]) and gamma[3] < lim[0] and gamma[4] > lim[1]
    lengths = None if layout == "dense" else sc.LENGTHS
    z32, i32, iT32, gz32, z64, i64 = reference(d, gamma, lim, lengths)
    gd = dev(gamma)
    aff = dict(bias=dev(d["bias"]), scale=dev(d["scale"]), shift=dev(d["shift"]))
    dirty = d["g"].copy()                                   # what g_i holds on padded steps is never read
    if lengths is not None:
        dirty[~pn.valid_mask(lengths, T)] = np.nan
    if layout == "packed":
        plan = plan_of(lengths, T)
        order = pn.plan_of(lengths)[0]
        kw = dict(pack=plan)
        pk = lambda a: dev(pn.pack(a, lengths)).unsqueeze(0)  # noqa: E731
        i, i_T = Fn.synapse_forward(pk(d["Wx"]), gd, lim, i0=dev(d["i0"][order]), want_final=True,
                                    out=poison(1, plan.n, H), **aff, **kw)
        assert same_bits(N(i)[0], pn.pack(i32, lengths)) and same_bits(N(i_T), iT32[order])
        runs = [Fn.synapse_backward(pk(d["g"]), i, gd, lim, i0=dev(d["i0"][order]), out=poison(1, plan.n, H), **kw)
                for _ in range(2)]
        assert same_bits(N(runs[0][0])[0], pn.pack(gz32, lengths))
    else:
        kw = {} if lengths is None else dict(lengths=dev_lengths(lengths))
        i, i_T = Fn.synapse_forward(dev(d["Wx"]), gd, lim, i0=dev(d["i0"]), want_final=True, out=poison(B, T, H),
                                    **aff, **kw)
        assert same_bits(N(i), i32) and same_bits(N(i_T), iT32)
        runs = [Fn.synapse_backward(dev(dirty), i, gd, lim, i0=dev(d["i0"]), out=poison(B, T, H), **kw) for _ in range(2)]
        assert same_bits(N(runs[0][0]), gz32)
        only_z, none = Fn.synapse_backward(dev(dirty), None, gd, lim, need_ggamma=False, **kw)
        assert none is None and same_bits(N(only_z), gz32)
    assert np.isfinite(i32).all() and (i32 != 0).any()
    g0, g1 = N(runs[0][1]), N(runs[1][1])
    assert same_bits(g0, g1)                                # no atomics: the same bits on every run
    ref, _ = syn.backward_gamma(d["g"], i64, gamma, *lim, d["i0"], lengths)
    bound = syn.gamma_bound(d["g"], z64, gamma, *lim, d["i0"], lengths)
    gate = syn.gate(gamma, *lim)
    assert (gate == 0).any() and (ref[gate == 1] != 0).all() and not g0[gate == 0].any()
    within(g0, ref, bound, f"g_gamma H={H} {layout}")
    Fn.check_status()


@pytest.mark.parametrize("ld", [11, 16])
def test_kernels_take_a_row_stride(ld):
    """H = 8 columns of rows ld elements apart, read and written where they lie: ld = 16 keeps the 16-byte pieces, ld = 11
    takes single elements; the columns behind H stay as they were."""
    Fn = _Fn()
    H, lim = 8, sc.LIMITS[1]
    d, gamma = sc.kernel_data(H), sc.gammas(H, *lim)
    _, i32, iT32, gz32, z64, i64 = reference(d, gamma, lim, sc.LENGTHS)
    kw = dict(lengths=dev_lengths(sc.LENGTHS))
    wide = poison(B, T, ld)
    wide[:, :, :H] = dev(d["Wx"])
    out = torch.full((B, T, ld), 5.0, dtype=torch.float32, device=DEV)
    i, i_T = Fn.synapse_forward(wide[:, :, :H], dev(gamma), lim, dev(d["bias"]), dev(d["scale"]), dev(d["shift"]),
                                i0=dev(d["i0"]), want_final=True, out=out[:, :, :H], **kw)
    assert i.data_ptr() == out.data_ptr() and same_bits(N(i.contiguous()), i32) and same_bits(N(i_T), iT32)
    assert bool((out[:, :, H:] == 5.0).all())
    gw = poison(B, T, ld)
    gw[:, :, :H] = dev(d["g"])
    gout = torch.full((B, T, ld), 3.0, dtype=torch.float32, device=DEV)
    g_z, g_gamma = Fn.synapse_backward(gw[:, :, :H], out[:, :, :H], dev(gamma), lim, i0=dev(d["i0"]), out=gout[:, :, :H], **kw)
    assert same_bits(N(g_z.contiguous()), gz32) and bool((gout[:, :, H:] == 3.0).all())
    ref, _ = syn.backward_gamma(d["g"], i64, gamma, *lim, d["i0"], sc.LENGTHS)
    within(N(g_gamma), ref, syn.gamma_bound(d["g"], z64, gamma, *lim, d["i0"], sc.LENGTHS), f"g_gamma ld={ld}")
    Fn.check_status()


@pytest.mark.parametrize("layout", ["dense", "lengths", "packed"])
@pytest.mark.parametrize("learn", [True, False], ids=["learnable", "fixed"])
@pytest.mark.parametrize("H", ALL_WIDTHS)
def test_the_backward_scan_adds_batchnorms_column_sums(H, learn, layout):
    """`bn=(x, mean, invstd)`: sum g_z and sum g_z xhat per column.  The per-sequence partial sums are fp32 sums in a
    fixed order, restated exactly (tests/synapse_numpy.py bn_partials); the device adds the B of them in double and
    rounds once, so the result lies within 2^-24 sum |partials| (that one rounding) of their exact sum.  H = 5: single
    columns per lane; fixed: the variant that does not read i.  g_z keeps its bits, g_gamma its bound."""
    Fn = _Fn()
    lim = sc.LIMITS[1]
    d, gamma = sc.kernel_data(H), sc.gammas(H, *lim)
    lengths = None if layout == "dense" else sc.LENGTHS
    _, i32, _, gz32, z64, i64 = reference(d, gamma, lim, lengths)
    rng = np.random.default_rng([H, 11])
    mean, invstd = rng.standard_normal(H).astype(F32), rng.uniform(0.5, 2.0, H).astype(F32)
    dy, dyx = syn.bn_partials(gz32, d["Wx"], mean, invstd, lengths)
    if layout == "packed":
        kw = dict(pack=plan_of(lengths, T))
        order = pn.plan_of(lengths)[0]
        pk = lambda a: dev(pn.pack(a, lengths)).unsqueeze(0)  # noqa: E731
        g_in, i_in, x_in, i0 = pk(d["g"]), pk(i32), pk(d["Wx"]), dev(d["i0"][order])
        gz_ref = pn.pack(gz32, lengths)[None]
    else:
        kw = {} if lengths is None else dict(lengths=dev_lengths(lengths))
        dirty = d["g"].copy()
        if lengths is not None:
            dirty[~pn.valid_mask(lengths, T)] = np.nan
        g_in, i_in, x_in, i0, gz_ref = dev(dirty), dev(i32), dev(d["Wx"]), dev(d["i0"]), gz32
    runs = [Fn.synapse_backward(g_in, i_in if learn else None, dev(gamma), lim, i0=i0, need_ggamma=learn,
                                bn=(x_in, dev(mean), dev(invstd)), **kw) for _ in range(2)]
    g_z, g_gamma, sums = runs[0]
    assert same_bits(N(g_z), gz_ref)
    for got, again, part, what in ((sums[0], runs[1][2][0], dy, "sum g_z"), (sums[1], runs[1][2][1], dyx, "sum g_z xhat")):
        assert same_bits(N(got), N(again))
        exact = part.astype(F64).sum(axis=0)
        assert exact.any()
        within(N(got), exact, 2.0 ** -24 * np.abs(part.astype(F64)).sum(axis=0), f"{what} H={H} {layout}")
    if learn:
        ref, _ = syn.backward_gamma(d["g"], i64, gamma, *lim, d["i0"], lengths)
        within(N(g_gamma), ref, syn.gamma_bound(d["g"], z64, gamma, *lim, d["i0"], lengths), f"g_gamma H={H} {layout}")
    else:
        assert g_gamma is None
    Fn.check_status()


@pytest.mark.parametrize("H", ALL_WIDTHS)
def test_the_stream_in_chunks_is_the_whole_sequence(H):
    Fn = _Fn()
    lim = sc.LIMITS[0]
    d, gamma = sc.kernel_data(H), sc.gammas(H, *lim)
    aff = dict(bias=dev(d["bias"]), scale=dev(d["scale"]), shift=dev(d["shift"]))
    whole, i_T = Fn.synapse_forward(dev(d["Wx"]), dev(gamma), lim, i0=dev(d["i0"]), want_final=True, **aff)
    state, parts, t0 = dev(d["i0"]), [], 0
    x = dev(d["Wx"])
    for n in (1, 2, 5, 1):
        parts.append(Fn.synapse_stream(x[:, t0:t0 + n], dev(gamma), lim, state, **aff))
        t0 += n
    assert t0 == T
    assert same_bits(torch.cat(parts, dim=1), whole) and same_bits(state, i_T)
    Fn.check_status()


# ------------------------------------------------------------------------------------------------ networks
def layer_rates(rates, c):
    sizes, n = c[6], 2 if c[2] else 1
    r, at, out = N(rates), 0, []
    for H in sizes[:-1]:
        out.append(float(r[at:at + H * n].mean()))
        at += H * n
    assert at == r.size
    return out


def assert_alive(rates, c):
    per_layer = layer_rates(rates, c)
    print(f"  firing rates per hidden layer: {per_layer}")
    assert all(RATE_WINDOW[0] <= r <= RATE_WINDOW[1] for r in per_layer), per_layer


PLAIN = [c for c in sc.CASES if not c[3] and not c[5]] + [c for c in sc.CASES if c[2] and c[3]]


@pytest.mark.parametrize("c", PLAIN, ids=sc.case_id)
def test_gamma_zero_is_the_network_without_a_synapse_bit_for_bit(sp, c):
    """One direction, and both directions called with lengths (a bidirectional case without lengths is given lengths = T
    on both sides here: one route).  A bidirectional network called WITHOUT lengths takes the doubled-batch route under
    a synapse and the dense two-direction kernels without one, which are not bit-equal in a training step: the test
    below holds that pair."""
    seed = sc.SEEDS[c]
    fw = dict(lengths=torch.full((sc.NB,), sc.NT)) if (c[2] and not c[3]) else {}
    plain = sc.device_run(sp, c, seed, net=sc.make_net(sp, c, synapse=None), **fw)
    zero_net = sc.make_net(sp, c)
    with torch.no_grad():
        for lay in zero_net.snn[:-1]:
            lay.gamma.zero_()
    zero = sc.device_run(sp, c, seed, net=zero_net, **fw)
    assert_alive(plain["rates"], c)
    for k in ("out", "rates", "loss"):
        assert same_bits(zero[k].detach(), plain[k].detach()), k
    grads = dict(zero["net"].named_parameters())
    for name, p in plain["net"].named_parameters():
        assert p.grad is not None and bool(p.grad.any()), name
        assert same_bits(grads[name].grad, p.grad), name
    for k in range(2):                                      # gamma itself has a gradient at 0 = lo
        g = grads[f"snn.{k}.gamma"].grad
        assert g is not None and bool(torch.isfinite(g).all()) and bool(g.any()), k


@pytest.mark.parametrize("c", [c for c in sc.CASES if c[2] and not c[3]], ids=sc.case_id)
def test_gamma_zero_bidirectional_without_lengths_against_the_plain_network(sp, c):
    """Both networks called without lengths: with a synapse the layers make lengths = T and run on the doubled batch,
    without one they run the dense two-direction kernels.  Eval mode: out, rates and every spike train bit-equal.  A
    training step: the spikes equal, out, loss, rates, every gradient and the running statistics to the bars that
    tests/test_bidir_ragged_gpu.py holds lengths = T against the plain path with (out 1e-4, rates 1e-6, loss 1e-5,
    gradients 5e-4 of max-abs, statistics rtol 1e-4 / atol 1e-6)."""
    seed = sc.SEEDS[c]
    x, _, _, init, _ = sc.inputs(c, seed)
    order = [st[k] for st in init for k in ("u0", "w0", "s0") if k in st]

    def zeroed():
        net = sc.make_net(sp, c)
        with torch.no_grad():
            for lay in net.snn[:-1]:
                lay.gamma.zero_()
        return net

    out_p, rates_p, rec_p = whole_forward(sc.make_net(sp, c, synapse=None).to(DEV).eval(), x.to(DEV), order)
    out_z, rates_z, rec_z = whole_forward(zeroed().to(DEV).eval(), x.to(DEV), order)
    assert same_bits(out_z, out_p) and same_bits(rates_z, rates_p) and sorted(rec_z) == sorted(rec_p) == [0, 1]
    for k in rec_p:
        assert torch.equal(rec_z[k], rec_p[k]), k
    plain = sc.device_run(sp, c, seed, net=sc.make_net(sp, c, synapse=None))
    zero = sc.device_run(sp, c, seed, net=zeroed())
    assert_alive(plain["rates"], c)
    for k in plain["spikes"]:
        assert float(plain["spikes"][k].sum()) > 0 and torch.equal(zero["spikes"][k], plain["spikes"][k]), k
    assert relmax(N(zero["out"]), N(plain["out"])) <= OUT_CAP and relmax(N(zero["rates"]), N(plain["rates"])) <= 1e-6
    lz, lp = float(zero["loss"].detach()), float(plain["loss"].detach())
    assert abs(lz - lp) <= LOSS_CAP * max(1.0, abs(lp))
    grads = dict(zero["net"].named_parameters())
    for name, p in plain["net"].named_parameters():
        assert p.grad is not None and bool(p.grad.any()), name
        e = relmax(N(grads[name].grad), N(p.grad))
        print(f"  {name}: {e:.3e}")
        assert e <= GRAD_CAP, (name, e)
    sz = zero["net"].state_dict()
    for k, v in plain["net"].state_dict().items():
        if "running" in k:
            np.testing.assert_allclose(N(sz[k]), N(v), rtol=1e-4, atol=1e-6, err_msg=k)
        elif "num_batches" in k:
            assert int(sz[k]) == int(v), k


@pytest.mark.parametrize("c", [sc.CASES[0], sc.CASES[9]], ids=sc.case_id)
def test_a_fixed_synapse_against_the_layer_oracle(sp, c):
    """learn_synapse=False under BatchNorm (the backward variant that adds the column sums without reading i): every
    other gradient against the oracle, to the same bars; gamma gets none."""
    seed = sc.SEEDS[c]
    _, _, r64, _ = sc.runs(c, seed)
    got = sc.device_run(sp, c, seed, net=sc.make_net(sp, c, learn_synapse=False))
    for k, s in got["spikes"].items():
        assert torch.equal(s.cpu().double(), r64["spikes"][k]), k
    named = dict(got["net"].named_parameters())
    for name, ref in r64["grads"].items():
        if name.endswith("gamma"):
            assert named[name].grad is None, name
            continue
        within(N(named[name].grad), ref.numpy(), GRAD_CAP * float(ref.abs().max()), name)


@pytest.mark.parametrize("c", sc.CASES, ids=sc.case_id)
def test_a_network_against_the_layer_oracle(sp, c):
    seed = sc.SEEDS[c]
    _, _, r64, _ = sc.runs(c, seed)
    got = sc.device_run(sp, c, seed)
    assert_alive(got["rates"], c)
    assert sorted(got["spikes"]) == [0, 1]
    for k, s in got["spikes"].items():
        assert float(s.sum()) > 0 and torch.equal(s.cpu().double(), r64["spikes"][k]), k
    top = float(r64["out"].abs().max())
    within(N(got["out"]), r64["out"].numpy(), OUT_CAP * top, "out")
    within(N(got["loss"]), r64["loss"].numpy(), LOSS_CAP * max(1.0, abs(float(r64["loss"]))), "loss")
    named = dict(got["net"].named_parameters())
    assert sum(k.endswith("gamma") for k in r64["grads"]) == 2
    for name, ref in r64["grads"].items():
        assert bool(ref.any()), name
        within(N(named[name].grad), ref.numpy(), GRAD_CAP * float(ref.abs().max()), name)


@pytest.mark.parametrize("c", [c for c in sc.CASES if c[3] and not c[2]], ids=sc.case_id)
def test_with_lengths_a_row_is_its_clip_run_alone_and_pack_equals_lengths(sp, c):
    """Eval mode: row b of net(x, lengths) equals net(x[b:b+1, :L_b]) with the same state rows, and pack=True gives the
    masked mode's out and rates bit for bit; train mode: pack=True to GRAD_CAP of the masked step's gradients."""
    seed = sc.SEEDS[c]
    x, y, cot, init, L = sc.inputs(c, seed)
    net = sc.make_net(sp, c).to(DEV).eval()
    xd = x.to(DEV)
    with torch.no_grad():
        with sc.dc.injected_states(init):
            out, rates = net(xd, lengths=torch.tensor(L))
        with sc.dc.injected_states(init):
            out_pk, rates_pk = net(xd, lengths=torch.tensor(L), pack=True)
        assert torch.equal(out, out_pk) and torch.equal(rates, rates_pk)
        for b, m in enumerate(L):
            with sc.dc.injected_states(init, slice(b, b + 1)):
                alone, _ = net(xd[b:b + 1, :m].contiguous())
            assert torch.equal(out[b:b + 1], alone), (b, m)
    masked = sc.device_run(sp, c, seed)
    packed = sc.device_run(sp, c, seed, pack=True)
    assert relmax(N(packed["out"]), N(masked["out"])) <= OUT_CAP
    got = dict(packed["net"].named_parameters())
    for name, p in masked["net"].named_parameters():
        assert p.grad is not None and bool(p.grad.any()), name
        e = relmax(N(got[name].grad), N(p.grad))
        print(f"  {name}: {e:.3e}")
        assert e <= GRAD_CAP, (name, e)
    _Fn().check_status()


@pytest.mark.parametrize("c", [sc.CASES[0], sc.CASES[4], sc.CASES[6], sc.CASES[12]], ids=sc.case_id)
def test_streaming_in_chunks_gives_the_whole_sequence_spikes(sp, c):
    seed = sc.SEEDS[c]
    x, _, _, init, _ = sc.inputs(c, seed)
    net = sc.make_net(sp, c).to(DEV).eval()
    x = x.to(DEV)
    order = [st[k] for st in init for k in ("u0", "w0", "s0") if k in st]
    out_w, rates_w, rec_w = whole_forward(net, x, order)
    st = sp.StreamingSNN(net, sc.NB)
    st.reset(states=init)
    outs, rec = run_stream(st, x, [1, 2, 5, 1, 3])
    _Fn().check_status()
    assert sorted(rec) == sorted(rec_w) == [0, 1]
    for k in rec:
        assert float(rec_w[k].sum()) > 0 and torch.equal(rec[k], rec_w[k]), k
    assert torch.equal(st.firing_rates(), rates_w)
    assert relmax(N(outs[-1]), N(out_w)) <= 2e-5
    state = st.get_state()
    assert all("i" in s and tuple(s["i"].shape) == (sc.NB, c[6][k]) and bool(s["i"].any()) for k, s in enumerate(state[:-1]))
    assert "i" not in state[-1]
    st.reset(states=[{k: v[1:2] for k, v in s.items()} for s in init], rows=[1])
    after = st.get_state()
    assert not after[0]["i"][1].any() and torch.equal(after[0]["i"][[0, 2]], state[0]["i"][[0, 2]])
    st.set_state(state)                                     # "i" round-trips
    assert all(torch.equal(a["i"], b["i"]) for a, b in zip(st.get_state()[:-1], state[:-1]))
    if c[1] != "layernorm":                                 # (LayerNorm: fused=True is refused for that already)
        for kw in (dict(fused=True), dict(fused=True, sparse=True), dict(graph=True)):
            with pytest.raises(ValueError, match="synaptic currents"):
                sp.StreamingSNN(net, sc.NB, **kw)


@pytest.mark.parametrize("c", [sc.CASES[3], sc.CASES[11]], ids=sc.case_id)
def test_one_adam_step_moves_gamma(sp, c):
    from sparch_amd import optim
    seed = sc.SEEDS[c]
    net = sc.make_net(sp, c).to(DEV)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    opt = optim.Adam(net.parameters(), 1e-2)
    sc.device_run(sp, c, seed, net=net)
    opt.step()
    for name, p in net.named_parameters():
        assert bool(torch.isfinite(p).all()), name
        if name.endswith("gamma"):                          # moved exactly where it has a gradient: not column 0, which
            moved = p.detach() != before[name]                # sits above hi, nor a neuron no gradient reaches
            assert torch.equal(moved, p.grad != 0) and bool(moved[1:].any()) and not bool(moved[0]), name
    fixed = sc.make_net(sp, c, learn_synapse=False)
    sc.device_run(sp, c, seed, net=fixed)
    for name, p in fixed.named_parameters():
        assert (p.grad is None) == name.endswith("gamma"), name


# ------------------------------------------------------------------------------------------------ the command line
def test_run_exp_trains_with_sparch_synapse(tmp_path):
    """run_exp.py --synthetic 1 with SPARCH_SYNAPSE=0:0.9 on a tiny shape, in a child process: two epochs, a finite
    loss, and every epoch logs each layer's mean and largest clamped gamma."""
    exp = tmp_path / "exp"
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPARCH_")}
    env["SPARCH_SYNAPSE"] = "0:0.9"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "run_exp.py"), "--model_type", "adLIF", "--dataset_name", "shd",
                          "--synthetic", "1", "--synthetic_batches", "2", "--seq_len", "20", "--nb_epochs", "2",
                          "--nb_layers", "3", "--nb_hiddens", "32", "--batch_size", "8", "--log_tofile", "1",
                          "--new_exp_folder", str(exp)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    text = (exp / "log" / "exp.log").read_text()
    assert "Synaptic currents: decay in [0, 0.9], init uniform, learnable, all layers (SPARCH_SYNAPSE)" in text
    for e in (1, 2):
        for layer in range(2):
            assert f"Epoch {e}: layer {layer} synapse: mean gamma=" in text, (e, layer)
    losses = [float(ln.split("train loss=")[1]) for ln in text.splitlines() if "train loss=" in ln]
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses) and "nan" not in text.lower()
