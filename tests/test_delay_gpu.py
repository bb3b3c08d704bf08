"""
Axonal delays on the device ("Axonal delays"), against the fp64 restatement tests/delay_numpy.py.

Kernels (sparch_delay_fwd / _bwd / _stream through functional.delay_forward / delay_backward / delay_stream): B = 3,
T = 9, K in {5, 8, 36}, D in {1, 4, 11}, 2- and 4-byte elements; dense, lengths = [9, 1, 4] and packed through
snns.prepare_packing; a non-contiguous row stride.  y and g_x are copies: bit-equal.  g_theta is an fp32 sum of at most
B T products, each of a rounded difference: within (B T + 2) 2^-24 sum |g_y dx| of fp64, bit-equal across two runs,
exactly 0 where the gate is 0.  The stream kernel in chunks of 1, 2 and 5 steps equals the whole-sequence gather.

Networks (all four kinds, 8 -> 12 -> 12 -> 5 and a recurrent width of 10, B = 3, T = 12, D = 3, dyadic weights scaled as
in tests/network_cases.py, data seeds picked by the CPU restatement in tests/delay_cases.py): every hidden layer fires
inside [0.02, 0.6] (asserted on the device's own rates);  delay = 0 is the network without delays, bit for bit, out,
rates and every gradient;  a delayed layer is the layer run alone on its host-shifted input, forward and every
parameter gradient, also bidirectional;  with lengths each clip run alone is its row of the batch;  pack=True equals
lengths (eval: bit-equal, as tests/test_packed_gpu.py holds it; train: gradients to its 5e-4);  a StreamingSNN fed in
chunks gives the whole-sequence spikes;  one Adam step moves the delays;  run_exp.py trains two epochs under
SPARCH_DELAYS=4:uniform.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import snn_oracle as orc
from tests import delay_cases as dc
from tests import delay_numpy as dn
from tests import packed_numpy as pn
from tests.kit import DEV, F32, F64, N, relmax, same_bits, within
from tests.kit import Fn as _Fn
from tests.kit import sp  # noqa: F401  (a fixture)
from tests.stream_cases import run_stream, whole_forward

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, T = dc.B, dc.T
DTYPES = {"bf16": torch.bfloat16, "f32": torch.float32}


def plan_of(lengths, T_):
    from sparch_amd import snns
    return snns.prepare_packing(torch.as_tensor(np.asarray(lengths)), len(lengths), T_, DEV)


def dev_lengths(lengths):
    return torch.from_numpy(np.asarray(lengths).astype(np.int32)).to(DEV), int(np.sum(lengths))


def as_dtype(a, dtype):
    """A host fp32 array on the device in `dtype` (0/1 and small integers are exact in bf16)."""
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(DEV).to(dtype)


def values(t):
    """A device tensor's values as a host fp32 array."""
    return N(t, torch.float32)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("layout", ["dense", "lengths", "packed"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("D", dc.CAPS)
@pytest.mark.parametrize("K", dc.WIDTHS)
def test_gather_kernels_are_copies_of_the_oracle(K, D, dtype, layout):
    Fn = _Fn()
    x, g, th = dc.kernel_data(K, D)
    lengths = None if layout == "dense" else dc.LENGTHS
    d = dn.steps(th, D)
    assert d[0] == 0 and (d == D).any() and ((th < 0) | (th > D)).any()
    if D > T:
        assert (d >= T).any()
    theta = torch.from_numpy(th).to(DEV)
    y_ref, gx_ref = dn.forward(x, th, D, lengths), dn.backward_x(g, th, D, lengths)
    if D > T:
        assert not y_ref[:, :, d >= T].any() and y_ref.any()
    dirty = g.copy()                                      # what g_y holds on padded steps is ignored
    if lengths is not None:
        dirty[~pn.valid_mask(lengths, T)] = np.nan
    if layout == "packed":
        plan = plan_of(lengths, T)
        xd = as_dtype(pn.pack(x, lengths), DTYPES[dtype]).unsqueeze(0)
        y = Fn.delay_forward(xd, theta, D, pack=plan)
        assert y.shape == xd.shape and y.dtype == xd.dtype
        assert same_bits(values(y)[0], pn.pack(y_ref, lengths))
        gx, _ = Fn.delay_backward(as_dtype(pn.pack(g, lengths), torch.float32).unsqueeze(0), theta, D, pack=plan,
                                  need_gdelay=False)
        assert same_bits(values(gx)[0], pn.pack(gx_ref, lengths))
        return
    kw = {} if lengths is None else {"lengths": dev_lengths(lengths)}
    xd = as_dtype(x, DTYPES[dtype])
    poison = torch.full((B, T, K), float("nan"), dtype=xd.dtype, device=DEV)        # every element is written
    y = Fn.delay_forward(xd, theta, D, out=poison, **kw)
    assert y is poison and same_bits(values(y), y_ref.astype(F32))
    gx, none = Fn.delay_backward(as_dtype(dirty, torch.float32), theta, D, need_gdelay=False, **kw)
    assert none is None and same_bits(values(gx), gx_ref)


@pytest.mark.parametrize("ld", [11, 16])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_gather_kernels_take_a_row_stride(dtype, ld):
    """K = 8 columns of rows ld elements apart, read and written where they lie: ld = 16 keeps the 16-byte pieces, ld = 11
    takes single elements; the columns behind K stay as they were."""
    Fn = _Fn()
    K, D = 8, 4
    x, g, th = dc.kernel_data(K, D)
    theta = torch.from_numpy(th).to(DEV)
    wide = torch.full((B, T, ld), 7.0, dtype=DTYPES[dtype], device=DEV)
    wide[:, :, :K] = as_dtype(x, DTYPES[dtype])
    out = torch.full((B, T, ld), 5.0, dtype=DTYPES[dtype], device=DEV)
    y = Fn.delay_forward(wide[:, :, :K], theta, D, out=out[:, :, :K])
    assert y.data_ptr() == out.data_ptr()
    assert same_bits(values(out[:, :, :K]), dn.forward(x, th, D)) and bool((out[:, :, K:] == 5.0).all())
    gw = torch.full((B, T, ld), float("nan"), dtype=torch.float32, device=DEV)
    gw[:, :, :K] = torch.from_numpy(g).to(DEV)
    gx, gth = Fn.delay_backward(gw[:, :, :K], theta, D, x=wide[:, :, :K], lengths=dev_lengths(dc.LENGTHS))
    assert same_bits(values(gx), dn.backward_x(g, th, D, dc.LENGTHS))
    ref, mag = dn.backward_theta(g, x, th, D, dc.LENGTHS)
    within(values(gth), ref, (B * T + 2) * 2.0 ** -24 * mag, "g_theta, strided rows")


@pytest.mark.parametrize("layout", ["dense", "lengths", "packed"])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("D", dc.CAPS)
@pytest.mark.parametrize("K", dc.WIDTHS)
def test_delay_gradient_against_fp64(K, D, dtype, layout):
    Fn = _Fn()
    x, g, th = dc.kernel_data(K, D)
    lengths = None if layout == "dense" else dc.LENGTHS
    scale = 1.25 if dtype == "bf16" else 1.0            # a spike plane travels with its dropout scale 1 / (1 - p)
    d, gate = dn.steps(th, D), dn.gate(th, D)
    ref, mag = dn.backward_theta(g, x.astype(F64) * scale, th, D, lengths)
    if layout == "dense":                               # Bernoulli(0.3): every column that can has something to sum
        assert (mag[d < T - 1] > 0).all() and (gate == 0).any() and (ref != 0).any()
    theta = torch.from_numpy(th).to(DEV)
    if layout == "packed":
        kw = {"pack": plan_of(lengths, T)}
        gd = torch.from_numpy(pn.pack(g, lengths)).to(DEV).unsqueeze(0)
        xd = as_dtype(pn.pack(x, lengths), DTYPES[dtype]).unsqueeze(0)
    else:
        kw = {} if lengths is None else {"lengths": dev_lengths(lengths)}
        dirty = g.copy()
        if lengths is not None:
            dirty[~pn.valid_mask(lengths, T)] = np.nan
        gd, xd = torch.from_numpy(dirty).to(DEV), as_dtype(x, DTYPES[dtype])
    runs = [values(Fn.delay_backward(gd, theta, D, x=xd, x_scale=scale, need_gx=False, **kw)[1]) for _ in range(2)]
    print(f"  K={K} D={D} {dtype} {layout}: max |g_theta| {np.abs(ref).max():.3e}, max |error| "
          f"{np.abs(runs[0] - ref).max():.3e}")
    assert same_bits(runs[0], runs[1])                  # no atomics: the same bits on every run
    assert same_bits(runs[0][gate == 0], np.zeros(int((gate == 0).sum()), F32))
    within(runs[0], ref, (B * T + 2) * 2.0 ** -24 * mag, "g_theta")


@pytest.mark.parametrize("chunk", [1, 2, 5])
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("D", dc.CAPS)
@pytest.mark.parametrize("K", dc.WIDTHS)
def test_stream_kernel_equals_the_whole_sequence_gather(K, D, dtype, chunk):
    Fn = _Fn()
    x, _, th = dc.kernel_data(K, D)
    theta = torch.from_numpy(th).to(DEV)
    xd = as_dtype(x, DTYPES[dtype])
    whole = Fn.delay_forward(xd, theta, D)
    assert same_bits(values(whole), dn.forward(x, th, D))
    hist = torch.zeros(B, D, K, dtype=xd.dtype, device=DEV)
    got, t0 = [], 0
    while t0 < T:
        n = min(chunk, T - t0)
        got.append(Fn.delay_stream(xd[:, t0:t0 + n], theta, D, hist))
        t0 += n
    assert same_bits(torch.cat(got, 1), whole)
    last = np.concatenate([np.zeros((B, D, K), F32), x], axis=1)[:, -D:]              # the last D input steps
    assert same_bits(values(hist), last)


@pytest.mark.parametrize("layout", ["dense", "lengths", "packed"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_kernels_over_several_tiles_and_slabs(dtype, layout):
    """T = 150 > 64 + D, K = 136 (tests/delay_cases.py): the staged gather runs three time tiles — a tile's source rows
    reach back over the tile before it, and forward over the next one in g_x — and five (fp32) or three (bf16) column
    tiles with a partial last one; the delay's gradient sums 15 slabs (packed: fewer rows, the same slabs' layout).  y
    and g_x bit-equal to the restatement, g_theta within (B T + 2) 2^-24 sum |g_y dx| of fp64 and bit-equal across
    two runs."""
    Fn = _Fn()
    Tb, K, D = dc.BIG_T, dc.BIG_K, dc.BIG_D
    x, g, th = dc.big_kernel_data()
    lengths = None if layout == "dense" else dc.BIG_LENGTHS
    scale = 1.25 if dtype == "bf16" else 1.0
    theta = torch.from_numpy(th).to(DEV)
    gate = dn.gate(th, D)
    y_ref, gx_ref = dn.forward(x, th, D, lengths), dn.backward_x(g, th, D, lengths)
    ref, mag = dn.backward_theta(g, x.astype(F64) * scale, th, D, lengths)
    assert y_ref[:, 64:].any() and gx_ref[:, :64].any() and (ref != 0).any() and (gate == 0).any()
    if layout == "packed":
        kw = {"pack": plan_of(lengths, Tb)}
        xd = as_dtype(pn.pack(x, lengths), DTYPES[dtype]).unsqueeze(0)
        gd = torch.from_numpy(pn.pack(g, lengths)).to(DEV).unsqueeze(0)
        y_ref, gx_ref = pn.pack(y_ref, lengths)[None], pn.pack(gx_ref, lengths)[None]
    else:
        kw = {} if lengths is None else {"lengths": dev_lengths(lengths)}
        dirty = g.copy()
        if lengths is not None:
            dirty[~pn.valid_mask(lengths, Tb)] = np.nan
        xd, gd = as_dtype(x, DTYPES[dtype]), torch.from_numpy(dirty).to(DEV)
    poison = torch.full(tuple(xd.shape), float("nan"), dtype=xd.dtype, device=DEV)
    y = Fn.delay_forward(xd, theta, D, out=poison, **kw)
    assert same_bits(values(y), y_ref.astype(F32))
    runs = [Fn.delay_backward(gd, theta, D, x=xd, x_scale=scale, **kw) for _ in range(2)]
    assert same_bits(values(runs[0][0]), gx_ref)
    gth = [values(r[1]) for r in runs]
    print(f"  {dtype} {layout}: max |g_theta| {np.abs(ref).max():.3e}, max |error| {np.abs(gth[0] - ref).max():.3e}")
    assert same_bits(gth[0], gth[1]) and same_bits(gth[0][gate == 0], np.zeros(int((gate == 0).sum()), F32))
    within(gth[0], ref, (B * Tb + 2) * 2.0 ** -24 * mag, "g_theta")
    with pytest.raises(ValueError, match="delays"):                     # a delay vector of another size is refused
        Fn.delay_backward(gd, theta[:-1], D, x=xd, **kw)
    with pytest.raises(ValueError, match="delays"):
        Fn.delay_stream(xd[:, :2], theta[:-1], D, torch.zeros(xd.shape[0], D, K, dtype=xd.dtype, device=DEV))


# ------------------------------------------------------------------------------------------------ networks
NETS = [(kind, dc.SIZES, False) for kind in dc.KINDS] + [("RLIF", dc.ODD_SIZES, False), ("RadLIF", dc.ODD_SIZES, False),
                                                          ("adLIF", dc.SIZES, True), ("RadLIF", dc.SIZES, True)]
net_ids = [f"{k}-{'x'.join(map(str, s))}-{'2dir' if b else '1dir'}" for k, s, b in NETS]


def layer_rates(rates, sizes, bidir):
    """The per-neuron firing rates of a forward -> one mean per hidden layer."""
    r, out, at = values(rates), [], 0
    for H in sizes[:-1]:
        n = H * (2 if bidir else 1)
        out.append(float(r[at:at + n].mean()))
        at += n
    assert at == r.size
    return out


def assert_alive(rates, sizes, bidir):
    per_layer = layer_rates(rates, sizes, bidir)
    print(f"  firing rates per hidden layer: {per_layer}")
    assert dc.in_window(per_layer), per_layer


def train_step(net, x, y, init, **kw):
    net.zero_grad()
    with dc.injected_states(init):
        out, rates = net(x, **kw)
        loss = orc.train_step_loss(out, rates, y, use_regularizers=True)
        loss.backward()
    _Fn().check_status()
    return out, rates, loss


@pytest.mark.parametrize("kind,sizes,bidir", NETS, ids=net_ids)
def test_zero_delays_are_the_network_without_delays_bit_for_bit(sp, kind, sizes, bidir):
    x, y, init = dc.net_inputs(kind, sizes, bidir, dc.seed_of(kind, sizes, bidir))
    x, y = x.to(DEV), y.to(DEV)
    plain = dc.make_net(sp, kind, sizes, bidir).to(DEV).train()
    zero = dc.make_net(sp, kind, sizes, bidir, max_delay=dc.ND).to(DEV).train()
    out_p, rates_p, loss_p = train_step(plain, x, y, init)
    out_z, rates_z, loss_z = train_step(zero, x, y, init)
    assert_alive(rates_p, sizes, bidir)
    assert same_bits(out_z, out_p) and same_bits(rates_z, rates_p) and same_bits(loss_z, loss_p)
    grads = dict(zero.named_parameters())
    for name, p in plain.named_parameters():
        assert p.grad is not None and bool(p.grad.any()), name
        assert same_bits(grads[name].grad, p.grad), name
    for i in range(3):                                                  # the delays themselves have a gradient
        gd = grads[f"snn.{i}.delay"].grad
        assert gd is not None and bool(torch.isfinite(gd).all()) and bool(gd.any()), i


@pytest.mark.parametrize("kind,sizes,bidir", NETS, ids=net_ids)
def test_a_delayed_layer_is_the_layer_alone_on_the_host_shifted_input(sp, kind, sizes, bidir):
    """Layer by layer: the delayed layer on its input against its twin without delays on the input shifted on the
    host (tests/delay_numpy.py), same states, same cotangent: spikes, rates and every parameter gradient bit for bit.
    Behind a layer of ours both read the bf16 plane of a tagged spike train."""
    from sparch_amd import snns
    x, _, init = dc.net_inputs(kind, sizes, bidir, dc.seed_of(kind, sizes, bidir))
    net = dc.make_net(sp, kind, sizes, bidir, max_delay=dc.ND).to(DEV).train()
    plain = dc.make_net(sp, kind, sizes, bidir).to(DEV).train()
    delays = dc.net_delays(net)
    dc.set_delays(net, {i: th.to(DEV) for i, th in delays.items()})
    g = torch.Generator().manual_seed(17)
    a, rates = x.to(DEV), []
    for k in range(3):
        lay_d, lay_p = net.snn[k], plain.snn[k]
        shifted = torch.from_numpy(dn.forward(values(a), delays[k].numpy(), dc.ND)).to(DEV)
        a_in = a.clone()
        if k > 0:
            assert set(np.unique(values(a))) <= {0.0, 1.0} and float(a.sum()) > 0 and not torch.equal(shifted, a)
            snns._tag_spikes(a_in, 1.0, a_in.to(torch.bfloat16))
            snns._tag_spikes(shifted, 1.0, shifted.to(torch.bfloat16))
        st = init[k]
        if k < 2:
            states = tuple(st[n].to(DEV) if n in st else None for n in ("u0", "w0", "s0"))
            s_d, r_d = lay_d.forward_with_rate(a_in, states=states)
            s_p, r_p = lay_p.forward_with_rate(shifted, states=states)
            cot = torch.randn(s_p.shape, generator=g).to(DEV)
            cot_r = torch.randn(r_p.shape, generator=g).to(DEV)
            ((s_d * cot).sum() + (r_d * cot_r).sum()).backward()
            ((s_p * cot).sum() + (r_p * cot_r).sum()).backward()
            assert same_bits(s_d.detach(), s_p.detach()) and same_bits(r_d.detach(), r_p.detach())
            rates.append(r_p.detach())
            a = s_p.detach()
        else:
            out_d = lay_d(a_in, u0=st["u0"].to(DEV))
            out_p = lay_p(shifted, u0=st["u0"].to(DEV))
            cot = torch.randn(out_p.shape, generator=g).to(DEV)
            (out_d * cot).sum().backward()
            (out_p * cot).sum().backward()
            assert same_bits(out_d.detach(), out_p.detach())
        got = dict(lay_d.named_parameters())
        for name, p in lay_p.named_parameters():
            assert p.grad is not None and bool(p.grad.any()), (k, name)
            assert same_bits(got[name].grad, p.grad), (k, name)
        assert got["delay"].grad is not None and bool(torch.isfinite(got["delay"].grad).all())
    _Fn().check_status()
    assert_alive(torch.cat(rates), sizes, bidir)


@pytest.mark.parametrize("kind", dc.KINDS)
def test_the_delay_gradient_of_a_layer_reads_the_scaled_spike_train(sp, kind):
    """The second layer fed by a spike train that travels as a bf16 0/1 plane with the scale 1.25 (what dropout 0.2
    gives): its `delay.grad` against the restatement on the VALUES plane x 1.25 and the gradient that reaches the
    delayed input (read off the twin without delays, run on the host-shifted input), to the kernel tests' bound."""
    from sparch_amd import snns
    scale = 1.25
    x, _, init = dc.net_inputs(kind, seed=dc.seed_of(kind))
    net = dc.make_net(sp, kind, max_delay=dc.ND).to(DEV).train()
    plain = dc.make_net(sp, kind).to(DEV).train()
    delays = dc.net_delays(net)
    dc.set_delays(net, {i: th.to(DEV) for i, th in delays.items()})
    state = lambda k: tuple(init[k][n].to(DEV) if n in init[k] else None for n in ("u0", "w0", "s0"))  # noqa: E731
    with torch.no_grad():
        spikes, _ = plain.snn[0].forward_with_rate(x.to(DEV), states=state(0))
    a = values(spikes)
    assert set(np.unique(a)) == {0.0, 1.0}
    th = delays[1].numpy()
    a_in = torch.from_numpy(a * F32(scale)).to(DEV)
    snns._tag_spikes(a_in, scale, torch.from_numpy(a).to(DEV).to(torch.bfloat16))
    shifted01 = dn.forward(a, th, dc.ND)
    shifted = torch.from_numpy(shifted01 * F32(scale)).to(DEV).requires_grad_(True)
    snns._tag_spikes(shifted, scale, torch.from_numpy(shifted01).to(DEV).to(torch.bfloat16))
    s_d, r_d = net.snn[1].forward_with_rate(a_in, states=state(1))
    s_p, r_p = plain.snn[1].forward_with_rate(shifted, states=state(1))
    assert same_bits(s_d.detach(), s_p.detach()) and float(s_p.detach().sum()) > 0
    g = torch.Generator().manual_seed(23)
    cot, cot_r = torch.randn(s_p.shape, generator=g).to(DEV), torch.randn(r_p.shape, generator=g).to(DEV)
    ((s_d * cot).sum() + (r_d * cot_r).sum()).backward()
    ((s_p * cot).sum() + (r_p * cot_r).sum()).backward()
    _Fn().check_status()
    g_y = values(shifted.grad)
    ref, mag = dn.backward_theta(g_y, a.astype(F64) * scale, th, dc.ND)
    assert (ref != 0).any() and (dn.gate(th, dc.ND) == 0).any()
    wrong, _ = dn.backward_theta(g_y, a, th, dc.ND)                      # without the scale: outside the bound
    bound = (dc.NB * dc.NT + 2) * 2.0 ** -24 * mag
    assert (np.abs(wrong - ref) > 4 * bound).any()
    within(values(net.snn[1].delay.grad), ref, bound, "delay.grad of layer 1")


@pytest.mark.parametrize("kind", dc.KINDS)
def test_with_lengths_a_row_is_its_clip_run_alone_and_pack_equals_lengths(sp, kind):
    """Eval mode, dyadic data (the invariant of tests/test_ragged_gpu.py and the bars of tests/test_packed_gpu.py): row b
    of net(x, lengths) equals net(x[b:b+1, :L_b]) with the same state rows, and pack=True gives the masked mode's
    out and rates bit for bit."""
    lengths = dc.NET_LENGTHS
    x, _, init = dc.net_inputs(kind, seed=dc.seed_of(kind))
    x = (x * torch.from_numpy(pn.valid_mask(lengths, dc.NT))[:, :, None]).to(DEV)
    net = dc.make_net(sp, kind, max_delay=dc.ND).to(DEV).eval()
    dc.set_delays(net, {i: th.to(DEV) for i, th in dc.net_delays(net).items()})
    with torch.no_grad():
        with dc.injected_states(init):
            out, rates = net(x, lengths=torch.tensor(lengths))
        with dc.injected_states(init):
            out_pk, rates_pk = net(x, lengths=torch.tensor(lengths), pack=True)
        assert torch.equal(out, out_pk) and torch.equal(rates, rates_pk)
        for b, m in enumerate(lengths):
            with dc.injected_states(init, slice(b, b + 1)):
                alone, _ = net(x[b:b + 1, :m].contiguous())
            assert torch.equal(out[b:b + 1], alone), (b, m)
        with dc.injected_states(init):
            out_full, rates_full = net(x)                   # without lengths the padded steps count: another result
    assert not torch.equal(out_full, out)
    assert_alive(rates, dc.SIZES, False)                    # (means over the valid steps; restated in tests/delay_cases.py)
    _Fn().check_status()


@pytest.mark.parametrize("kind", dc.KINDS)
def test_packed_training_step_equals_the_masked_one(sp, kind):
    """Train mode: out, rates and loss of pack=True against lengths, and every gradient, the delays' included, to the
    5e-4 of max-abs that tests/test_packed_gpu.py holds the packed gradients to."""
    lengths = dc.NET_LENGTHS
    x, y, init = dc.net_inputs(kind, seed=dc.seed_of(kind))
    x, y = (x * torch.from_numpy(pn.valid_mask(lengths, dc.NT))[:, :, None]).to(DEV), y.to(DEV)
    nets = []
    for _ in range(2):
        net = dc.make_net(sp, kind, max_delay=dc.ND).to(DEV).train()
        dc.set_delays(net, {i: th.to(DEV) for i, th in dc.net_delays(net).items()})
        nets.append(net)
    out_m, rates_m, loss_m = train_step(nets[0], x, y, init, lengths=torch.tensor(lengths))
    out_p, rates_p, loss_p = train_step(nets[1], x, y, init, lengths=torch.tensor(lengths), pack=True)
    assert_alive(rates_m, dc.SIZES, False)
    assert relmax(values(out_p), values(out_m)) <= 1e-4 and relmax(values(rates_p), values(rates_m)) <= 1e-6
    lp, lm = float(loss_p.detach()), float(loss_m.detach())
    assert abs(lp - lm) <= 1e-5 * max(1.0, abs(lm))
    packed = dict(nets[1].named_parameters())
    for name, p in nets[0].named_parameters():
        assert p.grad is not None and bool(p.grad.any()), name
        e = relmax(values(packed[name].grad), values(p.grad))
        print(f"  {name}: {e:.3e}")
        assert e <= 5e-4, (name, e)


@pytest.mark.parametrize("counts", [False, True], ids=["float", "uint8"])
@pytest.mark.parametrize("kind,sizes", [(k, dc.SIZES) for k in dc.KINDS] + [("RadLIF", dc.ODD_SIZES)])
def test_streaming_in_chunks_gives_the_whole_sequence_spikes(sp, kind, sizes, counts):
    x, _, init = dc.net_inputs(kind, sizes, seed=dc.seed_of(kind, sizes))
    net = dc.make_net(sp, kind, sizes, max_delay=dc.ND).to(DEV).eval()
    dc.set_delays(net, {i: th.to(DEV) for i, th in dc.net_delays(net).items()})
    x = x.to(DEV)
    order = [st[k] for st in init for k in ("u0", "w0", "s0") if k in st]
    out_w, rates_w, rec_w = whole_forward(net, x, order)
    assert_alive(rates_w, sizes, False)
    st = sp.StreamingSNN(net, dc.NB)
    st.reset(states=init)
    outs, rec = run_stream(st, x.to(torch.uint8) if counts else x, [1, 2, 5, 1, 3])
    _Fn().check_status()
    assert sorted(rec) == sorted(rec_w) == [0, 1]
    for k in rec:
        assert float(rec_w[k].sum()) > 0 and torch.equal(rec[k], rec_w[k]), k
    assert torch.equal(st.firing_rates(), rates_w)
    assert relmax(values(outs[-1]), values(out_w)) <= 2e-5
    state = st.get_state()
    assert all("hist" in s and s["hist"].shape[1] == dc.ND for s in state)
    assert same_bits(values(state[0]["hist"]), values(x[:, -dc.ND:]))                   # the last D input steps
    st.reset(states=[{k: v[1:2] for k, v in s.items()} for s in init], rows=[1])
    after = st.get_state()
    assert not after[0]["hist"][1].any() and torch.equal(after[0]["hist"][[0, 2]], state[0]["hist"][[0, 2]])


@pytest.mark.parametrize("kind", dc.KINDS)
def test_one_adam_step_moves_the_delays(sp, kind):
    from sparch_amd import optim
    x, y, init = dc.net_inputs(kind, seed=dc.seed_of(kind))
    x, y = x.to(DEV), y.to(DEV)
    net = dc.make_net(sp, kind, max_delay=dc.ND, delay_init="uniform").to(DEV).train()
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    opt = optim.Adam(net.parameters(), 1e-2)
    out, rates, loss = train_step(net, x, y, init)
    assert_alive(rates, dc.SIZES, False)
    opt.step()
    for name, p in net.named_parameters():
        assert bool(torch.isfinite(p).all()), name
        if name.endswith("delay"):
            assert not torch.equal(p.detach(), before[name]), name
    # fixed delays stay where they are and get no gradient; everything else still trains
    fixed = dc.make_net(sp, kind, max_delay=dc.ND, delay_init="uniform", learn_delays=False).to(DEV).train()
    train_step(fixed, x, y, init)
    for name, p in fixed.named_parameters():
        assert (p.grad is None) == name.endswith("delay"), name


@pytest.mark.parametrize("what", ["per_step", "softmax_mean", "u_max", "u_mean", "u_last", "triangle", "fast_sigmoid", "atan",
                                  "bf16"])
def test_the_other_switches_run_with_delays(sp, what):
    """per_step, every other readout, every smooth surrogate and the bf16 operand mode: with zero delays each gives what
    the network without delays gives, bit for bit (the gather does not care), and with delays a finite result."""
    from sparch_amd import functional
    assert set(functional.READOUT_MODES) == {"softmax_sum", "softmax_mean", "u_max", "u_mean", "u_last"}
    assert set(functional.SURROGATES) == {"boxcar", "triangle", "fast_sigmoid", "atan"}   # (the defaults: every other test)
    Fn = _Fn()
    kind = "adLIF"
    kw = dict(readout=what) if what in functional.READOUT_MODES else dict(surrogate=what) if what in functional.SURROGATES else {}
    fw = dict(per_step="sum") if what == "per_step" else {}
    x, y, init = dc.net_inputs(kind, seed=dc.seed_of(kind))
    x, y = x.to(DEV), y.to(DEV)
    prev = Fn.set_compute_dtype("bf16") if what == "bf16" else None
    try:
        results = []
        for net_kw in ({}, dict(max_delay=dc.ND)):
            net = dc.make_net(sp, kind, **kw, **net_kw).to(DEV).train()
            with dc.injected_states(init):
                out, rates, *seq = net(x, **fw)
            loss = orc.train_step_loss(out, rates, y) + (seq[0].mean() if seq else 0.0)
            loss.backward()
            results.append((out, rates, seq, {n: p.grad for n, p in net.named_parameters()}))
        (out_p, rates_p, seq_p, g_p), (out_z, rates_z, seq_z, g_z) = results
        assert same_bits(out_z, out_p) and same_bits(rates_z, rates_p)
        assert_alive(rates_p, dc.SIZES, False)
        if seq_p:
            assert same_bits(seq_z[0], seq_p[0])
        for name, gp in g_p.items():
            assert same_bits(g_z[name], gp), name
        net = dc.make_net(sp, kind, max_delay=dc.ND, **kw).to(DEV).train()
        dc.set_delays(net, {i: th.to(DEV) for i, th in dc.net_delays(net).items()})
        with dc.injected_states(init):
            out, rates, *seq = net(x, **fw)
        (orc.train_step_loss(out, rates, y) + (seq[0].mean() if seq else 0.0)).backward()
        assert not same_bits(out, out_p)
        assert_alive(rates, dc.SIZES, False)
        for name, p in net.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        Fn.check_status()
    finally:
        if prev is not None:
            Fn.set_compute_dtype(prev)


# ------------------------------------------------------------------------------------------------ the command line
def test_run_exp_trains_with_sparch_delays(tmp_path):
    """run_exp.py --synthetic 1 with SPARCH_DELAYS=4:uniform on a tiny shape, in a child process: two epochs, a finite
    loss, and every epoch logs each delayed layer's mean and largest delay."""
    exp = tmp_path / "exp"
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPARCH_")}
    env["SPARCH_DELAYS"] = "4:uniform"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "run_exp.py"), "--model_type", "adLIF", "--dataset_name", "shd",
                          "--synthetic", "1", "--synthetic_batches", "2", "--seq_len", "20", "--nb_epochs", "2",
                          "--nb_layers", "3", "--nb_hiddens", "32", "--batch_size", "8", "--log_tofile", "1",
                          "--new_exp_folder", str(exp)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    text = (exp / "log" / "exp.log").read_text()
    assert "Axonal delays: up to 4 steps, init uniform, learnable, all layers (SPARCH_DELAYS)" in text
    for e in (1, 2):
        for layer in range(3):
            assert f"Epoch {e}: layer {layer} delays: mean d=" in text, (e, layer)
    losses = [float(ln.split("train loss=")[1]) for ln in text.splitlines() if "train loss=" in ln]
    assert len(losses) == 2 and all(np.isfinite(v) for v in losses) and "nan" not in text.lower()
