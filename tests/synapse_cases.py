"""
Cases of the synaptic-current tests ("Synaptic currents"): the kernels' shapes and parameters
(tests/test_synapse_gpu.py), and small whole networks with the layer-level oracle they are held to.

The oracle composes the reference-faithful pieces — oracle.snn_oracle's normalisation, spiking_cell and readout (with
lengths: tests/ragged_oracle.py's, bidirectional: the stacking of tests/bidir_ragged_oracle.py) — with the filter in
torch between the normalisation and the cell, so autograd gives every gradient, gamma's included.  Run in fp64 and in
fp32 it also decides, before anything runs on a GPU, whether a case can be held to exact spikes: the keep rule of
tests/network_cases.py (MARGIN, RATE_WINDOW).  SEEDS holds the first data seed at which each case is kept;
tests/test_synapse_numpy_host.py re-derives the verdicts.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import snn_oracle as orc
from tests import bidir_ragged_oracle as bro
from tests import delay_cases as dc
from tests import ragged_oracle as rag
from tests.kit import DEV, F32
from tests.network_cases import MARGIN, RATE_WINDOW

# ------------------------------------------------------------------------------------------------ kernels
B, T = 3, 9
WIDTHS = (5, 8, 36)             # odd; two 16-byte pieces; nine of them
LENGTHS = [9, 1, 4]
LIMITS = ((0.0, 0.9), (0.25, 0.875))
# 66 pieces of four columns per sequence: the 64-lane workgroups are cut inside a row and across two sequences
WIDE_H = 264


def gammas(H, lo, hi, seed=0):
    """(H,) fp32: 0, lo, hi, a raw value below lo, one above hi — every column class in the first five columns — then
    random ones over a little more than the range."""
    rng = np.random.default_rng([seed, H])
    g = rng.uniform(lo - 0.05, hi + 0.05, H).astype(F32)
    head = np.array([0.0, lo, hi, lo - 0.125, hi + 0.0625], F32)
    g[:min(H, 5)] = head[:H]
    return g


def kernel_data(H, affine=True, seed=0):
    """dict(Wx, g (the cotangent), bias, scale, shift, i0): fp32, real-valued; affine=False: no bias / scale / shift."""
    rng = np.random.default_rng([seed, H, 7])
    d = dict(Wx=rng.standard_normal((B, T, H)).astype(F32), g=rng.standard_normal((B, T, H)).astype(F32),
             i0=rng.standard_normal((B, H)).astype(F32), bias=None, scale=None, shift=None)
    if affine:
        d.update(bias=rng.standard_normal(H).astype(F32), scale=rng.uniform(0.5, 2.0, H).astype(F32),
                 shift=rng.standard_normal(H).astype(F32))
    return d


# ------------------------------------------------------------------------------------------------ networks
KINDS = dc.KINDS
NB, NT, NC = dc.NB, dc.NT, dc.NC
SIZES, ODD_SIZES = dc.SIZES, dc.ODD_SIZES       # 8 -> 12 -> 12 -> 5, and a recurrent width of 10
NET_LENGTHS = dc.NET_LENGTHS
SYN_LIMITS = (0.0, 0.9)
AFFINE_GAIN = 1.75              # between tests/network_cases.py's 2.0 at T = 8 and 1.25 at T = 19
ND = dc.ND


def _case(kind, norm, bidir=False, lengths=False, surrogate=None, delay=False, sizes=SIZES):
    return (kind, norm, bool(bidir), bool(lengths), surrogate, bool(delay), tuple(sizes))


CASES = tuple(
    [_case(k, n) for k in KINDS for n in ("batchnorm", "layernorm", "none")]
    + [_case("RadLIF", "batchnorm", sizes=ODD_SIZES)]
    + [_case("LIF", "batchnorm", bidir=True), _case("RadLIF", "none", bidir=True)]
    + [_case("adLIF", "layernorm", bidir=True, lengths=True), _case("RLIF", "batchnorm", bidir=True, lengths=True)]
    + [_case("LIF", "batchnorm", lengths=True), _case("RadLIF", "layernorm", lengths=True),
       _case("adLIF", "none", lengths=True)]
    + [_case("adLIF", "batchnorm", surrogate="atan"), _case("LIF", "none", delay=True)])

# case -> the first data seed at which verdict() keeps it (tests/test_synapse_numpy_host.py re-derives every verdict)
SEEDS = dict(zip(CASES, (0, 2, 0, 0, 0, 0, 7, 0, 0, 1, 0, 0, 1, 0, 1, 0, 27, 1, 1, 0, 0, 0)))
assert len(SEEDS) == len(CASES)


def case_id(c):
    kind, norm, bidir, lengths, surrogate, delay, sizes = c
    parts = [kind, {"batchnorm": "bn", "layernorm": "ln", "none": "none"}[norm], "x".join(map(str, sizes))]
    parts += [n for n, on in (("2dir", bidir), ("len", lengths), (surrogate, surrogate), ("delay", delay)) if on]
    return "-".join(parts)


def make_net(sp, c, seed=3, synapse=SYN_LIMITS, **kw):
    """The dyadic network of tests/delay_cases.py with a normalisation: without one the weights' offset carries the
    mean drive (delay_cases.make_net); under one the affine does, on a 2^-4 grid (tests/network_cases.py).  gamma is
    drawn in (0.3, 0.9), its first column above the upper limit (clamped: its gradient is 0)."""
    kind, norm, bidir, _, surrogate, delay, sizes = c
    if surrogate:
        kw["surrogate"] = surrogate
    if delay:
        kw.update(max_delay=ND, learn_delays=False)
    if synapse is not None:
        kw["synapse"] = synapse
    torch.manual_seed(seed)
    net = sp.SNN((NB, None, NC), list(sizes), neuron_type=kind, normalization=norm, bidirectional=bidir, **kw)
    g = torch.Generator().manual_seed(seed + 100)
    density = dc.DENSITY
    with torch.no_grad():
        for k, lay in enumerate(net.snn):
            hidden = k < len(sizes) - 1
            offset = dc.PLAIN_DRIVE / (density * lay.input_size) if (norm == "none" and hidden) else 0.25
            lay.W.weight.copy_(torch.round((lay.W.weight * 4 + offset) * 64) / 64)
            density = dc.HIDDEN_DENSITY
            if hasattr(lay, "V"):
                lay.V.weight.copy_(torch.round(lay.V.weight * 64) / 64)
            if norm != "none":
                gain = AFFINE_GAIN if hidden else 1.0
                H = lay.hidden_size
                lay.norm.weight.copy_(torch.round((torch.rand(H, generator=g) + 1.0) * gain * 16) / 16)
                lay.norm.bias.copy_(torch.round((torch.rand(H, generator=g) * 0.5 + 0.25) * gain * 16) / 16)
            drawn = torch.rand(lay.hidden_size, generator=g) * 0.6 + 0.3   # (drawn with or without a synapse: the twin
            if getattr(lay, "synapse", None) is not None:                  # without one has the same other parameters)
                lay.gamma.copy_(drawn)
                lay.gamma[0] = 0.95
            if getattr(lay, "max_delay", 0):
                lay.delay.copy_(torch.randint(0, ND + 1, (lay.input_size,), generator=g).float())
    return net


def inputs(c, seed):
    """(x (NB,NT,NC) 0/1 — zero on the padding with lengths —, labels, a cotangent for the rates, initial states, lengths)."""
    kind, _, bidir, lengths, _, _, sizes = c
    x, y, init = dc.net_inputs(kind, list(sizes), bidir, seed)
    L = NET_LENGTHS if lengths else None
    if L is not None:
        x = x * rag.valid_mask(L, NT)[:, :, None].float()
    n_rates = sum(sizes[:-1]) * (2 if bidir else 1)
    cot = torch.randn(n_rates, generator=torch.Generator().manual_seed(2000 + seed))
    return x, y, cot, init, L


def loss_of(out, rates, y, cot):
    """The scalar both sides differentiate: the train step's cross-entropy, and a smooth term on the firing rates."""
    return orc.train_step_loss(out, rates, y) + (rates * cot.to(rates.dtype)).sum()


def synapse_filter(z, gamma, limits):
    """The filter in torch (any dtype, autograd): i_t = g i_{t-1} + (1 - g) z_t from zero, g = clamp(gamma, lo, hi)."""
    g = torch.clamp(gamma, min=limits[0], max=limits[1])
    cur = torch.zeros_like(z[:, 0])
    out = []
    for t in range(z.shape[1]):
        cur = g * cur + (1 - g) * z[:, t]
        out.append(cur)
    return torch.stack(out, dim=1)


def _shift(x, delay, D):
    """x (B,T,K) shifted by d_i = rint(clamp(delay_i, 0, D)) steps per feature, zeros shifted in (no gradient to delay)."""
    d = torch.round(delay.detach().clamp(0, D)).long()
    Tn = x.shape[1]
    src = torch.arange(Tn)[:, None] - d[None, :]                         # (T,K)
    idx = src.clamp(min=0)[None].expand(x.shape[0], -1, -1)
    return torch.gather(x, 1, idx) * (src >= 0)[None].to(x.dtype)


def hidden_layer(kind, x, L, p, prefix, init, *, normalization, bidirectional, theta=1.0, limits=SYN_LIMITS):
    """One hidden layer in train mode: the stacking, projection and normalisation of the oracles named above, the filter
    where the layer has a gamma, the cell, the validity mask."""
    Bn, Tn = x.shape[0], x.shape[1]
    full = [Tn] * Bn if L is None else L
    mask = rag.valid_mask(full, Tn)
    if prefix + "delay" in p:
        x = _shift(x, p[prefix + "delay"], ND)
    if bidirectional:
        x, mask = torch.cat([x, bro.flip_in_length(x, full)], dim=0), torch.cat([mask, mask], dim=0)
    Wx = F.linear(x, p[prefix + "W.weight"], p.get(prefix + "W.bias"))
    if L is None:
        Wx = orc._normalise(Wx, p, prefix, normalization, True, None)
    else:
        Wx = rag._normalise(Wx, mask, p, prefix, normalization, True, None)
    if prefix + "gamma" in p:
        Wx = synapse_filter(Wx, p[prefix + "gamma"], limits)
    cell_p = {n: p[prefix + n] for n in ("alpha", "beta", "a", "b") if prefix + n in p}
    if orc.RECURRENT[kind]:
        cell_p["V"] = p[prefix + "V.weight"]
    s = orc.spiking_cell(kind, Wx, cell_p, init["u0"], init.get("w0"), init["s0"], theta)
    s = s * mask[:, :, None].to(s.dtype)
    if bidirectional:
        s_f, s_b = s.chunk(2, dim=0)
        s = torch.cat([s_f, bro.flip_in_length(s_b, full)], dim=2)
    return s


class _Surrogate:
    """own_dtype_spikes of tests/bidir_ragged_oracle.py with a selectable surrogate."""

    def __init__(self, surrogate):
        self.seen, self.surrogate = [], surrogate

    def __enter__(self):
        from sparch_amd.snns import SpikeFunctionSurrogate, resolve_surrogate
        name, scale = resolve_surrogate(self.surrogate or "boxcar")

        def step(d):
            self.seen.append(d.detach())
            return SpikeFunctionSurrogate.apply(d, name, scale)
        self.old, orc.spike = orc.spike, step
        return self

    def __exit__(self, *exc):
        orc.spike = self.old


def oracle_run(c, params, x, y, cot, init, L, dtype=torch.float64, backward=True):
    """One train-mode step of case c in dtype: out, rates, spikes per hidden layer, u - theta per hidden layer as
    (rows, T, H), loss and every gradient."""
    kind, norm, bidir, _, surrogate, _, sizes = c

    def cast(t):
        return t.to(dtype) if t.is_floating_point() else t

    p = {k: cast(v).clone().requires_grad_(v.is_floating_point() and "running" not in k and not k.endswith("delay"))
         for k, v in params.items() if "num_batches" not in k}
    init = [{k: cast(v) for k, v in st.items()} for st in init]
    a, spikes = cast(x), []
    n_hidden = len(sizes) - 1
    with _Surrogate(surrogate) as rec:
        for k in range(n_hidden):
            a = hidden_layer(kind, a, L, p, f"snn.{k}.", init[k], normalization=norm, bidirectional=bidir)
            spikes.append(a)
    n_valid = float(NB * NT if L is None else sum(L))
    rates = torch.cat(spikes, dim=2).sum(dim=(0, 1)) / n_valid
    pre = f"snn.{n_hidden}."
    if pre + "delay" in p:
        a = _shift(a, p[pre + "delay"], ND)
    if L is None:
        out = orc.readout_layer(a, p, pre, init[n_hidden]["u0"], normalization=norm, training=True)
    else:
        out = rag.readout_layer(a, L, rag.valid_mask(L, NT), p, pre, init[n_hidden]["u0"], normalization=norm,
                                training=True)
    r = dict(out=out.detach(), rates=rates.detach(), spikes=[s.detach() for s in spikes],
             diffs=[torch.stack(rec.seen[k * NT:(k + 1) * NT], dim=1) for k in range(n_hidden)])
    if backward:
        loss = loss_of(out, rates, y, cot)
        loss.backward()
        r.update(loss=loss.detach(), grads={k: v.grad for k, v in p.items() if v.requires_grad})
    return r


def valid_rows(c, L):
    rows = NB * (2 if c[2] else 1)
    if L is None:
        return torch.ones(rows, NT, 1, dtype=torch.bool)
    m = rag.valid_mask(L, NT)
    return (torch.cat([m, m]) if c[2] else m)[:, :, None]


@functools.lru_cache(maxsize=None)
def runs(c, seed):
    """(the network's state_dict, the inputs, the fp64 run, the fp32 run) of case c at a data seed."""
    import sparch_amd as sp
    params = {k: v.detach().clone() for k, v in make_net(sp, c).state_dict().items()}
    data = inputs(c, seed)
    return params, data, oracle_run(c, params, *data, torch.float64), oracle_run(c, params, *data, torch.float32)


def verdict(c, seed):
    """(kept, reason): the keep rule of tests/network_cases.py on the oracle's two runs — the fp32 and fp64 spike trains
    agree, the smallest |u - theta| is MARGIN times the largest fp32-vs-fp64 difference of u - theta, every hidden
    layer fires inside RATE_WINDOW."""
    _, data, r64, r32 = runs(c, seed)
    m = valid_rows(c, data[4])
    for s64, s32 in zip(r64["spikes"], r32["spikes"]):
        if not torch.equal(s64.float(), s32):
            return False, "the spike trains of the fp32 and fp64 runs differ"
    margin = min(float(d[m.expand_as(d)].abs().min()) for d in r64["diffs"])
    err = max(float((d32.double() - d64)[m.expand_as(d64)].abs().max()) for d64, d32 in zip(r64["diffs"], r32["diffs"]))
    if not margin >= MARGIN * err or margin == 0.0:
        return False, f"margin {margin:.2e} under {MARGIN:g} x {err:.2e}"
    for d in r64["diffs"]:
        rate = float((d > 0)[m.expand_as(d)].double().mean())
        if not RATE_WINDOW[0] <= rate <= RATE_WINDOW[1]:
            return False, f"firing rate {rate:.3f}"
    return True, ""


def pick_seed(c, limit=64):
    for seed in range(limit):
        if verdict(c, seed)[0]:
            return seed
    raise AssertionError(f"no seed below {limit} keeps {case_id(c)}")


def device_run(sp, c, seed, net=None, grad=True, **fw):
    """One train-mode step of case c on the HIP path, the initial states injected: dict(net, out, rates, loss, spikes
    {layer: train}).  The spike trains are recorded around forward_with_rate, so the layers still hand each other
    placeholders and bf16 planes.  fw: further arguments of SNN.forward (pack=True)."""
    from sparch_amd import functional as Fn
    from sparch_amd import snns as snn_mod
    x, y, cot, init, L = inputs(c, seed)
    if net is None:
        net = make_net(sp, c)
    net = net.to(DEV).train()
    rec = {}
    for k, lay in enumerate(list(net.snn)[:-1]):
        def wrapped(inp, states=None, orig=lay.forward_with_rate, k=k, **kw):
            s, r = orig(inp, states=states, **kw)
            rec[k] = snn_mod.materialize_spikes(s).detach()
            return s, r
        lay.forward_with_rate = wrapped
    if L is not None:
        fw = dict(fw, lengths=torch.tensor(L))
    loss = None
    with torch.set_grad_enabled(grad), dc.injected_states(init):
        out, rates = net(x.to(DEV), **fw)
        if grad:
            loss = loss_of(out, rates, y.to(DEV), cot.to(DEV))
            loss.backward()
    Fn.check_status()
    for lay in list(net.snn)[:-1]:
        del lay.forward_with_rate
    return dict(net=net, out=out, rates=rates, loss=loss, spikes=rec)
