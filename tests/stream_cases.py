"""
Shared cases and check bodies of the streaming GPU tests (tests/test_streaming_gpu.py, tests/test_stream_fused_gpu.py,
tests/test_stream_sparse_gpu.py): dyadic networks and layers, a stream fed in chunks with its per-layer spikes, the eval
forward with injected initial states, and the check_* bodies that the fused tests run on sparch_amd and the sparse tests
on a stand-in whose fused streams are event-driven.  Nothing here touches the GPU at import.
"""
import contextlib

import numpy as np
import torch

from oracle import bptt_numpy as bp
from oracle import snn_oracle as orc
from tests.golden_io import layer_spikes, snn_case
from tests.kit import DEV, Fn
from tests.spiking_cases import build_snn, dyadic_cell_case_fwd


def chunkings(T):
    uneven, pat, i = [], [5, 1, 13, 2, 8, 1, 1, 30], 0
    while sum(uneven) < T:
        uneven.append(min(pat[i % len(pat)], T - sum(uneven)))
        i += 1
    return {"ones": [1] * T, "sevens": [7] * (T // 7) + ([T % 7] if T % 7 else []), "whole": [T], "uneven": uneven}


def run_stream(st, x, chunks):
    """Feed x (B,T,C) on the device in `chunks`; returns (final out or concatenated spikes, per-layer spikes)."""
    rec = {}
    st._spike_tap = lambda k, s: rec.setdefault(k, []).append(s.float().cpu())
    outs, t0 = [], 0
    for n in chunks:
        out = st.step(x[:, t0:t0 + n])
        outs.append(out.clone())
        t0 += n
    assert t0 == x.shape[1] and st.steps_seen >= t0
    st._spike_tap = None
    return outs, {k: torch.cat(v, dim=1) for k, v in rec.items()}


def whole_forward(net, x, order):
    """net(x) in eval with the initial states `order` (flat list, the draw order) injected; per-layer spikes taken
    from the layers' outputs as they travel (the bf16 plane)."""
    from sparch_amd import snns as snn_mod
    states = iter(order)

    def next_state(rows, cols, device):
        t = next(states)
        assert tuple(t.shape) == (rows, cols)
        return t.to(device)

    rec, originals = {}, []
    hidden = list(net.snn)[:-1] if net.use_readout_layer else list(net.snn)
    for k, lay in enumerate(hidden):
        def wrapped(inp, states=None, orig=lay.forward_with_rate, k=k, **kw):
            s, r = orig(inp, states=states, **kw)
            rec[k] = snn_mod.materialize_spikes(s).detach().float().cpu()
            return s, r
        originals.append(lay)
        lay.forward_with_rate = wrapped
    old = snn_mod._rand_to
    snn_mod._rand_to = next_state
    try:
        with torch.no_grad():
            out, rates = net(x)
    finally:
        snn_mod._rand_to = old
        for lay in originals:
            del lay.forward_with_rate
    return out, rates, rec


def dyadic_net(sp, kind, B, C, sizes, norm, seed):
    """A network with W on a 2^-6 grid (V too), BatchNorm statistics moved off their initial values, 0/1 input and
    initial states on a 2^-4 grid: every projection sum is exact in any order."""
    torch.manual_seed(seed)
    net = sp.SNN((B, None, C), sizes, neuron_type=kind, dropout=0.0, normalization=norm)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for lay in net.snn:
            lay.W.weight.copy_(torch.round(lay.W.weight * 4 * 64) / 64)
            if hasattr(lay, "V"):
                lay.V.weight.copy_(torch.round(lay.V.weight * 64) / 64)
            if norm == "batchnorm":
                lay.norm.running_mean.copy_(torch.rand(lay.hidden_size, generator=g) * 0.2 - 0.1)
                lay.norm.running_var.copy_(torch.rand(lay.hidden_size, generator=g) * 0.1 + 0.02)
                lay.norm.weight.copy_(torch.rand(lay.hidden_size, generator=g) + 0.5)
                lay.norm.bias.copy_(torch.rand(lay.hidden_size, generator=g) * 0.4)
    init = orc.draw_init_states(B, sizes, kind)
    init = [{k: torch.floor(v * 16) / 16 for k, v in st.items()} for st in init]
    return net.to(DEV).eval(), init


_plain = {}


def plain_stream(sp, name):
    """(out, integer spike counts) of the UNFUSED stream over the fixture in chunks of 1: made once per fixture."""
    if name not in _plain:
        cfg, x, y, params, init, z = snn_case(name)
        st = sp.StreamingSNN(build_snn(sp, cfg, params).eval(), cfg["B"])
        st.reset(states=init)
        xd = x.to(DEV)
        for t in range(cfg["T"]):
            out = st.step(xd[:, t:t + 1])
        Fn().check_status()
        _plain[name] = (out.cpu(), torch.cat([L.count[:L.H] for L in st._layers if not L.readout]).cpu())
    return _plain[name]


def both_parities_replayed(st):
    return len(st._fg) == 2 and all(g["replays"] >= 2 for g in st._fg.values())


def check_against_fixture(sp, st, name, outs, rec):
    cfg, x, y, params, init, z = snn_case(name)
    B, T = cfg["B"], cfg["T"]
    assert sorted(rec) == [0, 1]
    for k in sorted(rec):
        ref = layer_spikes(z, k)
        assert ref.sum() > 0
        got = rec[k].numpy()
        assert np.array_equal(got, ref), (k, float((got != ref).mean()))
    assert st.steps_seen == T
    assert np.abs(outs[-1].cpu().numpy() - z["out"]).max() <= 2e-5 * T
    out_plain, counts_plain = plain_stream(sp, name)
    assert torch.equal(outs[-1].cpu(), out_plain)
    counts = np.round(st.firing_rates().cpu().numpy().astype(np.float64) * B * T).astype(np.int64)
    counts_ref = np.round(z["rates"].astype(np.float64) * B * T).astype(np.int64)
    assert np.array_equal(counts, counts_ref) and np.array_equal(counts, counts_plain.numpy())


def one_layer_net(sp, kind, K, sizes, Ws, ps, use_bias=False, bias=None):
    """Hidden layers `sizes` on K inputs, no readout, the given projections and cell parameters."""
    torch.manual_seed(1)
    net = sp.SNN((1, None, K), list(sizes), neuron_type=kind, dropout=0.0, normalization="none",
                 use_readout_layer=False, use_bias=use_bias)
    with torch.no_grad():
        for lay, W, p in zip(net.snn, Ws, ps):
            lay.W.weight.copy_(W)
            if use_bias:
                lay.W.bias.fill_(bias)
            lay.alpha.copy_(p["alpha"])
            for k in ("beta", "a", "b"):
                if k in p:
                    getattr(lay, k).copy_(p[k])
            if "V" in p and hasattr(lay, "V"):
                lay.V.weight.copy_(p["V"])
    return net.to(DEV).eval()


def dyadic_layer(kind, B, T, K, H, seed):
    """W and V integers in [-24, 24] / 64 (W NOT the identity), cell parameters of spiking_cases.dyadic_cell_case,
    states on a 2^-4 grid: W x and s V are exact in any order."""
    g = torch.Generator().manual_seed(seed)
    W = torch.randint(-24, 25, (H, K), generator=g).float() / 64.0
    _, p, u0, w0, s0 = dyadic_cell_case_fwd("RadLIF" if kind in ("adLIF", "RadLIF") else "RLIF", B, 1, H, seed + 1)
    grid = lambda t: None if t is None else torch.floor(t * 16) / 16
    # (u0 in [0, 2): the smallest shapes, whose zero-mean projection alone rarely reaches the threshold, spike too)
    return W, p, grid(u0 * 2), (grid(w0) if kind in ("adLIF", "RadLIF") else None), grid(torch.rand(B, H, generator=g))


def exact_projection(x, W):
    Wx = (x.double() @ W.double().t())
    assert torch.equal(Wx.float().double(), Wx)
    return Wx.float()


def state_of(u0, w0, s0):
    st = {"u": u0, "s": s0}
    if w0 is not None:
        st["w"] = w0
    return st


def check_fused_stream_equals_reference_fixture(sp, name, graph):
    cfg, x, y, params, init, z = snn_case(name)
    net = build_snn(sp, cfg, params).eval()
    st = sp.StreamingSNN(net, cfg["B"], graph=graph, fused=True)
    assert st.fused_active
    st.reset(states=init)
    outs, rec = run_stream(st, x.to(DEV), [1] * cfg["T"])
    Fn().check_status()
    if graph:
        assert both_parities_replayed(st), "the two parities were not both captured and replayed"
    else:
        assert not st._fg
    assert all(L.binary for L in st._layers if not L.readout)
    check_against_fixture(sp, st, name, outs, rec)


def check_fused_equals_whole(sp, net, x, init, graph):
    """The assertions of check_stream_equals_whole (tests/test_streaming_gpu.py) on a fused stream in chunks of 1."""
    order = [st[k] for st in init for k in ("u0", "w0", "s0") if k in st]
    out_w, rates_w, rec_w = whole_forward(net, x, order)
    Fn().check_status()
    st = sp.StreamingSNN(net, x.shape[0], graph=graph, fused=True)
    st.reset(states=init)
    outs, rec = run_stream(st, x, [1] * x.shape[1])
    if graph:
        assert st._fg and all(g["replays"] >= 2 for g in st._fg.values())
    assert sorted(rec) == sorted(rec_w) and len(rec) > 0
    for k in sorted(rec):
        assert float(rec_w[k].sum()) > 0, k
        assert torch.equal(rec[k], rec_w[k]), (k, float((rec[k] != rec_w[k]).float().mean()))
    assert torch.equal(outs[-1], out_w)
    assert torch.equal(st.firing_rates(), rates_w)


def check_fused_stream_equals_eval_forward_with_batchnorm(sp, kind):
    if kind == "RadLIF":
        cfg, x, y, params, init, z = snn_case("dyadic_RadLIF_bn")
        for k in list(params):
            if "running" in k:
                params[k] = torch.from_numpy(z["after." + k])
        net = build_snn(sp, cfg, params).eval()
    else:
        B, T, C, sizes = 8, 40, 64, [64, 128, 20]
        net, init = dyadic_net(sp, kind, B, C, sizes, "batchnorm", 77)
        x = (torch.rand(B, T, C, generator=torch.Generator().manual_seed(5)) < 0.3).float()
    check_fused_equals_whole(sp, net, x.to(DEV), init, graph=False)
    check_fused_equals_whole(sp, net, x.to(DEV), init, graph=True)


MIX = [1, 1, 7, 1, 5, 1, 1, 1, 13, 1]


def mixed_chunks(T):
    chunks, i = [], 0
    while sum(chunks) < T:
        chunks.append(min(MIX[i % len(MIX)], T - sum(chunks)))
        i += 1
    return chunks


def check_fused_and_chunked_steps_alternate_on_one_state(sp, graph):
    name = "dyadic_RadLIF_none"
    cfg, x, y, params, init, z = snn_case(name)
    net = build_snn(sp, cfg, params).eval()
    st = sp.StreamingSNN(net, cfg["B"], graph=graph, fused=True)
    st.reset(states=init)
    chunks = mixed_chunks(cfg["T"])
    assert chunks[:5] == [1, 1, 7, 1, 5] and sum(1 for c in chunks if c == 1) % 2 == 1
    outs, rec = run_stream(st, x.to(DEV), chunks)
    Fn().check_status()
    if graph:
        assert both_parities_replayed(st)
    check_against_fixture(sp, st, name, outs, rec)


def check_stream_continues_behind_an_odd_number_of_fused_steps(sp, how, graph):
    """[1,1,7,1] is three fused steps: the current spike buffers are the second ones.  A fresh stream given
    get_state(), and the same stream after refresh(), go on to the undisturbed stream's result."""
    name = "dyadic_RadLIF_none"
    cfg, x, y, params, init, z = snn_case(name)
    T, xd = cfg["T"], x.to(DEV)
    net = build_snn(sp, cfg, params).eval()
    st = sp.StreamingSNN(net, cfg["B"], graph=graph, fused=True)
    st.reset(states=init)
    chunks = mixed_chunks(T)
    outs_a, rec_a = run_stream(st, xd[:, :10], chunks[:4])
    assert all(L.s is not L.s_first for L in st._layers if L.recurrent)
    if how == "set_state":
        st2 = sp.StreamingSNN(net, cfg["B"], graph=graph, fused=True)
        st2.set_state(st.get_state())
    else:
        st.refresh()
        st2 = st
        assert all(L.s is not L.s_first for L in st._layers if L.recurrent)      # (the state is kept by name)
    rest = chunks[4:]
    assert sum(rest) == T - 10
    outs_b, rec_b = run_stream(st2, xd[:, 10:], rest)
    Fn().check_status()
    for k in (0, 1):
        got = torch.cat([rec_a[k], rec_b[k]], dim=1).numpy()
        assert np.array_equal(got, layer_spikes(z, k)), k
    assert torch.equal(outs_b[-1].cpu(), plain_stream(sp, name)[0])


def check_fused_reset_rows_mid_stream(sp):
    """The scenario of test_streaming_gpu.test_reset_rows_mid_stream in chunks of 1."""
    cfg, x, y, params, init, z = snn_case("dyadic_RadLIF_none")
    B, T = cfg["B"], cfg["T"]
    net = build_snn(sp, cfg, params).eval()
    xd = x.to(DEV)
    rows, half = [1, 3], 21                      # (an odd number of fused steps before the row reset)
    fresh = [{k: torch.floor(v * 16) / 16 for k, v in stt.items()}
             for stt in orc.draw_init_states(len(rows), cfg["layer_sizes"], cfg["neuron_type"])]
    x2 = (torch.rand(len(rows), T - half, cfg["C"], generator=torch.Generator().manual_seed(8)) < 0.3).float().to(DEV)

    plain = sp.StreamingSNN(net, B, fused=True)
    plain.reset(states=init)
    outs_plain, rec_plain = run_stream(plain, xd, [1] * T)

    small = sp.StreamingSNN(net, len(rows), fused=True)
    small.reset(states=fresh)
    outs_small, rec_small = run_stream(small, x2, [1] * (T - half))

    st = sp.StreamingSNN(net, B, fused=True)
    st.reset(states=init)
    run_stream(st, xd[:, :half], [1] * half)
    st.reset(states=fresh, rows=rows)
    assert list(st.row_steps) == [half, 0, half, 0] + [half] * (B - 4) and st.steps_seen == half
    x_mix = xd[:, half:].clone()
    x_mix[rows] = x2
    outs, rec = run_stream(st, x_mix, [1] * (T - half))
    Fn().check_status()
    others = [r for r in range(B) if r not in rows]
    assert torch.equal(outs[-1][rows], outs_small[-1]) and torch.equal(outs[-1][others], outs_plain[-1][others])
    for k in rec:
        assert float(rec_small[k].sum()) > 0
        assert torch.equal(rec[k][rows], rec_small[k])
        assert torch.equal(rec[k][others], rec_plain[k][others, half:])
    assert list(st.row_steps) == [T, T - half, T, T - half] + [T] * (B - 4)


def check_fused_step_reads_uint8_counts_like_their_fp32_twin(sp):
    kind, B, K, H, T = "RLIF", 9, 48, 130, 12
    W, p, u0, w0, s0 = dyadic_layer(kind, B, T, K, H, 7)
    x = torch.randint(0, 4, (B, T, K), generator=torch.Generator().manual_seed(3)).float() * \
        (torch.rand(B, T, K, generator=torch.Generator().manual_seed(4)) < 0.3).float()
    assert x.max() > 1
    net = one_layer_net(sp, kind, K, [H], [W], [p])
    res = []
    for xin in (x.to(DEV), x.to(torch.uint8).to(DEV)):
        st = sp.StreamingSNN(net, B, fused=True)
        st.set_state([state_of(u0, w0, s0)])
        outs, _ = run_stream(st, xin, [1] * T)
        res.append((torch.cat(outs, dim=1).cpu(), st.get_state()[0]["u"].cpu()))
    with torch.no_grad():
        ref = orc.spiking_cell(kind, exact_projection(x, W), p, u0, w0, s0)
    assert ref.sum() > 0 and torch.equal(res[0][0], ref)
    assert torch.equal(res[1][0], res[0][0]) and torch.equal(res[1][1], res[0][1])


def check_padded_layer_feeds_the_next(sp, graph):
    """RLIF [130, 66]: the second layer reads the first one's state at its padded row stride (132 != K = 130)."""
    kind, B, K, T, sizes = "RLIF", 9, 48, 12, [130, 66]
    W1, p1, u1, _, s1 = dyadic_layer(kind, B, T, K, sizes[0], 21)
    W2, p2, u2, _, s2 = dyadic_layer(kind, B, T, sizes[0], sizes[1], 22)
    x = (torch.rand(B, T, K, generator=torch.Generator().manual_seed(6)) < 0.3).float()
    with torch.no_grad():
        ref1 = orc.spiking_cell(kind, exact_projection(x, W1), p1, u1, None, s1)
        ref2 = orc.spiking_cell(kind, exact_projection(ref1, W2), p2, u2, None, s2)
    assert ref1.sum() > 0 and ref2.sum() > 0
    st = sp.StreamingSNN(one_layer_net(sp, kind, K, sizes, [W1, W2], [p1, p2]), B, graph=graph, fused=True)
    st.set_state([state_of(u1, None, s1), state_of(u2, None, s2)])
    outs, rec = run_stream(st, x.to(DEV), [1] * T)
    Fn().check_status()
    if graph:
        assert both_parities_replayed(st)
    assert torch.equal(rec[0], ref1) and torch.equal(rec[1], ref2)
    assert torch.equal(torch.cat(outs, dim=1).cpu(), ref2)
    rates = torch.cat([ref1.sum(dim=(0, 1)), ref2.sum(dim=(0, 1))]).to(torch.int32) * (1.0 / float(B * T))
    assert torch.equal(st.firing_rates().cpu(), rates)


def check_fused_step_one_step_ahead_vs_oracle_trajectory(sp, kind, B, T, K, H, inp):
    """Real-valued W (Wx of std about 1.5, bias 0.5) and orthogonal V: teacher forcing with the yardstick and the bars
    of test_recurrent_stream_one_step_ahead_vs_oracle_trajectory.  The oracle runs on Wx computed in fp64 and rounded
    once; its (u, w, s)_{t-1} for EVERY t are the rows of one big batch, loaded with set_state, and ONE fused step is
    made.  A spike may differ only where the oracle's |u - 1| <= 1e-4; flips <= 1e-4 N + 2; oracle rate > 0.003."""
    g = torch.Generator().manual_seed(17 + H + K)
    if inp == "binary":
        x, ex2 = (torch.rand(B, T, K, generator=g) < 0.15).float(), 0.15
    else:
        x, ex2 = torch.rand(B, T, K, generator=g), 1.0 / 3.0           # the mel-feature case: the same code path
    lim = 1.5 * (3.0 / (K * ex2)) ** 0.5
    W = (torch.rand(H, K, generator=g) * 2 - 1) * lim
    p = {"alpha": torch.rand(H, generator=g) * 0.14 + 0.82}
    if kind in ("RLIF", "RadLIF"):
        p["V"] = torch.nn.init.orthogonal_(torch.empty(H, H), generator=g)
    if kind in ("adLIF", "RadLIF"):
        p.update(beta=torch.rand(H, generator=g) * 0.024 + 0.967, a=torch.rand(H, generator=g) * 2 - 1,
                 b=torch.rand(H, generator=g) * 2)
    u0, s0 = torch.rand(B, H, generator=g), torch.rand(B, H, generator=g)
    w0 = torch.rand(B, H, generator=g) if kind in ("adLIF", "RadLIF") else None
    Wx = (x.double() @ W.double().t() + 0.5).float()
    pn = {k: v.numpy() for k, v in p.items()}
    S, U, Wst = bp.cell_forward(kind, Wx.numpy(), pn, u0.numpy(), None if w0 is None else w0.numpy(), s0.numpy())
    rate = float(S.mean())
    assert rate > 0.003

    def before(traj, first):                     # (B,T,H) of step t-1's values, t = 0: the initial state
        prev = np.concatenate([first.numpy()[:, None], traj[:, :-1]], axis=1)
        return torch.from_numpy(prev.reshape(B * T, H).copy())

    state = {"u": before(U, u0), "s": before(S, s0)}
    if Wst is not None:
        state["w"] = before(Wst, w0)
    st = sp.StreamingSNN(one_layer_net(sp, kind, K, [H], [W], [p], use_bias=True, bias=0.5), B * T, fused=True)
    st.set_state([state])
    s = st.step(x.reshape(B * T, 1, K).to(DEV)).cpu().numpy().reshape(B, T, H)
    Fn().check_status()
    diff = s != S
    n = int(diff.sum())
    worst = float(np.abs(U[diff] - 1.0).max()) if n else 0.0
    print(f"{kind} {inp} B={B} T={T} K={K} H={H}: {n} flips in {S.size} spikes (cap {1e-4 * S.size + 2:.1f}), "
          f"worst |u - 1| at a flip {worst:.3g}, oracle rate {rate:.4f}")
    assert worst <= 1e-4
    assert n <= 1e-4 * S.size + 2


def check_step_geometry_vs_oracle(sp, kind, B, K, H, T, seed, x):
    """One fused layer on dyadic W and V in chunks of 1 over the input x (B,T,K), against the oracle: bit for bit."""
    W, p, u0, w0, s0 = dyadic_layer(kind, B, T, K, H, seed)
    with torch.no_grad():
        ref = orc.spiking_cell(kind, exact_projection(x, W), p, u0, w0, s0)
    assert ref.sum() > 0
    st = sp.StreamingSNN(one_layer_net(sp, kind, K, [H], [W], [p]), B, fused=True)
    st.set_state([state_of(u0, w0, s0)])
    outs, rec = run_stream(st, x.to(DEV), [1] * T)
    Fn().check_status()
    s = torch.cat(outs, dim=1).cpu()
    assert s.shape == ref.shape and torch.equal(s, ref), float((s != ref).float().mean())
    assert torch.equal(rec[0], ref)
    got = st.get_state()[0]
    assert got["u"].shape == (B, H) and torch.equal(got["s"].cpu(), ref[:, -1])
    assert torch.equal(st.firing_rates().cpu(), ref.sum(dim=(0, 1)).to(torch.int32) * (1.0 / float(B * T)))
    L = st._layers[0]
    if L.Hs != H:                                                   # the padded columns were never written
        assert float(L.s[:, H:].abs().sum()) == 0 and float(L.s_alt[:, H:].abs().sum()) == 0
        assert float(L.u[:, H:].abs().sum()) == 0 and int(L.count[H:].sum()) == 0


@contextlib.contextmanager
def recorded_calls(names):
    """The names of the library's entry points among `names` that were called meanwhile, in order."""
    from sparch_amd import _capi
    saved, seen = {}, []
    for name in names:
        f = getattr(_capi.lib, name)
        saved[name] = f

        def wrapped(*a, _f=f, _n=name):
            seen.append(_n)
            return _f(*a)
        setattr(_capi.lib, name, wrapped)
    try:
        yield seen
    finally:
        for name, f in saved.items():
            setattr(_capi.lib, name, f)


def calls_of(fn):
    """Every launching entry point that fn() calls, in order."""
    from sparch_amd import _capi
    names = [n for n in _capi.PROTOTYPES if not n.endswith("_bytes") and n not in ("sparch_device_cus",)]
    with recorded_calls(names) as seen:
        fn()
    return seen
