"""GPU: streaming inference (sparch_amd/streaming.py and the *_stream_fwd kernels) — chunked equals whole.

1. whole networks against the REFERENCE's dyadic fixtures, streamed in four chunkings, eager and as a replayed graph;
2. chunked stream == the existing eval forward net(x) with BatchNorm, for RadLIF / adLIF / LIF, fp32 and bf16 operands;
3. the cell kernels on real-valued data: LIF / adLIF / readout bit-equal to the whole-sequence kernels, RLIF / RadLIF
   teacher-forced against an oracle trajectory (the project's yardstick for real-valued V);
4. launch geometries: the headline (256, 1024) shape with the state carried 25 times, 1 and 33 rows, the step path
   (H = 1536), the zero-padded path (H = 130);
5. reset(rows=...) mid-stream;  6. nothing grows with the stream's length;  7. streamed filterbank.
"""
import numpy as np
import pytest
import torch

from oracle import bptt_numpy as bp
from oracle import snn_oracle as orc
from tests.golden_io import DYADIC_LONG, layer_spikes, snn_case
from tests.guarded import guard_arena
from tests.kit import DEV, bf16_mode, sp  # noqa: F401  (bf16_mode, sp: fixtures)
from tests.kit import Fn as _Fn
from tests.spiking_cases import build_snn as _build
from tests.spiking_cases import dyadic_cell_case_fwd as _dyadic_cell_case
from tests.stream_cases import chunkings, dyadic_net, run_stream, whole_forward

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ 1. reference-pinned
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("chunking", ["ones", "sevens", "whole", "uneven"])
@pytest.mark.parametrize("name", ["dyadic_RadLIF_none", "dyadic_RLIF_none_bias", DYADIC_LONG])
def test_stream_equals_reference_fixture(sp, name, chunking, graph):
    """Train-mode reference runs with dropout 0 and no normalisation (eval == train): every hidden layer's spikes bit
    for bit, the output within the parity test's 2e-5 * T, the firing rates as integer counts."""
    Fn = _Fn()
    cfg, x, y, params, init, z = snn_case(name)
    B, T = cfg["B"], cfg["T"]
    net = _build(sp, cfg, params).eval()
    st = sp.StreamingSNN(net, B, graph=graph)
    st.reset(states=init)
    outs, rec = run_stream(st, x.to(DEV), chunkings(T)[chunking])
    Fn.check_status()
    if graph and chunking in ("ones", "sevens"):     # (`whole` is one eager chunk; `uneven` replays where 5 recurs)
        assert st._g is not None and st._g_replays >= 2, "the step was never captured and replayed"
    assert sorted(rec) == [0, 1]
    for k in sorted(rec):
        ref = layer_spikes(z, k)
        assert ref.sum() > 0
        got = rec[k].numpy()
        assert np.array_equal(got, ref), (k, float((got != ref).mean()))
    assert st.steps_seen == T
    assert np.abs(outs[-1].cpu().numpy() - z["out"]).max() <= 2e-5 * T
    counts = np.round(st.firing_rates().cpu().numpy().astype(np.float64) * B * T).astype(np.int64)
    counts_ref = np.round(z["rates"].astype(np.float64) * B * T).astype(np.int64)
    assert np.array_equal(counts, counts_ref)


# ------------------------------------------------------------------------------------------ 2. chunked == whole
def check_stream_equals_whole(sp, net, x, init, chunks, graph=False, spiking=None):
    Fn = _Fn()
    order = [st[k] for st in init for k in ("u0", "w0", "s0") if k in st]
    out_w, rates_w, rec_w = whole_forward(net, x, order)
    Fn.check_status()
    st = sp.StreamingSNN(net, x.shape[0], graph=graph)
    st.reset(states=init)
    outs, rec = run_stream(st, x, chunks)
    Fn.check_status()
    if graph:
        assert st._g is not None and st._g_replays >= 2, "the step was never captured and replayed"
    assert sorted(rec) == sorted(rec_w) and len(rec) > 0
    for k in sorted(rec):
        if spiking is None or k in spiking:
            assert float(rec_w[k].sum()) > 0, k
        assert torch.equal(rec[k], rec_w[k]), (k, float((rec[k] != rec_w[k]).float().mean()))
    assert torch.equal(outs[-1], out_w)
    assert torch.equal(st.firing_rates(), rates_w)


@pytest.mark.parametrize("low", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["RadLIF", "adLIF", "LIF"])
def test_stream_equals_eval_forward_with_batchnorm(sp, kind, low):
    """The projection sums are exact and the eval affine is per element: equality is guaranteed, not observed."""
    Fn = _Fn()
    prev = Fn.set_compute_dtype("bf16" if low else "fp32")
    try:
        if kind == "RadLIF":
            cfg, x, y, params, init, z = snn_case("dyadic_RadLIF_bn")
            for k in list(params):
                if "running" in k:
                    params[k] = torch.from_numpy(z["after." + k])
            net = _build(sp, cfg, params).eval()
        else:
            B, T, C, sizes = 8, 40, 64, [64, 128, 20]
            net, init = dyadic_net(sp, kind, B, C, sizes, "batchnorm", 77)
            x = (torch.rand(B, T, C, generator=torch.Generator().manual_seed(5)) < 0.3).float()
        T = x.shape[1]
        check_stream_equals_whole(sp, net, x.to(DEV), init, chunkings(T)["uneven"])
        check_stream_equals_whole(sp, net, x.to(DEV), init, [4] * (T // 4), graph=True)
    finally:
        Fn.set_compute_dtype(prev)


@pytest.mark.parametrize("kind,sizes", [("adLIF", [64, 128, 20]), ("RLIF", [66, 64, 20])])
def test_stream_equals_eval_forward_with_layernorm(sp, kind, sizes):
    """LayerNorm is per row: chunked equals whole here too (dyadic W: the projection the norm sees is exact; the RLIF
    case has a hidden width that is not a multiple of 4, so the normalised rows run zero-padded).  Every layer's
    spikes must be equal; the first layer's must exist (a normalised second RLIF layer may stay silent)."""
    B, T, C = 8, 40, 64
    net, init = dyadic_net(sp, kind, B, C, sizes, "layernorm", 91)
    x = (torch.rand(B, T, C, generator=torch.Generator().manual_seed(9)) < 0.3).float().to(DEV)
    check_stream_equals_whole(sp, net, x, init, chunkings(T)["uneven"], spiking=[0])


def test_stream_takes_uint8_counts_and_draws_like_forward(sp):
    """uint8 spike counts give the float input's result, and reset() without states draws what one SNN.forward draws
    under the same torch.manual_seed."""
    Fn = _Fn()
    cfg, x, y, params, init, z = snn_case("dyadic_RadLIF_none")
    net = _build(sp, cfg, params).eval()
    xd = x.to(DEV)
    torch.manual_seed(99)
    with torch.no_grad():
        out_w, rates_w = net(xd)
    st = sp.StreamingSNN(net, cfg["B"])
    torch.manual_seed(99)
    st.reset()
    outs, _ = run_stream(st, xd.to(torch.uint8), [3, 17, 20])
    Fn.check_status()
    assert torch.equal(outs[-1], out_w) and torch.equal(st.firing_rates(), rates_w)


# ------------------------------------------------------------------------------------------ 3. cells, real-valued
def _cell_params(kind, H, g):
    p = {"alpha": torch.rand(H, generator=g) * 0.14 + 0.82}
    if kind in ("adLIF", "RadLIF"):
        p.update(beta=torch.rand(H, generator=g) * 0.024 + 0.967, a=torch.rand(H, generator=g) * 2 - 1,
                 b=torch.rand(H, generator=g) * 2)
    return p


RING_CHUNKS = [1, 7, 8, 9, 15, 16, 17, 2]     # around the scan kernels' ring depths (8 at 4 columns per thread, 16)


@pytest.mark.parametrize("kind", ["LIF", "adLIF"])
@pytest.mark.parametrize("Bp,H,chunks", [(1, 3, RING_CHUNKS), (33, 3, RING_CHUNKS), (65, 100, RING_CHUNKS),
                                         (1, 1024, RING_CHUNKS), (33, 100, RING_CHUNKS), (65, 1024, RING_CHUNKS),
                                         (1, 100, RING_CHUNKS), (33, 1024, RING_CHUNKS), (65, 3, RING_CHUNKS),
                                         (512, 1024, [1, 7, 8, 9, 11])])
def test_cell_stream_kernel_equals_whole_sequence_kernel(kind, Bp, H, chunks):
    """sparch_cell_stream_fwd over chunks of a fixed real-valued Wx against sparch_cell_fwd on the whole sequence:
    spikes, the final u / w / s (the whole run's last saved row) and the counts, bit for bit.  (512 x 1024 takes the
    four-columns-per-thread kernels.)"""
    from sparch_amd._capi import KIND, check, lib, ptr
    Fn = _Fn()
    T = sum(chunks)
    g = torch.Generator().manual_seed(Bp * 7 + H)
    p = {k: v.to(DEV) for k, v in _cell_params(kind, H, g).items()}
    Wx = (torch.randn(Bp, T, H, generator=g) * 1.5 + 0.5).to(DEV)
    scale, shift = (torch.rand(H, generator=g) + 0.5).to(DEV), (torch.rand(H, generator=g) * 0.2).to(DEV)
    u0, s0 = torch.rand(Bp, H, generator=g).to(DEV), torch.rand(Bp, H, generator=g).to(DEV)
    w0 = torch.rand(Bp, H, generator=g).to(DEV) if kind == "adLIF" else None
    k = KIND[kind]
    s_w = torch.empty(Bp, T, H, device=DEV)
    s16_w = torch.empty(Bp, T, H, dtype=torch.bfloat16, device=DEV)
    u_save = torch.empty(Bp, T, H, device=DEV)
    w_save = torch.empty(Bp, T, H, device=DEV) if kind == "adLIF" else None
    cnt_w = torch.zeros(H, dtype=torch.int32, device=DEV)
    check(lib.sparch_cell_fwd(k, Bp, 1, T, H, ptr(Wx), ptr(scale), ptr(shift), ptr(p["alpha"]), ptr(p.get("beta")),
                              ptr(p.get("a")), ptr(p.get("b")), ptr(u0), ptr(w0), ptr(s0), 1.0, 0.0, 0, ptr(s_w),
                              ptr(s16_w), ptr(u_save), ptr(w_save), 0, ptr(cnt_w), Fn._stream()), "sparch_cell_fwd")
    assert 0.003 < float(s_w.mean()) < 0.9
    u, s = u0.clone(), s0.clone()
    w = None if w0 is None else w0.clone()
    cnt = torch.zeros(H, dtype=torch.int32, device=DEV)
    got, got16, t0 = [], [], 0
    for n in chunks:
        Wc = Wx[:, t0:t0 + n].clone()         # (an allocation of its own: 16-byte aligned)
        s_c = torch.empty(Bp, n, H, device=DEV)
        s16_c = torch.empty(Bp, n, H, dtype=torch.bfloat16, device=DEV)
        check(lib.sparch_cell_stream_fwd(k, Bp, 1, n, H, ptr(Wc), ptr(scale), ptr(shift), ptr(p["alpha"]),
                                         ptr(p.get("beta")), ptr(p.get("a")), ptr(p.get("b")), ptr(u), ptr(w), ptr(s), 1.0,
                                         0.0, ptr(s_c), ptr(s16_c), ptr(cnt), Fn._stream()), "sparch_cell_stream_fwd")
        got.append(s_c)
        got16.append(s16_c)
        t0 += n
    assert torch.equal(torch.cat(got, 1), s_w) and torch.equal(torch.cat(got16, 1), s16_w)
    assert torch.equal(u, u_save[:, -1]) and torch.equal(s, s_w[:, -1]) and torch.equal(cnt, cnt_w)
    if w is not None:
        assert torch.equal(w, w_save[:, -1])


@pytest.mark.parametrize("B,C", [(1, 5), (33, 35), (4, 256)])
def test_readout_stream_kernel_equals_whole_sequence_kernel(B, C):
    """out and u bit-equal: the accumulator is carried into the kernel (T = 300 crosses the kernel's own 256-step
    staging chunk as well)."""
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    T, chunks = 300, [1, 7, 250, 1, 41]
    g = torch.Generator().manual_seed(B + C)
    Wx = (torch.randn(B, T, C, generator=g) * 1.5).to(DEV)
    alpha = (torch.rand(C, generator=g) * 0.14 + 0.82).to(DEV)
    scale, shift = (torch.rand(C, generator=g) + 0.5).to(DEV), (torch.rand(C, generator=g) * 0.2).to(DEV)
    u0 = torch.rand(B, C, generator=g).to(DEV)
    out_w, u_save = torch.empty(B, C, device=DEV), torch.empty(B, T, C, device=DEV)
    check(lib.sparch_readout_fwd(B, T, C, ptr(Wx), ptr(scale), ptr(shift), ptr(alpha), ptr(u0), ptr(out_w), ptr(u_save),
                                 Fn._stream()), "sparch_readout_fwd")
    u, out, t0 = u0.clone(), torch.zeros(B, C, device=DEV), 0
    for n in chunks:
        Wc = Wx[:, t0:t0 + n].clone()         # (an allocation of its own: 16-byte aligned)
        check(lib.sparch_readout_stream_fwd(B, n, C, ptr(Wc), ptr(scale), ptr(shift), ptr(alpha), ptr(u), ptr(out),
                                            Fn._stream()), "sparch_readout_stream_fwd")
        t0 += n
    assert torch.equal(out, out_w) and torch.equal(u, u_save[:, -1])
    assert abs(float(out_w.sum()) - B * T) <= 1e-3 * B * T


def cell_net(sp, kind, H, p):
    """One hidden layer, no readout, identity projection (x * 1.0 is exact in the split product): the stream's
    input IS the cell's Wx."""
    torch.manual_seed(1)
    net = sp.SNN((1, None, H), [H], neuron_type=kind, dropout=0.0, normalization="none", use_readout_layer=False)
    lay = net.snn[0]
    with torch.no_grad():
        lay.W.weight.copy_(torch.eye(H))
        lay.alpha.copy_(p["alpha"])
        for k in ("beta", "a", "b"):
            if k in p:
                getattr(lay, k).copy_(p[k])
        if "V" in p:
            lay.V.weight.copy_(p["V"])
    return net.to(DEV).eval()


@pytest.mark.parametrize("kind,Bp,T,H", [("RLIF", 48, 60, 128), ("RadLIF", 96, 80, 256), ("RadLIF", 33, 40, 1024)])
def test_recurrent_stream_one_step_ahead_vs_oracle_trajectory(sp, kind, Bp, T, H):
    """Real-valued orthogonal V: teacher forcing, the yardstick of test_recurrent_one_step_ahead_vs_oracle_trajectory.
    A stream is started at every t from the oracle's exact (u, w, s)_{t-1} via set_state and run for two one-step
    chunks: the first takes the dense boundary product, the second the exact spike product on the carried bf16
    plane.  A spike may differ only where the oracle's |u - 1| <= 1e-4; flips <= 1e-4 N + 2."""
    Fn = _Fn()
    g = torch.Generator().manual_seed(17 + H)
    V = torch.nn.init.orthogonal_(torch.empty(H, H), generator=g)
    Wx = torch.randn(Bp, T, H, generator=g) * 1.5 + 0.5
    p = {"alpha": torch.rand(H, generator=g) * 0.14 + 0.82, "V": V}
    if kind == "RadLIF":
        p.update(beta=torch.rand(H, generator=g) * 0.024 + 0.967, a=torch.rand(H, generator=g) * 2 - 1,
                 b=torch.rand(H, generator=g) * 2)
    u0, s0 = torch.rand(Bp, H, generator=g), torch.rand(Bp, H, generator=g)
    w0 = torch.rand(Bp, H, generator=g) if kind == "RadLIF" else None
    pn = {k: v.numpy() for k, v in p.items()}
    S, U, W = bp.cell_forward(kind, Wx.numpy(), pn, u0.numpy(), None if w0 is None else w0.numpy(), s0.numpy())
    assert S.mean() > 0.003
    ts = np.arange(1, T - 1)
    state = {"u": torch.from_numpy(U[:, ts - 1].reshape(-1, H).copy()),
             "s": torch.from_numpy(S[:, ts - 1].reshape(-1, H).copy())}
    if W is not None:
        state["w"] = torch.from_numpy(W[:, ts - 1].reshape(-1, H).copy())
    Wx2 = torch.from_numpy(np.stack([Wx.numpy()[:, ts], Wx.numpy()[:, ts + 1]], axis=2).reshape(-1, 2, H).copy()).to(DEV)
    ref_s = np.stack([S[:, ts], S[:, ts + 1]], axis=2).reshape(-1, 2, H)
    ref_u = np.stack([U[:, ts], U[:, ts + 1]], axis=2).reshape(-1, 2, H)
    st = sp.StreamingSNN(cell_net(sp, kind, H, p), Wx2.shape[0])
    st.set_state([state])
    s = torch.cat([st.step(Wx2[:, 0:1]), st.step(Wx2[:, 1:2])], dim=1).cpu().numpy()
    Fn.check_status()
    diff = s != ref_s
    n0, n1 = int(diff[:, 0].sum()), int(diff[:, 1].sum())
    if diff[:, 0].any():
        assert np.abs(ref_u[:, 0][diff[:, 0]] - 1.0).max() <= 1e-4
    ok_rows = ~diff[:, 0].any(axis=1)       # step 1 inherits step 0's (legitimate) flips
    d1 = diff[:, 1] & ok_rows[:, None]
    if d1.any():
        assert np.abs(ref_u[:, 1][d1] - 1.0).max() <= 1e-4
    print(f"{kind} H={H}: {n0}+{n1} near-threshold flips in {ref_s.size} spikes")
    assert (n0 + n1) <= 1e-4 * ref_s.size + 2


# ------------------------------------------------------------------------------------------ 4. geometry
@pytest.mark.parametrize("kind,Bp,T,H,chunk", [("RadLIF", 256, 250, 1024, 10), ("RadLIF", 1, 30, 64, 7),
                                               ("RLIF", 33, 30, 96, 4), ("RadLIF", 5, 12, 1536, 5),
                                               ("RLIF", 9, 20, 130, 3), ("RadLIF", 40, 20, 130, 20)])
def test_recurrent_stream_geometries_vs_oracle(sp, kind, Bp, T, H, chunk):
    """Dyadic V (every s @ V sum exact in any order): spikes equal oracle.spiking_cell.  (256, 1024) is the headline
    launch shape, its state carried 25 times; H = 1536 takes the step path, H = 130 the zero-padded one."""
    Fn = _Fn()
    Wx, p, u0, w0, s0 = _dyadic_cell_case(kind, Bp, T, H, 11 + H)
    with torch.no_grad():
        ref = orc.spiking_cell(kind, Wx, p, u0, w0, s0)
    assert ref.sum() > 0
    st = sp.StreamingSNN(cell_net(sp, kind, H, p), Bp)
    state = {"u": u0, "s": s0}
    if w0 is not None:
        state["w"] = w0
    st.set_state([state])
    chunks = [chunk] * (T // chunk) + ([T % chunk] if T % chunk else [])
    outs, rec = run_stream(st, Wx.to(DEV), chunks)
    Fn.check_status()
    s = torch.cat(outs, dim=1).cpu()
    assert torch.equal(s, ref), float((s != ref).float().mean())
    assert torch.equal(rec[0], ref)                                   # the bf16 plane says the same
    got = st.get_state()[0]
    assert got["u"].shape == (Bp, H) and torch.equal(got["s"].cpu(), ref[:, -1])
    assert torch.equal(st.firing_rates().cpu(), ref.sum(dim=(0, 1)).to(torch.int32) * (1.0 / float(Bp * T)))


# ------------------------------------------------------------------------------------------ 5. row reset
def test_reset_rows_mid_stream(sp):
    Fn = _Fn()
    cfg, x, y, params, init, z = snn_case("dyadic_RadLIF_none")
    B, T = cfg["B"], cfg["T"]
    net = _build(sp, cfg, params).eval()
    xd = x.to(DEV)
    rows, half = [1, 3], 20
    fresh = [{k: torch.floor(v * 16) / 16 for k, v in stt.items()}
             for stt in orc.draw_init_states(len(rows), cfg["layer_sizes"], cfg["neuron_type"])]
    x2 = (torch.rand(len(rows), T - half, cfg["C"], generator=torch.Generator().manual_seed(8)) < 0.3).float().to(DEV)

    plain = sp.StreamingSNN(net, B)                       # the undisturbed stream
    plain.reset(states=init)
    outs_plain, rec_plain = run_stream(plain, xd, [5] * (T // 5))

    small = sp.StreamingSNN(net, len(rows))               # a fresh stream of the two rows alone
    small.reset(states=fresh)
    outs_small, rec_small = run_stream(small, x2, [5] * ((T - half) // 5))

    st = sp.StreamingSNN(net, B)
    st.reset(states=init)
    run_stream(st, xd[:, :half], [5] * (half // 5))
    st.reset(states=fresh, rows=rows)
    assert list(st.row_steps) == [half, 0, half, 0] + [half] * (B - 4) and st.steps_seen == half
    x_mix = xd[:, half:].clone()
    x_mix[rows] = x2
    outs, rec = run_stream(st, x_mix, [5] * ((T - half) // 5))
    Fn.check_status()
    others = [r for r in range(B) if r not in rows]
    assert torch.equal(outs[-1][rows], outs_small[-1]) and torch.equal(outs[-1][others], outs_plain[-1][others])
    for k in rec:
        assert float(rec_small[k].sum()) > 0
        assert torch.equal(rec[k][rows], rec_small[k])
        assert torch.equal(rec[k][others], rec_plain[k][others, half:])
    assert list(st.row_steps) == [T, T - half, T, T - half] + [T] * (B - 4)


# ------------------------------------------------------------------------------------------ 6. footprint
@pytest.mark.parametrize("kind", ["LIF", "adLIF", "RadLIF"])
def test_stream_footprint_does_not_grow_and_keeps_no_state_tensors(sp, kind):
    """Peak allocated bytes of 100 chunk steps equal those of 10; under exact-size guarded allocations (the pattern
    of test_footprint_gpu.py) the results are the same bits, no guard byte is touched, and no fp32 tensor of a
    layer's (B,Tc,H) size is allocated by the streaming module at all — the projection (made by the GEMM wrapper)
    is the only one per layer."""
    from sparch_amd import streaming
    Fn = _Fn()
    B, Tc, C, sizes = 8, 10, 64, [64, 128, 20]
    net, init = dyadic_net(sp, kind, B, C, sizes, "batchnorm", 31)
    g = torch.Generator().manual_seed(6)
    xs = [(torch.rand(B, Tc, C, generator=g) < 0.3).float().to(DEV) for _ in range(4)]
    st = sp.StreamingSNN(net, B)
    st.reset(states=init)
    for i in range(3):
        st.step(xs[i % 4])
    torch.cuda.synchronize()

    def peak(n):
        torch.cuda.reset_peak_memory_stats()
        for i in range(n):
            st.step(xs[i % 4])
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated()

    p10, p100 = peak(10), peak(100)
    assert p100 == p10, (p10, p100)

    def run():
        st.reset(states=init)
        return [st.step(xs[i]) for i in range(4)] + [st.firing_rates()]

    Fn.status_word(DEV)
    with guard_arena(Fn) as arena_fn, guard_arena(streaming) as arena_st:
        got = [t.cpu() for t in run()]
        torch.cuda.synchronize()
        Fn.check_status()
    ref = [t.cpu() for t in run()]
    for a, b in zip(ref, got):
        assert not bool(torch.isnan(b).any()) and torch.equal(a, b)
    big = {B * Tc * h for h in sizes[:-1]}
    mine = [a for a in arena_st.allocs if a[3] == torch.float32 and int(np.prod(a[2])) in big]
    assert len(arena_st.allocs) > 0 and not mine, mine
    state_like = [a for a in arena_fn.allocs + arena_st.allocs
                  if a[3] == torch.float32 and tuple(a[2]) in {(B, Tc, h) for h in sizes[:-1]}]
    assert not state_like, state_like
    proj = [a for a in arena_fn.allocs if a[3] == torch.float32 and tuple(a[2]) in {(B * Tc, h) for h in sizes[:-1]}]
    assert len(proj) == 4 * len(sizes[:-1]), proj             # one projection per hidden layer and chunk step


# ------------------------------------------------------------------------------------------ 7. filterbank
def _random_cuts(N, rng, hi):
    cuts, left = [], N
    while left > 0:
        n = int(min(left, rng.integers(1, hi)))
        cuts.append(n)
        left -= n
    return cuts


@pytest.mark.parametrize("N", [399, 400, 16000, 16001])
def test_streaming_fbank_equals_whole_clip(sp, N):
    Fn = _Fn()
    B = 3
    wave = (torch.rand(B, N, generator=torch.Generator().manual_seed(N)) * 2 - 1).to(DEV)
    ref = Fn.fbank(wave) if N >= 400 else torch.empty(B, 0, 40, device=DEV)
    rng = np.random.default_rng(N)
    for hi in (200, 700, 5000):
        fb = sp.StreamingFbank(B)
        parts, t0 = [], 0
        for n in _random_cuts(N, rng, hi):
            parts.append(fb.push(wave[:, t0:t0 + n]))
            assert fb.tail.shape[1] <= 399
            t0 += n
        got = torch.cat(parts, dim=1)
        assert got.shape == ref.shape and torch.equal(got, ref)


def test_streaming_fbank_into_streaming_snn_equals_forward_on_whole_clip(sp):
    Fn = _Fn()
    B, N, sizes = 4, 16000, [64, 64, 10]
    net, init = dyadic_net(sp, "RadLIF", B, 40, sizes, "none", 55)
    clip = (torch.rand(B, N, generator=torch.Generator().manual_seed(2)) * 2 - 1).to(DEV)
    order = [st[k] for st in init for k in ("u0", "w0", "s0") if k in st]
    out_w, rates_w, rec_w = whole_forward(net, Fn.fbank(clip), order)
    assert all(float(v.sum()) > 0 for v in rec_w.values())
    fb, st = sp.StreamingFbank(B), sp.StreamingSNN(net, B)
    st.reset(states=init)
    out, t0 = None, 0
    for n in _random_cuts(N, np.random.default_rng(4), 3000):
        feats = fb.push(clip[:, t0:t0 + n])
        t0 += n
        if feats.shape[1]:
            out = st.step(feats)
    Fn.check_status()
    assert st.steps_seen == 98
    assert torch.equal(out, out_w) and torch.equal(st.firing_rates(), rates_w)
