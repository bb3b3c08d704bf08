"""
Does every kernel of the compute core stay inside the bytes it was given?

GPU AddressSanitizer is not available to this project, and every workspace the Python wrappers allocate comes from
torch's caching allocator, which rounds a request up to 512 bytes and pools it: a *_bytes query that under-reports by
a few words, or a kernel that stores one row too far, cannot be noticed there.  Here each path runs twice on the same
inputs — once on ordinary allocations, once with sparch_amd.functional allocating EXACT-size, 256-byte-aligned slices
of a pre-filled guard arena (tests/guarded.py) — and must
  * return bit-identical outputs (a kernel that read fill, or whose result depends on what lies behind a buffer,
    differs),
  * leave every guard byte of the arena untouched,
  * leave no NaN in any output (the arena's "uninitialised" memory is NaN: whatever is returned was written).
Shapes are the smallest the parity tests use for each path, bent so that H % 4 != 0, M % 4 != 0 and Bp % 32 != 0 occur.
This runs at exact size: sparch_bn_bwd_workspace_bytes, sparch_vpack_bytes, sparch_rec_chan_bytes,
sparch_ligru_vpack_bytes / _chan_bytes, sparch_gru_vpack_bytes / _chan_bytes, the three GEMM workspace queries and the
2 * ceil(M/128) * N colstat formula.
"""
import ctypes

import pytest
import torch

from tests.guarded import guard_arena
from tests.kit import DEV
from tests.kit import Fn as _Fn

pytestmark = pytest.mark.gpu


def _flat(out):
    """Every tensor of a nested result, in order, on the CPU."""
    if torch.is_tensor(out):
        return [out.detach().cpu()]
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in _flat(out[k])]
    if isinstance(out, (list, tuple)):
        return [t for o in out for t in _flat(o)]
    return []


def both_ways(fn, nbytes=64 << 20, min_allocs=1):
    """fn() under the guarded allocator, then on ordinary allocations: guards intact, same bits, no NaN.  (The guarded
    run comes first: a kernel that overruns a buffer is then stopped by the arena's check before it ever runs on
    memory the test does not own.)"""
    Fn = _Fn()
    Fn.status_word(DEV)                     # (cached per device: made before the arena exists)
    with guard_arena(Fn, nbytes=nbytes) as arena:
        got = _flat(fn())
        torch.cuda.synchronize()
        Fn.check_status()
    ref = _flat(fn())
    torch.cuda.synchronize()
    assert len(arena.allocs) >= min_allocs, "the path under test allocated nothing through sparch_amd.functional"
    assert len(ref) == len(got) and len(got) > 0
    for i, (a, b) in enumerate(zip(ref, got)):
        assert a.shape == b.shape and a.dtype == b.dtype
        if b.dtype.is_floating_point:
            assert not bool(torch.isnan(b.float()).any()), f"output {i}: NaN under the guarded allocator"
        assert torch.equal(a, b), f"output {i}: differs from the run on ordinary allocations"
    return arena


# ------------------------------------------------------------------------------------------ normalisation
@pytest.mark.parametrize("M,H,K", [(37, 30, 41), (300, 64, 70), (515, 36, 33)])
def test_batchnorm_forward_backward_footprint(M, H, K):
    Fn = _Fn()
    g = torch.Generator().manual_seed(M + H)
    x = (torch.rand(M, K, generator=g) < 0.2).float().to(DEV)
    W, bias = (torch.randn(H, K, generator=g) * 0.2).to(DEV), (torch.randn(H, generator=g) * 0.1).to(DEV)
    gamma, beta = (torch.rand(H, generator=g) + 0.5).to(DEV), (torch.randn(H, generator=g) * 0.1).to(DEV)
    dy = torch.randn(M, H, generator=g).to(DEV)
    dy2 = torch.randn(M, H, generator=g).to(DEV)

    def fn():
        rm, rv = torch.zeros(H, device=DEV), torch.ones(H, device=DEV)
        nbt = torch.zeros((), dtype=torch.int64, device=DEV)
        Wx_raw, ws = Fn.gemm_nt(x, W, bias, colstat=True)
        y, scale, shift, saved = Fn._Norm.forward("batchnorm", Wx_raw, ws, gamma, beta, rm, rv, True, 1, nbt=nbt)
        out = [Wx_raw, ws, scale, shift, saved, rm, rv, nbt]
        out.append(Fn._Norm.backward("batchnorm", dy.clone(), Wx_raw, gamma, saved, True))
        if H % 8 == 0:
            out.append(Fn._Norm.backward("batchnorm", dy.clone(), Wx_raw, gamma, saved, True, planes=True, dy2=dy2))
            dxn, dg, db, planes = Fn._Norm.backward("batchnorm", dy.clone(), Wx_raw, gamma, saved, True, planes=True,
                                                    keep_fp32=False)
            out += [dg, db, planes.view(torch.int16)]
        out.append(Fn._Norm.backward("batchnorm", dy.clone(), Wx_raw, gamma, saved, False))   # eval: fixed statistics
        return out

    both_ways(fn, min_allocs=8)


@pytest.mark.parametrize("M,H,Hn", [(37, 36, 30), (300, 64, 64), (5, 30, 30)])
def test_layernorm_forward_backward_footprint(M, H, Hn):
    Fn = _Fn()
    g = torch.Generator().manual_seed(M + H + Hn)
    x = torch.randn(M, H, generator=g)
    x[:, Hn:] = 0
    x = x.to(DEV)
    gamma, beta = (torch.rand(H, generator=g) + 0.5).to(DEV), (torch.randn(H, generator=g) * 0.1).to(DEV)
    dy = torch.randn(M, H, generator=g).to(DEV)

    def fn():
        y, _, _, saved = Fn._Norm.forward("layernorm", x, None, gamma, beta, None, None, True, 1, ln_width=Hn)
        return [y, saved, Fn._Norm.backward("layernorm", dy.clone(), x, gamma, saved, True, ln_width=Hn)]

    both_ways(fn, min_allocs=7)


@pytest.mark.parametrize("M,H", [(37, 30), (300, 64), (257, 7), (1, 5)])
def test_colsum_footprint(M, H):
    Fn = _Fn()
    x = torch.randn(M, H, generator=torch.Generator().manual_seed(M)).to(DEV)
    arena = both_ways(lambda: Fn._colsum(x), min_allocs=2)
    from sparch_amd._capi import lib
    assert arena.allocs[1][1] == lib.sparch_bn_bwd_workspace_bytes(M, H)


# ------------------------------------------------------------------------------------------ spiking cells
def _cell_case(kind, Bp, T, H, seed):
    g = torch.Generator().manual_seed(seed)
    rec, adaptive = kind in ("RLIF", "RadLIF"), kind in ("adLIF", "RadLIF")
    p = {"alpha": torch.rand(H, generator=g) * 0.2 + 0.78}
    if adaptive:
        p.update(beta=torch.rand(H, generator=g) * 0.05 + 0.95, a=torch.rand(H, generator=g) * 2.4 - 1.2,
                 b=torch.rand(H, generator=g) * 2.4 - 0.2)
    if rec:
        p["V"] = torch.randint(-24, 25, (H, H), generator=g).float() / 64.0
    Wx = torch.randn(Bp, T, H, generator=g) * 1.5 + 0.4
    u0 = torch.rand(Bp, H, generator=g)
    w0 = torch.rand(Bp, H, generator=g) if adaptive else None
    s0 = (torch.rand(Bp, H, generator=g) < 0.3).float()
    g_s = torch.randn(Bp, T, H, generator=g)
    return Wx, p, u0, w0, s0, g_s


def _cell_fn(kind, case, spl):
    Fn = _Fn()
    Wx, p, u0, w0, s0, g_s = [c.to(DEV) if torch.is_tensor(c) else c for c in case]
    p = {k: v.to(DEV) for k, v in p.items()}
    w0 = None if w0 is None else w0

    def fn():
        pd = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        Wxd = Wx.clone().requires_grad_(True)
        s = Fn.SpikingCellFn.apply(kind, 1.0, Wxd, pd["alpha"], pd.get("beta"), pd.get("a"), pd.get("b"), pd.get("V"),
                                   u0, w0, s0, spl)
        (s * g_s).sum().backward()
        return [s, Wxd.grad, {k: v.grad for k, v in pd.items()}]
    return fn


@pytest.mark.parametrize("kind,Bp,T,H", [("LIF", 5, 9, 30), ("adLIF", 5, 9, 30), ("LIF", 33, 7, 64), ("adLIF", 6, 40, 64)])
def test_non_recurrent_cell_footprint(kind, Bp, T, H):
    both_ways(_cell_fn(kind, _cell_case(kind, Bp, T, H, 3), None), min_allocs=5)


@pytest.mark.parametrize("spl", [None, 1, 7])
@pytest.mark.parametrize("kind,Bp,T,H", [("RLIF", 5, 9, 66), ("RadLIF", 5, 9, 66), ("RadLIF", 40, 9, 36), ("RLIF", 5, 33, 64)])
def test_recurrent_cell_persistent_footprint(kind, Bp, T, H, spl):
    """vpack / rec_chan at exactly the queried bytes; whole-sequence launches, one launch per step, 7-step chunks."""
    both_ways(_cell_fn(kind, _cell_case(kind, Bp, T, H, 4), spl), min_allocs=8)


@pytest.mark.parametrize("kind,Bp,T,H", [("RadLIF", 33, 5, 1028), ("RLIF", 3, 4, 1030)])
def test_recurrent_cell_step_path_footprint(kind, Bp, T, H):
    """H > 1024: one launch per step with the recurrent product on the GEMMs between them."""
    both_ways(_cell_fn(kind, _cell_case(kind, Bp, T, H, 5), None), nbytes=256 << 20, min_allocs=8)


@pytest.mark.parametrize("B,T,C", [(3, 1, 5), (5, 17, 7), (4, 300, 35), (9, 64, 64)])
def test_readout_cell_footprint(B, T, C):
    Fn = _Fn()
    g = torch.Generator().manual_seed(B + T + C)
    Wx = (torch.randn(B, T, C, generator=g) * 1.5).to(DEV)
    alpha = (torch.rand(C, generator=g) * 0.3 + 0.72).to(DEV)
    u0, g_out = torch.rand(B, C, generator=g).to(DEV), torch.randn(B, C, generator=g).to(DEV)

    def fn():
        Wd, ad = Wx.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
        out = Fn.ReadoutCellFn.apply(Wd, ad, u0)
        (out * g_out).sum().backward()
        return [out, Wd.grad, ad.grad]

    both_ways(fn, min_allocs=4)


# ------------------------------------------------------------------------------------------ ANN baseline layers
@pytest.mark.parametrize("path", ["persistent", "per_step_launches", "launch_per_step"])
@pytest.mark.parametrize("kind,bidir,norm", [("RNN", False, "batchnorm"), ("RNN", True, "layernorm"),
                                             ("LiGRU", True, "batchnorm"), ("LiGRU", False, "layernorm"),
                                             ("GRU", False, "batchnorm"), ("GRU", True, "batchnorm")])
def test_ann_layers_footprint(kind, bidir, norm, path, monkeypatch):
    """The RNN, LiGRU and GRU layers, forward and backward: persistent kernels (whole sequence / one launch per
    step: SPARCH_REC_STEPS_PER_LAUNCH=1) and the launch-per-step path with the recurrent products on the GEMMs.
    B * T = 35 rows (M % 4 != 0), Bp = 5 or 10 (Bp % 32 != 0)."""
    from sparch_amd import anns

    monkeypatch.setenv("SPARCH_REC_STEPS_PER_LAUNCH", "1" if path == "per_step_launches" else "")
    if path == "launch_per_step":
        monkeypatch.setenv({"RNN": "SPARCH_REC_STEP_PATH", "LiGRU": "SPARCH_LIGRU_PERSISTENT",
                            "GRU": "SPARCH_GRU_PERSISTENT"}[kind], "1" if kind == "RNN" else "0")
    B, T, C, H = 5, 7, 12, 32
    torch.manual_seed(41)
    cls = {"RNN": anns.RNNLayer, "LiGRU": anns.LiGRULayer, "GRU": anns.GRULayer}[kind]
    layer = cls(C, H, B, dropout=0.0, normalization=norm, use_bias=(norm == "layernorm"), bidirectional=bidir)
    layer = layer.to(DEV).train()
    state = {k: v.clone() for k, v in layer.state_dict().items()}
    g = torch.Generator().manual_seed(42)
    x = torch.randn(B, T, C, generator=g).to(DEV)
    gy = torch.randn(B, T, H * (2 if bidir else 1), generator=g).to(DEV)

    def fn():
        layer.load_state_dict(state)        # (BatchNorm's running statistics move with every training pass)
        layer.zero_grad()
        xd = x.clone().requires_grad_(True)
        y = layer(xd)
        (y * gy).sum().backward()
        return [y, xd.grad, {k: v.grad for k, v in layer.named_parameters()},
                {k: v for k, v in layer.state_dict().items() if "running" in k}]

    both_ways(fn, min_allocs=10)


# ------------------------------------------------------------------------------------------ element-wise / loss / Adam
@pytest.mark.parametrize("p_drop", [0.0, 0.25])
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("M,H", [(37, 52), (1, 4)])
def test_act_kernels_footprint(kind, p_drop, M, H):
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    g = torch.Generator().manual_seed(3)
    z, dy = (torch.randn(M, H, generator=g) * 2).to(DEV), torch.randn(M, H, generator=g).to(DEV)
    sc, sh = (torch.rand(H, generator=g) + 0.5).to(DEV), (torch.randn(H, generator=g) * 0.3).to(DEV)

    def fn():
        y, dz = Fn.torch.empty(M, H, dtype=torch.float32, device=DEV), Fn.torch.empty(M, H, dtype=torch.float32, device=DEV)
        check(lib.sparch_act_fwd(kind, M * H, H, ptr(z), ptr(sc), ptr(sh), p_drop, 99, ptr(y), Fn._stream()), "act_fwd")
        check(lib.sparch_act_bwd(kind, M * H, H, ptr(z), ptr(sc), ptr(sh), ptr(dy), p_drop, 99, ptr(dz), Fn._stream()),
              "act_bwd")
        return [y, dz]

    both_ways(fn, min_allocs=2)


@pytest.mark.parametrize("B,T,K", [(3, 17, 48), (1, 1, 4), (2, 9, 2052)])
def test_softmax_sum_footprint(B, T, K):
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    g = torch.Generator().manual_seed(B * 100 + T)
    x, gy = (torch.randn(B, T, K, generator=g) * 3).to(DEV), torch.randn(B, K, generator=g).to(DEV)

    def fn():
        out = Fn.torch.empty(B, K, dtype=torch.float32, device=DEV)
        dx = Fn.torch.empty(B, T, K, dtype=torch.float32, device=DEV)
        check(lib.sparch_softmax_sum_fwd(B, T, K, ptr(x), ptr(out), Fn._stream()), "softmax_sum_fwd")
        check(lib.sparch_softmax_sum_bwd(B, T, K, ptr(x), ptr(gy), ptr(dx), Fn._stream()), "softmax_sum_bwd")
        return [out, dx]

    both_ways(fn, min_allocs=2)


@pytest.mark.parametrize("B,C", [(1, 2), (37, 35), (300, 20), (5, 257)])
def test_ce_loss_footprint(B, C):
    Fn = _Fn()
    g = torch.Generator().manual_seed(B + C)
    x = (torch.randn(B, C, generator=g) * 3.0).to(DEV)
    y = torch.randint(0, C, (B,), generator=g).to(DEV)

    def fn():
        xd = x.clone().requires_grad_(True)
        loss = Fn.CrossEntropyLoss()(xd, y)
        (loss * 1.5).backward()
        return [loss, xd.grad]

    both_ways(fn, min_allocs=2)


def test_adam_step_footprint():
    """One launch over tensors of odd sizes, each parameter / gradient / moment an exact-size slice."""
    from sparch_amd._capi import check, lib
    Fn = _Fn()
    g = torch.Generator().manual_seed(5)
    shapes = [(3,), (1,), (4097,), (17, 5), (35, 30), (2, 1)] + [(7,)] * 26     # more than one batch of tensors
    init = [[torch.randn(*s, generator=g) for s in shapes] for _ in range(2)] + \
           [[torch.rand(*s, generator=g) * 0.01 for s in shapes] for _ in range(2)]

    def fn():
        sets = []
        for group in init:
            ts = []
            for t in group:
                d = Fn.torch.empty(*t.shape, dtype=torch.float32, device=DEV)
                d.copy_(t)
                ts.append(d)
            sets.append(ts)
        n = len(shapes)
        arr = ctypes.c_void_p * n
        ptrs = [arr(*[t.data_ptr() for t in ts]) for ts in sets]
        numel = (ctypes.c_int64 * n)(*[t.numel() for t in sets[0]])
        for step in (1, 2):
            check(lib.sparch_adam_step(n, ptrs[0], ptrs[1], ptrs[2], ptrs[3], numel, 1e-2 / (1 - 0.9 ** step), 0.9, 0.999,
                                       (1 - 0.999 ** step) ** 0.5, 1e-8, 1e-4, None, Fn.status_word(DEV).data_ptr(),
                                       Fn._stream()), "sparch_adam_step")
        return [sets[0], sets[2], sets[3]]

    both_ways(fn, min_allocs=4 * len(shapes))
