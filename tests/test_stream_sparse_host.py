"""CPU: the event-driven fused streaming step (csrc/streamsparse.hip, StreamingSNN(fused=True, sparse=True)) — what it
refuses, and its summation order, without a device.

* both entry points are bound, leave the ABI version alone, and return their error code for every bad argument before
  anything is dereferenced or launched (the pattern of test_stream_fused_host.py);
* the constructor refusals;
* `sparse_numpy.sparse_dot` (the kernel's documented order) equals an fp64 product bit for bit on dyadic data;
* that order stays inside the teacher-forced bars of the real-valued GPU test: one step from the oracle's
  (u, w, s)_{t-1} with `sparse_dot` for both products, on two of that test's cases.
"""
import numpy as np
import pytest
import torch

from oracle import bptt_numpy as bp
from tests.sparse_numpy import active_list, sparse_dot

P = 16   # any non-NULL, 16-byte aligned value: nothing is dereferenced before the checks
Q = 32   # another one


def test_sparse_entry_points_validate_without_launching():
    from sparch_amd import _capi
    lib = _capi.lib
    assert "sparch_stream_step_sparse_fwd" in _capi.PROTOTYPES
    assert "sparch_stream_step_sparse_readout" in _capi.PROTOTYPES

    def step(kind=3, B=2, K=12, H=8, ld=8, in_dtype=0, x=P, ldx=12, Wt=P, ldw=8, scale=None, shift=None, alpha=P,
             beta=P, a=P, b=P, vmask=P, u=P, w=P, s_in=P, s_out=Q):
        return lib.sparch_stream_step_sparse_fwd(kind, B, K, H, ld, in_dtype, x, ldx, Wt, ldw, None, scale, shift, alpha,
                                                 beta, a, b, vmask, u, w, s_in, s_out, None, 1.0, None, None)

    assert step(kind=4) == -1 and step(kind=-1) == -1                      # unknown kind
    assert step(in_dtype=2) == -1 and step(in_dtype=-1) == -1              # unknown input type
    for name in ("x", "Wt", "alpha", "u", "s_in", "s_out"):                # a required pointer is NULL
        assert step(**{name: None}) == -1, name
    for kind in (1, 3):                                                     # adLIF / RadLIF without an adaptive pointer
        for name in ("beta", "a", "b", "w"):
            assert step(kind=kind, **{name: None}) == -1, (kind, name)
    for kind in (2, 3):                                                     # RLIF / RadLIF
        assert step(kind=kind, vmask=None) == -1                           # ... without the masked V
        assert step(kind=kind, s_out=P) == -1                              # ... writing the spikes it reads
    assert step(scale=P) == -1 and step(shift=P) == -1                     # half an affine map
    assert step(ld=7) == -1 and step(ldx=11) == -1                         # strides below the widths
    assert step(ldw=4) == -1 and step(H=6, ld=6, ldw=6) == -1              # Wt's stride: below H / no multiple of 4
    assert step(B=0) == -1 and step(K=0) == -1 and step(H=0) == -1
    assert step(u=24) == -2 and step(Wt=20) == -2 and step(s_out=40) == -2 and step(vmask=20) == -2   # SPARCH_EALIGN
    assert step(u=24, x=None) == -1                                        # ... after every EINVAL check

    def ro(B=2, K=12, C=5, x=P, ldx=12, Wt=P, ldc=8, scale=None, shift=None, alpha=P, u=P, out=P):
        return lib.sparch_stream_step_sparse_readout(B, K, C, x, ldx, Wt, ldc, None, scale, shift, alpha, u, out, None)

    assert ro(C=257, ldc=260) == -1 and ro(C=0) == -1 and ro(B=0) == -1 and ro(K=0) == -1 and ro(ldx=11) == -1
    assert ro(ldc=4) == -1 and ro(ldc=6) == -1                             # Wt's stride: below C / no multiple of 4
    for name in ("x", "Wt", "alpha", "u", "out"):
        assert ro(**{name: None}) == -1, name
    assert ro(scale=P) == -1 and ro(shift=P) == -1
    assert ro(Wt=20) == -2
    assert lib.sparch_abi_version() == 5        # additive: the ABI version stays


def test_sparse_constructor_on_cpu_parameters_and_its_refusals():
    import sparch_amd

    torch.manual_seed(3)
    net = sparch_amd.SNN((4, None, 12), [16, 16, 5], neuron_type="RadLIF", dropout=0.1)
    with pytest.raises(ValueError, match="training mode"):
        sparch_amd.StreamingSNN(net, 4, fused=True, sparse=True)
    net = net.eval()
    with pytest.raises(ValueError, match="fused=True"):
        sparch_amd.StreamingSNN(net, 4, sparse=True)                        # sparse is a form of the fused step
    with pytest.raises(ValueError, match="fused=True"):
        sparch_amd.StreamingSNN(net, 4, graph=True, sparse=True)
    for graph in (False, True):
        st = sparch_amd.StreamingSNN(net, 4, graph=graph, fused=True, sparse=True)   # CPU parameters: fine until used
        assert st.fused and st.sparse and st.fused_active and st.sparse_active and st.steps_seen == 0
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            st.reset()
    dense = sparch_amd.StreamingSNN(net, 4, fused=True)
    assert dense.fused_active and not dense.sparse and not dense.sparse_active
    plain = sparch_amd.StreamingSNN(net, 4)
    assert not plain.sparse and not plain.sparse_active
    with pytest.raises(AttributeError):
        plain.sparse_active = True              # read-only
    ln = sparch_amd.SNN((4, None, 12), [16, 16, 5], neuron_type="adLIF", dropout=0.1, normalization="layernorm").eval()
    with pytest.raises(ValueError, match="LayerNorm"):
        sparch_amd.StreamingSNN(ln, 4, fused=True, sparse=True)
    bi = sparch_amd.SNN((4, None, 12), [16, 16, 5], neuron_type="RadLIF", dropout=0.1, bidirectional=True).eval()
    with pytest.raises(ValueError, match="not causal"):
        sparch_amd.StreamingSNN(bi, 4, fused=True, sparse=True)


def test_sparse_step_takes_the_chunk_path_in_the_bf16_operand_mode():
    import sparch_amd
    from sparch_amd import functional as Fn

    torch.manual_seed(3)
    net = sparch_amd.SNN((4, None, 12), [16, 16, 5], neuron_type="RadLIF", dropout=0.1).eval()
    prev = Fn.set_compute_dtype("bf16")
    try:
        st = sparch_amd.StreamingSNN(net, 4, fused=True, sparse=True)
        assert st.sparse and not st.fused_active and not st.sparse_active
    finally:
        Fn.set_compute_dtype(prev)


# ------------------------------------------------------------------------------------------ the summation order
def test_active_list_keeps_values_in_ascending_position():
    k, v = active_list(np.array([0, 2, 0, 0, 0.5, -0.0, 1, 0], np.float32))
    assert k.tolist() == [1, 4, 6] and v.tolist() == [2.0, 0.5, 1.0]
    k, v = active_list(np.zeros(9, np.float32))
    assert k.size == 0 and v.size == 0


@pytest.mark.parametrize("ways", [1, 4])
def test_sparse_dot_equals_fp64_product_on_dyadic_data(ways):
    rng = np.random.default_rng(5)
    K, H = 1030, 67
    Wt = (rng.integers(-24, 25, (K, H)) / 64.0).astype(np.float32)
    X = np.zeros((6, K), np.float32)
    X[1] = 1.0                                                              # an all-ones row (row 0: all zero)
    X[2] = rng.random(K) < 0.05
    X[3] = rng.integers(0, 4, K) * (rng.random(K) < 0.3)                    # counts above 1
    X[4] = np.floor(rng.random(K) * 16) / 16                                # a dyadic state, every position active
    X[5, K - 1] = 3.0                                                       # one entry, the last position
    assert X[3].max() > 1 and X[2].sum() > 0
    ref = X.astype(np.float64) @ Wt.astype(np.float64)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)   # (exact in fp32, hence in any order)
    got = sparse_dot(X, Wt, ways=ways)
    assert got.dtype == np.float32 and np.array_equal(got, ref.astype(np.float32))
    assert not got[0].any() and got[1].any()


def real_case(kind, B, T, K, H, inp):
    """The data of test_stream_fused_gpu.test_fused_step_one_step_ahead_vs_oracle_trajectory, drawn the same way."""
    g = torch.Generator().manual_seed(17 + H + K)
    if inp == "binary":
        x, ex2 = (torch.rand(B, T, K, generator=g) < 0.15).float(), 0.15
    else:
        x, ex2 = torch.rand(B, T, K, generator=g), 1.0 / 3.0
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
    return x, W, p, u0, w0, s0


@pytest.mark.parametrize("kind,B,T,K,H,inp", [("RadLIF", 16, 40, 200, 256, "binary"), ("RLIF", 7, 40, 100, 130, "real")])
def test_emulated_order_stays_inside_the_teacher_forced_bars(kind, B, T, K, H, inp):
    """One step from the oracle's (u, w, s)_{t-1} for every t, W x and s V in the kernel's order (`sparse_dot`), the
    pointwise update in fp32 as the kernel writes it.  The bars of the GPU test: a spike may differ only where the
    oracle's |u - 1| <= 1e-4; flips <= 1e-4 N + 2; oracle rate > 0.003."""
    f32 = np.float32
    x, W, p, u0, w0, s0 = real_case(kind, B, T, K, H, inp)
    Wx = (x.double() @ W.double().t() + 0.5).float()
    pn = {k: v.numpy() for k, v in p.items()}
    S, U, Wst = bp.cell_forward(kind, Wx.numpy(), pn, u0.numpy(), None if w0 is None else w0.numpy(), s0.numpy())
    rate = float(S.mean())
    assert rate > 0.003

    def before(traj, first):
        return np.concatenate([first.numpy()[:, None], traj[:, :-1]], axis=1).reshape(B * T, H).astype(f32)

    u, s = before(U, u0), before(S, s0)
    Vm = pn["V"].astype(f32).copy()
    np.fill_diagonal(Vm, 0)
    wx = sparse_dot(x.numpy().reshape(B * T, K), W.numpy().T.copy()) + f32(0.5)
    drive = wx + sparse_dot(s, Vm)
    al = bp._clamp(pn["alpha"], bp.ALPHA_LIM)
    if Wst is not None:
        be, pa, pb = bp._clamp(pn["beta"], bp.BETA_LIM), bp._clamp(pn["a"], bp.A_LIM), bp._clamp(pn["b"], bp.B_LIM)
        drive = drive - ((be * before(Wst, w0) + pa * u) + pb * s)
    u1 = al * (u - s) + (f32(1) - al) * drive
    assert u1.dtype == f32
    got = ((u1 - f32(1.0)) > 0).astype(f32).reshape(B, T, H)
    diff = got != S
    n = int(diff.sum())
    worst = float(np.abs(U[diff] - 1.0).max()) if n else 0.0
    print(f"{kind} {inp}: {n} flips in {S.size} spikes (cap {1e-4 * S.size + 2:.1f}), worst |u - 1| {worst:.3g}, "
          f"oracle rate {rate:.4f}")
    assert worst <= 1e-4
    assert n <= 1e-4 * S.size + 2
