"""
Packed ragged batches on the GPU (SNN.forward(x, lengths, pack=True), the `_pk` entry points; DESIGN.md section 6, "Packed
ragged batches").  Every test here fails without the feature: the entry points and `pack=` do not exist.

  sparch_pack_rows / sparch_unpack_rows   exact against tests/packed_numpy.py for 1-, 2- and 4-byte elements, the unpack
            target poisoned with NaN first.
  scan kernels alone (lengths already sorted: the order is the identity)
            forward   against the `_len` entry on the same inputs, BIT FOR BIT on every valid step: u_save, w_save and —
                      without dropout — spikes, plane and spike_count (one row's arithmetic does not know the layout;
                      tests/test_ragged_gpu.py holds `_len` against fp64).  With dropout the spikes are
                      [u_save - theta > 0] times the mask of tests/dropout_numpy.py on the PACKED element index.
            backward  on the kernel's own saves, unpacked to padded arrays with zero tails: the fp64 restatement with the
                      validity mask as its keep multiplier (tests/packed_cases.py), bound = 4 x the worst fp32-run error,
                      pooled over further seeds at the small shapes and capped at 1e-5 of max-abs, as
                      tests/test_ragged_gpu.py does it.
  readout kernels alone   per row against the restatement on the row's own steps, with a NaN guard row behind the N rows.
  whole networks    against tests/ragged_oracle.py in the data regime and with the bars of the masked mode's tests (dyadic
            weights, states on a 2^-4 grid: spike counts equal, outputs to 1e-4, loss to 1e-5, gradients to 5e-4 of max-abs
            or 2e-2 in the bf16 operand mode, running statistics rtol 1e-4 / atol 1e-6), on UNSORTED lengths; and the
            invariant itself, bit for bit.

  recurrent kernels alone   the same two comparisons (the `_len` kernels bit for bit on every valid step — every packed row
            of s_out, the plane, u_save and w_save, so a store across a row's end shows in the neighbour; the backward under
            the bound rule, dV and the column-summed parameter gradients included): two row tiles with the tile bound and
            the per-row predicate both at work, the 8-wave kernel shapes, bf16 saves, a smooth surrogate; in the bf16
            operand mode against the `_len` backward (the fp64 restatement does not round V): dWx bit for bit, dV and
            the column sums to 1e-4 of max-abs.  At the C ABI, on guarded buffers of the test's own: a sentinel in the N
            rows, NaN guard rows behind them — the guard stays intact and every packed row is overwritten.
"""
import numpy as np
import pytest
import torch

from oracle import snn_oracle as orc
from tests import packed_cases as pc
from tests import packed_numpy as pn
from tests import ragged_oracle as rag
from tests import spiking_numpy as sn
from tests import surrogate_numpy as sg
from tests.dropout_numpy import keep_mask
from tests.kit import DEV, F32, F64, SEED, D, N, bf16_mode, raw, record, relmax, same_bits, within  # noqa: F401  (bf16_mode: a fixture)
from tests.kit import Fn as _Fn
from tests.kit import sp  # noqa: F401  (a fixture)
from tests.spiking_cases import collect

pytestmark = pytest.mark.gpu
P_DROP = sn.P_DROP
SMOOTH = ("fast_sigmoid", sg.TEST_SCALE["fast_sigmoid"])


def plan_of(lens, T):
    from sparch_amd import snns
    return snns.prepare_packing(torch.as_tensor(np.asarray(lens)), len(lens), T, DEV)


def dev_lengths(lens):
    return torch.from_numpy(np.asarray(lens).astype(np.int32)).to(DEV), int(np.sum(lens))


# ------------------------------------------------------------------------------------------------ pack / unpack
@pytest.mark.parametrize("C", [35, 40, 64])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.bfloat16, torch.float32], ids=["u8", "bf16", "f32"])
def test_pack_and_unpack_rows(dtype, C):
    Fn = _Fn()
    lengths, B, T = [23, 1, 9, 17, 2, 22], 6, 23
    plan = plan_of(lengths, T)
    rng = np.random.default_rng(C)
    if dtype == torch.uint8:
        x = torch.from_numpy(rng.integers(1, 256, (B, T, C)).astype(np.uint8))
    else:
        x = torch.from_numpy(rng.uniform(0.5, 2.0, (B, T, C)).astype(F32)).to(dtype)     # (no zero: a zero is a tail)
    xp = Fn.pack_rows(x.to(DEV), plan)
    assert xp.shape == (sum(lengths), C) and xp.dtype == dtype
    want = pn.pack(raw(x), lengths)
    assert np.array_equal(raw(xp), want)
    # unpack over a poisoned target: every element is written, the tails with zeros
    poison = torch.full((B, T, C), float("nan") if dtype != torch.uint8 else 255, dtype=dtype, device=DEV)
    from sparch_amd._capi import check, lib, ptr
    check(lib.sparch_unpack_rows(B, T, C, x.element_size(), ptr(xp), ptr(poison), ptr(plan.order), ptr(plan.lengths),
                                 ptr(plan.offsets), plan.n, Fn._stream()), "sparch_unpack_rows")
    back = raw(poison)
    assert np.array_equal(back, pn.unpack(want, lengths, T))
    m = pn.valid_mask(lengths, T)
    assert np.array_equal(back[m], raw(x)[m]) and not back[~m].any()
    assert np.array_equal(raw(Fn.unpack_rows(xp, plan)), back)
    # a view whose base is 4-byte aligned only (the narrower pieces): the same rows
    if dtype == torch.float32 and C % 4 == 0:
        buf = torch.zeros(B * T * C + 1, dtype=dtype, device=DEV)
        buf[1:] = x.to(DEV).reshape(-1)
        assert np.array_equal(raw(Fn.pack_rows(buf[1:].view(B, T, C), plan)), want)


def test_pack_rows_gradients_are_each_other(sp):
    Fn = _Fn()
    lengths, B, T, C = [5, 1, 3], 3, 5, 8
    plan = plan_of(lengths, T)
    x = torch.rand(B, T, C, device=DEV).requires_grad_(True)
    xp = Fn.PackRowsFn.apply(x, plan)
    g = torch.rand_like(xp)
    xp.backward(g)
    assert np.array_equal(N(x.grad), pn.unpack(N(g), lengths, T))
    y = xp.detach().requires_grad_(True)
    up = Fn.UnpackRowsFn.apply(y, plan)
    gu = torch.full_like(up, float("nan"))
    gu[torch.from_numpy(pn.valid_mask(lengths, T)).to(DEV)] = 1.5
    up.backward(gu)
    assert np.array_equal(N(y.grad), np.full((plan.n, C), 1.5, F32))          # (the NaN on the padding is dropped)


# ------------------------------------------------------------------------------------------------ scan kernels
def check_cell_packed(c, lens, p_drop, with_bn, save16=False, capped=True, surrogate=None, against_len=False):
    """Forward and backward of one packed cell case (module docstring).  Returns the worst fraction of the bound.
    against_len: the backward is held to the `_len` backward's dWx, bit for bit, instead of the restatement."""
    Fn = _Fn()
    kind, B, T, H, theta = c["kind"], c["B"], c["T"], c["H"], c["theta"]
    assert c["dirs"] == 1 and (np.diff(lens) <= 0).all()
    plan = plan_of(lens, T)
    n = plan.n
    assert plan.host[0].tolist() == list(range(B)) and n == int(lens.sum()) and n < B * T
    pk = lambda a: D(pn.pack(a, lens))[None]  # noqa: E731  (the packed (1, n, .) tensor of a padded host array)
    d = {k: D(c[k]) for k in ("Wx", "scale", "shift", "u0", "w0", "s0", "g_rate")}
    d["p"] = {k: D(v) for k, v in c["p"].items()}
    common = dict(dirs=1, theta=theta, p_drop=p_drop, seed=SEED, surrogate=surrogate)
    prev = Fn.SAVE_BF16
    Fn.SAVE_BF16 = save16
    try:
        s_pk, count_pk, saved_pk, s16_pk = Fn.cell_forward(kind, pk(c["Wx"]), d["scale"], d["shift"], d["p"], d["u0"], d["w0"],
                                                           d["s0"], B=1, pack=plan, **common)
        s_len, count_len, saved_len, s16_len = Fn.cell_forward(kind, d["Wx"], d["scale"], d["shift"], d["p"], d["u0"], d["w0"],
                                                               d["s0"], B=B, lengths=dev_lengths(lens), **common)
    finally:
        Fn.SAVE_BF16 = prev
    Fn.check_status()
    assert saved_pk[0].dtype == (torch.bfloat16 if save16 else torch.float32)
    assert tuple(saved_pk[0].shape) == (1, n, H) and tuple(s_pk.shape) == (1, n, H)     # exactly N rows
    # the states of every valid step: the `_len` kernel's, bit for bit
    for a, b in zip(saved_pk[:2], saved_len[:2]):
        assert (a is None) == (b is None)
        if a is not None:
            assert same_bits(raw(a)[0], pn.pack(raw(b), lens))
    plane = N(s16_pk, torch.float32)[0]
    if p_drop == 0.0:
        assert same_bits(N(s_pk)[0], pn.pack(N(s_len), lens))
        assert same_bits(raw(s16_pk)[0], pn.pack(raw(s16_len), lens))
        assert np.array_equal(N(count_pk), N(count_len))
        assert 0.02 <= plane.mean() <= 0.7
    else:           # the mask is indexed by the position in the packed tensor
        assert not save16
        S = ((N(saved_pk[0])[0] - F32(theta)) > 0).astype(F32)
        assert 0.02 <= S.mean() <= 0.7
        want = S * keep_mask(SEED, (n, H), p_drop)
        assert np.array_equal(N(s_pk)[0], want), float((N(s_pk)[0] != want).mean())
        assert np.array_equal(plane, (want != 0).astype(F32))
        assert (want != S).any() and (want != 0).any()
    assert np.array_equal(N(count_pk).astype(np.int64), (plane != 0).sum(0))

    # ---- backward on the kernel's own saves
    bn = c["bn"] if with_bn else None
    dWx, grads = Fn.cell_backward(kind, pk(c["g_out"]), d["g_rate"], d["p"], d["u0"], d["w0"], d["s0"], saved_pk, B=1, dirs=1,
                                  T=n, H=H, theta=theta, p_drop=p_drop, seed=SEED,
                                  bn=None if bn is None else (pk(bn[0]), D(bn[1]), D(bn[2])), pack=plan, surrogate=surrogate)
    Fn.check_status()
    torch.cuda.synchronize()
    got = collect(dWx, grads, with_bn)
    assert got["dWx"].shape == (1, n, H)
    if against_len:
        g_len = np.where(pn.valid_mask(lens, T)[:, :, None], c["g_out"], np.nan).astype(F32)
        dWx_len, grads_len = Fn.cell_backward(kind, D(g_len), d["g_rate"], d["p"], d["u0"], d["w0"], d["s0"], saved_len, B=B, dirs=1,
                                      T=T, H=H, theta=theta, p_drop=p_drop, seed=SEED,
                                      bn=None if bn is None else tuple(D(v) for v in bn), lengths=dev_lengths(lens),
                                      surrogate=surrogate)
        Fn.check_status()
        assert same_bits(got["dWx"][0], pn.pack(N(dWx_len), lens)) and np.abs(got["dWx"]).max() > 0
        # dV, the column-summed parameter gradients and the BatchNorm sums: the same terms as the `_len` backward's, added
        # in another order (dV: a product over N packed rows instead of B T padded ones).  An fp32 sum of K <= B T = 760
        # terms moves by at most K 2^-24 = 4.5e-5 of the sum of their magnitudes when reordered; the bar is 1e-4 of the
        # `_len` tensor's max-abs.
        ref_len = collect(dWx_len, grads_len, with_bn)
        worst = 0.0
        for q in sn.bwd_tensors(kind, with_bn):
            if q != "dWx":
                e = relmax(got[q], ref_len[q])
                print(f"  {q}: {e:.3e} of max-abs against the `_len` backward")
                assert np.abs(ref_len[q]).max() > 0 and e <= 1e-4, (q, e)
                worst = max(worst, e / 1e-4)
        return worst
    got["dWx"] = pn.unpack_sorted(got["dWx"][0], lens, T)
    for k, v in got.items():
        assert not np.isnan(v).any(), k
    assert np.abs(got["dWx"]).max() > 0
    us = pn.unpack_sorted(N(saved_pk[0], torch.float32)[0], lens, T)
    ws = None if saved_pk[1] is None else pn.unpack_sorted(N(saved_pk[1], torch.float32)[0], lens, T)
    keep = pc.packed_keep(lens, T, H, p_drop) if p_drop else None
    ref, runs32 = pc.ragged_backward_runs(c, lens, us, ws, keep, with_bn, surrogate)
    names = sn.bwd_tensors(kind, with_bn)
    assert set(names) == set(got), (names, sorted(got))
    bound = sn.bound_of(runs32, ref, names)
    if capped and B * H < 4096:     # the small scan shapes: the fp32 error's sample pooled over further seeds
        rel = pc.pooled_relative_error(kind, B, T, H, tuple(int(v) for v in lens), p_drop, with_bn, surrogate)
        bound = {k: max(bound[k], 4.0 * rel[k] * float(np.abs(ref[k]).max())) for k in names}
    if capped:
        bound = sn.capped(bound, ref, names)
    return max([0.0] + [within(got[k], ref[k], bound[k], k) for k in names])


# ring depths of the scan kernels at one neuron per thread: 15 / 12 forward (LIF / adLIF, every output), 16 / 15 / 12
# backward — T below, at and just above them, and one that is no multiple of any
SCAN_T = (11, 12, 13, 15, 16, 17, 29)


@pytest.mark.parametrize("T", SCAN_T)
@pytest.mark.parametrize("H", [12, 64])
@pytest.mark.parametrize("kind", sn.SCAN_KINDS)
def test_scan_kernels_packed(kind, H, T, record_property):
    c = sn.scan_case(kind, 5, 1, T, H)
    lens = pc.sorted_lengths(5, T, 7 * T + H)
    assert {1, 2, T - 1, T} <= set(lens.tolist())
    worst = [check_cell_packed(c, lens, 0.0, True), check_cell_packed(c, lens, P_DROP, False)]
    if T == 17:
        worst += [check_cell_packed(c, lens, P_DROP, True), check_cell_packed(c, lens, 0.0, False)]
        if H % 4 == 0:
            worst.append(check_cell_packed(c, lens, 0.0, True, save16=True))
    record(record_property, *worst)


def test_scan_kernels_packed_four_neurons_per_thread(record_property):
    """The VEC = 4 instantiations (B H >= 524288, H % 4 == 0): ring depth 8, T = 9 and 17."""
    B, H = 33, 15888
    for kind in sn.SCAN_KINDS:
        for T in (9, 17):
            c = sn.scan_case(kind, B, 1, T, H)
            record(record_property, check_cell_packed(c, pc.sorted_lengths(B, T, T), 0.0 if T == 9 else P_DROP, True))


@pytest.mark.parametrize("H", [12, 64])
@pytest.mark.parametrize("kind", sn.SCAN_KINDS)
def test_scan_kernels_packed_with_a_smooth_surrogate(kind, H, record_property):
    """The smooth instantiations of the packed backward, with and without the folded BatchNorm sums and dropout."""
    T = 17
    c = sn.scan_case(kind, 5, 1, T, H)
    lens = pc.sorted_lengths(5, T, 7 * T + H)
    record(record_property, check_cell_packed(c, lens, 0.0, True, surrogate=SMOOTH),
           check_cell_packed(c, lens, P_DROP, False, surrogate=SMOOTH))


def test_scan_kernels_packed_four_neurons_per_thread_other_variants(record_property):
    """Four neurons per thread: bf16 saves (box-car) and a smooth surrogate (fp32 saves)."""
    B, H, T = 33, 15888, 9
    c = sn.scan_case("adLIF", B, 1, T, H)
    lens = pc.sorted_lengths(B, T, T)
    record(record_property, check_cell_packed(c, lens, 0.0, True, save16=True),
           check_cell_packed(c, lens, P_DROP, True, surrogate=SMOOTH))


# ------------------------------------------------------------------------------------------------ recurrent kernels
def rec_packed_case(kind, B, T, H, lens):
    c = sn.make_inputs(kind, B, 1, T, H, sn.case_seed(kind, B, 1, T, H), "drive")
    c["g_rate"] = (c["g_rate"] * F32(B * T)).astype(F32)    # (as drawn the rate term is 0.3 % of g_out)
    rng = np.random.default_rng(17)                         # the folded BatchNorm sums' operands, as spiking_numpy.scan_case's
    c["bn"] = ((c["Wx"] * F32(0.8) + F32(0.3)).astype(F32), rng.uniform(0.2, 0.6, H).astype(F32),
               rng.uniform(0.5, 1.5, H).astype(F32))
    return c, np.asarray(lens, np.int64)


def two_tile_lengths(T):
    """40 sorted lengths: tile 0 (32 rows) with more than four distinct lengths, its longest = T; tile 1 (8 rows) with its
    longest < T and one row of length 1 — the tile bound and the per-row predicate are both exercised."""
    rng = np.random.default_rng(5)
    tile0 = sorted([T, T - 1, T - 3, 12, 9, 8] + [int(v) for v in rng.integers(8, T + 1, 26)], reverse=True)
    lens = tile0 + [7, 6, 6, 5, 3, 2, 2, 1]
    assert len(lens) == 40 and len(set(tile0)) > 4 and tile0[0] == T and lens[32] < T and lens[-1] == 1
    return lens


def wide_lengths(T):
    return sorted([T, T, T - 1, 2, 1] + [int(v) for v in np.random.default_rng(3).integers(1, T + 1, 27)], reverse=True) + [1]


@pytest.mark.parametrize("mode", ["whole", "save_bf16", "smooth"])
@pytest.mark.parametrize("kind", ["RLIF", "RadLIF"])
def test_recurrent_kernels_packed(kind, mode, record_property):
    T = 19
    c, lens = rec_packed_case(kind, 40, T, 64, two_tile_lengths(T))
    kw = dict(save16=mode == "save_bf16", surrogate=SMOOTH if mode == "smooth" else None, capped=False)
    worst = [check_cell_packed(c, lens, 0.0, True, **kw)]
    if mode == "whole":
        worst.append(check_cell_packed(c, lens, 0.0, False, **kw))
    record(record_property, *worst)


@pytest.mark.parametrize("H", [132, 384, 1024])
def test_recurrent_kernels_packed_wider_kernel_shapes(H, record_property):
    """The packed instantiations of the 8-wave kernel shapes (k-group classes 2, 4 and 8): two tiles, the second of one
    row of length 1."""
    c, lens = rec_packed_case("RadLIF", 33, 6, H, wide_lengths(6))
    record(record_property, check_cell_packed(c, lens, 0.0, True, capped=False))


def test_recurrent_kernels_packed_bf16_operand_mode(bf16_mode):
    T = 19
    c, lens = rec_packed_case("RadLIF", 40, T, 64, two_tile_lengths(T))
    check_cell_packed(c, lens, 0.0, True, capped=False, against_len=True)


@pytest.mark.parametrize("kind", ["RLIF", "RadLIF"])
def test_recurrent_kernels_packed_write_their_own_rows_only(kind):
    """The `_pk` recurrent entries at the C ABI on buffers of this test's own: N rows filled with a sentinel and T guard
    rows of NaN behind them (more than the tile bound - 1: the length-1 row of tile 1, whose tile runs 7 steps, would put
    unpredicated stores on rows N .. N + 5).  Afterwards the guard is intact and every packed row is overwritten, in
    s_out, the plane, u_save, w_save, dWx and s_prev16; and the rows are what the host path computes, bit for bit."""
    from sparch_amd._capi import KIND, check, lib, ptr
    Fn = _Fn()
    B, T, H, SENT = 40, 19, 64, 7.0
    c, lens = rec_packed_case(kind, B, T, H, two_tile_lengths(T))
    plan = plan_of(lens, T)
    n, G, k = plan.n, T, KIND[kind]
    d = {q: D(c[q]) for q in ("u0", "w0", "s0", "g_rate")}
    pr = {q: D(v) for q, v in c["p"].items()}
    wx, g = D(pn.pack(c["Wx"], lens)), D(pn.pack(c["g_out"], lens))
    bn = (D(pn.pack(c["bn"][0], lens)), D(c["bn"][1]), D(c["bn"][2]))

    def guarded(fill, dtype=torch.float32):
        t = torch.full((n + G, H), float("nan"), dtype=dtype, device=DEV)
        t[:n] = fill
        return t

    def rows_of(t, what):
        a = N(t, torch.float32)
        assert np.isnan(a[n:]).all(), f"{what}: a store behind the packed rows"
        assert not np.isnan(a[:n]).any() and not (a[:n] == SENT).any(), f"{what}: a packed row was not written"
        return a[:n]

    vpack = torch.empty(lib.sparch_vpack_bytes(H) // 4, dtype=torch.float32, device=DEV)
    vpack_t, vmask = torch.empty_like(vpack), torch.empty(H, H, dtype=torch.float32, device=DEV)
    check(lib.sparch_vpack_both(H, ptr(pr["V"]), ptr(vpack), ptr(vpack_t), ptr(vmask), Fn._stream(), Fn._prec()), "sparch_vpack_both")
    rec0 = Fn._gemm_small(d["s0"], vmask, nn=True)
    nbytes = lib.sparch_rec_chan_bytes(B, T, H)
    chan = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=DEV)
    status = Fn.status_word(DEV)
    s_out, s16, u_save = guarded(SENT), guarded(SENT, torch.bfloat16), guarded(SENT)
    w_save = guarded(SENT) if kind == "RadLIF" else None
    count = torch.zeros(H, dtype=torch.int32, device=DEV)
    nrn = (ptr(pr["alpha"]), ptr(pr.get("beta")), ptr(pr.get("a")), ptr(pr.get("b")))
    check(lib.sparch_rec_cell_fwd_pk(k, B, 1, T, H, ptr(wx), None, None, *nrn, ptr(vpack), ptr(rec0), ptr(d["u0"]), ptr(d["w0"]),
                                     ptr(d["s0"]), c["theta"], 0.0, 0, ptr(s_out), ptr(s16), ptr(u_save), ptr(w_save), 0,
                                     ptr(count), *plan.args(), ptr(chan), nbytes, ptr(status), T, Fn._stream(), Fn._prec()),
          "sparch_rec_cell_fwd_pk")
    Fn.check_status()
    spikes = rows_of(s_out, "s_out")
    assert set(np.unique(spikes).tolist()) <= {0.0, 1.0} and 0.02 <= spikes.mean() <= 0.7
    assert np.array_equal(rows_of(s16, "s16_out"), spikes)
    rows_of(u_save, "u_save")
    if w_save is not None:
        rows_of(w_save, "w_save")
    s_ref, count_ref, saved_ref, _ = Fn.cell_forward(kind, wx[None], None, None, pr, d["u0"], d["w0"], d["s0"], B=1, dirs=1,
                                                     theta=c["theta"], p_drop=0.0, seed=0, pack=plan)
    assert same_bits(spikes, N(s_ref)[0]) and same_bits(N(u_save)[:n], N(saved_ref[0])[0])
    assert np.array_equal(N(count), N(count_ref))

    dWx, s_prev = guarded(SENT), guarded(SENT, torch.bfloat16)
    ws = torch.empty(8, B, H, dtype=torch.float32, device=DEV)
    check(lib.sparch_rec_cell_bwd_pk(k, B, 1, T, H, ptr(g), ptr(d["g_rate"]), ptr(u_save), ptr(w_save), 0, *nrn, ptr(vpack_t),
                                     ptr(d["u0"]), ptr(d["w0"]), ptr(d["s0"]), c["theta"], 0.0, 0, ptr(dWx), ptr(s_prev), ptr(ws),
                                     ptr(bn[0]), ptr(bn[1]), ptr(bn[2]), *plan.args(), ptr(chan), nbytes, ptr(status), T, 0, 0.0,
                                     Fn._stream(), Fn._prec()), "sparch_rec_cell_bwd_pk")
    Fn.check_status()
    got = rows_of(dWx, "dWx")
    prev = rows_of(s_prev, "s_prev16")
    assert set(np.unique(prev).tolist()) <= {0.0, 1.0} and np.abs(got).max() > 0
    # s_prev16 holds the spikes of the step before (a zero row at every sequence's step 0)
    off = plan.host[2]
    for j in range(B):
        assert not prev[off[j]].any() and np.array_equal(prev[off[j] + 1:off[j + 1]], spikes[off[j]:off[j + 1] - 1]), j
    dWx_ref, _ = Fn.cell_backward(kind, g[None], d["g_rate"], pr, d["u0"], d["w0"], d["s0"], saved_ref, B=1, dirs=1, T=n, H=H,
                                  theta=c["theta"], p_drop=0.0, seed=0, bn=bn, pack=plan)
    Fn.check_status()
    assert same_bits(got, N(dWx_ref)[0])


def test_recurrent_packed_launches_are_whole_sequences():
    """steps_per_launch < T is refused (SPARCH_EINVAL) before anything is launched."""
    Fn = _Fn()
    T = 19
    c, lens = rec_packed_case("RLIF", 40, T, 64, two_tile_lengths(T))
    plan = plan_of(lens, T)
    d = {k: D(c[k]) for k in ("u0", "s0")}
    with pytest.raises(ValueError, match="sparch_rec_cell_fwd_pk"):
        Fn.cell_forward("RLIF", D(pn.pack(c["Wx"], lens))[None], None, None, {k: D(v) for k, v in c["p"].items()}, d["u0"], None,
                        d["s0"], B=1, dirs=1, theta=c["theta"], p_drop=0.0, seed=0, steps_per_launch=7, pack=plan)


# ------------------------------------------------------------------------------------------------ readout kernels
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine_bn"])
def test_readout_kernels_packed(affine, record_property):
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    B, T, C = 5, 300, 35
    lens = np.asarray([300, 257, 256, 255, 1], np.int64)
    plan = plan_of(lens, T)
    n = plan.n
    assert plan.host[0].tolist() == list(range(B)) and n == 1069
    c = sn.readout_case(B, T, C)
    d = {k: D(c[k]) for k in ("u0", "alpha", "g_out", "scale", "shift")}
    x_host = c["bn"][0] if affine else c["Wx"]
    x = D(pn.pack(x_host, lens))
    scale, shift = (d["scale"], d["shift"]) if affine else (None, None)
    bn_dev = (x, D(c["bn"][1]), D(c["bn"][2]))
    nan_rows = lambda rows: torch.full((rows, C), float("nan"), dtype=torch.float32, device=DEV)  # noqa: E731
    out, u_save, dWx = nan_rows(B), nan_rows(n + 1), nan_rows(n + 1)          # (row n: a guard behind the packed rows)
    check(lib.sparch_readout_fwd_pk(B, T, C, ptr(x), ptr(scale), ptr(shift), ptr(d["alpha"]), ptr(d["u0"]), ptr(out),
                                    ptr(u_save), *plan.args(), Fn._stream()), "sparch_readout_fwd_pk")
    ws = torch.empty(3 if affine else 1, B, C, dtype=torch.float32, device=DEV)
    bnp = [ptr(v) for v in bn_dev] if affine else [None, None, None]
    check(lib.sparch_readout_bwd_pk(B, T, C, ptr(d["g_out"]), *bnp, ptr(u_save), ptr(d["alpha"]), ptr(d["u0"]), ptr(dWx),
                                    ptr(ws), *plan.args(), Fn._stream()), "sparch_readout_bwd_pk")
    if affine:
        dalpha, s1, s2 = Fn._finish_param_grads(ws, B, C, [d["alpha"], None, None], [Fn.ALPHA_LIM, (0.0, 0.0), (0.0, 0.0)])
        got = {"alpha": N(dalpha), "bn_dy": N(s1), "bn_dyx": N(s2)}
    else:
        got = {"alpha": N(Fn._finish_param_grads(ws, B, C, [d["alpha"]], [Fn.ALPHA_LIM])[0])}
    Fn.check_status()
    for k, t in (("u_save", u_save), ("dWx", dWx)):
        a = N(t)
        assert np.isnan(a[n]).all() and not np.isnan(a[:n]).any(), k            # the guard is intact, every row written
        got[k] = pn.unpack_sorted(a[:n], lens, T)
    got["out"] = N(out)
    assert not np.isnan(got["out"]).any() and not np.isnan(got["alpha"]).any()
    bn = c["bn"] if affine else None

    def run(dt, order):
        """Row by row on the row's own steps: the clip run alone."""
        res = {"out": np.zeros((B, C), dt), "dWx": np.zeros((B, T, C), dt), "u_save": np.zeros((B, T, C), dt)}
        sums = {}
        rows = range(B) if order != "desc" else range(B - 1, -1, -1)
        for b in rows:
            m = int(lens[b])
            u, o = sn.readout_forward(dt, x_host[b:b + 1, :m], None if scale is None else c["scale"],
                                      None if shift is None else c["shift"], c["alpha"], c["u0"][b:b + 1], order)
            res["u_save"][b, :m], res["out"][b] = u[0], o[0]
            bn_b = None if bn is None else (bn[0][b:b + 1, :m], bn[1], bn[2])
            r = sn.readout_backward(dt, c["g_out"][b:b + 1], got["u_save"][b:b + 1, :m], c["alpha"], c["u0"][b:b + 1],
                                    bn=bn_b, class_order=order)
            res["dWx"][b, :m] = r["dWx"][0]
            for k in ("alpha",) + (("bn_dy", "bn_dyx") if affine else ()):
                sums[k] = r[k].astype(dt) if k not in sums else (sums[k] + r[k]).astype(dt)
        res.update(sums)
        return res

    ref = run(F64, None)
    assert abs(ref["out"].sum() - lens.sum()) <= 1e-9 * lens.sum()          # a truncated sum, not a mean
    names = ("out", "dWx") + sn.READOUT_BWD_TENSORS[affine][1:]
    runs32 = [run(F32, "asc"), run(F32, "desc")]
    bound = sn.capped(sn.bound_of(runs32, ref, names), ref, names)
    worst = [within(got[k], ref[k], bound[k], k) for k in names]
    ub = sn.bound_of(runs32, ref, ("u_save",))["u_save"]
    worst.append(within(got["u_save"], ref["u_save"], ub, "u_save"))
    assert got["alpha"][0] == 0 and got["alpha"][1] == 0 and np.abs(got["alpha"][2:]).max() > 0
    record(record_property, *worst)


# ------------------------------------------------------------------------------------------------ whole networks
NB, NT, SIZES, LENGTHS = pc.NB, pc.NT, pc.SIZES, pc.NET_LENGTHS
KINDS = ["LIF", "adLIF", "RLIF", "RadLIF"]


def compare_with_oracle(net, params, kind, normalization, training, x, y, init, out, rates, loss, tol_g, drop_masks=None,
                        zero_grads=()):
    """zero_grads: parameters whose gradient is zero analytically, so that both sides hold only the rounding noise of a sum
    that cancels and the max-abs of the reference is no scale: `name -> the parameter whose gradient has the scale of the
    summands`; each side is held to tol_g of THAT gradient's max-abs."""
    po = {k: v.clone().requires_grad_(v.dtype == torch.float32 and "running" not in k) for k, v in params.items()}
    stats = {}
    x_o = x * rag.valid_mask(LENGTHS, NT)[:, :, None]
    out_o, rates_o = rag.snn_forward(x_o, LENGTHS, po, neuron_type=kind, num_layers=3, init_states=init,
                                     normalization=normalization, training=training, stats=stats, drop_masks=drop_masks)
    loss_o = orc.train_step_loss(out_o, rates_o, y, use_regularizers=True)
    loss_o.backward()
    n_valid = sum(LENGTHS)
    scale = 1.0 if drop_masks is None else 1.0 - P_DROP                       # (kept spikes count 1 / (1 - p) each)
    counts = torch.round(rates.detach().cpu() * n_valid * scale).long()
    counts_o = torch.round(rates_o.detach() * n_valid * scale).long()
    assert int(counts_o[:SIZES[0]].sum()) > 0 and int(counts_o[SIZES[0]:].sum()) > 0
    assert torch.equal(counts, counts_o), "per-neuron spike counts differ from the oracle"
    eo = relmax(N(out), out_o.detach().numpy())
    print(f"  out {eo:.3e}  loss {float(loss.detach()):.6f} / {float(loss_o.detach()):.6f}")
    assert eo <= 1e-4
    assert abs(float(loss) - float(loss_o)) <= 1e-5 * max(1.0, abs(float(loss_o)))
    assert relmax(N(rates), rates_o.detach().numpy()) <= 1e-6
    for k, v in net.named_parameters():
        if k in zero_grads:
            top = float(po[zero_grads[k]].grad.abs().max())
            noise = max(float(v.grad.abs().max()), float(po[k].grad.abs().max()))
            print(f"  {k}: {noise:.3e} on either side, {noise / top:.3e} of max|grad {zero_grads[k]}|")
            assert top > 0 and noise <= tol_g * top, (k, noise, top)
            continue
        e = relmax(N(v.grad), po[k].grad.numpy())
        print(f"  {k}: {e:.3e}")
        assert e <= tol_g, (k, e)
    for k, v in stats.items():
        np.testing.assert_allclose(N(net.state_dict()[k]), v.numpy(), rtol=1e-4, atol=1e-6, err_msg=k)


def run_packed(net, x, y, init):
    with pc.injected_states(init):
        out, rates = net(x.to(DEV), lengths=torch.tensor(LENGTHS), pack=True)
        loss = orc.train_step_loss(out, rates, y.to(DEV), use_regularizers=True)
        loss.backward()
        _Fn().check_status()
    return out, rates, loss


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("normalization", ["batchnorm", "layernorm", "none"])
@pytest.mark.parametrize("kind", KINDS)
def test_whole_network_packed_vs_ragged_oracle(sp, kind, normalization, training, compute, request):
    if compute == "bf16":
        request.getfixturevalue("bf16_mode")
    net = pc.make_net(sp, kind, normalization)
    params = {k: v.clone() for k, v in net.state_dict().items()}
    x, y, init = pc.net_inputs(orc, kind, zero_padding=False)       # (the padding holds spikes: the packed path never reads it)
    net = net.to(DEV).train(training)
    out, rates, loss = run_packed(net, x, y, init)
    compare_with_oracle(net, params, kind, normalization, training, x, y, init, out, rates, loss,
                        5e-4 if compute == "fp32" else 2e-2)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_whole_network_packed_batchnorm_with_bias(sp, training):
    """BatchNorm with use_bias=True: refused by the masked mode, accepted here (there is no padded row for the bias).
    In train mode BatchNorm subtracts the column mean, bias included: the bias's gradient is the column sum of a tensor
    whose columns sum to zero, i.e. rounding noise on both sides — held to 5e-4 of the max-abs of the same layer's
    weight gradient (sums of the same terms that do not cancel).  In eval mode (running statistics) the bias counts and
    its gradient goes through the bar of every other parameter."""
    net = pc.make_net(sp, "adLIF", "batchnorm", use_bias=True)
    params = {k: v.clone() for k, v in net.state_dict().items()}
    x, y, init = pc.net_inputs(orc, "adLIF")
    net = net.to(DEV).train(training)
    with pytest.raises(ValueError, match="use_bias"):
        net(x.to(DEV), lengths=torch.tensor(LENGTHS))
    out, rates, loss = run_packed(net, x, y, init)
    zero = {f"snn.{i}.W.bias": f"snn.{i}.W.weight" for i in range(3)} if training else {}
    compare_with_oracle(net, params, "adLIF", "batchnorm", training, x, y, init, out, rates, loss, 5e-4, zero_grads=zero)


@pytest.mark.parametrize("normalization", ["batchnorm", "layernorm", "none"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_packed_row_is_its_clip_run_alone_and_the_masked_row_bit_for_bit(sp, kind, normalization):
    """Eval mode, dyadic data: row b of net(x, lengths, pack=True) equals net(x[b:b+1, :L_b]) with the same state rows, and
    row b of the masked net(x, lengths); so do the firing rates of the two modes."""
    net = pc.make_net(sp, kind, normalization).to(DEV).eval()
    x, _, init = pc.net_inputs(orc, kind)
    with torch.no_grad():
        with pc.injected_states(init):
            out, rates = net(x.to(DEV), lengths=torch.tensor(LENGTHS), pack=True)
        with pc.injected_states(init):
            out_m, rates_m = net(x.to(DEV), lengths=torch.tensor(LENGTHS))
        assert torch.equal(out, out_m) and torch.equal(rates, rates_m)
        for b, m in enumerate(LENGTHS):
            with pc.injected_states(init, slice(b, b + 1)):
                alone, _ = net(x[b:b + 1, :m].contiguous().to(DEV))
            assert torch.equal(out[b:b + 1], alone), (b, m)
    assert float(rates.sum()) > 0
    _Fn().check_status()


def test_packed_input_gradient_is_zero_on_the_padding(sp):
    net = pc.make_net(sp, "adLIF", "batchnorm").to(DEV).train()
    x, y, init = pc.net_inputs(orc, "adLIF")
    xd = x.to(DEV).requires_grad_(True)
    with pc.injected_states(init):
        out, rates = net(xd, lengths=torch.tensor(LENGTHS, device=DEV), pack=True)    # (lengths on the device work too)
        orc.train_step_loss(out, rates, y.to(DEV), use_regularizers=True).backward()
    g = N(xd.grad)
    m = pn.valid_mask(LENGTHS, NT)[:, :, None]
    assert g.shape == tuple(x.shape) and not (g * ~m).any() and np.abs(g).max() > 0 and not np.isnan(g).any()
    xm = x.to(DEV).requires_grad_(True)
    net.zero_grad()
    with pc.injected_states(init):
        out_m, rates_m = net(xm, lengths=torch.tensor(LENGTHS))
        orc.train_step_loss(out_m, rates_m, y.to(DEV), use_regularizers=True).backward()
    assert relmax(g, N(xm.grad)) <= 5e-4                                           # the masked mode's gradient


@pytest.mark.parametrize("kind", KINDS)
def test_without_a_readout_layer_the_spikes_come_back_padded(sp, kind):
    net = pc.make_net(sp, kind, "batchnorm", use_readout_layer=False).to(DEV).eval()
    x, _, _ = pc.net_inputs(orc, kind)
    torch.manual_seed(13)       # three hidden layers here: u0, [w0,] s0 of each on the 2^-4 grid
    init = [{k: torch.floor(torch.rand(NB, H) * 16) / 16 for k in (("u0", "w0", "s0") if kind in ("adLIF", "RadLIF") else ("u0", "s0"))}
            for H in SIZES]
    with torch.no_grad():
        with pc.injected_states(init):
            s, rates = net(x.to(DEV), lengths=torch.tensor(LENGTHS), pack=True)
        with pc.injected_states(init):
            s_m, rates_m = net(x.to(DEV), lengths=torch.tensor(LENGTHS))
    m = torch.from_numpy(pn.valid_mask(LENGTHS, NT)).to(DEV)[:, :, None]
    assert tuple(s.shape) == (NB, NT, SIZES[-1]) and not (s * ~m).any() and float(s.sum()) > 0
    assert torch.equal(s, s_m) and torch.equal(rates, rates_m)
    _Fn().check_status()


@pytest.mark.parametrize("kind", ["adLIF", "RadLIF"])
def test_packed_dropout_on_vs_ragged_oracle(sp, kind):
    """Dropout on: the oracle is handed the masks of tests/dropout_numpy.py on the packed element index."""
    net = pc.make_net(sp, kind, "batchnorm", dropout=P_DROP)
    params = {k: v.clone() for k, v in net.state_dict().items()}
    x, y, init = pc.net_inputs(orc, kind)
    net = net.to(DEV).train()
    seeds = []
    for i, lay in enumerate(list(net.snn)[:-1]):
        lay._dropout_seed = lambda device, i=i: SEED + i
        seeds.append(SEED + i)
    out, rates, loss = run_packed(net, x, y, init)
    masks = pc.packed_drop_masks(LENGTHS, P_DROP, seeds, SIZES[:-1])
    assert all(0.6 < float((mk != 0)[torch.from_numpy(pn.valid_mask(LENGTHS, NT))].float().mean()) < 0.9 for mk in masks)
    compare_with_oracle(net, params, kind, "batchnorm", True, x, y, init, out, rates, loss, 5e-4, drop_masks=masks)


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_hd_with_packed_lengths(tmp_path, monkeypatch):
    """SPARCH_LENGTHS=pack run_exp.py --dataset_name hd on a tiny folder of unequal clips: two training steps, every batch
    goes to the network packed with its own unequal lengths and the loss is finite."""
    import run_exp
    import sparch_amd
    from sparch_amd import exp
    from tests.audio_trees import make_hd_tree
    root = str(tmp_path / "hd")
    make_hd_tree(root, n_train=8, n_test=4, lengths=(16000, 6400, 11200, 9000))
    monkeypatch.setenv("SPARCH_LENGTHS", "pack")
    seen = []
    forward = sparch_amd.SNN.forward
    loss_call = exp.Fn.CrossEntropyLoss.forward

    def spy(self, x, lengths=None, pack=False):
        seen.append((None if lengths is None else [int(v) for v in lengths], pack))
        return forward(self, x, lengths=lengths, pack=pack)

    losses = []

    def loss_spy(self, output, target):
        v = loss_call(self, output, target)
        losses.append(float(v))
        return v

    monkeypatch.setattr(sparch_amd.SNN, "forward", spy)
    monkeypatch.setattr(exp.Fn.CrossEntropyLoss, "forward", loss_spy)
    torch.manual_seed(5)
    run_exp.main(["--model_type", "adLIF", "--nb_layers", "3", "--nb_hiddens", "64", "--dataset_name", "hd",
                  "--data_folder", root, "--batch_size", "4", "--nb_epochs", "1", "--save_best", "0",
                  "--new_exp_folder", str(tmp_path / "exp")])
    assert len(seen) >= 3 and all(v is not None and pk is True for v, pk in seen)   # two training steps, then validation
    assert all(len(set(v)) > 1 for v, _ in seen[:2]), seen[:2]                      # unequal clips in a batch
    assert len(losses) >= 3 and all(np.isfinite(v) for v in losses), losses
