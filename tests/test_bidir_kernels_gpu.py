"""
The movers of csrc/bidir.hip at the C ABI against NumPy indexing (tests/bidir_numpy.py), EXACT: split and join move bytes,
the two adjoints add one fp32 sum (and, for the rate term, one fp32 product) that NumPy float32 reproduces bit for bit.

Shapes: T = 23 with the lengths [23, 1, 9, 17, 2, 22] of tests/test_ragged_gpu.py (a full clip, a one-step clip), one clip
alone with a length of T, of 1 and in between; row widths 5, 64 and 70 elements — for the three element sizes that is every
piece width the kernels choose (1, 2, 4 and 16 bytes) and a row that is no multiple of 16 bytes.  Padded destinations are
pre-filled with 0xFF bytes (NaN): the tails must come out as zeros; sources carry NaN / junk where nothing may read them.
Packed layouts: the single tensors packed by tests/packed_numpy.py, the doubled ones by the lengths twice.
Every test here is an AttributeError on a library without the entry points.
"""
import numpy as np
import pytest
import torch

from tests import bidir_numpy as bn
from tests import packed_numpy as pn
from tests.kit import DEV, D, N, ptr, same_bits
from tests.kit import Fn as _Fn

pytestmark = pytest.mark.gpu
T = 23
LENGTHS = ([23, 1, 9, 17, 2, 22], [23], [1], [9])
WIDTHS = (5, 64, 70)
DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def call(name, *args):
    from sparch_amd._capi import check, lib
    check(getattr(lib, name)(*args, _Fn()._stream()), name)
    torch.cuda.synchronize()


def layout(lengths, packed):
    """(B, T of the index space, the map arguments, what turns a padded single / doubled reference into the layout)."""
    B, n = len(lengths), int(np.sum(lengths))
    if not packed:
        L = D(np.asarray(lengths, np.int32))
        return B, T, (ptr(L), n), (lambda a: a), (lambda a: a), [L]
    order, lens, offsets, _ = pn.plan_of(lengths)
    _, _, _, _, fwd, rev = bn.doubled_plan(lengths)
    keep = [D(np.asarray(v, np.int32)) for v in (lens, offsets, fwd, rev)]
    return (B, int(lens[0]), tuple(ptr(v) for v in keep) + (n,), (lambda a: pn.pack(a, lengths)),
            (lambda a: bn.pack2(a, lengths)), keep)


def filled(shape, dtype):
    """A device tensor of 0xFF bytes (NaN for every float format)."""
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(255)
    return t


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
@pytest.mark.parametrize("elem_size", [1, 2, 4])
def test_split_moves_bytes(elem_size, packed):
    rng = np.random.default_rng(elem_size)
    sfx = "_pk" if packed else "_len"
    for lengths in LENGTHS:
        for C in WIDTHS:
            B, Tk, tail, one, two, keep = layout(lengths, packed)
            x = rng.integers(1, 1 << (8 * elem_size), (B, T, C), dtype=np.uint64).astype(DTYPES[elem_size])  # (no zeros)
            src = one(x)                                   # (padded: junk behind the lengths, which nothing may read)
            want = two(bn.split(x, lengths))
            dst = torch.full((int(np.prod(want.shape)) * elem_size,), 255, dtype=torch.uint8, device=DEV)
            src_d = torch.from_numpy(np.ascontiguousarray(src).view(np.uint8).copy()).to(DEV)
            call("sparch_bidir_split" + sfx, B, Tk, C, elem_size, ptr(src_d), ptr(dst), *tail)
            got = N(dst).view(DTYPES[elem_size]).reshape(want.shape)
            assert np.array_equal(got, want), (lengths, C)
            if not packed:
                m = pn.valid_mask(lengths, T)
                assert not got[np.concatenate([~m, ~m])].any() and (got[np.concatenate([m, m])] != 0).all()


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_split_backward_adds_the_two_directions(packed):
    rng = np.random.default_rng(7)
    sfx = "_pk" if packed else "_len"
    for lengths in LENGTHS:
        for C in WIDTHS:
            B, Tk, tail, one, two, keep = layout(lengths, packed)
            g = rng.standard_normal((2 * B, T, C)).astype(np.float32)
            m2 = np.concatenate([pn.valid_mask(lengths, T)] * 2)
            g[~m2] = np.nan                                # (nothing may read the doubled tensor's tails)
            want = one(bn.split_bwd(np.where(m2[:, :, None], g, 0).astype(np.float32), lengths))
            out = filled(want.shape, torch.float32)
            g_d = D(two(g))
            call("sparch_bidir_split_bwd" + sfx, B, Tk, C, ptr(g_d), ptr(out), *tail)
            assert same_bits(N(out), want), (lengths, C)


@pytest.mark.parametrize("fp32", [True, False], ids=["fp32_too", "plane_only"])
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_join_moves_the_plane_and_counts_spikes(packed, fp32):
    rng = np.random.default_rng(11)
    sfx = "_pk" if packed else "_len"
    one_bf16 = np.uint16(0x3F80)
    scale = np.float32(1.0) / np.float32(0.75)
    for lengths in LENGTHS:
        for H in WIDTHS:
            B, Tk, tail, one, two, keep = layout(lengths, packed)
            s = (rng.random((2 * B, T, H)) < 0.4).astype(np.uint16) * one_bf16
            m2 = np.concatenate([pn.valid_mask(lengths, T)] * 2)
            s[~m2] = one_bf16                              # (spikes on the doubled tensor's tails: never read, never counted)
            clean = np.where(m2[:, :, None], s, 0).astype(np.uint16)
            want = one(bn.join(clean, lengths))
            y16 = torch.full(want.shape, -1, dtype=torch.int16, device=DEV)
            y32 = filled(want.shape, torch.float32) if fp32 else None
            count = torch.full((2 * H,), 7, dtype=torch.int32, device=DEV)     # (added to: the caller owns and clears it)
            s_d = torch.from_numpy(two(s).view(np.int16)).to(DEV)
            call("sparch_bidir_join" + sfx, B, Tk, H, ptr(s_d), ptr(y16), ptr(y32), float(scale), ptr(count), *tail)
            assert np.array_equal(N(y16).view(np.uint16), want), (lengths, H)
            per_column = np.count_nonzero(want.reshape(-1, 2 * H), axis=0)
            assert np.array_equal(N(count).astype(np.int64), 7 + per_column), (lengths, H)
            assert per_column[:H].sum() > 0 and (len(lengths) == 1 or per_column[H:].sum() > 0)
            if fp32:
                assert same_bits(N(y32), (want != 0).astype(np.float32) * scale), (lengths, H)


@pytest.mark.parametrize("rate", [True, False], ids=["rate_gradient", "no_rate_gradient"])
@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_join_backward_gathers_and_adds_the_rate_gradient(packed, rate):
    rng = np.random.default_rng(13)
    sfx = "_pk" if packed else "_len"
    for lengths in LENGTHS:
        for H in WIDTHS:
            B, Tk, tail, one, two, keep = layout(lengths, packed)
            g = rng.standard_normal((B, T, 2 * H)).astype(np.float32)
            m = pn.valid_mask(lengths, T)
            g[~m] = np.nan                                 # (the gradient on the padding is never read)
            g_rate = rng.standard_normal(2 * H).astype(np.float32) if rate else None
            rate_scale = 1.0 / float(np.sum(lengths))
            want = two(bn.join_bwd(np.where(m[:, :, None], g, 0).astype(np.float32), g_rate, rate_scale, lengths))
            out = filled(want.shape, torch.float32)
            g_d, r_d = D(one(g)), D(g_rate)
            call("sparch_bidir_join_bwd" + sfx, B, Tk, H, ptr(g_d), ptr(r_d), rate_scale, ptr(out), *tail)
            assert same_bits(N(out), want), (lengths, H)


@pytest.mark.parametrize("packed", [False, True], ids=["padded", "packed"])
def test_base_addresses_off_the_wide_pieces(packed):
    """Rows of 64 elements (whole 16-byte pieces) at base addresses ONE ELEMENT behind an aligned one: the movers fall back
    to 4-, 2- and 1-byte pieces (fp32 / bf16 / uint8 rows; the fp32 adjoints to one float per thread), and give the same
    bytes."""
    rng = np.random.default_rng(23)
    sfx = "_pk" if packed else "_len"
    lengths, C = LENGTHS[0], 64
    B, Tk, tail, one, two, keep = layout(lengths, packed)
    m = pn.valid_mask(lengths, T)
    m2 = np.concatenate([m, m])

    def shifted(a):
        """a on the device, its first element one element behind the start of an (aligned) allocation."""
        a = np.ascontiguousarray(a)
        buf = torch.empty(a.size + 1, dtype=torch.from_numpy(a[:0].copy()).dtype, device=DEV)
        buf[1:] = torch.from_numpy(a.reshape(-1)).to(DEV)
        assert buf.data_ptr() % 16 == 0
        return buf[1:]

    def shifted_out(shape, np_dtype):
        t = shifted(np.zeros(shape, np_dtype))
        t.view(torch.uint8).fill_(255)
        return t

    for dt in (np.uint8, np.int16, np.int32):
        x = rng.integers(1, 100, (B, T, C)).astype(dt)
        want = two(bn.split(x, lengths))
        src, dst = shifted(one(x)), shifted_out(want.shape, dt)
        call("sparch_bidir_split" + sfx, B, Tk, C, x.itemsize, ptr(src), ptr(dst), *tail)
        assert np.array_equal(N(dst).reshape(want.shape), want), dt
    g = np.where(m2[:, :, None], rng.standard_normal((2 * B, T, C)), 0).astype(np.float32)
    want = one(bn.split_bwd(g, lengths))
    src, dst = shifted(two(g)), shifted_out(want.shape, np.float32)
    call("sparch_bidir_split_bwd" + sfx, B, Tk, C, ptr(src), ptr(dst), *tail)
    assert same_bits(N(dst).reshape(want.shape), want)
    s = np.where(m2[:, :, None], (rng.random((2 * B, T, C)) < 0.4), 0).astype(np.int16) * np.int16(0x3F80)
    want = one(bn.join(s, lengths))
    src, y16, y32 = shifted(two(s)), shifted_out(want.shape, np.int16), shifted_out(want.shape, np.float32)
    count = torch.zeros(2 * C, dtype=torch.int32, device=DEV)
    call("sparch_bidir_join" + sfx, B, Tk, C, ptr(src), ptr(y16), ptr(y32), 2.0, ptr(count), *tail)
    assert np.array_equal(N(y16).reshape(want.shape), want)
    assert same_bits(N(y32).reshape(want.shape), (want != 0).astype(np.float32) * np.float32(2.0))
    assert np.array_equal(N(count).astype(np.int64), np.count_nonzero(want.reshape(-1, 2 * C), axis=0))
    gy = np.where(m[:, :, None], rng.standard_normal((B, T, 2 * C)), 0).astype(np.float32)
    gr = rng.standard_normal(2 * C).astype(np.float32)
    want = two(bn.join_bwd(gy, gr, 0.25, lengths))
    src, r, dst = shifted(one(gy)), shifted(gr), shifted_out(want.shape, np.float32)
    call("sparch_bidir_join_bwd" + sfx, B, Tk, C, ptr(src), ptr(r), 0.25, ptr(dst), *tail)
    assert same_bits(N(dst).reshape(want.shape), want)


def test_the_functional_wrappers_round_trip():
    """functional.bidir_split / bidir_join and their adjoints under the cfg keys the layer sets, padded and packed."""
    Fn = _Fn()
    from sparch_amd import snns
    lengths = LENGTHS[0]
    B, H = len(lengths), 64
    rng = np.random.default_rng(17)
    x = rng.standard_normal((B, T, H)).astype(np.float32)
    m = pn.valid_mask(lengths, T)
    L = snns.prepare_lengths(lengths, B, T, DEV)
    plan = snns.prepare_packing(lengths, B, T, DEV)
    cfgs = {"mask": ({"lengths": L}, lambda a: a, lambda a: a),
            "pack": ({"pack": plan, "pack2": snns.prepare_bidir_packing(plan, DEV)},
                     lambda a: pn.pack(a, lengths)[None], lambda a: bn.pack2(a, lengths)[None])}
    for name, (cfg, one, two) in cfgs.items():
        x2 = Fn.bidir_split(D(one(x)), cfg)
        assert same_bits(N(x2), two(bn.split(x, lengths))), name
        back = Fn.bidir_split_backward(x2, cfg)
        assert same_bits(N(back), one(np.where(m[:, :, None], 2 * x, 0).astype(np.float32))), name
        plane = (x2 > 0).to(torch.bfloat16)
        y32, y16, count = Fn.bidir_join(plane, cfg, scale=2.0)
        want = one(bn.join(bn.split((x > 0).astype(np.float32), lengths), lengths))
        assert same_bits(N(y32), (want * 2).astype(np.float32)) and same_bits(N(y16, torch.float32), want), name
        assert np.array_equal(N(count), want.reshape(-1, 2 * H).sum(0).astype(np.int32)), name
        g2 = Fn.bidir_join_backward(y32, None, 0.0, cfg)
        assert same_bits(N(g2), two(bn.split((x > 0).astype(np.float32) * 2, lengths))), name
    _Fn().check_status()
