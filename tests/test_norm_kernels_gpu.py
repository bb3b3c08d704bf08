"""
The G2 entry points of include/sparch_hip.h (sparch_amd/csrc/norm.hip), each called through the C ABI and compared
with its fp64 restatement in tests/norm_numpy.py (itself pinned to torch fp64 by tests/test_norm_numpy_host.py):

  sparch_bn_finalize            a: synthetic partials, every side of col_sum64's 16 row-lanes and of its unrolled
                                   path (r + 112 < n); dup, eval mode, the skip word, the counter, NULL save_*, the
                                   v < 0 clamp, error codes
                                b: the GEMM epilogue's partials of columns with mean/std up to 100 (the variance
                                   comes from sum(v^2)/M - mean^2, which cancels there), both DENSE_GEMM settings
  sparch_bn_colstat_exact       b: the fp64 column sums in three fp32 terms, columns with mean/std up to 1000, through
                                   sparch_bn_finalize: the variance to u * var
  sparch_bn_bwd_reduce          c: colpartial_kernel<1>: vector and scalar column tails, ragged row blocks
  sparch_bn_bwd_apply_planes    d: odd M, a striding grid, dy2 / dx NULL or not; against sparch_bn_bwd_apply
  sparch_layernorm_fwd / _bwd   e: H < 64, H % 64 != 0, Hn < H, M % 4 != 0, offset rows, dx aliasing dy
  sparch_colsum, sparch_colsum_clamped, sparch_add_halves   f

Two kinds of values, as in tests/test_gemm_layouts_gpu.py:
  dyadic  small integers over a power of two (and power-of-two M, mean, invstd where they are multiplied in): every
          fp32 product and sum of the kernel is exact, so the result must be the fp64 one, bit for bit;
  randn   a stated bound: a column sum to 2e-6 * sum|terms| + 1e-6 (the form the GEMM tests use; 64 fp32 adds per
          256-row block, fp64 from there), an elementwise result to relmax 2e-5 (test_bn_backward_apply_in_place_
          any_row_count's bar).  u = 2^-24 below is the unit roundoff of fp32.

Every shape and pointer a kernel gets is valid; the error-code cases are refused on the host before any launch.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import norm_numpy as nn_
from tests.guarded import embed, guard_arena
from tests.kit import DEV, EALIGN, EINVAL, EWORKSPACE, F32, D, N, bits, nan_, relmax, same_bits, within
from tests.kit import capi as _capi

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
EPS = 1e-5
MOM32 = float(np.float32(nn_.BN_MOMENTUM))


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


# ================================================================================================ a. bn_finalize
class Finalize:
    """Device state of a sequence of sparch_bn_finalize calls on one set of buffers."""

    def __init__(self, s, ss, gamma, beta, rm, rv, skip=None, nbt=None):
        self.H = int(np.asarray(gamma).size)
        self.n_tiles = int(np.asarray(s).shape[0])
        self.ws = D(np.concatenate([np.asarray(s).reshape(-1), np.asarray(ss).reshape(-1)]), F32)
        self.gamma, self.beta, self.rm, self.rv = D(gamma, F32), D(beta, F32), D(rm, F32), D(rv, F32)
        self.skip = None if skip is None else torch.tensor([skip, 0, 0, 0], dtype=torch.int32, device=DEV)
        self.nbt = None if nbt is None else torch.tensor([nbt], dtype=torch.int64, device=DEV)
        self.o = {k: nan_(self.H) for k in ("scale", "shift", "save_mean", "save_invstd")}

    def call(self, M, dup=1, momentum=nn_.BN_MOMENTUM, training=1, save=True, ws=True, H=None, n_tiles=None,
             gamma=True):
        c = _capi()
        p = c.ptr
        rc = c.lib.sparch_bn_finalize(self.H if H is None else H, M, self.n_tiles if n_tiles is None else n_tiles, dup,
                                      p(self.ws) if ws else None, p(self.gamma) if gamma else None, p(self.beta),
                                      p(self.rm), p(self.rv), momentum, EPS, training, p(self.o["scale"]),
                                      p(self.o["shift"]), p(self.o["save_mean"]) if save else None,
                                      p(self.o["save_invstd"]) if save else None, p(self.skip), p(self.nbt), None)
        torch.cuda.synchronize()
        return rc

    def out(self):
        r = {k: N(v) for k, v in self.o.items()}
        r["running_mean"], r["running_var"] = N(self.rm), N(self.rv)
        return r


FIN_M = 128


def dyadic_partials(H, n_tiles, seed):
    """Partials k/8 whose fp64 sums are exact in any order; columns alternate in sign; with M = 128 the variance
    sum(ss)/M - (sum(s)/M)^2 >= 4n/128 - (n/128)^2 > 0 for n <= 512 tiles."""
    rng = np.random.default_rng(seed)
    sign = np.where(np.arange(H) % 2 == 0, 1.0, -1.0)
    s = (rng.integers(0, 9, (n_tiles, H)) / 8.0 * sign).astype(np.float32)
    ss = (rng.integers(32, 65, (n_tiles, H)) / 8.0).astype(np.float32)
    gamma = (rng.random(H) + 0.5).astype(np.float32)
    beta = rng.standard_normal(H).astype(np.float32)
    rm = ((rng.random(H) + 0.5) * sign).astype(np.float32)          # the sign of the column's mean: no cancellation
    rv = (rng.random(H) + 0.5).astype(np.float32)
    return s, ss, gamma, beta, rm, rv


def check_finalize(got, ref, beta, what):
    """save_mean bit-equal; invstd, scale, running stats to rtol 1e-6; shift to 1e-6 * (|beta| + |mean * scale|):
    fewer than ten fp32 roundings plus a device sqrtf and divide, each within a few 2^-24."""
    assert same_bits(got["save_mean"], f32(ref["mean"])), f"{what}: save_mean"
    for k, r in (("save_invstd", "invstd"), ("scale", "scale"), ("running_mean", "running_mean"),
                 ("running_var", "running_var")):
        np.testing.assert_allclose(got[k], ref[r], rtol=1e-6, atol=0, err_msg=f"{what}: {k}")
    within(got["shift"], ref["shift"], 1e-6 * (np.abs(beta.astype(np.float64)) + np.abs(ref["mean"] * ref["scale"])),
           f"{what}: shift")


@pytest.mark.parametrize("n_tiles", [1, 15, 16, 17, 112, 113, 128, 129, 257])
@pytest.mark.parametrize("H", [1, 15, 16, 17, 260])
def test_bn_finalize_from_dyadic_partials(H, n_tiles):
    s, ss, gamma, beta, rm, rv = dyadic_partials(H, n_tiles, 1000 * H + n_tiles)
    f = Finalize(s, ss, gamma, beta, rm, rv)
    assert f.call(FIN_M) == 0
    ref = nn_.bn_finalize(s, ss, FIN_M, 1, gamma, beta, rm, rv, momentum=MOM32, eps=EPS)
    check_finalize(f.out(), ref, beta, f"H={H} n_tiles={n_tiles}")


@pytest.mark.parametrize("H,n_tiles", [(17, 3), (260, 129)])
def test_bn_finalize_dup_changes_only_the_running_variance(H, n_tiles):
    s, ss, gamma, beta, rm, rv = dyadic_partials(H, n_tiles, 5)
    outs = {}
    for dup in (1, 2):
        f = Finalize(s, ss, gamma, beta, rm, rv)
        assert f.call(FIN_M, dup=dup) == 0
        outs[dup] = f.out()
        check_finalize(outs[dup], nn_.bn_finalize(s, ss, FIN_M, dup, gamma, beta, rm, rv, momentum=MOM32, eps=EPS), beta,
                       f"dup={dup}")
    for k in outs[1]:
        assert same_bits(outs[1][k], outs[2][k]) == (k != "running_var"), k
    # from running_var = 0 the update is momentum * unbiased alone: the two differ by the ratio of n / (n - 1)
    z = {}
    for dup in (1, 2):
        f = Finalize(s, ss, gamma, beta, rm, np.zeros(H))
        assert f.call(FIN_M, dup=dup) == 0
        z[dup] = np.float64(f.out()["running_var"])
    n1, n2 = float(FIN_M), 2.0 * FIN_M
    np.testing.assert_allclose(z[2] / z[1], (n2 / (n2 - 1)) / (n1 / (n1 - 1)), rtol=1e-6)


def test_bn_finalize_eval_mode_reads_the_running_statistics():
    H = 37
    s, ss, gamma, beta, rm, rv = dyadic_partials(H, 1, 6)
    f = Finalize(s, ss, gamma, beta, rm, rv, skip=0, nbt=41)
    assert f.call(FIN_M, training=0, ws=False) == 0
    got, ref = f.out(), nn_.bn_eval(gamma, beta, rm, rv, eps=EPS)
    assert same_bits(got["running_mean"], rm) and same_bits(got["running_var"], rv) and int(N(f.nbt)[0]) == 41
    assert same_bits(got["save_mean"], rm)
    np.testing.assert_allclose(got["save_invstd"], ref["invstd"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(got["scale"], ref["scale"], rtol=1e-6, atol=0)
    within(got["shift"], ref["shift"], 1e-6 * (np.abs(beta.astype(np.float64)) + np.abs(ref["mean"] * ref["scale"])), "shift")
    # M, n_tiles and dup play no part either
    g = Finalize(s, ss, gamma, beta, rm, rv)
    assert g.call(0, dup=0, training=0, ws=False, n_tiles=0) == 0
    for k, v in g.out().items():
        assert same_bits(v, got[k]), k


def test_bn_finalize_skip_word_and_counter():
    H, n_tiles = 37, 17
    s, ss, gamma, beta, rm, rv = dyadic_partials(H, n_tiles, 7)
    plain = Finalize(s, ss, gamma, beta, rm, rv, skip=0, nbt=5)
    assert plain.call(FIN_M) == 0
    want = plain.out()
    assert int(N(plain.nbt)[0]) == 6
    assert not same_bits(want["running_mean"], rm) and not same_bits(want["running_var"], rv)
    assert plain.call(FIN_M) == 0 and int(N(plain.nbt)[0]) == 7          # exactly one per call
    assert N(plain.skip).tolist() == [0, 0, 0, 0]
    skipped = Finalize(s, ss, gamma, beta, rm, rv, skip=1, nbt=5)
    assert skipped.call(FIN_M) == 0
    got = skipped.out()
    assert same_bits(got["running_mean"], rm) and same_bits(got["running_var"], rv) and int(N(skipped.nbt)[0]) == 5
    for k in ("scale", "shift", "save_mean", "save_invstd"):
        assert same_bits(got[k], want[k]), k
    assert N(skipped.skip).tolist() == [1, 0, 0, 0]
    # no skip word and no counter at all: the statistics move as with a zero word
    bare = Finalize(s, ss, gamma, beta, rm, rv)
    assert bare.call(FIN_M) == 0
    for k, v in bare.out().items():
        assert same_bits(v, want[k]), k


def test_bn_finalize_without_save_outputs():
    H, n_tiles = 37, 17
    s, ss, gamma, beta, rm, rv = dyadic_partials(H, n_tiles, 8)
    a, b = Finalize(s, ss, gamma, beta, rm, rv), Finalize(s, ss, gamma, beta, rm, rv)
    assert a.call(FIN_M) == 0 and b.call(FIN_M, save=False) == 0
    ga, gb = a.out(), b.out()
    for k in ("scale", "shift", "running_mean", "running_var"):
        assert same_bits(ga[k], gb[k]), k
    assert np.isnan(gb["save_mean"]).all() and np.isnan(gb["save_invstd"]).all()     # untouched


def constant_column_partials(M=128):
    """One tile of M rows of a constant c: s = M * c and ss = fl32(M * c^2) = M * fl32(c^2) are what an exact
    fp32-rounded sum holds; c is chosen so that fl32(c^2) < c^2, i.e. ss/M - (s/M)^2 < 0 in fp64."""
    for k in range(1, 200):
        c = np.float32(0.1) * np.float32(k)
        sq32 = np.float32(np.float64(c) * np.float64(c))
        if np.float64(sq32) < np.float64(c) * np.float64(c):
            return c, np.float32(M * np.float64(c)), np.float32(M * np.float64(sq32))
    raise AssertionError("no such constant")


def test_bn_finalize_clamps_a_variance_that_rounds_negative():
    M = 128
    c, s, ss = constant_column_partials(M)
    assert np.float64(ss) / M - (np.float64(s) / M) ** 2 < 0.0          # the fp64 expression of the kernel, on the CPU
    assert np.float64(s) / M == np.float64(c)
    one = np.ones(1, np.float32)
    f = Finalize([[s]], [[ss]], one, 0 * one, 0 * one, one)
    assert f.call(M, momentum=1.0) == 0            # momentum 1: running_var = the unbiased variance itself
    got = f.out()
    assert got["running_var"][0] == 0.0 and got["running_mean"][0] == c and got["save_mean"][0] == c
    np.testing.assert_allclose(got["save_invstd"], 1.0 / np.sqrt(EPS), rtol=1e-6)
    np.testing.assert_allclose(got["scale"], 1.0 / np.sqrt(EPS), rtol=1e-6)


def test_bn_finalize_error_codes():
    s, ss, gamma, beta, rm, rv = dyadic_partials(4, 2, 9)
    f = Finalize(s, ss, gamma, beta, rm, rv, skip=0, nbt=3)
    assert f.call(FIN_M, H=0) == EINVAL
    assert f.call(FIN_M, dup=0) == EINVAL
    assert f.call(FIN_M, n_tiles=0) == EINVAL
    assert f.call(FIN_M, gamma=False) == EINVAL
    assert f.call(FIN_M, ws=False) == EINVAL
    assert f.call(0) == EINVAL
    # one value per column has no unbiased variance (n - 1 = 0; nn.BatchNorm1d raises): refused, not a non-finite
    # running_var; two values (M = 1 seen twice, or M = 2) are fine
    assert f.call(1, dup=1) == EINVAL
    got = f.out()
    assert same_bits(got["running_mean"], rm) and same_bits(got["running_var"], rv) and int(N(f.nbt)[0]) == 3
    assert all(np.isnan(got[k]).all() for k in ("scale", "shift", "save_mean", "save_invstd"))     # nothing launched
    assert f.call(1, dup=2) == 0 and np.isfinite(f.out()["running_var"]).all()
    assert f.call(2, dup=1) == 0 and np.isfinite(f.out()["running_var"]).all()
    assert f.call(1, dup=1, training=0) == 0


def test_python_layer_refuses_a_single_value_per_channel_as_torch_does():
    from sparch_amd import functional as Fn
    H = 8
    x = torch.randn(1, H, device=DEV)
    ws = torch.cat([x.reshape(-1), (x * x).reshape(-1)])
    ones, zeros = torch.ones(H, device=DEV), torch.zeros(H, device=DEV)
    rm, rv = zeros.clone(), ones.clone()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        Fn._Norm.forward("batchnorm", x, ws, ones, zeros, rm, rv, True, 1)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        torch.nn.functional.batch_norm(x.cpu(), zeros.cpu(), ones.cpu(), ones.cpu(), zeros.cpu(), True, 0.05, 1e-5)
    assert torch.equal(rm, zeros) and torch.equal(rv, ones)
    _, scale, shift, _ = Fn._Norm.forward("batchnorm", x, ws, ones, zeros, rm, rv, True, 2)      # the row seen twice
    _, scale_e, _, _ = Fn._Norm.forward("batchnorm", x, ws, ones, zeros, rm, rv, False, 1)       # eval: any M
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rv).all()) and bool(torch.isfinite(scale).all()) and bool(torch.isfinite(scale_e).all())


# ============================================================================ b. GEMM epilogue -> finalize, off centre
RATIOS = (0.0, 1.0, 10.0, 100.0)     # column mean / std, a quarter of the columns each (column h: RATIOS[h % 4])


@pytest.mark.parametrize("dense", ["split6", "fp32"])
@pytest.mark.parametrize("M,K,H", [(300, 70, 36), (1000, 41, 129)])
def test_gemm_colstats_and_finalize_of_off_centre_columns(M, K, H, dense, monkeypatch, record_property):
    """BatchNorm's variance is sum(v^2)/M - mean^2 from fp32 per-tile partials: the error grows as 1 + mean^2/var.
    The reference is fp64 statistics of the C the kernel stored (this judges the statistics, not the product).

    Per-tile partials: each is a chain of at most 32 sequential fp32 adds in a lane (2 MFMA tiles x 16 rows; both
    the fp32 kernel of gemm.hip and the general split kernel of gemm_spike.hip, WI = 2, which these ragged shapes
    take), one shuffle add and one LDS add, plus one rounding for v * v — worst-case rounding bounds, not measurements:
        |sum_got - sum| <= 34 u sum|v|        |sumsq_got - sumsq| <= 35 u sum v^2
    Finalize (fp64 from the partials, one rounding to fp32 each):
        |mean_got - mean| <= 34 u E|v| + u |mean|
        |var_got - var|   <= u (35 E[v^2] + 68 |mean| E|v|) + u var
    var_got is read as running_var of a call with momentum 1 from running_var 0: fl32(var n/(n-1)), scaled back in
    fp64 — the one rounding the bound's last term allows.
    Observed on an MI355X (both shapes, both settings): at most 0.045 of either bound; the variance's relative error
    is 1e-7, 2.5e-7, 1.4e-5, 1.4e-3 at mean/std = 0, 1, 10, 100 ("BatchNorm arithmetic")."""
    from sparch_amd import functional as Fn
    monkeypatch.setattr(Fn, "DENSE_GEMM", dense)
    g = torch.Generator().manual_seed(M + H)
    A = (torch.rand(M, K, generator=g) < 0.05).float()
    W = torch.randn(H, K, generator=g) * 0.1
    lin = A.double() @ W.double().T
    ratio = torch.tensor(RATIOS, dtype=torch.float64)[torch.arange(H) % 4]
    bias = (ratio * lin.std(0, unbiased=False) - lin.mean(0)).float()
    C, ws = Fn.gemm_nt(A.to(DEV), W.to(DEV), bias.to(DEV), colstat=True)
    n_tiles = (M + 127) // 128
    assert ws.numel() == 2 * n_tiles * H
    v = N(C).astype(np.float64)
    assert relmax(v, (lin + bias.double()).numpy()) <= 2e-5
    got_ws = N(ws).astype(np.float64).reshape(2, n_tiles, H)
    s_ref, ss_ref = nn_.tile_partials(v)
    abs_ref, _ = nn_.tile_partials(np.abs(v))
    within(got_ws[0], s_ref, 34 * U * abs_ref + 1e-300, "per-tile sum")
    within(got_ws[1], ss_ref, 35 * U * ss_ref + 1e-300, "per-tile sum of squares")

    gamma, beta = np.ones(H, np.float32), np.zeros(H, np.float32)
    c = _capi()
    o = {k: nan_(H) for k in ("scale", "shift", "mean", "invstd")}
    rm, rv = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    gd, bd = D(gamma, F32), D(beta, F32)
    c.check(c.lib.sparch_bn_finalize(H, M, n_tiles, 1, c.ptr(ws), c.ptr(gd), c.ptr(bd), c.ptr(rm), c.ptr(rv),
                                     1.0, EPS, 1, c.ptr(o["scale"]), c.ptr(o["shift"]), c.ptr(o["mean"]),
                                     c.ptr(o["invstd"]), None, None, None), "sparch_bn_finalize")
    mean_got = N(o["mean"]).astype(np.float64)
    var_got = N(rv).astype(np.float64) * ((M - 1.0) / M)
    assert same_bits(N(rm), N(o["mean"]))
    mean, var = v.mean(0), v.var(0)
    e1, e2 = np.abs(v).mean(0), (v * v).mean(0)
    mean_bound = 34 * U * e1 + U * np.abs(mean)
    var_bound = U * (35 * e2 + 68 * np.abs(mean) * e1) + U * var
    mean_ratio, var_ratio = np.abs(mean_got - mean) / mean_bound, np.abs(var_got - var) / var_bound
    for i, r in enumerate(RATIOS):
        record_property(f"mean_err_over_bound[mean/std={r:g}]", float(mean_ratio[i::4].max()))
        record_property(f"var_err_over_bound[mean/std={r:g}]", float(var_ratio[i::4].max()))
        record_property(f"var_relerr[mean/std={r:g}]", float((np.abs(var_got - var) / var)[i::4].max()))
        print(f"colstats {dense} ({M},{K},{H}) mean/std={r:g}: mean err {mean_ratio[i::4].max():.3f} of its bound, "
              f"var err {var_ratio[i::4].max():.3f} of its bound, var rel err {(np.abs(var_got - var) / var)[i::4].max():.2e}")
    np.testing.assert_allclose(np.abs(mean[1::4]) / np.sqrt(var[1::4]), 1.0, rtol=1e-3)      # the classes are what they say
    np.testing.assert_allclose(np.abs(mean[3::4]) / np.sqrt(var[3::4]), 100.0, rtol=1e-3)
    assert (mean_ratio <= 1.0).all(), f"mean: {mean_ratio.max()} of the bound"
    assert (var_ratio <= 1.0).all(), f"var: {var_ratio.max()} of the bound"
    # what the cells are handed: invstd and the fold, from the variance the kernel arrived at
    np.testing.assert_allclose(N(o["invstd"]), 1.0 / np.sqrt(var_got + EPS), rtol=1e-6)


@pytest.mark.parametrize("M,H", [(1, 17), (2, 1), (9, 130), (17, 36), (33, 260), (130, 16), (1024, 20)])
def test_exact_colstats_and_finalize_of_off_centre_columns(M, H, record_property):
    """sparch_bn_colstat_exact: the fp64 column sums of x and x * x as three fp32 terms each, which sparch_bn_finalize
    sums as three tile rows.  Columns with mean / std = 0, 10, 100, 1000 (the baselines' readout reaches 180).  M: one
    row, fewer rows than the 16 row-lanes, more, a multiple of them and not; H: one column, a ragged last block of 16.

    The three terms of a sum add up to it exactly in fp64 (24 + 24 + 24 >= 53 bits), and the fp64 sums differ from
    numpy's only by the order of at most M additions: 2^-53 M sum|terms|.  The variance finalize forms from them is a
    difference in fp64 of two numbers that large, then one rounding to fp32:
        |var_got - var| <= u var + 2^-52 M (E[v^2] + 2 |mean| E|v|)
    so at mean / std = 1000 and M = 1024 the relative error stays at u, where the epilogue's partials give 1.4e-3 at
    mean / std = 100 (test_gemm_colstats_and_finalize_of_off_centre_columns)."""
    c = _capi()
    rng = np.random.default_rng(100 * M + H)
    ratios = np.array([0.0, 10.0, 100.0, 1000.0])[np.arange(H) % 4]
    v = rng.standard_normal((M, H))
    if M > 1:
        v = (v - v.mean(0)) / v.std(0) * rng.uniform(0.05, 2.0, H)
        v = v + ratios * v.std(0)
    x = embed(D(v, F32))
    v = N(x).astype(np.float64)
    ws = embed(nan_(6, H))
    assert c.lib.sparch_bn_colstat_exact(M, H, c.ptr(x), c.ptr(ws), None) == 0
    got = N(ws).astype(np.float64).reshape(2, 3, H)
    x.check("x")
    ws.check("colstat_ws")
    order = 2.0 ** -53 * M
    within(got[0].sum(0), v.sum(0), order * np.abs(v).sum(0) + 1e-300, "column sum")
    within(got[1].sum(0), (v * v).sum(0), order * (v * v).sum(0) + 1e-300, "column sum of squares")
    assert (np.abs(got[:, 1]) <= 2 * U * np.abs(got[:, 0])).all() and (np.abs(got[:, 2]) <= 2 * U * np.abs(got[:, 1])).all()
    for bad in ((0, H, c.ptr(x), c.ptr(ws)), (M, 0, c.ptr(x), c.ptr(ws)), (M, H, None, c.ptr(ws)), (M, H, c.ptr(x), None)):
        assert c.lib.sparch_bn_colstat_exact(*bad, None) == EINVAL
    if M == 1:          # one value per column: finalize refuses, as nn.BatchNorm1d does
        return
    o = {k: nan_(H) for k in ("scale", "shift", "mean", "invstd")}
    rm, rv = torch.zeros(H, device=DEV), torch.zeros(H, device=DEV)
    gd, bd = D(np.ones(H), F32), D(np.zeros(H), F32)
    c.check(c.lib.sparch_bn_finalize(H, M, 3, 1, c.ptr(ws), c.ptr(gd), c.ptr(bd), c.ptr(rm), c.ptr(rv), 1.0, EPS, 1,
                                     c.ptr(o["scale"]), c.ptr(o["shift"]), c.ptr(o["mean"]), c.ptr(o["invstd"]), None,
                                     None, None), "sparch_bn_finalize")
    mean, var = v.mean(0), v.var(0)
    var_got = N(rv).astype(np.float64) * ((M - 1.0) / M)
    e1, e2 = np.abs(v).mean(0), (v * v).mean(0)
    within(N(o["mean"]), mean, U * np.abs(mean) + 2.0 ** -52 * M * e1 + 1e-300, "mean")
    f = within(var_got, var, U * var + 2.0 ** -52 * M * (e2 + 2 * np.abs(mean) * e1), "variance")
    record_property("var_err_over_bound", f)
    record_property("var_relerr", float((np.abs(var_got - var) / var).max()))
    np.testing.assert_allclose(N(o["invstd"]), 1.0 / np.sqrt(var_got + EPS), rtol=1e-6)


# ================================================================================== c. bn_bwd_reduce, f. colsum
PAIRS =[(1, 1), (3, 3), (255, 4), (256, 30), (257, 252), (513, 256), (513, 260), (257, 1028), (1, 260), (255, 1028),
         (3, 30), (256, 3)]
assert {m for m, _ in PAIRS} == {1, 3, 255, 256, 257, 513} and {h for _, h in PAIRS} == {1, 3, 4, 30, 252, 256, 260, 1028}


def reduce_call(M, H, dy, x, mean, invstd, ws=None, ws_bytes=None):
    c = _capi()
    dg, db = nan_(H), nan_(H)
    need = c.lib.sparch_bn_bwd_workspace_bytes(M, H)
    assert need == 2 * ((M + 255) // 256) * H * 4
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = c.lib.sparch_bn_bwd_reduce(M, H, c.ptr(dy), c.ptr(x), c.ptr(mean), c.ptr(invstd), c.ptr(dg), c.ptr(db),
                                    c.ptr(ws), need if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return rc, dg, db


@pytest.mark.parametrize("M,H", PAIRS)
def test_bn_bwd_reduce_dyadic_is_exact(M, H):
    """dy, x, mean in k/8, invstd in {1/2, 1, 2}: every term is a multiple of 1/128 below 8 and every sum stays
    below 2^24 / 128."""
    rng = np.random.default_rng(M * 7 + H)
    dy = rng.integers(-8, 9, (M, H)) / 8.0
    x = rng.integers(-8, 9, (M, H)) / 8.0
    mean = rng.integers(-8, 9, H) / 8.0
    invstd = 2.0 ** rng.integers(-1, 2, H)
    with guard_arena(None, nbytes=1 << 20) as arena:
        ws = arena.empty(2 * ((M + 255) // 256) * H * 4, dtype=torch.uint8)       # exactly the queried size
        rc, dg, db = reduce_call(M, H, D(dy, F32), D(x, F32), D(mean, F32), D(invstd, F32), ws=ws)
        assert rc == 0
    dgamma, dbeta = nn_.bn_bwd_reduce(dy, x, mean, invstd)
    assert same_bits(N(dg), f32(dgamma)) and same_bits(N(db), f32(dbeta))
    assert (f32(dgamma).astype(np.float64) == dgamma).all()


@pytest.mark.parametrize("M,H", PAIRS)
def test_bn_bwd_reduce_randn_columns_with_offset_and_scale(M, H):
    rng = np.random.default_rng(M * 11 + H)
    scale, off = np.exp(rng.standard_normal(H)), 10.0 * rng.standard_normal(H)
    x = f32(rng.standard_normal((M, H)) * scale + off)
    dy = f32(rng.standard_normal((M, H)))
    mean = f32(x.astype(np.float64).mean(0))
    invstd = f32(1.0 / np.sqrt(x.astype(np.float64).var(0) + EPS))
    rc, dg, db = reduce_call(M, H, D(dy, F32), D(x, F32), D(mean, F32), D(invstd, F32))
    assert rc == 0
    dgamma, dbeta = nn_.bn_bwd_reduce(dy, x, mean, invstd)
    t1, t0 = nn_.bn_bwd_terms(dy, x, mean, invstd)
    within(N(dg), dgamma, 2e-6 * t1 + 1e-6, "dgamma")
    within(N(db), dbeta, 2e-6 * t0 + 1e-6, "dbeta")


def test_bn_bwd_reduce_error_codes():
    M, H = 257, 12
    dy, x = torch.zeros(M, H, device=DEV), torch.zeros(M, H, device=DEV)
    mean, invstd = torch.zeros(H, device=DEV), torch.ones(H, device=DEV)
    need = 2 * 2 * H * 4
    rc, dg, db = reduce_call(M, H, dy, x, mean, invstd, ws_bytes=need - 1)
    assert rc == EWORKSPACE and np.isnan(N(dg)).all() and np.isnan(N(db)).all()
    off = embed(dy, H, 1)                                            # 4 bytes behind a 256-byte boundary
    rc, dg, db = reduce_call(M, H, off, x, mean, invstd)
    assert rc == EALIGN and np.isnan(N(dg)).all()
    rc, dg, db = reduce_call(M, H, dy, embed(x, H, 1), mean, invstd)
    assert rc == EALIGN and np.isnan(N(dg)).all()
    off.check("dy")


def colsum_call(M, H, x, ws=None, ws_bytes=None):
    c = _capi()
    out = nan_(H)
    need = c.lib.sparch_bn_bwd_workspace_bytes(M, H)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    rc = c.lib.sparch_colsum(M, H, c.ptr(x), c.ptr(out), c.ptr(ws), need if ws_bytes is None else ws_bytes, None)
    torch.cuda.synchronize()
    return rc, out


@pytest.mark.parametrize("M,H", PAIRS)
def test_colsum_dyadic_exact_and_randn_bounded(M, H):
    rng = np.random.default_rng(M * 13 + H)
    x = rng.integers(-64, 65, (M, H)) / 8.0
    rc, out = colsum_call(M, H, D(x, F32))
    assert rc == 0 and same_bits(N(out), f32(x.sum(0)))
    x = f32(rng.standard_normal((M, H)) * np.exp(rng.standard_normal(H)) + rng.standard_normal(H))
    rc, out = colsum_call(M, H, D(x, F32))
    assert rc == 0
    within(N(out), x.astype(np.float64).sum(0), 2e-6 * np.abs(x.astype(np.float64)).sum(0) + 1e-6, "colsum")
    rc, out = colsum_call(M, H, D(x, F32), ws_bytes=2 * ((M + 255) // 256) * H * 4 - 1)
    assert rc == EWORKSPACE and np.isnan(N(out)).all()


# ================================================================================== d. bn_bwd_apply_planes
def planes_case(M, H, seed):
    """Plausible column constants rather than the statistics of these few rows (M = 1 has none): the pass is the
    formula dx = gamma * invstd * (dy - dbeta/M - xhat * dgamma/M) whatever they hold."""
    g = torch.Generator().manual_seed(seed)
    dy, dy2 = torch.randn(M, H, generator=g), torch.randn(M, H, generator=g)
    x = torch.randn(M, H, generator=g) * 2 + 0.5
    mean = 0.5 + 0.1 * torch.randn(H, generator=g)
    invstd = 0.5 / (torch.rand(H, generator=g) + 0.5)
    gamma = torch.rand(H, generator=g) + 0.5
    dgamma, dbeta = torch.randn(H, generator=g) * M ** 0.5, torch.randn(H, generator=g) * M ** 0.5
    return dy, dy2, x, mean, invstd, gamma, dgamma, dbeta


@pytest.mark.parametrize("M,H", [(1, 8), (2, 8), (7, 16), (257, 264), (8195, 8), (1031, 2056)])
def test_bn_bwd_apply_planes_against_apply_and_fp64(M, H):
    """(8195, 8) and (1031, 2056): bx = 1 and 2 column blocks with more than 2 * by rows, so the grid strides."""
    c = _capi()
    p = c.ptr
    dy, dy2, x, mean, invstd, gamma, dgamma, dbeta = planes_case(M, H, M + H)
    cols = [t.to(DEV) for t in (mean, invstd, gamma, dgamma, dbeta)]
    xd = x.to(DEV)
    for second in (False, True):
        total = dy + dy2 if second else dy                       # one fp32 add, as the kernel's
        ref = nn_.bn_bwd_apply(total.numpy(), x.numpy(), mean.numpy(), invstd.numpy(), gamma.numpy(), dgamma.numpy(),
                               dbeta.numpy())
        want, totd = nan_(M, H), total.to(DEV)
        c.check(c.lib.sparch_bn_bwd_apply(M, H, p(totd), p(xd), *[p(t) for t in cols], p(want), None),
                "sparch_bn_bwd_apply")
        want = N(want)
        assert relmax(want, ref) <= 2e-5
        dyd, dy2d = dy.to(DEV), (dy2.to(DEV) if second else None)
        runs = {}
        for with_dx in (True, False):
            # both outputs inside guard bands: the last trip of an odd M must write no row M
            planes = embed(torch.full((3 * M, H), 0x7FC0, dtype=torch.int16, device=DEV), H, 0)
            dx = embed(nan_(M, H), H, 0) if with_dx else None
            c.check(c.lib.sparch_bn_bwd_apply_planes(M, H, p(dyd), p(dy2d), p(xd), *[p(t) for t in cols], p(planes),
                                                     p(dx), None), "sparch_bn_bwd_apply_planes")
            runs[with_dx] = (N(planes).view(np.uint16).reshape(3, M, H), None if dx is None else N(dx))
            planes.check(f"M={M} H={H}: planes")
            if dx is not None:
                dx.check(f"M={M} H={H}: dx")
        pl, dx = runs[True]
        what = f"M={M} H={H} dy2={'given' if second else 'NULL'}"
        assert same_bits(dx, want), f"{what}: dx differs from sparch_bn_bwd_apply on dy + dy2"
        assert relmax(dx, ref) <= 2e-5, what
        assert (pl[0] == (bits(dx) >> 16).astype(np.uint16)).all(), f"{what}: plane 0 is not the truncation of dx"
        f = nn_.planes_to_f32(pl)
        assert same_bits((f[0] + f[1]) + f[2], dx), f"{what}: the planes do not add up to dx"
        assert (pl == nn_.split3_planes(dx)).all(), f"{what}: planes differ from the truncation split of dx"
        assert (runs[False][0] == pl).all(), f"{what}: planes differ when dx is NULL"
        assert same_bits(N(dyd), dy.numpy()) and same_bits(N(xd), x.numpy())       # inputs untouched


def test_bn_bwd_apply_planes_error_codes():
    c = _capi()
    p = c.ptr
    M = 5

    def attempt(H, planes=None, dy=None, dy2=None, dx=None):
        z = torch.zeros(M, max(H, 16), device=DEV)
        col = torch.ones(max(H, 16), device=DEV)
        planes = torch.full((3 * M, 16), 0x7FC0, dtype=torch.int16, device=DEV) if planes is None else planes
        rc = c.lib.sparch_bn_bwd_apply_planes(M, H, p(z if dy is None else dy), p(dy2), p(z), p(col), p(col), p(col),
                                              p(col), p(col), p(planes), p(dx), None)
        torch.cuda.synchronize()
        assert (N(planes).view(np.uint16) == 0x7FC0).all()
        return rc

    assert attempt(12) == EINVAL
    assert attempt(0) == EINVAL
    mis = embed(torch.full((3 * M, 16), 0x7FC0, dtype=torch.int16, device=DEV), 16, 1)      # 2 bytes off
    assert attempt(16, planes=mis) == EALIGN
    mis.check("planes")
    assert attempt(16, dy=embed(torch.zeros(M, 16, device=DEV), 16, 1)) == EALIGN
    assert attempt(16, dy2=embed(torch.zeros(M, 16, device=DEV), 16, 1)) == EALIGN
    assert attempt(16, dx=embed(torch.zeros(M, 16, device=DEV), 16, 1)) == EALIGN


# ================================================================================== e. LayerNorm
LN_WIDTHS = [(1, 1), (7, 7), (63, 63), (64, 64), (65, 65), (260, 260), (1030, 1030), (8, 5), (128, 100), (264, 260)]
LN_OFFSETS = (0.0, 1.0, 10.0, 100.0, -100.0)      # o / s of row m: LN_OFFSETS[m % 5]


def ln_case(M, H, Hn, seed):
    """Rows randn * s + o with o/s up to 100; the last row (M >= 3) is a constant 3; the padding columns hold 0 and
    gamma 0, as the layer passes them."""
    rng = np.random.default_rng(seed)
    s = np.exp(rng.standard_normal((M, 1)))
    o = s * np.asarray(LN_OFFSETS)[np.arange(M) % 5].reshape(M, 1)
    x = rng.standard_normal((M, H)) * s + o
    if M >= 3:
        x[M - 1] = 3.0
    gamma, beta = rng.random(H) + 0.5, rng.standard_normal(H)
    x[:, Hn:] = 0.0
    gamma[Hn:] = 0.0
    dy = rng.standard_normal((M, H))
    return f32(x), f32(gamma), f32(beta), f32(dy)


def ln_depth(Hn):
    """fp32 adds between an element and its row sum: ceil(Hn/64) in a lane, six shuffle steps."""
    return (Hn + 63) // 64 + 6


@pytest.mark.parametrize("M", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("H,Hn", LN_WIDTHS)
def test_layernorm_forward(M, H, Hn):
    """Against fp64.  The kernel is two-pass (mean, then centred squares), so a common offset of a row costs only the
    rounding of its fp32 mean: |mu_got - mu| <= dmu := (depth + 1) u max|x_row| (depth adds and the division).  y is
    held to the bar of test_projection_and_normalisation_vs_oracle, rtol 1e-4 + atol 2e-5 — y is the row in units of its
    own scale — plus what dmu moves it by, |gamma| rstd dmu (3e-6 at o/s = 100, Hn = 64); rstd to rtol 1e-4, where
    dmu enters only squared.  A row of variance 0 (Hn = 1, or constant): mu exact, rstd = 1/sqrt(eps), y = beta."""
    c = _capi()
    p = c.ptr
    x, gamma, beta, _ = ln_case(M, H, Hn, 1000 * M + H)
    y, mu, rstd = nan_(M, H), nan_(M), nan_(M)
    xd, gd, bd = D(x, F32), D(gamma, F32), D(beta, F32)
    c.check(c.lib.sparch_layernorm_fwd(M, H, Hn, p(xd), p(gd), p(bd), EPS, p(y), p(mu), p(rstd), None),
            "sparch_layernorm_fwd")
    y, mu, rstd = N(y), N(mu), N(rstd)
    ry, rmu, rrstd = nn_.layernorm_fwd(x, gamma, beta, Hn, eps=EPS)
    assert not y[:, Hn:].any() and same_bits(y[:, Hn:], np.zeros((M, H - Hn), np.float32)), "padding of y"
    dmu = (ln_depth(Hn) + 1) * U * np.abs(x[:, :Hn].astype(np.float64)).max(1)
    within(mu, rmu, dmu + 1e-300, "mu")
    np.testing.assert_allclose(rstd, rrstd, rtol=1e-4, atol=0, err_msg="rstd")
    bound = 1e-4 * np.abs(ry) + 2e-5 + np.abs(gamma.astype(np.float64))[None, :] * (rrstd * dmu)[:, None]
    within(y[:, :Hn], ry[:, :Hn], bound[:, :Hn], "y")
    flat = [m for m in range(M) if Hn == 1 or (M >= 3 and m == M - 1)]
    for m in flat:
        assert mu[m] == x[m, 0], "mean of a constant row"
        np.testing.assert_allclose(rstd[m], 1.0 / np.sqrt(EPS), rtol=1e-6)
        assert same_bits(y[m, :Hn], beta[:Hn]), "y of a constant row is beta"
    assert same_bits(N(xd), x)


@pytest.mark.parametrize("M", [1, 3, 4, 5, 257])
@pytest.mark.parametrize("H,Hn", LN_WIDTHS)
def test_layernorm_backward(M, H, Hn):
    """mu and rstd are handed in (the fp64 statistics rounded to fp32), and the fp64 reference uses the same values:
    dx per row to relmax 2e-5, dgamma / dbeta to 2e-6 * sum|terms| + 1e-6; dx written over dy gives the same bits."""
    c = _capi()
    p = c.ptr
    x, gamma, beta, dy = ln_case(M, H, Hn, 2000 * M + H)
    _, mu, rstd = nn_.layernorm_fwd(x, gamma, beta, Hn, eps=EPS)
    mu, rstd = f32(mu), f32(rstd)
    rdx, rdg, rdb = nn_.layernorm_bwd(dy, x, mu, rstd, gamma, Hn)
    t1, t0 = nn_.layernorm_bwd_terms(dy, x, mu, rstd)
    need = c.lib.sparch_bn_bwd_workspace_bytes(M, H)
    outs = []
    xd, mud, rstdd, gd = D(x, F32), D(mu, F32), D(rstd, F32), D(gamma, F32)
    with guard_arena(None, nbytes=4 << 20) as arena:
        for alias in (False, True):
            dyd = D(dy, F32)
            dx = dyd if alias else nan_(M, H)
            dg, db = nan_(H), nan_(H)
            ws = arena.empty(need, dtype=torch.uint8)
            c.check(c.lib.sparch_layernorm_bwd(M, H, Hn, p(dyd), p(xd), p(mud), p(rstdd), p(gd), p(dx),
                                               p(dg), p(db), p(ws), need, None), "sparch_layernorm_bwd")
            outs.append((N(dx), N(dg), N(db)))
            if not alias:
                assert same_bits(N(dyd), dy)
    dx, dg, db = outs[0]
    for a, b in zip(outs[0], outs[1]):
        assert same_bits(a, b), "dx aliasing dy changes the result"
    assert same_bits(dx[:, Hn:], np.zeros((M, H - Hn), np.float32)), "padding of dx"
    for m in range(M):
        assert relmax(dx[m, :Hn], rdx[m, :Hn]) <= 2e-5, f"dx row {m}: {relmax(dx[m, :Hn], rdx[m, :Hn])}"
    within(dg[:Hn], rdg[:Hn], 2e-6 * t1[:Hn] + 1e-6, "dgamma")
    within(db[:Hn], rdb[:Hn], 2e-6 * t0[:Hn] + 1e-6, "dbeta")
    assert np.isfinite(dg).all() and np.isfinite(db).all()
    within(db, rdb, 2e-6 * t0 + 1e-6, "dbeta, padding included")


def test_layernorm_error_codes():
    c = _capi()
    p = c.ptr
    M, H = 5, 8
    z, col, row = torch.zeros(M, H, device=DEV), torch.ones(H, device=DEV), torch.ones(M, device=DEV)
    y, mu, rstd = nan_(M, H), nan_(M), nan_(M)
    for Hn in (0, H + 1, -1):
        assert c.lib.sparch_layernorm_fwd(M, H, Hn, p(z), p(col), p(col), EPS, p(y), p(mu), p(rstd), None) == EINVAL
    need = c.lib.sparch_bn_bwd_workspace_bytes(M, H)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    dx, dg, db = nan_(M, H), nan_(H), nan_(H)

    def bwd(Hn, ws_bytes, dy=z):
        return c.lib.sparch_layernorm_bwd(M, H, Hn, p(dy), p(z), p(row), p(row), p(col), p(dx), p(dg), p(db), p(ws),
                                          ws_bytes, None)
    assert bwd(0, need) == EINVAL and bwd(H + 1, need) == EINVAL
    assert bwd(H, need - 1) == EWORKSPACE
    assert bwd(H, need, dy=embed(z, H, 1)) == EALIGN
    torch.cuda.synchronize()
    assert all(np.isnan(N(t)).all() for t in (y, mu, rstd, dx, dg, db))
    assert bwd(H, need) == 0


# ================================================================================== f. colsum_clamped, add_halves
CL_ROWS = [1, 16, 17, 112, 113, 129]


def clamped_call(ws, raws, lims, H, n_params=None, rows=None):
    """raws: None or a list of None / device tensors; lims: None or a flat list of 2 n floats."""
    c = _capi()
    n = ws.shape[0] if n_params is None else n_params
    outs = [nan_(H) for _ in range(max(n, 1))]
    raw_arr = None if raws is None else (ctypes.c_void_p * max(n, 1))(*[None if r is None else r.data_ptr()
                                                                       for r in raws[:max(n, 1)]])
    out_arr = (ctypes.c_void_p * max(n, 1))(*[o.data_ptr() for o in outs])
    lim_arr = None if lims is None else (ctypes.c_float * len(lims))(*lims)
    rc = c.lib.sparch_colsum_clamped(n, ws.shape[1] if rows is None else rows, H, c.ptr(ws), raw_arr, lim_arr, out_arr,
                                     None)
    torch.cuda.synchronize()
    return rc, [N(o) for o in outs]


@pytest.mark.parametrize("H", [1, 17, 260])
@pytest.mark.parametrize("n_params", [1, 3, 8])
def test_colsum_clamped_gate_is_torch_clamps(n_params, H):
    """Dyadic partials, so the fp64 sum is the fp32 result exactly; the raw parameters walk through: inside, exactly
    lo, exactly hi, one ulp outside each, NaN, one ulp inside each."""
    rng = np.random.default_rng(10 * n_params + H)
    lims = [(0.0, 1.0), (-1.0, 1.0), (float(np.float32(0.36787944)), float(np.float32(0.96)))]
    lims = [lims[j % 3] for j in range(n_params)]
    raws = []
    for j, (lo, hi) in enumerate(lims):
        raws.append(None if j % 3 == 1 else np.resize(nn_.edge_values(lo, hi), H + j)[j:])
    if n_params == 1:
        raws[0] = np.resize(nn_.edge_values(*lims[0])[1:], H)           # H = 1: the value exactly at lo
    flat = [v for lo_hi in lims for v in lo_hi]
    for rows in CL_ROWS:
        ws = rng.integers(-64, 65, (n_params, rows, H)) / 8.0
        wsd = D(ws, F32)
        raws_d = [None if r is None else D(r, F32) for r in raws]
        rc, outs = clamped_call(wsd, raws_d, flat, H)
        assert rc == 0
        ref = nn_.colsum_clamped(ws, raws, lims)
        for j in range(n_params):
            assert same_bits(outs[j], f32(ref[j])), f"rows={rows} param {j}"
            if raws[j] is not None and H >= 8:
                assert (outs[j] == 0).any() and (ws[j].sum(0)[outs[j] == 0] != 0).any(), "the gate never closed"
        plain = f32(ws.sum(1))
        rc, outs = clamped_call(wsd, raws_d, None, H)                 # lim NULL: nothing is gated
        assert rc == 0 and all(same_bits(outs[j], plain[j]) for j in range(n_params)), f"rows={rows} lim NULL"
        rc, outs = clamped_call(wsd, None, flat, H)                   # raw NULL altogether
        assert rc == 0 and all(same_bits(outs[j], plain[j]) for j in range(n_params)), f"rows={rows} raw NULL"


def test_colsum_clamped_refuses_other_parameter_counts():
    ws = torch.zeros(9, 4, 8, device=DEV)
    for n in (0, 9, -1):
        rc, outs = clamped_call(ws, None, None, 8, n_params=n)
        assert rc == EINVAL and all(np.isnan(o).all() for o in outs)
    rc, outs = clamped_call(ws, None, None, 8, n_params=8, rows=0)
    assert rc == EINVAL


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_add_halves(n):
    c = _capi()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(2 * n, generator=g) * torch.exp(3 * torch.randn(2 * n, generator=g))
    out = embed(torch.full((1, n), float("nan"), device=DEV), n, 0)
    xd = x.to(DEV)
    assert c.lib.sparch_add_halves(n, c.ptr(xd), c.ptr(out), None) == 0
    torch.cuda.synchronize()
    assert same_bits(N(out)[0], (x[:n] + x[n:]).numpy())
    out.check("out")
    assert c.lib.sparch_add_halves(0, c.ptr(xd), c.ptr(out), None) == EINVAL
