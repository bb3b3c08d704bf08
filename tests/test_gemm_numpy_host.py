"""
tests/gemm_numpy.py on the CPU, for every case of tests/test_gemm_planes_gpu.py (same seeds, same shapes): the fp64
reference is right, the planes are exact, the bound rule is wired up — and the bound is TIGHT enough: every mutant of
gemm_numpy.mutants (a second-order plane term or plane 2 of a weight lost on a quarter of K or in one row tile, a slab
missing from part of the reduction, truncation in bf16 mode, square partials taken before the bias) lands at least
2 x outside it.  That condition is what keeps the GPU test from being vacuous; if a seed or shape fails it, the seed or
shape changes, not the 2.  The last test records why the GPU file exists: the suite's fixed bound
2e-6 * sum|a||b| + 1e-6 accepts the quarter-K mutants at (96, 96, 520).
"""
import numpy as np
import pytest

from tests import gemm_numpy as gn
from tests.kit import F32, F64

IDS = [gn.case_id(k) for k in gn.CASE_KEYS]


def test_entry_table_covers_every_entry_row_of_the_layout_file():
    from tests.gemm_cases import CASES, ENTRY_NAMES
    assert list(gn.ENTRIES) == ENTRY_NAMES and len(ENTRY_NAMES) == 26
    assert sorted({(k[0], k[1]) for k in gn.CASE_KEYS}) == sorted(CASES)
    assert {s for _, _, s, _ in gn.CASE_KEYS} == set(gn.SHAPES)
    for a, b in gn.TWINS + gn.FLAGGED_TWINS:
        assert a in gn.ENTRIES and b in gn.ENTRIES


def test_k_ranges_of_the_cut_shapes():
    """(96, 96, 520) is cut in two by every rule, for any device with at least 2 CUs: ranges 288 and 232 wide, the second
    ending in a ragged tile; the other shapes are never cut."""
    for name, e in gn.ENTRIES.items():
        for key, shape in gn.SHAPES.items():
            for cus in (2, 8, 256, 304) if e.cut == "for" else (256,):
                s = gn.splits_of(e, shape, cus)
                if e.cut and key == "split" or e.cut and key == "fastsplit" and cus >= 256:
                    assert s == 2 and gn.k_ranges(shape[2], s) == [(0, 288), (288, 520)], (name, key, cus)
                elif key not in ("split", "fastsplit"):
                    assert s == 1 and gn.k_ranges(shape[2], s) == [(0, shape[2])], (name, key, cus)
    assert gn.k_per_split(288) == 288 and gn.k_per_split(300) == 320 and gn.k_per_split(41) == 64
    assert [gn.quarter_k(k) for k in (41, 70, 256, 288, 300, 520, 700)] == [41, 70, 64, 64, 64, 128, 160]


@pytest.mark.parametrize("key", gn.CASE_KEYS, ids=IDS)
def test_fp64_reference_of_a_dyadic_case_is_the_integer_result(key):
    c = gn.case(key, dyadic=True)
    M, N, K = c.shape
    ia = np.rint(c._mk(c.A).astype(F64) * 8).astype(np.int64)
    ib = np.rint(c._kn(c.B).astype(F64) * 8).astype(np.int64)
    want = ia @ ib                                     # in 1/64
    if c.var.get("zd"):
        np.fill_diagonal(want, 0)
    if c.bias is not None:
        want = want + np.rint(c.bias.astype(F64) * 64).astype(np.int64)
    if c.C0 is not None:
        want = want + np.rint(c.C0.astype(F64) * 64).astype(np.int64)
    assert np.array_equal(c.ref["C"] * 64, want.astype(F64))
    if c.var.get("colstat"):
        blocks = range(0, M, gn.STAT_ROWS)
        assert np.array_equal(c.ref["sum"] * 64, np.stack([want[r:r + 128].sum(0) for r in blocks]).astype(F64))
        assert np.array_equal(c.ref["sq"] * 4096, np.stack([(want[r:r + 128] ** 2).sum(0) for r in blocks]).astype(F64))
    # every plane is exact here, so both fp32 runs are the reference itself (not the square partials: multiples of
    # 1/4096 whose sums over 128 rows outgrow 24 bits)
    for r in c.runs32:
        for k in c.tensors():
            assert k == "sq" or np.array_equal(r[k].astype(F64), c.ref[k]), k


@pytest.mark.parametrize("key", gn.CASE_KEYS, ids=IDS)
def test_planes_bound_and_mutants(key, record_property):
    c = gn.case(key)
    # the planes sum back to the operand bit for bit; non-vacuity of the values
    for which in "ab":
        x = c.A if which == "a" else c.B
        p, scale = c.planes(which)
        if gn.value_kind(c.e, which) == "spike":
            assert np.array_equal(p[0] * F32(scale), x) and 0.2 <= c.spike_density(which) <= 0.4
        elif len(p) == 3:
            assert np.array_equal((p[0] + p[1]) + p[2], x) and np.array_equal(p[0], gn.bf16_trunc(x))
            assert all(np.array_equal(gn.bf16_trunc(q), q) for q in p)
            assert c.plane2_live(which) >= 0.9
        elif c.bf16 and gn.value_kind(c.e, which) == "dense":
            assert np.array_equal(gn.bf16_trunc(p[0]), p[0]) and np.abs(p[0] - x).max() > 0
        else:
            assert np.array_equal(p[0], x)
    # the rule's plumbing: both fp32 runs lie within a quarter of the bound
    for r in c.runs32:
        for k, f in gn.fraction_of_bound(c, {k: r[k] for k in c.tensors()}).items():
            assert c.bound[k] > 0 and f <= 0.25 + 1e-12, (k, f)
    # every mutant leaves the bound at least 2 x behind
    muts = gn.mutants(c)
    for name, got in muts.items():
        for k, f in gn.fraction_of_bound(c, got).items():
            record_property(f"{name} [{k}]", round(f, 2))
            assert f >= 2.0, f"{c.id}: mutant '{name}' is only {f:.2f} x the bound of {k}"
    # the mutants that must apply, do
    names = set(muts)
    pa, pb, terms, _ = c.model()
    if len(terms) == 6:
        assert sum("quarter" in n for n in names) == 3 and sum("row tile" in n for n in names) == 3
    if len(terms) == 3:
        assert "plane 2 of the dense operand lost on a quarter of K" in names
    if c.shape_key in ("split", "fastsplit"):
        assert "a K range's slab left out of the last 32 columns" in names
    if c.prec == 1:
        assert ("bf16 mode truncates instead of rounding" in names) == \
            ("dense" in (gn.value_kind(c.e, "a"), gn.value_kind(c.e, "b")))
    if c.var.get("colstat"):
        assert "square partials before the bias" in names


@pytest.mark.parametrize("name", ["gemm6_tn", "gemm_auto_tn_f0"])
def test_the_fixed_bound_accepts_the_quarter_k_mutants_at_96_96_520(name, record_property):
    """Why tests/test_gemm_planes_gpu.py exists: a second-order term lost on k < 128 of K = 520 stays inside
    2e-6 * sum|a||b| + 1e-6 everywhere (0.7 - 0.8 of it), and 3 - 5 x outside the restated bound."""
    c = gn.Case(name, 0, "split", dict(zd=1))
    old = c.old_bound()
    muts = {n: m for n, m in gn.mutants(c).items() if "quarter" in n}
    assert len(muts) == 3
    for n, got in muts.items():
        f_old = float((np.abs(got["C"].astype(F64) - c.ref["C"]) / old).max())
        f_new = gn.fraction_of_bound(c, got)["C"]
        record_property(n, (round(f_old, 2), round(f_new, 2)))
        assert f_old <= 1.0, (n, f_old)
        assert f_new >= 2.0, (n, f_new)
