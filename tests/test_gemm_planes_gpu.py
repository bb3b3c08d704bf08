"""
Every matrix product of the C ABI (the 26 entry rows of tests/gemm_cases.ENTRY_NAMES, both operand
precisions where the entry takes one) on REAL-VALUED operands, held to a bound that sees a lost bf16 plane term.

The suite's fixed bound, 2e-6 * sum|a||b| + 1e-6, is about twenty times looser than these kernels' arithmetic: a
second-order term (a0 b2, a2 b0, a1 b1) or plane 2 of a weight lost on a quarter of K passes it at K = 520
(tests/test_gemm_numpy_host.py records that).  Here the bound is, per output tensor (C, the column-sum partials, the
column-square partials), 4 x the worst max-abs error of two fp32 restatements of the same product (32-wide k blocks
ascending and descending, tests/gemm_numpy.py) against fp64 on the same inputs — the rule of
tests/test_gated_kernels_gpu.py and tests/test_rec_cell_real_V_gpu.py, never taken from the code under test.  The host
test shows that every such loss lands at least 2 x outside this bound in every case below.

Values: dense operands standard normal (every significand bit live: plane 2 non-zero in over 90 % of the elements),
spikes 30 % non-zero at c = 1.25, the flagged-exact operands (_f1) bf16-rounded normals.  Packed layouts only (strides
and offsets: tests/test_gemm_layouts_gpu.py).  Shapes (gemm_numpy.SHAPES), the smallest at which each kernel form exists:
  sweep     (37, 35, 41)     below one tile, nothing a multiple of 4: general kernels, scalar loads
  mid       (130, 131, 70)   ragged multi-tile, general kernels
  fast      (384, 384, 288)  the pipelined kernels at every tile shape, shifted edge tile, the smallest K they accept
  ktail     (384, 384, 300)  pipelined with a 12-deep last K tile; the pre-split entries fall back (K % 32 != 0)
  stats     (256, 256, 256)  NT with bias and column statistics: the pipelined statistics epilogue
  split     (96, 96, 520)    the smallest product every splitting rule cuts in two (ranges 288 and 232 wide, the second
                             ragged): TN with zero_diag and with accumulate, the _splitk NT / NN entries
  fastsplit (384, 384, 520)  TN, pipelined and cut in two at once
Bit-equal twins (gemm_numpy.TWINS): fp32 spikes / the bf16 spike plane; operands split on the fly / pre-split (_wp, _pp,
_ap); the gated entries with flag 0 / the six-term kernels, with flag 1 / the spike-plane kernels fed the flagged
operand as their plane; and a second call of every cut product.
Each case records its worst fraction of the bound (record_property "worst_fraction_of_bound"; DESIGN.md has the figures
measured on an MI355X).  Not reached: the persistent-grid walk of the pipelined kernels (more work items than CUs).
"""
import types

import numpy as np
import pytest
import torch

from tests import gemm_cases as lay
from tests import gemm_numpy as gn
from tests.guarded import embed
from tests.kit import DEV, F64, split3_host

pytestmark = pytest.mark.gpu

IDS = [gn.case_id(k) for k in gn.CASE_KEYS]


@pytest.fixture(scope="module")
def entries():
    E = lay._entries()
    assert set(E) == set(gn.ENTRIES)
    for n, e in E.items():
        s = gn.ENTRIES[n]
        assert (e.form, e.a, e.b, getattr(e, "flag", None), e.ws is not None, e.prec) == \
            (s.form, s.a, s.b, s.flag, s.cut is not None, not s.mfma32), n
    return E


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def call(e, c, plane_of_values=False):
    """One call of entry e on case c's packed operands; returns C and the statistics partials as fp64 arrays.
    plane_of_values: an "s16" operand is the operand's own (bf16-exact) values instead of its 0/1 pattern."""
    M, N, K = c.shape
    var = c.var
    x = types.SimpleNamespace(M=M, N=N, K=K, prec=c.prec, zd=int(bool(var.get("zd"))), acc=int(bool(var.get("acc"))),
                              A=None, B=None, A16=None, B16=None, Ap=None, Bp=None, bias=None, colstat=None, ws=None,
                              ws_bytes=0, flag=None, lda16=0, ldb16=0)
    guards = []
    for side, kind_, host in (("A", e.a, c.A), ("B", e.b, c.B)):
        host = torch.from_numpy(np.array(host))
        if kind_ == "s16":
            t = lay.place(host.to(torch.bfloat16) if plane_of_values else (host != 0).to(torch.bfloat16), lay.BASE)
            setattr(x, side + "16", t)
        else:
            t = lay.place(host, lay.BASE)
            setattr(x, side, t)
            if kind_ == "f32p":
                tp = embed(split3_host(host).to(DEV), t.ld, 0)
                setattr(x, side + "p", tp)
                guards.append((tp, side + " planes"))
            if kind_ == "ex16":       # upper halves, rows padded with zeros to a multiple of 8
                w8 = (host.shape[1] + 7) // 8 * 8
                up = torch.zeros(host.shape[0], w8, dtype=torch.bfloat16)
                up[:, :host.shape[1]] = (host.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
                t16 = lay.place(up, lay.BASE)
                setattr(x, side + "16", t16)
                setattr(x, "ld" + side.lower() + "16", t16.ld)
                guards.append((t16, side + " plane"))
        setattr(x, "ld" + side.lower(), t.ld)
        guards.append((t, side))
    C0 = torch.from_numpy(np.array(c.C0)) if c.C0 is not None else torch.full((M, N), float("nan"))
    x.C = lay.place(C0, lay.BASE)
    x.ldc = x.C.ld
    guards.append((x.C, "C"))
    if c.bias is not None:
        x.bias = torch.from_numpy(np.array(c.bias)).to(DEV)
    blocks = gn.cdiv(M, gn.STAT_ROWS)
    if var.get("colstat"):
        x.colstat = torch.full((2 * blocks * N,), float("nan"), device=DEV)
    if e.ws is not None:
        x.ws_bytes = e.ws(x)
        x.ws = torch.full((x.ws_bytes,), 0xFF, dtype=torch.uint8, device=DEV) if x.ws_bytes else None
    if hasattr(e, "flag"):
        x.flag = torch.full((1,), e.flag, dtype=torch.int32, device=DEV)
    rc = e.call(x)
    assert rc == 0, f"{c.id}: {e.name} returned {rc}"
    torch.cuda.synchronize()
    for t, name in guards:
        t.check(f"{c.id}: {name}")
    got = {"C": x.C.cpu().numpy().astype(F64)}
    if x.colstat is not None:
        cs = x.colstat.cpu().numpy().astype(F64).reshape(2, blocks, N)
        got["sum"], got["sq"] = cs[0], cs[1]
    for k, v in got.items():
        assert not np.isnan(v).any(), f"{c.id}: NaN in {k}"
    return got


@pytest.mark.parametrize("key", gn.CASE_KEYS, ids=IDS)
def test_product_within_the_restated_bound(entries, cus, key, record_property):
    c = gn.case(key, target_wgs=cus)
    e = entries[c.name]
    # non-vacuity, on the host values
    for which in "ab":
        live, dens = c.plane2_live(which), c.spike_density(which)
        assert live is None or live >= 0.9, (which, live)
        assert dens is None or 0.2 <= dens <= 0.4, (which, dens)
    if e.ws is not None and c.shape_key in ("split", "fastsplit"):
        assert c.splits == 2 and c.ranges == [(0, 288), (288, 520)]
    got = call(e, c)
    assert set(got) == set(c.tensors())
    fr = gn.fraction_of_bound(c, got)
    for k, f in fr.items():
        print(f"  {c.id} {k}: {f:.3f} of the bound {c.bound[k]:.3e}")
    record_property("worst_fraction_of_bound", round(max(fr.values()), 3))
    for k, f in fr.items():
        err = np.abs(got[k] - c.ref[k])
        assert f <= 1.0, (f"{c.id} {k}: {f:.3f} of the bound {c.bound[k]:.3e} (at "
                          f"{np.unravel_index(int(np.argmax(err)), err.shape)}; {int((err > c.bound[k]).sum())} of "
                          f"{err.size} elements above it)")
    if c.var.get("zd"):
        assert np.all(np.diag(got["C"]) == (np.diag(c.C0) if c.C0 is not None else 0))
    if c.splits > 1:      # a cut product: slabs reduced in fixed order, the same bits on every call
        again = call(e, c)
        assert np.array_equal(again["C"], got["C"]), f"{c.id}: a second call gave other bits"


def _twin_keys(a, b):
    """Case keys of entry a that entry b runs too (same precision, shape and variant)."""
    kb = {k[1:] for k in gn.CASE_KEYS if k[0] == b}
    return [k for k in gn.CASE_KEYS if k[0] == a and k[1:] in kb]


def _assert_same_bits(ga, gb, what):
    assert set(ga) == set(gb), what
    for k in ga:
        n = int((ga[k] != gb[k]).sum())
        assert n == 0, f"{what}: {n} of {ga[k].size} elements of {k} differ, by up to {np.abs(ga[k] - gb[k]).max():.3e}"


@pytest.mark.parametrize("a,b", gn.TWINS, ids=[f"{a}={b}" for a, b in gn.TWINS])
def test_twins_give_the_same_bits(entries, cus, a, b):
    keys = _twin_keys(a, b)
    assert len(keys) >= 8
    for key in keys:
        ca, cb = gn.case(key, target_wgs=cus), gn.case((b,) + key[1:], target_wgs=cus)
        assert np.array_equal(ca.A, cb.A) and np.array_equal(ca.B, cb.B) and ca.splits == cb.splits
        _assert_same_bits(call(entries[a], ca), call(entries[b], cb), f"{ca.id} = {b}")


@pytest.mark.parametrize("a,b", gn.FLAGGED_TWINS, ids=[f"{a}={b}" for a, b in gn.FLAGGED_TWINS])
def test_flag_1_is_the_spike_plane_kernel_on_the_flagged_operand(entries, cus, a, b, monkeypatch):
    """*_auto_*_f1 multiplies the flagged operand as ONE plane: the spike-plane entry, handed that operand's values as
    its bf16 plane at scale 1, forms the same products in the same order."""
    monkeypatch.setattr(lay, "C_SPK", 1.0)       # (the entry table's lambdas read it at call time)
    keys = _twin_keys(a, b)
    assert len(keys) >= 8
    for key in keys:
        ca = gn.case(key, target_wgs=cus)
        _assert_same_bits(call(entries[a], ca), call(entries[b], ca, plane_of_values=True), f"{ca.id} = {b} on the plane")
