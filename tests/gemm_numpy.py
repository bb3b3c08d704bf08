"""
The matrix products of sparch_amd/csrc/gemm_spike.hip and gemm.hip restated in numpy: the fp64 reference, the fp32
restatements the error bound is taken from, the cases of tests/test_gemm_planes_gpu.py, and the mutants with which
tests/test_gemm_numpy_host.py shows that the bound sees a lost bf16 plane term.  No GPU and no library import.

Model of a product (what a kernel may legitimately do), C = scale * sum over terms (i, j) of a_i @ b_j, per operand:
  spike    (fp32 0 / c, or a bf16 0/1 plane)          one plane (x != 0); c goes into `scale`
  exact    (the flagged operand of *_auto*_f1)         one plane, the values themselves
  dense    fp32 mode: the three planes of the truncation split (tests/kit.split3_host)
           bf16 mode: one plane, rounded once to nearest-even
  fp32 MFMA (gemm.hip)                                 one "plane", the fp32 values
dense x dense on three planes keeps six terms, smallest first: a1 b1, a2 b0, a0 b2, a1 b0, a0 b1, a0 b0; one plane
against three keeps three.  The restatements (`plain32`, `six32`, `spike32`, `bf16_32` are this one model with one, six,
three and one term) contract in 32-wide k blocks, every block product and every addition in fp32, with the blocks
ascending and descending.  A block product of bf16 planes has exact products and is summed as numpy sums it; the fp32
MFMA's block product is the k-ordered fmaf chain that instruction is (fmaf_chain), run in the blocks' direction.  A product cut into K ranges (gemm_plan::k_per_split, restated below) forms one partial
product per range, scales it, and adds the partials up in range order; then zero_diag, then `accumulate`.  Otherwise
the bias is added to scale * acc.  Column statistics: per 128-row block the sums of C and C * C over the rows, added
one row at a time in fp32, ascending and descending.

Bound (the rule of tests/test_gated_kernels_gpu.py and tests/test_rec_cell_real_V_gpu.py): per output tensor — C, the
sum partials, the square partials — FOUR times the worst max-abs error of the two fp32 runs against fp64 on the same
inputs.  Never taken from the code under test; 4 is the project's margin for a kernel whose summation order is neither
of the two restated, and is not to be raised to make a kernel pass.
"""
import functools
import types
import zlib

import numpy as np

from tests.kit import F32, F64

KB = 32
C_SPK = 1.25
STAT_ROWS = 128
TENSORS = ("C", "sum", "sq")

SHAPES = {"sweep": (37, 35, 41), "mid": (130, 131, 70), "fast": (384, 384, 288), "ktail": (384, 384, 300),
          "stats": (256, 256, 256), "split": (96, 96, 520), "fastsplit": (384, 384, 520)}

# The 26 entry rows of tests/gemm_cases.ENTRY_NAMES: form, what A and B are (that file's vocabulary), the
# flag of the gated entries, which rule cuts the product into K ranges (None: never cut), the tile the rule counts.
_E = types.SimpleNamespace
ENTRIES = {
    "gemm_nt": _E(form="nt", a="f32", b="f32", mfma32=True),
    "gemm_nn": _E(form="nn", a="f32", b="f32", mfma32=True),
    "gemm_tn": _E(form="tn", a="f32", b="f32", mfma32=True, cut="doubling", tile=(128, 128)),
    "gemm6_nt": _E(form="nt", a="f32", b="f32"),
    "gemm6_nn": _E(form="nn", a="f32", b="f32"),
    "gemm6_tn": _E(form="tn", a="f32", b="f32", cut="for", tile=(128, 128)),
    "gemm6_nt_splitk": _E(form="nt", a="f32", b="f32", cut="for", tile=(128, 128), plain=True),
    "gemm6_nn_splitk": _E(form="nn", a="f32", b="f32", cut="for", tile=(128, 128), plain=True),
    "gemm_spike_nt": _E(form="nt", a="spk", b="f32"),
    "gemm_spike_tn_s0": _E(form="tn", a="spk", b="f32", cut="for", tile=(256, 256)),
    "gemm_spike_tn_s1": _E(form="tn", a="f32", b="spk", cut="for", tile=(256, 256)),
    "gemm_spike16_nt": _E(form="nt", a="s16", b="f32"),
    "gemm_spike16_tn_s0": _E(form="tn", a="s16", b="f32", cut="for", tile=(256, 256)),
    "gemm_spike16_tn_s1": _E(form="tn", a="f32", b="s16", cut="for", tile=(256, 256)),
    "gemm_spike16_nt_wp": _E(form="nt", a="s16", b="f32p"),
    "gemm6_nn_wp": _E(form="nn", a="f32", b="f32p"),
    "gemm6_nn_pp": _E(form="nn", a="f32p", b="f32p"),
    "gemm_spike16_tn_ap": _E(form="tn", a="f32p", b="s16", cut="for", tile=(256, 256)),
}
for _n16 in ("", "16"):
    for _form, _tile in (("nt", None), ("tn", (256, 256))):
        for _f in (0, 1):
            _x = "ex" + _n16
            ENTRIES[f"gemm_auto{_n16}_{_form}_f{_f}"] = (
                _E(form="nt", a=_x, b="f32", flag=_f) if _form == "nt" else
                _E(form="tn", a="f32", b=_x, flag=_f, cut="for", tile=_tile))
for _n, _e in ENTRIES.items():
    _e.name = _n
    for _k, _v in (("mfma32", False), ("cut", None), ("tile", None), ("plain", False), ("flag", None)):
        if not hasattr(_e, _k):
            setattr(_e, _k, _v)

# Entries that promise the same products bit for bit (first = second): fp32 spikes / the bf16 spike plane, operands
# split on the fly / pre-split, the gated entries with flag 0 / the six-term kernels.  (Flag 1 against the spike-plane
# kernels needs a plane of the flagged values at scale 1: tests/test_gemm_planes_gpu.py builds that call itself.)
TWINS = [("gemm_spike_nt", "gemm_spike16_nt"), ("gemm_spike_tn_s0", "gemm_spike16_tn_s0"),
         ("gemm_spike_tn_s1", "gemm_spike16_tn_s1"), ("gemm_spike16_nt", "gemm_spike16_nt_wp"),
         ("gemm6_nn", "gemm6_nn_wp"), ("gemm6_nn", "gemm6_nn_pp"), ("gemm_spike16_tn_s1", "gemm_spike16_tn_ap"),
         ("gemm6_nt", "gemm_auto_nt_f0"), ("gemm6_nt", "gemm_auto16_nt_f0"), ("gemm6_tn", "gemm_auto_tn_f0"),
         ("gemm6_tn", "gemm_auto16_tn_f0"), ("gemm_auto_nt_f1", "gemm_auto16_nt_f1"),
         ("gemm_auto_tn_f1", "gemm_auto16_tn_f1")]
# flag 1 against the spike-plane kernel fed the flagged operand as its plane, scale 1
FLAGGED_TWINS = [("gemm_auto_nt_f1", "gemm_spike16_nt"), ("gemm_auto_tn_f1", "gemm_spike16_tn_s1")]


# ------------------------------------------------------------------------------------------------ gemm_plan.h
def cdiv(a, b):
    return -(-a // b)


def splits_for(M, N, K, BM, BN, target_wgs, BK=KB):
    tiles, kt = cdiv(M, BM) * cdiv(N, BN), cdiv(K, BK)
    return max(1, min(target_wgs // tiles, kt // 8))


def splits_doubling(M, N, K, BM=128, BN=128, BK=KB):
    tiles, kt = cdiv(M, BM) * cdiv(N, BN), cdiv(K, BK)
    s = 1
    while tiles * s < 1024 and kt // (s * 2) >= 8:
        s *= 2
    return s


def k_per_split(K, splits=1, BK=KB):
    return cdiv(cdiv(K, splits), BK) * BK


def splits_of(e, shape, target_wgs=256, bf16=False):
    """K ranges of entry e's product (target_wgs: the device's CU count; any value >= 2 * tiles gives the same here).
    In the bf16 operand mode every pipelined kernel works on 256 x 256 tiles, and the rule counts those."""
    if e.cut is None:
        return 1
    if e.cut == "doubling":
        return splits_doubling(*shape)
    return splits_for(*shape, *((256, 256) if bf16 else e.tile), target_wgs)


def k_ranges(K, splits):
    kps = k_per_split(K, splits)
    return [(z * kps, min(K, (z + 1) * kps)) for z in range(splits) if z * kps < K]


# ------------------------------------------------------------------------------------------------ values
def _torch():
    import torch
    return torch


def bf16_round(x):
    t = _torch()
    return t.from_numpy(np.array(x, dtype=F32)).to(t.bfloat16).to(t.float32).numpy()


def bf16_trunc(x):
    return (np.ascontiguousarray(x, dtype=F32).view(np.int32) & -65536).view(F32)


def split3(x):
    """The three planes of tests/kit.split3_host as fp32 arrays (not a second split)."""
    t = _torch()
    from tests.kit import split3_host
    x = np.array(x, dtype=F32)       # (a writable copy: torch refuses read-only arrays)
    return tuple(split3_host(t.from_numpy(x)).to(t.float32).numpy().reshape((3,) + x.shape))


def value_kind(e, which):
    what = getattr(e, which)
    if what in ("spk", "s16"):
        return "spike"
    if what in ("ex", "ex16") and e.flag == 1:
        return "exact"
    return "dense"


def operand_shape(form, which, M, N, K):
    return {"nt": {"a": (M, K), "b": (N, K)}, "nn": {"a": (M, K), "b": (K, N)},
            "tn": {"a": (K, M), "b": (K, N)}}[form][which]


@functools.lru_cache(maxsize=None)
def values(tag, shape, vkind, dyadic=False):
    """One host array, read-only; the seed depends on nothing but the arguments, so twins share their operands.
    dense: standard normal (every significand bit live); spike: 30 % non-zero at c; exact: bf16-rounded normal.
    dyadic (host test only): multiples of 1/8 up to 1 — every product and partial sum exact in fp32."""
    t = _torch()
    g = t.Generator().manual_seed(zlib.crc32(f"{tag} {shape} {vkind}".encode()))
    if vkind == "spike":
        x = (t.rand(shape, generator=g) < 0.3).float() * C_SPK
    elif dyadic:
        x = t.randint(-8, 9, shape, generator=g).float() / 8
    else:
        x = t.randn(shape, generator=g)
        if vkind == "exact":
            x = x.to(t.bfloat16).float()
    x = x.numpy()
    x.setflags(write=False)
    return x


class Case:
    """One (entry, precision, shape, variant): host values, the model of the product, reference, restatements, bound."""

    def __init__(self, name, prec, shape_key, var, dyadic=False, target_wgs=256):
        self.e, self.name, self.prec, self.shape_key, self.var = ENTRIES[name], name, prec, shape_key, dict(var)
        self.shape = M, N, K = SHAPES[shape_key]
        e = self.e
        self.A = values(e.form + " a", operand_shape(e.form, "a", M, N, K), value_kind(e, "a"), dyadic)
        self.B = values(e.form + " b", operand_shape(e.form, "b", M, N, K), value_kind(e, "b"), dyadic)
        self.bias = values("bias", (N,), "dense", dyadic) if var.get("bias") else None
        self.C0 = values("C0", (M, N), "dense", dyadic) if var.get("acc") else None
        self.bf16 = bool(prec) and not e.mfma32
        self.splits = splits_of(e, self.shape, target_wgs, self.bf16)
        self.ranges = k_ranges(K, self.splits)

    @property
    def id(self):
        v = "+".join(k for k in ("bias", "colstat", "zd", "acc") if self.var.get(k)) or "plain"
        return f"{self.name}-p{self.prec}-{self.shape_key}-{v}"

    def tensors(self):
        return TENSORS if self.var.get("colstat") else TENSORS[:1]

    # -- operands as (M, K) and (K, N)
    def _mk(self, a):
        return a.T if self.e.form == "tn" else a

    def _kn(self, b):
        return b.T if self.e.form == "nt" else b

    def planes(self, which, rounding=bf16_round):
        """The planes the kernel multiplies (fp32 arrays in the operand's own layout) and the operand's scale."""
        x = self.A if which == "a" else self.B
        kind = value_kind(self.e, which)
        if kind == "spike":
            return ((x != 0).astype(F32),), C_SPK
        if kind == "exact" or self.e.mfma32:
            return (x,), 1.0
        return ((rounding(x),) if self.bf16 else split3(x)), 1.0

    def model(self, rounding=bf16_round):
        (pa, sa), (pb, sb) = self.planes("a", rounding), self.planes("b", rounding)
        pa, pb = [self._mk(p) for p in pa], [self._kn(p) for p in pb]
        if len(pa) == 3 and len(pb) == 3:
            terms = [(1, 1), (2, 0), (0, 2), (1, 0), (0, 1), (0, 0)]
        else:
            terms = [(i, j) for i in reversed(range(len(pa))) for j in reversed(range(len(pb)))]
        return pa, pb, terms, F32(sa * sb)

    # -- fp64
    def seen64(self, which, rounding=bf16_round):
        """The value the kernel multiplies, as fp64 (bf16 mode: dense operands rounded once)."""
        x = self.A if which == "a" else self.B
        if self.bf16 and value_kind(self.e, which) == "dense":
            x = rounding(x)
        return (self._mk(x) if which == "a" else self._kn(x)).astype(F64)

    def finish64(self, prod):
        """zero_diag, bias, accumulate and the statistics of an fp64 product."""
        c = prod.copy()
        if self.var.get("zd"):
            np.fill_diagonal(c, 0)
        if self.bias is not None:
            c = c + self.bias.astype(F64)
        if self.C0 is not None:
            c = c + self.C0.astype(F64)
        out = {"C": c}
        if self.var.get("colstat"):
            out["sum"], out["sq"] = col_partials(c), col_partials(c * c)
        return out

    @functools.cached_property
    def ref(self):
        return self.finish64(self.seen64("a") @ self.seen64("b"))

    # -- fp32
    def run32(self, order, sq_before_bias=False):
        """One fp32 run: k blocks of each K range in `order` ("asc" / "desc"), rows of the statistics likewise."""
        pa, pb, terms, scale = self.model()
        M, N, _ = self.shape
        total = np.zeros((M, N), F32)
        for k0, k1 in self.ranges:
            starts = list(range(k0, k1, KB))
            acc = np.zeros((M, N), F32)
            for s in (starts if order == "asc" else starts[::-1]):
                if self.e.mfma32:
                    acc = fmaf_chain(acc, pa[0][:, s:min(s + KB, k1)], pb[0][s:min(s + KB, k1)], order)
                    continue
                for i, j in terms:
                    acc = acc + pa[i][:, s:min(s + KB, k1)] @ pb[j][s:min(s + KB, k1)]
            total = total + acc * scale if self.e.cut else acc * scale
        pre = total
        if self.var.get("zd"):
            total = total.copy()
            np.fill_diagonal(total, 0)
        if self.bias is not None:
            total = total + self.bias
        if self.C0 is not None:
            total = self.C0 + total
        assert total.dtype == F32
        out = {"C": total}
        if self.var.get("colstat"):
            out["sum"] = col_partials32(total, order)
            out["sq"] = col_partials32((pre * pre) if sq_before_bias else (total * total), order)
        return out

    @functools.cached_property
    def runs32(self):
        return [self.run32("asc"), self.run32("desc")]

    @functools.cached_property
    def bound(self):
        return {k: 4.0 * max(float(np.abs(r[k].astype(F64) - self.ref[k]).max()) for r in self.runs32)
                for k in self.tensors()}

    def old_bound(self):
        """The fixed bound of tests/test_hip_parity.py and tests/test_gemm_layouts_gpu.Problem, per element of C."""
        mag = np.abs(self.seen64("a")) @ np.abs(self.seen64("b"))
        if self.bias is not None:
            mag = mag + np.abs(self.bias.astype(F64))
        if self.C0 is not None:
            mag = mag + np.abs(self.C0.astype(F64))
        return 2e-6 * mag + 1e-6

    # -- non-vacuity
    def plane2_live(self, which):
        """Fraction of a three-plane operand's elements whose third plane is non-zero (None: no third plane)."""
        p, _ = self.planes(which)
        return float((p[2] != 0).mean()) if len(p) == 3 else None

    def spike_density(self, which):
        return float((getattr(self, which.upper()) != 0).mean()) if value_kind(self.e, which) == "spike" else None


def fmaf_chain(acc, a, b, order):
    """acc + a @ b as the fp32 MFMA forms it (gemm.hip: "an exact k-ordered fmaf chain, one rounding per product"):
    one k at a time, acc = fp32(acc + a_k * b_k) with the product exact — fp64 holds the product of two fp32 values
    exactly and its sum with acc to 53 bits, so rounding that sum to fp32 is the fused operation's one rounding.  (A
    BLAS block product adds its 32 terms in a tree of vector lanes and errs less than any chain a kernel can run.)"""
    a64, b64 = a.astype(F64), b.astype(F64)
    ks = range(a.shape[1]) if order == "asc" else range(a.shape[1] - 1, -1, -1)
    for k in ks:
        acc = (acc.astype(F64) + a64[:, k, None] * b64[None, k, :]).astype(F32)
    return acc


def col_partials(c):
    """fp64: per 128-row block, the column sums of c: (blocks, N)."""
    return np.stack([c[r:r + STAT_ROWS].sum(0) for r in range(0, c.shape[0], STAT_ROWS)])


def col_partials32(c, order):
    out = []
    for r in range(0, c.shape[0], STAT_ROWS):
        rows = c[r:r + STAT_ROWS]
        s = np.zeros(c.shape[1], F32)
        for row in (rows if order == "asc" else rows[::-1]):
            s = s + row
        out.append(s)
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ cases
def variants_of(e):
    """(shape key, variant) of every case entry e runs in tests/test_gemm_planes_gpu.py."""
    bias, stats = dict(bias=True), dict(bias=True, colstat=True)
    if e.form == "nt" and not e.plain:
        return [("sweep", stats), ("mid", stats), ("fast", bias), ("ktail", {}), ("stats", stats)]
    if e.form == "tn":
        return [("sweep", dict(zd=1)), ("mid", dict(acc=1)), ("fast", dict(zd=1, acc=1)), ("ktail", {}),
                ("split", dict(zd=1)), ("split", dict(acc=1)), ("fastsplit", {})]
    return [("sweep", {}), ("mid", {}), ("fast", {}), ("ktail", {})] + ([("split", {})] if e.cut else [])


def precisions_of(e):
    return (0,) if e.mfma32 else (0, 1)


CASE_KEYS = [(n, p, s, tuple(sorted(v.items()))) for n, e in ENTRIES.items() for p in precisions_of(e)
             for s, v in variants_of(e)]


def case_id(key):
    n, p, s, v = key
    return f"{n}-p{p}-{s}-" + ("+".join(k for k, _ in v) or "plain")


@functools.lru_cache(maxsize=8)
def case(key, dyadic=False, target_wgs=256):
    n, p, s, v = key
    return Case(n, p, s, dict(v), dyadic, target_wgs)


# ------------------------------------------------------------------------------------------------ mutants (host test)
def quarter_k(K):
    """The first quarter of K in whole 32-tiles, at least 32; all of K when K < 128."""
    return K if K < 128 else max(KB, K // 4 // KB * KB)


def _lost(c, i, j, kslice, rows=slice(None)):
    """scale * a_i[rows, kslice] @ b_j[kslice] in fp64, zero outside `rows` and (zero_diag) on the diagonal."""
    pa, pb, _, scale = c.model()
    out = np.zeros(c.shape[:2], F64)
    out[rows] = float(scale) * (pa[i][rows, kslice].astype(F64) @ pb[j][kslice].astype(F64))
    if c.var.get("zd"):
        np.fill_diagonal(out, 0)
    return out


def mutants(c):
    """{name: {tensor: array}} — results of a kernel that is wrong in one named way (the ascending fp32 run with the
    fault applied), for every mutant that applies to case c."""
    pa, pb, terms, _ = c.model()
    M, N, K = c.shape
    base = c.runs32[0]
    q = slice(0, quarter_k(K))
    last_tile = slice((M - 1) // 128 * 128, M)
    out = {}

    def minus(lost):
        return {"C": (base["C"].astype(F64) - lost).astype(F32)}

    if len(terms) == 6:
        for i, j in ((0, 2), (2, 0), (1, 1)):
            out[f"a{i}b{j} lost on a quarter of K"] = minus(_lost(c, i, j, q))
            out[f"a{i}b{j} lost in the last row tile"] = minus(_lost(c, i, j, slice(None), last_tile))
    elif len(terms) == 3:
        i, j = (0, 2) if len(pb) == 3 else (2, 0)
        out["plane 2 of the dense operand lost on a quarter of K"] = minus(_lost(c, i, j, q))
    if c.splits > 1:
        k0, k1 = c.ranges[-1]
        slab = sum(_lost(c, i, j, slice(k0, k1)) for i, j in terms)
        slab[:, :max(0, N - 32)] = 0
        out["a K range's slab left out of the last 32 columns"] = minus(slab)
    if c.bf16 and "dense" in (value_kind(c.e, "a"), value_kind(c.e, "b")):
        out["bf16 mode truncates instead of rounding"] = {
            "C": c.finish64(c.seen64("a", bf16_trunc) @ c.seen64("b", bf16_trunc))["C"].astype(F32)}
    if c.var.get("colstat") and c.bias is not None:
        out["square partials before the bias"] = {"sq": c.run32("asc", sq_before_bias=True)["sq"]}
    return out


def fraction_of_bound(c, got):
    """{tensor: max|got - ref| / bound} for the tensors in got."""
    return {k: float(np.abs(np.asarray(v, F64) - c.ref[k]).max()) / c.bound[k] for k, v in got.items()}
