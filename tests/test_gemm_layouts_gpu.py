"""
The leading-dimension / alignment contract of the G1 block of include/sparch_hip.h, through the C ABI, on operands
that are NOT the packed, 256-byte-aligned tensors every other test hands the GEMMs: rows wider than the matrix,
bases 4 or 16 bytes behind an aligned address, C with padding behind column N — each operand embedded in a parent
full of NaN (tests/guarded.py), every workspace, bias, statistics buffer and flag an exact-size slice of a guard
arena.

Values, two kinds per case:
  dyadic  operands k/8 with |k| <= 8, spikes 0 or c = 1.25, dyadic bias, K <= 5000: every product is a multiple of
          1/64 and every partial sum stays below 2^24/64, and k/8 has 4 significant bits (exact in one bf16 plane) —
          so EVERY kernel, in either precision and in any summation order, must return the fp64 result bit for bit;
  real    randn operands: |err| <= 2e-6 * sum|a||b| + 1e-6 against fp64 (in bf16 mode: against fp64 products of the
          bf16-rounded dense operands, as test_bf16_operand_mode_gemms) — these catch a LOW plane addressed with
          the wrong stride, which dyadic values (all in the first plane) cannot.
Column statistics are held to test_gemm_nt_bias_and_colstats' rtol 1e-4 / atol 1e-2 in both kinds.

After every call: the three parents' fill is bit-unchanged (which includes C's row padding between N and ldc), the
result holds no NaN (nothing outside an operand was read, every element of C was written) and the arena is intact.

Coverage: (entry point) x (layout), pairwise — one operand leaves the packed layout at a time — on the SWEEP shape
(M, N, K) = (37, 35, 41): below one tile, nothing a multiple of 4.  ld rules: w+1 (no vector loads), r4+4 =
roundup4(w)+4 (16-byte rows, ragged tail: the `k + 3 < kend` branches), r8+8 = roundup8(w)+8 (the same for 16-bit
planes: `inner + 7 < inner_end`), TH = 3*w (rows of a (Bp,T,H) parent).  Offsets: o1 = 1 element (misaligned base, a
legal ld: scalar fallback), oa = 16 bytes (4 fp32 / 8 uint16).  "all" = every operand r8+8 and oa at once.
FAST = (384, 384, 288) and, with statistics, (256, 256, 256): whole tiles, K % 32 == 0, K >= 256 — the pipelined
kernels (fast_ok), with a shifted edge tile — run packed, "all", TH and with A at o1 (which sends them back to the
general kernel).  MID = (130, 131, 70): ragged multi-tile.  SPLIT = (96, 96, 5000) and (128, 700, 3000) of
test_gemm_tn_splitk_deterministic, packed and "all".

  entry point                     A: w+1 r4+4 r8+8 TH o1 oa | B: same six | C: ldc>N (4 rules) o1 oa | epilogues on ldc>N
  sparch_gemm_nt                     x    x    x   x  x  x  |      x      |          x          x  x | bias, bias+colstat
  sparch_gemm_nn                     x    x    x   x  x  x  |      x      |          x          x  x |
  sparch_gemm_tn                     x    x    x   x  x  x  |      x      |          x          x  x | zero_diag, accumulate
  sparch_gemm6_nt / _nn / _tn        x    x    x   x  x  x  |      x      |          x          x  x | as above, both precisions
  sparch_gemm6_nt_splitk / _nn_..    x    x    x   x  x  x  |      x      |          x          x  x | (SPLIT: slabs in ws)
  sparch_gemm_spike_nt / _tn s0 s1   x    x    x   x  x  x  |      x      |          x          x  x | as nt / tn
  sparch_gemm_spike16_nt / _tn s0 s1 x    x    x   x  x  x  |      x      |          x          x  x | as nt / tn
  sparch_gemm_spike16_nt_wp          x    x    x   x  x  x  | x (B and planes) |     x          x  x | bias, bias+colstat
  sparch_gemm6_nn_wp                 x    x    x   x  x  x  | x (B and planes) |     x          x  x |
  sparch_gemm6_nn_pp                 x (A and planes)       | x (B and planes) |     x          x  x |
  sparch_gemm_spike16_tn_ap          x (A and planes)       |      x      |          x          x  x | zero_diag, accumulate
  sparch_gemm_auto_nt / _tn f0 f1    x    x    x   x  x  x  |      x      |          x          x  x | as nt / tn
  sparch_gemm_auto16_nt / _tn f0 f1  x (A/B and its plane)  |      x      |          x          x  x | as nt / tn
  sparch_plane_bf16_exact         ldx: all six; ldp: r8, r8+8, 3*r8; plane at oa; misaligned plane refused
  sparch_expand_counts_u8         ldx: all six; ldp as above; counts at any byte offset; x NULL
  sparch_flag_bf16_exact          n % 4 != 0, x at o1 / oa
  sparch_split3                   x / planes at oa; misaligned refused
Every row has ld > width, an offset and (where there is a ldc) ldc > N cells; nothing is skipped.

Pinned error contract: ld < width -> SPARCH_EINVAL; a workspace one word short of one slab -> SPARCH_EWORKSPACE;
after either, C is still all fill.  NO GEMM entry point refuses a misaligned pointer or an ld that is not a multiple
of 16 bytes: each one stages that operand with scalar loads instead (the o1 / w+1 cells above are that assertion).
SPARCH_EALIGN comes only from sparch_split3 (x, planes), sparch_plane_bf16_exact and sparch_expand_counts_u8 (plane);
an ldp that is not a multiple of 8 is SPARCH_EINVAL there.
"""
import types

import numpy as np
import pytest
import torch

from tests.gemm_cases import ALL, BASE, C_SPK, CASES, _entries, _lib, _stream, off_of, place
from tests.guarded import embed, guard_arena
from tests.kit import DEV, EALIGN, EINVAL, EWORKSPACE, split3_host
from tests.kit import ptr as P

pytestmark = pytest.mark.gpu

SWEEP = (37, 35, 41)
MID = (130, 131, 70)
FAST = (384, 384, 288)
FAST_STATS = (256, 256, 256)
SPLITS = [(96, 96, 5000), (128, 700, 3000)]

LD_RULES = ["w+1", "r4+4", "r8+8", "TH"]
ONE_AT_A_TIME = [(r, "o0") for r in LD_RULES] + [("w", "o1"), ("w", "oa")]


def _rb(x):
    return x.to(torch.bfloat16).double()


def shape_of(form, which, M, N, K):
    return {"nt": {"A": (M, K), "B": (N, K)}, "nn": {"A": (M, K), "B": (K, N)}, "tn": {"A": (K, M), "B": (K, N)}}[form][which]


def variants_of(e):
    if getattr(e, "plain", False) or e.form == "nn":
        return [dict()]
    if e.form == "nt":
        return [dict(), dict(bias=True), dict(bias=True, colstat=True)]
    return [dict(), dict(zd=1), dict(acc=1), dict(zd=1, acc=1)]


class Problem:
    """Host values and fp64 reference of one (entry, shape, value kind, precision, variant)."""

    def __init__(self, e, shape, kind, prec, var, seed):
        M, N, K = shape
        g = torch.Generator().manual_seed(seed)
        self.e, self.shape, self.kind, self.prec, self.var = e, shape, kind, prec, var

        def dense(s):
            if kind == "dyadic":
                return torch.randint(-8, 9, s, generator=g).float() / 8
            return torch.randn(s, generator=g)

        def operand(what, s):
            if what in ("spk", "s16"):
                return (torch.rand(s, generator=g) < 0.3).float() * C_SPK
            x = dense(s)
            if what in ("ex", "ex16") and e.flag == 1:
                x = x.to(torch.bfloat16).float()     # the flag's promise: every element exact in bf16
            return x

        self.A = operand(e.a, shape_of(e.form, "A", M, N, K))
        self.B = operand(e.b, shape_of(e.form, "B", M, N, K))
        self.bias = dense((N,)) if var.get("bias") else None
        self.C0 = dense((M, N)) if var.get("acc") else None

        def seen(what, x):     # the value the kernel multiplies, as fp64
            exact = what in ("spk", "s16") or (what in ("ex", "ex16") and e.flag == 1)
            return x.double() if (prec == 0 or exact) else _rb(x)
        a, b = seen(e.a, self.A), seen(e.b, self.B)
        if e.form == "nt":
            b = b.T
        elif e.form == "tn":
            a = a.T
        ref, mag = a @ b, a.abs() @ b.abs()
        if var.get("zd"):
            ref.fill_diagonal_(0)
        if self.bias is not None:
            ref, mag = ref + self.bias.double(), mag + self.bias.abs().double()
        if self.C0 is not None:
            ref, mag = ref + self.C0.double(), mag + self.C0.abs().double()
        self.ref, self.bound = ref, mag * 2e-6 + 1e-6
        if kind == "dyadic":
            assert torch.equal(ref.float().double(), ref), "the fp64 reference must survive a round trip through fp32"


def run(e, pb, arena, layA=BASE, layB=BASE, layC=BASE, tag=""):
    """One call of entry e on problem pb with the three layouts; asserts the result and every guard."""
    M, N, K = pb.shape
    var = pb.var
    what = f"{e.name} prec={pb.prec} {pb.kind} {pb.shape} A={layA} B={layB} C={layC} {var} {tag}"
    x = types.SimpleNamespace(M=M, N=N, K=K, prec=pb.prec, zd=int(bool(var.get("zd"))), acc=int(bool(var.get("acc"))),
                              A=None, B=None, A16=None, B16=None, Ap=None, Bp=None, bias=None, colstat=None, ws=None,
                              ws_bytes=0, flag=None, lda16=0, ldb16=0)
    guards = []
    for side, kind_, host, lay in (("A", e.a, pb.A, layA), ("B", e.b, pb.B, layB)):
        ld = None
        if kind_ == "s16":
            t = place((host != 0).to(torch.bfloat16), lay)
            setattr(x, side + "16", t)
            ld = t.ld
        else:
            t = place(host, lay)
            setattr(x, side, t)
            ld = t.ld
            if kind_ == "f32p":       # the planes: same layout and ld, a base pointer of their own
                tp = embed(split3_host(host).to(DEV), ld, off_of(lay[1], torch.empty(0, dtype=torch.bfloat16)))
                setattr(x, side + "p", tp)
                guards.append((tp, side + " planes"))
            if kind_ == "ex16":       # upper halves, rows padded with zeros to a multiple of 8 (sparch_plane_bf16_exact)
                w8 = (host.shape[1] + 7) // 8 * 8
                up = torch.zeros(host.shape[0], w8, dtype=torch.bfloat16)
                up[:, :host.shape[1]] = (host.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
                t16 = place(up, lay)
                setattr(x, side + "16", t16)
                setattr(x, "ld" + side.lower() + "16", t16.ld)
                guards.append((t16, side + " plane"))
        setattr(x, "ld" + side.lower(), ld)
        guards.append((t, side))
    C0 = pb.C0 if pb.C0 is not None else torch.full((M, N), float("nan"))
    x.C = place(C0, layC)
    x.ldc = x.C.ld
    guards.append((x.C, "C"))
    if pb.bias is not None:
        x.bias = arena.empty(N)
        x.bias.copy_(pb.bias)
    if var.get("colstat"):
        x.colstat = arena.empty(2 * ((M + 127) // 128) * N)
    if e.ws is not None:
        x.ws_bytes = e.ws(x)
        x.ws = arena.empty(x.ws_bytes, dtype=torch.uint8) if x.ws_bytes else None
    if hasattr(e, "flag"):
        x.flag = arena.empty(1, dtype=torch.int32)
        x.flag.fill_(e.flag)
    rc = e.call(x)
    assert rc == 0, f"{what}: returned {rc}"
    torch.cuda.synchronize()
    got = x.C.cpu().double()
    for t, name in guards:
        t.check(f"{what}: {name}")
    assert not bool(torch.isnan(got).any()), f"{what}: NaN in C ({int(torch.isnan(got).sum())} elements)"
    if pb.kind == "dyadic":
        assert torch.equal(got, pb.ref), f"{what}: {int((got != pb.ref).sum())} elements differ from the exact result"
    else:
        err = (got - pb.ref).abs()
        assert bool((err <= pb.bound).all()), f"{what}: {float((err / pb.bound).max())} of the bound"
    if x.colstat is not None:
        cs = x.colstat.cpu().double().view(2, (M + 127) // 128, N)
        np.testing.assert_allclose(cs[0].sum(0).numpy(), pb.ref.sum(0).numpy(), rtol=1e-4, atol=1e-2, err_msg=what)
        np.testing.assert_allclose(cs[1].sum(0).numpy(), (pb.ref * pb.ref).sum(0).numpy(), rtol=1e-4, atol=1e-2,
                                   err_msg=what)
    arena.verify(what)


@pytest.fixture(scope="module")
def entries():
    return _entries()


@pytest.mark.parametrize("kind", ["dyadic", "real"])
@pytest.mark.parametrize("name,prec", CASES)
def test_one_operand_at_a_time_leaves_the_packed_layout(entries, name, prec, kind):
    """SWEEP shape, every ld rule and offset on A, then B, then C, the epilogue variants rotating through them; then
    every variant on a C with ldc > N, and all three operands strided and offset at once."""
    e = entries[name]
    variants = variants_of(e)
    pbs = [Problem(e, SWEEP, kind, prec, v, seed=100 + i) for i, v in enumerate(variants)]
    with guard_arena(None, nbytes=8 << 20) as arena:
        run(e, pbs[0], arena)
        i = 0
        for which in range(3):
            for lay in ONE_AT_A_TIME:
                lays = [BASE, BASE, BASE]
                lays[which] = lay
                run(e, pbs[i % len(pbs)], arena, *lays)
                i += 1
        for pb in pbs:
            run(e, pb, arena, BASE, BASE, ("r4+4", "o0"))
            run(e, pb, arena, ALL, ALL, ALL)


@pytest.mark.parametrize("kind", ["dyadic", "real"])
@pytest.mark.parametrize("name,prec", CASES)
def test_pipelined_ragged_and_split_k_shapes_on_strided_operands(entries, name, prec, kind):
    """The pipelined kernels (whole tiles, K % 32 == 0, K >= 256) on rows that are not contiguous with each other, a
    ragged multi-tile shape, and split-K shapes whose slabs live in the workspace."""
    e = entries[name]
    variants = variants_of(e)
    TH = ("TH", "o0")
    with guard_arena(None, nbytes=128 << 20) as arena:
        for i, v in enumerate(variants):
            shape = FAST_STATS if v.get("colstat") else FAST
            pb = Problem(e, shape, kind, prec, v, seed=200 + i)
            run(e, pb, arena)
            run(e, pb, arena, ALL, ALL, ALL)
            if i == 0:
                run(e, pb, arena, TH, TH, TH)
                run(e, pb, arena, ("w", "o1"), BASE, BASE, tag="(A misaligned: general kernel)")
                run(e, pb, arena, BASE, ("r8+8", "o1"), ("w", "o1"))
        pb = Problem(e, MID, kind, prec, variants[-1], seed=300)
        run(e, pb, arena)
        run(e, pb, arena, ALL, ALL, ALL)
        run(e, pb, arena, ("r4+4", "o0"), ("w+1", "oa"), ("w+1", "o1"))
        if e.ws is not None:
            for j, shape in enumerate(SPLITS):
                pb = Problem(e, shape, kind, prec, variants[-1] if j == 0 else variants[0], seed=400 + j)
                run(e, pb, arena)
                run(e, pb, arena, ALL, ALL, ALL)


@pytest.mark.parametrize("name,prec", CASES)
def test_error_codes_launch_nothing(entries, name, prec):
    """ld < width: SPARCH_EINVAL; a workspace one word short of ONE slab: SPARCH_EWORKSPACE; C stays all fill."""
    e = entries[name]
    M, N, K = shape = SPLITS[0]
    pb = Problem(e, shape, "dyadic", prec, dict(), seed=7)
    pb.C0 = None
    with guard_arena(None, nbytes=16 << 20) as arena:
        def attempt(mutate, want, what):
            real_call = e.call

            def call(x):
                mutate(x)
                rc = real_call(x)
                torch.cuda.synchronize()
                assert rc == want, f"{e.name}: {what}: returned {rc}, expected {want}"
                assert bool(torch.isnan(x.C).all()), f"{e.name}: {what}: C was written"
                raise _Refused()
            e2 = types.SimpleNamespace(**{**vars(e), "call": call})
            with pytest.raises(_Refused):
                run(e2, pb, arena)
        wa, wb = shape_of(e.form, "A", M, N, K)[1], shape_of(e.form, "B", M, N, K)[1]
        attempt(lambda x: setattr(x, "lda", wa - 1), EINVAL, "lda < width")
        attempt(lambda x: setattr(x, "ldb", wb - 1), EINVAL, "ldb < width")
        attempt(lambda x: setattr(x, "ldc", N - 1), EINVAL, "ldc < N")
        if e.a == "ex16":
            attempt(lambda x: setattr(x, "lda16", wa - 1), EINVAL, "lda16 < width")
        if e.b == "ex16":
            attempt(lambda x: setattr(x, "ldb16", wb - 1), EINVAL, "ldb16 < width")
        if e.ws is not None:
            def short(x):
                x.ws_bytes = M * N * 4 - 4
                x.acc = 1      # (sparch_gemm_tn writes a single split straight to C unless it accumulates)
                x.C.copy_(torch.full((M, N), float("nan")))
            attempt(short, EWORKSPACE, "workspace one word short of one slab")
            attempt(lambda x: (setattr(x, "ws", None), setattr(x, "acc", 1)), EWORKSPACE, "no workspace")


class _Refused(Exception):
    pass


# ---------------------------------------------------------------------------------------------- helpers of G1
def _upper(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


@pytest.mark.parametrize("exact", [True, False])
def test_plane_bf16_exact_strided_input_and_wide_plane(exact):
    L = _lib()
    M, K = 37, 41
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, 9, (M, K), generator=g).float() if exact else torch.randn(M, K, generator=g)
    k8 = (K + 7) // 8 * 8
    with guard_arena(None, nbytes=4 << 20) as arena:
        for ldx, ox in [("w", "o0")] + ONE_AT_A_TIME:
            for ldp, op in ((k8, 0), (k8 + 8, 0), (3 * k8, 8)):
                ex = place(x, (ldx, ox))
                ep = embed(torch.full((M, ldp), float("nan"), dtype=torch.bfloat16, device=DEV), ldp, op)
                flag = arena.empty(1, dtype=torch.int32)
                rc = L.sparch_plane_bf16_exact(M, K, P(ex), ex.ld, P(ep), ldp, P(flag), _stream())
                assert rc == 0, (ldx, ox, ldp, op, rc)
                torch.cuda.synchronize()
                got = ep.cpu().float()
                assert torch.equal(got[:, :K], _upper(x)) and float(got[:, K:].abs().sum()) == 0.0, (ldx, ox, ldp)
                assert int(flag.item()) == int(exact)
                ex.check("x")
                ep.check("plane")
        # refused layouts: nothing is written
        ex = place(x, BASE)
        for ldp, op, want in ((k8, 1, EALIGN), (k8 + 4, 0, EINVAL), (K - 1, 0, EINVAL)):
            ep = embed(torch.full((M, k8 + 8), float("nan"), dtype=torch.bfloat16, device=DEV), k8 + 8, op)
            flag = arena.empty(1, dtype=torch.int32)
            assert L.sparch_plane_bf16_exact(M, K, P(ex), ex.ld, P(ep), ldp, P(flag), _stream()) == want
            torch.cuda.synchronize()
            assert bool(torch.isnan(ep.float()).all()) and bool(torch.isnan(flag.view(torch.float32)).all())
            ep.check("plane")
        assert L.sparch_plane_bf16_exact(M, K, P(ex), K - 1, P(ep), k8, P(flag), _stream()) == EINVAL


def test_expand_counts_u8_strided_outputs():
    L = _lib()
    M, K = 37, 41
    g = torch.Generator().manual_seed(6)
    counts = torch.randint(0, 256, (M, K), generator=g).to(torch.uint8)
    k8 = (K + 7) // 8 * 8
    for oc in (0, 1, 3):
        ec = embed(counts.to(DEV), K, oc)
        for ldx, ox in [("w", "o0")] + ONE_AT_A_TIME + [(None, None)]:
            for ldp, op in ((k8, 0), (k8 + 8, 8)):
                ep = embed(torch.full((M, ldp), float("nan"), dtype=torch.bfloat16, device=DEV), ldp, op)
                ex = None if ldx is None else place(torch.full((M, K), float("nan")), (ldx, ox))
                rc = L.sparch_expand_counts_u8(M, K, P(ec), P(ep), ldp, P(ex), 0 if ex is None else ex.ld, _stream())
                assert rc == 0
                torch.cuda.synchronize()
                got = ep.cpu().float()
                assert torch.equal(got[:, :K], counts.float()) and float(got[:, K:].abs().sum()) == 0.0
                if ex is not None:
                    assert torch.equal(ex.cpu(), counts.float())
                    ex.check("x")
                ep.check("plane")
        ec.check("counts")
    ep = embed(torch.full((M, k8), float("nan"), dtype=torch.bfloat16, device=DEV), k8, 1)
    assert L.sparch_expand_counts_u8(M, K, P(ec), P(ep), k8, None, 0, _stream()) == EALIGN
    assert L.sparch_expand_counts_u8(M, K, P(ec), P(ep), k8 + 4, None, 0, _stream()) == EINVAL
    ex = place(torch.full((M, K), float("nan")), BASE)
    ep0 = embed(torch.full((M, k8), float("nan"), dtype=torch.bfloat16, device=DEV), k8, 0)
    assert L.sparch_expand_counts_u8(M, K, P(ec), P(ep0), k8, P(ex), K - 1, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool(torch.isnan(ep.float()).all()) and bool(torch.isnan(ep0.float()).all()) and bool(torch.isnan(ex).all())


@pytest.mark.parametrize("n,off,vector", [(1480, 0, True), (1480, 4, True), (1481, 0, False), (1483, 0, False),
                                          (1480, 1, False), (1481, 1, False), (4, 0, True), (3, 0, False)])
def test_flag_bf16_exact_ragged_and_misaligned(n, off, vector):
    """The flag is 1 iff every element is bf16-exact AND the call could use 16-byte loads (n % 4 == 0, x 16-byte
    aligned); otherwise it is 0 whatever x holds — the conservative answer: its readers then take the six-term kernel,
    which is right for any input.  Pinned as the code behaves today; one word is written."""
    L = _lib()
    g = torch.Generator().manual_seed(n)
    exact = torch.randint(0, 9, (1, n), generator=g).float()
    inexact = exact.clone()
    inexact[0, n - 1] = 1.0 + 2.0 ** -12
    with guard_arena(None, nbytes=1 << 20) as arena:
        for x, want in ((exact, 1 if vector else 0), (inexact, 0)):
            ex = embed(x.to(DEV), n, off)
            flag = arena.empty(1, dtype=torch.int32)
            assert L.sparch_flag_bf16_exact(n, P(ex), P(flag), _stream()) == 0
            torch.cuda.synchronize()
            assert int(flag.item()) == want
            ex.check("x")


def test_split3_planes_and_alignment():
    L = _lib()
    n = 8 * 37
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1, n, generator=g) * torch.exp(4 * torch.randn(1, n, generator=g))
    for ox, op in ((0, 0), (4, 8)):
        ex = embed(x.to(DEV), n, ox)
        ep = embed(torch.full((1, 3 * n), float("nan"), dtype=torch.bfloat16, device=DEV), 3 * n, op)
        assert L.sparch_split3(n, P(ex), P(ep), _stream()) == 0
        torch.cuda.synchronize()
        p = ep.cpu().float().view(3, n)
        assert torch.equal((p[0] + p[1]) + p[2], x[0]) and torch.equal(p[0], _upper(x)[0])
        assert torch.equal(ep.cpu().view(3, n), split3_host(x).view(3, n))
        ex.check("x")
        ep.check("planes")
    for ox, op, nn, want in ((1, 0, n, EALIGN), (0, 1, n, EALIGN), (0, 0, n - 4, EINVAL), (0, 0, 0, EINVAL)):
        ex = embed(x.to(DEV), n, ox)
        ep = embed(torch.full((1, 3 * n), float("nan"), dtype=torch.bfloat16, device=DEV), 3 * n, op)
        assert L.sparch_split3(nn, P(ex), P(ep), _stream()) == want
        torch.cuda.synchronize()
        assert bool(torch.isnan(ep.float()).all())
        ep.check("planes")


@pytest.mark.parametrize("dense", ["split6", "fp32"])
@pytest.mark.parametrize("kind", ["dyadic", "real"])
def test_python_call_form_of_the_t0_term_of_dV(dense, kind, monkeypatch):
    """functional.cell_backward: gemm_tn(s0[rows], dWx[rows, t, :], zero_diag=True, out=dV) — B is a (B, H) view
    of a (Bp, T, H) tensor (ldb = T*H), A a row slice, C accumulated in place; under the guarded allocator."""
    from sparch_amd import functional as Fn
    monkeypatch.setattr(Fn, "DENSE_GEMM", dense)
    Bp, Bsz, T, H = 10, 5, 3, 37
    g = torch.Generator().manual_seed(12)
    draw = (lambda *s: torch.randint(-8, 9, s, generator=g).float() / 8) if kind == "dyadic" else \
        (lambda *s: torch.randn(*s, generator=g))
    s0, dWx, dV0 = draw(Bp, H), draw(Bp, T, H), draw(H, H)
    for dd, t in ((0, 0), (1, T - 1)):
        rows = slice(dd * Bsz, (dd + 1) * Bsz)
        a, b = s0[rows].double(), dWx[rows, t, :].double()
        ref = (a.T @ b).fill_diagonal_(0) + dV0.double()
        bound = (a.abs().T @ b.abs() + dV0.abs().double()) * 2e-6 + 1e-6
        eB = embed(dWx.view(Bp, T * H).to(DEV), T * H, 0)       # the (Bp,T,H) parent, itself inside guards
        dWx_d = eB.view(Bp, T, H)
        s0_d = embed(s0.to(DEV), H, 0)
        for ldc in (H, H + 3):
            dV = embed(dV0.to(DEV), ldc, 0)
            with guard_arena(Fn, nbytes=4 << 20) as arena:
                out = Fn.gemm_tn(s0_d[rows], dWx_d[rows, t, :], zero_diag=True, out=dV)
                torch.cuda.synchronize()
                assert len(arena.allocs) == 1           # the workspace, at exactly the queried size
            assert out is dV
            got = dV.cpu().double()
            if kind == "dyadic":
                assert torch.equal(got, ref)
            else:
                assert bool(((got - ref).abs() <= bound).all())
            dV.check("dV")
            eB.check("dWx")
            s0_d.check("s0")
