"""Return codes of the GEMM entry points (gemm_spike.hip, gemm.hip) for calls that are refused before anything is
launched: each probe starts from one valid argument list and breaks one thing (or two, for precedence).  Pointers are
the integer 16 (non-NULL, aligned: nothing is dereferenced before the checks), 20 (misaligned) or None.  No probe
reaches a launch, so the file needs no GPU.  Never call an entry's base list itself: for the direct products it is a
valid call (Entry refuses to).  The entries that take a workspace have it NULL in their base list and a shape that is
cut into K ranges, so their base list plus any harmless change is SPARCH_EWORKSPACE.

The contract (include/sparch_hip.h, G1): an unknown precision, then shape / NULL / leading-dimension faults, then a
spike_side outside {0, 1} are SPARCH_EINVAL; only then a missing or short workspace is SPARCH_EWORKSPACE; no matrix
product refuses for alignment."""
import re

import pytest

from tests.kit import EALIGN, EINVAL, EWORKSPACE

P, MIS = 16, 20
M, N, K = 16, 24, 40          # direct products
KC = 4096                      # the cut ones: one tile, 128 K tiles -> 16 K ranges by either split rule
SPLITS = 16
WIDTH = {"nt": dict(lda="K", ldb="K"), "nn": dict(lda="K", ldb="N"), "tn": dict(lda="M", ldb="N")}


class Entry:
    def __init__(self, name, form, sig, null_ok=(), **fixed):
        """sig: the argument names in order.  Sizes and leading dimensions get the valid values of `form`, pointers P
        (those of null_ok and the workspace None), everything else 0 unless `fixed` says otherwise."""
        self.name, self.form, self.names = name, form, sig.split()
        self.cut = "ws" in self.names
        dims = dict(M=M, N=N, K=KC if self.cut else K)
        dims.update(fixed)
        base = dict(dims, ldc=dims["N"], scale=1.0, stream=None, ws=None, ws_bytes=0,
                    **{ld: dims[d] for ld, d in WIDTH[form].items()})
        base.update(lda16=dims["K"], ldb16=dims["N"])
        self.ptrs = [n for n in self.names if n not in base and n[0].isupper() or n in ("bias", "colstat", "flag")]
        base.update({n: None if n in null_ok else P for n in self.ptrs})
        base.update(fixed)
        self.base = {n: base.get(n, 0) for n in self.names}
        # (A may be NULL where its planes are given instead)
        self.mandatory = [n for n in self.ptrs if n not in null_ok and not (n == "A" and "Ap" in self.names)]

    def __call__(self, **over):
        from sparch_amd._capi import lib
        assert over and not set(over) - set(self.names), (self.name, over)      # never the base list itself
        return getattr(lib, self.name)(*[over.get(n, self.base[n]) for n in self.names])

    def need(self):
        """Bytes of the slabs of the base shape (every split rule gives SPLITS ranges for it)."""
        return SPLITS * self.base["M"] * self.base["N"] * 4


NT_SIG = "M N K A lda scale B ldb C ldc bias colstat stream precision"
TN_SIG = "M N K A lda B ldb spike_side scale C ldc zero_diag accumulate ws ws_bytes stream precision"
D_NT = "M N K A lda B ldb C ldc bias colstat stream"
D_NN = "M N K A lda B ldb C ldc stream"
D_TN = "M N K A lda B ldb C ldc zero_diag accumulate ws ws_bytes stream"
OPT = ("bias", "colstat")

SPIKE_NT = Entry("sparch_gemm_spike_nt", "nt", NT_SIG, OPT)
SPIKE16_NT = Entry("sparch_gemm_spike16_nt", "nt", NT_SIG, OPT)
SPIKE16_NT_WP = Entry("sparch_gemm_spike16_nt_wp", "nt", NT_SIG.replace(" B ", " B Bp "), OPT + ("Bp",))
G6_NN_WP = Entry("sparch_gemm6_nn_wp", "nn", "M N K A lda B Bp ldb C ldc stream precision", ("Bp",))
G6_NN_PP = Entry("sparch_gemm6_nn_pp", "nn", "M N K A Ap lda B Bp ldb C ldc stream precision", ("Ap", "Bp"))
G6_NT = Entry("sparch_gemm6_nt", "nt", D_NT + " precision", OPT)
G6_NN = Entry("sparch_gemm6_nn", "nn", D_NN + " precision")
AUTO_NT = Entry("sparch_gemm_auto_nt", "nt", "M N K A lda B ldb C ldc bias colstat flag stream precision", OPT)
AUTO16_NT = Entry("sparch_gemm_auto16_nt", "nt",
                  "M N K A lda A16 lda16 B ldb C ldc bias colstat flag stream precision", OPT)
SPIKE_TN = Entry("sparch_gemm_spike_tn", "tn", TN_SIG)
SPIKE16_TN = Entry("sparch_gemm_spike16_tn", "tn", TN_SIG)
SPIKE16_TN_AP = Entry("sparch_gemm_spike16_tn_ap", "tn",
                      "M N K A Ap lda B ldb scale C ldc zero_diag accumulate ws ws_bytes stream precision", ("Ap",))
G6_NT_SPLITK = Entry("sparch_gemm6_nt_splitk", "nt", "M N K A lda B ldb C ldc ws ws_bytes stream precision")
G6_NN_SPLITK = Entry("sparch_gemm6_nn_splitk", "nn", "M N K A lda B ldb C ldc ws ws_bytes stream precision")
G6_TN = Entry("sparch_gemm6_tn", "tn", D_TN + " precision")
AUTO_TN = Entry("sparch_gemm_auto_tn", "tn",
                "M N K A lda B ldb C ldc zero_diag accumulate flag ws ws_bytes stream precision")
AUTO16_TN = Entry("sparch_gemm_auto16_tn", "tn",
                  "M N K A lda B ldb B16 ldb16 C ldc zero_diag accumulate flag ws ws_bytes stream precision")
F32_NT = Entry("sparch_gemm_nt", "nt", D_NT, OPT)
F32_NN = Entry("sparch_gemm_nn", "nn", D_NN)
F32_TN = Entry("sparch_gemm_tn", "tn", D_TN, accumulate=1)      # (without it one K range would be a direct product)

ALL = (SPIKE_NT, SPIKE16_NT, SPIKE16_NT_WP, G6_NN_WP, G6_NN_PP, G6_NT, G6_NN, AUTO_NT, AUTO16_NT, SPIKE_TN, SPIKE16_TN,
       SPIKE16_TN_AP, G6_NT_SPLITK, G6_NN_SPLITK, G6_TN, AUTO_TN, AUTO16_TN, F32_NT, F32_NN, F32_TN)
CUT = tuple(e for e in ALL if e.cut)
DIRECT = tuple(e for e in ALL if not e.cut)
PRECISE = tuple(e for e in ALL if "precision" in e.names)
SIDED = (SPIKE_TN, SPIKE16_TN)
PLANES = (G6_NN_PP, SPIKE16_TN_AP)          # A may be NULL when its planes are given
OTHERS = ("sparch_split3", "sparch_flag_bf16_exact", "sparch_plane_bf16_exact")      # gemm_spike.hip's other entries
ids = lambda e: e.name  # noqa: E731


def test_every_gemm_entry_is_covered():
    from sparch_amd._capi import PROTOTYPES
    gemm = {n for n in PROTOTYPES if re.fullmatch(r"sparch_gemm\w*", n) and not n.endswith("_workspace_bytes")}
    assert gemm == {e.name for e in ALL} and len(CUT) == 9 and len(DIRECT) == 11
    assert len([e for e in ALL if e not in (F32_NT, F32_NN, F32_TN)]) + len(OTHERS) == 20      # gemm_spike.hip
    for e in ALL:
        assert len(e.names) == len(PROTOTYPES[e.name][1]), e.name
    for e in CUT:                                           # the base lists are what the module docstring says
        assert e(stream=None) == EWORKSPACE, e.name


@pytest.mark.parametrize("e", ALL, ids=ids)
def test_sizes_and_leading_dimensions(e):
    for k in "MNK":
        assert e(**{k: 0}) == EINVAL and e(**{k: -1}) == EINVAL, k
    lds = [k for k in e.names if k.startswith("ld")]
    assert set(lds) >= {"lda", "ldb", "ldc"}
    for ld in lds:                                          # one below the width is refused, ...
        assert e(**{ld: e.base[ld] - 1}) == EINVAL, ld
        assert e(**{ld: 0}) == EINVAL and e(**{ld: -8}) == EINVAL, ld
    if e.cut:                                               # ... the width itself (the base list) and above are not
        for ld in lds:
            assert e(**{ld: e.base[ld] + 3}) == EWORKSPACE, ld


@pytest.mark.parametrize("e", ALL, ids=ids)
def test_null_pointers(e):
    for k in e.mandatory:
        assert e(**{k: None}) == EINVAL, k
    assert set(e.mandatory) >= {"B", "C"} and ("A" in e.mandatory) == (e not in PLANES)
    if e in PLANES:
        assert e(A=None, Ap=None) == EINVAL                 # either form of A serves; none does not
    if e.cut:                                               # the optional ones are optional
        assert e(stream=P) == EWORKSPACE
        if e in PLANES:
            assert e(A=None, Ap=P) == EWORKSPACE and e(Ap=P) == EWORKSPACE


@pytest.mark.parametrize("e", PRECISE, ids=ids)
def test_precision(e):
    for p in (-1, 2, 7):
        assert e(precision=p) == EINVAL, p
    if e.cut:
        assert e(precision=1) == EWORKSPACE
        assert e(precision=2, ws=P, ws_bytes=1 << 30) == EINVAL


@pytest.mark.parametrize("e", SIDED, ids=ids)
def test_spike_side(e):
    for s in (-1, 2, 3):
        assert e(spike_side=s) == EINVAL, s                 # ... although the workspace is missing too
        assert e(spike_side=s, ws=P, ws_bytes=1 << 30) == EINVAL
    assert e(spike_side=1) == EWORKSPACE


@pytest.mark.parametrize("precision", (0, 1))
@pytest.mark.parametrize("e", CUT, ids=ids)
def test_workspace(e, precision):
    prec = dict(precision=precision) if e in PRECISE else {}
    need, slab = e.need(), e.need() // SPLITS
    assert e(ws=None, ws_bytes=need, **prec) == EWORKSPACE
    assert e(ws=P, ws_bytes=0, **prec) == EWORKSPACE
    assert e(ws=P, ws_bytes=slab - 4, **prec) == EWORKSPACE      # one word short of one slab
    assert e(ws=P, ws_bytes=need - 4, **prec) == EWORKSPACE      # ... and of all of them
    # shape, NULL and leading-dimension faults come first
    assert e(ws=None, M=0, **prec) == EINVAL
    assert e(ws=None, C=None, **prec) == EINVAL
    assert e(ws=None, ldc=e.base["ldc"] - 1, **prec) == EINVAL
    assert e(ws=P, ws_bytes=need - 4, B=None, **prec) == EINVAL


@pytest.mark.parametrize("e", CUT, ids=ids)
def test_no_product_refuses_for_alignment(e):
    # probed where the call is refused later for another reason, so that nothing launches
    mis = {k: MIS for k in e.ptrs if k not in OPT}
    assert e(**mis) == EWORKSPACE
    assert e(**mis, ws=MIS, ws_bytes=e.need() - 4) == EWORKSPACE
    for ld in (k for k in e.names if k.startswith("ld")):   # odd leading dimensions likewise
        assert e(**{ld: e.base[ld] + 1}) == EWORKSPACE, ld


def test_split_k_workspace_matches_its_query():
    from sparch_amd._capi import lib
    for prec in (0, 1):
        assert lib.sparch_gemm6_splitk_workspace_bytes(M, N, KC, prec) == G6_NT_SPLITK.need()
        assert lib.sparch_gemm_spike_tn_workspace_bytes(M, N, KC, prec) == SPIKE_TN.need()
    assert lib.sparch_gemm_tn_workspace_bytes(M, N, KC) == F32_TN.need()


def test_ragged_plane_width_of_auto16_tn():
    e, n = AUTO16_TN, 12                                    # N8 = 16: the product and its slabs are 16 wide
    ragged = dict(N=n, ldb=n, ldc=n)
    assert e(**ragged, ldb16=16) == EWORKSPACE
    for ldb16 in (12, 15):                                  # the plane's rows must hold N8 columns
        assert e(**ragged, ldb16=ldb16) == EINVAL
        assert e(**ragged, ldb16=ldb16, ws=P, ws_bytes=1 << 30) == EINVAL
    assert e(**ragged, ldb16=16, ws=P, ws_bytes=SPLITS * M * n * 4) == EWORKSPACE      # enough for N-wide slabs only
    assert e(**ragged, ldb16=16, ws=P, ws_bytes=SPLITS * M * 16 * 4 - 4) == EWORKSPACE


def test_planes_that_do_not_apply_need_the_fp32_operand():
    # a 16-row product never takes the pipelined plane kernel; the general kernels read A itself
    assert G6_NN_PP(A=None, Ap=P, Bp=P) == EINVAL
    assert G6_NN_PP(A=None, Ap=MIS, Bp=P) == EINVAL
    for prec in (0, 1):
        assert SPIKE16_TN_AP(A=None, Ap=P, ws=P, ws_bytes=SPIKE16_TN_AP.need(), precision=prec) == EINVAL
        assert SPIKE16_TN_AP(A=None, Ap=P, ws=P, ws_bytes=SPIKE16_TN_AP.need() - 4, precision=prec) == EWORKSPACE


def test_the_other_entries_of_gemm_spike():
    from sparch_amd._capi import lib
    split3, flag, plane = lib.sparch_split3, lib.sparch_flag_bf16_exact, lib.sparch_plane_bf16_exact
    for n in (0, 4, 12):
        assert split3(n, P, P, None) == EINVAL
    assert split3(8, None, P, None) == EINVAL and split3(8, P, None, None) == EINVAL
    assert split3(8, MIS, P, None) == EALIGN and split3(8, P, MIS, None) == EALIGN
    assert split3(4, MIS, P, None) == EINVAL and split3(8, MIS, None, None) == EINVAL
    assert flag(0, P, P, None) == EINVAL and flag(8, None, P, None) == EINVAL and flag(8, P, None, None) == EINVAL
    good = dict(M=4, K=12, x=P, ldx=12, plane=P, ldp=16, flag=P, stream=None)
    bad = [dict(M=0), dict(K=0), dict(M=-1), dict(x=None), dict(plane=None), dict(flag=None), dict(ldx=11),
           dict(ldp=8), dict(ldp=12), dict(ldp=20)]
    for b in bad:
        assert plane(*{**good, **b}.values()) == EINVAL, b
        assert plane(*{**good, **b, "plane": None if "plane" in b else MIS}.values()) == EINVAL, b
    assert plane(*{**good, "plane": MIS}.values()) == EALIGN


# (M, N, K, spike_tn exact, spike_tn bf16, gemm6_splitk exact, gemm6_splitk bf16, gemm_tn) bytes, as recorded from the
# library before the split rules moved to gemm_plan.h; 256 CUs (the MI355X's, and the count taken without a device)
WORKSPACE_BYTES = [
    (1,1,31,4,4,0,0,4), (1,1,256,4,4,0,0,4), (1,1,257,4,4,0,0,4), (1,1,4096,64,64,64,64,64),
    (1,1,64000,1000,1000,1000,1000,512), (1,128,31,512,512,0,0,512), (1,128,256,512,512,0,0,512),
    (1,128,257,512,512,0,0,512), (1,128,4096,8192,8192,8192,8192,8192),
    (1,128,64000,128000,128000,128000,128000,65536), (1,129,31,516,516,0,0,516), (1,129,256,516,516,0,0,516),
    (1,129,257,516,516,0,0,516), (1,129,4096,8256,8256,8256,8256,8256), (1,129,64000,129000,129000,66048,66048,66048),
    (1,256,31,1024,1024,0,0,1024), (1,256,256,1024,1024,0,0,1024), (1,256,257,1024,1024,0,0,1024),
    (1,256,4096,16384,16384,16384,16384,16384), (1,256,64000,256000,256000,131072,131072,131072),
    (1,257,31,1028,1028,0,0,1028), (1,257,256,1028,1028,0,0,1028), (1,257,257,1028,1028,0,0,1028),
    (1,257,4096,16448,16448,16448,16448,16448), (1,257,64000,131584,131584,87380,87380,131584),
    (1,700,31,2800,2800,0,0,2800), (1,700,256,2800,2800,0,0,2800), (1,700,257,2800,2800,0,0,2800),
    (1,700,4096,44800,44800,44800,44800,44800), (1,700,64000,238000,238000,117600,117600,358400),
    (1,2048,31,8192,8192,0,0,8192), (1,2048,256,8192,8192,0,0,8192), (1,2048,257,8192,8192,0,0,8192),
    (1,2048,4096,131072,131072,131072,131072,131072), (1,2048,64000,262144,262144,131072,131072,524288),
    (127,1,31,508,508,0,0,508), (127,1,256,508,508,0,0,508), (127,1,257,508,508,0,0,508),
    (127,1,4096,8128,8128,8128,8128,8128), (127,1,64000,127000,127000,127000,127000,65024),
    (127,128,31,65024,65024,0,0,65024), (127,128,256,65024,65024,0,0,65024), (127,128,257,65024,65024,0,0,65024),
    (127,128,4096,1040384,1040384,1040384,1040384,1040384),
    (127,128,64000,16256000,16256000,16256000,16256000,8323072), (127,129,31,65532,65532,0,0,65532),
    (127,129,256,65532,65532,0,0,65532), (127,129,257,65532,65532,0,0,65532),
    (127,129,4096,1048512,1048512,1048512,1048512,1048512), (127,129,64000,16383000,16383000,8388096,8388096,8388096),
    (127,256,31,130048,130048,0,0,130048), (127,256,256,130048,130048,0,0,130048),
    (127,256,257,130048,130048,0,0,130048), (127,256,4096,2080768,2080768,2080768,2080768,2080768),
    (127,256,64000,32512000,32512000,16646144,16646144,16646144), (127,257,31,130556,130556,0,0,130556),
    (127,257,256,130556,130556,0,0,130556), (127,257,257,130556,130556,0,0,130556),
    (127,257,4096,2088896,2088896,2088896,2088896,2088896),
    (127,257,64000,16711168,16711168,11097260,11097260,16711168), (127,700,31,355600,355600,0,0,355600),
    (127,700,256,355600,355600,0,0,355600), (127,700,257,355600,355600,0,0,355600),
    (127,700,4096,5689600,5689600,5689600,5689600,5689600),
    (127,700,64000,30226000,30226000,14935200,14935200,45516800), (127,2048,31,1040384,1040384,0,0,1040384),
    (127,2048,256,1040384,1040384,0,0,1040384), (127,2048,257,1040384,1040384,0,0,1040384),
    (127,2048,4096,16646144,16646144,16646144,16646144,16646144),
    (127,2048,64000,33292288,33292288,16646144,16646144,66584576), (128,1,31,512,512,0,0,512),
    (128,1,256,512,512,0,0,512), (128,1,257,512,512,0,0,512), (128,1,4096,8192,8192,8192,8192,8192),
    (128,1,64000,128000,128000,128000,128000,65536), (128,128,31,65536,65536,0,0,65536),
    (128,128,256,65536,65536,0,0,65536), (128,128,257,65536,65536,0,0,65536),
    (128,128,4096,1048576,1048576,1048576,1048576,1048576),
    (128,128,64000,16384000,16384000,16384000,16384000,8388608), (128,129,31,66048,66048,0,0,66048),
    (128,129,256,66048,66048,0,0,66048), (128,129,257,66048,66048,0,0,66048),
    (128,129,4096,1056768,1056768,1056768,1056768,1056768), (128,129,64000,16512000,16512000,8454144,8454144,8454144),
    (128,256,31,131072,131072,0,0,131072), (128,256,256,131072,131072,0,0,131072),
    (128,256,257,131072,131072,0,0,131072), (128,256,4096,2097152,2097152,2097152,2097152,2097152),
    (128,256,64000,32768000,32768000,16777216,16777216,16777216), (128,257,31,131584,131584,0,0,131584),
    (128,257,256,131584,131584,0,0,131584), (128,257,257,131584,131584,0,0,131584),
    (128,257,4096,2105344,2105344,2105344,2105344,2105344),
    (128,257,64000,16842752,16842752,11184640,11184640,16842752), (128,700,31,358400,358400,0,0,358400),
    (128,700,256,358400,358400,0,0,358400), (128,700,257,358400,358400,0,0,358400),
    (128,700,4096,5734400,5734400,5734400,5734400,5734400),
    (128,700,64000,30464000,30464000,15052800,15052800,45875200), (128,2048,31,1048576,1048576,0,0,1048576),
    (128,2048,256,1048576,1048576,0,0,1048576), (128,2048,257,1048576,1048576,0,0,1048576),
    (128,2048,4096,16777216,16777216,16777216,16777216,16777216),
    (128,2048,64000,33554432,33554432,16777216,16777216,67108864), (129,1,31,516,516,0,0,516),
    (129,1,256,516,516,0,0,516), (129,1,257,516,516,0,0,516), (129,1,4096,8256,8256,8256,8256,8256),
    (129,1,64000,129000,129000,66048,66048,66048), (129,128,31,66048,66048,0,0,66048),
    (129,128,256,66048,66048,0,0,66048), (129,128,257,66048,66048,0,0,66048),
    (129,128,4096,1056768,1056768,1056768,1056768,1056768), (129,128,64000,16512000,16512000,8454144,8454144,8454144),
    (129,129,31,66564,66564,0,0,66564), (129,129,256,66564,66564,0,0,66564), (129,129,257,66564,66564,0,0,66564),
    (129,129,4096,1065024,1065024,1065024,1065024,1065024), (129,129,64000,16641000,16641000,4260096,4260096,8520192),
    (129,256,31,132096,132096,0,0,132096), (129,256,256,132096,132096,0,0,132096),
    (129,256,257,132096,132096,0,0,132096), (129,256,4096,2113536,2113536,2113536,2113536,2113536),
    (129,256,64000,33024000,33024000,8454144,8454144,16908288), (129,257,31,132612,132612,0,0,132612),
    (129,257,256,132612,132612,0,0,132612), (129,257,257,132612,132612,0,0,132612),
    (129,257,4096,2121792,2121792,2121792,2121792,2121792),
    (129,257,64000,16974336,16974336,5569704,5569704,16974336), (129,700,31,361200,361200,0,0,361200),
    (129,700,256,361200,361200,0,0,361200), (129,700,257,361200,361200,0,0,361200),
    (129,700,4096,5779200,5779200,5779200,5779200,5779200),
    (129,700,64000,30702000,30702000,7585200,7585200,46233600), (129,2048,31,1056768,1056768,0,0,1056768),
    (129,2048,256,1056768,1056768,0,0,1056768), (129,2048,257,1056768,1056768,0,0,1056768),
    (129,2048,4096,16908288,16908288,8454144,8454144,16908288),
    (129,2048,64000,33816576,33816576,8454144,8454144,33816576), (256,1,31,1024,1024,0,0,1024),
    (256,1,256,1024,1024,0,0,1024), (256,1,257,1024,1024,0,0,1024), (256,1,4096,16384,16384,16384,16384,16384),
    (256,1,64000,256000,256000,131072,131072,131072), (256,128,31,131072,131072,0,0,131072),
    (256,128,256,131072,131072,0,0,131072), (256,128,257,131072,131072,0,0,131072),
    (256,128,4096,2097152,2097152,2097152,2097152,2097152),
    (256,128,64000,32768000,32768000,16777216,16777216,16777216), (256,129,31,132096,132096,0,0,132096),
    (256,129,256,132096,132096,0,0,132096), (256,129,257,132096,132096,0,0,132096),
    (256,129,4096,2113536,2113536,2113536,2113536,2113536),
    (256,129,64000,33024000,33024000,8454144,8454144,16908288), (256,256,31,262144,262144,0,0,262144),
    (256,256,256,262144,262144,0,0,262144), (256,256,257,262144,262144,0,0,262144),
    (256,256,4096,4194304,4194304,4194304,4194304,4194304),
    (256,256,64000,65536000,65536000,16777216,16777216,33554432), (256,257,31,263168,263168,0,0,263168),
    (256,257,256,263168,263168,0,0,263168), (256,257,257,263168,263168,0,0,263168),
    (256,257,4096,4210688,4210688,4210688,4210688,4210688),
    (256,257,64000,33685504,33685504,11053056,11053056,33685504), (256,700,31,716800,716800,0,0,716800),
    (256,700,256,716800,716800,0,0,716800), (256,700,257,716800,716800,0,0,716800),
    (256,700,4096,11468800,11468800,11468800,11468800,11468800),
    (256,700,64000,60928000,60928000,15052800,15052800,91750400), (256,2048,31,2097152,2097152,0,0,2097152),
    (256,2048,256,2097152,2097152,0,0,2097152), (256,2048,257,2097152,2097152,0,0,2097152),
    (256,2048,4096,33554432,33554432,16777216,16777216,33554432),
    (256,2048,64000,67108864,67108864,16777216,16777216,67108864), (257,1,31,1028,1028,0,0,1028),
    (257,1,256,1028,1028,0,0,1028), (257,1,257,1028,1028,0,0,1028), (257,1,4096,16448,16448,16448,16448,16448),
    (257,1,64000,131584,131584,87380,87380,131584), (257,128,31,131584,131584,0,0,131584),
    (257,128,256,131584,131584,0,0,131584), (257,128,257,131584,131584,0,0,131584),
    (257,128,4096,2105344,2105344,2105344,2105344,2105344),
    (257,128,64000,16842752,16842752,11184640,11184640,16842752), (257,129,31,132612,132612,0,0,132612),
    (257,129,256,132612,132612,0,0,132612), (257,129,257,132612,132612,0,0,132612),
    (257,129,4096,2121792,2121792,2121792,2121792,2121792),
    (257,129,64000,16974336,16974336,5569704,5569704,16974336), (257,256,31,263168,263168,0,0,263168),
    (257,256,256,263168,263168,0,0,263168), (257,256,257,263168,263168,0,0,263168),
    (257,256,4096,4210688,4210688,4210688,4210688,4210688),
    (257,256,64000,33685504,33685504,11053056,11053056,33685504), (257,257,31,264196,264196,0,0,264196),
    (257,257,256,264196,264196,0,0,264196), (257,257,257,264196,264196,0,0,264196),
    (257,257,4096,4227136,4227136,4227136,4227136,4227136),
    (257,257,64000,16908544,16908544,7397488,7397488,33817088), (257,700,31,719600,719600,0,0,719600),
    (257,700,256,719600,719600,0,0,719600), (257,700,257,719600,719600,0,0,719600),
    (257,700,4096,11513600,11513600,10074400,10074400,11513600),
    (257,700,64000,30223200,30223200,10074400,10074400,46054400), (257,2048,31,2105344,2105344,0,0,2105344),
    (257,2048,256,2105344,2105344,0,0,2105344), (257,2048,257,2105344,2105344,0,0,2105344),
    (257,2048,4096,33685504,33685504,10526720,10526720,33685504),
    (257,2048,64000,33685504,33685504,10526720,10526720,67371008), (700,1,31,2800,2800,0,0,2800),
    (700,1,256,2800,2800,0,0,2800), (700,1,257,2800,2800,0,0,2800), (700,1,4096,44800,44800,44800,44800,44800),
    (700,1,64000,238000,238000,117600,117600,358400), (700,128,31,358400,358400,0,0,358400),
    (700,128,256,358400,358400,0,0,358400), (700,128,257,358400,358400,0,0,358400),
    (700,128,4096,5734400,5734400,5734400,5734400,5734400),
    (700,128,64000,30464000,30464000,15052800,15052800,45875200), (700,129,31,361200,361200,0,0,361200),
    (700,129,256,361200,361200,0,0,361200), (700,129,257,361200,361200,0,0,361200),
    (700,129,4096,5779200,5779200,5779200,5779200,5779200),
    (700,129,64000,30702000,30702000,7585200,7585200,46233600), (700,256,31,716800,716800,0,0,716800),
    (700,256,256,716800,716800,0,0,716800), (700,256,257,716800,716800,0,0,716800),
    (700,256,4096,11468800,11468800,11468800,11468800,11468800),
    (700,256,64000,60928000,60928000,15052800,15052800,91750400), (700,257,31,719600,719600,0,0,719600),
    (700,257,256,719600,719600,0,0,719600), (700,257,257,719600,719600,0,0,719600),
    (700,257,4096,11513600,11513600,10074400,10074400,11513600),
    (700,257,64000,30223200,30223200,10074400,10074400,46054400), (700,700,31,1960000,1960000,0,0,1960000),
    (700,700,256,1960000,1960000,0,0,1960000), (700,700,257,1960000,1960000,0,0,1960000),
    (700,700,4096,31360000,31360000,13720000,13720000,31360000),
    (700,700,64000,54880000,54880000,13720000,13720000,62720000), (700,2048,31,5734400,5734400,0,0,5734400),
    (700,2048,256,5734400,5734400,0,0,5734400), (700,2048,257,5734400,5734400,0,0,5734400),
    (700,2048,4096,57344000,57344000,11468800,11468800,91750400),
    (700,2048,64000,57344000,57344000,11468800,11468800,91750400), (1024,1,31,4096,4096,0,0,4096),
    (1024,1,256,4096,4096,0,0,4096), (1024,1,257,4096,4096,0,0,4096), (1024,1,4096,65536,65536,65536,65536,65536),
    (1024,1,64000,262144,262144,131072,131072,524288), (1024,128,31,524288,524288,0,0,524288),
    (1024,128,256,524288,524288,0,0,524288), (1024,128,257,524288,524288,0,0,524288),
    (1024,128,4096,8388608,8388608,8388608,8388608,8388608),
    (1024,128,64000,33554432,33554432,16777216,16777216,67108864), (1024,129,31,528384,528384,0,0,528384),
    (1024,129,256,528384,528384,0,0,528384), (1024,129,257,528384,528384,0,0,528384),
    (1024,129,4096,8454144,8454144,8454144,8454144,8454144),
    (1024,129,64000,33816576,33816576,8454144,8454144,33816576), (1024,256,31,1048576,1048576,0,0,1048576),
    (1024,256,256,1048576,1048576,0,0,1048576), (1024,256,257,1048576,1048576,0,0,1048576),
    (1024,256,4096,16777216,16777216,16777216,16777216,16777216),
    (1024,256,64000,67108864,67108864,16777216,16777216,67108864), (1024,257,31,1052672,1052672,0,0,1052672),
    (1024,257,256,1052672,1052672,0,0,1052672), (1024,257,257,1052672,1052672,0,0,1052672),
    (1024,257,4096,16842752,16842752,10526720,10526720,16842752),
    (1024,257,64000,33685504,33685504,10526720,10526720,67371008), (1024,700,31,2867200,2867200,0,0,2867200),
    (1024,700,256,2867200,2867200,0,0,2867200), (1024,700,257,2867200,2867200,0,0,2867200),
    (1024,700,4096,45875200,45875200,14336000,14336000,45875200),
    (1024,700,64000,60211200,60211200,14336000,14336000,91750400), (1024,2048,31,8388608,8388608,0,0,8388608),
    (1024,2048,256,8388608,8388608,0,0,8388608), (1024,2048,257,8388608,8388608,0,0,8388608),
    (1024,2048,4096,67108864,67108864,16777216,16777216,67108864),
    (1024,2048,64000,67108864,67108864,16777216,16777216,67108864),
]


def test_workspace_byte_queries():
    from sparch_amd._capi import lib
    assert len(WORKSPACE_BYTES) >= 200
    for m, n, k, s0, s1, k0, k1, t in WORKSPACE_BYTES:
        spike, splitk = lib.sparch_gemm_spike_tn_workspace_bytes, lib.sparch_gemm6_splitk_workspace_bytes
        got = (spike(m, n, k, 0), spike(m, n, k, 1), splitk(m, n, k, 0), splitk(m, n, k, 1),
               lib.sparch_gemm_tn_workspace_bytes(m, n, k))
        assert got == (s0, s1, k0, k1, t), (m, n, k)
    for bad in ((0, 8, 8), (8, -1, 8), (8, 8, 0)):
        assert lib.sparch_gemm_spike_tn_workspace_bytes(*bad, 0) == 0 and lib.sparch_gemm_tn_workspace_bytes(*bad) == 0
        assert lib.sparch_gemm6_splitk_workspace_bytes(*bad, 1) == 0
    for prec in (-1, 2):
        assert lib.sparch_gemm_spike_tn_workspace_bytes(256, 256, 4096, prec) == 0
        assert lib.sparch_gemm6_splitk_workspace_bytes(256, 256, 4096, prec) == 0
