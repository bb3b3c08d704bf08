"""
Shared cases of the GEMM tests: the table of entry points of the C ABI with the call of each, the (entry, precision)
cases, and the strided / offset operand layouts of tests/test_gemm_layouts_gpu.py.  Importing this touches no GPU: the
library is looked up when _entries() is called.
"""
import types

import torch

from tests.guarded import embed
from tests.kit import DEV
from tests.kit import ptr as P

C_SPK = 1.25
BASE = ("w", "o0")
ALL = ("r8+8", "oa")


def _lib():
    from sparch_amd._capi import lib
    return lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def ld_of(rule, w):
    return {"w": w, "w+1": w + 1, "r4+4": (w + 3) // 4 * 4 + 4, "r8+8": (w + 7) // 8 * 8 + 8, "TH": 3 * w}[rule]


def off_of(rule, t):
    return {"o0": 0, "o1": 1, "oa": 16 // t.element_size()}[rule]


def place(t, lay):
    """t on the device, embedded with the layout (ld rule, offset rule)."""
    return embed(t.to(DEV), ld_of(lay[0], t.shape[1]), off_of(lay[1], t))


# ---------------------------------------------------------------------------------------------- entry points
# form: which product; a / b: what the operand is —
#   f32 dense fp32 | spk spikes as fp32 (0 or c) | s16 spikes as a bf16 0/1 plane | f32p dense fp32 AND its 3 planes |
#   ex dense fp32 that the flag speaks about | ex16 the same AND its upper-half plane
# ws: the query that sizes the workspace (None: the entry takes none)
def _entries():
    L = _lib()
    st = _stream
    tnq = lambda x: L.sparch_gemm_spike_tn_workspace_bytes(x.M, x.N, x.K, x.prec)                       # noqa: E731
    E = {}

    def add(name, form, a, b, call, prec=True, ws=None, **kw):
        E[name] = types.SimpleNamespace(name=name, form=form, a=a, b=b, call=call, prec=prec, ws=ws, **kw)

    add("gemm_nt", "nt", "f32", "f32", prec=False, call=lambda x: L.sparch_gemm_nt(
        x.M, x.N, x.K, P(x.A), x.lda, P(x.B), x.ldb, P(x.C), x.ldc, P(x.bias), P(x.colstat), st()))
    add("gemm_nn", "nn", "f32", "f32", prec=False, call=lambda x: L.sparch_gemm_nn(
        x.M, x.N, x.K, P(x.A), x.lda, P(x.B), x.ldb, P(x.C), x.ldc, st()))
    add("gemm_tn", "tn", "f32", "f32", prec=False, ws=lambda x: L.sparch_gemm_tn_workspace_bytes(x.M, x.N, x.K),
        call=lambda x: L.sparch_gemm_tn(x.M, x.N, x.K, P(x.A), x.lda, P(x.B), x.ldb, P(x.C), x.ldc, x.zd, x.acc,
                                        P(x.ws), x.ws_bytes, st()))
    add("gemm6_nt", "nt", "f32", "f32", call=lambda x: L.sparch_gemm6_nt(
        x.M, x.N, x.K, P(x.A), x.lda, P(x.B), x.ldb, P(x.C), x.ldc, P(x.bias), P(x.colstat), st(), x.prec))
    add("gemm6_nn", "nn", "f32", "f32", call=lambda x: L.sparch_gemm6_nn(
        x.M, x.N, x.K, P(x.A), x.lda, P(x.B), x.ldb, P(x.C), x.ldc, st(), x.prec))
    add("gemm6_tn", "tn", "f32", "f32", ws=tnq, call=lambda x: L.sparch_gemm6_tn(
        x.M, x.N, x.K, P(x.A), x.lda, P(x.B), x.ldb, P(x.C), x.ldc, x.zd, x.acc, P(x.ws), x.ws_bytes, st(), x.prec))
    skq = lambda x: L.sparch_gemm6_splitk_workspace_bytes(x.M, x.N, x.K, x.prec)                        # noqa: E731
    add("gemm6_nt_splitk", "nt", "f32", "f32", ws=skq, plain=True, call=lambda x: L.sparch_gemm6_nt_splitk(
        x.M, x.N, x.K, P(x.A), x.lda, P(x.B), x.ldb, P(x.C), x.ldc, P(x.ws), x.ws_bytes, st(), x.prec))
    add("gemm6_nn_splitk", "nn", "f32", "f32", ws=skq, plain=True, call=lambda x: L.sparch_gemm6_nn_splitk(
        x.M, x.N, x.K, P(x.A), x.lda, P(x.B), x.ldb, P(x.C), x.ldc, P(x.ws), x.ws_bytes, st(), x.prec))
    add("gemm_spike_nt", "nt", "spk", "f32", call=lambda x: L.sparch_gemm_spike_nt(
        x.M, x.N, x.K, P(x.A), x.lda, C_SPK, P(x.B), x.ldb, P(x.C), x.ldc, P(x.bias), P(x.colstat), st(), x.prec))
    for side in (0, 1):
        add(f"gemm_spike_tn_s{side}", "tn", "spk" if side == 0 else "f32", "spk" if side == 1 else "f32", ws=tnq,
            call=lambda x, side=side: L.sparch_gemm_spike_tn(
                x.M, x.N, x.K, P(x.A), x.lda, P(x.B), x.ldb, side, C_SPK, P(x.C), x.ldc, x.zd, x.acc, P(x.ws),
                x.ws_bytes, st(), x.prec))
        add(f"gemm_spike16_tn_s{side}", "tn", "s16" if side == 0 else "f32", "s16" if side == 1 else "f32", ws=tnq,
            call=lambda x, side=side: L.sparch_gemm_spike16_tn(
                x.M, x.N, x.K, P(x.A16 if side == 0 else x.A), x.lda, P(x.B16 if side == 1 else x.B), x.ldb, side,
                C_SPK, P(x.C), x.ldc, x.zd, x.acc, P(x.ws), x.ws_bytes, st(), x.prec))
    add("gemm_spike16_nt", "nt", "s16", "f32", call=lambda x: L.sparch_gemm_spike16_nt(
        x.M, x.N, x.K, P(x.A16), x.lda, C_SPK, P(x.B), x.ldb, P(x.C), x.ldc, P(x.bias), P(x.colstat), st(), x.prec))
    add("gemm_spike16_nt_wp", "nt", "s16", "f32p", call=lambda x: L.sparch_gemm_spike16_nt_wp(
        x.M, x.N, x.K, P(x.A16), x.lda, C_SPK, P(x.B), P(x.Bp), x.ldb, P(x.C), x.ldc, P(x.bias), P(x.colstat), st(),
        x.prec))
    add("gemm6_nn_wp", "nn", "f32", "f32p", call=lambda x: L.sparch_gemm6_nn_wp(
        x.M, x.N, x.K, P(x.A), x.lda, P(x.B), P(x.Bp), x.ldb, P(x.C), x.ldc, st(), x.prec))
    add("gemm6_nn_pp", "nn", "f32p", "f32p", call=lambda x: L.sparch_gemm6_nn_pp(
        x.M, x.N, x.K, P(x.A), P(x.Ap), x.lda, P(x.B), P(x.Bp), x.ldb, P(x.C), x.ldc, st(), x.prec))
    add("gemm_spike16_tn_ap", "tn", "f32p", "s16", ws=tnq, call=lambda x: L.sparch_gemm_spike16_tn_ap(
        x.M, x.N, x.K, P(x.A), P(x.Ap), x.lda, P(x.B16), x.ldb, C_SPK, P(x.C), x.ldc, x.zd, x.acc, P(x.ws),
        x.ws_bytes, st(), x.prec))
    for f in (0, 1):
        add(f"gemm_auto_nt_f{f}", "nt", "ex", "f32", flag=f, call=lambda x: L.sparch_gemm_auto_nt(
            x.M, x.N, x.K, P(x.A), x.lda, P(x.B), x.ldb, P(x.C), x.ldc, P(x.bias), P(x.colstat), P(x.flag), st(),
            x.prec))
        add(f"gemm_auto_tn_f{f}", "tn", "f32", "ex", flag=f, ws=tnq, call=lambda x: L.sparch_gemm_auto_tn(
            x.M, x.N, x.K, P(x.A), x.lda, P(x.B), x.ldb, P(x.C), x.ldc, x.zd, x.acc, P(x.flag), P(x.ws), x.ws_bytes,
            st(), x.prec))
        add(f"gemm_auto16_nt_f{f}", "nt", "ex16", "f32", flag=f, call=lambda x: L.sparch_gemm_auto16_nt(
            x.M, x.N, x.K, P(x.A), x.lda, P(x.A16), x.lda16, P(x.B), x.ldb, P(x.C), x.ldc, P(x.bias), P(x.colstat),
            P(x.flag), st(), x.prec))
        add(f"gemm_auto16_tn_f{f}", "tn", "f32", "ex16", flag=f,   # (slabs at the plane's padded width)
            ws=lambda x: L.sparch_gemm_spike_tn_workspace_bytes(x.M, (x.N + 7) // 8 * 8, x.K, x.prec),
            call=lambda x: L.sparch_gemm_auto16_tn(
                x.M, x.N, x.K, P(x.A), x.lda, P(x.B), x.ldb, P(x.B16), x.ldb16, P(x.C), x.ldc, x.zd, x.acc, P(x.flag),
                P(x.ws), x.ws_bytes, st(), x.prec))
    return E


ENTRY_NAMES = ["gemm_nt", "gemm_nn", "gemm_tn", "gemm6_nt", "gemm6_nn", "gemm6_tn", "gemm6_nt_splitk",
               "gemm6_nn_splitk", "gemm_spike_nt", "gemm_spike_tn_s0", "gemm_spike_tn_s1", "gemm_spike16_nt",
               "gemm_spike16_tn_s0", "gemm_spike16_tn_s1", "gemm_spike16_nt_wp", "gemm6_nn_wp", "gemm6_nn_pp",
               "gemm_spike16_tn_ap", "gemm_auto_nt_f0", "gemm_auto_nt_f1", "gemm_auto_tn_f0", "gemm_auto_tn_f1",
               "gemm_auto16_nt_f0", "gemm_auto16_nt_f1", "gemm_auto16_tn_f0", "gemm_auto16_tn_f1"]
NO_PREC = {"gemm_nt", "gemm_nn", "gemm_tn"}
CASES = [(n, p) for n in ENTRY_NAMES for p in ((0,) if n in NO_PREC else (0, 1))]
