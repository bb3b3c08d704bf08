"""
tests/guarded.py on the CPU: planted numpy "kernels" with the defects the GPU tests are there to catch must be caught,
and a correct one must pass.  The kernels work the way the HIP ones do — on a base pointer (a flat array plus an element
offset) and a leading dimension — so that they CAN leave their operand.
"""
import types

import numpy as np
import pytest
import torch

from tests import guarded
from tests.guarded import GuardError, embed, guard_arena


def _mem(view):
    """(flat numpy array over the view's parent, element offset of the view's first element): a 'pointer'."""
    return view.parent.numpy(), view.start


def np_gemm_nt(M, N, K, A, lda, B, ldb, C, ldc, *, k_round4=False, prefetch_row_m=False, store_col_n=False):
    """C[M,N] = A[M,K] B[N,K]^T on 'pointers'.  The keyword switches plant one defect each:
    k_round4: the K loop runs to K rounded up to 4 (a vector load that ignores the tail);
    prefetch_row_m: row M of A is loaded and multiplied by a zero mask (harmless in exact arithmetic on finite data);
    store_col_n: the epilogue stores one column too many."""
    (a, a0), (b, b0), (c, c0) = A, B, C
    kk = (K + 3) // 4 * 4 if k_round4 else K
    for m in range(M):
        for n in range(N + (1 if store_col_n else 0)):
            acc = np.float64(0)
            for k in range(kk):
                acc += np.float64(a[a0 + m * lda + k]) * np.float64(b[b0 + min(n, N - 1) * ldb + k])
            if prefetch_row_m:
                acc += np.float64(0) * np.float64(a[a0 + M * lda])
            c[c0 + m * ldc + n] = acc


def np_spike_count(M, K, S, lds_, out, *, k_round8=False):
    """out[m] = number of spikes (x != 0) in row m of a 16-bit plane; k_round8 plants a 16-byte load past the tail."""
    s, s0 = S
    kk = (K + 7) // 8 * 8 if k_round8 else K
    for m in range(M):
        out[m] = sum(1 for k in range(kk) if s[s0 + m * lds_ + k] != 0)


def _case(lda, ldb, ldc, M=5, N=3, K=41, offset=0):
    g = torch.Generator().manual_seed(1)
    A = torch.randint(-8, 9, (M, K), generator=g).float() / 8
    B = torch.randint(-8, 9, (N, K), generator=g).float() / 8
    eA, eB = embed(A, lda, offset), embed(B, ldb, offset)
    eC = embed(torch.full((M, N), float("nan")), ldc, offset)
    return A, B, eA, eB, eC


def _outcome(eA, eB, eC, ref):
    """'ok', or what the harness noticed."""
    for e, what in ((eA, "A"), (eB, "B"), (eC, "C")):
        try:
            e.check(what)
        except GuardError as err:
            return f"guard: {err}"
    if bool(torch.isnan(eC).any()):
        return "nan in the result"
    if not torch.equal(eC.double(), ref):
        return "wrong result"
    return "ok"


@pytest.mark.parametrize("lda,ldb,ldc,offset", [(41, 41, 3, 0), (44, 44, 4, 0), (42, 48, 12, 1), (3 * 41, 44, 8, 4)])
def test_a_correct_kernel_passes(lda, ldb, ldc, offset):
    A, B, eA, eB, eC = _case(lda, ldb, ldc, offset=offset)
    np_gemm_nt(5, 3, 41, _mem(eA), lda, _mem(eB), ldb, _mem(eC), ldc)
    assert _outcome(eA, eB, eC, A.double() @ B.double().T) == "ok"
    assert eC.stride(0) == ldc and eA.stride(0) == lda
    assert (eA.start - offset) * 4 % 256 == 0


def test_a_k_loop_rounded_up_to_four_is_caught():
    """K = 41 in rows of 44: a 16-byte load that is legal (ld % 4 == 0) but must stop at the tail."""
    A, B, eA, eB, eC = _case(44, 44, 3)
    np_gemm_nt(5, 3, 41, _mem(eA), 44, _mem(eB), 44, _mem(eC), 3, k_round4=True)
    assert _outcome(eA, eB, eC, A.double() @ B.double().T) == "nan in the result"


def test_a_read_of_row_m_is_caught_even_when_it_is_masked():
    A, B, eA, eB, eC = _case(41, 41, 3)
    np_gemm_nt(5, 3, 41, _mem(eA), 41, _mem(eB), 41, _mem(eC), 3, prefetch_row_m=True)
    assert _outcome(eA, eB, eC, A.double() @ B.double().T) == "nan in the result"


def test_a_store_to_column_n_of_a_strided_c_is_caught():
    A, B, eA, eB, eC = _case(41, 41, 8)
    np_gemm_nt(5, 3, 41, _mem(eA), 41, _mem(eB), 41, _mem(eC), 8, store_col_n=True)
    out = _outcome(eA, eB, eC, A.double() @ B.double().T)
    assert out.startswith("guard: C") and "row 0, column 3" in out, out
    assert not eC.fill_intact() and eA.fill_intact()


def test_a_plane_load_past_the_tail_counts_the_fill_as_spikes():
    g = torch.Generator().manual_seed(2)
    S = (torch.rand(6, 41, generator=g) < 0.3).to(torch.bfloat16)
    eS = embed(S, 48)
    assert int(guarded._bits(eS.parent)[0]) == guarded.FILL16
    want = (S != 0).sum(1).numpy()
    mem = (guarded._bits(eS.parent).numpy(), eS.start)
    out = np.zeros(6, np.int64)
    np_spike_count(6, 41, mem, 48, out)
    assert np.array_equal(out, want)
    np_spike_count(6, 41, mem, 48, out, k_round8=True)
    assert np.array_equal(out, want + 7)
    eS.check()


def test_embed_owns_a_whole_tile_around_the_view():
    e = embed(torch.zeros(3, 5), 9, offset=1)
    before, behind = e.start, e.parent.numel() - (e.start + 3 * 9)
    assert before >= 128 * 9 + 1024 and behind >= 128 * 9 + 1024
    e.parent[e.start - 128 * 9] = 1.0        # a store one whole tile of rows in front of the view
    with pytest.raises(GuardError):
        e.check()
    e2 = embed(torch.zeros(3, 5), 9)
    e2.parent[e2.start + 5] = float("nan")   # a NaN with the fill's own bits is not a change ...
    e2.check()
    guarded._bits(e2.parent)[e2.start + 5] = 0x7FC00001   # ... any other NaN is
    with pytest.raises(GuardError):
        e2.check()


def _fake_module():
    return types.SimpleNamespace(torch=torch)


def test_the_guarded_allocator_hands_out_exact_sizes():
    mod = _fake_module()
    with guard_arena(mod, nbytes=1 << 20, device="cpu") as arena:
        assert mod.torch is not torch and mod.torch.float32 is torch.float32   # everything else is delegated
        a = mod.torch.empty(7, dtype=torch.float32, device="cpu")
        b = mod.torch.empty((3, 5), dtype=torch.bfloat16, device="cpu")
        c = mod.torch.zeros(2, 3, dtype=torch.int64, device="cpu")
        d = mod.torch.empty_like(b)
        e = mod.torch.empty(0, dtype=torch.bfloat16, device="cpu")
        f = mod.torch.empty(4, dtype=torch.uint8, device="cpu", pin_memory=False)   # an option it does not know: torch's
        for t in (a, b, c, d):
            assert t.data_ptr() % 256 == 0
        assert [arena.nbytes_of(t) for t in (a, b, c, d)] == [28, 30, 48, 30]
        assert arena.nbytes_of(f) is None and e.numel() == 0
        assert bool(torch.isnan(a).all()) and bool(torch.isnan(b.float()).all()) and int(c.abs().sum()) == 0
        buf, off = arena.buf, a.data_ptr() - arena.buf.data_ptr()
        assert buf[off + 28:off + 32].view(torch.int32).item() == 0x7FC07FC0   # the fill starts right behind the slice
        a.fill_(1.0)
        b.fill_(2.0)
        d.fill_(3.0)
    assert mod.torch is torch


def test_a_store_of_eight_bytes_behind_a_workspace_is_caught():
    mod = _fake_module()
    with pytest.raises(GuardError, match=r"0 byte\(s\) behind the end of slice #1 \(torch.float32, shape \(10,\), 40 bytes\)"):
        with guard_arena(mod, nbytes=1 << 20, device="cpu") as arena:
            mod.torch.empty(3, dtype=torch.float32, device="cpu").fill_(0)
            ws = mod.torch.empty(10, dtype=torch.float32, device="cpu")
            mem = arena.buf.numpy().view(np.float32)
            at = (ws.data_ptr() - arena.buf.data_ptr()) // 4
            mem[at:at + 12] = 0.5                      # a "kernel" that believes the workspace has 12 words
    assert mod.torch is torch


def test_the_module_is_restored_when_the_body_raises():
    mod = _fake_module()
    with pytest.raises(ZeroDivisionError):
        with guard_arena(mod, nbytes=1 << 16, device="cpu"):
            1 / 0
    assert mod.torch is torch
