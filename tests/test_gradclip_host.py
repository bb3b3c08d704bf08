"""Gradient clipping by global norm, the part that needs no GPU: the restatement of tests/clip_numpy.py against torch
(float64 CPU for the norm and the coefficient, fp32 CPU for the kernel's three-operation coefficient), every refusal of
the four C entries (sparch_grad_norm_ws_bytes, sparch_grad_norm, sparch_adam_step_clip, sparch_scale_grads: refused
before any device work, so the probes pass the integer 16 for a pointer), the workspace query, the constructor's and
the environment switch's argument checks, and that an optimizer made without max_grad_norm never reaches a new symbol."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import clip_numpy as cn
from tests.kit import EINVAL, EWORKSPACE, F32, F64

P = 16                          # a non-NULL pointer: nothing is dereferenced before the checks
U = 2.0 ** -24


def _host_table(n_tensors=9, seed=3):
    return [None if h is None else h[1] for h in cn.clip_table(n_tensors, seed=seed)]


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("case", ["clips", "does_not_clip", "all_zero"])
def test_norm_and_float64_coefficient_against_torch(case):
    grads = [g for g in _host_table() if g is not None]
    if case == "all_zero":
        grads = [np.zeros_like(g) for g in grads]
    norm = cn.norm_ref(grads)
    max_norm = {"clips": norm / 3.0, "does_not_clip": norm * 3.0, "all_zero": 1.0}[case]
    params = [torch.zeros(g.size, dtype=torch.float64, requires_grad=True) for g in grads]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g.astype(F64))
    total = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
    assert float(total) == pytest.approx(norm, rel=1e-12, abs=0.0)
    coef = cn.coef_ref(norm, max_norm)
    assert (coef < 1.0) == (case == "clips")
    if case == "all_zero":
        assert norm == 0.0 and coef == 1.0
    for p, g in zip(params, grads):
        np.testing.assert_allclose(p.grad.numpy(), g.astype(F64) * coef, rtol=1e-12, atol=0.0)


def test_norm_ref_skips_empty_entries_and_holds_1e20():
    assert cn.norm_ref([None, np.zeros(0, F32), np.array([3.0, 4.0], F32), None]) == 5.0
    big = cn.norm_ref([np.full(1000, 1e20, F32)])          # the sum of squares is 1e43: past fp32, nothing to float64
    assert math.isfinite(big) and big == pytest.approx(float(F32(1e20)) * math.sqrt(1000.0), rel=1e-12)


@pytest.mark.parametrize("norm", [0.0, 1e-7, 0.5, 1.0 - 2.0 ** -24, 1.0, 3.0, 1234.5678, 1e12, 1e30])
@pytest.mark.parametrize("max_norm", [1.0, 0.01, 5.0, float("inf")])
def test_coef_f32_against_torch_fp32(norm, max_norm):
    """torch forms max_norm / (norm + 1e-6) as reciprocal times scalar (two roundings), the kernel divides (one):
    2 u relative, not bit equality."""
    n32 = F32(norm)
    want = float(torch.clamp(max_norm / (torch.tensor(n32) + 1e-6), max=1.0))
    got = float(cn.coef_f32(n32, max_norm))
    assert abs(got - want) <= 2.0 * U * abs(want), (got, want)
    assert got <= 1.0 and (max_norm != float("inf") or got == 1.0)


def test_coef_f32_is_three_fp32_operations():
    n32 = F32(7.25)
    assert cn.coef_f32(n32, 2.0) == F32(F32(2.0) / F32(n32 + F32(1e-6)))
    assert cn.coef_f32(F32(0.0), 1.0) == F32(1.0) and cn.coef_f32(F32(0.5), 1.0) == F32(1.0)
    assert cn.coef_f32(F32(np.inf), 1.0) == F32(0.0) and cn.coef_f32(F32(np.nan), 1.0) == F32(1.0)   # fminf drops a NaN


def test_clip_table_layout():
    for n in (9, 25, 49):
        tab = cn.clip_table(n)
        assert len(tab) == n and (n == 9 or [i for i, h in enumerate(tab) if h is None] == [n // 2 - 1, n // 2])
        assert tab[cn.unaligned_slot(tab)][1].size == 4097
    g = np.concatenate([h[1] for h in cn.clip_table(9) if h is not None])
    assert np.abs(g).max() > 1e11 and 0 < np.abs(g[g != 0]).min() < 1e-11
    assert all((h[1] == F32(1e20)).all() for h in cn.clip_table(9, fill=1e20) if h is not None)


# ---------------------------------------------------------------------------------------------- the C entries' refusals
def _arr(kind, values):
    return (kind * max(len(values), 1))(*values)


def _ptrs(values):
    return _arr(ctypes.c_void_p, values)


def _numel(values):
    return _arr(ctypes.c_int64, values)


def _lib():
    from sparch_amd._capi import lib
    return lib


def _norm(n=2, grads=(P, P), numel=(5, 3), max_norm=1.0, ws=P, ws_bytes=1 << 20, clip=P, tables=True):
    return _lib().sparch_grad_norm(n, _ptrs(grads) if tables else None, _numel(numel) if tables else None, max_norm, ws,
                                   ws_bytes, clip, None, None, None)


def test_grad_norm_refusals():
    lib = _lib()
    assert _norm(n=-1) == EINVAL
    assert _norm(tables=False) == EINVAL                                   # NULL tables, n_tensors > 0
    assert lib.sparch_grad_norm(2, _ptrs((P, P)), None, 1.0, P, 1 << 20, P, None, None, None) == EINVAL
    assert lib.sparch_grad_norm(2, None, _numel((5, 3)), 1.0, P, 1 << 20, P, None, None, None) == EINVAL
    assert _norm(numel=(5, -1)) == EINVAL
    assert _norm(grads=(P, None)) == EINVAL                                # NULL behind a non-empty tensor
    for bad in (float("nan"), 0.0, -1.0, -float("inf")):
        assert _norm(max_norm=bad) == EINVAL, bad
    assert _norm(clip=None) == EINVAL
    need = lib.sparch_grad_norm_ws_bytes(2, _numel((5, 3)))
    assert need > 0
    assert _norm(ws=None) == EWORKSPACE and _norm(ws_bytes=0) == EWORKSPACE and _norm(ws_bytes=need - 1) == EWORKSPACE
    # every EINVAL comes in front of the workspace
    assert _norm(ws=None, clip=None) == EINVAL and _norm(ws_bytes=0, max_norm=0.0) == EINVAL
    assert _norm(ws_bytes=0, numel=(5, -1)) == EINVAL and _norm(ws=None, grads=(None, P)) == EINVAL


def _step_clip(n=2, tables=(0, 1, 2, 3, 4), p=(P, P), g=(P, P), m=(P, P), v=(P, P), numel=(5, 3), clip=P):
    args = [_ptrs(p), _ptrs(g), _ptrs(m), _ptrs(v), _numel(numel)]
    args = [a if i in tables else None for i, a in enumerate(args)]
    return _lib().sparch_adam_step_clip(n, *args, 0.01, 0.9, 0.999, 1.0, 1e-8, 0.0, None, None, clip, None)


def test_adam_step_clip_refusals():
    assert _step_clip(n=-1) == EINVAL
    for missing in range(5):
        assert _step_clip(tables=[i for i in range(5) if i != missing]) == EINVAL, missing
    assert _step_clip(numel=(5, -1)) == EINVAL
    for which in "pgmv":
        assert _step_clip(**{which: (P, None)}) == EINVAL, which
    assert _step_clip(clip=None) == EINVAL
    assert _step_clip(clip=None, numel=(0, 0), p=(None, None)) == EINVAL   # ... also when there is nothing to launch


def test_scale_grads_refusals():
    lib = _lib()
    assert lib.sparch_scale_grads(-1, _ptrs((P,)), _numel((4,)), P, None) == EINVAL
    assert lib.sparch_scale_grads(1, None, _numel((4,)), P, None) == EINVAL
    assert lib.sparch_scale_grads(1, _ptrs((P,)), None, P, None) == EINVAL
    assert lib.sparch_scale_grads(2, _ptrs((P, P)), _numel((4, -2)), P, None) == EINVAL
    assert lib.sparch_scale_grads(2, _ptrs((P, None)), _numel((4, 2)), P, None) == EINVAL
    assert lib.sparch_scale_grads(1, _ptrs((P,)), _numel((4,)), None, None) == EINVAL


def test_ws_bytes_is_monotone_and_covers_one_double_per_chunk():
    q = _lib().sparch_grad_norm_ws_bytes
    prev = 0
    for n in (0, 1, 4095, 4096, 4097, 8192, 8193, 1 << 20, (1 << 27) + 1):
        b = q(1, _numel((n,)))
        assert b >= 8 * -(-n // 4096) and b >= prev, n
        prev = b
    sizes = []
    prev = 0
    for n in (1, 4097, 0, 12289, 255, 0, 8192):                            # one more tensor never needs less
        sizes.append(n)
        b = q(len(sizes), _numel(sizes))
        assert b >= 8 * sum(-(-k // 4096) for k in sizes) and b >= prev, sizes
        prev = b
    assert q(0, None) == 0 and q(2, None) == 0 and q(1, _numel((-1,))) == 0


# ---------------------------------------------------------------------------------------------- Python arguments
@pytest.mark.parametrize("bad", [0, 0.0, -1, -1.0, float("nan"), "x", True, -float("inf")])
def test_adam_refuses_a_bad_max_grad_norm(bad):
    from sparch_amd.optim import Adam
    with pytest.raises(ValueError):
        Adam([torch.zeros(3, requires_grad=True)], 1e-2, max_grad_norm=bad)


def test_adam_accepts_a_positive_max_grad_norm_inf_and_none():
    from sparch_amd.optim import Adam
    for ok, want in ((0.5, 0.5), (2, 2.0), (float("inf"), float("inf")), (None, None)):
        assert Adam([torch.zeros(3, requires_grad=True)], 1e-2, max_grad_norm=ok).max_grad_norm == want


def test_clip_grad_environment_switch():
    from sparch_amd import exp
    assert exp.parse_clip_grad(None) is None and exp.parse_clip_grad("") is None and exp.parse_clip_grad("  ") is None
    assert exp.parse_clip_grad("0.5") == 0.5 and exp.parse_clip_grad(" 2 ") == 2.0
    assert exp.parse_clip_grad("inf") == float("inf")
    for bad in ("abc", "0", "-1", "nan", "-inf", "1,5"):
        with pytest.raises(ValueError):
            exp.parse_clip_grad(bad)


def test_adam_without_max_grad_norm_never_touches_the_new_symbols(monkeypatch):
    """The three launching symbols (and the query) are patched to raise; a plain Adam().step() then runs up to the
    device check that already exists (the parameters of this test live on the CPU) without meeting them."""
    from sparch_amd import optim

    def boom(*a, **k):
        raise AssertionError("an optimizer without max_grad_norm reached a clipping symbol")

    for name in ("sparch_grad_norm", "sparch_adam_step_clip", "sparch_scale_grads", "sparch_grad_norm_ws_bytes"):
        monkeypatch.setattr(optim.lib, name, boom, raising=True)
    p = torch.zeros(5, requires_grad=True)
    p.grad = torch.ones(5)
    opt = optim.Adam([p], 1e-2)
    assert opt.max_grad_norm is None and opt.sync_skipped() == 0
    with pytest.raises(RuntimeError, match="float32 dense parameters on the GPU only"):
        opt.step()
    # ... and with it the same device check comes first, before any norm is taken
    with pytest.raises(RuntimeError, match="float32 dense parameters on the GPU only"):
        optim.Adam([p], 1e-2, max_grad_norm=1.0).step()
