"""CPU: tests/kit.py decides whether a kernel passes, so its rules are shown to bite here, without a GPU."""
import numpy as np
import pytest
import torch

from tests import kit
from tests.kit import F32, F64, same_bits, within


# ------------------------------------------------------------------------------------------------ within
def test_within_passes_at_the_bound_and_returns_the_worst_fraction():
    ref = np.array([1.0, 2.0, 4.0])
    assert within(ref + np.array([0.25, 0.0, -0.5]), ref, 0.5, "scalar bound") == 1.0
    assert within(ref + np.array([0.25, 0.0, -0.5]), ref, np.array([1.0, 0.0, 2.0]), "array bound") == 0.25
    assert within(np.float32(3.0), 3.0, 0.0, "scalars, no error over a zero bound") == 0.0
    assert within(ref, ref, np.zeros(3), "no error over zero bounds") == 0.0
    assert within(np.zeros((0, 4)), np.zeros((0, 4)), 1.0, "empty") == 0.0


def test_within_takes_both_sides_to_fp64():
    got, ref = np.array([1.0], F32), np.array([1.0 + 2.0 ** -30])
    assert 0.0 < within(got, ref, 2.0 ** -29, "fp32 against fp64") <= 0.5       # the difference is seen, not rounded away


def test_within_refuses_a_nan_in_got():
    with pytest.raises(AssertionError, match="NaN"):
        within(np.array([1.0, np.nan]), np.array([1.0, 2.0]), 1e30, "x")
    with pytest.raises(AssertionError, match="NaN"):
        within(np.array([np.nan]), np.array([np.nan]), 1e30, "x")


def test_within_refuses_another_shape():
    with pytest.raises(AssertionError, match="shape"):
        within(np.zeros((2, 3)), np.zeros(3), 1.0, "a reference that would broadcast")
    with pytest.raises(AssertionError, match="shape"):
        within(np.zeros(3), 0.0, 1.0, "a scalar reference")


def test_within_refuses_one_element_above_an_array_bound_with_slack_elsewhere():
    ref, bound = np.zeros((2, 3)), np.full((2, 3), 10.0)
    got = ref.copy()
    bound[1, 2], got[1, 2], got[0, 0] = 1e-3, 2e-3, 5.0           # the largest error is inside its bound
    with pytest.raises(AssertionError, match=r"2\.000 of the bound .*\(1, 2\); 1 of 6 elements above it"):
        within(got, ref, bound, "x")
    assert within(got, ref, 10.0, "x") == 0.5
    with pytest.raises(AssertionError, match="1 of 6"):
        within(got, ref, np.array([10.0, 10.0, 1e-3]), "a bound that broadcasts over the rows")


def test_within_refuses_an_error_over_a_zero_negative_or_nan_bound():
    for bad in (0.0, -1.0, np.nan):
        with pytest.raises(AssertionError, match="inf of the bound"):
            within(np.array([0.0, 1e-300]), np.zeros(2), np.array([1.0, bad]), "x")


# ------------------------------------------------------------------------------------------------ bits
def test_same_bits_tells_the_zeros_and_nan_payloads_apart():
    for dt in (F32, F64):
        assert same_bits(np.zeros(3, dt), np.zeros(3, dt)) and not same_bits(np.zeros(3, dt), -np.zeros(3, dt))
    a = np.array([0x7FC00000, 0x7FC00001], np.uint32).view(F32)
    assert np.isnan(a).all() and same_bits(a, a.copy()) and not same_bits(a[:1], a[1:])
    t = torch.from_numpy(a)
    assert same_bits(t, t.clone()) and not same_bits(t[:1], t[1:])
    assert not same_bits(torch.zeros(2), -torch.zeros(2))


def test_same_bits_refuses_another_dtype_or_shape():
    assert not same_bits(np.ones(2, F32), np.ones(2, F64))
    assert not same_bits(np.zeros(2, F32), np.zeros(2, np.int32))                 # the same words, another type
    assert not same_bits(np.zeros((2, 1), F32), np.zeros(2, F32))
    assert not same_bits(torch.zeros(2), torch.zeros(2, dtype=torch.int32))
    assert not same_bits(torch.zeros(2), np.zeros(2, F32))
    assert not same_bits(torch.zeros(2, dtype=torch.bfloat16), torch.zeros(2, dtype=torch.float16))


def test_same_bits_and_bits_on_two_byte_words():
    a = torch.tensor([1.0, -0.0, 3.140625], dtype=torch.bfloat16)
    b = a.clone()
    assert same_bits(a, b)
    b[1] = 0.0
    assert not same_bits(a, b) and bool(torch.equal(a.float(), b.float()))        # equal values, other bits
    assert kit.bits(a).dtype == np.uint16 and kit.bits(a).tolist() == [0x3F80, 0x8000, 0x4049]
    assert np.array_equal(kit.words(a), kit.bits(a)) and kit.raw(a).dtype == np.int16
    assert kit.bits(np.ones(1, F32)).tolist() == [0x3F800000] and kit.bits(np.ones(1, F64)).dtype == np.uint64
    assert same_bits(np.arange(6, dtype=F32).reshape(2, 3).T, np.arange(6, dtype=F32).reshape(2, 3).T.copy())


def test_sha_is_stable_across_non_contiguous_views():
    a = np.arange(24, dtype=F32).reshape(4, 6)
    assert kit.sha(a.T) == kit.sha(np.ascontiguousarray(a.T)) and kit.sha(a[:, ::2]) == kit.sha(a[:, ::2].copy())
    assert kit.sha(a.T) != kit.sha(a) and kit.sha(a, a) != kit.sha(a)
    assert kit.sha(a.astype(F64)) != kit.sha(a)


# ------------------------------------------------------------------------------------------------ moves
def test_D_keeps_the_dtype_unless_told_otherwise(monkeypatch):
    monkeypatch.setattr(kit, "DEV", "cpu")
    x = np.arange(6, dtype=F64).reshape(2, 3)
    assert kit.D(x).dtype == torch.float64 and kit.D(x, F32).dtype == torch.float32
    assert kit.D(x.astype(np.int64)).dtype == torch.int64 and kit.D(None) is None
    assert kit.D(x.T).is_contiguous() and torch.equal(kit.D(x.T), torch.from_numpy(x).T)
    assert kit.N(None) is None and kit.ptr(None) is None
    b = torch.tensor([1.0, 2.5], dtype=torch.bfloat16, requires_grad=True)
    assert kit.N(b, torch.float32).tolist() == [1.0, 2.5] and kit.N(kit.D(x)).dtype == F64


def test_relmax_and_the_constants():
    assert kit.relmax([1.0, 2.0], [1.0, 4.0]) == pytest.approx(0.5, rel=1e-6)
    assert (kit.OK, kit.EINVAL, kit.EALIGN, kit.EWORKSPACE) == (0, -1, -2, -3)
    assert kit.SEED >> 32 and kit.SEED & 0xFFFFFFFF and kit.SEED < 2 ** 63        # both halves take part; no address


def test_split3_host_is_exact():
    x = torch.randn(5, 7, generator=torch.Generator().manual_seed(1))
    p = kit.split3_host(x)
    assert p.dtype == torch.bfloat16 and p.shape == (15, 7)
    assert torch.equal((p[:5].float() + p[5:10].float()) + p[10:].float(), x)
