"""
The one toolkit of the test tree: constants, lazy imports of the package, host <-> device moves, bit comparisons and
the acceptance rule `within`.  Every restatement (tests/*_numpy.py), every case module (tests/*_cases.py) and every
test module takes these from here; none defines its own.

Nothing here creates a tensor or touches torch.cuda at import, and sparch_amd is imported only inside functions: the
first GPU test of a session starts child processes that must come before any GPU use of the parent (tests/conftest.py).
"""
import hashlib

import numpy as np
import pytest
import torch

DEV = "cuda"
F32, F64 = np.float32, np.float64
SEED = 0x1234567_89ABCDEF                    # the shared dropout seed: both 32-bit halves of it take part
OK, EINVAL, EALIGN, EWORKSPACE = 0, -1, -2, -3

_WORD = {2: np.uint16, 4: np.uint32, 8: np.uint64}
_TWORD = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def Fn():
    from sparch_amd import functional
    return functional


def capi():
    from sparch_amd import _capi
    return _capi


def D(a, dtype=None):
    """A host array on the device, in its own dtype unless one is given."""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def N(t, dtype=None):
    """A tensor as a numpy array, after everything queued on the device has finished; dtype (a torch one) converts
    first: numpy has no bf16."""
    if t is None:
        return None
    t = t.detach()
    if t.is_cuda:
        torch.cuda.synchronize()
    return (t if dtype is None else t.to(dtype)).cpu().numpy()


def nan_(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def ptr(t):
    return None if t is None else t.data_ptr()


def bits(a):
    """The elements of a numpy array or a tensor as unsigned words of their own size (2, 4 or 8 bytes)."""
    if isinstance(a, torch.Tensor):
        a = a.detach().contiguous().cpu()
        a = a.view(_TWORD[a.element_size()]).numpy()
    a = np.ascontiguousarray(a)
    return a.view(_WORD[a.dtype.itemsize])


def same_bits(a, b):
    """Same dtype, same shape and every bit equal (+0.0 is not -0.0, a NaN equals only its own payload); two numpy
    arrays or two tensors."""
    if isinstance(a, torch.Tensor) or isinstance(b, torch.Tensor):
        if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)):
            return False
        w = _TWORD[a.element_size()]
        return a.dtype == b.dtype and a.shape == b.shape and bool(torch.equal(a.view(w), b.view(w)))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((bits(a) == bits(b)).all())


def words(t):
    """The 16-bit words of a bf16 device tensor."""
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def raw(t):
    """The bytes of a device tensor as a numpy array (bf16 as its 16-bit words)."""
    t = t.detach().contiguous().cpu()
    return (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).numpy()


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def relmax(a, b):
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-6))


def within(got, ref, bound, what):
    """Asserts |got - ref| <= bound everywhere and returns the worst fraction of the bound.  bound is a scalar or an
    array that broadcasts to the error.  It fails on differing shapes, on a NaN in the error and on any element above
    its bound; an element with no error passes whatever its bound, an error over a zero bound fails."""
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape}, the reference has {ref.shape}"
    err = np.abs(got - ref)
    assert not np.isnan(err).any(), f"{what}: NaN"
    if not err.any():
        return 0.0
    bound = np.broadcast_to(np.asarray(bound, F64), err.shape)
    above = (err != 0) & ~(err <= bound)                              # (~: a NaN bound holds nothing)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    r = np.where(above & ~(r > 1.0), np.inf, r)                       # (a negative or NaN bound)
    at = tuple(int(i) for i in np.unravel_index(int(np.argmax(r)), r.shape))
    f = float(r[at])
    print(f"  {what}: {f:.3f} of the bound {float(bound[at]):.3e}")
    assert not above.any(), (f"{what}: {f:.3f} of the bound {float(bound[at]):.3e} (at {at}; {int(above.sum())} of "
                             f"{err.size} elements above it)")
    return f


def record(record_property, *worst):
    record_property("worst_fraction_of_bound", round(max(worst), 3))
    print(f"  worst fraction of bound {max(worst):.3f}")


@pytest.fixture
def bf16_mode():
    """The bf16 operand mode (sparch_set_operand_precision) for one test; fp32 restored afterwards."""
    F = Fn()
    prev = F.set_compute_dtype("bf16")
    yield F
    F.set_compute_dtype(prev)


@pytest.fixture(scope="module")
def sp():
    """The package, imported when the first test of a module asks for it."""
    import sparch_amd
    return sparch_amd


def split3_host(x):
    """The exact truncation split x = p0 + p1 + p2 (include/sparch_hip.h sparch_split3) as (3 * rows, cols) bf16."""
    def trunc(v):
        return (v.contiguous().view(torch.int32) & -65536).view(torch.float32)
    p0 = trunc(x)
    r1 = x - p0
    p1 = trunc(r1)
    p2 = trunc(r1 - p1)
    return torch.cat([p0, p1, p2], 0).to(torch.bfloat16)
