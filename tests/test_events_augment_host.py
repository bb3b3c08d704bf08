"""CPU: the host side of SHD / SSC event augmentation — the spec's parser, the draws and their fixed order, the NumPy
restatement of the kernel (tests/events_augment_numpy.py) at the identity, the bound that decides between the bf16
plane and dense fp32, and the bindings."""
import math

import numpy as np
import pytest

from oracle import events_numpy as ev
from tests import events_augment_numpy as evaug
from tests.event_cases import fake_h5

FULL = "shift=40,scale=0.2,offset=0.1,drop=0.1,tmask=0.15,umask=70"


def _mod():
    from sparch_amd.dataloaders import event_augment
    return event_augment


def test_parser_accepts():
    ea = _mod()
    assert ea.parse_event_augment(FULL) == dict(shift=40, scale=0.2, offset=0.1, drop=0.1, tmask=0.15, umask=70)
    off = dict(shift=0, scale=0.0, offset=0.0, drop=0.0, tmask=0.0, umask=0)
    assert ea.parse_event_augment("") == off
    assert ea.parse_event_augment("drop=0.25") == dict(off, drop=0.25)
    assert ea.parse_event_augment(" umask=7 , shift=3 ") == dict(off, umask=7, shift=3)
    assert ea.parse_event_augment("scale=0.999,drop=0.999") == dict(off, scale=0.999, drop=0.999)
    assert isinstance(ea.parse_event_augment("shift=3")["shift"], int)


@pytest.mark.parametrize("text", ["jitter=0.1", "shift", "shift=", "shift=abc", "shift=1.5", "shift=-1", "scale=1",
                                  "scale=1.5", "drop=1", "drop=-0.1", "tmask=nan", "offset=inf", "shift=3,shift=4",
                                  "shift=70000", "umask=2.5", "drop=0.1;shift=2"])
def test_parser_refuses(text):
    with pytest.raises(ValueError):
        _mod().parse_event_augment(text)


def test_draws_are_deterministic_and_in_range():
    ea = _mod()
    spec = ea.parse_event_augment(FULL)
    n, nb_units, max_time = 4000, 700, 1.4
    t0, s0 = ea.draw_event_augmentation(n, spec, np.random.default_rng([5, 0, 1]), nb_units, max_time)
    t1, s1 = ea.draw_event_augmentation(n, FULL, np.random.default_rng([5, 0, 1]), nb_units, max_time)
    t2, s2 = ea.draw_event_augmentation(n, spec, np.random.default_rng([5, 0, 2]), nb_units, max_time)
    assert t0.dtype == np.float32 and t0.shape == (n, ea.EVAUG_FIELDS) and ea.EVAUG_FIELDS == 8
    assert np.array_equal(t0, t1) and s0 == s1 and isinstance(s0, int)
    assert not np.array_equal(t0, t2) and s0 != s2
    assert 0 <= s0 < 2 ** 63
    d, a, c, p, m0, m1, k0, k1 = t0.T
    assert np.array_equal(d, np.rint(d)) and d.min() == -40 and d.max() == 40
    assert a.min() >= np.float32(0.8) and a.max() <= np.float32(1.2) and a.std() > 0.05
    assert np.abs(c).max() <= np.float32(0.1) and c.min() < 0 < c.max()
    assert np.all(p == np.float32(0.1))
    assert m0.min() >= 0 and np.all(m1 >= m0) and (m1 - m0).max() <= 0.15 + 1e-6 and m1.max() <= 1.4 + 1e-6
    for k in (k0, k1):
        assert np.array_equal(k, np.rint(k))
    assert k0.min() >= 0 and np.all(k1 >= k0) and (k1 - k0).max() == 70 and k1.max() <= 700
    ea.check_event_augmentation(t0, n)                                   # what it draws, the store accepts


def test_field_order_is_pinned():
    """The documented order of the draws, restated call by call, and one table written out."""
    ea = _mod()
    table, seed = ea.draw_event_augmentation(3, FULL, np.random.default_rng(123), 700, 1.4)
    g = np.random.default_rng(123)
    d = g.integers(-40, 40, 3, endpoint=True)
    a = g.uniform(0.8, 1.2, 3)
    c = g.uniform(-0.1, 0.1, 3)
    w = g.uniform(0.0, 0.15, 3)
    m0 = g.uniform(0.0, 1.4 - w)
    kw = g.integers(0, 70, 3, endpoint=True)
    k0 = g.integers(0, 700 - kw, endpoint=True)
    restated = np.stack([d, a, c, np.full(3, 0.1), m0, m0 + w, k0, k0 + kw], axis=1).astype(np.float32)
    assert np.array_equal(table, restated)
    assert seed == int(g.integers(0, 2 ** 63))
    expected = np.array([[-39, 8.8814396e-01, 6.2418900e-02, 0.1, 3.1282881e-01, 4.3579200e-01, 103, 106],
                         [15, 8.7374872e-01, 8.4669001e-02, 0.1, 1.0439153e+00, 1.1773992e+00, 423, 452],
                         [8, 8.7036234e-01, -4.4685122e-02, 0.1, 2.8282005e-01, 3.5976562e-01, 284, 336]], np.float32)
    assert np.array_equal(table, expected)
    assert seed == 2138975501910086797
    # a transform that is off draws nothing: the later fields come from the same stream, earlier in it
    t2, _ = ea.draw_event_augmentation(3, "offset=0.1", np.random.default_rng(123), 700, 1.4)
    assert np.array_equal(t2[:, 2], np.random.default_rng(123).uniform(-0.1, 0.1, 3).astype(np.float32))


def test_everything_off_is_the_identity_row():
    ea = _mod()
    table, seed = ea.draw_event_augmentation(5, "", np.random.default_rng(1), 700, 1.4)
    assert np.array_equal(table, np.tile(np.array([0, 1, 0, 0, 0, 0, 0, 0], np.float32), (5, 1)))
    assert np.array_equal(table, ea.identity_rows(5))
    assert seed == int(np.random.default_rng(1).integers(0, 2 ** 63))     # the seed is drawn all the same


@pytest.mark.parametrize("tdtype", [np.float16, np.float32])
def test_restatement_at_the_identity_equals_bin_sample(tdtype):
    ea = _mod()
    h5 = fake_h5(tdtype=tdtype)
    samples = list(zip(h5["spikes"]["times"], h5["spikes"]["units"]))
    # events the reference's rule rejects, and a unit the store keeps as its marker
    samples[2] = (np.concatenate([samples[2][0], np.array([-0.1, 1.5, 0.5, 0.5], tdtype)]),
                  np.concatenate([samples[2][1], np.array([3, 3, 700, 70000], np.int64)]))
    idx = [0, 2, 4, 2, 10]
    got, lost = evaug.bin_batch_augmented(samples, idx, ea.identity_rows(len(idx)), 77, 100, 700, 1.4)
    want = 0
    for b, s in enumerate(idx):
        ref, nd = ev.bin_sample(samples[s][0], samples[s][1], 100, 700, 1.4)
        assert np.array_equal(got[b], ref)
        want += nd
    assert lost == want == 8                                              # four rejects, the sample drawn twice


def test_restatement_transforms():
    """Hand cases of the restatement itself: shift, scale + offset, masks, the marker, the drop draw."""
    from tests.dropout_numpy import uniforms

    t = np.array([0.1, 0.5, 0.9, 1.3], np.float32)
    u = np.array([0, 10, 699, 70000], np.int64)
    row = [5, 0.5, 0.25, 0, 0, 0, 0, 0]
    tp, up, gone = evaug.augment_sample(t, u, row, 1, 0)
    assert gone == 1 and up.tolist() == [5, 15, 704]                      # the marker never comes back
    assert np.array_equal(tp, (np.float32(0.5) * t[:3]).astype(np.float32) + np.float32(0.25))
    tp, up, gone = evaug.augment_sample(t, u, [5, 0.5, 0.25, 0, 0.45, 0.55, 704, 705], 1, 0)
    assert gone == 3 and up.tolist() == [5]                               # t' = 0.5 masked, u' = 704 masked
    r = uniforms(9, 4, first_index=3 << 32)
    tp, up, gone = evaug.augment_sample(t, u % 700, [0, 1, 0, 0.5, 0, 0, 0, 0], 9, 3)
    assert gone == int((r < np.float32(0.5)).sum()) and np.array_equal(tp, t[r >= np.float32(0.5)])
    other = uniforms(9, 4, first_index=4 << 32)
    assert not np.array_equal(r, other)                                   # the batch row enters the draw


def test_table_validation():
    ea = _mod()
    good = ea.identity_rows(3)
    assert ea.check_event_augmentation(good, 3).dtype == np.float32
    assert ea.check_event_augmentation(good.astype(np.float64).tolist()).shape == (3, 8)

    def changed(field, value):
        t = good.copy()
        t[1, field] = value
        return t

    for bad in (changed(1, 0.0), changed(1, -1.0), changed(2, np.nan), changed(4, np.inf), changed(3, 1.0),
                changed(3, -0.1), changed(0, 0.5), changed(6, 1.5), changed(7, 2.5), changed(0, 70000),
                good[:, :7], good[0], good.reshape(3, 2, 4)):
        with pytest.raises(ValueError):
            ea.check_event_augmentation(bad)
    with pytest.raises(ValueError):
        ea.check_event_augmentation(good, 4)


class _CountStore:
    """An EventStore whose largest bin count is given: `serves_plane` needs nothing else of it."""

    def __init__(self, top):
        self.top = top

    def prepare(self, nb_steps):
        return self.top


def test_plane_bound(monkeypatch):
    from sparch_amd import functional as Fn

    ea = _mod()
    assert [ea.plane_count_factor(s) for s in (0.0, 0.2, 0.5, 0.6, 0.75)] == [3, 4, 4, 5, 6]
    for s in (0.0, 0.2, 0.5, 0.9):
        assert ea.plane_count_factor(s) == math.ceil(1 / (1 - s)) + 2
    serves = Fn.EventStore.serves_plane
    monkeypatch.setattr(Fn, "DENSE_GEMM", "split6")                      # the plane is served with this GEMM only
    assert serves(_CountStore(255), 100) and not serves(_CountStore(256), 100)          # unaugmented: as before
    assert serves(_CountStore(63), 100, 0.2) and not serves(_CountStore(64), 100, 0.2)  # 63 * 4 = 252, 64 * 4 = 256
    assert serves(_CountStore(85), 100, 0.0) and not serves(_CountStore(86), 100, 0.0)  # 85 * 3 = 255
    assert serves(_CountStore(42), 100, 0.75) and not serves(_CountStore(43), 100, 0.75)  # 42 * 6 = 252
    with pytest.raises(ValueError):
        serves(_CountStore(1), 100, 1.0)


def test_augment_needs_the_resident_loader(monkeypatch):
    from sparch_amd.dataloaders import spiking_datasets as sd

    monkeypatch.delenv("SPARCH_EVENTS", raising=False)
    for resident in ("", None):
        with pytest.raises(ValueError, match="resident"):
            sd.load_shd_or_ssc("shd", "/unused", "train", 4, h5_file=fake_h5(), device="cpu", resident=resident,
                               augment="drop=0.1")
    with pytest.raises(ValueError, match="jitter"):                                     # the spec is parsed up front
        sd.load_shd_or_ssc("shd", "/unused", "train", 4, h5_file=fake_h5(), device="cpu", resident="resident",
                           augment="jitter=0.1")


def test_entry_point_is_bound():
    from sparch_amd import _capi

    assert _capi.lib.sparch_abi_version() == 5
    fn = _capi.lib.sparch_events_gather_bin_aug
    plain = _capi.lib.sparch_events_gather_bin
    assert len(fn.argtypes) == len(plain.argtypes) + 2
    assert list(fn.argtypes[:len(plain.argtypes) - 1]) == list(plain.argtypes[:-1])    # every argument of the plain call
    # every pointer refused before anything is launched (no device needed)
    assert fn(None, 0, None, None, None, 1, None, 1, 100, 700, 1.4, 1, None, None, None, None, None, None, 0, None, 0,
              None) == -1
