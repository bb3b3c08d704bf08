"""GPU: SHD / SSC event augmentation inside the gather-and-bin kernel.  `sparch_events_gather_bin_aug` (events.hip)
against its NumPy restatement (tests/events_augment_numpy.py), exact equality of dense, counts, plane and n_dropped;
against `sparch_events_gather_bin` at the identity; the resident loader's epochs against the restatement; run_exp.py
with SPARCH_EVENTS_AUGMENT on packs.  The sample maker and the fake file are those of the resident-store tests."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import events_numpy as ev
from tests import events_augment_numpy as evaug
from tests.event_cases import dense as _dense
from tests.event_cases import fake_h5 as _fake_h5
from tests.event_cases import samples as _samples
from tests.event_cases import store as _store
from tests.kit import DEV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_TIME = 1.4
BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))


def _ea():
    from sparch_amd.dataloaders import event_augment
    return event_augment


def _spec(nb_units):
    """Every transform on, the unit ranges scaled to the store's width (one unit: a shift of -1, 0 or 1)."""
    return f"shift={max(1, min(40, nb_units // 4))},scale=0.2,offset=0.1,drop=0.1,tmask=0.15,umask={max(1, nb_units // 10)}"


def _gather(store, idx, nb_steps, table, seed, **want):
    want = want or dict(plane=True, dense=True, counts=True, dropped=True)
    got = store.gather(torch.as_tensor(idx, dtype=torch.int64).to(DEV), nb_steps, augment=(table, seed), **want)
    torch.cuda.synchronize()
    return got


def _check(store, samples, idx, nb_steps, nb_units, table, seed, **want):
    """The kernel's outputs for (idx, table, seed) equal the restatement's; returns the restatement's batch."""
    got = _gather(store, idx, nb_steps, table, seed, **want)
    B, ldp = len(idx), (nb_units + 7) // 8 * 8
    ref, lost = evaug.bin_batch_augmented(samples, idx, table, seed, nb_steps, nb_units, store.max_time)
    assert np.array_equal(got["dense"].cpu().numpy(), ref)
    assert ref.max() <= 255                                               # exact as a byte and in bf16
    if "counts" in got:
        assert np.array_equal(got["counts"].cpu().numpy(), ref.astype(np.uint8))
    plane = got["plane"]
    assert tuple(plane.shape) == (B * nb_steps, ldp) and plane.dtype == torch.bfloat16
    p = plane.view(B, nb_steps, ldp)
    assert np.array_equal(p[:, :, :nb_units].float().cpu().numpy(), ref)
    assert int(p[:, :, nb_units:].contiguous().view(torch.int16).abs().max() if ldp > nb_units else 0) == 0
    if "n_dropped" in got:
        assert int(got["n_dropped"].item()) == lost
    assert got["y"].cpu().tolist() == [3 * s for s in idx]
    return ref, lost


def _hand_rows(nb_units):
    """(name, row): each pushes one rule to its limit."""
    ident = [0, 1, 0, 0, 0, 0, 0, 0]

    def row(**kw):
        r = list(ident)
        for k, v in kw.items():
            r["d a c p m0 m1 k0 k1".split().index(k)] = v
        return r

    return [("everything shifts out above", row(d=nb_units)),
            ("everything shifts out below", row(d=-nb_units)),
            ("compressed and pushed below 0", row(a=0.5, c=-0.2)),
            ("stretched past max_time", row(a=1.5)),
            ("stretched and late", row(a=1.5, c=0.3)),
            ("time mask over the whole window", row(m0=-1.0, m1=10.0)),
            ("band over all units", row(d=3, k0=0, k1=nb_units + 3)),
            ("an empty mask and an empty band", row(m0=0.5, m1=0.5, k0=7, k1=2)),
            ("p = 0", row(p=0.0, d=1)),
            ("p just below 1", row(p=BELOW_ONE))]


def _trimmed(samples, nb_units, nb_steps):
    if nb_units == 1:   # one unit: keep every bin count <= 255 under compression too (see the resident-store test)
        return [(t[:150], u[:150]) if len(t) > 150 and nb_steps > 2 else (t[:100], u[:100]) for t, u in samples]
    return samples


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("tdtype", [np.float16, np.float32])
@pytest.mark.parametrize("nb_units", [1, 700, 701])
@pytest.mark.parametrize("nb_steps", [2, 100, 250])
def test_kernel_equals_the_restatement(nb_steps, nb_units, tdtype, sort):
    ea = _ea()
    rng = np.random.default_rng(nb_steps * 1000 + nb_units)
    samples = _trimmed(_samples(rng, nb_steps, nb_units, MAX_TIME, tdtype, n_random=6, sort=sort), nb_units, nb_steps)
    store = _store(samples, nb_units, MAX_TIME)
    assert store.sorted == sort
    n = len(samples)
    draw = np.random.default_rng([nb_steps, nb_units, int(sort)])

    # identity rows: the augmenting entry point gives what the plain one gives, bit for bit
    everyone = list(range(n))
    idx_d = torch.as_tensor(everyone, dtype=torch.int64).to(DEV)
    plain = store.gather(idx_d, nb_steps, plane=True, dense=True, counts=True, dropped=True)
    same = _gather(store, everyone, nb_steps, ea.identity_rows(n), 5)
    for k in ("dense", "counts", "y", "n_dropped"):
        assert torch.equal(plain[k], same[k]), k
    assert torch.equal(plain["plane"].view(torch.int16), same["plane"].view(torch.int16))

    # random rows, every transform on: all samples, B = 1, a repeated index
    table, seed = ea.draw_event_augmentation(n, _spec(nb_units), draw, nb_units, MAX_TIME)
    ref, lost = _check(store, samples, everyone, nb_steps, nb_units, table, seed)
    assert lost >= 6                                                          # the hand-made sample's rejects at least
    assert ref.sum() > 0 or nb_units == 1
    _check(store, samples, [n - 2], nb_steps, nb_units, table[:1], seed)
    big = max(range(n), key=lambda s: len(samples[s][0]))
    assert len(samples[big][0]) >= 50
    rep = [big, n - 2, big, 0, big]
    # (one row, drop alone, for every copy of the repeated sample: only the batch row in the draw tells them apart)
    t5, seed5 = ea.draw_event_augmentation(5, _spec(nb_units), draw, nb_units, MAX_TIME)
    t5[[0, 2, 4]] = np.array([0, 1, 0, 0.3, 0, 0, 0, 0], np.float32)
    ref5, _ = _check(store, samples, rep, nb_steps, nb_units, t5, seed5)
    assert not np.array_equal(ref5[0], ref5[2]) and not np.array_equal(ref5[2], ref5[4])

    # hand-made rows on the large sample, the hand-made sample and an empty one
    hand = _hand_rows(nb_units)
    idx_h = [s for _ in hand for s in (1, n - 2, 0)]
    table_h = np.repeat(np.array([r for _, r in hand], np.float32), 3, axis=0)
    ref_h, _ = _check(store, samples, idx_h, nb_steps, nb_units, table_h, 99)
    placed = {name: float(ref_h[3 * i:3 * i + 3].sum()) for i, (name, _) in enumerate(hand)}
    for name in ("everything shifts out above", "time mask over the whole window", "band over all units"):
        assert placed[name] == 0, name
    assert placed["everything shifts out below"] == 1      # the hand-made sample's event at unit nb_units comes in
    assert placed["p = 0"] > 0 or nb_units == 1
    assert placed["p just below 1"] <= 1                                       # one uniform in 2^24 is not below it
    assert placed["stretched past max_time"] <= placed["an empty mask and an empty band"]
    if nb_units > 1 and placed["an empty mask and an empty band"] > 50:        # events all over the window
        assert placed["stretched past max_time"] < placed["an empty mask and an empty band"]

    if sort:   # the scan over the whole sample gives what the search on the transformed times gives
        store.sorted = False
        _check(store, samples, everyone, nb_steps, nb_units, table, seed)
        _check(store, samples, idx_h, nb_steps, nb_units, table_h, 99)


def test_column_slabs():
    """Rows wider than a tile: shifts carry events across column 16384 in both directions."""
    nb_units, nb_steps = 20000, 3
    t = np.array([0.1, 0.2, 0.69, 0.71, 0.9, 1.0, 1.3, 1.39, 0.5, 0.5], np.float32)
    u = np.array([16380, 16383, 16384, 16390, 0, 19999, 16383, 16384, 8000, 16384], np.int64)
    samples = [(t, u), (t[::2].copy(), u[::2].copy()), (np.zeros(0, np.float32), np.zeros(0, np.int64))]
    store = _store(samples, nb_units, MAX_TIME)
    rows = np.array([[0, 1, 0, 0, 0, 0, 0, 0],
                     [5, 1, 0, 0, 0, 0, 0, 0],              # 16380.. move over the boundary
                     [-7, 1, 0, 0, 0, 0, 0, 0],             # 16384.. move back under it
                     [3616, 0.75, 0.1, 0, 0, 0, 0, 0],      # 16384 -> 20000: out; 0 -> 3616
                     [-16384, 1.25, -0.05, 0, 0, 0, 0, 0],  # the upper slab lands at column 0, the lower one is out
                     [4, 1, 0, 0.5, 0, 0, 16384, 16390],    # a band right behind the boundary, half the events drawn out
                     [0, 1, 0, 0, 0.6, 0.8, 0, 0]], np.float32)
    idx = [0, 0, 0, 0, 0, 0, 1]
    ref, lost = _check(store, samples, idx, nb_steps, nb_units, rows, 3, plane=True, dense=True)
    assert ref[1][:, 16385].sum() == 1 and ref[2][:, 16377].sum() == 3 and ref[4][:, 0].sum() >= 1
    _check(store, samples, idx, nb_steps, nb_units, rows, 3, plane=True, dense=True, dropped=True)
    store.sorted = False
    _check(store, samples, idx, nb_steps, nb_units, rows, 3, plane=True, dense=True, dropped=True)


def test_bad_tables_are_refused_before_any_launch():
    from sparch_amd import functional as Fn

    ea = _ea()
    store = _store(_samples(np.random.default_rng(1), 100, 700, MAX_TIME, np.float32, 2, True), 700, MAX_TIME)
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    good = ea.identity_rows(2)

    def changed(field, value):
        t = good.copy()
        t[1, field] = value
        return t

    launches = []
    real = Fn.EventStore._launch
    Fn.EventStore._launch = lambda self, *a, **k: launches.append(1) or real(self, *a, **k)
    try:
        for bad in (changed(1, 0.0), changed(2, np.nan), changed(3, 1.0), changed(0, 0.5), changed(6, 0.5),
                    good[:1], good[:, :7], ea.identity_rows(3)):
            with pytest.raises(ValueError):
                store.gather(idx, 100, dense=True, augment=(bad, 1))
            with pytest.raises(ValueError):
                store.batch(idx, 100, augment=(bad, 1))
        with pytest.raises(ValueError):
            store.gather(idx, 100, dense=True, augment=good)                  # not a pair
        with pytest.raises(ValueError):
            store.gather(idx, 100, dense=True, augment=(good, -1))
        assert not launches
        store.gather(idx, 100, dense=True, augment=(good, 1))
        assert launches == [1]
    finally:
        Fn.EventStore._launch = real


def _epoch(loader):
    return [(_dense(x).cpu().numpy(), y.cpu().numpy()) for x, _, y in loader]


def _loader(h5, augment, split="train", **kw):
    from sparch_amd.dataloaders.spiking_datasets import load_shd_or_ssc

    kw.setdefault("shuffle", False)
    return load_shd_or_ssc("shd", "/unused", split, 4, h5_file=h5, device=DEV, resident="resident", augment=augment,
                           **kw)


def test_loader_epochs():
    from sparch_amd import functional as Fn

    ea = _ea()
    h5 = _fake_h5()
    spec = _spec(700)
    samples = list(zip(h5["spikes"]["times"], h5["spikes"]["units"]))
    a, b = _loader(h5, spec, augment_seed=7), _loader(h5, spec, augment_seed=7)
    for x, _, _ in a:
        assert Fn.input_plane_of(x) is not None                               # small counts: the plane is served
        break
    a.epoch_index = 0
    torch.manual_seed(3)
    ea0 = _epoch(a)
    state = torch.get_rng_state()
    torch.manual_seed(3)
    _epoch(_loader(h5, None))
    assert torch.equal(state, torch.get_rng_state())      # torch's generator: what an unaugmented epoch leaves
    ea1, eb0 = _epoch(a), _epoch(b)
    assert len(ea0) == 3 and [len(y) for _, y in ea0] == [4, 4, 3]
    for (x0, y0), (x1, y1), (x2, y2) in zip(ea0, eb0, ea1):
        assert np.array_equal(x0, x1) and np.array_equal(y0, y1)              # same seed, same epoch
        assert np.array_equal(y0, y2) and not np.array_equal(x0, x2)          # the second epoch is drawn anew
    other = _epoch(_loader(h5, spec, augment_seed=8))
    assert not np.array_equal(other[0][0], ea0[0][0])
    # the epochs against the restatement: the table of epoch e from default_rng([seed, rank, e]), a slice per batch
    for e, epoch in enumerate((ea0, ea1)):
        table, seed = ea.draw_event_augmentation(11, spec, np.random.default_rng([7, 0, e]), 700, MAX_TIME)
        at = 0
        for x, y in epoch:
            idx = list(range(at, at + len(y)))
            ref, _ = evaug.bin_batch_augmented(samples, idx, table[at:at + len(y)], seed, 100, 700, MAX_TIME)
            assert np.array_equal(x, ref) and y.tolist() == [int(h5["labels"][s]) for s in idx]
            at += len(y)
    # loaders without a spec (what valid and test get) serve the unaugmented batches
    for split in ("valid", "test"):
        plain = _epoch(_loader(h5, None, split=split))
        for b0, (x, y) in enumerate(plain):
            for k in range(len(y)):
                assert np.array_equal(x[k], ev.bin_sample(*samples[4 * b0 + k])[0])


def test_loader_serves_values_and_falls_back_to_fp32():
    from sparch_amd import functional as Fn

    ea = _ea()
    h5 = _fake_h5()
    t = np.concatenate([np.asarray(h5["spikes"]["times"][1]), np.full(3, 0.5, np.float32)])
    u = np.concatenate([np.asarray(h5["spikes"]["units"][1]), np.full(3, 123, np.int32)])
    o = np.argsort(t, kind="stable")
    h5["spikes"]["times"][1], h5["spikes"]["units"][1] = t[o], u[o]
    samples = list(zip(h5["spikes"]["times"], h5["spikes"]["units"]))
    for spec, values, plane in ((_spec(700), True, False), ("scale=0.995,drop=0.1", False, False),
                                ("scale=0.5,drop=0.1", False, True)):
        loader = _loader(h5, spec, values=values, augment_seed=2)
        top = loader.store.prepare(100)
        scale = ea.parse_event_augment(spec)["scale"]
        assert top >= 3 and (top * ea.plane_count_factor(scale) <= 255) == (plane or values)
        assert loader.store.serves_plane(100, scale) == (plane or values)
        table, seed = ea.draw_event_augmentation(11, spec, np.random.default_rng([2, 0, 0]), 700, MAX_TIME)
        at = 0
        for x, xlens, y in loader:
            assert (Fn.input_plane_of(x) is not None) == plane
            if not plane:
                assert x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (len(y), 100, 700)
            idx = list(range(at, at + len(y)))
            ref, _ = evaug.bin_batch_augmented(samples, idx, table[at:at + len(y)], seed, 100, 700, MAX_TIME)
            assert np.array_equal(_dense(x).cpu().numpy(), ref)
            at += len(y)
        assert at == 11


def _run_exp(tmp_path, env_extra, unset=()):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pack_events

    data = tmp_path / "shd"
    data.mkdir()
    pack_events.pack_mapping(_fake_h5(n=22, seed=1, tdtype=np.float16), str(data / "shd_train.events.npz"))
    pack_events.pack_mapping(_fake_h5(n=9, seed=2, tdtype=np.float16), str(data / "shd_test.events.npz"))
    exp = tmp_path / "exp"
    env = {k: v for k, v in os.environ.items() if k not in unset}
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_exp.py"), "--dataset_name", "shd", "--data_folder",
                        str(data), "--nb_epochs", "1", "--model_type", "RadLIF", "--nb_hiddens", "64", "--batch_size",
                        "4", "--use_augm", "1", "--log_tofile", "1", "--new_exp_folder", str(exp)],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    return r, exp


def test_run_exp_with_event_augmentation(tmp_path):
    r, exp = _run_exp(tmp_path, dict(SPARCH_EVENTS="resident", SPARCH_EVENTS_AUGMENT=_spec(700)))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    log = (exp / "log" / "exp.log").read_text()
    for line in ("Events of the train set are resident", "Events of the train set are augmented on the device",
                 "\nData augmentation is used\n", "Epoch 1: train loss=", "Epoch 1: valid acc=", "Test acc="):
        assert line in log, line
    assert "not implemented for SHD" not in log
    assert log.count("are augmented on the device") == 1                      # the train loader alone
    train = [float(v) for v in re.findall(r"Epoch \d+: train loss=(\S+)", log)]
    assert len(train) == 1 and np.isfinite(train[0])
    assert "nan" not in log.lower()


def test_run_exp_refuses_augmentation_without_the_resident_store(tmp_path):
    r, _ = _run_exp(tmp_path, dict(SPARCH_EVENTS_AUGMENT="drop=0.1"), unset=("SPARCH_EVENTS",))
    assert r.returncode != 0
    assert "ValueError" in r.stderr and "SPARCH_EVENTS=resident" in r.stderr and "SPARCH_EVENTS_AUGMENT" in r.stderr
