"""GPU: the resident SHD / SSC event store.  `sparch_events_gather_bin` (events.hip) against the NumPy statement of
the reference's binning (oracle/events_numpy.py::bin_sample), exact equality; the resident loader against the
per-sample loader batch by batch; the network on a resident batch against the network on the fp32 batch; run_exp.py
on packs with SPARCH_EVENTS=resident."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import events_numpy as ev
from tests.event_cases import dense as _dense
from tests.event_cases import fake_h5 as _fake_h5
from tests.event_cases import samples as _samples
from tests.event_cases import store as _store
from tests.kit import DEV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(store, samples, idx, nb_steps, nb_units, max_time):
    got = store.gather(torch.as_tensor(idx, dtype=torch.int64).to(DEV), nb_steps, plane=True, dense=True, counts=True,
                       dropped=True)
    torch.cuda.synchronize()
    B, ldp = len(idx), (nb_units + 7) // 8 * 8
    ref = np.zeros((B, nb_steps, nb_units), np.float32)
    lost = 0
    for b, s in enumerate(idx):
        ref[b], nd = ev.bin_sample(samples[s][0], samples[s][1], nb_steps, nb_units, max_time)
        lost += nd
    assert np.array_equal(got["dense"].cpu().numpy(), ref)
    assert np.array_equal(got["counts"].cpu().numpy(), np.minimum(ref, 255).astype(np.uint8))
    plane = got["plane"]
    assert tuple(plane.shape) == (B * nb_steps, ldp) and plane.dtype == torch.bfloat16
    p = plane.view(B, nb_steps, ldp)
    assert ref.max() <= 256                                                          # exact in bf16
    assert np.array_equal(p[:, :, :nb_units].float().cpu().numpy(), ref)
    assert int(p[:, :, nb_units:].contiguous().view(torch.int16).abs().max() if ldp > nb_units else 0) == 0
    assert int(got["n_dropped"].item()) == lost
    assert got["y"].cpu().tolist() == [3 * s for s in idx]
    return ref, lost


@pytest.mark.parametrize("sort", [True, False])
@pytest.mark.parametrize("tdtype", [np.float16, np.float32])
@pytest.mark.parametrize("nb_units", [1, 700, 701])
@pytest.mark.parametrize("nb_steps", [2, 100, 250])
def test_kernel_equals_the_oracle(nb_steps, nb_units, tdtype, sort):
    rng = np.random.default_rng(nb_steps * 1000 + nb_units)
    max_time = 1.4
    samples = _samples(rng, nb_steps, nb_units, max_time, tdtype, n_random=6, sort=sort)
    if nb_units == 1:   # one unit: keep every bin count exact in bf16 (<= 256) for the plane comparison
        samples = [(t[:150], u[:150]) if len(t) > 150 and nb_steps > 2 else (t[:100], u[:100]) for t, u in samples]
    store = _store(samples, nb_units, max_time)
    assert store.sorted == sort and store.times_dtype == (1 if tdtype == np.float16 else 0)
    n = len(samples)
    ref, lost = _check(store, samples, list(range(n)), nb_steps, nb_units, max_time)
    assert lost >= 6                                                                 # the hand-made sample's rejects
    _check(store, samples, [n - 2], nb_steps, nb_units, max_time)                    # B = 1
    _check(store, samples, [1, n - 2, 1, 0, 1], nb_steps, nb_units, max_time)        # a repeated index
    if sort:   # the scan over the whole sample gives what the search gives
        store.sorted = False
        _check(store, samples, list(range(n)), nb_steps, nb_units, max_time)


@pytest.mark.parametrize("sort", [True, False])
def test_kernel_at_batch_256(sort):
    rng = np.random.default_rng(7)
    samples = _samples(rng, 100, 700, 1.4, np.float16, n_random=40, sort=sort)
    store = _store(samples, 700, 1.4)
    idx = rng.integers(0, len(samples), 256).tolist()
    _check(store, samples, idx, 100, 700, 1.4)
    _check(store, samples, idx, 250, 700, 1.4)
    # the whole store, as prepare() walks it: largest count and rejected events
    refs = [ev.bin_sample(t, u, 100, 700, 1.4) for t, u in samples]
    assert store.prepare(100) == int(max(r[0].max() for r in refs))
    assert store.dropped(100) == sum(r[1] for r in refs)


def test_argument_checks():
    from sparch_amd import functional as Fn
    from sparch_amd._capi import lib

    store = _store(_samples(np.random.default_rng(1), 100, 700, 1.4, np.float32, 2, True), 700, 1.4)
    idx = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        store.gather(idx, 100)                                       # no output asked for
    with pytest.raises(ValueError):
        store.gather(idx.int(), 100, dense=True)
    with pytest.raises(ValueError):
        store.gather(idx, 1, dense=True)                             # nb_steps < 2: refused by the library
    with pytest.raises(ValueError):
        Fn.EventStore(Fn.event_arrays_from_mapping({"spikes": {"times": [[0.1]], "units": [[1]]}, "labels": [0]}),
                      device=DEV, nb_units=65536)
    assert lib.sparch_events_gather_bin_workspace_bytes(256, 100, 700) == 256 * 4 * 4
    assert lib.sparch_events_gather_bin_workspace_bytes(256, 250, 700) == 256 * 9 * 4
    assert lib.sparch_events_gather_bin_workspace_bytes(256, 100, 65536) == 0
    # an index outside the store: an empty sample with label -1, nothing read out of bounds
    got = store.gather(torch.tensor([1, 99, -1], dtype=torch.int64, device=DEV), 100, dense=True)
    assert got["y"].cpu().tolist()[1:] == [-1, -1] and float(got["dense"][1:].abs().sum()) == 0.0


@pytest.mark.parametrize("tdtype", [np.float16, np.float32])
@pytest.mark.parametrize("shuffle", [False, True])
def test_resident_loader_equals_the_per_sample_loader(shuffle, tdtype):
    from sparch_amd import functional as Fn
    from sparch_amd.dataloaders.spiking_datasets import ResidentEventLoader, load_shd_or_ssc

    h5 = _fake_h5(tdtype=tdtype)
    batches = []
    for resident in ("", "resident"):
        loader = load_shd_or_ssc("shd", "/unused", "train", 4, shuffle=shuffle, h5_file=h5, device=DEV,
                                 resident=resident)
        assert isinstance(loader, ResidentEventLoader) == (resident == "resident")
        assert len(loader) == 3
        torch.manual_seed(11)
        got = []
        for x, xlens, y in loader:
            assert x.is_cuda and tuple(x.shape) == (len(xlens), 100, 700)
            if resident:
                assert y.is_cuda and Fn.input_plane_of(x) is not None       # counts <= 255: the plane is served
            got.append((_dense(x).cpu(), xlens, y.cpu()))
        batches.append((got, torch.get_rng_state()))
    (today, rng_t), (res, rng_r) = batches
    assert len(today) == len(res) == 3 and len(res[-1][2]) == 3               # 11 samples: 4 + 4 + 3
    for (x0, l0, y0), (x1, l1, y1) in zip(today, res):
        assert torch.equal(x0, x1) and torch.equal(l0, l1) and l0.dtype == l1.dtype and torch.equal(y0, y1)
    assert torch.equal(rng_t, rng_r)
    # against the oracle too
    x, _, y = res[0]
    if not shuffle:
        for b in range(4):
            assert np.array_equal(x[b].numpy(), ev.bin_sample(h5["spikes"]["times"][b], h5["spikes"]["units"][b])[0])


def test_values_are_served_as_fp32_on_request():
    from sparch_amd import functional as Fn
    from sparch_amd.dataloaders.spiking_datasets import load_shd_or_ssc

    h5 = _fake_h5()
    loader = load_shd_or_ssc("shd", "/unused", "train", 4, shuffle=False, h5_file=h5, device=DEV, resident="resident",
                             values=True)
    x, _, _ = next(iter(loader))
    assert Fn.input_plane_of(x) is None and x.dtype == torch.float32 and x.is_contiguous()
    assert np.array_equal(x[2].cpu().numpy(), ev.bin_sample(h5["spikes"]["times"][2], h5["spikes"]["units"][2])[0])


def test_a_bin_above_255_is_served_as_fp32():
    from sparch_amd import functional as Fn
    from sparch_amd.dataloaders.spiking_datasets import load_shd_or_ssc

    h5 = _fake_h5()
    t = np.concatenate([np.asarray(h5["spikes"]["times"][1]), np.full(300, 0.5, np.float32)])
    u = np.concatenate([np.asarray(h5["spikes"]["units"][1]), np.full(300, 123, np.int32)])
    o = np.argsort(t, kind="stable")
    h5["spikes"]["times"][1], h5["spikes"]["units"][1] = t[o], u[o]
    loader = load_shd_or_ssc("shd", "/unused", "train", 4, shuffle=False, h5_file=h5, device=DEV, resident="resident")
    assert loader.store.prepare(100) >= 300 and not loader.store.serves_plane(100)
    seen = 0
    for x, xlens, y in loader:
        assert Fn.input_plane_of(x) is None and x.dtype == torch.float32
        for b in range(len(xlens)):
            ref, _ = ev.bin_sample(h5["spikes"]["times"][seen], h5["spikes"]["units"][seen])
            assert np.array_equal(x[b].cpu().numpy(), ref)
            assert int(y[b]) == int(h5["labels"][seen])
            seen += 1
    assert seen == 11 and ref.max() <= 255
    assert float(ev.bin_sample(h5["spikes"]["times"][1], h5["spikes"]["units"][1])[0].max()) >= 300


def test_network_on_a_resident_batch_equals_the_fp32_batch():
    import sparch_amd
    from sparch_amd import functional as Fn
    from sparch_amd.dataloaders.spiking_datasets import load_shd_or_ssc

    h5 = _fake_h5()
    xs = []
    for resident in ("", "resident"):
        loader = load_shd_or_ssc("shd", "/unused", "train", 8, shuffle=False, h5_file=h5, device=DEV,
                                 resident=resident)
        x, _, y = next(iter(loader))
        xs.append((x, y.to(DEV)))
    assert Fn.input_plane_of(xs[0][0]) is None and Fn.input_plane_of(xs[1][0]) is not None
    torch.manual_seed(2)
    net = sparch_amd.SNN((8, None, 700), [64, 48, 20], neuron_type="RadLIF", dropout=0.0).to(DEV).train()
    res = []
    for x, y in xs:
        net.zero_grad()
        torch.manual_seed(5)
        out, rates = net(x)
        torch.nn.functional.cross_entropy(out, y).backward()
        Fn.check_status()
        res.append((out.detach().clone(), rates.detach().clone(),
                    {k: v.grad.clone() for k, v in net.named_parameters()}))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].sum()) > 0
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k


@pytest.mark.parametrize("model_type,served", [("RadLIF", "bf16 plane"), ("MLP", "dense fp32")])
def test_run_exp_on_packs(tmp_path, model_type, served):
    """run_exp.py --dataset_name shd without --synthetic on a machine without h5py: the packs are the way in.  A
    spiking network is fed the plane, a non-spiking one the values."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pack_events

    data = tmp_path / "shd"
    data.mkdir()
    # 22 samples in batches of 4: a ragged last batch of TWO.  (A last batch of one sample gives the MLP's readout
    # BatchNorm a single value per channel, which nn.BatchNorm1d refuses in training and sparch_bn_finalize now refuses
    # as well; it used to write a non-finite running variance, and the evaluation behind it printed NaN.)
    pack_events.pack_mapping(_fake_h5(n=22, seed=1, tdtype=np.float16), str(data / "shd_train.events.npz"))
    pack_events.pack_mapping(_fake_h5(n=9, seed=2, tdtype=np.float16), str(data / "shd_test.events.npz"))
    exp = tmp_path / "exp"
    env = dict(os.environ, SPARCH_EVENTS="resident")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_exp.py"), "--dataset_name", "shd", "--data_folder",
                        str(data), "--nb_epochs", "2", "--model_type", model_type, "--nb_hiddens", "64", "--batch_size",
                        "4", "--log_tofile", "1", "--new_exp_folder", str(exp)],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    log = (exp / "log" / "exp.log").read_text()
    for line in ("Events of the train set are resident", served, "Epoch 1: train loss=", "Epoch 2: train loss=",
                 "Epoch 2: valid acc=", "Test acc="):
        assert line in log, line
    train = [float(v) for v in re.findall(r"Epoch \d+: train loss=(\S+)", log)]
    assert len(train) == 2 and all(np.isfinite(train))
    assert "nan" not in log.lower()
    assert ("bf16 plane" in log) == (served == "bf16 plane")
