"""
Streaming inference for the non-spiking baselines on the device: sparch_amd.StreamingANN and the two entry points of
sparch_amd/csrc/streamann.hip (sparch_ann_stream_step, sparch_ann_stream_readout).

  1  reference-pinned   the unidirectional ANN fixtures streamed in chunks of 1 against the real reference's eval-mode
                        output, at the bars the whole-sequence eval forward is held to (test_hip_parity.py: 1e-3 with
                        the readout, 2e-4 without); eager and graph=True (both parities captured and replayed, bit-equal
                        to the eager stream); the bidirectional fixture is refused
  2  chunking           chunks [7, 1, T-8] and one whole chunk: out and get_state() bit-equal to chunks of 1
  3  state              set_state(get_state()) and refresh() behind an odd number of steps change nothing; reset(rows=)
                        mid-stream restarts those rows and leaves the others alone, bit for bit
  4  kernel geometries  at the C ABI in guarded buffers (tests/guarded.embed), 6 free-running steps from a zero state,
                        every cell (the RNN with all three activations), against the fp64 restatement
                        tests/stream_ann_numpy.py
  5  readout alone      the same (B,K) with C in {1, 20, 35, 256}, all three norms
  6  launch count       one eager step is hidden layers (x 2 for the GRU) + 1 C-ABI calls; a LayerNorm layer adds its
                        GEMM and sparch_layernorm_fwd per gate

Bounds of 4 and 5 (the convention of tests/test_gated_kernels_gpu.py): |got - ref64| <= bound per element, one bound
per output tensor: FOUR times the larger of the worst absolute errors of two fp32 runs of the restatement on the same
inputs (numpy's matmul; K accumulated in chunks of 32) against its fp64 run, floored at 4 * 2^-24 * max|ref| (a
yardstick below one rounding of the tensor's largest value only says that the two numpy runs rounded alike).  The bound
is computed here from the references alone; each test records the worst fraction it saw (DESIGN.md has the table).

Every shape and pointer a kernel receives is valid.
"""
import ctypes
import functools
import json

import numpy as np
import pytest
import torch

from tests import stream_ann_numpy as sn
from tests.golden_io import load
from tests.guarded import embed
from tests.kit import DEV, F32, F64, D, N, nan_, ptr, relmax, same_bits, within

pytestmark = pytest.mark.gpu

FIXTURES = ["ann_MLP_bn", "ann_RNN_bn", "ann_LiGRU_bn", "ann_GRU_bn", "ann_MLP_ln_bias_noreadout"]
STEPS = 6


# ====================================================================================================== networks
@functools.lru_cache(maxsize=None)
def fixture(name):
    """(cfg, z, net on the device in eval mode with the reference's running statistics after its training step)."""
    from sparch_amd.anns import ANN

    z = load(name)
    cfg = json.loads(str(z["cfg"]))
    net = ANN(input_shape=(cfg["B"], None, cfg["C"]), layer_sizes=cfg["layer_sizes"], ann_type=cfg["ann_type"],
              dropout=0.0, normalization=cfg["normalization"], use_bias=cfg["use_bias"],
              bidirectional=cfg["bidirectional"], use_readout_layer=cfg["use_readout_layer"])
    sd = {k[len("param."):]: torch.from_numpy(v) for k, v in z.items() if k.startswith("param.")}
    sd.update({k[len("after."):]: torch.from_numpy(v) for k, v in z.items() if k.startswith("after.")})
    net.load_state_dict(sd)
    return cfg, z, net.to(DEV).eval()


def run_stream(st, x, cuts):
    """Feeds x (B,T,C) in chunks of the given lengths; returns the last `out` (readout) or all outputs (B,T,H), cloned."""
    outs, t0 = [], 0
    for n in cuts:
        outs.append(st.step(x[:, t0:t0 + n]).clone())
        t0 += n
    assert t0 == x.shape[1]
    return outs[-1] if st.net.use_readout_layer else torch.cat(outs, dim=1)


@functools.lru_cache(maxsize=None)
def eager_ones(name):
    """The stream in chunks of 1, eager, from a reset: (out, state) — what the other tests compare with (never written)."""
    import sparch_amd
    cfg, z, net = fixture(name)
    st = sparch_amd.StreamingANN(net, cfg["B"])
    st.reset()
    out = run_stream(st, torch.from_numpy(z["x"]).to(DEV), [1] * cfg["T"])
    assert st.steps_seen == cfg["T"] and st.row_steps.tolist() == [cfg["T"]] * cfg["B"]
    return out, st.get_state()


def states_equal(a, b):
    return len(a) == len(b) and all(sorted(p) == sorted(q) and all(same_bits(p[k], q[k]) for k in p) for p, q in zip(a, b))


# ====================================================================================================== 1. reference-pinned
@pytest.mark.parametrize("name", FIXTURES)
def test_stream_in_chunks_of_one_matches_the_reference_eval_output(name, record_property):
    import sparch_amd
    cfg, z, net = fixture(name)
    tol = 1e-3 if cfg["use_readout_layer"] else 2e-4
    out, _ = eager_ones(name)
    err = relmax(N(out), z["out_eval"])
    record_property("relmax_vs_out_eval", err)
    print(f"{name}: relmax {err:.3e} (bar {tol:.0e})")
    assert out.shape == z["out_eval"].shape and err <= tol
    # the same stream replayed from captured graphs: one per buffer parity, bit-equal to the eager launches
    st = sparch_amd.StreamingANN(net, cfg["B"], graph=True)
    st.reset()
    got = run_stream(st, torch.from_numpy(z["x"]).to(DEV), [1] * cfg["T"])
    assert sorted(st._g) == [0, 1], "both parities captured"
    assert all(g["replays"] >= 2 for g in st._g.values()), {k: g["replays"] for k, g in st._g.items()}
    assert sum(g["replays"] for g in st._g.values()) == cfg["T"] - 1      # one eager step before the capture
    assert same_bits(got, out), "the replayed stream differs from the eager one"
    assert states_equal(st.get_state(), eager_ones(name)[1])


def test_bidirectional_fixture_is_refused():
    import sparch_amd
    cfg, _, net = fixture("ann_RNN_bidir")
    with pytest.raises(ValueError, match="not causal"):
        sparch_amd.StreamingANN(net, cfg["B"])


# ====================================================================================================== 2. chunking
@pytest.mark.parametrize("name", FIXTURES)
def test_any_chunking_gives_the_same_bits(name):
    import sparch_amd
    cfg, z, net = fixture(name)
    T = cfg["T"]
    x = torch.from_numpy(z["x"]).to(DEV)
    want, want_state = eager_ones(name)
    for cuts in ([7, 1, T - 8], [T]):
        st = sparch_amd.StreamingANN(net, cfg["B"])
        st.reset()
        got = run_stream(st, x, cuts)
        assert same_bits(got, want), cuts
        assert states_equal(st.get_state(), want_state), cuts
        assert st.steps_seen == T


# ====================================================================================================== 3. state
@pytest.mark.parametrize("name", ["ann_RNN_bn", "ann_GRU_bn", "ann_MLP_bn"])
def test_state_round_trip_and_refresh_behind_an_odd_number_of_steps(name):
    import sparch_amd
    cfg, z, net = fixture(name)
    T = cfg["T"]
    x = torch.from_numpy(z["x"]).to(DEV)
    want, want_state = eager_ones(name)
    st = sparch_amd.StreamingANN(net, cfg["B"])
    st.reset()
    st.step(x[:, :5])                                        # an odd number: the second copy of y is the current one
    st.set_state(st.get_state())
    st.step(x[:, 5:8])
    st.refresh()
    got = st.step(x[:, 8:])
    assert st.steps_seen == T
    assert same_bits(got, want) and states_equal(st.get_state(), want_state)
    other = sparch_amd.StreamingANN(net, cfg["B"])           # a state moves to another stream object
    other.reset()
    other.step(x[:, :5])
    mid = other.get_state()
    fresh = sparch_amd.StreamingANN(net, cfg["B"])
    fresh.reset(states=mid)
    assert same_bits(fresh.step(x[:, 5:]), want)


@pytest.mark.parametrize("name", ["ann_LiGRU_bn", "ann_GRU_bn"])
def test_reset_of_some_rows_mid_stream(name):
    import sparch_amd
    cfg, z, net = fixture(name)
    B, T = cfg["B"], cfg["T"]
    assert B >= 4
    x = torch.from_numpy(z["x"]).to(DEV)
    cut, rows, others = 9, [1, 3], [b for b in range(B) if b not in (1, 3)]
    st = sparch_amd.StreamingANN(net, B)
    st.reset()
    st.step(x[:, :cut])
    st.reset(rows=rows)
    assert st.row_steps.tolist() == [0 if b in rows else cut for b in range(B)] and st.steps_seen == cut
    got = st.step(x[:, cut:])
    fresh = sparch_amd.StreamingANN(net, B)                  # the same batch size, fed the same inputs from the restart on
    fresh.reset()
    restart = fresh.step(x[:, cut:])
    want, want_state = eager_ones(name)
    assert same_bits(got[rows], restart[rows]), "the restarted rows differ from a fresh stream"
    assert same_bits(got[others], want[others]), "the other rows were disturbed"
    for a, f, w in zip(st.get_state(), fresh.get_state(), want_state):
        for k in a:
            assert same_bits(a[k][rows], f[k][rows]) and same_bits(a[k][others], w[k][others]), k


# ====================================================================================================== 4. kernel geometries
SHAPES = [(1, 3, 5), (3, 40, 32), (17, 70, 36), (2, 1100, 8), (5, 256, 256), (9, 1024, 1024)]
SHAPE_IDS = ["b1_k3_h5", "b3_k40_h32", "b17_k70_h36", "b2_k1100_h8", "b5_k256_h256", "b9_k1024_h1024"]
CELLS = [("MLP", "sigmoid"), ("RNN", "sigmoid"), ("RNN", "relu"), ("RNN", "tanh"), ("LiGRU", None), ("GRU", None)]
CELL_IDS = ["mlp", "rnn_sigmoid", "rnn_relu", "rnn_tanh", "ligru", "gru"]
CELL_CODE = {"MLP": 0, "RNN": 1, "LiGRU": 2, "GRU": 3}
ACT_CODE = {"sigmoid": 0, "relu": 1, "tanh": 2, None: 0}
SLOT = {"c": 0, "z": 1, "r": 2}


def strides(B, K, H):
    """(ld, ldx): the crossing shape runs with row strides that are no multiple of 4."""
    return (H + 2, K + 1) if (B, K, H) == (17, 70, 36) else (H, K)


def bound_of(ref, runs):
    """FOUR times the worst error of the fp32 runs against the fp64 one, floored at 4 * 2^-24 * max|ref|."""
    worst = max(float(np.abs(r.astype(F64) - ref).max()) for r in runs)
    return max(4.0 * worst, 4.0 * 2.0 ** -24 * float(np.abs(ref).max()))


@functools.lru_cache(maxsize=4)
def step_case(cell, act, B, K, H):
    """Inputs and the three free-running reference runs of one case (never written to)."""
    rng = np.random.default_rng(1000003 * B + 1009 * K + 31 * H + len(cell) + 7 * ACT_CODE[act])
    f = lambda a: np.ascontiguousarray(a, dtype=F32)  # noqa: E731
    gates = {}
    for g in sn.GATES[cell]:
        gates[g] = dict(W=f(rng.standard_normal((H, K)) * (0.5 / np.sqrt(K))), bias=f(rng.standard_normal(H) * 0.1),
                        scale=f(rng.uniform(0.7, 1.3, H)), shift=f(rng.uniform(-0.2, 0.2, H)),
                        V=None if cell == "MLP" else f(rng.standard_normal((H, H)) * (0.5 / np.sqrt(H))))
    xs = f(rng.standard_normal((STEPS, B, K)))
    runs = []
    for dt, mm in ((F64, np.matmul), (F32, np.matmul), (F32, sn.matmul_chunked)):
        y, ys = np.zeros((B, H), dt), []
        for t in range(STEPS):
            y = sn.hidden_step(cell, xs[t], y, gates, act or "sigmoid", dt, mm)["y"]
            ys.append(y)
        runs.append(np.stack(ys))
    return gates, xs, runs[0], bound_of(runs[0], runs[1:])


@pytest.mark.parametrize("B,K,H", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("cell,act", CELLS, ids=CELL_IDS)
def test_step_kernel_geometries_against_fp64(cell, act, B, K, H, record_property):
    """(1,3,5): scalar loads, one row, a ragged column group.  (3,40,32): RT = 4 with a ragged tile, 16-byte loads.
    (17,70,36): a second 16-row tile of one row, scalar loads, row strides 38 and 71.  (2,1100,8): K beyond one staged
    piece of 1024.  (5,256,256): RT = 8.  (9,1024,1024): the headline layer, RT = 16, two pieces per operand."""
    from sparch_amd._capi import lib
    gates, xs, ref, bound = step_case(cell, act, B, K, H)
    ld, ldx = strides(B, K, H)
    rec, gru = cell != "MLP", cell == "GRU"
    arr = ctypes.c_void_p * 3
    dev = {g: {k: (None if v is None else embed(D(v, F32).view(1, -1) if v.ndim == 1 else D(v, F32)))
               for k, v in gates[g].items()} for g in gates}
    slots = lambda k: arr(*[ptr(dev[g][k]) if g in dev else None for g in ("c", "z", "r")])  # noqa: E731
    x_dev = [embed(D(xs[t], F32), ldx, 0) for t in range(STEPS)]
    y = [embed(torch.zeros(B, H, device=DEV), ld, 0), embed(nan_(B, H), ld, 0)]      # the zero state, the other copy
    z, ry = (embed(nan_(B, H), ld, 0), embed(nan_(B, H), ld, 0)) if gru else (None, None)
    got = []
    for t in range(STEPS):
        y_in, y_out = y[t & 1], y[(t + 1) & 1]
        for phase in ((1, 2) if gru else (0,)):
            rc = lib.sparch_ann_stream_step(CELL_CODE[cell], phase, ACT_CODE[act], B, K, H, ld, ptr(x_dev[t]), ldx,
                                            slots("W"), slots("bias"), slots("scale"), slots("shift"), None,
                                            slots("V") if rec else None, ptr(y_in) if rec else None,
                                            None if phase == 1 else ptr(y_out), ptr(z), ptr(ry), None)
            assert rc == 0, (rc, t, phase)
        got.append(N(y_out).copy())
    got = np.stack(got)
    what = f"{cell} {act or ''} (B {B}, K {K}, H {H})"
    f = within(got, ref, bound, what)
    record_property("y_err_over_bound", f)
    record_property("bound", bound)
    print(f"{what}: y {f:.3f} of the bound {bound:.3e}")
    for name, t in [("y0", y[0]), ("y1", y[1]), ("z", z), ("ry", ry)] + [(f"x{i}", v) for i, v in enumerate(x_dev)] + \
            [(f"{g}.{k}", v) for g in dev for k, v in dev[g].items()]:
        if t is not None:
            assert not bool(torch.isnan(t).any()), f"{what}: NaN left in {name}"
            t.check(f"{what}: {name}")                                        # guards and padding columns untouched


def test_step_with_ready_made_projections_equals_the_one_launch_form():
    """x == NULL: the projections come from `pre` (the LayerNorm route).  With pre? = the affine projection computed
    in fp64 and rounded once, the kernel's output stays within the one-launch form's bound of the fp64 cell."""
    from sparch_amd._capi import lib
    B, K, H = 3, 40, 32
    gates, xs, _, _ = step_case("GRU", None, B, K, H)
    arr = ctypes.c_void_p * 3
    order = ("c", "z", "r")
    pre64 = {g: sn.projection(xs[0], gates[g], F64, np.matmul) for g in order}
    y0 = np.random.default_rng(5).uniform(-1, 1, (B, H)).astype(F32)
    ready = {g: dict(W=np.zeros((H, 1), F32), V=gates[g]["V"], bias=pre64[g].astype(F32)) for g in order}
    runs = []                                                    # x = 0 and bias = pre: the cell on a given projection
    for dt, mm in ((F64, np.matmul), (F32, np.matmul), (F32, sn.matmul_chunked)):
        runs.append(sn.hidden_step("GRU", np.zeros((B, 1), F32), y0, ready, "sigmoid", dt, mm)["y"])
    pre = {g: embed(D(pre64[g], F32)) for g in order}
    V = {g: embed(D(gates[g]["V"], F32)) for g in order}
    y_in, y_out, z, ry = embed(D(y0, F32)), embed(nan_(B, H)), embed(nan_(B, H)), embed(nan_(B, H))
    for phase in (1, 2):
        rc = lib.sparch_ann_stream_step(3, phase, 0, B, K, H, H, None, 0, None, None, None, None,
                                        arr(*[ptr(pre[g]) for g in order]), arr(*[ptr(V[g]) for g in order]), ptr(y_in),
                                        None if phase == 1 else ptr(y_out), ptr(z), ptr(ry), None)
        assert rc == 0
    within(N(y_out), runs[0], bound_of(runs[0], runs[1:]), "GRU on ready-made projections")
    for t in (y_in, y_out, z, ry, *pre.values(), *V.values()):
        assert not bool(torch.isnan(t).any())
        t.check("ready-made projections")


# ====================================================================================================== 5. readout alone
CLASSES = (1, 20, 35, 256)
NORM_CODE = {"none": 0, "affine": 1, "layernorm": 2}


@functools.lru_cache(maxsize=4)
def readout_case(B, K, C, norm):
    rng = np.random.default_rng(7919 * B + 31 * K + C + len(norm))
    f = lambda a: np.ascontiguousarray(a, dtype=F32)  # noqa: E731
    W, bias = f(rng.standard_normal((C, K)) * (0.5 / np.sqrt(K))), f(rng.standard_normal(C) * 0.1)
    p0, p1 = (None, None) if norm == "none" else (f(rng.uniform(0.7, 1.3, C)), f(rng.uniform(-0.2, 0.2, C)))
    ys = f(rng.standard_normal((STEPS, B, K)))
    runs = []
    for dt, mm in ((F64, np.matmul), (F32, np.matmul), (F32, sn.matmul_chunked)):
        acc, outs = np.zeros((B, K), dt), []
        for t in range(STEPS):
            acc, out = sn.readout_step(ys[t], acc, W, bias, norm, p0, p1, dt, mm)
            outs.append(out)
        runs.append((np.stack(outs), acc))
    return (W, bias, p0, p1, ys, runs[0][0], runs[0][1], bound_of(runs[0][0], [r[0] for r in runs[1:]]),
            bound_of(runs[0][1], [r[1] for r in runs[1:]]))


@pytest.mark.parametrize("norm", ["none", "affine", "layernorm"])
@pytest.mark.parametrize("B,K,H", SHAPES, ids=SHAPE_IDS)
def test_readout_kernel_against_fp64(B, K, H, norm, record_property):
    from sparch_amd._capi import lib
    ldy = strides(B, K, H)[1]
    worst = 0.0
    for C in CLASSES:
        W, bias, p0, p1, ys, ref_out, ref_acc, b_out, b_acc = readout_case(B, K, C, norm)
        row = lambda v: None if v is None else embed(D(v, F32).view(1, -1))  # noqa: E731
        Wd, bd, p0d, p1d = embed(D(W, F32)), row(bias), row(p0), row(p1)
        y_dev = [embed(D(ys[t], F32), ldy, 0) for t in range(STEPS)]
        acc, out = embed(torch.zeros(B, K, device=DEV)), embed(nan_(B, C))
        outs = []
        for t in range(STEPS):
            rc = lib.sparch_ann_stream_readout(B, K, C, ptr(y_dev[t]), ldy, ptr(acc), ptr(Wd), ptr(bd), NORM_CODE[norm],
                                               ptr(p0d), ptr(p1d), 1e-5, ptr(out), None)
            assert rc == 0, (rc, t)
            outs.append(N(out).copy())
        what = f"readout {norm} (B {B}, K {K}, C {C})"
        f_out = within(np.stack(outs), ref_out, b_out, f"{what}: out")
        f_acc = within(N(acc), ref_acc, b_acc, f"{what}: acc")
        np.testing.assert_allclose(N(acc).sum(axis=1), STEPS, rtol=1e-4, err_msg=f"{what}: acc rows sum to the step count")
        worst = max(worst, f_out, f_acc)
        print(f"{what}: out {f_out:.3f} of {b_out:.3e}, acc {f_acc:.3f} of {b_acc:.3e}")
        for name, t in [("acc", acc), ("out", out), ("W", Wd), ("bias", bd), ("p0", p0d), ("p1", p1d)] + \
                [(f"y{i}", v) for i, v in enumerate(y_dev)]:
            if t is not None:
                assert not bool(torch.isnan(t).any()), f"{what}: NaN left in {name}"
                t.check(f"{what}: {name}")
    record_property("err_over_bound", worst)


# ====================================================================================================== 6. launch count
class CountingLib:
    """The library with every sparch_* call counted by name (host side; nothing about the device)."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("sparch_"):
            return fn

        def counted(*a):
            self.calls.append(name)
            return fn(*a)
        return counted


def count_one_step(monkeypatch, name):
    import sparch_amd
    from sparch_amd import functional as Fn
    from sparch_amd import streaming_ann
    cfg, z, net = fixture(name)
    st = sparch_amd.StreamingANN(net, cfg["B"])
    st.reset()
    x = torch.from_numpy(z["x"]).to(DEV)
    st.step(x[:, :1])
    proxy = CountingLib(streaming_ann.lib)
    monkeypatch.setattr(streaming_ann, "lib", proxy)
    monkeypatch.setattr(Fn, "lib", proxy)
    st.step(x[:, 1:2])
    return cfg, proxy.calls


@pytest.mark.parametrize("name", ["ann_GRU_bn", "ann_LiGRU_bn"])
def test_one_eager_step_is_one_launch_per_layer_two_for_the_gru(name, monkeypatch):
    cfg, calls = count_one_step(monkeypatch, name)
    hidden = len(cfg["layer_sizes"]) - 1
    per_layer = 2 if cfg["ann_type"] == "GRU" else 1
    assert calls.count("sparch_ann_stream_step") == hidden * per_layer
    assert calls.count("sparch_ann_stream_readout") == 1
    assert len(calls) == hidden * per_layer + 1, calls


def test_a_layernorm_layer_adds_its_gemm_and_layernorm_calls(monkeypatch):
    cfg, calls = count_one_step(monkeypatch, "ann_MLP_ln_bias_noreadout")
    hidden = len(cfg["layer_sizes"])                       # no readout layer
    assert calls.count("sparch_ann_stream_step") == hidden
    assert calls.count("sparch_layernorm_fwd") == hidden
    assert len(calls) == 3 * hidden, calls                 # GEMM, LayerNorm, step per layer
