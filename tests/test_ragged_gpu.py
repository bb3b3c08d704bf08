"""
Ragged batches on the GPU: the `_len` kernels alone against the fp64 restatement tests/spiking_numpy.py, whole networks
against tests/ragged_oracle.py, and the invariant itself — row b of net(x, lengths) is net(x[b:b+1, :L_b]) bit for bit.
Every test that passes `lengths=` is a TypeError without the feature.

Kernels alone (functional.cell_forward / cell_backward with lengths=, the readout entries at the C ABI):
  forward   the spikes (fp32 tensor, bf16 plane, spike_count) equal [u_save - theta > 0] on the kernel's OWN u_save times
            the validity mask, exactly: the tail is exactly zero and is not counted.  u_save / w_save against the
            teacher-forced restatement over all T steps (the state runs on over the padding).
  backward  on the kernel's own saves, with NaN in g_out on every padded step: the restatement's reverse pass with the
            mask as its keep multiplier — g = (g_out + g_rate / N) * [t < L_b] — i.e. the incoming gradient of the tail
            taken as zero and the rate term scaled by 1 / N.  dWx on the tail is exactly 0 and nothing is NaN.
  readout   per row, the restatement on the row's own first L_b steps (a truncated sum); u_save behind L_b is not written
            (it keeps the NaN it was given), dWx behind L_b is exactly 0.
Bounds: the rule of the fp64 kernel tests — 4 x the worst error of the restatement's fp32 runs against its fp64 run, asserted
to stay under 1e-5 of the reference's max-abs for the scan and readout kernels (spiking_numpy.capped).  At the small scan
shapes the backward's fp32 sample is pooled over further seeds of the same case recipe (pooled_relative_error says why).

Whole networks: the data regime and the bars of tests/test_hip_parity.py's whole-network tests (dyadic weights, initial
states on a 2^-4 grid: per-neuron spike counts equal, outputs to 1e-4, loss to 1e-5, every gradient to 5e-4 of its max-abs
(2e-2 in the bf16 operand mode), running statistics rtol 1e-4 / atol 1e-6).
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import snn_oracle as orc
from tests import ragged_oracle as rag
from tests import spiking_numpy as sn
from tests import surrogate_numpy as sg
from tests.kit import DEV, F32, F64, SEED, D, N, bf16_mode, record, relmax, within  # noqa: F401  (bf16_mode: a fixture)
from tests.kit import Fn as _Fn
from tests.kit import sp  # noqa: F401  (a fixture)
from tests.spiking_cases import collect

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_DROP = sn.P_DROP


def lengths_for(B, T, seed):
    """{1, 2, T - 1, T} first, then random ones."""
    rng = np.random.default_rng(seed)
    fixed = [v for v in (1, 2, T - 1, T) if 1 <= v <= T]
    lens = (fixed + [int(v) for v in rng.integers(1, T + 1, max(B - len(fixed), 0))])[:B]
    return np.asarray(lens, np.int64)


def dev_lengths(lens):
    return torch.from_numpy(lens.astype(np.int32)).to(DEV), int(lens.sum())


def mask_of(lens, T):
    return (np.arange(T)[None, :] < lens[:, None])


# ------------------------------------------------------------------------------------------------ hidden-layer kernels
POOL_SEEDS = 8


def seeded_scan_case(kind, B, T, H, salt):
    """spiking_numpy.scan_case's recipe on another seed."""
    seed = sn.case_seed(kind, B, 1, T, H) + 7919 * salt
    c = sn.make_inputs(kind, B, 1, T, H, seed, "drive", affine_in=True)
    c["g_rate"] = c["g_rate"] * F32(B * T)
    for k in c["p"]:
        c["p"][k][0], c["p"][k][1] = sn.OUTSIDE[k]
    rng = np.random.default_rng(seed + 1)
    c["bn"] = ((c["Wx"] * F32(0.8) + F32(0.3)).astype(F32), rng.uniform(0.2, 0.6, H).astype(F32),
               rng.uniform(0.5, 1.5, H).astype(F32))
    return c


def ragged_backward_runs(c, lens, us, ws, keep, with_bn, surrogate=None):
    """The restatement's reverse pass with the mask as its keep multiplier, on the saves us / ws: (fp64 run, [fp32 runs])."""
    kind, B, T, H = c["kind"], c["B"], c["T"], c["H"]
    m = mask_of(lens, T)[:, :, None]
    g_clean = np.where(m, c["g_out"], 0).astype(F32)
    # the restatement applies g = (g_out + g_rate / (B T)) * keep: the mask is the keep multiplier, N the rate's count
    g_rate = (c["g_rate"].astype(F64) * (B * T / int(lens.sum()))).astype(F32)
    keep_m = (m * (keep if keep is not None else F32(1))).astype(F32) * np.ones((1, 1, H), F32)

    def bw(dt, ko, ro):
        return sn.flat(sg.backward(kind, dt, g_clean, g_rate, us, ws, c["p"], c["u0"], c["w0"], c["s0"], B=B, dirs=1,
                                   surrogate=surrogate or ("boxcar", None), theta=c["theta"], k_order=ko,
                                   bn=c["bn"] if with_bn else None, keep=keep_m, row_order=ro))
    return bw(F64, None, None), [bw(F32, "asc", "asc"), bw(F32, "desc", "desc")]


@functools.lru_cache(maxsize=None)
def pooled_relative_error(kind, B, T, H, lens, p_drop, with_bn, surrogate=None):
    """The rule of the fp64 kernel tests is 4 x the worst error of the restatement's fp32 runs against its fp64 run.  At
    the ragged scan shapes (5 rows, 12 or 64 columns, a few dozen valid steps) the two fp32 runs of ONE case are a sample
    of a dozen column sums, and their worst error moves by a factor of 50 from one seed to the next (adLIF (5, 11, 12),
    beta: 1.1e-7 on the case's own seed, up to 5.9e-6 over twelve).  So the sample is made larger, not the factor: the
    worst fp32 error RELATIVE to the fp64 tensor's max-abs over POOL_SEEDS further cases of the same recipe, shape,
    lengths and keep mask, each on the restatement's own free-running saves — nothing of the kernel enters."""
    lens = np.asarray(lens)
    names = sn.bwd_tensors(kind, with_bn)
    worst = {k: 0.0 for k in names}
    for salt in range(1, POOL_SEEDS + 1):
        c = seeded_scan_case(kind, B, T, H, salt)
        f = sn.forward(kind, F32, c["Wx"], c["scale"], c["shift"], c["p"], c["u0"], c["w0"], c["s0"], B=B, dirs=1,
                       theta=c["theta"])
        ref, runs = ragged_backward_runs(c, lens, f["u_save"], f["w_save"], sn.scan_keep(c, SEED) if p_drop else None, with_bn,
                                          surrogate)
        for k in names:
            top = float(np.abs(ref[k]).max())
            worst[k] = max(worst[k], max(float(np.abs(r[k].astype(F64) - ref[k]).max()) for r in runs) / top)
    return worst


def check_cell(c, lens, p_drop, with_bn, spl=None, save16=False, capped=True, surrogate=None):
    """Forward and backward of one cell case with lengths; surrogate: None (the box-car) or ("name", scale).  Returns the
    worst fraction of the bound."""
    Fn = _Fn()
    kind, B, T, H, theta = c["kind"], c["B"], c["T"], c["H"], c["theta"]
    assert c["dirs"] == 1
    adaptive = sn.ADAPTIVE[kind]
    d = {k: D(c[k]) for k in ("Wx", "scale", "shift", "u0", "w0", "s0", "g_rate")}
    d["p"] = {k: D(v) for k, v in c["p"].items()}
    L = dev_lengths(lens)
    m = mask_of(lens, T)[:, :, None]
    keep = sn.scan_keep(c, SEED) if p_drop else None
    prev = Fn.SAVE_BF16
    Fn.SAVE_BF16 = save16
    try:
        s_out, count, saved, s16 = Fn.cell_forward(kind, d["Wx"], d["scale"], d["shift"], d["p"], d["u0"], d["w0"], d["s0"],
                                                   B=B, dirs=1, theta=theta, p_drop=p_drop, seed=SEED, steps_per_launch=spl,
                                                   lengths=L, surrogate=surrogate)
        _, count_p, _, s16_p = Fn.cell_forward(kind, d["Wx"], d["scale"], d["shift"], d["p"], d["u0"], d["w0"], d["s0"],
                                               B=B, dirs=1, theta=theta, p_drop=p_drop, seed=SEED, steps_per_launch=spl,
                                               surrogate=surrogate)
    finally:
        Fn.SAVE_BF16 = prev
    Fn.check_status()
    assert saved[0].dtype == (torch.bfloat16 if save16 else torch.float32)
    us, ws = N(saved[0], torch.float32), N(saved[1], torch.float32)
    worst = [0.0]
    plane = N(s16, torch.float32)
    if not save16:  # (a bf16 u keeps the three decisions, so the plane below is still exact; the states are rounded)
        S = ((us - F32(theta)) > 0).astype(F32)
        want = S * (keep if p_drop else F32(1)) * m
        assert 0.02 <= S.mean() <= 0.7
        assert np.array_equal(N(s_out), want), float((N(s_out) != want).mean())
        assert np.array_equal(plane, (want != 0).astype(F32))
        args = (c["Wx"], c["scale"], c["shift"], c["p"], c["u0"], c["w0"], c["s0"], us, ws)
        tf = lambda dt, ko: sn.teacher_forced_forward(kind, dt, *args, B=B, dirs=1, theta=theta, k_order=ko)  # noqa: E731
        ref = tf(F64, None)
        names = sn.FWD_TENSORS[adaptive]
        bound = sn.bound_of([tf(F32, "asc"), tf(F32, "desc")], ref, names)
        if capped:
            bound = sn.capped(bound, ref, names)
        worst += [within({"u_save": us, "w_save": ws}[k], ref[k], bound[k], k) for k in names]
    # the tail is exactly zero and not counted; the valid steps are the plain kernel's, bit for bit
    assert not (N(s_out) * ~m).any() and not (plane * ~m).any()
    assert np.array_equal(plane * m, N(s16_p, torch.float32) * m)
    assert np.array_equal(N(count).astype(np.int64), (plane != 0).sum((0, 1)))
    assert (N(count) < N(count_p)).any()    # (the plain run does fire on the padding: the mask is not vacuous)

    # ---- backward: NaN on every padded step of g_out
    g_host = c["g_out"].copy()
    g_poison = np.where(m, g_host, np.nan).astype(F32)
    g_clean = np.where(m, g_host, 0).astype(F32)
    bn = c["bn"] if with_bn else None
    dWx, grads = Fn.cell_backward(kind, D(g_poison), d["g_rate"], d["p"], d["u0"], d["w0"], d["s0"], saved, B=B, dirs=1, T=T,
                                  H=H, theta=theta, p_drop=p_drop, seed=SEED, steps_per_launch=spl,
                                  bn=None if bn is None else tuple(D(v) for v in bn), lengths=L,
                                  surrogate=surrogate)
    Fn.check_status()
    torch.cuda.synchronize()
    got = collect(dWx, grads, with_bn)
    for k, v in got.items():
        assert not np.isnan(v).any(), k
    assert not (got["dWx"] * ~m).any() and np.abs(got["dWx"]).max() > 0
    ref, runs32 = ragged_backward_runs(c, lens, us, ws, keep, with_bn, surrogate)
    names = sn.bwd_tensors(kind, with_bn)
    assert set(names) == set(got), (names, sorted(got))
    bound = sn.bound_of(runs32, ref, names)
    if capped and B * H < 4096:     # the small scan shapes: the fp32 error's sample pooled over further seeds
        rel = pooled_relative_error(kind, B, T, H, tuple(int(v) for v in lens), p_drop, with_bn, surrogate)
        bound = {k: max(bound[k], 4.0 * rel[k] * float(np.abs(ref[k]).max())) for k in names}
    if capped:
        bound = sn.capped(bound, ref, names)
    worst += [within(got[k], ref[k], bound[k], k) for k in names]
    if "V" in got:
        assert np.all(np.diag(got["V"]) == 0) and np.abs(got["V"]).max() > 0
    return max(worst)


# ring depths of the scan kernels at one neuron per thread: 15 / 12 forward (LIF / adLIF, every output), 16 / 15 / 12
# backward — T below, at and just above them, and one that is no multiple of any
SCAN_T = (11, 12, 13, 15, 16, 17, 29)


@pytest.mark.parametrize("T", SCAN_T)
@pytest.mark.parametrize("H", [12, 64])
@pytest.mark.parametrize("kind", sn.SCAN_KINDS)
def test_scan_kernels_with_lengths(kind, H, T, record_property):
    c = sn.scan_case(kind, 5, 1, T, H)
    lens = lengths_for(5, T, 7 * T + H)
    assert set(lens[:4]) == {1, 2, T - 1, T}
    worst = [check_cell(c, lens, 0.0, True), check_cell(c, lens, P_DROP, False)]
    if T == 17:
        worst += [check_cell(c, lens, P_DROP, True), check_cell(c, lens, 0.0, False)]
        if H % 4 == 0:
            worst.append(check_cell(c, lens, 0.0, True, save16=True))
    record(record_property, *worst)


def test_scan_kernels_with_lengths_four_neurons_per_thread(record_property):
    """The VEC = 4 instantiations (B H >= 524288, H % 4 == 0): ring depth 8, T = 9 and 17."""
    B, H = 33, 15888
    for kind in sn.SCAN_KINDS:
        for T in (9, 17):
            c = sn.scan_case(kind, B, 1, T, H)
            record(record_property, check_cell(c, lengths_for(B, T, T), 0.0 if T == 9 else P_DROP, True))


SMOOTH = ("fast_sigmoid", sg.TEST_SCALE["fast_sigmoid"])


@pytest.mark.parametrize("H", [12, 64])
@pytest.mark.parametrize("kind", sn.SCAN_KINDS)
def test_scan_kernels_with_lengths_and_a_smooth_surrogate(kind, H, record_property):
    """The SMOOTH instantiations of the ragged backward (the gate is picked at compile time there), with and without the
    folded BatchNorm sums and dropout."""
    T = 17
    c = sn.scan_case(kind, 5, 1, T, H)
    lens = lengths_for(5, T, 7 * T + H)
    record(record_property, check_cell(c, lens, 0.0, True, surrogate=SMOOTH),
           check_cell(c, lens, P_DROP, False, surrogate=SMOOTH))


def test_scan_kernels_with_lengths_four_neurons_per_thread_other_variants(record_property):
    """Four neurons per thread: bf16 saves (box-car) and a smooth surrogate (fp32 saves)."""
    B, H, T = 33, 15888, 9
    c = sn.scan_case("adLIF", B, 1, T, H)
    lens = lengths_for(B, T, T)
    record(record_property, check_cell(c, lens, 0.0, True, save16=True), check_cell(c, lens, P_DROP, True, surrogate=SMOOTH))


def rec_ragged_case(kind, B, T, H):
    c = sn.make_inputs(kind, B, 1, T, H, sn.case_seed(kind, B, 1, T, H), "drive")
    c["g_rate"] = (c["g_rate"] * F32(B * T)).astype(F32)    # (as drawn the rate term is 0.3 % of g_out)
    rng = np.random.default_rng(17)                         # the folded BatchNorm sums' operands, as spiking_numpy.scan_case's
    c["bn"] = ((c["Wx"] * F32(0.8) + F32(0.3)).astype(F32), rng.uniform(0.2, 0.6, H).astype(F32),
               rng.uniform(0.5, 1.5, H).astype(F32))
    lens = lengths_for(B, T, 5)
    lens[31], lens[32] = T - 3, 2
    return c, lens


@pytest.mark.parametrize("kind", ["RLIF", "RadLIF"])
def test_recurrent_kernels_with_lengths_and_a_smooth_surrogate(kind, record_property):
    """The smooth arm of the ragged recurrent backward's gate."""
    c, lens = rec_ragged_case(kind, 33, 19, 64)
    record(record_property, check_cell(c, lens, 0.0, True, capped=False, surrogate=SMOOTH))


@pytest.mark.parametrize("H", [132, 384, 1024])
def test_recurrent_kernels_with_lengths_wider_kernel_shapes(H, record_property):
    """The ragged instantiations of the 8-wave kernel shapes (k-group classes 2, 4 and 8), T = 6 as the fp64 recurrent
    tests run them."""
    c, lens = rec_ragged_case("RadLIF", 33, 6, H)
    record(record_property, check_cell(c, lens, 0.0, True, capped=False))


@pytest.mark.parametrize("mode", ["whole", "chunks7", "save_bf16"])
@pytest.mark.parametrize("kind", ["RLIF", "RadLIF"])
def test_recurrent_kernels_with_lengths(kind, mode, record_property):
    """B = 33: two 32-row tiles, the second with one row; lengths differ inside the first tile and across the two."""
    T = 19
    c, lens = rec_ragged_case(kind, 33, T, 64)
    assert len(set(lens[:32])) > 4 and lens[32] != lens[31]
    spl = 7 if mode == "chunks7" else None
    record(record_property, check_cell(c, lens, 0.0, False, spl=spl, save16=mode == "save_bf16", capped=False),
           check_cell(c, lens, 0.0, True, spl=spl, save16=mode == "save_bf16", capped=False))


# ------------------------------------------------------------------------------------------------ readout kernels
@pytest.mark.parametrize("affine", [False, True], ids=["plain", "affine_bn"])
def test_readout_kernels_with_lengths(affine, record_property):
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    B, T, C = 5, 300, 35
    lens = np.asarray([1, 255, 256, 257, 300], np.int64)
    c = sn.readout_case(B, T, C)
    d = {k: D(c[k]) for k in ("Wx", "u0", "alpha", "g_out", "scale", "shift")}
    bn_dev = tuple(D(v) for v in c["bn"])
    L = dev_lengths(lens)
    x_host = c["bn"][0] if affine else c["Wx"]
    x, scale, shift = (bn_dev[0], d["scale"], d["shift"]) if affine else (d["Wx"], None, None)
    out = torch.full((B, C), float("nan"), dtype=torch.float32, device=DEV)
    u_save = torch.full((B, T, C), float("nan"), dtype=torch.float32, device=DEV)
    check(lib.sparch_readout_fwd_len(B, T, C, ptr(x), ptr(scale), ptr(shift), ptr(d["alpha"]), ptr(d["u0"]), ptr(out),
                                     ptr(u_save), ptr(L[0]), L[1], Fn._stream()), "sparch_readout_fwd_len")
    dWx = torch.full((B, T, C), float("nan"), dtype=torch.float32, device=DEV)
    ws = torch.empty(3 if affine else 1, B, C, dtype=torch.float32, device=DEV)
    bnp = [ptr(v) for v in bn_dev] if affine else [None, None, None]
    check(lib.sparch_readout_bwd_len(B, T, C, ptr(d["g_out"]), *bnp, ptr(u_save), ptr(d["alpha"]), ptr(d["u0"]), ptr(dWx),
                                     ptr(ws), ptr(L[0]), L[1], Fn._stream()), "sparch_readout_bwd_len")
    if affine:
        dalpha, s1, s2 = Fn._finish_param_grads(ws, B, C, [d["alpha"], None, None], [Fn.ALPHA_LIM, (0.0, 0.0), (0.0, 0.0)])
        got = {"alpha": N(dalpha), "bn_dy": N(s1), "bn_dyx": N(s2)}
    else:
        got = {"alpha": N(Fn._finish_param_grads(ws, B, C, [d["alpha"]], [Fn.ALPHA_LIM])[0])}
    Fn.check_status()
    got.update(u_save=N(u_save), out=N(out), dWx=N(dWx))
    m = mask_of(lens, T)[:, :, None]
    # behind a row's length: u_save not written, dWx exactly 0; nothing else is NaN
    assert np.isnan(got["u_save"][np.broadcast_to(~m, got["u_save"].shape)]).all()
    assert not np.isnan(got["u_save"][np.broadcast_to(m, got["u_save"].shape)]).any()
    assert not (got["dWx"] * ~m).any() and not np.isnan(got["dWx"]).any()
    for k in ("out", "alpha"):
        assert not np.isnan(got[k]).any(), k
    bn = c["bn"] if affine else None

    def run(dt, order):
        """Row by row on the row's own steps: the clip run alone."""
        res = {"out": np.zeros((B, C), dt), "dWx": np.zeros((B, T, C), dt), "u_save": np.zeros((B, T, C), dt)}
        sums = {}
        rows = range(B) if order != "desc" else range(B - 1, -1, -1)
        for b in rows:
            n = int(lens[b])
            u, o = sn.readout_forward(dt, x_host[b:b + 1, :n], None if scale is None else c["scale"],
                                      None if shift is None else c["shift"], c["alpha"], c["u0"][b:b + 1], order)
            res["u_save"][b, :n], res["out"][b] = u[0], o[0]
            bn_b = None if bn is None else (bn[0][b:b + 1, :n], bn[1], bn[2])
            r = sn.readout_backward(dt, c["g_out"][b:b + 1], got["u_save"][b:b + 1, :n], c["alpha"], c["u0"][b:b + 1],
                                    bn=bn_b, class_order=order)
            res["dWx"][b, :n] = r["dWx"][0]
            for k in ("alpha",) + (("bn_dy", "bn_dyx") if affine else ()):
                sums[k] = r[k].astype(dt) if k not in sums else (sums[k] + r[k]).astype(dt)
        res.update(sums)
        return res

    ref = run(F64, None)
    assert abs(ref["out"].sum() - lens.sum()) <= 1e-9 * lens.sum()          # a truncated sum, not a mean
    names = ("out", "dWx") + sn.READOUT_BWD_TENSORS[affine][1:]
    bound = sn.capped(sn.bound_of([run(F32, "asc"), run(F32, "desc")], ref, names), ref, names)
    worst = [within(got[k], ref[k], bound[k], k) for k in names]
    ub = sn.bound_of([run(F32, "asc"), run(F32, "desc")], ref, ("u_save",))["u_save"]
    worst.append(within(np.where(m, got["u_save"], 0), ref["u_save"], ub, "u_save"))
    assert got["alpha"][0] == 0 and got["alpha"][1] == 0 and np.abs(got["alpha"][2:]).max() > 0
    record(record_property, *worst)


# ------------------------------------------------------------------------------------------------ whole networks
SIZES, NB, NT, NC = [64, 64, 20], 6, 23, 40
NET_LENGTHS = [23, 1, 9, 17, 2, 22]


def make_net(sp, kind, normalization, dropout=0.0, seed=3):
    torch.manual_seed(seed)
    net = sp.SNN((NB, None, NC), SIZES, neuron_type=kind, dropout=dropout, normalization=normalization)
    with torch.no_grad():
        for lay in net.snn:
            lay.W.weight.copy_(torch.round((lay.W.weight * 4 + 0.25) * 64) / 64)   # (a positive drive: every layer spikes)
            if hasattr(lay, "V"):
                lay.V.weight.copy_(torch.round(lay.V.weight * 64) / 64)
            if normalization in ("batchnorm", "layernorm"):   # (a live affine: the normalised drive reaches the threshold)
                lay.norm.weight.copy_(torch.round((torch.rand_like(lay.norm.weight) + 1.0) * 16) / 16)
                lay.norm.bias.copy_(torch.round((torch.rand_like(lay.norm.bias) * 0.5 + 0.25) * 16) / 16)
    return net


def net_inputs(kind, seed=11, lengths=NET_LENGTHS):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(NB, NT, NC, generator=g) < 0.3).float()
    x = x * rag.valid_mask(lengths, NT)[:, :, None]
    y = torch.randint(0, SIZES[-1], (NB,), generator=g)
    torch.manual_seed(seed + 1)
    init = orc.draw_init_states(NB, SIZES, kind)
    init = [{k: torch.floor(v * 16) / 16 for k, v in st.items()} for st in init]
    return x, y, init


class injected_states:
    """The initial states of `init` (row range `rows`) handed to the network's draws, in the reference's order."""

    def __init__(self, init, rows=slice(None)):
        self.order = [st[k][rows] for st in init for k in ("u0", "w0", "s0") if k in st]

    def __enter__(self):
        from sparch_amd import snns as snn_mod
        it = iter(self.order)
        self.mod, self.old = snn_mod, snn_mod._rand_to
        snn_mod._rand_to = lambda rows, cols, device: next(it).to(device)

    def __exit__(self, *exc):
        self.mod._rand_to = self.old


@pytest.mark.parametrize("compute", ["fp32", "bf16"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("normalization", ["batchnorm", "layernorm", "none"])
@pytest.mark.parametrize("kind", ["LIF", "adLIF", "RLIF", "RadLIF"])
def test_whole_network_vs_ragged_oracle(sp, kind, normalization, training, compute, request):
    if compute == "bf16":
        request.getfixturevalue("bf16_mode")
    tol_g = 5e-4 if compute == "fp32" else 2e-2
    net = make_net(sp, kind, normalization)
    params = {k: v.clone() for k, v in net.state_dict().items()}
    x, y, init = net_inputs(kind)
    net = net.to(DEV).train(training)
    with injected_states(init):
        out, rates = net(x.to(DEV), lengths=torch.tensor(NET_LENGTHS))
        loss = orc.train_step_loss(out, rates, y.to(DEV), use_regularizers=True)
        loss.backward()
        _Fn().check_status()
    po = {k: v.clone().requires_grad_(v.dtype == torch.float32 and "running" not in k) for k, v in params.items()}
    stats = {}
    out_o, rates_o = rag.snn_forward(x, NET_LENGTHS, po, neuron_type=kind, num_layers=3, init_states=init,
                                     normalization=normalization, training=training, stats=stats)
    loss_o = orc.train_step_loss(out_o, rates_o, y, use_regularizers=True)
    loss_o.backward()
    n_valid = sum(NET_LENGTHS)
    counts, counts_o = torch.round(rates.detach().cpu() * n_valid).long(), torch.round(rates_o.detach() * n_valid).long()
    assert int(counts_o[:SIZES[0]].sum()) > 0 and int(counts_o[SIZES[0]:].sum()) > 0
    assert torch.equal(counts, counts_o), "per-neuron spike counts differ from the oracle"
    eo = relmax(N(out), out_o.detach().numpy())
    print(f"  out {eo:.3e}  loss {float(loss):.6f} / {float(loss_o):.6f}")
    assert eo <= 1e-4
    assert abs(float(loss) - float(loss_o)) <= 1e-5 * max(1.0, abs(float(loss_o)))
    assert relmax(N(rates), rates_o.detach().numpy()) <= 1e-6
    for k, v in net.named_parameters():
        e = relmax(N(v.grad), po[k].grad.numpy())
        assert e <= tol_g, (k, e)
    for k, v in stats.items():
        np.testing.assert_allclose(N(net.state_dict()[k]), v.numpy(), rtol=1e-4, atol=1e-6, err_msg=k)


def test_input_gradient_is_zero_on_the_padding(sp):
    net = make_net(sp, "adLIF", "batchnorm").to(DEV).train()
    x, y, init = net_inputs("adLIF")
    xd = x.to(DEV).requires_grad_(True)
    with injected_states(init):
        out, rates = net(xd, lengths=torch.tensor(NET_LENGTHS, device=DEV))    # (lengths on the device work too)
        orc.train_step_loss(out, rates, y.to(DEV), use_regularizers=True).backward()
    g = N(xd.grad)
    m = rag.valid_mask(NET_LENGTHS, NT).numpy()[:, :, None]
    assert not (g * ~m).any() and np.abs(g).max() > 0 and not np.isnan(g).any()


@pytest.mark.parametrize("normalization", ["batchnorm", "layernorm", "none"])
@pytest.mark.parametrize("kind", ["LIF", "adLIF", "RLIF", "RadLIF"])
def test_a_row_is_its_clip_run_alone_bit_for_bit(sp, kind, normalization):
    """Eval mode, dyadic data: net(x, lengths)[0][b] equals net(x[b:b+1, :L_b])[0]; another row's content or length does
    not change row b's bits."""
    net = make_net(sp, kind, normalization).to(DEV).eval()
    x, _, init = net_inputs(kind)
    with torch.no_grad():
        with injected_states(init):
            out, _ = net(x.to(DEV), lengths=torch.tensor(NET_LENGTHS))
        for b, n in enumerate(NET_LENGTHS):
            with injected_states(init, slice(b, b + 1)):
                alone, _ = net(x[b:b + 1, :n].contiguous().to(DEV))
            assert torch.equal(out[b:b + 1], alone), (b, n)
        x2, lens2 = x.clone(), list(NET_LENGTHS)
        x2[0] = (torch.rand(NT, NC) < 0.5).float()            # row 0: other content, row 3: another length
        lens2[3] = 5
        x2 = x2 * rag.valid_mask(lens2, NT)[:, :, None]
        with injected_states(init):
            out2, _ = net(x2.to(DEV), lengths=torch.tensor(lens2))
    keep = [1, 2, 4, 5]
    assert torch.equal(out2[keep], out[keep])
    assert not torch.equal(out2[0], out[0]) and not torch.equal(out2[3], out[3])
    _Fn().check_status()


@pytest.mark.parametrize("kind", ["adLIF", "RadLIF"])
def test_dropout_on(sp, kind):
    """Tails are zero; with every length == T the outputs are the plain forward's bits."""
    net = make_net(sp, kind, "batchnorm", dropout=0.25).to(DEV).train()
    for i, lay in enumerate(list(net.snn)[:-1]):
        lay._dropout_seed = lambda device, i=i: SEED + i
    x, _, init = net_inputs(kind)
    lay = net.snn[0]
    from sparch_amd import snns as snn_mod
    st = tuple(None if k not in init[0] else init[0][k].to(DEV) for k in ("u0", "w0", "s0"))
    with torch.no_grad():
        L = snn_mod.prepare_lengths(NET_LENGTHS, NB, NT, DEV)
        s, rate = lay.forward_with_rate(x.to(DEV), states=st, lengths=L)
        m = rag.valid_mask(NET_LENGTHS, NT).to(DEV)[:, :, None]
        assert not (s * ~m).any() and float(s.sum()) > 0
        assert set(np.unique(N(s)).tolist()) <= {0.0, float(np.float32(1.0) / np.float32(0.75))}
        np.testing.assert_allclose(N(rate), N(s.sum((0, 1)) / sum(NET_LENGTHS)), rtol=1e-6)
        xf, _, _ = net_inputs(kind, lengths=[NT] * NB)
        with injected_states(init):
            a, ra = net(xf.to(DEV))
        with injected_states(init):
            b, rb = net(xf.to(DEV), lengths=torch.tensor([NT] * NB))
    assert torch.equal(a, b) and torch.equal(ra, rb)
    _Fn().check_status()


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_hd_with_masked_lengths(tmp_path, monkeypatch):
    """SPARCH_LENGTHS=mask run_exp.py --dataset_name hd on a tiny folder of unequal clips: two training steps, every batch
    goes to the network with its own unequal lengths and the loss is finite.  The run is eager: run_exp.py has no
    captured-step mode to fall back from, and SNN.forward refuses lengths inside a captured step (tests/test_ragged_host.py)."""
    import run_exp
    import sparch_amd
    from sparch_amd import exp
    from tests.audio_trees import make_hd_tree
    root = str(tmp_path / "hd")
    make_hd_tree(root, n_train=8, n_test=4, lengths=(16000, 6400, 11200, 9000))
    monkeypatch.setenv("SPARCH_LENGTHS", "mask")
    seen = []
    forward = sparch_amd.SNN.forward
    loss_call = exp.Fn.CrossEntropyLoss.forward

    def spy(self, x, lengths=None):
        seen.append(None if lengths is None else [int(v) for v in lengths])
        assert getattr(self, "_static_states", None) is None      # eager
        return forward(self, x, lengths=lengths)

    losses = []

    def loss_spy(self, output, target):
        v = loss_call(self, output, target)
        losses.append(float(v))
        return v

    monkeypatch.setattr(sparch_amd.SNN, "forward", spy)
    monkeypatch.setattr(exp.Fn.CrossEntropyLoss, "forward", loss_spy)
    torch.manual_seed(5)
    run_exp.main(["--model_type", "adLIF", "--nb_layers", "3", "--nb_hiddens", "64", "--dataset_name", "hd",
                  "--data_folder", root, "--batch_size", "4", "--nb_epochs", "1", "--save_best", "0",
                  "--new_exp_folder", str(tmp_path / "exp")])
    train = seen[:2]
    assert len(seen) >= 3 and all(v is not None for v in seen)    # two training steps, then validation
    assert all(len(set(v)) > 1 for v in train), train             # unequal clips in a batch
    assert len(losses) >= 3 and all(np.isfinite(v) for v in losses), losses
