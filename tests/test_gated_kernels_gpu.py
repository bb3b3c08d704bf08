"""
The recurrent kernels of the non-spiking baselines — ann_rec_kernel (sparch_amd/csrc/reccell.hip), ligru_fwd/bwd_kernel
and gru_fwd/bwd_kernel (gatedcell.hip), the launch-per-step kernels sparch_ann_rec_step_fwd/_bwd and sparch_gate_step
(annstep.hip) — called through the C ABI at precision 0, every output prefilled with NaN inside the guard bands of
tests/guarded.embed, `chan` and the V packs sized exactly by the library's *_bytes functions (guarded too), the status
word checked after every launch group, and compared with the fp64 restatement tests/gated_numpy.py (pinned to the
oracle and to torch autograd by tests/test_gated_numpy_host.py):

  a  small shapes, every path   RNN (sigmoid, relu, tanh), LiGRU, GRU x one / two directions x dropout off / on at
                                (B 3, T 1, H 32), (B 33, T 9, H 96) and (B 5, T 40, H 64): the persistent kernels
                                launched whole, in chunks of 1 and of 7 steps (bit-identical to the whole launch, chunk
                                carry included), and the launch-per-step kernels with the recurrent product supplied
                                from the fp64 reference (no GEMM involved)
  b  the benchmark's geometry   H = 1024, T = 6, p_drop 0.1 with more row tiles than one launch holds, so that a second
                                row-tile group runs with rt_base > 0 and a short last group; a direction boundary
                                inside a row tile; a full machine of co-resident RNN workgroups; H = 512 with 9 row
                                tiles.  The batch sizes follow from sparch_device_cus()
  c  error codes                refused on the host, nothing launched or written
  d  the same bits              SHA-256 of every output of the whole-sequence persistent launches against
                                tests/golden/baseline_rec_bits.json: what the fp64 bounds cannot see (a reordered MFMA
                                term, another reduction order) changes a hash

Inputs: standard-normal projections and upstream gradients, scale in [0.7, 1.3], shift in [-0.2, 0.2], recurrent
matrices of standard deviation 0.5 / sqrt(H).  The backward kernels get the fp64 reference's saves rounded to fp32 (not
a forward kernel's output): forward error does not leak into the backward check, and the relu branch is decided by the
same c_save bits on both sides.

Every numeric comparison is |got - ref64| <= bound per element, one bound per output tensor: FOUR times the larger of
the worst absolute errors of two fp32 runs of the restatement on the same inputs (numpy's matmul; the recurrent product
accumulated over K in chunks of 32) against the fp64 run.  The factor four is the convention of tests/head_numpy.py —
margin over a reference-derived yardstick, never fitted to a kernel; the bound is computed here from the references
alone, and each test records the worst fraction it saw (record_property; DESIGN.md has the table measured on an
MI355X).  Layout facts are compared bit for bit: yprev_all (RNN: y_prev) is the input y_state moved one cell step and
re-indexed to the original time, +0.0 at the first step; ry_all = r_save * yprev in fp32; y_out is zero exactly where
the restated dropout mask is zero and y_state * 1/(1-p) elsewhere; no NaN is left in any output; the guards are intact.

Every shape and pointer a kernel receives is valid.
"""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import gated_numpy as gn
from tests.guarded import embed
from tests.kit import DEV, EINVAL, EWORKSPACE, F32, F64, D, N, nan_, ptr, same_bits, sha, within
from tests.kit import Fn as _Fn
from tests.kit import capi as _capi

pytestmark = pytest.mark.gpu

SEED = 0x1234567089ABCDEF                    # < 2^63: the seed, not an address; not kit.SEED: the recorded bits hold it

CELLS = [("RNN", "sigmoid"), ("RNN", "relu"), ("RNN", "tanh"), ("LiGRU", None), ("GRU", None)]
CELL_IDS = ["rnn_sigmoid", "rnn_relu", "rnn_tanh", "ligru", "gru"]
FWD_NUM = {"RNN": ("y_state", "y_out"), "LiGRU": ("y_state", "z_save", "c_save", "y_out"),
           "GRU": ("y_state", "z_save", "r_save", "c_save", "y_out")}
BWD_NUM = {"RNN": ("dpre",), "LiGRU": ("dz_all", "dc_all"), "GRU": ("dz_all", "dr_all", "dc_all")}
BWD_OUT = {"RNN": ("dpre", "y_prev"), "LiGRU": ("dz_all", "dc_all", "yprev_all"),
           "GRU": ("dz_all", "dr_all", "dc_all", "yprev_all", "ry_all")}
SAVES = {"RNN": ("y_state",), "LiGRU": ("y_state", "z_save", "c_save"), "GRU": ("y_state", "z_save", "r_save", "c_save")}


def guarded(rows, cols):
    """A NaN-filled (rows, cols) tensor between guard bands."""
    return embed(nan_(rows, cols), cols, 0)


def exact_bytes(nbytes):
    """A NaN-filled buffer of exactly nbytes (a multiple of 16) on a 256-byte boundary, between guard bands."""
    assert nbytes > 0 and nbytes % 16 == 0, nbytes
    n, cols = nbytes // 4, 1024
    while n % cols:
        cols //= 2
    return guarded(n // cols, cols)


# ====================================================================================================== references
class Case:
    pass


def _forward(cell, kind, X, V, dirs, p, dtype, mm):
    if cell == "RNN":
        return gn.rnn_forward(kind, *X["c"], V["c"], dirs, p, SEED, dtype, mm)
    return gn.gated_forward(cell, X, V, dirs, p, SEED, dtype, mm)


def _backward(cell, kind, g_out, saves, V, dirs, p, dtype, mm):
    if cell == "RNN":
        return gn.rnn_backward(kind, g_out, saves["y_state"], V["c"], dirs, p, SEED, dtype, mm)
    return gn.gated_backward(cell, g_out, saves, V, dirs, p, SEED, dtype, mm)


@functools.lru_cache(maxsize=2)
def case(cell, kind, B, T, H, dirs, p_drop):
    """Inputs, the fp64 reference of both passes and the bounds of one case, built once and shared by everything
    that runs on it (the arrays are never written to)."""
    c = Case()
    c.cell, c.kind, c.B, c.T, c.H, c.dirs, c.p = cell, kind, B, T, H, dirs, p_drop
    c.Bp, c.HO = B * dirs, H * dirs
    c.X, c.V, c.g_out = gn.inputs(cell, B, T, H, dirs, 1000003 * B + 1009 * T + 31 * H + 7 * dirs + len(cell))
    c.mask = gn.mask_of(SEED, (B, T, c.HO), p_drop, F32)
    runs = [(F64, np.matmul), (F32, np.matmul), (F32, gn.matmul_chunked)]
    fwd = [_forward(cell, kind, c.X, c.V, dirs, p_drop, dt, mm) for dt, mm in runs]
    c.saves = {k: fwd[0][k].astype(F32) for k in SAVES[cell]}       # what the backward kernels are given
    bwd = [_backward(cell, kind, c.g_out, c.saves, c.V, dirs, p_drop, dt, mm) for dt, mm in runs]
    c.ref_f, c.ref_b = fwd[0], bwd[0]
    c.bound = {}
    for names, res in ((FWD_NUM[cell], fwd), (BWD_NUM[cell], bwd)):
        for k in names:
            c.bound[k] = 4.0 * max(float(np.abs(r[k].astype(F64) - res[0][k]).max()) for r in res[1:])
    c.dev = None
    return c


def dev(c):
    if c.dev is None:
        c.dev = {"X": {m: tuple(D(a, F32) for a in c.X[m]) for m in c.X}, "V": {m: D(c.V[m], F32) for m in c.V},
                 "g_out": D(c.g_out, F32), "saves": {k: D(v, F32) for k, v in c.saves.items()}}
    return c.dev


def steps_first(a):
    """(Bp,T,W) in cell time order -> device (T,Bp,W): one contiguous (Bp,W) operand per step."""
    return D(np.asarray(a).transpose(1, 0, 2), F32)


# ====================================================================================================== launches
PER_ROW = ("carry", "ry", "dcp", "y_step", "dpre_step", "cdir0", "cdir1", "dgate")     # (Bp,H); dgate (Bp,2H)


def outputs(c, names):
    """NaN-filled, guarded: y_out (B*T, H*dirs), the PER_ROW buffers, everything else (Bp*T, H)."""
    def shape(k):
        if k in PER_ROW:
            return c.Bp, (2 * c.H if k == "dgate" else c.H)
        return (c.B * c.T, c.HO) if k == "y_out" else (c.Bp * c.T, c.H)
    return {k: guarded(*shape(k)) for k in names}


def collect(c, rcs, o, buffers, expect=0, scratch=()):
    """All return codes equal `expect`; the status word is clear; the guards of every output and buffer are intact.
    expect == 0: the outputs as numpy arrays (no NaN left in any but the `scratch` ones); otherwise nothing was
    launched: every output and buffer still holds its NaN fill."""
    assert all(rc == expect for rc in rcs), (rcs, expect)
    assert _Fn().check_status() is False
    for k, t in list(o.items()) + [(f"buffer {i}", b) for i, b in enumerate(buffers)]:
        t.check(f"{c.cell} {k}")
    if expect != 0:
        for k, t in list(o.items()) + [(f"buffer {i}", b) for i, b in enumerate(buffers)]:
            assert bool(torch.isnan(t).all()), f"{c.cell}: {k} was written by a refused call"
        return None
    got = {}
    for k, t in o.items():
        a = N(t)
        got[k] = a if k in PER_ROW else a.reshape((c.B, c.T, c.HO) if k == "y_out" else (c.Bp, c.T, c.H))
        assert k in scratch or not np.isnan(got[k]).any(), f"{c.cell}: NaN left in {k}"
    return got


def status():
    return _Fn().status_word(DEV)


def vpack_buffer(nbytes):
    """The exact-size V pack; a size query that returns 0 (unsupported H) gets a dummy the refused calls never touch."""
    return exact_bytes(nbytes if nbytes else 4096)


def rnn_fwd(c, L, act=None, chan_short=0, expect=0):
    lib, d = _capi().lib, dev(c)
    Wx, sc, sh = d["X"]["c"]
    o = outputs(c, ("y_out", "y_state"))
    vp = vpack_buffer(lib.sparch_vpack_bytes(c.H))
    assert lib.sparch_vpack(c.H, ptr(d["V"]["c"]), 1 | 2, ptr(vp), None, None, 0) == 0           # y V^T, dense
    nb = lib.sparch_rec_chan_bytes(c.Bp, c.T, c.H)
    chan = exact_bytes(nb)
    rc = lib.sparch_ann_rec_fwd(gn.ACT_KIND[c.kind] if act is None else act, c.B, c.dirs, c.T, c.H, ptr(Wx), ptr(sc),
                                ptr(sh), ptr(vp), c.p, SEED, ptr(o["y_out"]), ptr(o["y_state"]), ptr(chan),
                                nb - chan_short, ptr(status()), L, None)
    return collect(c, [rc], o, [chan], expect) if expect else collect(c, [rc], o, [vp, chan])


def rnn_bwd(c, L, act=None, chan_short=0, expect=0):
    lib, d = _capi().lib, dev(c)
    o = outputs(c, ("dpre", "y_prev"))
    vp = vpack_buffer(lib.sparch_vpack_bytes(c.H))
    assert lib.sparch_vpack(c.H, ptr(d["V"]["c"]), 0 | 2, ptr(vp), None, None, 0) == 0           # dpre V, dense
    nb = lib.sparch_rec_chan_bytes(c.Bp, c.T, c.H)
    chan = exact_bytes(nb)
    rc = lib.sparch_ann_rec_bwd(gn.ACT_KIND[c.kind] if act is None else act, c.B, c.dirs, c.T, c.H, ptr(d["g_out"]),
                                ptr(d["saves"]["y_state"]), ptr(vp), c.p, SEED, ptr(o["dpre"]), ptr(o["y_prev"]),
                                ptr(chan), nb - chan_short, ptr(status()), L, None)
    return collect(c, [rc], o, [chan], expect) if expect else collect(c, [rc], o, [vp, chan])


def rnn_fwd_steps(c, act=None, expect=0):
    lib, d = _capi().lib, dev(c)
    Wx, sc, sh = d["X"]["c"]
    o = outputs(c, ("y_out", "y_state", "y_step"))
    recs = steps_first(c.ref_f["rec"])
    rcs = [lib.sparch_ann_rec_step_fwd(gn.ACT_KIND[c.kind] if act is None else act, c.B, c.dirs, c.T, c.H, s, ptr(Wx),
                                       ptr(sc), ptr(sh), ptr(recs[s]) if s else None, c.p, SEED, ptr(o["y_out"]),
                                       ptr(o["y_state"]), ptr(o["y_step"]), None) for s in range(c.T)]
    got = collect(c, rcs, o, [], expect)
    if got is not None:
        assert same_bits(got["y_step"], got["y_state"][:, c.T - 1])
    return got


def rnn_bwd_steps(c, act=None, expect=0):
    lib, d = _capi().lib, dev(c)
    o = outputs(c, ("dpre", "y_prev", "dpre_step"))
    recs = steps_first(c.ref_b["rec"])
    rcs = []
    for s in range(c.T):
        t = c.T - 1 - s
        rcs.append(lib.sparch_ann_rec_step_bwd(gn.ACT_KIND[c.kind] if act is None else act, c.B, c.dirs, c.T, c.H, s,
                                               ptr(d["g_out"]), ptr(d["saves"]["y_state"]), ptr(recs[t]) if s else None,
                                               c.p, SEED, ptr(o["dpre"]), ptr(o["y_prev"]), ptr(o["dpre_step"]), None))
    got = collect(c, rcs, o, [], expect)
    if got is not None:
        assert same_bits(got["dpre_step"], gn.to_original(got["dpre"], c.B, c.dirs)[:, 0])     # cell step 0 came last
    return got


def gated_fwd(c, L, chan_short=0, expect=0):
    lib, d = _capi().lib, dev(c)
    gru = c.cell == "GRU"
    x = [ptr(a) for m in ("c", "z") + (("r",) if gru else ()) for a in d["X"][m]]
    o = outputs(c, FWD_NUM[c.cell])
    if gru:
        vg, vc = (vpack_buffer(lib.sparch_gru_vpack_bytes(c.H, 0, w)) for w in (0, 1))
        rcp = lib.sparch_gru_vpack(c.H, ptr(d["V"]["z"]), ptr(d["V"]["r"]), ptr(d["V"]["c"]), 0, ptr(vg), ptr(vc), None, 0)
        nb = lib.sparch_gru_chan_bytes(c.Bp, c.H)
        chan = exact_bytes(nb)
        rc = lib.sparch_gru_fwd(c.B, c.dirs, c.T, c.H, *x, ptr(vg), ptr(vc), c.p, SEED, ptr(o["y_out"]), ptr(o["y_state"]),
                                ptr(o["z_save"]), ptr(o["r_save"]), ptr(o["c_save"]), ptr(chan), nb - chan_short,
                                ptr(status()), L, None)
        packs = [vg, vc]
    else:
        vp = vpack_buffer(lib.sparch_ligru_vpack_bytes(c.H, 0))
        rcp = lib.sparch_ligru_vpack(c.H, ptr(d["V"]["z"]), ptr(d["V"]["c"]), 0, ptr(vp), None, 0)
        nb = lib.sparch_ligru_chan_bytes(c.Bp, c.H)
        chan = exact_bytes(nb)
        rc = lib.sparch_ligru_fwd(c.B, c.dirs, c.T, c.H, *x, ptr(vp), c.p, SEED, ptr(o["y_out"]), ptr(o["y_state"]),
                                  ptr(o["z_save"]), ptr(o["c_save"]), ptr(chan), nb - chan_short, ptr(status()), L, None)
        packs = [vp]
    if expect:
        assert rcp == (0 if c.H % 32 == 0 else EINVAL)
        return collect(c, [rc], o, [chan] + ([] if rcp == 0 else packs), expect)
    assert rcp == 0
    return collect(c, [rc], o, packs + [chan])


def gated_bwd(c, L, chan_short=0, expect=0):
    lib, d = _capi().lib, dev(c)
    gru = c.cell == "GRU"
    s = d["saves"]
    o = outputs(c, BWD_OUT[c.cell] + ("carry",))
    if gru:
        vg, vc = (vpack_buffer(lib.sparch_gru_vpack_bytes(c.H, 1, w)) for w in (0, 1))
        rcp = lib.sparch_gru_vpack(c.H, ptr(d["V"]["z"]), ptr(d["V"]["r"]), ptr(d["V"]["c"]), 1, ptr(vg), ptr(vc), None, 0)
        nb = lib.sparch_gru_chan_bytes(c.Bp, c.H)
        chan = exact_bytes(nb)
        rc = lib.sparch_gru_bwd(c.B, c.dirs, c.T, c.H, ptr(d["g_out"]), ptr(s["y_state"]), ptr(s["z_save"]), ptr(s["r_save"]),
                                ptr(s["c_save"]), ptr(vg), ptr(vc), c.p, SEED, ptr(o["dz_all"]), ptr(o["dr_all"]),
                                ptr(o["dc_all"]), ptr(o["yprev_all"]), ptr(o["ry_all"]), ptr(o["carry"]), ptr(chan),
                                nb - chan_short, ptr(status()), L, None)
        packs = [vg, vc]
    else:
        vp = vpack_buffer(lib.sparch_ligru_vpack_bytes(c.H, 1))
        rcp = lib.sparch_ligru_vpack(c.H, ptr(d["V"]["z"]), ptr(d["V"]["c"]), 1, ptr(vp), None, 0)
        nb = lib.sparch_ligru_chan_bytes(c.Bp, c.H)
        chan = exact_bytes(nb)
        rc = lib.sparch_ligru_bwd(c.B, c.dirs, c.T, c.H, ptr(d["g_out"]), ptr(s["y_state"]), ptr(s["z_save"]),
                                  ptr(s["c_save"]), ptr(vp), c.p, SEED, ptr(o["dz_all"]), ptr(o["dc_all"]),
                                  ptr(o["yprev_all"]), ptr(o["carry"]), ptr(chan), nb - chan_short, ptr(status()), L, None)
        packs = [vp]
    if expect:
        assert rcp == (0 if c.H % 32 == 0 else EINVAL)
        return collect(c, [rc], o, [chan] + ([] if rcp == 0 else packs), expect)
    assert rcp == 0
    return collect(c, [rc], o, packs + [chan])


def gate_step(c, mode, t, ins, outs):
    arr = ctypes.c_void_p * 14
    a_in = arr(*[ptr(ins.get(n)) for n in gn.IN_SLOTS])
    a_out = arr(*[ptr(outs.get(n)) for n in gn.OUT_SLOTS])
    return _capi().lib.sparch_gate_step(mode, c.B, c.dirs, c.T, c.H, t, a_in, a_out, c.p, SEED, None)


def gated_fwd_steps(c):
    d = dev(c)
    gru = c.cell == "GRU"
    names = ("Wx", "sc", "sh", "Wzx", "scz", "shz", "Wrx", "scr", "shr")
    ins = dict(zip(names, [a for m in ("c", "z") + (("r",) if gru else ()) for a in d["X"][m]]))
    o = outputs(c, FWD_NUM[c.cell] + (("ry",) if gru else ()))
    rec_gate = steps_first(np.concatenate([c.ref_f["rec_z"], c.ref_f["rec_r" if gru else "rec_c"]], axis=2))   # (T,Bp,2H)
    rec_cand = steps_first(c.ref_f["rec_c"]) if gru else None
    rcs = []
    for t in range(c.T):
        if gru:
            rcs.append(gate_step(c, 1, t, dict(ins, rec=rec_gate[t] if t else None), o))
            rcs.append(gate_step(c, 2, t, dict(ins, rec=rec_cand[t] if t else None), o))
        else:
            rcs.append(gate_step(c, 0, t, dict(ins, rec=rec_gate[t] if t else None), o))
    return collect(c, rcs, o, [])


def gated_bwd_steps(c):
    d = dev(c)
    gru = c.cell == "GRU"
    o = outputs(c, BWD_OUT[c.cell] + ("dgate", "cdir0", "cdir1") + (("dcp",) if gru else ()))
    carry_mv = steps_first(c.ref_b["carry_mv"])
    dry = steps_first(c.ref_b["dry"]) if gru else None
    rcs, carry_dir = [], None
    for t in range(c.T - 1, -1, -1):
        outs = dict(o, **d["saves"], carry_dir_out=o[f"cdir{t & 1}"])
        ins = {"g_out": d["g_out"], "carry_mv": carry_mv[t] if t + 1 < c.T else None, "carry_dir": carry_dir}
        if gru:
            rcs.append(gate_step(c, 4, t, ins, outs))
            rcs.append(gate_step(c, 5, t, {"dry": dry[t]}, outs))
        else:
            rcs.append(gate_step(c, 3, t, ins, outs))
        carry_dir = o[f"cdir{t & 1}"]
    # (dgate's second half is the LiGRU's dc_pre / the GRU's dr_pre; one ping-pong buffer stays untouched at T = 1)
    return collect(c, rcs, o, [], scratch=("cdir0", "cdir1"))


def fwd_whole(c, L):
    return rnn_fwd(c, L) if c.cell == "RNN" else gated_fwd(c, L)


def bwd_whole(c, L):
    return rnn_bwd(c, L) if c.cell == "RNN" else gated_bwd(c, L)


def fwd_steps(c):
    return rnn_fwd_steps(c) if c.cell == "RNN" else gated_fwd_steps(c)


def bwd_steps(c):
    return rnn_bwd_steps(c) if c.cell == "RNN" else gated_bwd_steps(c)


# ====================================================================================================== checks
def check_fwd(c, got, path, worst):
    what = f"{c.cell} {c.kind or ''} (B {c.B}, T {c.T}, H {c.H}, dirs {c.dirs}, p {c.p}) {path}"
    for k in FWD_NUM[c.cell]:
        f = within(got[k], c.ref_f[k], c.bound[k], f"{what}: {k}")
        worst[f"{path}_{k}"] = max(worst.get(f"{path}_{k}", 0.0), f)
    # dropout after the cell, directions side by side at the original time index: one fp32 product, bit for bit
    ys = gn.out_layout(got["y_state"], c.B, c.dirs)
    kept = c.mask != 0
    assert not got["y_out"][~kept].any(), f"{what}: y_out is not zero where the mask is"
    assert same_bits(got["y_out"][kept], (ys * c.mask)[kept]), f"{what}: y_out is not y_state * 1/(1-p) where kept"
    if c.p:
        assert 0 < (~kept).sum() < kept.size


def check_bwd(c, got, path, worst):
    what = f"{c.cell} {c.kind or ''} (B {c.B}, T {c.T}, H {c.H}, dirs {c.dirs}, p {c.p}) {path}"
    for k in BWD_NUM[c.cell]:
        f = within(got[k], c.ref_b[k], c.bound[k], f"{what}: {k}")
        worst[f"{path}_{k}"] = max(worst.get(f"{path}_{k}", 0.0), f)
    yprev = got["y_prev" if c.cell == "RNN" else "yprev_all"]
    want = gn.to_original(gn.shift_one_step(c.saves["y_state"]), c.B, c.dirs)
    assert same_bits(yprev, want), f"{what}: yprev is not y_state moved one cell step at the original time index"
    first = [yprev[:c.B, 0]] + ([yprev[c.B:, c.T - 1]] if c.dirs == 2 else [])
    assert all(same_bits(a, np.zeros_like(a)) for a in first), f"{what}: the first step's yprev rows are not +0.0"
    if c.cell == "GRU":
        assert same_bits(got["ry_all"], gn.to_original(c.saves["r_save"], c.B, c.dirs) * want), f"{what}: ry_all"


def identical(a, b, what):
    for k in a:
        if not k.startswith("cdir"):
            assert same_bits(a[k], b[k]), f"{what}: {k} differs from the whole launch"


def run_case(c, chunks, record_property):
    worst = {}
    f0, b0 = fwd_whole(c, c.T), bwd_whole(c, c.T)
    check_fwd(c, f0, "persistent", worst)
    check_bwd(c, b0, "persistent", worst)
    for L in chunks:
        identical(f0, fwd_whole(c, L), f"{c.cell} forward in chunks of {L}")
        identical(b0, bwd_whole(c, L), f"{c.cell} backward in chunks of {L}")
    check_fwd(c, fwd_steps(c), "per_step", worst)
    check_bwd(c, bwd_steps(c), "per_step", worst)
    for k, f in worst.items():
        record_property(f"{k}_err_over_bound", f)
    print(f"{c.cell} {c.kind or ''} B {c.B} T {c.T} H {c.H} dirs {c.dirs} p {c.p}: "
          + ", ".join(f"{k} {f:.3f}" for k, f in worst.items()) + " of the bound")


# ====================================================================================================== a. small shapes
SMALL = [(3, 1, 32), (33, 9, 96), (5, 40, 64)]


@pytest.mark.parametrize("p_drop", [0.0, 0.25])
@pytest.mark.parametrize("dirs", [1, 2])
@pytest.mark.parametrize("B,T,H", SMALL)
@pytest.mark.parametrize("cell,kind", CELLS, ids=CELL_IDS)
def test_small_shapes_every_path_against_fp64(cell, kind, B, T, H, dirs, p_drop, record_property):
    """(3,1,32): a single step, nothing recurrent.  (33,9,96): a ragged second row tile; 3 k-groups for 8 waves (the
    gated kernels) / 4 (the RNN), so some waves hold padding fragments only.  (5,40,64): a long sequence, the hand-off
    ring wraps many times and chunks of 7 leave a short last chunk."""
    run_case(case(cell, kind, B, T, H, dirs, p_drop), (1, 7), record_property)


# ====================================================================================================== b. the benchmark's geometry
def big_shape(cell, name):
    """(B, H, dirs) from the device's CU count, and the row tiles one launch holds.  The gated kernels launch H / 16
    workgroups per row tile, the RNN H / 32; a whole-sequence launch holds cus // that many row tiles of 32 rows."""
    cus = _capi().lib.sparch_device_cus()
    H = 512 if name == "h512" else 1024
    per_launch = cus // (H // (32 if cell == "RNN" else 16))
    assert per_launch >= 1, f"{cus} CUs cannot hold one row tile at H = {H}"
    B, dirs = {"tail_group": (32 * per_launch + (4 if cell == "RNN" else 2), 1),   # groups per_launch + 1, a short last tile
               "h512": (32 * per_launch + 4, 1),
               "boundary": (16 * per_launch + 6, 2),                              # Bp = 32 per_launch + 12
               "full_machine": (16 * per_launch, 2)}[name]                        # Bp = 32 per_launch exactly
    n_rt = -(-B * dirs // 32)
    if name == "full_machine":
        assert n_rt == per_launch and n_rt * (H // 32) <= cus
    else:
        assert n_rt > per_launch, "the shape does not reach a second row-tile group"
    if name == "boundary":
        assert B % 32 != 0, "the direction boundary falls on a row-tile edge"
    return B, H, dirs


BIG = ([("RNN", k, n) for n in ("tail_group", "full_machine") for k in ("sigmoid", "relu", "tanh")]
       + [(cell, None, n) for cell in ("LiGRU", "GRU") for n in ("tail_group", "boundary", "h512")])


@pytest.mark.parametrize("cell,kind,name", BIG, ids=[f"{c}{'_' + k if k else ''}_{n}".lower() for c, k, n in BIG])
def test_benchmark_launch_geometries_against_fp64(cell, kind, name, record_property):
    """With 256 CUs: LiGRU / GRU at H = 1024, B = 130 (5 row tiles in groups 4 + 1, the last tile 2 rows) and B = 70
    bidirectional (Bp = 140: the direction boundary inside a tile), at H = 512, Bp = 260 (9 tiles in groups 8 + 1, two
    k-groups per wave forward and four backward); the RNN at B = 260 (9 tiles in groups 8 + 1) and B = 128
    bidirectional (exactly one full machine of 256 co-resident workgroups).  The second group runs with rt_base > 0 and
    fewer row tiles than the first, while the hand-off rings are laid out for all of them."""
    B, H, dirs = big_shape(cell, name)
    run_case(case(cell, kind, B, 6, H, dirs, 0.1), (2,), record_property)


# ====================================================================================================== c. error codes
def test_error_codes_are_refused_before_any_launch():
    lib = _capi().lib
    for H in (16, 48, 1040):
        for backward in (0, 1):
            assert lib.sparch_ligru_vpack_bytes(H, backward) == 0
            assert all(lib.sparch_gru_vpack_bytes(H, backward, which) == 0 for which in (0, 1))
    for cell in ("LiGRU", "GRU"):
        bad = case(cell, None, 3, 2, 48, 1, 0.0)                       # H % 32 != 0 on the gated entry points
        gated_fwd(bad, 2, expect=EINVAL)
        gated_bwd(bad, 2, expect=EINVAL)
        ok = case(cell, None, 3, 2, 32, 2, 0.25)
        gated_fwd(ok, 2, chan_short=1, expect=EWORKSPACE)              # chan_bytes one byte short
        gated_bwd(ok, 2, chan_short=1, expect=EWORKSPACE)
    rnn = case("RNN", "tanh", 3, 2, 32, 2, 0.25)
    rnn_fwd(rnn, 2, chan_short=1, expect=EWORKSPACE)
    rnn_bwd(rnn, 2, chan_short=1, expect=EWORKSPACE)
    for act in (3, -1):                                                # an unknown activation
        rnn_fwd(rnn, 2, act=act, expect=EINVAL)
        rnn_bwd(rnn, 2, act=act, expect=EINVAL)
        rnn_fwd_steps(rnn, act=act, expect=EINVAL)
        rnn_bwd_steps(rnn, act=act, expect=EINVAL)
    worst = {}                                                         # ... and the same buffers are taken when valid
    check_fwd(rnn, rnn_fwd(rnn, 2), "persistent", worst)
    check_bwd(rnn, rnn_bwd(rnn, 2), "persistent", worst)


# ====================================================================================================== d. the same bits
BITS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "baseline_rec_bits.json")
BITS_B, BITS_T = 33, 6
BITS_H = {96: (2, 0.25), 256: (1, 0.0), 512: (1, 0.0), 1024: (2, 0.25)}        # H -> (dirs, p_drop)


def baseline_bits(cell, kind, H):
    """{"inputs": hash of everything the kernels are given, "fwd.<output>" / "bwd.<output>": hash of that tensor}."""
    dirs, p = BITS_H[H]
    c = case(cell, kind, BITS_B, BITS_T, H, dirs, p)
    bits = {"inputs": sha(*[a for m in sorted(c.X) for a in c.X[m]], *[c.V[m] for m in sorted(c.V)], c.g_out,
                          *[c.saves[k] for k in SAVES[cell]])}
    for name, got in (("fwd", fwd_whole(c, c.T)), ("bwd", bwd_whole(c, c.T))):
        bits.update({f"{name}.{k}": sha(a) for k, a in got.items()})
    return bits


@functools.lru_cache(maxsize=1)
def recorded_bits():
    with open(BITS_FILE) as f:
        return json.load(f)["bits"]


@pytest.mark.parametrize("H", sorted(BITS_H))
@pytest.mark.parametrize("cell,kind", CELLS, ids=CELL_IDS)
def test_whole_launch_outputs_have_the_recorded_bits(cell, kind, H):
    """Forward and backward, one persistent launch over the whole sequence, B = 33 (two row tiles, the second ragged),
    T = 6 (with a ring of 4 slots, slot 0 is reused and the sentinel is put back twice); two directions and p_drop 0.25
    at H = 96 and 1024, one direction without dropout at 256 and 512.  The four H select every instantiation: the gated
    forward with 1, 1, 2, 4 k-groups per wave, the gated backward with 1, 2, 4, 8, the RNN with 4 waves x 1, then
    8 waves x 1, 2, 4.  The kernels fix their reduction order (MFMA terms, k-groups of a wave, waves 0 .. NW-1), the
    dropout mask is a hash of the element index and the inputs come from numpy, so the outputs are reproducible to
    the bit; the fp64 tests above have tolerances and would pass a reordered sum.

    The file was recorded with the build of the commit BEFORE the kernels were rewritten on shared ring helpers, never
    from the code under test.  Re-record it (this module run with python -m, > the file, on the last commit
    whose bits are trusted) only for a new toolchain or a deliberate change of arithmetic, such as fp16 planes, and
    say which in the commit message.  A differing "inputs" hash means that the host-side numpy inputs moved, not a
    kernel."""
    want = recorded_bits()[f"{CELL_IDS[CELLS.index((cell, kind))]}-H{H}"]
    got = baseline_bits(cell, kind, H)
    assert got["inputs"] == want["inputs"], "the numpy inputs differ from the recorded ones (not a kernel's doing)"
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(got) if got[k] != want[k]]
    assert not differ, f"{cell} {kind or ''} H {H}: other bits than recorded in {differ}"


if __name__ == "__main__":
    print(json.dumps({"recorded_with": {"torch": torch.__version__, "hip": torch.version.hip, "numpy": np.__version__,
                                        "device": torch.cuda.get_device_name(0)},
                      "bits": {f"{i}-H{H}": baseline_bits(cell, kind, H) for (cell, kind), i in zip(CELLS, CELL_IDS)
                               for H in sorted(BITS_H)}}, indent=1, sort_keys=True))
