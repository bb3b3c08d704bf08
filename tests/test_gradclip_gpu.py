"""
Gradient clipping by global norm on the device — sparch_grad_norm, sparch_scale_grads (sparch_amd/csrc/gradclip.hip),
sparch_adam_step_clip (sparch_amd/csrc/optim.hip), sparch_amd.optim.Adam(max_grad_norm=...), optim.clip_grad_norm_,
SPARCH_CLIP_GRAD — against the restatement of tests/clip_numpy.py (pinned to torch by tests/test_gradclip_host.py):

   1  the norm and every tensor's own norm within 2 u relative of float64 (derived in clip_numpy); zeros; 1e20 everywhere
   2  the same table gives the same bits twice, and the same bits when the 4-byte aligned view is moved to a 16-byte
      aligned buffer
   3  the coefficient is coef_f32 of the device's own norm, bit for bit (max_norm above, below, inf)
   4  sparch_adam_step_clip == sparch_adam_step on fp32(g * coef), bit for bit; the gradients are not written
   5  a NaN / +inf / -inf gradient: flag, counters, untouched p / m / v, the tensor named by tensor_norms; the status word
   6  footprint under tests/guarded.py arenas
   7  sparch_scale_grads and optim.clip_grad_norm_
   8  optim.Adam(max_grad_norm=c), three steps against head_numpy.adam_step_ref; clip_stats, sync_skipped
   9  a captured step (GraphedTrainStep) against eager steps, bit for bit
  10  run_exp.py with and without SPARCH_CLIP_GRAD

The tables: head_numpy.ADAM_SIZES repeated to 25 and 49 tensors (24 travel per launch), two empty tensors (numel 0,
NULL pointers) in the middle, one gradient a view at element offset 1 of a larger buffer (4-byte aligned, not 16), the
values of head_numpy.adam_inputs (five scales from 1e-12 to 1e12 side by side).  Every shape and pointer a kernel gets
is valid; refusals are tested on the host (tests/test_gradclip_host.py).
"""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import clip_numpy as cn
from tests import head_numpy as hn
from tests.guarded import guard_arena
from tests.kit import DEV, F32, F64, D, N, bits, same_bits, sp, within  # noqa: F401  (sp: a fixture)
from tests.kit import capi as _capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
NAN = float("nan")


def _table(ts):
    return (ctypes.c_void_p * max(len(ts), 1))(*[None if t is None else t.data_ptr() for t in ts])


def _numel(sizes):
    return (ctypes.c_int64 * max(len(sizes), 1))(*sizes)


def _plain(n):
    return torch.empty(n, dtype=torch.float32, device=DEV)


class Table:
    """A tensor table on the device from the host arrays of clip_numpy.clip_table; the gradient of slot `self.u` is a
    view at element offset 1 of a larger buffer (aligned=True: an ordinary tensor instead).  alloc(n) -> fp32 tensor."""

    def __init__(self, host, alloc=_plain, aligned=False):
        self.host, self.alloc = host, alloc
        self.sizes = [0 if h is None else int(h[0].size) for h in host]
        self.u = cn.unaligned_slot(host)
        self.p, self.g, self.m, self.v = [], [], [], []
        for i, h in enumerate(host):
            if h is None:
                for lst in (self.p, self.g, self.m, self.v):
                    lst.append(None)
                continue
            n = h[0].size
            for lst, a in ((self.p, h[0]), (self.m, h[2]), (self.v, h[3])):
                t = alloc(n)
                t.copy_(D(a, F32))
                lst.append(t)
            if i == self.u and not aligned:
                buf = self.ubuf = alloc(n + 7)
                buf.fill_(NAN)
                g = buf[1:1 + n]
                assert g.data_ptr() % 16 == 4
            else:
                g = alloc(n)
                assert g.data_ptr() % 16 == 0
            g.copy_(D(h[1], F32))
            self.g.append(g)
        c = _capi()
        self.ws_bytes = int(c.lib.sparch_grad_norm_ws_bytes(len(self.sizes), _numel(self.sizes)))
        self.ws = alloc((self.ws_bytes + 3) // 4)
        self.ws.fill_(NAN)
        self.clip = alloc(8).view(torch.int32).zero_()
        self.norms = alloc(max(len(self.sizes), 1)).fill_(NAN)

    def set_grads(self, arrays):
        for g, a in zip(self.g, arrays):
            if g is not None:
                g.copy_(D(a, F32))

    def norm(self, max_norm, skip=None, norms=True):
        c = _capi()
        rc = c.lib.sparch_grad_norm(len(self.sizes), _table(self.g), _numel(self.sizes), float(max_norm),
                                    self.ws.data_ptr(), self.ws_bytes, self.clip.data_ptr(),
                                    self.norms.data_ptr() if norms else None, c.ptr(skip), None)
        torch.cuda.synchronize()
        assert rc == 0
        return self.state()

    def state(self):
        w = bits(self.clip)
        f = w.view(F32)
        return dict(norm=f[0], coef=f[1], flag=int(w[2]), skipped=int(w[3]), steps=int(w[4]), clipped=int(w[5]),
                    max=f[6], reserved=int(w[7]), words=w.copy())

    def step(self, s, clip=True, scalars_dev=None, skip=None):
        """sparch_adam_step_clip with this table's clip state (clip=False: sparch_adam_step)."""
        c = _capi()
        head = (len(self.sizes), _table(self.p), _table(self.g), _table(self.m), _table(self.v), _numel(self.sizes),
                float(s["step_size"]), float(s["beta1"]), float(s["beta2"]), float(s["bc2_sqrt"]), float(s["eps"]),
                float(s["weight_decay"]), c.ptr(scalars_dev), c.ptr(skip))
        if clip:
            rc = c.lib.sparch_adam_step_clip(*head, self.clip.data_ptr(), None)
        else:
            rc = c.lib.sparch_adam_step(*head, None)
        torch.cuda.synchronize()
        assert rc == 0

    def scale(self):
        rc = _capi().lib.sparch_scale_grads(len(self.sizes), _table(self.g), _numel(self.sizes), self.clip.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == 0

    def pmv(self):
        return [None if t is None else N(t).copy() for lst in (self.p, self.m, self.v) for t in lst]

    def grads(self):
        return [None if g is None else N(g).copy() for g in self.g]


def _same_lists(a, b):
    return len(a) == len(b) and all((x is None and y is None) or same_bits(x, y) for x, y in zip(a, b))


def _check_norms(tab, st, what):
    grads = tab.grads()
    ref = cn.norm_ref(grads)
    worst = within(st["norm"], ref, cn.NORM_U * ref + cn.TINY, f"{what}: global norm")
    per = N(tab.norms)
    for i, g in enumerate(grads):
        r = cn.norm_ref([g])
        if g is None:
            assert per[i] == 0.0 and not np.signbit(per[i]), f"{what}: empty tensor {i}"
        else:
            worst = max(worst, within(per[i], r, cn.NORM_U * r + cn.TINY, f"{what}: tensor {i} ({g.size})"))
    return worst


# ================================================================================================== 1. the norm
@pytest.mark.parametrize("n_tensors", [9, 25, 49])
def test_norm_against_float64(n_tensors, record_property):
    tab = Table(cn.clip_table(n_tensors, seed=n_tensors))
    st = tab.norm(1.0)
    record_property("worst_fraction_of_bound", round(_check_norms(tab, st, f"{n_tensors} tensors"), 3))
    assert st["flag"] == 0 and st["steps"] == 1 and st["skipped"] == 0 and st["reserved"] == 0
    assert st["clipped"] == 1 and st["coef"] < 1.0 and same_bits(st["max"], st["norm"])


def test_norm_of_zeros_is_zero_and_the_coefficient_exactly_one():
    tab = Table(cn.clip_table(25, fill=0.0))
    st = tab.norm(0.5)
    assert same_bits(st["norm"], F32(0.0)) and same_bits(st["coef"], F32(1.0))
    assert st["flag"] == 0 and st["steps"] == 1 and st["clipped"] == 0
    assert not N(tab.norms).any()
    c = _capi()                                                       # n_tensors == 0: a valid call, norm 0, coef 1
    clip = torch.full((8,), 5, dtype=torch.int32, device=DEV)
    assert c.lib.sparch_grad_norm(0, None, None, 0.25, None, 0, clip.data_ptr(), None, None, None) == 0
    w = N(clip).view(np.uint32)
    assert same_bits(w[:2].view(F32), np.array([0.0, 1.0], F32)) and w[2] == 0 and w[3] == 5 and w[4] == 6 and w[7] == 0


def test_norm_of_1e20_everywhere_is_finite():
    """The sum of squares (1e40 a term) is past fp32: what the double accumulation is for."""
    tab = Table(cn.clip_table(25, fill=1e20))
    st = tab.norm(1.0)
    assert np.isfinite(st["norm"]) and st["flag"] == 0 and st["skipped"] == 0 and st["clipped"] == 1
    _check_norms(tab, st, "1e20 everywhere")


# ================================================================================================== 2. reproducible
def test_same_table_same_bits_whatever_the_alignment():
    host = cn.clip_table(49, seed=5)
    tab = Table(host)
    a = tab.norm(1.0)
    per_a = N(tab.norms).copy()
    tab.ws.fill_(NAN)
    tab.norms.fill_(NAN)
    b = tab.norm(1.0)
    assert same_bits(a["norm"], b["norm"]) and same_bits(per_a, N(tab.norms))
    # the view moved to a 16-byte aligned tensor (the kernel may then read it with 16-byte loads): the same bits still,
    # which is what lets replicas whose allocators differ take the same decisions
    other = Table(host, aligned=True)
    c = other.norm(1.0)
    assert same_bits(a["norm"], c["norm"]) and same_bits(per_a, N(other.norms))


# ================================================================================================== 3. the coefficient
def test_coefficient_is_three_fp32_operations_on_the_device_norm():
    tab = Table(cn.clip_table(25, seed=2))
    ref = cn.norm_ref(tab.grads())
    for max_norm, clips in ((ref * 4.0, False), (ref / 7.0, True), (1.0, True), (float("inf"), False)):
        st = tab.norm(max_norm)
        want = cn.coef_f32(st["norm"], max_norm)
        assert same_bits(st["coef"], want), (max_norm, st["coef"], want)
        assert (st["coef"] < 1.0) == clips
        if not clips:
            assert same_bits(st["coef"], F32(1.0))                    # above the norm: exactly 1.0
    assert tab.state()["steps"] == 4 and tab.state()["clipped"] == 2


# ================================================================================================== 4. the fused step
@pytest.mark.parametrize("on_device", [False, True], ids=["arguments", "scalars_dev"])
@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
@pytest.mark.parametrize("t", [1, 1000])
def test_fused_step_is_the_plain_step_on_scaled_gradients(t, weight_decay, on_device):
    host = cn.clip_table(25, t=t, weight_decay=weight_decay, seed=100 + t)
    s = hn.adam_scalars32(t, eps=1e-8, weight_decay=weight_decay)
    sd = None
    if on_device:                                                     # the arguments are then deliberately wrong
        sd = D(np.array([s["step_size"], s["bc2_sqrt"]], dtype=F32), F32)
        s = dict(s, step_size=F32(0.5), bc2_sqrt=F32(0.25))
    ref_norm = cn.norm_ref([None if h is None else h[1] for h in host])
    for max_norm in (ref_norm / 5.0, float("inf")):
        fused, plain = Table(host), Table(host)
        st = fused.norm(max_norm)
        coef = st["coef"]
        assert (coef < 1.0) == (max_norm != float("inf")) and (coef < 1.0 or same_bits(coef, F32(1.0)))
        g_before = fused.grads()
        # the product in fp32, formed by numpy (coef == 1: g itself)
        plain.set_grads([None if g is None else (g * coef).astype(F32) for g in g_before])
        fused.step(s, scalars_dev=sd)
        plain.step(s, clip=False, scalars_dev=sd)
        assert _same_lists(fused.pmv(), plain.pmv()), (t, weight_decay, max_norm)
        assert not _same_lists(fused.pmv(), Table(host).pmv())          # (something was stepped)
        assert _same_lists(fused.grads(), g_before)                     # the fused path never writes gradients


# ================================================================================================== 5. non-finite
def _poison(tab, case):
    """Returns the slot that holds the value."""
    if case == "nan_last":                                            # the tail of the last workgroup's chunk
        i = max(k for k, g in enumerate(tab.g) if g is not None)
        tab.g[i][-1] = NAN
    elif case == "inf_first":
        i = min(k for k, g in enumerate(tab.g) if g is not None)
        tab.g[i][0] = float("inf")
    else:                                                             # inside the unaligned view
        i = tab.u
        tab.g[i][2049] = -float("inf")
    return i


@pytest.mark.parametrize("case", ["nan_last", "inf_first", "neg_inf_unaligned"])
def test_non_finite_gradient_skips_the_step_on_the_device(case):
    tab = Table(cn.clip_table(49, seed=9))                            # three launches
    s = hn.adam_scalars32(2, eps=1e-8)
    before = tab.norm(1.0)                                            # a finite step first: words 4-6 hold something
    assert (before["steps"], before["clipped"], before["skipped"]) == (1, 1, 0) and before["max"] > 0
    slot = _poison(tab, case)
    state0 = tab.pmv()
    st = tab.norm(1.0)
    assert st["flag"] == 1 and not np.isfinite(st["norm"])
    assert st["skipped"] == before["skipped"] + 1                     # once per step, not per launch
    assert (st["words"][4:7] == before["words"][4:7]).all()
    per = N(tab.norms)
    assert [i for i in range(len(per)) if not np.isfinite(per[i])] == [slot]
    skip = torch.zeros(4, dtype=torch.int32, device=DEV)
    tab.step(s, skip=skip)
    assert _same_lists(tab.pmv(), state0) and N(skip).tolist() == [0, 0, 0, 0]
    assert tab.state()["skipped"] == before["skipped"] + 1            # the step kernels count nothing
    st = tab.norm(1.0)                                                # the next bad step counts again
    assert st["skipped"] == before["skipped"] + 2 and (st["words"][4:7] == before["words"][4:7]).all()


def test_raised_status_word_keeps_todays_behaviour():
    tab = Table(cn.clip_table(49, seed=10))
    s = hn.adam_scalars32(2, eps=1e-8, weight_decay=0.01)
    before = tab.norm(1.0)
    state0 = tab.pmv()
    skip = torch.tensor([1, 0, 7, 9], dtype=torch.int32, device=DEV)
    st = tab.norm(1.0, skip=skip)                                     # finite gradients, a timed-out step
    assert same_bits(st["coef"], F32(1.0)) and st["flag"] == 0
    assert (st["words"][3:7] == before["words"][3:7]).all()
    tab.step(s, skip=skip)
    assert _same_lists(tab.pmv(), state0) and N(skip).tolist() == [1, 1, 7, 9]     # + 1 once per call
    tab.step(s, skip=skip)
    assert _same_lists(tab.pmv(), state0) and N(skip).tolist() == [1, 2, 7, 9]
    # the status word comes first: with a non-finite norm as well the skipped step is still counted in status[1]
    _poison(tab, "nan_last")
    assert tab.norm(1.0)["flag"] == 1
    tab.step(s, skip=skip)
    assert _same_lists(tab.pmv(), state0) and N(skip).tolist() == [1, 3, 7, 9]


# ================================================================================================== 6. footprint
def test_footprint_of_the_three_entries():
    """Every tensor, the workspace (exactly its query's bytes), the 8 words and tensor_norms are exact-size slices of a
    guard arena: nothing else is written."""
    host = cn.clip_table(49, seed=11)
    s = hn.adam_scalars32(2, eps=1e-8)
    with guard_arena(None, nbytes=16 << 20) as arena:
        tab = Table(host, alloc=lambda n: arena.empty(n, dtype=torch.float32))
        assert arena.nbytes_of(tab.ws) == tab.ws_bytes and tab.ws.data_ptr() % 8 == 0
        g0 = tab.grads()
        st = tab.norm(cn.norm_ref(g0) / 3.0)
        assert st["coef"] < 1.0
        tab.step(s)
        assert _same_lists(tab.grads(), g0)
        tab.scale()
        buf = N(tab.ubuf)
        assert np.isnan(buf[0]) and np.isnan(buf[-6:]).all()          # around the 4-byte aligned view
        assert not _same_lists(tab.grads(), g0)
    assert len(arena.allocs) >= 4 * 47


# ================================================================================================== 7. scale, clip_grad_norm_
def test_scale_grads_multiplies_in_place_and_leaves_non_finite_alone():
    tab = Table(cn.clip_table(25, seed=12))
    g0 = tab.grads()
    coef = tab.norm(cn.norm_ref(g0) / 2.5)["coef"]
    assert coef < 1.0
    tab.scale()
    assert _same_lists(tab.grads(), [None if g is None else (g * coef).astype(F32) for g in g0])
    _poison(tab, "neg_inf_unaligned")
    g1 = tab.grads()
    assert tab.norm(1.0)["flag"] == 1
    tab.scale()
    assert _same_lists(tab.grads(), g1)                               # (torch would have written NaN everywhere)


def test_clip_grad_norm_function():
    from sparch_amd.optim import clip_grad_norm_
    tab = Table(cn.clip_table(9, seed=13), aligned=True)
    g0 = tab.grads()
    want = tab.norm(1.0)
    per_want = N(tab.norms).copy()
    params = [torch.nn.Parameter(p) for p in tab.p] + [torch.nn.Parameter(torch.zeros(3, device=DEV))]    # one without grad
    for p, g in zip(params, tab.g):
        p.grad = g
    norm, per = clip_grad_norm_(params, 1.0, tensor_norms=True)
    assert norm.is_cuda and norm.ndim == 0 and norm.dtype == torch.float32 and per.is_cuda
    assert same_bits(N(norm), want["norm"]) and same_bits(N(per), per_want)
    assert _same_lists(tab.grads(), [(g * want["coef"]).astype(F32) for g in g0])
    again = clip_grad_norm_(params[0], float("inf"))                  # one tensor; inf: measure only
    assert again.is_cuda and float(again) == pytest.approx(cn.norm_ref([N(tab.g[0])]), rel=4 * U)
    with pytest.raises(ValueError):
        clip_grad_norm_(params, 0.0)


# ================================================================================================== 8. the optimizer
def test_optimizer_three_clipped_steps_then_a_nan(record_property):
    """Adam(max_grad_norm=c), c below every step's norm, fresh gradients per step.  Each step starts, for the
    reference, from the device's own fp32 state (nothing drifts) and is fed g * coef_device, the product in float64;
    the bound is adam_bound on the same inputs with u |g coef| added to the gradient magnitude (the one extra rounding
    of the kernel's fp32 product)."""
    from sparch_amd.optim import Adam
    c = 1.0
    host = cn.clip_table(9, seed=21)
    params = [torch.nn.Parameter(D(h[0], F32)) for h in host]
    opt = Adam(params, hn.ADAM_LR, max_grad_norm=c)
    worst = 0.0
    for step in (1, 2, 3):
        grads = [h[1] for h in cn.clip_table(9, seed=1000 * step)]
        assert cn.norm_ref(grads) > 10 * c
        for p, g in zip(params, grads):
            p.grad = D(g, F32)
        state0 = [(N(p).copy(), N(opt.state[p]["exp_avg"]).copy() if step > 1 else np.zeros(p.numel(), F32),
                   N(opt.state[p]["exp_avg_sq"]).copy() if step > 1 else np.zeros(p.numel(), F32)) for p in params]
        opt.step()
        stats = opt.clip_stats()
        coef = stats["coef"]
        want = cn.coef_ref(cn.norm_ref(grads), c)
        assert abs(coef - want) <= 4 * U * want, (coef, want)         # 2 u from the norm, two roundings
        s = hn.adam_scalars32(step, lr=hn.ADAM_LR)
        for p, g, (p0, m0, v0) in zip(params, grads, state0):
            gc = g.astype(F64) * float(coef)
            ref = hn.adam_step_ref(p0, gc, m0, v0, s)
            bound = hn.adam_bound(p0, gc * (1.0 + U), m0, v0, s)      # G + u |g coef|
            got = (N(p), N(opt.state[p]["exp_avg"]), N(opt.state[p]["exp_avg_sq"]))
            for name, a, r, b in zip("pmv", got, ref, bound):
                worst = max(worst, within(a, r, b, f"step {step}, tensor of {g.size}: {name}'"))
            assert same_bits(N(p.grad), g)                            # the gradients are read, never rewritten
    record_property("worst_fraction_of_bound", round(worst, 3))
    stats = opt.clip_stats()
    assert (stats["steps"], stats["clipped"], stats["skipped"], stats["nonfinite"]) == (3, 3, 0, False)
    assert opt.sync_skipped() == 0
    before = [N(p).copy() for p in params]
    params[4].grad[7] = NAN
    opt.step()
    assert all(float(opt.state[p]["step"]) == 4.0 for p in params)    # the host does not know yet
    assert opt.sync_skipped() == 1 and opt.sync_skipped() == 0
    assert all(float(opt.state[p]["step"]) == 3.0 for p in params)
    assert all(same_bits(N(p), b) for p, b in zip(params, before))
    stats = opt.clip_stats()
    assert (stats["steps"], stats["clipped"], stats["skipped"], stats["nonfinite"]) == (3, 3, 1, True)


# ================================================================================================== 9. a captured step
def test_captured_clipped_step_matches_eager_steps(sp):
    """GraphedTrainStep with a clipped optimizer, three replays, against three eager clipped steps from the same
    start, the same drawn states and the same batch: bit for bit.  Both optimizers are in graph mode (the per-step
    factors come from sparch_adam_scalars on the device either way; the host path rounds them from Python doubles),
    one of them captured, the other not."""
    from sparch_amd.graph import GraphedTrainStep
    from sparch_amd.optim import Adam
    from tests.kit import Fn

    B, T, C, sizes, c = 4, 20, 12, [16, 16, 5], 1e-4
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(B, T, C, generator=g) < 0.3).float().to(DEV)
    y = torch.randint(0, sizes[-1], (B,), generator=g).to(DEV)

    def make():
        torch.manual_seed(11)
        net = sp.SNN((B, None, C), sizes, neuron_type="LIF", dropout=0.0).to(DEV).train()
        return net, Adam(net.parameters(), 1e-2, max_grad_norm=c)

    loss_fn = torch.nn.CrossEntropyLoss()
    net_c, opt_c = make()
    torch.manual_seed(77)
    gs = GraphedTrainStep(net_c, opt_c, loss_fn, x, y, warmup=0)
    try:
        for _ in range(3):
            gs.step()
        Fn().check_status()
        stats = opt_c.clip_stats()
        assert (stats["steps"], stats["clipped"], stats["skipped"]) == (3, 3, 0) and stats["coef"] < 1.0
    finally:
        gs.close()
    # the eager twin: construction of the graphed step consumed two forwards' worth of draws (tests/test_hip_parity.py)
    net_d, opt_d = make()
    torch.manual_seed(77)
    net_d.draw_states(B, torch.device(DEV))
    net_d.draw_states(B, torch.device(DEV))
    opt_d.enable_graph_mode()
    try:
        for _ in range(3):
            opt_d.zero_grad(set_to_none=True)
            out, _ = net_d(x)
            loss_fn(out, y).backward()
            opt_d.step()
        Fn().check_status()
    finally:
        opt_d._g = None
    assert opt_d.clip_stats()["clipped"] == 3
    assert same_bits(F32(opt_d.clip_stats()["norm"]), F32(stats["norm"]))
    for (k, pa), pb in zip(net_d.named_parameters(), net_c.parameters()):
        assert same_bits(N(pa), N(pb)), k


# ================================================================================================== 10. run_exp.py
@pytest.mark.parametrize("clip", ["0.5", None])
def test_run_exp_logs_the_grad_norm_line_only_when_switched_on(tmp_path, clip):
    exp = tmp_path / "exp"
    env = {k: v for k, v in os.environ.items() if k != "SPARCH_CLIP_GRAD"}
    if clip is not None:
        env["SPARCH_CLIP_GRAD"] = clip
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_exp.py"), "--model_type", "LIF", "--nb_layers", "3",
                        "--nb_hiddens", "128", "--dataset_name", "shd", "--batch_size", "4", "--nb_epochs", "1",
                        "--synthetic", "1", "--synthetic_batches", "4", "--save_best", "0", "--log_tofile", "1",
                        "--new_exp_folder", str(exp)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    log = (exp / "log" / "exp.log").read_text()
    assert "Epoch 1: train loss=" in log
    if clip is None:
        assert "grad norm" not in log and "SPARCH_CLIP_GRAD" not in log
        return
    assert "(SPARCH_CLIP_GRAD)" in log
    line = next(ln for ln in log.splitlines() if "Epoch 1: grad norm max=" in ln)
    m = re.search(r"clipped (\d+) of (\d+) steps, skipped 0 non-finite", line)
    assert m and 0 <= int(m.group(1)) <= int(m.group(2)) and int(m.group(2)) >= 1, line
    assert math.isfinite(float(line.split("max=")[1].split(",")[0]))
