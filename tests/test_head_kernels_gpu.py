"""
The tail of the train step — sparch_adam_step, sparch_adam_scalars (sparch_amd/csrc/optim.hip, sparch_amd/optim.py),
sparch_ce_loss, sparch_act_fwd/_bwd, sparch_softmax_sum_fwd/_bwd (sparch_amd/csrc/act.hip) — called through the C ABI
(through sparch_amd.optim.Adam / sparch_amd.functional where the Python layer is what is tested), outputs prefilled
with NaN, and compared with the fp64 restatements of tests/head_numpy.py (pinned to torch fp64 by
tests/test_head_numpy_host.py):

  a  sparch_adam_step     one step from a shared fp32 state: chunk and thread edges, t, gradient scales, weight decay
                          with g + wd p cancelling, eps; tensor tables around 24 / 48 with empty tensors; the skip
                          word and its counter; scalars_dev; error codes
  b  sparch_adam_scalars  against Python double; graph mode eagerly and replayed from a captured graph, with an lr
                          change, a loaded step count, a skipped step (take_back); mixed steps and two groups (eager)
  c  sparch_ce_loss       rows of 0..3 trips per thread, one class, a long class loop; underflowing, equal, peaked and
                          offset logits; labels out of range; the Python layer's contiguity, fallback and device guard
  d  sparch_act_fwd/_bwd  a second grid-stride trip with a ragged tail, affine or not, dropout masks bit for bit,
                          saturation, zeros, non-finite inputs (also through a LiGRU layer, on both of its paths)
  e  sparch_softmax_sum   slab edges at 1024, the largest K, one step, a long time sum

Every numeric comparison is |got - ref| <= bound with the per-element forward-error bounds of head_numpy (their
constants are four times the worst ratio of a plain fp32 restatement against the same reference — never fitted to
a kernel); each test records the worst fraction of the bound it saw (record_property; DESIGN.md, "Train-step tail
against fp64", has the table measured on an MI355X).  Masks, skip-word no-ops, counters, guard bytes, rows next to
an ignored label and contiguous-versus-strided inputs are compared bit for bit.

Every shape and pointer a kernel gets is valid; the error-code cases are refused on the host before any launch.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import head_numpy as hn
from tests.dropout_numpy import keep_mask
from tests.guarded import embed
from tests.kit import DEV, EALIGN, EINVAL, F32, D, N, nan_, same_bits, within
from tests.kit import Fn as _Fn
from tests.kit import capi as _capi

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def adjacent32(got, want):
    """got (fp32) is fp32(want) or one of its two fp32 neighbours."""
    w = np.float32(want)
    return np.float32(got) in (w, np.nextafter(w, np.float32(np.inf)), np.nextafter(w, np.float32(-np.inf)))


# ================================================================================================ a. sparch_adam_step
def adam_call(ps, gs, ms, vs, numel, s, scalars_dev=None, skip=None, n=None, tables=True):
    """ps .. vs: lists of device tensors (None: a NULL entry); numel: list of ints; s: the scalars of adam_scalars32."""
    c = _capi()
    k = max(len(numel), 1)

    def table(ts):
        return (ctypes.c_void_p * k)(*[None if t is None else t.data_ptr() for t in ts]) if tables else None
    rc = c.lib.sparch_adam_step(len(numel) if n is None else n, table(ps), table(gs), table(ms), table(vs),
                                (ctypes.c_int64 * k)(*numel) if tables else None, float(s["step_size"]),
                                float(s["beta1"]), float(s["beta2"]), float(s["bc2_sqrt"]), float(s["eps"]),
                                float(s["weight_decay"]), c.ptr(scalars_dev), c.ptr(skip), None)
    torch.cuda.synchronize()
    return rc


class AdamTable:
    """A tensor table on the device: p, m, v inside guard bands, g plain; sizes may hold zeros (NULL entries)."""

    def __init__(self, sizes, t, weight_decay, seed, host=None):
        """host: the tensors' (p, g, m, v) themselves (None: drawn from adam_inputs, one draw per tensor)."""
        self.sizes = list(sizes)
        # (element 0 of adam_inputs has g = m = v = 0, a step that changes nothing: a one-element tensor starts at 1)
        self.host = host or [tuple(a[1:] for a in hn.adam_inputs(n + 1, t, weight_decay, seed + 31 * i)) if n else None
                             for i, n in enumerate(sizes)]
        self.p, self.g, self.m, self.v = [], [], [], []
        for h in self.host:
            if h is None:
                for lst in (self.p, self.g, self.m, self.v):
                    lst.append(None)
                continue
            n = h[0].size
            self.p.append(embed(D(h[0], F32).view(1, n), n, 0))
            self.g.append(D(h[1], F32))
            self.m.append(embed(D(h[2], F32).view(1, n), n, 0))
            self.v.append(embed(D(h[3], F32).view(1, n), n, 0))

    def call(self, s, **kw):
        return adam_call(self.p, self.g, self.m, self.v, self.sizes, s, **kw)

    def check_against_reference(self, s, what):
        """Every non-empty tensor stepped exactly once (a second step is thousands of bounds away), g untouched,
        nothing written outside any tensor.  Returns the worst fractions (p, m, v)."""
        worst = [0.0, 0.0, 0.0]
        for i, h in enumerate(self.host):
            if h is None:
                continue
            ref, bound = hn.adam_step_ref(*h, s), hn.adam_bound(*h, s)
            for j, (name, dev) in enumerate((("p", self.p[i]), ("m", self.m[i]), ("v", self.v[i]))):
                worst[j] = max(worst[j], within(N(dev)[0], ref[j], bound[j], f"{what}: tensor {i} ({h[0].size}) {name}'"))
                dev.check(f"{what}: tensor {i} {name}")
            assert same_bits(N(self.g[i]), h[1]), f"{what}: tensor {i}: g changed"
        return worst

    def unchanged(self):
        return all(h is None or (same_bits(N(self.p[i])[0], h[0]) and same_bits(N(self.m[i])[0], h[2])
                                 and same_bits(N(self.v[i])[0], h[3])) for i, h in enumerate(self.host))


@pytest.mark.parametrize("t,weight_decay,eps", list(hn.adam_cases()))
def test_adam_step_one_step_against_fp64(t, weight_decay, eps, record_property):
    """One call on the nine ADAM_SIZES tensors (the host test shows what the state holds: five gradient scales side by
    side, v = 0, g = 0, |g| < eps, moments zero at t = 1, and with weight decay a thousand elements whose g + wd p
    cancels to a few bits).  Kernel and reference start from the same fp32 state, so nothing drifts."""
    (p, g, m, v), _ = hn.adam_table(t, weight_decay)
    s = hn.adam_scalars32(t, eps=eps, weight_decay=weight_decay)
    cuts = np.cumsum(hn.ADAM_SIZES)[:-1]
    tab = AdamTable(hn.ADAM_SIZES, t, weight_decay, 0, host=list(zip(*[np.split(a, cuts) for a in (p, g, m, v)])))
    assert tab.call(s) == 0
    fp, fm, fv = tab.check_against_reference(s, f"t={t} wd={weight_decay} eps={eps}")
    for k, f in (("p", fp), ("m", fm), ("v", fv)):
        record_property(f"adam_{k}_err_over_bound", f)
    print(f"adam t={t} wd={weight_decay} eps={eps}: p {fp:.3f} m {fm:.3f} v {fv:.3f} of the bound")


TABLE_SIZES = (5, 1, 257, 17, 64, 3)


def _layout(name):
    if name.isdigit():
        return [TABLE_SIZES[i % len(TABLE_SIZES)] for i in range(int(name))]
    if name == "empties":                 # empty tensors at table positions 0, 23, 24 and last
        sizes = [TABLE_SIZES[i % len(TABLE_SIZES)] for i in range(51)]
        for i in (0, 23, 24, 50):
            sizes[i] = 0
        return sizes
    return [0] * 5                        # "all_empty"


@pytest.mark.parametrize("layout", ["24", "25", "48", "49", "empties", "all_empty"])
def test_adam_step_tensor_tables(layout, record_property):
    """24 tensors travel per launch: tables of exactly one and two launches, one more than each, empty tensors (NULL
    pointers, numel 0) at the first and last slot of a launch; every non-empty tensor is stepped exactly once."""
    sizes = _layout(layout)
    s = hn.adam_scalars32(2, eps=1e-8)
    tab = AdamTable(sizes, 2, 0.0, 1234)
    skip = torch.zeros(4, dtype=torch.int32, device=DEV)
    assert tab.call(s, skip=skip) == 0
    fr = tab.check_against_reference(s, layout)
    record_property("adam_table_err_over_bound", max(fr))
    print(f"adam table {layout}: {max(fr):.3f} of the bound")
    assert N(skip).tolist() == [0, 0, 0, 0]
    if layout == "all_empty":             # nothing to launch: not even the skip counter moves
        skip[0] = 1
        assert tab.call(s, skip=skip) == 0 and N(skip).tolist() == [1, 0, 0, 0]
        assert adam_call([], [], [], [], [], s, n=0, tables=False) == 0          # n_tensors = 0, NULL tables


def test_adam_step_skip_word_counts_once_per_call():
    """49 tensors are three launches; a raised word makes all of them no-ops and status[1] rises by one per CALL."""
    s = hn.adam_scalars32(2, eps=1e-8, weight_decay=0.01)
    tab = AdamTable(_layout("49"), 2, 0.01, 77)
    skip = torch.tensor([1, 0, 7, 9], dtype=torch.int32, device=DEV)
    assert tab.call(s, skip=skip) == 0
    assert tab.unchanged() and N(skip).tolist() == [1, 1, 7, 9]
    assert tab.call(s, skip=skip) == 0
    assert tab.unchanged() and N(skip).tolist() == [1, 2, 7, 9]
    skip.zero_()
    assert tab.call(s, skip=skip) == 0 and N(skip).tolist() == [0, 0, 0, 0]
    tab.check_against_reference(s, "after the word was cleared")


def test_adam_step_reads_the_device_scalars_when_given():
    s = hn.adam_scalars32(1000, eps=1e-8)
    wrong = dict(s, step_size=np.float32(0.5), bc2_sqrt=np.float32(0.25))
    a, b = AdamTable(_layout("25"), 1000, 0.0, 5), AdamTable(_layout("25"), 1000, 0.0, 5)
    sd = D(np.array([s["step_size"], s["bc2_sqrt"]], dtype=np.float32), F32)
    assert a.call(wrong, scalars_dev=sd) == 0          # the arguments are deliberately different: the pair is used
    a.check_against_reference(s, "scalars_dev")
    assert b.call(wrong) == 0                          # ... and without the pair the arguments are
    b.check_against_reference(wrong, "arguments")
    assert not same_bits(N(a.p[2]), N(b.p[2]))
    c = AdamTable(_layout("25"), 1000, 0.0, 5)
    assert c.call(dict(s, bc2_sqrt=np.float32(0.0)), scalars_dev=sd) == 0        # bc2_sqrt is not looked at then
    assert all(same_bits(N(x), N(y)) for x, y in zip(a.p, c.p))


def test_adam_error_codes():
    s = hn.adam_scalars32(2)
    tab = AdamTable([5, 3], 2, 0.0, 9)
    c = _capi()
    assert tab.call(s, n=-1) == EINVAL
    assert adam_call([], [], [], [], [], s, n=2, tables=False) == EINVAL                      # NULL table, n > 0
    assert adam_call(tab.p, tab.g, tab.m, tab.v, [5, -1], s) == EINVAL                         # negative numel
    assert adam_call([tab.p[0], None], tab.g, tab.m, tab.v, [5, 3], s) == EINVAL               # NULL entry, numel > 0
    assert adam_call(tab.p, tab.g, tab.m, [None, tab.v[1]], [5, 3], s) == EINVAL
    assert tab.call(dict(s, bc2_sqrt=np.float32(0.0))) == EINVAL
    assert tab.call(dict(s, bc2_sqrt=np.float32(-1.0))) == EINVAL
    assert tab.call(dict(s, bc2_sqrt=np.float32(np.nan))) == EINVAL
    assert tab.unchanged()                                                                     # nothing was launched
    t_dev = torch.zeros((), dtype=torch.float64, device=DEV)
    lr_dev = torch.full((), 1e-2, dtype=torch.float64, device=DEV)
    sc = nan_(2)
    for b1, b2 in ((1.0, 0.999), (-0.1, 0.999), (0.9, 1.0), (0.9, -1e-9), (float("nan"), 0.999)):
        assert c.lib.sparch_adam_scalars(c.ptr(t_dev), c.ptr(lr_dev), b1, b2, c.ptr(sc), None) == EINVAL
    assert c.lib.sparch_adam_scalars(None, c.ptr(lr_dev), 0.9, 0.999, c.ptr(sc), None) == EINVAL
    assert c.lib.sparch_adam_scalars(c.ptr(t_dev), None, 0.9, 0.999, c.ptr(sc), None) == EINVAL
    assert c.lib.sparch_adam_scalars(c.ptr(t_dev), c.ptr(lr_dev), 0.9, 0.999, None, None) == EINVAL
    assert float(N(t_dev)) == 0.0 and np.isnan(N(sc)).all()
    assert tab.call(s) == 0


# ============================================================================ b. sparch_adam_scalars, graph mode
@pytest.mark.parametrize("lr", [1e-2, 7e-3])
@pytest.mark.parametrize("t", [0, 1, 999, 99999])
def test_adam_scalars_against_python_double(t, lr):
    """t comes back as t + 1 exactly; each factor is fp32(the Python double) or its fp32 neighbour — the device's
    pow is not the host's, and a double one ulp off can round to the other side of an fp32 boundary; nothing wider."""
    c = _capi()
    t_dev = torch.full((), float(t), dtype=torch.float64, device=DEV)
    lr_dev = torch.full((), lr, dtype=torch.float64, device=DEV)
    sc = nan_(2)
    assert c.lib.sparch_adam_scalars(c.ptr(t_dev), c.ptr(lr_dev), 0.9, 0.999, c.ptr(sc), None) == 0
    t1, step_size, bc2_sqrt = hn.adam_scalars_ref(t, lr, 0.9, 0.999)
    got = N(sc)
    assert float(N(t_dev)) == t1 == t + 1
    assert adjacent32(got[0], step_size), (got[0], step_size)
    assert adjacent32(got[1], bc2_sqrt), (got[1], bc2_sqrt)
    assert float(N(lr_dev)) == lr


OPT_SHAPES = [(300,), (4097,), (17, 5), (1,)]


def _make_opt(lr=1e-2, step0=None, seed=0, groups=None, **kw):
    """sparch_amd.optim.Adam over OPT_SHAPES parameters with static .grad buffers; step0: load a state with that
    step count and populated moments (as a checkpoint would)."""
    from sparch_amd.optim import Adam
    rng = np.random.default_rng(seed)
    params = [torch.nn.Parameter(D(rng.standard_normal(sh), F32)) for sh in OPT_SHAPES]
    for p in params:
        p.grad = torch.zeros_like(p)
    opt = Adam(params if groups is None else groups(params), lr=lr, **kw)
    if step0 is not None:
        steps = step0 if isinstance(step0, (list, tuple)) else [step0] * len(params)
        state = {i: {"step": torch.tensor(float(steps[i])),
                     "exp_avg": D(0.1 * rng.standard_normal(p.shape), F32),
                     "exp_avg_sq": D(0.01 * (rng.random(p.shape) + 0.01), F32)} for i, p in enumerate(params)}
        opt.load_state_dict({"state": state, "param_groups": opt.state_dict()["param_groups"]})
    return opt, params


def _fill_grads(params, seed):
    rng = np.random.default_rng(seed)
    for i, p in enumerate(params):
        p.grad.copy_(D(rng.standard_normal(tuple(p.shape)) * 10.0 ** (i - 1), F32))


def _snapshot(opt, params):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        out.append(tuple(N(x).reshape(-1).copy() for x in (p, p.grad, st.get("exp_avg", torch.zeros_like(p)),
                                                           st.get("exp_avg_sq", torch.zeros_like(p)))))
    return out


def _check_step(opt, params, before, s, what):
    worst = 0.0
    for i, p in enumerate(params):
        ref, bound = hn.adam_step_ref(*before[i], s), hn.adam_bound(*before[i], s)
        st = opt.state[p]
        for j, dev in enumerate((p, st["exp_avg"], st["exp_avg_sq"])):
            worst = max(worst, within(N(dev).reshape(-1), ref[j], bound[j], f"{what}: parameter {i} {'pmv'[j]}'"))
    return worst


def _graph_scalars(opt, t, lr, eps=1e-8, wd=0.0):
    """The device pair of the step just taken — checked against Python double at ordinal t and the lr in force — as
    the reference's scalars (the kernel's fp32 scalars exactly)."""
    got = N(opt._g["scalars"])
    _, step_size, bc2_sqrt = hn.adam_scalars_ref(t - 1, lr, 0.9, 0.999)
    assert adjacent32(got[0], step_size) and adjacent32(got[1], bc2_sqrt), (t, lr, got, step_size, bc2_sqrt)
    return dict(hn.adam_scalars32(t, lr=lr, eps=eps, weight_decay=wd), step_size=got[0], bc2_sqrt=got[1])


def _counters(opt, params):
    return [float(opt.state[p]["step"]) for p in params], float(N(opt._g["t"]))


def _graph_stepper(opt, captured):
    """step() in graph mode: called eagerly, or captured ALONE in a graph (a linear chain: the scalars launch, then
    the Adam launches) and replayed, followed by note_replay() as GraphedTrainStep.step does."""
    if not captured:
        return opt.step
    _Fn().status_word(DEV)                                   # allocated before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()

    def step():
        graph.replay()
        opt.note_replay()
    step.graph = graph
    return step


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "replayed"])
def test_adam_graph_mode_steps_and_lr_change(captured, record_property):
    opt, params = _make_opt(lr=1e-2, step0=99999, seed=3)
    opt.enable_graph_mode()
    assert _counters(opt, params) == ([99999.0] * len(params), 99999.0)       # the device counter starts there
    step = _graph_stepper(opt, captured)
    assert _counters(opt, params) == ([99999.0] * len(params), 99999.0)       # capturing runs nothing
    lr, worst = 1e-2, 0.0
    for i in range(5):
        if i == 2:                                                            # between replays 2 and 3
            lr *= 0.7
            opt.param_groups[0]["lr"] = lr
        opt.sync_lr()
        _fill_grads(params, 100 + i)
        before = _snapshot(opt, params)
        step()
        t = 99999 + i + 1
        worst = max(worst, _check_step(opt, params, before, _graph_scalars(opt, t, lr), f"step {i}"))
        assert _counters(opt, params) == ([float(t)] * len(params), float(t))
        assert float(N(opt._g["lr"])) == lr
    record_property("adam_graph_err_over_bound", worst)
    print(f"adam graph mode {'replayed' if captured else 'eager'}: {worst:.3f} of the bound")


@pytest.mark.parametrize("mode", ["eager", "graph_eager", "graph_replayed"])
def test_adam_skipped_step_is_taken_back(mode, record_property):
    """Status word raised: the step leaves parameters and moments alone, but every counter has moved (the host's
    `step`, and in graph mode the device's t, which sparch_adam_scalars advances whatever the word says).
    poll_status reports one skipped step and Adam.take_back, through the listener, takes it back: the next step's
    bias corrections are those of the t that does not count the skipped one."""
    Fn = _Fn()
    opt, params = _make_opt(lr=1e-2, step0=3, seed=5)
    graph_mode = mode != "eager"
    if graph_mode:
        opt.enable_graph_mode()
    step = _graph_stepper(opt, mode == "graph_replayed") if graph_mode else opt.step
    word = Fn.status_word(DEV)
    word.zero_()

    def scalars(t):
        return _graph_scalars(opt, t, 1e-2) if graph_mode else hn.adam_scalars32(t, lr=1e-2)
    try:
        _fill_grads(params, 1)
        before = _snapshot(opt, params)
        step()
        worst = _check_step(opt, params, before, scalars(4), "step before")
        word[0] = 1
        _fill_grads(params, 2)
        before = _snapshot(opt, params)
        step()
        after = _snapshot(opt, params)
        assert all(same_bits(a, b) for x, y in zip(before, after) for a, b in zip(x, y)), "a skipped step wrote"
        assert N(word).tolist()[:2] == [1, 1]
        assert Fn.poll_status(DEV) is True
        assert Fn.last_timeout["skipped_steps"] == 1
        assert N(word).tolist() == [0, 0, 0, 0]
        assert [float(opt.state[p]["step"]) for p in params] == [4.0] * len(params)            # taken back
        if graph_mode:
            assert float(N(opt._g["t"])) == 4.0
        _fill_grads(params, 3)
        before = _snapshot(opt, params)
        step()
        worst = max(worst, _check_step(opt, params, before, scalars(5), "step after the skipped one"))
        assert [float(opt.state[p]["step"]) for p in params] == [5.0] * len(params)
        if graph_mode:
            assert float(N(opt._g["t"])) == 5.0
        assert Fn.poll_status(DEV) is False
    finally:
        word.zero_()
    record_property("adam_after_skip_err_over_bound", worst)
    print(f"adam around a skipped step ({mode}): {worst:.3f} of the bound")


def test_adam_eager_mixed_steps_and_two_groups(record_property):
    """One group whose parameters hold different `step` values (they joined at different times) and a second group
    with its own lr, eps and weight decay: each parameter is stepped once, with its own factors."""
    def groups(ps):
        return [{"params": ps[:3]}, {"params": ps[3:], "lr": 3e-3, "eps": 1e-3, "weight_decay": 0.01}]
    opt, params = _make_opt(lr=1e-2, step0=[5, 9, 5, 0], seed=7, groups=groups)
    _fill_grads(params, 11)
    before = _snapshot(opt, params)
    opt.step()
    worst = 0.0
    for i, (t, lr, eps, wd) in enumerate([(6, 1e-2, 1e-8, 0.0), (10, 1e-2, 1e-8, 0.0), (6, 1e-2, 1e-8, 0.0),
                                          (1, 3e-3, 1e-3, 0.01)]):
        s = hn.adam_scalars32(t, lr=lr, eps=eps, weight_decay=wd)
        worst = max(worst, _check_step(opt, params[i:i + 1], before[i:i + 1], s, f"parameter {i}"))
        assert float(opt.state[params[i]]["step"]) == t
    record_property("adam_groups_err_over_bound", worst)
    print(f"adam mixed steps / two groups: {worst:.3f} of the bound")


# ================================================================================================ c. sparch_ce_loss
def ce_call(x, y):
    c = _capi()
    B, C = x.shape
    xd, yd = D(x, F32), D(y, np.int64)
    loss, dl = nan_(1), embed(nan_(B, C), C, 0)
    rc = c.lib.sparch_ce_loss(B, C, c.ptr(xd), c.ptr(yd), c.ptr(loss), c.ptr(dl), None)
    torch.cuda.synchronize()
    dl.check(f"dlogits ({B},{C})")
    assert same_bits(N(xd), x)
    return rc, float(N(loss)[0]), N(dl)


@pytest.mark.parametrize("B,C", hn.CE_SHAPES)
def test_ce_loss_against_fp64(B, C, record_property):
    """Thread i owns rows i, i + 256, ...: 0, 1, 2 and 3 trips; a single class; a 1000-class loop.  Every family of
    head_numpy.ce_logits, labels 0 and C - 1 in every case."""
    Fn = _Fn()
    worst = {"loss": 0.0, "dlogits": 0.0, "rowsum": 0.0, "upstream": 0.0}
    for b_, c_, fam, x, y in hn.ce_cases():
        if (b_, c_) != (B, C):
            continue
        rc, loss, dl = ce_call(x, y)
        assert rc == 0
        r, b = hn.ce_ref(x, y), hn.ce_bound(x, y)
        what = f"({B},{C}) {fam}"
        worst["loss"] = max(worst["loss"], within(loss, r["loss"], b["loss"], what + " loss"))
        worst["dlogits"] = max(worst["dlogits"], within(dl, r["dlogits"], b["dlogits"], what + " dlogits"))
        worst["rowsum"] = max(worst["rowsum"], within(dl.astype(np.float64).sum(1), np.zeros(B), b["dlogits"].sum(1),
                                                      what + " sum_c dlogits"))
        # an upstream factor (the regulariser adds to the loss): one more rounding per element
        xd = D(x, F32).requires_grad_(True)
        got = Fn.CrossEntropyLoss()(xd, D(y, np.int64))
        (got * 1.5).backward()
        assert same_bits(N(got).reshape(1), np.float32([loss]))
        worst["upstream"] = max(worst["upstream"], within(N(xd.grad), 1.5 * r["dlogits"],
                                                          1.5 * b["dlogits"] + U * np.abs(1.5 * r["dlogits"]) + hn.TINY,
                                                          what + " upstream factor"))
    for k, f in worst.items():
        record_property(f"ce_{k}_err_over_bound", f)
    print(f"ce ({B},{C}): " + ", ".join(f"{k} {f:.3f}" for k, f in worst.items()) + " of the bound")


@pytest.mark.parametrize("B,C", [(3, 2), (257, 35), (700, 256)])
def test_ce_loss_ignores_labels_out_of_range(B, C, record_property):
    """include/sparch_hip.h: a row whose label is outside [0, C) adds nothing to the loss and has a ZERO gradient row;
    the divisor stays B.  The other rows do not notice: bit-identical to the call with in-range labels there."""
    y = hn.ce_labels(B, C, 5)[0]
    x = hn.ce_logits(B, C, "randn3", y, 6)
    bad = y.copy()
    rows = [1, B - 2] if B > 3 else [1]
    outside = [-100, C, 1 << 32, -1]
    for j, r_ in enumerate(rows):
        bad[r_] = outside[j]
    rc0, loss0, dl0 = ce_call(x, y)
    rc, loss, dl = ce_call(x, bad)
    assert rc0 == 0 and rc == 0
    keep = np.ones(B, bool)
    keep[rows] = False
    assert same_bits(dl[~keep], np.zeros((len(rows), C), np.float32)), "gradient of an ignored row"
    assert same_bits(dl[keep], dl0[keep]), "rows next to an ignored label"
    r, b = hn.ce_ref(x, bad), hn.ce_bound(x, bad)
    record_property("ce_ignored_loss_err_over_bound", within(loss, r["loss"], b["loss"], "loss"))
    np.testing.assert_allclose(r["loss"], hn.ce_ref(x, y)["rows"][keep].sum() * r["inv_b"], rtol=1e-13)   # divisor B
    for lab in (1 << 32, C, -1):                                                   # in every row position of a thread
        allbad = np.full(B, lab, dtype=np.int64)
        rc, loss, dl = ce_call(x, allbad)
        assert rc == 0 and loss == 0.0 and not dl.any()


def test_ce_python_layer_contiguity_fallback_and_device_guard():
    Fn = _Fn()
    B, C = 257, 35
    y = hn.ce_labels(B, C, 7)[0]
    x = hn.ce_logits(B, C, "randn3", y, 8)
    wide = D(np.concatenate([x, -x, x], axis=1), F32)
    y2 = D(np.stack([y, (y + 1) % C], axis=1).reshape(-1), np.int64)

    def run(xt, yt):
        xt = xt.detach().requires_grad_(True)
        loss = Fn.cross_entropy(xt, yt)
        return loss, xt
    l0, x0 = run(D(x, F32), D(y, np.int64))
    l0.backward()
    xs = wide[:, 2 * C:].detach()                    # a column slice and an every-other-element label view
    ys = y2[::2]
    assert not xs.is_contiguous() and not ys.is_contiguous()
    xs.requires_grad_(True)
    l1 = Fn.cross_entropy(xs, ys)
    l1.backward()
    assert same_bits(N(l1).reshape(1), N(l0).reshape(1)) and same_bits(N(xs.grad), N(x0.grad))
    assert type(l0.grad_fn).__name__.startswith("CrossEntropyFn")
    # int32 labels are not the kernel's: torch's own cross_entropy takes over
    try:
        l2, x2 = run(D(x, F32), D(y, np.int32))
    except RuntimeError as e:                         # (torch itself refuses int32 class indices on some builds)
        assert "sparch" not in str(e)
        l2 = None
    if l2 is not None:
        assert not type(l2.grad_fn).__name__.startswith("CrossEntropyFn")
        assert abs(float(l2) - float(l0)) <= 1e-5 * max(1.0, abs(float(l0)))
    with pytest.raises(RuntimeError, match="labels is on 'cpu'"):
        Fn.cross_entropy(D(x, F32).requires_grad_(True), torch.from_numpy(y))
    with pytest.raises(RuntimeError, match="logits is on 'cpu'"):
        Fn.cross_entropy(torch.from_numpy(x).requires_grad_(True), D(y, np.int64))
    c = _capi()
    one = nan_(1)
    assert c.lib.sparch_ce_loss(0, C, c.ptr(wide), c.ptr(y2), c.ptr(one), c.ptr(wide), None) == EINVAL
    assert c.lib.sparch_ce_loss(B, 0, c.ptr(wide), c.ptr(y2), c.ptr(one), c.ptr(wide), None) == EINVAL
    assert c.lib.sparch_ce_loss(B, C, c.ptr(wide), None, c.ptr(one), c.ptr(wide), None) == EINVAL
    torch.cuda.synchronize()
    assert np.isnan(N(one)).all()


# ================================================================================================ d. sparch_act_fwd/_bwd
def act_call(kind, z, sc, sh, dy, p_drop=0.0, seed=0, bwd=False, n=None, H=None, guard=True):
    """z, sc, sh, dy: device tensors (sc, sh, dy may be None).  Returns (rc, output as numpy)."""
    c = _capi()
    M, W = z.shape
    out = embed(nan_(M, W), W, 0) if guard else nan_(M, W)
    k = hn.ACT_KINDS[kind]
    n = M * W if n is None else n
    H = W if H is None else H
    if bwd:
        rc = c.lib.sparch_act_bwd(k, n, H, c.ptr(z), c.ptr(sc), c.ptr(sh), c.ptr(dy), p_drop, seed, c.ptr(out), None)
    else:
        rc = c.lib.sparch_act_fwd(k, n, H, c.ptr(z), c.ptr(sc), c.ptr(sh), p_drop, seed, c.ptr(out), None)
    torch.cuda.synchronize()
    if guard:
        out.check(f"{kind} ({M},{W}) {'dz' if bwd else 'y'}")
    return rc, N(out)


def _act_case(kind, M, H, fam, affine, z, sc, sh, dy, drops, worst):
    zd, dyd = D(z, F32), D(dy, F32)
    scd, shd = (D(sc, F32), D(sh, F32)) if affine else (None, None)
    what = f"{kind} ({M},{H}) {fam} affine={affine}"
    raw = None
    for p_drop, seed in drops:
        mask = keep_mask(seed, (M, H), p_drop) if p_drop else None
        rc, y = act_call(kind, zd, scd, shd, None, p_drop, seed)
        rc2, dz = act_call(kind, zd, scd, shd, dyd, p_drop, seed, bwd=True)
        assert rc == 0 and rc2 == 0
        (ry, rdz), (by, bdz) = hn.act_ref(kind, z, sc, sh, dy, mask), hn.act_bound(kind, z, sc, sh, dy, mask)
        worst["fwd"] = max(worst["fwd"], within(y, ry, by, f"{what} p={p_drop} y"))
        worst["bwd"] = max(worst["bwd"], within(dz, rdz, bdz, f"{what} p={p_drop} dz"))
        if mask is None:
            raw = y
        else:
            # the kernel's own undropped output times the restated mask, one fp32 product: bit for bit
            assert same_bits(y, raw * mask), f"{what} p={p_drop} seed={seed}: y is not raw * keep_mask"
            assert not dz[mask == 0].any(), f"{what} p={p_drop} seed={seed}: the backward's mask differs"
            if M * H >= 1000:
                assert ((mask != 0) & (raw != 0)).sum() >= 100 and ((mask == 0) & (raw != 0)).sum() >= 100
    if fam == "saturated":
        assert np.isfinite(raw).all()
        if kind == "sigmoid":
            assert set(np.unique(np.round(raw, 6)).tolist()) <= {0.0, 1.0}
    if fam == "zeros" and kind == "relu":
        assert (z == 0).sum() >= 2 or M * H < 100
        assert same_bits(raw[z == 0], np.zeros(int((z == 0).sum()), np.float32))      # +0.0 for 0.0 and -0.0 alike


@pytest.mark.parametrize("kind", list(hn.ACT_KINDS))
def test_act_kernels_against_fp64_small_shapes(kind, record_property):
    worst = {"fwd": 0.0, "bwd": 0.0}
    for k, M, H, fam, affine, z, sc, sh, dy in hn.act_cases(hn.ACT_SHAPES[:3]):
        if k == kind:
            _act_case(kind, M, H, fam, affine, z, sc, sh, dy, hn.ACT_DROPS, worst)
    for d, f in worst.items():
        record_property(f"act_{kind}_{d}_err_over_bound", f)
    print(f"act {kind} small: fwd {worst['fwd']:.3f} bwd {worst['bwd']:.3f} of the bound")


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("kind", list(hn.ACT_KINDS))
def test_act_kernels_grid_stride_second_trip(kind, affine, record_property):
    """(8196, 1024): 2,098,176 float4 elements against a grid of 8192 x 256 threads — every thread takes one trip, the
    first 1024 a second one.  One dropout seed here; both seeds run on the small shapes."""
    M, H = hn.ACT_SHAPES[3]
    worst = {"fwd": 0.0, "bwd": 0.0}
    for k, m_, h_, fam, aff, z, sc, sh, dy in hn.act_cases(hn.ACT_SHAPES[3:]):
        if k == kind and aff == affine:
            _act_case(kind, M, H, fam, affine, z, sc, sh, dy, hn.ACT_DROPS[:2], worst)
    for d, f in worst.items():
        record_property(f"act_{kind}_{d}_err_over_bound", f)
    print(f"act {kind} large affine={affine}: fwd {worst['fwd']:.3f} bwd {worst['bwd']:.3f} of the bound")


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("kind", list(hn.ACT_KINDS))
def test_act_kernels_nonfinite_inputs_as_torch(kind, affine):
    """NaN, +inf, -inf at a few elements: the forward output and the backward gradient are NaN exactly where torch
    fp32 on the CPU has NaN (torch.relu hands a NaN on; fmaxf(NaN, 0) = 0 did not)."""
    M, H = 37, 52
    z, sc, sh, dy = hn.act_inputs(M, H, "randn2", affine, 12)
    for i, val in enumerate([np.nan, np.inf, -np.inf] * 3):
        z[(5 * i + 1) % M, (11 * i + 3) % H] = val
    f = {"sigmoid": torch.sigmoid, "relu": torch.relu, "tanh": torch.tanh}[kind]
    zt = torch.from_numpy(z)
    v = (zt * torch.from_numpy(sc) + torch.from_numpy(sh)) if affine else zt.clone()
    v.requires_grad_(True)
    out = f(v)
    out.backward(torch.from_numpy(dy))
    scd, shd = (D(sc, F32), D(sh, F32)) if affine else (None, None)
    rc, y = act_call(kind, D(z, F32), scd, shd, None)
    rc2, dz = act_call(kind, D(z, F32), scd, shd, D(dy, F32), bwd=True)
    assert rc == 0 and rc2 == 0
    want_y, want_dz = np.isnan(out.detach().numpy()), np.isnan(v.grad.numpy())
    assert want_y.sum() >= 3
    assert (np.isnan(y) == want_y).all(), f"{kind}: forward NaN pattern"
    assert (np.isnan(dz) == want_dz).all(), f"{kind}: backward NaN pattern"
    fin = ~want_y & np.isfinite(out.detach().numpy())
    np.testing.assert_allclose(y[fin], out.detach().numpy()[fin], rtol=1e-5, atol=1e-6)
    assert (np.isinf(y) == np.isinf(out.detach().numpy())).all()


@pytest.mark.parametrize("persistent", [True, False], ids=["persistent", "per_step"])
def test_ligru_layer_propagates_nan_of_the_candidate_projection(persistent, monkeypatch):
    """The layer of test_gated_baseline_layers_vs_oracle (LiGRU, bidirectional, batchnorm, its shape) with one NaN in
    the candidate projection's weight: unit j's candidate is relu(NaN) = NaN in the reference (anns.py:458, nn.ReLU),
    so y is NaN in unit j at the first step of either direction and everywhere after it (y_{t-1} V^T) — where the
    oracle's output is NaN ours is, and ours is finite elsewhere; on the persistent kernels (gatedcell.hip) and on the
    launch-per-step path (annstep.hip)."""
    from oracle import ann_oracle as ao
    from sparch_amd import anns
    Fn = _Fn()
    monkeypatch.setenv("SPARCH_LIGRU_PERSISTENT", "1" if persistent else "0")
    monkeypatch.delenv("SPARCH_REC_STEPS_PER_LAUNCH", raising=False)
    B, T, C, H = 10, 19, 36, 64
    torch.manual_seed(23)
    layer = anns.LiGRULayer(C, H, B, dropout=0.0, normalization="batchnorm", use_bias=True, bidirectional=True)
    with torch.no_grad():
        for n in ("norm", "normz"):
            getattr(layer, n).weight.uniform_(0.7, 1.3)
            getattr(layer, n).bias.uniform_(-0.2, 0.2)
        layer.W.weight[5, 3] = float("nan")
    assert layer.uses_persistent_kernel == persistent
    g = torch.Generator().manual_seed(24)
    x = torch.randn(B, T, C, generator=g)
    p = {"ann.0." + k: v.detach().clone() for k, v in layer.state_dict().items() if "num_batches" not in k}
    ref = ao.hidden_layer("LiGRU", x, p, "ann.0", "batchnorm", True, training=True, running=None).detach().numpy()
    y = layer.to(DEV).train()(x.to(DEV))
    assert Fn.check_status() is False
    y = N(y)
    want = np.isnan(ref)
    assert 0 < want.sum() < want.size and not want[:, 0, :H][:, np.arange(H) != 5].any()
    assert (np.isnan(y) == want).all(), f"{int((np.isnan(y) != want).sum())} elements differ in NaN-ness"
    assert np.isfinite(y[~want]).all()
    np.testing.assert_allclose(y[~want], ref[~want], rtol=1e-4, atol=1e-5)


def test_act_error_codes():
    M, H = 6, 8
    z, dy = torch.zeros(M, H, device=DEV), torch.zeros(M, H, device=DEV)
    sc = torch.ones(H, device=DEV)

    def refused(code, *a, **kw):
        rc, out = act_call(*a, guard=False, **kw)
        return rc == code and bool(np.isnan(out).all())
    assert refused(EINVAL, "relu", torch.zeros(4, 6, device=DEV), None, None, None)            # H % 4 != 0
    assert refused(EINVAL, "relu", z, None, None, None, n=M * H - 4)                           # n % H != 0
    assert refused(EINVAL, "relu", z, None, None, None, n=0)
    assert refused(EINVAL, "relu", z, sc, None, None)                                          # only one of scale/shift
    assert refused(EINVAL, "relu", z, None, sc, None)
    assert refused(EINVAL, "tanh", z, None, None, None, bwd=True)                              # backward without dy
    assert refused(EINVAL, "tanh", z, None, None, None, p_drop=1.0)
    assert refused(EINVAL, "tanh", z, None, None, dy, p_drop=-0.1, bwd=True)
    c = _capi()
    out = nan_(M, H)
    assert c.lib.sparch_act_fwd(3, M * H, H, c.ptr(z), None, None, 0.0, 0, c.ptr(out), None) == EINVAL      # kind
    off = embed(z, H, 1)                                                                       # 4 bytes off
    assert refused(EALIGN, "sigmoid", off, None, None, None)
    assert refused(EALIGN, "sigmoid", z, embed(sc.view(1, H), H, 1), sc, None)
    assert refused(EALIGN, "sigmoid", z, None, None, embed(dy, H, 1), bwd=True)
    assert c.lib.sparch_act_fwd(0, M * H, H, c.ptr(z), None, None, 0.0, 0, c.ptr(embed(out, H, 1)), None) == EALIGN
    torch.cuda.synchronize()
    rc, y = act_call("sigmoid", z, None, None, None)
    assert rc == 0 and (y == 0.5).all()


# ================================================================================================ e. softmax-sum
def ss_call(x, g, B=None, T=None, K=None):
    c = _capi()
    b, t, k = x.shape
    out, dx = embed(nan_(b, k), k, 0), embed(nan_(b * t, k), k, 0)
    B, T, K = b if B is None else B, t if T is None else T, k if K is None else K
    rc1 = c.lib.sparch_softmax_sum_fwd(B, T, K, c.ptr(x), c.ptr(out), None)
    rc2 = c.lib.sparch_softmax_sum_bwd(B, T, K, c.ptr(x), c.ptr(g), c.ptr(dx), None)
    torch.cuda.synchronize()
    out.check("softmax_sum out")
    dx.check("softmax_sum dx")
    return rc1, rc2, N(out), N(dx).reshape(b, t, k)


@pytest.mark.parametrize("B,T,K", hn.SS_SHAPES)
def test_softmax_sum_against_fp64(B, T, K, record_property):
    """A thread holds 4 columns per 1024-column slab: K = 1020 / 1024 / 1028 sit either side of the slab edge, 4096 is
    the largest K, T = 1 a single step, T = 1000 a long time sum (accumulated in time order)."""
    worst = {"out": 0.0, "out_sum": 0.0, "dx": 0.0, "dx_sum": 0.0}
    for b_, t_, k_, fam, x, g in hn.ss_cases():
        if (b_, t_, k_) != (B, T, K):
            continue
        rc1, rc2, out, dx = ss_call(D(x, F32), D(g, F32))
        assert rc1 == 0 and rc2 == 0
        (ro, rdx), (bo, bdx) = hn.ss_ref(x, g), hn.ss_bound(x, g)
        what = f"({B},{T},{K}) {fam}"
        worst["out"] = max(worst["out"], within(out, ro, bo, what + " out"))
        worst["dx"] = max(worst["dx"], within(dx, rdx, bdx, what + " dx"))
        worst["out_sum"] = max(worst["out_sum"], within(out.astype(np.float64).sum(1), np.full(B, float(T)), bo.sum(1),
                                                        what + " sum_k out = T"))
        worst["dx_sum"] = max(worst["dx_sum"], within(dx.astype(np.float64).sum(2), np.zeros((B, T)), bdx.sum(2),
                                                      what + " sum_k dx = 0"))
    for k, f in worst.items():
        record_property(f"softmax_sum_{k}_err_over_bound", f)
    print(f"softmax_sum ({B},{T},{K}): " + ", ".join(f"{k} {f:.3f}" for k, f in worst.items()) + " of the bound")


def test_softmax_sum_error_codes():
    c = _capi()
    x, g = torch.zeros(2, 3, 4104, device=DEV), torch.zeros(2, 4104, device=DEV)

    def refused(code, **kw):
        rc1, rc2, out, dx = ss_call(x, g, **kw)
        return rc1 == code and rc2 == code and bool(np.isnan(out).all()) and bool(np.isnan(dx).all())
    assert refused(EINVAL, K=6)                    # K % 4 != 0
    assert refused(EINVAL, K=4100)                 # K > 4096
    assert refused(EINVAL, B=0) and refused(EINVAL, T=0) and refused(EINVAL, K=0)
    xs, gs = torch.zeros(2, 3, 8, device=DEV), torch.zeros(2, 8, device=DEV)
    out, dx = nan_(2, 8), nan_(6, 8)
    xo, go = embed(xs.view(6, 8), 8, 1), embed(gs, 8, 1)                     # 4 bytes off
    assert c.lib.sparch_softmax_sum_fwd(2, 3, 8, c.ptr(xo), c.ptr(out), None) == EALIGN
    assert c.lib.sparch_softmax_sum_fwd(2, 3, 8, c.ptr(xs), c.ptr(embed(out, 8, 1)), None) == EALIGN
    assert c.lib.sparch_softmax_sum_bwd(2, 3, 8, c.ptr(xs), c.ptr(go), c.ptr(dx), None) == EALIGN
    assert c.lib.sparch_softmax_sum_bwd(2, 3, 8, c.ptr(xs), c.ptr(gs), c.ptr(embed(dx, 8, 1)), None) == EALIGN
    torch.cuda.synchronize()
    assert np.isnan(N(out)).all() and np.isnan(N(dx)).all()
    rc1, rc2, o, d = ss_call(xs, gs)
    assert rc1 == 0 and rc2 == 0 and (o == 3 * 0.125).all() and not d.any()
