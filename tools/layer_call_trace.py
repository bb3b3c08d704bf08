#!/usr/bin/env python3
"""Which C-ABI calls the layer passes of sparch_amd.functional / streaming issue, in order, with their arguments.

    python tools/layer_call_trace.py            print the trace
    python tools/layer_call_trace.py --check    unified diff against tests/golden/layer_call_trace.txt.gz (exit 1 if any)
    python tools/layer_call_trace.py --write    regenerate that file (7 003 lines of text in 214 cases, kept gzipped: 60 KB)

Nothing runs on a device: the layer Functions are driven forward and backward on CPU tensors while
  * `functional.lib` / `streaming.lib` are a stand-in that logs every launching `sparch_*` call and returns 0, forwards
    the pure host queries (every `*_bytes` function) to the real library and answers `sparch_device_cus` with 256,
  * `ptr` hands the stand-in the tensor instead of its address, `_stream()` is None, `_require_device` and
    `snns._check_bidir_input` let CPU tensors through, SNN.forward draws its initial states with torch.rand
    (`snns._fast_rand_ok` is False), and `functional.timer` logs the labels it is started with (bench.py keys its
    roofline on them).
A line holds the entry point and every argument in the order of `_capi.PROTOTYPES`, which also tells pointers from
numbers.  A pointer is NULL or `dtype[shape]/(strides)#n+offset`: strides only when not contiguous, n the number of the
tensor's allocation in order of first appearance within the case (two arguments with one n alias), never an address.
Host arrays of pointers show their NULL pattern, host arrays of floats their values.  What the library derives from the
device — workspace and channel byte counts — appears as the number of the query (`q3`), the query itself being logged
with its arguments (numbered within the case); a buffer sized from it shows that name in place of its shape.  So the
file is the same on every machine, and a change to the host code that leaves it alone issues the same calls on the
same operands.

Values are never looked at, so every case uses the smallest shape at which its branch is taken.  SyncBN needs a process
group and is not traced.  The first 123 cases (3 447 lines) are the dense layer passes; the 91 behind them are what the
spiking layer path gained since: `lengths` / packed / bidirectional-ragged layouts, smooth surrogates, stateful
training, the selectable and per-step readouts, axonal delays, synaptic currents and the row movers.  New cases go to
the end, so that the text in front of them stays byte for byte what it was."""
import contextlib
import ctypes
import difflib
import gzip
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sparch_amd import _capi  # noqa: E402
from sparch_amd import functional as Fn  # noqa: E402
from sparch_amd import snns, streaming  # noqa: E402

TRACE_FILE = os.path.join(ROOT, "tests", "golden", "layer_call_trace.txt.gz")
ENV_SWITCHES = ("SPARCH_REC_STEP_PATH", "SPARCH_REC_STEPS_PER_LAUNCH", "SPARCH_LIGRU_PERSISTENT",
                "SPARCH_GRU_PERSISTENT")
DTYPE = {torch.float32: "f32", torch.bfloat16: "bf16", torch.int32: "i32", torch.int64: "i64", torch.uint8: "u8"}


class _Q(int):
    """A number the library derived from the device: behaves as that number, is logged as the query's name."""

    def __new__(cls, value, tag):
        q = super().__new__(cls, value)
        q.tag = tag
        return q

    def _derived(self, value):
        return _Q(value, self.tag if self.tag.startswith("~") else "~" + self.tag)

    def __floordiv__(self, o):
        return self._derived(int(self) // o)

    def __add__(self, o):
        return self._derived(int(self) + o)

    __radd__ = __add__

    def __lt__(self, o):  # max(q, 16) keeps q whatever the device's number is: the buffer stays tied to the query
        return False

    __hash__ = int.__hash__


class _Recorder:
    def __init__(self):
        self.lines = []
        self.new_case("")

    def new_case(self, name):
        self.allocs, self.keep, self.queries = {}, [], 0
        if name:
            self.lines.append(f"== {name}")

    def tensor(self, t):
        if t.numel() == 0 and getattr(t, "_trace_size", None) is None:
            return f"{DTYPE[t.dtype]}[{','.join(map(str, t.shape))}]"
        st = t.untyped_storage()
        n = self.allocs.get(st.data_ptr())
        if n is None:
            n = self.allocs[st.data_ptr()] = len(self.allocs)
            self.keep.append(st)  # a live allocation's address is not handed out again
        shape = getattr(t, "_trace_size", None) or ",".join(map(str, t.shape))
        s = f"{DTYPE[t.dtype]}[{shape}]"
        if not t.is_contiguous():
            s += "/(" + ",".join(map(str, t.stride())) + ")"
        s += f"#{n}"
        if t.storage_offset():
            s += f"+{t.storage_offset()}"
        return s

    def arg(self, a, ctype):
        if ctype is _capi.P:
            if a is None:
                return "NULL"
            if torch.is_tensor(a):
                return self.tensor(a)
            if isinstance(a, ctypes.Array):
                if a._type_ is ctypes.c_float:
                    return "{" + ",".join(repr(float(v)) for v in a) + "}"
                return "{" + ",".join("NULL" if not v else "*" for v in a) + "}"
            return "*" if a else "NULL"
        if isinstance(a, _Q):
            return a.tag
        if ctype in (ctypes.c_float, ctypes.c_double):
            return repr(float(a))
        return str(int(a))

    def call(self, name, args):
        types = _capi.PROTOTYPES[name][1]
        assert len(args) == len(types), f"{name}: {len(args)} arguments for {len(types)} parameters"
        return f"{name}(" + ", ".join(self.arg(a, c) for a, c in zip(args, types)) + ")"


class _Lib:
    """Stand-in for the ctypes library object."""

    def __init__(self, rec, real):
        self._rec, self._real = rec, real

    def __getattr__(self, name):
        rec, real = self._rec, self._real

        def fn(*args):
            text = rec.call(name, args)
            if name.endswith("_bytes"):
                tag = f"q{rec.queries}"
                rec.queries += 1
                rec.lines.append(f"{tag} = {text}")
                return _Q(getattr(real, name)(*[int(a) for a in args]), tag)
            rec.lines.append(text)
            return 256 if name == "sparch_device_cus" else 0
        return fn


class _Timer:
    enabled = False

    def __init__(self, rec):
        self._rec = rec

    def start(self, name):
        self._rec.lines.append(f"timer {name}")

    def stop(self, tok):
        pass


@contextlib.contextmanager
def _tracing(rec):
    """The patches, and the switches of the module at their defaults; everything is put back afterwards."""
    undo = []

    def patch(obj, name, value):
        undo.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    real_empty, real_empty_like = torch.empty, torch.empty_like

    def empty(*size, **kw):
        t = real_empty(*size, **kw)
        for s in size:
            if isinstance(s, _Q):
                t._trace_size = s.tag
        return t

    def empty_like(src, **kw):
        t = real_empty_like(src, **kw)
        if getattr(src, "_trace_size", None) is not None:
            t._trace_size = src._trace_size
        return t

    env = {k: os.environ.pop(k) for k in ENV_SWITCHES if k in os.environ}
    try:
        stand_in = _Lib(rec, _capi.lib)
        for mod in (Fn, streaming):
            patch(mod, "lib", stand_in)
            patch(mod, "ptr", lambda t: t)
        patch(Fn, "_stream", lambda: None)
        patch(Fn, "_require_device", lambda t, what: None)
        patch(snns, "_check_bidir_input", lambda net, x, what: None)
        # SNN.forward's own state draws stay with torch.rand: the host routine behind the fast draw is a library call,
        # and its one-time self-check would see the stand-in (and switch the fast draw off for the whole process)
        patch(snns, "_fast_rand_ok", False)
        patch(Fn, "timer", _Timer(rec))
        patch(torch, "empty", empty)
        patch(torch, "empty_like", empty_like)
        for name, default in (("DENSE_GEMM", "split6"), ("USE_DX_PLANES", "auto"), ("SAVE_BF16", False),
                              ("_precision", 0), ("SYNC_BN", None), ("persistent_hooks", []), ("_degraded", set()),
                              ("_status", {}), ("_flag_one", {}), ("_placeholder_zero", {})):
            patch(Fn, name, default)
        yield
    finally:
        for obj, name, value in reversed(undo):
            setattr(obj, name, value)
        for k in ENV_SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(env)


# ------------------------------------------------------------------------------------------ the drivers
def _p(*shape, grad=True):
    return torch.zeros(*shape).requires_grad_(grad)


def _norm_params(norm, H, grad):
    return (_p(H, grad=grad), _p(H, grad=grad)) if norm != "none" else (None, None)


def _norm_cfg(norm, H, train):
    bn = norm == "batchnorm"
    return {"normalization": norm, "training": train,
            "running_mean": torch.zeros(H) if bn else None, "running_var": torch.ones(H) if bn else None,
            "num_batches_tracked": torch.zeros((), dtype=torch.int64) if (bn and train) else None}


def _input(source, B, T, K, x_grad=False):
    """(x, the cfg entries that describe it)."""
    if source == "counts":
        x = Fn.input_from_counts(torch.zeros(B, T, K, dtype=torch.uint8))
        return x, {"in_plane": Fn.input_plane_of(x)}
    return _p(B, T, K, grad=x_grad), {}


def _spiking(x, xcfg, kind, norm, dirs, H, train=True, bias=False, fp32_out=True, rows=None):
    """One SpikingLayerFn.apply -> (s, rate, the next layer's description of s).  rows: the sequences of a packed x."""
    B, T, K = x.shape
    B = rows or B
    adaptive, rec = kind in ("adLIF", "RadLIF"), kind in ("RLIF", "RadLIF")
    g = train
    nw, nb = _norm_params(norm, H, g)
    beta, a, b = (_p(H, grad=g), _p(H, grad=g), _p(H, grad=g)) if adaptive else (None, None, None)
    cfg = dict(_norm_cfg(norm, H, train), kind=kind, dirs=dirs, theta=1.0, p_drop=0.0, seed=0, states_ready=None,
               fp32_out=fp32_out, in_spike_scale=None, in_spike16=None, in_plane=None)
    cfg.update(xcfg)
    Bp = B * dirs
    s, rate, s16 = Fn.SpikingLayerFn.apply(
        cfg, x, _p(H, K, grad=g), _p(H, grad=g) if bias else None, nw, nb, _p(H, grad=g), beta, a, b,
        _p(H, H, grad=g) if rec else None, torch.zeros(Bp, H), torch.zeros(Bp, H) if adaptive else None,
        torch.zeros(Bp, H))
    return s, rate, {"in_spike_scale": 1.0, "in_spike16": s16 if s16.numel() else None}


def _readout(x, xcfg, norm, C, train=True, bias=False, extra=None, rows=None, u0_grad=False):
    B, T, K = x.shape
    nw, nb = _norm_params(norm, C, train)
    cfg = dict(_norm_cfg(norm, C, train), in_spike_scale=None, in_spike16=None)
    cfg.update({k: v for k, v in xcfg.items() if k in cfg})
    cfg.update(extra or {})
    return Fn.ReadoutLayerFn.apply(cfg, x, _p(C, K, grad=train), _p(C, grad=train) if bias else None, nw, nb,
                                   _p(C, grad=train), _p(rows or B, C, grad=u0_grad))


def _backward(*outs):
    sum(o.sum() for o in outs).backward()


def case_spiking(kind, norm, dirs, B=4, T=3, K=32, H=128, train=True, bias=False, x_grad=False, source="dense"):
    with contextlib.ExitStack() as stack:
        if not train:
            stack.enter_context(torch.no_grad())
        x, xcfg = _input(source, B, T, K, x_grad)
        s, rate, _ = _spiking(x, xcfg, kind, norm, dirs, H, train=train, bias=bias)
        if train:
            _backward(s, rate)


def case_chain(kind, norm, dirs, B=4, T=3, K=32, H=128, first="LIF", first_H=None, bias=False, readout=None):
    """Two layers of ours: the second reads the first one's bf16 plane, its fp32 input is the placeholder; then,
    optionally, a readout on the second layer's plane."""
    x, xcfg = _input("dense", B, T, K)
    s, r1, tag = _spiking(x, xcfg, first, "none", 1, first_H or H, fp32_out=False)
    outs = [r1]
    s, r2, tag = _spiking(s, tag, kind, norm, dirs, H, bias=bias, fp32_out=readout is None)
    outs.append(r2)
    outs.append(s if readout is None else _readout(s, tag, readout, 5, bias=bias))
    _backward(*outs)


def case_readout(norm, source, bias, B=4, T=3, K=32, C=5):
    if source == "spikes":
        x, xcfg = _input("dense", B, T, K)
        s, r, tag = _spiking(x, xcfg, "LIF", "none", 1, K, fp32_out=False)
        _backward(_readout(s, tag, norm, C, bias=bias), r)
    else:
        x, xcfg = _input("dense", B, T, K, x_grad=True)
        _backward(_readout(x, xcfg, norm, C, bias=bias))


def case_cell(kind, Bp=4, T=3, H=8, steps_per_launch=None):
    adaptive, rec = kind in ("adLIF", "RadLIF"), kind in ("RLIF", "RadLIF")
    beta, a, b = (_p(H), _p(H), _p(H)) if adaptive else (None, None, None)
    s = Fn.SpikingCellFn.apply(kind, 1.0, _p(Bp, T, H), _p(H), beta, a, b, _p(H, H) if rec else None,
                               torch.zeros(Bp, H), torch.zeros(Bp, H) if adaptive else None, torch.zeros(Bp, H),
                               steps_per_launch)
    _backward(s)


def case_readout_cell():
    _backward(Fn.ReadoutCellFn.apply(_p(4, 3, 5), _p(5), torch.zeros(4, 5)))


def _ann_cfg(norm, H, dirs=1, ln_width=None):
    cfg = dict(_norm_cfg(norm, H, True), dirs=dirs, p_drop=0.0, seed=0, ln_width=ln_width, act="sigmoid")
    del cfg["num_batches_tracked"]  # (the modules of anns.py advance BatchNorm's counter themselves)
    return cfg


def case_mlp(norm, bias, ln_width=None):
    nw, nb = _norm_params(norm, 8, True)
    _backward(Fn.MLPLayerFn.apply(_ann_cfg(norm, 8, ln_width=ln_width), _p(4, 3, 12), _p(8, 12),
                                  _p(8) if bias else None, nw, nb))


def case_readout_ann(norm, bias):
    nw, nb = _norm_params(norm, 5, True)
    _backward(Fn.ReadoutANNFn.apply(_ann_cfg(norm, 5), _p(4, 3, 12), _p(5, 12), _p(5) if bias else None, nw, nb))


def case_rnn(norm, dirs, bias=False, H=32, x_grad=True):
    nw, nb = _norm_params(norm, H, True)
    _backward(Fn.RNNLayerFn.apply(_ann_cfg(norm, H, dirs), _p(4, 3, 12, grad=x_grad), _p(H, 12),
                                  _p(H) if bias else None, nw, nb, _p(H, H)))


def case_gated(kind, norm, dirs, H, bias=False, ln_width=None, x_grad=True):
    mats = ("c", "z", "r") if kind == "GRU" else ("c", "z")
    params = []
    for _ in mats:
        params += [_p(H, 12), _p(H) if bias else None, *_norm_params(norm, H, True), _p(H, H)]
    cfg = dict(_ann_cfg(norm, H, dirs, ln_width), kind=kind,
               running={m: (torch.zeros(H), torch.ones(H)) for m in mats})
    _backward(Fn.GatedLayerFn.apply(cfg, _p(4, 3, 12, grad=x_grad), *params))


def case_modules(kind, norm, bidirectional):
    """The modules of snns.py the way SNN.forward chains them, with explicit states (no pinned staging buffer)."""
    B, T, K, H, C = 4, 3, 32, 128, 5
    net = snns.SNN((B, None, K), [H, H, C], neuron_type=kind, normalization=norm, bidirectional=bidirectional,
                   use_bias=True).train()
    x, rates = torch.zeros(B, T, K), []
    for i, layer in enumerate(net.snn):
        if i == net.num_layers - 1:
            x = layer(x, u0=torch.zeros(B, C))
        else:
            rows = B * (2 if bidirectional else 1)
            states = (torch.zeros(rows, H), torch.zeros(rows, H) if kind in ("adLIF", "RadLIF") else None,
                      torch.zeros(rows, H))
            x, r = layer.forward_with_rate(x, states=states, fp32_out=False)
            rates.append(r)
    _backward(x, *rates)


def case_streaming(kind, norm, H, fp32_last=False):
    """Two chunks of the chunk path: the first starts from drawn states (the dense boundary product), the second from
    binary ones (the spike product); the second arrives as bytes."""
    B, Tc, K, C = 4, 3, 32, 5
    sizes = [H, H] if fp32_last else [H, H, C]
    net = snns.SNN((B, None, K), sizes, neuron_type=kind, normalization=norm, use_readout_layer=not fp32_last).eval()
    st = streaming.StreamingSNN(net, B)
    adaptive = kind in ("adLIF", "RadLIF")
    states = [(torch.zeros(B, H), torch.zeros(B, H) if adaptive else None, torch.zeros(B, H)) for _ in range(2)]
    st.reset(states=states + ([] if fp32_last else [torch.zeros(B, C)]))
    st.step(torch.zeros(B, Tc, K))
    st.step(torch.zeros(B, Tc, K, dtype=torch.uint8))


# ---------------------------------------------------------- ragged layouts, and what the layer path gained with them
LENGTHS = (3, 1, 2, 3)  # at B = 4, T = 3: a full row, a one-step row, and a sum (9) that is not B * T
SMOOTH = ("fast_sigmoid", 5.0)


def _layout(layout, dirs=1, B=4, T=3):
    """(the cfg entries of a layout the way snns.py assembles them, the leading shape of x, the sequences)."""
    if layout == "dense":
        return {}, (B, T), B
    if layout == "lengths":
        lengths = snns.prepare_lengths(torch.tensor(LENGTHS), B, T, "cpu")
        return dict(lengths=lengths, **({"lengths2": snns.double_lengths(lengths)} if dirs == 2 else {})), (B, T), B
    plan = snns.prepare_packing(torch.tensor(LENGTHS), B, T, "cpu")
    return dict(pack=plan, **({"pack2": snns.prepare_bidir_packing(plan, "cpu")} if dirs == 2 else {})), (1, plan.n), B


def case_layout(kind, norm, dirs, layout, K=32, H=128, x_grad=False, source="dense", **extra):
    """SpikingLayerFn on a ragged layout; extra: further cfg entries (surrogate)."""
    lay, (Bx, Tx), rows = _layout(layout, dirs)
    x, xcfg = _input(source, Bx, Tx, K, x_grad)
    s, rate, _ = _spiking(x, dict(xcfg, **lay, **extra), kind, norm, dirs, H, rows=rows)
    _backward(s, rate)


def case_readout_layout(norm, layout, K=32, C=5, only=None, **extra):
    """ReadoutLayerFn on a layout; extra: readout / per_step; only: the one output ("out" / "seq") that gets a gradient."""
    lay, (Bx, Tx), rows = _layout(layout)
    x, xcfg = _input("dense", Bx, Tx, K, True)
    res = _readout(x, xcfg, norm, C, extra=dict(lay, **extra), rows=rows, u0_grad=bool(extra.get("stateful")))
    if only is not None:
        res = res[("out", "seq").index(only)]
    _backward(*(res if isinstance(res, tuple) else (res,)))


def _tensors(res):
    for r in res if isinstance(res, (tuple, list)) else (res,):
        if isinstance(r, dict):
            yield from r.values()
        elif isinstance(r, (tuple, list)):
            yield from _tensors(r)
        else:
            yield r


def case_net(kind, norm, sizes=(128, 128, 5), K=32, source="dense", x_grad=False, lengths=False, train=True, fw=None,
             **net_kw):
    """Whole SNN.forward (states drawn by the network), backward through everything it returned."""
    B, T = 4, 3
    net = snns.SNN((B, None, K), list(sizes), neuron_type=kind, normalization=norm, **net_kw).train(train)
    fw = dict(fw or {}, **({"lengths": torch.tensor(LENGTHS)} if lengths else {}))
    with contextlib.ExitStack() as stack:
        if not train:
            stack.enter_context(torch.no_grad())
        res = net(_input(source, B, T, K, x_grad)[0], **fw)
        if train:
            _backward(*_tensors(res))


def case_stateful(kind, sizes=(128, 128, 5), K=32, only_state=False):
    """return_state=True, then the next chunk from that state; only_state: the gradient arrives on the final state
    alone."""
    B, T = 4, 3
    net = snns.SNN((B, None, K), list(sizes), neuron_type=kind, normalization="batchnorm").train()
    first = net(torch.zeros(B, T, K), return_state=True)
    second = net(torch.zeros(B, T, K), state=first[2], return_state=True)
    _backward(*_tensors(second[2] if only_state else (first[:2], second)))


def case_row_movers(C=8):
    plan = _layout("pack")[0]["pack"]
    xp = Fn.PackRowsFn.apply(_p(4, 3, C), plan)
    _backward(xp, Fn.UnpackRowsFn.apply(_p(plan.n, C), plan))


@contextlib.contextmanager
def _env(**kv):
    os.environ.update(kv)
    try:
        yield
    finally:
        for k in kv:
            os.environ.pop(k, None)


@contextlib.contextmanager
def _attr(name, value):
    old = getattr(Fn, name)
    setattr(Fn, name, value)
    try:
        yield
    finally:
        setattr(Fn, name, old)


def _cases():
    """(name, thunk) in file order."""
    kinds, norms = ("LIF", "adLIF", "RLIF", "RadLIF"), ("none", "batchnorm", "layernorm")
    out = []

    def add(name, fn, *a, **kw):
        out.append((name, lambda: fn(*a, **kw)))

    # SpikingLayerFn, dense fp32 input where the weight planes apply: every kind x normalisation x dirs, bias and
    # x.requires_grad alternating so that each appears with each kind and each normalisation
    n = 0
    for kind in kinds:
        for norm in norms:
            for dirs in (1, 2):
                bias, x_grad = bool(n & 1), bool(n & 2)
                n += 1
                add(f"spiking {kind} {norm} dirs={dirs} bias={int(bias)} x_grad={int(x_grad)} dense 4x3x32->128",
                    case_spiking, kind, norm, dirs, bias=bias, x_grad=x_grad)
    for i, kind in enumerate(kinds):  # eval without gradients: nothing is saved
        add(f"spiking {kind} {norms[i % 3]} eval 4x3x32->128", case_spiking, kind, norms[i % 3], 1 + (i & 1),
            train=False)
    for kind in kinds:  # the network input as bytes
        add(f"spiking {kind} batchnorm counts 4x3x32->128", case_spiking, kind, "batchnorm", 1, source="counts")
    add("spiking LIF none counts eval 4x3x12->8", case_spiking, "LIF", "none", 1, K=12, H=8, source="counts",
        train=False)
    for kind in kinds:  # behind a layer of ours: plane in, placeholder edge
        for norm in norms:
            dirs = 2 if (kind, norm) in (("LIF", "batchnorm"), ("RadLIF", "none"), ("adLIF", "layernorm")) else 1
            add(f"chain LIF -> {kind} {norm} dirs={dirs} 4x3x32->128->128", case_chain, kind, norm, dirs,
                bias=norm == "none")
    add("chain RLIF -> RadLIF batchnorm dirs=1 4x3x12->8->8", case_chain, "RadLIF", "batchnorm", 1, K=12, H=8,
        first="RLIF")
    add("chain LIF -> LIF batchnorm -> readout batchnorm 4x3x32->128->128->5", case_chain, "LIF", "batchnorm", 1,
        readout="batchnorm")
    for kind in kinds:  # no planes at this shape
        for j, norm in enumerate(norms):
            add(f"spiking {kind} {norm} dirs={1 + (j & 1)} x_grad={int(j != 1)} dense 4x3x12->8", case_spiking, kind,
                norm, 1 + (j & 1), K=12, H=8, bias=j == 2, x_grad=j != 1)
    for kind in ("RLIF", "RadLIF"):  # a recurrent width that runs zero-padded to a multiple of 4
        for dirs in (1, 2):
            add(f"spiking {kind} batchnorm dirs={dirs} dense 4x3x12->6", case_spiking, kind, "batchnorm", dirs, K=12,
                H=6, x_grad=True)
    add("spiking RLIF none eval 4x3x12->6", case_spiking, "RLIF", "none", 1, K=12, H=6, train=False)

    def switched(ctx, fn, *a, **kw):
        def run():
            with ctx():
                fn(*a, **kw)
        return run

    def add_sw(name, ctx, fn, *a, **kw):
        out.append((name, switched(ctx, fn, *a, **kw)))

    add_sw("SPARCH_REC_STEP_PATH=1 spiking RadLIF batchnorm dirs=2 dense 4x3x32->128",
           lambda: _env(SPARCH_REC_STEP_PATH="1"), case_spiking, "RadLIF", "batchnorm", 2, x_grad=True)
    for L in ("1", "2"):
        add_sw(f"SPARCH_REC_STEPS_PER_LAUNCH={L} spiking RLIF batchnorm dirs=1 dense 4x3x32->128",
               lambda L=L: _env(SPARCH_REC_STEPS_PER_LAUNCH=L), case_spiking, "RLIF", "batchnorm", 1)
    for kind in ("adLIF", "RadLIF"):
        add_sw(f"SAVE_BF16 spiking {kind} batchnorm dirs=1 dense 4x3x32->128", lambda: _attr("SAVE_BF16", True),
               case_spiking, kind, "batchnorm", 1)
    add_sw("compute dtype bf16 chain LIF -> RadLIF batchnorm dirs=2 4x3x32->128->128",
           lambda: _attr("_precision", 1), case_chain, "RadLIF", "batchnorm", 2)
    add("dx planes (auto) chain LIF -> LIF batchnorm dirs=2 8x32x32->256->256", case_chain, "LIF", "batchnorm", 2,
        B=8, T=32, H=256, bias=True)
    add_sw("dx planes (forced) chain LIF -> LIF batchnorm dirs=1 8x32x32->256->256",
           lambda: _attr("USE_DX_PLANES", True), case_chain, "LIF", "batchnorm", 1, B=8, T=32, H=256)
    add_sw("dx planes (off) chain LIF -> LIF batchnorm dirs=2 8x32x32->256->256",
           lambda: _attr("USE_DX_PLANES", False), case_chain, "LIF", "batchnorm", 2, B=8, T=32, H=256)
    add_sw("DENSE_GEMM=fp32 spiking RadLIF batchnorm dirs=1 dense 4x3x32->128", lambda: _attr("DENSE_GEMM", "fp32"),
           case_spiking, "RadLIF", "batchnorm", 1, x_grad=True)
    add_sw("DENSE_GEMM=fp32 chain LIF -> LIF batchnorm dirs=1 4x3x32->128->128", lambda: _attr("DENSE_GEMM", "fp32"),
           case_chain, "LIF", "batchnorm", 1)

    for norm in norms:
        for source in ("spikes", "dense"):
            for bias in (False, True):
                add(f"readout {norm} {source} bias={int(bias)} 4x3x32->5", case_readout, norm, source, bias)
    for kind in kinds:
        add(f"cell {kind} 4x3x8", case_cell, kind)
    add("cell RadLIF 4x3x6 steps_per_launch=1", case_cell, "RadLIF", H=6, steps_per_launch=1)
    add("readout cell 4x3x5", case_readout_cell)
    add("mlp batchnorm bias", case_mlp, "batchnorm", True)
    add("mlp layernorm ln_width=6", case_mlp, "layernorm", False, ln_width=6)
    add("mlp none", case_mlp, "none", False)
    add("readout ann batchnorm bias", case_readout_ann, "batchnorm", True)
    add("readout ann none", case_readout_ann, "none", False)
    for dirs in (1, 2):
        add(f"rnn batchnorm dirs={dirs} persistent", case_rnn, "batchnorm", dirs, bias=dirs == 2, x_grad=dirs == 1)
        add_sw(f"rnn layernorm dirs={dirs} step path", lambda: _env(SPARCH_REC_STEP_PATH="1"), case_rnn, "layernorm",
               dirs)
    for kind, sw in (("LiGRU", "SPARCH_LIGRU_PERSISTENT"), ("GRU", "SPARCH_GRU_PERSISTENT")):
        for dirs in (1, 2):
            add(f"gated {kind} batchnorm dirs={dirs} H=32 persistent", case_gated, kind, "batchnorm", dirs, 32,
                bias=dirs == 2, x_grad=dirs == 1)
            add(f"gated {kind} none dirs={dirs} H=8 launch per step", case_gated, kind, "none", dirs, 8)
        add_sw(f"gated {kind} batchnorm dirs=1 H=32 {sw}=0", lambda sw=sw: _env(**{sw: "0"}), case_gated, kind,
               "batchnorm", 1, 32)
        add(f"gated {kind} layernorm dirs=1 H=8 ln_width=6", case_gated, kind, "layernorm", 1, 8, ln_width=6)
    add_sw("SPARCH_REC_STEPS_PER_LAUNCH=1 gated GRU none dirs=1 H=32", lambda: _env(SPARCH_REC_STEPS_PER_LAUNCH="1"),
           case_gated, "GRU", "none", 1, 32)

    for kind in ("LIF", "RadLIF"):
        for norm, bidir in (("batchnorm", False), ("layernorm", True)):
            add(f"modules {kind} {norm} bidirectional={int(bidir)} 4x3x32->128->128->5", case_modules, kind, norm, bidir)
    add("streaming RadLIF batchnorm 4x(3+3)x32->128->128->5", case_streaming, "RadLIF", "batchnorm", 128)
    add("streaming adLIF layernorm 4x(3+3)x32->128->128->5", case_streaming, "adLIF", "layernorm", 128)
    add("streaming RLIF none, no readout, 4x(3+3)x32->6->6", case_streaming, "RLIF", "none", 6, fp32_last=True)
    add_sw("SPARCH_REC_STEP_PATH=1 streaming RadLIF batchnorm 4x(3+3)x32->128->128->5",
           lambda: _env(SPARCH_REC_STEP_PATH="1"), case_streaming, "RadLIF", "batchnorm", 128)

    # ---- everything below: what the spiking layer path gained since (ragged layouts, surrogates, stateful training,
    # readouts, delays, synapses, the row movers); lengths (3, 1, 2, 3) throughout
    n = 0
    for kind in kinds:  # SpikingLayerFn: every kind x layout x dirs; each normalisation meets each layout
        for layout in ("lengths", "pack"):
            for dirs in (1, 2):
                norm, x_grad = norms[n % 3], bool(n & 4)
                n += 1
                add(f"spiking {kind} {norm} dirs={dirs} x_grad={int(x_grad)} {layout} 4x3x32->128", case_layout, kind,
                    norm, dirs, layout, x_grad=x_grad)
    for kind, norm, dirs, layout in (("LIF", "batchnorm", 1, "lengths"), ("adLIF", "layernorm", 2, "pack"),
                                     ("RadLIF", "none", 2, "lengths"), ("RLIF", "batchnorm", 1, "pack")):
        add(f"spiking {kind} {norm} dirs={dirs} {layout} 4x3x12->8", case_layout, kind, norm, dirs, layout, K=12, H=8,
            x_grad=True)
    for kind, dirs, layout in (("RLIF", 1, "lengths"), ("RadLIF", 2, "lengths"), ("RLIF", 2, "pack"), ("RadLIF", 1, "pack")):
        add(f"spiking {kind} batchnorm dirs={dirs} {layout} 4x3x12->6", case_layout, kind, "batchnorm", dirs, layout,
            K=12, H=6, x_grad=True)
    add("spiking LIF batchnorm dirs=1 counts lengths 4x3x32->128", case_layout, "LIF", "batchnorm", 1, "lengths",
        source="counts")
    for kind, norm, bidir, fw in (("LIF", "batchnorm", False, {}), ("RadLIF", "layernorm", False, {"pack": True}),
                                  ("adLIF", "batchnorm", True, {}), ("RLIF", "none", True, {"pack": True})):
        add(f"net {kind} {norm} bidirectional={int(bidir)} {'pack' if fw else 'lengths'} 4x3x32->128->128->5", case_net,
            kind, norm, bidirectional=bidir, lengths=True, fw=fw)
    add("net RadLIF batchnorm bidirectional=1 lengths 4x3x12->6->6->5", case_net, "RadLIF", "batchnorm", sizes=(6, 6, 5),
        K=12, bidirectional=True, lengths=True, x_grad=True)
    add("net LIF batchnorm pack, no readout, counts 4x3x32->128->128", case_net, "LIF", "batchnorm", sizes=(128, 128),
        source="counts", lengths=True, fw={"pack": True}, use_readout_layer=False)

    # a smooth surrogate: the `_sg` backward entries, and the `_len` / `_pk` ones with its id and scale
    for kind in ("LIF", "RLIF"):
        for layout in ("dense", "lengths", "pack"):
            add(f"surrogate fast_sigmoid spiking {kind} batchnorm dirs=1 {layout} 4x3x32->128", case_layout, kind,
                "batchnorm", 1, layout, x_grad=True, surrogate=SMOOTH)
    add("surrogate fast_sigmoid spiking adLIF none dirs=2 dense 4x3x12->8", case_layout, "adLIF", "none", 2, "dense",
        K=12, H=8, surrogate=SMOOTH)
    add("surrogate fast_sigmoid spiking RadLIF batchnorm dirs=2 lengths 4x3x12->6", case_layout, "RadLIF", "batchnorm",
        2, "lengths", K=12, H=6, surrogate=SMOOTH)
    add_sw("SPARCH_REC_STEP_PATH=1 surrogate fast_sigmoid spiking RLIF batchnorm dirs=1 dense 4x3x32->128",
           lambda: _env(SPARCH_REC_STEP_PATH="1"), case_layout, "RLIF", "batchnorm", 1, "dense", surrogate=SMOOTH)
    add("surrogate triangle net RadLIF layernorm lengths 4x3x32->128->128->5", case_net, "RadLIF", "layernorm",
        lengths=True, surrogate="triangle")

    # stateful training: return_state=True, then state=
    for kind in ("LIF", "adLIF", "RLIF"):
        add(f"stateful net {kind} batchnorm 4x3x32->128->128->5", case_stateful, kind)
    for kind in ("RLIF", "RadLIF"):
        add(f"stateful net {kind} batchnorm 4x3x12->6->6->5", case_stateful, kind, sizes=(6, 6, 5), K=12)
    add("stateful net adLIF batchnorm, gradient on the final state only, 4x3x12->8->8->5", case_stateful, "adLIF",
        sizes=(8, 8, 5), K=12, only_state=True)
    add("stateful net RLIF batchnorm, gradient on the final state only, 4x3x12->6->6->5", case_stateful, "RLIF",
        sizes=(6, 6, 5), K=12, only_state=True)
    add("stateful readout none, gradient on u0, 4x3x32->5", case_readout_layout, "none", "dense", stateful=True)

    # the readout: every reduction x layout, the per-step forms, a gradient on one output only
    for i, mode in enumerate(Fn.READOUT_MODES):
        for j, layout in enumerate(("dense", "lengths", "pack")):
            add(f"readout={mode} {norms[(i + j) % 3]} {layout} 4x3x32->5", case_readout_layout, norms[(i + j) % 3],
                layout, readout=mode)
    for i, per_step in enumerate(Fn.SEQ_MODES):
        for j, layout in enumerate(("dense", "lengths")):
            add(f"per_step={per_step} {norms[(1 + i + j) % 3]} {layout} 4x3x32->5", case_readout_layout,
                norms[(1 + i + j) % 3], layout, per_step=per_step)
    add("per_step=prob batchnorm lengths, gradient on seq only, 4x3x32->5", case_readout_layout, "batchnorm", "lengths",
        per_step="prob", only="seq")
    add("per_step=sum none dense, gradient on out only, 4x3x32->5", case_readout_layout, "none", "dense",
        per_step="sum", only="out")
    add("per_step=prob net LIF batchnorm lengths 4x3x32->128->128->5", case_net, "LIF", "batchnorm", lengths=True,
        fw={"per_step": "prob"})
    add("readout=u_max net adLIF layernorm pack 4x3x12->8->8->5", case_net, "adLIF", "layernorm", sizes=(8, 8, 5), K=12,
        lengths=True, fw={"pack": True}, readout="u_max")

    # axonal delays: on dense fp32 input, on a spike plane of ours (the second layer), on byte input
    add("delays net LIF batchnorm dense 4x3x32->128->128->5", case_net, "LIF", "batchnorm", max_delay=2)
    add("delays net adLIF none dense x_grad=1 4x3x12->8->8->5", case_net, "adLIF", "none", sizes=(8, 8, 5), K=12,
        x_grad=True, max_delay=2)
    add("delays net RLIF layernorm counts 4x3x32->128->128->5", case_net, "RLIF", "layernorm", source="counts",
        max_delay=2)
    add("delays (fixed) net LIF batchnorm dense 4x3x32->128->128->5", case_net, "LIF", "batchnorm", max_delay=2,
        learn_delays=False)
    add("delays (hidden) net LIF batchnorm eval 4x3x32->128->128->5", case_net, "LIF", "batchnorm", train=False,
        max_delay=2, delay_layers="hidden")
    add("delays net RadLIF batchnorm lengths 4x3x32->128->128->5", case_net, "RadLIF", "batchnorm", lengths=True,
        max_delay=2)
    add("delays net LIF layernorm bidirectional=1 pack 4x3x32->128->128->5", case_net, "LIF", "layernorm", lengths=True,
        fw={"pack": True}, bidirectional=True, max_delay=2)
    add("delays net adLIF batchnorm counts pack 4x3x32->128->128->5", case_net, "adLIF", "batchnorm", source="counts",
        lengths=True, fw={"pack": True}, max_delay=2)

    # synaptic currents
    syn = (0.0, 0.9)
    add("synapse net LIF batchnorm dense 4x3x32->128->128->5", case_net, "LIF", "batchnorm", synapse=syn)
    add("synapse net RadLIF layernorm lengths 4x3x32->128->128->5", case_net, "RadLIF", "layernorm", lengths=True,
        synapse=syn)
    add("synapse net adLIF batchnorm pack 4x3x32->128->128->5", case_net, "adLIF", "batchnorm", lengths=True,
        fw={"pack": True}, synapse=syn)
    add("synapse net RLIF batchnorm lengths 4x3x12->6->6->5", case_net, "RLIF", "batchnorm", sizes=(6, 6, 5), K=12,
        lengths=True, synapse=syn)
    add("synapse net LIF batchnorm bidirectional=1 dense 4x3x32->128->128->5", case_net, "LIF", "batchnorm",
        bidirectional=True, synapse=syn)
    add("synapse net RadLIF none bidirectional=1 lengths 4x3x32->128->128->5", case_net, "RadLIF", "none",
        bidirectional=True, lengths=True, synapse=syn)
    add("synapse (fixed, hidden) net LIF batchnorm dense 4x3x32->128->128->5", case_net, "LIF", "batchnorm", synapse=syn,
        learn_synapse=False, synapse_layers="hidden")
    add("synapse net adLIF layernorm eval 4x3x12->8->8->5", case_net, "adLIF", "layernorm", sizes=(8, 8, 5), K=12,
        train=False, synapse=syn)
    add("synapse and delays net LIF batchnorm lengths 4x3x32->128->128->5", case_net, "LIF", "batchnorm", lengths=True,
        synapse=syn, max_delay=2)

    add("row movers 4x3x8", case_row_movers)
    add("spiking LIF batchnorm dirs=1, spikes that arrive without their plane, lengths 4x3x32->128", case_layout, "LIF",
        "batchnorm", 1, "lengths", x_grad=True, in_spike_scale=1.0)
    return out


def trace():
    """The whole trace as one string."""
    rec = _Recorder()
    with _tracing(rec):
        for name, run in _cases():
            rec.new_case(name)
            run()
    return "\n".join(rec.lines) + "\n"


def traced(run):
    """The lines of one case of the caller's: run(this module) under the tracer (the `*_host.py` tests)."""
    rec = _Recorder()
    with _tracing(rec):
        rec.new_case("case")
        run(sys.modules[__name__])
    return rec.lines


def calls(lines, name):
    """The lines of `lines` that call the entry point `name`."""
    return [ln for ln in lines if ln.startswith(name + "(")]


def recorded():
    """The committed trace."""
    with gzip.open(TRACE_FILE, "rt") as f:
        return f.read()


def difference(new):
    """Unified diff (a list of lines, empty when equal) from the committed trace to `new`."""
    return list(difflib.unified_diff(recorded().splitlines(), new.splitlines(), os.path.relpath(TRACE_FILE, ROOT),
                                     "this tree", lineterm="", n=1))


def main(argv):
    text = trace()
    if "--write" in argv:
        with open(TRACE_FILE, "wb") as f:
            f.write(gzip.compress(text.encode(), mtime=0))
        return 0
    if "--check" in argv:
        diff = difference(text)
        print("\n".join(diff) if diff else "layer call trace: unchanged")
        return 1 if diff else 0
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
