"""
Drop-in mirror of the reference's `sparch.models.snns` module API, backed by the
MI355X HIP library.

Same public names, constructor signatures, attribute / parameter / state_dict names,
construction-time RNG draw order and per-forward initial-state draw order as
/root/reference/sparch/models/snns.py (SNN 39-176, LIFLayer 179-303, adLIFLayer 306-445,
RLIFLayer 448-578, RadLIFLayer 581-727, ReadoutLayer 730-825, SpikeFunctionBoxcar 20-36),
so checkpoints, `Experiment` and user code keep working.  What differs is below the API:
a layer's forward is one autograd node (`functional.SpikingLayerFn`) that runs the
projection GEMM, the normalisation and the whole T-step cell recurrence as HIP kernels,
and `SNN.forward` obtains firing rates from spike counts the cell kernels already made
instead of materialising `cat(all_spikes)` (snns.py:174).

`sparch.models.snns` (repo root) re-exports this module under the reference's import path.
"""
import ctypes
import math
import os

import torch
import torch.nn as nn

from . import functional as Fn

_SPIKING_KINDS = ("LIF", "adLIF", "RLIF", "RadLIF")


class SpikeFunctionBoxcar(torch.autograd.Function):
    """Heaviside step with a box-car surrogate gradient (reference snns.py:20-36):
    forward `x > 0` (strict), backward passes the gradient where -0.5 < x <= 0.5.
    Kept for API compatibility; inside the layers this pair is fused into the cell kernels."""

    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        return (x > 0).to(torch.float32)

    @staticmethod
    def backward(ctx, grad_spikes):
        # the reference ASSIGNS zeros outside the box (snns.py:33-35): a non-finite upstream gradient is cleared
        # there, and a NaN x (both comparisons false) lets the gradient through — as the cell kernels do
        # (csrc/common.h boxcar_gate) and oracle/snn_oracle.py
        (x,) = ctx.saved_tensors
        grad_x = grad_spikes.clone()
        grad_x[x <= -0.5] = 0
        grad_x[x > 0.5] = 0
        return grad_x


# The selectable surrogates: name -> the scale k a bare name stands for, chosen so that the
# area under the gate is the box-car's 1 (triangle 1/k, fast sigmoid 2/k, arctangent pi/k).  Derived, not tuned.
SURROGATE_DEFAULT_SCALE = {"boxcar": None, "triangle": 1.0, "fast_sigmoid": 2.0, "atan": math.pi}


def resolve_surrogate(surrogate="boxcar", surrogate_scale=None):
    """(name, scale) checked and completed: the default scale for a bare name; ValueError for an unknown name, a
    scale that is not a finite number > 0, or any scale with the box-car (which has none)."""
    names = ", ".join(SURROGATE_DEFAULT_SCALE)
    if surrogate not in SURROGATE_DEFAULT_SCALE:
        raise ValueError(f"unknown surrogate {surrogate!r}: one of {names}")
    if surrogate == "boxcar":
        if surrogate_scale is not None:
            raise ValueError(f"the boxcar surrogate takes no scale (got {surrogate_scale!r}); surrogates: {names}")
        return "boxcar", None
    if surrogate_scale is None:
        return surrogate, SURROGATE_DEFAULT_SCALE[surrogate]
    try:
        k = float(surrogate_scale)
    except (TypeError, ValueError):
        k = float("nan")
    if not (k > 0.0 and math.isfinite(k)):
        raise ValueError(f"surrogate_scale must be a finite number > 0 (got {surrogate_scale!r}); surrogates: {names}")
    return surrogate, k


def parse_surrogate(text):
    """`name[:scale]` (the SPARCH_SURROGATE environment variable) -> (name, scale) as resolve_surrogate returns it."""
    name, sep, scale = text.strip().partition(":")
    if sep and not scale.strip():
        raise ValueError(f"malformed surrogate {text!r}: expected name[:scale]")
    if sep:
        try:
            scale = float(scale)
        except ValueError:
            raise ValueError(f"malformed surrogate {text!r}: the scale is not a number") from None
    return resolve_surrogate(name.strip(), scale if sep else None)


class SpikeFunctionSurrogate(torch.autograd.Function):
    """Heaviside step `x > 0` with a selectable surrogate gradient, in plain torch and in x's own dtype:
    SpikeFunctionSurrogate.apply(x, name, scale).  "boxcar" is SpikeFunctionBoxcar's rule (assignment); the smooth
    forms multiply: triangle max(0, 1 - k|x|), fast_sigmoid 1 / (1 + k|x|)^2, atan 1 / (1 + (k x)^2).
    Inside the layers the pair is fused into the cell kernels (csrc/common.h smooth_gate)."""

    @staticmethod
    def forward(ctx, x, name="boxcar", scale=None):
        ctx.save_for_backward(x)
        ctx.surrogate = resolve_surrogate(name, scale)
        return (x > 0).to(x.dtype)

    @staticmethod
    def backward(ctx, grad_spikes):
        (x,) = ctx.saved_tensors
        name, k = ctx.surrogate
        if name == "boxcar":
            grad_x = grad_spikes.clone()
            grad_x[x <= -0.5] = 0
            grad_x[x > 0.5] = 0
        elif name == "triangle":
            grad_x = grad_spikes * torch.clamp(1 - k * x.abs(), min=0)
        elif name == "fast_sigmoid":
            d = 1 + k * x.abs()
            grad_x = grad_spikes / (d * d)
        else:
            kx = k * x
            grad_x = grad_spikes / (1 + kx * kx)
        return grad_x, None, None


class _SurrogateSpike:
    """`spike_fct` of a layer with a smooth surrogate: x -> SpikeFunctionSurrogate.apply(x, name, scale) (picklable)."""

    def __init__(self, name, scale):
        self.name, self.scale = name, scale

    def __call__(self, x):
        return SpikeFunctionSurrogate.apply(x, self.name, self.scale)


def _tag_spikes(s, scale, s16, placeholder=False):
    """Mark `s` as a spike train of ours (entries 0 or `scale`, `s16` the same spikes as a bf16 0/1 plane) so
    that the next layer can take the exact spike GEMMs.  The tag carries the tensor's version counter: an
    in-place edit between the layers (mul_, masked fill, slice assignment) invalidates it.
    placeholder: `s` holds no values (forward_with_rate(fp32_out=False)); the plane is the data."""
    s._sparch_spike_tag = (s._version, tuple(s.shape), float(scale), s16, bool(placeholder))


def materialize_spikes(s):
    """The values of a spiking layer's output as an fp32 tensor: `s` itself, or — for the placeholder
    SNN.forward passes between its own layers — its bf16 plane times the dropout scale (the same numbers the
    reference's tensor holds, snns.py:278)."""
    tag = getattr(s, "_sparch_spike_tag", None)
    if tag is not None and len(tag) > 4 and tag[4]:
        return tag[3].float() * tag[2]
    return s


def _spike_tag(x):
    """(scale, s16) if x still is the untouched output of one of our spiking layers, else (None, None):
    the layer then treats x as an arbitrary real-valued input (device-gated exact path / dense GEMM)."""
    tag = getattr(x, "_sparch_spike_tag", None)
    if tag is None or tag[0] != x._version or tag[1] != tuple(x.shape):
        return None, None
    return tag[2], tag[3]


DELAY_INITS = ("zero", "uniform")
DELAY_LAYERS = ("all", "hidden")


def _refuse_stateful_delays(layer):
    if getattr(layer, "max_delay", 0):
        raise ValueError("sparch_amd: state / return_state with axonal delays is not supported (the last max_delay "
                         "input steps of a chunk are not carried into the next one)")


SYN_INITS = ("uniform", "lo")
SYN_LAYERS = ("all", "hidden")


def _check_synapse_call(layer, pack=None, stateful=False):
    """What a layer with a synapse (SNN(synapse=...)) refuses, before any kernel."""
    if stateful:
        raise ValueError("sparch_amd: state / return_state with a synapse is not supported (the carried state has no "
                         "synaptic current yet)")
    if pack is not None and layer.bidirectional:
        raise ValueError("sparch_amd: pack=True with bidirectional=True and a synapse is not supported (the doubled "
                         "packed batch has no filtered form)")
    if layer.bidirectional and hasattr(layer, "V") and Fn.rec_step_path(layer.hidden_size):
        # (the doubled batch runs the kernels with lengths, also where the caller passes none: their refusal, in the
        # caller's terms and before the projection)
        raise ValueError(f"sparch_amd: bidirectional=True with a synapse and a recurrent hidden size above 1024 (got "
                         f"{layer.hidden_size}) is not supported (the layer runs on the doubled batch, which the "
                         "per-step recurrent path does not take)")
    if layer.bidirectional and Fn.SYNC_BN is not None and Fn.SYNC_BN["world"] > 1:
        raise ValueError("sparch_amd: bidirectional=True with a synapse and --sync_bn is not supported (the layer runs "
                         "on the ragged route, which --sync_bn does not take)")


def _layout_cfg(x, lengths, pack, dirs=1, lengths2=None, pack2=None):
    """(the cfg entries that tell a layer Function how the batch's time axis lies in memory — functional.SeqLayout.of_cfg
    reads them; absent for a dense batch — and the rows of the layer's per-sequence tensors).  dirs == 2: with the
    doubled batch's lengths2 = double_lengths(lengths) / pack2 = prepare_bidir_packing(pack), made here when not given
    (SNN.forward makes them once for all its layers)."""
    cfg = {}
    if lengths is not None:
        cfg["lengths"] = lengths
    if pack is not None:
        cfg["pack"] = pack
    if dirs == 2 and pack is not None:
        cfg["pack2"] = pack2 if pack2 is not None else prepare_bidir_packing(pack, x.device)
    elif dirs == 2 and lengths is not None:
        cfg["lengths2"] = lengths2 if lengths2 is not None else double_lengths(lengths)
    return cfg, Fn.SeqLayout.of(lengths, pack).index(x.shape[0], x.shape[1])[0] * dirs


def _delayed_input(layer, x, lengths=None, pack=None):
    """x as a layer with axonal delays (SNN(max_delay=...)) reads it: every input feature shifted
    by its own delay, on the representation the layer's GEMMs read — the bf16 plane of a spike train of ours or of an
    input made by input_from_counts (x and the result are then placeholders; the tags travel on), else x's own values.
    A layer without delays returns x itself: nothing is launched."""
    D = getattr(layer, "max_delay", 0)
    if not D:
        return x
    Fn._require_device(x, "input")
    if x.ndim != 3 or x.shape[2] != layer.delay.numel():
        raise ValueError(f"sparch_amd: a layer with delays takes (batch, time, {layer.delay.numel()}) inputs, got "
                         f"{tuple(x.shape)}")
    cfg = dict(_layout_cfg(x, lengths, pack)[0], max_delay=D)
    B, T, K = x.shape
    scale, s16 = _spike_tag(x)
    if scale is not None and s16 is not None:
        cfg.update(plane=s16.view(B, T, K), scale=scale)
        y, y16 = Fn.DelayFn.apply(x, layer.delay, cfg)
        _tag_spikes(y, scale, y16.view(B, T, K), placeholder=True)
        return y
    tag = Fn.input_plane_of(x) if scale is None else None
    if tag is not None:
        plane, flag = tag
        ld = plane.shape[-1]
        cfg.update(plane=plane.view(B, T, ld)[:, :, :K], scale=1.0, ld_plane=ld)
        y, y16 = Fn.DelayFn.apply(x, layer.delay, cfg)
        y._sparch_input_plane = (tuple(y.shape), y16, flag)
        return y
    y, _ = Fn.DelayFn.apply(x, layer.delay, cfg)
    if scale is not None:  # a spike train without its plane: the entries stay 0 or `scale`
        _tag_spikes(y, scale, None)
    return y


# ---- initial-state draws.  The reference draws every layer's u0, [w0,] s0 with torch.rand from the global CPU
# generator at each forward (snns.py:286-287, 423-425, 558-559, 700-702, 812).  The values below are the same
# numbers from the same generator in the same order; what differs is who computes them: torch's serial loop
# costs ~5 ns per number (8.5 ms per step at the headline shape, more than the GPU needs for the step), the
# library's host routine `sparch_mt19937_uniform_f32` ~1 ns.  It works on the generator's serialized MT19937
# state (CPUGeneratorImplStateLegacy: seed u64, left i32, seeded i32, next u64, 624 state words as u64, ...),
# which is moved out, advanced, and written back — so anything else drawing from the global generator before or
# after sees the stream it would have seen.  The layout is verified once against torch.rand on a private
# generator; if that check ever fails (another torch build), the draws simply stay with torch.rand.
_MT_WORDS, _MT_OFF_LEFT, _MT_OFF_NEXT, _MT_OFF_KEY, _MT_STATE_BYTES = 624, 8, 16, 24, 24 + 624 * 8


def _mt_draw(state_bytes, outs):
    """Fill the fp32 CPU tensors `outs` (contiguous) in order from the serialized generator state
    `state_bytes` (uint8 tensor, modified in place).  Returns False if the state is not one this code reads."""
    import numpy as np

    raw = state_bytes.numpy()
    if raw.size < _MT_STATE_BYTES:
        return False
    left = int(raw[_MT_OFF_LEFT:_MT_OFF_LEFT + 4].view(np.int32)[0])
    nxt = int(raw[_MT_OFF_NEXT:_MT_OFF_NEXT + 8].view(np.uint64)[0])
    key64 = raw[_MT_OFF_KEY:_MT_OFF_KEY + _MT_WORDS * 8].view(np.uint64)
    if not (1 <= left <= _MT_WORDS and nxt <= _MT_WORDS and (left == 1 or left == _MT_WORDS + 1 - nxt)):
        return False
    key = key64.astype(np.uint32)
    pos = ctypes.c_int(_MT_WORDS if left == 1 else nxt)
    for t in outs:
        Fn.check(Fn.lib.sparch_mt19937_uniform_f32(key.ctypes.data, ctypes.byref(pos), t.numel(), t.data_ptr()),
                 "sparch_mt19937_uniform_f32")
    key64[:] = key
    p = pos.value
    raw[_MT_OFF_NEXT:_MT_OFF_NEXT + 8].view(np.uint64)[0] = p
    raw[_MT_OFF_LEFT:_MT_OFF_LEFT + 4].view(np.int32)[0] = 1 if p == _MT_WORDS else _MT_WORDS + 1 - p
    return True


_fast_rand_ok = None


def _fast_rand_available():
    """One-time check of the serialized-state layout: 300 k numbers across many block boundaries from a private
    generator, by torch.rand and by the host routine; the generator must also end in the same state."""
    global _fast_rand_ok
    if _fast_rand_ok is None:
        ok = False
        if os.environ.get("SPARCH_FAST_RAND", "1") != "0":
            try:
                g = torch.Generator()
                g.manual_seed(0x5eed)
                torch.rand(7, generator=g)  # somewhere inside a block
                st = g.get_state().clone()
                want = [torch.rand(300, 1001, generator=g), torch.rand(5, generator=g)]
                got = [torch.empty(300, 1001), torch.empty(5)]
                ok = _mt_draw(st, got) and all(torch.equal(a, b) for a, b in zip(want, got)) \
                    and torch.equal(st, g.get_state())
            except Exception:  # any surprise in the layout: keep torch.rand
                ok = False
        _fast_rand_ok = ok
    return _fast_rand_ok


def _rand_batch(shapes, device, out=None):
    """torch.rand(*shape) for every shape, in order, from the global CPU generator — as ONE pinned staging
    buffer and one asynchronous copy; returns the device tensors (views of one allocation, 256-byte aligned).
    out: the flat device buffer of an earlier call with the same shapes (`.flat` of its first tensor's list):
    refilled in place — the static inputs of a captured step."""
    if _rand_to is not _rand_to_default:  # a caller substituted the per-tensor draw (tests inject fixture states)
        return _StateList([_rand_to(r, c, device) for r, c in shapes], None)
    sizes = [int(r) * int(c) for r, c in shapes]
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + 63) // 64 * 64
    on_gpu = device.type == "cuda"
    slot = _staging_slot(total, device) if on_gpu else None
    host = slot[0] if on_gpu else torch.empty(total, dtype=torch.float32)
    views = [host[o:o + n].view(r, c) for o, n, (r, c) in zip(offs, sizes, shapes)]
    done = False
    if _fast_rand_available():
        st = torch.get_rng_state()
        done = _mt_draw(st, views)
        if done:
            torch.set_rng_state(st)
    if not done:
        for v in views:
            torch.rand(v.shape[0], v.shape[1], out=v)
    ready = None
    if out is not None and on_gpu:
        # static states of a captured step: the upload runs on the side stream into one of two device staging
        # buffers — under whatever replay the GPU is still busy with — and only a device-to-device copy (7 MB at the
        # headline shape: ~10 us against ~150 us over PCIe) sits in stream order in front of the next replay
        assert out.numel() == total and out.device == device
        main = torch.cuda.current_stream(device)
        side = _upload_stream(device)
        dslot = _device_staging_slot(total, device)
        if dslot[1] is not None:
            side.wait_event(dslot[1])  # the copy that last read this staging buffer
        with torch.cuda.stream(side):
            dslot[0].copy_(host, non_blocking=True)
            up = torch.cuda.Event()
            up.record(side)
        slot[1] = up
        main.wait_event(up)
        out.copy_(dslot[0], non_blocking=True)
        dslot[1] = torch.cuda.Event()
        dslot[1].record(main)
        dev = out
    elif out is not None:
        assert out.numel() == total and out.device == device
        out.copy_(host)
        dev = out
    elif on_gpu:
        # The upload (7 MB at the headline shape: ~150 us on the DMA engine) goes on a side stream, so that it
        # runs under whatever the compute stream does before it first needs a state (the first layer's
        # projection): in stream order it sat between two steps with the GPU idle.  `.ready` is the event
        # the consumer waits for (SNN.forward hands it to the first layer's cell call).
        main = torch.cuda.current_stream(device)
        side = _upload_stream(device)
        with torch.cuda.stream(side):
            dev = host.to(device, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record(side)
            slot[1] = ready
        dev.record_stream(main)  # allocated on the side stream's pool, consumed on the compute stream
    else:
        dev = host.to(device)
    return _StateList([dev[o:o + n].view(r, c) for o, n, (r, c) in zip(offs, sizes, shapes)], dev, ready)


_upload_streams = {}
# Pinned staging buffers of the draws: a ring of four per (size, device), each reused once the copy that last read it
# has completed (its event).  A fresh `torch.empty(pin_memory=True)` per step goes to hipHostMalloc whenever the host
# runs ahead of the GPU by more blocks than the caching allocator has seen freed — one ~1 ms call per step for the
# first dozens of replays of a captured step (BASELINE configs[1], 20 timed steps: 1.55 ms per step against 1.0 ms).
_staging = {}
_STAGING_DEPTH = 4


_device_staging = {}


def _device_staging_slot(total, device):
    """[buffer, event of the device-to-device copy that last read it] — two per (size, device), alternating."""
    key = (int(total), device.index if device.index is not None else torch.cuda.current_device())
    ring = _device_staging.get(key)
    if ring is None:
        if len(_device_staging) >= 4:
            _device_staging.clear()
        ring = _device_staging[key] = {"next": 0, "slots": [[torch.empty(total, dtype=torch.float32, device=device), None]
                                                             for _ in range(2)]}
    slot = ring["slots"][ring["next"]]
    ring["next"] ^= 1
    return slot


def _staging_slot(total, device):
    key = (int(total), device.type, device.index if device.index is not None else torch.cuda.current_device())
    ring = _staging.get(key)
    if ring is None:
        if len(_staging) >= 8:  # shapes come and go (tests, variable batch sizes): keep the pinned footprint bounded
            _staging.clear()
        ring = _staging[key] = {"next": 0, "slots": [[torch.empty(total, dtype=torch.float32, pin_memory=True), None]
                                                      for _ in range(_STAGING_DEPTH)]}
    slot = ring["slots"][ring["next"]]
    ring["next"] = (ring["next"] + 1) % _STAGING_DEPTH
    if slot[1] is not None:
        slot[1].synchronize()  # the host is four draws ahead of the GPU: wait for the oldest upload
        slot[1] = None
    return slot


def _upload_stream(device):
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    if key not in _upload_streams:
        _upload_streams[key] = torch.cuda.Stream(device=device)
    return _upload_streams[key]


class _StateList(list):
    """The tensors of one _rand_batch call; `.flat` is the single device allocation they are views of, `.ready`
    the event of their upload (None: already ordered on the compute stream)."""

    def __init__(self, tensors, flat, ready=None):
        super().__init__(tensors)
        self.flat = flat
        self.ready = ready

    def wait_ready(self):
        """Make the current stream wait for the upload (no-op when it was stream-ordered)."""
        if self.ready is not None:
            torch.cuda.current_stream().wait_event(self.ready)
            self.ready = None


def _rand_to(rows, cols, device):
    """torch.rand from the global CPU generator (the reference's source of initial states), staged
    in pinned memory and copied asynchronously so the host does not stall once per layer."""
    batch = _rand_batch([(rows, cols)], device)
    batch.wait_ready()
    return batch[0]


_rand_to_default = _rand_to


def _make_norm(normalization, hidden_size):
    """BatchNorm1d(momentum=0.05) / LayerNorm / nothing (reference snns.py:238-244).  The
    torch modules only hold the parameters and running statistics; the maths runs in HIP."""
    if normalization == "batchnorm":
        return nn.BatchNorm1d(hidden_size, momentum=Fn.BN_MOMENTUM), True
    if normalization == "layernorm":
        return nn.LayerNorm(hidden_size), True
    return None, False


class _SpikingLayer(nn.Module):
    """Shared implementation of the four spiking layer types; `kind` selects adaptation
    (adLIF, RadLIF) and layer-wise recurrence (RLIF, RadLIF)."""

    kind = None  # set by subclasses

    def __init__(self, input_size, hidden_size, batch_size, threshold=1.0, dropout=0.0,
                 normalization="batchnorm", use_bias=False, bidirectional=False, surrogate="boxcar",
                 surrogate_scale=None):
        super().__init__()
        self.surrogate, self.surrogate_scale = resolve_surrogate(surrogate, surrogate_scale)
        adaptive = self.kind in ("adLIF", "RadLIF")
        recurrent = self.kind in ("RLIF", "RadLIF")

        self.input_size = int(input_size)
        self.hidden_size = int(hidden_size)
        self.threshold = threshold
        self.dropout = dropout
        self.normalization = normalization
        self.use_bias = use_bias
        self.bidirectional = bidirectional
        self.batch_size = batch_size * (1 + self.bidirectional)
        self.alpha_lim = [math.exp(-1 / 5), math.exp(-1 / 25)]
        if adaptive:
            self.beta_lim = [math.exp(-1 / 30), math.exp(-1 / 120)]
            self.a_lim = [-1.0, 1.0]
            self.b_lim = [0.0, 2.0]
        self.spike_fct = (SpikeFunctionBoxcar.apply if self.surrogate == "boxcar"
                          else _SurrogateSpike(self.surrogate, self.surrogate_scale))

        # Parameters, created and initialised in the reference's order so that identical
        # seeds give identical initial weights (snns.py:233-235, 363-372, 502-507, 638-649).
        self.W = nn.Linear(self.input_size, self.hidden_size, bias=use_bias)
        if recurrent:
            self.V = nn.Linear(self.hidden_size, self.hidden_size, bias=False)
        self.alpha = nn.Parameter(torch.empty(self.hidden_size))
        if adaptive:
            self.beta = nn.Parameter(torch.empty(self.hidden_size))
            self.a = nn.Parameter(torch.empty(self.hidden_size))
            self.b = nn.Parameter(torch.empty(self.hidden_size))
        nn.init.uniform_(self.alpha, self.alpha_lim[0], self.alpha_lim[1])
        if adaptive:
            nn.init.uniform_(self.beta, self.beta_lim[0], self.beta_lim[1])
            nn.init.uniform_(self.a, self.a_lim[0], self.a_lim[1])
            nn.init.uniform_(self.b, self.b_lim[0], self.b_lim[1])
        if recurrent:
            nn.init.orthogonal_(self.V.weight)

        norm, self.normalize = _make_norm(normalization, self.hidden_size)
        if norm is not None:
            self.norm = norm
        self.drop = nn.Dropout(p=dropout)
        self._calls = 0
        self._layer_index = 0  # set by SNN; decorrelates dropout masks between layers

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_seed_word", None)  # graph mode's device-side dropout seed: a step's state, not the network's
        state.pop("_seed_word_owner_advances", None)
        return state

    # ------------------------------------------------------------------ helpers
    @property
    def uses_persistent_kernel(self):
        """True if this layer's time loop runs as ONE persistent launch whose workgroups wait for each other
        (RLIF / RadLIF up to 1024 hidden units) — what sparch_amd.dp keys its all-reduce policy on."""
        return self.kind in ("RLIF", "RadLIF") and not Fn.rec_step_path(self.hidden_size)

    def _draw_states(self, rows, device):
        """Random initial u, [w], s from torch's global CPU generator, in the reference's
        order (snns.py:286-287, 423-425, 558-559, 700-702), then moved to the device."""
        H = self.hidden_size
        u0 = _rand_to(rows, H, device)
        w0 = _rand_to(rows, H, device) if self.kind in ("adLIF", "RadLIF") else None
        s0 = _rand_to(rows, H, device)
        return u0, w0, s0

    def _dropout_seed(self, device):
        """Counter-based seed for the in-kernel dropout mask: device generator seed (no sync)
        mixed with this layer's call count.  Masks differ from torch's by construction."""
        # getattr defaults: modules un-pickled from a checkpoint written by the reference have neither field
        word = getattr(self, "_seed_word", None)
        if word is not None:
            # graph mode (sparch_amd.graph): the seed lives in device memory and is advanced by a captured op,
            # the kernels get its address (a kernel argument would be frozen at capture time)
            if not getattr(self, "_seed_word_owner_advances", False):  # (the captured step advances all layers' words at once)
                word.add_(1)
            return Fn.SEED_IN_MEMORY | word.data_ptr()
        self._calls = getattr(self, "_calls", 0) + 1
        index = getattr(self, "_layer_index", 0)
        base = torch.cuda.initial_seed() if device.type == "cuda" else torch.initial_seed()
        return (base * 0x9E3779B97F4A7C15 + (index + 1) * 0x100000001B3 + self._calls) & 0x7FFFFFFFFFFFFFFF

    def _surrogate(self):
        """None for the box-car (also: a module un-pickled from a checkpoint that predates the setting, or from the
        reference's), else ("name", scale) as the functional layer takes it."""
        name = getattr(self, "surrogate", "boxcar")
        return None if name == "boxcar" else (name, float(getattr(self, "surrogate_scale", None)))

    def extra_repr(self):
        sg = self._surrogate()
        return "" if sg is None else f"surrogate={sg[0]}, surrogate_scale={sg[1]:g}"

    def _cell_params(self):
        p = {"alpha": self.alpha}
        if self.kind in ("adLIF", "RadLIF"):
            p.update(beta=self.beta, a=self.a, b=self.b)
        if self.kind in ("RLIF", "RadLIF"):
            p["V"] = self.V.weight
        return p

    # ------------------------------------------------------------------ forward
    def forward_with_rate(self, x, states=None, states_ready=None, fp32_out=True, lengths=None, pack=None,
                          return_state=False, pack2=None, lengths2=None):
        """Returns (spikes (B,T,H*(1+bidir)), firing_rate (H*(1+bidir),)).  Equivalent to the
        reference forward (e.g. snns.py:663-694) followed by `.mean(dim=(0,1))` (174).
        states: (u0, w0, s0) drawn ahead of time by SNN.forward (same generator, same order);
        states_ready: callable that makes the current stream wait for their upload, called after the
        projection GEMM has been enqueued (the upload runs under it);
        fp32_out=False: the caller feeds the result to another layer of this module only — the returned
        tensor is then a placeholder of the right shape whose VALUES ARE NOT WRITTEN (the spikes travel as the
        bf16 plane in its tag); SNN.forward uses it between its own layers.
        lengths: None, or what prepare_lengths() returned for this batch — the layer's output is then exactly 0 on
        every row's padded steps and the firing rate is the mean over valid steps (SNN.forward has the contract).
        pack: None, or what prepare_packing() returned — x is then the PACKED batch (1, n, feat) (functional.pack_rows)
        and so is the result; `states` hold the plan's `batch` rows in its sorted order (drawn so when not given).
        A bidirectional layer with lengths or pack ("Bidirectional ragged batches") reads every clip
        backwards inside its own length: y[b, t, H:] is the reverse direction after the clip's steps lengths[b]-1 .. t.
        Its `states` have 2 * batch rows, row batch + b the reverse direction of clip b; with pack they are in the order
        of pack2 = prepare_bidir_packing(pack)'s doubled plan; pack2 and lengths2 = double_lengths(lengths) are made
        here when not given.
        return_state=True (stateful training, SNN.forward has the contract): returns (spikes, firing_rate, state) with
        state = {"u": u_T, ["w": w_T,] "s": 1[u_T > threshold]}, the raw spike before dropout; the three are nodes of the
        graph, and the gradient of `states` comes out of the backward.  LIF / adLIF, one direction, no lengths / pack."""
        if return_state:
            _refuse_stateful_delays(self)
            Fn.check_stateful(self.kind, self.hidden_size, dirs=2 if self.bidirectional else 1, lengths=lengths, pack=pack,
                              T=x.shape[1])
        synapse = getattr(self, "synapse", None)  # (a module pickled before the attribute: none)
        if synapse is not None:
            _check_synapse_call(self, pack=pack, stateful=return_state)
        if lengths is not None:
            _check_ragged_layer(self, lengths)
        if pack is not None:
            _check_packed_layer(self, pack, x)
        Fn._require_device(x, "input")
        if synapse is not None and self.bidirectional and lengths is None and pack is None:
            # each direction is filtered causally in its own time order: the layer takes the doubled-batch route of
            # the ragged batches, with every row's length T, made on the device
            lengths = (torch.full((x.shape[0],), x.shape[1], dtype=torch.int32, device=x.device), x.shape[0] * x.shape[1])
            lengths2 = None
        x = _delayed_input(self, x, lengths, pack)  # (x itself without delays)
        dirs = 2 if self.bidirectional else 1
        layout_cfg, rows = _layout_cfg(x, lengths, pack, dirs, lengths2, pack2)
        if self.batch_size != rows:
            self.batch_size = rows
        u0, w0, s0 = states if states is not None else self._draw_states(rows, x.device)
        p_drop = float(self.dropout) if self.training else 0.0
        is_bn = self.normalization == "batchnorm"
        in_scale, in_s16 = _spike_tag(x)
        cfg = {
            "kind": self.kind,
            "normalization": self.normalization if self.normalize else "none",
            "dirs": dirs,
            "training": bool(self.training),
            "theta": float(self.threshold),
            "p_drop": p_drop,
            "seed": self._dropout_seed(x.device) if p_drop > 0 else 0,
            "running_mean": self.norm.running_mean if is_bn else None,
            "running_var": self.norm.running_var if is_bn else None,
            # set when x came straight out of one of our spiking layers: entries are 0 or this constant
            "in_spike_scale": in_scale,
            "in_spike16": in_s16,  # the same spikes as a bf16 plane
            "states_ready": states_ready,
            "fp32_out": bool(fp32_out),
            # network input uploaded as bytes (functional.input_from_counts): its bf16 plane and the flag "exact"
            "in_plane": Fn.input_plane_of(x) if in_scale is None else None,
            # BatchNorm1d's counter: advanced by the statistics kernel (no separate launch; not on skipped steps)
            "num_batches_tracked": self.norm.num_batches_tracked if (is_bn and self.training) else None,
            # the backward's surrogate: None = the reference's box-car, else ("name", scale) — fp32 saves then
            "surrogate": self._surrogate(),
        }
        cfg.update(layout_cfg)
        if return_state:
            cfg["stateful"] = True
        syn_args = ()
        if synapse is not None:  # (absent without a synapse, and gamma not passed: the call is then what it always was)
            cfg["synapse"] = synapse
            syn_args = (self.gamma,)
        nw = self.norm.weight if self.normalize else None
        nb = self.norm.bias if self.normalize else None
        s, rate, s16, *final = Fn.SpikingLayerFn.apply(
            cfg, x, self.W.weight, self.W.bias, nw, nb, self.alpha,
            getattr(self, "beta", None), getattr(self, "a", None), getattr(self, "b", None),
            self.V.weight if hasattr(self, "V") else None, u0, w0, s0, *syn_args)
        # lets the next layer take the exact bf16-split GEMMs and read the spikes as a bf16 plane (half the bytes)
        _tag_spikes(s, 1.0 / (1.0 - p_drop), s16, placeholder=not fp32_out and not s.is_contiguous())
        if return_state:
            u_T, w_T, s_T = final
            return s, rate, ({"u": u_T, "s": s_T} if w_T is None else {"u": u_T, "w": w_T, "s": s_T})
        return s, rate

    def forward(self, x):
        return self.forward_with_rate(x)[0]

    def _cell(self, Wx):
        """The cell alone on an already projected/normalised input (B',T,H) -> spikes (B',T,H),
        as the reference's `_lif_cell` / `_adlif_cell` / `_rlif_cell` / `_radlif_cell`."""
        Fn._require_device(Wx, "Wx")
        u0, w0, s0 = self._draw_states(Wx.shape[0], Wx.device)
        p = self._cell_params()
        return Fn.SpikingCellFn.apply(self.kind, float(self.threshold), Wx, p["alpha"], p.get("beta"),
                                      p.get("a"), p.get("b"), p.get("V"), u0, w0, s0, None, self._surrogate())


class LIFLayer(_SpikingLayer):
    """Leaky integrate-and-fire layer without recurrence (reference LIFLayer, snns.py:179-303)."""
    kind = "LIF"

    def _lif_cell(self, Wx):
        return self._cell(Wx)


class adLIFLayer(_SpikingLayer):
    """Adaptive LIF layer without recurrence (reference adLIFLayer, snns.py:306-445)."""
    kind = "adLIF"

    def _adlif_cell(self, Wx):
        return self._cell(Wx)


class RLIFLayer(_SpikingLayer):
    """LIF layer with layer-wise recurrent weights V (reference RLIFLayer, snns.py:448-578)."""
    kind = "RLIF"

    def _rlif_cell(self, Wx):
        return self._cell(Wx)


class RadLIFLayer(_SpikingLayer):
    """Adaptive LIF layer with recurrent weights V (reference RadLIFLayer, snns.py:581-727)."""
    kind = "RadLIF"

    def _radlif_cell(self, Wx):
        return self._cell(Wx)


class ReadoutLayer(nn.Module):
    """Non-spiking leaky integrator whose output is the sum over time of softmax(u_t)
    (reference ReadoutLayer, snns.py:730-825).  No dropout is applied, as in the reference
    (the Dropout module exists at 791 but is never called).

    readout ("Selectable readout"): the reduction over time — "softmax_sum" (the default, the
    reference's), "softmax_mean" (that sum over the row's number of steps), or of the membrane itself "u_max" (ties:
    the earliest step), "u_mean", "u_last".  With lengths the row's own steps count."""

    def __init__(self, input_size, hidden_size, batch_size, dropout=0.0, normalization="batchnorm",
                 use_bias=False, readout="softmax_sum"):
        super().__init__()
        Fn.readout_mode(readout)
        self.readout = readout
        self.input_size = int(input_size)
        self.hidden_size = int(hidden_size)
        self.batch_size = batch_size
        self.dropout = dropout
        self.normalization = normalization
        self.use_bias = use_bias
        self.alpha_lim = [math.exp(-1 / 5), math.exp(-1 / 25)]

        self.W = nn.Linear(self.input_size, self.hidden_size, bias=use_bias)
        self.alpha = nn.Parameter(torch.empty(self.hidden_size))
        nn.init.uniform_(self.alpha, self.alpha_lim[0], self.alpha_lim[1])
        norm, self.normalize = _make_norm(normalization, self.hidden_size)
        if norm is not None:
            self.norm = norm
        self.drop = nn.Dropout(p=dropout)

    def extra_repr(self):
        name = getattr(self, "readout", "softmax_sum")
        return "" if name == "softmax_sum" else f"readout={name}"

    def forward(self, x, u0=None, lengths=None, pack=None, per_step=None, return_state=False):
        """lengths: None, or prepare_lengths()'s result — out[b] is then the sum of softmax(u_t) over t < lengths[b].
        pack: None, or prepare_packing()'s result — x is the packed batch (1, n, feat); out and u0 hold the plan's
        `batch` rows in its sorted order.
        per_step: None — returns out (batch, classes) — or "prob" / "sum" — returns (out, seq) with seq (batch, time,
        classes) = softmax(u_t), or the running sum of `out` after step t (seq[:, -1] is out); with lengths, seq is 0
        at t >= lengths[b].  Both are differentiable.  Not with pack.
        return_state=True (stateful training): returns (out, {"u": u_T}) — out is this chunk's own sum, u_T a node of the
        graph; the default readout only, no lengths / pack / per_step."""
        Fn.seq_mode(per_step)
        readout = getattr(self, "readout", "softmax_sum")  # (a module pickled before the attribute: the default)
        Fn.readout_mode(readout)
        if return_state:
            _refuse_stateful_delays(self)
            Fn.check_stateful(lengths=lengths, pack=pack, per_step=per_step, readout=readout)
        if per_step is not None and readout != "softmax_sum":
            raise ValueError(f"sparch_amd: per_step with readout={readout!r} is not supported (the per-step readout is "
                             "the softmax-sum's)")
        if per_step is not None and pack is not None:
            raise ValueError("sparch_amd: per_step with pack is not supported (the per-step readout has no packed form)")
        if lengths is not None:
            _check_ragged_layer(self, lengths)
        if pack is not None:
            _check_packed_layer(self, pack, x)
        Fn._require_device(x, "input")
        x = _delayed_input(self, x, lengths, pack)  # (x itself without delays)
        layout_cfg, rows = _layout_cfg(x, lengths, pack)
        if u0 is None:
            u0 = _rand_to(rows, self.hidden_size, x.device)  # snns.py:812
        is_bn = self.normalization == "batchnorm"
        in_scale, in_s16 = _spike_tag(x)
        cfg = {
            "normalization": self.normalization if self.normalize else "none",
            "training": bool(self.training),
            "running_mean": self.norm.running_mean if is_bn else None,
            "running_var": self.norm.running_var if is_bn else None,
            "in_spike_scale": in_scale,
            "in_spike16": in_s16,  # the same spikes as a bf16 plane
            "num_batches_tracked": self.norm.num_batches_tracked if (is_bn and self.training) else None,
        }
        cfg.update(layout_cfg)
        if per_step is not None:
            cfg["per_step"] = per_step
        if readout != "softmax_sum":
            cfg["readout"] = readout
        nw = self.norm.weight if self.normalize else None
        nb = self.norm.bias if self.normalize else None
        if return_state:
            cfg["stateful"] = True
            out, u_T = Fn.ReadoutLayerFn.apply(cfg, x, self.W.weight, self.W.bias, nw, nb, self.alpha, u0)
            return out, {"u": u_T}
        return Fn.ReadoutLayerFn.apply(cfg, x, self.W.weight, self.W.bias, nw, nb, self.alpha, u0)

    def _readout_cell(self, Wx):
        Fn._require_device(Wx, "Wx")
        u0 = _rand_to(Wx.shape[0], Wx.shape[2], Wx.device)
        readout = getattr(self, "readout", "softmax_sum")
        if readout == "softmax_sum":
            return Fn.ReadoutCellFn.apply(Wx, self.alpha, u0)
        return Fn.ReadoutCellFn.apply(Wx, self.alpha, u0, readout)


def prepare_lengths(lengths, batch, T, device):
    """lengths (B,) integers on the host or the device, 1 <= lengths[b] <= T  ->  (int32 tensor on `device`, their sum):
    what the layers take as `lengths`.  Made once per forward: one upload (or one read-back of min, max and sum for
    lengths that are already on the device)."""
    lengths = torch.as_tensor(lengths)
    if lengths.ndim != 1 or lengths.shape[0] != batch or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
        raise ValueError(f"lengths: expected {batch} integers, one per batch row (got {tuple(lengths.shape)}, {lengths.dtype})")
    if lengths.device.type == "cpu":
        lo, hi, n_valid = int(lengths.min()), int(lengths.max()), int(lengths.sum())
    else:
        lo, hi, n_valid = torch.stack([lengths.min(), lengths.max(), lengths.sum()]).tolist()
    if lo < 1 or hi > T:
        raise ValueError(f"lengths: every entry must be in [1, {T}] (got min {lo}, max {hi})")
    lengths = lengths.to(torch.int32).contiguous()
    if lengths.device.type == "cpu" and torch.device(device).type != "cpu":
        # pinned and non-blocking: a pageable upload makes the host wait for everything queued on the device, once per
        # forward (measured: 0.8 ms of a 6.4 ms step at BASELINE configs[2])
        lengths = lengths.pin_memory().to(device, non_blocking=True)
    return lengths.to(device), int(n_valid)


def prepare_packing(lengths, batch, T, device):
    """lengths as prepare_lengths takes them (and refuses them)  ->  the functional.PackPlan of the batch: the stable
    descending order of the lengths, the sorted lengths, their exclusive prefix sum, n = sum(lengths) and the longest
    length.  Made on the host (lengths on the device cost one read-back) and uploaded as one pinned buffer."""
    import numpy as np

    lengths = torch.as_tensor(lengths)
    if lengths.ndim != 1 or lengths.shape[0] != batch or lengths.dtype.is_floating_point or lengths.dtype == torch.bool:
        raise ValueError(f"lengths: expected {batch} integers, one per batch row (got {tuple(lengths.shape)}, {lengths.dtype})")
    host = lengths.detach().to("cpu", torch.int64).numpy()
    lo, hi = int(host.min()), int(host.max())
    if lo < 1 or hi > T:
        raise ValueError(f"lengths: every entry must be in [1, {T}] (got min {lo}, max {hi})")
    order = np.argsort(-host, kind="stable")
    lens = host[order]
    n = int(lens.sum())
    if n >= 2 ** 31:
        raise ValueError(f"lengths: the packed batch has {n} rows, more than the int32 offsets hold")
    buf = np.empty(4 * batch + 1, np.int32)
    buf[:batch] = order
    buf[batch:2 * batch] = lens
    buf[2 * batch] = 0
    np.cumsum(lens, out=buf[2 * batch + 1:3 * batch + 1])
    buf[3 * batch + 1 + order] = np.arange(batch, dtype=np.int32)
    flat = torch.from_numpy(buf)
    if torch.device(device).type != "cpu":  # (pinned and non-blocking: see prepare_lengths)
        flat = flat.pin_memory().to(device, non_blocking=True)
    cut = lambda a, b: flat[a:b]  # noqa: E731
    host_views = (buf[:batch], buf[batch:2 * batch], buf[2 * batch:3 * batch + 1])
    return Fn.PackPlan(cut(0, batch), cut(batch, 2 * batch), cut(2 * batch, 3 * batch + 1), cut(3 * batch + 1, 4 * batch + 1),
                       n, int(lens[0]), int(batch), int(T), host_views)


def double_lengths(lengths):
    """prepare_lengths()'s result for the doubled batch of a bidirectional layer: every clip and, behind the batch, its
    reversed copy — the lengths twice, and twice their sum."""
    return torch.cat((lengths[0], lengths[0])), 2 * lengths[1]


def prepare_bidir_packing(plan, device):
    """The functional.BidirPlan of a bidirectional layer on the packed batch `plan` (prepare_packing's): the 2 * batch
    sequences — batch row b is clip b, row batch + b clip b read backwards — get a PackPlan of their own by
    prepare_packing's rules (stable descending order of the doubled lengths, exclusive prefix sum, inverse), and fwd /
    rev say where in that doubled packed tensor the two copies of sequence j of `plan` start.  Made on the host from
    plan.host and uploaded as one pinned buffer."""
    import numpy as np

    order, lens, _ = plan.host
    B = plan.batch
    if 2 * plan.n >= 2 ** 31:
        raise ValueError(f"lengths: the doubled packed batch has {2 * plan.n} rows, more than the int32 offsets hold")
    by_row = np.empty(B, np.int64)
    by_row[order] = lens
    twice = np.concatenate([by_row, by_row])
    order2 = np.argsort(-twice, kind="stable")
    lens2 = twice[order2]
    B2 = 2 * B
    buf = np.empty(4 * B2 + 1 + 2 * B, np.int32)
    buf[:B2] = order2
    buf[B2:2 * B2] = lens2
    buf[2 * B2] = 0
    np.cumsum(lens2, out=buf[2 * B2 + 1:3 * B2 + 1])
    inverse2 = np.empty(B2, np.int64)
    inverse2[order2] = np.arange(B2)
    buf[3 * B2 + 1:4 * B2 + 1] = inverse2
    offsets2 = buf[2 * B2:3 * B2 + 1]
    buf[4 * B2 + 1:4 * B2 + 1 + B] = offsets2[inverse2[order]]
    buf[4 * B2 + 1 + B:] = offsets2[inverse2[B + np.asarray(order, np.int64)]]
    flat = torch.from_numpy(buf)
    if torch.device(device).type != "cpu":  # (pinned and non-blocking: see prepare_lengths)
        flat = flat.pin_memory().to(device, non_blocking=True)
    cut = lambda a, b: flat[a:b]  # noqa: E731
    host_views = (buf[:B2], buf[B2:2 * B2], buf[2 * B2:3 * B2 + 1])
    plan2 = Fn.PackPlan(cut(0, B2), cut(B2, 2 * B2), cut(2 * B2, 3 * B2 + 1), cut(3 * B2 + 1, 4 * B2 + 1), 2 * plan.n,
                        plan.t_max, B2, plan.T, host_views)
    return Fn.BidirPlan(plan2, cut(4 * B2 + 1, 4 * B2 + 1 + B), cut(4 * B2 + 1 + B, 4 * B2 + 1 + 2 * B))


def _check_packed_layer(layer, plan=None, x=None):
    """What a layer refuses with pack=True; plan / x: also checked to be prepare_packing()'s and
    the packed batch that goes with it."""
    if plan is not None and not isinstance(plan, Fn.PackPlan):
        raise ValueError("pack: pass what snns.prepare_packing() returns (SNN.forward(x, lengths, pack=True) does so itself)")
    if plan is not None and x is not None and (x.ndim != 3 or x.shape[0] != 1 or x.shape[1] != plan.n):
        raise ValueError(f"pack: the layer's input must be the packed batch (1, {plan.n}, features), got {tuple(x.shape)}")
    Fn._check_packed(True if plan is None else plan, 2 if getattr(layer, "bidirectional", False) else 1, hasattr(layer, "V"),
                     layer.hidden_size)
    if Fn.SYNC_BN is not None and Fn.SYNC_BN["world"] > 1:
        raise ValueError("sparch_amd: pack=True with --sync_bn is not supported")


def _check_ragged_layer(layer, lengths=None):
    """What a layer refuses with lengths; lengths: also checked to be prepare_lengths()'s."""
    if lengths is not None and not (isinstance(lengths, tuple) and len(lengths) == 2 and torch.is_tensor(lengths[0])
                                    and lengths[0].dtype == torch.int32):
        raise ValueError("lengths: pass what snns.prepare_lengths() returns (SNN.forward does so itself)")
    Fn._check_ragged(True, 2 if getattr(layer, "bidirectional", False) else 1, hasattr(layer, "V"), layer.hidden_size)
    if layer.normalization == "batchnorm" and layer.normalize and layer.use_bias:
        raise ValueError("sparch_amd: lengths with BatchNorm and use_bias=True is not supported (the bias makes the "
                         "padded rows non-zero, and BatchNorm removes the bias anyway)")
    if Fn.SYNC_BN is not None and Fn.SYNC_BN["world"] > 1:
        raise ValueError("sparch_amd: lengths with --sync_bn is not supported")


def _check_bidir_input(net, x, what):
    """A bidirectional network with lengths refuses a host tensor with the other refusals, as a ValueError before the
    first kernel: the reverse direction's flip inside each clip's own length exists as HIP kernels
    only (csrc/bidir.hip)."""
    if net.bidirectional and x.device.type != "cuda":
        raise ValueError(f"sparch_amd: {what} with bidirectional=True takes an input on the HIP device (got {x.device}: the "
                         "reverse direction flips inside each clip's own length in kernels that have no host form)")


_LAYER_CLASSES = {"LIF": LIFLayer, "adLIF": adLIFLayer, "RLIF": RLIFLayer, "RadLIF": RadLIFLayer}


def detach_state(state):
    """A state as SNN.forward(return_state=True) returns it, cut out of the graph: fed to the next chunk it gives
    classic truncated BPTT (no gradient crosses the boundary, and the chunk's saved tensors are freed by its own
    backward)."""
    return [{k: v.detach() for k, v in st.items()} if isinstance(st, dict) else st.detach() for st in state]


def _global_forward_hooks():
    """True if torch.nn.modules.module has forward hooks registered for ALL modules (they would see a layer's output)."""
    import torch.nn.modules.module as _m

    return bool(getattr(_m, "_global_forward_hooks", None)) or bool(getattr(_m, "_global_forward_hooks_always_called", None))


class SNN(nn.Module):
    """Multi-layer spiking network (reference SNN, snns.py:39-176).

    forward(x: (batch, time, feat) or 4-D (batch, time, feat, channel), lengths=None) ->
        (out, firing_rates): out is (batch, classes) with a readout layer, else
        (batch, time, feats); firing_rates has one entry per hidden neuron (all layers).

    lengths (ragged batches): integers (batch,), on the host or the device, 1 <= lengths[b] <=
    time, for an x that is ZERO at every row's steps t >= lengths[b] (what pad_sequence gives).  Row b of every output
    is then what the network gives for x[b:b+1, :lengths[b]] run on its own with the same initial-state rows (in train
    mode: with the same normalisation statistics, taken over the valid steps): hidden spikes are 0 on the padding, the
    readout sums over the row's own steps, firing rates are means over valid steps.  None: every row runs to `time`,
    as the reference does.  With bidirectional=True ("Bidirectional ragged batches") the reverse
    direction reads every clip backwards inside its own length — columns H: of a hidden layer's row b at step t are its
    state after the clip's steps lengths[b]-1 .. t — and each direction's firing rate is its own mean over the valid
    steps; also with pack=True.

    pack=True (with lengths; DESIGN.md section 6, "Packed ragged batches"): the same contract, but the padded steps are
    skipped instead of masked — the batch is packed to (sum(lengths), feat) rows, sorted by length, once; every layer runs
    on packed tensors; out and the firing rates come back in the caller's row order (without a readout layer the spikes
    are unpacked to (batch, time, feats) with zero tails).  x need not be zero on the padding: it is never read.
    Differences from the masked mode: dropout masks are indexed by the position in the packed tensor, no state exists
    for t >= lengths[b], and BatchNorm with use_bias=True is accepted.

    per_step="prob" / "sum" ("Per-step readout"; needs a readout layer, not with pack): forward
    returns THREE values, (out, firing_rates, seq): seq (batch, time, classes) is the readout after every step —
    softmax(u_t), or the running sum whose last step is `out` (row t is what StreamingSNN.step returns after t + 1
    steps).  With lengths, seq[b, t] is 0 for t >= lengths[b].  A loss may use out, seq or both.  per_step=None (the
    default): the two values above, nothing else changes.

    readout="softmax_sum" (the default) / "softmax_mean" / "u_max" / "u_mean" / "u_last" (DESIGN.md section 6,
    "Selectable readout"): the readout layer's reduction over time (ReadoutLayer); with lengths, also packed, over the
    row's own steps.  per_step needs the default.

    max_delay=D (1 .. 255; 0, the default: no delays, nothing registered; DESIGN.md section 6, "Axonal delays"): every
    layer — with delay_layers="hidden" every layer but the first — owns a parameter `delay` (one entry per input
    feature) and reads its input shifted by d_i = rint(clamp(delay_i, 0, D)) steps per feature, inside each row's own
    length; spikes shifted past a clip's end are dropped.  delay_init="zero" / "uniform" (in [0, D]);
    learn_delays=False keeps them fixed (no gradient).  The delay's gradient is the finite difference of the delayed
    input.  Not with state / return_state."""

    def __init__(self, input_shape, layer_sizes, neuron_type="LIF", threshold=1.0, dropout=0.0,
                 normalization="batchnorm", use_bias=False, bidirectional=False, use_readout_layer=True,
                 surrogate="boxcar", surrogate_scale=None, readout="softmax_sum", max_delay=0, delay_init="zero",
                 learn_delays=True, delay_layers="all", synapse=None, syn_init="uniform", learn_synapse=True,
                 synapse_layers="all"):
        super().__init__()
        self.synapse = Fn.check_synapse(synapse)
        if syn_init not in SYN_INITS:
            raise ValueError(f"sparch_amd: syn_init must be one of {', '.join(SYN_INITS)} (got {syn_init!r})")
        if synapse_layers not in SYN_LAYERS:
            raise ValueError(f"sparch_amd: synapse_layers must be one of {', '.join(SYN_LAYERS)} (got {synapse_layers!r})")
        self.syn_init, self.synapse_layers, self.learn_synapse = syn_init, synapse_layers, bool(learn_synapse)
        Fn.readout_mode(readout)
        Fn.check_max_delay(max_delay, zero_ok=True)
        if delay_init not in DELAY_INITS:
            raise ValueError(f"sparch_amd: delay_init must be one of {', '.join(DELAY_INITS)} (got {delay_init!r})")
        if delay_layers not in DELAY_LAYERS:
            raise ValueError(f"sparch_amd: delay_layers must be one of {', '.join(DELAY_LAYERS)} (got {delay_layers!r})")
        self.max_delay, self.delay_init, self.delay_layers = max_delay, delay_init, delay_layers
        self.learn_delays = bool(learn_delays)
        self.readout = readout
        self.surrogate, self.surrogate_scale = resolve_surrogate(surrogate, surrogate_scale)
        self.reshape = len(input_shape) > 3
        self.input_size = float(torch.prod(torch.tensor(input_shape[2:])))
        self.batch_size = input_shape[0]
        self.layer_sizes = layer_sizes
        self.num_layers = len(layer_sizes)
        self.num_outputs = layer_sizes[-1]
        self.neuron_type = neuron_type
        self.threshold = threshold
        self.dropout = dropout
        self.normalization = normalization
        self.use_bias = use_bias
        self.bidirectional = bidirectional
        self.use_readout_layer = use_readout_layer
        self.is_snn = True

        if neuron_type not in _SPIKING_KINDS:
            raise ValueError(f"Invalid neuron type {neuron_type}")

        self.snn = self._init_layers()
        self._init_delays()
        self._init_synapses()

    def _init_synapses(self):
        """Synaptic currents: every hidden spiking layer — with synapse_layers="hidden" every one
        but the first — gets `synapse` = (lo, hi) and an nn.Parameter `gamma`, one entry per neuron, U(lo, hi) or lo.
        Made after the whole network (and its delays), so that under one seed every other parameter is what it is
        without a synapse; synapse=None registers nothing (the state_dict keys are the reference's).  The readout layer
        never has one."""
        if self.synapse is None:
            return
        lo, hi = self.synapse
        n_hidden = self.num_layers - 1 if self.use_readout_layer else self.num_layers
        for i, layer in enumerate(self.snn[:n_hidden]):
            if i == 0 and self.synapse_layers == "hidden":
                continue
            layer.synapse = (lo, hi)
            init = torch.full((layer.hidden_size,), lo)
            if self.syn_init == "uniform":
                init.uniform_(lo, hi)
            layer.gamma = nn.Parameter(init, requires_grad=self.learn_synapse)

    def synapse_gammas(self):
        """{layer index: the clamped gamma (H,) as the kernels take it} of the layers with a synapse — for logging."""
        return {i: layer.gamma.detach().float().clamp(*layer.synapse)
                for i, layer in enumerate(self.snn) if getattr(layer, "synapse", None) is not None}

    def _init_delays(self):
        """Axonal delays: every delayed layer gets `max_delay` and an nn.Parameter `delay`, one
        entry per input feature.  Made after the whole network, so that under one seed every other parameter is what it
        is without delays; max_delay = 0 registers nothing (the state_dict keys are the reference's)."""
        if not self.max_delay:
            return
        for i, layer in enumerate(self.snn):
            if i == 0 and self.delay_layers == "hidden":
                continue
            layer.max_delay = self.max_delay
            init = torch.zeros(layer.input_size)
            if self.delay_init == "uniform":
                init.uniform_(0.0, float(self.max_delay))
            layer.delay = nn.Parameter(init, requires_grad=self.learn_delays)

    def delay_steps(self):
        """{layer index: the integer delays d = rint(clamp(delay, 0, max_delay)) as the kernels take them (K,) int64}
        of the delayed layers — for logging; the forward pass never reads the parameter on the host."""
        res = {}
        for i, layer in enumerate(self.snn):
            if getattr(layer, "max_delay", 0):
                res[i] = torch.round(layer.delay.detach().float().clamp(0, layer.max_delay)).long()
        return res

    def _init_layers(self):
        layers = nn.ModuleList([])
        layer_cls = _LAYER_CLASSES[self.neuron_type]
        n_hidden = self.num_layers - 1 if self.use_readout_layer else self.num_layers
        fan_in = self.input_size
        for i in range(n_hidden):
            layers.append(layer_cls(
                input_size=fan_in, hidden_size=self.layer_sizes[i], batch_size=self.batch_size,
                threshold=self.threshold, dropout=self.dropout, normalization=self.normalization,
                use_bias=self.use_bias, bidirectional=self.bidirectional, surrogate=self.surrogate,
                surrogate_scale=self.surrogate_scale))
            layers[-1]._layer_index = i
            fan_in = self.layer_sizes[i] * (1 + self.bidirectional)
        if self.use_readout_layer:
            layers.append(ReadoutLayer(
                input_size=fan_in, hidden_size=self.layer_sizes[-1], batch_size=self.batch_size,
                dropout=self.dropout, normalization=self.normalization, use_bias=self.use_bias,
                readout=self.readout))
        return layers

    def extra_repr(self):
        name = getattr(self, "surrogate", "boxcar")
        parts = [] if name == "boxcar" else [f"surrogate={name}, surrogate_scale={getattr(self, 'surrogate_scale', None):g}"]
        if getattr(self, "readout", "softmax_sum") != "softmax_sum":
            parts.append(f"readout={self.readout}")
        if getattr(self, "max_delay", 0):
            parts.append(f"max_delay={self.max_delay}, delay_init={self.delay_init}, learn_delays={self.learn_delays}, "
                         f"delay_layers={self.delay_layers}")
        if getattr(self, "synapse", None) is not None:
            parts.append(f"synapse=({self.synapse[0]:g}, {self.synapse[1]:g}), syn_init={self.syn_init}, "
                         f"learn_synapse={self.learn_synapse}, synapse_layers={self.synapse_layers}")
        return ", ".join(parts)

    def draw_states(self, batch, device, out=None):
        """Every layer's initial states for one forward, drawn from torch's global CPU generator in the
        reference's order (per hidden layer u, [w], s; then the readout's u): a list with one (u0, w0, s0)
        tuple per hidden layer and the readout's u0 tensor last.  out: the flat buffer of an earlier call
        (`.flat` of its result) to refill in place."""
        last = self.num_layers - 1
        shapes, plan = [], []
        for i, layer in enumerate(self.snn):
            if self.use_readout_layer and i == last:
                shapes.append((batch, layer.hidden_size))
                plan.append(None)
            else:
                rows = batch * (2 if layer.bidirectional else 1)
                adaptive = layer.kind in ("adLIF", "RadLIF")
                shapes += [(rows, layer.hidden_size)] * (3 if adaptive else 2)
                plan.append(adaptive)
        batch_list = _rand_batch(shapes, device, out=out)  # one staging buffer, one copy for the whole forward
        drawn = iter(batch_list)
        states = []
        for adaptive in plan:
            if adaptive is None:
                states.append(next(drawn))
            else:
                u0 = next(drawn)
                w0 = next(drawn) if adaptive else None
                states.append((u0, w0, next(drawn)))
        states = _StateList(states, batch_list.flat, batch_list.ready)
        return states

    def __getstate__(self):
        """Whole-module checkpoints (`torch.save(self.net)`, exp.py:462) hold the network, not a step's transient
        device state: the static states of a captured step (an event handle among them) stay out."""
        state = dict(self.__dict__)
        for k in ("_static_states", "_state_flat"):
            state.pop(k, None)
        return state

    def draw_states_into(self, static_states, batch):
        """The same draws (same generator, same order) written into the EXISTING device tensors `static_states`
        (an earlier draw_states result) — the static inputs of a captured step (sparch_amd.graph): one staging
        buffer and one stream-ordered copy into their common allocation."""
        flat = getattr(static_states, "flat", None)
        if flat is not None:
            self.draw_states(batch, flat.device, out=flat)
            return

        def fill(dst):
            dst.copy_(torch.rand(dst.shape[0], dst.shape[1], pin_memory=True), non_blocking=True)

        last = self.num_layers - 1
        for i, (layer, dst) in enumerate(zip(self.snn, static_states)):
            if self.use_readout_layer and i == last:
                fill(dst)
            else:
                u0, w0, s0 = dst
                assert u0.shape[0] == batch * (2 if layer.bidirectional else 1)
                fill(u0)
                if w0 is not None:
                    fill(w0)
                fill(s0)

    def _check_stateful(self, lengths, pack, per_step, T):
        """Every refusal of state / return_state, before the first kernel."""
        if getattr(self, "_static_states", None) is not None:
            raise ValueError("sparch_amd: state / return_state inside a captured step (GraphedTrainStep) is not "
                             "supported: the carried state changes with every chunk")
        last = self.num_layers - 1
        for layer in self.snn:
            _refuse_stateful_delays(layer)
        for i, layer in enumerate(self.snn):
            if self.use_readout_layer and i == last:
                Fn.check_stateful(lengths=lengths, pack=pack if pack else None, per_step=per_step,
                                  readout=getattr(layer, "readout", "softmax_sum"))
            else:
                Fn.check_stateful(layer.kind, layer.hidden_size, dirs=2 if layer.bidirectional else 1, lengths=lengths,
                                  pack=pack if pack else None, per_step=per_step, T=T)

    def _states_from(self, state, batch, device):
        """A caller's `state` (one dict per layer, StreamingSNN.get_state()'s format; other keys, such as its `out` and
        `steps`, are ignored) -> the list SNN.forward runs on: (u0, w0, s0) per hidden layer, the readout's u0 last."""
        if len(state) != len(self.snn):
            raise ValueError(f"sparch_amd: state has {len(state)} entries for {len(self.snn)} layers")
        last = self.num_layers - 1

        def take(st, what, i, cols):
            t = st.get(what) if isinstance(st, dict) else None
            if not torch.is_tensor(t):
                raise ValueError(f"sparch_amd: state[{i}] has no {what!r}")
            if tuple(t.shape) != (batch, cols):
                raise ValueError(f"sparch_amd: state[{i}][{what!r}] is {tuple(t.shape)}, expected {(batch, cols)}")
            if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"sparch_amd: state[{i}][{what!r}] must be a contiguous float32 tensor on {device}")
            return t

        states = []
        for i, (layer, st) in enumerate(zip(self.snn, state)):
            if self.use_readout_layer and i == last:
                states.append(take(st, "u", i, layer.hidden_size))
                continue
            adaptive = layer.kind in ("adLIF", "RadLIF")
            states.append((take(st, "u", i, layer.hidden_size), take(st, "w", i, layer.hidden_size) if adaptive else None,
                           take(st, "s", i, layer.hidden_size)))
        return states

    def forward(self, x, lengths=None, pack=False, per_step=None, state=None, return_state=False):
        """state / return_state (stateful training): `out, rates, state = net(x, state=st,
        return_state=True)` starts every layer from `st` — a list with one entry per layer, {"u", ["w",] "s"} (batch,
        hidden) per hidden layer and {"u"} (batch, classes) for the readout, StreamingSNN.get_state()'s format — instead
        of drawing from the host generator, and returns the state the chunk ended in: u_T, w_T and the raw spike
        s_T = 1[u_T > threshold] (before dropout) per hidden layer, u_T for the readout.  `out` is the chunk's own
        softmax-sum: the caller adds chunks.  The returned tensors are nodes of the graph: kept, the gradient crosses
        the chunk boundary exactly; through detach_state() it is classic truncated BPTT.  A `state` tensor with
        requires_grad gets its gradient.  state=None draws as always; return_state=False returns what it always did."""
        stateful = state is not None or return_state
        if getattr(self, "synapse", None) is not None:  # (the refusals come before anything else)
            if getattr(self, "_static_states", None) is not None:
                raise ValueError("sparch_amd: a synapse inside a captured step (GraphedTrainStep) is not supported")
            for layer in self.snn:
                if getattr(layer, "synapse", None) is not None:
                    _check_synapse_call(layer, pack=True if pack else None, stateful=stateful)
        if stateful:  # (the refusals come before anything else)
            self._check_stateful(lengths, pack, per_step, x.shape[1])
            if state is not None:
                state = self._states_from(state, x.shape[0], x.device)
        if per_step is not None:  # (the refusals come before anything else)
            Fn.seq_mode(per_step)
            if pack:
                raise ValueError("sparch_amd: per_step with pack=True is not supported (the per-step readout has no "
                                 "packed form)")
            if not self.use_readout_layer:
                raise ValueError("sparch_amd: per_step needs a readout layer (use_readout_layer=True)")
            readout = getattr(self.snn[-1], "readout", "softmax_sum")
            if readout != "softmax_sum":
                raise ValueError(f"sparch_amd: per_step with readout={readout!r} is not supported (the per-step readout "
                                 "is the softmax-sum's)")
        if self.reshape:
            if x.ndim == 4:
                x = x.reshape(x.shape[0], x.shape[1], x.shape[2] * x.shape[3])
            else:
                raise NotImplementedError
        if pack:
            return self._forward_packed(x, lengths)
        if lengths is not None:  # (the refusals come before anything else, the device check included)
            if getattr(self, "_static_states", None) is not None:
                raise ValueError("sparch_amd: lengths inside a captured step (GraphedTrainStep) is not supported: the "
                                 "lengths and their sum change with every batch")
            for layer in self.snn:  # every refusal before the first kernel
                _check_ragged_layer(layer)
            _check_bidir_input(self, x, "lengths")
            lengths = prepare_lengths(lengths, x.shape[0], x.shape[1], x.device)  # on the device once per forward
            if x.requires_grad:  # the input's gradient is 0 on the padding (x is 0 there: the values do not change)
                steps = torch.arange(x.shape[1], device=x.device)
                x = x * (steps[None, :] < lengths[0][:, None]).unsqueeze(-1).to(x.dtype)
        Fn._require_device(x, "input")
        # All initial states of this forward are drawn NOW, in the reference's order (layer by layer u, [w], s,
        # then the readout's u: snns.py:286-287 ... 812) from the same CPU generator, so the stream is the one
        # the reference consumes — but the host does its ~MBs of torch.rand while the GPU is still busy with
        # the previous step, instead of stalling the queue between two layers (120 us bubbles per layer in
        # the round-2 kernel trace).
        last = self.num_layers - 1
        states = getattr(self, "_static_states", None)  # graph mode: refilled by draw_states_into() per step
        if state is not None:  # a carried state: nothing is drawn
            states = state
        elif states is None:
            states = self.draw_states(x.shape[0], x.device)
        rates = []
        final = []  # stateful: every layer's final state
        ragged_kw = {} if lengths is None else {"lengths": lengths}
        if lengths is not None and self.bidirectional:  # the doubled batch's lengths, once for all layers
            ragged_kw["lengths2"] = double_lengths(lengths)
        wait = getattr(states, "wait_ready", None)  # the states' upload runs under the first projection GEMM
        for i, layer in enumerate(self.snn):
            if self.use_readout_layer and i == last:
                if wait is not None:
                    wait()
                x = layer(x, u0=states[i], lengths=lengths, per_step=per_step, return_state=stateful)
                if stateful:
                    x, st = x
                    final.append(st)
                elif per_step is not None:
                    x, seq = x
            else:
                # between two layers of ours the spikes travel as a bf16 plane: no fp32 copy (unless somebody
                # else may look at the layer's output: forward hooks, the network's own output)
                inner = i + 1 < len(self.snn) and not layer._forward_hooks and not _global_forward_hooks()
                if stateful:
                    x, r, st = layer.forward_with_rate(x, states=states[i], states_ready=wait if i == 0 else None,
                                                       fp32_out=not inner, return_state=True)
                    final.append(st)
                else:
                    x, r = layer.forward_with_rate(x, states=states[i], states_ready=wait if i == 0 else None,
                                                   fp32_out=not inner, **ragged_kw)
                if wait is not None:
                    wait()  # (no-op once the first layer's call has waited)
                rates.append(r)
        firing_rates = torch.cat(rates) if len(rates) > 1 else rates[0]
        if return_state:
            return x, firing_rates, final
        if per_step is not None:
            return x, firing_rates, seq
        return x, firing_rates

    def _forward_packed(self, x, lengths):
        """forward(x, lengths, pack=True): the batch packed once, every layer on packed tensors, the results back in the
        caller's row order (class docstring)."""
        if lengths is None:
            raise ValueError("sparch_amd: pack=True needs lengths (the packed layout is made from them)")
        if getattr(self, "_static_states", None) is not None:
            raise ValueError("sparch_amd: pack=True inside a captured step (GraphedTrainStep) is not supported: the "
                             "lengths, their order and their sum change with every batch")
        for layer in self.snn:  # every refusal before the first kernel
            _check_packed_layer(layer)
        batch, T = x.shape[0], x.shape[1]
        plan = prepare_packing(lengths, batch, T, x.device)
        for layer in self.snn:  # (what depends on the batch's longest sequence: chunked recurrent launches)
            _check_packed_layer(layer, plan)
        _check_bidir_input(self, x, "pack=True")
        Fn._require_device(x, "input")
        tag = Fn.input_plane_of(x)
        if tag is not None:  # input_from_counts: the bf16 plane is the data, x a placeholder without values
            plane = Fn.pack_rows(tag[0].view(batch, T, -1), plan)
            x = Fn.spike_placeholder(1, plan.n, x.shape[2], x.device).view(1, plan.n, x.shape[2])
            x._sparch_input_plane = (tuple(x.shape), plane, tag[1])
        else:
            if x.element_size() not in (1, 2, 4):
                x = x.float()
            x = Fn.PackRowsFn.apply(x, plan).unsqueeze(0)
        # the draws are the padded forward's (same generator, same order, one row per batch row); each sequence takes
        # its own row with it
        states = self.draw_states(batch, x.device)
        states.wait_ready()
        take = lambda t_: None if t_ is None else t_.index_select(0, plan.order)  # noqa: E731
        # bidirectional layers: 2 * batch state rows (row batch + b the reverse direction of clip b), in the doubled
        # batch's own sorted order
        plan2 = prepare_bidir_packing(plan, x.device) if self.bidirectional else None
        take2 = lambda t_: None if t_ is None else t_.index_select(0, plan2.plan.order)  # noqa: E731
        last = self.num_layers - 1
        rates = []
        for i, layer in enumerate(self.snn):
            if self.use_readout_layer and i == last:
                x = layer(x, u0=take(states[i]), pack=plan).index_select(0, plan.inverse)
            else:
                inner = i + 1 < len(self.snn) and not layer._forward_hooks and not _global_forward_hooks()
                rows_of = take2 if layer.bidirectional else take
                x, r = layer.forward_with_rate(x, states=tuple(rows_of(t_) for t_ in states[i]), fp32_out=not inner,
                                               pack=plan, pack2=plan2)
                rates.append(r)
        if not self.use_readout_layer:
            x = Fn.UnpackRowsFn.apply(x.reshape(plan.n, -1), plan)
        firing_rates = torch.cat(rates) if len(rates) > 1 else rates[0]
        return x, firing_rates
