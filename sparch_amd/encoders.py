"""
Spike encoders: real-valued features (B,T,K) -> spike counts ON THE DEVICE (csrc/encode.hip, `sparch_spike_encode`;
include/sparch_hip.h, "Spike encoders").  The result is what the network already takes from a
batch of binned events: the bf16 count plane behind a tagged placeholder (`functional.input_from_counts`), so that layer
0 of a network trained on audio runs the exact spike products like every other layer — spiking end to end.

    rate   one Bernoulli spike per element and step with p = clamp((x - lo) * scale, 0, 1); stateless, seeded
    if     integrate-and-fire: a non-leaky integrator per feature emits floor(v) and keeps the fraction; deterministic
    delta  send-on-delta: ON / OFF spikes whenever the feature has moved by a whole threshold since the last one sent;
           2 K output features

`SpikeEncoder.encode` turns a whole batch, `StreamingSpikeEncoder.push` a stream's next chunk (state and step count
carried: chunks give the whole sequence's spikes, bit for bit).  There is no CPU path.
"""
import math

import torch

from . import functional as Fn
from ._capi import check, lib, ptr

CODES = {"rate": 0, "if": 1, "delta": 2}
PREFETCH_DEPTH = 8     # SPARCH_ENCODE_PREFETCH: steps in flight per thread of the if / delta kernels
OUTPUTS = ("input", "counts", "dense")
_M64 = (1 << 64) - 1


def _mix64(base, n):
    """Seed n of the sequence that starts at `base` (splitmix64 on the host: no device work, no sync)."""
    z = (int(base) + (int(n) + 1) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return (z ^ (z >> 31)) & ~(1 << 63) & _M64   # bit 63 stays clear (SPARCH_SEED_IN_MEMORY marks an address elsewhere)


def parse_encode(spec):
    """`code[:key=value,...]` -> {"code": ..., key: value, ...}; None or empty -> None.  code: rate, if, delta.  Keys of
    rate and if: gain, lo, hi (numbers; hi > lo, gain > 0) and seed (an integer >= 0); of delta: delta (> 0) and seed.
    Each key at most once; anything else is refused with a ValueError."""
    if spec is None or spec.strip() == "":
        return None
    text = spec.strip()

    def bad(why):
        return ValueError(f"SPARCH_ENCODE={spec!r}: {why} (code[:key=value,...] with code rate | if | delta; keys "
                          "gain, lo, hi, seed for rate and if, delta and seed for delta)")

    head, sep, tail = text.partition(":")
    code = head.strip()
    if code not in CODES:
        raise bad(f"unknown code {code!r}")
    if sep and tail.strip() == "":
        raise bad("no key behind ':'")
    allowed = ("delta", "seed") if code == "delta" else ("gain", "lo", "hi", "seed")
    res = {"code": code}
    for item in (tail.split(",") if sep else []):
        key, eq, value = item.partition("=")
        key, value = key.strip(), value.strip()
        if not eq or key not in allowed or key in res or value == "":
            raise bad(f"bad item {item.strip()!r}")
        try:
            res[key] = int(value) if key == "seed" else float(value)
        except ValueError:
            raise bad(f"{key}={value!r} is not a number") from None
        if key == "seed" and res[key] < 0:
            raise bad("seed must be >= 0")
        if key != "seed" and not math.isfinite(res[key]):
            raise bad(f"{key} must be finite")
    if res.get("gain", 1.0) <= 0 or res.get("delta", 1.0) <= 0:
        raise bad("gain and delta must be > 0")
    if res.get("hi", 1.0) <= res.get("lo", 0.0):
        raise bad("hi must be above lo")
    return res


def _per_feature(value, K, what):
    t = torch.as_tensor(value, dtype=torch.float32).detach().to("cpu")
    if t.ndim == 0:
        t = t.expand(K)
    if t.shape != (K,):
        raise ValueError(f"SpikeEncoder: {what} is a scalar or a ({K},) vector (got {tuple(t.shape)})")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"SpikeEncoder: {what} must be finite")
    return t.clone().contiguous()


def _lengths_i32(lengths, B, device):
    if lengths is None:
        return None
    t = torch.as_tensor(lengths)
    if t.ndim != 1 or t.shape[0] != B or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"lengths: expected {B} integers, one per batch row (got {tuple(t.shape)}, {t.dtype})")
    t = t.to(torch.int32).contiguous()
    if t.device.type == "cpu":
        t = (t.pin_memory() if torch.cuda.is_available() else t).to(device, non_blocking=True)
    return t.to(device)


class SpikeEncoder:
    """SpikeEncoder(code, num_features, lo=0.0, hi=1.0, gain=1.0, delta=None, seed=None).

    rate / if: z = (x - lo) * scale with scale = gain / (hi - lo) (fp32; lo, hi scalars or (K,)): at gain 1 a feature at
    `hi` spikes with probability 1 (rate) or once per step (if).  delta: z = x / delta (lo = 0, scale = 1 / delta),
    `out_features` = 2 K: column k the ON spikes of feature k, column K + k the OFF spikes.
    seed: the base of the encoder's own seed sequence (rate; default torch.initial_seed()); every `encode` without a
    seed of its own takes the next one — drawn on the host, no sync."""

    def __init__(self, code, num_features, lo=None, hi=None, gain=1.0, delta=None, seed=None):
        if code not in CODES:
            raise ValueError(f"SpikeEncoder: code is one of {', '.join(CODES)} (got {code!r})")
        K = int(num_features)
        if K < 1 or isinstance(num_features, bool) or K != num_features:
            raise ValueError(f"SpikeEncoder: num_features is an integer >= 1 (got {num_features!r})")
        self.code, self.num_features = code, K
        self.out_features = int(lib.sparch_spike_encode_width(CODES[code], K))
        if self.out_features < 1 or self.out_features > 65535:
            raise ValueError(f"SpikeEncoder: {self.out_features or 2 * K} output features (the limit is 65535)")
        if code == "delta":
            if lo is not None or hi is not None or gain != 1.0:
                raise ValueError("SpikeEncoder: the delta code takes its threshold `delta`, not lo / hi / gain")
            d = _per_feature(1.0 if delta is None else delta, K, "delta")
            if not bool((d > 0).all()):
                raise ValueError("SpikeEncoder: delta must be > 0")
            self.gain = 1.0
            self._set(torch.zeros(K), None, 1.0 / d)
        else:
            if delta is not None:
                raise ValueError(f"SpikeEncoder: `delta` belongs to the delta code (got code {code!r})")
            self.gain = float(gain)
            if not (0 < self.gain < float("inf")):
                raise ValueError(f"SpikeEncoder: gain must be a finite number > 0 (got {gain!r})")
            self.set_range(0.0 if lo is None else lo, 1.0 if hi is None else hi)
        self.base_seed = (torch.initial_seed() if seed is None else int(seed)) & _M64
        self.calls = 0
        self._device = {}     # device -> (lo, scale, totals)

    @classmethod
    def from_spec(cls, spec, num_features):
        """The encoder of a `parse_encode` result (or of the string itself)."""
        spec = parse_encode(spec) if isinstance(spec, str) else dict(spec)
        return cls(spec.pop("code"), num_features, **spec)

    def __repr__(self):
        return f"SpikeEncoder({self.code!r}, {self.num_features} -> {self.out_features} features, gain={self.gain:g})"

    # ------------------------------------------------------------------ parameters
    def _set(self, lo, hi, scale):
        self.lo, self.hi, self.scale = lo.contiguous(), hi, scale.to(torch.float32).contiguous()
        self._device = {}

    def set_range(self, lo, hi):
        """Per-feature range of the rate / if codes: scale = fp32(gain) / (fp32(hi) - fp32(lo))."""
        if self.code == "delta":
            raise ValueError("SpikeEncoder: the delta code has no range (its threshold is `delta`)")
        K = self.num_features
        lo, hi = _per_feature(lo, K, "lo"), _per_feature(hi, K, "hi")
        if not bool((hi > lo).all()):
            raise ValueError("SpikeEncoder: hi must be above lo for every feature")
        scale = torch.tensor(self.gain, dtype=torch.float32) / (hi - lo)
        if not bool(torch.isfinite(scale).all()):
            raise ValueError("SpikeEncoder: gain / (hi - lo) is not finite in fp32")
        self._set(lo, hi, scale)

    def calibrate(self, x, lengths=None):
        """Set lo / hi per feature to the smallest / largest finite value over the valid steps of the batch x (B,T,K)
        (a feature that does not move gets hi = lo + 1).  One read-back; not a per-step call."""
        x = self._checked(x)
        B, T, K = x.shape
        ok = torch.isfinite(x)
        if lengths is not None:
            lens = _lengths_i32(lengths, B, x.device)
            ok &= (torch.arange(T, device=x.device)[None, :] < lens[:, None])[:, :, None]
        inf = torch.tensor(float("inf"), device=x.device)
        lo = torch.where(ok, x, inf).amin(dim=(0, 1))
        hi = torch.where(ok, x, -inf).amax(dim=(0, 1))
        lo, hi = lo.cpu(), hi.cpu()
        if not bool(torch.isfinite(lo).all()):
            raise ValueError("SpikeEncoder.calibrate: a feature has no finite value on a valid step")
        hi = torch.where(hi > lo, hi, lo + 1.0)
        self.set_range(lo, hi)
        return self

    def _on(self, device):
        key = str(device)
        got = self._device.get(key)
        if got is None:
            got = self._device[key] = (self.lo.to(device), self.scale.to(device),
                                       torch.zeros(self.out_features, dtype=torch.int32, device=device))
        return got

    def totals(self):
        """(K',) int64 on the host: the spikes emitted per output feature since the last call (one read-back)."""
        res = torch.zeros(self.out_features, dtype=torch.int64)
        for _, _, tot in self._device.values():
            res += tot.cpu().to(torch.int64) & 0xFFFFFFFF   # the kernels add uint32
            tot.zero_()
        return res

    def next_seed(self):
        s = _mix64(self.base_seed, self.calls)
        self.calls += 1
        return s

    # ------------------------------------------------------------------ encoding
    def _checked(self, x):
        if not isinstance(x, torch.Tensor) or x.ndim != 3 or x.shape[2] != self.num_features or not x.is_floating_point():
            raise ValueError(f"SpikeEncoder: a (B, T, {self.num_features}) floating-point tensor of features, got "
                             f"{tuple(getattr(x, 'shape', ()))}")
        Fn._require_device(x, "the encoder's input")
        if x.requires_grad:
            raise ValueError("SpikeEncoder: the encoders have no gradient; detach the features first")
        if x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"SpikeEncoder: an empty batch or sequence, {tuple(x.shape)}")
        return Fn._f32c(x)

    def _run(self, x, lengths, out, seed, state, fresh, t0):
        """One `sparch_spike_encode` call on checked features; returns the requested output."""
        if out not in OUTPUTS:
            raise ValueError(f"SpikeEncoder: out is one of {', '.join(OUTPUTS)} (got {out!r})")
        B, T, K = x.shape
        KW, dev = self.out_features, x.device
        lo, scale, totals = self._on(dev)
        lens = _lengths_i32(lengths, B, dev)
        ldp = (KW + 7) // 8 * 8
        plane = counts = dense = None
        if out == "input":
            plane = torch.empty(B * T, ldp, dtype=torch.bfloat16, device=dev)
        elif out == "counts":
            counts = torch.empty(B, T, KW, dtype=torch.uint8, device=dev)
        else:
            dense = torch.empty(B, T, KW, dtype=torch.float32, device=dev)
        check(lib.sparch_spike_encode(CODES[self.code], B, T, K, ptr(x), ptr(lo), ptr(scale), ptr(state), int(fresh),
                                      int(t0), int(seed) & _M64, ptr(lens), ptr(plane), ldp, ptr(counts), ptr(dense),
                                      ptr(totals), Fn._stream()), "sparch_spike_encode")
        if out == "input":
            return Fn.input_from_plane(plane, B, T, KW)
        return counts if out == "counts" else dense

    def encode(self, x, lengths=None, out="input", seed=None):
        """x (B,T,K) features on the device -> the spikes of the whole sequences.  out="input": the network input
        (`functional.input_from_counts`'s tagged placeholder); "counts": (B,T,K') uint8; "dense": (B,T,K') fp32.
        lengths (B,): steps at or past a row's length emit nothing.  seed (rate): this call's seed; default: the
        encoder's next one."""
        x = self._checked(x)
        if seed is None:
            seed = self.next_seed() if self.code == "rate" else 0
        state = None if self.code == "rate" else torch.empty(x.shape[0], self.num_features, dtype=torch.float32, device=x.device)
        return self._run(x, lengths, out, seed, state, True, 0)


class StreamingSpikeEncoder:
    """StreamingSpikeEncoder(encoder, batch_size, seed=None): `push(chunk (B,Tc,K))` encodes a stream's next steps,
    carrying the encoder's state (B,K) and the number of steps emitted, so that the chunks of a sequence give exactly
    the spikes `encoder.encode` gives for the whole of it (rate: under the same seed).  The result feeds
    `StreamingSNN.step`; the chunks may be `StreamingFbank.push`'s frames (an empty chunk gives None)."""

    def __init__(self, encoder, batch_size, seed=None):
        if not isinstance(encoder, SpikeEncoder):
            raise ValueError("StreamingSpikeEncoder: encoder is a SpikeEncoder")
        self.encoder, self.batch_size = encoder, int(batch_size)
        if self.batch_size < 1:
            raise ValueError("StreamingSpikeEncoder: batch_size >= 1")
        self.state = None
        self.reset(seed=seed)

    def reset(self, rows=None, seed=None):
        """Restart the stream: state and step count (and, for rate, a new seed: `seed`, or the encoder's next one).
        rows: only these batch rows restart — their if integrators are emptied; the step count and the seed belong to
        the whole stream and stay.  The delta code restarts as a whole only."""
        if rows is not None:
            if self.encoder.code == "delta":
                raise ValueError("StreamingSpikeEncoder.reset: the delta code restarts the whole batch only (rows=None)")
            if self.state is not None:
                self.state[torch.as_tensor(list(rows), dtype=torch.long, device=self.state.device)] = 0.0
            return
        self.t0, self.fresh = 0, True
        self.seed = (self.encoder.next_seed() if self.encoder.code == "rate" else 0) if seed is None else int(seed)

    def push(self, chunk, out="input"):
        enc = self.encoder
        if isinstance(chunk, torch.Tensor) and chunk.ndim == 3 and chunk.shape[1] == 0:
            return None
        x = enc._checked(chunk)
        if x.shape[0] != self.batch_size:
            raise ValueError(f"StreamingSpikeEncoder.push: a ({self.batch_size}, Tc, {enc.num_features}) chunk, got "
                             f"{tuple(x.shape)}")
        if enc.code != "rate" and (self.state is None or self.state.device != x.device):
            self.state = torch.zeros(self.batch_size, enc.num_features, dtype=torch.float32, device=x.device)
            self.fresh = self.fresh or self.t0 == 0
        res = enc._run(x, None, out, self.seed, self.state, self.fresh, self.t0)
        self.t0 += x.shape[1]
        self.fresh = False
        return res
