"""
Augmentation of SHD / SSC events on the device (not in the reference, which augments HD / SC audio only).

Three per-sample transforms of an event list, the ones published SHD results above the reference's rely on:
a channel shift, a time stretch with an offset, and dropping — single events at random, one window of time, one band
of channels.  They are applied inside the gather-and-bin kernel of the resident store
(`sparch_events_gather_bin_aug`, include/sparch_hip.h), which reads every event of a batch once anyway; the host
only draws one row of `EVAUG_FIELDS` numbers per sample.  This module is that host side: the spec's parser and the
draws.  It needs numpy only.

Spec: `shift=40,scale=0.2,offset=0.1,drop=0.1,tmask=0.15,umask=70` — any subset, a missing key leaves its
transform off.

    shift   units    d ~ integers [-shift, shift]             every unit of the sample moves by d
    scale   -        a ~ uniform [1 - scale, 1 + scale]       t' = a * t + c  (scale < 1: a stays positive)
    offset  seconds  c ~ uniform [-offset, offset]
    drop    -        p = drop                                 every event is removed with probability p
    tmask   seconds  width ~ uniform [0, tmask], start ~ uniform [0, max_time - width]     events of the window go
    umask   units    width ~ integers [0, umask], start ~ integers [0, nb_units - width]   events of the band go

Table row (float32): d, a, c, p, m0, m1, k0, k1 with the window [m0, m1) in transformed seconds and the band
[k0, k1) in shifted units.  The identity row is (0, 1, 0, 0, 0, 0, 0, 0).

ORDER OF THE DRAWS (fixed: a run is reproducible from the generator's state).  One vectorised draw of n values per
line, in this order, a line skipped when its transform is off:
    1. d            (shift)
    2. a            (scale)
    3. c            (offset)
    4. mask width, then 5. mask start      (tmask)
    6. band width, then 7. band start      (umask)
    8. the seed of the kernel's drop draws, one integer in [0, 2^63): always drawn, last.
`drop` draws nothing on the host.  The generator is a numpy Generator; torch's global generator is never touched, so
the network's initial-state draws are the same with augmentation on or off.
"""
import math

import numpy as np

EVAUG_FIELDS = 8  # SPARCH_EVAUG_FIELDS
_KEYS = ("shift", "scale", "offset", "drop", "tmask", "umask")
_INT_KEYS = ("shift", "umask")


def parse_event_augment(text):
    """The spec as a dict with every key of `_KEYS` (0 = off; shift and umask ints, the others floats).  ValueError
    for an unknown or repeated key, a value that is not a finite non-negative number (a whole one for shift and
    umask, shift <= 65535), scale >= 1 or drop >= 1."""
    spec = {k: (0 if k in _INT_KEYS else 0.0) for k in _KEYS}
    if isinstance(text, dict):
        items = list(text.items())
    else:
        items = []
        for part in str(text).split(","):
            if not part.strip():
                continue
            key, eq, value = part.partition("=")
            if not eq:
                raise ValueError(f"event augmentation '{text}': '{part}' is not key=value")
            items.append((key.strip(), value.strip()))
    seen = set()
    for key, value in items:
        if key not in _KEYS:
            raise ValueError(f"event augmentation '{text}': unknown key '{key}' (known: {', '.join(_KEYS)})")
        if key in seen:
            raise ValueError(f"event augmentation '{text}': key '{key}' is given twice")
        seen.add(key)
        try:
            v = int(value) if key in _INT_KEYS and not isinstance(value, float) else float(value)
        except (TypeError, ValueError):
            raise ValueError(f"event augmentation '{text}': {key}={value} is not "
                             f"{'a whole number' if key in _INT_KEYS else 'a number'}") from None
        if not math.isfinite(v) or v < 0 or (key in _INT_KEYS and v != int(v)):
            raise ValueError(f"event augmentation '{text}': {key}={value} must be a finite non-negative "
                             f"{'whole ' if key in _INT_KEYS else ''}number")
        spec[key] = int(v) if key in _INT_KEYS else v
    if spec["scale"] >= 1:
        raise ValueError(f"event augmentation '{text}': scale must be below 1 (the time scale stays positive)")
    if spec["drop"] >= 1:
        raise ValueError(f"event augmentation '{text}': drop must be below 1")
    if spec["shift"] > 65535:
        raise ValueError(f"event augmentation '{text}': shift must be at most 65535 (units are stored in 16 bits)")
    return spec


def identity_rows(n):
    """(n, EVAUG_FIELDS) float32 rows that change nothing."""
    table = np.zeros((n, EVAUG_FIELDS), np.float32)
    table[:, 1] = 1.0
    return table


def draw_event_augmentation(n, spec, rng, nb_units=700, max_time=1.4):
    """((n, EVAUG_FIELDS) float32 table, seed) for n samples, drawn from the numpy Generator `rng` in the order the
    module's docstring fixes.  `spec`: a parsed spec or its text."""
    if not isinstance(spec, dict) or set(spec) != set(_KEYS):
        spec = parse_event_augment(spec)
    table = identity_rows(n)
    if spec["shift"]:
        table[:, 0] = rng.integers(-spec["shift"], spec["shift"], n, endpoint=True)
    if spec["scale"]:
        table[:, 1] = rng.uniform(1.0 - spec["scale"], 1.0 + spec["scale"], n)
    if spec["offset"]:
        table[:, 2] = rng.uniform(-spec["offset"], spec["offset"], n)
    table[:, 3] = spec["drop"]
    if spec["tmask"]:
        width = rng.uniform(0.0, min(spec["tmask"], max_time), n)
        start = rng.uniform(0.0, max_time - width)
        table[:, 4], table[:, 5] = start, start + width
    if spec["umask"]:
        width = rng.integers(0, min(spec["umask"], nb_units), n, endpoint=True)
        start = rng.integers(0, nb_units - width, endpoint=True)
        table[:, 6], table[:, 7] = start, start + width
    seed = int(rng.integers(0, 2 ** 63))
    return table, seed


def check_event_augmentation(table, n=None, what="EventStore"):
    """The table as a contiguous (n, EVAUG_FIELDS) float32 array, ValueError unless the kernel's contract holds:
    shape, every value finite, a > 0, 0 <= p < 1, shift and band edges whole numbers, |shift| <= 65535."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != EVAUG_FIELDS or (n is not None and t.shape[0] != n):
        raise ValueError(f"{what}: the augmentation table must have shape ({'n' if n is None else n}, "
                         f"{EVAUG_FIELDS}), found {tuple(t.shape)}")
    if t.dtype.kind not in "fiu":
        raise ValueError(f"{what}: the augmentation table must be numeric, found {t.dtype}")
    t = np.ascontiguousarray(t, np.float32)
    if not np.isfinite(t).all():
        raise ValueError(f"{what}: the augmentation table holds a value that is not finite")
    if not (t[:, 1] > 0).all():
        raise ValueError(f"{what}: a time scale (field 1) is not positive")
    if not ((t[:, 3] >= 0) & (t[:, 3] < 1)).all():
        raise ValueError(f"{what}: a drop probability (field 3) is outside [0, 1)")
    if (t[:, [0, 6, 7]] != np.rint(t[:, [0, 6, 7]])).any():
        raise ValueError(f"{what}: unit shift and unit band (fields 0, 6, 7) must be whole numbers")
    if (np.abs(t[:, 0]) > 65535).any():
        raise ValueError(f"{what}: a unit shift (field 0) is beyond +-65535")
    return t


def plane_count_factor(scale):
    """By how much time compression can raise the largest bin count: a bin of t' = a * t + c covers at most
    ceil(1 / a) + 1 bins of t, a >= 1 - scale, plus one for the rounding of the edges."""
    if not 0 <= scale < 1:
        raise ValueError(f"scale bound {scale} outside [0, 1)")
    return math.ceil(1.0 / (1.0 - scale)) + 2
