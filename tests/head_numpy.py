"""
TEST INFRASTRUCTURE ONLY: the tail of the train step restated in plain numpy — sparch_adam_step / sparch_adam_scalars
(sparch_amd/csrc/optim.hip), sparch_ce_loss, sparch_act_fwd/_bwd and sparch_softmax_sum_fwd/_bwd
(sparch_amd/csrc/act.hip).  It shares no code with the product.  For every operation there are

  *_ref      the formula in float64, from the kernel's fp32 inputs and its fp32-ROUNDED scalars (step_size, bc2_sqrt,
             1 - beta, eps, weight_decay, 1 / (1 - p), 1 / B) taken exactly — what the kernel would give with exact
             arithmetic on the numbers it really gets;
  *_f32      the same formula in the kernel's documented operation order with every numpy operation rounded to
             float32.  It is NOT a reference: it exists to calibrate the constants below;
  *_bound    a forward-error bound per output element, c * u * (sum of the magnitudes that enter the result before
             any subtraction) + TINY, u = 2^-24.  TINY = 2^-126, the least normal fp32: below it a result has no
             relative precision (and a sigmoid of -100 is 4e-44 in fp64, 0 in fp32).

The constants c were measured against the REFERENCE, never against a kernel: the worst ratio |f32 - ref| / (u * mag)
over every input set of tests/test_head_kernels_gpu.py (the generators below), times four, rounded up.  The factor
four covers what the device does differently from numpy: its expf, logf, tanhf, sqrtf and divide may each be an ulp or
two off numpy's, and its 256-lane reduction trees hold at most 8 more additions.  tests/test_head_numpy_host.py
asserts that the restatement stays within a quarter of every bound on every input set, so no c can be set loose.

tests/test_head_numpy_host.py pins every *_ref to torch float64 without a GPU.
"""
import math

import numpy as np

from tests.dropout_numpy import keep_mask
from tests.kit import F32

U = 2.0 ** -24
TINY = 2.0 ** -126


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32)


# ====================================================================================================== Adam
# optim.hip:   g' = g + p * wd (wd != 0)          m' = m + (g' - m) * (1 - beta1)
#              v' = v * beta2 + (g' * g') * (1 - beta2)
#              d  = sqrt(v') / bc2_sqrt + eps      p' = p + (m' / d) * (-step_size)
C_ADAM_P, C_ADAM_M, C_ADAM_V = 4, 4, 24       # restatement's worst ratios 0.99, 0.99, 5.9 (calibrate()); v': 4 u |g'| G alone

ADAM_SIZES = (1, 255, 256, 257, 4095, 4096, 4097, 8192, 12289)      # ADAM_CHUNK = 4096 and 256-thread edges
ADAM_T = (1, 2, 1000, 100000)
ADAM_WD = (0.0, 0.01)
ADAM_EPS = (1e-8, 1e-3)
ADAM_GRAD_SCALES = (1e-12, 1e-6, 1.0, 1e3, 1e12)                    # element i: ADAM_GRAD_SCALES[i % 5]
ADAM_LR, ADAM_BETAS = 1e-2, (0.9, 0.999)


def adam_scalars_ref(t, lr, beta1, beta2):
    """sparch_adam_scalars in Python double: (t + 1, lr / (1 - beta1^(t+1)), sqrt(1 - beta2^(t+1)))."""
    t1 = float(t) + 1.0
    return t1, lr / (1.0 - beta1 ** t1), math.sqrt(1.0 - beta2 ** t1)


def adam_scalars32(t, lr=ADAM_LR, betas=ADAM_BETAS, eps=1e-8, weight_decay=0.0):
    """The fp32 scalars sparch_adam_step works with at step t (t >= 1), as sparch_amd.optim.Adam forms them: Python
    doubles rounded to fp32 once; 1 - beta is the KERNEL's fp32 subtraction from the rounded beta."""
    _, step_size, bc2_sqrt = adam_scalars_ref(t - 1, lr, betas[0], betas[1])
    b1, b2 = F32(betas[0]), F32(betas[1])
    return dict(step_size=F32(step_size), bc2_sqrt=F32(bc2_sqrt), beta1=b1, beta2=b2, w1=F32(1.0) - b1,
                w2=F32(1.0) - b2, eps=F32(eps), weight_decay=F32(weight_decay))


def adam_inputs(n, t, weight_decay, seed):
    """(p, g, m, v) fp32 of n elements.  Gradients at five scales side by side (element i: ADAM_GRAD_SCALES[i % 5]);
    moments zero at t = 1 and populated at the gradient's scale otherwise; every 11th element has v = m = 0, every
    13th g = 0 and every 17th |g| ~ 1e-10 (below either eps) — element 0 is all three; with weight decay every 7th
    element's g is -(wd * p) moved by a few 2^-21, so that g + wd * p cancels to a few bits."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    scale = np.asarray(ADAM_GRAD_SCALES)[i % 5]
    p = rng.standard_normal(n) * np.exp(rng.standard_normal(n))
    g = rng.standard_normal(n) * scale
    if t == 1:
        m, v = np.zeros(n), np.zeros(n)
    else:
        m = 0.5 * rng.standard_normal(n) * scale
        v = (rng.random(n) + 0.01) * scale * scale
    g[i % 17 == 0] = 1e-10 * rng.standard_normal(int((i % 17 == 0).sum()))
    g[i % 13 == 0] = 0.0
    m[i % 11 == 0] = 0.0
    v[i % 11 == 0] = 0.0
    p, g, m, v = _f32(p), _f32(g), _f32(m), _f32(v)
    if weight_decay != 0.0:
        c = (i % 7 == 3)
        wp = _f64(F32(weight_decay)) * _f64(p)
        g[c] = _f32(-wp * (1.0 + (1 + i % 8) * 2.0 ** -21))[c]
    return p, g, m, v


def adam_step_ref(p, g, m, v, s):
    """One step in float64 from fp32 state and the scalars of adam_scalars32 (or any floats): (p', m', v')."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    k = {a: float(b) for a, b in s.items()}
    if k["weight_decay"] != 0.0:
        g = g + p * k["weight_decay"]
    m1 = m + (g - m) * k["w1"]
    v1 = v * k["beta2"] + (g * g) * k["w2"]
    d = np.sqrt(v1) / k["bc2_sqrt"] + k["eps"]
    return p + (m1 / d) * (-k["step_size"]), m1, v1


def adam_step_f32(p, g, m, v, s):
    """The kernel's operation order, every operation rounded to fp32 (no fused multiply-add: -ffp-contract=off)."""
    p, g, m, v = (np.asarray(a, dtype=F32) for a in (p, g, m, v))
    k = {a: F32(b) for a, b in s.items()}
    if k["weight_decay"] != 0.0:
        g = g + p * k["weight_decay"]
    m1 = m + (g - m) * k["w1"]
    v1 = v * k["beta2"] + (g * g) * k["w2"]
    d = np.sqrt(v1) / k["bc2_sqrt"] + k["eps"]
    return p + (m1 / d) * (-k["step_size"]), m1, v1


def adam_mags(p, g, m, v, s):
    """Magnitudes behind the three bounds.  G = |g| + |wd p| is what g' is made of; with g' = g + wd p cancelled,
    g'^2 is wrong by 2 |g'| dg, dg ~ u G: the v' magnitude carries G (|g'| + u G), not g'^2.  d = sqrt(v')/bc2 + eps
    moves by dsv / bc2 with dsv = min(dv / (2 sqrt v'), sqrt(dv)) (the second where v' is about 0), and the update
    step * m' / d by step * (dm / d + |m'| dd / d^2): the sensitivities ride on the magnitude of p'."""
    _, m1, v1 = adam_step_ref(p, g, m, v, s)
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    k = {a: float(b) for a, b in s.items()}
    G = np.abs(g) + np.abs(p * k["weight_decay"])
    g1 = g + p * k["weight_decay"]
    mag_m = np.abs(m) + G
    mag_v = np.abs(v * k["beta2"]) + k["w2"] * G * (np.abs(g1) + U * G)
    sv = np.sqrt(v1)
    d = sv / k["bc2_sqrt"] + k["eps"]
    with np.errstate(divide="ignore", invalid="ignore"):
        dsv = np.where(sv > 0, np.minimum(mag_v / (2.0 * sv), np.sqrt(mag_v / U)), np.sqrt(mag_v / U))
    mag_d = dsv / k["bc2_sqrt"] + d
    upd = k["step_size"] * m1 / d
    mag_p = np.abs(p) + np.abs(upd) + k["step_size"] * (mag_m / d + np.abs(m1) * mag_d / (d * d))
    return mag_p, mag_m, mag_v


def adam_bound(p, g, m, v, s):
    mp, mm, mv = adam_mags(p, g, m, v, s)
    return C_ADAM_P * U * mp + TINY, C_ADAM_M * U * mm + TINY, C_ADAM_V * U * mv + TINY


# ====================================================================================================== cross-entropy
# act.hip ce_loss_kernel, row b:  mx = max_c x; s = sum_c expf(x - mx) (c ascending); lse = logf(s);
#   loss_b = (lse + mx) - x[y]; dlogits = (expf((x - mx) - lse) - onehot) * (1/B); a row whose label is outside
#   [0, C) adds nothing to the loss and has a zero gradient row, and the divisor stays B (include/sparch_hip.h).
#   The B row losses: thread i sums rows i, i + 256, ... in order, then a fixed 256-lane tree, times fp32(1/B).
C_CE_ROW, C_CE_MEAN, C_CE_GRAD = 6, 2, 6               # worst ratios 1.5, 0.41, 1.3

CE_SHAPES = ((1, 1), (1, 2), (255, 7), (256, 35), (257, 35), (700, 256), (64, 1000))
CE_FAMILIES = ("randn3", "randn100", "equal", "peak_on", "peak_off", "near1e4")


def ce_labels(B, C, seed):
    """Label vectors of a case: 0 and C - 1 both occur — in one vector, or for B = 1 in two."""
    rng = np.random.default_rng(seed)
    if B == 1:
        return [np.array([0], dtype=np.int64), np.array([C - 1], dtype=np.int64)][:max(1, min(C, 2))]
    y = rng.integers(0, C, B).astype(np.int64)
    y[0], y[-1] = 0, C - 1
    return [y]


def ce_logits(B, C, family, y, seed):
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((B, C))
    if family == "randn3":
        x = 3.0 * r
    elif family == "randn100":
        x = 100.0 * r                                    # most expf(x - max) underflow to zero
    elif family == "equal":
        x = np.repeat(3.0 * r[:, :1], C, axis=1)         # every logit of a row the same
    elif family in ("peak_on", "peak_off"):
        x = r.copy()
        col = y % C if family == "peak_on" else (y + 1) % C
        x[np.arange(B), col] += 80.0
    elif family == "near1e4":
        x = 1e4 * np.where(np.arange(B) % 2 == 0, 1.0, -1.0)[:, None] + r
    else:
        raise ValueError(family)
    return _f32(x)


def ce_cases():
    """Every (B, C, family, x, y) the GPU test runs."""
    for B, C in CE_SHAPES:
        for f, fam in enumerate(CE_FAMILIES):
            for j, y in enumerate(ce_labels(B, C, 100 * B + C)):
                yield B, C, fam, ce_logits(B, C, fam, y, 1000 * B + 10 * C + f), y


def _ce_parts(x, y):
    B, C = x.shape
    ok = (y >= 0) & (y < C)
    ys = np.where(ok, y, 0)
    mx = x.max(1)
    return B, C, ok, ys, mx


def ce_ref(x, y):
    """float64: dict(rows (B) — 0 where the label is out of range —, loss, dlogits (B, C), plus the pieces the
    bounds are stated in)."""
    x, y = _f64(x), np.asarray(y, dtype=np.int64)
    B, C, ok, ys, mx = _ce_parts(x, y)
    inv_b = float(F32(1.0) / F32(B))
    e = np.exp(x - mx[:, None])
    lse = np.log(e.sum(1))
    xl = x[np.arange(B), ys]
    rows = np.where(ok, (lse + mx) - xl, 0.0)
    p = np.exp((x - mx[:, None]) - lse[:, None])
    onehot = np.zeros((B, C))
    onehot[np.arange(B), ys] = 1.0
    dl = np.where(ok[:, None], (p - onehot) * inv_b, 0.0)
    return dict(rows=rows, loss=rows.sum() * inv_b, dlogits=dl, ok=ok, mx=mx, lse=lse, xl=xl, p=p, onehot=onehot,
                inv_b=inv_b)


def ce_f32(x, y):
    x, y = np.asarray(x, dtype=F32), np.asarray(y, dtype=np.int64)
    B, C, ok, ys, mx = _ce_parts(x, y)
    inv_b = F32(1.0) / F32(B)
    e = np.exp(x - mx[:, None])
    s = np.zeros(B, dtype=F32)
    for c in range(C):                                  # the kernel's class loop, in order
        s = s + e[:, c]
    lse = np.log(s)
    rows = np.where(ok, (lse + mx) - x[np.arange(B), ys], F32(0.0)).astype(F32)
    p = np.exp((x - mx[:, None]) - lse[:, None])
    onehot = np.zeros((B, C), dtype=F32)
    onehot[np.arange(B), ys] = 1.0
    dl = np.where(ok[:, None], (p - onehot) * inv_b, F32(0.0)).astype(F32)
    part = np.zeros(256, dtype=F32)
    for b0 in range(0, B, 256):                         # thread i: rows i, i + 256, ...
        chunk = rows[b0:b0 + 256]
        part[:chunk.size] = part[:chunk.size] + chunk
    o = 128
    while o > 0:                                        # the kernel's tree
        part[:o] = part[:o] + part[o:2 * o]
        o >>= 1
    return dict(rows=rows, loss=part[0] * inv_b, dlogits=dl)


def ce_bound(x, y):
    """rows: |max| + |x_label| + |lse| (what loss_b is added up from) + sqrt(C): s is a sequential fp32 sum of C
    positive terms, each with an expf and a rounded x - max behind it, whose rounding errors add as a random walk;
    d lse = ds / s.  loss: the row bounds, plus one rounding of the running sum per addition a row loss goes through —
    ceil(B/256) in its thread and 8 tree levels — on sum|loss_b|, plus the final product.  dlogits: p = exp((x-max) -
    lse) moves by p * (|x - max| + |lse| + the error of lse) roundings, then p - onehot and the product round once."""
    r = ce_ref(x, y)
    B, C = np.shape(x)
    xm = np.abs(_f64(x) - r["mx"][:, None])
    mag_row = np.where(r["ok"], np.abs(r["mx"]) + np.abs(r["xl"]) + np.abs(r["lse"]) + math.sqrt(C), 0.0)
    b_rows = C_CE_ROW * U * mag_row + TINY
    depth = (B + 255) // 256 + 8
    mag_loss = r["inv_b"] * (mag_row.sum() + depth * np.abs(r["rows"]).sum()) + abs(r["loss"])
    b_loss = C_CE_MEAN * U * mag_loss + TINY
    mag_dl = (r["p"] * (xm + np.abs(r["lse"])[:, None] + math.sqrt(C) + 1.0) + np.abs(r["p"] - r["onehot"])) * r["inv_b"]
    b_dl = np.where(r["ok"][:, None], C_CE_GRAD * U * mag_dl + TINY, 0.0)
    return dict(rows=b_rows, loss=b_loss, dlogits=b_dl)


# ====================================================================================================== activation
# act.hip act_kernel:  v = fmaf(z, scale[h], shift[h]) (common.h bn_affine: ONE rounding) or v = z;
#   a = 1 / (1 + expf(-v)) | v > 0 ? v : 0 (NaN stays NaN) | tanhf(v);   y = a * k;
#   dz = (dy * k) * act'(a),  act' = a (1 - a) | a > 0 | 1 - a a;   k = keep_mask(seed, (M, H), p)[element].
ACT_KINDS = {"sigmoid": 0, "relu": 1, "tanh": 2}          # SPARCH_ACT_*
C_ACT_FWD = {"sigmoid": 13, "relu": 6, "tanh": 7}        # worst ratios 3.2, 1.5, 1.7
C_ACT_BWD = {"sigmoid": 6, "relu": 4, "tanh": 10}        # worst ratios 1.3, 0.83, 2.3

ACT_SHAPES = ((1, 4), (37, 52), (3, 1028), (8196, 1024))  # the last: 2,098,176 float4 > the 8192 x 256 grid cap
ACT_FAMILIES = ("randn2", "saturated", "zeros")
ACT_DROPS = ((0.0, 0), (0.25, 99), (0.25, 0x1234567890ABCDEF))


def act_inputs(M, H, family, affine, seed):
    """(z, scale, shift, dy) fp32; scale = shift = None without the affine.  saturated: pre-activations in +-[20, 100];
    zeros: pre-activations that are exactly +0.0 or -0.0 in half of the elements (shift = 0 there)."""
    rng = np.random.default_rng(seed)
    sc = _f32(rng.random(H) + 0.5) if affine else None
    sh = _f32(0.3 * rng.standard_normal(H)) if affine else None
    dy = _f32(rng.standard_normal((M, H)))
    if family == "randn2":
        z = _f32(2.0 * rng.standard_normal((M, H)))
    elif family == "saturated":
        v = (20.0 + 80.0 * rng.random((M, H))) * np.where(rng.random((M, H)) < 0.5, -1.0, 1.0)
        z = _f32((v - _f64(sh)) / _f64(sc)) if affine else _f32(v)
    elif family == "zeros":
        z = _f32(rng.standard_normal((M, H)))
        pick = rng.integers(0, 4, (M, H))
        z[pick == 0] = 0.0
        z[pick == 1] = -0.0
        if affine:
            sh = np.zeros(H, dtype=F32)
    else:
        raise ValueError(family)
    return z, sc, sh, dy


def act_preact_ref(z, sc, sh):
    z = _f64(z)
    return z if sc is None else z * _f64(sc) + _f64(sh)


def _act64(kind, v):
    with np.errstate(over="ignore"):
        if kind == "sigmoid":
            return 1.0 / (1.0 + np.exp(-v))
        if kind == "relu":
            return np.maximum(v, 0.0)                       # numpy's maximum hands a NaN on, as torch.relu does
        return np.tanh(v)


def _dact64(kind, a):
    if kind == "sigmoid":
        return a * (1.0 - a)
    if kind == "relu":
        return np.where(a > 0, 1.0, 0.0)
    return 1.0 - a * a


def act_ref(kind, z, sc, sh, dy, mask=None):
    """float64 (y, dz); mask: keep_mask(seed, (M, H), p) or None."""
    v = act_preact_ref(z, sc, sh)
    k = 1.0 if mask is None else _f64(mask)
    a = _act64(kind, v)
    return a * k, (_f64(dy) * k) * _dact64(kind, a)


def act_f32(kind, z, sc, sh, dy, mask=None):
    z = np.asarray(z, dtype=F32)
    # fmaf: the product of two fp32 is exact in fp64; one fp64 addition, then ONE rounding to fp32 (the fp64 sum's own
    # rounding at 2^-53 can move that in about one case in 2^29)
    v = z if sc is None else (_f64(z) * _f64(sc) + _f64(sh)).astype(F32)
    k = F32(1.0) if mask is None else np.asarray(mask, dtype=F32)
    one = F32(1.0)
    with np.errstate(over="ignore"):
        if kind == "sigmoid":
            a = one / (one + np.exp(-v))
            df = a * (one - a)
        elif kind == "relu":
            a = np.maximum(v, F32(0.0))
            df = np.where(a > 0, one, F32(0.0))
        else:
            a = np.tanh(v)
            df = one - a * a
    return (a * k).astype(F32), ((np.asarray(dy, dtype=F32) * k) * df).astype(F32)


def act_bound(kind, z, sc, sh, dy, mask=None):
    """v has one rounding (u |v|; none without the affine, but the transcendental's argument error is of that size
    anyway).  mag_a = |a| + |act'(v)| |v|.  The backward's act' is formed from the ROUNDED a:
    a (1 - a) moves by |1 - 2a| da, 1 - a a by 2 |a| da — absolute errors of u where the true derivative has long
    underflowed (saturation) — so mag_act' = |d act'/da| mag_a + the sizes of its own operands."""
    v = act_preact_ref(z, sc, sh)
    k = 1.0 if mask is None else _f64(mask)
    a = _act64(kind, v)
    av = np.abs(v)
    if kind == "sigmoid":
        mag_a = a + a * (1.0 - a) * av
        mag_df = np.abs(1.0 - 2.0 * a) * mag_a + a * (1.0 - a) + a
    elif kind == "relu":
        mag_a = av
        mag_df = np.where(a > 0, 1.0, 0.0)
    else:
        mag_a = np.abs(a) + (1.0 - a * a) * av
        mag_df = 2.0 * np.abs(a) * mag_a + a * a + np.abs(1.0 - a * a)
    fy, fdz = act_floor(dy, mask)
    return C_ACT_FWD[kind] * U * mag_a * k + fy, C_ACT_BWD[kind] * U * np.abs(_f64(dy) * k) * mag_df + fdz


def act_floor(dy, mask=None):
    """What the bounds allow below fp32's normal range: an activation under TINY may come out as 0 (a sigmoid of -89:
    expf overflows, 1 / inf), and the outputs carry it times k and times dy k."""
    k = 1.0 if mask is None else _f64(mask)
    return TINY * np.maximum(1.0, k), TINY * np.maximum(1.0, np.abs(_f64(dy) * k))


# ====================================================================================================== softmax-sum
# act.hip softmax_sum_kernel, row (b, t): mx = max_k x; e = expf(x - mx); den = sum_k e (4 per slab in a lane, 64-lane
#   shuffle tree, 4 waves); p = e / den; forward out[b] = sum_t p_t accumulated in TIME order; backward
#   dot = sum_k p g; dx[b, t] = p (g - dot).
C_SS_FWD, C_SS_BWD = 2, 3                                 # worst ratios 0.35, 0.74

SS_SHAPES = ((1, 1, 4), (3, 17, 48), (2, 5, 1020), (2, 5, 1024), (2, 5, 1028), (1, 3, 4096), (2, 1000, 8))
SS_FAMILIES = ("randn3", "randn100", "equal_row", "peak")


def ss_inputs(B, T, K, family, seed):
    """x (B, T, K), g (B, K) fp32.  equal_row: every other (b, t) row holds one value; peak: one column 80 above."""
    rng = np.random.default_rng(seed)
    r = rng.standard_normal((B, T, K))
    if family == "randn3":
        x = 3.0 * r
    elif family == "randn100":
        x = 100.0 * r
    elif family == "equal_row":
        x = 3.0 * r
        x[:, ::2, :] = x[:, ::2, :1]
    elif family == "peak":
        x = r.copy()
        col = rng.integers(0, K, (B, T))
        np.put_along_axis(x, col[..., None], np.take_along_axis(x, col[..., None], 2) + 80.0, 2)
    else:
        raise ValueError(family)
    return _f32(x), _f32(rng.standard_normal((B, K)))


def ss_cases():
    for B, T, K in SS_SHAPES:
        for f, fam in enumerate(SS_FAMILIES):
            yield (B, T, K, fam) + ss_inputs(B, T, K, fam, 100000 * B + 100 * T + K + f)


def ss_ref(x, g):
    """float64 (out (B, K), dx (B, T, K)), the time sum in time order."""
    x, g = _f64(x), _f64(g)
    e = np.exp(x - x.max(2, keepdims=True))
    p = e / e.sum(2, keepdims=True)
    out = np.zeros((x.shape[0], x.shape[2]))
    for t in range(x.shape[1]):
        out = out + p[:, t]
    dot = (p * g[:, None, :]).sum(2, keepdims=True)
    return out, p * (g[:, None, :] - dot)


def ss_f32(x, g):
    x, g = np.asarray(x, dtype=F32), np.asarray(g, dtype=F32)
    e = np.exp(x - x.max(2, keepdims=True))
    p = e / e.sum(2, keepdims=True, dtype=F32)
    out = np.zeros((x.shape[0], x.shape[2]), dtype=F32)
    for t in range(x.shape[1]):
        out = out + p[:, t]
    dot = (p * g[:, None, :]).sum(2, keepdims=True, dtype=F32)
    return out, p * (g[:, None, :] - dot)


def ss_bound(x, g):
    """rel_p = |x - max| + depth + 2 roundings stand behind p (the rounded x - max inside expf, the den tree of depth
    4 * ceil(K/1024) + 8, expf and the divide).  out: sum_t p_t rel_p, plus one rounding per running sum of the time
    loop (sum_t acc_t).  dx: p (|g| + |dot|) (1 + rel_p) for the product and its subtraction, plus p times what dot
    is made of, sum_k p |g| (rel_p + depth)."""
    x, g = _f64(x), _f64(g)
    K = x.shape[2]
    depth = 4 * ((K + 1023) // 1024) + 8
    xm = np.abs(x - x.max(2, keepdims=True))
    e = np.exp(-xm)
    p = e / e.sum(2, keepdims=True)
    rel = xm + depth + 2.0
    ga = np.abs(g)[:, None, :]
    mag_out = (p * rel).sum(1) + np.cumsum(p, axis=1).sum(1)
    dot = (p * g[:, None, :]).sum(2, keepdims=True)
    mag_dot = (p * ga * (rel + depth)).sum(2, keepdims=True)
    mag_dx = p * (ga + np.abs(dot)) * (1.0 + rel) + p * mag_dot
    return C_SS_FWD * U * mag_out + TINY, C_SS_BWD * U * mag_dx + TINY


# ====================================================================================================== calibration
def worst(got, ref, mag, floor=TINY):
    """max |got - ref| / (u mag) over the elements where mag > 0 (the figure a constant c is four times of)."""
    with np.errstate(invalid="ignore"):
        err = np.maximum(np.abs(_f64(got) - _f64(ref)) - floor, 0.0)     # (what the floor allows is no rounding error)
    assert not np.isnan(err).any()
    mag = np.broadcast_to(_f64(mag), err.shape)
    sel = mag > 0
    return float((err[sel] / (U * mag[sel])).max()) if sel.any() else 0.0


def adam_table(t, weight_decay, seed=0):
    """The flat state of one Adam case and its split into the ADAM_SIZES tensors."""
    n = sum(ADAM_SIZES)
    p, g, m, v = adam_inputs(n, t, weight_decay, 7919 * t + int(weight_decay * 1000) + seed)
    cuts = np.cumsum(ADAM_SIZES)[:-1]
    return (p, g, m, v), [np.split(a, cuts) for a in (p, g, m, v)]


def adam_cases():
    for t in ADAM_T:
        for wd in ADAM_WD:
            for eps in ADAM_EPS:
                yield t, wd, eps


def act_cases(shapes=ACT_SHAPES):
    """Every (kind, M, H, family, affine, z, scale, shift, dy) of the GPU test; the large shape runs randn2 only."""
    for kind in ACT_KINDS:
        for M, H in shapes:
            for f, fam in enumerate(ACT_FAMILIES if M * H < (1 << 20) else ACT_FAMILIES[:1]):
                for affine in (True, False):
                    yield (kind, M, H, fam, affine) + act_inputs(M, H, fam, affine, 100 * M + H + 10 * f + int(affine))


def calibrate():
    """Worst ratios of the fp32 restatements against the fp64 references on every input set (python -m
    tests.head_numpy prints them): the constants above are ceil(4 x) of these."""
    w = {}

    def put(k, val):
        w[k] = max(w.get(k, 0.0), val)

    for t, wd, eps in adam_cases():
        (p, g, m, v), _ = adam_table(t, wd)
        s = adam_scalars32(t, eps=eps, weight_decay=wd)
        for name, a, b, mag in zip(("adam_p", "adam_m", "adam_v"), adam_step_f32(p, g, m, v, s),
                                   adam_step_ref(p, g, m, v, s), adam_mags(p, g, m, v, s)):
            put(name, worst(a, b, mag))
    for B, C, fam, x, y in ce_cases():
        r, f, b = ce_ref(x, y), ce_f32(x, y), ce_bound(x, y)
        put("ce_rows", worst(f["rows"], r["rows"], (b["rows"] - TINY) / (C_CE_ROW * U)))
        put("ce_grad", worst(f["dlogits"], r["dlogits"], (b["dlogits"] - TINY) / (C_CE_GRAD * U)))
        put("ce_loss", worst(f["loss"], r["loss"], (b["loss"] - TINY) / (C_CE_MEAN * U)))
    for kind, M, H, fam, affine, z, sc, sh, dy in act_cases():
        for p_drop, seed in ACT_DROPS[:2]:
            mask = keep_mask(seed, (M, H), p_drop) if p_drop else None
            (y, dz), (ry, rdz) = act_f32(kind, z, sc, sh, dy, mask), act_ref(kind, z, sc, sh, dy, mask)
            by, bdz = act_bound(kind, z, sc, sh, dy, mask)
            fy, fdz = act_floor(dy, mask)
            put(f"act_fwd_{kind}", worst(y, ry, (by - fy) / (C_ACT_FWD[kind] * U), fy))
            put(f"act_bwd_{kind}", worst(dz, rdz, (bdz - fdz) / (C_ACT_BWD[kind] * U), fdz))
    for B, T, K, fam, x, g in ss_cases():
        (o, dx), (ro, rdx), (bo, bdx) = ss_f32(x, g), ss_ref(x, g), ss_bound(x, g)
        put("ss_fwd", worst(o, ro, (bo - TINY) / (C_SS_FWD * U)))
        put("ss_bwd", worst(dx, rdx, (bdx - TINY) / (C_SS_BWD * U)))
    return w


if __name__ == "__main__":
    for k_, v_ in sorted(calibrate().items()):
        print(f"{k_:28s} {v_:.4f}   x4 -> {math.ceil(4 * v_)}")
