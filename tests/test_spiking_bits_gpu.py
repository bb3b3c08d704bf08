"""
The spiking FORWARD kernels, to the bit: a SHA-256 of every output of cell_fwd_pipe_kernel, rec_fwd_kernel,
readout_fwd_kernel (sparch_amd/csrc/cell.hip, reccell.hip) and of the fused streaming steps (streamstep.hip,
streamsparse.hip) against tests/golden/spiking_bits.json.

A stream may take a step through the chunk kernels, the dense fused kernel or the event-driven one, and switches between
them mid-stream: the membrane step must be the same expression tree everywhere (csrc/neuron.h).  The fp64 tests have
tolerances and pass a regrouped sum or a fused multiply-add; the dyadic fixtures are exact in any grouping.  Here the
inputs are REAL-valued, so every rounding of the tree shows: standard-normal projections, V ~ N(0, 0.5^2), theta 0.25,
alpha in [0.90, 0.96], beta / a / b inside their clamp ranges, and neuron 0 of every parameter below its range, neuron 1
above it (the clamps are exercised); u0 and a real-valued s0 uniform in [0, 0.5), w0 in [0, 0.1) (larger initial
states end in a burst at the first step and a silent population behind it: under 1 % spikes at the last step).

The file was recorded with the build of the commit BEFORE the kernels were rewritten on the shared helpers of neuron.h /
stream_common.h, twice in one visit with byte-identical results, never from the code under test.  Re-record it
(this module run with python -m, > the file, on the last commit whose bits are trusted) only for a new toolchain
or a deliberate change of arithmetic, and say which in the commit message.  A differing "inputs" hash means that the
host-side numpy inputs moved, not a kernel.  So that a hash cannot hide a dead case, every hashed spike tensor must hold
between 1 % and 50 % non-zeros: asserted here, and checked beforehand on the CPU with tests/spiking_numpy.py and
tests/sparse_numpy.py (a seed that fails it gets another one through SALT; the bounds stay).

Cases (B = 33: two row tiles, the second ragged; T = 6):
  whole   functional.cell_forward.  LIF / adLIF at H = 96, at H = 3 and at H = 15888; RLIF / RadLIF at H = 96, 132, 384,
          1024 (the KGW / NW instantiations).  cell.hip's dispatcher takes the VEC = 4 scan kernel only where
          B * dirs * H >= 2^19 and H % 4 == 0, so at B = 33 BOTH H = 96 and an H that is no multiple of 4 run the
          VEC = 1 kernel; H = 3 is the smallest width that holds an in-range neuron beside the two out-of-range ones,
          and H = 15888 is the smallest multiple of 4 that reaches VEC = 4.  Two directions with p_drop = 0.25 at the
          smallest and the largest H of a kind, one direction without dropout elsewhere; scale / shift on the adaptive
          kinds; bf16 saved states once per kind; the bf16 operand mode (NP = 1) and the launch-per-step path (EXT) once
          per recurrent kind.
  chunks  the streaming entry points (STATE / STREAM instantiations) at H = 96: chunks of 1, 4 and 1 steps on one
          carried state; the recurrent kinds through the persistent kernel and through the launch-per-step one.
  readout sparch_readout_fwd / sparch_readout_stream_fwd at C = 35, T = 11 (one unrolled group of 8 steps and a ragged
          tail of 3), with and without the affine.
  fused   sparch_stream_step_fwd / _sparse_fwd, all kinds, B = 1, 5, 33 (row tiles 1, 8, and 16 with a ragged second
          tile), H = 132, K = 130 (scalar weight loads) and 200 (16-byte loads), three consecutive steps, with bias and
          affine and with neither; a uint8 input once; the two readout steps at C = 35, K = 130 and 132.
"""
import contextlib
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

from tests import spiking_numpy as sn
from tests.kit import DEV, F32, D, raw, sha
from tests.kit import Fn as _Fn

pytestmark = pytest.mark.gpu

BITS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spiking_bits.json")
B, T, THETA = 33, 6, 0.25
KIND = {"LIF": 0, "adLIF": 1, "RLIF": 2, "RadLIF": 3}
SALT = {}       # case id -> another seed, where the first one left a spike tensor outside 1 .. 50 %


def sha_inputs(c):
    flat = []
    for k in sorted(c):
        v = c[k]
        if isinstance(v, dict):
            flat += [v[j] for j in sorted(v)]
        elif isinstance(v, np.ndarray):
            flat.append(v)
    return sha(*flat)


def rng_of(case_id):
    return np.random.default_rng(zlib.crc32(case_id.encode()) + SALT.get(case_id, 0))


def neuron_params(kind, H, rng, alpha_only=False):
    p = {"alpha": rng.uniform(0.90, 0.96, H).astype(F32)}
    if sn.ADAPTIVE.get(kind) and not alpha_only:
        p.update(beta=rng.uniform(0.968, 0.991, H).astype(F32), a=rng.uniform(-0.9, 0.9, H).astype(F32),
                 b=rng.uniform(0.1, 1.9, H).astype(F32))
    for k in p:
        p[k][0], p[k][1] = sn.OUTSIDE[k]
    if sn.RECURRENT.get(kind) and not alpha_only:
        p["V"] = (0.5 * rng.standard_normal((H, H))).astype(F32)
    return p


def spike_fraction_ok(frac, what):
    assert 0.01 <= frac <= 0.5, f"{what}: {frac:.4f} of the spike tensor is non-zero (a dead or saturated case)"


# ====================================================================================================== whole sequence
def _whole_cases():
    cases = {}
    for kinds, widths in ((("LIF", "adLIF"), (3, 96, 15888)), (("RLIF", "RadLIF"), (96, 132, 384, 1024))):
        for kind in kinds:
            for H in widths:
                two = H in (widths[0], widths[-1])
                cases[f"whole-{kind}-H{H}"] = (kind, H, 2 if two else 1, 0.25 if two else 0.0, "plain")
            cases[f"whole-{kind}-H96-save16"] = (kind, 96, 1, 0.0, "save16")
            if sn.RECURRENT[kind]:
                cases[f"whole-{kind}-H132-bf16"] = (kind, 132, 1, 0.0, "bf16")
                cases[f"whole-{kind}-H96-ext"] = (kind, 96, 1, 0.0, "ext")
    return cases


WHOLE = _whole_cases()


@functools.lru_cache(maxsize=2)
def whole_inputs(case_id):
    kind, H, dirs, _, _ = WHOLE.get(case_id) or CHUNKS[case_id]
    rng = rng_of(case_id)
    Bp = B * dirs
    c = {"p": neuron_params(kind, H, rng), "Wx": rng.standard_normal((B, T, H)).astype(F32),
         "u0": rng.uniform(0, 0.5, (Bp, H)).astype(F32), "s0": rng.uniform(0, 0.5, (Bp, H)).astype(F32)}
    if sn.ADAPTIVE[kind]:
        c.update(w0=rng.uniform(0, 0.1, (Bp, H)).astype(F32), scale=rng.uniform(0.7, 1.3, H).astype(F32),
                 shift=rng.uniform(0, 0.4, H).astype(F32))
    return c


@contextlib.contextmanager
def mode_of(mode):
    Fn = _Fn()
    save, dtype, env = Fn.SAVE_BF16, Fn.compute_dtype(), os.environ.get("SPARCH_REC_STEP_PATH")
    try:
        Fn.SAVE_BF16 = mode == "save16"
        Fn.set_compute_dtype("bf16" if mode == "bf16" else "fp32")
        if mode == "ext":
            os.environ["SPARCH_REC_STEP_PATH"] = "1"
        else:
            os.environ.pop("SPARCH_REC_STEP_PATH", None)
        yield Fn
    finally:
        Fn.SAVE_BF16 = save
        Fn.set_compute_dtype(dtype)
        os.environ.pop("SPARCH_REC_STEP_PATH", None)
        if env is not None:
            os.environ["SPARCH_REC_STEP_PATH"] = env


def whole_bits(case_id):
    kind, H, dirs, p_drop, mode = WHOLE[case_id]
    c = whole_inputs(case_id)
    with mode_of(mode) as Fn:
        assert not sn.RECURRENT[kind] or Fn.rec_step_path(H) == (mode == "ext")
        s_out, count, saved, s16 = Fn.cell_forward(kind, D(c["Wx"]), D(c.get("scale")), D(c.get("shift")),
                                                   {k: D(v) for k, v in c["p"].items()}, D(c["u0"]), D(c.get("w0")),
                                                   D(c["s0"]), B=B, dirs=dirs, theta=THETA, p_drop=p_drop, seed=20240229)
        Fn.check_status()
        torch.cuda.synchronize()
    assert (saved[0].dtype == torch.bfloat16) == (mode == "save16")
    bits = {"inputs": sha_inputs(c), "s_out": sha(raw(s_out)), "s16": sha(raw(s16)), "u_save": sha(raw(saved[0])),
            "count": sha(raw(count))}
    if sn.ADAPTIVE[kind]:
        bits["w_save"] = sha(raw(saved[1]))
    return bits, {"s_out": float((raw(s_out) != 0).mean()), "s16": float((raw(s16) != 0).mean())}


# ====================================================================================================== streaming chunks
CHUNKS = {f"chunks-{kind}-{how}": (kind, 96, 1, 0.0, how) for kind in sn.KINDS
          for how in (("persistent", "steps") if sn.RECURRENT[kind] else ("scan",))}
CHUNK_STEPS = (1, 4, 1)


def chunk_bits(case_id):
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    kind, H, _, _, how = CHUNKS[case_id]
    c = whole_inputs(case_id)
    k, st = KIND[kind], Fn._stream()
    p = {j: D(v) for j, v in c["p"].items()}
    scale, shift = D(c.get("scale")), D(c.get("shift"))
    u, w, s = D(c["u0"]), D(c.get("w0")), D(c["s0"])
    count = torch.zeros(H, dtype=torch.int32, device=DEV)
    if sn.RECURRENT[kind]:
        vmask = torch.empty(H, H, dtype=torch.float32, device=DEV)
        vpack = Fn._vpack(H, p["V"], 0, vmask=vmask)
        vmask_t = vmask.t().contiguous()
        s16_state, binary = torch.zeros(B, H, dtype=torch.bfloat16, device=DEV), False

        def drive():
            if binary:
                return Fn.gemm_nt(Fn.spike_placeholder(1, B, H, DEV).view(B, H), vmask_t, spike_scale=1.0, a16=s16_state)[0]
            return Fn.gemm_nn(s, vmask) if how == "steps" else Fn._gemm_small(s, vmask, nn=True)
    outs, outs16, t0 = [], [], 0
    for Tc in CHUNK_STEPS:
        Wx = D(c["Wx"][:, t0:t0 + Tc])
        t0 += Tc
        s_out = torch.empty(B, Tc, H, dtype=torch.float32, device=DEV)
        s16 = torch.empty(B, Tc, H, dtype=torch.bfloat16, device=DEV)
        if how == "scan":
            check(lib.sparch_cell_stream_fwd(k, B, 1, Tc, H, ptr(Wx), ptr(scale), ptr(shift), ptr(p["alpha"]),
                                             ptr(p.get("beta")), ptr(p.get("a")), ptr(p.get("b")), ptr(u), ptr(w), ptr(s),
                                             THETA, 0.0, ptr(s_out), ptr(s16), ptr(count), st), "sparch_cell_stream_fwd")
        elif how == "steps":
            for t in range(Tc):
                rec = drive()
                check(lib.sparch_rec_cell_step_stream_fwd(k, B, 1, Tc, H, t, ptr(Wx), ptr(scale), ptr(shift), ptr(p["alpha"]),
                                                          ptr(p.get("beta")), ptr(p.get("a")), ptr(p.get("b")), ptr(rec), ptr(u),
                                                          ptr(w), ptr(s), ptr(s16_state), THETA, 0.0, ptr(s_out), ptr(s16),
                                                          ptr(count), st), "sparch_rec_cell_step_stream_fwd")
                binary = True
        else:
            rec0 = drive()
            Fn._persistent(None, "sparch_rec_cell_stream_fwd",
                           (k, B, 1, Tc, H, ptr(Wx), ptr(scale), ptr(shift), ptr(p["alpha"]), ptr(p.get("beta")),
                            ptr(p.get("a")), ptr(p.get("b")), ptr(vpack), ptr(rec0), ptr(u), ptr(w), ptr(s), ptr(s16_state),
                            THETA, 0.0, ptr(s_out), ptr(s16), ptr(count)),
                           lib.sparch_rec_chan_bytes(B, Tc, H), torch.device(DEV), Fn.rec_steps_per_launch(Tc), Fn._prec())
            binary = True
        outs.append(raw(s_out))
        outs16.append(raw(s16))
    Fn.check_status()
    torch.cuda.synchronize()
    s_all, s16_all = np.concatenate(outs, axis=1), np.concatenate(outs16, axis=1)
    bits = {"inputs": sha_inputs(c), "s_out": sha(s_all), "s16": sha(s16_all), "u": sha(raw(u)), "s": sha(raw(s)),
            "count": sha(raw(count))}
    if sn.ADAPTIVE[kind]:
        bits["w"] = sha(raw(w))
    if sn.RECURRENT[kind]:
        bits["s16_state"] = sha(raw(s16_state))
    return bits, {"s_out": float((s_all != 0).mean()), "s16": float((s16_all != 0).mean()), "s": float((raw(s) != 0).mean())}


# ====================================================================================================== readout
RO_C, RO_T = 35, 11
READOUT = {f"readout-{'affine' if aff else 'plain'}": aff for aff in (False, True)}


@functools.lru_cache(maxsize=2)
def readout_inputs(case_id):
    rng = rng_of(case_id)
    c = {"p": neuron_params(None, RO_C, rng, alpha_only=True), "Wx": rng.standard_normal((B, RO_T, RO_C)).astype(F32),
         "u0": rng.uniform(0, 1, (B, RO_C)).astype(F32)}
    if READOUT[case_id]:
        c.update(scale=rng.uniform(0.7, 1.3, RO_C).astype(F32), shift=rng.uniform(-0.2, 0.2, RO_C).astype(F32))
    return c


def readout_bits(case_id):
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    c = readout_inputs(case_id)
    Wx, scale, shift, alpha = D(c["Wx"]), D(c.get("scale")), D(c.get("shift")), D(c["p"]["alpha"])
    out = torch.empty(B, RO_C, dtype=torch.float32, device=DEV)
    u_save = torch.empty(B, RO_T, RO_C, dtype=torch.float32, device=DEV)
    check(lib.sparch_readout_fwd(B, RO_T, RO_C, ptr(Wx), ptr(scale), ptr(shift), ptr(alpha), ptr(D(c["u0"])), ptr(out),
                                 ptr(u_save), Fn._stream()), "sparch_readout_fwd")
    u, acc = D(c["u0"]), torch.zeros(B, RO_C, dtype=torch.float32, device=DEV)
    check(lib.sparch_readout_stream_fwd(B, RO_T, RO_C, ptr(Wx), ptr(scale), ptr(shift), ptr(alpha), ptr(u), ptr(acc),
                                        Fn._stream()), "sparch_readout_stream_fwd")
    Fn.check_status()
    torch.cuda.synchronize()
    assert abs(float(out.sum()) - B * RO_T) <= 1e-3 * B * RO_T
    return {"inputs": sha_inputs(c), "out": sha(raw(out)), "u_save": sha(raw(u_save)), "stream.out": sha(raw(acc)),
            "stream.u": sha(raw(u))}, {}


# ====================================================================================================== fused steps
FUSED_H, FUSED_STEPS = 132, 3
FUSED = {f"fused-{kind}-B{Bn}-K{K}": (kind, Bn, K, False) for kind in sn.KINDS for Bn in (1, 5, 33) for K in (130, 200)}
FUSED["fused-RadLIF-B5-K200-uint8"] = ("RadLIF", 5, 200, True)
FUSED_RO = {f"fused-readout-K{K}": K for K in (130, 132)}


@functools.lru_cache(maxsize=2)
def fused_inputs(case_id):
    """The inputs of a hidden layer's fused step (W scaled so that x W^T is about standard normal), or of the readout's."""
    rng = rng_of(case_id)
    if case_id in FUSED_RO:
        kind, Bn, K, u8, H = None, B, FUSED_RO[case_id], False, RO_C
    else:
        (kind, Bn, K, u8), H = FUSED[case_id], FUSED_H
    on = rng.uniform(0, 1, (FUSED_STEPS, Bn, K)) < 0.3
    if u8:
        x = (on * rng.integers(1, 4, on.shape)).astype(np.uint8)
    else:
        x = (on * rng.uniform(0.5, 1.5, on.shape)).astype(F32)
    c = {"p": neuron_params(kind, H, rng, alpha_only=kind is None), "x": x,
         "W": (rng.standard_normal((H, K)) / np.sqrt(0.3 * K * float(np.mean(x[on].astype(np.float64) ** 2)))).astype(F32),
         "bias": (0.3 * rng.standard_normal(H)).astype(F32), "scale": rng.uniform(0.7, 1.3, H).astype(F32),
         "shift": rng.uniform(0, 0.4, H).astype(F32), "u0": rng.uniform(0, 0.5, (Bn, H)).astype(F32)}
    if kind is not None:
        c["s0"] = rng.uniform(0, 0.5, (Bn, H)).astype(F32)
        if sn.ADAPTIVE[kind]:
            c["w0"] = rng.uniform(0, 0.1, (Bn, H)).astype(F32)
        if sn.RECURRENT[kind]:
            c["Vm"] = c["p"].pop("V")
            np.fill_diagonal(c["Vm"], 0)
    return c


def padded_t(W):
    """W (N,K) -> W^T (K, N rounded up to a multiple of 4): the event-driven step's weight operand."""
    N = W.shape[0]
    return np.pad(W.T, ((0, 0), (0, (N + 3) // 4 * 4 - N)))


def fused_bits(case_id):
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    kind, Bn, K, u8 = FUSED[case_id]
    H, c, k, st = FUSED_H, fused_inputs(case_id), KIND[kind], Fn._stream()
    adaptive, recurrent = sn.ADAPTIVE[kind], sn.RECURRENT[kind]
    p = {j: D(v) for j, v in c["p"].items()}
    x, W, Wt = D(c["x"]), D(c["W"]), D(padded_t(c["W"]))
    Vm, VmT = (D(c["Vm"]), D(c["Vm"].T)) if recurrent else (None, None)
    bits, fracs = {"inputs": sha_inputs(c)}, {}
    for form in ("dense", "sparse"):
        for with_affine in (True, False):
            bias, scale, shift = (D(c["bias"]), D(c["scale"]), D(c["shift"])) if with_affine else (None, None, None)
            u, w, s_in = D(c["u0"]), D(c.get("w0")), D(c["s0"])
            s_out = torch.zeros_like(s_in)
            s16 = torch.zeros(Bn, H, dtype=torch.bfloat16, device=DEV)
            count = torch.zeros(H, dtype=torch.int32, device=DEV)
            got = {j: [] for j in ("u", "w", "s", "s16")}
            for t in range(FUSED_STEPS):
                if form == "dense":
                    check(lib.sparch_stream_step_fwd(k, Bn, K, H, H, int(u8), ptr(x[t]), K, ptr(W), ptr(bias), ptr(scale),
                                                     ptr(shift), ptr(p["alpha"]), ptr(p.get("beta")), ptr(p.get("a")),
                                                     ptr(p.get("b")), ptr(VmT), ptr(u), ptr(w), ptr(s_in), ptr(s_out),
                                                     ptr(s16), THETA, ptr(count), st), "sparch_stream_step_fwd")
                else:
                    check(lib.sparch_stream_step_sparse_fwd(k, Bn, K, H, H, int(u8), ptr(x[t]), K, ptr(Wt), Wt.shape[1],
                                                            ptr(bias), ptr(scale), ptr(shift), ptr(p["alpha"]),
                                                            ptr(p.get("beta")), ptr(p.get("a")), ptr(p.get("b")), ptr(Vm),
                                                            ptr(u), ptr(w), ptr(s_in), ptr(s_out), ptr(s16), THETA,
                                                            ptr(count), st), "sparch_stream_step_sparse_fwd")
                got["u"].append(raw(u))
                got["s"].append(raw(s_out))
                got["s16"].append(raw(s16))
                if adaptive:
                    got["w"].append(raw(w))
                s_in, s_out = s_out, s_in
            Fn.check_status()
            name = f"{form}.{'affine' if with_affine else 'plain'}"
            for j, v in got.items():
                if v:
                    bits[f"{name}.{j}"] = sha(*v)
            bits[f"{name}.count"] = sha(raw(count))
            fracs[f"{name}.s"] = float(np.mean([(a != 0).mean() for a in got["s"]]))
            fracs[f"{name}.s16"] = float(np.mean([(a != 0).mean() for a in got["s16"]]))
    return bits, fracs


def fused_readout_bits(case_id):
    from sparch_amd._capi import check, lib, ptr
    Fn = _Fn()
    K, C, c, st = FUSED_RO[case_id], RO_C, fused_inputs(case_id), Fn._stream()
    x, W, Wt, alpha = D(c["x"]), D(c["W"]), D(padded_t(c["W"])), D(c["p"]["alpha"])
    bits = {"inputs": sha_inputs(c)}
    for form in ("dense", "sparse"):
        for with_affine in (True, False):
            bias, scale, shift = (D(c["bias"]), D(c["scale"]), D(c["shift"])) if with_affine else (None, None, None)
            u, out = D(c["u0"]), torch.zeros(B, C, dtype=torch.float32, device=DEV)
            us = []
            for t in range(FUSED_STEPS):
                if form == "dense":
                    check(lib.sparch_stream_step_readout(B, K, C, ptr(x[t]), K, ptr(W), ptr(bias), ptr(scale), ptr(shift),
                                                         ptr(alpha), ptr(u), ptr(out), st), "sparch_stream_step_readout")
                else:
                    check(lib.sparch_stream_step_sparse_readout(B, K, C, ptr(x[t]), K, ptr(Wt), Wt.shape[1], ptr(bias),
                                                                ptr(scale), ptr(shift), ptr(alpha), ptr(u), ptr(out), st),
                          "sparch_stream_step_sparse_readout")
                us.append(raw(u))
            Fn.check_status()
            assert abs(float(out.sum()) - B * FUSED_STEPS) <= 1e-3 * B * FUSED_STEPS
            name = f"{form}.{'affine' if with_affine else 'plain'}"
            bits[f"{name}.u"], bits[f"{name}.out"] = sha(*us), sha(raw(out))
    return bits, {}


# ====================================================================================================== the test
FAMILIES = ((WHOLE, whole_bits), (CHUNKS, chunk_bits), (READOUT, readout_bits), (FUSED, fused_bits),
            (FUSED_RO, fused_readout_bits))
CASES = {case_id: fn for cases, fn in FAMILIES for case_id in cases}


@functools.lru_cache(maxsize=1)
def recorded_bits():
    with open(BITS_FILE) as f:
        return json.load(f)["bits"]


@pytest.mark.parametrize("case_id", list(CASES))
def test_spiking_forward_outputs_have_the_recorded_bits(case_id):
    """See the module docstring: recorded on the commit before the kernels moved onto neuron.h / stream_common.h, never
    from the code under test.  Re-record (this module run with python -m, > tests/golden/spiking_bits.json, on the
    last commit whose bits are trusted) only for a new toolchain or a deliberate change of arithmetic, and say which in
    the commit message.  A differing "inputs" hash means that the numpy inputs moved, not a kernel."""
    want = recorded_bits()[case_id]
    got, fracs = CASES[case_id](case_id)
    print(f"  {case_id}: spike fractions {fracs}")
    assert got["inputs"] == want["inputs"], "the numpy inputs differ from the recorded ones (not a kernel's doing)"
    for what, frac in fracs.items():
        spike_fraction_ok(frac, f"{case_id} {what}")
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(got) if got[k] != want[k]]
    assert not differ, f"{case_id}: other bits than recorded in {differ}"


if __name__ == "__main__":
    bits = {}
    for case_id, fn in CASES.items():
        bits[case_id], fracs = fn(case_id)
        for what, frac in fracs.items():
            spike_fraction_ok(frac, f"{case_id} {what}")
    print(json.dumps({"recorded_with": {"torch": torch.__version__, "hip": torch.version.hip, "numpy": np.__version__,
                                        "device": torch.cuda.get_device_name(0)}, "bits": bits}, indent=1, sort_keys=True))
