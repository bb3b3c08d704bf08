"""Return codes of the recurrent entry points (reccell.hip, gatedcell.hip) for calls that are refused before
anything is launched: each probe starts from one valid argument list and breaks one thing (or two, for precedence).
Pointers are the integer 16 (non-NULL, aligned: nothing is dereferenced before the checks), 20 (misaligned) or None.
No probe reaches a launch, so the file needs no GPU.  Never call an entry's base list itself: for the step entries it
is a valid call."""
import re

import pytest

from tests.entry_probes import ACT, HG, KIND, MIS, NAN, RADLIF, WS, Entry, H, P, T, head, ptrs
from tests.kit import EALIGN, EINVAL, EWORKSPACE

REC_FWD = Entry("sparch_rec_cell_fwd", head(KIND) + ptrs("Wx scale shift alpha beta a b vpack rec0 u0 w0 s0", "scale shift")
                + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)] + ptrs("s_out s16_out u_save w_save", "s16_out")
                + [("save_bf16", 0), ("spike_count", None)] + WS + [("precision", 0)])
REC_STREAM = Entry("sparch_rec_cell_stream_fwd", head(KIND)
                   + ptrs("Wx scale shift alpha beta a b vpack rec0 u w s s16_state", "scale shift")
                   + [("theta", 1.0), ("p_drop", 0.0)] + ptrs("s_out s16_out spike_count", "s16_out spike_count")
                   + WS + [("precision", 0)])
REC_BWD = Entry("sparch_rec_cell_bwd", head(KIND) + ptrs("g_out g_rate u_save w_save", "g_rate") + [("save_bf16", 0)]
                + ptrs("alpha beta a b vpack_t u0 w0 s0") + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)]
                + ptrs("dWx s_prev16 dparam_ws bn_x bn_mean bn_invstd", "bn_x bn_mean bn_invstd") + WS + [("precision", 0)])
REC_STEP_FWD = Entry("sparch_rec_cell_step_fwd", head(KIND, "t")
                     + ptrs("Wx scale shift alpha beta a b rec u0 w0 s0", "scale shift")
                     + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)]
                     + ptrs("s_out s16_out u_save w_save spike_count s_step16 stream", "s16_out spike_count stream"))
REC_STEP_STREAM = Entry("sparch_rec_cell_step_stream_fwd", head(KIND, "t")
                        + ptrs("Wx scale shift alpha beta a b rec u w s s16_state", "scale shift")
                        + [("theta", 1.0), ("p_drop", 0.0)]
                        + ptrs("s_out s16_out spike_count stream", "s16_out spike_count stream"))
REC_STEP_BWD = Entry("sparch_rec_cell_step_bwd", head(KIND, "t")
                     + ptrs("g_out g_rate u_save w_save alpha beta a b rec u0 w0 s0", "g_rate")
                     + [("theta", 1.0), ("p_drop", 0.0), ("seed", 1)]
                     + ptrs("dWx s_prev16 dparam_ws bn_x bn_mean bn_invstd dwx_step stream", "bn_x bn_mean bn_invstd stream"))
ANN_FWD = Entry("sparch_ann_rec_fwd", head(ACT) + ptrs("Wx scale shift vpack", "scale shift")
                + [("p_drop", 0.0), ("seed", 1)] + ptrs("y_out y_state") + WS)
ANN_BWD = Entry("sparch_ann_rec_bwd", head(ACT) + ptrs("g_out y_state vpack") + [("p_drop", 0.0), ("seed", 1)]
                + ptrs("dpre y_prev") + WS)
ANN_STEP_FWD = Entry("sparch_ann_rec_step_fwd", head(ACT, "s") + ptrs("Wx scale shift rec", "scale shift")
                     + [("p_drop", 0.0), ("seed", 1)] + ptrs("y_out y_state y_step stream", "stream"))
ANN_STEP_BWD = Entry("sparch_ann_rec_step_bwd", head(ACT, "s") + ptrs("g_out y_state rec")
                     + [("p_drop", 0.0), ("seed", 1)] + ptrs("dpre y_prev dpre_step stream", "stream"))
LIGRU_FWD = Entry("sparch_ligru_fwd", head(None, Hv=HG) + ptrs("Wx sc sh Wzx scz shz vpack", "sc sh scz shz")
                  + [("p_drop", 0.0), ("seed", 1)] + ptrs("y_out y_state z_save c_save") + WS)
LIGRU_BWD = Entry("sparch_ligru_bwd", head(None, Hv=HG) + ptrs("g_out y_state z_save c_save vpack_b")
                  + [("p_drop", 0.0), ("seed", 1)] + ptrs("dz_all dc_all yprev_all carry") + WS)
GRU_FWD = Entry("sparch_gru_fwd", head(None, Hv=HG)
                + ptrs("Wx sc sh Wzx scz shz Wrx scr shr vpack_gate vpack_cand", "sc sh scz shz scr shr")
                + [("p_drop", 0.0), ("seed", 1)] + ptrs("y_out y_state z_save r_save c_save") + WS)
GRU_BWD = Entry("sparch_gru_bwd", head(None, Hv=HG) + ptrs("g_out y_state z_save r_save c_save vpack_gate_b vpack_cand_b")
                + [("p_drop", 0.0), ("seed", 1)] + ptrs("dz_all dr_all dc_all yprev_all ry_all carry") + WS)

# entry -> what it checks.  mandatory: NULL is SPARCH_EINVAL; adapt: mandatory under RadLIF only; aligned: the slots of
# the entry's alignment check (a NULL optional pointer passes it); pairs: scale / shift go together.
SPEC = {
    REC_FWD: dict(mandatory="Wx alpha vpack rec0 u0 s0 s_out u_save status", adapt="beta a b w0 w_save",
                  aligned="Wx vpack rec0 u0 w0 s0 s_out s16_out u_save w_save chan", pairs=["scale shift"]),
    REC_STREAM: dict(mandatory="Wx alpha vpack rec0 u s s16_state s_out status", adapt="beta a b w",
                     aligned="Wx vpack rec0 u w s s16_state s_out s16_out chan", pairs=["scale shift"]),
    REC_BWD: dict(mandatory="g_out u_save alpha vpack_t u0 s0 dWx s_prev16 dparam_ws status", adapt="beta a b w0 w_save",
                  aligned="g_out u_save w_save vpack_t u0 w0 s0 dWx s_prev16 dparam_ws chan", pairs=[]),
    REC_STEP_FWD: dict(mandatory="Wx alpha rec u0 s0 s_out u_save s_step16", adapt="beta a b w0 w_save",
                       aligned="Wx rec u0 w0 s0 s_out s16_out u_save w_save s_step16", pairs=["scale shift"]),
    REC_STEP_STREAM: dict(mandatory="Wx alpha rec u s s16_state s_out", adapt="beta a b w",
                          aligned="Wx rec u w s s16_state s_out s16_out", pairs=["scale shift"]),
    REC_STEP_BWD: dict(mandatory="g_out u_save alpha rec u0 s0 dWx s_prev16 dparam_ws dwx_step", adapt="beta a b w0 w_save",
                       aligned="g_out u_save w_save rec u0 w0 s0 dWx s_prev16 dparam_ws dwx_step", pairs=[]),
    ANN_FWD: dict(mandatory="Wx vpack y_out y_state status", aligned="Wx scale shift vpack y_out y_state chan",
                  pairs=["scale shift"]),
    ANN_BWD: dict(mandatory="g_out y_state vpack dpre y_prev status", aligned="g_out y_state vpack dpre y_prev chan", pairs=[]),
    ANN_STEP_FWD: dict(mandatory="Wx y_out y_state y_step", aligned="Wx scale shift rec y_out y_state y_step",
                       pairs=["scale shift"]),
    ANN_STEP_BWD: dict(mandatory="g_out y_state dpre y_prev dpre_step", aligned="g_out y_state rec dpre y_prev dpre_step",
                       pairs=[]),
    LIGRU_FWD: dict(mandatory="Wx Wzx vpack y_out y_state z_save c_save status",
                    aligned="Wx sc sh Wzx scz shz vpack y_out y_state z_save c_save chan", pairs=["sc sh", "scz shz"]),
    LIGRU_BWD: dict(mandatory="g_out y_state z_save c_save vpack_b dz_all dc_all yprev_all carry status",
                    aligned="g_out y_state z_save c_save vpack_b dz_all dc_all yprev_all carry chan", pairs=[]),
    GRU_FWD: dict(mandatory="Wx Wzx Wrx vpack_gate vpack_cand y_out y_state z_save r_save c_save status",
                  aligned="Wx sc sh Wzx scz shz Wrx scr shr vpack_gate vpack_cand y_out y_state z_save r_save c_save chan",
                  pairs=["sc sh", "scz shz", "scr shr"]),
    GRU_BWD: dict(mandatory="g_out y_state z_save r_save c_save vpack_gate_b vpack_cand_b dz_all dr_all dc_all yprev_all "
                            "ry_all carry status",
                  aligned="g_out y_state z_save r_save c_save vpack_gate_b vpack_cand_b dz_all dr_all dc_all yprev_all "
                          "ry_all carry chan", pairs=[]),
}
SPIKING = (REC_FWD, REC_STREAM, REC_BWD, REC_STEP_FWD, REC_STEP_STREAM, REC_STEP_BWD)
ANN = (ANN_FWD, ANN_BWD, ANN_STEP_FWD, ANN_STEP_BWD)
GATED = (LIGRU_FWD, LIGRU_BWD, GRU_FWD, GRU_BWD)
STREAMS = (REC_STREAM, REC_STEP_STREAM)
ALL = SPIKING + ANN + GATED
ids = lambda e: e.name  # noqa: E731


def test_every_recurrent_entry_is_covered():
    from sparch_amd._capi import PROTOTYPES
    rec = {n for n in PROTOTYPES if re.fullmatch(r"sparch_(rec_cell|ann_rec|ligru|gru)(_step)?(_stream)?_(fwd|bwd)", n)}
    assert rec == {e.name for e in ALL} and set(SPEC) == set(ALL)
    for e in ALL:
        assert len(e.args) == len(PROTOTYPES[e.name][1]), e.name


@pytest.mark.parametrize("e", ALL, ids=ids)
def test_shape_refusals(e):
    for k in ("B", "T"):
        assert e(**{k: 0}) == EINVAL and e(**{k: -1}) == EINVAL, k
    bad_h = (0, -4, 2, 6) if e in SPIKING else (0, -4, 6) if e in ANN else (0, -32, 16, 48)
    for h in bad_h:
        assert e(H=h) == EINVAL, h
    for d in (0, 3) + ((2,) if e in STREAMS else ()):      # a stream is causal: one direction
        assert e(dirs=d) == EINVAL, d
    step = e.args[5][0] if e.args[5][0] in ("t", "s") else None      # the step index follows the shape
    if step:
        assert e(**{step: -1}) == EINVAL and e(**{step: T}) == EINVAL
    elif e in GATED:
        assert e(H=1056) == EINVAL          # no instantiation holds the slice: refused before the workspace check
    else:
        assert e(H=1028) == EINVAL


@pytest.mark.parametrize("e", SPIKING + ANN, ids=ids)
def test_unknown_kind_or_act(e):
    if e in SPIKING:
        for kind in (-1, 0, 1, 4):          # LIF / adLIF are not recurrent kinds
            assert e(kind=kind) == EINVAL, kind
    else:
        for act in (-1, 3):
            assert e(act=act) == EINVAL, act
        # the persistent entries refuse it before chan is looked at, and before the alignment check; the step entries
        # only when they pick the kernel, behind the alignment check
        mis = SPEC[e]["aligned"].split()[0]
        assert e(act=3, **{mis: MIS}) == (EINVAL if e in (ANN_FWD, ANN_BWD) else EALIGN)
        if e in (ANN_FWD, ANN_BWD):
            assert e(act=3, chan=P, chan_bytes=0) == EINVAL


@pytest.mark.parametrize("e", ALL, ids=ids)
def test_null_pointers(e):
    for k in SPEC[e]["mandatory"].split():
        assert e(**{k: None}) == EINVAL, k
    for k in SPEC[e].get("adapt", "").split():
        assert e(kind=RADLIF, **{k: None}) == EINVAL, k
    for pair in SPEC[e]["pairs"]:
        sc, sh = pair.split()
        assert e(**{sc: P}) == EINVAL and e(**{sh: P}) == EINVAL, pair
    if e in (REC_FWD, REC_STEP_FWD) + STREAMS:            # either spike output serves; none does not
        assert e(s_out=None, s16_out=None) == EINVAL
    if e is REC_STEP_BWD:
        assert e(t=0, rec=None) == EINVAL                  # steps before the last need the recurrent product
    if e in (ANN_STEP_FWD, ANN_STEP_BWD):
        assert e(s=1, rec=None) == EINVAL                  # steps after the first likewise


@pytest.mark.parametrize("e", ALL, ids=ids)
def test_p_drop_and_precision(e):
    for p in (-0.1, 1.0, NAN) + ((0.1,) if e in STREAMS else ()):      # a stream runs in eval: no dropout
        assert e(p_drop=p) == EINVAL, p
    if any(k == "precision" for k, _ in e.args):
        assert e(precision=7) == EINVAL and e(precision=-1) == EINVAL


@pytest.mark.parametrize("e", ALL, ids=ids)
def test_alignment_and_precedence(e):
    slots = SPEC[e]["aligned"].split()
    partner = {a: b for pair in SPEC[e]["pairs"] for a, b in (pair.split(), pair.split()[::-1])}
    for k in slots:
        both = {partner[k]: P} if k in partner else {}      # scale and shift come as a pair
        assert e(**{k: MIS}, **both) == EALIGN, k
    # every SPARCH_EINVAL check comes before the SPARCH_EALIGN check
    null = next(k for k in SPEC[e]["mandatory"].split() if k != slots[0])
    assert e(**{slots[0]: MIS, null: None}) == EINVAL
    assert e(**{slots[0]: MIS, "B": 0}) == EINVAL
    assert e(**{slots[0]: MIS, "p_drop": 1.0}) == EINVAL


@pytest.mark.parametrize("e", (REC_BWD, REC_STEP_BWD), ids=ids)
def test_batchnorm_triple(e):
    full = dict(bn_x=P, bn_mean=P, bn_invstd=P)
    assert e(bn_x=P) == EINVAL and e(bn_x=P, bn_mean=P) == EINVAL and e(bn_x=P, bn_invstd=P) == EINVAL
    for k in full:                                          # misaligned statistics are SPARCH_EINVAL, not SPARCH_EALIGN
        assert e(**{**full, k: MIS}) == EINVAL, k


@pytest.mark.parametrize("e", [x for x in ALL if any(k == "chan" for k, _ in x.args)], ids=ids)
def test_workspace(e):
    from sparch_amd._capi import lib
    shape = dict(e.args)
    Bp = shape["B"] * shape["dirs"]
    need = (lib.sparch_ligru_chan_bytes(Bp, HG) if e in (LIGRU_FWD, LIGRU_BWD) else
            lib.sparch_gru_chan_bytes(Bp, HG) if e in GATED else lib.sparch_rec_chan_bytes(Bp, T, H))
    assert need > 0
    assert e(chan=None, chan_bytes=need) == EWORKSPACE
    assert e(chan=P, chan_bytes=need - 1) == EWORKSPACE
    assert e(chan=P, chan_bytes=0) == EWORKSPACE
    for spl in (T, 1, 0):                                   # at any launch length
        assert e(chan=None, steps_per_launch=spl) == EWORKSPACE
    assert e(chan=MIS, chan_bytes=need - 1) == EALIGN       # alignment is checked first


def test_save_bf16_needs_the_whole_sequence_forward():
    for spl in (T - 1, 1, 0):
        assert REC_FWD(save_bf16=1, steps_per_launch=spl) == EINVAL, spl
        assert REC_FWD(save_bf16=1, steps_per_launch=spl, Wx=MIS) == EINVAL
        assert REC_BWD(save_bf16=1, steps_per_launch=spl) == EWORKSPACE      # the backward replays chunked: not refused
    assert REC_FWD(save_bf16=1, steps_per_launch=T) == EWORKSPACE
    assert REC_FWD(save_bf16=1, steps_per_launch=T + 5) == EWORKSPACE


def test_backward_ring_offsets_stay_below_2_31():
    # RING x row tiles x column tiles x 6 KiB plane tiles: 32-bit buffer offsets in the kernel.  Checked behind the
    # alignment check, before the workspace
    rows = 32 * 2731                                        # 2731 row tiles x 32 column tiles x 4 x 6144 B >= 2^31
    assert REC_BWD(B=rows, H=1024) == EINVAL and REC_BWD(B=rows - 32, H=1024) == EWORKSPACE
    assert REC_BWD(B=rows, H=1024, g_out=MIS) == EALIGN
