"""The C-ABI calls of the layer passes (tools/layer_call_trace.py) against the committed
tests/golden/layer_call_trace.txt.gz: entry points in order, scalar arguments, operands (dtype, shape, strides, which
allocation), timer labels.  Runs on CPU tensors against a recording stand-in for the library; no device."""
import os
import re

from tools import layer_call_trace as lct


def test_layer_passes_issue_the_recorded_calls():
    diff = lct.difference(lct.trace())
    assert not diff, ("the layer passes no longer issue the recorded calls (a change made on purpose: "
                      "python tools/layer_call_trace.py --write, and show this diff):\n" + "\n".join(diff[:80]))


def test_tracing_leaves_the_modules_as_they_were():
    from sparch_amd import _capi, snns, streaming
    from sparch_amd import functional as Fn

    def state():
        return (Fn.lib, Fn.ptr, Fn.timer, Fn._stream, Fn._status, streaming.lib, streaming.ptr, snns._check_bidir_input,
                snns._fast_rand_ok)

    before = state()
    lct.trace()
    assert before == state()
    assert Fn.lib is _capi.lib and Fn.ptr is _capi.ptr


# What functional.py names and the layer passes do not issue: the streaming entries (streaming.py's trace cases are its
# own), the loss, the data side, the host routine behind SNN.forward's state draws (the tracer keeps them with
# torch.rand), and the two GEMM forms that no layer input of _layer_input selects.
NOT_THE_LAYER_PATH = re.compile(r"sparch_(\w*stream\w*|mt19937_uniform_f32|ce_loss|bin_events|events_\w+|audio_\w+|"
                                r"augment_\w+|fbank_\w+|flac_\w+|gemm_auto_(nt|tn))")


def test_every_entry_point_the_host_code_names_is_in_the_trace():
    """The names come from the text of functional.py and snns.py — written out, or a written stem with the suffixes the
    host code appends — so an entry point that arrives later is either traced or listed above on purpose."""
    from sparch_amd import _capi

    text = "".join(open(os.path.join(lct.ROOT, "sparch_amd", f)).read() for f in ("functional.py", "snns.py"))
    stems = set(re.findall(r"sparch_[a-z0-9_]+", text))
    suffixes = re.compile(r"(_len|_pk|_sg|_st|_red|_seq)*")
    named = {n for n in _capi.PROTOTYPES for s in stems if n.startswith(s) and suffixes.fullmatch(n[len(s):])}
    named = {n for n in named if not NOT_THE_LAYER_PATH.fullmatch(n)}
    issued = set(re.findall(r"^(?:q\d+ = )?(sparch_\w+)\(", lct.recorded(), re.M))
    assert len(named) > 100 and not named - issued, f"named by the host code, never traced: {sorted(named - issued)}"
    for family in ("_len", "_pk", "_st", "_sg", "_red", "_seq"):
        assert any(n.endswith(family) for n in issued), family
    for stem in ("sparch_bidir_", "sparch_delay_", "sparch_synapse_", "sparch_pack_rows", "sparch_unpack_rows"):
        assert any(n.startswith(stem) for n in issued), stem
