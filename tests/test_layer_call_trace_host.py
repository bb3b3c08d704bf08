"""The C-ABI calls of the layer passes (tools/layer_call_trace.py) against the committed
tests/golden/layer_call_trace.txt.gz: entry points in order, scalar arguments, operands (dtype, shape, strides, which
allocation), timer labels.  Runs on CPU tensors against a recording stand-in for the library; no device."""
from tools import layer_call_trace as lct


def test_layer_passes_issue_the_recorded_calls():
    diff = lct.difference(lct.trace())
    assert not diff, ("the layer passes no longer issue the recorded calls (a change made on purpose: "
                      "python tools/layer_call_trace.py --write, and show this diff):\n" + "\n".join(diff[:80]))


def test_tracing_leaves_the_modules_as_they_were():
    from sparch_amd import _capi, streaming
    from sparch_amd import functional as Fn

    before = (Fn.lib, Fn.ptr, Fn.timer, Fn._stream, Fn._status, streaming.lib, streaming.ptr)
    lct.trace()
    assert before == (Fn.lib, Fn.ptr, Fn.timer, Fn._stream, Fn._status, streaming.lib, streaming.ptr)
    assert Fn.lib is _capi.lib and Fn.ptr is _capi.ptr
