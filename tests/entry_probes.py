"""
Probes of the recurrent entry points' argument checks (tests/test_rec_entry_validation_host.py, tests/test_surrogate_host.py):
an Entry is a name and one valid argument list, and a call of it overrides single arguments.  Pointers are the integer
16 (non-NULL, aligned: nothing is dereferenced before the checks), 20 (misaligned) or None.
"""

P, MIS = 16, 20
NAN = float("nan")
RLIF, RADLIF = 2, 3
B, T, H = 2, 3, 8          # spiking / ANN base shape
HG = 32                    # gated base hidden size


class Entry:
    def __init__(self, name, args):
        self.name, self.args = name, args

    def __call__(self, **over):
        from sparch_amd._capi import lib
        unknown = set(over) - {k for k, _ in self.args}
        assert not unknown, (self.name, unknown)
        return getattr(lib, self.name)(*[over.get(k, v) for k, v in self.args])


def head(first, step=None, Hv=H):
    a = [first, ("B", B), ("dirs", 1), ("T", T), ("H", Hv)]
    if first is None:
        a = a[1:]
    return a + ([(step, 0)] if step else [])


def ptrs(names, none=()):
    none = none.split() if isinstance(none, str) else none
    return [(n, None if n in none else P) for n in names.split()]


WS = [("chan", None), ("chan_bytes", 1 << 20), ("status", P), ("steps_per_launch", T), ("stream", None)]
KIND = ("kind", RADLIF)
ACT = ("act", 0)
