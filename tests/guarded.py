"""
Guard bands for kernels that cannot run under an address sanitizer.

Two tools, both plain torch (they work on CPU tensors too, which is how tests/test_guarded_host.py shows that they
bite):

embed(t, ld, offset)   a 2-D operand with leading dimension `ld` whose first element sits `offset` elements behind a
                       256-byte boundary, inside a larger parent tensor in which every other element is a fill value
                       (NaN; 0x7FC0 for 16-bit planes — a bf16 NaN, which a spike kernel's `x != 0` counts as a
                       spike).  A kernel that READS outside its operand pulls NaN into its result; one that WRITES
                       outside it is caught by view.check(), which compares every fill element bit for bit.  The
                       parent reaches 128 rows of `ld` plus 4 KiB to either side of the view, so an access that
                       strays by up to a whole tile lands in memory the test owns.

guard_arena(module)    a context manager that makes `module` (sparch_amd.functional) allocate from an arena for its
                       duration: module.torch is replaced by a proxy whose empty / empty_like / zeros hand out
                       EXACT-size, 256-byte-aligned slices of one pre-filled buffer (torch's caching allocator rounds
                       every request up to 512 bytes and pools it, so a workspace query that under-reports by a few
                       words can never be noticed there).  The fill begins at the first byte behind the requested
                       size; at exit every byte the arena did not hand out must still hold it.
"""
import math

import torch

FILL16 = 0x7FC0            # bf16 NaN; two of them side by side are an fp32 NaN (0x7FC07FC0)
_FILL_BYTES = (0xC0, 0x7F)  # little endian
ALIGN = 256
PAD_ROWS = 128
PAD_BYTES = 4096

_BITS = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _bits(t):
    """t reinterpreted as integers of its element size (bitwise comparisons; NaN != NaN otherwise)."""
    return t.view(_BITS[t.element_size()])


def default_fill(dtype):
    if dtype.is_floating_point:
        return math.nan
    size = torch.empty(0, dtype=dtype).element_size()
    return {1: 0xA5, 2: FILL16, 4: 0x7FC07FC0, 8: 0x7FC07FC07FC07FC0}[size]


class GuardError(AssertionError):
    pass


def embed(t, ld=None, offset=0, fill=None):
    """A view of shape t.shape (2-D) and strides (ld, 1) holding t's values, `offset` elements behind a 256-byte
    boundary of a parent tensor filled with `fill` (default: NaN, or the dtype's pattern of default_fill).  The
    returned tensor carries .parent, .ld, .check() and .fill_intact() (check() raises GuardError naming the first
    changed fill element relative to the view; fill_intact() returns a bool)."""
    if t.ndim != 2:
        raise ValueError("embed: a 2-D tensor")
    rows, cols = t.shape
    ld = cols if ld is None else int(ld)
    if ld < cols or offset < 0:
        raise ValueError("embed: ld >= width and offset >= 0")
    if fill is None:
        fill = default_fill(t.dtype)
    item = t.element_size()
    per = ALIGN // item
    front = -(-(PAD_ROWS * ld + PAD_BYTES // item) // per) * per       # elements, a multiple of 256 bytes
    back = PAD_ROWS * ld + PAD_BYTES // item
    start = front + offset
    total = start + rows * ld + back
    parent = torch.full((total,), fill, dtype=t.dtype, device=t.device)
    view = torch.as_strided(parent, (rows, cols), (ld, 1), start)
    view.copy_(t)
    owned = torch.zeros(total, dtype=torch.bool, device=t.device)
    torch.as_strided(owned, (rows, cols), (ld, 1), start).fill_(True)
    want = _bits(torch.full((1,), fill, dtype=t.dtype, device=t.device))[0]

    def dirty():
        return (~owned) & (_bits(parent) != want)

    def fill_intact():
        return not bool(dirty().any())

    def check(what="operand"):
        d = dirty()
        if bool(d.any()):
            at = int(torch.nonzero(d)[0]) - start
            r, c = divmod(at, ld)
            raise GuardError(f"{what}: {int(d.sum())} fill element(s) outside the {rows} x {cols} view (ld {ld}, offset "
                             f"{offset}) changed; the first one is at element {at} from the view's start "
                             f"(row {r}, column {c})")

    view.parent, view.ld, view.offset, view.start = parent, ld, offset, start
    view.check, view.fill_intact = check, fill_intact
    return view


class Arena:
    """One buffer, pre-filled with the 0x7FC0 pattern, handed out in exact-size slices that start on 256-byte
    boundaries and are never reused."""

    def __init__(self, nbytes=64 << 20, device="cuda"):
        self.device = torch.device(device)
        nbytes = -(-int(nbytes) // ALIGN) * ALIGN
        self.buf = torch.empty(nbytes + ALIGN, dtype=torch.uint8, device=self.device)
        self.base = (-self.buf.data_ptr()) % ALIGN          # the first 256-byte boundary of the buffer
        self.buf.view(torch.int16).fill_(FILL16)             # (buffers are at least 2-byte aligned)
        self.top = self.base
        self.allocs = []                                     # (offset, nbytes, shape, dtype)

    def empty(self, *size, dtype=None):
        if len(size) == 1 and not isinstance(size[0], int):
            size = tuple(size[0])
        size = tuple(int(s) for s in size)
        dtype = dtype or torch.float32
        nbytes = math.prod(size) * torch.empty(0, dtype=dtype).element_size()
        if nbytes == 0:
            return torch.empty(size, dtype=dtype, device=self.device)
        off = self.top
        if off + nbytes > self.buf.numel():
            raise MemoryError(f"guard arena of {self.buf.numel()} bytes is full: make it larger")
        self.top = self.base + -(-(off - self.base + nbytes) // ALIGN) * ALIGN
        self.allocs.append((off, nbytes, size, dtype))
        return self.buf[off:off + nbytes].view(dtype).view(size)

    def zeros(self, *size, dtype=None):
        return self.empty(*size, dtype=dtype).zero_()

    def nbytes_of(self, t):
        """Bytes the arena handed out for the slice t starts in (None: not an arena slice)."""
        off = t.data_ptr() - self.buf.data_ptr()
        for o, n, _, _ in self.allocs:
            if o == off:
                return n
        return None

    def dirty(self):
        """Offsets (bytes from the buffer's start) of the bytes outside every slice that no longer hold the fill."""
        n = min(self.buf.numel(), self.top + (4 << 20))   # (what lies further behind the last slice is not looked at)
        want = torch.tensor(_FILL_BYTES, dtype=torch.uint8, device=self.device).repeat(n // 2 + 1)[:n]
        marks = torch.zeros(n + 1, dtype=torch.int32, device=self.device)
        if self.allocs:
            starts = torch.tensor([a[0] for a in self.allocs], dtype=torch.int64, device=self.device)
            ends = torch.tensor([a[0] + a[1] for a in self.allocs], dtype=torch.int64, device=self.device)
            marks.index_add_(0, starts, torch.ones_like(starts, dtype=torch.int32))
            marks.index_add_(0, ends, -torch.ones_like(ends, dtype=torch.int32))
        owned = torch.cumsum(marks, 0)[:n] > 0
        return torch.nonzero((~owned) & (self.buf[:n] != want)).flatten()

    def verify(self, what="guard arena"):
        bad = self.dirty()
        if bad.numel() == 0:
            return
        at = int(bad[0])
        owner = None
        for i, (o, n, shape, dtype) in enumerate(self.allocs):
            if o <= at:
                owner = (i, o, n, shape, dtype)
        if owner is None:
            where = "in front of the first slice"
        else:
            i, o, n, shape, dtype = owner
            where = f"{at - (o + n)} byte(s) behind the end of slice #{i} ({dtype}, shape {shape}, {n} bytes)"
        raise GuardError(f"{what}: {bad.numel()} guard byte(s) overwritten; the first one lies {where}")


class _TorchProxy:
    """`torch` as a module under guard sees it: empty / empty_like / zeros on the arena's device come from the arena,
    everything else is torch's own."""

    def __init__(self, arena):
        self._arena = arena

    def __getattr__(self, name):
        return getattr(torch, name)

    def _mine(self, device, kw):
        if kw or device is None and self._arena.device.type != "cpu":
            return False
        return device is None or torch.device(device).type == self._arena.device.type

    def empty(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device, kw):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._arena.empty(*size, dtype=dtype)

    def zeros(self, *size, dtype=None, device=None, **kw):
        if not self._mine(device, kw):
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._arena.zeros(*size, dtype=dtype)

    def empty_like(self, t, **kw):
        if kw or t.device.type != self._arena.device.type:
            return torch.empty_like(t, **kw)
        return self._arena.empty(tuple(t.shape), dtype=t.dtype)


class guard_arena:
    """with guard_arena(functional) as arena: ...  — see the module docstring.  `module` may be None (an arena to
    allocate from by hand: arena.empty(...)).  The guards are verified at exit unless the body raised."""

    def __init__(self, module=None, nbytes=64 << 20, device="cuda"):
        self.module, self.nbytes, self.device = module, nbytes, device

    def __enter__(self):
        self.arena = Arena(self.nbytes, self.device)
        if self.module is not None:
            self._saved = self.module.torch
            self.module.torch = _TorchProxy(self.arena)
        return self.arena

    def __exit__(self, exc_type, exc, tb):
        if self.module is not None:
            self.module.torch = self._saved
        if exc_type is None:
            self.arena.verify()
        return False
