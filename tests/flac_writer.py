"""Test helper: a small FLAC encoder (RFC 9639) written from the format description, able to emit every coding the
decoder must handle on demand, and Heidelberg Digits trees of .flac files.  Nothing here is a test.

encode_flac(samples, bps, ...) -> bytes.  samples: (n,) or (n, channels) integers in the signed range of `bps` bits.
Per frame and channel, `plan(frame, channel, block)` returns the subframe coding as a dict (missing keys: defaults):
    kind       "constant" | "verbatim" | "fixed" | "lpc"            (default "lpc")
    order      fixed 0-4, lpc 1-32                                  (default 2 / 8)
    precision  lpc coefficient bits, 1-15                           (default 12)
    shift      lpc quantisation shift, 0-15 (None: from precision) (default None)
    wasted     wasted bits k (None: as many as the block has)       (default None)
    method     residual coding 0 (4-bit params) or 1 (5-bit)      (default: 1 when a parameter needs > 14)
    porder     partition order 0-8 (lowered until it is valid)      (default 0)
    params     Rice parameter per partition (None: chosen per partition)
    escape     partitions written escaped (raw bits; width 0 when all residuals are 0), or "all"
Frame-level options: blocks (a block size, or the list of block sizes: variable blocking or forced sizes),
variable, assignment ("independent" | "left_side" | "side_right" | "mid_side", or a callable of the frame),
bs_code / sr_code / ss_code forcing ("auto"), bad_crc8 / bad_crc16 (sets of frames written with a wrong CRC),
md5 (True: computed; False: zero; bytes: as given), metadata (extra (type, body) blocks after STREAMINFO), id3
(bytes of a leading ID3v2 tag body, or None), streaminfo overrides (dict).
"""
import hashlib
import os
import struct

import numpy as np

from tests.audio_trees import RATE, clip_pcm, hd_name

RATES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10,
         96000: 11}
SS_CODE = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}


def crc8(data, crc=0):
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = ((crc << 1) ^ 0x07) & 0xFF if crc & 0x80 else (crc << 1) & 0xFF
    return crc


_CRC16 = []
for _v in range(256):
    _r = _v << 8
    for _ in range(8):
        _r = ((_r << 1) ^ 0x8005) & 0xFFFF if _r & 0x8000 else (_r << 1) & 0xFFFF
    _CRC16.append(_r)


def crc16(data, crc=0):
    tab = _CRC16
    for b in data:
        crc = ((crc << 8) & 0xFFFF) ^ tab[(crc >> 8) ^ b]
    return crc


class BitWriter:
    """MSB-first bit fields, packed at the end (numpy: fields of up to 63 bits)."""

    def __init__(self):
        self.vals, self.widths = [], []

    def put(self, value, width):
        if width:
            self.vals.append(np.array([int(value) & ((1 << width) - 1)], np.uint64))
            self.widths.append(np.array([width], np.int64))

    def put_array(self, values, widths):
        values = np.asarray(values, np.int64)
        widths = np.broadcast_to(np.asarray(widths, np.int64), values.shape)
        keep = widths > 0
        mask = (np.left_shift(np.uint64(1), widths[keep].astype(np.uint64)) - np.uint64(1))
        self.vals.append(values[keep].astype(np.uint64) & mask)
        self.widths.append(widths[keep])

    def rice(self, u, p):
        """Rice codes of non-negative u with parameter p: q zeros, a one, p low bits."""
        u = np.asarray(u, np.int64)
        q, low = u >> p, u & ((1 << p) - 1)
        full, rem = q // 32, q % 32
        n_fields = full + 1
        vals = np.zeros(int(n_fields.sum()), np.int64)
        widths = np.full(len(vals), 32, np.int64)
        last = np.cumsum(n_fields) - 1
        vals[last] = (1 << p) | low
        widths[last] = rem + p + 1
        self.put_array(vals, widths)

    def nbits(self):
        return int(sum(int(w.sum()) for w in self.widths))

    def getbytes(self):
        """Packed bytes, zero-padded to a byte boundary."""
        if not self.vals:
            return b""
        vals, w = np.concatenate(self.vals), np.concatenate(self.widths)
        idx = np.repeat(np.arange(len(w)), w)
        starts = np.cumsum(w) - w
        k = np.arange(int(w.sum())) - starts[idx]
        bits = (vals[idx] >> (w[idx] - 1 - k).astype(np.uint64)) & np.uint64(1)
        return np.packbits(bits.astype(np.uint8)).tobytes()


def utf8_number(v):
    if v < 0x80:
        return bytes([v])
    for n, lim in ((2, 1 << 11), (3, 1 << 16), (4, 1 << 21), (5, 1 << 26), (6, 1 << 31), (7, 1 << 36)):
        if v < lim:
            out = []
            for _ in range(n - 1):
                out.append(0x80 | (v & 0x3F))
                v >>= 6
            lead = 0xFE if n == 7 else ((0xFF << (8 - n)) & 0xFF) | v
            return bytes([lead] + out[::-1])
    raise ValueError("number too large")


def zigzag(r):
    r = np.asarray(r, np.int64)
    return np.where(r >= 0, 2 * r, -2 * r - 1)


def best_param(u, limit):
    m = float(np.mean(u)) if len(u) else 0.0
    return int(min(limit, max(0, int(np.floor(np.log2(m + 1))) if m > 0 else 0)))


def lpc_coefs(x, order, precision, shift):
    """Least-squares predictor of x from its last `order` samples, quantised to `precision` bits."""
    x = np.asarray(x, np.float64)
    n = len(x)
    if n <= order:
        c = np.zeros(order)
    else:
        A = np.stack([x[order - 1 - j:n - 1 - j] for j in range(order)], axis=1)
        c = np.linalg.lstsq(A, x[order:], rcond=None)[0]
    cmax = float(np.max(np.abs(c))) if order else 0.0
    if shift is None:
        shift = precision - 1 - (int(np.ceil(np.log2(cmax))) if cmax > 0 else 0)
        shift = int(min(15, max(0, shift)))
    lo, hi = -(1 << (precision - 1)), (1 << (precision - 1)) - 1
    return np.clip(np.round(c * (1 << shift)), lo, hi).astype(np.int64), shift


def predict(x, coefs, shift):
    """Prediction of samples order.. of x: sum_j c_j x[i-1-j] >> shift (arbitrary precision via int64 / object)."""
    x = np.asarray(x, np.int64)
    order = len(coefs)
    n = len(x)
    acc = np.zeros(n - order, np.int64)
    for j, c in enumerate(coefs):
        acc += int(c) * x[order - 1 - j:n - 1 - j]
    return acc >> shift


FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


def write_residual(bw, res, order, bs, spec):
    porder = int(spec.get("porder", 0))
    while porder > 0 and ((bs >> porder) << porder != bs or (bs >> porder) < order):
        porder -= 1
    part = bs >> porder
    u = zigzag(res)
    bounds = [(0 if p == 0 else p * part - order, (p + 1) * part - order) for p in range(1 << porder)]
    params = spec.get("params")
    if params is None:
        params = [best_param(u[a:b], 30) for a, b in bounds]
    params = [int(p) for p in params]
    method = spec.get("method")
    if method is None:
        method = 1 if max(params) > 14 else 0
    escape_code = 31 if method else 15
    esc = spec.get("escape", ())
    esc = set(range(1 << porder)) if esc == "all" else set(esc)
    bw.put(method, 2)
    bw.put(porder, 4)
    for p, (a, b) in enumerate(bounds):
        r = np.asarray(res[a:b], np.int64)
        if p in esc:
            width = 0 if not len(r) or not np.any(r) else int(max(int(r.max()).bit_length(),
                                                                 int((-r - 1).max()).bit_length())) + 1
            bw.put(escape_code, 5 if method else 4)
            bw.put(width, 5)
            if width:
                bw.put_array(r, width)
        else:
            param = min(params[p], escape_code - 1)
            bw.put(param, 5 if method else 4)
            bw.rice(u[a:b], param)


def write_subframe(bw, x, bps, spec):
    x = np.asarray(x, np.int64)
    bs = len(x)
    kind = spec.get("kind", "lpc")
    wasted = spec.get("wasted")
    if wasted is None:
        nz = x[x != 0]
        wasted = 0 if not len(nz) else int(min(bps - 1, min((int(v) & -int(v)).bit_length() - 1 for v in
                                                            np.unique(np.abs(nz)))))
    if wasted and np.any(x & ((1 << wasted) - 1)):
        raise ValueError("samples not divisible by 2^wasted")
    y = x >> wasted
    b = bps - wasted
    type_code = {"constant": 0, "verbatim": 1}.get(kind)
    if kind == "fixed":
        order = min(int(spec.get("order", 2)), bs)
        type_code = 8 + order
    elif kind == "lpc":
        order = min(int(spec.get("order", 8)), bs)
        type_code = 31 + order
    bw.put(0, 1)
    bw.put(type_code, 6)
    if wasted:
        bw.put(1, 1)
        bw.put(1, wasted)          # k - 1 zeros, then a one
    else:
        bw.put(0, 1)
    if kind == "constant":
        if np.any(y != y[0]):
            raise ValueError("constant subframe of a non-constant block")
        bw.put(int(y[0]), b)
        return
    if kind == "verbatim":
        bw.put_array(y, b)
        return
    bw.put_array(y[:order], b)
    if kind == "fixed":
        coefs, shift = FIXED[order], 0
    else:
        precision = int(spec.get("precision", 12))
        coefs, shift = lpc_coefs(y, order, precision, spec.get("shift"))
        bw.put(precision - 1, 4)
        bw.put(shift, 5)
        bw.put_array(coefs, precision)
    res = y[order:] - predict(y, coefs, shift) if order < bs else y[:0]
    write_residual(bw, res, order, bs, spec)


def bs_code_of(bs, force="auto"):
    if force != "auto":
        return force
    if bs == 192:
        return 1
    for c in range(2, 6):
        if bs == 576 << (c - 2):
            return c
    for c in range(8, 16):
        if bs == 256 << (c - 8):
            return c
    return 6 if bs <= 256 else 7


def sr_code_of(rate, force="auto"):
    if force != "auto":
        return force
    if rate in RATES:
        return RATES[rate]
    if rate % 1000 == 0 and rate // 1000 < 256:
        return 12
    if rate < 65536:
        return 13
    return 14


def frame_header(bs, number, variable, assign, bps, rate, bs_code="auto", sr_code="auto", ss_code="auto"):
    bc, sc = bs_code_of(bs, bs_code), sr_code_of(rate, sr_code)
    ssc = SS_CODE.get(bps, 0) if ss_code == "auto" else ss_code
    h = bytearray([0xFF, 0xF8 | int(variable), (bc << 4) | sc, (assign << 4) | (ssc << 1)])
    h += utf8_number(number)
    if bc == 6:
        h += bytes([bs - 1])
    elif bc == 7:
        h += struct.pack(">H", bs - 1)
    if sc == 12:
        h += bytes([rate // 1000])
    elif sc == 13:
        h += struct.pack(">H", rate)
    elif sc == 14:
        h += struct.pack(">H", rate // 10)
    return bytes(h)


ASSIGN = {"left_side": 8, "side_right": 9, "mid_side": 10}


def encode_frame(block, number, variable, bps, rate, assignment="independent", plan=None, frame=0, bs_code="auto",
                 sr_code="auto", ss_code="auto", bad_crc8=False, bad_crc16=False):
    bs, ch = block.shape
    if assignment != "independent" and ch != 2:
        raise ValueError("stereo decorrelation needs 2 channels")
    if assignment == "independent":
        assign, chans, widths = ch - 1, [block[:, c] for c in range(ch)], [bps] * ch
    else:
        left, right = block[:, 0].astype(np.int64), block[:, 1].astype(np.int64)
        side = left - right
        assign = ASSIGN[assignment]
        chans, widths = {"left_side": ([left, side], [bps, bps + 1]),
                         "side_right": ([side, right], [bps + 1, bps]),
                         "mid_side": ([(left + right) >> 1, side], [bps, bps + 1])}[assignment]
    head = frame_header(bs, number, variable, assign, bps, rate, bs_code, sr_code, ss_code)
    head += bytes([crc8(head) ^ (0x55 if bad_crc8 else 0)])
    bw = BitWriter()
    for c, (x, w) in enumerate(zip(chans, widths)):
        write_subframe(bw, x, w, dict(plan(frame, c, x) if plan else {}))
    body = head + bw.getbytes()
    return body + struct.pack(">H", crc16(body) ^ (0x1234 if bad_crc16 else 0))


def md5_of(samples, bps):
    nb = (bps + 7) // 8
    raw = np.ascontiguousarray(np.asarray(samples, "<i4")).view(np.uint8).reshape(-1, 4)[:, :nb]
    return hashlib.md5(raw.tobytes()).digest()


def encode_flac(samples, bps, rate=RATE, *, blocks=4096, variable=False, assignment="independent", plan=None,
                bs_code="auto", sr_code="auto", ss_code="auto", bad_crc8=(), bad_crc16=(), md5=True, metadata=(),
                id3=None, streaminfo=None):
    x = np.asarray(samples, np.int64)
    if x.ndim == 1:
        x = x[:, None]
    n, ch = x.shape
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    if x.size and (x.min() < lo or x.max() > hi):
        raise ValueError("samples outside the signed range of bps bits")
    sizes = [blocks] * (-(-n // blocks)) if isinstance(blocks, int) else list(blocks)
    if isinstance(blocks, int):
        sizes[-1] = n - blocks * (len(sizes) - 1)
    if sum(sizes) != n:
        raise ValueError("block sizes do not add up to the sample count")
    frames, start = [], 0
    for f, bs in enumerate(sizes):
        assign = assignment(f) if callable(assignment) else assignment
        number = start if variable else f
        frames.append(encode_frame(x[start:start + bs], number, variable, bps, rate, assign, plan, f, bs_code,
                                   sr_code, ss_code, f in set(bad_crc8), f in set(bad_crc16)))
        start += bs
    if isinstance(blocks, int):
        min_bs = max_bs = blocks
    else:
        body = sizes[:-1] if len(sizes) > 1 else sizes
        min_bs, max_bs = min(body), max(sizes)
    info = dict(min_block=min_bs, max_block=max_bs, min_frame=min(len(f) for f in frames),
                max_frame=max(len(f) for f in frames), rate=rate, channels=ch, bps=bps, total=n,
                md5=md5_of(x.reshape(-1), bps) if md5 is True else (bytes(16) if md5 is False else md5))
    info.update(streaminfo or {})
    si = struct.pack(">HH", info["min_block"], info["max_block"])
    si += b"".join((v if v < 1 << 24 else 0).to_bytes(3, "big") for v in (info["min_frame"], info["max_frame"]))
    si += ((info["rate"] << 44) | ((info["channels"] - 1) << 41) | ((info["bps"] - 1) << 36) |
           info["total"]).to_bytes(8, "big")
    si += info["md5"]
    blocks_meta = [(0, si)] + list(metadata)
    out = bytearray()
    if id3 is not None:
        z = len(id3)
        out += b"ID3\x04\x00\x00" + bytes([(z >> 21) & 0x7F, (z >> 14) & 0x7F, (z >> 7) & 0x7F, z & 0x7F]) + id3
    out += b"fLaC"
    for i, (kind, body) in enumerate(blocks_meta):
        out += bytes([(0x80 if i == len(blocks_meta) - 1 else 0) | kind]) + len(body).to_bytes(3, "big") + body
    for fr in frames:
        out += fr
    return bytes(out)


def first_frame_offset(data):
    """Byte offset of the first frame of a stream written by encode_flac."""
    pos = 10 + ((data[6] << 21) | (data[7] << 14) | (data[8] << 7) | data[9]) if data[:3] == b"ID3" else 0
    pos += 4
    while True:
        head, size = data[pos], int.from_bytes(data[pos + 1:pos + 4], "big")
        pos += 4 + size
        if head & 0x80:
            return pos


def write_flac(path, samples, bps=16, rate=RATE, **kw):
    data = encode_flac(samples, bps, rate, **kw)
    with open(path, "wb") as f:
        f.write(data)
    return data


def make_hd_flac_tree(root, n_train=8, n_test=4, lengths=(16000,), rate=RATE, flac_every=1, **kw):
    """tests.audio_trees.make_hd_tree's layout, names and samples, with every `flac_every`-th file (file index k,
    counted over both splits) written as FLAC (name ending .flac) and the others as WAV."""
    from tests.audio_trees import write_pcm_wav
    os.makedirs(os.path.join(root, "audio"), exist_ok=True)
    out = {}
    k = 0
    for split, n in (("train", n_train), ("test", n_test)):
        out[split] = []
        for i in range(n):
            lang, digit = ("english", "german")[i % 2], (3 * i + len(split)) % 10
            pcm = clip_pcm(lengths[k % len(lengths)], 200.0 + 150.0 * digit, 100 + k)
            if k % flac_every == 0:
                name = hd_name(lang, i % 5, i, digit, ".flac")
                write_flac(os.path.join(root, "audio", name), pcm, 16, rate, **kw)
            else:
                name = hd_name(lang, i % 5, i, digit)
                write_pcm_wav(os.path.join(root, "audio", name), pcm, 2, rate)
            out[split].append((name, digit + (10 if lang == "german" else 0)))
            k += 1
        with open(os.path.join(root, f"{split}_filenames.txt"), "w") as f:
            f.write("".join(name + "\n" for name, _ in out[split]))
    return out
