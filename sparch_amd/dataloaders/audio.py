"""
Audio files of the HD and SC datasets -> host samples of channel 0 (replaces `torchaudio.load(path)` at
nonspiking_datasets.py:90, 188).

NORMALISATION UNPINNED, like the mel front-end: torchaudio is third-party and not installed, so the conversion of
integer PCM to [-1, 1) is restated from torchaudio's documented `load(normalize=True)` behaviour:

    8-bit unsigned  (x - 128) / 128        16-bit  x / 2^15        24-bit  x / 2^23        32-bit  x / 2^31

and WAVE_FORMAT_IEEE_FLOAT samples are taken as they are.  No resampling (the reference does none: its fbank
assumes 16 kHz whatever the file's rate); the rate is returned for the caller to warn about.

WAV files are recognised by their RIFF/WAVE header, not by their name, and read with the standard library:
`wave` for plain PCM, the `fmt ` and `data` chunks through `struct` for float data and WAVE_FORMAT_EXTENSIBLE
headers (Python 3.10's `wave` accepts plain PCM only).  16-bit mono PCM stays int16 (half the bytes to the
device; the fbank kernel scales it by 2^-15 on load, the same bits as the fp32 path on x / 2^15); every other
format becomes float32 here.

FLAC files (HD ships FLAC) are recognised by parse_flac, which reads the metadata on the host: an optional leading
ID3v2 tag, "fLaC", STREAMINFO, and the byte offset of the first frame.  The frames are decoded on the device
(sparch_flac_decode_padded, flac.hip): `read_clip` hands the loader the file's bytes and the descriptor, and the
collate function decodes the batch straight into its waveform buffer; `read_audio` decodes one file and copies it
back (it synchronises: for tools and tests).  Streams this build does not decode (32-bit samples, an unknown total
length, Ogg FLAC, a malformed STREAMINFO) and any other container are read with `soundfile`, imported when the
first such file is read; without it the read raises ImportError naming the package and the file.
"""
import hashlib
import os
import struct
import wave
from typing import NamedTuple

import numpy as np

WAVE_FORMAT_PCM = 0x0001
WAVE_FORMAT_IEEE_FLOAT = 0x0003
WAVE_FORMAT_EXTENSIBLE = 0xFFFE


def is_wav(path):
    with open(path, "rb") as f:
        head = f.read(12)
    return len(head) == 12 and head[:4] == b"RIFF" and head[8:12] == b"WAVE"


def read_audio(path):
    """(samples, sample_rate): samples is channel 0 as a 1-D array, int16 for 16-bit mono PCM, float32 in
    [-1, 1) otherwise (x * 2^-(bits - 1) for FLAC, the WAV rule)."""
    clip, rate = read_clip(path)
    if isinstance(clip, FlacStream):
        return _decode_flac(clip), rate
    return clip, rate


def read_clip(path):
    """(clip, sample_rate) without decoding FLAC on the host: clip is the samples of `read_audio` for a WAV file or
    a stream soundfile reads, and a FlacStream (the file's bytes and its descriptor) for a FLAC stream this build
    decodes on the device."""
    if is_wav(path):
        return _read_wav(path)
    with open(path, "rb") as f:
        data = f.read()
    info = parse_flac(data)
    if info is None:
        return _read_other(path)
    return FlacStream(data, info, str(path)), info.sample_rate


class FlacInfo(NamedTuple):
    """STREAMINFO of a FLAC stream, and where its first frame starts in the file."""
    min_block: int
    max_block: int
    sample_rate: int
    channels: int
    bps: int            # bits per sample
    total_samples: int  # per channel
    md5: bytes          # of the decoded samples (all channels, interleaved); 16 zero bytes: not computed
    first_frame: int    # byte offset in the file


class FlacStream(NamedTuple):
    data: bytes
    info: FlacInfo
    path: str


class FlacError(ValueError):
    """A FLAC file that does not decode, or whose samples do not match its STREAMINFO MD5."""


def _skip_id3v2(buf):
    """Length of a leading ID3v2 tag ("ID3", version, flags, 28-bit syncsafe size, optional 10-byte footer)."""
    if len(buf) < 10 or buf[:3] != b"ID3" or any(b & 0x80 for b in buf[6:10]):
        return 0
    size = (buf[6] << 21) | (buf[7] << 14) | (buf[8] << 7) | buf[9]
    return 10 + size + (10 if buf[5] & 0x10 else 0)


def parse_flac(src):
    """FlacInfo of the FLAC stream in `src` (a path or bytes), or None when this build does not decode it on the
    device: not "fLaC" after an optional ID3v2 tag (Ogg FLAC included), a STREAMINFO that is missing, not 34 bytes
    long or inconsistent, metadata running past the end of the file, or a stream outside 4-24 bits per sample, 1-8
    channels and total samples > 0.  Every metadata block after STREAMINFO is skipped by its length."""
    if isinstance(src, (str, os.PathLike)):
        with open(src, "rb") as f:
            src = f.read()
    buf = bytes(src)
    pos = _skip_id3v2(buf)
    if buf[pos:pos + 4] != b"fLaC":
        return None
    pos += 4
    if pos + 4 > len(buf):
        return None
    head, = struct.unpack_from(">I", buf, pos)
    if (head >> 24) & 0x7F != 0 or head & 0xFFFFFF != 34 or pos + 38 > len(buf):   # STREAMINFO comes first
        return None
    si = buf[pos + 4:pos + 38]
    min_block, max_block = struct.unpack_from(">HH", si, 0)
    bits, = struct.unpack_from(">Q", si, 10)
    rate, channels, bps, total = bits >> 44, ((bits >> 41) & 7) + 1, ((bits >> 36) & 31) + 1, bits & ((1 << 36) - 1)
    last = head >> 31
    pos += 38
    while not last:
        if pos + 4 > len(buf):
            return None
        head, = struct.unpack_from(">I", buf, pos)
        last, kind, size = head >> 31, (head >> 24) & 0x7F, head & 0xFFFFFF
        if kind == 0 or kind == 127 or pos + 4 + size > len(buf):   # a second STREAMINFO, an invalid type
            return None
        pos += 4 + size
    if not (16 <= min_block <= max_block and rate > 0 and 4 <= bps <= 24 and total > 0):
        return None
    if pos + 2 > len(buf) or buf[pos] != 0xFF or buf[pos + 1] & 0xFE != 0xF8:   # no frame where one must start
        return None
    return FlacInfo(min_block, max_block, rate, channels, bps, total, si[18:34], pos)


def flac_pcm_bytes(ints, bps):
    """Samples as STREAMINFO's MD5 hashes them: signed little-endian, ceil(bps / 8) bytes each."""
    nb = (bps + 7) // 8
    raw = np.ascontiguousarray(np.asarray(ints, dtype="<i4")).view(np.uint8).reshape(-1, 4)
    return raw[:, :nb].tobytes()


def flac_md5_ok(samples, info):
    """Whether decoded samples of a mono stream (int16, or float32 x * 2^-(bps-1)) hash to its STREAMINFO MD5.  True
    when the MD5 is zero (not computed by the encoder)."""
    if info.md5 == bytes(16):
        return True
    x = np.asarray(samples)
    ints = x.astype(np.int32) if x.dtype == np.int16 else np.rint(x.astype(np.float64) * 2.0 ** (info.bps - 1))
    return hashlib.md5(flac_pcm_bytes(ints.astype(np.int32), info.bps)).digest() == info.md5


def _decode_flac(stream):
    import torch

    from ..functional import flac_decode_padded, flac_error_message

    info = stream.info
    dtype = torch.int16 if info.bps == 16 and info.channels == 1 else torch.float32
    wave = torch.empty(1, info.total_samples, dtype=dtype, device="cuda")
    err = flac_decode_padded([stream.data], [info], wave)
    x, rec = wave[0].cpu().numpy(), err.cpu()
    msg = flac_error_message(rec, [stream.path])
    if msg:
        raise FlacError(msg)
    if info.channels == 1 and not flac_md5_ok(x, info):
        raise FlacError(f"{stream.path}: decoded samples do not match the STREAMINFO MD5")
    return x


def _read_wav(path):
    try:
        with wave.open(str(path), "rb") as w:
            tag, channels, rate, width = WAVE_FORMAT_PCM, w.getnchannels(), w.getframerate(), w.getsampwidth()
            data = w.readframes(w.getnframes())
    except wave.Error:  # not plain PCM: float or WAVE_FORMAT_EXTENSIBLE
        tag, channels, rate, width, data = _wav_chunks(path)
    return _decode(data, tag, channels, width, path), rate


def _wav_chunks(path):
    """(format tag, channels, rate, bytes per sample, data bytes) from the RIFF chunks; the tag of an extensible
    header is the one its SubFormat GUID starts with."""
    with open(path, "rb") as f:
        buf = f.read()
    pos, fmt = 12, None
    while pos + 8 <= len(buf):
        cid, size = struct.unpack_from("<4sI", buf, pos)
        body = buf[pos + 8:pos + 8 + size]
        if cid == b"fmt ":
            if len(body) < 16:
                raise ValueError(f"{path}: truncated fmt chunk")
            tag, channels, rate, _, block_align, _ = struct.unpack_from("<HHIIHH", body)
            if tag == WAVE_FORMAT_EXTENSIBLE:
                if len(body) < 40:
                    raise ValueError(f"{path}: truncated WAVE_FORMAT_EXTENSIBLE header")
                tag = struct.unpack_from("<H", body, 24)[0]
            if channels == 0 or block_align % channels:
                raise ValueError(f"{path}: bad fmt chunk ({channels} channels, block align {block_align})")
            fmt = (tag, channels, rate, block_align // channels)
        elif cid == b"data":
            if fmt is None:
                raise ValueError(f"{path}: data chunk before the fmt chunk")
            return (*fmt, body)
        pos += 8 + size + (size & 1)  # chunks are padded to an even size
    raise ValueError(f"{path}: no data chunk")


def _decode(data, tag, channels, width, path):
    n = len(data) // (width * channels)
    data = data[:n * width * channels]
    if tag == WAVE_FORMAT_PCM:
        if width == 1:
            x = np.frombuffer(data, np.uint8).reshape(n, channels)[:, 0]
            return (x.astype(np.float32) - np.float32(128)) / np.float32(128)
        if width == 2:
            x = np.frombuffer(data, "<i2").reshape(n, channels)[:, 0]
            return x.astype(np.int16) if channels == 1 else x.astype(np.float32) / np.float32(2 ** 15)
        if width == 3:
            b = np.frombuffer(data, np.uint8).reshape(n, channels, 3)[:, 0].astype(np.int32)
            x = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            x = np.where(x >= 1 << 23, x - (1 << 24), x)
            return x.astype(np.float32) / np.float32(2 ** 23)
        if width == 4:
            x = np.frombuffer(data, "<i4").reshape(n, channels)[:, 0]
            return x.astype(np.float32) / np.float32(2 ** 31)
    elif tag == WAVE_FORMAT_IEEE_FLOAT and width in (4, 8):
        x = np.frombuffer(data, "<f4" if width == 4 else "<f8").reshape(n, channels)[:, 0]
        return x.astype(np.float32)
    raise ValueError(f"{path}: unsupported WAV sample format (tag {tag:#x}, {8 * width} bits)")


def _read_other(path):
    try:
        import soundfile
    except ImportError as e:
        raise ImportError(f"sparch_amd.dataloaders: reading {path} (not a WAV file) needs the soundfile "
                          "package") from e
    info = soundfile.info(str(path))
    dtype = "int16" if info.channels == 1 and info.subtype == "PCM_16" else "float32"
    x, rate = soundfile.read(str(path), dtype=dtype, always_2d=True)
    return np.ascontiguousarray(x[:, 0]), rate
