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
format becomes float32 here.  Any other container (HD ships FLAC) is read with `soundfile`, imported when the
first such file is read; without it the read raises ImportError naming the package and the file.
"""
import struct
import wave

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
    [-1, 1) otherwise."""
    if is_wav(path):
        return _read_wav(path)
    return _read_other(path)


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
