"""CPU: the test encoder's CRCs, FLAC metadata parsing on the host (dataloaders/audio.py: parse_flac), the streams
this build leaves to soundfile, and the argument checks of the FLAC entry points (no launch)."""
import numpy as np
import pytest

from sparch_amd import _capi
from sparch_amd.dataloaders import audio
from tests import flac_writer as fw
from tests.audio_trees import clip_pcm


def test_encoder_crc_check_values():
    assert fw.crc8(b"123456789") == 0xF4
    assert fw.crc16(b"123456789") == 0xFEE8


def _stream(n=5000, **kw):
    return fw.encode_flac(clip_pcm(n, 440.0, 3), 16, 16000, blocks=1024, **kw)


def test_parse_flac_reads_streaminfo_and_skips_metadata(tmp_path):
    x = clip_pcm(5000, 440.0, 3)
    meta = [(1, bytes(37)), (4, b"\x05\x00\x00\x00hello\x00\x00\x00\x00"), (3, bytes(18 * 2))]
    for id3 in (None, b"TIT2" + bytes(20)):
        data = fw.encode_flac(x, 16, 22050, blocks=1024, metadata=meta, id3=id3)
        info = audio.parse_flac(data)
        assert info is not None
        assert (info.min_block, info.max_block, info.sample_rate, info.channels, info.bps, info.total_samples) == \
            (1024, 1024, 22050, 1, 16, 5000)
        assert info.first_frame == fw.first_frame_offset(data) and data[info.first_frame] == 0xFF
        assert info.md5 == fw.md5_of(x, 16)
        path = tmp_path / "clip.flac"
        path.write_bytes(data)
        assert audio.parse_flac(str(path)) == info and audio.parse_flac(path) == info
    stereo = fw.encode_flac(np.stack([x, x[::-1]], 1), 24, 48000, blocks=4096, md5=False)
    info = audio.parse_flac(stereo)
    assert (info.channels, info.bps, info.sample_rate, info.md5) == (2, 24, 48000, bytes(16))


def _unhandled():
    good = _stream()
    si = good.index(b"fLaC") + 4
    return {
        "32-bit": _stream(streaminfo=dict(bps=32)),
        "3-bit": _stream(streaminfo=dict(bps=3)),
        "unknown length": _stream(streaminfo=dict(total=0)),
        "min block < 16": _stream(streaminfo=dict(min_block=8)),
        "min > max block": _stream(streaminfo=dict(min_block=2048)),
        "rate 0": _stream(streaminfo=dict(rate=0)),
        "Ogg FLAC": b"OggS\x00\x02" + bytes(20) + b"\x7fFLAC" + good[si - 4:],
        "STREAMINFO 33 bytes": good[:si + 1] + b"\x00\x00\x21" + good[si + 4:],
        "STREAMINFO not first": good[:si] + b"\x01\x00\x00\x00" + good[si:],
        "metadata past the end": good[:si + 30],
        "zero-length STREAMINFO": b"fLaC" + bytes(64),
        "no frame after the metadata": good[:fw.first_frame_offset(good)] + b"\x00" * 16,
    }


@pytest.mark.parametrize("case", sorted(_unhandled()))
def test_unhandled_streams_go_to_soundfile(tmp_path, case):
    data = _unhandled()[case]
    assert audio.parse_flac(data) is None
    try:
        import soundfile  # noqa: F401
        return  # soundfile present: the missing-package path cannot be taken
    except ImportError:
        pass
    path = tmp_path / "lang-english_speaker-01_trial-0_digit-3.flac"
    path.write_bytes(data)
    for read in (audio.read_audio, audio.read_clip):
        with pytest.raises(ImportError, match="soundfile") as e:
            read(str(path))
        assert str(path) in str(e.value)


def test_md5_bytes_follow_the_sample_width():
    x = np.array([1, -2, 300, -40000], np.int64)
    assert fw.md5_of(x, 24) == audio.hashlib.md5(audio.flac_pcm_bytes(x, 24)).digest()
    assert audio.flac_pcm_bytes([1, -2], 12) == b"\x01\x00\xfe\xff"
    assert audio.flac_pcm_bytes([1, -2], 8) == b"\x01\xfe"
    assert audio.flac_pcm_bytes([-2], 20) == b"\xfe\xff\xff"


def test_flac_entry_points_reject_bad_arguments_without_launching():
    lib = _capi.lib
    assert lib.sparch_flac_workspace_bytes(10, 0) == 256
    assert lib.sparch_flac_workspace_bytes(17, 100) == 512 + 400
    for bad in ((0, 0), (-1, 0), (10, -1), (1 << 40, 0)):
        assert lib.sparch_flac_workspace_bytes(*bad) == 0, bad
    f = lib.sparch_flac_decode_padded
    ok = dict(n_clips=2, clips=256, bytes=256, n_bytes=1024, n_slots=8, n_scratch=0, n_rows=2, ld=1000, dtype=0,
              out=256, err=256, ws=256, ws_bytes=256)

    def call(**kw):
        a = {**ok, **kw}
        return f(a["n_clips"], a["clips"], a["bytes"], a["n_bytes"], a["n_slots"], a["n_scratch"], a["n_rows"],
                 a["ld"], a["dtype"], a["out"], a["err"], a["ws"], a["ws_bytes"], None)

    for bad in (dict(n_clips=0), dict(n_clips=65536), dict(clips=None), dict(bytes=None), dict(n_bytes=0),
                dict(n_rows=0), dict(ld=0), dict(dtype=2), dict(dtype=-1), dict(out=None), dict(err=None),
                dict(ws=None), dict(n_slots=0), dict(n_scratch=-1)):
        assert call(**bad) == -1, bad
    for bad in (dict(n_bytes=1022), dict(bytes=258), dict(ws=264), dict(err=260)):
        assert call(**bad) == -2, bad
    assert call(ws_bytes=255) == -3
