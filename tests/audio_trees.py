"""Test helpers: WAV files written with the standard library (float and extensible headers by hand) and small
Speech Commands / Heidelberg Digits folder trees built from them.  Nothing here is a test."""
import os
import struct
import wave

import numpy as np

RATE = 16000
SC_WORDS = ("no", "up", "yes")           # labels 0, 1, 2 (sorted, after _background_noise_)
SC_TONES = {"no": 300.0, "up": 900.0, "yes": 2500.0}


def write_pcm_wav(path, frames, width, rate=RATE):
    """frames: (n, channels) integers in the sample format's own range (unsigned for 8 bits)."""
    frames = np.asarray(frames)
    if frames.ndim == 1:
        frames = frames[:, None]
    if width == 1:
        raw = frames.astype(np.uint8).tobytes()
    elif width == 3:
        v = frames.astype(np.int64) & 0xFFFFFF
        raw = np.stack([v & 0xFF, (v >> 8) & 0xFF, (v >> 16) & 0xFF], axis=-1).astype(np.uint8).tobytes()
    else:
        raw = frames.astype({2: "<i2", 4: "<i4"}[width]).tobytes()
    with wave.open(str(path), "wb") as w:
        w.setnchannels(frames.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(raw)


def write_raw_wav(path, frames, tag, bits, rate=RATE, extensible=False):
    """A WAV file assembled with struct: format `tag` (1 PCM, 3 IEEE float), optionally behind a
    WAVE_FORMAT_EXTENSIBLE header whose SubFormat GUID carries the tag."""
    frames = np.asarray(frames)
    if frames.ndim == 1:
        frames = frames[:, None]
    ch = frames.shape[1]
    dt = {(1, 16): "<i2", (1, 32): "<i4", (3, 32): "<f4", (3, 64): "<f8"}[(tag, bits)]
    data = frames.astype(dt).tobytes()
    align = ch * bits // 8
    if extensible:
        guid = struct.pack("<H", tag) + bytes.fromhex("000000001000800000aa00389b71")
        fmt = struct.pack("<HHIIHHHHI", 0xFFFE, ch, rate, rate * align, align, bits, 22, bits, 0) + guid
    else:
        fmt = struct.pack("<HHIIHH", tag, ch, rate, rate * align, align, bits)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt
    if tag != 1:  # non-PCM files carry a fact chunk (sample frames); readers skip it
        chunks += b"fact" + struct.pack("<II", 4, len(frames))
    chunks += b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks)


def clip_pcm(n, tone_hz, seed):
    """n samples of int16 PCM: a tone plus noise."""
    g = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    x = 0.3 * np.sin(2 * np.pi * tone_hz * t + g.uniform(0, 2 * np.pi)) + 0.05 * g.uniform(-1, 1, n)
    return np.round(x * 32767).astype(np.int16)


def make_sc_tree(root, n_train=2, n_valid=1, n_test=1, lengths=(16000,), rate=RATE):
    """Speech Commands layout under `root`: _background_noise_ with one long file, one folder per SC_WORDS entry
    holding n_train + n_valid + n_test clips, validation_list.txt and testing_list.txt.  The lists interleave the
    words (not sorted) and write their first entry with a leading "./".  Returns {split: [(relpath, label)]} in
    the order the reference gives (training sorted, the lists in list order)."""
    os.makedirs(os.path.join(root, "_background_noise_"), exist_ok=True)
    write_pcm_wav(os.path.join(root, "_background_noise_", "white_noise.wav"), clip_pcm(3 * rate, 50.0, 1), 2, rate)
    split_of = ["training"] * n_train + ["validation"] * n_valid + ["testing"] * n_test
    files = {"training": [], "validation": [], "testing": []}
    k = 0
    for label, word in enumerate(SC_WORDS):
        os.makedirs(os.path.join(root, word), exist_ok=True)
        for i, split in enumerate(split_of):
            name = f"{word}/{i:02d}_nohash_0.wav"
            write_pcm_wav(os.path.join(root, name), clip_pcm(lengths[k % len(lengths)], SC_TONES[word], k), 2, rate)
            files[split].append((name, label))
            k += 1
    files["training"].sort()
    for split in ("validation", "testing"):  # list order: position-major over the words in reverse, not sorted
        n = len(files[split]) // len(SC_WORDS)
        files[split] = [files[split][w * n + i] for i in range(n) for w in reversed(range(len(SC_WORDS)))]
        with open(os.path.join(root, f"{split}_list.txt"), "w") as f:
            for j, (name, _) in enumerate(files[split]):
                f.write(("./" if j == 0 else "") + name + "\n")
    return files


def hd_name(lang, speaker, trial, digit, ext=".wav"):
    return f"lang-{lang}_speaker-{speaker:02d}_trial-{trial}_digit-{digit}{ext}"


def make_hd_tree(root, n_train=8, n_test=4, lengths=(16000,), rate=RATE):
    """Heidelberg Digits layout (audio/, train_filenames.txt, test_filenames.txt) with WAV files, English and
    German names.  Returns {split: [(name, label)]} in file order."""
    os.makedirs(os.path.join(root, "audio"), exist_ok=True)
    out = {}
    k = 0
    for split, n in (("train", n_train), ("test", n_test)):
        out[split] = []
        for i in range(n):
            lang, digit = ("english", "german")[i % 2], (3 * i + len(split)) % 10
            name = hd_name(lang, i % 5, i, digit)
            write_pcm_wav(os.path.join(root, "audio", name),
                          clip_pcm(lengths[k % len(lengths)], 200.0 + 150.0 * digit, 100 + k), 2, rate)
            out[split].append((name, digit + (10 if lang == "german" else 0)))
            k += 1
        with open(os.path.join(root, f"{split}_filenames.txt"), "w") as f:
            f.write("".join(name + "\n" for name, _ in out[split]))
    return out
