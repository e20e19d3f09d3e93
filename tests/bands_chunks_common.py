"""Shared by tests/test_gpu_pipeline_bands_chunks.py and the child processes it starts: the two shapes at which a host call
has several chunks AND bands of rows in every chunk, their steered inputs, and -- run as a program -- one encode and one
decode of a shape under DEGA_PIPELINE_TRACE=1, whose stderr the test reads (the flag is read once per process).

Shape A: C = 2 * 8192 + 1100 = 17 484 channels (chunks of 8 192, 8 192 and 1 100 under DEGA_PIPELINE_CHUNKS=3), T = 200:
DEGA_PIPELINE_BAND_BYTES=65536 gives bands of max(65536 / row bytes, 32) -> 32 rows in every chunk (200 >= the knob's
min_T of 64), 7 launches a chunk, the last of 8 rows.
Shape B: C = 16 * 8192 + 600 = 131 672, T = 96, DEGA_PIPELINE_CHUNKS=17: 17 chunks on the pipeline's 16 slots (chunk 16 takes
over slot 0 within the call), 3 bands a chunk, and more than 65 536 channels: the eight-pair decode workgroups."""
import os
import sys

import numpy as np

BAND_BYTES, BAND_ROWS = "65536", 32
CHUNK = 8192

CA, TA, CHUNKS_A = 2 * CHUNK + 1100, 200, 3
CB, TB, CHUNKS_B = 16 * CHUNK + 600, 96, 17
SLOTS = 16  # MAX_SLOTS of the pipeline

# shape A's steered channels, one of each kind per chunk where the kind allows it
NOISY = (9000, 17000)            # noise: the stream outgrows the usual slab, the chunk is redone (middle and last chunk)
BROKEN = (100, 8292, 16484)      # -1 from row 150 on: the error arises in band 4 and has to survive bands 5 and 6
BROKEN_FROM = 150
CONSTANT = (200, 8392, 16584)

KINDS = ("i32", "i32 static", "be32", "i64", "f32", "f32 48")


def knobs(chunks):
    return {"DEGA_PIPELINE_CHUNKS": str(chunks), "DEGA_PIPELINE_BAND_BYTES": BAND_BYTES}


def chunk_edges(Cn):
    """first and last channel of every chunk of 8 192 channels"""
    out = []
    for c0 in range(0, Cn, CHUNK):
        out += [c0, min(Cn, c0 + CHUNK) - 1]
    return out


def bands_of(T):
    return (T + BAND_ROWS - 1) // BAND_ROWS


def steer(x, noise, broken_value, constant_value):
    for c, col in zip(NOISY, noise):
        x[:, c] = col
    for c in BROKEN:
        x[BROKEN_FROM:, c] = broken_value
    for c in CONSTANT:
        x[:, c] = constant_value
    return x


def input_a(kind, dca):
    """(samples [TA, CA], keyword arguments of encode_job / decode_job) of shape A for a sample type"""
    rng = np.random.default_rng([1751, KINDS.index(kind.replace(" static", ""))])
    T, Cn = TA, CA
    if kind in ("i32", "i32 static", "be32"):
        x = np.cumsum(rng.integers(-50, 51, (T, Cn)), axis=0) + rng.integers(20000, 60000, Cn)[None, :]
        x = steer(np.clip(x, 0, 2 ** 31 - 1).astype(np.int32), [rng.integers(0, 1 << 30, T) for _ in NOISY], -1, 31337)
        if kind == "be32":
            return x.astype(">i4"), dict(adaptive=1, valuesize=32, samples=dca.SAMPLES_BE32)
        return x, dict(adaptive=0 if kind == "i32 static" else 1, valuesize=32, samples=dca.SAMPLES_I32)
    if kind == "i64":  # walks near 2^37: the `last` a launch leaves in seg_state has a non-zero high half
        x = ((1 << 37) + np.cumsum(rng.integers(-(1 << 20), (1 << 20) + 1, (T, Cn)), axis=0)).astype(np.int64)
        x = steer(x, [rng.integers(0, 1 << 38, T) for _ in NOISY], -1, (1 << 37) + 5)
        return x, dict(adaptive=1, valuesize=40, samples=dca.SAMPLES_I64)
    if kind == "f32":  # meter-like magnitudes: 0 ... 5000 with two decimals
        v = (np.round(rng.uniform(0.0, 5000.0, (T, Cn)) * 100.0) / 100.0).astype(np.float32)
        v = steer(v, [rng.integers(0, 1 << 30, T).astype(np.float32) / np.float32(100.0) for _ in NOISY], np.float32(-1.0), np.float32(230.25))
        return v, dict(adaptive=1, valuesize=32, samples=dca.SAMPLES_F32, factor=100.0)
    assert kind == "f32 48"  # * 100: around 2^45, the scale of test_bands_carry_a_64_bit_last_sample_between_launches
    v = (np.cumsum(rng.normal(0, 4e8, (T, Cn)), axis=0) + 3e11).astype(np.float32)
    v = steer(v, [rng.integers(0, 1 << 40, T).astype(np.float32) for _ in NOISY], np.float32(-1.0), np.float32(3e11))
    return v, dict(adaptive=1, valuesize=48, samples=dca.SAMPLES_F32, factor=100.0)


def input_b(kind, dca):
    rng = np.random.default_rng([1752, KINDS.index(kind)])
    if kind == "i32":
        x = np.cumsum(rng.integers(-50, 51, (TB, CB), dtype=np.int32), axis=0, dtype=np.int32) + rng.integers(20000, 60000, CB, dtype=np.int32)[None, :]
        return x, dict(adaptive=1, valuesize=32, samples=dca.SAMPLES_I32)
    assert kind == "f32"
    v = (np.round(rng.uniform(0.0, 5000.0, (TB, CB)) * 100.0) / 100.0).astype(np.float32)
    return v, dict(adaptive=1, valuesize=32, samples=dca.SAMPLES_F32, factor=100.0)


DAMAGED_WAVES = (range(640, 704), range(CHUNK + 320, CHUNK + 384), range(2 * CHUNK + 1024, 2 * CHUNK + 1088), range(2 * CHUNK + 1088, CA))
DAMAGE_SEED = 1753


def damaged_channels():
    """about one channel in eight of shape A: lone ones, the first and last channel of every chunk, and whole waves of 64 (one in
    every chunk, the last chunk's ragged last wave as well); the channels the encoder refused are left alone"""
    rng = np.random.default_rng(DAMAGE_SEED)
    sel = set(np.nonzero(rng.random(CA) < 0.1)[0].tolist()) | set(chunk_edges(CA))
    for w in DAMAGED_WAVES:
        sel |= set(w)
    return np.array(sorted(sel - set(BROKEN)))


def damage(packed, offsets, bits, channels):
    """a copy of the packed streams with 1 ... 3 bits flipped in each of `channels`: anywhere in the stream, and in every fourth
    of them one bit among the last 12 -- under the adaptive model a flip further up derails everything behind it, and a
    fixed-count decode accepts a damaged stream only if it still ends after exactly T samples"""
    rng = np.random.default_rng(DAMAGE_SEED + 1)
    out = np.array(packed, dtype=np.uint8)
    for i, c in enumerate(channels):
        nb, o = int(bits[c]), int(offsets[c])
        flips = [int(rng.integers(max(0, nb - 12), nb))] if i % 4 == 0 else [int(rng.integers(0, nb)) for _ in range(int(rng.integers(1, 4)))]
        for k in flips:
            out[o + k // 8] ^= 0x80 >> (k % 8)
    return out


def main(shape):
    """one encode, one fixed-count decode and -- behind a marker line -- one variable-count decode of the shape's int32 batch"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch  # noqa: F401  (before the library: one HIP runtime per process)
    from __graft_entry__ import load_package
    dca = load_package()
    ctx = dca.Context(0)
    x, kw = (input_a if shape == "A" else input_b)("i32", dca)
    T = x.shape[0]
    packed, offsets, bits, err = ctx.encode_job(x, **kw)
    back, derr = ctx.decode_job(packed, offsets, bits, T, **kw)
    ok = (err == 0) & (derr == 0)
    assert ok.sum() >= x.shape[1] - len(BROKEN) and (back[:, ok] == x[:, ok]).all()
    sys.stderr.flush()
    sys.stderr.write("== variable count ==\n")
    sys.stderr.flush()
    ctx.decode_job(packed, offsets, bits, T, var=True, **kw)
    ctx.close()


if __name__ == "__main__":
    main(sys.argv[1])
