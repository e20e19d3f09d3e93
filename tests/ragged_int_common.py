"""Ragged batches of integer samples: the steered input that tests/test_ragged_int_host.py (the emulator) and
tests/test_gpu_ragged_int.py (the library) share, and what the oracle's restatement gives on it.

C = 64 + 64 + 6 channels of T = 203 rows, so three filling waves:
  wave 0   counts 0, 1, 3, 4, 5, 7, 8, 9, 16, T - 1, T and random ones in between: T_all = 0 and T_end = T in one wave;
  wave 1   every count T ("full": the steady straight-line batch is taken) or T - 3 ("short");
  wave 2   six live lanes with mixed counts.
Every row at or beyond a channel's count holds a value that breaks the range check of diff.c:17-18 if it is looked at, and
would change `last` and the stream: all ones, the sign bit with the value's top bits, a jump of half the range -- in the
width of the kind (32 bits, the narrow value size, 40 bits in an int64; byte swapped for the big-endian kind).  One
channel (HONEST) has such a value INSIDE its count: its error must be reported.

Expected results: the oracle's chain on each channel's own first count[c] samples -- orc.encode_i32 at valuesize 32,
orc.stage("diff" -> "seg" -> "bac") with the exact bit length handed on at the other value sizes."""
import numpy as np

from oracle import orc

T = 203
C = 64 + 64 + 6
HONEST = 17  # a channel of wave 0 with a value out of range inside its count
INVALID = orc.ERROR_INVALID_VALUE

# name: (valuesize, adaptive, big_endian, wide)
KINDS = {
    "i32": (32, 1, False, False),
    "i32_static": (32, 0, False, False),
    "vs16": (16, 1, False, False),
    "vs7": (7, 1, False, False),
    "be32": (32, 1, True, False),
    "i64": (40, 1, False, True),
}


def counts(arrangement="full", seed=5):
    """uint64 [C]; arrangement: "full" (wave 1 all T) or "short" (wave 1 all T - 3)"""
    rng = np.random.default_rng(seed)
    fixed = [0, 1, 3, 4, 5, 7, 8, 9, 16, T - 1, T]
    w0 = np.concatenate([fixed, rng.integers(0, T + 1, 64 - len(fixed))])
    rng.shuffle(w0)
    w0[HONEST] = 120  # (the broken row must lie inside it)
    w1 = np.full(64, T if arrangement == "full" else T - 3)
    w2 = np.array([0, 2, 11, 100, T - 1, T])
    return np.concatenate([w0, w1, w2]).astype(np.uint64)


def poison_values(kind, near):
    """the values rows beyond a count hold, as unsigned container words; `near`: a value the channel's walk takes"""
    vs, _, _, wide = KINDS[kind]
    if wide:
        return [0xFFFFFFFFFFFFFFFF, (1 << 39) | (1 << 38) | 0x8000000000000000, (near + (1 << 39)) & 0xFFFFFFFFFF]
    if vs == 32:
        return [0xFFFFFFFF, 0x80000000, (near + (1 << 31)) & 0xFFFFFFFF]
    # narrow: the bits above the value size are junk the kernel must mask; the field itself is out of range
    return [0xFFFFFFFF, 0x80000000 | (1 << (vs - 1)) | (1 << (vs - 2)), ((near + (1 << (vs - 1)) + (1 << (vs - 3))) & ((1 << vs) - 1)) | 0x5A000000]


def steered(kind, count, seed=11):
    """(values uint64 [T, C] as the oracle reads them inside the counts, container array [T, C] as the kernel reads it).
    Walks stay below a quarter of the value range, so every poison value is out of range from any of them."""
    vs, _, big_endian, wide = KINDS[kind]
    rng = np.random.default_rng(seed + vs)
    if wide:
        start = (1 << 37) + rng.integers(0, 1 << 20, C)
        step = rng.integers(-3000, 3001, (T, C))
    elif vs == 32:
        start = np.where(np.arange(C) % 3 == 0, rng.integers(1 << 20, 1 << 29, C), rng.integers(100, 5000, C))
        start[64:128] = rng.integers(100, 5000, 64)  # wave 1: short codewords from the first sample on
        step = rng.integers(-60, 61, (T, C))
        step[:, 3] = rng.integers(-(1 << 20), 1 << 20, T)  # a channel of long codewords
    else:
        top = 1 << (vs - 2)
        start = rng.integers(top // 4, top // 2, C)
        step = rng.integers(-max(1, top // 32), max(1, top // 32) + 1, (T, C))
    step[0] = 0
    lim = (1 << 38) if wide else (1 << 29 if vs == 32 else (1 << (vs - 2)) - 1)
    vals = np.clip(start[None, :] + np.cumsum(step, axis=0), 1 if vs > 7 else 0, lim).astype(np.uint64)
    x = vals.copy()
    for c in range(C):
        n = int(min(int(count[c]), T))
        p = poison_values(kind, int(vals[min(n, T - 1), c]))
        for t in range(n, T):
            x[t, c] = p[(t + c) % len(p)]
    # the honest error: out of range inside the count
    p = poison_values(kind, int(vals[60, HONEST]))
    x[60, HONEST] = p[0]
    vals[60, HONEST] = p[0] & ((1 << vs) - 1)
    if not wide and vs < 32:  # junk above the value size inside the counts as well
        x |= (rng.integers(0, 1 << (32 - vs), (T, C)).astype(np.uint64) << np.uint64(vs)) * (np.arange(C)[None, :] % 2).astype(np.uint64)
    if wide:
        return vals, np.ascontiguousarray(x.view(np.int64))
    xi = np.ascontiguousarray((x & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32))
    if big_endian:
        xi = np.ascontiguousarray(xi.astype(">i4"))
    return vals, xi


def pack_be(vals, vs):
    v = np.asarray(vals, dtype=np.uint64)
    if vs % 8 == 0:  # whole bytes, most significant first
        return np.ascontiguousarray(v.astype(">u8").view(np.uint8).reshape(-1, 8)[:, 8 - vs // 8:]).tobytes(), len(v) * vs
    bits = np.zeros(len(v) * vs, dtype=np.uint8)
    for k in range(vs):
        bits[k::vs] = (v >> np.uint64(vs - 1 - k)) & np.uint64(1)
    return np.packbits(bits).tobytes(), len(v) * vs


def oracle_channel(vals, vs, adaptive):
    """(status, stream bytes, bits) of the reference chain on one channel's own samples (uint64 values of vs bits)"""
    vals = np.asarray(vals, dtype=np.uint64) & np.uint64((1 << vs) - 1 if vs < 64 else 0xFFFFFFFFFFFFFFFF)
    if vs == 32:
        return orc.encode_i32(vals.astype(np.uint32).view(np.int32), adaptive)
    data, n = pack_be(vals, vs)
    r = 0
    for name in ("diff", "seg", "bac"):
        r, data, n = orc.stage(name, True, data, n, valuesize=vs, adaptive=adaptive)
        if r != 0:
            return r, b"", 0
    return 0, data, n


_expected = {}


def expected(kind, vals, count, key=None):
    """per channel (status, bytes, bits) on its first count[c] samples; count[c] > T: (INVALID, b"", 0).  Computed once per
    key and shared."""
    vs, ad, _, _ = KINDS[kind]
    if key is not None and (kind, key) in _expected:
        return _expected[(kind, key)]
    rows = vals.shape[0]
    want = []
    for c in range(vals.shape[1]):
        n = int(count[c])
        want.append((INVALID, b"", 0) if n > rows else oracle_channel(vals[:n, c], vs, ad))
    if key is not None:
        _expected[(kind, key)] = want
    return want


def mismatch(want, out, bits, err, count=None, rows=None):
    """"" when every channel's status, bit length and stream bytes are the expected ones; else the first difference.
    out: [C, cap] slabs, or (packed, offsets)"""
    for c, (r, data, n) in enumerate(want):
        if int(err[c]) != r:
            return "channel %d: status %d, expected %d" % (c, int(err[c]), r)
        over = count is not None and int(count[c]) > rows
        if r != 0 and not over:
            continue
        if int(bits[c]) != n:
            return "channel %d: %d bits, expected %d" % (c, int(bits[c]), n)
        nb = (n + 7) // 8
        if isinstance(out, tuple):
            packed, offsets = out
            if int(offsets[c + 1]) - int(offsets[c]) != nb:
                return "channel %d: %d packed bytes, expected %d" % (c, int(offsets[c + 1]) - int(offsets[c]), nb)
            got = packed[int(offsets[c]):int(offsets[c]) + nb].tobytes()
        else:
            got = out[c, :nb].tobytes()
        if got != data[:nb]:
            return "channel %d: stream bytes differ" % c
    return ""
