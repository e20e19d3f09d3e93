"""Shared by tests/test_float_edges_host.py, tests/test_gpu_float_edges.py and tests/golden/make_golden_float_edges.py: the float
boundary of the DEGA chain -- Normalize in front of the encoder, Denormalize behind the decoder (normalize.c:9-41) -- walked
across float32.  Here: a plain restatement of the two in numpy float32 (one operation per rounding; independent of the
oracle's C, the two are held to each other and to the fixture in the host tests), the seeded corpus of values per (value size,
factor), every value with the name of its class, the channel sets that show the fused encoder's integers (an encoder shows them
only where the channel is coded), the integer series for the decoders' exit, conditions() that the corpus has to meet, and
tests/golden/float_edges.npz (what the compiled reference returned).  Integers, statuses and streams are compared bit for
bit; a float that is a NaN only has to be a NaN."""
import os
import zipfile
import zlib

import numpy as np

from oracle import orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "float_edges.npz")
INVALID = -1  # ERROR_INVALID_VALUE
INDEFINITE = np.uint64(0x8000000000000000)  # what the reference's conversion gives for a NaN and for 2^63 (cvttss2si)

VALUE_SIZES = (1, 2, 8, 17, 25, 26, 31, 32, 33, 40, 63, 64)
FACTORS = (100.0, 1.0, 0.5, 1000.0, 3.3, 1e-3, 0.0, -100.0, float("nan"))
HUGE_FACTORS = (1e38, 3e38)  # Denormalize: the quotients of +-1 (of +-1 .. +-3) are subnormal; Normalize: subnormal readings reach 0.5 and more
N_VALUES, N_ALIGNED = 4133, 4096  # values per (value size, factor): one per channel, no multiple of 4 / a multiple of 4
CLASSES = ("bounds", "ties", "absorbed", "specials", "printed", "random")
T_ROWS, N_CHANNELS = 26, 330  # rows (no multiple of the encoder's batch of 8 rows) and channels (two workgroups, the second partial)
# the fused forms: (value size, factor) -- 32 bits, narrow, the narrow size whose upper bound rounds up, two int64 sizes
FUSED = ((32, 100.0), (32, 0.5), (32, 3.3), (32, -100.0), (17, 100.0), (17, 3.3), (26, 100.0), (26, 0.5), (40, 100.0), (40, -100.0), (64, 100.0), (64, 3.3))
FUSED_SIZES = (32, 17, 26, 40, 64)
FUSED_IN_FIXTURE = ((32, 100.0), (32, 3.3), (17, 100.0), (26, 100.0), (40, 100.0), (64, 100.0))  # a thin sample of their channels through the reference
HUGE_SIZES = (17, 32, 64)


def factor_index(factor):
    for i, f in enumerate(FACTORS + HUGE_FACTORS):
        if f == factor or (f != f and factor != factor):
            return i
    raise KeyError(factor)


def key(vs, factor):
    return "n%d.f%d" % (vs, factor_index(factor))


def _keys():
    return tuple((vs, f) for vs in VALUE_SIZES for f in FACTORS) + tuple((vs, f) for vs in HUGE_SIZES for f in HUGE_FACTORS)


KEYS = _keys()  # every (value size, factor) of the corpus


def plain(factor):
    """a factor with which products can be steered: finite and not zero"""
    return factor == factor and factor != 0.0 and abs(factor) != float("inf")


# ---- the restatement ---------------------------------------------------------------------------------------------------------

def as_f32(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


def as_bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


def bounds(vs):
    """normalize.c:21: lo = -(float)2^(vs-1), hi = (float)(uint64)(2^(vs-1) - 1) -- which rounds up to 2^(vs-1) from 26 bits on"""
    lo = -np.float32(2.0 ** (vs - 1))
    hi = np.array([(1 << (vs - 1)) - 1], dtype=np.uint64).astype(np.float32)[0]
    return lo, hi


def mask(vs):
    return np.uint64((1 << vs) - 1)


def rounded(bits, factor):
    """normalize.c:17-20: p = f32(v * f), then f32(p + 0.5) or f32(p - 0.5) by the sign of v; NaN and zeros are left alone.
    Returns (p, w), float32."""
    v, f, h = as_f32(bits), np.float32(factor), np.float32(0.5)
    with np.errstate(all="ignore"):
        p = v * f
        w = np.where(v > 0, p + h, np.where(v < 0, p - h, v))
    assert p.dtype == np.float32 and w.dtype == np.float32
    return p, w


def normalize(bits, factor, vs):
    """(in range bool [n], the low vs bits of the truncated value uint64 [n] -- 0 where out of range)"""
    _, w = rounded(bits, factor)
    lo, hi = bounds(vs)
    with np.errstate(invalid="ignore"):
        ok = ~((w < lo) | (w > hi))
    with np.errstate(invalid="ignore"):
        wide = w.astype(np.float64)  # (a signalling NaN raises the flag)
    big = np.isnan(wide) | (wide >= 2.0 ** 63)
    n = np.trunc(np.where(big | ~ok, 0.0, wide)).astype(np.int64).view(np.uint64)  # (exact: a float32 in [-2^63, 2^63))
    n = np.where(big, INDEFINITE, n) & mask(vs)
    return ok, np.where(ok, n, np.uint64(0))


def sign_extend(u, vs):
    u = np.ascontiguousarray(u, dtype=np.uint64)
    if vs == 64:
        return u.view(np.int64)
    return (u << np.uint64(64 - vs)).view(np.int64) >> np.int64(64 - vs)


def denormalize(u, factor, vs):
    """normalize.c:36-38: f32(sign_extend(u, vs)) / f32(factor), as bit patterns uint32 [n]"""
    with np.errstate(all="ignore"):
        q = sign_extend(u, vs).astype(np.float32) / np.float32(factor)
    assert q.dtype == np.float32
    return as_bits(q)


def float_of_int(n):
    """float32 of a Python integer, rounded to nearest, ties to even, in integer arithmetic: what denormalize's cast is held to"""
    if n == 0:
        return np.float32(0.0)
    a = abs(n)
    drop = max(0, a.bit_length() - 24)
    m, rest = a >> drop, a & ((1 << drop) - 1)
    if drop and (rest > (1 << (drop - 1)) or (rest == (1 << (drop - 1)) and (m & 1))):
        m += 1
    x = np.float32(np.ldexp(np.float64(m), drop))  # (m <= 2^24: exact)
    return -x if n < 0 else x


def conversion_tie(n):
    """the integer lies exactly between two float32 values"""
    a = abs(int(n))
    drop = a.bit_length() - 24
    return drop >= 1 and (a & ((1 << drop) - 1)) == (1 << (drop - 1))


def same_float_bits(got, want):
    """bit for bit; a NaN only has to be a NaN"""
    got, want = np.ascontiguousarray(got, dtype=np.uint32), np.ascontiguousarray(want, dtype=np.uint32)
    nan = np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32))
    return (got == want) | nan


def neighbour(bits, k):
    """the float k steps above (k < 0: below) each of `bits`, by bit pattern, the zeros counted once, clipped at the infinities"""
    bits = np.asarray(bits, dtype=np.uint32).astype(np.int64)
    mag = bits & 0x7FFFFFFF
    at = np.where(bits & 0x80000000, -mag, mag) + np.asarray(k, dtype=np.int64)
    at = np.clip(at, -0x7F800000, 0x7F800000)
    return np.where(at < 0, 0x80000000 | -at, at).astype(np.uint32)


def fdiv(a, f):
    """float32 a / float32 f, as bit patterns"""
    with np.errstate(all="ignore"):
        return as_bits(np.asarray(a, dtype=np.float32) / np.float32(f))


# ---- the corpus --------------------------------------------------------------------------------------------------------------

SPECIALS = np.array(
    [0x00000000, 0x80000000,  # +-0
     0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,  # the smallest and the largest subnormal
     0x00800000, 0x80800000, 0x7F7FFFFF, 0xFF7FFFFF,  # +-FLT_MIN, +-FLT_MAX
     0x7F800000, 0xFF800000,  # +-inf
     0x7FC00000, 0xFFC00000, 0x7FC12345, 0xFFC54321, 0x7FFFFFFF, 0xFFFFFFFF,  # quiet NaNs
     0x7F800001, 0xFF800001, 0x7FA00000, 0xFFBFFFFF, 0x7F812345],  # signalling NaNs
    dtype=np.uint32)
SPECIAL_VALUES = (1e37, -1e37, 3e38, -3e38, 1e36, 3.5e35, -3.5e35, 4e38 / 3.3,  # products that overflow to inf with some factor
                  1e-30, -1e-30, 1e-40, -1e-40, 1e-44, -1e-44, 1.1e-38, -1.1e-38, 1.5e-36, -1.5e-36, 2e-41, 1e-38, -1e-38, 4e-39,  # ... that underflow
                  0.004, -0.004, 0.005, -0.005, 0.0049999, 0.5, -0.5, 1.0, -1.0)
PRINTED_FAMILY = (0.005, 1.005, 2.675, 0.015, 0.025, 0.035, 0.045, 1.115, 8.345, 10.235, 1.015, 4.175, 16.005, 100.005, 1024.125, 2.5, 0.125, 0.375)


def values(vs, factor):
    """(bit patterns uint32 [N_VALUES], class index uint8 [N_VALUES]) of one (value size, factor): the classes of CLASSES in
    turn, `random` filling up; the first N_ALIGNED leave only random values out"""
    rng = np.random.default_rng([2015, vs, factor_index(factor)])
    f = np.float32(factor)
    steer = f if plain(factor) else np.float32(1.0)  # (a factor of 0 or NaN steers nothing: the values are those of factor 1)
    lo, hi = bounds(vs)
    out, cls = [], []

    def add(name, bits):
        bits = np.asarray(bits, dtype=np.uint32).ravel()
        out.append(bits)
        cls.append(np.full(bits.size, CLASSES.index(name), dtype=np.uint8))

    steps = np.arange(-8, 9)
    h = np.float32(0.5)
    for b in (lo, hi, lo + h, hi - h, lo - h, hi + h):  # (the last four: products that the -+ 0.5 brings onto the bound, by the factor's sign)
        add("bounds", fdiv(as_f32(neighbour(as_bits(b), steps)), steer))  # the bound and its eight neighbours either way, over the factor
        add("bounds", neighbour(fdiv(b, steer), steps))  # the floats around bound / factor

    ks = list(range(41))
    for e in range(1, 23):
        ks += [(1 << e) - 1, 1 << e, (1 << e) + 1] + [int(k) for k in rng.integers(1 << e, 2 << e, 3)]
    ks += [1 << 23, (1 << 23) + 1, (1 << 24) - 1, 1 << 24] + [int(k) for k in rng.integers(1 << 23, 1 << 24, 16)]
    half_up = np.array(ks, dtype=np.float64) + 0.5
    for sign in (1.0, -1.0):
        q = fdiv((sign * half_up).astype(np.float32), steer)
        add("ties", np.stack([neighbour(q, -1), q, neighbour(q, 1)], axis=1))

    p = np.concatenate([rng.integers(1 << 23, 1 << 24, 60), rng.integers(1 << 23, 1 << 24, 40) | 1, rng.integers(1 << 24, 1 << 25, 100)]).astype(np.float64)
    add("absorbed", fdiv((p * np.where(rng.random(p.size) < 0.5, 1.0, -1.0)).astype(np.float32), steer))

    add("specials", SPECIALS)
    add("specials", as_bits(np.array(SPECIAL_VALUES, dtype=np.float64).astype(np.float32)))

    thousandths = np.concatenate([np.round(np.array(PRINTED_FAMILY) * 1000), rng.integers(0, 10 ** 5, 140) * 10 + 5, rng.integers(0, 50, 20) * 10 + 5])
    printed = (thousandths / 1000.0).astype(np.float32)
    add("printed", as_bits(np.concatenate([printed, -printed])))

    n = N_VALUES - sum(b.size for b in out)
    assert n >= 1500, n
    # random sign and mantissa; the exponent of |v * f|: half the draws from 2^-4 up to the value size's range, half around its end
    inside = rng.random(n) < 0.5
    e = np.where(inside, rng.integers(-4, max(-3, vs - 1), n), rng.integers(vs - 1, vs + 2, n))
    x = np.ldexp(1.0 + rng.random(n), e) / abs(float(steer))
    negative = rng.random(n) < 0.5
    if vs == 1:
        negative |= inside  # (hi = 0 at one bit: a positive reading is rounded up and away from it)
    add("random", as_bits(np.where(negative, -x, x).astype(np.float32)))
    return np.concatenate(out), np.concatenate(cls)


def integers(vs, n=N_VALUES):
    """vs-bit fields (uint64 [n]) for Denormalize: the edges of the sign extension and of the conversion to float32, integers
    that lie exactly between two floats, integers of every length"""
    rng = np.random.default_rng([2016, vs])
    half = 1 << (vs - 1)
    fixed = [0, 1, -1, 2, -2, 3, -3, half - 1, -half, half - 2, 1 - half]  # (1 .. 3 over a factor of 3e38: the subnormal quotients there are)
    for m in ((1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 24) + 2, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6, (1 << 31) - 65, (1 << 31) - 64, (1 << 31) - 1,
              (1 << 31) - 128, (1 << 31) - 129, 1 << 31, (1 << 32) - 1, (1 << 53) + 1, (1 << 62) + (1 << 38), (1 << 63) - 1, (1 << 63) - (1 << 38)):
        fixed += [m, -m]
    ties = []
    for b in range(25, vs):  # integers of b bits, the bits behind the 24th exactly one half
        for _ in range(12):
            m = (1 << 23) | int(rng.integers(0, 1 << 23))
            ties.append(((m << (b - 24)) | (1 << (b - 25))) * (1 if rng.random() < 0.5 else -1))
    fixed = [m for m in fixed + ties if -half <= m < half]
    length = rng.integers(1, vs + 1, n)
    rnd = [int(rng.integers(0, 1 << 32)) << 32 | int(rng.integers(0, 1 << 32)) for _ in range(n)]
    rnd = [r & ((1 << int(k)) - 1) for r, k in zip(rnd, length)]
    vals = ([m & ((1 << vs) - 1) for m in fixed] + rnd)[:n]
    return np.array(vals, dtype=np.uint64)


# ---- channels for the fused encoder ---------------------------------------------------------------------------------------------

def stairs(vs, factor):
    """the two rows in front of a channel of negative integers (diff.c:15-18 reads the fields unsigned, so a negative integer
    is reached from 0 in two steps): the largest value at or below the upper bound, then about -(3/4) 2^(vs-1)"""
    half = 1 << (vs - 1)
    lo, hi = bounds(vs)
    top = as_f32(neighbour(as_bits(hi), -1 if float(hi) == float(half) else 0))
    cand = np.concatenate([neighbour(fdiv(top, factor), np.arange(-40, 41)), neighbour(fdiv(top - np.float32(0.5), factor), np.arange(-40, 41))])
    ok, n = normalize(cand, factor, vs)
    good = ok & (n < np.uint64(half))
    first = cand[good][np.argmax(n[good])]
    cand = neighbour(fdiv(np.float32(-0.75 * half), factor), np.arange(-2, 3))
    ok, n = normalize(cand, factor, vs)
    good = ok & (n >= np.uint64(half))
    second = cand[good][0]
    return first, second


def channels(vs, factor, T=T_ROWS):
    """(bit patterns uint32 [T, N_CHANNELS], kind per channel): `codable_positive` -- integers in [0, 2^(vs-1)); `codable_negative`
    -- the two stairs, then negative integers; `verdict:<class>@<row>` -- a codable channel with one value that Normalize
    rejects at the first, a middle or the last row"""
    assert vs >= 4 and plain(factor)
    rng = np.random.default_rng([2017, vs, factor_index(factor)])
    bits, cls = values(vs, factor)
    ok, n = normalize(bits, factor, vs)
    half = np.uint64(1 << (vs - 1))

    def deal(pool, rows, count):
        """count channels of `rows` values: every value of the pool that is not random first, the rest random ones"""
        fixed = pool[cls[pool] != CLASSES.index("random")]
        rnd = pool[cls[pool] == CLASSES.index("random")]
        order = np.concatenate([rng.permutation(fixed), rng.permutation(rnd)])
        return bits[np.resize(order, rows * count)].reshape(count, rows).T

    n_pos, n_neg, n_bad = 110, 100, 40
    pos = deal(np.flatnonzero(ok & (n < half)), T, n_pos)
    first, second = stairs(vs, factor)
    neg = np.concatenate([np.full((1, n_neg), first, dtype=np.uint32), np.full((1, n_neg), second, dtype=np.uint32),
                          deal(np.flatnonzero(ok & (n >= half)), T - 2, n_neg)], axis=0)
    # the rejected values: every infinity and bound neighbour that is out of range, then others
    bad_all = np.flatnonzero(~ok)
    inf = bad_all[np.isinf(as_f32(bits[bad_all]))]
    edge = bad_all[cls[bad_all] == CLASSES.index("bounds")]
    rest = rng.permutation(np.setdiff1d(bad_all, np.concatenate([inf, edge])))
    bad = np.concatenate([inf[:4], rng.permutation(edge)[:16], rest])[:n_bad]
    assert bad.size == n_bad
    verdict, kinds = [], ["codable_positive"] * n_pos + ["codable_negative"] * n_neg
    for row in (0, T // 2, T - 1):
        for i, b in enumerate(bad):
            col = pos[:, (7 * i + row) % n_pos].copy()
            col[row] = bits[b]
            verdict.append(col)
            kinds.append("verdict:%s@%d" % (CLASSES[cls[b]], row))
    v = np.ascontiguousarray(np.concatenate([pos, neg, np.stack(verdict, axis=1)], axis=1))
    assert v.shape == (T, N_CHANNELS)
    return v, kinds


def counts_and_poison(vs, factor, T=T_ROWS):
    """the channels of channels() that are codable, a count 1 .. T each (both ends among them), and a value that Normalize
    rejects (or a NaN) right behind every count that is short of T: (bits [T, C], count int64 [C])"""
    v, kinds = channels(vs, factor, T)
    keep = [c for c, k in enumerate(kinds) if k.startswith("codable")]
    v = np.ascontiguousarray(v[:, keep])
    rng = np.random.default_rng([2018, vs, factor_index(factor)])
    count = rng.integers(1, T + 1, len(keep))
    count[:3], count[-3:] = (1, T, 2), (T - 1, T, 1)
    poison = np.array([0x7F800000, 0xFF800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7FC00000], dtype=np.uint32)
    for c in range(len(keep)):
        v[count[c]:, c] = poison[(c + np.arange(T - count[c])) % poison.size]
    return v, count.astype(np.int64)


def series(vs, T=T_ROWS, Cn=N_CHANNELS):
    """integer series for the decoders' exit, as vs-bit fields uint64 [T, Cn]: from 0 in steps that diff.c:15-18 accepts to the
    next value of integers(vs) -- a staircase up to the upper half, then samples over the whole range; the last two channels swing
    between 0 and the largest value instead"""
    pool = [int(x) for x in integers(vs)]
    half, full = 1 << (vs - 1), 1 << vs
    out = np.zeros((T, Cn), dtype=np.uint64)
    at = 0
    for c in range(Cn):
        rows, cur = [], 0
        while len(rows) < T:
            t = pool[at % len(pool)]
            at += 1
            if vs < 64:
                while t - cur > half - 1:
                    cur += half - 1
                    rows.append(cur)
                while t - cur < -half:
                    cur -= half
                    rows.append(cur)
            rows.append(t)
            cur = t
        assert all(0 <= r < full for r in rows)
        out[:, c] = rows[:T]
    # two channels whose every codeword is of the longest kind (2 min(vs, 63) + 1 bits, seg.c:55-56,74): the largest steps either way
    peak = half - 1 if vs < 64 else (1 << 62) + 12345
    out[:, Cn - 2] = [peak if t % 2 == 0 else 0 for t in range(T)]
    out[:, Cn - 1] = [peak if t % 2 == 1 else 1 for t in range(T)]
    return out


# ---- the oracle's chains -------------------------------------------------------------------------------------------------------

def pack_fields(vals, vs):
    """unsigned values as vs-bit big-endian fields -> (bytes, nbits): what a stage reads with valuesize=vs"""
    acc = 0
    for x in vals:
        acc = (acc << vs) | int(x)
    n = len(vals) * vs
    return (acc << (-n % 8)).to_bytes((n + 7) // 8, "big"), n


def unpack_fields(data, nbits, vs):
    acc = int.from_bytes(data[: (nbits + 7) // 8], "big") >> (-nbits % 8)
    k = nbits // vs
    return np.array([(acc >> (vs * (k - 1 - i))) & ((1 << vs) - 1) for i in range(k)], dtype=np.uint64)


def encode_chain(col_bits, vs, ad, factor):
    """one channel of float32 bit patterns through the oracle's normalize -> diff -> seg -> bac: (status, stream, bits)"""
    data, n = np.ascontiguousarray(col_bits, dtype=np.uint32).tobytes(), 32 * len(col_bits)
    for name in ("normalize", "diff", "seg", "bac"):
        r, data, n = orc.stage(name, True, data, n, valuesize=vs, adaptive=ad, factor=factor)
        if r != 0:
            return r, b"", 0
    return 0, data[: (n + 7) // 8], n


def decode_chain(data, n, vs, ad, factor):
    """the inverse: (status, float32 bit patterns)"""
    for name in ("bac", "seg", "diff", "normalize"):
        r, data, n = orc.stage(name, False, data, n, valuesize=vs, adaptive=ad, factor=factor)
        if r != 0:
            return r, np.zeros(0, dtype=np.uint32)
    return 0, np.frombuffer(data[: n // 8], dtype=np.uint32).copy()


def integer_chain(fields, vs, ad):
    """one channel of vs-bit fields through the oracle's diff -> seg -> bac: (status, stream, bits)"""
    data, n = pack_fields(fields, vs)
    for name in ("diff", "seg", "bac"):
        r, data, n = orc.stage(name, True, data, n, valuesize=vs, adaptive=ad)
        if r != 0:
            return r, b"", 0
    return 0, data[: (n + 7) // 8], n


def stream_cap(T, vs):
    return 4 * ((T * (2 * vs + 3) // 4 + 64) // 4 + 4)  # (bytes: room for the static model's log2(3) bits per seg bit)


class Expected:
    """what the oracle makes of a batch [T, C] of float32 bit patterns, column by column (count: only the first count[c] rows
    of column c): err int32 [C], bits uint64 [C], streams (list of bytes), and the floats its inverse chain gives back"""

    def __init__(self, v_bits, vs, ad, factor, count=None):
        T, Cn = v_bits.shape
        self.T, self.cap = T, stream_cap(T, vs)
        self.err = np.zeros(Cn, dtype=np.int32)
        self.bits = np.zeros(Cn, dtype=np.uint64)
        self.streams, self.back = [], []
        for c in range(Cn):
            col = v_bits[: (T if count is None else int(count[c])), c]
            r, data, n = encode_chain(col, vs, ad, factor)
            self.err[c], self.bits[c] = r, n
            self.streams.append(data)
            back = np.zeros(0, dtype=np.uint32)
            if r == 0:
                rb, back = decode_chain(data, n, vs, ad, factor)
                assert rb == 0 and back.size == col.size
            self.back.append(back)

    def slabs(self):
        """the streams as the decoders take them; a channel in error has an empty stream"""
        slabs = np.zeros((len(self.streams), self.cap), dtype=np.uint8)
        for c, st in enumerate(self.streams):
            slabs[c, : len(st)] = np.frombuffer(st, dtype=np.uint8)
        return slabs, np.where(self.err == 0, self.bits, 0).astype(np.uint64)

    def check_streams(self, out, bits, err, what, kinds=None):
        out, bits, err = np.asarray(out), np.asarray(bits), np.asarray(err)
        for c in range(len(self.streams)):
            name = (what, c, kinds[c] if kinds else "")
            assert int(err[c]) == int(self.err[c]), (name, "status", int(err[c]), int(self.err[c]))
            if self.err[c] == 0:
                assert int(bits[c]) == int(self.bits[c]), (name, "bits", int(bits[c]), int(self.bits[c]))
                assert out[c, : len(self.streams[c])].tobytes() == self.streams[c], (name, "stream")

    def check_back(self, back, derr, what, kinds=None):
        """back: float32 [T, C] (or its bit patterns) from a decoder that was given slabs()"""
        back = np.ascontiguousarray(back).view(np.uint32)
        for c in range(len(self.streams)):
            if self.err[c] == 0:
                name = (what, c, kinds[c] if kinds else "")
                k = self.back[c].size
                assert int(derr[c]) == 0, (name, int(derr[c]))
                same = same_float_bits(back[:k, c], self.back[c])
                assert same.all(), (name, int(np.flatnonzero(~same)[0]), hex(int(back[:k, c][~same][0])), hex(int(self.back[c][~same][0])))


_EXPECTED = {}


def expected_channels(vs, factor, ad):
    """channels(vs, factor) and the oracle's answer, computed once: (bits [T, C], kinds, Expected)"""
    k = (vs, factor, ad)
    if k not in _EXPECTED:
        v, kinds = channels(vs, factor)
        _EXPECTED[k] = (v, kinds, Expected(v, vs, ad, factor))
    return _EXPECTED[k]


class ExpectedSeries:
    """series(vs) through the oracle: the streams of its diff -> seg -> bac, and what Denormalize makes of the integers -- by
    the restatement and by the oracle's stage, which have to agree"""

    def __init__(self, vs, ad, factor):
        self.fields = series(vs)
        T, Cn = self.fields.shape
        self.T, self.cap = T, stream_cap(T, vs)
        self.slabs = np.zeros((Cn, self.cap), dtype=np.uint8)
        self.bits = np.zeros(Cn, dtype=np.uint64)
        self.back = denormalize(self.fields.ravel(), factor, vs).reshape(T, Cn)
        assert same_float_bits(self.back, as_bits(orc.denormalize_each(self.fields.ravel(), factor, vs)).reshape(T, Cn)).all()
        for c in range(Cn):
            r, data, n = integer_chain(self.fields[:, c], vs, ad)
            assert r == 0, (vs, c, r)
            self.slabs[c, : len(data)] = np.frombuffer(data, dtype=np.uint8)
            self.bits[c] = n

    def check_back(self, back, derr, what):
        back = np.ascontiguousarray(back).view(np.uint32)
        assert (np.asarray(derr) == 0).all(), what
        same = same_float_bits(back, self.back)
        assert same.all(), (what, [(int(t), int(c), hex(int(self.fields[t, c])), hex(int(back[t, c])), hex(int(self.back[t, c]))) for t, c in np.argwhere(~same)[:4]])


_SERIES = {}


def expected_series(vs, ad, factor):
    k = (vs, ad, factor)
    if k not in _SERIES:
        _SERIES[k] = ExpectedSeries(vs, ad, factor)
    return _SERIES[k]


# ---- one chain from text ---------------------------------------------------------------------------------------------------------

TEXT_LINES = (
    [b"12.34", b"12.50", b"13.01", b"12.99", b"0.00", b"7405.30"],
    [b"1.00", b"2.00", b"nan", b"3.00"],
    [b"5.25", b"-nan", b"5.50", b"nan", b"-nan"],
    [b"3.00", b"inf", b"4.00"],
    [b"0.50", b"1e-40", b"-1e-40", b"0.75"],
    [b"9.99", b"abc", b"10.01", b"-", b"10.02"],
    [b"nan", b"nan", b"2.50"],
    [b"8.00", b"8.25", b"-inf"],
    [b"21474836.48"],
    [b"21474837", b"1.00"],
)
TEXT_SIZES = (32, 64)


def text_chain_stages(vs, ad):
    opt = " valuesize=%d" % vs
    return ["decode csv", "encode normalize normalization_factor=100.0" + opt, "encode diff" + opt, "encode seg" + opt, "encode bac" + (" adaptive" if ad else "")]


# ---- conditions ------------------------------------------------------------------------------------------------------------------

def conditions(vs, factor):
    """what the corpus of (vs, factor) has to hold to be worth running, from the restatement and the oracle alone; a list of
    the conditions that are not met (empty: all are)"""
    missed = []
    bits, cls = values(vs, factor)
    p, w = rounded(bits, factor)
    ok, n = normalize(bits, factor, vs)
    lo, hi = bounds(vs)
    of = lambda name: cls == CLASSES.index(name)  # noqa: E731
    if bits.size != N_VALUES or not of("random")[N_ALIGNED:].all():
        missed.append("sizes")
    if plain(factor):
        r = of("random")
        if ok[r].mean() < 0.2 or (~ok[r]).mean() < 0.2:
            missed.append("random: %.2f in range" % ok[r].mean())
        with np.errstate(invalid="ignore"):
            b = of("bounds")
            sides = [(w[b] < lo).any(), (ok[b] & (w[b] <= lo + 1)).any(), (w[b] > hi).any(), (ok[b] & (w[b] >= hi - 1)).any()]
        if not all(sides):
            missed.append("bounds: sides %s" % sides)
        if vs >= 26 and not (ok & of("bounds") & (w == hi)).any():
            missed.append("bounds: no value passes the check and wraps")
        exact = p.astype(np.float64) + np.where(as_f32(bits) > 0, 0.5, -0.5)
        a = of("absorbed")
        if int((w[a].astype(np.float64) != exact[a]).sum()) < 50:
            missed.append("absorbed: %d inexact adds" % int((w[a].astype(np.float64) != exact[a]).sum()))
    if factor in (1.0, 0.5):
        t = of("ties")
        frac = np.abs(p[t].astype(np.float64)) % 1.0
        if int((frac == 0.5).sum()) < 200:
            missed.append("ties: %d products on k + 0.5" % int((frac == 0.5).sum()))
    if vs > 32:
        k = sum(conversion_tie(int(s)) for s in sign_extend(series(vs).ravel(), vs))
        if k < 100:
            missed.append("series: %d conversion ties" % k)
    if (vs, factor) in FUSED:
        for ad in (1, 0):
            _, kinds, want = expected_channels(vs, factor, ad)
            for c, kind in enumerate(kinds):
                if (want.err[c] == 0) != kind.startswith("codable"):
                    missed.append("channel %d (%s, model %d): oracle status %d" % (c, kind, ad, want.err[c]))
    return missed


# ---- the fixture -----------------------------------------------------------------------------------------------------------------

def save_npz(path, arrays):
    """np.savez_compressed with fixed time stamps and order: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            with z.open(info, "w") as fh:
                np.lib.format.write_array(fh, np.ascontiguousarray(arrays[name]), version=(1, 0), allow_pickle=False)


def crc(a):
    return np.uint32(zlib.crc32(np.ascontiguousarray(a).tobytes()))


class EdgeFixture:
    """float_edges.npz -- what the compiled reference returned.  Per (value size, factor) `k` = key(vs, factor):
      <k>.in         uint32      crc32 of values(vs, factor): the values the reference was given are the ones computed here
      <k>.status     uint8 [N]   `encode normalize` of every value alone failed (packed bits), xor the restatement's verdict
      <k>.int        uint64 [N]  the field it wrote (0 with a failure), xor the restatement's
      <k>.den.in     uint32      crc32 of integers(vs)
      <k>.den        uint32 [N]  `decode normalize` of integers(vs), xor the restatement's (a NaN for a NaN stored as 0)
      <k>.lit.*                  for factors 100 and 1 the classes `bounds` and `specials` once more in full: in, status, int
      <k>.<ad|st>.chain.*        a thin sample of channels(vs, factor) through the whole chain and back: idx, err, bits, stream,
                                 back (xor the restatement's Denormalize of its Normalize)
      text.*                     TEXT_LINES through `decode csv # encode normalize # ...` at TEXT_SIZES
    The xor arrays are zero wherever the restatement is right, which keeps the file small; test_fixture_is_not_blind names
    entries literally."""

    def __init__(self):
        self.z = np.load(FIXTURE)

    def has(self, name):
        return name in self.z.files

    def normalized(self, vs, factor):
        """(failed bool [N], fields uint64 [N]) as the reference returned them"""
        k = key(vs, factor)
        bits, _ = values(vs, factor)
        assert crc(bits) == self.z[k + ".in"], "the corpus of %s is not the one the fixture was made from" % k
        ok, n = normalize(bits, factor, vs)
        failed = np.unpackbits(self.z[k + ".status"])[: bits.size].astype(bool) ^ ~ok
        return failed, self.z[k + ".int"] ^ n

    def denormalized(self, vs, factor):
        k = key(vs, factor)
        u = integers(vs)
        assert crc(u) == self.z[k + ".den.in"], "the integers of %s are not the ones the fixture was made from" % k
        return self.z[k + ".den"] ^ denormalize(u, factor, vs)
