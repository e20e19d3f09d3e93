"""Shared by tests/test_axdr_host.py (the emulator of tests/sim/), tests/test_gpu_axdr.py (the C ABI) and
tests/golden/make_golden_axdr.py: A-XDR, every reading one big-endian field of `valuesize` bits, packed MSB first
(normalize.c:9-41), as dega_axdr_pack_kernel / dega_axdr_unpack_kernel (csrc/axdr_kernels.hpp) make and read it.

Expectations.  Float entry and exit: the oracle's stage, orc.stage("normalize", ...), per channel -- status, bit length and
every byte, or every float bit (same_float_bits).  Integer entries: pack_channel / unpack_channel below, plain numpy, tied to
the oracle in the host tests on fields that floats with factor 1 reach exactly, and to the compiled reference through
tests/golden/axdr.npz.  Everything is compared exactly and no channel is excused.

A case is a function of a backend `B` (the two test files have one each):
  B.buf(array, offset=0)   the array's bytes in memory of the backend's, `offset` bytes behind a 16-byte boundary
  B.ptr(h) / B.get(h)      its address / its bytes back (numpy uint8)
  B.pack(...) / B.unpack(...)   the entry points, arguments as the C ABI's without context and stream, addresses as integers;
                           they return the call's status.  `wide` / `gx_max` steer the emulator only (the 16-byte form on the
                           rows' side forced on or off, the tile index split over x and y); the library chooses by itself."""
import functools
import os

import numpy as np

import float_edges_common as fe
from oracle import orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "axdr.npz")

F32, I32, I64 = 0, 1, 2  # the kinds of rows: DEGA_SAMPLES_F32 = 3, _I32 = 0, _I64 = 2 in the C ABI
SAMPLES = {F32: 3, I32: 0, I64: 2}
OK, INVALID_VALUE, MEMORY, LIBRARY_CALL = 0, -1, -6, -11
R = 128  # the kernels' tile rows at value sizes 1..32; 64 at 33..64 (AX_ROWS; the host test holds sim_axdr_rows to both)
R_WIDE = 64
SIZES_4 = (1, 2, 3, 7, 8, 12, 16, 17, 24, 31, 32)
SIZES_8 = (33, 47, 63, 64)
SIZES = SIZES_4 + SIZES_8
CHANNELS = (1, 63, 64, 65, 130)
# 0, 1, 31, 32, 33, R - 1, R, R + 1, 2 R + 44 for both tile heights
ROWS = (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 172, 300)
FACTORS = (100.0, 1.0, 3.3, -100.0)
CANARY = 0xC5
POISON = np.array([0x7FC00000, 0x7F800000, 0xFF800000, 0x7F61B1E6], dtype=np.uint32)  # NaN, +-inf, 3e38: what lies behind a count


def kind_of(vs):
    return I32 if vs <= 32 else I64


def elem(kind):
    return np.dtype(np.int64) if kind == I64 else np.dtype(np.uint32)


def axdr_bytes(T, vs):
    return 4 * ((T * vs + 31) // 32)


# ---- the plain pack ------------------------------------------------------------------------------------------------------------

def pack_channel(col, vs):
    """fields (uint64 [n], the low vs bits) -> (the stream zero padded to whole 32-bit words, its bits)"""
    col = np.ascontiguousarray(col, dtype=np.uint64)
    if col.size == 0:
        return b"", 0
    shifts = np.arange(vs - 1, -1, -1, dtype=np.uint64)
    bits = ((col[:, None] >> shifts[None, :]) & np.uint64(1)).astype(np.uint8).ravel()
    data = np.packbits(bits).tobytes()
    return data + b"\0" * (-len(data) % 4), col.size * vs


def unpack_channel(data, nbits, vs):
    """the whole fields of a stream of nbits bits: uint64 [nbits // vs]"""
    k = nbits // vs
    if k == 0:
        return np.zeros(0, dtype=np.uint64)
    bits = np.unpackbits(np.frombuffer(bytes(data), dtype=np.uint8))[: k * vs].reshape(k, vs).astype(np.uint64)
    shifts = np.arange(vs - 1, -1, -1, dtype=np.uint64)
    return (bits << shifts[None, :]).sum(axis=1, dtype=np.uint64)  # (disjoint bits: the sum is their union)


# ---- the corpus ------------------------------------------------------------------------------------------------------------------

def mask(vs):
    return np.uint64((1 << vs) - 1)


@functools.lru_cache(maxsize=None)
def fields(vs, T, Cn, seed=0):
    """uint64 [T, Cn] over the full range of the value size; in every channel (as far as its rows reach) -2^(vs-1),
    2^(vs-1) - 1, -1, 0 and the two alternating patterns, each at a row of its own that moves from channel to channel"""
    rng = np.random.default_rng([2031, vs, T, Cn, seed])
    f = (rng.integers(0, 1 << 32, (T, Cn), dtype=np.uint64) << np.uint64(32) | rng.integers(0, 1 << 32, (T, Cn), dtype=np.uint64)) & mask(vs)
    special = [1 << (vs - 1), (1 << (vs - 1)) - 1, (1 << vs) - 1, 0, 0xAAAAAAAAAAAAAAAA & ((1 << vs) - 1), 0x5555555555555555 & ((1 << vs) - 1)]
    for c in range(Cn):
        for k, s in enumerate(special):
            if T:
                f[(5 * c + 11 * k) % T if T > 6 else (c + k) % T, c] = np.uint64(s)
    f.setflags(write=False)
    return f


def containers(f, vs, junk=True):
    """the fields in int32 / int64 containers, with set bits above the value size where there is room"""
    kind = kind_of(vs)
    width = 64 if kind == I64 else 32
    x = f.copy()
    if junk and vs < width:
        rng = np.random.default_rng([2032, vs])
        x |= (rng.integers(0, 1 << 32, f.shape, dtype=np.uint64) << np.uint64(32) | rng.integers(0, 1 << 32, f.shape, dtype=np.uint64)) << np.uint64(vs)
    return x.view(np.int64) if kind == I64 else (x & np.uint64(0xFFFFFFFF)).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def float_rows(vs, factor, T, Cn):
    """float32 bit patterns uint32 [T, Cn] that Normalize accepts: the codable channels of float_edges_common.channels(vs,
    factor) -- bounds and their neighbours, ties, NaNs, subnormals -- one below the other as far as T asks"""
    v, kinds = fe.channels(vs, factor)
    good = v[:, [c for c, k in enumerate(kinds) if k.startswith("codable")]]
    rng = np.random.default_rng([2033, vs, T, Cn])
    blocks = [good[:, rng.permutation(good.shape[1])[np.arange(Cn) % good.shape[1]]] for _ in range(T // good.shape[0] + 1)]
    out = np.ascontiguousarray(np.concatenate(blocks, axis=0)[:T])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rejected(vs, factor):
    """float32 bit patterns that Normalize rejects at (vs, factor): infinities, bound neighbours, 3e38"""
    bits, _ = fe.values(vs, factor)
    ok, _ = fe.normalize(bits, factor, vs)
    bad = bits[~ok]
    assert bad.size >= 8
    return bad


def oracle_pack(col_bits, vs, factor):
    """one channel of float32 bit patterns through the oracle's `encode normalize`: (status, stream padded to words, bits)"""
    col = np.ascontiguousarray(col_bits, dtype=np.uint32)
    r, data, n = orc.stage("normalize", True, col.tobytes(), 32 * col.size, valuesize=vs, factor=factor)
    if r != 0:
        return r, b"", 0
    data = data[: (n + 7) // 8]
    return 0, data + b"\0" * (-len(data) % 4), n


def oracle_unpack(data, nbits, vs, factor):
    """a stream through the oracle's `decode normalize`: (status, float32 bit patterns)"""
    r, out, n = orc.stage("normalize", False, data, nbits, valuesize=vs, factor=factor)
    if r != 0:
        return r, np.zeros(0, dtype=np.uint32)
    return 0, np.frombuffer(out[: n // 8], dtype=np.uint32).copy()


# ---- one call ----------------------------------------------------------------------------------------------------------------------

def image(B, logical, pitch, fill, offset):
    """[rows][pitch] with `fill` beside the logical columns, `offset` bytes off a 16-byte boundary -> its handle"""
    rows, used = logical.shape
    full = np.full((rows, pitch), fill, dtype=logical.dtype)
    full[:, :used] = logical
    return B.buf(full, offset)


class Packed:
    """the outputs of one pack call: slabs uint8 [C, cap], bits uint64 [C], err int32 [C]"""

    def __init__(self, slabs, bits, err):
        self.slabs, self.bits, self.err = slabs, bits, err


def run_pack(B, rows, kind, vs, factor=100.0, count=None, ld=None, x_offset=0, cap=None, slab_offset=0, wide=-1, gx_max=1 << 24, status=OK):
    """rows: the logical [T, C] image (uint32 float bits / uint32 / int64).  The slabs are canaries before the call; the
    columns beside the image hold NaN bits (floats) or all ones."""
    T, Cn = rows.shape
    ld = Cn if ld is None else ld
    cap = axdr_bytes(T, vs) if cap is None else cap
    fill = 0x7FC00001 if kind == F32 else -1 if kind == I64 else 0xFFFFFFFF
    x = image(B, np.ascontiguousarray(rows, dtype=elem(kind)), ld, fill, x_offset)
    slabs = B.buf(np.full(Cn * cap + 16, CANARY, dtype=np.uint8), slab_offset)
    bits = B.buf(np.full(Cn, 0x7777777777777777, dtype=np.uint64))
    err = B.buf(np.full(Cn, 77, dtype=np.int32))
    cnt = None if count is None else B.buf(np.ascontiguousarray(count, dtype=np.uint64))
    ret = B.pack(B.ptr(x), kind, Cn, T, ld, 0 if cnt is None else B.ptr(cnt), factor, vs, B.ptr(slabs), cap, B.ptr(bits), B.ptr(err), wide, gx_max)
    assert ret == status, ("pack", ret, vs, Cn, T)
    raw = B.get(slabs)
    assert (raw[Cn * cap:] == CANARY).all(), ("written behind the last slab", vs, Cn, T)
    assert (B.get(x) == np.frombuffer(B.initial(x), dtype=np.uint8)).all(), "the rows were written"
    return Packed(raw[: Cn * cap].reshape(Cn, cap), B.get(bits).view(np.uint64), B.get(err).view(np.int32))


def check_packed(got, want, what):
    """want: per channel (status, stream padded to words, bits).  Status; where it is 0 the bit length and every byte; every
    byte behind the stream's last word a canary (a channel in error that wrote nothing: all of them)"""
    for c, (status, data, nbits) in enumerate(want):
        name = (what, c)
        assert int(got.err[c]) == status, (name, "status", int(got.err[c]), status)
        if status == OK:
            assert int(got.bits[c]) == nbits, (name, "bits", int(got.bits[c]), nbits)
            assert len(data) <= got.slabs.shape[1], (name, "the expectation does not fit the slab")
            assert got.slabs[c, : len(data)].tobytes() == data, (name, "stream", np.flatnonzero(got.slabs[c, : len(data)] != np.frombuffer(data, np.uint8))[:4])
            assert (got.slabs[c, len(data):] == CANARY).all(), (name, "written behind the stream")
        elif status == MEMORY or nbits == 0:
            assert int(got.bits[c]) == 0, (name, "bits of a channel that was not packed", int(got.bits[c]))
            assert (got.slabs[c] == CANARY).all(), (name, "a channel that was not packed was written")


def want_int(f, vs, count=None, cap=None):
    T, Cn = f.shape
    out = []
    for c in range(Cn):
        n = T if count is None else int(count[c])
        if n > T:
            out.append((INVALID_VALUE, b"", 0))
        elif cap is not None and axdr_bytes(n, vs) > cap:
            out.append((MEMORY, b"", 0))
        else:
            out.append((OK,) + pack_channel(f[:n, c], vs))
    return out


def want_float(v, vs, factor, count=None, cap=None):
    T, Cn = v.shape
    out = []
    for c in range(Cn):
        n = T if count is None else int(count[c])
        if n > T:
            out.append((INVALID_VALUE, b"", 0))
        elif cap is not None and axdr_bytes(n, vs) > cap:
            out.append((MEMORY, b"", 0))
        else:
            r, data, nb = oracle_pack(v[:n, c], vs, factor)
            out.append((r, data, nb if r == 0 else -1))  # (-1: the reference stopped inside the channel; its bytes are not defined)
    return out


# ---- pack cases ------------------------------------------------------------------------------------------------------------------

def case_pack_int(B, vs, Cn, T, pitch_case=0, wide=-1, gx_max=1 << 24):
    """pitch_case 0: ld = C, bases aligned; 1: ld = C + 7, the rows' base one element off (the element load form), cap no
    multiple of 16 and the slabs' base 4 bytes off"""
    f = fields(vs, T, Cn)
    kind = kind_of(vs)
    esz = elem(kind).itemsize
    cap = axdr_bytes(T, vs)
    if pitch_case:
        cap += 4 if (cap + 4) % 16 else 8
    got = run_pack(B, containers(f, vs), kind, vs, ld=Cn + 7 * pitch_case, x_offset=esz * pitch_case, cap=cap, slab_offset=4 * pitch_case, wide=wide, gx_max=gx_max)
    check_packed(got, want_int(f, vs), ("pack int", vs, Cn, T, pitch_case, wide))


def case_pack_float(B, vs, factor, Cn, T, pitch_case=0, wide=-1):
    v = float_rows(vs, factor, T, Cn)
    got = run_pack(B, v, F32, vs, factor, ld=Cn + 7 * pitch_case, x_offset=4 * pitch_case, wide=wide)
    want = want_float(v, vs, factor)
    assert all(w[0] == OK for w in want)
    check_packed(got, want, ("pack float", vs, factor, Cn, T, pitch_case, wide))


def refusal_rows(T, tile_rows):
    return sorted({r for r in (0, 31, 32, tile_rows, T - 1) if r < T})


def case_refusals(B, vs, factor, Cn=130, T=300):
    """one reading that Normalize rejects at row 0, 31, 32, R or T - 1 of a single channel, healthy neighbours on both sides in
    the same wave; the same readings behind a count refuse nothing"""
    v = float_rows(vs, factor, T, Cn).copy()
    bad = rejected(vs, factor)
    rows = refusal_rows(T, R if vs <= 32 else R_WIDE)
    where = {}
    for k, r in enumerate(rows):
        c = 3 + 13 * k  # (channels 3, 16, 29, 42, 55: one wave, neighbours between them)
        v[r, c] = bad[k % bad.size]
        where[c] = r
    got = run_pack(B, v, F32, vs, factor)
    want = want_float(v, vs, factor)
    assert sorted(c for c, w in enumerate(want) if w[0] != OK) == sorted(where), "the oracle refuses exactly the channels that were spoilt"
    assert all(want[c][0] == INVALID_VALUE for c in where)
    check_packed(got, want, ("refusals", vs, factor))
    count = np.full(Cn, T, dtype=np.uint64)
    for c, r in where.items():
        count[c] = r  # the spoilt reading is the first one behind the count
    got = run_pack(B, v, F32, vs, factor, count=count)
    want = want_float(v, vs, factor, count)
    assert all(w[0] == OK for w in want)
    check_packed(got, want, ("refusals behind a count", vs, factor))


def counts_for(Cn, T):
    pool = [n for n in (0, 1, 31, 32, 33, T - 1, T, T + 1) if n >= 0]
    return np.array([pool[c % len(pool)] for c in range(Cn)], dtype=np.uint64)


def case_counts(B, vs, Cn, T, floats, factor=100.0, short_cap=False, wide=-1):
    """count[c] in {0, 1, 31, 32, 33, T - 1, T, T + 1}, NaN, infinity and 3e38 behind every count: each channel is the uniform
    call on that channel alone with T = count[c].  short_cap: the slabs four bytes short of T fields -- DEGA_ERROR_MEMORY for
    the channels that need them all, the neighbours exact"""
    count = counts_for(Cn, T)
    cap = axdr_bytes(T, vs) - (4 if short_cap else 0)
    if floats:
        v = float_rows(vs, factor, T, Cn).copy()
        for c in range(Cn):
            n = min(int(count[c]), T)
            v[n:, c] = POISON[(c + np.arange(T - n)) % POISON.size]
        got = run_pack(B, v, F32, vs, factor, count=count, cap=cap, wide=wide)
        want = want_float(v, vs, factor, count, cap)
    else:
        f = fields(vs, T, Cn, 1)
        x = containers(f, vs)
        got = run_pack(B, x, kind_of(vs), vs, count=count, cap=cap, wide=wide)
        want = want_int(f, vs, count, cap)
    if short_cap and T:
        assert any(w[0] == MEMORY for w in want) and any(w[0] == OK for w in want)
    assert all(w[0] in (OK, MEMORY) or int(count[c]) > T for c, w in enumerate(want))
    check_packed(got, want, ("counts", vs, Cn, T, floats, short_cap))


# ---- unpack cases ----------------------------------------------------------------------------------------------------------------

class Unpacked:
    def __init__(self, x, count, err):
        self.x, self.count, self.err = x, count, err


def run_unpack(B, streams, in_bits, vs, kind, max_T, factor=100.0, ld=None, x_offset=0, cap=None, wide=-1, gx_max=1 << 24, behind=None):
    """streams: per channel the bytes of its slab's head; the rest of a slab is `behind` (random bytes by default: what lies
    behind a stream is not the stream's).  The rows are [max_T + 1][ld] of canaries before the call: columns C .. ld - 1 and
    row max_T must keep them."""
    Cn = len(streams)
    ld = Cn if ld is None else ld
    cap = max([4] + [(len(s) + 3) // 4 * 4 for s in streams]) if cap is None else cap
    rng = np.random.default_rng([2034, vs, Cn, max_T])
    slabs = rng.integers(0, 256, (Cn, cap), dtype=np.uint8) if behind is None else np.full((Cn, cap), behind, dtype=np.uint8)
    for c, s in enumerate(streams):
        head = np.frombuffer(bytes(s), dtype=np.uint8)[:cap]
        whole = int(in_bits[c]) // 8
        slabs[c, : min(whole, head.size)] = head[: min(whole, head.size)]
        if int(in_bits[c]) % 8 and whole < head.size:  # the stream's last bits, random bits behind them in the same byte
            keep = 0xFF00 >> (int(in_bits[c]) % 8) & 0xFF
            slabs[c, whole] = (int(head[whole]) & keep) | (int(slabs[c, whole]) & (0xFF ^ keep))
    dt = np.dtype(np.int64) if kind == I64 else np.dtype(np.uint32)
    canary = np.full((max_T + 1, ld), 0x5A5A5A5A5A5A5A5A & ((1 << 8 * dt.itemsize) - 1), dtype=np.uint64).astype(dt) if dt.itemsize == 4 else \
        np.full((max_T + 1, ld), 0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    x = B.buf(canary, x_offset)
    s = B.buf(slabs)
    bits = B.buf(np.ascontiguousarray(in_bits, dtype=np.uint64))
    count = B.buf(np.full(Cn, 0x7777777777777777, dtype=np.uint64))
    err = B.buf(np.full(Cn, 77, dtype=np.int32))
    ret = B.unpack(B.ptr(s), cap, B.ptr(bits), Cn, max_T, ld, factor, vs, kind, B.ptr(x), B.ptr(count), B.ptr(err), wide, gx_max)
    assert ret == OK, ("unpack", ret)
    got = B.get(x).view(dt).reshape(max_T + 1, ld)
    assert (got[:, Cn:] == canary[:, Cn:]).all(), "columns C .. ld - 1 were written"
    assert (got[max_T] == canary[max_T]).all(), "row max_T was written"
    return Unpacked(got[:max_T, :Cn], B.get(count).view(np.uint64), B.get(err).view(np.int32))


def check_unpacked(got, want, kind, what):
    """want: per channel (status, count, values) -- float32 bit patterns or fields"""
    for c, (status, count, values) in enumerate(want):
        name = (what, c)
        assert int(got.err[c]) == status, (name, "status", int(got.err[c]), status)
        if status == OK:
            assert int(got.count[c]) == count, (name, "count", int(got.count[c]), count)
            col = got.x[:count, c]
            if kind == F32:
                same = fe.same_float_bits(col, values)
                assert same.all(), (name, int(np.flatnonzero(~same)[0]), hex(int(col[~same][0])), hex(int(values[~same][0])))
            else:
                assert (col.view(np.uint64 if kind == I64 else np.uint32) == values.astype(np.uint64 if kind == I64 else np.uint32)).all(), (name, "fields")


def want_unpack(streams, in_bits, vs, kind, max_T, factor):
    out = []
    for s, nb in zip(streams, in_bits):
        nb = int(nb)
        if kind == F32:
            r, vals = oracle_unpack(bytes(s)[: (nb + 7) // 8], nb, vs, factor)
        else:
            r, vals = (OK if nb % vs == 0 else LIBRARY_CALL), unpack_channel(s, nb, vs)
        if r == OK and vals.size > max_T:
            r = MEMORY
        out.append((r, vals.size, vals))
    return out


@functools.lru_cache(maxsize=None)
def oracle_streams(vs, factor, T, Cn):
    """the oracle's `encode normalize` of float_rows(vs, factor, T, Cn): per channel (stream, bits)"""
    v = float_rows(vs, factor, T, Cn)
    out = []
    for c in range(Cn):
        r, data, n = oracle_pack(v[:, c], vs, factor)
        assert r == 0 and n == T * vs
        out.append((data, n))
    return out


def int_streams(vs, T, Cn):
    f = fields(vs, T, Cn, 2)
    return [pack_channel(f[:, c], vs) for c in range(Cn)]


def case_unpack(B, vs, Cn, T, kind, factor=100.0, how="exact", pitch_case=0, wide=-1, gx_max=1 << 24):
    """how: "exact" bit lengths; "file" -- in_bits = 8 bytes of the file form (a phantom field, or -11); "zero"; "short" --
    max_T one too small for the channels that hold T fields"""
    coded = oracle_streams(vs, factor, T, Cn) if kind == F32 and vs >= 4 else int_streams(vs, T, Cn)
    streams = [d for d, _ in coded]
    in_bits = np.array([n for _, n in coded], dtype=np.uint64)
    max_T = T
    if how == "file":
        in_bits = (in_bits + np.uint64(7)) // np.uint64(8) * np.uint64(8)
        max_T = T + 8
    elif how == "zero":
        in_bits[:] = 0
    elif how == "short":
        in_bits = np.array([n if c % 3 else max(T - 1, 0) * vs for c, n in enumerate(in_bits)], dtype=np.uint64)
        max_T = max(T - 1, 0)
    esz = 8 if kind == I64 else 4
    got = run_unpack(B, streams, in_bits, vs, kind, max_T, factor, ld=Cn + 7 * pitch_case, x_offset=esz * pitch_case, wide=wide, gx_max=gx_max)
    want = want_unpack(streams, in_bits, vs, kind, max_T, factor)
    if how == "short" and T:
        assert all((w[0] == MEMORY) == (c % 3 != 0) for c, w in enumerate(want))
    check_unpacked(got, want, kind, ("unpack", vs, Cn, T, kind, factor, how, pitch_case, wide))


def case_unpack_cuts(B, vs, kind, factor=100.0):
    """one stream cut to every length from 0 to 2 vs + 1 bits, a channel per length"""
    T = 3
    data, n = (oracle_streams(vs, factor, T, 1) if kind == F32 and vs >= 4 else int_streams(vs, T, 1))[0]
    in_bits = np.arange(0, 2 * vs + 2, dtype=np.uint64)
    streams = [data] * in_bits.size
    got = run_unpack(B, streams, in_bits, vs, kind, T, factor)
    want = want_unpack(streams, in_bits, vs, kind, T, factor)
    assert [w[0] for w in want] == [OK if int(b) % vs == 0 else LIBRARY_CALL for b in in_bits]
    check_unpacked(got, want, kind, ("cuts", vs, kind, factor))


def case_round_trip(B, vs, factor, Cn, T):
    """unpack(pack(v)) is the oracle's `decode normalize` of its `encode normalize`"""
    v = float_rows(vs, factor, T, Cn)
    packed = run_pack(B, v, F32, vs, factor)
    assert (packed.err == 0).all()
    got = run_unpack(B, [packed.slabs[c].tobytes() for c in range(Cn)], packed.bits, vs, F32, T, factor, behind=CANARY)
    want = []
    for c in range(Cn):
        data, n = oracle_streams(vs, factor, T, Cn)[c]
        r, vals = oracle_unpack(data, n, vs, factor)
        want.append((r, vals.size, vals))
    check_unpacked(got, want, F32, ("round trip", vs, factor, Cn, T))


# ---- index width -------------------------------------------------------------------------------------------------------------------

def case_index_width(B, V, what):
    """V: a backend of tests/index_width_common.py (its sparse images).  "ld": rows [70][2^26] on BIG, t * ld beyond 2^32 bytes
    and elements; "cap": slabs [12][2^29] on TEXT, c * cap beyond 2^32 bytes.  Pack, then unpack what was packed."""
    import index_width_common as iw
    vs, T = 32, iw.T
    Cn = 68 if what == "ld" else iw.DEGA_C
    f = fields(vs, T, Cn, 3)
    if what == "ld":
        ld, cap = iw.PITCH4["BIG"], axdr_bytes(T, vs)
        a = V.view("BIG", "int32", ld)
        iw.put_filled(V, a, f.astype(np.uint32).view(np.int32), -1)
        iw.crossed(range(T), 4 * ld, elem=4)
        slabs = V.dev(np.full(Cn * cap, CANARY, dtype=np.uint8))
        x_ptr, s_ptr = V.ptr(a), V.ptr(slabs)
    else:
        ld, cap = Cn, iw.CAP
        s = V.view("TEXT", "uint8", cap)
        iw.poison(V, s, 0, Cn, 0, iw.DEGA_BAND_AT + iw.BAND)
        iw.poison(V, s, 0, Cn, cap - iw.BAND)
        iw.crossed(range(Cn), cap)
        x = V.dev(f.astype(np.uint32).view(np.int32))
        x_ptr, s_ptr = V.ptr(x), V.ptr(s)
    bits, err = iw.results(V, Cn), iw.results(V, Cn, np.int32, 77)
    assert B.pack(x_ptr, I32, Cn, T, ld, 0, 100.0, vs, s_ptr, cap, V.ptr(bits), V.ptr(err), -1, 1 << 24) == OK
    assert (V.host(err) == 0).all() and (V.host(bits).view(np.uint64) == T * vs).all()
    want = [pack_channel(f[:, c], vs)[0] for c in range(Cn)]
    if what == "ld":
        got = V.host(slabs).reshape(Cn, cap)
        assert all(got[c].tobytes() == want[c] for c in range(Cn)), "streams"
    else:
        assert all(V.get(s, c, c + 1, 0, len(want[c])).tobytes() == want[c] for c in range(Cn)), "streams"
        iw.holds(V, s, 0, Cn, iw.DEGA_BAND_AT, "axdr pack")
        iw.holds(V, s, 0, Cn, cap - iw.BAND, "axdr pack")
    # and back, into the other image where the rows were the large one
    count, derr = iw.results(V, Cn), iw.results(V, Cn, np.int32, 77)
    if what == "ld":
        out = V.view("MID", "int32", iw.PITCH4["MID"])
        iw.poison(V, out, 0, T, 0, Cn + iw.BAND)
        iw.crossed(range(T), 4 * iw.PITCH4["MID"])
        assert B.unpack(s_ptr, cap, V.ptr(bits), Cn, T, iw.PITCH4["MID"], 100.0, vs, I32, V.ptr(out), V.ptr(count), V.ptr(derr), -1, 1 << 24) == OK
        back = V.get(out, 0, T, 0, Cn)
        iw.holds(V, out, 0, T, Cn, "axdr unpack")
    else:
        o = V.dev(np.zeros(T * Cn, dtype=np.int32))
        assert B.unpack(s_ptr, cap, V.ptr(bits), Cn, T, Cn, 100.0, vs, I32, V.ptr(o), V.ptr(count), V.ptr(derr), -1, 1 << 24) == OK
        back = V.host(o).reshape(T, Cn)
    assert (V.host(derr) == 0).all() and (V.host(count).view(np.uint64) == T).all()
    assert (back.view(np.uint32) == f.astype(np.uint32)).all(), "fields"


# ---- the fixture -------------------------------------------------------------------------------------------------------------------

GOLDEN_SIZES = (8, 12, 17, 24, 32, 40, 64)
GOLDEN_ROWS = 37
GOLDEN_CHANNELS = 3


def golden_input(vs):
    """float32 bit patterns [GOLDEN_ROWS, GOLDEN_CHANNELS] for the fixture: accepted readings of (vs, 100.0)"""
    return float_rows(vs, 100.0, GOLDEN_ROWS, GOLDEN_CHANNELS)
