"""Shared by tests/test_index_width_host.py (the emulator of tests/sim/) and tests/test_gpu_index_width.py (the C ABI):
every kernel family held to its reference where its `index * pitch` products -- t * ld, c * stride, c * cap -- pass 2^31
bytes, 2^32 bytes and 2^32 elements.  The model is tests/test_gpu_channel_major.py::test_offsets_are_64_bit: a sparse
image with a huge pitch is allocated once and only its logical region is ever written or read, which costs nothing on the
GPU (torch.empty) and nothing on the CPU (numpy.empty commits only the pages that are touched).

The images, T = 70 rows everywhere, so every case has rows on both sides of each line:
  BIG    4-byte [70][2^26], also 8-byte [70][2^25]: row 8 starts at 2^31 bytes, row 16 at 2^32 bytes, row 64 at 2^32 elements
  MID    4-byte [70][2^24]: row 32 starts at 2^31 bytes, row 64 at 2^32 bytes
  TEXT, TEXT2  uint8 [6][2^30]: channel 2 starts at 2^31, channel 4 at 2^32; as slabs [12][2^29] channel 4 and channel 8
A wrapped offset lands inside the same allocation at offset mod 2^32, so the kernel would read or overwrite another row:
every case compares rows on both sides with the reference, exactly, and checks a poisoned band next to every output region.

A case is a function of a backend `B` (the two test files have one each):
  B.view(name, dtype, pitch)      the image as a 2-d array [rows][pitch] of int32, int64 or uint8
  B.put(a, r0, c0, block)         block (numpy, 2-d, the same item size) to a[r0:, c0:]
  B.get(a, r0, r1, c0, c1)        numpy copy of a[r0:r1, c0:c1]
  B.dev(x) / B.host(d) / B.ptr(d) a small array on the device, back, and its address (B.ptr of a view: its first byte);
                                  the backend keeps what dev() made alive until B.forget(), which run() calls behind a case
and one method per entry point, its arguments those of the C ABI without the context and the stream, addresses as integers.

That the cases bite was shown on the emulator, in a scratch copy, with one product per kernel narrowed to 32 bits (never
committed).  The mutation, and the cases of test_index_width_host.py that then failed:
  aggregate        a.v + (uint32_t)(t0 * a.ld), a.a + (uint32_t)(j0 * a.ld_out)     aggregate N=1 with that array on BIG
  levels, counted  the walking src / dst offset kept in 32 bits                      aggregate_levels*, that array on BIG
  DEGA encode      a.out + (uint32_t)(c * a.cap); a.x + (uint32_t)(t0 * a.ld)       every encode* case; encode, encode_var, encode_f32 BIG
  DEGA encode      the four-row load of a full wave: a.x + (uint32_t)(row * a.ld) + c_wave0 + q4 * 4u   all six cases at C=76 (int32 at 32
                   and 17 bits, counted, float; both models) and none at C=12, whose one partial wave never takes that load
  DEGA decode      (uint32_t)(row * a.ld) in the row store; a.in + (uint32_t)(c * a.cap)   decode, decode_var, decode_f32 BIG; every decode* case
  normalize, denormalize   (uint32_t)(t * a.ld) on the load, on the store             normalize BIG, denormalize BIG
  encode csv       a.out + (uint32_t)(c * a.stride); src + (uint32_t)(t * a.ld)     every csv_write* case (both stores, counted, split)
  decode csv       (uint32_t)(t * a.ld) in the row stores; a.text + (uint32_t)(c * a.stride)   csv_read BIG, csv_read_split BIG; all four
  LZMH             c * a.stride and c * a.cap narrowed on either side; a.x[(uint32_t)(t * a.ld) + c]   lzmh_encode, lzmh_decode, lzmh_render
  compaction       a.slabs + (uint32_t)(c * a.cap), gather and scatter               compact_gather, compact scatter
An element product on MID (70 x 2^24 elements) or on the int64 view (70 x 2^25) stays below 2^32, so those cases catch byte
offsets only; within a segment of encode_segment the rows are relative to the segment's base, which the caller computes."""
import functools

import numpy as np

import csv_common as cc
import csv_read_common as crc
import hostile_common as hc
import lzmh_hostile_common as lh
from agg_common import meter, same_floats, sequential
from oracle import orc

T = 70
IMAGES = {"BIG": 70 << 28, "MID": 70 << 26, "TEXT": 6 << 30, "TEXT2": 6 << 30}  # bytes
PITCH4 = {"BIG": 1 << 26, "MID": 1 << 24}  # 4-byte elements per row
STRIDE = 1 << 30   # TEXT as [6][2^30]
CAP = 1 << 29      # TEXT as [12][2^29]: the largest cap check_shape accepts
LIVE_BYTES = sum(IMAGES.values())
BAND = 16
POISON = 0x5A5A5A5A   # in every byte of a band: no text holds 'Z', no result below is this word
NAN_FILL = 0x7FC12345  # next to a float input region: a NaN with a payload
LINE31, LINE32 = 1 << 31, 1 << 32
DEGA_BAND_AT = 2048    # bytes into a slab: beyond every stream of 70 samples (70 * 130 bits = 1138 bytes), where nothing may write


# ---- the lines ---------------------------------------------------------------------------------------------------------------

class View:
    """an image as a 2-d array: `array` (numpy or torch) [rows][pitch] of dtype_name, its first byte at `address`"""

    def __init__(self, array, dtype_name, address):
        self.array, self.dtype_name, self.address = array, dtype_name, address


def crossed(rows, pitch_bytes, elem=0, low=True):
    """not vacuous: of the rows (channels) compared, `pitch_bytes` apart, one starts beyond 2^32 bytes, one below 2^31 (low)
    and -- where `elem` is the element size -- one beyond 2^32 elements"""
    starts = [r * pitch_bytes for r in rows]
    assert max(starts) >= LINE32, ("no row beyond 2^32 bytes", max(starts))
    assert not low or min(starts) < LINE31, ("no row below 2^31 bytes", min(starts))
    assert not elem or max(starts) // elem >= LINE32, ("no row beyond 2^32 elements", max(starts) // elem)


def i32(a):
    """any 4-byte array as the int32 the views hold"""
    return np.ascontiguousarray(a).view(np.int32)


def poison(B, a, r0, r1, c0, width=BAND):
    fill = np.full((r1 - r0, width), 0x5A, dtype=np.uint8) if a.dtype_name == "uint8" else \
        np.full((r1 - r0, width), POISON if a.dtype_name == "int32" else (POISON << 32) | POISON, dtype=a.dtype_name)
    B.put(a, r0, c0, fill)


def holds(B, a, r0, r1, c0, what, width=BAND):
    got = B.get(a, r0, r1, c0, c0 + width)
    want = 0x5A if a.dtype_name == "uint8" else (POISON if a.dtype_name == "int32" else (POISON << 32) | POISON)
    assert (got == want).all(), ("the band next to the output was written", what, np.argwhere(got != want)[0].tolist())


def put_filled(B, a, block, fill):
    """block at rows 0 .., columns 0 .., and `fill` in the 16 columns beyond it: what lies there is not the batch's"""
    wide = np.full((block.shape[0], block.shape[1] + BAND), fill, dtype=block.dtype)
    wide[:, : block.shape[1]] = block
    B.put(a, 0, 0, wide)


def results(B, n, dtype=np.uint64, value=0):
    return B.dev(np.full(n, value, dtype=dtype))


# ---- aggregate -----------------------------------------------------------------------------------------------------------------

LEVEL_AT = 1024  # a second window in an image, at this column: one image, one pitch, two arrays
# where the levels' sums go: the entry points refuse outputs whose address ranges overlap, so every level has an image of its
# own -- level 1 (70 rows) the case's output image at its pitch, level 7 (10 rows) TEXT at 2^27 elements (row 4 starts at
# 2^31 bytes, row 8 at 2^32), level 60 (2 rows) TEXT2 at 2^29 elements (row 1 starts at 2^31 bytes)
LEVELS = (1, 7, 60)
LEVEL_HOMES = (None, ("TEXT", 1 << 27), ("TEXT2", 1 << 29))


def agg_input(B, src, Cn, seed):
    v = meter(np.random.default_rng(seed), T, Cn)
    a = B.view(src, "int32", PITCH4[src])
    put_filled(B, a, i32(v), NAN_FILL)
    return v, a


def agg_outputs(B, dst, Cn, levels):
    """a view per level, poisoned where the sums go and in the band beside them -> (views, pitches, rows per level)"""
    homes = [(dst, PITCH4[dst])] + list(LEVEL_HOMES[1:len(levels)])
    outs = [B.view(name, "int32", pitch) for name, pitch in homes]
    rows = [(T + n - 1) // n for n in levels]
    for out, r in zip(outs, rows):
        poison(B, out, 0, r, 0, Cn + BAND)
    return outs, [pitch for _, pitch in homes], rows


def case_aggregate(B, src, dst, Cn, N, ranges=None):
    """ranges: None is the library's choice of ranges of output rows -- at these shapes a range per row, so that t0 * ld and
    j0 * ld_out cross the lines; the emulator also takes a number (few ranges: the walk inside a range crosses them)"""
    v, a = agg_input(B, src, Cn, 11)
    (out,), _, rows = agg_outputs(B, dst, Cn, [N])
    crossed(range(T), 4 * PITCH4[src], elem=4 if src == "BIG" else 0)
    if N == 1:
        crossed(range(rows[0]), 4 * PITCH4[dst], elem=4 if dst == "BIG" else 0)
    B.aggregate(B.ptr(a), Cn, T, PITCH4[src], N, B.ptr(out), PITCH4[dst], ranges)
    got = B.get(out, 0, rows[0], 0, Cn).view(np.float32)
    assert same_floats(got, sequential(v, N)), (src, dst, Cn, N, np.argwhere(got.view(np.uint32) != sequential(v, N).view(np.uint32))[:4].tolist())
    holds(B, out, 0, rows[0], Cn, "aggregate")


def case_aggregate_levels(B, src, dst, Cn):
    v, a = agg_input(B, src, Cn, 12)
    outs, pitches, rows = agg_outputs(B, dst, Cn, LEVELS)
    crossed(range(T), 4 * PITCH4[src], elem=4 if src == "BIG" else 0)
    crossed(range(rows[0]), 4 * pitches[0], elem=4 if dst == "BIG" else 0)
    crossed(range(rows[1]), 4 * pitches[1])
    B.aggregate_levels(B.ptr(a), Cn, T, PITCH4[src], LEVELS, [B.ptr(o) for o in outs], pitches)
    for n, r, out in zip(LEVELS, rows, outs):
        got = B.get(out, 0, r, 0, Cn).view(np.float32)
        assert same_floats(got, sequential(v, n)), (src, dst, Cn, n)
        holds(B, out, 0, r, Cn, ("aggregate_levels", n))


def ragged_counts(Cn):
    """a count per channel: T, T - 1, ... with a few short ones; the long ones keep rows beyond every line"""
    return np.array([T - (c % 6) if c % 11 != 7 else (c % 5) * 4 for c in range(Cn)], dtype=np.uint64)


def case_aggregate_levels_var(B, src, dst, Cn):
    v, a = agg_input(B, src, Cn, 13)
    count = ragged_counts(Cn)
    outs, pitches, rows = agg_outputs(B, dst, Cn, LEVELS)
    crossed(range(int(count.max())), 4 * PITCH4[src], elem=4 if src == "BIG" else 0)
    crossed(range(int(count.max())), 4 * pitches[0], elem=4 if dst == "BIG" else 0)
    crossed(range((int(count.max()) + 6) // 7), 4 * pitches[1])
    counts = [results(B, Cn) for _ in LEVELS]
    err = results(B, Cn, np.int32, 77)
    B.aggregate_levels_var(B.ptr(a), Cn, T, PITCH4[src], B.ptr(B.dev(count)), LEVELS, [B.ptr(o) for o in outs], pitches, [B.ptr(x) for x in counts], B.ptr(err))
    assert (B.host(err) == 0).all()
    for k, (n, r, out) in enumerate(zip(LEVELS, rows, outs)):
        got = B.get(out, 0, r, 0, Cn).view(np.float32)
        oc = B.host(counts[k])
        for c in range(Cn):
            m = int(count[c])
            want = sequential(v[:m, c:c + 1], n)[:, 0] if m else np.zeros(0, dtype=np.float32)
            assert int(oc[c]) == (m + n - 1) // n == want.size and same_floats(got[: want.size, c], want), (src, dst, Cn, n, c)
        holds(B, out, 0, r, Cn, ("aggregate_levels_var", n))


# ---- DEGA ----------------------------------------------------------------------------------------------------------------------

DEGA_C = 12
# The encoder fetches the rows of a wave whose 64 channels all exist four at a time (rows_x4 in dega_kernels.hpp: its own
# row * ld product); a wave with fewer channels takes the row-at-a-time load.  C = 12 reaches only the second, so the encode
# cases also run at C = 76: one full wave and a partial one, rows 16-byte aligned.  Their slabs are TEXT as [76][2^26]
# (channel 32 starts at 2^31 bytes, channel 64 at 2^32).
WAVE_C = 76
WAVE_CAP = 1 << 26


def cap_of(Cn):
    return CAP if Cn == DEGA_C else WAVE_CAP


@functools.lru_cache(maxsize=None)
def walks(vs, Cn=DEGA_C):
    x = hc.walks(np.random.default_rng([41, vs, Cn]), Cn, T, vs)  # uint64 [T][C]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def streams(vs, ad, ragged=False, Cn=DEGA_C):
    """the oracle's (bytes, bits) per channel of walks(vs, Cn), or of its first ragged_counts rows"""
    x = walks(vs, Cn)
    if not ragged:
        return hc.oracle_encode(x, vs, ad)
    count = ragged_counts(Cn)
    return [hc.oracle_encode(x[: int(count[c]), c:c + 1], vs, ad)[0] for c in range(Cn)]  # (an empty series too: the model's end alone)


def samples_in(B, vs, Cn=DEGA_C):
    """walks(vs) on BIG (int64 containers above 32 bits), -1 beside them -> (the view, its pitch in elements, the element size)"""
    wide = vs > 32
    a = B.view("BIG", "int64" if wide else "int32", PITCH4["BIG"] // (2 if wide else 1))
    x = walks(vs, Cn)
    put_filled(B, a, x.view(np.int64) if wide else x.astype(np.uint32).view(np.int32), -1)
    return a, PITCH4["BIG"] // (2 if wide else 1), 8 if wide else 4


def slabs_out(B, Cn=DEGA_C):
    """TEXT as [12][2^29] (or [76][2^26]) with the head of every slab and the tail of the one before it poisoned"""
    cap = cap_of(Cn)
    assert Cn * cap <= IMAGES["TEXT"]
    s = B.view("TEXT", "uint8", cap)
    poison(B, s, 0, Cn, 0, DEGA_BAND_AT + BAND)
    poison(B, s, 0, Cn, cap - BAND)
    crossed(range(Cn), cap)
    return s


def check_slabs(B, s, bits, err, want, what):
    bits, err = B.host(bits), B.host(err)
    Cn, cap = len(want), cap_of(len(want))
    for c, (data, nb) in enumerate(want):
        assert int(err[c]) == 0 and int(bits[c]) == nb, (what, c, int(err[c]), int(bits[c]), nb)
        assert B.get(s, c, c + 1, 0, len(data)).tobytes() == data, (what, c)
    holds(B, s, 0, Cn, DEGA_BAND_AT, what)
    holds(B, s, 0, Cn, cap - BAND, what)


def slabs_in(B, want):
    s = B.view("TEXT", "uint8", CAP)
    poison(B, s, 0, DEGA_C, 0, DEGA_BAND_AT)  # what lies behind a stream's bits is not the stream's
    for c, (data, _) in enumerate(want):
        if data:
            B.put(s, c, 0, np.frombuffer(data, dtype=np.uint8).reshape(1, -1))
    crossed(range(DEGA_C), CAP)
    return s, B.dev(np.array([nb for _, nb in want], dtype=np.uint64))


def case_dega_encode(B, vs, ad, how, Cn=DEGA_C):
    """how: "whole", "var" (a count per channel) or "segments" (cuts at the rows beside the lines)"""
    a, ld, eb = samples_in(B, vs, Cn)
    s = slabs_out(B, Cn)
    crossed(range(T), ld * eb, elem=4 if eb == 4 else 0)
    assert Cn == DEGA_C or (Cn > 64 and Cn % 64 != 0 and ld % 4 == 0 and B.ptr(a) % 16 == 0)  # (a full wave on the four-row load, and a partial one)
    bits, err = results(B, Cn), results(B, Cn, np.int32, 77)
    args = (Cn, T, ld)
    tail = (B.ptr(s), cap_of(Cn), B.ptr(bits), B.ptr(err))
    if how == "var":
        B.encode_var(B.ptr(a), *args, B.ptr(B.dev(ragged_counts(Cn))), ad, vs, *tail)
    elif how == "segments":
        B.encode_segments(B.ptr(a), *args, ad, vs, (0, 15, 16, 63, 64, T), *tail)
    elif vs > 32:
        B.encode64(B.ptr(a), *args, ad, vs, *tail)
    else:
        B.encode(B.ptr(a), *args, ad, vs, *tail)
    check_slabs(B, s, bits, err, streams(vs, ad, how == "var", Cn), ("encode", vs, ad, how, Cn))


def case_dega_decode(B, vs, ad, how):
    """how: "exact" (T samples or an error) or "var" (up to T, the count reported)"""
    want = streams(vs, ad, how == "var")
    s, bits = slabs_in(B, want)
    wide = vs > 32
    ld, eb = PITCH4["BIG"] // (2 if wide else 1), 8 if wide else 4
    x = B.view("BIG", "int64" if wide else "int32", ld)
    poison(B, x, 0, T, 0, DEGA_C + BAND)
    crossed(range(T), ld * eb, elem=4 if eb == 4 else 0)
    err = results(B, DEGA_C, np.int32, 77)
    counts = results(B, DEGA_C) if how == "var" else None
    args = (B.ptr(s), CAP, B.ptr(bits), DEGA_C, T, ld, ad, vs, B.ptr(x))
    if wide:
        B.decode64(*args, B.ptr(err))
    elif how == "var":
        B.decode_var(*args, B.ptr(counts), B.ptr(err))
    else:
        B.decode(*args, B.ptr(err))
    assert (B.host(err) == 0).all(), B.host(err)
    got = B.get(x, 0, T, 0, DEGA_C)
    w = walks(vs)
    w = w.view(np.int64) if wide else w.astype(np.uint32).view(np.int32)
    count = ragged_counts(DEGA_C) if how == "var" else np.full(DEGA_C, T)
    for c in range(DEGA_C):
        m = int(count[c])
        assert how != "var" or int(B.host(counts)[c]) == m, (vs, ad, c)
        assert (got[:m, c] == w[:m, c]).all(), (vs, ad, how, c, np.argwhere(got[:m, c] != w[:m, c])[:3].ravel().tolist())
    holds(B, x, 0, T, DEGA_C, ("decode", vs, ad, how))


# ---- DEGA, the float entry and exit ------------------------------------------------------------------------------------------------

FACTOR = 100.0


@functools.lru_cache(maxsize=None)
def readings(Cn=DEGA_C):
    v = meter(np.random.default_rng([43, Cn]), T, Cn, top=3000.0)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def float_streams(ad, N=1, Cn=DEGA_C):
    v = readings(Cn) if N == 1 else sequential(readings(Cn), N)
    res = []
    for c in range(Cn):
        ret, data, nb = orc.encode_f32(v[:, c], FACTOR, ad)
        assert ret == 0
        res.append((data, nb))
    return res


def case_float_encode(B, src, ad, N=1, Cn=DEGA_C):
    a = B.view(src, "int32", PITCH4[src])
    put_filled(B, a, i32(readings(Cn)), NAN_FILL)
    s = slabs_out(B, Cn)
    crossed(range(T), 4 * PITCH4[src], elem=4 if src == "BIG" else 0)
    assert Cn == DEGA_C or (Cn > 64 and Cn % 64 != 0 and B.ptr(a) % 16 == 0)
    bits, err = results(B, Cn), results(B, Cn, np.int32, 77)
    if N == 1:
        B.encode_f32(B.ptr(a), Cn, T, PITCH4[src], FACTOR, ad, 32, B.ptr(s), cap_of(Cn), B.ptr(bits), B.ptr(err))
    else:
        B.encode_agg_f32(B.ptr(a), Cn, T, PITCH4[src], N, FACTOR, ad, 32, B.ptr(s), cap_of(Cn), B.ptr(bits), B.ptr(err))
    check_slabs(B, s, bits, err, float_streams(ad, N, Cn), ("encode_f32", src, ad, N, Cn))


def case_float_decode(B, dst, ad):
    want = float_streams(ad)
    s, bits = slabs_in(B, want)
    v = B.view(dst, "int32", PITCH4[dst])
    poison(B, v, 0, T, 0, DEGA_C + BAND)
    crossed(range(T), 4 * PITCH4[dst], elem=4 if dst == "BIG" else 0)
    err = results(B, DEGA_C, np.int32, 77)
    B.decode_f32(B.ptr(s), CAP, B.ptr(bits), DEGA_C, T, PITCH4[dst], FACTOR, ad, 32, B.ptr(v), 0, B.ptr(err))
    assert (B.host(err) == 0).all()
    got = B.get(v, 0, T, 0, DEGA_C).view(np.float32)
    for c in range(DEGA_C):
        ret, w = orc.decode_f32(want[c][0], want[c][1], T, FACTOR, ad)
        assert ret == 0 and w.size == T and (got[:, c].view(np.uint32) == w.view(np.uint32)).all(), (dst, ad, c)
    holds(B, v, 0, T, DEGA_C, ("decode_f32", dst, ad))


def case_normalize(B, img):
    """one pitch for both arrays (the entry point has one ld): the readings at column 0, the samples at column LEVEL_AT of the
    same image; err is the caller's to zero"""
    v = readings()
    a = B.view(img, "int32", PITCH4[img])
    put_filled(B, a, i32(v), NAN_FILL)
    poison(B, a, 0, T, LEVEL_AT, DEGA_C + BAND)
    crossed(range(T), 4 * PITCH4[img], elem=4 if img == "BIG" else 0)
    err = results(B, DEGA_C, np.int32, 0)
    B.normalize(B.ptr(a), DEGA_C, T, PITCH4[img], FACTOR, 32, B.ptr(a) + 4 * LEVEL_AT, B.ptr(err))
    status, want = orc.normalize_each(v.ravel(), FACTOR, 32)
    assert (status == 0).all() and (B.host(err) == 0).all()
    got = B.get(a, 0, T, LEVEL_AT, LEVEL_AT + DEGA_C)
    assert (got.view(np.uint32) == want.astype(np.uint32).reshape(T, DEGA_C)).all(), img
    assert (B.get(a, 0, T, 0, DEGA_C) == i32(v)).all()
    holds(B, a, 0, T, LEVEL_AT + DEGA_C, ("normalize", img))


def case_denormalize(B, img):
    u = walks(32).astype(np.uint32)
    a = B.view(img, "int32", PITCH4[img])
    put_filled(B, a, i32(u), -1)
    poison(B, a, 0, T, LEVEL_AT, DEGA_C + BAND)
    crossed(range(T), 4 * PITCH4[img], elem=4 if img == "BIG" else 0)
    B.denormalize(B.ptr(a), DEGA_C, T, PITCH4[img], FACTOR, 32, B.ptr(a) + 4 * LEVEL_AT)
    want = orc.denormalize_each(u.astype(np.uint64).ravel(), FACTOR, 32).view(np.uint32).reshape(T, DEGA_C)
    assert (B.get(a, 0, T, LEVEL_AT, LEVEL_AT + DEGA_C).view(np.uint32) == want).all(), img
    holds(B, a, 0, T, LEVEL_AT + DEGA_C, ("denormalize", img))


# ---- encode csv ------------------------------------------------------------------------------------------------------------------

CSV_C = 6
TEXT_HEAD = 8192  # bytes of a channel's row that are poisoned before a text is written there: every text below is shorter


@functools.lru_cache(maxsize=None)
def edge_batch(d, column):
    """the readings of the fixture's `edge` list that the reference wrote at d decimals, over and over until they fill [T][C],
    as bit patterns, and every channel's text (py_lines, which is the reference's line for every one of them)"""
    bits, lines = cc.Fixture().lines("edge", d)
    assert bits.size >= 150 and cc.py_lines(bits, d) == lines
    batch = np.ascontiguousarray(np.resize(bits, T * CSV_C).reshape(T, CSV_C))
    sep = ";" if column != 1 else ","
    texts = [b"".join(cc.py_lines(batch[:, c], d, column, sep)) for c in range(CSV_C)]
    assert max(len(t) for t in texts) + 2 * cc.SLACK <= TEXT_HEAD
    return batch, texts, ord(sep)


def text_out(B, name="TEXT"):
    t = B.view(name, "uint8", STRIDE)
    poison(B, t, 0, CSV_C, 0, TEXT_HEAD)
    poison(B, t, 0, CSV_C, STRIDE - BAND)
    crossed(range(CSV_C), STRIDE)
    return t


def check_texts(B, t, lens, err, want, what, exact_end):
    """exact lengths, status 0 and bytes; behind a text the writer owns SLACK bytes (none in the split form: exact_end), and
    nothing behind those or in front of the row"""
    lens, err = B.host(lens), B.host(err)
    for c, w in enumerate(want):
        assert int(err[c]) == 0 and int(lens[c]) == len(w), (what, c, int(err[c]), int(lens[c]), len(w))
        assert B.get(t, c, c + 1, 0, len(w)).tobytes() == w, (what, c)
        free = len(w) + (0 if exact_end else cc.SLACK)
        holds(B, t, c, c + 1, free, (what, c), TEXT_HEAD - free)
    holds(B, t, 0, len(want), STRIDE - BAND, what)


def case_csv_write(B, d, column, form, how):
    """form: "store8" / "store64" (DEGA_CSV_STORE), how: "whole", "var", "split" or "split var" (block rows 16: blocks
    straddle rows 15 / 16 and 63 / 64)"""
    batch, texts, sep = edge_batch(d, column)
    a = B.view("BIG", "int32", PITCH4["BIG"])
    put_filled(B, a, i32(batch), NAN_FILL)
    t = text_out(B)
    crossed(range(T), 4 * PITCH4["BIG"], elem=4)
    lens, err = results(B, CSV_C), results(B, CSV_C, np.int32, 77)
    count = np.array([T, T - 1, 64, 17, T, 16], dtype=np.uint64) if "var" in how else None
    if count is not None:
        texts = [b"".join(cc.py_lines(batch[: int(count[c]), c], d, column, chr(sep))) for c in range(CSV_C)]
    cp = B.ptr(B.dev(count)) if count is not None else 0
    head = (B.ptr(a), CSV_C, T, PITCH4["BIG"])
    tail = (d, column, sep, B.ptr(t), STRIDE, B.ptr(lens), B.ptr(err))
    if how.startswith("split"):
        B.csv_write_split(*head, cp, *tail, 16)
    elif how == "var":
        B.csv_write_var(*head, cp, *tail, form=form)
    else:
        B.csv_write(*head, *tail, form=form)
    check_texts(B, t, lens, err, texts, ("csv_write", d, column, form, how), how.startswith("split"))


# ---- decode csv ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def field_texts():
    """six texts of 70 fields, one class of csv_read_common each, and libc's strtof of every field"""
    rng = np.random.default_rng(47)
    kinds = (lambda r, n: crc.fields_printed(r, n, 2), lambda r, n: crc.fields_printed(r, n, 6), crc.fields_digits, crc.fields_exponents,
             crc.fields_hex, crc.fields_midpoints)
    texts, want = [], []
    for make in kinds:
        t, w = crc.deal(make(rng, T), 1)
        texts.append(t[0])
        want.append(crc.expected(t[0])[0])
        assert (want[-1] == w[0]).all() and w[0].size == T and crc.expected(t[0])[1] == 0
    assert max(len(t) for t in texts) <= TEXT_HEAD
    return texts, want


def texts_in(B, texts, name="TEXT"):
    t = B.view(name, "uint8", STRIDE)
    poison(B, t, 0, len(texts), 0, TEXT_HEAD)  # what lies behind a text is not the text's
    for c, s in enumerate(texts):
        if s:
            B.put(t, c, 0, np.frombuffer(s, dtype=np.uint8).reshape(1, -1))
    crossed(range(len(texts)), STRIDE)
    return t, B.dev(np.array([len(s) for s in texts], dtype=np.uint64))


def case_csv_read(B, dst, block_bytes):
    """block_bytes: None for the unsplit reader, else the split reader with the backend's block (B.split_block_bytes)"""
    texts, want = field_texts()
    t, lens = texts_in(B, texts)
    v = B.view(dst, "int32", PITCH4[dst])
    poison(B, v, 0, T, 0, CSV_C + BAND)
    crossed(range(T), 4 * PITCH4[dst], elem=4 if dst == "BIG" else 0)
    count, err = results(B, CSV_C), results(B, CSV_C, np.int32, 77)
    args = (B.ptr(t), STRIDE, B.ptr(lens), CSV_C, 1, ord(","), B.ptr(v), T, PITCH4[dst], B.ptr(count), B.ptr(err))
    if block_bytes is None:
        B.csv_read(*args)
    else:
        B.csv_read_split(*args, B.split_block_bytes)
    got = B.get(v, 0, T, 0, CSV_C).view(np.uint32)
    assert crc.check_channels(got, B.host(count), B.host(err), want, [0] * CSV_C, T, ("csv_read", dst, block_bytes)) == T * CSV_C
    holds(B, v, 0, T, CSV_C, ("csv_read", dst, block_bytes))


# ---- LZMH --------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lzmh_texts():
    """six texts of a few KB, the kinds of lzmh_encoder_common, and the oracle's stream of each"""
    import lzmh_encoder_common as le
    texts = [le.text_of(c, 2000 + 300 * c)[: 2000 + 300 * c - c] for c in (0, 1, 2, 4, 5, 7)]
    assert max(len(s) for s in texts) + 64 <= TEXT_HEAD
    return texts, [lh.oracle_encode(s) for s in texts]


def case_lzmh_encode(B):
    texts, want = lzmh_texts()
    t, lens = texts_in(B, texts)
    out = text_out(B, "TEXT2")
    bits, err = results(B, CSV_C), results(B, CSV_C, np.int32, 77)
    B.lzmh_encode(B.ptr(t), STRIDE, B.ptr(lens), CSV_C, B.ptr(out), STRIDE, B.ptr(bits), B.ptr(err))
    bits, err = B.host(bits), B.host(err)
    for c, (data, nb) in enumerate(want):
        assert int(err[c]) == 0 and int(bits[c]) == nb, ("lzmh_encode", c, int(err[c]), int(bits[c]), nb)
        assert B.get(out, c, c + 1, 0, len(data)).tobytes() == data, ("lzmh_encode", c)
        free = (nb + 31) // 32 * 4 + 16  # (a stream's bytes in whole words and 16 more are the kernel's: dega_hip.hip, "When does a channel fit")
        holds(B, out, c, c + 1, free, ("lzmh_encode", c), TEXT_HEAD - free)
    holds(B, out, 0, CSV_C, STRIDE - BAND, "lzmh_encode")


def case_lzmh_decode(B):
    texts, want = lzmh_texts()
    s, bits = texts_in(B, [data for data, _ in want])
    bits = B.dev(np.array([nb for _, nb in want], dtype=np.uint64))
    out = text_out(B, "TEXT2")
    lens, err = results(B, CSV_C), results(B, CSV_C, np.int32, 77)
    B.lzmh_decode(B.ptr(s), STRIDE, B.ptr(bits), CSV_C, B.ptr(out), STRIDE, B.ptr(lens), B.ptr(err))
    lens, err = B.host(lens), B.host(err)
    for c, w in enumerate(texts):
        assert int(err[c]) == 0 and int(lens[c]) == len(w), ("lzmh_decode", c, int(err[c]), int(lens[c]), len(w))
        assert B.get(out, c, c + 1, 0, len(w)).tobytes() == w, ("lzmh_decode", c)
        free = (len(w) + 7) // 8 * 8  # (the decoder stores 8 bytes at a time)
        holds(B, out, c, c + 1, free, ("lzmh_decode", c), TEXT_HEAD - free)
    holds(B, out, 0, CSV_C, STRIDE - BAND, "lzmh_decode")


def case_lzmh_render(B):
    rng = np.random.default_rng(53)
    x = np.abs(np.cumsum(rng.integers(-300, 301, (T, CSV_C)), axis=0) + np.array([0, 99, 100, 23045, 2000000000, 7])).astype(np.int32)
    a = B.view("BIG", "int32", PITCH4["BIG"])
    put_filled(B, a, x, -1)
    t = text_out(B)
    crossed(range(T), 4 * PITCH4["BIG"], elem=4)
    lens, err = results(B, CSV_C), results(B, CSV_C, np.int32, 77)
    B.lzmh_render(B.ptr(a), CSV_C, T, PITCH4["BIG"], B.ptr(t), STRIDE, B.ptr(lens), B.ptr(err))
    lens, err = B.host(lens), B.host(err)
    for c in range(CSV_C):
        want = "".join("%d.%02d\n" % (v // 100, v % 100) for v in x[:, c].tolist()).encode()
        assert int(err[c]) == 0 and int(lens[c]) == len(want) and B.get(t, c, c + 1, 0, len(want)).tobytes() == want, ("lzmh_render", c)
        holds(B, t, c, c + 1, len(want) + 16, ("lzmh_render", c), TEXT_HEAD - len(want) - 16)
    holds(B, t, 0, CSV_C, STRIDE - BAND, "lzmh_render")


# ---- compaction --------------------------------------------------------------------------------------------------------------------

def case_compact(B, scatter):
    """slabs [12][2^29] on TEXT <-> packed, the bytes themselves; the lengths leave every alignment on the packed side"""
    rng = np.random.default_rng(59)
    sizes = [0, 1, 19, 20, 333, 1000, 16, 17, 4, 777, 35, 1023]
    data = [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in sizes]
    offsets = np.concatenate([[3], 3 + np.cumsum(sizes)]).astype(np.uint64)  # (a first offset that is no multiple of 4)
    total = int(offsets[-1])
    s = B.view("TEXT", "uint8", CAP)
    crossed(range(DEGA_C), CAP)
    poison(B, s, 0, DEGA_C, 0, DEGA_BAND_AT)
    poison(B, s, 0, DEGA_C, CAP - BAND)
    if scatter:
        packed = B.dev(np.frombuffer(b"\xee" * 3 + b"".join(data) + b"\xee" * 16, dtype=np.uint8).copy())
    else:
        for c, d in enumerate(data):
            if d:
                B.put(s, c, 0, np.frombuffer(d, dtype=np.uint8).reshape(1, -1))
        packed = B.dev(np.full(total + 16, 0xEE, dtype=np.uint8))
    B.compact(B.ptr(s), CAP, B.ptr(B.dev(offsets)), DEGA_C, B.ptr(packed), scatter)
    if scatter:
        for c, d in enumerate(data):
            assert B.get(s, c, c + 1, 0, len(d)).tobytes() == d, ("scatter", c)
            holds(B, s, c, c + 1, len(d), ("scatter", c), DEGA_BAND_AT - len(d))
        holds(B, s, 0, DEGA_C, CAP - BAND, "scatter")
    else:
        assert B.host(packed).tobytes() == b"\xee" * 3 + b"".join(data) + b"\xee" * 16


# ---- the chains: only the caller's arrays on the big pitch (GPU only) -----------------------------------------------------------

CHAIN_TEXT_STRIDE = 4096  # an ordinary one: the context's text scratch stays small


def case_chain_lzmh_encode_f32(B):
    batch, texts, sep = edge_batch(2, 1)
    assert max(len(t) for t in texts) + cc.SLACK <= CHAIN_TEXT_STRIDE
    a = B.view("BIG", "int32", PITCH4["BIG"])
    put_filled(B, a, i32(batch), NAN_FILL)
    crossed(range(T), 4 * PITCH4["BIG"], elem=4)
    cap = 8192
    out = B.dev(np.zeros(CSV_C * cap, dtype=np.uint8))
    bits, tl, err = results(B, CSV_C), results(B, CSV_C), results(B, CSV_C, np.int32, 77)
    B.lzmh_encode_f32(B.ptr(a), CSV_C, T, PITCH4["BIG"], 2, 1, sep, CHAIN_TEXT_STRIDE, B.ptr(out), cap, B.ptr(bits), B.ptr(tl), B.ptr(err))
    got = B.host(out).reshape(CSV_C, cap)
    for c, text in enumerate(texts):
        data, nb = lh.oracle_encode(text)
        assert int(B.host(err)[c]) == 0 and int(B.host(tl)[c]) == len(text) and int(B.host(bits)[c]) == nb, ("lzmh_encode_f32", c)
        assert got[c, : len(data)].tobytes() == data, ("lzmh_encode_f32", c)


def case_chain_encode_levels_f32(B):
    v = readings()
    a = B.view("BIG", "int32", PITCH4["BIG"])
    put_filled(B, a, i32(v), NAN_FILL)
    crossed(range(T), 4 * PITCH4["BIG"], elem=4)
    cap = 2048
    outs = [B.dev(np.zeros(DEGA_C * cap, dtype=np.uint8)) for _ in LEVELS]
    bits, err = [results(B, DEGA_C) for _ in LEVELS], [results(B, DEGA_C, np.int32, 77) for _ in LEVELS]
    B.encode_levels_f32(B.ptr(a), DEGA_C, T, PITCH4["BIG"], LEVELS, FACTOR, 1, 32, [B.ptr(o) for o in outs], [cap] * len(LEVELS),
                        [B.ptr(b) for b in bits], [B.ptr(e) for e in err])
    for k, n in enumerate(LEVELS):
        got = B.host(outs[k]).reshape(DEGA_C, cap)
        for c, (data, nb) in enumerate(float_streams(1, n)):
            assert int(B.host(err[k])[c]) == 0 and int(B.host(bits[k])[c]) == nb and got[c, : len(data)].tobytes() == data, ("encode_levels_f32", n, c)


def case_chain_lzmh_decode_f32(B):
    _, texts, sep = edge_batch(2, 1)
    coded = [lh.oracle_encode(t) for t in texts]
    cap = (max(len(d) for d, _ in coded) + 19) // 4 * 4
    slabs = np.full((CSV_C, cap), 0x5A, dtype=np.uint8)
    for c, (d, _) in enumerate(coded):
        slabs[c, : len(d)] = np.frombuffer(d, dtype=np.uint8)
    v = B.view("BIG", "int32", PITCH4["BIG"])
    poison(B, v, 0, T, 0, CSV_C + BAND)
    crossed(range(T), 4 * PITCH4["BIG"], elem=4)
    count, tl, err = results(B, CSV_C), results(B, CSV_C), results(B, CSV_C, np.int32, 77)
    B.lzmh_decode_f32(B.ptr(B.dev(slabs.ravel())), cap, B.ptr(B.dev(np.array([nb for _, nb in coded], dtype=np.uint64))), CSV_C, CHAIN_TEXT_STRIDE, 1, sep,
                      B.ptr(v), T, PITCH4["BIG"], B.ptr(count), B.ptr(tl), B.ptr(err))
    want = [crc.expected(t)[0] for t in texts]
    got = B.get(v, 0, T, 0, CSV_C).view(np.uint32)
    assert crc.check_channels(got, B.host(count), B.host(err), want, [0] * CSV_C, T, "lzmh_decode_f32") == T * CSV_C
    assert [int(n) for n in B.host(tl)] == [len(t) for t in texts]
    holds(B, v, 0, T, CSV_C, "lzmh_decode_f32")


# ---- the list ------------------------------------------------------------------------------------------------------------------------

PAIRS = (("BIG", "MID"), ("MID", "BIG"))  # two pitched 4-byte arrays: each on either image, so both cross the byte lines and the element line


def _cases():
    out = []
    add = lambda name, fn, *args, **kw: out.append((name, fn, args, kw))  # noqa: E731
    for src, dst in PAIRS:
        io = "%s to %s" % (src, dst)
        for Cn in (68, 67):
            for N in (1, 7):
                add("aggregate C=%d N=%d %s" % (Cn, N, io), case_aggregate, src, dst, Cn, N)
            add("aggregate_levels C=%d %s" % (Cn, io), case_aggregate_levels, src, dst, Cn)
            add("aggregate_levels_var C=%d %s" % (Cn, io), case_aggregate_levels_var, src, dst, Cn)
        add("normalize %s" % src, case_normalize, src)
        add("denormalize %s" % src, case_denormalize, src)
    for ad in (1, 0):
        model = "adaptive" if ad else "static"
        for vs in (32, 17):
            add("encode vs=%d %s" % (vs, model), case_dega_encode, vs, ad, "whole")
            add("decode vs=%d %s" % (vs, model), case_dega_decode, vs, ad, "exact")
        add("encode C=76 %s" % model, case_dega_encode, 32, ad, "whole", WAVE_C)
        add("encode_f32 C=76 %s" % model, case_float_encode, "BIG", ad, 1, WAVE_C)
        add("encode_var %s" % model, case_dega_encode, 32, ad, "var")
        add("decode_var %s" % model, case_dega_decode, 32, ad, "var")
        add("encode_segment %s" % model, case_dega_encode, 32, ad, "segments")
        add("encode64 vs=40 %s" % model, case_dega_encode, 40, ad, "whole")
        add("decode64 vs=40 %s" % model, case_dega_decode, 40, ad, "exact")
        for img in ("BIG", "MID"):
            add("encode_f32 %s %s" % (img, model), case_float_encode, img, ad)
            add("decode_f32 %s %s" % (img, model), case_float_decode, img, ad)
    add("encode vs=17 C=76", case_dega_encode, 17, 1, "whole", WAVE_C)
    add("encode_var C=76", case_dega_encode, 32, 1, "var", WAVE_C)
    add("encode_agg_f32 N=7", case_float_encode, "BIG", 1, 7)
    for form in ("store8", "store64"):
        for d in (2, 6):
            add("csv_write d=%d %s" % (d, form), case_csv_write, d, 1, form, "whole")
        add("csv_write_var %s" % form, case_csv_write, 2, 1, form, "var")
    add("csv_write column 3", case_csv_write, 2, 3, "store8", "whole")
    for d in (2, 6):
        add("csv_write_split d=%d" % d, case_csv_write, d, 1, None, "split")
    add("csv_write_split counted", case_csv_write, 2, 1, None, "split var")
    add("csv_write_split column 3", case_csv_write, 6, 3, None, "split")
    for img in ("BIG", "MID"):
        add("csv_read %s" % img, case_csv_read, img, None)
        add("csv_read_split %s" % img, case_csv_read, img, "split")
    add("lzmh_encode", case_lzmh_encode)
    add("lzmh_decode", case_lzmh_decode)
    add("lzmh_render", case_lzmh_render)
    add("compact_gather", case_compact, False)
    return out


CASES = _cases()
HOST_ONLY = [("compact scatter", case_compact, (True,), {})] + \
    [("aggregate C=%d N=1 %s to %s in three ranges" % (Cn, src, dst), case_aggregate, (src, dst, Cn, 1, 3), {}) for src, dst in PAIRS for Cn in (68, 67)]
GPU_ONLY = [("lzmh_encode_f32", case_chain_lzmh_encode_f32, (), {}), ("encode_levels_f32", case_chain_encode_levels_f32, (), {}),
            ("lzmh_decode_f32", case_chain_lzmh_decode_f32, (), {})]


def run(B, case):
    name, fn, args, kw = case
    try:
        fn(B, *args, **kw)
    finally:
        B.forget()
