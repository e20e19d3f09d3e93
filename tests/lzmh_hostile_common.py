"""Shared by tests/test_lzmh_hostile_host.py and tests/test_gpu_lzmh_hostile.py: damaged and hand-assembled LZMH streams and
the checker that holds a decoder to the oracle's answer on every one of them, in the style of tests/hostile_common.py.

The oracle's LZMH decoder (orc_lzmh_decode) is total: it returns 0 on every bit string, so every channel here has a defined
expected length and expected bytes, and no channel is excused.  Valid streams come from the oracle's encoder, never from the
kernels.  Three sources:
  * corpus(C, n): texts of five sorts, encoded, then damaged by the ten KINDS of hostile_common -- streams that build a
    frequency list and a history before (or while) they go wrong;
  * the assembler (Bits): streams written code by code, for what no encoder writes -- list codes that name unused entries,
    recent offsets never set, matches into history never written, every fill of the writer's 8-byte accumulator against
    every offset, every cut of one stream;
  * named(): single streams with a story.
Every set comes in the two forms of hostile_common: `clean` (beyond a stream's exact length lies what the damage left) and
`garbage` (every bit from there to the end of the slab random).  A decoder's result must not depend on the form."""
import functools
import itertools

import numpy as np

import hostile_common as hc
from oracle import orc

SORTS = ("meter lines", "random digits", "random bytes", "abcabcabd repeated", "bytes 0..2")

# What the oracle alone says about the damaged channels of corpus(C, n): (decoded bytes differ from the text the stream was
# made from, decoded text longer than it, shorter than it), as counted when the corpus was written; check_not_vacuous
# asserts three quarters of each (numpy promises the same random stream only within a version line) and, whatever the
# table says, three quarters / a tenth / a tenth of the damaged channels.  C = 70: 63 damaged channels, C = 130: 117.
ORACLE_COUNTS = {
    (70, 40): (62, 28, 24), (70, 600): (60, 24, 29),
    (130, 40): (113, 40, 44), (130, 600): (113, 41, 59), (130, 3000): (114, 35, 65),
}


def oracle_encode(text):
    r, b, n = orc.stage("lzmh", True, text, 8 * len(text))
    assert r == 0
    return b[: (n + 7) // 8], n


def oracle_decode(data, nbits):
    """the oracle on the first nbits bits of data (orc_bits_assign copies ceil(nbits / 8) bytes and clears the rest of the last)"""
    r, d, dn = orc.stage("lzmh", False, bytes(data[: (nbits + 7) // 8]), nbits)
    assert r == 0 and dn % 8 == 0
    return d[: dn // 8]


def text_of(rng, sort, n):
    if sort == 0:
        return "".join("%.2f\n" % v for v in 230 + np.cumsum(rng.normal(0, 0.3, n // 6 + 1))).encode()[:n]
    if sort == 1:
        return bytes(rng.integers(48, 58, n, dtype=np.uint8))
    if sort == 2:
        return bytes(rng.integers(0, 256, n, dtype=np.uint8))
    if sort == 3:
        return (b"abcabcabd" * (n // 9 + 1))[:n]
    return bytes(rng.integers(0, 3, n, dtype=np.uint8))


class Streams:
    """A batch of streams: name[c], slabs[form] uint8 [C][cap] (cap the smallest multiple of 4 that holds the longest), bits
    uint64 [C], and -- computed on first use and kept -- want[c], the bytes the oracle decodes channel c to.  Read-only."""

    def __init__(self, items, seed, to_slab_end=None):
        """items: (name, bytes, bits) per channel; to_slab_end: a channel whose length becomes 8 * cap (its bytes are zeros there)"""
        self.C = len(items)
        self.name = [i[0] for i in items]
        rows = [bytes(i[1]) for i in items]
        bits = np.array([i[2] for i in items], dtype=np.uint64)
        self.cap = 4 * ((max(max(len(r) for r in rows), 1) + 3) // 4)
        if to_slab_end is not None:
            bits[to_slab_end] = 8 * self.cap
            self.name[to_slab_end] += ", then to the end of the slab"
        clean, garbage = hc.slab_forms(np.random.default_rng([seed, self.C, self.cap]), rows, bits, self.cap)
        self.slabs = {"clean": clean, "garbage": garbage}
        self.bits = bits
        for a in (clean, garbage, bits):
            a.setflags(write=False)
        self._want = None

    @property
    def want(self):
        if self._want is None:
            self._want = [oracle_decode(self.slabs["clean"][c].tobytes(), int(self.bits[c])) for c in range(self.C)]
        return self._want

    def stride(self):
        """the row a decoder is given: the oracle's own longest output, rounded up to a multiple of 8"""
        return max(8, (max(len(w) for w in self.want) + 7) // 8 * 8)

    def pick(self, channels):
        """the same streams, fewer of them (own slabs, own garbage)"""
        clean = self.slabs["clean"]
        sub = Streams([(self.name[c], clean[c, : (int(self.bits[c]) + 7) // 8].tobytes(), int(self.bits[c])) for c in channels], 7)
        if self._want is not None:
            sub._want = [self._want[c] for c in channels]
        return sub


# ---- (a) the damaged corpus ----------------------------------------------------------------------------------------------------
class Corpus(Streams):
    """channel c: a text of n bytes of sort c % 5, encoded by the oracle, damaged by kind c % 10.  text[c], kind[c], sort[c]."""

    def __init__(self, C, n, seed=2025):
        rng = np.random.default_rng([seed, C, n])
        self.n = n
        self.kind, self.sort = np.arange(C) % 10, np.arange(C) % 5
        self.text, items = [], []
        for c in range(C):
            t = text_of(rng, int(self.sort[c]), n)
            b, nb = oracle_encode(t)
            k = int(self.kind[c])
            b, nb, what = hc.damage(rng, bytearray(b), nb, k, c)
            self.text.append(t)
            items.append(("%s, %s%s" % (SORTS[self.sort[c]], hc.KINDS[k], ": " + what if what else ""), b, nb))
        # the longest of the lengthened streams is lengthened further, to its slab's very end
        sevens = [c for c in range(C) if self.kind[c] == 7]
        Streams.__init__(self, items, seed, to_slab_end=max(sevens, key=lambda c: items[c][2]) if sevens else None)

    def damaged(self):
        return int((self.kind != 0).sum())

    def counts(self):
        """of the damaged channels: (decoded bytes differ from the text, longer than it, shorter than it)"""
        d = [c for c in range(self.C) if self.kind[c] != 0]
        return (sum(self.want[c] != self.text[c] for c in d), sum(len(self.want[c]) > len(self.text[c]) for c in d),
                sum(len(self.want[c]) < len(self.text[c]) for c in d))


@functools.lru_cache(maxsize=None)
def corpus(C, n):
    return Corpus(C, n)


def check_not_vacuous(C, n):
    """the oracle alone: the damage does damage (and the healthy channels are healthy)"""
    corp = corpus(C, n)
    for c in range(C):
        assert corp.kind[c] != 0 or corp.want[c] == corp.text[c], (C, n, c)
    got, damaged, table = corp.counts(), corp.damaged(), ORACLE_COUNTS[(C, n)]
    for k, floor in enumerate(((3 * damaged + 3) // 4, (damaged + 9) // 10, (damaged + 9) // 10)):
        assert got[k] >= floor and got[k] >= (3 * table[k] + 3) // 4, ((C, n), ("differ", "longer", "shorter")[k], got, table, damaged)
    return got, damaged


# ---- (b) the assembler ---------------------------------------------------------------------------------------------------------
def list_code(i):
    """the static prefix code of list position i < 19 (lzmh.c:86-106): 4 of 4 bits, 5 of 5, 4 of 6, 2 of 7, 4 of 8"""
    for first, top, k in ((15, 0x83, 8), (13, 0x43, 7), (9, 0x25, 6), (4, 0x17, 5), (0, 0x0F, 4)):
        if i >= first:
            return top - (i - first), k


class Bits:
    """an LZMH stream written code by code, MSB first; every call returns self"""

    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, v, k):
        assert 0 <= v < (1 << k)
        self.v, self.n = (self.v << k) | v, self.n + k
        return self

    def raw(self, byte):  # 00 + byte
        return self.put(byte, 10)

    def lst(self, i):  # 1... : the literal at list position i
        return self.put(*list_code(i))

    def length(self, L):  # 0 + 3 bits = 3..10 | 10 + 3 bits = 11..18 | 11 + 8 bits = 19..274
        return self.put(L - 3, 4) if L < 11 else self.put(0x10 | (L - 11), 5) if L < 19 else self.put(0x300 | (L - 19), 10)

    def match(self, offset, L):  # 010 + offset - 1 in 7 bits
        return self.put(0x100 | (offset - 1), 10).length(L)

    def rep(self, k, L):  # the k-th most recent offset: 0110 | 01110 | 011110 | 011111
        return self.put(*((0x06, 4), (0x0E, 5), (0x1E, 6), (0x1F, 6))[k]).length(L)

    def stream(self, cut=0):
        """(bytes, bits): the whole stream, or all but its last `cut` bits (the bytes keep them)"""
        pad = -self.n % 8
        return (self.v << pad).to_bytes((self.n + pad) // 8, "big"), self.n - cut


GRID_O = tuple(range(1, 13)) + (63, 64, 65) + tuple(range(120, 129))
GRID_L = tuple(range(3, 21)) + (273, 274)
GRID_P = tuple(range(0, 12)) + tuple(range(125, 130)) + tuple(range(250, 258))


def grid_cells(thin=1, ps=GRID_P):
    """(o, L, p) of the copy grid; thin > 1 keeps the cells whose three indices sum to a multiple of it -- a Latin selection:
    every value of every axis, and every pair of values of two axes for thin <= the third axis' length, stays"""
    return [(o, L, p) for (i, o), (j, L), (k, p) in itertools.product(enumerate(GRID_O), enumerate(GRID_L), enumerate(ps)) if (i + j + k) % thin == 0]


def grid_of(cells, seed=31):
    """one channel per cell (o, L, p): p random non-zero raw literals, one match(o, L), 9 raw literals; it decodes to
    p + L + 9 bytes.  .cells keeps the cells."""
    rng = np.random.default_rng(seed)
    items = []
    for o, L, p in cells:
        b = Bits()
        for byte in rng.integers(1, 256, p).tolist():
            b.raw(byte)
        b.match(o, L)
        for byte in rng.integers(1, 256, 9).tolist():
            b.raw(byte)
        items.append(("grid o=%d L=%d p=%d" % (o, L, p),) + b.stream())
    s = Streams(items, seed)
    s.cells = list(cells)
    return s


@functools.lru_cache(maxsize=None)
def copy_grid(thin=1, ps=GRID_P):
    """the copy grid: every hp & 3, every fill of the writer's 8-byte accumulator, the period path for every offset below 8,
    matches across the seam of the 256-byte ring, and reads of history never written (o > p)"""
    return grid_of(grid_cells(thin, ps))


SOUP_LENGTHS = (3, 10, 11, 18, 19, 274)


def soup_tokens(rng, b, count):
    """count random tokens appended to b: raw | list code 0..18, in use or not | new offset | recent offset 0..3, set or not"""
    for _ in range(count):
        kind = int(rng.integers(0, 4))
        if kind == 0:
            b.raw(int(rng.integers(0, 256)))
        elif kind == 1:
            b.lst(int(rng.integers(0, 19)))
        else:
            cls = int(rng.integers(0, 3))  # the three length classes, their ends half the time
            L = int(rng.choice(SOUP_LENGTHS[2 * cls: 2 * cls + 2])) if rng.random() < 0.5 else int(rng.integers((3, 11, 19)[cls], (11, 19, 275)[cls]))
            if kind == 2:
                b.match(int(rng.integers(1, 129)), L)
            else:
                b.rep(int(rng.integers(0, 4)), L)
    return b


@functools.lru_cache(maxsize=None)
def token_soup(C=520):
    rng = np.random.default_rng(32)
    return Streams([("soup %d" % c,) + soup_tokens(rng, Bits(), int(rng.integers(1, 121))).stream() for c in range(C)], 32)


def cut_stream():
    """102 bits: raw literals, list codes, a new-offset match with a long length, rep(0, 274), match(128, 19)"""
    return Bits().raw(0x61).raw(0x62).lst(0).raw(0x63).lst(1).raw(0x64).match(2, 40).rep(0, 274).match(128, 19)


@functools.lru_cache(maxsize=None)
def every_cut():
    """the stream above cut at every bit length 0 .. n, the bytes kept: one channel per cut"""
    b = cut_stream()
    return Streams([("cut to %d of %d bits" % (b.n - cut, b.n),) + b.stream(cut) for cut in range(b.n, -1, -1)], 33)


def named_items():
    items = [
        ("rep(0, 6) before any offset was set: six zero bytes, offset 0 acts as 128",) + Bits().rep(0, 6).raw(0x41).stream(),
        ("rep(0, 274) before any offset was set, after 130 literals: the byte 128 back",) +
        soup_literals(130).rep(0, 274).raw(0x41).stream(),
        ("rep(3, 20) with only two offsets set",) + Bits().raw(1).raw(2).raw(3).raw(4).match(1, 3).match(2, 4).rep(3, 20).rep(2, 5).rep(1, 3).raw(9).stream(),
        ("lst(18) on an empty list, raw(0), lst(0)",) + Bits().lst(18).raw(0).lst(0).raw(7).lst(1).lst(0).stream(),
        ("lst(18) 70 times on an empty list: the bubble-up goes past the two entries read ahead",) + repeat_lst(Bits(), 18, 70).raw(5).lst(0).lst(17).stream(),
        ("lst(10) 70 times behind four literals",) + repeat_lst(Bits().raw(65).raw(66).raw(65).raw(67), 10, 70).raw(0).raw(65).lst(3).stream(),
        ("an empty stream", b"", 0),
        ("37 zero bits", bytes(5), 37),
        ("one set bit", b"\x80", 1),
    ]
    for i in range(19):  # the last code is list code i with its last bit missing: the channel ends silently
        items.append(("raw, raw, lst(1), lst(%d) one bit short" % i,) + Bits().raw(0x41).raw(0x42).lst(1).lst(i).stream(cut=1))
    return items


def soup_literals(count):
    b = Bits()
    for i in range(count):
        b.raw(1 + (i * 7) % 255)
    return b


def repeat_lst(b, i, times):
    for _ in range(times):
        b.lst(i)
    return b


@functools.lru_cache(maxsize=None)
def named():
    return Streams(named_items(), 34)


# ---- (c) the checker -----------------------------------------------------------------------------------------------------------
def check(decode, streams, form="clean", stride=None):
    """decode(slabs, bits, stride) -> (out uint8 [C][stride], lens [C], err [C]).  Every channel: status 0, the oracle's length,
    the oracle's bytes.  Returns the arrays."""
    stride = streams.stride() if stride is None else stride
    out, lens, err = decode(streams.slabs[form], streams.bits, stride)
    for c in range(streams.C):
        want = streams.want[c]
        tag = (form, c, streams.name[c], int(streams.bits[c]))
        assert len(want) <= stride, tag
        assert err[c] == 0, (tag, int(err[c]))
        assert int(lens[c]) == len(want), (tag, int(lens[c]), len(want))
        got = out[c, : len(want)].tobytes()
        assert got == want, (tag, "first difference at byte %d of %d" % (next(i for i in range(len(want)) if got[i] != want[i]), len(want)))
    return out, lens, err


def check_both(decode, streams, stride=None):
    """the checker on both forms; the two results are the same arrays"""
    a = check(decode, streams, "clean", stride)
    b = check(decode, streams, "garbage", stride)
    assert all((x == y).all() for x, y in zip(a, b)), "the result depends on what lies beyond the stream's exact length"
    return b


# ---- (e) the compiled reference ------------------------------------------------------------------------------------------------
def check_reference(streams, channels):
    """the restatement against the compiled reference, where that is built, on channels the reference defines: it reads
    uninitialised memory for list entries never used, and maybe for history never written, so only streams that do neither"""
    for c in channels:
        n = int(streams.bits[c])
        ret, d, dn, _ = orc.ref_run_chain(streams.slabs["clean"][c, : (n + 7) // 8].tobytes(), n, ["decode lzmh"])
        assert ret == 0 and dn % 8 == 0 and d[: dn // 8] == streams.want[c], (c, streams.name[c])


# ---- the end of the row --------------------------------------------------------------------------------------------------------
BOUNDARY_STRIDE = 536  # a multiple of 8
CANARY = 0xA5


@functools.lru_cache(maxsize=None)
def boundary_streams():
    """Copy-grid channels around the end of a row of BOUNDARY_STRIDE bytes, each followed by a short healthy neighbour:
      * decoded lengths stride - 9 .. stride + 9 with a 274-byte match (p = len - 283 literals in front, 9 behind), for
        offsets on the period path, beyond it and at the ring's full reach;
      * a 274-byte match that begins 1 .. 273 bytes before the end of the row and runs across it.
    The neighbours decode to 20 bytes within their first passes, long before an overflowing lane of the same wave reaches
    the end of its row: a byte written past a row's end lands on bytes a neighbour has already written."""
    cells = [(o, 274, BOUNDARY_STRIDE + d - 283) for d in range(-9, 10) for o in (1, 3, 7, 8, 64, 128)]
    cells += [(o, 274, BOUNDARY_STRIDE - before) for before in (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 100, 256, 265, 272, 273) for o in (1, 5, 128)]
    grid = grid_of(cells, seed=35)
    items = []
    for c in range(grid.C):
        n = int(grid.bits[c])
        items.append((grid.name[c], grid.slabs["clean"][c, : (n + 7) // 8].tobytes(), n))
        b = Bits()
        for k in range(20):
            b.raw(1 + (c + 11 * k) % 255)
        items.append(("neighbour of " + grid.name[c],) + b.stream())
    return Streams(items, 35)


def check_boundary(decode_rows):
    """decode_rows(slabs, bits, stride, rows) -> (lens, err), decoding into rows uint8 [C + 1][stride], which come filled with
    the canary: one canary row behind the last channel's.  len <= stride: status 0, the length, the bytes, and behind the
    writer's last 8-byte store the canary.  len > stride: ERROR_MEMORY and length 0, whatever the row holds.  The canary
    row keeps the canary."""
    streams, stride = boundary_streams(), BOUNDARY_STRIDE
    lengths = set(len(w) for w in streams.want)
    assert all(stride + d in lengths for d in range(-9, 10)) and max(lengths) == stride + 282
    over = 0
    for form in ("clean", "garbage"):
        rows = np.full((streams.C + 1, stride), CANARY, dtype=np.uint8)
        lens, err = decode_rows(streams.slabs[form], streams.bits, stride, rows)
        assert (rows[streams.C] == CANARY).all(), "the canary row behind the last row was written"
        for c in range(streams.C):
            want, tag = streams.want[c], (form, c, streams.name[c], len(streams.want[c]), stride)
            if len(want) > stride:
                over += 1
                assert err[c] == orc.ERROR_MEMORY and lens[c] == 0, (tag, int(err[c]), int(lens[c]))
                continue
            assert err[c] == 0 and int(lens[c]) == len(want), (tag, int(err[c]), int(lens[c]))
            assert rows[c, : len(want)].tobytes() == want, tag
            # the writer's last store is 8 bytes wide: zeros up to the next multiple of 8, nothing behind
            assert (rows[c, (len(want) + 7) // 8 * 8:] == CANARY).all(), (tag, "bytes behind the channel's last store were written")
    assert over == 2 * (9 * 6 + 16 * 3)


def longest_match_strings():
    """32 texts for the ENCODER: a match of the maximum length (274) that begins at every position modulo 16 -- the window a
    lane reloads starts at (P - 128) rounded down to 16, and whatever the alignment it has to hold the whole match"""
    rng = np.random.default_rng(3)
    strings = []
    for k in range(32):
        head = bytes(rng.integers(0, 256, 130 + k, dtype=np.uint8))
        strings.append(head + bytes([65 + k]) * (700 + 3 * k) + head[:40])
    return strings
