"""Shared by tests/test_lzmh_encoder_host.py and tests/test_gpu_lzmh_encoder.py: a seeded corpus of TEXTS that steers the LZMH
encoder (lzmh_searching_wave and lzmh_coding_wave, data-compressor_amd/csrc/lzmh_kernels.hpp) onto the paths healthy text
never takes, the conditions -- computed from the oracle's stream and a replay of the reference's parse alone, never from
anything a kernel reports -- that say the corpus really does so, and the checkers that hold an encoder to the oracle's
stream on every channel.  In the manner of tests/encoder_regimes_common.py and tests/lzmh_hostile_common.py.

A channel's text depends on (SEED, c, n) alone, so a smaller batch is the head of a larger one; channel c is of kind c % 8
(KINDS), so every wave of 64 lanes holds every kind next to a healthy lane:
  0 meter lines   lzmh_hostile_common.text_of(rng, 0, .): the control
  1 ladder        blocks of a random word X written as X[:a] s, ..., X[:3] s, X, the prefixes shrinking towards X and every
                  s a byte of its own from outside X's alphabet: at the last X the nearest candidate is the shortest and
                  every farther one is longer, so `best` improves J = 8..12 times in one step, over several passes of six
                  and several mask registers; the prefixes reach 14 .. 24 bytes, so the `longer` round (bytes 8..15, then
                  byte by byte) runs for the far ones.  A block's history stays within the 128 bytes of reach
  2 deep list     60 distinct symbols once (12 meet a full list), then mostly symbols that sit at list positions 19..47
                  or were dropped, led by a model of the list and chosen so that 3-byte repeats within reach are rare:
                  positions 19..47 are found, counted and bubbled but coded raw; literals dropped on a full list; bubbles
                  through long runs of equal counts
  3 soup text     lzmh_hostile_common.soup_tokens assembled and DECODED BY THE ORACLE; the text that comes out is the input:
                  matches of every length class at its edges, offsets 1 and 128, 274-byte matches chained, steps with more
                  than 32 and up to 128 candidates (the runs of zeros that matches into unwritten history leave)
  4 four offsets  130 random bytes, then copies of seeded length from four fixed distances, one literal that ends each
                  copy between them: the 2nd, 3rd and 4th recent-offset code, and eviction by a fifth distance now and then
  5 runs          zeros, one repeated byte, and periods 2..9, of lengths such that the last match of a run ends in each
                  length class: 274 bytes a step, a window reload every step, the reload-and-retry path next to lanes in
                  the middle of a step
  6 near misses   the alphabets {0x60, 0x61} and {0x00, 0x01} at random, evenly and skewed: bytes that differ in the lowest bit
                  next to equal bytes are what lz_zero_bytes_approx flags falsely; more than 6 candidates in one mask
                  register, more than 32 in a step, true matches of exactly 2 bytes
  7 switch        a third of kind 1, a third of kind 5, a third of kind 2: a list and an offset cache built under one regime
                  and used under another

Lengths: n, except that every other group of eight channels is cut at a seeded point in [n / 10, n] (so that a match in
progress could run on into what lies behind the length), that channel c with c % 7 == 3 has a length of SPECIAL, by index (as
make_strings of tests/test_gpu_lzmh.py picks them; those beyond the stride give way to n), and that channel c with
c % 10 == 9 has the stride's length exactly.  The stride follows from n alone (stride_of).

The rows come in three FORMS for the same lengths: `clean` (zeros behind the length), `garbage` (random bytes behind it),
`continued` (the kind's text simply goes on behind the length, up to the stride).  The oracle sees the first len bytes; an
encoder's result must not depend on the form."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import lzmh_hostile_common as lc
from oracle import orc

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
REPLAY_SO = os.path.join(ORACLE_DIR, "liblzmhreplay.so")

KINDS = ("meter lines", "ladder", "deep list", "soup text", "four offsets", "runs", "near misses", "switch")
FORMS = ("clean", "garbage", "continued")
SPECIAL = (0, 1, 2, 3, 16, 402, 403, 404)
SEED = 2030  # (the first from 2026 on with a dozen channels of corpus(70, 600) between "must fit" and "must err", over CAPS)
CANARY = 0xA5
CAPS = (48, 64, 128, 208, 256, 304, 400)  # the short slabs, bytes; 48 is the entry point's minimum
SLAB_N = 600  # the corpus of the slab-end check

EVENTS = ("steps with >= 7 improvements", "steps with > 32 candidates", "recent offset 1", "recent offset 2", "recent offset 3",
          "length 3", "length 10", "length 11", "length 18", "length 19", "length 274", "offset 1", "offset 128",
          "list hits at 19 or deeper", "literals on a full list", "bubbles past > 3 entries")
# What the oracle alone says about corpus(C, n), event by event in the order of EVENTS, as counted when the corpus was
# written; check_not_vacuous asserts three quarters of each (numpy promises the same random stream only within a version
# line) and never less than one.  The rows of n = 40 are there for the ends of texts -- a few codes and an end, the row's
# end a few bytes on --, not for the rare paths: a text of 40 bytes holds no ladder, no 274-byte match, no offset of 128 and
# no list of 48, so those rows record what 40 bytes reach and their zeros are not asserted.
ORACLE_COUNTS = {
    (70, 40): (5, 0, 5, 2, 0, 20, 5, 3, 0, 3, 0, 27, 0, 5, 0, 37),
    (70, 600): (58, 107, 104, 80, 65, 205, 62, 66, 34, 36, 15, 68, 7, 2357, 1771, 2096),
    (130, 40): (7, 0, 10, 3, 1, 34, 10, 10, 0, 5, 0, 47, 0, 10, 0, 61),
    (130, 600): (108, 193, 176, 134, 117, 362, 109, 126, 69, 68, 25, 122, 8, 4477, 3530, 3991),
    (130, 3000): (474, 739, 777, 691, 629, 1665, 591, 661, 364, 340, 176, 354, 20, 23154, 17701, 16196),
    (300, 600): (244, 399, 411, 297, 259, 838, 263, 289, 157, 153, 54, 287, 18, 11048, 8424, 9792),
}


def stride_of(n):
    """the row of a batch of texts of n bytes: a multiple of 16 that holds n and, from 402 on, the special lengths"""
    return (max(n, 404 if n >= 402 else 0) + 15) // 16 * 16


def worst_case_bytes(stride):
    """dega_hip_lzmh_worst_case_bytes, restated (the GPU tests hold it to the library's)"""
    return ((stride * 10 + 7) // 8 + 32 + 15) // 16 * 16


# ---- the replay ------------------------------------------------------------------------------------------------------------
_lib = None
COLS = 10


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(REPLAY_SO):
            subprocess.run(["make", "-s", "-C", ORACLE_DIR, "oracle"], check=True)
        L = C.CDLL(REPLAY_SO)
        L.lzr_replay.restype = C.c_int64
        L.lzr_replay.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        _lib = L
    return _lib


class Trace:
    """The reference's parse and coder replayed on one text (oracle/lzmh_replay.c): nbits, stream, and per step pos, length,
    offset (0, 0: a literal), code (0..3 the k-th most recent offset, 4 a new offset, 5 a literal by list position, 6 a raw
    literal), cand (offsets within reach whose three bytes equal the next three), improved (how often the best length
    rose), sym, found (the list position, -1: not in the list), dropped (not in the list, and the list full), bubble
    (entries passed on the way to the front)."""

    def tokens(self):
        """the steps as the tokenizer names them"""
        out = []
        for code, length, offset, sym, found in zip(self.code.tolist(), self.length.tolist(), self.offset.tolist(), self.sym.tolist(), self.found.tolist()):
            out.append(("rep", code, length, offset) if code < 4 else ("match", offset, length) if code == 4 else ("lst", found) if code == 5 else ("raw", sym))
        return out

    def events(self):
        m = self.length > 0
        return np.array([(self.improved >= 7).sum(), (self.cand > 32).sum(), (m & (self.code == 1)).sum(), (m & (self.code == 2)).sum(),
                         (m & (self.code == 3)).sum()] + [(self.length == L).sum() for L in (3, 10, 11, 18, 19, 274)] +
                        [(self.offset == 1).sum(), (self.offset == 128).sum(), (self.found >= 19).sum(), (self.dropped != 0).sum(), (self.bubble > 3).sum()],
                        dtype=np.int64)


def replay(text):
    n = len(text)
    buf = np.frombuffer(text, dtype=np.uint8) if n else np.zeros(1, dtype=np.uint8)
    rec = np.zeros((n + 1, COLS), dtype=np.int32)
    cap = 10 * n // 8 + 8
    stream = np.zeros(cap, dtype=np.uint8)
    nbits = C.c_uint64(0)
    steps = lib().lzr_replay(buf.ctypes.data, n, rec.ctypes.data, n + 1, stream.ctypes.data, cap, C.byref(nbits))
    assert steps >= 0
    t = Trace()
    rec = rec[:steps]
    t.nbits, t.stream = int(nbits.value), stream[: (int(nbits.value) + 7) // 8].tobytes()
    t.pos, t.length, t.offset, t.code, t.cand, t.improved, t.sym, t.found, t.dropped, t.bubble = (rec[:, k].copy() for k in range(COLS))
    return t


# ---- the tokenizer ---------------------------------------------------------------------------------------------------------
LIST_CODES = {format(code, "0%db" % k): i for i, (code, k) in ((i, lc.list_code(i)) for i in range(19))}


def tokenize(stream, nbits):
    """An encoder's stream, code by code: ("raw", byte) | ("lst", list position) | ("match", offset, length): a new offset |
    ("rep", k, length, offset): the k-th most recent offset, resolved.  The inverse of lzmh_hostile_common.Bits; the prefix
    code is complete, so whatever the first bits are, exactly one code begins with them."""
    s = "".join(format(b, "08b") for b in stream)[:nbits]
    at, out, mru = 0, [], [0, 0, 0, 0]

    def take(k):
        nonlocal at
        assert at + k <= nbits, "the stream ends inside a code"
        at += k
        return int(s[at - k: at], 2)

    while at < nbits:
        if s[at] == "1":
            k = next(k for k in (4, 5, 6, 7, 8) if s[at: at + k] in LIST_CODES)
            out.append(("lst", LIST_CODES[s[at: at + k]]))
            at += k
            continue
        if s[at + 1] == "0":
            out.append(("raw", take(10) & 0xFF))
            continue
        at += 2
        if take(1) == 0:
            rep, offset = None, take(7) + 1
            mru = [offset] + mru[:3]
        else:
            rep = 0 if take(1) == 0 else 1 if take(1) == 0 else 2 + take(1)
            offset = mru.pop(rep)
            mru.insert(0, offset)
        length = take(3) + 3 if take(1) == 0 else take(3) + 11 if take(1) == 0 else take(8) + 19
        out.append(("match", offset, length) if rep is None else ("rep", rep, length, offset))
    return out


def assemble(tokens):
    """tokens -> (bytes, bits), with the assembler of lzmh_hostile_common"""
    b = lc.Bits()
    for t in tokens:
        if t[0] == "raw":
            b.raw(t[1])
        elif t[0] == "lst":
            b.lst(t[1])
        elif t[0] == "match":
            b.match(t[1], t[2])
        else:
            b.rep(t[1], t[2])
    return b.stream()


# ---- the texts -------------------------------------------------------------------------------------------------------------
def ladder(rng, total):
    out = bytearray()
    while len(out) < total:
        step = int(rng.integers(1, 4))
        lengths = [3]
        while sum(k + 1 for k in lengths) + lengths[-1] + step + 1 <= 124:
            lengths.append(lengths[-1] + step)
        first = int(rng.integers(97, 110))
        word = bytes(rng.integers(first, first + 13, lengths[-1] + int(rng.integers(2, 9)), dtype=np.uint8))
        seps = rng.permutation(np.arange(128, 256))[: len(lengths)].tolist()
        for k, s in zip(reversed(lengths), seps):
            out += word[:k] + bytes([s])
        out += word
    return bytes(out[:total])


def deep_list(rng, total):
    """a model of the frequency list leads the choice (every byte is taken for a literal, which it nearly always is)"""
    symbols = rng.permutation(256)[:60].tolist()
    out = list(symbols)
    entries = [[s, 1] for s in symbols[:48]]  # [symbol, count], as the list stands after the first 60 bytes
    dropped = symbols[48:]
    seen = {}
    for i in range(2, len(out)):
        seen[tuple(out[i - 2: i + 1])] = i
    while len(out) < total:
        for _ in range(4):  # a few tries for a byte that completes no 3-byte repeat within reach
            u = rng.random()
            if u < 0.70:
                b = entries[int(rng.integers(19, 48))][0]
            elif u < 0.85:
                b = dropped[int(rng.integers(0, len(dropped)))]
            else:
                b = entries[int(rng.integers(0, 19))][0]
            if len(out) - seen.get((out[-2], out[-1], b), -1000) > 130:
                break
        out.append(b)
        seen[tuple(out[-3:])] = len(out) - 1
        i = next((i for i, e in enumerate(entries) if e[0] == b), None)
        if i is not None:
            nc = entries[i][1] + 1
            while i > 0 and nc > entries[i - 1][1]:
                entries[i][0] = entries[i - 1][0]
                i -= 1
            entries[i] = [b, nc]
    return bytes(out[:total])


def soup_text(rng, total):
    b = lc.Bits()
    while True:
        lc.soup_tokens(rng, b, 8 + total // 16)
        text = lc.oracle_decode(*b.stream())
        if len(text) >= total:
            return text[:total]


def four_offsets(rng, total):
    out = bytearray(rng.integers(0, 256, 130, dtype=np.uint8).tobytes())
    dist = (rng.permutation(126)[:4] + 3).tolist()  # the four, most recent first
    while len(out) < total:
        if rng.random() < 0.1:  # a fifth distance: the oldest of the four is evicted
            d = int(rng.integers(3, 129))
            dist = [d] + [x for x in dist if x != d][:3]
        else:
            k = int(rng.integers(0, 4))
            d = dist.pop(k)
            dist.insert(0, d)
        L = int(rng.choice((3, 4, 10, 11, 18, 19, 30))) if rng.random() < 0.7 else int(rng.integers(3, 60))
        for _ in range(L):
            out.append(out[-d])
        lit = int(rng.integers(0, 256))
        out.append(lit if lit != out[-d] else lit ^ 0x80)  # the copy ends here
    return bytes(out[:total])


RUN_TAILS = (3, 10, 11, 18, 19, 274, 275, 277, 284, 285, 292, 293, 548, 570)  # a run of period p is p + one of these long


def runs(rng, total, variant):
    if variant == 0:
        return bytes(total)
    if variant == 1:
        return bytes([int(rng.integers(1, 256))]) * total
    out = bytearray()
    turn = int(rng.integers(0, len(RUN_TAILS)))
    while len(out) < total:
        p = int(rng.integers(1, 10))
        unit = bytes(rng.integers(0, 256, p, dtype=np.uint8))
        length = p + RUN_TAILS[turn % len(RUN_TAILS)]
        turn += 1
        out += (unit * (length // p + 1))[:length]
        out.append(int(rng.integers(0, 256)))
    return bytes(out[:total])


def near_misses(rng, total, variant):
    low = (0x60, 0x00)[variant]
    out = bytearray()
    while len(out) < total:
        p = (0.5, 0.85, 0.15)[int(rng.integers(0, 3))]
        out += bytes((low + (rng.random(64) >= p)).astype(np.uint8))
    return bytes(out[:total])


def text_of(c, n):
    """channel c's text, stride_of(n) bytes of it: the channel's length decides how much of it the oracle sees"""
    rng = np.random.default_rng([SEED, c, n])
    total, k, variant = stride_of(n), c % 8, c // 8
    if k == 0:
        return lc.text_of(rng, 0, total)
    if k == 1:
        return ladder(rng, total)
    if k == 2:
        return deep_list(rng, total)
    if k == 3:
        return soup_text(rng, total)
    if k == 4:
        return four_offsets(rng, total)
    if k == 5:
        return runs(rng, total, variant % 4)
    if k == 6:
        return near_misses(rng, total, variant % 2)
    a, b = total // 3, 2 * (total // 3)
    return ladder(rng, a) + runs(rng, b - a, 2) + deep_list(rng, total - b)


def length_of(c, n):
    stride = stride_of(n)
    if c % 10 == 9:
        return stride
    if c % 7 == 3 and SPECIAL[(c // 7) % len(SPECIAL)] <= stride:
        return SPECIAL[(c // 7) % len(SPECIAL)]
    if (c // 8) % 2:
        return int(np.random.default_rng([SEED, c, n, 1]).integers(n // 10, n + 1))
    return n


class Corpus:
    """text[c] (stride bytes), lens uint64 [C], kind [C], rows[form] uint8 [C][stride]; the oracle's streams (want[c] =
    (bytes, bits)), the replay's traces (trace(c)) and the tokens (tokens(c)), made on first use and kept.  A trace is handed
    out only after its stream has been found to be the oracle's, bit for bit.  Read-only."""

    def __init__(self, Cn, n):
        self.C, self.n, self.stride = Cn, n, stride_of(n)
        self.kind = np.arange(Cn) % 8
        self.text = [text_of(c, n) for c in range(Cn)]
        self.lens = np.array([length_of(c, n) for c in range(Cn)], dtype=np.uint64)
        assert all(len(t) == self.stride for t in self.text) and int(self.lens.max()) == self.stride
        continued = np.stack([np.frombuffer(t, dtype=np.uint8) for t in self.text])
        behind = np.arange(self.stride)[None, :] >= self.lens[:, None].astype(np.int64)
        garbage = np.where(behind, np.random.default_rng([SEED, Cn, n, 2]).integers(0, 256, continued.shape, dtype=np.uint8), continued)
        self.rows = {"clean": np.where(behind, np.uint8(0), continued), "garbage": garbage, "continued": continued.copy()}
        for a in (self.kind, self.lens) + tuple(self.rows.values()):
            a.setflags(write=False)
        self._want, self._traces = None, {}

    def seen(self, c):
        """what the oracle sees of channel c"""
        return self.text[c][: int(self.lens[c])]

    @property
    def want(self):
        if self._want is None:
            self._want = [lc.oracle_encode(self.seen(c)) for c in range(self.C)]
        return self._want

    def want_words(self):
        """W: the oracle's streams rounded up to whole 32-bit words, in bytes"""
        return np.array([(nb + 31) // 32 * 4 for _, nb in self.want], dtype=np.int64)

    def trace(self, c):
        if c not in self._traces:
            t = replay(self.seen(c))
            assert (t.stream, t.nbits) == self.want[c], ("the replay's stream is not the oracle's", c, KINDS[c % 8])
            self._traces[c] = t
        return self._traces[c]

    def tokens(self, c):
        return tokenize(*self.want[c])

    def events(self, channels=None):
        """EVENTS counted over the batch (or over some of its channels), from the replay"""
        return sum((self.trace(c).events() for c in (range(self.C) if channels is None else channels)), np.zeros(len(EVENTS), dtype=np.int64))

    def of_kind(self, *kinds):
        return [c for c in range(self.C) if self.kind[c] in kinds]

    def waves(self):
        return [range(w, min(w + 64, self.C)) for w in range(0, self.C, 64)]


@functools.lru_cache(maxsize=None)
def corpus(Cn, n):
    return Corpus(Cn, n)


# ---- the conditions ----------------------------------------------------------------------------------------------------------
def check_not_vacuous(Cn, n):
    """the oracle alone: the corpus reaches what it was built to reach, and the control does not.  -> the counts, as EVENTS"""
    corp = corpus(Cn, n)
    got, table = corp.events(), ORACLE_COUNTS[(Cn, n)]
    for k, name in enumerate(EVENTS):
        if n >= SLAB_N or table[k] > 0:
            assert got[k] >= max(1, (3 * table[k] + 3) // 4), ((Cn, n), name, int(got[k]), table[k])
    for wave in corp.waves():
        if len(wave) >= 8:
            assert sorted(set(corp.kind[list(wave)].tolist())) == list(range(8)), ("a wave without one of the kinds", wave)
    if n == SLAB_N:  # the control: none of the deep-list or many-improvement events in healthy text, or the corpus would prove nothing about it
        control = dict(zip(EVENTS, corp.events(corp.of_kind(0)).tolist()))
        for name in ("steps with >= 7 improvements", "list hits at 19 or deeper", "literals on a full list"):
            assert control[name] == 0, (name, control[name])
    return got


# ---- the checkers ------------------------------------------------------------------------------------------------------------
def check(encode, corp, form, cap=None):
    """encode(rows uint8 [C][stride], lens uint64 [C], cap) -> (out uint8 [C][cap], bits [C], err [C]).  Every channel: status
    0, the oracle's exact bit length, the oracle's bytes.  Returns the arrays."""
    cap = worst_case_bytes(corp.stride) if cap is None else cap
    out, bits, err = (np.asarray(a) for a in encode(corp.rows[form], corp.lens, cap))
    assert out.shape == (corp.C, cap)
    for c in range(corp.C):
        want, nb = corp.want[c]
        tag = (form, c, KINDS[c % 8], int(corp.lens[c]))
        assert err[c] == 0, (tag, int(err[c]))
        assert int(bits[c]) == nb, (tag, int(bits[c]), nb)
        got = out[c, : len(want)].tobytes()
        assert got == want, (tag, "first difference at byte %d of %d" % (next(i for i in range(len(want)) if got[i] != want[i]), len(want)))
    return out, bits, err


def check_all_forms(encode, corp, cap=None):
    """the checker on the three forms; bits, statuses and stream bytes are the same arrays"""
    results = [check(encode, corp, form, cap) for form in FORMS]
    nbytes = (np.asarray(results[0][1]).astype(np.int64) + 7) // 8
    for form, (out, bits, err) in zip(FORMS[1:], results[1:]):
        assert (np.asarray(bits) == np.asarray(results[0][1])).all() and (np.asarray(err) == np.asarray(results[0][2])).all(), form
        for c in range(corp.C):
            assert (out[c, : nbytes[c]] == results[0][0][c, : nbytes[c]]).all(), ("the stream depends on what lies behind the length", form, c)
    return results[0]


def slab_bands(corp):
    """per cap of CAPS: (channels that must fit, that may do either, that must err), from the oracle's lengths alone"""
    W = corp.want_words()
    return {cap: (np.flatnonzero(W + 16 <= cap), np.flatnonzero((W + 16 > cap) & (W <= cap)), np.flatnonzero(W > cap)) for cap in CAPS}


def check_slab_is_not_vacuous(corp):
    bands = slab_bands(corp)
    for cap, (fit, either, over) in bands.items():
        assert len(fit) >= 1 and len(over) >= 1, (cap, len(fit), len(over))
    between = sum(len(either) for _, either, _ in bands.values())
    assert between >= 10, between
    return {cap: tuple(len(b) for b in band) for cap, band in bands.items()}


def check_slab_end(encode_rows, Cn, form="continued"):
    """encode_rows(rows, lens, cap, out) -> (bits, err), encoding into out uint8 [C + 1][cap], which comes filled with the canary:
    one canary row behind the last channel's.  With W the oracle's stream in whole 32-bit words (bytes):
      W + 16 <= cap   status 0, the oracle's bits and bytes (what the two tests of lzmh_coding_wave guarantee: its 16-byte
                      stores end at or before 16 * (full words / 4) <= W, and the last of them is let through when 16 more
                      bytes fit behind it; finish needs one word behind the full ones)
      W > cap         ERROR_MEMORY and out_bits 0
      in between      either; with status 0 the bits and bytes are the oracle's
    Always: the canary row keeps the canary, and a channel that fits keeps it behind its last word."""
    corp = corpus(Cn, SLAB_N)
    check_slab_is_not_vacuous(corp)
    for cap, (fit, either, over) in slab_bands(corp).items():
        out = np.full((corp.C + 1, cap), CANARY, dtype=np.uint8)
        bits, err = (np.asarray(a) for a in encode_rows(corp.rows[form], corp.lens, cap, out))
        assert (out[corp.C] == CANARY).all(), (cap, "the canary row behind the last slab was written")
        for c in range(corp.C):
            want, nb = corp.want[c]
            tag = (cap, form, c, KINDS[c % 8], "stream of %d bits" % nb)
            if c in over or (c in either and err[c] != 0):
                assert err[c] == orc.ERROR_MEMORY and bits[c] == 0, (tag, int(err[c]), int(bits[c]))
                continue
            assert err[c] == 0 and int(bits[c]) == nb, (tag, int(err[c]), int(bits[c]))
            assert out[c, : len(want)].tobytes() == want, tag
            assert (out[c, (nb + 31) // 32 * 4:] == CANARY).all(), (tag, "bytes behind the channel's last word were written")


def tightest_fit():
    """(rows uint8 [1][256], lens, cap): the 256 byte values once each -- no repeat, and no symbol in the list but at its own
    first sight, so every byte costs 10 bits -- at len == stride and cap = the worst case of that stride, which 2560 bits
    + the 32 bytes the kernel keeps free fill to the byte: "never overflows" at its tightest"""
    text = np.random.default_rng([SEED, 256]).permutation(256).astype(np.uint8)
    want, nb = lc.oracle_encode(text.tobytes())
    assert nb == 2560 and worst_case_bytes(256) == 320 + 32
    return text[None, :].copy(), np.array([256], dtype=np.uint64), worst_case_bytes(256), (want, nb)
