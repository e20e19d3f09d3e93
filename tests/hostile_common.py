"""Shared by tests/test_decode_hostile_host.py and tests/test_gpu_decode_hostile.py: a seeded corpus of damaged DEGA
streams and the checker that holds a variable-count decoder to the oracle's verdict on every one of them.

The valid streams come from the oracle (oracle/orc.py), never from the kernels, so the corpus is the same wherever it is
made.  Channel c is of kind c % 10 (KINDS below): every wave of 64 lanes holds every kind next to healthy lanes.  The
oracle's verdict on a stream is the stage chain `decode bac` -> `decode seg` -> `decode diff`; a damaged stream ends in one
of three ways, in comparable shares: bac refuses it (ERROR_INVALID_FORMAT, -3: more than 14 phantom bits, bac.c:171-186),
seg refuses it (ERROR_LIBRARY_CALL, -11: a short read inside a codeword; or -3: a zero prefix beyond the cap, seg.c:55-56),
or the chain accepts it and returns samples no encoder meant -- which pins a decoder bit for bit on inputs no encoder
produces.

Two forms of every corpus: `clean` (what lies beyond a stream's exact length is whatever the damage left there -- zeros,
or, for the shortened kinds, the rest of the stream) and `garbage` (every bit beyond the exact length, up to the end of
the slab, random).  A decoder's result must not depend on the form (the loading wave clears the bits beyond
the exact length and puts zeros after the last word)."""
import functools

import numpy as np

from oracle import orc

KINDS = ("healthy", "flip anywhere", "flip in the first 64 bits", "flip in the last 16 bits", "4 random bytes", "bits shortened by 1..40",
         "bits cut to a random length", "bits lengthened over zero bytes", "every byte random", "constant bytes / no bits")
CONSTANT_BYTES = (0x00, 0xFF, 0xAA)  # kind 9 cycles through these and `bits = 0`
CONSTANT_MAX_BITS = 4096
EXCUSED_CAP = 0.02 # of the channels the oracle refuses, per call: the share that may report ERROR_MEMORY instead (see check)

# What the oracle alone says about each (C, valuesize, adaptive) corpus, its lengths T taken together: (accepted damaged
# channels whose samples differ from the original, channels refused with -3, channels refused with -11), as counted when
# the corpus was written.  `check_not_vacuous` asserts three quarters of each (numpy promises the same random stream only
# within a version line).  Every class is well above a tenth of the damaged channels but one: under the adaptive model a
# damaged stream rarely finds an EOF symbol at all, so most of what seg would refuse with -11 bac has refused with -3
# before it.  The static model has no state to derail; its -3 come from the cuts (kinds 5, 6, 9).
#   C = 70: T = 33 and 300, 126 damaged channels (the emulator);  C = 130: T = 33 and 300, 234 damaged channels, at value
#   size 32 also T = 3000, 351 damaged channels (the GPU)
ORACLE_COUNTS = {
    (70, 32, 1): (41, 60, 10), (70, 32, 0): (46, 35, 30),
    (70, 12, 1): (37, 66, 9), (70, 12, 0): (49, 33, 29),
    (70, 40, 1): (42, 61, 8), (70, 40, 0): (54, 36, 22),
    (70, 64, 1): (42, 55, 14), (70, 64, 0): (49, 38, 25),
    (130, 32, 1): (104, 170, 34), (130, 32, 0): (145, 102, 64),
    (130, 31, 1): (75, 116, 17), (130, 31, 0): (83, 68, 56),
    (130, 12, 1): (65, 120, 20), (130, 12, 0): (102, 66, 40),
    (130, 5, 1): (79, 121, 7), (130, 5, 0): (125, 69, 11),
    (130, 33, 1): (76, 114, 18), (130, 33, 0): (88, 70, 49),
    (130, 48, 1): (64, 110, 32), (130, 48, 0): (90, 69, 49),
    (130, 64, 1): (73, 115, 19), (130, 64, 0): (89, 71, 47),
}


def lengths(C, vs):
    return (33, 300, 3000) if (C == 130 and vs == 32) else (33, 300)


def pack_be(vals, vs):
    v = np.asarray(vals, dtype=np.uint64)
    bits = np.zeros(len(v) * vs, dtype=np.uint8)
    for k in range(vs):
        bits[k::vs] = (v >> np.uint64(vs - 1 - k)) & np.uint64(1)
    return np.packbits(bits).tobytes(), len(v) * vs


def unpack_be(data, nbits, vs):
    """nbits of big-endian valuesize-bit fields -> uint64 (a trailing partial field is dropped, as `decode diff` writes none)"""
    n = nbits // vs
    if vs == 32:
        return np.frombuffer(data, dtype=">u4", count=n).astype(np.uint64)
    if vs == 64:
        return np.frombuffer(data, dtype=">u8", count=n).astype(np.uint64)
    bits = np.unpackbits(np.frombuffer(data, dtype=np.uint8))[: n * vs].reshape(n, vs).astype(np.uint64)
    out = np.zeros(n, dtype=np.uint64)
    for k in range(vs):
        out |= bits[:, k] << np.uint64(vs - 1 - k)
    return out


def walks(rng, C, T, vs):
    """+-60 walks (narrower where the value size asks for it: a difference has to fit valuesize bits signed, and the first
    sample is differenced against 0, diff.c:11-18)"""
    step = min(60, max(1, (1 << vs) >> 3))
    base = min(30000, (1 << vs) >> 2)
    x = np.cumsum(rng.integers(-step, step + 1, (T, C)), axis=0) + base
    if vs < 32:
        x = x.clip(0, (1 << (vs - 1)) - 1)
    return x.astype(np.uint64)


def oracle_encode(x, vs, ad):
    """-> list of (bytes, nbits) per channel; every walk of `walks` is encodable"""
    T, C = x.shape
    if vs == 32:
        out, bits, err = orc.encode_batch_tc(x.astype(np.uint32).view(np.int32), ad)
        assert (err == 0).all()
        return [(out[c, : (int(bits[c]) + 7) // 8].tobytes(), int(bits[c])) for c in range(C)]
    res = []
    for c in range(C):
        d, n = pack_be(x[:, c], vs)
        for name in ("diff", "seg", "bac"):
            r, d, n = orc.stage(name, True, d, n, valuesize=vs, adaptive=ad)
            assert r == 0, (vs, ad, c, name, r)
        res.append((d[: (n + 7) // 8], n))
    return res


def oracle_verdict(data, nbits, vs, ad):
    """the stage chain on one stream -> (status, samples uint64 or None).  orc_bits_assign copies ceil(nbits / 8) bytes and
    clears the bits of the last one beyond nbits, so the oracle never sees what lies beyond the exact length."""
    d, n = bytes(data[: (nbits + 7) // 8]), nbits
    for name in ("bac", "seg", "diff"):
        r, d, n = orc.stage(name, False, d, n, valuesize=vs, adaptive=ad)
        if r != 0:
            return r, None
    return 0, unpack_be(d, n, vs)


def damage(rng, b, n, k, c):
    """the stream b (a bytearray) of n bits, damaged by kind k (KINDS); c picks among kind 9's variants.  -> (bytes, bits, what
    was done).  The bits beyond the new length keep whatever the damage left there."""
    what = ""
    if k in (1, 2, 3):
        lo, hi = (0, n) if k == 1 else (0, min(64, n)) if k == 2 else (max(0, n - 16), n)
        at = int(rng.integers(lo, hi))
        b[at // 8] ^= 0x80 >> (at % 8)
        what = "bit %d of %d flipped" % (at, n)
    elif k == 4:
        at = int(rng.integers(0, max(1, len(b) - 3)))
        b[at: at + 4] = bytes(rng.integers(0, 256, 4, dtype=np.uint8))[: len(b) - at]
        what = "bytes %d..%d random" % (at, at + 3)
    elif k == 5:
        cut = int(rng.integers(1, 41))
        what = "%d bits shortened by %d, bytes kept" % (n, cut)
        n = max(1, n - cut)
    elif k == 6:
        what = "%d bits cut" % n
        n = int(rng.integers(1, n))
        what += " to %d, bytes kept" % n
    elif k == 7:
        more = int(rng.integers(1, 65))
        what = "%d bits lengthened by %d over zero bytes" % (n, more)
        n += more
        b += bytes((n + 7) // 8 - len(b))
    elif k == 8:
        b = bytearray(rng.integers(0, 256, len(b), dtype=np.uint8).tobytes())
        what = "every byte random"
    elif k == 9:
        which = (c // 10) % 4
        if which == 3:
            n, what = 0, "healthy bytes, bits = 0"
        else:
            # (at most CONSTANT_MAX_BITS: the adaptive model decodes 0xFF bytes to thousands of seg bits per stream
            # bit, every one of which the oracle's bac stage writes out before it refuses the stream)
            n = min(n, CONSTANT_MAX_BITS)
            b = bytearray([CONSTANT_BYTES[which]]) * ((n + 7) // 8)
            what = "%d bits, every byte 0x%02X" % (n, CONSTANT_BYTES[which])
    return b, n, what


def slab_forms(rng, rows, bits, cap):
    """the streams `rows` (bytes each) of `bits` bits as slabs uint8 [C][cap] in the two forms: clean, and garbage -- every bit
    from a stream's exact length to the end of its slab random"""
    C = len(rows)
    clean = np.zeros((C, cap), dtype=np.uint8)
    for c in range(C):
        clean[c, : len(rows[c])] = np.frombuffer(rows[c], dtype=np.uint8)
    garbage = clean.copy()
    junk = rng.integers(0, 256, (C, cap), dtype=np.uint8)
    for c in range(C):
        n = int(bits[c])
        garbage[c, (n + 7) // 8:] = junk[c, (n + 7) // 8:]
        if n % 8:
            keep = (0xFF00 >> (n % 8)) & 0xFF
            garbage[c, n // 8] = (int(garbage[c, n // 8]) & keep) | (int(junk[c, n // 8]) & (0xFF ^ keep))
    return clean, garbage


class Corpus:
    """slabs[form] uint8 [C][cap], bits uint64 [C], kind [C], made_from[c] (a line of text), x uint64 [T][C] (the samples the
    healthy streams code), plus the oracle's verdicts, computed on first use and kept.  Arrays are read-only."""

    def __init__(self, C, T, vs, ad, seed=2024):
        self.C, self.T, self.vs, self.ad = C, T, vs, ad
        rng = np.random.default_rng([seed, C, T, vs, ad])
        self.x = walks(rng, C, T, vs)
        streams = oracle_encode(self.x, vs, ad)
        self.kind = np.arange(C) % 10
        rows, bits, made = [], np.zeros(C, dtype=np.uint64), []
        for c in range(C):
            k = int(self.kind[c])
            b, n, what = damage(rng, bytearray(streams[c][0]), streams[c][1], k, c)
            rows.append(bytes(b))
            bits[c] = n
            made.append("%s: %s" % (KINDS[k], what) if what else KINDS[k])
        # the smallest slab (a multiple of 4 bytes) that holds the longest stream; the longest of the lengthened streams
        # is then lengthened further, to the slab's very end: its last bit is the slab's last bit
        cap = 4 * ((max(max(len(r) for r in rows), 1) + 3) // 4)
        sevens = [c for c in range(C) if self.kind[c] == 7]
        if sevens:
            c7 = max(sevens, key=lambda c: int(bits[c]))
            bits[c7] = 8 * cap
            made[c7] += ", then to the end of the slab"
        self.cap = cap
        clean, garbage = slab_forms(rng, rows, bits, cap)
        self.slabs = {"clean": clean, "garbage": garbage}
        self.bits, self.made_from = bits, made
        for a in (self.x, clean, garbage, bits, self.kind):
            a.setflags(write=False)
        self._verdicts = {}

    def verdict(self, c):
        """(status, samples) of the oracle on channel c"""
        if c not in self._verdicts:
            self._verdicts[c] = oracle_verdict(self.slabs["clean"][c].tobytes(), int(self.bits[c]), self.vs, self.ad)
        return self._verdicts[c]

    def damaged(self):
        return int((self.kind != 0).sum())

    def counts(self):
        """(accepted damaged channels whose samples differ from the original, refused with -3, refused with -11, refused otherwise)"""
        wrong = m3 = m11 = other = 0
        for c in range(self.C):
            r, want = self.verdict(c)
            if r == orc.ERROR_INVALID_FORMAT:
                m3 += 1
            elif r == orc.ERROR_LIBRARY_CALL:
                m11 += 1
            elif r != 0:
                other += 1
            elif self.kind[c] != 0 and (len(want) != self.T or (want != self.x[:, c]).any()):
                wrong += 1
        return wrong, m3, m11, other

    def room(self):
        """rows a variable-count decoder is given: the largest count the oracle reports for an accepted channel plus 64, and
        never less than 2 * bits + 64 -- a decoded sample takes at least one seg bit, and on these walks a stream bit
        decodes to at most 1.07 seg bits, so no accepted channel can run out of room and few refused ones do"""
        most = max([len(self.verdict(c)[1]) for c in range(self.C) if self.verdict(c)[0] == 0] + [0])
        return max(most + 64, 2 * int(self.bits.max()) + 64)


@functools.lru_cache(maxsize=None)
def corpus(C, T, vs, ad):
    return Corpus(C, T, vs, ad)


def check(decode_var, corp, form="clean", channels=None, room=None):
    """decode_var(slabs, bits, room) -> (y [room][C], counts [C], err [C]).  Per channel: the status is the oracle's; where
    it is 0 the count and every sample are the oracle's; healthy channels give back the original samples.  The one excuse:
    a channel the oracle REFUSES may come back as ERROR_MEMORY -- the fused decoder parses while it decodes and can run
    out of rows before it reaches the place where the stage-wise chain fails -- for at most EXCUSED_CAP of the refused
    channels of the call.  Returns what happened, for the records: (result arrays, stats)."""
    room = corp.room() if room is None else room
    y, counts, err = decode_var(corp.slabs[form], corp.bits, room)
    sel = range(corp.C) if channels is None else channels
    refused = excused = 0
    for c in sel:
        r, want = corp.verdict(c)
        tag = (corp.vs, corp.ad, corp.T, form, int(c), corp.made_from[c])
        if r != 0:
            refused += 1
            if err[c] == orc.ERROR_MEMORY:
                excused += 1
                continue
            assert err[c] == r, (tag, int(err[c]), r)
            continue
        assert len(want) <= room, tag
        assert err[c] == 0, (tag, int(err[c]))
        assert int(counts[c]) == len(want), (tag, int(counts[c]), len(want))
        got = y[: len(want), c]
        got = got.view(np.uint64) if got.dtype.itemsize == 8 else got.view(np.uint32).astype(np.uint64)
        assert (got == want).all(), (tag, "first difference at row %d" % int(np.nonzero(got != want)[0][0]))
        if corp.kind[c] == 0:
            assert len(want) == corp.T and (want == corp.x[:, c]).all(), tag
    assert excused <= EXCUSED_CAP * refused, ("too many channels excused by the ERROR_MEMORY rule: enlarge room", excused, refused, room)
    return (y, counts, err), {"refused": refused, "excused": excused, "room": room}


def whole_codewords(seg, nbits, vs):
    """the whole exp-Golomb codewords at the head of a seg stream: up to the first that the stream's end cuts short (or that
    seg refuses for its zero prefix, seg.c:55-56)"""
    bits = np.unpackbits(np.frombuffer(seg, dtype=np.uint8))[:nbits]
    ones = np.flatnonzero(bits)
    cap = min(vs + 1, 64)
    pos = n = 0
    while True:
        i = int(np.searchsorted(ones, pos))
        if i == len(ones):
            return n  # zeros to the end: padding
        zeros = int(ones[i]) - pos
        if zeros >= cap or int(ones[i]) + 1 + zeros > nbits:
            return n
        n, pos = n + 1, int(ones[i]) + 1 + zeros


# Named cases: healthy oracle streams of 33-sample walks whose length was cut.  The reference refuses each with -3 at its
# 15th phantom bit.  A decoder that instead goes on decoding the zeros behind the stream until an EOF symbol turns up among
# them (the fused decoder did) produces `runaway` samples first.  Under the adaptive model that is more than a thousand
# from some 260 bits: it runs out of the `room` given here, which the samples of the stream proper fit, and reports
# ERROR_MEMORY -- the adaptive cases fail on such a decoder.  Under the static model a third of every interval is the EOF
# symbol's: four samples more at the most (the longest of 512 cuts tried), and they arrive together with the refusal, which
# wins; the static cases pin the status, they could not have found the bug.  (name, valuesize, adaptive, bits, room, runaway, hex)
NAMED_CUT_STREAMS = (
    ("cut, adaptive, 32", 32, 1, 264, 256, 1500, "fe3a7d4b54e979fd705d943b102bb2a517e92983b4c8c1b490d9c9480788613d18"),
    ("cut, adaptive, 64", 64, 1, 237, 256, 1500, "fe3a7d4dfd605fb9c61a27ce0c4cbd73cabc698f9d69b14e4a2bea3c9dbc"),
    ("cut, static, 32", 32, 0, 558, 34, 35,
     "ffffff6e72f0d3a7691516b09dff00e3396bdb9121019368cd37ec419e200c4cdce0f460a7c00aac1e2b3e464f6057bf56b0a11376e7e15388b69cbe26a3719574e6f4abb429"),
    ("cut, static, 64", 64, 0, 508, 33, 34,
     "ffffff6e72fd2f91a470f9bcd01139a2946bd37a1df9b13d6d6e3c39baf84ace17bda1056fa81d4fc75b755d27228e157d907f456ff3a256aa4e16ed5dc4b58d"),
)


def check_named_cut_streams(decode_var_for):
    """decode_var_for(vs, ad) -> decode_var.  Every named stream, alone and with ones behind its exact length: the status is
    -3, the oracle's, and nothing else -- no ERROR_MEMORY excuse here."""
    for name, vs, ad, nbits, room, _, hexed in NAMED_CUT_STREAMS:
        data = bytes.fromhex(hexed)
        assert len(data) == (nbits + 7) // 8 and oracle_verdict(data, nbits, vs, ad)[0] == orc.ERROR_INVALID_FORMAT, name
        cap = 4 * ((len(data) + 3) // 4) + 8
        slabs = np.zeros((2, cap), dtype=np.uint8)
        slabs[1] = 0xFF
        for c in range(2):
            slabs[c, : len(data)] = np.frombuffer(data, dtype=np.uint8)
        if nbits % 8:
            slabs[1, nbits // 8] |= 0xFF >> (nbits % 8)
        y, counts, err = decode_var_for(vs, ad)(slabs, np.full(2, nbits, dtype=np.uint64), room)
        assert err.tolist() == [orc.ERROR_INVALID_FORMAT] * 2, (name, err.tolist(), counts.tolist(), room)


def stump_stream(col, vs, ad, stump="00011"):
    """the samples of col as a seg stream, then a codeword cut short inside its residual, coded by the oracle's bac: bac
    finds its EOF symbol, seg its short read (ERROR_LIBRARY_CALL) -- the ending that a damaged adaptive stream rarely
    reaches, because bac has usually refused it before"""
    d, nb = pack_be(col, vs)
    for name in ("diff", "seg"):
        r, d, nb = orc.stage(name, True, d, nb, valuesize=vs)
        assert r == 0
    seg = np.concatenate([np.unpackbits(np.frombuffer(d, dtype=np.uint8))[:nb], np.array([int(b) for b in stump], dtype=np.uint8)])
    r, b, nb = orc.stage("bac", True, np.packbits(seg).tobytes(), len(seg), adaptive=ad)
    assert r == 0
    return b[: (nb + 7) // 8], nb


def slabs_of(streams, extra=0):
    cap = 4 * ((max(len(b) for b, _ in streams) + 3) // 4) + extra
    slabs = np.zeros((len(streams), cap), dtype=np.uint8)
    for i, (b, _) in enumerate(streams):
        slabs[i, : len(b)] = np.frombuffer(b, dtype=np.uint8)
    return slabs, np.array([nb for _, nb in streams], dtype=np.uint64)


def check_named_stumps(decode_var_for, sizes):
    """66 walks of 1 .. 66 samples per value size and model, each followed by a stump (two kinds in turn): the oracle says
    -11 for every one of them, and so must the decoder -- next to each other in a full wave and a ragged one"""
    for vs in sizes:
        for ad in (1, 0):
            x = walks(np.random.default_rng([11, vs, ad]), 66, 66, vs)
            streams = [stump_stream(x[: c + 1, c], vs, ad, ("00011", "0000101")[c % 2]) for c in range(66)]
            slabs, bits = slabs_of(streams)
            for c in (0, 1, 32, 65):
                assert oracle_verdict(slabs[c].tobytes(), int(bits[c]), vs, ad)[0] == orc.ERROR_LIBRARY_CALL, (vs, ad, c)
            y, counts, err = decode_var_for(vs, ad)(slabs, bits, 128)
            assert (err == orc.ERROR_LIBRARY_CALL).all(), (vs, ad, err.tolist())


def same_where_defined(a, b):
    """two results (y, counts, err) of the same call: every status, and for the channels with status 0 the count and the
    samples below it.  (What a refused channel leaves in its column and its count is not defined: how much of the window
    the parser had taken when the refusal reached it depends on the waves' timing.  Nor are the rows at or beyond a
    channel's count: a wave writes zeros there up to its longest channel and nothing below.)"""
    (ya, ca, ea), (yb, cb, eb) = a, b
    ok = ea == 0
    if not ((ea == eb).all() and (ca[ok] == cb[ok]).all()):
        return False
    valid = (np.arange(ya.shape[0], dtype=np.uint64)[:, None] < ca[None, :].astype(np.uint64)) & ok[None, :]
    return bool((ya[valid] == yb[valid]).all())


def check_not_vacuous(C, vs, ad):
    """the (C, vs, ad) corpus, its lengths taken together, exercises all three ends a damaged stream can come to"""
    got, damaged = [0, 0, 0, 0], 0
    for T in lengths(C, vs):
        corp = corpus(C, T, vs, ad)
        got = [g + n for g, n in zip(got, corp.counts())]
        damaged += corp.damaged()
    assert got[3] == 0, got  # the chain refuses with -3 or -11 only
    want = ORACLE_COUNTS[(C, vs, ad)]
    for k in range(3):
        assert got[k] >= (3 * want[k] + 3) // 4, ((C, vs, ad), ("wrong samples", "refused -3", "refused -11")[k], got, want, damaged)
    return tuple(got[:3]), damaged
