"""Shared by tests/test_seg_ladder_host.py and tests/test_gpu_seg_ladder.py: a closed-form corpus of INPUT series that puts
every exp-Golomb codeword length a value size has at every bit position of the seg stream, the conditions that say it does
so -- computed from the series and the oracle's stage chain alone, never from anything a kernel reports -- and the checkers
that hold an encoder and a decoder to the oracle on it, channel by channel.

The stage is diff plus signed exp-Golomb (diff.c, seg.c): a difference d of magnitude m is the codeword of w = 2 m (d > 0)
or 2 m + 1 (d <= 0), p = floor(log2 w) zeros and then the p + 1 bits of w -- 2 p + 1 bits.  +-m share p for
2^(p-1) <= m <= 2^p - 1; the one difference with p = valuesize is -2^(valuesize-1), the largest negative one diff.c:17-18
lets through.

The building block is the LADDER: for p = 1 .. vs - 1 the two edge magnitudes of the length class, m = 2^(p-1) and
m = 2^p - 1, each as the pair of samples `m, 0` (the differences +m and -m), then, for 2 <= vs < 64, `2^(vs-1) - 1,
2^(vs-1), 0`, whose last difference is -2^(vs-1).  1 + pad zero samples in front (one-bit codewords) shift every later
codeword by pad bits and pad rows.  A SHORT ladder keeps the groups whose magnitudes are at most 32767 (p <= 15).

C = 390 channels at every value size; a channel's series depends on (SEED, vs, c) alone:
  wave 0, channels 0..63     short ladders, pad = c % 32, ascending for c % 64 < 32 and descending otherwise: at value size
                             32 every full batch of 8 rows is one the filling wave appends straight-line (`plain`)
  wave 1, channels 64..127   the same, but lane PLANT_DIFF carries a single difference of 32768 in batch 3 (vs >= 17) and
                             lane PLANT_TOP a single sample >= 2^31 in batch 5 (vs >= 32): the wave goes general and returns
  from channel 128 on        kind c % 8 (KINDS), pad = (c // 8) % 32:
    0 ascending   the full ladder
    1 descending  the full ladder, groups in reverse order
    2 random      prefix length uniform in 0 .. vs - 1, random residual and sign, reflected into [0, 2^vs)
    3 worst       0 and 2^(vs-1) - 1 - r (r cycling 0..4, fewer where vs is small) in turn: every codeword 2 vs - 1 bits
    4 refused     one difference of +2^(vs-1) or -2^(vs-1) - 1 -- at row 0 (x[0] = 2^(vs-1)), 1, 7, 8 or T - 1 in turn --
                  next to the full ladder; reached over legal differences only, so it is the one thing wrong.  At value
                  size 64, which has no range check, the wrapped difference +-2^63 instead: coded like 0, lossy
    5 control     a +-3 walk
    6 dirty       kind 0 with random bits above the value size in the container (int32 below 32, int64 for 33..63); at 32
                  and 64, where there are none, samples with the top bit set whose differences are small
    7 three parts control, the rows of the ladder that fall into the middle third, control
T = the longest series of the size (the full ladder at pad 31); shorter series repeat their last sample."""
import functools

import numpy as np

import hostile_common as hc
from oracle import orc

SIZES = (1, 2, 3, 8, 15, 16, 17, 31, 32, 33, 47, 63, 64)
CN = 128 + 256 + 6  # two plain waves, every kind at every pad, a ragged last wave
SEED = 2026
KINDS = ("ascending", "descending", "random", "worst", "refused", "control", "dirty", "three parts")
ROWS = 8  # rows per batch of the filling wave
PLANT_DIFF, PLANT_TOP = 64 + 5, 64 + 41  # the two lanes of wave 1 that leave the straight-line batch, and their batches
PLANT_DIFF_BATCH, PLANT_TOP_BATCH = 3, 5
SPOIL_ROWS = ("0", "1", "7", "8", "T-1")
U64 = (1 << 64) - 1


def kind_of(c):
    return c % 8 if c >= 128 else (0 if c % 64 < 32 else 1)


def pad_of(c):
    return (c // 8) % 32 if c >= 128 else c % 32


# ---- the series (lists of Python integers) -----------------------------------------------------------------------------------
def groups(vs, short=False):
    """the ladder's groups, ascending; every group starts from a sample of 0 and ends in one"""
    half = 1 << (vs - 1)
    g = []
    for p in range(1, vs):
        for m in sorted({1 << (p - 1), (1 << p) - 1}):
            if not short or m <= 32767:
                g.append([m, 0])
    if 2 <= vs < 64 and (not short or half <= 32767):
        g.append([half - 1, half, 0])
    return g


def ladder(vs, pad, descending=False, short=False):
    g = groups(vs, short)
    return [0] * (1 + pad) + [v for grp in (g[::-1] if descending else g) for v in grp]


def length(vs):
    return len(ladder(vs, 31))


def control(rng, vs, n):
    top = min(200, (1 << (vs - 1)) - 1)
    x, v = [], top // 2
    for step in rng.integers(-3, 4, n):
        v = min(max(v + int(step), 0), top)
        x.append(v)
    return x


def random_series(rng, vs, n):
    x, v = [], 0
    for _ in range(n):
        p = int(rng.integers(0, vs))
        m = 0 if p == 0 else (1 << (p - 1)) + (int(rng.integers(0, 1 << 62)) % (1 << (p - 1)))
        d = m if rng.integers(0, 2) else -m
        if not 0 <= v + d < (1 << vs):
            d = -d
        v += d
        x.append(v)
    return x


def worst(vs, n):
    if vs == 1:
        return [0] * n
    span = min(5, 1 << (vs - 2))
    return [0 if t % 2 == 0 else (1 << (vs - 1)) - 1 - (t // 2) % span for t in range(n)]


def climb_and_drop(vs):
    """from a sample of 0: steps of the largest positive difference up to a sample of at least 2^(vs-1) + 1, then the
    difference -2^(vs-1) - 1 -- the only one out of range"""
    half = 1 << (vs - 1)
    x = [half - 1]
    while x[-1] < half + 1:
        x.append(x[-1] + half - 1)
    return x + [x[-1] - half - 1]


def refused(vs, c, T):
    """-> (series, row of the spoiled difference, its sign)"""
    half = 1 << (vs - 1)
    n = (c // 8) % (2 * len(SPOIL_ROWS))
    row = (0, 1, 7, 8, T - 1)[n % len(SPOIL_ROWS)]
    # (a negative spoil needs a sample of 2^(vs-1) + 1 in front of it, which takes at least two legal steps from 0)
    up = vs == 1 or row < 7 or n >= len(SPOIL_ROWS)
    if vs == 64:
        bad = [half] if up else [half + 5, 5]  # 0 -> 2^63, or 2^63 + 5 -> 5: both wrap to the difference -2^63
    else:
        bad = [half] if up else climb_and_drop(vs)
    body = [v for grp in groups(vs) for v in grp]
    if row == T - 1:
        x = [0] * (T - len(body) - len(bad)) + body + bad
    else:
        x = [0] * (row + 1 - len(bad)) + bad + [0] + body
    return x, row, 1 if up else -1


def dirty_top(rng, vs, pad, T):
    """value sizes 32 and 64: up to 2^(vs-1) - 1 in one legal step, then a +-60 walk above 2^(vs-1)"""
    half = 1 << (vs - 1)
    x = [0] * (1 + pad) + [half - 1]
    v = half + 30000
    while len(x) < T:
        x.append(v)
        v += int(rng.integers(-60, 61))
    return x


def planted(vs, c):
    """wave 1's two lanes: zeros, the plant, the short ladder.  The difference of 32768 stands in the last row of its batch
    behind 31 one-bit codewords: its 33 bits meet a bit queue that holds 31, the most it ever does between two codewords."""
    body = [v for grp in groups(vs, short=True) for v in grp]
    if c == PLANT_DIFF and vs >= 17:
        return [0] * (ROWS * PLANT_DIFF_BATCH + 7) + [32768, 1, 0] + body  # +32768 (w = 2^16), then -32767 and -1: short again
    if c == PLANT_TOP and vs >= 32:
        top = 1 << 31
        return [0] * (ROWS * PLANT_TOP_BATCH + 2) + [top - 1, top + 3, top - 2, 0] + body
    return None


def series(vs, c, T):
    """channel c's samples at value size vs: T Python integers in [0, 2^vs)"""
    rng = np.random.default_rng([SEED, vs, c])
    k, pad = kind_of(c), pad_of(c)
    if c < 128:
        x = planted(vs, c) or ladder(vs, pad, descending=k == 1, short=True)
    elif k in (0, 1):
        x = ladder(vs, pad, descending=k == 1)
    elif k == 2:
        x = random_series(rng, vs, T)
    elif k == 3:
        x = worst(vs, T)
    elif k == 4:
        x = refused(vs, c, T)[0]
    elif k == 5:
        x = control(rng, vs, T)
    elif k == 6:
        x = dirty_top(rng, vs, pad, T) if vs in (32, 64) else ladder(vs, pad)
    else:
        a, b = T // 3, 2 * (T // 3)
        mid = ladder(vs, pad)
        mid = mid + [mid[-1]] * T
        while mid[a - 1] != 0:  # (enter where the ladder stands at 0: 2^(vs-1) is reachable from 2^(vs-1) - 1 only)
            a += 1
        mid = mid[a:b]
        x = control(rng, vs, a) + mid + control(rng, vs, T - b)
    assert 1 <= len(x) <= T, (vs, c, len(x), T)
    x = x + [x[-1]] * (T - len(x))
    assert all(0 <= v < (1 << vs) for v in x), (vs, c)
    return x


# ---- a plain restatement of diff and seg ---------------------------------------------------------------------------------------
def prefixes(col, vs):
    """the prefix length of every sample's codeword (2 p + 1 bits each), and whether diff.c:17-18 lets every difference
    through.  At value size 64 the difference wraps, and so does w: +-2^63 gives w = 1."""
    ps, ok, last = [], True, 0
    half = 1 << (vs - 1)
    for v in col:
        d = v - last
        if vs == 64:
            d = (d + (1 << 63)) % (1 << 64) - (1 << 63)
        elif not -half <= d <= half - 1:
            ok = False
        w = (2 * abs(d) + (0 if d > 0 else 1)) & U64
        ps.append(w.bit_length() - 1)
        last = v
    return ps, ok


# ---- the corpus ----------------------------------------------------------------------------------------------------------------
class Corpus:
    """One value size.  x uint64 [T][C]: the samples (the low vs bits); xin [T][C]: the containers a kernel reads (int32 up to
    32, int64 above; kind 6 with junk above the value size); kind, pad [C].  The oracle's results are made on first use and
    kept: seg_bits(), encoded(ad), decoder_input(ad).  Arrays are read-only."""

    def __init__(self, vs, C_=CN):
        self.vs, self.C, self.T = vs, C_, length(vs)
        cols = [series(vs, c, self.T) for c in range(C_)]
        self.cols = cols
        self.x = np.array(cols, dtype=np.uint64).T.copy()
        self.kind = np.array([kind_of(c) for c in range(C_)])
        self.pad = np.array([pad_of(c) for c in range(C_)])
        raw = self.x.copy()
        if vs not in (32, 64):
            width = 32 if vs < 32 else 64
            for c in range(128, C_):
                if self.kind[c] == 6:
                    junk = np.random.default_rng([SEED, vs, c, 6]).integers(0, 1 << min(width - vs, 62), self.T, dtype=np.uint64)
                    raw[:, c] |= junk << np.uint64(vs)
        self.xin = np.ascontiguousarray(raw.astype(np.uint32).view(np.int32) if vs <= 32 else raw.view(np.int64))
        self.cap = 4 * ((self.T * (2 * vs + 1) * 2 + 64) // 32 + 4)  # two stream bits per seg bit and the coder's tail
        for a in (self.x, self.xin, self.kind, self.pad):
            a.setflags(write=False)
        self._seg, self._enc, self._dec, self._cut, self._counts = None, {}, {}, {}, None

    def refused_channels(self):
        return [c for c in range(self.C) if c >= 128 and self.kind[c] == 4 and self.vs < 64]

    def accepted(self):
        bad = set(self.refused_channels())
        return [c for c in range(self.C) if c not in bad]

    def seg(self):
        """per channel (status, seg stream bytes, seg bits) of `encode diff` -> `encode seg`"""
        if self._seg is None:
            res = []
            for c in range(self.C):
                d, n = hc.pack_be(self.x[:, c], self.vs)
                r = 0
                for name in ("diff", "seg"):
                    r, d, n = orc.stage(name, True, d, n, valuesize=self.vs)
                    if r != 0:
                        break
                res.append((r, d, n) if r == 0 else (r, b"", 0))
            self._seg = res
        return self._seg

    def encoded(self, ad):
        """(out uint8 [C][cap] zero padded, bits uint64 [C], err int32 [C]) of the oracle's chain; a refused channel has its
        status and nothing else"""
        if ad not in self._enc:
            out = np.zeros((self.C, self.cap), dtype=np.uint8)
            bits = np.zeros(self.C, dtype=np.uint64)
            err = np.zeros(self.C, dtype=np.int32)
            for c, (r, d, n) in enumerate(self.seg()):
                err[c] = r
                if r == 0:
                    r, b, nb = orc.stage("bac", True, d, n, adaptive=ad)
                    assert r == 0 and (nb + 7) // 8 <= self.cap, (self.vs, ad, c, r, nb)
                    out[c, : (nb + 7) // 8] = np.frombuffer(b[: (nb + 7) // 8], dtype=np.uint8)
                    bits[c] = nb
            if self.vs == 32:  # the whole-chain entry of the restatement says the same
                o2, b2, e2 = orc.encode_batch_tc(self.xin, ad, cap=self.cap)
                assert (e2 == err).all()
                ok = err == 0
                assert (b2[ok] == bits[ok]).all() and (o2[ok] == out[ok]).all()
            for a in (out, bits, err):
                a.setflags(write=False)
            self._enc[ad] = (out, bits, err)
        return self._enc[ad]

    def decoder_input(self, ad):
        """What the decoders are given: the oracle's stream of every accepted channel and, for a refused one (it has no
        stream), the oracle's stream of the unspoiled ladder at the channel's pad.  -> (slabs uint8 [C][cap], bits uint64 [C],
        verdicts: per channel the oracle's (status, samples uint64) on exactly that stream)"""
        if ad not in self._dec:
            out, bits, err = self.encoded(ad)
            slabs, bits = out.copy(), bits.copy()
            for c in self.refused_channels():
                col = ladder(self.vs, int(self.pad[c]))
                col = np.array(col + [col[-1]] * (self.T - len(col)), dtype=np.uint64)
                (b, nb), = hc.oracle_encode(col[:, None], self.vs, ad)
                slabs[c, : len(b)] = np.frombuffer(b, dtype=np.uint8)
                bits[c] = nb
            verdicts = [hc.oracle_verdict(slabs[c].tobytes(), int(bits[c]), self.vs, ad) for c in range(self.C)]
            slabs.setflags(write=False)
            bits.setflags(write=False)
            self._dec[ad] = (slabs, bits, verdicts)
        return self._dec[ad]

    def counts(self):
        """a ragged batch: counts that end some ladders inside the row of their longest codeword's pair, one row before and
        one after it, and leave every fourth channel whole (0 and 1 are in it)"""
        if self._counts is None:
            n = np.full(self.C, self.T, dtype=np.uint64)
            for c in range(self.C):
                ps = prefixes(self.cols[c], self.vs)[0]
                at = int(np.argmax(ps))  # the row of the (first) longest codeword
                n[c] = (self.T, at, at + 1, max(at - 1, 0))[c % 4]
            n[2], n[3] = 0, 1
            n.setflags(write=False)
            self._counts = n
        return self._counts

    def encoded_counted(self, ad):
        """per channel (status, bytes, bits) of the oracle's chain on the channel's own first counts()[c] samples"""
        if ad not in self._cut:
            res = []
            for c, n in enumerate(self.counts()):
                d, nb = hc.pack_be(self.x[: int(n), c], self.vs)
                r = 0
                for name in ("diff", "seg", "bac"):
                    r, d, nb = orc.stage(name, True, d, nb, valuesize=self.vs, adaptive=ad)
                    if r != 0:
                        break
                res.append((0, d[: (nb + 7) // 8], nb) if r == 0 else (r, b"", 0))
            self._cut[ad] = res
        return self._cut[ad]

    def head(self, n):
        return Head(self, n)


class Head:
    """the first n channels of a corpus (a channel's series does not depend on the batch): what the emulator is given"""

    def __init__(self, corp, n):
        self.full, self.vs, self.C, self.T, self.cap = corp, corp.vs, n, corp.T, corp.cap
        self.x, self.xin, self.kind, self.pad = corp.x[:, :n], np.ascontiguousarray(corp.xin[:, :n]), corp.kind[:n], corp.pad[:n]

    def refused_channels(self):
        return [c for c in self.full.refused_channels() if c < self.C]

    def encoded(self, ad):
        return tuple(a[: self.C] for a in self.full.encoded(ad))

    def decoder_input(self, ad):
        slabs, bits, verdicts = self.full.decoder_input(ad)
        return slabs[: self.C], bits[: self.C], verdicts[: self.C]


@functools.lru_cache(maxsize=None)
def corpus(vs):
    return Corpus(vs)


def golden_channels():
    """the channels of tests/golden/seg_ladder.npz: one of every kind at pad 19 -- the refused one with the positive difference
    at row T - 1 -- and channel 180, refused for the negative difference at row 7"""
    return list(range(152, 160)) + [180]


def segment_cuts(T):
    """launch boundaries at rows 1, 7, 8, 9 and twice in the middle of the ladder"""
    return [0, 1, 7, 8, 9, T // 2, T // 2 + 3, T]


# ---- the conditions ----------------------------------------------------------------------------------------------------------
def conditions(corp):
    """What the corpus exercises, from the series, the restatement above and the oracle's stages alone.  Asserts the
    conditions and returns the measured figures."""
    vs, T = corp.vs, corp.T
    seen = {"value size": vs, "C, T": (corp.C, T)}
    accepted = corp.accepted()
    want_refused = corp.refused_channels()
    pairs, lengths_seen, total = set(), set(), 0
    for c in range(corp.C):
        ps, ok = prefixes(corp.cols[c], vs)
        r, _, nseg = corp.seg()[c]
        if c in want_refused:
            assert not ok and r == orc.ERROR_INVALID_VALUE, (vs, c, ok, r)
            # exactly one difference is out of range, the spoiled one, at the row the kind says
            col, row, sign = refused(vs, c, T)
            half = 1 << (vs - 1)
            d = [v - u for u, v in zip([0] + corp.cols[c][:-1], corp.cols[c])]
            out_of_range = [t for t in range(T) if not -half <= d[t] <= half - 1]
            assert out_of_range == [row] and d[row] == (half if sign > 0 else -half - 1), (vs, c, out_of_range, row)
            continue
        assert ok and r == 0, (vs, c, KINDS[corp.kind[c]], ok, r)
        assert sum(2 * p + 1 for p in ps) == nseg, ("the restatement's codeword lengths are not the oracle's", vs, c, sum(2 * p + 1 for p in ps), nseg)
        pos = 0
        for p in ps:
            pairs.add((p, pos % 32))
            pos += 2 * p + 1
        lengths_seen |= set(ps)
        total += nseg
    want_lengths = {0} if vs == 1 else set(range(vs + 1 if vs < 64 else 64))
    assert lengths_seen == want_lengths, (vs, sorted(lengths_seen))
    missing = [(p, ph) for p in sorted(want_lengths) for ph in range(32) if (p, ph) not in pairs]
    assert not missing, (vs, missing[:16])
    seen["prefix lengths among accepted channels"] = "%d..%d" % (min(lengths_seen), max(lengths_seen))
    seen["(prefix, bit position mod 32) pairs present, missing"] = (len(pairs), len(missing))
    seen["accepted, refused channels"] = (len(accepted), len(want_refused))
    seen["seg bits of the accepted channels"] = total
    if vs == 64:  # the wrapped difference: accepted, and the chain does not give the samples back
        wrapped = [c for c in range(128, corp.C) if corp.kind[c] == 4]
        for c in wrapped:
            assert (1 << 63) in [abs(v - u) for u, v in zip([0] + corp.cols[c][:-1], corp.cols[c])], c
        seen["channels with a difference of +-2^63"] = len(wrapped)
    if vs == 32:
        seen.update(plain_waves(corp))
    if 2 <= vs < 64:
        rows = sorted({refused(vs, c, T)[1] for c in want_refused})
        signs = sorted({refused(vs, c, T)[2] for c in want_refused})
        assert rows == [0, 1, 7, 8, T - 1] and signs == [-1, 1], (vs, rows, signs)
        seen["rows of the spoiled differences"] = rows
    # the decode chain: every accepted channel comes back as its masked samples (value size 64: but for the wrapped ones)
    for ad in (1, 0):
        _, _, verdicts = corp.decoder_input(ad)
        lossy = 0
        for c in accepted:
            r, back = verdicts[c]
            assert r == 0 and len(back) == T, (vs, ad, c, r)
            same = bool((back == corp.x[:, c]).all())
            assert same or (vs == 64 and corp.kind[c] == 4 and c >= 128), (vs, ad, c)
            lossy += not same
        for c in want_refused:  # (the unspoiled ladder's stream)
            assert verdicts[c][0] == 0 and len(verdicts[c][1]) == T
        if vs == 64:
            seen["channels the chain decodes lossily (%s)" % ("adaptive" if ad else "static")] = lossy
            assert lossy == len([c for c in range(128, corp.C) if corp.kind[c] == 4])
    return seen


def plain_waves(corp):
    """value size 32, waves 0 and 1: a batch of 8 rows is `plain` for a lane when every sample of it, and the one before
    it, is below 2^31 and every w below 2^16 (encode_filling_wave); the wave appends straight-line only when all 64 are"""
    T = corp.T
    full = T // ROWS
    at_row = [set() for _ in range(ROWS)]
    not_plain = {}
    for c in range(128):
        col = corp.cols[c]
        ps = prefixes(col, 32)[0]
        last = 0
        for b in range(full):
            rows = range(ROWS * b, ROWS * b + ROWS)
            ok = last < (1 << 31) and all(col[t] < (1 << 31) and ps[t] <= 15 for t in rows)
            last = col[rows[-1]]
            if not ok:
                not_plain.setdefault((c // 64, b), []).append(c)
    assert not_plain == {(1, PLANT_DIFF_BATCH): [PLANT_DIFF], (1, PLANT_TOP_BATCH): [PLANT_TOP]}, not_plain
    assert sum(1 for v in corp.cols[PLANT_DIFF] if v >= 32768) == 1 and sum(1 for v in corp.cols[PLANT_TOP] if v >= (1 << 31)) == 1
    for c in range(128):
        ps = prefixes(corp.cols[c], 32)[0]
        for t in range(ROWS * full):
            if (c // 64, t // ROWS) not in not_plain:
                at_row[t % ROWS].add(ps[t])
    assert all(s == set(range(16)) for s in at_row), [sorted(s) for s in at_row]
    return {"full batches per wave, all plain but": (full, sorted(not_plain)), "prefix lengths at every row mod 8 of the plain batches": "0..15"}


# ---- the checkers ------------------------------------------------------------------------------------------------------------
def check_encode(corp, ad, out, bits, err, what="", channels=None):
    """Status per channel; for the accepted ones the bit length and every byte of the slab -- the stream, and zeros behind
    it.  A refused channel is held to its status alone (what it leaves in its slab is not defined); its neighbours are held
    in full.  channels: the results are those of these channels."""
    want_out, want_bits, want_err = corp.encoded(ad)
    if channels is not None:
        want_out, want_bits, want_err = want_out[channels], want_bits[channels], want_err[channels]
    out, bits, err = np.asarray(out), np.asarray(bits).astype(np.uint64), np.asarray(err)
    tag = (what, corp.vs, ad)
    assert len(err) == len(want_err) and out.shape[0] == len(want_err), tag
    assert (err == want_err).all(), (tag, "status", np.flatnonzero(err != want_err)[:8].tolist(), err[err != want_err][:8].tolist())
    ok = want_err == 0
    assert (bits[ok] == want_bits[ok]).all(), (tag, "bit length", np.flatnonzero(ok & (bits != want_bits))[:8].tolist())
    n = min(out.shape[1], want_out.shape[1])
    bad = np.flatnonzero(ok & (out[:, :n] != want_out[:, :n]).any(axis=1))
    assert len(bad) == 0, (tag, "bytes", [(int(c), int(np.flatnonzero(out[c, :n] != want_out[c, :n])[0])) for c in bad[:8]])
    assert not out[ok][:, n:].any() and not want_out[ok][:, n:].any(), tag


def check_encode_short(corp, ad, cap, out, bits, err, what=""):
    """The short-slab contract (encoder_regimes_common.check_short): ERROR_MEMORY where the oracle's stream does not fit cap
    bytes, the oracle's bit length either way, and the oracle's bytes in front of the cap.  Refused channels: status alone."""
    want_out, want_bits, want_err = corp.encoded(ad)
    out, bits, err = np.asarray(out), np.asarray(bits).astype(np.uint64), np.asarray(err)
    tag = (what, corp.vs, ad, cap)
    assert out.shape == (corp.C, cap), tag
    want = np.where(want_err != 0, want_err, np.where((want_bits + np.uint64(7)) // np.uint64(8) > cap, orc.ERROR_MEMORY, 0))
    assert (err == want).all(), (tag, "status", np.flatnonzero(err != want)[:8].tolist(), err[err != want][:8].tolist())
    ok = want_err == 0
    assert (bits[ok] == want_bits[ok]).all(), (tag, "bit length", np.flatnonzero(ok & (bits != want_bits))[:8].tolist())
    bad = np.flatnonzero(ok & (out != want_out[:, :cap]).any(axis=1))
    assert len(bad) == 0, (tag, "bytes in front of the cap", [(int(c), KINDS[corp.kind[c]], int(np.flatnonzero(out[c] != want_out[c, :cap])[0])) for c in bad[:8]])


def short_cap(corp, part=2):
    """The worst case (corp.cap: two stream bits per seg bit of the longest codewords) divided by `part`, rounded to 4.
    Asserted from the oracle: at least 3 channels fit, and at least 3 worst-case channels do not -- at half the worst case
    under the static model only (the adaptive model codes a worst-case channel in a little less than its seg bits, just
    below the half: that run holds whole streams to a tight slab), at a quarter under both.  -> (cap, models that overflow)"""
    cap = (corp.cap // part + 3) & ~3
    overflowing = []
    for ad in (1, 0):
        _, bits, err = corp.encoded(ad)
        nbytes = (bits + np.uint64(7)) // np.uint64(8)
        over = [c for c in range(128, corp.C) if corp.kind[c] == 3 and nbytes[c] > cap]
        fit = [c for c in range(corp.C) if err[c] == 0 and nbytes[c] <= cap]
        assert len(fit) >= 3 and (len(over) >= 3 or (ad == 1 and part == 2)), (corp.vs, ad, cap, len(over), len(fit))
        if len(over) >= 3:
            overflowing.append(ad)
    assert 0 in overflowing
    return cap, overflowing


def check_encode_counted(corp, ad, out, bits, err, what=""):
    """a ragged batch against the oracle on each channel's own prefix: status; where it is 0 the bit length, the stream and
    zeros behind it"""
    out, bits, err = np.asarray(out), np.asarray(bits), np.asarray(err)
    for c, (r, data, n) in enumerate(corp.encoded_counted(ad)):
        tag = (what, corp.vs, ad, c, KINDS[corp.kind[c]], int(corp.counts()[c]))
        assert int(err[c]) == r, (tag, int(err[c]), r)
        if r == 0:
            assert int(bits[c]) == n, (tag, int(bits[c]), n)
            assert out[c, : len(data)].tobytes() == data and not out[c, len(data):].any(), tag


def check_decode(corp, ad, y, counts, err, what=""):
    """A decoder on decoder_input(ad): status, count and every sample of every channel are the oracle's verdict on the very
    stream it was given.  counts None: a fixed-length decoder that was asked for T samples, which every verdict has."""
    _, _, verdicts = corp.decoder_input(ad)
    y, err = np.asarray(y), np.asarray(err)
    assert y.shape[1] == corp.C and len(err) == corp.C
    for c in range(corp.C):
        r, want = verdicts[c]
        tag = (what, corp.vs, ad, c, KINDS[corp.kind[c]], int(corp.pad[c]))
        assert int(err[c]) == r, (tag, int(err[c]), r)
        assert r == 0 and len(want) == corp.T, tag  # (every stream of this corpus is a valid one)
        if counts is not None:
            assert int(counts[c]) == len(want), (tag, int(counts[c]), len(want))
        got = y[: len(want), c]
        got = got.view(np.uint64) if got.dtype.itemsize == 8 else got.view(np.uint32).astype(np.uint64)
        assert (got == want).all(), (tag, "first difference at row %d" % int(np.nonzero(got != want)[0][0]))
