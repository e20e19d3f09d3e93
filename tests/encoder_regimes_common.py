"""Shared by tests/test_encoder_regimes_host.py and tests/test_gpu_encoder_regimes.py: a seeded corpus of INPUT series that
steers the DEGA encoder onto the paths healthy data never takes, and the conditions -- computed from the oracle's stream
and a replay of the reference's coder alone, never from anything a kernel reports -- that say the corpus really does so.

Meter-like walks keep the coder on its eight-symbol word path (CLS_FAST8, dega_lane.hpp) with a halving word now and then.
Channel c of this corpus is of kind c % 8 (KINDS), so every wave of 64 lanes holds every kind next to healthy lanes; a
channel's series depends on (seed, c) alone, so a smaller batch is the head of a larger one:
  0 healthy       a +-60 walk, the control
  1 still         x[0] = 0 and zeros: the less probable symbol's count stays 1 and cum[0] + 31 > 128 * f2 within four
                  words -- bit at a time (CLS_BITS); every other channel sits still, jumps once, and sits still again
  2 sparse        steps of +-1, mostly one every 8..48 samples: the model lives between 11 * f2 and 128 * f2 (CLS_FAST4);
                  a still start and a dense stretch take it across both limits, in both directions
  3 balanced      differences from {0, +-1, +-2}, chosen so that the two symbols' counts tie again and again: exchanges
                  of the more and the less probable symbol (bac.c:68-77), the general word path (CLS_GENERAL)
  4 pending up    steered (oracle/regimes.c, rg_steer): every seg bit is the one whose sub-interval still straddles the
                  half point, so no bit gets out and the owed ("pending") bits grow -- to a wanted run that cycles through
                  WANTED --, then the run is ended upward: a carry through that many ones, in the writer's terms
                  (BacWriter::ripple_carry_from: "once in 2^32 hand-overs of random data")
  5 pending down  the same, ended downward: the run of ones stands
  6 jumps         2^31 - 1, 0, small, ...: codewords of 63..65 bits next to one-bit ones inside one batch of 8 rows, and so
                  many coded bits that the counts halve (bac.c:57-67) before the channel ends
  7 switch        kind 1 for the first third, kind 4 for the second, kind 0 for the last: the coder's look-ahead (`safe`)
                  runs out in the middle of a stream
The steered kinds try up to STEER_TRIES parameter sets (seeded) and keep the first whose stream has a run of at least
LONG_RUN owed bits ended the wanted way: that is how "pick the seeds" is done, by rule.

Under the static model (adaptive = 0) the same series are coded and compared, but no condition is attached: a third of
every interval is the EOF symbol's there, which breaks the runs -- greedy steering against the static model reaches 20..33
owed bits, and the static coder has one word path."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

from oracle import orc

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE_DIR = os.path.join(os.path.dirname(HERE), "oracle")
REGIMES_SO = os.path.join(ORACLE_DIR, "libregimes.so")

KINDS = ("healthy", "still", "sparse", "balanced", "pending up", "pending down", "jumps", "switch")
WANTED = (36, 48, 70, 100, 170, 250)
CAPS = (64, 128, 200, 256, 300, 400)  # the short slabs, bytes
SEED = 2025
STEER_TRIES = 16
# Owed bits from which on a run is "long".  The 31 + 32 bits that put an aligned word inside the run, plus what the writer's
# collector F holds (at most 62), plus the coder's finished bits (at most 30) make 155: beyond that the held-back word or
# one already handed on is all ones when the carry arrives, whatever the phase.
LONG_RUN = 160
PAST_A_WORD = 33  # owed bits from which on a run covers at least one bit of a second word


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(REGIMES_SO):
            subprocess.run(["make", "-s", "-C", ORACLE_DIR, "oracle"], check=True)
        L = C.CDLL(REGIMES_SO)
        L.rg_seg_bits.restype = C.c_int64
        L.rg_seg_bits.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rg_replay.restype = C.c_int64
        L.rg_replay.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
        L.rg_steer.restype = C.c_int
        L.rg_steer.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint, C.c_void_p, C.c_size_t, C.c_int, C.c_int64, C.c_int64, C.c_void_p]
        _lib = L
    return _lib


# ---- the replay ------------------------------------------------------------------------------------------------------------
class Trace:
    """The reference's coder replayed on one series.  nbits, stream (bytes, zero padded); per emit event -- a bit that gets
    out and settles the bits owed until then as its inverse -- ev_pos (the stream position of that bit), ev_bit, ev_pend
    (the owed bits it settles), ev_row (the row whose codeword was being coded; T for the EOF symbol), ev_from (the row at
    which the previous event happened: the run was built from there on); per word of 32 seg bits word_tot (cum[0]) and
    word_f2 (the count of the less probable symbol) at its start; swap_sym / halve_sym: the seg bits at whose model update
    the two symbols exchanged their indices / the counts were halved, halve_row the rows of the latter; seg_bits."""

    def pending_of_every_bit(self):
        """(pending, row) for every bit of the stream: those of the event the bit belongs to"""
        reps = self.ev_pend.astype(np.int64) + 1
        return np.repeat(self.ev_pend, reps), np.repeat(self.ev_row, reps)

    def carries(self, least, beyond_byte=0):
        """events that end a run of >= least owed bits in a carry, the bit that takes the carry at or beyond a byte offset"""
        return np.flatnonzero((self.ev_bit == 1) & (self.ev_pend >= least) & (self.ev_pos >= 8 * beyond_byte))

    def stands(self, least):
        """events that end a run of >= least owed bits without a carry"""
        return np.flatnonzero((self.ev_bit == 0) & (self.ev_pend >= least))


def seg_bits(col):
    """the seg stream of a series (int32, the 32 bits read as unsigned) -> (bits uint8 one per entry, row_end uint32 [T])"""
    col = np.ascontiguousarray(col, dtype=np.int32)
    bits = np.zeros(65 * len(col) + 1, dtype=np.uint8)
    row_end = np.zeros(len(col), dtype=np.uint32)
    n = lib().rg_seg_bits(col.ctypes.data, len(col), bits.ctypes.data, len(bits), row_end.ctypes.data)
    assert n >= 0, ("a difference of the series does not fit 32 bits", n)
    return bits[:n], row_end


def replay(col, adaptive):
    col = np.ascontiguousarray(col, dtype=np.int32)
    seg, row_end = seg_bits(col)
    n = len(seg)
    cap = 16 * n + 64  # (a symbol costs at most 14 bits, log2 of MAX_FREQUENCY)
    out = np.zeros(cap, dtype=np.uint8)
    ev_pos, ev_pend, ev_sym = (np.zeros(cap, dtype=np.uint32) for _ in range(3))
    ev_bit = np.zeros(cap, dtype=np.uint8)
    words = (n + 31) // 32
    word_tot, word_f2 = np.zeros(words, dtype=np.uint32), np.zeros(words, dtype=np.uint32)
    swap_sym, halve_sym = np.zeros(n + 1, dtype=np.uint32), np.zeros(64, dtype=np.uint32)
    counts = np.zeros(4, dtype=np.uint64)
    nbits = lib().rg_replay(seg.ctypes.data, n, adaptive, out.ctypes.data, cap, ev_pos.ctypes.data, ev_pend.ctypes.data, ev_sym.ctypes.data, ev_bit.ctypes.data,
                            cap, word_tot.ctypes.data, word_f2.ctypes.data, swap_sym.ctypes.data, len(swap_sym), halve_sym.ctypes.data, len(halve_sym),
                            counts.ctypes.data)
    assert nbits >= 0 and counts[2] <= len(halve_sym)
    t = Trace()
    nev = int(counts[0])
    t.nbits, t.seg_bits = int(nbits), n
    t.stream = np.packbits(out[:nbits]).tobytes()
    t.ev_pos, t.ev_pend, t.ev_bit = ev_pos[:nev].copy(), ev_pend[:nev].copy(), ev_bit[:nev].copy()
    t.ev_row = np.searchsorted(row_end, ev_sym[:nev], side="right").astype(np.uint32)  # (the EOF symbol: row T)
    t.ev_from = np.concatenate([[0], t.ev_row[:-1]]).astype(np.uint32)
    t.word_tot, t.word_f2 = word_tot, word_f2
    t.swap_sym, t.halve_sym = swap_sym[: int(counts[1])].copy(), halve_sym[: int(counts[2])].copy()
    t.halve_row = np.searchsorted(row_end, t.halve_sym, side="right").astype(np.uint32)
    assert int(t.ev_pend.sum()) + nev == t.nbits
    return t


# ---- the series ------------------------------------------------------------------------------------------------------------
def walk(rng, n, start):
    return start + np.cumsum(rng.integers(-60, 61, n))


def still(rng, T, variant):
    x = np.zeros(T, dtype=np.int64)
    if variant:
        x[int(rng.integers(2 * T // 3, 5 * T // 6)):] = int(rng.integers(1000, 1 << 20))  # (late: the jump's codeword brings f2 to a dozen)
    return x


def sparse(rng, T):
    """Steps of +-1, their spacing led by the model's two counts (cum[0] = 3 + bits coded, f2 = 1 + zeros coded: a zero
    difference is the one-bit codeword `1`, a step is `010` or `011`): still from x[0] = 0 until cum[0] has been beyond
    128 * f2 for two words; then a step every 8..48 samples for 120 rows; then a step every other sample until cum[0] is
    below 11 * f2 for a word to come; then every 8..48 samples again, which takes it back over that limit."""
    x, v = [], 0
    tot, f2 = 4, 1  # after x[0] = 0
    mode, held, wait, since = "still", 0, 0, 0
    for t in range(1, T):
        d = 0
        if mode == "still":
            held += tot + 31 > 128 * f2
            if held >= 70:
                mode = "sparse"
        elif mode == "dense":
            if t % 2:
                d = 1
            if tot + 63 <= 11 * f2:
                mode, since = "sparse", -T
        if mode == "sparse":
            since += 1
            if wait == 0:
                d, wait = 1, int(rng.integers(8, 49))
            wait -= 1
            if since == 120:
                mode = "dense"
        if d:
            d = 1 if (v == 0 or rng.integers(0, 2)) else -1
        v += d
        x.append(v)
        tot += 3 if d else 1
        f2 += 2 if d > 0 else 1 if d < 0 else 0
    return np.array([0] + x, dtype=np.int64)


BALANCED_CODES = {0: "1", 1: "010", -1: "011", 2: "00100", -2: "00101"}  # seg.c:11-28


def balanced(rng, T):
    """Replays the model's two counts bit by bit (bac.c:68-80 without the halving, which 600 such samples never reach): of
    the five differences the one after whose codeword the counts are nearest a tie, the series kept inside [100, 5000]; one
    sample in four is drawn at random, so that the counts drift apart and have to come back."""
    f = [1, 1]
    x = [1000]
    for ch in format(2000, "b").rjust(21, "0"):  # the codeword of x[0]: 1000 - 0 -> w = 2000, ten zeros in front
        f[int(ch)] += 1
    for _ in range(T - 1):
        options = [d for d in BALANCED_CODES if 100 <= x[-1] + d <= 5000]
        if rng.integers(0, 4) == 0:
            d = options[int(rng.integers(0, len(options)))]
        else:
            def apart(d):
                code = BALANCED_CODES[d]
                return abs((f[0] + code.count("0")) - (f[1] + code.count("1")))
            best = min(apart(d) for d in options)
            ties = [d for d in options if apart(d) == best]
            d = ties[int(rng.integers(0, len(ties)))]
        for ch in BALANCED_CODES[d]:
            f[int(ch)] += 1
        x.append(x[-1] + d)
    return np.array(x, dtype=np.int64)


def jumps(rng, T):
    """2^31 - 1, 0 and a few small samples, over and over; one group in four goes over 2^31 (as a 32-bit sample) and down
    from there, the one difference of 65 bits (-2^31)"""
    x = []
    while len(x) < T:
        x.append((1 << 31) - 1)
        if rng.integers(0, 4) == 0:
            x.append(1 << 31)
        x.append(0)
        x.extend(int(v) for v in rng.integers(0, 4, int(rng.integers(0, 3))))
    return np.array(x[:T], dtype=np.int64)


def steer(head, n, maxprefix, wanted, up):
    head = np.ascontiguousarray(head, dtype=np.int32)
    wanted = np.ascontiguousarray(wanted, dtype=np.uint32)
    out = np.zeros(len(head) + n, dtype=np.int32)
    r = lib().rg_steer(head.ctypes.data, len(head), n, maxprefix, wanted.ctypes.data, len(wanted), up, 1 << 16, 1 << 23, out.ctypes.data)
    assert r == 0
    return out.astype(np.int64)


def steered(c, T, up):
    """x[0] = 2^20, up to five samples of a walk (they vary the state the steering starts from), the rest steered"""
    for attempt in range(STEER_TRIES):
        rng = np.random.default_rng([SEED, c, attempt])
        head = np.concatenate([[1 << 20], walk(rng, int(rng.integers(0, 6)), 1 << 20)])
        turn = int(rng.integers(0, len(WANTED)))
        x = steer(head, T - len(head), int(rng.integers(8, 17)), WANTED[turn:] + WANTED[:turn], up)
        t = replay(x.astype(np.int32), 1)
        if len(t.carries(LONG_RUN) if up else t.stands(LONG_RUN)) > 0:
            return x
    raise AssertionError("no long run in %d tries, channel %d" % (STEER_TRIES, c))


def switch(rng, T):
    a, b = T // 3, 2 * (T // 3)
    head = np.concatenate([np.zeros(a, dtype=np.int64), [1 << 20]])
    turn = int(rng.integers(0, len(WANTED)))
    x = steer(head, b - len(head), int(rng.integers(8, 17)), WANTED[turn:] + WANTED[:turn], 1)
    return np.concatenate([x, walk(rng, T - b, x[-1])])


def series(c, T):
    """channel c's samples, int64 (all within [0, 2^32): kind 6 alone goes beyond 2^24)"""
    rng = np.random.default_rng([SEED, c])
    k = c % 8
    if k == 0:
        return walk(rng, T, 30000)
    if k == 1:
        return still(rng, T, (c // 8) % 2)
    if k == 2:
        return sparse(rng, T)
    if k == 3:
        return balanced(rng, T)
    if k in (4, 5):
        return steered(c, T, 1 if k == 4 else 0)
    if k == 6:
        return jumps(rng, T)
    return switch(rng, T)


def longest_run(stream, nbits, bit):
    b = np.unpackbits(np.frombuffer(stream, dtype=np.uint8))[:nbits]
    edges = np.flatnonzero(np.diff(np.concatenate([[1 - bit], b, [1 - bit]]) == bit))
    return int((edges[1::2] - edges[::2]).max()) if len(edges) else 0


class Corpus:
    """x int32 [T][C] (read-only; kind 6 holds samples of 2^31 and more, negative as int32), kind [C]; the oracle's streams
    under either model (oracle(ad) -> out uint8 [C][cap], bits uint64 [C], all statuses 0, cap the worst case rounded up to
    a multiple of 4) and the replay's traces (trace(c, ad)), made on first use and kept.  A trace is handed out only after
    its stream has been found to be the oracle's, bit for bit."""

    def __init__(self, C_, T):
        self.C, self.T = C_, T
        x = np.stack([series(c, T) for c in range(C_)], axis=1)
        assert x.shape == (T, C_) and x.min() >= 0 and x.max() < (1 << 32)
        self.kind = np.arange(C_) % 8
        self.x = x.astype(np.uint32).view(np.int32)
        self.cap = (orc.lib().orc_dega_worst_case_bytes(T) + 3) & ~3
        self.x.setflags(write=False)
        self.kind.setflags(write=False)
        self._oracle, self._traces = {}, {}

    def oracle(self, ad):
        if ad not in self._oracle:
            out, bits, err = orc.encode_batch_tc(self.x, ad, cap=self.cap)
            assert (err == 0).all()
            for a in (out, bits, err):
                a.setflags(write=False)
            self._oracle[ad] = (out, bits, err)
        return self._oracle[ad]

    def trace(self, c, ad=1):
        if (c, ad) not in self._traces:
            t = replay(self.x[:, c], ad)
            out, bits, _ = self.oracle(ad)
            assert t.nbits == int(bits[c]) and t.stream == out[c, : (t.nbits + 7) // 8].tobytes(), ("the replay's stream is not the oracle's", c, ad)
            self._traces[(c, ad)] = t
        return self._traces[(c, ad)]

    def of_kind(self, *kinds):
        return [c for c in range(self.C) if self.kind[c] in kinds]

    def waves(self):
        return [range(w, min(w + 64, self.C)) for w in range(0, self.C, 64)]

    def cuts(self, runs=2):
        """Launch boundaries taken from the replay (adaptive model): for the `runs` longest runs ended in a carry and the
        `runs` longest ended without one (one per channel, each of at least 100 owed bits) the row r at which the run is
        settled, the row before it -- so [r - 1, r) is a launch of one row -- and a single row m in the middle of the
        run.  -> a sorted list that starts with 0 and ends with T"""
        found = {0: [], 1: []}
        for c in self.of_kind(4, 5, 7):
            t = self.trace(c)
            for bit in (0, 1):
                ev = np.flatnonzero((t.ev_bit == bit) & (t.ev_pend >= 100) & (t.ev_row < self.T) & (t.ev_row > t.ev_from + 3))
                if len(ev):
                    e = ev[np.argmax(t.ev_pend[ev])]
                    found[bit].append((int(t.ev_pend[e]), c, int(t.ev_from[e]), int(t.ev_row[e])))
        cuts = {0, self.T}
        for bit in (0, 1):
            assert len(found[bit]) >= runs
            for _, c, a, r in sorted(found[bit], reverse=True)[:runs]:
                m = (a + r) // 2
                cuts |= {r - 1, r, m, m + 1}
        return sorted(cuts)

    def single_rows(self):
        """[a, a + 1, ..., r + 1] across the longest run of the corpus that ended in a carry, then T"""
        best = None
        for c in self.of_kind(4, 7):
            t = self.trace(c)
            ev = t.carries(LONG_RUN)
            ev = ev[t.ev_row[ev] + 1 < self.T]
            for e in ev:
                if best is None or t.ev_pend[e] > best[0]:
                    best = (int(t.ev_pend[e]), int(t.ev_from[e]), int(t.ev_row[e]))
        assert best is not None
        return [0] + list(range(max(1, best[1]), best[2] + 2)) + [self.T]

    def runs_across(self, every, least=100):
        """the channels with a run of >= least owed bits that is being built when row k * every begins, for some k: a launch
        boundary at every `every` rows falls inside it"""
        found = []
        for c in self.of_kind(4, 5, 7):
            t = self.trace(c)
            a, r = t.ev_from.astype(np.int64), t.ev_row.astype(np.int64)
            if ((t.ev_pend >= least) & (r // every > a // every)).any():
                found.append(c)
        return found

    def carries_beyond(self, cap, least=PAST_A_WORD):
        """the channels with a carry after >= least owed bits whose landing bit lies at or beyond byte `cap`"""
        return [c for c in self.of_kind(4, 5, 7) if len(self.trace(c).carries(least, beyond_byte=cap))]


@functools.lru_cache(maxsize=None)
def corpus(C_, T):
    return Corpus(C_, T)


# ---- the conditions ----------------------------------------------------------------------------------------------------------
def conditions(corp):
    """What the corpus exercises, from the oracle's streams and the replay alone (adaptive model).  Asserts the conditions
    and returns the measured figures."""
    seen = {}
    per = [len(corp.trace(c).carries(PAST_A_WORD)) for c in corp.of_kind(4, 5, 7)]
    seen["carries after >= 33 owed bits, per channel of kinds 4, 5, 7 (mean)"] = sum(per) / len(per)
    assert sum(per) >= 4 * len(per), per
    for wave in corp.waves():
        up = [c for c in wave if len(corp.trace(c).carries(LONG_RUN))]
        down = [c for c in wave if len(corp.trace(c).stands(LONG_RUN))]
        assert up and down, ("a wave without a long run ended in a carry, or without one left standing", wave, up, down)
    seen["channels with a carry after >= 160 owed bits"] = sum(1 for c in range(corp.C) if len(corp.trace(c).carries(LONG_RUN)))
    seen["channels with >= 160 owed bits settled without a carry"] = sum(1 for c in range(corp.C) if len(corp.trace(c).stands(LONG_RUN)))
    seen["longest run of owed bits"] = max(int(corp.trace(c).ev_pend.max()) for c in corp.of_kind(4, 5, 7))

    def words(c, what):
        t = corp.trace(c)
        tot, f2 = t.word_tot.astype(np.int64) + 31, t.word_f2.astype(np.int64)
        return int((tot > 128 * f2).sum()) if what == "bits" else int(((tot > 11 * f2) & (tot <= 128 * f2)).sum())

    bits_words = [words(c, "bits") for c in corp.of_kind(1)]
    seen["kind 1: words that begin with tot + 31 > 128 f2 (min, max)"] = (min(bits_words), max(bits_words))
    assert min(bits_words) >= 10
    fast4 = [words(c, "fast4") for c in corp.of_kind(2)]
    seen["kind 2: words with 11 f2 < tot + 31 <= 128 f2 (min, max)"] = (min(fast4), max(fast4))
    assert min(fast4) >= 5
    for c in corp.of_kind(2):  # ... and both limits are crossed in both directions
        t = corp.trace(c)
        tot, f2 = t.word_tot.astype(np.int64) + 31, t.word_f2.astype(np.int64)
        for lim in (11, 128):
            over = (tot > lim * f2).astype(np.int8)
            assert (np.diff(over) == 1).any() and (np.diff(over) == -1).any(), (c, lim)
    swaps = [len(corp.trace(c).swap_sym) for c in corp.of_kind(3)]
    seen["kind 3: exchanges of the two symbols (min, max)"] = (min(swaps), max(swaps))
    assert min(swaps) >= 8
    halvings = [corp.trace(c).halve_sym for c in corp.of_kind(6)]
    seen["kind 6: halvings (min, max)"] = (min(len(h) for h in halvings), max(len(h) for h in halvings))
    seen["kind 6: coded bits (min, max)"] = (min(corp.trace(c).seg_bits for c in corp.of_kind(6)), max(corp.trace(c).seg_bits for c in corp.of_kind(6)))
    assert min(len(h) for h in halvings) >= 1
    # ... at places that differ among the lanes of a wave.  cum[0] grows by one per coded bit, so the FIRST halving is at
    # coded bit 16380 in every channel there is; what differs is the row at which a lane gets there (the waves step through
    # the rows together), and with it the phase of every later word against the rows.
    for wave in corp.waves():
        first = [int(corp.trace(c).halve_row[0]) for c in wave if corp.kind[c] == 6]
        assert len(first) < 2 or len(set(first)) > len(first) // 2, (wave, first)  # (no two lanes need differ, most do)
    seen["kind 6: row of the first halving (min, max)"] = (min(int(h[0]) for h in (corp.trace(c).halve_row for c in corp.of_kind(6))),
                                                           max(int(h[0]) for h in (corp.trace(c).halve_row for c in corp.of_kind(6))))
    # A SECOND halving does come at a coded bit of the lane's own (cum[0] restarts at 8193 or 8194, as the parities of the
    # three counts fall): among the channels that have one, the positions differ.
    second = [int(h[1]) for h in halvings if len(h) > 1]
    seen["kind 6: coded bit of the second halving (channels, positions)"] = (len(second), sorted(set(second)))
    assert len(second) >= 2 and len(set(second)) > 1, second
    ones = max(longest_run(corp.trace(c).stream, corp.trace(c).nbits, 1) for c in corp.of_kind(4, 5, 7))
    zeros = max(longest_run(corp.trace(c).stream, corp.trace(c).nbits, 0) for c in corp.of_kind(4, 5, 7))
    seen["longest runs of one-bits and of zero-bits in a stream"] = (ones, zeros)
    assert ones >= 195
    return seen


# ---- the checkers ------------------------------------------------------------------------------------------------------------
def check_full(corp, ad, out, bits, err, what="", channels=None):
    """status, bit length and every byte of the slab are the oracle's (channels: the results are those of these channels)"""
    want_out, want_bits, want_err = corp.oracle(ad)
    if channels is not None:
        want_out, want_bits, want_err = want_out[channels], want_bits[channels], want_err[channels]
    out, bits, err = np.asarray(out), np.asarray(bits).astype(np.uint64), np.asarray(err)
    assert (err == want_err).all(), (what, ad, "status", np.flatnonzero(err != want_err)[:8].tolist(), err[err != want_err][:8].tolist())
    assert (bits == want_bits).all(), (what, ad, "bit length", np.flatnonzero(bits != want_bits)[:8].tolist())
    n = min(out.shape[1], want_out.shape[1])
    bad = np.flatnonzero((out[:, :n] != want_out[:, :n]).any(axis=1))
    assert len(bad) == 0, (what, ad, "bytes", [(int(c), int(np.flatnonzero(out[c, :n] != want_out[c, :n])[0])) for c in bad[:8]])
    assert not out[:, n:].any() and not want_out[:, n:].any()


def check_short(corp, ad, cap, out, bits, err, what=""):
    """The short-slab contract, per channel: ERROR_MEMORY (-6) where the stream does not fit `cap` bytes (0 where it does:
    the still channels' streams are a few bytes), the oracle's length either way, and every byte below cap is the byte of
    the oracle's full stream."""
    want_out, want_bits, _ = corp.oracle(ad)
    out, bits, err = np.asarray(out), np.asarray(bits).astype(np.uint64), np.asarray(err)
    assert out.shape[1] == cap
    want_err = np.where((want_bits + np.uint64(7)) // np.uint64(8) > cap, orc.ERROR_MEMORY, 0)
    assert (err == want_err).all(), (what, ad, cap, "status", np.flatnonzero(err != want_err)[:8].tolist())
    assert (bits == want_bits).all(), (what, ad, cap, "bit length", np.flatnonzero(bits != want_bits)[:8].tolist())
    bad = np.flatnonzero((out != want_out[:, :cap]).any(axis=1))
    assert len(bad) == 0, (what, ad, cap, "bytes in front of the cap", [(int(c), KINDS[c % 8], int(np.flatnonzero(out[c] != want_out[c, :cap])[0])) for c in bad[:8]])


def check_short_is_not_vacuous(corp, cap):
    """at least 3 channels have a carry after >= 33 owed bits BEYOND the cap (from the replay): a writer that lets such a
    carry run into the words it kept spoils bytes in front of the cap"""
    n = len(corp.carries_beyond(cap))
    assert n >= 3, (cap, n)
    return n
