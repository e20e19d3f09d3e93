"""Shared by tests/test_csv_write_split_host.py and tests/test_gpu_csv_write_split.py: the batches built to put block edges
at every byte of an 8-byte word (closed form, no random numbers), the values where a digit count by comparisons could part
from the digits, the counts, and the check every test ends with.  What is expected comes from csv_common.py_lines (pinned to
the compiled reference by test_csv_host.test_fixture_is_not_blind) or from the fixture itself.  The split writer is handed
in as run(batch uint32 [T][ld], Cn, d, column, sep, stride, block_rows, count) -> (rows uint8 [Cn][stride] that were
pre-filled with CANARY, lens, err)."""
import numpy as np

from csv_common import ERROR_MEMORY, SLACK, arrange, py_lines

CANARY = 0xEE  # no byte of any text: digits, '-', '.', '\n', separators, "inf", "nan"
ERROR_INVALID_VALUE = -1
NAN, INF, NEG_INF = 0x7FC00000, 0x7F800000, 0xFF800000


def f32_bits(values):
    return np.array(values, dtype=np.float64).astype(np.float32).view(np.uint32)


def stride_for(texts, spare=0):
    """the smallest legal stride that fits every text, plus `spare` multiples of 16"""
    return (max([len(t) for t in texts] + [0]) + SLACK + 15) // 16 * 16 + 16 * spare


def check(rows, lens, err, want, stride, what, invalid=()):
    """exact bytes and exact lengths for every channel that fits, and the canary from lens[c] on; ERROR_MEMORY (or, for the
    channels of `invalid`, ERROR_INVALID_VALUE), length 0 and an untouched row for every other.  Returns (fit, refused)."""
    rows = np.asarray(rows)
    assert rows.shape == (len(want), stride), (what, rows.shape)
    fit = over = 0
    for c, w in enumerate(want):
        if c in invalid:
            code, n = ERROR_INVALID_VALUE, 0
        elif len(w) + SLACK <= stride:
            code, n = 0, len(w)
        else:
            code, n = ERROR_MEMORY, 0
        assert int(err[c]) == code and int(lens[c]) == n, (what, c, int(err[c]), int(lens[c]), code, n)
        assert rows[c, :n].tobytes() == w[:n], (what, c)
        assert (rows[c, n:] == CANARY).all(), (what, c, "a byte at or beyond out_len was written")
        fit += code == 0
        over += code != 0
    return fit, over


# ---- the edge ladder: every (offset mod 8, line length) for lines of 2 .. 24 bytes -----------------------------------------

LADDER_LENGTHS = tuple(range(2, 25))


def ladder_series():
    """readings for d = 0 whose lines put one of every length 2 .. 24 at every offset mod 8: `0` (2 bytes) and `-7` (3
    bytes) move the offset, then 3 x 10^k (k + 2 bytes) or its negative (k + 3 bytes) is the line.  float64 values."""
    step = {0: [], 1: [3, 3, 3], 2: [2], 3: [3], 4: [2, 2], 5: [2, 3], 6: [3, 3], 7: [2, 2, 3]}
    short = {2: 0.0, 3: -7.0}
    values, at = [], 0
    for length in LADDER_LENGTHS:
        for offset in range(8):
            for n in step[(offset - at) % 8]:
                values.append(short[n])
                at += n
            assert at % 8 == offset
            values.append(-3.0 * 10.0 ** (length - 3) if length >= 3 and offset % 2 else 3.0 * 10.0 ** (length - 2))
            at += length
    return values


def ladder_batch():
    """(batch uint32 [T][3], texts of the 2 channels): the series, and the series backwards (other edges, same lines)"""
    bits = f32_bits(ladder_series())
    T = bits.size
    batch = np.full((T, 3), 0x7FC12345, dtype=np.uint32)
    batch[:, 0] = bits
    batch[:, 1] = bits[::-1]
    texts = [b"".join(py_lines(batch[:, c], 0)) for c in range(2)]
    return batch, texts


def ladder_coverage(text, block_rows=1):
    """from an expected text alone: the set of (offset mod 8, length) of its blocks of block_rows lines, and how many blocks
    lie wholly inside one 8-byte word with a neighbour on both sides"""
    lines = text.split(b"\n")[:-1]
    pairs, inside, at = set(), 0, 0
    for i in range(0, len(lines), block_rows):
        n = sum(len(s) + 1 for s in lines[i: i + block_rows])
        pairs.add((at % 8, n))
        if at % 8 != 0 and at % 8 + n < 8 and i + block_rows < len(lines):
            inside += 1
        at += n
    return pairs, inside


def check_ladder(run, block_rows):
    batch, texts = ladder_batch()
    pairs, inside = ladder_coverage(texts[0])
    assert pairs >= {(o, n) for o in range(8) for n in LADDER_LENGTHS} and inside >= 40, "the series does not cover what it was built for"
    stride = stride_for(texts)
    rows, lens, err = run(batch, 2, 0, 1, ",", stride, block_rows, None)
    assert check(rows, lens, err, texts, stride, ("ladder", block_rows)) == (2, 0)
    return batch.shape[0]


# ---- the digit-count ladder: where a count by comparisons could part from the digits ---------------------------------------

def digit_ladder_bits():
    """10^k and its float32 neighbours for k = 0 .. 38, both signs, then the carries: values that round up into one digit more"""
    powers = f32_bits([10.0 ** k for k in range(39)])
    around = np.concatenate([powers - 1, powers, powers + 1]).astype(np.uint32)
    carries = [9.995, 99999.996, 0.9999995, 0.5, 1.5, 2.5, 9.5, 10.5, 99.5, 999.5, 9999.5, 99999.5, 999999.5, 9999999.0, 0.95, 0.995, 0.9995, 9.9995,
               99.995, 99.9951, 999.995, 9999.995, 999.9995, 0.99999949, 0.99999951, 9.9999995, 99.999995, 9.4999995, 0.4999999, 0.05, 0.005, 0.0000005,
               16777215.0, 16777216.0, 67108860.0, 67108864.0, 67108868.0, 99999992.0, 99999996.0, 100000000.0, 100000008.0, 999999936.0,
               4294967296.0, 9999999.5, 3.4028234663852886e38, 1.401298464324817e-45, 1.1754943508222875e-38]
    c = f32_bits(carries)
    near = np.concatenate([c - 1, c, c + 1]).astype(np.uint32)
    both = np.concatenate([around, near])
    return np.concatenate([both, both | np.uint32(0x80000000), np.array([NAN, INF, NEG_INF, NAN | 0x80000000, 0, 0x80000000], dtype=np.uint32)])


DIGIT_DECIMALS = (0, 2, 6)


def check_digit_ladder(run, block_rows, Cn=3):
    n = 0
    bits = digit_ladder_bits()
    for d in DIGIT_DECIMALS:
        lines = py_lines(bits, d)
        batch, want = arrange(bits, lines, Cn, Cn + 1, py_lines([0], d)[0])
        stride = stride_for(want)
        rows, lens, err = run(batch, Cn, d, 1, ",", stride, block_rows, None)
        assert check(rows, lens, err, want, stride, ("digits", d, block_rows)) == (Cn, 0)
        n += len(lines)
    return n


# ---- counts ----------------------------------------------------------------------------------------------------------------

COUNT_T, COUNT_BLOCK_ROWS = 20, 4
COUNTS = (0, 6, 8, 20, 21, 1, 19)  # none; mid-block; on a block edge; T; T + 1: INVALID_VALUE; one; T - 1


def counts_batch(d=2):
    """(batch uint32 [T][ld], counts, texts, the channels over T): two-decimal readings; the rows behind a channel's count
    hold NaN and infinities in turn, which must influence nothing"""
    Cn = len(COUNTS)
    i = np.arange(COUNT_T * Cn, dtype=np.float64)
    vals = ((i * i * 37.0 + 11.0 * i) % 100000.0) / 100.0 * np.where(i % 5 == 3, -1.0, 1.0)
    batch = np.full((COUNT_T, Cn + 2), 0x7FC12345, dtype=np.uint32)
    batch[:, :Cn] = f32_bits(vals).reshape(COUNT_T, Cn)
    texts = []
    for c, n in enumerate(COUNTS):
        k = n if n <= COUNT_T else 0
        texts.append(b"".join(py_lines(batch[:k, c], d)))
        batch[k:, c] = np.resize(np.array([NAN, INF, NEG_INF], dtype=np.uint32), COUNT_T - k)
    invalid = {c for c, n in enumerate(COUNTS) if n > COUNT_T}
    return batch, np.array(COUNTS, dtype=np.uint64), texts, invalid


def check_counts(run, block_rows=COUNT_BLOCK_ROWS):
    batch, counts, texts, invalid = counts_batch()
    stride = stride_for(texts)
    rows, lens, err = run(batch, len(COUNTS), 2, 1, ",", stride, block_rows, counts)
    fit, refused = check(rows, lens, err, texts, stride, ("counts", block_rows), invalid)
    assert (fit, refused) == (len(COUNTS) - 1, 1) and int(err[4]) == ERROR_INVALID_VALUE


# ---- room ------------------------------------------------------------------------------------------------------------------

def room_boundary(bits, lines):
    """the shortest prefix of one channel's lines that ends 16 bytes before a multiple of 16: (T, its length)"""
    total = 0
    for T, s in enumerate(lines[:64], 1):
        total += len(s)
        if (total + SLACK) % 16 == 0:
            return T, total
    raise AssertionError("no prefix of the list ends 16 bytes before a multiple of 16")
