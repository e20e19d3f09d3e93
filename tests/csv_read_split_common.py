"""Shared by tests/test_csv_read_split_host.py and tests/test_gpu_csv_read_split.py: the batches built to put block edges at
every place of a line (closed form, no random numbers), the fields of 48 characters and more, and the rooms too small.  A
batch is (what, texts, column, separator); what is expected of it comes from csv_read_common.expected (csv.c:20-42
restated and libc's strtof).  The split reader itself is handed in as `run`."""
import numpy as np

import csv_read_common as crc

FILLER = 0x7FC12345  # what rows at or beyond max_T and columns C .. ld - 1 hold: no call may touch it (the existing tests' convention)
LONG47 = b"-340282346638528859811704183484516925440.000000"
assert len(LONG47) == 47


def two_decimal_lines(n):
    """n two-decimal fields in closed form: signs, leading zeros, one to five digits in front of the point"""
    return [("%s%d.%02d" % ("-" if i % 5 == 3 else "", (i * i * 37 + 11 * i) % (10 ** (1 + i % 5)), (i * 29) % 100)).encode() for i in range(n)]


def ladder(B):
    """the batches of the block-edge ladder for blocks of B bytes: [(what, texts, column, sep)]"""
    base = crc.lines_text(two_decimal_lines(30))
    out = []
    # a first line of k bytes in front: a newline on the last byte of a block, on the first byte of the next, and between
    # (behind its first field the line goes on in a column that is not read, so that it may be longer than a field)
    first = lambda k: (b"7," + b"7" * (k - 3) if k >= 3 else b"7" * (k - 1)) + b"\n" if k else b""  # noqa: E731
    assert all(len(first(k)) == k for k in range(B + 2))
    out.append(("first line of k bytes", [first(k) + base for k in range(B + 2)], 1, ","))
    # every text length: the last byte is a digit, a point, a '-' or a newline
    out.append(("every length", [base[:n] for n in range(101)], 1, ","))
    assert {t[-1:] for t in out[-1][1]} >= {b"-", b".", b"\n"} and any(t[-1:].isdigit() for t in out[-1][1])
    # lines longer than a block: blocks that own nothing
    out.append(("47 characters", [crc.lines_text([LONG47] * 9 + [b"1.25"]), crc.lines_text([b"0" * 46 + b"7", b"2.50", LONG47, b"3"]),
                                  b"\n" * 3 + LONG47 + b"\n" + b"4\n"], 1, ","))
    out.append(("empty lines", [b"\n" * 500, b"\n" * 499 + b"1", b"\n"], 1, ","))
    out.append(("crlf", [b"".join(f + b"\r\n" for f in two_decimal_lines(25)), b"\r\n" * 40, b"1.5\r\n2.5\r"], 1, ","))
    for column in (1, 2):
        out.append(("ends in the separator, column %d" % column, [b"1,2\n3,4\n5,", b"1,2\n3,4\n5,6,", b"," * (B + 1), b"1.5,2.5\n" * 7 + b"9,", b","], column, ","))
    # separators and newlines at every offset against the block edges; a line with fewer fields than `column` across an edge
    for column, sep in ((2, ","), (3, ";")):
        s = sep.encode()
        texts = []
        for k in range(B + 2):
            lines = [b"9" * k + s + b"1.25" + s + b"-2.50" + s + b"x", b"3" + s + b"4.75" + s + b"5.5", b"6" * (B - 2), b"7" + s + b"8.25", s + s + s,
                     b"", b"1" + s + b"2" + s + b"3"]
            texts.append(b"".join(x + b"\n" for x in lines) + b"4" + s + b"5" + s + b"6")
        out.append(("column %d, separator %r" % (column, sep), texts, column, sep))
    return out


def long_field_cases():
    """(text, column, values in front, too long?): the ten cases of the unsplit kernel's test, then two long fields in
    different blocks (the first decides), a long field across block edges, and one in a column that is not read"""
    return [
        (b"1\n2\n" + b"1" * 48 + b"\n3\n", 1, 2, True),
        (b"1" * 48, 1, 0, True),
        (b"1" * 47, 1, 1, False),
        (LONG47 + b"\n1\n", 1, 2, False),
        (b"5\n" + LONG47 + b"\n", 1, 1, True),  # the last line: its newline is appended
        (b"5\n" + LONG47, 1, 2, False),
        (b"1,2\n3," + b"0" * 47 + b"7\n5,6\n", 2, 1, True),
        (b"1,2\n3," + b"0" * 47 + b"7\n5,6\n", 1, 3, False),  # (too long, but in a column that is not read)
        (b" " * 47 + b"1\n", 1, 0, True),
        (b"1.5\n" * 40 + b"9" * 100 + b"\n" + b"2.5\n" * 40, 1, 40, True),
        (b"1.5\n" * 10 + b"8" * 48 + b"\n" + b"2.5\n" * 50 + b"9" * 60 + b"\n3.5\n", 1, 10, True),  # two, far apart: the first decides
        (b"1\n" * 5 + b"2" * 50 + b"\n" + b"3" * 49 + b"\n" + b"4\n" * 5, 1, 5, True),  # two, one behind the other
        (b"12345678\n" + b"6" * 48 + b"\n7\n", 1, 1, True),  # starts at byte 9: across the edges at 16, 32 and 48
        (b"1,22\n3," + b"4" * 70 + b"\n" + b"5,66\n" * 9, 2, 1, True),
        (b"1,22\n3," + b"4" * 70 + b"\n" + b"5,66\n" * 9, 1, 11, False),  # (in a column that is not read)
        (b"1.25\n" * 60, 1, 60, False),  # valid lines beside the flagged ones: they must not notice
    ]


LONG_FLAGGED = 10


def room_set():
    """the 70 channels of the unsplit kernel's room test: channel c has c % 40 + 1 values"""
    rng = np.random.default_rng(12)
    fields = crc.fields_printed(rng, 3000, 2)
    texts, want = [], []
    for c in range(70):
        mine = fields[40 * c: 40 * c + (c % 40) + 1]
        texts.append(crc.lines_text(mine))
        want.append(np.array([crc.strtof_bits(f) for f in mine], dtype=np.uint32))
    return texts, want


ROOMS = (0, 1, 7, 16, 17, 39, 40)


def check_ladder(run, B):
    """every batch of the ladder through run(texts, max_T, column, sep, B) -> (v uint32 [max_T][ld], count, err); returns the
    number of values compared.  No status but 0 is expected anywhere."""
    n = 0
    for what, texts, column, sep in ladder(B):
        want, status = zip(*[crc.expected(t, column, sep) for t in texts])
        assert all(s == 0 for s in status), what
        max_T = max(len(w) for w in want) + 1
        v, count, err = run(texts, max_T, column, sep, B)
        n += crc.check_channels(v, count, err, want, status, max_T, (what, B))
    return n


def check_long_fields(run, B):
    """the cases of long_field_cases() through run(), grouped by column; returns the number of flagged channels"""
    flagged = 0
    for column in (1, 2):
        mine = [c for c in long_field_cases() if c[1] == column]
        texts = [c[0] for c in mine]
        want, status = zip(*[crc.expected(t, column) for t in texts])
        for (t, _, n, long_), w, s in zip(mine, want, status):
            assert len(w) == n and (s == crc.ERROR_INVALID_FORMAT) == long_, t
            flagged += long_
        v, count, err = run(texts, 64, column, ",", B)
        crc.check_channels(v, count, err, want, status, 64, (column, B))
        assert int((err != 0).sum()) == sum(c[3] for c in mine)
    return flagged
