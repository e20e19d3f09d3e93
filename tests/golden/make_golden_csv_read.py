#!/usr/bin/env python3
"""Generates tests/golden/csv_read.npz from the COMPILED REFERENCE LIBRARY in process (oracle/_ref/libdcref.so through
orc.ref_run_chain, as make_golden_csv.py does for the other direction).  Build container only:

    make -C oracle && python tests/golden/make_golden_csv_read.py

`decode csv` (ReadCSV, DCLib/src/csv.c:13-44) splits a text into fields and writes strtof(field) for every field of the
chosen column.  Data only.  Per case `name`:
  <name>.opt    int64 [2]   column, separator_char
  <name>.text   uint8 [..]  the text given to the reference -- absent for the cases that read the writer's fixture back
                            (back.<list>.d<d>: <list>.d<d>.text of csv.npz; back.<chain>.c<c>: channel c of <chain>.text) and
                            for `input` (input.txt.gz)
  <name>.bits   uint32 [n]  the floats it returned, as bit patterns -- for the cases without a text of their own <name>.xor
                            instead: those bit patterns xor float32(float(field)) (csv_read_common.predicted), which is zero
                            on nearly all of the writer's 130 000 lines and keeps the file small; the tests undo it
Nothing of 48 or more characters in a selected field is given to the reference: its field buffer has 48 bytes
(csv.c:11,18).  The tests check those against the stated error instead.

The generator asserts three things, so that the fixture cannot go blind: libc's strtof through ctypes agrees with the
reference on every stored field; float32(float(field)) -- double rounding -- disagrees on some stored field; keeping only
19 significant digits disagrees on some stored field.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import orc  # noqa: E402
import csv_read_common as crc  # noqa: E402
from csv_common import Fixture, input_series, input_txt  # noqa: E402


def ref_floats(text, column, sep):
    ret, b, n, _ = orc.ref_run_chain(text, 8 * len(text), ["decode csv column=%d separator_char=%s" % (column, chr(sep))])
    assert ret == 0 and n % 32 == 0, (ret, n)
    return np.frombuffer(b, dtype=np.uint32).copy()


GRAMMAR = ["0", "-0", "+0", "1e", "1e+", "1e-", "5.", ".5", ".", "-.", "+.5", "1", "-1", "1.5", "abc", "-", "-abc", "+", "1e5", "1E5", "1e+5", "1e-5", "1.e5",
           ".e5", "1e5.5", "1..", "1.2.3", "12abc", "1e5e5", "0e5000", "00012.500", "000", "0.0", "-0.0", "-0.00", "1_000", "1,5", "0x", "-0x", "0xg",
           "0x1", "0X1", "0x1.8", "0x.8", "0x.", "0x.p1", "0xp1", "0x0p5", "0x1p", "0x1p+", "0x1p-", "0x1p4", "0X1P+4", "0x1p-4", "0x1e2", "1p3", "0x1.p1",
           "0x1.000001p0", "0x1.000003p0", "0x1.000002p0", "0x1.0000018p0", "0x1.00000100000000000000000000000001p0", "0x1.fffffep127",
           "0x1.ffffffp127", "0x1.fffffefp127", "0x1p128", "0x1p-149", "0x1p-150", "0x1.8p-150", "0x1.000001p-150", "0x1p-151", "0x1.fffffcp-127",
           "0x1.fffffep-127", "0x1.ffffffp-127", "0x0.000001p-126", "0x123456789abcdef", "0x1ffffffffffffffff1", "0xABCDEF", "0x.0000000000000000001p70",
           "inf", "INF", "Inf", "-inf", "+inf", "infinity", "INFINITY", "-Infinity", "infinit", "infin", "in", "i", "infx", "infinityx", "nan", "NAN", "NaN",
           "-nan", "+nan", "n", "na", "nanx", "nan(", "nan()", "NAN()", "nan(0)", "nan(1)", "nan(123)", "nan(0x123)", "-nan(0x7fffff)", "nan(0x3fffff)",
           "nan(0x400000)", "nan(0x400001)", "nan(zz)", "nan(09)", "nan(017)", "nan(0x)", "nan(0xg)", "nan(_)", "nan(1_)", "nan(1)x", "nan(1", "nan( 1)",
           "nan(18446744073709551615)", "nan(18446744073709551616)", "nan(99999999999999999999999)", "nan(0xffffffffffffffffff)", "NAN(0X1F)",
           " 1.5", "  -2.5", "\t3.5", "\v4.5", "\f5.5", "\r6.5", " \t\v\f\r 7.5", "1.5 ", "1 .5", "- 1", " ", "\t", "3.40282347e38", "3.40282346e38",
           "3.40282348e38", "3.40282357e38", "3.4028235677973366e38", "3.4028235677973367e38", "3.4028235677973365e38", "3.4028235677973366164e38",
           "340282346638528859811704183484516925440", "340282356779733661637539395458142568447", "340282356779733661637539395458142568448",
           "340282356779733661637539395458142568449", "-340282356779733661637539395458142568448", "1e38", "1e39", "-1e39", "1e40", "1e+38", "123456789e31",
           "0.000001e45", "1e5000", "-1e5000", "1e-5000", "1e99999999999999999999", "1e-99999999999999999999", "1e-45", "1e-46", "1e-47", "7e-46", "8e-46",
           "1.4e-45", "2.1e-45", "2.2e-45", "7.006492321624085e-46", "7.0064923216240853546186479164495806e-46", "7.0064923216240853546186479164495807e-46",
           "7.0064923216240853546186479164495808e-46", "1.4012984643248170709237295832899161e-45", "2.1019476964872256063855943749348742e-45",
           "2.1019476964872256063855943749348741e-45", "0.000000000000000000000000000000000000000000001", "0.00000000000000000000000000000000000000000001",
           "1.17549435e-38", "1.17549428e-38", "1.1754943508222875e-38", "1.1754942807573643e-38", "1.1754943157898259e-38", "16777216", "16777217",
           "16777218", "16777219", "16777217.0000000000000000000000000000000000001", "9007199254740993", "1.00000005960464477539062500000000000000000001",
           "1.000000059604644775390625", "1.0000000596046447753906249999999999999999999", "12345678901234567890", "1234567890123456789",
           "1234567891234567891234567891234567891234567", "9999999999999999999999999999999999999999999999", "0.99999999999999999999999999999999999999999999",
           "0.1", "0.2", "0.3", "7405.30", "12.34", "-12.34", "0.01", "100000000000000000000", "00000000000000000000000000000000000000000001.5"]


def binade_fields():
    """the first and last float of every binade and their neighbours, as nine significant digits (which read back exactly)
    and as 40 digits cut off (which do not always)"""
    from decimal import Decimal
    out = []
    for E in range(0, 255, 3):
        for M in (0, 1, 0x7FFFFF):
            bits = (E << 23) | M
            if bits == 0:
                continue
            x = float(np.array([bits], dtype=np.uint32).view(np.float32)[0])
            out.append("%.8e" % x)
            out.append(format(Decimal(x), ".39E")[:46])
    return out


def small_cases():
    """texts that end without a newline, in a separator, in a newline; empty fields, short lines; other columns"""
    c = {}
    c["end.plain"] = (b"1.5\n2.5\n3.5", 1, ",")
    c["end.newline"] = (b"1.5\n2.5\n3.5\n", 1, ",")
    c["end.two_newlines"] = (b"1.5\n2.5\n\n", 1, ",")
    c["end.separator"] = (b"1.5,9\n2.5,9\n3.5,", 1, ",")
    c["end.separator_col2"] = (b"1.5,9\n2.5,8\n3.5,7,", 2, ",")
    c["end.separator_only"] = (b",", 1, ",")
    c["end.one_byte"] = (b"7", 1, ",")
    c["end.one_newline"] = (b"\n", 1, ",")
    c["end.digit_is_last_of_other_column"] = (b"1,2\n3,4", 1, ",")
    c["end.last_byte_joins_number"] = (b"1,2\n3,45", 2, ",")
    c["empty.fields"] = (b"\n\n1\n\n,\n,,\n2,\n", 1, ",")
    c["empty.col2"] = (b"1\n1,\n1,2\n1,,3\n,\n,5\n1,2,3\n\n9,8", 2, ",")
    c["short.col3"] = (b"1;2;3\n4;5\n6\n;;7\n;;\n8;9;10;11\n;;;\n1;2;3.5;4\n", 3, ";")
    c["crlf"] = (b"1.5\r\n2.5\r\n-3.25\r\n\r\n4\r\n", 1, ",")
    c["crlf.col2"] = (b"a,1.5\r\nb,2.5\r\nc\r\nd,\r\n", 2, ",")
    c["tab.separator"] = (b"1\t2\t3\n4\t5\t6\n", 2, "\t")
    c["colon.separator"] = (b"1:2:3\n4:5:6\n", 3, ":")
    c["long.other_column"] = (b"1," + b"9" * 80 + b",3\n4," + b"8" * 60 + b",6\n", 3, ",")
    c["long.other_column_first"] = (b"9" * 100 + b";2\n" + b"8" * 48 + b";5\n", 2, ";")
    c["line47"] = (b"-340282346638528859811704183484516925440.000000\n1\n", 1, ",")
    return c


def main():
    assert orc.have_ref(), "oracle/_ref/libdcref.so is not built (make -C oracle)"
    rng = np.random.default_rng(20154)
    out = {}
    stored = double_differs = trunc_differs = 0

    def add(name, text, column, sep, keep_text=True):
        nonlocal stored, double_differs, trunc_differs
        sep = ord(sep) if isinstance(sep, str) else int(sep)
        fields, status = crc.split(text, column, sep)
        assert status == 0 and all(len(f) < crc.FIELD_LIMIT for f in fields), name
        bits = ref_floats(text, column, sep)
        assert bits.size == len(fields), (name, bits.size, len(fields))
        for f, b in zip(fields, bits.tolist()):
            assert crc.strtof_bits(f) == b, (name, f, hex(b), hex(crc.strtof_bits(f)))
            plain = f.strip().lstrip(b"+-")
            if plain and plain.replace(b".", b"", 1).isdigit() and b & 0x7FFFFFFF < 0x7F800000:
                double_differs += crc.float32_via_double(f.strip()) != b
                trunc_differs += crc.strtof_bits(crc.truncated_19(f)) != b
            stored += 1
        out[name + ".opt"] = np.array([column, sep], dtype=np.int64)
        if keep_text:
            out[name + ".bits"] = bits
            out[name + ".text"] = np.frombuffer(text, dtype=np.uint8)
        else:  # many lines of the writer's: the difference to float32(float(field)), zero nearly everywhere
            out[name + ".xor"] = bits ^ crc.predicted(fields)
        return bits

    # every line of csv.npz read back
    fx = Fixture()
    for name in fx.lists():
        column, sep = fx.options(name)
        for d in range(7):
            add("back.%s.d%d" % (name, d), fx.z["%s.d%d.text" % (name, d)].tobytes(), column, sep, keep_text=False)
    for key in ("meter.plain", "meter.N1", "meter.N7", "meter.N60", "series.N60"):
        for c, t in enumerate(fx.chain(key)[0]):
            add("back.%s.c%d" % (key, c), t, 1, ",", keep_text=False)
    series = add("input", input_txt(), 1, ",", keep_text=False)
    assert (series == input_series().view(np.uint32).ravel()).all(), "`decode csv` of input.txt is not csv_common.input_series()"

    add("grammar", crc.lines_text([s.encode() for s in GRAMMAR]), 1, ",")
    add("grammar.col3", b"".join(b"x;;" + s.encode() + b";y\n" for s in GRAMMAR if ";" not in s), 3, ";")
    add("binades", crc.lines_text([s.encode() for s in binade_fields()]), 1, ",")
    add("midpoints", crc.lines_text(crc.short_one_last(crc.fields_midpoints(rng, 1500))), 1, ",")
    add("digits", crc.lines_text(crc.short_one_last(crc.fields_digits(rng, 400))), 1, ",")
    add("exponents", crc.lines_text(crc.short_one_last(crc.fields_exponents(rng, 400))), 1, ",")
    add("hex", crc.lines_text(crc.short_one_last(crc.fields_hex(rng, 400))), 1, ",")
    for name, (text, column, sep) in small_cases().items():
        add(name, text, column, sep)
    # every field of the grammar list once more as a text of its own, without a newline and behind one: the last byte
    for i, s in enumerate(GRAMMAR[::7]):
        add("alone.%03d" % i, s.encode() if s else b"\n", 1, ",")
        add("alone_col2.%03d" % i, b"0," + s.encode() + b",", 2, ",")

    assert double_differs > 0 and trunc_differs > 0, (double_differs, trunc_differs)
    path = os.path.join(HERE, "csv_read.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes; %d fields stored; double rounding differs on %d, 19 digits on %d"
          % (path, len(out), os.path.getsize(path), stored, double_differs, trunc_differs))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "csv.npz"))


if __name__ == "__main__":
    main()
