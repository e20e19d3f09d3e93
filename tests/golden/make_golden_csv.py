#!/usr/bin/env python3
"""Generates tests/golden/csv.npz from the COMPILED REFERENCE LIBRARY in process (oracle/_ref/libdcref.so through
orc.ref_run_chain; not the DCCLI binary, whose start-up code flushes subnormals).  Build container only:

    make -C oracle && python tests/golden/make_golden_csv.py

`encode csv` (WriteCSV, DCLib/src/csv.c:46-65) writes, per float32 reading, `column - 1` separators and "%.*f\\n".  Data only.
Per list of values `name` (LISTS below) and num_decimal_places d = 0 .. 6:
  <name>.bits          uint32 [n]   the readings as bit patterns (NaN payloads and signs survive)
  <name>.d<d>.keep     bool [n]     which of them the reference was given (see below)
  <name>.d<d>.text     uint8 [..]   what it wrote for those, one '\\n'-terminated line per kept value, in order
`col3.*` is the edge list again with `column=3 separator_char=;`.
Lines of 48 characters or more are LEFT OUT (keep = False): the reference's line buffer has 48 bytes (csv.c:11) and the
fortified build aborts there; the tests check those against Python's formatting instead.
Chains, num_decimal_places 2, per channel of `meter.v` (float32 [T][C]; channel 0 starts with a -0.0f reading):
  meter.plain.*        `encode csv # encode lzmh`
  meter.N<N>.*         `encode aggregate num_values=N # encode csv # encode lzmh`, N = 1, 7, 60
  with  .text uint8 [C][longest] / .text_len int64 [C] / .stream uint8 [C][longest] / .bits uint64 [C]
  series.N60.*         the same chain over the reference's own series (input.txt.gz after `decode csv`), one channel;
                       its plain text is input.txt again (asserted here, not stored twice)

The generator asserts three things, so that the fixture cannot go blind: Python's "%.*f" reproduces the reference on
every stored line except `nan` with the sign bit set (glibc prints -nan); truncation instead of rounding differs on some
stored line; round-half-up instead of half-to-even differs on some stored line.
"""
import gzip
import os
import sys
from decimal import ROUND_DOWN, ROUND_HALF_UP, Decimal, localcontext

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import orc  # noqa: E402

DECIMALS = range(7)
LINE_LIMIT = 48  # csv.c:11


def f32(values):
    return np.array(values, dtype=np.float32).view(np.uint32)


def as_float(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def py_line(bits, d, prefix=""):
    """Python's formatting of one reading, with glibc's sign of NaN"""
    x = as_float(bits)
    s = ("-nan" if bits >> 31 else "nan") if np.isnan(x) else "%.*f" % (d, float(x))
    return prefix + s + "\n"


def other_rounding(bits, d, mode):
    x = as_float(bits)
    if not np.isfinite(x):
        return py_line(bits, d)
    with localcontext() as ctx:
        ctx.prec = 200  # FLT_MAX has 39 digits, the smallest subnormal 149 decimals
        return format(Decimal(float(x)).quantize(Decimal(1).scaleb(-d), rounding=mode), "f") + "\n"


def ref_text(bits, options):
    data = np.ascontiguousarray(bits, dtype=np.uint32).tobytes()
    ret, b, n, _ = orc.ref_run_chain(data, 8 * len(data), ["encode csv " + options])
    assert ret == 0 and n % 8 == 0, (ret, n)
    return b


def ref_chain(col, stages):
    col = np.ascontiguousarray(col, dtype=np.float32)
    ret, b, n, _ = orc.ref_run_chain(col.tobytes(), 32 * col.size, stages)
    assert ret == 0, (ret, stages)
    return b[: (n + 7) // 8], n


def edge_list():
    tiny, sub_max, flt_min, flt_max = 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF
    pos = [0x00000000, tiny, sub_max, flt_min, flt_max, 0x7F800000, 0x7FC00000, 0x7F800001, 0x7FFFFFFF]
    bits = pos + [b | 0x80000000 for b in pos]
    vals = [2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 26, 2.0 ** 26 - 4, 99999999.0, 100000000.0, 2.0 ** 32, 2.0 ** 40, 2.0 ** 41, 2.0 ** 63, 2.0 ** 64, 2.0 ** 96,
            2.0 ** 127, 1e8, 1e9, 1e16, 1e17, 1e24, 1e32, 1e38, 9.995, 0.9999995, 99999.996, 9.5, 99.5, 0.95, 0.995, 0.9995, 0.99995, 0.999995, 0.9999999,
            9.9999999, 999.9995, 0.5, 1.5, 2.5, 0.05, 0.005, 0.0005, 0.00005, 0.000005, 0.0000005, 0.00000049, 0.001, 0.004, 0.006, 0.049, 0.051, 0.4, 0.6,
            1e-7, 1e-10, 1e-20, 1e-38, 1.0, 10.0, 12.34, 7405.3003, 0.125, 0.375, 16777215.0, 8388607.5, 4194303.75, 0.1, 0.2, 0.3, 123456.789, 1e-3]
    bits += [int(b) for b in f32(vals)] + [int(b) | 0x80000000 for b in f32(vals)]
    return np.array(bits, dtype=np.uint32)


def binades(rng):
    bits = []
    for E in range(1, 255):
        for M in (0, 1, 0x7FFFFF, int(rng.integers(0, 1 << 23))):
            bits += [(E << 23) | M, 0x80000000 | (E << 23) | M]
    return np.array(bits, dtype=np.uint32)


def ties(d):
    """exact ties at d decimals: j / 2^(d+1), j odd -- next to even and odd last digits and, at d = 0, to carries"""
    js = list(range(1, 200, 2)) + [2 ** (d + 1) * k + 2 ** d for k in (9, 99, 999, 4999, 8388607 >> (d + 1))]
    vals = [j / 2.0 ** (d + 1) for j in js]
    assert all(float(np.float32(v)) == v for v in vals)
    b = f32(vals)
    return np.concatenate([b, b | np.uint32(0x80000000)])


def meter(rng, T, Cn, top=5000.0):
    return (np.round(rng.uniform(0.0, top, (T, Cn)) * 100.0) / 100.0).astype(np.float32)


def rows_of(items, dtype):
    out = np.zeros((len(items), max(1, max(len(s) for s in items))), dtype=dtype)
    for c, s in enumerate(items):
        out[c, : len(s)] = np.frombuffer(s, dtype=np.uint8)
    return out


def main():
    assert orc.have_ref(), "oracle/_ref/libdcref.so is not built (make -C oracle)"
    rng = np.random.default_rng(20153)
    lists = {"edge": edge_list(), "binades": binades(rng)}
    for d in DECIMALS:
        lists["ties_d%d" % d] = ties(d)
    out = {}
    stored = nan_signed = trunc_differs = half_up_differs = left_out = 0

    def add(name, bits, options_of, prefix):
        nonlocal stored, nan_signed, trunc_differs, half_up_differs, left_out
        out[name + ".bits"] = bits
        for d in DECIMALS:
            want = [py_line(int(b), d, prefix) for b in bits]
            keep = np.array([len(s) - len(prefix) < LINE_LIMIT for s in want])  # what sprintf writes, '\n' included, plus its '\0' must fit
            left_out += int((~keep).sum())
            text = ref_text(bits[keep], options_of(d))
            lines = text.split(b"\n")
            assert lines[-1] == b"" and len(lines) - 1 == int(keep.sum()), (name, d)
            for b, w, got in zip(bits[keep], [w for w, k in zip(want, keep) if k], lines):
                got = got + b"\n"
                x = as_float(b)
                if np.isnan(x) and b >> 31:
                    assert got == prefix.encode() + b"-nan\n" and ("%.*f" % (d, float(x))) == "nan"
                    nan_signed += 1
                assert got == w.encode(), (name, d, hex(b), got, w)
                trunc_differs += got != (prefix + other_rounding(int(b), d, ROUND_DOWN)).encode()
                half_up_differs += got != (prefix + other_rounding(int(b), d, ROUND_HALF_UP)).encode()
                stored += 1
            out["%s.d%d.keep" % (name, d)] = keep
            out["%s.d%d.text" % (name, d)] = np.frombuffer(text, dtype=np.uint8)

    for name, bits in lists.items():
        add(name, bits, lambda d: "num_decimal_places=%d" % d, "")
    add("col3", lists["edge"], lambda d: "num_decimal_places=%d column=3 separator_char=;" % d, ";;")
    assert nan_signed > 0 and trunc_differs > 0 and half_up_differs > 0 and left_out > 0, (nan_signed, trunc_differs, half_up_differs, left_out)

    # chains: meter-like channels, their sums, and LZMH behind the text
    v = meter(rng, 420, 6)
    v[0, 0] = -0.0
    v[:, 5] = meter(rng, 420, 1, top=40.0)[:, 0]
    out["meter.v"] = v

    def chain(key, series, front):
        texts, streams, bits = [], [], []
        for c in range(series.shape[1]):
            t, n = ref_chain(series[:, c], front + ["encode csv num_decimal_places=2"])
            assert n % 8 == 0
            s, b = ref_chain(series[:, c], front + ["encode csv num_decimal_places=2", "encode lzmh"])
            texts.append(t)
            streams.append(s)
            bits.append(b)
        out[key + ".text"], out[key + ".text_len"] = rows_of(texts, np.uint8), np.array([len(t) for t in texts], dtype=np.int64)
        out[key + ".stream"], out[key + ".bits"] = rows_of(streams, np.uint8), np.array(bits, dtype=np.uint64)
        return texts

    assert chain("meter.plain", v, [])[0].startswith(b"-0.00\n")
    for N in (1, 7, 60):
        texts = chain("meter.N%d" % N, v, ["encode aggregate num_values=%d" % N])
        if N == 1:
            assert texts[0].startswith(b"0.00\n")  # +0.0f + -0.0f

    with gzip.open(os.path.join(HERE, "input.txt.gz"), "rb") as f:
        input_txt = f.read()
    series = np.array(input_txt.split(), dtype=np.float64).astype(np.float32).reshape(-1, 1)
    t, n = ref_chain(series[:, 0], ["encode csv num_decimal_places=2"])
    assert t == input_txt, "`decode csv # encode csv` does not give input.txt again"
    chain("series.N60", series, ["encode aggregate num_values=60"])

    path = os.path.join(HERE, "csv.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes; %d lines stored (%d left out as too long), %d -nan; truncation differs on %d, round-half-up on %d; series N=60: %d bits"
          % (path, len(out), os.path.getsize(path), stored, left_out, nan_signed, trunc_differs, half_up_differs, int(out["series.N60.bits"][0])))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "aggregate_levels.npz"))


if __name__ == "__main__":
    main()
