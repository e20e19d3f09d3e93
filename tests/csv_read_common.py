"""Shared by tests/test_csv_read_host.py, tests/test_gpu_csv_read.py and tests/golden/make_golden_csv_read.py: libc's strtof
through ctypes (what the reference calls, csv.c:32), the control flow of ReadCSV (csv.c:20-42) restated for one text,
tests/golden/csv_read.npz (what the compiled reference's `decode csv` returned), the layout of a batch of texts, and the
classes of random fields.  Every comparison is exact bit patterns and exact counts."""
import ctypes as C
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERROR_INVALID_VALUE, ERROR_INVALID_FORMAT, ERROR_MEMORY = -1, -3, -6
FIELD_LIMIT = 48  # the reference's buffer (csv.c:11,18): a selected field of this many characters overruns it

_libc = C.CDLL("libc.so.6")
_libc.strtof.restype = C.c_float
_libc.strtof.argtypes = [C.c_char_p, C.c_void_p]


def strtof_bits(field):
    """the bit pattern of strtof(field) in the C locale (pytest never calls setlocale)"""
    f = C.c_float(_libc.strtof(bytes(field), None))
    return C.cast(C.byref(f), C.POINTER(C.c_uint32))[0]


def split(text, column=1, sep=","):
    """csv.c:20-42: the selected fields of one text, in order, as the reference hands them to strtof -- the last byte of the
    text appended to a selected field whatever it is.  Returns (fields, status): status is ERROR_INVALID_FORMAT, and the
    list ends, in front of the first field of 48 characters or more."""
    sep = ord(sep) if isinstance(sep, (str, bytes)) else int(sep)
    fields, col, buf, n = [], 1, bytearray(), len(text)
    for i, ch in enumerate(bytes(text)):
        last = i == n - 1
        if ch == sep or ch == 10 or last:
            if last and col == column:
                buf.append(ch)
            if col == column:
                if len(buf) >= FIELD_LIMIT:
                    return fields, ERROR_INVALID_FORMAT
                fields.append(bytes(buf))
                buf.clear()
            col += 1
        elif col == column:
            buf.append(ch)
        if ch == 10:
            col = 1
    return fields, 0


def expected(text, column=1, sep=","):
    """(bit patterns uint32 [n], status) of one text: split() and libc's strtof"""
    fields, status = split(text, column, sep)
    return np.array([strtof_bits(f) for f in fields], dtype=np.uint32), status


def lines_text(fields):
    """one field per line, column 1; the last line's newline is appended to its field (csv.c:25-26), which strtof ignores"""
    return b"".join(f + b"\n" for f in fields)


def short_one_last(fields):
    """the same fields with one of at most 46 characters at the end, so that the newline appended to the last field of a
    text (csv.c:25-26) does not make it 48: a field of 47 characters at the end changes places with the nearest shorter one"""
    fields = list(fields)
    if fields and len(fields[-1]) > FIELD_LIMIT - 2:
        shorter = [i for i, f in enumerate(fields) if len(f) <= FIELD_LIMIT - 2]
        assert shorter, "every field has 47 characters: none can end the text"
        k = shorter[-1]
        fields[k], fields[-1] = fields[-1], fields[k]
    return fields


def pack(texts, stride=None, fill=0x5A):
    """texts of a batch as uint8 [C][stride] (16-byte aligned, stride a multiple of 16) and their lengths; bytes beyond a text
    hold `fill`, which no value may show"""
    longest = max([len(t) for t in texts] + [1])
    if stride is None:
        stride = (longest + 15) // 16 * 16
    raw = np.full(len(texts) * stride + 16, fill, dtype=np.uint8)
    at = (-raw.ctypes.data) % 16
    rows = raw[at: at + len(texts) * stride].reshape(len(texts), stride)
    lens = np.zeros(len(texts), dtype=np.uint64)
    for c, t in enumerate(texts):
        rows[c, : len(t)] = np.frombuffer(t, dtype=np.uint8)
        lens[c] = len(t)
    return rows, lens


def deal(fields, Cn):
    """fields dealt to Cn channels in turn (channel c gets fields c, c + Cn, ...; a field of 47 characters that would end its
    channel changes places with an earlier one of the channel): (texts, expected bit patterns per channel)."""
    texts, want = [], []
    for c in range(Cn):
        mine = short_one_last(fields[c::Cn])
        assert all(len(f) < FIELD_LIMIT for f in mine) and (not mine or len(mine[-1]) <= FIELD_LIMIT - 2)
        texts.append(lines_text(mine))
        want.append(np.array([strtof_bits(f) for f in mine], dtype=np.uint32))
    return texts, want


def check_channels(got, count, err, want, status, max_T, what):
    """got: uint32 [max_T][ld].  Exact counts, exact status, exact bit patterns of the rows a channel has.  `status`: per
    channel the expected code apart from ERROR_MEMORY, which follows from max_T.  Returns the number of values compared."""
    n = 0
    for c, w in enumerate(want):
        code = status[c] if status[c] != 0 else (ERROR_MEMORY if len(w) > max_T else 0)
        assert int(err[c]) == code and int(count[c]) == len(w), (what, c, int(err[c]), code, int(count[c]), len(w))
        k = min(len(w), max_T)
        bad = np.nonzero(got[:k, c] != w[:k])[0]
        assert bad.size == 0, (what, c, int(bad[0]), hex(int(got[bad[0], c])), hex(int(w[bad[0]])))
        n += k
    return n


# ---- the fixture -------------------------------------------------------------------------------------------------------------

class ReadFixture:
    """csv_read.npz: per case `name` the text (<name>.text, or taken from csv.npz / input.txt.gz for the cases that read the
    writer's fixture back), its options (<name>.opt = [column, separator_char]) and the floats the reference returned
    (<name>.bits, or <name>.xor: see bits())."""

    def __init__(self):
        self.z = np.load(os.path.join(GOLDEN, "csv_read.npz"))
        self.w = np.load(os.path.join(GOLDEN, "csv.npz"))

    def cases(self):
        return sorted(k[: -len(".opt")] for k in self.z.files if k.endswith(".opt"))

    def text(self, name):
        if name + ".text" in self.z.files:
            return self.z[name + ".text"].tobytes()
        if name == "input":
            from csv_common import input_txt
            return input_txt()
        assert name.startswith("back."), name
        key = name[len("back."):]
        if key.startswith(("meter.", "series.")):  # back.<chain>.c<channel>
            key, c = key.rsplit(".c", 1)
            return self.w[key + ".text"][int(c), : int(self.w[key + ".text_len"][int(c)])].tobytes()
        return self.w[key + ".text"].tobytes()

    def options(self, name):
        column, sep = self.z[name + ".opt"]
        return int(column), int(sep)

    def bits(self, name):
        """the floats the reference returned.  The cases that read the writer's fixture back have many lines: they are stored
        as the difference (xor) to float32(float(field)), which is zero nearly everywhere and compresses to little."""
        if name + ".bits" in self.z.files:
            return self.z[name + ".bits"]
        column, sep = self.options(name)
        return self.z[name + ".xor"] ^ predicted(split(self.text(name), column, sep)[0])


# ---- classes of random fields (each a list of bytes of at most 47 characters; deal() keeps the longest from ending a text) --------------------------

def fields_printed(rng, n, d):
    """"%.*f" of random bit patterns, as `encode csv` writes them (nan / -nan / inf included)"""
    out = []
    while len(out) < n:
        bits = rng.integers(0, 2 ** 32, 2 * (n - len(out)) + 16, dtype=np.uint64).astype(np.uint32)
        with np.errstate(invalid="ignore"):
            vals = bits.view(np.float32).astype(np.float64).tolist()
        for x, neg in zip(vals, (bits >> 31).tolist()):
            s = ("-nan" if neg else "nan") if x != x else "%.*f" % (d, x)
            if len(s) < FIELD_LIMIT and len(out) < n:
                out.append(s.encode())
    return out


def _digits(rng, n):
    return "".join(map(str, rng.integers(0, 10, n).tolist()))


def fields_digits(rng, n, tail=lambda rng: ""):
    """random digit strings of 1 .. 47 characters with a point anywhere (or none), a third of them negative"""
    out = []
    for _ in range(n):
        t = tail(rng)
        k = int(rng.integers(1, FIELD_LIMIT - len(t)))  # 1 .. 47 characters with the tail
        s = _digits(rng, k)
        if k > 1 and rng.random() < 0.9:
            p = int(rng.integers(0, k))
            s = s[:p] + "." + s[p + 1:]
        if rng.random() < 0.33 and len(s) + len(t) < FIELD_LIMIT - 1:
            s = "-" + s
        out.append((s + t).encode())
    return out


def _exponent(rng):
    r = rng.random()
    e = int(rng.integers(-60, 51)) if r < 0.5 else (int(rng.integers(-99, 100)) if r < 0.8 else int(rng.integers(-400, 400)))
    return ("e%+d" if rng.random() < 0.6 else "E%d") % e


def fields_exponents(rng, n):
    return fields_digits(rng, n, _exponent)


def fields_hex(rng, n):
    out = []
    for _ in range(n):
        r = rng.random()
        p = "" if r < 0.2 else ("p%+d" % int(rng.integers(-200, 200)) if r < 0.7 else "P-%d" % int(rng.integers(100, 320)))
        k = int(rng.integers(1, FIELD_LIMIT - 3 - len(p)))  # up to 47 characters with sign, 0x and exponent
        s = "".join("0123456789abcdefABCDEF"[i] for i in rng.integers(0, 22, k).tolist())
        if k > 1 and rng.random() < 0.7:
            q = int(rng.integers(0, k))
            s = s[:q] + "." + s[q + 1:]
        out.append((("-" if rng.random() < 0.25 else "") + ("0x" if rng.random() < 0.8 else "0X") + s + p).encode())
    return out


def midpoint(m, e):
    """the exact decimal expansion of (2m + 1) / 2 x 2^e, e <= 0: halfway between the floats m x 2^e and (m + 1) x 2^e"""
    k = 1 - e
    digits = str((2 * m + 1) * 5 ** k)
    return (digits[:-k] if len(digits) > k else "0") + "." + digits[-k:].rjust(k, "0")


def fields_midpoints(rng, n, exponents=(-30, -24, -20, -10, 0)):
    """exact midpoints between neighbouring floats, and the same with the last digit one up and one down"""
    out = []
    while len(out) < n:
        s = midpoint(int(rng.integers(2 ** 23, 2 ** 24)), int(exponents[int(rng.integers(0, len(exponents)))]))
        assert len(s) <= FIELD_LIMIT - 2
        last = int(s[-1])  # (5: a midpoint's expansion ends in it)
        out += [s.encode(), (s[:-1] + str(last + 1)).encode(), (s[:-1] + str(last - 1)).encode()]
    return out[:n]


def float32_via_double(field):
    """double rounding: what a conversion through double gives"""
    with np.errstate(over="ignore"):
        return int(np.array([float(field)], dtype=np.float64).astype(np.float32).view(np.uint32)[0])


def predicted(fields):
    """float32(float(field)) per field, 0 where Python reads no number: what the `.xor` arrays of csv_read.npz are relative to"""
    out = np.zeros(len(fields), dtype=np.uint32)
    for i, f in enumerate(fields):
        try:
            out[i] = float32_via_double(f)
        except ValueError:
            pass
    return out


def truncated_19(field):
    """the field with its significant digits beyond the 19th replaced by zeros (plain decimal fields only)"""
    out, seen = [], 0
    for ch in field.decode():
        if ch.isdigit() and (seen or ch != "0"):
            seen += 1
            out.append(ch if seen <= 19 else "0")
        else:
            out.append(ch)
    return "".join(out).encode()
