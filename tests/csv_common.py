"""Shared by tests/test_csv_host.py and tests/test_gpu_csv.py: tests/golden/csv.npz (what the compiled reference's
`encode csv` wrote; tests/golden/make_golden_csv.py), Python's formatting with glibc's sign of NaN, and the arrangement
of a list of readings as a [T][C] batch with the text every channel must get."""
import gzip
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERROR_MEMORY = -6
SLACK = 16  # a channel fits when text + 16 bytes <= stride (include/dega_hip.h)
DECIMALS = tuple(range(7))


def py_lines(bits, d, column=1, sep=","):
    """one line per reading as sprintf("%.*f\\n") of glibc writes it behind column - 1 separators (csv.c:56-60)"""
    bits = np.ascontiguousarray(bits, dtype=np.uint32).ravel()
    with np.errstate(invalid="ignore"):  # (signalling NaNs among random bit patterns)
        vals = bits.view(np.float32).astype(np.float64).tolist()
    neg = (bits >> 31).tolist()
    prefix = sep * (column - 1)
    out = []
    for x, n in zip(vals, neg):
        s = ("-nan" if n else "nan") if x != x else "%.*f" % (d, x)  # Python prints nan whatever the sign bit says
        out.append((prefix + s + "\n").encode())
    return out


class Fixture:
    def __init__(self):
        self.z = np.load(os.path.join(GOLDEN, "csv.npz"))

    def lists(self):
        return sorted(k[: -len(".d0.keep")] for k in self.z.files if k.endswith(".d0.keep"))

    @staticmethod
    def options(name):
        return (3, ";") if name == "col3" else (1, ",")

    def lines(self, name, d):
        """(bit patterns the reference was given, the line it wrote for each)"""
        bits = self.z[name + ".bits"][self.z["%s.d%d.keep" % (name, d)]]
        lines = self.z["%s.d%d.text" % (name, d)].tobytes().split(b"\n")
        assert lines[-1] == b"" and len(lines) - 1 == bits.size
        return bits, [s + b"\n" for s in lines[:-1]]

    def left_out(self, name, d):
        return self.z[name + ".bits"][~self.z["%s.d%d.keep" % (name, d)]]

    def meter(self):
        return self.z["meter.v"]

    def chain(self, key):
        """(texts, streams, bits) per channel of `meter.plain`, `meter.N<N>` or `series.N60`"""
        text, tl = self.z[key + ".text"], self.z[key + ".text_len"]
        stream, bits = self.z[key + ".stream"], self.z[key + ".bits"]
        texts = [text[c, : int(tl[c])].tobytes() for c in range(tl.size)]
        streams = [stream[c, : (int(bits[c]) + 7) // 8].tobytes() for c in range(tl.size)]
        return texts, streams, [int(b) for b in bits]


def input_txt():
    with gzip.open(os.path.join(GOLDEN, "input.txt.gz"), "rb") as f:
        return f.read()


def input_series():
    return np.array(input_txt().split(), dtype=np.float64).astype(np.float32).reshape(-1, 1)


def arrange(bits, lines, Cn, ld, pad_line, filler=0x7FC12345):
    """n readings as a batch [T][ld] of bit patterns, reading i in row i // Cn, channel i % Cn; the rows' tail is +0.0f
    (whose line is pad_line), the columns beyond Cn hold `filler`, which no text may show.  Returns (batch, texts)."""
    n = len(lines)
    T = max(1, -(-n // Cn))
    batch = np.full((T, ld), filler, dtype=np.uint32)
    compact = np.zeros(T * Cn, dtype=np.uint32)
    compact[:n] = bits
    batch[:, :Cn] = compact.reshape(T, Cn)
    texts = []
    for c in range(Cn):
        mine = lines[c::Cn]
        texts.append(b"".join(mine) + pad_line * (T - len(mine)))
    return batch, texts


def check_channels(got_text, got_len, got_err, want, stride, what):
    """exact bytes and exact lengths for every channel that fits; ERROR_MEMORY and length 0 for every one that does not.
    Returns (channels that fit, channels that do not)."""
    fit = over = 0
    for c, w in enumerate(want):
        if len(w) + SLACK <= stride:
            assert int(got_err[c]) == 0 and int(got_len[c]) == len(w), (what, c, int(got_err[c]), int(got_len[c]), len(w))
            assert bytes(got_text[c][: len(w)]) == w, (what, c)
            fit += 1
        else:
            assert int(got_err[c]) == ERROR_MEMORY and int(got_len[c]) == 0, (what, c, int(got_err[c]), int(got_len[c]))
            over += 1
    return fit, over
