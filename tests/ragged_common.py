"""Shared by tests/test_ragged_host.py and tests/test_gpu_ragged.py: tests/golden/ragged.npz (the compiled reference's
results per channel on that channel's own readings; tests/golden/make_golden_ragged.py) and the poison that marks what a
counted kernel must not look at."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = (1, 7, 60)
SETS = ((32, 1), (32, 0), (16, 1), (64, 1))  # (valuesize, adaptive)
FACTOR = 100.0
HONEST = 5  # the channel whose reading of 400.0, inside its count, leaves 16 bits
POISON = np.array([np.nan, np.inf, 3e38, -0.0], dtype=np.float32)
CASES = ("long", "short")


class Fixture:
    def __init__(self):
        self.path = os.path.join(ROOT, "tests", "golden", "ragged.npz")
        self.z = dict(np.load(self.path))

    def v(self, case):
        return self.z[case + ".v"]

    def count(self, case):
        return self.z[case + ".count"]

    def rows(self, case, N):
        return self.z["%s.N%d.rows" % (case, N)]

    def sums(self, case, N):
        return self.z["%s.N%d.sums" % (case, N)]

    def poisoned_sums(self, case, N):
        """the level's sums with poison in every row at or beyond a channel's row count: what a counted kernel behind the
        aggregate is given (the aggregate promises nothing there)"""
        return poisoned(self.sums(case, N), self.rows(case, N))

    def text(self, case, N):
        return self.z["%s.N%d.text" % (case, N)], self.z["%s.N%d.text_len" % (case, N)]

    def lzmh(self, case, N):
        return self.z["%s.N%d.lzmh" % (case, N)], self.z["%s.N%d.lzmh_bits" % (case, N)]

    def dega(self, case, N, vs, ad):
        k = "%s.N%d.vs%d.%s" % (case, N, vs, "ad" if ad else "st")
        return self.z[k + ".stream"], self.z[k + ".bits"], self.z[k + ".err"]


def poisoned(a, rows):
    a = np.array(a, dtype=np.float32, copy=True)
    for c in range(a.shape[1]):
        for t in range(int(rows[c]), a.shape[0]):
            a[t, c] = POISON[(t - int(rows[c])) % 4]
    return a


def same_rows(got, want, rows):
    """column c of got equals column c of want in its first rows[c] rows, bit for bit (a NaN only has to be a NaN)"""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    live = np.arange(want.shape[0])[:, None] < np.asarray(rows)[None, :]
    g, w = got[: want.shape[0], : want.shape[1]], want
    return bool((~live | (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))).all())


def untouched(got, rows, sentinel):
    """rows at or beyond a channel's count were left as they were"""
    dead = np.arange(got.shape[0])[:, None] >= np.asarray(rows)[None, :]
    return bool((~dead | (got[:, : len(rows)] == sentinel)).all())


def same_streams(out, bits, err, want_out, want_bits, want_err, channels=None):
    """per channel: the status, the exact bit length and the bytes of the stream"""
    n = len(want_bits) if channels is None else channels
    for c in range(n):
        if int(err[c]) != int(want_err[c]):
            return "channel %d: status %d, expected %d" % (c, err[c], want_err[c])
        if int(want_err[c]) != 0:
            continue
        if int(bits[c]) != int(want_bits[c]):
            return "channel %d: %d bits, expected %d" % (c, bits[c], want_bits[c])
        nb = (int(want_bits[c]) + 7) // 8
        if out[c, :nb].tobytes() != want_out[c, :nb].tobytes():
            return "channel %d: stream bytes differ" % c
    return ""


def same_texts(out, lens, want, want_len, channels=None):
    n = len(want_len) if channels is None else channels
    for c in range(n):
        if int(lens[c]) != int(want_len[c]):
            return "channel %d: %d bytes of text, expected %d" % (c, lens[c], want_len[c])
        if out[c, : int(lens[c])].tobytes() != want[c, : int(want_len[c])].tobytes():
            return "channel %d: text differs" % c
    return ""
