"""Index width without a GPU: the cases of tests/index_width_common.py -- every kernel family where t * ld, c * stride and
c * cap pass 2^31 bytes, 2^32 bytes and 2^32 elements, each held exactly to its reference -- on the shipped kernel source
and launch code compiled by g++ under the thread-per-lane emulator of tests/sim/.  The images are numpy.empty arrays of
up to 18.8 GB of which only the pages of the logical regions are ever touched (the model is
tests/test_gpu_channel_major.py::test_offsets_are_64_bit; tests/test_gpu_index_width.py runs the same cases through the C
ABI).  A 32-bit product here reads or writes another row of the same image, or -- sign-extended -- memory below it, which
on the CPU is a mismatch or a segmentation fault and nothing worse: these cases pass before the GPU file is run.

The split reader sweeps its whole stride in blocks (a lane per block, whatever the text's length), so under the emulator,
which starts a thread per lane, its block is 2^20 bytes: every text lies in its channel's first block, and c * stride
and row * ld still cross the lines.  The GPU file splits the same texts into blocks of 1 KiB.  (c * blocks + b stays far
below 2^31 in both, 6 x 1 024 and 6 x 2^20 pairs: only a batch of some million channels would take it there.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import index_width_common as iw  # noqa: E402
from sim_build import sim_library  # noqa: E402

P, Z, I, U, F = C.c_void_p, C.c_size_t, C.c_int, C.c_uint, C.c_float

SIGNATURES = {
    "aggregate": {"sim_aggregate": [P, Z, Z, Z, Z, P, Z, I, Z]},
    "aggregate_levels": {"sim_aggregate_levels": [P, Z, Z, Z, P, Z, P, P, I, Z]},
    "ragged": {"sim_aggregate_var": [P, Z, Z, Z, P, P, Z, P, P, P, P, I, Z], "sim_csv_var": [P, Z, Z, Z, P, U, Z, I, P, Z, P, P, I]},
    "ragged_int": {"sim_encode_int_var": [P, Z, Z, Z, P, I, I, I, I, P, Z, P, P]},
    "csv": {"sim_csv": [P, Z, Z, Z, U, Z, I, P, Z, P, P, I]},
    "csv_write_split": {"sim_csv_write_split": [P, Z, Z, Z, P, U, Z, I, P, Z, P, P, Z]},
    "csv_read": {"sim_csv_read": [P, Z, P, Z, Z, I, P, Z, Z, P, P]},
    "csv_read_split": {"sim_csv_read_split": [P, Z, P, Z, Z, I, P, Z, Z, P, P, Z]},
    "dega": {"sim_encode_vs": [P, Z, Z, Z, I, I, P, Z, P, P], "sim_decode_var_vs": [P, Z, P, Z, Z, Z, I, I, P, P, P],
             "sim_encode64": [P, Z, Z, Z, I, I, P, Z, P, P], "sim_decode64": [P, Z, P, Z, Z, Z, I, I, P, P, P],
             "sim_encode_segments": [P, Z, Z, Z, I, F, I, I, P, I, P, Z, P, P], "sim_encode_f32": [P, Z, Z, Z, F, I, I, P, Z, P, P],
             "sim_decode_f32": [P, Z, P, Z, Z, Z, F, I, I, P, P, P], "sim_normalize_vs": [P, Z, Z, Z, F, I, P, P],
             "sim_denormalize_vs": [P, Z, Z, Z, F, I, P], "sim_lzmh_encode": [P, Z, P, Z, P, Z, P, P], "sim_lzmh_decode": [P, Z, P, Z, P, Z, P, P],
             "sim_lzmh_render": [P, Z, Z, Z, P, Z, P, P]},
    "compact": {"sim_compact": [P, Z, P, Z, P, I]},  # (tests/sim/sim_compact.cpp: the compaction kernels had no driver)
}


class Emulator:
    """the backend of index_width_common over tests/sim/: numpy arrays, the emulator's entry points"""
    split_block_bytes = 1 << 20

    def __init__(self):
        self.lib, self.kept = {}, []
        for name, table in SIGNATURES.items():
            L = sim_library(name)
            for fn, sig in table.items():
                getattr(L, fn).argtypes = sig
                getattr(L, fn).restype = C.c_int
                self.lib[fn] = getattr(L, fn)
        self.images = {name: np.empty(size, dtype=np.uint8) for name, size in iw.IMAGES.items()}  # (sparse: only touched pages are committed)

    def close(self):
        self.images.clear()

    def call(self, fn, *args):
        assert self.lib[fn](*args) == 0, fn

    # ---- memory ----
    def view(self, name, dtype, pitch):
        a = self.images[name].view(dtype).reshape(-1, pitch)
        return iw.View(a, dtype, a.ctypes.data)

    def put(self, a, r0, c0, block):
        assert block.dtype.itemsize == a.array.dtype.itemsize
        a.array[r0:r0 + block.shape[0], c0:c0 + block.shape[1]] = block.view(a.array.dtype)

    def get(self, a, r0, r1, c0, c1):
        return a.array[r0:r1, c0:c1].copy()

    def dev(self, x):
        self.kept.append(np.ascontiguousarray(x).copy())  # (alive until forget(): the cases pass addresses on)
        return self.kept[-1]

    def forget(self):
        self.kept.clear()

    def host(self, d):
        return d

    def ptr(self, d):
        return d.address if isinstance(d, iw.View) else d.ctypes.data

    @staticmethod
    def array(values, ctype):
        return (ctype * len(values))(*values)

    # ---- the entry points (arguments as the C ABI's) ----
    def aggregate(self, v, Cn, T, ld, N, a, ld_out, ranges=None):
        self.call("sim_aggregate", v, Cn, T, ld, N, a, ld_out, int(Cn % 4 == 0), ranges or T)  # (the library: a range per output row at these shapes)

    def aggregate_levels(self, v, Cn, T, ld, levels, a, ld_out):
        K = len(levels)
        self.call("sim_aggregate_levels", v, Cn, T, ld, self.array(levels, Z), K, self.array(a, P), self.array(ld_out, Z), int(Cn % 4 == 0), T)

    def aggregate_levels_var(self, v, Cn, T, ld, count, levels, a, ld_out, out_count, err):
        K = len(levels)
        self.call("sim_aggregate_var", v, Cn, T, ld, count, self.array(levels, Z), K, self.array(a, P), self.array(ld_out, Z), self.array(out_count, P), err,
                  int(Cn % 4 == 0), T)

    def encode(self, x, Cn, T, ld, ad, vs, out, cap, bits, err):
        self.call("sim_encode_vs", x, Cn, T, ld, ad, vs, out, cap, bits, err)

    def encode64(self, x, Cn, T, ld, ad, vs, out, cap, bits, err):
        self.call("sim_encode64", x, Cn, T, ld, ad, vs, out, cap, bits, err)

    def encode_var(self, x, Cn, T, ld, count, ad, vs, out, cap, bits, err):
        self.call("sim_encode_int_var", x, Cn, T, ld, count, 0, 0, ad, vs, out, cap, bits, err)

    def encode_segments(self, x, Cn, T, ld, ad, vs, cuts, out, cap, bits, err):
        self.call("sim_encode_segments", x, Cn, T, ld, 0, 0.0, ad, vs, self.array(cuts, Z), len(cuts), out, cap, bits, err)

    def decode(self, s, cap, bits, Cn, T, ld, ad, vs, x, err):
        self.call("sim_decode_var_vs", s, cap, bits, Cn, T, ld, ad, vs, x, None, err)

    def decode_var(self, s, cap, bits, Cn, T, ld, ad, vs, x, counts, err):
        self.call("sim_decode_var_vs", s, cap, bits, Cn, T, ld, ad, vs, x, counts, err)

    def decode64(self, s, cap, bits, Cn, T, ld, ad, vs, x, err):
        self.call("sim_decode64", s, cap, bits, Cn, T, ld, ad, vs, x, None, err)

    def encode_f32(self, v, Cn, T, ld, factor, ad, vs, out, cap, bits, err):
        self.call("sim_encode_f32", v, Cn, T, ld, factor, ad, vs, out, cap, bits, err)

    def encode_agg_f32(self, v, Cn, T, ld, N, factor, ad, vs, out, cap, bits, err):
        """the library's two launches: the sums into a scratch of the natural pitch, then the float entry over them"""
        T_out = (T + N - 1) // N
        sums = np.empty((T_out, Cn), dtype=np.float32)
        self.aggregate(v, Cn, T, ld, N, sums.ctypes.data, Cn)
        self.encode_f32(sums.ctypes.data, Cn, T_out, Cn, factor, ad, vs, out, cap, bits, err)

    def decode_f32(self, s, cap, bits, Cn, T, ld, factor, ad, vs, v, counts, err):
        self.call("sim_decode_f32", s, cap, bits, Cn, T, ld, factor, ad, vs, v, counts or None, err)

    def normalize(self, v, Cn, T, ld, factor, vs, x, err):
        self.call("sim_normalize_vs", v, Cn, T, ld, factor, vs, x, err)

    def denormalize(self, x, Cn, T, ld, factor, vs, v):
        self.call("sim_denormalize_vs", x, Cn, T, ld, factor, vs, v)

    def csv_write(self, v, Cn, T, ld, d, column, sep, out, stride, lens, err, form):
        self.call("sim_csv", v, Cn, T, ld, d, column, sep, out, stride, lens, err, int(form == "store64"))

    def csv_write_var(self, v, Cn, T, ld, count, d, column, sep, out, stride, lens, err, form):
        self.call("sim_csv_var", v, Cn, T, ld, count, d, column, sep, out, stride, lens, err, int(form == "store64"))

    def csv_write_split(self, v, Cn, T, ld, count, d, column, sep, out, stride, lens, err, block_rows):
        self.call("sim_csv_write_split", v, Cn, T, ld, count or None, d, column, sep, out, stride, lens, err, block_rows)

    def csv_read(self, text, stride, lens, Cn, column, sep, v, max_T, ld, count, err):
        self.call("sim_csv_read", text, stride, lens, Cn, column, sep, v, max_T, ld, count, err)

    def csv_read_split(self, text, stride, lens, Cn, column, sep, v, max_T, ld, count, err, block_bytes):
        self.call("sim_csv_read_split", text, stride, lens, Cn, column, sep, v, max_T, ld, count, err, block_bytes)

    def lzmh_encode(self, text, stride, lens, Cn, out, cap, bits, err):
        self.call("sim_lzmh_encode", text, stride, lens, Cn, out, cap, bits, err)

    def lzmh_decode(self, s, cap, bits, Cn, out, stride, lens, err):
        self.call("sim_lzmh_decode", s, cap, bits, Cn, out, stride, lens, err)

    def lzmh_render(self, x, Cn, T, ld, out, stride, lens, err):
        self.call("sim_lzmh_render", x, Cn, T, ld, out, stride, lens, err)

    def compact(self, slabs, cap, offsets, Cn, packed, scatter):
        self.call("sim_compact", slabs, cap, offsets, Cn, packed, int(scatter))


@pytest.fixture(scope="module")
def B():
    try:
        b = Emulator()
    except MemoryError:
        pytest.skip("numpy.empty refuses the sparse images on this machine")
    yield b
    b.close()


def test_the_images_put_rows_on_both_sides_of_every_line():
    """the geometry the cases lean on, from the shapes alone"""
    assert 8 * 4 * iw.PITCH4["BIG"] == iw.LINE31 and 16 * 4 * iw.PITCH4["BIG"] == iw.LINE32 and 64 * iw.PITCH4["BIG"] == iw.LINE32
    assert 32 * 4 * iw.PITCH4["MID"] == iw.LINE31 and 64 * 4 * iw.PITCH4["MID"] == iw.LINE32
    assert 2 * iw.STRIDE == iw.LINE31 and 4 * iw.STRIDE == iw.LINE32 and 4 * iw.CAP == iw.LINE31 and 8 * iw.CAP == iw.LINE32
    assert iw.T * 4 * iw.PITCH4["BIG"] == iw.IMAGES["BIG"] and iw.T * 4 * iw.PITCH4["MID"] == iw.IMAGES["MID"]
    assert 6 * iw.STRIDE == 12 * iw.CAP == iw.IMAGES["TEXT"] == iw.IMAGES["TEXT2"] and iw.T > 64
    with pytest.raises(AssertionError):
        iw.crossed(range(16), 4 * iw.PITCH4["BIG"])  # rows 0 .. 15 of BIG stay below 2^32 bytes: such a case would prove nothing
    with pytest.raises(AssertionError):
        iw.crossed(range(64), 4 * iw.PITCH4["BIG"], elem=4)
    names = [c[0] for c in iw.CASES + iw.HOST_ONLY + iw.GPU_ONLY]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("case", iw.CASES + iw.HOST_ONLY, ids=lambda c: c[0])
def test_offsets_are_64_bit_under_the_emulator(B, case):
    iw.run(B, case)
