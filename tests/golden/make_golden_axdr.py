#!/usr/bin/env python3
"""Generates tests/golden/axdr.npz from the COMPILED REFERENCE LIBRARY in process (oracle/_ref/libdcref.so through
orc.ref_run_chain, as the other generators do).  Build container only:

    make -C oracle && python tests/golden/make_golden_axdr.py

A few channels per value size (tests/axdr_common.py: golden_input, seeded; the fixture stores a checksum of what the
reference was given) through `encode normalize` and back through `decode normalize`: the packed STREAM the reference
wrote, not only its values, pins the restatement's field order, bit order and padding.  Data only:
  n<vs>.in            uint32   crc32 of golden_input(vs)
  n<vs>.c<c>.stream   uint8    the stream of channel c, ceil(bits / 8) bytes
  n<vs>.c<c>.bits     uint64   its bit length
  n<vs>.c<c>.back     uint32   the float32 bit patterns `decode normalize` makes of it
The same run gives the same bytes.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import orc  # noqa: E402
import axdr_common as ax  # noqa: E402
import float_edges_common as fe  # noqa: E402


def main():
    assert orc.have_ref(), "oracle/_ref is not built: make -C oracle"
    arrays = {}
    for vs in ax.GOLDEN_SIZES:
        options = " normalization_factor=100.0 valuesize=%d" % vs
        v = ax.golden_input(vs)
        arrays["n%d.in" % vs] = fe.crc(v)
        for c in range(ax.GOLDEN_CHANNELS):
            col = np.ascontiguousarray(v[:, c])
            ret, data, n, _ = orc.ref_run_chain(col.tobytes(), 32 * col.size, ["encode normalize" + options])
            assert ret == 0 and n == vs * col.size, (vs, c, ret, n)
            ret, back, nb, _ = orc.ref_run_chain(data, n, ["decode normalize" + options])
            assert ret == 0 and nb == 32 * col.size, (vs, c, ret, nb)
            arrays["n%d.c%d.stream" % (vs, c)] = np.frombuffer(data[: (n + 7) // 8], dtype=np.uint8)
            arrays["n%d.c%d.bits" % (vs, c)] = np.uint64(n)
            arrays["n%d.c%d.back" % (vs, c)] = np.frombuffer(back[: nb // 8], dtype=np.uint32)
    fe.save_npz(ax.GOLDEN, arrays)
    print("wrote %s (%d bytes)" % (ax.GOLDEN, os.path.getsize(ax.GOLDEN)))


if __name__ == "__main__":
    main()
