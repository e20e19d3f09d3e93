"""python tools/host_forms_bench.py LABEL [LIB]: wall time of each synchronous host form (dega_hip_aggregate_host,
dega_hip_csv_write_host, dega_hip_csv_read_host, dega_hip_lzmh_encode_host, dega_hip_lzmh_decode_host) at one single-chunk
shape from pageable memory: a warm-up call and RUNS timed calls each (host clock around the call; every form ends in a
device synchronise), and a digest of every result.  LIB: another build of libdega_hip.so to time instead of the tree's,
e.g. the parent commit's (profiles/host_forms_parent_vs_change.txt).  Every line starts with LABEL."""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

RUNS = 6
label = sys.argv[1]
dca = load_package()
if len(sys.argv) > 2:
    dca.LIB_PATH = os.path.abspath(sys.argv[2])
L = dca.library()
ctx = dca.Context(0)
assert "DEGA_HOST_CHUNK_BYTES" not in os.environ


def say(s):
    print(s, flush=True)


def timed(name, shape, mb, call, digest):
    ret = call()
    assert ret == 0, (name, ret, ctx.last_error())
    ms = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        ret = call()
        ms.append((time.perf_counter() - t0) * 1e3)
        assert ret == 0
    s = sorted(ms)
    say("%-6s %-26s %s, %d MB through the link: median %.2f ms, fastest %.2f, slowest %.2f | runs %s | digest %s"
        % (label, name, shape, mb, (s[RUNS // 2 - 1] + s[RUNS // 2]) / 2, s[0], s[-1], " ".join("%.2f" % m for m in ms), digest()))


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def upto(rows, lens):
    """rows with everything at and beyond lens[c] cleared"""
    out = rows.copy()
    out[np.arange(rows.shape[1])[None, :] >= lens[:, None].astype(np.int64)] = 0
    return out


rng = np.random.default_rng(1)
Cn = 16384

# aggregate: 16384 channels x 4096 readings, num_values 4
T, N = 4096, 4
v = (np.round(rng.uniform(0, 5000, (T, Cn)) * 100) / 100).astype(np.float32)
a = np.zeros((T // N, Cn), dtype=np.float32)
timed("dega_hip_aggregate_host", "%d x %d float32, num_values %d" % (Cn, T, N), (v.nbytes + a.nbytes) >> 20,
      lambda: L.dega_hip_aggregate_host(ctx._h, v.ctypes.data, Cn, T, Cn, N, a.ctypes.data, Cn), lambda: sha(a))

# csv write: 16384 channels x 512 readings, two decimals, worst-case rows
Tw = 512
stride = dca.csv_worst_case_bytes(Tw, 2, 1)
text, lens, err = np.zeros((Cn, stride), dtype=np.uint8), np.zeros(Cn, dtype=np.uint64), np.zeros(Cn, dtype=np.int32)
vw = v[:Tw].copy()
timed("dega_hip_csv_write_host", "%d x %d float32, stride %d" % (Cn, Tw, stride), (vw.nbytes + text.nbytes) >> 20,
      lambda: L.dega_hip_csv_write_host(ctx._h, vw.ctypes.data, Cn, Tw, Cn, 2, 1, 44, text.ctypes.data, stride, lens.ctypes.data, err.ctypes.data),
      lambda: sha(lens, err, upto(text, lens)))
assert (err == 0).all()

del text

# csv read: the text of 2048 readings per channel (written here, untimed) back, rows of 16400 bytes
Tr = 2048
rstride = Tr * 8 + 16
vr = np.ascontiguousarray(v[:Tr])
rtext, rlen, werr = np.zeros((Cn, rstride), dtype=np.uint8), np.zeros(Cn, dtype=np.uint64), np.zeros(Cn, dtype=np.int32)
assert L.dega_hip_csv_write_host(ctx._h, vr.ctypes.data, Cn, Tr, Cn, 2, 1, 44, rtext.ctypes.data, rstride, rlen.ctypes.data, werr.ctypes.data) == 0
assert (werr == 0).all()
back, count, rerr = np.zeros((Tr, Cn), dtype=np.float32), np.zeros(Cn, dtype=np.uint64), np.zeros(Cn, dtype=np.int32)
timed("dega_hip_csv_read_host", "%d texts, stride %d, max_T %d" % (Cn, rstride, Tr), (rtext.nbytes + back.nbytes) >> 20,
      lambda: L.dega_hip_csv_read_host(ctx._h, rtext.ctypes.data, rstride, rlen.ctypes.data, Cn, 1, 44, back.ctypes.data, Tr, Cn, count.ctypes.data,
                                       rerr.ctypes.data), lambda: sha(back, count, rerr))
assert (rerr == 0).all() and (count == Tr).all() and (back.view(np.uint32) == vr.view(np.uint32)).all()
del rtext, back

# LZMH encode: 16384 texts of 16384 bytes (meter lines), worst-case slabs
ls = 16384
lines = (np.round(230 + np.cumsum(rng.normal(0, 0.3, (64, 2400)), axis=1), 2))
base = np.zeros((64, ls), dtype=np.uint8)
for r in range(64):
    t = "".join("%.2f\n" % x for x in lines[r]).encode()[:ls]
    assert len(t) == ls
    base[r] = np.frombuffer(t, dtype=np.uint8)
ltext = np.ascontiguousarray(np.tile(base, (Cn // 64, 1)))
llen = np.full(Cn, ls, dtype=np.uint64)
cap = dca.lzmh_worst_case_bytes(ls)
slabs, bits, lerr = np.zeros((Cn, cap), dtype=np.uint8), np.zeros(Cn, dtype=np.uint64), np.zeros(Cn, dtype=np.int32)
timed("dega_hip_lzmh_encode_host", "%d texts of %d bytes, cap %d" % (Cn, ls, cap), ltext.nbytes >> 20,
      lambda: L.dega_hip_lzmh_encode_host(ctx._h, ltext.ctypes.data, ls, llen.ctypes.data, Cn, slabs.ctypes.data, cap, bits.ctypes.data, lerr.ctypes.data),
      lambda: sha(bits, lerr, upto(slabs, (bits + 7) // 8)))
assert (lerr == 0).all()
say("%-6s   (lzmh encode: %d MB of text up, the slabs' first %d bytes each down)" % (label, ltext.nbytes >> 20, (int(((bits + 7) // 8).max()) + 15) // 16 * 16))

# LZMH decode: those slabs back
dstride = ls + 8
dout, dlen, derr = np.zeros((Cn, dstride), dtype=np.uint8), np.zeros(Cn, dtype=np.uint64), np.zeros(Cn, dtype=np.int32)
timed("dega_hip_lzmh_decode_host", "%d slabs of %d bytes, stride %d" % (Cn, cap, dstride), (slabs.nbytes + dout.nbytes) >> 20,
      lambda: L.dega_hip_lzmh_decode_host(ctx._h, slabs.ctypes.data, cap, bits.ctypes.data, Cn, dout.ctypes.data, dstride, dlen.ctypes.data, derr.ctypes.data),
      lambda: sha(dlen, derr, upto(dout, dlen)))
assert (derr == 0).all() and (dlen == ls).all() and (dout[:, :ls] == ltext).all()
ctx.close()
