#!/usr/bin/env python3
"""Times the channel-major surface and writes profiles/layout_bench.txt.

    python tools/layoutbench.py [--channels 65536] [--samples 86400] [--runs 10] [--warmup 2] [--skip-host]

(a) dega_hip_to_time_major_dev / dega_hip_to_channel_major_dev on a resident batch of 4-byte elements, with and without
    counts, and one 8-byte case, against yardsticks measured IN THE SAME SESSION, run by run in turn with them: a float4
    copy of the same image (tools/layout_copy.hip, built into tools/liblayout_copy.so on first use: it reads and writes what
    the transposition reads and writes), torch's own device-to-device copy beside it, and dega_hip_aggregate_dev at N = 2
    (the streaming kernel DESIGN 4.5 quotes).  Fractions are of the float4 copy.  hipEvents on the launches' stream
    (torch.cuda.Event is one), warm-up runs, medians with fastest, 90th percentile and slowest.
(b) encode_job / decode_job with layout="channel" against the same calls on the same data time-major, from pinned memory,
    65 536 x 10 800 (the shape of tools/e2e_probe.py) and 8 192 x 86 400; the candidates alternate call by call.  These calls
    are synchronous, so their time is the host's wall clock around the call.  Beside them the wall time of the transposition
    a caller does today on this machine's CPU: numpy (one thread) and torch with 16 threads.
Every output is verified before anything is timed."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.aggbench import COPY_TBS, event_ms, spread  # noqa: E402


def copy_library():
    """tools/liblayout_copy.so (the float4-copy yardstick), compiled from tools/layout_copy.hip when it is not there yet"""
    import ctypes as C
    import subprocess
    so, src = os.path.join(ROOT, "tools", "liblayout_copy.so"), os.path.join(ROOT, "tools", "layout_copy.hip")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-shared", src, "-o", so, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    lib = C.CDLL(so)
    lib.layout_copy_f4.restype = C.c_int
    lib.layout_copy_f4.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=86400)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-runs", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layout_bench.txt"))
    args = ap.parse_args()
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    dca = load_package()
    L = dca.library()
    ctx = dca.Context(0)
    lines, results = [], {}

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def line(what, sp, moved_bytes, extra=""):
        tbs = moved_bytes / (sp["median_ms"] * 1e-3) / 1e12
        say("  %-44s median %8.3f ms (fastest %8.3f, p90 %8.3f, slowest %8.3f)  %.2f TB/s%s" % (what, sp["median_ms"], sp["fastest_ms"], sp["p90_ms"], sp["slowest_ms"], tbs, extra))
        return tbs

    def in_turn(cands):
        """cands: {name: fn}; every run times each of them once, in the same order"""
        for _ in range(args.warmup):
            for fn in cands.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in cands}
        for _ in range(args.runs):
            for k, fn in cands.items():
                ms[k].append(event_ms(fn))
        return {k: spread(v) for k, v in ms.items()}

    if not args.skip_kernel:
        copier = copy_library()
        for esz, Cn in ((4, args.channels), (8, args.channels // 2)):
            T = args.samples
            dt = torch.int32 if esz == 4 else torch.int64
            say("kernel, resident: %d channels x %d elements of %d bytes (%.1f GB an image); %d timed runs per candidate, in turn, %d warm-up runs; hipEvents"
                % (Cn, T, esz, Cn * T * esz / 1e9, args.runs, args.warmup))
            x_ct = torch.empty((Cn, T), dtype=dt, device="cuda")
            for c0 in range(0, Cn, 4096):  # (made in bands: randint's temporaries are int64)
                n = min(4096, Cn - c0)
                x_ct[c0 : c0 + n] = torch.randint(0, 2 ** 31 - 1, (n, T), dtype=dt, device="cuda")
            x_tc = torch.empty((T, Cn), dtype=dt, device="cuda")
            back = torch.empty((Cn, T), dtype=dt, device="cuda")
            count = torch.randint(T - T // 10, T + 1, (Cn,), dtype=torch.int64, device="cuda")
            # verified first: against torch on a band of channels, the round trip on everything
            ctx.to_time_major(x_ct, out=x_tc)
            ctx.to_channel_major(x_tc, out=back)
            torch.cuda.synchronize()
            assert torch.equal(x_tc[:, 1000:1300], x_ct[1000:1300].t()) and torch.equal(back, x_ct)
            ctx.to_time_major(x_ct, count=count, out=x_tc)
            live = torch.arange(T, device="cuda")[:, None] < count[None, 500:600]
            assert torch.equal(x_tc[:, 500:600], torch.where(live, x_ct[500:600].t(), torch.zeros((), dtype=dt, device="cuda")))

            def float4_copy():
                assert copier.layout_copy_f4(x_ct.data_ptr(), back.data_ptr(), Cn * T * esz, ctx._stream()) == 0
            back.zero_()
            float4_copy()
            torch.cuda.synchronize()
            assert torch.equal(back, x_ct)
            cands = {
                "float4 copy (the yardstick)": float4_copy,
                "copy (torch, device to device)": lambda: back.copy_(x_ct),
                "to_time_major": lambda: ctx.to_time_major(x_ct, out=x_tc),
                "to_channel_major": lambda: ctx.to_channel_major(x_tc, out=back),
                "to_time_major, counts in [0.9 T, T]": lambda: ctx.to_time_major(x_ct, count=count, out=x_tc),
                "to_channel_major, counts in [0.9 T, T]": lambda: ctx.to_channel_major(x_tc, count=count, out=back),
            }
            agg = None
            if esz == 4:
                agg = torch.empty(((T + 1) // 2, Cn), dtype=torch.float32, device="cuda")
                s = ctx._stream()
                ctx.to_time_major(x_ct, out=x_tc)  # (the aggregate kernel only adds: any bits will do)
                cands["aggregate N = 2 (reads 1, writes 1/2)"] = lambda: L.dega_hip_aggregate_dev(ctx._h, x_tc.data_ptr(), Cn, T, Cn, 2, agg.data_ptr(), Cn, s)
            got = in_turn(cands)
            moved = 2.0 * Cn * T * esz
            copy_tbs = None
            res = {}
            for k, sp in got.items():
                m = moved * 0.75 if k.startswith("aggregate") else moved
                tbs = line(k, sp, m, "" if copy_tbs is None else "  %.2f of this session's float4 copy" % (m / (sp["median_ms"] * 1e-3) / 1e12 / copy_tbs))
                if copy_tbs is None:
                    copy_tbs = tbs
                res[k] = dict(sp, tbs=round(tbs, 3), of_copy=round(tbs / copy_tbs, 3))
            say("  (the float4-copy figure tools/aggbench.py carries from its own session is %.2f TB/s)" % COPY_TBS)
            results["kernel_%d_byte" % esz] = res
            del x_ct, x_tc, back, agg, cands
            torch.cuda.empty_cache()

    if not args.skip_host:
        for Cn, T in ((65536, 10800), (8192, 86400)):
            say("host path from pinned memory: %d channels x %d int32 samples; %d calls per candidate, alternating, one warm-up call each; wall clock around the synchronous call"
                % (Cn, T, args.host_runs))
            x_tc_dev = ctx.synth(Cn, T)
            p_tc = dca.PinnedArray((T, Cn), np.int32)
            p_ct = dca.PinnedArray((Cn, T), np.int32)
            p_tc.array[:] = x_tc_dev.cpu().numpy()
            del x_tc_dev
            t0 = time.perf_counter()
            p_ct.array[:] = p_tc.array.T
            np_s = time.perf_counter() - t0
            torch.set_num_threads(16)
            tt = torch.from_numpy(p_tc.array)
            t0 = time.perf_counter()
            tt.t().contiguous()
            th_s = time.perf_counter() - t0
            say("  the transposition on the CPU today: numpy, one thread, %.0f ms (%.2f Gsamples/s); torch, 16 threads, %.0f ms (%.2f Gsamples/s)"
                % (np_s * 1e3, Cn * T / np_s / 1e9, th_s * 1e3, Cn * T / th_s / 1e9))
            dst = dca.PinnedArray((Cn * (2 * T + 64),), np.uint8)
            enc = {"time": lambda: ctx.encode_job(p_tc.array, packed=dst.array), "channel": lambda: ctx.encode_job(p_ct.array, packed=dst.array, layout="channel")}
            want = enc["time"]()
            want = tuple(a.copy() for a in want)
            got = enc["channel"]()
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), "layouts disagree"
            pk = dca.PinnedArray((want[0].size,), np.uint8)
            pk.array[:] = want[0]
            b_tc = dca.PinnedArray((T, Cn), np.int32)
            b_ct = dca.PinnedArray((Cn, T), np.int32)
            dec = {"time": lambda: ctx.decode_job(pk.array, want[1], want[2], T, out=b_tc.array),
                   "channel": lambda: ctx.decode_job(pk.array, want[1], want[2], T, out=b_ct.array, layout="channel")}
            dec["time"]()
            dec["channel"]()
            assert (b_tc.array == p_tc.array).all() and (b_ct.array == p_ct.array).all(), "decode does not return the samples"
            res = {"numpy_transpose_ms": round(np_s * 1e3, 1), "torch16_transpose_ms": round(th_s * 1e3, 1)}
            for what, cands in (("encode_job", enc), ("decode_job", dec)):
                ms = {k: [] for k in cands}
                for _ in range(args.host_runs):
                    for k, fn in cands.items():
                        t0 = time.perf_counter()
                        fn()
                        ms[k].append((time.perf_counter() - t0) * 1e3)
                sp = {k: spread(v) for k, v in ms.items()}
                for k in cands:
                    say("  %-10s layout=%-8s median %8.2f ms (fastest %8.2f, slowest %8.2f)  %.2f Gsamples/s"
                        % (what, k, sp[k]["median_ms"], sp[k]["fastest_ms"], sp[k]["slowest_ms"], Cn * T / (sp[k]["median_ms"] * 1e-3) / 1e9))
                say("  %-10s channel / time = %.3f" % (what, sp["channel"]["median_ms"] / sp["time"]["median_ms"]))
                res[what] = dict(sp, ratio=round(sp["channel"]["median_ms"] / sp["time"]["median_ms"], 3))
            results["host_%dx%d" % (Cn, T)] = res
            for p in (p_tc, p_ct, dst, pk, b_tc, b_ct):
                p.free()
        say("  (channel-major jobs take whole chunks: no bands, no in-place read of pinned rows -- the time-major call has both)")
    say(json.dumps(results))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
