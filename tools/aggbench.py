#!/usr/bin/env python3
"""Times the aggregate kernel (dega_hip_aggregate_dev) alone, and dega_hip_encode_agg_f32_dev against the plain
dega_hip_encode_f32_dev over the full-resolution rows, on one batch of float32 readings resident on the device.

    python tools/aggbench.py [--channels 65536] [--samples 86400] [--num-values 2 60 900] [--runs 10] [--warmup 2]

hipEvents on the stream the launches use (torch.cuda.Event is one), a few warm-up runs, then the median and the fastest of
`--runs` runs.  The aggregate kernel's figure is GB/s of bytes read plus bytes written (T + ceil(T / N) rows of C floats).
Prints one line per measurement and a JSON summary at the end.

    python tools/aggbench.py --levels 60 300 900 3600 [--runs 50]

times a level set instead: (a) dega_hip_aggregate_dev for each level alone and (b) one dega_hip_aggregate_levels_dev for
all of them, alternating run by run in one session (at least 50 timed runs each: a 4 ms kernel timed ten times is mostly
the clock), medians and the spread, the plan's pass count; then (c) the K dega_hip_encode_agg_f32_dev calls against one
dega_hip_encode_levels_f32_dev.  --host-levels N N ... times Context.encode_job_levels against the K
encode_job(num_values=N) calls on pinned float32 samples (default 65 536 x 10 800 there, the shape of tools/e2e_probe.py)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29  # float4 copy on the MI355X, the streaming yardstick (TB/s)


def timed(fn, runs, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return ms[len(ms) // 2], ms[0]


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": round(ms[len(ms) // 2], 3), "fastest_ms": round(ms[0], 3), "p90_ms": round(ms[(len(ms) * 9) // 10], 3), "slowest_ms": round(ms[-1], 3)}


def readings(ctx, Cn, T):
    """meter-like readings: the library's synthetic random walk (centi-units) as float32 with two decimals, made in bands of rows"""
    import torch
    v = torch.empty((T, Cn), dtype=torch.float32, device="cuda")
    walk = ctx.synth(Cn, T, seed=1234, S=50)
    for t0 in range(0, T, 4096):
        v[t0:t0 + 4096] = walk[t0:t0 + 4096].to(torch.float32) / 100.0
    del walk
    torch.cuda.synchronize()
    return v


def levels(args):
    import ctypes as C
    import torch
    from __graft_entry__ import load_package
    dca = load_package()
    L = dca.library()
    ctx = dca.Context(0)
    Cn, T, Ns = args.channels, args.samples, args.levels
    K, runs = len(Ns), max(args.runs, 50)
    v = readings(ctx, Cn, T)
    s = ctx._stream()
    rows = [L.dega_hip_aggregate_rows(T, N) for N in Ns]
    outs = [torch.empty((r, Cn), dtype=torch.float32, device="cuda") for r in rows]
    nv = (C.c_size_t * K)(*Ns)
    a_ptrs = (C.c_void_p * K)(*[o.data_ptr() for o in outs])
    lds = (C.c_size_t * K)(*[Cn] * K)
    pass_of, step_of = dca.aggregate_levels_plan(Cn, T, Ns, Cn % 4 == 0)

    def single(k):
        return lambda: L.dega_hip_aggregate_dev(ctx._h, v.data_ptr(), Cn, T, Cn, Ns[k], outs[k].data_ptr(), Cn, s)

    def onepass():
        assert L.dega_hip_aggregate_levels_dev(ctx._h, v.data_ptr(), Cn, T, Cn, nv, K, a_ptrs, lds, s) == 0
    for _ in range(args.warmup):
        for k in range(K):
            assert single(k)() == 0
        onepass()
    torch.cuda.synchronize()
    a_ms, b_ms = [[] for _ in range(K)], []
    for _ in range(runs):  # (a) and (b) alternate run by run
        for k in range(K):
            a_ms[k].append(event_ms(single(k)))
        b_ms.append(event_ms(onepass))
    res = {"channels": Cn, "samples": T, "levels": Ns, "runs": runs, "warmup": args.warmup, "passes": len(step_of), "pass_of": pass_of, "step_of": step_of}
    res["single"] = [dict(num_values=N, **spread(a_ms[k])) for k, N in enumerate(Ns)]
    res["one_call"] = spread(b_ms)
    slowest = max(x["median_ms"] for x in res["single"])
    total = sum(x["median_ms"] for x in res["single"])
    res["one_call_over_slowest_single"] = round(res["one_call"]["median_ms"] / slowest, 3)
    res["one_call_over_sum_of_singles"] = round(res["one_call"]["median_ms"] / total, 3)
    print("levels %s on %d x %d: plan = %d pass(es), pass_of %s, step_of %s; %d timed runs each, alternating" % (Ns, Cn, T, len(step_of), pass_of, step_of, runs))
    for x in res["single"]:
        print("(a) aggregate_dev N %5d           median %8.3f ms  fastest %8.3f  p90 %8.3f  slowest %8.3f" % (x["num_values"], x["median_ms"], x["fastest_ms"], x["p90_ms"], x["slowest_ms"]))
    x = res["one_call"]
    print("(b) aggregate_levels_dev, %d levels  median %8.3f ms  fastest %8.3f  p90 %8.3f  slowest %8.3f   = %.3f x the slowest single level (%.3f ms), %.3f x the sum of (a) (%.3f ms)"
          % (K, x["median_ms"], x["fastest_ms"], x["p90_ms"], x["slowest_ms"], res["one_call_over_slowest_single"], slowest, res["one_call_over_sum_of_singles"], total))
    # (c) in front of the coder
    caps = [(4 * r + 64 + 3) & ~3 for r in rows]
    eo = [torch.empty((Cn, c), dtype=torch.uint8, device="cuda") for c in caps]
    eb = [torch.zeros(Cn, dtype=torch.int64, device="cuda") for _ in range(K)]
    ee = [torch.zeros(Cn, dtype=torch.int32, device="cuda") for _ in range(K)]
    ptrs = lambda ts: (C.c_void_p * K)(*[t.data_ptr() for t in ts])  # noqa: E731
    cap_arr = (C.c_size_t * K)(*caps)

    def k_calls():
        for k in range(K):
            assert L.dega_hip_encode_agg_f32_dev(ctx._h, v.data_ptr(), Cn, T, Cn, Ns[k], 100.0, 1, 32, eo[k].data_ptr(), caps[k], eb[k].data_ptr(), ee[k].data_ptr(), s) == 0

    def one_call():
        assert L.dega_hip_encode_levels_f32_dev(ctx._h, v.data_ptr(), Cn, T, Cn, nv, K, 100.0, 1, 32, ptrs(eo), cap_arr, ptrs(eb), ptrs(ee), s) == 0
    for _ in range(args.warmup):
        k_calls()
        one_call()
    torch.cuda.synchronize()
    c_k, c_one = [], []
    enc_runs = max(10, runs // 5)
    for _ in range(enc_runs):
        c_k.append(event_ms(k_calls))
        c_one.append(event_ms(one_call))
    res["encode_k_calls"], res["encode_one_call"] = spread(c_k), spread(c_one)
    res["encode_error_channels"] = int(sum(int((e != 0).sum().item()) for e in ee))
    print("(c) %d x encode_agg_f32_dev          median %8.3f ms  fastest %8.3f   |   encode_levels_f32_dev  median %8.3f ms  fastest %8.3f   (%d runs each, alternating; %d channels with errors)"
          % (K, res["encode_k_calls"]["median_ms"], res["encode_k_calls"]["fastest_ms"], res["encode_one_call"]["median_ms"], res["encode_one_call"]["fastest_ms"],
             enc_runs, res["encode_error_channels"]))
    print(json.dumps(res))
    ctx.close()


def host_levels(args):
    import time
    import numpy as np
    import torch
    from __graft_entry__ import load_package
    dca = load_package()
    ctx = dca.Context(0)
    Ns = args.host_levels
    Cn, T = args.channels, (args.samples if args.samples != 86400 else 10800)
    pin = dca.PinnedArray((T, Cn), np.float32)
    walk = ctx.synth(Cn, T, seed=1234, S=50)
    pin.array[:] = (walk.to(torch.float32) / 100.0).cpu().numpy()
    del walk
    runs = max(3, min(args.runs, 10))
    k_ms, one_ms = [], []
    for i in range(args.warmup + runs):
        t0 = time.perf_counter()
        a = [ctx.encode_job(pin.array, adaptive=1, samples=dca.SAMPLES_F32, factor=100.0, num_values=N) for N in Ns]
        t1 = time.perf_counter()
        b = ctx.encode_job_levels(pin.array, Ns, adaptive=1, factor=100.0)
        t2 = time.perf_counter()
        if i >= args.warmup:
            k_ms.append((t1 - t0) * 1e3)
            one_ms.append((t2 - t1) * 1e3)
        assert all((x[0] == y[0]).all() and (x[1] == y[1]).all() for x, y in zip(a, b))
    res = {"channels": Cn, "samples": T, "levels": Ns, "runs": runs, "k_encode_job_calls": spread(k_ms), "encode_job_levels": spread(one_ms)}
    print("host, pinned %d x %d floats, levels %s: %d x encode_job(num_values=N) median %8.1f ms fastest %8.1f | encode_job_levels median %8.1f ms fastest %8.1f  (%d runs, wall clock incl. the binding's buffers)"
          % (Cn, T, Ns, len(Ns), res["k_encode_job_calls"]["median_ms"], res["k_encode_job_calls"]["fastest_ms"], res["encode_job_levels"]["median_ms"],
             res["encode_job_levels"]["fastest_ms"], runs))
    print(json.dumps(res))
    pin.free()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=86400)
    ap.add_argument("--num-values", type=int, nargs="+", default=[2, 60, 900])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--levels", type=int, nargs="+", default=None, help="time this level set: single-level calls against the one-pass call")
    ap.add_argument("--host-levels", type=int, nargs="+", default=None, help="time encode_job_levels against K encode_job calls on pinned samples")
    args = ap.parse_args()
    if args.host_levels is not None:
        return host_levels(args)
    if args.levels is not None:
        return levels(args)
    import torch
    from __graft_entry__ import load_package
    dca = load_package()
    L = dca.library()
    ctx = dca.Context(0)
    Cn, T = args.channels, args.samples
    # meter-like readings: the library's synthetic random walk (centi-units) as float32 with two decimals, made in bands of rows
    v = torch.empty((T, Cn), dtype=torch.float32, device="cuda")
    walk = ctx.synth(Cn, T, seed=1234, S=50)
    for t0 in range(0, T, 4096):
        v[t0:t0 + 4096] = walk[t0:t0 + 4096].to(torch.float32) / 100.0
    del walk
    torch.cuda.synchronize()
    cap = (4 * T + 64 + 3) & ~3  # a stream is rarely longer than its samples (what the host pipeline starts from too)
    out = torch.empty((Cn, cap), dtype=torch.uint8, device="cuda")
    bits = torch.zeros(Cn, dtype=torch.int64, device="cuda")
    err = torch.zeros(Cn, dtype=torch.int32, device="cuda")
    s = ctx._stream()
    res = {"channels": Cn, "samples": T, "runs": args.runs, "warmup": args.warmup, "levels": []}

    def full():
        assert L.dega_hip_encode_f32_dev(ctx._h, v.data_ptr(), Cn, T, Cn, 100.0, 1, 32, out.data_ptr(), cap, bits.data_ptr(), err.data_ptr(), s) == 0
    full_ms, full_min = timed(full, args.runs, args.warmup)
    assert int((err != 0).sum().item()) == 0
    res["encode_f32_dev_full_resolution_ms"] = round(full_ms, 3)
    print("encode_f32_dev            %d x %d                 median %8.3f ms  fastest %8.3f ms" % (Cn, T, full_ms, full_min))
    for N in args.num_values:
        T_out = L.dega_hip_aggregate_rows(T, N)
        a = torch.empty((T_out, Cn), dtype=torch.float32, device="cuda")

        def agg():
            assert L.dega_hip_aggregate_dev(ctx._h, v.data_ptr(), Cn, T, Cn, N, a.data_ptr(), Cn, s) == 0

        def enc():
            assert L.dega_hip_encode_agg_f32_dev(ctx._h, v.data_ptr(), Cn, T, Cn, N, 100.0, 1, 32, out.data_ptr(), cap, bits.data_ptr(), err.data_ptr(), s) == 0
        agg_ms, agg_min = timed(agg, args.runs, args.warmup)
        moved = 4.0 * Cn * (T + T_out)
        gbs = moved / (agg_ms * 1e-3) / 1e9
        enc_ms, enc_min = timed(enc, args.runs, args.warmup)
        bad = int((err != 0).sum().item())
        print("aggregate_dev      N %4d  %d x %d -> %6d rows  median %8.3f ms  fastest %8.3f ms  %8.1f GB/s read + written  (%.2f of the %.2f TB/s copy figure)"
              % (N, Cn, T, T_out, agg_ms, agg_min, gbs, gbs / 1e3 / COPY_TBS, COPY_TBS))
        print("encode_agg_f32_dev N %4d                                 median %8.3f ms  fastest %8.3f ms  %.3f of encode_f32_dev at full resolution; %d channels with errors"
              % (N, enc_ms, enc_min, enc_ms / full_ms, bad))
        res["levels"].append({"num_values": N, "rows_out": T_out, "aggregate_ms": round(agg_ms, 3), "aggregate_GBps": round(gbs, 1),
                              "fraction_of_copy": round(gbs / 1e3 / COPY_TBS, 3), "encode_agg_ms": round(enc_ms, 3),
                              "encode_agg_over_full": round(enc_ms / full_ms, 3), "error_channels": bad})
        del a
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
