#!/usr/bin/env python3
"""Times the aggregate kernel (dega_hip_aggregate_dev) alone, and dega_hip_encode_agg_f32_dev against the plain
dega_hip_encode_f32_dev over the full-resolution rows, on one batch of float32 readings resident on the device.

    python tools/aggbench.py [--channels 65536] [--samples 86400] [--num-values 2 60 900] [--runs 10] [--warmup 2]

hipEvents on the stream the launches use (torch.cuda.Event is one), a few warm-up runs, then the median and the fastest of
`--runs` runs.  The aggregate kernel's figure is GB/s of bytes read plus bytes written (T + ceil(T / N) rows of C floats).
Prints one line per measurement and a JSON summary at the end."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=86400)
    ap.add_argument("--num-values", type=int, nargs="+", default=[2, 60, 900])
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
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
