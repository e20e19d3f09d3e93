#!/usr/bin/env python3
"""Times the `encode csv` kernel (dega_hip_csv_write_dev) on one batch of float32 two-decimal readings resident on the
device, in the manner of tools/aggbench.py: hipEvents on the stream the launches use, warm-up runs, then medians and the
spread of `--runs` timed runs (at least 50 for anything that takes less than 10 ms).

    python tools/csvbench.py [--channels 65536] [--samples 86400] [--runs 50] [--warmup 2] [--lzmh-runs 2]

In one session, alternating run by run:
  (a) dega_hip_csv_write_dev with 8-byte stores, (b) the same with LDS-staged 64-byte blocks (DEGA_CSV_STORE), and
  (c) dega_hip_lzmh_render_dev on the int32 centi-unit version of the same readings (what the library had before; the
      same text, which is checked).
Then the stages around it: (d) dega_hip_lzmh_encode_dev over the produced text (the stage it feeds), (e)
dega_hip_decode_f32_dev over the DEGA streams of the same readings (the stage it follows in the decode direction).
The kernel's two bounds are printed beside (a)/(b): bytes read plus text bytes written over the float4-copy yardstick, and
the issue floor from --valu-per-value (the kernel's VALU instructions per value, counted in its ISA) x 4.3 cycles x T at
one wave per SIMD.  Prints one line per measurement and a JSON summary at the end.

    python tools/csvbench.py --split [--split-channels 1,16,256,4096,65536] [--split-block-rows 1,4,...] [--samples 86400]

The sweep of the split writer (dega_hip_csv_write_split_dev): per channel count one batch of the same readings, and per
block_rows -- the library's choice (0) first, then the list -- the split call beside dega_hip_csv_write_dev on the same
data, alternating run by run; every split result is compared with the unsplit bytes, lengths and status before anything is
timed.  Cells with more than --split-max-pairs (channel, block) pairs are left out.  One line per cell: median, fastest and
slowest of both."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29    # float4 copy on the MI355X, the streaming yardstick (TB/s; tools/aggbench.py)
CLOCK_GHZ = 2.4    # MI355X peak engine clock
CYCLES_PER_VALU = 4.3  # measured cost of a dependent VALU instruction of one wave


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
    return {"runs": len(ms), "median_ms": round(ms[len(ms) // 2], 3), "fastest_ms": round(ms[0], 3), "p90_ms": round(ms[(len(ms) * 9) // 10], 3),
            "slowest_ms": round(ms[-1], 3)}


def show(label, x, extra=""):
    print("%-46s median %10.3f ms  fastest %10.3f  p90 %10.3f  slowest %10.3f  (%d runs)%s"
          % (label, x["median_ms"], x["fastest_ms"], x["p90_ms"], x["slowest_ms"], x["runs"], extra))


def split_sweep(args):
    import torch
    from __graft_entry__ import load_package
    dca = load_package()
    L = dca.library()
    ctx = dca.Context(0)
    s = ctx._stream()
    T = args.samples
    stride = (T * 9 + 16 + 15) // 16 * 16
    res = {"samples": T, "cells": []}
    for Cn in [int(c) for c in args.split_channels.split(",")]:
        x = ctx.synth(Cn, T, seed=1234, S=50)  # centi-units, the workload of bench.py
        v = torch.empty((T, Cn), dtype=torch.float32, device="cuda")
        for t0 in range(0, T, 4096):
            v[t0:t0 + 4096] = x[t0:t0 + 4096].to(torch.float32) / 100.0
        del x
        text = torch.empty((Cn, stride), dtype=torch.uint8, device="cuda")
        text0 = torch.empty((Cn, stride), dtype=torch.uint8, device="cuda")
        lens, lens0 = torch.zeros(Cn, dtype=torch.int64, device="cuda"), torch.zeros(Cn, dtype=torch.int64, device="cuda")
        err, err0 = torch.zeros(Cn, dtype=torch.int32, device="cuda"), torch.zeros(Cn, dtype=torch.int32, device="cuda")

        def unsplit():
            assert L.dega_hip_csv_write_dev(ctx._h, v.data_ptr(), Cn, T, Cn, 2, 1, 44, text0.data_ptr(), stride, lens0.data_ptr(), err0.data_ptr(), s) == 0

        unsplit()
        torch.cuda.synchronize()
        assert int((err0 != 0).sum().item()) == 0
        chosen = dca.csv_write_split_block_rows(Cn, T)
        print("%d channels x %d readings, %d text bytes; the library's block_rows: %d" % (Cn, T, int(lens0.sum().item()), chosen))
        for R in [0] + [int(r) for r in args.split_block_rows.split(",")]:
            rows = chosen if R == 0 else min(R, T)
            pairs = Cn * (-(-T // rows))
            if pairs > args.split_max_pairs:
                print("  block_rows %6d: %d pairs, left out" % (rows, pairs))
                continue

            def split():
                assert L.dega_hip_csv_write_split_dev(ctx._h, v.data_ptr(), Cn, T, Cn, None, 2, 1, 44, text.data_ptr(), stride, lens.data_ptr(), err.data_ptr(),
                                                      R, s) == 0

            text.fill_(0xEE)
            split()
            torch.cuda.synchronize()
            assert torch.equal(lens, lens0) and torch.equal(err, err0), "the split writer disagrees on the lengths"
            for c0 in range(0, Cn, 256):  # (the benchmark's channels differ in length by a few bytes)
                n = int(lens0[c0:c0 + 256].min())
                assert torch.equal(text[c0:c0 + 256, :n], text0[c0:c0 + 256, :n]), "the split writer disagrees on the text"
                assert bool((text[c0:c0 + 256, int(lens0[c0:c0 + 256].max()):] == 0xEE).all()), "the split writer wrote behind the text"
            first = event_ms(split)
            runs = 30 if first < 5.0 else (10 if first < 60.0 else 3)
            a, b = [], []
            for _ in range(runs):  # alternating run by run
                a.append(event_ms(split))
                b.append(event_ms(unsplit))
            cell = {"channels": Cn, "block_rows": rows, "library_choice": R == 0, "pairs": pairs, "split": spread(a), "unsplit": spread(b)}
            res["cells"].append(cell)
            print("  block_rows %6d%s %10d pairs  split median %9.3f fastest %9.3f slowest %9.3f | unsplit median %9.3f fastest %9.3f slowest %9.3f ms  (%d runs)  %.2fx"
                  % (rows, "*" if R == 0 else " ", pairs, cell["split"]["median_ms"], cell["split"]["fastest_ms"], cell["split"]["slowest_ms"],
                     cell["unsplit"]["median_ms"], cell["unsplit"]["fastest_ms"], cell["unsplit"]["slowest_ms"], runs,
                     cell["unsplit"]["median_ms"] / cell["split"]["median_ms"]), flush=True)
        del v, text, text0
    print(json.dumps(res))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=65536)
    ap.add_argument("--samples", type=int, default=86400)
    ap.add_argument("--runs", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lzmh-runs", type=int, default=2, help="timed runs of the LZMH encoder over the text (seconds each at full size)")
    ap.add_argument("--valu-per-value", type=float, default=0.0, help="VALU instructions per value of the kernel's loop, for the issue floor")
    ap.add_argument("--split", action="store_true", help="the sweep of the split writer instead (see the top)")
    ap.add_argument("--split-channels", default="1,16,256,4096,65536")
    ap.add_argument("--split-block-rows", default="1,4,16,64,256,1024,4096,21600,86400")
    ap.add_argument("--split-max-pairs", type=int, default=400 << 20)
    args = ap.parse_args()
    if args.split:
        return split_sweep(args)
    import torch
    from __graft_entry__ import load_package
    dca = load_package()
    L = dca.library()
    ctx = dca.Context(0)
    Cn, T = args.channels, args.samples
    s = ctx._stream()
    x = ctx.synth(Cn, T, seed=1234, S=50)  # centi-units, the workload of bench.py
    v = torch.empty((T, Cn), dtype=torch.float32, device="cuda")
    for t0 in range(0, T, 4096):
        v[t0:t0 + 4096] = x[t0:t0 + 4096].to(torch.float32) / 100.0
    stride = (T * 9 + 16 + 15) // 16 * 16
    text = torch.empty((Cn, stride), dtype=torch.uint8, device="cuda")
    text_old = torch.empty((Cn, stride), dtype=torch.uint8, device="cuda")
    lens = torch.zeros(Cn, dtype=torch.int64, device="cuda")
    lens_old = torch.zeros(Cn, dtype=torch.int64, device="cuda")
    err = torch.zeros(Cn, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def csv(form):
        def run():
            os.environ["DEGA_CSV_STORE"] = form
            assert L.dega_hip_csv_write_dev(ctx._h, v.data_ptr(), Cn, T, Cn, 2, 1, 44, text.data_ptr(), stride, lens.data_ptr(), err.data_ptr(), s) == 0
        return run

    def render_old():
        assert L.dega_hip_lzmh_render_dev(ctx._h, x.data_ptr(), Cn, T, Cn, text_old.data_ptr(), stride, lens_old.data_ptr(), err.data_ptr(), s) == 0

    fns = {"csv_write_dev, 8-byte stores": csv("8"), "csv_write_dev, 64-byte blocks (LDS)": csv("64"), "lzmh_render_dev (int32 centi-units)": render_old}
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    first = event_ms(fns["csv_write_dev, 8-byte stores"])
    runs = max(args.runs, 50) if first < 10.0 else args.runs
    ms = {k: [] for k in fns}
    for _ in range(runs):  # alternating run by run
        for k, fn in fns.items():
            ms[k].append(event_ms(fn))
    assert int((err != 0).sum().item()) == 0
    assert torch.equal(lens, lens_old), "the two renderers disagree on the lengths"
    same = all(torch.equal(text[c0:c0 + 256, :int(lens[c0:c0 + 256].min())], text_old[c0:c0 + 256, :int(lens[c0:c0 + 256].min())]) for c0 in range(0, Cn, 256))
    assert same, "the two renderers disagree on the text"
    text_bytes = int(lens.sum().item())
    moved = 4.0 * Cn * T + text_bytes
    bw_floor_ms = moved / (COPY_TBS * 1e12) * 1e3
    waves_per_simd = max(1.0, Cn / 64.0 / 1024.0)  # 256 CUs x 4 SIMDs
    issue_floor_ms = args.valu_per_value * CYCLES_PER_VALU * T * waves_per_simd / (CLOCK_GHZ * 1e9) * 1e3
    res = {"channels": Cn, "samples": T, "warmup": args.warmup, "text_bytes": text_bytes, "bytes_per_value": round(text_bytes / (Cn * T), 3),
           "bandwidth_floor_ms": round(bw_floor_ms, 3), "valu_per_value": args.valu_per_value, "issue_floor_ms": round(issue_floor_ms, 3)}
    print("%d channels x %d readings, %.2f text bytes per value; bounds: %.3f ms at %.2f TB/s for %.2f GB read + written; issue floor %.3f ms (%.0f VALU/value x %.1f cycles x T x %.2f waves/SIMD at %.1f GHz)"
          % (Cn, T, res["bytes_per_value"], bw_floor_ms, COPY_TBS, moved / 1e9, issue_floor_ms, args.valu_per_value, CYCLES_PER_VALU, waves_per_simd, CLOCK_GHZ))
    for k in fns:
        res[k] = spread(ms[k])
        extra = ""
        if k.startswith("csv"):
            extra = "  %.1f GB/s; %.2f x the bandwidth bound" % (moved / (res[k]["median_ms"] * 1e-3) / 1e9, res[k]["median_ms"] / bw_floor_ms)
            if issue_floor_ms > 0:
                extra += ", %.2f x the issue floor" % (res[k]["median_ms"] / issue_floor_ms)
        show(k, res[k], extra)
    best = min(res["csv_write_dev, 8-byte stores"]["median_ms"], res["csv_write_dev, 64-byte blocks (LDS)"]["median_ms"])
    del text_old, lens_old

    # (d) the stage it feeds
    if args.lzmh_runs > 0:
        cap = (stride // 2 + 64 + 15) // 16 * 16  # meter text codes to about a third
        out = torch.empty((Cn, cap), dtype=torch.uint8, device="cuda")
        bits = torch.zeros(Cn, dtype=torch.int64, device="cuda")

        def lz():
            assert L.dega_hip_lzmh_encode_dev(ctx._h, text.data_ptr(), stride, lens.data_ptr(), Cn, out.data_ptr(), cap, bits.data_ptr(), err.data_ptr(), s) == 0
        lz()
        torch.cuda.synchronize()
        res["lzmh_encode_dev over the text"] = spread([event_ms(lz) for _ in range(args.lzmh_runs)])
        res["lzmh_error_channels"] = int((err != 0).sum().item())
        res["renderer_share_of_lzmh_encode"] = round(best / res["lzmh_encode_dev over the text"]["median_ms"], 4)
        show("lzmh_encode_dev over the text", res["lzmh_encode_dev over the text"],
             "  renderer = %.4f of it; %d channels with errors" % (res["renderer_share_of_lzmh_encode"], res["lzmh_error_channels"]))
        del out, bits
    del text

    # (e) the stage it follows in the decode direction
    cap = (4 * T + 64 + 3) & ~3
    streams = torch.empty((Cn, cap), dtype=torch.uint8, device="cuda")
    sbits = torch.zeros(Cn, dtype=torch.int64, device="cuda")
    assert L.dega_hip_encode_f32_dev(ctx._h, v.data_ptr(), Cn, T, Cn, 100.0, 1, 32, streams.data_ptr(), cap, sbits.data_ptr(), err.data_ptr(), s) == 0
    torch.cuda.synchronize()

    def dec():
        assert L.dega_hip_decode_f32_dev(ctx._h, streams.data_ptr(), cap, sbits.data_ptr(), Cn, T, Cn, 100.0, 1, 32, v.data_ptr(), None, err.data_ptr(), s) == 0
    dec()
    torch.cuda.synchronize()
    res["decode_f32_dev"] = spread([event_ms(dec) for _ in range(max(5, min(runs, 20)))])
    res["renderer_over_decode_f32"] = round(best / res["decode_f32_dev"]["median_ms"], 3)
    show("decode_f32_dev", res["decode_f32_dev"], "  renderer = %.3f x it" % res["renderer_over_decode_f32"])
    print(json.dumps(res))
    ctx.close()


if __name__ == "__main__":
    main()
