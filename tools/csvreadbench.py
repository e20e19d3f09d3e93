#!/usr/bin/env python3
"""Times the `decode csv` kernel (dega_hip_csv_read_dev) on the two-decimal text of the benchmark's walk resident on the
device, in the manner of tools/csvbench.py: hipEvents on the stream the launches use, warm-up runs, then medians and the
spread of `--runs` timed runs, the candidates alternating run by run.

    python tools/csvreadbench.py [--channels 256 65536] [--samples 86400] [--runs 10] [--warmup 2] [--out profiles/csv_read_bench.txt]

Candidates, per channel count:
  (a) dega_hip_csv_read_dev over the text,
  (b) dega_hip_lzmh_decode_dev producing the same text from its LZMH streams: the stage (a) follows,
  (c) dega_hip_csv_write_dev producing the text from the floats: its mirror,
  (d) dega_hip_lzmh_decode_f32_dev: (b) + (a) + the status launch, as a whole.
What (a) reads back is compared with the floats the text was written from, bit for bit.  The kernel's two bounds are printed
beside (a): text bytes read plus float bytes written over the float4-copy yardstick, and the issue floor from
--instr-per-byte and --instr-per-value (the kernel's instructions per text byte and per value, counted in its ISA) x 4.3
cycles at the waves per SIMD the batch gives.  Prints one line per measurement and a JSON summary per channel count; --out
also writes them to a file.

    python tools/csvreadbench.py --split [--channels 1 16 256 4096 65536] [--out profiles/csv_read_split_bench.txt]

measures instead dega_hip_csv_read_split_dev (one channel's text split over lanes) at block_bytes 64, 256, 1 024, 4 096,
16 384 and at the library's choice, alternating run by run with (a), the existing kernel, in the same session.  Every split
result is compared bit for bit with the floats the text was written from before anything is timed.  One line per
candidate (median, fastest .. slowest, the ratio of (a)'s median to it) and a JSON summary per channel count."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_TBS = 6.29    # float4 copy on the MI355X, the streaming yardstick (TB/s; tools/aggbench.py)
CLOCK_GHZ = 2.4    # MI355X peak engine clock
CYCLES_PER_INSTR = 4.3  # measured cost of a dependent VALU instruction of one wave


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


def one_size(dca, ctx, Cn, T, args, say):
    import torch
    L = dca.library()
    s = ctx._stream()
    x = ctx.synth(Cn, T, seed=1234, S=50)  # centi-units, the workload of bench.py
    v = torch.empty((T, Cn), dtype=torch.float32, device="cuda")
    hundred = torch.full((), 100.0, dtype=torch.float64, device="cuda")  # (a tensor: torch multiplies by the reciprocal of a scalar divisor)
    for t0 in range(0, T, 4096):  # floats of two-decimal numbers: divided in double, rounded once
        v[t0:t0 + 4096] = (x[t0:t0 + 4096].to(torch.float64) / hundred).to(torch.float32)
    del x
    stride = (T * 9 + 16 + 15) // 16 * 16
    text = torch.empty((Cn, stride), dtype=torch.uint8, device="cuda")
    lens = torch.zeros(Cn, dtype=torch.int64, device="cuda")
    err = torch.zeros(Cn, dtype=torch.int32, device="cuda")
    back = torch.empty((T, Cn), dtype=torch.float32, device="cuda")
    count = torch.zeros(Cn, dtype=torch.int64, device="cuda")

    def write():
        assert L.dega_hip_csv_write_dev(ctx._h, v.data_ptr(), Cn, T, Cn, 2, 1, 44, text.data_ptr(), stride, lens.data_ptr(), err.data_ptr(), s) == 0
    write()
    torch.cuda.synchronize()
    assert int((err != 0).sum().item()) == 0
    text_bytes = int(lens.sum().item())
    # the LZMH streams of that text, once (seconds at full size)
    cap = (stride // 2 + 64 + 15) // 16 * 16  # meter text codes to about a third
    streams = torch.empty((Cn, cap), dtype=torch.uint8, device="cuda")
    bits = torch.zeros(Cn, dtype=torch.int64, device="cuda")
    enc_ms = event_ms(lambda: L.dega_hip_lzmh_encode_dev(ctx._h, text.data_ptr(), stride, lens.data_ptr(), Cn, streams.data_ptr(), cap, bits.data_ptr(),
                                                         err.data_ptr(), s))
    assert int((err != 0).sum().item()) == 0, "the LZMH encoder ran out of room"
    lens2 = torch.zeros(Cn, dtype=torch.int64, device="cuda")

    def read():
        assert L.dega_hip_csv_read_dev(ctx._h, text.data_ptr(), stride, lens.data_ptr(), Cn, 1, 44, back.data_ptr(), T, Cn, count.data_ptr(), err.data_ptr(), s) == 0

    def lz_decode():  # (into the text it was coded from: the same bytes)
        assert L.dega_hip_lzmh_decode_dev(ctx._h, streams.data_ptr(), cap, bits.data_ptr(), Cn, text.data_ptr(), stride, lens2.data_ptr(), err.data_ptr(), s) == 0

    def whole():
        assert L.dega_hip_lzmh_decode_f32_dev(ctx._h, streams.data_ptr(), cap, bits.data_ptr(), Cn, stride, 1, 44, back.data_ptr(), T, Cn, count.data_ptr(),
                                              lens2.data_ptr(), err.data_ptr(), s) == 0

    def checked(what):
        torch.cuda.synchronize()
        assert int((err != 0).sum().item()) == 0 and int((count != T).sum().item()) == 0, what
        assert all(torch.equal(back[t0:t0 + 4096].view(torch.int32), v[t0:t0 + 4096].view(torch.int32)) for t0 in range(0, T, 4096)), what

    fns = {"csv_read_dev": read, "lzmh_decode_dev (the same text)": lz_decode, "csv_write_dev (its mirror)": write, "lzmh_decode_f32_dev (whole)": whole}
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    read()
    checked("csv_read_dev does not return the floats the text was written from")
    back.zero_()
    whole()
    checked("lzmh_decode_f32_dev does not return the floats the text was written from")
    assert torch.equal(lens, lens2)
    ms = {k: [] for k in fns}
    for _ in range(args.runs):  # alternating run by run
        for k, fn in fns.items():
            ms[k].append(event_ms(fn))
    moved = text_bytes + 4.0 * Cn * T
    bw_floor_ms = moved / (COPY_TBS * 1e12) * 1e3
    waves_per_simd = max(1.0, Cn / 64.0 / 1024.0)  # 256 CUs x 4 SIMDs
    instr = args.instr_per_byte * text_bytes / Cn + args.instr_per_value * T  # per lane
    issue_floor_ms = instr * CYCLES_PER_INSTR * waves_per_simd / (CLOCK_GHZ * 1e9) * 1e3
    res = {"channels": Cn, "samples": T, "warmup": args.warmup, "text_bytes": text_bytes, "bytes_per_value": round(text_bytes / (Cn * T), 3),
           "bandwidth_floor_ms": round(bw_floor_ms, 3), "instr_per_byte": args.instr_per_byte, "instr_per_value": args.instr_per_value,
           "issue_floor_ms": round(issue_floor_ms, 3), "lzmh_encode_dev_once_ms": round(enc_ms, 1)}
    say("%d channels x %d readings, %.2f text bytes per value; bounds: %.3f ms at %.2f TB/s for %.2f GB read + written; issue floor %.3f ms "
        "((%.0f instr/byte x %.2f bytes + %.0f instr/value) x T x %.1f cycles x %.2f waves/SIMD at %.1f GHz)"
        % (Cn, T, res["bytes_per_value"], bw_floor_ms, COPY_TBS, moved / 1e9, issue_floor_ms, args.instr_per_byte, res["bytes_per_value"], args.instr_per_value,
           CYCLES_PER_INSTR, waves_per_simd, CLOCK_GHZ))
    for k in fns:
        res[k] = spread(ms[k])
        extra = ""
        if k == "csv_read_dev":
            extra = "  %.1f GB/s; %.2f x the bandwidth bound" % (moved / (res[k]["median_ms"] * 1e-3) / 1e9, res[k]["median_ms"] / bw_floor_ms)
            if issue_floor_ms > 0:
                extra += ", %.2f x the issue floor" % (res[k]["median_ms"] / issue_floor_ms)
        x = res[k]
        say("%-34s median %10.3f ms  fastest %10.3f  p90 %10.3f  slowest %10.3f  (%d runs)%s"
            % (k, x["median_ms"], x["fastest_ms"], x["p90_ms"], x["slowest_ms"], x["runs"], extra))
    r = res["csv_read_dev"]["median_ms"]
    res["reader_over_lzmh_decode"] = round(r / res["lzmh_decode_dev (the same text)"]["median_ms"], 3)
    res["reader_over_writer"] = round(r / res["csv_write_dev (its mirror)"]["median_ms"], 3)
    res["whole_over_parts"] = round(res["lzmh_decode_f32_dev (whole)"]["median_ms"] / (r + res["lzmh_decode_dev (the same text)"]["median_ms"]), 3)
    say("reader = %.3f x the LZMH decoder in front of it, %.3f x the writer; the whole = %.3f x (decoder + reader)"
        % (res["reader_over_lzmh_decode"], res["reader_over_writer"], res["whole_over_parts"]))
    say(json.dumps(res))
    return res


SPLIT_BLOCKS = (64, 256, 1024, 4096, 16384)


def one_size_split(dca, ctx, Cn, T, args, say):
    import torch
    L = dca.library()
    s = ctx._stream()
    x = ctx.synth(Cn, T, seed=1234, S=50)
    v = torch.empty((T, Cn), dtype=torch.float32, device="cuda")
    hundred = torch.full((), 100.0, dtype=torch.float64, device="cuda")
    for t0 in range(0, T, 4096):
        v[t0:t0 + 4096] = (x[t0:t0 + 4096].to(torch.float64) / hundred).to(torch.float32)
    del x
    stride = (T * 9 + 16 + 15) // 16 * 16
    text = torch.empty((Cn, stride), dtype=torch.uint8, device="cuda")
    lens = torch.zeros(Cn, dtype=torch.int64, device="cuda")
    err = torch.zeros(Cn, dtype=torch.int32, device="cuda")
    back = torch.empty((T, Cn), dtype=torch.float32, device="cuda")
    count = torch.zeros(Cn, dtype=torch.int64, device="cuda")
    assert L.dega_hip_csv_write_dev(ctx._h, v.data_ptr(), Cn, T, Cn, 2, 1, 44, text.data_ptr(), stride, lens.data_ptr(), err.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert int((err != 0).sum().item()) == 0
    text_bytes = int(lens.sum().item())
    chosen = dca.csv_read_split_block_bytes(Cn, stride)

    def read():
        assert L.dega_hip_csv_read_dev(ctx._h, text.data_ptr(), stride, lens.data_ptr(), Cn, 1, 44, back.data_ptr(), T, Cn, count.data_ptr(), err.data_ptr(), s) == 0

    def split(block_bytes):
        def fn():
            assert L.dega_hip_csv_read_split_dev(ctx._h, text.data_ptr(), stride, lens.data_ptr(), Cn, 1, 44, back.data_ptr(), T, Cn, count.data_ptr(),
                                                 err.data_ptr(), block_bytes, s) == 0
        return fn

    def checked(what):
        torch.cuda.synchronize()
        assert int((err != 0).sum().item()) == 0 and int((count != T).sum().item()) == 0, what
        assert all(torch.equal(back[t0:t0 + 4096].view(torch.int32), v[t0:t0 + 4096].view(torch.int32)) for t0 in range(0, T, 4096)), what

    fns = {"csv_read_dev": read}
    for B in SPLIT_BLOCKS:
        fns["csv_read_split_dev block_bytes=%d" % B] = split(B)
    fns["csv_read_split_dev library's choice (%d)" % chosen] = split(0)
    for k, fn in fns.items():  # right before it is timed
        back.zero_()
        count.zero_()
        fn()
        checked(k + " does not return the floats the text was written from")
    for _ in range(args.warmup):
        for fn in fns.values():
            fn()
    ms = {k: [] for k in fns}
    for _ in range(args.runs):  # alternating run by run
        for k, fn in fns.items():
            ms[k].append(event_ms(fn))
    res = {"channels": Cn, "samples": T, "warmup": args.warmup, "stride": stride, "text_bytes": text_bytes, "library_block_bytes": chosen,
           "library_pairs": Cn * ((stride + chosen - 1) // chosen)}
    say("%d channels x %d readings, %d text bytes, stride %d; the library's choice of block_bytes: %d (%d pairs)"
        % (Cn, T, text_bytes, stride, chosen, res["library_pairs"]))
    base = None
    for k in fns:
        x = res[k] = spread(ms[k])
        base = x if base is None else base
        say("%-46s median %10.3f ms  fastest %10.3f .. slowest %10.3f  (%d runs)  existing / this = %8.3f"
            % (k, x["median_ms"], x["fastest_ms"], x["slowest_ms"], x["runs"], base["median_ms"] / x["median_ms"]))
    mine = res["csv_read_split_dev library's choice (%d)" % chosen]
    res["existing_over_library_choice"] = round(base["median_ms"] / mine["median_ms"], 3)
    res["ranges_apart"] = mine["slowest_ms"] < base["fastest_ms"]
    say("library's choice: slowest %.3f ms %s the existing kernel's fastest %.3f ms" % (mine["slowest_ms"], "<" if res["ranges_apart"] else ">=", base["fastest_ms"]))
    say(json.dumps(res))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, nargs="+", default=None, help="default 256 65536; with --split 1 16 256 4096 65536")
    ap.add_argument("--split", action="store_true", help="measure dega_hip_csv_read_split_dev against the existing kernel instead")
    ap.add_argument("--samples", type=int, default=86400)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--instr-per-byte", type=float, default=0.0, help="instructions per text byte of the kernel's loop, for the issue floor")
    ap.add_argument("--instr-per-value", type=float, default=0.0, help="instructions per value (conversion and store), for the issue floor")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    import torch
    from __graft_entry__ import load_package
    dca = load_package()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)
    if args.channels is None:
        args.channels = [1, 16, 256, 4096, 65536] if args.split else [256, 65536]
    for Cn in args.channels:
        ctx = dca.Context(0)
        (one_size_split if args.split else one_size)(dca, ctx, Cn, args.samples, args, say)
        ctx.close()
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
