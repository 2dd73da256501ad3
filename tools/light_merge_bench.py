#!/usr/bin/env python3
"""Times the merge of light accumulators (rt4.h rt4_light_merge_device) on the MI355X: K = 8 source
accumulators of 1920 x 1080 pixels merged into one, as the root of an 8-GPU frame-split run does.

  one_call     one rt4_light_merge_device with n_srcs = 8: 32 (K + 2) B per pixel (dst read and written, every source read)
  eight_calls  eight calls with one source each, the same result bit for bit: 96 K B per pixel

The sources are synthetic accumulators (random means, n = 4 each): the kernel's work does not depend on the values.
Each variant is timed between two device events around --inner back-to-back calls on the stream, after --warmup such
groups; the median of --reps groups is reported with the smallest and the largest, per call. The two variants alternate
twice, so that neither always has the warmer chip; the two medians are averaged. Rates are the bytes named above over
the time: achieved bytes per second of the algorithm's traffic, not a counter reading (8 sources of 66 MB do not stay
in the 256 MiB Infinity Cache between calls). Informational: there is no earlier merge to compare against.
One JSON line; --out also writes it to a file.
Usage (GPU): python tools/light_merge_bench.py [--reps 20] [--warmup 3] [--inner 10] [--out profiles/light_merge_bench.json]
A run without a GPU fails: nothing here is measured on the CPU."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, K, PX = 1920, 1080, 8, 32


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("light_merge_bench: no GPU")
    torch.cuda.init()
    rt4 = importlib.import_module("4d_ray_tracing_amd.rt4")
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream

    def median_ms(fn):
        def group():
            for _ in range(args.inner):
                fn()

        for _ in range(args.warmup):
            group()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            group()
            e1.record(stream)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / args.inner)
        return statistics.median(times), min(times), max(times)

    t = rt4.Tracer(device=0)
    try:
        gen = torch.Generator(device="cuda").manual_seed(7)

        def accumulators(n):
            a = torch.rand((n, H, W, 8), generator=gen, device="cuda", dtype=torch.float32)
            a[..., 5] = torch.tensor(4, dtype=torch.int32).view(torch.float32)  # n = 4 frames
            a[..., 6:] = 0
            return a

        srcs, dst0 = accumulators(K), accumulators(1)[0]
        # the two variants agree bit for bit before either is timed
        once, many = dst0.clone(), dst0.clone()
        t.light_merge_device(once.data_ptr(), W, srcs.data_ptr(), W, W * H, K, W, H, s)
        for q in range(K):
            t.light_merge_device(many.data_ptr(), W, srcs[q].data_ptr(), W, W * H, 1, W, H, s)
        torch.cuda.synchronize()
        if not torch.equal(once.view(torch.int32), many.view(torch.int32)):
            sys.exit("light_merge_bench: one call and eight calls differ")
        if int(once[0, 0, 5].view(torch.int32).item()) != 4 * (K + 1):
            sys.exit("light_merge_bench: unexpected frame count after the merge")
        dst = dst0.clone()

        def one_call():
            t.light_merge_device(dst.data_ptr(), W, srcs.data_ptr(), W, W * H, K, W, H, s)

        def eight_calls():
            for q in range(K):
                t.light_merge_device(dst.data_ptr(), W, srcs[q].data_ptr(), W, W * H, 1, W, H, s)

        order = [("one_call", one_call), ("eight_calls", eight_calls)]
        runs = {name: [] for name, _ in order}
        for _ in range(2):
            for name, fn in order:
                runs[name].append(median_ms(fn))
        torch.cuda.synchronize()
        ms = {name: sum(r[0] for r in rs) / len(rs) for name, rs in runs.items()}
        npx = W * H
        bytes_moved = {"one_call": PX * (K + 2) * npx, "eight_calls": 3 * PX * K * npx}
        result = {"width": W, "height": H, "sources": K, "reps": args.reps, "warmup": args.warmup, "inner": args.inner}
        for name, rs in runs.items():
            result[name + "_ms"] = round(ms[name], 4)
            result[name + "_ms_runs"] = [round(r[0], 4) for r in rs]
            result[name + "_ms_min_max"] = [round(min(r[1] for r in rs), 4), round(max(r[2] for r in rs), 4)]
            result[name + "_bytes"] = bytes_moved[name]
            result[name + "_gbytes_per_s"] = round(bytes_moved[name] / (ms[name] * 1e-3) / 1e9, 1)
        result["eight_calls_over_one_call"] = round(ms["eight_calls"] / ms["one_call"], 3)
        result["devices"] = torch.cuda.device_count()
        result["build"] = rt4.lib.rt4_build_info().decode()
        line = json.dumps(result)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
    finally:
        t.close()


if __name__ == "__main__":
    main()
