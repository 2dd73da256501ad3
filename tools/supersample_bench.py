#!/usr/bin/env python3
"""Times the downsample of supersampled light accumulators (rt4.h rt4_light_downsample_device) on the
MI355X, and what --supersample costs a render at equal rays.

  (a) the kernel: output 1920 x 1080 at s = 2 and output 960 x 540 at s = 4, both from a 3840 x 2160 fine accumulator:
      32 (s^2 + 1) B per output pixel. Next to it, in the same process and on the same fine pixels, the yardstick:
      rt4_light_merge_device with one source (96 B per pixel: dst read and written, the source read).
      Then s = 2 and the merge once more on four times the pixels (a 7680 x 4320 fine accumulator), which separates
      what a call costs from what a byte costs.
  (b) the render: rt4_render_light_device of sphere at 1920 x 1080, 16 spp, 64 frames, against 3840 x 2160, 16 spp,
      16 frames plus one downsample at s = 2. The same number of rays.

The accumulators of (a) are synthetic (random means, n = 4): the kernel's work does not depend on the values. Each leg is
timed between two device events around --inner back-to-back calls on the stream ((b): one call), after --warmup such
groups; the median of --reps groups is reported with the smallest and the largest, per call. The legs of a part
alternate twice, so that none always has the warmer chip; the two medians are averaged, and their difference is the
spread a difference between legs has to exceed. Rates are the bytes named above over the time: achieved bytes per second
of the algorithm's traffic, not a counter reading. One 265 MB fine accumulator would nearly fit the 256 MiB Infinity
Cache, so the downsample legs read two of them in turn, the two the merge leg reads: every leg moves 531 MB between two
reads of the same byte. One JSON line; --out also writes it to a file.
Usage (GPU): python tools/supersample_bench.py [--reps 30] [--warmup 5] [--inner 10] [--render-reps 5] [--out profiles/supersample_bench.json]
A run without a GPU fails: nothing here is measured on the CPU."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FW, FH, PX = 3840, 2160, 32
KERNEL_CASES = [(1920, 1080, 2), (960, 540, 4)]  # output w, h, s: both read the FW x FH accumulator
RW, RH, SPP, BOUNCES, FRAMES, RS = 1920, 1080, 16, 8, 64, 2  # the render of (b)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--inner", type=int, default=10)
    p.add_argument("--render-reps", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("supersample_bench: no GPU")
    torch.cuda.init()
    rt4 = importlib.import_module("4d_ray_tracing_amd.rt4")
    stream = torch.cuda.current_stream()
    st = stream.cuda_stream

    def median_ms(fn, inner, warmup, reps):
        def group():
            for _ in range(inner):
                fn()

        for _ in range(warmup):
            group()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            group()
            e1.record(stream)
            e1.synchronize()
            times.append(e0.elapsed_time(e1) / inner)
        return statistics.median(times), min(times), max(times)

    def alternate(legs, inner, warmup, reps):
        """{name: [(median, min, max), (median, min, max)]}: every leg twice, in turn."""
        runs = {name: [] for name, _ in legs}
        for _ in range(2):
            for name, fn in legs:
                runs[name].append(median_ms(fn, inner, warmup, reps))
        torch.cuda.synchronize()
        return runs

    def report(result, runs, bytes_moved):
        for name, rs in runs.items():
            ms = sum(r[0] for r in rs) / len(rs)
            result[name + "_ms"] = round(ms, 4)
            result[name + "_ms_runs"] = [round(r[0], 4) for r in rs]
            result[name + "_ms_min_max"] = [round(min(r[1] for r in rs), 4), round(max(r[2] for r in rs), 4)]
            if name in bytes_moved:
                result[name + "_bytes"] = bytes_moved[name]
                result[name + "_gbytes_per_s"] = round(bytes_moved[name] / (ms * 1e-3) / 1e9, 1)

    result = {"fine_width": FW, "fine_height": FH, "reps": args.reps, "warmup": args.warmup, "inner": args.inner,
              "render_reps": args.render_reps}
    t = rt4.Tracer(device=0, flags=rt4.FLAG_SAMPLER_LUT)
    try:
        # ---- (a) the kernel next to the merge ----
        gen = torch.Generator(device="cuda").manual_seed(7)

        def accumulator(h, w):
            a = torch.rand((h, w, 8), generator=gen, device="cuda", dtype=torch.float32)
            a[..., 5] = torch.tensor(4, dtype=torch.int32).view(torch.float32)  # n = 4 frames
            a[..., 6:] = 0
            return a

        fine, dst = accumulator(FH, FW), accumulator(FH, FW)
        outs = {s: torch.zeros((h, w, 8), device="cuda", dtype=torch.float32) for w, h, s in KERNEL_CASES}
        for w, h, s in KERNEL_CASES:  # what is timed is the kernel the tests check: n' = 4 everywhere, reserved 0
            t.light_downsample_device(fine.data_ptr(), FW, outs[s].data_ptr(), w, w, h, s, st)
            torch.cuda.synchronize()
            o = outs[s].view(torch.int32)
            if not bool((o[..., 5] == 4).all()) or bool(o[..., 6:].any()):
                sys.exit("supersample_bench: unexpected output of the downsample")

        def merge_one():
            t.light_merge_device(dst.data_ptr(), FW, fine.data_ptr(), FW, FW * FH, 1, FW, FH, st)

        def downsample(w, h, s):
            turn = [0]

            def call():  # the two fine accumulators in turn: 531 MB between two reads of a byte, as in the merge leg
                turn[0] ^= 1
                t.light_downsample_device((fine, dst)[turn[0]].data_ptr(), FW, outs[s].data_ptr(), w, w, h, s, st)

            return call

        legs = [(f"downsample_s{s}", downsample(w, h, s)) for w, h, s in KERNEL_CASES] + [("merge_one_source", merge_one)]
        bytes_moved = {f"downsample_s{s}": PX * (s * s + 1) * w * h for w, h, s in KERNEL_CASES}
        bytes_moved["merge_one_source"] = 3 * PX * FW * FH
        runs = alternate(legs, args.inner, args.warmup, args.reps)
        report(result, runs, bytes_moved)
        result["outputs"] = {f"downsample_s{s}": [w, h] for w, h, s in KERNEL_CASES}
        result["copy_yardstick_gbytes_per_s"] = 6290.0  # the measured device copy rate of the MI355X guide, for scale
        del dst

        # ---- (a2) the same two kernels on four times the pixels: what of a difference is per call, what per byte ----
        bw, bh = 2 * FW, 2 * FH
        big = [accumulator(bh, bw) for _ in range(2)]
        big_out = torch.zeros((bh // 2, bw // 2, 8), device="cuda", dtype=torch.float32)
        turn = [0]

        def big_downsample():
            turn[0] ^= 1
            t.light_downsample_device(big[turn[0]].data_ptr(), bw, big_out.data_ptr(), bw // 2, bw // 2, bh // 2, 2, st)

        def big_merge():
            t.light_merge_device(big[1].data_ptr(), bw, big[0].data_ptr(), bw, bw * bh, 1, bw, bh, st)

        runs = alternate([("downsample_s2_4x", big_downsample), ("merge_one_source_4x", big_merge)], args.inner, args.warmup,
                         args.reps)
        report(result, runs, {"downsample_s2_4x": PX * 5 * (bw // 2) * (bh // 2), "merge_one_source_4x": 3 * PX * bw * bh})
        result["outputs"]["downsample_s2_4x"] = [bw // 2, bh // 2]
        del big, big_out

        # ---- (b) equal rays: 64 frames at the output resolution against 16 at twice the resolution + one downsample ----
        t.set_scene(rt4.Scene.builtin("sphere"))
        base = rt4.make_uniforms(RW, RH, samples=SPP, reflections=BOUNCES, seed=4321)
        fine_base = rt4.upscale_uniforms(base, RS)
        us = [rt4.progressive_uniforms(base, n) for n in range(1, FRAMES + 1)]
        fus = [rt4.progressive_uniforms(fine_base, n) for n in range(1, FRAMES // (RS * RS) + 1)]
        reg, freg = rt4.region(RW, RH), rt4.region(RW * RS, RH * RS)
        acc = torch.zeros((RH, RW, 8), device="cuda", dtype=torch.float32)
        cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        out = outs[RS]

        def plain():
            t.render_light_device(us, reg, acc.data_ptr(), RW, cnt[0:].data_ptr(), st)

        def supersampled():
            t.render_light_device(fus, freg, fine.data_ptr(), RW * RS, cnt[1:].data_ptr(), st)
            t.light_downsample_device(fine.data_ptr(), RW * RS, out.data_ptr(), RW, RW, RH, RS, st)

        fine.zero_()
        legs = [("render_plain", plain), ("render_supersampled", supersampled)]
        rruns = alternate(legs, 1, 1, args.render_reps)
        report(result, rruns, {})
        calls = 2 * (1 + args.render_reps)
        counts = [int(c) // calls for c in cnt.tolist()]
        result.update({"render": {"scene": "sphere", "width": RW, "height": RH, "samples": SPP, "bounces": BOUNCES,
                                  "plain_frames": FRAMES, "supersample": RS, "supersampled_frames": len(fus)},
                       "render_plain_intersections": counts[0], "render_supersampled_intersections": counts[1],
                       "render_supersampled_over_plain": round(result["render_supersampled_ms"] / result["render_plain_ms"], 4)})
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
