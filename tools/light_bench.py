#!/usr/bin/env python3
"""Times the light accumulator (rt4.h rt4_render_light_device, rt4_light_resolve_device, rt4_light_noise_device;
DESIGN.md §4.37) on the MI355X: the sphere scene at 1920 x 1080, 16 spp, 8 bounces, 20 progressive frames.

  light     rt4_render_light_device of the 20 frames into a light accumulator
  colour    rt4_render_frames_device of the same 20 frames into an fp32 frame, in the same process
  resolve   rt4_light_resolve_device of the accumulator into an fp32 frame
  noise     rt4_light_noise_device with both maps, the tile image and the statistics
  noise_stats_only  the same with every optional output NULL

Each call is timed alone between two device events on the stream after warm-up calls; the median of --reps
repetitions is reported. The two 20-frame calls differ only in their fold: light - colour is what the light fold
costs more than the colour fold (48 more state bytes per pixel). The folds themselves cannot be launched alone; their
own durations come from a kernel trace of this program (rocprofv3 --kernel-trace --stats -- python
tools/light_bench.py --reps 20) whose <name>_kernel_stats.csv is passed to a second, untraced run with --kernel-stats:
the light fold's average is then reported against the 16 * 20 + 64 B per pixel it must move, as a rate. Resolve moves
32 + 16 B per pixel, noise 32 + 4 + 4 B (32 B stats only). One JSON line; --out also writes it to a file.
There is no threshold: nothing was measured before this tool.
Usage (GPU): python tools/light_bench.py [--reps 30] [--warmup 5] [--kernel-stats CSV] [--out profiles/light_bench.json]
A run without a GPU fails: nothing here is measured on the CPU."""
import argparse
import csv
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE, W, H, SPP, BOUNCES, FRAMES = "sphere", 1920, 1080, 16, 8, 20
FOLD_BYTES_PER_PIXEL = 16 * FRAMES + 64
RESOLVE_BYTES_PER_PIXEL = 32 + 16
NOISE_BYTES_PER_PIXEL = 32 + 4 + 4


def kernel_averages(path):
    """{kernel name fragment: average ms} of the kernels of interest in a rocprofv3 kernel stats CSV."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for key in ("rt4_fold_light_kernel", "rt4_fold_frames_kernel", "rt4_light_resolve_kernel", "rt4_light_noise_kernel",
                        "rt4_trace_kernel"):
                if key in row["Name"]:
                    out[key] = (float(row["AverageNs"]) * 1e-6, int(row["Calls"]))
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--kernel-stats", default=None)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.reps < 20:
        p.error("--reps must be at least 20")
    import torch

    if not torch.cuda.is_available():
        sys.exit("light_bench: no GPU")
    torch.cuda.init()
    rt4 = importlib.import_module("4d_ray_tracing_amd.rt4")
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream

    def median_ms(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        return statistics.median(times), min(times), max(times)

    t = rt4.Tracer(device=0, flags=rt4.FLAG_SAMPLER_LUT, scene=rt4.Scene.named(SCENE))
    try:
        base = rt4.make_uniforms(W, H, samples=SPP, reflections=BOUNCES, seed=12345)
        us = [rt4.progressive_uniforms(base, n) for n in range(1, FRAMES + 1)]
        reg = rt4.region(W, H)
        k = base.light_to_color_conversion_coefficient
        light = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
        frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        image = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        se = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        q = torch.zeros((H, W), dtype=torch.float32, device="cuda")
        tiles = torch.zeros(((H + 7) // 8, (W + 7) // 8), dtype=torch.int32, device="cuda")
        stats = torch.zeros(4, dtype=torch.int64, device="cuda")
        t.reserve_frames(W, H)

        def light_run():
            t.render_light_device(us, reg, light.data_ptr(), W, 0, s)

        def colour_run():
            t.render_frames_device(us, reg, frame.data_ptr(), rt4.FRAME_RGBA32F, W, 0, s)

        def resolve():
            t.light_resolve_device(light.data_ptr(), W, k, image.data_ptr(), rt4.FRAME_RGBA32F, W, W, H, s)

        def noise():
            t.light_noise_device(light.data_ptr(), W, W, H, k, 1.0 / 255.0, se.data_ptr(), q.data_ptr(), W, tiles.data_ptr(),
                                 stats.data_ptr(), s)

        def noise_stats_only():
            t.light_noise_device(light.data_ptr(), W, W, H, k, 1.0 / 255.0, 0, 0, W, 0, stats.data_ptr(), s)

        # the two 20-frame calls in alternation, so that neither has the warmer chip
        l1 = median_ms(light_run)
        c1 = median_ms(colour_run)
        l2 = median_ms(light_run)
        c2 = median_ms(colour_run)
        l_ms, c_ms = (l1[0] + l2[0]) / 2, (c1[0] + c2[0]) / 2
        r_ms = median_ms(resolve)
        n_ms = median_ms(noise)
        o_ms = median_ms(noise_stats_only)
        torch.cuda.synchronize()
        st = stats.cpu().numpy()
        npx = W * H
        result = {
            "scene": SCENE, "width": W, "height": H, "samples": SPP, "bounces": BOUNCES, "frames": FRAMES, "reps": args.reps,
            "light_ms": round(l_ms, 4), "light_ms_runs": [round(l1[0], 4), round(l2[0], 4)],
            "light_ms_min_max": [round(min(l1[1], l2[1]), 4), round(max(l1[2], l2[2]), 4)],
            "colour_ms": round(c_ms, 4), "colour_ms_runs": [round(c1[0], 4), round(c2[0], 4)],
            "colour_ms_min_max": [round(min(c1[1], c2[1]), 4), round(max(c1[2], c2[2]), 4)],
            "light_minus_colour_ms": round(l_ms - c_ms, 4), "light_over_colour": round(l_ms / c_ms, 5),
            "resolve_ms": round(r_ms[0], 4), "resolve_ms_min_max": [round(r_ms[1], 4), round(r_ms[2], 4)],
            "resolve_gbytes_per_s": round(RESOLVE_BYTES_PER_PIXEL * npx / (r_ms[0] * 1e-3) / 1e9, 1),
            "noise_ms": round(n_ms[0], 4), "noise_ms_min_max": [round(n_ms[1], 4), round(n_ms[2], 4)],
            "noise_gbytes_per_s": round(NOISE_BYTES_PER_PIXEL * npx / (n_ms[0] * 1e-3) / 1e9, 1),
            "noise_stats_only_ms": round(o_ms[0], 4), "noise_stats_only_ms_min_max": [round(o_ms[1], 4), round(o_ms[2], 4)],
            "noise_stats": {"pixels": int(st[0]), "measured": int(st[1]), "above": int(st[2])},
            "accumulator_frames": int(light[0, 0, 5].view(torch.int32).item()),
            "fold_bytes": FOLD_BYTES_PER_PIXEL * npx, "build": rt4.lib.rt4_build_info().decode(),
        }
        if args.kernel_stats:
            for key, (ms, calls) in kernel_averages(args.kernel_stats).items():
                result[key + "_ms"] = round(ms, 4)
                result[key + "_calls"] = calls
            if "rt4_fold_light_kernel_ms" in result:
                result["fold_light_gbytes_per_s"] = round(FOLD_BYTES_PER_PIXEL * npx / (result["rt4_fold_light_kernel_ms"] * 1e-3) / 1e9, 1)
        line = json.dumps(result)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
    finally:
        t.close()


if __name__ == "__main__":
    main()
