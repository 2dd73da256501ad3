#!/usr/bin/env python3
"""Times the variance-guided filter of a light accumulator (rt4.h rt4_light_denoise_device) on the
MI355X: the sphere scene at 1920 x 1080, fp32 frames, on an accumulator of 20 progressive frames of 16 spp, 8 bounces.

  light_denoise_3, light_denoise_5  rt4_light_denoise_device at 3 and at 5 (the default) levels, d_filtered NULL
  light_denoise_5_filtered          the default with d_filtered given
  light_denoise_0                   no levels: the plain resolve through this entry point
  denoise                           rt4_denoise_device at its defaults (3 levels) on the resolved frame, same G-buffer
  frame                             one 16-spp rt4_render_device_ex frame of the same view

Each call is timed alone between two device events on the stream after --warmup calls, all in one process; the median
of --reps repetitions is reported with the smallest and the largest. For each level count: the time, the rate at which
the floor traffic (64 B per pixel and level: 44 B of state and guide read, 20 B of state written; the pack pass and the
neighbours' reads are on top) would have moved in that time, and the time per level over the colour filter's time per
level. The one condition: the default call costs less than the 16-spp frame measured beside it (otherwise rendering
another frame is the better use of the time); `default_cheaper_than_frame` says so and the exit status is 1 if not.
One JSON line; --out also writes it to a file.
Usage (GPU): python tools/light_denoise_bench.py [--reps 30] [--warmup 5] [--out profiles/light_denoise_bench.json]
A run without a GPU fails: nothing here is measured on the CPU."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE, W, H, SPP, BOUNCES, FRAMES = "sphere", 1920, 1080, 16, 8, 20
FLOOR_BYTES_PER_PIXEL_AND_LEVEL = 64


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("light_denoise_bench: no GPU")
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
        one = rt4.progressive_uniforms(base, 1)
        one.part = 1.0
        reg = rt4.region(W, H)
        k = base.light_to_color_conversion_coefficient
        light = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
        gbuf = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
        resolved = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        image = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        filtered = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        t.reserve_frames(W, H)
        t.render_light_device(us, reg, light.data_ptr(), W, 0, s)
        t.render_gbuffer_device(base, reg, gbuf.data_ptr(), W, s)
        t.light_resolve_device(light.data_ptr(), W, k, resolved.data_ptr(), rt4.FRAME_RGBA32F, W, W, H, s)
        torch.cuda.synchronize()

        def light_denoise(levels, fl=0):
            p_ = rt4.light_denoise_params(levels=levels)
            return lambda: t.light_denoise_device(light.data_ptr(), W, gbuf.data_ptr(), W, k, image.data_ptr(), rt4.FRAME_RGBA32F,
                                                  W, W, H, p_, fl, W, s)

        def denoise():
            t.denoise_device(resolved.data_ptr(), W, image.data_ptr(), W, rt4.FRAME_RGBA32F, W, H, gbuf.data_ptr(), W, None, s)

        def one_frame():
            t.render_device_ex(one, reg, frame.data_ptr(), rt4.FRAME_RGBA32F, W, 0, s)

        # twice each, in alternation, so that no call always has the warmer chip; the two medians are averaged
        order = [("light_denoise_3", light_denoise(3)), ("light_denoise_5", light_denoise(5)), ("denoise", denoise),
                 ("frame", one_frame), ("light_denoise_5_filtered", light_denoise(5, filtered.data_ptr())),
                 ("light_denoise_0", light_denoise(0))]
        runs = {name: [] for name, _ in order}
        for _ in range(2):
            for name, fn in order:
                runs[name].append(median_ms(fn))
        torch.cuda.synchronize()
        ms = {name: sum(r[0] for r in rs) / len(rs) for name, rs in runs.items()}
        npx = W * H
        colour_levels = rt4.denoise_params().levels
        result = {"scene": SCENE, "width": W, "height": H, "samples": SPP, "bounces": BOUNCES, "accumulator_frames":
                  int(light[0, 0, 5].view(torch.int32).item()), "reps": args.reps, "warmup": args.warmup,
                  "hit_pixels": int((gbuf[..., 5].view(torch.int32) >= 0).sum().item())}
        for name, rs in runs.items():
            result[name + "_ms"] = round(ms[name], 4)
            result[name + "_ms_runs"] = [round(r[0], 4) for r in rs]
            result[name + "_ms_min_max"] = [round(min(r[1] for r in rs), 4), round(max(r[2] for r in rs), 4)]
        result["denoise_levels"] = colour_levels
        result["denoise_ms_per_level"] = round(ms["denoise"] / colour_levels, 4)
        for levels in (3, 5):
            key = f"light_denoise_{levels}"
            floor = FLOOR_BYTES_PER_PIXEL_AND_LEVEL * npx * levels
            result[key + "_floor_bytes"] = floor
            result[key + "_floor_gbytes_per_s"] = round(floor / (ms[key] * 1e-3) / 1e9, 1)
            result[key + "_ms_per_level"] = round(ms[key] / levels, 4)
            result[key + "_per_level_over_denoise_per_level"] = round((ms[key] / levels) / (ms["denoise"] / colour_levels), 3)
        result["default_over_frame"] = round(ms["light_denoise_5"] / ms["frame"], 3)
        result["default_cheaper_than_frame"] = bool(ms["light_denoise_5"] < ms["frame"])
        result["light_denoise_bytes"] = t.light_denoise_bytes()
        result["build"] = rt4.lib.rt4_build_info().decode()
        line = json.dumps(result)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
    finally:
        t.close()
    sys.exit(0 if result["default_cheaper_than_frame"] else 1)


if __name__ == "__main__":
    main()
