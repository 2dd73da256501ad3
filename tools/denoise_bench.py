#!/usr/bin/env python3
"""Times the primary-hit G-buffer and the edge-stopping filter (rt4.h rt4_render_gbuffer_device, rt4_denoise_device;
DESIGN.md §4.33) on the MI355X, at the two frame sizes of the benchmark configs:

  config 2: the sphere scene at 1920 x 1080            config 4: tiger_two_mirrors at 3840 x 2160

fp32 frames, the default parameters (3 levels). Each call is timed alone between two device events on the stream after
warm-up launches; the median of --reps repetitions is reported. One JSON line per config:
  gbuffer_ms, denoise_ms, denoise_floor_bytes (per level: read 16 B colour + 32 B guide, write 16 B, per pixel),
  denoise_gbytes_per_s (that floor over the measured time), and per filter level count 1..3 the time, so that the
  cost of each stride shows (level 3's stride-4 pass gathers from global memory; strides 1 and 2 stage tiles in LDS).
The input frame is one rendered frame of the config's scene at 1 spp (the filter's time does not depend on the colours,
only on how many taps the guide lets through).
Usage (GPU): python tools/denoise_bench.py [--reps 30] [--warmup 5] [--configs 2 4]
A run without a GPU fails: nothing here is measured on the CPU."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {2: ("sphere", 1920, 1080), 4: ("tiger_two_mirrors", 3840, 2160)}  # bench.py CONFIGS: scene and frame size
FLOOR_BYTES_PER_PIXEL_LEVEL = 16 + 32 + 16


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--configs", type=int, nargs="+", default=[2, 4], choices=sorted(CONFIGS))
    args = p.parse_args()
    if args.reps < 20:
        p.error("--reps must be at least 20")
    import torch

    if not torch.cuda.is_available():
        sys.exit("denoise_bench: no GPU")
    torch.cuda.init()
    rt4 = importlib.import_module("4d_ray_tracing_amd.rt4")
    stream = torch.cuda.current_stream()

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

    for cfg in args.configs:
        name, w, h = CONFIGS[cfg]
        t = rt4.Tracer(device=0, flags=rt4.FLAG_SAMPLER_LUT, scene=rt4.Scene.named(name))
        try:
            u = rt4.make_uniforms(w, h, samples=1, reflections=4, seed=12345)
            reg = rt4.region(w, h)
            frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            out = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
            gbuf = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
            t.render_device_ex(u, reg, frame.data_ptr(), rt4.FRAME_RGBA32F, w, 0, stream.cuda_stream)
            torch.cuda.synchronize()

            def gbuffer():
                t.render_gbuffer_device(u, reg, gbuf.data_ptr(), w, stream.cuda_stream)

            def denoise(levels):
                prm = rt4.denoise_params(levels=levels)
                return lambda: t.denoise_device(frame.data_ptr(), w, out.data_ptr(), w, rt4.FRAME_RGBA32F, w, h, gbuf.data_ptr(),
                                                w, prm, stream.cuda_stream)

            g_ms = median_ms(gbuffer)
            by_levels = {levels: median_ms(denoise(levels)) for levels in (1, 2, 3)}
            surface = gbuf.cpu().numpy().view("int32")[..., 5]
            d_ms = by_levels[3][0]
            floor = 3 * FLOOR_BYTES_PER_PIXEL_LEVEL * w * h
            print(json.dumps({
                "config": cfg, "scene": name, "width": w, "height": h, "reps": args.reps,
                "gbuffer_ms": round(g_ms[0], 4), "gbuffer_ms_min_max": [round(g_ms[1], 4), round(g_ms[2], 4)],
                "denoise_ms": round(d_ms, 4), "denoise_ms_min_max": [round(by_levels[3][1], 4), round(by_levels[3][2], 4)],
                "denoise_ms_by_levels": {str(k): round(v[0], 4) for k, v in by_levels.items()},
                "denoise_floor_bytes": floor, "denoise_gbytes_per_s": round(floor / (d_ms * 1e-3) / 1e9, 1),
                "hit_fraction": round(float((surface >= 0).mean()), 4), "denoise_scratch_bytes": t.denoise_bytes(),
                "build": rt4.lib.rt4_build_info().decode(),
            }), flush=True)
        finally:
            t.close()


if __name__ == "__main__":
    main()
