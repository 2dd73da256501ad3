#!/usr/bin/env python3
"""Times adaptive light sampling (rt4.h rt4_light_select_tiles_device, rt4_render_light_tiles_device) on
the MI355X: the sphere scene at 1920 x 1080, 16 spp, 8 bounces, 20 progressive frames per call.

  full            rt4_render_light_device of the 20 frames, two legs
  tiles_100       rt4_render_light_tiles_device with every tile listed ascending, two legs, alternating with `full`: it
                  hands out the same items in the same order, so its time is compared with `full` in the same process;
                  the margin is the spread between the full call's own two legs
  tiles_50/10/1   the same with ascending lists of 50 %, 10 % and 1 % of the tiles, two kinds of list each:
                  `selected`: the selection's own list of an accumulator of 16 frames (threshold 1/255, no dilation, min_above
                  the quantile of the tiles' hot counts that gives that share; thinned evenly if ties make it longer),
                  `spread`: evenly spread tiles of the same length
  select, noise   rt4_light_select_tiles_device (default parameters, no state image) next to rt4_light_noise_device
                  (statistics and tile image only) on that accumulator: they read the same bytes

Each call is timed alone between two device events on the stream after warm-up calls; the median of --reps
repetitions is reported. One JSON line; --out also writes it to a file. There is no threshold: nothing was measured
before this tool.
Usage (GPU): python tools/adaptive_bench.py [--reps 30] [--warmup 5] [--out profiles/adaptive_bench.json]
A run without a GPU fails: nothing here is measured on the CPU."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE, W, H, SPP, BOUNCES, FRAMES, ACC_FRAMES = "sphere", 1920, 1080, 16, 8, 20, 16
SHARES = (50, 10, 1)


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.reps < 20:
        p.error("--reps must be at least 20")
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        sys.exit("adaptive_bench: no GPU")
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
        return statistics.median(times)

    t = rt4.Tracer(device=0, flags=rt4.FLAG_SAMPLER_LUT, scene=rt4.Scene.named(SCENE))
    try:
        base = rt4.make_uniforms(W, H, samples=SPP, reflections=BOUNCES, seed=12345)
        us = [rt4.progressive_uniforms(base, n) for n in range(1, FRAMES + 1)]
        reg = rt4.region(W, H)
        k = base.light_to_color_conversion_coefficient
        tx, ty = (W + 7) // 8, (H + 7) // 8
        tiles = tx * ty
        light = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")  # the accumulator the timed calls write
        acc = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")    # 16 frames: what selection and noise read
        d_list = torch.zeros(tiles, dtype=torch.int32, device="cuda")
        d_count = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_above = torch.zeros(tiles, dtype=torch.int32, device="cuda")
        stats = torch.zeros(4, dtype=torch.int64, device="cuda")
        t.reserve_frames(W, H)
        t.render_light_device(us[:ACC_FRAMES], reg, acc.data_ptr(), W, 0, s)
        t.light_noise_device(acc.data_ptr(), W, W, H, k, 1.0 / 255.0, 0, 0, W, d_above.data_ptr(), stats.data_ptr(), s)
        torch.cuda.synchronize()
        above = d_above.cpu().numpy()

        def tiles_run(lst):
            d = torch.from_numpy(np.ascontiguousarray(lst, np.uint32).view(np.int32)).cuda()
            return lambda: t.render_light_tiles_device(us, reg, d.data_ptr(), len(lst), light.data_ptr(), W, 0, s)

        def full_run():
            t.render_light_device(us, reg, light.data_ptr(), W, 0, s)

        every = tiles_run(np.arange(tiles))
        f1 = median_ms(full_run)
        a1 = median_ms(every)
        f2 = median_ms(full_run)
        a2 = median_ms(every)
        full_ms, all_ms = (f1 + f2) / 2, (a1 + a2) / 2
        result = {
            "scene": SCENE, "width": W, "height": H, "samples": SPP, "bounces": BOUNCES, "frames": FRAMES, "reps": args.reps,
            "tiles": tiles, "full_ms": round(full_ms, 4), "full_ms_runs": [round(f1, 4), round(f2, 4)],
            "tiles_100_ms": round(all_ms, 4), "tiles_100_ms_runs": [round(a1, 4), round(a2, 4)],
            "tiles_100_over_full": round(all_ms / full_ms, 5), "full_legs_spread": round(abs(f1 - f2) / full_ms, 5),
        }
        for share in SHARES:
            n = max(1, tiles * share // 100)
            # the selection's own list: the threshold on the hot count that leaves about n tiles, through the library
            order = np.sort(above)[::-1]
            sel = rt4.tile_select_params(threshold=1.0 / 255.0, min_above=max(1, min(64, int(order[n - 1]))), min_frames=0, dilate=0)
            t.light_select_tiles_device(acc.data_ptr(), W, W, H, k, sel, d_list.data_ptr(), d_count.data_ptr(), 0, s)
            torch.cuda.synchronize()
            count = int(d_count.cpu().numpy().view(np.uint32)[0])
            selected = d_list.cpu().numpy().view(np.uint32)[:count]
            if count > n:  # ties at the threshold: an evenly thinned, still ascending part of the list
                selected = selected[np.linspace(0, count - 1, n).astype(np.int64)]
            spread = np.linspace(0, tiles - 1, len(selected)).astype(np.uint32)
            ms_sel, ms_spread = median_ms(tiles_run(selected)), median_ms(tiles_run(spread))
            result[f"tiles_{share}"] = {"listed": int(len(selected)), "selected_ms": round(ms_sel, 4), "spread_ms": round(ms_spread, 4),
                                        "selected_over_full": round(ms_sel / full_ms, 5),
                                        "spread_over_full": round(ms_spread / full_ms, 5)}
        defaults = rt4.tile_select_params()

        def select():
            t.light_select_tiles_device(acc.data_ptr(), W, W, H, k, defaults, d_list.data_ptr(), d_count.data_ptr(), 0, s)

        def noise():
            t.light_noise_device(acc.data_ptr(), W, W, H, k, 1.0 / 255.0, 0, 0, W, d_above.data_ptr(), stats.data_ptr(), s)

        result["select_ms"] = round(median_ms(select), 4)
        result["noise_ms"] = round(median_ms(noise), 4)
        torch.cuda.synchronize()
        result["select_default_count"] = int(d_count.cpu().numpy().view(np.uint32)[0])
        result["select_bytes"] = t.select_bytes()
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
