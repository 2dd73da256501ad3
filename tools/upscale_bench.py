#!/usr/bin/env python3
"""Times the window-resolution output (rt4.h rt4_upscale_device, rt4_window_present_device) on the
MI355X: the sphere scene, fp32 frames, the default parameters, at two shapes: the properties' main window (121 x 75
cells, scale 7: 847 x 525 pixels) and 480 x 270 cells at scale 4 (1920 x 1080).

  gbuffer_window   rt4_render_gbuffer_device at window resolution
  guided           rt4_upscale_device, RT4_UPSCALE_GUIDED
  nearest          rt4_upscale_device, RT4_UPSCALE_NEAREST (the reference's block stretch)
  moving           a whole rt4_window_present_device whose pose differs from the previous present's (the camera
                   alternates between two poses): both G-buffers + the guided upscale
  resting          the same with the pose unchanged: the guided upscale alone
  cell_frame       one 16-spp rt4_render_device_ex frame at cell resolution
  window_frame     one 16-spp rt4_render_device_ex frame at window resolution: what the window costs traced in full

Each call is timed alone between two device events on the stream after warm-up launches; the median of --reps
repetitions is reported. The bytes a pass must move count every image once: the window G-buffer writes 32 B per window
pixel; the guided upscale reads the window G-buffer (32 B) and writes the colour (16 B) per window pixel and reads the
cell's G-buffer record and colour (48 B) per cell; nearest writes 16 B per window pixel and reads 16 B per cell.
ratio = (cell_frame + moving) / window_frame: below 1 the cell frame presented at window resolution is cheaper than
tracing the window. One JSON line; --out also writes it to a file. There is no threshold on the times: nothing was
measured before this tool.
Usage (GPU): python tools/upscale_bench.py [--reps 30] [--warmup 5] [--out profiles/upscale_bench.json]
A run without a GPU fails: nothing here is measured on the CPU."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE, SAMPLES = "sphere", 16
SHAPES = [("main_window", 121, 75, 7), ("1080p", 480, 270, 4)]  # name, cells_w, cells_h, scale


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    if args.reps < 20:
        p.error("--reps must be at least 20")
    import torch

    if not torch.cuda.is_available():
        sys.exit("upscale_bench: no GPU")
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
    shapes = {}
    try:
        for name, cw, ch, scale in SHAPES:
            W, H = cw * scale, ch * scale
            u_a = rt4.make_uniforms(cw, ch, samples=SAMPLES, reflections=4, seed=12345)
            u_b = rt4.make_uniforms(cw, ch, samples=SAMPLES, reflections=4, seed=12345, focus=(0.05, -2.0, 0.0, 0.0))
            uw = rt4.upscale_uniforms(u_a, scale)
            reg_c, reg_w = rt4.region(cw, ch), rt4.region(W, H)
            cells = torch.zeros((ch, cw, 4), dtype=torch.float32, device="cuda")
            frame_w = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
            out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
            g_c = torch.zeros((ch, cw, 8), dtype=torch.float32, device="cuda")
            g_w = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
            t.render_device_ex(u_a, reg_c, cells.data_ptr(), rt4.FRAME_RGBA32F, cw, 0, s)
            t.render_gbuffer_device(u_a, reg_c, g_c.data_ptr(), cw, s)
            t.render_gbuffer_device(uw, reg_w, g_w.data_ptr(), W, s)
            torch.cuda.synchronize()
            guided_p, nearest_p = rt4.upscale_params(), rt4.upscale_params(mode=rt4.UPSCALE_NEAREST)

            def gbuffer_window():
                t.render_gbuffer_device(uw, reg_w, g_w.data_ptr(), W, s)

            def guided():
                t.upscale_device(u_a, scale, cells.data_ptr(), cw, g_c.data_ptr(), cw, g_w.data_ptr(), W, out.data_ptr(), W,
                                 rt4.FRAME_RGBA32F, cw, ch, guided_p, s)

            def nearest():
                t.upscale_device(u_a, scale, cells.data_ptr(), cw, 0, cw, 0, W, out.data_ptr(), W, rt4.FRAME_RGBA32F, cw, ch,
                                 nearest_p, s)

            def cell_frame():
                t.render_device_ex(u_a, reg_c, cells.data_ptr(), rt4.FRAME_RGBA32F, cw, 0, s)

            def window_frame():
                t.render_device_ex(uw, reg_w, frame_w.data_ptr(), rt4.FRAME_RGBA32F, W, 0, s)

            ms = {"gbuffer_window": median_ms(gbuffer_window), "guided": median_ms(guided), "nearest": median_ms(nearest)}
            window = rt4.Window(t, cw, ch, scale, rt4.FRAME_RGBA32F)
            try:
                window.present(u_a, cells.data_ptr(), stream=s)
                flip = [0]

                def moving():
                    flip[0] ^= 1
                    window.present(u_b if flip[0] else u_a, cells.data_ptr(), stream=s)

                def resting():
                    window.present(u_b if flip[0] else u_a, cells.data_ptr(), stream=s)

                ms["moving"] = median_ms(moving)
                ms["resting"] = median_ms(resting)
                window_bytes = window.bytes()
            finally:
                window.close()
            ms["cell_frame"] = median_ms(cell_frame)
            ms["window_frame"] = median_ms(window_frame)
            npx, ncells = W * H, cw * ch
            floor = {"gbuffer_window": 32 * npx, "guided": 48 * npx + 48 * ncells, "nearest": 16 * npx + 16 * ncells}
            entry = {"cells": [cw, ch], "scale": scale, "window": [W, H], "window_bytes": window_bytes}
            for k, (med, lo, hi) in ms.items():
                entry[k + "_ms"] = round(med, 4)
                entry[k + "_ms_min_max"] = [round(lo, 4), round(hi, 4)]
            for k, b in floor.items():
                entry[k + "_bytes"] = b
                entry[k + "_gbytes_per_s"] = round(b / (ms[k][0] * 1e-3) / 1e9, 1)
            entry["ratio_cell_frame_plus_moving_over_window_frame"] = round((ms["cell_frame"][0] + ms["moving"][0]) / ms["window_frame"][0], 4)
            shapes[name] = entry
        result = {"scene": SCENE, "format": "f32", "samples": SAMPLES, "reps": args.reps, "shapes": shapes,
                  "build": rt4.lib.rt4_build_info().decode()}
        line = json.dumps(result)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
    finally:
        t.close()


if __name__ == "__main__":
    main()
