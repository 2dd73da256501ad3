#!/usr/bin/env python3
"""Times temporal reprojection (rt4.h rt4_reproject_device, rt4_temporal_blend_device, rt4_temporal_frame_device;
DESIGN.md §4.34) on the MI355X: the sphere scene at 1920 x 1080, fp32 frames, the default parameters.

  reproject   the image and history of the default camera carried into the view 0.05 to the right
  blend       one sample frame blended into the accumulator
  moving      a whole rt4_temporal_frame_device frame at 1 spp whose pose differs from the previous frame's (the camera
              alternates between the two poses): G-buffer + reprojection + render + blend
  resting     the same with the pose unchanged: render + blend
  plain       one rt4_render_device_ex frame of the same shape at 1 spp: what a frame costs without any of this

Each call is timed alone between two device events on the stream after warm-up launches; the median of --reps
repetitions is reported. The bytes a pass must move count every image once: reprojection reads both G-buffers (32 B),
the old colour (16 B) and history (4 B) and writes colour and history (104 B per pixel); the blend reads the sample
and reads and writes accumulator and history (56 B per pixel). One JSON line; --out also writes it to a file.
There is no threshold: nothing was measured before this tool.
Usage (GPU): python tools/temporal_bench.py [--reps 30] [--warmup 5] [--out profiles/temporal_bench.json]
A run without a GPU fails: nothing here is measured on the CPU."""
import argparse
import importlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENE, W, H = "sphere", 1920, 1080
REPROJECT_BYTES_PER_PIXEL = 32 + 32 + 16 + 4 + 16 + 4
BLEND_BYTES_PER_PIXEL = 16 + 16 + 16 + 4 + 4


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
        sys.exit("temporal_bench: no GPU")
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
    temporal = None
    try:
        u_a = rt4.make_uniforms(W, H, samples=1, reflections=4, seed=12345)
        u_b = rt4.make_uniforms(W, H, samples=1, reflections=4, seed=12345, focus=(0.05, -2.0, 0.0, 0.0))
        reg = rt4.region(W, H)
        frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        acc_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        hist = torch.full((H, W), 8, dtype=torch.int32, device="cuda")
        hist_out = torch.zeros((H, W), dtype=torch.int32, device="cuda")
        g_a = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
        g_b = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
        t.render_device_ex(u_a, reg, frame.data_ptr(), rt4.FRAME_RGBA32F, W, 0, s)
        t.render_device_ex(u_a, reg, acc.data_ptr(), rt4.FRAME_RGBA32F, W, 0, s)
        t.render_gbuffer_device(u_a, reg, g_a.data_ptr(), W, s)
        t.render_gbuffer_device(u_b, reg, g_b.data_ptr(), W, s)
        torch.cuda.synchronize()
        prm = rt4.reproject_params()

        def reproject():
            t.reproject_device(u_b, g_b.data_ptr(), W, u_a, g_a.data_ptr(), W, acc.data_ptr(), W, hist.data_ptr(), W,
                               acc_out.data_ptr(), W, hist_out.data_ptr(), W, rt4.FRAME_RGBA32F, W, H, prm, s)

        def blend():
            t.temporal_blend_device(frame.data_ptr(), W, acc.data_ptr(), W, rt4.FRAME_RGBA32F, hist.data_ptr(), W, W, H, s)

        def plain():
            t.render_device_ex(u_a, reg, frame.data_ptr(), rt4.FRAME_RGBA32F, W, 0, s)

        r_ms = median_ms(reproject)
        kept = float((hist_out > 0).float().mean().item())
        b_ms = median_ms(blend)
        p_ms = median_ms(plain)
        temporal = rt4.Temporal(t, W, H, rt4.FRAME_RGBA32F)
        temporal.frame(u_a, None, 0, s)
        flip = [0]

        def moving():
            flip[0] ^= 1
            temporal.frame(u_b if flip[0] else u_a, None, 0, s)

        def resting():
            temporal.frame(u_b if flip[0] else u_a, None, 0, s)

        m_ms = median_ms(moving)
        s_ms = median_ms(resting)
        npx = W * H
        result = {
            "scene": SCENE, "width": W, "height": H, "format": "f32", "samples": 1, "reps": args.reps,
            "reproject_ms": round(r_ms[0], 4), "reproject_ms_min_max": [round(r_ms[1], 4), round(r_ms[2], 4)],
            "reproject_bytes": REPROJECT_BYTES_PER_PIXEL * npx,
            "reproject_gbytes_per_s": round(REPROJECT_BYTES_PER_PIXEL * npx / (r_ms[0] * 1e-3) / 1e9, 1),
            "reproject_kept_fraction": round(kept, 4),
            "blend_ms": round(b_ms[0], 4), "blend_ms_min_max": [round(b_ms[1], 4), round(b_ms[2], 4)],
            "blend_bytes": BLEND_BYTES_PER_PIXEL * npx,
            "blend_gbytes_per_s": round(BLEND_BYTES_PER_PIXEL * npx / (b_ms[0] * 1e-3) / 1e9, 1),
            "moving_frame_ms": round(m_ms[0], 4), "moving_frame_ms_min_max": [round(m_ms[1], 4), round(m_ms[2], 4)],
            "resting_frame_ms": round(s_ms[0], 4), "resting_frame_ms_min_max": [round(s_ms[1], 4), round(s_ms[2], 4)],
            "plain_frame_ms": round(p_ms[0], 4), "plain_frame_ms_min_max": [round(p_ms[1], 4), round(p_ms[2], 4)],
            "moving_overhead_ms": round(m_ms[0] - p_ms[0], 4),
            "temporal_bytes": temporal.bytes(), "build": rt4.lib.rt4_build_info().decode(),
        }
        line = json.dumps(result)
        print(line, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
    finally:
        if temporal is not None:
            temporal.close()
        t.close()


if __name__ == "__main__":
    main()
