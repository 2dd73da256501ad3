#!/usr/bin/env python3
"""Times the 3D retina view (rt4.h rt4_retina) on the MI355X: the default window's retina, 121 x 75
cells x 64 slices, projected to the window's 847 x 525 pixels, fp32 frames, on the scenes `sphere` and `tiger` at the
properties' 100 samples and 4 bounces.

  voxelize             (a) rt4_retina_voxelize_device of the whole volume
  project_yaw0         (b) rt4_retina_project_device, the rays along the slices' axis (yaw 0, pitch 0)
  project_yaw30        (b) the same at yaw 30 degrees, pitch 20 degrees: the view rt4_render --retina writes by default
  accumulate_frame     (c) one more frame of the volume, rt4_retina_accumulate_device: one launch per slice
  light_frame_121x4800 (d) one frame of rt4_render_light_device on a single 121 x 4800 image of the same scene and
                           camera: the volume's pixel count (64 x 75 rows) in one launch

Each call is timed alone between two device events on the stream after --warmup calls, all in one process; every call
runs in two rounds in alternation with the others, so that none always has the warmer chip. Reported per call: the mean
of the two rounds' medians of --reps repetitions, both medians, and the smallest and largest single time. The ratios
project / accumulate_frame say what another view of an accumulated volume costs against another frame of it;
accumulate_frame / light_frame_121x4800 is what batching the slices into one launch would be worth. No threshold: the
parent has nothing of this to compare with. One JSON line; --out also writes it to a file.
Usage (GPU): python tools/retina_bench.py [--reps 20] [--warmup 3] [--out profiles/retina_bench.json]
A run without a GPU fails: nothing here is measured on the CPU."""
import argparse
import importlib
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = ("sphere", "tiger")
W, H, D, SCALE, SPP, BOUNCES = 121, 75, 64, 7, 100, 4
TALL = H * D  # 4800 rows: the volume's pixels as one image


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("retina_bench: no GPU")
    torch.cuda.init()
    rt4 = importlib.import_module("4d_ray_tracing_amd.rt4")
    stream = torch.cuda.current_stream()
    s = stream.cuda_stream
    ow, oh = W * SCALE, H * SCALE

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

    result = {"width": W, "height": H, "depth": D, "out_width": ow, "out_height": oh, "samples": SPP, "bounces": BOUNCES,
              "reps": args.reps, "warmup": args.warmup, "voxel_volume_bytes": W * H * D * 16, "scenes": {}}
    for scene in SCENES:
        t = rt4.Tracer(device=0, flags=rt4.FLAG_SAMPLER_LUT, scene=rt4.Scene.named(scene))
        ret = rt4.Retina(t, W, H, D)
        try:
            u = rt4.make_uniforms(W, H, samples=SPP, reflections=BOUNCES, seed=12345)
            w_drct = rt4.Orientation(0.0, 0.0, 0.0).w_drct
            ds = float(u.mtr_sizes[1])
            k = float(u.light_to_color_conversion_coefficient)
            box = (float(u.mtr_sizes[0]), float(u.mtr_sizes[1]), ds)
            params = rt4.retina_params()
            views = {"project_yaw0": rt4.retina_view(W, H, D, box, 0.0, 0.0, 0.0, ow, oh, 1.0),
                     "project_yaw30": rt4.retina_view(W, H, D, box, math.radians(30), math.radians(20), 0.0, ow, oh, 1.0)}
            frame = torch.zeros((oh, ow, 4), dtype=torch.float32, device="cuda")
            tall = torch.zeros((TALL, W, 8), dtype=torch.float32, device="cuda")
            u_tall = rt4.make_uniforms(W, TALL, samples=SPP, reflections=BOUNCES, seed=12345)
            reg_tall = rt4.region(W, TALL)
            t.reserve_frames(W, TALL)
            ret.accumulate(u, w_drct, ds, 2, stream=s)  # the G-buffer volume and two frames: what the views show
            ret.present(views["project_yaw30"], k, frame.data_ptr(), rt4.FRAME_RGBA32F, ow, oh, params=params, stream=s)
            torch.cuda.synchronize()
            st = (W, W * H)
            frame_no = [0]

            def voxelize():
                t.retina_voxelize_device(ret.light_ptr(), st, ret.gbuffer_ptr(), st, k, params, ret.voxels_ptr(), st, W, H, D, s)

            def project(view):
                return lambda: t.retina_project_device(ret.voxels_ptr(), st, W, H, D, view, params, frame.data_ptr(),
                                                       rt4.FRAME_RGBA32F, ow, ow, oh, s)

            def accumulate_frame():
                ret.accumulate(u, w_drct, ds, 1, stream=s)

            def light_frame():
                frame_no[0] += 1
                t.render_light_device([rt4.progressive_uniforms(u_tall, frame_no[0])], reg_tall, tall.data_ptr(), W, 0, s)

            order = [("voxelize", voxelize), ("project_yaw0", project(views["project_yaw0"])), ("accumulate_frame", accumulate_frame),
                     ("project_yaw30", project(views["project_yaw30"])), ("light_frame_121x4800", light_frame)]
            runs = {name: [] for name, _ in order}
            for _ in range(2):
                for name, fn in order:
                    runs[name].append(median_ms(fn))
            torch.cuda.synchronize()
            ms = {name: sum(r[0] for r in rs) / len(rs) for name, rs in runs.items()}
            r = {"frames_accumulated": ret.frames_done(), "steps_yaw0": views["project_yaw0"].steps,
                 "steps_yaw30": views["project_yaw30"].steps}
            for name, rs in runs.items():
                r[name + "_ms"] = round(ms[name], 4)
                r[name + "_ms_runs"] = [round(x[0], 4) for x in rs]
                r[name + "_ms_min_max"] = [round(min(x[1] for x in rs), 4), round(max(x[2] for x in rs), 4)]
            for name in ("project_yaw0", "project_yaw30"):
                r[name + "_over_accumulate_frame"] = round(ms[name] / ms["accumulate_frame"], 4)
            r["accumulate_frame_over_light_frame"] = round(ms["accumulate_frame"] / ms["light_frame_121x4800"], 3)
            r["voxelize_gbytes_per_s"] = round(W * H * D * (32 + 32 + 16) / (ms["voxelize"] * 1e-3) / 1e9, 1)
            result["scenes"][scene] = r
        finally:
            ret.close()
            t.close()
    result["build"] = rt4.lib.rt4_build_info().decode()
    line = json.dumps(result)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
