"""rt4_render --light --adaptive: the host program's adaptive loop against Tracer.render_light_adaptive,
the same loop from Python: the same images and the same per-pass log; with -3; and the combinations it refuses."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SECTION_TAGS = ("yxz", "ywz", "yxw")


def render_paths(rt4):
    lib_dir = os.path.dirname(rt4.LIB_PATH)
    return os.path.join(lib_dir, "rt4_render"), os.path.join(lib_dir, "..", "..", "properties.txt")


def quick_properties(rt4, tmp_path, samples=8):
    """The repository's properties with fewer samples per frame (the loop is the same; the test stays quick)."""
    _, props_path = render_paths(rt4)
    text = re.sub(r"ray_tracing\.samples\s*=\s*\d+", f"ray_tracing.samples = {samples}", open(props_path).read())
    path = str(tmp_path / "properties.txt")
    open(path, "w").write(text)
    return path


def cli_log(stdout, tag):
    return [(m.group(1), int(m.group(2)), int(m.group(3)))
            for m in re.finditer(rf"adaptive {tag}: (\w+) tiles (\d+) frames (\d+)", stdout)]


def python_run(rt4, tracer, props_path, scene, section, w, h, seed, budget, select, warmup, pass_frames, full_every):
    props = rt4.Properties(path=props_path)
    base = rt4.uniforms_from_properties(props, w, h, section)
    ub = rt4.Camera(props).frame_uniforms(base, section, seed)
    tracer.set_scene(rt4.Scene.builtin(scene))
    return tracer.render_light_adaptive(ub, w, h, budget, select, warmup, pass_frames, full_every), ub


def check_section(rt4, tracer, tmp_path, pre, tag, stdout, acc, log, ub):
    assert cli_log(stdout, tag) == log, (tag, stdout)
    k = ub.light_to_color_conversion_coefficient
    rt4.write_ppm(str(tmp_path / "py.ppm"), tracer.light_resolve_host(acc, k))
    assert open(str(tmp_path / "py.ppm"), "rb").read() == open(f"{pre}_{tag}.ppm", "rb").read(), tag
    h, w = acc.shape
    grey = np.ones((h, w, 4), np.float32)
    grey[..., :3] = (acc["n"].astype(np.float32) / np.float32(acc["n"].max()))[..., None]
    rt4.write_ppm(str(tmp_path / "py_n.ppm"), grey)
    assert open(str(tmp_path / "py_n.ppm"), "rb").read() == open(f"{pre}_{tag}_n.ppm", "rb").read(), tag
    m = re.search(rf"adaptive {tag}: n min (\d+), median (\d+), max (\d+)", stdout)
    n_sorted = np.sort(acc["n"].reshape(-1))
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (n_sorted[0], n_sorted[len(n_sorted) // 2], n_sorted[-1])
    assert f"noise {tag}: pixels {w * h}" in stdout


def test_cpp_host_adaptive(rt4, tracer_lut, tmp_path):
    """-s sphere at 48 x 32, a budget of 12 frames, a warm-up of 4, passes of 2, a whole frame every third pass,
    min_above 2, no dilation: the images, the n image and the log are the Python loop's."""
    exe, _ = render_paths(rt4)
    props_path = quick_properties(rt4, tmp_path)
    seed, budget, w, h = 4321, 12, 48, 32
    pre = str(tmp_path / "a")
    r = subprocess.run([exe, "-p", props_path, "-s", "sphere", "-W", str(w), "-H", str(h), "-n", str(budget), "--seed", str(seed),
                        "--light", "--adaptive", "--adaptive-warmup", "4", "--adaptive-pass", "2", "--adaptive-full-every", "3",
                        "--adaptive-min-above", "2", "--adaptive-dilate", "0", "--noise-threshold", "0.01", "-o", pre],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    sel = rt4.tile_select_params(threshold=0.01, min_above=2, dilate=0)
    (acc, _, log), ub = python_run(rt4, tracer_lut, props_path, "sphere", rt4.SECTION_YXZ, w, h, seed, budget, sel, 4, 2, 3)
    tiles = 6 * 4
    assert log[0] == ("warmup", tiles, 4) and any(kind == "tiles" and 0 < n < tiles for kind, n, _ in log)
    assert any(kind == "full" for kind, _, _ in log)
    assert budget * tiles - tiles < sum(n * f for _, n, f in log) <= budget * tiles
    assert acc["n"].min() >= 4 and acc["n"].max() > budget  # the sky keeps the floor; the noisy tiles got more
    check_section(rt4, tracer_lut, tmp_path, pre, "yxz", r.stdout, acc, log, ub)


def test_cpp_host_adaptive_three_sections_defaults(rt4, tracer_lut, tmp_path):
    """-3 with every default: each section runs its own loop."""
    exe, _ = render_paths(rt4)
    props_path = quick_properties(rt4, tmp_path, samples=4)
    seed, budget = 99, 14
    pre = str(tmp_path / "t")
    r = subprocess.run([exe, "-p", props_path, "-s", "tiger", "-3", "-W", "40", "-H", "24", "-n", str(budget), "--seed", str(seed),
                        "--light", "--adaptive", "-o", pre], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    props = rt4.Properties(path=props_path)
    aw, ah = rt4.window_cells(props, "additional")
    sizes = [(40, 24), (aw, ah), (aw, ah)]
    sections = [rt4.SECTION_YXZ, rt4.SECTION_YWZ, rt4.SECTION_YXW]
    for tag, section, (w, h) in zip(SECTION_TAGS, sections, sizes):
        (acc, _, log), ub = python_run(rt4, tracer_lut, props_path, "tiger", section, w, h, seed, budget, None,
                                       rt4.ADAPTIVE_WARMUP, rt4.ADAPTIVE_PASS_FRAMES, rt4.ADAPTIVE_FULL_EVERY)
        assert log[0][0] == "warmup" and log[0][2] == rt4.ADAPTIVE_WARMUP and len(log) > 1
        check_section(rt4, tracer_lut, tmp_path, pre, tag, r.stdout, acc, log, ub)


@pytest.mark.parametrize("extra", [["--reproject"], ["--resume", "none.ckpt"], ["--checkpoint", "c.ckpt"], ["--gpus", "2"],
                                   ["--frame-by-frame"]], ids=lambda e: e[0])
def test_cpp_host_adaptive_refuses_what_light_refuses(rt4, tmp_path, extra):
    exe, props_path = render_paths(rt4)
    r = subprocess.run([exe, "-p", props_path, "-s", "sphere", "-W", "16", "-H", "8", "--light", "--adaptive", "-o",
                        str(tmp_path / "x")] + extra, capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode != 0 and "--light" in r.stderr, (extra, r.stderr)


@pytest.mark.parametrize("args", [["--adaptive"], ["--adaptive-pass", "2"], ["--light", "--adaptive-pass", "2"],
                                  ["--light", "--adaptive", "--adaptive-pass", "0"],
                                  ["--light", "--adaptive", "--adaptive-min-above", "65"],
                                  ["--light", "--adaptive", "--adaptive-dilate", "3"],
                                  ["--light", "--adaptive", "--adaptive-warmup", "-1"]], ids=lambda a: " ".join(a))
def test_cpp_host_adaptive_refusals(rt4, tmp_path, args):
    exe, props_path = render_paths(rt4)
    r = subprocess.run([exe, "-p", props_path, "-s", "sphere", "-W", "16", "-H", "8", "-o", str(tmp_path / "x")] + args,
                       capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode != 0 and "--adaptive" in r.stderr, (args, r.stderr)
