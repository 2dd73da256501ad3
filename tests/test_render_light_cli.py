"""rt4_render --light: the host program's light-domain run against the same steps from Python, and the combinations it
refuses."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def render_paths(rt4):
    lib_dir = os.path.dirname(rt4.LIB_PATH)
    return os.path.join(lib_dir, "rt4_render"), os.path.join(lib_dir, "..", "..", "properties.txt")


def test_cpp_host_light(rt4, tracer_lut, tmp_path):
    """-s sphere -n 4 --light --noise-map at the properties' cell size: the image is the Python resolve of the same
    frames, the map is their q as grey, and the statistics printed are the library's."""
    exe, props_path = render_paths(rt4)
    seed, frames, thr = 4321, 4, 0.01
    pre = str(tmp_path / "l")
    r = subprocess.run([exe, "-p", props_path, "-s", "sphere", "-n", str(frames), "--seed", str(seed), "--light", "--noise-map",
                        "--noise-threshold", str(thr), "-o", pre], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    props = rt4.Properties(path=props_path)
    w, h = rt4.window_cells(props, "main")
    base = rt4.uniforms_from_properties(props, w, h)
    cam = rt4.Camera(props)
    us = [cam.frame_uniforms(base, rt4.SECTION_YXZ, seed ^ ((n * 0x9E3779B9) & 0xFFFFFFFF)) for n in range(1, frames + 1)]
    tracer_lut.set_scene(rt4.Scene.builtin("sphere"))
    acc, _ = tracer_lut.render_light_host(us, rt4.region(w, h))
    k = base.light_to_color_conversion_coefficient
    rt4.write_ppm(str(tmp_path / "py.ppm"), tracer_lut.light_resolve_host(acc, k))
    assert open(str(tmp_path / "py.ppm"), "rb").read() == open(pre + "_yxz.ppm", "rb").read()
    _, q, _, stats = tracer_lut.light_noise_host(acc, k, thr, se=False, tiles=False)
    grey = np.ones((h, w, 4), np.float32)
    grey[..., :3] = np.where(np.isnan(q), np.float32(0), q)[..., None]
    rt4.write_ppm(str(tmp_path / "py_q.ppm"), grey)
    assert open(str(tmp_path / "py_q.ppm"), "rb").read() == open(pre + "_yxz_q.ppm", "rb").read()
    m = re.search(r"noise yxz: pixels (\d+), measured (\d+), above (\d+) \(threshold ([^)]+)\), max_q (\S+), max_se (\S+)", r.stdout)
    assert m, r.stdout
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (w * h, stats["measured"], stats["above"])
    assert stats["measured"] == w * h and 0 < stats["above"] < w * h
    assert float(m.group(5)) == pytest.approx(stats["max_q"], rel=1e-5) and float(m.group(6)) == pytest.approx(stats["max_se"], rel=1e-5)
    # the light image is not the colour image of the same frames
    r2 = subprocess.run([exe, "-p", props_path, "-s", "sphere", "-n", str(frames), "--seed", str(seed), "-o", str(tmp_path / "c")],
                        capture_output=True, text=True, timeout=120)
    assert r2.returncode == 0, r2.stderr
    assert open(str(tmp_path / "c_yxz.ppm"), "rb").read() != open(pre + "_yxz.ppm", "rb").read()


def test_cpp_host_light_sections_denoise_window(rt4, tmp_path):
    """--light composes with -3, --denoise and --window: every section's files are written and its statistics printed."""
    exe, props_path = render_paths(rt4)
    pre = str(tmp_path / "s")
    r = subprocess.run([exe, "-p", props_path, "-s", "tiger", "-n", "3", "-3", "--light", "--denoise", "2", "--window", "2",
                        "-o", pre], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    for tag in ("yxz", "ywz", "yxw"):
        for suffix in ("", "_dn", "_win"):
            assert os.path.getsize(f"{pre}_{tag}{suffix}.ppm") > 0, (tag, suffix)
        assert f"noise {tag}: pixels" in r.stdout


@pytest.mark.parametrize("extra", [["--reproject"], ["--resume", "none.ckpt"], ["--checkpoint", "c.ckpt"], ["--gpus", "2"],
                                   ["--frame-by-frame"]], ids=lambda e: e[0])
def test_cpp_host_light_refusals(rt4, tmp_path, extra):
    exe, props_path = render_paths(rt4)
    r = subprocess.run([exe, "-p", props_path, "-s", "sphere", "-W", "16", "-H", "8", "--light", "-o", str(tmp_path / "x")] + extra,
                       capture_output=True, text=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode != 0 and "--light" in r.stderr, (extra, r.stderr)
