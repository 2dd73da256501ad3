"""rt4_render --retina on the CPU: every command line that the retina's refusals turn down exits with status 1 and
exactly `rt4_render: --retina: <why>` on stderr before any HIP call, and writes nothing (the style of
test_render_cli_refusals.py). The --retina checks run ahead of every other refusal, so a command line that also breaks
an older rule still hears the retina's reason."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEED = "--retina-size / --retina-view / --retina-turntable / --retina-step need --retina D"
DEPTH = "D must be 1..256 slices"
GPUS = "not with --gpus / --light-gpus: the volume is accumulated on one GPU"
THREE = "not with -3: the volume holds the main section's view"
REPROJECT = "not with --reproject: the volume is a light accumulation of one view"
ADAPTIVE = "not with --adaptive: every slice takes every frame"
DENOISE = "not with --denoise / --light-denoise: the projection is not filtered"
WINDOW = "not with --window: the projection is written at the window's size already"
FILES = "not with --resume / --checkpoint / --light-resume / --light-checkpoint / --light-pool: no file format holds a volume"
FRAME_BY_FRAME = "not with --frame-by-frame: the frames go through rt4_render_light_device"
MOVING = "needs a resting camera: the volume accumulates one view"
VALUES = "size >= 0 (0: the matrix height), a view of two angles in degrees, turntable >= 0, step > 0"
MOVE = ["--keys", "W", "--move-seconds", "0.1"]

# (arguments after `-p properties -s sphere -W 16 -H 12 -o prefix`, why)
CASES = [
    (["--retina-size", "2"], NEED),
    (["--retina-view", "30", "20"], NEED),
    (["--retina-turntable", "4"], NEED),
    (["--retina-step", "0.5"], NEED),
    (["--retina", "0"], DEPTH),
    (["--retina", "257"], DEPTH),
    (["--retina", "-3"], DEPTH),
    (["--retina", "5", "--gpus", "2"], GPUS),
    (["--retina", "5", "--light", "--light-gpus", "2"], GPUS),
    (["--retina", "5", "-3"], THREE),
    (["--retina", "5", "--reproject"], REPROJECT),
    (["--retina", "5", "--light", "--adaptive"], ADAPTIVE),
    (["--retina", "5", "--adaptive-pass", "2"], ADAPTIVE),
    (["--retina", "5", "--denoise"], DENOISE),
    (["--retina", "5", "--light", "--light-denoise"], DENOISE),
    (["--retina", "5", "--window"], WINDOW),
    (["--retina", "5", "--window-nearest"], WINDOW),
    (["--retina", "5", "--resume", "x"], FILES),
    (["--retina", "5", "--checkpoint", "x"], FILES),
    (["--retina", "5", "--light", "--light-resume", "x"], FILES),
    (["--retina", "5", "--light", "--light-checkpoint", "x"], FILES),
    (["--retina", "5", "--light-pool", "a", "b"], FILES),
    (["--retina", "5", "--frame-by-frame"], FRAME_BY_FRAME),
    (["--retina", "5"] + MOVE, MOVING),
    (["--retina", "5", "-n", "0"], "frames must be >= 1"),
    (["--retina", "5", "--retina-step", "0"], VALUES),
    (["--retina", "5", "--retina-step", "nan"], VALUES),
    (["--retina", "5", "--retina-size", "-1"], VALUES),
    (["--retina", "5", "--retina-view", "inf", "0"], VALUES),
    (["--retina", "5", "--retina-turntable", "-2"], VALUES),
    # two rules at once: the retina's own order, and the retina's reason ahead of an older rule's
    (["--retina", "300", "--gpus", "2"], DEPTH),
    (["--retina", "5", "-3", "--reproject"], THREE),
    (["--retina", "5", "--reproject", "--gpus", "2"], GPUS),
    (["--retina", "5", "--light", "--reproject"], REPROJECT),
    (["--retina", "5", "--light-checkpoint", "c"], FILES),
    (["--retina", "5", "--denoise", "--window"], DENOISE),
    (["--retina-step", "2", "--gpus", "2", "--window"], NEED),
]


@pytest.fixture(scope="module")
def exe(rt4):
    path = os.path.join(os.path.dirname(rt4.LIB_PATH), "rt4_render")
    assert os.path.exists(path), "lib/rt4_render not built"
    return path


@pytest.mark.parametrize("args, why", CASES, ids=[" ".join(c[0]) for c in CASES])
def test_retina_refused(exe, tmp_path, args, why):
    pre = str(tmp_path / "out")
    cmd = [exe, "-p", os.path.join(ROOT, "properties.txt"), "-s", "sphere", "-W", "16", "-H", "12", "-o", pre]
    r = subprocess.run(cmd + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert r.stderr == f"rt4_render: --retina: {why}\n"
    assert r.stdout == "" and glob.glob(pre + "*") == []


def test_step_too_small_for_the_box_is_refused_before_any_device_call(exe, tmp_path):
    """What depends on the inputs: a step that needs more than RT4_RETINA_MAX_STEPS samples is turned down by
    rt4_retina_view_make once the properties are read, still ahead of the first HIP call."""
    pre = str(tmp_path / "out")
    cmd = [exe, "-p", os.path.join(ROOT, "properties.txt"), "-s", "sphere", "-W", "16", "-H", "12", "-o", pre, "--retina", "5",
           "--retina-step", "0.001"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and r.stdout == "" and glob.glob(pre + "*") == []
    assert r.stderr.startswith("rt4_render: rt4_retina_view_make(") and "more than 4096" in r.stderr
