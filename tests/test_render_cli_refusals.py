"""rt4_render's refusals, on the CPU: every command line that parse_args or refuse_conflicts turns
down, and every checkpoint the loaders turn down, exits with status 1 and exactly `rt4_render: <what>: <why>` on
stderr before any HIP call, and writes nothing. Command lines that break two rules pin which one is reported: the
first check in the program's order. The expected strings were recorded from the program before its main was split
into steps; the GPU tests of the same flags only look for substrings."""
import glob
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 16, 8

REPROJECT_GPUS = ("--reproject", "not with --gpus: the temporal image lives on one GPU")
REPROJECT_CKPT = ("--reproject", "not with --resume / --checkpoint: a checkpoint holds no per-pixel history")
LIGHT_CKPT = ("--light", "not with --resume / --checkpoint: a checkpoint holds colours, not a light accumulator "
                         "(--light-resume / --light-checkpoint save and continue a light accumulator)")
LIGHT_GPUS = ("--light", "not with --gpus: that gathers colour frames (--light-gpus N runs a light accumulator on N GPUs)")
NEED_LIGHT = ("--light-resume / --light-checkpoint / --light-gpus / --light-split", "need --light")
LIGHT_GPUS_N = ("--light-gpus", "N must be 1..16 (RT4_LIGHT_MERGE_MAX: one merge takes that many accumulators)")
LIGHT_GPUS_ADAPTIVE = ("--light-gpus", "not with --adaptive: the tile selection runs on one GPU")
POOL = ("--light-pool", "renders nothing: only with -o, --png, --raw, --noise-map, --noise-threshold, --light-checkpoint")
NOISE = ("--noise-map / --noise-threshold", "need --light")
ADAPTIVE_LIGHT = ("--adaptive", "needs --light: it samples by the light accumulator's standard error")
ADAPTIVE_RANGE = ("--adaptive", "warmup >= 0, pass >= 1, full-every >= 0, min-above 1..64, dilate 0..2, a threshold that is a number")
ONE_SECTION_ONE_GPU = ("--resume/--checkpoint", "need one section on one GPU")
LIGHT_ONE_SECTION = ("--light-resume / --light-checkpoint", "need one section")
LIGHT_GPUS_FRAMES = ("--light-gpus", "frames and band must be >= 1")
DENOISE_GPUS = ("--denoise", "not with --gpus: the frame is not filtered after the gather")
WINDOW_GPUS = ("--window", "not with --gpus: the frame is not upscaled after the gather")
GPUS_RESTING = ("--gpus", "needs one section and a resting camera")
GPUS_FRAMES = ("--gpus", "frames and band must be >= 1")
MOVE = ["--keys", "W", "--move-seconds", "0.1"]

# (arguments after `-p properties -s sphere -W 16 -H 8 -o prefix`, what, why)
OPTION_CASES = [
    # parse_args: the value checks of single flags, in the order of the command line
    (["-n"], "missing value for", "-n"),
    (["--light-checkpoint"], "missing value for", "--light-checkpoint"),
    (["--bogus"], "unknown argument", "--bogus"),
    (["--window", "0"], "--window", "SCALE must be 1..64"),
    (["--window", "65"], "--window", "SCALE must be 1..64"),
    (["--denoise", "0"], "--denoise", "levels must be 1..6"),
    (["--denoise", "7"], "--denoise", "levels must be 1..6"),
    (["--light", "--light-denoise", "7"], "--light-denoise", "levels must be 0..6"),
    (["--light-pool"], "--light-pool", "needs two or more light checkpoints"),
    (["--light-pool", "a", "--raw"], "--light-pool", "needs two or more light checkpoints"),
    (["--denoise", "0", "--bogus"], "--denoise", "levels must be 1..6"),
    (["--bogus", "--denoise", "0"], "unknown argument", "--bogus"),
    (["--reproject", "--gpus", "2", "--window", "0"], "--window", "SCALE must be 1..64"),
    # refuse_conflicts, in its order
    (["--reproject", "--gpus", "2"],) + REPROJECT_GPUS,
    (["--reproject", "--resume", "x"],) + REPROJECT_CKPT,
    (["--reproject", "--checkpoint", "x"],) + REPROJECT_CKPT,
    (["--reproject", "--frame-by-frame"], "--reproject", "not with --frame-by-frame: every temporal frame is a launch of its own"),
    (["--light", "--reproject"], "--light", "not with --reproject: the temporal history is a colour average"),
    (["--light", "--resume", "x"],) + LIGHT_CKPT,
    (["--light", "--checkpoint", "x"],) + LIGHT_CKPT,
    (["--light", "--gpus", "2"],) + LIGHT_GPUS,
    (["--light-gpus", "2"],) + NEED_LIGHT,
    (["--light-checkpoint", "c"],) + NEED_LIGHT,
    (["--light-resume", "c"],) + NEED_LIGHT,
    (["--light-split", "bands"],) + NEED_LIGHT,
    (["--light", "--light-split", "bands"], "--light-split", "needs --light-gpus"),
    (["--light", "--light-gpus", "2", "--light-split", "rows"], "--light-split", "frames or bands"),
    (["--light", "--light-gpus", "17"],) + LIGHT_GPUS_N,
    (["--light", "--light-gpus", "-1"],) + LIGHT_GPUS_N,
    (["--light", "--light-gpus", "2", "--adaptive"],) + LIGHT_GPUS_ADAPTIVE,
    (["--light", "--light-gpus", "2", "--light-resume", "c"], "--light-gpus", "not with --light-resume: resume on one GPU"),
    (["--light", "--light-resume", "c", "--adaptive"], "--light-resume",
     "not with --adaptive: a light checkpoint does not hold the adaptive loop's pass state"),
    (["--light-pool", "a", "b", "--adaptive"],) + POOL,
    (["--light-pool", "a", "b", "--light-resume", "c"],) + POOL,
    (["--light-pool", "a", "b", "-3"],) + POOL,
    (["--light-pool", "a", "b", "--denoise"],) + POOL,
    (["--light-pool", "a", "b", "--light-denoise"],) + POOL,
    (["--light-pool", "a", "b", "--window"],) + POOL,
    (["--light", "--frame-by-frame"], "--light", "not with --frame-by-frame: the frames go through rt4_render_light_device"),
    (["--light"] + MOVE, "--light", "needs a resting camera: the accumulator averages one view"),
    (["--noise-map"],) + NOISE,
    (["--noise-threshold", "0.5"],) + NOISE,
    (["--adaptive"],) + ADAPTIVE_LIGHT,
    (["--adaptive-pass", "2"],) + ADAPTIVE_LIGHT,
    (["--light", "--adaptive-pass", "2"], "--adaptive-*", "need --adaptive"),
    (["--light", "--adaptive", "--adaptive-warmup", "-1"],) + ADAPTIVE_RANGE,
    (["--light", "--adaptive", "--adaptive-pass", "0"],) + ADAPTIVE_RANGE,
    (["--light", "--adaptive", "--adaptive-full-every", "-1"],) + ADAPTIVE_RANGE,
    (["--light", "--adaptive", "--adaptive-min-above", "65"],) + ADAPTIVE_RANGE,
    (["--light", "--adaptive", "--adaptive-dilate", "3"],) + ADAPTIVE_RANGE,
    (["--light", "--adaptive", "--noise-threshold", "nan"],) + ADAPTIVE_RANGE,
    (["--light-denoise"], "--light-denoise", "needs --light: it filters the light accumulator"),
    (["--light", "--light-denoise", "--denoise"], "--light-denoise", "not with --denoise: one filtered frame per image"),
    # the checks that depend on the options alone and used to run after the files were read
    (["--checkpoint", "x", "-3"],) + ONE_SECTION_ONE_GPU,
    (["--resume", "x", "--gpus", "2"],) + ONE_SECTION_ONE_GPU,
    (["--light", "--light-checkpoint", "c", "-3"],) + LIGHT_ONE_SECTION,
    (["--light", "--light-resume", "c", "-3"],) + LIGHT_ONE_SECTION,
    (["--light", "--light-gpus", "2", "-3"], "--light-gpus", "needs one section"),
    (["--light", "--light-gpus", "2", "-n", "0"],) + LIGHT_GPUS_FRAMES,
    (["--light", "--light-gpus", "2", "--band", "0"],) + LIGHT_GPUS_FRAMES,
    (["--gpus", "2", "--denoise"],) + DENOISE_GPUS,
    (["--gpus", "2", "--window"],) + WINDOW_GPUS,
    (["--gpus", "2", "--window-nearest"],) + WINDOW_GPUS,
    (["--gpus", "2", "-3"],) + GPUS_RESTING,
    (["--gpus", "2"] + MOVE,) + GPUS_RESTING,
    (["--gpus", "2", "-n", "0"],) + GPUS_FRAMES,
    (["--gpus", "2", "--band", "0"],) + GPUS_FRAMES,
    # two rules broken at once: the earlier check is the one reported
    (["--light", "--reproject", "--gpus", "2"],) + REPROJECT_GPUS,
    (["--reproject", "--frame-by-frame", "--resume", "x"],) + REPROJECT_CKPT,
    (["--light", "--gpus", "2", "--checkpoint", "x"],) + LIGHT_CKPT,
    (["--light-gpus", "2", "--light-split", "rows"],) + NEED_LIGHT,
    (["--light", "--light-gpus", "17", "--adaptive"],) + LIGHT_GPUS_N,
    (["--light", "--light-gpus", "2", "--adaptive", "--light-resume", "c"],) + LIGHT_GPUS_ADAPTIVE,
    (["--light-pool", "a", "b", "--light-gpus", "2", "--adaptive"],) + LIGHT_GPUS_ADAPTIVE,
    (["--light-pool", "a", "b", "--reproject"], "--light", "not with --reproject: the temporal history is a colour average"),
    (["--adaptive", "--noise-map"],) + NOISE,
    (["--light", "--light-denoise", "--denoise", "--gpus", "2"],) + LIGHT_GPUS,
    (["--checkpoint", "x", "-3", "--gpus", "2", "--denoise"],) + ONE_SECTION_ONE_GPU,
    (["--light", "--light-gpus", "2", "-3", "--light-checkpoint", "c"],) + LIGHT_ONE_SECTION,
    (["--light", "--light-gpus", "2", "-3", "-n", "0"], "--light-gpus", "needs one section"),
    (["--gpus", "2", "--denoise", "--window", "-3"],) + DENOISE_GPUS,
    (["--gpus", "2", "--window", "-3"],) + WINDOW_GPUS,
    (["--gpus", "2", "-3", "-n", "0"],) + GPUS_RESTING,
]


@pytest.fixture(scope="module")
def exe(rt4):
    path = os.path.join(os.path.dirname(rt4.LIB_PATH), "rt4_render")
    if not os.path.exists(path):
        pytest.skip("lib/rt4_render not built")
    return path


def refused(exe, tmp_path, args, what, why, size=(W, H)):
    pre = str(tmp_path / "out")
    cmd = [exe, "-p", os.path.join(ROOT, "properties.txt"), "-s", "sphere", "-W", str(size[0]), "-H", str(size[1]), "-o", pre]
    r = subprocess.run(cmd + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert r.stderr == f"rt4_render: {what}: {why}\n"
    assert r.stdout == "" and glob.glob(pre + "*") == []


@pytest.mark.parametrize("args, what, why", OPTION_CASES, ids=[" ".join(c[0]) for c in OPTION_CASES])
def test_options_refused(exe, tmp_path, args, what, why):
    refused(exe, tmp_path, args, what, why)


KEY, SEED = 0xDEADBEEF, 7  # a key no run has; KEY ^ 1 is another; key 0 is "not recorded" and never compared on a resume


@pytest.fixture(scope="module")
def files(rt4, tmp_path_factory):
    """Checkpoints of 16 x 8 (and one of 17 x 8) empty accumulators, written by the host-only savers."""
    d = tmp_path_factory.mktemp("ckpt")

    def light(name, seed=SEED, key=0, flags=0, w=W, issued=3):
        rt4.light_save(str(d / name), np.zeros((H, w), rt4.LIGHT_DTYPE), issued, seed, key=key, flags=flags)
        return str(d / name)

    def colour(name, key=0):
        rt4.accum_save(str(d / name), np.zeros((H, W, 4), np.float32), 2, SEED, key=key)
        return str(d / name)

    return {"light": light("l"), "light_key": light("lk", key=KEY), "light_pooled": light("lp", flags=rt4.LIGHT_POOLED),
            "light_full": light("lf", issued=0xFFFFFFFF), "colour": colour("c"), "colour_key": colour("ck", key=KEY),
            "a": light("a", seed=1, key=KEY), "a_again": light("a2", seed=1, key=KEY), "b": light("b", seed=2, key=KEY),
            "wide": light("w", seed=2, key=KEY, w=W + 1), "other": light("o", seed=2, key=KEY ^ 1),
            "wide_other": light("wo", seed=1, key=KEY ^ 1, w=W + 1), "other_again": light("o2", seed=1, key=KEY ^ 1)}


OTHER_SEED = "the checkpoint was made with another --seed"
OTHER_KEY = "the checkpoint was made with another scene, properties or camera"
POOLED = "the checkpoint pools runs of several seeds: it cannot be resumed"
OTHER_SIZE = f"the checkpoint holds a {W}x{H} accumulator, not {W + 1}x{H}"

# (arguments, the files' names in them replaced by their paths; size; what; why)
RESUME_CASES = [
    (["--seed", "8", "--resume", "colour"], (W, H), "--resume", OTHER_SEED),
    (["--seed", "7", "--resume", "colour_key"], (W, H), "--resume", OTHER_KEY),
    (["--seed", "8", "--resume", "colour_key"], (W, H), "--resume", OTHER_SEED),
    (["--light", "--seed", "8", "--light-resume", "light"], (W, H), "--light-resume", OTHER_SEED),
    (["--light", "--seed", "7", "--light-resume", "light_key"], (W, H), "--light-resume", OTHER_KEY),
    (["--light", "--seed", "7", "--light-resume", "light"], (W + 1, H), "--light-resume", OTHER_SIZE),
    (["--light", "--seed", "7", "--light-resume", "light_pooled"], (W, H), "--light-resume", POOLED),
    (["--light", "--seed", "7", "--light-resume", "light_full"], (W, H), "--light-resume", "frame numbers beyond 2^32 - 1"),
    # two at once: pooled before size before seed before key
    (["--light", "--seed", "8", "--light-resume", "light_pooled"], (W + 1, H), "--light-resume", POOLED),
    (["--light", "--seed", "8", "--light-resume", "light_key"], (W + 1, H), "--light-resume", OTHER_SIZE),
    (["--light", "--seed", "8", "--light-resume", "light_key"], (W, H), "--light-resume", OTHER_SEED),
]


@pytest.mark.parametrize("args, size, what, why", RESUME_CASES, ids=[f"{' '.join(c[0])} {c[1][0]}x{c[1][1]}" for c in RESUME_CASES])
def test_checkpoints_refused(exe, files, tmp_path, args, size, what, why):
    refused(exe, tmp_path, [files.get(a, a) for a in args], what, why, size)


POOL_SIZE = "--light-pool: another image size than the first file's"
POOL_KEY = "--light-pool: another scene, properties or camera than the first file's"
POOL_SEED = "--light-pool: the same --seed as an earlier file, the same frames would count twice"

# (the pool's files, what; the why is the path of the last file)
POOL_CASES = [
    (["a", "a_again"], POOL_SEED),
    (["a", "b", "a_again"], POOL_SEED),
    (["a", "wide"], POOL_SIZE),
    (["a", "other"], POOL_KEY),
    # two at once: size before key before seed
    (["a", "wide_other"], POOL_SIZE),
    (["a", "other_again"], POOL_KEY),
]


@pytest.mark.parametrize("names, what", POOL_CASES, ids=[" ".join(c[0]) for c in POOL_CASES])
def test_pools_refused(exe, files, tmp_path, names, what):
    paths = [files[n] for n in names]
    refused(exe, tmp_path, ["--light-pool"] + paths + ["--raw"], what, paths[-1])
