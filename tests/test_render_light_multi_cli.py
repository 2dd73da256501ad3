"""rt4_render's light runs beyond one process on one GPU: --light-gpus in bands and in frame blocks
(rehearsed on one device), --light-checkpoint / --light-resume, --light-pool, and the combinations they refuse."""
import os
import re
import subprocess

import numpy as np
import pytest

import light_merge_ref
import light_ref

pytestmark = pytest.mark.gpu

W, H, SEED, FRAMES = 40, 24, 4321, 5  # a partial 32 x 8 block; 5 frames leave ranks without frames at N = 8
SIZE = ["-W", str(W), "-H", str(H)]


@pytest.fixture(scope="module")
def props_path(tmp_path_factory):
    """The repository's properties with 4 samples and 3 bounces: the runs here take a moment each."""
    src = open(os.path.join(os.path.dirname(__file__), "..", "properties.txt")).read()
    src = re.sub(r"ray_tracing\.samples = \d+", "ray_tracing.samples = 4", src)
    src = re.sub(r"ray_tracing\.reflections_amount = \d+", "ray_tracing.reflections_amount = 3", src)
    path = tmp_path_factory.mktemp("props") / "properties.txt"
    path.write_text(src)
    return str(path)


def render(rt4, props_path, args, env=None, scene="sphere"):
    exe = os.path.join(os.path.dirname(rt4.LIB_PATH), "rt4_render")
    return subprocess.run([exe, "-p", props_path, "-s", scene, "--light"] + args, capture_output=True, text=True, timeout=120,
                          env=dict(os.environ, **(env or {})))


def ok(r):
    assert r.returncode == 0, r.stdout + r.stderr
    return r


def read_acc(pre):
    return np.fromfile(pre + "_yxz_light.raw", light_ref.LIGHT_DTYPE).reshape(H, W)


def read_image(pre):
    return np.fromfile(pre + "_yxz.raw", np.float32).reshape(H, W, 4)


def frame_uniforms(rt4, props_path, numbers, seed=SEED):
    """The uniforms rt4_render gives the progressive frames `numbers` of the main section."""
    props = rt4.Properties(path=props_path)
    base = rt4.uniforms_from_properties(props, W, H)
    cam = rt4.Camera(props)
    return [cam.frame_uniforms(base, rt4.SECTION_YXZ, seed ^ ((n * 0x9E3779B9) & 0xFFFFFFFF)) for n in numbers], base


def python_blocks(rt4, tracer, props_path, blocks, seed=SEED):
    """One accumulator per (first, count) block of frame numbers, each rendered from empty on this GPU."""
    tracer.set_scene(rt4.Scene.builtin("sphere"))
    out = []
    for first, count in blocks:
        us, _ = frame_uniforms(rt4, props_path, range(first + 1, first + count + 1), seed)
        out.append(tracer.render_light_host(us, rt4.region(W, H))[0] if count else np.zeros((H, W), rt4.LIGHT_DTYPE))
    return [np.ascontiguousarray(a).view(light_ref.LIGHT_DTYPE) for a in out]


@pytest.fixture(scope="module")
def single(rt4, props_path, tmp_path_factory):
    """The one-GPU --light run of FRAMES frames: its accumulator and resolved image (read-only) and its output."""
    pre = str(tmp_path_factory.mktemp("single") / "one")
    r = ok(render(rt4, props_path, SIZE + ["-n", str(FRAMES), "--seed", str(SEED), "--raw", "-o", pre]))
    acc, image = read_acc(pre), read_image(pre)
    acc.setflags(write=False)
    image.setflags(write=False)
    return acc, image, r.stdout


@pytest.mark.parametrize("gpus", [2, 3, 8])
def test_band_split_equals_one_gpu(rt4, props_path, single, tmp_path, gpus):
    acc, image, _ = single
    pre = str(tmp_path / "b")
    r = ok(render(rt4, props_path, SIZE + ["-n", str(FRAMES), "--seed", str(SEED), "--raw", "-o", pre, "--light-gpus", str(gpus),
                                           "--light-split", "bands", "--band", "4", "--rehearse"]))
    assert read_acc(pre).tobytes() == acc.tobytes() and read_image(pre).tobytes() == image.tobytes()
    assert f"measured {W * H}," in r.stdout


@pytest.mark.parametrize("gpus", [2, 3, 8])
def test_frame_split_equals_the_merge_of_its_blocks(rt4, tracer_lut, props_path, single, tmp_path, gpus):
    """The root's accumulator is the merge (light_merge_ref) of one-GPU renders of the frame_split blocks, every pixel
    is measured, and accumulator and image stay within the partition bound of test_light_merge_ref.py of the one-GPU
    run: against float64 means of the five frames' light, the frame split's relative error is at most 4x the
    sequential fold's (here the one-GPU accumulator's). For the image: both means lie within 5 e of each other relative
    to the mean (e the fold's error, 4 e the split's), the tone curve t(v) = 1 - 1/(k v + 1) has v t'(v) =
    k v / (k v + 1)^2 <= 1/4, and its three fp32 operations on values in [0, 2] round by at most 3 * 2^-24 together, for
    each of the two images."""
    acc, image, _ = single
    pre = str(tmp_path / "f")
    r = ok(render(rt4, props_path, SIZE + ["-n", str(FRAMES), "--seed", str(SEED), "--raw", "-o", pre, "--light-gpus", str(gpus),
                                           "--rehearse"]))
    got = read_acc(pre)
    blocks = python_blocks(rt4, tracer_lut, props_path, [rt4.frame_split(FRAMES, gpus, rank) for rank in range(gpus)])
    want = light_merge_ref.merge_all(np.zeros((H, W), light_ref.LIGHT_DTYPE), blocks)
    assert light_ref.same_acc(got, want)
    assert (got["n"] == FRAMES).all() and f"measured {W * H}," in r.stdout
    assert re.search(rf"light gpus {gpus} \(frames\), frames {FRAMES},", r.stdout), r.stdout
    # the partition bound on real frames: each frame's light is the mean of its own one-frame accumulator
    xs = python_blocks(rt4, tracer_lut, props_path, [(n, 1) for n in range(FRAMES)])
    mean64 = np.mean([x["mean"].astype(np.float64) for x in xs], axis=0)
    lit = mean64 > 0
    assert (got["mean"][~lit] == 0).all() and (acc["mean"][~lit] == 0).all()

    def rel(a):
        return float((np.abs(a["mean"].astype(np.float64) - mean64)[lit] / mean64[lit]).max())

    e_fold, e_split = rel(acc), rel(got)
    diff = float(np.abs(read_image(pre).astype(np.float64) - image.astype(np.float64)).max())
    print(f"gpus {gpus}: mean error {e_split:.3e} (one GPU {e_fold:.3e}), image differs by at most {diff:.3e}")
    assert e_split <= 4 * e_fold
    assert diff <= 5 * e_fold / 4 + 6 * 2.0 ** -24


def test_checkpoint_and_resume_give_the_unbroken_run(rt4, props_path, tmp_path):
    ck, a, b, c = str(tmp_path / "c.rt4l"), str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "c")
    seed = ["--seed", str(SEED), "--raw"]
    r = ok(render(rt4, props_path, SIZE + seed + ["-n", "5", "--light-checkpoint", ck, "-o", a]))
    assert "light checkpoint" in r.stdout and not os.path.exists(ck + ".tmp")
    info = rt4.light_info(ck)
    assert (info["w"], info["h"], info["frames_issued"], info["seed"], info["flags"]) == (W, H, 5, SEED, 0) and info["key"] != 0
    assert rt4.light_load(ck)[0].tobytes() == read_acc(a).tobytes()
    ok(render(rt4, props_path, SIZE + seed + ["-n", "3", "--light-resume", ck, "--light-checkpoint", ck, "-o", b]))
    ok(render(rt4, props_path, SIZE + seed + ["-n", "8", "-o", c]))
    assert read_acc(b).tobytes() == read_acc(c).tobytes() and read_image(b).tobytes() == read_image(c).tobytes()
    assert (read_acc(b)["n"] == 8).all() and rt4.light_info(ck)["frames_issued"] == 8  # the checkpoint was replaced
    # what a resume refuses: another seed, scene or size, and --adaptive
    resume = ["-n", "1", "--light-resume", ck, "-o", str(tmp_path / "x")]
    for args, scene, word in ((SIZE + ["--seed", "5"] + resume, "sphere", "seed"), (SIZE + seed + resume, "tiger", "scene"),
                              (["-W", "41", "-H", "24"] + seed + resume, "sphere", "40x24"),
                              (SIZE + seed + resume + ["--adaptive"], "sphere", "--adaptive")):
        r = render(rt4, props_path, args, scene=scene)
        assert r.returncode != 0 and "--light-resume" in r.stderr + " " and word in r.stderr, (word, r.stderr)
    assert not os.path.exists(str(tmp_path / "x") + "_yxz.ppm")


def test_adaptive_run_saves_a_checkpoint(rt4, props_path, tmp_path):
    """--adaptive with --light-checkpoint: frames_issued is the loop's last frame number, no pixel's n in particular."""
    ck, pre = str(tmp_path / "a.rt4l"), str(tmp_path / "a")
    ok(render(rt4, props_path, SIZE + ["-n", "12", "--seed", str(SEED), "--adaptive", "--raw", "--light-checkpoint", ck, "-o", pre]))
    acc, info = rt4.light_load(ck)
    assert acc.tobytes() == read_acc(pre).tobytes() and info["frames_issued"] >= int(acc["n"].max()) >= 8


def test_pool_of_two_seeds(rt4, props_path, tmp_path):
    cks = [str(tmp_path / f"s{s}.rt4l") for s in (1, 2)]
    for s, ck in zip((1, 2), cks):
        ok(render(rt4, props_path, SIZE + ["-n", "3", "--seed", str(s), "--light-checkpoint", ck, "-o", str(tmp_path / f"r{s}")]))
    pooled, pre = str(tmp_path / "p.rt4l"), str(tmp_path / "p")
    r = ok(render(rt4, props_path, ["--light-pool"] + cks + ["--raw", "--light-checkpoint", pooled, "-o", pre]))
    accs = [np.ascontiguousarray(rt4.light_load(ck)[0]).view(light_ref.LIGHT_DTYPE) for ck in cks]
    want = light_merge_ref.merge_all(np.zeros((H, W), light_ref.LIGHT_DTYPE), accs)
    assert light_ref.same_acc(read_acc(pre), want) and (want["n"] == 6).all()
    assert f"noise yxz: pixels {W * H}, measured {W * H}," in r.stdout and os.path.getsize(pre + "_yxz.ppm") > 0
    info = rt4.light_info(pooled)
    assert info["flags"] == rt4.LIGHT_POOLED and info["key"] == rt4.light_info(cks[0])["key"]
    assert rt4.light_load(pooled)[0].tobytes() == read_acc(pre).tobytes()
    # a pooled file cannot be resumed; the same seed twice, another size or another scene cannot be pooled
    r = render(rt4, props_path, SIZE + ["--seed", "1", "-n", "1", "--light-resume", pooled, "-o", str(tmp_path / "x")])
    assert r.returncode != 0 and "--light-resume" in r.stderr and "pool" in r.stderr, r.stderr
    r = render(rt4, props_path, ["--light-pool", cks[0], cks[0], "-o", str(tmp_path / "x")])
    assert r.returncode != 0 and "--light-pool" in r.stderr and "seed" in r.stderr, r.stderr
    other = str(tmp_path / "o.rt4l")
    ok(render(rt4, props_path, SIZE + ["-n", "1", "--seed", "3", "--light-checkpoint", other, "-o", str(tmp_path / "o")], scene="tiger"))
    r = render(rt4, props_path, ["--light-pool", cks[0], other, "-o", str(tmp_path / "x")])
    assert r.returncode != 0 and "--light-pool" in r.stderr and "scene" in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "x") + "_yxz.ppm")


@pytest.mark.parametrize("extra, word", [(["--light-gpus", "2", "--adaptive"], "--adaptive"),
                                         (["--light-gpus", "17"], "16"), (["--light-gpus", "2", "--light-split", "rows"], "frames or bands"),
                                         (["--light-gpus", "2", "-3"], "one section"), (["--light-split", "bands"], "--light-gpus")],
                         ids=lambda e: " ".join(e) if isinstance(e, list) else None)
def test_refusals(rt4, props_path, tmp_path, extra, word):
    r = render(rt4, props_path, SIZE + ["-n", "2", "--rehearse", "-o", str(tmp_path / "x")] + extra)
    assert r.returncode != 0 and "--light-" in r.stderr and word in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "x") + "_yxz.ppm")


def test_light_flags_need_light(rt4, props_path, tmp_path):
    exe = os.path.join(os.path.dirname(rt4.LIB_PATH), "rt4_render")
    for extra in (["--light-gpus", "2"], ["--light-checkpoint", "c"], ["--light-resume", "c"]):
        r = subprocess.run([exe, "-p", props_path, "-s", "sphere"] + SIZE + ["-o", str(tmp_path / "x")] + extra,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "need --light" in r.stderr, r.stderr


@pytest.mark.parametrize("split", ["frames", "bands"])
def test_failed_rank_skips_the_collective(rt4, props_path, tmp_path, split):
    """The hooks of --gpus on the shared machinery: rank 2's set-up fails, every rank skips render, gather and the root's
    last step, status 1 names the rank, nothing is written."""
    pre = str(tmp_path / "f")
    r = render(rt4, props_path, SIZE + ["-n", "3", "--light-gpus", "3", "--light-split", split, "--rehearse", "-o", pre],
               env={"RT4_RENDER_FAIL_RANK": "2"})
    assert r.returncode == 1, r.stdout + r.stderr
    assert "--light-gpus" in r.stderr and "rank 2: set-up failure injected" in r.stderr, r.stderr
    assert not os.path.exists(pre + "_yxz.ppm")
