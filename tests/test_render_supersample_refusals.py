"""rt4_render --supersample's refusals, on the CPU, in the style of test_render_cli_refusals: each exits
with status 1 and exactly `rt4_render: --supersample: <why>` on stderr before any HIP call and writes nothing. They
stand at the end of parse_args' value checks and of refuse_conflicts, so every earlier rule is reported first: the
double-rule cases pin that."""
import glob
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 16, 8

RANGE = "S must be 1..8"
NEEDS_LIGHT = "needs --light: it averages light accumulators"
NOT_WITH = "not with --light-gpus, --light-pool or --retina"


def too_large(w, h):
    return f"the render would be {w}x{h}: the light render takes at most 8191 x 8191"


# (arguments after `-p properties -s sphere -W w -H h -o prefix`, size, what, why)
CASES = [
    (["--light", "--supersample", "0"], (W, H), "--supersample", RANGE),
    (["--light", "--supersample", "9"], (W, H), "--supersample", RANGE),
    (["--light", "--supersample", "-2"], (W, H), "--supersample", RANGE),
    (["--light", "--supersample", "x"], (W, H), "--supersample", RANGE),
    (["--supersample", "2"], (W, H), "--supersample", NEEDS_LIGHT),
    (["--light", "--supersample", "2", "--light-gpus", "2"], (W, H), "--supersample", NOT_WITH),
    (["--supersample", "2", "--light-pool", "a", "b"], (W, H), "--supersample", NOT_WITH),
    (["--light", "--supersample", "2", "--retina", "4"], (W, H), "--supersample", NOT_WITH),
    (["--light", "--supersample", "2"], (4096, H), "--supersample", too_large(8192, 2 * H)),
    (["--light", "--supersample", "8"], (W, 1024), "--supersample", too_large(8 * W, 8192)),
    (["--light", "--supersample", "1"], (8192, H), "--supersample", too_large(8192, H)),
    # two rules broken at once: the value check of parse_args before every conflict, and the conflicts in their order
    (["--supersample", "9"], (W, H), "--supersample", RANGE),
    (["--supersample", "2", "--light-gpus", "2"], (W, H), "--light-resume / --light-checkpoint / --light-gpus / --light-split",
     "need --light"),
    (["--supersample", "9", "--denoise", "0"], (W, H), "--denoise", "levels must be 1..6"),
    (["--supersample", "2", "--light-gpus", "2", "--light"], (4096, H), "--supersample", NOT_WITH),
    (["--supersample", "2"], (4096, H), "--supersample", NEEDS_LIGHT),
]


@pytest.fixture(scope="module")
def exe(rt4):
    path = os.path.join(os.path.dirname(rt4.LIB_PATH), "rt4_render")
    if not os.path.exists(path):
        pytest.skip("lib/rt4_render not built")
    return path


@pytest.mark.parametrize("args, size, what, why", CASES, ids=[f"{' '.join(c[0])} {c[1][0]}x{c[1][1]}" for c in CASES])
def test_supersample_refused(exe, tmp_path, args, size, what, why):
    pre = str(tmp_path / "out")
    cmd = [exe, "-p", os.path.join(ROOT, "properties.txt"), "-s", "sphere", "-W", str(size[0]), "-H", str(size[1]), "-o", pre]
    r = subprocess.run(cmd + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert r.stderr == f"rt4_render: {what}: {why}\n"
    assert r.stdout == "" and glob.glob(pre + "*") == []


def test_properties_cells_are_checked_too(exe, tmp_path):
    """Without -W -H the output is the properties' cells, known once they are read: still before any HIP call."""
    text = open(os.path.join(ROOT, "properties.txt")).read()
    assert "window.main.cell_size = 7 " in text and "window.main.width = 850 " in text
    props = tmp_path / "p.txt"  # 1100 cells wide
    props.write_text(text.replace("window.main.cell_size = 7 ", "window.main.cell_size = 1 ").replace("window.main.width = 850 ",
                                                                                                    "window.main.width = 1100 "))
    pre = str(tmp_path / "out")
    r = subprocess.run([exe, "-p", str(props), "-s", "sphere", "--light", "--supersample", "8", "-o", pre], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 1, (r.returncode, r.stdout, r.stderr)
    assert r.stderr.startswith("rt4_render: --supersample: the render would be 8800x")
    assert r.stderr.endswith(": the light render takes at most 8191 x 8191\n")
    assert r.stdout == "" and glob.glob(pre + "*") == []
