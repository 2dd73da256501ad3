"""rt4_render_light_tiles_device on the GPU (rt4.h): the listed tiles hold the bytes of the full light
render and nothing else changes, in every kernel variant; lists (empty, all, permuted, one, entries to ignore); regions
(padded, offset, banded); a launch boundary; the argument errors; and the context's other launches afterwards."""
import ctypes

import numpy as np
import pytest

import adaptive_ref
import light_ref
from denoise_ref import region_rows

pytestmark = pytest.mark.gpu

ERR_ARG = -1
SCENES = ["sphere", "all_primitives", "tiger"]
FLAGS = {"default": 0, "generic": 0x2, "lut": 0x1, "reuse": 0x4, "serial": 0x8}
POISON = 0xAB


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def as_ref(acc):
    return np.ascontiguousarray(acc).view(light_ref.LIGHT_DTYPE)


def n_tiles_of(w, h):
    return ((w + 7) // 8) * ((h + 7) // 8)


@pytest.fixture(scope="module")
def tracers(rt4):
    made = {}

    def get(flag_name):
        if flag_name not in made:
            made[flag_name] = rt4.Tracer(device=0, flags=FLAGS[flag_name])
        return made[flag_name]

    yield get
    for t in made.values():
        t.close()


def frame_uniforms(rt4, w, h, first, n, spp=2, bounces=3):
    return [rt4.make_uniforms(w, h, samples=spp, reflections=bounces, seed=s) for s in range(first, first + n)]


def check_listed(got, full, start, mask, what):
    """The listed tiles' pixels are the full render's, every other pixel is the start's."""
    assert light_ref.same_acc(as_ref(got)[mask], as_ref(full)[mask]), what
    assert raw(got[~mask]) == raw(start[~mask]), what


# ------------------------------------------------------------------------------------------ 1. against the full render
@pytest.mark.parametrize("flag_name", list(FLAGS))
@pytest.mark.parametrize("name", SCENES)
def test_listed_tiles_equal_the_full_render(rt4, tracers, name, flag_name):
    """33 x 17: 5 x 3 tiles, the right column 1 pixel wide, the bottom row 1 pixel high. 3 frames onto 2."""
    w, h = 33, 17
    lst = [0, 4, 7, 14]
    t = tracers(flag_name)
    t.set_scene(rt4.Scene.named(name))
    reg = rt4.region(w, h)
    start, _ = t.render_light_host(frame_uniforms(rt4, w, h, 1, 2), reg)
    us = frame_uniforms(rt4, w, h, 3, 3)
    full, n_full = t.render_light_host(us, reg, start.copy())
    got, n_list = t.render_light_tiles_host(us, reg, lst, start.copy())
    rest = [x for x in range(15) if x not in lst]
    other, n_rest = t.render_light_tiles_host(us, reg, rest, start.copy())
    mask = adaptive_ref.tile_mask(lst, w, h)
    assert mask.sum() == 64 + 8 + 64 + 1
    check_listed(got, full, start, mask, (name, flag_name))
    check_listed(other, full, start, ~mask, (name, flag_name, "complement"))
    assert (got["n"][mask] == 5).all() and (got["n"][~mask] == 2).all()
    assert 0 < n_list < n_full and n_list + n_rest == n_full


# ------------------------------------------------------------------------------------------ 2. lists
SHAPES = [(1, 1), (8, 8), (9, 9), (64, 1), (1, 64), (33, 17)]


@pytest.mark.parametrize("w, h", SHAPES)
def test_lists(rt4, tracers, w, h):
    t = tracers("default")
    t.set_scene(rt4.Scene.named("sphere"))
    reg = rt4.region(w, h)
    tiles = n_tiles_of(w, h)
    start, _ = t.render_light_host(frame_uniforms(rt4, w, h, 1, 1), reg)
    us = frame_uniforms(rt4, w, h, 2, 2)
    full, n_full = t.render_light_host(us, reg, start.copy())
    assert raw(full) != raw(start)
    # empty
    got, n = t.render_light_tiles_host(us, reg, [], start.copy())
    assert raw(got) == raw(start) and n == 0
    # all tiles, ascending and permuted: the full render byte for byte, the count included
    for lst in (np.arange(tiles), np.random.default_rng(w * 100 + h).permutation(tiles)):
        got, n = t.render_light_tiles_host(us, reg, lst, start.copy())
        assert raw(got) == raw(full) and n == n_full, lst
    # one tile: the last one (partial on 9x9 and 33x17)
    got, n_one = t.render_light_tiles_host(us, reg, [tiles - 1], start.copy())
    check_listed(got, full, start, adaptive_ref.tile_mask([tiles - 1], w, h), "one")
    # entries >= tiles are ignored (the list may be no longer than the tile count)
    if tiles >= 3:
        got, n = t.render_light_tiles_host(us, reg, [tiles, tiles - 1, 0xFFFFFFFF], start.copy())
        assert raw(got) == raw(t.render_light_tiles_host(us, reg, [tiles - 1], start.copy())[0]) and n == n_one
    else:
        for bad in (tiles, 0xFFFFFFFF, 0x80000000):
            got, n = t.render_light_tiles_host(us, reg, [bad], start.copy())
            assert raw(got) == raw(start) and n == 0, bad


# ------------------------------------------------------------------------------------------ 3. regions
def padded(rt4, acc, extra):
    """acc in the left columns of a wider array whose padding holds other bytes."""
    h, w = acc.shape
    a = np.zeros((h, w + extra), rt4.LIGHT_DTYPE)
    a.view(np.uint8).reshape(h, w + extra, 32)[:, w:] = POISON
    a[:, :w] = acc
    return a


def padding_kept(a, w):
    return (a.view(np.uint8).reshape(a.shape[0], a.shape[1], 32)[:, w:] == POISON).all()


def test_regions(rt4, tracers):
    """Tile numbers are region-local: a padded stride, an offset region and a banded region."""
    t = tracers("default")
    t.set_scene(rt4.Scene.named("sphere"))
    us_pre, us = frame_uniforms(rt4, 33, 17, 1, 1), frame_uniforms(rt4, 33, 17, 2, 3)
    regs = [(rt4.region(33, 17), 3), (rt4.region(20, 9, x0=7, y0=5), 0), (rt4.region(20, 9, x0=7, y0=5), 2)]
    regs += [(rt4.band_plan(33, 17, 3, rank, band=2)[0], 1) for rank in range(3)]
    whole, _ = t.render_light_host(us_pre + us, rt4.region(33, 17))
    for reg, extra in regs:
        w, h = reg.w, reg.h
        tiles = n_tiles_of(w, h)
        lst = sorted({0, tiles - 1, tiles // 2})
        start, _ = t.render_light_host(us_pre, reg)
        full, n_full = t.render_light_host(us, reg, start.copy())
        rows = region_rows(reg) if reg.band_rows else slice(reg.y0, reg.y0 + h)
        assert light_ref.same_acc(as_ref(full), as_ref(whole[rows, reg.x0:reg.x0 + w]))  # the region's own pixels
        acc = padded(rt4, start, extra)
        _, n = t.render_light_tiles_host(us, reg, lst, acc, row_stride_px=w + extra)
        mask = adaptive_ref.tile_mask(lst, w, h)
        check_listed(acc[:, :w], full, start, mask, (reg.x0, reg.y0, w, h, reg.band_rows, extra))
        assert padding_kept(acc, w) and 0 < n < n_full


# ------------------------------------------------------------------------------------------ 4. launches
def test_across_a_launch_boundary(rt4, tracers):
    """MAX_FRAMES + 1 frames of tile 1 of a 16 x 8 image: two launches, the fold of the per-frame lights."""
    t = tracers("default")
    t.set_scene(rt4.Scene.named("sphere"))
    w, h = 16, 8
    n = rt4.MAX_FRAMES + 1
    assert t.frames_per_launch(w, h) == rt4.MAX_FRAMES
    us = frame_uniforms(rt4, w, h, 1, n, spp=1)
    reg = rt4.region(w, h)
    singles = [t.render_light_host([u], reg)[0] for u in us]
    want = light_ref.fold(np.zeros((h, w), light_ref.LIGHT_DTYPE), [a["mean"] for a in singles])
    got, _ = t.render_light_tiles_host(us, reg, [1])
    assert light_ref.same_acc(as_ref(got[:, 8:]), np.ascontiguousarray(want[:, 8:])) and (got["n"][:, 8:] == n).all()
    assert not got[:, :8].view(np.uint8).any()


def test_frame_by_frame_scene(rt4, tracers):
    """scenes/tiger_two_mirrors.frag, the scene that once ran frame by frame, at 17 x 9: 3 frames of tiles {0, 2}."""
    import os

    t = tracers("default")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    t.set_scene(rt4.Scene.load_frag(os.path.join(root, "scenes", "tiger_two_mirrors.frag")))
    w, h = 17, 9
    reg = rt4.region(w, h)
    us = frame_uniforms(rt4, w, h, 1, 3)
    start = np.zeros((h, w), rt4.LIGHT_DTYPE)
    full, n_full = t.render_light_host(us, reg, start.copy())
    got, n = t.render_light_tiles_host(us, reg, [0, 2], start.copy())
    check_listed(got, full, start, adaptive_ref.tile_mask([0, 2], w, h), "two mirrors")
    one_by_one = start.copy()
    for u in us:  # and launch by launch
        t.render_light_tiles_host([u], reg, [0, 2], one_by_one)
    assert raw(one_by_one) == raw(got) and 0 < n < n_full


# ------------------------------------------------------------------------------------------ 5. errors
def test_argument_errors_write_nothing(rt4, tracers):
    import torch

    t = tracers("default")
    t.set_scene(rt4.Scene.named("sphere"))
    w, h = 16, 8
    u = rt4.make_uniforms(w, h, samples=1, reflections=1)
    buf = torch.full((9 * w, 8), 0.25, dtype=torch.float32, device="cuda")  # the accumulator rows 0..7, then the list
    lst = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    before = buf.cpu().numpy().copy()
    stream = torch.cuda.current_stream().cuda_stream
    light, tiles_ptr = buf.data_ptr(), lst.data_ptr()
    reg = rt4.region(w, h)

    def call(us=(u,), reg=reg, tiles=tiles_ptr, n=2, light=light, stride=w):
        try:
            t.render_light_tiles_device(list(us), reg, tiles, n, light, stride, cnt.data_ptr(), stream)
        except rt4.RT4Error as e:
            return e.status
        return 0

    def call_raw(us, n_frames):
        err = ctypes.create_string_buffer(256)
        return rt4.lib.rt4_render_light_tiles_device(t._h, us, n_frames, ctypes.byref(reg), tiles_ptr, 2, light, w, None, stream,
                                                     err, len(err))

    assert call(light=0) == ERR_ARG and call_raw(None, 1) == ERR_ARG
    assert call_raw((rt4.Uniforms * 1)(u), 0) == ERR_ARG
    assert call(n=-1) == ERR_ARG and call(n=3) == ERR_ARG  # 2 tiles
    assert call(tiles=0) == ERR_ARG and call(tiles=tiles_ptr + 2) == ERR_ARG
    assert call(tiles=0, n=0) == 0  # no list needed for no tiles
    assert call(light=light + 8) == ERR_ARG and call(stride=w - 1) == ERR_ARG
    assert call(reg=rt4.region(8192, 1), stride=8192) == ERR_ARG and call(reg=rt4.region(1, 8192), stride=1) == ERR_ARG
    u2 = rt4.Uniforms.from_buffer_copy(bytes(u))
    u2.samples = 2
    assert call(us=(u, u2)) == ERR_ARG
    assert call(reg=rt4.region(w, h, band_rows=2, band_step=1)) == ERR_ARG
    torch.cuda.synchronize()
    assert raw(buf.cpu().numpy()) == raw(before) and int(cnt.item()) == 0
    buf[:8 * w] = 0
    assert call() == 0
    torch.cuda.synchronize()
    acc = buf.cpu().numpy()[:8 * w].view(rt4.LIGHT_DTYPE).reshape(h, w)
    assert (acc["n"] == 1).all() and int(cnt.item()) > 0 and raw(buf.cpu().numpy()[8 * w:]) == raw(before[8 * w:])
    assert t.select_bytes() >= (2 + 2) * 4


# ------------------------------------------------------------------------------------------ 6. the context afterwards
@pytest.mark.parametrize("flag_name", ["default", "serial"])
def test_other_launches_after_tile_launches(rt4, tracers, oracle, flag_name):
    """rt4_render_device_ex (the serial context's uses the pre-pass order), rt4_render_frames_device and
    rt4_render_light_device between and after tile launches on the same context still match the oracle."""
    import torch

    t = tracers(flag_name)
    scene = rt4.Scene.named("sphere")
    t.set_scene(scene)
    w, h = 33, 17
    reg = rt4.region(w, h)
    base = rt4.make_uniforms(w, h, samples=2, reflections=3, seed=99)
    us = [rt4.progressive_uniforms(base, n) for n in range(1, 4)]
    stream = torch.cuda.current_stream().cuda_stream
    light = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
    light2 = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    single = torch.zeros((2, h, w, 4), dtype=torch.float32, device="cuda")
    lst = torch.tensor([14, 3, 0xFFFFFFF], dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    t.render_device_ex(us[0], reg, single[0].data_ptr(), 0, w, cnt[2:].data_ptr(), stream)  # makes the pre-pass order
    t.render_light_tiles_device(us, reg, lst.data_ptr(), 3, light.data_ptr(), w, cnt[0:].data_ptr(), stream)
    t.render_device_ex(us[0], reg, single[1].data_ptr(), 0, w, cnt[2:].data_ptr(), stream)  # reuses it
    t.render_frames_device(us, reg, frame.data_ptr(), 0, w, cnt[1:].data_ptr(), stream)
    t.render_light_tiles_device(us[:1], reg, lst.data_ptr(), 2, light.data_ptr(), w, cnt[0:].data_ptr(), stream)
    t.render_light_device(us, reg, light2.data_ptr(), w, cnt[3:].data_ptr(), stream)
    torch.cuda.synchronize()
    want, m = np.zeros((h, w, 4), np.float32), []
    for uf in us:
        m.append(oracle.render_fmt(scene.desc, uf, reg, 0, frame=want)[1])
    first, _ = oracle.render_fmt(scene.desc, us[0], reg, 0)
    assert raw(frame.cpu().numpy()) == raw(want)
    assert raw(single[0].cpu().numpy()) == raw(first) and raw(single[1].cpu().numpy()) == raw(first)
    counts = cnt.cpu().tolist()
    assert counts[1:] == [sum(m), 2 * m[0], sum(m)] and 0 < counts[0] < sum(m)
    acc = light.cpu().numpy().view(rt4.LIGHT_DTYPE).reshape(h, w)
    mask = adaptive_ref.tile_mask([14, 3], w, h)
    assert (acc["n"][mask] == 4).all() and not acc[~mask].view(np.uint8).any()
    full = light2.cpu().numpy().view(rt4.LIGHT_DTYPE).reshape(h, w)
    image = t.light_resolve_host(np.ascontiguousarray(full), base.light_to_color_conversion_coefficient)
    assert (full["n"] == 3).all() and image.shape == (h, w, 4)
    one, _ = t.render_light_host(us[:1], reg)
    assert raw(t.light_resolve_host(one, base.light_to_color_conversion_coefficient)) == raw(first)  # against the oracle
