"""rt4_light_select_tiles_device on the GPU (rt4.h) against adaptive_ref.select_tiles, exactly: the
list (ascending), the count and the state per tile, for accumulators no renderer made and a rendered one, the edges of
every parameter, dilation at the grid's borders, shapes on both sides of the compaction's chunk, and the outputs' bytes."""
import numpy as np
import pytest

import adaptive_ref
import light_ref
from adaptive_ref import Params
from test_gpu_light import synthetic_acc, thresholds_of

pytestmark = pytest.mark.gpu

ERR_ARG = -1
CHUNK = 1024  # rt4_light_tiles.h SELECT_CHUNK: tiles per step of the compaction


def raw(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.fixture(scope="module")
def t(rt4):
    tr = rt4.Tracer(device=0)
    yield tr
    tr.close()


def check(rt4, t, acc, k, p, what=None, w=None):
    """The library's selection of acc (its left w columns) equals the reference's; returns (tiles, state)."""
    img = np.ascontiguousarray(acc if w is None else acc[:, :w])
    want_tiles, want_state = adaptive_ref.select_tiles(img.view(light_ref.LIGHT_DTYPE), k, p)
    params = rt4.tile_select_params(p.threshold, p.min_above, p.min_frames, p.dilate)
    tiles, state = t.light_select_tiles_host(np.ascontiguousarray(acc).view(rt4.LIGHT_DTYPE), k, params, w=w)
    assert tiles.dtype == np.uint32 and tiles.tolist() == want_tiles.tolist(), (what, p)
    assert raw(state) == raw(want_state), (what, p)
    return tiles, state


def quiet(h, w, n=16):
    acc = np.zeros((h, w), light_ref.LIGHT_DTYPE)
    acc["n"] = n
    acc["mean_y"] = 0.5
    acc["mean"] = 0.5
    return acc


def hot_tile(acc, tile, count=64):
    """`count` hot pixels (as many as the tile has inside the image, at most) in a tile."""
    tx = (acc.shape[1] + 7) // 8
    y0, x0 = 8 * (tile // tx), 8 * (tile % tx)
    idx = np.arange(count)
    ys, xs = y0 + idx // 8, x0 + idx % 8
    ok = (ys < acc.shape[0]) & (xs < acc.shape[1])
    acc["m2"][ys[ok], xs[ok]] = 100.0


# ------------------------------------------------------------------------------------------ accumulators
@pytest.mark.parametrize("k", [1.0, 0.7])
def test_synthetic_accumulator(rt4, t, k):
    acc = synthetic_acc()
    assert set(np.unique(acc["n"])) >= {0, 1, 2, light_ref.INT32_MAX} and np.isnan(acc["m2"]).any() and np.isinf(acc["m2"]).any()
    seen = set()
    for thr in thresholds_of(acc, k) + [-1.0, float("inf")]:
        for min_above in (1, 8, 30):
            for min_frames in (0, 3):
                for dilate in (0, 1):
                    tiles, _ = check(rt4, t, acc, k, Params(thr, min_above, min_frames, dilate), "synthetic")
                    seen.add(len(tiles))
    assert 0 in seen and 15 in seen and len(seen) > 3  # nothing, everything and lists in between


def test_rendered_accumulator(rt4, t):
    t.set_scene(rt4.Scene.named("sphere"))
    w, h = 33, 17
    us = [rt4.make_uniforms(w, h, samples=2, reflections=3, seed=s) for s in range(1, 9)]
    acc, _ = t.render_light_host(us, rt4.region(w, h))
    lens = []
    for thr in thresholds_of(acc.view(light_ref.LIGHT_DTYPE), 1.0):
        for min_above in (1, 4, 16):
            for dilate in (0, 1, 2):
                lens.append(len(check(rt4, t, acc, 1.0, Params(thr, min_above, 8, dilate), "rendered")[0]))
    print(sorted(set(lens)))
    assert min(lens) == 0 and max(lens) >= 10 and len(set(lens)) > 3
    assert len(check(rt4, t, acc, 1.0, Params(1.0, 1, 9, 0), "all young")[0]) == 15


# ------------------------------------------------------------------------------------------ parameter edges
def test_threshold_equal_to_a_q(rt4, t):
    acc = quiet(8, 16)
    acc["m2"][0, 0], acc["m2"][0, 8] = 100.0, 1.0
    q = light_ref.noise(acc, 1.0, 0.0)[1]
    assert check(rt4, t, acc, 1.0, Params(float(q[0, 8]), 1, 0, 0))[0].tolist() == [0]
    assert check(rt4, t, acc, 1.0, Params(float(np.nextafter(q[0, 8], np.float32(0))), 1, 0, 0))[0].tolist() == [0, 1]


@pytest.mark.parametrize("min_above", [1, 3, 64])
def test_min_above_exactly_and_one_fewer(rt4, t, min_above):
    acc = quiet(8, 16)
    hot_tile(acc, 0, min_above)
    hot_tile(acc, 1, min_above - 1)
    assert check(rt4, t, acc, 1.0, Params(0.01, min_above, 0, 0))[0].tolist() == [0]


@pytest.mark.parametrize("min_frames", [0, 2, 5])
def test_min_frames_with_one_pixel_at_four(rt4, t, min_frames):
    acc = quiet(8, 24)
    acc["n"][7, 23] = 4
    tiles, state = check(rt4, t, acc, 1.0, Params(0.01, 1, min_frames, 0))
    assert tiles.tolist() == ([2] if min_frames > 4 else [])


def test_poisoned_row_padding(rt4, t):
    """The padding of a padded row never counts: young and hot records there, a 9 x 9 image in rows of 12."""
    wide = quiet(9, 12)
    wide["m2"][:, 9:] = 100.0
    wide["n"][:, 10:] = 0
    assert check(rt4, t, wide, 1.0, Params(0.01, 1, 8, 2), w=9)[0].tolist() == []
    wide["m2"][8, 8] = 100.0  # the one pixel of the corner tile
    assert check(rt4, t, wide, 1.0, Params(0.01, 1, 8, 0), w=9)[0].tolist() == [3]
    assert check(rt4, t, wide, 1.0, Params(0.01, 2, 8, 0), w=9)[0].tolist() == []


# ------------------------------------------------------------------------------------------ dilation
@pytest.mark.parametrize("dilate", [0, 1, 2])
@pytest.mark.parametrize("tile", [0, 4, 14, 7, 5, 9])  # 5 x 3 tiles: corners, the ends of tile rows, inside
def test_dilation(rt4, t, tile, dilate):
    acc = quiet(17, 33)
    hot_tile(acc, tile)
    tiles, state = check(rt4, t, acc, 1.0, Params(0.01, 1, 0, dilate), tile)
    ty, tx = divmod(tile, 5)
    assert len(tiles) == (min(tx + dilate, 4) - max(tx - dilate, 0) + 1) * (min(ty + dilate, 2) - max(ty - dilate, 0) + 1)
    assert state[ty, tx] == 2 and (state == 2).sum() == 1


# ------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize("w, h", [(1, 1), (8, 8), (9, 9), (64, 1), (1, 64), (33, 17)])
def test_shapes(rt4, t, w, h):
    rng = np.random.default_rng(w * 100 + h)
    acc = quiet(h, w)
    acc["m2"] = np.where(rng.random((h, w)) < 0.3, 100.0, 0.0).astype(np.float32)
    acc["n"] = rng.choice([1, 4, 16], (h, w), p=[0.02, 0.08, 0.9]).astype(np.int32)
    for p in (Params(0.01, 1, 0, 0), Params(0.01, 20, 2, 0), Params(0.01, 3, 5, 1), Params(0.01, 64, 0, 2)):
        check(rt4, t, acc, 1.0, p, (w, h))
    assert len(check(rt4, t, quiet(h, w), 1.0, Params(0.01, 1, 16, 2))[0]) == 0
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    assert check(rt4, t, quiet(h, w), 1.0, Params(0.01, 1, 17, 0))[0].tolist() == list(range(tiles))


@pytest.mark.parametrize("dilate", [0, 1])
def test_1025_tiles_in_a_row(rt4, t, dilate):
    """8200 x 8: one tile row of 1025 tiles, one more than the compaction's chunk."""
    acc = quiet(8, 8200)
    marks = [0, 255, 256, 511, 512, CHUNK - 1, CHUNK]
    for m in marks:
        hot_tile(acc, m, 3)
    tiles, _ = check(rt4, t, acc, 1.0, Params(0.01, 3, 0, dilate), "8200x8")
    assert set(marks) <= set(tiles.tolist()) and len(tiles) == (len(marks) if dilate == 0 else 2 + 4 + 4 + 3)
    only_last = quiet(8, 8200)
    hot_tile(only_last, CHUNK)
    assert check(rt4, t, only_last, 1.0, Params(0.01, 1, 0, 0))[0].tolist() == [CHUNK]
    assert len(check(rt4, t, quiet(8, 8200), 1.0, Params(0.01, 1, 17, 0))[0]) == CHUNK + 1  # every tile


@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_33_by_33_tiles(rt4, t, dilate):
    """264 x 264: 1089 tiles, dilation across tile rows and across the chunk boundary (tile 1024 is row 31, column 1)."""
    acc = quiet(264, 264)
    for m in (0, 32, 33, 31 * 33, 31 * 33 + 1, 32 * 33 + 32, 16 * 33 + 16, 30 * 33 + 32):
        hot_tile(acc, m, 2)
    tiles, state = check(rt4, t, acc, 1.0, Params(0.01, 2, 0, dilate), "264x264")
    assert (state == 2).sum() == 8 and (tiles < CHUNK).any() and (tiles >= CHUNK).any()


# ------------------------------------------------------------------------------------------ outputs
def device_select(rt4, t, acc, k, p, d_tiles, d_count, d_state):
    import torch

    h, w = acc.shape
    d_acc = torch.from_numpy(acc.view(np.uint8).reshape(h, w * 32).copy()).cuda()
    params = rt4.tile_select_params(p.threshold, p.min_above, p.min_frames, p.dilate)
    t.light_select_tiles_device(d_acc.data_ptr(), w, w, h, k, params, d_tiles.data_ptr(), d_count.data_ptr(),
                                d_state.data_ptr() if d_state is not None else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert raw(d_acc.cpu().numpy()) == raw(acc)  # read only
    return d_tiles.cpu().numpy().view(np.uint32), int(d_count.cpu().numpy().view(np.uint32)[0])


def test_outputs(rt4, t):
    """Entries past the count keep their poison; the state given and NULL; two calls into the same buffers."""
    import torch

    acc = synthetic_acc()
    k = 1.0
    thr = thresholds_of(acc, k)[1]
    d_tiles = torch.full((15,), -7, dtype=torch.int32, device="cuda")
    d_count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    d_state = torch.full((15,), -7, dtype=torch.int32, device="cuda")
    p1, p2 = Params(thr, 4, 0, 0), Params(thr, 12, 0, 0)
    w1, s1 = adaptive_ref.select_tiles(acc, k, p1)
    w2, s2 = adaptive_ref.select_tiles(acc, k, p2)
    assert 0 < len(w2) < len(w1) < 15
    tiles, n = device_select(rt4, t, acc, k, p1, d_tiles, d_count, d_state)
    assert n == len(w1) and tiles[:n].tolist() == w1.tolist() and (tiles[n:].view(np.int32) == -7).all()
    assert raw(d_state.cpu().numpy()) == raw(s1)
    # a second, shorter selection into the same buffers, without the state: the first one's tail and state stay
    tiles, n = device_select(rt4, t, acc, k, p2, d_tiles, d_count, None)
    assert n == len(w2) and tiles[:n].tolist() == w2.tolist() and tiles[n:len(w1)].tolist() == w1[n:].tolist()
    assert (tiles[len(w1):].view(np.int32) == -7).all() and raw(d_state.cpu().numpy()) == raw(s1)
    assert t.select_bytes() >= 15 * 4


def test_scratch_grows_with_the_tiles(rt4):
    tr = rt4.Tracer(device=0)
    try:
        assert tr.select_bytes() == 0
        tr.light_select_tiles_host(quiet(8, 16).view(rt4.LIGHT_DTYPE), 1.0)
        assert tr.select_bytes() == 2 * 4
        tr.light_select_tiles_host(quiet(17, 33).view(rt4.LIGHT_DTYPE), 1.0)
        assert tr.select_bytes() == 15 * 4
        tr.light_select_tiles_host(quiet(8, 16).view(rt4.LIGHT_DTYPE), 1.0)
        assert tr.select_bytes() == 15 * 4
    finally:
        tr.close()


def test_defaults(rt4):
    p = rt4.tile_select_params()
    d = Params()
    assert (np.float32(p.threshold), p.min_above, p.min_frames, p.dilate) == (np.float32(d.threshold), d.min_above, d.min_frames, d.dilate)
    assert (rt4.ADAPTIVE_WARMUP, rt4.ADAPTIVE_PASS_FRAMES, rt4.ADAPTIVE_FULL_EVERY) == (adaptive_ref.WARMUP, adaptive_ref.PASS_FRAMES,
                                                                                         adaptive_ref.FULL_EVERY)


# ------------------------------------------------------------------------------------------ errors
def test_argument_errors_write_nothing(rt4, t):
    import torch

    w, h = 16, 8
    # rows of w 32-B records: the accumulator rows 0..7, then the list, the count and the state in row 8
    buf = torch.full((9 * w, 8), 0.25, dtype=torch.float32, device="cuda")
    before = buf.cpu().numpy().copy()
    stream = torch.cuda.current_stream().cuda_stream
    row = w * 32
    light = buf.data_ptr()
    tiles, count, state = light + 8 * row, light + 8 * row + 64, light + 8 * row + 128

    def call(light=light, ls=w, ww=w, hh=h, p=None, tiles=tiles, count=count, state=state):
        try:
            t.light_select_tiles_device(light, ls, ww, hh, 1.0, p, tiles, count, state, stream)
        except rt4.RT4Error as e:
            return e.status
        return 0

    P = rt4.tile_select_params
    assert call(light=0) == ERR_ARG and call(tiles=0) == ERR_ARG and call(count=0) == ERR_ARG
    assert call(ls=w - 1) == ERR_ARG and call(ww=0) == ERR_ARG and call(hh=65536) == ERR_ARG
    assert call(light=light + 8) == ERR_ARG and call(tiles=tiles + 2) == ERR_ARG and call(count=count + 1) == ERR_ARG
    assert call(state=state + 2) == ERR_ARG
    assert call(p=P(threshold=float("nan"))) == ERR_ARG
    assert call(p=P(min_above=0)) == ERR_ARG and call(p=P(min_above=65)) == ERR_ARG
    assert call(p=P(min_frames=-1)) == ERR_ARG
    assert call(p=P(dilate=-1)) == ERR_ARG and call(p=P(dilate=rt4.SELECT_MAX_DILATE + 1)) == ERR_ARG
    assert call(tiles=light + 8 * row - 4) == ERR_ARG and call(count=light) == ERR_ARG and call(state=light + 64) == ERR_ARG
    assert call(count=tiles + 4) == ERR_ARG and call(state=tiles) == ERR_ARG and call(state=count - 4) == ERR_ARG
    torch.cuda.synchronize()
    assert raw(buf.cpu().numpy()) == raw(before)
    # adjacent, not overlapping: accepted (the list right behind the accumulator, the count right behind the list)
    assert call(count=tiles + 8, state=tiles + 12) == 0 and call(state=0) == 0
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert raw(after[:8 * w]) == raw(before[:8 * w])
    words = after[8 * w:].view(np.uint32).reshape(-1)  # the list in words 0..1, the count in 2, the state in 3..4
    want, want_state = adaptive_ref.select_tiles(before[:8 * w].view(light_ref.LIGHT_DTYPE).reshape(h, w), 1.0, Params())
    assert words[2] == len(want) and words[:words[2]].tolist() == want.tolist()
    assert words[3:5].view(np.int32).tolist() == want_state.reshape(-1).tolist()
