"""numpy restatement of adaptive light sampling of include/rt4.h (rt4_light_select_tiles_device, the loop of
Tracer.render_light_adaptive and rt4_render --light --adaptive) — a plain helper, not a test module.

  select_tiles()  the selected 8x8 tiles of an accumulator, ascending, and the state per tile
  tile_mask()     the pixels of a tile list
  adaptive()      the loop over a callable that yields a frame's light

Built on light_ref (noise() gives the hot count per tile, apply() one frame)."""
from dataclasses import dataclass

import numpy as np

import light_ref

MAX_DILATE = 2


@dataclass
class Params:  # rt4.h rt4_tile_select_params; the defaults of rt4_tile_select_params_default
    threshold: float = float(np.float32(1.0) / np.float32(255.0))
    min_above: int = 4
    min_frames: int = 8
    dilate: int = 1


# the loop's defaults (rt4.ADAPTIVE_WARMUP, ADAPTIVE_PASS_FRAMES, ADAPTIVE_FULL_EVERY)
WARMUP, PASS_FRAMES, FULL_EVERY = 8, 4, 4


def select_tiles(acc, k, params):
    """(tiles uint32 ascending, state int32 (ceil(h/8), ceil(w/8))) of an accumulator (h, w) of LIGHT_DTYPE: state 2 for
    a tile that qualifies (a pixel with n < min_frames, or at least min_above pixels with n >= 2 and q > threshold), 1
    for a tile within `dilate` tiles of one (inside the grid), else 0."""
    assert params.threshold == params.threshold and 1 <= params.min_above <= 64 and params.min_frames >= 0
    assert 0 <= params.dilate <= MAX_DILATE
    h, w = acc.shape
    hot = light_ref.noise(acc, k, params.threshold)[2]
    ty, tx = hot.shape
    young = np.zeros((ty, tx), bool)
    for y in range(ty):
        for x in range(tx):
            young[y, x] = (acc["n"][8 * y:8 * y + 8, 8 * x:8 * x + 8] < params.min_frames).any()
    qual = young | (hot >= params.min_above)
    near = np.zeros((ty, tx), bool)
    d = params.dilate
    for y in range(ty):
        for x in range(tx):
            near[y, x] = qual[max(y - d, 0):y + d + 1, max(x - d, 0):x + d + 1].any()
    state = np.where(qual, 2, np.where(near, 1, 0)).astype(np.int32)
    return np.flatnonzero(state.reshape(-1)).astype(np.uint32), state


def tile_mask(tiles, w, h):
    """(h, w) bool: the pixels of the listed tiles (numbers >= the tile count are ignored)."""
    tx, ty = (w + 7) // 8, (h + 7) // 8
    m = np.zeros((h, w), bool)
    for t in np.asarray(tiles, np.int64):
        if t < tx * ty:
            y, x = divmod(int(t), tx)
            m[8 * y:8 * y + 8, 8 * x:8 * x + 8] = True
    return m


def adaptive(frame_light, w, h, k, budget_frames, params=None, warmup=WARMUP, pass_frames=PASS_FRAMES,
             full_every=FULL_EVERY, acc=None):
    """The adaptive loop. frame_light(g) -> the light (h, w, 3) float32 of frame g = 1, 2, ... (the frame
    rt4_progressive_uniforms(base, g) renders). Returns (acc, log, frames): log a list of (kind, listed tiles, frames)
    with kind "warmup", "full", "empty" or "tiles"; frames the number of frame numbers used."""
    params = Params() if params is None else Params(**vars(params))
    if acc is None:
        acc = np.zeros((h, w), light_ref.LIGHT_DTYPE)
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    budget = budget_frames * tiles
    spent, g, log = 0, 0, []

    def run(n, mask):
        nonlocal acc, g
        for _ in range(n):
            g += 1
            new = light_ref.apply(acc, frame_light(g))
            acc = new if mask is None else np.where(mask, new, acc)

    warm = min(warmup, budget_frames)
    params.min_frames = warm
    if warm > 0:
        run(warm, None)
        spent += warm * tiles
        log.append(("warmup", tiles, warm))
    n_pass = 0
    while True:
        n_pass += 1
        kind, listed, mask = "full", tiles, None
        if not (full_every > 0 and n_pass % full_every == 0):
            lst, _ = select_tiles(acc, k, params)
            if len(lst) == 0:
                kind = "empty"
            else:
                kind, listed, mask = "tiles", len(lst), tile_mask(lst, w, h)
        n = min(pass_frames, (budget - spent) // listed)
        if n <= 0:
            break
        run(n, mask)
        spent += n * listed
        log.append((kind, listed, n))
    return acc, log, g
