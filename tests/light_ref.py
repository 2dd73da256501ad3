"""numpy restatement of the light accumulator of include/rt4.h (rt4_light_px, rt4_light_resolve_device,
rt4_light_noise_device) — a plain helper, not a test module.

  fold()     frames of light (light sum / samples) applied in order to an accumulator
  resolve()  the accumulator's image in a frame format
  noise()    the standard-error map, the display-error map q, `above` per 8x8 tile and the statistics

Everything is fp32 with one rounding per operation; the fused multiply-adds are denoise_ref.fma32 (exact), the stored
formats denoise_ref.encode. The accumulator is a numpy array of LIGHT_DTYPE (rt4.LIGHT_DTYPE has the same layout)."""
import numpy as np

from denoise_ref import encode, fma32

F32 = np.float32
INT32_MAX = 2 ** 31 - 1
LIGHT_DTYPE = np.dtype([("mean", "<f4", (3,)), ("mean_y", "<f4"), ("m2", "<f4"), ("n", "<i4"), ("reserved", "<f4", (2,))])
LUMA = (F32(0.2126), F32(0.7152), F32(0.0722))


def light_of(light_sum, samples):
    """x = L / (float)samples, the division of the tone map."""
    with np.errstate(all="ignore"):
        return np.asarray(light_sum, F32) / F32(samples)


def luminance(x):
    with np.errstate(all="ignore"):
        return fma32(LUMA[0], x[..., 0], fma32(LUMA[1], x[..., 1], LUMA[2] * x[..., 2]))


def apply(acc, x):
    """One frame of light x (h, w, 3) float32 folded into a copy of acc (h, w) of LIGHT_DTYPE."""
    out = acc.copy()
    x = np.asarray(x, F32)
    with np.errstate(all="ignore"):
        y = luminance(x)
        n1 = np.minimum(acc["n"].astype(np.int64) + 1, INT32_MAX)
        inv = F32(1.0) / n1.astype(F32)
        for c in range(3):
            out["mean"][..., c] = fma32(x[..., c] - acc["mean"][..., c], inv, acc["mean"][..., c])
        dy = y - acc["mean_y"]
        out["mean_y"] = fma32(dy, inv, acc["mean_y"])
        out["m2"] = fma32(dy, y - out["mean_y"], acc["m2"])
    out["n"] = n1.astype(np.int32)
    out["reserved"] = 0
    return out


def fold(acc, xs):
    """The frames xs applied in order."""
    for x in xs:
        acc = apply(acc, x)
    return acc


def tone(k, v):
    with np.errstate(all="ignore"):
        return F32(1.0) - F32(1.0) / fma32(F32(k), v, F32(1.0))


def resolve(acc, k, dtype=np.float32):
    """(h, w, 4) of dtype: 1 - 1/fma(k, mean, 1) stored by the format's rule with alpha 1; n == 0 gives colour 0."""
    h, w = acc.shape
    c = np.where((acc["n"] == 0)[..., None], F32(0), tone(k, acc["mean"]).reshape(h, w, 3))
    c = fma32(c, F32(1.0), F32(0.0)).reshape(h, w, 3)  # the blend with part 1 into a zero pixel
    out = np.empty((h, w, 4), dtype)
    with np.errstate(all="ignore"):
        out[..., :3] = encode(c, dtype)
    out[..., 3] = 255 if dtype == np.uint8 else 1
    return out


def noise(acc, k, threshold):
    """(se (h, w) float32, q (h, w) float32, tile_above (ceil(h/8), ceil(w/8)) int32, stats dict)."""
    h, w = acc.shape
    n = acc["n"].astype(np.int64)
    measured = n >= 2
    with np.errstate(all="ignore"):
        se_m = np.sqrt((acc["m2"] / (n - 1).astype(F32)) / n.astype(F32)).astype(F32)
        q_m = tone(k, acc["mean_y"] + se_m).reshape(h, w) - tone(k, acc["mean_y"]).reshape(h, w)
        se = np.where(measured, se_m, F32(np.inf)).astype(F32)
        q = np.where(measured, q_m, F32(np.inf)).astype(F32)
        above = measured & (q > F32(threshold))  # false for NaN
        vq = np.where(measured & (q > 0), q, F32(0))  # the maxima start from 0 and ignore NaN
        vse = np.where(measured & (se > 0), se, F32(0))
    tiles = np.zeros(((h + 7) // 8, (w + 7) // 8), np.int32)
    for ty in range(tiles.shape[0]):
        for tx in range(tiles.shape[1]):
            tiles[ty, tx] = above[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].sum()
    stats = {"pixels": h * w, "measured": int(measured.sum()), "above": int(above.sum()), "max_q": float(vq.max()),
             "max_se": float(vse.max())}
    return se, q, tiles, stats


def same_floats(a, b):
    """Bit-equal float32 arrays, any NaN matching any NaN (rt4.h leaves a NaN's payload undefined)."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def same_acc(a, b):
    """Bit-equal accumulators up to NaN payloads."""
    return (a.shape == b.shape and np.array_equal(a["n"], b["n"]) and same_floats(a["mean"], b["mean"])
            and same_floats(a["mean_y"], b["mean_y"]) and same_floats(a["m2"], b["m2"])
            and np.array_equal(a["reserved"].view(np.uint32), b["reserved"].view(np.uint32)))
