"""numpy restatement of the variance-guided a-trous filter of include/rt4.h (rt4_light_denoise_device) — a plain
helper, not a test module.

  state0()         level 0: the surface id of every filterable pixel (else -1), L_0, Y_0, V_0
  level()          one level: the 3 x 3 variance pre-filter at unit stride, then the 25 taps at stride s
  light_denoise()  the frame in a format and the optional filtered light {L_r, L_g, L_b, V}

Everything is fp32 with one rounding per operation; the fused multiply-adds are denoise_ref.fma32 (exact), the dot
of the normals denoise_ref.dot4, the stored formats denoise_ref.encode, the pixels that are not filterable
light_ref.resolve. A NaN's payload is not defined: compare floats with light_ref.same_floats."""
import numpy as np

import light_ref
from denoise_ref import H5, dot4, encode, fma32

F32 = np.float32
MAX_LEVELS = 6
G3 = [F32(1 / 4), F32(1 / 2), F32(1 / 4)]
DEFAULTS = dict(levels=5, cos_min=0.9, depth_tol=0.1, max_refl_prob=0.5, sigma=4.0, eps=1e-6)


def variance0(acc):
    """V_0 = (m2 / (float)(n - 1)) / (float)n: the radicand of light_ref.noise's se. Meaningless where n < 2."""
    n = acc["n"].astype(np.int64)
    with np.errstate(all="ignore"):
        return ((acc["m2"] / (n - 1).astype(F32)) / n.astype(F32)).astype(F32)


def state0(acc, gbuf, max_refl_prob):
    """(id (h, w) int32, L (h, w, 3), Y (h, w), V (h, w)) of level 0."""
    with np.errstate(invalid="ignore"):
        filt = (gbuf["surface"] >= 0) & (gbuf["refl_prob"] <= F32(max_refl_prob)) & (acc["n"] >= 2)
    ids = np.where(filt, gbuf["surface"], -1).astype(np.int32)
    return ids, acc["mean"].astype(F32).copy(), acc["mean_y"].astype(F32).copy(), variance0(acc)


def _taps(h, w, dy, dx, step):
    ys, xs = np.mgrid[0:h, 0:w]
    qy, qx = ys + step * dy, xs + step * dx
    inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
    return np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1), inside


def level(L, Y, V, gbuf, ids, step, cos_min, depth_tol, sigma, eps):
    """(L, Y, V) of level l + 1 from level l, s = step."""
    h, w = ids.shape
    filt = ids >= 0
    n, z = gbuf["normal"], gbuf["depth"]
    with np.errstate(all="ignore"):
        # 1. the variance pre-filter at unit stride
        va, vw = np.zeros((h, w), F32), np.zeros((h, w), F32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                g = G3[dy + 1] * G3[dx + 1]
                qy, qx, inside = _taps(h, w, dy, dx, 1)
                counts = filt & (inside & (ids[qy, qx] == ids) if (dx or dy) else True)
                va = np.where(counts, va + g * V[qy, qx], va)  # a multiply, then an add
                vw = np.where(counts, vw + g, vw)
        den = fma32(F32(sigma), np.sqrt(va / vw), F32(eps)).reshape(h, w)
        # 2. the 25 taps
        tol = F32(depth_tol) * z
        aL, aY, aV, wsum = np.zeros((h, w, 3), F32), np.zeros((h, w), F32), np.zeros((h, w), F32), np.zeros((h, w), F32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                k = H5[dy + 2] * H5[dx + 2]
                qy, qx, inside = _taps(h, w, dy, dx, step)
                om = np.full((h, w), k, F32)
                if dx == 0 and dy == 0:
                    counts = filt.copy()
                else:
                    counts = filt & inside & (ids[qy, qx] == ids)
                    idx = np.nonzero(counts)  # the fma chains only where the cheap conditions hold
                    qi = (qy[idx], qx[idx])
                    geo = (dot4(n[idx], n[qi]) >= F32(cos_min)) & (np.abs(z[qi] - z[idx]) <= tol[idx])
                    t = np.abs(Y[qi] - Y[idx]) / den[idx]
                    wl = F32(1.0) / fma32(t, t, F32(1.0))
                    o = k * wl
                    om[idx] = o
                    counts[idx] = geo & (o > 0)  # false for NaN
                aL = np.where(counts[..., None], aL + om[..., None] * L[qy, qx], aL)
                aY = np.where(counts, aY + om * Y[qy, qx], aY)
                aV = np.where(counts, aV + (om * om) * V[qy, qx], aV)
                wsum = np.where(counts, wsum + om, wsum)
        # 3.
        Ln, Yn, Vn = L.copy(), Y.copy(), V.copy()
        Ln[filt] = aL[filt] / wsum[filt][:, None]
        Yn[filt] = aY[filt] / wsum[filt]
        Vn[filt] = aV[filt] / (wsum[filt] * wsum[filt])
    return Ln, Yn, Vn


def filter_light(acc, gbuf, levels=5, cos_min=0.9, depth_tol=0.1, max_refl_prob=0.5, sigma=4.0, eps=1e-6):
    """(id, L_levels, V_levels): the filtered light of every pixel (a pixel that is not filterable keeps level 0)."""
    ids, L, Y, V = state0(acc, gbuf, max_refl_prob)
    for l in range(levels):
        L, Y, V = level(L, Y, V, gbuf, ids, 1 << l, cos_min, depth_tol, sigma, eps)
    return ids, L, V


def light_denoise(acc, gbuf, k, dtype=np.float32, **params):
    """(frame (h, w, 4) of dtype, filtered (h, w, 4) float32) of rt4_light_denoise_device."""
    p = dict(DEFAULTS)
    p.update(params)
    ids, L, V = filter_light(acc, gbuf, **p)
    filt = ids >= 0
    h, w = ids.shape
    frame = light_ref.resolve(acc, k, dtype)
    with np.errstate(all="ignore"):
        c = light_ref.tone(k, L).reshape(h, w, 3)
        c = fma32(c, F32(1.0), F32(0.0)).reshape(h, w, 3)  # the store rule: the blend with part 1 into a zero pixel
        frame[..., :3] = np.where(filt[..., None], encode(c, dtype), frame[..., :3])
    filtered = np.empty((h, w, 4), F32)
    filtered[..., :3] = L
    filtered[..., 3] = np.where(filt, V, np.where(acc["n"] >= 2, variance0(acc), F32(np.inf)))
    return frame, filtered
