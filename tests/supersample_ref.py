"""numpy restatement of rt4_light_downsample_device of include/rt4.h — a plain helper, not a test module.

  downsample(fine, s)  the (h*s, w*s) accumulator's s x s strata into the (h, w) accumulator
  variance(fine, s)    the pixel's variance in float64: the sum of the strata's se^2 over s^4 (what m2' encodes)

fp32 with one rounding per operation, on light_ref's types. Unlike the fold and the merge this definition has no fused
multiply-add (nothing here needs denoise_ref.fma32): every sum, product and quotient below is numpy's own float32
operation, correctly rounded, denormals kept."""
import numpy as np

from light_ref import F32, LIGHT_DTYPE

SUPERSAMPLE_MAX = 8


def strata(fine, s):
    """The strata of every output pixel in the definition's order i = b*s + a: (s*s, h, w) views of fine."""
    assert 1 <= s <= SUPERSAMPLE_MAX and fine.shape[0] % s == 0 and fine.shape[1] % s == 0
    return [fine[b::s, a::s] for b in range(s) for a in range(s)]


def downsample(fine, s):
    """(h, w) of LIGHT_DTYPE from fine (h*s, w*s): equal-weight means, n' = min n, m2' so that the noise map's se is the
    root of sum se_i^2 / s^4; a pixel with an unsampled stratum is the empty accumulator."""
    fine = np.ascontiguousarray(fine).view(LIGHT_DTYPE)
    parts = strata(fine, s)
    h, w = parts[0].shape
    inv = F32(1.0) / F32(s * s)
    out = np.zeros((h, w), LIGHT_DTYPE)
    nmin = parts[0]["n"].copy()
    for p in parts[1:]:
        nmin = np.minimum(nmin, p["n"])
    with np.errstate(all="ignore"):
        mean = np.zeros((h, w, 3), F32)
        mean_y = np.zeros((h, w), F32)
        sv = np.zeros((h, w), F32)
        for p in parts:
            mean = mean + p["mean"]
            mean_y = mean_y + p["mean_y"]
            n = p["n"].astype(np.int64)
            sv = sv + (p["m2"] / (n - 1).astype(F32)) / n.astype(F32)
        mean, mean_y = mean * inv, mean_y * inv
        var = (sv * inv) * inv
        m2 = (var * nmin.astype(F32)) * (nmin.astype(np.int64) - 1).astype(F32)
    live = nmin > 0
    out["mean"] = np.where(live[..., None], mean, F32(0))
    out["mean_y"] = np.where(live, mean_y, F32(0))
    out["m2"] = np.where(nmin >= 2, m2, F32(0))
    out["n"] = np.where(live, nmin, 0)
    return out


def variance(fine, s):
    """float64 (h, w): sum_i se_i^2 / s^4 from the strata's m2 and n (inf where a stratum has n < 2)."""
    fine = np.ascontiguousarray(fine).view(LIGHT_DTYPE)
    total = 0.0
    with np.errstate(all="ignore"):
        for p in strata(fine, s):
            n = p["n"].astype(np.float64)
            total = total + np.where(n >= 2, p["m2"].astype(np.float64) / (n - 1) / n, np.inf)
    return total / float(s) ** 4
