"""numpy restatement of rt4_light_merge_device of include/rt4.h — a plain helper, not a test module.

  merge(a, b)           accumulator b merged into a copy of accumulator a (Chan's pairwise update)
  merge_all(dst, srcs)  the left fold merge(... merge(merge(dst, srcs[0]), srcs[1]) ...)

fp32 with one rounding per operation, the fused multiply-adds exact (denoise_ref.fma32), as light_ref.py."""
import numpy as np

from denoise_ref import fma32
from light_ref import F32, INT32_MAX


def merge(a, b):
    """(h, w) of LIGHT_DTYPE: b.n == 0 keeps a, else a.n == 0 takes b, else the pairwise update; reserved = 0."""
    out = a.copy()
    na, nb = a["n"].astype(np.int64), b["n"].astype(np.int64)
    N = na + nb
    with np.errstate(all="ignore"):
        fb = nb.astype(F32) / N.astype(F32)
        wa = na.astype(F32) * fb
        mean = np.empty_like(a["mean"])
        for c in range(3):
            mean[..., c] = fma32(b["mean"][..., c] - a["mean"][..., c], fb, a["mean"][..., c])
        dy = b["mean_y"] - a["mean_y"]
        mean_y = fma32(dy, fb, a["mean_y"])
        m2 = fma32(dy * dy, wa, a["m2"] + b["m2"])
    take_b = (nb != 0) & (na == 0)
    both = (nb != 0) & (na != 0)
    for name, val in (("mean_y", mean_y), ("m2", m2)):
        out[name] = np.where(both, np.asarray(val, F32).reshape(a.shape), np.where(take_b, b[name], a[name]))
    out["mean"] = np.where(both[..., None], np.asarray(mean, F32).reshape(a["mean"].shape),
                           np.where(take_b[..., None], b["mean"], a["mean"]))
    out["n"] = np.where(nb == 0, na, np.minimum(N, INT32_MAX)).astype(np.int32)
    out["reserved"] = 0
    return out


def merge_all(dst, srcs):
    """The sources merged into a copy of dst in order."""
    for s in srcs:
        dst = merge(dst, s)
    return dst
