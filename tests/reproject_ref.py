"""numpy restatement of the temporal reprojection and the per-pixel blend of include/rt4.h (rt4_reproject_device,
rt4_temporal_blend_device) — a plain helper, not a test module.

  reproject()   steps 1-6 of the definition, vectorised over the image
  blend()       the per-pixel progressive blend
  POSES / pose_uniforms()   the camera moves the tests share

Everything is fp32 with one rounding per operation; the multiply-adds go through denoise_ref.fma32 (single-rounded).
"""
import types

import numpy as np

from denoise_ref import F32, decode, dot4, encode, fma32, primary_rays

INT32_MAX = np.int32(2 ** 31 - 1)
DEFAULTS = dict(cos_min=0.9, plane_tol=0.02, slice_tol=0.01, max_refl_prob=0.5, max_history=255)

# (name, kind, amount): the camera of the new view relative to the default camera of rt4.make_uniforms. Moves are
# in scene units along x, the viewing direction, the image's up direction and w; rotations in radians.
POSES = [("identity", "x", 0.0), ("x+0.05", "x", 0.05), ("x+0.3", "x", 0.3), ("forward+0.2", "forward", 0.2),
         ("up+0.1", "up", 0.1), ("fi+0.05", "fi", 0.05), ("te+0.05", "te", 0.05),
         ("w+0.3", "w", 0.3), ("psi+0.2", "psi", 0.2), ("w+0.05", "w", 0.05)]
KEPT = ["identity", "x+0.05", "x+0.3", "forward+0.2", "up+0.1", "fi+0.05", "te+0.05"]  # kept share >= 0.9
DROPPED = ["w+0.3", "psi+0.2"]  # kept share <= 0.15
PARTIAL = ["w+0.05"]  # strictly between


def pose_uniforms(rt4, w, h, kind, amount, **kw):
    """The uniforms of the default camera moved or rotated by `amount` (kw: samples, reflections, seed)."""
    kw = dict(dict(samples=4, reflections=4, seed=12345), **kw)
    base = rt4.make_uniforms(w, h, **kw)
    focus = np.array(list(base.focus), np.float64)
    if kind in ("fi", "te", "psi"):
        return rt4.make_uniforms(w, h, **kw, **{kind: float(np.degrees(amount))})
    if kind == "x":
        focus[0] += amount
    elif kind == "w":
        focus[3] += amount
    elif kind == "forward":
        f = np.array(list(base.vec_to_mtr), np.float64)
        focus += amount * f / np.linalg.norm(f)
    elif kind == "up":
        focus += amount * np.array(list(base.top_drct), np.float64)
    else:
        raise ValueError(kind)
    return rt4.make_uniforms(w, h, **kw, focus=tuple(float(F32(v)) for v in focus))


def _vec(v):
    return np.array(list(v), F32)


def _directions(u, w, h):
    return primary_rays(u, types.SimpleNamespace(x0=0, y0=0, w=w, h=h, band_rows=0, band_step=0))[..., 4:]


def reproject(u_cur, g_cur, u_prev, g_prev, acc_prev, hist_prev, cos_min=0.9, plane_tol=0.02, slice_tol=0.01,
              max_refl_prob=0.5, max_history=255, details=False):
    """(acc_out, hist_out) of rt4_reproject_device for whole frames (h, w): G-buffers of rt4.GBUFFER_DTYPE, acc_prev
    (h, w, 4) in a frame dtype, hist_prev (h, w) int32. details=True adds a dict: eligible, kept, all4 (every one of the
    four taps counted), fx, fy."""
    h, w = g_cur.shape
    cos_min, plane_tol, slice_tol, max_refl_prob = F32(cos_min), F32(plane_tol), F32(slice_tol), F32(max_refl_prob)
    one, half = F32(1), F32(0.5)
    with np.errstate(all="ignore"):
        # 1. eligible
        z = g_cur["depth"]
        elig = (g_cur["surface"] >= 0) & (g_cur["refl_prob"] <= max_refl_prob) & (np.abs(z) < F32(np.inf))
        n_p = g_cur["normal"]
        # 2. the hit point
        X = fma32(_directions(u_cur, w, h), z[..., None], _vec(u_cur.focus))
        # 3. the old camera's coordinates
        fp, F, T, R = _vec(u_prev.focus), _vec(u_prev.vec_to_mtr), _vec(u_prev.top_drct), _vec(u_prev.right_drct)
        v = X - fp
        a = dot4(v, F) / dot4(F, F)
        ok = elig & (a > 0)
        t, r = dot4(v, T), dot4(v, R)
        e = fma32(R, -r[..., None], fma32(T, -t[..., None], fma32(F, -a[..., None], v)))
        vv = dot4(v, v)
        ok &= dot4(e, e) <= (slice_tol * slice_tol) * vv
        dv = np.sqrt(vv)
        # 4. the old screen position
        mtr, res = _vec(u_prev.mtr_sizes), _vec(u_prev.resolution)
        sx = (r / a) / mtr[0] + half
        sy = half - (t / a) / mtr[1]
        fx = sx * res[0] - half
        fy = sy * res[1] - half
        ok &= (fx > -one) & (fx < F32(w)) & (fy > -one) & (fy < F32(h))
        xf, yf = np.floor(fx), np.floor(fy)
        ax, ay = fx - xf, fy - yf
        x0 = np.where(ok, xf, 0).astype(np.int64)
        y0 = np.where(ok, yf, 0).astype(np.int64)
        tol = plane_tol * dv
        # 5. the taps
        d_prev, z_prev = _directions(u_prev, w, h), g_prev["depth"]
        C = decode(acc_prev)[..., :3]
        acc = np.zeros((h, w, 3), F32)
        wsum = np.zeros((h, w), F32)
        nmin = np.full((h, w), INT32_MAX, np.int32)
        ntaps = np.zeros((h, w), np.int32)
        for ty in (0, 1):
            for tx in (0, 1):
                qx, qy = x0 + tx, y0 + ty
                k = (ax if tx else one - ax) * (ay if ty else one - ay)
                counts = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h) & (k > 0)
                qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                hq = hist_prev[qy, qx]
                counts &= (hq > 0) & (g_prev["surface"][qy, qx] == g_cur["surface"])
                idx = np.nonzero(counts)  # the fma chains only where the cheap conditions hold
                qi = (qy[idx], qx[idx])
                good = dot4(n_p[idx], g_prev["normal"][qi]) >= cos_min
                Xq = fma32(d_prev[qi], z_prev[qi][:, None], fp)
                good &= np.abs(dot4(n_p[idx], Xq - X[idx])) <= tol[idx]
                counts[idx] = good
                acc = np.where(counts[..., None], acc + k[..., None] * C[qy, qx], acc)  # a multiply, then an add
                wsum = np.where(counts, wsum + k, wsum)
                nmin = np.where(counts, np.minimum(nmin, hq), nmin)
                ntaps += counts
        # 6. the result
        kept = wsum > 0
        c = fma32(acc / wsum[..., None], one, F32(0) * F32(0))  # blend_*(c, 1, 0)
        out = np.zeros((h, w, 4), acc_prev.dtype)
        out[..., :3] = np.where(kept[..., None], encode(np.where(kept[..., None], c, F32(0)), acc_prev.dtype), 0)
        out[..., 3] = 255 if acc_prev.dtype == np.uint8 else 1
        hist = np.where(kept, np.minimum(nmin, np.int32(max_history)), 0).astype(np.int32)
    if details:
        return out, hist, dict(eligible=elig, kept=kept, all4=ntaps == 4, fx=fx, fy=fy)
    return out, hist


def blend(new, acc, hist):
    """(acc, hist) after rt4_temporal_blend_device: new (h, w, 4) float32, acc (h, w, 4) in a frame dtype, hist int32."""
    n = np.where(hist == INT32_MAX, hist, hist + np.int32(1)).astype(np.int32)
    with np.errstate(all="ignore"):
        part = F32(1) / n.astype(F32)
        keep = F32(1) - part
        b = fma32(new[..., :3], part[..., None], decode(acc)[..., :3] * keep[..., None])
    out = np.empty_like(acc)
    out[..., :3] = encode(b, acc.dtype)
    out[..., 3] = 255 if acc.dtype == np.uint8 else 1
    return out, n
