"""numpy restatements for the G-buffer and denoiser tests — a plain helper, not a test module.

  primary_rays()      the trace kernel's primary-ray arithmetic (rt4_trace.hip refill: scr_coord, ray_drct, normalise)
  gbuffer_reference() those rays through the oracle's find_intersection, laid out as rt4.GBUFFER_DTYPE
  atrous()            the filter definition of include/rt4.h (rt4_denoise_device), level by level

Everything is fp32 with one rounding per operation. The multiply-adds of the ray generation and of dot() are
single-rounded: fma32 evaluates a*b + c as an exact Fraction and picks the nearest float32, ties to even (a float64
product rounded twice can differ in the last bit).
"""
from fractions import Fraction

import numpy as np

F32 = np.float32
H5 = [F32(1 / 16), F32(1 / 4), F32(3 / 8), F32(1 / 4), F32(1 / 16)]


def _fma_scalar(a, b, c):
    a, b, c = float(a), float(b), float(c)
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return F32(np.float64(a) * np.float64(b) + np.float64(c))  # inf / NaN: no rounding to get wrong
    fr = Fraction(a) * Fraction(b) + Fraction(c)
    if fr == 0:  # exact zero: -0 only when the product and the addend are both negative zeros
        neg_prod = np.signbit(a) != np.signbit(b)
        return F32(-0.0) if (neg_prod and a * b == 0.0 and np.signbit(c)) else F32(0.0)
    mid = F32(float(fr))  # a float32 within an ulp of the result
    best, best_err = None, None
    for v in (np.nextafter(mid, F32(-np.inf)), mid, np.nextafter(mid, F32(np.inf))):
        if not np.isfinite(v):
            continue
        e = abs(Fraction(float(v)) - fr)
        even = (int(np.array(v, F32).view(np.uint32)) & 1) == 0
        if best is None or e < best_err or (e == best_err and even):
            best, best_err = v, e
    return F32(best)


def fma32(a, b, c):
    """Element-wise float32 fma(a, b, c) with a single rounding."""
    a, b, c = np.broadcast_arrays(*(np.atleast_1d(np.asarray(v, F32)) for v in (a, b, c)))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)  # exact: 24 x 24 bits
        c64 = c.astype(np.float64)
        s = p + c64  # one rounding to 53 bits; TwoSum's error term says whether it was exact
        t = s - p
        err = (p - (s - t)) + (c64 - t)
        out = s.astype(F32)  # correct unless the inexact float64 sum sits on a float32 rounding boundary
    # Those elements go through exact Fractions: a float64 sum that was rounded and whose low 29 bits are a float32
    # tie (1 followed by zeros), and anything in float32's subnormal range, where the tie bit sits elsewhere.
    low = np.ascontiguousarray(s).view(np.uint64) & np.uint64(0x1FFFFFFF)
    with np.errstate(invalid="ignore"):
        slow = np.isfinite(s) & (err != 0) & ((low == np.uint64(0x10000000)) | (np.abs(s) < 2.0 ** -125))
    out = np.ascontiguousarray(out)
    for i in zip(*np.nonzero(slow)):
        out[i] = _fma_scalar(a[i], b[i], c[i])
    return out


def dot4(a, b):
    """dot() of rt4_device_math.h: fma(a.w, b.w, fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)))."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    r = a[..., 0] * b[..., 0]
    for k in (1, 2, 3):
        r = fma32(a[..., k], b[..., k], r)
    return r


def region_rows(reg):
    """Image row of every local row of a region (rt4.h rt4_region)."""
    i = np.arange(reg.h)
    return reg.y0 + ((i // reg.band_rows) * reg.band_step + i % reg.band_rows if reg.band_rows > 0 else i)


def primary_rays(u, reg):
    """(h, w, 8) float32: focus and normalised direction of every pixel's primary ray, op for op as the kernel."""
    res, mtr = np.array(u.resolution, F32), np.array(u.mtr_sizes, F32)
    right, top, vec = (np.array(list(v), F32) for v in (u.right_drct, u.top_drct, u.vec_to_mtr))
    sx = (np.arange(reg.x0, reg.x0 + reg.w).astype(F32) + F32(0.5)) / res[0]
    sy = (region_rows(reg).astype(F32) + F32(0.5)) / res[1]
    mx = (sx - F32(0.5)) * mtr[0]
    my = (F32(0.5) - sy) * mtr[1]
    # mad(right, mx, mad(top, my, vec)): the inner one depends on the row only
    inner = fma32(top[None, :], my[:, None], vec[None, :])  # (h, 4)
    dd = fma32(right[None, None, :], mx[None, :, None], inner[:, None, :])  # (h, w, 4)
    length = np.sqrt(dot4(dd, dd))  # IEEE sqrt of float32
    dd = dd / length[..., None]
    rays = np.empty((reg.h, reg.w, 8), F32)
    rays[..., :4] = np.array(list(u.focus), F32)
    rays[..., 4:] = dd
    return rays


def gbuffer_reference(rt4, oracle, desc, u, reg):
    """(G-buffer (h, w) of rt4.GBUFFER_DTYPE with surface = 0 on hits, hit mask, colours (h, w, 3)) from the numpy rays
    and the oracle's find_intersection. The oracle does not number surfaces: the caller derives them from colours."""
    rays = primary_rays(u, reg)
    out, col = oracle.find_intersection(desc, rays.reshape(-1, 8))
    out, col = out.reshape(reg.h, reg.w, 8), col.reshape(reg.h, reg.w, 3)
    hit = out[..., 0] > 0
    g = np.zeros((reg.h, reg.w), rt4.GBUFFER_DTYPE)
    g["normal"] = np.where(hit[..., None], out[..., 2:6], F32(0))
    g["depth"] = np.where(hit, out[..., 1], F32(np.inf))
    g["surface"] = np.where(hit, 0, -1)
    g["refl_prob"] = np.where(hit, out[..., 7], F32(0))
    g["glow"] = np.where(hit, out[..., 6], F32(0))
    return g, hit, col


def unique_colors(rt4, desc):
    """Overwrites the material colour of every surface of desc (in place) with a value no other surface has and returns
    {colour triple: surface index}. The kernel shape does not depend on colours."""
    n = rt4.lib.rt4_scene_surface_count(desc)
    mats = surface_materials(desc)
    assert len(mats) == n
    table = {}
    for k, m in enumerate(mats):
        c = (float(F32((k % 7 + 1) / 8.0)), float(F32((k // 7 % 7 + 1) / 8.0)), float(F32((k // 49 + 1) / 8.0)))
        m.color[0], m.color[1], m.color[2] = c
        table[c] = k
    return table


def surface_materials(desc):
    """The rt4.Material of every surface in surface order, straight from the SceneDesc fields."""
    out = [desc.spaces[i].material for i in range(desc.n_spaces)]
    out += [desc.spheres[i].material for i in range(desc.n_spheres)]
    out += [desc.cylinders[i].material for i in range(desc.n_cylinders)]
    for i in range(desc.n_unions):
        out += [desc.unions[i].cylinder1.material, desc.unions[i].cylinder2.material]
    for i in range(desc.n_hypercubes):
        out += [desc.hypercubes[i].cubes[k].material for k in range(8)]
    for i in range(desc.n_tigers):
        t = desc.tigers[i]
        out += [t.inner_cyl1.material, t.outer_cyl1.material, t.inner_cyl2.material, t.outer_cyl2.material]
    return out


def surfaces_from_colors(table, hit, col):
    """Surface index per pixel from the oracle's colours (unique_colors' table); -1 on a miss."""
    s = np.full(hit.shape, -1, np.int32)
    for (y, x) in zip(*np.nonzero(hit)):
        s[y, x] = table[tuple(float(v) for v in col[y, x])]
    return s


# ------------------------------------------------------------------------------------------------ filter
def decode(frame):
    """C_0: the stored frame as float32 (h, w, 4)."""
    if frame.dtype == np.uint8:
        return frame.astype(F32) / F32(255.0)
    return frame.astype(F32)


def encode(c, dtype):
    """float32 colours stored in a frame format: half rounds to nearest even, RGBA8 by the rule of rt4.h."""
    if dtype == np.uint8:
        v = np.fmin(np.fmax(c, F32(0)), F32(1)) * F32(255.0) + F32(0.5)
        return v.astype(np.uint8)
    return c.astype(dtype)


def filterable(gbuf, max_refl_prob):
    with np.errstate(invalid="ignore"):
        return (gbuf["surface"] >= 0) & (gbuf["refl_prob"] <= F32(max_refl_prob))


def atrous_level(c, gbuf, filt, step, cos_min, depth_tol):
    """One level: C_l -> C_{l+1} for the rgb channels of c (h, w, 3), float32."""
    h, w = filt.shape
    n, z, sid = gbuf["normal"], gbuf["depth"], gbuf["surface"]
    acc = np.zeros((h, w, 3), F32)
    wsum = np.zeros((h, w), F32)
    ys, xs = np.mgrid[0:h, 0:w]
    with np.errstate(invalid="ignore", over="ignore"):
        tol = F32(depth_tol) * z
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                k = H5[dy + 2] * H5[dx + 2]
                qy, qx = ys + step * dy, xs + step * dx
                inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
                qy, qx = np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)
                if dx == 0 and dy == 0:
                    counts = filt.copy()
                else:
                    counts = filt & inside & filt[qy, qx] & (sid[qy, qx] == sid)
                    # the fma chain only where the cheap conditions hold (it runs on exact Fractions)
                    idx = np.nonzero(counts)
                    d = dot4(n[idx], n[qy[idx], qx[idx]])
                    ok = (d >= F32(cos_min)) & (np.abs(z[qy[idx], qx[idx]] - z[idx]) <= tol[idx])
                    counts[idx] = ok
                term = k * c[qy, qx]  # one multiply ...
                acc = np.where(counts[..., None], acc + term, acc)  # ... then one add
                wsum = np.where(counts, wsum + k, wsum)
        out = c.copy()
        out[filt] = acc[filt] / wsum[filt][:, None]
    return out


def atrous(frame, gbuf, levels=3, cos_min=0.9, depth_tol=0.1, max_refl_prob=0.5):
    """The filtered frame in the input's format (rt4.h rt4_denoise_device): alpha and pixels that are not filterable
    keep the stored bits."""
    c0 = decode(frame)
    filt = filterable(gbuf, max_refl_prob)
    c = c0[..., :3].copy()
    for l in range(levels):
        c = atrous_level(c, gbuf, filt, 1 << l, cos_min, depth_tol)
    out = frame.copy()
    enc = encode(c, frame.dtype)
    out[..., :3] = np.where(filt[..., None], enc, frame[..., :3])
    return out
