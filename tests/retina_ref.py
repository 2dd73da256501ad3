"""numpy restatement of the 3D retina view of include/rt4.h (§1-§3 of its definition) — a plain helper, not a test
module.

  slice_uniforms()  §1: the uniforms of one slice (matrix centre shifted along w_drct, seed decorrelated)
  voxelize()        §2: light volume + G-buffer volume -> premultiplied float4 voxels, with the plan (edge / fill / sky)
  project()         §3: voxels + view -> the picture in a frame dtype, with the plan (samples inside / partly outside /
                    outside, rays that stopped early, rays that never entered); project_colours() + store() are its halves

Everything is fp32 with one rounding per operation; every fma goes through denoise_ref.fma32 (single-rounded). Volumes
are indexed (slice, row, column).
"""
import ctypes

import numpy as np

from denoise_ref import F32, encode, fma32

DEFAULTS = dict(alpha_sky=0.0, alpha_fill=1.0 / 32.0, alpha_edge=0.5, t_min=1.0 / 256.0, background=(0.0, 0.0, 0.0))


# --------------------------------------------------------------------------------------------------------- §1 slices
def slice_t(depth, depth_size, s):
    return ((F32(s) + F32(0.5)) / F32(depth) - F32(0.5)) * F32(depth_size)


def slice_uniforms(u, w_drct, depth, depth_size, s):
    """A copy of the ctypes Uniforms u for slice s of depth."""
    out = type(u).from_buffer_copy(bytes(u))
    t = slice_t(depth, depth_size, s)
    if t != 0:
        v = fma32(np.array(list(w_drct), F32), t, np.array(list(u.vec_to_mtr), F32))
        for c in range(4):
            out.vec_to_mtr[c] = float(v[c])
    seed = ((u.seed & 0xFFFFFFFF) + ((s - depth // 2) & 0xFFFFFFFF) * 0x85EBCA6B) & 0xFFFFFFFF
    out.seed = ctypes.c_int32(seed).value
    return out


# ------------------------------------------------------------------------------------------------------- §2 voxelize
def edges(surface):
    """edge(v): surface(v) >= 0 and a face neighbour inside the volume has another surface value."""
    e = np.zeros(surface.shape, bool)
    for axis in range(3):
        n = surface.shape[axis]
        if n < 2:
            continue
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, n - 1), slice(1, n)
        lo, hi = tuple(lo), tuple(hi)
        differ = surface[lo] != surface[hi]
        e[lo] |= differ
        e[hi] |= differ
    return e & (surface >= 0)


def voxelize(light, gbuf, k, alpha_sky=DEFAULTS["alpha_sky"], alpha_fill=DEFAULTS["alpha_fill"],
             alpha_edge=DEFAULTS["alpha_edge"]):
    """(V (d, h, w, 4) float32, plan) from light (d, h, w) of rt4.LIGHT_DTYPE and gbuf (d, h, w) of rt4.GBUFFER_DTYPE."""
    surface = gbuf["surface"]
    with np.errstate(all="ignore"):
        tone = F32(1) - F32(1) / fma32(F32(k), light["mean"], F32(1))  # (d, h, w, 3)
    c = np.where((light["n"] == 0)[..., None], F32(0), tone).astype(F32)
    edge = edges(surface)
    hit = surface >= 0
    a = np.where(edge, F32(alpha_edge), np.where(hit, F32(alpha_fill), F32(alpha_sky))).astype(F32)
    V = np.empty(surface.shape + (4,), F32)
    with np.errstate(all="ignore"):
        V[..., :3] = a[..., None] * c  # plain multiplies
    V[..., 3] = a
    plan = dict(edge=int(edge.sum()), fill=int((hit & ~edge).sum()), sky=int((~hit).sum()),
                surfaces=int(np.unique(surface[hit]).size))
    return V, plan


# -------------------------------------------------------------------------------------------------------- §3 project
def store(c, dtype=np.float32):
    """Colours (oh, ow, 3) float32 as a frame of dtype: the store rule blend_*(c, 1, 0), alpha 1."""
    with np.errstate(all="ignore"):
        c = fma32(c, F32(1), F32(0) * F32(0))
    out = np.empty(c.shape[:2] + (4,), dtype)
    out[..., :3] = encode(c, np.dtype(dtype))
    out[..., 3] = 255 if np.dtype(dtype) == np.uint8 else 1
    return out


def project(V, view, ow, oh, t_min=DEFAULTS["t_min"], background=DEFAULTS["background"], dtype=np.float32):
    """(frame (oh, ow, 4) of dtype, plan) from the voxel volume V (d, h, w, 4) and a view with origin, du, dv, dt (three
    floats each) and steps."""
    c, plan = project_colours(V, view, ow, oh, t_min, background)
    return store(c, dtype), plan


def project_colours(V, view, ow, oh, t_min=DEFAULTS["t_min"], background=DEFAULTS["background"]):
    """(colours (oh, ow, 3) float32 before the store, plan): everything of §3 but the frame format."""
    d, h, w = V.shape[:3]
    N = [F32(w), F32(h), F32(d)]
    origin, du, dv, dt = ([F32(x) for x in list(v)] for v in (view.origin, view.du, view.dv, view.dt))
    with np.errstate(all="ignore"):
        a = (np.arange(ow).astype(F32) + F32(0.5)) / F32(ow) - F32(0.5)
        b = F32(0.5) - (np.arange(oh).astype(F32) + F32(0.5)) / F32(oh)
        base = [fma32(b[:, None], dv[c], fma32(a[None, :], du[c], origin[c])) for c in range(3)]  # (oh, ow) each
        C = np.zeros((oh, ow, 3), F32)
        T = np.ones((oh, ow), F32)
        alive = np.ones((oh, ow), bool)
        entered = np.zeros((oh, ow), bool)
        stopped = np.zeros((oh, ow), bool)
        plan = dict(inside=0, partly=0, outside=0)
        for n in range(int(view.steps)):
            tn = F32(n) + F32(0.5)
            f = [fma32(tn, dt[c], base[c]) for c in range(3)]
            inside = (f[0] > F32(-1)) & (f[0] < N[0]) & (f[1] > F32(-1)) & (f[1] < N[1]) & (f[2] > F32(-1)) & (f[2] < N[2])
            plan["outside"] += int((alive & ~inside).sum())
            act = alive & inside
            if not act.any():
                continue
            entered |= act
            idx = np.nonzero(act)
            f0 = [np.floor(f[c][idx]) for c in range(3)]
            w1 = [f[c][idx] - f0[c] for c in range(3)]
            w0 = [F32(1) - w1[c] for c in range(3)]
            i0 = [f0[c].astype(np.int64) for c in range(3)]
            S = np.zeros((idx[0].size, 4), F32)
            taps_in = np.zeros(idx[0].size, np.int32)
            for tz in (0, 1):
                for ty in (0, 1):
                    for tx in (0, 1):
                        xi, yi, zi = i0[0] + tx, i0[1] + ty, i0[2] + tz
                        ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h) & (zi >= 0) & (zi < d)
                        wgt = ((w1[2] if tz else w0[2]) * (w1[1] if ty else w0[1])) * (w1[0] if tx else w0[0])
                        v = V[np.clip(zi, 0, d - 1), np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)]
                        S = np.where(ok[:, None], fma32(wgt[:, None], v, S), S)
                        taps_in += ok
            plan["inside"] += int((taps_in == 8).sum())
            plan["partly"] += int((taps_in < 8).sum())
            Ti = T[idx]
            C[idx] = fma32(Ti[:, None], S[:, :3], C[idx])
            Ti = Ti * np.fmax(F32(1) - S[:, 3], F32(0))
            T[idx] = Ti
            stop = Ti < F32(t_min)
            stopped[idx] = stop
            alive[idx] = ~stop
        bg = np.array(list(background), F32)
        c = fma32(T[..., None], bg[None, None, :], C)
    plan.update(stopped=int(stopped.sum()), ran_out=int((entered & ~stopped).sum()), never_entered=int((~entered).sum()))
    return c, plan


def over(V, background=(0.0, 0.0, 0.0)):
    """The plain front-to-back "over" of the slices of V per column, slice 0 in front: (h, w, 3) float32. Written
    independently of project(): scalar loops, the operator as textbooks state it."""
    d, h, w = V.shape[:3]
    out = np.zeros((h, w, 3), F32)
    for i in range(h):
        for j in range(w):
            C = [F32(0)] * 3
            T = F32(1)
            for s in range(d):
                r, g, b, a = V[s, i, j]
                C = [fma32(T, x, c)[0] for x, c in zip((r, g, b), C)]
                T = T * max(F32(1) - a, F32(0))
            out[i, j] = [fma32(T, F32(bg), c)[0] for bg, c in zip(background, C)]
    return out
