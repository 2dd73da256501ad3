"""numpy restatement of the window-resolution upscale of include/rt4.h (rt4_upscale_device) — a plain helper, not a
test module.

  tap_positions()     step 2: the first tap and its weight for every window column (or row), in integers
  window_uniforms()   rt4_upscale_uniforms for the fields a primary ray needs
  upscale()           steps 1-5 of the definition, vectorised over the window
  bilinear()          the same weights with no guide: every tap inside the cell image counts

Everything is fp32 with one rounding per operation; the multiply-adds go through denoise_ref.fma32 (single-rounded).
"""
import types

import numpy as np

from denoise_ref import F32, decode, dot4, encode, fma32, primary_rays

NEAREST, GUIDED = 0, 1
DEFAULTS = dict(cos_min=0.9, plane_tol=0.02)


def tap_positions(n_cells, s):
    """(x0, ax) for the n_cells * s window columns: x0 int64 in [-1, n_cells - 1], ax float32 in [0, 1)."""
    x = np.arange(n_cells * s, dtype=np.int64)
    cx = x // s
    t = 2 * (x % s) + 1 - s
    x0 = np.where(t < 0, cx - 1, cx)
    nx = np.where(t < 0, t + 2 * s, t)
    return x0, nx.astype(F32) / F32(2 * s)  # one division


def window_uniforms(u_cells, s):
    """What primary_rays reads of rt4_upscale_uniforms(u_cells, s): the resolution times s, the rest as it is."""
    res = [F32(u_cells.resolution[0]) * F32(s), F32(u_cells.resolution[1]) * F32(s)]
    return types.SimpleNamespace(resolution=res, mtr_sizes=list(u_cells.mtr_sizes), focus=list(u_cells.focus),
                                 vec_to_mtr=list(u_cells.vec_to_mtr), top_drct=list(u_cells.top_drct),
                                 right_drct=list(u_cells.right_drct))


def _directions(u, w, h):
    return primary_rays(u, types.SimpleNamespace(x0=0, y0=0, w=w, h=h, band_rows=0, band_step=0))[..., 4:]


def nearest(cells, s):
    """Step 1: every cell's stored bits as an s x s block."""
    return np.repeat(np.repeat(cells, s, axis=0), s, axis=1)


def tap_plan(u_cells, s, g_cells, g_win, cos_min=0.9, plane_tol=0.02):
    """Steps 2-4 without the colours: which taps count. g_cells (ch, cw) and g_win (ch*s, cw*s) of rt4.GBUFFER_DTYPE.
    Returns dict(taps=[(qy, qx, k, counts)] in tap order, counted, candidates (taps per pixel that counted / that were
    inside the image with k > 0), dist=[|dot(n_p, X_q - X)| per tap, NaN where the tap never got that far])."""
    ch, cw = g_cells.shape
    H, W = ch * s, cw * s
    assert g_win.shape == (H, W)
    cos_min, plane_tol, one = F32(cos_min), F32(plane_tol), F32(1)
    focus = np.array(list(u_cells.focus), F32)
    with np.errstate(all="ignore"):
        x0, ax = tap_positions(cw, s)
        y0, ay = tap_positions(ch, s)
        x0, ax = np.broadcast_to(x0[None, :], (H, W)), np.broadcast_to(ax[None, :], (H, W))
        y0, ay = np.broadcast_to(y0[:, None], (H, W)), np.broadcast_to(ay[:, None], (H, W))
        # 3. the hit point
        z = g_win["depth"]
        sid = g_win["surface"]
        n_p = g_win["normal"]
        X = fma32(_directions(window_uniforms(u_cells, s), W, H), z[..., None], focus)
        tol = plane_tol * np.abs(z)
        Xc = fma32(_directions(u_cells, cw, ch), g_cells["depth"][..., None], focus)
        counted = np.zeros((H, W), np.int32)
        candidates = np.zeros((H, W), np.int32)
        taps, dists = [], []
        for ty in (0, 1):  # 4. the taps
            for tx in (0, 1):
                qx, qy = x0 + tx, y0 + ty
                k = (ax if tx else one - ax) * (ay if ty else one - ay)
                counts = (qx >= 0) & (qx < cw) & (qy >= 0) & (qy < ch) & (k > 0)
                candidates += counts
                qx, qy = np.clip(qx, 0, cw - 1), np.clip(qy, 0, ch - 1)
                counts &= g_cells["surface"][qy, qx] == sid
                idx = np.nonzero(counts & (sid >= 0))  # the fma chains only where the cheap conditions hold
                qi = (qy[idx], qx[idx])
                dist = np.abs(dot4(n_p[idx], Xc[qi] - X[idx]))
                counts[idx] = (dot4(n_p[idx], g_cells["normal"][qi]) >= cos_min) & (dist <= tol[idx])
                full = np.full((H, W), np.nan, F32)
                full[idx] = dist
                dists.append(full)
                taps.append((qy, qx, k, counts))
                counted += counts
    return dict(taps=taps, counted=counted, candidates=candidates, dist=dists, kept=counted > 0)


def apply_plan(plan, s, cells):
    """The rest of step 4 and step 5 for one cell frame (ch, cw, 4) in a frame dtype."""
    ch, cw = cells.shape[:2]
    H, W = ch * s, cw * s
    near = nearest(cells, s)
    with np.errstate(all="ignore"):
        C = decode(cells)[..., :3]
        acc = np.zeros((H, W, 3), F32)
        wsum = np.zeros((H, W), F32)
        for qy, qx, k, counts in plan["taps"]:
            acc = np.where(counts[..., None], acc + k[..., None] * C[qy, qx], acc)  # a multiply, then an add
            wsum = np.where(counts, wsum + k, wsum)
        kept = wsum > 0  # the weights are positive: the pixels with a counted tap
        c = fma32(acc / wsum[..., None], F32(1), F32(0) * F32(0))  # blend_*(c, 1, 0)
        out = near.copy()
        enc = encode(np.where(kept[..., None], c, F32(0)), cells.dtype)
        out[..., :3] = np.where(kept[..., None], enc, near[..., :3])
        out[..., 3] = np.where(kept, 255 if cells.dtype == np.uint8 else 1, near[..., 3])
    return out


def upscale(u_cells, s, cells, g_cells=None, g_win=None, mode=GUIDED, cos_min=0.9, plane_tol=0.02, details=False):
    """The window image (ch*s, cw*s, 4) of rt4_upscale_device: cells (ch, cw, 4) in a frame dtype, g_cells (ch, cw) and
    g_win (ch*s, cw*s) of rt4.GBUFFER_DTYPE. details=True adds tap_plan's dict (kept: the pixels with a counted tap)."""
    ch, cw = cells.shape[:2]
    if mode == NEAREST:
        near = nearest(cells, s)
        return (near, dict(kept=np.zeros((ch * s, cw * s), bool))) if details else near
    assert g_cells.shape == (ch, cw)
    plan = tap_plan(u_cells, s, g_cells, g_win, cos_min, plane_tol)
    out = apply_plan(plan, s, cells)
    return (out, plan) if details else out


def bilinear(u_cells, s, cells):
    """Plain bilinear interpolation with the definition's weights: all-miss G-buffers, so every tap inside the cell image
    counts (two misses match with no further test)."""
    dt = np.dtype([("normal", "<f4", (4,)), ("depth", "<f4"), ("surface", "<i4")])  # what tap_plan reads of a G-buffer
    ch, cw = cells.shape[:2]
    gc, gw = np.zeros((ch, cw), dt), np.zeros((ch * s, cw * s), dt)
    gc["surface"] = -1
    gw["surface"] = -1
    return upscale(u_cells, s, cells, gc, gw)
