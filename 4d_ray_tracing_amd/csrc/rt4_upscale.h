// rt4_upscale.h — window-resolution output of rt4.h (rt4_upscale_device, rt4_window): kernels and
// entry points. From rt4_post.h: the argument checks, the launch bracket, the pixel grid, px_decode / px_store_opaque,
// HostStage and alloc_zeroed; from rt4_temporal.h: RpCam, rp_cam, rp_primary and rp_same_pose. No trace kernel uses
// anything from here.
//
// The guided upscale is a gather: one lane per window pixel in 32x8 blocks. scale^2 window pixels share each cell, so
// a prologue computes the record of every cell the block can tap once: the cell's hit point X_q (a normalised primary
// direction: a sqrt and four divisions), its normal, its surface and its decoded colour, 12 dwords, kept in LDS as
// twelve dword arrays (a 32-lane half of a wave reads consecutive or equal dwords of one array, which ds_read_b32's
// 32-bank rule serves without conflicts). The block touches the cells [ox/s - 1, (ox+31)/s + 1] x [oy/s - 1,
// (oy+7)/s + 1]: at most 34 x 10 of them (scale 1). The taps then read LDS only; the fallback and NEAREST copy the
// stored bits of the pixel's own cell from global memory.
#pragma once

namespace {

constexpr int UP_CELLS_MAX = (PX_BX + 2) * (PX_BY + 2);  // cells a block can tap: scale 1

struct UpArgs {
  RpCam cells, win;
  const void* src;  // the cell frame
  const rt4_gbuffer_px* gcells;
  const rt4_gbuffer_px* gwin;
  void* out;
  int64_t src_stride, gcells_stride, gwin_stride, out_stride;
  int32_t cw, ch, s, format;
  float cos_min, plane_tol;
};

// The stored bits of cell (cx, cy) into window pixel (x, y): rt4.h step 1, and the fallback of step 5.
__device__ __forceinline__ void up_copy_cell(const void* src, int64_t si, void* out, int64_t oi, int32_t format) {
  if (format == RT4_FRAME_RGBA16F) reinterpret_cast<uint2*>(out)[oi] = reinterpret_cast<const uint2*>(src)[si];
  else if (format == RT4_FRAME_RGBA8) reinterpret_cast<uint32_t*>(out)[oi] = reinterpret_cast<const uint32_t*>(src)[si];
  else reinterpret_cast<float4*>(out)[oi] = reinterpret_cast<const float4*>(src)[si];
}

// rt4.h RT4_UPSCALE_NEAREST: the reference's sprite.
__global__ __launch_bounds__(256) void rt4_upscale_nearest_kernel(const void* __restrict__ src, int64_t src_stride,
                                                                  void* __restrict__ out, int64_t out_stride, int32_t format,
                                                                  int32_t W, int32_t H, int32_t s) {
  const int2 xy = px_xy();
  const int x = xy.x, y = xy.y;
  if (x >= W || y >= H) return;
  up_copy_cell(src, static_cast<int64_t>(y / s) * src_stride + x / s, out, static_cast<int64_t>(y) * out_stride + x, format);
}

// rt4.h RT4_UPSCALE_GUIDED, steps 2-5.
__global__ __launch_bounds__(256) void rt4_upscale_guided_kernel(const UpArgs a) {
  __shared__ float l_x0[UP_CELLS_MAX], l_x1[UP_CELLS_MAX], l_x2[UP_CELLS_MAX], l_x3[UP_CELLS_MAX];
  __shared__ float l_n0[UP_CELLS_MAX], l_n1[UP_CELLS_MAX], l_n2[UP_CELLS_MAX], l_n3[UP_CELLS_MAX];
  __shared__ float l_r[UP_CELLS_MAX], l_g[UP_CELLS_MAX], l_b[UP_CELLS_MAX];
  __shared__ int l_s[UP_CELLS_MAX];
  const int s = a.s, cw = a.cw, ch = a.ch;
  const int W = cw * s, H = ch * s;
  const int ox = static_cast<int>(blockIdx.x) * PX_BX, oy = static_cast<int>(blockIdx.y) * PX_BY;
  // the cells this block can tap (block-uniform): one before the first pixel's cell, one after the last pixel's
  const int bx = ox / s - 1, by = oy / s - 1;
  const int ncx = (ox + PX_BX - 1) / s - bx + 2, ncy = (oy + PX_BY - 1) / s - by + 2;  // <= 34, <= 10
  const V4 focus = ld4(a.cells.focus);
  for (int k = static_cast<int>(threadIdx.x); k < ncx * ncy; k += 256) {
    const int ly = k / ncx, lx = k - ly * ncx;
    const int qx = bx + lx, qy = by + ly;
    V4 Xq{0.0f, 0.0f, 0.0f, 0.0f}, nq = Xq;
    V3 c{0.0f, 0.0f, 0.0f};
    int sq = -1;  // outside the cell image: never read (the taps test the bounds themselves)
    if (qx >= 0 && qx < cw && qy >= 0 && qy < ch) {
      const float4* gq = reinterpret_cast<const float4*>(a.gcells + static_cast<int64_t>(qy) * a.gcells_stride + qx);
      const float4 n4 = gq[0], m = gq[1];  // m: depth, surface, refl_prob, glow
      nq = V4{n4.x, n4.y, n4.z, n4.w};
      sq = __float_as_int(m.y);
      Xq = mad(rp_primary(a.cells, qx, qy), m.x, focus);
      const float4 cq = px_decode(a.src, a.format, static_cast<int64_t>(qy) * a.src_stride + qx);
      c = V3{cq.x, cq.y, cq.z};
    }
    l_x0[k] = Xq.x; l_x1[k] = Xq.y; l_x2[k] = Xq.z; l_x3[k] = Xq.w;
    l_n0[k] = nq.x; l_n1[k] = nq.y; l_n2[k] = nq.z; l_n3[k] = nq.w;
    l_r[k] = c.x; l_g[k] = c.y; l_b[k] = c.z;
    l_s[k] = sq;
  }
  __syncthreads();
  const int x = ox + static_cast<int>(threadIdx.x & 31u), y = oy + static_cast<int>(threadIdx.x >> 5);
  if (x >= W || y >= H) return;
  const float4* gp = reinterpret_cast<const float4*>(a.gwin + static_cast<int64_t>(y) * a.gwin_stride + x);
  const float4 n4 = gp[0], m = gp[1];
  const int surface = __float_as_int(m.y);
  const V4 np{n4.x, n4.y, n4.z, n4.w};
  const int cx = x / s, cy = y / s;
  // 2. floor and frac of (x + 0.5)/s - 0.5 in integers: twice the offset from the cell's centre, in pixels
  const int tx2 = 2 * (x - cx * s) + 1 - s, ty2 = 2 * (y - cy * s) + 1 - s;
  const int x0 = tx2 < 0 ? cx - 1 : cx, y0 = ty2 < 0 ? cy - 1 : cy;
  const float den = static_cast<float>(2 * s);
  const float ax = static_cast<float>(tx2 < 0 ? tx2 + 2 * s : tx2) / den;
  const float ay = static_cast<float>(ty2 < 0 ? ty2 + 2 * s : ty2) / den;
  // 3. the hit point
  const V4 X = mad(rp_primary(a.win, x, y), m.x, focus);
  const float tol = __fmul_rn(a.plane_tol, __builtin_fabsf(m.x));
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f;
#pragma unroll
  for (int ty = 0; ty < 2; ty++) {  // 4. the taps
#pragma unroll
    for (int tx = 0; tx < 2; tx++) {
      const int qx = x0 + tx, qy = y0 + ty;
      const float k = __fmul_rn(tx ? ax : __fsub_rn(1.0f, ax), ty ? ay : __fsub_rn(1.0f, ay));
      if (qx < 0 || qx >= cw || qy < 0 || qy >= ch || !(k > 0.0f)) continue;
      const int lq = (qy - by) * ncx + (qx - bx);  // in [0, ncx * ncy): x0 >= ox/s - 1, x0 + 1 <= (ox+31)/s + 1
      if (l_s[lq] != surface) continue;
      if (surface >= 0) {
        if (!(dot(np, V4{l_n0[lq], l_n1[lq], l_n2[lq], l_n3[lq]}) >= a.cos_min)) continue;
        const V4 Xq{l_x0[lq], l_x1[lq], l_x2[lq], l_x3[lq]};
        if (!(__builtin_fabsf(dot(np, sub(Xq, X))) <= tol)) continue;  // off the pixel's tangent plane
      }
      ar = __fadd_rn(ar, __fmul_rn(k, l_r[lq]));
      ag = __fadd_rn(ag, __fmul_rn(k, l_g[lq]));
      ab = __fadd_rn(ab, __fmul_rn(k, l_b[lq]));
      wsum = __fadd_rn(wsum, k);
    }
  }
  // 5.
  const int64_t ao = static_cast<int64_t>(y) * a.out_stride + x;
  if (!(wsum > 0.0f)) {
    up_copy_cell(a.src, static_cast<int64_t>(cy) * a.src_stride + cx, a.out, ao, a.format);
    return;
  }
  px_store_opaque(a.out, a.format, ao, V3{ar / wsum, ag / wsum, ab / wsum});
}

bool up_scale_ok(int32_t scale) { return scale >= 1 && scale <= RT4_UPSCALE_MAX_SCALE; }

}  // namespace

struct rt4_window {
  rt4_context* ctx = nullptr;
  int32_t cw = 0, ch = 0, scale = 0, format = 0;
  void* d_image = nullptr;
  rt4_gbuffer_px* d_gwin = nullptr;
  rt4_gbuffer_px* d_gcells = nullptr;
  bool have_gwin = false;    // d_gwin holds the G-buffer of `prev` at window resolution
  bool have_gcells = false;  // d_gcells holds the G-buffer of `prev`
  rt4_uniforms prev;         // the pose the G-buffers were rendered for (valid when have_gwin)
};

extern "C" {

void rt4_upscale_params_default(rt4_upscale_params* p) {
  if (!p) return;
  p->mode = RT4_UPSCALE_GUIDED;
  p->cos_min = 0.9f;
  p->plane_tol = 0.02f;
}

int rt4_upscale_uniforms(const rt4_uniforms* u_cells, int32_t scale, rt4_uniforms* u_window) {
  if (!u_cells || !u_window || !up_scale_ok(scale)) return RT4_ERR_ARG;
  const float fs = static_cast<float>(scale);
  const float w = u_cells->resolution[0] * fs, h = u_cells->resolution[1] * fs;
  if (!(w <= 65535.0f) || !(h <= 16383.0f)) return RT4_ERR_ARG;  // one rt4_region; false for NaN
  *u_window = *u_cells;
  u_window->resolution[0] = w;
  u_window->resolution[1] = h;
  return RT4_OK;
}

int rt4_upscale_device(rt4_context* ctx, const rt4_uniforms* u_cells, int32_t scale, const void* d_cells,
                       int64_t cells_stride, const rt4_gbuffer_px* d_gcells, int64_t gcells_stride,
                       const rt4_gbuffer_px* d_gwin, int64_t gwin_stride, void* d_out, int64_t out_stride, int32_t format,
                       int32_t cells_w, int32_t cells_h, const rt4_upscale_params* params, void* stream, char* err,
                       size_t errlen) {
  if (!ctx || !u_cells || !d_cells || !d_out || !params) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (params->mode != RT4_UPSCALE_NEAREST && params->mode != RT4_UPSCALE_GUIDED)
    return rt4_set_err(err, errlen, "unknown upscale mode %d", params->mode), RT4_ERR_ARG;
  const bool guided = params->mode == RT4_UPSCALE_GUIDED;
  if (guided && (!d_gcells || !d_gwin)) return rt4_set_err(err, errlen, "NULL G-buffer"), RT4_ERR_ARG;
  const int32_t px_bytes = rt4_frame_format_bytes(format);
  if (px_bytes == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  if (!up_scale_ok(scale)) return rt4_set_err(err, errlen, "scale %d not in [1, %d]", scale, RT4_UPSCALE_MAX_SCALE), RT4_ERR_ARG;
  if (cells_w <= 0 || cells_h <= 0 || cells_w > 65535 / scale || cells_h > 65535 / scale)
    return rt4_set_err(err, errlen, "cells %d x %d at scale %d: the window is not in [1, 65535]", cells_w, cells_h, scale), RT4_ERR_ARG;
  if (u_cells->resolution[0] != static_cast<float>(cells_w) || u_cells->resolution[1] != static_cast<float>(cells_h))
    return rt4_set_err(err, errlen, "the uniforms' resolution is not the cell image's size %d x %d", cells_w, cells_h), RT4_ERR_ARG;
  const int32_t W = cells_w * scale, H = cells_h * scale;
  // nearest mode neither reads nor checks the G-buffers: they are not in the list
  const PostImage out = post_image(d_out, out_stride, W, H, static_cast<size_t>(px_bytes), "output");
  const PostImage in[3] = {post_image(d_cells, cells_stride, cells_w, cells_h, static_cast<size_t>(px_bytes), "cell frame"),
                           post_image(d_gcells, gcells_stride, cells_w, cells_h, sizeof(rt4_gbuffer_px), "cell G-buffer"),
                           post_image(d_gwin, gwin_stride, W, H, sizeof(rt4_gbuffer_px), "window G-buffer")};
  const int st = post_check_args(&out, 1, in, guided ? 3 : 1, err, errlen);
  if (st != RT4_OK) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return post_launch(ctx, s, "upscale kernel", err, errlen, [&] {
    const dim3 grid = px_grid(W, H), block(256);
    if (guided) {
      UpArgs a;
      a.cells = rp_cam(u_cells);
      a.win = a.cells;
      a.win.res[0] = static_cast<float>(W);  // rt4_upscale_uniforms: the products are exact
      a.win.res[1] = static_cast<float>(H);
      a.src = d_cells;
      a.gcells = d_gcells;
      a.gwin = d_gwin;
      a.out = d_out;
      a.src_stride = cells_stride;
      a.gcells_stride = gcells_stride;
      a.gwin_stride = gwin_stride;
      a.out_stride = out_stride;
      a.cw = cells_w;
      a.ch = cells_h;
      a.s = scale;
      a.format = format;
      a.cos_min = params->cos_min;
      a.plane_tol = params->plane_tol;
      hipLaunchKernelGGL(rt4_upscale_guided_kernel, grid, block, 0, s, a);
    } else {
      hipLaunchKernelGGL(rt4_upscale_nearest_kernel, grid, block, 0, s, d_cells, cells_stride, d_out, out_stride, format, W, H, scale);
    }
    return hipGetLastError();
  });
}

int rt4_upscale_host(rt4_context* ctx, const rt4_uniforms* u_cells, int32_t scale, const void* cells, int64_t cells_stride,
                     const rt4_gbuffer_px* gcells, int64_t gcells_stride, const rt4_gbuffer_px* gwin, int64_t gwin_stride,
                     void* out, int64_t out_stride, int32_t format, int32_t cells_w, int32_t cells_h,
                     const rt4_upscale_params* params, char* err, size_t errlen) {
  if (!ctx || !u_cells || !cells || !out || !params) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (params->mode != RT4_UPSCALE_NEAREST && params->mode != RT4_UPSCALE_GUIDED)
    return rt4_set_err(err, errlen, "unknown upscale mode %d", params->mode), RT4_ERR_ARG;
  const bool guided = params->mode == RT4_UPSCALE_GUIDED;
  if (guided && (!gcells || !gwin)) return rt4_set_err(err, errlen, "NULL G-buffer"), RT4_ERR_ARG;
  const int32_t px_bytes = rt4_frame_format_bytes(format);
  if (px_bytes == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  if (!up_scale_ok(scale)) return rt4_set_err(err, errlen, "scale %d not in [1, %d]", scale, RT4_UPSCALE_MAX_SCALE), RT4_ERR_ARG;
  if (cells_w <= 0 || cells_h <= 0 || cells_w > 65535 / scale || cells_h > 65535 / scale)
    return rt4_set_err(err, errlen, "cells %d x %d at scale %d: the window is not in [1, 65535]", cells_w, cells_h, scale), RT4_ERR_ARG;
  const int32_t W = cells_w * scale, H = cells_h * scale;
  if (cells_stride < cells_w || out_stride < W || (guided && (gcells_stride < cells_w || gwin_stride < W)))
    return rt4_set_err(err, errlen, "row stride smaller than width"), RT4_ERR_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  HostStage dc, dgc, dgw, dout;  // nearest mode stages no G-buffer
  hipError_t e = dc.up(cells, image_span(cells_stride, cells_w, cells_h) * static_cast<size_t>(px_bytes));
  if (e == hipSuccess && guided) e = dgc.up(gcells, image_span(gcells_stride, cells_w, cells_h) * sizeof(rt4_gbuffer_px));
  if (e == hipSuccess && guided) e = dgw.up(gwin, image_span(gwin_stride, W, H) * sizeof(rt4_gbuffer_px));
  if (e == hipSuccess) e = dout.up(out, image_span(out_stride, W, H) * static_cast<size_t>(px_bytes));
  if (e == hipSuccess) {
    const int st = rt4_upscale_device(ctx, u_cells, scale, dc.d, cells_stride, dgc.as<const rt4_gbuffer_px>(), gcells_stride,
                                      dgw.as<const rt4_gbuffer_px>(), gwin_stride, dout.d, out_stride, format, cells_w, cells_h,
                                      params, nullptr, err, errlen);
    if (st != RT4_OK) return st;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = dout.down(out);
  }
  if (e != hipSuccess) return rt4_set_err(err, errlen, "upscale_host failed: %s", hipGetErrorString(e)), RT4_ERR_HIP;
  return RT4_OK;
}

// ---- rt4_window ---------------------------------------------------------------------------------------------------
uint64_t rt4_window_bytes(const rt4_window* win) {
  if (!win) return 0u;
  const uint64_t ncells = static_cast<uint64_t>(win->cw) * static_cast<uint64_t>(win->ch);
  const uint64_t npx = ncells * static_cast<uint64_t>(win->scale) * static_cast<uint64_t>(win->scale);
  return npx * (static_cast<uint64_t>(rt4_frame_format_bytes(win->format)) + sizeof(rt4_gbuffer_px)) + ncells * sizeof(rt4_gbuffer_px);
}

void rt4_window_destroy(rt4_window* win) {
  if (!win) return;
  (void)hipSetDevice(win->ctx->device);
  if (win->ctx->launched) (void)hipEventSynchronize(win->ctx->done);  // no launch still reads or writes the buffers
  if (win->d_image) (void)hipFree(win->d_image);
  if (win->d_gwin) (void)hipFree(win->d_gwin);
  if (win->d_gcells) (void)hipFree(win->d_gcells);
  delete win;
}

int rt4_window_create(rt4_context* ctx, int32_t cells_w, int32_t cells_h, int32_t scale, int32_t format, rt4_window** out,
                      char* err, size_t errlen) {
  if (!ctx || !out) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  *out = nullptr;
  const int32_t px_bytes = rt4_frame_format_bytes(format);
  if (px_bytes == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  if (!up_scale_ok(scale)) return rt4_set_err(err, errlen, "scale %d not in [1, %d]", scale, RT4_UPSCALE_MAX_SCALE), RT4_ERR_ARG;
  if (cells_w <= 0 || cells_h <= 0 || cells_w > 65535 / scale || cells_h > 16383 / scale)  // the window: one rt4_region
    return rt4_set_err(err, errlen, "cells %d x %d at scale %d: the window is not in [1, 65535] x [1, 16383]", cells_w, cells_h, scale),
           RT4_ERR_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  rt4_window* win = new rt4_window();
  win->ctx = ctx;
  win->cw = cells_w;
  win->ch = cells_h;
  win->scale = scale;
  win->format = format;
  const size_t ncells = static_cast<size_t>(cells_w) * static_cast<size_t>(cells_h);
  const size_t npx = ncells * static_cast<size_t>(scale) * static_cast<size_t>(scale);
  hipError_t e = alloc_zeroed(&win->d_image, npx * static_cast<size_t>(px_bytes));
  if (e == hipSuccess) e = alloc_zeroed(reinterpret_cast<void**>(&win->d_gwin), npx * sizeof(rt4_gbuffer_px));
  if (e == hipSuccess) e = alloc_zeroed(reinterpret_cast<void**>(&win->d_gcells), ncells * sizeof(rt4_gbuffer_px));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    rt4_set_err(err, errlen, "window_create failed: %s", hipGetErrorString(e));
    rt4_window_destroy(win);
    return RT4_ERR_HIP;
  }
  *out = win;
  return RT4_OK;
}

void rt4_window_reset(rt4_window* win) {
  if (win) win->have_gwin = win->have_gcells = false;
}

int rt4_window_present_device(rt4_window* win, const rt4_uniforms* u_cells, const void* d_cells, int64_t cells_stride,
                              const rt4_gbuffer_px* d_gcells, int64_t gcells_stride, const rt4_upscale_params* params,
                              void* stream, char* err, size_t errlen) {
  if (!win || !u_cells || !d_cells) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (u_cells->resolution[0] != static_cast<float>(win->cw) || u_cells->resolution[1] != static_cast<float>(win->ch))
    return rt4_set_err(err, errlen, "the uniforms' resolution is not the cell image's size %d x %d", win->cw, win->ch), RT4_ERR_ARG;
  rt4_upscale_params dp;
  if (!params) {
    rt4_upscale_params_default(&dp);
    params = &dp;
  }
  rt4_context* ctx = win->ctx;
  const int32_t W = win->cw * win->scale, H = win->ch * win->scale;
  if (params->mode == RT4_UPSCALE_GUIDED) {
    if (win->have_gwin && !rp_same_pose(u_cells, &win->prev)) win->have_gwin = win->have_gcells = false;  // the camera moved
    if (!win->have_gwin) {
      rt4_uniforms uw;
      int st = rt4_upscale_uniforms(u_cells, win->scale, &uw);
      if (st != RT4_OK) return rt4_set_err(err, errlen, "the window of these uniforms is out of range"), st;
      const rt4_region reg{0, 0, W, H, 0, 0};
      st = rt4_render_gbuffer_device(ctx, &uw, &reg, win->d_gwin, W, stream, err, errlen);
      if (st != RT4_OK) return st;
      win->have_gwin = true;
      win->have_gcells = false;
      win->prev = *u_cells;
    }
    if (!d_gcells) {
      if (!win->have_gcells) {
        const rt4_region reg{0, 0, win->cw, win->ch, 0, 0};
        const int st = rt4_render_gbuffer_device(ctx, u_cells, &reg, win->d_gcells, win->cw, stream, err, errlen);
        if (st != RT4_OK) return st;
        win->have_gcells = true;
      }
      d_gcells = win->d_gcells;
      gcells_stride = win->cw;
    }
  }
  return rt4_upscale_device(ctx, u_cells, win->scale, d_cells, cells_stride, d_gcells, gcells_stride, win->d_gwin, W, win->d_image,
                            W, win->format, win->cw, win->ch, params, stream, err, errlen);
}

void* rt4_window_image(const rt4_window* win) { return win ? win->d_image : nullptr; }
const rt4_gbuffer_px* rt4_window_gbuffer(const rt4_window* win) { return win ? win->d_gwin : nullptr; }

int rt4_window_read_host(rt4_window* win, void* image, rt4_gbuffer_px* gbuf, char* err, size_t errlen) {
  if (!win) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  HIP_TRY(hipSetDevice(win->ctx->device));
  if (win->ctx->launched) HIP_TRY(hipEventSynchronize(win->ctx->done));
  const size_t npx = static_cast<size_t>(win->cw) * static_cast<size_t>(win->ch) * static_cast<size_t>(win->scale) *
                     static_cast<size_t>(win->scale);
  if (image) HIP_TRY(hipMemcpy(image, win->d_image, npx * static_cast<size_t>(rt4_frame_format_bytes(win->format)), hipMemcpyDeviceToHost));
  if (gbuf) HIP_TRY(hipMemcpy(gbuf, win->d_gwin, npx * sizeof(rt4_gbuffer_px), hipMemcpyDeviceToHost));
  return RT4_OK;
}

}  // extern "C"
