// rt4_temporal.h — temporal reprojection of rt4.h (rt4_reproject_device, rt4_temporal_blend_device, rt4_temporal;
// DESIGN.md §4.34): kernels and entry points. From rt4_post.h: the argument checks, the launch bracket, the pixel
// grid, px_decode / px_store_opaque, HostStage and alloc_zeroed; from no other pass. rt4_upscale.h takes RpCam, rp_cam,
// rp_primary and rp_same_pose from here. No trace kernel uses anything from here.
//
// Reprojection is a gather: one lane per pixel of the new view in 32x8 blocks. The lane rebuilds its hit point from
// the new G-buffer, projects it into the old camera (both cameras are kernel arguments: SGPRs), and reads up to four
// taps of the old view. Per tap the 16-B word {depth, surface, refl_prob, glow} of the old G-buffer comes first, so a
// tap on another surface costs that one load; the history, the normal and the colour follow only as far as the tap
// still counts. No LDS. The blend is one lane per pixel: the sample, the accumulator and the history, each once.
#pragma once

namespace {

struct RpCam {  // what a primary ray and a projection need of rt4_uniforms
  float res[2], mtr[2], focus[4], vec[4], top[4], right[4];
};

struct RpArgs {
  RpCam cur, prev;
  const rt4_gbuffer_px* gcur;
  const rt4_gbuffer_px* gprev;
  const void* accp;
  const int32_t* histp;
  void* acco;
  int32_t* histo;
  int64_t gcur_stride, gprev_stride, accp_stride, histp_stride, acco_stride, histo_stride;
  int32_t w, h, format, max_history;
  float cos_min, plane_tol, slice_tol, max_refl_prob;
};

RpCam rp_cam(const rt4_uniforms* u) {
  RpCam c;
  std::memcpy(c.res, u->resolution, sizeof c.res);
  std::memcpy(c.mtr, u->mtr_sizes, sizeof c.mtr);
  std::memcpy(c.focus, u->focus, sizeof c.focus);
  std::memcpy(c.vec, u->vec_to_mtr, sizeof c.vec);
  std::memcpy(c.top, u->top_drct, sizeof c.top);
  std::memcpy(c.right, u->right_drct, sizeof c.right);
  return c;
}

// The primary direction of pixel (x, y), op for op as rt4_gbuffer_kernel builds it.
__device__ __forceinline__ V4 rp_primary(const RpCam& c, int x, int y) {
  const float sx = (static_cast<float>(x) + 0.5f) / c.res[0];
  const float sy = (static_cast<float>(y) + 0.5f) / c.res[1];
  const float mx = (sx - 0.5f) * c.mtr[0];
  const float my = (0.5f - sy) * c.mtr[1];
  const V4 dd = mad(ld4(c.right), mx, mad(ld4(c.top), my, ld4(c.vec)));
  return divs(dd, length(dd));
}

// rt4.h rt4_reproject_device, steps 1-6.
__global__ __launch_bounds__(256) void rt4_reproject_kernel(const RpArgs a) {
  const int2 xy = px_xy();
  const int x = xy.x, y = xy.y;
  const int w = a.w, h = a.h;
  if (x >= w || y >= h) return;
  const float4* gp = reinterpret_cast<const float4*>(a.gcur + static_cast<int64_t>(y) * a.gcur_stride + x);
  const float4 m = gp[1];  // depth, surface, refl_prob, glow
  const int surface = __float_as_int(m.y);
  float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f;
  int32_t nmin = INT32_MAX;
  if (surface >= 0 && m.z <= a.max_refl_prob && __builtin_fabsf(m.x) < __builtin_inff()) {  // 1. eligible
    const float4 n4 = gp[0];
    const V4 np{n4.x, n4.y, n4.z, n4.w};
    const V4 X = mad(rp_primary(a.cur, x, y), m.x, ld4(a.cur.focus));  // 2. the hit point
    const V4 fp = ld4(a.prev.focus), F = ld4(a.prev.vec), T = ld4(a.prev.top), R = ld4(a.prev.right);
    const V4 v = sub(X, fp);  // 3. in the old camera's coordinates
    const float aa = dot(v, F) / dot(F, F);
    if (aa > 0.0f) {
      const float t = dot(v, T), r = dot(v, R);
      const V4 e = mad(R, -r, mad(T, -t, mad(F, -aa, v)));
      const float vv = dot(v, v);
      if (dot(e, e) <= __fmul_rn(__fmul_rn(a.slice_tol, a.slice_tol), vv)) {  // still in the old camera's slice
        const float dv = sqrt_(vv);
        const float sx = (r / aa) / a.prev.mtr[0] + 0.5f;  // 4. the old screen position
        const float sy = 0.5f - (t / aa) / a.prev.mtr[1];
        const float fx = __fsub_rn(__fmul_rn(sx, a.prev.res[0]), 0.5f);
        const float fy = __fsub_rn(__fmul_rn(sy, a.prev.res[1]), 0.5f);
        if (fx > -1.0f && fx < static_cast<float>(w) && fy > -1.0f && fy < static_cast<float>(h)) {  // false for NaN
          const float xf = __builtin_floorf(fx), yf = __builtin_floorf(fy);
          const float ax = __fsub_rn(fx, xf), ay = __fsub_rn(fy, yf);
          const int x0 = static_cast<int>(xf), y0 = static_cast<int>(yf);  // in [-1, w-1] x [-1, h-1]
          const float tol = __fmul_rn(a.plane_tol, dv);
#pragma unroll
          for (int ty = 0; ty < 2; ty++) {  // 5. the taps
#pragma unroll
            for (int tx = 0; tx < 2; tx++) {
              const int qx = x0 + tx, qy = y0 + ty;
              const float k = __fmul_rn(tx ? ax : __fsub_rn(1.0f, ax), ty ? ay : __fsub_rn(1.0f, ay));
              if (qx < 0 || qx >= w || qy < 0 || qy >= h || !(k > 0.0f)) continue;
              const float4* gq = reinterpret_cast<const float4*>(a.gprev + static_cast<int64_t>(qy) * a.gprev_stride + qx);
              const float4 mq = gq[1];
              if (__float_as_int(mq.y) != surface) continue;
              const int32_t hq = a.histp[static_cast<int64_t>(qy) * a.histp_stride + qx];
              if (hq <= 0) continue;
              const float4 nq = gq[0];
              if (!(dot(np, V4{nq.x, nq.y, nq.z, nq.w}) >= a.cos_min)) continue;
              const V4 Xq = mad(rp_primary(a.prev, qx, qy), mq.x, fp);
              if (!(__builtin_fabsf(dot(np, sub(Xq, X))) <= tol)) continue;  // off the new hit's tangent plane
              const float4 c = px_decode(a.accp, a.format, static_cast<int64_t>(qy) * a.accp_stride + qx);
              ar = __fadd_rn(ar, __fmul_rn(k, c.x));
              ag = __fadd_rn(ag, __fmul_rn(k, c.y));
              ab = __fadd_rn(ab, __fmul_rn(k, c.z));
              wsum = __fadd_rn(wsum, k);
              nmin = hq < nmin ? hq : nmin;
            }
          }
        }
      }
    }
  }
  // 6. a restarted pixel stores the zero colour. px_store_opaque written out: calling it here changes this kernel's
  // generated code (one more instruction), and a refactoring may not.
  const bool kept = wsum > 0.0f;
  const V3 c = kept ? V3{ar / wsum, ag / wsum, ab / wsum} : V3{0.0f, 0.0f, 0.0f};
  const int64_t ao = static_cast<int64_t>(y) * a.acco_stride + x;
  if (a.format == RT4_FRAME_RGBA16F) {
    h4v zero;
    zero[0] = zero[1] = zero[2] = zero[3] = static_cast<_Float16>(0.0f);
    reinterpret_cast<h4v*>(a.acco)[ao] = blend_f16(c, 1.0f, zero);
  } else if (a.format == RT4_FRAME_RGBA8) {
    reinterpret_cast<uint32_t*>(a.acco)[ao] = blend_u8(c, 1.0f, 0u);
  } else {
    reinterpret_cast<float4*>(a.acco)[ao] = blend_f32(c, 1.0f, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  }
  a.histo[static_cast<int64_t>(y) * a.histo_stride + x] = kept ? (nmin < a.max_history ? nmin : a.max_history) : 0;
}

// rt4.h rt4_temporal_blend_device: write_pixel's blend with a part of the pixel's own.
__global__ __launch_bounds__(256) void rt4_temporal_blend_kernel(const float4* __restrict__ fresh, int64_t fresh_stride,
                                                                 void* __restrict__ acc, int64_t acc_stride, int32_t format,
                                                                 int32_t* __restrict__ hist, int64_t hist_stride, int32_t w,
                                                                 int32_t h) {
  const int2 xy = px_xy();
  const int x = xy.x, y = xy.y;
  if (x >= w || y >= h) return;
  int32_t* hp = hist + static_cast<int64_t>(y) * hist_stride + x;
  const int32_t n0 = *hp, n = n0 == INT32_MAX ? n0 : n0 + 1;
  const float part = 1.0f / static_cast<float>(n);
  const float4 f = fresh[static_cast<int64_t>(y) * fresh_stride + x];
  const V3 c{f.x, f.y, f.z};
  const int64_t at = static_cast<int64_t>(y) * acc_stride + x;
  if (format == RT4_FRAME_RGBA16F) {
    h4v* px = reinterpret_cast<h4v*>(acc) + at;
    *px = blend_f16(c, part, *px);
  } else if (format == RT4_FRAME_RGBA8) {
    uint32_t* px = reinterpret_cast<uint32_t*>(acc) + at;
    *px = blend_u8(c, part, *px);
  } else {
    float4* px = reinterpret_cast<float4*>(acc) + at;
    *px = blend_f32(c, part, *px);
  }
  *hp = n;
}

// The pose of a frame: the bytes of resolution, mtr_sizes, focus, vec_to_mtr, top_drct, right_drct.
bool rp_same_pose(const rt4_uniforms* a, const rt4_uniforms* b) {
  return std::memcmp(a->resolution, b->resolution, sizeof a->resolution) == 0 &&
         std::memcmp(a->mtr_sizes, b->mtr_sizes, sizeof a->mtr_sizes) == 0 &&
         std::memcmp(a->focus, b->focus, sizeof a->focus) == 0 &&
         std::memcmp(a->vec_to_mtr, b->vec_to_mtr, sizeof a->vec_to_mtr) == 0 &&
         std::memcmp(a->top_drct, b->top_drct, sizeof a->top_drct) == 0 &&
         std::memcmp(a->right_drct, b->right_drct, sizeof a->right_drct) == 0;
}

}  // namespace

struct rt4_temporal {
  rt4_context* ctx = nullptr;
  int32_t w = 0, h = 0, format = 0;
  void* d_acc[2] = {nullptr, nullptr};
  int32_t* d_hist[2] = {nullptr, nullptr};
  rt4_gbuffer_px* d_gbuf[2] = {nullptr, nullptr};
  float* d_sample = nullptr;
  int cur = 0;        // the pair that holds the image
  bool first = true;  // no frame since create / reset: the history restarts
  rt4_uniforms prev;  // the previous frame's uniforms (valid when !first)
};

extern "C" {

void rt4_reproject_params_default(rt4_reproject_params* p) {
  if (!p) return;
  p->cos_min = 0.9f;
  p->plane_tol = 0.02f;
  p->slice_tol = 0.01f;
  p->max_refl_prob = 0.5f;
  p->max_history = 255;
}

int rt4_reproject_device(rt4_context* ctx, const rt4_uniforms* u_cur, const rt4_gbuffer_px* d_gcur, int64_t gcur_stride,
                         const rt4_uniforms* u_prev, const rt4_gbuffer_px* d_gprev, int64_t gprev_stride,
                         const void* d_acc_prev, int64_t accp_stride, const int32_t* d_hist_prev, int64_t histp_stride,
                         void* d_acc_out, int64_t acco_stride, int32_t* d_hist_out, int64_t histo_stride, int32_t format,
                         int32_t w, int32_t h, const rt4_reproject_params* params, void* stream, char* err, size_t errlen) {
  if (!ctx || !u_cur || !d_gcur || !u_prev || !d_gprev || !d_acc_prev || !d_hist_prev || !d_acc_out || !d_hist_out || !params)
    return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const size_t px_bytes = static_cast<size_t>(rt4_frame_format_bytes(format));
  if (px_bytes == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || w > 65535 || h > 65535)
    return rt4_set_err(err, errlen, "frame size %d x %d not in [1, 65535]", w, h), RT4_ERR_ARG;
  const float fw = static_cast<float>(w), fh = static_cast<float>(h);
  if (u_cur->resolution[0] != fw || u_cur->resolution[1] != fh || u_prev->resolution[0] != fw || u_prev->resolution[1] != fh)
    return rt4_set_err(err, errlen, "the uniforms' resolution is not the frame size %d x %d", w, h), RT4_ERR_ARG;
  if (params->max_history < 1) return rt4_set_err(err, errlen, "max_history %d below 1", params->max_history), RT4_ERR_ARG;
  const PostImage in[4] = {post_image(d_gcur, gcur_stride, w, h, sizeof(rt4_gbuffer_px), "current G-buffer"),
                           post_image(d_gprev, gprev_stride, w, h, sizeof(rt4_gbuffer_px), "previous G-buffer"),
                           post_image(d_acc_prev, accp_stride, w, h, px_bytes, "previous accumulator"),
                           post_image(d_hist_prev, histp_stride, w, h, sizeof(int32_t), "previous history")};
  const PostImage out[2] = {post_image(d_acc_out, acco_stride, w, h, px_bytes, "output accumulator"),
                            post_image(d_hist_out, histo_stride, w, h, sizeof(int32_t), "output history")};
  const int st = post_check_args(out, 2, in, 4, err, errlen);
  if (st != RT4_OK) return st;
  RpArgs a;
  a.cur = rp_cam(u_cur);
  a.prev = rp_cam(u_prev);
  a.gcur = d_gcur;
  a.gprev = d_gprev;
  a.accp = d_acc_prev;
  a.histp = d_hist_prev;
  a.acco = d_acc_out;
  a.histo = d_hist_out;
  a.gcur_stride = gcur_stride;
  a.gprev_stride = gprev_stride;
  a.accp_stride = accp_stride;
  a.histp_stride = histp_stride;
  a.acco_stride = acco_stride;
  a.histo_stride = histo_stride;
  a.w = w;
  a.h = h;
  a.format = format;
  a.max_history = params->max_history;
  a.cos_min = params->cos_min;
  a.plane_tol = params->plane_tol;
  a.slice_tol = params->slice_tol;
  a.max_refl_prob = params->max_refl_prob;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return post_launch(ctx, s, "reproject kernel", err, errlen, [&] {
    hipLaunchKernelGGL(rt4_reproject_kernel, px_grid(w, h), dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

int rt4_reproject_host(rt4_context* ctx, const rt4_uniforms* u_cur, const rt4_gbuffer_px* gcur, int64_t gcur_stride,
                       const rt4_uniforms* u_prev, const rt4_gbuffer_px* gprev, int64_t gprev_stride, const void* acc_prev,
                       int64_t accp_stride, const int32_t* hist_prev, int64_t histp_stride, void* acc_out, int64_t acco_stride,
                       int32_t* hist_out, int64_t histo_stride, int32_t format, int32_t w, int32_t h,
                       const rt4_reproject_params* params, char* err, size_t errlen) {
  if (!ctx || !u_cur || !gcur || !u_prev || !gprev || !acc_prev || !hist_prev || !acc_out || !hist_out || !params)
    return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const int32_t px_bytes = rt4_frame_format_bytes(format);
  if (px_bytes == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || gcur_stride < w || gprev_stride < w || accp_stride < w || histp_stride < w || acco_stride < w ||
      histo_stride < w)
    return rt4_set_err(err, errlen, "bad frame size or row stride"), RT4_ERR_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  HostStage gc, gp, ap, hp, ao, ho;
  hipError_t e = gc.up(gcur, image_span(gcur_stride, w, h) * sizeof(rt4_gbuffer_px));
  if (e == hipSuccess) e = gp.up(gprev, image_span(gprev_stride, w, h) * sizeof(rt4_gbuffer_px));
  if (e == hipSuccess) e = ap.up(acc_prev, image_span(accp_stride, w, h) * static_cast<size_t>(px_bytes));
  if (e == hipSuccess) e = hp.up(hist_prev, image_span(histp_stride, w, h) * sizeof(int32_t));
  if (e == hipSuccess) e = ao.up(acc_out, image_span(acco_stride, w, h) * static_cast<size_t>(px_bytes));
  if (e == hipSuccess) e = ho.up(hist_out, image_span(histo_stride, w, h) * sizeof(int32_t));
  if (e == hipSuccess) {
    const int st = rt4_reproject_device(ctx, u_cur, gc.as<const rt4_gbuffer_px>(), gcur_stride, u_prev,
                                        gp.as<const rt4_gbuffer_px>(), gprev_stride, ap.d, accp_stride, hp.as<const int32_t>(),
                                        histp_stride, ao.d, acco_stride, ho.as<int32_t>(), histo_stride, format, w, h, params,
                                        nullptr, err, errlen);
    if (st != RT4_OK) return st;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = ao.down(acc_out);
    if (e == hipSuccess) e = ho.down(hist_out);
  }
  if (e != hipSuccess) return rt4_set_err(err, errlen, "reproject_host failed: %s", hipGetErrorString(e)), RT4_ERR_HIP;
  return RT4_OK;
}

int rt4_temporal_blend_device(rt4_context* ctx, const float* d_new_rgba32f, int64_t new_stride, void* d_acc, int64_t acc_stride,
                              int32_t format, int32_t* d_hist, int64_t hist_stride, int32_t w, int32_t h, void* stream,
                              char* err, size_t errlen) {
  if (!ctx || !d_new_rgba32f || !d_acc || !d_hist) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const size_t px_bytes = static_cast<size_t>(rt4_frame_format_bytes(format));
  if (px_bytes == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || w > 65535 || h > 65535)
    return rt4_set_err(err, errlen, "frame size %d x %d not in [1, 65535]", w, h), RT4_ERR_ARG;
  const PostImage in = post_image(d_new_rgba32f, new_stride, w, h, 16u, "sample frame");
  const PostImage out[2] = {post_image(d_acc, acc_stride, w, h, px_bytes, "accumulator"),  // both read and written
                            post_image(d_hist, hist_stride, w, h, sizeof(int32_t), "history")};
  const int st = post_check_args(out, 2, &in, 1, err, errlen);
  if (st != RT4_OK) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return post_launch(ctx, s, "temporal blend kernel", err, errlen, [&] {
    hipLaunchKernelGGL(rt4_temporal_blend_kernel, px_grid(w, h), dim3(256), 0, s, reinterpret_cast<const float4*>(d_new_rgba32f),
                       new_stride, d_acc, acc_stride, format, d_hist, hist_stride, w, h);
    return hipGetLastError();
  });
}

// ---- rt4_temporal -------------------------------------------------------------------------------------------------
uint64_t rt4_temporal_bytes(const rt4_temporal* t) {
  if (!t) return 0u;
  const uint64_t npx = static_cast<uint64_t>(t->w) * static_cast<uint64_t>(t->h);
  return npx * (2u * static_cast<uint64_t>(rt4_frame_format_bytes(t->format)) + 2u * sizeof(int32_t) +
                2u * sizeof(rt4_gbuffer_px) + 16u);
}

void rt4_temporal_destroy(rt4_temporal* t) {
  if (!t) return;
  (void)hipSetDevice(t->ctx->device);
  if (t->ctx->launched) (void)hipEventSynchronize(t->ctx->done);  // no launch still reads or writes the buffers
  for (int q = 0; q < 2; q++) {
    if (t->d_acc[q]) (void)hipFree(t->d_acc[q]);
    if (t->d_hist[q]) (void)hipFree(t->d_hist[q]);
    if (t->d_gbuf[q]) (void)hipFree(t->d_gbuf[q]);
  }
  if (t->d_sample) (void)hipFree(t->d_sample);
  delete t;
}

int rt4_temporal_create(rt4_context* ctx, int32_t w, int32_t h, int32_t format, rt4_temporal** out, char* err, size_t errlen) {
  if (!ctx || !out) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  *out = nullptr;
  const int32_t px_bytes = rt4_frame_format_bytes(format);
  if (px_bytes == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || w > 65535 || h > 16383)  // one rt4_region
    return rt4_set_err(err, errlen, "frame size %d x %d not in [1, 65535] x [1, 16383]", w, h), RT4_ERR_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  rt4_temporal* t = new rt4_temporal();
  t->ctx = ctx;
  t->w = w;
  t->h = h;
  t->format = format;
  const size_t npx = static_cast<size_t>(w) * static_cast<size_t>(h);
  hipError_t e = hipSuccess;
  for (int q = 0; q < 2 && e == hipSuccess; q++) {
    e = alloc_zeroed(&t->d_acc[q], npx * static_cast<size_t>(px_bytes));
    if (e == hipSuccess) e = alloc_zeroed(reinterpret_cast<void**>(&t->d_hist[q]), npx * sizeof(int32_t));
    if (e == hipSuccess) e = alloc_zeroed(reinterpret_cast<void**>(&t->d_gbuf[q]), npx * sizeof(rt4_gbuffer_px));
  }
  // finite: a render with part = 1 then stores the colour itself
  if (e == hipSuccess) e = alloc_zeroed(reinterpret_cast<void**>(&t->d_sample), npx * 16u);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    rt4_set_err(err, errlen, "temporal_create failed: %s", hipGetErrorString(e));
    rt4_temporal_destroy(t);
    return RT4_ERR_HIP;
  }
  *out = t;
  return RT4_OK;
}

void rt4_temporal_reset(rt4_temporal* t) {
  if (t) t->first = true;
}

int rt4_temporal_frame_device(rt4_temporal* t, const rt4_uniforms* u, const rt4_reproject_params* params,
                              unsigned long long* d_counter, void* stream, char* err, size_t errlen) {
  if (!t || !u) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (u->resolution[0] != static_cast<float>(t->w) || u->resolution[1] != static_cast<float>(t->h))
    return rt4_set_err(err, errlen, "the uniforms' resolution is not the frame size %d x %d", t->w, t->h), RT4_ERR_ARG;
  rt4_reproject_params dp;
  if (!params) {
    rt4_reproject_params_default(&dp);
    params = &dp;
  }
  if (params->max_history < 1) return rt4_set_err(err, errlen, "max_history %d below 1", params->max_history), RT4_ERR_ARG;
  rt4_context* ctx = t->ctx;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const rt4_region reg{0, 0, t->w, t->h, 0, 0};
  const int64_t stride = t->w;
  int st = RT4_OK;
  if (t->first) {  // (a) the history restarts: hist = 0 makes the blend below store the sample
    st = rt4_render_gbuffer_device(ctx, u, &reg, t->d_gbuf[t->cur], stride, stream, err, errlen);
    if (st != RT4_OK) return st;
    st = post_launch(ctx, s, "temporal_frame: history reset", err, errlen, [&] {  // a launch of the context's like any other
      return hipMemsetAsync(t->d_hist[t->cur], 0, static_cast<size_t>(t->w) * static_cast<size_t>(t->h) * sizeof(int32_t), s);
    });
    if (st != RT4_OK) return st;
  } else if (!rp_same_pose(u, &t->prev)) {  // (b) the camera moved: carry image and history over
    const int nxt = 1 - t->cur;
    st = rt4_render_gbuffer_device(ctx, u, &reg, t->d_gbuf[nxt], stride, stream, err, errlen);
    if (st != RT4_OK) return st;
    st = rt4_reproject_device(ctx, u, t->d_gbuf[nxt], stride, &t->prev, t->d_gbuf[t->cur], stride, t->d_acc[t->cur], stride,
                              t->d_hist[t->cur], stride, t->d_acc[nxt], stride, t->d_hist[nxt], stride, t->format, t->w, t->h,
                              params, stream, err, errlen);
    if (st != RT4_OK) return st;
    t->cur = nxt;
  }
  t->first = false;
  t->prev = *u;
  rt4_uniforms uc = *u;  // (c) one sample frame: part = 1 stores the tone-mapped colour itself
  uc.part = 1.0f;
  st = rt4_render_device_ex(ctx, &uc, &reg, t->d_sample, RT4_FRAME_RGBA32F, stride, d_counter, stream, err, errlen);
  if (st != RT4_OK) {
    t->first = true;  // the images no longer belong together: restart
    return st;
  }
  // (d)
  return rt4_temporal_blend_device(ctx, t->d_sample, stride, t->d_acc[t->cur], stride, t->format, t->d_hist[t->cur], stride,
                                   t->w, t->h, stream, err, errlen);
}

void* rt4_temporal_image(const rt4_temporal* t) { return t ? t->d_acc[t->cur] : nullptr; }
int32_t* rt4_temporal_history(const rt4_temporal* t) { return t ? t->d_hist[t->cur] : nullptr; }
const rt4_gbuffer_px* rt4_temporal_gbuffer(const rt4_temporal* t) { return t ? t->d_gbuf[t->cur] : nullptr; }

int rt4_temporal_read_host(rt4_temporal* t, void* image, int32_t* history, rt4_gbuffer_px* gbuf, char* err, size_t errlen) {
  if (!t) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  HIP_TRY(hipSetDevice(t->ctx->device));
  if (t->ctx->launched) HIP_TRY(hipEventSynchronize(t->ctx->done));
  const size_t npx = static_cast<size_t>(t->w) * static_cast<size_t>(t->h);
  if (image)
    HIP_TRY(hipMemcpy(image, t->d_acc[t->cur], npx * static_cast<size_t>(rt4_frame_format_bytes(t->format)), hipMemcpyDeviceToHost));
  if (history) HIP_TRY(hipMemcpy(history, t->d_hist[t->cur], npx * sizeof(int32_t), hipMemcpyDeviceToHost));
  if (gbuf) HIP_TRY(hipMemcpy(gbuf, t->d_gbuf[t->cur], npx * sizeof(rt4_gbuffer_px), hipMemcpyDeviceToHost));
  return RT4_OK;
}

}  // extern "C"
