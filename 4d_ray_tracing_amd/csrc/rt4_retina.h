// rt4_retina.h — the 3D retina view of rt4.h (rt4_retina_voxelize_device, rt4_retina_project_device, rt4_retina;
// DESIGN.md §4.47): kernels and entry points. From rt4_post.h: the launch bracket, the pixel grid, px_store_opaque,
// HostStage and alloc_zeroed; from rt4_light.h: light_tone. The host-only parts (rt4_retina_slice_uniforms,
// rt4_retina_params_default, rt4_retina_view_make) are rt4_host.cpp's. No trace kernel uses anything from here.
//
// The definition, op by op (rt4.h has the same text; fp32 round-to-nearest, no contraction, every fma explicit,
// division correctly rounded, comparisons with NaN false):
//   Voxelize, voxel v = (s, i, j):
//     c_ch = (L(v).n == 0) ? 0 : 1.0f - 1.0f / fmaf(k, L(v).mean_ch, 1.0f)
//     edge(v) iff G(v).surface >= 0 and a face neighbour of v inside the volume has another surface value
//     a = edge ? alpha_edge : (G(v).surface >= 0 ? alpha_fill : alpha_sky);  V(v) = (a*c_r, a*c_g, a*c_b, a)
//   Project, pixel (i, j):
//     a = ((float)j + 0.5f) / (float)ow - 0.5f;  b = 0.5f - ((float)i + 0.5f) / (float)oh
//     base_c = fmaf(b, dv_c, fmaf(a, du_c, origin_c));  f_c(n) = fmaf((float)n + 0.5f, dt_c, base_c)
//     sample n is inside iff f_c > -1.0f && f_c < (float)N_c for c = x, y, z
//     x0 = floorf(f_x), wx1 = f_x - x0, wx0 = 1.0f - wx1 (y, z alike); taps tz outer, ty, tx inner, weight
//     (wz * wy) * wx, skipped when an index is outside [0, N_c); S_c = fmaf(weight, V_c, S_c) from 0
//     C_c = fmaf(T, S_c, C_c); T = T * fmaxf(1.0f - S_a, 0.0f); stop if T < t_min     (from C = 0, T = 1, n ascending)
//     pixel = fmaf(T, background_c, C_c), alpha 1, through px_store_opaque
//
// Skipping. Only outside samples are skipped, so no rounding is involved. f_c(n) is the rounding of an exact value
// that is monotone in n ((float)n + 0.5f is exact for n <= 4096), and rounding is monotone, so on every axis f_c is
// either non-decreasing (dt_c >= 0), non-increasing (dt_c <= 0) or NaN for every n. Hence if sample m fails an axis on
// the side the ray comes from (dt_c >= 0 and !(f_c(m) > -1), or dt_c <= 0 and !(f_c(m) < N_c)), every sample before m
// fails it too; likewise behind the volume. The kernel guesses the first and last inside sample from a slab test in
// plain float arithmetic (any error allowed), checks the guess with these two exact tests on the real f_c, and walks
// the whole ray when a check does not hold. Inside the walk every sample is still tested as defined.
//
// Shape. One lane per picture pixel on the 32x8 grid. The rays are parallel, so the 64 samples a wave takes at one
// step lie on one plane patch of the volume: the two tx taps of a sample are 32 contiguous bytes, and neighbouring
// lanes' taps overlap or share cache lines. A 121 x 75 x 64 volume is 9.3 MB of float4: larger than one XCD's 4 MiB
// L2, well inside the Infinity Cache.
#pragma once

namespace {

struct RetProject {
  const float4* vox;
  int64_t vrs, vss;  // row and slice stride in voxels
  int32_t w, h, d;
  float origin[3], du[3], dv[3], dt[3];
  int32_t steps;
  float t_min, bg[3];
  void* out;
  int64_t out_stride;
  int32_t format, ow, oh;
};

// rt4.h step 2.
__global__ __launch_bounds__(256) void rt4_retina_voxelize_kernel(const rt4_light_px* __restrict__ light, int64_t lrs, int64_t lss,
                                                                  const rt4_gbuffer_px* __restrict__ gbuf, int64_t grs, int64_t gss,
                                                                  float k, float a_sky, float a_fill, float a_edge,
                                                                  float4* __restrict__ vox, int64_t vrs, int64_t vss, int32_t w,
                                                                  int32_t h, int32_t d) {
  const int2 xy = px_xy();
  const int x = xy.x, y = xy.y, z = static_cast<int>(blockIdx.z);
  if (x >= w || y >= h || z >= d) return;
  const rt4_gbuffer_px* g = gbuf + static_cast<int64_t>(z) * gss + static_cast<int64_t>(y) * grs + x;
  const int32_t sid = g->surface;
  bool edge = false;
  if (sid >= 0) {  // the neighbours inside the volume only
    if (x > 0) edge |= g[-1].surface != sid;
    if (x + 1 < w) edge |= g[1].surface != sid;
    if (y > 0) edge |= g[-grs].surface != sid;
    if (y + 1 < h) edge |= g[grs].surface != sid;
    if (z > 0) edge |= g[-gss].surface != sid;
    if (z + 1 < d) edge |= g[gss].surface != sid;
  }
  const float4* st = reinterpret_cast<const float4*>(light + static_cast<int64_t>(z) * lss + static_cast<int64_t>(y) * lrs + x);
  const float4 m = st[0];
  const int32_t n = __float_as_int(st[1].y);
  const V3 c = n == 0 ? V3{0.0f, 0.0f, 0.0f} : V3{light_tone(k, m.x), light_tone(k, m.y), light_tone(k, m.z)};
  const float a = edge ? a_edge : (sid >= 0 ? a_fill : a_sky);
  vox[static_cast<int64_t>(z) * vss + static_cast<int64_t>(y) * vrs + x] =
      make_float4(__fmul_rn(a, c.x), __fmul_rn(a, c.y), __fmul_rn(a, c.z), a);
}

// f_c(n) of the definition.
__device__ __forceinline__ float ret_at(int n, float dt, float base) {
  return __builtin_fmaf(__fadd_rn(static_cast<float>(n), 0.5f), dt, base);
}

// Sample m fails an axis on the side the ray comes from (before = true: every sample before m is outside too) or on the
// side it leaves to (before = false: every sample behind m is outside too). The argument is at the top of this file.
__device__ __forceinline__ bool ret_outside_from(bool before, int m, const float* dt, const float* base, const float* N) {
  bool out = false;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float f = ret_at(m, dt[c], base[c]);
    const bool below = !(f > -1.0f), above = !(f < N[c]);
    out |= before ? ((dt[c] >= 0.0f && below) || (dt[c] <= 0.0f && above)) : ((dt[c] >= 0.0f && above) || (dt[c] <= 0.0f && below));
  }
  return out;
}

// rt4.h step 3.
__global__ __launch_bounds__(256) void rt4_retina_project_kernel(const RetProject a) {
  const int2 xy = px_xy();
  const int j = xy.x, i = xy.y;
  if (j >= a.ow || i >= a.oh) return;
  const float pa = __fsub_rn(__fadd_rn(static_cast<float>(j), 0.5f) / static_cast<float>(a.ow), 0.5f);
  const float pb = __fsub_rn(0.5f, __fadd_rn(static_cast<float>(i), 0.5f) / static_cast<float>(a.oh));
  float base[3], dt[3];
  const float N[3] = {static_cast<float>(a.w), static_cast<float>(a.h), static_cast<float>(a.d)};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    base[c] = __builtin_fmaf(pb, a.dv[c], __builtin_fmaf(pa, a.du[c], a.origin[c]));
    dt[c] = a.dt[c];
  }
  // The guess: a slab test in sample numbers, in plain arithmetic. Nothing below depends on its accuracy.
  const float fsteps = static_cast<float>(a.steps);
  float t_in = 0.0f, t_out = fsteps;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (dt[c] != 0.0f) {
      const float inv = 1.0f / dt[c];
      const float t1 = (-1.0f - base[c]) * inv - 0.5f, t2 = (N[c] - base[c]) * inv - 0.5f;
      t_in = fmaxf(t_in, fminf(t1, t2));
      t_out = fminf(t_out, fmaxf(t1, t2));
    }
  }
  // clamped as floats to [0, steps] before the conversion (fmaxf / fminf drop a NaN)
  const int lo_guess = static_cast<int>(fminf(fmaxf(floorf(t_in) - 1.0f, 0.0f), fsteps));
  const int hi_guess = static_cast<int>(fminf(fmaxf(ceilf(t_out) + 2.0f, 0.0f), fsteps));
  // The checks: exact, on the definition's own f_c.
  const int lo = (lo_guess > 0 && ret_outside_from(true, lo_guess - 1, dt, base, N)) ? lo_guess : 0;
  const int hi = (hi_guess < a.steps && ret_outside_from(false, hi_guess, dt, base, N)) ? hi_guess : a.steps;
  float Cr = 0.0f, Cg = 0.0f, Cb = 0.0f, T = 1.0f;
  for (int n = lo; n < hi; n++) {
    const float fx = ret_at(n, dt[0], base[0]), fy = ret_at(n, dt[1], base[1]), fz = ret_at(n, dt[2], base[2]);
    if (!(fx > -1.0f && fx < N[0] && fy > -1.0f && fy < N[1] && fz > -1.0f && fz < N[2])) continue;
    const float x0f = floorf(fx), y0f = floorf(fy), z0f = floorf(fz);
    const float wx1 = __fsub_rn(fx, x0f), wy1 = __fsub_rn(fy, y0f), wz1 = __fsub_rn(fz, z0f);
    const float wx0 = __fsub_rn(1.0f, wx1), wy0 = __fsub_rn(1.0f, wy1), wz0 = __fsub_rn(1.0f, wz1);
    const int x0 = static_cast<int>(x0f), y0 = static_cast<int>(y0f), z0 = static_cast<int>(z0f);  // in [-1, N_c - 1]
    float Sr = 0.0f, Sg = 0.0f, Sb = 0.0f, Sa = 0.0f;
#pragma unroll
    for (int tz = 0; tz < 2; tz++) {
#pragma unroll
      for (int ty = 0; ty < 2; ty++) {
#pragma unroll
        for (int tx = 0; tx < 2; tx++) {
          const int xi = x0 + tx, yi = y0 + ty, zi = z0 + tz;
          if (xi < 0 || xi >= a.w || yi < 0 || yi >= a.h || zi < 0 || zi >= a.d) continue;  // every load index-checked
          const float wgt = __fmul_rn(__fmul_rn(tz ? wz1 : wz0, ty ? wy1 : wy0), tx ? wx1 : wx0);
          const float4 v = a.vox[static_cast<int64_t>(zi) * a.vss + static_cast<int64_t>(yi) * a.vrs + xi];
          Sr = __builtin_fmaf(wgt, v.x, Sr);
          Sg = __builtin_fmaf(wgt, v.y, Sg);
          Sb = __builtin_fmaf(wgt, v.z, Sb);
          Sa = __builtin_fmaf(wgt, v.w, Sa);
        }
      }
    }
    Cr = __builtin_fmaf(T, Sr, Cr);
    Cg = __builtin_fmaf(T, Sg, Cg);
    Cb = __builtin_fmaf(T, Sb, Cb);
    T = __fmul_rn(T, fmaxf(__fsub_rn(1.0f, Sa), 0.0f));
    if (T < a.t_min) break;
  }
  px_store_opaque(a.out, a.format, static_cast<int64_t>(i) * a.out_stride + j,
                  V3{__builtin_fmaf(T, a.bg[0], Cr), __builtin_fmaf(T, a.bg[1], Cg), __builtin_fmaf(T, a.bg[2], Cb)});
}

// ---- argument checks ---------------------------------------------------------------------------------------------------
struct RetVolume {  // one strided volume of a pass's argument list
  const void* p;
  int64_t row, slice;  // strides in elements
  size_t elem;
  const char* name;
};

size_t ret_span(const RetVolume& v, int32_t w, int32_t h, int32_t d) {  // elements up to the last voxel's end
  return static_cast<size_t>(d - 1) * static_cast<size_t>(v.slice) + image_span(v.row, w, h);
}

int ret_check_dims(int32_t w, int32_t h, int32_t d, char* err, size_t errlen) {
  if (w <= 0 || h <= 0 || w > 65535 || h > 65535)
    return rt4_set_err(err, errlen, "volume slice %d x %d not in [1, 65535]", w, h), RT4_ERR_ARG;
  if (d < 1 || d > RT4_RETINA_MAX_DEPTH) return rt4_set_err(err, errlen, "depth %d not in [1, %d]", d, RT4_RETINA_MAX_DEPTH), RT4_ERR_ARG;
  return RT4_OK;
}

int ret_check_strides(const RetVolume& v, int32_t w, int32_t h, char* err, size_t errlen) {
  if (v.row < w) return rt4_set_err(err, errlen, "%s: row stride smaller than width", v.name), RT4_ERR_ARG;
  if (v.slice < static_cast<int64_t>(h - 1) * v.row + w)
    return rt4_set_err(err, errlen, "%s: slice stride smaller than a slice", v.name), RT4_ERR_ARG;
  return RT4_OK;
}

int ret_check_aligned(const RetVolume& v, char* err, size_t errlen) {
  if (reinterpret_cast<uintptr_t>(v.p) % 16u != 0) return rt4_set_err(err, errlen, "%s not aligned to 16 bytes", v.name), RT4_ERR_ARG;
  return RT4_OK;
}

// The half-open byte ranges [p, p + bytes): ranges that only touch do not overlap.
bool ret_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

bool ret_unit(float v) { return v >= 0.0f && v <= 1.0f; }  // false for NaN

int ret_check_params(const rt4_retina_params* p, char* err, size_t errlen) {
  if (!ret_unit(p->alpha_sky) || !ret_unit(p->alpha_fill) || !ret_unit(p->alpha_edge))
    return rt4_set_err(err, errlen, "retina params: an alpha outside [0, 1]"), RT4_ERR_ARG;
  if (!(p->t_min >= 0.0f && p->t_min < 1.0f)) return rt4_set_err(err, errlen, "retina params: t_min outside [0, 1)"), RT4_ERR_ARG;
  return RT4_OK;
}

// What voxelize checks besides pointers and alignment, shared by the _device and _host variants.
int ret_check_voxelize(const RetVolume& L, const RetVolume& G, const RetVolume& V, const rt4_retina_params* params, int32_t w,
                       int32_t h, int32_t d, char* err, size_t errlen) {
  int st = ret_check_dims(w, h, d, err, errlen);
  if (st == RT4_OK) st = ret_check_strides(L, w, h, err, errlen);
  if (st == RT4_OK) st = ret_check_strides(G, w, h, err, errlen);
  if (st == RT4_OK) st = ret_check_strides(V, w, h, err, errlen);
  if (st == RT4_OK) st = ret_check_params(params, err, errlen);
  return st;
}

// The same for project.
int ret_check_project(const RetVolume& V, int32_t w, int32_t h, int32_t d, const rt4_retina_view* view,
                      const rt4_retina_params* params, int32_t format, int64_t frame_stride, int32_t ow, int32_t oh, char* err,
                      size_t errlen) {
  if (rt4_frame_format_bytes(format) == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  int st = ret_check_dims(w, h, d, err, errlen);
  if (st == RT4_OK) st = ret_check_strides(V, w, h, err, errlen);
  if (st != RT4_OK) return st;
  if (ow <= 0 || oh <= 0 || ow > 65535 || oh > 65535)
    return rt4_set_err(err, errlen, "picture size %d x %d not in [1, 65535]", ow, oh), RT4_ERR_ARG;
  if (frame_stride < ow) return rt4_set_err(err, errlen, "frame: row stride smaller than width"), RT4_ERR_ARG;
  if (view->steps < 1 || view->steps > RT4_RETINA_MAX_STEPS)
    return rt4_set_err(err, errlen, "view: steps %d not in [1, %d]", view->steps, RT4_RETINA_MAX_STEPS), RT4_ERR_ARG;
  return ret_check_params(params, err, errlen);
}

}  // namespace

struct rt4_retina {
  rt4_context* ctx = nullptr;
  int32_t w = 0, h = 0, depth = 0;
  rt4_light_px* d_light = nullptr;
  rt4_gbuffer_px* d_gbuf = nullptr;
  float* d_vox = nullptr;
  bool have = false;        // the G-buffer volume is `u`'s and the light volume holds frames_done frames of it
  int64_t frames_done = 0;
  rt4_uniforms u;           // what the volumes were accumulated for (valid when have)
  float w_drct[4];
  float depth_size = 0.0f;
  bool vox_valid = false;   // d_vox is the voxelization of the volumes as they are, with vox_alpha and vox_k
  float vox_alpha[3], vox_k = 0.0f;

  size_t voxels() const { return static_cast<size_t>(w) * static_cast<size_t>(h) * static_cast<size_t>(depth); }
};

extern "C" {

int rt4_retina_voxelize_device(rt4_context* ctx, const rt4_light_px* d_light, int64_t light_row_stride,
                               int64_t light_slice_stride, const rt4_gbuffer_px* d_gbuf, int64_t gbuf_row_stride,
                               int64_t gbuf_slice_stride, float k, const rt4_retina_params* params, float* d_voxels,
                               int64_t vox_row_stride, int64_t vox_slice_stride, int32_t w, int32_t h, int32_t d,
                               void* stream, char* err, size_t errlen) {
  if (!ctx || !d_light || !d_gbuf || !params || !d_voxels) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const RetVolume L{d_light, light_row_stride, light_slice_stride, sizeof(rt4_light_px), "light volume"};
  const RetVolume G{d_gbuf, gbuf_row_stride, gbuf_slice_stride, sizeof(rt4_gbuffer_px), "G-buffer volume"};
  const RetVolume V{d_voxels, vox_row_stride, vox_slice_stride, sizeof(float4), "voxel volume"};
  int st = ret_check_voxelize(L, G, V, params, w, h, d, err, errlen);
  if (st == RT4_OK) st = ret_check_aligned(L, err, errlen);
  if (st == RT4_OK) st = ret_check_aligned(G, err, errlen);
  if (st == RT4_OK) st = ret_check_aligned(V, err, errlen);
  if (st != RT4_OK) return st;
  const size_t v_bytes = ret_span(V, w, h, d) * V.elem;
  if (ret_overlap(V.p, v_bytes, L.p, ret_span(L, w, h, d) * L.elem))
    return rt4_set_err(err, errlen, "voxel volume overlaps light volume"), RT4_ERR_ARG;
  if (ret_overlap(V.p, v_bytes, G.p, ret_span(G, w, h, d) * G.elem))
    return rt4_set_err(err, errlen, "voxel volume overlaps G-buffer volume"), RT4_ERR_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return post_launch(ctx, s, "retina voxelize kernel", err, errlen, [&] {
    dim3 grid = px_grid(w, h);
    grid.z = static_cast<unsigned>(d);
    hipLaunchKernelGGL(rt4_retina_voxelize_kernel, grid, dim3(256), 0, s, d_light, light_row_stride, light_slice_stride, d_gbuf,
                       gbuf_row_stride, gbuf_slice_stride, k, params->alpha_sky, params->alpha_fill, params->alpha_edge,
                       reinterpret_cast<float4*>(d_voxels), vox_row_stride, vox_slice_stride, w, h, d);
    return hipGetLastError();
  });
}

int rt4_retina_voxelize_host(rt4_context* ctx, const rt4_light_px* light, int64_t light_row_stride,
                             int64_t light_slice_stride, const rt4_gbuffer_px* gbuf, int64_t gbuf_row_stride,
                             int64_t gbuf_slice_stride, float k, const rt4_retina_params* params, float* voxels,
                             int64_t vox_row_stride, int64_t vox_slice_stride, int32_t w, int32_t h, int32_t d, char* err,
                             size_t errlen) {
  if (!ctx || !light || !gbuf || !params || !voxels) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const RetVolume L{light, light_row_stride, light_slice_stride, sizeof(rt4_light_px), "light volume"};
  const RetVolume G{gbuf, gbuf_row_stride, gbuf_slice_stride, sizeof(rt4_gbuffer_px), "G-buffer volume"};
  const RetVolume V{voxels, vox_row_stride, vox_slice_stride, sizeof(float4), "voxel volume"};
  const int ck = ret_check_voxelize(L, G, V, params, w, h, d, err, errlen);
  if (ck != RT4_OK) return ck;
  HIP_TRY(hipSetDevice(ctx->device));
  HostStage dl, dg, dv;
  hipError_t e = dl.up(light, ret_span(L, w, h, d) * L.elem);
  if (e == hipSuccess) e = dg.up(gbuf, ret_span(G, w, h, d) * G.elem);
  if (e == hipSuccess) e = dv.up(voxels, ret_span(V, w, h, d) * V.elem);
  if (e == hipSuccess) {
    const int st = rt4_retina_voxelize_device(ctx, dl.as<const rt4_light_px>(), light_row_stride, light_slice_stride,
                                              dg.as<const rt4_gbuffer_px>(), gbuf_row_stride, gbuf_slice_stride, k, params,
                                              dv.as<float>(), vox_row_stride, vox_slice_stride, w, h, d, nullptr, err, errlen);
    if (st != RT4_OK) return st;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = dv.down(voxels);
  }
  if (e != hipSuccess) return rt4_set_err(err, errlen, "retina_voxelize_host failed: %s", hipGetErrorString(e)), RT4_ERR_HIP;
  return RT4_OK;
}

int rt4_retina_project_device(rt4_context* ctx, const float* d_voxels, int64_t vox_row_stride, int64_t vox_slice_stride,
                              int32_t w, int32_t h, int32_t d, const rt4_retina_view* view,
                              const rt4_retina_params* params, void* d_frame, int32_t format, int64_t frame_stride,
                              int32_t ow, int32_t oh, void* stream, char* err, size_t errlen) {
  if (!ctx || !d_voxels || !view || !params || !d_frame) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const RetVolume V{d_voxels, vox_row_stride, vox_slice_stride, sizeof(float4), "voxel volume"};
  int st = ret_check_project(V, w, h, d, view, params, format, frame_stride, ow, oh, err, errlen);
  if (st == RT4_OK) st = ret_check_aligned(V, err, errlen);
  if (st != RT4_OK) return st;
  const size_t px_bytes = static_cast<size_t>(rt4_frame_format_bytes(format));
  const PostImage out = post_image(d_frame, frame_stride, ow, oh, px_bytes, "frame");
  st = post_check_image(out, err, errlen);
  if (st != RT4_OK) return st;
  if (ret_overlap(d_frame, post_bytes(out), d_voxels, ret_span(V, w, h, d) * V.elem))
    return rt4_set_err(err, errlen, "frame overlaps voxel volume"), RT4_ERR_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return post_launch(ctx, s, "retina project kernel", err, errlen, [&] {
    RetProject a;
    a.vox = reinterpret_cast<const float4*>(d_voxels);
    a.vrs = vox_row_stride;
    a.vss = vox_slice_stride;
    a.w = w;
    a.h = h;
    a.d = d;
    for (int c = 0; c < 3; c++) {
      a.origin[c] = view->origin[c];
      a.du[c] = view->du[c];
      a.dv[c] = view->dv[c];
      a.dt[c] = view->dt[c];
      a.bg[c] = params->background[c];
    }
    a.steps = view->steps;
    a.t_min = params->t_min;
    a.out = d_frame;
    a.out_stride = frame_stride;
    a.format = format;
    a.ow = ow;
    a.oh = oh;
    hipLaunchKernelGGL(rt4_retina_project_kernel, px_grid(ow, oh), dim3(256), 0, s, a);
    return hipGetLastError();
  });
}

int rt4_retina_project_host(rt4_context* ctx, const float* voxels, int64_t vox_row_stride, int64_t vox_slice_stride,
                            int32_t w, int32_t h, int32_t d, const rt4_retina_view* view, const rt4_retina_params* params,
                            void* frame, int32_t format, int64_t frame_stride, int32_t ow, int32_t oh, char* err,
                            size_t errlen) {
  if (!ctx || !voxels || !view || !params || !frame) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const RetVolume V{voxels, vox_row_stride, vox_slice_stride, sizeof(float4), "voxel volume"};
  const int ck = ret_check_project(V, w, h, d, view, params, format, frame_stride, ow, oh, err, errlen);
  if (ck != RT4_OK) return ck;
  HIP_TRY(hipSetDevice(ctx->device));
  HostStage dv, dout;
  hipError_t e = dv.up(voxels, ret_span(V, w, h, d) * V.elem);
  if (e == hipSuccess) e = dout.up(frame, image_span(frame_stride, ow, oh) * static_cast<size_t>(rt4_frame_format_bytes(format)));
  if (e == hipSuccess) {
    const int st = rt4_retina_project_device(ctx, dv.as<const float>(), vox_row_stride, vox_slice_stride, w, h, d, view, params,
                                             dout.d, format, frame_stride, ow, oh, nullptr, err, errlen);
    if (st != RT4_OK) return st;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = dout.down(frame);
  }
  if (e != hipSuccess) return rt4_set_err(err, errlen, "retina_project_host failed: %s", hipGetErrorString(e)), RT4_ERR_HIP;
  return RT4_OK;
}

// ---- rt4_retina ------------------------------------------------------------------------------------------------------
uint64_t rt4_retina_bytes(const rt4_retina* ret) {
  if (!ret) return 0u;
  return static_cast<uint64_t>(ret->voxels()) * (sizeof(rt4_light_px) + sizeof(rt4_gbuffer_px) + sizeof(float4));
}

void rt4_retina_destroy(rt4_retina* ret) {
  if (!ret) return;
  (void)hipSetDevice(ret->ctx->device);
  if (ret->ctx->launched) (void)hipEventSynchronize(ret->ctx->done);  // no launch still reads or writes the volumes
  if (ret->d_light) (void)hipFree(ret->d_light);
  if (ret->d_gbuf) (void)hipFree(ret->d_gbuf);
  if (ret->d_vox) (void)hipFree(ret->d_vox);
  delete ret;
}

int rt4_retina_create(rt4_context* ctx, int32_t w, int32_t h, int32_t depth, rt4_retina** out, char* err, size_t errlen) {
  if (!ctx || !out) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  *out = nullptr;
  if (w <= 0 || h <= 0 || w > 8191 || h > 8191)  // rt4_render_light_device's limit
    return rt4_set_err(err, errlen, "retina slice %d x %d not in [1, 8191]", w, h), RT4_ERR_ARG;
  if (depth < 1 || depth > RT4_RETINA_MAX_DEPTH)
    return rt4_set_err(err, errlen, "depth %d not in [1, %d]", depth, RT4_RETINA_MAX_DEPTH), RT4_ERR_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  rt4_retina* ret = new rt4_retina();
  ret->ctx = ctx;
  ret->w = w;
  ret->h = h;
  ret->depth = depth;
  const size_t n = ret->voxels();
  hipError_t e = alloc_zeroed(reinterpret_cast<void**>(&ret->d_light), n * sizeof(rt4_light_px));
  if (e == hipSuccess) e = alloc_zeroed(reinterpret_cast<void**>(&ret->d_gbuf), n * sizeof(rt4_gbuffer_px));
  if (e == hipSuccess) e = alloc_zeroed(reinterpret_cast<void**>(&ret->d_vox), n * sizeof(float4));
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    rt4_set_err(err, errlen, "retina_create failed: %s", hipGetErrorString(e));
    (void)hipGetLastError();  // an allocation failure is not sticky: the context stays usable
    rt4_retina_destroy(ret);
    return RT4_ERR_HIP;
  }
  *out = ret;
  return RT4_OK;
}

void rt4_retina_reset(rt4_retina* ret) {
  if (!ret) return;
  ret->have = ret->vox_valid = false;
  ret->frames_done = 0;
}

int64_t rt4_retina_frames_done(const rt4_retina* ret) { return ret ? ret->frames_done : 0; }
rt4_light_px* rt4_retina_light(const rt4_retina* ret) { return ret ? ret->d_light : nullptr; }
rt4_gbuffer_px* rt4_retina_gbuffer(const rt4_retina* ret) { return ret ? ret->d_gbuf : nullptr; }
float* rt4_retina_voxels(const rt4_retina* ret) { return ret ? ret->d_vox : nullptr; }

int rt4_retina_accumulate_device(rt4_retina* ret, const rt4_uniforms* u, const float w_drct[4], float depth_size,
                                 int32_t n_frames, unsigned long long* d_counter, void* stream, char* err, size_t errlen) {
  if (!ret || !u || !w_drct) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (n_frames < 1) return rt4_set_err(err, errlen, "n_frames %d < 1", n_frames), RT4_ERR_ARG;
  if (u->resolution[0] != static_cast<float>(ret->w) || u->resolution[1] != static_cast<float>(ret->h))
    return rt4_set_err(err, errlen, "the uniforms' resolution is not the retina's slice size %d x %d", ret->w, ret->h), RT4_ERR_ARG;
  rt4_uniforms su;
  if (rt4_retina_slice_uniforms(u, w_drct, ret->depth, depth_size, 0, &su) != RT4_OK)
    return rt4_set_err(err, errlen, "depth_size must be finite and > 0"), RT4_ERR_ARG;
  rt4_context* ctx = ret->ctx;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const rt4_region reg{0, 0, ret->w, ret->h, 0, 0};
  const size_t slice_px = static_cast<size_t>(ret->w) * static_cast<size_t>(ret->h);
  if (ret->have && (std::memcmp(u, &ret->u, sizeof *u) != 0 || std::memcmp(w_drct, ret->w_drct, sizeof ret->w_drct) != 0 ||
                    std::memcmp(&depth_size, &ret->depth_size, sizeof depth_size) != 0))
    rt4_retina_reset(ret);  // another view: start over
  const int64_t first = ret->frames_done;
  if (first + n_frames > 0xFFFFFFFFll) return rt4_set_err(err, errlen, "frame numbers beyond 2^32 - 1"), RT4_ERR_ARG;
  const bool fresh = !ret->have;
  rt4_retina_reset(ret);  // until every launch below is enqueued: an error leaves the object reset
  if (fresh) {
    int st = post_launch(ctx, s, "retina reset", err, errlen,
                         [&] { return hipMemsetAsync(ret->d_light, 0, ret->voxels() * sizeof(rt4_light_px), s); });
    for (int32_t q = 0; q < ret->depth && st == RT4_OK; q++) {
      rt4_retina_slice_uniforms(u, w_drct, ret->depth, depth_size, q, &su);
      st = rt4_render_gbuffer_device(ctx, &su, &reg, ret->d_gbuf + static_cast<size_t>(q) * slice_px, ret->w, stream, err, errlen);
    }
    if (st != RT4_OK) return st;
  }
  std::vector<rt4_uniforms> us(static_cast<size_t>(n_frames));
  for (int32_t q = 0; q < ret->depth; q++) {
    rt4_retina_slice_uniforms(u, w_drct, ret->depth, depth_size, q, &su);
    for (int32_t f = 0; f < n_frames; f++)
      rt4_progressive_uniforms(&su, static_cast<uint32_t>(first + 1 + f), &us[static_cast<size_t>(f)]);
    const int st = rt4_render_light_device(ctx, us.data(), n_frames, &reg, ret->d_light + static_cast<size_t>(q) * slice_px, ret->w,
                                           d_counter, stream, err, errlen);
    if (st != RT4_OK) return st;
  }
  ret->have = true;
  ret->frames_done = first + n_frames;
  ret->u = *u;
  std::memcpy(ret->w_drct, w_drct, sizeof ret->w_drct);
  ret->depth_size = depth_size;
  return RT4_OK;
}

int rt4_retina_present_device(rt4_retina* ret, const rt4_retina_view* view, const rt4_retina_params* params, float k,
                              void* d_frame, int32_t format, int64_t frame_stride, int32_t ow, int32_t oh, void* stream,
                              char* err, size_t errlen) {
  if (!ret || !view || !d_frame) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (!ret->have) return rt4_set_err(err, errlen, "nothing accumulated (rt4_retina_accumulate_device)"), RT4_ERR_ARG;
  rt4_retina_params dp;
  if (!params) {
    rt4_retina_params_default(&dp);
    params = &dp;
  }
  const int64_t rs = ret->w, ss = static_cast<int64_t>(ret->w) * ret->h;
  const float alpha[3] = {params->alpha_sky, params->alpha_fill, params->alpha_edge};
  if (!ret->vox_valid || std::memcmp(alpha, ret->vox_alpha, sizeof alpha) != 0 || std::memcmp(&k, &ret->vox_k, sizeof k) != 0) {
    ret->vox_valid = false;
    const int st = rt4_retina_voxelize_device(ret->ctx, ret->d_light, rs, ss, ret->d_gbuf, rs, ss, k, params, ret->d_vox, rs, ss,
                                              ret->w, ret->h, ret->depth, stream, err, errlen);
    if (st != RT4_OK) return st;
    ret->vox_valid = true;
    std::memcpy(ret->vox_alpha, alpha, sizeof alpha);
    ret->vox_k = k;
  }
  return rt4_retina_project_device(ret->ctx, ret->d_vox, rs, ss, ret->w, ret->h, ret->depth, view, params, d_frame, format,
                                   frame_stride, ow, oh, stream, err, errlen);
}

int rt4_retina_read_host(rt4_retina* ret, rt4_light_px* light, rt4_gbuffer_px* gbuf, float* voxels, char* err,
                         size_t errlen) {
  if (!ret) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  HIP_TRY(hipSetDevice(ret->ctx->device));
  if (ret->ctx->launched) HIP_TRY(hipEventSynchronize(ret->ctx->done));
  const size_t n = ret->voxels();
  if (light) HIP_TRY(hipMemcpy(light, ret->d_light, n * sizeof(rt4_light_px), hipMemcpyDeviceToHost));
  if (gbuf) HIP_TRY(hipMemcpy(gbuf, ret->d_gbuf, n * sizeof(rt4_gbuffer_px), hipMemcpyDeviceToHost));
  if (voxels) HIP_TRY(hipMemcpy(voxels, ret->d_vox, n * sizeof(float4), hipMemcpyDeviceToHost));
  return RT4_OK;
}

}  // extern "C"
