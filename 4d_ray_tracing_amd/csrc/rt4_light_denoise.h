// rt4_light_denoise.h — the variance-guided a-trous filter of a light accumulator of rt4.h (rt4_light_denoise_device;
// DESIGN.md §4.38): kernels and entry points. Part of rt4_trace.hip's translation unit (included at its end, after
// rt4_light.h: the context, the blend_* store helpers, the launch ordering, rp_span / rp_overlap, light_tone,
// light_check_image and LightStage live there); no other kernel uses anything from here.
//
// One call, in the shape of rt4_denoise.h: a pack pass builds level 0 (the state: {L, Y} 16 B and V 4 B) and the guide
// (normal 16 B; {id, depth} 8 B with id = the surface of a filterable pixel, else -1), then one pass per level between
// the two state images; the last level tone-maps and stores into the caller's frame in its format (fused: the level's
// result is in registers, an epilogue would write and re-read 20 B per pixel for it). Strides 1 and 2 stage a 32x8
// tile plus its halo in LDS as eleven dword arrays of at most 40 x 16 (a 32-lane half of a wave reads 32 consecutive
// dwords of one array, which ds_read_b32's 32-bank rule serves without conflicts at any row pitch: rt4_denoise.h);
// larger strides gather from global memory, the guide's id first so that a tap on another surface costs one 8-B load.
// The variance pre-filter reads p's eight unit neighbours: from the tile where there is one (its halo is >= 2).
// A pixel that is not filterable carries V = (n >= 2 ? V_0 : +inf) through the levels (nobody taps it), which is what
// d_filtered wants for it; its n == 0 case (colour 0) is read from the accumulator by the last level.
#pragma once

namespace {

constexpr int LD_BX = 32, LD_BY = 8;                    // pixels per workgroup (one lane each)
constexpr int LD_MAX_TILED_STEP = 2;                    // strides staged in LDS
constexpr int LD_TILE_MAX = (LD_BX + 4 * LD_MAX_TILED_STEP) * (LD_BY + 4 * LD_MAX_TILED_STEP);  // 40 x 16 pixels
constexpr size_t LD_SCRATCH_PX_BYTES = 64;              // 2 x (16 + 4) state, 16 + 8 guide

struct LdArgs {
  int32_t w, h, step;
  float cos_min, depth_tol, sigma, eps, k;
  const float4* src;   // level l: {L_r, L_g, L_b, Y}, row stride w
  const float* src_v;  // level l: V
  const float4* gn;    // guide: normals
  const int2* gi;      // guide: {id, depth bits}
  float4* dst;         // level l + 1, or null: the last level stores into frame / filtered
  float* dst_v;
  const rt4_light_px* light;  // the last level: n of the pixels that are not filterable
  int64_t light_stride;
  void* frame;
  int64_t frame_stride;
  int32_t format;
  float4* filtered;    // may be null
  int64_t filtered_stride;
};

// rt4.h: V_0, the radicand of se in rt4_light_noise_kernel.
__device__ __forceinline__ float ld_variance0(float m2, int32_t n) {
  return (m2 / static_cast<float>(n - 1)) / static_cast<float>(n);
}

// A colour through the store rule of the format, alpha 1 (rt4_light_resolve_kernel does the same).
__device__ __forceinline__ void ld_store(void* frame, int32_t format, int64_t at, V3 c) {
  if (format == RT4_FRAME_RGBA16F) {
    h4v zero;
    zero[0] = zero[1] = zero[2] = zero[3] = static_cast<_Float16>(0.0f);
    reinterpret_cast<h4v*>(frame)[at] = blend_f16(c, 1.0f, zero);
  } else if (format == RT4_FRAME_RGBA8) {
    reinterpret_cast<uint32_t*>(frame)[at] = blend_u8(c, 1.0f, 0u);
  } else {
    reinterpret_cast<float4*>(frame)[at] = blend_f32(c, 1.0f, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
  }
}

// levels = 0: rt4_light_resolve_kernel's frame, and {mean, n >= 2 ? V_0 : +inf} into filtered. The G-buffer plays no
// part: a filterable pixel has n >= 2, and its L_0 and V_0 are these.
__global__ __launch_bounds__(256) void rt4_light_denoise_level0_kernel(const rt4_light_px* __restrict__ light, int64_t light_stride,
                                                                       float k, void* __restrict__ frame, int32_t format,
                                                                       int64_t frame_stride, float4* __restrict__ filtered,
                                                                       int64_t filtered_stride, int32_t w, int32_t h) {
  const int x = static_cast<int>(blockIdx.x) * LD_BX + static_cast<int>(threadIdx.x & 31u);
  const int y = static_cast<int>(blockIdx.y) * LD_BY + static_cast<int>(threadIdx.x >> 5);
  if (x >= w || y >= h) return;
  const float4* st = reinterpret_cast<const float4*>(light + static_cast<int64_t>(y) * light_stride + x);
  const float4 m = st[0], t = st[1];
  const int32_t n = __float_as_int(t.y);
  const V3 c = n == 0 ? V3{0.0f, 0.0f, 0.0f} : V3{light_tone(k, m.x), light_tone(k, m.y), light_tone(k, m.z)};
  ld_store(frame, format, static_cast<int64_t>(y) * frame_stride + x, c);
  if (filtered)
    filtered[static_cast<int64_t>(y) * filtered_stride + x] =
        make_float4(m.x, m.y, m.z, n >= 2 ? ld_variance0(t.x, n) : __builtin_inff());
}

// Level 0 and the guide (rt4.h: p is filterable iff surface(p) >= 0 && refl_prob(p) <= max_refl_prob && n(p) >= 2).
__global__ __launch_bounds__(256) void rt4_light_denoise_pack_kernel(const rt4_light_px* __restrict__ light, int64_t light_stride,
                                                                     const rt4_gbuffer_px* __restrict__ gbuf, int64_t gbuf_stride,
                                                                     int32_t w, int32_t h, float max_refl_prob,
                                                                     float4* __restrict__ s0, float* __restrict__ v0,
                                                                     float4* __restrict__ gn, int2* __restrict__ gi) {
  const int x = static_cast<int>(blockIdx.x) * LD_BX + static_cast<int>(threadIdx.x & 31u);
  const int y = static_cast<int>(blockIdx.y) * LD_BY + static_cast<int>(threadIdx.x >> 5);
  if (x >= w || y >= h) return;
  const float4* st = reinterpret_cast<const float4*>(light + static_cast<int64_t>(y) * light_stride + x);
  const float4 m = st[0], t = st[1];  // m: mean rgb, mean_y; t: m2, n
  const int32_t n = __float_as_int(t.y);
  const float4* g = reinterpret_cast<const float4*>(gbuf + static_cast<int64_t>(y) * gbuf_stride + x);
  const float4 nn = g[0], gm = g[1];  // gm: depth, surface, refl_prob, glow
  const int surface = __float_as_int(gm.y);
  const bool filterable = surface >= 0 && gm.z <= max_refl_prob && n >= 2;
  const int64_t p = static_cast<int64_t>(y) * w + x;
  s0[p] = m;
  v0[p] = n >= 2 ? ld_variance0(t.x, n) : __builtin_inff();
  gn[p] = nn;
  gi[p] = make_int2(filterable ? surface : -1, __float_as_int(gm.x));
}

// One level (rt4.h): the pre-filter's taps dy = -1..1 (outer), dx = -1..1 (inner) at unit stride, then the 25 taps
// dy = -2..2 (outer), dx = -2..2 (inner) at stride s; every acc = acc + o * x is a multiply, then an add.
template <bool TILED>
__global__ __launch_bounds__(256) void rt4_light_denoise_level_kernel(const LdArgs a) {
  constexpr float H[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
  constexpr float G3[3] = {1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f};
  constexpr int LN = TILED ? LD_TILE_MAX : 1;
  __shared__ float l_r[LN], l_g[LN], l_b[LN], l_y[LN], l_v[LN];
  __shared__ float l_nx[LN], l_ny[LN], l_nz[LN], l_nw[LN], l_z[LN];
  __shared__ int l_id[LN];
  const int tx = static_cast<int>(threadIdx.x & 31u), ty = static_cast<int>(threadIdx.x >> 5);
  const int ox = static_cast<int>(blockIdx.x) * LD_BX, oy = static_cast<int>(blockIdx.y) * LD_BY;
  const int x = ox + tx, y = oy + ty;
  const int s = a.step, w = a.w, h = a.h;
  const int R = 2 * s, T = LD_BX + 2 * R;  // halo, LDS row pitch (TILED)
  if (TILED) {
    const int n = T * (LD_BY + 2 * R);  // <= LD_TILE_MAX: the host launches this instantiation for s <= 2 only
    for (int k = static_cast<int>(threadIdx.x); k < n; k += 256) {
      const int ly = k / T, lx = k - ly * T;
      const int gx = ox - R + lx, gy = oy - R + ly;
      int id = -2;  // outside the image: equal to no filterable pixel's id
      float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nn = c;
      float z = 0.0f, v = 0.0f;
      if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
        const int64_t q = static_cast<int64_t>(gy) * w + gx;
        const int2 gi = a.gi[q];
        id = gi.x;
        z = __int_as_float(gi.y);
        nn = a.gn[q];
        c = a.src[q];
        v = a.src_v[q];
      }
      l_id[k] = id;
      l_z[k] = z;
      l_nx[k] = nn.x; l_ny[k] = nn.y; l_nz[k] = nn.z; l_nw[k] = nn.w;
      l_r[k] = c.x; l_g[k] = c.y; l_b[k] = c.z; l_y[k] = c.w;
      l_v[k] = v;
    }
    __syncthreads();
  }
  if (x >= w || y >= h) return;
  const int64_t p = static_cast<int64_t>(y) * w + x;
  const int lp = (ty + R) * T + tx + R;  // p in the LDS tile
  const float4 cp = a.src[p];
  const float vp = a.src_v[p];
  const int2 gp = a.gi[p];
  const int idp = gp.x;
  float cr = cp.x, cg = cp.y, cb = cp.z, cy = cp.w, cv = vp;
  if (idp >= 0) {  // filterable
    // 1. the variance pre-filter
    float va = 0.0f, vw = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
      for (int dx = -1; dx <= 1; dx++) {
        const float g = G3[dy + 1] * G3[dx + 1];  // exact: a power of two
        bool counts = true;
        float qv = vp;
        if (dx != 0 || dy != 0) {
          if (TILED) {
            const int lq = lp + dy * T + dx;
            counts = l_id[lq] == idp;
            qv = l_v[lq];
          } else {
            const int qx = x + dx, qy = y + dy;
            counts = false;
            if (qx >= 0 && qx < w && qy >= 0 && qy < h) {
              const int64_t q = static_cast<int64_t>(qy) * w + qx;
              if (a.gi[q].x == idp) {
                counts = true;
                qv = a.src_v[q];
              }
            }
          }
        }
        if (counts) {
          va = __fadd_rn(va, __fmul_rn(g, qv));
          vw = __fadd_rn(vw, g);
        }
      }
    }
    const float den = fmaf_(a.sigma, sqrt_(va / vw), a.eps);  // the centre tap always counts: vw >= 1/4
    // 2. the 25 taps
    const float zp = __int_as_float(gp.y);
    const float4 n4 = a.gn[p];
    const V4 np{n4.x, n4.y, n4.z, n4.w};
    const float tol = __fmul_rn(a.depth_tol, zp);
    const float cos_min = a.cos_min;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, ay = 0.0f, av = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
      for (int dx = -2; dx <= 2; dx++) {
        const float k = H[dy + 2] * H[dx + 2];  // exact: a dyadic rational with a 4-bit numerator
        bool counts = true;
        float om = k;
        float qr = cp.x, qg = cp.y, qb = cp.z, qy_ = cp.w, qv = vp;
        if (dx != 0 || dy != 0) {
          if (TILED) {
            const int lq = lp + (dy * T + dx) * s;
            counts = l_id[lq] == idp && dot(np, V4{l_nx[lq], l_ny[lq], l_nz[lq], l_nw[lq]}) >= cos_min &&
                     __builtin_fabsf(__fsub_rn(l_z[lq], zp)) <= tol;
            qr = l_r[lq]; qg = l_g[lq]; qb = l_b[lq]; qy_ = l_y[lq]; qv = l_v[lq];
          } else {
            const int qx = x + s * dx, qy = y + s * dy;
            counts = false;
            if (qx >= 0 && qx < w && qy >= 0 && qy < h) {
              const int64_t q = static_cast<int64_t>(qy) * w + qx;
              const int2 gq = a.gi[q];
              if (gq.x == idp && __builtin_fabsf(__fsub_rn(__int_as_float(gq.y), zp)) <= tol) {
                const float4 nq = a.gn[q];
                if (dot(np, V4{nq.x, nq.y, nq.z, nq.w}) >= cos_min) {
                  const float4 cq = a.src[q];
                  counts = true;
                  qr = cq.x; qg = cq.y; qb = cq.z; qy_ = cq.w;
                  qv = a.src_v[q];
                }
              }
            }
          }
          if (counts) {  // the geometry test passed: the luminance edge-stop
            const float t = __builtin_fabsf(__fsub_rn(qy_, cp.w)) / den;
            const float wl = 1.0f / fmaf_(t, t, 1.0f);
            om = __fmul_rn(k, wl);
            counts = om > 0.0f;  // false for NaN
          }
        }
        if (counts) {
          ar = __fadd_rn(ar, __fmul_rn(om, qr));
          ag = __fadd_rn(ag, __fmul_rn(om, qg));
          ab = __fadd_rn(ab, __fmul_rn(om, qb));
          ay = __fadd_rn(ay, __fmul_rn(om, qy_));
          av = __fadd_rn(av, __fmul_rn(__fmul_rn(om, om), qv));
          wsum = __fadd_rn(wsum, om);
        }
      }
    }
    // 3. the centre tap always counts: wsum >= 9/64
    cr = ar / wsum;
    cg = ag / wsum;
    cb = ab / wsum;
    cy = ay / wsum;
    cv = av / __fmul_rn(wsum, wsum);
  }
  if (a.dst) {
    a.dst[p] = make_float4(cr, cg, cb, cy);
    a.dst_v[p] = cv;
    return;
  }
  // the last level: the tone map once, the caller's format, alpha 1; a pixel that is not filterable gets what
  // rt4_light_resolve_kernel writes (its state is still the accumulator's mean; colour 0 for n == 0)
  bool empty = false;
  if (idp < 0)
    empty = reinterpret_cast<const int32_t*>(a.light + static_cast<int64_t>(y) * a.light_stride + x)[5] == 0;
  const V3 c = empty ? V3{0.0f, 0.0f, 0.0f} : V3{light_tone(a.k, cr), light_tone(a.k, cg), light_tone(a.k, cb)};
  ld_store(a.frame, a.format, static_cast<int64_t>(y) * a.frame_stride + x, c);
  if (a.filtered) a.filtered[static_cast<int64_t>(y) * a.filtered_stride + x] = make_float4(cr, cg, cb, cv);
}

}  // namespace

extern "C" {

uint64_t rt4_context_light_denoise_bytes(const rt4_context* ctx) {
  return ctx ? static_cast<uint64_t>(ctx->light_denoise_px) * LD_SCRATCH_PX_BYTES : 0u;
}

int rt4_light_denoise_device(rt4_context* ctx, const rt4_light_px* d_light, int64_t light_stride,
                             const rt4_gbuffer_px* d_gbuf, int64_t gbuf_stride, float k,
                             const rt4_light_denoise_params* params, void* d_frame, int32_t format, int64_t frame_stride,
                             float* d_filtered, int64_t filtered_stride, int32_t w, int32_t h, void* stream, char* err,
                             size_t errlen) {
  if (!ctx || !d_light || !d_gbuf || !params || !d_frame) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const int32_t px_bytes = rt4_frame_format_bytes(format);
  if (px_bytes == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || w > 65535 || h > 65535)
    return rt4_set_err(err, errlen, "image size %d x %d not in [1, 65535]", w, h), RT4_ERR_ARG;
  int st = light_check_image(d_light, light_stride, w, "light accumulator", 16u, err, errlen);
  if (st == RT4_OK) st = light_check_image(d_gbuf, gbuf_stride, w, "G-buffer", 16u, err, errlen);
  if (st == RT4_OK) st = light_check_image(d_frame, frame_stride, w, "frame", static_cast<size_t>(px_bytes), err, errlen);
  if (st == RT4_OK && d_filtered) st = light_check_image(d_filtered, filtered_stride, w, "filtered light", 16u, err, errlen);
  if (st != RT4_OK) return st;
  if (params->levels < 0 || params->levels > RT4_LIGHT_DENOISE_MAX_LEVELS)
    return rt4_set_err(err, errlen, "levels %d not in [0, %d]", params->levels, RT4_LIGHT_DENOISE_MAX_LEVELS), RT4_ERR_ARG;
  if (!(params->sigma >= 0.0f) || !(params->eps >= 0.0f))  // negative or NaN
    return rt4_set_err(err, errlen, "sigma and eps must be >= 0"), RT4_ERR_ARG;
  const RpSpan in[2] = {rp_span(d_light, light_stride, w, h, sizeof(rt4_light_px)),
                        rp_span(d_gbuf, gbuf_stride, w, h, sizeof(rt4_gbuffer_px))};
  RpSpan out[2];
  int n_out = 0;
  out[n_out++] = rp_span(d_frame, frame_stride, w, h, static_cast<size_t>(px_bytes));
  if (d_filtered) out[n_out++] = rp_span(d_filtered, filtered_stride, w, h, 16u);
  if (n_out == 2 && rp_overlap(out[0], out[1])) return rt4_set_err(err, errlen, "the two outputs overlap"), RT4_ERR_ARG;
  for (int o = 0; o < n_out; o++)
    for (const RpSpan& i : in)
      if (rp_overlap(out[o], i)) return rt4_set_err(err, errlen, "an output overlaps an input"), RT4_ERR_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t npx = static_cast<size_t>(w) * static_cast<size_t>(h);
  const int32_t levels = params->levels;
  if (levels > 0 && ctx->light_denoise_px < npx) {  // a larger image than any before: wait for the launches in flight, grow once
    HIP_TRY(hipStreamSynchronize(s));
    if (ctx->launched) HIP_TRY(hipEventSynchronize(ctx->done));
    if (ctx->d_light_denoise) (void)hipFree(ctx->d_light_denoise);
    ctx->d_light_denoise = nullptr;
    ctx->light_denoise_px = 0;
    HIP_TRY(hipMalloc(&ctx->d_light_denoise, npx * LD_SCRATCH_PX_BYTES));
    ctx->light_denoise_px = npx;
  }
  // the six arrays of the scratch, each for the context's largest image (offsets are multiples of their alignment)
  char* base = static_cast<char*>(ctx->d_light_denoise);
  const size_t cap = ctx->light_denoise_px;
  float4* level[2] = {reinterpret_cast<float4*>(base), reinterpret_cast<float4*>(base + cap * 16u)};
  float4* gn = reinterpret_cast<float4*>(base + cap * 32u);
  int2* gi = reinterpret_cast<int2*>(base + cap * 48u);
  float* level_v[2] = {reinterpret_cast<float*>(base + cap * 56u), reinterpret_cast<float*>(base + cap * 60u)};
  int rc = order_launch(ctx, s, err, errlen);
  if (rc != RT4_OK) return rc;
  const dim3 grid(static_cast<unsigned>((w + LD_BX - 1) / LD_BX), static_cast<unsigned>((h + LD_BY - 1) / LD_BY)), block(256);
  float4* filtered = reinterpret_cast<float4*>(d_filtered);
  (void)hipGetLastError();
  if (levels == 0)
    hipLaunchKernelGGL(rt4_light_denoise_level0_kernel, grid, block, 0, s, d_light, light_stride, k, d_frame, format,
                       frame_stride, filtered, filtered_stride, w, h);
  else
    hipLaunchKernelGGL(rt4_light_denoise_pack_kernel, grid, block, 0, s, d_light, light_stride, d_gbuf, gbuf_stride, w, h,
                       params->max_refl_prob, level[0], level_v[0], gn, gi);
  hipError_t le = hipGetLastError();
  for (int32_t l = 0; l < levels && le == hipSuccess; l++) {
    const bool last = l + 1 == levels;
    LdArgs a;
    a.w = w;
    a.h = h;
    a.step = 1 << l;
    a.cos_min = params->cos_min;
    a.depth_tol = params->depth_tol;
    a.sigma = params->sigma;
    a.eps = params->eps;
    a.k = k;
    a.src = level[l & 1];
    a.src_v = level_v[l & 1];
    a.gn = gn;
    a.gi = gi;
    a.dst = last ? nullptr : level[(l + 1) & 1];
    a.dst_v = last ? nullptr : level_v[(l + 1) & 1];
    a.light = d_light;
    a.light_stride = light_stride;
    a.frame = d_frame;
    a.frame_stride = frame_stride;
    a.format = format;
    a.filtered = filtered;
    a.filtered_stride = filtered_stride;
    if (a.step <= LD_MAX_TILED_STEP) hipLaunchKernelGGL(rt4_light_denoise_level_kernel<true>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(rt4_light_denoise_level_kernel<false>, grid, block, 0, s, a);
    le = hipGetLastError();
  }
  rc = done_launch(ctx, s, err, errlen);
  if (le != hipSuccess) {
    rt4_set_err(err, errlen, "light denoise kernel launch failed: %s", hipGetErrorString(le));
    return RT4_ERR_HIP;
  }
  return rc;
}

int rt4_light_denoise_host(rt4_context* ctx, const rt4_light_px* light, int64_t light_stride, const rt4_gbuffer_px* gbuf,
                           int64_t gbuf_stride, float k, const rt4_light_denoise_params* params, void* frame,
                           int32_t format, int64_t frame_stride, float* filtered, int64_t filtered_stride, int32_t w,
                           int32_t h, char* err, size_t errlen) {
  if (!ctx || !light || !gbuf || !params || !frame) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const int32_t px_bytes = rt4_frame_format_bytes(format);
  if (px_bytes == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || light_stride < w || gbuf_stride < w || frame_stride < w || (filtered && filtered_stride < w))
    return rt4_set_err(err, errlen, "bad image size or row stride"), RT4_ERR_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  LightStage acc, g, out, fl;
  hipError_t e = acc.up(light, image_span(light_stride, w, h) * sizeof(rt4_light_px));
  if (e == hipSuccess) e = g.up(gbuf, image_span(gbuf_stride, w, h) * sizeof(rt4_gbuffer_px));
  if (e == hipSuccess) e = out.up(frame, image_span(frame_stride, w, h) * static_cast<size_t>(px_bytes));
  if (e == hipSuccess && filtered) e = fl.up(filtered, image_span(filtered_stride, w, h) * 16u);
  if (e == hipSuccess) {
    const int st = rt4_light_denoise_device(ctx, static_cast<const rt4_light_px*>(acc.d), light_stride,
                                            static_cast<const rt4_gbuffer_px*>(g.d), gbuf_stride, k, params, out.d, format,
                                            frame_stride, static_cast<float*>(fl.d), filtered_stride, w, h, nullptr, err,
                                            errlen);
    if (st != RT4_OK) return st;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = out.down(frame);
    if (e == hipSuccess && filtered) e = fl.down(filtered);
  }
  if (e != hipSuccess) return rt4_set_err(err, errlen, "light_denoise_host failed: %s", hipGetErrorString(e)), RT4_ERR_HIP;
  return RT4_OK;
}

}  // extern "C"
