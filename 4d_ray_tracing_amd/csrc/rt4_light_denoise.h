// rt4_light_denoise.h — the variance-guided a-trous filter of a light accumulator of rt4.h (rt4_light_denoise_device;
// DESIGN.md §4.38): kernels and entry points. From rt4_post.h: the argument checks, the launch bracket, the pixel grid,
// px_store_opaque, HostStage and grow_scratch; from rt4_light.h: light_tone and light_image. No other kernel uses
// anything from here.
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

constexpr int LD_MAX_TILED_STEP = 2;                    // strides staged in LDS
constexpr int LD_TILE_MAX = (PX_BX + 4 * LD_MAX_TILED_STEP) * (PX_BY + 4 * LD_MAX_TILED_STEP);  // 40 x 16 pixels
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

// levels = 0: rt4_light_resolve_kernel's frame, and {mean, n >= 2 ? V_0 : +inf} into filtered. The G-buffer plays no
// part: a filterable pixel has n >= 2, and its L_0 and V_0 are these.
__global__ __launch_bounds__(256) void rt4_light_denoise_level0_kernel(const rt4_light_px* __restrict__ light, int64_t light_stride,
                                                                       float k, void* __restrict__ frame, int32_t format,
                                                                       int64_t frame_stride, float4* __restrict__ filtered,
                                                                       int64_t filtered_stride, int32_t w, int32_t h) {
  const int2 xy = px_xy();
  const int x = xy.x, y = xy.y;
  if (x >= w || y >= h) return;
  const float4* st = reinterpret_cast<const float4*>(light + static_cast<int64_t>(y) * light_stride + x);
  const float4 m = st[0], t = st[1];
  const int32_t n = __float_as_int(t.y);
  const V3 c = n == 0 ? V3{0.0f, 0.0f, 0.0f} : V3{light_tone(k, m.x), light_tone(k, m.y), light_tone(k, m.z)};
  px_store_opaque(frame, format, static_cast<int64_t>(y) * frame_stride + x, c);
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
  const int2 xy = px_xy();
  const int x = xy.x, y = xy.y;
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
  const int ox = static_cast<int>(blockIdx.x) * PX_BX, oy = static_cast<int>(blockIdx.y) * PX_BY;
  const int x = ox + tx, y = oy + ty;
  const int s = a.step, w = a.w, h = a.h;
  const int R = 2 * s, T = PX_BX + 2 * R;  // halo, LDS row pitch (TILED)
  if (TILED) {
    const int n = T * (PX_BY + 2 * R);  // <= LD_TILE_MAX: the host launches this instantiation for s <= 2 only
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
  px_store_opaque(a.frame, a.format, static_cast<int64_t>(y) * a.frame_stride + x, c);
  if (a.filtered) a.filtered[static_cast<int64_t>(y) * a.filtered_stride + x] = make_float4(cr, cg, cb, cv);
}

}  // namespace

extern "C" {

uint64_t rt4_context_light_denoise_bytes(const rt4_context* ctx) {
  return ctx ? static_cast<uint64_t>(ctx->light_denoise.cap) * LD_SCRATCH_PX_BYTES : 0u;
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
  const PostImage in[2] = {light_image(d_light, light_stride, w, h),
                           post_image(d_gbuf, gbuf_stride, w, h, sizeof(rt4_gbuffer_px), "G-buffer")};
  const PostImage out[2] = {post_image(d_frame, frame_stride, w, h, static_cast<size_t>(px_bytes), "frame"),
                            post_image(d_filtered, filtered_stride, w, h, 16u, "filtered light")};
  int st = post_check_args(out, d_filtered ? 2 : 1, in, 2, err, errlen);
  if (st != RT4_OK) return st;
  if (params->levels < 0 || params->levels > RT4_LIGHT_DENOISE_MAX_LEVELS)
    return rt4_set_err(err, errlen, "levels %d not in [0, %d]", params->levels, RT4_LIGHT_DENOISE_MAX_LEVELS), RT4_ERR_ARG;
  if (!(params->sigma >= 0.0f) || !(params->eps >= 0.0f))  // negative or NaN
    return rt4_set_err(err, errlen, "sigma and eps must be >= 0"), RT4_ERR_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int32_t levels = params->levels;
  if (levels > 0) {  // a larger image than any before grows the scratch once
    st = grow_scratch(ctx, ctx->light_denoise, s, static_cast<size_t>(w) * static_cast<size_t>(h), LD_SCRATCH_PX_BYTES, err, errlen);
    if (st != RT4_OK) return st;
  }
  // the six arrays of the scratch, each for the context's largest image (offsets are multiples of their alignment)
  char* base = static_cast<char*>(ctx->light_denoise.d);
  const size_t cap = ctx->light_denoise.cap;
  float4* level[2] = {reinterpret_cast<float4*>(base), reinterpret_cast<float4*>(base + cap * 16u)};
  float4* gn = reinterpret_cast<float4*>(base + cap * 32u);
  int2* gi = reinterpret_cast<int2*>(base + cap * 48u);
  float* level_v[2] = {reinterpret_cast<float*>(base + cap * 56u), reinterpret_cast<float*>(base + cap * 60u)};
  return post_launch(ctx, s, "light denoise kernel", err, errlen, [&] {
    const dim3 grid = px_grid(w, h), block(256);
    float4* filtered = reinterpret_cast<float4*>(d_filtered);
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
    return le;
  });
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
  HostStage acc, g, out, fl;
  hipError_t e = acc.up(light, image_span(light_stride, w, h) * sizeof(rt4_light_px));
  if (e == hipSuccess) e = g.up(gbuf, image_span(gbuf_stride, w, h) * sizeof(rt4_gbuffer_px));
  if (e == hipSuccess) e = out.up(frame, image_span(frame_stride, w, h) * static_cast<size_t>(px_bytes));
  if (e == hipSuccess && filtered) e = fl.up(filtered, image_span(filtered_stride, w, h) * 16u);
  if (e == hipSuccess) {
    const int st = rt4_light_denoise_device(ctx, acc.as<const rt4_light_px>(), light_stride, g.as<const rt4_gbuffer_px>(),
                                            gbuf_stride, k, params, out.d, format, frame_stride, fl.as<float>(),
                                            filtered_stride, w, h, nullptr, err, errlen);
    if (st != RT4_OK) return st;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = out.down(frame);
    if (e == hipSuccess && filtered) e = fl.down(filtered);
  }
  if (e != hipSuccess) return rt4_set_err(err, errlen, "light_denoise_host failed: %s", hipGetErrorString(e)), RT4_ERR_HIP;
  return RT4_OK;
}

}  // extern "C"
