// rt4_denoise.h — the edge-stopping a-trous filter of rt4.h (rt4_denoise_device): kernels and
// entry points. From rt4_post.h: the argument checks, the launch bracket, the pixel grid, px_decode, HostStage and
// grow_scratch; from no other pass. No trace kernel uses anything from here.
//
// One call: a pack pass decodes the input frame to fp32 (level 0) and repacks the G-buffer into the guide
// (normal 16 B; {id, depth} 8 B with id = the surface of a filterable pixel, else -1), then one pass per level
// between the two scratch images; the last level stores into the caller's frame in its format.
// Strides 1 and 2 stage a 32x8 tile plus its halo in LDS (36 B per pixel as nine dword arrays: a 32-lane half of a
// wave reads 32 consecutive dwords of one array, which ds_read_b32's 32-bank rule serves without conflicts at any
// row pitch); larger strides gather from global memory, the guide's id first so that a tap on another surface costs
// one 8-B load.
#pragma once

namespace {

constexpr int DN_MAX_TILED_STEP = 2;                    // strides staged in LDS
constexpr int DN_TILE_MAX = (PX_BX + 4 * DN_MAX_TILED_STEP) * (PX_BY + 4 * DN_MAX_TILED_STEP);  // 40 x 16 pixels

struct DnArgs {
  int32_t w, h, step;
  float cos_min, depth_tol;
  const float4* src;  // level l, row stride w
  const float4* gn;   // guide: normals
  const int2* gi;     // guide: {id, depth bits}
  float4* dst;        // level l + 1, or null: the last level stores into out
  const void* in;     // the caller's input frame (stored alpha; stored bits of pixels that are not filterable)
  void* out;
  int64_t in_stride, out_stride;
  int32_t format;
};

// C_0 and the guide (rt4.h: p is filterable iff surface(p) >= 0 && refl_prob(p) <= max_refl_prob).
__global__ __launch_bounds__(256) void rt4_denoise_pack_kernel(const void* __restrict__ in, int64_t in_stride, int32_t format,
                                                               const rt4_gbuffer_px* __restrict__ gbuf, int64_t gbuf_stride,
                                                               int32_t w, int32_t h, float max_refl_prob,
                                                               float4* __restrict__ c0, float4* __restrict__ gn,
                                                               int2* __restrict__ gi) {
  const int2 xy = px_xy();
  const int x = xy.x, y = xy.y;
  if (x >= w || y >= h) return;
  const float4 c = px_decode(in, format, static_cast<int64_t>(y) * in_stride + x);
  const float4* g = reinterpret_cast<const float4*>(gbuf + static_cast<int64_t>(y) * gbuf_stride + x);
  const float4 n = g[0], m = g[1];  // m: depth, surface, refl_prob, glow
  const int surface = __float_as_int(m.y);
  const bool filterable = surface >= 0 && m.z <= max_refl_prob;
  const int64_t p = static_cast<int64_t>(y) * w + x;
  c0[p] = c;
  gn[p] = n;
  gi[p] = make_int2(filterable ? surface : -1, __float_as_int(m.x));
}

// One level (rt4.h): taps dy = -2..2 (outer), dx = -2..2 (inner), acc = acc + k * C as a multiply, then an add.
template <bool TILED>
__global__ __launch_bounds__(256) void rt4_denoise_level_kernel(const DnArgs a) {
  constexpr float H[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
  __shared__ float l_r[TILED ? DN_TILE_MAX : 1], l_g[TILED ? DN_TILE_MAX : 1], l_b[TILED ? DN_TILE_MAX : 1];
  __shared__ float l_nx[TILED ? DN_TILE_MAX : 1], l_ny[TILED ? DN_TILE_MAX : 1], l_nz[TILED ? DN_TILE_MAX : 1],
      l_nw[TILED ? DN_TILE_MAX : 1], l_z[TILED ? DN_TILE_MAX : 1];
  __shared__ int l_id[TILED ? DN_TILE_MAX : 1];
  const int tx = static_cast<int>(threadIdx.x & 31u), ty = static_cast<int>(threadIdx.x >> 5);
  const int ox = static_cast<int>(blockIdx.x) * PX_BX, oy = static_cast<int>(blockIdx.y) * PX_BY;
  const int x = ox + tx, y = oy + ty;
  const int s = a.step, w = a.w, h = a.h;
  const int R = 2 * s, T = PX_BX + 2 * R;  // halo, LDS row pitch (TILED)
  if (TILED) {
    const int n = T * (PX_BY + 2 * R);  // <= DN_TILE_MAX: the host launches this instantiation for s <= 2 only
    for (int k = static_cast<int>(threadIdx.x); k < n; k += 256) {
      const int ly = k / T, lx = k - ly * T;
      const int gx = ox - R + lx, gy = oy - R + ly;
      int id = -2;  // outside the image: equal to no filterable pixel's id
      float4 c = make_float4(0.0f, 0.0f, 0.0f, 0.0f), nn = c;
      float z = 0.0f;
      if (gx >= 0 && gx < w && gy >= 0 && gy < h) {
        const int64_t q = static_cast<int64_t>(gy) * w + gx;
        const int2 gi = a.gi[q];
        id = gi.x;
        z = __int_as_float(gi.y);
        nn = a.gn[q];
        c = a.src[q];
      }
      l_id[k] = id;
      l_z[k] = z;
      l_nx[k] = nn.x; l_ny[k] = nn.y; l_nz[k] = nn.z; l_nw[k] = nn.w;
      l_r[k] = c.x; l_g[k] = c.y; l_b[k] = c.z;
    }
    __syncthreads();
  }
  if (x >= w || y >= h) return;
  const int64_t p = static_cast<int64_t>(y) * w + x;
  const int lp = (ty + R) * T + tx + R;  // p in the LDS tile
  const float4 cp = a.src[p];
  const int2 gp = a.gi[p];
  const int idp = gp.x;
  float cr = cp.x, cg = cp.y, cb = cp.z;
  if (idp >= 0) {  // filterable
    const float zp = __int_as_float(gp.y);
    const float4 n4 = a.gn[p];
    const V4 np{n4.x, n4.y, n4.z, n4.w};
    const float tol = __fmul_rn(a.depth_tol, zp);
    const float cos_min = a.cos_min;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, wsum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
      for (int dx = -2; dx <= 2; dx++) {
        const float k = H[dy + 2] * H[dx + 2];  // exact: a dyadic rational with a 4-bit numerator
        bool counts = true;
        float qr = cp.x, qg = cp.y, qb = cp.z;
        if (dx != 0 || dy != 0) {
          if (TILED) {
            const int lq = lp + (dy * T + dx) * s;
            counts = l_id[lq] == idp && dot(np, V4{l_nx[lq], l_ny[lq], l_nz[lq], l_nw[lq]}) >= cos_min &&
                     __builtin_fabsf(__fsub_rn(l_z[lq], zp)) <= tol;
            qr = l_r[lq]; qg = l_g[lq]; qb = l_b[lq];
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
                  qr = cq.x; qg = cq.y; qb = cq.z;
                }
              }
            }
          }
        }
        if (counts) {
          ar = __fadd_rn(ar, __fmul_rn(k, qr));
          ag = __fadd_rn(ag, __fmul_rn(k, qg));
          ab = __fadd_rn(ab, __fmul_rn(k, qb));
          wsum = __fadd_rn(wsum, k);
        }
      }
    }
    cr = ar / wsum;  // the centre tap always counts: wsum >= 9/64
    cg = ag / wsum;
    cb = ab / wsum;
  }
  if (a.dst) {
    a.dst[p] = make_float4(cr, cg, cb, cp.w);
    return;
  }
  // the last level: the caller's format, the input's stored alpha; a pixel that is not filterable keeps the input's
  // stored bits. blend_*(c, 1, 0) is the store rule of the format (c * 1 + 0 * 0, then the format's rounding).
  const int64_t ai = static_cast<int64_t>(y) * a.in_stride + x, ao = static_cast<int64_t>(y) * a.out_stride + x;
  const V3 c{cr, cg, cb};
  if (a.format == RT4_FRAME_RGBA16F) {
    const h4v vin = reinterpret_cast<const h4v*>(a.in)[ai];
    h4v v = vin;
    if (idp >= 0) {
      h4v zero;
      zero[0] = zero[1] = zero[2] = zero[3] = static_cast<_Float16>(0.0f);
      v = blend_f16(c, 1.0f, zero);
      v[3] = vin[3];
    }
    reinterpret_cast<h4v*>(a.out)[ao] = v;
  } else if (a.format == RT4_FRAME_RGBA8) {
    const uint32_t vin = reinterpret_cast<const uint32_t*>(a.in)[ai];
    reinterpret_cast<uint32_t*>(a.out)[ao] = idp >= 0 ? ((blend_u8(c, 1.0f, 0u) & 0x00FFFFFFu) | (vin & 0xFF000000u)) : vin;
  } else {
    const float4 vin = reinterpret_cast<const float4*>(a.in)[ai];
    reinterpret_cast<float4*>(a.out)[ao] = idp >= 0 ? make_float4(cr, cg, cb, vin.w) : vin;
  }
}

}  // namespace

extern "C" {

uint64_t rt4_context_denoise_bytes(const rt4_context* ctx) { return ctx ? static_cast<uint64_t>(ctx->denoise.cap) * 56u : 0u; }

int rt4_denoise_device(rt4_context* ctx, const void* d_in, int64_t in_stride_px, void* d_out, int64_t out_stride_px,
                       int32_t format, int32_t w, int32_t h, const rt4_gbuffer_px* d_gbuf, int64_t gbuf_stride_px,
                       const rt4_denoise_params* params, void* stream, char* err, size_t errlen) {
  if (!ctx || !d_in || !d_out || !d_gbuf || !params) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const size_t px_bytes = static_cast<size_t>(rt4_frame_format_bytes(format));
  if (px_bytes == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || w > 65535 || h > 65535)
    return rt4_set_err(err, errlen, "frame size %d x %d not in [1, 65535]", w, h), RT4_ERR_ARG;
  if (params->levels < 1 || params->levels > RT4_DENOISE_MAX_LEVELS)
    return rt4_set_err(err, errlen, "levels %d not in [1, %d]", params->levels, RT4_DENOISE_MAX_LEVELS), RT4_ERR_ARG;
  // rt4.h promises the overlap check for d_in and d_out only: the G-buffer is checked for itself
  const PostImage in = post_image(d_in, in_stride_px, w, h, px_bytes, "d_in");
  const PostImage out = post_image(d_out, out_stride_px, w, h, px_bytes, "d_out");
  int st = post_check_image(post_image(d_gbuf, gbuf_stride_px, w, h, sizeof(rt4_gbuffer_px), "G-buffer"), err, errlen);
  if (st == RT4_OK) st = post_check_args(&out, 1, &in, 1, err, errlen);
  if (st != RT4_OK) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // a larger frame than any before grows the scratch once
  st = grow_scratch(ctx, ctx->denoise, s, static_cast<size_t>(w) * static_cast<size_t>(h), 56u, err, errlen);
  if (st != RT4_OK) return st;
  // the four arrays of the scratch, each for the context's largest frame (16-B aligned: multiples of 16 B)
  char* base = static_cast<char*>(ctx->denoise.d);
  float4* level[2] = {reinterpret_cast<float4*>(base), reinterpret_cast<float4*>(base + ctx->denoise.cap * 16u)};
  float4* gn = reinterpret_cast<float4*>(base + ctx->denoise.cap * 32u);
  int2* gi = reinterpret_cast<int2*>(base + ctx->denoise.cap * 48u);
  return post_launch(ctx, s, "denoise kernel", err, errlen, [&] {
    const dim3 grid = px_grid(w, h), block(256);
    hipLaunchKernelGGL(rt4_denoise_pack_kernel, grid, block, 0, s, d_in, in_stride_px, format, d_gbuf, gbuf_stride_px, w, h,
                       params->max_refl_prob, level[0], gn, gi);
    hipError_t le = hipGetLastError();
    for (int32_t l = 0; l < params->levels && le == hipSuccess; l++) {
      DnArgs a;
      a.w = w;
      a.h = h;
      a.step = 1 << l;
      a.cos_min = params->cos_min;
      a.depth_tol = params->depth_tol;
      a.src = level[l & 1];
      a.gn = gn;
      a.gi = gi;
      a.dst = l + 1 < params->levels ? level[(l + 1) & 1] : nullptr;
      a.in = d_in;
      a.out = d_out;
      a.in_stride = in_stride_px;
      a.out_stride = out_stride_px;
      a.format = format;
      if (a.step <= DN_MAX_TILED_STEP) hipLaunchKernelGGL(rt4_denoise_level_kernel<true>, grid, block, 0, s, a);
      else hipLaunchKernelGGL(rt4_denoise_level_kernel<false>, grid, block, 0, s, a);
      le = hipGetLastError();
    }
    return le;
  });
}

int rt4_denoise_host(rt4_context* ctx, const void* in, int64_t in_stride_px, void* out, int64_t out_stride_px,
                     int32_t format, int32_t w, int32_t h, const rt4_gbuffer_px* gbuf, int64_t gbuf_stride_px,
                     const rt4_denoise_params* params, char* err, size_t errlen) {
  if (!ctx || !in || !out || !gbuf || !params) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const size_t px_bytes = static_cast<size_t>(rt4_frame_format_bytes(format));
  if (px_bytes == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || in_stride_px < w || out_stride_px < w || gbuf_stride_px < w)
    return rt4_set_err(err, errlen, "bad frame size or row stride"), RT4_ERR_ARG;
  const PostImage hi = post_image(in, in_stride_px, w, h, px_bytes, "in"), ho = post_image(out, out_stride_px, w, h, px_bytes, "out");
  if (post_check_overlap(&ho, 1, &hi, 1, err, errlen) != RT4_OK) return RT4_ERR_ARG;  // the host images themselves
  HIP_TRY(hipSetDevice(ctx->device));
  HostStage di, dout, dg;
  hipError_t e = di.up(in, post_bytes(hi));
  if (e == hipSuccess) e = dout.up(out, post_bytes(ho));
  if (e == hipSuccess) e = dg.up(gbuf, image_span(gbuf_stride_px, w, h) * sizeof(rt4_gbuffer_px));
  if (e == hipSuccess) {
    const int st = rt4_denoise_device(ctx, di.d, in_stride_px, dout.d, out_stride_px, format, w, h, dg.as<const rt4_gbuffer_px>(),
                                      gbuf_stride_px, params, nullptr, err, errlen);
    if (st != RT4_OK) return st;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = dout.down(out);
  }
  if (e != hipSuccess) return rt4_set_err(err, errlen, "denoise_host failed: %s", hipGetErrorString(e)), RT4_ERR_HIP;
  return RT4_OK;
}

}  // extern "C"
