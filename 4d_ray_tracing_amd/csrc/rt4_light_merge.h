// rt4_light_merge.h — combining light accumulators of rt4.h (rt4_light_merge_device, rt4_light_bands_unpermute_device;
// DESIGN.md §4.41): kernel and entry points. From rt4_post.h: the argument checks, the launch bracket, the pixel grid
// and HostStage; from rt4_light.h: light_image; rt4_unpermute_kernel is rt4_trace.hip's. No trace kernel, fold or other
// pass uses anything from here.
//
// One lane per pixel. The pixel's state is read as two 16-B words, the sources' states are loaded a batch at a time
// ahead of the chain that depends on them (as rt4_fold_light_kernel loads its light sums), applied in order, and the
// state is written once: 32 (K + 2) B per pixel for K sources, memory-bound.
#pragma once

namespace {

constexpr int LIGHT_MERGE_BATCH = 4;  // source states in flight per lane ahead of the chain: 8 16-B loads, 32 VGPRs

// rt4.h rt4_light_merge_device: source state (bm: mean rgb + mean_y, bm2, bn) merged into the state (m, m2, n).
// N < 2^32 - 1 for n, bn >= 0, so the unsigned sum is the definition's int64 sum and converts as it does.
__device__ __forceinline__ void light_merge_apply(float4& m, float& m2, int32_t& n, float4 bm, float bm2, int32_t bn) {
  if (bn == 0) return;
  if (n == 0) {
    m = bm;
    m2 = bm2;
    n = bn;
    return;
  }
  const uint32_t N = static_cast<uint32_t>(n) + static_cast<uint32_t>(bn);
  const float fb = static_cast<float>(bn) / static_cast<float>(N);
  const float wa = __fmul_rn(static_cast<float>(n), fb);
  m.x = __builtin_fmaf(__fsub_rn(bm.x, m.x), fb, m.x);
  m.y = __builtin_fmaf(__fsub_rn(bm.y, m.y), fb, m.y);
  m.z = __builtin_fmaf(__fsub_rn(bm.z, m.z), fb, m.z);
  const float dy = __fsub_rn(bm.w, m.w);
  m.w = __builtin_fmaf(dy, fb, m.w);
  m2 = __builtin_fmaf(__fmul_rn(dy, dy), wa, __fadd_rn(m2, bm2));
  n = N > static_cast<uint32_t>(INT32_MAX) ? INT32_MAX : static_cast<int32_t>(N);
}

// rt4.h rt4_light_merge_device: dst = merge(... merge(merge(dst, src_0), src_1) ..., src_{n_srcs - 1}) per pixel.
__global__ __launch_bounds__(256) void rt4_light_merge_kernel(rt4_light_px* __restrict__ dst, int64_t dst_stride,
                                                              const rt4_light_px* __restrict__ srcs, int64_t src_stride,
                                                              int64_t src_plane_stride, int32_t n_srcs, int32_t w,
                                                              int32_t h) {
  const int2 xy = px_xy();
  const int x = xy.x, y = xy.y;
  if (x >= w || y >= h) return;
  float4* st = reinterpret_cast<float4*>(dst + static_cast<int64_t>(y) * dst_stride + x);
  const float4* src = reinterpret_cast<const float4*>(srcs + static_cast<int64_t>(y) * src_stride + x);
  const int64_t plane = src_plane_stride * 2;  // in 16-B words
  float4 m = st[0];
  const float4 t = st[1];
  float m2 = t.x;
  int32_t n = __float_as_int(t.y);
  // The sources do not depend on the chain: a batch of them is loaded (the last batch re-reads the last source
  // instead of branching), then applied in order.
  for (int s0 = 0; s0 < n_srcs; s0 += LIGHT_MERGE_BATCH) {
    float4 bm[LIGHT_MERGE_BATCH], bt[LIGHT_MERGE_BATCH];
#pragma unroll
    for (int q = 0; q < LIGHT_MERGE_BATCH; q++) {
      const int s = s0 + q < n_srcs ? s0 + q : n_srcs - 1;
      const float4* p = src + static_cast<int64_t>(s) * plane;
      bm[q] = p[0];
      bt[q] = p[1];
    }
#pragma unroll
    for (int q = 0; q < LIGHT_MERGE_BATCH; q++)
      if (s0 + q < n_srcs) light_merge_apply(m, m2, n, bm[q], bt[q].x, __float_as_int(bt[q].y));
  }
  st[0] = m;
  st[1] = make_float4(m2, __int_as_float(n), 0.0f, 0.0f);
}

// The checks of rt4_light_merge_device / _host: sizes and the plane stride here, every image's stride, alignment
// (`align`: 16 for device pointers, 1 for host pointers, which are only staged) and the overlaps in post_check_args.
int light_merge_check(const rt4_light_px* dst, int64_t dst_stride, const rt4_light_px* srcs, int64_t src_stride,
                      int64_t src_plane_stride, int32_t n_srcs, int32_t w, int32_t h, size_t align, char* err,
                      size_t errlen) {
  if (n_srcs < 1 || n_srcs > RT4_LIGHT_MERGE_MAX)
    return rt4_set_err(err, errlen, "n_srcs %d not in [1, %d]", n_srcs, RT4_LIGHT_MERGE_MAX), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || w > 65535 || h > 65535)
    return rt4_set_err(err, errlen, "image size %d x %d not in [1, 65535]", w, h), RT4_ERR_ARG;
  PostImage out = light_image(dst, dst_stride, w, h);
  out.align = align;
  PostImage in[RT4_LIGHT_MERGE_MAX];
  for (int32_t s = 0; s < n_srcs; s++) {
    in[s] = post_image(srcs + static_cast<int64_t>(s) * src_plane_stride, src_stride, w, h, sizeof(rt4_light_px),
                       "light source");
    in[s].align = align;
  }
  if (src_stride >= w && src_plane_stride < static_cast<int64_t>(h - 1) * src_stride + w)
    return rt4_set_err(err, errlen, "light source: plane stride smaller than one image"), RT4_ERR_ARG;
  return post_check_args(&out, 1, in, static_cast<size_t>(n_srcs), err, errlen);
}

}  // namespace

extern "C" {

int rt4_light_merge_device(rt4_context* ctx, rt4_light_px* d_dst, int64_t dst_stride, const rt4_light_px* d_srcs,
                           int64_t src_stride, int64_t src_plane_stride, int32_t n_srcs, int32_t w, int32_t h, void* stream,
                           char* err, size_t errlen) {
  if (!ctx || !d_dst || !d_srcs) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const int st = light_merge_check(d_dst, dst_stride, d_srcs, src_stride, src_plane_stride, n_srcs, w, h, 16u, err, errlen);
  if (st != RT4_OK) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return post_launch(ctx, s, "light merge kernel", err, errlen, [&] {
    hipLaunchKernelGGL(rt4_light_merge_kernel, px_grid(w, h), dim3(256), 0, s, d_dst, dst_stride, d_srcs, src_stride,
                       src_plane_stride, n_srcs, w, h);
    return hipGetLastError();
  });
}

int rt4_light_merge_host(rt4_context* ctx, rt4_light_px* dst, int64_t dst_stride, const rt4_light_px* srcs,
                         int64_t src_stride, int64_t src_plane_stride, int32_t n_srcs, int32_t w, int32_t h, char* err,
                         size_t errlen) {
  if (!ctx || !dst || !srcs) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const int ck = light_merge_check(dst, dst_stride, srcs, src_stride, src_plane_stride, n_srcs, w, h, 1u, err, errlen);
  if (ck != RT4_OK) return ck;
  HIP_TRY(hipSetDevice(ctx->device));
  HostStage acc, in;
  hipError_t e = acc.up(dst, image_span(dst_stride, w, h) * sizeof(rt4_light_px));
  if (e == hipSuccess)
    e = in.up(srcs, (static_cast<size_t>(n_srcs - 1) * static_cast<size_t>(src_plane_stride) + image_span(src_stride, w, h)) *
                        sizeof(rt4_light_px));
  if (e == hipSuccess) {
    const int st = rt4_light_merge_device(ctx, acc.as<rt4_light_px>(), dst_stride, in.as<const rt4_light_px>(), src_stride,
                                          src_plane_stride, n_srcs, w, h, nullptr, err, errlen);
    if (st != RT4_OK) return st;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = acc.down(dst);
  }
  if (e != hipSuccess) return rt4_set_err(err, errlen, "light_merge_host failed: %s", hipGetErrorString(e)), RT4_ERR_HIP;
  return RT4_OK;
}

int rt4_light_bands_unpermute_device(const rt4_light_px* d_gathered, rt4_light_px* d_image, int32_t width, int32_t height,
                                     int32_t world, int32_t band, int32_t rows_max, void* stream, char* err, size_t errlen) {
  if (!d_gathered || !d_image) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (width < 1 || height < 1 || world < 1 || band < 1 || rows_max < 1)
    return rt4_set_err(err, errlen, "unpermute: width, height, world, band and rows_max must be >= 1"), RT4_ERR_ARG;
  // every image row's source must lie inside the gather: the plan's rows_max (rt4_band_plan) or more
  const int64_t need = rt4_band_rows_max(height, world, band);
  if (static_cast<int64_t>(rows_max) < need)
    return rt4_set_err(err, errlen, "unpermute: rows_max %d below the plan's %lld", rows_max, static_cast<long long>(need)),
           RT4_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(d_gathered) % 16u != 0 || reinterpret_cast<uintptr_t>(d_image) % 16u != 0)
    return rt4_set_err(err, errlen, "unpermute: light accumulator not 16-byte aligned"), RT4_ERR_ARG;
  const int64_t words = static_cast<int64_t>(width) * static_cast<int64_t>(sizeof(rt4_light_px) / 16u);
  if (words > INT32_MAX) return rt4_set_err(err, errlen, "unpermute: width %d too large", width), RT4_ERR_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(rt4_unpermute_kernel<uint4>, dim3(static_cast<unsigned>(height)), dim3(256), 0, s,
                     reinterpret_cast<const uint4*>(d_gathered), reinterpret_cast<uint4*>(d_image), static_cast<int32_t>(words),
                     world, band, rows_max);
  HIP_TRY(hipGetLastError());
  return RT4_OK;
}

}  // extern "C"
