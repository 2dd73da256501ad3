// rt4_light_downsample.h — supersampled light accumulators of rt4.h (rt4_light_downsample_device):
// kernel and entry points. From rt4_post.h: the argument checks, the launch bracket, the pixel grid and HostStage; from
// rt4_light.h: light_image. No trace kernel, fold or other pass uses anything from here.
//
// One lane per output pixel. The pixel's s x s strata are read as 16-B words, a batch of them loaded ahead of the add
// chains that depend on them (as rt4_light_merge_kernel loads its sources) and added in the definition's order (b outer,
// a inner); the lane keeps four sums, the sum of the strata's se^2 and the smallest n, and writes its state once:
// 32 (s^2 + 1) B per output pixel, memory-bound. A lane's sub-row is 32 s contiguous bytes and a wave's 32 lanes cover
// 1024 s contiguous bytes of it, so every cache line fetched is used whole by the 2 s loads of the sub-row.
#pragma once

namespace {

constexpr int LIGHT_DOWN_BATCH = 4;  // strata in flight per lane ahead of the chains: 8 16-B loads, 32 VGPRs
constexpr int LIGHT_DOWN_UNROLL_S = 2;  // the largest s whose sub-row loop is unrolled

// rt4.h rt4_light_downsample_device for one output pixel; fine points at its stratum (0, 0), stride in 16-B words.
template <int S>
__global__ __launch_bounds__(256) void rt4_light_downsample_kernel(const rt4_light_px* __restrict__ fine,
                                                                   int64_t fine_stride, rt4_light_px* __restrict__ out,
                                                                   int64_t out_stride, int32_t w, int32_t h) {
  const int2 xy = px_xy();
  const int x = xy.x, y = xy.y;
  if (x >= w || y >= h) return;
  const float4* src = reinterpret_cast<const float4*>(fine + static_cast<int64_t>(y) * S * fine_stride +
                                                      static_cast<int64_t>(x) * S);
  const int64_t row = fine_stride * 2;  // in 16-B words
  float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  float sv = 0.0f;
  int32_t nmin = INT32_MAX;
  // Up to s = 2 the sub-rows unroll into one block; beyond that a sub-row per trip (its strata still unrolled), so that
  // the loads in flight stay a few batches and every s keeps 8 waves/SIMD: unrolled whole, s = 8 held 130 VGPRs, and
  // the register allocator of the iterative-ilp stress build (csrc/Makefile) crashed on the s = 3 body.
#pragma unroll S <= LIGHT_DOWN_UNROLL_S ? S : 1
  for (int b = 0; b < S; b++) {
    const float4* p = src + static_cast<int64_t>(b) * row;
#pragma unroll
    for (int a0 = 0; a0 < S; a0 += LIGHT_DOWN_BATCH) {
      constexpr int B = LIGHT_DOWN_BATCH;
      float4 fm[B], ft[B];
#pragma unroll
      for (int q = 0; q < B; q++)
        if (a0 + q < S) {
          fm[q] = p[2 * (a0 + q)];
          ft[q] = p[2 * (a0 + q) + 1];
        }
#pragma unroll
      for (int q = 0; q < B; q++)
        if (a0 + q < S) {
          const int32_t n = __float_as_int(ft[q].y);
          sum.x = __fadd_rn(sum.x, fm[q].x);
          sum.y = __fadd_rn(sum.y, fm[q].y);
          sum.z = __fadd_rn(sum.z, fm[q].z);
          sum.w = __fadd_rn(sum.w, fm[q].w);
          // the radicand of se in rt4_light_noise_kernel; only read when every stratum has n >= 2
          const int32_t n1 = static_cast<int32_t>(static_cast<uint32_t>(n) - 1u);
          sv = __fadd_rn(sv, (ft[q].x / static_cast<float>(n1)) / static_cast<float>(n));
          nmin = n < nmin ? n : nmin;
        }
    }
  }
  float4* st = reinterpret_cast<float4*>(out + static_cast<int64_t>(y) * out_stride + x);
  if (nmin <= 0) {  // a stratum nobody sampled: the empty accumulator
    st[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    st[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  constexpr float inv = 1.0f / static_cast<float>(S * S);
  float m2 = 0.0f;
  if (nmin >= 2) {
    const float var = __fmul_rn(__fmul_rn(sv, inv), inv);
    m2 = __fmul_rn(__fmul_rn(var, static_cast<float>(nmin)), static_cast<float>(nmin - 1));
  }
  st[0] = make_float4(__fmul_rn(sum.x, inv), __fmul_rn(sum.y, inv), __fmul_rn(sum.z, inv), __fmul_rn(sum.w, inv));
  st[1] = make_float4(m2, __int_as_float(nmin), 0.0f, 0.0f);
}

// The checks of rt4_light_downsample_device / _host: s and the sizes here, the strides, the alignment (`align`: 16 for
// device pointers, 1 for host pointers, which are only staged) and the overlap in post_check_args.
int light_downsample_check(const rt4_light_px* fine, int64_t fine_stride, const rt4_light_px* out, int64_t out_stride,
                           int32_t w, int32_t h, int32_t s, size_t align, char* err, size_t errlen) {
  if (s < 1 || s > RT4_SUPERSAMPLE_MAX)
    return rt4_set_err(err, errlen, "s %d not in [1, %d]", s, RT4_SUPERSAMPLE_MAX), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || w > 65535 / s || h > 65535 / s)
    return rt4_set_err(err, errlen, "image size %d x %d at s %d: w, h, w*s and h*s not in [1, 65535]", w, h, s), RT4_ERR_ARG;
  PostImage o = light_image(out, out_stride, w, h);
  o.align = align;
  PostImage in = post_image(fine, fine_stride, w * s, h * s, sizeof(rt4_light_px), "fine light accumulator");
  in.align = align;
  return post_check_args(&o, 1, &in, 1, err, errlen);
}

template <int S>
hipError_t light_downsample_launch(hipStream_t st, const rt4_light_px* fine, int64_t fine_stride, rt4_light_px* out,
                                   int64_t out_stride, int32_t w, int32_t h) {
  hipLaunchKernelGGL(rt4_light_downsample_kernel<S>, px_grid(w, h), dim3(256), 0, st, fine, fine_stride, out, out_stride, w, h);
  return hipGetLastError();
}

}  // namespace

extern "C" {

int rt4_light_downsample_device(rt4_context* ctx, const rt4_light_px* d_fine, int64_t fine_stride, rt4_light_px* d_out,
                                int64_t out_stride, int32_t w, int32_t h, int32_t s, void* stream, char* err,
                                size_t errlen) {
  if (!ctx || !d_fine || !d_out) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const int ck = light_downsample_check(d_fine, fine_stride, d_out, out_stride, w, h, s, 16u, err, errlen);
  if (ck != RT4_OK) return ck;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return post_launch(ctx, st, "light downsample kernel", err, errlen, [&] {
    switch (s) {  // s = 1 .. RT4_SUPERSAMPLE_MAX (checked): one instantiation each, so the loop over a sub-row's strata unrolls
      case 1: return light_downsample_launch<1>(st, d_fine, fine_stride, d_out, out_stride, w, h);
      case 2: return light_downsample_launch<2>(st, d_fine, fine_stride, d_out, out_stride, w, h);
      case 3: return light_downsample_launch<3>(st, d_fine, fine_stride, d_out, out_stride, w, h);
      case 4: return light_downsample_launch<4>(st, d_fine, fine_stride, d_out, out_stride, w, h);
      case 5: return light_downsample_launch<5>(st, d_fine, fine_stride, d_out, out_stride, w, h);
      case 6: return light_downsample_launch<6>(st, d_fine, fine_stride, d_out, out_stride, w, h);
      case 7: return light_downsample_launch<7>(st, d_fine, fine_stride, d_out, out_stride, w, h);
      default: return light_downsample_launch<8>(st, d_fine, fine_stride, d_out, out_stride, w, h);
    }
  });
}

int rt4_light_downsample_host(rt4_context* ctx, const rt4_light_px* fine, int64_t fine_stride, rt4_light_px* out,
                              int64_t out_stride, int32_t w, int32_t h, int32_t s, char* err, size_t errlen) {
  if (!ctx || !fine || !out) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const int ck = light_downsample_check(fine, fine_stride, out, out_stride, w, h, s, 1u, err, errlen);
  if (ck != RT4_OK) return ck;
  HIP_TRY(hipSetDevice(ctx->device));
  HostStage in, acc;
  hipError_t e = in.up(fine, image_span(fine_stride, w * s, h * s) * sizeof(rt4_light_px));
  if (e == hipSuccess) e = acc.up(out, image_span(out_stride, w, h) * sizeof(rt4_light_px));
  if (e == hipSuccess) {
    const int st = rt4_light_downsample_device(ctx, in.as<const rt4_light_px>(), fine_stride, acc.as<rt4_light_px>(),
                                               out_stride, w, h, s, nullptr, err, errlen);
    if (st != RT4_OK) return st;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = acc.down(out);
  }
  if (e != hipSuccess)
    return rt4_set_err(err, errlen, "light_downsample_host failed: %s", hipGetErrorString(e)), RT4_ERR_HIP;
  return RT4_OK;
}

}  // extern "C"
