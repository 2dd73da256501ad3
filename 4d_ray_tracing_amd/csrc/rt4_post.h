// rt4_post.h — what the render path and every post pass of rt4.h share and none owns: the
// argument checks of strided device images, the launch bracket that orders a pass with the context's launches, the 32x8
// pixel grid, the stores and decodes of the frame formats, the staging of the _host variants and the context's growing
// scratch buffers. Part of rt4_trace.hip's translation unit, included directly behind the context and HIP_TRY, ahead of
// the render entry points and the pass headers (rt4_denoise.h ... rt4_retina.h): it needs the context, HIP_TRY and
// the blend_* store helpers from there and nothing from the launch path or any pass.
#pragma once

namespace {

// ---- strided images --------------------------------------------------------------------------------------------------
// Elements of a strided w x h image: the last row ends at its w-th pixel.
size_t image_span(int64_t stride_px, int32_t w, int32_t h) {
  return static_cast<size_t>(h - 1) * static_cast<size_t>(stride_px) + static_cast<size_t>(w);
}

struct PostImage {  // one strided image of a pass's argument list
  const void* p;
  int64_t stride;  // row stride in elements
  int32_t w, h;
  size_t elem, align;  // bytes of an element; alignment of the base
  const char* name;    // for messages
};
// An image whose base is aligned as its element is loaded: as a whole up to 16 B, as 16-B words beyond.
PostImage post_image(const void* p, int64_t stride, int32_t w, int32_t h, size_t elem, const char* name) {
  return PostImage{p, stride, w, h, elem, elem < 16u ? elem : 16u, name};
}
size_t post_bytes(const PostImage& m) { return image_span(m.stride, m.w, m.h) * m.elem; }

int post_check_image(const PostImage& m, char* err, size_t errlen) {
  if (m.stride < m.w) return rt4_set_err(err, errlen, "%s: row stride smaller than width", m.name), RT4_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(m.p) % m.align != 0)
    return rt4_set_err(err, errlen, "%s not aligned to %zu bytes", m.name, m.align), RT4_ERR_ARG;
  return RT4_OK;
}

// No output may share a byte with an input or with another output: the half-open ranges [p, p + bytes), so images
// that only touch are accepted.
bool post_overlap(const PostImage& a, const PostImage& b) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
  return a0 < b0 + post_bytes(b) && b0 < a0 + post_bytes(a);
}
int post_check_overlap(const PostImage* out, size_t n_out, const PostImage* in, size_t n_in, char* err, size_t errlen) {
  for (size_t o = 0; o < n_out; o++) {
    for (size_t i = 0; i < n_in; i++)
      if (post_overlap(out[o], in[i]))
        return rt4_set_err(err, errlen, "%s overlaps %s", out[o].name, in[i].name), RT4_ERR_ARG;
    for (size_t b = o + 1; b < n_out; b++)
      if (post_overlap(out[o], out[b]))
        return rt4_set_err(err, errlen, "%s overlaps %s", out[o].name, out[b].name), RT4_ERR_ARG;
  }
  return RT4_OK;
}
// The argument list of a pass: every image's stride and alignment, then the overlaps. An absent optional image is
// simply not in the lists.
int post_check_args(const PostImage* out, size_t n_out, const PostImage* in, size_t n_in, char* err, size_t errlen) {
  for (size_t i = 0; i < n_in; i++)
    if (post_check_image(in[i], err, errlen) != RT4_OK) return RT4_ERR_ARG;
  for (size_t o = 0; o < n_out; o++)
    if (post_check_image(out[o], err, errlen) != RT4_OK) return RT4_ERR_ARG;
  return post_check_overlap(out, n_out, in, n_in, err, errlen);
}

// ---- launch bracket --------------------------------------------------------------------------------------------------
// A launch of the context on stream s that is not a render: ordered behind the context's previous launch when that ran
// on another stream. done_launch() afterwards: rt4_context_set_scene and the next launch on another stream wait for it.
int order_launch(rt4_context* ctx, hipStream_t s, char* err, size_t errlen) {
  if (ctx->launched && s != ctx->last_stream) HIP_TRY(hipStreamWaitEvent(s, ctx->done, 0));
  return RT4_OK;
}
int done_launch(rt4_context* ctx, hipStream_t s, char* err, size_t errlen) {
  const hipError_t re = hipEventRecord(ctx->done, s);
  ctx->last_stream = s;
  ctx->launched = true;
  if (re != hipSuccess) {
    rt4_set_err(err, errlen, "hipEventRecord failed: %s", hipGetErrorString(re));
    return RT4_ERR_HIP;
  }
  return RT4_OK;
}

// The launches of one pass between the two: `launches` puts kernels (and memsets) on s and returns the first error,
// hipGetLastError() after a kernel. A sticky error of an earlier, unrelated call is cleared first, so that it is not
// taken for this pass's.
template <class F>
int post_launch(rt4_context* ctx, hipStream_t s, const char* what, char* err, size_t errlen, F&& launches) {
  int rc = order_launch(ctx, s, err, errlen);
  if (rc != RT4_OK) return rc;
  (void)hipGetLastError();
  const hipError_t le = launches();
  rc = done_launch(ctx, s, err, errlen);
  if (le != hipSuccess) {
    rt4_set_err(err, errlen, "%s launch failed: %s", what, hipGetErrorString(le));
    return RT4_ERR_HIP;
  }
  return rc;
}

// ---- pixel grid ------------------------------------------------------------------------------------------------------
constexpr int PX_BX = 32, PX_BY = 8;  // pixels per workgroup of 256 (one lane each)

dim3 px_grid(int32_t w, int32_t h) {
  return dim3(static_cast<unsigned>((w + PX_BX - 1) / PX_BX), static_cast<unsigned>((h + PX_BY - 1) / PX_BY));
}
__device__ __forceinline__ int2 px_xy() {
  return make_int2(static_cast<int>(blockIdx.x) * PX_BX + static_cast<int>(threadIdx.x & 31u),
                   static_cast<int>(blockIdx.y) * PX_BY + static_cast<int>(threadIdx.x >> 5));
}

// ---- frame formats ---------------------------------------------------------------------------------------------------
// Colour c with alpha 1 through the store rule of the format: blend_*(c, 1, 0) is c * 1 + 0 * 0, then the format's
// rounding.
__device__ __forceinline__ void px_store_opaque(void* frame, int32_t format, int64_t at, V3 c) {
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

// A stored pixel as fp32.
__device__ __forceinline__ float4 px_decode(const void* frame, int32_t format, int64_t at) {
  if (format == RT4_FRAME_RGBA16F) {
    const h4v v = reinterpret_cast<const h4v*>(frame)[at];
    return make_float4(static_cast<float>(v[0]), static_cast<float>(v[1]), static_cast<float>(v[2]), static_cast<float>(v[3]));
  }
  if (format == RT4_FRAME_RGBA8) {
    const uint32_t v = reinterpret_cast<const uint32_t*>(frame)[at];
    return make_float4(static_cast<float>(v & 0xFFu) / 255.0f, static_cast<float>((v >> 8) & 0xFFu) / 255.0f,
                       static_cast<float>((v >> 16) & 0xFFu) / 255.0f, static_cast<float>(v >> 24) / 255.0f);
  }
  return reinterpret_cast<const float4*>(frame)[at];
}

// ---- host staging ----------------------------------------------------------------------------------------------------
// Host staging of the _host variants: a device copy of a strided host image (the padding of an output keeps its bytes
// on the way back because it made the way there). Freed on every way out.
struct HostStage {
  void* d = nullptr;
  size_t bytes = 0;
  hipError_t up(const void* host, size_t n) {
    bytes = n;
    hipError_t e = hipMalloc(&d, n);
    if (e == hipSuccess && host) e = hipMemcpy(d, host, n, hipMemcpyHostToDevice);
    return e;
  }
  hipError_t down(void* host) const { return hipMemcpy(host, d, bytes, hipMemcpyDeviceToHost); }
  template <class T>
  T* as() const { return static_cast<T*>(d); }
  ~HostStage() {
    if (d) (void)hipFree(d);
  }
};

hipError_t alloc_zeroed(void** p, size_t bytes) {
  const hipError_t e = hipMalloc(p, bytes);
  return e == hipSuccess ? hipMemset(*p, 0, bytes) : e;
}

// ---- context scratch -------------------------------------------------------------------------------------------------
// sc holds at least `units` units of unit_bytes afterwards. Growing waits for the stream and for the context's launches
// in flight (they may still use the old buffer), once per larger need; a failed allocation leaves {nullptr, 0}.
int grow_scratch(rt4_context* ctx, CtxScratch& sc, hipStream_t s, size_t units, size_t unit_bytes, char* err,
                 size_t errlen) {
  if (sc.cap >= units) return RT4_OK;
  HIP_TRY(hipStreamSynchronize(s));
  if (ctx->launched) HIP_TRY(hipEventSynchronize(ctx->done));
  if (sc.d) (void)hipFree(sc.d);
  sc.d = nullptr;
  sc.cap = 0;
  HIP_TRY(hipMalloc(&sc.d, units * unit_bytes));
  sc.cap = units;
  return RT4_OK;
}

}  // namespace
