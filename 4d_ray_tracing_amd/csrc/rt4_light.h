// rt4_light.h — light-domain accumulation of rt4.h (rt4_render_light_device, rt4_light_resolve_device,
// rt4_light_noise_device): kernels and entry points. From rt4_post.h: the argument checks, the launch
// bracket, the pixel grid, px_store_opaque and HostStage; from no other pass (KernelArgs, launch_jobs and TileList are
// rt4_trace.hip's). rt4_light_denoise.h and rt4_light_tiles.h take light_tone, light_apply, LIGHT_LOAD_BATCH and
// render_light / render_light_staged from here, rt4_light_merge.h light_image. No trace kernel uses anything from here.
//
// The trace kernels already hand every frame's raw light sum to the frame-colour scratch (KernelArgs::fcolor); the
// colour accumulators tone-map it in rt4_fold_frames_kernel. The light accumulator is a second fold over the same
// scratch: one lane per pixel, the pixel's 32-B state read as two 16-B words, the launch's frames applied in order,
// the state written once. Resolve is one lane per pixel; noise takes a wave per 8x8 tile, so the tile's count is
// one ballot, and the statistics are integer atomics of one lane per workgroup (exact in any order).
#pragma once

namespace {

constexpr int LIGHT_LOAD_BATCH = 8;  // light sums in flight per lane ahead of the recurrence

// rt4.h rt4_light_px: one frame's light sum folded into the state (m: mean rgb + mean_y, m2, n).
__device__ __forceinline__ void light_apply(float4& m, float& m2, int32_t& n, float4 l, float ns) {
  const float xr = l.x / ns, xg = l.y / ns, xb = l.z / ns;  // the division of tone_map
  const float y = __builtin_fmaf(0.2126f, xr, __builtin_fmaf(0.7152f, xg, __fmul_rn(0.0722f, xb)));
  n = n == INT32_MAX ? n : n + 1;
  const float inv = 1.0f / static_cast<float>(n);
  m.x = __builtin_fmaf(__fsub_rn(xr, m.x), inv, m.x);
  m.y = __builtin_fmaf(__fsub_rn(xg, m.y), inv, m.y);
  m.z = __builtin_fmaf(__fsub_rn(xb, m.z), inv, m.z);
  const float dy = __fsub_rn(y, m.w);
  m.w = __builtin_fmaf(dy, inv, m.w);
  m2 = __builtin_fmaf(dy, __fsub_rn(y, m.w), m2);
}

// The frames of a launch folded in order into the light accumulator (rt4_render_light_device): the grid of
// rt4_fold_frames_kernel, in whose place it runs. count_src: as there (an overlapped launch's count, moved into the
// caller's counter and reset); light launches do not overlap today, so it is null.
__global__ __launch_bounds__(256) void rt4_fold_light_kernel(const KernelArgs a, rt4_light_px* __restrict__ light,
                                                             int64_t light_stride, unsigned long long* count_src,
                                                             unsigned long long* count_dst) {
  const JobArgs& J = a.jobs[0];
  const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (count_src && p == 0) {
    if (count_dst) atomicAdd(count_dst, *count_src);
    *count_src = 0ull;
  }
  const int64_t npx = static_cast<int64_t>(J.reg.w) * J.reg.h;
  if (p >= npx) return;
  const int i = static_cast<int>(p / J.reg.w), j = static_cast<int>(p - static_cast<int64_t>(i) * J.reg.w);
  float4* st = reinterpret_cast<float4*>(light + static_cast<int64_t>(i) * light_stride + j);
  float4 m = st[0];
  const float4 t = st[1];
  float m2 = t.x;
  int32_t n = __float_as_int(t.y);
  const float ns = static_cast<float>(a.samples);
  const float4* src = a.fcolor + J.fc_base + p;
  const int nf = a.n_frames;
  // The light sums do not depend on the recurrence: a batch of them is loaded (the last batch re-reads the launch's
  // last frame instead of branching), then applied in order. 16 * n_frames + 64 B per pixel: memory-bound.
  for (int f0 = 0; f0 < nf; f0 += LIGHT_LOAD_BATCH) {
    float4 l[LIGHT_LOAD_BATCH];
#pragma unroll
    for (int q = 0; q < LIGHT_LOAD_BATCH; q++) {
      const int f = f0 + q < nf ? f0 + q : nf - 1;
      l[q] = src[static_cast<int64_t>(f) * npx];
    }
#pragma unroll
    for (int q = 0; q < LIGHT_LOAD_BATCH; q++)
      if (f0 + q < nf) light_apply(m, m2, n, l[q], ns);
  }
  st[0] = m;
  st[1] = make_float4(m2, __int_as_float(n), 0.0f, 0.0f);
}

// rt4.h: the tone curve of tone_map on a mean (the same ops).
__device__ __forceinline__ float light_tone(float k, float v) { return 1.0f - 1.0f / sfma_(k, v, 1.0f); }

// rt4.h rt4_light_resolve_device.
__global__ __launch_bounds__(256) void rt4_light_resolve_kernel(const rt4_light_px* __restrict__ light, int64_t light_stride,
                                                                float k, void* __restrict__ frame, int32_t format,
                                                                int64_t frame_stride, int32_t w, int32_t h) {
  const int2 xy = px_xy();
  const int x = xy.x, y = xy.y;
  if (x >= w || y >= h) return;
  const float4* st = reinterpret_cast<const float4*>(light + static_cast<int64_t>(y) * light_stride + x);
  const float4 m = st[0];
  const int32_t n = __float_as_int(st[1].y);
  const V3 c = n == 0 ? V3{0.0f, 0.0f, 0.0f} : V3{light_tone(k, m.x), light_tone(k, m.y), light_tone(k, m.z)};
  px_store_opaque(frame, format, static_cast<int64_t>(y) * frame_stride + x, c);
}

constexpr unsigned NOISE_MAX_BLOCKS = 512;   // workgroups of the noise kernel: each sends one set of atomics

// rt4.h rt4_light_noise_device: a wave takes one 8x8 tile at a time (four waves per workgroup, the workgroups stride
// over the tiles), so a tile's count is one ballot. The statistics are kept per wave across its tiles, joined per
// workgroup in LDS, and one lane per workgroup sends the integer atomics: one set per tile, all on one 32-B line,
// measured 5.1 ms at 1080p (32400 tiles), this 0.05 ms. stats->pixels is the host's.
__global__ __launch_bounds__(256) void rt4_light_noise_kernel(const rt4_light_px* __restrict__ light, int64_t light_stride,
                                                              int32_t w, int32_t h, float k, float threshold,
                                                              float* __restrict__ se_map, float* __restrict__ q_map,
                                                              int64_t map_stride, int32_t* __restrict__ tile_above,
                                                              rt4_noise_stats* stats) {
  __shared__ unsigned wave_meas[4], wave_above[4], wave_q[4], wave_se[4];
  const unsigned tiles_x = static_cast<unsigned>((w + 7) / 8), tiles = tiles_x * static_cast<unsigned>((h + 7) / 8);
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  unsigned sum_meas = 0, sum_above = 0;  // wave-uniform
  float vq = 0.0f, vse = 0.0f;  // the lane's maxima over its pixels: a value counts if measured and > 0 (so not NaN)
  for (unsigned tile = blockIdx.x * 4u + wave; tile < tiles; tile += gridDim.x * 4u) {
    const int x = static_cast<int>((tile % tiles_x) * 8u + (lane & 7u));
    const int y = static_cast<int>((tile / tiles_x) * 8u + (lane >> 3));
    bool measured = false, above = false;
    if (x < w && y < h) {
      const float* st = reinterpret_cast<const float*>(light + static_cast<int64_t>(y) * light_stride + x);
      const float mean_y = st[3], m2 = st[4];
      const int32_t n = __float_as_int(st[5]);
      float se = __builtin_inff(), q = __builtin_inff();
      if (n >= 2) {
        measured = true;
        se = sqrt_((m2 / static_cast<float>(n - 1)) / static_cast<float>(n));
        q = __fsub_rn(light_tone(k, __fadd_rn(mean_y, se)), light_tone(k, mean_y));
        above = q > threshold;
        vq = q > vq ? q : vq;
        vse = se > vse ? se : vse;
      }
      const int64_t at = static_cast<int64_t>(y) * map_stride + x;
      if (se_map) se_map[at] = se;
      if (q_map) q_map[at] = q;
    }
    const unsigned n_above = static_cast<unsigned>(__popcll(__ballot(above)));
    sum_above += n_above;
    sum_meas += static_cast<unsigned>(__popcll(__ballot(measured)));
    if (tile_above && lane == 0) tile_above[tile] = static_cast<int32_t>(n_above);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {  // non-negative, no NaN: any order gives the same maximum
    vq = fmaxf(vq, __shfl_xor(vq, d, 64));
    vse = fmaxf(vse, __shfl_xor(vse, d, 64));
  }
  if (lane == 0) {
    wave_meas[wave] = sum_meas;
    wave_above[wave] = sum_above;
    wave_q[wave] = __float_as_uint(vq);  // the bit patterns of non-negative floats are ordered like the floats
    wave_se[wave] = __float_as_uint(vse);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long n_meas = 0, n_above = 0;
    unsigned bq = 0, bs = 0;
    for (int q = 0; q < 4; q++) {
      n_meas += wave_meas[q];
      n_above += wave_above[q];
      bq = wave_q[q] > bq ? wave_q[q] : bq;
      bs = wave_se[q] > bs ? wave_se[q] : bs;
    }
    // integer atomics: exact in any order. A zero operand changes nothing and is not sent.
    if (n_meas) atomicAdd(reinterpret_cast<unsigned long long*>(&stats->measured), n_meas);
    if (n_above) atomicAdd(reinterpret_cast<unsigned long long*>(&stats->above), n_above);
    if (bq) atomicMax(reinterpret_cast<unsigned*>(&stats->max_q), bq);
    if (bs) atomicMax(reinterpret_cast<unsigned*>(&stats->max_se), bs);
  }
}

PostImage light_image(const rt4_light_px* p, int64_t stride, int32_t w, int32_t h) {
  return post_image(p, stride, w, h, sizeof(rt4_light_px), "light accumulator");
}

// rt4_render_light_device, and with a tile list rt4_render_light_tiles_device (rt4_light_tiles.h): the checks, then the
// frames in launches of rt4_context_frames_per_launch.
int render_light(rt4_context* ctx, const rt4_uniforms* u, int32_t n_frames, const rt4_region* region, const TileList* tl,
                 rt4_light_px* d_light, int64_t row_stride_px, unsigned long long* d_counter, void* stream, char* err,
                 size_t errlen) {
  if (!ctx || !u || !region || !d_light) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (n_frames < 1) return rt4_set_err(err, errlen, "n_frames %d < 1", n_frames), RT4_ERR_ARG;
  if (region->w > 8191 || region->h > 8191)
    return rt4_set_err(err, errlen, "light accumulation: region %d x %d larger than 8191 x 8191", region->w, region->h),
           RT4_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(d_light) % 16u != 0)
    return rt4_set_err(err, errlen, "light accumulator not 16-byte aligned"), RT4_ERR_ARG;
  for (int32_t f = 1; f < n_frames; f++) {  // only seed and part may change from frame to frame
    rt4_uniforms x = u[f];
    x.seed = u[0].seed;
    x.part = u[0].part;
    if (std::memcmp(&x, &u[0], sizeof x) != 0)
      return rt4_set_err(err, errlen, "frame %d: uniforms other than seed/part differ from frame 0", f), RT4_ERR_ARG;
  }
  if (tl) {  // an empty list returns below without a launch: what launch_jobs would refuse is refused here first
    const int st = rt4_check_render_args(u, region, row_stride_px, err, errlen);
    if (st != RT4_OK) return st;
    if (!ctx->has_scene) return rt4_set_err(err, errlen, "context has no scene (rt4_context_set_scene)"), RT4_ERR_ARG;
    const int64_t tiles = static_cast<int64_t>((region->w + 7) / 8) * ((region->h + 7) / 8);
    if (tl->n < 0 || tl->n > tiles)
      return rt4_set_err(err, errlen, "n_tiles %d not in [0, %lld]", tl->n, static_cast<long long>(tiles)), RT4_ERR_ARG;
    if (tl->n > 0 && (!tl->d_tiles || reinterpret_cast<uintptr_t>(tl->d_tiles) % 4u != 0))
      return rt4_set_err(err, errlen, "tile list NULL or not 4-byte aligned"), RT4_ERR_ARG;
    if (tl->n == 0) return RT4_OK;
  }
  rt4_section_job job;
  job.region = *region;
  job.d_frame = d_light;  // launch_jobs wants a frame; the fold takes the accumulator as an argument of its own
  job.row_stride_px = row_stride_px;
  const LightTarget lt{d_light, row_stride_px, tl};
  const int32_t chunk = rt4_context_frames_per_launch(ctx, region->w, region->h);
  int32_t seeds[RT4_MAX_FRAMES];
  float parts[RT4_MAX_FRAMES];
  for (int32_t f0 = 0; f0 < n_frames; f0 += chunk) {
    const int32_t n = std::min(chunk, n_frames - f0);
    job.u = u[f0];  // a launch of one frame reads its seed here
    job.u.part = 1.0f;
    for (int32_t f = 0; f < n; f++) {
      seeds[f] = u[f0 + f].seed;
      parts[f] = 1.0f;
    }
    const FramePlan fp{n, seeds, parts, &lt};
    const int st = launch_jobs(ctx, &job, 1, RT4_FRAME_RGBA32F, d_counter, stream, err, errlen, &fp);
    if (st != RT4_OK) return st;
  }
  return RT4_OK;
}

// The staging of rt4_render_light_host and rt4_render_light_tiles_host behind their own argument checks: the
// accumulator both ways, a zeroed counter, and the tile list when there is one (`listed`; it may be empty).
int render_light_staged(rt4_context* ctx, const rt4_uniforms* u, int32_t n_frames, const rt4_region* region, bool listed,
                        const uint32_t* tiles, int32_t n_tiles, rt4_light_px* light, int64_t row_stride_px,
                        uint64_t* n_intersections, const char* what, char* err, size_t errlen) {
  HIP_TRY(hipSetDevice(ctx->device));
  HostStage acc, cnt, lst;
  hipError_t e = acc.up(light, image_span(row_stride_px, region->w, region->h) * sizeof(rt4_light_px));
  if (e == hipSuccess) e = cnt.up(nullptr, sizeof(unsigned long long));
  if (e == hipSuccess) e = hipMemset(cnt.d, 0, sizeof(unsigned long long));
  if (e == hipSuccess && listed && n_tiles > 0) e = lst.up(tiles, static_cast<size_t>(n_tiles) * sizeof(uint32_t));
  if (e == hipSuccess) {
    const TileList tl{lst.as<const uint32_t>(), n_tiles};
    const int st = render_light(ctx, u, n_frames, region, listed ? &tl : nullptr, acc.as<rt4_light_px>(), row_stride_px,
                                cnt.as<unsigned long long>(), nullptr, err, errlen);
    if (st != RT4_OK) return st;
    e = hipDeviceSynchronize();
    unsigned long long c = 0;
    if (e == hipSuccess) e = acc.down(light);
    if (e == hipSuccess) e = hipMemcpy(&c, cnt.d, sizeof c, hipMemcpyDeviceToHost);
    if (e == hipSuccess && n_intersections) *n_intersections = c;
  }
  if (e != hipSuccess) return rt4_set_err(err, errlen, "%s failed: %s", what, hipGetErrorString(e)), RT4_ERR_HIP;
  return RT4_OK;
}

}  // namespace

extern "C" {

int rt4_render_light_device(rt4_context* ctx, const rt4_uniforms* u, int32_t n_frames, const rt4_region* region,
                            rt4_light_px* d_light, int64_t row_stride_px, unsigned long long* d_counter, void* stream,
                            char* err, size_t errlen) {
  return render_light(ctx, u, n_frames, region, nullptr, d_light, row_stride_px, d_counter, stream, err, errlen);
}

int rt4_render_light_host(rt4_context* ctx, const rt4_uniforms* u, int32_t n_frames, const rt4_region* region,
                          rt4_light_px* light, int64_t row_stride_px, uint64_t* n_intersections, char* err, size_t errlen) {
  if (!ctx || !u || !region || !light) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (n_frames < 1) return rt4_set_err(err, errlen, "n_frames %d < 1", n_frames), RT4_ERR_ARG;
  const int st = rt4_check_render_args(u, region, row_stride_px, err, errlen);
  if (st != RT4_OK) return st;
  if (n_intersections) *n_intersections = 0;
  if (region->w == 0 || region->h == 0) return RT4_OK;
  return render_light_staged(ctx, u, n_frames, region, false, nullptr, 0, light, row_stride_px, n_intersections,
                             "render_light_host", err, errlen);
}

int rt4_light_resolve_device(rt4_context* ctx, const rt4_light_px* d_light, int64_t light_stride, float k, void* d_frame,
                             int32_t format, int64_t frame_stride, int32_t w, int32_t h, void* stream, char* err,
                             size_t errlen) {
  if (!ctx || !d_light || !d_frame) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const int32_t px_bytes = rt4_frame_format_bytes(format);
  if (px_bytes == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || w > 65535 || h > 65535)
    return rt4_set_err(err, errlen, "image size %d x %d not in [1, 65535]", w, h), RT4_ERR_ARG;
  const PostImage in = light_image(d_light, light_stride, w, h);
  const PostImage out = post_image(d_frame, frame_stride, w, h, static_cast<size_t>(px_bytes), "frame");
  const int st = post_check_args(&out, 1, &in, 1, err, errlen);
  if (st != RT4_OK) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return post_launch(ctx, s, "light resolve kernel", err, errlen, [&] {
    hipLaunchKernelGGL(rt4_light_resolve_kernel, px_grid(w, h), dim3(256), 0, s, d_light, light_stride, k, d_frame, format,
                       frame_stride, w, h);
    return hipGetLastError();
  });
}

int rt4_light_resolve_host(rt4_context* ctx, const rt4_light_px* light, int64_t light_stride, float k, void* frame,
                           int32_t format, int64_t frame_stride, int32_t w, int32_t h, char* err, size_t errlen) {
  if (!ctx || !light || !frame) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  const int32_t px_bytes = rt4_frame_format_bytes(format);
  if (px_bytes == 0) return rt4_set_err(err, errlen, "unknown frame format %d", format), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || light_stride < w || frame_stride < w)
    return rt4_set_err(err, errlen, "bad image size or row stride"), RT4_ERR_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  HostStage acc, out;
  hipError_t e = acc.up(light, image_span(light_stride, w, h) * sizeof(rt4_light_px));
  if (e == hipSuccess) e = out.up(frame, image_span(frame_stride, w, h) * static_cast<size_t>(px_bytes));
  if (e == hipSuccess) {
    const int st = rt4_light_resolve_device(ctx, acc.as<const rt4_light_px>(), light_stride, k, out.d, format, frame_stride, w,
                                            h, nullptr, err, errlen);
    if (st != RT4_OK) return st;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = out.down(frame);
  }
  if (e != hipSuccess) return rt4_set_err(err, errlen, "light_resolve_host failed: %s", hipGetErrorString(e)), RT4_ERR_HIP;
  return RT4_OK;
}

int rt4_light_noise_device(rt4_context* ctx, const rt4_light_px* d_light, int64_t light_stride, int32_t w, int32_t h,
                           float k, float threshold, float* d_se, float* d_q, int64_t map_stride, int32_t* d_tile_above,
                           rt4_noise_stats* d_stats, void* stream, char* err, size_t errlen) {
  if (!ctx || !d_light || !d_stats) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || w > 65535 || h > 65535)
    return rt4_set_err(err, errlen, "image size %d x %d not in [1, 65535]", w, h), RT4_ERR_ARG;
  const int32_t tx = (w + 7) / 8, ty = (h + 7) / 8;
  const PostImage in = light_image(d_light, light_stride, w, h);
  PostImage outs[4];
  size_t n_out = 0;
  outs[n_out++] = PostImage{d_stats, 1, 1, 1, sizeof(rt4_noise_stats), 8u, "statistics"};
  if (d_se) outs[n_out++] = post_image(d_se, map_stride, w, h, sizeof(float), "se map");
  if (d_q) outs[n_out++] = post_image(d_q, map_stride, w, h, sizeof(float), "q map");
  if (d_tile_above) outs[n_out++] = post_image(d_tile_above, tx, tx, ty, sizeof(int32_t), "tile image");
  const int st = post_check_args(outs, n_out, &in, 1, err, errlen);
  if (st != RT4_OK) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  return post_launch(ctx, s, "light noise", err, errlen, [&] {
    // the statistics start from zero on every call; pixels (< 2^32) is the host's: its low word, after the zeroes
    hipError_t le = hipMemsetAsync(d_stats, 0, sizeof(rt4_noise_stats), s);
    if (le == hipSuccess)
      le = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(&d_stats->pixels),
                             static_cast<int>(static_cast<uint32_t>(w) * static_cast<uint32_t>(h)), 1, s);
    if (le == hipSuccess) {
      const unsigned tiles = static_cast<unsigned>(tx) * static_cast<unsigned>(ty);
      hipLaunchKernelGGL(rt4_light_noise_kernel, dim3(std::min((tiles + 3u) / 4u, NOISE_MAX_BLOCKS)), dim3(256), 0, s, d_light,
                         light_stride, w, h, k, threshold, d_se, d_q, map_stride, d_tile_above, d_stats);
      le = hipGetLastError();
    }
    return le;
  });
}

int rt4_light_noise_host(rt4_context* ctx, const rt4_light_px* light, int64_t light_stride, int32_t w, int32_t h, float k,
                         float threshold, float* se, float* q, int64_t map_stride, int32_t* tile_above,
                         rt4_noise_stats* stats, char* err, size_t errlen) {
  if (!ctx || !light || !stats) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || light_stride < w || ((se || q) && map_stride < w))
    return rt4_set_err(err, errlen, "bad image size or row stride"), RT4_ERR_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  HostStage acc, dse, dq, dt, ds;
  const size_t map_bytes = (se || q) ? image_span(map_stride, w, h) * sizeof(float) : 0;
  const size_t tile_bytes = static_cast<size_t>((w + 7) / 8) * static_cast<size_t>((h + 7) / 8) * sizeof(int32_t);
  hipError_t e = acc.up(light, image_span(light_stride, w, h) * sizeof(rt4_light_px));
  if (e == hipSuccess && se) e = dse.up(se, map_bytes);
  if (e == hipSuccess && q) e = dq.up(q, map_bytes);
  if (e == hipSuccess && tile_above) e = dt.up(tile_above, tile_bytes);
  if (e == hipSuccess) e = ds.up(stats, sizeof(rt4_noise_stats));
  if (e == hipSuccess) {
    const int st = rt4_light_noise_device(ctx, acc.as<const rt4_light_px>(), light_stride, w, h, k, threshold, dse.as<float>(),
                                          dq.as<float>(), map_stride, dt.as<int32_t>(), ds.as<rt4_noise_stats>(), nullptr,
                                          err, errlen);
    if (st != RT4_OK) return st;
    e = hipDeviceSynchronize();
    if (e == hipSuccess && se) e = dse.down(se);
    if (e == hipSuccess && q) e = dq.down(q);
    if (e == hipSuccess && tile_above) e = dt.down(tile_above);
    if (e == hipSuccess) e = ds.down(stats);
  }
  if (e != hipSuccess) return rt4_set_err(err, errlen, "light_noise_host failed: %s", hipGetErrorString(e)), RT4_ERR_HIP;
  return RT4_OK;
}

}  // extern "C"
