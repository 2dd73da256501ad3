// rt4_light_tiles.h — adaptive light sampling of rt4.h (rt4_light_select_tiles_device, rt4_render_light_tiles_device;
// DESIGN.md §4.39): kernels and entry points. From rt4_post.h: the argument checks, the launch bracket, HostStage and
// grow_scratch; from rt4_light.h: light_apply, light_tone, LIGHT_LOAD_BATCH, light_image and render_light /
// render_light_staged (TileList is rt4_trace.hip's). No trace kernel uses anything from here, and none is changed: a
// tile-list launch hands the trace kernel its list through KernelArgs::order, the way the pre-pass hands it the
// longest-first order.
//
// Selection is two kernels: the flags (a wave per 8x8 tile as in rt4_light_noise_kernel, the hot count one ballot) into
// context-owned scratch, then one workgroup that walks the tiles in chunks of its size, dilates the flags, and writes
// the selected tiles behind a running base, so the list comes out ascending whatever order the waves ran in.
#pragma once

namespace {

constexpr unsigned SELECT_MAX_BLOCKS = 512;  // workgroups of the flags kernel (as NOISE_MAX_BLOCKS)
constexpr unsigned SELECT_CHUNK = 1024;      // tiles per step of the compaction: its workgroup, one tile per lane

// rt4.h rt4_light_select_tiles_device, step 1: flags[tile] = 1 iff the tile qualifies (a young pixel, or min_above hot
// ones). q op for op as rt4_light_noise_kernel.
__global__ __launch_bounds__(256) void rt4_light_tile_flags_kernel(const rt4_light_px* __restrict__ light, int64_t light_stride,
                                                                   int32_t w, int32_t h, float k, float threshold,
                                                                   int32_t min_above, int32_t min_frames,
                                                                   uint32_t* __restrict__ flags) {
  const unsigned tiles_x = static_cast<unsigned>((w + 7) / 8), tiles = tiles_x * static_cast<unsigned>((h + 7) / 8);
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  for (unsigned tile = blockIdx.x * 4u + wave; tile < tiles; tile += gridDim.x * 4u) {
    const int x = static_cast<int>((tile % tiles_x) * 8u + (lane & 7u));
    const int y = static_cast<int>((tile / tiles_x) * 8u + (lane >> 3));
    bool hot = false, young = false;
    if (x < w && y < h) {
      const float* st = reinterpret_cast<const float*>(light + static_cast<int64_t>(y) * light_stride + x);
      const float mean_y = st[3], m2 = st[4];
      const int32_t n = __float_as_int(st[5]);
      young = n < min_frames;
      if (n >= 2) {
        const float se = sqrt_((m2 / static_cast<float>(n - 1)) / static_cast<float>(n));
        const float q = __fsub_rn(light_tone(k, __fadd_rn(mean_y, se)), light_tone(k, mean_y));
        hot = q > threshold;
      }
    }
    const int n_hot = __popcll(__ballot(hot));
    const bool any_young = __ballot(young) != 0ull;
    if (lane == 0) flags[tile] = (any_young || n_hot >= min_above) ? 1u : 0u;
  }
}

// Step 2: one workgroup of SELECT_CHUNK lanes. Lane t of a step owns tile base_tile + t: its state is 2 when its own
// flag is set, 1 when a flag within `dilate` tiles of it (inside the grid: no wrap-around) is, else 0. The selected
// tiles of a step go to tiles[base ..) in lane order (a ballot per wave, the waves' counts through LDS), and base
// runs on: ascending, exact. The LDS counts alternate between two rows, so a step needs one barrier.
__global__ __launch_bounds__(SELECT_CHUNK) void rt4_light_tile_compact_kernel(const uint32_t* __restrict__ flags,
                                                                              int32_t tiles_x, int32_t tiles_y, int32_t dilate,
                                                                              uint32_t* __restrict__ tiles_out,
                                                                              uint32_t* __restrict__ count_out,
                                                                              int32_t* __restrict__ state_out) {
  constexpr unsigned WAVES = SELECT_CHUNK / 64u;
  __shared__ unsigned wave_n[2][WAVES];
  const unsigned tiles = static_cast<unsigned>(tiles_x) * static_cast<unsigned>(tiles_y);
  const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  unsigned base = 0, row = 0;  // workgroup-uniform
  for (unsigned t0 = 0; t0 < tiles; t0 += SELECT_CHUNK, row ^= 1u) {
    const unsigned t = t0 + threadIdx.x;
    int state = 0;
    if (t < tiles) {
      const int tx = static_cast<int>(t % static_cast<unsigned>(tiles_x)), ty = static_cast<int>(t / static_cast<unsigned>(tiles_x));
      if (flags[t] != 0u) {
        state = 2;
      } else {
        const int x0 = max(tx - dilate, 0), x1 = min(tx + dilate, tiles_x - 1);
        const int y0 = max(ty - dilate, 0), y1 = min(ty + dilate, tiles_y - 1);
        for (int yy = y0; yy <= y1; yy++)
          for (int xx = x0; xx <= x1; xx++)
            if (flags[static_cast<unsigned>(yy) * static_cast<unsigned>(tiles_x) + static_cast<unsigned>(xx)] != 0u) state = 1;
      }
      if (state_out) state_out[t] = state;
    }
    const unsigned long long sel = __ballot(state != 0);
    if (lane == 0) wave_n[row][wave] = static_cast<unsigned>(__popcll(sel));
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (unsigned q = 0; q < WAVES; q++) {
      const unsigned c = wave_n[row][q];
      before += q < wave ? c : 0u;
      all += c;
    }
    if (state != 0) {
      const unsigned r = __builtin_amdgcn_mbcnt_hi(static_cast<unsigned>(sel >> 32),
                                                   __builtin_amdgcn_mbcnt_lo(static_cast<unsigned>(sel), 0u));
      tiles_out[base + before + r] = t;  // base + before + r < the selected tiles so far <= tiles
    }
    base += all;
  }
  if (threadIdx.x == 0) *count_out = base;
}

// rt4.h rt4_render_light_tiles_device: the caller's list copied into the context's, every entry clamped to `tiles`
// (the tile one row below the image: every pixel of it fails the trace kernel's ii < reg.h test), so no raw entry reaches
// the trace kernel's tile arithmetic.
__global__ __launch_bounds__(256) void rt4_tile_list_clamp_kernel(const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                                                  uint32_t n, uint32_t tiles) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) dst[t] = min(src[t], tiles);
}

// rt4_fold_light_kernel for the listed tiles only: a wave per listed tile, lane -> pixel as the trace kernel's
// claim_batch (lane & 7, lane >> 3). a.order is the context's clamped list, a.frame_tiles its length.
__global__ __launch_bounds__(256) void rt4_fold_light_tiles_kernel(const KernelArgs a, rt4_light_px* __restrict__ light,
                                                                   int64_t light_stride) {
  const JobArgs& J = a.jobs[0];
  const unsigned lane = threadIdx.x & 63u;
  const unsigned item = blockIdx.x * 4u + (threadIdx.x >> 6);
  if (item >= a.frame_tiles) return;
  const unsigned tile = a.order[item];
  const unsigned tiles = J.tiles_x * static_cast<unsigned>((J.reg.h + 7) / 8);
  if (tile >= tiles) return;
  const int jj = static_cast<int>((tile % J.tiles_x) * 8u + (lane & 7u));
  const int ii = static_cast<int>((tile / J.tiles_x) * 8u + (lane >> 3));
  if (jj >= J.reg.w || ii >= J.reg.h) return;
  const int64_t npx = static_cast<int64_t>(J.reg.w) * J.reg.h;
  const int64_t p = static_cast<int64_t>(ii) * J.reg.w + jj;
  float4* st = reinterpret_cast<float4*>(light + static_cast<int64_t>(ii) * light_stride + jj);
  float4 m = st[0];
  const float4 t = st[1];
  float m2 = t.x;
  int32_t n = __float_as_int(t.y);
  const float ns = static_cast<float>(a.samples);
  const float4* src = a.fcolor + J.fc_base + p;
  const int nf = a.n_frames;
  for (int f0 = 0; f0 < nf; f0 += LIGHT_LOAD_BATCH) {  // the batched loads of rt4_fold_light_kernel
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

// launch_jobs with a tile list (rt4_trace.hip): the context's copy of the list holds at least `tiles` entries, followed
// by the two words {0, 1} the trace kernel reads as KernelArgs::order_ends (a non-zero second word switches its order
// on): the last two of the scratch's words. Growing waits as grow_scratch does, once per larger region.
int ensure_tile_list(rt4_context* ctx, unsigned tiles, hipStream_t s, char* err, size_t errlen) {
  CtxScratch& tl = ctx->tile_list;
  const size_t words = static_cast<size_t>(tiles) + 2;
  if (tl.cap >= words) return RT4_OK;
  const int st = grow_scratch(ctx, tl, s, words, sizeof(uint32_t), err, errlen);
  if (st != RT4_OK) return st;
  const uint32_t ends[2] = {0u, 1u};
  const hipError_t e = hipMemcpy(static_cast<uint32_t*>(tl.d) + tiles, ends, sizeof ends, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    tl.cap = 0;  // no list without its end words: the next call grows again
    return rt4_set_err(err, errlen, "tile list upload failed: %s", hipGetErrorString(e)), RT4_ERR_HIP;
  }
  return RT4_OK;
}

// The list part of a tile-list launch, on the trace kernel's stream behind the waits of launch_jobs: the clamped copy,
// then order, order_ends of `a` (frame_tiles and total were set with the frame plan).
int stage_tile_list(rt4_context* ctx, const TileList& tl, unsigned tiles, KernelArgs& a, hipStream_t s, char* err,
                    size_t errlen) {
  const int st = ensure_tile_list(ctx, tiles, s, err, errlen);
  if (st != RT4_OK) return st;
  const uint32_t n = static_cast<uint32_t>(tl.n);
  uint32_t* list = static_cast<uint32_t*>(ctx->tile_list.d);
  (void)hipGetLastError();
  hipLaunchKernelGGL(rt4_tile_list_clamp_kernel, dim3((n + 255u) / 256u), dim3(256), 0, s, tl.d_tiles, list, n, tiles);
  HIP_TRY(hipGetLastError());
  a.order = list;
  a.order_ends = list + ctx->tile_list.cap - 2;
  return RT4_OK;
}

void launch_fold_light_tiles(const KernelArgs& a, const LightTarget& lt, hipStream_t s) {
  hipLaunchKernelGGL(rt4_fold_light_tiles_kernel, dim3((a.frame_tiles + 3u) / 4u), dim3(256), 0, s, a, lt.light,
                     lt.row_stride_px);
}

int select_check_params(const rt4_tile_select_params* p, char* err, size_t errlen) {
  if (p->threshold != p->threshold) return rt4_set_err(err, errlen, "threshold is NaN"), RT4_ERR_ARG;
  if (p->min_above < 1 || p->min_above > 64)
    return rt4_set_err(err, errlen, "min_above %d not in [1, 64]", p->min_above), RT4_ERR_ARG;
  if (p->min_frames < 0) return rt4_set_err(err, errlen, "min_frames %d < 0", p->min_frames), RT4_ERR_ARG;
  if (p->dilate < 0 || p->dilate > RT4_SELECT_MAX_DILATE)
    return rt4_set_err(err, errlen, "dilate %d not in [0, %d]", p->dilate, RT4_SELECT_MAX_DILATE), RT4_ERR_ARG;
  return RT4_OK;
}

}  // namespace

extern "C" {

void rt4_tile_select_params_default(rt4_tile_select_params* p) {
  if (!p) return;
  p->threshold = 1.0f / 255.0f;
  p->min_above = 4;
  p->min_frames = 8;
  p->dilate = 1;
}

uint64_t rt4_context_select_bytes(const rt4_context* ctx) {
  if (!ctx) return 0u;
  return (static_cast<uint64_t>(ctx->select.cap) + static_cast<uint64_t>(ctx->tile_list.cap)) * sizeof(uint32_t);
}

int rt4_light_select_tiles_device(rt4_context* ctx, const rt4_light_px* d_light, int64_t light_stride, int32_t w, int32_t h,
                                  float k, const rt4_tile_select_params* params, uint32_t* d_tiles, uint32_t* d_count,
                                  int32_t* d_tile_state, void* stream, char* err, size_t errlen) {
  if (!ctx || !d_light || !params || !d_tiles || !d_count) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || w > 65535 || h > 65535)
    return rt4_set_err(err, errlen, "image size %d x %d not in [1, 65535]", w, h), RT4_ERR_ARG;
  const int32_t tx = (w + 7) / 8, ty = (h + 7) / 8;
  const PostImage in = light_image(d_light, light_stride, w, h);
  const PostImage outs[3] = {post_image(d_tiles, tx, tx, ty, sizeof(uint32_t), "tile list"),
                             post_image(d_count, 1, 1, 1, sizeof(uint32_t), "count"),
                             post_image(d_tile_state, tx, tx, ty, sizeof(int32_t), "tile state")};
  int st = post_check_args(outs, d_tile_state ? 3 : 2, &in, 1, err, errlen);
  if (st == RT4_OK) st = select_check_params(params, err, errlen);
  if (st != RT4_OK) return st;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const unsigned tiles = static_cast<unsigned>(tx) * static_cast<unsigned>(ty);
  st = grow_scratch(ctx, ctx->select, s, tiles, sizeof(uint32_t), err, errlen);  // more tiles than any call before
  if (st != RT4_OK) return st;
  uint32_t* flags = static_cast<uint32_t*>(ctx->select.d);
  return post_launch(ctx, s, "tile selection", err, errlen, [&] {
    hipLaunchKernelGGL(rt4_light_tile_flags_kernel, dim3(std::min((tiles + 3u) / 4u, SELECT_MAX_BLOCKS)), dim3(256), 0, s,
                       d_light, light_stride, w, h, k, params->threshold, params->min_above, params->min_frames, flags);
    hipError_t le = hipGetLastError();
    if (le == hipSuccess) {
      hipLaunchKernelGGL(rt4_light_tile_compact_kernel, dim3(1), dim3(SELECT_CHUNK), 0, s, flags, tx, ty, params->dilate,
                         d_tiles, d_count, d_tile_state);
      le = hipGetLastError();
    }
    return le;
  });
}

int rt4_light_select_tiles_host(rt4_context* ctx, const rt4_light_px* light, int64_t light_stride, int32_t w, int32_t h,
                                float k, const rt4_tile_select_params* params, uint32_t* tiles, uint32_t* count,
                                int32_t* tile_state, char* err, size_t errlen) {
  if (!ctx || !light || !params || !tiles || !count) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (w <= 0 || h <= 0 || light_stride < w) return rt4_set_err(err, errlen, "bad image size or row stride"), RT4_ERR_ARG;
  HIP_TRY(hipSetDevice(ctx->device));
  HostStage acc, dl, dc, ds;
  const size_t n_tiles = static_cast<size_t>((w + 7) / 8) * static_cast<size_t>((h + 7) / 8);
  hipError_t e = acc.up(light, image_span(light_stride, w, h) * sizeof(rt4_light_px));
  if (e == hipSuccess) e = dl.up(tiles, n_tiles * sizeof(uint32_t));
  if (e == hipSuccess) e = dc.up(count, sizeof(uint32_t));
  if (e == hipSuccess && tile_state) e = ds.up(tile_state, n_tiles * sizeof(int32_t));
  if (e == hipSuccess) {
    const int st = rt4_light_select_tiles_device(ctx, acc.as<const rt4_light_px>(), light_stride, w, h, k, params,
                                                 dl.as<uint32_t>(), dc.as<uint32_t>(), ds.as<int32_t>(), nullptr, err, errlen);
    if (st != RT4_OK) return st;
    e = hipDeviceSynchronize();
    if (e == hipSuccess) e = dl.down(tiles);
    if (e == hipSuccess) e = dc.down(count);
    if (e == hipSuccess && tile_state) e = ds.down(tile_state);
  }
  if (e != hipSuccess) return rt4_set_err(err, errlen, "light_select_tiles_host failed: %s", hipGetErrorString(e)), RT4_ERR_HIP;
  return RT4_OK;
}

int rt4_render_light_tiles_device(rt4_context* ctx, const rt4_uniforms* u, int32_t n_frames, const rt4_region* region,
                                  const uint32_t* d_tiles, int32_t n_tiles, rt4_light_px* d_light, int64_t row_stride_px,
                                  unsigned long long* d_counter, void* stream, char* err, size_t errlen) {
  const TileList tl{d_tiles, n_tiles};
  return render_light(ctx, u, n_frames, region, &tl, d_light, row_stride_px, d_counter, stream, err, errlen);
}

int rt4_render_light_tiles_host(rt4_context* ctx, const rt4_uniforms* u, int32_t n_frames, const rt4_region* region,
                                const uint32_t* tiles, int32_t n_tiles, rt4_light_px* light, int64_t row_stride_px,
                                uint64_t* n_intersections, char* err, size_t errlen) {
  if (!ctx || !u || !region || !light) return rt4_set_err(err, errlen, "NULL argument"), RT4_ERR_ARG;
  if (n_frames < 1) return rt4_set_err(err, errlen, "n_frames %d < 1", n_frames), RT4_ERR_ARG;
  int st = rt4_check_render_args(u, region, row_stride_px, err, errlen);
  if (st != RT4_OK) return st;
  if (n_tiles < 0 || (n_tiles > 0 && !tiles)) return rt4_set_err(err, errlen, "bad tile list"), RT4_ERR_ARG;
  if (n_intersections) *n_intersections = 0;
  if (region->w == 0 || region->h == 0) return n_tiles == 0 ? RT4_OK : (rt4_set_err(err, errlen, "n_tiles %d not 0", n_tiles), RT4_ERR_ARG);
  return render_light_staged(ctx, u, n_frames, region, true, tiles, n_tiles, light, row_stride_px, n_intersections,
                             "render_light_tiles_host", err, errlen);
}

}  // extern "C"
