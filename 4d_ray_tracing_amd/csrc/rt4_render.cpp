// rt4_render — the reference's frame loop (src/main.cpp:57-111) offscreen, as a C++ host program over
// the C ABI of librt4.so: properties.txt + a scene .frag in, progressive frames of one section or of
// the three ThreeWindowGroup sections rendered on one GPU, PPM images out. What it replaces:
//   Properties props("properties.txt")            -> rt4_properties_load
//   initShader / initControls                     -> rt4_uniforms_from_properties / rt4_camera_init
//   shader.loadFromFile(shader_filename)          -> rt4_scene_load_frag (snippet or whole shader.frag)
//   seed ^= generateSeed(timer); part = 1/frame    -> seed ^ n*0x9E3779B9 (deterministic), camera uniforms
//   windowGroup->drawShaderImage()                -> rt4_render_sections_device (one launch, 1 or 3 images)
//   windowGroup->display()                        -> rt4_write_ppm after the last frame
//   one GL draw of the whole texture (windows.cpp:45) -> with --gpus N: the frame's pixel bands over N GPUs,
//                                                    one host thread per device, each rank's frames in one
//                                                    rt4_render_frames_device call, one RCCL ncclGather of the
//                                                    padded shards to GPU 0 over xGMI, rt4_bands_unpermute_device
// Usage: rt4_render [-p properties.txt] [-s scene(.frag|builtin name)] [-n frames] [-3] [-W width -H height]
//                   [-f f32|f16|rgba8] [--seed S] [-o prefix] [-d device] [--keys WASD...] [--move-seconds t]
//                   [--frame-by-frame]  (one section and a resting camera: rt4_render_frames_device unless given)
//                   [--gpus N [--band B] [--rehearse]]  (one section, resting camera: bands over devices 0..N-1 +
//                   RCCL gather; --rehearse: N ranks on device 0, the gather as device copies, for one-GPU tests)
//                   [--png]  (PNG images instead of PPM)
//                   [--raw]  (also the frame's bytes as stored, <prefix>_<section>.raw: bit-exact comparisons)
//                   [--resume ckpt] [--checkpoint ckpt]  (one section: continue / save the progressive
//                   accumulator, rt4_accum_load / rt4_accum_save; the reference has no counterpart)
//                   [--denoise [levels]]  (next to every image also <name>_dn.<ext>: the final frame through the
//                   edge-stopping filter, rt4_render_gbuffer_device of the last camera pose + rt4_denoise_device; the
//                   accumulator itself is never filtered. One GPU only: not with --gpus)
//                   [--reproject]  (temporal reprojection: one rt4_temporal per section takes every frame, so the
//                   accumulated image survives --keys / --move-seconds instead of restarting; the images written are
//                   the temporal images, --denoise filters them with the temporal G-buffer. A resting camera gives the
//                   image of a run without the flag. Not with --gpus, --resume, --checkpoint, --frame-by-frame)
//                   [--window [SCALE]] [--window-nearest]  (next to every image also <name>_win.<ext>: the image at
//                   window resolution, what the reference's renderWindow.draw(sprite) shows: cells * SCALE pixels,
//                   SCALE = the window's cell_size from the properties unless given (main for YXZ, additional for the
//                   other two). Interpolated along the primary hits of the window's pixels (one rt4_window per section,
//                   rt4_window_present_device); --window-nearest: the reference's block stretch. With --denoise the
//                   filtered frame is upscaled, with --reproject the temporal image with the temporal G-buffer.
//                   One GPU only: not with --gpus)
//                   [--light [--noise-threshold Q] [--noise-map]]  (light-domain accumulation, a resting camera: the -n
//                   frames of every section go through rt4_render_light_device into a light accumulator and the image
//                   written is its resolve, rt4_light_resolve_device; the rt4_noise_stats of every section are printed
//                   at the end, for the threshold Q in display units (default 1/255, one 8-bit step); --noise-map: also
//                   <prefix>_<section>_q.<ext>, the display error q as grey. An error estimate, not a stop rule: on
//                   scenes lit by small emitters `above` rises over the first hundred frames. --denoise and --window
//                   work on the resolved image; with --raw also <prefix>_<section>_light.raw, the accumulator's bytes. Not
//                   with --reproject, --frame-by-frame, nor with --resume, --checkpoint, --gpus: those are the colour
//                   path's and its file format's; the light path has the three flags below)
//                   [--light-checkpoint F] [--light-resume F]  (need --light, one section: save the light accumulator,
//                   rt4_light_save, with the last frame number issued, the seed and the run's key / continue one with
//                   frame frames_issued + 1, -n more frames: the bytes of an unbroken run. A resume refuses another
//                   --seed, scene, properties, camera or size, a pooled file, and --adaptive, whose pass state the file
//                   does not hold; --adaptive with --light-checkpoint is fine)
//                   [--light-gpus N [--light-split frames|bands] [--band B] [--rehearse]]  (needs --light, one section, not
//                   with --adaptive or --light-resume, N <= 16. frames, the default: rt4_frame_split, rank r renders the
//                   whole image for its block of the frame numbers, one gather, one rt4_light_merge_device of the N
//                   accumulators into the root's empty one; every rank's launch is as large as the one-GPU launch, so it
//                   scales at window sizes where bands cannot fill a GPU, and the result is as accurate as the one-GPU
//                   accumulator but not bit-equal. bands: the bands of --gpus, rt4_light_bands_unpermute_device: bit-equal.
//                   Resolve, statistics, --noise-map, --light-denoise, --denoise and --window run on the root's
//                   accumulator; --rehearse and the RT4_RENDER_FAIL_* hooks as with --gpus)
//                   [--light-pool A B [C ...]]  (renders nothing: loads light checkpoints of runs that differ only in
//                   --seed, refuses another key or size and a seed twice, merges them in order, rt4_light_merge_host, and
//                   writes the resolve, the statistics and, with --light-checkpoint, a pooled file, which cannot be resumed)
//                   [--light-denoise [levels]]  (needs --light: next to every image also <name>_ldn.<ext>, the light
//                   accumulator through the variance-guided filter, rt4_render_gbuffer_device of the section's pose +
//                   rt4_light_denoise_device, tone-mapped once at the end; with --window the filtered frame is the one
//                   upscaled. Not with --denoise, which filters the resolved colours)
//                   [--adaptive [--adaptive-warmup W] [--adaptive-pass F] [--adaptive-full-every M]
//                    [--adaptive-min-above A] [--adaptive-dilate D]]  (needs --light: -n N becomes a budget of N
//                   whole-frame equivalents, N x tiles tile-frames per section. W whole frames first, then passes of F
//                   frames of the 8x8 tiles rt4_light_select_tiles_device picks for --noise-threshold (A hot pixels,
//                   grown by D tiles), rendered by rt4_render_light_tiles_device; every M-th pass, and a pass with an
//                   empty selection, is a whole-frame pass; the loop never stops early. One line per pass, the min /
//                   median / max of n at the end, and <prefix>_<section>_n.<ext>: n over the largest n as grey.
//                   Defaults 8, 4, 4, 4, 1: the values of the study in DESIGN.md §4.39)
//                   [--supersample S]  (needs --light, S 1..8: anti-aliased pixels, DESIGN.md §4.48. -W/-H, or the
//                   properties' cells, name the output; the accumulation (the -n frames, --adaptive, --light-resume)
//                   runs at S times that, the view of rt4_upscale_uniforms, whose pixel centres are an S x S grid
//                   inside every output pixel, and one rt4_light_downsample_device per section follows. The resolve, the
//                   statistics, --noise-map, --light-denoise, --denoise, --window, the images and the _n picture see the
//                   output-resolution accumulator; --light-checkpoint saves the fine one, which --light-resume with the same S
//                   continues. -n keeps meaning frames at the render resolution: S^2 times fewer frames cast the same
//                   rays. Not with --light-gpus, --light-pool or --retina; S times the output at most 8191 per side)
//                   [--retina D [--retina-size X] [--retina-view YAW PITCH] [--retina-turntable N] [--retina-step S]]
//                   (the 3D retina view, DESIGN.md §4.47: the -n frames go into a D-slice light volume of the section's
//                   view, the slices spread over X scene units along the camera's w axis (default: the matrix height),
//                   rt4_retina_accumulate_device; the volume is projected, rt4_retina_present_device, to
//                   <prefix>_yxz_retina.<ext> at the window's pixel size (cells * the main window's cell_size), seen
//                   from YAW PITCH degrees (default 30 20), S voxels per sample (default 1). --retina-turntable N: instead
//                   N pictures <prefix>_yxz_retina_000 .. at yaw 360 k / N, all from the one accumulated volume. One
//                   section, one GPU, a resting camera; --light is implied. Not with -3, --gpus, --light-gpus,
//                   --reproject, --adaptive, --denoise, --light-denoise, --window, --frame-by-frame, nor any checkpoint flag)
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/rt4.h"

namespace {

[[noreturn]] void die(const char* what, const char* err) {
  std::fprintf(stderr, "rt4_render: %s: %s\n", what, err);
  std::exit(1);
}

#define RT4_CHECK(call)                       \
  do {                                        \
    if ((call) != RT4_OK) die(#call, err);    \
  } while (0)
#define HIP_CHECK(call)                                                 \
  do {                                                                  \
    hipError_t e_ = (call);                                             \
    if (e_ != hipSuccess) die(#call, hipGetErrorString(e_));            \
  } while (0)

// A reusable barrier for the device threads (C++17 has no std::barrier).
class Barrier {
 public:
  explicit Barrier(int n) : n_(n) {}
  void wait() {
    std::unique_lock<std::mutex> lk(mu_);
    const long gen = gen_;
    if (++count_ == n_) {
      count_ = 0;
      ++gen_;
      cv_.notify_all();
    } else {
      cv_.wait(lk, [&] { return gen_ != gen; });
    }
  }

 private:
  std::mutex mu_;
  std::condition_variable cv_;
  int n_, count_ = 0;
  long gen_ = 0;
};

struct BandRun {  // one GPU's share of a --gpus run
  std::string error;
  unsigned long long count = 0;
  double ms = 0.0;  // this rank's wall time from the start barrier to its gather (and, on rank 0, the un-permute)
};

// Every rank's verdict on one step, agreed before anything collective runs: each rank posts its own
// result, waits at the barrier and reads them all (the barrier's mutex orders the posts before the reads).
// A rank that failed never leaves the others waiting in a collective, and no collective sees a null or
// partly set-up buffer: when any rank failed, every rank skips the gather and the un-permute.
class Agreement {
 public:
  Agreement(int n, Barrier& bar) : ok_(static_cast<size_t>(n), 1), bar_(bar) {}
  bool all(int rank, bool ok) {
    ok_[static_cast<size_t>(rank)] = ok ? 1 : 0;
    bar_.wait();
    bool all_ok = true;
    for (char v : ok_) all_ok = all_ok && v;
    bar_.wait();  // everyone has read before the next step posts again
    return all_ok;
  }

 private:
  std::vector<char> ok_;
  Barrier& bar_;
};

// What a multi-GPU run is made of besides the machinery of render_shards: the size of every rank's shard and of
// the root's image, the rank's own set-up, its render call and the root's last step. Three runs fill it in:
// --gpus (colour frames in pixel bands), --light-gpus --light-split bands (a light accumulator in the same bands)
// and --light-gpus --light-split frames (whole-image light accumulators of disjoint frame blocks, merged).
struct ShardJob {
  const char* flag;                  // "--gpus" / "--light-gpus": names the run in error messages
  size_t shard_bytes, image_bytes;   // every rank's shard (equal sizes: one gather); the root's result
  // rank r's set-up on its context, after its allocations (false: err holds the reason)
  std::function<bool(int r, rt4_context* ctx, char* err, size_t errlen)> setup;
  // rank r's renders into its zeroed shard, enqueued on stream (an RT4 status)
  std::function<int(int r, rt4_context* ctx, void* shard, unsigned long long* d_count, hipStream_t stream, char* err,
                    size_t errlen)> render;
  // the root's last step: the gathered shards (rank-major) into the zeroed image (an RT4 status)
  std::function<int(rt4_context* ctx, const void* gathered, void* image, hipStream_t stream, char* err, size_t errlen)> finish;
};

// The test switches of a multi-GPU run, read once (shard_hooks): --rehearse, RT4_RENDER_FAIL_RANK (this rank's set-up
// fails) and RT4_RENDER_FAIL_STAGE=gather (its part of the gather fails instead); what they do: render_shards.
struct ShardHooks {
  bool rehearse;
  int fail_rank;
  bool fail_gather;
};

ShardHooks shard_hooks(bool rehearse) {
  const char* fail_env = std::getenv("RT4_RENDER_FAIL_RANK");
  const char* stage_env = std::getenv("RT4_RENDER_FAIL_STAGE");
  return {rehearse, fail_env ? std::atoi(fail_env) : -1, stage_env && std::strcmp(stage_env, "gather") == 0};
}

struct ShardResult {
  std::vector<unsigned char> image;  // the root's result on the host
  unsigned long long count;          // intersections of all ranks
  double ms;                         // the slowest rank's time
};

// One section on `gpus` devices: every rank renders its shard (job.render), one ncclGather of the
// shards to rank 0, and the root's last step there (job.finish). For --gpus that is: pixel bands dealt round-robin
// (rt4_band_plan), each rank's frames pipelined in one rt4_render_frames_device call into a padded
// shard of rows_max rows, and rt4_bands_unpermute_device on the root.
// The image equals a one-GPU render bit for bit (every pixel is independent: shader.frag:104-108).
//
// rehearse (--rehearse, a test switch for boxes with one GPU): every rank is a host thread with its own
// context, stream and buffers on device 0, and each rank copies its shard into its slot of rank 0's
// gathered buffer with hipMemcpyAsync where the real run calls ncclGather; the plan, the barrier,
// the agreements and the last step are the real ones. fail_rank >= 0 (the RT4_RENDER_FAIL_RANK test hook)
// makes that rank's set-up fail after its allocations, or with fail_gather (RT4_RENDER_FAIL_STAGE=gather) its
// gather: the rank does not enqueue its part of the collective and reports an error, as when ncclGather fails.
// After the gather is enqueued the ranks agree once more: if any rank failed, every rank aborts its communicator
// (ncclCommAbort), so no rank waits forever in a collective its peer never joined. While the gather runs, every
// rank also watches its communicator's asynchronous error (ncclCommGetAsyncError) and a shared abort flag.
// Returns the root's result on the host (rank 0's), or exits with status 1 naming the failed rank(s).
// rank_main below is, word for word, the function it was before this program was cut into steps:
// its branch without --rehearse needs two GPUs to run, so only the way it receives rehearse, fail_rank and
// fail_gather changed.
ShardResult render_shards(int gpus, const rt4_scene_desc* scene, const ShardJob& job, const ShardHooks& hooks) {
  const bool rehearse = hooks.rehearse, fail_gather = hooks.fail_gather;
  const int fail_rank = hooks.fail_rank;
  std::vector<ncclComm_t> comms(static_cast<size_t>(gpus), nullptr);
  if (!rehearse) {
    std::vector<int> devs(static_cast<size_t>(gpus));
    for (int r = 0; r < gpus; r++) devs[static_cast<size_t>(r)] = r;
    if (ncclCommInitAll(comms.data(), gpus, devs.data()) != ncclSuccess) die("ncclCommInitAll", "failed");
  }
  std::vector<BandRun> runs(static_cast<size_t>(gpus));
  std::vector<unsigned char> image(job.image_bytes);
  const size_t shard_bytes = job.shard_bytes;
  Barrier bar(gpus);
  Agreement agree(gpus, bar);
  void* root_gathered = nullptr;  // rank 0's gathered buffer (rehearse: the other ranks copy into it)
  std::atomic<bool> abort_all{false};  // a rank saw its communicator fail: every rank aborts its own
  auto rank_main = [&](int r) {
    BandRun& run = runs[static_cast<size_t>(r)];
    char err[1024] = {0};
    rt4_context* ctx = nullptr;
    void *shard = nullptr, *gathered = nullptr, *img = nullptr;
    unsigned long long* d_count = nullptr;
    hipStream_t stream = nullptr;
    const int dev = rehearse ? 0 : r;
    auto fail = [&](const char* what) {
      if (run.error.empty()) run.error = what;
      return false;
    };
    bool ok = (hipSetDevice(dev) == hipSuccess && hipStreamCreateWithFlags(&stream, hipStreamNonBlocking) == hipSuccess) ||
              fail("hipSetDevice / hipStreamCreate");
    if (ok && (rt4_context_create(dev, RT4_FLAG_SAMPLER_LUT, &ctx, err, sizeof err) != RT4_OK ||
               rt4_context_set_scene(ctx, scene, err, sizeof err) != RT4_OK))
      ok = fail(err);
    if (ok) {
      ok = (hipMalloc(&shard, shard_bytes) == hipSuccess && hipMemset(shard, 0, shard_bytes) == hipSuccess &&
            hipMalloc(&d_count, sizeof *d_count) == hipSuccess && hipMemset(d_count, 0, sizeof *d_count) == hipSuccess) ||
           fail("device allocation");
      if (ok && r == 0)
        ok = (hipMalloc(&gathered, shard_bytes * gpus) == hipSuccess && hipMalloc(&img, image.size()) == hipSuccess &&
              hipMemset(img, 0, image.size()) == hipSuccess) ||
             fail("device allocation");
    }
    if (ok && !job.setup(r, ctx, err, sizeof err)) ok = fail(err);
    if (ok && r == fail_rank && !fail_gather) ok = fail("set-up failure injected (RT4_RENDER_FAIL_RANK)");
    if (ok) ok = hipDeviceSynchronize() == hipSuccess || fail("hipDeviceSynchronize");
    if (r == 0) root_gathered = gathered;  // read by the other ranks only after the agreement's barrier
    // every rank set up (the agreement is also the start barrier): otherwise nobody renders or gathers
    const bool all_set = agree.all(r, ok);
    const auto t0 = std::chrono::steady_clock::now();
    if (all_set && job.render(r, ctx, shard, d_count, stream, err, sizeof err) != RT4_OK) ok = fail(err);
    // the renders were enqueued everywhere: only then the collective (a launch error skips it on every rank)
    const bool all_rendered = all_set && agree.all(r, ok);
    bool all_gathered = false;
    if (all_rendered) {
      ncclComm_t comm = rehearse ? nullptr : comms[static_cast<size_t>(r)];
      if (r == fail_rank && fail_gather) {
        ok = fail(rehearse ? "rehearsal gather copy failure injected (RT4_RENDER_FAIL_STAGE=gather)"
                           : "ncclGather failure injected (RT4_RENDER_FAIL_STAGE=gather)");
      } else if (rehearse) {
        ok = (hipMemcpyAsync(static_cast<char*>(root_gathered) + static_cast<size_t>(r) * shard_bytes, shard, shard_bytes,
                             hipMemcpyDeviceToDevice, stream) == hipSuccess &&
              hipStreamSynchronize(stream) == hipSuccess) ||
             fail("rehearsal gather copy");
      } else if (ncclGather(shard, gathered, shard_bytes, ncclUint8, 0, comm, stream) != ncclSuccess) {
        ok = fail("ncclGather failed");
      }
      // every rank enqueued its part (rehearse: every shard is in rank 0's buffer): otherwise the ranks that did
      // wait for a peer that never joins, so every rank aborts its communicator instead of synchronising
      all_gathered = agree.all(r, ok);
      if (!all_gathered) {
        abort_all = true;
      } else if (!rehearse) {
        // the gather runs: watch the communicator (an asynchronous error on any rank aborts them all)
        hipError_t q;
        while ((q = hipStreamQuery(stream)) == hipErrorNotReady && !abort_all) {
          ncclResult_t ae = ncclSuccess;
          if (ncclCommGetAsyncError(comm, &ae) != ncclSuccess || ae != ncclSuccess) {
            ok = fail("RCCL asynchronous error in ncclGather");
            abort_all = true;
          }
          std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
        if (q != hipSuccess && q != hipErrorNotReady) ok = fail("hipStreamQuery after ncclGather");
      }
      if (abort_all && comm) {
        (void)ncclCommAbort(comm);  // returns the pending collective; the communicator is gone
        comms[static_cast<size_t>(r)] = nullptr;
        if (ok) ok = fail("communicator aborted: another rank failed in the gather");
      }
      if (ok && !abort_all && r == 0 && job.finish(ctx, gathered, img, stream, err, sizeof err) != RT4_OK) ok = fail(err);
    }
    if (stream && hipStreamSynchronize(stream) != hipSuccess && !abort_all) ok = fail("hipStreamSynchronize");
    run.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if ((!all_rendered || !all_gathered) && ok) fail("skipped: another rank failed");
    if (ok && hipMemcpy(&run.count, d_count, sizeof run.count, hipMemcpyDeviceToHost) != hipSuccess) fail("count");
    if (ok && r == 0 && hipMemcpy(image.data(), img, image.size(), hipMemcpyDeviceToHost) != hipSuccess)
      fail("image copy");
    if (shard) (void)hipFree(shard);
    if (gathered) (void)hipFree(gathered);
    if (img) (void)hipFree(img);
    if (d_count) (void)hipFree(d_count);
    if (stream) (void)hipStreamDestroy(stream);
    rt4_context_destroy(ctx);
  };
  std::vector<std::thread> threads;
  for (int r = 0; r < gpus; r++) threads.emplace_back(rank_main, r);
  for (auto& t : threads) t.join();
  for (auto& c : comms)
    if (c) (void)ncclCommDestroy(c);
  unsigned long long count = 0;
  double ms = 0.0;
  std::string errors;
  for (int r = 0; r < gpus; r++) {
    const BandRun& run = runs[static_cast<size_t>(r)];
    if (!run.error.empty()) errors += (errors.empty() ? "rank " : "; rank ") + std::to_string(r) + ": " + run.error;
    count += run.count;
    ms = std::max(ms, run.ms);  // the job's time: the slowest rank
  }
  if (!errors.empty()) die(job.flag, errors.c_str());
  return {std::move(image), count, ms};
}

// The band plan of every rank (rt4_band_plan), shared by the two band-split jobs below.
struct BandPlans {
  std::vector<rt4_region> reg;
  int32_t rows_max = 0;
  BandPlans(int gpus, int band, int32_t w, int32_t h, const char* flag) : reg(static_cast<size_t>(gpus)) {
    char err[1024] = {0};
    for (int r = 0; r < gpus; r++)
      if (rt4_band_plan(w, h, gpus, band, r, &reg[static_cast<size_t>(r)], &rows_max, err, sizeof err) != RT4_OK) die(flag, err);
  }
};

// --gpus: the colour frames of one section in pixel bands.
ShardResult render_bands(int gpus, int band, const rt4_scene_desc* scene, const std::vector<rt4_uniforms>& us, int32_t w,
                         int32_t h, int32_t format, bool frame_by_frame, const ShardHooks& hooks) {
  const size_t px = static_cast<size_t>(rt4_frame_format_bytes(format));
  const BandPlans plan(gpus, band, w, h, "--gpus");
  std::vector<char> pipelined(static_cast<size_t>(gpus), 0);
  ShardJob job;
  job.flag = "--gpus";
  job.shard_bytes = static_cast<size_t>(plan.rows_max) * w * px;
  job.image_bytes = static_cast<size_t>(w) * h * px;
  job.setup = [&](int r, rt4_context* ctx, char* err, size_t errlen) {
    const rt4_region& reg = plan.reg[static_cast<size_t>(r)];
    pipelined[static_cast<size_t>(r)] =
        !frame_by_frame && us.size() >= 2 && reg.h > 0 && rt4_context_frames_per_launch(ctx, reg.w, reg.h) > 1;
    return !pipelined[static_cast<size_t>(r)] || rt4_context_reserve_frames(ctx, reg.w, reg.h, err, errlen) == RT4_OK;
  };
  job.render = [&](int r, rt4_context* ctx, void* shard, unsigned long long* d_count, hipStream_t stream, char* err,
                   size_t errlen) {
    const rt4_region& reg = plan.reg[static_cast<size_t>(r)];
    int st = RT4_OK;
    if (reg.h <= 0) return st;
    if (pipelined[static_cast<size_t>(r)]) {
      st = rt4_render_frames_device(ctx, us.data(), static_cast<int32_t>(us.size()), &reg, shard, format, w, d_count, stream,
                                    err, errlen);
    } else {
      for (size_t f = 0; f < us.size() && st == RT4_OK; f++)
        st = rt4_render_device_ex(ctx, &us[f], &reg, shard, format, w, d_count, stream, err, errlen);
    }
    return st;
  };
  job.finish = [&](rt4_context*, const void* gathered, void* image, hipStream_t stream, char* err, size_t errlen) {
    return rt4_bands_unpermute_device(gathered, image, w, h, gpus, band, plan.rows_max, format, stream, err, errlen);
  };
  return render_shards(gpus, scene, job, hooks);
}

// --light-gpus: the light accumulator of one section. bands: the accumulator's pixels in the bands of --gpus, every rank
// all frames of its bands, rt4_light_bands_unpermute_device on the root: bit for bit the one-GPU accumulator. frames:
// every rank the whole image for its block of the frame numbers (rt4_frame_split; a rank without frames leaves its
// shard empty), one rt4_light_merge_device of all ranks' accumulators into the root's empty one: as accurate as the
// one-GPU accumulator, not bit-equal to it. us[n - 1] holds the uniforms of frame n.
ShardResult render_light_shards(int gpus, bool split_bands, int band, const rt4_scene_desc* scene,
                                const std::vector<rt4_uniforms>& us, int32_t w, int32_t h, const ShardHooks& hooks) {
  const size_t px = sizeof(rt4_light_px);
  const int32_t n_frames = static_cast<int32_t>(us.size());
  ShardJob job;
  job.flag = "--light-gpus";
  job.image_bytes = static_cast<size_t>(w) * h * px;
  if (split_bands) {
    const BandPlans plan(gpus, band, w, h, "--light-gpus");
    job.shard_bytes = static_cast<size_t>(plan.rows_max) * w * px;
    job.setup = [&](int r, rt4_context* ctx, char* err, size_t errlen) {
      const rt4_region& reg = plan.reg[static_cast<size_t>(r)];
      return reg.h <= 0 || rt4_context_reserve_frames(ctx, reg.w, reg.h, err, errlen) == RT4_OK;
    };
    job.render = [&](int r, rt4_context* ctx, void* shard, unsigned long long* d_count, hipStream_t stream, char* err,
                     size_t errlen) {
      const rt4_region& reg = plan.reg[static_cast<size_t>(r)];
      if (reg.h <= 0) return static_cast<int>(RT4_OK);
      return rt4_render_light_device(ctx, us.data(), n_frames, &reg, static_cast<rt4_light_px*>(shard), w, d_count, stream,
                                     err, errlen);
    };
    job.finish = [&](rt4_context*, const void* gathered, void* image, hipStream_t stream, char* err, size_t errlen) {
      return rt4_light_bands_unpermute_device(static_cast<const rt4_light_px*>(gathered), static_cast<rt4_light_px*>(image), w,
                                              h, gpus, band, plan.rows_max, stream, err, errlen);
    };
    return render_shards(gpus, scene, job, hooks);
  }
  const rt4_region whole{0, 0, w, h, 0, 0};
  std::vector<int32_t> first(static_cast<size_t>(gpus)), count(static_cast<size_t>(gpus));
  char perr[1024] = {0};
  for (int r = 0; r < gpus; r++)
    if (rt4_frame_split(n_frames, gpus, r, &first[static_cast<size_t>(r)], &count[static_cast<size_t>(r)], perr, sizeof perr) !=
        RT4_OK)
      die("--light-gpus", perr);
  job.shard_bytes = job.image_bytes;
  job.setup = [&](int r, rt4_context* ctx, char* err, size_t errlen) {
    return count[static_cast<size_t>(r)] == 0 || rt4_context_reserve_frames(ctx, w, h, err, errlen) == RT4_OK;
  };
  job.render = [&](int r, rt4_context* ctx, void* shard, unsigned long long* d_count, hipStream_t stream, char* err,
                   size_t errlen) {
    if (count[static_cast<size_t>(r)] == 0) return static_cast<int>(RT4_OK);
    return rt4_render_light_device(ctx, us.data() + first[static_cast<size_t>(r)], count[static_cast<size_t>(r)], &whole,
                                   static_cast<rt4_light_px*>(shard), w, d_count, stream, err, errlen);
  };
  job.finish = [&](rt4_context* ctx, const void* gathered, void* image, hipStream_t stream, char* err, size_t errlen) {
    return rt4_light_merge_device(ctx, static_cast<rt4_light_px*>(image), w, static_cast<const rt4_light_px*>(gathered), w,
                                  static_cast<int64_t>(w) * h, gpus, w, h, stream, err, errlen);
  };
  return render_shards(gpus, scene, job, hooks);
}

uint32_t keys_from(const char* s) {  // controls.cpp:98-113 key names; other letters are ignored
  static const char names[] = "WSDA ULEQ";
  static const uint32_t bits[] = {RT4_KEY_FORWARD, RT4_KEY_BACK, RT4_KEY_RIGHT, RT4_KEY_LEFT, RT4_KEY_UP,
                                  RT4_KEY_UP,      RT4_KEY_DOWN, RT4_KEY_W_POS, RT4_KEY_W_NEG};
  uint32_t k = 0;
  for (; *s; ++s) if (const char* at = std::strchr(names, *s)) k |= bits[at - names];
  return k;
}

// A params struct of the library with its defaults: defaults(rt4_denoise_params_default).
template <class P> P defaults(void (*fill)(P*)) {
  P p;
  fill(&p);
  return p;
}

// The command line (parse_args). What may go together is refuse_conflicts' business.
struct Options {
  // what to render, from where, and where to write it
  std::string props_path = "properties.txt", scene_arg, out = "frame", fmt_name = "f32";
  int frames = 1, device = 0, width = 0, height = 0;
  int32_t format = RT4_FRAME_RGBA32F;  // from fmt_name (-f)
  uint32_t seed = 12345, keys = 0;
  float move_seconds = 0.0f;
  bool three = false, frame_by_frame = false, png = false, raw = false, reproject = false;
  // --gpus and --light-gpus (the light path's own)
  int gpus = 0, light_gpus = 0, band = 8;
  bool rehearse = false, light_split_given = false;
  std::string light_split = "frames";
  // checkpoints: the colour path's; the light path's own, and the files of --light-pool
  std::string resume_path, checkpoint_path, light_resume_path, light_checkpoint_path;
  std::vector<std::string> light_pool;
  // --denoise: 0 = off; --light-denoise: -1 = off; --window: 0 = off, -1 = the properties' cell_size
  int denoise_levels = 0, light_denoise_levels = -1, window_scale = 0;
  bool window_nearest = false, light = false, noise_map = false;
  float noise_threshold = 1.0f / 255.0f;  // --noise-threshold: one 8-bit step
  int supersample = 0;                    // --supersample S: 0 = off
  bool supersample_given = false;
  // --adaptive (needs --light): the loop of DESIGN.md §4.39 in place of -n uniform frames; -n is then the budget in
  // whole-frame equivalents. The defaults are the values of that section's study.
  bool adaptive = false, ad_given = false;
  int ad_warmup = 8, ad_pass = 4, ad_full_every = 4;  // --adaptive-warmup / --adaptive-pass / --adaptive-full-every
  // --adaptive-min-above / --adaptive-dilate; threshold: --noise-threshold
  rt4_tile_select_params ad_select = defaults(rt4_tile_select_params_default);
  // --retina D: 0 = off; the --retina-* flags: size 0 = the matrix height, the view in degrees
  int retina_depth = 0, retina_turntable = 0;
  bool retina = false, retina_given = false;
  float retina_size = 0.0f, retina_yaw = 30.0f, retina_pitch = 20.0f, retina_step = 1.0f;

  bool pool() const { return !light_pool.empty(); }
  bool moving() const { return keys && move_seconds > 0.0f; }
  bool checkpoints() const { return !resume_path.empty() || !checkpoint_path.empty(); }
  int32_t px() const { return rt4_frame_format_bytes(format); }  // bytes per pixel of a frame
  // One section and a resting camera (progressive accumulation): the frames go to the library in one
  // rt4_render_frames_device call (pipelined through one pixel queue; the same final image).
  bool pipelined() const { return !three && !moving() && !frame_by_frame && !reproject && !light; }
};

// The number after a flag that may also stand alone: the next argument if it starts with a digit, else alone.
int optional_number(int argc, char** argv, int& i, int alone) {
  return i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9' ? std::atoi(argv[++i]) : alone;
}

Options parse_args(int argc, char** argv) {
  Options o;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto next = [&]() -> const char* {
      if (i + 1 >= argc) die("missing value for", a.c_str());
      return argv[++i];
    };
    if (a == "-p") o.props_path = next();
    else if (a == "-s") o.scene_arg = next();
    else if (a == "-n") o.frames = std::atoi(next());
    else if (a == "-3") o.three = true;
    else if (a == "-W") o.width = std::atoi(next());
    else if (a == "-H") o.height = std::atoi(next());
    else if (a == "-f") o.fmt_name = next();
    else if (a == "--seed") o.seed = static_cast<uint32_t>(std::strtoul(next(), nullptr, 0));
    else if (a == "-o") o.out = next();
    else if (a == "-d") o.device = std::atoi(next());
    else if (a == "--keys") o.keys = keys_from(next());
    else if (a == "--frame-by-frame") o.frame_by_frame = true;
    else if (a == "--move-seconds") o.move_seconds = static_cast<float>(std::atof(next()));
    else if (a == "--gpus") o.gpus = std::atoi(next());
    else if (a == "--band") o.band = std::atoi(next());
    else if (a == "--resume") o.resume_path = next();
    else if (a == "--checkpoint") o.checkpoint_path = next();
    else if (a == "--png") o.png = true;
    else if (a == "--raw") o.raw = true;
    else if (a == "--rehearse") o.rehearse = true;
    else if (a == "--reproject") o.reproject = true;
    else if (a == "--light") o.light = true;
    else if (a == "--noise-map") o.noise_map = true;
    else if (a == "--noise-threshold") o.noise_threshold = static_cast<float>(std::atof(next()));
    else if (a == "--supersample") o.supersample = std::atoi(next()), o.supersample_given = true;
    else if (a == "--light-resume") o.light_resume_path = next();
    else if (a == "--light-checkpoint") o.light_checkpoint_path = next();
    else if (a == "--light-gpus") o.light_gpus = std::atoi(next());
    else if (a == "--light-split") o.light_split = next(), o.light_split_given = true;
    else if (a == "--light-pool") {  // every following argument up to the next flag
      while (i + 1 < argc && argv[i + 1][0] != '-') o.light_pool.push_back(argv[++i]);
      if (o.light_pool.size() < 2) die("--light-pool", "needs two or more light checkpoints");
      o.light = true;
    } else if (a == "--adaptive") o.adaptive = true;
    else if (a == "--adaptive-warmup") o.ad_warmup = std::atoi(next()), o.ad_given = true;
    else if (a == "--adaptive-pass") o.ad_pass = std::atoi(next()), o.ad_given = true;
    else if (a == "--adaptive-full-every") o.ad_full_every = std::atoi(next()), o.ad_given = true;
    else if (a == "--adaptive-min-above") o.ad_select.min_above = std::atoi(next()), o.ad_given = true;
    else if (a == "--adaptive-dilate") o.ad_select.dilate = std::atoi(next()), o.ad_given = true;
    else if (a == "--retina") o.retina_depth = std::atoi(next()), o.retina = true;
    else if (a == "--retina-size") o.retina_size = static_cast<float>(std::atof(next())), o.retina_given = true;
    else if (a == "--retina-view") {
      o.retina_yaw = static_cast<float>(std::atof(next()));
      o.retina_pitch = static_cast<float>(std::atof(next()));
      o.retina_given = true;
    } else if (a == "--retina-turntable") o.retina_turntable = std::atoi(next()), o.retina_given = true;
    else if (a == "--retina-step") o.retina_step = static_cast<float>(std::atof(next())), o.retina_given = true;
    else if (a == "--window-nearest") o.window_nearest = true, o.window_scale = o.window_scale ? o.window_scale : -1;
    else if (a == "--window") {
      o.window_scale = optional_number(argc, argv, i, -1);
      if (o.window_scale != -1 && (o.window_scale < 1 || o.window_scale > RT4_UPSCALE_MAX_SCALE))
        die("--window", "SCALE must be 1..64");
    } else if (a == "--denoise") {
      o.denoise_levels = optional_number(argc, argv, i, defaults(rt4_denoise_params_default).levels);
      if (o.denoise_levels < 1 || o.denoise_levels > RT4_DENOISE_MAX_LEVELS) die("--denoise", "levels must be 1..6");
    } else if (a == "--light-denoise") {
      o.light_denoise_levels = optional_number(argc, argv, i, defaults(rt4_light_denoise_params_default).levels);
      if (o.light_denoise_levels < 0 || o.light_denoise_levels > RT4_LIGHT_DENOISE_MAX_LEVELS)
        die("--light-denoise", "levels must be 0..6");
    } else die("unknown argument", a.c_str());
  }
  if (o.supersample_given && (o.supersample < 1 || o.supersample > RT4_SUPERSAMPLE_MAX)) die("--supersample", "S must be 1..8");
  o.format = o.fmt_name == "f16" ? RT4_FRAME_RGBA16F : o.fmt_name == "rgba8" ? RT4_FRAME_RGBA8 : RT4_FRAME_RGBA32F;
  if (o.pool()) o.frames = 0;  // nothing is rendered
  return o;
}

// --retina and its flags, ahead of every other refusal (a command line without them passes straight through): the
// volume is one section's light accumulation on one GPU with a resting camera, and it writes projections only.
void refuse_retina_conflicts(const Options& o) {
  const char* f = "--retina";
  if (o.retina_given && !o.retina) die(f, "--retina-size / --retina-view / --retina-turntable / --retina-step need --retina D");
  if (!o.retina) return;
  if (o.retina_depth < 1 || o.retina_depth > RT4_RETINA_MAX_DEPTH) die(f, "D must be 1..256 slices");
  if (o.gpus > 0 || o.light_gpus != 0) die(f, "not with --gpus / --light-gpus: the volume is accumulated on one GPU");
  if (o.three) die(f, "not with -3: the volume holds the main section's view");
  if (o.reproject) die(f, "not with --reproject: the volume is a light accumulation of one view");
  if (o.adaptive || o.ad_given) die(f, "not with --adaptive: every slice takes every frame");
  if (o.denoise_levels > 0 || o.light_denoise_levels >= 0) die(f, "not with --denoise / --light-denoise: the projection is not filtered");
  if (o.window_scale != 0) die(f, "not with --window: the projection is written at the window's size already");
  if (o.checkpoints() || !o.light_resume_path.empty() || !o.light_checkpoint_path.empty() || o.pool())
    die(f, "not with --resume / --checkpoint / --light-resume / --light-checkpoint / --light-pool: no file format holds a volume");
  if (o.frame_by_frame) die(f, "not with --frame-by-frame: the frames go through rt4_render_light_device");
  if (o.moving()) die(f, "needs a resting camera: the volume accumulates one view");
  if (o.frames < 1) die(f, "frames must be >= 1");
  if (o.retina_given && (!(o.retina_size >= 0.0f) || !std::isfinite(o.retina_size) || !std::isfinite(o.retina_yaw) ||
                         !std::isfinite(o.retina_pitch) || o.retina_turntable < 0 || !(o.retina_step > 0.0f) ||
                         !std::isfinite(o.retina_step)))
    die(f, "size >= 0 (0: the matrix height), a view of two angles in degrees, turntable >= 0, step > 0");
}

// --supersample: the render is S times the output, and rt4_render_light_device takes at most 8191 per side. With -W -H
// refuse_conflicts knows the output; the properties' cells are known once load_inputs has read them.
void refuse_supersample_size(const Options& o, int32_t w, int32_t h) {
  const long long fw = static_cast<long long>(w) * o.supersample, fh = static_cast<long long>(h) * o.supersample;
  if (fw > 8191 || fh > 8191)
    die("--supersample", ("the render would be " + std::to_string(fw) + "x" + std::to_string(fh) +
                          ": the light render takes at most 8191 x 8191").c_str());
}

// Every combination of flags that is refused whatever the files hold, in one place: the first check that fails is the
// one reported, so the order below is part of the program's behaviour (tests/test_render_cli_refusals.py pins it).
// What depends on a file's contents (a checkpoint's seed, key, size, pooled flag; the 2^32 frame bound) is refused by
// load_inputs, and a missing device by need_devices, after this.
void refuse_conflicts(const Options& o) {
  refuse_retina_conflicts(o);
  if (o.reproject && o.gpus > 0) die("--reproject", "not with --gpus: the temporal image lives on one GPU");
  if (o.reproject && o.checkpoints())
    die("--reproject", "not with --resume / --checkpoint: a checkpoint holds no per-pixel history");
  if (o.reproject && o.frame_by_frame)
    die("--reproject", "not with --frame-by-frame: every temporal frame is a launch of its own");
  if (o.light && o.reproject) die("--light", "not with --reproject: the temporal history is a colour average");
  if (o.light && o.checkpoints())
    die("--light", "not with --resume / --checkpoint: a checkpoint holds colours, not a light accumulator "
                   "(--light-resume / --light-checkpoint save and continue a light accumulator)");
  if (o.light && o.gpus > 0)
    die("--light", "not with --gpus: that gathers colour frames (--light-gpus N runs a light accumulator on N GPUs)");
  const bool light_files = !o.light_resume_path.empty() || !o.light_checkpoint_path.empty();
  if ((light_files || o.light_gpus != 0 || o.light_split_given) && !o.light)
    die("--light-resume / --light-checkpoint / --light-gpus / --light-split", "need --light");
  if (o.light_split_given && o.light_gpus == 0) die("--light-split", "needs --light-gpus");
  if (o.light_split != "frames" && o.light_split != "bands") die("--light-split", "frames or bands");
  if (o.light_gpus != 0 && (o.light_gpus < 1 || o.light_gpus > RT4_LIGHT_MERGE_MAX))
    die("--light-gpus", "N must be 1..16 (RT4_LIGHT_MERGE_MAX: one merge takes that many accumulators)");
  if (o.light_gpus > 0 && o.adaptive) die("--light-gpus", "not with --adaptive: the tile selection runs on one GPU");
  if (o.light_gpus > 0 && !o.light_resume_path.empty()) die("--light-gpus", "not with --light-resume: resume on one GPU");
  if (!o.light_resume_path.empty() && o.adaptive)
    die("--light-resume", "not with --adaptive: a light checkpoint does not hold the adaptive loop's pass state");
  if (o.pool() && (o.adaptive || o.light_gpus > 0 || !o.light_resume_path.empty() || o.three || o.denoise_levels > 0 ||
                   o.light_denoise_levels >= 0 || o.window_scale != 0 || o.reproject))
    die("--light-pool", "renders nothing: only with -o, --png, --raw, --noise-map, --noise-threshold, --light-checkpoint");
  if (o.light && o.frame_by_frame) die("--light", "not with --frame-by-frame: the frames go through rt4_render_light_device");
  if (o.light && o.moving()) die("--light", "needs a resting camera: the accumulator averages one view");
  if ((o.noise_map || o.noise_threshold != 1.0f / 255.0f) && !o.light) die("--noise-map / --noise-threshold", "need --light");
  if ((o.adaptive || o.ad_given) && !o.light)
    die("--adaptive", "needs --light: it samples by the light accumulator's standard error");
  if (o.ad_given && !o.adaptive) die("--adaptive-*", "need --adaptive");
  if (o.adaptive && (o.ad_warmup < 0 || o.ad_pass < 1 || o.ad_full_every < 0 || o.ad_select.min_above < 1 ||
                     o.ad_select.min_above > 64 || o.ad_select.dilate < 0 || o.ad_select.dilate > RT4_SELECT_MAX_DILATE ||
                     o.noise_threshold != o.noise_threshold))
    die("--adaptive", "warmup >= 0, pass >= 1, full-every >= 0, min-above 1..64, dilate 0..2, a threshold that is a number");
  if (o.light_denoise_levels >= 0 && !o.light) die("--light-denoise", "needs --light: it filters the light accumulator");
  if (o.light_denoise_levels >= 0 && o.denoise_levels > 0)
    die("--light-denoise", "not with --denoise: one filtered frame per image");
  // These once ran between and after the loads. Whenever a checkpoint loader could have run ahead of one of them, a
  // check above has already refused the command line, so only a command line that is refused here and also names a
  // properties or scene file that does not load hears another message than it used to: this one.
  if (o.checkpoints() && (o.three || o.gpus > 0)) die("--resume/--checkpoint", "need one section on one GPU");
  if (light_files && o.three) die("--light-resume / --light-checkpoint", "need one section");
  // as --gpus: one section (the camera rests in every --light run)
  if (o.light_gpus > 0 && o.three) die("--light-gpus", "needs one section");
  if (o.light_gpus > 0 && (o.frames < 1 || o.band < 1)) die("--light-gpus", "frames and band must be >= 1");
  if (o.gpus > 0 && o.denoise_levels > 0) die("--denoise", "not with --gpus: the frame is not filtered after the gather");
  if (o.gpus > 0 && o.window_scale != 0) die("--window", "not with --gpus: the frame is not upscaled after the gather");
  // pixel bands over GPUs 0..gpus-1, one RCCL gather (one section, resting camera)
  if (o.gpus > 0 && (o.three || o.moving())) die("--gpus", "needs one section and a resting camera");
  if (o.gpus > 0 && (o.frames < 1 || o.band < 1)) die("--gpus", "frames and band must be >= 1");
  if (o.supersample_given && !o.light) die("--supersample", "needs --light: it averages light accumulators");
  if (o.supersample_given && (o.light_gpus != 0 || o.pool() || o.retina))
    die("--supersample", "not with --light-gpus, --light-pool or --retina");
  if (o.supersample_given && o.width > 0 && o.height > 0) refuse_supersample_size(o, o.width, o.height);
}

// --gpus / --light-gpus without --rehearse (a rehearsal puts every rank on device 0 and reports a missing device per rank)
void need_devices(const char* flag, int n) {
  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  if (n > ndev) die(flag, ("only " + std::to_string(ndev) + " HIP devices").c_str());
}

// One image of the run: the main section (window.main cells, or -W/-H) or, with -3, YWZ / YXW (window.additional).
struct Section {
  int id;
  const char *name, *window;  // "yxz", and whose cells and cell_size in the properties: "main" / "additional"
  int32_t w = 0, h = 0;
  rt4_uniforms base = {};           // from the properties, at w x h
  // What the frames are rendered at: w x h and base, or with --supersample S the view at S times the resolution
  // (rt4_upscale_uniforms), whose accumulator d_fine is downsampled into d_light.
  int32_t fw = 0, fh = 0;
  rt4_uniforms fine = {};
  rt4_light_px* d_fine = nullptr;
  int32_t win_scale = 0;            // --window: this section's scale
  void* d_frame = nullptr;          // the image, in the run's frame format
  rt4_light_px* d_light = nullptr;  // --light: the accumulator
  rt4_temporal* temporal = nullptr;  // --reproject
  rt4_uniforms last_u = {};         // the last frame's uniforms: the camera pose the images show

  size_t pixels() const { return static_cast<size_t>(w) * h; }
  size_t frame_bytes(int32_t px) const { return pixels() * static_cast<size_t>(px); }
  rt4_region region() const { return rt4_region{0, 0, w, h, 0, 0}; }
  size_t fine_pixels() const { return static_cast<size_t>(fw) * fh; }
  rt4_region fine_region() const { return rt4_region{0, 0, fw, fh, 0, 0}; }
  rt4_light_px* accum() const { return d_fine ? d_fine : d_light; }  // --light: the accumulator the frames fold into
  float tone() const { return base.light_to_color_conversion_coefficient; }  // of the tone curve (resolve, filter, noise)
};

char err[1024] = {0};  // RT4_CHECK's message buffer in the steps below (the main thread's)

// What the steps hand on: everything the run reads before it touches a GPU (load_inputs), and the one-GPU run's
// device state besides the sections' buffers (open_render).
struct Run {
  rt4_properties* props = nullptr;
  rt4_scene_desc* scene = nullptr;
  std::vector<Section> sections;
  rt4_camera cam;
  // the run's key, checked on --resume and recorded by --checkpoint: the first frame's uniforms (seed and
  // part aside they are every resting frame's)
  uint32_t run_key = 0;
  int64_t frames_done = 0;  // frames already blended into the accumulator (a resumed run continues at frame frames_done + 1)
  std::vector<unsigned char> resumed;     // --resume: the loaded frame
  std::vector<rt4_light_px> light_start;  // --light-resume: the loaded accumulator; --light-pool: every file's, in order
  uint32_t pool_seed = 0, pool_key = 0;   // --light-pool: the first file's
  int64_t pool_issued = 0;

  rt4_context* ctx = nullptr;
  unsigned long long* d_count = nullptr;
  hipEvent_t e0, e1;             // around render_frames
  std::vector<rt4_uniforms> us;  // the pipelined run's frames (pipelined_frames)
  int64_t light_issued = 0;  // the last progressive frame number folded into the light accumulator, for --light-checkpoint
  double shards_ms = -1.0;   // --light-gpus: the slowest rank's time, in place of the events'
  unsigned long long shards_count = 0, count = 0;  // intersections: the ranks'; the run's (render_frames)
  float ms = 0.0f;                                 // render_frames: the time between its two event records
};

// --resume: the accumulator the run continues, refused rather than mixed with another run's frames
void load_resumed(const Options& o, Run& r) {
  const Section& s = r.sections[0];
  uint32_t ck_seed = 0, ck_key = 0;
  r.resumed.resize(s.frame_bytes(o.px()));
  RT4_CHECK(rt4_accum_load(o.resume_path.c_str(), r.resumed.data(), o.format, s.w, s.h, s.w, &r.frames_done, &ck_seed, err,
                           sizeof err));
  if (ck_seed != o.seed) die("--resume", "the checkpoint was made with another --seed");
  // the checkpoint's run key (scene, samples, bounces, resolution, camera ...): a checkpoint of
  // another run would be blended in silently
  RT4_CHECK(rt4_accum_key_of(o.resume_path.c_str(), &ck_key, err, sizeof err));
  if (ck_key != 0u && ck_key != r.run_key) die("--resume", "the checkpoint was made with another scene, properties or camera");
  r.cam.frame_number = static_cast<uint32_t>(r.frames_done + 1);
}

// --light-resume: the light accumulator the run continues (frames frames_done + 1 ...)
void load_light_resumed(const Options& o, Run& r) {
  const Section& s = r.sections[0];
  const char* path = o.light_resume_path.c_str();
  uint32_t ck_seed = 0, ck_key = 0, ck_flags = 0;
  int32_t ck_w = 0, ck_h = 0;
  RT4_CHECK(rt4_light_info(path, &ck_w, &ck_h, nullptr, &ck_seed, &ck_key, &ck_flags, err, sizeof err));
  if (ck_flags & RT4_LIGHT_POOLED) die("--light-resume", "the checkpoint pools runs of several seeds: it cannot be resumed");
  if (ck_w != s.fw || ck_h != s.fh)
    die("--light-resume", ("the checkpoint holds a " + std::to_string(ck_w) + "x" + std::to_string(ck_h) + " accumulator, not " +
                           std::to_string(s.fw) + "x" + std::to_string(s.fh)).c_str());
  if (ck_seed != o.seed) die("--light-resume", "the checkpoint was made with another --seed");
  if (ck_key != 0u && ck_key != r.run_key)
    die("--light-resume", "the checkpoint was made with another scene, properties or camera");
  r.light_start.resize(s.fine_pixels());
  RT4_CHECK(rt4_light_load(path, r.light_start.data(), s.fw, s.fh, s.fw, &r.frames_done, nullptr, nullptr, nullptr, err,
                           sizeof err));
  if (r.frames_done + o.frames > 0xFFFFFFFFll) die("--light-resume", "frame numbers beyond 2^32 - 1");
  r.cam.frame_number = static_cast<uint32_t>(r.frames_done + 1);
}

// --light-pool: the accumulators of independent runs, merged once there is a context. The main section takes its size
// from the first file, while its uniforms (the tone curve's coefficient is what the outputs use) stay the properties'.
void load_pool(const Options& o, Run& r) {
  Section& s = r.sections[0];
  std::vector<uint32_t> seeds;
  for (size_t f = 0; f < o.light_pool.size(); f++) {
    const char* path = o.light_pool[f].c_str();
    int32_t fw = 0, fh = 0;
    int64_t issued = 0;
    uint32_t ck_seed = 0, ck_key = 0;
    RT4_CHECK(rt4_light_info(path, &fw, &fh, &issued, &ck_seed, &ck_key, nullptr, err, sizeof err));
    if (f == 0) {
      s.w = s.fw = fw, s.h = s.fh = fh, r.pool_seed = ck_seed, r.pool_key = ck_key, r.pool_issued = issued;
      r.light_start.resize(o.light_pool.size() * s.pixels());
    }
    if (fw != s.w || fh != s.h) die("--light-pool: another image size than the first file's", path);
    if (ck_key != r.pool_key) die("--light-pool: another scene, properties or camera than the first file's", path);
    if (std::find(seeds.begin(), seeds.end(), ck_seed) != seeds.end())
      die("--light-pool: the same --seed as an earlier file, the same frames would count twice", path);
    seeds.push_back(ck_seed);
    RT4_CHECK(rt4_light_load(path, r.light_start.data() + f * s.pixels(), fw, fh, fw, nullptr, nullptr, nullptr, nullptr, err,
                             sizeof err));
  }
}

// Step 1: properties, scene, sections, camera, the run's key, and the checkpoints of --resume, --light-resume, --light-pool.
Run load_inputs(const Options& o) {
  Run r;
  RT4_CHECK(rt4_properties_load(o.props_path.c_str(), &r.props, err, sizeof err));
  // scene: -s builtin name or .frag path; else the properties' shader_filename (main.cpp:26)
  r.scene = static_cast<rt4_scene_desc*>(std::calloc(1, sizeof(rt4_scene_desc)));
  std::string scene_arg = o.scene_arg;
  if (scene_arg.empty()) {
    char buf[4096];
    size_t need = 0;
    RT4_CHECK(rt4_properties_get_string(r.props, "shader_filename", buf, sizeof buf, &need, err, sizeof err));
    scene_arg = buf;
  }
  if (scene_arg.size() > 5 && scene_arg.compare(scene_arg.size() - 5, 5, ".frag") == 0)
    RT4_CHECK(rt4_scene_load_frag(scene_arg.c_str(), r.scene, err, sizeof err));
  else
    RT4_CHECK(rt4_scene_builtin(scene_arg.c_str(), r.scene, err, sizeof err));

  static const Section kinds[3] = {{RT4_SECTION_YXZ, "yxz", "main"}, {RT4_SECTION_YWZ, "ywz", "additional"},
                                   {RT4_SECTION_YXW, "yxw", "additional"}};
  r.sections.assign(kinds, kinds + (o.three ? 3 : 1));
  Section& yxz = r.sections[0];
  const bool sized = o.width > 0 && o.height > 0;  // -W -H: the main section's cells, in place of the properties'
  for (Section& s : r.sections)
    if (!(sized && &s == &yxz)) RT4_CHECK(rt4_window_cells(r.props, s.window, &s.w, &s.h, err, sizeof err));
  if (sized) yxz.w = o.width, yxz.h = o.height;
  for (Section& s : r.sections) {
    RT4_CHECK(rt4_uniforms_from_properties(r.props, s.w, s.h, s.id, &s.base, nullptr, err, sizeof err));
    s.fw = s.w, s.fh = s.h, s.fine = s.base;
    if (!o.supersample_given) continue;
    refuse_supersample_size(o, s.w, s.h);
    s.fw = s.w * o.supersample, s.fh = s.h * o.supersample;
    if (rt4_upscale_uniforms(&s.base, o.supersample, &s.fine) != RT4_OK) die("--supersample", "rt4_upscale_uniforms refused the view");
  }
  RT4_CHECK(rt4_camera_init(r.props, &r.cam, err, sizeof err));
  rt4_camera c0 = r.cam;
  rt4_uniforms u0;
  RT4_CHECK(rt4_camera_frame_uniforms(&c0, &yxz.fine, yxz.id, 0, &u0));
  r.run_key = rt4_accum_key(r.scene, &u0);

  if (!o.resume_path.empty()) load_resumed(o, r);
  if (!o.light_resume_path.empty()) load_light_resumed(o, r);
  if (o.pool()) load_pool(o, r);
  return r;
}

// --window: every section's scale, the flag's or the cell_size of the section's window in the properties
void window_scales(const Options& o, Run& r) {
  for (Section& s : r.sections) {
    s.win_scale = o.window_scale;
    const std::string key = std::string("window.") + s.window + ".cell_size";
    if (o.window_scale < 0) RT4_CHECK(rt4_properties_get_int(r.props, key.c_str(), &s.win_scale, err, sizeof err));
  }
}

// The seed of progressive frame n, counted from the run's first frame (a resumed run passes frames_done + n):
// main.cpp's seed ^= generateSeed(timer), deterministic.
int32_t frame_seed(uint32_t seed, int64_t n) { return static_cast<int32_t>(seed ^ (static_cast<uint32_t>(n) * 0x9E3779B9u)); }

// The uniforms of the run's -n frames of a section with a resting camera, at the resolution they are rendered at
// (s.fine: s.base unless --supersample); the camera's frame number moves on by -n.
std::vector<rt4_uniforms> resting_frames(const Options& o, Run& r, const Section& s) {
  std::vector<rt4_uniforms> us(static_cast<size_t>(std::max(o.frames, 0)));
  for (int64_t n = 1; n <= o.frames; n++)
    RT4_CHECK(rt4_camera_frame_uniforms(&r.cam, &s.fine, s.id, frame_seed(o.seed, r.frames_done + n), &us[n - 1]));
  return us;
}

void write_raw(const std::string& path, const void* data, size_t bytes) {  // --raw
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) die("--raw", path.c_str());
  const bool ok = std::fwrite(data, 1, bytes, f) == bytes;
  if (std::fclose(f) != 0 || !ok) die("--raw: write failed", path.c_str());
}

// One image of a section, <prefix>_<section><suffix>.png or .ppm: w x h pixels of `format` in `bytes` bytes at data.
// raw_twin: with --raw also the bytes themselves, <prefix>_<section><suffix>.raw. Then the line "wrote <path>
// (<w> x <h><note>)"; a note starts with ", ".
void write_image(const Options& o, const char* section, const char* suffix, const void* data, size_t bytes, int32_t format,
                 int32_t w, int32_t h, bool raw_twin, const std::string& note) {
  const std::string stem = o.out + "_" + section + suffix, path = stem + (o.png ? ".png" : ".ppm");
  RT4_CHECK((o.png ? rt4_write_png : rt4_write_ppm)(path.c_str(), data, format, w, h, w, err, sizeof err));
  if (raw_twin && o.raw) write_raw(stem + ".raw", data, bytes);
  std::printf("wrote %s (%d x %d%s)\n", path.c_str(), w, h, note.c_str());
}

// One value per pixel as an opaque grey fp32 frame (the _q and _n maps; the writers clamp to [0, 1]).
std::vector<float> grey_image(const std::vector<float>& values) {
  std::vector<float> grey(values.size() * 4, 1.0f);
  for (size_t p = 0; p < values.size(); p++) grey[4 * p] = grey[4 * p + 1] = grey[4 * p + 2] = values[p];
  return grey;
}

template <class T> T* device_alloc(size_t n, bool zeroed = false) {
  void* p = nullptr;
  HIP_CHECK(hipMalloc(&p, n * sizeof(T)));
  if (zeroed) HIP_CHECK(hipMemset(p, 0, n * sizeof(T)));
  return static_cast<T*>(p);
}

template <class T> std::vector<T> device_read(const void* d, size_t n) {
  std::vector<T> host(n);
  HIP_CHECK(hipMemcpy(host.data(), d, n * sizeof(T), hipMemcpyDeviceToHost));
  return host;
}

// The run in one line; gpus: what a multi-GPU run puts in front ("gpus 3, ").
void print_summary(const std::string& gpus, int frames, size_t images, unsigned long long count, double ms_per_frame, double ms) {
  std::printf("%sframes %d, images %zu, intersections %llu, %.3f ms/frame, %.3e intersections/s\n", gpus.c_str(), frames, images,
              count, ms_per_frame, static_cast<double>(count) / (ms * 1e-3));
}

// Step 2 with --gpus: the whole run. Pixel bands over GPUs 0..gpus-1, one RCCL gather, the image and the summary. The
// ranks create their own contexts; none is created here.
void run_bands(const Options& o, const ShardHooks& hooks, Run& r) {
  const Section& s = r.sections[0];
  const ShardResult res =
      render_bands(o.gpus, o.band, r.scene, resting_frames(o, r, s), s.w, s.h, o.format, o.frame_by_frame, hooks);
  write_image(o, s.name, "", res.image.data(), res.image.size(), o.format, s.w, s.h, true, "");
  print_summary("gpus " + std::to_string(o.gpus) + ", ", o.frames, 1, res.count, res.ms / o.frames, res.ms);
}

// Step 2 on one GPU: the context, every section's cleared frame (the --resume frame in the main one), the counter, and
// with --reproject one rt4_temporal per section.
void open_render(const Options& o, Run& r) {
  RT4_CHECK(rt4_context_create(o.device, RT4_FLAG_SAMPLER_LUT, &r.ctx, err, sizeof err));
  RT4_CHECK(rt4_context_set_scene(r.ctx, r.scene, err, sizeof err));
  for (Section& s : r.sections) s.d_frame = device_alloc<unsigned char>(s.frame_bytes(o.px()), true);  // cleared RenderTexture
  if (!r.resumed.empty()) HIP_CHECK(hipMemcpy(r.sections[0].d_frame, r.resumed.data(), r.resumed.size(), hipMemcpyHostToDevice));
  r.d_count = device_alloc<unsigned long long>(1, true);
  HIP_CHECK(hipEventCreate(&r.e0));
  HIP_CHECK(hipEventCreate(&r.e1));
  for (Section& s : r.sections)
    if (o.reproject) RT4_CHECK(rt4_temporal_create(r.ctx, s.w, s.h, o.format, &s.temporal, err, sizeof err));
}

// The pipelined run's frames, and the frame-colour scratch only when frames are actually pipelined (>= 2 frames, a
// scene that does not run frame by frame), and only for the frames of one chunk.
void pipelined_frames(const Options& o, Run& r) {
  Section& s = r.sections[0];
  if (o.frames >= 2 && rt4_context_frames_per_launch(r.ctx, s.w, s.h) > 1)
    RT4_CHECK(rt4_context_reserve_frames(r.ctx, s.w, s.h, err, sizeof err));
  r.us = resting_frames(o, r, s);
  if (!r.us.empty()) s.last_u = r.us.back();
}

// --light: one empty accumulator per section; the main one continues --light-resume's, or is --light-pool's files
// merged in order, RT4_LIGHT_MERGE_MAX of them per call, and resolved into the section's frame.
void open_light(const Options& o, Run& r) {
  for (Section& s : r.sections) {
    s.d_light = device_alloc<rt4_light_px>(s.pixels(), true);
    if (o.supersample_given) s.d_fine = device_alloc<rt4_light_px>(s.fine_pixels(), true);  // --supersample: the frames' own
  }
  Section& s = r.sections[0];
  const size_t bytes = s.pixels() * sizeof(rt4_light_px);
  r.light_issued = o.pool() ? r.pool_issued : r.frames_done + o.frames;
  if (!o.light_resume_path.empty())
    HIP_CHECK(hipMemcpy(s.accum(), r.light_start.data(), s.fine_pixels() * sizeof(rt4_light_px), hipMemcpyHostToDevice));
  if (!o.light_resume_path.empty() && s.d_fine)  // with -n 0 nothing else brings the resumed strata into d_light
    RT4_CHECK(rt4_light_downsample_device(r.ctx, s.d_fine, s.fw, s.d_light, s.w, s.w, s.h, o.supersample, nullptr, err, sizeof err));
  if (!o.pool()) return;
  std::vector<rt4_light_px> merged(s.pixels());  // empty: value-initialised
  const int64_t plane = static_cast<int64_t>(s.pixels());
  for (size_t f0 = 0; f0 < o.light_pool.size(); f0 += RT4_LIGHT_MERGE_MAX)
    RT4_CHECK(rt4_light_merge_host(r.ctx, merged.data(), s.w, r.light_start.data() + f0 * s.pixels(), s.w, plane,
                                   static_cast<int32_t>(std::min<size_t>(RT4_LIGHT_MERGE_MAX, o.light_pool.size() - f0)), s.w,
                                   s.h, err, sizeof err));
  HIP_CHECK(hipMemcpy(s.d_light, merged.data(), bytes, hipMemcpyHostToDevice));
  RT4_CHECK(rt4_light_resolve_device(r.ctx, s.d_light, s.w, s.tone(), s.d_frame, o.format, s.w, s.w, s.h, nullptr, err,
                                     sizeof err));
}

// --adaptive, one section: the loop of DESIGN.md §4.39 (Tracer.render_light_adaptive is the same loop): warm-up whole
// frames, then passes of the selected tiles, every ad_full_every-th pass and a pass with an empty selection a whole
// frame; frame g is rt4_progressive_uniforms(ub: the section's uniforms with --seed, g), g running on across the
// passes. Returns the loop's last frame number, whatever share of the image each frame covered.
uint32_t adaptive_passes(const Options& o, Run& r, const Section& s, const rt4_uniforms& ub) {
  const rt4_region reg = s.fine_region();  // the render resolution, as the accumulator the frames fold into
  rt4_light_px* const d_acc = s.accum();
  const long long tiles = static_cast<long long>((s.fw + 7) / 8) * ((s.fh + 7) / 8);
  const long long budget = static_cast<long long>(o.frames) * tiles;
  uint32_t* d_tiles = device_alloc<uint32_t>(static_cast<size_t>(tiles));
  uint32_t* d_n = device_alloc<uint32_t>(1);
  rt4_tile_select_params sel = o.ad_select;
  sel.threshold = o.noise_threshold;
  long long spent = 0;
  uint32_t g = 0;
  std::vector<rt4_uniforms> pus;
  auto pass_uniforms = [&](int n) {
    pus.resize(static_cast<size_t>(n));
    for (int f = 0; f < n; f++) rt4_progressive_uniforms(&ub, ++g, &pus[static_cast<size_t>(f)]);
  };
  const int warm = std::min(o.ad_warmup, o.frames);
  sel.min_frames = warm;
  if (warm > 0) {
    pass_uniforms(warm);
    RT4_CHECK(rt4_render_light_device(r.ctx, pus.data(), warm, &reg, d_acc, s.fw, r.d_count, nullptr, err, sizeof err));
    spent += warm * tiles;
    std::printf("adaptive %s: warmup tiles %lld frames %d\n", s.name, tiles, warm);
  }
  for (int n_pass = 1;; n_pass++) {
    const char* kind = "full";
    long long listed = tiles;
    if (!(o.ad_full_every > 0 && n_pass % o.ad_full_every == 0)) {
      RT4_CHECK(rt4_light_select_tiles_device(r.ctx, d_acc, s.fw, s.fw, s.fh, ub.light_to_color_conversion_coefficient, &sel,
                                              d_tiles, d_n, nullptr, nullptr, err, sizeof err));
      uint32_t n_sel = 0;  // the one 4-byte read of the pass (synchronises)
      HIP_CHECK(hipMemcpy(&n_sel, d_n, sizeof n_sel, hipMemcpyDeviceToHost));
      kind = n_sel == 0 ? "empty" : "tiles";
      if (n_sel != 0) listed = n_sel;
    }
    const int n = static_cast<int>(std::min<long long>(o.ad_pass, (budget - spent) / listed));
    if (n <= 0) break;
    pass_uniforms(n);
    if (listed == tiles && kind[0] != 't')  // a selection that lists every tile still goes through the tile path
      RT4_CHECK(rt4_render_light_device(r.ctx, pus.data(), n, &reg, d_acc, s.fw, r.d_count, nullptr, err, sizeof err));
    else
      RT4_CHECK(rt4_render_light_tiles_device(r.ctx, pus.data(), n, &reg, d_tiles, static_cast<int32_t>(listed), d_acc, s.fw,
                                              r.d_count, nullptr, err, sizeof err));
    spent += n * listed;
    std::printf("adaptive %s: %s tiles %lld frames %d\n", s.name, kind, listed, n);
  }
  HIP_CHECK(hipDeviceSynchronize());
  (void)hipFree(d_tiles);
  (void)hipFree(d_n);
  return g;
}

// --light, one section: its frames into its accumulator (frame n of every section has the same seed, as in
// render_colour_frames) in one of three ways, with --supersample at S times the resolution and downsampled once, then
// the image: the accumulator resolved into the section's frame.
// frame_number: the camera's before the first section, so that every section renders the same frames.
void render_light_section(const Options& o, const ShardHooks& hooks, Run& r, Section& s, uint32_t frame_number) {
  r.cam.frame_number = frame_number;
  const std::vector<rt4_uniforms> lus = resting_frames(o, r, s);
  s.last_u = lus.back();  // the pose the output-resolution images show: the G-buffer and the window render it at w x h
  s.last_u.resolution[0] = s.base.resolution[0], s.last_u.resolution[1] = s.base.resolution[1];
  const rt4_region reg = s.fine_region();
  if (o.light_gpus > 0) {
    // the accumulator of the section from light_gpus devices; resolve and everything after it run here, on the root's
    // accumulator, as in a one-GPU run
    const ShardResult acc = render_light_shards(o.light_gpus, o.light_split == "bands", o.band, r.scene, lus, s.w, s.h, hooks);
    r.shards_count = acc.count, r.shards_ms = acc.ms;
    HIP_CHECK(hipSetDevice(o.device));  // the rank threads chose their own
    HIP_CHECK(hipMemcpy(s.d_light, acc.image.data(), acc.image.size(), hipMemcpyHostToDevice));
  } else if (o.adaptive) {
    rt4_uniforms ub;
    r.cam.frame_number = frame_number;
    RT4_CHECK(rt4_camera_frame_uniforms(&r.cam, &s.fine, s.id, static_cast<int32_t>(o.seed), &ub));
    r.cam.frame_number = frame_number + static_cast<uint32_t>(o.frames);  // as the uniform frames above left it
    r.light_issued = adaptive_passes(o, r, s, ub);
  } else {
    RT4_CHECK(rt4_render_light_device(r.ctx, lus.data(), o.frames, &reg, s.accum(), s.fw, r.d_count, nullptr, err, sizeof err));
  }
  if (s.d_fine)  // the S x S strata of every output pixel into its accumulator; everything below reads that one
    RT4_CHECK(rt4_light_downsample_device(r.ctx, s.d_fine, s.fw, s.d_light, s.w, s.w, s.h, o.supersample, nullptr, err, sizeof err));
  RT4_CHECK(rt4_light_resolve_device(r.ctx, s.d_light, s.w, s.tone(), s.d_frame, o.format, s.w, s.w, s.h, nullptr, err,
                                     sizeof err));
}

// The colour frames: pipelined (us: pipelined_frames), or frame by frame: all sections of a frame in one launch, the
// camera moved after it (--keys), or with --reproject every section's frame through its rt4_temporal, whose images
// are then the images written.
void render_colour_frames(const Options& o, Run& r) {
  if (o.pipelined()) {
    const Section& s = r.sections[0];
    const rt4_region reg = s.region();
    RT4_CHECK(rt4_render_frames_device(r.ctx, r.us.data(), o.frames, &reg, s.d_frame, o.format, s.w, r.d_count, nullptr, err,
                                       sizeof err));
    return;
  }
  const int n_img = static_cast<int>(r.sections.size());
  for (int n = 1; n <= o.frames; n++) {
    rt4_section_job jobs[3];
    const uint32_t frame_number = r.cam.frame_number;
    for (int q = 0; q < n_img; q++) {
      Section& s = r.sections[static_cast<size_t>(q)];
      r.cam.frame_number = frame_number;  // one frame: every section gets the same part
      RT4_CHECK(rt4_camera_frame_uniforms(&r.cam, &s.base, s.id, frame_seed(o.seed, r.frames_done + n), &jobs[q].u));
      jobs[q].region = s.region();
      jobs[q].d_frame = s.d_frame;
      jobs[q].row_stride_px = s.w;
      s.last_u = jobs[q].u;
      if (o.reproject) RT4_CHECK(rt4_temporal_frame_device(s.temporal, &jobs[q].u, nullptr, r.d_count, nullptr, err, sizeof err));
    }
    if (!o.reproject) RT4_CHECK(rt4_render_sections_device(r.ctx, jobs, n_img, o.format, r.d_count, nullptr, err, sizeof err));
    if (o.moving()) rt4_camera_move(&r.cam, o.keys, o.move_seconds);  // move(seconds), main.cpp:95-96
  }
  if (!o.reproject) return;
  for (Section& s : r.sections)  // the images written are the temporal images
    HIP_CHECK(hipMemcpyAsync(s.d_frame, rt4_temporal_image(s.temporal), s.frame_bytes(o.px()), hipMemcpyDeviceToDevice, nullptr));
}

// Step 3: every frame of every section between two event records, and what they counted and took.
void render_frames(const Options& o, const ShardHooks& hooks, Run& r) {
  HIP_CHECK(hipEventRecord(r.e0, nullptr));
  const uint32_t frame_number = r.cam.frame_number;
  for (Section& s : r.sections)
    if (o.light && o.frames >= 1) render_light_section(o, hooks, r, s, frame_number);
  if (!o.light) render_colour_frames(o, r);
  HIP_CHECK(hipEventRecord(r.e1, nullptr));
  HIP_CHECK(hipEventSynchronize(r.e1));
  HIP_CHECK(hipEventElapsedTime(&r.ms, r.e0, r.e1));
  HIP_CHECK(hipMemcpy(&r.count, r.d_count, sizeof r.count, hipMemcpyDeviceToHost));
  // --light-gpus: the ranks counted and timed the frames
  if (r.shards_ms >= 0.0) r.ms = static_cast<float>(r.shards_ms), r.count += r.shards_count;
}

// --denoise / --light-denoise, one section: <name>_dn / <name>_ldn, the picture to look at. The final frame filtered
// along the primary hits of its camera pose (one G-buffer per pose and section; --reproject: the temporal object
// already holds it), or the light accumulator filtered along them with each pixel's own standard error as the
// luminance tolerance and tone-mapped once. d_frame and d_light are only read. d_gbuf and d_dn stay for --window.
void filtered_frame(const Options& o, Run& r, const Section& s, rt4_gbuffer_px*& d_gbuf, void*& d_dn) {
  const int32_t format = o.format, px = o.px();
  const bool of_light = o.light_denoise_levels >= 0;
  d_gbuf = device_alloc<rt4_gbuffer_px>(s.pixels());
  d_dn = device_alloc<unsigned char>(s.frame_bytes(px));
  const rt4_region reg = s.region();
  if (!o.reproject) RT4_CHECK(rt4_render_gbuffer_device(r.ctx, &s.last_u, &reg, d_gbuf, s.w, nullptr, err, sizeof err));
  if (of_light) {
    rt4_light_denoise_params lp = defaults(rt4_light_denoise_params_default);
    lp.levels = o.light_denoise_levels;
    RT4_CHECK(rt4_light_denoise_device(r.ctx, s.d_light, s.w, d_gbuf, s.w, s.tone(), &lp, d_dn, format, s.w, nullptr, 0, s.w, s.h,
                                       nullptr, err, sizeof err));
  } else {
    rt4_denoise_params dp = defaults(rt4_denoise_params_default);
    dp.levels = o.denoise_levels;
    RT4_CHECK(rt4_denoise_device(r.ctx, s.d_frame, s.w, d_dn, s.w, format, s.w, s.h,
                                 o.reproject ? rt4_temporal_gbuffer(s.temporal) : d_gbuf, s.w, &dp, nullptr, err, sizeof err));
  }
  HIP_CHECK(hipDeviceSynchronize());
  const std::vector<unsigned char> dn = device_read<unsigned char>(d_dn, s.frame_bytes(px));
  const int levels = of_light ? o.light_denoise_levels : o.denoise_levels;
  write_image(o, s.name, of_light ? "_ldn" : "_dn", dn.data(), dn.size(), format, s.w, s.h, true,
              ", " + std::to_string(levels) + (of_light ? " light filter levels" : " filter levels"));
}

// --window, one section: <name>_win, what the reference's window shows: the cell image (d_dn, the filtered one, if
// there is one) stretched over cells * scale pixels, interpolated along the window pixels' own primary hits unless
// --window-nearest. A cell G-buffer of the last pose that already exists is passed on (the temporal one with
// --reproject, else d_gbuf when a filter ran); otherwise the window renders its own.
void window_image(const Options& o, Run& r, const Section& s, const rt4_gbuffer_px* d_gbuf, const void* d_dn) {
  const int32_t sc = s.win_scale, ww = s.w * sc, wh = s.h * sc, format = o.format;
  rt4_window* win = nullptr;
  RT4_CHECK(rt4_window_create(r.ctx, s.w, s.h, sc, format, &win, err, sizeof err));
  rt4_upscale_params up = defaults(rt4_upscale_params_default);
  if (o.window_nearest) up.mode = RT4_UPSCALE_NEAREST;
  const rt4_gbuffer_px* d_cells = o.reproject ? rt4_temporal_gbuffer(s.temporal) : d_dn ? d_gbuf : nullptr;
  RT4_CHECK(rt4_window_present_device(win, &s.last_u, d_dn ? d_dn : s.d_frame, s.w, d_cells, s.w, &up, nullptr, err, sizeof err));
  std::vector<unsigned char> wimg(static_cast<size_t>(ww) * wh * o.px());
  RT4_CHECK(rt4_window_read_host(win, wimg.data(), nullptr, err, sizeof err));
  write_image(o, s.name, "_win", wimg.data(), wimg.size(), format, ww, wh, true,
              ", scale " + std::to_string(sc) + (o.window_nearest ? ", nearest" : ", guided"));
  rt4_window_destroy(win);
}

// --light, one section: with --raw the accumulator's bytes, from the main section --light-checkpoint (the accumulator
// with what a resume or a pool must know), the error estimate (the statistics and, with --noise-map, the display
// error q as grey) and, with --adaptive, where the frames went: min / median / max of n, and n over the largest as grey.
void light_outputs(const Options& o, Run& r, const Section& s) {
  const size_t npx = s.pixels();
  const bool checkpoint = s.id == RT4_SECTION_YXZ && !o.light_checkpoint_path.empty();
  std::vector<rt4_light_px> acc;
  if (o.raw || checkpoint || o.adaptive) acc = device_read<rt4_light_px>(s.d_light, npx);
  if (o.raw) write_raw(o.out + "_" + s.name + "_light.raw", acc.data(), npx * sizeof(rt4_light_px));
  if (checkpoint) {
    // with --supersample the fine accumulator, so that a resume continues the bytes the frames fold into
    const std::vector<rt4_light_px> fine = s.d_fine ? device_read<rt4_light_px>(s.d_fine, s.fine_pixels()) : std::vector<rt4_light_px>();
    RT4_CHECK(rt4_light_save(o.light_checkpoint_path.c_str(), s.d_fine ? fine.data() : acc.data(), s.fw, s.fh, s.fw, r.light_issued,
                             o.pool() ? r.pool_seed : o.seed, o.pool() ? r.pool_key : r.run_key, o.pool() ? RT4_LIGHT_POOLED : 0u,
                             err, sizeof err));
    std::printf("light checkpoint %s (frames issued %lld%s)\n", o.light_checkpoint_path.c_str(),
                static_cast<long long>(r.light_issued), o.pool() ? ", pooled" : "");
  }
  float* d_q = o.noise_map ? device_alloc<float>(npx) : nullptr;
  rt4_noise_stats* d_stats = device_alloc<rt4_noise_stats>(1);
  RT4_CHECK(rt4_light_noise_device(r.ctx, s.d_light, s.w, s.w, s.h, s.tone(), o.noise_threshold, nullptr, d_q, s.w, nullptr,
                                   d_stats, nullptr, err, sizeof err));
  HIP_CHECK(hipDeviceSynchronize());
  const rt4_noise_stats ns = device_read<rt4_noise_stats>(d_stats, 1)[0];
  if (o.noise_map) {
    std::vector<float> qv = device_read<float>(d_q, npx);
    for (float& v : qv)  // the writers clamp to [0, 1]: an unmeasured pixel (+inf) is white; NaN black
      if (std::isnan(v)) v = 0.0f;
    write_image(o, s.name, "_q", grey_image(qv).data(), 0, RT4_FRAME_RGBA32F, s.w, s.h, false, ", display error q");
    (void)hipFree(d_q);
  }
  (void)hipFree(d_stats);
  std::printf("noise %s: pixels %llu, measured %llu, above %llu (threshold %.6g), max_q %.6g, max_se %.6g\n", s.name,
              static_cast<unsigned long long>(ns.pixels), static_cast<unsigned long long>(ns.measured),
              static_cast<unsigned long long>(ns.above), static_cast<double>(o.noise_threshold),
              static_cast<double>(ns.max_q), static_cast<double>(ns.max_se));
  if (!o.adaptive) return;
  std::vector<int32_t> sorted(npx);
  for (size_t p = 0; p < npx; p++) sorted[p] = acc[p].n;
  std::sort(sorted.begin(), sorted.end());
  const int32_t n_max = sorted.back();
  std::vector<float> share(npx);
  for (size_t p = 0; p < npx; p++) share[p] = n_max > 0 ? static_cast<float>(acc[p].n) / static_cast<float>(n_max) : 0.0f;
  write_image(o, s.name, "_n", grey_image(share).data(), 0, RT4_FRAME_RGBA32F, s.w, s.h, false, ", frames per pixel");
  std::printf("adaptive %s: n min %d, median %d, max %d\n", s.name, sorted.front(), sorted[npx / 2], n_max);
}

// Step 4, one section: its image; next to it the filtered frame and the window image (which share d_gbuf and d_dn);
// the light path's statistics, maps and checkpoint; from the main section --checkpoint.
void write_section_outputs(const Options& o, Run& r, const Section& s) {
  const std::vector<unsigned char> host = device_read<unsigned char>(s.d_frame, s.frame_bytes(o.px()));
  write_image(o, s.name, "", host.data(), host.size(), o.format, s.w, s.h, true, "");
  rt4_gbuffer_px* d_gbuf = nullptr;  // the G-buffer of the last pose and the filtered frame
  void* d_dn = nullptr;
  if ((o.denoise_levels > 0 || o.light_denoise_levels >= 0) && o.frames >= 1) filtered_frame(o, r, s, d_gbuf, d_dn);
  if (o.window_scale != 0 && o.frames >= 1) window_image(o, r, s, d_gbuf, d_dn);
  if (d_gbuf) (void)hipFree(d_gbuf);
  if (d_dn) (void)hipFree(d_dn);
  if (o.light) light_outputs(o, r, s);
  if (s.id == RT4_SECTION_YXZ && !o.checkpoint_path.empty()) {
    // frames_done counts camera-resting frames only: a moving camera restarts the blend (frame_number 1)
    const long long rested = static_cast<long long>(r.cam.frame_number) - 1;
    RT4_CHECK(rt4_accum_save_key(o.checkpoint_path.c_str(), host.data(), o.format, s.w, s.h, s.w, rested, o.seed, r.run_key, err,
                                 sizeof err));
    std::printf("checkpoint %s (%lld frames)\n", o.checkpoint_path.c_str(), rested);
  }
}

// --retina: the whole run on one GPU. The -n frames into the D-slice volume of the main section's view, then one
// projection per picture: every picture after the first costs no tracing.
void run_retina(const Options& o, Run& r) {
  const Section& s = r.sections[0];
  int32_t scale = 1;
  RT4_CHECK(rt4_properties_get_int(r.props, "window.main.cell_size", &scale, err, sizeof err));
  if (scale < 1 || s.w > 65535 / scale || s.h > 65535 / scale) die("--retina", "the window's pixel size is not in [1, 65535]");
  const int32_t ow = s.w * scale, oh = s.h * scale;
  rt4_uniforms u;
  RT4_CHECK(rt4_camera_frame_uniforms(&r.cam, &s.base, s.id, static_cast<int32_t>(o.seed), &u));
  const float depth_size = o.retina_size > 0.0f ? o.retina_size : u.mtr_sizes[1];
  const float size[3] = {u.mtr_sizes[0], u.mtr_sizes[1], depth_size};
  const float rad = 3.14159265358979323846f / 180.0f;
  const int n_views = std::max(o.retina_turntable, 1);
  std::vector<rt4_retina_view> views(static_cast<size_t>(n_views));
  for (int v = 0; v < n_views; v++) {  // before any HIP call: a step too small for the box is refused here
    const float yaw = o.retina_turntable > 0 ? 360.0f * static_cast<float>(v) / static_cast<float>(n_views) : o.retina_yaw;
    RT4_CHECK(rt4_retina_view_make(s.w, s.h, o.retina_depth, size, yaw * rad, o.retina_pitch * rad, 0.0f, ow, oh, o.retina_step,
                                   &views[static_cast<size_t>(v)], err, sizeof err));
  }
  RT4_CHECK(rt4_context_create(o.device, RT4_FLAG_SAMPLER_LUT, &r.ctx, err, sizeof err));
  RT4_CHECK(rt4_context_set_scene(r.ctx, r.scene, err, sizeof err));
  rt4_retina* ret = nullptr;
  RT4_CHECK(rt4_retina_create(r.ctx, s.w, s.h, o.retina_depth, &ret, err, sizeof err));
  r.d_count = device_alloc<unsigned long long>(1, true);
  void* d_frame = device_alloc<unsigned char>(static_cast<size_t>(ow) * oh * o.px());
  HIP_CHECK(hipEventCreate(&r.e0));
  HIP_CHECK(hipEventCreate(&r.e1));
  HIP_CHECK(hipEventRecord(r.e0, nullptr));
  RT4_CHECK(rt4_retina_accumulate_device(ret, &u, r.cam.orientation.w_drct, depth_size, o.frames, r.d_count, nullptr, err, sizeof err));
  HIP_CHECK(hipEventRecord(r.e1, nullptr));
  HIP_CHECK(hipEventSynchronize(r.e1));
  HIP_CHECK(hipEventElapsedTime(&r.ms, r.e0, r.e1));
  HIP_CHECK(hipMemcpy(&r.count, r.d_count, sizeof r.count, hipMemcpyDeviceToHost));
  for (int v = 0; v < n_views; v++) {
    RT4_CHECK(rt4_retina_present_device(ret, &views[static_cast<size_t>(v)], nullptr, s.tone(), d_frame, o.format, ow, ow, oh,
                                        nullptr, err, sizeof err));
    HIP_CHECK(hipDeviceSynchronize());
    const std::vector<unsigned char> host = device_read<unsigned char>(d_frame, static_cast<size_t>(ow) * oh * o.px());
    char suffix[32] = "_retina";
    if (o.retina_turntable > 0) std::snprintf(suffix, sizeof suffix, "_retina_%03d", v);
    write_image(o, s.name, suffix, host.data(), host.size(), o.format, ow, oh, true,
                ", " + std::to_string(o.retina_depth) + " slices, " + std::to_string(views[static_cast<size_t>(v)].steps) + " steps");
  }
  print_summary("retina " + std::to_string(o.retina_depth) + " slices, ", o.frames, static_cast<size_t>(n_views), r.count,
                r.ms / o.frames, r.ms);
  (void)hipFree(d_frame);
  (void)hipFree(r.d_count);
  rt4_retina_destroy(ret);
  rt4_context_destroy(r.ctx);
}

// Step 5 on one GPU: the summary, and the device state released.
void close_render(const Options& o, Run& r) {
  if (o.pool())
    std::printf("pooled %zu light checkpoints, images 1\n", o.light_pool.size());
  else
    print_summary(o.light_gpus > 0 ? "light gpus " + std::to_string(o.light_gpus) + " (" + o.light_split + "), " : "", o.frames,
                  r.sections.size(), r.count, r.ms / o.frames, r.ms);
  for (Section& s : r.sections) {
    rt4_temporal_destroy(s.temporal);
    if (s.d_light) (void)hipFree(s.d_light);
    if (s.d_fine) (void)hipFree(s.d_fine);
    (void)hipFree(s.d_frame);
  }
  (void)hipFree(r.d_count);
  rt4_context_destroy(r.ctx);
}

}  // namespace

// The steps: options, refusals, inputs, then either the --gpus run or, on one GPU, device state,
// frames, every section's outputs and the summary.
int main(int argc, char** argv) {
  // The frame loop's overlapped launches of small frames use up to 8 side streams: give the
  // process 8 hardware queues unless the environment says otherwise (read when the HIP runtime starts).
  setenv("GPU_MAX_HW_QUEUES", "8", 0);
  const Options o = parse_args(argc, argv);
  refuse_conflicts(o);
  const ShardHooks hooks = shard_hooks(o.rehearse);
  Run r = load_inputs(o);
  if (o.light_gpus > 0 && !o.rehearse) need_devices("--light-gpus", o.light_gpus);
  window_scales(o, r);
  if (o.gpus > 0 && !o.rehearse) need_devices("--gpus", o.gpus);
  if (o.retina) {
    run_retina(o, r);
  } else if (o.gpus > 0) {
    run_bands(o, hooks, r);
  } else {
    open_render(o, r);
    if (o.pipelined()) pipelined_frames(o, r);
    if (o.light) open_light(o, r);
    render_frames(o, hooks, r);
    for (const Section& s : r.sections) write_section_outputs(o, r, s);
    close_render(o, r);
  }
  rt4_properties_free(r.props);
  std::free(r.scene);
  return 0;
}

