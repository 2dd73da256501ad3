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
std::vector<unsigned char> render_shards(int gpus, const rt4_scene_desc* scene, const ShardJob& job, bool rehearse,
                                         int fail_rank, bool fail_gather, unsigned long long* count_out, double* ms_out) {
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
  *count_out = count;
  *ms_out = ms;
  return image;
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
std::vector<unsigned char> render_bands(int gpus, int band, const rt4_scene_desc* scene, const std::vector<rt4_uniforms>& us,
                                        int32_t w, int32_t h, int32_t format, bool frame_by_frame, bool rehearse,
                                        int fail_rank, bool fail_gather, unsigned long long* count_out, double* ms_out) {
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
  return render_shards(gpus, scene, job, rehearse, fail_rank, fail_gather, count_out, ms_out);
}

// --light-gpus: the light accumulator of one section. bands: the accumulator's pixels in the bands of --gpus, every rank
// all frames of its bands, rt4_light_bands_unpermute_device on the root: bit for bit the one-GPU accumulator. frames:
// every rank the whole image for its block of the frame numbers (rt4_frame_split; a rank without frames leaves its
// shard empty), one rt4_light_merge_device of all ranks' accumulators into the root's empty one: as accurate as the
// one-GPU accumulator, not bit-equal to it. us[n - 1] holds the uniforms of frame n.
std::vector<unsigned char> render_light_shards(int gpus, bool split_bands, int band, const rt4_scene_desc* scene,
                                               const std::vector<rt4_uniforms>& us, int32_t w, int32_t h, bool rehearse,
                                               int fail_rank, bool fail_gather, unsigned long long* count_out,
                                               double* ms_out) {
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
    return render_shards(gpus, scene, job, rehearse, fail_rank, fail_gather, count_out, ms_out);
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
  return render_shards(gpus, scene, job, rehearse, fail_rank, fail_gather, count_out, ms_out);
}

void write_raw(const std::string& path, const std::vector<unsigned char>& bytes) {  // --raw
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f) die("--raw", path.c_str());
  const bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
  if (std::fclose(f) != 0 || !ok) die("--raw: write failed", path.c_str());
}

uint32_t keys_from(const char* s) {  // controls.cpp:98-113 key names
  uint32_t k = 0;
  for (; *s; ++s) switch (*s) {
      case 'W': k |= RT4_KEY_FORWARD; break;
      case 'S': k |= RT4_KEY_BACK; break;
      case 'D': k |= RT4_KEY_RIGHT; break;
      case 'A': k |= RT4_KEY_LEFT; break;
      case ' ': case 'U': k |= RT4_KEY_UP; break;
      case 'L': k |= RT4_KEY_DOWN; break;
      case 'E': k |= RT4_KEY_W_POS; break;
      case 'Q': k |= RT4_KEY_W_NEG; break;
      default: break;
    }
  return k;
}

}  // namespace

int main(int argc, char** argv) {
  // The frame loop's overlapped launches of small frames use up to 8 side streams: give the
  // process 8 hardware queues unless the environment says otherwise (read when the HIP runtime starts).
  setenv("GPU_MAX_HW_QUEUES", "8", 0);
  std::string props_path = "properties.txt", scene_arg, out = "frame", fmt_name = "f32";
  int frames = 1, device = 0, width = 0, height = 0;
  bool three = false, frame_by_frame = false;
  int gpus = 0, band = 8;
  uint32_t seed = 12345, keys = 0;
  float move_seconds = 0.0f;
  std::string resume_path, checkpoint_path;
  bool png = false, rehearse = false, raw = false;
  int denoise_levels = 0;  // --denoise: 0 = off
  int light_denoise_levels = -1;  // --light-denoise: -1 = off
  bool reproject = false;
  int window_scale = 0;  // --window: 0 = off, -1 = the properties' cell_size
  bool window_nearest = false;
  bool light = false, noise_map = false;  // --light, --noise-map
  float noise_threshold = 1.0f / 255.0f;  // --noise-threshold: one 8-bit step
  // --adaptive (needs --light): the loop of DESIGN.md §4.39 in place of -n uniform frames; -n is then the budget in
  // whole-frame equivalents. The defaults are the values of that section's study.
  bool adaptive = false, ad_given = false;
  int ad_warmup = 8, ad_pass = 4, ad_full_every = 4;  // --adaptive-warmup / --adaptive-pass / --adaptive-full-every
  rt4_tile_select_params ad_select;                   // --adaptive-min-above / --adaptive-dilate; threshold: --noise-threshold
  rt4_tile_select_params_default(&ad_select);
  // --light-resume / --light-checkpoint / --light-gpus / --light-pool: the light path's own restart,
  // multi-GPU and pooling flags; --resume, --checkpoint and --gpus stay the colour path's
  std::string light_resume_path, light_checkpoint_path, light_split = "frames";
  bool light_split_given = false;
  int light_gpus = 0;
  std::vector<std::string> light_pool;
  for (int i = 1; i < argc; i++) {
    const std::string a = argv[i];
    auto next = [&]() -> const char* {
      if (i + 1 >= argc) die("missing value for", a.c_str());
      return argv[++i];
    };
    if (a == "-p") props_path = next();
    else if (a == "-s") scene_arg = next();
    else if (a == "-n") frames = std::atoi(next());
    else if (a == "-3") three = true;
    else if (a == "-W") width = std::atoi(next());
    else if (a == "-H") height = std::atoi(next());
    else if (a == "-f") fmt_name = next();
    else if (a == "--seed") seed = static_cast<uint32_t>(std::strtoul(next(), nullptr, 0));
    else if (a == "-o") out = next();
    else if (a == "-d") device = std::atoi(next());
    else if (a == "--keys") keys = keys_from(next());
    else if (a == "--frame-by-frame") frame_by_frame = true;
    else if (a == "--move-seconds") move_seconds = static_cast<float>(std::atof(next()));
    else if (a == "--gpus") gpus = std::atoi(next());
    else if (a == "--band") band = std::atoi(next());
    else if (a == "--resume") resume_path = next();
    else if (a == "--checkpoint") checkpoint_path = next();
    else if (a == "--png") png = true;
    else if (a == "--raw") raw = true;
    else if (a == "--rehearse") rehearse = true;
    else if (a == "--reproject") reproject = true;
    else if (a == "--light") light = true;
    else if (a == "--noise-map") noise_map = true;
    else if (a == "--noise-threshold") noise_threshold = static_cast<float>(std::atof(next()));
    else if (a == "--light-resume") light_resume_path = next();
    else if (a == "--light-checkpoint") light_checkpoint_path = next();
    else if (a == "--light-gpus") light_gpus = std::atoi(next());
    else if (a == "--light-split") light_split = next(), light_split_given = true;
    else if (a == "--light-pool") {  // every following argument up to the next flag
      while (i + 1 < argc && argv[i + 1][0] != '-') light_pool.push_back(argv[++i]);
      if (light_pool.size() < 2) die("--light-pool", "needs two or more light checkpoints");
      light = true;
    }
    else if (a == "--adaptive") adaptive = true;
    else if (a == "--adaptive-warmup") ad_warmup = std::atoi(next()), ad_given = true;
    else if (a == "--adaptive-pass") ad_pass = std::atoi(next()), ad_given = true;
    else if (a == "--adaptive-full-every") ad_full_every = std::atoi(next()), ad_given = true;
    else if (a == "--adaptive-min-above") ad_select.min_above = std::atoi(next()), ad_given = true;
    else if (a == "--adaptive-dilate") ad_select.dilate = std::atoi(next()), ad_given = true;
    else if (a == "--window-nearest") {
      window_nearest = true;
      if (window_scale == 0) window_scale = -1;
    }
    else if (a == "--window") {
      window_scale = -1;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') {
        window_scale = std::atoi(argv[++i]);
        if (window_scale < 1 || window_scale > RT4_UPSCALE_MAX_SCALE) die("--window", "SCALE must be 1..64");
      }
    }
    else if (a == "--denoise") {
      rt4_denoise_params dp;
      rt4_denoise_params_default(&dp);
      denoise_levels = dp.levels;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') denoise_levels = std::atoi(argv[++i]);
      if (denoise_levels < 1 || denoise_levels > RT4_DENOISE_MAX_LEVELS) die("--denoise", "levels must be 1..6");
    }
    else if (a == "--light-denoise") {
      rt4_light_denoise_params lp;
      rt4_light_denoise_params_default(&lp);
      light_denoise_levels = lp.levels;
      if (i + 1 < argc && argv[i + 1][0] >= '0' && argv[i + 1][0] <= '9') light_denoise_levels = std::atoi(argv[++i]);
      if (light_denoise_levels < 0 || light_denoise_levels > RT4_LIGHT_DENOISE_MAX_LEVELS)
        die("--light-denoise", "levels must be 0..6");
    }
    else die("unknown argument", a.c_str());
  }
  if (reproject && gpus > 0) die("--reproject", "not with --gpus: the temporal image lives on one GPU");
  if (reproject && (!resume_path.empty() || !checkpoint_path.empty()))
    die("--reproject", "not with --resume / --checkpoint: a checkpoint holds no per-pixel history");
  if (reproject && frame_by_frame) die("--reproject", "not with --frame-by-frame: every temporal frame is a launch of its own");
  if (light && reproject) die("--light", "not with --reproject: the temporal history is a colour average");
  if (light && (!resume_path.empty() || !checkpoint_path.empty()))
    die("--light", "not with --resume / --checkpoint: a checkpoint holds colours, not a light accumulator "
                   "(--light-resume / --light-checkpoint save and continue a light accumulator)");
  if (light && gpus > 0)
    die("--light", "not with --gpus: that gathers colour frames (--light-gpus N runs a light accumulator on N GPUs)");
  const bool pool = !light_pool.empty();
  if ((!light_resume_path.empty() || !light_checkpoint_path.empty() || light_gpus != 0 || light_split_given) && !light)
    die("--light-resume / --light-checkpoint / --light-gpus / --light-split", "need --light");
  if (light_split_given && light_gpus == 0) die("--light-split", "needs --light-gpus");
  if (light_split != "frames" && light_split != "bands") die("--light-split", "frames or bands");
  if (light_gpus != 0 && (light_gpus < 1 || light_gpus > RT4_LIGHT_MERGE_MAX))
    die("--light-gpus", "N must be 1..16 (RT4_LIGHT_MERGE_MAX: one merge takes that many accumulators)");
  if (light_gpus > 0 && adaptive) die("--light-gpus", "not with --adaptive: the tile selection runs on one GPU");
  if (light_gpus > 0 && !light_resume_path.empty()) die("--light-gpus", "not with --light-resume: resume on one GPU");
  if (!light_resume_path.empty() && adaptive)
    die("--light-resume", "not with --adaptive: a light checkpoint does not hold the adaptive loop's pass state");
  if (pool && (adaptive || light_gpus > 0 || !light_resume_path.empty() || three || denoise_levels > 0 ||
               light_denoise_levels >= 0 || window_scale != 0 || reproject))
    die("--light-pool", "renders nothing: only with -o, --png, --raw, --noise-map, --noise-threshold, --light-checkpoint");
  if (light && frame_by_frame) die("--light", "not with --frame-by-frame: the frames go through rt4_render_light_device");
  if (light && keys && move_seconds > 0.0f) die("--light", "needs a resting camera: the accumulator averages one view");
  if ((noise_map || noise_threshold != 1.0f / 255.0f) && !light) die("--noise-map / --noise-threshold", "need --light");
  if ((adaptive || ad_given) && !light) die("--adaptive", "needs --light: it samples by the light accumulator's standard error");
  if (ad_given && !adaptive) die("--adaptive-*", "need --adaptive");
  if (adaptive && (ad_warmup < 0 || ad_pass < 1 || ad_full_every < 0 || ad_select.min_above < 1 || ad_select.min_above > 64 ||
                   ad_select.dilate < 0 || ad_select.dilate > RT4_SELECT_MAX_DILATE || noise_threshold != noise_threshold))
    die("--adaptive", "warmup >= 0, pass >= 1, full-every >= 0, min-above 1..64, dilate 0..2, a threshold that is a number");
  if (light_denoise_levels >= 0 && !light) die("--light-denoise", "needs --light: it filters the light accumulator");
  if (light_denoise_levels >= 0 && denoise_levels > 0)
    die("--light-denoise", "not with --denoise: one filtered frame per image");
  const int32_t format = fmt_name == "f16" ? RT4_FRAME_RGBA16F : fmt_name == "rgba8" ? RT4_FRAME_RGBA8 : RT4_FRAME_RGBA32F;
  char err[1024] = {0};
  rt4_properties* props = nullptr;
  RT4_CHECK(rt4_properties_load(props_path.c_str(), &props, err, sizeof err));

  // scene: -s builtin name or .frag path; else the properties' shader_filename (main.cpp:26)
  rt4_scene_desc* scene = static_cast<rt4_scene_desc*>(std::calloc(1, sizeof(rt4_scene_desc)));
  if (scene_arg.empty()) {
    char buf[4096];
    size_t need = 0;
    RT4_CHECK(rt4_properties_get_string(props, "shader_filename", buf, sizeof buf, &need, err, sizeof err));
    scene_arg = buf;
  }
  if (scene_arg.size() > 5 && scene_arg.compare(scene_arg.size() - 5, 5, ".frag") == 0)
    RT4_CHECK(rt4_scene_load_frag(scene_arg.c_str(), scene, err, sizeof err));
  else
    RT4_CHECK(rt4_scene_builtin(scene_arg.c_str(), scene, err, sizeof err));

  // images: the main section (window.main cells, or -W/-H) and, with -3, YWZ / YXW (window.additional)
  const int n_img = three ? 3 : 1;
  int32_t cw[3], ch[3];
  if (width > 0 && height > 0) {
    cw[0] = width;
    ch[0] = height;
  } else {
    RT4_CHECK(rt4_window_cells(props, "main", &cw[0], &ch[0], err, sizeof err));
  }
  if (three) {
    RT4_CHECK(rt4_window_cells(props, "additional", &cw[1], &ch[1], err, sizeof err));
    cw[2] = cw[1];
    ch[2] = ch[1];
  }
  const int sections[3] = {RT4_SECTION_YXZ, RT4_SECTION_YWZ, RT4_SECTION_YXW};
  rt4_uniforms base[3];
  for (int q = 0; q < n_img; q++)
    RT4_CHECK(rt4_uniforms_from_properties(props, cw[q], ch[q], sections[q], &base[q], nullptr, err, sizeof err));
  rt4_camera cam;
  RT4_CHECK(rt4_camera_init(props, &cam, err, sizeof err));

  // the run's key, checked on --resume and recorded by --checkpoint: the first frame's uniforms (seed and
  // part aside they are every resting frame's)
  uint32_t run_key = 0;
  {
    rt4_camera c0 = cam;
    rt4_uniforms u0;
    RT4_CHECK(rt4_camera_frame_uniforms(&c0, &base[0], sections[0], 0, &u0));
    run_key = rt4_accum_key(scene, &u0);
  }
  if ((!resume_path.empty() || !checkpoint_path.empty()) && (three || gpus > 0))
    die("--resume/--checkpoint", "need one section on one GPU");
  // frames already blended into the accumulator (a resumed run continues at frame frames_done + 1)
  int64_t frames_done = 0;
  std::vector<unsigned char> resumed;
  if (!resume_path.empty()) {
    uint32_t ck_seed = 0;
    resumed.resize(static_cast<size_t>(cw[0]) * ch[0] * rt4_frame_format_bytes(format));
    RT4_CHECK(rt4_accum_load(resume_path.c_str(), resumed.data(), format, cw[0], ch[0], cw[0], &frames_done, &ck_seed, err,
                             sizeof err));
    if (ck_seed != seed) die("--resume", "the checkpoint was made with another --seed");
    // the checkpoint's run key (scene, samples, bounces, resolution, camera ...): a checkpoint of
    // another run would be blended in silently
    uint32_t ck_key = 0;
    RT4_CHECK(rt4_accum_key_of(resume_path.c_str(), &ck_key, err, sizeof err));
    if (ck_key != 0u && ck_key != run_key)
      die("--resume", "the checkpoint was made with another scene, properties or camera");
    cam.frame_number = static_cast<uint32_t>(frames_done + 1);
  }
  // --light-resume: the accumulator the run continues (frames frames_done + 1 ...); --light-pool: the accumulators of
  // independent runs, merged once there is a context. Both are refused rather than mixed with another run's frames.
  if ((!light_resume_path.empty() || !light_checkpoint_path.empty()) && three)
    die("--light-resume / --light-checkpoint", "need one section");
  std::vector<rt4_light_px> light_start;  // --light-resume: the loaded accumulator; --light-pool: every file's, in order
  uint32_t pool_seed = 0, pool_key = 0;
  int64_t pool_issued = 0;
  if (!light_resume_path.empty()) {
    uint32_t ck_seed = 0, ck_key = 0, ck_flags = 0;
    int32_t ck_w = 0, ck_h = 0;
    RT4_CHECK(rt4_light_info(light_resume_path.c_str(), &ck_w, &ck_h, nullptr, &ck_seed, &ck_key, &ck_flags, err, sizeof err));
    if (ck_flags & RT4_LIGHT_POOLED) die("--light-resume", "the checkpoint pools runs of several seeds: it cannot be resumed");
    if (ck_w != cw[0] || ck_h != ch[0])
      die("--light-resume", ("the checkpoint holds a " + std::to_string(ck_w) + "x" + std::to_string(ck_h) + " accumulator, not " +
                             std::to_string(cw[0]) + "x" + std::to_string(ch[0])).c_str());
    if (ck_seed != seed) die("--light-resume", "the checkpoint was made with another --seed");
    if (ck_key != 0u && ck_key != run_key)
      die("--light-resume", "the checkpoint was made with another scene, properties or camera");
    light_start.resize(static_cast<size_t>(cw[0]) * ch[0]);
    RT4_CHECK(rt4_light_load(light_resume_path.c_str(), light_start.data(), cw[0], ch[0], cw[0], &frames_done, nullptr, nullptr,
                             nullptr, err, sizeof err));
    if (frames_done + frames > 0xFFFFFFFFll) die("--light-resume", "frame numbers beyond 2^32 - 1");
    cam.frame_number = static_cast<uint32_t>(frames_done + 1);
  }
  if (pool) {
    std::vector<uint32_t> seeds;
    for (size_t s = 0; s < light_pool.size(); s++) {
      int32_t fw = 0, fh = 0;
      int64_t issued = 0;
      uint32_t ck_seed = 0, ck_key = 0;
      RT4_CHECK(rt4_light_info(light_pool[s].c_str(), &fw, &fh, &issued, &ck_seed, &ck_key, nullptr, err, sizeof err));
      if (s == 0) {
        cw[0] = fw, ch[0] = fh, pool_seed = ck_seed, pool_key = ck_key, pool_issued = issued;
        light_start.resize(light_pool.size() * static_cast<size_t>(fw) * fh);
      }
      if (fw != cw[0] || fh != ch[0]) die("--light-pool: another image size than the first file's", light_pool[s].c_str());
      if (ck_key != pool_key) die("--light-pool: another scene, properties or camera than the first file's", light_pool[s].c_str());
      if (std::find(seeds.begin(), seeds.end(), ck_seed) != seeds.end())
        die("--light-pool: the same --seed as an earlier file, the same frames would count twice", light_pool[s].c_str());
      seeds.push_back(ck_seed);
      RT4_CHECK(rt4_light_load(light_pool[s].c_str(), light_start.data() + s * static_cast<size_t>(fw) * fh, fw, fh, fw, nullptr,
                               nullptr, nullptr, nullptr, err, sizeof err));
    }
    frames = 0;  // nothing is rendered
  }
  if (light_gpus > 0) {  // as --gpus: one section (the camera rests in every --light run)
    if (three) die("--light-gpus", "needs one section");
    if (frames < 1 || band < 1) die("--light-gpus", "frames and band must be >= 1");
    if (!rehearse) {
      int ndev = 0;
      HIP_CHECK(hipGetDeviceCount(&ndev));
      if (light_gpus > ndev) die("--light-gpus", ("only " + std::to_string(ndev) + " HIP devices").c_str());
    }
  }

  if (gpus > 0 && denoise_levels > 0) die("--denoise", "not with --gpus: the frame is not filtered after the gather");
  if (gpus > 0 && window_scale != 0) die("--window", "not with --gpus: the frame is not upscaled after the gather");
  int32_t win_scale[3] = {window_scale, window_scale, window_scale};  // per section
  if (window_scale < 0) {
    RT4_CHECK(rt4_properties_get_int(props, "window.main.cell_size", &win_scale[0], err, sizeof err));
    if (three) RT4_CHECK(rt4_properties_get_int(props, "window.additional.cell_size", &win_scale[1], err, sizeof err));
    win_scale[2] = win_scale[1];
  }
  if (gpus > 0) {  // pixel bands over GPUs 0..gpus-1, one RCCL gather (one section, resting camera)
    if (three || (keys && move_seconds > 0.0f)) die("--gpus", "needs one section and a resting camera");
    if (frames < 1 || band < 1) die("--gpus", "frames and band must be >= 1");
    if (!rehearse) {  // a rehearsal puts every rank on device 0 and reports a missing device per rank
      int ndev = 0;
      HIP_CHECK(hipGetDeviceCount(&ndev));
      if (gpus > ndev) die("--gpus", ("only " + std::to_string(ndev) + " HIP devices").c_str());
    }
    const char* fail_env = std::getenv("RT4_RENDER_FAIL_RANK");  // test hook: this rank's set-up fails,
    const int fail_rank = fail_env ? std::atoi(fail_env) : -1;
    const char* stage_env = std::getenv("RT4_RENDER_FAIL_STAGE");  // or with "gather" its part of the gather
    const bool fail_gather = stage_env && std::strcmp(stage_env, "gather") == 0;
    std::vector<rt4_uniforms> us;
    for (int n = 1; n <= frames; n++) {
      rt4_uniforms u;
      RT4_CHECK(rt4_camera_frame_uniforms(&cam, &base[0], sections[0],
                                          static_cast<int32_t>(seed ^ (static_cast<uint32_t>(n) * 0x9E3779B9u)), &u));
      us.push_back(u);
    }
    unsigned long long count = 0;
    double ms = 0.0;
    const std::vector<unsigned char> img =
        render_bands(gpus, band, scene, us, cw[0], ch[0], format, frame_by_frame, rehearse, fail_rank, fail_gather, &count,
                     &ms);
    const std::string path = out + (png ? "_yxz.png" : "_yxz.ppm");
    RT4_CHECK((png ? rt4_write_png : rt4_write_ppm)(path.c_str(), img.data(), format, cw[0], ch[0], cw[0], err, sizeof err));
    if (raw) write_raw(out + "_yxz.raw", img);
    std::printf("wrote %s (%d x %d)\n", path.c_str(), cw[0], ch[0]);
    std::printf("gpus %d, frames %d, images 1, intersections %llu, %.3f ms/frame, %.3e intersections/s\n", gpus,
                frames, count, ms / frames, static_cast<double>(count) / (ms * 1e-3));
    rt4_properties_free(props);
    std::free(scene);
    return 0;
  }

  rt4_context* ctx = nullptr;
  RT4_CHECK(rt4_context_create(device, RT4_FLAG_SAMPLER_LUT, &ctx, err, sizeof err));
  RT4_CHECK(rt4_context_set_scene(ctx, scene, err, sizeof err));
  const int32_t px = rt4_frame_format_bytes(format);
  void* d_frame[3] = {nullptr, nullptr, nullptr};
  for (int q = 0; q < n_img; q++) {
    HIP_CHECK(hipMalloc(&d_frame[q], static_cast<size_t>(cw[q]) * ch[q] * px));
    HIP_CHECK(hipMemset(d_frame[q], 0, static_cast<size_t>(cw[q]) * ch[q] * px));  // cleared RenderTexture
  }
  if (!resumed.empty()) HIP_CHECK(hipMemcpy(d_frame[0], resumed.data(), resumed.size(), hipMemcpyHostToDevice));
  unsigned long long* d_count = nullptr;
  HIP_CHECK(hipMalloc(&d_count, sizeof *d_count));
  HIP_CHECK(hipMemset(d_count, 0, sizeof *d_count));
  hipEvent_t e0, e1;
  HIP_CHECK(hipEventCreate(&e0));
  HIP_CHECK(hipEventCreate(&e1));

  // One section and a resting camera (progressive accumulation): the frames go to the library in one
  // rt4_render_frames_device call (pipelined through one pixel queue; the same final image).
  const bool pipelined = n_img == 1 && !(keys && move_seconds > 0.0f) && !frame_by_frame && !reproject && !light;
  rt4_temporal* temporal[3] = {nullptr, nullptr, nullptr};  // --reproject: one per section
  for (int q = 0; q < n_img && reproject; q++)
    RT4_CHECK(rt4_temporal_create(ctx, cw[q], ch[q], format, &temporal[q], err, sizeof err));
  std::vector<rt4_uniforms> us;
  if (pipelined) {
    // the frame-colour scratch only when frames are actually pipelined (>= 2 frames, a scene that does
    // not run frame by frame), and only for the frames of one chunk
    if (frames >= 2 && rt4_context_frames_per_launch(ctx, cw[0], ch[0]) > 1)
      RT4_CHECK(rt4_context_reserve_frames(ctx, cw[0], ch[0], err, sizeof err));
    for (int n = 1; n <= frames; n++) {
      rt4_uniforms u;
      const uint32_t fn = static_cast<uint32_t>(frames_done + n);
      RT4_CHECK(rt4_camera_frame_uniforms(&cam, &base[0], sections[0], static_cast<int32_t>(seed ^ (fn * 0x9E3779B9u)), &u));
      us.push_back(u);
    }
  }
  rt4_uniforms last_u[3];  // the last frame's uniforms of every section: the camera pose the images show
  if (pipelined && !us.empty()) last_u[0] = us.back();
  static const char* names[3] = {"yxz", "ywz", "yxw"};
  rt4_light_px* d_light[3] = {nullptr, nullptr, nullptr};  // --light: one accumulator per section
  for (int q = 0; q < n_img && light; q++) {
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_light[q]), static_cast<size_t>(cw[q]) * ch[q] * sizeof(rt4_light_px)));
    HIP_CHECK(hipMemset(d_light[q], 0, static_cast<size_t>(cw[q]) * ch[q] * sizeof(rt4_light_px)));  // empty
  }
  const size_t light_bytes0 = static_cast<size_t>(cw[0]) * ch[0] * sizeof(rt4_light_px);
  if (!light_resume_path.empty()) HIP_CHECK(hipMemcpy(d_light[0], light_start.data(), light_bytes0, hipMemcpyHostToDevice));
  if (pool) {
    // the files merged in order into an empty accumulator, RT4_LIGHT_MERGE_MAX of them per call
    std::vector<rt4_light_px> merged(static_cast<size_t>(cw[0]) * ch[0]);
    std::memset(merged.data(), 0, light_bytes0);
    const int64_t plane = static_cast<int64_t>(cw[0]) * ch[0];
    for (size_t s0 = 0; s0 < light_pool.size(); s0 += RT4_LIGHT_MERGE_MAX)
      RT4_CHECK(rt4_light_merge_host(ctx, merged.data(), cw[0], light_start.data() + s0 * static_cast<size_t>(plane), cw[0], plane,
                                     static_cast<int32_t>(std::min<size_t>(RT4_LIGHT_MERGE_MAX, light_pool.size() - s0)), cw[0],
                                     ch[0], err, sizeof err));
    HIP_CHECK(hipMemcpy(d_light[0], merged.data(), light_bytes0, hipMemcpyHostToDevice));
    RT4_CHECK(rt4_light_resolve_device(ctx, d_light[0], cw[0], base[0].light_to_color_conversion_coefficient, d_frame[0], format,
                                       cw[0], cw[0], ch[0], nullptr, err, sizeof err));
  }
  // the last progressive frame number folded into the light accumulator: what --light-checkpoint records
  int64_t light_issued = pool ? pool_issued : frames_done + frames;
  double shards_ms = -1.0;  // --light-gpus: the slowest rank's time, in place of the events' below
  unsigned long long shards_count = 0;
  HIP_CHECK(hipEventRecord(e0, nullptr));
  if (light && frames >= 1) {
    // every section's frames in one rt4_render_light_device call (frame n of every section has the same seed, as in
    // the loop below), then the image: the accumulator resolved into the section's frame
    const uint32_t frame_number = cam.frame_number;
    for (int q = 0; q < n_img; q++) {
      std::vector<rt4_uniforms> lus(static_cast<size_t>(frames));
      cam.frame_number = frame_number;
      for (int n = 1; n <= frames; n++)  // frames_done: the frames a --light-resume checkpoint already holds
        RT4_CHECK(rt4_camera_frame_uniforms(&cam, &base[q], sections[q],
                                            static_cast<int32_t>(seed ^ (static_cast<uint32_t>(frames_done + n) * 0x9E3779B9u)),
                                            &lus[static_cast<size_t>(n - 1)]));
      last_u[q] = lus.back();
      const rt4_region reg{0, 0, cw[q], ch[q], 0, 0};
      if (light_gpus > 0) {
        // the accumulator of the section from light_gpus devices; resolve and everything after it run here, on the root's
        // accumulator, as in a one-GPU run
        const char* fail_env = std::getenv("RT4_RENDER_FAIL_RANK");  // the test hooks of --gpus
        const char* stage_env = std::getenv("RT4_RENDER_FAIL_STAGE");
        const std::vector<unsigned char> acc =
            render_light_shards(light_gpus, light_split == "bands", band, scene, lus, cw[q], ch[q], rehearse,
                                fail_env ? std::atoi(fail_env) : -1, stage_env && std::strcmp(stage_env, "gather") == 0,
                                &shards_count, &shards_ms);
        HIP_CHECK(hipSetDevice(device));  // the rank threads chose their own
        HIP_CHECK(hipMemcpy(d_light[q], acc.data(), acc.size(), hipMemcpyHostToDevice));
      } else if (adaptive) {
        // The loop of DESIGN.md §4.39 (Tracer.render_light_adaptive is the same loop): warm-up whole frames, then passes
        // of the selected tiles, every ad_full_every-th pass and a pass with an empty selection a whole frame; frame g is
        // rt4_progressive_uniforms(the section's uniforms with --seed, g), g running on across the passes.
        rt4_uniforms ub;
        cam.frame_number = frame_number;
        RT4_CHECK(rt4_camera_frame_uniforms(&cam, &base[q], sections[q], static_cast<int32_t>(seed), &ub));
        cam.frame_number = frame_number + static_cast<uint32_t>(frames);  // as the uniform frames above left it
        const long long tiles = static_cast<long long>((cw[q] + 7) / 8) * ((ch[q] + 7) / 8);
        const long long budget = static_cast<long long>(frames) * tiles;
        uint32_t *d_tiles = nullptr, *d_n = nullptr;
        HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_tiles), static_cast<size_t>(tiles) * sizeof(uint32_t)));
        HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_n), sizeof(uint32_t)));
        rt4_tile_select_params sel = ad_select;
        sel.threshold = noise_threshold;
        long long spent = 0;
        uint32_t g = 0;
        std::vector<rt4_uniforms> pus;
        auto pass_uniforms = [&](int n) {
          pus.resize(static_cast<size_t>(n));
          for (int f = 0; f < n; f++) rt4_progressive_uniforms(&ub, ++g, &pus[static_cast<size_t>(f)]);
        };
        const int warm = std::min(ad_warmup, frames);
        sel.min_frames = warm;
        if (warm > 0) {
          pass_uniforms(warm);
          RT4_CHECK(rt4_render_light_device(ctx, pus.data(), warm, &reg, d_light[q], cw[q], d_count, nullptr, err, sizeof err));
          spent += warm * tiles;
          std::printf("adaptive %s: warmup tiles %lld frames %d\n", names[q], tiles, warm);
        }
        for (int n_pass = 1;; n_pass++) {
          const char* kind = "full";
          long long listed = tiles;
          if (!(ad_full_every > 0 && n_pass % ad_full_every == 0)) {
            RT4_CHECK(rt4_light_select_tiles_device(ctx, d_light[q], cw[q], cw[q], ch[q], ub.light_to_color_conversion_coefficient,
                                                    &sel, d_tiles, d_n, nullptr, nullptr, err, sizeof err));
            uint32_t n_sel = 0;  // the one 4-byte read of the pass (synchronises)
            HIP_CHECK(hipMemcpy(&n_sel, d_n, sizeof n_sel, hipMemcpyDeviceToHost));
            kind = n_sel == 0 ? "empty" : "tiles";
            if (n_sel != 0) listed = n_sel;
          }
          const int n = static_cast<int>(std::min<long long>(ad_pass, (budget - spent) / listed));
          if (n <= 0) break;
          pass_uniforms(n);
          if (listed == tiles && kind[0] != 't')
            RT4_CHECK(rt4_render_light_device(ctx, pus.data(), n, &reg, d_light[q], cw[q], d_count, nullptr, err, sizeof err));
          else
            RT4_CHECK(rt4_render_light_tiles_device(ctx, pus.data(), n, &reg, d_tiles, static_cast<int32_t>(listed), d_light[q],
                                                    cw[q], d_count, nullptr, err, sizeof err));
          spent += n * listed;
          std::printf("adaptive %s: %s tiles %lld frames %d\n", names[q], kind, listed, n);
        }
        light_issued = g;  // the loop's last frame number, whatever share of the image each frame covered
        HIP_CHECK(hipDeviceSynchronize());
        (void)hipFree(d_tiles);
        (void)hipFree(d_n);
      } else {
        RT4_CHECK(rt4_render_light_device(ctx, lus.data(), frames, &reg, d_light[q], cw[q], d_count, nullptr, err, sizeof err));
      }
      RT4_CHECK(rt4_light_resolve_device(ctx, d_light[q], cw[q], base[q].light_to_color_conversion_coefficient, d_frame[q],
                                         format, cw[q], cw[q], ch[q], nullptr, err, sizeof err));
    }
  }
  if (pipelined) {
    const rt4_region reg{0, 0, cw[0], ch[0], 0, 0};
    RT4_CHECK(rt4_render_frames_device(ctx, us.data(), frames, &reg, d_frame[0], format, cw[0], d_count, nullptr, err,
                                       sizeof err));
  }
  for (int n = 1; n <= frames && !pipelined && !light; n++) {
    const int32_t s_n = static_cast<int32_t>(seed ^ (static_cast<uint32_t>(frames_done + n) * 0x9E3779B9u));
    rt4_section_job jobs[3];
    const uint32_t frame_number = cam.frame_number;
    for (int q = 0; q < n_img; q++) {
      cam.frame_number = frame_number;  // one frame: every section gets the same part
      RT4_CHECK(rt4_camera_frame_uniforms(&cam, &base[q], sections[q], s_n, &jobs[q].u));
      jobs[q].region = rt4_region{0, 0, cw[q], ch[q], 0, 0};
      jobs[q].d_frame = d_frame[q];
      jobs[q].row_stride_px = cw[q];
      last_u[q] = jobs[q].u;
      if (reproject) RT4_CHECK(rt4_temporal_frame_device(temporal[q], &jobs[q].u, nullptr, d_count, nullptr, err, sizeof err));
    }
    if (!reproject) RT4_CHECK(rt4_render_sections_device(ctx, jobs, n_img, format, d_count, nullptr, err, sizeof err));
    if (keys && move_seconds > 0.0f) rt4_camera_move(&cam, keys, move_seconds);  // move(seconds), main.cpp:95-96
  }
  for (int q = 0; q < n_img && reproject; q++)  // the images written are the temporal images
    HIP_CHECK(hipMemcpyAsync(d_frame[q], rt4_temporal_image(temporal[q]), static_cast<size_t>(cw[q]) * ch[q] * px,
                             hipMemcpyDeviceToDevice, nullptr));
  HIP_CHECK(hipEventRecord(e1, nullptr));
  HIP_CHECK(hipEventSynchronize(e1));
  float ms = 0.0f;
  HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
  unsigned long long count = 0;
  HIP_CHECK(hipMemcpy(&count, d_count, sizeof count, hipMemcpyDeviceToHost));
  if (shards_ms >= 0.0) {  // --light-gpus: the ranks counted and timed the frames
    ms = static_cast<float>(shards_ms);
    count += shards_count;
  }

  for (int q = 0; q < n_img; q++) {
    std::vector<unsigned char> host(static_cast<size_t>(cw[q]) * ch[q] * px);
    HIP_CHECK(hipMemcpy(host.data(), d_frame[q], host.size(), hipMemcpyDeviceToHost));
    const std::string path = out + "_" + names[q] + (png ? ".png" : ".ppm");
    RT4_CHECK((png ? rt4_write_png : rt4_write_ppm)(path.c_str(), host.data(), format, cw[q], ch[q], cw[q], err, sizeof err));
    if (raw) write_raw(out + "_" + names[q] + ".raw", host);
    std::printf("wrote %s (%d x %d)\n", path.c_str(), cw[q], ch[q]);
    rt4_gbuffer_px* d_gbuf = nullptr;  // --denoise: the G-buffer of the last pose and the filtered frame
    void* d_dn = nullptr;
    if (denoise_levels > 0 && frames >= 1) {
      // the picture to look at: the final frame filtered along the primary hits of its camera pose (one G-buffer
      // per pose and section); d_frame stays the accumulator
      const size_t npx = static_cast<size_t>(cw[q]) * ch[q];
      HIP_CHECK(hipMalloc(&d_gbuf, npx * sizeof(rt4_gbuffer_px)));
      HIP_CHECK(hipMalloc(&d_dn, npx * px));
      const rt4_region reg{0, 0, cw[q], ch[q], 0, 0};
      rt4_denoise_params dp;
      rt4_denoise_params_default(&dp);
      dp.levels = denoise_levels;
      // --reproject: the temporal object already holds the G-buffer of the last pose
      if (!reproject) RT4_CHECK(rt4_render_gbuffer_device(ctx, &last_u[q], &reg, d_gbuf, cw[q], nullptr, err, sizeof err));
      RT4_CHECK(rt4_denoise_device(ctx, d_frame[q], cw[q], d_dn, cw[q], format, cw[q], ch[q],
                                   reproject ? rt4_temporal_gbuffer(temporal[q]) : d_gbuf, cw[q], &dp, nullptr, err, sizeof err));
      HIP_CHECK(hipDeviceSynchronize());
      std::vector<unsigned char> dn(host.size());
      HIP_CHECK(hipMemcpy(dn.data(), d_dn, dn.size(), hipMemcpyDeviceToHost));
      const std::string dn_path = out + "_" + names[q] + "_dn" + (png ? ".png" : ".ppm");
      RT4_CHECK((png ? rt4_write_png : rt4_write_ppm)(dn_path.c_str(), dn.data(), format, cw[q], ch[q], cw[q], err, sizeof err));
      if (raw) write_raw(out + "_" + names[q] + "_dn.raw", dn);
      std::printf("wrote %s (%d x %d, %d filter levels)\n", dn_path.c_str(), cw[q], ch[q], denoise_levels);
    }
    if (light_denoise_levels >= 0 && frames >= 1) {
      // --light-denoise: the section's light accumulator filtered along the primary hits of its pose, with each
      // pixel's own standard error as the luminance tolerance, and tone-mapped once; the accumulator is only read
      const size_t npx = static_cast<size_t>(cw[q]) * ch[q];
      HIP_CHECK(hipMalloc(&d_gbuf, npx * sizeof(rt4_gbuffer_px)));
      HIP_CHECK(hipMalloc(&d_dn, npx * px));
      const rt4_region reg{0, 0, cw[q], ch[q], 0, 0};
      rt4_light_denoise_params lp;
      rt4_light_denoise_params_default(&lp);
      lp.levels = light_denoise_levels;
      RT4_CHECK(rt4_render_gbuffer_device(ctx, &last_u[q], &reg, d_gbuf, cw[q], nullptr, err, sizeof err));
      RT4_CHECK(rt4_light_denoise_device(ctx, d_light[q], cw[q], d_gbuf, cw[q], base[q].light_to_color_conversion_coefficient,
                                         &lp, d_dn, format, cw[q], nullptr, 0, cw[q], ch[q], nullptr, err, sizeof err));
      HIP_CHECK(hipDeviceSynchronize());
      std::vector<unsigned char> dn(host.size());
      HIP_CHECK(hipMemcpy(dn.data(), d_dn, dn.size(), hipMemcpyDeviceToHost));
      const std::string dn_path = out + "_" + names[q] + "_ldn" + (png ? ".png" : ".ppm");
      RT4_CHECK((png ? rt4_write_png : rt4_write_ppm)(dn_path.c_str(), dn.data(), format, cw[q], ch[q], cw[q], err, sizeof err));
      if (raw) write_raw(out + "_" + names[q] + "_ldn.raw", dn);
      std::printf("wrote %s (%d x %d, %d light filter levels)\n", dn_path.c_str(), cw[q], ch[q], light_denoise_levels);
    }
    if (window_scale != 0 && frames >= 1) {
      // what the reference's window shows: the cell image (filtered, if it was) stretched over cells * scale pixels,
      // interpolated along the window pixels' own primary hits unless --window-nearest
      const int32_t sc = win_scale[q], ww = cw[q] * sc, wh = ch[q] * sc;
      rt4_window* win = nullptr;
      RT4_CHECK(rt4_window_create(ctx, cw[q], ch[q], sc, format, &win, err, sizeof err));
      rt4_upscale_params up;
      rt4_upscale_params_default(&up);
      if (window_nearest) up.mode = RT4_UPSCALE_NEAREST;
      // a cell G-buffer of the last pose that already exists is passed on; otherwise the window renders its own
      const rt4_gbuffer_px* d_gcells = reproject ? rt4_temporal_gbuffer(temporal[q]) : d_dn ? d_gbuf : nullptr;
      RT4_CHECK(rt4_window_present_device(win, &last_u[q], d_dn ? d_dn : d_frame[q], cw[q], d_gcells, cw[q], &up, nullptr, err,
                                          sizeof err));
      std::vector<unsigned char> wimg(static_cast<size_t>(ww) * wh * px);
      RT4_CHECK(rt4_window_read_host(win, wimg.data(), nullptr, err, sizeof err));
      const std::string win_path = out + "_" + names[q] + "_win" + (png ? ".png" : ".ppm");
      RT4_CHECK((png ? rt4_write_png : rt4_write_ppm)(win_path.c_str(), wimg.data(), format, ww, wh, ww, err, sizeof err));
      if (raw) write_raw(out + "_" + names[q] + "_win.raw", wimg);
      std::printf("wrote %s (%d x %d, scale %d, %s)\n", win_path.c_str(), ww, wh, sc, window_nearest ? "nearest" : "guided");
      rt4_window_destroy(win);
    }
    if (d_gbuf) (void)hipFree(d_gbuf);
    if (d_dn) (void)hipFree(d_dn);
    if (light) {
      // the error estimate of the section: its statistics and, with --noise-map, the display error q as grey
      const size_t npx = static_cast<size_t>(cw[q]) * ch[q];
      if (raw || (q == 0 && !light_checkpoint_path.empty())) {
        // --raw: the accumulator's bytes too; --light-checkpoint: the accumulator with what a resume or a pool must know
        std::vector<unsigned char> acc(npx * sizeof(rt4_light_px));
        HIP_CHECK(hipMemcpy(acc.data(), d_light[q], acc.size(), hipMemcpyDeviceToHost));
        if (raw) write_raw(out + "_" + names[q] + "_light.raw", acc);
        if (q == 0 && !light_checkpoint_path.empty()) {
          RT4_CHECK(rt4_light_save(light_checkpoint_path.c_str(), reinterpret_cast<const rt4_light_px*>(acc.data()), cw[0], ch[0],
                                   cw[0], light_issued, pool ? pool_seed : seed, pool ? pool_key : run_key,
                                   pool ? RT4_LIGHT_POOLED : 0u, err, sizeof err));
          std::printf("light checkpoint %s (frames issued %lld%s)\n", light_checkpoint_path.c_str(),
                      static_cast<long long>(light_issued), pool ? ", pooled" : "");
        }
      }
      float* d_q = nullptr;
      rt4_noise_stats* d_stats = nullptr;
      if (noise_map) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_q), npx * sizeof(float)));
      HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_stats), sizeof(rt4_noise_stats)));
      RT4_CHECK(rt4_light_noise_device(ctx, d_light[q], cw[q], cw[q], ch[q], base[q].light_to_color_conversion_coefficient,
                                       noise_threshold, nullptr, d_q, cw[q], nullptr, d_stats, nullptr, err, sizeof err));
      HIP_CHECK(hipDeviceSynchronize());
      rt4_noise_stats ns;
      HIP_CHECK(hipMemcpy(&ns, d_stats, sizeof ns, hipMemcpyDeviceToHost));
      if (noise_map) {
        std::vector<float> qv(npx), grey(npx * 4);
        HIP_CHECK(hipMemcpy(qv.data(), d_q, npx * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t p = 0; p < npx; p++) {  // the writers clamp to [0, 1]: an unmeasured pixel (+inf) is white; NaN black
          const float v = std::isnan(qv[p]) ? 0.0f : qv[p];
          grey[4 * p] = grey[4 * p + 1] = grey[4 * p + 2] = v;
          grey[4 * p + 3] = 1.0f;
        }
        const std::string q_path = out + "_" + names[q] + "_q" + (png ? ".png" : ".ppm");
        RT4_CHECK((png ? rt4_write_png : rt4_write_ppm)(q_path.c_str(), grey.data(), RT4_FRAME_RGBA32F, cw[q], ch[q], cw[q], err,
                                                        sizeof err));
        std::printf("wrote %s (%d x %d, display error q)\n", q_path.c_str(), cw[q], ch[q]);
        (void)hipFree(d_q);
      }
      (void)hipFree(d_stats);
      std::printf("noise %s: pixels %llu, measured %llu, above %llu (threshold %.6g), max_q %.6g, max_se %.6g\n", names[q],
                  static_cast<unsigned long long>(ns.pixels), static_cast<unsigned long long>(ns.measured),
                  static_cast<unsigned long long>(ns.above), static_cast<double>(noise_threshold),
                  static_cast<double>(ns.max_q), static_cast<double>(ns.max_se));
      if (adaptive) {
        // where the frames went: min / median / max of n, and n over the largest n as grey
        std::vector<rt4_light_px> acc(npx);
        HIP_CHECK(hipMemcpy(acc.data(), d_light[q], npx * sizeof(rt4_light_px), hipMemcpyDeviceToHost));
        std::vector<int32_t> nv(npx);
        for (size_t p = 0; p < npx; p++) nv[p] = acc[p].n;
        std::vector<int32_t> sorted = nv;
        std::sort(sorted.begin(), sorted.end());
        const int32_t n_max = sorted.back();
        std::vector<float> grey(npx * 4);
        for (size_t p = 0; p < npx; p++) {
          grey[4 * p] = grey[4 * p + 1] = grey[4 * p + 2] = n_max > 0 ? static_cast<float>(nv[p]) / static_cast<float>(n_max) : 0.0f;
          grey[4 * p + 3] = 1.0f;
        }
        const std::string n_path = out + "_" + names[q] + "_n" + (png ? ".png" : ".ppm");
        RT4_CHECK((png ? rt4_write_png : rt4_write_ppm)(n_path.c_str(), grey.data(), RT4_FRAME_RGBA32F, cw[q], ch[q], cw[q], err,
                                                        sizeof err));
        std::printf("wrote %s (%d x %d, frames per pixel)\n", n_path.c_str(), cw[q], ch[q]);
        std::printf("adaptive %s: n min %d, median %d, max %d\n", names[q], sorted.front(), sorted[npx / 2], n_max);
      }
    }
    if (q == 0 && !checkpoint_path.empty()) {
      // frames_done counts camera-resting frames only: a moving camera restarts the blend (frame_number 1)
      RT4_CHECK(rt4_accum_save_key(checkpoint_path.c_str(), host.data(), format, cw[0], ch[0], cw[0],
                                   static_cast<int64_t>(cam.frame_number) - 1, seed, run_key, err, sizeof err));
      std::printf("checkpoint %s (%lld frames)\n", checkpoint_path.c_str(), static_cast<long long>(cam.frame_number) - 1);
    }
  }
  if (pool)
    std::printf("pooled %zu light checkpoints, images 1\n", light_pool.size());
  else if (light_gpus > 0)
    std::printf("light gpus %d (%s), frames %d, images 1, intersections %llu, %.3f ms/frame, %.3e intersections/s\n", light_gpus,
                light_split.c_str(), frames, count, ms / frames, static_cast<double>(count) / (ms * 1e-3));
  else
    std::printf("frames %d, images %d, intersections %llu, %.3f ms/frame, %.3e intersections/s\n", frames, n_img,
                count, ms / frames, static_cast<double>(count) / (ms * 1e-3));

  for (int q = 0; q < n_img; q++) rt4_temporal_destroy(temporal[q]);
  for (int q = 0; q < n_img; q++)
    if (d_light[q]) (void)hipFree(d_light[q]);
  for (int q = 0; q < n_img; q++) (void)hipFree(d_frame[q]);
  (void)hipFree(d_count);
  rt4_context_destroy(ctx);
  rt4_properties_free(props);
  std::free(scene);
  return 0;
}
