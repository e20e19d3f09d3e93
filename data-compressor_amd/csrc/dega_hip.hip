// dega_hip.hip -- host side of libdega_hip.so: the C ABI declared in include/dega_hip.h.
//
// One context per device: the division table in HBM, pooled hipEvents for the optional kernel timing, and -- for the
// host-pointer entry points -- a pipeline of streams with grow-only device and pinned-host buffers (dega_pipeline.hpp).
// A group (dega_hip_group) is a set of contexts, one host thread per device, channel ranges per device, host-side
// concatenation of the packed streams; no collective.  Built for gfx950 only:
//   hipcc --offload-arch=gfx950 -O3 -shared -fPIC dega_hip.hip -o libdega_hip.so      (see csrc/Makefile)
#include <hip/hip_runtime.h>

#include "../../include/dega_hip.h"
#include "dega_kernels.hpp"
#include "lzmh_kernels.hpp"
#include "aggregate_kernels.hpp"
#include "aggregate_levels_kernels.hpp"
#include "aggregate_var_kernels.hpp"
#include "csv_kernels.hpp"
#include "csv_read_kernels.hpp"
#include "csv_read_split_kernels.hpp"
#include "csv_write_split_kernels.hpp"
#include "transpose_kernels.hpp"
#include "axdr_kernels.hpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

using namespace dg;

struct Pipeline;
static void pipeline_destroy(Pipeline *p);

// A block of device memory between the launches of one call.  The block is shared by all calls on the context, whatever
// their streams: `done` is recorded behind every call's last launch that uses the block, and a call on another stream
// than the last one makes its stream wait for it before its first launch writes the block (on the device; the host never
// waits).  It grows only, by doubling, and a block it has outgrown is kept until the context goes -- freeing would
// synchronise the device; the blocks kept back sum to less than the live one.
struct Scratch
{
  uint8_t *p = nullptr;
  size_t bytes = 0;
  hipEvent_t done = nullptr;    // behind the last call's last launch on the block (nullptr until the first call)
  hipStream_t stream = nullptr; // the stream that call used
  bool pending = false;         // done has been recorded
};

struct dega_hip_ctx
{
  int device;
  uint32_t *div_magic; // device, DIV_TABLE_SIZE entries
  char last_error[256];
  bool profile;
  std::vector<hipEvent_t> ev[4]; // start/stop pairs per kernel kind (0 encode, 1 decode, 2 lzmh encode, 3 lzmh decode)
  std::vector<hipEvent_t> ev_pool; // events handed back by profile_read, reused by the next timed launches
  int force_waves; // 0 = choose by batch size; 4 / 8 = pairs of waves per workgroup, DEGA_WAVES_PER_WORKGROUP (measurement knob)
  Pipeline *pipe;  // streams and buffers of the host-pointer entry points, created on first use
  // `sums`: the aggregated rows between the launches of the level calls; `text`: the text between the launches of
  // dega_hip_lzmh_encode_f32_dev / dega_hip_lzmh_encode_levels_f32_dev / dega_hip_lzmh_decode_f32_dev (in front of it
  // the per-channel status and lengths, TextScratch); `split`: the [C][blocks] counts and first rows between the launches
  // of dega_hip_csv_read_split_dev; `wsplit`: the [C][blocks] lengths and byte offsets between the launches of
  // dega_hip_csv_write_split_dev.  Blocks they have outgrown are kept in `agg_retired`.
  Scratch sums, text, split, wsplit;
  std::vector<void *> agg_retired;
};

static int fail(dega_hip_ctx *ctx, int code, const char *what, hipError_t e)
{
  if (ctx != nullptr)
    snprintf(ctx->last_error, sizeof(ctx->last_error), "%s: %s", what, e == hipSuccess ? "invalid argument" : hipGetErrorString(e));
  return code;
}

#define HIP_TRY(ctx, expr, code)                      \
  do                                                  \
  {                                                   \
    const hipError_t e_ = (expr);                     \
    if (e_ != hipSuccess)                             \
      return fail((ctx), (code), #expr, e_);          \
  } while (0)

// The library's backend of the launch descriptions at the foot of the kernel headers (dega_launch.hpp): the kernel on the
// call's stream.  Every kernel of those headers is launched from here.
struct OnStream
{
  hipStream_t s;
  template <typename A>
  void operator()(void (*kernel)(A), LaunchGrid grid, uint32_t block, const A &a) const
  {
    hipLaunchKernelGGL(kernel, dim3(grid.x, grid.y), dim3(block), 0, s, a);
  }
};

extern "C" int dega_hip_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

extern "C" const char *dega_hip_version(void)
{
  return "dega-hip 0.2 (gfx950)";
}

extern "C" size_t dega_hip_worst_case_bytes(size_t T)
{
  // seg: <= 65 bits per sample (seg.c:18-19).  bac: a coded bit costs at most log2(cum[0]/freq) <= 14 bits in the worst
  // model state, but over a whole stream the adaptive coder stays within a few percent of 1 bit/bit plus the counts'
  // learning cost; the static coder (frequencies 1:1:1) costs log2(3) bits per bit.  2 output bits per seg bit covers both.
  const size_t bits = T * 65 * 2 + 64;
  return ((bits + 7) / 8 + 16 + 3) & ~(size_t)3;
}

extern "C" size_t dega_hip_worst_case_bytes64(size_t T)
{
  const size_t bits = T * 127 * 2 + 64; // as above with the 127-bit worst-case codeword of 64-bit values
  return ((bits + 7) / 8 + 16 + 3) & ~(size_t)3;
}

extern "C" int dega_hip_create(int device, dega_hip_ctx **out)
{
  if (out == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n)
    return DEGA_ERROR_LIBRARY_INIT; // no CPU fallback: fail loudly
  dega_hip_ctx *ctx = new dega_hip_ctx();
  ctx->device = device;
  ctx->div_magic = nullptr;
  ctx->last_error[0] = '\0';
  ctx->profile = false;
  ctx->pipe = nullptr;
  {
    const char *w = getenv("DEGA_WAVES_PER_WORKGROUP");
    const int v = w != nullptr ? atoi(w) : 0;
    ctx->force_waves = (v == 4 || v == 8) ? v : 0;
  }
  if (hipSetDevice(device) != hipSuccess)
  {
    delete ctx;
    return DEGA_ERROR_LIBRARY_INIT;
  }
  std::vector<uint32_t> tab;
  build_div_table(tab);
  if (hipMalloc((void **)&ctx->div_magic, tab.size() * sizeof(uint32_t)) != hipSuccess)
  {
    delete ctx;
    return DEGA_ERROR_MEMORY;
  }
  if (hipMemcpy(ctx->div_magic, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
  {
    (void)hipFree(ctx->div_magic);
    delete ctx;
    return DEGA_ERROR_LIBRARY_INIT;
  }
  *out = ctx;
  return DEGA_OK;
}

extern "C" void dega_hip_destroy(dega_hip_ctx *ctx)
{
  if (ctx == nullptr)
    return;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  pipeline_destroy(ctx->pipe);
  for (int k = 0; k < 4; k++)
    for (hipEvent_t e : ctx->ev[k])
      (void)hipEventDestroy(e);
  for (hipEvent_t e : ctx->ev_pool)
    (void)hipEventDestroy(e);
  (void)hipFree(ctx->div_magic);
  for (Scratch *b : {&ctx->sums, &ctx->text, &ctx->split, &ctx->wsplit})
  {
    if (b->p != nullptr)
      (void)hipFree(b->p);
    if (b->done != nullptr)
      (void)hipEventDestroy(b->done);
  }
  for (void *p : ctx->agg_retired)
    (void)hipFree(p);
  delete ctx;
}

extern "C" const char *dega_hip_last_error(const dega_hip_ctx *ctx)
{
  return ctx == nullptr ? "no context" : ctx->last_error;
}

extern "C" int dega_hip_profile(dega_hip_ctx *ctx, int enable)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  ctx->profile = enable != 0;
  return DEGA_OK;
}

extern "C" int dega_hip_profile_read(dega_hip_ctx *ctx, int which, double *avg_ms, int reset)
{
  if (ctx == nullptr || which < 0 || which > 3 || avg_ms == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  (void)hipSetDevice(ctx->device);
  std::vector<hipEvent_t> &v = ctx->ev[which];
  double sum = 0.0;
  int n = 0;
  for (size_t i = 0; i + 1 < v.size(); i += 2)
  {
    float ms = 0.f;
    if (hipEventSynchronize(v[i + 1]) == hipSuccess && hipEventElapsedTime(&ms, v[i], v[i + 1]) == hipSuccess)
    {
      sum += ms;
      n++;
    }
  }
  *avg_ms = n ? sum / n : 0.0;
  if (reset)
  {
    ctx->ev_pool.insert(ctx->ev_pool.end(), v.begin(), v.end()); // kept for the next timed launches
    v.clear();
  }
  return n;
}

// Brackets a launch with events on the launch's own stream when profiling is on.  Events come from the context's pool;
// a context never holds more than DEGA_MAX_TIMED launches' worth (later launches go untimed until profile_read resets).
constexpr size_t DEGA_MAX_TIMED = 4096;
struct LaunchTimer
{
  dega_hip_ctx *ctx;
  int which;
  hipStream_t s;
  bool armed;
  static bool take(dega_hip_ctx *ctx, hipEvent_t *e)
  {
    if (!ctx->ev_pool.empty())
    {
      *e = ctx->ev_pool.back();
      ctx->ev_pool.pop_back();
      return true;
    }
    return hipEventCreate(e) == hipSuccess;
  }
  LaunchTimer(dega_hip_ctx *c, int w, hipStream_t st) : ctx(c), which(w), s(st), armed(false)
  {
    hipEvent_t e;
    if (ctx->profile && ctx->ev[which].size() < 2 * DEGA_MAX_TIMED && take(ctx, &e))
    {
      (void)hipEventRecord(e, s);
      ctx->ev[which].push_back(e);
      armed = true;
    }
  }
  ~LaunchTimer()
  {
    if (!armed)
      return;
    hipEvent_t e;
    if (take(ctx, &e))
    {
      (void)hipEventRecord(e, s);
      ctx->ev[which].push_back(e);
    }
    else
    {
      ctx->ev_pool.push_back(ctx->ev[which].back());
      ctx->ev[which].pop_back();
    }
  }
};

constexpr size_t DEGA_MAX_T = (size_t)1 << 25; // samples per channel and call: T * 65 seg bits are counted in 32 bits

static int check_shape(dega_hip_ctx *ctx, size_t C, size_t T, size_t ld, size_t cap, int valuesize)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (valuesize < 1 || valuesize > 32)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "valuesize must be 1..32 for the [T][C] int32 layout", hipSuccess);
  if (ld < C)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "ld < C", hipSuccess);
  if (cap % 4 != 0 || cap > ((size_t)1 << 29))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "cap must be a multiple of 4 and at most 512 MiB", hipSuccess);
  if (T > DEGA_MAX_T)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "at most 2^25 samples per channel and call", hipSuccess);
  return DEGA_OK;
}

// ---- kernel dispatch ---------------------------------------------------------------------------------------------------
// One batch: its size and what its samples are (include/dega_hip.h: DEGA_SAMPLES_*)
struct Shape
{
  size_t C, T, ld;
  int adaptive, valuesize, samples;
  float factor;
  bool cmajor = false; // host jobs only: the caller's array is [C][ld], ld >= T (DEGA_SAMPLES_CHANNEL_MAJOR; `samples` holds the type alone)
  const uint64_t *count = nullptr; // host encode jobs only: a HOST array of C counts, one per channel (the launches get device copies as arguments of their own)
};

static int check_job_shape(dega_hip_ctx *ctx, const Shape &j, size_t cap)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  const bool wide = j.valuesize > 32;
  if (j.samples < DEGA_SAMPLES_I32 || j.samples > DEGA_SAMPLES_F32 || j.valuesize < 1 || j.valuesize > 64 ||
      ((j.samples == DEGA_SAMPLES_I32 || j.samples == DEGA_SAMPLES_BE32) && wide) || (j.samples == DEGA_SAMPLES_I64 && !wide))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "sample type and valuesize do not go together (int32 / big-endian: 1..32, int64: 33..64, float32: 1..64)",
                hipSuccess);
  if (j.cmajor && j.ld < j.T)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "ld < T (channel-major samples: ld is the pitch between channels)", hipSuccess);
  return check_shape(ctx, j.C, j.T, j.cmajor ? j.C : j.ld, cap, 32);
}

static int launch_encode(dega_hip_ctx *ctx, const void *x, const Shape &j, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err,
                         hipStream_t s, uint32_t *seg_state = nullptr, uint32_t seg_flags = 0, const uint64_t *count = nullptr, size_t row0 = 0,
                         size_t T_total = 0)
{
  int ret;
  if ((ret = check_job_shape(ctx, j, cap)) != DEGA_OK)
    return ret;
  if (count != nullptr && ((uintptr_t)count & 7u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "encode: count must be a device array of C 64-bit entries, 8-byte aligned", hipSuccess);
  // counts with a segment state: the launch is rows row0 .. row0 + T - 1 of a series of T_total rows
  if (count != nullptr && seg_state != nullptr && (T_total > DEGA_MAX_T || row0 > T_total || j.T > T_total - row0))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "encode segment: row0 + T_seg <= T_total <= 2^25", hipSuccess);
  if (j.C == 0)
    return DEGA_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  const bool f32 = j.samples == DEGA_SAMPLES_F32;
  const EncodeArgs a = encode_args(x, j.C, j.T, j.ld, out, cap, out_bits, err, ctx->div_magic, j.valuesize, j.samples == DEGA_SAMPLES_BE32, j.factor, seg_state,
                                   seg_flags, count, row0, T_total);
  {
    LaunchTimer lt(ctx, 0, s);
    if (!launch(encode_variant(j.C, j.T, seg_state != nullptr, count != nullptr, j.valuesize, f32, j.adaptive != 0), a, OnStream{s}))
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "encode: no kernel for this sample type and valuesize", hipSuccess);
  }
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

static int launch_decode(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, const Shape &j, size_t batch_C, void *x,
                         uint64_t *out_count, int32_t *err, hipStream_t s, uint32_t *rows_done = nullptr, uint32_t band_rows = 0)
{
  int ret;
  if ((ret = check_job_shape(ctx, j, cap)) != DEGA_OK)
    return ret;
  if (j.C == 0)
    return DEGA_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  const bool f32 = j.samples == DEGA_SAMPLES_F32;
  const DecodeArgs a = decode_args(in, cap, in_bits, j.C, j.T, j.ld, x, out_count, err, ctx->div_magic, j.valuesize, j.samples == DEGA_SAMPLES_BE32, j.factor,
                                   rows_done, band_rows);
  {
    LaunchTimer lt(ctx, 1, s);
    if (!launch(decode_variant(batch_C, ctx->force_waves, j.valuesize, f32, j.adaptive != 0), a, OnStream{s}))
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "decode: no kernel for this sample type and valuesize", hipSuccess);
  }
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

static Shape shape_of(size_t C, size_t T, size_t ld, int adaptive, int valuesize, int samples, float factor = 0.0f)
{
  Shape j;
  j.C = C;
  j.T = T;
  j.ld = ld;
  j.adaptive = adaptive;
  j.valuesize = valuesize;
  j.samples = samples;
  j.factor = factor;
  return j;
}

// ---- device-pointer entry points ---------------------------------------------------------------------------------------

extern "C" int dega_hip_encode_dev(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T, size_t ld, int adaptive, int valuesize,
                                   uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream)
{
  int ret;
  if ((ret = check_shape(ctx, C, T, ld, cap, valuesize)) != DEGA_OK)
    return ret;
  return launch_encode(ctx, x_tc, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_I32), out, cap, out_bits, err, (hipStream_t)stream);
}

extern "C" size_t dega_hip_encode_state_bytes(size_t C)
{
  return (size_t)ENC_STATE_WORDS * C * sizeof(uint32_t);
}

extern "C" int dega_hip_encode_segment_dev(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T_seg, size_t ld, int adaptive, int valuesize,
                                           uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *state, unsigned flags, void *stream)
{
  int ret;
  if ((ret = check_shape(ctx, C, T_seg, ld, cap, valuesize)) != DEGA_OK)
    return ret;
  if (state == nullptr || (flags & ~(unsigned)(DEGA_SEGMENT_CONTINUES | DEGA_SEGMENT_MORE)) != 0u || ((uintptr_t)state & 3u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "encode segment: state (device memory, dega_hip_encode_state_bytes) and flags DEGA_SEGMENT_*", hipSuccess);
  static_assert(DEGA_SEGMENT_CONTINUES == ENC_SEG_CONTINUES && DEGA_SEGMENT_MORE == ENC_SEG_MORE, "the flags of the header are the kernel's");
  return launch_encode(ctx, x_tc, shape_of(C, T_seg, ld, adaptive, valuesize, DEGA_SAMPLES_I32), out, cap, out_bits, err, (hipStream_t)stream,
                       (uint32_t *)state, flags);
}

// what the counted integer entry points add to their uniform twins' refusals (check_counts, below, with its `err`)
static int check_counts(dega_hip_ctx *ctx, size_t C, size_t T, const uint64_t *count, uint64_t *const *out_count, size_t K, const int32_t *err);

extern "C" int dega_hip_encode_var_dev(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T, size_t ld, const uint64_t *count, int adaptive,
                                       int valuesize, int samples, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream)
{
  int ret;
  if ((ret = check_shape(ctx, C, T, ld, cap, valuesize)) != DEGA_OK)
    return ret;
  if (samples != DEGA_SAMPLES_I32 && samples != DEGA_SAMPLES_BE32)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "encode: samples must be DEGA_SAMPLES_I32 or DEGA_SAMPLES_BE32", hipSuccess);
  if ((ret = check_counts(ctx, C, T, count, nullptr, 0, err)) != DEGA_OK)
    return ret;
  return launch_encode(ctx, x_tc, shape_of(C, T, ld, adaptive, valuesize, samples), out, cap, out_bits, err, (hipStream_t)stream, nullptr, 0, count);
}

extern "C" int dega_hip_encode_segment_var_dev(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T_seg, size_t ld, const uint64_t *count, size_t row0,
                                               size_t T_total, int adaptive, int valuesize, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err,
                                               void *state, unsigned flags, void *stream)
{
  int ret;
  if ((ret = check_shape(ctx, C, T_seg, ld, cap, valuesize)) != DEGA_OK)
    return ret;
  if (state == nullptr || (flags & ~(unsigned)(DEGA_SEGMENT_CONTINUES | DEGA_SEGMENT_MORE)) != 0u || ((uintptr_t)state & 3u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "encode segment: state (device memory, dega_hip_encode_state_bytes) and flags DEGA_SEGMENT_*", hipSuccess);
  if (T_total > DEGA_MAX_T || row0 > T_total || T_seg > T_total - row0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "encode segment: row0 + T_seg <= T_total <= 2^25", hipSuccess);
  if ((ret = check_counts(ctx, C, T_total, count, nullptr, 0, err)) != DEGA_OK)
    return ret;
  return launch_encode(ctx, x_tc, shape_of(C, T_seg, ld, adaptive, valuesize, DEGA_SAMPLES_I32), out, cap, out_bits, err, (hipStream_t)stream,
                       (uint32_t *)state, flags, count, row0, T_total);
}

extern "C" int dega_hip_decode_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t T, size_t ld,
                                   int adaptive, int valuesize, int32_t *x_tc, int32_t *err, void *stream)
{
  int ret;
  if ((ret = check_shape(ctx, C, T, ld, cap, valuesize)) != DEGA_OK)
    return ret;
  return launch_decode(ctx, in, cap, in_bits, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_I32), C, x_tc, nullptr, err, (hipStream_t)stream);
}

extern "C" int dega_hip_decode_var_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld,
                                       int adaptive, int valuesize, int32_t *x_tc, uint64_t *out_count, int32_t *err, void *stream)
{
  int ret;
  if (out_count == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if ((ret = check_shape(ctx, C, max_T, ld, cap, valuesize)) != DEGA_OK)
    return ret;
  return launch_decode(ctx, in, cap, in_bits, shape_of(C, max_T, ld, adaptive, valuesize, DEGA_SAMPLES_I32), C, x_tc, out_count, err, (hipStream_t)stream);
}

extern "C" int dega_hip_encode_f32_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, float factor, int adaptive, int valuesize,
                                       uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream)
{
  return launch_encode(ctx, v_tc, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_F32, factor), out, cap, out_bits, err, (hipStream_t)stream);
}

extern "C" int dega_hip_decode_f32_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t T, size_t ld,
                                       float factor, int adaptive, int valuesize, float *v_tc, uint64_t *out_count, int32_t *err, void *stream)
{
  return launch_decode(ctx, in, cap, in_bits, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_F32, factor), C, v_tc, out_count, err, (hipStream_t)stream);
}

extern "C" int dega_hip_encode_f32_var_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count, float factor,
                                           int adaptive, int valuesize, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (count == nullptr && C != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "encode: count must be a device array of C entries", hipSuccess);
  return launch_encode(ctx, v_tc, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_F32, factor), out, cap, out_bits, err, (hipStream_t)stream, nullptr, 0,
                       count);
}

extern "C" int dega_hip_normalize_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, float factor, int valuesize,
                                      int32_t *x_tc, int32_t *err, void *stream)
{
  int ret;
  if ((ret = check_shape(ctx, C, T, ld, 0, valuesize)) != DEGA_OK)
    return ret;
  if (C == 0)
    return DEGA_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(ctx, hipMemsetAsync(err, 0, C * sizeof(int32_t), s), DEGA_ERROR_LIBRARY_CALL);
  if (T == 0)
    return DEGA_OK;
  launch(normalize_args(v_tc, x_tc, C, T, ld, factor, err, valuesize), rowsplit_ranges(C, T), OnStream{s});
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

extern "C" int dega_hip_denormalize_dev(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T, size_t ld, float factor, int valuesize,
                                        float *v_tc, void *stream)
{
  int ret;
  if ((ret = check_shape(ctx, C, T, ld, 0, valuesize)) != DEGA_OK)
    return ret;
  if (C == 0 || T == 0)
    return DEGA_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  launch(denormalize_args(x_tc, v_tc, C, T, ld, factor, valuesize), rowsplit_ranges(C, T), OnStream{(hipStream_t)stream});
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

// ---- aggregate (DCLib/src/aggregate.c) --------------------------------------------------------------------------------------

extern "C" size_t dega_hip_aggregate_rows(size_t T, size_t num_values)
{
  return num_values == 0 ? 0 : T / num_values + (T % num_values != 0 ? 1 : 0);
}

static bool f32_array(const void *p) // a float32 device array, as far as the host can tell
{
  return p != nullptr && ((uintptr_t)p & 3u) == 0;
}

// the bytes from the first to the last value of a [rows][ld] float32 image of C channels (rows at least 1)
static size_t image_bytes(size_t rows, size_t ld, size_t C)
{
  return ((rows - 1) * ld + C) * sizeof(float);
}

static int launch_aggregate(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, size_t N, float *a_tc, size_t ld_out, hipStream_t s)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (N == 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate: num_values must be at least 1 (the reference does not terminate on 0)", hipSuccess);
  if (ld < C || ld_out < C)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate: ld < C or ld_out < C", hipSuccess);
  if (C == 0 || T == 0)
    return DEGA_OK;
  if (!f32_array(v_tc) || !f32_array(a_tc))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate: v_tc and a_tc must be float32 device arrays", hipSuccess);
  const size_t T_out = dega_hip_aggregate_rows(T, N);
  {
    // a_tc may not alias v_tc
    const uintptr_t v0 = (uintptr_t)v_tc, v1 = v0 + image_bytes(T, ld, C);
    const uintptr_t a0 = (uintptr_t)a_tc, a1 = a0 + image_bytes(T_out, ld_out, C);
    if (a0 < v1 && v0 < a1)
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate: a_tc overlaps v_tc", hipSuccess);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  const bool wide = aggregate_wide(v_tc, C, ld);
  if (!launch(AggregateVariant{wide, 1}, aggregate_args(v_tc, C, T, ld, N, a_tc, ld_out, wide, aggregate_row_ranges(C, T_out, wide)), OnStream{s}))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate: too many channels for one launch", hipSuccess);
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

extern "C" int dega_hip_aggregate_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, size_t num_values, float *a_tc,
                                      size_t ld_out, void *stream)
{
  return launch_aggregate(ctx, v_tc, C, T, ld, num_values, a_tc, ld_out, (hipStream_t)stream);
}

// ---- channel-major <-> time-major ---------------------------------------------------------------------------------------

// S[R][sp] -> D[K][dp], D[k][r] = S[r][k]; the channel (what `count` is indexed by) is the source row when channel_rows.
// to time-major: R = C, K = T; to channel-major: R = T, K = C.
static int launch_transpose(dega_hip_ctx *ctx, const void *src, size_t R, size_t K, size_t sp, size_t esz, const uint64_t *count, bool channel_rows,
                            void *dst, size_t dp, hipStream_t s)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (esz != 4 && esz != 8)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "transpose: elem_bytes must be 4 or 8", hipSuccess);
  if (sp < K || dp < R)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "transpose: ld < C or stride < T", hipSuccess);
  if (R == 0 || K == 0)
    return DEGA_OK;
  if (src == nullptr || dst == nullptr || ((uintptr_t)src & (esz - 1)) != 0 || ((uintptr_t)dst & (esz - 1)) != 0 || ((uintptr_t)count & 7u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "transpose: the images must be aligned to their elements, the counts to 8 bytes", hipSuccess);
  {
    // the byte ranges of the two images; sizes whose ranges do not fit the address space are refused, not wrapped
    size_t sn, dn;
    uintptr_t s1, d1;
    const uintptr_t s0 = (uintptr_t)src, d0 = (uintptr_t)dst;
    if (__builtin_mul_overflow(R - 1, sp, &sn) || __builtin_add_overflow(sn, K, &sn) || __builtin_mul_overflow(sn, esz, &sn) ||
        __builtin_add_overflow(s0, sn, &s1) || __builtin_mul_overflow(K - 1, dp, &dn) || __builtin_add_overflow(dn, R, &dn) ||
        __builtin_mul_overflow(dn, esz, &dn) || __builtin_add_overflow(d0, dn, &d1))
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "transpose: an image does not fit the address space", hipSuccess);
    if (d0 < s1 && s0 < d1)
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "transpose: source and destination overlap", hipSuccess);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  if (!launch(transpose_variant(src, sp, dst, dp, esz), transpose_args(src, R, K, sp, count, channel_rows, dst, dp), TR_GRID_X, OnStream{s}))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "transpose: too many tiles for one launch", hipSuccess);
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

extern "C" int dega_hip_to_time_major_dev(dega_hip_ctx *ctx, const void *x_ct, size_t C, size_t T, size_t stride, size_t elem_bytes, const uint64_t *count,
                                          void *x_tc, size_t ld, void *stream)
{
  return launch_transpose(ctx, x_ct, C, T, stride, elem_bytes, count, true, x_tc, ld, (hipStream_t)stream);
}

extern "C" int dega_hip_to_channel_major_dev(dega_hip_ctx *ctx, const void *x_tc, size_t C, size_t T, size_t ld, size_t elem_bytes, const uint64_t *count,
                                             void *x_ct, size_t stride, void *stream)
{
  return launch_transpose(ctx, x_tc, T, C, ld, elem_bytes, count, false, x_ct, stride, (hipStream_t)stream);
}

// `bytes` of the block for a call on s: grown if need be, and s behind the block's last user where that was another stream.
static int scratch_acquire(dega_hip_ctx *ctx, Scratch &b, size_t bytes, hipStream_t s)
{
  if (bytes > b.bytes)
  {
    const size_t want = std::max(bytes, 2 * b.bytes); // doubling: the blocks kept back sum to less than the live one
    uint8_t *p = nullptr;
    HIP_TRY(ctx, hipMalloc((void **)&p, want), DEGA_ERROR_MEMORY);
    if (b.p != nullptr)
      ctx->agg_retired.push_back(b.p); // (a kernel may still read it: kept until the context goes)
    b.p = p;
    b.bytes = want;
  }
  if (b.done == nullptr)
    HIP_TRY(ctx, hipEventCreateWithFlags(&b.done, hipEventDisableTiming), DEGA_ERROR_LIBRARY_CALL);
  // the block may still be in use by a launch of an earlier call on another stream: this stream goes on behind it
  if (b.pending && b.stream != s)
    HIP_TRY(ctx, hipStreamWaitEvent(s, b.done, 0), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

// The call's launches are on s: the block's event behind them, unless the caller has `recorded` it already behind the
// block's last user.  A launcher comes here whatever its launches said.
static int scratch_release(dega_hip_ctx *ctx, Scratch &b, hipStream_t s, bool recorded = false)
{
  if (!recorded)
    HIP_TRY(ctx, hipEventRecord(b.done, s), DEGA_ERROR_LIBRARY_CALL);
  b.stream = s;
  b.pending = true;
  return DEGA_OK;
}

extern "C" int dega_hip_encode_agg_f32_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, size_t num_values, float factor,
                                           int adaptive, int valuesize, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (num_values == 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate: num_values must be at least 1 (the reference does not terminate on 0)", hipSuccess);
  // one level of the levels form: an aggregate launch into the context's scratch and the coder over it, or, for
  // num_values = 1, the coder straight over v_tc (0.0f + v differs from v for -0.0f only, and Normalize maps both zeros to 0)
  return dega_hip_encode_levels_f32_dev(ctx, v_tc, C, T, ld, &num_values, 1, factor, adaptive, valuesize, &out, &cap, &out_bits, &err, stream);
}

// ---- several granularities from one pass over the base series (aggregate_levels_kernels.hpp), for ragged batches with a
// ---- count per channel (aggregate_var_kernels.hpp) ------------------------------------------------------------------------

static_assert(DEGA_AGG_MAX_LEVELS == AGG_MAX_LEVELS, "the header's limit is the kernel's");

// A pass needs this many workgroups before a level may join it.  REASONED, not measured: two workgroups per CU (256 CUs);
// the streaming figure is about 32 KiB of loads in flight per CU, and one workgroup of the kernel holds 4 waves x 16 KiB
// in the 16-byte form.  tools/aggbench.py --levels on a narrow batch (a few hundred channels) is the measurement that
// would revisit it.
constexpr size_t AGG_LEVELS_MIN_WORKGROUPS = 512;
static size_t levels_min_workgroups() // DEGA_AGG_LEVELS_MIN_WORKGROUPS=n: measurement / test knob (1: levels share a pass whatever the batch size)
{
  const char *e = getenv("DEGA_AGG_LEVELS_MIN_WORKGROUPS");
  const long long v = e != nullptr ? atoll(e) : 0;
  return v >= 1 ? (size_t)v : AGG_LEVELS_MIN_WORKGROUPS;
}

static size_t gcd_of(size_t x, size_t y)
{
  while (y != 0)
  {
    const size_t r = x % y;
    x = y;
    y = r;
  }
  return x;
}

// least common multiple, anything above `top` counts as `top` (no product is formed that could wrap)
static size_t lcm_capped(size_t x, size_t y, size_t top)
{
  const size_t q = y / gcd_of(x, y);
  if (x >= top || q > top / x)
    return top;
  return std::min(x * q, top);
}

struct LevelsPlan
{
  int passes = 0;
  int pass_of[AGG_MAX_LEVELS];
  size_t step_of[AGG_MAX_LEVELS];
};

// 0 = fine; the levels themselves (K <= 8, no N = 0, no N twice)
static int check_level_list(const size_t *num_values, size_t K)
{
  if (K > AGG_MAX_LEVELS || (K != 0 && num_values == nullptr))
    return DEGA_ERROR_INVALID_VALUE;
  for (size_t k = 0; k < K; k++)
  {
    if (num_values[k] == 0)
      return DEGA_ERROR_INVALID_VALUE;
    for (size_t i = 0; i < k; i++)
      if (num_values[i] == num_values[k])
        return DEGA_ERROR_INVALID_VALUE;
  }
  return DEGA_OK;
}

// Which levels share a pass.  Levels in ascending N; a level joins the first pass whose least common multiple L, with it,
// still leaves gx x ceil(T / L) >= AGG_LEVELS_MIN_WORKGROUPS workgroups, else it opens a pass of its own.  A pass of one
// level is launch_aggregate as it is, so the worst case is K passes: what K calls do.  There is no cap on the levels of a
// pass: measured, eight levels in one pass take 14.1 ms where two passes of four take 16.4.
static void plan_levels(size_t C, size_t T, const size_t *num_values, size_t K, bool wide, LevelsPlan &p)
{
  const size_t gx = std::max<size_t>(aggregate_gx(C, wide), 1), Tn = std::max<size_t>(T, 1);
  const size_t min_workgroups = levels_min_workgroups();
  size_t order[AGG_MAX_LEVELS], L_of[AGG_MAX_LEVELS], members[AGG_MAX_LEVELS];
  for (size_t k = 0; k < K; k++)
    order[k] = k;
  std::sort(order, order + K, [&](size_t x, size_t y) { return num_values[x] < num_values[y]; });
  p.passes = 0;
  for (size_t i = 0; i < K; i++)
  {
    const size_t k = order[i], N = std::min(num_values[k], Tn);
    int at = -1;
    for (int q = 0; q < p.passes && at < 0 && Tn <= 0xFFFFFFFFu; q++) // (the kernel's counters are 32-bit: longer series go level by level)
    {
      const size_t L = lcm_capped(L_of[q], N, Tn);
      if (gx * ((Tn + L - 1) / L) >= min_workgroups)
      {
        at = q;
        L_of[q] = L;
        members[q]++;
      }
    }
    if (at < 0)
    {
      at = p.passes++;
      L_of[at] = N;
      members[at] = 1;
    }
    p.pass_of[k] = at;
  }
  const size_t want = std::max<size_t>(1, (2048 + gx - 1) / gx); // ranges launch_aggregate aims for
  for (int q = 0; q < p.passes; q++)
  {
    const size_t L = L_of[q], ranges = (Tn + L - 1) / L;
    if (members[q] == 1) // what launch_aggregate does with this level: whole output rows per range
    {
      const size_t gy = std::min<size_t>(std::min<size_t>(ranges, 65535), want);
      p.step_of[q] = (ranges + gy - 1) / gy * L;
      continue;
    }
    size_t m = std::max<size_t>(std::max<size_t>(1, ranges / want), (ranges + 65534) / 65535);
    p.step_of[q] = L * m; // (L <= T < 2^32 and m <= ranges: no wrap)
  }
}

extern "C" int dega_hip_aggregate_levels_plan(size_t C, size_t T, const size_t *num_values, size_t K, int wide, int *pass_of, size_t *step_of)
{
  if (check_level_list(num_values, K) != DEGA_OK || (K != 0 && (pass_of == nullptr || step_of == nullptr)))
    return DEGA_ERROR_INVALID_VALUE;
  LevelsPlan p;
  plan_levels(C, T, num_values, K, wide != 0 && C % 4 == 0, p);
  for (size_t k = 0; k < K; k++)
    pass_of[k] = p.pass_of[k];
  for (int q = 0; q < p.passes; q++)
    step_of[q] = p.step_of[q];
  return p.passes;
}

// Everything launch_aggregate and the pass launches would refuse, for all levels, before the first launch.
static int check_levels_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const size_t *num_values, size_t K, float *const *a_tc,
                            const size_t *ld_out)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (check_level_list(num_values, K) != DEGA_OK)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate levels: at most 8 levels, every num_values at least 1, none twice", hipSuccess);
  if (K == 0)
    return DEGA_OK;
  if (a_tc == nullptr || ld_out == nullptr)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate levels: a_tc and ld_out are arrays of K entries", hipSuccess);
  if (ld < C)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate levels: ld < C", hipSuccess);
  for (size_t k = 0; k < K; k++)
    if (ld_out[k] < C)
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate levels: ld_out < C", hipSuccess);
  if (C == 0 || T == 0)
    return DEGA_OK;
  if (!f32_array(v_tc))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate levels: v_tc must be a float32 device array", hipSuccess);
  if (aggregate_gx(C, false) > 0x7FFFFFFFu)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate levels: too many channels for one launch", hipSuccess);
  uintptr_t lo[AGG_MAX_LEVELS + 1], hi[AGG_MAX_LEVELS + 1];
  lo[K] = (uintptr_t)v_tc;
  hi[K] = lo[K] + image_bytes(T, ld, C);
  for (size_t k = 0; k < K; k++)
  {
    if (!f32_array(a_tc[k]))
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate levels: every a_tc[k] must be a float32 device array", hipSuccess);
    lo[k] = (uintptr_t)a_tc[k];
    hi[k] = lo[k] + image_bytes(dega_hip_aggregate_rows(T, num_values[k]), ld_out[k], C);
    if (lo[k] < hi[K] && lo[K] < hi[k])
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate levels: an output overlaps v_tc", hipSuccess);
    for (size_t i = 0; i < k; i++)
      if (lo[k] < hi[i] && lo[i] < hi[k])
        return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate levels: two levels' outputs overlap", hipSuccess);
  }
  return DEGA_OK;
}

// what the counted entry points add to their uniform twins' refusals
static int check_counts(dega_hip_ctx *ctx, size_t C, size_t T, const uint64_t *count, uint64_t *const *out_count, size_t K, const int32_t *err)
{
  if (C == 0)
    return DEGA_OK;
  if (count == nullptr || ((uintptr_t)count & 7u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "counts: count must be a device array of C 64-bit entries, 8-byte aligned", hipSuccess);
  if (err == nullptr || ((uintptr_t)err & 3u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "counts: err must be a device array of C entries", hipSuccess);
  if (K != 0 && out_count == nullptr)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "counts: out_count is an array of K entries", hipSuccess);
  for (size_t k = 0; k < K; k++)
    if (out_count[k] == nullptr || ((uintptr_t)out_count[k] & 7u) != 0)
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "counts: every out_count[k] must be a device array of C 64-bit entries, 8-byte aligned", hipSuccess);
  if (T > 0xFFFFFFFFu)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "counts: at most 2^32 - 1 rows", hipSuccess);
  return DEGA_OK;
}

// The passes of the plan on s.  `count`, `out_count` and `err` are null for a uniform batch; with them the passes (planned
// on T, as for the uniform call) go through the counted kernel.  The arguments have been through check_levels_dev and,
// for a counted batch, check_counts.
static int launch_aggregate_levels(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count, const size_t *num_values,
                                   size_t K, float *const *a_tc, const size_t *ld_out, uint64_t *const *out_count, int32_t *err, hipStream_t s)
{
  if (K == 0 || C == 0 || (T == 0 && count == nullptr)) // (a counted batch still launches at T = 0: the counts and the status are the kernel's)
    return DEGA_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  const bool wide = aggregate_wide(v_tc, C, ld);
  LevelsPlan p;
  plan_levels(C, T, num_values, K, wide, p);
  for (int q = 0; q < p.passes; q++)
  {
    size_t N[AGG_MAX_LEVELS], ldo[AGG_MAX_LEVELS];
    float *a[AGG_MAX_LEVELS];
    uint64_t *oc[AGG_MAX_LEVELS];
    uint32_t n = 0;
    for (size_t k = 0; k < K; k++)
      if (p.pass_of[k] == q)
      {
        N[n] = num_values[k];
        a[n] = a_tc[k];
        ldo[n] = ld_out[k];
        oc[n] = count != nullptr ? out_count[k] : nullptr;
        n++;
      }
    if (count == nullptr && n == 1) // the existing kernel and launcher, as they are
    {
      const int ret = launch_aggregate(ctx, v_tc, C, T, ld, N[0], a[0], ldo[0], s);
      if (ret != DEGA_OK)
        return ret;
      continue;
    }
    const AggregatePass pass{v_tc, C, T, ld, p.step_of[q], N, a, ldo};
    // (counted: the status is one pass's to write)
    if (!(count != nullptr ? launch(AggregateVariant{wide, n}, pass, AggregateCounts{count, oc, q == 0 ? err : nullptr}, OnStream{s})
                           : launch(AggregateVariant{wide, n}, pass, OnStream{s})))
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate levels: too many channels for one launch", hipSuccess);
    HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  }
  return DEGA_OK;
}

// One body for the uniform and the counted ("ragged", aggregate_var_kernels.hpp) form of each level call.  `counted`: the
// call came through a counted entry point; its `count` may still be null, which check_counts refuses where C is not 0, so
// past that check `count != nullptr` says the same.
static int aggregate_levels(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, bool counted, const uint64_t *count,
                            const size_t *num_values, size_t K, float *const *a_tc, const size_t *ld_out, uint64_t *const *out_count, int32_t *err,
                            hipStream_t s)
{
  int ret;
  if ((ret = check_levels_dev(ctx, v_tc, C, T, ld, num_values, K, a_tc, ld_out)) != DEGA_OK)
    return ret;
  if (counted)
  {
    if (K == 0)
      return DEGA_OK;
    if ((ret = check_counts(ctx, C, T, count, out_count, K, err)) != DEGA_OK)
      return ret;
  }
  return launch_aggregate_levels(ctx, v_tc, C, T, ld, count, num_values, K, a_tc, ld_out, out_count, err, s);
}

extern "C" int dega_hip_aggregate_levels_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const size_t *num_values, size_t K,
                                             float *const *a_tc, const size_t *ld_out, void *stream)
{
  return aggregate_levels(ctx, v_tc, C, T, ld, false, nullptr, num_values, K, a_tc, ld_out, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int dega_hip_aggregate_levels_var_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count,
                                                 const size_t *num_values, size_t K, float *const *a_tc, const size_t *ld_out, uint64_t *const *out_count,
                                                 int32_t *err, void *stream)
{
  return aggregate_levels(ctx, v_tc, C, T, ld, true, count, num_values, K, a_tc, ld_out, out_count, err, (hipStream_t)stream);
}

static size_t round4(size_t n)
{
  return (n + 3) & ~(size_t)3;
}

// The summed levels of a call, one behind the other in a block of floats with pitch ld: level i of them is the caller's
// level `level[i]`, off[i] floats into the block.  The offsets are multiples of four floats: every level's sums keep the
// 16-byte alignment of the block.  A level with num_values 1 is summed only where the caller asks for it (`with_one`).
struct LevelSums
{
  size_t n = 0, floats = 0;
  size_t level[AGG_MAX_LEVELS], N[AGG_MAX_LEVELS], off[AGG_MAX_LEVELS], ldo[AGG_MAX_LEVELS];
  float *a[AGG_MAX_LEVELS];
  LevelSums(const size_t *num_values, size_t K, size_t T, size_t ld, bool with_one)
  {
    for (size_t k = 0; k < K; k++)
    {
      if (num_values[k] == 1 && !with_one)
        continue;
      level[n] = k;
      N[n] = num_values[k];
      off[n] = floats;
      ldo[n] = ld;
      floats += round4(dega_hip_aggregate_rows(T, num_values[k]) * ld);
      n++;
    }
  }
  void place(float *block)
  {
    for (size_t i = 0; i < n; i++)
      a[i] = block + off[i];
  }
};

// err[c] = src[c] where that is set, and the channel's 64-bit result (its bits or its count) 0: a channel that an earlier
// launch of the chain gave up reports that launch's status and nothing else
__global__ void __launch_bounds__(256) dega_status_kernel(const int32_t *src, size_t C, int32_t *err, uint64_t *result)
{
  const size_t c = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (c < C && src[c] != 0)
  {
    err[c] = src[c];
    result[c] = 0;
  }
}

// (no HIP_TRY: a launcher that is told of a failed launch still has its event to record)
static int launch_status(dega_hip_ctx *ctx, const int32_t *src, size_t C, int32_t *err, uint64_t *result, hipStream_t s)
{
  hipLaunchKernelGGL(dega_status_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, src, C, err, result);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? DEGA_OK : fail(ctx, DEGA_ERROR_LIBRARY_CALL, "hipLaunchKernel", e);
}

// a level with num_values 1 is coded from the readings: its counts are the caller's, 0 where one is above T
__global__ void __launch_bounds__(256) dega_level_counts_kernel(const uint64_t *count, size_t C, size_t T, uint64_t *out_count)
{
  const size_t c = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (c < C)
    out_count[c] = count[c] > T ? 0u : count[c];
}

// `counted` as in aggregate_levels
static int encode_levels(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, bool counted, const uint64_t *count, const size_t *num_values,
                         size_t K, float factor, int adaptive, int valuesize, uint8_t *const *out, const size_t *cap, uint64_t *const *out_bits,
                         uint64_t *const *out_count, int32_t *const *err, hipStream_t s)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (check_level_list(num_values, K) != DEGA_OK)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "encode levels: at most 8 levels, every num_values at least 1, none twice", hipSuccess);
  if (K == 0)
    return DEGA_OK;
  if (out == nullptr || cap == nullptr || out_bits == nullptr || err == nullptr || (counted && out_count == nullptr))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE,
                counted ? "encode levels: out, cap, out_bits, out_count and err are arrays of K entries"
                        : "encode levels: out, cap, out_bits and err are arrays of K entries",
                hipSuccess);
  int ret;
  // every level's encode launch judged before the first launch (cap[k] and the 2^25 limit against level k's rows, for a
  // counted batch the rows T allows), and the levels that are summed (N = 1 is coded straight from v_tc)
  Shape j[AGG_MAX_LEVELS];
  for (size_t k = 0; k < K; k++)
  {
    j[k] = shape_of(C, dega_hip_aggregate_rows(T, num_values[k]), ld, adaptive, valuesize, DEGA_SAMPLES_F32, factor);
    if ((ret = check_job_shape(ctx, j[k], cap[k])) != DEGA_OK)
      return ret;
    if (C != 0 && (out[k] == nullptr || out_bits[k] == nullptr || err[k] == nullptr || (counted && ((uintptr_t)err[k] & 3u) != 0)))
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "encode levels: null output", hipSuccess);
  }
  LevelSums sums(num_values, K, T, ld, false);
  if (C == 0)
    return DEGA_OK;
  if (counted && (ret = check_counts(ctx, C, T, count, out_count, K, err[0])) != DEGA_OK)
    return ret;
  if (!f32_array(v_tc))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "encode levels: v_tc must be a float32 device array", hipSuccess);
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  // a counted batch: the summed levels' common status (a count above T) in front of their sums
  const size_t head = count != nullptr ? round4(C) : 0;
  if ((ret = scratch_acquire(ctx, ctx->sums, (head + std::max<size_t>(sums.floats, 4)) * sizeof(float), s)) != DEGA_OK)
    return ret;
  int32_t *const first = count != nullptr ? (int32_t *)ctx->sums.p : nullptr;
  sums.place((float *)ctx->sums.p + head);
  if ((ret = check_levels_dev(ctx, v_tc, C, T, ld, sums.N, sums.n, sums.a, sums.ldo)) != DEGA_OK)
    return ret;
  uint64_t *oc[AGG_MAX_LEVELS];
  for (size_t i = 0; i < sums.n && count != nullptr; i++)
    oc[i] = out_count[sums.level[i]];
  if ((ret = launch_aggregate_levels(ctx, v_tc, C, T, ld, count, sums.N, sums.n, sums.a, sums.ldo, oc, first, s)) == DEGA_OK)
  {
    size_t i = 0;
    for (size_t k = 0; k < K && ret == DEGA_OK; k++)
    {
      if (num_values[k] == 1)
      {
        if (count != nullptr) // coded from v_tc with `count` itself
          hipLaunchKernelGGL(dega_level_counts_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, count, C, T, out_count[k]);
        ret = launch_encode(ctx, v_tc, j[k], out[k], cap[k], out_bits[k], err[k], s, nullptr, 0, count);
        continue;
      }
      // (counted: a channel whose count is above T has level counts of 0: it is coded as empty, and the status launch names it)
      ret = launch_encode(ctx, sums.a[i++], j[k], out[k], cap[k], out_bits[k], err[k], s, nullptr, 0, count != nullptr ? out_count[k] : nullptr);
      if (count != nullptr && ret == DEGA_OK)
        ret = launch_status(ctx, first, C, err[k], out_bits[k], s);
    }
  }
  // (recorded whatever the launches said: behind the LAST launch on the stream that reads the scratch)
  const int rel = scratch_release(ctx, ctx->sums, s);
  return rel != DEGA_OK ? rel : ret;
}

extern "C" int dega_hip_encode_levels_f32_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const size_t *num_values, size_t K,
                                              float factor, int adaptive, int valuesize, uint8_t *const *out, const size_t *cap, uint64_t *const *out_bits,
                                              int32_t *const *err, void *stream)
{
  return encode_levels(ctx, v_tc, C, T, ld, false, nullptr, num_values, K, factor, adaptive, valuesize, out, cap, out_bits, nullptr, err, (hipStream_t)stream);
}

extern "C" int dega_hip_encode_levels_f32_var_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count,
                                                  const size_t *num_values, size_t K, float factor, int adaptive, int valuesize, uint8_t *const *out,
                                                  const size_t *cap, uint64_t *const *out_bits, uint64_t *const *out_count, int32_t *const *err, void *stream)
{
  return encode_levels(ctx, v_tc, C, T, ld, true, count, num_values, K, factor, adaptive, valuesize, out, cap, out_bits, out_count, err, (hipStream_t)stream);
}

// ---- A-XDR: packed fields (axdr_kernels.hpp), the study's third chain ----------------------------------------------------------

extern "C" size_t dega_hip_axdr_bytes(size_t T, int valuesize)
{
  size_t bits;
  if (valuesize < 1 || valuesize > 64 || __builtin_mul_overflow(T, (size_t)valuesize, &bits) || bits > ~(size_t)0 - 31)
    return 0;
  return (bits + 31) / 32 * 4;
}

// What every A-XDR entry point refuses before the device is touched, the host forms included.  rows: T or max_T; x_tc: the
// rows; slabs, bits, err: the per-channel arrays of either direction; counts: `count` (may be null) or `out_count` (may not).
static int check_axdr(dega_hip_ctx *ctx, int samples, int valuesize, size_t C, size_t rows, size_t ld, size_t cap, const void *x_tc, const void *slabs,
                      const void *bits, const void *err, const void *counts, bool counts_needed)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (samples != DEGA_SAMPLES_F32 && samples != DEGA_SAMPLES_I32 && samples != DEGA_SAMPLES_I64)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "axdr: samples must be DEGA_SAMPLES_F32, _I32 or _I64, time-major", hipSuccess);
  if (valuesize < 1 || valuesize > 64 || (samples == DEGA_SAMPLES_I32 && valuesize > 32) || (samples == DEGA_SAMPLES_I64 && valuesize <= 32))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "axdr: sample type and valuesize do not go together (int32: 1..32, int64: 33..64, float32: 1..64)", hipSuccess);
  if (ld < C)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "axdr: ld < C", hipSuccess);
  size_t all;
  if (cap % 4 != 0 || __builtin_mul_overflow(C, cap, &all))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "axdr: cap must be a multiple of 4, and C * cap fit the address space", hipSuccess);
  if (rows > AX_MAX_T)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "axdr: at most 2^32 - 1 rows", hipSuccess);
  if (C == 0)
    return DEGA_OK;
  const uintptr_t esz = samples == DEGA_SAMPLES_I64 ? 8 : 4;
  if ((x_tc == nullptr && rows != 0) || ((uintptr_t)x_tc & (esz - 1)) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "axdr: the rows must be an array aligned to its elements", hipSuccess);
  if ((slabs == nullptr && cap != 0) || ((uintptr_t)slabs & 3u) != 0 || bits == nullptr || ((uintptr_t)bits & 7u) != 0 || err == nullptr ||
      ((uintptr_t)err & 3u) != 0 || (counts == nullptr && counts_needed) || ((uintptr_t)counts & 7u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "axdr: the slabs (4-byte aligned), the bit lengths and counts (8) and err (4) must be arrays", hipSuccess);
  return DEGA_OK;
}

static uint32_t axdr_kind(int samples)
{
  return samples == DEGA_SAMPLES_F32 ? AX_F32 : (samples == DEGA_SAMPLES_I32 ? AX_I32 : AX_I64);
}

// The status zeroed and the pack kernel behind it on s; the arguments have been through check_axdr, and C is not 0
static int launch_axdr_pack(dega_hip_ctx *ctx, const void *x_tc, int samples, size_t C, size_t T, size_t ld, const uint64_t *count, float factor, int valuesize,
                            uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, hipStream_t s)
{
  HIP_TRY(ctx, hipMemsetAsync(err, 0, C * sizeof(int32_t), s), DEGA_ERROR_LIBRARY_CALL);
  if (!launch(axdr_variant(axdr_kind(samples), valuesize, x_tc, ld), axdr_pack_args(x_tc, C, T, ld, count, factor, valuesize, out, cap, out_bits, err), TR_GRID_X,
              OnStream{s}))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "axdr encode: too many tiles for one launch", hipSuccess);
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

static int launch_axdr_unpack(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld, float factor,
                              int valuesize, int samples, void *x_tc, uint64_t *out_count, int32_t *err, hipStream_t s)
{
  if (!launch(axdr_variant(axdr_kind(samples), valuesize, x_tc, ld), axdr_unpack_args(in, cap, in_bits, C, max_T, ld, factor, valuesize, x_tc, out_count, err),
              TR_GRID_X, OnStream{s}))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "axdr decode: too many tiles for one launch", hipSuccess);
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

extern "C" int dega_hip_axdr_encode_dev(dega_hip_ctx *ctx, const void *x_tc, int samples, size_t C, size_t T, size_t ld, const uint64_t *count, float factor,
                                        int valuesize, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream)
{
  int ret;
  if ((ret = check_axdr(ctx, samples, valuesize, C, T, ld, cap, x_tc, out, out_bits, err, count, false)) != DEGA_OK || C == 0)
    return ret;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  return launch_axdr_pack(ctx, x_tc, samples, C, T, ld, count, factor, valuesize, out, cap, out_bits, err, (hipStream_t)stream);
}

extern "C" int dega_hip_axdr_decode_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld,
                                        float factor, int valuesize, int samples, void *x_tc, uint64_t *out_count, int32_t *err, void *stream)
{
  int ret;
  if ((ret = check_axdr(ctx, samples, valuesize, C, max_T, ld, cap, x_tc, in, in_bits, err, out_count, true)) != DEGA_OK || C == 0)
    return ret;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  return launch_axdr_unpack(ctx, in, cap, in_bits, C, max_T, ld, factor, valuesize, samples, x_tc, out_count, err, (hipStream_t)stream);
}

// encode_levels with the pack kernel in the coder's place: aggregate into the context's scratch, then one pack per level.
// A null `count` is the uniform form (out_count is not looked at then).
extern "C" int dega_hip_axdr_encode_levels_f32_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count,
                                                   const size_t *num_values, size_t K, float factor, int valuesize, uint8_t *const *out, const size_t *cap,
                                                   uint64_t *const *out_bits, uint64_t *const *out_count, int32_t *const *err, void *stream)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (check_level_list(num_values, K) != DEGA_OK)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "axdr levels: at most 8 levels, every num_values at least 1, none twice", hipSuccess);
  if (K == 0)
    return DEGA_OK;
  const bool counted = count != nullptr;
  if (out == nullptr || cap == nullptr || out_bits == nullptr || err == nullptr || (counted && out_count == nullptr))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "axdr levels: out, cap, out_bits, err (and out_count with count) are arrays of K entries", hipSuccess);
  int ret;
  size_t rows[AGG_MAX_LEVELS];
  for (size_t k = 0; k < K; k++) // every level's pack judged before the first launch
  {
    rows[k] = dega_hip_aggregate_rows(T, num_values[k]);
    if ((ret = check_axdr(ctx, DEGA_SAMPLES_F32, valuesize, C, rows[k], ld, cap[k], v_tc, out[k], out_bits[k], err[k], counted ? out_count[k] : nullptr,
                          counted)) != DEGA_OK)
      return ret;
  }
  LevelSums sums(num_values, K, T, ld, false);
  if (C == 0)
    return DEGA_OK;
  if (counted && (ret = check_counts(ctx, C, T, count, out_count, K, err[0])) != DEGA_OK)
    return ret;
  hipStream_t s = (hipStream_t)stream;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  const size_t head = counted ? round4(C) : 0; // a counted batch: the summed levels' common status (a count above T) in front of their sums
  if ((ret = scratch_acquire(ctx, ctx->sums, (head + std::max<size_t>(sums.floats, 4)) * sizeof(float), s)) != DEGA_OK)
    return ret;
  int32_t *const first = counted ? (int32_t *)ctx->sums.p : nullptr;
  sums.place((float *)ctx->sums.p + head);
  if ((ret = check_levels_dev(ctx, v_tc, C, T, ld, sums.N, sums.n, sums.a, sums.ldo)) != DEGA_OK)
    return ret;
  uint64_t *oc[AGG_MAX_LEVELS];
  for (size_t i = 0; i < sums.n && counted; i++)
    oc[i] = out_count[sums.level[i]];
  if ((ret = launch_aggregate_levels(ctx, v_tc, C, T, ld, count, sums.N, sums.n, sums.a, sums.ldo, oc, first, s)) == DEGA_OK)
  {
    size_t i = 0;
    for (size_t k = 0; k < K && ret == DEGA_OK; k++)
    {
      if (num_values[k] == 1) // packed from the readings, with `count` itself
      {
        if (counted)
          hipLaunchKernelGGL(dega_level_counts_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, count, C, T, out_count[k]);
        ret = launch_axdr_pack(ctx, v_tc, DEGA_SAMPLES_F32, C, T, ld, count, factor, valuesize, out[k], cap[k], out_bits[k], err[k], s);
        continue;
      }
      // (counted: a channel whose count is above T has level counts of 0: it is packed as empty, and the status launch names it)
      ret = launch_axdr_pack(ctx, sums.a[i++], DEGA_SAMPLES_F32, C, rows[k], ld, counted ? out_count[k] : nullptr, factor, valuesize, out[k], cap[k],
                             out_bits[k], err[k], s);
      if (counted && ret == DEGA_OK)
        ret = launch_status(ctx, first, C, err[k], out_bits[k], s);
    }
  }
  const int rel = scratch_release(ctx, ctx->sums, s);
  return rel != DEGA_OK ? rel : ret;
}

// exclusive prefix sum of ceil(bits/8) over channels: one block, chunked (C is at most a few million; not a hot path)
__global__ void __launch_bounds__(1024) dega_offsets_kernel(const uint64_t *bits, size_t C, uint64_t *offsets)
{
  __shared__ uint64_t part[1024];
  __shared__ uint64_t carry;
  if (threadIdx.x == 0)
    carry = 0;
  __syncthreads();
  for (size_t base = 0; base < C; base += 1024)
  {
    const size_t i = base + threadIdx.x;
    const uint64_t v = i < C ? (bits[i] + 7) / 8 : 0;
    part[threadIdx.x] = v;
    __syncthreads();
    for (unsigned d = 1; d < 1024; d <<= 1)
    {
      const uint64_t add = threadIdx.x >= d ? part[threadIdx.x - d] : 0;
      __syncthreads();
      part[threadIdx.x] += add;
      __syncthreads();
    }
    if (i < C)
      offsets[i] = carry + part[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 1023)
      carry += part[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0)
    offsets[C] = carry;
}

extern "C" int dega_hip_compact_offsets_dev(dega_hip_ctx *ctx, const uint64_t *bits, size_t C, uint64_t *offsets, void *stream)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  hipLaunchKernelGGL(dega_offsets_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, bits, C, offsets);
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

extern "C" int dega_hip_compact_gather_dev(dega_hip_ctx *ctx, const uint8_t *slabs, size_t cap, const uint64_t *offsets, size_t C,
                                           uint8_t *packed, void *stream)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (C == 0)
    return DEGA_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  GatherArgs a{slabs, cap, offsets, C, packed};
  hipLaunchKernelGGL(dega_gather_kernel, dim3((unsigned)((C + WAVES - 1) / WAVES)), dim3(BLOCK), 0, (hipStream_t)stream, a);
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

extern "C" int dega_hip_synth_dev(dega_hip_ctx *ctx, int32_t *x_tc, size_t C, size_t T, size_t ld, uint64_t seed, uint64_t c0, uint32_t S, void *stream)
{
  if (ctx == nullptr || ld < C)
    return DEGA_ERROR_INVALID_VALUE;
  if (C == 0 || T == 0)
    return DEGA_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  SynthArgs a{x_tc, C, T, ld, seed, c0, S};
  launch(a, OnStream{(hipStream_t)stream});
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

// ---- valuesize 33..64: int64 containers ----------------------------------------------------------------------------------

static int check_shape64(dega_hip_ctx *ctx, size_t C, size_t T, size_t ld, size_t cap, int valuesize)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (valuesize < 33 || valuesize > 64)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "valuesize must be 33..64 for the [T][C] int64 layout", hipSuccess);
  return check_shape(ctx, C, T, ld, cap, 32);
}

extern "C" int dega_hip_encode64_dev(dega_hip_ctx *ctx, const int64_t *x_tc, size_t C, size_t T, size_t ld, int adaptive, int valuesize,
                                     uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream)
{
  int ret;
  if ((ret = check_shape64(ctx, C, T, ld, cap, valuesize)) != DEGA_OK)
    return ret;
  return launch_encode(ctx, x_tc, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_I64), out, cap, out_bits, err, (hipStream_t)stream);
}

extern "C" int dega_hip_encode64_var_dev(dega_hip_ctx *ctx, const int64_t *x_tc, size_t C, size_t T, size_t ld, const uint64_t *count, int adaptive,
                                         int valuesize, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, void *stream)
{
  int ret;
  if ((ret = check_shape64(ctx, C, T, ld, cap, valuesize)) != DEGA_OK || (ret = check_counts(ctx, C, T, count, nullptr, 0, err)) != DEGA_OK)
    return ret;
  return launch_encode(ctx, x_tc, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_I64), out, cap, out_bits, err, (hipStream_t)stream, nullptr, 0, count);
}

extern "C" int dega_hip_decode64_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t T, size_t ld,
                                     int adaptive, int valuesize, int64_t *x_tc, int32_t *err, void *stream)
{
  int ret;
  if ((ret = check_shape64(ctx, C, T, ld, cap, valuesize)) != DEGA_OK)
    return ret;
  return launch_decode(ctx, in, cap, in_bits, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_I64), C, x_tc, nullptr, err, (hipStream_t)stream);
}

extern "C" int dega_hip_decode64_var_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld,
                                         int adaptive, int valuesize, int64_t *x_tc, uint64_t *out_count, int32_t *err, void *stream)
{
  int ret;
  if (out_count == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if ((ret = check_shape64(ctx, C, max_T, ld, cap, valuesize)) != DEGA_OK)
    return ret;
  return launch_decode(ctx, in, cap, in_bits, shape_of(C, max_T, ld, adaptive, valuesize, DEGA_SAMPLES_I64), C, x_tc, out_count, err, (hipStream_t)stream);
}

// ---- LZMH (BASELINE config 4) ----------------------------------------------------------------------------------------

extern "C" size_t dega_hip_lzmh_worst_case_bytes(size_t n)
{
  return ((n * 10u + 7u) / 8u + 32u + 15u) / 16u * 16u; // every byte a 10-bit literal + the room the kernel keeps for its last words
}

static bool aligned16(const void *p)
{
  return ((uintptr_t)p & 15u) == 0;
}

// What the LZMH entry points refuse about their row sizes, for device and host pointers alike (`aligned`: the device
// arrays are on the kernels' boundaries -- the caller's, or a slot's own)
static int check_lzmh_encode(dega_hip_ctx *ctx, size_t stride, size_t cap, bool aligned)
{
  if (stride == 0 || (stride & 15u) != 0 || (cap & 15u) != 0 || cap < 48 || stride > 0x7FFFFFF0u || !aligned)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh encode: stride/cap must be multiples of 16 (cap >= 48), buffers 16-byte aligned", hipSuccess);
  return DEGA_OK;
}

static int check_lzmh_decode(dega_hip_ctx *ctx, size_t cap, size_t stride, bool aligned)
{
  if (cap < 4 || (cap & 3u) != 0 || stride < 8 || (stride & 7u) != 0 || !aligned)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh decode: cap must be a multiple of 4, stride a multiple of 8", hipSuccess);
  return DEGA_OK;
}

// When does a channel fit its slab?  With F the full 32-bit words of its stream and W = 4 * ceil(bits / 32) its bytes in whole
// words, lzmh_coding_wave stores F / 4 blocks of 16 bytes, the k-th at byte 16 * k and only if 16 * k + 32 <= cap, and then,
// in finish, the F % 4 words left and the partial one, only if 4 * (F + 1) <= cap.  16 * (F / 4) <= 4 * F <= W, so
//   W + 16 <= cap   is SUFFICIENT: the last block passes (16 * (F / 4 - 1) + 32 <= W + 16) and so does finish (4 * F + 4 <= W + 4);
//   W > cap         always fails in finish (W is 4 * F or 4 * F + 4): ERROR_MEMORY, out_bits 0;
// in between either happens, by F % 4.  dega_hip_lzmh_worst_case_bytes(n) >= ceil(10 * n / 8) + 32 >= W + 29 satisfies the
// sufficient condition for every text of n bytes (no code spends more than 10 bits on a byte).  tests/lzmh_encoder_common.py
// (check_slab_end) holds the kernel to exactly this, with a canary behind every slab.
extern "C" int dega_hip_lzmh_encode_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t stride, const uint64_t *in_len, size_t C, uint8_t *out,
                                        size_t cap, uint64_t *out_bits, int32_t *err, void *stream)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  int ret;
  if ((ret = check_lzmh_encode(ctx, stride, cap, aligned16(in) && aligned16(out))) != DEGA_OK)
    return ret;
  if (C == 0)
    return DEGA_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  LzmhEncodeArgs a{in, stride, in_len, C, out, cap, out_bits, err};
  hipStream_t s = (hipStream_t)stream;
  {
    LaunchTimer lt(ctx, 2, s);
    launch(a, OnStream{s});
  }
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

extern "C" int dega_hip_lzmh_decode_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, uint8_t *out,
                                        size_t stride, uint64_t *out_len, int32_t *err, void *stream)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  int ret;
  if ((ret = check_lzmh_decode(ctx, cap, stride, ((uintptr_t)in & 3u) == 0 && ((uintptr_t)out & 7u) == 0)) != DEGA_OK)
    return ret;
  if (C == 0)
    return DEGA_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  LzmhDecodeArgs a{in, cap, in_bits, C, out, stride, out_len, err};
  hipStream_t s = (hipStream_t)stream;
  {
    LaunchTimer lt(ctx, 3, s);
    launch(a, OnStream{s});
  }
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

extern "C" int dega_hip_lzmh_render_dev(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T, size_t ld, uint8_t *out, size_t stride,
                                        uint64_t *out_len, int32_t *err, void *stream)
{
  if (ctx == nullptr || ld < C || stride < 16 || (stride & 15u) != 0 || !aligned16(out))
    return DEGA_ERROR_INVALID_VALUE;
  if (C == 0)
    return DEGA_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  RenderArgs a{x_tc, C, T, ld, out, stride, out_len, err};
  launch(a, OnStream{(hipStream_t)stream});
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

// ---- encode csv (DCLib/src/csv.c:46-65): float32 series as text, alone and in front of LZMH --------------------------------

extern "C" size_t dega_hip_csv_line_max(unsigned decimals, size_t column)
{
  if (decimals > CSV_MAX_DECIMALS || column == 0)
    return 0;
  // '-' + the 39 digits of FLT_MAX + '.' and the decimals + '\n'
  const size_t value = 1 + 39 + (decimals != 0 ? 1 + (size_t)decimals : 0) + 1;
  if (column - 1 > SIZE_MAX - value)
    return 0;
  return column - 1 + value;
}

extern "C" size_t dega_hip_csv_worst_case_bytes(size_t T, unsigned decimals, size_t column)
{
  const size_t line = dega_hip_csv_line_max(decimals, column);
  if (line == 0 || T > (SIZE_MAX - CSV_SLACK - 15) / line)
    return 0;
  return (T * line + CSV_SLACK + 15) & ~(size_t)15;
}

constexpr bool CSV_DEFAULT_WIDE_STORES = false; // measured at 64 Ki x 86 400: 63.7 ms with 8-byte stores, 73.6 ms with staged 64-byte blocks
static bool csv_wide_stores() // DEGA_CSV_STORE=8 | 64: measurement / test knob, the output form of dega_csv_kernel (same bytes either way)
{
  const char *e = getenv("DEGA_CSV_STORE");
  const int v = e != nullptr ? atoi(e) : 0;
  return v == 64 ? true : (v == 8 ? false : CSV_DEFAULT_WIDE_STORES);
}

static bool ranges_overlap(const void *p, size_t np, const void *q, size_t nq)
{
  const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
  return np != 0 && nq != 0 && p0 < q0 + nq && q0 < p0 + np;
}

// The options of the stage and the text layout (everything but the pointers), for every entry point that renders.
static int check_csv_options(dega_hip_ctx *ctx, size_t C, size_t ld, unsigned decimals, size_t column, int separator_char, size_t stride)
{
  if (decimals > CSV_MAX_DECIMALS || column == 0 || separator_char < 0 || separator_char > 255)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: num_decimal_places 0..6, column at least 1, separator_char one byte", hipSuccess);
  if (stride < 16 || (stride & 15u) != 0 || stride > 0x7FFFFFF0u || column - 1 >= stride)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: stride must be a multiple of 16 (16 .. 0x7FFFFFF0) and longer than the empty columns", hipSuccess);
  if (ld < C)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: ld < C", hipSuccess);
  return DEGA_OK;
}

// The arguments have been checked; C and T are not 0.
static int launch_csv(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, unsigned decimals, size_t column, int separator_char,
                      uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err, hipStream_t s, const uint64_t *count = nullptr)
{
  if (!launch(csv_variant(csv_wide_stores(), count), csv_args(v_tc, C, T, ld, decimals, column, separator_char, out, stride, out_len, err, count), OnStream{s}))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: too many channels for one launch", hipSuccess);
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

// `counted` as in aggregate_levels
static int csv_write(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, bool counted, const uint64_t *count, unsigned decimals,
                     size_t column, int separator_char, uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err, hipStream_t s)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  int ret;
  if ((ret = check_csv_options(ctx, C, ld, decimals, column, separator_char, stride)) != DEGA_OK)
    return ret;
  if (!aligned16(out))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: out must be 16-byte aligned", hipSuccess);
  if (C == 0)
    return DEGA_OK;
  if (out == nullptr || out_len == nullptr || err == nullptr || ((uintptr_t)out_len & 7u) != 0 || ((uintptr_t)err & 3u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: out, out_len and err must be device arrays", hipSuccess);
  if (counted && (ret = check_counts(ctx, C, T, count, nullptr, 0, err)) != DEGA_OK)
    return ret;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  if (T == 0 && count == nullptr) // no reading, no text: lengths 0, nothing launched
  {
    HIP_TRY(ctx, hipMemsetAsync(out_len, 0, C * sizeof(uint64_t), s), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, hipMemsetAsync(err, 0, C * sizeof(int32_t), s), DEGA_ERROR_LIBRARY_CALL);
    return DEGA_OK;
  }
  if (T != 0 && !f32_array(v_tc))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: v_tc must be a float32 device array", hipSuccess);
  if (T != 0 && ranges_overlap(out, C * stride, v_tc, image_bytes(T, ld, C)))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: out overlaps v_tc", hipSuccess);
  // (a counted batch still launches at T = 0: a count above it is the kernel's to report)
  return launch_csv(ctx, v_tc, C, T, ld, decimals, column, separator_char, out, stride, out_len, err, s, count);
}

extern "C" int dega_hip_csv_write_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, unsigned decimals, size_t column,
                                      int separator_char, uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err, void *stream)
{
  return csv_write(ctx, v_tc, C, T, ld, false, nullptr, decimals, column, separator_char, out, stride, out_len, err, (hipStream_t)stream);
}

extern "C" int dega_hip_csv_write_var_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count, unsigned decimals,
                                          size_t column, int separator_char, uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err, void *stream)
{
  return csv_write(ctx, v_tc, C, T, ld, true, count, decimals, column, separator_char, out, stride, out_len, err, (hipStream_t)stream);
}

// ---- the same for few long channels: one channel's rows split over lanes (csv_write_split_kernels.hpp) -----------------------

extern "C" size_t dega_hip_csv_write_split_block_rows(size_t C, size_t T)
{
  return csv_write_split_block_rows(C, T);
}

extern "C" int dega_hip_csv_write_split_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count, unsigned decimals,
                                            size_t column, int separator_char, uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err,
                                            size_t block_rows, void *stream)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  int ret;
  // the refusals of csv_write, in its order
  if ((ret = check_csv_options(ctx, C, ld, decimals, column, separator_char, stride)) != DEGA_OK)
    return ret;
  if (!aligned16(out))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: out must be 16-byte aligned", hipSuccess);
  if (C == 0)
    return DEGA_OK;
  if (out == nullptr || out_len == nullptr || err == nullptr || ((uintptr_t)out_len & 7u) != 0 || ((uintptr_t)err & 3u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: out, out_len and err must be device arrays", hipSuccess);
  if (count != nullptr && (ret = check_counts(ctx, C, T, count, nullptr, 0, err)) != DEGA_OK)
    return ret;
  if (T != 0 && !f32_array(v_tc))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: v_tc must be a float32 device array", hipSuccess);
  if (T != 0 && ranges_overlap(out, C * stride, v_tc, image_bytes(T, ld, C)))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: out overlaps v_tc", hipSuccess);
  if (block_rows == 0 && (block_rows = csv_write_split_block_rows(C, T)) == 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv write split: 2^32 rows and more need a block_rows of the caller's", hipSuccess);
  const size_t blocks = csv_write_split_blocks(T, block_rows);
  if (blocks > 0xFFFFFFFFu || csv_write_split_grid(C, blocks) == 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv write split: too many blocks for one launch", hipSuccess);
  if (C > SIZE_MAX / sizeof(uint32_t) / blocks)
    return fail(ctx, DEGA_ERROR_MEMORY, "csv write split: the blocks of the batch do not fit the address space", hipSuccess);
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  hipStream_t s = (hipStream_t)stream;
  if (T == 0 && count == nullptr) // no reading, no text: lengths 0, nothing launched
  {
    HIP_TRY(ctx, hipMemsetAsync(out_len, 0, C * sizeof(uint64_t), s), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, hipMemsetAsync(err, 0, C * sizeof(int32_t), s), DEGA_ERROR_LIBRARY_CALL);
    return DEGA_OK;
  }
  // (a counted batch still launches length and scan at T = 0, as the unsplit call does: a count above it is theirs to report)
  if ((ret = scratch_acquire(ctx, ctx->wsplit, C * blocks * sizeof(uint32_t), s)) != DEGA_OK)
    return ret;
  const CsvArgs a = csv_args(v_tc, C, T, ld, decimals, column, separator_char, out, stride, out_len, err, count);
  if (!launch(csv_write_split_args(a, block_rows, (uint32_t *)ctx->wsplit.p), OnStream{s}))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv write split: too many blocks for one launch", hipSuccess); // (nothing launched)
  const hipError_t launched = hipGetLastError();
  ret = launched == hipSuccess ? DEGA_OK : fail(ctx, DEGA_ERROR_LIBRARY_CALL, "csv write split: launch", launched);
  // (recorded whatever the launches said: the first may be on the stream and writes the scratch)
  const int rel = scratch_release(ctx, ctx->wsplit, s);
  return rel != DEGA_OK ? rel : ret;
}

static size_t round16(size_t n)
{
  return (n + 15) & ~(size_t)15;
}

// The text scratch: [C] int32 status of the launch that writes the text | [C] uint64 text lengths | [C][text_stride] text,
// each 16-byte aligned.
struct TextScratch
{
  int32_t *csv_err;
  uint64_t *len;
  uint8_t *text;
};

// the context's text block for C channels of text_stride bytes, for a call on s (scratch_acquire), and its parts
static int text_scratch_acquire(dega_hip_ctx *ctx, size_t C, size_t text_stride, hipStream_t s, TextScratch &t)
{
  const size_t head = round16(C * sizeof(int32_t)) + round16(C * sizeof(uint64_t));
  if (C > (SIZE_MAX - head) / text_stride)
    return fail(ctx, DEGA_ERROR_MEMORY, "csv: the text of the batch does not fit the address space", hipSuccess);
  const int ret = scratch_acquire(ctx, ctx->text, head + C * text_stride, s);
  if (ret != DEGA_OK)
    return ret;
  t.csv_err = (int32_t *)ctx->text.p;
  t.len = (uint64_t *)(ctx->text.p + round16(C * sizeof(int32_t)));
  t.text = ctx->text.p + head;
  return DEGA_OK;
}

// what dega_hip_lzmh_encode_dev would refuse, and the arrays of one level
static int check_lzmh_outputs(dega_hip_ctx *ctx, size_t C, const uint8_t *out, size_t cap, const uint64_t *out_bits, const int32_t *err)
{
  if ((cap & 15u) != 0 || cap < 48 || !aligned16(out))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh encode: cap must be a multiple of 16 (>= 48), out 16-byte aligned", hipSuccess);
  if (C != 0 && (out == nullptr || out_bits == nullptr || err == nullptr))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh encode: null output", hipSuccess);
  return DEGA_OK;
}

// render + LZMH encode + status on s; the text scratch is the caller's to guard (event protocol)
static int launch_csv_lzmh(dega_hip_ctx *ctx, const float *rows, size_t C, size_t T, size_t ld, unsigned decimals, size_t column, int separator_char,
                           const TextScratch &t, size_t text_stride, uint8_t *out, size_t cap, uint64_t *out_bits, uint64_t *text_len, int32_t *err,
                           hipStream_t s, bool *rendered, hipEvent_t rows_read, const uint64_t *count = nullptr)
{
  uint64_t *const len = text_len != nullptr ? text_len : t.len;
  int ret;
  if ((ret = launch_csv(ctx, rows, C, T, ld, decimals, column, separator_char, t.text, text_stride, len, t.csv_err, s, count)) != DEGA_OK)
    return ret;
  *rendered = true;
  if (rows_read != nullptr) // the caller's event for "`rows` may be overwritten"
    HIP_TRY(ctx, hipEventRecord(rows_read, s), DEGA_ERROR_LIBRARY_CALL);
  if ((ret = dega_hip_lzmh_encode_dev(ctx, t.text, text_stride, len, C, out, cap, out_bits, err, s)) != DEGA_OK)
    return ret;
  // A channel whose text did not fit its row was coded as the empty text: it reports the renderer's status and no stream.
  return launch_status(ctx, t.csv_err, C, err, out_bits, s);
}

static int zero_lzmh_outputs(dega_hip_ctx *ctx, size_t C, uint64_t *out_bits, uint64_t *text_len, int32_t *err, hipStream_t s)
{
  HIP_TRY(ctx, hipMemsetAsync(out_bits, 0, C * sizeof(uint64_t), s), DEGA_ERROR_LIBRARY_CALL);
  HIP_TRY(ctx, hipMemsetAsync(err, 0, C * sizeof(int32_t), s), DEGA_ERROR_LIBRARY_CALL);
  if (text_len != nullptr)
    HIP_TRY(ctx, hipMemsetAsync(text_len, 0, C * sizeof(uint64_t), s), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

extern "C" int dega_hip_lzmh_encode_f32_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, unsigned decimals, size_t column,
                                            int separator_char, size_t text_stride, uint8_t *out, size_t cap, uint64_t *out_bits, uint64_t *text_len,
                                            int32_t *err, void *stream)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  int ret;
  if ((ret = check_csv_options(ctx, C, ld, decimals, column, separator_char, text_stride)) != DEGA_OK)
    return ret;
  if ((ret = check_lzmh_outputs(ctx, C, out, cap, out_bits, err)) != DEGA_OK)
    return ret;
  if (C == 0)
    return DEGA_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  hipStream_t s = (hipStream_t)stream;
  if (T == 0)
    return zero_lzmh_outputs(ctx, C, out_bits, text_len, err, s);
  if (!f32_array(v_tc))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: v_tc must be a float32 device array", hipSuccess);
  if (ranges_overlap(out, C * cap, v_tc, image_bytes(T, ld, C)))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh encode: out overlaps v_tc", hipSuccess);
  TextScratch t;
  if ((ret = text_scratch_acquire(ctx, C, text_stride, s, t)) != DEGA_OK)
    return ret;
  bool rendered = false;
  ret = launch_csv_lzmh(ctx, v_tc, C, T, ld, decimals, column, separator_char, t, text_stride, out, cap, out_bits, text_len, err, s, &rendered, nullptr);
  if (rendered) // (whatever the later launches said: the renderer is on the stream and writes the scratch)
  {
    const int rel = scratch_release(ctx, ctx->text, s);
    if (rel != DEGA_OK)
      return rel;
  }
  return ret;
}

// `counted` as in aggregate_levels
static int lzmh_encode_levels(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, bool counted, const uint64_t *count,
                              const size_t *num_values, size_t K, unsigned decimals, size_t column, int separator_char, const size_t *text_stride,
                              uint8_t *const *out, const size_t *cap, uint64_t *const *out_bits, uint64_t *const *text_len, uint64_t *const *out_count,
                              int32_t *const *err, hipStream_t s)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (check_level_list(num_values, K) != DEGA_OK)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh encode levels: at most 8 levels, every num_values at least 1, none twice", hipSuccess);
  if (K == 0)
    return DEGA_OK;
  if (text_stride == nullptr || out == nullptr || cap == nullptr || out_bits == nullptr || err == nullptr || (counted && out_count == nullptr))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE,
                counted ? "lzmh encode levels: text_stride, out, cap, out_bits, out_count and err are arrays of K entries"
                        : "lzmh encode levels: text_stride, out, cap, out_bits and err are arrays of K entries",
                hipSuccess);
  int ret;
  size_t widest = 0;
  for (size_t k = 0; k < K; k++) // every level judged before the first launch
  {
    if ((ret = check_csv_options(ctx, C, ld, decimals, column, separator_char, text_stride[k])) != DEGA_OK)
      return ret;
    if ((ret = check_lzmh_outputs(ctx, C, out[k], cap[k], out_bits[k], err[k])) != DEGA_OK)
      return ret;
    for (size_t i = 0; i < k; i++)
      if (ranges_overlap(out[k], C * cap[k], out[i], C * cap[i]))
        return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh encode levels: two levels' outputs overlap", hipSuccess);
    widest = std::max(widest, text_stride[k]);
  }
  // every level through the aggregate stage, num_values 1 included: the chain has `aggregate` in it (+0.0f + v)
  LevelSums sums(num_values, K, T, ld, true);
  if (C == 0)
    return DEGA_OK;
  if (counted)
  {
    if ((ret = check_counts(ctx, C, T, count, out_count, K, err[0])) != DEGA_OK)
      return ret;
    for (size_t k = 0; k < K; k++)
      if (((uintptr_t)err[k] & 3u) != 0 || ((uintptr_t)out_bits[k] & 7u) != 0)
        return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh encode levels: misaligned output", hipSuccess);
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  if (T == 0 && count == nullptr)
  {
    for (size_t k = 0; k < K; k++)
      if ((ret = zero_lzmh_outputs(ctx, C, out_bits[k], text_len != nullptr ? text_len[k] : nullptr, err[k], s)) != DEGA_OK)
        return ret;
    return DEGA_OK;
  }
  // (a counted batch still launches at T = 0, where v_tc may be null)
  if (T != 0 && !f32_array(v_tc))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh encode levels: v_tc must be a float32 device array", hipSuccess);
  for (size_t k = 0; k < K && T != 0; k++)
    if (ranges_overlap(out[k], C * cap[k], v_tc, image_bytes(T, ld, C)))
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh encode levels: an output overlaps v_tc", hipSuccess);
  const size_t head = count != nullptr ? round4(C) : 0; // a counted batch: the aggregate pass's status (a count above T) in front of the sums
  if ((ret = scratch_acquire(ctx, ctx->sums, (head + std::max<size_t>(sums.floats, 4)) * sizeof(float), s)) != DEGA_OK)
    return ret;
  int32_t *const first = count != nullptr ? (int32_t *)ctx->sums.p : nullptr;
  sums.place((float *)ctx->sums.p + head);
  if ((ret = check_levels_dev(ctx, v_tc, C, T, ld, num_values, K, sums.a, sums.ldo)) != DEGA_OK)
    return ret;
  TextScratch t;
  if ((ret = text_scratch_acquire(ctx, C, widest, s, t)) != DEGA_OK) // the largest level's text; reused level after level in stream order
    return ret;
  bool rendered = false;
  ret = launch_aggregate_levels(ctx, v_tc, C, T, ld, count, num_values, K, sums.a, sums.ldo, out_count, first, s);
  for (size_t k = 0; k < K && ret == DEGA_OK; k++)
  {
    // uniform: the sums' event behind the last renderer, their last reader -- what follows it only reads the text;
    // counted: each level with its own counts, and the status launches read the head of the sums, so their event goes last
    ret = launch_csv_lzmh(ctx, sums.a[k], C, dega_hip_aggregate_rows(T, num_values[k]), ld, decimals, column, separator_char, t, text_stride[k], out[k], cap[k],
                          out_bits[k], text_len != nullptr ? text_len[k] : nullptr, err[k], s, &rendered,
                          count == nullptr && k + 1 == K ? ctx->sums.done : nullptr, count != nullptr ? out_count[k] : nullptr);
    if (count != nullptr && ret == DEGA_OK)
      ret = launch_status(ctx, first, C, err[k], out_bits[k], s);
  }
  // (recorded whatever the launches said; uniform, when all went well, the sums' event is already on the stream)
  int rel = scratch_release(ctx, ctx->sums, s, count == nullptr && ret == DEGA_OK);
  if (rel == DEGA_OK && rendered)
    rel = scratch_release(ctx, ctx->text, s);
  return rel != DEGA_OK ? rel : ret;
}

extern "C" int dega_hip_lzmh_encode_levels_f32_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const size_t *num_values, size_t K,
                                                   unsigned decimals, size_t column, int separator_char, const size_t *text_stride, uint8_t *const *out,
                                                   const size_t *cap, uint64_t *const *out_bits, uint64_t *const *text_len, int32_t *const *err,
                                                   void *stream)
{
  return lzmh_encode_levels(ctx, v_tc, C, T, ld, false, nullptr, num_values, K, decimals, column, separator_char, text_stride, out, cap, out_bits, text_len,
                            nullptr, err, (hipStream_t)stream);
}

extern "C" int dega_hip_lzmh_encode_levels_f32_var_dev(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, const uint64_t *count,
                                                       const size_t *num_values, size_t K, unsigned decimals, size_t column, int separator_char,
                                                       const size_t *text_stride, uint8_t *const *out, const size_t *cap, uint64_t *const *out_bits,
                                                       uint64_t *const *text_len, uint64_t *const *out_count, int32_t *const *err, void *stream)
{
  return lzmh_encode_levels(ctx, v_tc, C, T, ld, true, count, num_values, K, decimals, column, separator_char, text_stride, out, cap, out_bits, text_len,
                            out_count, err, (hipStream_t)stream);
}

// ---- decode csv (DCLib/src/csv.c:13-44): text as float32 series, alone and behind LZMH ------------------------------------

// The options of the stage and both layouts (everything but the pointers), for every entry point that reads.
static int check_csv_read_options(dega_hip_ctx *ctx, size_t C, size_t column, int separator_char, size_t stride, size_t ld)
{
  if (column == 0 || separator_char < 0 || separator_char > 255)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: column at least 1, separator_char one byte", hipSuccess);
  if (stride < 16 || (stride & 15u) != 0 || stride > 0x7FFFFFF0u)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: stride must be a multiple of 16 (16 .. 0x7FFFFFF0)", hipSuccess);
  if (ld < C)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: ld < C", hipSuccess);
  return DEGA_OK;
}

// The arguments have been checked; C is not 0.
static int launch_csv_read(dega_hip_ctx *ctx, const uint8_t *text, size_t stride, const uint64_t *len, size_t C, size_t column, int separator_char,
                           float *v_tc, size_t max_T, size_t ld, uint64_t *out_count, int32_t *err, hipStream_t s)
{
  if (!launch(csv_read_args(text, stride, len, C, column, separator_char, v_tc, max_T, ld, out_count, err), OnStream{s}))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: too many channels for one launch", hipSuccess);
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

static int check_csv_read_outputs(dega_hip_ctx *ctx, const float *v_tc, size_t max_T, const uint64_t *out_count, const int32_t *err)
{
  if (out_count == nullptr || err == nullptr || ((uintptr_t)out_count & 7u) != 0 || ((uintptr_t)err & 3u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: out_count and err must be arrays", hipSuccess);
  if (max_T != 0 && !f32_array(v_tc))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: v_tc must be a float32 array", hipSuccess);
  return DEGA_OK;
}

extern "C" int dega_hip_csv_read_dev(dega_hip_ctx *ctx, const uint8_t *text, size_t stride, const uint64_t *len, size_t C, size_t column,
                                     int separator_char, float *v_tc, size_t max_T, size_t ld, uint64_t *out_count, int32_t *err, void *stream)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  int ret;
  if ((ret = check_csv_read_options(ctx, C, column, separator_char, stride, ld)) != DEGA_OK)
    return ret;
  if (!aligned16(text))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: text must be 16-byte aligned", hipSuccess);
  if (C == 0)
    return DEGA_OK;
  if (text == nullptr || len == nullptr || ((uintptr_t)len & 7u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: text and len must be device arrays", hipSuccess);
  if ((ret = check_csv_read_outputs(ctx, v_tc, max_T, out_count, err)) != DEGA_OK)
    return ret;
  if (max_T != 0 && ranges_overlap(text, C * stride, v_tc, image_bytes(max_T, ld, C)))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: v_tc overlaps text", hipSuccess);
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  return launch_csv_read(ctx, text, stride, len, C, column, separator_char, v_tc, max_T, ld, out_count, err, (hipStream_t)stream);
}

// ---- the same for few long channels: one channel's text split over lanes (csv_read_split_kernels.hpp) -----------------------

extern "C" size_t dega_hip_csv_read_split_block_bytes(size_t C, size_t stride)
{
  return csv_read_split_block_bytes(C, stride);
}

extern "C" int dega_hip_csv_read_split_dev(dega_hip_ctx *ctx, const uint8_t *text, size_t stride, const uint64_t *len, size_t C, size_t column,
                                           int separator_char, float *v_tc, size_t max_T, size_t ld, uint64_t *out_count, int32_t *err,
                                           size_t block_bytes, void *stream)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  int ret;
  if ((ret = check_csv_read_options(ctx, C, column, separator_char, stride, ld)) != DEGA_OK)
    return ret;
  if (block_bytes == 0)
    block_bytes = csv_read_split_block_bytes(C, stride);
  if (block_bytes < 16 || (block_bytes & 15u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read split: block_bytes must be 0 or a multiple of 16 (at least 16)", hipSuccess);
  if (!aligned16(text))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: text must be 16-byte aligned", hipSuccess);
  if (C == 0)
    return DEGA_OK;
  if (text == nullptr || len == nullptr || ((uintptr_t)len & 7u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: text and len must be device arrays", hipSuccess);
  if ((ret = check_csv_read_outputs(ctx, v_tc, max_T, out_count, err)) != DEGA_OK)
    return ret;
  if (max_T != 0 && ranges_overlap(text, C * stride, v_tc, image_bytes(max_T, ld, C)))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: v_tc overlaps text", hipSuccess);
  const size_t blocks = csv_read_split_blocks(stride, block_bytes);
  if (C > SIZE_MAX / sizeof(uint32_t) / blocks)
    return fail(ctx, DEGA_ERROR_MEMORY, "csv read split: the blocks of the batch do not fit the address space", hipSuccess);
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  hipStream_t s = (hipStream_t)stream;
  if ((ret = scratch_acquire(ctx, ctx->split, C * blocks * sizeof(uint32_t), s)) != DEGA_OK)
    return ret;
  const CsvReadArgs r = csv_read_args(text, stride, len, C, column, separator_char, v_tc, max_T, ld, out_count, err);
  if (!launch(csv_read_split_args(r, block_bytes, (uint32_t *)ctx->split.p), OnStream{s}))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read split: too many blocks for one launch", hipSuccess); // (nothing launched)
  const hipError_t launched = hipGetLastError();
  ret = launched == hipSuccess ? DEGA_OK : fail(ctx, DEGA_ERROR_LIBRARY_CALL, "csv read split: launch", launched);
  // (recorded whatever the launches said: the first may be on the stream and writes the scratch)
  const int rel = scratch_release(ctx, ctx->split, s);
  return rel != DEGA_OK ? rel : ret;
}

extern "C" int dega_hip_lzmh_decode_f32_dev(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t text_stride,
                                            size_t column, int separator_char, float *v_tc, size_t max_T, size_t ld, uint64_t *out_count,
                                            uint64_t *text_len, int32_t *err, void *stream)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  int ret;
  if ((ret = check_csv_read_options(ctx, C, column, separator_char, text_stride, ld)) != DEGA_OK)
    return ret;
  if (cap < 4 || (cap & 3u) != 0 || ((uintptr_t)in & 3u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh decode: cap must be a multiple of 4, in 4-byte aligned", hipSuccess);
  if (C == 0)
    return DEGA_OK;
  if (in == nullptr || in_bits == nullptr || ((uintptr_t)in_bits & 7u) != 0 || ((uintptr_t)text_len & 7u) != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh decode: in and in_bits must be device arrays", hipSuccess);
  if ((ret = check_csv_read_outputs(ctx, v_tc, max_T, out_count, err)) != DEGA_OK)
    return ret;
  if (max_T != 0 && ranges_overlap(in, C * cap, v_tc, image_bytes(max_T, ld, C)))
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh decode: v_tc overlaps in", hipSuccess);
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  hipStream_t s = (hipStream_t)stream;
  TextScratch t;
  if ((ret = text_scratch_acquire(ctx, C, text_stride, s, t)) != DEGA_OK)
    return ret;
  uint64_t *const len = text_len != nullptr ? text_len : t.len;
  // (t.csv_err holds the LZMH decoder's status here)
  ret = dega_hip_lzmh_decode_dev(ctx, in, cap, in_bits, C, t.text, text_stride, len, t.csv_err, s);
  if (ret == DEGA_OK)
    ret = launch_csv_read(ctx, t.text, text_stride, len, C, column, separator_char, v_tc, max_T, ld, out_count, err, s);
  // A channel whose text did not fit its row was read as the empty text: it reports the LZMH decoder's status and no value.
  if (ret == DEGA_OK)
    ret = launch_status(ctx, t.csv_err, C, err, out_count, s);
  // (recorded whatever the launches said: the decoder may be on the stream and writes the scratch)
  const int rel = scratch_release(ctx, ctx->text, s);
  return rel != DEGA_OK ? rel : ret;
}

// ---- host-pointer entry points: the pipeline and the multi-device group ------------------------------------------------------
#include "dega_pipeline.hpp"
