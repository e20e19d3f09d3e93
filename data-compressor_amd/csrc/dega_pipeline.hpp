// dega_pipeline.hpp -- the host-pointer entry points of libdega_hip.so (included by dega_hip.hip).
//
// What DCCLI's stage loop hands a codec is host memory (DCCLI/src/cli.c:430-466); a batch of C channels therefore has to
// cross PCIe twice.  Everything here is about doing that at link speed:
//   * a batch is cut into chunks of channels; every chunk has a stream of its own that carries   H2D of its columns ->
//     encode kernel -> offsets -> gather -> D2H of its packed streams   (decode: the mirror image), so that the copy
//     engines and the kernels of different chunks overlap.  One channel of T samples takes the same time whatever the
//     batch size (the coder is serial per channel), so chunks also have to run side by side -- they do, on their streams;
//   * nothing is allocated per call: device buffers and the small pinned mirrors belong to the context and only grow;
//   * only stream bytes come back (packed, channel order); slabs are sized for the usual case (no longer than the
//     samples) and a chunk that does not fit is redone with worst-case slabs -- never a worst-case memset or D2H.
// A group runs one such pipeline per device on a host thread each, over contiguous channel ranges; the packed streams
// of the devices are concatenated by the host (each device copies to its final place once the sizes in front of it are
// known).  No collective, no peer traffic (channels are independent: diff.c:11, bac.c:150).
#pragma once

#include <sched.h>

struct GrowDev // device buffer that only grows
{
  void *p = nullptr;
  size_t cap = 0;
  hipError_t need(size_t n)
  {
    if (n <= cap)
      return hipSuccess;
    if (p != nullptr)
      (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = n + n / 8 + 4096;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess)
    {
      (void)hipGetLastError();
      want = n;
      e = hipMalloc(&p, want);
    }
    if (e == hipSuccess)
      cap = want;
    else
      p = nullptr;
    return e;
  }
  void release()
  {
    if (p != nullptr)
      (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct GrowPin // pinned host buffer that only grows
{
  void *p = nullptr;
  size_t cap = 0;
  hipError_t need(size_t n)
  {
    if (n <= cap)
      return hipSuccess;
    if (p != nullptr)
      (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = n + n / 8 + 4096;
    const hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess)
      cap = want;
    else
      p = nullptr;
    return e;
  }
  void release()
  {
    if (p != nullptr)
      (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

// A few host threads that copy rows between the caller's (pageable, pitched) arrays and the pinned staging ring; eight of
// them with cache-bypassing stores keep up with the PCIe link (~57 GB/s) on pitched rows.
// memcpy whose stores bypass the cache: the destination (a staging buffer the DMA engine reads next, or the caller's
// array) is not read back by this thread, and ordinary stores would first fetch every destination line
static void copy_streaming(uint8_t *dst, const uint8_t *src, size_t n)
{
  typedef long long v2 __attribute__((vector_size(16), aligned(16)));
  typedef long long v2u __attribute__((vector_size(16), aligned(1)));
  if (n < 4096)
  {
    memcpy(dst, src, n);
    return;
  }
  const size_t head = (16 - ((uintptr_t)dst & 15)) & 15;
  memcpy(dst, src, head);
  dst += head;
  src += head;
  n -= head;
  const size_t body = n & ~(size_t)63;
  for (size_t i = 0; i < body; i += 64)
  {
    const v2 a = *(const v2u *)(src + i), b = *(const v2u *)(src + i + 16), c = *(const v2u *)(src + i + 32), d = *(const v2u *)(src + i + 48);
    __builtin_nontemporal_store(a, (v2 *)(dst + i));
    __builtin_nontemporal_store(b, (v2 *)(dst + i + 16));
    __builtin_nontemporal_store(c, (v2 *)(dst + i + 32));
    __builtin_nontemporal_store(d, (v2 *)(dst + i + 48));
  }
  memcpy(dst + body, src + body, n - body);
}

struct CopyPool
{
  static constexpr int N = 8; // (measured again in round 3 with 12 and 16 threads on a 16-core share: no difference -- the ring is not the limit)
  std::thread th[N];
  std::mutex m;
  std::condition_variable cv_work, cv_done;
  std::function<void(int)> job;
  uint64_t generation = 0;
  int pending = 0;
  bool stop = false, started = false;

  void start()
  {
    if (started)
      return;
    started = true;
    for (int i = 0; i < N; i++)
      th[i] = std::thread([this, i] {
        uint64_t seen = 0;
        for (;;)
        {
          std::function<void(int)> f;
          {
            std::unique_lock<std::mutex> lk(m);
            cv_work.wait(lk, [&] { return stop || generation != seen; });
            if (stop)
              return;
            seen = generation;
            f = job;
          }
          f(i);
          {
            std::lock_guard<std::mutex> lk(m);
            if (--pending == 0)
              cv_done.notify_all();
          }
        }
      });
  }
  void run(const std::function<void(int)> &f) // f(part) for part = 0 .. N-1, returns when all are done
  {
    start();
    std::unique_lock<std::mutex> lk(m);
    job = f;
    pending = N;
    generation++;
    cv_work.notify_all();
    cv_done.wait(lk, [&] { return pending == 0; });
  }
  ~CopyPool()
  {
    if (!started)
      return;
    {
      std::lock_guard<std::mutex> lk(m);
      stop = true;
    }
    cv_work.notify_all();
    for (int i = 0; i < N; i++)
      th[i].join();
  }
  // rows x row_bytes from src (pitch sp) to dst (pitch dp), split over the threads
  void copy_rows(uint8_t *dst, size_t dp, const uint8_t *src, size_t sp, size_t row_bytes, size_t rows)
  {
    if (rows * row_bytes < ((size_t)1 << 20))
    {
      for (size_t r = 0; r < rows; r++)
        memcpy(dst + r * dp, src + r * sp, row_bytes);
      return;
    }
    if (rows >= (size_t)N)
      run([=](int part) {
        const size_t r0 = rows * (size_t)part / N, r1 = rows * ((size_t)part + 1) / N;
        if (dp == row_bytes && sp == row_bytes)
          copy_streaming(dst + r0 * dp, src + r0 * sp, (r1 - r0) * row_bytes);
        else
          for (size_t r = r0; r < r1; r++)
            copy_streaming(dst + r * dp, src + r * sp, row_bytes);
        __builtin_ia32_sfence();
      });
    else // few long rows: split each row
      run([=](int part) {
        const size_t b0 = row_bytes * (size_t)part / N, b1 = row_bytes * ((size_t)part + 1) / N;
        for (size_t r = 0; r < rows; r++)
          copy_streaming(dst + r * dp + b0, src + r * sp + b0, b1 - b0);
        __builtin_ia32_sfence();
      });
  }
};

// The pinned staging ring between pageable host memory and the device: NB buffers in flight, each with the event of the
// DMA that last used it.  Uploads: rows are packed into a buffer by the copy threads, then one contiguous DMA.  Downloads:
// one contiguous DMA into a buffer, and when the ring comes round (or at drain) its rows are copied out to their place.
struct Stager
{
  static constexpr int NB = 6;
  static constexpr size_t SB = (size_t)24 << 20;
  void *buf[NB] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  hipEvent_t ev[NB] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool busy[NB] = {false, false, false, false, false, false};
  struct Out
  {
    uint8_t *dst = nullptr; // where the buffer's rows go when its download has landed (nullptr: nothing to do)
    size_t pitch = 0, row_bytes = 0, rows = 0;
  } out[NB];
  int next = 0;
  CopyPool pool;

  hipError_t init()
  {
    for (int i = 0; i < NB; i++)
      if (buf[i] == nullptr)
      {
        hipError_t e = hipHostMalloc(&buf[i], SB, hipHostMallocDefault);
        if (e != hipSuccess)
          return e;
        if ((e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming)) != hipSuccess)
          return e;
      }
    return hipSuccess;
  }
  void release()
  {
    for (int i = 0; i < NB; i++)
    {
      if (buf[i] != nullptr)
        (void)hipHostFree(buf[i]);
      if (ev[i] != nullptr)
        (void)hipEventDestroy(ev[i]);
      buf[i] = nullptr;
      ev[i] = nullptr;
    }
  }
  hipError_t settle(int b) // wait for buffer b's DMA; finish its download
  {
    if (!busy[b])
      return hipSuccess;
    const hipError_t e = hipEventSynchronize(ev[b]);
    busy[b] = false;
    if (e != hipSuccess)
      return e;
    if (out[b].dst != nullptr)
      pool.copy_rows(out[b].dst, out[b].pitch, (const uint8_t *)buf[b], out[b].row_bytes, out[b].row_bytes, out[b].rows);
    out[b].dst = nullptr;
    return hipSuccess;
  }
  hipError_t drain()
  {
    hipError_t first = hipSuccess;
    for (int k = 0; k < NB; k++)
    {
      const hipError_t e = settle((next + k) % NB);
      if (e != hipSuccess && first == hipSuccess)
        first = e;
    }
    return first;
  }
  // host rows (pitch sp) -> contiguous rows at dev
  hipError_t upload(hipStream_t s, void *dev, const uint8_t *src, size_t sp, size_t row_bytes, size_t rows)
  {
    hipError_t e;
    if ((e = init()) != hipSuccess)
      return e;
    if (row_bytes == 0 || rows == 0)
      return hipSuccess;
    if (row_bytes > SB) // a single row longer than a buffer (one long channel): treat the block as a byte string
    {
      if (rows != 1 && sp != row_bytes)
        return hipErrorInvalidValue;
      const size_t total = row_bytes * rows;
      for (size_t o = 0; o < total; o += SB)
        if ((e = upload(s, (uint8_t *)dev + o, src + o, std::min(SB, total - o), std::min(SB, total - o), 1)) != hipSuccess)
          return e;
      return hipSuccess;
    }
    const size_t per = std::max<size_t>(1, SB / row_bytes);
    for (size_t r0 = 0; r0 < rows; r0 += per)
    {
      const size_t n = std::min(per, rows - r0);
      const int b = next;
      next = (next + 1) % NB;
      if ((e = settle(b)) != hipSuccess)
        return e;
      pool.copy_rows((uint8_t *)buf[b], row_bytes, src + r0 * sp, sp, row_bytes, n);
      if ((e = hipMemcpyAsync((uint8_t *)dev + r0 * row_bytes, buf[b], n * row_bytes, hipMemcpyHostToDevice, s)) != hipSuccess)
        return e;
      if ((e = hipEventRecord(ev[b], s)) != hipSuccess)
        return e;
      busy[b] = true;
    }
    return hipSuccess;
  }
  // contiguous rows at dev -> host rows (pitch dp); complete only after drain()
  hipError_t download(hipStream_t s, uint8_t *dst, size_t dp, const void *dev, size_t row_bytes, size_t rows)
  {
    hipError_t e;
    if ((e = init()) != hipSuccess)
      return e;
    if (row_bytes == 0 || rows == 0)
      return hipSuccess;
    if (row_bytes > SB)
    {
      if (rows != 1 && dp != row_bytes)
        return hipErrorInvalidValue;
      const size_t total = row_bytes * rows;
      for (size_t o = 0; o < total; o += SB)
        if ((e = download(s, dst + o, std::min(SB, total - o), (const uint8_t *)dev + o, std::min(SB, total - o), 1)) != hipSuccess)
          return e;
      return hipSuccess;
    }
    const size_t per = std::max<size_t>(1, SB / row_bytes);
    for (size_t r0 = 0; r0 < rows; r0 += per)
    {
      const size_t n = std::min(per, rows - r0);
      const int b = next;
      next = (next + 1) % NB;
      if ((e = settle(b)) != hipSuccess)
        return e;
      if ((e = hipMemcpyAsync(buf[b], (const uint8_t *)dev + r0 * row_bytes, n * row_bytes, hipMemcpyDeviceToHost, s)) != hipSuccess)
        return e;
      if ((e = hipEventRecord(ev[b], s)) != hipSuccess)
        return e;
      busy[b] = true;
      out[b].dst = dst + r0 * dp;
      out[b].pitch = dp;
      out[b].row_bytes = row_bytes;
      out[b].rows = n;
    }
    return hipSuccess;
  }
};

// true when p is host memory the runtime has pinned (hipHostMalloc / hipHostRegister): DMA can use it in place
static bool is_pinned(const void *p)
{
  if (p == nullptr)
    return false;
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess)
  {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

// Per-chunk small arrays, same layout on the device and in the pinned mirror
struct MetaView
{
  uint64_t *bits, *offsets, *counts;
  int32_t *err;
  static size_t bytes(size_t n)
  {
    return (3 * n + 1) * sizeof(uint64_t) + n * sizeof(int32_t);
  }
  MetaView(void *base, size_t n)
  {
    bits = (uint64_t *)base;
    offsets = bits + n;
    counts = offsets + n + 1;
    err = (int32_t *)(counts + n);
  }
};

struct Slot
{
  hipStream_t s = nullptr;
  GrowDev a, b, meta; // encode: a = samples, then the packed streams; b = slabs.  decode: a = packed streams, b = slabs, c = samples
  GrowDev c;          // (encode at coarser granularities: c = the fine readings as uploaded, later the packed streams; a = the levels' sums)
  GrowPin hmeta, stage;
  // few, long channels: encode uploads the rows in bands and codes every band as it lands (one launch per band, the lanes'
  // state saved in between: EncodeArgs::seg_state); decode downloads in bands beside the running kernel.  The copies'
  // stream, one event per band, the state of the encode launches / the waves' progress words of the decode kernel.
  hipStream_t s2 = nullptr;
  std::vector<hipEvent_t> band_ev;
  hipEvent_t reuse_ev = nullptr;
  GrowDev seg_state;
  GrowPin progress_values;
};

constexpr int MAX_SLOTS = 16;

struct Pipeline
{
  Slot slot[MAX_SLOTS];
  hipStream_t up = nullptr; // decode: the chunks' packed streams go up one after the other on this stream (each at the link's full rate)
  GrowDev redo_slabs, redo_packed, redo_meta;
  GrowPin redo_hmeta;
  Stager stager;
};

// Host rows <-> device, by the faster route: in place when the caller's memory is pinned and the rows are long enough for
// the DMA engine's 2-D copies (they cost about a microsecond per row), through the staging ring otherwise.
constexpr size_t DIRECT_2D_MIN_ROW = (size_t)16 << 10;
static hipError_t rows_to_device(Pipeline *pl, hipStream_t s, void *dev, const uint8_t *src, size_t sp, size_t row_bytes, size_t rows, bool pinned)
{
  if (rows == 0 || row_bytes == 0)
    return hipSuccess;
  if (pinned && sp == row_bytes)
    return hipMemcpyAsync(dev, src, rows * row_bytes, hipMemcpyHostToDevice, s);
  if (pinned && row_bytes >= DIRECT_2D_MIN_ROW)
    return hipMemcpy2DAsync(dev, row_bytes, src, sp, row_bytes, rows, hipMemcpyHostToDevice, s);
  return pl->stager.upload(s, dev, src, sp, row_bytes, rows);
}
static hipError_t rows_to_host(Pipeline *pl, hipStream_t s, uint8_t *dst, size_t dp, const void *dev, size_t row_bytes, size_t rows, bool pinned)
{
  if (rows == 0 || row_bytes == 0)
    return hipSuccess;
  if (pinned && dp == row_bytes)
    return hipMemcpyAsync(dst, dev, rows * row_bytes, hipMemcpyDeviceToHost, s);
  if (pinned && row_bytes >= DIRECT_2D_MIN_ROW)
    return hipMemcpy2DAsync(dst, dp, dev, row_bytes, row_bytes, rows, hipMemcpyDeviceToHost, s);
  return pl->stager.download(s, dst, dp, dev, row_bytes, rows);
}

// DEGA_PIPELINE_TRACE=1: host timestamps of the pipeline's stages on stderr (measurement aid)
static bool trace_on()
{
  static const int on = getenv("DEGA_PIPELINE_TRACE") != nullptr ? 1 : 0;
  return on != 0;
}
static double trace_now()
{
  struct timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
#define TRACE(...) do { if (trace_on()) { fprintf(stderr, "[dega %10.3f ms] ", trace_now()); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

static void pipeline_destroy(Pipeline *p)
{
  if (p == nullptr)
    return;
  for (Slot &sl : p->slot)
  {
    if (sl.s != nullptr)
      (void)hipStreamDestroy(sl.s);
    if (sl.s2 != nullptr)
      (void)hipStreamDestroy(sl.s2);
    for (hipEvent_t e : sl.band_ev)
      (void)hipEventDestroy(e);
    sl.band_ev.clear();
    if (sl.reuse_ev != nullptr)
      (void)hipEventDestroy(sl.reuse_ev);
    sl.seg_state.release();
    sl.progress_values.release();
    sl.a.release();
    sl.b.release();
    sl.c.release();
    sl.meta.release();
    sl.hmeta.release();
    sl.stage.release();
  }
  if (p->up != nullptr)
    (void)hipStreamDestroy(p->up);
  p->redo_slabs.release();
  p->redo_packed.release();
  p->redo_meta.release();
  p->redo_hmeta.release();
  p->stager.release();
  delete p;
}

static int pipeline_get(dega_hip_ctx *ctx, Pipeline **out)
{
  if (ctx->pipe == nullptr)
    ctx->pipe = new Pipeline();
  *out = ctx->pipe;
  return DEGA_OK;
}

static int slot_stream(dega_hip_ctx *ctx, Slot &sl)
{
  if (sl.s == nullptr)
    HIP_TRY(ctx, hipStreamCreateWithFlags(&sl.s, hipStreamNonBlocking), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

static size_t sample_bytes(const Shape &j)
{
  return j.samples == DEGA_SAMPLES_I64 ? 8 : 4;
}

static size_t worst_cap(const Shape &j)
{
  return j.valuesize > 32 ? dega_hip_worst_case_bytes64(j.T) : dega_hip_worst_case_bytes(j.T);
}

// slab bytes per channel for the first attempt: a stream no longer than its samples (plus the coder's tail)
static size_t usual_cap(const Shape &j)
{
  const size_t vbytes = j.valuesize > 32 ? 8 : 4;
  const size_t c = (j.T * vbytes + 64 + 3) & ~(size_t)3;
  return std::min(c, worst_cap(j));
}

struct ChunkPlan
{
  size_t chunk_channels; // multiple of 512 unless the batch is one chunk
  size_t nchunks;
  int nslots;
};

// Chunks: enough of them to overlap copies and kernels (about 64 MiB of samples each, at most MAX_SLOTS at a time), whole
// workgroups of channels, and -- when the batch does not fit the device beside its slabs -- as many slots as fit.
static ChunkPlan plan_chunks(size_t C, size_t bytes_per_channel_in, size_t bytes_per_channel_dev, int want_all_resident, size_t most = 8)
{
  ChunkPlan p;
  const size_t total = C * bytes_per_channel_in;
  size_t n = total / ((size_t)64 << 20);
  n = std::max<size_t>(1, std::min<size_t>(n, most));
  if (getenv("DEGA_PIPELINE_CHUNKS") != nullptr) // measurement knob
    n = std::max(1, atoi(getenv("DEGA_PIPELINE_CHUNKS")));
  if (C <= 512)
    n = 1;
  size_t cc = (C + n - 1) / n;
  if (n > 1)
    cc = std::max<size_t>((cc + 511) / 512 * 512, std::min<size_t>(C, 8192)); // rows of a chunk: 32 KiB or more (copies of narrow rows are slow: two chunks of 4 096 channels took 81 ms where one of 8 192 takes 66)
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess)
    free_b = (size_t)8 << 30;
  const size_t budget = free_b / 10 * 8;
  while (cc > 512 && cc * bytes_per_channel_dev > budget) // a single chunk must fit
    cc = (cc / 2 + 511) / 512 * 512;
  p.chunk_channels = std::max<size_t>(cc, 1);
  p.nchunks = C == 0 ? 0 : (C + p.chunk_channels - 1) / p.chunk_channels;
  size_t fit = std::max<size_t>(1, budget / std::max<size_t>(1, p.chunk_channels * bytes_per_channel_dev));
  p.nslots = (int)std::min<size_t>(std::min<size_t>(fit, MAX_SLOTS), std::max<size_t>(p.nchunks, 1));
  if (want_all_resident && (size_t)p.nslots < p.nchunks)
    p.nslots = -1; // the caller has to split the batch
  return p;
}

// Chunk k of a share of C channels: its channels [c0, c0 + n) and the slot it runs on
struct Chunk
{
  size_t c0 = 0, n = 0;
  int slot = 0;
  void place(const ChunkPlan &plan, size_t C, size_t k)
  {
    c0 = k * plan.chunk_channels;
    n = std::min(plan.chunk_channels, C - c0);
    slot = (int)(k % (size_t)plan.nslots);
  }
};

// The software pipeline over a share's chunks: the first stage of chunk k is enqueued `ahead` chunks before the second
// stage of the same chunk.  Chunk k + nslots reuses the slot of chunk k, so ahead <= nslots and the second stage of
// chunk k - ahead goes BEFORE the first stage of chunk k: a slot is reused only after its previous chunk's second stage.
template <class Stage1, class Stage2>
static int run_chunks(size_t nchunks, size_t ahead, Stage1 stage1, Stage2 stage2)
{
  int ret;
  for (size_t k = 0; k < nchunks + ahead; k++)
  {
    if (k >= ahead && (ret = stage2(k - ahead)) != DEGA_OK)
      return ret;
    if (k < nchunks && (ret = stage1(k)) != DEGA_OK)
      return ret;
  }
  return DEGA_OK;
}

// The loop of the synchronous host forms: chunks of channels through the context's first slot, one after the other, as
// many channels at a time as keep what a chunk holds on the device (bytes_per_channel each, never 0) under a gigabyte.
// body(pl, sl, c0, n) grows the slot's buffers, uploads, launches and downloads channels [c0, c0 + n); every chunk starts
// on an idle stream and ends with the staging ring's downloads in their place.
template <class Body>
static int first_slot_chunks(dega_hip_ctx *ctx, size_t C, size_t bytes_per_channel, Body body)
{
  int ret;
  Pipeline *pl;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  if ((ret = pipeline_get(ctx, &pl)) != DEGA_OK)
    return ret;
  Slot &sl = pl->slot[0];
  if ((ret = slot_stream(ctx, sl)) != DEGA_OK)
    return ret;
  size_t budget = (size_t)1 << 30;
  if (const char *e = getenv("DEGA_HOST_CHUNK_BYTES")) // measurement / test knob: the budget in bytes, at least 1
    budget = std::max<size_t>(1, (size_t)strtoull(e, nullptr, 10));
  size_t step = std::max<size_t>(1, budget / bytes_per_channel);
  if (step >= 4)
    step = step / 4 * 4; // whole 16-byte units of float32 columns: the chunks' images stay on the 16-byte path
  for (size_t c0 = 0; c0 < C; c0 += step)
  {
    HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL);
    if ((ret = body(pl, sl, c0, std::min(step, C - c0))) != DEGA_OK)
      return ret;
    HIP_TRY(ctx, pl->stager.drain(), DEGA_ERROR_LIBRARY_CALL);
  }
  HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

// everything the chunks left in flight: the staging ring's downloads to their place, then the slots' streams
static int finish_slots(dega_hip_ctx *ctx, Pipeline *pl, int nslots)
{
  HIP_TRY(ctx, pl->stager.drain(), DEGA_ERROR_LIBRARY_CALL);
  for (int s = 0; s < nslots; s++)
    if (pl->slot[s].s != nullptr)
      HIP_TRY(ctx, hipStreamSynchronize(pl->slot[s].s), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

// Rows per band when a chunk's samples cross the link in bands (0: in one piece, the usual way): encode codes every band
// with a launch of its own as soon as it has landed -- plain stream order, an event per band; nothing on the device ever
// waits for the host -- and decode sends every band home as soon as all waves have stored it.  Worth it when the channels
// are long (a launch per band has its fixed costs); bands end on multiples of 32 rows (whole 128-byte lines of the device
// array) and are about 32 MiB each.
static size_t band_rows_of(const ChunkPlan &plan, const Shape &j, size_t row_bytes)
{
  size_t band_bytes = (size_t)32 << 20, min_T = 4096;
  if (const char *e = getenv("DEGA_PIPELINE_BAND_BYTES")) // measurement / test knob: 0 = no bands, else the size of a band
  {
    band_bytes = (size_t)strtoull(e, nullptr, 10);
    min_T = 64;
  }
  (void)plan; // (any number of chunks: a chunk's kernels start with its first band, so only the last band's kernel and the
              //  last chunk's download are left over when the last byte has gone up)
  if (band_bytes == 0 || j.T < min_T || row_bytes == 0)
    return 0;
  size_t rows = std::max<size_t>(band_bytes / row_bytes, 32);
  rows = (rows + 31) / 32 * 32;
  return rows >= j.T ? 0 : rows;
}

// ---- encode ------------------------------------------------------------------------------------------------------------

// The packed outputs of a call (of one device's share of it; of one level), every codec's: streams back to back
struct PackedOut
{
  uint8_t *packed = nullptr;
  size_t packed_cap = 0;
  uint64_t *offsets = nullptr; // channel c at packed[offsets[c] .. offsets[c+1]); C + 1 entries, relative to the share
  uint64_t *bits = nullptr;
  int32_t *err = nullptr;
  uint64_t total = 0; // out: packed bytes of the chunks handed out so far, in the end of the share (the size needed when full)
  bool full = false;  // out: packed_cap was too small; the share was sized, not delivered (means nothing where no buffer was given)
};

static PackedOut packed_out(uint8_t *packed, size_t packed_cap, uint64_t *offsets, uint64_t *bits, int32_t *err)
{
  PackedOut out;
  out.packed = packed;
  out.packed_cap = packed_cap;
  out.offsets = offsets;
  out.bits = bits;
  out.err = err;
  return out;
}

struct EncodeSink : PackedOut // the plain encoder's: packed mode, or
{
  uint8_t *slabs = nullptr; // slab mode: channel c at slabs + c * slab_cap
  size_t slab_cap = 0;
};

static Shape chunk_shape(const Shape &j, size_t n) // n channels of a batch as a time-major image of their own on the device
{
  Shape cj = j;
  cj.C = n;
  cj.ld = n;
  return cj;
}

// ---- the encode tail, every codec's: from the bit lengths of a chunk's streams on the device to their bytes on the host ----

// Sizes on their way home: the streams' offsets from their bit lengths (dm), and -- where the chunk has one set of the
// small arrays -- the set into its pinned mirror
static int sizes_home(dega_hip_ctx *ctx, hipStream_t s, const MetaView &dm, size_t n, void *mirror)
{
  hipLaunchKernelGGL(dega_offsets_kernel, dim3(1), dim3(1024), 0, s, dm.bits, n, dm.offsets);
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  if (mirror != nullptr)
    HIP_TRY(ctx, hipMemcpyAsync(mirror, dm.bits, MetaView::bytes(n), hipMemcpyDeviceToHost, s), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

// n streams between their slabs (channel i at slabs + i * cap) and back to back at `packed`, by offsets[n + 1] on the device
static int launch_gather(dega_hip_ctx *ctx, hipStream_t s, const void *slabs, size_t cap, const uint64_t *offsets, size_t n, void *packed, bool scatter = false)
{
  GatherArgs g{(const uint8_t *)slabs, cap, offsets, n, (uint8_t *)packed};
  if (scatter)
    hipLaunchKernelGGL(dega_scatter_kernel, dim3((unsigned)((n + WAVES - 1) / WAVES)), dim3(BLOCK), 0, s, g);
  else
    hipLaunchKernelGGL(dega_gather_kernel, dim3((unsigned)((n + WAVES - 1) / WAVES)), dim3(BLOCK), 0, s, g);
  HIP_TRY(ctx, hipGetLastError(), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}
static int launch_scatter(dega_hip_ctx *ctx, hipStream_t s, void *slabs, size_t cap, const uint64_t *offsets, size_t n, const void *packed)
{
  return launch_gather(ctx, s, slabs, cap, offsets, n, const_cast<void *>(packed), true);
}

// Chunk out, the host's half: the sizes of channels [c0, c0 + n) are on the host (hm, offsets relative to the chunk).  Hands
// out bits / err / offsets at the running total; true when the chunk's bytes are to go to out.packed + base now -- there are
// some, and they and everything before them fit (after the first chunk that does not, the rest is only sized: the caller
// learns what it needs).
static bool chunk_sized(PackedOut &out, size_t c0, size_t n, const MetaView &hm, uint64_t &base)
{
  base = out.total;
  for (size_t i = 0; i < n; i++)
  {
    out.bits[c0 + i] = hm.bits[i];
    out.err[c0 + i] = hm.err[i];
  }
  if (out.offsets != nullptr)
    for (size_t i = 0; i < n; i++)
      out.offsets[c0 + i] = base + hm.offsets[i];
  out.total += hm.offsets[n];
  out.full = out.full || out.total > out.packed_cap;
  return !out.full && hm.offsets[n] > 0;
}

// Chunk out, the device's half: the chunk's `total` bytes are gathered from (slabs, cap) into dev -- a buffer of the slot
// that is free by now -- and sent to dst; the bytes of a chunk that was redone are on the host already (redo) and copied.
static int chunk_home(dega_hip_ctx *ctx, Pipeline *pl, hipStream_t s, uint8_t *dst, bool dst_pinned, size_t total, const std::vector<uint8_t> *redo,
                      const void *slabs, size_t cap, const uint64_t *dev_offsets, size_t n, void *dev)
{
  if (redo != nullptr)
  {
    memcpy(dst, redo->data(), total);
    return DEGA_OK;
  }
  const int ret = launch_gather(ctx, s, slabs, cap, dev_offsets, n, dev);
  if (ret != DEGA_OK)
    return ret;
  HIP_TRY(ctx, rows_to_host(pl, s, dst, total, dev, total, 1, dst_pinned), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

struct EncChunk : Chunk
{
  uint64_t total = 0; // packed bytes of the chunk
  bool gathered = false, redone = false;
  bool bands = false; // its rows went up in bands, each coded by a launch of its own
  const uint8_t *rows = nullptr; // where the kernels read the chunk's samples: the slot's buffer, or the caller's pinned array in place
  const uint64_t *counts = nullptr; // a counted job: the chunk's counts on the device (the slot's metadata buffer)
  size_t rows_ld = 0;            // ... and its row pitch in samples
  std::vector<uint8_t> redo_bytes; // a chunk that needed worst-case slabs: its packed streams, already on the host
};

struct EncodeRun // state of one device's share of a batch between the two phases of a group call
{
  std::vector<EncChunk> chunks;
};

// the worst-case pass over one chunk, a few channels at a time, synchronous: rare (streams longer than their samples)
static int encode_redo_chunk(dega_hip_ctx *ctx, Pipeline *pl, Slot &sl, const Shape &cj, size_t batch_C, EncChunk &ch, MetaView &hm)
{
  const size_t wc = worst_cap(cj);
  size_t step = std::max<size_t>(64, std::min<size_t>(1024, ((size_t)1 << 30) / std::max<size_t>(wc, 1) / 64 * 64));
  ch.redo_bytes.clear();
  uint64_t running = 0;
  for (size_t j0 = 0; j0 < ch.n; j0 += step)
  {
    const size_t n = std::min(step, ch.n - j0);
    HIP_TRY(ctx, pl->redo_slabs.need(n * wc), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, pl->redo_meta.need(MetaView::bytes(n)), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, pl->redo_hmeta.need(MetaView::bytes(n)), DEGA_ERROR_MEMORY);
    MetaView dm(pl->redo_meta.p, n), rm(pl->redo_hmeta.p, n);
    Shape sj = cj;
    sj.C = n; // columns j0 .. j0+n of the chunk's [T][chunk] image; ld stays the image's pitch
    sj.ld = ch.rows_ld;
    int ret;
    if ((ret = launch_encode(ctx, ch.rows + j0 * sample_bytes(cj), sj, (uint8_t *)pl->redo_slabs.p, wc, dm.bits, dm.err, sl.s, nullptr, 0,
                             ch.counts != nullptr ? ch.counts + j0 : nullptr)) != DEGA_OK)
      return ret;
    if ((ret = sizes_home(ctx, sl.s, dm, n, pl->redo_hmeta.p)) != DEGA_OK)
      return ret;
    HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL);
    const uint64_t tot = rm.offsets[n];
    HIP_TRY(ctx, pl->redo_packed.need((size_t)tot + 16), DEGA_ERROR_MEMORY);
    if (tot > 0)
    {
      if ((ret = launch_gather(ctx, sl.s, pl->redo_slabs.p, wc, dm.offsets, n, pl->redo_packed.p)) != DEGA_OK)
        return ret;
      ch.redo_bytes.resize((size_t)(running + tot));
      HIP_TRY(ctx, hipMemcpyAsync(ch.redo_bytes.data() + running, pl->redo_packed.p, (size_t)tot, hipMemcpyDeviceToHost, sl.s), DEGA_ERROR_LIBRARY_CALL);
      HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL);
    }
    for (size_t i = 0; i < n; i++)
    {
      hm.bits[j0 + i] = rm.bits[i];
      hm.err[j0 + i] = rm.err[i];
      hm.offsets[j0 + i] = running + rm.offsets[i];
    }
    running += tot;
  }
  hm.offsets[ch.n] = running;
  ch.redone = true;
  return DEGA_OK;
}

// How far an encode call's first stages run ahead of the second ones (DEGA_PIPELINE_AHEAD=n: measurement; default 2).
// Not as far as the slots would allow: HIP puts the streams on a few hardware queues, and a queue takes its packets in
// order -- with all eight chunks' first stages enqueued up front, chunk 0's gather and download (enqueued when its sizes
// were on the host, 7 ms into the call) sat behind the launches of a later chunk that were still waiting for their
// bands, and went out at 46 ms; every chunk's streams came home after the last upload (trace of 65 536 x 10 800,
// tools/e2eprof.sh; 66 ms a call). Two chunks ahead keep the link busy (enqueueing a chunk takes 0.15 ms) and a
// download waits for one chunk's launches at most.
static size_t stages_ahead(const ChunkPlan &plan)
{
  const char *e = getenv("DEGA_PIPELINE_AHEAD");
  const long v = e != nullptr ? atol(e) : 2;
  return std::min<size_t>((size_t)std::max(plan.nslots, 1), (size_t)(v < 1 ? 1 : v));
}

static bool decode_uploads_first() // DEGA_PIPELINE_UPLOADS_FIRST=0: upload and kernel enqueued chunk by chunk (measurement)
{
  const char *e = getenv("DEGA_PIPELINE_UPLOADS_FIRST");
  return e == nullptr || atoi(e) != 0;
}
static size_t decode_stages_ahead() // DEGA_PIPELINE_AHEAD_DECODE=n: the same for a decode call (default: as far as the slots allow)
{
  const char *e = getenv("DEGA_PIPELINE_AHEAD_DECODE");
  const long v = e != nullptr ? atol(e) : MAX_SLOTS;
  return (size_t)(v < 1 ? 1 : v);
}

// Pinned samples are read by the encode kernel where they lie (DEGA_PIPELINE_IN_PLACE=0: through the copy engine instead)
static bool read_in_place()
{
  const char *e = getenv("DEGA_PIPELINE_IN_PLACE");
  return e == nullptr || atoi(e) != 0;
}

// Phase A of one device's share: channels [0, j.C) of `samples` (host, row pitch j.ld).  Uploads, codes and sizes every
// chunk; with `deliver` the packed bytes of each chunk also go out at once (base = running total); without, they stay
// on the device (gathered) for encode_deliver().  bits / err / offsets (relative to this share) are final on return.
static int encode_share(dega_hip_ctx *ctx, const Shape &job, const void *samples, EncodeSink &sink, bool deliver, EncodeRun &run)
{
  // Channel-major samples ([C][ld], ld >= T): a chunk's channels go up as they lie -- n rows of T samples, one contiguous
  // copy when ld == T -- into the slot's SLAB buffer, which is free until the chunk's encode launch writes it (everything
  // is on the slot's stream), and dega_transpose_kernel makes the time-major image in the samples' buffer from there.  No
  // staging buffer of its own: the slabs hold max(cap, T * esz) bytes per channel then, and plan_chunks is told so.
  // Whole chunks only: no bands and no in-place read of pinned memory (the kernel's filling waves read rows).
  // A counted job (job.count, host): a chunk's counts go up on the slot's stream ahead of its launches, into the `counts`
  // array of the slot's metadata (free in an encode call), and every launch of the chunk -- whole, in place, per band,
  // redone -- is the counted one.  The transpose of channel-major samples takes them too: the tails of the time-major
  // image are zero bits, whatever lies behind a count in the caller's array.
  const bool cmajor = job.cmajor;
  const uint64_t *const count = job.count;
  Shape j = job;
  j.cmajor = false; // (the chunks' shapes below describe time-major images on the device)
  j.count = nullptr;
  int ret;
  Pipeline *pl;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  if ((ret = pipeline_get(ctx, &pl)) != DEGA_OK)
    return ret;
  const size_t esz = sample_bytes(j);
  const size_t cap = usual_cap(j);
  const size_t slab_bytes = cmajor ? std::max(cap, j.T * esz) : cap; // per channel, what the slot's slab buffer holds
  const size_t dev_per_channel = std::max(j.T * esz + 64, cap) + 16 + slab_bytes + 64;
  const ChunkPlan plan = plan_chunks(j.C, j.T * esz, dev_per_channel, deliver ? 0 : 1);
  if (plan.nslots < 0)
    return fail(ctx, DEGA_ERROR_MEMORY, "the device's share of the batch does not fit its memory", hipSuccess);
  run.chunks.assign(plan.nchunks, EncChunk());
  sink.total = 0;
  sink.full = false;
  const bool samples_pinned = is_pinned(samples), packed_pinned = is_pinned(sink.packed);
  const bool in_place = samples_pinned && read_in_place() && !cmajor;

  TRACE("encode share: C %zu T %zu, %zu chunks of %zu channels, %d slots", j.C, j.T, plan.nchunks, plan.chunk_channels, plan.nslots);
  auto stage1 = [&](size_t k) -> int {
    EncChunk &ch = run.chunks[k];
    TRACE("chunk %zu stage1 begin", k);
    ch.place(plan, j.C, k);
    Slot &sl = pl->slot[ch.slot];
    int r;
    if ((r = slot_stream(ctx, sl)) != DEGA_OK)
      return r;
    HIP_TRY(ctx, sl.a.need(ch.n * std::max(j.T * esz + 64, cap) + 4096), DEGA_ERROR_MEMORY); // the samples, later the packed streams
    HIP_TRY(ctx, sl.b.need(ch.n * slab_bytes + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.meta.need(MetaView::bytes(ch.n)), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.hmeta.need(MetaView::bytes(ch.n)), DEGA_ERROR_MEMORY);
    MetaView dm(sl.meta.p, ch.n);
    if (count != nullptr)
    {
      // through the pinned mirror, which is free too (a slot is reused only after its previous chunk's second stage)
      MetaView hm(sl.hmeta.p, ch.n);
      memcpy(hm.counts, count + ch.c0, ch.n * sizeof(uint64_t));
      HIP_TRY(ctx, hipMemcpyAsync(dm.counts, hm.counts, ch.n * sizeof(uint64_t), hipMemcpyHostToDevice, sl.s), DEGA_ERROR_LIBRARY_CALL);
      ch.counts = dm.counts;
    }
    Shape cj = chunk_shape(j, ch.n);
    const uint8_t *const src = (const uint8_t *)samples + ch.c0 * (cmajor ? j.ld : 1) * esz;
    const size_t band_rows = cmajor ? 0 : band_rows_of(plan, j, ch.n * esz);
    ch.rows = (const uint8_t *)sl.a.p;
    ch.rows_ld = ch.n;
    void *dev_src = nullptr;
    if (in_place && ch.n == j.ld && hipHostGetDevicePointer(&dev_src, const_cast<uint8_t *>(src), 0) != hipSuccess)
    {
      (void)hipGetLastError(); // (pinned, but not mapped into the device's address space: the copy engine takes it)
      dev_src = nullptr;
    }
    if (dev_src != nullptr)
    {
      // The caller's array is pinned and the chunk is all of its columns: the kernel's filling waves fetch their rows
      // from it themselves (LDS-DMA over the link, 256-byte row segments: 8 192 x 86 400 in 65.2 ms against 66.5 ms
      // with bands through the copy engine) -- no image of the samples on the device, one launch.  Only for whole
      // rows: a chunk of the columns of a wider array is read at 32 - 36 GB/s this way (rows 256 KiB apart: a
      // translation per row), where the copy engine runs at the link's rate (56.8 GB/s, tools/pcie_bench).
      ch.rows = (const uint8_t *)dev_src;
      ch.rows_ld = j.ld;
      cj.ld = j.ld;
      if ((r = launch_encode(ctx, ch.rows, cj, (uint8_t *)sl.b.p, cap, dm.bits, dm.err, sl.s, nullptr, 0, ch.counts)) != DEGA_OK)
        return r;
      TRACE("chunk %zu: read in place", k);
    }
    else if (cmajor)
    {
      HIP_TRY(ctx, rows_to_device(pl, sl.s, sl.b.p, src, j.ld * esz, j.T * esz, ch.n, samples_pinned), DEGA_ERROR_LIBRARY_CALL);
      if ((r = launch_transpose(ctx, sl.b.p, ch.n, j.T, j.T, esz, ch.counts, true, sl.a.p, ch.n, sl.s)) != DEGA_OK ||
          (r = launch_encode(ctx, sl.a.p, cj, (uint8_t *)sl.b.p, cap, dm.bits, dm.err, sl.s, nullptr, 0, ch.counts)) != DEGA_OK)
        return r;
      TRACE("chunk %zu: channel-major, transposed on the device", k);
    }
    else if (band_rows == 0)
    {
      HIP_TRY(ctx, rows_to_device(pl, sl.s, sl.a.p, src, j.ld * esz, ch.n * esz, j.T, samples_pinned), DEGA_ERROR_LIBRARY_CALL);
      if ((r = launch_encode(ctx, sl.a.p, cj, (uint8_t *)sl.b.p, cap, dm.bits, dm.err, sl.s, nullptr, 0, ch.counts)) != DEGA_OK)
        return r;
    }
    else
    {
      // Few, long channels: a channel's serial chain takes the same kernel time however few channels there are, so
      // upload and kernel of the (only) chunk must not take turns.  The rows go up in bands on a second stream, and every
      // band is coded by a launch of its own that waits for nothing but its band's event: each launch takes the lanes'
      // state where the one before left it (EncodeArgs::seg_state), the last one ends the streams.
      if (sl.s2 == nullptr)
        HIP_TRY(ctx, hipStreamCreateWithFlags(&sl.s2, hipStreamNonBlocking), DEGA_ERROR_LIBRARY_CALL);
      if (sl.reuse_ev == nullptr)
        HIP_TRY(ctx, hipEventCreateWithFlags(&sl.reuse_ev, hipEventDisableTiming), DEGA_ERROR_LIBRARY_CALL);
      const size_t nbands = (j.T + band_rows - 1) / band_rows;
      while (sl.band_ev.size() < nbands)
      {
        hipEvent_t e;
        HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming), DEGA_ERROR_LIBRARY_CALL);
        sl.band_ev.push_back(e);
      }
      HIP_TRY(ctx, sl.seg_state.need((size_t)ENC_STATE_WORDS * ch.n * sizeof(uint32_t)), DEGA_ERROR_MEMORY);
      // the slot's buffers may still be read by what its previous chunk left on the slot's stream (gather, download):
      // the copies start behind that
      HIP_TRY(ctx, hipEventRecord(sl.reuse_ev, sl.s), DEGA_ERROR_LIBRARY_CALL);
      HIP_TRY(ctx, hipStreamWaitEvent(sl.s2, sl.reuse_ev, 0), DEGA_ERROR_LIBRARY_CALL);
      for (size_t b = 0; b < nbands; b++)
      {
        const size_t t0 = b * band_rows, t1 = std::min(j.T, t0 + band_rows);
        uint8_t *const dev_rows = (uint8_t *)sl.a.p + t0 * ch.n * esz;
        HIP_TRY(ctx, rows_to_device(pl, sl.s2, dev_rows, src + t0 * j.ld * esz, j.ld * esz, ch.n * esz, t1 - t0, samples_pinned), DEGA_ERROR_LIBRARY_CALL);
        HIP_TRY(ctx, hipEventRecord(sl.band_ev[b], sl.s2), DEGA_ERROR_LIBRARY_CALL);
        HIP_TRY(ctx, hipStreamWaitEvent(sl.s, sl.band_ev[b], 0), DEGA_ERROR_LIBRARY_CALL);
        Shape bj = cj;
        bj.T = t1 - t0;
        const uint32_t flags = (b > 0 ? ENC_SEG_CONTINUES : 0u) | (b + 1 < nbands ? ENC_SEG_MORE : 0u);
        if ((r = launch_encode(ctx, dev_rows, bj, (uint8_t *)sl.b.p, cap, dm.bits, dm.err, sl.s, (uint32_t *)sl.seg_state.p, flags, ch.counts, t0, j.T)) != DEGA_OK)
          return r;
      }
      TRACE("chunk %zu: %zu bands of %zu rows, one launch each", k, nbands, band_rows);
      ch.bands = true;
    }
    if ((r = sizes_home(ctx, sl.s, dm, ch.n, sl.hmeta.p)) != DEGA_OK)
      return r;
    TRACE("chunk %zu stage1 enqueued", k);
    return DEGA_OK;
  };

  // sizes of chunk k are on the host: hand out bits / err / offsets, gather its streams, and (deliver) send them home
  auto stage2 = [&](size_t k) -> int {
    EncChunk &ch = run.chunks[k];
    Slot &sl = pl->slot[ch.slot];
    TRACE("chunk %zu stage2 wait", k);
    MetaView hm(sl.hmeta.p, ch.n), dm(sl.meta.p, ch.n);
    HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL);
    TRACE("chunk %zu sizes on the host", k);
    bool too_small = false;
    if (cap < worst_cap(j))
      for (size_t i = 0; i < ch.n && !too_small; i++)
        too_small = hm.err[i] == DEGA_ERROR_MEMORY;
    int r;
    if (too_small && (r = encode_redo_chunk(ctx, pl, sl, chunk_shape(j, ch.n), j.C, ch, hm)) != DEGA_OK)
      return r;
    ch.total = hm.offsets[ch.n];
    uint64_t base;
    const bool fits = chunk_sized(sink, ch.c0, ch.n, hm, base);
    ch.gathered = true;
    // the samples are no longer needed: their buffer takes the packed streams (it holds max(samples, slabs) bytes)
    if (deliver && sink.slabs == nullptr) // packed mode: the streams go home at once
      return !fits ? DEGA_OK
                   : chunk_home(ctx, pl, sl.s, sink.packed + base, packed_pinned, (size_t)ch.total, ch.redone ? &ch.redo_bytes : nullptr, sl.b.p, cap, dm.offsets,
                                ch.n, sl.a.p);
    if (!ch.redone && ch.total > 0 && (r = launch_gather(ctx, sl.s, sl.b.p, cap, dm.offsets, ch.n, sl.a.p)) != DEGA_OK)
      return r;
    if (!deliver) // the streams stay where they are for encode_deliver()
      return DEGA_OK;
    // slab mode: through the pinned stage, then channel by channel to its slab
    const uint8_t *srcb = nullptr;
    if (ch.redone)
      srcb = ch.redo_bytes.data();
    else if (ch.total > 0)
    {
      HIP_TRY(ctx, sl.stage.need((size_t)ch.total), DEGA_ERROR_MEMORY);
      HIP_TRY(ctx, hipMemcpyAsync(sl.stage.p, sl.a.p, (size_t)ch.total, hipMemcpyDeviceToHost, sl.s), DEGA_ERROR_LIBRARY_CALL);
      HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL);
      srcb = (const uint8_t *)sl.stage.p;
    }
    for (size_t i = 0; i < ch.n; i++)
    {
      const size_t nb = (size_t)(hm.offsets[i + 1] - hm.offsets[i]);
      if (nb > sink.slab_cap && sink.err[ch.c0 + i] == DEGA_OK)
        sink.err[ch.c0 + i] = DEGA_ERROR_MEMORY; // the stream does not fit the caller's slab: its head is there, its length is reported
      if (nb > 0)
        memcpy(sink.slabs + (ch.c0 + i) * sink.slab_cap, srcb + hm.offsets[i], std::min(nb, sink.slab_cap));
    }
    return DEGA_OK;
  };

  if ((ret = run_chunks(plan.nchunks, stages_ahead(plan), stage1, stage2)) != DEGA_OK)
    return ret;
  TRACE("all chunks enqueued");
  if ((ret = finish_slots(ctx, pl, plan.nslots)) != DEGA_OK)
    return ret;
  TRACE("encode share done");
  if (sink.offsets != nullptr)
    sink.offsets[j.C] = sink.total;
  if (deliver && sink.slabs == nullptr && sink.full)
    return fail(ctx, DEGA_ERROR_MEMORY, "packed buffer too small: offsets[C] holds the size needed", hipSuccess);
  return DEGA_OK;
}

// Phase B: the packed streams of this device's chunks, still on the device, to packed + base (host)
static int encode_deliver(dega_hip_ctx *ctx, EncodeRun &run, uint8_t *packed, uint64_t base)
{
  Pipeline *pl = ctx->pipe;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  const bool pinned = is_pinned(packed);
  for (EncChunk &ch : run.chunks)
  {
    Slot &sl = pl->slot[ch.slot];
    if (ch.total > 0)
    {
      if (ch.redone)
        memcpy(packed + base, ch.redo_bytes.data(), (size_t)ch.total);
      else
        HIP_TRY(ctx, rows_to_host(pl, sl.s, packed + base, (size_t)ch.total, sl.a.p, (size_t)ch.total, 1, pinned), DEGA_ERROR_LIBRARY_CALL);
    }
    base += ch.total;
  }
  HIP_TRY(ctx, pl->stager.drain(), DEGA_ERROR_LIBRARY_CALL);
  for (EncChunk &ch : run.chunks)
    HIP_TRY(ctx, hipStreamSynchronize(pl->slot[ch.slot].s), DEGA_ERROR_LIBRARY_CALL);
  return DEGA_OK;
}

// ---- encode, several granularities from one upload (dega_hip_encode_levels_job_host) -------------------------------------------

static size_t meta_stride(size_t n) // the K MetaViews of a slot lie one behind the other, each 8-byte aligned
{
  return (MetaView::bytes(n) + 7) & ~(size_t)7;
}

// One device's share of a batch coded at K granularities (K = 1: the single-level aggregated forms).  A function of its
// own beside encode_share, which codes the rows as they are, with its habits: chunks of channels on the slots' streams,
// nothing allocated per call beyond growing the slot's buffers, only stream bytes come back, first stages two chunks
// ahead, a level of a chunk whose stream outgrows the usual slab redone with worst-case slabs.  Whole-chunk launches
// behind a copy-engine upload: the link carries the fine rows, N times what a level's coder sees, and is the bound; no
// bands, no in-place read of pinned rows.  A chunk's fine rows cross the link ONCE; a slot holds them (c), the sums
// of all summed levels (a), K slab regions (b) and K sets of the small arrays (meta).  When the K encode launches of a
// chunk are done its fine rows are no longer needed, and their buffer takes the packed streams, level behind level.
// j: C, ld, factor, adaptive, valuesize of the job; j.T the FINE length.  Always delivers (no resident phase).
// `sized`: set once every chunk has been coded and sized, i.e. bits / err / offsets / total of every level are complete;
// a DEGA_ERROR_MEMORY with `sized` false is a failed allocation, one with `sized` true a packed buffer that is too small.
static int encode_levels_share(dega_hip_ctx *ctx, const Shape &job, const size_t *num_values, size_t K, const void *samples, PackedOut *sink, bool &sized)
{
  // channel-major samples: as in encode_share, through the slot's slab buffer (free until the first encode launch of the
  // chunk), which then holds max(the levels' slabs, T * esz) bytes per channel
  const bool cmajor = job.cmajor;
  Shape j = job;
  j.cmajor = false;
  sized = false;
  int ret;
  Pipeline *pl;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  if ((ret = pipeline_get(ctx, &pl)) != DEGA_OK)
    return ret;
  const size_t esz = sizeof(float);
  Shape lj[AGG_MAX_LEVELS]; // level k as the coder sees it
  size_t cap[AGG_MAX_LEVELS], sum_rows = 0, cap_sum = 0;
  for (size_t k = 0; k < K; k++)
  {
    lj[k] = j;
    lj[k].T = dega_hip_aggregate_rows(j.T, num_values[k]);
    cap[k] = usual_cap(lj[k]);
    cap_sum += cap[k];
    if (num_values[k] != 1) // N = 1 is coded straight from the fine rows
      sum_rows += lj[k].T;
    sink[k].total = 0;
    sink[k].full = false;
  }
  const size_t fine_bytes = std::max(j.T * esz + 64, cap_sum); // per channel: the fine rows, later every level's packed streams
  const size_t slab_bytes = cmajor ? std::max(cap_sum, j.T * esz) : cap_sum;
  const size_t dev_per_channel = fine_bytes + 16 + sum_rows * esz + 16 * K + slab_bytes + 64 + K * 32;
  const ChunkPlan plan = plan_chunks(j.C, j.T * esz, dev_per_channel, 0);
  struct LevelChunk : Chunk
  {
    EncChunk lv[AGG_MAX_LEVELS]; // per level: rows / rows_ld / total / redone / redo_bytes
  };
  std::vector<LevelChunk> chunks(plan.nchunks);
  const bool samples_pinned = is_pinned(samples);
  bool packed_pinned[AGG_MAX_LEVELS];
  for (size_t k = 0; k < K; k++)
    packed_pinned[k] = is_pinned(sink[k].packed);
  TRACE("encode levels share: C %zu T %zu, %zu levels, %zu chunks of %zu channels, %d slots", j.C, j.T, K, plan.nchunks, plan.chunk_channels, plan.nslots);

  auto stage1 = [&](size_t q) -> int {
    LevelChunk &ch = chunks[q];
    ch.place(plan, j.C, q);
    Slot &sl = pl->slot[ch.slot];
    int r;
    if ((r = slot_stream(ctx, sl)) != DEGA_OK)
      return r;
    const size_t n = ch.n;
    HIP_TRY(ctx, sl.c.need(n * fine_bytes + 4096), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.a.need((sum_rows * n + 4 * K) * esz + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.b.need(n * slab_bytes + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.meta.need(K * meta_stride(n)), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.hmeta.need(K * meta_stride(n)), DEGA_ERROR_MEMORY);
    const uint8_t *const src = (const uint8_t *)samples + ch.c0 * (cmajor ? j.ld : 1) * esz;
    if (cmajor)
    {
      HIP_TRY(ctx, rows_to_device(pl, sl.s, sl.b.p, src, j.ld * esz, j.T * esz, n, samples_pinned), DEGA_ERROR_LIBRARY_CALL);
      if ((r = launch_transpose(ctx, sl.b.p, n, j.T, j.T, esz, nullptr, true, sl.c.p, n, sl.s)) != DEGA_OK)
        return r;
    }
    else
      HIP_TRY(ctx, rows_to_device(pl, sl.s, sl.c.p, src, j.ld * esz, n * esz, j.T, samples_pinned), DEGA_ERROR_LIBRARY_CALL);
    // the sums of the summed levels: the plan's passes over the chunk's image (pitch n), every level 16-byte aligned
    LevelSums sums(num_values, K, j.T, n, false);
    sums.place((float *)sl.a.p);
    for (size_t k = 0, m = 0; k < K; k++)
    {
      EncChunk &e = ch.lv[k];
      e.n = n;
      e.rows_ld = n;
      e.redone = false;
      e.total = 0;
      e.rows = num_values[k] == 1 ? (const uint8_t *)sl.c.p : (const uint8_t *)sums.a[m++];
    }
    if ((r = check_levels_dev(ctx, (const float *)sl.c.p, n, j.T, n, sums.N, sums.n, sums.a, sums.ldo)) != DEGA_OK ||
        (r = launch_aggregate_levels(ctx, (const float *)sl.c.p, n, j.T, n, nullptr, sums.N, sums.n, sums.a, sums.ldo, nullptr, nullptr, sl.s)) != DEGA_OK)
      return r;
    size_t slab_off = 0;
    for (size_t k = 0; k < K; k++)
    {
      MetaView dm((uint8_t *)sl.meta.p + k * meta_stride(n), n);
      if ((r = launch_encode(ctx, ch.lv[k].rows, chunk_shape(lj[k], n), (uint8_t *)sl.b.p + slab_off, cap[k], dm.bits, dm.err, sl.s)) != DEGA_OK ||
          (r = sizes_home(ctx, sl.s, dm, n, nullptr)) != DEGA_OK) // (the K sets go home in one copy, below)
        return r;
      slab_off += n * cap[k];
    }
    HIP_TRY(ctx, hipMemcpyAsync(sl.hmeta.p, sl.meta.p, K * meta_stride(n), hipMemcpyDeviceToHost, sl.s), DEGA_ERROR_LIBRARY_CALL);
    TRACE("levels chunk %zu stage1 enqueued", q);
    return DEGA_OK;
  };

  auto stage2 = [&](size_t q) -> int {
    LevelChunk &ch = chunks[q];
    Slot &sl = pl->slot[ch.slot];
    const size_t n = ch.n;
    HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL);
    int r;
    // first every redo (it reads the level's rows, for N = 1 the fine rows), then the gathers (which overwrite the fine rows)
    for (size_t k = 0; k < K; k++)
    {
      MetaView hm((uint8_t *)sl.hmeta.p + k * meta_stride(n), n);
      bool too_small = false;
      if (cap[k] < worst_cap(lj[k]))
        for (size_t i = 0; i < n && !too_small; i++)
          too_small = hm.err[i] == DEGA_ERROR_MEMORY;
      if (too_small && (r = encode_redo_chunk(ctx, pl, sl, chunk_shape(lj[k], n), j.C, ch.lv[k], hm)) != DEGA_OK)
        return r;
    }
    size_t slab_off = 0, packed_off = 0;
    for (size_t k = 0; k < K; k++)
    {
      MetaView hm((uint8_t *)sl.hmeta.p + k * meta_stride(n), n), dm((uint8_t *)sl.meta.p + k * meta_stride(n), n);
      EncChunk &e = ch.lv[k];
      e.total = hm.offsets[n];
      const size_t slabs_at = slab_off;
      slab_off += n * cap[k];
      uint64_t base;
      if (!chunk_sized(sink[k], ch.c0, n, hm, base))
        continue;
      const size_t packed_at = packed_off; // (not redone: at most n * cap[k] bytes, and the buffer holds n * the sum of the caps)
      if (!e.redone)
        packed_off += (size_t)((e.total + 15) & ~(uint64_t)15);
      if ((r = chunk_home(ctx, pl, sl.s, sink[k].packed + base, packed_pinned[k], (size_t)e.total, e.redone ? &e.redo_bytes : nullptr,
                          (const uint8_t *)sl.b.p + slabs_at, cap[k], dm.offsets, n, (uint8_t *)sl.c.p + packed_at)) != DEGA_OK)
        return r;
    }
    return DEGA_OK;
  };

  if ((ret = run_chunks(plan.nchunks, stages_ahead(plan), stage1, stage2)) != DEGA_OK || (ret = finish_slots(ctx, pl, plan.nslots)) != DEGA_OK)
    return ret;
  bool any_full = false;
  sized = true;
  for (size_t k = 0; k < K; k++)
  {
    sink[k].offsets[j.C] = sink[k].total;
    any_full = any_full || sink[k].full;
  }
  if (any_full)
    return fail(ctx, DEGA_ERROR_MEMORY, "a level's packed buffer is too small: its offsets[C] holds the size needed", hipSuccess);
  return DEGA_OK;
}

// ---- decode ------------------------------------------------------------------------------------------------------------

// The decode head, every codec's: the streams of a chunk's n channels -- offsets[0 .. n] into the caller's packed buffer,
// bits[0 .. n) -- go up on stream `us` and are spread into slabs in the slot's buffer b, one per channel and as long as
// the chunk's longest stream needs: `cap`, which is returned.  The bit lengths and the offsets, rebased to the chunk, go
// through the slot's pinned mirror (the caller has waited for the slot's stream: nothing of the slot's is still in use);
// the packed bytes through its buffer a, which holds at least a_floor bytes.
static int chunk_in(dega_hip_ctx *ctx, Pipeline *pl, Slot &sl, hipStream_t us, const uint8_t *packed, const uint64_t *offsets, const uint64_t *bits, size_t n,
                    bool packed_pinned, size_t a_floor, size_t &cap)
{
  const uint64_t o0 = offsets[0], nbytes = offsets[n] - o0;
  uint64_t longest = 0;
  for (size_t i = 0; i < n; i++)
    longest = std::max<uint64_t>(longest, offsets[i + 1] - offsets[i]);
  cap = ((size_t)longest + 16 + 3) & ~(size_t)3; // room for the decoder's word look-ahead
  HIP_TRY(ctx, sl.a.need(std::max((size_t)nbytes, a_floor) + 64), DEGA_ERROR_MEMORY);
  HIP_TRY(ctx, sl.b.need(n * cap + 64), DEGA_ERROR_MEMORY);
  HIP_TRY(ctx, sl.meta.need(MetaView::bytes(n)), DEGA_ERROR_MEMORY);
  HIP_TRY(ctx, sl.hmeta.need(MetaView::bytes(n)), DEGA_ERROR_MEMORY);
  MetaView hm(sl.hmeta.p, n), dm(sl.meta.p, n);
  for (size_t i = 0; i < n; i++)
  {
    hm.bits[i] = bits[i];
    hm.offsets[i] = offsets[i] - o0;
  }
  hm.offsets[n] = nbytes;
  HIP_TRY(ctx, hipMemcpyAsync(sl.meta.p, sl.hmeta.p, (2 * n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, us), DEGA_ERROR_LIBRARY_CALL);
  HIP_TRY(ctx, rows_to_device(pl, us, sl.a.p, packed + o0, (size_t)nbytes, (size_t)nbytes, 1, packed_pinned), DEGA_ERROR_LIBRARY_CALL);
  return launch_scatter(ctx, us, sl.b.p, cap, dm.offsets, n, sl.a.p);
}

static int decode_share(dega_hip_ctx *ctx, const Shape &job, const uint8_t *packed, const uint64_t *offsets, const uint64_t *bits, void *samples,
                        uint64_t *out_count, int32_t *err)
{
  // Channel-major samples ([C][ld], ld >= T): dega_transpose_kernel runs behind the chunk's decode kernel, from the samples'
  // buffer into the buffer of the chunk's packed streams -- free once they have been spread into slabs, which the slot's
  // stream has waited for -- which holds max(the streams, n * T samples) then (plan_chunks is told so).  With out_count the
  // kernel gets the chunk's device counts, so the tail of every series goes home as zeros; the download is n rows of T
  // samples at the caller's pitch, whose padding is not touched.  Whole chunks only: no bands.
  const bool cmajor = job.cmajor;
  Shape j = job;
  j.cmajor = false;
  int ret;
  Pipeline *pl;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  if ((ret = pipeline_get(ctx, &pl)) != DEGA_OK)
    return ret;
  const size_t osz = sample_bytes(j);
  // the longest stream sets the slab size of a chunk; the average one the device bytes per channel
  const uint64_t span = j.C > 0 ? offsets[j.C] - offsets[0] : 0;
  uint64_t longest_all = 0;
  for (size_t c = 0; c < j.C; c++)
    longest_all = std::max<uint64_t>(longest_all, offsets[c + 1] - offsets[c]);
  const size_t mean_stream = (size_t)(span / std::max<size_t>(j.C, 1));
  const size_t dev_per_channel = j.T * osz + (cmajor ? std::max(mean_stream, j.T * osz) : mean_stream) + (size_t)longest_all + 64;
  // At most four chunks: a decode kernel takes its channels' serial time however few they are, the hardware queues run
  // few of them side by side, and the rows go home in bands beside the running kernel anyway (65 536 x 10 800 from
  // pinned memory: 8 chunks 83 ms, 4: 63 ms, 2: 66.5 ms, 1: 66 ms).
  const ChunkPlan plan = plan_chunks(j.C, j.T * osz, dev_per_channel, 0, 4);
  struct DecChunk : Chunk
  {
    size_t band_rows; // 0: the samples come home after the kernel; else in bands of rows beside it
    size_t cap;       // slab bytes per channel
  };
  std::vector<DecChunk> chunks(plan.nchunks);
  const bool samples_pinned = is_pinned(samples), packed_pinned = is_pinned(packed);
  const bool all_uploads_first = (size_t)plan.nslots >= plan.nchunks && decode_uploads_first();
  TRACE("decode share: C %zu T %zu, %zu chunks of %zu channels, %d slots, %s", j.C, j.T, plan.nchunks, plan.chunk_channels, plan.nslots,
        all_uploads_first ? "all uploads first" : "chunk by chunk");

  // (the slot's stream is idle when stage1a runs -- it synchronises it -- so nothing of the slot's is still in use)
  const bool one_upload_stream = packed_pinned && decode_uploads_first();
  // first stage, part a: the chunk's packed streams go up and are spread into slabs
  auto stage1a = [&](size_t k) -> int {
    DecChunk &ch = chunks[k];
    ch.place(plan, j.C, k);
    Slot &sl = pl->slot[ch.slot];
    int r;
    if ((r = slot_stream(ctx, sl)) != DEGA_OK)
      return r;
    HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL); // the pinned mirror is about to be rewritten
    HIP_TRY(ctx, sl.c.need(ch.n * j.T * osz + 64), DEGA_ERROR_MEMORY);
    // The uploads of all chunks share ONE stream: side by side on their own streams they share the link, every one of
    // them takes as long as all together, and the first kernel starts when the last upload is done (two chunks: 74 ms a
    // call where one chunk takes 66).  The chunk's own stream goes on behind the upload's event.
    hipStream_t us = sl.s;
    if (one_upload_stream)
    {
      if (pl->up == nullptr)
        HIP_TRY(ctx, hipStreamCreateWithFlags(&pl->up, hipStreamNonBlocking), DEGA_ERROR_LIBRARY_CALL);
      if (sl.reuse_ev == nullptr)
        HIP_TRY(ctx, hipEventCreateWithFlags(&sl.reuse_ev, hipEventDisableTiming), DEGA_ERROR_LIBRARY_CALL);
      us = pl->up;
    }
    if ((r = chunk_in(ctx, pl, sl, us, packed, offsets + ch.c0, bits + ch.c0, ch.n, packed_pinned, cmajor ? ch.n * j.T * osz : 0, ch.cap)) != DEGA_OK)
      return r;
    if (us != sl.s)
    {
      HIP_TRY(ctx, hipEventRecord(sl.reuse_ev, us), DEGA_ERROR_LIBRARY_CALL);
      HIP_TRY(ctx, hipStreamWaitEvent(sl.s, sl.reuse_ev, 0), DEGA_ERROR_LIBRARY_CALL);
    }
    return DEGA_OK;
  };
  // first stage, part b: the decode kernel
  auto stage1b = [&](size_t k) -> int {
    DecChunk &ch = chunks[k];
    Slot &sl = pl->slot[ch.slot];
    const size_t cap = ch.cap;
    MetaView hm(sl.hmeta.p, ch.n), dm(sl.meta.p, ch.n);
    int r;
    const Shape cj = chunk_shape(j, ch.n);
    // few, long channels (see encode_share): the rows go home in bands while the kernel is still decoding; every wave of 64
    // channels reports the rows it has stored in a word of pinned host memory
    ch.band_rows = out_count == nullptr && !cmajor ? band_rows_of(plan, j, ch.n * osz) : 0;
    uint32_t *reports = nullptr;
    if (ch.band_rows != 0)
    {
      const size_t waves = (ch.n + 63) / 64;
      HIP_TRY(ctx, sl.progress_values.need(sizeof(uint32_t) * waves), DEGA_ERROR_MEMORY);
      reports = (uint32_t *)sl.progress_values.p;
      memset(reports, 0, sizeof(uint32_t) * waves);
      if (sl.s2 == nullptr)
        HIP_TRY(ctx, hipStreamCreateWithFlags(&sl.s2, hipStreamNonBlocking), DEGA_ERROR_LIBRARY_CALL);
      TRACE("decode chunk %zu: %zu bands of %zu rows, sent home beside the kernel", k, (j.T + ch.band_rows - 1) / ch.band_rows, ch.band_rows);
    }
    if ((r = launch_decode(ctx, (const uint8_t *)sl.b.p, cap, dm.bits, cj, j.C, sl.c.p, out_count != nullptr ? dm.counts : nullptr, dm.err, sl.s, reports,
                           (uint32_t)ch.band_rows)) != DEGA_OK)
      return r;
    if (cmajor && (r = launch_transpose(ctx, sl.c.p, j.T, ch.n, ch.n, osz, out_count != nullptr ? dm.counts : nullptr, false, sl.a.p, j.T, sl.s)) != DEGA_OK)
      return r;
    // counts and err come back right behind the kernel
    HIP_TRY(ctx, hipMemcpyAsync(hm.counts, dm.counts, ch.n * sizeof(uint64_t) + ch.n * sizeof(int32_t), hipMemcpyDeviceToHost, sl.s), DEGA_ERROR_LIBRARY_CALL);
    return DEGA_OK;
  };
  // the samples of chunk k come home (through the staging ring unless the caller's array is pinned)
  auto stage2 = [&](size_t k) -> int {
    DecChunk &ch = chunks[k];
    Slot &sl = pl->slot[ch.slot];
    if (cmajor)
      HIP_TRY(ctx, rows_to_host(pl, sl.s, (uint8_t *)samples + ch.c0 * j.ld * osz, j.ld * osz, sl.a.p, j.T * osz, ch.n, samples_pinned), DEGA_ERROR_LIBRARY_CALL);
    else if (ch.band_rows == 0)
      HIP_TRY(ctx, rows_to_host(pl, sl.s, (uint8_t *)samples + ch.c0 * osz, j.ld * osz, sl.c.p, ch.n * osz, j.T, samples_pinned), DEGA_ERROR_LIBRARY_CALL);
    else
    {
      const volatile uint32_t *const reports = (const volatile uint32_t *)sl.progress_values.p;
      const size_t waves = (ch.n + 63) / 64;
      bool kernel_over = false;
      for (size_t t0 = 0; t0 < j.T; t0 += ch.band_rows)
      {
        const size_t t1 = std::min(j.T, t0 + ch.band_rows);
        for (;;) // until every wave has stored the band's rows (or the kernel is over: then they are all there)
        {
          uint32_t least = 0xFFFFFFFFu;
          for (size_t w = 0; w < waves; w++)
          {
            const uint32_t v = reports[w];
            least = v < least ? v : least;
          }
          if (least >= t1 || kernel_over)
            break;
          if (hipStreamQuery(sl.s) != hipErrorNotReady)
            kernel_over = true;
          else
            sched_yield();
        }
        HIP_TRY(ctx, rows_to_host(pl, sl.s2, (uint8_t *)samples + (t0 * j.ld + ch.c0) * osz, j.ld * osz, (const uint8_t *)sl.c.p + t0 * ch.n * osz, ch.n * osz,
                                  t1 - t0, samples_pinned),
                DEGA_ERROR_LIBRARY_CALL);
      }
      HIP_TRY(ctx, hipStreamSynchronize(sl.s2), DEGA_ERROR_LIBRARY_CALL);
    }
    HIP_TRY(ctx, pl->stager.drain(), DEGA_ERROR_LIBRARY_CALL); // the slot's buffers are free for its next chunk only after this
    HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL);
    MetaView hm(sl.hmeta.p, ch.n);
    for (size_t i = 0; i < ch.n; i++)
      err[ch.c0 + i] = hm.err[i];
    if (out_count != nullptr)
      for (size_t i = 0; i < ch.n; i++)
        out_count[ch.c0 + i] = hm.counts[i];
    return DEGA_OK;
  };
  if (all_uploads_first)
  {
    // Every chunk has a slot of its own: all the uploads are enqueued before the first decode kernel.  HIP puts the
    // streams on a few hardware queues that take their packets in order; with upload and kernel enqueued chunk by chunk,
    // the upload of chunk 4 sat behind the 8 ms kernel of chunk 0 on their queue, chunks 6 and 7 behind that of chunk 4,
    // and the link stood idle for 20 ms of an 80 ms call (trace of 65 536 x 10 800, gpurun_out/e2eprof_dec).
    for (size_t k = 0; k < plan.nchunks; k++)
      if ((ret = stage1a(k)) != DEGA_OK)
        return ret;
    for (size_t k = 0; k < plan.nchunks; k++)
      if ((ret = stage1b(k)) != DEGA_OK)
        return ret;
    for (size_t k = 0; k < plan.nchunks; k++)
      if ((ret = stage2(k)) != DEGA_OK)
        return ret;
    return DEGA_OK;
  }
  auto stage1 = [&](size_t k) -> int {
    const int r = stage1a(k);
    return r != DEGA_OK ? r : stage1b(k);
  };
  return run_chunks(plan.nchunks, std::min<size_t>((size_t)plan.nslots, decode_stages_ahead()), stage1, stage2);
}

// What is wrong with the packed streams a decode call was given (nullptr: nothing): offsets[C + 1] and bits[C] as the
// encode calls write them, no stream longer than the codec's decoder takes (`longest`; too_long: what to say of one that is)
static const char *packed_input_fault(size_t C, const uint64_t *offsets, const uint64_t *bits, uint64_t longest, const char *too_long)
{
  static const char *const order = "offsets must grow and hold ceil(bits / 8) bytes per channel";
  for (size_t c = 0; c < C; c++)
  {
    // (bits + 7) / 8 would wrap for lengths near 2^64: compare without the rounding add
    if (offsets[c + 1] < offsets[c] || bits[c] / 8 > offsets[c + 1] - offsets[c] || (bits[c] / 8 == offsets[c + 1] - offsets[c] && (bits[c] & 7) != 0))
      return order;
    if (offsets[c + 1] - offsets[c] > longest)
      return too_long != nullptr ? too_long : order;
  }
  return nullptr;
}

static int check_packed_input(dega_hip_ctx *ctx, const Shape &j, const uint8_t *packed, const uint64_t *offsets, const uint64_t *bits)
{
  if (offsets == nullptr || bits == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (j.C > 0 && packed == nullptr && offsets[j.C] != offsets[0])
    return DEGA_ERROR_INVALID_VALUE;
  const char *const what = packed_input_fault(j.C, offsets, bits, ((uint64_t)1 << 29) - 64, "a stream of more than 512 MiB");
  return what == nullptr ? DEGA_OK : fail(ctx, DEGA_ERROR_INVALID_VALUE, what, hipSuccess);
}

// ---- the group: one pipeline per device, a host thread each ------------------------------------------------------------------

struct dega_hip_group
{
  std::vector<dega_hip_ctx *> ctx;
  char last_error[320];
};

extern "C" int dega_hip_group_create(const int *devices, int n, dega_hip_group **out)
{
  if (out == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  *out = nullptr;
  std::vector<int> devs;
  if (devices != nullptr && n > 0)
    devs.assign(devices, devices + n);
  else
  {
    // every visible device, or the list in DEGA_DEVICES ("0,2,3"); DEGA_DEVICE (one index) is honoured too
    const char *list = getenv("DEGA_DEVICES");
    const char *one = getenv("DEGA_DEVICE");
    if (list != nullptr && *list != '\0')
    {
      const char *p = list;
      while (*p != '\0')
      {
        char *end;
        const long v = strtol(p, &end, 10);
        if (end == p)
          break;
        devs.push_back((int)v);
        p = *end == ',' ? end + 1 : end;
      }
    }
    else if (one != nullptr && *one != '\0')
      devs.push_back(atoi(one));
    else
      for (int d = 0; d < dega_hip_device_count(); d++)
        devs.push_back(d);
  }
  if (devs.empty())
    return DEGA_ERROR_LIBRARY_INIT; // no GPU: no CPU fallback
  dega_hip_group *g = new dega_hip_group();
  g->last_error[0] = '\0';
  for (int d : devs)
  {
    dega_hip_ctx *c = nullptr;
    const int ret = dega_hip_create(d, &c);
    if (ret != DEGA_OK)
    {
      for (dega_hip_ctx *x : g->ctx)
        dega_hip_destroy(x);
      delete g;
      return ret;
    }
    g->ctx.push_back(c);
  }
  *out = g;
  return DEGA_OK;
}

extern "C" void dega_hip_group_destroy(dega_hip_group *g)
{
  if (g == nullptr)
    return;
  for (dega_hip_ctx *c : g->ctx)
    dega_hip_destroy(c);
  delete g;
}

extern "C" int dega_hip_group_size(const dega_hip_group *g)
{
  return g == nullptr ? 0 : (int)g->ctx.size();
}

extern "C" dega_hip_ctx *dega_hip_group_context(dega_hip_group *g, int i)
{
  return g == nullptr || i < 0 || i >= (int)g->ctx.size() ? nullptr : g->ctx[(size_t)i];
}

extern "C" const char *dega_hip_group_last_error(const dega_hip_group *g)
{
  return g == nullptr ? "no group" : g->last_error;
}

static Shape shape_from_job(const dega_hip_job *job)
{
  // (any other bit above the sample types stays in `samples` and is refused with it)
  Shape j = shape_of(job->C, job->T, job->ld, job->adaptive, job->valuesize, job->samples & ~DEGA_SAMPLES_CHANNEL_MAJOR, job->factor);
  j.cmajor = (job->samples & DEGA_SAMPLES_CHANNEL_MAJOR) != 0;
  return j;
}

// how many of a group's members a call of C channels uses: those that get a workgroup's `granule` of channels
static size_t members_for(const dega_hip_group *grp, size_t C, size_t granule)
{
  return std::max<size_t>(1, std::min<size_t>(grp->ctx.size(), (C + granule - 1) / granule));
}

// contiguous channel ranges [c_g, c_g+1) for G members, cut at whole workgroups of `granule` channels (the coder's 512:
// only where that leaves every member two of them -- a smaller batch is shared evenly; LZMH's 256: always)
static std::vector<size_t> split_channels(size_t C, size_t G, size_t granule = 512)
{
  std::vector<size_t> cut(G + 1, 0);
  for (size_t g = 1; g < G; g++)
  {
    size_t c = C / G * g + std::min(C % G, g);
    if (granule < 512 || C >= G * 2 * granule)
      c = c / granule * granule;
    cut[g] = c;
  }
  cut[G] = C;
  return cut;
}

extern "C" int dega_hip_split_channels(size_t C, int G, size_t *cuts)
{
  if (G < 1 || cuts == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  const std::vector<size_t> c = split_channels(C, (size_t)G);
  for (size_t g = 0; g <= (size_t)G; g++)
    cuts[g] = c[g];
  return DEGA_OK;
}

static int group_fail(dega_hip_group *g, int code, dega_hip_ctx *c, size_t dev_index)
{
  snprintf(g->last_error, sizeof(g->last_error), "device %d (member %zu): %s", c->device, dev_index, c->last_error);
  return code;
}

// work(g) for every member g < G, each on a host thread of its own (in the caller's when there is one member); the
// first member that failed is the call's failure
template <class Work>
static int on_members(dega_hip_group *grp, size_t G, Work work)
{
  std::vector<int> rets(G, DEGA_OK);
  if (G == 1)
    rets[0] = work((size_t)0);
  else
  {
    std::vector<std::thread> th;
    for (size_t g = 0; g < G; g++)
      th.emplace_back([&, g] { rets[g] = work(g); });
    for (std::thread &t : th)
      t.join();
  }
  for (size_t g = 0; g < G; g++)
    if (rets[g] != DEGA_OK)
      return group_fail(grp, rets[g], grp->ctx[g], g);
  return DEGA_OK;
}

// the group of the single-context (`*_host`) forms: the caller's context alone
static dega_hip_group group_of_one(dega_hip_ctx *ctx)
{
  dega_hip_group one;
  one.ctx.push_back(ctx);
  one.last_error[0] = '\0';
  return one;
}

// the packed form of a call's outputs, from the ABI's arguments (offsets[0] = 0 is written here, once)
static EncodeSink packed_sink(uint8_t *packed, size_t packed_cap, uint64_t *offsets, uint64_t *out_bits, int32_t *err)
{
  EncodeSink sink;
  static_cast<PackedOut &>(sink) = packed_out(packed, packed_cap, offsets, out_bits, err);
  if (offsets != nullptr)
    offsets[0] = 0;
  return sink;
}

// Host-side concatenate for a group whose members have each delivered their share into a buffer of their own: member g's
// streams (member(g): offsets relative to its share, total, full, and its buffer as `packed`) go behind those of the members
// in front of it.  Writes the call's offsets and total; its bytes unless it, or a member, is full.
template <class Member>
static void concat_members(const std::vector<size_t> &cut, Member member, PackedOut &out)
{
  const size_t G = cut.size() - 1;
  out.total = 0;
  out.full = false;
  for (size_t g = 0; g < G; g++)
  {
    const PackedOut &m = member(g);
    for (size_t i = 0; i < cut[g + 1] - cut[g]; i++)
      out.offsets[cut[g] + i] = out.total + m.offsets[i];
    out.total += m.total;
    out.full = out.full || m.full;
  }
  out.offsets[cut[G]] = out.total;
  out.full = out.full || out.total > out.packed_cap;
  for (size_t g = 0; g < G && !out.full; g++)
    if (member(g).total > 0)
      memcpy(out.packed + out.offsets[cut[g]], member(g).packed, (size_t)member(g).total);
}

static int encode_on_group(dega_hip_group *grp, const Shape &j, const void *samples, EncodeSink sink)
{
  if (grp == nullptr || grp->ctx.empty())
    return DEGA_ERROR_LIBRARY_INIT;
  int ret;
  if ((ret = check_job_shape(grp->ctx[0], j, 0)) != DEGA_OK)
    return group_fail(grp, ret, grp->ctx[0], 0);
  if (sink.bits == nullptr || sink.err == nullptr || (sink.slabs == nullptr && (sink.offsets == nullptr || (sink.packed == nullptr && sink.packed_cap != 0))) ||
      (samples == nullptr && j.C * j.T != 0))
    return DEGA_ERROR_INVALID_VALUE;
  const size_t esz = sample_bytes(j);
  // devices that get no channels are left out; a single device delivers as it goes (copies overlap the kernels)
  const size_t G = members_for(grp, j.C, 512);
  if (G == 1)
  {
    EncodeRun run;
    ret = encode_share(grp->ctx[0], j, samples, sink, true, run);
    return ret == DEGA_OK ? DEGA_OK : group_fail(grp, ret, grp->ctx[0], 0);
  }
  // Several members: packed mode (slab mode is the single-context forms', which come as a group of one).
  // Rounds: what the devices can hold at once (samples + slabs resident until the sizes in front are known) -- by the
  // member with the least free memory, and with the bytes per channel that encode_share reserves
  size_t free_b = ~(size_t)0;
  for (size_t g = 0; g < G; g++)
  {
    size_t f = 0, t = 0;
    if (hipSetDevice(grp->ctx[g]->device) != hipSuccess || hipMemGetInfo(&f, &t) != hipSuccess)
    {
      (void)hipGetLastError();
      f = (size_t)64 << 30;
    }
    free_b = std::min(free_b, f);
  }
  const size_t per_channel = std::max(j.T * esz + 64, usual_cap(j)) + 16 + (j.cmajor ? std::max(usual_cap(j), j.T * esz) : usual_cap(j)) + 64 + 256;
  size_t round_channels = std::max<size_t>(G * 512, std::min<size_t>(j.C, free_b / 10 * 6 / per_channel * G / 512 * 512));
  for (size_t r0 = 0; r0 < j.C;)
  {
    const size_t rC = std::min(round_channels, j.C - r0);
    const std::vector<size_t> cut = split_channels(rC, G);
    std::vector<EncodeRun> runs(G);
    std::vector<EncodeSink> ss(G); // the members' shares: sized, their streams resident (no buffer, so `full` says nothing)
    std::vector<int> rets(G, DEGA_OK);
    std::vector<std::vector<uint64_t>> rel(G);
    std::vector<std::thread> th;
    for (size_t g = 0; g < G; g++)
      th.emplace_back([&, g] {
        Shape sj = j;
        sj.C = cut[g + 1] - cut[g];
        rel[g].assign(sj.C + 1, 0);
        ss[g].offsets = rel[g].data();
        ss[g].bits = sink.bits + r0 + cut[g];
        ss[g].err = sink.err + r0 + cut[g];
        if (j.count != nullptr)
          sj.count = j.count + r0 + cut[g];
        rets[g] = encode_share(grp->ctx[g], sj, (const uint8_t *)samples + (r0 + cut[g]) * (j.cmajor ? j.ld : 1) * esz, ss[g], false, runs[g]);
      });
    for (std::thread &t : th)
      t.join();
    {
      // a member that cannot keep its share resident after all (another process took memory meanwhile): a smaller round
      bool too_big = false;
      for (size_t g = 0; g < G; g++)
        too_big = too_big || (rets[g] == DEGA_ERROR_MEMORY && round_channels > G * 512);
      if (too_big)
      {
        round_channels = std::max<size_t>(G * 512, round_channels / 2 / 512 * 512);
        continue;
      }
    }
    for (size_t g = 0; g < G; g++)
      if (rets[g] != DEGA_OK)
        return group_fail(grp, rets[g], grp->ctx[g], g);
    // host-side concatenate: every device's streams go behind those of the devices (and rounds) in front of it
    std::vector<uint64_t> dev_base(G);
    for (size_t g = 0; g < G; g++)
    {
      dev_base[g] = sink.total;
      for (size_t i = 0; i < cut[g + 1] - cut[g]; i++)
        sink.offsets[r0 + cut[g] + i] = sink.total + rel[g][i];
      sink.total += ss[g].total;
    }
    sink.full = sink.full || sink.total > sink.packed_cap;
    if (!sink.full && // (else: keep sizing)
        (ret = on_members(grp, G, [&](size_t g) -> int { return encode_deliver(grp->ctx[g], runs[g], sink.packed, dev_base[g]); })) != DEGA_OK)
      return ret;
    r0 += rC;
  }
  sink.offsets[j.C] = sink.total;
  if (sink.full)
  {
    snprintf(grp->last_error, sizeof(grp->last_error), "packed buffer too small: offsets[C] holds the size needed");
    return DEGA_ERROR_MEMORY;
  }
  return DEGA_OK;
}

static int decode_on_group(dega_hip_group *grp, const Shape &j, const uint8_t *packed, const uint64_t *offsets, const uint64_t *bits, void *samples,
                           uint64_t *out_count, int32_t *err)
{
  if (grp == nullptr || grp->ctx.empty())
    return DEGA_ERROR_LIBRARY_INIT;
  int ret;
  if ((ret = check_job_shape(grp->ctx[0], j, 0)) != DEGA_OK || (ret = check_packed_input(grp->ctx[0], j, packed, offsets, bits)) != DEGA_OK)
    return group_fail(grp, ret, grp->ctx[0], 0);
  if (err == nullptr || (samples == nullptr && j.C * j.T != 0))
    return DEGA_ERROR_INVALID_VALUE;
  const size_t G = members_for(grp, j.C, 512);
  const size_t osz = sample_bytes(j);
  const std::vector<size_t> cut = split_channels(j.C, G);
  return on_members(grp, G, [&](size_t g) -> int {
    Shape sj = j;
    sj.C = cut[g + 1] - cut[g];
    return decode_share(grp->ctx[g], sj, packed, offsets + cut[g], bits + cut[g], (uint8_t *)samples + cut[g] * (j.cmajor ? j.ld : 1) * osz,
                        out_count != nullptr ? out_count + cut[g] : nullptr, err + cut[g]);
  });
}

extern "C" int dega_hip_group_encode(dega_hip_group *grp, const dega_hip_job *job, const void *samples, uint8_t *packed, size_t packed_cap,
                                     uint64_t *offsets, uint64_t *out_bits, int32_t *err)
{
  if (job == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  return encode_on_group(grp, shape_from_job(job), samples, packed_sink(packed, packed_cap, offsets, out_bits, err));
}

extern "C" int dega_hip_group_decode(dega_hip_group *grp, const dega_hip_job *job, const uint8_t *packed, const uint64_t *offsets, const uint64_t *in_bits,
                                     void *samples, uint64_t *out_count, int32_t *err)
{
  if (job == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  return decode_on_group(grp, shape_from_job(job), packed, offsets, in_bits, samples, out_count, err);
}

// ---- single-context forms ----------------------------------------------------------------------------------------------------

static int encode_on_ctx(dega_hip_ctx *ctx, const Shape &j, const void *samples, const EncodeSink &sink)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  dega_hip_group one = group_of_one(ctx);
  return encode_on_group(&one, j, samples, sink);
}

static int decode_on_ctx(dega_hip_ctx *ctx, const Shape &j, const uint8_t *packed, const uint64_t *offsets, const uint64_t *bits, void *samples,
                         uint64_t *out_count, int32_t *err)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  dega_hip_group one = group_of_one(ctx);
  return decode_on_group(&one, j, packed, offsets, bits, samples, out_count, err);
}

extern "C" int dega_hip_encode_job_host(dega_hip_ctx *ctx, const dega_hip_job *job, const void *samples, uint8_t *packed, size_t packed_cap,
                                        uint64_t *offsets, uint64_t *out_bits, int32_t *err)
{
  if (job == nullptr || offsets == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  return encode_on_ctx(ctx, shape_from_job(job), samples, packed_sink(packed, packed_cap, offsets, out_bits, err));
}

// ---- the counted job: a count per channel, host memory -------------------------------------------------------------------

static Shape counted_shape(const dega_hip_job *job, const uint64_t *count)
{
  Shape j = shape_from_job(job);
  j.count = count;
  return j;
}

extern "C" int dega_hip_encode_var_job_host(dega_hip_ctx *ctx, const dega_hip_job *job, const uint64_t *count, const void *samples, uint8_t *packed,
                                            size_t packed_cap, uint64_t *offsets, uint64_t *out_bits, int32_t *err)
{
  if (ctx == nullptr || job == nullptr || offsets == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (count == nullptr && job->C != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "encode: count must be a host array of job->C entries", hipSuccess);
  return encode_on_ctx(ctx, counted_shape(job, count), samples, packed_sink(packed, packed_cap, offsets, out_bits, err));
}

extern "C" int dega_hip_group_encode_var(dega_hip_group *grp, const dega_hip_job *job, const uint64_t *count, const void *samples, uint8_t *packed,
                                         size_t packed_cap, uint64_t *offsets, uint64_t *out_bits, int32_t *err)
{
  if (grp == nullptr || job == nullptr || offsets == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (count == nullptr && job->C != 0)
  {
    snprintf(grp->last_error, sizeof(grp->last_error), "encode: count must be a host array of job->C entries");
    return DEGA_ERROR_INVALID_VALUE;
  }
  return encode_on_group(grp, counted_shape(job, count), samples, packed_sink(packed, packed_cap, offsets, out_bits, err));
}

// ---- K granularities from one upload ---------------------------------------------------------------------------------------

// the arguments of the two levels forms; `what` gets the reason of a refusal
static int check_levels_job(const dega_hip_job *job, const size_t *num_values, size_t K, const void *samples, uint8_t *const *packed,
                            const size_t *packed_cap, uint64_t *const *offsets, uint64_t *const *out_bits, int32_t *const *err, const char **what)
{
  *what = "encode levels: at most 8 levels, every num_values at least 1, none twice";
  if (check_level_list(num_values, K) != DEGA_OK)
    return DEGA_ERROR_INVALID_VALUE;
  *what = "encode levels: the job's samples must be DEGA_SAMPLES_F32, ld >= C (channel-major: ld >= T)";
  if (job == nullptr || (job->samples & ~DEGA_SAMPLES_CHANNEL_MAJOR) != DEGA_SAMPLES_F32 ||
      job->ld < ((job->samples & DEGA_SAMPLES_CHANNEL_MAJOR) != 0 ? job->T : job->C))
    return DEGA_ERROR_INVALID_VALUE;
  *what = "encode levels: packed, packed_cap, offsets, out_bits and err are arrays of K entries, samples float32 rows";
  if (K != 0 && (packed == nullptr || packed_cap == nullptr || offsets == nullptr || out_bits == nullptr || err == nullptr))
    return DEGA_ERROR_INVALID_VALUE;
  for (size_t k = 0; k < K; k++)
    if (offsets[k] == nullptr || (job->C != 0 && (out_bits[k] == nullptr || err[k] == nullptr)) || (packed[k] == nullptr && packed_cap[k] != 0))
      return DEGA_ERROR_INVALID_VALUE;
  if ((samples == nullptr || ((uintptr_t)samples & 3u) != 0) && job->C * job->T != 0)
    return DEGA_ERROR_INVALID_VALUE;
  return DEGA_OK;
}

static int encode_levels_on_group(dega_hip_group *grp, const dega_hip_job *job, const size_t *num_values, size_t K, const void *samples,
                                  uint8_t *const *packed, const size_t *packed_cap, uint64_t *const *offsets, uint64_t *const *out_bits,
                                  int32_t *const *err)
{
  if (grp == nullptr || grp->ctx.empty())
    return DEGA_ERROR_LIBRARY_INIT;
  const Shape j = shape_from_job(job);
  int ret;
  for (size_t k = 0; k < K; k++) // what the K encode launches would refuse, before anything is enqueued
  {
    Shape lj = j;
    lj.T = dega_hip_aggregate_rows(j.T, num_values[k]);
    if ((ret = check_job_shape(grp->ctx[0], lj, 0)) != DEGA_OK)
      return group_fail(grp, ret, grp->ctx[0], 0);
    offsets[k][0] = 0;
  }
  if (K == 0)
    return DEGA_OK;
  const size_t G = members_for(grp, j.C, 512);
  PackedOut out[AGG_MAX_LEVELS]; // the call's outputs, level by level
  for (size_t k = 0; k < K; k++)
    out[k] = packed_out(packed[k], packed_cap[k], offsets[k], out_bits[k], err[k]);
  if (G == 1)
  {
    bool sized;
    ret = encode_levels_share(grp->ctx[0], j, num_values, K, samples, out, sized);
    return ret == DEGA_OK ? DEGA_OK : group_fail(grp, ret, grp->ctx[0], 0);
  }
  // Several members: contiguous channel ranges, one host thread each; every member delivers each level into a host
  // buffer of its own (no larger than the caller's: a share that does not fit there does not fit the call), and the
  // caller's packed[k] is filled by host-side copies once the sizes in front are known.
  const std::vector<size_t> cut = split_channels(j.C, G);
  std::vector<std::vector<PackedOut>> sinks(G, std::vector<PackedOut>(K));
  std::vector<std::vector<std::unique_ptr<uint8_t[]>>> tmp(G);
  std::vector<std::vector<std::vector<uint64_t>>> rel(G, std::vector<std::vector<uint64_t>>(K));
  for (size_t g = 0; g < G; g++)
  {
    tmp[g].resize(K);
    const size_t n = cut[g + 1] - cut[g];
    for (size_t k = 0; k < K; k++)
    {
      Shape lj = j;
      lj.T = dega_hip_aggregate_rows(j.T, num_values[k]);
      const size_t room = std::min(packed_cap[k], n * usual_cap(lj));
      tmp[g][k].reset(new uint8_t[std::max<size_t>(room, 1)]);
      rel[g][k].assign(n + 1, 0);
      sinks[g][k] = packed_out(tmp[g][k].get(), room, rel[g][k].data(), out_bits[k] + cut[g], err[k] + cut[g]);
    }
  }
  ret = on_members(grp, G, [&](size_t g) -> int {
    Shape sj = j;
    sj.C = cut[g + 1] - cut[g];
    const void *const src = (const uint8_t *)samples + cut[g] * (j.cmajor ? j.ld : 1) * sizeof(float);
    bool sized = false;
    int r = encode_levels_share(grp->ctx[g], sj, num_values, K, src, sinks[g].data(), sized);
    // A level that outgrew the member's buffer but fits the caller's (a chunk redone with worst-case slabs): once more,
    // with what it asked for.  Decided level by level: a level that does not fit the caller's buffer either stays
    // sized only, and the others are still delivered.
    bool retry = false;
    for (size_t k = 0; k < K && r == DEGA_ERROR_MEMORY && sized; k++)
      if (sinks[g][k].full && sinks[g][k].total <= packed_cap[k])
      {
        tmp[g][k].reset(new uint8_t[(size_t)sinks[g][k].total + 1]);
        sinks[g][k].packed = tmp[g][k].get();
        sinks[g][k].packed_cap = (size_t)sinks[g][k].total;
        retry = true;
      }
    if (retry)
      r = encode_levels_share(grp->ctx[g], sj, num_values, K, src, sinks[g].data(), sized);
    // any failure of a member is the call's, as in encode_on_group; DEGA_ERROR_MEMORY is "a packed buffer is too small"
    // only where the member sized all its channels (its levels' `full` say which) -- otherwise an allocation failed and
    // its outputs are incomplete
    return r == DEGA_ERROR_MEMORY && sized ? DEGA_OK : r;
  });
  if (ret != DEGA_OK)
    return ret;
  bool any_full = false;
  for (size_t k = 0; k < K; k++)
  {
    concat_members(cut, [&](size_t g) -> const PackedOut & { return sinks[g][k]; }, out[k]);
    any_full = any_full || out[k].full;
  }
  if (any_full)
  {
    snprintf(grp->last_error, sizeof(grp->last_error), "a level's packed buffer is too small: its offsets[C] holds the size needed");
    return DEGA_ERROR_MEMORY;
  }
  return DEGA_OK;
}

extern "C" int dega_hip_group_encode_levels(dega_hip_group *grp, const dega_hip_job *job, const size_t *num_values, size_t K, const void *samples,
                                            uint8_t *const *packed, const size_t *packed_cap, uint64_t *const *offsets, uint64_t *const *out_bits,
                                            int32_t *const *err)
{
  if (grp == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  const char *what;
  if (check_levels_job(job, num_values, K, samples, packed, packed_cap, offsets, out_bits, err, &what) != DEGA_OK)
  {
    snprintf(grp->last_error, sizeof(grp->last_error), "%s", what);
    return DEGA_ERROR_INVALID_VALUE;
  }
  return encode_levels_on_group(grp, job, num_values, K, samples, packed, packed_cap, offsets, out_bits, err);
}

extern "C" int dega_hip_encode_levels_job_host(dega_hip_ctx *ctx, const dega_hip_job *job, const size_t *num_values, size_t K, const void *samples,
                                               uint8_t *const *packed, const size_t *packed_cap, uint64_t *const *offsets, uint64_t *const *out_bits,
                                               int32_t *const *err)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  const char *what;
  if (check_levels_job(job, num_values, K, samples, packed, packed_cap, offsets, out_bits, err, &what) != DEGA_OK)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, what, hipSuccess);
  dega_hip_group one = group_of_one(ctx);
  return encode_levels_on_group(&one, job, num_values, K, samples, packed, packed_cap, offsets, out_bits, err);
}

// ---- one coarser granularity: the levels call with K = 1 -------------------------------------------------------------------

// the arguments of the two single-level forms; `what` gets the reason of a refusal
static int check_agg_job(const dega_hip_job *job, size_t num_values, const void *samples, uint8_t *packed, size_t packed_cap, uint64_t *offsets,
                         uint64_t *out_bits, int32_t *err, const char **what)
{
  *what = "encode_agg: num_values must be at least 1 and the job's samples DEGA_SAMPLES_F32";
  if (job == nullptr || num_values == 0 || (job->samples & ~DEGA_SAMPLES_CHANNEL_MAJOR) != DEGA_SAMPLES_F32 || offsets == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  return num_values == 1 ? DEGA_OK : check_levels_job(job, &num_values, 1, samples, &packed, &packed_cap, &offsets, &out_bits, &err, what);
}

// num_values = 1 is the plain call (the same streams: Normalize maps both zeros to 0), with its in-place and band paths
static int encode_agg_on_group(dega_hip_group *grp, const dega_hip_job *job, size_t num_values, const void *samples, uint8_t *packed, size_t packed_cap,
                               uint64_t *offsets, uint64_t *out_bits, int32_t *err)
{
  if (num_values == 1)
    return encode_on_group(grp, shape_from_job(job), samples, packed_sink(packed, packed_cap, offsets, out_bits, err));
  return encode_levels_on_group(grp, job, &num_values, 1, samples, &packed, &packed_cap, &offsets, &out_bits, &err);
}

extern "C" int dega_hip_group_encode_agg(dega_hip_group *grp, const dega_hip_job *job, size_t num_values, const void *samples, uint8_t *packed,
                                         size_t packed_cap, uint64_t *offsets, uint64_t *out_bits, int32_t *err)
{
  if (grp == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  const char *what;
  if (check_agg_job(job, num_values, samples, packed, packed_cap, offsets, out_bits, err, &what) != DEGA_OK)
  {
    snprintf(grp->last_error, sizeof(grp->last_error), "%s", what);
    return DEGA_ERROR_INVALID_VALUE;
  }
  return encode_agg_on_group(grp, job, num_values, samples, packed, packed_cap, offsets, out_bits, err);
}

extern "C" int dega_hip_encode_agg_job_host(dega_hip_ctx *ctx, const dega_hip_job *job, size_t num_values, const void *samples, uint8_t *packed,
                                            size_t packed_cap, uint64_t *offsets, uint64_t *out_bits, int32_t *err)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  const char *what;
  if (check_agg_job(job, num_values, samples, packed, packed_cap, offsets, out_bits, err, &what) != DEGA_OK)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, what, hipSuccess);
  dega_hip_group one = group_of_one(ctx);
  return encode_agg_on_group(&one, job, num_values, samples, packed, packed_cap, offsets, out_bits, err);
}

// float32 rows in host memory -> their sums in host memory, synchronous (first_slot_chunks): a chunk holds the two images
extern "C" int dega_hip_aggregate_host(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, size_t num_values, float *a_tc,
                                       size_t ld_out)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (num_values == 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate: num_values must be at least 1 (the reference does not terminate on 0)", hipSuccess);
  if (ld < C || ld_out < C)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "aggregate: ld < C or ld_out < C", hipSuccess);
  if (C == 0 || T == 0)
    return DEGA_OK;
  if (v_tc == nullptr || a_tc == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  const size_t T_out = dega_hip_aggregate_rows(T, num_values);
  const bool in_pinned = is_pinned(v_tc), out_pinned = is_pinned(a_tc);
  return first_slot_chunks(ctx, C, (T + T_out) * sizeof(float), [&](Pipeline *pl, Slot &sl, size_t c0, size_t n) -> int {
    HIP_TRY(ctx, sl.c.need(n * T * sizeof(float) + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.a.need(n * T_out * sizeof(float) + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, rows_to_device(pl, sl.s, sl.c.p, (const uint8_t *)(v_tc + c0), ld * sizeof(float), n * sizeof(float), T, in_pinned), DEGA_ERROR_LIBRARY_CALL);
    const int ret = launch_aggregate(ctx, (const float *)sl.c.p, n, T, n, num_values, (float *)sl.a.p, n, sl.s);
    if (ret != DEGA_OK)
      return ret;
    HIP_TRY(ctx, rows_to_host(pl, sl.s, (uint8_t *)(a_tc + c0), ld_out * sizeof(float), sl.a.p, n * sizeof(float), T_out, out_pinned), DEGA_ERROR_LIBRARY_CALL);
    return DEGA_OK;
  });
}

// float32 rows in host memory -> their text in host memory, synchronous, chunked as dega_hip_aggregate_host is: a chunk
// holds its readings and their text
extern "C" int dega_hip_csv_write_host(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, unsigned decimals, size_t column,
                                       int separator_char, uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  int ret;
  if ((ret = check_csv_options(ctx, C, ld, decimals, column, separator_char, stride)) != DEGA_OK)
    return ret;
  if (C == 0)
    return DEGA_OK;
  if (out == nullptr || out_len == nullptr || err == nullptr)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: out, out_len and err must be arrays", hipSuccess);
  if (T == 0)
  {
    memset(out_len, 0, C * sizeof(uint64_t));
    memset(err, 0, C * sizeof(int32_t));
    return DEGA_OK;
  }
  if (v_tc == nullptr)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv: v_tc must be a float32 array", hipSuccess);
  const bool in_pinned = is_pinned(v_tc), out_pinned = is_pinned(out), len_pinned = is_pinned(out_len), err_pinned = is_pinned(err);
  return first_slot_chunks(ctx, C, T * sizeof(float) + stride, [&](Pipeline *pl, Slot &sl, size_t c0, size_t n) -> int {
    HIP_TRY(ctx, sl.c.need(n * T * sizeof(float) + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.a.need(n * stride + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.meta.need(n * (sizeof(uint64_t) + sizeof(int32_t)) + 64), DEGA_ERROR_MEMORY);
    uint64_t *const d_len = (uint64_t *)sl.meta.p;
    int32_t *const d_err = (int32_t *)((uint8_t *)sl.meta.p + n * sizeof(uint64_t));
    HIP_TRY(ctx, rows_to_device(pl, sl.s, sl.c.p, (const uint8_t *)(v_tc + c0), ld * sizeof(float), n * sizeof(float), T, in_pinned), DEGA_ERROR_LIBRARY_CALL);
    if ((ret = launch_csv(ctx, (const float *)sl.c.p, n, T, n, decimals, column, separator_char, (uint8_t *)sl.a.p, stride, d_len, d_err, sl.s)) != DEGA_OK)
      return ret;
    HIP_TRY(ctx, rows_to_host(pl, sl.s, out + c0 * stride, stride, sl.a.p, stride, n, out_pinned), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, rows_to_host(pl, sl.s, (uint8_t *)(out_len + c0), n * sizeof(uint64_t), d_len, n * sizeof(uint64_t), 1, len_pinned), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, rows_to_host(pl, sl.s, (uint8_t *)(err + c0), n * sizeof(int32_t), d_err, n * sizeof(int32_t), 1, err_pinned), DEGA_ERROR_LIBRARY_CALL);
    return DEGA_OK;
  });
}

// Text rows in host memory -> float32 rows in host memory, synchronous, chunked likewise: a chunk holds its text and its values
extern "C" int dega_hip_csv_read_host(dega_hip_ctx *ctx, const uint8_t *text, size_t stride, const uint64_t *len, size_t C, size_t column,
                                      int separator_char, float *v_tc, size_t max_T, size_t ld, uint64_t *out_count, int32_t *err)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  int ret;
  if ((ret = check_csv_read_options(ctx, C, column, separator_char, stride, ld)) != DEGA_OK)
    return ret;
  if (C == 0)
    return DEGA_OK;
  if (text == nullptr || len == nullptr)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: text and len must be arrays", hipSuccess);
  if ((ret = check_csv_read_outputs(ctx, v_tc, max_T, out_count, err)) != DEGA_OK)
    return ret;
  for (size_t c = 0; c < C; c++)
    if (len[c] > stride)
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "csv read: a len[c] is larger than stride", hipSuccess);
  // a text of `stride` bytes holds at most `stride` values: more room than that is never used, and sizes stay far from wrapping
  const size_t rows = std::min(max_T, stride);
  const bool in_pinned = is_pinned(text), len_pinned = is_pinned(len), out_pinned = is_pinned(v_tc), count_pinned = is_pinned(out_count),
             err_pinned = is_pinned(err);
  return first_slot_chunks(ctx, C, rows * sizeof(float) + stride, [&](Pipeline *pl, Slot &sl, size_t c0, size_t n) -> int {
    HIP_TRY(ctx, sl.a.need(n * stride + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.c.need(n * rows * sizeof(float) + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.meta.need(n * (2 * sizeof(uint64_t) + sizeof(int32_t)) + 64), DEGA_ERROR_MEMORY);
    uint64_t *const d_len = (uint64_t *)sl.meta.p;
    uint64_t *const d_count = d_len + n;
    int32_t *const d_err = (int32_t *)(d_count + n);
    HIP_TRY(ctx, rows_to_device(pl, sl.s, sl.a.p, text + c0 * stride, stride, stride, n, in_pinned), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, rows_to_device(pl, sl.s, d_len, (const uint8_t *)(len + c0), n * sizeof(uint64_t), n * sizeof(uint64_t), 1, len_pinned),
            DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, hipMemsetAsync(sl.c.p, 0, n * rows * sizeof(float) + 64, sl.s), DEGA_ERROR_LIBRARY_CALL); // (rows beyond a channel's count come back as +0.0f)
    if ((ret = launch_csv_read(ctx, (const uint8_t *)sl.a.p, stride, d_len, n, column, separator_char, (float *)sl.c.p, rows, n, d_count, d_err,
                               sl.s)) != DEGA_OK)
      return ret;
    HIP_TRY(ctx, rows_to_host(pl, sl.s, (uint8_t *)(v_tc + c0), ld * sizeof(float), sl.c.p, n * sizeof(float), rows, out_pinned), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, rows_to_host(pl, sl.s, (uint8_t *)(out_count + c0), n * sizeof(uint64_t), d_count, n * sizeof(uint64_t), 1, count_pinned),
            DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, rows_to_host(pl, sl.s, (uint8_t *)(err + c0), n * sizeof(int32_t), d_err, n * sizeof(int32_t), 1, err_pinned), DEGA_ERROR_LIBRARY_CALL);
    return DEGA_OK;
  });
}

// Rows in host memory -> their A-XDR streams in host slabs, synchronous, chunked likewise: a chunk holds its rows and its
// slabs.  Of a slab only the stream's own bytes come back (the bytes behind them are the caller's): the chunk's bit lengths
// and statuses first, then one 2-D copy per run of channels whose streams are equally long -- one, for a uniform batch.
extern "C" int dega_hip_axdr_encode_host(dega_hip_ctx *ctx, const void *x_tc, int samples, size_t C, size_t T, size_t ld, const uint64_t *count, float factor,
                                         int valuesize, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err)
{
  int ret;
  if ((ret = check_axdr(ctx, samples, valuesize, C, T, ld, cap, x_tc, out, out_bits, err, count, false)) != DEGA_OK || C == 0)
    return ret;
  const size_t esz = samples == DEGA_SAMPLES_I64 ? 8 : 4;
  const bool in_pinned = is_pinned(x_tc), count_pinned = is_pinned(count), bits_pinned = is_pinned(out_bits), err_pinned = is_pinned(err);
  return first_slot_chunks(ctx, C, T * esz + cap + 16, [&](Pipeline *pl, Slot &sl, size_t c0, size_t n) -> int {
    HIP_TRY(ctx, sl.c.need(n * T * esz + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.b.need(n * cap + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.meta.need(MetaView::bytes(n)), DEGA_ERROR_MEMORY);
    MetaView dm(sl.meta.p, n);
    HIP_TRY(ctx, rows_to_device(pl, sl.s, sl.c.p, (const uint8_t *)x_tc + c0 * esz, ld * esz, n * esz, T, in_pinned), DEGA_ERROR_LIBRARY_CALL);
    if (count != nullptr)
      HIP_TRY(ctx, rows_to_device(pl, sl.s, dm.counts, (const uint8_t *)(count + c0), n * sizeof(uint64_t), n * sizeof(uint64_t), 1, count_pinned),
              DEGA_ERROR_LIBRARY_CALL);
    if ((ret = launch_axdr_pack(ctx, sl.c.p, samples, n, T, n, count != nullptr ? dm.counts : nullptr, factor, valuesize, (uint8_t *)sl.b.p, cap, dm.bits, dm.err,
                                sl.s)) != DEGA_OK)
      return ret;
    HIP_TRY(ctx, rows_to_host(pl, sl.s, (uint8_t *)(out_bits + c0), n * sizeof(uint64_t), dm.bits, n * sizeof(uint64_t), 1, bits_pinned), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, rows_to_host(pl, sl.s, (uint8_t *)(err + c0), n * sizeof(int32_t), dm.err, n * sizeof(int32_t), 1, err_pinned), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, pl->stager.drain(), DEGA_ERROR_LIBRARY_CALL);
    auto bytes_of = [&](size_t c) -> size_t { return err[c] == DEGA_OK ? (size_t)((out_bits[c] + 31) / 32 * 4) : 0; };
    for (size_t i = 0; i < n;)
    {
      const size_t len = bytes_of(c0 + i);
      size_t k = i + 1;
      while (k < n && bytes_of(c0 + k) == len)
        k++;
      if (len != 0)
        HIP_TRY(ctx, hipMemcpy2DAsync(out + (c0 + i) * cap, cap, (const uint8_t *)sl.b.p + i * cap, cap, len, k - i, hipMemcpyDeviceToHost, sl.s),
                DEGA_ERROR_LIBRARY_CALL);
      i = k;
    }
    return DEGA_OK;
  });
}

// A-XDR streams in host slabs -> rows in host memory, synchronous, chunked likewise.  Of a slab the bytes up to the longest
// stream of the chunk go up; the rows come back whole (those behind a channel's count as +0 / 0).
extern "C" int dega_hip_axdr_decode_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld,
                                         float factor, int valuesize, int samples, void *x_tc, uint64_t *out_count, int32_t *err)
{
  int ret;
  if ((ret = check_axdr(ctx, samples, valuesize, C, max_T, ld, cap, x_tc, in, in_bits, err, out_count, true)) != DEGA_OK || C == 0)
    return ret;
  const size_t esz = samples == DEGA_SAMPLES_I64 ? 8 : 4;
  const bool bits_pinned = is_pinned(in_bits), out_pinned = is_pinned(x_tc), count_pinned = is_pinned(out_count), err_pinned = is_pinned(err);
  return first_slot_chunks(ctx, C, max_T * esz + cap + 16, [&](Pipeline *pl, Slot &sl, size_t c0, size_t n) -> int {
    HIP_TRY(ctx, sl.a.need(n * cap + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.c.need(n * max_T * esz + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.meta.need(MetaView::bytes(n)), DEGA_ERROR_MEMORY);
    MetaView dm(sl.meta.p, n);
    uint64_t longest = 0;
    for (size_t c = c0; c < c0 + n; c++)
      longest = std::max(longest, std::min<uint64_t>(cap, (in_bits[c] + 31) / 32 * 4));
    if (longest > 0)
      HIP_TRY(ctx, hipMemcpy2DAsync(sl.a.p, cap, in + c0 * cap, cap, (size_t)longest, n, hipMemcpyHostToDevice, sl.s), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, rows_to_device(pl, sl.s, dm.bits, (const uint8_t *)(in_bits + c0), n * sizeof(uint64_t), n * sizeof(uint64_t), 1, bits_pinned),
            DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, hipMemsetAsync(sl.c.p, 0, n * max_T * esz + 64, sl.s), DEGA_ERROR_LIBRARY_CALL);
    if ((ret = launch_axdr_unpack(ctx, (const uint8_t *)sl.a.p, cap, dm.bits, n, max_T, n, factor, valuesize, samples, sl.c.p, dm.counts, dm.err, sl.s)) != DEGA_OK)
      return ret;
    HIP_TRY(ctx, rows_to_host(pl, sl.s, (uint8_t *)x_tc + c0 * esz, ld * esz, sl.c.p, n * esz, max_T, out_pinned), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, rows_to_host(pl, sl.s, (uint8_t *)(out_count + c0), n * sizeof(uint64_t), dm.counts, n * sizeof(uint64_t), 1, count_pinned),
            DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, rows_to_host(pl, sl.s, (uint8_t *)(err + c0), n * sizeof(int32_t), dm.err, n * sizeof(int32_t), 1, err_pinned), DEGA_ERROR_LIBRARY_CALL);
    return DEGA_OK;
  });
}

extern "C" int dega_hip_decode_job_host(dega_hip_ctx *ctx, const dega_hip_job *job, const uint8_t *packed, const uint64_t *offsets, const uint64_t *in_bits,
                                        void *samples, uint64_t *out_count, int32_t *err)
{
  if (job == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  return decode_on_ctx(ctx, shape_from_job(job), packed, offsets, in_bits, samples, out_count, err);
}

// slabs in and out: the older, simpler surface on top of the same pipeline
static int encode_slabs(dega_hip_ctx *ctx, const Shape &j, const void *samples, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (cap % 4 != 0)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "cap must be a multiple of 4", hipSuccess);
  if (out == nullptr && j.C != 0)
    return DEGA_ERROR_INVALID_VALUE;
  EncodeSink sink;
  sink.slabs = out;
  sink.slab_cap = cap;
  sink.bits = out_bits;
  sink.err = err;
  return encode_on_ctx(ctx, j, samples, sink);
}

static int decode_slabs(dega_hip_ctx *ctx, const Shape &j, const uint8_t *in, size_t cap, const uint64_t *in_bits, void *samples, uint64_t *out_count,
                        int32_t *err)
{
  if (ctx == nullptr || in_bits == nullptr || (in == nullptr && j.C != 0))
    return DEGA_ERROR_INVALID_VALUE;
  // pack on the host: only ceil(bits / 8) bytes per channel cross PCIe, not C x cap
  std::vector<uint64_t> offsets(j.C + 1, 0);
  for (size_t c = 0; c < j.C; c++)
  {
    const uint64_t nb = in_bits[c] / 8 + ((in_bits[c] & 7) != 0 ? 1 : 0);
    if (nb > cap)
      return fail(ctx, DEGA_ERROR_INVALID_VALUE, "a stream's bit length exceeds its slab", hipSuccess);
    offsets[c + 1] = offsets[c] + nb;
  }
  std::vector<uint8_t> packed((size_t)offsets[j.C] + 1);
  for (size_t c = 0; c < j.C; c++)
    memcpy(packed.data() + offsets[c], in + c * cap, (size_t)(offsets[c + 1] - offsets[c]));
  return decode_on_ctx(ctx, j, packed.data(), offsets.data(), in_bits, samples, out_count, err);
}

extern "C" int dega_hip_encode_host(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T, size_t ld, int adaptive, int valuesize,
                                    uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err)
{
  int ret;
  if ((ret = check_shape(ctx, C, T, ld, 0, valuesize)) != DEGA_OK)
    return ret;
  return encode_slabs(ctx, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_I32), x_tc, out, cap, out_bits, err);
}

extern "C" int dega_hip_decode_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t T, size_t ld,
                                    int adaptive, int valuesize, int32_t *x_tc, int32_t *err)
{
  int ret;
  if ((ret = check_shape(ctx, C, T, ld, 0, valuesize)) != DEGA_OK)
    return ret;
  return decode_slabs(ctx, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_I32), in, cap, in_bits, x_tc, nullptr, err);
}

extern "C" int dega_hip_decode_var_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld,
                                        int adaptive, int valuesize, int32_t *x_tc, uint64_t *out_count, int32_t *err)
{
  int ret;
  if (out_count == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if ((ret = check_shape(ctx, C, max_T, ld, 0, valuesize)) != DEGA_OK)
    return ret;
  return decode_slabs(ctx, shape_of(C, max_T, ld, adaptive, valuesize, DEGA_SAMPLES_I32), in, cap, in_bits, x_tc, out_count, err);
}

extern "C" int dega_hip_encode_f32_host(dega_hip_ctx *ctx, const float *v_tc, size_t C, size_t T, size_t ld, float factor, int adaptive, int valuesize,
                                        uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err)
{
  return encode_slabs(ctx, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_F32, factor), v_tc, out, cap, out_bits, err);
}

extern "C" int dega_hip_decode_f32_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t T, size_t ld,
                                        float factor, int adaptive, int valuesize, float *v_tc, int32_t *err)
{
  return decode_slabs(ctx, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_F32, factor), in, cap, in_bits, v_tc, nullptr, err);
}

extern "C" int dega_hip_decode_f32_var_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld,
                                            float factor, int adaptive, int valuesize, float *v_tc, uint64_t *out_count, int32_t *err)
{
  if (out_count == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  return decode_slabs(ctx, shape_of(C, max_T, ld, adaptive, valuesize, DEGA_SAMPLES_F32, factor), in, cap, in_bits, v_tc, out_count, err);
}

extern "C" int dega_hip_encode64_host(dega_hip_ctx *ctx, const int64_t *x_tc, size_t C, size_t T, size_t ld, int adaptive, int valuesize,
                                      uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err)
{
  int ret;
  if ((ret = check_shape64(ctx, C, T, ld, 0, valuesize)) != DEGA_OK)
    return ret;
  return encode_slabs(ctx, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_I64), x_tc, out, cap, out_bits, err);
}

extern "C" int dega_hip_decode64_var_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld,
                                          int adaptive, int valuesize, int64_t *x_tc, uint64_t *out_count, int32_t *err)
{
  int ret;
  if (out_count == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if ((ret = check_shape64(ctx, C, max_T, ld, 0, valuesize)) != DEGA_OK)
    return ret;
  return decode_slabs(ctx, shape_of(C, max_T, ld, adaptive, valuesize, DEGA_SAMPLES_I64), in, cap, in_bits, x_tc, out_count, err);
}

extern "C" int dega_hip_encode_packed_host(dega_hip_ctx *ctx, const int32_t *x_tc, size_t C, size_t T, size_t ld, int adaptive, int valuesize,
                                           uint8_t *packed, size_t packed_cap, uint64_t *offsets, uint64_t *out_bits, int32_t *err)
{
  int ret;
  if ((ret = check_shape(ctx, C, T, ld, 0, valuesize)) != DEGA_OK)
    return ret;
  if (offsets == nullptr || out_bits == nullptr || err == nullptr || (packed == nullptr && packed_cap != 0))
    return DEGA_ERROR_INVALID_VALUE;
  return encode_on_ctx(ctx, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_I32), x_tc, packed_sink(packed, packed_cap, offsets, out_bits, err));
}

extern "C" int dega_hip_decode_packed_host(dega_hip_ctx *ctx, const uint8_t *packed, const uint64_t *offsets, const uint64_t *in_bits, size_t C, size_t T,
                                           size_t ld, int adaptive, int valuesize, int32_t *x_tc, uint64_t *out_count, int32_t *err)
{
  int ret;
  if (ctx == nullptr || offsets == nullptr || in_bits == nullptr || x_tc == nullptr || err == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if ((ret = check_shape(ctx, C, T, ld, 0, valuesize)) != DEGA_OK)
    return ret;
  return decode_on_ctx(ctx, shape_of(C, T, ld, adaptive, valuesize, DEGA_SAMPLES_I32), packed, offsets, in_bits, x_tc, out_count, err);
}

// ---- pinned host memory for callers that can place their samples there (copies then run at link speed without staging) ---
extern "C" void *dega_hip_pinned_alloc(size_t bytes)
{
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes > 0 ? bytes : 1, hipHostMallocDefault) != hipSuccess)
  {
    (void)hipGetLastError();
    return nullptr;
  }
  return p;
}

extern "C" void dega_hip_pinned_free(void *p)
{
  if (p != nullptr)
    (void)hipHostFree(p);
}

// ---- LZMH, host pointers: context-owned buffers, no per-call allocation --------------------------------------------------------

// Synchronous, chunked as dega_hip_aggregate_host is: a chunk holds its texts and its slabs.  Plain copies from and to the
// caller's arrays, no staging ring.
extern "C" int dega_hip_lzmh_encode_host(dega_hip_ctx *ctx, const uint8_t *in, size_t stride, const uint64_t *in_len, size_t C, uint8_t *out,
                                         size_t cap, uint64_t *out_bits, int32_t *err)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (C == 0)
    return DEGA_OK;
  if (in == nullptr || in_len == nullptr || out == nullptr || out_bits == nullptr || err == nullptr)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh encode: in, in_len, out, out_bits and err must be arrays", hipSuccess);
  int ret;
  if ((ret = check_lzmh_encode(ctx, stride, cap, true)) != DEGA_OK)
    return ret;
  return first_slot_chunks(ctx, C, stride + cap, [&](Pipeline *, Slot &sl, size_t c0, size_t n) -> int {
    HIP_TRY(ctx, sl.a.need(n * stride + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.b.need(n * cap + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.meta.need(MetaView::bytes(n)), DEGA_ERROR_MEMORY);
    MetaView dm(sl.meta.p, n);
    HIP_TRY(ctx, hipMemcpyAsync(sl.a.p, in + c0 * stride, n * stride, hipMemcpyHostToDevice, sl.s), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, hipMemcpyAsync(dm.counts, in_len + c0, n * sizeof(uint64_t), hipMemcpyHostToDevice, sl.s), DEGA_ERROR_LIBRARY_CALL);
    if ((ret = dega_hip_lzmh_encode_dev(ctx, (const uint8_t *)sl.a.p, stride, dm.counts, n, (uint8_t *)sl.b.p, cap, dm.bits, dm.err, sl.s)) != DEGA_OK)
      return ret;
    HIP_TRY(ctx, hipMemcpyAsync(out_bits + c0, dm.bits, n * sizeof(uint64_t), hipMemcpyDeviceToHost, sl.s), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, hipMemcpyAsync(err + c0, dm.err, n * sizeof(int32_t), hipMemcpyDeviceToHost, sl.s), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL);
    // only the bytes each stream of the chunk holds come back (whole 16-byte groups, as the kernel stores them)
    uint64_t longest = 0;
    for (size_t c = c0; c < c0 + n; c++)
      longest = std::max(longest, std::min<uint64_t>(cap, ((out_bits[c] + 7) / 8 + 15) / 16 * 16));
    if (longest > 0)
      HIP_TRY(ctx, hipMemcpy2DAsync(out + c0 * cap, cap, sl.b.p, cap, (size_t)longest, n, hipMemcpyDeviceToHost, sl.s), DEGA_ERROR_LIBRARY_CALL);
    return DEGA_OK;
  });
}

extern "C" int dega_hip_lzmh_decode_host(dega_hip_ctx *ctx, const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, uint8_t *out,
                                         size_t stride, uint64_t *out_len, int32_t *err)
{
  if (ctx == nullptr)
    return DEGA_ERROR_INVALID_VALUE;
  if (C == 0)
    return DEGA_OK;
  if (in == nullptr || in_bits == nullptr || out == nullptr || out_len == nullptr || err == nullptr)
    return fail(ctx, DEGA_ERROR_INVALID_VALUE, "lzmh decode: in, in_bits, out, out_len and err must be arrays", hipSuccess);
  int ret;
  if ((ret = check_lzmh_decode(ctx, cap, stride, true)) != DEGA_OK)
    return ret;
  return first_slot_chunks(ctx, C, stride + cap, [&](Pipeline *, Slot &sl, size_t c0, size_t n) -> int {
    HIP_TRY(ctx, sl.a.need(n * cap + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.b.need(n * stride + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.meta.need(MetaView::bytes(n)), DEGA_ERROR_MEMORY);
    MetaView dm(sl.meta.p, n);
    HIP_TRY(ctx, hipMemcpyAsync(sl.a.p, in + c0 * cap, n * cap, hipMemcpyHostToDevice, sl.s), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, hipMemcpyAsync(dm.bits, in_bits + c0, n * sizeof(uint64_t), hipMemcpyHostToDevice, sl.s), DEGA_ERROR_LIBRARY_CALL);
    if ((ret = dega_hip_lzmh_decode_dev(ctx, (const uint8_t *)sl.a.p, cap, dm.bits, n, (uint8_t *)sl.b.p, stride, dm.counts, dm.err, sl.s)) != DEGA_OK)
      return ret;
    HIP_TRY(ctx, hipMemcpyAsync(out + c0 * stride, sl.b.p, n * stride, hipMemcpyDeviceToHost, sl.s), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, hipMemcpyAsync(out_len + c0, dm.counts, n * sizeof(uint64_t), hipMemcpyDeviceToHost, sl.s), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, hipMemcpyAsync(err + c0, dm.err, n * sizeof(int32_t), hipMemcpyDeviceToHost, sl.s), DEGA_ERROR_LIBRARY_CALL);
    return DEGA_OK;
  });
}

// ---- LZMH through the pipeline: chunks of channels on their own streams, packed streams out / in, and the group -----------
// A channel's text is a row of `stride` bytes ([C][stride], in_len[c] of them meaningful), so a range of channels is one
// contiguous block: upload -> encode kernel -> offsets -> gather -> download of the packed stream bytes per chunk, the
// chunks overlapping on their streams exactly as the DEGA path's do.  Channels are independent (every stream starts from
// an empty history: lzmh.c:139-143,396), so a group gives every device a contiguous range and the host concatenates.

static ChunkPlan lzmh_plan(size_t C, size_t stride, size_t cap)
{
  ChunkPlan p = plan_chunks(C, stride, 2 * stride + 2 * cap + 64, 0);
  // (whole 256-channel workgroups per chunk where the batch allows: plan_chunks rounds to 512)
  return p;
}

static int lzmh_encode_share(dega_hip_ctx *ctx, const uint8_t *in, size_t stride, const uint64_t *in_len, size_t C, PackedOut &out)
{
  int ret;
  Pipeline *pl;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  if ((ret = pipeline_get(ctx, &pl)) != DEGA_OK)
    return ret;
  const size_t cap = dega_hip_lzmh_worst_case_bytes(stride);
  const ChunkPlan plan = lzmh_plan(C, stride, cap);
  const bool in_pinned = is_pinned(in), out_pinned = is_pinned(out.packed);
  std::vector<Chunk> chunks(plan.nchunks);
  out.total = 0;
  out.full = false;
  auto stage1 = [&](size_t k) -> int {
    Chunk &ch = chunks[k];
    ch.place(plan, C, k);
    Slot &sl = pl->slot[ch.slot];
    int r;
    if ((r = slot_stream(ctx, sl)) != DEGA_OK)
      return r;
    HIP_TRY(ctx, sl.a.need(ch.n * stride + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.b.need(ch.n * cap + 64), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.meta.need(MetaView::bytes(ch.n)), DEGA_ERROR_MEMORY);
    HIP_TRY(ctx, sl.hmeta.need(MetaView::bytes(ch.n)), DEGA_ERROR_MEMORY);
    MetaView hm(sl.hmeta.p, ch.n), dm(sl.meta.p, ch.n);
    memcpy(hm.counts, in_len + ch.c0, ch.n * sizeof(uint64_t));
    HIP_TRY(ctx, hipMemcpyAsync(dm.counts, hm.counts, ch.n * sizeof(uint64_t), hipMemcpyHostToDevice, sl.s), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, rows_to_device(pl, sl.s, sl.a.p, in + ch.c0 * stride, ch.n * stride, ch.n * stride, 1, in_pinned), DEGA_ERROR_LIBRARY_CALL);
    if ((r = dega_hip_lzmh_encode_dev(ctx, (const uint8_t *)sl.a.p, stride, dm.counts, ch.n, (uint8_t *)sl.b.p, cap, dm.bits, dm.err, sl.s)) != DEGA_OK)
      return r;
    return sizes_home(ctx, sl.s, dm, ch.n, sl.hmeta.p); // (the lengths come back with the set, as they went up)
  };
  auto stage2 = [&](size_t k) -> int {
    const Chunk &ch = chunks[k];
    Slot &sl = pl->slot[ch.slot];
    MetaView hm(sl.hmeta.p, ch.n), dm(sl.meta.p, ch.n);
    HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL);
    const size_t tot = (size_t)hm.offsets[ch.n];
    uint64_t base;
    if (!chunk_sized(out, ch.c0, ch.n, hm, base))
      return DEGA_OK;
    HIP_TRY(ctx, sl.c.need(tot + 64), DEGA_ERROR_MEMORY);
    return chunk_home(ctx, pl, sl.s, out.packed + base, out_pinned, tot, nullptr, sl.b.p, cap, dm.offsets, ch.n, sl.c.p);
  };
  if ((ret = run_chunks(plan.nchunks, (size_t)plan.nslots, stage1, stage2)) != DEGA_OK || (ret = finish_slots(ctx, pl, plan.nslots)) != DEGA_OK)
    return ret;
  out.offsets[C] = out.total;
  if (out.full)
    return fail(ctx, DEGA_ERROR_MEMORY, "packed buffer too small: offsets[C] holds the size needed", hipSuccess);
  return DEGA_OK;
}

static int lzmh_decode_share(dega_hip_ctx *ctx, const uint8_t *packed, const uint64_t *offsets, const uint64_t *in_bits, size_t C, uint8_t *out, size_t stride,
                             uint64_t *out_len, int32_t *err)
{
  int ret;
  Pipeline *pl;
  HIP_TRY(ctx, hipSetDevice(ctx->device), DEGA_ERROR_LIBRARY_CALL);
  if ((ret = pipeline_get(ctx, &pl)) != DEGA_OK)
    return ret;
  uint64_t longest_all = 0;
  for (size_t c = 0; c < C; c++)
    longest_all = std::max<uint64_t>(longest_all, offsets[c + 1] - offsets[c]);
  const ChunkPlan plan = lzmh_plan(C, stride, (size_t)longest_all + 32);
  const bool in_pinned = is_pinned(packed), out_pinned = is_pinned(out);
  std::vector<Chunk> chunks(plan.nchunks);
  auto stage1 = [&](size_t k) -> int {
    Chunk &ch = chunks[k];
    ch.place(plan, C, k);
    Slot &sl = pl->slot[ch.slot];
    int r;
    if ((r = slot_stream(ctx, sl)) != DEGA_OK)
      return r;
    HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL); // the pinned mirror is about to be rewritten
    size_t cap;
    HIP_TRY(ctx, sl.c.need(ch.n * stride + 64), DEGA_ERROR_MEMORY);
    if ((r = chunk_in(ctx, pl, sl, sl.s, packed, offsets + ch.c0, in_bits + ch.c0, ch.n, in_pinned, 0, cap)) != DEGA_OK)
      return r;
    MetaView hm(sl.hmeta.p, ch.n), dm(sl.meta.p, ch.n);
    if ((r = dega_hip_lzmh_decode_dev(ctx, (const uint8_t *)sl.b.p, cap, dm.bits, ch.n, (uint8_t *)sl.c.p, stride, dm.counts, dm.err, sl.s)) != DEGA_OK)
      return r;
    HIP_TRY(ctx, hipMemcpyAsync(hm.counts, dm.counts, ch.n * sizeof(uint64_t) + ch.n * sizeof(int32_t), hipMemcpyDeviceToHost, sl.s), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, rows_to_host(pl, sl.s, out + ch.c0 * stride, ch.n * stride, sl.c.p, ch.n * stride, 1, out_pinned), DEGA_ERROR_LIBRARY_CALL);
    return DEGA_OK;
  };
  auto stage2 = [&](size_t k) -> int {
    const Chunk &ch = chunks[k];
    Slot &sl = pl->slot[ch.slot];
    HIP_TRY(ctx, pl->stager.drain(), DEGA_ERROR_LIBRARY_CALL);
    HIP_TRY(ctx, hipStreamSynchronize(sl.s), DEGA_ERROR_LIBRARY_CALL);
    MetaView hm(sl.hmeta.p, ch.n);
    for (size_t i = 0; i < ch.n; i++)
    {
      out_len[ch.c0 + i] = hm.counts[i];
      err[ch.c0 + i] = hm.err[i];
    }
    return DEGA_OK;
  };
  return run_chunks(plan.nchunks, (size_t)plan.nslots, stage1, stage2);
}

static int lzmh_check(dega_hip_group *grp, size_t stride, bool encode)
{
  if (grp == nullptr || grp->ctx.empty())
    return DEGA_ERROR_LIBRARY_INIT;
  if (encode ? (stride == 0 || (stride & 15u) != 0 || stride > 0x7FFFFFF0u) : (stride < 8 || (stride & 7u) != 0))
  {
    snprintf(grp->last_error, sizeof(grp->last_error), encode ? "lzmh encode: stride must be a multiple of 16" : "lzmh decode: stride must be a multiple of 8");
    return DEGA_ERROR_INVALID_VALUE;
  }
  return DEGA_OK;
}

extern "C" int dega_hip_group_lzmh_encode(dega_hip_group *grp, const uint8_t *in, size_t stride, const uint64_t *in_len, size_t C, uint8_t *packed,
                                          size_t packed_cap, uint64_t *offsets, uint64_t *out_bits, int32_t *err)
{
  int ret;
  if ((ret = lzmh_check(grp, stride, true)) != DEGA_OK)
    return ret;
  if (offsets == nullptr || out_bits == nullptr || err == nullptr || in_len == nullptr || (in == nullptr && C != 0) || (packed == nullptr && packed_cap != 0))
    return DEGA_ERROR_INVALID_VALUE;
  offsets[0] = 0;
  if (C == 0)
    return DEGA_OK;
  const size_t G = members_for(grp, C, 256);
  PackedOut out = packed_out(packed, packed_cap, offsets, out_bits, err);
  if (G == 1)
  {
    ret = lzmh_encode_share(grp->ctx[0], in, stride, in_len, C, out);
    return ret == DEGA_OK ? DEGA_OK : group_fail(grp, ret, grp->ctx[0], 0);
  }
  // every device codes its range of channels into a buffer of its own; the host puts them behind one another
  const std::vector<size_t> cut = split_channels(C, G, 256);
  std::vector<std::vector<uint8_t>> tmp(G);
  std::vector<std::vector<uint64_t>> rel(G);
  std::vector<PackedOut> share(G);
  ret = on_members(grp, G, [&](size_t g) -> int {
    const size_t n = cut[g + 1] - cut[g];
    uint64_t text = 0;
    for (size_t i = 0; i < n; i++)
      text += in_len[cut[g] + i];
    tmp[g].resize((size_t)(text + text / 4 + 64 * n + 64)); // a stream is at most 10 bits per byte of text
    rel[g].assign(n + 1, 0);
    share[g] = packed_out(tmp[g].data(), tmp[g].size(), rel[g].data(), out_bits + cut[g], err + cut[g]);
    return n == 0 ? DEGA_OK : lzmh_encode_share(grp->ctx[g], in + cut[g] * stride, stride, in_len + cut[g], n, share[g]);
  });
  if (ret != DEGA_OK)
    return ret;
  concat_members(cut, [&](size_t g) -> const PackedOut & { return share[g]; }, out);
  if (out.full)
  {
    snprintf(grp->last_error, sizeof(grp->last_error), "packed buffer too small: offsets[C] holds the size needed");
    return DEGA_ERROR_MEMORY;
  }
  return DEGA_OK;
}

extern "C" int dega_hip_group_lzmh_decode(dega_hip_group *grp, const uint8_t *packed, const uint64_t *offsets, const uint64_t *in_bits, size_t C, uint8_t *out,
                                          size_t stride, uint64_t *out_len, int32_t *err)
{
  int ret;
  if ((ret = lzmh_check(grp, stride, false)) != DEGA_OK)
    return ret;
  if (offsets == nullptr || in_bits == nullptr || out_len == nullptr || err == nullptr || (out == nullptr && C != 0))
    return DEGA_ERROR_INVALID_VALUE;
  if (C == 0)
    return DEGA_OK;
  if (const char *const what = packed_input_fault(C, offsets, in_bits, (uint64_t)1 << 31, nullptr))
  {
    snprintf(grp->last_error, sizeof(grp->last_error), "%s", what);
    return DEGA_ERROR_INVALID_VALUE;
  }
  const size_t G = members_for(grp, C, 256);
  const std::vector<size_t> cut = split_channels(C, G, 256);
  return on_members(grp, G, [&](size_t g) -> int {
    const size_t n = cut[g + 1] - cut[g];
    return n == 0 ? DEGA_OK
                  : lzmh_decode_share(grp->ctx[g], packed, offsets + cut[g], in_bits + cut[g], n, out + cut[g] * stride, stride, out_len + cut[g], err + cut[g]);
  });
}
