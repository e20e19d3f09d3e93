// sim_lzmh_encoder_main.cpp -- the emulated LZMH encoder on the steered text corpus (tests/lzmh_encoder_common.py), as a
// stand-alone program for the host sanitizers (tests/sim/Makefile `lzmh_encoder_asan`; started by
// tests/test_lzmh_encoder_host.py as a child process).  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Every buffer is a heap
// block of exactly the size the encoder is told about -- C * stride bytes of rows (16-byte aligned, as the entry point
// demands), C lengths, C * cap bytes of slabs --, so the last row ends with its allocation and a window load before a row's
// start or past the last row's end, or a store past a slab's, is the sanitizer's to report.
//
//   sim_lzmh_encoder <corpus file> <result file>
// corpus file: 8 x uint64 {magic, C, stride, number of forms, cap of the full slab, number of short caps, drag (microseconds
//              per pass of the coding waves, 0: none), 0}, short caps uint64 [], lens uint64 [C], rows uint8 [forms][C][stride]
// result file: one block {err int32 [C], bits uint64 [C], out uint8 [C][cap]} per call: every form at the full slab, then the
//              LAST form once per short cap; the slabs come filled with 0xA5
#include "sim_main.cpp"

#include <cstdlib>
#include <memory>

static const uint64_t LZENC_MAGIC = 0x434e45484d5a4cull; // "LZMHENC"

struct FreeDeleter
{
  void operator()(void *p) const { free(p); }
};

int main(int argc, char **argv)
{
  if (argc != 3)
  {
    fprintf(stderr, "usage: %s corpus result\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  uint64_t head[8];
  if (f == nullptr || fread(head, sizeof(uint64_t), 8, f) != 8 || head[0] != LZENC_MAGIC)
  {
    fprintf(stderr, "%s: not a corpus file\n", argv[1]);
    return 2;
  }
  const size_t C = head[1], stride = head[2], forms = head[3], full = head[4], ncaps = head[5];
  const int drag_us = (int)head[6];
  if (C == 0 || stride == 0 || stride % 16 != 0 || forms == 0)
  {
    fprintf(stderr, "%s: bad shape\n", argv[1]);
    return 2;
  }
  std::unique_ptr<uint64_t[]> caps(new uint64_t[ncaps]), lens(new uint64_t[C]);
  std::unique_ptr<std::unique_ptr<uint8_t, FreeDeleter>[]> rows(new std::unique_ptr<uint8_t, FreeDeleter>[forms]);
  bool ok = fread(caps.get(), sizeof(uint64_t), ncaps, f) == ncaps && fread(lens.get(), sizeof(uint64_t), C, f) == C;
  for (size_t k = 0; k < forms && ok; k++)
  {
    rows[k].reset(static_cast<uint8_t *>(aligned_alloc(16, C * stride)));
    ok = rows[k] != nullptr && fread(rows[k].get(), 1, C * stride, f) == C * stride;
  }
  if (!ok)
  {
    fprintf(stderr, "%s: short corpus file\n", argv[1]);
    return 2;
  }
  fclose(f);
  FILE *g = fopen(argv[2], "wb");
  if (g == nullptr)
  {
    fprintf(stderr, "%s: cannot write\n", argv[2]);
    return 2;
  }
  if (drag_us > 0)
    sim_set_drag(4, drag_us); // waves 4..7 of the workgroup are the coding waves
  std::unique_ptr<int32_t[]> err(new int32_t[C]);
  std::unique_ptr<uint64_t[]> bits(new uint64_t[C]);
  for (size_t call = 0; call < forms + ncaps && ok; call++)
  {
    const size_t cap = call < forms ? full : (size_t)caps[call - forms];
    const uint8_t *in = rows[call < forms ? call : forms - 1].get();
    std::unique_ptr<uint8_t, FreeDeleter> out(static_cast<uint8_t *>(aligned_alloc(16, C * cap)));
    if (out == nullptr || cap % 16 != 0)
      return 2;
    memset(out.get(), 0xA5, C * cap);
    sim_lzmh_encode(in, stride, lens.get(), C, out.get(), cap, bits.get(), err.get());
    ok = fwrite(err.get(), sizeof(int32_t), C, g) == C && fwrite(bits.get(), sizeof(uint64_t), C, g) == C && fwrite(out.get(), 1, C * cap, g) == C * cap;
  }
  if (!ok || fclose(g) != 0)
  {
    fprintf(stderr, "%s: cannot write\n", argv[2]);
    return 2;
  }
  return 0;
}
