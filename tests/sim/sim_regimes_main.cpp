// sim_regimes_main.cpp -- the emulated encoder on the steered input corpus (tests/encoder_regimes_common.py), as a
// stand-alone program for the host sanitizers (tests/sim/Makefile `regimes_asan`; started by
// tests/test_encoder_regimes_host.py as a child process).  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Every buffer is a heap
// block of exactly the size the encoder is told about -- T * C samples in, C * cap bytes out --, so a read or a write past
// either end, a carry that runs past the front of a slab included, is the sanitizer's to report.
//
//   sim_regimes <corpus file> <result file>
// corpus file: 8 x uint64 {magic, C, T, adaptive, cap of the full slab (bytes, a multiple of 4), number of cuts, number of
//              short caps, 0}, cuts uint64 [] (0 ... T), short caps uint64 [], x int32 [T][C]
// result file: one block {err int32 [C], bits uint64 [C], out uint8 [C][cap]} per call: one launch at the full slab, the
//              launches of the cuts at the full slab, then one launch per short cap
#include "sim_main.cpp"

#include <memory>

static const uint64_t REGIMES_MAGIC = 0x53454d49474552ull; // "REGIMES"

static bool write_block(FILE *g, size_t C, size_t cap, const int32_t *err, const uint64_t *bits, const uint8_t *out)
{
  return fwrite(err, sizeof(int32_t), C, g) == C && fwrite(bits, sizeof(uint64_t), C, g) == C && fwrite(out, 1, C * cap, g) == C * cap;
}

int main(int argc, char **argv)
{
  if (argc != 3)
  {
    fprintf(stderr, "usage: %s corpus result\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  uint64_t head[8];
  if (f == nullptr || fread(head, sizeof(uint64_t), 8, f) != 8 || head[0] != REGIMES_MAGIC)
  {
    fprintf(stderr, "%s: not a corpus file\n", argv[1]);
    return 2;
  }
  const size_t C = head[1], T = head[2], full = head[4], ncuts = head[5], ncaps = head[6];
  const int adaptive = (int)head[3];
  std::unique_ptr<uint64_t[]> cuts64(new uint64_t[ncuts]), caps(new uint64_t[ncaps]);
  std::unique_ptr<int32_t[]> x(new int32_t[T * C]);
  if (fread(cuts64.get(), sizeof(uint64_t), ncuts, f) != ncuts || fread(caps.get(), sizeof(uint64_t), ncaps, f) != ncaps ||
      fread(x.get(), sizeof(int32_t), T * C, f) != T * C)
  {
    fprintf(stderr, "%s: short corpus file\n", argv[1]);
    return 2;
  }
  fclose(f);
  std::unique_ptr<size_t[]> cuts(new size_t[ncuts]);
  for (size_t k = 0; k < ncuts; k++)
    cuts[k] = (size_t)cuts64[k];
  FILE *g = fopen(argv[2], "wb");
  if (g == nullptr)
  {
    fprintf(stderr, "%s: cannot write\n", argv[2]);
    return 2;
  }
  std::unique_ptr<int32_t[]> err(new int32_t[C]);
  std::unique_ptr<uint64_t[]> bits(new uint64_t[C]);
  bool ok = true;
  for (size_t call = 0; call < 2 + ncaps && ok; call++)
  {
    const size_t cap = call < 2 ? full : (size_t)caps[call - 2];
    std::unique_ptr<uint8_t[]> out(new uint8_t[C * cap]);
    memset(out.get(), 0, C * cap);
    if (call == 1)
      sim_encode_segments(x.get(), C, T, C, 0, 0.0f, adaptive, 32, cuts.get(), (int)ncuts, out.get(), cap, bits.get(), err.get());
    else
      sim_encode(x.get(), C, T, C, adaptive, out.get(), cap, bits.get(), err.get());
    ok = write_block(g, C, cap, err.get(), bits.get(), out.get());
  }
  if (!ok || fclose(g) != 0)
  {
    fprintf(stderr, "%s: cannot write\n", argv[2]);
    return 2;
  }
  return 0;
}
