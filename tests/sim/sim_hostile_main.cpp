// sim_hostile_main.cpp -- the emulated decoders on a corpus of damaged streams, as a stand-alone program for the host
// sanitizers (tests/sim/Makefile `hostile_asan`; started by tests/test_decode_hostile_host.py as a child process).
// TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Every buffer is a heap block of exactly the size the decoder is told about --
// C * cap bytes in, room * ld samples out -- so a read or a write past either end is the sanitizer's to report.
//
//   sim_hostile <corpus file> <result file>
// corpus file: 8 x uint64 {magic, C, cap, room, valuesize, adaptive, shape (0: three waves per group, 1: wide pairs,
//              2: 64-bit containers, 3: the LZMH decoder -- room is then the bytes of an output row, valuesize and adaptive
//              are not used), drag (microseconds per step of the parsing side -- LZMH: the writing side --, 0: none)},
//              bits uint64 [C], slabs uint8 [C][cap]
// result file: err int32 [C], counts uint64 [C], samples [room][C] (int32, or int64 for shape 2; shape 3: bytes uint8 [C][room])
#include "sim_main.cpp"

#include <memory>

static const uint64_t HOSTILE_MAGIC = 0x454c4954534f48ull; // "HOSTILE"

int main(int argc, char **argv)
{
  if (argc != 3)
  {
    fprintf(stderr, "usage: %s corpus result\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  uint64_t head[8];
  if (f == nullptr || fread(head, sizeof(uint64_t), 8, f) != 8 || head[0] != HOSTILE_MAGIC)
  {
    fprintf(stderr, "%s: not a corpus file\n", argv[1]);
    return 2;
  }
  const size_t C = head[1], cap = head[2], room = head[3];
  const int valuesize = (int)head[4], adaptive = (int)head[5], shape = (int)head[6], drag_us = (int)head[7];
  const size_t width = shape == 2 ? 8 : shape == 3 ? 1 : 4;
  std::unique_ptr<uint64_t[]> bits(new uint64_t[C]);
  std::unique_ptr<uint8_t[]> slabs(new uint8_t[C * cap]);
  if (fread(bits.get(), sizeof(uint64_t), C, f) != C || fread(slabs.get(), 1, C * cap, f) != C * cap)
  {
    fprintf(stderr, "%s: short corpus file\n", argv[1]);
    return 2;
  }
  fclose(f);
  std::unique_ptr<int32_t[]> err(new int32_t[C]);
  std::unique_ptr<uint64_t[]> counts(new uint64_t[C]);
  std::unique_ptr<uint8_t[]> x(new uint8_t[room * C * width]); // (operator new aligns for any sample type)
  memset(x.get(), 0, room * C * width);
  if (drag_us > 0)
    sim_set_drag(shape == 1 ? 8 : 4, drag_us); // the parsing waves (and the loading waves behind them) of either workgroup shape; LZMH's writing waves
  if (shape == 3)
    sim_lzmh_decode(slabs.get(), cap, bits.get(), C, x.get(), room, counts.get(), err.get());
  else if (shape == 2)
    sim_decode64(slabs.get(), cap, bits.get(), C, room, C, adaptive, valuesize, reinterpret_cast<int64_t *>(x.get()), counts.get(), err.get());
  else if (shape == 1)
    sim_decode_wide_var(slabs.get(), cap, bits.get(), C, room, C, adaptive, reinterpret_cast<int32_t *>(x.get()), counts.get(), err.get());
  else
    sim_decode_var_vs(slabs.get(), cap, bits.get(), C, room, C, adaptive, valuesize, reinterpret_cast<int32_t *>(x.get()), counts.get(), err.get());
  FILE *g = fopen(argv[2], "wb");
  if (g == nullptr || fwrite(err.get(), sizeof(int32_t), C, g) != C || fwrite(counts.get(), sizeof(uint64_t), C, g) != C ||
      fwrite(x.get(), width, room * C, g) != room * C || fclose(g) != 0)
  {
    fprintf(stderr, "%s: cannot write\n", argv[2]);
    return 2;
  }
  return 0;
}
