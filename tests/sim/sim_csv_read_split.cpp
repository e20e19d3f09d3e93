// sim_csv_read_split.cpp -- runs the shipped split `decode csv` kernels (data-compressor_amd/csrc/csv_read_split_kernels.hpp)
// under the thread-per-lane emulator of hipsim.hpp, through the header's own launch table.  TEST INFRASTRUCTURE ONLY; see
// hipsim.hpp.  Built by the pattern rule of tests/sim/Makefile (libcsv_read_split_sim.so) for
// tests/test_csv_read_split_host.py, and included by sim_csv_read_split_main.cpp (the stand-alone sanitizer program).
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "sim_launch.hpp"

#include "../../data-compressor_amd/csrc/csv_read_split_kernels.hpp"

#include <vector>

using namespace dg;

// Guards what the kernels rely on (what dega_hip_csv_read_split_dev refuses; the library's own checks are tested on the
// GPU); block_bytes 0 is the library's choice.  The [C][blocks] array between the launches is exactly as large as it may be.
extern "C" __attribute__((visibility("default"))) int sim_csv_read_split(const uint8_t *text, size_t stride, const uint64_t *len, size_t C, size_t column,
                                                                         int sep, float *v, size_t max_T, size_t ld, uint64_t *out_count, int32_t *err,
                                                                         size_t block_bytes)
{
  if (C == 0 || column == 0 || sep < 0 || sep > 255 || ld < C || stride < 16 || stride % 16 != 0 || stride > 0x7FFFFFF0u ||
      ((uintptr_t)text & 15u) != 0 || ((uintptr_t)v & 3u) != 0)
    return -1;
  for (size_t c = 0; c < C; c++)
    if (len[c] > stride)
      return -1;
  if (block_bytes == 0)
    block_bytes = csv_read_split_block_bytes(C, stride);
  if (block_bytes < 16 || block_bytes % 16 != 0)
    return -1;
  std::vector<uint32_t> work(C * csv_read_split_blocks(stride, block_bytes));
  const CsvReadArgs r = csv_read_args(text, stride, len, C, column, sep, v, max_T, ld, out_count, err);
  return launch(csv_read_split_args(r, block_bytes, work.data()), OnEmulator{}) ? 0 : -1;
}

extern "C" __attribute__((visibility("default"))) size_t sim_csv_read_split_block_bytes(size_t C, size_t stride)
{
  return csv_read_split_block_bytes(C, stride);
}
