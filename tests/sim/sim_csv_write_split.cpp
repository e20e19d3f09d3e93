// sim_csv_write_split.cpp -- runs the shipped split `encode csv` kernels (data-compressor_amd/csrc/csv_write_split_kernels.hpp)
// under the thread-per-lane emulator of hipsim.hpp, through the header's own launch table.  TEST INFRASTRUCTURE ONLY; see
// hipsim.hpp.  Built by the pattern rule of tests/sim/Makefile (libcsv_write_split_sim.so) for
// tests/test_csv_write_split_host.py, and included by sim_csv_write_split_main.cpp (the stand-alone sanitizer program).
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "sim_launch.hpp"

#include "../../data-compressor_amd/csrc/csv_write_split_kernels.hpp"

#include <vector>

using namespace dg;

// Guards what the kernels rely on (what dega_hip_csv_write_split_dev refuses; the library's own checks are tested on the
// GPU); count may be null, block_rows 0 is the library's choice.  The [C][blocks] array between the launches is exactly as
// large as it may be.  T = 0 is taken with a count only (the library launches nothing for it without one).
extern "C" __attribute__((visibility("default"))) int sim_csv_write_split(const float *v, size_t C, size_t T, size_t ld, const uint64_t *count,
                                                                          unsigned decimals, size_t column, int sep, uint8_t *out, size_t stride,
                                                                          uint64_t *out_len, int32_t *err, size_t block_rows)
{
  if (C == 0 || (T == 0 && count == nullptr) || T > 0xFFFFFFFFu || ld < C || decimals > CSV_MAX_DECIMALS || column == 0 || sep < 0 || sep > 255 ||
      stride < 16 || stride % 16 != 0 || stride > 0x7FFFFFF0u || column - 1 >= stride || ((uintptr_t)out & 15u) != 0)
    return -1;
  if (block_rows == 0)
    block_rows = csv_write_split_block_rows(C, T);
  const size_t blocks = csv_write_split_blocks(T, block_rows);
  if (csv_write_split_grid(C, blocks) == 0)
    return -1;
  std::vector<uint32_t> work(C * blocks);
  const CsvArgs a = csv_args(v, C, T, ld, decimals, column, sep, out, stride, out_len, err, count);
  return launch(csv_write_split_args(a, block_rows, work.data()), OnEmulator{}) ? 0 : -1;
}

extern "C" __attribute__((visibility("default"))) size_t sim_csv_write_split_block_rows(size_t C, size_t T)
{
  return csv_write_split_block_rows(C, T);
}

// the unsplit kernel (8-byte stores) on the same arguments, for the test that one block per channel equals it
extern "C" __attribute__((visibility("default"))) int sim_csv_write_unsplit(const float *v, size_t C, size_t T, size_t ld, const uint64_t *count,
                                                                            unsigned decimals, size_t column, int sep, uint8_t *out, size_t stride,
                                                                            uint64_t *out_len, int32_t *err)
{
  if (C == 0 || T == 0 || ld < C || decimals > CSV_MAX_DECIMALS || column == 0 || sep < 0 || sep > 255 || stride < 16 || stride % 16 != 0 ||
      stride > 0x7FFFFFF0u || column - 1 >= stride || ((uintptr_t)out & 15u) != 0)
    return -1;
  return launch(csv_variant(false, count), csv_args(v, C, T, ld, decimals, column, sep, out, stride, out_len, err, count), OnEmulator{}) ? 0 : -1;
}
