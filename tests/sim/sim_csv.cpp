// sim_csv.cpp -- runs the shipped `encode csv` kernel source (data-compressor_amd/csrc/csv_kernels.hpp) under the
// thread-per-lane emulator of hipsim.hpp.  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built by the pattern rule of
// tests/sim/Makefile (libcsv_sim.so) for tests/test_csv_host.py.
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "sim_launch.hpp"

#include "../../data-compressor_amd/csrc/csv_kernels.hpp"

using namespace dg;

// wide != 0: the LDS-staged 64-byte store form, else the 8-byte form.  The checks are the library's.
extern "C" __attribute__((visibility("default"))) int sim_csv(const float *v, size_t C, size_t T, size_t ld, unsigned decimals, size_t column, int sep,
                                                              uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err, int wide)
{
  if (C == 0 || T == 0 || ld < C || decimals > CSV_MAX_DECIMALS || column == 0 || sep < 0 || sep > 255 || stride < 16 || stride % 16 != 0 ||
      stride > 0x7FFFFFF0u || column - 1 >= stride || ((uintptr_t)out & 15u) != 0)
    return -1;
  return launch(csv_variant(wide != 0, nullptr), csv_args(v, C, T, ld, decimals, column, sep, out, stride, out_len, err, nullptr), OnEmulator{}) ? 0 : -1;
}
