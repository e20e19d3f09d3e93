// sim_csv.cpp -- runs the shipped `encode csv` kernel source (data-compressor_amd/csrc/csv_kernels.hpp) under the
// thread-per-lane emulator of hipsim.hpp.  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built by tests/test_csv_host.py (its
// own g++ step, as sim_aggregate.cpp has; tests/sim/Makefile stays as it is).
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "hipsim.hpp"

#include "../../data-compressor_amd/csrc/csv_kernels.hpp"

using namespace dg;

// wide != 0: the LDS-staged 64-byte store form, else the 8-byte form.  The checks are the library's.
extern "C" __attribute__((visibility("default"))) int sim_csv(const float *v, size_t C, size_t T, size_t ld, unsigned decimals, size_t column, int sep,
                                                              uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err, int wide)
{
  if (C == 0 || T == 0 || ld < C || decimals > CSV_MAX_DECIMALS || column == 0 || sep < 0 || sep > 255 || stride < 16 || stride % 16 != 0 ||
      stride > 0x7FFFFFF0u || column - 1 >= stride || ((uintptr_t)out & 15u) != 0)
    return -1;
  CsvArgs a;
  a.v = v;
  a.C = C;
  a.T = T;
  a.ld = ld;
  a.decimals = decimals;
  a.nsep = (uint32_t)(column - 1);
  a.sep = (uint32_t)sep;
  a.out = out;
  a.stride = stride;
  a.out_len = out_len;
  a.err = err;
  const dim3 grid((unsigned)((C + CSV_BLOCK - 1) / CSV_BLOCK));
  if (wide)
    sim::launch(dega_csv_kernel<CsvStore64>, grid, dim3(CSV_BLOCK), a);
  else
    sim::launch(dega_csv_kernel<CsvStore8>, grid, dim3(CSV_BLOCK), a);
  return 0;
}
