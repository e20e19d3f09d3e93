// sim_aggregate.cpp -- runs the shipped aggregate kernel source (data-compressor_amd/csrc/aggregate_kernels.hpp) under the
// thread-per-lane emulator of hipsim.hpp.  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built by tests/test_aggregate_host.py
// (its own g++ step; tests/sim/Makefile builds the coder kernels' emulator and stays as it is).
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "hipsim.hpp"

#include "../../data-compressor_amd/csrc/aggregate_kernels.hpp"

using namespace dg;

// wide != 0: the 16-byte form (four channels per lane; C and ld multiples of 4, as the library requires of it).
// row_ranges: how many ranges of output rows the grid's y dimension has (the library picks it by batch size).
extern "C" __attribute__((visibility("default"))) int sim_aggregate(const float *v, size_t C, size_t T, size_t ld, size_t N, float *a, size_t ld_out,
                                                                    int wide, size_t row_ranges)
{
  if (N == 0 || C == 0 || T == 0 || ld < C || ld_out < C || row_ranges == 0 || (wide && (C % 4 != 0 || ld % 4 != 0)))
    return -1;
  AggregateArgs g;
  g.v = v;
  g.a = a;
  g.C = C;
  g.T = T;
  g.ld = ld;
  g.N = N;
  g.T_out = T / N + (T % N != 0 ? 1 : 0);
  g.ld_out = ld_out;
  if (row_ranges > g.T_out)
    row_ranges = g.T_out;
  g.rows_per_block = (g.T_out + row_ranges - 1) / row_ranges;
  g.wide_out = 0;
  const size_t units = wide ? C / 4 : C;
  const dim3 grid((unsigned)((units + AGG_BLOCK - 1) / AGG_BLOCK), (unsigned)((g.T_out + g.rows_per_block - 1) / g.rows_per_block));
  if (wide)
    sim::launch(dega_aggregate_kernel<AggF4>, grid, dim3(AGG_BLOCK), g);
  else
    sim::launch(dega_aggregate_kernel<float>, grid, dim3(AGG_BLOCK), g);
  return 0;
}
