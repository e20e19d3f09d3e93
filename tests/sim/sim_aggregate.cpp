// sim_aggregate.cpp -- runs the shipped aggregate kernel source (data-compressor_amd/csrc/aggregate_kernels.hpp) under the
// thread-per-lane emulator of hipsim.hpp.  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built by the pattern rule of
// tests/sim/Makefile (libaggregate_sim.so) for tests/test_aggregate_host.py.
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "sim_launch.hpp"

#include "../../data-compressor_amd/csrc/aggregate_kernels.hpp"

using namespace dg;

// wide != 0: the 16-byte form (four channels per lane; C and ld multiples of 4, as the library requires of it).
// row_ranges: how many ranges of output rows the grid's y dimension has (the library picks it by batch size).
extern "C" __attribute__((visibility("default"))) int sim_aggregate(const float *v, size_t C, size_t T, size_t ld, size_t N, float *a, size_t ld_out,
                                                                    int wide, size_t row_ranges)
{
  if (N == 0 || C == 0 || T == 0 || ld < C || ld_out < C || row_ranges == 0 || (wide && (C % 4 != 0 || ld % 4 != 0)))
    return -1;
  return launch(AggregateVariant{wide != 0, 1}, aggregate_args(v, C, T, ld, N, a, ld_out, wide != 0, row_ranges), OnEmulator{}) ? 0 : -1;
}
