// sim_aggregate_levels.cpp -- runs the shipped multi-level aggregate kernel source
// (data-compressor_amd/csrc/aggregate_levels_kernels.hpp) under the thread-per-lane emulator of hipsim.hpp.
// TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built by the pattern rule of tests/sim/Makefile (libaggregate_levels_sim.so)
// for tests/test_aggregate_levels_host.py.
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "sim_launch.hpp"

#include "../../data-compressor_amd/csrc/aggregate_levels_kernels.hpp"

using namespace dg;

// wide != 0: the 16-byte form (C and ld multiples of 4).  step: base rows per range of the grid's y dimension; the caller
// passes a multiple of every N[l], or a value >= T (what the library's planner guarantees), anything else is refused.
extern "C" __attribute__((visibility("default"))) int sim_aggregate_levels(const float *v, size_t C, size_t T, size_t ld, const size_t *N, size_t K,
                                                                           float *const *a, const size_t *ld_out, int wide, size_t step)
{
  if (K < 2 || K > AGG_MAX_LEVELS || C == 0 || T == 0 || T > 0xFFFFFFFFu || ld < C || step == 0 || (wide && (C % 4 != 0 || ld % 4 != 0)))
    return -1;
  for (size_t l = 0; l < K; l++)
    if (N[l] == 0 || ld_out[l] < C || (step < T && step % N[l] != 0))
      return -1;
  return launch(AggregateVariant{wide != 0, (uint32_t)K}, AggregatePass{v, C, T, ld, step, N, a, ld_out}, OnEmulator{}) ? 0 : -1;
}
