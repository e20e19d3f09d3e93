// sim_aggregate_levels.cpp -- runs the shipped multi-level aggregate kernel source
// (data-compressor_amd/csrc/aggregate_levels_kernels.hpp) under the thread-per-lane emulator of hipsim.hpp.
// TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built by tests/test_aggregate_levels_host.py (its own g++ step, as
// sim_aggregate.cpp has; tests/sim/Makefile stays as it is).
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "hipsim.hpp"

#include "../../data-compressor_amd/csrc/aggregate_levels_kernels.hpp"

using namespace dg;

template <uint32_t K>
static void run(const float *v, size_t C, size_t T, size_t ld, const size_t *N, float *const *a, const size_t *ld_out, int wide, size_t step)
{
  AggregateLevelsArgs<K> g;
  g.v = v;
  g.C = C;
  g.T = T;
  g.ld = ld;
  g.step = step;
  for (uint32_t l = 0; l < K; l++)
  {
    g.a[l] = a[l];
    g.ld_out[l] = ld_out[l];
    g.N[l] = (uint32_t)(N[l] < T ? N[l] : T); // as the library's launcher
    g.wide_out[l] = 0;
  }
  const size_t units = wide ? C / 4 : C;
  const dim3 grid((unsigned)((units + AGG_BLOCK - 1) / AGG_BLOCK), (unsigned)((T + step - 1) / step));
  if (wide)
    sim::launch(dega_aggregate_levels_kernel<AggF4, K>, grid, dim3(AGG_BLOCK), g);
  else
    sim::launch(dega_aggregate_levels_kernel<float, K>, grid, dim3(AGG_BLOCK), g);
}

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
  switch (K)
  {
    case 2: run<2>(v, C, T, ld, N, a, ld_out, wide, step); break;
    case 3: run<3>(v, C, T, ld, N, a, ld_out, wide, step); break;
    case 4: run<4>(v, C, T, ld, N, a, ld_out, wide, step); break;
    case 5: run<5>(v, C, T, ld, N, a, ld_out, wide, step); break;
    case 6: run<6>(v, C, T, ld, N, a, ld_out, wide, step); break;
    case 7: run<7>(v, C, T, ld, N, a, ld_out, wide, step); break;
    default: run<8>(v, C, T, ld, N, a, ld_out, wide, step); break;
  }
  return 0;
}
