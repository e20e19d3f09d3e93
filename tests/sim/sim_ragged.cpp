// sim_ragged.cpp -- runs the shipped counted kernels (ragged batches: a count per channel) under the thread-per-lane
// emulator of hipsim.hpp: dega_aggregate_var_kernel (aggregate_var_kernels.hpp), the VAR form of dega_csv_kernel
// (csv_kernels.hpp) and the VAR instantiations of dega_encode_kernel (dega_kernels.hpp) that the library dispatches to.
// TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built by the pattern rule of tests/sim/Makefile (libragged_sim.so) for
// tests/test_ragged_host.py.
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "sim_launch.hpp"

#include "../../data-compressor_amd/csrc/aggregate_var_kernels.hpp"
#include "../../data-compressor_amd/csrc/csv_kernels.hpp"

#include <vector>

using namespace dg;

// a slow coding wave (waves from_wave .. of a workgroup sleep at every peer_load): the rings between the waves run full
extern "C" __attribute__((visibility("default"))) void sim_ragged_set_drag(int from_wave, int microseconds)
{
  sim::g_drag_from = from_wave;
  sim::g_drag_us = microseconds;
}

// wide != 0: the 16-byte form (C and ld multiples of 4).  step: base rows per range of the grid's y dimension, a multiple of
// every N[l] or a value >= T (what the library's planner guarantees); anything else is refused.
extern "C" __attribute__((visibility("default"))) int sim_aggregate_var(const float *v, size_t C, size_t T, size_t ld, const uint64_t *count, const size_t *N,
                                                                        size_t K, float *const *a, const size_t *ld_out, uint64_t *const *out_count,
                                                                        int32_t *err, int wide, size_t step)
{
  if (K < 1 || K > AGG_MAX_LEVELS || C == 0 || T > 0xFFFFFFFFu || ld < C || step == 0 || (wide && (C % 4 != 0 || ld % 4 != 0)))
    return -1;
  for (size_t l = 0; l < K; l++)
    if (N[l] == 0 || ld_out[l] < C || (step < T && step % N[l] != 0))
      return -1;
  const AggregatePass pass{v, C, T, ld, step, N, a, ld_out};
  return launch(AggregateVariant{wide != 0, (uint32_t)K}, pass, AggregateCounts{count, out_count, err}, OnEmulator{}) ? 0 : -1;
}

// wide != 0: the LDS-staged 64-byte store form, else the 8-byte form.  The checks are the library's.
extern "C" __attribute__((visibility("default"))) int sim_csv_var(const float *v, size_t C, size_t T, size_t ld, const uint64_t *count, unsigned decimals,
                                                                  size_t column, int sep, uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err, int wide)
{
  if (C == 0 || T > 0xFFFFFFFFu || ld < C || decimals > CSV_MAX_DECIMALS || column == 0 || sep < 0 || sep > 255 || stride < 16 || stride % 16 != 0 ||
      stride > 0x7FFFFFF0u || column - 1 >= stride || ((uintptr_t)out & 15u) != 0)
    return -1;
  return launch(csv_variant(wide != 0, count), csv_args(v, C, T, ld, decimals, column, sep, out, stride, out_len, err, count), OnEmulator{}) ? 0 : -1;
}

// the float entry of the encoder over a ragged batch
extern "C" __attribute__((visibility("default"))) int sim_encode_f32_var(const float *v, size_t C, size_t T, size_t ld, const uint64_t *count, float factor,
                                                                         int adaptive, int valuesize, uint8_t *out, size_t cap, uint64_t *bits, int32_t *err)
{
  if (C == 0 || ld < C || valuesize < 1 || valuesize > 64 || cap % 4 != 0)
    return -1;
  const EncodeArgs a = encode_args(v, C, T, ld, out, cap, bits, err, sim_div_table(), valuesize, false, factor, nullptr, 0, count);
  return launch(encode_variant(C, T, false, true, valuesize, true, adaptive != 0), a, OnEmulator{}) ? 0 : -1;
}
