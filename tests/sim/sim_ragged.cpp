// sim_ragged.cpp -- runs the shipped counted kernels (ragged batches: a count per channel) under the thread-per-lane
// emulator of hipsim.hpp: dega_aggregate_var_kernel (aggregate_var_kernels.hpp), the VAR form of dega_csv_kernel
// (csv_kernels.hpp) and the VAR instantiations of dega_encode_kernel (dega_kernels.hpp) that the library dispatches to.
// TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built by tests/test_ragged_host.py (its own g++ step, as sim_aggregate.cpp
// has; tests/sim/Makefile stays as it is).
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "hipsim.hpp"

#include "../../data-compressor_amd/csrc/dega_kernels.hpp"
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

template <uint32_t K>
static void run_aggregate(const float *v, size_t C, size_t T, size_t ld, const uint64_t *count, const size_t *N, float *const *a, const size_t *ld_out,
                          uint64_t *const *out_count, int32_t *err, int wide, size_t step)
{
  AggregateVarArgs<K> g;
  g.v = v;
  g.C = C;
  g.T = T;
  g.ld = ld;
  g.step = step;
  g.count = count;
  g.err = err;
  const size_t top = T > 0 ? T : 1;
  for (uint32_t l = 0; l < K; l++)
  {
    g.a[l] = a[l];
    g.ld_out[l] = ld_out[l];
    g.N[l] = (uint32_t)(N[l] < top ? N[l] : top); // as the library's launcher
    g.wide_out[l] = 0;
    g.out_count[l] = out_count[l];
  }
  const size_t units = wide ? C / 4 : C, ranges = (T + step - 1) / step;
  const dim3 grid((unsigned)((units + AGG_BLOCK - 1) / AGG_BLOCK), (unsigned)(ranges > 0 ? ranges : 1));
  if (wide)
    sim::launch(dega_aggregate_var_kernel<AggF4, K>, grid, dim3(AGG_BLOCK), g);
  else
    sim::launch(dega_aggregate_var_kernel<float, K>, grid, dim3(AGG_BLOCK), g);
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
  switch (K)
  {
    case 1: run_aggregate<1>(v, C, T, ld, count, N, a, ld_out, out_count, err, wide, step); break;
    case 2: run_aggregate<2>(v, C, T, ld, count, N, a, ld_out, out_count, err, wide, step); break;
    case 3: run_aggregate<3>(v, C, T, ld, count, N, a, ld_out, out_count, err, wide, step); break;
    case 4: run_aggregate<4>(v, C, T, ld, count, N, a, ld_out, out_count, err, wide, step); break;
    case 5: run_aggregate<5>(v, C, T, ld, count, N, a, ld_out, out_count, err, wide, step); break;
    case 6: run_aggregate<6>(v, C, T, ld, count, N, a, ld_out, out_count, err, wide, step); break;
    case 7: run_aggregate<7>(v, C, T, ld, count, N, a, ld_out, out_count, err, wide, step); break;
    default: run_aggregate<8>(v, C, T, ld, count, N, a, ld_out, out_count, err, wide, step); break;
  }
  return 0;
}

// wide != 0: the LDS-staged 64-byte store form, else the 8-byte form.  The checks are the library's.
extern "C" __attribute__((visibility("default"))) int sim_csv_var(const float *v, size_t C, size_t T, size_t ld, const uint64_t *count, unsigned decimals,
                                                                  size_t column, int sep, uint8_t *out, size_t stride, uint64_t *out_len, int32_t *err, int wide)
{
  if (C == 0 || T > 0xFFFFFFFFu || ld < C || decimals > CSV_MAX_DECIMALS || column == 0 || sep < 0 || sep > 255 || stride < 16 || stride % 16 != 0 ||
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
  a.count = count;
  const dim3 grid((unsigned)((C + CSV_BLOCK - 1) / CSV_BLOCK));
  if (wide)
    sim::launch(dega_csv_kernel<CsvStore64, true>, grid, dim3(CSV_BLOCK), a);
  else
    sim::launch(dega_csv_kernel<CsvStore8, true>, grid, dim3(CSV_BLOCK), a);
  return 0;
}

static std::vector<uint32_t> make_table()
{
  std::vector<uint32_t> tab(DIV_TABLE_SIZE + 32, 0u); // + the look-ahead of BacEncoder::fetch_magics
  for (uint32_t t = 3; t < DIV_TABLE_SIZE; t++)
  {
    uint32_t L = 0;
    while ((1u << L) < t)
      L++;
    const unsigned __int128 num = (unsigned __int128)1 << (30 + L);
    tab[t] = (uint32_t)((num + t - 1) / t);
  }
  return tab;
}

// the float entry of the encoder over a ragged batch: the six instantiations the library's launcher chooses between
extern "C" __attribute__((visibility("default"))) int sim_encode_f32_var(const float *v, size_t C, size_t T, size_t ld, const uint64_t *count, float factor,
                                                                         int adaptive, int valuesize, uint8_t *out, size_t cap, uint64_t *bits, int32_t *err)
{
  static const std::vector<uint32_t> tab = make_table();
  if (C == 0 || ld < C || valuesize < 1 || valuesize > 64 || cap % 4 != 0)
    return -1;
  EncodeArgs a{reinterpret_cast<const int32_t *>(v), C, T, ld, out, cap, bits, err, tab.data(), (uint32_t)valuesize};
  a.big_endian = 0;
  a.factor = factor;
  a.lo = -(float)((uint64_t)1 << (valuesize - 1)); // as the library's launcher
  a.hi = (float)(((uint64_t)1 << (valuesize - 1)) - 1);
  a.seg_state = nullptr;
  a.seg_flags = 0;
  a.count = count;
  const dim3 grid((unsigned)((C + ENC_CHANNELS - 1) / ENC_CHANNELS));
  const int sel = valuesize > 32 ? (adaptive ? 5 : 4) : (adaptive ? 2 : 0) | (valuesize < 32 ? 1 : 0);
  switch (sel)
  {
    case 0: sim::launch(dega_encode_kernel<false, false, ENC_ROWS, ENC_RING, ENC_RAW, ENC_ORING, false, true, ENC_PAIRS, DIV_TABLE_SIZE, true>, grid, dim3(ENC_BLOCK), a); break;
    case 1: sim::launch(dega_encode_kernel<false, true, ENC_ROWS, ENC_RING, ENC_RAW, ENC_ORING, false, true, ENC_PAIRS, DIV_TABLE_SIZE, true>, grid, dim3(ENC_BLOCK), a); break;
    case 2: sim::launch(dega_encode_kernel<true, false, ENC_ROWS, ENC_RING, ENC_RAW, ENC_ORING, false, true, ENC_PAIRS, DIV_TABLE_SIZE, true>, grid, dim3(ENC_BLOCK), a); break;
    case 3: sim::launch(dega_encode_kernel<true, true, ENC_ROWS, ENC_RING, ENC_RAW, ENC_ORING, false, true, ENC_PAIRS, DIV_TABLE_SIZE, true>, grid, dim3(ENC_BLOCK), a); break;
    case 4: sim::launch(dega_encode_kernel<false, false, 4, 32, 16, 32, true, true, ENC_PAIRS, DIV_TABLE_SIZE, true>, grid, dim3(ENC_BLOCK), a); break;
    default: sim::launch(dega_encode_kernel<true, false, 4, 32, 16, 32, true, true, ENC_PAIRS, DIV_TABLE_SIZE, true>, grid, dim3(ENC_BLOCK), a); break;
  }
  return 0;
}
