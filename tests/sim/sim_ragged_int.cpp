// sim_ragged_int.cpp -- runs the counted integer instantiations of dega_encode_kernel (dega_kernels.hpp: int32 at
// valuesize 32, the narrow value sizes, byte-swapped words, int64 containers), whole channels in one launch and over
// several launches with a segment state, under the thread-per-lane emulator of hipsim.hpp.  Variant, arguments and grid
// come from the launch table the library dispatches from.  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built by the pattern
// rule of tests/sim/Makefile (libragged_int_sim.so) for tests/test_ragged_int_host.py.
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "sim_launch.hpp"

#include <vector>

using namespace dg;

// a slow coding wave (waves from_wave .. of a workgroup sleep at every peer_load): the rings between the waves run full
extern "C" __attribute__((visibility("default"))) void sim_ragged_int_set_drag(int from_wave, int microseconds)
{
  sim::g_drag_from = from_wave;
  sim::g_drag_us = microseconds;
}

// the library's refusals that bear on memory safety here: the shape, and the pairing of container and value size
static bool shape_ok(size_t C, size_t T, size_t ld, int valuesize, int wide, size_t cap)
{
  return C != 0 && ld >= C && T <= ((size_t)1 << 25) && cap % 4 == 0 && (wide ? valuesize >= 33 && valuesize <= 64 : valuesize >= 1 && valuesize <= 32);
}

// x: int32 [T][ld] (big_endian != 0: byte-swapped words), or with wide != 0 int64 [T][ld]
extern "C" __attribute__((visibility("default"))) int sim_encode_int_var(const void *x, size_t C, size_t T, size_t ld, const uint64_t *count, int wide,
                                                                         int big_endian, int adaptive, int valuesize, uint8_t *out, size_t cap, uint64_t *bits,
                                                                         int32_t *err)
{
  if (!shape_ok(C, T, ld, valuesize, wide, cap) || count == nullptr || (wide && big_endian))
    return -1;
  const EncodeArgs a = encode_args(x, C, T, ld, out, cap, bits, err, sim_div_table(), valuesize, big_endian != 0, 0.0f, nullptr, 0, count);
  return launch(encode_variant(C, T, false, true, valuesize, false, adaptive != 0), a, OnEmulator{}) ? 0 : -1;
}

// the same channels over several launches: rows [cuts[k], cuts[k + 1]) each, row0 = cuts[k], T_total = T, the lanes' state
// saved in between (it starts as garbage: the first launch restores nothing)
extern "C" __attribute__((visibility("default"))) int sim_encode_int_var_segments(const void *x, size_t C, size_t T, size_t ld, const uint64_t *count, int wide,
                                                                                  int big_endian, int adaptive, int valuesize, const size_t *cuts, int ncuts,
                                                                                  uint8_t *out, size_t cap, uint64_t *bits, int32_t *err)
{
  if (!shape_ok(C, T, ld, valuesize, wide, cap) || count == nullptr || (wide && big_endian) || ncuts < 2 || cuts[0] != 0 || cuts[ncuts - 1] != T)
    return -1;
  for (int k = 0; k + 1 < ncuts; k++)
    if (cuts[k] > cuts[k + 1])
      return -1;
  std::vector<uint32_t> state(ENC_STATE_WORDS * C, 0xDEADBEEFu);
  const size_t row_bytes = ld * (wide ? sizeof(int64_t) : sizeof(int32_t));
  for (int k = 0; k + 1 < ncuts; k++)
  {
    const size_t T_seg = cuts[k + 1] - cuts[k];
    // (an empty segment behind the last row: the pointer stays inside the array)
    const uint8_t *const rows = static_cast<const uint8_t *>(x) + (T_seg != 0 ? cuts[k] : 0) * row_bytes;
    const uint32_t flags = (k > 0 ? ENC_SEG_CONTINUES : 0u) | (k + 2 < ncuts ? ENC_SEG_MORE : 0u);
    const EncodeArgs a = encode_args(rows, C, T_seg, ld, out, cap, bits, err, sim_div_table(), valuesize, big_endian != 0, 0.0f, state.data(), flags, count, cuts[k], T);
    if (!launch(encode_variant(C, T_seg, true, true, valuesize, false, adaptive != 0), a, OnEmulator{}))
      return -1;
  }
  return 0;
}
