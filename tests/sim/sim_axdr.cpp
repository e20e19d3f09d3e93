// sim_axdr.cpp -- runs the shipped dega_axdr_pack_kernel / dega_axdr_unpack_kernel (axdr_kernels.hpp) under the thread-per-lane
// emulator of hipsim.hpp.  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built by the pattern rule of tests/sim/Makefile
// (libaxdr_sim.so) for tests/test_axdr_host.py, and included by sim_axdr_main.cpp, the stand-alone program under the host
// sanitizers.
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "sim_launch.hpp"

#include "../../data-compressor_amd/csrc/axdr_kernels.hpp"

#include <string.h>

using namespace dg;

// kind: 0 float32, 1 int32, 2 int64 rows.  wide: -1 the library's choice of the 16-byte form on the rows' side, 0 / 1 forced
// (1 is refused where the library would not choose it).  gx_max: workgroups along x before the tile index continues in y.
static bool sim_axdr_variant(int kind, int valuesize, const void *x_tc, size_t ld, int wide, AxdrVariant &v)
{
  if (kind < 0 || kind > 2)
    return false;
  v = axdr_variant((uint32_t)kind, valuesize, x_tc, ld);
  if (wide == 1 && !v.wide)
    return false;
  if (wide == 0)
    v.wide = false;
  return axdr_goes_together(v, (uint32_t)valuesize);
}

extern "C" __attribute__((visibility("default"))) int sim_axdr_rows(int wide64)
{
  return (int)ax_rows(wide64 != 0);
}

// As dega_hip_axdr_encode_dev launches it: err zeroed, then the pack kernel.
extern "C" __attribute__((visibility("default"))) int sim_axdr_pack(const void *x_tc, int kind, size_t C, size_t T, size_t ld, const uint64_t *count, float factor,
                                                                    int valuesize, uint8_t *out, size_t cap, uint64_t *out_bits, int32_t *err, int wide,
                                                                    size_t gx_max)
{
  AxdrVariant v;
  if (ld < C || cap % 4 != 0 || gx_max == 0 || C == 0 || valuesize < 1 || valuesize > 64 || !sim_axdr_variant(kind, valuesize, x_tc, ld, wide, v))
    return -1;
  memset(err, 0, C * sizeof(int32_t));
  return launch(v, axdr_pack_args(x_tc, C, T, ld, count, factor, valuesize, out, cap, out_bits, err), gx_max, OnEmulator{}) ? 0 : -1;
}

extern "C" __attribute__((visibility("default"))) int sim_axdr_unpack(const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld,
                                                                      float factor, int valuesize, int kind, void *x_tc, uint64_t *out_count, int32_t *err,
                                                                      int wide, size_t gx_max)
{
  AxdrVariant v;
  if (ld < C || cap % 4 != 0 || gx_max == 0 || C == 0 || valuesize < 1 || valuesize > 64 || !sim_axdr_variant(kind, valuesize, x_tc, ld, wide, v))
    return -1;
  return launch(v, axdr_unpack_args(in, cap, in_bits, C, max_T, ld, factor, valuesize, x_tc, out_count, err), gx_max, OnEmulator{}) ? 0 : -1;
}
