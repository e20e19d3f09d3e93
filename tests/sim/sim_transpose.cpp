// sim_transpose.cpp -- runs the shipped dega_transpose_kernel (transpose_kernels.hpp) under the thread-per-lane emulator of
// hipsim.hpp.  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built by the pattern rule of tests/sim/Makefile (libtranspose_sim.so) for
// tests/test_channel_major_host.py.
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "sim_launch.hpp"

#include "../../data-compressor_amd/csrc/transpose_kernels.hpp"

using namespace dg;

// S[R][sp] -> D[K][dp] as the library launches it: to time-major R = C, K = T, count_on_rows = 1; to channel-major R = T,
// K = C, count_on_rows = 0.  wide_ld / wide_st: the 16-byte form on that side; the checks are the library's (base and pitch),
// anything else is refused.  gx_max: workgroups along x before the tile index continues in y.
extern "C" __attribute__((visibility("default"))) int sim_transpose(const void *src, size_t R, size_t K, size_t sp, size_t elem_bytes, const uint64_t *count,
                                                                    int count_on_rows, void *dst, size_t dp, int wide_ld, int wide_st, size_t gx_max)
{
  if ((elem_bytes != 4 && elem_bytes != 8) || sp < K || dp < R || gx_max == 0 || R == 0 || K == 0)
    return -1;
  const size_t V = 16 / elem_bytes;
  if (wide_ld && (((uintptr_t)src & 15u) != 0 || sp % V != 0))
    return -1;
  if (wide_st && (((uintptr_t)dst & 15u) != 0 || dp % V != 0))
    return -1;
  TransposeVariant tv = transpose_variant(src, sp, dst, dp, elem_bytes);
  tv.wide_ld = wide_ld != 0;
  tv.wide_st = wide_st != 0;
  return launch(tv, transpose_args(src, R, K, sp, count, count_on_rows != 0, dst, dp), gx_max, OnEmulator{}) ? 0 : -1;
}
