// sim_transpose.cpp -- runs the shipped dega_transpose_kernel (transpose_kernels.hpp) under the thread-per-lane emulator of
// hipsim.hpp.  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built by tests/test_channel_major_host.py (its own g++ step, as
// sim_ragged.cpp has; tests/sim/Makefile stays as it is).
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "hipsim.hpp"

#include "../../data-compressor_amd/csrc/transpose_kernels.hpp"

using namespace dg;

template <typename E>
static void run(const TransposeArgs &a, dim3 grid, int wide_ld, int wide_st)
{
  constexpr uint32_t V = 16 / sizeof(E);
  if (wide_ld && wide_st)
    sim::launch(dega_transpose_kernel<E, V, V>, grid, dim3(TR_BLOCK), a);
  else if (wide_ld)
    sim::launch(dega_transpose_kernel<E, V, 1>, grid, dim3(TR_BLOCK), a);
  else if (wide_st)
    sim::launch(dega_transpose_kernel<E, 1, V>, grid, dim3(TR_BLOCK), a);
  else
    sim::launch(dega_transpose_kernel<E, 1, 1>, grid, dim3(TR_BLOCK), a);
}

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
  TransposeArgs a;
  a.src = src;
  a.dst = dst;
  a.R = R;
  a.K = K;
  a.sp = sp;
  a.dp = dp;
  a.count = count;
  a.count_on_rows = count_on_rows ? 1u : 0u;
  uint32_t gx, gy;
  if (!tr_plan(R, K, gx_max, a, gx, gy))
    return -1;
  if (elem_bytes == 4)
    run<uint32_t>(a, dim3(gx, gy), wide_ld, wide_st);
  else
    run<uint64_t>(a, dim3(gx, gy), wide_ld, wide_st);
  return 0;
}
