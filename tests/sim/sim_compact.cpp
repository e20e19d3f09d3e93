// sim_compact.cpp -- runs the shipped stream compaction kernels (dega_gather_kernel and dega_scatter_kernel of
// data-compressor_amd/csrc/dega_kernels.hpp) under the thread-per-lane emulator of hipsim.hpp.  TEST INFRASTRUCTURE ONLY; see
// hipsim.hpp.  Built by the pattern rule of tests/sim/Makefile (libcompact_sim.so) for tests/test_index_width_host.py.
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "sim_launch.hpp"

using namespace dg;

// One wave per channel, as the library launches them: [C][cap] slabs -> packed, or with scatter != 0 the inverse.
extern "C" __attribute__((visibility("default"))) int sim_compact(uint8_t *slabs, size_t cap, const uint64_t *offsets, size_t C, uint8_t *packed, int scatter)
{
  if (C == 0)
    return 0;
  const size_t gx = (C + WAVES - 1) / WAVES;
  if (gx > LAUNCH_MAX_GX)
    return -1;
  const GatherArgs a{slabs, cap, offsets, C, packed};
  OnEmulator{}(scatter != 0 ? dega_scatter_kernel : dega_gather_kernel, LaunchGrid{(uint32_t)gx, 1}, BLOCK, a);
  return 0;
}
