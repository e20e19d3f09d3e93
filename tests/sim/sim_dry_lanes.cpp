// sim_dry_lanes.cpp -- the emulator's entry points (sim_main.cpp) plus a getter for the coding waves' pass counts, for
// tests/test_kernel_sim_dry_lanes.py: a CPU test can tell which word path the steps of a launch took.
// TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built as libdry_lanes_sim.so by the pattern rule of tests/sim/Makefile.
#include "sim_main.cpp"

// the coding waves' passes by kind since the last reset (dega_kernels.hpp, DG_COUNT): steady, steady masked, other word
// paths, waits, steady masked with a dry lane, other word paths that a dry lane alone kept off the steady ones
extern "C" __attribute__((visibility("default"))) void sim_encode_step_counts(uint64_t *counts6, int reset)
{
  for (int k = 0; k < 6; k++)
  {
    if (counts6 != nullptr)
      counts6[k] = __atomic_load_n(&sim_enc_steps[k], __ATOMIC_RELAXED);
    if (reset)
      __atomic_store_n(&sim_enc_steps[k], 0, __ATOMIC_RELAXED);
  }
}
