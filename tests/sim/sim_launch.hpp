// sim_launch.hpp -- the emulator's backend of the launch descriptions at the foot of the kernel headers
// (data-compressor_amd/csrc/dega_launch.hpp): the drivers of this directory take the variant from the library's chooser
// (overriding the one field a test forces), the arguments from the library's fill, and hand both to the library's launch()
// with OnEmulator in place of the library's stream.  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.
#pragma once

#include "hipsim.hpp"

#include "../../data-compressor_amd/csrc/dega_kernels.hpp"

#include <vector>

namespace dg
{

struct OnEmulator
{
  template <typename A>
  void operator()(void (*kernel)(A), LaunchGrid grid, uint32_t block, const A &a) const
  {
    sim::launch(kernel, dim3(grid.x, grid.y), dim3(block), a);
  }
};

// The library's division magics with 32 zero words of slack behind them: sim_fast_vs_slow hands the table straight to
// BacCoder::fetch_magics_first, which reads up to a word's worth of entries ahead of the one it needs (the kernels copy
// the table into LDS, where the rings lie behind it).
inline const uint32_t *sim_div_table()
{
  static const std::vector<uint32_t> tab = [] {
    std::vector<uint32_t> t;
    build_div_table(t, 32);
    return t;
  }();
  return tab.data();
}

} // namespace dg
