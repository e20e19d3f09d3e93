// dega_launch.hpp -- what the launch descriptions at the foot of the kernel headers share.
//
// Every kernel header ends with host-only code that says how its kernels are launched: a plain struct of the run-time facts
// that pick an instantiation (the variant), a pure function that computes it from what the caller has (the chooser), one
// function that produces the kernel's argument struct (the fill), and launch(variant, args, L), which maps the variant to
// the instantiation, computes grid and block and calls L(kernel, grid, block, args) once.  L is the backend: the library
// passes hipLaunchKernelGGL on the call's stream (dega_hip.hip), the emulator sim::launch (tests/sim/sim_launch.hpp), so
// both run the same selection, fill and grid code.  A launch that cannot be made (no such instantiation, a grid beyond the
// limits) is reported by `false`, as tr_plan does; nothing has been launched then.
//
// Plain C++17, no HIP runtime: compiled by hipcc (dega_hip.hip) and by g++ (tests/sim/).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <type_traits>

namespace dg
{

struct LaunchGrid
{
  uint32_t x, y;
};

constexpr size_t LAUNCH_MAX_GX = 0x7FFFFFFFu; // workgroups along x of the launches that check it

// f(std::bool_constant<b0>(), std::bool_constant<b1>(), ...) for the run-time bools b0, b1, ... behind f
template <bool... Bs, typename F>
inline void with_bools(F &&f)
{
  f(std::integral_constant<bool, Bs>()...);
}

template <bool... Bs, typename F, typename... Rest>
inline void with_bools(F &&f, bool b, Rest... rest)
{
  if (b)
    with_bools<Bs..., true>(f, rest...);
  else
    with_bools<Bs..., false>(f, rest...);
}

} // namespace dg
