// aggregate_levels_kernels.hpp -- several granularities of the `aggregate` stage (DCLib/src/aggregate.c:9-26) from ONE pass
// over the base series, for gfx950 (MI355X).
//
// The granularity study codes the same readings at several resolutions.  dega_aggregate_kernel reads all T rows per
// level, and its time is that read; here a lane walks its rows once and keeps K independent accumulators, each of which
// takes every row.  A coarser level is never formed from a finer level's sums: sums of sums round differently (58 - 86 %
// of the outputs of the fixture series differ), and what has to match the reference is the rounding.  So per level
// exactly what aggregate_kernels.hpp does: the sum starts at +0.0f, one rounding per add, rows from left to right, the
// short last group written as it stands; no cross-lane operation, no atomic, nothing combined afterwards.
//
// Same load shape as dega_aggregate_kernel (AggLane, AGG_BLOCK, AGG_DEPTH are its): lanes are adjacent channels, four per
// lane in the 16-byte form, AGG_DEPTH independent row loads before the first dependent add.  Per row K adds (4 K in the
// 16-byte form) and K wave-uniform counter steps; a level whose counter reaches its N stores to its own array.
// blockIdx.y takes a range of `step` BASE rows, and the host makes `step` a multiple of every level's N in the launch
// (or one range of all T rows): every range begins on a group boundary of every level.
//
// K is a template parameter so that the accumulators and counters stay in registers (no scratch memory in any
// instantiation: DESIGN.md 4.5 has the figures).  Counters are 32-bit: the host clamps N to T and takes T < 2^32.
//
// Compiled by hipcc (dega_hip.hip) and, for offline checking only, by g++ under tests/sim/.
#pragma once

#include "aggregate_kernels.hpp"

namespace dg
{

constexpr uint32_t AGG_MAX_LEVELS = 8; // DEGA_AGG_MAX_LEVELS of include/dega_hip.h

template <uint32_t K>
struct AggregateLevelsArgs
{
  const float *v; // [T][ld]
  size_t C, T, ld;
  size_t step;        // base rows per blockIdx.y: a multiple of every N[l], or >= T
  float *a[K];        // level l: [ceil(T / N[l])][ld_out[l]]
  size_t ld_out[K];
  uint32_t N[K];      // 1 .. T
  uint32_t wide_out[K]; // 16-byte form: level l's array and pitch allow 16-byte stores
};

// V as in dega_aggregate_kernel: float for any ld and alignment, AggF4 where the host has checked the 16-byte conditions.
template <typename V, uint32_t K>
__global__ void __launch_bounds__(256) dega_aggregate_levels_kernel(const AggregateLevelsArgs<K> a)
{
  static_assert(K >= 2 && K <= AGG_MAX_LEVELS, "one level is dega_aggregate_kernel");
  typedef AggLane<V> L;
  const size_t c = ((size_t)blockIdx.x * AGG_BLOCK + threadIdx.x) * L::WIDTH;
  if (c >= a.C)
    return;
  const size_t t0 = (size_t)blockIdx.y * a.step;
  if (t0 >= a.T)
    return;
  const size_t t1 = a.step < a.T - t0 ? t0 + a.step : a.T;
  const float *src = a.v + t0 * a.ld + c;
  float *dst[K];
  V sum[K];
  uint32_t k[K]; // rows of level l's open group already added (wave-uniform)
#pragma unroll
  for (uint32_t l = 0; l < K; l++)
  {
    dst[l] = a.a[l] + (t0 / a.N[l]) * a.ld_out[l] + c; // t0 is a multiple of N[l]: the range opens a group of every level
    sum[l] = L::zero();
    k[l] = 0;
  }
  size_t t = t0;
  for (; t + AGG_DEPTH <= t1; t += AGG_DEPTH)
  {
    V row[AGG_DEPTH];
#pragma unroll
    for (uint32_t u = 0; u < AGG_DEPTH; u++) // loads first ...
      row[u] = L::load(src + (size_t)u * a.ld);
    src += (size_t)AGG_DEPTH * a.ld;
#pragma unroll
    for (uint32_t u = 0; u < AGG_DEPTH; u++) // ... the adds, in row order, after: every level takes every row
    {
#pragma unroll
      for (uint32_t l = 0; l < K; l++)
      {
        L::add(sum[l], row[u]);
        if (++k[l] == a.N[l])
        {
          L::store(dst[l], sum[l], a.wide_out[l]);
          dst[l] += a.ld_out[l];
          sum[l] = L::zero();
          k[l] = 0;
        }
      }
    }
  }
  for (; t < t1; t++) // fewer than AGG_DEPTH rows left in the range
  {
    const V r = L::load(src);
    src += a.ld;
#pragma unroll
    for (uint32_t l = 0; l < K; l++)
    {
      L::add(sum[l], r);
      if (++k[l] == a.N[l])
      {
        L::store(dst[l], sum[l], a.wide_out[l]);
        dst[l] += a.ld_out[l];
        sum[l] = L::zero();
        k[l] = 0;
      }
    }
  }
#pragma unroll
  for (uint32_t l = 0; l < K; l++)
    if (k[l] != 0) // only where the series ends inside a group of level l: aggregate.c:21-22 writes what it has
      L::store(dst[l], sum[l], a.wide_out[l]);
}

// ---- host side: how the kernel is launched (dega_launch.hpp) ----------------------------------------------------------------

// f(std::integral_constant<uint32_t, n>()) for the n = 1 .. AGG_MAX_LEVELS levels of a pass
template <typename F>
inline void for_levels_of_pass(uint32_t n, F &&f)
{
  switch (n)
  {
    case 1: f(std::integral_constant<uint32_t, 1>()); break;
    case 2: f(std::integral_constant<uint32_t, 2>()); break;
    case 3: f(std::integral_constant<uint32_t, 3>()); break;
    case 4: f(std::integral_constant<uint32_t, 4>()); break;
    case 5: f(std::integral_constant<uint32_t, 5>()); break;
    case 6: f(std::integral_constant<uint32_t, 6>()); break;
    case 7: f(std::integral_constant<uint32_t, 7>()); break;
    default: f(std::integral_constant<uint32_t, 8>()); break;
  }
}

// One pass over the image: the levels it sums (as many as the variant says) and the base rows per range of the grid's y
// dimension, a multiple of every N[l] or a value >= T.
struct AggregatePass
{
  const float *v;
  size_t C, T, ld, step;
  const size_t *N;
  float *const *a;
  const size_t *ld_out;
};

// what AggregateLevelsArgs<n> and AggregateVarArgs<n> share: the image and the n levels of the pass
template <typename Args>
inline void fill_pass(Args &g, uint32_t n, bool wide, const AggregatePass &p)
{
  g.v = p.v;
  g.C = p.C;
  g.T = p.T;
  g.ld = p.ld;
  g.step = p.step;
  const size_t top = p.T > 1 ? p.T : 1;
  for (uint32_t l = 0; l < n; l++)
  {
    g.a[l] = p.a[l];
    g.ld_out[l] = p.ld_out[l];
    g.N[l] = (uint32_t)(p.N[l] < top ? p.N[l] : top);
    g.wide_out[l] = aggregate_wide_out(wide, p.a[l], p.ld_out[l]) ? 1u : 0u;
  }
}

// two to AGG_MAX_LEVELS levels (one level is dega_aggregate_kernel)
template <typename L>
inline bool launch(const AggregateVariant &v, const AggregatePass &p, L &&launch_one)
{
  const size_t gx = aggregate_gx(p.C, v.wide);
  if (v.levels < 2 || v.levels > AGG_MAX_LEVELS || p.step == 0 || gx > LAUNCH_MAX_GX)
    return false;
  const LaunchGrid grid{(uint32_t)gx, (uint32_t)((p.T + p.step - 1) / p.step)};
  for_levels_of_pass(v.levels, [&](auto levels) {
    constexpr uint32_t NL = decltype(levels)::value;
    if constexpr (NL >= 2)
    {
      AggregateLevelsArgs<NL> g;
      fill_pass(g, NL, v.wide, p);
      with_bools([&](auto wide) { launch_one(dega_aggregate_levels_kernel<std::conditional_t<decltype(wide)::value, AggF4, float>, NL>, grid, AGG_BLOCK, g); },
                 v.wide);
    }
  });
  return true;
}

} // namespace dg
