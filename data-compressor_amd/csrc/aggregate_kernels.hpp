// aggregate_kernels.hpp -- the reference's `aggregate` stage (DCLib/src/aggregate.c:9-26) for gfx950 (MI355X).
//
// Sums every num_values consecutive readings of a channel: float32 [T][ld] -> float32 [ceil(T / N)][ld_out].  What has
// to match the reference is the rounding: Aggregate is `sum = 0; sum += value` from left to right, one rounding per
// add, and any other order gives other floats (and, behind Normalize, other streams).  So:
//   * one lane owns one (channel, output row) pair -- in the 16-byte form four adjacent channels, four independent
//     sums -- and walks its rows in order; a group is never split over lanes, waves or workgroups, nothing is combined
//     afterwards, there is no cross-lane operation and no atomic;
//   * every sum starts at +0.0f and its first add is 0.0f + v (aggregate.c:13,20: -0.0f comes out as +0.0f, also for
//     num_values = 1);
//   * the short last group of a series whose length is no multiple of N is written as it stands (aggregate.c:21-22).
// Parallelism is channels x output rows: lanes are adjacent channels (a wave's row read is one 256-byte or 1-KiB
// segment), blockIdx.y takes a range of OUTPUT rows, so ranges are cut at multiples of N by construction.
//
// The bound is HBM (T rows read, T / N written), the adds are nothing; what matters is loads in flight.  A lane issues
// AGG_DEPTH independent row loads, then does the dependent adds, whatever N is: the walk is over input rows, and a
// counter tells where a group ends (wave-uniform, a scalar branch), so N = 2 keeps as many loads in flight as N = 900.
//
// This header is compiled by hipcc (dega_hip.hip) and, for offline checking only, by g++ under tests/sim/.
#pragma once

#include "dega_intrinsics.hpp"
#include "dega_launch.hpp"

#include <stddef.h>

namespace dg
{

constexpr uint32_t AGG_BLOCK = 256; // lanes per workgroup: 256 (dword form) or 1 024 (16-byte form) adjacent channels
constexpr uint32_t AGG_DEPTH = 16;  // rows loaded before the first of them is added: 16 KiB per wave in the 16-byte form

struct AggregateArgs
{
  const float *v; // [T][ld]
  float *a;       // [T_out][ld_out]
  size_t C, T, ld, N, T_out, ld_out;
  size_t rows_per_block; // output rows per blockIdx.y
  uint32_t wide_out;     // 16-byte form: a and ld_out allow 16-byte stores as well (else four dword stores per lane)
};

struct AggF4 // four adjacent channels; 16-byte aligned where the kernel uses it
{
  float x, y, z, w;
};

template <typename V>
struct AggLane;

template <>
struct AggLane<float>
{
  static constexpr size_t WIDTH = 1;
  static DG_DEV float zero() { return 0.0f; }
  static DG_DEV float load(const float *p) { return *p; }
  static DG_DEV void add(float &s, const float v) { s = fadd_once(s, v); }
  static DG_DEV void store(float *p, const float s, uint32_t) { *p = s; }
};

template <>
struct AggLane<AggF4>
{
  static constexpr size_t WIDTH = 4;
  static DG_DEV AggF4 zero() { return AggF4{0.0f, 0.0f, 0.0f, 0.0f}; }
  static DG_DEV AggF4 load(const float *p)
  {
#if defined(DEGA_SIM)
    return AggF4{p[0], p[1], p[2], p[3]};
#else
    const float4 q = *reinterpret_cast<const float4 *>(p); // one global_load_dwordx4
    return AggF4{q.x, q.y, q.z, q.w};
#endif
  }
  static DG_DEV void add(AggF4 &s, const AggF4 v)
  {
    s.x = fadd_once(s.x, v.x);
    s.y = fadd_once(s.y, v.y);
    s.z = fadd_once(s.z, v.z);
    s.w = fadd_once(s.w, v.w);
  }
  static DG_DEV void store(float *p, const AggF4 s, uint32_t wide) // wide is the same for every lane
  {
#if !defined(DEGA_SIM)
    if (wide)
    {
      *reinterpret_cast<float4 *>(p) = make_float4(s.x, s.y, s.z, s.w);
      return;
    }
#endif
    p[0] = s.x;
    p[1] = s.y;
    p[2] = s.z;
    p[3] = s.w;
  }
};

// V = float: any ld and alignment.  V = AggF4: C and ld multiples of 4 and v 16-byte aligned (the host checks), so that
// a lane's four channels are one aligned 16-byte load that stays inside the row's C values.
template <typename V>
__global__ void __launch_bounds__(256) dega_aggregate_kernel(const AggregateArgs a)
{
  typedef AggLane<V> L;
  const size_t c = ((size_t)blockIdx.x * AGG_BLOCK + threadIdx.x) * L::WIDTH;
  if (c >= a.C)
    return;
  const size_t j0 = (size_t)blockIdx.y * a.rows_per_block;
  if (j0 >= a.T_out)
    return;
  const size_t j1 = j0 + a.rows_per_block < a.T_out ? j0 + a.rows_per_block : a.T_out;
  const size_t t0 = j0 * a.N;                          // (j0 < T_out = ceil(T / N), so t0 < T)
  const size_t t1 = j1 == a.T_out ? a.T : j1 * a.N;    // only the series' last group may be short
  const float *src = a.v + t0 * a.ld + c;
  float *dst = a.a + j0 * a.ld_out + c;
  V sum = L::zero();
  size_t k = 0; // rows of the open group already added
  size_t t = t0;
  for (; t + AGG_DEPTH <= t1; t += AGG_DEPTH)
  {
    V row[AGG_DEPTH];
#pragma unroll
    for (uint32_t u = 0; u < AGG_DEPTH; u++) // loads first ...
      row[u] = L::load(src + (size_t)u * a.ld);
    src += (size_t)AGG_DEPTH * a.ld;
#pragma unroll
    for (uint32_t u = 0; u < AGG_DEPTH; u++) // ... the adds, in row order, after
    {
      L::add(sum, row[u]);
      if (++k == a.N)
      {
        L::store(dst, sum, a.wide_out);
        dst += a.ld_out;
        sum = L::zero();
        k = 0;
      }
    }
  }
  for (; t < t1; t++) // fewer than AGG_DEPTH rows left in the range
  {
    L::add(sum, L::load(src));
    src += a.ld;
    if (++k == a.N)
    {
      L::store(dst, sum, a.wide_out);
      dst += a.ld_out;
      sum = L::zero();
      k = 0;
    }
  }
  if (k != 0) // the series ended inside a group: aggregate.c:21-22 writes what it has
    L::store(dst, sum, a.wide_out);
}

// ---- host side: how the aggregate kernels are launched (dega_launch.hpp) -----------------------------------------------------
// One variant for this kernel, dega_aggregate_levels_kernel and dega_aggregate_var_kernel.
struct AggregateVariant
{
  bool wide;       // the 16-byte form: four channels per lane
  uint32_t levels; // levels summed in the pass (1 for this kernel)
};

// four channels per lane where every row allows aligned 16-byte loads that stay inside its C values; else one
inline bool aggregate_wide(const float *v, size_t C, size_t ld)
{
  return C % 4 == 0 && ld % 4 == 0 && ((uintptr_t)v & 15u) == 0;
}

inline bool aggregate_wide_out(bool wide, const float *a, size_t ld_out)
{
  return wide && ld_out % 4 == 0 && ((uintptr_t)a & 15u) == 0;
}

inline size_t aggregate_gx(size_t C, bool wide)
{
  const size_t units = wide ? C / 4 : C;
  return (units + AGG_BLOCK - 1) / AGG_BLOCK;
}

inline size_t aggregate_rows(size_t T, size_t N)
{
  return N == 0 ? 0 : T / N + (T % N != 0 ? 1 : 0);
}

// Ranges of output rows along y (the unit is an output row, so the ranges are cut at multiples of N): enough workgroups for
// eight per CU where the batch has them, never more ranges than output rows.
inline size_t aggregate_row_ranges(size_t C, size_t T_out, bool wide)
{
  const size_t gx = aggregate_gx(C, wide), want = (2048 + gx - 1) / gx;
  const size_t most = T_out < 65535 ? T_out : 65535;
  return most < want ? most : (want > 1 ? want : 1);
}

// `row_ranges`: aggregate_row_ranges, or what a test forces (at most T_out are used)
inline AggregateArgs aggregate_args(const float *v, size_t C, size_t T, size_t ld, size_t N, float *a, size_t ld_out, bool wide, size_t row_ranges)
{
  AggregateArgs g;
  g.v = v;
  g.a = a;
  g.C = C;
  g.T = T;
  g.ld = ld;
  g.N = N;
  g.T_out = aggregate_rows(T, N);
  g.ld_out = ld_out;
  if (row_ranges > g.T_out)
    row_ranges = g.T_out;
  g.rows_per_block = (g.T_out + row_ranges - 1) / row_ranges;
  g.wide_out = aggregate_wide_out(wide, a, ld_out) ? 1u : 0u;
  return g;
}

template <typename L>
inline bool launch(const AggregateVariant &v, const AggregateArgs &a, L &&launch_one)
{
  const size_t gx = aggregate_gx(a.C, v.wide);
  if (v.levels != 1 || gx > LAUNCH_MAX_GX)
    return false;
  const LaunchGrid grid{(uint32_t)gx, (uint32_t)((a.T_out + a.rows_per_block - 1) / a.rows_per_block)};
  with_bools([&](auto wide) { launch_one(dega_aggregate_kernel<std::conditional_t<decltype(wide)::value, AggF4, float>>, grid, AGG_BLOCK, a); }, v.wide);
  return true;
}

} // namespace dg
