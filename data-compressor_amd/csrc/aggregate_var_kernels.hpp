// aggregate_var_kernels.hpp -- the `aggregate` stage (DCLib/src/aggregate.c:9-26) over a RAGGED batch, for gfx950 (MI355X).
//
// The readers report a count per channel (dega_hip_csv_read_*, the decoders' out_count); here channel c is rows
// 0 .. count[c] - 1 of its column and the rows behind them are unspecified -- NaN, infinities, anything.  Per channel the
// result is what dega_aggregate_kernel / dega_aggregate_levels_kernel give for that channel alone with T = count[c]:
// K independent float32 accumulators from +0.0f, one rounding per add, rows from left to right.
//
// The walk is the uniform kernels' (AggLane, AGG_BLOCK, AGG_DEPTH are theirs): lanes are adjacent channels, four per lane in
// the 16-byte form, AGG_DEPTH independent row loads before the first dependent add, group boundaries are wave-uniform
// counters and blockIdx.y takes `step` base rows, a multiple of every level's N (or all T rows).  What differs:
//   * a wave walks its range only up to the largest count among its lanes, and in two phases: while every lane still has
//     AGG_DEPTH rows the loop body is the uniform kernel's, instruction for instruction; from the wave's smallest count on
//     a row is added under `t < count` -- a SELECT, never a multiply by 0: the dead rows may be NaN;
//   * a group is stored by the lanes that have at least one reading in it (the group's first row is below their count),
//     so a channel's short last group is per lane and level l gets exactly ceil(count / N[l]) rows of column c;
//   * the first range of a column reports those row counts, and the status: count[c] > T gives the channel
//     ERR_INVALID_VALUE, no row and counts of 0.
// K = 1 .. AGG_MAX_LEVELS: one level is this kernel with K = 1.  Counters are 32-bit: the host refuses T >= 2^32.
//
// Compiled by hipcc (dega_hip.hip) and, for offline checking only, by g++ under tests/sim/.
#pragma once

#include "aggregate_levels_kernels.hpp"

namespace dg
{

constexpr int32_t AGGV_OK = 0, AGGV_ERR_INVALID_VALUE = -1; // DEGA_OK, DEGA_ERROR_INVALID_VALUE

template <uint32_t K>
struct AggregateVarArgs
{
  const float *v; // [T][ld]
  size_t C, T, ld;
  size_t step;           // base rows per blockIdx.y: a multiple of every N[l], or >= T
  const uint64_t *count; // [C]
  float *a[K];           // level l: rows 0 .. ceil(count[c] / N[l]) - 1 of column c
  size_t ld_out[K];
  uint32_t N[K];         // 1 .. max(T, 1)
  uint32_t wide_out[K];  // 16-byte form: level l's array and pitch allow 16-byte stores
  uint64_t *out_count[K]; // [C] each
  int32_t *err;          // [C], or NULL in every pass of a call but its first
};

// A lane's end(s): the counts of its WIDTH channels, and the adds and stores that look at them.
template <typename V>
struct AggEnds;

template <>
struct AggEnds<float>
{
  uint32_t n;
  DG_DEV void load(const uint64_t *count, size_t T, int32_t *err, bool report)
  {
    const uint64_t k = *count;
    n = k > T ? 0u : (uint32_t)k;
    if (report && err != nullptr)
      *err = k > T ? AGGV_ERR_INVALID_VALUE : AGGV_OK;
  }
  DG_DEV void none() { n = 0; }
  DG_DEV uint32_t most() const { return n; }
  DG_DEV uint32_t least() const { return n; }
  DG_DEV void add(float &s, const float v, uint32_t t) const
  {
    const float r = fadd_once(s, v);
    s = t < n ? r : s;
  }
  DG_DEV void store(float *p, const float s, uint32_t first, uint32_t) const // first: the group's first row
  {
    if (first < n)
      *p = s;
  }
  DG_DEV void rows(uint64_t *out, uint32_t N) const { *out = ((uint64_t)n + (N - 1u)) / N; }
};

template <>
struct AggEnds<AggF4>
{
  uint32_t n[4];
  DG_DEV void load(const uint64_t *count, size_t T, int32_t *err, bool report)
  {
#pragma unroll
    for (uint32_t i = 0; i < 4; i++)
    {
      const uint64_t k = count[i];
      n[i] = k > T ? 0u : (uint32_t)k;
      if (report && err != nullptr)
        err[i] = k > T ? AGGV_ERR_INVALID_VALUE : AGGV_OK;
    }
  }
  DG_DEV void none() { n[0] = n[1] = n[2] = n[3] = 0; }
  DG_DEV uint32_t most() const
  {
    const uint32_t x = n[0] > n[1] ? n[0] : n[1], y = n[2] > n[3] ? n[2] : n[3];
    return x > y ? x : y;
  }
  DG_DEV uint32_t least() const
  {
    const uint32_t x = n[0] < n[1] ? n[0] : n[1], y = n[2] < n[3] ? n[2] : n[3];
    return x < y ? x : y;
  }
  DG_DEV void add(AggF4 &s, const AggF4 v, uint32_t t) const
  {
    const float x = fadd_once(s.x, v.x), y = fadd_once(s.y, v.y), z = fadd_once(s.z, v.z), w = fadd_once(s.w, v.w);
    s.x = t < n[0] ? x : s.x;
    s.y = t < n[1] ? y : s.y;
    s.z = t < n[2] ? z : s.z;
    s.w = t < n[3] ? w : s.w;
  }
  DG_DEV void store(float *p, const AggF4 s, uint32_t first, uint32_t wide) const
  {
    if (first < least())
    {
      AggLane<AggF4>::store(p, s, wide);
      return;
    }
    if (first < n[0])
      p[0] = s.x;
    if (first < n[1])
      p[1] = s.y;
    if (first < n[2])
      p[2] = s.z;
    if (first < n[3])
      p[3] = s.w;
  }
  DG_DEV void rows(uint64_t *out, uint32_t N) const
  {
#pragma unroll
    for (uint32_t i = 0; i < 4; i++)
      out[i] = ((uint64_t)n[i] + (N - 1u)) / N;
  }
};

// V as in dega_aggregate_kernel: float for any ld and alignment, AggF4 where the host has checked the 16-byte conditions.
template <typename V, uint32_t K>
__global__ void __launch_bounds__(256) dega_aggregate_var_kernel(const AggregateVarArgs<K> a)
{
  static_assert(K >= 1 && K <= AGG_MAX_LEVELS, "levels per pass");
  typedef AggLane<V> L;
  const size_t c = ((size_t)blockIdx.x * AGG_BLOCK + threadIdx.x) * L::WIDTH;
  const bool live = c < a.C;
  AggEnds<V> ends;
  if (live)
    ends.load(a.count + c, a.T, a.err != nullptr ? a.err + c : nullptr, blockIdx.y == 0);
  else
    ends.none();
  // the wave's rows: up to its longest channel; from its shortest one on, adds are selected per lane
  const size_t wave_end = wave_uniform(wave_max_u32(ends.most()));
  const size_t wave_all = wave_uniform(wave_min_u32(live ? ends.least() : 0xFFFFFFFFu));
  if (!live)
    return;
  if (blockIdx.y == 0)
  {
#pragma unroll
    for (uint32_t l = 0; l < K; l++)
      ends.rows(a.out_count[l] + c, a.N[l]);
  }
  const size_t t0 = (size_t)blockIdx.y * a.step;
  if (t0 >= wave_end)
    return;
  const size_t t1 = a.step < wave_end - t0 ? t0 + a.step : wave_end;
  const float *src = a.v + t0 * a.ld + c;
  float *dst[K];
  V sum[K];
  uint32_t k[K];     // rows of level l's open group already walked (wave-uniform)
  uint32_t first[K]; // the first row of that group (wave-uniform)
#pragma unroll
  for (uint32_t l = 0; l < K; l++)
  {
    dst[l] = a.a[l] + (t0 / a.N[l]) * a.ld_out[l] + c; // t0 is a multiple of N[l]: the range opens a group of every level
    sum[l] = L::zero();
    k[l] = 0;
    first[l] = (uint32_t)t0;
  }
  size_t t = t0;
  // ---- every lane still has these rows: the uniform kernel's loop ----
  const size_t t_all = wave_all < t1 ? wave_all : t1;
  for (; t + AGG_DEPTH <= t_all; t += AGG_DEPTH)
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
          L::store(dst[l], sum[l], a.wide_out[l]); // (the group's rows are all below every lane's count)
          dst[l] += a.ld_out[l];
          sum[l] = L::zero();
          k[l] = 0;
          first[l] += a.N[l];
        }
      }
    }
  }
  // ---- some lane has ended: the same walk, a row added only below the lane's count ----
  for (; t + AGG_DEPTH <= t1; t += AGG_DEPTH)
  {
    V row[AGG_DEPTH];
#pragma unroll
    for (uint32_t u = 0; u < AGG_DEPTH; u++)
      row[u] = L::load(src + (size_t)u * a.ld);
    src += (size_t)AGG_DEPTH * a.ld;
#pragma unroll
    for (uint32_t u = 0; u < AGG_DEPTH; u++)
    {
#pragma unroll
      for (uint32_t l = 0; l < K; l++)
      {
        ends.add(sum[l], row[u], (uint32_t)t + u);
        if (++k[l] == a.N[l])
        {
          ends.store(dst[l], sum[l], first[l], a.wide_out[l]);
          dst[l] += a.ld_out[l];
          sum[l] = L::zero();
          k[l] = 0;
          first[l] += a.N[l];
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
      ends.add(sum[l], r, (uint32_t)t);
      if (++k[l] == a.N[l])
      {
        ends.store(dst[l], sum[l], first[l], a.wide_out[l]);
        dst[l] += a.ld_out[l];
        sum[l] = L::zero();
        k[l] = 0;
        first[l] += a.N[l];
      }
    }
  }
#pragma unroll
  for (uint32_t l = 0; l < K; l++)
    if (k[l] != 0) // the wave's rows end inside a group of level l: aggregate.c:21-22 writes what it has, lane by lane
      ends.store(dst[l], sum[l], first[l], a.wide_out[l]);
}

// ---- host side: how the kernel is launched (dega_launch.hpp) ----------------------------------------------------------------

// what a counted pass has beside its AggregatePass
struct AggregateCounts
{
  const uint64_t *count;
  uint64_t *const *out_count; // one array per level of the pass
  int32_t *err;               // the status is one pass's to write: null in every pass of a call but its first
};

// one to AGG_MAX_LEVELS levels; p.step 0 counts as 1, and an image without rows still has one range (the counts and the
// status are the kernel's)
template <typename L>
inline bool launch(const AggregateVariant &v, const AggregatePass &pass, const AggregateCounts &c, L &&launch_one)
{
  const size_t gx = aggregate_gx(pass.C, v.wide);
  if (v.levels < 1 || v.levels > AGG_MAX_LEVELS || gx > LAUNCH_MAX_GX)
    return false;
  AggregatePass p = pass;
  p.step = p.step > 1 ? p.step : 1;
  const size_t ranges = (p.T + p.step - 1) / p.step;
  const LaunchGrid grid{(uint32_t)gx, (uint32_t)(ranges > 1 ? ranges : 1)};
  for_levels_of_pass(v.levels, [&](auto levels) {
    constexpr uint32_t NL = decltype(levels)::value;
    AggregateVarArgs<NL> g;
    fill_pass(g, NL, v.wide, p);
    g.count = c.count;
    g.err = c.err;
    for (uint32_t l = 0; l < NL; l++)
      g.out_count[l] = c.out_count[l];
    with_bools([&](auto wide) { launch_one(dega_aggregate_var_kernel<std::conditional_t<decltype(wide)::value, AggF4, float>, NL>, grid, AGG_BLOCK, g); },
               v.wide);
  });
  return true;
}

} // namespace dg
