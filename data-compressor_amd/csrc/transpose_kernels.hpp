// transpose_kernels.hpp -- channel-major <-> time-major images of a batch for gfx950 (MI355X).
//
// The coders take samples time-major, [T][ld] with channel c in column c; a caller's series lie one after the other,
// [C][stride].  dega_transpose_kernel turns one image into the other on the device.  Both directions are the same
// transposition of a row-major source S[R][sp] (K used elements per row) into D[K][dp], D[k][r] = S[r][k]:
//   to time-major:    S = x_ct, R = C, K = T, sp = stride;  D = x_tc, dp = ld      (the channel is the SOURCE row)
//   to channel-major: S = x_tc, R = T, K = C, sp = ld;      D = x_ct, dp = stride  (the channel is the source COLUMN)
// Elements are 4 or 8 opaque bytes (float32 / int32 / big-endian int32; int64): nothing is computed on them.
//
// Contract:
//   * only the logical R x K region is read and only the K x R region written; pitch padding (dp - R elements behind
//     every destination row) is not touched, sp and dp may be odd, the bases need element alignment only;
//   * count (optional, uint64 per channel): element (c, t) with t >= min(count[c], T) is written as all-zero bits; its
//     source element may be loaded but is replaced before it is staged, so NaNs or poison there influence nothing;
//   * all offsets are 64-bit; the tiles are numbered along one flat index (blockIdx.y * gridDim.x + blockIdx.x) that
//     fills x first (2^24 - 1 workgroups, so that the launch's lanes along x stay below 2^32) and goes on in y, so
//     neither axis of the image is bounded by gridDim.y's 65 535;
//   * plain C++: no atomics, no cross-lane operation, one __syncthreads() per tile.
//
// A workgroup of 256 lanes (four waves) moves one tile of 64 x 64 elements through LDS.  Load: a wave reads whole rows
// of the source tile -- element form: 64 lanes x one element = one 256-byte (512-byte for 8-byte elements) segment of
// one row; 16-byte form: 16 (32) lanes x 16 bytes per row, 4 (2) rows per wave instruction -- and all of a lane's loads
// (16 / 4 / 8) are issued before the first is staged.  Store: the same pattern along the destination's rows.  The
// 16-byte forms are chosen per side by the launcher (base 16-byte aligned and pitch a multiple of 16 bytes, as the
// aggregate kernels decide it).  A tile that lies inside the region -- all but the last of a row or column of tiles --
// takes a path without a single test, so its loads go out back to back; an edge tile tests every element, and a vector
// that crosses the edge of the logical region falls back to elements in its lane, so the extent need not be a multiple
// of the vector.
//
// LDS layout: tile[64][65] elements, i.e. a row pitch of 65 dwords (4-byte) or 130 dwords (8-byte).  From the bank
// table of the LDS (ds_write_b32 / ds_read_b32: bank (a/4) mod 32 within the lane groups {0-31}, {32-63};
// ds_write_b64: bank (a/4) mod 32 within 4 groups of 16 lanes; ds_read_b64: bank (a/4) mod 64 within {0-31}, {32-63}):
//   4-byte, element form.  staging: lane l writes dword 65 i + l, banks l mod 32 -- 32 distinct, no conflict.
//     reading: lane l reads dword 65 l + j, bank (l + j) mod 32 -- 32 distinct, no conflict.
//   4-byte, 16-byte form.  staging: lane (i', l16) writes dwords 65 (i + i') + 4 l16 + q, one ds_write_b32 per q: within
//     a 32-lane group two rows, banks (i' + 4 l16 + q) mod 32 -- l16 and l16 + 8 meet: 2-way, which a ds_write_b32
//     hides behind its 4 issue cycles.  reading: lane reads dwords 65 (4 l16 + q) + j + j', bank (4 l16 + q + j + j')
//     mod 32 -- again l16 and l16 + 8: 2-way, 4 instead of 2 LDS cycles per ds_read_b32.
//   8-byte, element form.  staging (ds_write_b64): lane l writes dwords 130 i + 2 l, +1: 16 lanes cover 32 distinct banks,
//     no conflict.  reading (ds_read_b64): lane l reads dwords 130 l + 2 j, +1, banks (2 l + 2 j) mod 64, +1: 32 lanes,
//     64 distinct banks, no conflict.
//   8-byte, 16-byte form.  staging: dwords 130 (i + i') + 4 l32 + 2 q, +1: in a group of 16 lanes l32 and l32 + 8 meet:
//     2-way.  reading: dwords 130 (2 l32 + q) + 2 (j + j'), banks (4 l32 + 2 q + 2 j) mod 64: l32 and l32 + 16: 2-way.
// (The compiler pairs a lane's dword accesses into ds_write2_b32 / ds_read2_b32, which bank as two dword accesses.)
// A tile is 32 KiB (64 KiB) of HBM traffic against at most 512 (1 024) LDS cycles, a fifth of what the CU's share of
// HBM needs for it, so the 2-way cases cost nothing that shows; a swizzle would buy nothing.
//
// This header is compiled by hipcc (dega_hip.hip) and, for offline checking only, by g++ under tests/sim/.
#pragma once

#include "dega_intrinsics.hpp"
#include "dega_launch.hpp"

#include <stddef.h>

namespace dg
{

constexpr uint32_t TR_TILE = 64;   // elements per side of a tile
constexpr uint32_t TR_BLOCK = 256; // lanes per workgroup
constexpr uint32_t TR_GRID_X = 0xFFFFFFu; // workgroups along x in the library's launches: gridDim.x * TR_BLOCK stays below 2^32

struct TransposeArgs
{
  const void *src; // S[R][sp]
  void *dst;       // D[K][dp]
  size_t R, K, sp, dp;
  const uint64_t *count;  // per channel, or nullptr
  uint32_t count_on_rows; // the channel is the source row (to time-major); else the source column
  uint64_t tiles_k;       // tiles along K; tile q covers source rows 64 (q / tiles_k) .. and columns 64 (q % tiles_k) ..
  uint64_t tiles;
};

// Host side: the tiles of an R x K source and the grid that numbers them, at most gx_max workgroups along x (the
// library passes TR_GRID_X, so up to 2^24 x 65 535 tiles fit a launch; the emulator's tests pass a small number, so
// that the y part of the index is exercised).
// False when even gridDim.y cannot hold them.
inline bool tr_plan(size_t R, size_t K, uint64_t gx_max, TransposeArgs &a, uint32_t &gx, uint32_t &gy)
{
  const uint64_t tiles_r = ((uint64_t)R + TR_TILE - 1) / TR_TILE;
  a.tiles_k = ((uint64_t)K + TR_TILE - 1) / TR_TILE;
  if (a.tiles_k != 0 && tiles_r > ~(uint64_t)0 / a.tiles_k)
    return false;
  a.tiles = tiles_r * a.tiles_k;
  const uint64_t x = a.tiles < gx_max ? a.tiles : gx_max;
  const uint64_t y = x == 0 ? 0 : (a.tiles + x - 1) / x;
  if (y > 65535)
    return false;
  gx = (uint32_t)x;
  gy = (uint32_t)y;
  return true;
}

// V consecutive elements, the first at p: one load / store of sizeof(E) * V bytes where the launcher has checked the alignment
// (V = 16 / sizeof(E): global_load_dwordx4 / global_store_dwordx4)
template <typename E, uint32_t V>
static DG_DEV void tr_load(const E *p, E (&v)[V])
{
#if defined(DEGA_SIM)
  for (uint32_t q = 0; q < V; q++)
    v[q] = p[q];
#else
  typedef E Vec __attribute__((ext_vector_type(V)));
  const Vec w = *reinterpret_cast<const Vec *>(p);
#pragma unroll
  for (uint32_t q = 0; q < V; q++)
    v[q] = w[q];
#endif
}

template <typename E, uint32_t V>
static DG_DEV void tr_store(E *p, const E (&v)[V])
{
#if defined(DEGA_SIM)
  for (uint32_t q = 0; q < V; q++)
    p[q] = v[q];
#else
  typedef E Vec __attribute__((ext_vector_type(V)));
  Vec w;
#pragma unroll
  for (uint32_t q = 0; q < V; q++)
    w[q] = v[q];
  *reinterpret_cast<Vec *>(p) = w;
#endif
}

template <typename E>
using TrTile = E[TR_TILE][TR_TILE + 1];

// Source tile -> LDS.  A lane owns columns j .. j + VL - 1 of the tile rows i_first + 4 RPW u.  FULL: the tile lies inside
// the region (the same for the whole workgroup), so nothing is tested and every lane's loads are issued back to back;
// else every element is tested, and a vector that crosses the region's edge is done by elements.
template <typename E, uint32_t VL, bool FULL>
static DG_DEV void tr_stage(const TransposeArgs &a, TrTile<E> &tile, size_t r0, size_t k0, uint32_t lane, uint32_t wave)
{
  constexpr uint32_t LPR = TR_TILE / VL;          // lanes per row of the tile
  constexpr uint32_t RPW = 64 / LPR;              // rows per wave and step
  constexpr uint32_t STEPS = TR_TILE / (4 * RPW); // steps of the four waves
  const uint32_t j = (lane % LPR) * VL, i_first = wave * RPW + lane / LPR;
  const size_t k = k0 + j, r_first = r0 + i_first;
  const E *const p_first = static_cast<const E *>(a.src) + r_first * a.sp + k;
  const size_t step = (size_t)(4 * RPW) * a.sp; // (the same for every lane: the rows of a step lie one stride apart)
  E v[STEPS][VL];
#pragma unroll
  for (uint32_t u = 0; u < STEPS; u++) // every load of the lane first ...
  {
    const E *const p = p_first + u * step;
    if (FULL)
    {
      tr_load<E, VL>(p, v[u]);
      continue;
    }
#pragma unroll
    for (uint32_t e = 0; e < VL; e++)
      v[u][e] = 0;
    if (r_first + u * (4 * RPW) < a.R && k < a.K)
    {
      if (VL > 1 && k + VL <= a.K)
        tr_load<E, VL>(p, v[u]);
      else
        for (uint32_t e = 0; e < VL && k + e < a.K; e++)
          v[u][e] = p[e];
    }
  }
  // ... then they are staged; what lies behind a channel's count becomes zero bits on the way
  uint64_t n_col[VL]; // the channel is the source column: a lane's columns are the same in every step
#pragma unroll
  for (uint32_t e = 0; e < VL; e++)
    n_col[e] = a.count != nullptr && !a.count_on_rows && (FULL || k + e < a.K) ? a.count[k + e] : ~(uint64_t)0;
#pragma unroll
  for (uint32_t u = 0; u < STEPS; u++)
  {
    const size_t r = r_first + u * (4 * RPW);
    const uint64_t n_row = a.count != nullptr && a.count_on_rows && (FULL || r < a.R) ? a.count[r] : ~(uint64_t)0; // the channel is the source row
#pragma unroll
    for (uint32_t e = 0; e < VL; e++)
      tile[i_first + u * (4 * RPW)][j + e] = (k + e >= n_row || r >= n_col[e]) ? (E)0 : v[u][e];
  }
}

// LDS -> destination.  A lane owns source rows i .. i + VS - 1 (adjacent in a destination row) of the tile columns
// j_first + 4 RPW u.
template <typename E, uint32_t VS, bool FULL>
static DG_DEV void tr_drain(const TransposeArgs &a, const TrTile<E> &tile, size_t r0, size_t k0, uint32_t lane, uint32_t wave)
{
  constexpr uint32_t LPR = TR_TILE / VS;
  constexpr uint32_t RPW = 64 / LPR;
  constexpr uint32_t STEPS = TR_TILE / (4 * RPW);
  const uint32_t i = (lane % LPR) * VS, j_first = wave * RPW + lane / LPR;
  const size_t r = r0 + i, k_first = k0 + j_first;
  E *const p_first = static_cast<E *>(a.dst) + k_first * a.dp + r;
  const size_t step = (size_t)(4 * RPW) * a.dp;
#pragma unroll
  for (uint32_t u = 0; u < STEPS; u++)
  {
    E v[VS];
#pragma unroll
    for (uint32_t e = 0; e < VS; e++)
      v[e] = tile[i + e][j_first + u * (4 * RPW)];
    E *const p = p_first + u * step;
    if (FULL)
      tr_store<E, VS>(p, v);
    else if (k_first + u * (4 * RPW) < a.K && r < a.R)
    {
      if (VS > 1 && r + VS <= a.R)
        tr_store<E, VS>(p, v);
      else
        for (uint32_t e = 0; e < VS && r + e < a.R; e++)
          p[e] = v[e];
    }
  }
}

// E: uint32_t or uint64_t.  VL / VS: elements per lane and access on the load / store side, 1 or 16 / sizeof(E); with
// VL > 1 src is 16-byte aligned and sp a multiple of VL, with VS > 1 the same of dst and dp (the host checks).
template <typename E, uint32_t VL, uint32_t VS>
__global__ void __launch_bounds__(256) dega_transpose_kernel(const TransposeArgs a)
{
  __shared__ E tile[TR_TILE][TR_TILE + 1];
  const uint64_t q = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (q >= a.tiles) // (the whole workgroup: nobody is left waiting at the barrier)
    return;
  const size_t r0 = (size_t)(q / a.tiles_k) * TR_TILE, k0 = (size_t)(q % a.tiles_k) * TR_TILE;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const bool full = r0 + TR_TILE <= a.R && k0 + TR_TILE <= a.K; // all but the last tile of a row or column of tiles
  if (full)
    tr_stage<E, VL, true>(a, tile, r0, k0, lane, wave);
  else
    tr_stage<E, VL, false>(a, tile, r0, k0, lane, wave);
  __syncthreads();
  if (full)
    tr_drain<E, VS, true>(a, tile, r0, k0, lane, wave);
  else
    tr_drain<E, VS, false>(a, tile, r0, k0, lane, wave);
}

// ---- host side: how the kernel is launched (dega_launch.hpp) ----------------------------------------------------------------
struct TransposeVariant
{
  uint32_t elem_bytes; // 4 or 8
  bool wide_ld;        // 16-byte loads
  bool wide_st;        // 16-byte stores
};

// 16-byte loads / stores on each side whose every row starts on a 16-byte boundary (a vector that crosses the edge of the
// logical region is done by elements in its lane, so the extents do not matter)
inline TransposeVariant transpose_variant(const void *src, size_t sp, const void *dst, size_t dp, size_t elem_bytes)
{
  const size_t V = 16 / elem_bytes;
  return TransposeVariant{(uint32_t)elem_bytes, ((uintptr_t)src & 15u) == 0 && sp % V == 0, ((uintptr_t)dst & 15u) == 0 && dp % V == 0};
}

// S[R][sp] -> D[K][dp]; the channel (what `count` is indexed by) is the source row when channel_rows.  The tiles are
// launch()'s to fill in (tr_plan).
inline TransposeArgs transpose_args(const void *src, size_t R, size_t K, size_t sp, const uint64_t *count, bool channel_rows, void *dst, size_t dp)
{
  TransposeArgs a;
  a.src = src;
  a.dst = dst;
  a.R = R;
  a.K = K;
  a.sp = sp;
  a.dp = dp;
  a.count = count;
  a.count_on_rows = channel_rows ? 1u : 0u;
  a.tiles_k = a.tiles = 0;
  return a;
}

// `gx_max`: as tr_plan's
template <typename L>
inline bool launch(const TransposeVariant &v, TransposeArgs a, uint64_t gx_max, L &&launch_one)
{
  LaunchGrid grid;
  if ((v.elem_bytes != 4 && v.elem_bytes != 8) || !tr_plan(a.R, a.K, gx_max, a, grid.x, grid.y))
    return false;
  with_bools(
      [&](auto wide_elem, auto wide_ld, auto wide_st) {
        typedef std::conditional_t<decltype(wide_elem)::value, uint64_t, uint32_t> E;
        constexpr uint32_t V = 16 / sizeof(E);
        launch_one(dega_transpose_kernel<E, decltype(wide_ld)::value ? V : 1, decltype(wide_st)::value ? V : 1>, grid, TR_BLOCK, a);
      },
      v.elem_bytes == 8, v.wide_ld, v.wide_st);
  return true;
}

} // namespace dg
