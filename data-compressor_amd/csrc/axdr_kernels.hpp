// axdr_kernels.hpp -- A-XDR, the reference's third coding (`decode csv # encode normalize`), for gfx950 (MI355X).
//
// A-XDR is every reading of a channel as one big-endian two's-complement field of `valuesize` bits, packed MSB first, the
// last byte zero padded: what Normalize writes (DCLib/src/normalize.c:9-27) and Denormalize reads (:29-41), and the
// uncompressed size a compression ratio is taken against.  dega_axdr_pack_kernel turns time-major rows [T][ld] (float32
// readings, or int32 / int64 containers of fields) into one field stream per channel, uint8 [C][cap] -- the container of
// the DEGA streams: big-endian 32-bit words, the exact bit length in out_bits[c]; dega_axdr_unpack_kernel is the inverse.
// Both are a transposition with a bit pack in the middle, built on the pattern of transpose_kernels.hpp.
//
// Mapping.  A workgroup of 256 lanes (four waves) takes a tile of 64 channels x R rows, R = 128 for value sizes 1..32 and
// 64 for 33..64.  R is a multiple of 32, so a channel's share of a tile is a whole number of 32-bit words whatever the
// value size: R vs / 32 of them (4 vs, 2 vs), word aligned in the slab -- no word belongs to two tiles, and no tile waits
// for another.  Tiles are numbered along one flat index as tr_plan's are (x first, then y); tile q covers rows
// R (q / tiles_c) .. and channels 64 (q % tiles_c) ..; all offsets (t ld, c cap, the word position (t / 32) vs) are 64-bit.
//
// Pack.  Load side: the transposition's -- a wave reads whole row segments, 64 lanes x one element (256 bytes; 512 for
// int64) or 16 bytes per lane where base and pitch allow (the launcher decides as transpose_variant does), all of a
// lane's loads (32 / 8; wide 16 / 8 / 4) issued before the first is staged.  On the way into LDS a float is normalized
// with normalize_value / normalize_value64 and their lo / hi / mask (the one restatement of normalize.c:17-24 there is);
// an integer keeps its low valuesize bits, whatever lies above them in the container.  A row at or behind the channel's
// count (count[c], else T) may be loaded but is staged as the field 0 and judged by nobody, so the last word of a channel
// is zero behind its last field.  A lane's channels are the same in every step: its verdict (normalize.c:21 failed on a
// row that counts) is one plain store of DEGA_ERROR_INVALID_VALUE to err[c], which the caller has zeroed; every lane that
// finds one stores the same value.  Store side: the 64 x (R vs / 32) words of the tile are numbered channel by channel
// and dealt to the lanes in turn, so consecutive lanes store consecutive words of one channel's run (a wave: 256
// contiguous bytes, or the ends of two runs).  A word gathers the fields that touch it from LDS: the first is
// floor(32 w / vs) -- a multiply-high with ceil(2^32 / vs), exact below 2^32 / 64 bits, which a tile's 4 096 are -- then
// at most one more for vs >= 32 and ceil(32 / vs) more below.  The word is stored byte swapped.  A tile inside the region
// of a call without counts whose streams fit takes both sides without a per-element test; every other tile tests rows
// against the channel's count and words against the channel's length (lim_of[], in LDS before the barrier).
// The tile of a channel's first rows also writes out_bits[c] and a channel-level status (count[c] > T:
// DEGA_ERROR_INVALID_VALUE; a stream that does not fit cap: DEGA_ERROR_MEMORY; both with 0 bits and nothing written, and
// no verdict on their rows -- so no two stores to err[c] ever differ).
//
// Unpack.  Load side: the same dealing of words to lanes -- a channel's run for the tile goes to LDS coalesced along the
// run, byte swapped; eight loads of a lane are issued before the first is staged.  Words are loaded as far as the slab
// reaches (cap), not as far as the stream does: what lies at or beyond in_bits may be loaded, but no field that is stored
// holds a bit of it.  Store side: the transposition's -- a lane extracts field (channel, row) from the 2 (vs <= 32) or 3
// words that hold it, leaves it as it is (int32 / int64: the field in the low bits, zero above) or sign-extends, converts
// and divides it (denormalize_value; the 64-bit conversion is the decoders' float exit's), and rows are stored whole, by
// elements or 16 bytes per lane.  Per channel count = in_bits / vs; status 0, or DEGA_ERROR_LIBRARY_CALL (-11: the
// reference's READ_BITS_CHECKED on a stream that ends inside a field) where in_bits % vs != 0, DEGA_ERROR_MEMORY where
// count > max_T (out_count[c] = the room needed), DEGA_ERROR_INVALID_VALUE where in_bits > 8 cap; a channel in error
// stores no row.  The tile of a channel's first rows writes out_count[c] and err[c].
//
// Plain C++: no atomics, no cross-lane operation, no waiting wave, one __syncthreads() per tile.
//
// LDS layout (bank table: transpose_kernels.hpp).
//   pack: tile[64][R + 1] fields -- uint32 for vs <= 32 (pitch 129 dwords, 33 KiB), uint64 above (pitch 130 dwords, 33 KiB).
//     staging, element form: lane l writes dword 129 l + i, banks (l + i) mod 32: 32 distinct, no conflict; 8-byte fields
//     (ds_write_b64) dwords 130 l + 2 i, +1: 16 lanes cover 32 banks, no conflict.  16-byte form: lane (i', l16) writes dwords
//     129 (4 l16 + q) + i + i': l16 and l16 + 8 meet, 2-way, hidden behind a ds_write_b32's 4 issue cycles (8-byte: the
//     transposition's 2-way case likewise).
//     gathering: lane reads dword 129 j + f with f = floor(32 w / vs) + k.  vs >= 32: consecutive lanes read the same or
//     the next address -- no conflict (a broadcast where they share a field).  vs < 32: consecutive words lie 32 / vs rows
//     apart, so the 32 lanes of a group meet on 32 / (32 / vs) = vs banks where vs divides 32 -- and a group that holds
//     several channels (4 vs < 32) spreads them over one more bank each: 4-way at vs 1, 2, 4 and 8, 2-way at 16, between
//     them for the others.  Its price: a lane makes 32 + vs reads per tile, at 4-way 8 LDS cycles per wave instruction,
//     so four waves spend at most 4 x 64 x 8 = 2 048 LDS cycles on a tile of 32 KiB loaded and 1 KiB vs stored -- of the
//     order of 4 000 cycles of the CU's share of HBM (one of 256 CUs at about 5 TB/s and 2.4 GHz).  REASONED from the
//     bank table, not measured; a swizzle of the rows would remove it and has not been tried.
//   unpack: words[64][131] dwords (the longest run, 128 words, and the two words behind it that the extraction of the last
//     fields may touch; 33 KiB).  staging: consecutive lanes, consecutive dwords: no conflict.  extraction, element form:
//     lane l reads dword 131 l + wi, banks (3 l + wi) mod 32 -- 3 is odd: 32 distinct, no conflict; 16-byte form: lane
//     (i', l16) reads dwords 131 (4 l16 + q) + wi(i + i'), banks (12 l16 + 3 q + wi) mod 32: l16 and l16 + 8 meet, 2-way.
//
// This header is compiled by hipcc (dega_hip.hip) and, for offline checking only, by g++ under tests/sim/.
#pragma once

#include "dega_kernels.hpp"
#include "transpose_kernels.hpp"

#include <stddef.h>

namespace dg
{

constexpr uint32_t AX_CH = 64;     // channels per tile
constexpr uint32_t AX_BLOCK = 256; // lanes per workgroup
constexpr uint32_t AX_UNPACK_PITCH = 131; // dwords per channel of the unpack kernel's LDS image
constexpr uint32_t AX_F32 = 0, AX_I32 = 1, AX_I64 = 2; // what the rows hold (DEGA_SAMPLES_F32, _I32, _I64)
constexpr size_t AX_MAX_T = 0xFFFFFFFFu; // rows per channel and call: a channel's rows are counted in 32 bits

constexpr uint32_t ax_rows(bool w64) // R
{
  return w64 ? 64u : 128u;
}

struct AxdrPackArgs
{
  const void *x; // [T][ld]: float32 bits, int32 or int64
  size_t C, T, ld;
  const uint64_t *count; // per channel, or nullptr
  uint8_t *out;          // [C][cap]
  size_t cap;            // bytes per channel, a multiple of 4
  uint64_t *out_bits;
  int32_t *err;          // [C], zeroed by the caller
  uint32_t vs, vs_magic; // value size; ceil(2^32 / vs) (vs = 1: not used)
  float factor, lo, hi;  // float rows: normalize.c:21's range for the value size, rounded to float by the host compiler
  uint64_t mask;         // the low vs bits
  uint32_t fits_T;       // a stream of T fields fits cap
  uint64_t tiles_c;      // tiles along the channels
  uint64_t tiles;
};

struct AxdrUnpackArgs
{
  const uint8_t *in; // [C][cap]
  size_t cap;
  const uint64_t *in_bits;
  size_t C, max_T, ld;
  void *x; // [max_T][ld]: float32, int32 or int64
  uint64_t *out_count;
  int32_t *err;
  uint32_t vs;
  float factor;
  uint64_t mask;
  uint64_t tiles_c, tiles;
};

DG_DEV uint64_t ax_words(uint64_t fields, uint32_t vs) // 32-bit words of a stream (fields < 2^32)
{
  return (fields * vs + 31u) >> 5;
}

// The rows of channel c that are packed, with the channel-level status: none of a channel whose count is above T or
// whose stream does not fit its slab.
DG_DEV uint32_t ax_pack_rows(const AxdrPackArgs &a, size_t c, int32_t &status)
{
  const uint64_t n = a.count != nullptr ? a.count[c] : (uint64_t)a.T;
  status = OK;
  if (n > a.T)
    status = ERR_INVALID_VALUE;
  else if (ax_words(n, a.vs) * 4u > a.cap)
    status = ERR_MEMORY;
  return status == OK ? (uint32_t)n : 0u;
}

// The fields of channel c that are unpacked, with its status and the count it reports
DG_DEV uint32_t ax_unpack_rows(const AxdrUnpackArgs &a, size_t c, int32_t &status, uint64_t &count)
{
  const uint64_t bits = a.in_bits[c];
  status = OK;
  count = 0;
  if (bits > 8u * (uint64_t)a.cap)
    status = ERR_INVALID_VALUE;
  else
  {
    count = bits / a.vs;
    if (count * a.vs != bits)
      status = ERR_LIBRARY_CALL; // the stream ends inside a field (normalize.c:36)
    else if (count > a.max_T)
      status = ERR_MEMORY;
  }
  return status == OK ? (uint32_t)count : 0u;
}

// The words of the tile's run (word0 ..) that a channel of `words` words holds
DG_DEV uint32_t ax_run_words(uint64_t words, uint64_t word0, uint32_t run)
{
  if (words <= word0)
    return 0u;
  return words - word0 < run ? (uint32_t)(words - word0) : run;
}

DG_DEV uint32_t ax_first_field(uint32_t bit, uint32_t vs, uint32_t magic) // floor(bit / vs) for bit < 2^26
{
  return vs == 1u ? bit : mulhi32(bit, magic);
}

// Word w of a run from the fields of its channel: every field that touches bits 32 w .. 32 w + 31
template <typename F>
static DG_DEV uint32_t ax_gather(const F *fields, uint32_t w, uint32_t vs, uint32_t magic)
{
  const uint32_t b0 = 32u * w;
  uint32_t f = ax_first_field(b0, vs, magic); // the first field index of an output word
  int32_t sh = 32 - (int32_t)vs + (int32_t)(b0 - f * vs); // the field's last bit lies sh bits above the word's last (sh < 0: below)
  uint32_t word = 0;
  do
  {
    const F v = fields[f];
    if constexpr (sizeof(F) == 4)
      word |= (uint32_t)(((uint64_t)v << 32) >> (32 - sh)); // (sh in -31 .. 31)
    else
      word |= (uint32_t)(sh >= 0 ? v << sh : v >> -sh); // (sh in -63 .. 31)
    f++;
    sh -= (int32_t)vs;
  } while (sh > -(int32_t)vs);
  return word;
}

// Source rows -> fields in LDS.  A lane owns channels j .. j + VL - 1 of the tile rows i_first + 4 RPW u.  FULL: the tile
// lies inside the region, so nothing is tested and every lane's loads are issued back to back.
template <uint32_t KIND, bool W64, uint32_t VL, bool FULL, typename F>
static DG_DEV void ax_stage(const AxdrPackArgs &a, F (&tile)[AX_CH][ax_rows(W64) + 1], size_t t0, size_t c0, uint32_t lane, uint32_t wave)
{
  typedef std::conditional_t<KIND == AX_I64, uint64_t, uint32_t> E;
  constexpr uint32_t R = ax_rows(W64);
  constexpr uint32_t LPR = AX_CH / VL;
  constexpr uint32_t RPW = 64 / LPR;
  constexpr uint32_t STEPS = R / (4 * RPW);
  const uint32_t j = (lane % LPR) * VL, i_first = wave * RPW + lane / LPR;
  const size_t c = c0 + j, t_first = t0 + i_first;
  const E *const p_first = static_cast<const E *>(a.x) + t_first * a.ld + c;
  const size_t step = (size_t)(4 * RPW) * a.ld;
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
    if (VL == 1)
    {
      // an edge tile by elements: the element of the region's last row / last channel in place of one beyond it, so that the
      // loads go out back to back here too -- it is staged as the field 0 like every row that does not count
      if (a.T != 0)
      {
        const size_t t = t_first + u * (4 * RPW);
        v[u][0] = static_cast<const E *>(a.x)[(t < a.T ? t : a.T - 1) * a.ld + (c < a.C ? c : a.C - 1)];
      }
    }
    else if (t_first + u * (4 * RPW) < a.T && c < a.C)
    {
      if (VL > 1 && c + VL <= a.C)
        tr_load<E, VL>(p, v[u]);
      else
        for (uint32_t e = 0; e < VL && c + e < a.C; e++)
          v[u][e] = p[e];
    }
  }
  // ... then they become fields; what lies at or behind a channel's count becomes the field 0 and is not judged
  uint32_t n[VL];
  bool bad[VL];
#pragma unroll
  for (uint32_t e = 0; e < VL; e++)
  {
    int32_t status;
    n[e] = (FULL || c + e < a.C) ? ax_pack_rows(a, c + e, status) : 0u;
    bad[e] = false;
  }
#pragma unroll
  for (uint32_t u = 0; u < STEPS; u++)
  {
    const size_t t = t_first + u * (4 * RPW);
#pragma unroll
    for (uint32_t e = 0; e < VL; e++)
    {
      F f;
      bool in_range = true;
      if constexpr (KIND == AX_F32)
      {
        // one reading at a time, between two points the compiler keeps in order: left alone, hipcc packs the multiplies and
        // adds of all the steps into vectors of floats (v_pk_*), keeps every step's operands alive and runs out of registers
        E raw = v[u][e];
        DG_MATERIALISE(raw);
        if constexpr (W64)
        {
          uint64_t wide;
          in_range = normalize_value64(__uint_as_float(raw), a.factor, wide, a.lo, a.hi, a.mask);
          f = wide;
        }
        else
        {
          int32_t narrow;
          in_range = normalize_value(__uint_as_float(raw), a.factor, narrow, a.lo, a.hi, (uint32_t)a.mask);
          f = (uint32_t)narrow;
        }
        DG_MATERIALISE(f);
      }
      else
        f = (F)v[u][e] & (F)a.mask;
      const bool counts = t < n[e];
      bad[e] = bad[e] || (counts && !in_range);
      tile[j + e][i_first + u * (4 * RPW)] = counts ? f : (F)0;
    }
  }
#pragma unroll
  for (uint32_t e = 0; e < VL; e++)
    if (bad[e])
      a.err[c + e] = ERR_INVALID_VALUE;
}

// The tile's words, numbered channel by channel, dealt to the lanes in turn: word index e = 256 u + thread, channel
// e / run, word e % run -- kept by steps of 256 / run and 256 % run instead of a division per word.
struct AxdrDeal
{
  uint32_t j, w, run, dq, dr;
  DG_DEV AxdrDeal(uint32_t thread, uint32_t run_) : run(run_)
  {
    j = thread / run;
    w = thread - j * run;
    dq = AX_BLOCK / run;
    dr = AX_BLOCK - dq * run;
  }
  DG_DEV bool live() const
  {
    return j < AX_CH;
  }
  DG_DEV void next()
  {
    w += dr;
    j += dq;
    if (w >= run)
    {
      w -= run;
      j++;
    }
  }
};

// Fields in LDS -> the words of the channels' runs.  PLAIN: every word of the tile exists (no count, the streams fit, the
// tile lies inside the region).
template <bool W64, bool PLAIN, typename F>
static DG_DEV void ax_drain(const AxdrPackArgs &a, const F (&tile)[AX_CH][ax_rows(W64) + 1], const uint32_t (&lim_of)[AX_CH], size_t t0, size_t c0,
                            uint32_t thread)
{
  constexpr uint32_t R = ax_rows(W64);
  const uint32_t run = (R / 32u) * a.vs;
  const uint64_t word0 = (uint64_t)(t0 / 32u) * a.vs;
  for (AxdrDeal d(thread, run); d.live(); d.next())
  {
    if (!PLAIN && d.w >= lim_of[d.j])
      continue;
    const uint32_t word = ax_gather<F>(tile[d.j], d.w, a.vs, a.vs_magic);
    uint8_t *const slab = a.out + (uint64_t)(c0 + d.j) * a.cap;
    reinterpret_cast<uint32_t *>(slab)[word0 + d.w] = bswap32(word);
  }
}

// KIND: AX_F32, AX_I32 or AX_I64; W64: value size 33..64 (fields of 8 bytes in LDS, tiles of 64 rows); VL: elements per
// lane and load, 1 or 16 / sizeof(element) -- with VL > 1 x is 16-byte aligned and ld a multiple of VL (the host checks).
template <uint32_t KIND, bool W64, uint32_t VL>
__global__ void __launch_bounds__(256) dega_axdr_pack_kernel(const AxdrPackArgs a)
{
  typedef std::conditional_t<W64, uint64_t, uint32_t> F;
  constexpr uint32_t R = ax_rows(W64);
  __shared__ F tile[AX_CH][R + 1];
  __shared__ uint32_t lim_of[AX_CH];
  const uint64_t q = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (q >= a.tiles) // (the whole workgroup: nobody is left waiting at the barrier)
    return;
  const size_t t0 = (size_t)(q / a.tiles_c) * R, c0 = (size_t)(q % a.tiles_c) * AX_CH;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const bool full = t0 + R <= a.T && c0 + AX_CH <= a.C;
  const bool plain = full && a.count == nullptr && a.fits_T != 0u;
  if (!plain && threadIdx.x < AX_CH) // the channels' lengths, and what the tile of their first rows says about them
  {
    const size_t c = c0 + threadIdx.x;
    uint32_t lim = 0;
    if (c < a.C)
    {
      int32_t status;
      const uint32_t n = ax_pack_rows(a, c, status);
      lim = ax_run_words(ax_words(n, a.vs), (uint64_t)(t0 / 32u) * a.vs, (R / 32u) * a.vs);
      if (t0 == 0)
      {
        a.out_bits[c] = (uint64_t)n * a.vs;
        if (status != OK)
          a.err[c] = status;
      }
    }
    lim_of[threadIdx.x] = lim;
  }
  if (plain && t0 == 0 && threadIdx.x < AX_CH)
    a.out_bits[c0 + threadIdx.x] = (uint64_t)a.T * a.vs;
  if (full)
    ax_stage<KIND, W64, VL, true, F>(a, tile, t0, c0, lane, wave);
  else
    ax_stage<KIND, W64, VL, false, F>(a, tile, t0, c0, lane, wave);
  __syncthreads();
  if (plain)
    ax_drain<W64, true, F>(a, tile, lim_of, t0, c0, threadIdx.x);
  else
    ax_drain<W64, false, F>(a, tile, lim_of, t0, c0, threadIdx.x);
}

// Field (channel, row i of the tile) from the channel's words in LDS
template <bool W64>
static DG_DEV uint64_t ax_extract(const uint32_t *words, uint32_t i, uint32_t vs, uint64_t mask)
{
  const uint32_t p = i * vs, wi = p >> 5, end = (p & 31u) + vs; // the field ends `end` bits into word wi
  const uint64_t top = ((uint64_t)words[wi] << 32) | words[wi + 1];
  if constexpr (!W64)
    return (top >> (64u - end)) & mask; // (end in 1 .. 63)
  else
  {
    if (end <= 64u) // (end in 33 .. 95)
      return (top >> (64u - end)) & mask;
    return ((top << (end - 64u)) | (words[wi + 2] >> (96u - end))) & mask;
  }
}

// KIND, W64: as the pack kernel's; VS: elements per lane and store, 1 or 16 / sizeof(element) -- with VS > 1 x is 16-byte
// aligned and ld a multiple of VS (the host checks).
template <uint32_t KIND, bool W64, uint32_t VS>
__global__ void __launch_bounds__(256) dega_axdr_unpack_kernel(const AxdrUnpackArgs a)
{
  typedef std::conditional_t<KIND == AX_F32, float, std::conditional_t<KIND == AX_I64, uint64_t, uint32_t>> E;
  constexpr uint32_t R = ax_rows(W64);
  __shared__ uint32_t words[AX_CH][AX_UNPACK_PITCH];
  __shared__ uint32_t n_of[AX_CH];
  const uint64_t q = (uint64_t)blockIdx.y * gridDim.x + blockIdx.x;
  if (q >= a.tiles)
    return;
  const size_t t0 = (size_t)(q / a.tiles_c) * R, c0 = (size_t)(q % a.tiles_c) * AX_CH;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x < AX_CH) // the channels' counts, and what the tile of their first rows says about them
  {
    const size_t c = c0 + threadIdx.x;
    uint32_t n = 0;
    if (c < a.C)
    {
      int32_t status;
      uint64_t count;
      n = ax_unpack_rows(a, c, status, count);
      if (t0 == 0)
      {
        a.out_count[c] = count;
        a.err[c] = status;
      }
    }
    n_of[threadIdx.x] = n;
  }
  // ---- the channels' runs -> LDS, consecutive lanes along a run; as far as the slab reaches ---------------------------
  {
    const uint32_t run = (R / 32u) * a.vs;
    const uint64_t word0 = (uint64_t)(t0 / 32u) * a.vs, slab_words = a.cap / 4u;
    constexpr uint32_t BATCH = 8;
    for (AxdrDeal d(threadIdx.x, run); d.live();)
    {
      uint32_t v[BATCH], at[BATCH];
      AxdrDeal ahead = d;
#pragma unroll
      for (uint32_t k = 0; k < BATCH; k++)
      {
        v[k] = 0;
        at[k] = 0xFFFFFFFFu;
        if (ahead.live())
        {
          at[k] = ahead.j * AX_UNPACK_PITCH + ahead.w;
          if (c0 + ahead.j < a.C && word0 + ahead.w < slab_words)
            v[k] = reinterpret_cast<const uint32_t *>(a.in + (uint64_t)(c0 + ahead.j) * a.cap)[word0 + ahead.w];
          ahead.next();
        }
      }
#pragma unroll
      for (uint32_t k = 0; k < BATCH; k++)
        if (at[k] != 0xFFFFFFFFu)
          (&words[0][0])[at[k]] = bswap32(v[k]);
      d = ahead;
    }
  }
  __syncthreads();
  // ---- fields -> rows.  A lane owns channels j .. j + VS - 1 of the tile rows i_first + 4 RPW u -------------------------
  constexpr uint32_t LPR = AX_CH / VS;
  constexpr uint32_t RPW = 64 / LPR;
  constexpr uint32_t STEPS = R / (4 * RPW);
  const uint32_t j = (lane % LPR) * VS, i_first = wave * RPW + lane / LPR;
  E *const p_first = static_cast<E *>(a.x) + (t0 + i_first) * a.ld + c0 + j;
  const size_t step = (size_t)(4 * RPW) * a.ld;
  uint32_t n[VS], n_min = 0xFFFFFFFFu;
#pragma unroll
  for (uint32_t e = 0; e < VS; e++)
  {
    n[e] = n_of[j + e];
    n_min = n[e] < n_min ? n[e] : n_min;
  }
  const uint32_t sh32 = 32u - (W64 ? 32u : a.vs), sh64 = 64u - a.vs;
#pragma unroll 4
  for (uint32_t u = 0; u < STEPS; u++)
  {
    const uint32_t i = i_first + u * (4 * RPW);
    const size_t t = t0 + i;
    E v[VS];
#pragma unroll
    for (uint32_t e = 0; e < VS; e++)
    {
      const uint64_t field = ax_extract<W64>(words[j + e], i, a.vs, a.mask);
      if constexpr (KIND == AX_F32 && W64)
        v[e] = denormalize_value((float)((int64_t)(field << sh64) >> sh64), a.factor);
      else if constexpr (KIND == AX_F32)
        v[e] = denormalize_value((float)((int32_t)((uint32_t)field << sh32) >> sh32), a.factor);
      else
        v[e] = (E)field;
    }
    E *const p = p_first + u * step;
    if (VS > 1 && t < n_min)
      tr_store<E, VS>(p, v);
    else
      for (uint32_t e = 0; e < VS; e++)
        if (t < n[e])
          p[e] = v[e];
  }
}

// ---- host side: how the kernels are launched (dega_launch.hpp) -----------------------------------------------------------------
struct AxdrVariant
{
  uint32_t kind; // AX_F32, AX_I32, AX_I64
  bool w64;      // value size 33..64
  bool wide;     // 16-byte loads (pack) / stores (unpack) on the rows' side
};

// `kind` and the value size as the caller gave them (launch() refuses pairs that do not go together); 16-byte accesses on
// rows whose every start lies on a 16-byte boundary, as transpose_variant decides it
inline AxdrVariant axdr_variant(uint32_t kind, int valuesize, const void *x_tc, size_t ld)
{
  const size_t V = 16 / (kind == AX_I64 ? 8 : 4);
  return AxdrVariant{kind, valuesize > 32, ((uintptr_t)x_tc & 15u) == 0 && ld % V == 0};
}

inline bool axdr_goes_together(const AxdrVariant &v, uint32_t vs)
{
  return vs >= 1 && vs <= 64 && v.w64 == (vs > 32) && (v.kind == AX_F32 || (v.kind == AX_I32 && !v.w64) || (v.kind == AX_I64 && v.w64));
}

inline uint64_t axdr_mask(int valuesize)
{
  return valuesize >= 64 ? ~(uint64_t)0 : (((uint64_t)1 << valuesize) - 1u);
}

// The tiles are launch()'s to fill in.
inline AxdrPackArgs axdr_pack_args(const void *x_tc, size_t C, size_t T, size_t ld, const uint64_t *count, float factor, int valuesize, uint8_t *out,
                                   size_t cap, uint64_t *out_bits, int32_t *err)
{
  AxdrPackArgs a;
  a.x = x_tc;
  a.C = C;
  a.T = T;
  a.ld = ld;
  a.count = count;
  a.out = out;
  a.cap = cap;
  a.out_bits = out_bits;
  a.err = err;
  a.vs = (uint32_t)valuesize;
  a.vs_magic = valuesize >= 2 ? (uint32_t)((((uint64_t)1 << 32) + (uint64_t)valuesize - 1u) / (uint64_t)valuesize) : 0u;
  a.factor = factor;
  // the bounds of normalize.c:21, rounded to float by the host compiler exactly as the reference's are
  a.lo = -(float)((uint64_t)1 << (valuesize - 1));
  a.hi = (float)(((uint64_t)1 << (valuesize - 1)) - 1);
  a.mask = axdr_mask(valuesize);
  a.fits_T = (((uint64_t)T * a.vs + 31u) >> 5) * 4u <= cap ? 1u : 0u;
  a.tiles_c = a.tiles = 0;
  return a;
}

inline AxdrUnpackArgs axdr_unpack_args(const uint8_t *in, size_t cap, const uint64_t *in_bits, size_t C, size_t max_T, size_t ld, float factor, int valuesize,
                                       void *x_tc, uint64_t *out_count, int32_t *err)
{
  AxdrUnpackArgs a;
  a.in = in;
  a.cap = cap;
  a.in_bits = in_bits;
  a.C = C;
  a.max_T = max_T;
  a.ld = ld;
  a.x = x_tc;
  a.out_count = out_count;
  a.err = err;
  a.vs = (uint32_t)valuesize;
  a.factor = factor;
  a.mask = axdr_mask(valuesize);
  a.tiles_c = a.tiles = 0;
  return a;
}

// The tiles of C channels x T rows and the grid that numbers them, as tr_plan does; a channel has a tile of first rows
// even where T is 0 (it carries the channel's bits / count and status).  False when gridDim.y cannot hold them.
inline bool ax_plan(size_t C, size_t T, uint32_t R, uint64_t gx_max, uint64_t &tiles_c, uint64_t &tiles, LaunchGrid &grid)
{
  const uint64_t tiles_r = T == 0 ? 1u : ((uint64_t)T + R - 1) / R;
  tiles_c = ((uint64_t)C + AX_CH - 1) / AX_CH;
  if (tiles_c != 0 && tiles_r > ~(uint64_t)0 / tiles_c)
    return false;
  tiles = tiles_r * tiles_c;
  const uint64_t x = tiles < gx_max ? tiles : gx_max;
  const uint64_t y = x == 0 ? 0 : (tiles + x - 1) / x;
  if (y > 65535)
    return false;
  grid.x = (uint32_t)x;
  grid.y = (uint32_t)y;
  return true;
}

// `gx_max`: as tr_plan's.  Nothing is launched for C = 0.
template <typename L>
inline bool launch(const AxdrVariant &v, AxdrPackArgs a, uint64_t gx_max, L &&launch_one)
{
  LaunchGrid grid;
  if (!axdr_goes_together(v, a.vs) || a.T > AX_MAX_T || !ax_plan(a.C, a.T, ax_rows(v.w64), gx_max, a.tiles_c, a.tiles, grid))
    return false;
  if (a.tiles == 0)
    return true;
  with_bools(
      [&](auto wide) {
        constexpr bool W = decltype(wide)::value;
        if (v.kind == AX_F32 && v.w64)
          launch_one(dega_axdr_pack_kernel<AX_F32, true, W ? 4 : 1>, grid, AX_BLOCK, a);
        else if (v.kind == AX_F32)
          launch_one(dega_axdr_pack_kernel<AX_F32, false, W ? 4 : 1>, grid, AX_BLOCK, a);
        else if (v.kind == AX_I32)
          launch_one(dega_axdr_pack_kernel<AX_I32, false, W ? 4 : 1>, grid, AX_BLOCK, a);
        else
          launch_one(dega_axdr_pack_kernel<AX_I64, true, W ? 2 : 1>, grid, AX_BLOCK, a);
      },
      v.wide);
  return true;
}

template <typename L>
inline bool launch(const AxdrVariant &v, AxdrUnpackArgs a, uint64_t gx_max, L &&launch_one)
{
  LaunchGrid grid;
  if (!axdr_goes_together(v, a.vs) || a.max_T > AX_MAX_T || !ax_plan(a.C, a.max_T, ax_rows(v.w64), gx_max, a.tiles_c, a.tiles, grid))
    return false;
  if (a.tiles == 0)
    return true;
  with_bools(
      [&](auto wide) {
        constexpr bool W = decltype(wide)::value;
        if (v.kind == AX_F32 && v.w64)
          launch_one(dega_axdr_unpack_kernel<AX_F32, true, W ? 4 : 1>, grid, AX_BLOCK, a);
        else if (v.kind == AX_F32)
          launch_one(dega_axdr_unpack_kernel<AX_F32, false, W ? 4 : 1>, grid, AX_BLOCK, a);
        else if (v.kind == AX_I32)
          launch_one(dega_axdr_unpack_kernel<AX_I32, false, W ? 4 : 1>, grid, AX_BLOCK, a);
        else
          launch_one(dega_axdr_unpack_kernel<AX_I64, true, W ? 2 : 1>, grid, AX_BLOCK, a);
      },
      v.wide);
  return true;
}

} // namespace dg
