// csv_kernels.hpp -- the reference's `encode csv` stage (WriteCSV, DCLib/src/csv.c:46-65) for gfx950 (MI355X).
//
// float32 [T][ld] -> per channel the text the reference writes: for every reading `column - 1` copies of separator_char
// (csv.c:56-59), then sprintf("%.*f\n", num_decimal_places, value) (csv.c:60) -- byte for byte what glibc prints, in the
// layout dega_hip_lzmh_encode_dev takes as it is (uint8 [C][stride], 16-byte aligned, stride a multiple of 16).
//
// The formatting is INTEGER ONLY.  A float is m x 2^e exactly (m < 2^24); printf rounds that exact value half-to-even to
// d <= 6 decimals.  With s = -e > 0:  the integer part is m >> s, the fraction's numerator f = m mod 2^s, and
// F = f x 10^d < 2^44 scaled by 2^-s gives the decimals: F >> s, rounded up when the bits shifted out are above half, or
// exactly half with an odd last digit (the last digit of the whole scaled value: of the integer part when d = 0); a
// shift of 45 or more leaves nothing (F < 2^44).  A carry out of the decimals goes into the integer part.  For e >= 0
// the value is the integer m << e and the decimals are zeros; from 10^8 on (e > 2: up to 2^128, 39 digits) it is
// converted limb by limb, eight digits per division of the four 32-bit limbs by 10^8 -- a rare branch.  The sign is the
// sign BIT (-0.0f prints -0.00, a NaN with the bit set -nan), infinities and NaNs print inf / nan without decimals.
// No float or double arithmetic anywhere: one rounding and a tie goes the wrong way.
//
// Mapping: one lane = one channel, like every serial kernel here -- where a line starts depends on the lengths of all
// lines before it.  A wave's row read is one 256-byte segment.
//   in   CSV_DEPTH rows ahead: the wave's next CSV_DEPTH rows are on their way from HBM straight into LDS (LDS-DMA, no
//        register waits for them) while the lane formats the CSV_DEPTH rows before them out of the other half of the
//        buffer, so the loop never waits for device memory and stays rolled (the formatting is ~150 instructions).
//   out  bytes collect in a 64-bit register.  CsvStore8: every full register is one 8-byte store (64 lanes, 64 rows), as
//        lzmh_render_kernel does.  CsvStore64: full registers are staged in the lane's LDS column and leave as four
//        16-byte stores, one whole 64-byte block of the row.  Measured, the first is faster (63.7 against 73.6 ms at
//        64 Ki channels x 86 400: the kernel is bound by its instructions, not its stores) and is the
//        library's default; DEGA_CSV_STORE picks the other.
// A channel whose text does not fit -- text + CSV_SLACK bytes <= stride is what fits -- gets ERR_MEMORY and out_len 0;
// the others are unaffected.  Bytes of a row beyond out_len are unspecified.
//
// This header is compiled by hipcc (dega_hip.hip) and, for offline checking only, by g++ under tests/sim/.
#pragma once

#include "dega_intrinsics.hpp"
#include "dega_launch.hpp"

#include <stddef.h>

namespace dg
{

constexpr uint32_t CSV_BLOCK = 256;        // lanes = adjacent channels per workgroup
constexpr uint32_t CSV_DEPTH = 16;         // rows in flight per lane (AGG_DEPTH of aggregate_kernels.hpp)
constexpr uint32_t CSV_SLACK = 16;         // room a row keeps behind its text: the last, partly filled 8-byte store
constexpr uint32_t CSV_MAX_DECIMALS = 6;   // num_decimal_places, DCLib/src/enc_dec.c:69
constexpr uint32_t CSV_STAGE_WORDS = 8;    // CsvStore64: 8-byte words staged per lane before they are stored (64 bytes)
constexpr int32_t CSV_OK = 0, CSV_ERR_MEMORY = -6; // DEGA_OK, DEGA_ERROR_MEMORY
constexpr int32_t CSV_ERR_INVALID_VALUE = -1;      // DEGA_ERROR_INVALID_VALUE

struct CsvArgs
{
  const float *v;        // [T][ld]
  size_t C, T, ld;
  uint32_t decimals;     // 0 .. 6
  uint32_t nsep;         // column - 1 separators in front of every value
  uint32_t sep;          // separator_char
  uint8_t *out;          // [C][stride], 16-byte aligned
  size_t stride;         // a multiple of 16, at most 0x7FFFFFF0
  uint64_t *out_len;     // [C]
  int32_t *err;          // [C]
  const uint64_t *count = nullptr; // the counted variant (VAR): channel c is rows 0 .. count[c] - 1 of its column
};

DG_DEV uint32_t csv_div10(uint32_t n) // exact for every 32-bit n
{
  return mulhi32(n, 0xCCCCCCCDu) >> 3;
}

// the decimal digits of n as ASCII, first digit in the lowest byte; returns how many (at least one)
DG_DEV uint32_t csv_digits(uint32_t n, uint64_t &text)
{
  uint32_t count = 0;
  text = 0;
  do
  {
    const uint32_t q = csv_div10(n);
    text = (text << 8) | (uint64_t)(0x30u + n - 10u * q);
    n = q;
    count++;
  } while (n != 0);
  return count;
}

// exactly `count` <= 8 digits of n, leading zeros included
DG_DEV uint64_t csv_digits_fixed(uint32_t n, uint32_t count)
{
  uint64_t text = 0;
  for (uint32_t k = 0; k < count; k++)
  {
    const uint32_t q = csv_div10(n);
    text = (text << 8) | (uint64_t)(0x30u + n - 10u * q);
    n = q;
  }
  return text;
}

// ---- where finished 8-byte words go ----------------------------------------------------------------------------------
struct CsvStore8 // straight to the row
{
  static constexpr uint32_t LDS_WORDS = 1; // (unused)
  uint8_t *dst;
  uint32_t pos; // bytes stored
  DG_DEV void init(uint8_t *row, uint64_t *) { dst = row; pos = 0; }
  DG_DEV uint32_t written() const { return pos; }
  DG_DEV void word(uint64_t w)
  {
    *reinterpret_cast<uint64_t *>(dst + pos) = w;
    pos += 8;
  }
  DG_DEV void finish() {}
};

struct CsvStore64 // CSV_STAGE_WORDS words in the lane's LDS column, then four 16-byte stores: one 64-byte block of the row
{
  static constexpr uint32_t LDS_WORDS = CSV_STAGE_WORDS * CSV_BLOCK;
  uint8_t *dst;
  uint64_t *stage; // word k of this lane: stage[k * CSV_BLOCK]
  uint32_t pos, staged;
  DG_DEV void init(uint8_t *row, uint64_t *lds_column) { dst = row; stage = lds_column; pos = 0; staged = 0; }
  DG_DEV uint32_t written() const { return pos + 8u * staged; }
  DG_DEV void word(uint64_t w)
  {
    stage[staged * CSV_BLOCK] = w;
    if (++staged == CSV_STAGE_WORDS)
    {
#pragma unroll
      for (uint32_t k = 0; k < CSV_STAGE_WORDS; k += 2)
      {
        const uint64_t a = stage[k * CSV_BLOCK], b = stage[(k + 1u) * CSV_BLOCK];
        store_x4(reinterpret_cast<uint32_t *>(dst + pos + 8u * k), (uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
      }
      pos += 8u * CSV_STAGE_WORDS;
      staged = 0;
    }
  }
  DG_DEV void finish() // what is staged when the series ends
  {
    for (uint32_t k = 0; k < staged; k++)
      *reinterpret_cast<uint64_t *>(dst + pos + 8u * k) = stage[k * CSV_BLOCK];
    pos += 8u * staged;
    staged = 0;
  }
};

// One channel's text in the making: up to 7 pending bytes in acc (first byte lowest), whole words behind it in S.
template <typename S>
struct CsvWriter
{
  S store;
  uint64_t acc;
  uint32_t nacc;
  DG_DEV uint32_t length() const { return store.written() + nacc; }
  DG_DEV void put(uint64_t text, uint32_t n) // n <= 8 bytes, the bytes of text above them zero
  {
    acc |= text << (8u * nacc);
    uint32_t total = nacc + n;
    if (total >= 8u)
    {
      store.word(acc);
      acc = (text >> (63u - 8u * nacc)) >> 1; // the bytes that did not fit (nacc = 0: none, a shift by 64 in two steps)
      total -= 8u;
    }
    nacc = total;
  }
};

constexpr uint32_t CSV_POW10[CSV_MAX_DECIMALS + 1] = {1u, 10u, 100u, 1000u, 10000u, 100000u, 1000000u};

// V: CsvStore8 or CsvStore64.
// VAR: a ragged batch.  A lane's text ends with its own count[c]-th reading; rows are fetched up to the largest count of
// the wave, and what lies at or beyond a lane's count (NaN, infinities, anything) is formatted like any row -- the lanes
// stay in step -- but never written nor counted against the row's room.  count[c] > T: CSV_ERR_INVALID_VALUE, no text.
template <typename V, bool VAR = false>
__global__ void __launch_bounds__(256) dega_csv_kernel(const CsvArgs a)
{
  // rows on their way: [half][row][lane], a wave's row is 64 consecutive dwords (what one LDS-DMA load fills)
  __shared__ uint32_t rows[2 * CSV_DEPTH * CSV_BLOCK];
  __shared__ uint64_t staged[V::LDS_WORDS];
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave0 = wave_uniform(threadIdx.x & ~63u); // the wave's first lane of the workgroup
  const size_t c = (size_t)blockIdx.x * CSV_BLOCK + threadIdx.x;
  const bool live = c < a.C;
  const float *const src = a.v + (live ? c : a.C - 1); // (a lane without a channel reads the last one's: a valid address)
  const uint32_t stride = (uint32_t)a.stride;
  const uint32_t d = a.decimals, p10 = CSV_POW10[d];
  // separators: whole words of eight, the rest in front of the sign in one word
  const uint64_t sep8 = (uint64_t)(a.sep & 0xFFu) * 0x0101010101010101ull;
  const uint32_t sep_words = a.nsep >> 3, sep_rest = a.nsep & 7u;
  const uint64_t sep_text = sep_rest != 0 ? sep8 >> (64u - 8u * sep_rest) : 0ull;
  const uint32_t tail_len = d != 0 ? d + 2u : 1u; // '.' + decimals + '\n', or the '\n' alone

  CsvWriter<V> w;
  w.store.init(a.out + (live ? c : 0) * a.stride, staged + threadIdx.x);
  w.acc = 0;
  w.nacc = 0;
  bool ok = live;
  // the lane's end and the wave's: both a.T in the uniform form (T_end is a constant copy of it there)
  uint32_t mine = 0;
  bool over = false;
  if constexpr (VAR)
  {
    const uint64_t n = live ? a.count[c] : 0u;
    over = n > a.T;
    mine = over ? 0u : (uint32_t)n; // (the host refuses T >= 2^32 in the counted form)
  }
  const size_t T_end = VAR ? (size_t)wave_uniform(wave_max_u32(mine)) : a.T;

  auto fetch = [&](size_t t0, uint32_t half) { // rows t0 .. t0 + CSV_DEPTH - 1 (clamped to the series) into `half`
    wait_lds(); // what was read out of this half is out of it
#pragma unroll
    for (uint32_t u = 0; u < CSV_DEPTH; u++)
    {
      const size_t t = t0 + u < a.T ? t0 + u : a.T - 1;
      dma_row_to_lds(reinterpret_cast<const int32_t *>(src + t * a.ld), rows + (half * CSV_DEPTH + u) * CSV_BLOCK + wave0, lane);
    }
  };

  if (T_end != 0)
    fetch(0, 0);
  uint32_t half = 0;
  for (size_t t0 = 0; t0 < T_end; t0 += CSV_DEPTH, half ^= 1u)
  {
    wait_vector_memory(); // this batch has landed (asked for one batch ago)
    if (t0 + CSV_DEPTH < T_end)
      fetch(t0 + CSV_DEPTH, half ^ 1u);
    const uint32_t n_rows = T_end - t0 < CSV_DEPTH ? (uint32_t)(T_end - t0) : CSV_DEPTH;
    for (uint32_t u = 0; u < n_rows; u++)
    {
      const bool has = VAR ? (uint32_t)t0 + u < mine : true; // the row is one of this lane's readings
      const uint32_t bits = peer_load(rows + (half * CSV_DEPTH + u) * CSV_BLOCK + threadIdx.x);
      const uint32_t sign = bits >> 31, E = (bits >> 23) & 0xFFu, M = bits & 0x7FFFFFu;
      const uint32_t m = E != 0 ? M | 0x800000u : M; // the value is m x 2^e
      const int32_t e = (int32_t)(E != 0 ? E : 1u) - 150;
      const bool special = E == 0xFFu, big = !special && e > 2; // big: an integer of 2^26 or more

      // ---- the common case: integer part below 10^8, the decimals rounded half-to-even on the exact value ----
      uint32_t ip = 0, fq = 0;
      if (e >= 0)
        ip = big || special ? 0u : m << e;
      else
      {
        const uint32_t s = (uint32_t)(-e); // 1 .. 149
        const uint32_t f = s < 24u ? m & ((1u << s) - 1u) : m;
        ip = s < 24u ? m >> s : 0u;
        if (s <= 44u) // (beyond: F < 2^44 is below half of 2^s)
        {
          const uint64_t F = (uint64_t)f * p10;
          const uint64_t rem = F & ((1ull << s) - 1ull), half_ulp = 1ull << (s - 1u);
          fq = (uint32_t)(F >> s);
          const uint32_t last = d != 0 ? fq : ip; // the last digit printed
          fq += (rem > half_ulp || (rem == half_ulp && (last & 1u) != 0)) ? 1u : 0u;
          if (fq == p10) // carried out of the decimals
          {
            fq = 0;
            ip++;
          }
        }
      }
      uint64_t int_text;
      uint32_t int_len = csv_digits(ip, int_text);
      if (special)
      {
        int_text = M != 0 ? 0x6E616Eull : 0x666E69ull; // "nan" : "inf"
        int_len = 3;
      }
      uint64_t tail = 0x0Aull;
      if (d != 0 && !special)
        tail = 0x2Eull | (csv_digits_fixed(fq, d) << 8) | (0x0Aull << (8u * (d + 1u)));
      const uint32_t this_tail = special ? 1u : tail_len;

      // ---- the rare case: 10^8 .. 2^128 as eight-digit groups, lowest first, from the four limbs of m << e ----
      uint32_t g0 = 0, g1 = 0, g2 = 0, g3 = 0, g4 = 0, top = 0;
      if (big)
      {
        const uint32_t ws = (uint32_t)e >> 5, bs = (uint32_t)e & 31u;
        const uint64_t mm = (uint64_t)m << bs;
        uint32_t limb[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; i++)
          limb[i] = (i == ws ? (uint32_t)mm : 0u) | (i == ws + 1u ? (uint32_t)(mm >> 32) : 0u);
        uint32_t g[5];
#pragma unroll
        for (uint32_t k = 0; k < 5; k++)
        {
          uint64_t r = 0;
#pragma unroll
          for (uint32_t i = 4; i-- > 0;)
          {
            const uint64_t cur = (r << 32) | limb[i];
            limb[i] = (uint32_t)(cur / 100000000u);
            r = cur % 100000000u;
          }
          g[k] = (uint32_t)r;
        }
        g0 = g[0], g1 = g[1], g2 = g[2], g3 = g[3], g4 = g[4];
        top = g4 != 0 ? 4u : (g3 != 0 ? 3u : (g2 != 0 ? 2u : (g1 != 0 ? 1u : 0u)));
        const uint32_t gt = top == 4u ? g4 : (top == 3u ? g3 : (top == 2u ? g2 : (top == 1u ? g1 : g0)));
        int_len = csv_digits(gt, int_text);
      }

      // ---- does the line fit?  (length() + CSV_SLACK <= stride holds before every line) ----
      const uint32_t line = a.nsep + sign + int_len + 8u * top + this_tail;
      if (ok && has && line > stride - CSV_SLACK - w.length())
        ok = false;
      if (ok && has)
      {
        for (uint32_t k = 0; k < sep_words; k++)
          w.put(sep8, 8);
        if (sep_rest + sign != 0)
          w.put(sign != 0 ? sep_text | (0x2Dull << (8u * sep_rest)) : sep_text, sep_rest + sign);
        w.put(int_text, int_len);
        for (uint32_t k = top; k-- > 0;) // the groups below the first: eight digits each
          w.put(csv_digits_fixed(k == 3u ? g3 : (k == 2u ? g2 : (k == 1u ? g1 : g0)), 8), 8);
        w.put(tail, this_tail);
      }
    }
  }
  if (!live)
    return;
  uint64_t len = 0;
  if (ok)
  {
    w.store.finish();
    if (w.nacc != 0)
      *reinterpret_cast<uint64_t *>(w.store.dst + w.store.pos) = w.acc;
    len = (uint64_t)w.store.pos + w.nacc;
  }
  a.out_len[c] = VAR && over ? 0u : len;
  a.err[c] = VAR && over ? CSV_ERR_INVALID_VALUE : (ok ? CSV_OK : CSV_ERR_MEMORY);
}

// ---- host side: how the kernel is launched (dega_launch.hpp) ----------------------------------------------------------------
struct CsvVariant
{
  bool wide_stores; // the LDS-staged 64-byte store form, else the 8-byte form (same bytes either way)
  bool counted;     // a ragged batch: a count per channel
};

inline CsvVariant csv_variant(bool wide_stores, const uint64_t *count)
{
  return CsvVariant{wide_stores, count != nullptr};
}

inline CsvArgs csv_args(const float *v, size_t C, size_t T, size_t ld, unsigned decimals, size_t column, int separator_char, uint8_t *out, size_t stride,
                        uint64_t *out_len, int32_t *err, const uint64_t *count)
{
  CsvArgs a;
  a.v = v;
  a.C = C;
  a.T = T;
  a.ld = ld;
  a.decimals = decimals;
  a.nsep = (uint32_t)(column - 1);
  a.sep = (uint32_t)separator_char;
  a.out = out;
  a.stride = stride;
  a.out_len = out_len;
  a.err = err;
  a.count = count;
  return a;
}

template <typename L>
inline bool launch(const CsvVariant &v, const CsvArgs &a, L &&launch_one)
{
  const size_t gx = (a.C + CSV_BLOCK - 1) / CSV_BLOCK;
  if (gx > LAUNCH_MAX_GX || v.counted != (a.count != nullptr))
    return false;
  with_bools(
      [&](auto wide, auto counted) {
        launch_one(dega_csv_kernel<std::conditional_t<decltype(wide)::value, CsvStore64, CsvStore8>, decltype(counted)::value>, LaunchGrid{(uint32_t)gx, 1},
                   CSV_BLOCK, a);
      },
      v.wide_stores, v.counted);
  return true;
}

} // namespace dg
