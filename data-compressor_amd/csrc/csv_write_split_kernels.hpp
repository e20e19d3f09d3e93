// csv_write_split_kernels.hpp -- `encode csv` (WriteCSV, DCLib/src/csv.c:46-65) for few long channels: one channel's rows
// split over lanes.  For gfx950 (MI355X).
//
// The same input, output and results as csv_kernels.hpp: out_len[c], err[c] and bytes [0, out_len[c]) of every row.  What
// differs is the unit of parallelism.  There a lane is a channel, because where a line starts depends on the lengths of all
// lines before it.  Here a lane is a (channel, block of rows) pair: block b of channel c owns rows
// [b * R, min((b + 1) * R, n_c)), n_c being T or count[c].  A line depends on nothing but its own reading, so only the byte
// offset of a block is global to the channel.  Three launches on one stream settle it:
//   length  a lane per pair adds up the lengths of its lines into work[c][b], a 32-bit word that saturates at 2^31 - 1 (above
//           every legal stride).  No digit text: the digit count comes from the rounded integer part by comparisons.
//   scan    a workgroup per channel: the exclusive prefix over the channel's blocks in 64 bits, in place -- work[c][b]
//           becomes the block's byte offset, or CSVWS_NOTHING for every block of a channel that reports an error -- and
//           out_len[c] and err[c] as the unsplit kernel decides them: the text fits iff total + CSV_SLACK <= stride (the
//           unsplit kernel's test before every line is monotone in the length so far, so it fails at some line iff it
//           fails for the whole text), else CSV_ERR_MEMORY and length 0; count[c] > T is CSV_ERR_INVALID_VALUE and length 0.
//   write   the same walk with the digits: the lane's bytes go to [off, off + len) of the row.  Block edges fall at any
//           byte and no two lanes may store to the same byte, so the bytes in front of the lane's first 8-byte boundary and
//           behind its last one leave as 1-, 2- and 4-byte stores (csv_store_bytes), everything between as whole 8-byte
//           words; a block inside one word is narrow stores only.  No atomics; every byte of [0, out_len[c]) is written by
//           exactly one lane, NO BYTE AT OR BEYOND out_len[c] IS WRITTEN, and nothing at all for a channel with an error
//           (stricter than the unsplit kernel, which uses the CSV_SLACK bytes).  Not launched for T = 0.
// length and write are two instantiations of one walk over one formatter (csv_format<TEXT>), so they cannot disagree about
// a line.
//
// THE FORMATTER IS RESTATED HERE.  The per-reading arithmetic of dega_csv_kernel (mantissa and exponent, the half-to-even
// rounding on the exact value, the carry, inf / nan, the limb branch) was lifted into csv_format and called from that
// kernel; the gfx950 instruction streams of its instantiations then differed from the parent's (register allocation and 0.6
// to 1.5 % more instructions; profiles/csv_write_split_resource_usage.txt), so that kernel's body stays as it was and
// csv_format repeats its arithmetic line for line.  Both are held to the same fixture (tests/golden/csv.npz) and to the
// same Python formatting on the same random bit patterns; what they share by inclusion is csv_div10, csv_digits,
// csv_digits_fixed, CsvWriter and CSV_POW10.
//
// Mapping: a workgroup is a tile of cw adjacent channels x 256 / cw consecutive blocks, channels fastest; cw = 64 for
// C >= 64, else the smallest power of two >= C.  A single channel spreads over the device (adjacent lanes hold adjacent
// blocks), and from 64 channels on a wave reads whole 256-byte row segments like the unsplit kernel.  Plain loads, the next
// row asked for while this one is formatted, no LDS: occupancy hides the latency that the unsplit kernel's LDS-DMA double
// buffer has to hide alone (DESIGN.md 4.6.1 says what was measured).
//
// Reads: v[t][c] for t < n_c <= T, c < C only.  Writes: work[c][b]; out_len[c], err[c]; bytes [0, out_len[c]) of row c.
//
// This header is compiled by hipcc (dega_hip.hip) and, for offline checking only, by g++ under tests/sim/.
#pragma once

#include "csv_kernels.hpp"

namespace dg
{

constexpr uint32_t CSVWS_BLOCK = 256;            // lanes = (channel, block) pairs per workgroup of length and write
constexpr uint32_t CSVWS_SCAN_BLOCK = 256;       // lanes of the workgroup that scans one channel
constexpr uint32_t CSVWS_MAX_CW = 64;            // channels across a tile: one wave's 256-byte row segment
constexpr uint32_t CSVWS_SATURATED = 0x7FFFFFFFu; // work[c][b] after length: at least this many bytes
constexpr uint32_t CSVWS_NOTHING = 0xFFFFFFFFu;  // work[c][b] after scan: the block writes nothing

// dega_hip_csv_write_split_block_rows: the largest R that still gives the batch CSVWS_FILL_PAIRS (channel, block) pairs, not
// below CSVWS_FLOOR_ROWS.  Both from the sweep of tools/csvbench.py --split (the benchmark's two-decimal walk, 86 400 readings
// per channel, block_rows 1 .. 86 400; profiles/csv_write_split_bench.txt).  The floor: at 1 and at 16 channels, which never
// get to the pair count, the rows "block_rows 16" are the fastest (0.039 and 0.049 ms; 4 rows a block cost 0.062 and 0.076,
// 64 rows 0.083 and 0.092).  The pair count: at 4 096 channels the time is flat from 16 to 1 024 rows a block (5.13 .. 5.42
// ms; 4 rows 6.21, 4 096 rows 6.39), and 5 Mi pairs -- 67 rows there, 5.54 ms -- is where a first session, not in the profile,
// had that row's minimum (64 rows, 5.5 M pairs); the runs do not resolve it better than that.  At 65 536 channels the row
// of 64 is the fastest and more pairs than these would serve better, but there the unsplit kernel is the one to call.  At
// 256 channels the floor holds the block at 16 rows (0.344 ms), where the row of 4 measured 0.285 ms: a rule of this form
// cannot have both that and the single channel's 16.  DESIGN.md 4.6.1 has the table.
constexpr size_t CSVWS_FILL_PAIRS = (size_t)5 << 20;
constexpr size_t CSVWS_FLOOR_ROWS = 16;

struct CsvWriteSplitArgs
{
  CsvArgs a;            // what the unsplit kernel takes (count null: the uniform form)
  uint64_t block_rows;  // R: 1 .. max(1, T)
  uint32_t blocks;      // per channel: ceil(T / R), at least 1
  uint32_t cw_log2;     // the tile is 2^cw_log2 channels x (CSVWS_BLOCK >> cw_log2) blocks
  uint32_t tiles_c;     // tiles across the channels; blockIdx.x = tile_b * tiles_c + tile_c
  uint32_t *work;       // [C][blocks]
};

// Pure host code: the library's choice of block_rows; 0 for a T the counted form refuses.
inline size_t csv_write_split_block_rows(size_t C, size_t T)
{
  if (T > 0xFFFFFFFFu)
    return 0;
  const size_t rows = T != 0 ? T : 1;
  const size_t floor_rows = CSVWS_FLOOR_ROWS < rows ? CSVWS_FLOOR_ROWS : rows;
  const size_t need = C == 0 ? CSVWS_FILL_PAIRS : (CSVWS_FILL_PAIRS + C - 1) / C; // blocks per channel that fill the device
  if (need <= 1)
    return rows;
  // ceil(rows / R) >= need  <=>  R <= (rows - 1) / (need - 1)
  const size_t most = (rows - 1) / (need - 1);
  return most < floor_rows ? floor_rows : (most > rows ? rows : most);
}

// how many decimal digits n has (at least one), by comparisons: what csv_digits returns, without the digits
DG_DEV uint32_t csv_digit_count(uint32_t n)
{
  return n < 10000u ? (n < 100u ? (n < 10u ? 1u : 2u) : (n < 1000u ? 3u : 4u))
                    : (n < 100000000u ? (n < 1000000u ? (n < 100000u ? 5u : 6u) : (n < 10000000u ? 7u : 8u)) : (n < 1000000000u ? 9u : 10u));
}

// One reading as its line, without the separators in front: '-' when sign is set, the int_len <= 8 characters of int_text
// (the digits in front of the first eight-digit group, or "inf" / "nan"), `top` groups of eight digits (g3 .. g0, the
// highest first: the rare 10^8 .. 2^128 case), then the tail_len <= 8 characters of tail ('.', the decimals and '\n').
struct CsvLine
{
  uint32_t sign, int_len, top, tail_len;
  uint64_t int_text, tail; // (TEXT only)
  uint32_t g0, g1, g2, g3; // (TEXT only) the groups below the first, lowest first
  DG_DEV uint32_t length() const { return sign + int_len + 8u * top + tail_len; }
};

// The arithmetic of the stage (the top of csv_kernels.hpp), as in dega_csv_kernel: bits is the float32,
// d = num_decimal_places, p10 = 10^d.  TEXT: the digit text as well; without it only the lengths, the digit count by
// comparisons on the same rounded integer part and the same top group.
template <bool TEXT>
DG_DEV CsvLine csv_format(uint32_t bits, uint32_t d, uint32_t p10)
{
  const uint32_t tail_len = d != 0 ? d + 2u : 1u; // '.' + decimals + '\n', or the '\n' alone
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
  CsvLine l;
  l.sign = sign;
  l.int_text = 0;
  l.int_len = TEXT ? csv_digits(ip, l.int_text) : csv_digit_count(ip);
  if (special)
  {
    l.int_text = M != 0 ? 0x6E616Eull : 0x666E69ull; // "nan" : "inf"
    l.int_len = 3;
  }
  l.tail = 0x0Aull;
  if (TEXT && d != 0 && !special)
    l.tail = 0x2Eull | (csv_digits_fixed(fq, d) << 8) | (0x0Aull << (8u * (d + 1u)));
  l.tail_len = special ? 1u : tail_len;

  // ---- the rare case: 10^8 .. 2^128 as eight-digit groups, lowest first, from the four limbs of m << e ----
  l.g0 = l.g1 = l.g2 = l.g3 = 0;
  l.top = 0;
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
    l.g0 = g[0], l.g1 = g[1], l.g2 = g[2], l.g3 = g[3];
    l.top = g[4] != 0 ? 4u : (g[3] != 0 ? 3u : (g[2] != 0 ? 2u : (g[1] != 0 ? 1u : 0u)));
    const uint32_t gt = l.top == 4u ? g[4] : (l.top == 3u ? g[3] : (l.top == 2u ? g[2] : (l.top == 1u ? g[1] : g[0])));
    l.int_len = TEXT ? csv_digits(gt, l.int_text) : csv_digit_count(gt);
  }
  return l;
}

// the column - 1 separators in front of every value: whole words of eight, the rest in front of the sign in one word
struct CsvSeparators
{
  uint64_t sep8, sep_text;
  uint32_t sep_words, sep_rest;
  DG_DEV CsvSeparators(uint32_t sep, uint32_t nsep)
  {
    sep8 = (uint64_t)(sep & 0xFFu) * 0x0101010101010101ull;
    sep_words = nsep >> 3;
    sep_rest = nsep & 7u;
    sep_text = sep_rest != 0 ? sep8 >> (64u - 8u * sep_rest) : 0ull;
  }
};

// the line of one reading into w (a CsvWriter): separators, sign, integer part, groups, tail -- as dega_csv_kernel puts them
template <typename W>
DG_DEV void csv_put_line(W &w, const CsvLine &f, const CsvSeparators &s)
{
  for (uint32_t k = 0; k < s.sep_words; k++)
    w.put(s.sep8, 8);
  if (s.sep_rest + f.sign != 0)
    w.put(f.sign != 0 ? s.sep_text | (0x2Dull << (8u * s.sep_rest)) : s.sep_text, s.sep_rest + f.sign);
  w.put(f.int_text, f.int_len);
  for (uint32_t k = f.top; k-- > 0;) // the groups below the first: eight digits each
    w.put(csv_digits_fixed(k == 3u ? f.g3 : (k == 2u ? f.g2 : (k == 1u ? f.g1 : f.g0)), 8), 8);
  w.put(f.tail, f.tail_len);
}

// Bytes lo .. hi - 1 (0 <= lo, hi <= 8) of the 8-byte word w to the 8-byte aligned address word8, and no other byte: at most
// one store each of 1, 2, 4, 2 and 1 bytes, every one aligned to its size.
DG_DEV void csv_store_bytes(uint8_t *word8, uint64_t w, uint32_t lo, uint32_t hi)
{
  uint32_t p = lo;
  if ((p & 1u) != 0 && p < hi)
  {
    word8[p] = (uint8_t)(w >> (8u * p));
    p += 1u;
  }
  if ((p & 2u) != 0 && p + 2u <= hi)
  {
    *reinterpret_cast<uint16_t *>(word8 + p) = (uint16_t)(w >> (8u * p));
    p += 2u;
  }
  if ((p & 3u) == 0 && p + 4u <= hi)
  {
    *reinterpret_cast<uint32_t *>(word8 + p) = (uint32_t)(w >> (8u * p));
    p += 4u;
  }
  if ((p & 1u) == 0 && p + 2u <= hi)
  {
    *reinterpret_cast<uint16_t *>(word8 + p) = (uint16_t)(w >> (8u * p));
    p += 2u;
  }
  if (p < hi)
    word8[p] = (uint8_t)(w >> (8u * p));
}

// Where a block's finished words go (the S of CsvWriter): whole 8-byte stores, but of the first word -- the one the block
// starts in -- only the bytes from `head` on.  The writer starts with nacc = head and those bytes of acc zero.
struct CsvStoreEdges
{
  uint8_t *dst;  // the 8-byte word that the writer's pending bytes belong to
  uint32_t head; // the first byte of that word that is this block's; 0 once a word has gone out
  DG_DEV void word(uint64_t w)
  {
    if (head != 0)
      csv_store_bytes(dst, w, head, 8u);
    else
      *reinterpret_cast<uint64_t *>(dst) = w;
    head = 0;
    dst += 8;
  }
};

// The rows block b of channel c owns, walked once.  WRITE = false: the length; true: the text.
template <bool WRITE>
__global__ void __launch_bounds__(256) dega_csv_write_split_walk_kernel(const CsvWriteSplitArgs s)
{
  const CsvArgs &a = s.a;
  const uint32_t tile_b = blockIdx.x / s.tiles_c, tile_c = blockIdx.x - tile_b * s.tiles_c;
  const size_t c = ((size_t)tile_c << s.cw_log2) + (threadIdx.x & ((1u << s.cw_log2) - 1u));
  const uint64_t b = (uint64_t)tile_b * (CSVWS_BLOCK >> s.cw_log2) + (threadIdx.x >> s.cw_log2);
  if (c >= a.C || b >= s.blocks)
    return;
  uint32_t *const mine = s.work + c * (size_t)s.blocks + b;
  uint32_t off = 0;
  if (WRITE)
  {
    off = *mine;
    if (off == CSVWS_NOTHING)
      return;
  }
  uint64_t n = a.T;
  if (a.count != nullptr)
  {
    n = a.count[c];
    n = n > a.T ? 0u : n; // (the scan reports it; the channel owns nothing)
  }
  const uint64_t first = b * s.block_rows; // (below 2^32 x max(1, T): no overflow)
  const uint64_t end = first + s.block_rows < n ? first + s.block_rows : n;
  if (first >= end)
  {
    if (!WRITE)
      *mine = 0;
    return;
  }
  const uint32_t d = a.decimals, p10 = CSV_POW10[d];
  const uint32_t *const src = reinterpret_cast<const uint32_t *>(a.v) + c;

  if (WRITE)
  {
    const CsvSeparators seps(a.sep, a.nsep);
    CsvWriter<CsvStoreEdges> w;
    w.store.dst = a.out + c * a.stride + (off & ~7u); // (a row starts at a multiple of 16)
    w.store.head = off & 7u;
    w.acc = 0;
    w.nacc = off & 7u;
    uint32_t next = src[first * a.ld];
    for (uint64_t t = first; t < end; t++)
    {
      const uint32_t bits = next;
      if (t + 1u < end)
        next = src[(t + 1u) * a.ld];
      csv_put_line(w, csv_format<true>(bits, d, p10), seps);
    }
    csv_store_bytes(w.store.dst, w.acc, w.store.head, w.nacc); // behind the last boundary (or all of a block inside one word)
  }
  else
  {
    uint32_t sum = 0;
    uint32_t next = src[first * a.ld];
    for (uint64_t t = first; t < end; t++)
    {
      const uint32_t bits = next;
      if (t + 1u < end)
        next = src[(t + 1u) * a.ld];
      // (sum <= 2^31 - 1 and a line is below 2^31 + 64: the addition stays within 32 bits)
      sum += a.nsep + csv_format<false>(bits, d, p10).length();
      sum = sum < CSVWS_SATURATED ? sum : CSVWS_SATURATED;
    }
    *mine = sum;
  }
}

// One workgroup per channel: lengths -> byte offsets, in place, and the channel's length and status.
__global__ void __launch_bounds__(256) dega_csv_write_split_scan_kernel(const CsvWriteSplitArgs s)
{
  __shared__ uint64_t sum[2][CSVWS_SCAN_BLOCK]; // bytes of the lanes' chunks, scanned
  const CsvArgs &a = s.a;
  const size_t c = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  uint32_t *const work = s.work + c * (size_t)s.blocks;
  const uint32_t per = (s.blocks + CSVWS_SCAN_BLOCK - 1u) / CSVWS_SCAN_BLOCK;
  const uint64_t lo64 = (uint64_t)tid * per;
  const uint32_t lo = lo64 < s.blocks ? (uint32_t)lo64 : s.blocks;
  const uint32_t hi = lo64 + per < s.blocks ? (uint32_t)(lo64 + per) : s.blocks;

  uint64_t mine = 0;
  for (uint32_t i = lo; i < hi; i++)
    mine += work[i];
  sum[0][tid] = mine;
  __syncthreads();
  uint32_t from = 0;
  for (uint32_t k = 1; k < CSVWS_SCAN_BLOCK; k <<= 1, from ^= 1u) // inclusive, Hillis-Steele
  {
    uint64_t x = sum[from][tid];
    if (tid >= k)
      x += sum[from][tid - k];
    sum[from ^ 1u][tid] = x;
    __syncthreads();
  }
  const uint64_t total = sum[from][CSVWS_SCAN_BLOCK - 1u]; // (a saturated block makes it 2^31 - 1 or more: above stride - CSV_SLACK)
  const bool over = a.count != nullptr && a.count[c] > a.T;
  const bool fits = !over && total + CSV_SLACK <= a.stride;
  uint64_t at = sum[from][tid] - mine;
  for (uint32_t i = lo; i < hi; i++)
  {
    const uint32_t w = work[i];
    work[i] = fits ? (uint32_t)at : CSVWS_NOTHING; // (at < stride < 2^31: never CSVWS_NOTHING)
    at += w;
  }
  if (tid == 0)
  {
    a.out_len[c] = fits ? total : 0u;
    a.err[c] = over ? CSV_ERR_INVALID_VALUE : (fits ? CSV_OK : CSV_ERR_MEMORY);
  }
}

// ---- host side: how the kernels are launched (dega_launch.hpp) ---------------------------------------------------------------

// blocks per channel at block_rows >= 1 (at or above T: one block; T = 0: one, empty); may be beyond 32 bits: the caller checks
inline size_t csv_write_split_blocks(size_t T, size_t block_rows)
{
  return block_rows >= T ? 1 : (T - 1) / block_rows + 1;
}

inline uint32_t csv_write_split_cw_log2(size_t C) // cw = 64 for C >= 64, otherwise the smallest power of two >= C
{
  uint32_t k = 0;
  while ((1u << k) < CSVWS_MAX_CW && ((size_t)1 << k) < C)
    k++;
  return k;
}

// workgroups of length and of write for C channels of `blocks` blocks; 0: beyond the limits of a launch
inline size_t csv_write_split_grid(size_t C, size_t blocks)
{
  if (C == 0 || blocks == 0 || blocks > 0xFFFFFFFFu || C > LAUNCH_MAX_GX)
    return 0;
  const uint32_t k = csv_write_split_cw_log2(C);
  const size_t tiles_c = ((C - 1) >> k) + 1, bw = CSVWS_BLOCK >> k, tiles_b = (blocks - 1) / bw + 1;
  return tiles_b > LAUNCH_MAX_GX / tiles_c ? 0 : tiles_c * tiles_b;
}

// a: csv_args(...), its count null for the uniform form; block_rows >= 1
inline CsvWriteSplitArgs csv_write_split_args(const CsvArgs &a, size_t block_rows, uint32_t *work)
{
  CsvWriteSplitArgs s;
  s.a = a;
  const size_t rows = a.T != 0 ? a.T : 1;
  s.block_rows = block_rows < rows ? block_rows : rows;
  s.blocks = (uint32_t)csv_write_split_blocks(a.T, block_rows);
  s.cw_log2 = csv_write_split_cw_log2(a.C);
  s.tiles_c = a.C != 0 ? (uint32_t)(((a.C - 1) >> s.cw_log2) + 1) : 0;
  s.work = work;
  return s;
}

// length, scan and -- unless T is 0 -- write, in this order on the backend's stream
template <typename L>
inline bool launch(const CsvWriteSplitArgs &s, L &&launch_one)
{
  const size_t gx = s.block_rows != 0 && csv_write_split_blocks(s.a.T, s.block_rows) == s.blocks ? csv_write_split_grid(s.a.C, s.blocks) : 0;
  if (gx == 0)
    return false;
  launch_one(dega_csv_write_split_walk_kernel<false>, LaunchGrid{(uint32_t)gx, 1}, CSVWS_BLOCK, s);
  launch_one(dega_csv_write_split_scan_kernel, LaunchGrid{(uint32_t)s.a.C, 1}, CSVWS_SCAN_BLOCK, s);
  if (s.a.T != 0)
    launch_one(dega_csv_write_split_walk_kernel<true>, LaunchGrid{(uint32_t)gx, 1}, CSVWS_BLOCK, s);
  return true;
}

} // namespace dg
