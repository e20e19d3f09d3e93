// csv_read_split_kernels.hpp -- `decode csv` (ReadCSV, DCLib/src/csv.c:13-44) for few long channels: one channel's text
// split over lanes.  For gfx950 (MI355X).
//
// The same input, output and results as csv_read_kernels.hpp, whose conversion this header reuses as it stands (CsvrField,
// csvr_feed_slow, csvr_steady, csvr_finish, CSVR_POW5); what differs is the unit of parallelism.  There a lane is a channel,
// because where a value lands depends on every line before it.  Here a lane is a (channel, block) pair.
//
// The reader's state behind a '\n' is always the same: column 1 and an empty field (csv.c:27-41).  So a text can be cut at
// line starts.  A channel's len[c] bytes are cut into blocks of block_bytes; block b covers bytes [b*B, (b+1)*B).
//   A BLOCK OWNS EXACTLY THE LINES THAT START INSIDE IT.  A line starts at byte 0 or at a byte whose predecessor is '\n'.
//   A lane whose block starts mid-line skips to just behind the first '\n' of its block (none, or one on the block's last
//   byte: it owns nothing), then runs csv.c:22-41 byte by byte, past the block's end if need be, and stops behind the first
//   '\n' whose successor lies in a later block, or behind byte len[c] - 1.  That last byte is appended to a selected field
//   and ends it whatever it is (csv.c:23-26); only the lane that gets there sees it.
// Two things are global to a channel: its values are numbered across blocks, and the reader stops at the first selected
// field of more than CSVR_FIELD_MAX characters.  Three launches on one stream settle both:
//   count  a lane per pair walks its lines with the splitting only (column, field length, field ends; no digit arithmetic)
//          and writes the number of values it owns to work[c][b], bit 31 set when it stopped at such a field (the count is
//          then that of the values in front of it).
//   scan   a workgroup per channel: the exclusive prefix over the channel's blocks, cut behind the first flagged block,
//          in place -- work[c][b] becomes the block's first row, or CSVRS_NO_ROWS for the blocks behind the flagged one --
//          and out_count[c] and err[c] as the unsplit kernel would write them.
//   parse  a lane per pair walks the same lines with the full conversion and stores value i of its block at row base + i
//          of column c where that row is below max_T.  Not launched for max_T = 0.
// count and parse are two instantiations of one walk, so they cannot disagree about the lines.
//
// Mapping: pair index = c * blocks + b, a lane per pair, blocks fastest.  Adjacent lanes hold adjacent blocks of ONE channel,
// so a single channel spreads over the whole device, the 16-byte pieces a wave asks for lie block_bytes apart in one text
// (whole cache lines are used within a few steps) and the rows a wave stores lie close together in one column.  A field is
// converted where it ends, in the lane, not queued for the wave: the queue of the unsplit kernel exists because its four
// waves are all there is, while here the device is full of waves that hide one another's divergence; without the queue the
// walk needs no LDS but the 448 bytes of the steady path's table, and nothing limits its occupancy but registers.
//
// Reads: 16-byte pieces at multiples of 16 below len[c] <= stride, so never outside the channel's stride bytes.  Writes:
// only rows below max_T of column c < C; every defined row by exactly one lane; no atomics.
//
// This header is compiled by hipcc (dega_hip.hip) and, for offline checking only, by g++ under tests/sim/.
#pragma once

#include "csv_read_kernels.hpp"

namespace dg
{

constexpr uint32_t CSVRS_BLOCK = 256;              // lanes = (channel, block) pairs per workgroup of count and parse
constexpr uint32_t CSVRS_SCAN_BLOCK = 256;         // lanes of the workgroup that scans one channel
constexpr uint32_t CSVRS_FLAG = 0x80000000u;       // work[c][b] after count: the block stopped at a field too long
constexpr uint32_t CSVRS_NO_ROWS = 0xFFFFFFFFu;    // work[c][b] after scan: the block stores nothing

// dega_hip_csv_read_split_block_bytes: the largest block that still gives the batch CSVRS_FILL_PAIRS (channel, block) pairs,
// not below CSVRS_FLOOR_BYTES.  Both from the sweep of profiles/csv_read_split_bench.txt (86 400 readings per channel, blocks of
// 64 .. 16 384 bytes): the time falls with the block size until the batch has about 12 M pairs -- the fastest row at 4 096
// channels is 256 bytes, 4 096 x 3 038 = 12.4 M pairs -- and at 1, 16 and 256 channels, which never get there, the smallest
// block of the sweep, 64 bytes, is the fastest.  (Small blocks win for a second reason that the pair count does not name: a
// wave's 64 pieces then lie within a few KiB of one text.)  DESIGN.md 4.7.1 names the rows.
constexpr size_t CSVRS_FILL_PAIRS = 12u << 20;
constexpr size_t CSVRS_FLOOR_BYTES = 64;

struct alignas(16) CsvrsPiece // 16 bytes of text: one load
{
  uint32_t x, y, z, w;
};

struct CsvReadSplitArgs
{
  CsvReadArgs r;         // what the unsplit kernel takes
  uint32_t block_bytes;  // a multiple of 16, at most max(16, stride)
  uint32_t blocks;       // per channel: ceil(stride / block_bytes)
  uint32_t *work;        // [C][blocks]
};

// Pure host code: the library's choice of block_bytes; 0 for a stride the reader refuses.
inline size_t csv_read_split_block_bytes(size_t C, size_t stride)
{
  if (stride < 16 || (stride & 15u) != 0 || stride > 0x7FFFFFF0u)
    return 0;
  const size_t floor_bytes = CSVRS_FLOOR_BYTES < stride ? CSVRS_FLOOR_BYTES : stride;
  const size_t need = C == 0 ? CSVRS_FILL_PAIRS : (CSVRS_FILL_PAIRS + C - 1) / C; // blocks per channel that fill the device
  if (need <= 1)
    return stride;
  // ceil(stride / B) >= need  <=>  B <= (stride - 1) / (need - 1)
  const size_t most = ((stride - 1) / (need - 1)) & ~(size_t)15;
  return most < floor_bytes ? floor_bytes : (most > stride ? stride : most);
}

// The lines block b of channel c owns, walked once.  PARSE = false: count; true: convert and store.
template <bool PARSE>
__global__ void __launch_bounds__(256) dega_csv_read_split_walk_kernel(const CsvReadSplitArgs s)
{
  __shared__ uint64_t pow5[2 * (CSVR_STEADY_DECIMALS + 1)]; // (parse only) the steady path's divisors, a lane's index away
  if (PARSE)
  {
    if (threadIdx.x <= CSVR_STEADY_DECIMALS)
    {
      pow5[2 * threadIdx.x] = CSVR_POW5[threadIdx.x][0];
      pow5[2 * threadIdx.x + 1] = CSVR_POW5[threadIdx.x][1];
    }
    __syncthreads(); // (in front of every return: all lanes come here)
  }
  const CsvReadArgs &a = s.r;
  const size_t pair = (size_t)blockIdx.x * CSVRS_BLOCK + threadIdx.x;
  if (pair >= a.C * (size_t)s.blocks)
    return;
  const size_t c = pair / s.blocks;
  const uint32_t b = (uint32_t)(pair - c * s.blocks);
  const uint64_t len64 = a.len[c];
  const uint32_t n = len64 > a.stride ? 0u : (uint32_t)len64; // (a channel longer than its row owns nothing)
  const uint64_t first64 = (uint64_t)b * s.block_bytes;
  uint32_t base = 0;
  if (PARSE)
  {
    base = s.work[pair];
    if (base == CSVRS_NO_ROWS)
      return;
  }
  if (first64 >= n)
  {
    if (!PARSE)
      s.work[pair] = 0;
    return;
  }
  const uint32_t first = (uint32_t)first64;
  const uint64_t end64 = first64 + s.block_bytes;
  const uint32_t block_end = end64 < n ? (uint32_t)end64 : n; // lines that start at or behind it are another lane's
  const uint8_t *const src = a.text + c * a.stride;
  const uint32_t column = a.column, sep = a.sep & 0xFFu;
  const uint32_t T32 = a.max_T < 0xFFFFFFFFu ? (uint32_t)a.max_T : 0xFFFFFFFFu;
  uint32_t *const dst = PARSE ? reinterpret_cast<uint32_t *>(a.v) + c : nullptr; // (a counting call may have no v at all)

  CsvrField f;
  f.reset();
  uint32_t col = 1, flen = 0;
  uint32_t t = 0; // values of this block so far
  bool flagged = false;
  // a block behind the first starts one byte early, looking for the '\n' in front of its first line
  bool skipping = b != 0;
  uint32_t pos = skipping ? first - 1u : 0u;
  bool running = true;

  auto step = [&](uint32_t ch, bool last) { // csv.c:22-41 for one character, as in dega_csv_read_kernel
    const bool end = ch == sep || ch == 0x0Au || last;
    const bool selected = col == column;
    if (selected && (!end || last))
    {
      flen++;
      if (PARSE)
      {
        const uint32_t d = ch - 0x30u;
        if (d < 10u && f.st <= CSVR_FRAC && f.nd < 19u) // the steady form: a digit of a decimal number
        {
          f.kind = CSVR_DEC;
          f.st = f.st == CSVR_FRAC ? CSVR_FRAC : ((f.st <= CSVR_SIGNED && d == 0) ? CSVR_ZERO : CSVR_INT);
          f.w0 = f.w0 * 10u + d;
          f.nd += (f.nd | d) != 0 ? 1u : 0u;
          f.fdig += f.st == CSVR_FRAC ? 1u : 0u;
        }
        else if (ch == 0x2Eu && (f.st == CSVR_ZERO || f.st == CSVR_INT))
          f.st = CSVR_FRAC;
        else
          csvr_feed_slow(f, ch);
      }
      if (flen > CSVR_FIELD_MAX) // the reference's buffer overruns here: the channel stops in front of this field
      {
        flagged = true;
        running = false;
        return;
      }
    }
    if (end)
    {
      if (selected)
      {
        if (PARSE)
        {
          uint32_t bits;
          if (f.st >= CSVR_ZERO && f.st <= CSVR_FRAC && f.nd <= 19u && f.fdig <= CSVR_STEADY_DECIMALS)
            bits = csvr_steady(f.w0, f.fdig, pow5[2 * f.fdig], pow5[2 * f.fdig + 1]) | (f.neg << 31);
          else
            bits = csvr_finish(f);
          const uint32_t row = base + t; // (below 2^31: a channel has fewer values than bytes)
          if (row < T32)
            dst[(size_t)row * a.ld] = bits;
          f.reset();
        }
        flen = 0;
        t++;
      }
      col++;
    }
    if (ch == 0x0Au)
      col = 1;
  };

  // 16-byte pieces, the next one asked for while this one is consumed; every piece lies below n <= stride rounded to 16
  const CsvrsPiece *const pieces = reinterpret_cast<const CsvrsPiece *>(src);
  uint32_t piece = pos >> 4;
  const uint32_t piece_last = (n - 1u) >> 4;
  CsvrsPiece next = pieces[piece];
  while (running)
  {
    const CsvrsPiece cur = next;
    if (piece < piece_last)
      next = pieces[piece + 1u];
    const uint32_t w[4] = {cur.x, cur.y, cur.z, cur.w};
    const uint32_t stop = (piece + 1u) << 4;
#pragma unroll 1
    for (; running && pos < stop; pos++)
    {
      const uint32_t k = pos & 15u;
      const uint32_t word = k < 8u ? (k < 4u ? w[0] : w[1]) : (k < 12u ? w[2] : w[3]);
      const uint32_t ch = (word >> (8u * (k & 3u))) & 0xFFu;
      const bool last = pos + 1u == n;
      if (skipping)
      {
        if (pos + 1u >= block_end) // no line starts inside this block
          running = false;
        else if (ch == 0x0Au)
          skipping = false;
      }
      else
      {
        step(ch, last);
        if (last || (ch == 0x0Au && pos + 1u >= block_end))
          running = false;
      }
    }
    piece++;
  }
  if (!PARSE)
    s.work[pair] = t | (flagged ? CSVRS_FLAG : 0u);
}

// One workgroup per channel: counts -> first rows, in place, and the channel's count and status.
__global__ void __launch_bounds__(256) dega_csv_read_split_scan_kernel(const CsvReadSplitArgs s)
{
  __shared__ uint32_t sum[2][CSVRS_SCAN_BLOCK];  // values of the lanes' chunks (cut behind a flagged block), scanned
  __shared__ uint32_t stop[2][CSVRS_SCAN_BLOCK]; // the first lane with a flagged block, scanned with min
  const CsvReadArgs &a = s.r;
  const size_t c = blockIdx.x;
  const uint32_t tid = threadIdx.x;
  uint32_t *const work = s.work + c * (size_t)s.blocks;
  const uint32_t per = (s.blocks + CSVRS_SCAN_BLOCK - 1u) / CSVRS_SCAN_BLOCK;
  const uint64_t lo64 = (uint64_t)tid * per;
  const uint32_t lo = lo64 < s.blocks ? (uint32_t)lo64 : s.blocks;
  const uint32_t hi = lo64 + per < s.blocks ? (uint32_t)(lo64 + per) : s.blocks;

  uint32_t mine = 0;
  bool flagged = false;
  for (uint32_t i = lo; i < hi && !flagged; i++)
  {
    const uint32_t w = work[i];
    mine += w & ~CSVRS_FLAG;
    flagged = (w & CSVRS_FLAG) != 0;
  }
  sum[0][tid] = mine;
  stop[0][tid] = flagged ? tid : CSVRS_SCAN_BLOCK;
  __syncthreads();
  uint32_t from = 0;
  for (uint32_t d = 1; d < CSVRS_SCAN_BLOCK; d <<= 1, from ^= 1u) // inclusive, Hillis-Steele
  {
    uint32_t x = sum[from][tid], y = stop[from][tid];
    if (tid >= d)
    {
      x += sum[from][tid - d];
      const uint32_t o = stop[from][tid - d];
      y = o < y ? o : y;
    }
    sum[from ^ 1u][tid] = x;
    stop[from ^ 1u][tid] = y;
    __syncthreads();
  }
  const uint32_t first_flagged = stop[from][CSVRS_SCAN_BLOCK - 1u]; // CSVRS_SCAN_BLOCK: none
  // (the sums of the lanes in front of the first flagged one are whole, its own is cut: the inclusive scan there is the count)
  uint32_t row = sum[from][tid] - mine;
  bool cut = tid > first_flagged;
  for (uint32_t i = lo; i < hi; i++)
  {
    const uint32_t w = work[i];
    work[i] = cut ? CSVRS_NO_ROWS : row;
    row += w & ~CSVRS_FLAG;
    cut = cut || (w & CSVRS_FLAG) != 0;
  }
  if (tid == 0)
  {
    const bool any = first_flagged < CSVRS_SCAN_BLOCK;
    const uint32_t total = sum[from][any ? first_flagged : CSVRS_SCAN_BLOCK - 1u];
    const bool too_long = a.len[c] > a.stride;
    a.out_count[c] = total; // (0 for a channel longer than its row: its blocks own nothing)
    a.err[c] = too_long ? CSVR_ERR_INVALID_VALUE : (any ? CSVR_ERR_INVALID_FORMAT : (total > a.max_T ? CSVR_ERR_MEMORY : CSVR_OK));
  }
}

// ---- host side: how the kernels are launched (dega_launch.hpp) ---------------------------------------------------------------

// blocks per channel at block_bytes (a multiple of 16, at least 16; above stride: one block)
inline size_t csv_read_split_blocks(size_t stride, size_t block_bytes)
{
  return block_bytes >= stride ? 1 : (stride + block_bytes - 1) / block_bytes;
}

inline CsvReadSplitArgs csv_read_split_args(const CsvReadArgs &r, size_t block_bytes, uint32_t *work)
{
  CsvReadSplitArgs s;
  s.r = r;
  s.block_bytes = (uint32_t)(block_bytes >= r.stride ? r.stride : block_bytes);
  s.blocks = (uint32_t)csv_read_split_blocks(r.stride, block_bytes);
  s.work = work;
  return s;
}

// count, scan and -- unless max_T is 0 -- parse, in this order on the backend's stream
template <typename L>
inline bool launch(const CsvReadSplitArgs &s, L &&launch_one)
{
  const size_t C = s.r.C;
  if (s.blocks == 0 || C > LAUNCH_MAX_GX || C > (LAUNCH_MAX_GX * (size_t)CSVRS_BLOCK) / s.blocks)
    return false;
  const size_t gx = (C * s.blocks + CSVRS_BLOCK - 1) / CSVRS_BLOCK;
  launch_one(dega_csv_read_split_walk_kernel<false>, LaunchGrid{(uint32_t)gx, 1}, CSVRS_BLOCK, s);
  launch_one(dega_csv_read_split_scan_kernel, LaunchGrid{(uint32_t)C, 1}, CSVRS_SCAN_BLOCK, s);
  if (s.r.max_T != 0)
    launch_one(dega_csv_read_split_walk_kernel<true>, LaunchGrid{(uint32_t)gx, 1}, CSVRS_BLOCK, s);
  return true;
}

} // namespace dg
