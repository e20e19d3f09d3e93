// sim_axdr_main.cpp -- the emulated A-XDR kernels as a stand-alone program for the host sanitizers (tests/test_axdr_host.py
// compiles it with -fsanitize=address,undefined and runs it as a child process; never loaded into Python, never run on a
// GPU).  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.
//
//   sim_axdr_asan
// A fixed selection: per (value size, C, T, pitch, counted, 16-byte form) a pack of pseudo-random fields, the streams compared
// with a bit-by-bit pack written here, and the unpack of those streams compared with the fields.  Every array is allocated
// as large as the call may touch and no larger than the next 16 bytes -- T x ld elements less the last row's padding, C x
// cap bytes with cap exactly the stream's words -- so that a read or a write a row or a slab outside is the sanitizer's to
// report.  Prints "axdr: ok".
#include "sim_axdr.cpp"

#include <stdio.h>
#include <stdlib.h>

#include <vector>

static uint64_t next_random(uint64_t &s)
{
  s += 0x9E3779B97F4A7C15ull;
  uint64_t z = s;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static void put_bit(std::vector<uint8_t> &bytes, size_t at, unsigned bit)
{
  if (bit)
    bytes[at >> 3] |= (uint8_t)(0x80u >> (at & 7u));
}

struct Case
{
  int vs;
  size_t C, T, pad;
  bool counted, wide;
};

static int run_case(const Case &k, uint64_t &seed)
{
  const bool w64 = k.vs > 32;
  const size_t esz = w64 ? 8 : 4, ld = k.C + k.pad, cap = 4 * ((k.T * (size_t)k.vs + 31) / 32);
  const uint64_t mask = k.vs == 64 ? ~0ull : (1ull << k.vs) - 1;
  const size_t elems = k.T == 0 ? 0 : (k.T - 1) * ld + k.C; // (the last row ends with its last channel)
  // (aligned_alloc: the 16-byte form needs its base, and the call a size that is a multiple of 16 -- up to 15 bytes of room
  // behind the last element that the sanitizer does not watch)
  uint8_t *x = elems != 0 ? (uint8_t *)aligned_alloc(16, (elems * esz + 15) / 16 * 16) : nullptr;
  std::vector<uint64_t> field(k.T * k.C), count(k.C);
  for (size_t t = 0; t < k.T; t++)
    for (size_t c = 0; c < ld; c++)
    {
      if ((t * ld + c) >= elems)
        continue;
      const uint64_t r = next_random(seed);
      if (c < k.C)
        field[t * k.C + c] = r & mask;
      if (w64)
        ((uint64_t *)x)[t * ld + c] = r;
      else
        ((uint32_t *)x)[t * ld + c] = (uint32_t)r | (k.vs < 32 ? (uint32_t)(r >> 32) << k.vs : 0u); // (junk above the field)
    }
  if (!w64)
    for (size_t t = 0; t < k.T; t++)
      for (size_t c = 0; c < k.C; c++)
        field[t * k.C + c] = ((uint32_t *)x)[t * ld + c] & mask;
  for (size_t c = 0; c < k.C; c++)
    count[c] = k.counted ? next_random(seed) % (k.T + 1) : k.T;
  uint8_t *out = (uint8_t *)aligned_alloc(16, k.C * cap != 0 ? (k.C * cap + 15) / 16 * 16 : 16);
  memset(out, 0xC5, k.C * cap);
  std::vector<uint64_t> bits(k.C, 7);
  std::vector<int32_t> err(k.C, 77);
  const int kind = w64 ? 2 : 1;
  if (sim_axdr_pack(x, kind, k.C, k.T, ld, k.counted ? count.data() : nullptr, 1.0f, k.vs, out, cap, bits.data(), err.data(), k.wide ? 1 : 0, 5) != 0)
    return 10;
  for (size_t c = 0; c < k.C; c++)
  {
    const size_t n = count[c], words = (n * (size_t)k.vs + 31) / 32;
    std::vector<uint8_t> want(cap, 0xC5);
    for (size_t b = 0; b < 4 * words; b++)
      want[b] = 0;
    for (size_t t = 0; t < n; t++)
      for (int b = 0; b < k.vs; b++)
        put_bit(want, t * (size_t)k.vs + (size_t)b, (unsigned)(field[t * k.C + c] >> (k.vs - 1 - b)) & 1u);
    if (err[c] != 0 || bits[c] != n * (uint64_t)k.vs || (cap != 0 && memcmp(want.data(), out + c * cap, cap) != 0))
      return 11;
  }
  // and back: exactly max_T x ld elements less the last row's padding
  const size_t max_T = k.T;
  uint8_t *y = elems != 0 ? (uint8_t *)aligned_alloc(16, (elems * esz + 15) / 16 * 16) : nullptr;
  if (y != nullptr)
    memset(y, 0x5A, elems * esz);
  std::vector<uint64_t> got_count(k.C, 7);
  if (sim_axdr_unpack(out, cap, bits.data(), k.C, max_T, ld, 1.0f, k.vs, kind, y, got_count.data(), err.data(), k.wide ? 1 : 0, 5) != 0)
    return 12;
  for (size_t c = 0; c < k.C; c++)
  {
    if (err[c] != 0 || got_count[c] != count[c])
      return 13;
    for (size_t t = 0; t < count[c]; t++)
      if ((w64 ? ((uint64_t *)y)[t * ld + c] : (uint64_t)((uint32_t *)y)[t * ld + c]) != field[t * k.C + c])
        return 14;
    for (size_t t = count[c]; t < k.T; t++) // rows behind a count keep what they held
      if ((w64 ? ((uint64_t *)y)[t * ld + c] : (uint64_t)((uint32_t *)y)[t * ld + c]) != (w64 ? 0x5A5A5A5A5A5A5A5Aull : 0x5A5A5A5Aull))
        return 15;
  }
  free(y);
  free(out);
  free(x);
  return 0;
}

int main()
{
  const Case cases[] = {
      {1, 65, 129, 0, false, false}, {3, 64, 33, 0, true, true},    {8, 130, 300, 7, false, false}, {12, 68, 128, 0, false, true},
      {17, 1, 127, 0, true, false},  {24, 63, 31, 1, false, false}, {31, 65, 1, 0, true, false},    {32, 64, 128, 0, false, true},
      {32, 5, 0, 0, false, false},   {33, 65, 65, 3, true, false},  {47, 66, 172, 0, false, true},  {63, 1, 64, 0, false, false},
      {64, 130, 63, 0, true, true},
  };
  uint64_t seed = 2015;
  for (const Case &k : cases)
  {
    const int r = run_case(k, seed);
    if (r != 0)
    {
      printf("axdr: case vs=%d C=%zu T=%zu failed with %d\n", k.vs, k.C, k.T, r);
      return r;
    }
  }
  printf("axdr: ok\n");
  return 0;
}
