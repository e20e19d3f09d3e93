// sim_csv_write_split_main.cpp -- the emulated split `encode csv` kernels as a stand-alone program for the host sanitizers
// (tests/test_csv_write_split_host.py compiles it with -fsanitize=address,undefined and runs it as a child process; never
// loaded into Python, never run on a GPU).  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.
//
//   sim_csv_write_split_asan <batches in> <results out>
// in:  per batch  uint64 {C, T, ld, decimals, column, separator_char, stride, block_rows, counted}, uint64 count[C] when
//                 counted is not 0, uint32 v[T][ld]
// out: per batch  uint64 out_len[C], int32 err[C], uint8 text[C][stride] (pre-filled with the canary 0xEE)
// Every array is allocated exactly as large as the call may touch: C x stride bytes of text, T x ld floats (none at all for
// T = 0), so that a read or a write one element outside is the sanitizer's to report.
#include "sim_csv_write_split.cpp"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int main(int argc, char **argv)
{
  if (argc != 3)
    return 2;
  FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
  if (in == nullptr || out == nullptr)
    return 2;
  uint64_t head[9];
  size_t batches = 0;
  while (fread(head, sizeof(uint64_t), 9, in) == 9)
  {
    const size_t C = head[0], T = head[1], ld = head[2], column = head[4], stride = head[6], block_rows = head[7];
    const unsigned decimals = (unsigned)head[3];
    const int sep = (int)head[5];
    uint64_t *count = head[8] != 0 ? (uint64_t *)malloc(C * sizeof(uint64_t)) : nullptr;
    if (count != nullptr && fread(count, sizeof(uint64_t), C, in) != C)
      return 3;
    uint32_t *v = T * ld != 0 ? (uint32_t *)malloc(T * ld * sizeof(uint32_t)) : nullptr;
    if (v != nullptr && fread(v, sizeof(uint32_t), T * ld, in) != T * ld)
      return 3;
    uint8_t *text = (uint8_t *)aligned_alloc(16, C * stride);
    memset(text, 0xEE, C * stride);
    uint64_t *len = (uint64_t *)malloc(C * sizeof(uint64_t));
    int32_t *err = (int32_t *)malloc(C * sizeof(int32_t));
    if (sim_csv_write_split((const float *)v, C, T, ld, count, decimals, column, sep, text, stride, len, err, block_rows) != 0)
      return 4;
    fwrite(len, sizeof(uint64_t), C, out);
    fwrite(err, sizeof(int32_t), C, out);
    fwrite(text, 1, C * stride, out);
    free(err);
    free(len);
    free(text);
    free(v);
    free(count);
    batches++;
  }
  fclose(in);
  if (fclose(out) != 0)
    return 5;
  printf("%zu batches\n", batches);
  return 0;
}
