// sim_csv_read_split_main.cpp -- the emulated split `decode csv` kernels as a stand-alone program for the host sanitizers
// (tests/test_csv_read_split_host.py compiles it with -fsanitize=address,undefined and runs it as a child process; never
// loaded into Python, never run on a GPU).  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.
//
//   sim_csv_read_split_asan <batches in> <results out>
// in:  per batch  uint64 {C, stride, column, separator_char, max_T, ld, block_bytes}, uint64 len[C], uint8 text[C][stride]
// out: per batch  uint64 out_count[C], int32 err[C], uint32 v[max_T][ld]
// Every array is allocated exactly as large as the call may touch: C x stride bytes of text, max_T x ld floats (none at all
// for max_T = 0), so that a read or a write one element outside is the sanitizer's to report.
#include "sim_csv_read_split.cpp"

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
  uint64_t head[7];
  size_t batches = 0;
  while (fread(head, sizeof(uint64_t), 7, in) == 7)
  {
    const size_t C = head[0], stride = head[1], column = head[2], max_T = head[4], ld = head[5], block_bytes = head[6];
    const int sep = (int)head[3];
    uint64_t *len = (uint64_t *)malloc(C * sizeof(uint64_t));
    uint8_t *text = (uint8_t *)aligned_alloc(16, C * stride);
    if (fread(len, sizeof(uint64_t), C, in) != C || fread(text, 1, C * stride, in) != C * stride)
      return 3;
    uint64_t *count = (uint64_t *)malloc(C * sizeof(uint64_t));
    int32_t *err = (int32_t *)malloc(C * sizeof(int32_t));
    uint32_t *v = max_T * ld != 0 ? (uint32_t *)malloc(max_T * ld * sizeof(uint32_t)) : nullptr;
    for (size_t i = 0; i < max_T * ld; i++)
      v[i] = 0x7FC12345u;
    if (sim_csv_read_split(text, stride, len, C, column, sep, (float *)v, max_T, ld, count, err, block_bytes) != 0)
      return 4;
    fwrite(count, sizeof(uint64_t), C, out);
    fwrite(err, sizeof(int32_t), C, out);
    if (v != nullptr)
      fwrite(v, sizeof(uint32_t), max_T * ld, out);
    free(v);
    free(err);
    free(count);
    free(text);
    free(len);
    batches++;
  }
  fclose(in);
  if (fclose(out) != 0)
    return 5;
  printf("%zu batches\n", batches);
  return 0;
}
