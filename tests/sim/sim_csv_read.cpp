// sim_csv_read.cpp -- runs the shipped `decode csv` kernel source (data-compressor_amd/csrc/csv_read_kernels.hpp) under the
// thread-per-lane emulator of hipsim.hpp.  TEST INFRASTRUCTURE ONLY; see hipsim.hpp.  Built by the pattern rule of
// tests/sim/Makefile (libcsv_read_sim.so) for tests/test_csv_read_host.py.
#define DEGA_SIM 1
#define dg dgsim // keep the emulated kernels' symbols apart from libdega_hip.so's
#include "sim_launch.hpp"

#include "../../data-compressor_amd/csrc/csv_read_kernels.hpp"

using namespace dg;

// Guards what the kernel relies on (what dega_hip_csv_read_* refuses; the library's own checks are tested on the GPU).
extern "C" __attribute__((visibility("default"))) int sim_csv_read(const uint8_t *text, size_t stride, const uint64_t *len, size_t C, size_t column, int sep,
                                                                   float *v, size_t max_T, size_t ld, uint64_t *out_count, int32_t *err)
{
  if (C == 0 || column == 0 || sep < 0 || sep > 255 || ld < C || stride < 16 || stride % 16 != 0 || stride > 0x7FFFFFF0u ||
      ((uintptr_t)text & 15u) != 0 || ((uintptr_t)v & 3u) != 0)
    return -1;
  for (size_t c = 0; c < C; c++)
    if (len[c] > stride)
      return -1;
  return launch(csv_read_args(text, stride, len, C, column, sep, v, max_T, ld, out_count, err), OnEmulator{}) ? 0 : -1;
}

// one field through the kernel's own conversion, without the emulator: the field's float, or -1 when it has 48 characters
// or more
extern "C" __attribute__((visibility("default"))) int64_t sim_csv_read_field(const uint8_t *field, size_t n)
{
  CsvrField f;
  f.reset();
  for (size_t i = 0; i < n; i++)
  {
    if (++f.flen > CSVR_FIELD_MAX)
      return -1;
    csvr_feed_slow(f, field[i]);
  }
  if (f.st >= CSVR_ZERO && f.st <= CSVR_FRAC && f.nd <= 19u && f.fdig <= CSVR_STEADY_DECIMALS)
    return (int64_t)(csvr_steady(f.w0, f.fdig, CSVR_POW5[f.fdig][0], CSVR_POW5[f.fdig][1]) | (f.neg << 31));
  return (int64_t)csvr_finish(f);
}
