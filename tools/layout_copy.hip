// layout_copy.hip -- the streaming yardstick of tools/layoutbench.py: a float4 copy, device to device.  Every lane moves
// four float4 that lie one workgroup apart (four 16-byte loads in flight, then four stores), a wave reads and writes whole
// 1-KiB segments; 8 bytes of traffic per 4-byte element, like the transposition it is measured beside.
//   hipcc --offload-arch=gfx950 -O3 -fPIC -shared tools/layout_copy.hip -o tools/liblayout_copy.so   (layoutbench.py does it)
#include <hip/hip_runtime.h>
#include <stddef.h>

constexpr unsigned BLOCK = 256, PER_LANE = 4;

__global__ void __launch_bounds__(256) copy_f4_kernel(const float4 *src, float4 *dst, size_t n)
{
  const size_t i0 = (size_t)blockIdx.x * (BLOCK * PER_LANE) + threadIdx.x;
  float4 v[PER_LANE];
#pragma unroll
  for (unsigned u = 0; u < PER_LANE; u++)
    if (i0 + u * BLOCK < n)
      v[u] = src[i0 + u * BLOCK];
#pragma unroll
  for (unsigned u = 0; u < PER_LANE; u++)
    if (i0 + u * BLOCK < n)
      dst[i0 + u * BLOCK] = v[u];
}

// bytes: a multiple of 16, both pointers 16-byte aligned; returns 0, or -1 for arguments it does not take
extern "C" int layout_copy_f4(const void *src, void *dst, size_t bytes, void *stream)
{
  const size_t n = bytes / 16, per_block = (size_t)BLOCK * PER_LANE, blocks = (n + per_block - 1) / per_block;
  if (bytes % 16 != 0 || (((size_t)src | (size_t)dst) & 15u) != 0 || blocks == 0 || blocks > 0xFFFFFFu)
    return -1;
  hipLaunchKernelGGL(copy_f4_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, (hipStream_t)stream, (const float4 *)src, (float4 *)dst, n);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
