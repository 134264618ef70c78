// where the time of the band statistics kernel (openjph_amd/csrc/kernels_stats.hip) goes: 100 M fp32 coefficients read
// linearly with its load shape (16-byte loads, four in flight per lane, 2048 workgroups), then (a) nothing but an xor of the
// words, (b) the bin of every word computed and summed, (c) the bins counted in the column table in LDS as the kernel does.
//   hipcc --offload-arch=gfx950 -O3 tools/micro/stats_floor.hip -o tools/micro/stats_floor && tools/micro/stats_floor
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("hip error %d line %d\n", (int)e, __LINE__); exit(1); } } while (0)

__global__ void fill(uint32_t* p, size_t n)
{
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    uint32_t h = (uint32_t)i * 2654435761u; h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    // exponents 110..121 (a dozen octaves, like a band of a real frame), random mantissa and sign
    p[i] = (h & 0x807FFFFFu) | ((110u + (h >> 8) % 12u) << 23);
  }
}

__device__ __forceinline__ uint32_t bin_of(uint32_t u)
{
  int e = (int)((u >> 22) & 0x1FFu) - 191;
  return (uint32_t)(e < 0 ? 0 : e > 79 ? 79 : e);
}

template <int MODE>
__global__ __launch_bounds__(256) void walk(const uint4* __restrict__ s, size_t n4, uint32_t* __restrict__ out)
{
  __shared__ uint32_t tab[40 * 64];
  const uint32_t t = threadIdx.x, lane = t & 63u;
  for (uint32_t i = t; i < 40 * 64; i += 256) tab[i] = 0;
  __syncthreads();
  uint32_t acc = 0;
  for (size_t i0 = (size_t)blockIdx.x * 1024; i0 < n4; i0 += (size_t)gridDim.x * 1024) {
    uint4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = s[std::min(i0 + (size_t)k * 256 + t, n4 - 1)];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t w[4] = { v[k].x, v[k].y, v[k].z, v[k].w };
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (MODE == 0) acc ^= w[c];
        else if (MODE == 1) acc += bin_of(w[c]);
        else { const uint32_t e = bin_of(w[c]); atomicAdd(&tab[(e >> 1) * 64 + lane], 1u << ((e & 1u) * 16u)); }
      }
    }
  }
  __syncthreads();
  if (MODE == 2) for (uint32_t i = t; i < 40 * 64; i += 256) acc += tab[i];
  if (acc == 0x12345678u) out[blockIdx.x] = acc;             // (keeps the work alive)
}

int main()
{
  const size_t n = (size_t)7680 * 4320 * 3, n4 = n / 4;
  uint32_t* d; uint32_t* out;
  CK(hipMalloc(&d, n * 4)); CK(hipMalloc(&out, 4096 * 4));
  hipLaunchKernelGGL(fill, dim3(4096), dim3(256), 0, 0, d, n);
  hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
  const char* names[3] = { "loads + xor", "loads + bins", "loads + bins + LDS columns" };
  for (int grid : { 2048, 4096 }) for (int mode = 0; mode < 3; ++mode) {
    std::vector<float> ms;
    for (int it = 0; it < 25; ++it) {
      CK(hipEventRecord(a, 0));
      if (mode == 0) hipLaunchKernelGGL(walk<0>, dim3(grid), dim3(256), 0, 0, (const uint4*)d, n4, out);
      if (mode == 1) hipLaunchKernelGGL(walk<1>, dim3(grid), dim3(256), 0, 0, (const uint4*)d, n4, out);
      if (mode == 2) hipLaunchKernelGGL(walk<2>, dim3(grid), dim3(256), 0, 0, (const uint4*)d, n4, out);
      CK(hipEventRecord(b, 0)); CK(hipEventSynchronize(b));
      float t; CK(hipEventElapsedTime(&t, a, b));
      if (it >= 5) ms.push_back(t);
    }
    std::sort(ms.begin(), ms.end());
    printf("grid %4d  %-28s median %.4f ms  %.2f TB/s\n", grid, names[mode], ms[ms.size() / 2], n * 4.0 / (ms[ms.size() / 2] * 1e-3) / 1e12);
  }
  CK(hipFree(d)); CK(hipFree(out));
  return 0;
}
