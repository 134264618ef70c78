// tools/sanitize/hip_shim/hip/hip_runtime.h -- just enough of the HIP device dialect for g++ to compile the text of a data-
// movement kernel (no LDS, no barriers, no cross-lane traffic but readfirstlane) for the HOST, so that a stand-alone program
// can run it lane by lane under the address and undefined-behaviour sanitizers (tools/sanitize/run_video420.sh).  Put in front
// of the include path, this file is what `#include <hip/hip_runtime.h>` finds.  The vector types carry the alignment the
// hardware instructions assume, so a 16-byte piece at an address that is not a multiple of 16 is an alignment error here.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __launch_bounds__(...)

struct dim3 { unsigned x, y, z; dim3(unsigned x_ = 1, unsigned y_ = 1, unsigned z_ = 1) : x(x_), y(y_), z(z_) {} };
struct alignas(16) uint4 { uint32_t x, y, z, w; };
struct alignas(8) uint2 { uint32_t x, y; };
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{ x, y, z, w }; }
inline uint2 make_uint2(uint32_t x, uint32_t y) { return uint2{ x, y }; }

typedef void* hipStream_t;
enum hipError_t { hipSuccess = 0 };
inline hipError_t hipGetLastError() { return hipSuccess; }

inline dim3 threadIdx, blockIdx, blockDim, gridDim;

namespace hip_shim {
// readfirstlane: the lanes of a wavefront run one after the other; call n of a lane must see the value call n of the
// wavefront's first lane saw, or the kernel's claim that the value is wave-uniform is wrong
inline std::vector<int> wave_values;
inline size_t lane_calls = 0;
inline int readfirstlane(int v)
{
  if (lane_calls == wave_values.size()) wave_values.push_back(v);
  else if (wave_values[lane_calls] != v) { fprintf(stderr, "hip_shim: readfirstlane of a value that differs inside the wavefront\n"); abort(); }
  return wave_values[lane_calls++];
}
// v_perm_b32: byte i of the result is the byte of the eight of {hi, lo} that byte i of the selector names (0 to 3: of lo, 4 to 7:
// of hi); the selectors above 7 (constants, sign bytes) are not used by the kernels compiled here
inline uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
  const uint64_t both = (uint64_t)hi << 32 | lo;
  uint32_t r = 0;
  for (int i = 0; i < 4; ++i) {
    const uint32_t s = (sel >> (8 * i)) & 0xFFu;
    if (s > 7) { fprintf(stderr, "hip_shim: perm selector byte 0x%x\n", s); abort(); }
    r |= (uint32_t)((both >> (8 * s)) & 0xFFu) << (8 * i);
  }
  return r;
}
template <class F> void launch(dim3 grid, dim3 block, F&& body)
{
  gridDim = grid; blockDim = block;
  const unsigned lanes = block.x * block.y * block.z;
  for (unsigned bz = 0; bz < grid.z; ++bz) for (unsigned by = 0; by < grid.y; ++by) for (unsigned bx = 0; bx < grid.x; ++bx) {
    blockIdx = dim3(bx, by, bz);
    for (unsigned t = 0; t < lanes; ++t) {
      if (t % 64 == 0) wave_values.clear();
      lane_calls = 0;
      threadIdx = dim3(t % block.x, (t / block.x) % block.y, t / (block.x * block.y));
      body();
    }
  }
}
}  // namespace hip_shim

#define __builtin_amdgcn_readfirstlane hip_shim::readfirstlane
#define __builtin_amdgcn_perm hip_shim::perm
#define hipLaunchKernelGGL(kernel, grid, block, lds, stream, ...) hip_shim::launch(grid, block, [&] { kernel(__VA_ARGS__); })
