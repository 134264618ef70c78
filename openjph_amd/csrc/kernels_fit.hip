// openjph_amd/csrc/kernels_fit.hip -- what recoding through the sample domain (include/ojphgpu.h section 5e) adds on the device:
//   frame_fit_kernel   an int32 frame as the decoder hands it over -> the frame an encoder of another bit depth takes: per
//                      component a shift to the output's depth (down: round half up, an arithmetic shift evaluated in 64
//                      bits; up: a left shift), the clamp to the output's nominal range -- a decoded sample may lie past
//                      its range, which int32 hands over as it is --, and the store into the output's container (int8 /
//                      int16 where the range is signed, uint8 / uint16 where not, int32)
//
// One pass over HBM with next to no arithmetic: 4 bytes read and 1, 2 or 4 written per sample.  Modelled on
// frame_error_kernel (kernels_quality.hip): a group is the four samples of one 16-byte load, stored with one 4-, 8- or
// 16-byte store; scalar edges; nothing is written outside the `count` elements of a component's run.  No LDS.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ojph_plan.h"

namespace {

constexpr uint32_t WG = 256;

// shift > 0: (v + 2^(shift - 1)) >> shift; shift < 0: v << -shift; |shift| <= 31, so nothing leaves 64 bits
__device__ __forceinline__ int32_t fit_sample(int32_t v, int shift, int32_t lo, int32_t hi)
{
  int64_t x = v;
  if (shift > 0) x = (x + ((int64_t)1 << (shift - 1))) >> shift;
  else if (shift < 0) x = x * ((int64_t)1 << -shift);
  x = x < (int64_t)lo ? (int64_t)lo : x;
  x = x > (int64_t)hi ? (int64_t)hi : x;
  return (int32_t)x;
}

template <typename TD> struct Pack;                         // four fitted samples as one store
template <> struct Pack<int32_t> { typedef uint4 type; };
template <> struct Pack<int16_t> { typedef uint2 type; };
template <> struct Pack<uint16_t> { typedef uint2 type; };
template <> struct Pack<int8_t> { typedef uint32_t type; };
template <> struct Pack<uint8_t> { typedef uint32_t type; };

// the elements [0, count) of src -> dst: the part of this workgroup (bx of nbx) and this thread.  dst may be src (TD =
// int32_t): every element is read and written by the same thread, the read first.
template <typename TD>
__device__ void frame_fit_run(const int32_t* src, TD* dst, uint64_t count, int shift, int32_t lo, int32_t hi, uint32_t bx, uint32_t nbx)
{
  typedef typename Pack<TD>::type V;
  constexpr int U = 4;                                      // groups in flight: four 16-byte loads per thread
  const uint32_t t = threadIdx.x;
  const uintptr_t ps = (uintptr_t)src, pd = (uintptr_t)dst;
  // scalar head up to the first element at which the source stands on a 16-byte boundary; the destination must then stand
  // on the boundary of its own group (containers are naturally aligned)
  const uint64_t to_boundary = ((16u - (ps & 15u)) & 15u) / 4u;
  if (((pd + to_boundary * sizeof(TD)) & (sizeof(V) - 1)) != 0) {
    // the two frames sit differently in their 16 bytes: sample by sample
    for (uint64_t i = (uint64_t)bx * WG + t; i < count; i += (uint64_t)nbx * WG) dst[i] = (TD)fit_sample(src[i], shift, lo, hi);
    return;
  }
  const uint64_t head = count < to_boundary ? count : to_boundary;
  const uint64_t ng = (count - head) / 4u, tail0 = head + ng * 4u;
  if (bx == 0) {                                            // (head <= 3, count - tail0 <= 3)
    if (t < head) dst[t] = (TD)fit_sample(src[t], shift, lo, hi);
    if (tail0 + t < count) dst[tail0 + t] = (TD)fit_sample(src[tail0 + t], shift, lo, hi);
  }
  const uint4* vs = reinterpret_cast<const uint4*>(src + head);
  V* vd = reinterpret_cast<V*>(dst + head);
  const uint64_t stride = (uint64_t)nbx * WG;
  for (uint64_t g0 = (uint64_t)bx * WG + t; g0 < ng; g0 += U * stride) {
    uint4 x[U]; bool ok[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const uint64_t g = g0 + (uint64_t)k * stride;
      ok[k] = g < ng;
      x[k] = vs[ok[k] ? g : g0];                            // (a clamped address; the group is not stored)
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      if (!ok[k]) continue;
      int32_t e[4]; TD o[4];
      __builtin_memcpy(e, &x[k], sizeof(e));
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = (TD)fit_sample(e[i], shift, lo, hi);
      V v;
      __builtin_memcpy(&v, o, sizeof(v));
      vd[g0 + (uint64_t)k * stride] = v;
    }
  }
}

// grid = (workgroups per component, components)
__global__ __launch_bounds__(WG) void frame_fit_kernel(const int32_t* src, void* dst, int bits, const ojphgpu_fit_comp* __restrict__ comps)
{
  const ojphgpu_fit_comp c = comps[blockIdx.y];
  if (c.shift < -31 || c.shift > 31 || c.lo > c.hi) return;  // (not a fit: the component is left alone)
  const uint32_t bx = blockIdx.x, nbx = gridDim.x;
  const int32_t* s = src + c.first_elem;
  if (bits == 8) {
    if (c.lo < 0) frame_fit_run<int8_t>(s, (int8_t*)dst + c.first_elem, c.count, c.shift, max(c.lo, -128), min(c.hi, 127), bx, nbx);
    else frame_fit_run<uint8_t>(s, (uint8_t*)dst + c.first_elem, c.count, c.shift, c.lo, min(c.hi, 255), bx, nbx);
  } else if (bits == 16) {
    if (c.lo < 0) frame_fit_run<int16_t>(s, (int16_t*)dst + c.first_elem, c.count, c.shift, max(c.lo, -32768), min(c.hi, 32767), bx, nbx);
    else frame_fit_run<uint16_t>(s, (uint16_t*)dst + c.first_elem, c.count, c.shift, c.lo, min(c.hi, 65535), bx, nbx);
  } else
    frame_fit_run<int32_t>(s, (int32_t*)dst + c.first_elem, c.count, c.shift, c.lo, c.hi, bx, nbx);
}

}  // namespace

extern "C" int ojphgpu_frame_fit(void* stream, const int32_t* d_src, void* d_dst, int container_bits, const ojphgpu_fit_comp* d_comps,
                                 uint32_t n_comps)
{
  if (!d_src || !d_dst || !d_comps || (container_bits != 8 && container_bits != 16 && container_bits != 32)) return OJPHGPU_E_INVALID;
  if (n_comps == 0) return OJPHGPU_OK;
  if (n_comps > 65535u) return OJPHGPU_E_INVALID;
  // the frames must be containers in their natural alignment (the head of a run is counted up to a 16-byte boundary)
  if (((uintptr_t)d_src & 3u) != 0 || ((uintptr_t)d_dst & (uintptr_t)(container_bits / 8 - 1)) != 0) return OJPHGPU_E_INVALID;
  // the frames are one buffer or apart: a narrower frame laid over its source would be overwritten before it is read
  if (container_bits != 32 && (const void*)d_src == (const void*)d_dst) return OJPHGPU_E_INVALID;
  // about 2048 workgroups over the components (eight per compute unit), each striding over its component's run
  const uint32_t gx = std::max(1u, 2048u / n_comps);
  hipLaunchKernelGGL(frame_fit_kernel, dim3(gx, n_comps), dim3(WG), 0, (hipStream_t)stream, d_src, d_dst, container_bits, d_comps);
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}
