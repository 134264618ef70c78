// openjph_amd/csrc/kernels_video_pieces.h -- what the video-buffer kernels share (kernels_video.hip: 4:2:2, one packed
// buffer; kernels_video420.hip: 4:2:0, two planes): samples in and out of containers held as dwords, a lane's run of dwords
// <-> memory in the widest pieces a wave-uniform alignment allows (one pair of functions for the long runs of the 4:2:2
// kernels, one for the short runs of the 4:2:0 kernels), the clamp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// sample j of a run of containers held as dwords (j is a compile-time constant wherever these are called)
template <typename D> __device__ __forceinline__ void put(uint32_t* w, int j, uint32_t v)
{
  if (sizeof(D) == 4) w[j] = v;
  else if (sizeof(D) == 2) w[j >> 1] |= v << (16 * (j & 1));
  else w[j >> 2] |= v << (8 * (j & 3));
}
template <typename D> __device__ __forceinline__ int32_t get(const uint32_t* w, int j)
{
  if (sizeof(D) == 4) return (int32_t)w[j];
  if (sizeof(D) == 2) return (int32_t)((w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
  return (int32_t)((w[j >> 2] >> (8 * (j & 3))) & 0xFFu);
}

// NW dwords (a multiple of four) <-> memory in the widest pieces the (wave-uniform) alignment `al` of the address allows;
// MIN: what the element type guarantees anyway.  The 4:2:2 kernels' pair, beside load_run / store_run on purpose: one pair for
// both (the run generalised to any multiple of four dwords) changes all twenty 4:2:2 kernels, five take more VGPRs and
// pack_video_kernel<V210, int> goes from 706 to 759 instructions and 63 to 84 global loads (profiles/video_pieces_fold_isa.txt).
template <int NW, int MIN> __device__ __forceinline__ void store_words(uint8_t* p, const uint32_t* w, uint32_t al)
{
  if ((al & 15u) == 0) {
#pragma unroll
    for (int i = 0; i < NW / 4; ++i) *(uint4*)(p + 16 * i) = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
  } else if ((al & 7u) == 0) {
#pragma unroll
    for (int i = 0; i < NW / 2; ++i) *(uint2*)(p + 8 * i) = make_uint2(w[2 * i], w[2 * i + 1]);
  } else if (MIN >= 4 || (al & 3u) == 0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) *(uint32_t*)(p + 4 * i) = w[i];
  } else if (MIN >= 2 || (al & 1u) == 0) {
#pragma unroll
    for (int i = 0; i < 2 * NW; ++i) *(uint16_t*)(p + 2 * i) = (uint16_t)(w[i >> 1] >> (16 * (i & 1)));
  } else {
#pragma unroll
    for (int i = 0; i < 4 * NW; ++i) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  }
}
template <int NW, int MIN> __device__ __forceinline__ void load_words(const uint8_t* p, uint32_t* w, uint32_t al)
{
  if ((al & 15u) == 0) {
#pragma unroll
    for (int i = 0; i < NW / 4; ++i) { const uint4 v = *(const uint4*)(p + 16 * i); w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w; }
  } else if ((al & 7u) == 0) {
#pragma unroll
    for (int i = 0; i < NW / 2; ++i) { const uint2 v = *(const uint2*)(p + 8 * i); w[2 * i] = v.x; w[2 * i + 1] = v.y; }
  } else if (MIN >= 4 || (al & 3u) == 0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = *(const uint32_t*)(p + 4 * i);
  } else if (MIN >= 2 || (al & 1u) == 0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = (uint32_t)*(const uint16_t*)(p + 4 * i) | (uint32_t)*(const uint16_t*)(p + 4 * i + 2) << 16;
  } else {
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
  }
}

// The same for a lane's SMALL run of NW = 1, 2 or 4 dwords (the 4:2:0 kernels): `al` is the address of the row, p lies a
// whole number of runs into it, so a power of two that divides the row's address and is not longer than the run divides p.
// The wide pieces are native vectors on purpose: a struct such as uint4 is taken apart into four dword stores, the optimiser
// then moves the store that the three alignment branches have in common behind them, and what is left comes out as a
// 12-byte and a 4-byte instruction on every branch -- the wavefront's instruction no longer writes whole lines.
typedef uint32_t u32x4 __attribute__((vector_size(16)));
typedef uint32_t u32x2 __attribute__((vector_size(8)));
template <int NW, int MIN> __device__ __forceinline__ void store_run(uint8_t* p, const uint32_t* w, uint32_t al)
{
  static_assert(NW == 1 || NW == 2 || NW == 4, "a run of 4, 8 or 16 bytes");
  if (NW == 4 && (al & 15u) == 0) {
    const u32x4 v = { w[0], w[NW > 1 ? 1 : 0], w[NW > 2 ? 2 : 0], w[NW > 3 ? 3 : 0] };
    *(u32x4*)p = v;
  } else if (NW >= 2 && (al & 7u) == 0) {
#pragma unroll
    for (int i = 0; i < NW / 2; ++i) { const u32x2 v = { w[2 * i], w[NW > 1 ? 2 * i + 1 : 0] }; *(u32x2*)(p + 8 * i) = v; }
  } else if (MIN >= 4 || (al & 3u) == 0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) *(uint32_t*)(p + 4 * i) = w[i];
  } else if (MIN >= 2 || (al & 1u) == 0) {
#pragma unroll
    for (int i = 0; i < 2 * NW; ++i) *(uint16_t*)(p + 2 * i) = (uint16_t)(w[i >> 1] >> (16 * (i & 1)));
  } else {
#pragma unroll
    for (int i = 0; i < 4 * NW; ++i) p[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
  }
}
template <int NW, int MIN> __device__ __forceinline__ void load_run(const uint8_t* p, uint32_t* w, uint32_t al)
{
  static_assert(NW == 1 || NW == 2 || NW == 4, "a run of 4, 8 or 16 bytes");
  if (NW == 4 && (al & 15u) == 0) {
    const u32x4 v = *(const u32x4*)p;
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = v[i & 3];
  } else if (NW >= 2 && (al & 7u) == 0) {
#pragma unroll
    for (int i = 0; i < NW / 2; ++i) { const u32x2 v = *(const u32x2*)(p + 8 * i); w[2 * i] = v[0]; w[NW > 1 ? 2 * i + 1 : 0] = v[1]; }
  } else if (MIN >= 4 || (al & 3u) == 0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = *(const uint32_t*)(p + 4 * i);
  } else if (MIN >= 2 || (al & 1u) == 0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = (uint32_t)*(const uint16_t*)(p + 4 * i) | (uint32_t)*(const uint16_t*)(p + 4 * i + 2) << 16;
  } else {
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
  }
}

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

__device__ __forceinline__ uint32_t clamp_sample(int32_t v, int32_t maxv) { return (uint32_t)(v < 0 ? 0 : (v > maxv ? maxv : v)); }

}  // namespace
