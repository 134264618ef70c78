// openjph_amd/csrc/kernels_chroma.hip -- a Y, Cb, Cr frame of one chroma format -> the same frame in another (include/ojphgpu.h
// section 7f): 4:4:4, 4:2:2, 4:2:0 and 4:4:0 into each other over planar containers, exact integer arithmetic, one rounding.
//   frame_rechroma_kernel   one launch for the three planes (blockIdx.y).  Luma, and a chroma plane whose cells are equal,
//                      goes through a straight 16-byte copy loop (copy_run).  A chroma plane, per direction: halved -- the
//                      taps (1, 2, 1) of frame_resample_kernel (kernels_fit.hip) ON source sample 2 i, indices clamped into
//                      the plane, 2 bits; doubled -- the weights (2) / (1, 1) of colour_inverse_kernel (kernels_colour.hip),
//                      1 bit; the 2-D product, rounded once: (acc + 2^(k - 1)) >> k.  Every weight is positive and they sum
//                      to 2^k, so an output lies between the smallest and the largest input: no clamp.
// Modelled on frame_resample_kernel and the colour kernels: an item is the group of output columns one 16-byte store covers
// (16, 8 or 4), walked down eight output rows.  Halved vertically, the bottom row's horizontal sums are carried as the next
// top row; doubled vertically, the lower source row as the next upper one.  The one sample a group needs beyond its own loads
// -- the left neighbour of a halved row, the right neighbour of a doubled one -- is an extra load, not a lane exchange.  A row
// that does not stand on the load's boundary, or a group over the row's end, goes sample by sample with clamped indices.
// 8- and 16-bit containers are unsigned and sum in 32 bits (16 weights over 16-bit samples: 20 bits); the 32-bit container is
// int32 and sums in 64.  Plain vector stores, no LDS, no scratch.  The frame is a kernel argument.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "ojph_plan.h"

namespace {

constexpr uint32_t WG = 256;
constexpr uint32_t ROWS = 8;                                // output rows an item walks down

template <typename T> struct Acc { typedef int32_t type; };
template <> struct Acc<int32_t> { typedef int64_t type; };
template <typename T> struct Group { static constexpr int N = 16 / (int)sizeof(T); };   // output columns of an item

template <int BYTES> struct Vec;
template <> struct Vec<8> { typedef uint2 type; };
template <> struct Vec<16> { typedef uint4 type; };

enum { SAME = 0, HALVE = 1, DOUBLE = 2 };                   // what a direction does to a chroma plane
template <int M> struct Bits { static constexpr int K = M == HALVE ? 2 : M == DOUBLE ? 1 : 0; };

// the samples x0 .. x0 + N - 1 of a row of w (8 or 16 bytes): one load where all exist and the address allows, else one by
// one, the index clamped into the row (a sample past the row's end is never stored, but it IS the clamped tap of its neighbour)
template <typename T, int N, typename A>
__device__ __forceinline__ void load_group(const T* __restrict__ row, uint64_t x0, uint64_t w, A e[N])
{
  constexpr int B = N * (int)sizeof(T);
  typedef typename Vec<B>::type V;
  const T* p = row + x0;
  if (x0 + (uint64_t)N <= w && ((uintptr_t)p & (uintptr_t)(B - 1)) == 0) {
    const V v = *reinterpret_cast<const V*>(p);
    T raw[N];
    __builtin_memcpy(raw, &v, B);
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = (A)raw[i];
  } else {
    const uint64_t last = w - 1u;
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = (A)row[min(x0 + (uint64_t)i, last)];
  }
}

// the horizontal sums of output columns o .. o + G - 1 (o a multiple of G) over one source row of sw >= 1 samples
template <typename T, int MX>
__device__ __forceinline__ void row_sums(const T* __restrict__ row, uint64_t sw, uint64_t o, typename Acc<T>::type h[Group<T>::N])
{
  typedef typename Acc<T>::type A;
  constexpr int G = Group<T>::N;
  if constexpr (MX == SAME) {
    load_group<T, G, A>(row, o, sw, h);
  } else if constexpr (MX == HALVE) {                       // s[2 x - 1] + 2 s[2 x] + s[2 x + 1]; 2 o <= sw - 1: the size rule
    A e[2 * G];
    load_group<T, G, A>(row, 2u * o, sw, e);
    load_group<T, G, A>(row, 2u * o + G, sw, e + G);
    A prev = (A)row[o ? 2u * o - 1u : 0u];
#pragma unroll
    for (int i = 0; i < G; ++i) {
      h[i] = prev + 2 * e[2 * i] + e[2 * i + 1];
      prev = e[2 * i + 1];
    }
  } else {                                                  // 2 C[x / 2] (x even), C[(x - 1) / 2] + C[min((x + 1) / 2, sw - 1)] (x odd)
    A e[G / 2];
    const uint64_t xc = o / 2u;                             // (<= sw - 1: the size rule)
    load_group<T, G / 2, A>(row, xc, sw, e);
    const A right = (A)row[min(xc + (uint64_t)(G / 2), sw - 1u)];
#pragma unroll
    for (int j = 0; j < G / 2; ++j) {
      h[2 * j] = 2 * e[j];
      h[2 * j + 1] = e[j] + (j + 1 < G / 2 ? e[(j + 1) % (G / 2)] : right);
    }
  }
}

// one output row of a group: rounded once, stored -- as one 16-byte store where all exist and the address allows, else singly
template <typename T, int K>
__device__ __forceinline__ void store_row(T* drow, uint64_t o, uint64_t dw, const typename Acc<T>::type a[Group<T>::N])
{
  typedef typename Acc<T>::type A;
  constexpr int G = Group<T>::N;
  T q[G];
#pragma unroll
  for (int i = 0; i < G; ++i) q[i] = K ? (T)((a[i] + ((A)1 << (K ? K - 1 : 0))) >> K) : (T)a[i];
  T* p = drow + o;
  if (o + (uint64_t)G <= dw && ((uintptr_t)p & 15u) == 0) {
    uint4 v;
    __builtin_memcpy(&v, q, 16);
    *reinterpret_cast<uint4*>(p) = v;
  } else {
#pragma unroll
    for (int i = 0; i < G; ++i) if (o + (uint64_t)i < dw) p[i] = q[i];
  }
}

// a chroma plane sw x sh -> dw x dh: the part of this workgroup (bx of nbx) and this thread.  The planes do not overlap.
template <typename T, int MX, int MY>
__device__ void rechroma_run(const T* __restrict__ src, T* dst, uint64_t sw, uint64_t sh, uint64_t dw, uint64_t dh, uint32_t bx, uint32_t nbx)
{
  typedef typename Acc<T>::type A;
  constexpr int G = Group<T>::N, K = Bits<MX>::K + Bits<MY>::K;
  const uint64_t ncg = (dw + G - 1u) / G, nrb = (dh + ROWS - 1u) / ROWS, items = ncg * nrb;
  for (uint64_t it = (uint64_t)bx * WG + threadIdx.x; it < items; it += (uint64_t)nbx * WG) {
    const uint64_t band = it / ncg, o = (it - band * ncg) * G;
    const uint64_t j0 = band * ROWS, j1 = min(j0 + ROWS, dh);
    if constexpr (MY == SAME) {
      for (uint64_t j = j0; j < j1; ++j) {
        A a[G];
        row_sums<T, MX>(src + j * sw, sw, o, a);
        store_row<T, K>(dst + j * dw, o, dw, a);
      }
    } else if constexpr (MY == HALVE) {
      A top[G];                                             // source row 2 j - 1, clamped; below the first row: the carry
      row_sums<T, MX>(src + (j0 ? 2u * j0 - 1u : 0u) * sw, sw, o, top);
      for (uint64_t j = j0; j < j1; ++j) {
        const uint64_t r = 2u * j;                          // (< sh: the size rule)
        A mid[G], bot[G], a[G];
        row_sums<T, MX>(src + r * sw, sw, o, mid);
        row_sums<T, MX>(src + min(r + 1u, sh - 1u) * sw, sw, o, bot);
#pragma unroll
        for (int i = 0; i < G; ++i) { a[i] = top[i] + 2 * mid[i] + bot[i]; top[i] = bot[i]; }
        store_row<T, K>(dst + j * dw, o, dw, a);
      }
    } else {
      A up[G];                                              // source row j / 2; below the first pair: the carry
      uint64_t r = j0 / 2u;                                 // (j0 is even; r < sh: the size rule)
      row_sums<T, MX>(src + r * sw, sw, o, up);
      for (uint64_t j = j0; j < j1; j += 2u, ++r) {
        A lo[G], a[G];
        row_sums<T, MX>(src + min(r + 1u, sh - 1u) * sw, sw, o, lo);
#pragma unroll
        for (int i = 0; i < G; ++i) a[i] = 2 * up[i];
        store_row<T, K>(dst + j * dw, o, dw, a);
        if (j + 1u < dh) {
#pragma unroll
          for (int i = 0; i < G; ++i) a[i] = up[i] + lo[i];
          store_row<T, K>(dst + (j + 1u) * dw, o, dw, a);
        }
#pragma unroll
        for (int i = 0; i < G; ++i) up[i] = lo[i];
      }
    }
  }
}

// the elements [0, count) of src -> dst as they are: the part of this workgroup (bx of nbx) and this thread
template <typename T>
__device__ void copy_run(const T* __restrict__ src, T* dst, uint64_t count, uint32_t bx, uint32_t nbx)
{
  constexpr int G = Group<T>::N, U = 4;                     // U groups in flight: four 16-byte loads per thread
  const uint32_t t = threadIdx.x;
  const uintptr_t ps = (uintptr_t)src, pd = (uintptr_t)dst;
  const uint64_t stride = (uint64_t)nbx * WG;
  if (((ps ^ pd) & 15u) != 0) {                             // the two planes sit differently in their 16 bytes: sample by sample
    for (uint64_t i = (uint64_t)bx * WG + t; i < count; i += stride) dst[i] = src[i];
    return;
  }
  const uint64_t to_boundary = ((16u - (ps & 15u)) & 15u) / sizeof(T);
  const uint64_t head = count < to_boundary ? count : to_boundary;
  const uint64_t ng = (count - head) / G, tail0 = head + ng * G;
  if (bx == 0) {                                            // (head < G, count - tail0 < G, G <= 16)
    if (t < head) dst[t] = src[t];
    if (tail0 + t < count) dst[tail0 + t] = src[tail0 + t];
  }
  const uint4* vs = reinterpret_cast<const uint4*>(src + head);
  uint4* vd = reinterpret_cast<uint4*>(dst + head);
  for (uint64_t g0 = (uint64_t)bx * WG + t; g0 < ng; g0 += U * stride) {
    uint4 x[U]; bool ok[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const uint64_t g = g0 + (uint64_t)k * stride;
      ok[k] = g < ng;
      x[k] = vs[ok[k] ? g : g0];                            // (a clamped address; the group is not stored)
    }
#pragma unroll
    for (int k = 0; k < U; ++k) if (ok[k]) vd[g0 + (uint64_t)k * stride] = x[k];
  }
}

// grid = (workgroups per plane, 3)
template <typename T, int MX, int MY>
__global__ __launch_bounds__(WG) void frame_rechroma_kernel(const T* src, T* dst, const ojphgpu_chroma_frame f)
{
  const uint32_t p = blockIdx.y, bx = blockIdx.x, nbx = gridDim.x;
  const T* s = src + f.src_off[p];
  T* d = dst + f.dst_off[p];
  const uint64_t w = f.w, h = f.h;
  const uint64_t sw = (w + f.sfx - 1u) / f.sfx, sh = (h + f.sfy - 1u) / f.sfy;
  if (p == 0) { copy_run<T>(s, d, w * h, bx, nbx); return; }
  if constexpr (MX == SAME && MY == SAME) copy_run<T>(s, d, sw * sh, bx, nbx);
  else rechroma_run<T, MX, MY>(s, d, sw, sh, (w + f.dfx - 1u) / f.dfx, (h + f.dfy - 1u) / f.dfy, bx, nbx);
}

template <typename T, int MX>
void launch_y(hipStream_t stream, uint32_t gx, int my, const void* src, void* dst, const ojphgpu_chroma_frame& f)
{
  const dim3 grid(gx, 3), block(WG);
  if (my == SAME) hipLaunchKernelGGL((frame_rechroma_kernel<T, MX, SAME>), grid, block, 0, stream, (const T*)src, (T*)dst, f);
  else if (my == HALVE) hipLaunchKernelGGL((frame_rechroma_kernel<T, MX, HALVE>), grid, block, 0, stream, (const T*)src, (T*)dst, f);
  else hipLaunchKernelGGL((frame_rechroma_kernel<T, MX, DOUBLE>), grid, block, 0, stream, (const T*)src, (T*)dst, f);
}

template <typename T>
void launch_x(hipStream_t stream, uint32_t gx, int mx, int my, const void* src, void* dst, const ojphgpu_chroma_frame& f)
{
  if (mx == SAME) launch_y<T, SAME>(stream, gx, my, src, dst, f);
  else if (mx == HALVE) launch_y<T, HALVE>(stream, gx, my, src, dst, f);
  else launch_y<T, DOUBLE>(stream, gx, my, src, dst, f);
}

int mode_of(uint32_t s, uint32_t d) { return s == d ? SAME : d == 2u * s ? HALVE : DOUBLE; }

}  // namespace

extern "C" int ojphgpu_frame_rechroma(void* stream, const void* d_src, void* d_dst, int container_bits, const ojphgpu_chroma_frame* frame)
{
  if (!d_src || !d_dst || !frame || (container_bits != 8 && container_bits != 16 && container_bits != 32)) return OJPHGPU_E_INVALID;
  const ojphgpu_chroma_frame f = *frame;
  if (f.w == 0 || f.h == 0) return OJPHGPU_E_INVALID;
  for (uint32_t c : { f.sfx, f.sfy, f.dfx, f.dfy }) if (c != 1 && c != 2) return OJPHGPU_E_INVALID;
  const uint64_t b = (uint64_t)container_bits / 8u;
  if (((uintptr_t)d_src & (uintptr_t)(b - 1u)) != 0 || ((uintptr_t)d_dst & (uintptr_t)(b - 1u)) != 0) return OJPHGPU_E_INVALID;
  // no source plane over a destination plane (byte ranges)
  const uint64_t luma = (uint64_t)f.w * f.h;
  const uint64_t sc = (uint64_t)((f.w + f.sfx - 1u) / f.sfx) * (uint64_t)((f.h + f.sfy - 1u) / f.sfy);
  const uint64_t dc = (uint64_t)((f.w + f.dfx - 1u) / f.dfx) * (uint64_t)((f.h + f.dfy - 1u) / f.dfy);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const uintptr_t s0 = (uintptr_t)d_src + f.src_off[i] * b, s1 = s0 + (i ? sc : luma) * b;
      const uintptr_t d0 = (uintptr_t)d_dst + f.dst_off[j] * b, d1 = d0 + (j ? dc : luma) * b;
      if (s0 < d1 && d0 < s1) return OJPHGPU_E_INVALID;
    }
  const char* e = getenv("OJPHGPU_CHROMA_WGS");
  const long v = e ? atol(e) : 0;
  const uint64_t cap = v > 0 && v <= 65535 ? (uint64_t)v : 2048u;   // eight workgroups per compute unit over the three planes
  // the luma plane's copy has the most items: one per 16 bytes (a chroma plane's: one per eight rows of 16 bytes)
  const uint64_t items = (luma * b + 15u) / 16u;
  const uint32_t gx = (uint32_t)std::max<uint64_t>(1u, std::min(cap / 3u, (items + WG - 1u) / WG));
  const int mx = mode_of(f.sfx, f.dfx), my = mode_of(f.sfy, f.dfy);
  if (container_bits == 8) launch_x<uint8_t>((hipStream_t)stream, gx, mx, my, d_src, d_dst, f);
  else if (container_bits == 16) launch_x<uint16_t>((hipStream_t)stream, gx, mx, my, d_src, d_dst, f);
  else launch_x<int32_t>((hipStream_t)stream, gx, mx, my, d_src, d_dst, f);
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}
