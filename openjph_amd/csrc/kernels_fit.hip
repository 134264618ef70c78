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
//
//   frame_resample_kernel   the same pass with a component halved on the way, horizontally, vertically or both (section 5e,
//                      "a resampling recode"): taps (1, 2, 1) centred ON source sample 2 i + phase, indices clamped into the
//                      plane, exact in 64 bits with one rounding, then the fit above.  An item is four output columns
//                      walked down ROWS output rows: per output row two new source rows (two 16-byte loads and one extra
//                      dword -- the left or right neighbour of the group -- each), the bottom row's horizontal sums carried
//                      as the next top row.  A component with both factors 1 goes through frame_fit_run.  No LDS, no scratch.
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

// ---------------------------------------------------------------------------------------------
// the fit with a component halved on the way
// ---------------------------------------------------------------------------------------------
constexpr uint32_t ROWS = 8;                                // output rows an item walks down

// the horizontal sums of output columns o .. o + 3 over one source row (sw >= 1 samples at `row`): FX == 2: s[c - 1] +
// 2 s[c] + s[c + 1] at c = 2 (o + i) + px, indices clamped into the row; FX == 1: the samples themselves.  Columns past
// the row's last output are computed from clamped (in-bounds) indices and never stored.
template <int FX>
__device__ __forceinline__ void row_sums(const int32_t* __restrict__ row, uint32_t sw, uint32_t px, uint32_t o, int64_t h[4])
{
  if (FX == 1) {
    if ((uint64_t)o + 4u <= sw && ((uintptr_t)(row + o) & 15u) == 0) {
      const uint4 x = *reinterpret_cast<const uint4*>(row + o);
      int32_t e[4];
      __builtin_memcpy(e, &x, sizeof(e));
#pragma unroll
      for (int i = 0; i < 4; ++i) h[i] = e[i];
    } else {
      const uint64_t last = (uint64_t)sw - 1u;
#pragma unroll
      for (int i = 0; i < 4; ++i) h[i] = row[min((uint64_t)o + (uint64_t)i, last)];
    }
    return;
  }
  const uint64_t b = 2u * (uint64_t)o, last = (uint64_t)sw - 1u;   // the group's eight samples b .. b + 7, and one more: b - 1 (px == 0) or b + 8
  if (b + 8u <= sw && ((uintptr_t)(row + b) & 15u) == 0) {
    const uint4 x0 = *reinterpret_cast<const uint4*>(row + b), x1 = *reinterpret_cast<const uint4*>(row + b + 4);
    const int32_t x = row[px ? min(b + 8u, last) : (b ? b - 1u : 0u)];
    int32_t e[8];
    __builtin_memcpy(e, &x0, 16); __builtin_memcpy(e + 4, &x1, 16);
    // the nine samples around the four centres: x, e[0..7] at px == 0, e[0..7], x at px == 1 (chosen with a mask: an index
    // that depends on px would put e[] into scratch)
    const int32_t m = -(int32_t)px;
    int32_t s[9];
    s[0] = x ^ ((x ^ e[0]) & m);
#pragma unroll
    for (int k = 1; k < 8; ++k) s[k] = e[k - 1] ^ ((e[k - 1] ^ e[k]) & m);
    s[8] = e[7] ^ ((e[7] ^ x) & m);
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = (int64_t)s[2 * i] + 2 * (int64_t)s[2 * i + 1] + (int64_t)s[2 * i + 2];
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint64_t c = min(b + 2u * (uint64_t)i + px, last);
      const uint64_t l = c ? c - 1u : 0u, r = min(c + 1u, last);
      h[i] = (int64_t)row[l] + 2 * (int64_t)row[c] + (int64_t)row[r];
    }
  }
}

// the four samples of one output row: rounded once, fitted, stored -- as one group where all four exist and the address
// allows it, else one by one
template <typename TD, int K>
__device__ __forceinline__ void store_row(TD* drow, uint32_t o, uint32_t dw, const int64_t a[4], int shift, int32_t lo, int32_t hi)
{
  typedef typename Pack<TD>::type V;
  TD q[4];
#pragma unroll
  for (int i = 0; i < 4; ++i)                               // (a weighted mean of int32 samples, rounded: an int32)
    q[i] = (TD)fit_sample((int32_t)((a[i] + ((int64_t)1 << (K - 1))) >> K), shift, lo, hi);
  if ((uint64_t)o + 4u <= dw && ((uintptr_t)(drow + o) & (sizeof(V) - 1)) == 0) {
    V v;
    __builtin_memcpy(&v, q, sizeof(v));
    *reinterpret_cast<V*>(drow + o) = v;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) if ((uint64_t)o + (uint64_t)i < dw) drow[o + i] = q[i];
  }
}

// a component with a factor of 2: the part of this workgroup (bx of nbx) and this thread.  The planes do not overlap.
template <typename TD, int FX, int FY>
__device__ void frame_resample_run(const int32_t* __restrict__ src, TD* dst, const ojphgpu_resample_comp& c, int32_t lo, int32_t hi, uint32_t bx, uint32_t nbx)
{
  constexpr int K = 2 * ((FX == 2) + (FY == 2));            // (2 or 4)
  const uint32_t sw = c.src_w, sh = c.src_h, dw = c.dst_w, dh = c.dst_h, px = c.px, py = c.py;
  const uint64_t ncg = ((uint64_t)dw + 3u) / 4u, nrb = ((uint64_t)dh + ROWS - 1u) / ROWS, items = ncg * nrb;
  for (uint64_t it = (uint64_t)bx * WG + threadIdx.x; it < items; it += (uint64_t)nbx * WG) {
    const uint64_t band = it / ncg;
    const uint32_t o = (uint32_t)(it - band * ncg) * 4u;
    const uint32_t j0 = (uint32_t)band * ROWS, j1 = (uint32_t)min((uint64_t)j0 + ROWS, (uint64_t)dh);
    if (FY == 1) {
      for (uint32_t j = j0; j < j1; ++j) {
        int64_t a[4];
        row_sums<FX>(src + (uint64_t)j * sw, sw, px, o, a);
        store_row<TD, K>(dst + (uint64_t)j * dw, o, dw, a, c.shift, lo, hi);
      }
    } else {
      int64_t top[4];                                       // source row 2 j + py - 1, clamped; below the first row: the carry
      const uint64_t r0 = 2u * (uint64_t)j0 + py;
      row_sums<FX>(src + (r0 ? r0 - 1u : 0u) * sw, sw, px, o, top);
      for (uint32_t j = j0; j < j1; ++j) {
        const uint64_t r = 2u * (uint64_t)j + py;           // (< sh: the size rule)
        int64_t mid[4], bot[4], a[4];
        row_sums<FX>(src + r * sw, sw, px, o, mid);
        row_sums<FX>(src + min(r + 1u, (uint64_t)sh - 1u) * sw, sw, px, o, bot);
#pragma unroll
        for (int i = 0; i < 4; ++i) { a[i] = top[i] + 2 * mid[i] + bot[i]; top[i] = bot[i]; }
        store_row<TD, K>(dst + (uint64_t)j * dw, o, dw, a, c.shift, lo, hi);
      }
    }
  }
}

template <typename TD>
__device__ __forceinline__ void frame_resample_comp(const int32_t* src, TD* dst, const ojphgpu_resample_comp& c, int32_t lo, int32_t hi, uint32_t bx, uint32_t nbx)
{
  if (c.fx == 1 && c.fy == 1) frame_fit_run<TD>(src, dst, (uint64_t)c.dst_w * c.dst_h, c.shift, lo, hi, bx, nbx);
  else if (c.fy == 1) frame_resample_run<TD, 2, 1>(src, dst, c, lo, hi, bx, nbx);
  else if (c.fx == 1) frame_resample_run<TD, 1, 2>(src, dst, c, lo, hi, bx, nbx);
  else frame_resample_run<TD, 2, 2>(src, dst, c, lo, hi, bx, nbx);
}

// grid = (workgroups per component, components)
__global__ __launch_bounds__(WG) void frame_resample_kernel(const int32_t* src, void* dst, int bits, const ojphgpu_resample_comp* __restrict__ comps)
{
  const ojphgpu_resample_comp c = comps[blockIdx.y];
  // (not a resampling: the component is left alone)
  if (c.shift < -31 || c.shift > 31 || c.lo > c.hi || c.fx < 1 || c.fx > 2 || c.fy < 1 || c.fy > 2 || c.px > 1 || c.py > 1) return;
  if (c.dst_w != (c.fx == 2 ? (uint32_t)(((uint64_t)c.src_w + 1u - c.px) / 2u) : c.src_w) ||
      c.dst_h != (c.fy == 2 ? (uint32_t)(((uint64_t)c.src_h + 1u - c.py) / 2u) : c.src_h)) return;
  if (c.dst_w == 0 || c.dst_h == 0) return;
  const uint32_t bx = blockIdx.x, nbx = gridDim.x;
  const int32_t* s = src + c.src_first;
  if (bits == 8) {
    if (c.lo < 0) frame_resample_comp<int8_t>(s, (int8_t*)dst + c.dst_first, c, max(c.lo, -128), min(c.hi, 127), bx, nbx);
    else frame_resample_comp<uint8_t>(s, (uint8_t*)dst + c.dst_first, c, c.lo, min(c.hi, 255), bx, nbx);
  } else if (bits == 16) {
    if (c.lo < 0) frame_resample_comp<int16_t>(s, (int16_t*)dst + c.dst_first, c, max(c.lo, -32768), min(c.hi, 32767), bx, nbx);
    else frame_resample_comp<uint16_t>(s, (uint16_t*)dst + c.dst_first, c, c.lo, min(c.hi, 65535), bx, nbx);
  } else
    frame_resample_comp<int32_t>(s, (int32_t*)dst + c.dst_first, c, c.lo, c.hi, bx, nbx);
}

}  // namespace

extern "C" int ojphgpu_frame_resample(void* stream, const int32_t* d_src, void* d_dst, int container_bits, const ojphgpu_resample_comp* d_comps,
                                      uint32_t n_comps)
{
  if (!d_src || !d_dst || !d_comps || (container_bits != 8 && container_bits != 16 && container_bits != 32)) return OJPHGPU_E_INVALID;
  if (n_comps == 0) return OJPHGPU_OK;
  if (n_comps > 65535u) return OJPHGPU_E_INVALID;
  if (((uintptr_t)d_src & 3u) != 0 || ((uintptr_t)d_dst & (uintptr_t)(container_bits / 8 - 1)) != 0) return OJPHGPU_E_INVALID;
  if ((const void*)d_src == (const void*)d_dst) return OJPHGPU_E_INVALID;    // the layouts differ: never in place
  const uint32_t gx = std::max(1u, 2048u / n_comps);        // as the fit: each workgroup strides over its component's items
  hipLaunchKernelGGL(frame_resample_kernel, dim3(gx, n_comps), dim3(WG), 0, (hipStream_t)stream, d_src, d_dst, container_bits, d_comps);
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

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
