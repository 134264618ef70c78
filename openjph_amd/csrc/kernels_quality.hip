// openjph_amd/csrc/kernels_quality.hip -- what encoding to a quality target (include/ojphgpu.h section 5c) adds on the device:
//   band_requantise_kernel  the sub-band planes as the decoder would hold them after decoding the codestream of another
//                           base step: quantised as the block coder's loads quantise them, cut to the bits the cleanup pass
//                           carries, de-quantised as the block decoder's stores do (ht_quant.h: the same three functions)
//   frame_error_kernel      exact squared error and peak absolute error between two frames, per component; the second frame
//                           may be int32 whatever the first's container (a decoded sample can lie one past its range, which
//                           only int32 hands over as it is: kernels_dwt.hip fit_container)
//
// Both are one pass over HBM with next to no arithmetic: the first reads and writes 4 bytes per coefficient, the second
// reads two frames in their containers.  16-byte loads and stores wherever the addresses allow, scalar edges; nothing is
// written outside the w x h samples of a plane (the padding of the second arena stays what the decoder's would be: zero).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "ht_quant.h"
#include "ojph_plan.h"

namespace {

constexpr uint32_t WG = 256, UNIT_ROWS = 8, MAX_W = 1u << 21;

__device__ __forceinline__ uint32_t requantise(uint32_t raw, float delta_inv, float delta, uint32_t p)
{
  uint32_t over = 0;
  return ojphgpu::dequantise(ojphgpu::coded_word(ojphgpu::to_sign_mag(raw, false, 0, delta_inv, over), p), false, 0, delta);
}

// unit u = (descriptor u / row_units, rows [8 (u % row_units), + 8) of its plane); workgroup b takes units b, b + grid, ...
// (the cut of kernels_stats.hip: the large planes spread over all workgroups)
__global__ __launch_bounds__(WG) void band_requantise_kernel(const ojphgpu_requant_desc* __restrict__ descs, uint32_t max_w, uint32_t row_units,
                                                             uint32_t units, int aligned, const uint32_t* __restrict__ src, uint32_t* __restrict__ dst)
{
  const uint32_t t = threadIdx.x;
  for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
    const uint32_t di = u / row_units, y0 = (u - di * row_units) * UNIT_ROWS;
    const ojphgpu_requant_desc d = descs[di];
    // (wider than promised: the item arithmetic below would not hold; a K_max the half bit has no room under: no such band)
    if (d.w == 0 || d.w > max_w || y0 >= d.h || d.K_max == 0 || d.K_max > 30) continue;
    const uint32_t rows = min(UNIT_ROWS, d.h - y0), p = 31u - d.K_max;
    const uint64_t base = d.plane_off + (uint64_t)y0 * d.pitch;
    if (aligned && ((d.plane_off | d.pitch) & 3u) == 0 && d.pitch >= d.w) {
      // rows start on 16-byte boundaries: an item is four samples of a row, whole ones as one 16-byte load and store, the
      // last of a row whose width is no multiple of four sample by sample.  Row and column of an item by a float
      // reciprocal and one correction either way (items <= 2^22: exact as floats, the quotient is off by one at most)
      const uint32_t cw = (d.w + 3u) >> 2, items = rows * cw;
      const float inv = 1.0f / (float)cw;
      for (uint32_t it = t; it < items; it += WG) {
        uint32_t r = (uint32_t)((float)it * inv);
        int rem = (int)(it - r * cw);
        if (rem < 0) { --r; rem += (int)cw; } else if (rem >= (int)cw) { ++r; rem -= (int)cw; }
        const uint32_t x = (uint32_t)rem * 4u;
        const uint64_t at = base + (uint64_t)r * d.pitch + x;
        if (x + 4u <= d.w) {
          uint4 v = *reinterpret_cast<const uint4*>(src + at);
          v.x = requantise(v.x, d.delta_inv, d.delta, p); v.y = requantise(v.y, d.delta_inv, d.delta, p);
          v.z = requantise(v.z, d.delta_inv, d.delta, p); v.w = requantise(v.w, d.delta_inv, d.delta, p);
          *reinterpret_cast<uint4*>(dst + at) = v;
        } else
          for (uint32_t k = 0; x + k < d.w; ++k) dst[at + k] = requantise(src[at + k], d.delta_inv, d.delta, p);
      }
    } else {
      const uint64_t items = (uint64_t)rows * d.w;
      for (uint64_t it = t; it < items; it += WG) {
        const uint64_t r = it / d.w, at = base + r * d.pitch + (it - r * d.w);
        dst[at] = requantise(src[at], d.delta_inv, d.delta, p);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
struct Err { uint64_t sse; uint32_t pae; };

template <typename TA, typename TB> __device__ __forceinline__ void add_pair(Err& e, TA a, TB b)
{
  if constexpr (sizeof(TA) == 4 || sizeof(TB) == 4) {       // (int32 samples: the difference needs 33 bits)
    const int64_t d = (int64_t)a - (int64_t)b;
    const uint64_t m = (uint64_t)(d < 0 ? -d : d);
    e.sse += m * m; e.pae = max(e.pae, (uint32_t)m);
  } else {                                                  // |d| < 2^16: its square fits 32 bits, the sum does not
    const int d = (int)a - (int)b;
    const uint32_t m = (uint32_t)(d < 0 ? -d : d);
    e.sse += (uint64_t)(m * m); e.pae = max(e.pae, m);
  }
}

// the elements [0, count) of a and b: the part of this workgroup (bx of nbx) and this thread.  The two frames may sit in
// containers of different widths: a group is what 16 bytes of the narrower one hold, NA / NB 16-byte loads of each.
template <typename TA, typename TB>
__device__ void frame_error_run(Err& e, const TA* __restrict__ a, const TB* __restrict__ b, uint64_t count, uint32_t bx, uint32_t nbx)
{
  constexpr uint32_t G = 16 / (sizeof(TA) < sizeof(TB) ? sizeof(TA) : sizeof(TB));
  constexpr int NA = (int)(G * sizeof(TA) / 16), NB = (int)(G * sizeof(TB) / 16);
  constexpr int U = (NA > NB ? NA : NB) >= 4 ? 1 : (NA > NB ? NA : NB) == 2 ? 2 : 4;      // groups in flight: four loads of the wider frame
  const uint32_t t = threadIdx.x;
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  // scalar head up to the first element at which both frames stand on a 16-byte boundary (containers are naturally
  // aligned; the narrower frame decides where that can be), whole groups, scalar tail
  const uint64_t to_a = ((16u - (pa & 15u)) & 15u) / sizeof(TA), to_b = ((16u - (pb & 15u)) & 15u) / sizeof(TB);
  const uint64_t to_boundary = sizeof(TA) <= sizeof(TB) ? to_a : to_b;
  if (((pa + to_boundary * sizeof(TA)) & 15u) != 0 || ((pb + to_boundary * sizeof(TB)) & 15u) != 0) {
    // the two frames sit differently in their 16 bytes: sample by sample
    for (uint64_t i = (uint64_t)bx * WG + t; i < count; i += (uint64_t)nbx * WG) add_pair<TA, TB>(e, a[i], b[i]);
    return;
  }
  const uint64_t head = count < to_boundary ? count : to_boundary;
  const uint64_t ng = (count - head) / G, tail0 = head + ng * G;
  if (bx == 0) {
    if (t < head) add_pair<TA, TB>(e, a[t], b[t]);
    if (tail0 + t < count) add_pair<TA, TB>(e, a[tail0 + t], b[tail0 + t]);
  }
  const uint4* va = reinterpret_cast<const uint4*>(a + head);
  const uint4* vb = reinterpret_cast<const uint4*>(b + head);
  const uint64_t stride = (uint64_t)nbx * WG;
  for (uint64_t g0 = (uint64_t)bx * WG + t; g0 < ng; g0 += U * stride) {
    uint4 xa[U][NA], xb[U][NB]; bool ok[U];
#pragma unroll
    for (int k = 0; k < U; ++k) {
      const uint64_t g = g0 + (uint64_t)k * stride;
      ok[k] = g < ng;
      const uint64_t c = ok[k] ? g : g0;                    // (a clamped address; the group is not counted)
#pragma unroll
      for (int i = 0; i < NA; ++i) xa[k][i] = va[c * NA + i];
#pragma unroll
      for (int i = 0; i < NB; ++i) xb[k][i] = vb[c * NB + i];
    }
#pragma unroll
    for (int k = 0; k < U; ++k) {
      if (!ok[k]) continue;
      TA ea[G]; TB eb[G];
      __builtin_memcpy(ea, xa[k], sizeof(ea)); __builtin_memcpy(eb, xb[k], sizeof(eb));
#pragma unroll
      for (uint32_t i = 0; i < G; ++i) add_pair<TA, TB>(e, ea[i], eb[i]);
    }
  }
}

// b in the same container as a (bits_b == bits_a) or in int32 (bits_b == 32)
template <typename TA>
__device__ __forceinline__ void frame_error_comp(Err& e, const void* fa, const void* fb, bool wide_b, const ojphgpu_error_comp& c, uint32_t bx, uint32_t nbx)
{
  if (wide_b) frame_error_run<TA, int32_t>(e, (const TA*)fa + c.first_elem, (const int32_t*)fb + c.first_elem, c.count, bx, nbx);
  else frame_error_run<TA, TA>(e, (const TA*)fa + c.first_elem, (const TA*)fb + c.first_elem, c.count, bx, nbx);
}

// grid = (workgroups per component, components).  64 bits per lane, wavefront shuffles, one atomic per workgroup and
// component for each of the two figures: integer sums, so the result does not depend on the order.
__global__ __launch_bounds__(WG) void frame_error_kernel(const void* __restrict__ fa, int bits_a, const void* __restrict__ fb, int bits_b,
                                                         const ojphgpu_error_comp* __restrict__ comps, ojphgpu_frame_err* __restrict__ out)
{
  __shared__ uint64_t s_sse[WG / 64];
  __shared__ uint32_t s_pae[WG / 64];
  const ojphgpu_error_comp c = comps[blockIdx.y];
  Err e{ 0, 0 };
  const uint32_t bx = blockIdx.x, nbx = gridDim.x;
  const bool wide_b = bits_b != bits_a;
  if (bits_a == 8) {
    if (c.is_signed) frame_error_comp<int8_t>(e, fa, fb, wide_b, c, bx, nbx); else frame_error_comp<uint8_t>(e, fa, fb, wide_b, c, bx, nbx);
  } else if (bits_a == 16) {
    if (c.is_signed) frame_error_comp<int16_t>(e, fa, fb, wide_b, c, bx, nbx); else frame_error_comp<uint16_t>(e, fa, fb, wide_b, c, bx, nbx);
  } else
    frame_error_run<int32_t, int32_t>(e, (const int32_t*)fa + c.first_elem, (const int32_t*)fb + c.first_elem, c.count, bx, nbx);
  for (int m = 32; m >= 1; m >>= 1) {
    e.sse += (uint64_t)__shfl_xor((unsigned long long)e.sse, m, 64);
    e.pae = max(e.pae, (uint32_t)__shfl_xor((int)e.pae, m, 64));
  }
  const uint32_t t = threadIdx.x;
  if ((t & 63u) == 0) { s_sse[t >> 6] = e.sse; s_pae[t >> 6] = e.pae; }
  __syncthreads();
  if (t == 0) {
    uint64_t sse = 0; uint32_t pae = 0;
    for (uint32_t w = 0; w < WG / 64; ++w) { sse += s_sse[w]; pae = max(pae, s_pae[w]); }
    if (sse) atomicAdd((unsigned long long*)&out[blockIdx.y].sse, (unsigned long long)sse);
    if (pae) atomicMax(&out[blockIdx.y].pae, pae);
  }
}

}  // namespace

extern "C" int ojphgpu_band_requantise(void* stream, const ojphgpu_requant_desc* d_descs, uint32_t n, uint32_t max_w, uint32_t max_h,
                                       const void* d_src_arena, void* d_dst_arena)
{
  if (!d_descs || !d_src_arena || !d_dst_arena) return OJPHGPU_E_INVALID;
  if (n == 0 || max_w == 0 || max_h == 0) return OJPHGPU_OK;
  if (max_w > MAX_W) return OJPHGPU_E_INVALID;
  const uint64_t row_units = ((uint64_t)max_h + UNIT_ROWS - 1) / UNIT_ROWS, units = row_units * n;
  if (units > 0xFFFFFFFFull) return OJPHGPU_E_INVALID;
  const int aligned = (((uintptr_t)d_src_arena | (uintptr_t)d_dst_arena) & 15u) == 0;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(units, 4096);
  hipLaunchKernelGGL(band_requantise_kernel, dim3(grid), dim3(WG), 0, (hipStream_t)stream, d_descs, max_w, (uint32_t)row_units,
                     (uint32_t)units, aligned, (const uint32_t*)d_src_arena, (uint32_t*)d_dst_arena);
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

extern "C" int ojphgpu_frame_error_ex(void* stream, const void* d_a, int bits_a, const void* d_b, int bits_b, const ojphgpu_error_comp* d_comps,
                                      uint32_t n_comps, ojphgpu_frame_err* d_out)
{
  if (!d_a || !d_b || !d_comps || !d_out || (bits_a != 8 && bits_a != 16 && bits_a != 32) || (bits_b != bits_a && bits_b != 32)) return OJPHGPU_E_INVALID;
  if (n_comps == 0) return OJPHGPU_OK;
  if (n_comps > 65535u) return OJPHGPU_E_INVALID;
  // the frames must be containers in their natural alignment (the head of a run is counted up to a 16-byte boundary)
  if (((uintptr_t)d_a & (uintptr_t)(bits_a / 8 - 1)) != 0 || ((uintptr_t)d_b & (uintptr_t)(bits_b / 8 - 1)) != 0) return OJPHGPU_E_INVALID;
  // about 2048 workgroups over the components (eight per compute unit), each striding over its component's run
  const uint32_t gx = std::max(1u, 2048u / n_comps);
  hipLaunchKernelGGL(frame_error_kernel, dim3(gx, n_comps), dim3(WG), 0, (hipStream_t)stream, d_a, bits_a, d_b, bits_b, d_comps, d_out);
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

extern "C" int ojphgpu_frame_error(void* stream, const void* d_a, const void* d_b, int container_bits, const ojphgpu_error_comp* d_comps,
                                   uint32_t n_comps, ojphgpu_frame_err* d_out)
{
  return ojphgpu_frame_error_ex(stream, d_a, container_bits, d_b, container_bits, d_comps, n_comps, d_out);
}
