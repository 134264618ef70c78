// openjph_amd/csrc/kernels_stats.hip -- what encoding to a byte budget (include/ojphgpu.h section 5b) adds on the device:
//   band_stats_kernel  half-octave histograms of the magnitudes of the sub-band planes, one pass behind the forward DWT
//   requant_frames_kernel  the blocks' delta / K_max / missing_msbs of another base step into the block descriptors, every
//                      frame of the encoder at a step of its own
//
// The histogram pass reads 4 bytes per coefficient and writes next to nothing: its roof is HBM, like a DWT level's (what it
// reaches of it: DESIGN 1.2), and the counting has to stay out of the loads' way.  The exponents of a real frame sit in ten to twenty bins, so an atomic per
// sample on a shared counter would land on one address and be served one at a time.  Instead a workgroup keeps one table
// of 64 COLUMNS per bin in LDS -- lane l of every wavefront counts in column l, so the 64 adds of one ds_add instruction
// fall into 64 different banks and never meet -- with two bins packed into a word as 16-bit halves (10 KB per workgroup).
// The work is cut into units of 8 rows of one plane; a bounded grid strides over them, so that the units of the large
// planes (three quarters of the samples sit in the nine level-1 bands of a frame) spread over all workgroups.  When the slot
// changes, before a half could overflow, and at the end a workgroup sums the columns of the occupied bins with wavefront
// shuffles and sends at most 80 global atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "ojph_plan.h"

namespace {

constexpr uint32_t BINS = OJPHGPU_STATS_BINS, PAIRS = BINS / 2, COLS = 64;
constexpr uint32_t WG = 256, UNIT_ROWS = 8, WIDE = 32768, MAX_W = 1u << 21;
// a half holds 65535; what a unit can add to one is bounded by the samples its four threads of one lane take (unit_cost)
constexpr uint32_t FLUSH_AT = 60000;

// INT false: u is an fp32 coefficient, the bin its exponent field and top mantissa bit (include/ojphgpu.h, ojphgpu_band_stats);
// INT true: u is an int32 coefficient of a reversible plane, the bin the bit length of |u| -- 0 for 0, 32 for INT_MIN
// (ojphgpu_band_stats_int; section 5f builds on it)
template <bool INT>
__device__ __forceinline__ void count(uint32_t* tab, uint32_t lane, uint32_t u, bool valid)
{
  int e;
  if (INT) {
    const int v = (int)u;
    const uint32_t a = v < 0 ? 0u - u : u;                   // |INT_MIN| = 2^31 as unsigned
    e = 32 - (int)__clz((int)a);                             // (__clz(0) = 32)
  } else {
    e = (int)((u >> 22) & 0x1FFu) - 191;
    e = e < 0 ? 0 : e > (int)BINS - 1 ? (int)BINS - 1 : e;
  }
  // no branch around the add: a sample that does not count adds nothing to the (valid) place its bits name
  atomicAdd(&tab[((uint32_t)e >> 1) * COLS + lane], valid ? 1u << (((uint32_t)e & 1u) * 16u) : 0u);
}

// sums the columns of the table into d_hist[slot] and clears it; every thread of the workgroup calls it
__device__ void flush(uint32_t* tab, uint32_t t, uint32_t* __restrict__ hist, uint32_t slot)
{
  __syncthreads();
  const uint32_t lane = t & 63u, wave = t >> 6;
  for (uint32_t p = wave; p < PAIRS; p += WG / 64) {
    const uint32_t v = tab[p * COLS + lane];
    if (__ballot(v != 0) == 0) continue;                     // (a frame's exponents sit in a quarter of the bins)
    tab[p * COLS + lane] = 0;
    uint32_t lo = v & 0xFFFFu, hi = v >> 16;
    for (int m = 32; m >= 1; m >>= 1) { lo += __shfl_xor(lo, m, 64); hi += __shfl_xor(hi, m, 64); }
    if (lane == 0) {
      if (lo) atomicAdd(&hist[(size_t)slot * BINS + 2 * p], lo);
      if (hi) atomicAdd(&hist[(size_t)slot * BINS + 2 * p + 1], hi);
    }
  }
  __syncthreads();
}

// unit u = (descriptor u / row_units, rows [unit_rows (u % row_units), + unit_rows) of its plane); workgroup b takes units
// b, b + grid, ...  Everything that decides a branch around a barrier is uniform over the workgroup.
template <bool INT>
__global__ __launch_bounds__(WG) void band_stats_kernel(const ojphgpu_stats_desc* __restrict__ descs, uint32_t max_w, uint32_t row_units, uint32_t unit_rows,
                                                        uint32_t units, const uint32_t* __restrict__ coef,
                                                        uint32_t* __restrict__ hist)
{
  __shared__ uint32_t tab[PAIRS * COLS];
  const uint32_t t = threadIdx.x, lane = t & 63u;
  for (uint32_t i = t; i < PAIRS * COLS; i += WG) tab[i] = 0;
  bool pending = false;
  uint32_t cur = 0, acc = 0;
  __syncthreads();
  for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {
    const uint32_t di = u / row_units, y0 = (u - di * row_units) * unit_rows;
    const ojphgpu_stats_desc d = descs[di];
    if (d.w == 0 || d.w > max_w || y0 >= d.h) continue;         // (wider than promised: the bound below would not hold)
    const uint32_t rows = min(unit_rows, d.h - y0);
    const bool vec = ((d.plane_off | d.pitch) & 3u) == 0 && d.pitch >= d.w;
    // the four threads of a lane take at most ceil(items / 256) items each, of 4 samples (vector path) or 1
    const uint32_t unit_cost = vec ? 16u * ((rows * ((d.w + 3u) >> 2) + WG - 1u) / WG) : 4u * ((rows * d.w + WG - 1u) / WG);
    if (pending && (cur != d.slot || acc + unit_cost > FLUSH_AT)) { flush(tab, t, hist, cur); acc = 0; }
    pending = true; cur = d.slot; acc += unit_cost;
    const uint32_t* base = coef + d.plane_off + (uint64_t)y0 * d.pitch;
    if (vec) {
      // rows start on 16-byte boundaries: 16-byte loads, four of them in flight per lane; the loads are unconditional from
      // clamped addresses (the last vector of a row may reach into the pitch padding), the mask is applied at use
      // row and column of an item by a float reciprocal and one correction either way (items < 2^22: exact as floats, the
      // quotient is off by one at most) -- an integer division per load costs more than the counting
      const uint32_t cw = (d.w + 3u) >> 2, items = rows * cw;
      const float inv = 1.0f / (float)cw;
      for (uint32_t i0 = 0; i0 < items; i0 += 4 * WG) {
        uint4 v[4]; uint32_t nv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t it = i0 + (uint32_t)k * WG + t, c = min(it, items - 1u);
          uint32_t r = (uint32_t)((float)c * inv);
          int rem = (int)(c - r * cw);
          if (rem < 0) { --r; rem += (int)cw; } else if (rem >= (int)cw) { ++r; rem -= (int)cw; }
          const uint32_t x = (uint32_t)rem * 4u;
          v[k] = *reinterpret_cast<const uint4*>(base + (uint64_t)r * d.pitch + x);
          nv[k] = it < items ? d.w - x : 0u;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          count<INT>(tab, lane, v[k].x, nv[k] > 0); count<INT>(tab, lane, v[k].y, nv[k] > 1);
          count<INT>(tab, lane, v[k].z, nv[k] > 2); count<INT>(tab, lane, v[k].w, nv[k] > 3);
        }
      }
    } else {
      const uint64_t items = (uint64_t)rows * d.w;
      for (uint64_t i0 = 0; i0 < items; i0 += 4 * WG) {
        uint32_t v[4]; bool ok[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint64_t it = i0 + (uint32_t)k * WG + t, c = it < items ? it : items - 1u;
          const uint64_t r = c / d.w;
          v[k] = base[r * d.pitch + (c - r * d.w)];
          ok[k] = it < items;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) count<INT>(tab, lane, v[k], ok[k]);
      }
    }
  }
  if (pending) flush(tab, t, hist, cur);
}

// descriptor f * nb + i = block i of frame f: the class list is the frame shape's, the table holds a row per frame
__global__ void requant_frames_kernel(ojphgpu_cb_desc* __restrict__ descs, uint32_t nb, uint32_t frames, const uint32_t* __restrict__ cls,
                                      const ojphgpu::BandQuant* __restrict__ q, uint32_t nclasses)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, f = blockIdx.y;
  if (i >= nb || f >= frames) return;
  const ojphgpu::BandQuant b = q[(size_t)f * nclasses + cls[i]];
  ojphgpu_cb_desc& d = descs[(size_t)f * nb + i];
  d.K_max = (uint8_t)b.K_max;
  d.missing_msbs = (uint8_t)(b.K_max - 1u);
  d.delta = b.delta;
}

// a truncation table into the block descriptors (section 5f): block i drops drop[cls[i]] planes.  0 planes: the plan's own
// descriptor (bit 3 clear, missing_msbs = K_max - 1), so level 0 puts back what the encoder was made with.
__global__ void trunc_descs_kernel(ojphgpu_cb_desc* __restrict__ descs, uint32_t nb, const uint32_t* __restrict__ cls,
                                   const uint8_t* __restrict__ drop)
{
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nb) return;
  ojphgpu_cb_desc& d = descs[i];
  const uint32_t top = d.K_max ? d.K_max - 1u : 0u, t = min((uint32_t)drop[cls[i]], top);   // (a flagged block keeps its top plane)
  d.missing_msbs = (uint8_t)(top - t);
  d.reversible = (uint8_t)(t ? d.reversible | 8u : d.reversible & ~8u);
}

}  // namespace

template <bool INT>
static int band_stats_launch(void* stream, const ojphgpu_stats_desc* d_descs, uint32_t n, uint32_t max_w, uint32_t max_h,
                             const void* d_coef, uint32_t* d_hist)
{
  if (!d_descs || !d_coef || !d_hist) return OJPHGPU_E_INVALID;
  if (n == 0 || max_w == 0 || max_h == 0) return OJPHGPU_OK;
  if (max_w > MAX_W) return OJPHGPU_E_INVALID;
  // 8 rows of a plane per unit; planes so wide that 8 rows could overflow a 16-bit half of the table: one row
  const uint32_t unit_rows = max_w > WIDE ? 1u : UNIT_ROWS;
  const uint64_t row_units = ((uint64_t)max_h + unit_rows - 1) / unit_rows, units = row_units * n;
  if (units > 0xFFFFFFFFull) return OJPHGPU_E_INVALID;
  // a bounded grid that strides over the units: eight workgroups per compute unit of the largest part
  const uint32_t grid = (uint32_t)std::min<uint64_t>(units, 2048);
  hipLaunchKernelGGL(band_stats_kernel<INT>, dim3(grid), dim3(WG), 0, (hipStream_t)stream, d_descs,
                     max_w, (uint32_t)row_units, unit_rows, (uint32_t)units, (const uint32_t*)d_coef, d_hist);
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

extern "C" int ojphgpu_band_stats(void* stream, const ojphgpu_stats_desc* d_descs, uint32_t n, uint32_t max_w, uint32_t max_h,
                                  const void* d_coef, uint32_t* d_hist)
{
  return band_stats_launch<false>(stream, d_descs, n, max_w, max_h, d_coef, d_hist);
}

extern "C" int ojphgpu_band_stats_int(void* stream, const ojphgpu_stats_desc* d_descs, uint32_t n, uint32_t max_w, uint32_t max_h,
                                      const void* d_coef, uint32_t* d_hist)
{
  return band_stats_launch<true>(stream, d_descs, n, max_w, max_h, d_coef, d_hist);
}

namespace ojphgpu {

int requant_frames_launch(void* stream, ojphgpu_cb_desc* d_descs, uint32_t nb, uint32_t frames, const uint32_t* d_class, const BandQuant* d_quant,
                          uint32_t nclasses)
{
  if (nb == 0 || frames == 0) return OJPHGPU_OK;
  if (frames > 65535u) return OJPHGPU_E_INVALID;           // (the grid's y extent)
  hipLaunchKernelGGL(requant_frames_kernel, dim3((nb + 255u) / 256u, frames), dim3(256), 0, (hipStream_t)stream, d_descs, nb, frames, d_class,
                     d_quant, nclasses);
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

int trunc_descs_launch(void* stream, ojphgpu_cb_desc* d_descs, uint32_t nb, const uint32_t* d_class, const uint8_t* d_drop)
{
  if (nb == 0) return OJPHGPU_OK;
  hipLaunchKernelGGL(trunc_descs_kernel, dim3((nb + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, d_descs, nb, d_class, d_drop);
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

}  // namespace ojphgpu
