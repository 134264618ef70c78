// openjph_amd/csrc/kernels_video.hip -- 4:2:2 video buffers as capture cards, SDI / ST 2110 receivers and display paths
// hold them (UYVY and YUY2 at 8 bits, v210 at 10, Y210 / Y212 / Y216 above; ojphgpu.h section 7b) <-> the planar sample
// containers the codec works on (Y [H][W], then Cb and Cr [H][ceil(W / 2)], 8 / 16 / 32 bits per sample).
//
// No counterpart in the reference, whose readers take planar .yuv files (yuv_in::read, src/apps/others/ojph_img_io.cpp)
// sample by sample on the host.  Pure data movement, HBM-bound, next to unpack_kernel / pack_kernel of kernels_pixels.hip.
//
// A lane owns one UNIT of one row: a run of consecutive pairs (Y0 Y1 Cb Cr) whose bytes are a multiple of 16 on the packed
// side and in every plane, so that whatever alignment a row starts at holds for every unit of that row:
//   v210          24 pairs = 8 groups = 128 bytes: the 48 pixels a v210 row is padded to, so a row is a whole number of
//                 units and 16-byte aligned by construction; 48 luma + 2 x 24 chroma = 96 + 2 x 48 bytes of 16-bit containers
//   UYVY / YUY2   16 pairs = 64 bytes into 8-bit containers (32 + 2 x 16 bytes), 8 pairs = 32 bytes into wider ones
//   Y2XX          8 pairs = 64 bytes (32 + 2 x 16 bytes of 16-bit containers)
// A wavefront is 64 units of ONE row (the workgroup is 64 x 4: four rows), so the alignment of the row on the packed side
// and in each of the three planes is the same in every lane: the kernel picks, per row and per stream, the widest piece (16,
// 8, 4, 2, 1 bytes) that address allows, by a wave-uniform branch.  The last unit of a row, when the row does not fill it,
// goes a pair (v210: a group) at a time and sample by sample in the planes, its loads unconditional from clamped indices.
// No division, no LDS, no scratch: a unit lives in registers as dwords (`put` / `get` address them with compile-time
// indices).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ojphgpu.h"
#include "kernels_video_pieces.h"
#include "video_formats.h"

namespace {

enum { UYVY = OJPHGPU_VIDEO_UYVY, YUY2 = OJPHGPU_VIDEO_YUY2, V210 = OJPHGPU_VIDEO_V210, Y2XX = OJPHGPU_VIDEO_Y2XX };

template <int F, typename D> struct Unit {
  static constexpr int NP = F == V210 ? 24 : (F == Y2XX ? 8 : (sizeof(D) == 1 ? 16 : 8));   // pairs
  static constexpr int PAIR_WORDS = F == Y2XX ? 2 : 1;                                       // dwords of a pair (not v210)
  static constexpr int PW = F == V210 ? 32 : NP * PAIR_WORDS;                                // dwords on the packed side
  static constexpr int YW = 2 * NP * (int)sizeof(D) / 4, CW = NP * (int)sizeof(D) / 4;       // dwords in the planes
};

// pair k of a unit's packed dwords; sh = 16 - bit depth (Y2XX).  v210: the unit's 96 fields in order are the pairs' Cb Y0
// Cr Y1, field q in bits [10 * (q % 3), +10) of dword q / 3
template <int F> __device__ __forceinline__ void get_pair(const uint32_t* pw, int k, uint32_t sh, uint32_t& y0, uint32_t& y1, uint32_t& cb, uint32_t& cr)
{
  if (F == UYVY) { const uint32_t d = pw[k]; cb = d & 0xFFu; y0 = (d >> 8) & 0xFFu; cr = (d >> 16) & 0xFFu; y1 = d >> 24; }
  else if (F == YUY2) { const uint32_t d = pw[k]; y0 = d & 0xFFu; cb = (d >> 8) & 0xFFu; y1 = (d >> 16) & 0xFFu; cr = d >> 24; }
  else if (F == Y2XX) {
    const uint32_t a = pw[2 * k], b = pw[2 * k + 1];
    y0 = (a & 0xFFFFu) >> sh; cb = (a >> 16) >> sh; y1 = (b & 0xFFFFu) >> sh; cr = (b >> 16) >> sh;
  } else {
    const int q = 4 * k;
    cb = (pw[q / 3] >> (10 * (q % 3))) & 0x3FFu;             y0 = (pw[(q + 1) / 3] >> (10 * ((q + 1) % 3))) & 0x3FFu;
    cr = (pw[(q + 2) / 3] >> (10 * ((q + 2) % 3))) & 0x3FFu; y1 = (pw[(q + 3) / 3] >> (10 * ((q + 3) % 3))) & 0x3FFu;
  }
}
// the way back into zeroed dwords; the values are inside [0, 2^depth - 1]
template <int F> __device__ __forceinline__ void put_pair(uint32_t* pw, int k, uint32_t sh, uint32_t y0, uint32_t y1, uint32_t cb, uint32_t cr)
{
  if (F == UYVY) pw[k] = cb | y0 << 8 | cr << 16 | y1 << 24;
  else if (F == YUY2) pw[k] = y0 | cb << 8 | y1 << 16 | cr << 24;
  else if (F == Y2XX) { pw[2 * k] = (y0 << sh) | (cb << sh) << 16; pw[2 * k + 1] = (y1 << sh) | (cr << sh) << 16; }
  else {
    const int q = 4 * k;
    pw[q / 3] |= cb << (10 * (q % 3));             pw[(q + 1) / 3] |= y0 << (10 * ((q + 1) % 3));
    pw[(q + 2) / 3] |= cr << (10 * ((q + 2) % 3)); pw[(q + 3) / 3] |= y1 << (10 * ((q + 3) % 3));
  }
}

// the rows' geometry, the same for both directions: planes = Y [height][width], Cb, Cr [height][cw]
struct Geo { uint32_t width, height, cw, row_bytes, units, shift; };

// the row's last unit when the row does not fill it: STEP pairs at a time (a v210 group, a pair of the others), not unrolled
template <int F> struct Step {
  static constexpr int NP = F == V210 ? 3 : 1, W = F == V210 ? 4 : (F == Y2XX ? 2 : 1);     // pairs, dwords
};
template <int F> __device__ __forceinline__ void load_step(const uint8_t* q, uint32_t* w)
{
  if (F == V210) { const uint4 v = *(const uint4*)q; w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
  else if (F == Y2XX) { const uint2 v = *(const uint2*)q; w[0] = v.x; w[1] = v.y; }
  else w[0] = *(const uint32_t*)q;
}
template <int F> __device__ __forceinline__ void store_step(uint8_t* q, const uint32_t* w)
{
  if (F == V210) *(uint4*)q = make_uint4(w[0], w[1], w[2], w[3]);
  else if (F == Y2XX) *(uint2*)q = make_uint2(w[0], w[1]);
  else *(uint32_t*)q = w[0];
}

template <int F, typename D>
__global__ __launch_bounds__(256) void unpack_video_kernel(const uint8_t* __restrict__ src, D* __restrict__ dst, Geo g)
{
  typedef Unit<F, D> U;
  typedef Step<F> S;
  const uint32_t u = blockIdx.x * 64u + threadIdx.x;
  if (u >= g.units) return;
  const uint32_t k0 = u * U::NP;                       // first pair of the unit
  const bool full = 2ull * ((uint64_t)k0 + U::NP) <= g.width;
  const size_t ysz = (size_t)g.width * g.height, csz = (size_t)g.cw * g.height;
  for (uint32_t y = blockIdx.y * 4u + threadIdx.y; y < g.height; y += gridDim.y * 4u) {
    const uint8_t* prow = src + (size_t)y * g.row_bytes;
    D* yrow = dst + (size_t)y * g.width;
    D* brow = dst + ysz + (size_t)y * g.cw;
    D* rrow = brow + csz;
    if (full) {
      uint32_t pw[U::PW];
      load_words<U::PW, F == Y2XX ? 8 : 4>(prow + (size_t)u * (U::PW * 4), pw, F == V210 ? 0u : uniform((uint32_t)(uintptr_t)prow));
      uint32_t wy[U::YW], wb[U::CW], wr[U::CW];
      if (sizeof(D) != 4) {
#pragma unroll
        for (int i = 0; i < U::YW; ++i) wy[i] = 0;
#pragma unroll
        for (int i = 0; i < U::CW; ++i) wb[i] = wr[i] = 0;
      }
#pragma unroll
      for (int k = 0; k < U::NP; ++k) {
        uint32_t y0, y1, cb, cr;
        get_pair<F>(pw, k, g.shift, y0, y1, cb, cr);
        put<D>(wy, 2 * k, y0); put<D>(wy, 2 * k + 1, y1); put<D>(wb, k, cb); put<D>(wr, k, cr);
      }
      store_words<U::YW, sizeof(D)>((uint8_t*)(yrow + 2 * (size_t)k0), wy, uniform((uint32_t)(uintptr_t)yrow));
      store_words<U::CW, sizeof(D)>((uint8_t*)(brow + k0), wb, uniform((uint32_t)(uintptr_t)brow));
      store_words<U::CW, sizeof(D)>((uint8_t*)(rrow + k0), wr, uniform((uint32_t)(uintptr_t)rrow));
    } else {                                           // sample by sample, what the row holds of the unit
      const uint8_t* q = prow + (size_t)u * (U::PW * 4);
#pragma unroll 1
      for (uint32_t k = k0; k < g.cw; k += S::NP, q += S::W * 4) {
        uint32_t w[S::W];
        load_step<F>(q, w);
#pragma unroll
        for (int t = 0; t < S::NP; ++t) {
          uint32_t y0, y1, cb, cr;
          get_pair<F>(w, t, g.shift, y0, y1, cb, cr);
          const uint32_t kk = k + t;
          if (2 * kk < g.width) yrow[2 * (size_t)kk] = (D)y0;
          if (2 * kk + 1 < g.width) yrow[2 * (size_t)kk + 1] = (D)y1;
          if (kk < g.cw) { brow[kk] = (D)cb; rrow[kk] = (D)cr; }
        }
      }
    }
  }
}

// planes -> the video buffer; samples clamped to [0, maxv] as pack_kernel does; every byte of the rows is written, padding as zero
template <int F, typename D>
__global__ __launch_bounds__(256) void pack_video_kernel(const D* __restrict__ src, uint8_t* __restrict__ dst, Geo g, int32_t maxv)
{
  typedef Unit<F, D> U;
  typedef Step<F> S;
  const uint32_t u = blockIdx.x * 64u + threadIdx.x;
  if (u >= g.units) return;
  const uint32_t k0 = u * U::NP;
  const bool full = 2ull * ((uint64_t)k0 + U::NP) <= g.width;
  const size_t ysz = (size_t)g.width * g.height, csz = (size_t)g.cw * g.height;
  for (uint32_t y = blockIdx.y * 4u + threadIdx.y; y < g.height; y += gridDim.y * 4u) {
    uint8_t* prow = dst + (size_t)y * g.row_bytes;
    const D* yrow = src + (size_t)y * g.width;
    const D* brow = src + ysz + (size_t)y * g.cw;
    const D* rrow = brow + csz;
    if (full) {
      uint32_t wy[U::YW], wb[U::CW], wr[U::CW];
      load_words<U::YW, sizeof(D)>((const uint8_t*)(yrow + 2 * (size_t)k0), wy, uniform((uint32_t)(uintptr_t)yrow));
      load_words<U::CW, sizeof(D)>((const uint8_t*)(brow + k0), wb, uniform((uint32_t)(uintptr_t)brow));
      load_words<U::CW, sizeof(D)>((const uint8_t*)(rrow + k0), wr, uniform((uint32_t)(uintptr_t)rrow));
      uint32_t pw[U::PW];
      if (F == V210) {
#pragma unroll
        for (int i = 0; i < U::PW; ++i) pw[i] = 0;
      }
#pragma unroll
      for (int k = 0; k < U::NP; ++k)
        put_pair<F>(pw, k, g.shift, clamp_sample(get<D>(wy, 2 * k), maxv), clamp_sample(get<D>(wy, 2 * k + 1), maxv),
                    clamp_sample(get<D>(wb, k), maxv), clamp_sample(get<D>(wr, k), maxv));
      store_words<U::PW, F == Y2XX ? 8 : 4>(prow + (size_t)u * (U::PW * 4), pw, F == V210 ? 0u : uniform((uint32_t)(uintptr_t)prow));
    } else {
      // the row's last unit: sample by sample, the loads unconditional from clamped indices; what lies beyond the row packs
      // as zero, and of a v210 unit every group is written: the padding
      uint8_t* q = prow + (size_t)u * (U::PW * 4);
      const uint32_t kend = F == V210 ? k0 + U::NP : g.cw;
#pragma unroll 1
      for (uint32_t k = k0; k < kend; k += S::NP, q += S::W * 4) {
        uint32_t w[S::W];
#pragma unroll
        for (int i = 0; i < S::W; ++i) w[i] = 0;
#pragma unroll
        for (int t = 0; t < S::NP; ++t) {
          const uint32_t kk = k + t, xa = 2 * kk, xb = 2 * kk + 1;
          const int32_t a = (int32_t)yrow[xa < g.width ? xa : g.width - 1], b = (int32_t)yrow[xb < g.width ? xb : g.width - 1];
          const int32_t c = (int32_t)brow[kk < g.cw ? kk : g.cw - 1], d = (int32_t)rrow[kk < g.cw ? kk : g.cw - 1];
          put_pair<F>(w, t, g.shift, xa < g.width ? clamp_sample(a, maxv) : 0u, xb < g.width ? clamp_sample(b, maxv) : 0u,
                      kk < g.cw ? clamp_sample(c, maxv) : 0u, kk < g.cw ? clamp_sample(d, maxv) : 0u);
        }
        store_step<F>(q, w);
      }
    }
  }
}

template <int F, typename D>
int launch(hipStream_t st, bool unpack, const void* src, void* dst, const Geo& g, uint32_t bit_depth)
{
  const uint32_t rows4 = (g.height + 3) / 4;
  const dim3 grid((g.units + 63) / 64, rows4 < 65535u ? rows4 : 65535u), wg(64, 4);
  if (unpack) hipLaunchKernelGGL((unpack_video_kernel<F, D>), grid, wg, 0, st, (const uint8_t*)src, (D*)dst, g);
  else hipLaunchKernelGGL((pack_video_kernel<F, D>), grid, wg, 0, st, (const D*)src, (uint8_t*)dst, g, (int32_t)((1u << bit_depth) - 1u));
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

template <int F>
int launch_container(hipStream_t st, bool unpack, const void* src, void* dst, const Geo& g, uint32_t bit_depth, int container_bits)
{
  if (container_bits == 16) return launch<F, uint16_t>(st, unpack, src, dst, g, bit_depth);
  return launch<F, int32_t>(st, unpack, src, dst, g, bit_depth);
}

int run(void* stream, bool unpack, int format, const void* d_video, const void* d_planes, uint32_t width, uint32_t height,
        uint32_t bit_depth, int container_bits)
{
  Geo g{};
  uint64_t chroma_offset = 0, frame_bytes = 0;
  const VideoDesc* v = video_desc(format, OJPHGPU_VIDEO_FAMILY_422);
  if (!d_video || !d_planes || !video_check(v, width, height, bit_depth, container_bits)) return OJPHGPU_E_INVALID;
  if (!video_layout(v, width, height, &g.row_bytes, &chroma_offset, &frame_bytes) || ((uintptr_t)d_video & (v->r.pointer_align - 1))) return OJPHGPU_E_INVALID;
  g.width = width; g.height = height; g.cw = (uint32_t)(((uint64_t)width + 1) / 2);
  g.shift = format == Y2XX ? 16u - bit_depth : 0u;
  const uint32_t np = format == V210 ? 24u : (format == Y2XX || container_bits != 8 ? 8u : 16u);
  g.units = (g.cw + np - 1) / np;
  hipStream_t st = (hipStream_t)stream;
  const void* src = unpack ? d_video : d_planes;
  void* dst = const_cast<void*>(unpack ? d_planes : d_video);
  switch (format) {
    case UYVY: return container_bits == 8 ? launch<UYVY, uint8_t>(st, unpack, src, dst, g, bit_depth) : launch_container<UYVY>(st, unpack, src, dst, g, bit_depth, container_bits);
    case YUY2: return container_bits == 8 ? launch<YUY2, uint8_t>(st, unpack, src, dst, g, bit_depth) : launch_container<YUY2>(st, unpack, src, dst, g, bit_depth, container_bits);
    case V210: return launch_container<V210>(st, unpack, src, dst, g, bit_depth, container_bits);
    default: return launch_container<Y2XX>(st, unpack, src, dst, g, bit_depth, container_bits);
  }
}

}  // namespace

extern "C" int ojphgpu_video_format_info(int format, ojphgpu_video_info* out)
{
  const VideoDesc* v = video_desc(format);
  if (v && out) *out = v->r;
  return v && out ? OJPHGPU_OK : OJPHGPU_E_INVALID;
}

extern "C" int ojphgpu_video_layout(int format, uint32_t width, uint32_t height, uint32_t* row_bytes, uint64_t* frame_bytes)
{
  uint64_t chroma_offset = 0;
  if (!row_bytes || !frame_bytes) return OJPHGPU_E_INVALID;
  return video_layout(video_desc(format, OJPHGPU_VIDEO_FAMILY_422), width, height, row_bytes, &chroma_offset, frame_bytes) ? OJPHGPU_OK : OJPHGPU_E_INVALID;
}

extern "C" int ojphgpu_unpack_video(void* stream, int format, const void* d_video, void* d_planes, uint32_t width, uint32_t height,
                                     uint32_t bit_depth, int container_bits)
{
  return run(stream, true, format, d_video, d_planes, width, height, bit_depth, container_bits);
}

extern "C" int ojphgpu_pack_video(void* stream, int format, const void* d_planes, void* d_video, uint32_t width, uint32_t height,
                                   int container_bits, uint32_t bit_depth)
{
  return run(stream, false, format, d_video, d_planes, width, height, bit_depth, container_bits);
}
