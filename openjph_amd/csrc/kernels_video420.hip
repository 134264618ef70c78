// openjph_amd/csrc/kernels_video420.hip -- 4:2:0 video buffers as hardware video decoders and encoders, ffmpeg's hardware
// frames and most 8-bit and HDR delivery paths hold them (NV12 / NV21 at 8 bits, P010 / P012 / P016 above; ojphgpu.h section
// 7c): a luma plane and a plane of interleaved (Cb, Cr) pairs, each with its own pitch <-> the planar sample containers the
// codec works on (Y [H][W], then Cb and Cr [ceil(H / 2)][ceil(W / 2)], 8 / 16 / 32 bits per sample).
//
// No counterpart in the reference, whose readers take planar .yuv files (yuv_in::read, src/apps/others/ojph_img_io.cpp)
// sample by sample on the host.  Pure data movement, HBM-bound, written the way the finding of DESIGN 1.4 asks: a lane takes
// a SMALL piece, so that one load or store instruction of a wavefront covers contiguous whole 128-byte lines.
//
// On the video side a luma row and a chroma row look the same: cw = ceil(W / 2) PAIRS of two elements (Y[2k] Y[2k + 1], the
// second one padding in the last pair of an odd row; Cb[k] Cr[k]), row_bytes = cw pairs.  One launch runs over the H + ch
// rows of both planes.  A lane takes 8 / sizeof(container) consecutive pairs of one row:
//   the planes      16 bytes of a luma row, or 8 bytes of the Cb row and 8 of the Cr row
//   the video side  16, 8 or 4 bytes (NV12 into 8-, 16-, 32-bit containers), 16 or 8 (P0XX into 16-, 32-bit ones)
// each moved by ONE instruction when the row's address allows, next to the neighbour lanes': an instruction of a wavefront
// covers 256 to 1024 contiguous bytes.  A wavefront is 64 such pieces of ONE row (the workgroup is 64 x 4: four rows), so the
// alignment of the row on the video side and in the planes is the same in every lane, and rows of any alignment -- a chroma
// plane 2 bytes off a dword, a pitch that shifts every row -- stay correct through the wave-uniform choice of piece width of
// kernels_video_pieces.h.  The last piece of a row, when the row does not fill it, goes pair by pair.  NV21 is NV12 with the
// two chroma planes' pointers exchanged.  No division, no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ojphgpu.h"
#include "kernels_video_pieces.h"
#include "video_formats.h"

namespace {

// V: element of the video side (uint8_t: NV12 / NV21; uint16_t: P0XX); D: container of the planes
template <typename V, typename D> struct Piece {
  static constexpr int NP = 8 / (int)sizeof(D);                              // pairs
  static constexpr int VW = 2 * NP * (int)sizeof(V) / 4;                      // dwords on the video side
  static constexpr int YW = 4, CW = 2;                                       // dwords of a luma row, of each chroma row
};

// the two planes' geometry, the same for both directions: planes = Y [height][width], Cb, Cr [ch][cw]
struct Geo420 { uint32_t width, height, cw, ch, pieces, shift, luma_pitch, chroma_pitch; };

// the pair at q as one element of twice the width
template <typename V> __device__ __forceinline__ uint32_t load_pair(const uint8_t* q)
{
  return sizeof(V) == 1 ? (uint32_t)*(const uint16_t*)q : *(const uint32_t*)q;
}
template <typename V> __device__ __forceinline__ void store_pair(uint8_t* q, uint32_t a, uint32_t b)
{
  if (sizeof(V) == 1) *(uint16_t*)q = (uint16_t)(a | b << 8);
  else *(uint32_t*)q = a | b << 16;
}

template <typename V, typename D>
__global__ __launch_bounds__(256) void unpack_video420_kernel(const uint8_t* __restrict__ luma, const uint8_t* __restrict__ chroma,
                                                              D* __restrict__ dst, Geo420 g, bool crcb)
{
  typedef Piece<V, D> P;
  const uint32_t u = blockIdx.x * 64u + threadIdx.x;
  if (u >= g.pieces) return;
  const uint32_t k0 = u * P::NP;                       // first pair of the piece
  const bool fits = (uint64_t)k0 + P::NP <= g.cw;      // (a chroma piece; a luma piece also needs its last sample)
  const uint32_t kend = fits ? k0 + P::NP : g.cw;
  const uint32_t rows = g.height + g.ch;
  const size_t ysz = (size_t)g.width * g.height, csz = (size_t)g.cw * g.ch;
  D* const cplane0 = dst + ysz + (crcb ? csz : 0);     // where the first element of a chroma pair goes
  D* const cplane1 = dst + ysz + (crcb ? 0 : csz);
  for (uint64_t r = blockIdx.y * 4u + threadIdx.y; r < rows; r += gridDim.y * 4u) {
    const bool is_luma = r < g.height;                 // (wave-uniform: a wavefront is one row)
    const uint32_t y = (uint32_t)(is_luma ? r : r - g.height);
    const uint8_t* vrow = is_luma ? luma + (size_t)y * g.luma_pitch : chroma + (size_t)y * g.chroma_pitch;
    D* row0 = is_luma ? dst + (size_t)y * g.width : cplane0 + (size_t)y * g.cw;
    D* row1 = cplane1 + (size_t)y * g.cw;
    const uint32_t val = uniform((uint32_t)(uintptr_t)vrow), al0 = uniform((uint32_t)(uintptr_t)row0), al1 = uniform((uint32_t)(uintptr_t)row1);
    if (fits && (!is_luma || 2ull * ((uint64_t)k0 + P::NP) <= g.width)) {
      uint32_t pw[P::VW];
      load_run<P::VW, 2 * sizeof(V)>(vrow + (size_t)u * (P::VW * 4), pw, val);
      if (is_luma) {
        uint32_t wy[P::YW] = { 0, 0, 0, 0 };
#pragma unroll
        for (int j = 0; j < 2 * P::NP; ++j) put<D>(wy, j, (uint32_t)get<V>(pw, j) >> g.shift);
        store_run<P::YW, sizeof(D)>((uint8_t*)(row0 + 2 * (size_t)k0), wy, al0);
      } else {
        uint32_t w0[P::CW] = { 0, 0 }, w1[P::CW] = { 0, 0 };
#pragma unroll
        for (int k = 0; k < P::NP; ++k) {
          put<D>(w0, k, (uint32_t)get<V>(pw, 2 * k) >> g.shift);
          put<D>(w1, k, (uint32_t)get<V>(pw, 2 * k + 1) >> g.shift);
        }
        store_run<P::CW, sizeof(D)>((uint8_t*)(row0 + k0), w0, al0);
        store_run<P::CW, sizeof(D)>((uint8_t*)(row1 + k0), w1, al1);
      }
    } else {                                           // pair by pair, what the row holds of the piece
#pragma unroll 1
      for (uint32_t k = k0; k < kend; ++k) {
        const uint32_t e = load_pair<V>(vrow + (size_t)k * (2 * sizeof(V)));
        const uint32_t a = (e & (sizeof(V) == 1 ? 0xFFu : 0xFFFFu)) >> g.shift, b = (e >> (8 * sizeof(V))) >> g.shift;
        if (is_luma) {
          row0[2 * (size_t)k] = (D)a;
          if (2 * k + 1 < g.width) row0[2 * (size_t)k + 1] = (D)b;
        } else { row0[k] = (D)a; row1[k] = (D)b; }
      }
    }
  }
}

// planes -> the two planes of the video buffer; samples clamped to [0, maxv] as pack_kernel does; every byte of [0, row_bytes)
// of every row is written, the padding sample of an odd luma row as zero, and nothing between row_bytes and the pitch
template <typename V, typename D>
__global__ __launch_bounds__(256) void pack_video420_kernel(const D* __restrict__ src, uint8_t* __restrict__ luma, uint8_t* __restrict__ chroma,
                                                            Geo420 g, bool crcb, int32_t maxv)
{
  typedef Piece<V, D> P;
  const uint32_t u = blockIdx.x * 64u + threadIdx.x;
  if (u >= g.pieces) return;
  const uint32_t k0 = u * P::NP;
  const bool fits = (uint64_t)k0 + P::NP <= g.cw;
  const uint32_t kend = fits ? k0 + P::NP : g.cw;
  const uint32_t rows = g.height + g.ch;
  const size_t ysz = (size_t)g.width * g.height, csz = (size_t)g.cw * g.ch;
  const D* const cplane0 = src + ysz + (crcb ? csz : 0);
  const D* const cplane1 = src + ysz + (crcb ? 0 : csz);
  for (uint64_t r = blockIdx.y * 4u + threadIdx.y; r < rows; r += gridDim.y * 4u) {
    const bool is_luma = r < g.height;
    const uint32_t y = (uint32_t)(is_luma ? r : r - g.height);
    uint8_t* vrow = is_luma ? luma + (size_t)y * g.luma_pitch : chroma + (size_t)y * g.chroma_pitch;
    const D* row0 = is_luma ? src + (size_t)y * g.width : cplane0 + (size_t)y * g.cw;
    const D* row1 = cplane1 + (size_t)y * g.cw;
    const uint32_t val = uniform((uint32_t)(uintptr_t)vrow), al0 = uniform((uint32_t)(uintptr_t)row0), al1 = uniform((uint32_t)(uintptr_t)row1);
    if (fits && (!is_luma || 2ull * ((uint64_t)k0 + P::NP) <= g.width)) {
      uint32_t pw[P::VW];
#pragma unroll
      for (int i = 0; i < P::VW; ++i) pw[i] = 0;
      if (is_luma) {
        uint32_t wy[P::YW];
        load_run<P::YW, sizeof(D)>((const uint8_t*)(row0 + 2 * (size_t)k0), wy, al0);
#pragma unroll
        for (int j = 0; j < 2 * P::NP; ++j) put<V>(pw, j, clamp_sample(get<D>(wy, j), maxv) << g.shift);
      } else {
        uint32_t w0[P::CW], w1[P::CW];
        load_run<P::CW, sizeof(D)>((const uint8_t*)(row0 + k0), w0, al0);
        load_run<P::CW, sizeof(D)>((const uint8_t*)(row1 + k0), w1, al1);
#pragma unroll
        for (int k = 0; k < P::NP; ++k) {
          put<V>(pw, 2 * k, clamp_sample(get<D>(w0, k), maxv) << g.shift);
          put<V>(pw, 2 * k + 1, clamp_sample(get<D>(w1, k), maxv) << g.shift);
        }
      }
      store_run<P::VW, 2 * sizeof(V)>(vrow + (size_t)u * (P::VW * 4), pw, val);
    } else {
      // the row's last piece: pair by pair, the loads unconditional from clamped indices; the sample beyond an odd luma row
      // packs as zero
#pragma unroll 1
      for (uint32_t k = k0; k < kend; ++k) {
        int32_t a, b;
        bool has_b = true;
        if (is_luma) {
          const uint32_t xb = 2 * k + 1;
          has_b = xb < g.width;
          a = (int32_t)row0[2 * (size_t)k]; b = (int32_t)row0[has_b ? xb : g.width - 1];
        } else { a = (int32_t)row0[k]; b = (int32_t)row1[k]; }
        store_pair<V>(vrow + (size_t)k * (2 * sizeof(V)), clamp_sample(a, maxv) << g.shift, has_b ? clamp_sample(b, maxv) << g.shift : 0u);
      }
    }
  }
}

enum { NV12 = OJPHGPU_VIDEO_NV12, NV21 = OJPHGPU_VIDEO_NV21, P0XX = OJPHGPU_VIDEO_P0XX };

template <typename V, typename D>
int launch420(hipStream_t st, bool unpack, const void* planes, const void* luma, const void* chroma, const Geo420& g, bool crcb, uint32_t bit_depth)
{
  const uint32_t rows4 = (uint32_t)(((uint64_t)g.height + g.ch + 3) / 4);
  const dim3 grid((g.pieces + 63) / 64, rows4 < 65535u ? rows4 : 65535u), wg(64, 4);
  if (unpack) hipLaunchKernelGGL((unpack_video420_kernel<V, D>), grid, wg, 0, st, (const uint8_t*)luma, (const uint8_t*)chroma, (D*)planes, g, crcb);
  else hipLaunchKernelGGL((pack_video420_kernel<V, D>), grid, wg, 0, st, (const D*)planes, (uint8_t*)luma, (uint8_t*)chroma, g, crcb,
                          (int32_t)((1u << bit_depth) - 1u));
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

int run420(void* stream, bool unpack, int format, const void* d_luma, uint32_t luma_pitch, const void* d_chroma, uint32_t chroma_pitch,
           const void* d_planes, uint32_t width, uint32_t height, uint32_t bit_depth, int container_bits)
{
  Geo420 g{};
  uint32_t row_bytes = 0; uint64_t chroma_offset = 0, frame_bytes = 0;
  const VideoDesc* v = video_desc(format, OJPHGPU_VIDEO_FAMILY_420);
  if (!d_luma || !d_chroma || !d_planes || !video_check(v, width, height, bit_depth, container_bits)) return OJPHGPU_E_INVALID;
  if (!video_layout(v, width, height, &row_bytes, &chroma_offset, &frame_bytes) || luma_pitch < row_bytes || chroma_pitch < row_bytes) return OJPHGPU_E_INVALID;
  // a chroma pair: what every row of both planes must be aligned to
  if ((((uintptr_t)d_luma | (uintptr_t)d_chroma) & (v->r.pointer_align - 1)) || ((luma_pitch | chroma_pitch) & (v->r.pitch_align - 1))) return OJPHGPU_E_INVALID;
  g.width = width; g.height = height; g.cw = (uint32_t)(((uint64_t)width + 1) / 2); g.ch = (uint32_t)(((uint64_t)height + 1) / 2);
  g.shift = format == P0XX ? 16u - bit_depth : 0u;
  g.luma_pitch = luma_pitch; g.chroma_pitch = chroma_pitch;
  const uint32_t np = 8u / (uint32_t)(container_bits / 8);
  g.pieces = (g.cw + np - 1) / np;
  hipStream_t st = (hipStream_t)stream;
  const bool crcb = format == NV21;
  if (format == P0XX)
    return container_bits == 16 ? launch420<uint16_t, uint16_t>(st, unpack, d_planes, d_luma, d_chroma, g, crcb, bit_depth)
                                : launch420<uint16_t, int32_t>(st, unpack, d_planes, d_luma, d_chroma, g, crcb, bit_depth);
  if (container_bits == 8) return launch420<uint8_t, uint8_t>(st, unpack, d_planes, d_luma, d_chroma, g, crcb, bit_depth);
  if (container_bits == 16) return launch420<uint8_t, uint16_t>(st, unpack, d_planes, d_luma, d_chroma, g, crcb, bit_depth);
  return launch420<uint8_t, int32_t>(st, unpack, d_planes, d_luma, d_chroma, g, crcb, bit_depth);
}

}  // namespace

extern "C" int ojphgpu_video420_layout(int format, uint32_t width, uint32_t height, uint32_t* row_bytes, uint64_t* chroma_offset, uint64_t* frame_bytes)
{
  if (!row_bytes || !chroma_offset || !frame_bytes) return OJPHGPU_E_INVALID;
  return video_layout(video_desc(format, OJPHGPU_VIDEO_FAMILY_420), width, height, row_bytes, chroma_offset, frame_bytes) ? OJPHGPU_OK : OJPHGPU_E_INVALID;
}

extern "C" int ojphgpu_unpack_video420(void* stream, int format, const void* d_luma, uint32_t luma_pitch, const void* d_chroma, uint32_t chroma_pitch,
                                        void* d_planes, uint32_t width, uint32_t height, uint32_t bit_depth, int container_bits)
{
  return run420(stream, true, format, d_luma, luma_pitch, d_chroma, chroma_pitch, d_planes, width, height, bit_depth, container_bits);
}

extern "C" int ojphgpu_pack_video420(void* stream, int format, const void* d_planes, void* d_luma, uint32_t luma_pitch, void* d_chroma,
                                      uint32_t chroma_pitch, uint32_t width, uint32_t height, int container_bits, uint32_t bit_depth)
{
  return run420(stream, false, format, d_luma, luma_pitch, d_chroma, chroma_pitch, d_planes, width, height, bit_depth, container_bits);
}
