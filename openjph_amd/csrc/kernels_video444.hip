// openjph_amd/csrc/kernels_video444.hip -- 4:4:4 packed video as capture cards, SDI / ST 2110 receivers, graphics surfaces and
// ffmpeg's rawvideo hold it (v410, Y410, R210, R10k, Y412 / Y416, AYUV, BGRA, RGBA, ARGB; ojphgpu.h section 7d): ONE
// interleaved word per pixel, rows at a pitch <-> the three planar sample containers the codec works on ([H][W] each, 8 / 16 /
// 32 bits per sample).
//
// No counterpart in the reference, whose readers take .ppm / .yuv files sample by sample on the host.  Pure data movement,
// HBM-bound, written the way the finding of DESIGN 1.4 / 1.5 asks: a lane takes a SMALL piece, so that one load or store
// instruction of a wavefront covers contiguous whole 128-byte lines on each of its four streams.
//
// A lane takes 16 bytes of one row of the video side -- four pixels of a dword format, two of Y4XX -- and with them
//   the planes      4, 8 or 16 bytes of each of the three rows (four pixels in 8-, 16-, 32-bit containers), Y4XX: 4 or 8
// each moved by ONE instruction when the row's address allows, next to the neighbour lanes': an instruction of a wavefront
// covers 256 to 1024 contiguous bytes.  A wavefront is 64 such pieces of ONE row (the workgroup is 64 x 4: four rows), so the
// alignment of the row on the video side and in each plane is the same in every lane, and rows of any alignment -- a pitch
// that shifts every row, a plane of odd width -- stay correct through the wave-uniform choice of piece width of
// kernels_video_pieces.h.  The last piece of a row, when the row does not fill it, goes pixel by pixel.
//
// The nine formats are three kernels per direction and container.  A dword format is three fields of FB = 10 or 8 bits at
// `base`, `base + FB`, `base + 2 FB` of a little-endian dword, OR-ed with a constant (the alpha); which plane the low, the
// middle and the high field belong to is three plane pointers, and a big-endian format (R210, R10k) or a byte order that is
// the mirror of another (ARGB of BGRA) is the same behind a byte permutation of the dword whose selector is a kernel
// argument.  Y4XX is two dwords.  No division, no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ojphgpu.h"
#include "kernels_video_pieces.h"
#include "video_formats.h"

namespace {

// how a format sits in its pixel: the fields' first bit (Y4XX: 16 - depth, the shift of a word), the byte selector that turns
// the dword as it lies in memory into the little-endian one the fields are cut from (and back: both selectors used here are
// their own inverse), the constant bits (alpha) and the components the low, middle and high field (Y4XX: word 0, 1, 2) hold
struct Fmt444 { uint32_t base, sel, fill, c_lo, c_mi, c_hi; };
struct Geo444 { uint32_t width, height, pieces, pitch; };

enum : uint32_t { SEL_LE = 0x03020100u, SEL_BE = 0x00010203u };

// FB: bits of a field (10, 8; 16: Y4XX); D: container of the planes
template <int FB, typename D> struct Piece444 {
  static constexpr int DW = FB == 16 ? 2 : 1;                                // dwords of a pixel
  static constexpr int NP = 4 / DW;                                          // pixels of a piece: 16 bytes of the video side
  static constexpr int PW = NP * (int)sizeof(D) / 4;                         // dwords of each plane's row
  static_assert(PW >= 1, "a plane's run is at least a dword");
};

// the pixel at p[0 .. DW) -> the three fields, low, middle, high
template <int FB> __device__ __forceinline__ void split(const uint32_t* p, const Fmt444& f, uint32_t& lo, uint32_t& mi, uint32_t& hi)
{
  if constexpr (FB == 16) {
    lo = (p[0] & 0xFFFFu) >> f.base; mi = (p[0] >> 16) >> f.base; hi = (p[1] & 0xFFFFu) >> f.base;
  } else {
    const uint32_t v = __builtin_amdgcn_perm(0u, p[0], f.sel) >> f.base, m = (1u << FB) - 1u;
    lo = v & m; mi = (v >> FB) & m; hi = (v >> (2 * FB)) & m;
  }
}
// ... and back; the fields are clamped samples
template <int FB> __device__ __forceinline__ void join(uint32_t* p, const Fmt444& f, uint32_t lo, uint32_t mi, uint32_t hi)
{
  if constexpr (FB == 16) {
    p[0] = lo << f.base | (mi << f.base) << 16; p[1] = hi << f.base | f.fill;
  } else {
    p[0] = __builtin_amdgcn_perm(0u, (lo | mi << FB | hi << (2 * FB)) << f.base | f.fill, f.sel);
  }
}

template <int FB, typename D>
__global__ __launch_bounds__(256) void unpack_video444_kernel(const uint8_t* __restrict__ video, D* __restrict__ dst, Geo444 g, Fmt444 f)
{
  typedef Piece444<FB, D> P;
  const uint32_t u = blockIdx.x * 64u + threadIdx.x;
  if (u >= g.pieces) return;
  const uint32_t x0 = u * P::NP;                       // first pixel of the piece
  const bool fits = (uint64_t)x0 + P::NP <= g.width;
  const uint32_t xend = fits ? x0 + P::NP : g.width;
  const size_t psz = (size_t)g.width * g.height;
  D* const plo = dst + f.c_lo * psz; D* const pmi = dst + f.c_mi * psz; D* const phi = dst + f.c_hi * psz;
  for (uint64_t y = blockIdx.y * 4u + threadIdx.y; y < g.height; y += gridDim.y * 4u) {
    const uint8_t* vrow = video + (size_t)y * g.pitch;
    const size_t ro = (size_t)y * g.width;
    D* rlo = plo + ro; D* rmi = pmi + ro; D* rhi = phi + ro;
    const uint32_t val = uniform((uint32_t)(uintptr_t)vrow), al0 = uniform((uint32_t)(uintptr_t)rlo), al1 = uniform((uint32_t)(uintptr_t)rmi),
                   al2 = uniform((uint32_t)(uintptr_t)rhi);
    if (fits) {
      uint32_t pw[4], w0[P::PW], w1[P::PW], w2[P::PW];
      load_run<4, 4 * P::DW>(vrow + (size_t)u * 16, pw, val);
#pragma unroll
      for (int i = 0; i < P::PW; ++i) w0[i] = w1[i] = w2[i] = 0;
#pragma unroll
      for (int j = 0; j < P::NP; ++j) {
        uint32_t lo, mi, hi;
        split<FB>(pw + j * P::DW, f, lo, mi, hi);
        put<D>(w0, j, lo); put<D>(w1, j, mi); put<D>(w2, j, hi);
      }
      store_run<P::PW, sizeof(D)>((uint8_t*)(rlo + x0), w0, al0);
      store_run<P::PW, sizeof(D)>((uint8_t*)(rmi + x0), w1, al1);
      store_run<P::PW, sizeof(D)>((uint8_t*)(rhi + x0), w2, al2);
    } else {                                           // pixel by pixel, what the row holds of the piece
#pragma unroll 1
      for (uint32_t x = x0; x < xend; ++x) {
        const uint32_t* q = (const uint32_t*)(vrow + (size_t)x * (4 * P::DW));
        const uint32_t e[2] = { q[0], q[P::DW - 1] };
        uint32_t lo, mi, hi;
        split<FB>(e, f, lo, mi, hi);
        rlo[x] = (D)lo; rmi[x] = (D)mi; rhi[x] = (D)hi;
      }
    }
  }
}

// planes -> the video buffer; samples clamped to [0, maxv] as pack_kernel does; every byte of [0, row_bytes) of every row is
// written, padding as zero and alpha opaque, and nothing between row_bytes and the pitch
template <int FB, typename D>
__global__ __launch_bounds__(256) void pack_video444_kernel(const D* __restrict__ src, uint8_t* __restrict__ video, Geo444 g, Fmt444 f, int32_t maxv)
{
  typedef Piece444<FB, D> P;
  const uint32_t u = blockIdx.x * 64u + threadIdx.x;
  if (u >= g.pieces) return;
  const uint32_t x0 = u * P::NP;
  const bool fits = (uint64_t)x0 + P::NP <= g.width;
  const uint32_t xend = fits ? x0 + P::NP : g.width;
  const size_t psz = (size_t)g.width * g.height;
  const D* const plo = src + f.c_lo * psz; const D* const pmi = src + f.c_mi * psz; const D* const phi = src + f.c_hi * psz;
  for (uint64_t y = blockIdx.y * 4u + threadIdx.y; y < g.height; y += gridDim.y * 4u) {
    uint8_t* vrow = video + (size_t)y * g.pitch;
    const size_t ro = (size_t)y * g.width;
    const D* rlo = plo + ro; const D* rmi = pmi + ro; const D* rhi = phi + ro;
    const uint32_t val = uniform((uint32_t)(uintptr_t)vrow), al0 = uniform((uint32_t)(uintptr_t)rlo), al1 = uniform((uint32_t)(uintptr_t)rmi),
                   al2 = uniform((uint32_t)(uintptr_t)rhi);
    if (fits) {
      uint32_t pw[4], w0[P::PW], w1[P::PW], w2[P::PW];
      load_run<P::PW, sizeof(D)>((const uint8_t*)(rlo + x0), w0, al0);
      load_run<P::PW, sizeof(D)>((const uint8_t*)(rmi + x0), w1, al1);
      load_run<P::PW, sizeof(D)>((const uint8_t*)(rhi + x0), w2, al2);
#pragma unroll
      for (int j = 0; j < P::NP; ++j)
        join<FB>(pw + j * P::DW, f, clamp_sample(get<D>(w0, j), maxv), clamp_sample(get<D>(w1, j), maxv), clamp_sample(get<D>(w2, j), maxv));
      store_run<4, 4 * P::DW>(vrow + (size_t)u * 16, pw, val);
    } else {
#pragma unroll 1
      for (uint32_t x = x0; x < xend; ++x) {
        uint32_t e[2];
        join<FB>(e, f, clamp_sample((int32_t)rlo[x], maxv), clamp_sample((int32_t)rmi[x], maxv), clamp_sample((int32_t)rhi[x], maxv));
        uint32_t* q = (uint32_t*)(vrow + (size_t)x * (4 * P::DW));
        q[0] = e[0];
        if (P::DW == 2) q[P::DW - 1] = e[P::DW - 1];
      }
    }
  }
}

// format (one of this section: video_formats.h has judged it) -> field bits, how it sits in its pixel
struct Desc444 { int fb; Fmt444 f; };

Desc444 describe444(int format)
{
  switch (format) {                                  //  fb   base  selector fill         low mid high
  case OJPHGPU_VIDEO_V410: return Desc444{ 10, { 2, SEL_LE, 0u, 1, 0, 2 } };            // Cb Y Cr
  case OJPHGPU_VIDEO_Y410: return Desc444{ 10, { 0, SEL_LE, 3u << 30, 1, 0, 2 } };
  case OJPHGPU_VIDEO_R210: return Desc444{ 10, { 0, SEL_BE, 0u, 2, 1, 0 } };            // B G R
  case OJPHGPU_VIDEO_R10K: return Desc444{ 10, { 2, SEL_BE, 0u, 2, 1, 0 } };
  case OJPHGPU_VIDEO_Y4XX: return Desc444{ 16, { 0, SEL_LE, 0u, 1, 0, 2 } };            // words Cb Y Cr; base, fill: by depth
  case OJPHGPU_VIDEO_AYUV: return Desc444{ 8, { 0, SEL_LE, 0xFFu << 24, 2, 1, 0 } };     // bytes Cr Cb Y A
  case OJPHGPU_VIDEO_BGRA: return Desc444{ 8, { 0, SEL_LE, 0xFFu << 24, 2, 1, 0 } };     // bytes B G R A
  case OJPHGPU_VIDEO_RGBA: return Desc444{ 8, { 0, SEL_LE, 0xFFu << 24, 0, 1, 2 } };     // bytes R G B A
  case OJPHGPU_VIDEO_ARGB: return Desc444{ 8, { 0, SEL_BE, 0xFFu << 24, 2, 1, 0 } };     // bytes A R G B: BGRA mirrored
  }
  return Desc444{ 0, { 0, 0, 0, 0, 0, 0 } };
}

template <int FB, typename D>
int launch444(hipStream_t st, bool unpack, const void* planes, const void* video, const Geo444& g, const Fmt444& f, uint32_t bit_depth)
{
  const uint32_t rows4 = (uint32_t)(((uint64_t)g.height + 3) / 4);
  const dim3 grid((g.pieces + 63) / 64, rows4 < 65535u ? rows4 : 65535u), wg(64, 4);
  if (unpack) hipLaunchKernelGGL((unpack_video444_kernel<FB, D>), grid, wg, 0, st, (const uint8_t*)video, (D*)planes, g, f);
  else hipLaunchKernelGGL((pack_video444_kernel<FB, D>), grid, wg, 0, st, (const D*)planes, (uint8_t*)video, g, f, (int32_t)((1u << bit_depth) - 1u));
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

int run444(void* stream, bool unpack, int format, const void* d_video, uint32_t pitch, const void* d_planes, uint32_t width, uint32_t height,
           uint32_t bit_depth, int container_bits)
{
  uint32_t row_bytes = 0; uint64_t chroma_offset = 0, frame_bytes = 0;
  const VideoDesc* v = video_desc(format, OJPHGPU_VIDEO_FAMILY_444);
  if (!d_video || !d_planes || !video_check(v, width, height, bit_depth, container_bits)) return OJPHGPU_E_INVALID;
  if (!video_layout(v, width, height, &row_bytes, &chroma_offset, &frame_bytes) || pitch < row_bytes) return OJPHGPU_E_INVALID;
  if (((uintptr_t)d_video & (v->r.pointer_align - 1)) || (pitch & (v->r.pitch_align - 1))) return OJPHGPU_E_INVALID;
  Desc444 d = describe444(format);
  if (d.fb == 16) { d.f.base = 16u - bit_depth; d.f.fill = (((1u << bit_depth) - 1u) << d.f.base) << 16; }
  Geo444 g{};
  g.width = width; g.height = height; g.pitch = pitch;
  const uint32_t np = 16u / v->unit_bytes;             // pixels of a piece
  g.pieces = (uint32_t)(((uint64_t)width + np - 1) / np);
  hipStream_t st = (hipStream_t)stream;
  if (d.fb == 16)
    return container_bits == 16 ? launch444<16, uint16_t>(st, unpack, d_planes, d_video, g, d.f, bit_depth)
                                : launch444<16, int32_t>(st, unpack, d_planes, d_video, g, d.f, bit_depth);
  if (d.fb == 10)
    return container_bits == 16 ? launch444<10, uint16_t>(st, unpack, d_planes, d_video, g, d.f, bit_depth)
                                : launch444<10, int32_t>(st, unpack, d_planes, d_video, g, d.f, bit_depth);
  if (container_bits == 8) return launch444<8, uint8_t>(st, unpack, d_planes, d_video, g, d.f, bit_depth);
  if (container_bits == 16) return launch444<8, uint16_t>(st, unpack, d_planes, d_video, g, d.f, bit_depth);
  return launch444<8, int32_t>(st, unpack, d_planes, d_video, g, d.f, bit_depth);
}

}  // namespace

extern "C" int ojphgpu_video444_layout(int format, uint32_t width, uint32_t height, uint32_t* row_bytes, uint64_t* frame_bytes)
{
  if (!row_bytes || !frame_bytes) return OJPHGPU_E_INVALID;
  uint64_t chroma_offset = 0;
  return video_layout(video_desc(format, OJPHGPU_VIDEO_FAMILY_444), width, height, row_bytes, &chroma_offset, frame_bytes) ? OJPHGPU_OK : OJPHGPU_E_INVALID;
}

extern "C" int ojphgpu_unpack_video444(void* stream, int format, const void* d_video, uint32_t pitch, void* d_planes, uint32_t width, uint32_t height,
                                        uint32_t bit_depth, int container_bits)
{
  return run444(stream, true, format, d_video, pitch, d_planes, width, height, bit_depth, container_bits);
}

extern "C" int ojphgpu_pack_video444(void* stream, int format, const void* d_planes, void* d_video, uint32_t pitch, uint32_t width, uint32_t height,
                                      int container_bits, uint32_t bit_depth)
{
  return run444(stream, false, format, d_video, pitch, d_planes, width, height, bit_depth, container_bits);
}
