// openjph_amd/csrc/kernels_colour.hip -- RGB <-> YCbCr 4:4:4 / 4:2:2 / 4:2:0 over planar containers (include/ojphgpu.h
// section 7e): the matrix of a video standard, the range mapping, the change of depth and the halving / doubling of chroma
// in one integer pass.
//   ojphgpu_colour_table_make   host only: the 16-bit fixed-point table of a standard, a direction, two depths, two ranges
//   colour_forward_kernel       three w x h planes R, G, B -> Y w x h, Cb and Cr cw x ch: per pixel t_c = m[c] . (R, G, B)
//                      in 64 bits; chroma through the taps (1, 2, 1) of frame_resample_kernel (kernels_fit.hip), centred ON
//                      source sample (fx i, fy j), indices clamped into the plane; one rounding
//   colour_inverse_kernel       the mirror: chroma doubled by the weights (2) / (1, 1), luma scaled alike, the matrix, one
//                      rounding
// Modelled on frame_resample_kernel: an item is a group of luma columns -- what one 16-byte load per plane covers, eight at
// the most (8-bit containers: one 8-byte load) -- walked down a band of rows.  Forward, halved horizontally: one extra sample
// per plane and row, the group's left neighbour, completes the (1, 2, 1) of its first chroma column; inverse: the chroma
// group's right neighbour completes the last odd column.  Halved vertically, the bottom row's horizontal sums are carried as
// the next top row (forward), the lower chroma row of a pair as the next upper one (inverse).  A row that does not stand on
// the load's boundary, or a group over the row's end, goes sample by sample with clamped indices; outputs leave as one 2-
// to 16-byte store (32 bytes: two) where all exist and the address allows, else singly.  Plain vector stores, no LDS, no
// scratch.  Table and frame are kernel arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "ojph_plan.h"

namespace {

constexpr uint32_t WG = 256;
constexpr int K = 16;                                       // fraction bits of a table
constexpr uint32_t ROWS = 8;                                // rows of the vertically smaller side an item walks down

template <typename T> struct Group { static constexpr int N = sizeof(T) == 4 ? 4 : 8; };   // luma columns of an item

template <int BYTES> struct Vec;
template <> struct Vec<2> { typedef uint16_t type; };
template <> struct Vec<4> { typedef uint32_t type; };
template <> struct Vec<8> { typedef uint2 type; };
template <> struct Vec<16> { typedef uint4 type; };

// the samples x0 .. x0 + N - 1 of a row of w: one load where all exist and the address allows, else one by one, the index
// clamped into the row (a sample past the row's end is never stored, but it IS the clamped tap of its neighbour)
template <typename T, int N>
__device__ __forceinline__ void load_group(const T* __restrict__ row, uint64_t x0, uint64_t w, uint32_t e[N])
{
  constexpr int B = N * (int)sizeof(T);
  typedef typename Vec<B>::type V;
  const T* p = row + x0;
  if (x0 + (uint64_t)N <= w && ((uintptr_t)p & (uintptr_t)(B - 1)) == 0) {
    const V v = *reinterpret_cast<const V*>(p);
    T raw[N];
    __builtin_memcpy(raw, &v, B);
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = raw[i];
  } else {
    const uint64_t last = w - 1u;
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = row[min(x0 + (uint64_t)i, last)];
  }
}

// N finished samples to x0 .. of a row of w: as one store (above 16 bytes: 16 at a time), or those that exist one by one
template <typename T, int N>
__device__ __forceinline__ void store_group(T* row, uint64_t x0, uint64_t w, const uint32_t q[N])
{
  constexpr int B = N * (int)sizeof(T), P = B > 16 ? 16 : B;    // bytes of the group, of a piece
  typedef typename Vec<P>::type V;
  T* p = row + x0;
  if (x0 + (uint64_t)N <= w && ((uintptr_t)p & (uintptr_t)(P - 1)) == 0) {
    T o[N];
#pragma unroll
    for (int i = 0; i < N; ++i) o[i] = (T)q[i];
#pragma unroll
    for (int k = 0; k < B / P; ++k) {
      V v;
      __builtin_memcpy(&v, (const char*)o + k * P, P);
      reinterpret_cast<V*>(p)[k] = v;
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) if (x0 + (uint64_t)i < w) p[i] = (T)q[i];
  }
}

// m . (a0, a1, a2) in 64-bit two's complement
__device__ __forceinline__ uint64_t dot3(const int32_t m[3], uint64_t a0, uint64_t a1, uint64_t a2)
{
  return (uint64_t)(int64_t)m[0] * a0 + (uint64_t)(int64_t)m[1] * a1 + (uint64_t)(int64_t)m[2] * a2;
}

// (acc + (off << KK) + half) >> (K + KK), arithmetic, clamped
template <int KK>
__device__ __forceinline__ uint32_t finish(uint64_t acc, int64_t off, int32_t lo, int32_t hi)
{
  int64_t v = (int64_t)(acc + ((uint64_t)off << KK) + ((uint64_t)1 << (K + KK - 1))) >> (K + KK);
  v = v < (int64_t)lo ? (int64_t)lo : v;
  v = v > (int64_t)hi ? (int64_t)hi : v;
  return (uint32_t)v;
}

// ---------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------
template <int G> struct RgbRow { uint32_t e[3][G]; uint32_t left[3]; };   // a group of one row of R, G, B; its left neighbour

template <typename TS, int FX>
__device__ __forceinline__ void fwd_load(const TS* const s[3], uint64_t r, uint64_t x0, uint64_t w, RgbRow<Group<TS>::N>& a)
{
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const TS* row = s[p] + r * w;
    load_group<TS, Group<TS>::N>(row, x0, w, a.e[p]);
    a.left[p] = FX == 2 ? (uint32_t)row[x0 ? x0 - 1u : 0u] : 0u;
  }
}

// a loaded row -> its luma sums y[G] (LUMA) and, per chroma component, the horizontal sums hc[c][G / FX]: FX == 2: t[2 j - 1] +
// 2 t[2 j] + t[2 j + 1] around luma column x0 + 2 j, FX == 1: t itself
template <int G, int FX, bool LUMA>
__device__ __forceinline__ void fwd_sums(const RgbRow<G>& a, const ojphgpu_colour_table& T, uint64_t y[G], uint64_t hc[2][G / FX])
{
  if (LUMA) {
#pragma unroll
    for (int i = 0; i < G; ++i) y[i] = dot3(T.m[0], a.e[0][i], a.e[1][i], a.e[2][i]);
  }
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    uint64_t t[G];
#pragma unroll
    for (int i = 0; i < G; ++i) t[i] = dot3(T.m[c + 1], a.e[0][i], a.e[1][i], a.e[2][i]);
    if constexpr (FX == 1) {
#pragma unroll
      for (int i = 0; i < G; ++i) hc[c][i] = t[i];
    } else {
      uint64_t prev = dot3(T.m[c + 1], a.left[0], a.left[1], a.left[2]);
#pragma unroll
      for (int j = 0; j < G / 2; ++j) {
        hc[c][j] = prev + 2u * t[2 * j] + t[2 * j + 1];
        prev = t[2 * j + 1];
      }
    }
  }
}

template <typename TD, int G>
__device__ __forceinline__ void fwd_store_luma(TD* row, uint64_t x0, uint64_t w, const uint64_t y[G], const ojphgpu_colour_table& T)
{
  uint32_t q[G];
#pragma unroll
  for (int i = 0; i < G; ++i) q[i] = finish<0>(y[i], T.off[0], T.lo[0], T.hi[0]);
  store_group<TD, G>(row, x0, w, q);
}

template <typename TD, int GC, int KK>
__device__ __forceinline__ void fwd_store_chroma(TD* const d[3], uint64_t j, uint64_t xc, uint64_t cw, const uint64_t acc[2][GC], const ojphgpu_colour_table& T)
{
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    uint32_t q[GC];
#pragma unroll
    for (int i = 0; i < GC; ++i) q[i] = finish<KK>(acc[c][i], T.off[c + 1], T.lo[c + 1], T.hi[c + 1]);
    store_group<TD, GC>(d[c + 1] + j * cw, xc, cw, q);
  }
}

template <typename TS, typename TD, int FX, int FY>
__global__ __launch_bounds__(WG) void colour_forward_kernel(const TS* __restrict__ rgb, TD* __restrict__ ycc, const ojphgpu_colour_frame f,
                                                            const ojphgpu_colour_table T)
{
  constexpr int G = Group<TS>::N, GC = G / FX, KK = 2 * ((FX == 2) + (FY == 2));
  const uint64_t w = f.w, h = f.h, cw = FX == 2 ? (w + 1u) / 2u : w, ch = FY == 2 ? (h + 1u) / 2u : h;
  const TS* const s[3] = { rgb + f.rgb_first[0], rgb + f.rgb_first[1], rgb + f.rgb_first[2] };
  TD* const d[3] = { ycc + f.ycc_first[0], ycc + f.ycc_first[1], ycc + f.ycc_first[2] };
  const uint64_t ncg = (w + G - 1u) / G, nrb = (ch + ROWS - 1u) / ROWS, items = ncg * nrb;
  for (uint64_t it = (uint64_t)blockIdx.x * WG + threadIdx.x; it < items; it += (uint64_t)gridDim.x * WG) {
    const uint64_t band = it / ncg, x0 = (it - band * ncg) * G, xc = x0 / FX;
    const uint64_t j0 = band * ROWS, j1 = min(j0 + ROWS, ch);
    if (FY == 1) {
      for (uint64_t j = j0; j < j1; ++j) {
        RgbRow<G> a;
        uint64_t y[G], hc[2][GC];
        fwd_load<TS, FX>(s, j, x0, w, a);
        fwd_sums<G, FX, true>(a, T, y, hc);
        fwd_store_luma<TD, G>(d[0] + j * w, x0, w, y, T);
        fwd_store_chroma<TD, GC, KK>(d, j, xc, cw, hc, T);
      }
    } else {
      uint64_t top[2][GC];                                  // luma row 2 j - 1, clamped; below the first chroma row: the carry
      {
        RgbRow<G> a;
        uint64_t y[G];
        fwd_load<TS, FX>(s, j0 ? 2u * j0 - 1u : 0u, x0, w, a);
        fwd_sums<G, FX, false>(a, T, y, top);
      }
      for (uint64_t j = j0; j < j1; ++j) {
        const uint64_t r = 2u * j, rb = min(r + 1u, h - 1u);  // (r < h: the size rule)
        RgbRow<G> a, b;
        fwd_load<TS, FX>(s, r, x0, w, a);
        fwd_load<TS, FX>(s, rb, x0, w, b);
        uint64_t ya[G], yb[G], mid[2][GC], bot[2][GC], acc[2][GC];
        fwd_sums<G, FX, true>(a, T, ya, mid);
        fwd_sums<G, FX, true>(b, T, yb, bot);
        fwd_store_luma<TD, G>(d[0] + r * w, x0, w, ya, T);
        if (r + 1u < h) fwd_store_luma<TD, G>(d[0] + (r + 1u) * w, x0, w, yb, T);
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
          for (int i = 0; i < GC; ++i) { acc[c][i] = top[c][i] + 2u * mid[c][i] + bot[c][i]; top[c][i] = bot[c][i]; }
        fwd_store_chroma<TD, GC, KK>(d, j, xc, cw, acc, T);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// inverse
// ---------------------------------------------------------------------------------------------
// one row of a chroma plane under the luma columns x0 .. x0 + G - 1, weight FX: FX == 2: 2 C[x / 2] (x even), C[(x - 1) / 2] +
// C[min((x + 1) / 2, cw - 1)] (x odd); FX == 1: the samples
template <typename TS, int FX>
__device__ __forceinline__ void inv_chroma_row(const TS* __restrict__ row, uint64_t xc, uint64_t cw, uint64_t hx[Group<TS>::N])
{
  constexpr int G = Group<TS>::N, GC = G / FX;
  uint32_t e[GC];
  load_group<TS, GC>(row, xc, cw, e);
  if constexpr (FX == 1) {
#pragma unroll
    for (int i = 0; i < G; ++i) hx[i] = e[i];
  } else {
    const uint32_t right = row[min(xc + (uint64_t)GC, cw - 1u)];
#pragma unroll
    for (int j = 0; j < G / 2; ++j) {
      const uint32_t c0 = e[j], c1 = j + 1 < GC ? e[(j + 1) % GC] : right;
      hx[2 * j] = 2u * (uint64_t)c0;
      hx[2 * j + 1] = (uint64_t)c0 + (uint64_t)c1;
    }
  }
}

// a luma row and the chroma under it (weights included) -> R, G, B
template <typename TD, int G, int KK>
__device__ __forceinline__ void inv_store(TD* const d[3], uint64_t r, uint64_t x0, uint64_t w, const uint32_t y[G], const uint64_t cb[G],
                                          const uint64_t cr[G], const ojphgpu_colour_table& T)
{
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    uint32_t q[G];
#pragma unroll
    for (int i = 0; i < G; ++i) q[i] = finish<KK>(dot3(T.m[c], (uint64_t)y[i] << KK, cb[i], cr[i]), T.off[c], T.lo[c], T.hi[c]);
    store_group<TD, G>(d[c] + r * w, x0, w, q);
  }
}

template <typename TS, typename TD, int FX, int FY>
__global__ __launch_bounds__(WG) void colour_inverse_kernel(const TS* __restrict__ ycc, TD* __restrict__ rgb, const ojphgpu_colour_frame f,
                                                            const ojphgpu_colour_table T)
{
  constexpr int G = Group<TS>::N, KK = (FX == 2) + (FY == 2);
  const uint64_t w = f.w, h = f.h, cw = FX == 2 ? (w + 1u) / 2u : w, ch = FY == 2 ? (h + 1u) / 2u : h;
  const TS* const s[3] = { ycc + f.ycc_first[0], ycc + f.ycc_first[1], ycc + f.ycc_first[2] };
  TD* const d[3] = { rgb + f.rgb_first[0], rgb + f.rgb_first[1], rgb + f.rgb_first[2] };
  const uint64_t ncg = (w + G - 1u) / G, nrb = (ch + ROWS - 1u) / ROWS, items = ncg * nrb;
  for (uint64_t it = (uint64_t)blockIdx.x * WG + threadIdx.x; it < items; it += (uint64_t)gridDim.x * WG) {
    const uint64_t band = it / ncg, x0 = (it - band * ncg) * G, xc = x0 / FX;
    const uint64_t j0 = band * ROWS, j1 = min(j0 + ROWS, ch);
    if (FY == 1) {
      for (uint64_t j = j0; j < j1; ++j) {
        uint32_t y[G];
        uint64_t cb[G], cr[G];
        load_group<TS, G>(s[0] + j * w, x0, w, y);
        inv_chroma_row<TS, FX>(s[1] + j * cw, xc, cw, cb);
        inv_chroma_row<TS, FX>(s[2] + j * cw, xc, cw, cr);
        inv_store<TD, G, KK>(d, j, x0, w, y, cb, cr, T);
      }
    } else {
      uint64_t cb0[G], cr0[G];                              // chroma row j; below the first: the carry
      inv_chroma_row<TS, FX>(s[1] + j0 * cw, xc, cw, cb0);
      inv_chroma_row<TS, FX>(s[2] + j0 * cw, xc, cw, cr0);
      for (uint64_t j = j0; j < j1; ++j) {
        const uint64_t r = 2u * j, jn = min(j + 1u, ch - 1u);
        uint32_t ya[G], yb[G];
        uint64_t cb1[G], cr1[G], cbe[G], cre[G], cbo[G], cro[G];
        load_group<TS, G>(s[0] + r * w, x0, w, ya);
        load_group<TS, G>(s[0] + min(r + 1u, h - 1u) * w, x0, w, yb);
        inv_chroma_row<TS, FX>(s[1] + jn * cw, xc, cw, cb1);
        inv_chroma_row<TS, FX>(s[2] + jn * cw, xc, cw, cr1);
#pragma unroll
        for (int i = 0; i < G; ++i) {
          cbe[i] = 2u * cb0[i]; cre[i] = 2u * cr0[i];
          cbo[i] = cb0[i] + cb1[i]; cro[i] = cr0[i] + cr1[i];
          cb0[i] = cb1[i]; cr0[i] = cr1[i];
        }
        inv_store<TD, G, KK>(d, r, x0, w, ya, cbe, cre, T);
        if (r + 1u < h) inv_store<TD, G, KK>(d, r + 1u, x0, w, yb, cbo, cro, T);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------------------
template <bool FORWARD, typename TS, typename TD, int FX, int FY>
void launch(hipStream_t stream, uint32_t grid, const void* src, void* dst, const ojphgpu_colour_frame& f, const ojphgpu_colour_table& T)
{
  if constexpr (FORWARD) hipLaunchKernelGGL((colour_forward_kernel<TS, TD, FX, FY>), dim3(grid), dim3(WG), 0, stream, (const TS*)src, (TD*)dst, f, T);
  else hipLaunchKernelGGL((colour_inverse_kernel<TS, TD, FX, FY>), dim3(grid), dim3(WG), 0, stream, (const TS*)src, (TD*)dst, f, T);
}

template <bool FORWARD, typename TS, typename TD>
void launch_factors(hipStream_t stream, uint32_t grid, const void* src, void* dst, const ojphgpu_colour_frame& f, const ojphgpu_colour_table& T)
{
  if (f.fx == 1 && f.fy == 1) launch<FORWARD, TS, TD, 1, 1>(stream, grid, src, dst, f, T);
  else if (f.fy == 1) launch<FORWARD, TS, TD, 2, 1>(stream, grid, src, dst, f, T);
  else if (f.fx == 1) launch<FORWARD, TS, TD, 1, 2>(stream, grid, src, dst, f, T);
  else launch<FORWARD, TS, TD, 2, 2>(stream, grid, src, dst, f, T);
}

template <bool FORWARD, typename TS>
void launch_dst(hipStream_t stream, uint32_t grid, const void* src, void* dst, int dst_bits, const ojphgpu_colour_frame& f, const ojphgpu_colour_table& T)
{
  if (dst_bits == 8) launch_factors<FORWARD, TS, uint8_t>(stream, grid, src, dst, f, T);
  else if (dst_bits == 16) launch_factors<FORWARD, TS, uint16_t>(stream, grid, src, dst, f, T);
  else launch_factors<FORWARD, TS, uint32_t>(stream, grid, src, dst, f, T);
}

bool container_ok(int bits) { return bits == 8 || bits == 16 || bits == 32; }

// the judgement of both stages, and the launch: src / dst with their containers; which of the frame's plane sets is the source
template <bool FORWARD>
int colour_stage(void* stream, const void* d_src, int src_bits, void* d_dst, int dst_bits, const ojphgpu_colour_frame* frame,
                 const ojphgpu_colour_table* table)
{
  if (!d_src || !d_dst || !frame || !table || !container_ok(src_bits) || !container_ok(dst_bits)) return OJPHGPU_E_INVALID;
  const ojphgpu_colour_frame f = *frame;
  ojphgpu_colour_table T = *table;
  if (f.w == 0 || f.h == 0 || (f.fx != 1 && f.fx != 2) || (f.fy != 1 && f.fy != 2) || T.k != (uint32_t)K) return OJPHGPU_E_INVALID;
  const uint64_t sb = (uint64_t)src_bits / 8u, db = (uint64_t)dst_bits / 8u;
  if (((uintptr_t)d_src & (uintptr_t)(sb - 1u)) != 0 || ((uintptr_t)d_dst & (uintptr_t)(db - 1u)) != 0) return OJPHGPU_E_INVALID;
  // [lo, hi] inside the destination's container
  const int64_t top = dst_bits == 32 ? (int64_t)INT32_MAX : ((int64_t)1 << dst_bits) - 1;
  for (int c = 0; c < 3; ++c) {
    T.lo[c] = std::max(T.lo[c], 0); T.hi[c] = (int32_t)std::min((int64_t)T.hi[c], top);
    if (T.lo[c] > T.hi[c]) return OJPHGPU_E_INVALID;
  }
  // no source plane over a destination plane (byte ranges)
  const uint64_t luma = (uint64_t)f.w * f.h, chroma = (uint64_t)((f.w + f.fx - 1u) / f.fx) * (uint64_t)((f.h + f.fy - 1u) / f.fy);
  const uint64_t* const sf = FORWARD ? f.rgb_first : f.ycc_first; const uint64_t* const df = FORWARD ? f.ycc_first : f.rgb_first;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const uint64_t sn = FORWARD || i == 0 ? luma : chroma, dn = !FORWARD || j == 0 ? luma : chroma;
      const uintptr_t s0 = (uintptr_t)d_src + sf[i] * sb, s1 = s0 + sn * sb, d0 = (uintptr_t)d_dst + df[j] * db, d1 = d0 + dn * db;
      if (s0 < d1 && d0 < s1) return OJPHGPU_E_INVALID;
    }
  const char* e = getenv("OJPHGPU_COLOUR_WGS");
  const long v = e ? atol(e) : 0;
  const uint64_t cap = v > 0 && v <= 65535 ? (uint64_t)v : 2048u;   // eight workgroups per compute unit stride over the items
  const uint64_t g = src_bits == 32 ? 4u : 8u, rows = ((uint64_t)f.h + f.fy - 1u) / f.fy;
  const uint64_t items = (((uint64_t)f.w + g - 1u) / g) * ((rows + ROWS - 1u) / ROWS);
  const uint32_t grid = (uint32_t)std::min(cap, (items + WG - 1u) / WG);
  if (src_bits == 8) launch_dst<FORWARD, uint8_t>((hipStream_t)stream, grid, d_src, d_dst, dst_bits, f, T);
  else if (src_bits == 16) launch_dst<FORWARD, uint16_t>((hipStream_t)stream, grid, d_src, d_dst, dst_bits, f, T);
  else launch_dst<FORWARD, uint32_t>((hipStream_t)stream, grid, d_src, d_dst, dst_bits, f, T);
  return hipGetLastError() == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

}  // namespace

extern "C" int ojphgpu_colour_table_make(int standard, int direction, uint32_t rgb_depth, uint32_t ycc_depth, int rgb_range, int ycc_range,
                                         ojphgpu_colour_table* out)
{
  if (!out || rgb_depth < 8 || rgb_depth > 16 || ycc_depth < 8 || ycc_depth > 16) return OJPHGPU_E_INVALID;
  if ((direction != OJPHGPU_COLOUR_FORWARD && direction != OJPHGPU_COLOUR_INVERSE) || (rgb_range != OJPHGPU_COLOUR_FULL && rgb_range != OJPHGPU_COLOUR_NARROW) ||
      (ycc_range != OJPHGPU_COLOUR_FULL && ycc_range != OJPHGPU_COLOUR_NARROW)) return OJPHGPU_E_INVALID;
  double Kr, Kb;
  switch (standard) {
  case OJPHGPU_COLOUR_BT601: Kr = 0.299; Kb = 0.114; break;
  case OJPHGPU_COLOUR_BT709: Kr = 0.2126; Kb = 0.0722; break;
  case OJPHGPU_COLOUR_BT2020: Kr = 0.2627; Kb = 0.0593; break;
  default: return OJPHGPU_E_INVALID;
  }
  const double Kg = 1.0 - Kr - Kb;
  // offset and span of a signal: RGB or luma, chroma (the numpy statement, pipeline.colour_table, writes every double
  // expression below in the same order)
  const int64_t sr = (int64_t)1 << (rgb_depth - 8), sy = (int64_t)1 << (ycc_depth - 8);
  const int64_t full_r = ((int64_t)1 << rgb_depth) - 1, full_y = ((int64_t)1 << ycc_depth) - 1;
  const int64_t off_rgb = rgb_range == OJPHGPU_COLOUR_FULL ? 0 : 16 * sr, span_rgb_i = rgb_range == OJPHGPU_COLOUR_FULL ? full_r : 219 * sr;
  const int64_t off_ycc[3] = { ycc_range == OJPHGPU_COLOUR_FULL ? 0 : 16 * sy, 128 * sy, 128 * sy };
  const int64_t span_y = ycc_range == OJPHGPU_COLOUR_FULL ? full_y : 219 * sy, span_c = ycc_range == OJPHGPU_COLOUR_FULL ? full_y : 224 * sy;
  const double span_rgb = (double)span_rgb_i, span_ycc[3] = { (double)span_y, (double)span_c, (double)span_c };
  int64_t m[3][3];
  ojphgpu_colour_table T{};
  T.k = (uint32_t)K;
  if (direction == OJPHGPU_COLOUR_FORWARD) {
    const double A[3][3] = { { Kr, Kg, Kb },
                             { -Kr / (2.0 * (1.0 - Kb)), -Kg / (2.0 * (1.0 - Kb)), (1.0 - Kb) / (2.0 * (1.0 - Kb)) },
                             { (1.0 - Kr) / (2.0 * (1.0 - Kr)), -Kg / (2.0 * (1.0 - Kr)), -Kb / (2.0 * (1.0 - Kr)) } };
    for (int c = 0; c < 3; ++c) {
      m[c][0] = (int64_t)llround(A[c][0] * span_ycc[c] / span_rgb * 65536.0);
      m[c][2] = (int64_t)llround(A[c][2] * span_ycc[c] / span_rgb * 65536.0);
      const int64_t total = c == 0 ? (int64_t)llround(span_ycc[0] / span_rgb * 65536.0) : 0;
      m[c][1] = total - m[c][0] - m[c][2];
      T.off[c] = off_ycc[c] * 65536 - off_rgb * (m[c][0] + m[c][1] + m[c][2]);
      T.lo[c] = 0; T.hi[c] = (int32_t)full_y;
    }
  } else {
    const double Ci[3][3] = { { 1.0, 0.0, 2.0 * (1.0 - Kr) },
                              { 1.0, -(2.0 * Kb * (1.0 - Kb) / Kg), -(2.0 * Kr * (1.0 - Kr) / Kg) },
                              { 1.0, 2.0 * (1.0 - Kb), 0.0 } };
    for (int c = 0; c < 3; ++c) {
      int64_t sum = 0;
      for (int i = 0; i < 3; ++i) {
        m[c][i] = Ci[c][i] == 0.0 ? 0 : (int64_t)llround(Ci[c][i] * span_rgb / span_ycc[i] * 65536.0);
        sum += m[c][i] * off_ycc[i];
      }
      T.off[c] = off_rgb * 65536 - sum;
      T.lo[c] = 0; T.hi[c] = (int32_t)full_r;
    }
  }
  for (int c = 0; c < 3; ++c)
    for (int i = 0; i < 3; ++i) {
      if (m[c][i] < -(int64_t)INT32_MAX || m[c][i] > (int64_t)INT32_MAX) return OJPHGPU_E_INVALID;   // (never: the depths are 8 .. 16)
      T.m[c][i] = (int32_t)m[c][i];
    }
  *out = T;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_frame_rgb_to_ycc(void* stream, const void* d_rgb, int rgb_container_bits, void* d_ycc, int ycc_container_bits,
                                        const ojphgpu_colour_frame* frame, const ojphgpu_colour_table* table)
{
  return colour_stage<true>(stream, d_rgb, rgb_container_bits, d_ycc, ycc_container_bits, frame, table);
}

extern "C" int ojphgpu_frame_ycc_to_rgb(void* stream, const void* d_ycc, int ycc_container_bits, void* d_rgb, int rgb_container_bits,
                                        const ojphgpu_colour_frame* frame, const ojphgpu_colour_table* table)
{
  return colour_stage<false>(stream, d_ycc, ycc_container_bits, d_rgb, rgb_container_bits, frame, table);
}
