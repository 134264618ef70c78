// openjph_amd/csrc/ojphgpu_pipe.cpp -- frame pipelines: what ojph::codestream's exchange() ... flush() /
// read_headers() ... pull() contract (ojph_codestream_local.cpp:1148-1270, :912-1146) becomes when the hot
// path runs on a GPU behind PCIe and frames follow each other (video, image sequences, a tiled image cut
// into independent codestreams).
//
// One frame alone is bound by the PCIe copies either side of 0.6 ms of kernels; a SEQUENCE is not, if the
// stages of consecutive frames overlap.  A pipe keeps `depth` frames in flight, each in a slot of its own:
//
//   encoder   caller fills slot n+1's pinned frame  |  H2D of n+1  |  kernels of n  |  D2H of n-1's block
//             lengths -> packet headers on host threads -> placement kernel -> D2H of n-1's finished codestream
//   decoder   host threads parse n+1's packet headers  |  H2D of n+1's bytes + descriptors  |  kernels of n  |
//             D2H of n-1's frame into pinned memory the caller reads rows from
//   a view    (ojphgpu_dec_pipe_create_view: reduced resolution, a window) the same, with the plan of every frame restricted
//             as the first one's was and the H2D of the bytes done by a kernel that reads the runs of the view's blocks out
//             of the pinned codestream (kernels_assemble.hip, gather_runs_kernel): only those bytes cross PCIe
//   transcoder  host threads parse n+1's packet headers  |  H2D of n+1's bytes + descriptors  |  block decoder, verdicts and
//             block coder (or the trials of a budget's search) of n  |  packet headers of n-1 on host threads -> placement
//             kernel -> D2H of n-1's finished codestream (the end of this file)
//
// on separate HIP streams (copy-in, compute, copy-out) with events between them.  The coded bytes never
// pass through a host memcpy: the encoder's codestream is assembled in HBM (kernels_assemble.hip) from the
// layout the host Tier-2 computes out of the block LENGTHS, and arrives in pinned memory ready to be
// written to a file; the decoder uploads the codestream as it is and addresses the blocks inside it.
//
// An encoder pipe with a byte budget (ojphgpu_enc_pipe_set_budget) searches the quantisation step of every frame: the
// compute stream then carries, per frame, transform + statistics and the trials of the search, issued by one ordered
// worker thread -- the pipe has one encoder and one arena, so frame n+1's transform must not be enqueued before frame n's
// last trial -- while uploads, Tier-2 of the chosen step and copy-outs of the neighbouring frames go on as above.  A quality
// target (ojphgpu_enc_pipe_set_quality) rides on the same worker: transform, the trials of its search -- requantise, the
// decoder's synthesis and the error sums against the slot's own copy of the frame, no block coded -- then the blocks of j*,
// once.
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <new>
#include <thread>

#include "ojphgpu_objects.h"
#include "ojph_pool.h"
#include "video_formats.h"

namespace ojphgpu {
int assemble_launch(void* stream, const T2Job* d_jobs, uint32_t njobs, const uint8_t* d_blob, const uint8_t* d_data, uint8_t* d_out);
int copy_to_host_launch(void* stream, void* d_dst, const void* src, size_t bytes);
int publish_words_launch(void* stream, uint32_t* d_dst, const uint32_t* src, uint32_t n);
int gather_runs_launch(void* stream, const void* d_src, size_t src_cap, const void* d_runs, uint32_t nruns, void* d_dst, uint64_t staged_len);
}

namespace {

// Pinned host memory, mapped into the device's address space and coherent: uploads from it go through
// hipMemcpyAsync (SDMA); what comes BACK is written into it by kernels (`d` = its device address), see
// kernels_assemble.hip for why.
struct Pinned {
  uint8_t* p = nullptr; uint8_t* d = nullptr; size_t cap = 0;
  int reserve(size_t bytes) {
    if (bytes <= cap) return 0;
    release();
    void* q = nullptr; void* dq = nullptr;
    if (hipHostMalloc(&q, bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { (void)hipGetLastError(); return -1; }
    if (hipHostGetDevicePointer(&dq, q, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(q); return -1; }
    p = (uint8_t*)q; d = (uint8_t*)dq; cap = bytes;
    return 0;
  }
  void release() { if (p) (void)hipHostFree(p); p = nullptr; d = nullptr; cap = 0; }
};

struct Grow {                       // device buffer that grows (never shrinks)
  DeviceBuf b; size_t cap = 0;
  int reserve(size_t bytes) {
    if (bytes <= cap) return 0;
    b.release();
    if (b.alloc(bytes + 64)) { cap = 0; return -1; }
    cap = bytes;
    return 0;
  }
};

enum SlotState { FREE = 0, ACQUIRED, SUBMITTED, DONE, HELD };

// Which engine moves which direction (the two directions of one pipe must not share the SDMA engine, see
// kernels_assemble.hip): 0 = upload by hipMemcpyAsync (SDMA), download by a copy kernel; 1 = upload by a copy
// kernel reading the pinned memory, download by hipMemcpyAsync; 2 = both by hipMemcpyAsync (the runtime decides).
// The stream of the device -> host copies: those are kernels (see kernels_assemble.hip) and must get their few
// workgroups onto the chip while the block coder of the next frames keeps every CU full -- highest priority.
hipError_t create_copy_out_stream(hipStream_t* s)
{
  int lo = 0, hi = 0;
  (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
  if (getenv("OJPHGPU_COPY_PRIO_OFF")) return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  return hipStreamCreateWithPriority(s, hipStreamNonBlocking, hi);
}

int copy_mode(const char* name, int dflt)
{
  const char* e = getenv(name);
  const int v = e ? atoi(e) : dflt;
  return v >= 0 && v <= 2 ? v : dflt;
}

int upload(int mode, hipStream_t st, void* d_dst, const Pinned& src, size_t src_off, size_t bytes);
int download(int mode, hipStream_t st, const Pinned& dst, const void* d_src, size_t bytes);

int upload(int mode, hipStream_t st, void* d_dst, const Pinned& src, size_t src_off, size_t bytes)
{
  if (bytes == 0) return OJPHGPU_OK;
  if (mode == 1 && ((src_off | (uintptr_t)d_dst) & 15u) == 0) return copy_to_host_launch(st, d_dst, src.d + src_off, bytes);   // the kernel copies either way
  return hipMemcpyAsync(d_dst, src.p + src_off, bytes, hipMemcpyHostToDevice, st) == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

int download(int mode, hipStream_t st, const Pinned& dst, const void* d_src, size_t bytes)
{
  if (bytes == 0) return OJPHGPU_OK;
  if (mode == 0) return copy_to_host_launch(st, dst.d, d_src, bytes);
  return hipMemcpyAsync(dst.p, d_src, bytes, hipMemcpyDeviceToHost, st) == hipSuccess ? OJPHGPU_OK : OJPHGPU_E_HIP;
}

double now_ms()
{
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// The worker loops: the next slot of a queue, or false once `stop` is up and the queue is empty.
bool pop_work(std::mutex& mu, std::condition_variable& cv, std::deque<uint32_t>& q, const bool& stop, uint32_t& si)
{
  std::unique_lock<std::mutex> lk(mu);
  cv.wait(lk, [&] { return stop || !q.empty(); });
  if (q.empty()) return false;
  si = q.front(); q.pop_front();
  return true;
}

// ---- the hand-over: how a frame crosses PCIe -- the encoder's going in, the decoder's coming out.  PLANES: as the codec
// holds it, straight into / out of the slot's image.  The other kinds go through the slot's staging buffer (`pixels`) and a
// launch on the compute stream: PIXELS pixel-interleaved (_set_pixels), PACKED one bit string (_set_packed), VIDEO one video
// buffer in its format's tight layout (_set_video, ojphgpu.h sections 7b - 7d; the formats' rules: the one table of
// video_formats.h).  A pipe has one; everything the launch needs is fixed when it is set.
enum HandoverKind { PLANES = 0, PIXELS, PACKED, VIDEO };

struct Handover {
  int kind = PLANES;
  int bits = 0, big_endian = 0;                      // PIXELS: 8 / 16 per sample; PACKED: 10 / 12 / 14
  int format = 0;                                    // VIDEO: OJPHGPU_VIDEO_*
  uint32_t row_bytes = 0; uint64_t chroma_offset = 0; // VIDEO: the tight layout inside the staging buffer (video_layout)
  uint32_t w = 0, h = 0, depth = 0;                  // PIXELS, VIDEO: the (luma) plane; the depth a decoder clamps to
  size_t bytes = 0;                                  // of a frame as handed over: what _acquire / _collect report and PCIe carries
  // VIDEO with a colour spec (_set_video_colour, ojphgpu.h section 7e): the buffer holds R, G, B, the plan Y, Cb, Cr.  depth:
  // the RGB side's; table: forward for an encoder pipe, inverse for a decoder pipe; frame: where the six planes stand -- R, G,
  // B w x h one after the other in the slot's `rgb` buffer, the plan's in its image
  bool colour = false;
  ojphgpu_colour_spec spec{};
  ojphgpu_colour_table table{};
  ojphgpu_colour_frame frame{};
  size_t rgb_bytes = 0;                              // of the slot's `rgb` buffer: 3 w h containers (chroma: the format's planes)
  // VIDEO through _set_video_chroma (section 7f): the buffer holds Y, Cb, Cr in the FORMAT's chroma cell, the plan in its own.
  // chroma: the setter's mode (0: another setter's); stage: the cells differ, so two launches -- the format's planes stand one
  // after the other in the slot's `rgb` buffer, cframe says where (source: the buffer's side for an encoder pipe, the plan's
  // for a decoder pipe).  Equal cells: the plain VIDEO hand-over
  int chroma = 0; bool stage = false;
  ojphgpu_chroma_frame cframe{};
};

enum { ODD_X0 = 1, ODD_Y0 = 2 };                    // a decoder pipe's window begins on an odd column / row

// The plan judgement of the two _set_video_colour setters (every refusal that needs no device): `want` (format, spec) -> the
// rest of it.
int handover_fit_colour(const Plan& P, int container, bool decoding, int odd_origin, Handover& want)
{
  const VideoDesc* v = video_desc(want.format, OJPHGPU_VIDEO_FAMILY_444); uint64_t bytes = 0;
  if (!v || P.comps.size() != 3) return OJPHGPU_E_INVALID;
  // the RGB members of the family; the others hold Y, Cb, Cr already
  if (want.format != OJPHGPU_VIDEO_BGRA && want.format != OJPHGPU_VIDEO_RGBA && want.format != OJPHGPU_VIDEO_ARGB &&
      want.format != OJPHGPU_VIDEO_R210 && want.format != OJPHGPU_VIDEO_R10K) return OJPHGPU_E_INVALID;
  const CompGeo& Y = P.comps[0]; const CompGeo& Cb = P.comps[1]; const CompGeo& Cr = P.comps[2];
  // three unsigned components of one depth of 8 .. 16 bits, the chroma planes (fx, fy) smaller, each factor 1 or 2
  for (const CompGeo& g : P.comps) if (g.is_signed || g.bit_depth != Y.bit_depth) return OJPHGPU_E_INVALID;
  if (Y.bit_depth < 8 || Y.bit_depth > 16 || Y.bit_depth > (uint32_t)container || Y.w == 0 || Y.h == 0) return OJPHGPU_E_INVALID;
  if (Y.dx != 1 || Y.dy != 1 || Cb.dx != Cr.dx || Cb.dy != Cr.dy || (Cb.dx != 1 && Cb.dx != 2) || (Cb.dy != 1 && Cb.dy != 2)) return OJPHGPU_E_INVALID;
  const uint32_t fx = Cb.dx, fy = Cb.dy;
  const uint32_t cw = (uint32_t)(((uint64_t)Y.w + fx - 1) / fx), ch = (uint32_t)(((uint64_t)Y.h + fy - 1) / fy);
  if (Cb.w != cw || Cb.h != ch || Cr.w != cw || Cr.h != ch) return OJPHGPU_E_INVALID;
  // a chroma sample stands ON the first luma sample of its cell (phase 0): no odd image offset, no window from an odd column
  // or row, in a halved direction
  if ((fx == 2 && ((P.p.image_x0 & 1u) || (odd_origin & ODD_X0))) || (fy == 2 && ((P.p.image_y0 & 1u) || (odd_origin & ODD_Y0)))) return OJPHGPU_E_INVALID;
  if (P.has_region && P.skip_recon) {                 // a window at a reduced resolution: its origin is even on THAT grid
    if (P.skip_recon > 30) return OJPHGPU_E_INVALID;
    const uint32_t cell = 2u << P.skip_recon;
    if ((fx == 2 && P.region[0] % cell) || (fy == 2 && P.region[1] % cell)) return OJPHGPU_E_INVALID;
  }
  // a decoder's 32-bit planes are int32 and may hold negative samples, which the stage's unsigned containers cannot say
  if (decoding && container == 32) return OJPHGPU_E_INVALID;
  const uint32_t rgb_depth = want.spec.rgb_depth ? want.spec.rgb_depth : Y.bit_depth;
  if (!video_check(v, Y.w, Y.h, rgb_depth, container) || !video_layout(v, Y.w, Y.h, &want.row_bytes, &want.chroma_offset, &bytes)) return OJPHGPU_E_INVALID;
  const int rc = ojphgpu_colour_table_make(want.spec.standard, decoding ? OJPHGPU_COLOUR_INVERSE : OJPHGPU_COLOUR_FORWARD, rgb_depth, Y.bit_depth,
                                           want.spec.rgb_range, want.spec.ycc_range, &want.table);
  if (rc) return rc;
  const uint64_t wh = (uint64_t)Y.w * Y.h;
  want.w = Y.w; want.h = Y.h; want.depth = rgb_depth;
  want.frame = ojphgpu_colour_frame{ Y.w, Y.h, fx, fy, { 0, wh, 2 * wh }, { Y.frame_off, Cb.frame_off, Cr.frame_off } };
  want.rgb_bytes = (size_t)(3 * wh) * (size_t)(container / 8);
  want.bytes = (size_t)bytes;
  return OJPHGPU_OK;
}

int handover_fit(const Plan& P, int container, bool decoding, int odd_origin, Handover& want);

// The plan judgement of the two _set_video_chroma setters (every refusal that needs no device): `want` (format, chroma) -> the
// rest of it.  A format of the plan's own cell is judged as the plain VIDEO hand-over, behind the origin rule of this one.
int handover_fit_chroma(const Plan& P, int container, bool decoding, int odd_origin, Handover& want)
{
  const VideoDesc* v = video_desc(want.format); uint64_t bytes = 0;
  if (!v || P.comps.size() != 3 || want.chroma != OJPHGPU_CHROMA_COSITED) return OJPHGPU_E_INVALID;
  // the RGB members of the 4:4:4 family hold R, G, B: _set_video_colour is their way
  if (want.format == OJPHGPU_VIDEO_BGRA || want.format == OJPHGPU_VIDEO_RGBA || want.format == OJPHGPU_VIDEO_ARGB ||
      want.format == OJPHGPU_VIDEO_R210 || want.format == OJPHGPU_VIDEO_R10K) return OJPHGPU_E_INVALID;
  const CompGeo& Y = P.comps[0]; const CompGeo& Cb = P.comps[1]; const CompGeo& Cr = P.comps[2];
  for (const CompGeo& g : P.comps) if (g.is_signed || g.bit_depth != Y.bit_depth) return OJPHGPU_E_INVALID;
  if (Y.w == 0 || Y.h == 0) return OJPHGPU_E_INVALID;
  if (Y.dx != 1 || Y.dy != 1 || Cb.dx != Cr.dx || Cb.dy != Cr.dy || (Cb.dx != 1 && Cb.dx != 2) || (Cb.dy != 1 && Cb.dy != 2)) return OJPHGPU_E_INVALID;
  const uint32_t pfx = Cb.dx, pfy = Cb.dy, ffx = v->r.sub_x, ffy = v->r.sub_y;   // the plan's cell, the format's
  const uint32_t cw = (uint32_t)(((uint64_t)Y.w + pfx - 1) / pfx), ch = (uint32_t)(((uint64_t)Y.h + pfy - 1) / pfy);
  const uint64_t wh = (uint64_t)Y.w * Y.h;
  if (Cb.w != cw || Cb.h != ch || Cr.w != cw || Cr.h != ch) return OJPHGPU_E_INVALID;
  if (Y.frame_off != 0 || Cb.frame_off != wh || Cr.frame_off != wh + (uint64_t)cw * ch) return OJPHGPU_E_INVALID;   // the tight frame layout
  // a chroma sample stands ON the first luma sample of its cell (phase 0) on BOTH sides: no odd image offset, no window from
  // an odd column or row, in a direction where either cell is 2
  const bool cx = pfx == 2 || ffx == 2, cy = pfy == 2 || ffy == 2;
  if ((cx && ((P.p.image_x0 & 1u) || (odd_origin & ODD_X0))) || (cy && ((P.p.image_y0 & 1u) || (odd_origin & ODD_Y0)))) return OJPHGPU_E_INVALID;
  if (P.has_region && P.skip_recon) {                 // a window at a reduced resolution: its origin is even on THAT grid
    if (P.skip_recon > 30) return OJPHGPU_E_INVALID;
    const uint32_t cell = 2u << P.skip_recon;
    if ((cx && P.region[0] % cell) || (cy && P.region[1] % cell)) return OJPHGPU_E_INVALID;
  }
  if (pfx == ffx && pfy == ffy) {                     // the plain hand-over: one launch, no intermediate buffer
    Handover plain = want;
    plain.chroma = 0;
    const int rc = handover_fit(P, container, decoding, odd_origin, plain);
    if (rc) return rc;
    plain.chroma = want.chroma; plain.stage = false;
    plain.cframe = ojphgpu_chroma_frame{ Y.w, Y.h, pfx, pfy, pfx, pfy, { 0, wh, wh + (uint64_t)cw * ch }, { 0, wh, wh + (uint64_t)cw * ch } };
    want = plain;
    return OJPHGPU_OK;
  }
  if (!video_check(v, Y.w, Y.h, Y.bit_depth, container) || !video_layout(v, Y.w, Y.h, &want.row_bytes, &want.chroma_offset, &bytes)) return OJPHGPU_E_INVALID;
  const uint64_t fc = (((uint64_t)Y.w + ffx - 1) / ffx) * (((uint64_t)Y.h + ffy - 1) / ffy);   // samples of a chroma plane of the format
  want.w = Y.w; want.h = Y.h; want.depth = Y.bit_depth;
  want.stage = true;
  if (decoding) want.cframe = ojphgpu_chroma_frame{ Y.w, Y.h, pfx, pfy, ffx, ffy, { Y.frame_off, Cb.frame_off, Cr.frame_off }, { 0, wh, wh + fc } };
  else want.cframe = ojphgpu_chroma_frame{ Y.w, Y.h, ffx, ffy, pfx, pfy, { 0, wh, wh + fc }, { Y.frame_off, Cb.frame_off, Cr.frame_off } };
  want.rgb_bytes = (size_t)(wh + 2 * fc) * (size_t)(container / 8);
  want.bytes = (size_t)bytes;
  return OJPHGPU_OK;
}

// Every refusal of the three setters, and the size of the frame: `want` (kind, bits, big_endian, format) -> the rest of it.
// decoding: the frame comes back, clamped to one range; odd_origin: the pipe decodes a window whose first column (ODD_X0) or
// first row (ODD_Y0) is odd.
int handover_fit(const Plan& P, int container, bool decoding, int odd_origin, Handover& want)
{
  if (want.kind == VIDEO && want.colour) return handover_fit_colour(P, container, decoding, odd_origin, want);
  if (want.kind == VIDEO && want.chroma) return handover_fit_chroma(P, container, decoding, odd_origin, want);
  const CompGeo& Y = P.comps[0];
  want.w = Y.w; want.h = Y.h; want.depth = 0;
  for (const CompGeo& g : P.comps) want.depth = std::max(want.depth, g.bit_depth);
  switch (want.kind) {
  case PLANES:
    want.bytes = (size_t)P.frame_elems * (size_t)(container / 8);
    return OJPHGPU_OK;
  case PIXELS:                                        // one size for all components (so every plane is w x h), unsigned, depths that fit
    if ((want.bits != 8 && want.bits != 16) || want.bits > container) return OJPHGPU_E_INVALID;
    if (P.skip_recon || P.has_region) {               // a view's frame (a decoder pipe): planes of one size
      for (const CompGeo& g : P.comps) if (g.w != Y.w || g.h != Y.h || g.w == 0 || g.h == 0) return OJPHGPU_E_INVALID;
    } else if (P.frame_elems != (uint64_t)P.p.width * P.p.height * P.p.num_comps) return OJPHGPU_E_INVALID;   // sub-sampled components
    for (const CompGeo& g : P.comps) {
      if (g.is_signed || g.bit_depth > (uint32_t)want.bits) return OJPHGPU_E_INVALID;
      if (decoding && g.bit_depth != Y.bit_depth) return OJPHGPU_E_INVALID;   // one clamp range per frame
    }
    want.bytes = (size_t)P.frame_elems * (size_t)(want.bits / 8);
    return OJPHGPU_OK;
  case PACKED:
    if ((want.bits != 10 && want.bits != 12 && want.bits != 14) || (container != 16 && container != 32)) return OJPHGPU_E_INVALID;
    for (const CompGeo& g : P.comps) if (g.is_signed || g.bit_depth > (uint32_t)want.bits) return OJPHGPU_E_INVALID;
    want.bytes = (size_t)((P.frame_elems + 31) / 32) * 4u * (size_t)want.bits;
    return OJPHGPU_OK;
  case VIDEO: {
    // three unsigned components of one depth, the chroma planes the format's cell smaller than the luma plane (rounded up),
    // tightly packed -> the format's tight layout of that frame.  A window's first column and row must open a chroma cell
    const VideoDesc* v = video_desc(want.format); uint64_t bytes = 0;
    if (!v || P.comps.size() != 3) return OJPHGPU_E_INVALID;
    const uint32_t cw = (uint32_t)(((uint64_t)Y.w + v->r.sub_x - 1) / v->r.sub_x), ch = (uint32_t)(((uint64_t)Y.h + v->r.sub_y - 1) / v->r.sub_y);
    for (const CompGeo& g : P.comps) if (g.is_signed || g.bit_depth != Y.bit_depth) return OJPHGPU_E_INVALID;
    for (size_t c = 1; c < 3; ++c) if (P.comps[c].w != cw || P.comps[c].h != ch) return OJPHGPU_E_INVALID;
    if (P.comps[1].frame_off != (uint64_t)Y.w * Y.h || P.comps[2].frame_off != (uint64_t)Y.w * Y.h + (uint64_t)cw * ch) return OJPHGPU_E_INVALID;
    if (!video_check(v, Y.w, Y.h, Y.bit_depth, container) || !video_layout(v, Y.w, Y.h, &want.row_bytes, &want.chroma_offset, &bytes)) return OJPHGPU_E_INVALID;
    if (((odd_origin & ODD_X0) && v->r.sub_x == 2) || ((odd_origin & ODD_Y0) && v->r.sub_y == 2)) return OJPHGPU_E_INVALID;
    want.bytes = (size_t)bytes;
    return OJPHGPU_OK;
  }
  }
  return OJPHGPU_E_INVALID;
}

// a video buffer in its tight layout <-> tightly packed planes of the format's cell (4:2:0 and 4:4:4: rows, of both planes, at row_bytes)
int video_launch(hipStream_t stream, const Handover& h, int container, bool unpack, void* d_staged, void* d_planes)
{
  uint8_t* const luma = (uint8_t*)d_staged;
  switch (video_desc(h.format)->r.family) {
  case OJPHGPU_VIDEO_FAMILY_444:
    return unpack ? ojphgpu_unpack_video444(stream, h.format, d_staged, h.row_bytes, d_planes, h.w, h.h, h.depth, container)
                  : ojphgpu_pack_video444(stream, h.format, d_planes, d_staged, h.row_bytes, h.w, h.h, container, h.depth);
  case OJPHGPU_VIDEO_FAMILY_420:
    return unpack ? ojphgpu_unpack_video420(stream, h.format, luma, h.row_bytes, luma + h.chroma_offset, h.row_bytes, d_planes, h.w, h.h, h.depth, container)
                  : ojphgpu_pack_video420(stream, h.format, d_planes, luma, h.row_bytes, luma + h.chroma_offset, h.row_bytes, h.w, h.h, container, h.depth);
  }
  return unpack ? ojphgpu_unpack_video(stream, h.format, d_staged, d_planes, h.w, h.h, h.depth, container)
                : ojphgpu_pack_video(stream, h.format, d_planes, d_staged, h.w, h.h, container, h.depth);
}

// The launch of a hand-over on `stream`: staged frame -> planes (unpack: the encoder) or planes -> staged frame, clamped
// (the decoder).  Nothing for PLANES.
int handover_launch(hipStream_t stream, const Handover& h, const Plan& P, int container, bool unpack, void* d_staged, void* d_planes, void* d_rgb)
{
  if (h.kind == VIDEO && h.colour) {                  // two launches: the buffer <-> R, G, B planes <-> the plan's Y, Cb, Cr
    int rc;
    if (unpack) {
      if ((rc = ojphgpu_unpack_video444(stream, h.format, d_staged, h.row_bytes, d_rgb, h.w, h.h, h.depth, container)) != 0) return rc;
      return ojphgpu_frame_rgb_to_ycc(stream, d_rgb, container, d_planes, container, &h.frame, &h.table);
    }
    if ((rc = ojphgpu_frame_ycc_to_rgb(stream, d_planes, container, d_rgb, container, &h.frame, &h.table)) != 0) return rc;
    return ojphgpu_pack_video444(stream, h.format, d_rgb, d_staged, h.row_bytes, h.w, h.h, container, h.depth);
  }
  if (h.kind == VIDEO && h.stage) {                   // two launches: the buffer <-> planes of the format's cell <-> the plan's planes
    int rc;
    if (unpack) {
      if ((rc = video_launch(stream, h, container, true, d_staged, d_rgb)) != 0) return rc;
      return ojphgpu_frame_rechroma(stream, d_rgb, d_planes, container, &h.cframe);
    }
    if ((rc = ojphgpu_frame_rechroma(stream, d_planes, d_rgb, container, &h.cframe)) != 0) return rc;
    return video_launch(stream, h, container, false, d_staged, d_rgb);
  }
  switch (h.kind) {
  case PIXELS:                                        // the file's / capture buffer's / display buffer's pixel order
    return unpack ? ojphgpu_unpack_pixels(stream, d_staged, d_planes, h.w, h.h, P.p.num_comps, h.bits, h.big_endian, container)
                  : ojphgpu_pack_pixels(stream, d_planes, d_staged, h.w, h.h, P.p.num_comps, container, h.bits, h.big_endian, h.depth);
  case PACKED:
    return unpack ? ojphgpu_unpack_bits(stream, d_staged, d_planes, P.frame_elems, h.bits, container)
                  : ojphgpu_pack_bits(stream, d_planes, d_staged, P.frame_elems, container, h.bits);
  case VIDEO:
    return video_launch(stream, h, container, unpack, d_staged, d_planes);
  }
  return OJPHGPU_OK;
}

// the device buffer of a slot that the PCIe copy of the frame touches
template <class Slot> void* handover_device_side(const Handover& h, Slot& s) { return h.kind == PLANES ? s.image.p : s.pixels.b.p; }

// The three setters of a pipe, after their own precondition.  `kind`: the setter's, arg: its bits / format (0: planes
// again); frame: the slot's pinned frame.  Refused while another kind is on, and by handover_fit; then every slot's pinned
// frame and staging buffer hold the new size -- both only grow, so the call may be repeated -- and the pipe takes the
// hand-over.  A refusal changes nothing.
template <class Pipe, class Slot>
int handover_set(Pipe* p, Pinned Slot::*frame, bool decoding, int odd_origin, int kind, int arg, int big_endian, const ojphgpu_colour_spec* spec = nullptr,
                 int chroma = 0)
{
  // (_set_video, _set_video_colour and _set_video_chroma -- chroma != 0 -- exclude each other too)
  if (p->ho.kind != PLANES && (p->ho.kind != kind || p->ho.colour != (spec != nullptr) || (p->ho.chroma != 0) != (chroma != 0))) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    Handover h;
    h.kind = arg ? kind : PLANES; h.big_endian = big_endian ? 1 : 0;
    (kind == VIDEO ? h.format : h.bits) = arg;
    if (spec && arg) { h.colour = true; h.spec = *spec; }
    if (chroma && arg) h.chroma = chroma;
    const int rc = handover_fit(*p->P, p->container, decoding, odd_origin, h);
    if (rc) return rc;
    if (h.kind != PLANES) {
      HIPCHK(hipSetDevice(p->device));
      for (Slot& s : p->slots) if ((s.*frame).reserve(h.bytes + 64) || s.pixels.reserve(h.bytes) || s.rgb.reserve(h.rgb_bytes)) return OJPHGPU_E_NOMEM;
    }
    p->ho = h;
    return OJPHGPU_OK;
  });
}

}  // namespace

// =============================================================================================
// encoder pipe
// =============================================================================================
// What the block coder writes for one frame: the compacted bytes, the cursors, and the per-block records + the two
// published status words in pinned memory.  A slot owns one; a pipe with a byte budget keeps one more (the spare), and the
// trials of a frame's search alternate between the slot's and the spare so that the best fitting trial is never overwritten.
struct EncOut {
  Pinned h_res;
  DeviceBuf out, counters;
  void release() { h_res.release(); out.release(); counters.release(); }
  // where a coding of nb blocks into this set lands: the records, then the two published words; `done`: recorded behind a trial
  RateTrialOut trial(size_t nb, hipEvent_t done) const {
    const size_t words = nb * sizeof(ojphgpu_cb_result);
    return RateTrialOut{ out.p, (ojphgpu_cb_result*)h_res.d, (uint32_t*)counters.p, (const ojphgpu_cb_result*)h_res.p,
                         (uint32_t*)(h_res.d + words), (const uint32_t*)(h_res.p + words), done };
  }
};

// What the search of a frame found (a pipe with a byte budget: rate; with a quality target: quality, the first index it
// tried and the figures of every component at j*).  A slot holds its frame's; the pipe, the frame's collected last.
struct EncSearchResult {
  ojphgpu_rate_info rate{}; bool have_rate = false;
  ojphgpu_quality_info quality{}; uint32_t first_guess = 0; bool have_quality = false;
  ojphgpu_capped_info capped{}; bool have_capped = false;   // a target under a byte cap: this instead of `quality`
  std::vector<ojphgpu_frame_err> comps;
};

struct EncSlot {
  SlotState state = FREE;
  Pinned h_in, h_lay, h_cs;
  EncOut o;
  DeviceBuf image;
  Grow cs, pixels;                                  // pixels: the frame as it was handed over, unless that is as planes
  Grow rgb;                                         // a hand-over of two launches (a colour spec: R, G, B; a chroma stage: the format's planes): what stands between them
  hipEvent_t ev_in = nullptr, ev_kern = nullptr, ev_done = nullptr;
  int rc = 0; size_t cs_len = 0;
  double t_submit = 0, t_done = 0, t_t2 = 0;
  // a pipe that searches: the frame's byte budget or quality target, what its search found, and the plan at the step it
  // chose (the finisher lays the codestream out from it while the worker re-quantises for the next frame)
  uint64_t budget = 0, target = 0, cap = 0;         // (cap: the byte cap of a frame with a target; 0 = none)
  ojphgpu_plan* rplan = nullptr;
  EncSearchResult found;
};

struct ojphgpu_enc_pipe {
  const ojphgpu_plan* handle = nullptr; const Plan* P = nullptr;
  int device = 0, container = 16;
  int mode = copy_mode("OJPHGPU_ENC_COPY_MODE", 0);
  uint32_t depth = 0;
  ojphgpu_encoder* enc = nullptr;
  hipStream_t s_h2d = nullptr, s_comp = nullptr, s_d2h = nullptr;
  std::vector<EncSlot> slots;
  size_t frame_bytes = 0, res_bytes = 0;
  Handover ho;                                      // how frames are handed over; ho.bytes: what _acquire hands out
  uint64_t n_acq = 0, n_sub = 0, n_col = 0;
  std::mutex mu; std::condition_variable cv_work, cv_done;
  std::deque<uint32_t> work; bool stop = false;
  std::vector<std::thread> finishers;
  double sum_t2 = 0, sum_latency = 0; uint64_t n_done = 0;
  // byte budget (ojphgpu_enc_pipe_set_budget): on from before the first _acquire, or never
  bool budget_on = false;
  bool dead = false;                                // switching a search on failed half way (enc_search_on): nothing more runs on this pipe
  uint64_t max_bytes = 0;                           // the budget the next _submit gives its frame
  EncOut spare;
  Pinned h_hist;                                    // the band statistics of the frame being searched (the worker's)
  hipEvent_t ev_trial = nullptr;
  int hint = -1;                                    // j* of the last frame that was certified
  EncSearchResult last;                             // of the frame collected last
  // quality target (ojphgpu_enc_pipe_set_quality): the same rules, never together with a budget
  bool quality_on = false;
  uint64_t max_sse = 0;                             // the target the next _submit gives its frame
  Pinned h_qdescs, h_qerr;                          // a trial's requantise descriptors going out, its error words coming back
  std::vector<std::vector<ojphgpu_frame_err>> q_by_index;   // the figures of every index the search of the worker's frame tried
  // a target under a byte cap (ojphgpu_enc_pipe_set_quality_capped): a quality pipe that has the spare set and the pinned
  // histograms from the start.  `hint` is then the last certified frame's q, hint_b the last BY_BUDGET frame's j*
  bool capped = false;
  uint64_t cap_bytes = 0;                           // the cap the next _submit gives its frame
  int hint_b = -1;
  // the ordered worker of a pipe that searches, whichever search it is: it owns the compute stream
  bool searching() const { return budget_on || quality_on; }
  std::deque<uint32_t> search_work; bool stop_search = false;
  std::condition_variable cv_search;
  std::thread search_worker;
};

// What a finisher does for a frame whose blocks are coded (its kernels have finished): the encoder pipe's frames and the
// transcode pipe's alike.  P: the plan the blocks were quantised with; o: the output set they were coded into; the slot's
// layout staging, codestream in HBM and pinned output, and the event behind its download.
struct CodedFrame {
  const Plan& P; const std::vector<uint32_t>& block_ids; const EncOut& o;
  Pinned& h_lay; Grow& cs; Pinned& h_cs; hipEvent_t ev_done;
};
static int finish_coded_frame(const CodedFrame& f, hipStream_t s_d2h, int mode, size_t& cs_len, double& t_t2)
{
  const double t0 = now_ms();
  const RateTrialOut coded = f.o.trial(f.block_ids.size(), nullptr);
  const ojphgpu_cb_result* res = coded.h_results;
  if (coded.h_publish[1]) return OJPHGPU_E_OVERFLOW;
  return no_throw([&]() -> int {
    std::vector<ojphgpu_coded_block> cb;
    ojphgpu_coded_blocks(f.P, f.block_ids, res, cb);
    T2Layout L;
    int r2 = t2_layout_codestream(f.P, cb.data(), L);
    if (r2) return r2;
    t_t2 = now_ms() - t0;
    // the layout goes into the slot's pinned staging -- jobs, then the blob (64-byte aligned) -- where the
    // placement kernel reads it in place; the codestream is laid out in HBM and written to the slot's pinned
    // output by a copy kernel
    const size_t jbytes = L.jobs.size() * sizeof(T2Job), boff = (jbytes + 63) & ~(size_t)63;
    const size_t lbytes = boff + L.blob.size() + 16;
    if (f.h_lay.reserve(lbytes + lbytes / 4)) return OJPHGPU_E_NOMEM;
    if (f.cs.reserve((size_t)L.total + (size_t)L.total / 8 + 64) || f.h_cs.reserve((size_t)L.total + (size_t)L.total / 8 + 64)) return OJPHGPU_E_NOMEM;
    memcpy(f.h_lay.p, L.jobs.data(), jbytes);
    memcpy(f.h_lay.p + boff, L.blob.data(), L.blob.size());
    r2 = assemble_launch(s_d2h, (const T2Job*)f.h_lay.d, (uint32_t)L.jobs.size(), f.h_lay.d + boff,
                         (const uint8_t*)f.o.out.p, (uint8_t*)f.cs.b.p);
    if (r2) return r2;
    r2 = download(mode, s_d2h, f.h_cs, f.cs.b.p, (size_t)L.total);
    if (r2) return r2;
    HIPCHK(hipEventRecord(f.ev_done, s_d2h));
    HIPCHK(hipEventSynchronize(f.ev_done));
    cs_len = (size_t)L.total;
    return OJPHGPU_OK;
  });
}

static void enc_finish_frame(ojphgpu_enc_pipe* p, EncSlot& s)
{
  const Plan& P = p->searching() ? s.rplan->plan : *p->P;    // (a budget, a target: the plan at the step the frame's search chose)
  auto fail = [&](int rc) { s.rc = rc; };
  if (hipSetDevice(p->device) != hipSuccess) return fail(OJPHGPU_E_HIP);
  if (hipEventSynchronize(s.ev_kern) != hipSuccess) return fail(OJPHGPU_E_HIP);
  const int rc = finish_coded_frame(CodedFrame{ P, p->enc->block_ids, s.o, s.h_lay, s.cs, s.h_cs, s.ev_done }, p->s_d2h, p->mode, s.cs_len, s.t_t2);
  if (rc) {
    // uploads, kernels or the copy-out of this slot may already be enqueued: nothing of the slot may be rewritten or
    // re-reserved (hipHostFree / hipFree in reserve()) by the next _acquire while they are in flight
    hipStreamSynchronize(p->s_h2d); hipStreamSynchronize(p->s_comp); hipStreamSynchronize(p->s_d2h);
    fail(rc);
  }
}

// The kernels of every frame start the same way, on the compute stream behind the frame's upload: the frame as it was handed
// over -> planes in the slot's image, then the encoder's run into the slot's output set (a plain pipe: the whole encode;
// a budget: transform + statistics; a target: conversion + DWT).  The block coder writes its per-block {offset, length}
// records straight into the set's pinned memory (8 bytes per block, posted PCIe writes): all the host needs to code the
// packet headers.
static int enc_begin_frame(ojphgpu_enc_pipe* p, EncSlot& s)
{
  ojphgpu_encoder* e = p->enc;
  HIPCHK(hipStreamWaitEvent(p->s_comp, s.ev_in, 0));
  const int rc = handover_launch(p->s_comp, p->ho, *p->P, p->container, true, s.pixels.b.p, s.image.p, s.rgb.b.p);
  if (rc) return rc;
  e->o_out = s.o.out.p; e->o_results = s.o.h_res.d; e->o_counters = s.o.counters.p;
  return ojphgpu_encoder_run_container(e, s.image.p, p->container);
}

// the frame of a slot is over, whatever its outcome (s.rc): collectable, and counted
static void retire(ojphgpu_enc_pipe* p, EncSlot& s)
{
  {
    std::lock_guard<std::mutex> lk(p->mu);
    s.t_done = now_ms();
    s.state = DONE;
    p->sum_t2 += s.t_t2; p->sum_latency += s.t_done - s.t_submit; p->n_done++;
  }
  p->cv_done.notify_all();
}

// ---- byte budget: the ordered worker.  Per frame, on the compute stream: unpack, transform and statistics; the histograms
// come back; the search, started from the last certified frame's answer, codes its trials into the slot's output set and
// the spare in turn.  Afterwards the slot holds the set with j*, its plan copy stands at qstep(j*), and the finishers take
// over as for any frame.
// (the encoder pipe's frames, and the transcode pipe's: `e` is then the encoder half of its transcoder)
struct RateFrame {
  ojphgpu_encoder* e; Plan* Q;                       // Q: the slot's plan copy, left at qstep(j*)
  uint64_t budget;
  EncOut* slot; EncOut* spare;                       // the slot's output set and the pipe's spare
  hipEvent_t ev_trial;
};
struct EncTrialCtx {
  const RateFrame* f;
  EncOut* best; EncOut* next;                        // best: holds the finest trial that fit so far (null: none); next: written next
  int at;                                            // grid index f->Q stands at
};

static int64_t enc_pipe_trial(void* user, uint32_t j)
{
  EncTrialCtx& c = *(EncTrialCtx*)user;
  const RateFrame& f = *c.f;
  c.at = -1;
  const int64_t size = ojphgpu_encoder_rate_trial(f.e, *f.Q, c.next->trial(f.e->block_ids.size(), f.ev_trial), j);
  if (size < 0) return size;
  c.at = (int)j;
  if ((uint64_t)size <= f.budget) {                  // the finest that fits so far (the search never goes back below one): keep it
    EncOut* other = c.best ? c.best : (c.next == f.slot ? f.spare : f.slot);
    c.best = c.next; c.next = other;
  }
  return size;
}

// The search of one frame, its histograms on the host: started from `hint` (moved to j* when the frame is certified), the
// trials alternating between the two sets; *have: info holds something (OJPHGPU_OK, or OJPHGPU_E_BUDGET: passes, first_guess)
static int rate_search_frame(const RateFrame& f, const uint32_t* h_hist, int& hint, ojphgpu_rate_info& info, bool& have)
{
  EncTrialCtx c{ &f, nullptr, f.slot, -1 };
  const int rc = rate_search(f.e->rate->table, h_hist, f.budget, hint, enc_pipe_trial, &c, &info);
  have = rc == OJPHGPU_OK || rc == OJPHGPU_E_BUDGET;
  if (rc) return rc;
  hint = (int)info.grid_index;
  if (c.best != f.slot) std::swap(*f.slot, *f.spare);   // (pointers only) the slot keeps the set with j*, the other is the spare
  if (c.at != (int)info.grid_index && !rate_apply_step(*f.Q, info.qstep)) return OJPHGPU_E_INVALID;
  return OJPHGPU_OK;
}

static int enc_rate_frame(ojphgpu_enc_pipe* p, EncSlot& s)
{
  ojphgpu_encoder* e = p->enc;
  EncoderRate& R = *e->rate;
  HIPCHK(hipSetDevice(p->device));
  int rc = enc_begin_frame(p, s);                    // transform + statistics (the encoder has a budget)
  if (rc) return rc;
  if ((rc = copy_to_host_launch(p->s_comp, p->h_hist.d, R.hist.p, R.h_hist.size() * 4)) != 0) return rc;
  HIPCHK(hipEventRecord(p->ev_trial, p->s_comp));
  HIPCHK(hipEventSynchronize(p->ev_trial));
  const RateFrame f{ e, &s.rplan->plan, s.budget, &s.o, &p->spare, p->ev_trial };
  if ((rc = rate_search_frame(f, (const uint32_t*)p->h_hist.p, p->hint, s.found.rate, s.found.have_rate)) != 0) return rc;
  HIPCHK(hipEventRecord(s.ev_kern, p->s_comp));
  return OJPHGPU_OK;
}

// ---- quality target: the same worker.  Per frame, on the compute stream: unpack and transform; the search, started from
// the last certified frame's answer, measures SSE(j) against the slot's image -- the planes in the pipe's container, which
// the slot owns until _collect -- with the descriptors and the error words in pinned memory; then j* is block-coded, once,
// into the slot's output set, as a trial of the budget is.
struct EncQualityCtx { ojphgpu_enc_pipe* p; EncSlot* s; };

static int64_t enc_pipe_quality_trial(void* user, uint32_t j, uint64_t* sse)
{
  EncQualityCtx& c = *(EncQualityCtx*)user;
  ojphgpu_enc_pipe* p = c.p;
  std::vector<ojphgpu_frame_err>& got = p->q_by_index[j];
  got.assign(p->P->comps.size(), ojphgpu_frame_err{ 0, 0, 0 });
  const QualityTrialIo io{ c.s->image.p, p->container, (ojphgpu_requant_desc*)p->h_qdescs.p, p->h_qdescs.d,
                           (const ojphgpu_frame_err*)p->h_qerr.p, p->h_qerr.d, p->ev_trial };
  const int rc = ojphgpu_encoder_quality_trial(p->enc, io, j, got.data());
  if (rc) return rc;
  uint64_t total = 0;
  for (const ojphgpu_frame_err& e : got) total += e.sse;
  *sse = total;
  return 0;
}

static int enc_quality_frame(ojphgpu_enc_pipe* p, EncSlot& s)
{
  ojphgpu_encoder* e = p->enc;
  EncSearchResult& f = s.found;
  HIPCHK(hipSetDevice(p->device));
  int rc = enc_begin_frame(p, s);                    // conversion + DWT (e->quality_on)
  if (rc) return rc;
  EncQualityCtx c{ p, &s };
  rc = ojphgpu_quality_search_hint(s.target, p->hint, enc_pipe_quality_trial, &c, &f.quality, &f.first_guess);
  f.have_quality = rc == OJPHGPU_OK || rc == OJPHGPU_E_QUALITY;
  if (rc) return rc;
  f.comps = p->q_by_index[f.quality.grid_index];
  for (const ojphgpu_frame_err& k : f.comps) f.quality.pae = std::max(f.quality.pae, k.pae);
  p->hint = (int)f.quality.grid_index;
  const int64_t size = ojphgpu_encoder_rate_trial(e, s.rplan->plan, s.o.trial(e->block_ids.size(), p->ev_trial), f.quality.grid_index);   // (leaves rplan at qstep(j*))
  if (size < 0) { f.have_quality = false; return size < INT32_MIN ? OJPHGPU_E_INVALID : (int)size; }
  f.quality.bytes = (uint64_t)size;
  HIPCHK(hipEventRecord(s.ev_kern, p->s_comp));
  return OJPHGPU_OK;
}

// ---- a target under a byte cap: the same worker, both kinds of trial.  Per frame, on the compute stream: unpack and
// transform; ojphgpu_capped_search through the two trial callbacks above -- quality trials started from the last certified
// frame's q, size trials alternating between the slot's output set and the spare, started from the last bound frame's j* --
// and the band statistics only when the cap binds, while the unquantised planes are still in the arena.  Afterwards the
// slot holds the set with j* and its plan copy stands at qstep(j*), as after a budget's search.
struct EncCappedCtx { EncQualityCtx q; EncTrialCtx t; int hist_rc; };

static int64_t enc_capped_sse(void* user, uint32_t j, uint64_t* sse) { return enc_pipe_quality_trial(&((EncCappedCtx*)user)->q, j, sse); }
static int64_t enc_capped_size(void* user, uint32_t j) { return enc_pipe_trial(&((EncCappedCtx*)user)->t, j); }

static const uint32_t* enc_capped_hist(void* user)
{
  EncCappedCtx& c = *(EncCappedCtx*)user;
  ojphgpu_enc_pipe* p = c.q.p;
  ojphgpu_encoder* e = p->enc;
  EncoderRate& R = *e->rate;
  c.hist_rc = no_throw([&]() -> int {
    HIPCHK(hipMemsetAsync(R.hist.p, 0, R.hist.n, p->s_comp));
    int rc = ojphgpu_band_stats(p->s_comp, (const ojphgpu_stats_desc*)R.stats_descs.p, R.n_stats, R.stats_max_w, R.stats_max_h, e->arena.p, (uint32_t*)R.hist.p);
    if (rc || (rc = copy_to_host_launch(p->s_comp, p->h_hist.d, R.hist.p, R.h_hist.size() * 4)) != 0) return rc;
    HIPCHK(hipEventRecord(p->ev_trial, p->s_comp));
    HIPCHK(hipEventSynchronize(p->ev_trial));
    return OJPHGPU_OK;
  });
  return c.hist_rc ? nullptr : (const uint32_t*)p->h_hist.p;   // (a failure: halving, and the frame ends with it below)
}

static int enc_capped_frame(ojphgpu_enc_pipe* p, EncSlot& s)
{
  ojphgpu_encoder* e = p->enc;
  EncSearchResult& f = s.found;
  HIPCHK(hipSetDevice(p->device));
  int rc = enc_begin_frame(p, s);                    // conversion + DWT (e->quality_on)
  if (rc) return rc;
  const RateFrame rf{ e, &s.rplan->plan, s.cap, &s.o, &p->spare, p->ev_trial };
  EncCappedCtx c{ EncQualityCtx{ p, &s }, EncTrialCtx{ &rf, nullptr, rf.slot, -1 }, OJPHGPU_OK };
  for (std::vector<ojphgpu_frame_err>& v : p->q_by_index) v.clear();
  rc = capped_search(e->rate->table, s.target, s.cap, p->hint, p->hint_b, enc_capped_sse, enc_capped_size, enc_capped_hist, &c, &f.capped);
  f.have_capped = rc == OJPHGPU_OK || rc == OJPHGPU_E_BUDGET;
  if (c.hist_rc) { f.have_capped = false; return c.hist_rc; }
  if (rc) return rc;
  const ojphgpu_capped_info& I = f.capped;
  if (c.t.best != rf.slot) std::swap(*rf.slot, *rf.spare);   // (pointers only) the slot keeps the set with j*, the other is the spare
  if (c.t.at != (int)I.grid_index && !rate_apply_step(*rf.Q, I.qstep)) { f.have_capped = false; return OJPHGPU_E_INVALID; }
  f.comps = p->q_by_index[I.grid_index];
  if (f.comps.size() != p->P->comps.size()) { f.have_capped = false; return OJPHGPU_E_INVALID; }
  for (const ojphgpu_frame_err& k : f.comps) f.capped.pae = std::max(f.capped.pae, k.pae);
  if (I.quality_index < OJPHGPU_RATE_GRID) p->hint = (int)I.quality_index;
  if (I.outcome == OJPHGPU_CAPPED_BY_BUDGET) p->hint_b = (int)I.grid_index;
  HIPCHK(hipEventRecord(s.ev_kern, p->s_comp));
  return OJPHGPU_OK;
}

static void enc_search_worker(ojphgpu_enc_pipe* p)
{
  for (uint32_t si; pop_work(p->mu, p->cv_search, p->search_work, p->stop_search, si);) {
    EncSlot& s = p->slots[si];
    const int rc = no_throw([&] { return p->capped ? enc_capped_frame(p, s) : p->quality_on ? enc_quality_frame(p, s) : enc_rate_frame(p, s); });
    if (rc) {                                        // the frame ends here (OJPHGPU_E_BUDGET / _E_QUALITY among the reasons); see enc_finish_frame
      hipStreamSynchronize(p->s_h2d); hipStreamSynchronize(p->s_comp);
      s.rc = rc;
      retire(p, s);
      continue;
    }
    { std::lock_guard<std::mutex> lk(p->mu); p->work.push_back(si); }
    p->cv_work.notify_one();
  }
}

static void enc_finisher(ojphgpu_enc_pipe* p)
{
  for (uint32_t si; pop_work(p->mu, p->cv_work, p->work, p->stop, si);) {
    enc_finish_frame(p, p->slots[si]);
    retire(p, p->slots[si]);
  }
}

extern "C" void ojphgpu_enc_pipe_destroy(ojphgpu_enc_pipe* p)
{
  if (!p) return;
  (void)hipSetDevice(p->device);
  if (p->search_worker.joinable()) {                 // it hands its frames to the finishers: it ends first
    { std::lock_guard<std::mutex> lk(p->mu); p->stop_search = true; }
    p->cv_search.notify_all();
    p->search_worker.join();
  }
  { std::lock_guard<std::mutex> lk(p->mu); p->stop = true; }
  p->cv_work.notify_all();
  for (std::thread& t : p->finishers) t.join();
  for (hipStream_t s : { p->s_h2d, p->s_comp, p->s_d2h }) if (s) (void)hipStreamSynchronize(s);
  if (p->enc) ojphgpu_encoder_destroy(p->enc);
  for (EncSlot& s : p->slots) {
    s.h_in.release(); s.o.release(); s.h_lay.release(); s.h_cs.release();
    for (DeviceBuf* b : { &s.image, &s.cs.b, &s.pixels.b, &s.rgb.b }) b->release();
    for (hipEvent_t ev : { s.ev_in, s.ev_kern, s.ev_done }) if (ev) (void)hipEventDestroy(ev);
    delete s.rplan;
  }
  p->spare.release(); p->h_hist.release(); p->h_qdescs.release(); p->h_qerr.release();
  if (p->ev_trial) (void)hipEventDestroy(p->ev_trial);
  for (hipStream_t s : { p->s_h2d, p->s_comp, p->s_d2h }) if (s) (void)hipStreamDestroy(s);
  delete p;
}

extern "C" int ojphgpu_enc_pipe_create(const ojphgpu_plan* plan, int device, uint32_t depth, int container_bits,
                                        uint32_t host_threads, ojphgpu_enc_pipe** out)
{
  if (!plan || !out || depth < 2 || depth > 16 || (container_bits != 8 && container_bits != 16 && container_bits != 32)) return OJPHGPU_E_INVALID;
  *out = nullptr;
  return no_throw([&]() -> int {
    HIPCHK(hipSetDevice(device));
    ojphgpu_enc_pipe* p = new (std::nothrow) ojphgpu_enc_pipe();
    if (!p) return OJPHGPU_E_NOMEM;
    struct Owner { ojphgpu_enc_pipe* p; ~Owner() { if (p) ojphgpu_enc_pipe_destroy(p); } } owner{ p };
    const Plan& P = plan->plan;
    p->handle = plan; p->P = &P; p->device = device; p->container = container_bits; p->depth = depth;
    if (container_bits != 32) for (const CompGeo& g : P.comps) if (g.bit_depth > (uint32_t)container_bits) return OJPHGPU_E_INVALID;
    for (hipStream_t* s : { &p->s_h2d, &p->s_comp }) HIPCHK(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    HIPCHK(create_copy_out_stream(&p->s_d2h));
    int rc = ojphgpu_encoder_create_joined(plan, device, p->s_comp, &p->enc);
    if (rc) return rc;
    (void)ojphgpu_encoder_set_timing(p->enc, 0);
    ojphgpu_encoder* e = p->enc;
    const size_t nb = e->block_ids.size();
    p->frame_bytes = (size_t)P.frame_elems * (size_t)(container_bits / 8);
    p->ho.bytes = p->frame_bytes;
    p->res_bytes = nb * sizeof(ojphgpu_cb_result) + 16;
    // the codestream of a frame: sized from the samples (1 byte each is generous for natural content), grown when a frame needs more
    const size_t cs_guess = std::min<size_t>((size_t)e->out_cap, (size_t)P.frame_elems + (1u << 20));
    p->slots.resize(depth);
    for (EncSlot& s : p->slots) {
      if (s.h_in.reserve(p->frame_bytes + 64) || s.o.h_res.reserve(p->res_bytes + 64) || s.h_cs.reserve(cs_guess)) return OJPHGPU_E_NOMEM;
      if (s.image.alloc(p->frame_bytes + 64) || s.o.out.alloc((size_t)e->out_cap + 64) || s.o.counters.alloc(e->counters_bytes) ||
          s.cs.reserve(cs_guess)) return OJPHGPU_E_NOMEM;
      const size_t lay_guess = nb * sizeof(T2Job) + nb * 8 + (1u << 16);
      if (s.h_lay.reserve(lay_guess)) return OJPHGPU_E_NOMEM;
      for (hipEvent_t* ev : { &s.ev_in, &s.ev_kern, &s.ev_done }) HIPCHK(hipEventCreateWithFlags(ev, hipEventDisableTiming | hipEventReleaseToSystem));
    }
    const uint32_t nthreads = host_threads ? std::min<uint32_t>(host_threads, 16) : 2;
    for (uint32_t i = 0; i < nthreads; ++i) p->finishers.emplace_back(enc_finisher, p);
    owner.p = nullptr;
    *out = p;
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_enc_pipe_acquire(ojphgpu_enc_pipe* p, void** h_frame, size_t* bytes)
{
  if (!p || !h_frame || p->dead) return OJPHGPU_E_INVALID;
  EncSlot& s = p->slots[p->n_acq % p->depth];
  {
    std::lock_guard<std::mutex> lk(p->mu);
    if (s.state == ACQUIRED) { *h_frame = s.h_in.p; if (bytes) *bytes = p->ho.bytes; return OJPHGPU_OK; }   // asked twice
    if (s.state != FREE) return OJPHGPU_E_AGAIN;      // every slot is in flight: collect a codestream first
    s.state = ACQUIRED;
  }
  *h_frame = s.h_in.p;
  if (bytes) *bytes = p->ho.bytes;
  return OJPHGPU_OK;
}

// before the first _acquire: the hand-over may still be set (and set again)
static int enc_set_handover(ojphgpu_enc_pipe* p, int kind, int arg, int big_endian, const ojphgpu_colour_spec* spec = nullptr, int chroma = 0)
{
  if (!p || p->dead || p->n_acq != 0 || p->slots[0].state != FREE) return OJPHGPU_E_INVALID;
  return handover_set(p, &EncSlot::h_in, false, 0, kind, arg, big_endian, spec, chroma);
}

// mode of a _set_video_chroma call: COSITED, or 0 together with format 0 (planes again)
static bool chroma_mode_ok(int format, int mode) { return mode == OJPHGPU_CHROMA_COSITED || (mode == 0 && format == 0); }

extern "C" int ojphgpu_enc_pipe_set_pixels(ojphgpu_enc_pipe* p, int pixel_bits, int big_endian) { return enc_set_handover(p, PIXELS, pixel_bits, big_endian); }
extern "C" int ojphgpu_enc_pipe_set_packed(ojphgpu_enc_pipe* p, int bits) { return enc_set_handover(p, PACKED, bits, 0); }
extern "C" int ojphgpu_enc_pipe_set_video(ojphgpu_enc_pipe* p, int format) { return enc_set_handover(p, VIDEO, format, 0); }
extern "C" int ojphgpu_enc_pipe_set_video_colour(ojphgpu_enc_pipe* p, int format, const ojphgpu_colour_spec* spec)
{
  return spec ? enc_set_handover(p, VIDEO, format, 0, spec) : OJPHGPU_E_INVALID;
}

extern "C" int ojphgpu_enc_pipe_set_video_chroma(ojphgpu_enc_pipe* p, int format, int mode)
{
  return chroma_mode_ok(format, mode) ? enc_set_handover(p, VIDEO, format, 0, nullptr, OJPHGPU_CHROMA_COSITED) : OJPHGPU_E_INVALID;
}

extern "C" int ojphgpu_enc_pipe_submit(ojphgpu_enc_pipe* p)
{
  if (!p || p->dead) return OJPHGPU_E_INVALID;
  const uint32_t si = (uint32_t)(p->n_acq % p->depth);
  EncSlot& s = p->slots[si];
  { std::lock_guard<std::mutex> lk(p->mu); if (s.state != ACQUIRED) return OJPHGPU_E_INVALID; }
  HIPCHK(hipSetDevice(p->device));
  s.rc = 0; s.cs_len = 0; s.t_t2 = 0; s.t_submit = now_ms();
  { const int r0 = upload(p->mode, p->s_h2d, handover_device_side(p->ho, s), s.h_in, 0, p->ho.bytes); if (r0) return r0; }
  HIPCHK(hipEventRecord(s.ev_in, p->s_h2d));
  if (p->searching()) {                              // everything on the compute stream is the search worker's, frame by frame
    std::lock_guard<std::mutex> lk(p->mu);
    s.budget = p->max_bytes; s.target = p->max_sse; s.cap = p->capped ? p->cap_bytes : 0; s.found = EncSearchResult{};
    s.state = SUBMITTED;
    p->search_work.push_back(si);
    p->n_acq++; p->n_sub++;
    p->cv_search.notify_one();
    return OJPHGPU_OK;
  }
  int rc = enc_begin_frame(p, s);
  if (rc) return rc;
  const RateTrialOut coded = s.o.trial(p->enc->block_ids.size(), nullptr);
  rc = publish_words_launch(p->s_comp, coded.d_publish, coded.d_counters, 2);
  if (rc) return rc;
  HIPCHK(hipEventRecord(s.ev_kern, p->s_comp));
  {
    std::lock_guard<std::mutex> lk(p->mu);
    s.state = SUBMITTED;
    p->work.push_back(si);
    p->n_acq++; p->n_sub++;
  }
  p->cv_work.notify_one();
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_enc_pipe_collect(ojphgpu_enc_pipe* p, const uint8_t** h_codestream, size_t* len)
{
  if (!p || !h_codestream || !len) return OJPHGPU_E_INVALID;
  std::unique_lock<std::mutex> lk(p->mu);
  if (p->n_col >= p->n_sub) return OJPHGPU_E_INVALID;            // nothing in flight
  if (p->n_col > 0) {                                              // the codestream handed out last time is released now
    EncSlot& prev = p->slots[(p->n_col - 1) % p->depth];
    if (prev.state == HELD) prev.state = FREE;
  }
  EncSlot& s = p->slots[p->n_col % p->depth];
  p->cv_done.wait(lk, [&] { return s.state == DONE; });
  p->n_col++;
  p->last = s.found;
  if (s.rc) { s.state = FREE; return s.rc; }
  s.state = HELD;
  *h_codestream = s.h_cs.p; *len = s.cs_len;
  return OJPHGPU_OK;
}

// Switching a search mode on, once the encoder has taken it (ojphgpu_encoder_set_budget / _set_quality: refused there, the
// encoder and the pipe are as they were).  From here the encoder runs in that mode and the buffers change hands: a failure
// (memory, the thread) leaves neither a plain pipe nor a searching one, so the pipe is dead -- it refuses everything but
// _destroy -- until the setter that called this has its own buffers too and says otherwise.  Here: every slot's output set
// at the bound of the finest step and its copy of the plan, the spare set's pinned half, the event of the trials, the worker.
static int enc_search_on(ojphgpu_enc_pipe* p, bool with_spare)
{
  ojphgpu_encoder* e = p->enc;
  p->dead = true;
  for (EncSlot& s : p->slots) {
    s.o.out.release(); s.o.counters.release();
    if (s.o.out.alloc((size_t)e->out_cap + 64) || s.o.counters.alloc(e->counters_bytes)) return OJPHGPU_E_NOMEM;
    if (!s.rplan) s.rplan = new ojphgpu_plan{ *p->P };
  }
  if (with_spare && p->spare.h_res.reserve(p->res_bytes + 64)) return OJPHGPU_E_NOMEM;
  if (!p->ev_trial) HIPCHK(hipEventCreateWithFlags(&p->ev_trial, hipEventDisableTiming | hipEventReleaseToSystem));
  p->search_worker = std::thread(enc_search_worker, p);
  p->hint = -1;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_enc_pipe_set_budget(ojphgpu_enc_pipe* p, uint64_t max_bytes)
{
  if (!p || p->dead || p->quality_on) return OJPHGPU_E_INVALID;
  if (p->n_acq != 0 || p->slots[0].state != FREE) {  // frames have been handed out: the mode stays, the budget may move
    if (!p->budget_on || max_bytes == 0) return OJPHGPU_E_INVALID;
    p->max_bytes = max_bytes;
    return OJPHGPU_OK;
  }
  if (max_bytes == 0) return p->budget_on ? OJPHGPU_E_INVALID : OJPHGPU_OK;   // (once on, the buffers and the worker are there)
  if (p->budget_on) { p->max_bytes = max_bytes; return OJPHGPU_OK; }
  return no_throw([&]() -> int {
    HIPCHK(hipSetDevice(p->device));
    ojphgpu_encoder* e = p->enc;
    int rc = ojphgpu_encoder_set_budget(e, max_bytes);   // the refusals, the statistics, scratch and output bound of the finest step
    if (rc || (rc = enc_search_on(p, true)) != 0) return rc;
    p->spare.out = e->out; p->spare.counters = e->counters;   // the encoder's own output set becomes the spare
    e->out = DeviceBuf(); e->counters = DeviceBuf();
    if (p->h_hist.reserve(e->rate->h_hist.size() * 4 + 64)) return OJPHGPU_E_NOMEM;
    p->budget_on = true; p->max_bytes = max_bytes; p->dead = false;
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_enc_pipe_rate_info(ojphgpu_enc_pipe* p, ojphgpu_rate_info* info)
{
  if (!p || !info) return OJPHGPU_E_INVALID;
  std::lock_guard<std::mutex> lk(p->mu);
  if (!p->last.have_rate) return OJPHGPU_E_INVALID;
  *info = p->last.rate;
  return OJPHGPU_OK;
}

// The mode is the budget's, with another search: on from before the first _acquire, or never; the target may move between
// frames; 0 is a target, so the first call is the switch.
extern "C" int ojphgpu_enc_pipe_set_quality(ojphgpu_enc_pipe* p, uint64_t max_sse)
{
  if (!p || p->dead || p->budget_on) return OJPHGPU_E_INVALID;
  if (p->n_acq != 0 || p->slots[0].state != FREE) {  // frames have been handed out: the mode stays, the target may move
    if (!p->quality_on) return OJPHGPU_E_INVALID;
    p->max_sse = max_sse;
    return OJPHGPU_OK;
  }
  if (p->quality_on) { p->max_sse = max_sse; return OJPHGPU_OK; }
  return no_throw([&]() -> int {
    HIPCHK(hipSetDevice(p->device));
    ojphgpu_encoder* e = p->enc;
    // the refusals; scratch and output bound of the finest step, the second arena, the synthesis-only decoder and the
    // int32 reconstructed frame
    int rc = ojphgpu_encoder_set_quality(e, max_sse);
    if (rc || (rc = enc_search_on(p, false)) != 0) return rc;
    e->out.release(); e->counters.release();             // a frame's blocks are coded once: no spare, the encoder's own set goes
    if (p->h_qdescs.reserve(e->quality->h_descs.size() * sizeof(ojphgpu_requant_desc) + 64) ||
        p->h_qerr.reserve(p->P->comps.size() * sizeof(ojphgpu_frame_err) + 64)) return OJPHGPU_E_NOMEM;
    p->q_by_index.assign(OJPHGPU_RATE_GRID, {});
    p->quality_on = true; p->max_sse = max_sse; p->dead = false;
    return OJPHGPU_OK;
  });
}

// A target under a byte cap: a quality pipe that also takes what a budget pipe takes -- the encoder's own output set as the
// spare, the pinned histograms -- so it is that from the first call, or never: a quality pipe made without a cap has
// released the set and cannot gain one, and a capped pipe's cap cannot go back to 0.
extern "C" int ojphgpu_enc_pipe_set_quality_capped(ojphgpu_enc_pipe* p, uint64_t max_sse, uint64_t cap_bytes)
{
  if (!p || p->dead || p->budget_on) return OJPHGPU_E_INVALID;
  if (cap_bytes == 0) return p->capped ? OJPHGPU_E_INVALID : ojphgpu_enc_pipe_set_quality(p, max_sse);
  if (p->quality_on || p->n_acq != 0 || p->slots[0].state != FREE) {   // the mode stays, both values may move
    if (!p->capped) return OJPHGPU_E_INVALID;
    p->max_sse = max_sse; p->cap_bytes = cap_bytes;
    return OJPHGPU_OK;
  }
  return no_throw([&]() -> int {
    HIPCHK(hipSetDevice(p->device));
    ojphgpu_encoder* e = p->enc;
    int rc = ojphgpu_encoder_set_quality(e, max_sse);        // (the encoder's own cap stays 0: the pipe runs the search)
    if (rc || (rc = enc_search_on(p, true)) != 0) return rc;
    p->spare.out = e->out; p->spare.counters = e->counters;   // the encoder's own output set becomes the spare
    e->out = DeviceBuf(); e->counters = DeviceBuf();
    if (p->h_hist.reserve(e->rate->h_hist.size() * 4 + 64) ||
        p->h_qdescs.reserve(e->quality->h_descs.size() * sizeof(ojphgpu_requant_desc) + 64) ||
        p->h_qerr.reserve(p->P->comps.size() * sizeof(ojphgpu_frame_err) + 64)) return OJPHGPU_E_NOMEM;
    p->q_by_index.assign(OJPHGPU_RATE_GRID, {});
    p->quality_on = true; p->capped = true; p->max_sse = max_sse; p->cap_bytes = cap_bytes; p->hint_b = -1; p->dead = false;
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_enc_pipe_capped_info(ojphgpu_enc_pipe* p, ojphgpu_capped_info* info)
{
  if (!p || !info) return OJPHGPU_E_INVALID;
  std::lock_guard<std::mutex> lk(p->mu);
  if (!p->last.have_capped) return OJPHGPU_E_INVALID;
  *info = p->last.capped;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_enc_pipe_quality_info(ojphgpu_enc_pipe* p, ojphgpu_quality_info* info, uint32_t* first_guess)
{
  if (!p || !info || !first_guess) return OJPHGPU_E_INVALID;
  std::lock_guard<std::mutex> lk(p->mu);
  if (!p->last.have_quality) return OJPHGPU_E_INVALID;
  *info = p->last.quality; *first_guess = p->last.first_guess;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_enc_pipe_quality_comp(ojphgpu_enc_pipe* p, uint32_t comp, uint64_t* sse, uint32_t* pae)
{
  if (!p || !sse || !pae) return OJPHGPU_E_INVALID;
  std::lock_guard<std::mutex> lk(p->mu);
  if (!(p->last.have_quality || p->last.have_capped) || comp >= p->last.comps.size()) return OJPHGPU_E_INVALID;
  *sse = p->last.comps[comp].sse; *pae = p->last.comps[comp].pae;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_enc_pipe_stats(ojphgpu_enc_pipe* p, double out[4])
{
  if (!p || !out) return OJPHGPU_E_INVALID;
  std::lock_guard<std::mutex> lk(p->mu);
  out[0] = (double)p->n_done;
  out[1] = p->n_done ? p->sum_t2 / (double)p->n_done : 0.0;          // host Tier-2 (layout) per frame, ms
  out[2] = p->n_done ? p->sum_latency / (double)p->n_done : 0.0;     // submit -> codestream in pinned memory, ms
  out[3] = (double)pool_threads();
  return OJPHGPU_OK;
}

// =============================================================================================
// decoder pipe
// =============================================================================================
struct DecSlot {
  SlotState state = FREE;
  Pinned h_cs, h_descs, h_img, h_status;
  Grow data, pixels;                                // pixels: the frame as it is handed back, unless that is as planes
  Grow rgb;                                         // a hand-over of two launches (a colour spec: R, G, B; a chroma stage: the format's planes): what stands between them
  DeviceBuf image, cb_descs, status, runs;          // runs: a view's run table, copied there for the gather kernel
  hipEvent_t ev_in = nullptr, ev_kern = nullptr, ev_done = nullptr;
  size_t cs_len = 0;
  int rc = 0; uint32_t failed = 0;
  double t_submit = 0, t_done = 0, t_parse = 0;
  uint64_t view_info[5] = {};                       // see ojphgpu_dec_pipe_view_info
};

struct ojphgpu_dec_pipe {
  ojphgpu_plan* first = nullptr;                     // parsed from the first codestream: the geometry of every frame
  const Plan* P = nullptr;
  int device = 0, container = 16, resilient = 0;
  // a view (ojphgpu_dec_pipe_create_view): what every frame's plan is restricted by, as the first one's was; the frame's
  // bytes then go up as runs, gathered by a kernel from the slot's pinned codestream (the run table: in h_descs at runs_off,
  // copied to the slot's `runs` in HBM)
  bool view = false, has_region = false;
  uint32_t skip_data = 0, skip_recon = 0, region[4] = {};
  size_t runs_off = 0;
  uint64_t last_view_info[5] = {}; bool have_view_info = false;   // of the frame collected last
  int mode = copy_mode("OJPHGPU_DEC_COPY_MODE", 0);
  uint32_t depth = 0;
  // Consecutive frames go to different decoder objects (own scratch, own compute stream): step 1 of the block decoder
  // is a 0.2 ms chain that leaves most of the chip idle whatever the frame size, so for frames below ~8K one compute
  // stream running frame after frame sets the pace (4K 8-bit: 0.82 ms per frame against 0.44 ms of PCIe); with two
  // objects frame n+1's chains run beside frame n's step 2 and synthesis.  The objects run without their side
  // stream (streams share 4 hardware queues; the frames overlap each other instead).
  static constexpr uint32_t MAX_OBJECTS = 4;
  uint32_t nobj = 0;
  ojphgpu_decoder* decs[MAX_OBJECTS] = {};
  hipStream_t s_comps[MAX_OBJECTS] = {};
  std::mutex enqueue_mus[MAX_OBJECTS];
  hipStream_t s_h2d = nullptr, s_d2h = nullptr;
  std::vector<DecSlot> slots;
  size_t frame_bytes = 0;
  Handover ho;                                      // how frames are handed back; ho.bytes: what _collect hands out
  uint64_t n_acq = 0, n_sub = 0, n_col = 0;
  std::mutex mu; std::condition_variable cv_work, cv_done;
  std::deque<uint32_t> work; bool stop = false;
  std::vector<std::thread> workers;
  double sum_parse = 0, sum_latency = 0; uint64_t n_done = 0;
};

static void dec_process_frame(ojphgpu_dec_pipe* p, DecSlot& s)
{
  const Plan& P = *p->P;
  const uint32_t k = (uint32_t)(&s - p->slots.data()) % p->nobj;
  ojphgpu_decoder* d = p->decs[k];
  hipStream_t s_comp = p->s_comps[k];
  auto fail = [&](int rc) { s.rc = rc; };
  if (hipSetDevice(p->device) != hipSuccess) return fail(OJPHGPU_E_HIP);
  const double t0 = now_ms();
  ojphgpu_plan* q = nullptr;
  int rc = ojphgpu_t2_parse(s.h_cs.p, s.cs_len, p->resilient, &q);
  if (rc) return fail(rc);
  struct Hold { ojphgpu_plan* q; ~Hold() { ojphgpu_plan_destroy(q); } } hold{ q };
  rc = no_throw([&]() -> int {
    int r2;
    if ((p->skip_data || p->skip_recon) && (r2 = ojphgpu_plan_restrict_resolution(q, p->skip_data, p->skip_recon)) != 0) return r2;
    if (p->has_region && (r2 = ojphgpu_plan_restrict_region(q, p->region[0], p->region[1], p->region[2], p->region[3])) != 0) return r2;
    const Plan& Q = q->plan;
    r2 = ojphgpu_same_frame_geometry(P, Q, true);
    if (r2) return r2;
    const size_t nb = d->block_ids.size();
    ojphgpu_cb_desc* bd = (ojphgpu_cb_desc*)s.h_descs.p;
    DecFrameInfo fi;
    ojphgpu_decoder_fill_descs(P, Q, d->block_ids, 0, 0, bd, fi, p->view);
    uint64_t coded = 0;
    for (size_t i = 0; i < nb; ++i) coded += (uint64_t)bd[i].len1 + bd[i].len2;
    s.view_info[0] = nb; s.view_info[1] = Q.blocks.size(); s.view_info[2] = fi.len; s.view_info[3] = fi.runs.size(); s.view_info[4] = coded;
    uint64_t nquads = 0, naux = 0;
    if (ojphgpu_ht_decode_layout(bd, (uint32_t)nb, &nquads, &naux) != OJPHGPU_OK) return OJPHGPU_E_INVALID;
    if ((naux + 16) * 4 > d->aux.n || (nquads + 16) * 4 > d->quads.n) return OJPHGPU_E_INVALID;     // sized for the worst case at create
    s.t_parse = now_ms() - t0;
    if (p->view) {                                     // the runs of the view's blocks: every one inside this codestream
      if (fi.runs.size() > nb) return OJPHGPU_E_INVALID;          // (a run holds a block at least: the table's room)
      for (const DecRun& r : fi.runs) if (r.src > s.cs_len || r.n > s.cs_len - r.src) return OJPHGPU_E_CODESTREAM;
    } else if (fi.first + fi.len > s.cs_len) return OJPHGPU_E_CODESTREAM;
    if (s.data.reserve((size_t)fi.data_bytes() + (size_t)fi.len / 4 + 128)) return OJPHGPU_E_NOMEM;
    if (p->view) {
      // the table goes into the slot's pinned descriptor memory behind the block descriptors and from there in one small
      // copy into HBM: every workgroup of the kernel reads a window of it per step, which would otherwise cross PCIe
      // beside the payload.  The kernel writes all of [0, fi.len): the runs, and zeros over whatever a longer frame left
      if (!fi.runs.empty()) memcpy(s.h_descs.p + p->runs_off, fi.runs.data(), fi.runs.size() * sizeof(DecRun));
      if ((r2 = upload(p->mode, p->s_h2d, s.runs.p, s.h_descs, p->runs_off, fi.runs.size() * sizeof(DecRun))) != 0) return r2;
      if ((r2 = gather_runs_launch(p->s_h2d, s.h_cs.d, s.h_cs.cap & ~(size_t)3, s.runs.p, (uint32_t)fi.runs.size(),
                                   s.data.b.p, fi.len)) != 0) return r2;
    } else if ((r2 = upload(p->mode, p->s_h2d, s.data.b.p, s.h_cs, (size_t)fi.first, (size_t)fi.len)) != 0) return r2;
    if ((r2 = ojphgpu_decoder_upload_pads(p->s_h2d, (uint8_t*)s.data.b.p, s.h_cs.p, s.cs_len, fi.pads)) != 0) return r2;   // (damaged codestreams only)
    if ((r2 = upload(p->mode, p->s_h2d, s.cb_descs.p, s.h_descs, 0, nb * sizeof(ojphgpu_cb_desc))) != 0) return r2;
    HIPCHK(hipEventRecord(s.ev_in, p->s_h2d));
    // kernels of the frame on the object's compute stream, then the downloads; `separate`: the repeat a fused launch asked for
    const size_t st_bytes = ((nb + 3) & ~(size_t)3) + 4;    // the status bytes + the RETRY word behind them
    uint32_t epoch = 0; bool was_fused = false;
    auto run_and_fetch = [&](bool separate) -> int {
      int r3;
      {
        // a decoder object is shared by the frames in flight on it: what a run reads is set and enqueued under a lock
        std::lock_guard<std::mutex> lk(p->enqueue_mus[k]);
        HIPCHK(hipStreamWaitEvent(s_comp, s.ev_in, 0));
        d->o_cb_descs = s.cb_descs.p; d->o_data = s.data.b.p; d->o_status = s.status.p;
        d->any_refine = fi.any_refine; d->kinds = fi.kinds; d->max_len1 = fi.max_len1;
        d->force_separate = separate;
        r3 = ojphgpu_decoder_run_container(d, s.image.p, p->container);
        d->force_separate = false;
        if (r3) return r3;
        epoch = d->fused_epoch; was_fused = d->last_fused;
        if (separate) d->fused_retries++;
        if ((r3 = handover_launch(s_comp, p->ho, P, p->container, false, s.pixels.b.p, s.image.p, s.rgb.b.p)) != 0) return r3;   // planes -> the frame as it is handed back
        HIPCHK(hipEventRecord(s.ev_kern, s_comp));
      }
      HIPCHK(hipStreamWaitEvent(p->s_d2h, s.ev_kern, 0));
      if ((r3 = download(p->mode, p->s_d2h, s.h_img, handover_device_side(p->ho, s), p->ho.bytes)) != 0) return r3;       // beside the next frame's upload
      if ((r3 = download(p->mode, p->s_d2h, s.h_status, s.status.p, st_bytes)) != 0) return r3;
      HIPCHK(hipEventRecord(s.ev_done, p->s_d2h));
      HIPCHK(hipEventSynchronize(s.ev_done));
      return OJPHGPU_OK;
    };
    if ((r2 = run_and_fetch(false)) != 0) return r2;
    // the fused block-decoder launch of this run gave up waiting (the chip was held up for seconds by other work) and marked
    // the run instead of failing blocks: once more through the separate launches (see ojphgpu_decoder_failed_blocks)
    if (was_fused) {
      const bool again = ojphgpu_fused_retry_wanted(s.h_status.p, (uint32_t)nb, epoch);
      { std::lock_guard<std::mutex> lk(p->enqueue_mus[k]); d->fused_outcome(again); }
      if (again && (r2 = run_and_fetch(true)) != 0) return r2;
    }
    uint32_t failed = 0;
    for (size_t i = 0; i < nb; ++i) failed += s.h_status.p[i] != 0;
    s.failed = failed;
    return OJPHGPU_OK;
  });
  if (rc) {
    // the slot goes DONE -> FREE next: whatever was enqueued for it must have finished before _acquire rewrites or
    // re-reserves its buffers, and the shared decoder object must not keep pointing at them
    hipStreamSynchronize(p->s_h2d); hipStreamSynchronize(s_comp); hipStreamSynchronize(p->s_d2h);
    std::lock_guard<std::mutex> lk(p->enqueue_mus[k]);
    if (d->o_cb_descs == s.cb_descs.p) { d->o_cb_descs = nullptr; d->o_data = nullptr; d->o_status = nullptr; }
    fail(rc);
  }
}

// the frame of a slot is over, whatever its outcome (s.rc): collectable, and counted
static void retire(ojphgpu_dec_pipe* p, DecSlot& s)
{
  {
    std::lock_guard<std::mutex> lk(p->mu);
    s.t_done = now_ms();
    s.state = DONE;
    p->sum_parse += s.t_parse; p->sum_latency += s.t_done - s.t_submit; p->n_done++;
  }
  p->cv_done.notify_all();
}

static void dec_worker(ojphgpu_dec_pipe* p)
{
  for (uint32_t si; pop_work(p->mu, p->cv_work, p->work, p->stop, si);) {
    dec_process_frame(p, p->slots[si]);
    retire(p, p->slots[si]);
  }
}

extern "C" void ojphgpu_dec_pipe_destroy(ojphgpu_dec_pipe* p)
{
  if (!p) return;
  (void)hipSetDevice(p->device);
  { std::lock_guard<std::mutex> lk(p->mu); p->stop = true; }
  p->cv_work.notify_all();
  for (std::thread& t : p->workers) t.join();
  for (hipStream_t s : { p->s_h2d, p->s_comps[0], p->s_comps[1], p->s_comps[2], p->s_comps[3], p->s_d2h }) if (s) (void)hipStreamSynchronize(s);
  for (ojphgpu_decoder* d : p->decs) if (d) ojphgpu_decoder_destroy(d);
  for (DecSlot& s : p->slots) {
    s.h_cs.release(); s.h_descs.release(); s.h_img.release(); s.h_status.release();
    for (DeviceBuf* b : { &s.data.b, &s.image, &s.cb_descs, &s.status, &s.pixels.b, &s.rgb.b, &s.runs }) b->release();
    for (hipEvent_t ev : { s.ev_in, s.ev_kern, s.ev_done }) if (ev) (void)hipEventDestroy(ev);
  }
  for (hipStream_t s : { p->s_h2d, p->s_comps[0], p->s_comps[1], p->s_comps[2], p->s_comps[3], p->s_d2h }) if (s) (void)hipStreamDestroy(s);
  if (p->first) ojphgpu_plan_destroy(p->first);
  delete p;
}

extern "C" int ojphgpu_dec_pipe_create(const uint8_t* h_codestream, size_t len, int resilient, int device, uint32_t depth,
                                        int container_bits, uint32_t host_threads, ojphgpu_dec_pipe** out)
{
  return ojphgpu_dec_pipe_create_view(h_codestream, len, resilient, 0, 0, nullptr, device, depth, container_bits, host_threads, out);
}

extern "C" int ojphgpu_dec_pipe_create_view(const uint8_t* h_codestream, size_t len, int resilient, uint32_t skipped_res_for_data,
                                             uint32_t skipped_res_for_recon, const uint32_t* region, int device, uint32_t depth,
                                             int container_bits, uint32_t host_threads, ojphgpu_dec_pipe** out)
{
  if (!h_codestream || !out || depth < 2 || depth > 16 || (container_bits != 8 && container_bits != 16 && container_bits != 32)) return OJPHGPU_E_INVALID;
  *out = nullptr;
  return no_throw([&]() -> int {
    HIPCHK(hipSetDevice(device));
    ojphgpu_dec_pipe* p = new (std::nothrow) ojphgpu_dec_pipe();
    if (!p) return OJPHGPU_E_NOMEM;
    struct Owner { ojphgpu_dec_pipe* p; ~Owner() { if (p) ojphgpu_dec_pipe_destroy(p); } } owner{ p };
    int rc = ojphgpu_t2_parse(h_codestream, len, resilient, &p->first);
    if (rc) return rc;
    // the view: the first plan restricted as a single decoder's would be (the refusals of the two calls are the pipe's)
    if ((skipped_res_for_data || skipped_res_for_recon) &&
        (rc = ojphgpu_plan_restrict_resolution(p->first, skipped_res_for_data, skipped_res_for_recon)) != 0) return rc;
    if (region && (rc = ojphgpu_plan_restrict_region(p->first, region[0], region[1], region[2], region[3])) != 0) return rc;
    p->skip_data = skipped_res_for_data; p->skip_recon = skipped_res_for_recon; p->has_region = region != nullptr;
    if (region) memcpy(p->region, region, sizeof(p->region));
    p->view = p->has_region || skipped_res_for_data || skipped_res_for_recon;
    const Plan& P = p->first->plan;
    p->P = &P; p->device = device; p->container = container_bits; p->depth = depth; p->resilient = resilient;
    if (container_bits != 32) for (const CompGeo& g : P.comps) if (g.bit_depth > (uint32_t)container_bits) return OJPHGPU_E_INVALID;
    HIPCHK(hipStreamCreateWithFlags(&p->s_h2d, hipStreamNonBlocking));
    HIPCHK(create_copy_out_stream(&p->s_d2h));
    {
      const char* e = getenv("OJPHGPU_DEC_PIPE_OBJECTS"); const long v = e ? atol(e) : 0;
      p->nobj = v >= 1 && v <= (long)ojphgpu_dec_pipe::MAX_OBJECTS ? (uint32_t)v : 2u;
      p->nobj = std::min(p->nobj, depth);
    }
    for (uint32_t k = 0; k < p->nobj; ++k) {
      HIPCHK(hipStreamCreateWithFlags(&p->s_comps[k], hipStreamNonBlocking));
      rc = ojphgpu_decoder_create_joined(p->first, device, p->s_comps[k], 0, (uint32_t)p->first->plan.tiles.size(), &p->decs[k]);
      if (rc) return rc;
      ojphgpu_decoder* dk = p->decs[k];
      (void)ojphgpu_decoder_set_timing(dk, 0);
      if (p->nobj > 1 && dk->side) {                     // no fork inside a frame: the frames overlap each other
        (void)hipStreamDestroy(dk->side); dk->side = nullptr; dk->n_low = 0;
      }
      // the flat VLC / MEL strings of any later frame fit: the worst case of every block (Lcup <= 4079 + slack)
      uint64_t worst = (uint64_t)dk->block_ids.size() * ojphgpu_ht_decode_aux_words(4079) + 64;
      if (P.any_wide)                                      // 64-bit sample path: the flat MagSgn strings, bounded by what a block of that size can code
        for (uint32_t id : dk->block_ids) {
          const Block& k = P.blocks[id]; const Band& B = P.bands[k.band];
          if (is_wide(P, B.comp)) worst += ojphgpu::ht_decode64_extra_aux_words(block_scratch_bytes(k.r.w, k.r.h, 62));
        }
      dk->aux.release();
      if (dk->aux.alloc((size_t)worst * 4 + 64)) return OJPHGPU_E_NOMEM;
    }
    ojphgpu_decoder* d = p->decs[0];
    const size_t nb = d->block_ids.size();
    p->frame_bytes = (size_t)P.frame_elems * (size_t)(container_bits / 8);
    p->ho.bytes = p->frame_bytes;
    p->runs_off = (nb * sizeof(ojphgpu_cb_desc) + 63) & ~(size_t)63;   // a view's run table: a run holds a block at least
    const size_t descs_bytes = p->view ? p->runs_off + nb * sizeof(DecRun) : nb * sizeof(ojphgpu_cb_desc);
    p->slots.resize(depth);
    for (DecSlot& s : p->slots) {
      if (s.h_cs.reserve(len + len / 4 + (1u << 16)) || s.h_descs.reserve(descs_bytes + 64) ||
          s.h_img.reserve(p->frame_bytes + 64) || s.h_status.reserve(nb + 64)) return OJPHGPU_E_NOMEM;
      if (s.data.reserve(len + len / 4 + 64) || s.image.alloc((size_t)P.frame_elems * 4 + 64) || s.cb_descs.alloc(nb * sizeof(ojphgpu_cb_desc) + 64) ||
          s.status.alloc(nb + 64) || (p->view && s.runs.alloc(nb * sizeof(DecRun) + 64))) return OJPHGPU_E_NOMEM;
      HIPCHK(hipMemset(s.status.p, 0, nb + 64));
      for (hipEvent_t* ev : { &s.ev_in, &s.ev_kern, &s.ev_done }) HIPCHK(hipEventCreateWithFlags(ev, hipEventDisableTiming | hipEventReleaseToSystem));
    }
    const uint32_t nthreads = host_threads ? std::min<uint32_t>(host_threads, 16) : 2;
    for (uint32_t i = 0; i < nthreads; ++i) p->workers.emplace_back(dec_worker, p);
    owner.p = nullptr;
    *out = p;
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_dec_pipe_acquire(ojphgpu_dec_pipe* p, size_t len, uint8_t** h_codestream)
{
  if (!p || !h_codestream || len == 0) return OJPHGPU_E_INVALID;
  DecSlot& s = p->slots[p->n_acq % p->depth];
  {
    std::lock_guard<std::mutex> lk(p->mu);
    if (s.state != FREE && s.state != ACQUIRED) return OJPHGPU_E_AGAIN;     // every slot is in flight: collect a frame first
    s.state = ACQUIRED;
  }
  if (hipSetDevice(p->device) != hipSuccess) return OJPHGPU_E_HIP;
  if (s.h_cs.reserve(len + len / 4 + 64)) { std::lock_guard<std::mutex> lk(p->mu); s.state = FREE; return OJPHGPU_E_NOMEM; }
  s.cs_len = len;
  *h_codestream = s.h_cs.p;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_dec_pipe_submit(ojphgpu_dec_pipe* p)
{
  if (!p) return OJPHGPU_E_INVALID;
  const uint32_t si = (uint32_t)(p->n_acq % p->depth);
  DecSlot& s = p->slots[si];
  std::lock_guard<std::mutex> lk(p->mu);
  if (s.state != ACQUIRED) return OJPHGPU_E_INVALID;
  s.rc = 0; s.failed = 0; s.t_submit = now_ms();
  memset(s.view_info, 0, sizeof(s.view_info));
  s.state = SUBMITTED;
  p->work.push_back(si);
  p->n_acq++; p->n_sub++;
  p->cv_work.notify_one();
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_dec_pipe_collect(ojphgpu_dec_pipe* p, const void** h_frame, size_t* bytes, uint32_t* failed_blocks)
{
  if (!p || !h_frame) return OJPHGPU_E_INVALID;
  std::unique_lock<std::mutex> lk(p->mu);
  if (p->n_col >= p->n_sub) return OJPHGPU_E_INVALID;
  if (p->n_col > 0) {
    DecSlot& prev = p->slots[(p->n_col - 1) % p->depth];
    if (prev.state == HELD) prev.state = FREE;
  }
  DecSlot& s = p->slots[p->n_col % p->depth];
  p->cv_done.wait(lk, [&] { return s.state == DONE; });
  p->n_col++;
  memcpy(p->last_view_info, s.view_info, sizeof(s.view_info)); p->have_view_info = true;
  if (s.rc) { s.state = FREE; return s.rc; }
  s.state = HELD;
  *h_frame = s.h_img.p;
  if (bytes) *bytes = p->ho.bytes;
  if (failed_blocks) *failed_blocks = s.failed;
  return (s.failed && !p->resilient) ? OJPHGPU_E_BLOCK : OJPHGPU_OK;
}

// before the first _submit: the hand-over may still be set (and set again)
static int dec_set_handover(ojphgpu_dec_pipe* p, int kind, int arg, int big_endian, const ojphgpu_colour_spec* spec = nullptr, int chroma = 0)
{
  if (!p || p->n_sub != 0) return OJPHGPU_E_INVALID;
  const int odd_origin = !p->has_region ? 0 : ((p->region[0] & 1u) ? ODD_X0 : 0) | ((p->region[1] & 1u) ? ODD_Y0 : 0);
  return handover_set(p, &DecSlot::h_img, true, odd_origin, kind, arg, big_endian, spec, chroma);
}

extern "C" int ojphgpu_dec_pipe_set_pixels(ojphgpu_dec_pipe* p, int pixel_bits, int big_endian) { return dec_set_handover(p, PIXELS, pixel_bits, big_endian); }
extern "C" int ojphgpu_dec_pipe_set_packed(ojphgpu_dec_pipe* p, int bits) { return dec_set_handover(p, PACKED, bits, 0); }
extern "C" int ojphgpu_dec_pipe_set_video(ojphgpu_dec_pipe* p, int format) { return dec_set_handover(p, VIDEO, format, 0); }
extern "C" int ojphgpu_dec_pipe_set_video_colour(ojphgpu_dec_pipe* p, int format, const ojphgpu_colour_spec* spec)
{
  return spec ? dec_set_handover(p, VIDEO, format, 0, spec) : OJPHGPU_E_INVALID;
}

extern "C" int ojphgpu_dec_pipe_set_video_chroma(ojphgpu_dec_pipe* p, int format, int mode)
{
  return chroma_mode_ok(format, mode) ? dec_set_handover(p, VIDEO, format, 0, nullptr, OJPHGPU_CHROMA_COSITED) : OJPHGPU_E_INVALID;
}

// the judgement of the two _set_video_chroma setters on a plan alone, without a pipe or a device
extern "C" int ojphgpu_video_chroma_fit(const ojphgpu_plan* plan, int container_bits, int decoding, int format, int mode, ojphgpu_chroma_frame* frame,
                                        uint64_t* buffer_bytes)
{
  if (!plan || (container_bits != 8 && container_bits != 16 && container_bits != 32) || mode != OJPHGPU_CHROMA_COSITED) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    const Plan& P = plan->plan;
    Handover h;
    h.kind = VIDEO; h.format = format; h.chroma = mode;
    const int odd_origin = !P.has_region ? 0 : ((P.region[0] & 1u) ? ODD_X0 : 0) | ((P.region[1] & 1u) ? ODD_Y0 : 0);
    const int rc = handover_fit(P, container_bits, decoding != 0, odd_origin, h);
    if (rc) return rc;
    if (frame) *frame = h.cframe;
    if (buffer_bytes) *buffer_bytes = h.bytes;
    return OJPHGPU_OK;
  });
}

// the judgement of the two _set_video_colour setters on a plan alone, without a pipe or a device
extern "C" int ojphgpu_video_colour_fit(const ojphgpu_plan* plan, int container_bits, int decoding, int format, const ojphgpu_colour_spec* spec,
                                        ojphgpu_colour_table* table, ojphgpu_colour_frame* frame, uint64_t* frame_bytes)
{
  if (!plan || !spec || (container_bits != 8 && container_bits != 16 && container_bits != 32)) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    const Plan& P = plan->plan;
    Handover h;
    h.kind = VIDEO; h.format = format; h.colour = true; h.spec = *spec;
    const int odd_origin = !P.has_region ? 0 : ((P.region[0] & 1u) ? ODD_X0 : 0) | ((P.region[1] & 1u) ? ODD_Y0 : 0);
    const int rc = handover_fit(P, container_bits, decoding != 0, odd_origin, h);
    if (rc) return rc;
    if (table) *table = h.table;
    if (frame) *frame = h.frame;
    if (frame_bytes) *frame_bytes = h.bytes;
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_dec_pipe_plan(ojphgpu_dec_pipe* p, const ojphgpu_plan** plan)
{
  if (!p || !plan) return OJPHGPU_E_INVALID;
  *plan = p->first;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_dec_pipe_view_info(ojphgpu_dec_pipe* p, uint64_t out[5])
{
  if (!p || !out) return OJPHGPU_E_INVALID;
  std::lock_guard<std::mutex> lk(p->mu);
  if (!p->have_view_info) return OJPHGPU_E_INVALID;
  memcpy(out, p->last_view_info, sizeof(p->last_view_info));
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_dec_pipe_fused_retries(ojphgpu_dec_pipe* p, uint32_t* count)
{
  if (!p || !count) return OJPHGPU_E_INVALID;
  uint32_t n = 0;
  for (uint32_t k = 0; k < p->nobj; ++k) {
    std::lock_guard<std::mutex> lk(p->enqueue_mus[k]);
    n += p->decs[k]->fused_retries;
  }
  *count = n;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_dec_pipe_stats(ojphgpu_dec_pipe* p, double out[4])
{
  if (!p || !out) return OJPHGPU_E_INVALID;
  std::lock_guard<std::mutex> lk(p->mu);
  out[0] = (double)p->n_done;
  out[1] = p->n_done ? p->sum_parse / (double)p->n_done : 0.0;       // host parse + descriptor fill per frame, ms
  out[2] = p->n_done ? p->sum_latency / (double)p->n_done : 0.0;     // submit -> frame in pinned memory, ms
  out[3] = (double)p->workers.size();
  return OJPHGPU_OK;
}

// =============================================================================================
// transcode pipe
// =============================================================================================
// Host codestream in, host codestream out (section 5d's T, source after source).  A frame passes three stages, and the frames
// of a sequence overlap each other across them:
//   front     host threads: parse, the checks of a later source, the block descriptors into the slot's pinned memory, then
//             the uploads of the block bytes and the descriptors on the copy-in stream
//   device    ONE ordered thread, the owner of the compute stream (the encoder pipe's search worker, generalised): the block
//             decoder over the slot's bytes, the verdicts (and the repeat a one-launch run may ask for), then the blocks coded
//             into the slot's output set -- plainly, or by the budget's search with the spare set.  The transcoder has one
//             arena: frame n + 1's block decoder writes the planes frame n's coding reads, so the frames are strictly serial
//             here, in submit order; only the front and the finish of the neighbouring frames run beside them
//   finish    host threads: Tier-2's layout from the block lengths, the assembly in HBM and the download on the copy-out
//             stream (finish_coded_frame, the encoder pipe's)
struct TcSlot {
  SlotState state = FREE;
  Pinned h_src, h_descs, h_status, h_lay, h_cs;
  EncOut o;
  Grow data, cs;
  DeviceBuf cb_descs, status;
  hipEvent_t ev_in = nullptr, ev_kern = nullptr, ev_done = nullptr;
  size_t src_len = 0, cs_len = 0;
  int rc = 0; uint32_t failed = 0;
  bool front_done = false;                           // the front is through with the frame (s.rc says how): the device worker's turn
  bool any_refine = false; int kinds = 0; uint32_t max_len1 = 0;   // of the frame's descriptors (DecFrameInfo)
  double t_submit = 0, t_done = 0, t_parse = 0, t_t2 = 0;
  uint64_t budget = 0;
  ojphgpu_plan* rplan = nullptr;                     // a budget: the output plan at the step the frame's search chose
  ojphgpu_rate_info rate{}; bool have_rate = false;
};

struct ojphgpu_tc_pipe {
  ojphgpu_plan* first = nullptr;                     // parsed from the first source: the geometry of every source
  const ojphgpu_plan* out = nullptr;                 // the caller's output plan
  int device = 0, resilient = 0;
  int mode_in = copy_mode("OJPHGPU_DEC_COPY_MODE", 0), mode_out = copy_mode("OJPHGPU_ENC_COPY_MODE", 0);
  uint32_t depth = 0;
  ojphgpu_transcoder* t = nullptr;                   // one object: one arena, one compute stream
  hipStream_t s_h2d = nullptr, s_comp = nullptr, s_d2h = nullptr;
  std::vector<TcSlot> slots;
  size_t res_bytes = 0, st_bytes = 0;
  uint64_t n_acq = 0, n_sub = 0, n_col = 0;
  std::mutex mu; std::condition_variable cv_front, cv_dev, cv_fin, cv_done;
  std::deque<uint32_t> front_work, fin_work;
  bool stop_front = false, stop_dev = false, stop_fin = false;
  std::vector<std::thread> fronts, finishers;
  std::thread device_worker;
  double sum_parse = 0, sum_t2 = 0, sum_latency = 0; uint64_t n_done = 0;
  uint32_t fused_retries = 0;                        // (under mu) the decoder half's count after the frame the worker did last
  hipEvent_t ev_host = nullptr;                      // the device worker's: behind what it waits for (verdicts, histograms, trials)
  // byte budget (ojphgpu_tc_pipe_set_budget): the encoder pipe's rules
  bool budget_on = false, dead = false;
  uint64_t max_bytes = 0;
  EncOut spare;
  Pinned h_hist;
  int hint = -1;                                     // j* of the last frame that was certified
  ojphgpu_rate_info last{}; bool have_last = false;  // of the frame collected last
};

// the frame of a slot is over, whatever its outcome (s.rc): collectable, and counted
static void retire(ojphgpu_tc_pipe* p, TcSlot& s)
{
  {
    std::lock_guard<std::mutex> lk(p->mu);
    s.t_done = now_ms();
    s.state = DONE;
    p->sum_parse += s.t_parse; p->sum_t2 += s.t_t2; p->sum_latency += s.t_done - s.t_submit; p->n_done++;
  }
  p->cv_done.notify_all();
}

// ---- stage 1
static void tc_front_frame(ojphgpu_tc_pipe* p, TcSlot& s)
{
  auto fail = [&](int rc) { s.rc = rc; };
  if (hipSetDevice(p->device) != hipSuccess) return fail(OJPHGPU_E_HIP);
  const double t0 = now_ms();
  ojphgpu_plan* q = nullptr;
  int rc = ojphgpu_t2_parse(s.h_src.p, s.src_len, p->resilient, &q);
  if (rc) return fail(rc);
  struct Hold { ojphgpu_plan* q; ~Hold() { ojphgpu_plan_destroy(q); } } hold{ q };
  rc = no_throw([&]() -> int {
    const Plan& Q = q->plan;
    int r2 = ojphgpu_transcoder_check_source(p->t, Q);
    if (r2) return r2;
    const size_t nb = p->t->dec->block_ids.size();
    DecFrameInfo fi;
    if ((r2 = ojphgpu_transcoder_fill_descs(p->t, Q, s.src_len, (ojphgpu_cb_desc*)s.h_descs.p, fi)) != 0) return r2;
    s.t_parse = now_ms() - t0;
    if (s.data.reserve((size_t)fi.data_bytes() + (size_t)fi.len / 4 + 128)) return OJPHGPU_E_NOMEM;
    if ((r2 = upload(p->mode_in, p->s_h2d, s.data.b.p, s.h_src, (size_t)fi.first, (size_t)fi.len)) != 0) return r2;
    if ((r2 = ojphgpu_decoder_upload_pads(p->s_h2d, (uint8_t*)s.data.b.p, s.h_src.p, s.src_len, fi.pads)) != 0) return r2;   // (damaged codestreams only)
    if ((r2 = upload(p->mode_in, p->s_h2d, s.cb_descs.p, s.h_descs, 0, nb * sizeof(ojphgpu_cb_desc))) != 0) return r2;
    HIPCHK(hipEventRecord(s.ev_in, p->s_h2d));
    s.any_refine = fi.any_refine; s.kinds = fi.kinds; s.max_len1 = fi.max_len1;
    return OJPHGPU_OK;
  });
  if (rc) {                                          // (uploads of the slot may be enqueued: see enc_finish_frame)
    hipStreamSynchronize(p->s_h2d);
    fail(rc);
  }
}

static void tc_front(ojphgpu_tc_pipe* p)
{
  for (uint32_t si; pop_work(p->mu, p->cv_front, p->front_work, p->stop_front, si);) {
    tc_front_frame(p, p->slots[si]);
    { std::lock_guard<std::mutex> lk(p->mu); p->slots[si].front_done = true; }
    p->cv_dev.notify_all();
  }
}

// ---- stage 2
// the verdicts of the slot's run -- and, with a budget, the histograms taken behind it -- through the copy kernel into pinned memory
struct TcFetch { ojphgpu_tc_pipe* p; TcSlot* s; };
static int tc_fetch_status(void* user, const uint8_t** h_status)
{
  ojphgpu_tc_pipe* p = ((TcFetch*)user)->p; TcSlot& s = *((TcFetch*)user)->s;
  int rc = copy_to_host_launch(p->s_comp, s.h_status.d, s.status.p, p->st_bytes);
  if (rc) return rc;
  if (p->budget_on) {
    const EncoderRate& R = *p->t->enc->rate;
    if ((rc = copy_to_host_launch(p->s_comp, p->h_hist.d, R.hist.p, R.h_hist.size() * 4)) != 0) return rc;
  }
  HIPCHK(hipEventRecord(p->ev_host, p->s_comp));
  HIPCHK(hipEventSynchronize(p->ev_host));
  *h_status = s.h_status.p;
  return OJPHGPU_OK;
}

static int tc_device_frame(ojphgpu_tc_pipe* p, TcSlot& s)
{
  ojphgpu_transcoder* t = p->t;
  ojphgpu_decoder* d = t->dec; ojphgpu_encoder* e = t->enc;
  HIPCHK(hipSetDevice(p->device));
  HIPCHK(hipStreamWaitEvent(p->s_comp, s.ev_in, 0));
  d->o_cb_descs = s.cb_descs.p; d->o_data = s.data.b.p; d->o_status = s.status.p;
  int rc = ojphgpu_transcoder_decode(t, s.any_refine, s.kinds, s.max_len1);
  if (rc) return rc;
  const uint32_t repeats = d->fused_retries;
  TcFetch fetch{ p, &s };
  rc = ojphgpu_transcoder_verdicts(t, tc_fetch_status, &fetch, p->resilient != 0, &s.failed);   // no block is coded before the verdicts are in
  { std::lock_guard<std::mutex> lk(p->mu); p->fused_retries = d->fused_retries; }
  if (rc) return rc;
  const size_t nb = e->block_ids.size();
  if (!p->budget_on) {
    const RateTrialOut coded = s.o.trial(nb, nullptr);
    if ((rc = ojphgpu_transcoder_code(t, coded.out, coded.d_results, coded.d_counters)) != 0) return rc;
    if ((rc = publish_words_launch(p->s_comp, coded.d_publish, coded.d_counters, 2)) != 0) return rc;
  } else {
    if (d->fused_retries != repeats) {               // the statistics were taken again over the repeated planes: fetch them again
      const EncoderRate& R = *e->rate;
      if ((rc = copy_to_host_launch(p->s_comp, p->h_hist.d, R.hist.p, R.h_hist.size() * 4)) != 0) return rc;
      HIPCHK(hipEventRecord(p->ev_host, p->s_comp));
      HIPCHK(hipEventSynchronize(p->ev_host));
    }
    const RateFrame f{ e, &s.rplan->plan, s.budget, &s.o, &p->spare, p->ev_host };
    if ((rc = rate_search_frame(f, (const uint32_t*)p->h_hist.p, p->hint, s.rate, s.have_rate)) != 0) return rc;
  }
  HIPCHK(hipEventRecord(s.ev_kern, p->s_comp));
  return OJPHGPU_OK;
}

// frames in submit order, whichever front thread finished first: the hint of a frame is its predecessor's answer
static void tc_device_worker(ojphgpu_tc_pipe* p)
{
  for (uint64_t k = 0;; ++k) {
    const uint32_t si = (uint32_t)(k % p->depth);
    TcSlot& s = p->slots[si];
    {
      std::unique_lock<std::mutex> lk(p->mu);
      auto ready = [&] { return k < p->n_sub && s.front_done; };
      p->cv_dev.wait(lk, [&] { return p->stop_dev || ready(); });
      if (!ready()) return;
      s.front_done = false;
    }
    int rc = s.rc;                                   // (a frame the front refused: nothing of it reached the compute stream)
    if (!rc && (rc = no_throw([&] { return tc_device_frame(p, s); })) != 0) {
      // the frame ends here (OJPHGPU_E_BLOCK / _E_BUDGET among the reasons); see enc_finish_frame.  The arena keeps whatever
      // its block decoder wrote: the next frame's writes every block's rectangle again, zeros where nothing is coded
      hipStreamSynchronize(p->s_h2d); hipStreamSynchronize(p->s_comp);
      ojphgpu_decoder* d = p->t->dec;
      d->o_cb_descs = nullptr; d->o_data = nullptr; d->o_status = nullptr;
    }
    if (rc) {
      s.rc = rc;
      retire(p, s);
      continue;
    }
    { std::lock_guard<std::mutex> lk(p->mu); p->fin_work.push_back(si); }
    p->cv_fin.notify_one();
  }
}

// ---- stage 3
static void tc_finisher(ojphgpu_tc_pipe* p)
{
  for (uint32_t si; pop_work(p->mu, p->cv_fin, p->fin_work, p->stop_fin, si);) {
    TcSlot& s = p->slots[si];
    int rc = OJPHGPU_E_HIP;
    if (hipSetDevice(p->device) == hipSuccess && hipEventSynchronize(s.ev_kern) == hipSuccess) {
      const Plan& P = p->budget_on ? s.rplan->plan : p->out->plan;   // (a budget: the plan at the step the frame's search chose)
      rc = finish_coded_frame(CodedFrame{ P, p->t->enc->block_ids, s.o, s.h_lay, s.cs, s.h_cs, s.ev_done }, p->s_d2h, p->mode_out, s.cs_len, s.t_t2);
    }
    if (rc) {                                        // see enc_finish_frame
      hipStreamSynchronize(p->s_h2d); hipStreamSynchronize(p->s_comp); hipStreamSynchronize(p->s_d2h);
      s.rc = rc;
    }
    retire(p, s);
  }
}

extern "C" void ojphgpu_tc_pipe_destroy(ojphgpu_tc_pipe* p)
{
  if (!p) return;
  (void)hipSetDevice(p->device);
  // stage by stage: each hands its frames to the next
  { std::lock_guard<std::mutex> lk(p->mu); p->stop_front = true; }
  p->cv_front.notify_all();
  for (std::thread& th : p->fronts) th.join();
  if (p->device_worker.joinable()) {
    { std::lock_guard<std::mutex> lk(p->mu); p->stop_dev = true; }
    p->cv_dev.notify_all();
    p->device_worker.join();
  }
  { std::lock_guard<std::mutex> lk(p->mu); p->stop_fin = true; }
  p->cv_fin.notify_all();
  for (std::thread& th : p->finishers) th.join();
  for (hipStream_t s : { p->s_h2d, p->s_comp, p->s_d2h }) if (s) (void)hipStreamSynchronize(s);
  if (p->t) ojphgpu_transcoder_destroy(p->t);
  for (TcSlot& s : p->slots) {
    for (Pinned* b : { &s.h_src, &s.h_descs, &s.h_status, &s.h_lay, &s.h_cs }) b->release();
    s.o.release();
    for (DeviceBuf* b : { &s.data.b, &s.cs.b, &s.cb_descs, &s.status }) b->release();
    for (hipEvent_t ev : { s.ev_in, s.ev_kern, s.ev_done }) if (ev) (void)hipEventDestroy(ev);
    delete s.rplan;
  }
  p->spare.release(); p->h_hist.release();
  if (p->ev_host) (void)hipEventDestroy(p->ev_host);
  for (hipStream_t s : { p->s_h2d, p->s_comp, p->s_d2h }) if (s) (void)hipStreamDestroy(s);
  if (p->first) ojphgpu_plan_destroy(p->first);
  delete p;
}

extern "C" int ojphgpu_tc_pipe_create(const uint8_t* h_codestream, size_t len, int resilient, const ojphgpu_plan* out_plan, int device,
                                       uint32_t depth, uint32_t host_threads, ojphgpu_tc_pipe** out)
{
  if (!h_codestream || !len || !out_plan || !out || depth < 2 || depth > 16) return OJPHGPU_E_INVALID;
  *out = nullptr;
  return no_throw([&]() -> int {
    HIPCHK(hipSetDevice(device));
    ojphgpu_tc_pipe* p = new (std::nothrow) ojphgpu_tc_pipe();
    if (!p) return OJPHGPU_E_NOMEM;
    struct Owner { ojphgpu_tc_pipe* p; ~Owner() { if (p) ojphgpu_tc_pipe_destroy(p); } } owner{ p };
    int rc = ojphgpu_t2_parse(h_codestream, len, resilient, &p->first);
    if (rc) return rc;
    p->out = out_plan; p->device = device; p->depth = depth; p->resilient = resilient;
    for (hipStream_t* s : { &p->s_h2d, &p->s_comp }) HIPCHK(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    HIPCHK(create_copy_out_stream(&p->s_d2h));
    if ((rc = ojphgpu_transcoder_create(p->first, out_plan, device, p->s_comp, &p->t)) != 0) return rc;   // (the refusals)
    ojphgpu_decoder* d = p->t->dec; ojphgpu_encoder* e = p->t->enc;
    (void)ojphgpu_decoder_set_timing(d, 0); (void)ojphgpu_encoder_set_timing(e, 0);
    const size_t nbs = d->block_ids.size(), nbo = e->block_ids.size();
    p->res_bytes = nbo * sizeof(ojphgpu_cb_result) + 16;
    p->st_bytes = ((nbs + 3) & ~(size_t)3) + 4;        // the status bytes + the RETRY word behind them
    HIPCHK(hipEventCreateWithFlags(&p->ev_host, hipEventDisableTiming | hipEventReleaseToSystem));
    const size_t cs_guess = std::min<size_t>((size_t)e->out_cap, len + len / 4 + (1u << 20));
    p->slots.resize(depth);
    for (TcSlot& s : p->slots) {
      if (s.h_src.reserve(len + len / 4 + (1u << 16)) || s.h_descs.reserve(nbs * sizeof(ojphgpu_cb_desc) + 64) || s.h_status.reserve(nbs + 64) ||
          s.o.h_res.reserve(p->res_bytes + 64) || s.h_cs.reserve(cs_guess) || s.h_lay.reserve(nbo * sizeof(T2Job) + nbo * 8 + (1u << 16))) return OJPHGPU_E_NOMEM;
      if (s.data.reserve(len + len / 4 + 64) || s.cb_descs.alloc(nbs * sizeof(ojphgpu_cb_desc) + 64) || s.status.alloc(nbs + 64) ||
          s.o.out.alloc((size_t)e->out_cap + 64) || s.o.counters.alloc(e->counters_bytes) || s.cs.reserve(cs_guess)) return OJPHGPU_E_NOMEM;
      HIPCHK(hipMemset(s.status.p, 0, nbs + 64));
      for (hipEvent_t* ev : { &s.ev_in, &s.ev_kern, &s.ev_done }) HIPCHK(hipEventCreateWithFlags(ev, hipEventDisableTiming | hipEventReleaseToSystem));
    }
    const uint32_t nthreads = host_threads ? std::min<uint32_t>(host_threads, 16) : 2;
    for (uint32_t i = 0; i < nthreads; ++i) p->fronts.emplace_back(tc_front, p);
    p->device_worker = std::thread(tc_device_worker, p);
    for (uint32_t i = 0; i < nthreads; ++i) p->finishers.emplace_back(tc_finisher, p);
    owner.p = nullptr;
    *out = p;
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_tc_pipe_acquire(ojphgpu_tc_pipe* p, size_t len, uint8_t** h_codestream)
{
  if (!p || !h_codestream || len == 0 || p->dead) return OJPHGPU_E_INVALID;
  const Plan& O = p->out->plan;
  if (!p->budget_on && !plan_all_reversible(O) && !(O.p.qstep > 0.0f)) return OJPHGPU_E_INVALID;   // no step and no budget
  TcSlot& s = p->slots[p->n_acq % p->depth];
  {
    std::lock_guard<std::mutex> lk(p->mu);
    if (s.state != FREE && s.state != ACQUIRED) return OJPHGPU_E_AGAIN;     // every slot is in flight: collect a codestream first
    s.state = ACQUIRED;
  }
  if (hipSetDevice(p->device) != hipSuccess) return OJPHGPU_E_HIP;
  if (s.h_src.reserve(len + len / 4 + 64)) { std::lock_guard<std::mutex> lk(p->mu); s.state = FREE; return OJPHGPU_E_NOMEM; }
  s.src_len = len;
  *h_codestream = s.h_src.p;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_tc_pipe_submit(ojphgpu_tc_pipe* p)
{
  if (!p || p->dead) return OJPHGPU_E_INVALID;
  const uint32_t si = (uint32_t)(p->n_acq % p->depth);
  TcSlot& s = p->slots[si];
  {
    std::lock_guard<std::mutex> lk(p->mu);
    if (s.state != ACQUIRED) return OJPHGPU_E_INVALID;
    s.rc = 0; s.failed = 0; s.cs_len = 0; s.t_parse = s.t_t2 = 0; s.t_submit = now_ms();
    s.budget = p->max_bytes; s.have_rate = false; s.rate = ojphgpu_rate_info{};
    s.front_done = false;
    s.state = SUBMITTED;
    p->front_work.push_back(si);
    p->n_acq++; p->n_sub++;
  }
  p->cv_front.notify_one();
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_tc_pipe_collect(ojphgpu_tc_pipe* p, const uint8_t** h_out, size_t* len, uint32_t* failed_blocks)
{
  if (!p || !h_out || !len) return OJPHGPU_E_INVALID;
  std::unique_lock<std::mutex> lk(p->mu);
  if (p->n_col >= p->n_sub) return OJPHGPU_E_INVALID;            // nothing in flight
  if (p->n_col > 0) {                                              // the codestream handed out last time is released now
    TcSlot& prev = p->slots[(p->n_col - 1) % p->depth];
    if (prev.state == HELD) prev.state = FREE;
  }
  TcSlot& s = p->slots[p->n_col % p->depth];
  p->cv_done.wait(lk, [&] { return s.state == DONE; });
  p->n_col++;
  p->last = s.rate; p->have_last = s.have_rate;
  if (failed_blocks) *failed_blocks = s.failed;
  if (s.rc) { s.state = FREE; return s.rc; }
  s.state = HELD;
  *h_out = s.h_cs.p; *len = s.cs_len;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_tc_pipe_set_budget(ojphgpu_tc_pipe* p, uint64_t max_bytes)
{
  if (!p || p->dead) return OJPHGPU_E_INVALID;
  if (p->n_acq != 0 || p->slots[0].state != FREE) {  // sources have been handed in: the mode stays, the budget may move
    if (!p->budget_on || max_bytes == 0) return OJPHGPU_E_INVALID;
    p->max_bytes = max_bytes;
    return OJPHGPU_OK;
  }
  if (max_bytes == 0) return p->budget_on ? OJPHGPU_E_INVALID : OJPHGPU_OK;   // (once on, the buffers are there)
  if (p->budget_on) { p->max_bytes = max_bytes; return OJPHGPU_OK; }
  return no_throw([&]() -> int {
    HIPCHK(hipSetDevice(p->device));
    ojphgpu_encoder* e = p->t->enc;
    const int rc = ojphgpu_transcoder_set_budget(p->t, max_bytes);   // the refusals, the statistics, scratch and output bound of the finest step
    if (rc) return rc;
    // from here the encoder half runs in that mode and the buffers change hands (enc_search_on): every slot's output set at
    // the bound of the finest step and its copy of the plan, the spare set -- the encoder half's own -- and the histograms
    p->dead = true;
    for (TcSlot& s : p->slots) {
      s.o.out.release(); s.o.counters.release();
      if (s.o.out.alloc((size_t)e->out_cap + 64) || s.o.counters.alloc(e->counters_bytes)) return OJPHGPU_E_NOMEM;
      if (!s.rplan) s.rplan = new ojphgpu_plan{ p->out->plan };
    }
    if (p->spare.h_res.reserve(p->res_bytes + 64)) return OJPHGPU_E_NOMEM;
    p->spare.out = e->out; p->spare.counters = e->counters;
    e->out = DeviceBuf(); e->counters = DeviceBuf();
    if (p->h_hist.reserve(e->rate->h_hist.size() * 4 + 64)) return OJPHGPU_E_NOMEM;
    p->hint = -1;
    p->budget_on = true; p->max_bytes = max_bytes; p->dead = false;
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_tc_pipe_rate_info(ojphgpu_tc_pipe* p, ojphgpu_rate_info* info)
{
  if (!p || !info) return OJPHGPU_E_INVALID;
  std::lock_guard<std::mutex> lk(p->mu);
  if (!p->have_last) return OJPHGPU_E_INVALID;
  *info = p->last;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_tc_pipe_fused_retries(ojphgpu_tc_pipe* p, uint32_t* count)
{
  if (!p || !count) return OJPHGPU_E_INVALID;
  std::lock_guard<std::mutex> lk(p->mu);
  *count = p->fused_retries;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_tc_pipe_stats(ojphgpu_tc_pipe* p, double out[4])
{
  if (!p || !out) return OJPHGPU_E_INVALID;
  std::lock_guard<std::mutex> lk(p->mu);
  out[0] = (double)p->n_done;
  out[1] = p->n_done ? p->sum_parse / (double)p->n_done : 0.0;       // host parse + descriptor fill per frame, ms
  out[2] = p->n_done ? p->sum_t2 / (double)p->n_done : 0.0;          // host Tier-2 (layout) per frame, ms
  out[3] = p->n_done ? p->sum_latency / (double)p->n_done : 0.0;     // submit -> codestream in pinned memory, ms
  return OJPHGPU_OK;
}
