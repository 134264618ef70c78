// openjph_amd/csrc/ojphgpu_codec.cpp -- whole-frame encoder / decoder objects of the C ABI.
//
// These are what an ojph::codestream-compatible facade calls where the reference runs its
// per-line object tree: ojphgpu_encoder_* replaces tile::push -> resolution::push_line ->
// subband::push_line -> codeblock::push/encode (ojph_tile.cpp:332, ojph_resolution.cpp:547,
// ojph_subband.cpp:292, ojph_codeblock.cpp:115-175) followed by codestream::flush
// (ojph_codestream_local.cpp:1148); ojphgpu_decoder_* replaces codestream::read
// (ojph_codestream_local.cpp:912) and the pull chain tile::pull -> resolution::pull_line ->
// subband::pull_line -> codeblock::decode/pull_line (ojph_tile.cpp:425, ojph_resolution.cpp:713,
// ojph_subband.cpp:336, ojph_codeblock.cpp:190-266).
//
// Layout in HBM (one arena of 32-bit elements per codec object, planned once per frame shape):
//   [ tile-component planes per resolution | sub-band planes ]   see ojph_plan.cpp (alloc)
// plus descriptor tables, the per-block scratch slots and the compacted code-block bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "ht_tables.h"
#include "ojph_plan.h"
#include "ojph_pool.h"

using namespace ojphgpu;

namespace ojphgpu {

int ensure_tables()
{
  static std::mutex mu;
  static bool done[64] = { false };
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return -1;
  std::lock_guard<std::mutex> lock(mu);
  if (done[dev]) return 0;
  static HtTables tables;
  static bool built = false;
  if (!built) { build_ht_tables(tables); built = true; }
  if (upload_enc_tables(tables) != 0 || upload_dec_tables(tables) != 0) return -1;
  done[dev] = true;
  return 0;
}

}  // namespace ojphgpu

#include "ojphgpu_objects.h"

extern "C" void ojphgpu_encoder_destroy(ojphgpu_encoder* e)
{
  if (!e) return;
  (void)hipSetDevice(e->device);
  // a released run may still be coding on the object's own streams: nothing is freed under it
  if (e->side) (void)hipStreamSynchronize(e->side);
  if (e->low) (void)hipStreamSynchronize(e->low);
  e->pending = e->other.pending = false;
  for (DeviceBuf* b : { &e->arena, &e->image, &e->dwt_descs, &e->img_descs, &e->cb_descs, &e->conv_descs, &e->scratch, &e->out,
                        &e->results, &e->counters, &e->regions, &e->other.arena, &e->other.out, &e->other.results,
                        &e->other.counters }) b->release();
  e->h_out.release(); e->h_res.release();
  if (e->side) (void)hipStreamDestroy(e->side);
  if (e->low) (void)hipStreamDestroy(e->low);
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->ev_join) (void)hipEventDestroy(e->ev_join);
  if (e->ev_low) (void)hipEventDestroy(e->ev_low);
  if (e->other.ev_join) (void)hipEventDestroy(e->other.ev_join);
  if (e->other.ev_low) (void)hipEventDestroy(e->other.ev_low);
  if (e->ev_clear) (void)hipEventDestroy(e->ev_clear);
  e->timer.destroy();
  delete e->quality;
  delete e->rate;
  delete e->trunc;
  delete e;
}

extern "C" int ojphgpu_encoder_create(const ojphgpu_plan* plan, int device, void* stream, ojphgpu_encoder** out)
{
  if (!plan) return OJPHGPU_E_INVALID;
  return ojphgpu_encoder_create_tiles(plan, device, stream, 0, (uint32_t)plan->plan.tiles.size(), out);
}

// blocks_only: the encoder half of a transcoder (section 5d) -- the block coder alone: no conversion or DWT descriptors and no
// arena of its own (its owner lends it one)
static int encoder_create(const ojphgpu_plan* plan, int device, void* stream, uint32_t tile_first, uint32_t tile_count,
                          uint32_t nframes, ojphgpu_encoder** out, bool blocks_only = false, bool joined_only = false);

extern "C" int ojphgpu_encoder_create_tiles(const ojphgpu_plan* plan, int device, void* stream, uint32_t tile_first,
                                             uint32_t tile_count, ojphgpu_encoder** out)
{
  return no_throw([&] { return encoder_create(plan, device, stream, tile_first, tile_count, 1, out); });
}

// the encoder of a frame pipe: every run writes into a slot and ends joined, so it gets no second stream (ojphgpu_objects.h)
int ojphgpu_encoder_create_joined(const ojphgpu_plan* plan, int device, void* stream, ojphgpu_encoder** out)
{
  if (!plan) return OJPHGPU_E_INVALID;
  return no_throw([&] { return encoder_create(plan, device, stream, 0, (uint32_t)plan->plan.tiles.size(), 1, out, false, true); });
}

extern "C" int ojphgpu_encoder_create_batch(const ojphgpu_plan* plan, int device, void* stream, uint32_t num_frames,
                                             ojphgpu_encoder** out)
{
  if (!plan) return OJPHGPU_E_INVALID;
  return no_throw([&] { return encoder_create(plan, device, stream, 0, (uint32_t)plan->plan.tiles.size(), num_frames, out); });
}

// The block descriptors of the encoder's blocks with their scratch slots, and the compacted output with its regions (e->
// out_cap, nreg, h_regions, counters_bytes).  band_kmax: per band of the plan, the K_max the slots and the output are sized
// for where it exceeds the plan's own (an encoder with a byte budget: the finest step its search may visit); null = the plan's.
// Which block encoder kernels the two launches of a cut at n_top need (ht_encode_launch's `widths`)
// percent of the top resolution's blocks on the side stream in a released run where OJPHGPU_ENC_TOP_SHARE_RELEASED is unset;
// 0 = the joined cut
#ifndef OJPHGPU_ENC_TOP_SHARE_RELEASED_DEFAULT
#define OJPHGPU_ENC_TOP_SHARE_RELEASED_DEFAULT 10
#endif
#ifndef OJPHGPU_ENC_TOP_SHARE_RELEASED_LARGE
#define OJPHGPU_ENC_TOP_SHARE_RELEASED_LARGE 8192    // blocks in the top resolution above which the default above holds (two rounds of
#endif                                               // the 4 096 wavefront slots the narrow block encoder has on 256 CUs); up to it:
#ifndef OJPHGPU_ENC_TOP_SHARE_RELEASED_SMALL
#define OJPHGPU_ENC_TOP_SHARE_RELEASED_SMALL 50
#endif
static ojphgpu_encoder::EncoderCut encoder_cut(const ojphgpu_encoder* e, uint32_t n_top)
{
  const Plan& P = *e->P;
  ojphgpu_encoder::EncoderCut c; c.n_top = n_top;
  int top = 0, rest = 0;                                   // the blocks' own statements, OR-ed (ht_encode_block_widths, ht_tables.h)
  for (size_t i = 0; i < e->block_ids.size(); ++i) {
    const Block& k = P.blocks[e->block_ids[i]]; const Band& B = P.bands[k.band];
    // (the descriptor's `reversible` as encoder_block_layout writes it)
    (i < n_top ? top : rest) |= ojphgpu::ht_encode_block_widths(k.r.w, (P.style(B.comp).rev ? 1u : 0u) | (is_wide(P, B.comp) ? 4u : 0u));
  }
  // bit 4: every block of the range at most 32 samples wide (e.g. the IMF profile's 32 x 32); bit 6: none wider than 128
  // samples (128 x 32 blocks take the narrow kernel, too)
  c.widths_top = ojphgpu::ht_encode_range_widths(top);
  c.widths_rest = ojphgpu::ht_encode_range_widths(rest);
  return c;
}

static void encoder_block_layout(ojphgpu_encoder* e, const uint32_t* band_kmax, std::vector<ojphgpu_cb_desc>& bd, uint64_t& scratch_total,
                                 bool* clamped = nullptr)
{
  if (clamped) *clamped = false;
  const Plan& P = *e->P;
  const uint32_t nframes = e->nframes;
  bd.assign(e->block_ids.size(), ojphgpu_cb_desc());
  uint64_t scratch_bytes = 0, samples = 0;
  for (size_t i = 0; i < bd.size(); ++i) {
    const Block& k = P.blocks[e->block_ids[i]]; const Band& B = P.bands[k.band];
    samples += (uint64_t)k.r.w * k.r.h;
    ojphgpu_cb_desc& d = bd[i]; memset(&d, 0, sizeof(d));
    const bool wide = is_wide(P, B.comp);                  // 64-bit samples: two arena elements each
    d.coef_off = B.plane_off + ((uint64_t)k.r.y0 * B.pitch + k.r.x0) * (wide ? 2u : 1u); d.pitch = B.pitch;
    d.w = (uint16_t)k.r.w; d.h = (uint16_t)k.r.h; d.K_max = (uint8_t)B.K_max; d.reversible = (uint8_t)((P.style(B.comp).rev ? 1 : 0) | (wide ? 4 : 0));
    d.missing_msbs = (uint8_t)(B.K_max - 1); d.num_passes = 1; d.delta = B.delta;
    d.data_off = scratch_bytes; d.scratch_cap = block_scratch_bytes(k.r.w, k.r.h, band_kmax ? std::max(B.K_max, band_kmax[k.band]) : B.K_max);
    scratch_bytes += d.scratch_cap;
  }
  if (nframes > 1) {                                      // replicate the block descriptors, frame-major
    const size_t nb = bd.size();
    bd.resize(nb * nframes);
    for (uint32_t f = 1; f < nframes; ++f)
      for (size_t i = 0; i < nb; ++i) {
        ojphgpu_cb_desc d = bd[i];
        d.coef_off += (uint64_t)f * P.arena_elems; d.data_off += (uint64_t)f * scratch_bytes;
        bd[f * nb + i] = d;
      }
    scratch_bytes *= nframes; samples *= nframes;
  }
  // The compacted output: scratch_bytes is a true upper bound of what the blocks can produce (K_max + 2 bits per
  // sample plus stuffing); samples * 3 bytes covers every bit depth up to 20 on any content and keeps the buffer of
  // the usual frames small -- deeper samples get the true bound, so that incompressible content cannot overflow.
  // The byte cursor is 32 bits wide: a batch whose bound exceeds 4 GiB is clamped there and a frame batch that
  // really produces more reports OJPHGPU_E_OVERFLOW (code fewer frames per batch).
  uint32_t kmax_all = 0;
  for (size_t b = 0; b < P.bands.size(); ++b) kmax_all = std::max(kmax_all, band_kmax ? std::max(P.bands[b].K_max, band_kmax[b]) : P.bands[b].K_max);
  uint64_t cap = kmax_all > 20 ? scratch_bytes : std::min<uint64_t>(scratch_bytes, samples * 3 + (1u << 20));
  if (clamped && cap > 0xFFFFFF00ull) *clamped = true;
  cap = std::min<uint64_t>(cap, 0xFFFFFF00ull);
  // ... split into regions (see ojphgpu_objects.h): a region holds the sum of its own blocks' shares of that bound
  {
    const char* ev = getenv("OJPHGPU_ENC_REGIONS"); const long v = ev ? atol(ev) : 16;
    uint32_t R = (v >= 0 && v <= 64 && (v & (v - 1)) == 0) ? (uint32_t)v : 16u;
    if (bd.size() < 4 * (size_t)R) R = 0;                   // a handful of blocks: one cursor
    std::vector<uint64_t> rc(R ? R : 1, 0);
    if (R) for (size_t i = 0; i < bd.size(); ++i) {
      const uint64_t own = kmax_all > 20 ? bd[i].scratch_cap : std::min<uint64_t>(bd[i].scratch_cap, (uint64_t)bd[i].w * bd[i].h * 3 + 64);
      rc[i & (R - 1)] += own;                                // (the kernels: the launch's first index + the index inside the launch)
    }
    uint64_t total = 0;
    e->h_regions.assign(2 * (size_t)R, 0);
    for (uint32_t r = 0; r < R; ++r) {
      const uint64_t c = (rc[r] + (1u << 16) + 255) & ~(uint64_t)255;
      if (total + c > 0xFFFFFF00ull) {                       // the byte offsets are 32 bits wide: one clamped cursor, as before
        if (clamped) *clamped = true;
        R = 0; break;
      }
      e->h_regions[2 * r] = (uint32_t)total; e->h_regions[2 * r + 1] = (uint32_t)c;
      total += c;
    }
    e->nreg = R;
    if (R) cap = total; else e->h_regions.clear();
    e->counters_bytes = R ? (size_t)R * 128 : 16;
  }
  e->out_cap = (uint32_t)cap;
  scratch_total = scratch_bytes;
}

static int encoder_create(const ojphgpu_plan* plan, int device, void* stream, uint32_t tile_first, uint32_t tile_count,
                          uint32_t nframes, ojphgpu_encoder** out, bool blocks_only, bool joined_only)
{
  if (!plan || !out || nframes == 0) return OJPHGPU_E_INVALID;
  *out = nullptr;
  if ((uint64_t)tile_first + tile_count > plan->plan.tiles.size()) return OJPHGPU_E_INVALID;
  if (plan->plan.skip_read || plan->plan.skip_recon) return OJPHGPU_E_INVALID;     // a decoding-only restriction
  HIPCHK(hipSetDevice(device));
  if (ensure_tables() != 0) return OJPHGPU_E_HIP;
  ojphgpu_encoder* e = new (std::nothrow) ojphgpu_encoder();
  if (!e) return OJPHGPU_E_NOMEM;
  struct Owner { ojphgpu_encoder* p; ~Owner() { if (p) ojphgpu_encoder_destroy(p); } } owner{ e };   // also when a container throws
  const Plan& P = plan->plan;
  e->handle = plan; e->P = &P; e->device = device; e->stream = (hipStream_t)stream;
  auto bail = [&](int rc) { return rc; };

  e->tiles = TileRange{ tile_first, tile_count };
  e->nframes = nframes;
  const TileRange tr = e->tiles;
  const uint64_t frame_elems = P.frame_elems;
  std::vector<ojphgpu_dwt_desc> dd, idd;
  std::vector<ojphgpu_convert_desc> cd;
  if (!blocks_only) {
    build_level_batches(P, tr, dd, e->batches);
    build_image_level_descs(P, tr, dd, e->batches, idd);
    replicate_levels(dd, idd, e->batches, nframes, P.arena_elems, frame_elems);
    e->need_convert = build_convert_descs(P, tr, cd, e->conv_max_w, e->conv_max_h);
    replicate_converts(cd, nframes, P.arena_elems, P.frame_elems);
  }
  e->block_ids = blocks_of_tiles(P, tr);
  uint32_t n_top_released = 0;
  if (nframes == 1 && max_recon_decomps(P) >= 2 && getenv("OJPHGPU_NO_OVERLAP") == nullptr) {
    auto top = [&](uint32_t id) { const Band& B = P.bands[P.blocks[id].band]; return B.res == P.style(B.comp).L; };
    auto mid = std::stable_partition(e->block_ids.begin(), e->block_ids.end(), top);
    e->n_top = (uint32_t)(mid - e->block_ids.begin());
    {
      // How many of the top resolution's blocks the side stream's launch takes; the rest join the main stream's launch behind
      // the lower levels.  The main stream waits for the side stream at the end of the encode, and a wait on another queue
      // that is not yet satisfied when it is reached costs ~20 us on top of what is waited for (kernel trace of a step:
      // the next launch started 22 us after the side stream's had ended) -- so the branches are cut for the SIDE one to
      // end first, by a model of what each costs on this device (MI355X, profiles/r06_*): the block coder 3.8 us per
      // million samples of the top resolution and 1.6 x that below it (more bytes per sample, shorter launches), a lower
      // analysis level its bytes at 3 TB/s or a 12 us launch floor.  8K 4:4:4: 90 % (step 0.957 -> 0.938 ms); a 4K frame's
      // main branch is the longer one already: 100 %.  OJPHGPU_ENC_TOP_SHARE=<percent> overrides the model.
      // That is the joined schedule's cut.  A released run (ojphgpu_objects.h), whose branches nobody waits for, has a cut
      // of its own: OJPHGPU_ENC_TOP_SHARE_RELEASED=<percent>, read at every creation; unset: 10 % -- blocks moved to the
      // second stream's launch are coded beside the synthesis levels (HBM-bound) instead of beside the fused block decoder
      // (issue-bound like the coder).  With the decoder's fused launch on the caller's stream the 8K step was 0.843 ms at 50
      // against 0.854 / 0.849 at 40 / 60 and 0.869 at 90 (profiles/enc_sets_ab.txt); since that launch runs on a stream of
      // its own the optimum is at the other end: 0.7952 at 10, 0.7994 at 20, 0.8051 at 30, 0.8159 at 50, five alternating
      // rounds, every round in this order (profiles/enc_block_runs_ab.txt).  The run picks the pair (run_container); the
      // blocks' output regions do not depend on it (encoder_block_layout).
      static const int share_env = [] { const char* v = getenv("OJPHGPU_ENC_TOP_SHARE"); const int x = v ? atoi(v) : 0; return x < 10 ? 0 : x > 100 ? 100 : x; }();
      double s_top = 0, s_low = 0;                         // millions of samples
      for (size_t i = 0; i < e->block_ids.size(); ++i) {
        const Block& k = P.blocks[e->block_ids[i]];
        (i < e->n_top ? s_top : s_low) += (double)k.r.w * k.r.h * 1e-6;
      }
      double dwt_us = 0, level_bytes = 8.0 * (s_top + s_low) * 1e6 / 4.0;
      for (uint32_t l = 2; l <= max_recon_decomps(P); ++l, level_bytes /= 4.0) dwt_us += std::max(12.0, level_bytes / 3.0e6);
      const double us_per_ms = 3.8, margin_us = 30.0;
      const double move = (s_top + margin_us / us_per_ms - 1.6 * s_low - dwt_us / us_per_ms) / 2.0;   // top samples the main branch should take
      int share = share_env;
      if (!share) { share = s_top > 0 && move > 0 ? (int)(100.0 * (1.0 - move / s_top)) : 100; share = share < 50 ? 50 : share > 100 ? 100 : share; }
      const uint32_t n_res_top = e->n_top;
      e->n_top = (uint32_t)((uint64_t)n_res_top * (uint32_t)share / 100u);
      const char* rv = getenv("OJPHGPU_ENC_TOP_SHARE_RELEASED");
      // (unset: 10 where the top resolution has more blocks than OJPHGPU_ENC_TOP_SHARE_RELEASED_LARGE -- the 8K frame's
      // 18 360; 50, as before, below that: a 4K frame's 4 590 blocks are one round of the chip's coder slots, and its step
      // is 1.6 % LONGER at 10, 0.3026 against 0.2977 ms in five alternating pairs.  Not swept between the two sizes.)
      const int rshare = rv ? std::min(100, std::max(10, atoi(rv)))
                            : n_res_top > (uint32_t)OJPHGPU_ENC_TOP_SHARE_RELEASED_LARGE ? OJPHGPU_ENC_TOP_SHARE_RELEASED_DEFAULT : OJPHGPU_ENC_TOP_SHARE_RELEASED_SMALL;
      n_top_released = rshare ? (uint32_t)((uint64_t)n_res_top * (uint32_t)rshare / 100u) : e->n_top;
      if (n_top_released == 0 || n_top_released == e->block_ids.size()) n_top_released = e->n_top;
    }
    if (e->n_top == 0 || e->n_top == e->block_ids.size()) e->n_top = 0;
    else {
      // the side stream carries the long launch of the pair (the top resolution's blocks); the main stream's branch -- four
      // small transform launches, then the other blocks -- is the one that ends last when both share the chip evenly:
      // OJPHGPU_ENC_SIDE_PRIO=low lets the dispatcher prefer the main branch (high: the opposite; normal: equal; unset: below)
      int prio_lo = 0, prio_hi = 0;
      (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
      const char* pe = getenv("OJPHGPU_ENC_SIDE_PRIO");
      const int prio = pe && pe[0] == 'l' ? prio_lo : pe && pe[0] == 'h' ? prio_hi : (prio_lo + prio_hi) / 2;
      // Released runs (ojphgpu_objects.h) need a second stream -- the lower levels and their blocks -- and both own
      // streams at the LOWEST priority: what runs beside them is the caller's next job, whose result the caller waits
      // for, while theirs is not needed before the object's next run -- at equal priority the three launches that start
      // behind level 1 share the chip evenly and a decode enqueued behind the encode takes as long as the time it saves
      // (8K step 0.953 ms at equal priority, 0.931 with both low, 0.956 joined; profiles/enc_release_ab.txt).
      // OJPHGPU_ENC_SIDE_PRIO overrides the priority of both.  An encoder whose runs always end joined -- a transcoder's
      // block coder, a frame pipe's encoder (joined_only), OJPHGPU_ENC_RELEASE=0 -- keeps the one side stream at the
      // caller's priority.  Both streams are made HERE, next to each other: made by the first released run instead
      // (behind a decoder's streams) they measured 1.32 ms per 8K step against 0.93 (supposed, not shown: streams
      // are dealt onto the runtime's four hardware queues in the order they are created, and the late ones share one).
      const char* rel = getenv("OJPHGPU_ENC_RELEASE");
      e->can_release = !blocks_only && !joined_only && !(rel && rel[0] == '0');
      const int own_prio = pe ? prio : e->can_release ? prio_lo : 0;
      if (hipStreamCreateWithPriority(&e->side, hipStreamNonBlocking, own_prio) != hipSuccess ||
          hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess) return bail(OJPHGPU_E_HIP);
      if (e->can_release &&
          (hipStreamCreateWithPriority(&e->low, hipStreamNonBlocking, own_prio) != hipSuccess ||
           hipEventCreateWithFlags(&e->ev_low, hipEventDisableTiming) != hipSuccess)) return bail(OJPHGPU_E_HIP);
      // A second product set for the object that can release (ojphgpu_objects.h) unless OJPHGPU_ENC_SETS=1 (for an A/B, and
      // for a caller short of memory: the set is one more arena, output buffer and results table), and the event behind
      // the counter clear on the side stream unless OJPHGPU_ENC_SIDE_CLEAR=0.  Both read at every creation.
      const char* sets = getenv("OJPHGPU_ENC_SETS"); const char* sc = getenv("OJPHGPU_ENC_SIDE_CLEAR");
      e->two_sets = e->can_release && !(sets && atoi(sets) == 1);
      e->clear_on_side = e->can_release && !(sc && sc[0] == '0');
      if (e->two_sets &&
          (hipEventCreateWithFlags(&e->other.ev_join, hipEventDisableTiming) != hipSuccess ||
           hipEventCreateWithFlags(&e->other.ev_low, hipEventDisableTiming) != hipSuccess)) return bail(OJPHGPU_E_HIP);
      if (e->clear_on_side && hipEventCreateWithFlags(&e->ev_clear, hipEventDisableTiming) != hipSuccess) return bail(OJPHGPU_E_HIP);
    }
  }
  e->cut_joined = encoder_cut(e, e->n_top);
  e->cut_released = e->can_release ? encoder_cut(e, n_top_released) : e->cut_joined;
  e->take_cut(e->cut_joined);
  std::vector<ojphgpu_cb_desc> bd;
  uint64_t scratch_bytes = 0;
  encoder_block_layout(e, nullptr, bd, scratch_bytes);
  const uint64_t cap = e->out_cap;

  if ((!blocks_only && (e->arena.alloc(P.arena_elems * 4 * nframes) || e->dwt_descs.alloc(dd.size() * sizeof(dd[0])) ||
                        e->img_descs.alloc(idd.size() * sizeof(dd[0])) || e->conv_descs.alloc(cd.size() * sizeof(cd[0])))) ||
      e->cb_descs.alloc(bd.size() * sizeof(bd[0])) ||
      e->scratch.alloc(scratch_bytes) || e->out.alloc(cap) ||
      e->results.alloc(bd.size() * sizeof(ojphgpu_cb_result)) || e->counters.alloc(e->counters_bytes) ||
      (e->nreg && e->regions.alloc(e->h_regions.size() * 4)))
    return bail(OJPHGPU_E_NOMEM);
  if (e->two_sets) {                                        // the second set, exactly as the first
    if (e->other.arena.alloc(P.arena_elems * 4) || e->other.out.alloc(cap) ||
        e->other.results.alloc(bd.size() * sizeof(ojphgpu_cb_result)) || e->other.counters.alloc(e->counters_bytes))
      return bail(OJPHGPU_E_NOMEM);
    if (hipMemset(e->other.arena.p, 0, P.arena_elems * 4) != hipSuccess) return bail(OJPHGPU_E_HIP);
  }
  if (e->nreg && hipMemcpy(e->regions.p, e->h_regions.data(), e->h_regions.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return bail(OJPHGPU_E_HIP);
  if (!blocks_only && hipMemset(e->arena.p, 0, P.arena_elems * 4 * nframes) != hipSuccess) return bail(OJPHGPU_E_HIP);
  if (!dd.empty() && hipMemcpy(e->dwt_descs.p, dd.data(), dd.size() * sizeof(dd[0]), hipMemcpyHostToDevice) != hipSuccess) return bail(OJPHGPU_E_HIP);
  if (!idd.empty() && hipMemcpy(e->img_descs.p, idd.data(), idd.size() * sizeof(idd[0]), hipMemcpyHostToDevice) != hipSuccess) return bail(OJPHGPU_E_HIP);
  if (!bd.empty() && hipMemcpy(e->cb_descs.p, bd.data(), bd.size() * sizeof(bd[0]), hipMemcpyHostToDevice) != hipSuccess) return bail(OJPHGPU_E_HIP);
  if (!cd.empty() && hipMemcpy(e->conv_descs.p, cd.data(), cd.size() * sizeof(cd[0]), hipMemcpyHostToDevice) != hipSuccess) return bail(OJPHGPU_E_HIP);
  e->h_results.resize(bd.size());
  if (e->timer.init() != 0) return bail(OJPHGPU_E_HIP);
  owner.p = nullptr;
  *out = e;
  return OJPHGPU_OK;
}

int ojphgpu_encoder_run_container(ojphgpu_encoder* e, const void* d_image, int container);

extern "C" int ojphgpu_encoder_run_device(ojphgpu_encoder* e, const int32_t* d_image) { return ojphgpu_encoder_run_container(e, d_image, 32); }
extern "C" int ojphgpu_encoder_run_device16(ojphgpu_encoder* e, const uint16_t* d_image) { return ojphgpu_encoder_run_container(e, d_image, 16); }
extern "C" int ojphgpu_encoder_run_device8(ojphgpu_encoder* e, const uint8_t* d_image) { return ojphgpu_encoder_run_container(e, d_image, 8); }

// The block coder's schedule over an encoder's `nblocks` blocks (all frames of the run): the counters are cleared; the top
// resolution's share [0, n_top) is coded on the side stream from the point where the main stream stands at fork_top() -- its
// blocks need the first DWT level only -- the rest on the main stream, which then waits for the side stream (join).  The
// products go to out / res / cnt; T (optional) takes an SP_HT_ENC span per launch.
namespace {
struct BlockCoderRun {
  ojphgpu_encoder* e; uint8_t* out; ojphgpu_cb_result* res; uint32_t* cnt; uint32_t nblocks; Spans* T;
  bool forked = false, cleared_on_side = false;
  int more_widths = 0;                                      // `widths` bits this run adds to the cut's (section 5f: bit 7)
  int launch(hipStream_t st, uint32_t first, uint32_t n, int widths) {
    const int sh = T ? T->begin(SP_HT_ENC, st) : -1;
    int rc = ojphgpu::ht_encode_launch(st, (const ojphgpu_cb_desc*)e->cb_descs.p + first, n, e->arena.p, (uint8_t*)e->scratch.p, out,
                                       e->out_cap, res + first, cnt, cnt + 1, widths | more_widths, (const uint32_t*)e->regions.p, e->nreg, first);
    if (rc) return rc;
    if (T) T->end(sh, st);
    return OJPHGPU_OK;
  }
  // (every run of the block coder starts here: a released run of the object that is still coding is joined first)
  int clear() {
    int rc = encoder_settle(e);
    if (rc) return rc;
    e->stream_wrote = true;                                 // (launches on the caller's stream will count in this set)
    HIPCHK(hipMemsetAsync(cnt, 0, e->counters_bytes, e->stream));
    return OJPHGPU_OK;
  }
  // ... but a released run: only the set it is about to reuse (the run two back, where the object has two) is joined on the
  // caller's stream, whose next launch overwrites that set's arena.  The clear itself is off that stream (clear_on_side):
  // `side` -- in order behind the set's last top launch -- waits for the set's low branch (whether or not the caller's
  // stream has: that wait does not order `side`), clears, and ev_clear lets `low` follow (fork_top); the side launch of this
  // run is behind the clear in stream order.  Not where the set's last run counted on the caller's stream (a joined or
  // searching run: stream_wrote), which `side` is not ordered behind: there the clear stays on the caller's stream, behind
  // that run and in front of this run's fork.
  int clear_released() {
    int rc = encoder_settle_last(e);
    if (rc) return rc;
    cleared_on_side = e->clear_on_side && !e->stream_wrote;
    e->stream_wrote = false;
    if (!cleared_on_side) { HIPCHK(hipMemsetAsync(cnt, 0, e->counters_bytes, e->stream)); return OJPHGPU_OK; }
    HIPCHK(hipStreamWaitEvent(e->side, e->ev_low, 0));      // (never recorded, or long complete: no wait)
    HIPCHK(hipMemsetAsync(cnt, 0, e->counters_bytes, e->side));
    HIPCHK(hipEventRecord(e->ev_clear, e->side));
    return OJPHGPU_OK;
  }
  // the top resolution's blocks are ready to be coded; release: the caller's stream is left here, the rest of the run goes to e->low
  int fork_top(bool release = false) {
    forked = true;
    HIPCHK(hipEventRecord(e->ev_fork, e->stream));
    HIPCHK(hipStreamWaitEvent(e->side, e->ev_fork, 0));
    int rc = launch(e->side, 0, e->n_top, e->widths_top);
    if (rc) return rc;
    HIPCHK(hipEventRecord(e->ev_join, e->side));
    if (release) {                                          // (pending from here: also a run that fails below)
      e->pending = true;
      HIPCHK(hipStreamWaitEvent(e->low, e->ev_fork, 0));
      if (cleared_on_side) HIPCHK(hipStreamWaitEvent(e->low, e->ev_clear, 0));
    }
    return OJPHGPU_OK;
  }
  // the other blocks behind the lower levels on e->low; nobody waits yet (the caller records ev_low: ReleasedBranch)
  int rest_released() { return launch(e->low, e->n_top, nblocks - e->n_top, e->widths_rest); }
  int rest_and_join() {                                     // (forks here if nobody has)
    int rc = e->n_top && !forked ? fork_top() : OJPHGPU_OK;
    if (rc) return rc;
    rc = launch(e->stream, e->n_top, nblocks - e->n_top, e->widths_rest);
    if (rc) return rc;
    if (e->n_top) HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join, 0));
    return OJPHGPU_OK;
  }
};
// From the fork of a released run on, EVERY way out of the run records ev_low behind what has been queued on e->low -- a run
// that fails half way has launches there too, and the settle of the next run must wait for them, not for an older record.
struct ReleasedBranch {
  ojphgpu_encoder* e; bool armed = false;
  ~ReleasedBranch() { if (armed) (void)hipEventRecord(e->ev_low, e->low); }
};
}  // namespace

// container: 32 = int32 samples, 16 / 8 = 16- / 8-bit samples (two's complement for signed components, else unsigned)
int ojphgpu_encoder_run_container(ojphgpu_encoder* e, const void* d_image, int container)
{
  if (!e || !d_image) return OJPHGPU_E_INVALID;
  const Plan& P = *e->P;
  if (container != 32 && container != 16 && container != 8) return OJPHGPU_E_INVALID;
  if (container != 32) for (const CompGeo& g : P.comps) if (g.bit_depth > (uint32_t)container) return OJPHGPU_E_INVALID;
  hipStream_t s = e->stream;
  Spans& T = e->timer;
  const bool release = encoder_releases(e);                 // the caller's stream is left behind the last launch that reads the frame
  if (release) encoder_next_set(e);                         // (from here on arena / out / results / counters are this run's)
  e->take_cut(release ? e->cut_released : e->cut_joined);
  BlockCoderRun coder{ e, (uint8_t*)(e->o_out ? e->o_out : e->out.p),         // a pipeline slot's buffers, or the object's own
                       (ojphgpu_cb_result*)(e->o_results ? e->o_results : e->results.p),
                       (uint32_t*)(e->o_counters ? e->o_counters : e->counters.p), (uint32_t)e->block_ids.size() * e->nframes, &T };
  int rc = release ? coder.clear_released() : coder.clear();   // (joins the released runs of this object that are in its way)
  if (rc) return rc;
  ReleasedBranch branch{ e };
  T.start(s);
  if (e->need_convert) {
    const int sp = T.begin(SP_CONVERT, s);
    rc = ojphgpu_convert_forward_ex(s, &P.p, (const ojphgpu_convert_desc*)e->conv_descs.p, e->tiles.count * e->nframes,
                                    e->conv_max_w, e->conv_max_h, d_image, e->arena.p, container);
    T.end(sp, s);
  }
  if (rc) return rc;
  const bool budget = e->searches() || e->trunc_on;         // the blocks are coded by the search, in ojphgpu_encoder_finish*
  for (size_t i = 0; i < e->batches.size(); ++i) {
    const LevelBatch& b = e->batches[i];
    const int sp = T.begin(SP_DWT, s);
    if (b.img_first >= 0) {                                 // level shift / int->float applied in the loads
      ojphgpu_params pp = P.p; pp.reversible = b.rev ? 1 : 0; pp.bit_depth = b.img_depth; pp.is_signed = b.img_signed;
      const ojphgpu_dwt_desc* idesc = (const ojphgpu_dwt_desc*)e->img_descs.p + b.img_first;
      rc = b.general ? ojphgpu_dwt_forward_general_image(s, &b.k, &pp, idesc, b.count, b.max_w, b.max_h, d_image, e->arena.p, container)
                     : ojphgpu_dwt_forward_image_ex(s, &pp, idesc, b.count, b.max_w, b.max_h, d_image, e->arena.p, container, b.nc == 3);
    } else if (b.general)                                   // 64-bit samples, Part-2 wavelets / decompositions: the general lifting kernels
      rc = ojphgpu_dwt_forward_general(s, &b.k, (const ojphgpu_dwt_desc*)e->dwt_descs.p + b.first, b.count, b.max_w, b.max_h, e->arena.p);
    else
      rc = ojphgpu_dwt_forward(s, b.rev ? 1 : 0, (const ojphgpu_dwt_desc*)e->dwt_descs.p + b.first, b.count,
                               b.max_w, b.max_h, e->arena.p);
    if (rc) return rc;
    T.end(sp, s);
    const bool top_done = b.depth == 0 && (i + 1 == e->batches.size() || e->batches[i + 1].depth != 0);
    if (!budget && e->n_top && top_done) {
      if ((rc = coder.fork_top(release)) != 0) return rc;
      if (release) { s = e->low; branch.armed = true; }     // nothing behind this point touches the caller's memory
    }
  }
  if (e->trunc_on) {                                        // section 5f: under a cap the search wants the integer statistics
    EncoderTrunc& R = *e->trunc;
    if (e->trunc_level < 0) {
      HIPCHK(hipMemsetAsync(R.hist.p, 0, R.hist.n, s));
      const int sp = T.begin(SP_STATS, s);
      rc = ojphgpu_band_stats_int(s, (const ojphgpu_stats_desc*)R.stats_descs.p, R.n_stats, R.stats_max_w, R.stats_max_h, e->arena.p, (uint32_t*)R.hist.p);
      if (rc) return rc;
      T.end(sp, s);
    }
    T.finish(s);
    R.searched = false;
    e->ran = true; e->fetched = false;
    return OJPHGPU_OK;
  }
  if (e->quality_on) {                                      // the search reads the planes in the arena and the caller's frame
    T.finish(s);
    e->quality->frame = d_image; e->quality->container = container;
    e->rate->searched = false;
    e->ran = true; e->fetched = false;
    return OJPHGPU_OK;
  }
  if (budget) {
    EncoderRate& R = *e->rate;
    HIPCHK(hipMemsetAsync(R.hist.p, 0, R.hist.n, s));
    const int sp = T.begin(SP_STATS, s);
    rc = ojphgpu_band_stats(s, (const ojphgpu_stats_desc*)R.stats_descs.p, R.n_stats, R.stats_max_w, R.stats_max_h, e->arena.p, (uint32_t*)R.hist.p);
    if (rc) return rc;
    T.end(sp, s);
    T.finish(s);
    R.searched = false;
    e->ran = true; e->fetched = false;
    return OJPHGPU_OK;
  }
  if (release && coder.forked) {
    if ((rc = coder.rest_released()) != 0) return rc;
    T.finish_two(s, e->side);
  } else {
    if ((rc = coder.rest_and_join()) != 0) return rc;
    T.finish(s);
  }
  e->ran = true; e->fetched = false;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_encoder_set_timing(ojphgpu_encoder* e, int per_launch)
{
  if (!e) return OJPHGPU_E_INVALID;
  e->timer.detail = per_launch != 0;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_encoder_is_pending(const ojphgpu_encoder* e, int* pending)
{
  if (!e || !pending) return OJPHGPU_E_INVALID;
  *pending = e->pending ? 1 : 0;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_encoder_coded_bytes(ojphgpu_encoder* e, uint64_t* bytes)
{
  if (!e || !bytes || !e->ran) return OJPHGPU_E_INVALID;
  int rc = encoder_settle(e);                               // (every finish comes through here before it reads a product)
  if (rc) return rc;
  e->h_cursors.assign(e->counters_bytes / 4, 0);
  HIPCHK(hipMemcpyAsync(e->h_cursors.data(), e->counters.p, e->counters_bytes, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  uint64_t total = e->h_cursors[0];
  for (uint32_t r = 1; r < e->nreg; ++r) total += e->h_cursors[32 * (size_t)r];
  *bytes = total;
  return e->h_cursors[1] ? OJPHGPU_E_OVERFLOW : OJPHGPU_OK;
}

// D2H of the block bytes + lengths of the last run (once per run); fills the plan-order coded-block
// table of frame `frame`
static int encoder_fetch(ojphgpu_encoder* e, uint32_t frame, std::vector<ojphgpu_coded_block>& cb)
{
  if (frame >= e->nframes) return OJPHGPU_E_INVALID;
  // (a byte budget, a quality target: the plan at the step the search chose for this frame)
  const Plan& P = e->searches() ? e->rate->frame_plan[frame]->plan : *e->P;
  if (!e->fetched) {
    int rc = ojphgpu_encoder_coded_bytes(e, &e->nbytes);
    if (rc) return rc;
    const size_t rbytes = e->h_results.size() * sizeof(ojphgpu_cb_result);
    if (e->h_out.reserve(std::max<size_t>((size_t)e->nbytes + 16, (size_t)e->out_cap / 4)) || e->h_res.reserve(rbytes + 16))
      return OJPHGPU_E_NOMEM;
    if (rbytes) HIPCHK(hipMemcpyAsync(e->h_res.p, e->results.p, rbytes, hipMemcpyDeviceToHost, e->stream));
    // the used part of every region goes to a compact host buffer; the blocks' offsets are moved along below
    std::vector<uint64_t> hpos(e->nreg ? e->nreg : 1, 0);
    if (e->nreg) {
      uint64_t at = 0;
      for (uint32_t r = 0; r < e->nreg; ++r) {
        const uint32_t used = e->h_cursors[32 * (size_t)r];
        hpos[r] = at;
        if (used) HIPCHK(hipMemcpyAsync(e->h_out.p + at, (const uint8_t*)e->out.p + e->h_regions[2 * r], used, hipMemcpyDeviceToHost, e->stream));
        at += used;
      }
    } else if (e->nbytes) HIPCHK(hipMemcpyAsync(e->h_out.p, e->out.p, (size_t)e->nbytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    if (rbytes) memcpy(e->h_results.data(), e->h_res.p, rbytes);
    if (e->nreg)
      for (size_t i = 0; i < e->h_results.size(); ++i) {
        const uint32_t r = (uint32_t)i & (e->nreg - 1);     // (by the index among all blocks: encoder_block_layout)
        if (e->h_results[i].length) e->h_results[i].offset = (uint32_t)(e->h_results[i].offset - e->h_regions[2 * r] + hpos[r]);
      }
    e->fetched = true;
  }
  ojphgpu_coded_blocks(P, e->block_ids, e->h_results.data() + (size_t)frame * e->block_ids.size(), cb,
                       e->trunc_on ? e->trunc->band_drop.data() : nullptr);
  return OJPHGPU_OK;
}

static int encoder_rate_search(ojphgpu_encoder* e);
static int encoder_trunc_code(ojphgpu_encoder* e);
static int encoder_quality_search(ojphgpu_encoder* e);
static int encoder_capped_search(ojphgpu_encoder* e);

extern "C" int ojphgpu_encoder_finish(ojphgpu_encoder* e, uint8_t* h_out, size_t cap, size_t* out_len)
{
  if (!e || !out_len || !e->ran) return OJPHGPU_E_INVALID;
  return ojphgpu_encoder_finish_frame(e, 0, h_out, cap, out_len);
}

extern "C" int ojphgpu_encoder_finish_frame(ojphgpu_encoder* e, uint32_t frame, uint8_t* h_out, size_t cap, size_t* out_len)
{
  if (!e || !out_len || !e->ran) return OJPHGPU_E_INVALID;
  if (e->tiles.first != 0 || e->tiles.count != e->P->tiles.size()) return OJPHGPU_E_INVALID;   // use _finish_tiles
  if (frame >= e->nframes) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
  std::vector<ojphgpu_coded_block> cb;
  const bool tm = getenv("OJPHGPU_TIMING") != nullptr;
  auto now = [] { return std::chrono::steady_clock::now(); };
  auto t0 = now();
  const bool budgets = !e->budgets.empty();
  int rc = e->trunc_on ? encoder_trunc_code(e)
         : e->quality_on ? (e->cap_bytes ? encoder_capped_search(e) : encoder_quality_search(e)) : budgets ? encoder_rate_search(e) : OJPHGPU_OK;
  if (rc) return rc;
  ojphgpu_rate_info info;
  if (budgets && (rc = ojphgpu_rate_rounds_frame(e->rate->rounds, frame, &info)) != 0) return rc;   // (OJPHGPU_E_BUDGET: this frame's alone)
  if (e->searches()) t0 = now();
  rc = encoder_fetch(e, frame, cb);
  if (rc) return rc;
  auto t1 = now();
  rc = ojphgpu_t2_write(e->searches() ? e->rate->frame_plan[frame] : e->handle, e->h_out.p, cb.data(), h_out, cap, out_len);
  if (budgets) e->rate->final_ms = std::chrono::duration<double, std::milli>(now() - t0).count();
  if (e->trunc_on && e->trunc_level >= 0 && (rc == OJPHGPU_OK || rc == OJPHGPU_E_OVERFLOW)) e->trunc->info.bytes = *out_len;   // (a fixed level: nothing measured it)
  if (e->quality_on) e->quality->final_ms += std::chrono::duration<double, std::milli>(now() - t0).count();
  if (tm) fprintf(stderr, "ojphgpu: finish frame %u: D2H %.2f ms, Tier-2 %.2f ms\n", frame,
                  std::chrono::duration<double, std::milli>(t1 - t0).count(),
                  std::chrono::duration<double, std::milli>(now() - t1).count());
  return rc;
  });
}

extern "C" int ojphgpu_encoder_finish_tiles(ojphgpu_encoder* e, uint8_t* h_out, size_t cap, size_t* out_len,
                                             uint32_t* tile_part_len)
{
  if (!e || !out_len || !e->ran || e->searches() || e->trunc_on) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    std::vector<ojphgpu_coded_block> cb;
    int rc = encoder_fetch(e, 0, cb);
    if (rc) return rc;
    return ojphgpu_t2_write_tiles(e->handle, e->h_out.p, cb.data(), e->tiles.first, e->tiles.count, h_out, cap,
                                  out_len, tile_part_len);
  });
}

namespace ojphgpu {
int assemble_launch(void* stream, const T2Job* d_jobs, uint32_t njobs, const uint8_t* d_blob, const uint8_t* d_data, uint8_t* d_out);
int publish_words_launch(void* stream, uint32_t* d_dst, const uint32_t* src, uint32_t n);
int copy_to_host_launch(void* stream, void* d_dst, const void* src, size_t bytes);
}

// The tile-parts of the range assembled in HBM (kernels_assemble.hip) instead of on the host: only the block
// lengths come to the host, the layout goes back, and the bytes stay on the device -- where the final
// codestream gather of a multi-GPU encode picks them up (RCCL send over xGMI, openjph_amd/shard.py).
extern "C" int ojphgpu_encoder_finish_tiles_device(ojphgpu_encoder* e, uint8_t* d_out, size_t cap, size_t* out_len,
                                                    uint32_t* tile_part_len)
{
  if (!e || !out_len || !e->ran || e->searches() || e->trunc_on) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    const Plan& P = *e->P;
    uint64_t nbytes = 0;
    int rc = ojphgpu_encoder_coded_bytes(e, &nbytes);
    if (rc) return rc;
    const size_t rbytes = e->h_results.size() * sizeof(ojphgpu_cb_result);
    if (rbytes) HIPCHK(hipMemcpyAsync(e->h_results.data(), e->results.p, rbytes, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    e->fetched = false;                                   // h_results holds device offsets again
    std::vector<ojphgpu_coded_block> cb;
    ojphgpu_coded_blocks(P, e->block_ids, e->h_results.data(), cb);
    T2Layout L;
    rc = t2_layout_tiles(P, cb.data(), e->tiles.first, (size_t)e->tiles.first + e->tiles.count, L, tile_part_len);
    if (rc) return rc;
    *out_len = (size_t)L.total;
    if (!d_out || cap < L.total) return OJPHGPU_E_OVERFLOW;
    const size_t jbytes = L.jobs.size() * sizeof(T2Job), boff = (jbytes + 63) & ~(size_t)63;
    DeviceBuf lay;
    if (lay.alloc(boff + L.blob.size() + 64)) return OJPHGPU_E_NOMEM;
    struct Free { DeviceBuf& b; ~Free() { b.release(); } } fr{ lay };
    if (jbytes) HIPCHK(hipMemcpyAsync(lay.p, L.jobs.data(), jbytes, hipMemcpyHostToDevice, e->stream));
    if (!L.blob.empty()) HIPCHK(hipMemcpyAsync((uint8_t*)lay.p + boff, L.blob.data(), L.blob.size(), hipMemcpyHostToDevice, e->stream));
    rc = assemble_launch(e->stream, (const T2Job*)lay.p, (uint32_t)L.jobs.size(), (const uint8_t*)lay.p + boff,
                         (const uint8_t*)(e->o_out ? e->o_out : e->out.p), d_out);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));            // the layout staging goes away with this call
    return OJPHGPU_OK;
  });
}

// ---------------------------------------------------------------------------------------------
// encoding to a byte budget (include/ojphgpu.h section 5b)
// ---------------------------------------------------------------------------------------------
// the block descriptors of an encoder that searched go back to the plan's own step
static int encoder_restore_descs(ojphgpu_encoder* e)
{
  HIPCHK(hipSetDevice(e->device));
  int rc = encoder_settle(e);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  const std::vector<ojphgpu_cb_desc>& bd = e->rate->bd;
  if (!bd.empty()) HIPCHK(hipMemcpy(e->cb_descs.p, bd.data(), bd.size() * sizeof(bd[0]), hipMemcpyHostToDevice));
  e->ran = false;
  return OJPHGPU_OK;
}

static bool encoder_may_search(const ojphgpu_encoder* e)
{
  const Plan& P = *e->P;
  return e->tiles.first == 0 && e->tiles.count == P.tiles.size() && !e->o_out && rate_plan_ok(P);
}

static int encoder_rate_setup(ojphgpu_encoder* e);

extern "C" int ojphgpu_encoder_set_budget(ojphgpu_encoder* e, uint64_t max_bytes)
{
  if (!e) return OJPHGPU_E_INVALID;
  if (max_bytes == 0) {
    if (!e->budgets.empty() && e->rate) { const int rc = encoder_restore_descs(e); if (rc) return rc; }
    e->budgets.clear();
    return OJPHGPU_OK;
  }
  if (e->nframes > 1) return OJPHGPU_E_INVALID;             // (a batch encoder: ojphgpu_encoder_set_budgets, also for equal budgets)
  return ojphgpu_encoder_set_budgets(e, &max_bytes, 1);
}

extern "C" int ojphgpu_encoder_set_budgets(ojphgpu_encoder* e, const uint64_t* max_bytes, uint32_t n)
{
  if (!e || !max_bytes || n != e->nframes) return OJPHGPU_E_INVALID;
  uint32_t zeros = 0;
  for (uint32_t f = 0; f < n; ++f) zeros += max_bytes[f] == 0;
  if (zeros == n) return ojphgpu_encoder_set_budget(e, 0);
  if (zeros) return OJPHGPU_E_INVALID;
  if (!encoder_may_search(e) || e->quality_on) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    if (!e->rate) { const int rc = encoder_rate_setup(e); if (rc) return rc; }
    { const int rc = encoder_settle(e); if (rc) return rc; }   // an object that gains a budget: no released run is left in flight
    e->budgets.assign(max_bytes, max_bytes + n);
    e->ran = false;
    return OJPHGPU_OK;
  });
}

// what a searching encoder needs (the first ojphgpu_encoder_set_budget / _set_quality): the quantisation of every step, the
// band statistics' tables, the blocks' classes, and scratch slots and an output that hold the finest step of the grid
static int encoder_rate_setup(ojphgpu_encoder* e)
{
  const Plan& P = *e->P;
  return no_throw([&]() -> int {
    HIPCHK(hipSetDevice(e->device));
    EncoderRate* R = new EncoderRate();
    struct Owner { EncoderRate* p; ~Owner() { delete p; } } owner{ R };
    for (const Band& B : P.bands) if ((uint64_t)B.r.w * B.r.h > 0xFFFFFFFFull) return OJPHGPU_E_INVALID;   // the counts are 32 bits wide
    int rc = rate_table_build(P, R->table);
    if (rc) return rc;
    const uint32_t nframes = e->nframes;
    if ((uint64_t)P.bands.size() * nframes > 0xFFFFFFFFull) return OJPHGPU_E_INVALID;   // (the slots are 32 bits wide)
    std::vector<ojphgpu_stats_desc> sd;
    for (uint32_t f = 0; f < nframes; ++f)                    // frame-major: the histograms are [frames][bands][bins]
      for (size_t i = 0; i < P.bands.size(); ++i) {
        const Band& B = P.bands[i];
        if (B.empty) continue;
        sd.push_back(ojphgpu_stats_desc{ B.plane_off + (uint64_t)f * P.arena_elems, B.pitch, B.r.w, B.r.h, (uint32_t)(f * P.bands.size() + i) });
        R->stats_max_w = std::max(R->stats_max_w, B.r.w); R->stats_max_h = std::max(R->stats_max_h, B.r.h);
      }
    R->n_stats = (uint32_t)sd.size();
    std::vector<uint32_t> cls(e->block_ids.size());
    for (size_t i = 0; i < cls.size(); ++i) cls[i] = R->table.band_class[P.blocks[e->block_ids[i]].band];
    // The scratch slots and the compacted output are sized for the finest step of the grid -- the largest K_max a trial can
    // give a band -- so that no trial can overflow them whatever the budget
    const uint32_t nc = R->table.nclasses;
    std::vector<uint32_t> kfine(P.bands.size());
    for (size_t i = 0; i < kfine.size(); ++i) kfine[i] = R->table.quant[(size_t)(OJPHGPU_RATE_GRID - 1) * nc + R->table.band_class[i]].K_max;
    std::vector<ojphgpu_cb_desc>& bd = R->bd;
    uint64_t scratch_bytes = 0;
    {
      // A batch: the bound of all frames at the finest step has to fit the 32-bit byte cursor unclamped -- a clamped output
      // could overflow in a fine trial, which the search takes as impossible.  Refused with the encoder as it was.
      const uint32_t out_cap = e->out_cap, nreg = e->nreg; const size_t counters_bytes = e->counters_bytes;
      const std::vector<uint32_t> regions = e->h_regions;
      bool clamped = false;
      encoder_block_layout(e, kfine.data(), bd, scratch_bytes, &clamped);
      if (clamped && nframes > 1) {                           // fewer frames per batch
        e->out_cap = out_cap; e->nreg = nreg; e->counters_bytes = counters_bytes; e->h_regions = regions;
        return OJPHGPU_E_INVALID;
      }
    }
    { const int rc = encoder_settle(e); if (rc) return rc; }   // a released run still codes into the buffers replaced below
    HIPCHK(hipStreamSynchronize(e->stream));
    if (e->side) HIPCHK(hipStreamSynchronize(e->side));
    e->scratch.release(); e->out.release(); e->regions.release(); e->counters.release();
    if (e->two_sets) {                                      // (the sets keep equal sizes: released runs come back with budget 0)
      e->other.out.release(); e->other.counters.release();
      if (e->other.out.alloc(e->out_cap) || e->other.counters.alloc(e->counters_bytes)) return OJPHGPU_E_NOMEM;
    }
    if (e->scratch.alloc(scratch_bytes) || e->out.alloc(e->out_cap) || e->counters.alloc(e->counters_bytes) ||
        (e->nreg && e->regions.alloc(e->h_regions.size() * 4)) ||
        R->stats_descs.alloc(sd.size() * sizeof(sd[0])) || R->hist.alloc(P.bands.size() * OJPHGPU_STATS_BINS * 4 * nframes) ||
        R->block_class.alloc(cls.size() * 4) || R->quant.alloc((size_t)nc * sizeof(BandQuant) * nframes))
      return OJPHGPU_E_NOMEM;
    if (e->nreg) HIPCHK(hipMemcpy(e->regions.p, e->h_regions.data(), e->h_regions.size() * 4, hipMemcpyHostToDevice));
    if (!bd.empty()) HIPCHK(hipMemcpy(e->cb_descs.p, bd.data(), bd.size() * sizeof(bd[0]), hipMemcpyHostToDevice));
    if (!sd.empty()) HIPCHK(hipMemcpy(R->stats_descs.p, sd.data(), sd.size() * sizeof(sd[0]), hipMemcpyHostToDevice));
    if (!cls.empty()) HIPCHK(hipMemcpy(R->block_class.p, cls.data(), cls.size() * 4, hipMemcpyHostToDevice));
    R->h_hist.assign(P.bands.size() * OJPHGPU_STATS_BINS * nframes, 0);
    R->h_quant.assign((size_t)nc * nframes, BandQuant{ 0.0f, 0 });
    e->rate = R; owner.p = nullptr;
    e->ran = false;
    return OJPHGPU_OK;
  });
}

// One coding round of a search: frame f of the encoder coded at grid index idx[f] into the output set `o`, in the schedule of
// a plain run (BlockCoderRun, fork and rest back to back) -- so the compacted output and its cursors are what a plain run
// leaves.  The block lengths of all frames come to the host, *lengths, the way the set says: into mapped pinned memory the
// coder writes itself (a frame pipeline), or by a copy into the encoder's pageable table.
static int encoder_code_round(ojphgpu_encoder* e, const RateTrialOut& o, const uint32_t* idx, const ojphgpu_cb_result** lengths)
{
  EncoderRate& R = *e->rate;
  hipStream_t s = e->stream;
  const uint32_t F = e->nframes, nc = R.table.nclasses, nb = (uint32_t)e->block_ids.size();
  for (uint32_t f = 0; f < F; ++f) std::copy_n(&R.table.quant[(size_t)idx[f] * nc], nc, &R.h_quant[(size_t)f * nc]);
  HIPCHK(hipMemcpyAsync(R.quant.p, R.h_quant.data(), R.h_quant.size() * sizeof(BandQuant), hipMemcpyHostToDevice, s));
  int rc = requant_frames_launch(s, (ojphgpu_cb_desc*)e->cb_descs.p, nb, F, (const uint32_t*)R.block_class.p, (const BandQuant*)R.quant.p, nc);
  if (rc) return rc;
  BlockCoderRun coder{ e, (uint8_t*)o.out, o.d_results, o.d_counters, nb * F, nullptr };
  if ((rc = coder.clear()) != 0 || (rc = coder.rest_and_join()) != 0) return rc;
  uint32_t status = 0;
  const auto w0 = std::chrono::steady_clock::now();
  if (o.h_results) {                                        // the coder wrote them there; the cursors follow, then the event
    if ((rc = publish_words_launch(s, o.d_publish, o.d_counters, 2)) != 0) return rc;
    HIPCHK(hipEventRecord(o.done, s));
    HIPCHK(hipEventSynchronize(o.done));
    status = o.h_publish[1];
    *lengths = o.h_results;
  } else {                                                  // (a copy into pageable memory waits for the launches before it)
    const size_t rbytes = e->h_results.size() * sizeof(ojphgpu_cb_result);
    if (rbytes) HIPCHK(hipMemcpyAsync(e->h_results.data(), o.d_results, rbytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(&status, o.d_counters + 1, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    *lengths = e->h_results.data();
  }
  R.wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
  e->fetched = false;
  return status ? OJPHGPU_E_OVERFLOW : OJPHGPU_OK;          // (cannot happen: the buffers hold the finest step's bound; a batch's unclamped)
}

// size(j) of one frame: the length of the codestream Tier-2 lays out from the frame's block lengths, with Q -- the
// encoder's plan at the step the blocks were coded at; or an error (< 0)
static int64_t rate_layout_bytes(const Plan& Q, const std::vector<uint32_t>& block_ids, const ojphgpu_cb_result* lengths)
{
  std::vector<ojphgpu_coded_block> cb;
  ojphgpu_coded_blocks(Q, block_ids, lengths, cb);
  T2Layout L;
  const int rc = t2_layout_codestream(Q, cb.data(), L);
  return rc ? (int64_t)rc : (int64_t)L.total;
}

// one trial for a caller with a plan copy and output sets of its own (the frame pipelines): Q is left at the step of j
int64_t ojphgpu_encoder_rate_trial(ojphgpu_encoder* e, Plan& Q, const RateTrialOut& o, uint32_t j)
{
  if (!rate_apply_step(Q, rate_grid_qstep(j))) return OJPHGPU_E_INVALID;
  const ojphgpu_cb_result* lengths = nullptr;
  const int rc = encoder_code_round(e, o, &j, &lengths);
  return rc ? (int64_t)rc : rate_layout_bytes(Q, e->block_ids, lengths);
}

// The encoder's plan at the index of every frame of a round, R.frame_plan, from the copies kept by visited index
static int encoder_plans_at(ojphgpu_encoder* e, const std::vector<uint32_t>& idx)
{
  EncoderRate& R = *e->rate;
  if (R.plans.size() > 32)                                  // (a sequence that wanders: keep what this round uses)
    for (auto it = R.plans.begin(); it != R.plans.end();) {
      if (std::find(idx.begin(), idx.end(), it->first) == idx.end()) { delete it->second; it = R.plans.erase(it); } else ++it;
    }
  R.frame_plan.assign(idx.size(), nullptr);
  for (size_t f = 0; f < idx.size(); ++f) {
    auto it = R.plans.find(idx[f]);
    if (it == R.plans.end()) {
      std::unique_ptr<ojphgpu_plan> q(new ojphgpu_plan{ *e->P });
      if (!rate_apply_step(q->plan, rate_grid_qstep(idx[f]))) return OJPHGPU_E_INVALID;
      it = R.plans.emplace(idx[f], q.release()).first;
    }
    R.frame_plan[f] = it->second;
  }
  return OJPHGPU_OK;
}

// The search of the last run, once, for the one frame of a single encoder or the frames of a batch: the rounds of
// ojphgpu_rate_rounds (ojph_rate.cpp), which says what every frame is coded at and which frames measure.  The block
// lengths of a round come back once, and the layouts of the frames that measure (independent of each other) run on the
// pool.  When the rounds end the device holds every frame as finish_frame writes it, and R.frame_plan stands at its step.
static int encoder_rate_search(ojphgpu_encoder* e)
{
  EncoderRate& R = *e->rate;
  if (R.searched) return R.search_rc;
  const auto t0 = std::chrono::steady_clock::now();
  R.wait_ms = 0;
  auto run = [&]() -> int {
    const uint32_t F = e->nframes, nb = (uint32_t)e->block_ids.size();
    if (e->budgets.size() != F) return OJPHGPU_E_INVALID;
    HIPCHK(hipMemcpyAsync(R.h_hist.data(), R.hist.p, R.h_hist.size() * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    R.wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ojphgpu_rate_rounds_destroy(R.rounds); R.rounds = nullptr;
    int rc = rate_rounds_create(R.table, R.h_hist.data(), e->P->bands.size() * OJPHGPU_STATS_BINS, e->budgets.data(), F, -1, &R.rounds);
    if (rc) return rc;
    const RateTrialOut own{ e->out.p, (ojphgpu_cb_result*)e->results.p, (uint32_t*)e->counters.p, nullptr, nullptr, nullptr, nullptr };
    std::vector<uint32_t> idx(F, 0), list; std::vector<uint8_t> measures(F, 0); std::vector<int64_t> sizes(F, 0);
    while ((rc = ojphgpu_rate_rounds_next(R.rounds, idx.data(), measures.data())) == 1) {
      const ojphgpu_cb_result* lengths = nullptr;
      if ((rc = encoder_plans_at(e, idx)) != 0 || (rc = encoder_code_round(e, own, idx.data(), &lengths)) != 0) return rc;
      list.clear();
      for (uint32_t f = 0; f < F; ++f) if (measures[f]) list.push_back(f);
      parallel_for(list.size(), [&](size_t k) {
        const uint32_t f = list[k];
        sizes[f] = rate_layout_bytes(R.frame_plan[f]->plan, e->block_ids, lengths + (size_t)f * nb);
      });
      if ((rc = ojphgpu_rate_rounds_feed(R.rounds, sizes.data())) != 0) return rc;
    }
    return rc;
  };
  R.search_rc = no_throw(run);
  R.searched = true;
  R.search_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return R.search_rc;
}

// OJPHGPU_E_BUDGET: nothing fits that frame's budget (info: passes, first_guess)
extern "C" int ojphgpu_encoder_rate_info_frame(ojphgpu_encoder* e, uint32_t frame, ojphgpu_rate_info* info)
{
  if (!e || !info || !e->rate || frame >= e->nframes) return OJPHGPU_E_INVALID;
  const EncoderRate& R = *e->rate;
  if (e->budgets.empty() || !R.searched || R.search_rc) return OJPHGPU_E_INVALID;
  return ojphgpu_rate_rounds_frame(R.rounds, frame, info);
}

extern "C" int ojphgpu_encoder_rate_info(ojphgpu_encoder* e, ojphgpu_rate_info* info)
{
  const int rc = ojphgpu_encoder_rate_info_frame(e, 0, info);
  return rc == OJPHGPU_E_BUDGET ? OJPHGPU_OK : rc;
}

extern "C" int ojphgpu_encoder_rate_rounds(ojphgpu_encoder* e, uint32_t* rounds)
{
  if (!e || !rounds || !e->rate || !e->rate->searched || e->budgets.empty()) return OJPHGPU_E_INVALID;
  return ojphgpu_rate_rounds_count(e->rate->rounds, rounds);
}

extern "C" int ojphgpu_encoder_rate_timing(ojphgpu_encoder* e, float out[4])
{
  if (!e || !out || !e->rate || !e->rate->searched || !e->ran) return OJPHGPU_E_INVALID;
  out[0] = (float)e->rate->search_ms; out[1] = (float)e->rate->wait_ms; out[2] = (float)e->rate->final_ms;
  if (e->timer.read(SP_STATS, &out[3])) return OJPHGPU_E_HIP;
  return OJPHGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// a reversible frame under a byte cap (include/ojphgpu.h section 5f)
// ---------------------------------------------------------------------------------------------
static int encoder_trunc_setup(ojphgpu_encoder* e)
{
  const Plan& P = *e->P;
  return no_throw([&]() -> int {
    HIPCHK(hipSetDevice(e->device));
    std::unique_ptr<EncoderTrunc> R(new EncoderTrunc());
    for (const Band& B : P.bands) if ((uint64_t)B.r.w * B.r.h > 0xFFFFFFFFull) return OJPHGPU_E_INVALID;   // the counts are 32 bits wide
    int rc = trunc_ladder_build(P, R->ladder);
    if (rc) return rc;
    std::vector<ojphgpu_stats_desc> sd;
    for (size_t i = 0; i < P.bands.size(); ++i) {
      const Band& B = P.bands[i];
      if (B.empty) continue;
      sd.push_back(ojphgpu_stats_desc{ B.plane_off, B.pitch, B.r.w, B.r.h, (uint32_t)i });
      R->stats_max_w = std::max(R->stats_max_w, B.r.w); R->stats_max_h = std::max(R->stats_max_h, B.r.h);
    }
    R->n_stats = (uint32_t)sd.size();
    std::vector<uint32_t> cls(e->block_ids.size());
    for (size_t i = 0; i < cls.size(); ++i) cls[i] = R->ladder.band_class[P.blocks[e->block_ids[i]].band];
    const size_t nc = R->ladder.class_band.size();
    if (R->stats_descs.alloc(std::max<size_t>(sd.size(), 1) * sizeof(sd[0])) || R->hist.alloc(P.bands.size() * OJPHGPU_STATS_BINS * 4) ||
        R->block_class.alloc(std::max<size_t>(cls.size(), 1) * 4) || R->drop.alloc(std::max<size_t>(nc, 4)))
      return OJPHGPU_E_NOMEM;
    if (!sd.empty()) HIPCHK(hipMemcpy(R->stats_descs.p, sd.data(), sd.size() * sizeof(sd[0]), hipMemcpyHostToDevice));
    if (!cls.empty()) HIPCHK(hipMemcpy(R->block_class.p, cls.data(), cls.size() * 4, hipMemcpyHostToDevice));
    R->h_hist.assign(P.bands.size() * OJPHGPU_STATS_BINS, 0);
    R->h_drop.assign(nc, 0); R->band_drop.assign(P.bands.size(), 0);
    e->trunc = R.release();
    return OJPHGPU_OK;
  });
}

// the table of `level` into the block descriptors, on the encoder's stream
static int encoder_trunc_descs(ojphgpu_encoder* e, uint32_t level)
{
  EncoderTrunc& R = *e->trunc;
  for (size_t c = 0; c < R.h_drop.size(); ++c) R.h_drop[c] = R.ladder.drop(level, R.ladder.class_band[c]);
  HIPCHK(hipMemcpyAsync(R.drop.p, R.h_drop.data(), R.h_drop.size(), hipMemcpyHostToDevice, e->stream));
  return trunc_descs_launch(e->stream, (ojphgpu_cb_desc*)e->cb_descs.p, (uint32_t)e->block_ids.size(), (const uint32_t*)R.block_class.p,
                            (const uint8_t*)R.drop.p);
}

static bool encoder_may_truncate(const ojphgpu_encoder* e)
{
  const Plan& P = *e->P;
  return e->nframes == 1 && e->tiles.first == 0 && e->tiles.count == P.tiles.size() && !e->o_out && !e->o_results && !e->o_counters &&
         !e->searches() && trunc_plan_ok(P);
}

// switches the mode on (cap > 0, or level >= 0) or off; off puts the plan's own descriptors back
static int encoder_trunc_mode(ojphgpu_encoder* e, uint64_t cap, int32_t level)
{
  const bool on = cap > 0 || level >= 0;
  if (!on) {
    if (!e->trunc_on) return OJPHGPU_OK;
    HIPCHK(hipSetDevice(e->device));
    int rc = encoder_settle(e);
    if (rc || (rc = encoder_trunc_descs(e, 0)) != 0) return rc;
    HIPCHK(hipStreamSynchronize(e->stream));
    e->trunc_on = false; e->trunc_bytes = 0; e->trunc_level = -1; e->ran = false;
    return OJPHGPU_OK;
  }
  if (!encoder_may_truncate(e)) return OJPHGPU_E_INVALID;
  if (!e->trunc) { const int rc = encoder_trunc_setup(e); if (rc) return rc; }
  if (level >= 0 && (uint32_t)level >= e->trunc->ladder.levels) return OJPHGPU_E_INVALID;
  { const int rc = encoder_settle(e); if (rc) return rc; }    // an object that gains the mode: no released run is left in flight
  e->trunc_on = true; e->trunc_bytes = cap; e->trunc_level = level;
  e->trunc->have_info = false; e->trunc->searched = false;
  e->ran = false;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_encoder_set_truncation(ojphgpu_encoder* e, uint64_t max_bytes)
{
  if (!e) return OJPHGPU_E_INVALID;
  return encoder_trunc_mode(e, max_bytes, -1);
}

extern "C" int ojphgpu_encoder_set_trunc_level(ojphgpu_encoder* e, int32_t j)
{
  if (!e) return OJPHGPU_E_INVALID;
  return encoder_trunc_mode(e, 0, j < 0 ? -1 : j);
}

extern "C" int ojphgpu_encoder_trunc_timing(ojphgpu_encoder* e, float out[2])
{
  if (!e || !out || !e->trunc_on || !e->trunc || !e->trunc->searched || !e->ran) return OJPHGPU_E_INVALID;
  out[0] = (float)e->trunc->search_ms;
  out[1] = 0.0f;
  if (e->trunc_level < 0 && e->timer.read(SP_STATS, &out[1])) return OJPHGPU_E_HIP;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_encoder_trunc_info(ojphgpu_encoder* e, ojphgpu_trunc_info* info)
{
  if (!e || !info || !e->trunc_on || !e->trunc || !e->trunc->have_info || !e->trunc->searched) return OJPHGPU_E_INVALID;
  *info = e->trunc->info;
  return OJPHGPU_OK;
}

// The blocks of the last run coded at `level` in the schedule of a plain run (so level 0 leaves what a plain run leaves); the
// block lengths come to the host and Tier-2 lays the codestream out: size(level), or an error (< 0).  R.band_drop then
// stands at that level.
static int64_t encoder_trunc_trial(ojphgpu_encoder* e, uint32_t level)
{
  EncoderTrunc& R = *e->trunc;
  const Plan& P = *e->P;
  hipStream_t s = e->stream;
  const uint32_t nb = (uint32_t)e->block_ids.size();
  BlockCoderRun coder{ e, (uint8_t*)e->out.p, (ojphgpu_cb_result*)e->results.p, (uint32_t*)e->counters.p, nb, nullptr };
  int rc = coder.clear();                                   // (settles; the descriptors are rewritten behind every earlier launch)
  if (rc || (rc = encoder_trunc_descs(e, level)) != 0) return rc;
  bool any = false;
  for (size_t b = 0; b < R.band_drop.size(); ++b) { R.band_drop[b] = R.ladder.drop(level, b); any = any || R.band_drop[b]; }
  // the blocks that drop planes take the instantiations of their own (`widths` bit 7) behind the plain ones of the cut: above
  // level 0 both kinds run over all blocks, each skipping the other's
  coder.more_widths = any ? 128 : 0;
  if ((rc = coder.rest_and_join()) != 0) return rc;
  uint32_t status = 0;
  const size_t rbytes = e->h_results.size() * sizeof(ojphgpu_cb_result);
  if (rbytes) HIPCHK(hipMemcpyAsync(e->h_results.data(), e->results.p, rbytes, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&status, (uint32_t*)e->counters.p + 1, 4, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  e->fetched = false;
  if (status) return OJPHGPU_E_OVERFLOW;                    // (cannot happen: fewer planes need no more room than all of them)
  std::vector<ojphgpu_coded_block> cb;
  ojphgpu_coded_blocks(P, e->block_ids, e->h_results.data(), cb, R.band_drop.data());
  T2Layout L;
  rc = t2_layout_codestream(P, cb.data(), L);
  return rc ? (int64_t)rc : (int64_t)L.total;
}

// What ojphgpu_encoder_finish does first in this mode, once per run: the search under the cap, or the fixed level.  When it
// returns OJPHGPU_OK the device holds the frame as finish writes it.
static int encoder_trunc_code(ojphgpu_encoder* e)
{
  EncoderTrunc& R = *e->trunc;
  if (R.searched) return R.search_rc;
  const auto t0 = std::chrono::steady_clock::now();
  auto run = [&]() -> int {
    HIPCHK(hipSetDevice(e->device));
    R.have_info = true;
    memset(&R.info, 0, sizeof(R.info));
    if (e->trunc_level >= 0) {
      const int64_t size = encoder_trunc_trial(e, (uint32_t)e->trunc_level);
      if (size < 0) return (int)size;
      R.info.level = R.info.first_guess = (uint32_t)e->trunc_level; R.info.passes = 1; R.info.bytes = (uint64_t)size;
      R.info.lossless = e->trunc_level == 0;
      for (uint8_t t : R.band_drop) R.info.max_dropped = std::max<uint32_t>(R.info.max_dropped, t);
      return OJPHGPU_OK;
    }
    HIPCHK(hipMemcpyAsync(R.h_hist.data(), R.hist.p, R.h_hist.size() * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    struct Ctx { ojphgpu_encoder* e; int64_t last; } ctx{ e, -1 };
    auto fn = [](void* u, uint32_t j) -> int64_t { Ctx* c = (Ctx*)u; c->last = (int64_t)j; return encoder_trunc_trial(c->e, j); };
    int rc = trunc_search(R.ladder, e->P->blocks.size(), R.h_hist.data(), e->trunc_bytes, fn, &ctx, &R.info);
    if (rc) return rc;
    if (ctx.last != (int64_t)R.info.level) {                // the last trial was not j*: coded once more, the size must be the one measured
      const int64_t size = encoder_trunc_trial(e, R.info.level);
      if (size < 0) return (int)size;
      if ((uint64_t)size != R.info.bytes) return OJPHGPU_E_HIP;
    }
    return OJPHGPU_OK;
  };
  R.search_rc = no_throw(run);
  R.searched = true;
  R.search_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return R.search_rc;
}

// ---------------------------------------------------------------------------------------------
// encoding to a quality target (include/ojphgpu.h section 5c)
// ---------------------------------------------------------------------------------------------
static int decoder_create_synthesis(const ojphgpu_plan* plan, int device, void* stream, ojphgpu_decoder** out);
static int decoder_synthesis_only(ojphgpu_decoder* d, void* d_image, int container);

extern "C" int ojphgpu_encoder_clear_quality(ojphgpu_encoder* e)
{
  if (!e) return OJPHGPU_E_INVALID;
  if (e->quality_on && e->rate) { const int rc = encoder_restore_descs(e); if (rc) return rc; }
  e->quality_on = false; e->cap_bytes = 0;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_encoder_set_quality(ojphgpu_encoder* e, uint64_t max_sse)
{
  if (!e) return OJPHGPU_E_INVALID;
  if (e->nframes > 1 || !encoder_may_search(e) || !e->budgets.empty()) return OJPHGPU_E_INVALID;
  const Plan& P = *e->P;
  for (const CompGeo& g : P.comps) if (g.bit_depth > 16) return OJPHGPU_E_INVALID;
  if (e->quality) {
    if (encoder_settle(e)) return OJPHGPU_E_HIP;            // (as an object that gains a budget)
    e->max_sse = max_sse; e->cap_bytes = 0; e->quality_on = true; e->ran = false;
    return OJPHGPU_OK;
  }
  return no_throw([&]() -> int {
    HIPCHK(hipSetDevice(e->device));
    {                                                       // the half bit needs room below the coded bits at every step
      RateTable T;
      const int rc = e->rate ? OJPHGPU_OK : rate_table_build(P, T);
      if (rc) return rc;
      const RateTable& U = e->rate ? e->rate->table : T;
      for (uint32_t c = 0; c < U.nclasses; ++c) if (U.quant[(size_t)(OJPHGPU_RATE_GRID - 1) * U.nclasses + c].K_max > 30) return OJPHGPU_E_INVALID;
    }
    if (!e->rate) { const int rc = encoder_rate_setup(e); if (rc) return rc; }
    EncoderQuality* Q = new EncoderQuality();
    struct Owner { EncoderQuality* p; ~Owner() { delete p; } } owner{ Q };
    int rc = decoder_create_synthesis(e->handle, e->device, e->stream, &Q->syn);
    if (rc) return rc;
    for (size_t i = 0; i < P.bands.size(); ++i) {
      const Band& B = P.bands[i];
      if (B.empty) continue;
      ojphgpu_requant_desc d; memset(&d, 0, sizeof(d));
      d.plane_off = B.plane_off; d.pitch = B.pitch; d.w = B.r.w; d.h = B.r.h;
      Q->h_descs.push_back(d); Q->desc_band.push_back((uint32_t)i);
      Q->max_w = std::max(Q->max_w, B.r.w); Q->max_h = std::max(Q->max_h, B.r.h);
    }
    std::vector<ojphgpu_error_comp> ec;
    for (const CompGeo& g : P.comps) ec.push_back(ojphgpu_error_comp{ g.frame_off, (uint64_t)g.w * g.h, g.is_signed ? 1u : 0u, 0u });
    Q->h_err.assign(ec.size(), ojphgpu_frame_err{ 0, 0, 0 }); Q->best = Q->h_err;
    if (Q->recon.alloc((size_t)P.frame_elems * 4) || Q->descs.alloc(Q->h_descs.size() * sizeof(ojphgpu_requant_desc)) ||
        Q->comps.alloc(ec.size() * sizeof(ec[0])) || Q->err.alloc(ec.size() * sizeof(ojphgpu_frame_err)))
      return OJPHGPU_E_NOMEM;
    if (!ec.empty()) HIPCHK(hipMemcpy(Q->comps.p, ec.data(), ec.size() * sizeof(ec[0]), hipMemcpyHostToDevice));
    e->quality = Q; owner.p = nullptr;
    e->max_sse = max_sse; e->cap_bytes = 0; e->quality_on = true; e->ran = false;
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_encoder_set_quality_capped(ojphgpu_encoder* e, uint64_t max_sse, uint64_t cap_bytes)
{
  const int rc = ojphgpu_encoder_set_quality(e, max_sse);
  if (rc == OJPHGPU_OK) e->cap_bytes = cap_bytes;
  return rc;
}

// One trial of the search: SSE(j) of the frame of the last run.  The planes of the arena, requantised with the band
// parameters of j into the synthesis decoder's arena, go through the decoder's synthesis launches into the reconstructed
// frame (int32); the error sums against the frame `io` names, in its own container, come to the host: comps[component].
// No block is coded.  The descriptors and the sums travel the way `io` says: through mapped pinned memory and an event (a
// frame pipeline), or by copies from and into the encoder's pageable tables.
int ojphgpu_encoder_quality_trial(ojphgpu_encoder* e, const QualityTrialIo& io, uint32_t j, ojphgpu_frame_err* comps)
{
  EncoderRate& R = *e->rate; EncoderQuality& Q = *e->quality;
  hipStream_t s = e->stream;
  auto hip = [](hipError_t x) { return x == hipSuccess; };
  const uint32_t nc = R.table.nclasses;
  for (size_t i = 0; i < Q.h_descs.size(); ++i) {
    const BandQuant& q = R.table.quant[(size_t)j * nc + R.table.band_class[Q.desc_band[i]]];
    Q.h_descs[i].delta = q.delta; Q.h_descs[i].delta_inv = 1.0f / q.delta; Q.h_descs[i].K_max = q.K_max;   // (as rate_apply_step has them)
  }
  const size_t dbytes = Q.h_descs.size() * sizeof(ojphgpu_requant_desc), ebytes = Q.h_err.size() * sizeof(ojphgpu_frame_err);
  int rc;
  if (io.h_descs) {                                         // (the last trial that read them has been waited for)
    memcpy(io.h_descs, Q.h_descs.data(), dbytes);
    if ((rc = copy_to_host_launch(s, Q.descs.p, io.d_descs, dbytes)) != 0) return rc;   // the kernel copies either way
  } else if (dbytes && !hip(hipMemcpyAsync(Q.descs.p, Q.h_descs.data(), dbytes, hipMemcpyHostToDevice, s))) return OJPHGPU_E_HIP;
  rc = ojphgpu_band_requantise(s, (const ojphgpu_requant_desc*)Q.descs.p, (uint32_t)Q.h_descs.size(), Q.max_w, Q.max_h, e->arena.p, Q.syn->arena.p);
  if (rc) return rc;
  // (int32 whatever the run's container: a sample the reference leaves one past its range must not saturate, fit_container)
  if ((rc = decoder_synthesis_only(Q.syn, Q.recon.p, 32)) != 0) return rc;
  if (!hip(hipMemsetAsync(Q.err.p, 0, ebytes, s))) return OJPHGPU_E_HIP;
  rc = ojphgpu_frame_error_ex(s, io.frame, io.container, Q.recon.p, 32, (const ojphgpu_error_comp*)Q.comps.p, (uint32_t)Q.h_err.size(), (ojphgpu_frame_err*)Q.err.p);
  if (rc) return rc;
  const auto w0 = std::chrono::steady_clock::now();
  if (io.h_err) {
    if ((rc = copy_to_host_launch(s, io.d_err, Q.err.p, ebytes)) != 0) return rc;
    if (!hip(hipEventRecord(io.done, s)) || !hip(hipEventSynchronize(io.done))) return OJPHGPU_E_HIP;
    memcpy(comps, io.h_err, ebytes);
  } else if (!hip(hipMemcpyAsync(comps, Q.err.p, ebytes, hipMemcpyDeviceToHost, s)) || !hip(hipStreamSynchronize(s))) return OJPHGPU_E_HIP;
  Q.wait_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
  return OJPHGPU_OK;
}

// ... of a single encoder: against the caller's frame of the last run, through its own tables
static int64_t encoder_quality_trial(void* user, uint32_t j, uint64_t* sse)
{
  ojphgpu_encoder* e = (ojphgpu_encoder*)user;
  EncoderQuality& Q = *e->quality;
  const QualityTrialIo own{ Q.frame, Q.container, nullptr, nullptr, nullptr, nullptr, nullptr };
  const int rc = ojphgpu_encoder_quality_trial(e, own, j, Q.h_err.data());
  if (rc) return rc;
  uint64_t total = 0;
  for (const ojphgpu_frame_err& c : Q.h_err) total += c.sse;
  Q.by_index[j] = Q.h_err;
  *sse = total;
  return 0;
}

// the search of the last run, once: afterwards the device holds the coded blocks of j* and R.frame_plan[0] stands at its step
static int encoder_quality_search(ojphgpu_encoder* e)
{
  EncoderRate& R = *e->rate; EncoderQuality& Q = *e->quality;
  if (R.searched) return R.search_rc;
  const auto t0 = std::chrono::steady_clock::now();
  Q.wait_ms = 0; Q.final_ms = 0;
  auto run = [&]() -> int {
    if (!Q.frame) return OJPHGPU_E_INVALID;
    Q.by_index.assign(OJPHGPU_RATE_GRID, {});
    int rc = ojphgpu_quality_search(e->max_sse, encoder_quality_trial, e, &Q.info);
    Q.have_info = rc == OJPHGPU_OK || rc == OJPHGPU_E_QUALITY; Q.have_capped = false;
    Q.search_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc) return rc;
    Q.best = Q.by_index[Q.info.grid_index];
    for (const ojphgpu_frame_err& c : Q.best) Q.info.pae = std::max(Q.info.pae, c.pae);
    const auto t1 = std::chrono::steady_clock::now();
    // j* is block-coded, once, as a round of the byte budget's search codes its frame
    const RateTrialOut own{ e->out.p, (ojphgpu_cb_result*)e->results.p, (uint32_t*)e->counters.p, nullptr, nullptr, nullptr, nullptr };
    const ojphgpu_cb_result* lengths = nullptr;
    if ((rc = encoder_plans_at(e, { Q.info.grid_index })) != 0 || (rc = encoder_code_round(e, own, &Q.info.grid_index, &lengths)) != 0) return rc;
    const int64_t size = rate_layout_bytes(R.frame_plan[0]->plan, e->block_ids, lengths);
    Q.final_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
    if (size < 0) return size < INT32_MIN ? OJPHGPU_E_INVALID : (int)size;
    Q.info.bytes = (uint64_t)size;
    return OJPHGPU_OK;
  };
  R.search_rc = no_throw(run);
  R.searched = true;
  return R.search_rc;
}

// One size trial of the capped search: the frame's blocks coded at j into the encoder's own output, as a round of the byte
// budget's search codes them; R.frame_plan[0] is left at the step of j
static int64_t encoder_size_trial(void* user, uint32_t j)
{
  ojphgpu_encoder* e = (ojphgpu_encoder*)user;
  EncoderRate& R = *e->rate;
  const RateTrialOut own{ e->out.p, (ojphgpu_cb_result*)e->results.p, (uint32_t*)e->counters.p, nullptr, nullptr, nullptr, nullptr };
  const ojphgpu_cb_result* lengths = nullptr;
  int rc;
  if ((rc = encoder_plans_at(e, { j })) != 0 || (rc = encoder_code_round(e, own, &j, &lengths)) != 0) return rc;
  e->quality->coded_at = (int)j;
  return rate_layout_bytes(R.frame_plan[0]->plan, e->block_ids, lengths);
}

// The band statistics of the frame in the arena, for the model of the budget stepper: launched only when the cap binds.
// A failure leaves the search without a model (plain halving) and is reported when the search has ended.
static const uint32_t* encoder_capped_hist(void* user)
{
  ojphgpu_encoder* e = (ojphgpu_encoder*)user;
  EncoderRate& R = *e->rate;
  int& verdict = e->quality->hist_rc;
  hipStream_t s = e->stream;
  auto hip = [](hipError_t x) { return x == hipSuccess; };
  verdict = OJPHGPU_E_HIP;
  if (!hip(hipMemsetAsync(R.hist.p, 0, R.hist.n, s))) return nullptr;
  if ((verdict = ojphgpu_band_stats(s, (const ojphgpu_stats_desc*)R.stats_descs.p, R.n_stats, R.stats_max_w, R.stats_max_h, e->arena.p, (uint32_t*)R.hist.p)) != 0) return nullptr;
  verdict = OJPHGPU_E_HIP;
  if (!hip(hipMemcpyAsync(R.h_hist.data(), R.hist.p, R.h_hist.size() * 4, hipMemcpyDeviceToHost, s)) || !hip(hipStreamSynchronize(s))) return nullptr;
  verdict = OJPHGPU_OK;
  return R.h_hist.data();
}

// the capped search of the last run, once: afterwards the device holds the coded blocks of j* and R.frame_plan[0] stands at its step
static int encoder_capped_search(ojphgpu_encoder* e)
{
  EncoderRate& R = *e->rate; EncoderQuality& Q = *e->quality;
  if (R.searched) return R.search_rc;
  const auto t0 = std::chrono::steady_clock::now();
  Q.wait_ms = 0; Q.final_ms = 0; R.wait_ms = 0;
  auto run = [&]() -> int {
    if (!Q.frame) return OJPHGPU_E_INVALID;
    Q.by_index.assign(OJPHGPU_RATE_GRID, {});
    Q.coded_at = -1; Q.have_info = false; Q.hist_rc = OJPHGPU_OK;
    int rc = capped_search(R.table, e->max_sse, e->cap_bytes, -1, -1, encoder_quality_trial, encoder_size_trial, encoder_capped_hist, e, &Q.capped);
    Q.have_capped = !Q.hist_rc && (rc == OJPHGPU_OK || rc == OJPHGPU_E_BUDGET);
    if (Q.hist_rc) return Q.hist_rc;
    if (rc) return rc;
    ojphgpu_capped_info& I = Q.capped;
    if (Q.coded_at != (int)I.grid_index) {                   // the last coding was another index: j* once more, counted and checked
      const int64_t size = encoder_size_trial(e, I.grid_index);
      I.rate_passes++;
      if (size < 0) return size < INT32_MIN ? OJPHGPU_E_INVALID : (int)size;
      if ((uint64_t)size != I.bytes) return OJPHGPU_E_HIP;   // the same blocks at the same step: anything else is a fault
    }
    Q.best = Q.by_index[I.grid_index];
    if (Q.best.size() != Q.h_err.size()) return OJPHGPU_E_INVALID;
    for (const ojphgpu_frame_err& c : Q.best) I.pae = std::max(I.pae, c.pae);
    return OJPHGPU_OK;
  };
  R.search_rc = no_throw(run);
  R.searched = true;
  Q.search_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  Q.wait_ms += R.wait_ms;
  return R.search_rc;
}

extern "C" int ojphgpu_encoder_capped_info(ojphgpu_encoder* e, ojphgpu_capped_info* info)
{
  if (!e || !info || !e->quality || !e->quality_on || !e->cap_bytes || !e->quality->have_capped || !e->rate->searched) return OJPHGPU_E_INVALID;
  *info = e->quality->capped;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_encoder_quality_info(ojphgpu_encoder* e, ojphgpu_quality_info* info)
{
  if (!e || !info || !e->quality || e->cap_bytes || !e->quality->have_info) return OJPHGPU_E_INVALID;
  *info = e->quality->info;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_encoder_quality_comp(ojphgpu_encoder* e, uint32_t comp, uint64_t* sse, uint32_t* pae)
{
  if (!e || !sse || !pae || !e->quality || !(e->quality->have_info || e->quality->have_capped) || !e->rate->searched || e->rate->search_rc || comp >= e->quality->best.size())
    return OJPHGPU_E_INVALID;
  *sse = e->quality->best[comp].sse; *pae = e->quality->best[comp].pae;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_encoder_quality_timing(ojphgpu_encoder* e, float out[3])
{
  if (!e || !out || !e->quality || !e->rate->searched) return OJPHGPU_E_INVALID;
  out[0] = (float)e->quality->search_ms; out[1] = (float)e->quality->wait_ms; out[2] = (float)e->quality->final_ms;
  return OJPHGPU_OK;
}

static int encode_host(ojphgpu_encoder* e, const void* h_image, int container, uint8_t* h_out, size_t cap, size_t* out_len)
{
  if (!e || !h_image) return OJPHGPU_E_INVALID;
  const Plan& P = *e->P;
  const size_t bytes = (size_t)P.frame_elems * 4 * e->nframes;          // sized for the wider container, used by both
  if (!e->image.p && e->image.alloc(bytes)) return OJPHGPU_E_NOMEM;
  HIPCHK(hipMemcpyAsync(e->image.p, h_image, bytes / (32 / container), hipMemcpyHostToDevice, e->stream));
  int rc = ojphgpu_encoder_run_container(e, e->image.p, container);
  if (rc) return rc;
  return ojphgpu_encoder_finish(e, h_out, cap, out_len);
}

extern "C" int ojphgpu_encode(ojphgpu_encoder* e, const int32_t* h_image, uint8_t* h_out, size_t cap, size_t* out_len)
{
  return encode_host(e, h_image, 32, h_out, cap, out_len);
}

extern "C" int ojphgpu_encode16(ojphgpu_encoder* e, const uint16_t* h_image, uint8_t* h_out, size_t cap, size_t* out_len)
{
  return encode_host(e, h_image, 16, h_out, cap, out_len);
}

extern "C" int ojphgpu_encoder_timing(ojphgpu_encoder* e, float out[4])
{
  if (!e || !out || !e->ran) return OJPHGPU_E_INVALID;
  if (encoder_settle(e)) return OJPHGPU_E_HIP;              // (a released run: its total ends with the later of its two branches)
  if (e->timer.read(SP_CONVERT, &out[0]) || e->timer.read(SP_DWT, &out[1]) || e->timer.read(SP_HT_ENC, &out[2]) ||
      e->timer.read(-1, &out[3])) return OJPHGPU_E_HIP;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_encoder_ht_timing(ojphgpu_encoder* e, float* out, uint32_t cap, uint32_t* n, uint32_t* n_top)
{
  if (!e || !out || !n || !e->ran) return OJPHGPU_E_INVALID;
  if (encoder_settle(e)) return OJPHGPU_E_HIP;
  int k = e->timer.read_each(SP_HT_ENC, out, cap);
  if (k < 0) return OJPHGPU_E_HIP;
  *n = (uint32_t)k;
  if (n_top) *n_top = e->n_top;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_encoder_level_timing(ojphgpu_encoder* e, float* out, uint32_t cap, uint32_t* n)
{
  if (!e || !out || !n || !e->ran) return OJPHGPU_E_INVALID;
  if (encoder_settle(e)) return OJPHGPU_E_HIP;
  int k = e->timer.read_each(SP_DWT, out, cap);
  if (k < 0) return OJPHGPU_E_HIP;
  *n = (uint32_t)k;
  return OJPHGPU_OK;
}

// ---------------------------------------------------------------------------------------------
extern "C" void ojphgpu_decoder_destroy(ojphgpu_decoder* d)
{
  if (!d) return;
  (void)hipSetDevice(d->device);
  // a released run may still be decoding, an upload still copying, on the object's own stream: nothing is freed under them
  if (d->can_release && d->side) (void)hipStreamSynchronize(d->side);
  d->pending = false;
  for (DeviceBuf* b : { &d->arena, &d->arena2, &d->image, &d->dwt_descs, &d->img_descs, &d->cb_descs, &d->conv_descs, &d->data, &d->status, &d->quads,
                       &d->aux, &d->fstate, &d->dwt_regs, &d->img_regs })
    b->release();
  for (hipEvent_t ev : { d->ev_done, d->ev_up, d->ev_read, d->ev_read2 }) if (ev) (void)hipEventDestroy(ev);
  if (d->h_retry) (void)hipHostFree(d->h_retry);
  if (d->h_stage) (void)hipHostFree(d->h_stage);
  if (d->ev_stage) (void)hipEventDestroy(d->ev_stage);
  if (d->side) (void)hipStreamDestroy(d->side);
  if (d->ev_fork) (void)hipEventDestroy(d->ev_fork);
  if (d->ev_join) (void)hipEventDestroy(d->ev_join);
  d->timer.destroy();
  delete d;
}

extern "C" int ojphgpu_decoder_create(const ojphgpu_plan* plan, int device, void* stream, ojphgpu_decoder** out)
{
  if (!plan) return OJPHGPU_E_INVALID;
  return ojphgpu_decoder_create_tiles(plan, device, stream, 0, (uint32_t)plan->plan.tiles.size(), out);
}

// blocks_only: the decoder half of a transcoder (section 5d) -- the block decoder alone: no level batches, no conversion
static int decoder_create(const ojphgpu_plan* const* plans, uint32_t nframes, int device, void* stream, uint32_t tile_first,
                          uint32_t tile_count, ojphgpu_decoder** out, bool blocks_only = false, bool may_release = false);

extern "C" int ojphgpu_decoder_create_tiles(const ojphgpu_plan* plan, int device, void* stream, uint32_t tile_first,
                                             uint32_t tile_count, ojphgpu_decoder** out)
{
  return no_throw([&] { return decoder_create(&plan, 1, device, stream, tile_first, tile_count, out, false, true); });
}

// the decoder of a frame pipe or of a multi-device decoder: its runs never release (ojphgpu_objects.h)
int ojphgpu_decoder_create_joined(const ojphgpu_plan* plan, int device, void* stream, uint32_t tile_first, uint32_t tile_count, ojphgpu_decoder** out)
{
  if (!plan) return OJPHGPU_E_INVALID;
  return no_throw([&] { return decoder_create(&plan, 1, device, stream, tile_first, tile_count, out); });
}

extern "C" int ojphgpu_decoder_create_batch(const ojphgpu_plan* const* plans, uint32_t num_frames, int device, void* stream,
                                             ojphgpu_decoder** out)
{
  if (!plans || num_frames == 0 || !plans[0]) return OJPHGPU_E_INVALID;
  return no_throw([&] { return decoder_create(plans, num_frames, device, stream, 0, (uint32_t)plans[0]->plan.tiles.size(), out); });
}

// Two parsed codestreams describe frames one decoder object can take turns on: same frame format, same
// place for every code-block.  Quantisation may differ (K_max / delta are per frame).
int ojphgpu_same_frame_geometry(const Plan& P, const Plan& Q, bool compare_blocks)
{
  if (Q.coded.size() != Q.blocks.size()) return OJPHGPU_E_INVALID;    // plans must come from ojphgpu_t2_parse
  if (Q.skip_read != P.skip_read || Q.skip_recon != P.skip_recon) return OJPHGPU_E_INVALID;
  if (Q.has_region != P.has_region || memcmp(Q.region, P.region, sizeof(P.region)) != 0) return OJPHGPU_E_INVALID;   // one region
  if (Q.blocks.size() != P.blocks.size() || Q.arena_elems != P.arena_elems || Q.p.width != P.p.width ||
      Q.p.height != P.p.height || Q.p.num_comps != P.p.num_comps || Q.p.bit_depth != P.p.bit_depth ||
      Q.p.is_signed != P.p.is_signed || Q.p.reversible != P.p.reversible || Q.p.num_decomps != P.p.num_decomps ||
      Q.p.color_transform != P.p.color_transform || Q.p.tile_w != P.p.tile_w || Q.p.tile_h != P.p.tile_h ||
      Q.p.block_w != P.p.block_w || Q.p.block_h != P.p.block_h ||
      Q.p.image_x0 != P.p.image_x0 || Q.p.image_y0 != P.p.image_y0 || Q.p.tile_x0 != P.p.tile_x0 || Q.p.tile_y0 != P.p.tile_y0 ||
      memcmp(Q.p.comp_dx, P.p.comp_dx, sizeof(P.p.comp_dx)) != 0 || memcmp(Q.p.comp_dy, P.p.comp_dy, sizeof(P.p.comp_dy)) != 0 ||
      memcmp(Q.p.comp_depth, P.p.comp_depth, sizeof(P.p.comp_depth)) != 0 || memcmp(Q.p.comp_sign, P.p.comp_sign, sizeof(P.p.comp_sign)) != 0 ||
      Q.nlt3 != P.nlt3 || Q.wide != P.wide || Q.bands.size() != P.bands.size() || memcmp(Q.p.coc, P.p.coc, sizeof(P.p.coc)) != 0)
    return OJPHGPU_E_INVALID;
  if (!compare_blocks) return OJPHGPU_OK;
  // the launches are laid out from the first frame's geometry: every block must sit where that frame has it
  // (precinct sizes move the code-block grid)
  for (size_t i = 0; i < P.blocks.size(); ++i) {
    const Block& a = P.blocks[i]; const Block& b = Q.blocks[i];
    if (a.band != b.band || a.r.x0 != b.r.x0 || a.r.y0 != b.r.y0 || a.r.w != b.r.w || a.r.h != b.r.h) return OJPHGPU_E_INVALID;
  }
  for (size_t i = 0; i < P.bands.size(); ++i)
    if (P.bands[i].plane_off != Q.bands[i].plane_off || P.bands[i].pitch != Q.bands[i].pitch) return OJPHGPU_E_INVALID;
  return OJPHGPU_OK;
}

// Block descriptors of one frame: geometry from P (the decoder's plan), what the packet headers and the
// QCD / QCC of THIS frame's codestream say from Q.  arena_off = element offset of the frame's arena,
// data_base = where the frame's byte range [fi.first, fi.first + fi.len) of the codestream will sit in the
// device data buffer.  scratch_cap / reserved are left to ojphgpu_ht_decode_layout.  want_runs: the frame's bytes as runs
// (fi.runs) also for a plan without a region -- one restricted in resolution under PCRL / CPRL has the skipped resolutions'
// blocks between the others all over the codestream; a region plan always gets runs.
void ojphgpu_decoder_fill_descs(const Plan& P, const Plan& Q, const std::vector<uint32_t>& ids, uint64_t arena_off,
                                uint64_t data_base, ojphgpu_cb_desc* bd, DecFrameInfo& fi, bool want_runs)
{
  uint64_t max_off = 0, min_off = ~0ull;
  fi.any_refine = false; fi.max_len1 = 0; fi.kinds = 0; fi.pads.clear(); fi.pad_len = 0;
  // blocks whose tile-part ended before their bytes did: the reference decodes what there is with zeros behind it
  // (bb_read_chunk, ojph_bitbuffer_read.h:134-150).  `coded` calls them not coded; here they get what the packet header
  // said and a place of their own behind the uploaded byte range (PadCopy), where the upload puts bytes + zeros.
  std::vector<std::pair<uint32_t, const Plan::PaddedBlock*>> padded_idx;   // by block id, first entry of an id wins (as a linear search would)
  padded_idx.reserve(Q.padded.size());
  for (const Plan::PaddedBlock& pb : Q.padded) padded_idx.emplace_back(pb.block, &pb);
  std::stable_sort(padded_idx.begin(), padded_idx.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
  auto padded_of = [&](uint32_t id) -> const Plan::PaddedBlock* {
    auto it = std::lower_bound(padded_idx.begin(), padded_idx.end(), id, [](const auto& a, uint32_t v) { return a.first < v; });
    return it != padded_idx.end() && it->first == id ? it->second : nullptr;
  };
  std::vector<std::pair<size_t, const Plan::PaddedBlock*>> padded_at;
  for (size_t i = 0; i < ids.size(); ++i) {
    const Block& k = P.blocks[ids[i]]; const Band& B = Q.bands[k.band];
    const Plan::PaddedBlock* pb = Q.padded.empty() ? nullptr : padded_of(ids[i]);
    const CodedBlock& c = pb ? pb->hdr : Q.coded[ids[i]];   // this frame's own K_max / delta
    if (pb) padded_at.emplace_back(i, pb);
    ojphgpu_cb_desc& o = bd[i]; memset(&o, 0, sizeof(o));
    const bool wide = is_wide(Q, B.comp);                  // (same_frame_geometry: the same components as in P)
    o.coef_off = arena_off + P.bands[k.band].plane_off + ((uint64_t)k.r.y0 * B.pitch + k.r.x0) * (wide ? 2u : 1u); o.pitch = B.pitch;
    o.w = (uint16_t)k.r.w; o.h = (uint16_t)k.r.h; o.K_max = (uint8_t)B.K_max;
    o.reversible = (uint8_t)((Q.style(B.comp).rev ? 1u : 0u) | (Q.style(B.comp).causal ? 2u : 0u) | (wide ? 4u : 0u));   // bit 1: vertically causal, bit 2: 64-bit samples
    o.missing_msbs = (uint8_t)std::min<uint32_t>(c.missing_msbs, 255); o.num_passes = (uint8_t)c.num_passes;
    o.delta = B.delta; o.len1 = c.len1; o.len2 = c.len2; o.data_off = c.offset;
    fi.kinds |= ojphgpu::ht_decode_block_kinds(k.r.w, o.reversible, c.num_passes, c.len2);   // (ht_tables.h)
    if (fi.kinds & 16) fi.any_refine = true;
    fi.max_len1 = std::max(fi.max_len1, c.len1);
    if ((c.len1 + c.len2) && !pb) {
      max_off = std::max<uint64_t>(max_off, c.offset + c.len1 + c.len2);
      min_off = std::min<uint64_t>(min_off, c.offset);
    }
  }
  if (min_off > max_off) min_off = max_off = 0;
  min_off &= ~(uint64_t)15;                                             // only this byte range of the codestream is uploaded
  fi.runs.clear();
  if (P.has_region || want_runs) {
    // a region decoder's blocks are scattered over the codestream (progression orders interleave them): the runs of blocks
    // adjacent in the codestream are placed one after another, 64 zero bytes on either side of each
    std::vector<std::pair<uint64_t, uint64_t>> spans;                    // (offset, end) of every block with bytes here
    for (size_t i = 0; i < ids.size(); ++i) {
      const ojphgpu_cb_desc& o = bd[i];
      if ((o.len1 + o.len2) && (padded_at.empty() || std::none_of(padded_at.begin(), padded_at.end(), [&](const auto& pp) { return pp.first == i; })))
        spans.emplace_back(o.data_off, o.data_off + o.len1 + o.len2);
    }
    std::sort(spans.begin(), spans.end());
    uint64_t at = 0;
    for (const auto& sp : spans) {
      if (!fi.runs.empty() && sp.first <= fi.runs.back().src + fi.runs.back().n) {
        DecRun& r = fi.runs.back();
        r.n = std::max(r.n, sp.second - r.src);
        continue;
      }
      if (!fi.runs.empty()) at = ((fi.runs.back().dst + fi.runs.back().n + 63) & ~(uint64_t)63);
      at += 64;
      fi.runs.push_back(DecRun{ sp.first, at, sp.second - sp.first });
    }
    const uint64_t staged = fi.runs.empty() ? 0 : ((fi.runs.back().dst + fi.runs.back().n + 63) & ~(uint64_t)63) + 64;
    for (size_t i = 0; i < ids.size(); ++i) {
      ojphgpu_cb_desc& o = bd[i];
      if (!(o.len1 + o.len2)) { o.data_off = 0; continue; }
      auto it = std::upper_bound(fi.runs.begin(), fi.runs.end(), o.data_off, [](uint64_t v, const DecRun& r) { return v < r.src; });
      if (it != fi.runs.begin()) { --it; o.data_off = data_base + it->dst + (o.data_off - it->src); }
    }
    fi.first = 0; fi.len = staged;
  } else {
    for (size_t i = 0; i < ids.size(); ++i) {
      ojphgpu_cb_desc& o = bd[i];
      if (o.len1 + o.len2) o.data_off = o.data_off - min_off + data_base; else o.data_off = 0;
    }
    fi.first = min_off; fi.len = max_off - min_off;
  }
  uint64_t at = (fi.len + 63) & ~(uint64_t)63;                          // padded blocks: behind the range, 64 bytes apart at least
  for (const auto& pp : padded_at) {
    ojphgpu_cb_desc& o = bd[pp.first]; const Plan::PaddedBlock& pb = *pp.second;
    const uint32_t total = pb.hdr.len1 + pb.hdr.len2;
    if (total == 0) continue;
    at += 64;                                                           // (room below the block: the VLC partner's 16-byte loads)
    fi.pads.push_back(PadCopy{ pb.hdr.offset, at, std::min(pb.got, total), total });
    o.data_off = data_base + at;
    at = (at + total + 63) & ~(uint64_t)63;
  }
  if (!fi.pads.empty()) at += 64;                                       // (ojphgpu_decoder_upload_pads zeroes a 64-byte margin behind the last block too)
  fi.pad_len = at - ((fi.len + 63) & ~(uint64_t)63);
}

extern "C" int ojphgpu_plan_upload_runs(const ojphgpu_plan* plan, ojphgpu_run* out, size_t cap, size_t* count, uint64_t* staged_len)
{
  if (!plan || !count || !staged_len) return OJPHGPU_E_INVALID;
  const Plan& P = plan->plan;
  if (P.coded.size() != P.blocks.size()) return OJPHGPU_E_INVALID;    // a parsed codestream only
  return no_throw([&]() -> int {
    const std::vector<uint32_t> ids = blocks_of_tiles(P, TileRange{ 0, (uint32_t)P.tiles.size() });
    std::vector<ojphgpu_cb_desc> bd(ids.size());
    DecFrameInfo fi;
    ojphgpu_decoder_fill_descs(P, P, ids, 0, 0, bd.data(), fi, true);
    *count = fi.runs.size(); *staged_len = fi.len;
    if (!out) return OJPHGPU_OK;
    if (cap < fi.runs.size()) return OJPHGPU_E_OVERFLOW;
    for (size_t i = 0; i < fi.runs.size(); ++i) out[i] = ojphgpu_run{ fi.runs[i].src, fi.runs[i].dst, fi.runs[i].n };
    return OJPHGPU_OK;
  });
}

int ojphgpu_decoder_upload_pads(hipStream_t s, uint8_t* d_frame_data, const uint8_t* h_codestream, size_t cs_len, const std::vector<PadCopy>& pads)
{
  for (const PadCopy& c : pads) {
    if (c.src + c.got > cs_len) return OJPHGPU_E_INVALID;
    HIPCHK(hipMemsetAsync(d_frame_data + c.dst - 64, 0, (size_t)c.total + 128, s));     // zeros: the padding, and a margin either side
    if (c.got) HIPCHK(hipMemcpyAsync(d_frame_data + c.dst, h_codestream + c.src, c.got, hipMemcpyHostToDevice, s));
  }
  return OJPHGPU_OK;
}

static int decoder_create(const ojphgpu_plan* const* plans, uint32_t nframes, int device, void* stream, uint32_t tile_first,
                          uint32_t tile_count, ojphgpu_decoder** out, bool blocks_only, bool may_release)
{
  if (!plans || !plans[0] || !out || nframes == 0) return OJPHGPU_E_INVALID;
  *out = nullptr;
  const ojphgpu_plan* plan = plans[0];
  const Plan& P = plan->plan;
  if ((uint64_t)tile_first + tile_count > P.tiles.size()) return OJPHGPU_E_INVALID;
  if (P.has_region && (tile_first != 0 || tile_count != P.tiles.size())) return OJPHGPU_E_INVALID;   // a region decoder decodes whole frames
  for (uint32_t f = 0; f < nframes; ++f) {                              // every frame of a batch has the same geometry
    if (!plans[f]) return OJPHGPU_E_INVALID;
    const int rc = ojphgpu_same_frame_geometry(P, plans[f]->plan, f != 0);
    if (rc) return rc;
  }
  HIPCHK(hipSetDevice(device));
  if (ensure_tables() != 0) return OJPHGPU_E_HIP;
  ojphgpu_decoder* d = new (std::nothrow) ojphgpu_decoder();
  if (!d) return OJPHGPU_E_NOMEM;
  struct Owner { ojphgpu_decoder* p; ~Owner() { if (p) ojphgpu_decoder_destroy(p); } } owner{ d };   // also when a container throws
  d->P = &P; d->device = device; d->stream = (hipStream_t)stream;
  d->cus = ojphgpu::device_cus(device);
  auto bail = [&](int rc) { return rc; };

  d->tiles = TileRange{ tile_first, tile_count };
  d->nframes = nframes;
  const TileRange tr = d->tiles;
  const uint64_t frame_elems = P.frame_elems;
  d->blocks_only = blocks_only;
  std::vector<ojphgpu_dwt_desc> dd, idd;
  if (!blocks_only) {
    build_level_batches(P, tr, dd, d->batches);
    build_image_level_descs(P, tr, dd, d->batches, idd);
  }
  std::vector<ojphgpu_dwt_region> rg, irg;
  d->region = P.has_region;
  if (d->region) {                                          // region synthesis: the levels the region needs, each with its exact range
    restrict_levels_to_region(P, tr, dd, idd, d->batches, rg, irg);
    replicate_regions(rg, irg, d->batches, nframes, frame_elems);
  }
  replicate_levels(dd, idd, d->batches, nframes, P.arena_elems, frame_elems);
  std::reverse(d->batches.begin(), d->batches.end());                 // synthesis: lowest resolution first
  std::vector<ojphgpu_convert_desc> cd;
  if (!blocks_only) d->need_convert = build_convert_descs(P, tr, cd, d->conv_max_w, d->conv_max_h);
  d->conv_tiles = tile_count; d->tiles_touched = tile_count;
  if (d->region) {
    d->conv_tiles = d->tiles_touched = restrict_converts_to_region(P, tr, cd, d->conv_max_w, d->conv_max_h);
    d->need_convert = d->need_convert && d->conv_max_w && d->conv_max_h;
  }
  replicate_converts(cd, nframes, P.arena_elems, P.frame_elems);
  std::vector<uint32_t> ids = blocks_of_tiles(P, tr);
  // Overlap of the lower synthesis levels with the block decoder: the blocks below the top
  // resolution come first in descriptor order; once step 2 has produced them, the small, latency-bound
  // launches of levels L .. 2 run on a second stream while step 2 works through the top resolution's
  // blocks (3/4 of the samples) on the main one.  Prep and step 1 stay single launches over all blocks:
  // step 1 costs one serial chain however few blocks it is given, splitting it would pay that twice
  // (measured: 0.96 vs 0.91 ms at 8K with every stage split in two).
  if (nframes == 1 && max_recon_decomps(P) >= 2 && d->batches.size() >= 2 && d->batches.front().depth > 0 && !P.any_wide &&
      getenv("OJPHGPU_NO_OVERLAP") == nullptr) {
    auto low = [&](uint32_t id) { const Band& B = P.bands[P.blocks[id].band]; return B.res < P.recon_decomps(B.comp); };
    auto mid = std::stable_partition(ids.begin(), ids.end(), low);
    d->n_low = (uint32_t)(mid - ids.begin());
    int prio_lo = 0, prio_hi = 0;                         // the short launches of the side stream go first at the dispatcher
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    int prio = prio_hi;
    // (a decoder that may release runs its block launch there too: OJPHGPU_DEC_AHEAD_PRIO, read once, here)
    const char* ahead_prio = may_release && !blocks_only && !P.has_region ? getenv("OJPHGPU_DEC_AHEAD_PRIO") : nullptr;
    if (ahead_prio && !strcmp(ahead_prio, "low")) prio = prio_lo;
    else if (ahead_prio && !strcmp(ahead_prio, "normal")) prio = (prio_lo + prio_hi) / 2;
    if (d->n_low == 0 || d->n_low == ids.size()) d->n_low = 0;
    else if (hipStreamCreateWithPriority(&d->side, hipStreamNonBlocking, prio) != hipSuccess ||
             hipEventCreateWithFlags(&d->ev_fork, hipEventDisableTiming) != hipSuccess ||
             hipEventCreateWithFlags(&d->ev_join, hipEventDisableTiming) != hipSuccess) return bail(OJPHGPU_E_HIP);
  }
  d->block_ids = ids;
  d->nblocks = (uint32_t)(ids.size() * nframes);
  std::vector<ojphgpu_cb_desc> bd(ids.size() * nframes);
  uint64_t nquads = 0, naux = 0, data_total = 0;
  d->f_first.assign(nframes, 0); d->f_len.assign(nframes, 0); d->f_base.assign(nframes, 0); d->f_pads.assign(nframes, {});
  d->f_runs.assign(nframes, {});
  for (uint32_t f = 0; f < nframes; ++f) {
    DecFrameInfo fi;
    ojphgpu_decoder_fill_descs(P, plans[f]->plan, ids, (uint64_t)f * P.arena_elems, data_total, bd.data() + (size_t)f * ids.size(), fi);
    d->any_refine |= fi.any_refine; d->kinds |= fi.kinds; d->max_len1 = std::max(d->max_len1, fi.max_len1);
    d->f_first[f] = (size_t)fi.first; d->f_len[f] = (size_t)fi.len; d->f_base[f] = (size_t)data_total;
    d->f_pads[f] = fi.pads;
    d->f_runs[f] = fi.runs;
    d->stage_cap = std::max(d->stage_cap, (size_t)fi.len);
    data_total += fi.data_bytes();
  }
  d->data_first = d->f_first[0];
  d->data_len = (size_t)data_total;
  // scratch of step 1's records and of the flat VLC / MEL strings (prep and step 1 are single launches
  // over all descriptors)
  if (ojphgpu_ht_decode_layout(bd.data(), (uint32_t)bd.size(), &nquads, &naux) != OJPHGPU_OK) return bail(OJPHGPU_E_INVALID);
  if (nquads >= 0xFFFFFFFFull || naux >= 0xFFFFFFFFull) return bail(OJPHGPU_E_INVALID);
  if (d->quads.alloc((size_t)nquads * 4 + 64) || d->aux.alloc((size_t)naux * 4 + 64)) return bail(OJPHGPU_E_NOMEM);
  for (const ojphgpu_cb_desc& b : bd) d->max_block_h = std::max<uint32_t>(d->max_block_h, b.h);
  if (ojphgpu::dec_fuses()) {                              // flags and per-block state of the fused step 1 + step 2 launch
    const size_t fw = (size_t)ojphgpu::ht_decode_fused_state_words((uint32_t)bd.size());
    if (d->fstate.alloc(fw * 4)) return bail(OJPHGPU_E_NOMEM);
    if (hipMemset(d->fstate.p, 0, fw * 4) != hipSuccess) return bail(OJPHGPU_E_HIP);
    // (a word the launch can reach in host memory: see ojphgpu_decoder::h_retry; without it the notice is simply not given)
    void* hp = nullptr; void* dp = nullptr;
    if (hipHostMalloc(&hp, 64, hipHostMallocMapped) == hipSuccess && hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) {
      d->h_retry = (uint32_t*)hp; d->d_h_retry = (uint32_t*)dp; *d->h_retry = 0;
    } else { (void)hipGetLastError(); if (hp) (void)hipHostFree(hp); }
  }
  if (d->arena.alloc(P.arena_elems * 4 * nframes) || d->dwt_descs.alloc(dd.size() * sizeof(dd[0])) ||
      d->img_descs.alloc(idd.size() * sizeof(dd[0])) || d->cb_descs.alloc(bd.size() * sizeof(bd[0])) || d->conv_descs.alloc(cd.size() * sizeof(cd[0])) ||
      d->data.alloc(d->data_len + 128) || d->status.alloc(bd.size() + 16))
    return bail(OJPHGPU_E_NOMEM);
  if (hipMemset(d->status.p, 0, bd.size() + 16) != hipSuccess) return bail(OJPHGPU_E_HIP);      // (the RETRY word behind the status bytes)
  if (hipMemset(d->arena.p, 0, P.arena_elems * 4 * nframes) != hipSuccess) return bail(OJPHGPU_E_HIP);
  if (!dd.empty() && hipMemcpy(d->dwt_descs.p, dd.data(), dd.size() * sizeof(dd[0]), hipMemcpyHostToDevice) != hipSuccess) return bail(OJPHGPU_E_HIP);
  if (!idd.empty() && hipMemcpy(d->img_descs.p, idd.data(), idd.size() * sizeof(idd[0]), hipMemcpyHostToDevice) != hipSuccess) return bail(OJPHGPU_E_HIP);
  if (!bd.empty() && hipMemcpy(d->cb_descs.p, bd.data(), bd.size() * sizeof(bd[0]), hipMemcpyHostToDevice) != hipSuccess) return bail(OJPHGPU_E_HIP);
  if (!cd.empty() && hipMemcpy(d->conv_descs.p, cd.data(), cd.size() * sizeof(cd[0]), hipMemcpyHostToDevice) != hipSuccess) return bail(OJPHGPU_E_HIP);
  if (d->region) {
    if (d->dwt_regs.alloc(rg.size() * sizeof(ojphgpu_dwt_region)) || d->img_regs.alloc(irg.size() * sizeof(ojphgpu_dwt_region))) return bail(OJPHGPU_E_NOMEM);
    if (!rg.empty() && hipMemcpy(d->dwt_regs.p, rg.data(), rg.size() * sizeof(rg[0]), hipMemcpyHostToDevice) != hipSuccess) return bail(OJPHGPU_E_HIP);
    if (!irg.empty() && hipMemcpy(d->img_regs.p, irg.data(), irg.size() * sizeof(irg[0]), hipMemcpyHostToDevice) != hipSuccess) return bail(OJPHGPU_E_HIP);
    void* hp = nullptr;                                     // the staging buffer of the uploads
    if (d->stage_cap && hipHostMalloc(&hp, d->stage_cap, hipHostMallocDefault) != hipSuccess) return bail(OJPHGPU_E_NOMEM);
    d->h_stage = (uint8_t*)hp;
    if (hipEventCreateWithFlags(&d->ev_stage, hipEventDisableTiming) != hipSuccess) return bail(OJPHGPU_E_HIP);
  }
  if (d->timer.init() != 0) return bail(OJPHGPU_E_HIP);
  // Released runs (ojphgpu_objects.h): only an object that would release its next run as it stands -- the switches are read
  // once, here -- holds the events, takes its uploads on its own stream and, unless OJPHGPU_DEC_SETS=1, a second arena
  const char* rel = getenv("OJPHGPU_DEC_RELEASE"); const char* sets = getenv("OJPHGPU_DEC_SETS"); const char* lv = getenv("OJPHGPU_DEC_AHEAD_LEVELS");
  d->can_release = may_release && !(rel && !strcmp(rel, "0")) && getenv("OJPHGPU_NO_OVERLAP") == nullptr &&
                   tile_first == 0 && tile_count == P.tiles.size();   // (a tile range is one worker's share of a frame: collected on the spot)
  d->timer.detail = false;
  d->can_release = d->can_release && decoder_releases(d);
  d->timer.detail = true;
  if (d->can_release) {
    d->ahead_levels = lv && !strcmp(lv, "1");               // (measured: the block launch alone wins)
    d->two_arenas = !(sets && !strcmp(sets, "1"));
    for (hipEvent_t* ev : { &d->ev_done, &d->ev_up, &d->ev_read, &d->ev_read2 })
      if (hipEventCreateWithFlags(ev, hipEventDisableTiming) != hipSuccess) return bail(OJPHGPU_E_HIP);
    if (d->two_arenas) {                                    // the second arena, exactly as the first
      if (d->arena2.alloc(P.arena_elems * 4)) return bail(OJPHGPU_E_NOMEM);
      if (hipMemset(d->arena2.p, 0, P.arena_elems * 4) != hipSuccess) return bail(OJPHGPU_E_HIP);
    }
  }
  owner.p = nullptr;
  *out = d;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_decoder_upload(ojphgpu_decoder* d, const uint8_t* h_codestream, size_t len)
{
  return ojphgpu_decoder_upload_frame(d, 0, h_codestream, len);
}

extern "C" int ojphgpu_decoder_upload_frame(ojphgpu_decoder* d, uint32_t frame, const uint8_t* h_codestream, size_t len)
{
  if (!d || !h_codestream || frame >= d->nframes) return OJPHGPU_E_INVALID;
  if (d->region) {                                          // the runs of the decoded blocks, gathered, then one copy
    const std::vector<DecRun>& runs = d->f_runs[frame];
    for (const DecRun& r : runs) if (r.src + r.n > len) return OJPHGPU_E_INVALID;
    if (d->f_len[frame]) {
      if (d->ev_stage) HIPCHK(hipEventSynchronize(d->ev_stage));   // the copy of the previous upload has left the staging buffer
      uint8_t* st = d->h_stage;
      uint64_t at = 0;
      for (const DecRun& r : runs) {
        memset(st + at, 0, r.dst - at);
        memcpy(st + r.dst, h_codestream + r.src, r.n);
        at = r.dst + r.n;
      }
      memset(st + at, 0, d->f_len[frame] - at);
      HIPCHK(hipMemcpyAsync((uint8_t*)d->data.p + d->f_base[frame], st, d->f_len[frame], hipMemcpyHostToDevice, d->stream));
      HIPCHK(hipEventRecord(d->ev_stage, d->stream));
    }
    return ojphgpu_decoder_upload_pads(d->stream, (uint8_t*)d->data.p + d->f_base[frame], h_codestream, len, d->f_pads[frame]);
  }
  if (len < d->f_first[frame] + d->f_len[frame]) return OJPHGPU_E_INVALID;
  // A decoder that can release copies on its own stream: in order behind the last block launch that read `data` (a joined
  // run's sits on the caller's stream: decoder_own_follows_joined) and in front of the next one, beside whatever the
  // caller's stream still holds.  The caller's stream follows (ev_up), so a caller that synchronises it may reuse the
  // host buffer, and a joined run reads the new bytes.
  hipStream_t us = d->stream;
  if (d->can_release) {
    int rc = decoder_own_follows_joined(d);
    if (rc) return rc;
    us = d->side;
  }
  if (d->f_len[frame])
    HIPCHK(hipMemcpyAsync((uint8_t*)d->data.p + d->f_base[frame], h_codestream + d->f_first[frame], d->f_len[frame],
                          hipMemcpyHostToDevice, us));
  const int rc = ojphgpu_decoder_upload_pads(us, (uint8_t*)d->data.p + d->f_base[frame], h_codestream, len, d->f_pads[frame]);
  if (d->can_release) {                                     // (also behind a copy that failed half way)
    HIPCHK(hipEventRecord(d->ev_up, d->side));
    HIPCHK(hipStreamWaitEvent(d->stream, d->ev_up, 0));
  }
  return rc;
}

// prep + step 1 of every block (one launch each: step 1 costs one serial chain however few blocks it gets)
static int decode_chains(ojphgpu_decoder* d, hipStream_t s)
{
  if (d->nblocks == 0 || (d->kinds & 3) == 0) return OJPHGPU_OK;     // (nothing but blocks of the 64-bit sample path: decode_samples)
  Spans& T = d->timer;
  const ojphgpu_cb_desc* cbd = (const ojphgpu_cb_desc*)(d->o_cb_descs ? d->o_cb_descs : d->cb_descs.p);
  uint8_t* status = (uint8_t*)(d->o_status ? d->o_status : d->status.p);
  const uint8_t* data = (const uint8_t*)(d->o_data ? d->o_data : d->data.p);
  int sp = T.begin(SP_PREP, s);
  int rc = ojphgpu_ht_decode_prep(s, cbd, d->nblocks, data, (uint32_t*)d->aux.p);
  if (rc) return rc;
  T.end(sp, s);
  sp = T.begin(SP_STEP1, s);
  rc = ojphgpu_ht_decode_step1(s, cbd, d->nblocks, data, (const uint32_t*)d->aux.p, (uint32_t*)d->quads.p, status);
  if (rc) return rc;
  T.end(sp, s);
  return OJPHGPU_OK;
}

// step 2 (+ the refinement passes) over descriptors [first, first + count) on stream s
static int decode_samples(ojphgpu_decoder* d, hipStream_t s, uint32_t first, uint32_t count)
{
  if (count == 0) return OJPHGPU_OK;
  Spans& T = d->timer;
  const ojphgpu_cb_desc* cbd = (const ojphgpu_cb_desc*)(d->o_cb_descs ? d->o_cb_descs : d->cb_descs.p) + first;
  uint8_t* status = (uint8_t*)(d->o_status ? d->o_status : d->status.p) + first;
  const uint8_t* data = (const uint8_t*)(d->o_data ? d->o_data : d->data.p);
  int sp = T.begin(SP_STEP2, s);
  int rc = (d->kinds & 3) ? ojphgpu::ht_decode_step2_launch(s, cbd, count, data, (const uint32_t*)d->quads.p, d->arena.p, status, d->kinds & ~32) : OJPHGPU_OK;
  if (rc) return rc;
  if (d->kinds & 32) {                                      // the blocks on the 64-bit sample path: all their launches (the others skip them)
    rc = ojphgpu::ht_decode64_launch(s, cbd, count, data, (uint32_t*)d->aux.p, (uint32_t*)d->quads.p, d->arena.p, status, d->any_refine ? 1 : 0);
    if (rc) return rc;
  }
  T.end(sp, s);
  if (d->any_refine && (d->kinds & 3)) {
    sp = T.begin(SP_REFINE, s);
    rc = ojphgpu_ht_decode_refine(s, cbd, count, data, (const uint32_t*)d->quads.p, d->arena.p, status);
    if (rc) return rc;
    T.end(sp, s);
  }
  return OJPHGPU_OK;
}

// The synthesis of a run, from the level batches through the conversion: the sub-band planes in the decoder's arena ->
// d_image.  low != null: the levels below the top run on that stream (forked by the caller) and finish_blocks -- the
// rest of the block decoder on the main stream (a released run: nothing), then the join; it sets `joined` -- is called
// before the top level.  What
// ojphgpu_decoder_run_container issues behind its block decoder, and all that the synthesis-only decoder of an encoder
// with a quality target (section 5c) ever issues: one schedule, so a trial of that search sees the decoder's own samples.
template <typename F>
static int decoder_synthesis(ojphgpu_decoder* d, void* d_image, int container, hipStream_t low, bool& joined, F finish_blocks)
{
  const Plan& P = *d->P;
  hipStream_t s = d->stream;
  Spans& T = d->timer;
  int rc = OJPHGPU_OK;
  for (const LevelBatch& b : d->batches) {
    const bool top = b.depth == 0;                          // the last level of its components (there may be two such launches)
    hipStream_t ls = (low && !top) ? low : s;
    if (top && low && !joined && (rc = finish_blocks()) != 0) return rc;
    const int sp = T.begin(SP_DWT, ls);
    if (d->region) {                                        // region synthesis (the Part-1 wavelets only: plan_restrict_region)
      const ojphgpu_dwt_region* regs = (const ojphgpu_dwt_region*)(b.img_first >= 0 ? d->img_regs.p : d->dwt_regs.p) + (b.img_first >= 0 ? b.img_first : (int)b.first);
      const ojphgpu_dwt_desc* descs = (const ojphgpu_dwt_desc*)(b.img_first >= 0 ? d->img_descs.p : d->dwt_descs.p) + (b.img_first >= 0 ? b.img_first : (int)b.first);
      rc = ojphgpu::dwt_inverse_region_launch(ls, b.rev ? 1 : 0, descs, regs, b.count, b.rgrid, d->arena.p, b.img_first >= 0 ? d_image : nullptr,
                                              container, b.img_first >= 0 ? b.nc : 1);
    } else if (b.img_first >= 0) {                          // float->int / level shift applied in the stores
      ojphgpu_params pp = P.p; pp.reversible = b.rev ? 1 : 0; pp.bit_depth = b.img_depth; pp.is_signed = b.img_signed;
      const ojphgpu_dwt_desc* idesc = (const ojphgpu_dwt_desc*)d->img_descs.p + b.img_first;
      rc = b.general ? ojphgpu_dwt_inverse_general_image(ls, &b.k, &pp, idesc, b.count, b.max_w, b.max_h, d_image, d->arena.p, container)
                     : ojphgpu_dwt_inverse_image_ex(ls, &pp, idesc, b.count, b.max_w, b.max_h, d_image, d->arena.p, container, b.nc == 3);
    } else if (b.general)
      rc = ojphgpu_dwt_inverse_general(ls, &b.k, (const ojphgpu_dwt_desc*)d->dwt_descs.p + b.first, b.count, b.max_w, b.max_h, d->arena.p);
    else
      rc = ojphgpu_dwt_inverse(ls, b.rev ? 1 : 0, (const ojphgpu_dwt_desc*)d->dwt_descs.p + b.first, b.count,
                               b.max_w, b.max_h, d->arena.p);
    if (rc) return rc;
    T.end(sp, ls);
  }
  if (low && !joined && (rc = finish_blocks()) != 0) return rc;
  if (d->need_convert) {
    const int sp = T.begin(SP_CONVERT, s);
    rc = ojphgpu_convert_inverse_ex(s, &P.p, (const ojphgpu_convert_desc*)d->conv_descs.p, d->conv_tiles * d->nframes,
                                    d->conv_max_w, d->conv_max_h, d_image, d->arena.p, container);
    if (rc) return rc;
    T.end(sp, s);
  }
  return OJPHGPU_OK;
}

// The block decoder of a run takes the one launch for step 1 and step 2 (chains first, step-2 workers behind them slice by
// slice, kernels_ht_dec.hip) when every block is at most 64 samples wide, of one wavelet and without refinement passes -- and
// where it pays: blocks of 64 rows, few enough for resident workers (ht_decode_fused_pays).  Otherwise: the separate launches.
bool decoder_fuses(const ojphgpu_decoder* d)
{
  return d->fstate.p && !d->force_separate && !d->fused_off && !d->any_refine && (d->kinds & (3 | 32)) == 1 && ((d->kinds & 12) == 4 || (d->kinds & 12) == 8) &&
         d->nblocks > 0 && ojphgpu::ht_decode_fused_pays(d->nblocks, d->max_block_h, d->cus);
}

// ... and its launches on stream s (the caller's; a released run: the object's own): the one launch over all blocks, or prep + step 1 of all blocks and step 2 of the
// first `count` descriptors (the rest is the caller's: decode_samples beside the lower synthesis levels)
static int decoder_block_launches(ojphgpu_decoder* d, bool fused, uint32_t count, hipStream_t s)
{
  Spans& T = d->timer;
  if (fused) {
    const ojphgpu_cb_desc* cbd = (const ojphgpu_cb_desc*)(d->o_cb_descs ? d->o_cb_descs : d->cb_descs.p);
    uint8_t* status = (uint8_t*)(d->o_status ? d->o_status : d->status.p);
    const uint8_t* data = (const uint8_t*)(d->o_data ? d->o_data : d->data.p);
    const int sp = T.begin(SP_STEP2, s);
    const int rc = ojphgpu::ht_decode_fused_launch(s, cbd, d->nblocks, data, (uint32_t*)d->quads.p, d->arena.p, status, (uint32_t*)d->fstate.p,
                                                   ++d->fused_epoch, d->max_block_h, d->kinds, d->cus, d->d_h_retry);
    if (rc) return rc;
    d->uncollected = true;
    T.end(sp, s);
    return OJPHGPU_OK;
  }
  const int rc = decode_chains(d, s);
  return rc ? rc : decode_samples(d, s, 0, count);
}

// A run of a blocks-only decoder (the decoder half of a transcoder): the block decoder as ojphgpu_decoder_run_container
// chooses it, and nothing behind it -- the sub-band planes stay in the arena.  The run's timer is left open for its owner
// (who may have the band statistics follow) to close.
static int decoder_run_blocks(ojphgpu_decoder* d)
{
  if (!d || !d->blocks_only) return OJPHGPU_E_INVALID;
  d->timer.start(d->stream);
  const bool fused = decoder_fuses(d);
  d->last_fused = fused; d->last_image = nullptr; d->last_container = 0;
  const int rc = decoder_block_launches(d, fused, d->nblocks, d->stream);
  if (rc) return rc;
  d->ran = true;
  return OJPHGPU_OK;
}

// A released run (ojphgpu_objects.h; decoder_releases() has admitted it): the one block launch -- under
// OJPHGPU_DEC_AHEAD_LEVELS=1 synthesis levels L..2 too -- on the object's own stream, behind the object's last upload and
// the last reader of the arena it writes and NOT behind the caller's stream; the caller's stream waits for it (ev_done)
// and runs the synthesis; only the top level and the conversion write the image.  T.start / T.finish stay on the caller's stream.
namespace {
// From the first launch on the own stream on, EVERY way out of the run records ev_done behind what has been queued there -- a
// run that fails half way has launches there too, and whoever settles must wait for them, not for an older record.
struct ReleasedDecode {
  ojphgpu_decoder* d; bool armed = false;
  void done() { if (armed) (void)hipEventRecord(d->ev_done, d->side); armed = false; }
  ~ReleasedDecode() { done(); }
};
}  // namespace
static int decoder_run_released(ojphgpu_decoder* d, void* d_image, int container)
{
  hipStream_t s = d->stream, own = d->side;
  Spans& T = d->timer;
  if (d->two_arenas) { std::swap(d->arena, d->arena2); std::swap(d->ev_read, d->ev_read2); }   // (from here on `arena` is this run's)
  if (d->last_joined) {                                     // quads / fstate / data were last used on the caller's stream
    HIPCHK(hipStreamWaitEvent(own, d->two_arenas ? d->ev_read2 : d->ev_read, 0));
    d->last_joined = false;
  }
  HIPCHK(hipStreamWaitEvent(own, d->ev_read, 0));           // the last synthesis that read this arena (never recorded: no wait)
  T.start(s);
  d->last_fused = true; d->last_image = d_image; d->last_container = container;
  ReleasedDecode branch{ d, true };
  d->pending = true;                                        // (from here: also a run that fails below)
  int rc = decoder_block_launches(d, true, d->nblocks, own);
  if (rc) return rc;
  bool joined = false;
  auto join = [&]() -> int {                                // the caller's stream gets behind the own stream's part of the run
    joined = true;
    branch.done();
    HIPCHK(hipStreamWaitEvent(s, d->ev_done, 0));
    return OJPHGPU_OK;
  };
  if (!d->ahead_levels && (rc = join()) != 0) return rc;
  rc = decoder_synthesis(d, d_image, container, d->ahead_levels ? own : nullptr, joined, join);
  (void)hipEventRecord(d->ev_read, s);                      // behind the last launch of this run that reads the arena
  if (rc) return rc;
  T.finish(s);
  d->ran = true;
  return OJPHGPU_OK;
}

int ojphgpu_decoder_run_container(ojphgpu_decoder* d, void* d_image, int container);
static int decode_host(ojphgpu_decoder* d, const uint8_t* h_codestream, size_t len, void* h_image, int container);

extern "C" int ojphgpu_decoder_run_device(ojphgpu_decoder* d, int32_t* d_image) { return ojphgpu_decoder_run_container(d, d_image, 32); }
extern "C" int ojphgpu_decoder_run_device16(ojphgpu_decoder* d, uint16_t* d_image) { return ojphgpu_decoder_run_container(d, d_image, 16); }
extern "C" int ojphgpu_decoder_run_device8(ojphgpu_decoder* d, uint8_t* d_image) { return ojphgpu_decoder_run_container(d, d_image, 8); }

int ojphgpu_decoder_run_container(ojphgpu_decoder* d, void* d_image, int container)
{
  if (!d || (!d_image && !(d->region && d->P->frame_elems == 0))) return OJPHGPU_E_INVALID;   // (a region may hold no sample at a reduced resolution)
  if (d->blocks_only) return OJPHGPU_E_INVALID;             // (a transcoder's half: decoder_run_blocks)
  const Plan& P = *d->P;
  if (container != 32 && container != 16 && container != 8) return OJPHGPU_E_INVALID;
  if (container != 32) for (const CompGeo& g : P.comps) if (g.bit_depth > (uint32_t)container) return OJPHGPU_E_INVALID;
  hipStream_t s = d->stream;
  Spans& T = d->timer;
  // A run before this one asked to be decoded again and nobody collected it (ojphgpu_decoder_failed_blocks does): its
  // frame was handed out partly decoded.  The launch writes its epoch into h_retry only when its wait has run out (about two
  // seconds after it started), so the notice may arrive more than one call later: epochs only grow, and every epoch found
  // there that has not been acknowledged yet is reported once.  (A frame pipeline's runs -- o_status set -- are always
  // collected by the pipeline.)
  if (!d->o_status && !d->force_separate && d->h_retry) {
    const uint32_t gave_up = *(volatile uint32_t*)d->h_retry;
    if ((int32_t)(gave_up - d->retry_acked) > 0) {
      d->retry_acked = gave_up; d->uncollected = false;
      return OJPHGPU_E_UNCOLLECTED;
    }
  }
  // One launch for step 1 and step 2 (chains first, step-2 workers behind them slice by slice, kernels_ht_dec.hip) when
  // every block is at most 64 samples wide, of one wavelet and without refinement passes -- and where it pays: blocks
  // of 64 rows, few enough for resident workers (ht_decode_fused_pays); the synthesis levels follow on the same stream.  Otherwise: the separate launches, with the lower synthesis levels beside step 2 of the top resolution.
  const bool fused = decoder_fuses(d);
  if (decoder_releases(d)) return decoder_run_released(d, d_image, container);
  int rc = decoder_settle(d);                               // a joined run behind released ones: the last run's arena, behind all of them
  if (rc) return rc;
  struct JoinedRun {                                        // every way out: the own stream's next job can be put behind this run
    ojphgpu_decoder* d;
    ~JoinedRun() { if (d->can_release) { (void)hipEventRecord(d->ev_read, d->stream); d->last_joined = true; } }
  } joined_run{ d };
  T.start(s);
  d->last_fused = fused; d->last_image = d_image; d->last_container = container;
  const uint32_t n_low = fused ? 0u : d->n_low;
  rc = decoder_block_launches(d, fused, n_low ? n_low : d->nblocks, s);
  if (rc) return rc;
  if (n_low) {                                              // fork: the lower synthesis levels on the side stream
    HIPCHK(hipEventRecord(d->ev_fork, s));
    HIPCHK(hipStreamWaitEvent(d->side, d->ev_fork, 0));
  }
  bool joined = false;
  auto finish_blocks = [&]() -> int {                       // meanwhile, on the main stream: the top resolution's blocks
    joined = true;
    HIPCHK(hipEventRecord(d->ev_join, d->side));
    int r2 = decode_samples(d, s, n_low, d->nblocks - n_low);
    if (r2) return r2;
    HIPCHK(hipStreamWaitEvent(s, d->ev_join, 0));           // join before the top synthesis level
    return OJPHGPU_OK;
  };
  if ((rc = decoder_synthesis(d, d_image, container, n_low ? d->side : nullptr, joined, finish_blocks)) != 0) return rc;
  T.finish(s);
  d->ran = true;
  return OJPHGPU_OK;
}

static int decoder_synthesis_only(ojphgpu_decoder* d, void* d_image, int container)
{
  bool joined = true;
  return decoder_synthesis(d, d_image, container, nullptr, joined, [] { return OJPHGPU_OK; });
}

// A decoder object that only synthesises: the level batches, the conversion and an arena (zeroed, as a decoder's is) of a
// plan that was not parsed from a codestream -- an encoder's own.  No block decoder, no codestream bytes; whoever owns it
// fills the sub-band planes of its arena and calls decoder_synthesis_only.
static int decoder_create_synthesis(const ojphgpu_plan* plan, int device, void* stream, ojphgpu_decoder** out)
{
  if (!plan || !out) return OJPHGPU_E_INVALID;
  *out = nullptr;
  const Plan& P = plan->plan;
  if (P.has_region || P.skip_read || P.skip_recon) return OJPHGPU_E_INVALID;
  HIPCHK(hipSetDevice(device));
  ojphgpu_decoder* d = new (std::nothrow) ojphgpu_decoder();
  if (!d) return OJPHGPU_E_NOMEM;
  struct Owner { ojphgpu_decoder* p; ~Owner() { if (p) ojphgpu_decoder_destroy(p); } } owner{ d };
  d->P = &P; d->device = device; d->stream = (hipStream_t)stream;
  d->tiles = TileRange{ 0, (uint32_t)P.tiles.size() };
  const TileRange tr = d->tiles;
  std::vector<ojphgpu_dwt_desc> dd, idd;
  build_level_batches(P, tr, dd, d->batches);
  build_image_level_descs(P, tr, dd, d->batches, idd);
  std::reverse(d->batches.begin(), d->batches.end());                 // synthesis: lowest resolution first
  std::vector<ojphgpu_convert_desc> cd; d->need_convert = build_convert_descs(P, tr, cd, d->conv_max_w, d->conv_max_h);
  d->conv_tiles = d->tiles_touched = tr.count;
  if (d->arena.alloc(P.arena_elems * 4) || d->dwt_descs.alloc(dd.size() * sizeof(dd[0])) || d->img_descs.alloc(idd.size() * sizeof(dd[0])) ||
      d->conv_descs.alloc(cd.size() * sizeof(cd[0])))
    return OJPHGPU_E_NOMEM;
  HIPCHK(hipMemset(d->arena.p, 0, P.arena_elems * 4));
  if (!dd.empty()) HIPCHK(hipMemcpy(d->dwt_descs.p, dd.data(), dd.size() * sizeof(dd[0]), hipMemcpyHostToDevice));
  if (!idd.empty()) HIPCHK(hipMemcpy(d->img_descs.p, idd.data(), idd.size() * sizeof(idd[0]), hipMemcpyHostToDevice));
  if (!cd.empty()) HIPCHK(hipMemcpy(d->conv_descs.p, cd.data(), cd.size() * sizeof(cd[0]), hipMemcpyHostToDevice));
  d->timer.detail = false;                                  // (no spans: nobody reads this object's timing)
  owner.p = nullptr;
  *out = d;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_decoder_set_timing(ojphgpu_decoder* d, int per_launch)
{
  if (!d) return OJPHGPU_E_INVALID;
  const int rc = decoder_settle(d);                         // (the next run may be of the other schedule)
  if (rc) return rc;
  d->timer.detail = per_launch != 0;
  return OJPHGPU_OK;
}

// the run that has just been enqueued again, through the separate step 1 / step 2 launches (a fused launch asked for it)
int ojphgpu_decoder_repeat_separate(ojphgpu_decoder* d)
{
  if (!d || (!d->last_image && !d->blocks_only)) return OJPHGPU_E_INVALID;
  d->force_separate = true;
  int rc = d->blocks_only ? decoder_run_blocks(d) : ojphgpu_decoder_run_container(d, d->last_image, d->last_container);
  if (d->blocks_only && rc == OJPHGPU_OK) d->timer.finish(d->stream);
  d->force_separate = false;
  d->fused_retries++;
  return rc;
}

// The verdicts of the run enqueued last, however its status bytes reach the host: fetch(user, &st) brings the status bytes + the
// RETRY word behind them to the host once the launches enqueued so far have finished (ojphgpu_decoder_failed_blocks: a copy
// into pageable memory and a wait for the stream; a frame pipeline: a copy kernel into pinned memory and an event).
int ojphgpu_decoder_collect(ojphgpu_decoder* d, ojphgpu_status_fetch fetch, void* user, uint32_t* count)
{
  if (!d || !fetch || !count) return OJPHGPU_E_INVALID;
  d->uncollected = false;
  const uint8_t* st = nullptr;
  for (int pass = 0; pass < 2; ++pass) {
    int rc = decoder_settle(d);                             // a released run: the fetch reads its status on the caller's stream
    if (rc) return rc;
    rc = fetch(user, &st);
    if (rc) return rc;
    // a fused launch whose workers gave up waiting for their chains (the chip was held up for seconds by other work): its
    // blocks have no verdict yet -- the frame is decoded again through the separate launches, into the same image
    if (pass == 0 && d->last_fused) {
      const bool again = ojphgpu_fused_retry_wanted(st, d->nblocks, d->fused_epoch);
      d->fused_outcome(again);
      if (again) {
        rc = ojphgpu_decoder_repeat_separate(d);
        if (rc) return rc;
        continue;
      }
    }
    break;
  }
  // (the stream is drained: every give-up of the runs enqueued so far has reached h_retry; the run collected here has been
  // repeated above if it was one of them, earlier uncollected ones are beyond repair -- ojphgpu_decoder_giveup_epoch tells)
  if (d->h_retry) d->retry_acked = *(volatile uint32_t*)d->h_retry;
  uint32_t n = 0;
  for (uint32_t i = 0; i < d->nblocks; ++i) n += st[i] != 0;
  *count = n;
  return OJPHGPU_OK;
}

namespace {
struct PageableStatus { ojphgpu_decoder* d; std::vector<uint8_t> st; };
int fetch_pageable_status(void* user, const uint8_t** h_status)
{
  PageableStatus& f = *(PageableStatus*)user;
  ojphgpu_decoder* d = f.d;
  const uint8_t* status = (const uint8_t*)(d->o_status ? d->o_status : d->status.p);
  HIPCHK(hipMemcpyAsync(f.st.data(), status, f.st.size(), hipMemcpyDeviceToHost, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  *h_status = f.st.data();
  return OJPHGPU_OK;
}
}  // namespace

extern "C" int ojphgpu_decoder_failed_blocks(ojphgpu_decoder* d, uint32_t* count)
{
  if (!d || !count || !d->ran) return OJPHGPU_E_INVALID;
  const size_t tail = ((size_t)d->nblocks + 3u) & ~(size_t)3u;
  PageableStatus f{ d, std::vector<uint8_t>(tail + 4) };
  return ojphgpu_decoder_collect(d, fetch_pageable_status, &f, count);
}

extern "C" int ojphgpu_decoder_giveup_epoch(ojphgpu_decoder* d, uint32_t* last_giveup, uint32_t* current)
{
  if (!d || !last_giveup || !current) return OJPHGPU_E_INVALID;
  const int rc = decoder_settle(d);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(d->stream));
  if (d->can_release) HIPCHK(hipStreamSynchronize(d->side));   // (a released run that failed half way; an upload)
  *last_giveup = d->h_retry ? *(volatile uint32_t*)d->h_retry : 0u;
  *current = d->fused_epoch;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_decoder_region_info(ojphgpu_decoder* d, uint64_t out[4])
{
  if (!d || !out) return OJPHGPU_E_INVALID;
  uint64_t bytes = d->f_len.empty() ? 0 : d->f_len[0];
  if (!d->f_pads.empty()) for (const PadCopy& c : d->f_pads[0]) bytes += c.got;
  out[0] = d->block_ids.size(); out[1] = d->P->blocks.size(); out[2] = bytes; out[3] = d->tiles_touched;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_decoder_pending(const ojphgpu_decoder* d, int* pending)
{
  if (!d || !pending) return OJPHGPU_E_INVALID;
  *pending = d->pending ? 1 : 0;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_decoder_fused_retries(ojphgpu_decoder* d, uint32_t* count)
{
  if (!d || !count) return OJPHGPU_E_INVALID;
  *count = d->fused_retries;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_decode(ojphgpu_decoder* d, const uint8_t* h_codestream, size_t len, int32_t* h_image)
{
  return decode_host(d, h_codestream, len, h_image, 32);
}

extern "C" int ojphgpu_decode16(ojphgpu_decoder* d, const uint8_t* h_codestream, size_t len, uint16_t* h_image)
{
  return decode_host(d, h_codestream, len, h_image, 16);
}

static int decode_host(ojphgpu_decoder* d, const uint8_t* h_codestream, size_t len, void* h_image, int container)
{
  if (!d || !h_image) return OJPHGPU_E_INVALID;
  const Plan& P = *d->P;
  if (d->nframes != 1) return OJPHGPU_E_INVALID;           // batches: upload_frame + run_device
  const size_t bytes = (size_t)P.frame_elems * 4;
  if (!d->image.p && d->image.alloc(bytes)) return OJPHGPU_E_NOMEM;
  int rc = ojphgpu_decoder_upload(d, h_codestream, len);
  if (rc) return rc;
  rc = ojphgpu_decoder_run_container(d, d->image.p, container);
  if (rc) return rc;
  uint32_t failed = 0;
  rc = ojphgpu_decoder_failed_blocks(d, &failed);          // first: it may repeat the run (see there), and the image is read after that
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(h_image, d->image.p, bytes / (32 / container), hipMemcpyDeviceToHost, d->stream));
  HIPCHK(hipStreamSynchronize(d->stream));
  return failed ? OJPHGPU_E_BLOCK : OJPHGPU_OK;
}

extern "C" int ojphgpu_decoder_timing(ojphgpu_decoder* d, float out[4])
{
  if (!d || !out || !d->ran) return OJPHGPU_E_INVALID;
  if (decoder_settle(d)) return OJPHGPU_E_HIP;
  float a = 0, b = 0, c = 0, r = 0;
  if (d->timer.read(SP_PREP, &a) || d->timer.read(SP_STEP1, &b) || d->timer.read(SP_STEP2, &c) || d->timer.read(SP_REFINE, &r) ||
      d->timer.read(SP_DWT, &out[1]) || d->timer.read(SP_CONVERT, &out[2]) || d->timer.read(-1, &out[3])) return OJPHGPU_E_HIP;
  out[0] = a + b + c + r;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_decoder_ht_timing(ojphgpu_decoder* d, float out[3])
{
  if (!d || !out || !d->ran) return OJPHGPU_E_INVALID;
  if (decoder_settle(d)) return OJPHGPU_E_HIP;
  if (d->timer.read(SP_PREP, &out[0]) || d->timer.read(SP_STEP1, &out[1]) || d->timer.read(SP_STEP2, &out[2])) return OJPHGPU_E_HIP;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_decoder_level_timing(ojphgpu_decoder* d, float* out, uint32_t cap, uint32_t* n)
{
  if (!d || !out || !n || !d->ran) return OJPHGPU_E_INVALID;
  if (decoder_settle(d)) return OJPHGPU_E_HIP;
  int k = d->timer.read_each(SP_DWT, out, cap);
  if (k < 0) return OJPHGPU_E_HIP;
  *n = (uint32_t)k;
  return OJPHGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// transcoding (include/ojphgpu.h section 5d): the decoder's first half and the encoder's second half on one arena
// ---------------------------------------------------------------------------------------------
extern "C" void ojphgpu_transcoder_destroy(ojphgpu_transcoder* t)
{
  if (!t) return;
  (void)hipSetDevice(t->device);
  (void)hipStreamSynchronize(t->stream);
  if (t->enc) {
    if (t->enc->side) (void)hipStreamSynchronize(t->enc->side);
    t->enc->arena.p = nullptr;                              // the decoder's
    ojphgpu_encoder_destroy(t->enc);
  }
  if (t->dec) ojphgpu_decoder_destroy(t->dec);
  delete t;
}

extern "C" int ojphgpu_transcoder_create(const ojphgpu_plan* src, const ojphgpu_plan* out, int device, void* stream, ojphgpu_transcoder** tout)
{
  if (!src || !out || !tout) return OJPHGPU_E_INVALID;
  *tout = nullptr;
  return no_throw([&]() -> int {
    const Plan& S = src->plan; const Plan& O = out->plan;
    if (!transcode_plans_fit(S, O)) return OJPHGPU_E_INVALID;
    ojphgpu_transcoder* t = new ojphgpu_transcoder();
    struct Owner { ojphgpu_transcoder* p; ~Owner() { if (p) ojphgpu_transcoder_destroy(p); } } owner{ t };
    t->S = &S; t->O = &O; t->device = device; t->stream = (hipStream_t)stream;
    const uint32_t ntiles = (uint32_t)S.tiles.size();
    int rc = decoder_create(&src, 1, device, stream, 0, ntiles, &t->dec, true);
    if (rc) return rc;
    if ((rc = encoder_create(out, device, stream, 0, ntiles, 1, &t->enc, true)) != 0) return rc;
    ojphgpu_decoder* d = t->dec;
    t->enc->arena.p = d->arena.p;                           // one arena: the block decoder writes the planes the block coder reads
    // the flat VLC / MEL strings of any later source fit: the worst case of every block (Lcup <= 4079 + slack)
    const uint64_t worst = (uint64_t)d->block_ids.size() * ojphgpu_ht_decode_aux_words(4079) + 64;
    d->aux.release();
    if (d->aux.alloc((size_t)worst * 4 + 64)) return OJPHGPU_E_NOMEM;
    t->h_descs.resize(d->block_ids.size());
    owner.p = nullptr;
    *tout = t;
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_transcoder_set_budget(ojphgpu_transcoder* t, uint64_t max_bytes)
{
  if (!t) return OJPHGPU_E_INVALID;
  HIPCHK(hipSetDevice(t->device));
  HIPCHK(hipStreamSynchronize(t->stream));
  const int rc = ojphgpu_encoder_set_budget(t->enc, max_bytes);
  if (rc == OJPHGPU_OK) t->stage = 0;                       // (a source submitted under the other mode is dropped)
  return rc;
}

// ---- what one source needs of a transcoder, piece by piece: ojphgpu_transcoder_submit / _finish below put them together for
// a single call, with the waits only a single call needs between them; the transcode pipe (ojphgpu_pipe.cpp) spreads them
// over its stages.

// the band statistics of the planes the block decoder leaves: what the search's model starts from
int ojphgpu_transcoder_stats(ojphgpu_transcoder* t)
{
  ojphgpu_decoder* d = t->dec; ojphgpu_encoder* e = t->enc;
  EncoderRate& R = *e->rate;
  hipStream_t s = t->stream;
  HIPCHK(hipMemsetAsync(R.hist.p, 0, R.hist.n, s));
  const int sp = d->timer.begin(SP_STATS, s);
  const int rc = ojphgpu_band_stats(s, (const ojphgpu_stats_desc*)R.stats_descs.p, R.n_stats, R.stats_max_w, R.stats_max_h, e->arena.p, (uint32_t*)R.hist.p);
  if (rc) return rc;
  d->timer.end(sp, s);
  R.searched = false;
  return OJPHGPU_OK;
}

// a later source against the first one and the output: the same geometry, no causal blocks, the reversible K_max rule
int ojphgpu_transcoder_check_source(const ojphgpu_transcoder* t, const Plan& Q)
{
  const Plan& S = *t->S; const Plan& O = *t->O;
  const int rc = ojphgpu_same_frame_geometry(S, Q, true);
  if (rc) return rc;
  for (uint32_t c = 0; c < Q.p.num_comps; ++c) if (Q.style(c).causal) return OJPHGPU_E_INVALID;
  for (size_t i = 0; i < Q.bands.size(); ++i)               // (K_max is this frame's own: transcode_plans_fit saw the first frame's)
    if (Q.style(Q.bands[i].comp).rev && O.bands[i].K_max < Q.bands[i].K_max) return OJPHGPU_E_INVALID;
  return OJPHGPU_OK;
}

// its block descriptors into bd (one per block of the decoder half), with the layout and size checks; fi: what to upload
int ojphgpu_transcoder_fill_descs(const ojphgpu_transcoder* t, const Plan& Q, size_t cs_len, ojphgpu_cb_desc* bd, DecFrameInfo& fi)
{
  const ojphgpu_decoder* d = t->dec;
  const size_t nb = d->block_ids.size();
  ojphgpu_decoder_fill_descs(*t->S, Q, d->block_ids, 0, 0, bd, fi);
  uint64_t nquads = 0, naux = 0;
  if (ojphgpu_ht_decode_layout(bd, (uint32_t)nb, &nquads, &naux) != OJPHGPU_OK) return OJPHGPU_E_INVALID;
  if ((naux + 16) * 4 > d->aux.n || (nquads + 16) * 4 > d->quads.n) return OJPHGPU_E_INVALID;     // sized for the worst case at create
  if (fi.first + fi.len > cs_len) return OJPHGPU_E_CODESTREAM;
  return OJPHGPU_OK;
}

// "decode the blocks of these bytes": the block decoder over what the decoder half points at (its own buffers, or a pipe
// slot's through o_cb_descs / o_data / o_status), with a budget the band statistics behind it
int ojphgpu_transcoder_decode(ojphgpu_transcoder* t, bool any_refine, int kinds, uint32_t max_len1)
{
  ojphgpu_decoder* d = t->dec;
  int rc;
  d->any_refine = any_refine; d->kinds = kinds; d->max_len1 = max_len1;
  if ((rc = decoder_run_blocks(d)) != 0) return rc;
  if (!t->enc->budgets.empty() && (rc = ojphgpu_transcoder_stats(t)) != 0) return rc;
  d->timer.finish(t->stream);
  return OJPHGPU_OK;
}

// "collect verdicts and repeat": the verdicts first (and the repeat of a one-launch run whose wait ran out) -- only then is a
// block coded.  OJPHGPU_E_BLOCK: a failed block of a source that was not parsed resiliently (*failed counts them).  The
// statistics of a repeated run were taken over planes the repeat has written again: once more.
int ojphgpu_transcoder_verdicts(ojphgpu_transcoder* t, ojphgpu_status_fetch fetch, void* user, bool resilient, uint32_t* failed)
{
  ojphgpu_decoder* d = t->dec;
  const uint32_t repeats = d->fused_retries;
  const int rc = ojphgpu_decoder_collect(d, fetch, user, failed);
  if (rc) return rc;
  if (*failed && !resilient) return OJPHGPU_E_BLOCK;
  if (!t->enc->budgets.empty() && d->fused_retries != repeats) return ojphgpu_transcoder_stats(t);
  return OJPHGPU_OK;
}

// "code, plain, into this output set": the encoder half's plain schedule over the arena
int ojphgpu_transcoder_code(ojphgpu_transcoder* t, void* out, ojphgpu_cb_result* d_results, uint32_t* d_counters)
{
  ojphgpu_encoder* e = t->enc;
  int rc;
  BlockCoderRun coder{ e, (uint8_t*)out, d_results, d_counters, (uint32_t)e->block_ids.size(), &e->timer };
  e->timer.start(t->stream);
  if ((rc = coder.clear()) != 0 || (rc = coder.rest_and_join()) != 0) return rc;
  e->timer.finish(t->stream);
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_transcoder_submit(ojphgpu_transcoder* t, const uint8_t* h_codestream, size_t len, int resilient)
{
  if (!t || !h_codestream || len == 0) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    ojphgpu_decoder* d = t->dec; ojphgpu_encoder* e = t->enc;
    const Plan& O = *t->O;
    hipStream_t s = t->stream;
    const bool budget = !e->budgets.empty();
    if (!budget && !plan_all_reversible(O) && !(O.p.qstep > 0.0f)) return OJPHGPU_E_INVALID;   // no step and no budget
    HIPCHK(hipSetDevice(t->device));
    ojphgpu_plan* q = nullptr;
    int rc = ojphgpu_t2_parse(h_codestream, len, resilient, &q);
    if (rc) return rc;
    struct Hold { ojphgpu_plan* q; ~Hold() { ojphgpu_plan_destroy(q); } } hold{ q };
    const Plan& Q = q->plan;
    if ((rc = ojphgpu_transcoder_check_source(t, Q)) != 0) return rc;
    const size_t nb = d->block_ids.size();
    ojphgpu_cb_desc* bd = t->h_descs.data();
    // the launches of the last source have read what is replaced now (descriptors on the host and on the device, the bytes)
    HIPCHK(hipStreamSynchronize(s));
    if (e->side) HIPCHK(hipStreamSynchronize(e->side));
    DecFrameInfo fi;
    if ((rc = ojphgpu_transcoder_fill_descs(t, Q, len, bd, fi)) != 0) return rc;
    t->stage = 0;
    const size_t need = (size_t)fi.data_bytes() + 128;
    if (need > d->data.n) {
      d->data.release();
      if (d->data.alloc(need + need / 4)) return OJPHGPU_E_NOMEM;
    }
    if (fi.len) HIPCHK(hipMemcpyAsync(d->data.p, h_codestream + fi.first, (size_t)fi.len, hipMemcpyHostToDevice, s));
    if ((rc = ojphgpu_decoder_upload_pads(s, (uint8_t*)d->data.p, h_codestream, len, fi.pads)) != 0) return rc;
    if (nb) HIPCHK(hipMemcpyAsync(d->cb_descs.p, bd, nb * sizeof(ojphgpu_cb_desc), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));                        // the caller's codestream may go
    if ((rc = ojphgpu_transcoder_decode(t, fi.any_refine, fi.kinds, fi.max_len1)) != 0) return rc;
    e->ran = false; e->fetched = false;
    t->resilient = resilient != 0; t->failed = 0; t->code_ms = t->final_ms = 0;
    t->stage = 1;
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_transcoder_finish(ojphgpu_transcoder* t, uint8_t* h_out, size_t cap, size_t* out_len, uint32_t* failed_blocks)
{
  if (!t || !out_len || t->stage == 0) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    ojphgpu_decoder* d = t->dec; ojphgpu_encoder* e = t->enc;
    hipStream_t s = t->stream;
    HIPCHK(hipSetDevice(t->device));
    const bool budget = !e->budgets.empty();
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    int rc;
    if (t->stage == 1) {
      if (!d->ran) { t->stage = 0; return OJPHGPU_E_INVALID; }
      const size_t tail = ((size_t)d->nblocks + 3u) & ~(size_t)3u;
      PageableStatus f{ d, std::vector<uint8_t>(tail + 4) };
      rc = ojphgpu_transcoder_verdicts(t, fetch_pageable_status, &f, t->resilient, &t->failed);
      if (failed_blocks && (rc == OJPHGPU_OK || rc == OJPHGPU_E_BLOCK)) *failed_blocks = t->failed;
      if (rc) { t->stage = 0; return rc; }
      const auto t0 = now();
      if (!budget) {
        if ((rc = ojphgpu_transcoder_code(t, e->out.p, (ojphgpu_cb_result*)e->results.p, (uint32_t*)e->counters.p)) != 0) { t->stage = 0; return rc; }
        HIPCHK(hipStreamSynchronize(s));
        t->code_ms = ms(t0, now());
      }
      e->ran = true; e->fetched = false;
      t->stage = 2;
    }
    if (failed_blocks) *failed_blocks = t->failed;
    const auto t1 = now();
    rc = ojphgpu_encoder_finish(e, h_out, cap, out_len);
    if (budget && e->rate->searched) { t->code_ms = e->rate->search_ms; t->final_ms = e->rate->final_ms; }
    else t->final_ms = ms(t1, now());
    if (rc != OJPHGPU_E_OVERFLOW) t->stage = 0;             // (too small a buffer: *out_len holds the need, the call may be repeated)
    return rc;
  });
}

extern "C" int ojphgpu_transcoder_rate_info(ojphgpu_transcoder* t, ojphgpu_rate_info* info)
{
  if (!t) return OJPHGPU_E_INVALID;
  return ojphgpu_encoder_rate_info(t->enc, info);
}

extern "C" int ojphgpu_transcoder_timing(ojphgpu_transcoder* t, float out[4])
{
  if (!t || !out || !t->dec->ran) return OJPHGPU_E_INVALID;
  HIPCHK(hipStreamSynchronize(t->stream));
  Spans& T = t->dec->timer;
  float a = 0, b = 0, c = 0, r = 0;
  if (T.read(SP_PREP, &a) || T.read(SP_STEP1, &b) || T.read(SP_STEP2, &c) || T.read(SP_REFINE, &r) || T.read(SP_STATS, &out[1])) return OJPHGPU_E_HIP;
  out[0] = a + b + c + r; out[2] = (float)t->code_ms; out[3] = (float)t->final_ms;
  return OJPHGPU_OK;
}

// ---------------------------------------------------------------------------------------------
// recoding through the sample domain (include/ojphgpu.h section 5e): a decoder and an encoder with one frame between them
// ---------------------------------------------------------------------------------------------
extern "C" void ojphgpu_recoder_destroy(ojphgpu_recoder* r)
{
  if (!r) return;
  (void)hipSetDevice(r->device);
  (void)hipStreamSynchronize(r->stream);
  if (r->enc) ojphgpu_encoder_destroy(r->enc);              // (both wait for their side streams)
  if (r->dec) ojphgpu_decoder_destroy(r->dec);
  for (DeviceBuf* b : { &r->frame, &r->fitted, &r->comps }) b->release();
  for (hipEvent_t ev : { r->ev_fit0, r->ev_fit1 }) if (ev) (void)hipEventDestroy(ev);
  delete r;
}

// may a decoder of S (parsed, under its view) feed an encoder of O through the fit?
static bool recode_plans_fit(const Plan& S, const Plan& O)
{
  if (!S.parsed || S.coded.size() != S.blocks.size() || O.parsed || !O.coded.empty()) return false;
  if (O.skip_read || O.skip_recon || O.has_region) return false;
  if (S.any_wide || O.any_wide || S.comps.size() != O.comps.size() || S.comps.empty() || S.frame_elems == 0) return false;
  for (size_t c = 0; c < S.comps.size(); ++c) {
    const CompGeo& a = S.comps[c]; const CompGeo& b = O.comps[c];
    if (a.w != b.w || a.h != b.h || a.is_signed != b.is_signed || a.frame_off != b.frame_off) return false;
    if (a.bit_depth == 0 || a.bit_depth > 32 || b.bit_depth == 0 || b.bit_depth > 32) return false;
    if (S.has_region) {                                     // the window starts on a sample of every component
      const uint64_t fx = (uint64_t)a.dx << S.skip_recon, fy = (uint64_t)a.dy << S.skip_recon;
      if (((uint64_t)S.p.image_x0 + S.region[0]) % fx != 0 || ((uint64_t)S.p.image_y0 + S.region[1]) % fy != 0) return false;
    }
  }
  return S.frame_elems == O.frame_elems;
}

// the output's nominal range and the shift to its depth: what the fit of component a -> b takes
static void recode_fit_range(const CompGeo& a, const CompGeo& b, int32_t& shift, int32_t& lo, int32_t& hi)
{
  shift = (int32_t)a.bit_depth - (int32_t)b.bit_depth;
  lo = (int32_t)(b.is_signed ? -((int64_t)1 << (b.bit_depth - 1)) : 0);
  hi = (int32_t)(b.is_signed ? ((int64_t)1 << (b.bit_depth - 1)) - 1 : std::min<int64_t>(((int64_t)1 << b.bit_depth) - 1, INT32_MAX));
}

// may a decoder of S (parsed, under its view) feed an encoder of O through the resampling fit?  Fills the table of
// ojphgpu_frame_resample, one entry per component.  recode_plans_fit with the size rule replaced: b.dx == a.dx * fx (rows
// alike), fx 1 or 2, and b's size what the halved grid gives
static bool recode_plans_resample(const Plan& S, const Plan& O, std::vector<ojphgpu_resample_comp>& tab)
{
  if (!S.parsed || S.coded.size() != S.blocks.size() || O.parsed || !O.coded.empty()) return false;
  if (O.skip_read || O.skip_recon || O.has_region) return false;
  if (S.any_wide || O.any_wide || S.comps.size() != O.comps.size() || S.comps.empty() || S.frame_elems == 0) return false;
  const bool view = S.skip_read || S.skip_recon || S.has_region;
  const uint64_t ax0 = (uint64_t)S.p.image_x0 + (S.has_region ? S.region[0] : 0), ay0 = (uint64_t)S.p.image_y0 + (S.has_region ? S.region[1] : 0);
  tab.assign(S.comps.size(), ojphgpu_resample_comp{});
  for (size_t c = 0; c < S.comps.size(); ++c) {
    const CompGeo& a = S.comps[c]; const CompGeo& b = O.comps[c];
    if (a.is_signed != b.is_signed) return false;
    if (a.bit_depth == 0 || a.bit_depth > 32 || b.bit_depth == 0 || b.bit_depth > 32) return false;
    if (a.dx == 0 || a.dy == 0 || b.dx % a.dx != 0 || b.dy % a.dy != 0) return false;     // (upsampling, or no whole factor)
    const uint32_t fx = b.dx / a.dx, fy = b.dy / a.dy;
    if (fx < 1 || fx > 2 || fy < 1 || fy > 2) return false;
    // a view starts on a sample of every OUTPUT component (a whole-frame view of a resampled component included: its
    // output has no image offset, so the decimation starts at phase 0 and the view's first sample must be an even one)
    if (S.has_region || (view && (fx == 2 || fy == 2))) {
      const uint64_t gx = (uint64_t)b.dx << S.skip_recon, gy = (uint64_t)b.dy << S.skip_recon;
      if (ax0 % gx != 0 || ay0 % gy != 0) return false;
    }
    const uint32_t px = view ? 0u : (a.x0 & 1u), py = view ? 0u : (a.y0 & 1u);
    const uint32_t w = fx == 2 ? (uint32_t)(((uint64_t)a.w + 1u - px) / 2u) : a.w, h = fy == 2 ? (uint32_t)(((uint64_t)a.h + 1u - py) / 2u) : a.h;
    if (b.w != w || b.h != h) return false;
    ojphgpu_resample_comp& t = tab[c];
    t.src_first = a.frame_off; t.dst_first = b.frame_off;
    t.src_w = a.w; t.src_h = a.h; t.dst_w = b.w; t.dst_h = b.h;
    t.fx = fx; t.fy = fy; t.px = fx == 2 ? px : 0u; t.py = fy == 2 ? py : 0u;
    recode_fit_range(a, b, t.shift, t.lo, t.hi);
  }
  return O.frame_elems != 0;
}

extern "C" int ojphgpu_recoder_resample_table(const ojphgpu_plan* src, const ojphgpu_plan* out, int resample, ojphgpu_resample_comp* comps,
                                              uint32_t cap, uint32_t* n)
{
  if (!src || !out || !comps || !n) return OJPHGPU_E_INVALID;
  *n = 0;
  if (resample != OJPHGPU_RESAMPLE_NONE && resample != OJPHGPU_RESAMPLE_COSITED) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    const Plan& S = src->plan; const Plan& O = out->plan;
    std::vector<ojphgpu_resample_comp> tab;
    if (resample == OJPHGPU_RESAMPLE_NONE) {                 // the fit's own judgement, its components as entries with both factors 1
      if (!recode_plans_fit(S, O)) return OJPHGPU_E_INVALID;
      tab.assign(S.comps.size(), ojphgpu_resample_comp{});
      for (size_t c = 0; c < S.comps.size(); ++c) {
        const CompGeo& a = S.comps[c]; const CompGeo& b = O.comps[c];
        ojphgpu_resample_comp& t = tab[c];
        t.src_first = a.frame_off; t.dst_first = b.frame_off;
        t.src_w = t.dst_w = a.w; t.src_h = t.dst_h = a.h;
        t.fx = t.fy = 1;
        recode_fit_range(a, b, t.shift, t.lo, t.hi);
      }
    } else if (!recode_plans_resample(S, O, tab)) return OJPHGPU_E_INVALID;
    if (tab.size() > cap) return OJPHGPU_E_INVALID;
    std::copy(tab.begin(), tab.end(), comps);
    *n = (uint32_t)tab.size();
    return OJPHGPU_OK;
  });
}

static int recoder_create(const ojphgpu_plan* src, const ojphgpu_plan* out, int resample, int device, void* stream, ojphgpu_recoder** rout)
{
  if (!src || !out || !rout) return OJPHGPU_E_INVALID;
  *rout = nullptr;
  if (resample != OJPHGPU_RESAMPLE_NONE && resample != OJPHGPU_RESAMPLE_COSITED) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    const Plan& S = src->plan; const Plan& O = out->plan;
    std::vector<ojphgpu_resample_comp> tab;
    if (resample == OJPHGPU_RESAMPLE_NONE ? !recode_plans_fit(S, O) : !recode_plans_resample(S, O, tab)) return OJPHGPU_E_INVALID;
    bool resampled = false;
    for (const ojphgpu_resample_comp& t : tab) resampled = resampled || t.fx == 2 || t.fy == 2;
    ojphgpu_recoder* r = new ojphgpu_recoder();
    struct Owner { ojphgpu_recoder* p; ~Owner() { if (p) ojphgpu_recoder_destroy(p); } } owner{ r };
    r->S = &S; r->O = &O; r->device = device; r->stream = (hipStream_t)stream;
    int rc = decoder_create(&src, 1, device, stream, 0, (uint32_t)S.tiles.size(), &r->dec, false);
    if (rc) return rc;
    if ((rc = ojphgpu_encoder_create_joined(out, device, stream, &r->enc)) != 0) return rc;
    ojphgpu_decoder* d = r->dec;
    // the flat VLC / MEL strings of any later source fit: the worst case of every block (Lcup <= 4079 + slack)
    const uint64_t worst = (uint64_t)d->block_ids.size() * ojphgpu_ht_decode_aux_words(4079) + 64;
    d->aux.release();
    if (d->aux.alloc((size_t)worst * 4 + 64)) return OJPHGPU_E_NOMEM;
    r->h_descs.resize(d->block_ids.size());
    uint32_t deepest = 0;
    std::vector<ojphgpu_fit_comp> fc(S.comps.size());
    for (size_t c = 0; c < S.comps.size(); ++c) {
      const CompGeo& a = S.comps[c]; const CompGeo& b = O.comps[c];
      deepest = std::max(deepest, b.bit_depth);
      int32_t shift, lo, hi;
      recode_fit_range(a, b, shift, lo, hi);
      fc[c] = ojphgpu_fit_comp{ a.frame_off, (uint64_t)a.w * a.h, shift, lo, hi, 0 };
    }
    r->container = deepest <= 8 ? 8 : deepest <= 16 ? 16 : 32;
    r->ncomps = (uint32_t)fc.size();
    r->resampled = resampled;
    // (a resampled G has the output's layout: never the int32 frame itself)
    const bool own_g = r->container != 32 || resampled;
    const void* table = resampled ? (const void*)tab.data() : (const void*)fc.data();
    const size_t table_bytes = resampled ? tab.size() * sizeof(tab[0]) : fc.size() * sizeof(fc[0]);
    HIPCHK(hipSetDevice(device));
    if (r->frame.alloc((size_t)S.frame_elems * 4 + 64) || r->comps.alloc(table_bytes) ||
        (own_g && r->fitted.alloc((size_t)O.frame_elems * (size_t)(r->container / 8) + 64))) return OJPHGPU_E_NOMEM;
    HIPCHK(hipMemcpy(r->comps.p, table, table_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipEventCreate(&r->ev_fit0));
    HIPCHK(hipEventCreate(&r->ev_fit1));
    owner.p = nullptr;
    *rout = r;
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_recoder_create(const ojphgpu_plan* src, const ojphgpu_plan* out, int device, void* stream, ojphgpu_recoder** rout)
{
  return recoder_create(src, out, OJPHGPU_RESAMPLE_NONE, device, stream, rout);
}

extern "C" int ojphgpu_recoder_create_resampled(const ojphgpu_plan* src, const ojphgpu_plan* out, int resample, int device, void* stream,
                                                ojphgpu_recoder** rout)
{
  return recoder_create(src, out, resample, device, stream, rout);
}

extern "C" int ojphgpu_recoder_encoder(ojphgpu_recoder* r, ojphgpu_encoder** enc)
{
  if (!r || !enc) return OJPHGPU_E_INVALID;
  *enc = r->enc;
  return OJPHGPU_OK;
}

// the fit of the frame the decoder has written, and the encoder's run on it
static int recoder_fit_and_run(ojphgpu_recoder* r)
{
  hipStream_t s = r->stream;
  HIPCHK(hipEventRecord(r->ev_fit0, s));
  int rc = r->resampled
             ? ojphgpu_frame_resample(s, (const int32_t*)r->frame.p, r->g(), r->container, (const ojphgpu_resample_comp*)r->comps.p, r->ncomps)
             : ojphgpu_frame_fit(s, (const int32_t*)r->frame.p, r->g(), r->container, (const ojphgpu_fit_comp*)r->comps.p, r->ncomps);
  if (rc) return rc;
  HIPCHK(hipEventRecord(r->ev_fit1, s));
  return ojphgpu_encoder_run_container(r->enc, r->g(), r->container);
}

extern "C" int ojphgpu_recoder_submit(ojphgpu_recoder* r, const uint8_t* h_codestream, size_t len, int resilient)
{
  if (!r || !h_codestream || len == 0) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    ojphgpu_decoder* d = r->dec; ojphgpu_encoder* e = r->enc;
    const Plan& S = *r->S;
    hipStream_t s = r->stream;
    HIPCHK(hipSetDevice(r->device));
    ojphgpu_plan* q = nullptr;
    int rc = ojphgpu_t2_parse(h_codestream, len, resilient, &q);
    if (rc) return rc;
    struct Hold { ojphgpu_plan* q; ~Hold() { ojphgpu_plan_destroy(q); } } hold{ q };
    // the view: restricted as `src` was (the refusals of the two calls are a geometry that differs)
    if ((S.skip_read || S.skip_recon) && ojphgpu_plan_restrict_resolution(q, S.skip_read, S.skip_recon) != 0) return OJPHGPU_E_INVALID;
    if (S.has_region && ojphgpu_plan_restrict_region(q, S.region[0], S.region[1], S.region[2], S.region[3]) != 0) return OJPHGPU_E_INVALID;
    const Plan& Q = q->plan;
    if ((rc = ojphgpu_same_frame_geometry(S, Q, true)) != 0) return rc;
    // the launches of the last source have read what is replaced now (descriptors on the host and on the device, the bytes),
    // and a search of the last finish may still hold the frame
    HIPCHK(hipStreamSynchronize(s));
    if (d->side) HIPCHK(hipStreamSynchronize(d->side));
    if (e->side) HIPCHK(hipStreamSynchronize(e->side));
    const size_t nb = d->block_ids.size();
    ojphgpu_cb_desc* bd = r->h_descs.data();
    DecFrameInfo fi;
    ojphgpu_decoder_fill_descs(S, Q, d->block_ids, 0, 0, bd, fi);
    uint64_t nquads = 0, naux = 0;
    if (ojphgpu_ht_decode_layout(bd, (uint32_t)nb, &nquads, &naux) != OJPHGPU_OK) return OJPHGPU_E_INVALID;
    if ((naux + 16) * 4 > d->aux.n || (nquads + 16) * 4 > d->quads.n) return OJPHGPU_E_INVALID;     // sized for the worst case at create
    const bool runs = S.has_region;                         // (as the view decoder uploads: ojphgpu_decoder_upload_frame)
    if (runs) { for (const DecRun& k : fi.runs) if (k.src > len || k.n > len - k.src) return OJPHGPU_E_CODESTREAM; }
    else if (fi.first + fi.len > len) return OJPHGPU_E_CODESTREAM;
    r->stage = 0;
    const size_t need = (size_t)fi.data_bytes() + 128;
    if (need > d->data.n) {
      d->data.release();
      if (d->data.alloc(need + need / 4)) return OJPHGPU_E_NOMEM;
    }
    if (runs && fi.len) {                                   // the runs at their places, zeros between them
      r->h_stage.assign((size_t)fi.len, 0);
      for (const DecRun& k : fi.runs) memcpy(r->h_stage.data() + k.dst, h_codestream + k.src, (size_t)k.n);
      HIPCHK(hipMemcpyAsync(d->data.p, r->h_stage.data(), (size_t)fi.len, hipMemcpyHostToDevice, s));
    } else if (fi.len) HIPCHK(hipMemcpyAsync(d->data.p, h_codestream + fi.first, (size_t)fi.len, hipMemcpyHostToDevice, s));
    if ((rc = ojphgpu_decoder_upload_pads(s, (uint8_t*)d->data.p, h_codestream, len, fi.pads)) != 0) return rc;
    if (nb) HIPCHK(hipMemcpyAsync(d->cb_descs.p, bd, nb * sizeof(ojphgpu_cb_desc), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));                        // the caller's codestream may go
    d->any_refine = fi.any_refine; d->kinds = fi.kinds; d->max_len1 = fi.max_len1;
    rc = ojphgpu_decoder_run_container(d, r->frame.p, 32);
    if (rc == OJPHGPU_E_UNCOLLECTED) rc = ojphgpu_decoder_run_container(d, r->frame.p, 32);   // (a source submitted and never finished: dropped)
    if (rc) return rc;
    if ((rc = recoder_fit_and_run(r)) != 0) return rc;
    r->resilient = resilient != 0; r->failed = 0; r->final_ms = 0;
    r->stage = 1;
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_recoder_finish(ojphgpu_recoder* r, uint8_t* h_out, size_t cap, size_t* out_len, uint32_t* failed_blocks)
{
  if (!r || !out_len || r->stage == 0) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    ojphgpu_decoder* d = r->dec; ojphgpu_encoder* e = r->enc;
    HIPCHK(hipSetDevice(r->device));
    int rc;
    if (r->stage == 1) {
      // the verdicts first, and the repeat of a one-launch run whose wait ran out: it decodes into the int32 frame again, so
      // the fit and the encoder's run follow it once more
      const uint32_t repeats = d->fused_retries;
      const size_t tail = ((size_t)d->nblocks + 3u) & ~(size_t)3u;
      PageableStatus f{ d, std::vector<uint8_t>(tail + 4) };
      rc = ojphgpu_decoder_collect(d, fetch_pageable_status, &f, &r->failed);
      if (rc) { r->stage = 0; return rc; }
      if (failed_blocks) *failed_blocks = r->failed;
      if (r->failed && !r->resilient) { r->stage = 0; return OJPHGPU_E_BLOCK; }
      if (d->fused_retries != repeats && (rc = recoder_fit_and_run(r)) != 0) { r->stage = 0; return rc; }
      r->stage = 2;
    }
    if (failed_blocks) *failed_blocks = r->failed;
    const auto t0 = std::chrono::steady_clock::now();
    rc = ojphgpu_encoder_finish(e, h_out, cap, out_len);
    r->final_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (rc != OJPHGPU_E_OVERFLOW) r->stage = 0;             // (too small a buffer: *out_len holds the need, the call may be repeated)
    return rc;
  });
}

extern "C" int ojphgpu_recoder_frame(ojphgpu_recoder* r, const void** d_frame, int* container_bits)
{
  if (!r || !d_frame || !container_bits || !r->dec->ran) return OJPHGPU_E_INVALID;
  *d_frame = r->g(); *container_bits = r->container;
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_recoder_timing(ojphgpu_recoder* r, float out[4])
{
  if (!r || !out || !r->dec->ran || !r->enc->ran) return OJPHGPU_E_INVALID;
  HIPCHK(hipSetDevice(r->device));
  HIPCHK(hipStreamSynchronize(r->stream));
  float t[4];
  int rc = ojphgpu_decoder_timing(r->dec, t);
  if (rc) return rc;
  out[0] = t[3];
  HIPCHK(hipEventElapsedTime(&out[1], r->ev_fit0, r->ev_fit1));
  if ((rc = ojphgpu_encoder_timing(r->enc, t)) != 0) return rc;
  out[2] = t[3]; out[3] = (float)r->final_ms;
  return OJPHGPU_OK;
}
