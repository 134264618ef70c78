// openjph_amd/csrc/ojphgpu_objects.h -- internals shared by the whole-frame codec objects
// (ojphgpu_codec.cpp) and the frame pipelines built on them (ojphgpu_pipe.cpp): device / pinned host
// buffers, launch batching, per-run event timing, and the encoder / decoder objects themselves.
#ifndef OJPHGPU_OBJECTS_H
#define OJPHGPU_OBJECTS_H
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "dwt_region.h"
#include "ht_tables.h"
#include "ojph_plan.h"

using namespace ojphgpu;

namespace {

#define HIPCHK(x) do { if ((x) != hipSuccess) return OJPHGPU_E_HIP; } while (0)

struct DeviceBuf {
  void* p = nullptr; size_t n = 0;
  int alloc(size_t bytes) { n = bytes; return hipMalloc(&p, bytes ? bytes : 16) == hipSuccess ? 0 : -1; }
  void release() { if (p) (void)hipFree(p); p = nullptr; }
};

// pinned host staging buffer (grows, never shrinks): D2H lands here at PCIe speed and without the
// page-fault cost of a fresh pageable allocation
struct HostBuf {
  uint8_t* p = nullptr; size_t cap = 0; bool pinned = false; unsigned uses = 0;
  // the first run of a codec object gets plain memory (pinning costs more than one pageable copy
  // saves); an object that is run again is a long-lived one and gets a pinned buffer
  int reserve(size_t bytes) {
    const bool want_pin = ++uses >= 2;
    if (bytes <= cap && (pinned || !want_pin)) return 0;
    release();
    void* q = nullptr;
    if (want_pin && hipHostMalloc(&q, bytes, hipHostMallocDefault) == hipSuccess) { p = (uint8_t*)q; pinned = true; }
    else { (void)hipGetLastError(); p = (uint8_t*)malloc(bytes); pinned = false; }
    cap = p ? bytes : 0;
    return p ? 0 : -1;
  }
  void release() { if (p) { if (pinned) (void)hipHostFree(p); else free(p); } p = nullptr; cap = 0; }
};

// One DWT launch: the levels `depth` steps below the top of their component, of the components with
// the same wavelet.  Without COCs that is one batch per resolution; with them a component may have
// fewer levels than another, or the other wavelet, and a depth splits in two.
// nc = 3: the batch holds the top levels of the three colour components of every tile, as triples, and the
// component transform is applied inside the DWT kernel (kernels_dwt.hip); group: 0 all components, 1 the colour
// components (0..2), 2 the others -- how a depth is split when the colour transform is fused
// general: levels of components that need the general lifting kernels (a Part-2 wavelet or decomposition, or 64-bit samples;
// kernels_dwt.hip's WvGen pipeline or kernels_lift.hip) -- k describes the level; components with equal k share a batch
struct LevelBatch { uint32_t first, count, max_w, max_h, depth; bool rev; int img_first; int nc; int group; bool general; ojphgpu_lift k;
                    std::vector<uint32_t> comps;           // comps: the components of a general-lifting batch, in descriptor order
                    ojphgpu::DwtRegionGrid rgrid;          // region decoders: what sizes the batch's region launch
                    uint32_t img_depth = 0, img_signed = 0; }; // img_first >= 0: the deepest sample format among the batch's image planes

// DWT descriptors grouped so that one launch handles every tile-component
struct TileRange { uint32_t first, count; bool has(uint32_t t) const { return t >= first && t - first < count; } };

inline bool in_group(uint32_t comp, int group) { return group == 0 || (group == 1) == (comp < 3); }

// The component transform is applied inside the top DWT level of the three colour components (no conversion pass)
// when every one of them has such a level and no non-linearity sits between the samples and the transform
inline bool is_wide(const Plan& P, uint32_t comp) { return comp < P.wide.size() && P.wide[comp] != 0; }
// samples deeper than 26 bits are converted by the conversion kernels, not inside the top DWT level (whose conversion
// arithmetic was built and tested for the depths the 32-bit path had until round 4)
inline bool deep(const Plan& P, uint32_t comp) { return P.comps[comp].bit_depth > 26 || P.general(comp); }

// A component of the general lifting kernels (an ATK marker segment's wavelet) whose top level can take the conversion from /
// to the image samples itself, like the 5/3 and 9/7 launches do (kernels_dwt.hip: WvGen with an image side): 32-bit working
// samples, at most 26 bits deep, a top level that transforms both directions with at most four steps, no colour transform
// over it.  All or nothing per codestream (general_fused): the conversion kernels then have nothing left to do for them.
inline bool general_image_fusable(const Plan& P, uint32_t c)
{
  if (!P.general(c) || is_wide(P, c) || P.comps[c].bit_depth > 26 || P.recon_decomps(c) == 0) return false;
  if (P.p.color_transform && c < 3) return false;
  const ojphgpu_lift k = P.lift_of(c, P.skip_recon + 1);
  return k.horz && k.vert && k.num_steps >= 1 && k.num_steps <= 4 && k.elem != 1;
}
inline bool general_fused(const Plan& P);

inline bool colour_fused(const Plan& P)
{
  if (!P.p.color_transform || P.any_nlt3 || P.p.num_comps < 3) return false;
  for (uint32_t c = 0; c < 3; ++c) if (P.recon_decomps(c) == 0 || deep(P, c)) return false;
  const char* off = getenv("OJPHGPU_NO_COLOUR_FUSION");          // test switch: "1" keeps the stand-alone conversion kernels
  return !(off && off[0] && off[0] != '0');
}

inline bool general_fused(const Plan& P)
{
  const char* off = getenv("OJPHGPU_NO_GENERAL_FUSION");         // test switch: "1" keeps the stand-alone conversion kernels
  if ((off && off[0] && off[0] != '0') || P.any_nlt3 || (P.p.color_transform && !colour_fused(P))) return false;
  bool any = false;
  for (uint32_t c = 0; c < P.p.num_comps; ++c) {
    if (!P.general(c) || P.recon_decomps(c) == 0) continue;
    if (!general_image_fusable(P, c)) return false;
    any = true;
  }
  return any;
}

// gen_comp < 0: the levels of the components the two built-in wavelets' kernels transform; >= 0: of that component alone
template <typename F>
void for_levels_of(const Plan& P, TileRange tr, uint32_t depth, bool rev, int group, int gen_comp, F f)
{
  for (const ojphgpu_level_info& lv : P.levels) {
    if (!tr.has(lv.tile) || P.style(lv.comp).rev != rev || !in_group(lv.comp, group)) continue;
    if (gen_comp < 0 ? P.general(lv.comp) : (int)lv.comp != gen_comp) continue;
    const uint32_t L = P.recon_decomps(lv.comp);            // reduced-resolution decoding stops below the top levels
    if (L > depth && lv.res == L - depth) f(lv);
  }
}

uint32_t max_recon_decomps(const Plan& P)
{
  uint32_t m = 0;
  for (uint32_t c = 0; c < P.p.num_comps; ++c) m = std::max(m, P.recon_decomps(c));
  return m;
}

inline void push_level_desc(const ojphgpu_level_info& lv, std::vector<ojphgpu_dwt_desc>& descs, LevelBatch& b)
{
  ojphgpu_dwt_desc d; memset(&d, 0, sizeof(d));
  d.src_off = lv.src_off; d.ll_off = lv.ll_off; d.hl_off = lv.hl_off; d.lh_off = lv.lh_off; d.hh_off = lv.hh_off;
  d.src_pitch = lv.src_pitch; d.ll_pitch = lv.ll_pitch; d.hl_pitch = lv.hl_pitch; d.lh_pitch = lv.lh_pitch;
  d.hh_pitch = lv.hh_pitch; d.w = lv.w; d.h = lv.h; d.x_even = lv.x_even; d.y_even = lv.y_even;
  descs.push_back(d);
  b.count++; b.max_w = std::max(b.max_w, lv.w); b.max_h = std::max(b.max_h, lv.h);
}

void build_level_batches(const Plan& P, TileRange tr, std::vector<ojphgpu_dwt_desc>& descs, std::vector<LevelBatch>& batches)
{
  descs.clear(); batches.clear();
  const uint32_t depths = max_recon_decomps(P);
  const bool fused = colour_fused(P);
  ojphgpu_lift none; memset(&none, 0, sizeof(none));
  for (uint32_t depth = 0; depth < depths; ++depth) {
    for (int rev = 0; rev < 2; ++rev)
    for (int group = (fused && depth == 0) ? 1 : 0; group <= ((fused && depth == 0) ? 2 : 0); ++group) {
      LevelBatch b{ (uint32_t)descs.size(), 0, 0, 0, depth, rev != 0, -1, group == 1 ? 3 : 1, group, false, none };
      for_levels_of(P, tr, depth, rev != 0, group, -1, [&](const ojphgpu_level_info& lv) { push_level_desc(lv, descs, b); });
      if (b.count) batches.push_back(b);
    }
    for (uint32_t c = 0; c < P.p.num_comps; ++c) {            // components of the general lifting kernels: a batch each
      if (!P.general(c)) continue;
      const uint32_t L = P.recon_decomps(c);
      if (L <= depth) continue;
      // the level `depth` steps below the component's reconstructed top is decomposition level (skipped + depth + 1)
      LevelBatch b{ (uint32_t)descs.size(), 0, 0, 0, depth, P.style(c).rev, -1, 1, 0, true, P.lift_of(c, P.skip_recon + depth + 1) };
      for_levels_of(P, tr, depth, P.style(c).rev, 0, (int)c, [&](const ojphgpu_level_info& lv) { push_level_desc(lv, descs, b); });
      if (!b.count) continue;
      b.comps.push_back(c);
      // components that share a kernel and a kind of level (the usual case: one ATK for the whole codestream) share the launch
      LevelBatch* prev = batches.empty() ? nullptr : &batches.back();
      if (prev && prev->general && prev->depth == depth && prev->first + prev->count == b.first && memcmp(&prev->k, &b.k, sizeof(b.k)) == 0) {
        prev->count += b.count; prev->max_w = std::max(prev->max_w, b.max_w); prev->max_h = std::max(prev->max_h, b.max_h);
        prev->comps.push_back(c);
      } else batches.push_back(b);
    }
  }
}

// Descriptors of the top DWT level of every component with the un-decomposed plane addressed inside
// the image-sized component planes (for ojphgpu_dwt_forward_image / _inverse_image); batch.img_first
// points at them.  None when the fused path does not apply (colour transform).
void build_image_level_descs(const Plan& P, TileRange tr, const std::vector<ojphgpu_dwt_desc>& descs, std::vector<LevelBatch>& batches,
                             std::vector<ojphgpu_dwt_desc>& out)
{
  out.clear();
  if (P.any_nlt3 || (P.p.color_transform && !colour_fused(P))) return;   // those conversions live in the conversion kernels
  const bool gfused = general_fused(P);
  // each plane is converted in its own format (desc.reserved); the launch is validated against the deepest of them, not
  // against component 0's, which may not be in the batch at all
  auto note_format = [&](LevelBatch& b, const CompGeo& g) {
    if (g.bit_depth > b.img_depth) { b.img_depth = g.bit_depth; b.img_signed = g.is_signed ? 1 : 0; }
  };
  auto image_desc = [&](const ojphgpu_level_info& lv, ojphgpu_dwt_desc d) {
    const TileComp& tc = P.tcomps[P.tiles[lv.tile].comps[lv.comp]];
    const CompGeo& g = P.comps[lv.comp];
    const Rect& rr = P.ress[tc.res[lv.res]].r;              // the tile-component at the reconstructed resolution
    d.src_off = g.frame_off + (uint64_t)(rr.y0 - g.y0) * g.w + (rr.x0 - g.x0);
    d.src_pitch = g.w;
    d.reserved = g.bit_depth | (g.is_signed ? 0x100u : 0u);   // the component's sample format for the fused conversion
    return d;
  };
  for (LevelBatch& b : batches) {
    if (b.depth == 0 && b.count && b.general && gfused) {    // the general lifting kernels' top level, conversion included
      b.img_first = (int)out.size();
      size_t k = 0;
      for (uint32_t c : b.comps)
        for_levels_of(P, tr, 0, P.style(c).rev, 0, (int)c, [&](const ojphgpu_level_info& lv) {
          note_format(b, P.comps[lv.comp]);
          out.push_back(image_desc(lv, descs[b.first + k++]));
        });
      continue;
    }
    if (b.depth != 0 || b.count == 0 || b.general) continue;
    bool all_shallow = true;                                  // (a batch with a deep component keeps the conversion kernels)
    for_levels_of(P, tr, 0, b.rev, b.group, -1, [&](const ojphgpu_level_info& lv) { all_shallow = all_shallow && !deep(P, lv.comp); });
    if (!all_shallow) continue;
    b.img_first = (int)out.size();
    size_t k = 0;
    for_levels_of(P, tr, 0, b.rev, b.group, -1, [&](const ojphgpu_level_info& lv) {
      ojphgpu_dwt_desc d = descs[b.first + k++];
      const TileComp& tc = P.tcomps[P.tiles[lv.tile].comps[lv.comp]];
      const CompGeo& g = P.comps[lv.comp];
      const Rect& rr = P.ress[tc.res[lv.res]].r;              // the tile-component at the reconstructed resolution
      d.src_off = g.frame_off + (uint64_t)(rr.y0 - g.y0) * g.w + (rr.x0 - g.x0);
      d.src_pitch = g.w;
      d.reserved = g.bit_depth | (g.is_signed ? 0x100u : 0u);   // the component's sample format for the fused conversion
      note_format(b, g);
      out.push_back(d);
    });
  }
}

// One descriptor per tile and component, in that order; a component whose conversion is fused into
// its top DWT level (no colour transform, at least one level) gets an empty one.  Returns whether
// any component is left for the conversion kernels.
bool build_convert_descs(const Plan& P, TileRange tr, std::vector<ojphgpu_convert_desc>& descs, uint32_t& max_w, uint32_t& max_h)
{
  descs.clear(); max_w = max_h = 0;
  bool any = false;
  for (const Tile& t : P.tiles) {
    if (!tr.has(t.idx)) continue;
    for (uint32_t c = 0; c < P.p.num_comps; ++c) {
      const uint32_t L = P.recon_decomps(c);
      const TileComp& tc = P.tcomps[t.comps[c]];
      const Resolution& R = P.ress[tc.res[L]];
      ojphgpu_convert_desc d; memset(&d, 0, sizeof(d));
      if (L == 0) { const Band& B = P.bands[(size_t)R.band[0]]; d.plane_off = B.plane_off; d.pitch = B.pitch; }
      else { d.plane_off = R.plane_off; d.pitch = R.pitch; }
      const CompGeo& g = P.comps[c];
      d.src_x0 = R.r.x0 - g.x0; d.src_y0 = R.r.y0 - g.y0;
      d.img_pitch = g.w; d.img_off = g.frame_off;
      d.fmt = g.bit_depth | (g.is_signed ? 0x100u : 0u) | 0x200u | (P.style(c).rev ? 0x400u : 0u) | (P.nlt3[c] ? 0x800u : 0u) |   // 0x200: bit 10 says which conversion
              (is_wide(P, c) ? 0x1000u : 0u);
      // (a batch of the top DWT level converts its components itself only when none of them is deep: the batch of the
      // component's wavelet, see build_image_level_descs)
      bool batch_deep = false;
      const int grp = colour_fused(P) ? (c < 3 ? 1 : 2) : 0;
      for (uint32_t o = 0; o < P.p.num_comps; ++o)
        batch_deep = batch_deep || (P.style(o).rev == P.style(c).rev && in_group(o, grp) && !P.general(o) && deep(P, o) && P.recon_decomps(o) > 0);
      if ((P.p.color_transform && !colour_fused(P)) || P.any_nlt3 || L == 0 || (P.general(c) && !general_fused(P)) || batch_deep) { d.w = R.r.w; d.h = R.r.h; any |= d.w && d.h; }
      descs.push_back(d);
      max_w = std::max(max_w, d.w); max_h = std::max(max_h, d.h);
    }
  }
  return any;
}

// Region decoders (Plan::has_region): the exact range of a level's output plane, in plane coordinates; the top level writes it
// into the region frame (out_off, out_pitch)
inline ojphgpu_dwt_region region_of_level(const Plan& P, const ojphgpu_level_info& lv, bool top)
{
  const TileComp& tc = P.tcomps[P.tiles[lv.tile].comps[lv.comp]];
  const uint32_t rid = tc.res[lv.res];
  const Rect& E = P.reg_exact[rid]; const Rect& R = P.ress[rid].r;
  ojphgpu_dwt_region r; memset(&r, 0, sizeof(r));
  if (E.w == 0 || E.h == 0) return r;
  r.rx0 = E.x0 - R.x0; r.ry0 = E.y0 - R.y0; r.rx1 = r.rx0 + E.w; r.ry1 = r.ry0 + E.h;
  if (top) {
    const CompGeo& g = P.comps[lv.comp];
    r.out_off = g.frame_off + (uint64_t)(E.y0 - g.y0) * g.w + (E.x0 - g.x0); r.out_pitch = g.w;
  }
  return r;
}

// Keeps the descriptors of the levels whose exact range is not empty and gives each its region; the batches follow (a batch
// left empty goes).  descs / img_descs as build_level_batches / build_image_level_descs made them.
void restrict_levels_to_region(const Plan& P, TileRange tr, std::vector<ojphgpu_dwt_desc>& descs, std::vector<ojphgpu_dwt_desc>& img_descs,
                               std::vector<LevelBatch>& batches, std::vector<ojphgpu_dwt_region>& regs, std::vector<ojphgpu_dwt_region>& img_regs)
{
  std::vector<ojphgpu_dwt_desc> od, oi; std::vector<LevelBatch> ob;
  regs.clear(); img_regs.clear();
  for (const LevelBatch& b : batches) {
    LevelBatch n = b;
    n.first = (uint32_t)od.size(); n.count = 0; n.img_first = b.img_first >= 0 ? (int)oi.size() : -1;
    n.rgrid = ojphgpu::DwtRegionGrid();
    size_t k = 0;
    for_levels_of(P, tr, b.depth, b.rev, b.group, -1, [&](const ojphgpu_level_info& lv) {
      const size_t i = k++;
      const ojphgpu_dwt_region r = region_of_level(P, lv, b.img_first >= 0);
      if (r.rx1 <= r.rx0) return;
      od.push_back(descs[b.first + i]); regs.push_back(r);
      if (b.img_first >= 0) { oi.push_back(img_descs[(size_t)b.img_first + i]); img_regs.push_back(r); }
      ojphgpu::dwt_region_grid_add(n.rgrid, descs[b.first + i], r);
      n.count++;
    });
    if (n.count) ob.push_back(n);
  }
  descs.swap(od); img_descs.swap(oi); batches.swap(ob);
}

// the same regions for every frame of a batch decoder (call before replicate_levels, on the batches it is given)
void replicate_regions(std::vector<ojphgpu_dwt_region>& regs, std::vector<ojphgpu_dwt_region>& img_regs, const std::vector<LevelBatch>& batches,
                       uint32_t nframes, uint64_t frame_elems)
{
  if (nframes <= 1) return;
  std::vector<ojphgpu_dwt_region> out, iout;
  for (const LevelBatch& b : batches)
    for (uint32_t f = 0; f < nframes; ++f)
      for (uint32_t i = 0; i < b.count; ++i) {
        out.push_back(regs[b.first + i]);
        if (b.img_first >= 0) { ojphgpu_dwt_region r = img_regs[(size_t)b.img_first + i]; r.out_off += (uint64_t)f * frame_elems; iout.push_back(r); }
      }
  regs.swap(out); img_regs.swap(iout);
}

// Region decoders: the conversion descriptors of the tiles the region touches (one per component, in that order), each
// moved to the corner of its tile-component's region part and writing into the region frame.  Returns the tiles kept.
uint32_t restrict_converts_to_region(const Plan& P, TileRange tr, std::vector<ojphgpu_convert_desc>& descs, uint32_t& max_w, uint32_t& max_h)
{
  std::vector<ojphgpu_convert_desc> out;
  max_w = max_h = 0;
  uint32_t kept = 0, ti = 0;
  for (const Tile& t : P.tiles) {
    if (!tr.has(t.idx)) continue;
    const size_t base = (size_t)(ti++) * P.p.num_comps;
    if (!P.reg_tiles[t.idx]) continue;
    ++kept;
    for (uint32_t c = 0; c < P.p.num_comps; ++c) {
      ojphgpu_convert_desc d = descs[base + c];
      const TileComp& tc = P.tcomps[t.comps[c]];
      const uint32_t rid = tc.res[P.recon_decomps(c)];
      const Rect& E = P.reg_exact[rid]; const Rect& R = P.ress[rid].r;
      const CompGeo& g = P.comps[c];
      if (d.w && d.h && E.w && E.h) {
        d.plane_off += (uint64_t)(E.y0 - R.y0) * d.pitch + (E.x0 - R.x0);
        d.w = E.w; d.h = E.h;
        d.src_x0 = E.x0 - g.x0; d.src_y0 = E.y0 - g.y0;
        d.img_pitch = g.w; d.img_off = g.frame_off;
      } else d.w = d.h = 0;
      max_w = std::max(max_w, d.w); max_h = std::max(max_h, d.h);
      out.push_back(d);
    }
  }
  descs.swap(out);
  return kept;
}

// Frame batches: the same plan applied to `nframes` independent frames in one set of launches
// (config C5: a batch of independent 4K frames).  Frame f lives f * arena_elems further in the arena
// and f * frame_elems further in the image buffer; descriptors are simply replicated, batch by batch.
void replicate_levels(std::vector<ojphgpu_dwt_desc>& descs, std::vector<ojphgpu_dwt_desc>& img_descs, std::vector<LevelBatch>& batches,
                      uint32_t nframes, uint64_t arena_elems, uint64_t frame_elems)
{
  if (nframes <= 1) return;
  std::vector<ojphgpu_dwt_desc> out, iout; std::vector<LevelBatch> nb;
  for (const LevelBatch& b : batches) {
    LevelBatch n = b;
    n.first = (uint32_t)out.size(); n.count = b.count * nframes;
    if (b.img_first >= 0) n.img_first = (int)iout.size();
    for (uint32_t f = 0; f < nframes; ++f)
      for (uint32_t i = 0; i < b.count; ++i) {
        const uint64_t o = (uint64_t)f * arena_elems;
        ojphgpu_dwt_desc d = descs[b.first + i];
        d.src_off += o; d.ll_off += o; d.hl_off += o; d.lh_off += o; d.hh_off += o;
        out.push_back(d);
        if (b.img_first >= 0) {
          d = img_descs[(size_t)b.img_first + i];
          d.src_off += (uint64_t)f * frame_elems; d.ll_off += o; d.hl_off += o; d.lh_off += o; d.hh_off += o;
          iout.push_back(d);
        }
      }
    nb.push_back(n);
  }
  descs.swap(out); img_descs.swap(iout); batches.swap(nb);
}

void replicate_converts(std::vector<ojphgpu_convert_desc>& descs, uint32_t nframes, uint64_t arena_elems, uint64_t frame_elems)
{
  if (nframes <= 1 || descs.empty()) return;
  const size_t n = descs.size();
  for (uint32_t f = 1; f < nframes; ++f)
    for (size_t i = 0; i < n; ++i) {
      ojphgpu_convert_desc d = descs[i];
      d.plane_off += (uint64_t)f * arena_elems; d.img_off += (uint64_t)f * frame_elems;
      descs.push_back(d);
    }
}

// plan-order indices of the code-blocks that belong to the tile range
std::vector<uint32_t> blocks_of_tiles(const Plan& P, TileRange tr)
{
  std::vector<uint32_t> ids;
  for (size_t i = 0; i < P.blocks.size(); ++i) {
    const Band& B = P.bands[P.blocks[i].band];
    if (P.has_region && !P.reg_blocks[i]) continue;          // a region decoder: the blocks the region depends on
    if (tr.has(B.tile) && B.res <= P.top_read_res(B.comp)) ids.push_back((uint32_t)i);   // resolutions above are not decoded: their bands stay zero
  }
  return ids;
}

// Timing of one run_device: every launch (or group of launches) is bracketed by a pair of HIP events
// on the stream it is issued on -- launches of one run may sit on two streams -- and tagged with a
// kind; per-kind sums and the wall time of the whole run are read back afterwards.
struct Spans {
  struct Span { hipEvent_t a, b; int kind; };
  std::vector<Span> pool;            // events are created once and reused
  size_t used = 0;
  hipEvent_t t0 = nullptr, t1 = nullptr, t2 = nullptr;
  bool ok = false;
  bool detail = true;                // per-launch spans on; off = only the wall time of the run (two events)
  bool two = false;                  // the run ended on two streams (an encoder's released run): t1 and t2, the later one counts
  int init() { ok = hipEventCreate(&t0) == hipSuccess && hipEventCreate(&t1) == hipSuccess && hipEventCreate(&t2) == hipSuccess; return ok ? 0 : -1; }
  void destroy() {
    for (Span& x : pool) { (void)hipEventDestroy(x.a); (void)hipEventDestroy(x.b); }
    if (t0) (void)hipEventDestroy(t0);
    if (t1) (void)hipEventDestroy(t1);
    if (t2) (void)hipEventDestroy(t2);
    pool.clear();
  }
  void start(hipStream_t s) { used = 0; two = false; if (ok) (void)hipEventRecord(t0, s); }
  void finish(hipStream_t s) { if (ok) (void)hipEventRecord(t1, s); }
  void finish_two(hipStream_t s, hipStream_t other) { finish(s); two = ok; if (ok) (void)hipEventRecord(t2, other); }
  int begin(int kind, hipStream_t s) {
    if (!ok || !detail) return -1;
    if (used == pool.size()) {
      Span x{ nullptr, nullptr, kind };
      if (hipEventCreate(&x.a) != hipSuccess || hipEventCreate(&x.b) != hipSuccess) { ok = false; return -1; }
      pool.push_back(x);
    }
    pool[used].kind = kind;
    (void)hipEventRecord(pool[used].a, s);
    return (int)used++;
  }
  void end(int id, hipStream_t s) { if (ok && id >= 0) (void)hipEventRecord(pool[(size_t)id].b, s); }
  // sum of the spans of `kind`; kind < 0: wall time of the run
  int read(int kind, float* out) {
    if (!ok || hipEventSynchronize(t1) != hipSuccess) return -1;
    if (kind < 0) {
      if (hipEventElapsedTime(out, t0, t1) != hipSuccess) return -1;
      float other = 0;
      if (two && (hipEventSynchronize(t2) != hipSuccess || hipEventElapsedTime(&other, t0, t2) != hipSuccess)) return -1;
      *out = std::max(*out, other);
      return 0;
    }
    float sum = 0;
    for (size_t i = 0; i < used; ++i)
      if (pool[i].kind == kind) { float ms = 0; if (hipEventElapsedTime(&ms, pool[i].a, pool[i].b) != hipSuccess) return -1; sum += ms; }
    *out = sum;
    return 0;
  }
  // the individual spans of `kind`, in issue order
  int read_each(int kind, float* out, uint32_t cap) {
    if (!ok || hipEventSynchronize(t1) != hipSuccess) return -1;
    int n = 0;
    for (size_t i = 0; i < used; ++i)
      if (pool[i].kind == kind && (uint32_t)n < cap) { if (hipEventElapsedTime(&out[n], pool[i].a, pool[i].b) != hipSuccess) return -1; ++n; }
    return n;
  }
};
enum { SP_CONVERT = 0, SP_DWT = 1, SP_HT_ENC = 2, SP_PREP = 3, SP_STEP1 = 4, SP_STEP2 = 5, SP_REFINE = 6, SP_STATS = 7 };

}  // namespace

// What an encoder with a byte budget keeps (include/ojphgpu.h section 5b; made by the first ojphgpu_encoder_set_budget(s));
// stats_descs / hist / h_hist / quant hold a part per frame of the encoder
struct EncoderRate {
  RateTable table;                                 // the quantisation of every class of bands at every step of the grid
  DeviceBuf stats_descs, hist, block_class, quant;
  uint32_t n_stats = 0, stats_max_w = 0, stats_max_h = 0;
  std::vector<uint32_t> h_hist;
  std::vector<BandQuant> h_quant;                  // the rows of `table` a round uploads, one per frame
  std::vector<ojphgpu_cb_desc> bd;                 // the block descriptors at the plan's own step (what budget 0 puts back)
  bool searched = false; int search_rc = 0;        // the last run has been searched, with this verdict
  double search_ms = 0, wait_ms = 0, final_ms = 0;
  // The search of a run (ojphgpu_rate_rounds: per frame its verdict and what it found) and per frame the encoder's plan at
  // the step the device results stand at: what Tier-2 writes from.  The plan copies are kept by grid index across runs --
  // the frames of a sequence settle on a handful of indices.
  ojphgpu_rate_rounds* rounds = nullptr;
  std::vector<ojphgpu_plan*> frame_plan;           // (owned by plans)
  std::map<uint32_t, ojphgpu_plan*> plans;
  ~EncoderRate() {
    for (DeviceBuf* b : { &stats_descs, &hist, &block_class, &quant }) b->release();
    for (auto& kv : plans) delete kv.second;
    ojphgpu_rate_rounds_destroy(rounds);
  }
};

// What an encoder with a quality target keeps on top of that (section 5c; made by the first ojphgpu_encoder_set_quality).
// The final coding of j* goes through the byte budget's trial machinery, so such an encoder has an EncoderRate as well.
struct ojphgpu_decoder;
struct EncoderQuality {
  ojphgpu_decoder* syn = nullptr;                  // synthesis-only decoder made from the encoder's plan; its arena is the second arena
  DeviceBuf recon, descs, comps, err;              // the reconstructed frame, the requantise / component descriptors, the trial's figures
  std::vector<uint32_t> desc_band;                 // band of the plan behind each requantise descriptor (the non-empty ones)
  std::vector<ojphgpu_requant_desc> h_descs;
  uint32_t max_w = 0, max_h = 0;
  const void* frame = nullptr; int container = 0;  // the caller's frame of the last run: the search compares against it
  std::vector<ojphgpu_frame_err> h_err, best;      // per component: of the last trial, of j*
  std::vector<std::vector<ojphgpu_frame_err>> by_index;   // the figures of every index tried in this search
  bool have_info = false;
  ojphgpu_quality_info info;
  // under a byte cap (ojphgpu_encoder_set_quality_capped): what the last capped finish found, and the index the device holds
  bool have_capped = false;
  ojphgpu_capped_info capped;
  int coded_at = -1;
  int hist_rc = 0;                                 // of the statistics pass of that search, when the cap bound (encoder_capped_hist)
  double search_ms = 0, wait_ms = 0, final_ms = 0;
  ~EncoderQuality();
};

// What an encoder that codes reversible frames under a byte cap keeps (include/ojphgpu.h section 5f; made by the first
// ojphgpu_encoder_set_truncation / _set_trunc_level)
struct EncoderTrunc {
  TruncLadder ladder;
  DeviceBuf block_class, drop, stats_descs, hist;  // the blocks' classes, a table (a byte per class), the integer statistics
  uint32_t n_stats = 0, stats_max_w = 0, stats_max_h = 0;
  std::vector<uint32_t> h_hist;
  std::vector<uint8_t> h_drop, band_drop;          // per class: the table being uploaded; per band: the table the device results stand at
  bool searched = false; int search_rc = 0;        // the last run has been coded, with this verdict
  bool have_info = false;
  ojphgpu_trunc_info info;
  double search_ms = 0;                            // host clock of the last finish's coding: every trial, and j* once more
  ~EncoderTrunc() { for (DeviceBuf* b : { &block_class, &drop, &stats_descs, &hist }) b->release(); }
};

struct ojphgpu_encoder {
  const ojphgpu_plan* handle = nullptr;
  const Plan* P = nullptr;
  int device = 0; hipStream_t stream = nullptr;
  // out / counters are null in the encoder of a frame pipeline with a byte budget: the pipe takes them over as its spare
  // output set (ojphgpu_enc_pipe_set_budget); one with a quality target codes every frame once, into its slot's set, and
  // releases them (ojphgpu_enc_pipe_set_quality).  Such an encoder runs only through o_out / o_results / o_counters,
  // ojphgpu_encoder_rate_trial and ojphgpu_encoder_quality_trial; _finish, _coded_bytes and the encoder's own searches,
  // which read these two, are not for it.
  DeviceBuf arena, image, dwt_descs, img_descs, cb_descs, conv_descs, scratch, out, results, counters;
  bool need_convert = false;                       // some component is not converted inside its top DWT level
  std::vector<LevelBatch> batches;
  uint32_t conv_max_w = 0, conv_max_h = 0, out_cap = 0;
  TileRange tiles{ 0, 0 };
  uint32_t nframes = 1;                            // frames coded per run_device (batch)
  bool fetched = false;                            // results / bytes of the last run are on the host
  uint64_t nbytes = 0;
  std::vector<uint32_t> block_ids;                 // plan-order index of each block this encoder codes (per frame)
  std::vector<ojphgpu_cb_result> h_results;
  HostBuf h_out, h_res;
  Spans timer;
  bool ran = false;
  // overlap of the block coder with the lower DWT levels: the blocks of the top resolution (3/4 of
  // the samples) only need the first DWT level, so they are coded on a second stream while the
  // small, latency-bound launches of levels 2..L run on the main one
  // The cut is a pair, one per schedule (EncoderCut): a joined run wants the side launch to end first, a released run -- whose
  // branches nobody waits for -- measures best with about half of the top resolution on either stream.  A block's output
  // region goes by its index among ALL blocks (encoder_block_layout), so the products do not depend on the cut and
  // run_container takes the pair of the run it is about to make.  n_top / widths_*: the cut of the last run; before any run,
  // of the schedule the next run would take.
  uint32_t n_top = 0;                              // descriptors [0, n_top) = the side launch's blocks (all of the top resolution)
  int widths_top = 0, widths_rest = 0;             // which block encoder kernels each range needs (bit 0 narrow, bit 1 wide, bit 2 reversible, bit 3 irreversible)
  struct EncoderCut { uint32_t n_top = 0; int widths_top = 0, widths_rest = 0; } cut_joined, cut_released;
  void take_cut(const EncoderCut& c) { n_top = c.n_top; widths_top = c.widths_top; widths_rest = c.widths_rest; }
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // A released run (include/ojphgpu.h section 5, "what a run leaves"): behind the last launch that reads the caller's frame
  // nothing of an encode touches the caller's memory, so the rest is issued on streams of the object's own -- the top
  // resolution's blocks on `side`, levels 2..L and the other blocks on `low` -- and the caller's stream is NOT made to wait
  // for them at the end of the run: `pending` says that ev_join / ev_low are still to be waited for, and whatever reads or
  // overwrites the products (out, results, counters, arena, scratch) calls encoder_settle() first.  Only a plain
  // single-frame run into the object's own buffers with per-launch timing off is released (encoder_releases()).
  // low / ev_low exist only where can_release holds (encoder_create): an object whose runs always end joined holds the one
  // side stream it always had, at the caller's priority.
  hipStream_t low = nullptr;
  hipEvent_t ev_low = nullptr;
  bool pending = false, can_release = false;
  bool stream_wrote = false;                       // the set's counters were last counted in by launches on the caller's stream (a joined or searching run)
  // Two product sets (two_sets; only where can_release holds, OJPHGPU_ENC_SETS=1 at creation: one).  What a run produces and
  // the coder reads -- arena, out, results, counters -- with the set's own ev_join / ev_low / pending exists twice, so that
  // the transform of run n + 1 need not wait for the block coder of run n.  arena / out / results / counters / ev_join /
  // ev_low / pending above are ALWAYS the set of the last run (what every accessor reads); `other` is the set of the run
  // before it.  A released run begins by exchanging the two (encoder_next_set) and waits, on the caller's stream, only for
  // the set it then holds -- the run two back.  Every other run, and everything that reads or replaces products, waits for
  // both (encoder_settle) and uses the set of the last run.  Both sets always have the same sizes (encoder_rate_setup).
  // `scratch` stays single: a block's slot is touched only by the launch that codes the block; released runs all use
  // cut_released, so in consecutive released runs that launch sits on the same in-order stream (side or low); any other run
  // settles both sets first, and the next released run's launches sit on streams that wait for a fork event recorded on the
  // caller's stream behind that run.
  struct OtherSet {
    DeviceBuf arena, out, results, counters;
    hipEvent_t ev_join = nullptr, ev_low = nullptr;
    bool pending = false, stream_wrote = false;
  } other;
  bool two_sets = false;
  // the counter clear of a released run goes on `side` (BlockCoderRun::clear_released), `low` waits for ev_clear
  hipEvent_t ev_clear = nullptr;
  bool clear_on_side = false;
  // where a run writes its products: the object's own buffers (null), or -- for a frame pipeline that keeps
  // several frames in flight -- the buffers of the frame's slot (ojphgpu_pipe.cpp)
  void* o_out = nullptr; void* o_results = nullptr; void* o_counters = nullptr;
  // The compacted output is split into nreg regions with a cursor each (block i allocates in region i % nreg), so
  // that the blocks' allocation atomics do not all queue on one cache line (claim_output, kernels_ht_enc.hip).
  // h_regions[2r] = first byte, [2r + 1] = capacity; counters: word 32 r = cursor of region r, word 1 = status.
  uint32_t nreg = 0;
  std::vector<uint32_t> h_regions, h_cursors;
  DeviceBuf regions;
  size_t counters_bytes = 16;
  std::vector<uint64_t> budgets;                   // one per frame: frame f of every run is coded to budgets[f]; empty: off
  EncoderRate* rate = nullptr;
  bool quality_on = false; uint64_t max_sse = 0;   // every frame is coded to this quality target (never together with a budget)
  uint64_t cap_bytes = 0;                          // ... and under this byte cap (0: none; ojphgpu_encoder_set_quality_capped)
  EncoderQuality* quality = nullptr;
  // the blocks are coded by a search in ojphgpu_encoder_finish*, and Tier-2 writes from the search's plan
  bool searches() const { return !budgets.empty() || quality_on; }
  // section 5f: reversible frames under a byte cap (trunc_bytes) or at a fixed level of the ladder (trunc_level >= 0); the
  // blocks are coded in ojphgpu_encoder_finish, Tier-2 writes from the encoder's own plan with the table's missing_msbs
  bool trunc_on = false; uint64_t trunc_bytes = 0; int32_t trunc_level = -1;
  EncoderTrunc* trunc = nullptr;
};
// May the next run of e be released?  Not one that writes into a frame pipe's slot (the pipe records its own hand-over
// events behind the run), not a searching one (the search goes on reading the arena on the caller's stream), and not with
// per-launch timing on (the spans of a run are read as parts of one total).  Frame batches, tile ranges without a side
// launch, blocks-only encoders, OJPHGPU_NO_OVERLAP=1 and OJPHGPU_ENC_RELEASE=0 never can (can_release).
inline bool encoder_releases(const ojphgpu_encoder* e)
{
  return e->can_release && e->cut_released.n_top && !e->o_out && !e->o_results && !e->o_counters && !e->searches() && !e->trunc_on && !e->timer.detail;
}
// The stream-level join of a released run: e->stream waits for the branches' done events (no host synchronisation).
// Called before anything is enqueued on e->stream -- or e->stream is synchronised -- to read or overwrite the products.
inline int encoder_settle_last(ojphgpu_encoder* e)          // the set of the last run only
{
  if (!e->pending) return OJPHGPU_OK;
  HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join, 0));
  HIPCHK(hipStreamWaitEvent(e->stream, e->ev_low, 0));
  e->pending = false;
  return OJPHGPU_OK;
}
inline int encoder_settle(ojphgpu_encoder* e)               // every pending set
{
  if (e->other.pending) {
    HIPCHK(hipStreamWaitEvent(e->stream, e->other.ev_join, 0));
    HIPCHK(hipStreamWaitEvent(e->stream, e->other.ev_low, 0));
    e->other.pending = false;
  }
  return encoder_settle_last(e);
}
// A released run of an object with two sets takes the set the last run did not use: afterwards arena / out / ... are that
// set -- still pending if the run two back has not been waited for -- and `other` is the last run's.
inline void encoder_next_set(ojphgpu_encoder* e)
{
  if (!e->two_sets) return;
  std::swap(e->arena, e->other.arena); std::swap(e->out, e->other.out);
  std::swap(e->results, e->other.results); std::swap(e->counters, e->other.counters);
  std::swap(e->ev_join, e->other.ev_join); std::swap(e->ev_low, e->other.ev_low);
  std::swap(e->pending, e->other.pending); std::swap(e->stream_wrote, e->other.stream_wrote);
}
// Where one trial of the budget search writes, and how its block lengths reach the host.  h_results != null: d_results is the
// device address of that mapped pinned memory, the coder's records land in it, the two status words of d_counters are
// published to d_publish (h_publish on the host) and `done` is recorded behind them and waited for.  Null: the records are
// copied into the encoder's own pageable table.
struct RateTrialOut {
  void* out; ojphgpu_cb_result* d_results; uint32_t* d_counters;
  const ojphgpu_cb_result* h_results; uint32_t* d_publish; const uint32_t* h_publish; hipEvent_t done;
};
// a single-frame encoder's blocks coded at grid index j into `o`, Q left at that step: size(j), or an error (< 0)
int64_t ojphgpu_encoder_rate_trial(ojphgpu_encoder* e, Plan& Q, const RateTrialOut& o, uint32_t j);
// What one trial of the quality search compares against, and how its small data travel.  frame / container: the original,
// on the device.  h_descs != null: mapped pinned memory the requantise descriptors are written into (d_descs: its device
// address; a copy kernel takes them to the device), the error words (one ojphgpu_frame_err per component) are written to
// d_err (h_err on the host) by a copy kernel and `done` is recorded behind them and waited for.  Null: copies from and into
// the encoder's own pageable tables.
struct QualityTrialIo {
  const void* frame; int container;
  ojphgpu_requant_desc* h_descs; const void* d_descs;
  const ojphgpu_frame_err* h_err; void* d_err; hipEvent_t done;
};
int ojphgpu_encoder_quality_trial(ojphgpu_encoder* e, const QualityTrialIo& io, uint32_t j, ojphgpu_frame_err* comps);   // comps[component] = SSE / PAE at j
// the device part of an encode: d_image holds the frame in `container`-bit elements (32 / 16)
int ojphgpu_encoder_run_container(ojphgpu_encoder* e, const void* d_image, int container);
// ojphgpu_encoder_create for an owner whose runs never release (a frame pipe): no second stream, the side stream as before
int ojphgpu_encoder_create_joined(const ojphgpu_plan* plan, int device, void* stream, ojphgpu_encoder** out);

// The plan-order coded-block table of one frame from the block coder's results: res[i] = the frame's block block_ids[i];
// P = the plan the blocks were quantised with (its bands give K_max); blocks outside block_ids stay empty.  band_drop
// (section 5f; null: none): the bit-planes the blocks of every band of the plan were coded without
inline void ojphgpu_coded_blocks(const Plan& P, const std::vector<uint32_t>& block_ids, const ojphgpu_cb_result* res,
                                 std::vector<ojphgpu_coded_block>& cb, const uint8_t* band_drop = nullptr)
{
  cb.assign(P.blocks.size(), ojphgpu_coded_block{ 0, 0, 0, 0, 0 });
  for (size_t i = 0; i < block_ids.size(); ++i) {
    const ojphgpu_cb_result& r = res[i];
    ojphgpu_coded_block& c = cb[block_ids[i]];
    c.offset = r.offset; c.len1 = r.length; c.len2 = 0;
    const uint32_t band = P.blocks[block_ids[i]].band;
    c.missing_msbs = r.length ? P.bands[band].K_max - 1 - (band_drop ? band_drop[band] : 0u) : 0;   // ojph_codeblock.cpp:148
    c.num_passes = r.length ? 1 : 0;
  }
}

// A block the reference decodes from bytes the codestream does not hold (Plan::padded: its tile-part ended early and
// bb_read_chunk, ojph_bitbuffer_read.h:134-150, handed over zeros for the rest): `got` bytes at `src` of the codestream,
// then zeros up to `total`, placed at `dst` -- an offset into the frame's part of the device data buffer, BEHIND the byte
// range that is uploaded as it is.
struct PadCopy { uint64_t src, dst; uint32_t got, total; };
// a run of decoded blocks adjacent in the codestream: n bytes at src, placed at dst of the frame's staged bytes (64 zero bytes
// on either side: the VLC partner's 16-byte loads)
struct DecRun { uint64_t src, dst, n; };
struct ojphgpu_decoder {
  const Plan* P = nullptr;
  int device = 0; hipStream_t stream = nullptr;
  DeviceBuf arena, image, dwt_descs, img_descs, cb_descs, conv_descs, data, status, quads, aux;
  DeviceBuf fstate; uint32_t fused_epoch = 0, max_block_h = 0;     // the fused step 1 + step 2 launch: its flags / per-block state, run counter
  uint32_t cus = 256;                               // compute units of `device` (the fused launch is shaped for them)
  // A fused launch whose workers gave up waiting (a chip held up for seconds by other work) marks the run in the RETRY word
  // behind the block status array; whoever collects the run's verdicts (ojphgpu_decoder_failed_blocks, the decoder pipe)
  // then repeats the run through the separate launches: last_* is what that repeat needs.
  bool last_fused = false, force_separate = false;
  void* last_image = nullptr; int last_container = 0;
  uint32_t fused_retries = 0;                       // runs repeated that way so far
  // A caller of ojphgpu_decoder_run_device that never collects its runs would never learn that one asked for a repeat: the
  // fused launch also writes the run's epoch into h_retry -- a word of mapped host memory (d_h_retry: its device address) --
  // and the next run of this object finds it there (OJPHGPU_E_UNCOLLECTED).  uncollected: a fused run has been enqueued
  // and nobody has read its verdicts yet.
  uint32_t* h_retry = nullptr; uint32_t* d_h_retry = nullptr; bool uncollected = false;
  uint32_t retry_acked = 0;                         // the newest epoch found in h_retry that has been reported or collected
  // eight repeats in a row and the object stops using the one launch: a wait that runs out costs seconds, and a chip (or a
  // device layout) on which it keeps running out is better served by the separate launches than by trying again
  uint32_t fused_strikes = 0; bool fused_off = false;
  void fused_outcome(bool repeated) { if (!repeated) fused_strikes = 0; else if (++fused_strikes >= 8u) fused_off = true; }
  // descriptors [0, n_low) = blocks below the top resolution (0 = no overlap of the lower synthesis
  // levels with step 2, see decoder_create)
  uint32_t n_low = 0;
  hipStream_t side = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool need_convert = false;                       // some component is not converted inside its top DWT level
  TileRange tiles{ 0, 0 };
  uint32_t nframes = 1;
  bool any_refine = false;                         // some block carries SigProp / MagRef passes
  int kinds = 0;                                   // block kinds of the frame(s), for ht_decode_step2_launch
  std::vector<size_t> f_first, f_len, f_base;      // per frame: codestream byte range uploaded, its place in `data`
  std::vector<std::vector<PadCopy>> f_pads;        // per frame: blocks uploaded with zeros behind their bytes (PadCopy)
  // region decoders (Plan::has_region): the frame's bytes are the runs of its decoded blocks (DecRun), gathered into the pinned
  // h_stage and copied at once; f_len = the bytes staged.  DWT descriptors get their regions (dwt_regs, img_regs) and the
  // conversion kernels take conv_tiles tiles per frame
  bool region = false;
  std::vector<std::vector<DecRun>> f_runs;
  uint8_t* h_stage = nullptr; size_t stage_cap = 0;
  hipEvent_t ev_stage = nullptr;                   // recorded behind the copy out of h_stage: an upload waits for it, not for runs
  DeviceBuf dwt_regs, img_regs;
  uint32_t conv_tiles = 0, tiles_touched = 0;
  uint32_t nblocks = 0;                            // code-blocks of the tile range (all frames)
  std::vector<LevelBatch> batches;
  uint32_t conv_max_w = 0, conv_max_h = 0, max_len1 = 0;
  size_t data_first = 0, data_len = 0;              // byte range of the codestream holding this range's block data
  Spans timer;
  bool ran = false;
  std::vector<uint32_t> block_ids;                 // plan-order index of each block descriptor (per frame)
  // what a run reads: the object's own buffers (null), or those of a frame pipeline's slot
  const void* o_cb_descs = nullptr; const void* o_data = nullptr; void* o_status = nullptr;
  // the decoder half of a transcoder (section 5d): the block decoder alone -- no level batches, no conversion, no frame; a
  // run ends with the sub-band planes in the arena
  bool blocks_only = false;
  // A released run (include/ojphgpu.h, ojphgpu_decoder_run_device): nothing in the block decoder and in synthesis levels
  // L..2 touches the caller's memory -- they read the object's codestream bytes and descriptors and read and write its
  // arena, records and status -- so a run that decoder_releases() admits issues the block launch (with ahead_levels:
  // levels L..2 as well) on `side`, the object's own stream, and the caller's stream waits for ev_done, recorded behind
  // them, in front of the first level it runs itself.  The uploads of
  // such an object go on `side` too (ev_up lets the caller's stream follow), in order with the block launches that read
  // `data`.  pending: ev_done has been recorded and nothing but the run itself has waited for it; whatever reads the status
  // or the arena on the caller's stream, or frees anything, calls decoder_settle() first.
  // Two arenas (two_arenas; OJPHGPU_DEC_SETS=1 at creation: one): released runs alternate, `arena` is ALWAYS the last
  // run's, `arena2` the one before it.  ev_read / ev_read2: recorded on the caller's stream behind the last synthesis
  // that read arena / arena2; `side` waits for the event of the arena it is about to write -- the run two back -- and,
  // behind a joined run (last_joined: its block launches used quads / fstate / data on the caller's stream), for that run's
  // as well.  quads, fstate, status and aux stay single: the block launches of released runs sit on one in-order stream.
  bool can_release = false, pending = false, two_arenas = false, last_joined = false;
  bool ahead_levels = false;                       // OJPHGPU_DEC_AHEAD_LEVELS=1: levels L..2 of a released run go with the block launch (default: they stay on the caller's stream)
  DeviceBuf arena2;
  hipEvent_t ev_done = nullptr, ev_up = nullptr, ev_read = nullptr, ev_read2 = nullptr;
};
// May the next run of d be released?  A single-frame decoder with a side stream whose block decoder is the one launch,
// into its own buffers (not a pipe's slot), whole frames (no region, not a transcoder's half), with per-launch timing off
// (the spans of a run are read as parts of one total).  can_release: what was settled at creation -- made through the
// public single-frame create, fusing then, not under OJPHGPU_NO_OVERLAP=1 / OJPHGPU_DEC_RELEASE=0.
bool decoder_fuses(const ojphgpu_decoder* d);
inline bool decoder_releases(const ojphgpu_decoder* d)
{
  return d->can_release && d->nframes == 1 && d->n_low != 0 && d->side && decoder_fuses(d) && !d->o_cb_descs && !d->o_data && !d->o_status &&
         !d->blocks_only && !d->region && !d->force_separate && !d->timer.detail;
}
// The stream-level join of a released run: d->stream waits for what the own stream holds (no host synchronisation).
inline int decoder_settle(ojphgpu_decoder* d)
{
  if (!d->pending) return OJPHGPU_OK;
  HIPCHK(hipStreamWaitEvent(d->stream, d->ev_done, 0));
  d->pending = false;
  return OJPHGPU_OK;
}
// the own stream gets behind a joined run of the object (its block launches and synthesis on the caller's stream)
inline int decoder_own_follows_joined(ojphgpu_decoder* d)
{
  if (!d->last_joined) return OJPHGPU_OK;
  HIPCHK(hipStreamWaitEvent(d->side, d->ev_read, 0));
  d->last_joined = false;
  return OJPHGPU_OK;
}
// ojphgpu_decoder_create for an owner whose runs never release (a frame pipe, a multi-device decoder): one arena, the
// uploads on the caller's stream
int ojphgpu_decoder_create_joined(const ojphgpu_plan* plan, int device, void* stream, uint32_t tile_first, uint32_t tile_count, ojphgpu_decoder** out);
// A transcoder: the block decoder of the source plan and the block coder of the output plan on the decoder's arena (the
// encoder is created without one and borrows it: enc->arena.p is not the encoder's to free)
struct ojphgpu_transcoder {
  ojphgpu_decoder* dec = nullptr; ojphgpu_encoder* enc = nullptr;
  const Plan* S = nullptr; const Plan* O = nullptr;
  int device = 0; hipStream_t stream = nullptr;
  std::vector<ojphgpu_cb_desc> h_descs;            // this frame's block descriptors
  int stage = 0;                                   // 0 idle, 1 submitted, 2 collected and coded (a finish may be repeated)
  bool resilient = false;                          // how the submitted source was parsed
  uint32_t failed = 0;
  double code_ms = 0, final_ms = 0;
};
// A recoder (section 5e): a whole decoder of the source plan -- under its view, if it has one -- and a whole encoder of the
// output plan, with one int32 frame and the fit between them.  Both halves are the objects anybody else gets; what the
// recoder adds is that a later source's descriptors replace the first one's in the decoder (as a decoder pipe's slots do).
struct ojphgpu_recoder {
  ojphgpu_decoder* dec = nullptr; ojphgpu_encoder* enc = nullptr;
  const Plan* S = nullptr; const Plan* O = nullptr;
  int device = 0; hipStream_t stream = nullptr;
  DeviceBuf frame, fitted, comps;                  // F (int32; at 32 bits also G, fitted in place), G in a narrower container or resampled, the stage's components
  int container = 32; uint32_t ncomps = 0;
  bool resampled = false;                          // comps holds ojphgpu_resample_comp: the stage is ojphgpu_frame_resample, G the output's layout
  std::vector<ojphgpu_cb_desc> h_descs;            // this source's block descriptors
  std::vector<uint8_t> h_stage;                    // a view's runs, gathered for one copy
  hipEvent_t ev_fit0 = nullptr, ev_fit1 = nullptr;
  int stage = 0;                                   // 0 idle, 1 submitted, 2 collected (a finish may be repeated)
  bool resilient = false;
  uint32_t failed = 0;
  double final_ms = 0;
  void* g() const { return container == 32 && !resampled ? frame.p : fitted.p; }
};
struct DecFrameInfo;
// How the status bytes of a run (+ the RETRY word behind them) reach the host for whoever collects its verdicts: called once
// the run is enqueued, returns with them readable at *h_status
typedef int (*ojphgpu_status_fetch)(void* user, const uint8_t** h_status);
// ojphgpu_decoder_failed_blocks with the fetch of the caller's choice (a frame pipeline's: a copy kernel into pinned memory)
int ojphgpu_decoder_collect(ojphgpu_decoder* d, ojphgpu_status_fetch fetch, void* user, uint32_t* count);
// What one source needs of a transcoder, piece by piece (ojphgpu_codec.cpp, above ojphgpu_transcoder_submit): shared by the
// single transcoder's two calls and the transcode pipe
int ojphgpu_transcoder_check_source(const ojphgpu_transcoder* t, const Plan& Q);
int ojphgpu_transcoder_fill_descs(const ojphgpu_transcoder* t, const Plan& Q, size_t cs_len, ojphgpu_cb_desc* bd, DecFrameInfo& fi);
int ojphgpu_transcoder_decode(ojphgpu_transcoder* t, bool any_refine, int kinds, uint32_t max_len1);
int ojphgpu_transcoder_stats(ojphgpu_transcoder* t);
int ojphgpu_transcoder_verdicts(ojphgpu_transcoder* t, ojphgpu_status_fetch fetch, void* user, bool resilient, uint32_t* failed);
int ojphgpu_transcoder_code(ojphgpu_transcoder* t, void* out, ojphgpu_cb_result* d_results, uint32_t* d_counters);
struct DecFrameInfo {
  std::vector<DecRun> runs;                                  // region decoders: the runs; first = 0, len = the bytes staged
  uint64_t first = 0, len = 0; bool any_refine = false; uint32_t max_len1 = 0; int kinds = 0;   // kinds: see ht_decode_step2_launch; bit 5: blocks on the 64-bit sample path
  std::vector<PadCopy> pads; uint64_t pad_len = 0;         // padded blocks: their copies, the bytes they take behind `len` (rounded up to 64)
  uint64_t data_bytes() const { return ((len + 63) & ~(uint64_t)63) + pad_len; }
};
// enqueues the copies of a frame's padded blocks (d_frame_data = where the frame's byte range starts in device memory)
int ojphgpu_decoder_upload_pads(hipStream_t s, uint8_t* d_frame_data, const uint8_t* h_codestream, size_t cs_len, const std::vector<PadCopy>& pads);
int  ojphgpu_same_frame_geometry(const Plan& P, const Plan& Q, bool compare_blocks);
void ojphgpu_decoder_fill_descs(const Plan& P, const Plan& Q, const std::vector<uint32_t>& ids, uint64_t arena_off,
                                uint64_t data_base, ojphgpu_cb_desc* bd, DecFrameInfo& fi, bool want_runs = false);
int  ojphgpu_decoder_run_container(ojphgpu_decoder* d, void* d_image, int container);
inline EncoderQuality::~EncoderQuality()
{
  for (DeviceBuf* b : { &recon, &descs, &comps, &err }) b->release();
  if (syn) ojphgpu_decoder_destroy(syn);
}
// after a run has completed, with the status bytes + the RETRY word behind them on the host (nblocks bytes, then the word at
// the next multiple of 4): did the fused launch of that run (epoch) ask for a repeat?
inline bool ojphgpu_fused_retry_wanted(const uint8_t* h_status, uint32_t nblocks, uint32_t epoch)
{
  uint32_t w; memcpy(&w, h_status + ((nblocks + 3u) & ~3u), 4);
  return w == epoch;
}


#endif
