// openjph_amd/csrc/ojph_transcode.cpp -- the output plan of a transcode (include/ojphgpu.h section 5d), host only.
//
// A transcoder decodes the code-blocks of a source codestream into the sub-band planes of an arena and codes the blocks of
// another plan from the same planes.  assign_planes (ojph_plan.cpp) places a band by its size alone, so the code-block size,
// the precincts, the progression order, TLM and the tile-part divisions of the output may differ from the source's and the
// planes stay where they are; everything that moves a sample -- the frame, the tiles, the components, the wavelet, the
// decompositions, the colour transform -- may not.
#include <cstring>
#include <memory>

#include "ojph_plan.h"

namespace ojphgpu {

bool transcode_plans_fit(const Plan& S, const Plan& O)
{
  if (S.coded.size() != S.blocks.size()) return false;                       // the source comes from ojphgpu_t2_parse
  if (O.coded.size() == O.blocks.size() && !O.blocks.empty()) return false;  // ... and the output does not
  for (const Plan* P : { &S, &O }) {
    if (P->skip_read || P->skip_recon || P->has_region || P->no_packets) return false;
    if (P->any_wide || !P->atks.empty() || !P->dfss.empty()) return false;
    for (uint32_t c = 0; c < P->p.num_comps; ++c) if (P->general(c) || P->style(c).causal) return false;
  }
  if (S.p.num_comps != O.p.num_comps || S.arena_elems != O.arena_elems || S.bands.size() != O.bands.size() ||
      S.tiles.size() != O.tiles.size()) return false;
  for (uint32_t c = 0; c < S.p.num_comps; ++c) {
    const CodStyle& a = S.style(c); const CodStyle& b = O.style(c);
    if (a.rev != b.rev || a.L != b.L) return false;
  }
  for (size_t i = 0; i < S.bands.size(); ++i) {
    const Band& a = S.bands[i]; const Band& b = O.bands[i];
    if (a.tile != b.tile || a.comp != b.comp || a.res != b.res || a.band != b.band || memcmp(&a.r, &b.r, sizeof(Rect)) != 0 ||
        a.plane_off != b.plane_off || a.pitch != b.pitch || a.empty != b.empty) return false;
    // a reversible band is coded as it was decoded: the output's K_max has to hold the source's magnitudes (a foreign
    // source may carry more guard bits than this library writes)
    if (S.style(a.comp).rev && b.K_max < a.K_max) return false;
  }
  return true;
}

}  // namespace ojphgpu

using namespace ojphgpu;

extern "C" int ojphgpu_plan_create_transcode(const ojphgpu_plan* src, const ojphgpu_params* out_params, ojphgpu_plan** out)
{
  if (!src || !out_params || !out) return OJPHGPU_E_INVALID;
  *out = nullptr;
  return no_throw([&]() -> int {
    const Plan& S = src->plan;
    if (S.coded.size() != S.blocks.size()) return OJPHGPU_E_INVALID;
    // whatever may change is taken out of the comparison; the rest is the source's, bit for bit (the caller starts from
    // ojphgpu_plan_params(src))
    ojphgpu_params a = S.p, b = *out_params;
    for (ojphgpu_params* p : { &a, &b }) {
      p->block_w = p->block_h = 0; p->precinct_w = p->precinct_h = 0; memset(p->precinct_exps, 0, sizeof(p->precinct_exps));
      p->prog_order = 0; p->tlm = 0; p->reserved[1] = 0; p->qstep = 0.0f;
    }
    if (memcmp(&a, &b, sizeof(a)) != 0) return OJPHGPU_E_INVALID;
    if (out_params->reserved[2]) return OJPHGPU_E_INVALID;                     // quality factors
    for (uint32_t c = 0; c < OJPHGPU_MAX_COC_COMPS; ++c) if (out_params->qcc_qfactor[c]) return OJPHGPU_E_INVALID;
    if (plan_all_reversible(S) && out_params->qstep > 0.0f) return OJPHGPU_E_INVALID;   // a step with nothing to quantise
    std::unique_ptr<ojphgpu_plan> h(new ojphgpu_plan());
    const int rc = build_plan(*out_params, h->plan);
    if (rc != OJPHGPU_OK) return rc;
    if (!transcode_plans_fit(S, h->plan)) return OJPHGPU_E_INVALID;
    *out = h.release();
    return OJPHGPU_OK;
  });
}
