// openjph_amd/csrc/dwt_region.h -- the launch of the region synthesis (kernels_dwt.hip, dwt_inverse_region_kernel) as the
// decoder objects call it: the grid is sized from the host copies of a batch's descriptors and regions.
#ifndef OJPH_DWT_REGION_H
#define OJPH_DWT_REGION_H

#include <cstdint>
#include "../../include/ojphgpu.h"

namespace ojphgpu {

// what sizes one launch: the largest region extent (row pairs per chunk, as pick_row_pairs / fit_rounds take it), the most
// strips and row pairs one descriptor's region spans
struct DwtRegionGrid { uint32_t max_w = 0, max_h = 0, strips = 0, pairs_y = 0; };
void dwt_region_grid_add(DwtRegionGrid& g, const ojphgpu_dwt_desc& d, const ojphgpu_dwt_region& r);
// n descriptors (nc = 3: triples of the colour planes); d_image == nullptr: a lower level into the arena; else the top level
// into the region frame in `container`-bit samples, converted with each descriptor's `reserved` format (bit depth | signed << 8)
int dwt_inverse_region_launch(void* stream, int reversible, const ojphgpu_dwt_desc* d_descs, const ojphgpu_dwt_region* d_regions,
                              uint32_t n, const DwtRegionGrid& g, void* d_base, void* d_image, int container, int nc);

}  // namespace ojphgpu
#endif
