// tests/facade/region_lines.cpp -- codestream::restrict_input_region through the facade: argv = file.j2c x0 y0 w h.  The
// file is decoded whole by one object and for the region by another (planar lines); param_siz::get_recon_width / _height of
// the second report the region's size on every component's grid, and its lines equal the crop of the first's.  With a 6th
// argument n the same with restrict_input_resolution(n, n) first.  Exit code 0 = all checks passed.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>
#include "../../include/ojph_gpu_codestream.h"

namespace {

struct Frame { std::vector<unsigned> w, h, x0, y0; std::vector<std::vector<int>> planes; };

Frame decode(const char* path, const unsigned* region, unsigned skip)
{
  ojph::codestream cs;
  ojph::j2c_infile file;
  file.open(path);
  cs.read_headers(&file);
  if (skip) cs.restrict_input_resolution(skip, skip);
  if (region) cs.restrict_input_region(region[0], region[1], region[2], region[3]);
  ojph::param_siz siz = cs.access_siz();
  Frame f;
  const unsigned nc = siz.get_num_components();
  for (unsigned c = 0; c < nc; ++c) {
    f.w.push_back(siz.get_recon_width(c)); f.h.push_back(siz.get_recon_height(c));
    const ojph::point d = siz.get_downsampling(c);
    const unsigned fx = d.x << skip, fy = d.y << skip;
    const unsigned ax = siz.get_image_offset().x + (region ? region[0] : 0), ay = siz.get_image_offset().y + (region ? region[1] : 0);
    f.x0.push_back((ax + fx - 1) / fx); f.y0.push_back((ay + fy - 1) / fy);
    f.planes.emplace_back((size_t)f.w[c] * f.h[c]);
  }
  cs.set_planar(true);
  cs.create();
  for (unsigned c = 0; c < nc; ++c)
    for (unsigned y = 0; y < f.h[c]; ++y) {
      ojph::ui32 comp = 0;
      ojph::line_buf* line = cs.pull(comp);
      if (!line || comp != c) throw std::runtime_error("line order");
      for (unsigned x = 0; x < f.w[c]; ++x) f.planes[c][(size_t)y * f.w[c] + x] = line->i32[x];
    }
  cs.close();
  return f;
}

}  // namespace

int main(int argc, char** argv)
{
  if (argc < 6) { fprintf(stderr, "usage: %s file.j2c x0 y0 w h [skip]\n", argv[0]); return 2; }
  const unsigned r[4] = { (unsigned)atoi(argv[2]), (unsigned)atoi(argv[3]), (unsigned)atoi(argv[4]), (unsigned)atoi(argv[5]) };
  const unsigned skip = argc > 6 ? (unsigned)atoi(argv[6]) : 0;
  int failures = 0;
  try {
    const Frame full = decode(argv[1], nullptr, skip), reg = decode(argv[1], r, skip);
    for (size_t c = 0; c < full.planes.size(); ++c) {
      // the region's place in the whole frame on the component's grid (the origins are ceil(A0 / f))
      const unsigned ox = reg.x0[c] - full.x0[c], oy = reg.y0[c] - full.y0[c];
      if (ox + reg.w[c] > full.w[c] || oy + reg.h[c] > full.h[c]) { ++failures; fprintf(stderr, "FAILED: region size of component %zu\n", c); continue; }
      for (unsigned y = 0; y < reg.h[c]; ++y)
        for (unsigned x = 0; x < reg.w[c]; ++x)
          if (reg.planes[c][(size_t)y * reg.w[c] + x] != full.planes[c][(size_t)(y + oy) * full.w[c] + x + ox]) {
            ++failures; fprintf(stderr, "FAILED: component %zu sample (%u, %u)\n", c, x, y); y = reg.h[c]; break;
          }
    }
    if (reg.w.empty() || reg.w[0] == 0) { ++failures; fprintf(stderr, "FAILED: empty region frame\n"); }
  } catch (const std::exception& e) { fprintf(stderr, "FAILED: %s\n", e.what()); return 1; }
  return failures ? 1 : 0;
}
