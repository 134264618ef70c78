// tests/facade/truncation_budget.cpp -- codestream::set_truncation_budget through the facade: argv = in.i32 w h num_comps
// bit_depth num_decomps colour_transform max_bytes out.j2c.  in.i32 holds the frame as int32 planes; it is coded reversibly
// under a cap of max_bytes bytes and written to out.j2c.  Prints "level <j> bytes <length> passes <n>".  Exit code 0 = coded
// and get_truncation_result agrees with the file; 3 = flush() reported that the cap cannot be met (and wrote nothing);
// 4 = write_headers refused the cap (argv[10] = "irreversible": the same frame asked for irreversibly); 1 = anything else.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>
#include "../../include/ojph_gpu_codestream.h"

int main(int argc, char** argv)
{
  if (argc < 10) { fprintf(stderr, "usage: %s in.i32 w h nc bit_depth num_decomps ct max_bytes out.j2c [irreversible]\n", argv[0]); return 2; }
  const unsigned w = (unsigned)atoi(argv[2]), h = (unsigned)atoi(argv[3]), nc = (unsigned)atoi(argv[4]), bd = (unsigned)atoi(argv[5]);
  const unsigned L = (unsigned)atoi(argv[6]);
  const bool ct = atoi(argv[7]) != 0, rev = !(argc > 10 && !strcmp(argv[10], "irreversible"));
  const size_t budget = (size_t)atoll(argv[8]);
  std::vector<int> img((size_t)w * h * nc);
  FILE* f = fopen(argv[1], "rb");
  if (!f || fread(img.data(), sizeof(int), img.size(), f) != img.size()) { fprintf(stderr, "FAILED: cannot read %s\n", argv[1]); return 1; }
  fclose(f);
  int stage = 0;
  try {
    ojph::codestream cs;
    ojph::param_siz siz = cs.access_siz();
    siz.set_image_extent(ojph::point(w, h));
    siz.set_num_components(nc);
    for (unsigned c = 0; c < nc; ++c) siz.set_component(c, ojph::point(1, 1), bd, false);
    siz.set_image_offset(ojph::point(0, 0));
    siz.set_tile_size(ojph::size(0, 0));
    siz.set_tile_offset(ojph::point(0, 0));
    ojph::param_cod cod = cs.access_cod();
    cod.set_num_decomposition(L);
    cod.set_block_dims(64, 64);
    cod.set_progression_order("RPCL");
    cod.set_reversible(rev);
    cod.set_color_transform(ct);
    if (!rev) cs.access_qcd().set_irrev_quant(0.01f);
    cs.set_planar(!ct);
    cs.set_truncation_budget(budget);
    ojph::j2c_outfile file;
    file.open(argv[9]);
    stage = 1;
    cs.write_headers(&file);
    stage = 2;
    ojph::ui32 next = 0;
    ojph::line_buf* line = cs.exchange(nullptr, next);
    std::vector<unsigned> row(nc, 0);
    while (line) {
      memcpy(line->i32, img.data() + ((size_t)next * h + row[next]) * w, w * sizeof(int));
      row[next]++;
      line = cs.exchange(line, next);
    }
    stage = 3;
    cs.flush();
    stage = 4;
    ojph::ui32 j = 0, passes = 0; ojph::ui64 bytes = 0;
    if (!cs.get_truncation_result(j, bytes, passes)) { fprintf(stderr, "FAILED: no result of the cap\n"); return 1; }
    cs.close();
    printf("level %u bytes %llu passes %u\n", j, (unsigned long long)bytes, passes);
    FILE* g = fopen(argv[9], "rb");
    if (!g) { fprintf(stderr, "FAILED: no output file\n"); return 1; }
    fseek(g, 0, SEEK_END);
    const long len = ftell(g);
    fclose(g);
    if ((ojph::ui64)len != bytes || (size_t)len > budget) { fprintf(stderr, "FAILED: %ld bytes in the file, %llu reported, budget %zu\n", len, (unsigned long long)bytes, budget); return 1; }
  } catch (const std::exception& e) {
    if (stage == 3) return 3;
    if (stage == 1) return 4;
    fprintf(stderr, "FAILED: %s\n", e.what());
    return 1;
  }
  return 0;
}
