// openjph_amd/apps/ojph_compress.cpp -- command-line encoder on the GPU path, option-compatible
// with the reference's ojph_compress for the options the GPU path implements
// (src/apps/ojph_compress/ojph_compress.cpp:361-1226; defaults :495-510: irreversible, RPCL,
// 5 decompositions, 64x64 blocks; PPM input switches the colour transform on, :754-757; .yuv /
// .raw input needs -dims -num_comps -bit_depth [-signed] and is planar without colour transform,
// :997-1021).  Prints "Elapsed time = ..." like the reference (:1220-1222).
#include <algorithm>
#include <chrono>
#include <cmath>
#include "ojph_app_common.h"
#include "../../include/ojph_gpu_codestream.h"

static void usage() {
  printf("ojph_compress (GPU path) -i in.{pgm,ppm,yuv,raw} -o out.j2c [-reversible true|false] [-qstep f | -qfactor 1..100 | -max_bytes n | -min_psnr dB [-cap_bytes n] | -truncate_to n]\n"
         "  [-num_decomps n] [-block_size {w,h}] [-precincts {w,h}] [-prog_order LRCP|RLCP|RPCL|PCRL|CPRL]\n"
         "  [-colour_trans true|false] [-tile_size {w,h}] [-tlm_marker true|false] [-device n | -devices n,n,...]\n"
         "  [-image_offset {x,y}] [-tile_offset {x,y}] [-tileparts R|C|RC] [-profile IMF|BROADCAST] [-com \"text\"]\n"
         "  raw input: -dims {w,h} -num_comps n -bit_depth b [-signed true|false] [-downsamp {x,y},{x,y},...]\n");
}

int main(int argc, char** argv) {
  Args a(argc, argv);
  const char* in = a.get("-i"); const char* out = a.get("-o");
  if (!in || !out) { usage(); return -1; }
  try {
    Image img;
    std::vector<unsigned> dsx, dsy;                  // -downsamp {x,y} per component; the last pair repeats (ojph_compress.cpp:1003-1016)
    const std::string ins(in);
    const bool pnm = ends_with(ins, ".pgm") || ends_with(ins, ".ppm");
    if (pnm) read_pnm(in, img);
    else if (ends_with(ins, ".yuv") || ends_with(ins, ".raw")) {
      auto dims = Args::numbers(a.get("-dims"));
      if (dims.size() != 2 || !a.get("-num_comps") || !a.get("-bit_depth"))
        throw std::runtime_error("raw input needs -dims {w,h} -num_comps n -bit_depth b");
      img.width = (unsigned)dims[0]; img.height = (unsigned)dims[1];
      img.num_comps = (unsigned)atoi(a.get("-num_comps"));
      auto bdl = Args::numbers(a.get("-bit_depth"));           // one value, or one per component (the last repeats)
      img.bit_depth = (unsigned)bdl[0];
      auto sg = Args::bools(a.get("-signed")); img.is_signed = !sg.empty() && sg[0];
      for (unsigned c = 0; c < img.num_comps; ++c) {
        img.depth.push_back((unsigned)bdl[std::min<size_t>(c, bdl.size() - 1)]);
        img.sgn.push_back(sg.empty() ? false : (bool)sg[std::min<size_t>(c, sg.size() - 1)]);
      }
      auto ds = Args::numbers(a.get("-downsamp"));
      if (ds.size() % 2) throw std::runtime_error("-downsamp takes {x,y} pairs");
      for (unsigned c = 0; c < img.num_comps && !ds.empty(); ++c) {
        const size_t k = std::min<size_t>(c, ds.size() / 2 - 1);
        if (ds[2 * k] < 1 || ds[2 * k + 1] < 1 || ds[2 * k] > 255 || ds[2 * k + 1] > 255) throw std::runtime_error("-downsamp factors must be 1..255");
        dsx.push_back((unsigned)ds[2 * k]); dsy.push_back((unsigned)ds[2 * k + 1]);
      }
      img.layout(dsx, dsy);
      read_raw(in, img);
    } else throw std::runtime_error("unknown input file extension (pgm, ppm, yuv, raw)");

    const auto t0 = std::chrono::steady_clock::now();
    ojph::codestream cs;
    if (a.get("-device")) cs.set_device(atoi(a.get("-device")));
    if (a.get("-devices")) {                        // a tiled frame over several GPUs (contiguous runs of tiles)
      std::vector<int> devs;
      for (long v : Args::numbers(a.get("-devices"))) devs.push_back((int)v);
      if (!devs.empty()) cs.set_devices(devs.data(), (ojph::ui32)devs.size());
    }
    ojph::param_siz siz = cs.access_siz();
    auto io = Args::numbers(a.get("-image_offset")), to = Args::numbers(a.get("-tile_offset"));
    const ojph::point image_offset(io.size() == 2 ? (unsigned)io[0] : 0, io.size() == 2 ? (unsigned)io[1] : 0);
    if ((image_offset.x || image_offset.y) && !dsx.empty())
      for (unsigned c = 0; c < img.num_comps; ++c)
        if (dsx[c] != 1 || dsy[c] != 1) throw std::runtime_error("-image_offset together with -downsamp: the planes of the input file would not match the reference grid");
    siz.set_image_extent(ojph::point(image_offset.x + img.width, image_offset.y + img.height));       // ojph_compress.cpp:681-683
    siz.set_num_components(img.num_comps);
    for (unsigned c = 0; c < img.num_comps; ++c)
      siz.set_component(c, ojph::point(c < dsx.size() ? dsx[c] : 1, c < dsy.size() ? dsy[c] : 1), img.bd(c), img.sg(c));
    siz.set_image_offset(image_offset);
    auto ts = Args::numbers(a.get("-tile_size"));
    siz.set_tile_size(ts.size() == 2 ? ojph::size((unsigned)ts[0], (unsigned)ts[1]) : ojph::size(0, 0));
    siz.set_tile_offset(ojph::point(to.size() == 2 ? (unsigned)to[0] : 0, to.size() == 2 ? (unsigned)to[1] : 0));

    ojph::param_cod cod = cs.access_cod();
    cod.set_num_decomposition(a.get("-num_decomps") ? (unsigned)atoi(a.get("-num_decomps")) : 5);
    auto bs = Args::numbers(a.get("-block_size"));
    cod.set_block_dims(bs.size() == 2 ? (unsigned)bs[0] : 64, bs.size() == 2 ? (unsigned)bs[1] : 64);
    auto pr = Args::numbers(a.get("-precincts"));
    if (pr.size() >= 2) {
      std::vector<ojph::size> ps;
      for (size_t i = 0; i + 1 < pr.size(); i += 2) ps.push_back(ojph::size((unsigned)pr[i], (unsigned)pr[i + 1]));
      cod.set_precinct_size((int)ps.size(), ps.data());
    }
    cod.set_progression_order(a.get("-prog_order") ? a.get("-prog_order") : "RPCL");
    const bool reversible = Args::to_bool(a.get("-reversible"));
    cod.set_reversible(reversible);
    bool ct = pnm && img.num_comps == 3;                       // PPM turns the colour transform on by default
    if (a.get("-colour_trans")) ct = Args::to_bool(a.get("-colour_trans"));
    cod.set_color_transform(ct);
    if (a.get("-qfactor") && a.get("-qstep")) throw std::runtime_error("-qfactor and -qstep cannot be used together");   // ojph_compress.cpp:644-649
    if (a.get("-qfactor") && (atoi(a.get("-qfactor")) < 1 || atoi(a.get("-qfactor")) > 100)) throw std::runtime_error("-qfactor must be between 1 and 100");
    if (!reversible && a.get("-qstep")) cs.access_qcd().set_irrev_quant((float)atof(a.get("-qstep")));
    if (!reversible && a.get("-qfactor")) {
      if (img.num_comps != 1 && img.num_comps != 3) throw std::runtime_error("-qfactor is only supported for images with 1 or 3 components");   // :921-926
      cs.access_qcd().set_qfactor((ojph::ui8)atoi(a.get("-qfactor")));
    }
    if (a.get("-max_bytes")) {                                  // GPU path only: the finest step of the rate grid that fits
      if (reversible) throw std::runtime_error("-max_bytes needs irreversible coding (-reversible false)");
      if (a.get("-qfactor") || a.get("-qstep")) throw std::runtime_error("-max_bytes chooses the quantisation step itself: it cannot be used together with -qstep or -qfactor");
      if (a.get("-devices")) throw std::runtime_error("-max_bytes codes on one device: it cannot be used together with -devices");
      const long long mb = atoll(a.get("-max_bytes"));
      if (mb <= 0) throw std::runtime_error("-max_bytes must be a positive number of bytes");
      cs.set_byte_budget((size_t)mb);
    }
    if (a.get("-truncate_to")) {                                // GPU path only: lossless where it fits, else the first truncation level that does
      if (!reversible) throw std::runtime_error("-truncate_to needs reversible coding (-reversible true); an irreversible byte budget is -max_bytes");
      if (a.get("-devices")) throw std::runtime_error("-truncate_to codes on one device: it cannot be used together with -devices");
      const long long tb = atoll(a.get("-truncate_to"));
      if (tb <= 0) throw std::runtime_error("-truncate_to must be a positive number of bytes");
      cs.set_truncation_budget((size_t)tb);
    }
    unsigned long long max_sse = 0;
    if (a.get("-cap_bytes") && !a.get("-min_psnr")) throw std::runtime_error("-cap_bytes caps a quality target: it needs -min_psnr (a byte budget alone is -max_bytes)");
    if (a.get("-min_psnr")) {                                   // GPU path only: the coarsest step of the rate grid found to reach the PSNR
      if (reversible) throw std::runtime_error("-min_psnr needs irreversible coding (-reversible false)");
      if (a.get("-qfactor") || a.get("-qstep")) throw std::runtime_error("-min_psnr chooses the quantisation step itself: it cannot be used together with -qstep or -qfactor");
      if (a.get("-max_bytes")) throw std::runtime_error("-min_psnr and -max_bytes cannot be used together: a quality target under a byte cap is -min_psnr with -cap_bytes");
      if (a.get("-devices")) throw std::runtime_error("-min_psnr codes on one device: it cannot be used together with -devices");
      unsigned long long n = 0;
      for (unsigned c = 0; c < img.num_comps; ++c) {
        if (img.bd(c) != img.bd(0)) throw std::runtime_error("-min_psnr needs components of one bit depth");
        n += (unsigned long long)img.cw[c] * img.ch[c];
      }
      if (img.bd(0) > 16) throw std::runtime_error("-min_psnr needs components of at most 16 bits");
      const unsigned long long peak = (1ull << img.bd(0)) - 1;
      max_sse = (unsigned long long)((double)(n * peak * peak) / pow(10.0, atof(a.get("-min_psnr")) / 10.0));   // (plan.psnr_to_sse)
      if (a.get("-cap_bytes")) {                                // ... but never above this many bytes: the cap wins
        const long long cb = atoll(a.get("-cap_bytes"));
        if (cb <= 0) throw std::runtime_error("-cap_bytes must be a positive number of bytes");
        cs.set_max_sse(max_sse, (unsigned long long)cb);
      } else
        cs.set_max_sse(max_sse);
    }
    if (a.get("-tlm_marker")) cs.request_tlm_marker(Args::to_bool(a.get("-tlm_marker")));
    if (a.get("-profile")) cs.set_profile(a.get("-profile"));
    if (a.get("-tileparts")) {                                  // ojph_compress.cpp:324-356: letters R and / or C
      const std::string tp(a.get("-tileparts"));
      for (char ch : tp) if (ch != 'R' && ch != 'C') throw std::runtime_error("could not interpret -tileparts fields; allowed values are \"R\" \"C\" and \"RC\"");
      cs.set_tilepart_divisions(tp.find('R') != std::string::npos, tp.find('C') != std::string::npos);
    }
    cs.set_planar(!ct);

    ojph::j2c_outfile file;
    file.open(out);
    ojph::comment_exchange com;
    if (a.get("-com")) com.set_string(a.get("-com"));
    cs.write_headers(&file, a.get("-com") ? &com : nullptr, a.get("-com") ? 1 : 0);
    ojph::ui32 next = 0;
    ojph::line_buf* line = cs.exchange(nullptr, next);
    std::vector<unsigned> row(img.num_comps, 0);
    while (line) {                                   // the codestream says which component it wants next
      if (row[next] < img.ch[next])
        memcpy(line->i32, img.plane(next) + (size_t)row[next] * img.cw[next], img.cw[next] * sizeof(int));
      row[next]++;
      line = cs.exchange(line, next);
    }
    cs.flush();
    {
      ojph::ui32 gi = 0, passes = 0; float q = 0; ojph::ui64 nbytes = 0;
      if (a.get("-max_bytes") && cs.get_byte_budget_result(gi, q, nbytes, passes))
        printf("Byte budget %s: qstep = %.9g (grid index %u), %llu bytes, %u passes\n", a.get("-max_bytes"), (double)q, gi, (unsigned long long)nbytes, passes);
    }
    {
      ojph::ui32 level = 0, passes = 0; ojph::ui64 nbytes = 0;
      if (a.get("-truncate_to") && cs.get_truncation_result(level, nbytes, passes))
        printf("Truncation budget %s: level %u%s, %llu bytes, %u passes\n", a.get("-truncate_to"), level, level ? "" : " (lossless)", (unsigned long long)nbytes, passes);
    }
    {
      ojph::ui32 gi = 0, passes = 0, pae = 0; float q = 0; ojph::ui64 nbytes = 0, sse = 0, coarser = 0;
      if (a.get("-min_psnr") && cs.get_quality_info(gi, q, sse, coarser, pae, nbytes, passes))
        printf("Quality target %s dB: max_sse %llu, qstep = %.9g (grid index %u), sse %llu, one step coarser %llu, largest difference %u, %llu bytes, %u trials\n",
               a.get("-min_psnr"), max_sse, (double)q, gi, (unsigned long long)sse, (unsigned long long)coarser, pae, (unsigned long long)nbytes, passes);
      bool met = false; ojph::ui32 qi = 0, qpasses = 0, rpasses = 0;
      if (a.get("-cap_bytes") && cs.get_capped_info(gi, q, met, qi, sse, pae, nbytes, qpasses, rpasses))
        printf("Quality target %s dB under %s bytes: max_sse %llu, outcome %s, qstep = %.9g (grid index %u, the target's %u), sse %llu, largest difference %u, %llu bytes, %u quality trials, %u codings\n",
               a.get("-min_psnr"), a.get("-cap_bytes"), max_sse, met ? "MET" : "BY_BUDGET", (double)q, gi, qi, (unsigned long long)sse, pae,
               (unsigned long long)nbytes, qpasses, rpasses);
    }
    cs.close();
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    printf("Elapsed time = %f\n", dt);
  } catch (const std::exception& e) {
    const char* w = e.what();
    if (w && strncmp(w, "ojph error", 10) != 0) printf("%s\n", w);
    return -1;
  }
  return 0;
}
