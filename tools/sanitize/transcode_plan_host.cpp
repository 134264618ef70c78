// tools/sanitize/transcode_plan_host.cpp -- ojphgpu_plan_create_transcode (openjph_amd/csrc/ojph_transcode.cpp) under the host
// sanitizers: codestreams without a coded block are written from a few parameter sets, parsed, and the output plan is asked
// for with everything that may change and with a series of things that may not.  CPU only; see run_transcode_plan.sh.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ojphgpu.h"

static int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { ++failures; fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)

static ojphgpu_params base(uint32_t w, uint32_t h, uint32_t nc, bool rev, uint32_t tile)
{
  ojphgpu_params p; memset(&p, 0, sizeof(p));
  p.width = w; p.height = h; p.num_comps = nc; p.bit_depth = 10; p.reversible = rev ? 1 : 0; p.num_decomps = 4;
  p.block_w = p.block_h = 64; p.color_transform = nc >= 3; p.tile_w = p.tile_h = tile; p.prog_order = 2; p.qstep = rev ? -1.0f : 0.004f;
  return p;
}

static ojphgpu_plan* parsed_source(const ojphgpu_params& p)
{
  ojphgpu_plan* built = nullptr;
  if (ojphgpu_plan_create(&p, &built) != OJPHGPU_OK) return nullptr;
  uint64_t cnt[8];
  ojphgpu_plan_counts(built, cnt);
  std::vector<ojphgpu_coded_block> cb((size_t)cnt[2]);            // nothing coded: headers and empty packets
  memset(cb.data(), 0, cb.size() * sizeof(cb[0]));
  std::vector<uint8_t> out(1 << 20), data(16);
  size_t n = 0;
  ojphgpu_plan* src = nullptr;
  if (ojphgpu_t2_write(built, data.data(), cb.data(), out.data(), out.size(), &n) == OJPHGPU_OK)
    (void)ojphgpu_t2_parse(out.data(), n, 0, &src);
  ojphgpu_plan_destroy(built);
  return src;
}

static int ask(const ojphgpu_plan* src, const ojphgpu_params& p)
{
  ojphgpu_plan* out = nullptr;
  const int rc = ojphgpu_plan_create_transcode(src, &p, &out);
  EXPECT((rc == OJPHGPU_OK) == (out != nullptr));
  if (out) {
    uint64_t a[8], b[8];
    ojphgpu_plan_counts(src, a); ojphgpu_plan_counts(out, b);
    EXPECT(a[1] == b[1] && a[4] == b[4]);                         // the bands and the arena of the source
    ojphgpu_plan_destroy(out);
  }
  return rc;
}

int main()
{
  const ojphgpu_params sets[] = { base(312, 200, 3, false, 0), base(257, 301, 1, false, 0), base(384, 256, 3, false, 128),
                                  base(220, 180, 1, true, 0), base(384, 256, 3, true, 128) };
  for (const ojphgpu_params& made : sets) {
    ojphgpu_plan* src = parsed_source(made);
    EXPECT(src != nullptr);
    if (!src) continue;
    ojphgpu_params p;
    ojphgpu_plan_params(src, &p);
    const bool rev = p.reversible != 0;
    EXPECT(p.qstep == 0.0f);
    if (!rev) p.qstep = 0.004f;
    EXPECT(ask(src, p) == OJPHGPU_OK);
    for (uint32_t bw = 4; bw <= 1024; bw *= 2)
      for (uint32_t bh = 4; bh <= 1024; bh *= 2) {
        ojphgpu_params q = p; q.block_w = bw; q.block_h = bh;
        EXPECT(ask(src, q) == (bw * bh <= 4096 ? OJPHGPU_OK : OJPHGPU_E_INVALID));
      }
    for (uint32_t order = 0; order <= 5; ++order)
      for (uint32_t div = 0; div <= 3; ++div) {
        ojphgpu_params q = p; q.prog_order = order; q.reserved[1] = div; q.tlm = order & 1;
        q.precinct_w = 128; q.precinct_h = 64;
        EXPECT(ask(src, q) == (order <= 4 ? OJPHGPU_OK : OJPHGPU_E_INVALID));
      }
    { ojphgpu_params q = p; for (uint32_t i = 0; i <= q.num_decomps; ++i) q.precinct_exps[i] = (uint8_t)(0x55 + 0x11 * (i > 2)); EXPECT(ask(src, q) == OJPHGPU_OK); }
    { ojphgpu_params q = p; q.qstep = rev ? 0.01f : -1.0f; EXPECT(ask(src, q) == (rev ? OJPHGPU_E_INVALID : OJPHGPU_OK)); }
    // a byte of everything else flipped, one at a time: any other difference from the source is refused
    const size_t skip_lo = offsetof(ojphgpu_params, block_w), skip_hi = offsetof(ojphgpu_params, color_transform);
    for (size_t at = 0; at < sizeof(p); at += 3) {
      if ((at >= skip_lo && at < skip_hi) || (at >= offsetof(ojphgpu_params, prog_order) && at < offsetof(ojphgpu_params, reserved)) ||
          (at >= offsetof(ojphgpu_params, reserved) + 4 && at < offsetof(ojphgpu_params, reserved) + 8) ||
          (at >= offsetof(ojphgpu_params, precinct_exps) && at < offsetof(ojphgpu_params, image_x0))) continue;
      ojphgpu_params q = p;
      ((uint8_t*)&q)[at] ^= 0x01;
      EXPECT(ask(src, q) == OJPHGPU_E_INVALID);
    }
    EXPECT(ojphgpu_plan_create_transcode(nullptr, &p, nullptr) == OJPHGPU_E_INVALID);
    ojphgpu_plan* again = nullptr;
    EXPECT(ojphgpu_plan_restrict_resolution(src, 1, 1) == OJPHGPU_OK);
    EXPECT(ojphgpu_plan_create_transcode(src, &p, &again) == OJPHGPU_E_INVALID && again == nullptr);
    ojphgpu_plan_destroy(src);
  }
  printf("transcode_plan_host: %d failures\n", failures);
  return failures ? 1 : 0;
}
