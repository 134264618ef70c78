// tools/sanitize/rate_rounds_host.cpp -- the rounds of the byte-budget search (ojphgpu_rate_rounds_*, openjph_amd/csrc/ojph_rate.cpp)
// driven through the C ABI over a synthetic monotone size table, for a build under -fsanitize=address,undefined
// (tools/sanitize/run_rate_rounds.sh).  Host code only.  One frame: the rounds must ask what ojphgpu_rate_search_hint asks,
// then j* once more when the last trial was not j*; four frames with mixed outcomes: each ends as it does alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/ojphgpu.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x); exit(1); } } while (0)

static std::vector<int64_t> table(int64_t base, double growth)
{
  std::vector<int64_t> t(OJPHGPU_RATE_GRID);
  double s = (double)base;
  for (uint32_t j = 0; j < OJPHGPU_RATE_GRID; ++j) { t[j] = (int64_t)s; s = s * growth + 1.0; }
  return t;
}

struct Asked { const std::vector<int64_t>* tab; std::vector<uint32_t> idx; };
static int64_t size_fn(void* user, uint32_t j) { Asked* a = (Asked*)user; a->idx.push_back(j); return (*a->tab)[j]; }

struct Result { int code; ojphgpu_rate_info info; };

// F frames in rounds; asked[f]: the indices frame f measured at, in order
static std::vector<Result> rounds(const ojphgpu_plan* plan, const uint32_t* hist, const std::vector<uint64_t>& budgets,
                                  const std::vector<const std::vector<int64_t>*>& tabs, std::vector<std::vector<uint32_t>>& asked, uint32_t* count)
{
  const uint32_t F = (uint32_t)budgets.size();
  ojphgpu_rate_rounds* r = nullptr;
  CHECK(ojphgpu_rate_rounds_create(plan, hist, budgets.data(), F, -1, &r) == OJPHGPU_OK && r);
  std::vector<uint32_t> idx(F); std::vector<uint8_t> m(F); std::vector<int64_t> sizes(F);
  asked.assign(F, {});
  int code;
  while ((code = ojphgpu_rate_rounds_next(r, idx.data(), m.data())) == 1) {
    for (uint32_t f = 0; f < F; ++f) {
      CHECK(idx[f] < OJPHGPU_RATE_GRID);
      sizes[f] = m[f] ? (*tabs[f])[idx[f]] : INT64_MIN;
      if (m[f]) asked[f].push_back(idx[f]);
    }
    CHECK(ojphgpu_rate_rounds_feed(r, sizes.data()) == OJPHGPU_OK);
  }
  CHECK(code == OJPHGPU_OK);
  CHECK(ojphgpu_rate_rounds_next(r, idx.data(), m.data()) == OJPHGPU_E_INVALID);
  std::vector<Result> out(F);
  for (uint32_t f = 0; f < F; ++f) out[f].code = ojphgpu_rate_rounds_frame(r, f, &out[f].info);
  CHECK(ojphgpu_rate_rounds_count(r, count) == OJPHGPU_OK && *count <= 17);
  ojphgpu_rate_rounds_destroy(r);
  return out;
}

static Result alone(const ojphgpu_plan* plan, const uint32_t* hist, uint64_t budget, const std::vector<int64_t>& tab)
{
  Asked a{ &tab, {} };
  Result want;
  want.code = ojphgpu_rate_search_hint(plan, hist, budget, -1, size_fn, &a, &want.info);
  CHECK(want.code == OJPHGPU_OK || want.code == OJPHGPU_E_BUDGET);
  const bool recode = want.code == OJPHGPU_OK && a.idx.back() != want.info.grid_index;
  if (recode) { a.idx.push_back(want.info.grid_index); want.info.passes++; }
  std::vector<std::vector<uint32_t>> asked; uint32_t count = 0;
  const std::vector<Result> got = rounds(plan, hist, { budget }, { &tab }, asked, &count);
  CHECK(asked[0] == a.idx);
  CHECK(got[0].code == want.code && memcmp(&got[0].info, &want.info, sizeof(want.info)) == 0);
  CHECK(count == want.info.passes);
  return got[0];
}

int main()
{
  ojphgpu_params p; memset(&p, 0, sizeof(p));
  p.width = 200; p.height = 120; p.num_comps = 3; p.bit_depth = 10; p.num_decomps = 4; p.block_w = 64; p.block_h = 64;
  p.color_transform = 1; p.prog_order = 2; p.qstep = -1.0f;
  ojphgpu_plan* plan = nullptr;
  CHECK(ojphgpu_plan_create(&p, &plan) == OJPHGPU_OK && plan);
  uint64_t counts[8] = { 0 };
  CHECK(ojphgpu_plan_counts(plan, counts) == OJPHGPU_OK);
  const size_t hist_per = (size_t)counts[1] * OJPHGPU_STATS_BINS;
  const std::vector<int64_t> small = table(500, 1.03), large = table(3000, 1.025);
  const std::vector<uint64_t> budgets = { 20000, 100, 1ull << 40, 20000 };          // certified, nothing fits, everything fits, equal
  const std::vector<const std::vector<int64_t>*> tabs = { &small, &small, &small, &large };
  std::vector<uint32_t> hists(4 * hist_per, 0);
  for (size_t f = 0; f < 4; ++f)
    for (size_t b = 0; b < counts[1]; ++b)
      for (uint32_t k = 20; k < 60; ++k) hists[f * hist_per + b * OJPHGPU_STATS_BINS + k] = (uint32_t)(1000 / (1 + (k > 40 ? k - 40 : 40 - k)) + 7 * f);
  unsigned searches = 0, recodes = 0;
  for (const uint32_t* hist : { (const uint32_t*)hists.data(), (const uint32_t*)nullptr }) {
    std::vector<Result> each;
    for (size_t f = 0; f < 4; ++f) {
      each.push_back(alone(plan, hist ? hist + f * hist_per : nullptr, budgets[f], *tabs[f]));
      Asked a{ tabs[f], {} }; ojphgpu_rate_info plain;
      if (ojphgpu_rate_search_hint(plan, hist ? hist + f * hist_per : nullptr, budgets[f], -1, size_fn, &a, &plain) == OJPHGPU_OK)
        recodes += plain.passes != each.back().info.passes;
      ++searches;
    }
    for (uint64_t b = 600; b < 600000; b = b * 3 / 2) { alone(plan, hist, b, small); alone(plan, hist, b, large); searches += 2; }
    CHECK(each[0].code == OJPHGPU_OK && each[1].code == OJPHGPU_E_BUDGET && each[2].code == OJPHGPU_OK && each[2].info.grid_index == OJPHGPU_RATE_GRID - 1);
    std::vector<std::vector<uint32_t>> asked; uint32_t count = 0, most = 0;
    const std::vector<Result> got = rounds(plan, hist, budgets, tabs, asked, &count);
    for (size_t f = 0; f < 4; ++f) {
      CHECK(got[f].code == each[f].code && memcmp(&got[f].info, &each[f].info, sizeof(each[f].info)) == 0);
      CHECK(asked[f].size() == got[f].info.passes);
      most = got[f].info.passes > most ? got[f].info.passes : most;
    }
    CHECK(count >= most && count <= 17);
  }
  ojphgpu_plan_destroy(plan);
  printf("rate rounds: %u single searches (%u of the four mixed frames recoded j*), 2 searches of four frames, all as the callback search\n", searches, recodes);
  return 0;
}
