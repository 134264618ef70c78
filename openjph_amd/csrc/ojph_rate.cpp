// openjph_amd/csrc/ojph_rate.cpp -- encoding to a byte budget, host side (include/ojphgpu.h section 5b): the grid of base
// steps, the quantisation of every band at every step of it, the model that turns the band statistics into predicted bytes
// and the search that finds the finest step whose codestream fits.  Needs no GPU: the size of a trial comes from a callback.
//
// The reference side of it is param_qcd::set_irrev_quant (ojph_params.cpp:1542-1599), which scales the base step per
// sub-band, and encode_SPqcd (:1602-1613), which rounds it to 5 + 11 bits; derive_quant (ojph_plan.cpp) restates both, and
// the table below is nothing but derive_quant at the 241 steps.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <vector>

#include "ojph_plan.h"

namespace ojphgpu {

float rate_grid_qstep(uint32_t j) { return (float)std::exp2(-1.0 - (double)j / 16.0); }

bool rate_plan_ok(const Plan& P)
{
  if (P.parsed || P.p.reserved[2] != 0 || !P.atks.empty() || !P.dfss.empty() || P.p.wavelet != 0) return false;
  for (uint32_t c = 0; c < P.p.num_comps; ++c) {
    const CodStyle& st = P.style(c);
    if (st.rev || st.wavelet >= 2 || st.dfs >= 0) return false;
    if (c < OJPHGPU_MAX_COC_COMPS && P.p.qcc_qfactor[c] != 0) return false;
  }
  return !P.cod.rev;
}

bool rate_apply_step(Plan& Q, float qstep)
{
  Q.p.qstep = qstep;
  if (!derive_quant(Q)) return false;
  for (Band& B : Q.bands) {                                  // as build_plan fills them (ojph_subband.cpp:156-164)
    B.K_max = band_Kmax(Q, B.comp, B.res, B.band);
    if (B.K_max == 0 || B.K_max > 31) return false;
    float d = band_delta(Q, B.comp, B.res, B.band);
    d /= (float)(1u << ((31u - B.K_max) & 31u));
    B.delta = d; B.delta_inv = 1.0f / d;
  }
  return true;
}

int rate_table_build(const Plan& P, RateTable& T)
{
  if (!rate_plan_ok(P)) return OJPHGPU_E_INVALID;
  std::map<uint64_t, uint32_t> ids;
  std::vector<Band> reps;                                    // one band per class
  T.band_class.resize(P.bands.size());
  for (size_t i = 0; i < P.bands.size(); ++i) {
    const Band& B = P.bands[i];
    const uint64_t key = ((uint64_t)B.comp << 16) | ((uint64_t)B.res << 8) | B.band;
    auto it = ids.find(key);
    if (it == ids.end()) { it = ids.emplace(key, (uint32_t)reps.size()).first; reps.push_back(B); }
    T.band_class[i] = it->second;
  }
  T.nclasses = (uint32_t)reps.size();
  T.num_blocks = P.blocks.size();
  // what derive_quant and band_Kmax / band_delta read of a plan, and nothing of its tables
  Plan L;
  L.p = P.p; L.comps = P.comps; L.cod = P.cod; L.coc = P.coc; L.frame_elems = P.frame_elems;
  L.bands = reps;
  T.quant.assign((size_t)OJPHGPU_RATE_GRID * T.nclasses, BandQuant{ 0.0f, 0 });
  T.log2_step.assign(T.quant.size(), 0.0);
  for (uint32_t j = 0; j < OJPHGPU_RATE_GRID; ++j) {
    if (!rate_apply_step(L, rate_grid_qstep(j))) return OJPHGPU_E_INVALID;
    for (uint32_t c = 0; c < T.nclasses; ++c) {
      const Band& B = L.bands[c];
      T.quant[(size_t)j * T.nclasses + c] = BandQuant{ B.delta, B.K_max };
      T.log2_step[(size_t)j * T.nclasses + c] = std::log2((double)B.delta) + (double)(31u - B.K_max);
    }
  }
  return OJPHGPU_OK;
}

// The model.  A coefficient whose half octave lies below its band's step costs nothing; one at t = log2(|c| / step) > 0
// costs t magnitude bits plus about three for its sign and its share of the VLC and MEL strings; the half octave around
// the step is significant for part of its members.  Per block a few bytes of packet header, per codestream its markers.
// Its absolute level is off by 10 % at the usual rates and by far more near the knee, where most coefficients are
// within a factor of two of the step -- the search rescales it by what a trial measures.
struct RateModel {
  const RateTable& T;
  std::vector<double> h;                                     // [nclasses][BINS]: the bands' histograms summed per class
  std::vector<uint8_t> used;                                 // per class: the bins that hold anything, as a list
  std::vector<uint32_t> used_first;
  double memo[OJPHGPU_RATE_GRID];
  RateModel(const RateTable& t, const uint32_t* hist) : T(t), h((size_t)t.nclasses * OJPHGPU_STATS_BINS, 0.0)
  {
    for (size_t b = 0; b < T.band_class.size(); ++b)
      for (uint32_t k = 0; k < OJPHGPU_STATS_BINS; ++k) h[(size_t)T.band_class[b] * OJPHGPU_STATS_BINS + k] += hist[b * OJPHGPU_STATS_BINS + k];
    used_first.assign(T.nclasses + 1, 0);
    for (uint32_t c = 0; c < T.nclasses; ++c) {
      for (uint32_t k = 1; k < OJPHGPU_STATS_BINS; ++k) if (h[(size_t)c * OJPHGPU_STATS_BINS + k] > 0) used.push_back((uint8_t)k);
      used_first[c + 1] = (uint32_t)used.size();
    }
    for (double& m : memo) m = -1.0;
  }
  double bytes(uint32_t j)
  {
    if (memo[j] >= 0) return memo[j];
    double bits = 0;
    for (uint32_t c = 0; c < T.nclasses; ++c) {
      const double ld = T.log2_step[(size_t)j * T.nclasses + c];
      for (uint32_t i = used_first[c]; i < used_first[c + 1]; ++i) {
        const uint32_t k = used[i];
        // bin k holds 2^e (1 + m / 2) .. with e = (k + 1) / 2 - 32, m = the top mantissa bit: log2 of its middle
        const double mid = (double)((int)((k + 1) / 2) - 32) + (((k + 1) & 1u) == 0 ? 0.29 : 0.79);
        const double t = mid - ld;
        if (t > -0.5) bits += h[(size_t)c * OJPHGPU_STATS_BINS + k] * (std::max(t, 0.0) + 3.0) * (t > 0.5 ? 1.0 : 0.6);
      }
    }
    return memo[j] = bits / 8.0 + 300.0 + 6.0 * (double)T.num_blocks;
  }
};

}  // namespace ojphgpu

// The search as a state machine, so that several of them can advance together over shared measurements (the rounds below):
// _next hands out the index to measure, _feed takes its size.  hint: a grid index to try first (the previous frame's answer),
// then its neighbour on the side the result points to and, if that points the same way, the index beyond it, before the
// model proposes anything; -1 = none.  The hinted trials shrink the interval like any other and count among the six
// model-led ones, so the guarantees of the plain search hold.
struct ojphgpu_rate_stepper {
  enum Phase { HINT, HINT_FED, NEIGHBOUR, MAIN, ENDED };
  static constexpr int N = OJPHGPU_RATE_GRID;
  ojphgpu::RateTable own;                                    // of a stepper made from a plan: what its model reads
  std::unique_ptr<ojphgpu::RateModel> model;
  uint64_t max_bytes = 0;
  int hint = -1;
  std::vector<int64_t> size = std::vector<int64_t>((size_t)N, -1);
  // every index <= lo that was tried fits, every index >= hi that was tried does not; lo and hi themselves were tried (or are
  // the ends -1 / N).  hi - lo == 1 is the certificate: size(lo) <= B < size(lo + 1), both measured.
  int lo = -1, hi = N;
  double scale = 1.0;
  Phase phase = MAIN;
  int dir = 0, k = 0;                                        // of the hinted trials: the side they walk to, how far
  int pending = -1;                                          // the index handed out and not fed yet
  ojphgpu_rate_info info;
  // c < N: size(c) = cs > budget was measured by the caller -- the search runs below c, and cs is the model's first scale
  void start(const ojphgpu::RateTable& t, const uint32_t* hist, uint64_t budget, int h, int c = N, uint64_t cs = 0)
  {
    max_bytes = budget; hint = h;
    if (hist) model.reset(new ojphgpu::RateModel(t, hist));
    if (c < N) {
      hi = c; size[(size_t)c] = (int64_t)cs;                  // (a ceiling is nothing but the first hi, measured by the caller)
      if (hint >= c) hint = c - 1;
      if (model) { const double p = model->bytes((uint32_t)c); if (p > 0) scale = (double)cs / p; }
    }
    phase = hint >= 0 ? HINT : MAIN;
    memset(&info, 0, sizeof(info));
  }
  int hand(int j, uint32_t* out)
  {
    if (info.passes == 0) info.first_guess = (uint32_t)j;
    pending = j; *out = (uint32_t)j;
    return 1;
  }
  int next(uint32_t* out)
  {
    if (phase == ENDED || pending >= 0) return OJPHGPU_E_INVALID;
    if (phase == HINT) { phase = HINT_FED; return hand(hint, out); }
    if (phase == NEIGHBOUR) {
      // the neighbour the result points to and, when that one points the same way, the next index on: an answer one step
      // from the hint is certified by three trials whatever the model makes of the frame.  Each only where the index
      // exists and the certificate is still open.
      const int nb = hint + k * dir;
      if (k <= 2 && hi - lo > 1 && nb > lo && nb < hi) return hand(nb, out);
      phase = MAIN;
    }
    if (hi - lo > 1) {
      int j = (lo + hi) / 2;
      if (model && info.passes < 6) {
        // the finest candidate the rescaled model lets fit (its prediction grows with j: bisection over the candidates)
        int a = lo, b = hi;                                  // a fits (or is the end), b does not
        while (b - a > 1) { const int m = (a + b) / 2; if (scale * model->bytes((uint32_t)m) <= (double)max_bytes) a = m; else b = m; }
        j = std::min(std::max(a, lo + 1), hi - 1);
      }
      return hand(j, out);
    }
    phase = ENDED;
    if (lo < 0) return OJPHGPU_E_BUDGET;
    info.grid_index = (uint32_t)lo; info.qstep = ojphgpu::rate_grid_qstep((uint32_t)lo);
    info.bytes = (uint64_t)size[(size_t)lo];
    info.bytes_finer = hi < N ? (uint64_t)size[(size_t)hi] : 0;
    return OJPHGPU_OK;
  }
  int feed(int64_t s)
  {
    if (phase == ENDED || pending < 0) return OJPHGPU_E_INVALID;
    const int j = pending;
    pending = -1;
    info.passes++;
    if (s < 0) { phase = ENDED; return s < INT32_MIN ? OJPHGPU_E_INVALID : (int)s; }
    size[(size_t)j] = s;
    if (model) { const double p = model->bytes((uint32_t)j); scale = p > 0 ? (double)s / p : 1.0; }
    if ((uint64_t)s <= max_bytes) lo = j; else hi = j;
    if (phase == HINT_FED) { dir = lo == hint ? 1 : -1; k = 1; phase = NEIGHBOUR; }
    else if (phase == NEIGHBOUR) {
      if ((dir > 0) != (lo == j)) phase = MAIN;              // it turned round: the certificate, or a table that is not monotone
      else ++k;
    }
    return OJPHGPU_OK;
  }
};

// The searches of the F frames of one encoder run, advanced together in ROUNDS: one stepper per frame over shared
// measurements.  A round codes every frame -- an open one at the index its stepper hands out, a certified one at its j*, one
// nothing fits at index 0 -- and the sizes of the frames that measure come back together.  Closed frames are coded again
// in every later round: device time, accepted for that.  Host only: whoever drives it does the coding (the encoder), or
// reads the sizes from a table (the tests).  One frame is the single encoder's search: the indices of rate_search, then j*
// once more when the last trial was not j*, and rounds == passes.
struct ojphgpu_rate_rounds {
  enum Measure { IDLE = 0, TRIAL = 1, VERIFY = 2 };          // what a frame's size of this round is for
  ojphgpu::RateTable own;                                    // of an object made from a plan; the steppers point at it
  std::vector<ojphgpu_rate_stepper> st;
  std::vector<int> at, measure, rc;                          // the index a frame was coded at in the last round (-1: none); its verdict
  std::vector<uint32_t> idx;                                 // the index a frame is coded at in this round
  std::vector<char> open;
  std::vector<ojphgpu_rate_info> info;
  uint32_t rounds = 0;
  bool out = false, ended = false; int failed = 0;           // a round is handed out and not fed; no round follows; what ended the search early
  void start(const ojphgpu::RateTable& T, const uint32_t* hist, size_t hist_per, const uint64_t* budgets, uint32_t F, int hint)
  {
    st = std::vector<ojphgpu_rate_stepper>(F);
    for (uint32_t f = 0; f < F; ++f) st[f].start(T, hist ? hist + f * hist_per : nullptr, budgets[f], hint);
    at.assign(F, -1); measure.assign(F, IDLE); rc.assign(F, OJPHGPU_E_INVALID); idx.assign(F, 0); open.assign(F, 1);
    ojphgpu_rate_info none; memset(&none, 0, sizeof(none));
    info.assign(F, none);
  }
  int fail(int code) { ended = true; failed = code; return code; }
  int next(uint32_t* idx_out, uint8_t* measures)
  {
    if (ended || out) return OJPHGPU_E_INVALID;
    bool work = false;
    for (size_t f = 0; f < st.size(); ++f) {
      measure[f] = IDLE;
      if (open[f]) {
        uint32_t j = 0;
        const int r = st[f].next(&j);
        if (r == 1) { idx[f] = j; measure[f] = TRIAL; }
        else if (r == OJPHGPU_OK || r == OJPHGPU_E_BUDGET) {
          // A frame nothing fits stands at index 0 already: with lo == -1 the search can only end on the feed that set
          // hi = 0, so its last trial was index 0 and it never causes a round of its own -- a single encoder's
          // OJPHGPU_E_BUDGET costs the passes of its search and no more.
          open[f] = 0; rc[f] = r; info[f] = st[f].info;
          idx[f] = r == OJPHGPU_OK ? info[f].grid_index : 0;
          // the last trial was j* + 1: j* is coded once more, counted and checked
          if (r == OJPHGPU_OK && at[f] != (int)idx[f]) { info[f].passes++; measure[f] = VERIFY; }
        } else return fail(r);
      }
      if (measure[f] != IDLE || at[f] != (int)idx[f]) work = true;
    }
    if (!work) { ended = true; return OJPHGPU_OK; }          // nobody measures and every frame stands at its index
    ++rounds; out = true;
    for (size_t f = 0; f < st.size(); ++f) { idx_out[f] = idx[f]; measures[f] = (uint8_t)measure[f]; }
    return 1;
  }
  int feed(const int64_t* sizes)
  {
    if (ended || !out) return OJPHGPU_E_INVALID;
    out = false;
    for (size_t f = 0; f < st.size(); ++f) {
      const int64_t s = sizes[f];
      at[f] = (int)idx[f];
      if (measure[f] == TRIAL) { const int r = st[f].feed(s); if (r) return fail(r); }
      else if (measure[f] == VERIFY) {
        if (s < 0) return fail(s < INT32_MIN ? OJPHGPU_E_INVALID : (int)s);
        if ((uint64_t)s != info[f].bytes) return fail(OJPHGPU_E_HIP);   // the same blocks at the same step: anything else is a fault
      }
    }
    return OJPHGPU_OK;
  }
};

namespace ojphgpu {

int rate_rounds_create(const RateTable& T, const uint32_t* hist, size_t hist_per, const uint64_t* max_bytes, uint32_t frames, int hint,
                       ojphgpu_rate_rounds** out)
{
  if (!out || !max_bytes || frames == 0 || hint < -1 || hint >= (int)OJPHGPU_RATE_GRID) return OJPHGPU_E_INVALID;
  std::unique_ptr<ojphgpu_rate_rounds> r(new ojphgpu_rate_rounds());
  r->start(T, hist, hist_per, max_bytes, frames, hint);
  *out = r.release();
  return OJPHGPU_OK;
}

// the one search there is: a loop over the stepper
int rate_search(const RateTable& T, const uint32_t* hist, uint64_t max_bytes, int hint, ojphgpu_size_fn fn, void* user, ojphgpu_rate_info* out)
{
  if (!fn || !out || hint < -1 || hint >= (int)OJPHGPU_RATE_GRID) return OJPHGPU_E_INVALID;
  memset(out, 0, sizeof(*out));
  ojphgpu_rate_stepper st;
  st.start(T, hist, max_bytes, hint);
  for (;;) {
    uint32_t j = 0;
    int rc = st.next(&j);
    if (rc == 1) rc = st.feed(fn(user, j)); else { *out = st.info; return rc; }
    if (rc) { *out = st.info; return rc; }
  }
}

}  // namespace ojphgpu

using namespace ojphgpu;

extern "C" int ojphgpu_rate_grid_qstep(uint32_t j, float* qstep)
{
  if (j >= OJPHGPU_RATE_GRID || !qstep) return OJPHGPU_E_INVALID;
  *qstep = rate_grid_qstep(j);
  return OJPHGPU_OK;
}

extern "C" int ojphgpu_rate_search_hint(const ojphgpu_plan* plan, const uint32_t* hist, uint64_t max_bytes, int32_t hint, ojphgpu_size_fn fn,
                                        void* user, ojphgpu_rate_info* out)
{
  if (!plan || !fn || !out) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    RateTable T;
    const int rc = rate_table_build(plan->plan, T);
    if (rc) return rc;
    return rate_search(T, hist, max_bytes, hint, fn, user, out);
  });
}

extern "C" int ojphgpu_rate_stepper_create(const ojphgpu_plan* plan, const uint32_t* hist, uint64_t max_bytes, int32_t hint,
                                           ojphgpu_rate_stepper** out)
{
  return ojphgpu_rate_stepper_create_under(plan, hist, max_bytes, hint, OJPHGPU_RATE_GRID, 0, out);
}

extern "C" int ojphgpu_rate_stepper_create_under(const ojphgpu_plan* plan, const uint32_t* hist, uint64_t max_bytes, int32_t hint,
                                                 uint32_t ceil_index, uint64_t ceil_size, ojphgpu_rate_stepper** out)
{
  if (!plan || !out || hint < -1 || hint >= (int32_t)OJPHGPU_RATE_GRID) return OJPHGPU_E_INVALID;
  if (ceil_index == 0 || ceil_index > OJPHGPU_RATE_GRID) return OJPHGPU_E_INVALID;
  if (ceil_index < OJPHGPU_RATE_GRID && (ceil_size <= max_bytes || ceil_size > (uint64_t)INT64_MAX)) return OJPHGPU_E_INVALID;   // (no ceiling: not read)
  *out = nullptr;
  return no_throw([&]() -> int {
    std::unique_ptr<ojphgpu_rate_stepper> st(new ojphgpu_rate_stepper());
    const int rc = rate_table_build(plan->plan, st->own);
    if (rc) return rc;
    st->start(st->own, hist, max_bytes, hint, (int)ceil_index, ceil_size);
    *out = st.release();
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_rate_stepper_next(ojphgpu_rate_stepper* st, uint32_t* j)
{
  if (!st || !j) return OJPHGPU_E_INVALID;
  return no_throw([&] { return st->next(j); });
}

extern "C" int ojphgpu_rate_stepper_feed(ojphgpu_rate_stepper* st, int64_t size)
{
  if (!st) return OJPHGPU_E_INVALID;
  return no_throw([&] { return st->feed(size); });
}

extern "C" int ojphgpu_rate_stepper_info(const ojphgpu_rate_stepper* st, ojphgpu_rate_info* out)
{
  if (!st || !out) return OJPHGPU_E_INVALID;
  *out = st->info;
  return OJPHGPU_OK;
}

extern "C" void ojphgpu_rate_stepper_destroy(ojphgpu_rate_stepper* st) { delete st; }

extern "C" int ojphgpu_rate_rounds_create(const ojphgpu_plan* plan, const uint32_t* hist, const uint64_t* max_bytes, uint32_t frames, int32_t hint,
                                          ojphgpu_rate_rounds** out)
{
  if (!plan || !out || !max_bytes || frames == 0 || hint < -1 || hint >= (int32_t)OJPHGPU_RATE_GRID) return OJPHGPU_E_INVALID;
  *out = nullptr;
  return no_throw([&]() -> int {
    std::unique_ptr<ojphgpu_rate_rounds> r(new ojphgpu_rate_rounds());
    const int rc = rate_table_build(plan->plan, r->own);
    if (rc) return rc;
    r->start(r->own, hist, plan->plan.bands.size() * OJPHGPU_STATS_BINS, max_bytes, frames, hint);
    *out = r.release();
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_rate_rounds_next(ojphgpu_rate_rounds* r, uint32_t* idx, uint8_t* measures)
{
  if (!r || !idx || !measures) return OJPHGPU_E_INVALID;
  return no_throw([&] { return r->next(idx, measures); });
}

extern "C" int ojphgpu_rate_rounds_feed(ojphgpu_rate_rounds* r, const int64_t* sizes)
{
  if (!r || !sizes) return OJPHGPU_E_INVALID;
  return no_throw([&] { return r->feed(sizes); });
}

extern "C" int ojphgpu_rate_rounds_frame(const ojphgpu_rate_rounds* r, uint32_t frame, ojphgpu_rate_info* info)
{
  if (!r || !info || frame >= r->st.size() || r->failed || r->open[frame]) return OJPHGPU_E_INVALID;
  *info = r->info[frame];
  return r->rc[frame];
}

extern "C" int ojphgpu_rate_rounds_count(const ojphgpu_rate_rounds* r, uint32_t* rounds)
{
  if (!r || !rounds) return OJPHGPU_E_INVALID;
  *rounds = r->rounds;
  return OJPHGPU_OK;
}

extern "C" void ojphgpu_rate_rounds_destroy(ojphgpu_rate_rounds* r) { delete r; }

extern "C" int ojphgpu_rate_search(const ojphgpu_plan* plan, const uint32_t* hist, uint64_t max_bytes, ojphgpu_size_fn fn, void* user,
                                   ojphgpu_rate_info* out)
{
  return ojphgpu_rate_search_hint(plan, hist, max_bytes, -1, fn, user, out);
}

// Encoding to a quality target (include/ojphgpu.h section 5c): the coarsest index found whose trial meets max_sse.  Index 240
// first (the target cannot be met at all: OJPHGPU_E_QUALITY), then 0 (everything meets it), then halving between an index
// that failed (lo) and one that met (hi).  Nothing is assumed about fn between the two: whatever it returns, lo fails and hi
// meets and both were measured, so hi - lo == 1 is the certificate.  2 + ceil(log2(240)) = 10 trials at most, each at an
// index strictly inside the interval: none twice.
extern "C" int ojphgpu_quality_search(uint64_t max_sse, ojphgpu_sse_fn fn, void* user, ojphgpu_quality_info* out)
{
  if (!fn || !out) return OJPHGPU_E_INVALID;
  memset(out, 0, sizeof(*out));
  int64_t err = 0;
  auto trial = [&](uint32_t j, uint64_t& sse) -> bool {
    sse = 0;
    err = fn(user, j, &sse);
    out->passes++;
    return err >= 0;
  };
  auto fail = [&]() -> int { return err < INT32_MIN ? OJPHGPU_E_INVALID : (int)err; };
  uint32_t lo = 0, hi = OJPHGPU_RATE_GRID - 1;
  uint64_t sse_lo = 0, sse_hi = 0;
  if (!trial(hi, sse_hi)) return fail();
  if (sse_hi > max_sse) return OJPHGPU_E_QUALITY;
  if (!trial(lo, sse_lo)) return fail();
  if (sse_lo <= max_sse) { hi = 0; sse_hi = sse_lo; sse_lo = 0; }
  while (hi > lo + 1) {
    const uint32_t j = (lo + hi) / 2;
    uint64_t s;
    if (!trial(j, s)) return fail();
    if (s <= max_sse) { hi = j; sse_hi = s; } else { lo = j; sse_lo = s; }
  }
  out->grid_index = hi; out->qstep = rate_grid_qstep(hi);
  out->sse = sse_hi; out->sse_coarser = hi ? sse_lo : 0;
  return OJPHGPU_OK;
}

// The same search started from a guess, for the frames of a sequence (hint = the j* of the last certified frame).  lo = an
// index measured to fail (-1: none yet), hi = one measured to meet (241: none yet); hi - lo == 1 is the certificate, with lo
// == -1 standing for "j* == 0".  The hint first, then up to two neighbours on the side its result points to -- downwards
// while they still meet, upwards while they still fail -- and the first that turns round completes the certificate.  What
// is still open afterwards has one measured side: the probe of the other end (240, then 0, as the plain search asks them)
// and halving.  Nothing is assumed between two measured indices.  3 + 1 + ceil(log2(238)) = 12 trials at most, each
// strictly inside (lo, hi): none twice.
extern "C" int ojphgpu_quality_search_hint(uint64_t max_sse, int32_t hint, ojphgpu_sse_fn fn, void* user, ojphgpu_quality_info* out,
                                           uint32_t* first_guess)
{
  const int N = OJPHGPU_RATE_GRID;
  if (!fn || !out || !first_guess || hint < -1 || hint >= N) return OJPHGPU_E_INVALID;
  memset(out, 0, sizeof(*out));
  *first_guess = 0;
  int lo = -1, hi = N;
  uint64_t sse_lo = 0, sse_hi = 0;
  int64_t err = 0;
  auto trial = [&](int j) -> bool {                          // false: fn failed, err holds its value
    if (out->passes == 0) *first_guess = (uint32_t)j;
    uint64_t s = 0;
    err = fn(user, (uint32_t)j, &s);
    out->passes++;
    if (err < 0) return false;
    if (s <= max_sse) { hi = j; sse_hi = s; } else { lo = j; sse_lo = s; }
    return true;
  };
  auto fail = [&]() -> int { return err < INT32_MIN ? OJPHGPU_E_INVALID : (int)err; };
  if (hint >= 0) {
    if (!trial(hint)) return fail();
    const int dir = hi == hint ? -1 : 1;                     // it meets: a coarser step may, too; it fails: a finer one is needed
    for (int k = 1; k <= 2 && hi - lo > 1; ++k) {
      const int nb = hint + k * dir;
      if (nb <= lo || nb >= hi) break;                       // (off the grid)
      if (!trial(nb)) return fail();
    }
  }
  if (hi == N) {                                             // nothing meets so far: the finest step must
    if (lo < N - 1 && !trial(N - 1)) return fail();
    if (hi == N) return OJPHGPU_E_QUALITY;                   // SSE(240) > max_sse, measured
  }
  if (lo < 0 && hi > 0 && !trial(0)) return fail();          // nothing fails so far: the coarsest step may meet
  while (hi - lo > 1)
    if (!trial((lo + hi) / 2)) return fail();
  out->grid_index = (uint32_t)hi; out->qstep = rate_grid_qstep((uint32_t)hi);
  out->sse = sse_hi; out->sse_coarser = hi ? sse_lo : 0;
  return OJPHGPU_OK;
}

// Encoding to a quality target under a byte cap (include/ojphgpu.h section 5c, "under a byte cap"): the quality search, one
// size trial at its answer q and, only where that does not fit, the budget stepper below the ceiling q.  Every figure
// reported was measured; neither callback is asked an index twice.
namespace ojphgpu {
int capped_search(const RateTable& T, uint64_t max_sse, uint64_t cap_bytes, int hint_q, int hint_b, ojphgpu_sse_fn sse_fn,
                  ojphgpu_size_fn size_fn, ojphgpu_hist_fn hist_fn, void* user, ojphgpu_capped_info* info)
{
  const int N = OJPHGPU_RATE_GRID;
  if (!sse_fn || !size_fn || !hist_fn || !info || cap_bytes == 0 || hint_q < -1 || hint_q >= N || hint_b < -1 || hint_b >= N) return OJPHGPU_E_INVALID;
  memset(info, 0, sizeof(*info));
  info->quality_index = (uint32_t)N;
  struct Seen { ojphgpu_sse_fn fn; void* user; std::vector<int64_t> sse; } seen{ sse_fn, user, std::vector<int64_t>((size_t)N, -1) };
  auto record = [](void* u, uint32_t j, uint64_t* sse) -> int64_t {
    Seen& s = *(Seen*)u;
    const int64_t rc = s.fn(s.user, j, sse);
    if (rc >= 0 && j < (uint32_t)OJPHGPU_RATE_GRID) s.sse[j] = (int64_t)std::min<uint64_t>(*sse, (uint64_t)INT64_MAX);
    return rc;
  };
  ojphgpu_quality_info qi;
  int rc = ojphgpu_quality_search_hint(max_sse, hint_q, record, &seen, &qi, &info->first_guess_q);
  info->quality_passes = qi.passes;
  if (rc != OJPHGPU_OK && rc != OJPHGPU_E_QUALITY) return rc;
  const bool have_q = rc == OJPHGPU_OK;
  auto code = [](int64_t s) -> int { return s < INT32_MIN ? OJPHGPU_E_INVALID : (int)s; };
  int ceil = N; uint64_t ceil_size = 0;
  if (have_q) {
    const uint32_t q = qi.grid_index;
    info->quality_index = q;
    info->first_guess_b = q;
    const int64_t s = size_fn(user, q);
    info->rate_passes = 1;
    if (s < 0) return code(s);
    info->quality_bytes = (uint64_t)s;
    if ((uint64_t)s <= cap_bytes) {
      info->outcome = OJPHGPU_CAPPED_MET;
      info->grid_index = q; info->qstep = rate_grid_qstep(q);
      info->bytes = (uint64_t)s;
      info->sse = qi.sse; info->sse_coarser = qi.sse_coarser;
      return OJPHGPU_OK;
    }
    if (q == 0) return OJPHGPU_E_BUDGET;                     // size(0) > B, measured
    ceil = (int)q; ceil_size = (uint64_t)s;
  }
  info->outcome = OJPHGPU_CAPPED_BY_BUDGET;
  const uint32_t* hist = hist_fn(user);                      // once; NULL: plain halving
  ojphgpu_rate_stepper st;
  st.start(T, hist, cap_bytes, hint_b, ceil, ceil_size);
  for (;;) {
    uint32_t j = 0;
    rc = st.next(&j);
    if (rc == 1) rc = st.feed(size_fn(user, j)); else break;
    if (rc) break;
  }
  info->rate_passes += st.info.passes;
  if (st.info.passes) info->first_guess_b = st.info.first_guess;
  if (rc) return rc;                                         // OJPHGPU_E_BUDGET as it is
  const uint32_t j = st.info.grid_index;
  info->grid_index = j; info->qstep = st.info.qstep; info->bytes = st.info.bytes; info->bytes_finer = st.info.bytes_finer;
  if (seen.sse[j] < 0) {                                     // not among the quality trials: measured now, and counted
    uint64_t s = 0;
    const int64_t e = record(&seen, j, &s);
    info->quality_passes++;
    if (e < 0) return code(e);
    info->sse = s;
  } else info->sse = (uint64_t)seen.sse[j];
  return OJPHGPU_OK;
}
}  // namespace ojphgpu

extern "C" int ojphgpu_capped_search(const ojphgpu_plan* plan, uint64_t max_sse, uint64_t cap_bytes, int32_t hint_q, int32_t hint_b,
                                     ojphgpu_sse_fn sse_fn, ojphgpu_size_fn size_fn, ojphgpu_hist_fn hist_fn, void* user, ojphgpu_capped_info* info)
{
  if (!plan) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    RateTable T;
    const int rc = rate_table_build(plan->plan, T);
    if (rc) return rc;
    return capped_search(T, max_sse, cap_bytes, hint_q, hint_b, sse_fn, size_fn, hist_fn, user, info);
  });
}

extern "C" int ojphgpu_rate_predict(const ojphgpu_plan* plan, const uint32_t* hist, double* out)
{
  if (!plan || !hist || !out) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    RateTable T;
    const int rc = rate_table_build(plan->plan, T);
    if (rc) return rc;
    RateModel m(T, hist);
    for (uint32_t j = 0; j < OJPHGPU_RATE_GRID; ++j) out[j] = m.bytes(j);
    return OJPHGPU_OK;
  });
}

// ---------------------------------------------------------------------------------------------------------------------
// A reversible frame under a byte cap (include/ojphgpu.h section 5f): the ladder of truncation tables and the search.
// ---------------------------------------------------------------------------------------------------------------------
namespace ojphgpu {

bool trunc_plan_ok(const Plan& P)
{
  if (P.parsed || !P.atks.empty() || !P.dfss.empty() || P.p.wavelet != 0 || P.any_wide || P.p.num_comps == 0) return false;
  const CodStyle& s0 = P.style(0);
  for (uint32_t c = 0; c < P.p.num_comps; ++c) {
    const CodStyle& st = P.style(c);
    if (!st.rev || st.wavelet >= 2 || st.dfs >= 0 || st.L != s0.L) return false;
    if (c < P.wide.size() && P.wide[c]) return false;
  }
  return true;
}

// L2 norm of the 1-D 5/3 synthesis basis vector of the low (high) branch at decomposition depth d: a unit impulse in that
// band taken through the linear inverse lifting, d levels, in double, in the middle of a line of 64 coefficients at depth d
// (the vector spans fewer than 8 of them, so the borders play no part).  Beyond depth 12 the line would get long for
// nothing: every further level of low-pass synthesis multiplies the norm by sqrt(2) to within 4^-d.
static double trunc_synth_norm(uint32_t d, bool high)
{
  if (d == 0) return 1.0;
  const uint32_t dd = std::min(d, 12u);
  size_t n = 64;
  std::vector<double> s(n, 0.0), h(n, 0.0), x;
  (high ? h : s)[n / 2] = 1.0;
  for (uint32_t lev = dd; lev >= 1; --lev) {
    x.assign(2 * n, 0.0);
    for (size_t i = 0; i < n; ++i) x[2 * i] = s[i] - (h[i ? i - 1 : 0] + h[i]) / 4.0;
    for (size_t i = 0; i < n; ++i) x[2 * i + 1] = h[i] + (x[2 * i] + x[i + 1 < n ? 2 * i + 2 : 2 * i]) / 2.0;
    s = x; n *= 2; h.assign(n, 0.0);
  }
  double e = 0;
  for (double v : x) e += v * v;
  return std::sqrt(e) * std::exp2(0.5 * (double)(d - dd));
}

int trunc_ladder_build(const Plan& P, TruncLadder& T)
{
  if (!trunc_plan_ok(P) || P.bands.empty()) return OJPHGPU_E_INVALID;
  const size_t nb = P.bands.size();
  std::vector<double> w(nb);
  std::map<uint32_t, double> lo, hi;                         // by depth
  auto norm = [&](uint32_t d, bool high) { auto& m = high ? hi : lo; auto it = m.find(d); if (it == m.end()) it = m.emplace(d, trunc_synth_norm(d, high)).first; return it->second; };
  const bool rct = P.p.color_transform != 0 && P.p.num_comps >= 3;
  double wmin = 0;
  for (size_t i = 0; i < nb; ++i) {
    const Band& B = P.bands[i];
    const uint32_t L = P.style(B.comp).L, d = B.res == 0 ? L : L - B.res + 1;
    const bool hh = B.band == 1 || B.band == 3, vh = B.band == 2 || B.band == 3;   // HL, HH: high horizontally; LH, HH: vertically
    const double gc = rct && B.comp < 3 ? (B.comp == 0 ? std::sqrt(3.0) : std::sqrt(11.0 / 16.0)) : 1.0;
    w[i] = std::log2(norm(d, hh) * norm(d, vh) * gc);
    if (i == 0 || w[i] < wmin) wmin = w[i];
  }
  T.q.resize(nb); T.top.resize(nb);
  int64_t last = 0;
  for (size_t i = 0; i < nb; ++i) {
    T.q[i] = (int32_t)std::floor(4.0 * (w[i] - wmin) + 0.5);
    T.top[i] = (uint8_t)(P.bands[i].K_max ? std::min(P.bands[i].K_max, 32u) - 1u : 0u);
    last = std::max<int64_t>(last, 4 * (int64_t)T.top[i] + T.q[i]);
  }
  T.levels = (uint32_t)std::max<int64_t>(last - 3 + 1, 1);
  // the classes of bands (component, resolution, orientation): a table has one entry per class on the device
  std::map<uint64_t, uint32_t> ids;
  T.band_class.resize(nb); T.class_band.clear();
  for (size_t i = 0; i < nb; ++i) {
    const Band& B = P.bands[i];
    const uint64_t key = ((uint64_t)B.comp << 16) | ((uint64_t)B.res << 8) | B.band;
    auto it = ids.find(key);
    if (it == ids.end()) { it = ids.emplace(key, (uint32_t)T.class_band.size()).first; T.class_band.push_back((uint32_t)i); }
    T.band_class[i] = it->second;
  }
  return OJPHGPU_OK;
}

// The model of the search: a coefficient of bit length len > t costs about len - t + 3 bits, the constants are those of
// RateModel.  Only its shape matters: it is rescaled by what a trial measures.
static double trunc_predict(const TruncLadder& T, const uint32_t* hist, uint64_t num_blocks, uint32_t j)
{
  double bits = 0;
  for (size_t b = 0; b < T.q.size(); ++b) {
    const uint32_t t = T.drop(j, b);
    for (uint32_t len = t + 1; len <= 32; ++len) bits += (double)hist[b * OJPHGPU_STATS_BINS + len] * (double)(len - t + 3);
  }
  return bits / 8.0 + 300.0 + 6.0 * (double)num_blocks;
}

// the levels whose table differs from the level before (level 0 first)
std::vector<uint32_t> trunc_distinct_levels(const TruncLadder& T)
{
  std::vector<uint32_t> u;
  for (uint32_t j = 0; j < T.levels; ++j) {
    bool differs = j == 0;
    for (size_t b = 0; b < T.q.size() && !differs; ++b) differs = T.drop(j, b) != T.drop(j - 1, b);
    if (differs) u.push_back(j);
  }
  return u;
}

int trunc_search(const TruncLadder& T, uint64_t num_blocks, const uint32_t* hist, uint64_t max_bytes, ojphgpu_size_fn fn, void* user, ojphgpu_trunc_info* out)
{
  memset(out, 0, sizeof(*out));
  const std::vector<uint32_t> u = trunc_distinct_levels(T);   // only they are measured
  const int64_t U = (int64_t)u.size();
  // lo: the largest index measured NOT to fit (-1: none), hi: the smallest measured to fit (U: none); hi - lo == 1 ends it
  int64_t lo = -1, hi = U; uint64_t size_lo = 0, size_hi = 0;
  double scale = 1.0;
  bool guided = false;                                      // the model has led its trial: level 0, the model's level, then halving (the pass cap)
  auto measure = [&](int64_t k) -> int {
    const int64_t sz = fn(user, u[(size_t)k]);
    if (sz < 0) return (int)sz;
    out->passes++;
    if (hist) { const double pr = trunc_predict(T, hist, num_blocks, u[(size_t)k]); if (pr > 0) scale = (double)sz / pr; }
    if ((uint64_t)sz <= max_bytes) { hi = k; size_hi = (uint64_t)sz; } else { lo = k; size_lo = (uint64_t)sz; }
    return 0;
  };
  auto propose = [&]() -> int64_t {                         // the first index the (rescaled) model says fits, inside (lo, hi)
    for (int64_t k = lo + 1; k < hi; ++k) if (scale * trunc_predict(T, hist, num_blocks, u[(size_t)k]) <= (double)max_bytes) return k;
    return hi - 1;
  };
  while (hi - lo > 1) {
    int64_t k;
    if (out->passes == 0) k = 0;                             // lossless first: a frame that fits takes one pass, and its size scales the model
    else if (hist && !guided) { guided = true; k = propose(); }
    else k = lo + (hi - lo) / 2;
    if (out->passes <= 1) out->first_guess = u[(size_t)k];
    const int rc = measure(k);
    if (rc) return rc;
  }
  if (hi == U) return OJPHGPU_E_BUDGET;
  out->level = u[(size_t)hi]; out->bytes = size_hi; out->bytes_finer = lo >= 0 ? size_lo : 0;
  out->lossless = hi == 0;
  for (size_t b = 0; b < T.q.size(); ++b) out->max_dropped = std::max<uint32_t>(out->max_dropped, T.drop(out->level, b));
  return OJPHGPU_OK;
}

// Near-lossless coding (include/ojphgpu.h section 5g): the coarsest distinct level found that meets both bounds, by halving
// between level 0 (meets by contract, never measured) and a virtual level behind the last (does not meet).  Nothing is
// assumed of fn between two measured levels: the certificate is the measurement of u[k*] and that of u[k* + 1].
int near_lossless_search(const TruncLadder& T, uint64_t max_sse, uint32_t max_pae, ojphgpu_err_fn fn, void* user, ojphgpu_near_lossless_info* out)
{
  memset(out, 0, sizeof(*out));
  if (max_sse == UINT64_MAX && max_pae == UINT32_MAX) return OJPHGPU_E_INVALID;
  const std::vector<uint32_t> u = trunc_distinct_levels(T);
  size_t lo = 0, hi = max_sse == 0 || max_pae == 0 ? 1 : u.size();   // (a bound of 0: level 0, the only level known to meet it)
  while (hi - lo > 1) {
    const size_t k = lo + (hi - lo) / 2;
    uint64_t sse = 0; uint32_t pae = 0;
    const int rc = fn(user, u[k], &sse, &pae);
    if (rc) return rc;
    out->passes++;
    if (sse <= max_sse && pae <= max_pae) { lo = k; out->sse = sse; out->pae = pae; }
    else { hi = k; out->level_coarser = u[k]; out->sse_coarser = sse; out->pae_coarser = pae; }
  }
  out->level = u[lo]; out->lossless = lo == 0;
  for (size_t b = 0; b < T.q.size(); ++b) out->max_dropped = std::max<uint32_t>(out->max_dropped, T.drop(out->level, b));
  return OJPHGPU_OK;
}

}  // namespace ojphgpu

extern "C" int ojphgpu_plan_trunc_levels(const ojphgpu_plan* plan, uint32_t* levels)
{
  if (!plan || !levels) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    TruncLadder T;
    const int rc = trunc_ladder_build(plan->plan, T);
    if (rc) return rc;
    *levels = T.levels;
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_plan_trunc_weights(const ojphgpu_plan* plan, int32_t* q)
{
  if (!plan || !q) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    TruncLadder T;
    const int rc = trunc_ladder_build(plan->plan, T);
    if (rc) return rc;
    std::copy(T.q.begin(), T.q.end(), q);
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_plan_trunc_table(const ojphgpu_plan* plan, uint32_t j, uint8_t* t)
{
  if (!plan || !t) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    TruncLadder T;
    const int rc = trunc_ladder_build(plan->plan, T);
    if (rc) return rc;
    if (j >= T.levels) return OJPHGPU_E_INVALID;
    for (size_t b = 0; b < T.q.size(); ++b) t[b] = T.drop(j, b);
    return OJPHGPU_OK;
  });
}

extern "C" int ojphgpu_trunc_search(const ojphgpu_plan* plan, const uint32_t* hist, uint64_t max_bytes, ojphgpu_size_fn fn, void* user,
                                    ojphgpu_trunc_info* info)
{
  if (!plan || !fn || !info) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    TruncLadder T;
    const int rc = trunc_ladder_build(plan->plan, T);
    if (rc) return rc;
    return trunc_search(T, plan->plan.blocks.size(), hist, max_bytes, fn, user, info);
  });
}

extern "C" int ojphgpu_near_lossless_search(const ojphgpu_plan* plan, uint64_t max_sse, uint32_t max_pae, ojphgpu_err_fn err_fn, void* user,
                                            ojphgpu_near_lossless_info* info)
{
  if (!plan || !err_fn || !info) return OJPHGPU_E_INVALID;
  return no_throw([&]() -> int {
    TruncLadder T;
    const int rc = trunc_ladder_build(plan->plan, T);
    if (rc) return rc;
    for (const CompGeo& g : plan->plan.comps) if (g.bit_depth > 16) return OJPHGPU_E_INVALID;
    return near_lossless_search(T, max_sse, max_pae, err_fn, user, info);
  });
}
