// The host model of the mate-pair join (ghostm_amd/csrc/pair_join_host.cpp,
// pair_join.h), without a device: random calls through GhostmPairJoinHost
// against an evaluation that lists every concordant (i, j) of a pair and sorts
// the list, the contract's limits, and every refusal with the outputs untouched.
// Build: g++ -std=c++17 -fsanitize=address,undefined tests/native/test_pair_join.cpp
// ghostm_amd/csrc/pair_join_host.cpp; it runs directly, with nothing preloaded.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "../../ghostm_amd/csrc/pair_join.h"

namespace ghostm {
static std::string g_last;
void SetLastErrorMessage(const std::string &m) { g_last = m; }
}  // namespace ghostm

using namespace ghostm;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static bool Has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

struct Call {
  std::vector<uint32_t> begin, offset;
  std::vector<GhostmPairHit> hit;
  uint32_t max_span = 600, orient = 1;
};

struct Result {
  std::vector<GhostmLcaHit> cand;
  std::vector<uint32_t> partner;
  std::vector<GhostmPairOut> out;
};

static bool SameHit(const GhostmLcaHit &a, const GhostmLcaHit &b) {
  return a.node == b.node && a.score == b.score && a.q_lo == b.q_lo && a.q_hi == b.q_hi;
}

// every concordant (i, j) of a pair in one list, sorted by i, then score of j descending, then j
static Result ByLists(const Call &c) {
  const size_t n = c.hit.size(), np = c.offset.size();
  Result r{std::vector<GhostmLcaHit>(n, GhostmLcaHit{0, 0, 0, 0}), std::vector<uint32_t>(n, kPairNone),
           std::vector<GhostmPairOut>(np, GhostmPairOut{0, 0, 0, 0})};
  for (size_t p = 0; p < np; ++p) {
    const uint32_t b = c.begin[2 * p], m = c.begin[2 * p + 1], e = c.begin[2 * p + 2], off = c.offset[p];
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t>> list;  // i, ~score_j, j
    for (uint32_t i = b; i < m; ++i)
      for (uint32_t j = m; j < e; ++j) {
        const GhostmPairHit &x = c.hit[i], &y = c.hit[j];
        if (!x.score || !y.score || x.subject != y.subject) continue;
        if (c.orient && x.strand == y.strand) continue;
        const uint64_t lo = std::min(x.s_lo, y.s_lo), hi = std::max(x.s_hi, y.s_hi);
        if (hi - lo + 1 > c.max_span) continue;
        list.emplace_back(i, ~y.score, j);
      }
    std::sort(list.begin(), list.end());
    GhostmPairOut &o = r.out[p];
    uint32_t span_score = 0;
    for (size_t k = 0; k < list.size(); ++k) {
      const uint32_t i = std::get<0>(list[k]), j = std::get<2>(list[k]);
      if (k && std::get<0>(list[k - 1]) == i) continue;  // the first entry of i is its partner
      r.partner[i] = j;
      if (r.partner[j] == kPairNone) r.partner[j] = i;  // i ascends
      ++o.joined;
      const uint32_t total = c.hit[i].score + c.hit[j].score;
      r.cand[i] = GhostmLcaHit{c.hit[i].node, total, c.hit[i].q_lo, off + c.hit[j].q_hi};
      if (total > span_score) {
        span_score = total;
        o.best_span = std::max(c.hit[i].s_hi, c.hit[j].s_hi) - std::min(c.hit[i].s_lo, c.hit[j].s_lo) + 1;
      }
    }
    for (uint32_t i = b; i < e; ++i) {
      const GhostmPairHit &h = c.hit[i];
      if (!h.score) continue;
      o.mates |= i < m ? 1u : 2u;
      if (r.partner[i] == kPairNone) {
        const uint32_t add = i < m ? 0 : off;
        r.cand[i] = GhostmLcaHit{h.node, h.score, h.q_lo + add, h.q_hi + add};
      }
      o.best_score = std::max(o.best_score, r.cand[i].score);
    }
  }
  return r;
}

static int Run(const Call &c, Result *r, uint32_t fill = 0) {
  const size_t n = c.hit.size(), np = c.offset.size();
  r->cand.assign(n, GhostmLcaHit{fill, fill, fill, fill});
  r->partner.assign(n, fill ? fill : kPairNone);
  r->out.assign(np, GhostmPairOut{fill, fill, fill, fill});
  return GhostmPairJoinHost((uint32_t)np, c.begin.data(), c.offset.data(), (uint32_t)n, c.hit.data(), c.max_span,
                            c.orient, r->cand.data(), r->partner.data(), r->out.data());
}

static Call RandomCall(std::mt19937 &g) {
  Call c;
  c.max_span = std::vector<uint32_t>{1, 150, 600, 600, 1u << 24}[g() % 5];
  c.orient = g() % 2;
  const uint32_t np = 1 + g() % 5;
  c.begin.push_back(0);
  for (uint32_t p = 0; p < np; ++p) {
    c.offset.push_back(std::vector<uint32_t>{0, 1, 100, 151}[g() % 4]);
    for (int half = 0; half < 2; ++half) {
      const uint32_t k = std::vector<uint32_t>{0, 1, 2, 3, 8, 20, 40, 90}[g() % 8];
      for (uint32_t t = 0; t < k; ++t) {
        GhostmPairHit h{};
        h.subject = g() % 5;
        h.node = h.subject ? 10 + h.subject : kPairNone;
        h.score = g() % 7 == 0 ? 0 : std::vector<uint32_t>{20, 30, 30, 40, 1 + g() % 199}[g() % 5];
        h.q_lo = g() % 60;
        h.q_hi = h.q_lo + g() % 90;
        h.s_lo = g() % 1200;
        h.s_hi = h.s_lo + g() % 150;
        h.strand = g() % 2;
        c.hit.push_back(h);
      }
      c.begin.push_back((uint32_t)c.hit.size());
    }
  }
  return c;
}

int main() {
  std::mt19937 g(20270104);
  uint64_t joined = 0, taken = 0, trials = 0;
  for (int t = 0; t < 400; ++t) {
    const Call c = RandomCall(g);
    Result got;
    CHECK(Run(c, &got) == 0);
    const Result want = ByLists(c);
    for (size_t i = 0; i < c.hit.size(); ++i) {
      CHECK(SameHit(got.cand[i], want.cand[i]));
      CHECK(got.partner[i] == want.partner[i]);
    }
    for (size_t p = 0; p < c.offset.size(); ++p) {
      const GhostmPairOut &a = got.out[p], &b = want.out[p];
      CHECK(a.joined == b.joined && a.mates == b.mates && a.best_score == b.best_score && a.best_span == b.best_span);
      joined += a.joined;
      for (uint32_t j = c.begin[2 * p + 1]; j < c.begin[2 * p + 2]; ++j) taken += got.partner[j] != kPairNone;
    }
    ++trials;
  }
  CHECK(joined > 1000 && taken > 500 && taken < joined);

  // the limits: the largest values join and stay below 2^25
  {
    Call c;
    const uint32_t top = kPairValueLimit - 1;
    c.begin = {0, 1, 2};
    c.offset = {top};
    c.hit = {GhostmPairHit{3, 5, top, 0, top, 0, top, 0}, GhostmPairHit{3, 5, top, top, top, 0, top, 1}};
    c.max_span = kPairValueLimit;
    Result r;
    CHECK(Run(c, &r) == 0);
    CHECK(r.cand[0].score == 2 * top && r.cand[0].q_hi == 2 * top && r.cand[0].q_hi < (1u << 25));
    CHECK(r.out[0].joined == 1 && r.out[0].best_span == kPairValueLimit && r.partner[1] == 0 && r.cand[1].score == 0);
    c.max_span = kPairValueLimit - 1;
    CHECK(Run(c, &r) == 0);
    CHECK(r.out[0].joined == 0 && r.cand[1].q_lo == 2 * top);
  }

  // the refusals: each names its reason and writes nothing
  {
    Call ok;
    ok.begin = {0, 2, 3, 3, 4};
    ok.offset = {100, 120};
    ok.hit = {GhostmPairHit{7, 70, 50, 0, 49, 100, 149, 0}, GhostmPairHit{8, 80, 40, 0, 49, 10, 59, 1},
              GhostmPairHit{7, 70, 30, 0, 49, 300, 349, 1}, GhostmPairHit{8, 80, 20, 0, 49, 30, 90, 0}};
    const uint32_t fill = 0xC3C3C3C3u;
    const auto refused = [&](const Call &c, const char *reason) {
      Result r;
      CHECK(Run(c, &r, fill) == 1);
      CHECK(Has(g_last, "GhostmPairJoinHost: ") && Has(g_last, reason));
      for (const GhostmLcaHit &h : r.cand) CHECK(h.node == fill && h.score == fill && h.q_lo == fill && h.q_hi == fill);
      for (uint32_t v : r.partner) CHECK(v == fill);
      for (const GhostmPairOut &o : r.out) CHECK(o.joined == fill && o.mates == fill && o.best_span == fill);
      ++trials;
    };
    Call c = ok;
    c.begin = {0, 3, 2, 3, 4};
    refused(c, "reads: ");
    c = ok;
    c.begin = {0, 2, 3, 3, 5};
    refused(c, "reads: ");
    c = ok;
    c.hit.assign(kPairHitLimit + 1, GhostmPairHit{});
    c.begin = {0, 9000, kPairHitLimit + 1};
    c.offset = {100};
    refused(c, "reads: ");
    c = ok;
    c.hit[1].q_lo = 50;
    refused(c, "range: ");
    c = ok;
    c.hit[2].s_lo = 350;
    refused(c, "range: ");
    c = ok;
    c.hit[3].q_hi = kPairValueLimit;
    refused(c, "bounds: ");
    c = ok;
    c.hit[0].score = kPairValueLimit;
    refused(c, "bounds: ");
    c = ok;
    c.hit[0].strand = 2;
    refused(c, "bounds: ");
    c = ok;
    c.offset[1] = kPairValueLimit;
    refused(c, "bounds: ");
    c = ok;
    c.max_span = 0;
    refused(c, "param: ");
    c = ok;
    c.max_span = kPairValueLimit + 1;
    refused(c, "param: ");
    c = ok;
    c.orient = 2;
    refused(c, "param: ");
    Result r;
    CHECK(Run(ok, &r) == 0);
    CHECK(GhostmPairJoinHost(2, ok.begin.data(), ok.offset.data(), 4, ok.hit.data(), 600, 1, nullptr, r.partner.data(),
                             r.out.data()) == 1 && Has(g_last, "null: "));
    CHECK(GhostmPairJoinHost(2, nullptr, ok.offset.data(), 4, ok.hit.data(), 600, 1, r.cand.data(), r.partner.data(),
                             r.out.data()) == 1 && Has(g_last, "null: "));
    CHECK(GhostmPairJoinHost(0, nullptr, nullptr, 0, nullptr, 600, 1, nullptr, nullptr, nullptr) == 0);
    // pairs without hits past the first hit need no cand: no arithmetic on a null pointer
    const std::vector<uint32_t> flat{4, 4, 4, 4, 4};
    CHECK(GhostmPairJoinHost(2, flat.data(), ok.offset.data(), 4, ok.hit.data(), 600, 1, nullptr, nullptr,
                             r.out.data()) == 0 && r.out[1].mates == 0);
  }
  std::printf("%llu trials ok\n", (unsigned long long)trials);
  return 0;
}
