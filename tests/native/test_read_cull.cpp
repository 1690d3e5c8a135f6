// The segment arithmetic of the read-level cull (ghostm_amd/csrc/read_cull.h),
// without a device: the covered count of a range and the whole cull of a read
// on sorted endpoints, against one counter per position; the rank key, the two
// tests at their limits, the table size and the refusals.
// Build: g++ -std=c++17 tests/native/test_read_cull.cpp (the test adds
// -fsanitize=address,undefined in a second run).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../ghostm_amd/csrc/read_cull.h"

using namespace ghostm;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

// the cull of one read with a counter per position
static std::vector<GhostmCullOut> PerPosition(const std::vector<GhostmCullHit> &hit, uint32_t base, uint32_t top_k,
                                              uint32_t pct, uint32_t span) {
  const uint32_t n = (uint32_t)hit.size();
  std::vector<GhostmCullOut> out(n);
  std::vector<uint32_t> depth(span, 0), done(n, 0), kept;
  for (uint32_t r = 0; r < n; ++r) {
    uint32_t best = n;  // selection: the highest score not yet taken, the lowest index first
    for (uint32_t i = 0; i < n; ++i)
      if (!done[i] && (best == n || hit[i].score > hit[best].score)) best = i;
    done[best] = 1;
    const GhostmCullHit &h = hit[best];
    GhostmCullOut o{r, GHOSTM_CULL_EMPTY, 0xFFFFFFFFu, 0};
    if (h.score) {
      bool dup = false;
      for (uint32_t k : kept) {
        const GhostmCullHit &o2 = hit[k];
        bool q = false, s = false;
        for (uint32_t p = h.q_lo; p <= h.q_hi && !q; ++p) q = p >= o2.q_lo && p <= o2.q_hi;
        for (uint32_t p = h.s_lo; p <= h.s_hi && !s; ++p) s = p >= o2.s_lo && p <= o2.s_hi;
        if (o2.subject == h.subject && q && s) {
          o.status = GHOSTM_CULL_DUP;
          o.detail = base + k;
          dup = true;
          break;
        }
      }
      if (!dup) {
        uint32_t d = 0;
        for (uint32_t p = h.q_lo; p <= h.q_hi; ++p) d += depth[p] >= top_k;
        o.detail = d;
        if ((uint64_t)d * 100 >= (uint64_t)pct * (h.q_hi - h.q_lo + 1)) {
          o.status = GHOSTM_CULL_CULLED;
        } else {
          o.status = GHOSTM_CULL_KEPT;
          o.kept_rank = (uint32_t)kept.size();
          kept.push_back(best);
          for (uint32_t p = h.q_lo; p <= h.q_hi; ++p) ++depth[p];
        }
      }
    }
    out[best] = o;
  }
  return out;
}

static bool Same(const GhostmCullOut &a, const GhostmCullOut &b) {
  return a.order == b.order && a.status == b.status && a.kept_rank == b.kept_rank && a.detail == b.detail;
}

int main() {
  // the key: score descending, then index ascending; a score of 0 is last
  CHECK(CullKey(9, 5) < CullKey(8, 0));
  CHECK(CullKey(9, 0) < CullKey(9, 1));
  CHECK(CullKey(1, 0xFFFFFFFFu) < CullKey(0, 0));
  CHECK(CullKey(0xFFFFFFFFu, 0) == 0);
  // the cull test at the coordinate limit: 2^25 positions, all covered
  CHECK(CullCovered(kCullCoordLimit, kCullCoordLimit, 100));
  CHECK(!CullCovered(kCullCoordLimit - 1, kCullCoordLimit, 100));
  CHECK(CullCovered(50, 100, 50) && !CullCovered(49, 100, 50) && CullCovered(1, 100, 1) && !CullCovered(0, 1, 1));
  // ranges meet on a shared position only
  {
    const GhostmCullHit a{1, 5, 0, 99, 0, 99}, b{1, 4, 100, 120, 50, 60}, c{1, 3, 99, 120, 99, 99},
        d{2, 3, 99, 120, 99, 99}, e{1, 3, 99, 120, 100, 100};
    CHECK(!CullSameAlignment(a, b) && CullSameAlignment(a, c) && CullSameAlignment(c, a));
    CHECK(!CullSameAlignment(a, d) && !CullSameAlignment(a, e));
  }
  CHECK(CullPow2(0) == 2 && CullPow2(2) == 2 && CullPow2(3) == 4 && CullPow2(1024) == 1024 && CullPow2(1025) == 2048);
  CHECK(CullPow2(kCullReadLimit) == kCullReadLimit);
  CHECK((uint64_t)kCullTableArrays * kCullReadLimit < (1ull << 32));

  // segments: equal endpoints, a hit of one position, the table's ends
  {
    const std::vector<GhostmCullHit> h = {{0, 9, 10, 19, 0, 9}, {1, 8, 10, 10, 0, 0}, {2, 7, 19, 30, 0, 11},
                                          {3, 0, 0, 100, 0, 100}, {4, 6, 10, 19, 0, 9}};
    CullSegments seg;
    seg.Build(h.data(), (uint32_t)h.size());
    CHECK(seg.ep.size() == 8);  // the hit without a score has no endpoint
    CHECK(seg.Covered(10, 19, 1) == 0);
    seg.Add(10, 19);
    CHECK(seg.Covered(10, 19, 1) == 10 && seg.Covered(10, 10, 1) == 1 && seg.Covered(19, 30, 1) == 1);
    CHECK(seg.Covered(10, 19, 2) == 0);
    seg.Add(19, 30);
    CHECK(seg.Covered(10, 19, 2) == 1 && seg.Covered(19, 30, 1) == 12 && seg.Covered(10, 10, 2) == 0);
  }

  // random reads against the per-position cull
  std::mt19937 gen(20261120);
  const auto rng = [&] { return (uint32_t)gen(); };
  unsigned trials = 0, seen[4] = {0, 0, 0, 0};
  for (int t = 0; t < 600; ++t) {
    const uint32_t span = t % 3 == 0 ? 4 : t % 3 == 1 ? 60 : 700;
    const uint32_t n = rng() % (t % 5 == 0 ? 90 : 12);
    const uint32_t top_k = t % 7 == 0 ? 255 : 1 + rng() % 3, pct = 1 + rng() % 100, base = rng() % 1000;
    std::vector<GhostmCullHit> hit(n);
    for (auto &h : hit) {
      h.subject = rng() % 3;
      h.score = rng() % 8 == 0 ? 0 : 1 + rng() % 20;
      h.q_lo = rng() % span;
      h.q_hi = std::min(span - 1, h.q_lo + rng() % (1 + rng() % span));
      h.s_lo = rng() % span;
      h.s_hi = std::min(span - 1, h.s_lo + rng() % (1 + rng() % span));
    }
    std::vector<GhostmCullOut> got(n);
    CullRead(hit.data(), n, base, top_k, pct, got.data());
    const std::vector<GhostmCullOut> want = PerPosition(hit, base, top_k, pct, span);
    for (uint32_t i = 0; i < n; ++i) {
      CHECK(Same(got[i], want[i]));
      ++seen[got[i].status];
    }
    ++trials;
  }
  CHECK(seen[0] > 100 && seen[1] > 100 && seen[2] > 100 && seen[3] > 100);

  // the refusals, in the order of the checks
  {
    const uint32_t rb[3] = {0, 2, 3}, back[3] = {0, 3, 2}, past[3] = {0, 2, 4};
    GhostmCullHit h[3] = {{1, 5, 0, 9, 0, 9}, {1, 4, 5, 6, 5, 6}, {2, 3, 0, 0, 0, 0}};
    CHECK(ValidateReadCull(2, rb, 3, h, 1, 50).empty());
    CHECK(ValidateReadCull(0, nullptr, 0, nullptr, 255, 100).empty());
    CHECK(ValidateReadCull(2, rb, 3, h, 0, 50).rfind("param: ", 0) == 0);
    CHECK(ValidateReadCull(2, rb, 3, h, 256, 50).rfind("param: ", 0) == 0);
    CHECK(ValidateReadCull(2, rb, 3, h, 1, 0).rfind("param: ", 0) == 0);
    CHECK(ValidateReadCull(2, rb, 3, h, 1, 101).rfind("param: ", 0) == 0);
    CHECK(ValidateReadCull(2, nullptr, 3, h, 1, 50).rfind("null: ", 0) == 0);
    CHECK(ValidateReadCull(2, rb, 3, nullptr, 1, 50).rfind("null: ", 0) == 0);
    CHECK(ValidateReadCull(2, back, 3, h, 1, 50).rfind("reads: ", 0) == 0);
    CHECK(ValidateReadCull(2, past, 3, h, 1, 50).rfind("reads: ", 0) == 0);
    const uint32_t huge[2] = {0, kCullReadLimit + 1};
    CHECK(ValidateReadCull(1, huge, kCullReadLimit + 1, h, 1, 50).rfind("reads: ", 0) == 0);
    h[1].q_lo = 7;
    CHECK(ValidateReadCull(2, rb, 3, h, 1, 50).rfind("range: ", 0) == 0);
    h[1].q_lo = 5;
    h[2].s_hi = kCullCoordLimit;
    CHECK(ValidateReadCull(2, rb, 3, h, 1, 50).rfind("bounds: ", 0) == 0);
    h[2].s_hi = h[2].s_lo = kCullCoordLimit - 1;
    CHECK(ValidateReadCull(2, rb, 3, h, 1, 50).empty());
  }
  std::printf("%u trials ok\n", trials);
  return 0;
}
