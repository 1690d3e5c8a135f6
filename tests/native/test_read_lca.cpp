// The host arithmetic of the per-read taxonomic assignment
// (ghostm_amd/csrc/read_lca.h), without a device: the depths and their
// refusals, one read's climb against counts over explicit ancestor paths on
// random trees, the score test and the threshold at their limits, the checks,
// and the two text parsers.
// Build: g++ -std=c++17 tests/native/test_read_lca.cpp (the test adds
// -fsanitize=address,undefined in a second run).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../../ghostm_amd/csrc/read_lca.h"

using namespace ghostm;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static bool Has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

// one read by ancestor paths: a counter per node
static GhostmLcaOut ByPaths(const std::vector<uint32_t> &parent, const std::vector<uint32_t> &depth,
                            const std::vector<GhostmLcaHit> &hit, uint32_t top_pct, uint32_t support_pct) {
  GhostmLcaOut o{kLcaNone, 0, 0, 0, kLcaNone, 0, 0, 0};
  std::map<uint32_t, uint32_t> count;
  for (const GhostmLcaHit &h : hit) {
    if (!h.score) continue;
    ++o.candidates;
    o.best_score = std::max(o.best_score, h.score);
    uint32_t ref = 0;
    for (const GhostmLcaHit &g : hit) {
      bool shared = false;
      if (g.score)
        for (uint32_t p = g.q_lo; p <= g.q_hi && !shared; ++p) shared = p >= h.q_lo && p <= h.q_hi;
      if (shared) ref = std::max(ref, g.score);
    }
    if ((uint64_t)h.score * 100 < (uint64_t)(100 - top_pct) * ref) continue;
    if (h.node == kLcaNone) {
      ++o.unmapped;
      continue;
    }
    ++o.votes;
    for (uint32_t n = h.node;; n = parent[n]) {
      ++count[n];
      if (parent[n] == n) break;
    }
  }
  if (!o.votes) return o;
  const uint32_t thr = (support_pct * o.votes + 99) / 100;
  for (const auto &kv : count) {
    if (kv.second >= thr && (o.node == kLcaNone || depth[kv.first] > o.depth)) {
      o.node = kv.first;
      o.depth = depth[kv.first];
      o.support = kv.second;
    }
    if (kv.second == o.votes && (o.lca == kLcaNone || depth[kv.first] > depth[o.lca])) o.lca = kv.first;
  }
  return o;
}

static bool Same(const GhostmLcaOut &a, const GhostmLcaOut &b) {
  return a.node == b.node && a.depth == b.depth && a.votes == b.votes && a.support == b.support && a.lca == b.lca &&
         a.candidates == b.candidates && a.unmapped == b.unmapped && a.best_score == b.best_score;
}

int main() {
  std::vector<uint32_t> depth;
  // the depths and their refusals
  {
    const std::vector<uint32_t> par{0, 0, 1, 1, 2, 2, 3, 0, 7, 8};
    CHECK(TaxonomyDepths(10, par.data(), &depth).empty());
    CHECK((depth == std::vector<uint32_t>{0, 1, 2, 2, 3, 3, 3, 1, 2, 3}));
    const std::vector<uint32_t> two{0, 1, 0}, none{1, 0}, cyc{0, 2, 3, 1, 0}, far{0, 0, 3};
    CHECK(Has(TaxonomyDepths(3, two.data(), &depth), "taxonomy: node 1: a second root"));
    CHECK(Has(TaxonomyDepths(2, none.data(), &depth), "taxonomy: no root"));
    CHECK(Has(TaxonomyDepths(5, cyc.data(), &depth), "taxonomy: node 1: a cycle"));
    CHECK(Has(TaxonomyDepths(3, far.data(), &depth), "taxonomy: node 2: parent out of range"));
    CHECK(Has(TaxonomyDepths(0, far.data(), &depth), "taxonomy: 0 nodes"));
    CHECK(Has(TaxonomyDepths(3, nullptr, &depth), "null: "));
    std::vector<uint32_t> chain(257);
    for (uint32_t i = 0; i < 257; ++i) chain[i] = i ? i - 1 : 0;
    CHECK(TaxonomyDepths(256, chain.data(), &depth).empty() && depth[255] == 255);
    CHECK(Has(TaxonomyDepths(257, chain.data(), &depth), "taxonomy: node 256: deeper than 255"));
    // the root last, every parent above its child
    std::vector<uint32_t> rev(100);
    for (uint32_t i = 0; i < 100; ++i) rev[i] = i == 99 ? 99 : i + 1;
    CHECK(TaxonomyDepths(100, rev.data(), &depth).empty() && depth[0] == 99 && depth[99] == 0);
    CHECK(LcaWord(255, (1u << 24) - 1) == 0xFFFFFFFFu && LcaWord(3, 7) == 0x03000007u);
  }
  // the two tests at their limits
  CHECK(LcaPasses(90, 100, 10) && !LcaPasses(89, 100, 10) && LcaPasses(1, 100, 100) && !LcaPasses(99, 100, 0));
  CHECK(LcaPasses(kLcaValueLimit - 1, kLcaValueLimit - 1, 0));
  CHECK(LcaThreshold(3, 67) == 3 && LcaThreshold(3, 66) == 2 && LcaThreshold(100, 51) == 51 && LcaThreshold(1, 51) == 1 &&
        LcaThreshold(16384, 100) == 16384);
  CHECK(LcaPow2(1025) == 2048 && LcaPow2(16384) == 16384 && LcaPow2(1) == 2);
  // random reads on random trees against the paths
  std::mt19937 rng(20261205);
  uint32_t inner = 0, split = 0, trials = 0;
  for (uint32_t t = 0; t < 300; ++t) {
    const uint32_t nn = 1 + rng() % 200;
    std::vector<uint32_t> par(nn), perm(nn), p2(nn);
    for (uint32_t i = 0; i < nn; ++i) par[i] = i ? (uint32_t)(rng() % i > 8 ? i - 1 - rng() % 8 : rng() % i) : 0, perm[i] = i;
    for (uint32_t i = nn; i-- > 1;) std::swap(perm[i], perm[rng() % (i + 1)]);
    for (uint32_t i = 0; i < nn; ++i) p2[perm[i]] = perm[par[i]];
    CHECK(TaxonomyDepths(nn, p2.data(), &depth).empty());
    const std::vector<uint32_t> tax = TaxonomyWords(nn, p2.data(), depth);
    const uint32_t n = rng() % 40;
    std::vector<GhostmLcaHit> hit(n);
    for (GhostmLcaHit &h : hit) {
      h.node = rng() % 10 == 0 ? kLcaNone : (rng() % 3 ? (uint32_t)(rng() % nn) : perm[nn - 1]);
      h.score = rng() % 8 == 0 ? 0 : 50 + rng() % 20;
      h.q_lo = rng() % 100;
      h.q_hi = h.q_lo + rng() % 60;
    }
    static const uint32_t kTops[4] = {0, 10, 30, 100};
    const uint32_t top = kTops[rng() % 4], sup = 51 + rng() % 50;
    std::vector<uint32_t> ncand;
    const uint32_t rb[2] = {0, n};
    CHECK(ValidateReadLca(nn, 1, rb, n, hit.data(), top, sup, &ncand).empty());
    const GhostmLcaOut got = LcaRead(tax.data(), hit.data(), n, top, sup), want = ByPaths(p2, depth, hit, top, sup);
    CHECK(Same(got, want));
    CHECK(ncand[0] == want.candidates);
    inner += want.votes && want.node != want.lca;
    split += want.votes > 1;
    ++trials;
  }
  CHECK(inner > 20 && split > 200);
  // the checks
  {
    const std::vector<GhostmLcaHit> h{{4, 50, 0, 99}, {9, 40, 10, 20}, {kLcaNone, 30, 100, 120}};
    const uint32_t rb[3] = {0, 2, 3}, back[3] = {0, 3, 2}, past[3] = {0, 2, 4};
    std::vector<uint32_t> nc;
    CHECK(ValidateReadLca(10, 2, rb, 3, h.data(), 10, 100, &nc).empty() && nc[0] == 2 && nc[1] == 1);
    CHECK(Has(ValidateReadLca(0, 2, rb, 3, h.data(), 10, 100, nullptr), "taxonomy: "));
    CHECK(Has(ValidateReadLca(10, 2, back, 3, h.data(), 10, 100, nullptr), "reads: "));
    CHECK(Has(ValidateReadLca(10, 2, past, 3, h.data(), 10, 100, nullptr), "reads: "));
    CHECK(Has(ValidateReadLca(10, 2, rb, 3, h.data(), 101, 100, nullptr), "param: "));
    CHECK(Has(ValidateReadLca(10, 2, rb, 3, h.data(), 10, 50, nullptr), "param: "));
    CHECK(Has(ValidateReadLca(10, 2, nullptr, 3, h.data(), 10, 100, nullptr), "null: "));
    CHECK(Has(ValidateReadLca(10, 2, rb, 3, nullptr, 10, 100, nullptr), "null: "));
    CHECK(Has(ValidateReadLca(9, 2, rb, 3, h.data(), 10, 100, nullptr), "node: hit 1"));
    std::vector<GhostmLcaHit> g = h;
    g[1].q_lo = 21;
    CHECK(Has(ValidateReadLca(10, 2, rb, 3, g.data(), 10, 100, nullptr), "range: hit 1"));
    g = h;
    g[2].q_hi = kLcaValueLimit;
    CHECK(Has(ValidateReadLca(10, 2, rb, 3, g.data(), 10, 100, nullptr), "bounds: hit 2"));
    g = h;
    g[0].score = kLcaValueLimit;
    CHECK(Has(ValidateReadLca(10, 2, rb, 3, g.data(), 10, 100, nullptr), "bounds: hit 0"));
    std::vector<GhostmLcaHit> many(kLcaReadLimit + 1, GhostmLcaHit{kLcaNone, 1, 0, 0});
    const uint32_t all[2] = {0, kLcaReadLimit + 1}, fits[2] = {0, kLcaReadLimit};
    CHECK(Has(ValidateReadLca(10, 1, all, kLcaReadLimit + 1, many.data(), 10, 100, nullptr), "reads: read 0"));
    CHECK(ValidateReadLca(10, 1, fits, kLcaReadLimit + 1, many.data(), 10, 100, nullptr).empty());
    many[5].score = 0;  // a hit that is no candidate does not count
    CHECK(ValidateReadLca(10, 1, all, kLcaReadLimit + 1, many.data(), 10, 100, nullptr).empty());
  }
  // the parsers
  {
    TaxonomyFile f;
    const std::string dmp =
        "1\t|\t1\t|\tno rank\t|\n"
        "\n"
        "2 | 131567 | superkingdom |\n"
        "131567\t1\tno rank\n"
        "   \t\n"
        "1224|2|phylum\r\n"
        "4000000000 1224";
    CHECK(ParseTaxonomyNodes(dmp, &f).empty());
    CHECK((f.taxid == std::vector<uint32_t>{1, 2, 131567, 1224, 4000000000u}));
    CHECK((f.parent == std::vector<uint32_t>{0, 2, 0, 1, 3}));
    CHECK(Has(ParseTaxonomyNodes("1 1\n2 1\n\n2 1\n", &f), "taxonomy: nodes line 4: taxid 2 repeated"));
    CHECK(Has(ParseTaxonomyNodes("1 1\n\n3 2\n", &f), "taxonomy: nodes line 3: parent 2 is not defined"));
    CHECK(Has(ParseTaxonomyNodes("1 1\nx 1\n", &f), "taxonomy: nodes line 2"));
    CHECK(Has(ParseTaxonomyNodes("1 1\n5\n", &f), "taxonomy: nodes line 2"));
    CHECK(Has(ParseTaxonomyNodes("1 1\n0 1\n", &f), "taxonomy: nodes line 2: taxid 0"));
    CHECK(Has(ParseTaxonomyNodes("1 1\n4294967296 1\n", &f), "taxonomy: nodes line 2"));
    CHECK(ParseTaxonomyNodes("", &f).empty() && f.taxid.empty());
    std::vector<std::pair<std::string, uint32_t>> m;
    std::vector<uint32_t> line;
    CHECK(ParseTaxonomyMap("geneA\t7\n\n  geneB   9 extra\ngeneA 8\r\n", &m, &line).empty());
    CHECK(m.size() == 3 && m[0].first == "geneA" && m[0].second == 7 && m[1].first == "geneB" && m[1].second == 9 &&
          m[2].first == "geneA" && m[2].second == 8);
    CHECK((line == std::vector<uint32_t>{1, 3, 4}));
    CHECK(Has(ParseTaxonomyMap("geneA 7\ngeneB\n", &m, &line), "map: line 2"));
    CHECK(Has(ParseTaxonomyMap("geneA seven\n", &m, &line), "map: line 1"));
    CHECK(LcaNameKey("sp|P1|X some protein") == "sp|P1|X" && LcaNameKey("a\tb") == "a" && LcaNameKey("whole") == "whole");
  }
  std::printf("%u trials ok\n", trials);
  return 0;
}
