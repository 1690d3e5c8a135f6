// The host arithmetic of a sample's taxon profile
// (ghostm_amd/csrc/taxon_profile.h), without a device: the profile against
// counts over explicit ancestor paths on random trees, the invariants, the
// floor at its limits, the summary, the checks with their reasons, and the
// report text of a hand-written ten-node tree.
// Build: g++ -std=c++17 tests/native/test_taxon_profile.cpp (the test adds
// -fsanitize=address,undefined in a second run).
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <vector>

#include "../../ghostm_amd/csrc/taxon_profile.h"

using namespace ghostm;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static bool Has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

struct ByPaths {
  std::map<uint32_t, uint32_t> direct, clade, kept;
  std::vector<uint32_t> fin;
  uint64_t classified = 0, kept_reads = 0, moved = 0;
};

// the definitions, read by read
static ByPaths Paths(const std::vector<uint32_t> &parent, const std::vector<uint32_t> &node, uint32_t min_reads) {
  ByPaths p;
  for (uint32_t n : node) {
    if (n == kLcaNone) continue;
    ++p.classified;
    ++p.direct[n];
    for (uint32_t a = n;; a = parent[a]) {
      ++p.clade[a];
      if (parent[a] == a) break;
    }
  }
  for (uint32_t n : node) {
    uint32_t f = kLcaNone;
    if (n != kLcaNone)
      for (uint32_t a = n;; a = parent[a]) {
        if (p.clade[a] >= min_reads) {
          f = a;
          break;
        }
        if (parent[a] == a) break;
      }
    p.fin.push_back(f);
    if (f != kLcaNone) {
      ++p.kept[f];
      ++p.kept_reads;
      p.moved += f != n;
    }
  }
  return p;
}

static void Compare(const std::vector<uint32_t> &parent, const std::vector<uint32_t> &node, uint32_t min_reads) {
  std::vector<uint32_t> depth;
  const uint32_t nnodes = (uint32_t)parent.size(), nreads = (uint32_t)node.size();
  CHECK(TaxonomyDepths(nnodes, parent.data(), &depth).empty());
  const std::vector<uint32_t> tax = TaxonomyWords(nnodes, parent.data(), depth);
  std::vector<uint32_t> fin(nreads, 7);
  const std::vector<GhostmTaxonCount> rec =
      TaxonProfileModel(nnodes, tax.data(), nreads, node.data(), min_reads, nreads ? fin.data() : nullptr);
  const ByPaths want = Paths(parent, node, min_reads);
  CHECK(rec.size() == want.clade.size());
  size_t k = 0;
  for (const auto &kv : want.clade) {  // a map walks in ascending node index
    const GhostmTaxonCount &r = rec[k++];
    CHECK(r.node == kv.first && r.clade_reads == kv.second);
    const auto d = want.direct.find(r.node), kp = want.kept.find(r.node);
    CHECK(r.direct_reads == (d == want.direct.end() ? 0u : d->second));
    CHECK(r.kept_reads == (kp == want.kept.end() ? 0u : kp->second));
    CHECK(r.clade_reads >= min_reads || r.kept_reads == 0);
    CHECK(want.clade.at(parent[r.node]) >= r.clade_reads);  // never shrinks towards the root
  }
  CHECK(fin == want.fin);
  const GhostmTaxonSummary s = TaxonSummary(nreads, rec.data(), rec.size(), min_reads);
  CHECK(s.reads == nreads && s.classified == want.classified && s.kept == want.kept_reads && s.moved == want.moved);
  CHECK(s.nodes == rec.size());
  CHECK(s.kept == (s.classified >= min_reads ? s.classified : 0));
  uint64_t nodes_kept = 0;
  for (const GhostmTaxonCount &r : rec) nodes_kept += r.clade_reads >= min_reads;
  CHECK(s.nodes_kept == nodes_kept);
  if (min_reads == 1) CHECK(s.moved == 0 && fin == node);
  if (s.classified) {
    uint32_t root = 0;
    while (parent[root] != root) ++root;
    CHECK(want.clade.at(root) == s.classified);
  }
}

int main() {
  const std::vector<uint32_t> small{0, 0, 1, 1, 2, 2, 3, 0, 7, 8};
  const std::vector<uint32_t> taxid{1, 10, 20, 21, 30, 31, 32, 5, 22, 33};
  const uint32_t N = kLcaNone;
  const std::vector<uint32_t> reads{N, 4, 9, 4, 5, 9, 0, 6, 9, N, 4, 9, 9};
  std::vector<uint32_t> depth;
  CHECK(TaxonomyDepths(10, small.data(), &depth).empty());
  const std::vector<uint32_t> tax = TaxonomyWords(10, small.data(), depth);

  // the hand-written sample: records, summary, report
  {
    std::vector<uint32_t> fin(reads.size());
    const std::vector<GhostmTaxonCount> rec = TaxonProfileModel(10, tax.data(), 13, reads.data(), 2, fin.data());
    const uint32_t want[10][4] = {{0, 11, 1, 1}, {1, 5, 0, 1}, {2, 4, 0, 1}, {3, 1, 0, 0}, {4, 3, 3, 3},
                                  {5, 1, 1, 0},  {6, 1, 1, 0}, {7, 5, 0, 0}, {8, 5, 0, 0}, {9, 5, 5, 5}};
    CHECK(rec.size() == 10);
    for (size_t k = 0; k < 10; ++k)
      CHECK(rec[k].node == want[k][0] && rec[k].clade_reads == want[k][1] && rec[k].direct_reads == want[k][2] &&
            rec[k].kept_reads == want[k][3]);
    CHECK((fin == std::vector<uint32_t>{N, 4, 9, 4, 2, 9, 0, 1, 9, N, 4, 9, 9}));
    const GhostmTaxonSummary s = TaxonSummary(13, rec.data(), rec.size(), 2);
    CHECK(s.reads == 13 && s.classified == 11 && s.kept == 11 && s.moved == 2 && s.nodes == 10 && s.nodes_kept == 7);
    const std::string text = TaxonReport(rec.data(), rec.size(), 2, 13, small.data(), depth.data(), taxid.data());
    const char *expected =
        "15.38\t2\t2\t2\t0\t0\t0\n"     // 2 of 13 unclassified
        "84.62\t11\t1\t1\t0\t1\t1\n"    // 84.615 rounds up; the root prints itself as parent
        "38.46\t5\t0\t0\t1\t5\t1\n"     // the tie of the two families: taxid 5 before taxid 10
        "38.46\t5\t0\t0\t2\t22\t5\n"
        "38.46\t5\t5\t5\t3\t33\t22\n"
        "38.46\t5\t1\t0\t1\t10\t1\n"
        "30.77\t4\t1\t0\t2\t20\t10\n"
        "23.08\t3\t3\t3\t3\t30\t20\n";
    CHECK(text == expected);
    // no reads: no text; a floor above everything: the unclassified line alone
    CHECK(TaxonReport(nullptr, 0, 1, 0, small.data(), depth.data(), taxid.data()).empty());
    const std::vector<GhostmTaxonCount> high = TaxonProfileModel(10, tax.data(), 13, reads.data(), 12, fin.data());
    CHECK(high.size() == 10);
    for (uint32_t f : fin) CHECK(f == N);
    CHECK(TaxonReport(high.data(), high.size(), 12, 13, small.data(), depth.data(), taxid.data()) ==
          "100.00\t13\t13\t13\t0\t0\t0\n");
    // everything classified and kept: no unclassified line
    const std::vector<uint32_t> two{9, 9};
    const std::vector<GhostmTaxonCount> all = TaxonProfileModel(10, tax.data(), 2, two.data(), 1, nullptr);
    CHECK(TaxonReport(all.data(), all.size(), 1, 2, small.data(), depth.data(), taxid.data()) ==
          "100.00\t2\t0\t0\t0\t1\t1\n100.00\t2\t0\t0\t1\t5\t1\n100.00\t2\t0\t0\t2\t22\t5\n100.00\t2\t2\t2\t3\t33\t22\n");
  }

  // the percent: hundredths, half up, in 64 bits
  {
    std::string s;
    TaxonPercent(&s, 1, 3);
    CHECK(s == "33.33");
    s.clear();
    TaxonPercent(&s, 2, 3);
    CHECK(s == "66.67");
    s.clear();
    TaxonPercent(&s, 1, 20000);  // 0.005 per cent rounds up
    CHECK(s == "0.01");
    s.clear();
    TaxonPercent(&s, 4294967295ull, 4294967295ull);  // clade * 10000 needs 64 bits
    CHECK(s == "100.00");
    s.clear();
    TaxonPercent(&s, 1, 4294967295ull);
    CHECK(s == "0.00");
  }

  // the checks
  {
    GhostmTaxonCount out[16];
    size_t nout = 0;
    CHECK(Has(ValidateTaxonProfile(10, 13, reads.data(), 0, 16, out, &nout), "param: "));
    CHECK(Has(ValidateTaxonProfile(10, 13, nullptr, 1, 16, out, &nout), "null: node"));
    CHECK(Has(ValidateTaxonProfile(10, 13, reads.data(), 1, 16, out, nullptr), "null: nout"));
    CHECK(Has(ValidateTaxonProfile(10, 13, reads.data(), 1, 16, nullptr, &nout), "null: out"));
    CHECK(Has(ValidateTaxonProfile(0, 13, reads.data(), 1, 16, out, &nout), "taxonomy: "));
    std::vector<uint32_t> bad = reads;
    bad[5] = 10;
    CHECK(Has(ValidateTaxonProfile(10, 13, bad.data(), 1, 16, out, &nout), "node: read 5:"));
    bad[5] = N - 1;
    CHECK(Has(ValidateTaxonProfile(10, 13, bad.data(), 1, 16, out, &nout), "node: read 5:"));
    CHECK(ValidateTaxonProfile(10, 13, reads.data(), 1, 16, out, &nout).empty());
    CHECK(ValidateTaxonProfile(10, 0, nullptr, 1, 0, nullptr, &nout).empty());
    CHECK(Has(TaxonProfileCap(10, 9, out), "cap: 10 "));
    CHECK(Has(TaxonProfileCap(10, 0, out), "cap: 10 "));
    CHECK(TaxonProfileCap(10, 10, out).empty() && TaxonProfileCap(10, 0, nullptr).empty());
  }

  // random trees (a parent's index on either side of its child's) and samples
  std::mt19937 rng(20270103);
  uint32_t trials = 0;
  for (uint32_t t = 0; t < 60; ++t) {
    const uint32_t nnodes = 1 + rng() % (t < 10 ? 6 : 400);
    std::vector<uint32_t> par(nnodes, 0), perm(nnodes), parent(nnodes);
    for (uint32_t i = 1; i < nnodes; ++i) par[i] = i - 1 - rng() % std::min<uint32_t>(i, 1 + rng() % 40);
    for (uint32_t i = 0; i < nnodes; ++i) perm[i] = i;
    for (uint32_t i = nnodes; i > 1; --i) std::swap(perm[i - 1], perm[rng() % i]);
    for (uint32_t i = 0; i < nnodes; ++i) parent[perm[i]] = perm[par[i]];
    std::vector<uint32_t> d;
    if (!TaxonomyDepths(nnodes, parent.data(), &d).empty()) continue;  // deeper than 255
    for (uint32_t s = 0; s < 6; ++s) {
      const uint32_t nreads = s == 0 ? 0 : rng() % 600;
      std::vector<uint32_t> node(nreads);
      const uint32_t hot = rng() % nnodes;
      for (uint32_t &n : node) {
        const uint32_t x = rng() % 10;
        n = x == 0 ? N : x < 5 ? hot : rng() % nnodes;
      }
      for (uint32_t min_reads : {1u, 2u, 3u, 10u, nreads + 1}) {
        Compare(parent, node, min_reads);
        ++trials;
      }
    }
  }
  CHECK(trials > 1000);
  std::printf("%u trials ok\n", trials);
  return 0;
}
