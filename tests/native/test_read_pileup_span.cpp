// The span rule of the read-level pile-up (ghostm_amd/csrc/read_pileup.h) and
// the plan it feeds (pileup_plan.h), without a device: a path is given to every
// tile its charged positions meet, a position that only a shift column charges
// included, and to no other. Checked against a column-by-column walk.
// Build: g++ -std=c++17 tests/native/test_read_pileup_span.cpp (the test adds
// -fsanitize=address,undefined in a second run).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "../../ghostm_amd/csrc/pileup_plan.h"
#include "../../ghostm_amd/csrc/read_pileup.h"

using namespace ghostm;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);  \
      std::exit(1);                                               \
    }                                                             \
  } while (0)

static uint32_t W(uint32_t len, uint32_t op) { return len << 4 | op; }

// the positions a path charges, column by column
static std::set<uint64_t> Charged(uint32_t s_start, const std::vector<uint32_t> &words) {
  std::set<uint64_t> out;
  uint64_t s = s_start;
  for (uint32_t w : words)
    for (uint32_t k = 0; k < (w >> 4); ++k) {
      const uint32_t op = w & 7u;
      if (op <= 1 || op == 3) out.insert(s++);
      else if (op >= 4) out.insert(s);
    }
  return out;
}

static GhostmHitPath Path(uint32_t s_start, size_t n_runs) {
  GhostmHitPath p{};
  p.s_start = s_start;
  p.n_runs = (uint32_t)n_runs;
  p.ops_offset = 0;
  return p;
}

// the tiles of the plan that list slot 0
static std::set<uint32_t> PlannedTiles(uint32_t s_start, uint32_t span, uint32_t T, uint32_t ntiles) {
  PileupPlan plan;
  CHECK(BuildPileupPlan(1, [&](uint32_t) { return s_start; }, [&](uint32_t) { return span; }, T, 0, ntiles, 7, &plan));
  std::set<uint32_t> out;
  for (const PileupPart &p : plan.parts) out.insert(p.tile);
  return out;
}

static void CheckPath(uint32_t s_start, const std::vector<uint32_t> &words, uint32_t T, uint32_t db_len) {
  const GhostmHitPath p = Path(s_start, words.size());
  bool by_shift = false;
  const uint64_t span = ReadPileupSpan(p, words.data(), &by_shift);
  const std::set<uint64_t> charged = Charged(s_start, words);
  if (charged.empty()) {
    CHECK(span == 0);
    return;
  }
  CHECK(*charged.begin() >= s_start);
  CHECK(s_start + span == *charged.rbegin() + 1);
  std::set<uint32_t> want;
  for (uint64_t c : charged) want.insert((uint32_t)(c / T));
  // a path's charged positions are consecutive: the tiles between its first and last are all met
  std::vector<uint32_t> spans;
  const std::string why = ReadPileupSpans(db_len, 1, &p, words.data(), &spans);
  if (s_start + span > db_len) {
    CHECK(why.find("bounds") == 0);
    return;
  }
  CHECK(why.empty() && spans[0] == span);
  const std::set<uint32_t> got = PlannedTiles(s_start, (uint32_t)span, T, (db_len + T - 1) / T);
  std::set<uint32_t> full;
  for (uint32_t t = (uint32_t)(s_start / T); t <= (uint32_t)((s_start + span - 1) / T); ++t) full.insert(t);
  CHECK(got == full);
  for (uint32_t t : want) CHECK(got.count(t));
}

int main() {
  const uint32_t T = 32;
  // a trailing shift at a tile edge: residues 20..31, the shift stands at 32 and brings tile 1 into the plan
  {
    const std::vector<uint32_t> words = {W(12, 0), W(1, 4)};
    const GhostmHitPath p = Path(20, words.size());
    bool by_shift = false;
    CHECK(ReadPileupSpan(p, words.data(), &by_shift) == 13 && by_shift);
    CHECK(PlannedTiles(20, 13, T, 4) == (std::set<uint32_t>{0, 1}));
    CHECK(PlannedTiles(20, 12, T, 4) == (std::set<uint32_t>{0}));  // what the residues alone would plan
  }
  // the same shift with a pair behind it adds no position of its own
  {
    const std::vector<uint32_t> words = {W(12, 0), W(1, 5), W(1, 1)};
    const GhostmHitPath p = Path(20, words.size());
    bool by_shift = true;
    CHECK(ReadPileupSpan(p, words.data(), &by_shift) == 13 && !by_shift);
  }
  // shifts and insertions alone: one position; insertions alone: none
  {
    const std::vector<uint32_t> a = {W(3, 4), W(2, 2), W(1, 5)}, b = {W(5, 2)};
    CHECK(ReadPileupSpan(Path(64, a.size()), a.data(), nullptr) == 1);
    CHECK(ReadPileupSpan(Path(64, b.size()), b.data(), nullptr) == 0);
    CHECK(ReadPileupSpan(Path(64, 0), nullptr, nullptr) == 0);
  }
  // a shift standing at db_len is refused, one at db_len - 1 is not
  {
    const std::vector<uint32_t> words = {W(3, 0), W(1, 4)};
    std::vector<uint32_t> spans;
    GhostmHitPath p = Path(97, words.size());
    CHECK(ReadPileupSpans(100, 1, &p, words.data(), &spans).find("bounds") == 0);
    p = Path(96, words.size());
    CHECK(ReadPileupSpans(100, 1, &p, words.data(), &spans).empty() && spans[0] == 4);
  }
  // random paths against the column-by-column walk
  std::mt19937 rng(20261101);
  int trials = 0;
  for (; trials < 4000; ++trials) {
    std::vector<uint32_t> words;
    const int n = (int)(rng() % 8);
    for (int k = 0; k < n; ++k) words.push_back(W(1 + rng() % 40, rng() % 6));
    CheckPath(rng() % 200, words, T, 300);
  }
  std::printf("%d trials ok\n", trials);
  return 0;
}
