// The pile-up's host plan (ghostm_amd/csrc/pileup_plan.h) on random spans and
// on the edge cases written out below: every (slot, tile) incidence appears
// exactly once, over the whole chunk and over the windows' plans together; a
// tile's list keeps slot order; parts hold 1..P slots, tile the lists in order;
// windows are whole tiles within the budget, at least one tile each, and tile
// the chunk.
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <utility>
#include <vector>

#include "../../ghostm_amd/csrc/pileup_plan.h"

using namespace ghostm;

#define FAIL(...)        \
  do {                   \
    printf(__VA_ARGS__); \
    printf("\n");        \
    return 1;            \
  } while (0)

struct Span {
  uint32_t start, len;
};

// the incidences a plan must hold, written out the slow way: position by position
static std::multiset<std::pair<uint32_t, uint32_t>> Expected(const std::vector<Span> &sp, uint32_t T, uint32_t t0,
                                                             uint32_t t1) {
  std::set<std::pair<uint32_t, uint32_t>> once;
  for (uint32_t s = 0; s < sp.size(); ++s)
    for (uint64_t p = sp[s].start; p < (uint64_t)sp[s].start + sp[s].len; ++p)
      if (p / T >= t0 && p / T < t1) once.insert({(uint32_t)(p / T), s});
  return std::multiset<std::pair<uint32_t, uint32_t>>(once.begin(), once.end());
}

static int CheckPlan(const std::vector<Span> &sp, uint32_t T, uint32_t t0, uint32_t t1, uint32_t P,
                     std::multiset<std::pair<uint32_t, uint32_t>> *seen) {
  PileupPlan plan;
  if (!BuildPileupPlan((uint32_t)sp.size(), [&](uint32_t s) { return sp[s].start; },
                       [&](uint32_t s) { return sp[s].len; }, T, t0, t1, P, &plan))
    FAIL("plan refused");
  if (plan.tile_first.size() != (size_t)(t1 - t0) + 1 || plan.tile_first[0] != 0 ||
      plan.tile_first.back() != plan.list.size())
    FAIL("CSR shape");
  std::multiset<std::pair<uint32_t, uint32_t>> got;
  for (uint32_t t = 0; t < t1 - t0; ++t) {
    if (plan.tile_first[t] > plan.tile_first[t + 1]) FAIL("CSR not monotone");
    for (uint32_t k = plan.tile_first[t]; k < plan.tile_first[t + 1]; ++k) {
      if (k > plan.tile_first[t] && plan.list[k - 1] >= plan.list[k]) FAIL("tile %u: slot order lost", t0 + t);
      got.insert({t0 + t, plan.list[k]});
    }
  }
  if (got != Expected(sp, T, t0, t1)) FAIL("incidences differ (T %u, tiles [%u, %u))", T, t0, t1);
  // parts: tile order, in list order, 1..P slots, covering every list exactly
  uint32_t at = 0, tile = t0;
  for (const PileupPart &p : plan.parts) {
    if (p.count == 0 || p.count > P) FAIL("part of %u slots (P %u)", p.count, P);
    if (p.tile < tile || p.tile >= t1) FAIL("part tile order");
    tile = p.tile;
    if (p.first != at) FAIL("parts do not tile the list");
    if (p.first < plan.tile_first[p.tile - t0] || p.first + p.count > plan.tile_first[p.tile - t0 + 1])
      FAIL("part crosses its tile's list");
    // a part is full unless it is its tile's last
    if (p.count < P && p.first + p.count != plan.tile_first[p.tile - t0 + 1]) FAIL("short part inside a list");
    at += p.count;
  }
  if (at != plan.list.size()) FAIL("parts cover %u of %zu", at, plan.list.size());
  if (seen) seen->insert(got.begin(), got.end());
  return 0;
}

static int CheckWindows(uint32_t db_len, uint32_t T, size_t budget, std::vector<uint32_t> *out) {
  const std::vector<uint32_t> w = PileupWindows(db_len, T, budget);
  const uint32_t ntiles = (uint32_t)(((uint64_t)db_len + T - 1) / T);
  if (ntiles == 0) {
    if (!w.empty()) FAIL("windows of an empty chunk");
    *out = w;
    return 0;
  }
  if (w.size() < 2 || w.front() != 0 || w.back() != ntiles) FAIL("windows do not span the tiles");
  for (size_t k = 0; k + 1 < w.size(); ++k) {
    if (w[k + 1] <= w[k]) FAIL("empty window");
    const uint64_t bytes = (uint64_t)(w[k + 1] - w[k]) * T * 128;
    if (bytes > budget && w[k + 1] - w[k] > 1) FAIL("window of %llu bytes over %zu", (unsigned long long)bytes, budget);
  }
  *out = w;
  return 0;
}

int main() {
  // the edge cases, T = 32: a span ending on a tile's last position, one starting on a tile's first,
  // one over three tiles, an empty path, one position, the chunk's first and last positions
  {
    const uint32_t T = 32, db_len = 200;
    const std::vector<Span> sp = {{20, 12}, {32, 5}, {30, 40}, {50, 0}, {63, 1}, {64, 1}, {0, 1}, {199, 1}, {31, 2}};
    PileupPlan plan;
    BuildPileupPlan((uint32_t)sp.size(), [&](uint32_t s) { return sp[s].start; },
                    [&](uint32_t s) { return sp[s].len; }, T, 0, 7, 2, &plan);
    const std::vector<std::vector<uint32_t>> want = {{0, 2, 6, 8}, {1, 2, 4, 8}, {2, 5}, {}, {}, {}, {7}};
    for (uint32_t t = 0; t < 7; ++t) {
      const std::vector<uint32_t> got(plan.list.begin() + plan.tile_first[t], plan.list.begin() + plan.tile_first[t + 1]);
      if (got != want[t]) FAIL("edge cases: tile %u", t);
    }
    if (plan.parts.size() != 2 + 2 + 1 + 1) FAIL("edge cases: %zu parts", plan.parts.size());
    if (CheckPlan(sp, T, 0, 7, 2, nullptr)) return 1;
    if (CheckPlan(sp, T, 1, 2, 1, nullptr)) return 1;
    std::vector<uint32_t> w;
    if (CheckWindows(db_len, T, 2 * T * 128, &w)) return 1;
    if (w != std::vector<uint32_t>({0, 2, 4, 6, 7})) FAIL("edge cases: windows");
    if (CheckWindows(db_len, T, 1, &w)) return 1;  // a budget below one tile: one tile per window
    if (w.size() != 8) FAIL("edge cases: one tile per window");
    if (CheckWindows(0, T, 1 << 20, &w)) return 1;
  }
  // the default budget on a chunk far larger than it: 1 GiB of profile = 2^23 positions
  {
    std::vector<uint32_t> w;
    if (CheckWindows(0xFFFFFFFFu, 256, (size_t)1024 << 20, &w)) return 1;
    if (w.size() != 513 || w[1] != (1u << 23) / 256) FAIL("default windows: %zu", w.size());
  }
  if (PileupClampTile(1) != 32 || PileupClampTile(100) != 100 || PileupClampTile(100000) != kPileupTileMax)
    FAIL("tile clamp");
  std::mt19937 rng(12345);
  int trials = 0;
  for (; trials < 300; ++trials) {
    const uint32_t T = 32 + rng() % 225, db_len = 1 + rng() % 5000, P = 1 + rng() % 9;
    const uint32_t n = rng() % 200;
    std::vector<Span> sp(n);
    for (Span &s : sp) {
      s.start = rng() % db_len;
      const uint32_t kind = rng() % 8;
      s.len = kind == 0 ? 0 : std::min<uint32_t>(db_len - s.start, kind == 1 ? 1 + rng() % (3 * T) : 1 + rng() % 130);
      if (kind == 2) s.start -= s.start % T;                                         // starts on a tile's first position
      if (kind == 3 && (s.start + s.len) % T < s.len) s.len -= (s.start + s.len) % T;  // ends on a tile's last
    }
    const uint32_t ntiles = (db_len + T - 1) / T;
    if (CheckPlan(sp, T, 0, ntiles, P, nullptr)) return 1;
    std::vector<uint32_t> w;
    if (CheckWindows(db_len, T, (size_t)(1 + rng() % 6) * T * 128 + rng() % 128, &w)) return 1;
    std::multiset<std::pair<uint32_t, uint32_t>> seen;
    for (size_t k = 0; k + 1 < w.size(); ++k)
      if (CheckPlan(sp, T, w[k], w[k + 1], P, &seen)) return 1;
    if (seen != Expected(sp, T, 0, ntiles)) FAIL("the windows' plans together differ from the chunk's");
  }
  printf("%d trials ok\n", trials);
  return 0;
}
