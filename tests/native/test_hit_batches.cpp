// The detail passes' host arithmetic (ghostm_amd/csrc/hit_batches.h) on random
// hit arrays: the column counts against both callers' formulas written out
// here, the launch order against std::stable_sort, the batch cuts (they tile
// the slots in order, hold 1..max_hits slots, stay within the budget unless a
// single slot exceeds it, and are maximal), the batch counts the GPU tests pin,
// and every refusal's exact text.
#include <algorithm>
#include <cstdio>
#include <numeric>
#include <random>
#include <string>
#include <vector>

#include "../../ghostm_amd/csrc/hit_batches.h"

#define FAIL(...)        \
  do {                   \
    printf(__VA_ARGS__); \
    printf("\n");        \
    return 1;            \
  } while (0)

// every batch of n slots; 0 when they are as the header promises
static int CheckBatches(const std::vector<size_t> &cost, size_t max_hits, size_t budget, size_t *batches) {
  const uint32_t n = (uint32_t)cost.size();
  *batches = 0;
  for (uint32_t b0 = 0; b0 < n;) {
    size_t bytes = ~(size_t)0;
    const uint32_t b1 = ghostm::CutBatch(b0, n, max_hits, budget, [&](uint32_t s) { return cost[s]; }, &bytes);
    if (b1 <= b0 || b1 > n) FAIL("batch [%u, %u) of %u slots", b0, b1, n);
    if (b1 - b0 > max_hits) FAIL("batch [%u, %u) holds more than %zu", b0, b1, max_hits);
    size_t sum = 0;
    for (uint32_t s = b0; s < b1; ++s) sum += cost[s];
    if (bytes != sum) FAIL("batch [%u, %u): %zu bytes reported, %zu summed", b0, b1, bytes, sum);
    if (sum > budget && b1 - b0 > 1) FAIL("batch [%u, %u) of %zu bytes exceeds %zu", b0, b1, sum, budget);
    if (b1 < n && b1 - b0 < max_hits && sum + cost[b1] <= budget) FAIL("batch [%u, %u) is not maximal", b0, b1);
    ++*batches;
    b0 = b1;
  }
  return 0;
}

static int Refusals() {
  const uint32_t qid[2] = {0, 3}, end[2] = {10, 99}, start[2] = {5, 99};
  struct Case {
    const char *want;
    bool refuse_empty;
    uint32_t nq, L, db_len, base;
    uint32_t qid1, end1, start1;
  };
  const Case cases[] = {
      {"", false, 4, 75, 100, 40, 3, 99, 99},
      {"", false, 4, 127, 100, 0, 3, 99, 99},  // the extended traceback takes an empty window
      {"", true, 4, 1, 100, 32766, 3, 99, 99},
      {"P: query length outside 1..127", false, 4, 0, 100, 40, 3, 99, 99},
      {"P: query length outside 1..127", true, 4, 128, 100, 40, 3, 99, 99},
      {"P: window too wide for F", false, 4, 75, 100, 32768 - 75, 3, 99, 99},
      {"P: empty window", true, 4, 75, 100, 0, 3, 99, 99},
      {"P: hit outside the resident chunk", false, 4, 75, 100, 40, 4, 99, 99},
      {"P: hit outside the resident chunk", true, 4, 75, 100, 40, 3, 100, 99},
      {"P: start after end", false, 4, 75, 100, 40, 3, 98, 99},
  };
  for (const Case &c : cases) {
    const uint32_t q[2] = {qid[0], c.qid1}, e[2] = {end[0], c.end1}, s[2] = {start[0], c.start1};
    const std::string got = ghostm::RefuseHits("P: ", "F", c.refuse_empty, c.nq, c.L, c.db_len, 2, q, e, s, c.base);
    if (got != c.want) FAIL("refusal: got '%s', want '%s'", got.c_str(), c.want);
  }
  // without known starts there is no start to refuse
  if (!ghostm::RefuseHits("P: ", "F", true, 4, 75, 100, 2, qid, end, nullptr, 40).empty()) FAIL("null starts refused");
  // the callers' texts
  const std::string ext = ghostm::RefuseHits("extended traceback: ", "the packed fields", false, 4, 75, 100, 2, qid, end,
                                             start, 40000);
  if (ext != "extended traceback: window too wide for the packed fields") FAIL("got '%s'", ext.c_str());
  const std::string path = ghostm::RefuseHits("path traceback: ", "the run-length words", true, 4, 75, 100, 2, qid, end,
                                              start, 40000);
  if (path != "path traceback: window too wide for the run-length words") FAIL("got '%s'", path.c_str());
  return 0;
}

int main() {
  std::mt19937_64 rng(20240607);
  auto pick = [&](uint64_t lo, uint64_t hi) { return (uint32_t)(lo + rng() % (hi - lo + 1)); };
  int trials = 0;
  for (; trials < 4000; ++trials) {
    const uint32_t n = pick(0, 300), base = pick(1, 200);
    const bool known = trials & 1, clip = trials & 2;
    std::vector<uint32_t> end(n), start(n);
    for (uint32_t k = 0; k < n; ++k) {
      end[k] = pick(0, 2) ? pick(0, 3 * base) : pick(0, base - 1);  // below and above the window
      start[k] = pick(0, 3) ? end[k] - std::min(end[k], pick(0, base + 20)) : end[k];
    }
    std::vector<uint32_t> ncols(7, 99), order(3, 99);  // stale contents are replaced
    ghostm::ColumnOrder(n, end.data(), known ? start.data() : nullptr, base, clip, &ncols, &order);
    if (ncols.size() != n || order.size() != n) FAIL("trial %d: sizes", trials);
    for (uint32_t k = 0; k < n; ++k) {
      uint32_t want;
      if (clip) {  // the path traceback's
        want = end[k] < base ? end[k] + 1 : base;
        if (known) want = std::min(want, end[k] - start[k] + 1);
      } else {  // the extended traceback's (it sorts only with known starts)
        want = known ? std::min(end[k] - start[k] + 1, base) : base;
      }
      if (ncols[k] != want) FAIL("trial %d: ncols[%u] = %u, want %u", trials, k, ncols[k], want);
    }
    std::vector<uint32_t> want(n);
    std::iota(want.begin(), want.end(), 0u);
    std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) { return ncols[a] < ncols[b]; });
    if (order != want) FAIL("trial %d: the order is not the stable sort by ncols", trials);  // so a permutation too

    // the path traceback's cost (direction bytes over the sorted order) and the rows' (3 bytes a column)
    const size_t colw = pick(1, 16);
    std::vector<size_t> cost(n);
    size_t largest = 0, smallest = ~(size_t)0, total = 0;
    for (uint32_t s = 0; s < n; ++s) {
      cost[s] = trials & 4 ? (size_t)ncols[order[s]] * colw * 4 : 3 * (size_t)ncols[s];
      largest = std::max(largest, cost[s]);
      smallest = std::min(smallest, cost[s]);
      total += cost[s];
    }
    const size_t budgets[] = {0, n ? smallest - (smallest > 0) : 0, largest, (size_t)pick(0, 2 * largest + 1),
                              (size_t)pick(0, total + 1), ~(size_t)0};
    const size_t caps[] = {1, 7, 50, (size_t)pick(1, 400), ~(size_t)0};
    for (size_t budget : budgets)
      for (size_t cap : caps) {
        size_t batches = 0;
        if (CheckBatches(cost, cap, budget, &batches)) FAIL("  (trial %d, budget %zu, cap %zu)", trials, budget, cap);
        if (budget == ~(size_t)0 && cap != ~(size_t)0 && batches != (n + cap - 1) / cap)
          FAIL("trial %d: %u hits, cap %zu: %zu batches", trials, n, cap, batches);
        if ((cap == 1 || budget < smallest) && batches != n) FAIL("trial %d: not one hit a batch", trials);
      }
  }
  // the GPU tests' fixed case: 60 hits, at most 7 a batch, the default budget
  size_t batches = 0;
  if (CheckBatches(std::vector<size_t>(60, 3 * 80), 7, (size_t)1024 << 20, &batches) || batches != 9)
    FAIL("60 hits with 7 a batch: %zu batches", batches);
  if (Refusals()) return 1;
  printf("%d trials ok\n", trials);
  return 0;
}
