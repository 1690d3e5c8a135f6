// The per-read passes' batch plan (ghostm_amd/csrc/read_classes.h) on reads of
// sizes 0, 1, 64, 65, 256, 257, 1024, 1025 and 3000, in that order and under
// seeded shuffles, with the cull's bounds {64, 256, 1024} and the LCA's {64,
// 1024}, with and without the size arrays. The expected words are written out
// here from the layout's description: the read_begin slice, per class the list
// (and the sizes), padding to an even word, the u64 table offsets.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../ghostm_amd/csrc/read_classes.h"

#define FAIL(...)        \
  do {                   \
    printf(__VA_ARGS__); \
    printf("\n");        \
    return 1;            \
  } while (0)

// a table's words by the read's size: 13 arrays of the next power of two, as the cull sizes its own
static size_t TableWords(uint32_t size) {
  size_t p = 1;
  while (p < size) p <<= 1;
  return 13 * p;
}

static int Check(const std::vector<uint32_t> &size, const std::vector<uint32_t> &bound, bool with_sizes, int trial) {
  const uint32_t m = (uint32_t)size.size();
  // a slice that does not begin at 0, every read with at least its size in hits
  std::vector<uint32_t> read_begin(m + 1);
  read_begin[0] = 777;
  for (uint32_t r = 0; r < m; ++r) read_begin[r + 1] = read_begin[r] + size[r] + (r % 3);
  const size_t classes = bound.size() + 1;
  size_t asked = 0;
  ghostm::ReadClassPlan plan;
  plan.meta.assign(5, 0xDEADu);  // stale contents are replaced
  plan.Build(read_begin.data(), m, size.data(), bound.data(), bound.size(), with_sizes, [&](uint32_t r) {
    ++asked;
    return TableWords(size[r]);
  });

  // the class a size belongs to: a size equal to a bound stays in the lower class
  const auto class_of = [&](uint32_t n) {
    size_t c = 0;
    while (c < bound.size() && n > bound[c]) ++c;
    return c;
  };
  std::vector<uint32_t> want(read_begin);
  std::vector<size_t> want_at(classes), want_len(classes);
  size_t launched = 0, global_reads = 0;
  for (size_t c = 0; c < classes; ++c) {
    want_at[c] = want.size();
    for (uint32_t r = 0; r < m; ++r)
      if (size[r] && class_of(size[r]) == c) want.push_back(r);
    want_len[c] = want.size() - want_at[c];
    launched += want_len[c];
    if (with_sizes)
      for (size_t k = 0; k < want_len[c]; ++k) want.push_back(size[want[want_at[c] + k]]);
  }
  if (want.size() % 2) want.push_back(0);
  const size_t want_offs_at = want.size();
  unsigned long long total = 0;
  for (uint32_t r = 0; r < m; ++r)
    if (size[r] > bound.back()) {
      // little-endian host: the low word first, as the device reads the u64
      want.push_back((uint32_t)(total & 0xFFFFFFFFu));
      want.push_back((uint32_t)(total >> 32));
      total += TableWords(size[r]);
      ++global_reads;
    }

  if (plan.list_at.size() != classes || plan.list_len.size() != classes) FAIL("trial %d: class count", trial);
  for (size_t c = 0; c < classes; ++c)
    if (plan.list_at[c] != want_at[c] || plan.list_len[c] != want_len[c])
      FAIL("trial %d: class %zu at %zu + %zu, want %zu + %zu", trial, c, plan.list_at[c], plan.list_len[c], want_at[c],
           want_len[c]);
  if (plan.offs_at != want_offs_at || plan.offs_at % 2) FAIL("trial %d: offsets at word %zu", trial, plan.offs_at);
  if (plan.table_words != total) FAIL("trial %d: %zu table words, want %llu", trial, plan.table_words, total);
  if (plan.launched != launched) FAIL("trial %d: %zu reads launched, want %zu", trial, plan.launched, launched);
  if (asked != global_reads) FAIL("trial %d: %zu tables asked for, %zu global reads", trial, asked, global_reads);
  if (plan.meta != want) {
    for (size_t k = 0; k < std::min(plan.meta.size(), want.size()); ++k)
      if (plan.meta[k] != want[k]) FAIL("trial %d: meta[%zu] = %u, want %u", trial, k, plan.meta[k], want[k]);
    FAIL("trial %d: %zu meta words, want %zu", trial, plan.meta.size(), want.size());
  }

  // the same read from the plan alone, as a kernel indexes it
  if (memcmp(plan.meta.data(), read_begin.data(), (m + 1) * 4)) FAIL("trial %d: meta does not begin with read_begin", trial);
  std::vector<int> seen(m, 0);
  for (size_t c = 0; c < classes; ++c) {
    const uint32_t *list = plan.meta.data() + plan.list_at[c];
    for (size_t k = 0; k < plan.list_len[c]; ++k) {
      const uint32_t r = list[k];
      if (r >= m) FAIL("trial %d: class %zu lists read %u of %u", trial, c, r, m);
      if (k && list[k - 1] >= r) FAIL("trial %d: class %zu is not in read order", trial, c);
      if (size[r] == 0 || class_of(size[r]) != c) FAIL("trial %d: read %u of size %u in class %zu", trial, r, size[r], c);
      if (with_sizes && list[plan.list_len[c] + k] != size[r]) FAIL("trial %d: class %zu entry %zu: size", trial, c, k);
      ++seen[r];
    }
  }
  for (uint32_t r = 0; r < m; ++r)
    if (seen[r] != (size[r] != 0)) FAIL("trial %d: read %u of size %u listed %d times", trial, r, size[r], seen[r]);
  // each table offset: the table words of the global-class reads before it
  const uint32_t *glist = plan.meta.data() + plan.list_at[classes - 1];
  unsigned long long sum = 0;
  for (size_t k = 0; k < plan.list_len[classes - 1]; ++k) {
    unsigned long long off;
    memcpy(&off, plan.meta.data() + plan.offs_at + 2 * k, 8);
    if (off != sum) FAIL("trial %d: table offset %zu = %llu, want %llu", trial, k, off, sum);
    sum += TableWords(size[glist[k]]);
  }
  if (plan.meta.size() != plan.offs_at + 2 * plan.list_len[classes - 1]) FAIL("trial %d: words after the offsets", trial);
  return 0;
}

int main() {
  const std::vector<uint32_t> fixed = {0, 1, 64, 65, 256, 257, 1024, 1025, 3000};
  const std::vector<std::vector<uint32_t>> bounds = {{64, 256, 1024}, {64, 1024}};
  std::mt19937 rng(20261021);
  int trials = 0;
  for (int round = 0; round < 200; ++round) {
    std::vector<uint32_t> size = fixed;
    if (round) std::shuffle(size.begin(), size.end(), rng);
    if (round % 5 == 4) size.insert(size.end(), fixed.begin(), fixed.end());  // every size twice
    for (const std::vector<uint32_t> &b : bounds)
      for (int with_sizes = 0; with_sizes < 2; ++with_sizes, ++trials)
        if (Check(size, b, with_sizes != 0, trials)) return 1;
  }
  // nothing to launch: no read, and reads of size 0 alone
  for (const std::vector<uint32_t> &b : bounds)
    for (int with_sizes = 0; with_sizes < 2; ++with_sizes, trials += 2) {
      if (Check({}, b, with_sizes != 0, trials)) return 1;
      if (Check({0, 0, 0}, b, with_sizes != 0, trials + 1)) return 1;
    }
  // the padding both ways: an odd and an even number of words before the offsets
  if (Check({3000}, bounds[1], false, trials++)) return 1;        // 2 + 1 words: padded
  if (Check({3000, 2000}, bounds[1], false, trials++)) return 1;  // 3 + 2 words: padded
  if (Check({3000}, bounds[1], true, trials++)) return 1;         // 2 + 2 words: none
  printf("%d trials ok\n", trials);
  return 0;
}
