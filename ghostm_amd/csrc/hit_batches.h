// hit_batches.h — host arithmetic shared by the per-hit detail passes
// (DeviceModule::TraceBackExt, TraceBackPath, PathRows): the hit arrays' checks,
// the column counts with their launch order, and the batch cuts. Plain C++, so
// tests/native/test_hit_batches.cpp runs it without a device.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace ghostm {

// Why a reverse-DP detail pass refuses its hits, with the caller's prefix
// ("path traceback: "), or "" when it takes them. nq, L, db_len: the resident
// chunks; start may be null; base: the DP window. fields names what L + base
// must fit ("the packed fields"); a pass that cannot run an empty window says so.
inline std::string RefuseHits(const std::string &prefix, const char *fields, bool refuse_empty_window, uint32_t nq,
                              uint32_t L, uint32_t db_len, uint32_t n, const uint32_t *qid, const uint32_t *end,
                              const uint32_t *start, uint32_t base) {
  if (L == 0 || L > 127) return prefix + "query length outside 1..127";
  if ((uint64_t)L + base >= 32768) return prefix + "window too wide for " + fields;
  if (refuse_empty_window && base == 0) return prefix + "empty window";
  for (uint32_t k = 0; k < n; ++k) {
    if (qid[k] >= nq || end[k] >= db_len) return prefix + "hit outside the resident chunk";
    if (start && start[k] > end[k]) return prefix + "start after end";
  }
  return std::string();
}

// Every hit's column count and the launch order, a stable counting sort by it:
// hits of about equal column counts share a wave, whose loop runs to the
// widest. A hit's columns are the window (base), cut to the known start's span
// end - start + 1 when start is given; clip_at_zero first clips the window at
// DB position 0 (end + 1 columns): the path traceback sizes its buffers by the
// count.
inline void ColumnOrder(uint32_t n, const uint32_t *end, const uint32_t *start, uint32_t base, bool clip_at_zero,
                        std::vector<uint32_t> *ncols, std::vector<uint32_t> *order) {
  ncols->resize(n);
  order->resize(n);
  std::vector<uint32_t> first((size_t)base + 2, 0);
  for (uint32_t k = 0; k < n; ++k) {
    uint32_t w = clip_at_zero && end[k] < base ? end[k] + 1 : base;
    if (start) w = std::min(w, end[k] - start[k] + 1);
    (*ncols)[k] = w;
    ++first[w + 1];
  }
  for (size_t c = 1; c < first.size(); ++c) first[c] += first[c - 1];
  for (uint32_t k = 0; k < n; ++k) (*order)[first[(*ncols)[k]]++] = k;
}

// The batch [b0, b1) of n slots: at least one slot, then as many as fit budget
// bytes, at most max_hits. cost(s) is slot s's bytes; *bytes receives the
// batch's. Returns b1.
template <class Cost>
inline uint32_t CutBatch(uint32_t b0, uint32_t n, size_t max_hits, size_t budget, Cost cost, size_t *bytes) {
  uint32_t b1 = b0;
  *bytes = 0;
  while (b1 < n && b1 - b0 < max_hits) {
    const size_t sz = cost(b1);
    if (b1 > b0 && *bytes + sz > budget) break;
    *bytes += sz;
    ++b1;
  }
  return b1;
}

}  // namespace ghostm
