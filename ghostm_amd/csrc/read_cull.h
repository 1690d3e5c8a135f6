// read_cull.h — the host arithmetic of the read-level cull (ReadCullGpu,
// GhostmReadCullHost; the contract is above ReadCullGpu in
// include/ghostm_hip.h): the checks every call makes before anything is
// uploaded or launched, the rank key, the two tests on a hit, and the cull of
// one read on elementary segments, written as k_read_cull (kernels.h) does it
// and not per position. Plain C++ beside read_pileup.h;
// tests/native/test_read_cull.cpp runs it without a device, and kernels.h
// restates the small functions for the device.
//
// Segments: the read's endpoints q_lo and q_hi + 1 of its non-empty hits,
// sorted (equal values stay, they bound segments of length 0). Segment j is
// [ep[j], ep[j + 1]). A hit's range is the segments [lo, hi) with lo =
// lower_bound(q_lo), hi = lower_bound(q_hi + 1); every segment lies inside or
// outside every hit, so one counter per segment holds the coverage of all its
// positions.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"

namespace ghostm {

constexpr uint32_t kCullCoordLimit = 1u << 25;  // coordinates stay below: d * 100 fits 32 bits
constexpr uint32_t kCullReadLimit = 1u << 24;   // hits per read: the table offsets stay in 32 bits
constexpr uint32_t kCullNone = 0xFFFFFFFFu;

// The rank key: ascending keys are score descending, then index ascending.
inline uint64_t CullKey(uint32_t score, uint32_t index) { return ((uint64_t)(~score) << 32) | index; }

// The duplicate test's geometry: same subject, both ranges intersect.
inline bool CullSameAlignment(const GhostmCullHit &a, const GhostmCullHit &b) {
  return a.subject == b.subject && a.q_lo <= b.q_hi && b.q_lo <= a.q_hi && a.s_lo <= b.s_hi && b.s_lo <= a.s_hi;
}

// The cull test: d covered positions of len.
inline bool CullCovered(uint32_t d, uint32_t len, uint32_t cover_pct) { return d * 100u >= cover_pct * len; }

// Why a call is refused, or "" when it is taken. hit may be null when nhits is
// 0, read_begin when nreads is 0.
inline std::string ValidateReadCull(uint32_t nreads, const uint32_t *read_begin, uint32_t nhits,
                                    const GhostmCullHit *hit, uint32_t top_k, uint32_t cover_pct) {
  if (top_k < 1 || top_k > 255) return "param: top_k outside 1..255";
  if (cover_pct < 1 || cover_pct > 100) return "param: cover_pct outside 1..100";
  if (nreads && !read_begin) return "null: read_begin";
  if (nhits && !hit) return "null: the hits";
  for (uint32_t r = 0; r < nreads; ++r) {
    if (read_begin[r] > read_begin[r + 1]) return "reads: read " + std::to_string(r) + " ends before it begins";
    if (read_begin[r + 1] - read_begin[r] > kCullReadLimit)
      return "reads: read " + std::to_string(r) + " has more than 2^24 hits";
  }
  if (nreads && read_begin[nreads] > nhits) return "reads: the last read ends past nhits";
  for (uint32_t i = 0; i < nhits; ++i) {
    const GhostmCullHit &h = hit[i];
    if (h.q_lo > h.q_hi || h.s_lo > h.s_hi) return "range: hit " + std::to_string(i) + ": lo above hi";
    if (h.q_hi >= kCullCoordLimit || h.s_hi >= kCullCoordLimit)
      return "bounds: hit " + std::to_string(i) + ": a coordinate at or over 2^25";
  }
  return std::string();
}

// A read's segment table: the sorted endpoints and one counter per segment.
struct CullSegments {
  std::vector<uint32_t> ep, count;

  // the endpoints of the n hits with a score
  void Build(const GhostmCullHit *hit, uint32_t n) {
    ep.clear();
    for (uint32_t i = 0; i < n; ++i)
      if (hit[i].score) {
        ep.push_back(hit[i].q_lo);
        ep.push_back(hit[i].q_hi + 1);
      }
    std::sort(ep.begin(), ep.end());
    count.assign(ep.size(), 0);
  }
  uint32_t Lower(uint32_t v) const { return (uint32_t)(std::lower_bound(ep.begin(), ep.end(), v) - ep.begin()); }
  // the positions of [q_lo, q_hi] that at least top_k added hits contain
  uint32_t Covered(uint32_t q_lo, uint32_t q_hi, uint32_t top_k) const {
    uint32_t d = 0;
    for (uint32_t j = Lower(q_lo), hi = Lower(q_hi + 1); j < hi; ++j)
      if (count[j] >= top_k) d += ep[j + 1] - ep[j];
    return d;
  }
  void Add(uint32_t q_lo, uint32_t q_hi) {
    for (uint32_t j = Lower(q_lo), hi = Lower(q_hi + 1); j < hi; ++j) ++count[j];
  }
};

// The cull of one read of n hits; base is the first hit's index in the call
// (dup_of is an index of the call's hit array). out has n records.
inline void CullRead(const GhostmCullHit *hit, uint32_t n, uint32_t base, uint32_t top_k, uint32_t cover_pct,
                     GhostmCullOut *out) {
  std::vector<uint64_t> key(n);
  for (uint32_t i = 0; i < n; ++i) key[i] = CullKey(hit[i].score, i);
  std::sort(key.begin(), key.end());
  CullSegments seg;
  seg.Build(hit, n);
  std::vector<uint32_t> kept;
  for (uint32_t r = 0; r < n; ++r) {
    const uint32_t i = (uint32_t)key[r];
    const GhostmCullHit &h = hit[i];
    GhostmCullOut o{r, GHOSTM_CULL_EMPTY, kCullNone, 0};
    if (h.score) {
      uint32_t dup = kCullNone;
      for (uint32_t k : kept)
        if (CullSameAlignment(hit[k], h)) {
          dup = k;
          break;
        }
      if (dup != kCullNone) {
        o.status = GHOSTM_CULL_DUP;
        o.detail = base + dup;
      } else {
        o.detail = seg.Covered(h.q_lo, h.q_hi, top_k);
        if (CullCovered(o.detail, h.q_hi - h.q_lo + 1, cover_pct)) {
          o.status = GHOSTM_CULL_CULLED;
        } else {
          o.status = GHOSTM_CULL_KEPT;
          o.kept_rank = (uint32_t)kept.size();
          kept.push_back(i);
          seg.Add(h.q_lo, h.q_hi);
        }
      }
    }
    out[i] = o;
  }
}

// Table words of a read of n hits in k_read_cull's layout: 13 arrays of P
// words, P the power of two at or above n (at least 2).
inline uint32_t CullPow2(uint32_t n) {
  uint32_t p = 2;
  while (p < n) p <<= 1;
  return p;
}
constexpr uint32_t kCullTableArrays = 13;

}  // namespace ghostm
