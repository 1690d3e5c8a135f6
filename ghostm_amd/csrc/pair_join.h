// pair_join.h — the host arithmetic of the mate-pair join (PairJoinGpu,
// GhostmPairJoinHost; the contract is above PairJoinGpu in
// include/ghostm_hip.h): the checks every call makes before anything is
// uploaded or launched, the concordance test, and the join of one pair written
// as k_pair_join (kernels.h) does it: the partner choice per mate-1 hit, then
// the taken marks and the pair's record. Plain C++ beside read_cull.h;
// tests/native/test_pair_join.cpp runs it without a device, and kernels.h
// restates the small functions for the device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"

namespace ghostm {

constexpr uint32_t kPairValueLimit = 1u << 24;  // scores, coordinates, offsets stay below: a sum stays below the LCA's 2^25
constexpr uint32_t kPairHitLimit = 16384;       // hits per pair: the LCA's largest read
constexpr uint32_t kPairWave = 64, kPairCap = 1024;  // the classes' largest pairs, in hits
constexpr uint32_t kPairNone = 0xFFFFFFFFu;

// The span of two hits on one subject.
inline uint32_t PairSpan(const GhostmPairHit &a, const GhostmPairHit &b) {
  return std::max(a.s_hi, b.s_hi) - std::min(a.s_lo, b.s_lo) + 1;
}

// Candidates a of mate 1 and b of mate 2 are concordant.
inline bool PairConcordant(const GhostmPairHit &a, const GhostmPairHit &b, uint32_t max_span, uint32_t orient) {
  return a.subject == b.subject && (orient == 0 || a.strand != b.strand) && PairSpan(a, b) <= max_span;
}

// Why a call is refused, or "" when it is taken. hit may be null when nhits is
// 0; pair_begin and offset when npairs is 0.
inline std::string ValidatePairJoin(uint32_t npairs, const uint32_t *pair_begin, const uint32_t *offset, uint32_t nhits,
                                    const GhostmPairHit *hit, uint32_t max_span, uint32_t orient) {
  if (max_span < 1 || max_span > kPairValueLimit) return "param: max_span outside 1..2^24";
  if (orient > 1) return "param: orient outside 0..1";
  if (npairs > 0x7FFFFFFFu) return "reads: more than 2^31 - 1 pairs";
  if (npairs && !pair_begin) return "null: pair_begin";
  if (npairs && !offset) return "null: offset";
  if (nhits && !hit) return "null: the hits";
  for (uint32_t p = 0; p < npairs; ++p) {
    const uint32_t *b = pair_begin + 2 * (size_t)p;
    if (b[0] > b[1] || b[1] > b[2]) return "reads: a mate of pair " + std::to_string(p) + " ends before it begins";
    if (b[2] - b[0] > kPairHitLimit) return "reads: pair " + std::to_string(p) + " has more than 16384 hits";
  }
  if (npairs && pair_begin[2 * (size_t)npairs] > nhits) return "reads: the last pair ends past nhits";
  for (uint32_t i = 0; i < nhits; ++i) {
    const GhostmPairHit &h = hit[i];
    if (h.q_lo > h.q_hi || h.s_lo > h.s_hi) return "range: hit " + std::to_string(i) + ": lo above hi";
    if (h.q_hi >= kPairValueLimit || h.s_hi >= kPairValueLimit || h.score >= kPairValueLimit)
      return "bounds: hit " + std::to_string(i) + ": a score or coordinate at or over 2^24";
    if (h.strand > 1) return "bounds: hit " + std::to_string(i) + ": a strand above 1";
  }
  for (uint32_t p = 0; p < npairs; ++p)
    if (offset[p] >= kPairValueLimit) return "bounds: pair " + std::to_string(p) + ": an offset at or over 2^24";
  return std::string();
}

// The join of one pair: n1 hits of mate 1, then n2 of mate 2; base is the first
// hit's index in the call (partners are indices of the call's hit array). cand
// and partner have n1 + n2 entries.
inline GhostmPairOut PairJoinOne(const GhostmPairHit *hit, uint32_t n1, uint32_t n2, uint32_t base, uint32_t offset,
                                 uint32_t max_span, uint32_t orient, GhostmLcaHit *cand, uint32_t *partner) {
  const uint32_t n = n1 + n2;
  GhostmPairOut o{0, 0, 0, 0};
  std::vector<uint32_t> chooser(n, kPairNone);  // of a mate-2 hit: the lowest mate-1 hit that chose it
  uint32_t span_score = 0;                      // the score best_span belongs to
  // 1. the partner choice
  for (uint32_t i = 0; i < n1; ++i) {
    const GhostmPairHit &h = hit[i];
    cand[i] = GhostmLcaHit{0, 0, 0, 0};
    partner[i] = kPairNone;
    if (!h.score) continue;
    o.mates |= 1u;
    uint32_t best = 0, bj = kPairNone;
    for (uint32_t j = n1; j < n; ++j)
      if (hit[j].score > best && PairConcordant(h, hit[j], max_span, orient)) {
        best = hit[j].score;
        bj = j;
      }
    cand[i] = GhostmLcaHit{h.node, h.score + best, h.q_lo, bj == kPairNone ? h.q_hi : offset + hit[bj].q_hi};
    o.best_score = std::max(o.best_score, cand[i].score);
    if (bj == kPairNone) continue;
    partner[i] = base + bj;
    chooser[bj] = std::min(chooser[bj], i);
    ++o.joined;
    if (cand[i].score > span_score) {  // the first of the highest
      span_score = cand[i].score;
      o.best_span = PairSpan(h, hit[bj]);
    }
  }
  // 2. the taken marks
  for (uint32_t j = n1; j < n; ++j) {
    const GhostmPairHit &h = hit[j];
    cand[j] = GhostmLcaHit{0, 0, 0, 0};
    partner[j] = kPairNone;
    if (!h.score) continue;
    o.mates |= 2u;
    if (chooser[j] != kPairNone) {
      partner[j] = base + chooser[j];
      continue;
    }
    cand[j] = GhostmLcaHit{h.node, h.score, h.q_lo + offset, h.q_hi + offset};
    o.best_score = std::max(o.best_score, h.score);
  }
  return o;
}

}  // namespace ghostm
