// query_mask.h — host arithmetic of the low-complexity mask of a query set
// (GhostmMaskRecordsHost, MaskRecordsGpu, DeviceModule::MaskQuery, the session's
// SetMask): the rule's table and thresholds, the checks every call makes before
// anything is uploaded or launched, and the flag words a source's windows take.
// Plain C++, so tests/native/test_query_mask.cpp runs it without a device;
// query_mask.hip restates the tile addressing for the device.
//
// The rule (include/ghostm_hip.h, above GhostmMaskRecordsHost): the raw segments
// of SEG's first stage in integer arithmetic. Window i covers letters [i, i + w)
// of a source; it is evaluated when all its codes are below kBaseX, and then
//   S = sum over the letters a of T[count_a],  d = 100 * (T[w] - S)
//   low:     d <= extend  * 1024 * w
//   trigger: d <= trigger * 1024 * w
// A maximal run of low windows i..j that holds a trigger masks letters
// [i, j + w).
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "band_align.h"
#include "common.h"

namespace ghostm {

constexpr uint32_t kMaskWindowMin = 6, kMaskWindowMax = 32;
constexpr uint32_t kMaskLevelMax = 500;  // hundredths of a bit: log2(32) = 5 bits

struct MaskParams {
  uint32_t window = 0, trigger = 0, extend = 0;  // window 0: masking is off
};

// T[c] = lround(1024 * c * log2(c)), T[0] = 0, for c up to the largest window
struct MaskTable {
  uint32_t T[kMaskWindowMax + 1];
};
inline MaskTable MakeMaskTable() {
  MaskTable t;
  t.T[0] = 0;
  for (uint32_t c = 1; c <= kMaskWindowMax; ++c) t.T[c] = (uint32_t)std::lround(1024.0 * c * std::log2((double)c));
  return t;
}

// "window" / "levels", each followed by the detail, or ""
inline std::string ValidateMaskParams(uint32_t window, uint32_t trigger, uint32_t extend) {
  if (window < kMaskWindowMin || window > kMaskWindowMax)
    return "window: " + std::to_string(window) + " outside 6..32";
  if (!(trigger <= extend && extend <= kMaskLevelMax))
    return "levels: 0 <= trigger <= extend <= 500 is required";
  return std::string();
}

// Why a call is refused ("window", "levels", "source", "overlap", each followed
// by the detail), or "". nq, W: the records. The source conditions are the
// band pass's (ValidateBand).
inline std::string ValidateMask(uint32_t nq, uint32_t W, uint32_t nsrc, const GhostmBandSource *src, uint32_t step,
                                uint32_t window, uint32_t trigger, uint32_t extend) {
  std::string why = ValidateMaskParams(window, trigger, extend);
  if (!why.empty()) return why;
  if (W == 0) return "source: a record width of 0";
  if (step == 0 || step > W) return "source: tile step outside 1..the record width";
  std::vector<uint8_t> taken(nq, 0);
  for (uint32_t h = 0; h < nsrc; ++h) {
    const GhostmBandSource &s = src[h];
    const std::string at = "source " + std::to_string(h);
    if (s.letters == 0 || s.tiles == 0) return "source: " + at + " has no letters or no tiles";
    if (s.tiles != TileCount(s.letters, W, step)) return "source: " + at + ": tiles disagrees with letters, W and step";
    if (s.tiles > 1 && s.stride == 0) return "source: " + at + ": stride 0";
    const uint64_t last = (uint64_t)s.first_record + (s.tiles > 1 ? (uint64_t)s.stride * (s.tiles - 1) : 0);
    if (last >= nq) return "source: " + at + ": a record outside the records given";
    for (uint32_t t = 0; t < s.tiles; ++t) {
      uint8_t &seen = taken[s.first_record + (s.tiles > 1 ? s.stride * t : 0)];
      if (seen) return "overlap: " + at + " shares a record with an earlier source";
      seen = 1;
    }
  }
  return std::string();
}

// The flag words of the sources' windows: source h has windows(h) = letters -
// w + 1 windows (0 when letters < w) and takes ceil(windows / 64) words of each
// of the two flag arrays from word_off[h] on.
struct MaskPlan {
  std::vector<uint32_t> word_off;  // nsrc + 1 entries
  uint64_t windows = 0;
  uint64_t sources = 0;  // sources with at least one window
};
inline MaskPlan PlanMask(uint32_t nsrc, const GhostmBandSource *src, uint32_t window) {
  MaskPlan p;
  p.word_off.resize((size_t)nsrc + 1);
  uint32_t at = 0;  // the sources share no record, so their letters are at most 4 G and the words fit
  for (uint32_t h = 0; h < nsrc; ++h) {
    p.word_off[h] = at;
    if (src[h].letters < window) continue;
    const uint32_t nw = src[h].letters - window + 1;
    at += (nw + 63) / 64;
    p.windows += nw;
    ++p.sources;
  }
  p.word_off[nsrc] = at;
  return p;
}

// The two counters of a pass (masked sources, masked source letters) are kept
// in kMaskCounterSlots slots of kMaskCounterWords 64-bit words (a cache line
// each; words 0 and 1 used), a wave adding its sums to the slot of its number:
// one pair of addresses for every masked source's adds serialised them (5 ms
// for 390 K masked sources). The caller adds the slots up.
constexpr uint32_t kMaskCounterSlots = 128, kMaskCounterWords = 16;

// Launches k_mask_windows and k_mask_apply (query_mask.hip) on the caller's
// stream over a resident chunk's records d_seq (nq records of W codes): d_src =
// the nsrc sources, d_word_off = the plan's offsets, d_low / d_trig = the plan's
// words each (need not be cleared), d_masked = nq words and d_counters = the
// counter slots, both zero on entry. The caller has made ValidateMask's checks.
void LaunchQueryMask(void *stream, uint8_t *d_seq, uint32_t W, const GhostmBandSource *d_src,
                     const uint32_t *d_word_off, uint32_t nsrc, uint32_t step, const MaskParams &p,
                     uint64_t *d_low, uint64_t *d_trig, uint32_t *d_masked, uint64_t *d_counters);

}  // namespace ghostm
