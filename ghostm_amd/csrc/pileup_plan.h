// pileup_plan.h — host arithmetic of the subject pile-up (DeviceModule::PathPileup,
// kern::k_pileup): the DB chunk's positions cut into tiles, the tiles into
// windows whose profile fits a byte budget, and per launch the hits of every
// tile as a CSR cut into parts. Plain C++, so tests/native/test_pileup_plan.cpp
// runs it without a device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ghostm {

constexpr uint32_t kPileupSlots = 32;          // dwords of a profile row (27, 28: the read-level pile-up's shifts; 29..31 stay 0)
constexpr uint32_t kPileupTileMin = 32;        // GHOSTM_PILEUP_TILE's range; the upper end is the
constexpr uint32_t kPileupTileMax = 256;       // kernel's LDS histogram (256 x 33 dwords = 33 KB)
// The defaults, from tools/bench_pileup.py --sweep 64,128,256:128,512,2048 on
// one MI355X (profiles/pileup/). T = 256: a
// workgroup's cost is mostly zeroing and flushing its tile, so the time goes
// with the number of parts: cfg4 (10 M hits on 10 M positions) took 10.75 ms at
// T = 256, 15.94 ms at 128 and 30.14 ms at 64. P = 512: cfg4 10.75 ms against
// 10.92 ms at 128 and 10.76 ms at 2048; cfg2 (212 k hits on 375 positions)
// 0.346 ms against 0.303 ms at 128 and 1.10 ms at 2048, where 131 workgroups
// leave half the CUs idle.
constexpr uint32_t kPileupTileDefault = 256;
constexpr uint32_t kPileupPartDefault = 512;

inline uint32_t PileupClampTile(size_t t) {
  return (uint32_t)std::min<size_t>(std::max<size_t>(t, kPileupTileMin), kPileupTileMax);
}

// Windows of whole tiles: window w holds tiles [first[w], first[w + 1]). A
// position costs kPileupSlots * 4 bytes of profile; a window holds as many tiles
// as fit budget_bytes, at least one. db_len = 0 gives no window.
inline std::vector<uint32_t> PileupWindows(uint32_t db_len, uint32_t T, size_t budget_bytes) {
  const uint32_t ntiles = (uint32_t)(((uint64_t)db_len + T - 1) / T);
  const uint64_t per_tile = (uint64_t)T * kPileupSlots * 4;
  const uint32_t step = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(budget_bytes / per_tile, 1), UINT32_MAX);
  std::vector<uint32_t> first;
  for (uint64_t t = 0; t < ntiles; t += step) first.push_back((uint32_t)t);
  first.push_back(ntiles);
  if (ntiles == 0) first.clear();
  return first;
}

// One workgroup's work: count hits of tile `tile`, list[first .. first + count).
struct PileupPart {
  uint32_t tile, first, count;
};

struct PileupPlan {
  std::vector<uint32_t> tile_first;  // CSR over tiles [t0, t1): t1 - t0 + 1 entries into list
  std::vector<uint32_t> list;        // slot numbers, per tile in slot order
  std::vector<PileupPart> parts;     // in tile order, a tile's parts in list order
};

// The plan of n slots against tiles [t0, t1) of T positions: slot s covers the
// subject positions [start(s), start(s) + len(s)) and belongs to every tile of
// the range that span meets (len 0: none), once each. Every tile's list is cut
// into parts of at most P slots. Returns false when the incidences do not fit
// 32 bits.
template <class Start, class Len>
inline bool BuildPileupPlan(uint32_t n, Start start, Len len, uint32_t T, uint32_t t0, uint32_t t1, uint32_t P,
                            PileupPlan *plan) {
  const uint32_t nt = t1 - t0;
  plan->tile_first.assign((size_t)nt + 1, 0);
  plan->list.clear();
  plan->parts.clear();
  if (P == 0) P = 1;
  // a slot's tiles inside the range: [a, b)
  const auto range = [&](uint32_t s, uint32_t *a, uint32_t *b) {
    const uint64_t p0 = start(s), p1 = p0 + len(s);
    if (p1 == p0) return false;
    const uint64_t ta = std::max<uint64_t>(p0 / T, t0), tb = std::min<uint64_t>((p1 - 1) / T + 1, t1);
    if (ta >= tb) return false;
    *a = (uint32_t)ta - t0;
    *b = (uint32_t)tb - t0;
    return true;
  };
  uint64_t total = 0;
  uint32_t a, b;
  for (uint32_t s = 0; s < n; ++s)
    if (range(s, &a, &b)) {
      for (uint32_t t = a; t < b; ++t) ++plan->tile_first[(size_t)t + 1];
      total += b - a;
    }
  if (total > UINT32_MAX) return false;
  for (uint32_t t = 0; t < nt; ++t) plan->tile_first[(size_t)t + 1] += plan->tile_first[t];
  plan->list.resize(total);
  std::vector<uint32_t> at(plan->tile_first.begin(), plan->tile_first.end() - 1);
  for (uint32_t s = 0; s < n; ++s)
    if (range(s, &a, &b))
      for (uint32_t t = a; t < b; ++t) plan->list[at[t]++] = s;
  for (uint32_t t = 0; t < nt; ++t)
    for (uint32_t f = plan->tile_first[t]; f < plan->tile_first[(size_t)t + 1]; f += P)
      plan->parts.push_back(PileupPart{t0 + t, f, std::min(P, plan->tile_first[(size_t)t + 1] - f)});
  return true;
}

}  // namespace ghostm
