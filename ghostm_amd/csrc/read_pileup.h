// read_pileup.h — the host arithmetic the read-level pile-up adds to
// ValidateReadRows (read_rows.h) and the plan (pileup_plan.h): the span of
// subject positions a read-level path charges. Plain C++ beside read_rows.h;
// tests/native/test_read_pileup_span.cpp runs it without a device.
//
// A column of op 0, 1 or 3 charges the subject position it stands on. A shift
// column (ops 4 and 5, frame mode) touches no residue and is charged to the
// position the path stands at: s_start + the subject residues of the columns
// before it. So a path may charge one position past its last residue, when
// shift columns stand after it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"

namespace ghostm {

// The charged span of one path whose words ValidateReadRows has accepted:
// positions [s_start, s_start + span) hold every position the path charges;
// 0 when it charges none. *shift_end is set when the last of them is charged
// by a shift alone (it then is s_start + the path's subject residues).
inline uint64_t ReadPileupSpan(const GhostmHitPath &p, const uint32_t *ops, bool *shift_end) {
  uint64_t s = 0, span = 0;
  bool by_shift = false;
  for (uint32_t r = 0; r < p.n_runs; ++r) {
    const uint32_t w = ops[p.ops_offset + r], op = w & 7u;
    const uint64_t len = w >> 4;
    if (op <= 1 || op == 3) {
      s += len;
      span = s;
      by_shift = false;
    } else if (op >= 4 && s + 1 > span) {
      span = s + 1;
      by_shift = true;
    }
  }
  if (shift_end) *shift_end = by_shift;
  return span;
}

// Every hit's span after ValidateReadRows: returns an empty string, or the
// "bounds" reason when a shift column stands at a position >= db_len (the only
// charged position ValidateReadRows' residue check does not cover).
inline std::string ReadPileupSpans(uint32_t db_len, uint32_t nhits, const GhostmHitPath *rec, const uint32_t *ops,
                                   std::vector<uint32_t> *span) {
  span->assign(nhits, 0);
  for (uint32_t h = 0; h < nhits; ++h) {
    const uint64_t n = ReadPileupSpan(rec[h], ops, nullptr);
    if (n && (uint64_t)rec[h].s_start + n > db_len)
      return "bounds: hit " + std::to_string(h) + ": a shift column stands past the DB chunk";
    (*span)[h] = (uint32_t)n;
  }
  return std::string();
}

}  // namespace ghostm
