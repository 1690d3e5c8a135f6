// pileup_host.cpp — host model of the subject pile-up (GhostmPathPileupHost,
// include/ghostm_hip.h). It walks every hit's run-length words column by column
// into a whole-chunk profile and finishes every position from its row. No
// device call: this is the model k_pileup and k_pileup_finish (kernels.h) are
// checked against. The checks are PathRowsGpu's (ValidatePathRows, path_rows.h).
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "path_rows.h"
#include "pileup_plan.h"

namespace ghostm {
void SetLastErrorMessage(const std::string &m);
}

namespace {

int Fail(const std::string &m) {
  ghostm::SetLastErrorMessage("GhostmPathPileupHost: " + m);
  return 1;
}

inline uint32_t Slot(uint8_t c) { return c < 25 ? c : 25; }

}  // namespace

extern "C" int GhostmPathPileupHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                                    uint32_t db_len, const int score_matrix[], uint32_t nhits,
                                    const uint32_t query_ids[], const GhostmHitPath rec[], const uint32_t ops[],
                                    size_t ops_len, uint32_t query_sequence_length, uint32_t depth[],
                                    uint32_t identities[], uint8_t consensus[], uint32_t profile[]) {
  (void)score_matrix;
  constexpr uint32_t S = ghostm::kPileupSlots;
  if (!depth || !identities || !consensus) return Fail("null output array");
  if ((!db && db_len) || (nhits && (!query_seqs || !query_ids || !rec))) return Fail("null argument");
  if (query_sequence_length != L) return Fail("query shape differs from the query set's");
  if (nhits) {
    const std::string why = ghostm::ValidatePathRows(nq, L, db_len, nhits, query_ids, rec, ops, ops_len, nullptr);
    if (!why.empty()) return Fail(why);
  }
  std::vector<uint32_t> own;
  uint32_t *prof = profile;
  if (!prof) {
    own.resize((size_t)db_len * S);
    prof = own.data();
  }
  if (db_len) std::memset(prof, 0, (size_t)db_len * S * 4);
  for (uint32_t h = 0; h < nhits; ++h) {
    const GhostmHitPath &p = rec[h];
    const uint8_t *qs = query_seqs + (size_t)query_ids[h] * L;
    uint32_t q = p.q_start, s = p.s_start;
    for (uint32_t r = 0; r < p.n_runs; ++r) {
      const uint32_t w = ops[p.ops_offset + r], op = w & 3u;
      for (uint32_t k = 0; k < (w >> 4); ++k) {
        if (op < 2) ++prof[(size_t)s++ * S + Slot(qs[q++])];
        else if (op == 2) ++q;
        else ++prof[(size_t)s++ * S + 26];
      }
    }
  }
  for (uint32_t p = 0; p < db_len; ++p) {
    const uint32_t *row = prof + (size_t)p * S;
    uint32_t sum = 0, best = 0, arg = 255;
    for (uint32_t c = 0; c < 27; ++c) {
      sum += row[c];
      if (c < 25 && row[c] > best) best = row[c], arg = c;
    }
    depth[p] = sum;
    identities[p] = row[Slot(db[p])];
    consensus[p] = (uint8_t)arg;
  }
  return 0;
}
