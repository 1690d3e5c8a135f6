// traceback_ext_host.cpp — host restatement of the extended traceback
// (GhostmTraceBackExtHost, include/ghostm_hip.h): the reference TraceBack
// (aligner.cpp:771-949) with every H cell carrying, besides the reference's
// (alignment length, matches), the mismatches, gap opens, the query row the
// path began in and the step that chose the cell. A cell's bookkeeping is taken
// from the H cell it steps from, also for the E and F chains (the reference's
// rule for length and matches). No device call: this is the model
// k_traceback_ext (kernels.h) is checked against.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"

namespace ghostm {
void SetLastErrorMessage(const std::string &m);
}

namespace {

constexpr uint8_t kEnd = 25;  // SEQUENCE_END, common.h:34
enum Op : uint32_t { kNone = 0, kDiag = 1, kIns = 2, kDel = 3 };

struct Cell {
  uint32_t len = 0, match = 0, mism = 0, gapopen = 0, origin = 0, op = kNone;
};

// the cell reached by a gap step (E: op = ins, F: op = del) from H cell p, in row k
Cell GapStep(const Cell &p, uint32_t k, uint32_t op) {
  Cell c = p;
  c.len = p.len + 1;
  c.gapopen = p.gapopen + (p.op != op ? 1 : 0);
  c.origin = p.len == 0 ? k : p.origin;
  c.op = op;
  return c;
}

}  // namespace

extern "C" int GhostmTraceBackExtHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                                      uint32_t db_len, const int score_matrix[], uint32_t nhits,
                                      const uint32_t query_ids[], const uint32_t db_ends[],
                                      uint32_t base_search_length, int open_gap, int extend_gap,
                                      uint32_t db_starts[], uint32_t aln_lens[], uint32_t aln_matches[],
                                      GhostmHitExt ext[]) {
  if (nhits == 0) return 0;
  if (!query_seqs || !db || !score_matrix || !query_ids || !db_ends || L == 0) {
    ghostm::SetLastErrorMessage("GhostmTraceBackExtHost: null argument or zero query length");
    return 1;
  }
  for (uint32_t h = 0; h < nhits; ++h) {
    if (query_ids[h] >= nq || db_ends[h] >= db_len) {
      ghostm::SetLastErrorMessage("GhostmTraceBackExtHost: hit " + std::to_string(h) + " outside the query set or DB");
      return 1;
    }
  }
  std::vector<int> H(L + 1), E(L + 1);
  std::vector<Cell> T(L + 1);
  for (uint32_t h = 0; h < nhits; ++h) {
    const uint8_t *qs = query_seqs + (size_t)query_ids[h] * L;
    const uint32_t p0 = db_ends[h];
    const uint32_t width = p0 < base_search_length ? p0 + 1 : base_search_length;
    std::fill(H.begin(), H.end(), 0);
    std::fill(E.begin(), E.end(), 0);
    std::fill(T.begin(), T.end(), Cell());
    int best = 0;
    uint32_t best_j = 0, best_k = 0;
    Cell best_t;
    for (uint32_t j = 0; j < width; ++j) {
      const uint8_t c = db[p0 - j];
      if (c == kEnd) break;
      const int *row = score_matrix + (size_t)c * 32;
      int diag = 0, F = 0;
      Cell dt;  // the tuple of H(j-1, k+1)
      for (int k = (int)L - 1; k >= 0; --k) {
        int cell = 0;
        Cell t;
        const int s = diag + row[qs[k]];
        if (s > 0) {
          cell = s;
          t = dt;
          t.len = dt.len + 1;
          t.match = dt.match + (c == qs[k] ? 1 : 0);
          t.mism = dt.mism + (c != qs[k] ? 1 : 0);
          t.origin = dt.len == 0 ? (uint32_t)k : dt.origin;
          t.op = kDiag;
        }
        E[k] = std::max(E[k] + extend_gap, H[k] + open_gap);
        if (E[k] > cell) {
          cell = E[k];
          t = GapStep(T[k], (uint32_t)k, kIns);
        }
        F = std::max(F + extend_gap, H[k + 1] + open_gap);
        if (F > cell) {
          cell = F;
          t = GapStep(T[k + 1], (uint32_t)k, kDel);
        }
        diag = H[k];
        H[k] = cell;
        dt = T[k];
        T[k] = t;
        if (cell > best) {
          best = cell;
          best_j = j;
          best_k = (uint32_t)k;
          best_t = t;
        }
      }
    }
    if (db_starts) db_starts[h] = p0 - best_j;
    if (aln_lens) aln_lens[h] = best_t.len;
    if (aln_matches) aln_matches[h] = best_t.match;
    if (ext) ext[h] = GhostmHitExt{best_k, best_t.origin, best_t.mism, best_t.gapopen};
  }
  return 0;
}
