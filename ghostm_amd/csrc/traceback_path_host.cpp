// traceback_path_host.cpp — host model of the alignment-path traceback
// (GhostmTraceBackPathHost, include/ghostm_hip.h): the reverse DP of
// traceback_ext_host.cpp with every cell recording which term its H took
// (hsel: 0 zero, 1 diagonal, 2 E, 3 F) and whether its E and F extended
// (strictly) or opened, then a three-state walk from the first strict maximum
// towards column 0 and row L-1, which is forward in both sequences. No device
// call: this is the model k_tb_path_fill / k_tb_path_walk (kernels.h) are
// checked against.
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
enum Op : uint32_t { kEq = 0, kMis = 1, kIns = 2, kDel = 3 };
constexpr uint8_t kEExt = 4, kFExt = 8;

int Fail(const std::string &m) {
  ghostm::SetLastErrorMessage("GhostmTraceBackPathHost: " + m);
  return 1;
}

}  // namespace

extern "C" int GhostmTraceBackPathHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                                       uint32_t db_len, const int score_matrix[], uint32_t nhits,
                                       const uint32_t query_ids[], const uint32_t db_ends[],
                                       const uint32_t db_starts_in[], uint32_t base_search_length, int open_gap,
                                       int extend_gap, GhostmHitPath rec[], uint32_t ops[], size_t ops_cap,
                                       size_t *ops_used) {
  if (ops_used) *ops_used = 0;
  if (nhits == 0) return 0;
  if (!query_seqs || !db || !score_matrix || !query_ids || !db_ends || L == 0) return Fail("null argument or zero query length");
  if (L > 127) return Fail("query length outside 1..127");
  if ((uint64_t)L + base_search_length >= 32768) return Fail("window too wide for the run-length words");
  for (uint32_t h = 0; h < nhits; ++h) {
    if (query_ids[h] >= nq || db_ends[h] >= db_len) return Fail("hit " + std::to_string(h) + " outside the query set or DB");
    if (db_starts_in && db_starts_in[h] > db_ends[h]) return Fail("hit " + std::to_string(h) + ": start after end");
  }
  std::vector<int> H(L + 1), E(L + 1);
  std::vector<uint8_t> dir;
  std::vector<uint32_t> runs;
  size_t used = 0;
  for (uint32_t h = 0; h < nhits; ++h) {
    const uint8_t *qs = query_seqs + (size_t)query_ids[h] * L;
    const uint32_t p0 = db_ends[h];
    uint32_t width = p0 < base_search_length ? p0 + 1 : base_search_length;
    if (db_starts_in) width = std::min(width, p0 - db_starts_in[h] + 1);
    std::fill(H.begin(), H.end(), 0);
    std::fill(E.begin(), E.end(), 0);
    dir.assign((size_t)width * L, 0);
    int best = 0;
    uint32_t best_j = 0, best_k = 0;
    for (uint32_t j = 0; j < width; ++j) {
      const uint8_t c = db[p0 - j];
      if (c == kEnd) break;
      const int *row = score_matrix + (size_t)c * 32;
      uint8_t *d = dir.data() + (size_t)j * L;
      int diag = 0, F = 0;
      for (int k = (int)L - 1; k >= 0; --k) {
        int cell = 0;
        uint8_t bits = 0;
        const int s = diag + row[qs[k]];
        if (s > 0) { cell = s; bits = 1; }
        const int ee = E[k] + extend_gap, eo = H[k] + open_gap;
        E[k] = std::max(ee, eo);
        if (E[k] > cell) { cell = E[k]; bits = 2; }
        const int fe = F + extend_gap, fo = H[k + 1] + open_gap;
        F = std::max(fe, fo);
        if (F > cell) { cell = F; bits = 3; }
        d[k] = bits | (ee > eo ? kEExt : 0) | (fe > fo ? kFExt : 0);  // a tie opens
        diag = H[k];
        H[k] = cell;
        if (cell > best) {
          best = cell;
          best_j = j;
          best_k = (uint32_t)k;
        }
      }
    }
    // the walk: H, E or F state at (j, k); every operation consumes a subject
    // residue (j - 1) or a query residue (k + 1) or both
    runs.clear();
    int j = (int)best_j, k = (int)best_k;
    if (best > 0) {
      int state = 0;
      uint32_t cur = kEq, len = 0;
      auto emit = [&](uint32_t op) {
        if (len && op != cur) {
          runs.push_back(len << 4 | cur);
          len = 0;
        }
        cur = op;
        ++len;
      };
      while (j >= 0 && k < (int)L) {
        const uint8_t b = dir[(size_t)j * L + k];
        if (state == 0) {
          const uint32_t sel = b & 3u;
          if (sel == 0) break;
          if (sel == 1) {
            emit(db[p0 - j] == qs[k] ? kEq : kMis);
            --j;
            ++k;
          } else {
            state = sel == 2 ? 1 : 2;
          }
        } else if (state == 1) {
          emit(kDel);
          state = (b & kEExt) ? 1 : 0;
          --j;
        } else {
          emit(kIns);
          state = (b & kFExt) ? 2 : 0;
          ++k;
        }
      }
      if (len) runs.push_back(len << 4 | cur);
    }
    if (rec) {
      GhostmHitPath &r = rec[h];
      r.q_start = best_k;
      r.s_start = p0 - best_j;
      r.score = (uint32_t)best;
      // an empty path (score 0) ends where it starts
      r.q_end = best > 0 ? (uint32_t)(k - 1) : best_k;
      r.s_end = best > 0 ? p0 - (uint32_t)(j + 1) : p0 - best_j;
      r.n_runs = (uint32_t)runs.size();
      r.ops_offset = used;
    }
    if (ops) {
      if (used + runs.size() > ops_cap) return Fail("the operations do not fit ops_cap");
      std::copy(runs.begin(), runs.end(), ops + used);
    }
    used += runs.size();
  }
  if (ops_used) *ops_used = used;
  return 0;
}
