// frame_align_host.cpp — host model of the frameshift-aware read-level alignment
// (GhostmFrameAlignHost, include/ghostm_hip.h): the reverse three-frame Gotoh DP
// over the band cells of one strand of a DNA read (its three frames, read
// through their tile records) against one subject range. Rows are strand
// positions p; a pair column continues in frame at p + 3 or, for the frameshift
// cost, one nucleotide early (p + 2) or late (p + 4). Every cell records the
// term its H took, which of the three continuations its pair took and whether
// its E and F extended or opened; then the walk from the first strict maximum,
// forward in both sequences. The recurrence is run cell by cell, sequentially;
// no device call: this is the model k_band_fill<true> / k_band_walk<true>
// (kernels.h) are checked against.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "frame_align.h"

namespace ghostm {
void SetLastErrorMessage(const std::string &m);
}

namespace {

enum Op : uint32_t { kEq = 0, kMis = 1, kIns = 2, kDel = 3, kLate = 4, kEarly = 5 };
constexpr uint8_t kEExt = 4, kFExt = 8;

int Fail(const std::string &m) {
  ghostm::SetLastErrorMessage("GhostmFrameAlignHost: " + m);
  return 1;
}

}  // namespace

extern "C" int GhostmFrameAlignHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                                    uint32_t db_len, const int score_matrix[], uint32_t nhits,
                                    const GhostmBandSource src[], const int32_t diagonal[], const uint32_t s_lo[],
                                    const uint32_t s_hi[], uint32_t query_sequence_length, uint32_t step,
                                    uint32_t band, int open_gap, int extend_gap, int shift_cost, GhostmHitPath rec[],
                                    uint32_t ops[], size_t ops_cap, size_t *ops_used) {
  using namespace ghostm;
  if (!ops_used) return Fail("null: ops_used");
  if (nhits == 0) {
    *ops_used = 0;
    return 0;
  }
  if (!query_seqs || !db || !score_matrix || !src || !diagonal || !s_lo || !s_hi) return Fail("null: an input array");
  if (query_sequence_length != L) return Fail("source: query_sequence_length differs from the records' width");
  const std::string why =
      ValidateFrame(nq, L, db_len, nhits, src, s_lo, s_hi, step, band, open_gap, extend_gap, shift_cost);
  if (!why.empty()) return Fail(why);
  const int B = (int)band, lanes = 2 * B + 1, neg = kBandNegInf;
  std::vector<GhostmHitPath> out(nhits);
  std::vector<uint32_t> words;
  std::vector<uint8_t> dir;
  // H and F of rows p .. p + 4 by lane, row p in slot p % 5; E of the row being run
  std::vector<int> Hr(5 * lanes), Fr(5 * lanes), Ec(lanes + 1);
  for (uint32_t h = 0; h < nhits; ++h) {
    const GhostmBandSource &S = src[h];
    const int64_t m = S.letters, P = 3 * m, D = diagonal[h], lo = s_lo[h], hi = s_hi[h];
    // the lane of (p, j) if it is a band cell, else -1
    auto lane_of = [&](int64_t p, int64_t j) -> int {
      if (p < 0 || p >= P || j < lo || j > hi) return -1;
      const int64_t b = j - p / 3 - D + B;
      return b < 0 || b >= lanes ? -1 : (int)b;
    };
    auto Hat = [&](int64_t p, int64_t j) {
      const int b = lane_of(p, j);
      return b < 0 ? 0 : Hr[(size_t)(p % 5) * lanes + b];
    };
    auto Fat = [&](int64_t p, int64_t j) {
      const int b = lane_of(p, j);
      return b < 0 ? neg : Fr[(size_t)(p % 5) * lanes + b];
    };
    dir.assign((size_t)P * lanes, 0);
    int best = 0;
    int64_t bp = 0, bj = lo;
    for (int64_t p = P - 1; p >= 0; --p) {
      const uint32_t qc = query_seqs[FrameStrandLetterAt(S, (uint32_t)p, L, step)] & 31u;
      int *Hc = &Hr[(size_t)(p % 5) * lanes], *Fc = &Fr[(size_t)(p % 5) * lanes];
      Ec[lanes] = neg;
      for (int b = lanes - 1; b >= 0; --b) {
        const int64_t j = p / 3 + D - B + b;
        if (j < lo || j > hi) {  // no band cell
          Hc[b] = 0;
          Ec[b] = Fc[b] = neg;
          continue;
        }
        const uint32_t dc = db[j] & 31u;
        int diag = Hat(p + 3, j + 1);
        uint8_t fsel = 0;
        const int d1 = Hat(p + 2, j + 1) + shift_cost, d2 = Hat(p + 4, j + 1) + shift_cost;
        if (d1 > diag) { diag = d1; fsel = 1; }
        if (d2 > diag) { diag = d2; fsel = 2; }
        int cell = 0;
        uint8_t bits = 0;
        const int s = diag + score_matrix[dc * 32 + qc];
        if (s > 0) { cell = s; bits = 1; }
        const bool right = lane_of(p, j + 1) >= 0;  // (p, j + 1): lane b + 1 of this row
        const int ee = (right ? Ec[b + 1] : neg) + extend_gap, eo = (right ? Hc[b + 1] : 0) + open_gap;
        const int E = std::max(ee, eo);
        if (E > cell) { cell = E; bits = 2; }
        const int fe = Fat(p + 3, j) + extend_gap, fo = Hat(p + 3, j) + open_gap;
        const int F = std::max(fe, fo);
        if (F > cell) { cell = F; bits = 3; }
        dir[(size_t)p * lanes + b] =
            bits | (ee > eo ? kEExt : 0) | (fe > fo ? kFExt : 0) | (uint8_t)(fsel << 5);  // a tie opens
        Hc[b] = cell;
        Ec[b] = E;
        Fc[b] = F;
        if (cell > best) {
          best = cell;
          bp = p;
          bj = j;
        }
      }
    }
    // the walk: H, E or F state at (p, j); it stops at hsel 0 and where it leaves the band cells
    const size_t first = words.size();
    int64_t p = bp, j = bj;
    if (best > 0) {
      int state = 0;
      uint32_t cur = kEq, len = 0;
      auto emit = [&](uint32_t op) {
        if (len && op != cur) {
          words.push_back(len << 4 | cur);
          len = 0;
        }
        cur = op;
        ++len;
      };
      for (;;) {
        const int b = lane_of(p, j);
        if (b < 0) break;
        const uint8_t d = dir[(size_t)p * lanes + b];
        if (state == 0) {
          const uint32_t sel = d & 3u;
          if (sel == 0) break;
          if (sel == 1) {
            const uint32_t qc = query_seqs[FrameStrandLetterAt(S, (uint32_t)p, L, step)] & 31u;
            emit((db[j] & 31u) == qc ? kEq : kMis);
            const uint32_t fsel = (d >> 5) & 3u;
            if (fsel == 1) emit(kEarly);
            if (fsel == 2) emit(kLate);
            p += fsel == 1 ? 2 : fsel == 2 ? 4 : 3;
            ++j;
          } else {
            state = sel == 2 ? 1 : 2;
          }
        } else if (state == 1) {
          emit(kDel);
          state = (d & kEExt) ? 1 : 0;
          ++j;
        } else {
          emit(kIns);
          state = (d & kFExt) ? 2 : 0;
          p += 3;
        }
      }
      if (len) words.push_back(len << 4 | cur);
    }
    GhostmHitPath &r = out[h];
    r.q_start = (uint32_t)bp;
    r.s_start = (uint32_t)bj;
    r.score = (uint32_t)best;
    // an empty path (score 0) starts at strand position 0 and s_lo and ends there
    r.q_end = best > 0 ? (uint32_t)(p - 1) : (uint32_t)bp;
    r.s_end = best > 0 ? (uint32_t)(j - 1) : (uint32_t)bj;
    r.n_runs = (uint32_t)(words.size() - first);
    r.ops_offset = first;
  }
  if (ops && words.size() > ops_cap) return Fail("ops_cap: the operations do not fit");
  if (rec) std::copy(out.begin(), out.end(), rec);
  if (ops) std::copy(words.begin(), words.end(), ops);
  *ops_used = words.size();
  return 0;
}
