// band_align_host.cpp — host model of the read-level banded alignment
// (GhostmBandAlignHost, include/ghostm_hip.h): a reverse Gotoh DP over the band
// cells of a whole source (a protein record or one frame of a DNA read, read
// through its tile records) against one subject range, every cell recording the
// term its H took and whether its E and F extended or opened, then the
// three-state walk of traceback_path_host.cpp from the first strict maximum,
// forward in both sequences. The recurrence is run cell by cell, sequentially;
// no device call: this is the model k_band_fill / k_band_walk (kernels.h) are
// checked against.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "band_align.h"

namespace ghostm {
void SetLastErrorMessage(const std::string &m);
}

namespace {

enum Op : uint32_t { kEq = 0, kMis = 1, kIns = 2, kDel = 3 };
constexpr uint8_t kEExt = 4, kFExt = 8;

int Fail(const std::string &m) {
  ghostm::SetLastErrorMessage("GhostmBandAlignHost: " + m);
  return 1;
}

}  // namespace

extern "C" int GhostmBandAlignHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                                   uint32_t db_len, const int score_matrix[], uint32_t nhits,
                                   const GhostmBandSource src[], const int32_t diagonal[], const uint32_t s_lo[],
                                   const uint32_t s_hi[], uint32_t query_sequence_length, uint32_t step,
                                   uint32_t band, int open_gap, int extend_gap, GhostmHitPath rec[], uint32_t ops[],
                                   size_t ops_cap, size_t *ops_used) {
  using namespace ghostm;
  if (!ops_used) return Fail("null: ops_used");
  if (nhits == 0) {
    *ops_used = 0;
    return 0;
  }
  if (!query_seqs || !db || !score_matrix || !src || !diagonal || !s_lo || !s_hi) return Fail("null: an input array");
  if (query_sequence_length != L) return Fail("source: query_sequence_length differs from the records' width");
  const std::string why = ValidateBand(nq, L, db_len, nhits, src, s_lo, s_hi, step, band, open_gap, extend_gap);
  if (!why.empty()) return Fail(why);
  const int B = (int)band, lanes = 2 * B + 1, neg = kBandNegInf;
  std::vector<GhostmHitPath> out(nhits);
  std::vector<uint32_t> words;
  std::vector<uint8_t> dir;
  // lane b of the previous row and of this one; index lanes = the neighbour past lane 2B, no band cell
  std::vector<int> Hp(lanes + 1), Fp(lanes + 1), Hc(lanes + 1), Ec(lanes + 1), Fc(lanes + 1);
  for (uint32_t h = 0; h < nhits; ++h) {
    const GhostmBandSource &S = src[h];
    const int64_t m = S.letters, D = diagonal[h], lo = s_lo[h], hi = s_hi[h];
    dir.assign((size_t)m * lanes, 0);
    std::fill(Hp.begin(), Hp.end(), 0);
    std::fill(Fp.begin(), Fp.end(), neg);
    int best = 0;
    int64_t bi = 0, bj = lo;
    for (int64_t i = m - 1; i >= 0; --i) {
      const uint32_t qc = query_seqs[BandLetterAt(S, (uint32_t)i, L, step)] & 31u;
      Hc[lanes] = 0;
      Ec[lanes] = neg;
      for (int b = lanes - 1; b >= 0; --b) {
        const int64_t j = i + D - B + b;
        if (j < lo || j > hi) {  // no band cell
          Hc[b] = 0;
          Ec[b] = Fc[b] = neg;
          continue;
        }
        const uint32_t dc = db[j] & 31u;
        int cell = 0;
        uint8_t bits = 0;
        const int s = Hp[b] + score_matrix[dc * 32 + qc];
        if (s > 0) { cell = s; bits = 1; }
        const int ee = Ec[b + 1] + extend_gap, eo = Hc[b + 1] + open_gap;
        const int E = std::max(ee, eo);
        if (E > cell) { cell = E; bits = 2; }
        const int fe = (b ? Fp[b - 1] : neg) + extend_gap, fo = (b ? Hp[b - 1] : 0) + open_gap;
        const int F = std::max(fe, fo);
        if (F > cell) { cell = F; bits = 3; }
        dir[(size_t)i * lanes + b] = bits | (ee > eo ? kEExt : 0) | (fe > fo ? kFExt : 0);  // a tie opens
        Hc[b] = cell;
        Ec[b] = E;
        Fc[b] = F;
        if (cell > best) {
          best = cell;
          bi = i;
          bj = j;
        }
      }
      std::swap(Hp, Hc);
      std::swap(Fp, Fc);
    }
    // the walk: H, E or F state at (i, j); it stops at hsel 0 and where it leaves the band cells
    const size_t first = words.size();
    int64_t i = bi, j = bj;
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
      while (i < m && j <= hi) {
        const int64_t b = j - i - D + B;
        if (b < 0 || b >= lanes) break;
        const uint8_t d = dir[(size_t)i * lanes + b];
        if (state == 0) {
          const uint32_t sel = d & 3u;
          if (sel == 0) break;
          if (sel == 1) {
            emit(db[j] == query_seqs[BandLetterAt(S, (uint32_t)i, L, step)] ? kEq : kMis);
            ++i;
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
          ++i;
        }
      }
      if (len) words.push_back(len << 4 | cur);
    }
    GhostmHitPath &r = out[h];
    r.q_start = (uint32_t)bi;
    r.s_start = (uint32_t)bj;
    r.score = (uint32_t)best;
    // an empty path (score 0) starts at row 0 and s_lo and ends there
    r.q_end = best > 0 ? (uint32_t)(i - 1) : (uint32_t)bi;
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
