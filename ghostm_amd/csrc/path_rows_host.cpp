// path_rows_host.cpp — host model of the aligned residue rows
// (GhostmPathRowsHost, include/ghostm_hip.h) and the checks shared with the
// device call (ValidatePathRows, path_rows.h). The model walks every hit's
// run-length words column by column: the query letter, the midline and the
// subject letter, the counts and the rescore. No device call: this is the
// model k_path_rows (kernels.h) is checked against.
#include "path_rows.h"

#include <cstring>

#include "../../include/ghostm_hip.h"

namespace ghostm {

void SetLastErrorMessage(const std::string &m);

std::string ValidatePathRows(uint32_t nq, uint32_t L, uint32_t db_len, uint32_t nhits, const uint32_t *query_ids,
                             const GhostmHitPath *rec, const uint32_t *ops, size_t ops_len,
                             std::vector<uint32_t> *columns) {
  if (columns) columns->assign(nhits, 0);
  for (uint32_t h = 0; h < nhits; ++h) {
    const GhostmHitPath &p = rec[h];
    const std::string at = "hit " + std::to_string(h) + ": ";
    if (query_ids[h] >= nq) return at + "query record outside the resident chunk";
    if (p.ops_offset > ops_len || p.n_runs > ops_len - p.ops_offset || (p.n_runs && !ops))
      return at + "its runs lie outside ops";
    uint64_t count[4] = {0, 0, 0, 0};
    for (uint32_t r = 0; r < p.n_runs; ++r) {
      const uint32_t w = ops[p.ops_offset + r];
      if ((w & 12u) || (w >> 4) == 0) return at + "malformed word " + std::to_string(r);
      count[w & 3u] += w >> 4;
    }
    const uint64_t cols = count[0] + count[1] + count[2] + count[3];
    if (cols == 0) continue;
    if (cols > UINT32_MAX) return at + "out of bounds: more than 2^32 - 1 columns";
    if ((uint64_t)p.q_start + count[0] + count[1] + count[2] > L)
      return at + "out of bounds: the query residues run past the record";
    if ((uint64_t)p.s_start + count[0] + count[1] + count[3] > db_len)
      return at + "out of bounds: the subject residues run past the DB chunk";
    if (columns) (*columns)[h] = (uint32_t)cols;
  }
  return std::string();
}

}  // namespace ghostm

namespace {

const char kLetters[] = "ARNDCQEGHILKMFPSTWYVBJZX*";  // formats.cpp's order

inline uint8_t Letter(uint8_t c) { return c < 25 ? (uint8_t)kLetters[c] : (uint8_t)'?'; }

int Fail(const std::string &m) {
  ghostm::SetLastErrorMessage("GhostmPathRowsHost: " + m);
  return 1;
}

}  // namespace

extern "C" int GhostmPathRowsHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                                  uint32_t db_len, const int score_matrix[], uint32_t nhits,
                                  const uint32_t query_ids[], const GhostmHitPath rec[], const uint32_t ops[],
                                  size_t ops_len, uint32_t query_sequence_length, int open_gap, int extend_gap,
                                  GhostmHitRows out[], uint8_t rows[], size_t rows_cap, size_t *rows_used) {
  if (nhits == 0) {
    if (rows_used) *rows_used = 0;
    return 0;
  }
  if (!query_seqs || !db || !score_matrix || !query_ids || !rec) return Fail("null argument");
  if (query_sequence_length != L) return Fail("query shape differs from the query set's");
  std::vector<uint32_t> columns;
  const std::string why = ghostm::ValidatePathRows(nq, L, db_len, nhits, query_ids, rec, ops, ops_len, &columns);
  if (!why.empty()) return Fail(why);
  size_t total = 0;
  for (uint32_t h = 0; h < nhits; ++h) total += 3 * (size_t)columns[h];
  if (rows && total > rows_cap) return Fail("the rows do not fit rows_cap");
  size_t at = 0;
  for (uint32_t h = 0; h < nhits; ++h) {
    const GhostmHitPath &p = rec[h];
    const uint8_t *qs = query_seqs + (size_t)query_ids[h] * L;
    const size_t n = columns[h];
    uint8_t *rq = rows ? rows + at : nullptr;
    uint32_t ident = 0, posit = 0, gaps = 0, col = 0, q = p.q_start, s = p.s_start;
    int score = 0;
    for (uint32_t r = 0; r < p.n_runs; ++r) {
      const uint32_t w = ops[p.ops_offset + r], op = w & 3u;
      for (uint32_t k = 0; k < (w >> 4); ++k, ++col) {
        uint8_t ql = '-', sl = '-', ml = ' ';
        if (op < 2) {
          const uint8_t qc = qs[q++], sc = db[s++];
          const int m = score_matrix[(sc & 31) * 32 + (qc & 31)];
          ql = Letter(qc);
          sl = Letter(sc);
          score += m;
          posit += m > 0;
          ident += op == 0;
          if (op == 0) ml = ql;
          else if (m > 0) ml = '+';
        } else {
          if (op == 2) ql = Letter(qs[q++]);
          else sl = Letter(db[s++]);
          ++gaps;
          score += k == 0 ? open_gap : extend_gap;
        }
        if (rq) {
          rq[col] = ql;
          rq[n + col] = ml;
          rq[2 * n + col] = sl;
        }
      }
    }
    if (out) out[h] = GhostmHitRows{query_ids[h], (uint32_t)n, ident, posit, gaps, score, (uint64_t)at};
    at += 3 * n;
  }
  if (rows_used) *rows_used = total;
  return 0;
}
