// read_rows_host.cpp — host model of the read-level aligned rows
// (GhostmReadRowsHost, include/ghostm_hip.h) and the checks shared with the
// device call (ValidateReadRows, read_rows.h). The model walks every hit's
// run-length words column by column: the query letter through the source's
// tile records (and, in frame mode, the strand's three frames), the midline and
// the subject letter, the counts and the rescore. No device call: this is the
// model k_read_rows (kernels.h) is checked against.
#include "read_rows.h"

#include <cstring>

namespace ghostm {

void SetLastErrorMessage(const std::string &m);

std::string ValidateReadRows(uint32_t nq, uint32_t W, uint32_t db_len, uint32_t nhits, const GhostmBandSource *src,
                             const GhostmHitPath *rec, const uint32_t *ops, size_t ops_len, uint32_t step, bool frame,
                             int shift, std::vector<uint32_t> *columns) {
  if (columns) columns->assign(nhits, 0);
  if (frame && (shift > 0 || shift < kFrameShiftMin)) return "shift: the frameshift cost must lie in -(1 << 20)..0";
  if (step == 0 || step > W) return "source: tile step outside 1..the record width";
  for (uint32_t h = 0; h < nhits; ++h) {
    const GhostmBandSource &s = src[h];
    const GhostmHitPath &p = rec[h];
    const std::string at = "hit " + std::to_string(h);
    if (s.letters == 0 || s.tiles == 0) return "source: " + at + " has no letters or no tiles";
    if (s.tiles != TileCount(s.letters, W, step)) return "source: " + at + ": tiles disagrees with letters, W and step";
    if (s.tiles > 1 && s.stride == 0) return "source: " + at + ": stride 0";
    const uint64_t last =
        (uint64_t)s.first_record + (frame ? 2 : 0) + (s.tiles > 1 ? (uint64_t)s.stride * (s.tiles - 1) : 0);
    if (last >= nq) return "source: " + at + ": a record outside the resident chunk";
    if (p.ops_offset > ops_len || p.n_runs > ops_len - p.ops_offset || (p.n_runs && !ops))
      return "ops: " + at + ": its runs lie outside ops";
    const int64_t limit = (int64_t)s.letters * (frame ? 3 : 1);
    if (limit > (int64_t)UINT32_MAX) return "bounds: " + at + ": the strand has more than 2^32 - 1 positions";
    int64_t pos = p.q_start;
    uint64_t cols = 0, subject = 0;
    if (p.n_runs && pos >= limit) return "bounds: " + at + ": q_start outside the source";
    for (uint32_t r = 0; r < p.n_runs; ++r) {
      const uint32_t w = ops[p.ops_offset + r], op = w & 7u;
      const int64_t len = w >> 4;
      if ((w & 8u) || len == 0 || op > (frame ? 5u : 3u)) return "word: " + at + ": malformed word " + std::to_string(r);
      const int64_t adv = ReadRowsAdvance(frame, op);
      if (op <= 2 && (pos < 0 || pos + adv * (len - 1) >= limit))
        return "bounds: " + at + ": the query letters of word " + std::to_string(r) + " lie outside the source";
      pos += adv * len;
      cols += (uint64_t)len;
      if (op == 0 || op == 1 || op == 3) subject += (uint64_t)len;
    }
    if (cols > UINT32_MAX) return "bounds: " + at + ": more than 2^32 - 1 columns";
    if (cols && (uint64_t)p.s_start + subject > db_len)
      return "bounds: " + at + ": the subject residues run past the DB chunk";
    if (columns) (*columns)[h] = (uint32_t)cols;
  }
  return std::string();
}

}  // namespace ghostm

namespace {

const char kLetters[] = "ARNDCQEGHILKMFPSTWYVBJZX*";  // formats.cpp's order

inline uint8_t Letter(uint8_t c) { return c < 25 ? (uint8_t)kLetters[c] : (uint8_t)'?'; }

int Fail(const std::string &m) {
  ghostm::SetLastErrorMessage("GhostmReadRowsHost: " + m);
  return 1;
}

}  // namespace

extern "C" int GhostmReadRowsHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                                  uint32_t db_len, const int score_matrix[], uint32_t nhits,
                                  const GhostmBandSource src[], const GhostmHitPath rec[], const uint32_t ops[],
                                  size_t ops_len, uint32_t query_sequence_length, uint32_t step, int frame_mode,
                                  int open_gap, int extend_gap, int shift_cost, GhostmHitReadRows out[],
                                  uint8_t rows[], size_t rows_cap, size_t *rows_used) {
  using namespace ghostm;
  if (nhits == 0) {
    if (rows_used) *rows_used = 0;
    return 0;
  }
  if (!query_seqs || !db || !score_matrix || !src || !rec) return Fail("null: an input array");
  if (query_sequence_length != L) return Fail("source: query shape differs from the query set's");
  const bool frame = frame_mode != 0;
  std::vector<uint32_t> columns;
  const std::string why = ValidateReadRows(nq, L, db_len, nhits, src, rec, ops, ops_len, step, frame, shift_cost, &columns);
  if (!why.empty()) return Fail(why);
  size_t total = 0;
  for (uint32_t h = 0; h < nhits; ++h) total += 3 * (size_t)columns[h];
  if (rows && total > rows_cap) return Fail("rows_cap: the rows do not fit");
  size_t at = 0;
  for (uint32_t h = 0; h < nhits; ++h) {
    const GhostmHitPath &p = rec[h];
    const GhostmBandSource &S = src[h];
    const size_t n = columns[h];
    uint8_t *rq = rows ? rows + at : nullptr;
    uint32_t ident = 0, posit = 0, gaps = 0, shifts = 0, col = 0, s = p.s_start;
    int64_t pos = p.q_start;
    int score = 0;
    // the letter at the position: letter pos of the source, or letter pos / 3 of frame pos % 3
    const auto query_code = [&]() -> uint8_t {
      const uint32_t u = (uint32_t)pos;
      return query_seqs[frame ? SourceLetterAt(S, u % 3, u / 3, L, step) : SourceLetterAt(S, 0, u, L, step)];
    };
    for (uint32_t r = 0; r < p.n_runs; ++r) {
      const uint32_t w = ops[p.ops_offset + r], op = w & 7u;
      for (uint32_t k = 0; k < (w >> 4); ++k, ++col) {
        uint8_t ql = '-', sl = '-', ml = ' ';
        if (op < 2) {
          const uint8_t qc = query_code(), sc = db[s++];
          const int m = score_matrix[(sc & 31) * 32 + (qc & 31)];
          ql = Letter(qc);
          sl = Letter(sc);
          score += m;
          posit += m > 0;
          ident += op == 0;
          if (op == 0) ml = ql;
          else if (m > 0) ml = '+';
        } else if (op < 4) {
          if (op == 2) ql = Letter(query_code());
          else sl = Letter(db[s++]);
          ++gaps;
          score += k == 0 ? open_gap : extend_gap;
        } else {
          ql = op == 4 ? '\\' : '/';
          ++shifts;
          score += shift_cost;
        }
        pos += ReadRowsAdvance(frame, op);
        if (rq) {
          rq[col] = ql;
          rq[n + col] = ml;
          rq[2 * n + col] = sl;
        }
      }
    }
    if (out)
      out[h] = GhostmHitReadRows{ReadRowsFirstRecord(S, p, L, step, frame), (uint32_t)n, ident, posit, gaps, score,
                                 (uint64_t)at, shifts, 0};
    at += 3 * n;
  }
  if (rows_used) *rows_used = total;
  return 0;
}
