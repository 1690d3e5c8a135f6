// read_pileup_host.cpp — host model of the read-level subject pile-up
// (GhostmReadPileupHost, include/ghostm_hip.h). It walks every hit's run-length
// words column by column into a whole-chunk profile, the query letter through
// the hit's source, a shift column charged to the position the path stands at,
// and finishes every position from its row. No device call: this is the model
// k_read_pileup and k_pileup_finish<true> (kernels.h) are checked against. The
// checks are ReadRowsGpu's (ValidateReadRows, read_rows.h) and the shift
// positions' (ReadPileupSpans, read_pileup.h).
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "pileup_plan.h"
#include "read_pileup.h"
#include "read_rows.h"

namespace ghostm {
void SetLastErrorMessage(const std::string &m);
}

namespace {

int Fail(const std::string &m) {
  ghostm::SetLastErrorMessage("GhostmReadPileupHost: " + m);
  return 1;
}

inline uint32_t Slot(uint8_t c) { return c < 25 ? c : 25; }

}  // namespace

extern "C" int GhostmReadPileupHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                                    uint32_t db_len, uint32_t nhits, const GhostmBandSource src[],
                                    const GhostmHitPath rec[], const uint32_t ops[], size_t ops_len,
                                    uint32_t query_sequence_length, uint32_t step, int frame_mode, uint32_t depth[],
                                    uint32_t identities[], uint8_t consensus[], uint32_t shifts[],
                                    uint32_t profile[]) {
  using namespace ghostm;
  constexpr uint32_t S = kPileupSlots;
  const bool frame = frame_mode != 0;
  if (!depth || !identities || !consensus) return Fail("null: an output array");
  if ((!db && db_len) || (nhits && (!query_seqs || !src || !rec))) return Fail("null: an input array");
  if (query_sequence_length != L) return Fail("source: query shape differs from the query set's");
  if (nhits) {
    std::string why = ValidateReadRows(nq, L, db_len, nhits, src, rec, ops, ops_len, step, frame, 0, nullptr);
    std::vector<uint32_t> span;
    if (why.empty()) why = ReadPileupSpans(db_len, nhits, rec, ops, &span);
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
    const GhostmBandSource &B = src[h];
    int64_t pos = p.q_start;
    uint32_t s = p.s_start;
    for (uint32_t r = 0; r < p.n_runs; ++r) {
      const uint32_t w = ops[p.ops_offset + r], op = w & 7u;
      for (uint32_t k = 0; k < (w >> 4); ++k) {
        if (op < 2) {
          // the letter at the position: letter pos of the source, or letter pos / 3 of frame pos % 3
          const uint32_t u = (uint32_t)pos;
          const uint8_t qc =
              query_seqs[frame ? SourceLetterAt(B, u % 3, u / 3, L, step) : SourceLetterAt(B, 0, u, L, step)];
          ++prof[(size_t)s++ * S + Slot(qc)];
        } else if (op == 3) {
          ++prof[(size_t)s++ * S + 26];
        } else if (op >= 4) {
          ++prof[(size_t)s * S + (op == 4 ? 27 : 28)];
        }
        pos += ReadRowsAdvance(frame, op);
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
    if (shifts) shifts[p] = row[27] + row[28];
  }
  return 0;
}
