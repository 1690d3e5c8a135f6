// read_rows.h — the checks every read-level rows call makes on the host before
// anything is uploaded or launched (ReadRowsGpu, GhostmReadRowsHost, the
// session's read-rows post-passes), so that k_read_rows never receives an index
// it could read out of bounds with, and the source-letter addressing the host
// model uses. Plain C++ beside band_align.h and frame_align.h;
// tests/native/test_read_rows.cpp runs it without a device, and kernels.h
// restates SourceLetterAt for the device.
//
// A path's position runs from q_start: a source letter in band mode, a strand
// position p = 3c + g in frame mode (the contract is above GhostmHitReadRows in
// include/ghostm_hip.h).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "frame_align.h"

namespace ghostm {

// Letter c of frame offset g of a source (band mode: g = 0): the byte's index
// in the chunk's records. FrameLetterAt with the two modes under one name.
inline size_t SourceLetterAt(const GhostmBandSource &s, uint32_t g, uint32_t c, uint32_t W, uint32_t step) {
  return FrameLetterAt(s, g, c, W, step);
}

// How far a column of `op` moves the query position, in the position's units.
inline int64_t ReadRowsAdvance(bool frame, uint32_t op) {
  if (op <= 2) return frame ? 3 : 1;
  if (op == 4) return 1;
  if (op == 5) return -1;
  return 0;
}

// Checks nhits read-level paths against a query chunk of nq records of W
// letters and a DB chunk of db_len residues; rec[i].s_start is absolute in the
// chunk. Returns an empty string and every hit's column count, or the reason
// and its detail:
//   "shift"   frame mode: shift outside -(1 << 20)..0
//   "source"  ValidateBand's / ValidateFrame's source checks
//   "ops"     ops_offset + n_runs > ops_len
//   "word"    a zero length or bit 3 set; an op above 3 (band) or above 5 (frame)
//   "bounds"  a letter column whose position leaves [0, letters) or
//             [0, 3 * letters), or the q_start of a path with words outside
//             it; subject residues past db_len; columns or strand positions
//             past 2^32 - 1
std::string ValidateReadRows(uint32_t nq, uint32_t W, uint32_t db_len, uint32_t nhits, const GhostmBandSource *src,
                             const GhostmHitPath *rec, const uint32_t *ops, size_t ops_len, uint32_t step, bool frame,
                             int shift, std::vector<uint32_t> *columns);

// The record of a path's first query letter, the letter at q_start; a path
// without words: the source's first record.
inline uint32_t ReadRowsFirstRecord(const GhostmBandSource &s, const GhostmHitPath &p, uint32_t W, uint32_t step,
                                    bool frame) {
  if (p.n_runs == 0) return s.first_record;
  const uint32_t c = frame ? p.q_start / 3 : p.q_start, g = frame ? p.q_start % 3 : 0;
  return (uint32_t)(SourceLetterAt(s, g, c, W, step) / W);
}

}  // namespace ghostm
