// frame_align.h — host arithmetic of the frameshift-aware read-level alignment
// (FrameAlignGpu, GhostmFrameAlignHost, the session's frame post-pass), beside
// band_align.h: the checks every call makes before anything is uploaded or
// launched, the rows a hit's band runs, its scratch bytes and the bound on its
// run-length words. Plain C++, so tests/native/test_frame_align.cpp runs it
// without a device; kernels.h restates FrameLetterAt for the device.
//
// A strand source is three frames g = 0, 1, 2 of m letters each. The rows are
// strand positions p = 3c + g, 0 <= p < 3m; a hit's band cells are (p, j) with
// s_lo <= j <= s_hi and |j - p/3 - D| <= B. Lane b = j - p/3 - D + B in 0..2B
// owns one codon diagonal.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/ghostm_hip.h"
#include "band_align.h"

namespace ghostm {

constexpr int kFrameShiftMin = -(1 << 20);  // the cheapest frameshift a call may ask for

// Why a call is refused (ValidateBand's reasons and "shift"), or "". The three
// frames' records are first_record + g + stride * t: the last one is two
// records past what ValidateBand checks.
inline std::string ValidateFrame(uint32_t nq, uint32_t W, uint32_t db_len, uint32_t nhits, const GhostmBandSource *src,
                                 const uint32_t *s_lo, const uint32_t *s_hi, uint32_t step, uint32_t band, int open,
                                 int ext, int shift) {
  if (shift > 0 || shift < kFrameShiftMin) return "shift: the frameshift cost must lie in -(1 << 20)..0";
  const std::string why = ValidateBand(nq, W, db_len, nhits, src, s_lo, s_hi, step, band, open, ext);
  if (!why.empty()) return why;
  for (uint32_t h = 0; h < nhits; ++h) {
    const GhostmBandSource &s = src[h];
    const uint64_t last = (uint64_t)s.first_record + 2 + (s.tiles > 1 ? (uint64_t)s.stride * (s.tiles - 1) : 0);
    if (last >= nq) return "source: hit " + std::to_string(h) + ": a frame's record outside the resident chunk";
  }
  return std::string();
}

// The rows run: the nucleotide rows of the codon rows BandRowRange gives,
// p_top = 3 * c_top + 2 down to 3 * c_bot; every other row holds no band cell.
struct FrameRows {
  uint32_t c_top = 0, codons = 0;  // BandRowRange's i_top and rows
  uint32_t p_top = 0, rows = 0;    // rows = 3 * codons
};
inline FrameRows FrameRowRange(uint32_t m, int32_t D, uint32_t B, uint32_t s_lo, uint32_t s_hi) {
  const BandRows c = BandRowRange(m, D, B, s_lo, s_hi);
  FrameRows r;
  if (c.rows) {
    r.c_top = c.i_top;
    r.codons = c.rows;
    r.p_top = 3 * c.i_top + 2;
    r.rows = 3 * c.rows;
  }
  return r;
}

// Direction bytes of one hit: one byte per lane and row, BandDirStride(B) a row.
inline size_t FrameDirBytes(uint32_t rows, uint32_t B) { return (size_t)rows * BandDirStride(B); }

// The run-length words a hit's walk can emit at most, by counting operations
// (a word holds at least one). Every operation but a shift advances j by 1
// ('=', 'X', 'D') or p by 3 ('I'), and a shift follows a pair:
//   pairs + 'D'  <= the columns the rows' bands cover = codons + 2B
//   shifts       <= pairs
//   'I'          <= codons: an 'I' starts at a band cell, so at one of the
//                   3 * codons rows run, and between the starts of two of them
//                   p has grown by at least the first one's 3 (a pair with its
//                   shift still advances p by 2, a 'D' leaves it)
// so words <= 2 * (codons + 2B) + codons = rows + 4B; the slot adds 4 spare.
constexpr size_t FrameOpsSlot(uint32_t rows, uint32_t B) { return rows ? (size_t)rows + 4 * B + 4 : 0; }

// The scratch bytes of one hit in a batch: its direction bytes and word slot.
inline size_t FrameScratchBytes(uint32_t rows, uint32_t B) { return FrameDirBytes(rows, B) + 4 * FrameOpsSlot(rows, B); }

// Letter c of frame g of a strand source: the record and the byte in it.
inline size_t FrameLetterAt(const GhostmBandSource &s, uint32_t g, uint32_t c, uint32_t W, uint32_t step) {
  return BandLetterAt(s, c, W, step) + (size_t)g * W;
}
// The letter q(p) of strand position p.
inline size_t FrameStrandLetterAt(const GhostmBandSource &s, uint32_t p, uint32_t W, uint32_t step) {
  return FrameLetterAt(s, p % 3, p / 3, W, step);
}

}  // namespace ghostm
