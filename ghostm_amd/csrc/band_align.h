// band_align.h — host arithmetic of the read-level banded alignment
// (BandAlignGpu, GhostmBandAlignHost, the session's band post-pass): the checks
// every call makes before anything is uploaded or launched, the rows a hit's
// band runs, and its scratch bytes. Plain C++, so tests/native/test_band_align.cpp
// runs it without a device; kernels.h restates BandLetterAt for the device.
//
// A hit's band cells are (i, j) with 0 <= i < m, s_lo <= j <= s_hi and
// |j - i - D| <= B. Lane b = j - i - D + B in 0..2B owns one diagonal.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/ghostm_hip.h"
#include "query_tiles.h"

namespace ghostm {

constexpr uint32_t kBandMax = 31;          // 2 * 31 + 1 = 63 lanes of a wave
constexpr int kBandNegInf = -(1 << 29);    // E and F of a neighbour that is no band cell

// Why a call is refused ("source", "band", "bounds", "gaps", each followed by
// the detail), or "". nq, W: the resident query chunk; db_len: the DB chunk.
inline std::string ValidateBand(uint32_t nq, uint32_t W, uint32_t db_len, uint32_t nhits, const GhostmBandSource *src,
                                const uint32_t *s_lo, const uint32_t *s_hi, uint32_t step, uint32_t band, int open,
                                int ext) {
  if (band < 1 || band > kBandMax) return "band: half-width outside 1..31";
  if (!(open <= ext && ext <= 0)) return "gaps: open_gap <= extend_gap <= 0 is required";
  if (step == 0 || step > W) return "source: tile step outside 1..the record width";
  for (uint32_t h = 0; h < nhits; ++h) {
    const GhostmBandSource &s = src[h];
    const std::string at = "hit " + std::to_string(h);
    if (s.letters == 0 || s.tiles == 0) return "source: " + at + " has no letters or no tiles";
    if (s.tiles != TileCount(s.letters, W, step)) return "source: " + at + ": tiles disagrees with letters, W and step";
    if (s.tiles > 1 && s.stride == 0) return "source: " + at + ": stride 0";
    const uint64_t last = (uint64_t)s.first_record + (s.tiles > 1 ? (uint64_t)s.stride * (s.tiles - 1) : 0);
    if (last >= nq) return "source: " + at + ": a record outside the resident chunk";
    if (s_lo[h] > s_hi[h] || s_hi[h] >= db_len) return "bounds: " + at + ": subject range outside the resident chunk";
  }
  return std::string();
}

// The rows whose band meets [s_lo, s_hi]: i_top down to i_top - rows + 1; every
// other row holds no band cell. rows may be 0 (the band misses the rectangle).
struct BandRows {
  uint32_t i_top = 0, rows = 0;
};
inline BandRows BandRowRange(uint32_t m, int32_t D, uint32_t B, uint32_t s_lo, uint32_t s_hi) {
  const int64_t top = std::min<int64_t>((int64_t)m - 1, (int64_t)s_hi - D + B);
  const int64_t bot = std::max<int64_t>(0, (int64_t)s_lo - D - B);
  BandRows r;
  if (top >= bot) {
    r.i_top = (uint32_t)top;
    r.rows = (uint32_t)(top - bot + 1);
  }
  return r;
}

// Direction bytes of one row (one byte per lane 0..2B, rounded up to a dword),
// of one hit, and the run-length words its walk can emit at most: every
// operation advances i or j, i over the rows and j over rows + 2B columns.
inline uint32_t BandDirStride(uint32_t B) { return (2 * B + 1 + 3) & ~3u; }
inline size_t BandDirBytes(uint32_t rows, uint32_t B) { return (size_t)rows * BandDirStride(B); }
constexpr size_t BandOpsSlot(uint32_t rows, uint32_t B) { return rows ? 2 * (size_t)rows + 2 * B + 2 : 0; }

// Letter p of a source through the tile table: the record and the byte in it.
inline size_t BandLetterAt(const GhostmBandSource &s, uint32_t p, uint32_t W, uint32_t step) {
  const uint32_t t = std::min(p / step, s.tiles - 1);
  const uint32_t rec = s.first_record + (s.tiles > 1 ? s.stride * t : 0);
  return (size_t)rec * W + (p - TileStart(t, s.tiles, s.letters, W, step));
}

}  // namespace ghostm
