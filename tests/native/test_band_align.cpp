// The band pass's host arithmetic (ghostm_amd/csrc/band_align.h) on random hits:
// the rows run against a brute-force scan of every row for a band cell, the
// letter addressing against the tile plan written out here (every letter of a
// source found in exactly the tile the formula names, inside the record), the
// scratch formulas against a walk of the longest possible path, and every
// refusal's reason.
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../ghostm_amd/csrc/band_align.h"

#define FAIL(...)        \
  do {                   \
    printf(__VA_ARGS__); \
    printf("\n");        \
    return 1;            \
  } while (0)

using namespace ghostm;

static int Rows(std::mt19937 &rng) {
  for (int trial = 0; trial < 20000; ++trial) {
    const uint32_t m = 1 + rng() % 300, B = 1 + rng() % 31;
    const uint32_t s_lo = rng() % 500, s_hi = s_lo + rng() % 400;
    const int32_t D = (int32_t)(rng() % 1400) - 500;
    // brute force: the rows that hold a band cell
    int64_t top = -1, bot = -1, count = 0;
    for (int64_t i = 0; i < m; ++i) {
      bool any = false;
      for (int64_t b = 0; b <= 2 * (int64_t)B && !any; ++b) {
        const int64_t j = i + D - B + b;
        any = j >= s_lo && j <= s_hi;
      }
      if (any) {
        if (bot < 0) bot = i;
        top = i;
        ++count;
      }
    }
    const BandRows r = BandRowRange(m, D, B, s_lo, s_hi);
    if (count == 0) {
      if (r.rows != 0) FAIL("trial %d: %u rows where no row holds a band cell", trial, r.rows);
      continue;
    }
    if (count != top - bot + 1) FAIL("trial %d: the rows with band cells are not contiguous", trial);
    if (r.rows != count || r.i_top != top) FAIL("trial %d: rows %u top %u, want %lld top %lld", trial, r.rows, r.i_top,
                                                (long long)count, (long long)top);
    if (BandDirStride(B) < 2 * B + 1 || BandDirStride(B) % 4 || BandDirStride(B) > 64) FAIL("stride of B %u", B);
    if (BandDirBytes(r.rows, B) != (size_t)r.rows * BandDirStride(B)) FAIL("direction bytes");
    // a path advances i or j with every operation: at most rows + (rows + 2B) of them, plus the last one
    if (BandOpsSlot(r.rows, B) < 2 * (size_t)r.rows + 2 * B + 1) FAIL("word slot of %u rows", r.rows);
  }
  // extremes: the arithmetic is 64-bit
  if (BandRowRange(5, INT32_MIN, 31, 0, UINT32_MAX - 1).rows != 0) FAIL("D = INT32_MIN");
  if (BandRowRange(5, INT32_MAX, 31, 0, 10).rows != 0) FAIL("D = INT32_MAX");
  const BandRows r = BandRowRange(1000, INT32_MAX, 31, 0, UINT32_MAX - 1);
  if (r.rows != 1000 || r.i_top != 999) FAIL("D = INT32_MAX on a long chunk: %u rows", r.rows);
  return 0;
}

static int Letters(std::mt19937 &rng) {
  for (int trial = 0; trial < 3000; ++trial) {
    const uint32_t W = 1 + rng() % 127, step = 1 + rng() % W, m = 1 + rng() % 700;
    const uint32_t stride = rng() % 2 ? 1 : 6, first = rng() % 50;
    const uint32_t tiles = TileCount(m, W, step);
    const GhostmBandSource s{first, stride, tiles, m};
    for (uint32_t p = 0; p < m; ++p) {
      const size_t at = BandLetterAt(s, p, W, step);
      const uint32_t rec = (uint32_t)(at / W), byte = (uint32_t)(at % W);
      if (rec < first || (tiles > 1 && (rec - first) % stride) || (tiles == 1 && rec != first))
        FAIL("trial %d: letter %u in record %u", trial, p, rec);
      const uint32_t t = tiles > 1 ? (rec - first) / stride : 0;
      if (t >= tiles) FAIL("trial %d: letter %u in tile %u of %u", trial, p, t, tiles);
      if (TileStart(t, tiles, m, W, step) + byte != p) FAIL("trial %d: letter %u read as byte %u of tile %u", trial, p, byte, t);
    }
  }
  return 0;
}

static int Refusals() {
  const uint32_t W = 127, step = 64, nq = 10, db_len = 1000;
  const GhostmBandSource good{2, 1, 3, 200};  // 200 letters: tiles at 0, 64 and 73
  const uint32_t lo = 10, hi = 400;
  struct Case {
    const char *want;
    GhostmBandSource s;
    uint32_t lo, hi, step, band;
    int open, ext;
  };
  const Case cases[] = {
      {"", good, lo, hi, step, 31, -11, -1},
      {"", good, lo, hi, step, 1, -1, -1},
      {"", good, lo, hi, step, 31, 0, 0},
      {"", GhostmBandSource{9, 0, 1, 127}, lo, hi, step, 31, -11, -1},  // one tile: the stride is not read
      {"band", good, lo, hi, step, 0, -11, -1},
      {"band", good, lo, hi, step, 32, -11, -1},
      {"gaps", good, lo, hi, step, 31, -1, -2},
      {"gaps", good, lo, hi, step, 31, -11, 1},
      {"source", good, lo, hi, 0, 31, -11, -1},
      {"source", good, lo, hi, 128, 31, -11, -1},
      {"source", GhostmBandSource{2, 1, 0, 200}, lo, hi, step, 31, -11, -1},
      {"source", GhostmBandSource{2, 1, 2, 200}, lo, hi, step, 31, -11, -1},
      {"source", GhostmBandSource{2, 1, 3, 0}, lo, hi, step, 31, -11, -1},
      {"source", GhostmBandSource{2, 0, 3, 200}, lo, hi, step, 31, -11, -1},
      {"source", GhostmBandSource{8, 1, 3, 200}, lo, hi, step, 31, -11, -1},   // its last tile is record 10
      {"source", GhostmBandSource{0, 6, 3, 200}, lo, hi, step, 31, -11, -1},   // ... record 12
      {"source", GhostmBandSource{UINT32_MAX, UINT32_MAX, 3, 200}, lo, hi, step, 31, -11, -1},
      {"bounds", good, 401, 400, step, 31, -11, -1},
      {"bounds", good, lo, 1000, step, 31, -11, -1},
  };
  for (const Case &c : cases) {
    const std::string why = ValidateBand(nq, W, db_len, 1, &c.s, &c.lo, &c.hi, c.step, c.band, c.open, c.ext);
    if (*c.want ? why.rfind(c.want, 0) != 0 : !why.empty()) FAIL("want '%s', got '%s'", c.want, why.c_str());
  }
  return 0;
}

int main() {
  std::mt19937 rng(20261020);
  if (Rows(rng) || Letters(rng) || Refusals()) return 1;
  printf("trials ok\n");
  return 0;
}
