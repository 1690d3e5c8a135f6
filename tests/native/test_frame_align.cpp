// The frame pass's host arithmetic (ghostm_amd/csrc/frame_align.h) on random
// hits: the rows run against a brute-force scan of every nucleotide row for a
// band cell, the letter addressing of the three frames against the tile plan
// written out here, the scratch formula, the bound on a slot's words against
// random walks that obey the walk's rules, and the refusals ValidateFrame adds.
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "../../ghostm_amd/csrc/frame_align.h"

#define FAIL(...)        \
  do {                   \
    printf(__VA_ARGS__); \
    printf("\n");        \
    return 1;            \
  } while (0)

using namespace ghostm;

static bool Cell(int64_t p, int64_t j, uint32_t m, int32_t D, uint32_t B, uint32_t s_lo, uint32_t s_hi) {
  if (p < 0 || p >= 3 * (int64_t)m || j < s_lo || j > s_hi) return false;
  const int64_t b = j - p / 3 - D + B;
  return b >= 0 && b <= 2 * (int64_t)B;
}

static int Rows(std::mt19937 &rng) {
  for (int trial = 0; trial < 20000; ++trial) {
    const uint32_t m = 1 + rng() % 300, B = 1 + rng() % 31;
    const uint32_t s_lo = rng() % 500, s_hi = s_lo + rng() % 400;
    const int32_t D = (int32_t)(rng() % 1400) - 500;
    int64_t top = -1, bot = -1, count = 0;
    for (int64_t p = 0; p < 3 * (int64_t)m; ++p) {
      bool any = false;
      for (int64_t b = 0; b <= 2 * (int64_t)B && !any; ++b) any = Cell(p, p / 3 + D - B + b, m, D, B, s_lo, s_hi);
      if (any) {
        if (bot < 0) bot = p;
        top = p;
        ++count;
      }
    }
    const FrameRows r = FrameRowRange(m, D, B, s_lo, s_hi);
    if (count == 0) {
      if (r.rows != 0 || r.codons != 0) FAIL("trial %d: %u rows where no row holds a band cell", trial, r.rows);
      if (FrameOpsSlot(r.rows, B) != 0 || FrameScratchBytes(r.rows, B) != 0) FAIL("trial %d: scratch of no rows", trial);
      continue;
    }
    if (count != top - bot + 1) FAIL("trial %d: the rows with band cells are not contiguous", trial);
    if (r.rows != count || r.p_top != top || r.rows != 3 * r.codons || r.p_top != 3 * r.c_top + 2 ||
        (int64_t)r.p_top - r.rows + 1 != bot || bot % 3)
      FAIL("trial %d: rows %u top %u, want %lld top %lld", trial, r.rows, r.p_top, (long long)count, (long long)top);
    if (FrameDirBytes(r.rows, B) != (size_t)r.rows * BandDirStride(B)) FAIL("direction bytes");
    if (FrameScratchBytes(r.rows, B) != FrameDirBytes(r.rows, B) + 4 * FrameOpsSlot(r.rows, B)) FAIL("scratch bytes");
    if (FrameOpsSlot(r.rows, B) < (size_t)r.rows + 4 * B) FAIL("word slot of %u rows", r.rows);
    // random walks by the walk's rules from a random band cell: a pair (with or
    // without a shift after it, which must land on a band cell), 'D' or 'I',
    // until the walk leaves the band cells; the operations must fit the slot
    for (int w = 0; w < 4; ++w) {
      int64_t p = bot + rng() % count, j = p / 3 + D - B + rng() % (2 * B + 1);
      if (!Cell(p, j, m, D, B, s_lo, s_hi)) continue;
      size_t ops = 0;
      while (Cell(p, j, m, D, B, s_lo, s_hi)) {
        const uint32_t k = rng() % 8;
        if (k == 0) {
          ++j;  // 'D'
          ++ops;
        } else if (k == 1) {
          p += 3;  // 'I'
          ++ops;
        } else {
          const int64_t step = k == 2 ? 2 : k == 3 ? 4 : 3;
          if (step != 3 && !Cell(p + step, j + 1, m, D, B, s_lo, s_hi)) continue;  // a shift never ends a path
          p += step;
          ++j;
          ops += step == 3 ? 1 : 2;
        }
      }
      if (ops > FrameOpsSlot(r.rows, B)) FAIL("trial %d: a walk of %zu operations over a slot of %zu", trial, ops,
                                              FrameOpsSlot(r.rows, B));
    }
  }
  return 0;
}

static int Letters(std::mt19937 &rng) {
  for (int trial = 0; trial < 2000; ++trial) {
    const uint32_t W = 1 + rng() % 127, step = 1 + rng() % W, m = 1 + rng() % 700;
    const uint32_t first = rng() % 50, tiles = TileCount(m, W, step);
    const GhostmBandSource s{first, 6, tiles, m};
    for (uint32_t p = 0; p < 3 * m; ++p) {
      const uint32_t g = p % 3, c = p / 3;
      const size_t at = FrameStrandLetterAt(s, p, W, step);
      if (at != FrameLetterAt(s, g, c, W, step)) FAIL("trial %d: position %u", trial, p);
      const uint32_t rec = (uint32_t)(at / W), byte = (uint32_t)(at % W);
      if (rec < first + g || (rec - first - g) % 6) FAIL("trial %d: position %u in record %u", trial, p, rec);
      const uint32_t t = (rec - first - g) / 6;
      if (t >= tiles || (tiles == 1 && t)) FAIL("trial %d: position %u in tile %u of %u", trial, p, t, tiles);
      if (TileStart(t, tiles, m, W, step) + byte != c) FAIL("trial %d: position %u read as byte %u of tile %u", trial, p, byte, t);
    }
  }
  return 0;
}

static int Refusals() {
  const uint32_t W = 127, step = 64, nq = 20, db_len = 1000, lo = 10, hi = 400;
  const GhostmBandSource good{2, 6, 3, 200};  // frame 2's last tile is record 2 + 2 + 12 = 16
  struct Case {
    const char *want;
    GhostmBandSource s;
    uint32_t band;
    int open, ext, shift;
  };
  const Case cases[] = {
      {"", good, 31, -11, -1, -15},
      {"", good, 1, -1, -1, 0},
      {"", good, 31, -11, -1, -(1 << 20)},
      {"", GhostmBandSource{5, 6, 3, 200}, 31, -11, -1, -15},         // ... record 19
      {"", GhostmBandSource{17, 0, 1, 127}, 31, -11, -1, -15},        // one tile: the stride is not read
      {"shift", good, 31, -11, -1, 1},
      {"shift", good, 31, -11, -1, -(1 << 20) - 1},
      {"band", good, 0, -11, -1, -15},
      {"gaps", good, 31, -1, -2, -15},
      {"source", GhostmBandSource{6, 6, 3, 200}, 31, -11, -1, -15},   // frame 0 fits (record 18), frame 2 does not
      {"source", GhostmBandSource{18, 0, 1, 127}, 31, -11, -1, -15},  // one tile: frame 2 is record 20
      {"source", GhostmBandSource{UINT32_MAX - 1, 6, 1, 100}, 31, -11, -1, -15},
  };
  for (const Case &c : cases) {
    const std::string why = ValidateFrame(nq, W, db_len, 1, &c.s, &lo, &hi, step, c.band, c.open, c.ext, c.shift);
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
