// query_tiles.h — the tile plan of a tiled query set (Session::SetQueriesTiled,
// GhostmSessionSetQueries*Tiled, GhostmQueryTilePlan): a source longer than the
// record width W enters the search as overlapping W-letter tile records under
// its name, so the kernels behind the formatter stay at kMaxQueryLength. Plain
// host C++ beside query_set.h; qformat.hip restates TileCount / TileStart for
// the device.
//
// A source is a protein record's kept letters or one frame of a DNA read (n / 3
// letters). With 1 <= step <= W:
//   tiles    = 1 when m <= W, else 1 + ceil((m - W) / step)
//   start(t) = t * step for t < tiles - 1
//   start(tiles - 1) = max(m - W, 0): the last tile is flush right, so every
//              tile of a long source is full width and there is no stub tile
// Consecutive tiles overlap by at least W - step letters, so every window of at
// most W - step + 1 letters lies wholly inside some tile.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "common.h"

namespace ghostm {

// The most output records one source record may become. K4 keeps a name
// group's keys in LDS up to kMergeCap (kernels.h) and sends larger groups down
// its one-lane path; every tile record of a group can bring keys, so a group of
// more records than that could never take the wave path. 1024 tiles of a
// protein record, 170 tiles x 6 frames of a DNA read.
constexpr uint32_t kMaxTileRecords = 1024;

inline uint32_t TileCount(uint32_t m, uint32_t W, uint32_t step) {
  return m <= W ? 1u : 1u + (uint32_t)(((uint64_t)(m - W) + step - 1) / step);
}

inline uint32_t TileStart(uint32_t t, uint32_t tiles, uint32_t m, uint32_t W, uint32_t step) {
  return t + 1 < tiles ? t * step : (m > W ? m - W : 0u);
}

// the kept letters of a record of len letters (nt for DNA) under max_len (0: no cut)
inline uint32_t TileKept(uint32_t len, uint32_t max_len) { return max_len && len > max_len ? max_len : len; }

inline void CheckTileStep(uint32_t W, uint32_t step) {
  if (step == 0) throw Error("query tiles: a tile step of 0");
  if (step > W) throw Error("query tiles: tile step " + std::to_string(step) + " over the record width " + std::to_string(W));
}

// The output records of source record `record` (kept letters: nt for DNA) in
// output order: a protein record's tiles consecutive, a DNA read's tile-major
// and frame-minor (index 6 t + f). Returns their number; out may be null.
// Throws over kMaxTileRecords.
inline uint32_t AppendTiles(uint32_t record, uint32_t kept, uint32_t W, bool dna, uint32_t step,
                            std::vector<GhostmQueryTile> *out) {
  const uint32_t m = dna ? kept / 3 : kept, per = dna ? 6 : 1;
  const uint32_t tiles = TileCount(m, W, step);
  if ((uint64_t)tiles * per > kMaxTileRecords)
    throw Error("query tiles: record " + std::to_string(record) + " makes " + std::to_string((uint64_t)tiles * per) +
                " tile records, over the limit of " + std::to_string(kMaxTileRecords));
  if (out)
    for (uint32_t t = 0; t < tiles; ++t)
      for (uint32_t f = 0; f < per; ++f) out->push_back(GhostmQueryTile{record, TileStart(t, tiles, m, W, step), m, f});
  return tiles * per;
}

// A chunk's row count and bytes must fit the 32-bit fields of the chunk
// (QueryChunk::nseq, the kernels' byte offsets).
inline void CheckTiledChunk(uint64_t rows, uint32_t W) {
  if (rows > UINT32_MAX || rows * W + 16 > UINT32_MAX)
    throw Error("query tiles: a chunk of " + std::to_string(rows) + " tile records of " + std::to_string(W) +
                " letters wraps a 32-bit field");
}

}  // namespace ghostm
