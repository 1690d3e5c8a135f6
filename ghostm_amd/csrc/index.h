// index.h — the k-mer index kernels (index.hip) as their two callers launch
// them: GhostmBuildIndexGpu (`db -D`: residues up, keys_count and positions
// back) and the resident build of a session's database
// (DeviceModule::FormatDb), on a stream and device buffers of the caller's.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ghostm {

// Throws unless the seed is one the index takes (not empty, weight at most 6)
// and kcl = 32^weight + 1.
void CheckIndexSeed(uint32_t seed, uint32_t kcl);

// The build's device temporaries for a chunk of len residues: four arrays of
// `pairs` bytes (the (key, position) pairs and their ping-pong copies: 16 bytes
// per position together) and the scans' small `tiles` and `hist` arrays.
struct IndexScratchBytes {
  size_t pairs = 0, tiles = 0, hist = 0;
};
IndexScratchBytes IndexScratchSize(uint32_t len, uint32_t kcl);

struct IndexScratch {
  uint32_t *key, *key2, *val, *val2, *tiles, *hist;
};

// Enqueues the whole build on `stream` (k_index_keys, the three-kernel scan,
// the LSD radix sort) over the len > 0 device residues d_seq. Afterwards, in
// stream order, d_counts[0 .. kcl) is keys_count, npos = d_counts[kcl - 1],
// and the first npos words at the returned pointer (s.val or s.val2) are the
// positions. No host wait and no copy.
const uint32_t *LaunchIndexBuild(void *stream, const uint8_t *d_seq, uint32_t len, uint32_t seed, uint32_t kcl,
                                 uint32_t *d_counts, const IndexScratch &s);

}  // namespace ghostm
