// qformat.h — the query formatting kernels (qformat.hip) as the device module
// launches them: on a stream and device buffers of the caller's.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ghostm {

// The kernels' lookup tables (letter -> code, codon -> code): their size and
// their bytes, to be placed in device memory by the caller.
size_t QueryFormatTableBytes();
void QueryFormatTables(void *host_dst);

// Codes (dna_len = 0) or six-frame-translates (dna_len = the chunk's read
// length, at least 1) n records into d_out: n (x 6) records of `width` codes.
// d_qlen (may be null): QueryResidues of every output record. Record r's
// letters are d_raw[d_off[r] .. d_off[r] + d_len[r]); the caller has checked
// them against the buffer.
void LaunchQueryFormat(void *stream, const uint8_t *d_raw, const uint64_t *d_off, const uint32_t *d_len, uint32_t n,
                       uint32_t width, uint32_t dna_len, uint8_t *d_out, uint32_t *d_qlen, const void *d_tab);

// The tiled forms (query_tiles.h): n source records become the output records
// d_first[r] .. of `width` codes each, a protein record's tiles consecutive, a
// DNA read's at d_first[r] + 6 t + f; d_len holds the kept letters (nt for
// DNA, every read translated at its own length), 1 <= step <= width. d_qlen:
// QueryResidues of every output record (never null). The caller has checked
// the records against the buffer and the tile counts against the plan's limit.
void LaunchQueryFormatTiled(void *stream, const uint8_t *d_raw, const uint64_t *d_off, const uint32_t *d_len,
                            const uint32_t *d_first, uint32_t n, uint32_t width, bool dna, uint32_t step,
                            uint8_t *d_out, uint32_t *d_qlen, const void *d_tab);

}  // namespace ghostm
