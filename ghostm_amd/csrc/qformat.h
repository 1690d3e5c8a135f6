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

}  // namespace ghostm
