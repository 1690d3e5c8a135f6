// path_rows.h — the checks every aligned-rows call makes on the host before
// anything is uploaded or launched (PathRowsGpu, GhostmPathRowsHost, the
// session's rows post-pass), so that k_path_rows never receives an index it
// could read out of bounds with.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

struct GhostmHitPath;  // include/ghostm_hip.h

namespace ghostm {

// Checks nhits paths against a query chunk of nq records of L residues and a DB
// chunk of db_len residues; rec[i].s_start is absolute in the chunk. Returns an
// empty string and every hit's column count, or the reason:
//   "query"   query_ids[i] >= nq
//   "ops"     ops_offset + n_runs > ops_len
//   "word"    a word with bits 2-3 set or a zero length
//   "bounds"  the path's query residues run past L, its subject residues past
//             db_len, or its columns past 2^32 - 1
std::string ValidatePathRows(uint32_t nq, uint32_t L, uint32_t db_len, uint32_t nhits, const uint32_t *query_ids,
                             const GhostmHitPath *rec, const uint32_t *ops, size_t ops_len,
                             std::vector<uint32_t> *columns);

}  // namespace ghostm
