// db_set.h — what `ghostm db` and a session's replaced database
// (Session::SetDb, GhostmSessionSetDb*) share: the chunk cut of the reference
// DBCreator (db_creator.cpp:88-128), so both cut a FASTA file into the same
// chunks. The FASTA reader is query_set.h's.
//
// The rule: a record joins the chunk while the sum of length + 1 (its letters
// and its END) stays within `db -l` MiB; the record that exceeds it is carried
// into the next chunk. A record that alone is over the limit is reported in
// either position. `ghostm db` keeps the reference's two behaviours on top of
// that: carried from an earlier chunk it is "too small max length", as the
// file's first record it silently ends the database with no chunk at all. The
// library (GhostmDbChunkCuts, GhostmSessionSetDb*) refuses in both positions.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "query_set.h"

namespace ghostm {

// db -l: the most bytes (letters and ENDs) of a chunk; 0: db's default.
constexpr uint32_t kDbChunkMbMax = 2047;  // 2048 MiB and more do not fit the 32-bit chunk offsets
inline uint32_t DbChunkLimit(uint32_t mb) { return mb ? mb * (1u << 20) : 1u << 27; }

class DbChunkCutter {
 public:
  explicit DbChunkCutter(uint32_t max_concat) : max_(max_concat) {}
  // a new chunk, with the record carried from the previous one (if any);
  // false: that record alone is over the limit
  bool Begin(bool carried, uint32_t len) {
    sum_ = carried ? (uint64_t)len + 1 : 0;
    return sum_ <= max_;
  }
  // the next record: true = it is the chunk's, false = it is carried
  bool Add(uint32_t len) {
    if (sum_ + len + 1 > max_) return false;
    sum_ += (uint64_t)len + 1;
    return true;
  }

 private:
  uint64_t max_, sum_ = 0;
};

// The records of a FASTA file chunk by chunk.
class DbChunkReader {
 public:
  DbChunkReader(const std::string &path, uint32_t max_concat) : reader_(path), cut_(max_concat) {}
  // 1: the next chunk's records; 0: no more; -1: a record alone is over the
  // limit (the file's first record, or the one carried into this chunk)
  int Next(std::vector<FastaRecord> *recs) {
    recs->clear();
    if (!cut_.Begin(pending_valid_, (uint32_t)pending_.seq.size())) return -1;
    if (pending_valid_) {
      recs->push_back(std::move(pending_));
      pending_valid_ = false;
    }
    FastaRecord r;
    while (reader_.Next(&r)) {
      if (!cut_.Add((uint32_t)r.seq.size())) {
        pending_ = r;
        pending_valid_ = true;
        break;
      }
      recs->push_back(r);
    }
    if (recs->empty()) return pending_valid_ ? -1 : 0;
    return 1;
  }

 private:
  FastaReader reader_;
  DbChunkCutter cut_;
  FastaRecord pending_;
  bool pending_valid_ = false;
};

// The same cuts over n record lengths: chunk c is records [cuts[c], cuts[c + 1]).
// false: a record alone is over the limit (the cuts made before it are kept).
inline bool DbChunkCuts(const uint32_t *len, uint64_t n, uint32_t max_concat, std::vector<uint64_t> *cuts) {
  DbChunkCutter cut(max_concat);
  cuts->assign(1, 0);
  uint64_t i = 0;
  while (i < n) {
    // record i starts the chunk: the file's first, or the one carried
    if (!cut.Begin(true, len[i])) return false;
    ++i;
    while (i < n && cut.Add(len[i])) ++i;
    cuts->push_back(i);
  }
  return true;
}

}  // namespace ghostm
