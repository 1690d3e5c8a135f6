// query_set.h — what `ghostm qry` and a session's replaced query set
// (Session::SetQueries, GhostmSessionSetQueries*) share: the FASTA reader, the
// record width rule and the chunk cuts of the reference QueryCreator
// (query_creator.cpp:119-240), so both cut a read set into the same chunks.
#pragma once
#include <cstdint>
#include <fstream>
#include <string>
#include <vector>

#include "common.h"

namespace ghostm {

struct FastaRecord {
  std::string name, seq;
};

// One record per Next(); the header line of the following record is kept
// (fasta_sequence_reader.cpp:34-86).
class FastaReader {
 public:
  explicit FastaReader(const std::string &path) : in_(path.c_str()) {}
  bool Next(FastaRecord *r);

 private:
  std::ifstream in_;
  std::string held_;
};

// qry -l / -t d: the record width; a DNA set's is a third of the read length
// given; at most kMaxQueryLength (*capped: qry prints its warning).
inline uint32_t QueryRecordWidth(uint32_t width, bool dna, bool *capped) {
  if (dna) width /= 3;
  *capped = width >= kMaxQueryLength;
  return *capped ? kMaxQueryLength : width;
}

// qry -L / -t d: the most letters a chunk holds; mb MiB (given) or qry's
// default, halved for DNA.
inline uint32_t QueryChunkLimit(bool given, uint32_t mb, bool dna) {
  const uint32_t max_concat = given ? mb * (1u << 20) : 1u << 27;
  return dna ? max_concat / 2 : max_concat;
}

// The chunk cut: records are added to a chunk while their letters' sum stays
// within the limit; the record that exceeds it is carried into the next chunk.
class QueryChunkCutter {
 public:
  explicit QueryChunkCutter(uint32_t max_concat) : max_(max_concat) {}
  // a new chunk, with the record carried from the previous one (if any);
  // false: that record alone is over the limit ("too small max length")
  bool Begin(bool carried, uint32_t len) {
    sum_ = carried ? len : 0;
    return sum_ <= max_;
  }
  // the next record: true = it is the chunk's, false = it is carried
  bool Add(uint32_t len) {
    sum_ += len;
    return sum_ <= max_;
  }

 private:
  uint32_t max_, sum_ = 0;
};

// The records of a FASTA file chunk by chunk.
class QueryChunkReader {
 public:
  QueryChunkReader(const std::string &path, uint32_t max_concat) : reader_(path), cut_(max_concat) {}
  // 1: the next chunk's records; 0: no more (as qry, also when the first
  // record of the file is over the limit); -1: too small max length
  int Next(std::vector<FastaRecord> *recs);

 private:
  FastaReader reader_;
  QueryChunkCutter cut_;
  FastaRecord pending_;
  bool pending_valid_ = false;
};

// The same cuts over n record lengths: chunk c is records [cuts[c], cuts[c + 1]).
// false: too small max length (the cuts made before it are kept).
bool QueryChunkCuts(const uint32_t *len, uint64_t n, uint32_t max_concat, std::vector<uint64_t> *cuts);

}  // namespace ghostm
