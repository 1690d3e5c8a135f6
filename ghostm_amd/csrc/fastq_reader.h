// fastq_reader.h — strict four-line FASTQ (the session's SetQueriesFastq*Tiled,
// `ghostm search` on a file that begins with '@'). A file of its own with no
// other header of the project, so tests/native/test_read_quality.cpp compiles
// it without the session.
//   @name        the name is the line after '@' with leading blanks dropped
//   letters      one line
//   +anything
//   qualities    one line, as many bytes as letters
// CRLF is tolerated; blank lines are allowed only between records and at the
// end. Multi-line FASTQ and compressed files are not read.
#pragma once
#include <cstdint>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

namespace ghostm {

// what Next() throws: "fastq: record N: <reason>", N counted from 1
struct FastqError : std::runtime_error {
  explicit FastqError(const std::string &m) : std::runtime_error(m) {}
};

struct FastqRecord {
  std::string name, seq, qual;
};

class FastqReader {
 public:
  explicit FastqReader(const std::string &path) : in_(path.c_str(), std::ios::binary) {}
  bool ok() const { return in_.is_open(); }
  // the next record; false at the end of the file; throws FastqError
  bool Next(FastqRecord *r);

 private:
  bool Line(std::string *line);  // without its "\n" or "\r\n"; false at the end
  std::ifstream in_;
  uint64_t record_ = 0;
};

// A whole file's reads in one letter and one quality buffer: read r is len[r]
// bytes at off[r] of both.
struct FastqSet {
  std::string letters, qual;
  std::vector<uint64_t> off;
  std::vector<uint32_t> len;
  std::vector<std::string> names;
};
// throws FastqError (also "fastq: cannot open PATH" and a read of over 4 G letters)
void ReadFastqSet(const std::string &path, FastqSet *set);

// true when the file's first byte is '@'
bool LooksLikeFastq(const std::string &path);

}  // namespace ghostm
