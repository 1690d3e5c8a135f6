// fastq_reader.cpp — the strict four-line FASTQ reader (fastq_reader.h)
#include "fastq_reader.h"

namespace ghostm {

bool FastqReader::Line(std::string *line) {
  if (!std::getline(in_, *line)) return false;
  if (!line->empty() && line->back() == '\r') line->pop_back();
  return true;
}

bool FastqReader::Next(FastqRecord *r) {
  std::string line;
  do {
    if (!Line(&line)) return false;
  } while (line.empty());  // blank lines between records and at the end
  const std::string at = "fastq: record " + std::to_string(++record_) + ": ";
  if (line[0] != '@') throw FastqError(at + "header does not begin with '@'");
  r->name.clear();
  const size_t p = line.find_first_not_of(" ", 1);
  if (p != std::string::npos) r->name = line.substr(p);
  if (!Line(&r->seq)) throw FastqError(at + "truncated");
  if (!Line(&line)) throw FastqError(at + "truncated");
  if (line.empty() || line[0] != '+') throw FastqError(at + "no '+' line");
  if (!Line(&r->qual)) {
    if (!r->seq.empty()) throw FastqError(at + "truncated");
    r->qual.clear();  // an empty read whose empty quality line ends the file without a newline
  }
  if (r->qual.size() != r->seq.size())
    throw FastqError(at + std::to_string(r->seq.size()) + " letters, " + std::to_string(r->qual.size()) + " qualities");
  return true;
}

void ReadFastqSet(const std::string &path, FastqSet *set) {
  FastqReader reader(path);
  if (!reader.ok()) throw FastqError("fastq: cannot open " + path);
  *set = FastqSet();
  FastqRecord r;
  while (reader.Next(&r)) {
    if (r.seq.size() > UINT32_MAX) throw FastqError("fastq: record " + std::to_string(set->len.size() + 1) + ": over 4 G letters");
    set->off.push_back(set->letters.size());
    set->len.push_back((uint32_t)r.seq.size());
    set->letters += r.seq;
    set->qual += r.qual;
    set->names.push_back(r.name);
  }
}

bool LooksLikeFastq(const std::string &path) {
  std::ifstream in(path.c_str(), std::ios::binary);
  char c = 0;
  return in.get(c) && c == '@';
}

}  // namespace ghostm
