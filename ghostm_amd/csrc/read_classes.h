// read_classes.h — the batch plan of the per-read passes (DeviceModule::ReadCull,
// ReadLca): a batch's reads listed by size class and the `meta` words a class's
// launch indexes. Plain C++, so tests/native/test_read_classes.cpp runs it
// without a device.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace ghostm {

// One batch of m reads. A read's size (its hits for the cull, its candidates
// for the LCA) puts it in the first class whose bound it does not exceed, or in
// the global class above the last bound; a read of size 0 is not launched. The
// uploaded words:
//   meta[0 .. m]         the batch's slice of read_begin
//   per class, in order  its list (batch-local read indices in read order),
//                        then with_sizes those reads' sizes
//   padding to an even word
//   meta[offs_at ..]     one u64 per global-class read, in read order: the
//                        first word of its table
struct ReadClassPlan {
  std::vector<uint32_t> meta;
  std::vector<size_t> list_at, list_len;  // per class (the bounds and the global one): its list's place in meta
  size_t offs_at = 0;                     // the table offsets' place in meta, an even word
  size_t table_words = 0;                 // the tables together
  size_t launched = 0;                    // reads in a list

  // size[m]; bound[nbounds] ascending; table_words_of(r) is asked for every read above the last bound
  template <class TableWords>
  void Build(const uint32_t *read_begin, uint32_t m, const uint32_t *size, const uint32_t *bound, size_t nbounds,
             bool with_sizes, TableWords table_words_of) {
    const size_t classes = nbounds + 1;
    std::vector<std::vector<uint32_t>> list(classes);
    std::vector<unsigned long long> offs;
    table_words = 0;
    launched = 0;
    for (uint32_t r = 0; r < m; ++r) {
      if (size[r] == 0) continue;
      size_t c = 0;
      while (c < nbounds && size[r] > bound[c]) ++c;
      list[c].push_back(r);
      ++launched;
      if (c == nbounds) {
        offs.push_back(table_words);
        table_words += table_words_of(r);
      }
    }
    meta.assign(read_begin, read_begin + m + 1);
    list_at.assign(classes, 0);
    list_len.assign(classes, 0);
    for (size_t c = 0; c < classes; ++c) {
      list_at[c] = meta.size();
      list_len[c] = list[c].size();
      meta.insert(meta.end(), list[c].begin(), list[c].end());
      if (with_sizes)
        for (uint32_t r : list[c]) meta.push_back(size[r]);
    }
    if (meta.size() & 1) meta.push_back(0);
    offs_at = meta.size();
    meta.resize(offs_at + 2 * offs.size());
    if (!offs.empty()) memcpy(meta.data() + offs_at, offs.data(), offs.size() * 8);
  }
};

}  // namespace ghostm
