// read_adapter_host.cpp — host model of the adapter stage (GhostmAdapterTrimHost,
// include/ghostm_hip.h): every start of every read and every fragment length of
// every pair is counted letter by letter, straight from the rule in
// read_adapter.h. No device call: this is the model k_adapter_find and
// k_pair_overlap (read_adapter.hip) are checked against.
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "read_adapter.h"

namespace ghostm {
void SetLastErrorMessage(const std::string &m);
}

extern "C" int GhostmAdapterTrimHost(const uint8_t *letters, uint64_t total, const uint64_t offsets[],
                                     const uint32_t lengths[], uint32_t n, const char *adapter1, const char *adapter2,
                                     uint32_t min_overlap, uint32_t err_pct, uint32_t pair_overlap,
                                     GhostmAdapterOut out[]) {
  using namespace ghostm;
  AdapterParams p;
  std::string why = MakeAdapterParams(adapter1, adapter2, min_overlap, err_pct, pair_overlap, &p);
  if (why.empty()) why = ValidateAdapters(letters, total, offsets, lengths, n, p.On() ? pair_overlap : 0, out);
  if (!why.empty()) {
    SetLastErrorMessage("GhostmAdapterTrimHost: " + why);
    return 1;
  }
  if (!p.On()) {  // off: the letters are not read
    for (uint32_t r = 0; r < n; ++r) out[r] = AdapterResult(lengths[r], lengths[r], 0, 0, 0);
    return 0;
  }
  std::vector<const uint8_t *> reads(n);
  for (uint32_t r = 0; r < n; ++r) reads[r] = letters + offsets[r];
  AdapterTrimReads(reads.data(), lengths, n, p, out, nullptr);
  return 0;
}
