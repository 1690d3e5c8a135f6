// read_quality_host.cpp — host model of the quality stage (GhostmQualityTrimHost,
// include/ghostm_hip.h): every read is walked letter by letter from each end,
// straight from the rule in read_quality.h. No device call: this is the model
// k_qual_trim (read_quality.hip) is checked against.
#include <cstdint>
#include <string>

#include "../../include/ghostm_hip.h"
#include "read_quality.h"

namespace ghostm {
void SetLastErrorMessage(const std::string &m);
}

extern "C" int GhostmQualityTrimHost(uint8_t *letters, const uint8_t *qual, uint64_t total, const uint64_t offsets[],
                                     const uint32_t lengths[], uint32_t n, uint32_t trim_q, uint32_t mask_q,
                                     uint32_t min_len, GhostmQualOut out[]) {
  using namespace ghostm;
  const std::string why = ValidateQuality(letters, qual, total, offsets, lengths, n, trim_q, mask_q, min_len, out);
  if (!why.empty()) {
    SetLastErrorMessage("GhostmQualityTrimHost: " + why);
    return 1;
  }
  QualParams p;
  p.trim_q = trim_q;
  p.mask_q = mask_q;
  p.min_len = min_len;
  for (uint32_t r = 0; r < n; ++r) {
    if (!p.On()) out[r] = GhostmQualOut{0, lengths[r], 0, 0};  // off: the qualities are not read
    else out[r] = QualTrimRead(letters + offsets[r], qual + offsets[r], lengths[r], p);
  }
  return 0;
}
