// pair_join_host.cpp — host model of the mate-pair join (GhostmPairJoinHost,
// include/ghostm_hip.h): every pair through PairJoinOne (pair_join.h), in the
// kernel's order of phases. No device call: this is the model k_pair_join
// (kernels.h) is checked against. The checks are PairJoinGpu's
// (ValidatePairJoin).
#include <string>

#include "../../include/ghostm_hip.h"
#include "pair_join.h"

namespace ghostm {
void SetLastErrorMessage(const std::string &m);
}

extern "C" int GhostmPairJoinHost(uint32_t npairs, const uint32_t pair_begin[], const uint32_t offset[],
                                  uint32_t nhits, const GhostmPairHit hit[], uint32_t max_span, uint32_t orient,
                                  GhostmLcaHit cand[], uint32_t partner[], GhostmPairOut out[]) {
  using namespace ghostm;
  std::string why = ValidatePairJoin(npairs, pair_begin, offset, nhits, hit, max_span, orient);
  if (why.empty() && npairs && !out) why = "null: out";
  if (why.empty() && npairs && pair_begin[2 * (size_t)npairs] > pair_begin[0] && (!cand || !partner))
    why = "null: cand or partner";
  if (!why.empty()) {
    SetLastErrorMessage("GhostmPairJoinHost: " + why);
    return 1;
  }
  for (uint32_t p = 0; p < npairs; ++p) {
    const uint32_t b = pair_begin[2 * (size_t)p], n1 = pair_begin[2 * (size_t)p + 1] - b,
                   n2 = pair_begin[2 * (size_t)p + 2] - pair_begin[2 * (size_t)p + 1];
    if (n1 + n2 == 0) out[p] = GhostmPairOut{0, 0, 0, 0};
    else out[p] = PairJoinOne(hit + b, n1, n2, b, offset[p], max_span, orient, cand + b, partner + b);
  }
  return 0;
}
