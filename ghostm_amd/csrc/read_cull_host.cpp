// read_cull_host.cpp — host model of the read-level cull (GhostmReadCullHost,
// include/ghostm_hip.h): every read through CullRead (read_cull.h), the cull on
// elementary segments in the kernel's order of steps. No device call: this is
// the model k_read_cull (kernels.h) is checked against. The checks are
// ReadCullGpu's (ValidateReadCull).
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "read_cull.h"

namespace ghostm {
void SetLastErrorMessage(const std::string &m);
}

extern "C" int GhostmReadCullHost(uint32_t nreads, const uint32_t read_begin[], uint32_t nhits,
                                  const GhostmCullHit hit[], uint32_t top_k, uint32_t cover_pct,
                                  GhostmCullOut out[]) {
  using namespace ghostm;
  std::string why = ValidateReadCull(nreads, read_begin, nhits, hit, top_k, cover_pct);
  if (why.empty() && !out && nreads && read_begin[nreads] > read_begin[0]) why = "null: out";
  if (!why.empty()) {
    SetLastErrorMessage("GhostmReadCullHost: " + why);
    return 1;
  }
  for (uint32_t r = 0; r < nreads; ++r) {
    const uint32_t b = read_begin[r], n = read_begin[r + 1] - b;
    if (n) CullRead(hit + b, n, b, top_k, cover_pct, out + b);
  }
  return 0;
}
