// read_lca_host.cpp — host model of the per-read taxonomic assignment
// (GhostmReadLcaHost, GhostmTaxonomyDepths; include/ghostm_hip.h): the
// taxonomy through TaxonomyDepths, every read through LcaRead (read_lca.h), in
// the kernel's order of phases. No device call: this is the model k_read_lca
// (kernels.h) is checked against. The checks are SetTaxonomyGpu's and
// ReadLcaGpu's.
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "read_lca.h"

namespace ghostm {
void SetLastErrorMessage(const std::string &m);
}

extern "C" int GhostmTaxonomyDepths(uint32_t nnodes, const uint32_t parent[], uint32_t depth_out[]) {
  using namespace ghostm;
  std::vector<uint32_t> depth;
  std::string why = TaxonomyDepths(nnodes, parent, &depth);
  if (why.empty() && !depth_out) why = "null: depth_out";
  if (!why.empty()) {
    SetLastErrorMessage("GhostmTaxonomyDepths: " + why);
    return 1;
  }
  std::copy(depth.begin(), depth.end(), depth_out);
  return 0;
}

extern "C" int GhostmReadLcaHost(uint32_t nnodes, const uint32_t parent[], uint32_t nreads,
                                 const uint32_t read_begin[], uint32_t nhits, const GhostmLcaHit hit[],
                                 uint32_t top_pct, uint32_t support_pct, GhostmLcaOut out[]) {
  using namespace ghostm;
  std::vector<uint32_t> depth;
  std::string why = TaxonomyDepths(nnodes, parent, &depth);
  if (why.empty()) why = ValidateReadLca(nnodes, nreads, read_begin, nhits, hit, top_pct, support_pct, nullptr);
  if (why.empty() && !out && nreads) why = "null: out";
  if (!why.empty()) {
    SetLastErrorMessage("GhostmReadLcaHost: " + why);
    return 1;
  }
  const std::vector<uint32_t> tax = TaxonomyWords(nnodes, parent, depth);
  for (uint32_t r = 0; r < nreads; ++r) {
    const uint32_t b = read_begin[r];
    out[r] = LcaRead(tax.data(), hit + b, read_begin[r + 1] - b, top_pct, support_pct);
  }
  return 0;
}
