// taxon_profile_host.cpp — host model of a sample's taxon profile
// (GhostmTaxonProfileHost; include/ghostm_hip.h): the taxonomy through
// TaxonomyDepths (read_lca.h), the profile through TaxonProfileModel
// (taxon_profile.h), written from the definitions. No device call: this is the
// model the k_taxon_* kernels (kernels.h) are checked against. The checks are
// SetTaxonomyGpu's and TaxonProfileGpu's.
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "taxon_profile.h"

namespace ghostm {
void SetLastErrorMessage(const std::string &m);
}

extern "C" int GhostmTaxonProfileHost(uint32_t nnodes, const uint32_t parent[], uint32_t nreads, const uint32_t node[],
                                      uint32_t min_reads, size_t cap, GhostmTaxonCount out[], size_t *nout,
                                      uint32_t final_node[], GhostmTaxonSummary *summary) {
  using namespace ghostm;
  std::vector<uint32_t> depth;
  std::string why = TaxonomyDepths(nnodes, parent, &depth);
  if (why.empty()) why = ValidateTaxonProfile(nnodes, nreads, node, min_reads, cap, out, nout);
  std::vector<GhostmTaxonCount> rec;
  std::vector<uint32_t> fin;
  if (why.empty()) {
    const std::vector<uint32_t> tax = TaxonomyWords(nnodes, parent, depth);
    if (final_node) fin.resize(nreads);
    rec = TaxonProfileModel(nnodes, tax.data(), nreads, node, min_reads, final_node ? fin.data() : nullptr);
    why = TaxonProfileCap(rec.size(), cap, out);
  }
  if (!why.empty()) {
    SetLastErrorMessage("GhostmTaxonProfileHost: " + why);
    return 1;
  }
  *nout = rec.size();
  if (!out) return 0;  // the count was asked for
  std::copy(rec.begin(), rec.end(), out);
  if (final_node) std::copy(fin.begin(), fin.end(), final_node);
  if (summary) *summary = TaxonSummary(nreads, rec.data(), rec.size(), min_reads);
  return 0;
}
