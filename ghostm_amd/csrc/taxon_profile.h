// taxon_profile.h — the host arithmetic of a sample's taxon profile
// (TaxonProfileGpu, GhostmTaxonProfileHost; the contract is above
// TaxonProfileGpu in include/ghostm_hip.h): the checks every call makes before
// anything is uploaded or launched, the profile written from the definitions
// (a dense count per node, a climb per node with a direct count), the summary,
// which follows from the records alone, and the text of -y 24 / -y 25. Plain
// C++ beside read_lca.h; tests/native/test_taxon_profile.cpp runs it without a
// device. The kernels (k_taxon_count, k_taxon_climb, k_taxon_floor,
// k_taxon_final, k_taxon_emit; kernels.h) reach the same records through lists
// of the nodes a call touches.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "read_lca.h"

namespace ghostm {

// Why a call is refused before its counts are known, or "" when it goes on.
// nnodes 0: no taxonomy.
inline std::string ValidateTaxonProfile(uint32_t nnodes, uint32_t nreads, const uint32_t *node, uint32_t min_reads,
                                        size_t cap, const GhostmTaxonCount *out, const size_t *nout) {
  if (min_reads == 0) return "param: min_reads 0";
  if (nreads && !node) return "null: node";
  if (!nout) return "null: nout";
  if (cap && !out) return "null: out";
  if (nnodes == 0) return "taxonomy: none is set";
  for (uint32_t r = 0; r < nreads; ++r)
    if (node[r] != kLcaNone && node[r] >= nnodes) return "node: read " + std::to_string(r) + ": no such node";
  return std::string();
}

// The refusal of a call whose records do not fit, or "" (cap 0 without out asks
// for the count).
inline std::string TaxonProfileCap(size_t need, size_t cap, const GhostmTaxonCount *out) {
  if (!out && cap == 0) return std::string();
  if (need > cap) return "cap: " + std::to_string(need) + " records needed, cap " + std::to_string(cap);
  return std::string();
}

// The summary of a call: everything but `reads` follows from the records.
// kept(n) counts the reads that end at n, so moved is kept less the direct
// reads of the nodes at or over the floor, which stay where they are.
inline GhostmTaxonSummary TaxonSummary(uint32_t nreads, const GhostmTaxonCount *rec, size_t nrec, uint32_t min_reads) {
  GhostmTaxonSummary s{};
  s.reads = nreads;
  s.nodes = nrec;
  uint64_t stay = 0;
  for (size_t k = 0; k < nrec; ++k) {
    s.classified += rec[k].direct_reads;
    s.kept += rec[k].kept_reads;
    if (rec[k].clade_reads >= min_reads) {
      ++s.nodes_kept;
      stay += rec[k].direct_reads;
    }
  }
  s.moved = s.kept - stay;
  return s;
}

// The profile from the definitions, over the packed words of a checked
// taxonomy and checked reads: the records in ascending node index, and
// final_node[nreads] when it is not null.
inline std::vector<GhostmTaxonCount> TaxonProfileModel(uint32_t nnodes, const uint32_t *tax, uint32_t nreads,
                                                       const uint32_t *node, uint32_t min_reads, uint32_t *final_node) {
  std::vector<uint32_t> direct(nnodes, 0), clade(nnodes, 0), kept(nnodes, 0), fin(nnodes, kLcaNone);
  std::vector<uint32_t> listed;  // the nodes with a direct count
  for (uint32_t r = 0; r < nreads; ++r)
    if (node[r] != kLcaNone && direct[node[r]]++ == 0) listed.push_back(node[r]);
  const auto up = [&](uint32_t n) { return tax[n] & 0xFFFFFFu; };
  for (uint32_t n : listed)
    for (uint32_t a = n;; a = up(a)) {
      clade[a] += direct[n];
      if (up(a) == a) break;
    }
  for (uint32_t n : listed)
    for (uint32_t a = n;; a = up(a)) {
      if (clade[a] >= min_reads) {
        fin[n] = a;
        kept[a] += direct[n];
        break;
      }
      if (up(a) == a) break;
    }
  if (final_node)
    for (uint32_t r = 0; r < nreads; ++r) final_node[r] = node[r] == kLcaNone ? kLcaNone : fin[node[r]];
  std::vector<GhostmTaxonCount> rec;
  for (uint32_t n = 0; n < nnodes; ++n)
    if (clade[n]) rec.push_back(GhostmTaxonCount{n, clade[n], direct[n], kept[n]});
  return rec;
}

// percent in hundredths, rounded half up in 64 bits, printed I.FF
inline void TaxonPercent(std::string *out, uint64_t part, uint64_t total) {
  const uint64_t h = (part * 10000u + total / 2) / total;
  out->append(std::to_string(h / 100));
  out->push_back('.');
  out->push_back((char)('0' + h / 10 % 10));
  out->push_back((char)('0' + h % 10));
}

inline void TaxonLine(std::string *out, uint64_t total, uint64_t clade, uint64_t kept, uint64_t direct, uint32_t depth,
                      uint32_t taxid, uint32_t parent_taxid) {
  TaxonPercent(out, clade, total);
  const uint64_t cols[6] = {clade, kept, direct, depth, taxid, parent_taxid};
  for (uint64_t c : cols) {
    out->push_back('\t');
    out->append(std::to_string(c));
  }
  out->push_back('\n');
}

// The report of -y 24 / -y 25 from a call's records (ascending node index):
// per line percent, clade_reads, kept_reads, direct_reads, depth, taxid,
// parent_taxid. First the unclassified reads (total - kept) when there are
// any, then the nodes at or over the floor in depth-first pre-order from the
// root, a node's children by clade_reads descending, then taxid ascending.
// total: the reads of the sample; 0 gives no text. parent, depth and taxid are
// indexed by node.
inline std::string TaxonReport(const GhostmTaxonCount *rec, size_t nrec, uint32_t min_reads, uint64_t total,
                               const uint32_t *parent, const uint32_t *depth, const uint32_t *taxid) {
  std::string out;
  if (total == 0) return out;
  std::vector<size_t> keep;  // the records at or over the floor
  uint64_t kept = 0;
  for (size_t k = 0; k < nrec; ++k) {
    kept += rec[k].kept_reads;
    if (rec[k].clade_reads >= min_reads) keep.push_back(k);
  }
  if (total > kept) TaxonLine(&out, total, total - kept, total - kept, total - kept, 0, 0, 0);
  if (keep.empty()) return out;
  // a kept node's parent is kept (clade never shrinks towards the root), so
  // the kept records are one tree; child lists as ranges of `order`
  const auto slot_of = [&](uint32_t n) {
    const auto it = std::lower_bound(keep.begin(), keep.end(), n, [&](size_t k, uint32_t v) { return rec[k].node < v; });
    return (size_t)(it - keep.begin());
  };
  const size_t m = keep.size();
  std::vector<size_t> par(m), first(m + 1, 0), order(m);
  size_t root = m;
  for (size_t s = 0; s < m; ++s) {
    const uint32_t n = rec[keep[s]].node;
    if (parent[n] == n) {
      root = s;
      par[s] = m;
      continue;
    }
    par[s] = slot_of(parent[n]);
    ++first[par[s] + 1];
  }
  if (root == m) return out;
  for (size_t s = 0; s < m; ++s) first[s + 1] += first[s];
  std::vector<size_t> fill(first.begin(), first.end() - 1);
  for (size_t s = 0; s < m; ++s)
    if (s != root) order[fill[par[s]]++] = s;
  const auto before = [&](size_t a, size_t b) {
    const GhostmTaxonCount &x = rec[keep[a]], &y = rec[keep[b]];
    if (x.clade_reads != y.clade_reads) return x.clade_reads > y.clade_reads;
    return taxid[x.node] < taxid[y.node];
  };
  for (size_t s = 0; s < m; ++s) std::sort(order.begin() + (long)first[s], order.begin() + (long)first[s + 1], before);
  std::vector<size_t> stack{root};
  while (!stack.empty()) {
    const size_t s = stack.back();
    stack.pop_back();
    const GhostmTaxonCount &x = rec[keep[s]];
    TaxonLine(&out, total, x.clade_reads, x.kept_reads, x.direct_reads, depth[x.node], taxid[x.node],
              taxid[parent[x.node]]);
    for (size_t k = first[s + 1]; k-- > first[s];) stack.push_back(order[k]);  // the first child on top
  }
  return out;
}

}  // namespace ghostm
