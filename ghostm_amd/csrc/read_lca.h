// read_lca.h — the host arithmetic of the per-read taxonomic assignment
// (SetTaxonomyGpu, ReadLcaGpu, GhostmReadLcaHost, GhostmTaxonomyDepths; the
// contract is above ReadLcaGpu in include/ghostm_hip.h): the checks every call
// makes before anything is uploaded or launched, the taxonomy's depths and
// packed words, the two text parsers of GhostmSessionSetTaxonomyFiles, and one
// read's assignment written as k_read_lca (kernels.h) does it: the score test
// over the compacted candidates, then the climb level by level from the read's
// deepest vote, counting equal nodes at each level. Plain C++ beside
// read_cull.h; tests/native/test_read_lca.cpp runs it without a device, and
// kernels.h restates the small functions for the device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/ghostm_hip.h"

namespace ghostm {

constexpr uint32_t kLcaNone = 0xFFFFFFFFu;
constexpr uint32_t kLcaMaxNodes = 1u << 24;     // a node's index fits the low 24 bits of its word
constexpr uint32_t kLcaMaxDepth = 255;          // and its depth the high 8
constexpr uint32_t kLcaValueLimit = 1u << 25;   // scores and coordinates stay below: score * 100 fits 32 bits
// Candidates per read. The score test is quadratic in a read's candidates:
// 16384^2 pair tests over a workgroup's 1024 lanes is 262144 iterations per
// lane, which stays in the milliseconds; a larger read is refused ("reads").
constexpr uint32_t kLcaReadLimit = 16384;
constexpr uint32_t kLcaWave = 64, kLcaCap = 1024;  // the classes' largest reads, in candidates

// A node's word: depth << 24 | parent.
inline uint32_t LcaWord(uint32_t depth, uint32_t parent) { return depth << 24 | parent; }

// The taxonomy's checks and depths. Returns "" and fills depth[nnodes], or the
// reason, naming the first offending node. A node's depth is found by walking
// up to the first node whose depth is known; a walk that meets a node of its
// own is a cycle.
inline std::string TaxonomyDepths(uint32_t nnodes, const uint32_t *parent, std::vector<uint32_t> *depth) {
  if (nnodes < 1 || nnodes > kLcaMaxNodes) return "taxonomy: " + std::to_string(nnodes) + " nodes outside 1..2^24";
  if (!parent) return "null: parent";
  uint32_t root = kLcaNone;
  for (uint32_t i = 0; i < nnodes; ++i) {
    if (parent[i] >= nnodes) return "taxonomy: node " + std::to_string(i) + ": parent out of range";
    if (parent[i] == i) {
      if (root != kLcaNone) return "taxonomy: node " + std::to_string(i) + ": a second root";
      root = i;
    }
  }
  if (root == kLcaNone) return "taxonomy: no root (no node is its own parent)";
  std::vector<uint32_t> &d = *depth;
  d.assign(nnodes, kLcaNone);
  d[root] = 0;
  std::vector<uint32_t> walk;
  for (uint32_t i = 0; i < nnodes; ++i) {
    if (d[i] != kLcaNone) continue;
    walk.clear();
    uint32_t n = i;
    while (d[n] == kLcaNone) {
      walk.push_back(n);
      d[n] = kLcaNone - 1;  // on this walk
      n = parent[n];
      if (d[n] == kLcaNone - 1) return "taxonomy: node " + std::to_string(i) + ": a cycle (the root is not reached)";
    }
    uint32_t at = d[n];
    for (size_t k = walk.size(); k-- > 0;) d[walk[k]] = ++at;
  }
  for (uint32_t i = 0; i < nnodes; ++i)
    if (d[i] > kLcaMaxDepth) return "taxonomy: node " + std::to_string(i) + ": deeper than 255";
  return std::string();
}

// The packed words of a checked taxonomy.
inline std::vector<uint32_t> TaxonomyWords(uint32_t nnodes, const uint32_t *parent, const std::vector<uint32_t> &depth) {
  std::vector<uint32_t> w(nnodes);
  for (uint32_t i = 0; i < nnodes; ++i) w[i] = LcaWord(depth[i], parent[i]);
  return w;
}

// The score test: h passes beside the best score ref of its stretch.
inline bool LcaPasses(uint32_t score, uint32_t ref, uint32_t top_pct) { return score * 100u >= (100u - top_pct) * ref; }

// thr of V votes.
inline uint32_t LcaThreshold(uint32_t votes, uint32_t support_pct) { return (support_pct * votes + 99u) / 100u; }

// Why a call is refused, or "" when it is taken; ncand (may be null) gets every
// read's candidate count. nnodes 0: no taxonomy.
inline std::string ValidateReadLca(uint32_t nnodes, uint32_t nreads, const uint32_t *read_begin, uint32_t nhits,
                                   const GhostmLcaHit *hit, uint32_t top_pct, uint32_t support_pct,
                                   std::vector<uint32_t> *ncand) {
  if (top_pct > 100) return "param: top_pct outside 0..100";
  if (support_pct < 51 || support_pct > 100) return "param: support_pct outside 51..100";
  if (nreads && !read_begin) return "null: read_begin";
  if (nhits && !hit) return "null: the hits";
  if (nnodes == 0) return "taxonomy: none is set";
  for (uint32_t r = 0; r < nreads; ++r)
    if (read_begin[r] > read_begin[r + 1]) return "reads: read " + std::to_string(r) + " ends before it begins";
  if (nreads && read_begin[nreads] > nhits) return "reads: the last read ends past nhits";
  for (uint32_t i = 0; i < nhits; ++i) {
    const GhostmLcaHit &h = hit[i];
    if (h.q_lo > h.q_hi) return "range: hit " + std::to_string(i) + ": q_lo above q_hi";
    if (h.q_hi >= kLcaValueLimit || h.score >= kLcaValueLimit)
      return "bounds: hit " + std::to_string(i) + ": a score or coordinate at or over 2^25";
    if (h.node != kLcaNone && h.node >= nnodes) return "node: hit " + std::to_string(i) + ": no such node";
  }
  if (ncand) ncand->assign(nreads, 0);
  for (uint32_t r = 0; r < nreads; ++r) {
    uint32_t c = 0;
    for (uint32_t i = read_begin[r]; i < read_begin[r + 1]; ++i) c += hit[i].score != 0;
    if (c > kLcaReadLimit) return "reads: read " + std::to_string(r) + " has more than 16384 candidates";
    if (ncand) (*ncand)[r] = c;
  }
  return std::string();
}

// The record of a read without a vote.
inline GhostmLcaOut LcaNoVote(uint32_t candidates, uint32_t unmapped, uint32_t best_score) {
  return GhostmLcaOut{kLcaNone, 0, 0, 0, kLcaNone, candidates, unmapped, best_score};
}

// One read's assignment, in the kernel's phases. tax: the packed words.
inline GhostmLcaOut LcaRead(const uint32_t *tax, const GhostmLcaHit *hit, uint32_t n, uint32_t top_pct,
                            uint32_t support_pct) {
  // 1. compact
  std::vector<GhostmLcaHit> c;
  for (uint32_t i = 0; i < n; ++i)
    if (hit[i].score) c.push_back(hit[i]);
  const uint32_t nc = (uint32_t)c.size();
  uint32_t best = 0, unmapped = 0, maxd = 0;
  // 2. the score test; the votes' cur and depth
  std::vector<uint32_t> cur, dep;
  for (uint32_t i = 0; i < nc; ++i) {
    uint32_t ref = 0;
    for (uint32_t j = 0; j < nc; ++j)
      if (c[j].q_lo <= c[i].q_hi && c[i].q_lo <= c[j].q_hi) ref = std::max(ref, c[j].score);
    best = std::max(best, c[i].score);
    if (!LcaPasses(c[i].score, ref, top_pct)) continue;
    if (c[i].node == kLcaNone) {
      ++unmapped;
      continue;
    }
    cur.push_back(c[i].node);
    dep.push_back(tax[c[i].node] >> 24);
    maxd = std::max(maxd, dep.back());
  }
  const uint32_t V = (uint32_t)cur.size();
  if (V == 0) return LcaNoVote(nc, unmapped, best);
  const uint32_t thr = LcaThreshold(V, support_pct);
  GhostmLcaOut o{kLcaNone, 0, V, 0, kLcaNone, nc, unmapped, best};
  // 3. the climb
  for (uint32_t level = maxd;; --level) {
    for (uint32_t v = 0; v < V && o.lca == kLcaNone; ++v) {
      if (dep[v] != level) continue;
      uint32_t count = 0;
      for (uint32_t w = 0; w < V; ++w) count += cur[w] == cur[v];  // equal nodes have equal depths
      if (o.node == kLcaNone && count >= thr) {
        o.node = cur[v];
        o.depth = level;
        o.support = count;
      }
      if (count == V) o.lca = cur[v];
    }
    if (o.lca != kLcaNone || level == 0) break;
    for (uint32_t v = 0; v < V; ++v)
      if (dep[v] == level) {
        cur[v] = tax[cur[v]] & 0xFFFFFFu;
        dep[v] = level - 1;
      }
  }
  return o;
}

// ------------------------------------------------------------------ the files
// A text file's taxonomy: nodes in file order.
struct TaxonomyFile {
  std::vector<uint32_t> taxid, parent;  // parent: node indices
};

inline bool LcaSep(char ch) { return ch == '\t' || ch == ' ' || ch == '|' || ch == '\r'; }

// an unsigned decimal at p (after separators); false when there is none or it
// does not fit 32 bits
inline bool LcaNumber(const char *&p, const char *end, uint32_t *v) {
  while (p < end && LcaSep(*p)) ++p;
  if (p == end || *p < '0' || *p > '9') return false;
  uint64_t x = 0;
  while (p < end && *p >= '0' && *p <= '9') {
    x = x * 10 + (uint64_t)(*p - '0');
    if (x > 0xFFFFFFFFull) return false;
    ++p;
  }
  *v = (uint32_t)x;
  return true;
}

// The nodes file: per line taxid and parent taxid, separated by any run of
// tabs, spaces and '|'; further fields ignored; blank lines skipped. "" or the
// reason with the line number (from 1).
inline std::string ParseTaxonomyNodes(const std::string &text, TaxonomyFile *out) {
  out->taxid.clear();
  out->parent.clear();
  std::vector<uint32_t> ptax, line_of;
  std::unordered_map<uint32_t, uint32_t> index;
  size_t pos = 0;
  uint32_t line = 0;
  while (pos < text.size()) {
    size_t nl = text.find('\n', pos);
    if (nl == std::string::npos) nl = text.size();
    ++line;
    const char *p = text.data() + pos, *end = text.data() + nl;
    pos = nl + 1;
    const char *q = p;
    while (q < end && LcaSep(*q)) ++q;
    if (q == end) continue;
    uint32_t t = 0, pt = 0;
    if (!LcaNumber(p, end, &t) || !LcaNumber(p, end, &pt))
      return "taxonomy: nodes line " + std::to_string(line) + ": two unsigned integers expected";
    if (t == 0) return "taxonomy: nodes line " + std::to_string(line) + ": taxid 0";
    if (!index.emplace(t, (uint32_t)out->taxid.size()).second)
      return "taxonomy: nodes line " + std::to_string(line) + ": taxid " + std::to_string(t) + " repeated";
    out->taxid.push_back(t);
    ptax.push_back(pt);
    line_of.push_back(line);
  }
  out->parent.resize(ptax.size());
  for (size_t i = 0; i < ptax.size(); ++i) {
    const auto it = index.find(ptax[i]);
    if (it == index.end())
      return "taxonomy: nodes line " + std::to_string(line_of[i]) + ": parent " + std::to_string(ptax[i]) +
             " is not defined";
    out->parent[i] = it->second;
  }
  return std::string();
}

// The map file: per line name, whitespace, taxid. names (name, taxid) in file
// order and their line numbers; the caller lets a later line win. "" or the reason with the line number.
inline std::string ParseTaxonomyMap(const std::string &text, std::vector<std::pair<std::string, uint32_t>> *out,
                                    std::vector<uint32_t> *line_of) {
  out->clear();
  line_of->clear();
  size_t pos = 0;
  uint32_t line = 0;
  while (pos < text.size()) {
    size_t nl = text.find('\n', pos);
    if (nl == std::string::npos) nl = text.size();
    ++line;
    const char *p = text.data() + pos, *end = text.data() + nl;
    pos = nl + 1;
    while (p < end && (*p == ' ' || *p == '\t' || *p == '\r')) ++p;
    if (p == end) continue;
    const char *name = p;
    while (p < end && *p != ' ' && *p != '\t' && *p != '\r') ++p;
    const std::string nm(name, p);
    uint32_t t = 0;
    const char *q = p;
    while (q < end && (*q == ' ' || *q == '\t')) ++q;
    if (!LcaNumber(q, end, &t)) return "map: line " + std::to_string(line) + ": name and taxid expected";
    out->emplace_back(nm, t);
    line_of->push_back(line);
  }
  return std::string();
}

// A subject's name as the map compares it: up to its first space or tab.
inline std::string LcaNameKey(const std::string &name) {
  const size_t e = name.find_first_of(" \t");
  return e == std::string::npos ? name : name.substr(0, e);
}

// Table words of a read of nc candidates above kLcaCap, in k_read_lca's layout:
// 10 arrays of P words, P the power of two at or above nc.
inline uint32_t LcaPow2(uint32_t n) {
  uint32_t p = 2;
  while (p < n) p <<= 1;
  return p;
}
constexpr uint32_t kLcaTableArrays = 10;

}  // namespace ghostm
