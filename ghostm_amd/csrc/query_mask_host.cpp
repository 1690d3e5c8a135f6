// query_mask_host.cpp — host model of the low-complexity mask
// (GhostmMaskRecordsHost, include/ghostm_hip.h): every source's letters are read
// through its tile records, every window's counts are taken letter by letter,
// the runs of low windows are walked one window at a time, and the masked
// letters are stored into every tile record that covers them. No device call:
// this is the model k_mask_windows / k_mask_apply (query_mask.hip) are checked
// against.
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "query_mask.h"

namespace ghostm {
void SetLastErrorMessage(const std::string &m);
}

namespace {

int Fail(const std::string &m) {
  ghostm::SetLastErrorMessage("GhostmMaskRecordsHost: " + m);
  return 1;
}

}  // namespace

extern "C" int GhostmMaskRecordsHost(uint8_t *query_seqs, uint32_t nq, uint32_t L, uint32_t nsrc,
                                     const GhostmBandSource src[], uint32_t step, uint32_t window, uint32_t trigger,
                                     uint32_t extend, uint32_t masked[]) {
  using namespace ghostm;
  if ((nq && (!query_seqs || !masked)) || (nsrc && !src)) return Fail("null: an array");
  const std::string why = ValidateMask(nq, L, nsrc, src, step, window, trigger, extend);
  if (!why.empty()) return Fail(why);
  const MaskTable tab = MakeMaskTable();
  const uint32_t w = window;
  const uint64_t low_at = (uint64_t)extend * 1024 * w, trigger_at = (uint64_t)trigger * 1024 * w;
  std::fill(masked, masked + nq, 0u);
  std::vector<uint8_t> letter, low, trig, mask;
  for (uint32_t h = 0; h < nsrc; ++h) {
    const GhostmBandSource &S = src[h];
    const uint32_t m = S.letters;
    if (m < w) continue;
    letter.resize(m);
    for (uint32_t p = 0; p < m; ++p) letter[p] = query_seqs[BandLetterAt(S, p, L, step)];
    const uint32_t nw = m - w + 1;
    low.assign(nw, 0);
    trig.assign(nw, 0);
    for (uint32_t i = 0; i < nw; ++i) {
      uint32_t count[kBaseX] = {0};
      bool evaluated = true;
      for (uint32_t j = 0; j < w; ++j) {
        if (letter[i + j] >= kBaseX) evaluated = false;
        else ++count[letter[i + j]];
      }
      if (!evaluated) continue;
      uint64_t sum = 0;
      for (uint32_t a = 0; a < kBaseX; ++a) sum += tab.T[count[a]];
      const uint64_t d = 100 * ((uint64_t)tab.T[w] - sum);
      low[i] = d <= low_at;
      trig[i] = d <= trigger_at;
    }
    mask.assign(m, 0);
    for (uint32_t i = 0; i < nw;) {
      if (!low[i]) {
        ++i;
        continue;
      }
      uint32_t j = i;
      bool has = false;
      for (; j < nw && low[j]; ++j) has = has || trig[j];
      if (has) std::fill(mask.begin() + i, mask.begin() + (j - 1 + w), 1);  // windows i..j-1: letters [i, j - 1 + w)
      i = j;
    }
    for (uint32_t t = 0; t < S.tiles; ++t) {
      const uint32_t start = TileStart(t, S.tiles, m, L, step);
      const size_t rec = S.first_record + (S.tiles > 1 ? (size_t)S.stride * t : 0);
      for (uint32_t k = 0; k < L && start + k < m; ++k) {
        if (!mask[start + k]) continue;
        query_seqs[rec * L + k] = kBaseX;
        ++masked[rec];
      }
    }
  }
  return 0;
}
