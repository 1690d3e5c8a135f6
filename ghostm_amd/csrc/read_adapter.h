// read_adapter.h — host arithmetic of the adapter stage of a FASTQ read set
// (GhostmAdapterTrimHost, AdapterTrimGpu, DeviceModule::AdapterTrim, the
// session's SetAdapters): the parameters' ranges, the checks every call makes
// before anything is uploaded or launched, the rule for one read and for one
// pair of mates, and the counters a read adds. Plain C++, so
// tests/native/test_read_adapter.cpp runs it without a device;
// read_adapter.hip restates the rule for one wave.
//
// The rule (include/ghostm_hip.h, above GhostmAdapterTrimHost). Letters: a read
// byte is upper-cased and is then A, C, G, T or "other"; an adapter letter is
// A, C, G, T or N, and N matches every read byte, while "other" matches nothing
// else. Adapter rule: start p, L = min(m, n - p), mm(p) the mismatches over L,
// p accepted when L >= min_overlap and mm * 100 <= err_pct * L; adapter_at is
// the smallest accepted p, or n. Pair rule: fragment length f in
// pair_overlap..min(n1, n2), pm(f) the i < f where R1[i] is not the complement
// of R2[f - 1 - i]; f accepted when pm * 100 <= err_pct * f; pair_len is the
// greatest accepted f, or 0. kept = min(adapter_at, pair_len ? pair_len : n).
// No indels: fastp's and Trimmomatic's rule, not cutadapt's alignment.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/ghostm_hip.h"

namespace ghostm {

constexpr uint32_t kAdapterLettersMax = 64;        // of an adapter: one lane's count fits the wave's group
constexpr uint32_t kAdapterOverlapMax = 64;        // min_overlap 1..64
constexpr uint32_t kAdapterErrPctMax = 50;         // err_pct 0..50
constexpr uint32_t kAdapterPairLettersMax = 1024;  // of a mate the pair rule examines, and pair_overlap's greatest value
constexpr uint32_t kAdapterLengthMax = 1u << 24;   // of a read

// letter codes: 0..3 = A C G T; a read's other bytes are kAdapterOther, an adapter's N is kAdapterAny
constexpr uint8_t kAdapterOther = 4, kAdapterAny = 0xFF;

inline uint8_t AdapterReadCode(uint8_t byte) {
  if (byte >= 'a' && byte <= 'z') byte = (uint8_t)(byte - 32);
  return byte == 'A' ? 0 : byte == 'C' ? 1 : byte == 'G' ? 2 : byte == 'T' ? 3 : kAdapterOther;
}

struct AdapterParams {
  // the adapters as codes (0..3, kAdapterAny); m1, m2 letters, 0: none
  uint8_t a1[kAdapterLettersMax] = {}, a2[kAdapterLettersMax] = {};
  uint32_t m1 = 0, m2 = 0;
  uint32_t min_overlap = 5, err_pct = 10, pair_overlap = 0;
  bool On() const { return m1 || m2 || pair_overlap; }
  // record r's adapter: adapter2 for the odd records when there is one
  const uint8_t *Adapter(uint32_t r, uint32_t *m) const {
    const bool second = (r & 1) && m2;
    *m = second ? m2 : m1;
    return second ? a2 : a1;
  }
};

// "param" followed by the detail, or ""
inline std::string ValidateAdapterParams(uint32_t min_overlap, uint32_t err_pct, uint32_t pair_overlap) {
  if (min_overlap < 1 || min_overlap > kAdapterOverlapMax)
    return "param: min_overlap " + std::to_string(min_overlap) + " outside 1..64";
  if (err_pct > kAdapterErrPctMax) return "param: err_pct " + std::to_string(err_pct) + " outside 0..50";
  if (pair_overlap > kAdapterPairLettersMax)
    return "param: pair_overlap " + std::to_string(pair_overlap) + " outside 0..1024";
  return std::string();
}

// One adapter (null: none) into codes; "adapter" followed by the detail, or "".
inline std::string AdapterCodes(const char *text, const char *which, uint8_t *codes, uint32_t *m) {
  *m = 0;
  if (!text) return std::string();
  uint32_t n = 0;
  for (; text[n]; ++n) {
    if (n >= kAdapterLettersMax) return std::string("adapter: ") + which + " has over 64 letters";
    const uint8_t c = (uint8_t)text[n];
    const uint8_t code = AdapterReadCode(c);
    if (code != kAdapterOther) codes[n] = code;
    else if (c == 'N' || c == 'n') codes[n] = kAdapterAny;
    else return std::string("adapter: ") + which + " letter " + std::to_string(n) + " is none of ACGTN";
  }
  *m = n;
  return std::string();
}

// The parameters and both adapters; "param" or "adapter" followed by the detail, or "". *p is set only on "".
inline std::string MakeAdapterParams(const char *adapter1, const char *adapter2, uint32_t min_overlap, uint32_t err_pct,
                                     uint32_t pair_overlap, AdapterParams *p) {
  std::string why = ValidateAdapterParams(min_overlap, err_pct, pair_overlap);
  if (!why.empty()) return why;
  AdapterParams q;
  why = AdapterCodes(adapter1, "adapter1", q.a1, &q.m1);
  if (why.empty()) why = AdapterCodes(adapter2, "adapter2", q.a2, &q.m2);
  if (!why.empty()) return why;
  q.min_overlap = min_overlap;
  q.err_pct = err_pct;
  q.pair_overlap = pair_overlap;
  *p = q;
  return std::string();
}

// Why a call is refused ("null", "record", "length", "pairs", each followed by
// the detail), or "". The parameters and the adapters are checked before, by
// MakeAdapterParams.
inline std::string ValidateAdapters(const uint8_t *letters, uint64_t total, const uint64_t *offsets,
                                    const uint32_t *lengths, uint32_t n, uint32_t pair_overlap,
                                    const GhostmAdapterOut *out) {
  if (n && (!offsets || !lengths || !out)) return "null: an array";
  if (total && n && !letters) return "null: the letters";
  for (uint32_t r = 0; r < n; ++r) {
    if (offsets[r] > total || lengths[r] > total - offsets[r])
      return "record: read " + std::to_string(r) + " outside the " + std::to_string(total) + " bytes given";
    if (lengths[r] > kAdapterLengthMax) return "length: read " + std::to_string(r) + " has over 2^24 letters";
  }
  if (pair_overlap && (n & 1)) return "pairs: " + std::to_string(n) + " records are no whole pairs";
  return std::string();
}

// The adapter rule for one read, letter by letter: adapter_at (n: none) and the accepted match's mismatches.
inline uint32_t AdapterFind(const uint8_t *read, uint32_t n, const uint8_t *adapter, uint32_t m, uint32_t min_overlap,
                            uint32_t err_pct, uint32_t *mismatches) {
  *mismatches = 0;
  if (m == 0) return n;
  for (uint32_t p = 0; p < n; ++p) {
    const uint32_t L = m < n - p ? m : n - p;
    if (L < min_overlap) break;  // L only falls from here on
    uint32_t mm = 0;
    for (uint32_t i = 0; i < L; ++i) mm += adapter[i] != kAdapterAny && AdapterReadCode(read[p + i]) != adapter[i];
    if (mm * 100 <= err_pct * L) {
      *mismatches = mm;
      return p;
    }
  }
  return n;
}

// Whether the pair rule examines a pair; *skipped: it is over the letter limit.
inline bool AdapterPairExamined(uint32_t n1, uint32_t n2, uint32_t pair_overlap, bool *skipped) {
  *skipped = pair_overlap && (n1 > kAdapterPairLettersMax || n2 > kAdapterPairLettersMax);
  return pair_overlap && !*skipped && (n1 < n2 ? n1 : n2) >= pair_overlap;
}

// The pair rule for one pair, letter by letter: pair_len (0: none) and the accepted length's mismatches.
inline uint32_t AdapterPairLen(const uint8_t *r1, uint32_t n1, const uint8_t *r2, uint32_t n2, uint32_t pair_overlap,
                               uint32_t err_pct, uint32_t *mismatches) {
  *mismatches = 0;
  bool skipped;
  if (!AdapterPairExamined(n1, n2, pair_overlap, &skipped)) return 0;
  for (uint32_t f = n1 < n2 ? n1 : n2; f >= pair_overlap; --f) {
    uint32_t pm = 0;
    for (uint32_t i = 0; i < f; ++i) {
      const uint8_t x = AdapterReadCode(r1[i]), y = AdapterReadCode(r2[f - 1 - i]);
      pm += x == kAdapterOther || y == kAdapterOther || x != 3 - y;
    }
    if (pm * 100 <= err_pct * f) {
      *mismatches = pm;
      return f;
    }
  }
  return 0;
}

inline GhostmAdapterOut AdapterResult(uint32_t n, uint32_t adapter_at, uint32_t adapter_mm, uint32_t pair_len,
                                      uint32_t pair_mm) {
  const uint32_t by_pair = pair_len ? pair_len : n;
  GhostmAdapterOut o;
  o.kept = adapter_at < by_pair ? adapter_at : by_pair;
  o.adapter_at = adapter_at;
  o.pair_len = pair_len;
  o.adapter_mismatches = (uint16_t)adapter_mm;
  o.pair_mismatches = (uint16_t)pair_mm;
  return o;
}

// The counters of a pass besides launches, reads, letters and the time: what
// the reads add up to. pair_found and pair_skipped count pairs (the even record
// adds them), the others reads; emptied are the reads with letters that keep none.
struct AdapterSums {
  uint64_t cut_reads = 0, cut_letters = 0, adapter_found = 0, pair_found = 0, pair_skipped = 0, emptied = 0;
};
inline void AdapterAdd(AdapterSums *s, uint32_t r, uint32_t n, const GhostmAdapterOut &o, bool pair_skipped) {
  s->cut_reads += o.kept < n;
  s->cut_letters += n - o.kept;
  s->adapter_found += o.adapter_at < n;
  s->pair_found += !(r & 1) && o.pair_len;
  s->pair_skipped += !(r & 1) && pair_skipped;
  s->emptied += n && !o.kept;
}

// The whole rule over n reads (read r = lengths[r] bytes at reads[r]); with
// pair_overlap > 0 n is even. The model behind GhostmAdapterTrimHost.
inline void AdapterTrimReads(const uint8_t *const *reads, const uint32_t *lengths, uint32_t n, const AdapterParams &p,
                             GhostmAdapterOut *out, AdapterSums *sums) {
  for (uint32_t r = 0; r < n; ++r) {
    uint32_t pair_len = 0, pair_mm = 0;
    bool skipped = false;
    if (p.pair_overlap) {
      const uint32_t e = r & ~1u;
      AdapterPairExamined(lengths[e], lengths[e + 1], p.pair_overlap, &skipped);
      if (r & 1) pair_len = out[e].pair_len, pair_mm = out[e].pair_mismatches;
      else pair_len = AdapterPairLen(reads[e], lengths[e], reads[e + 1], lengths[e + 1], p.pair_overlap, p.err_pct, &pair_mm);
    }
    uint32_t m, mm;
    const uint8_t *adapter = p.Adapter(r, &m);
    const uint32_t at = AdapterFind(reads[r], lengths[r], adapter, m, p.min_overlap, p.err_pct, &mm);
    out[r] = AdapterResult(lengths[r], at, mm, pair_len, pair_mm);
    if (sums) AdapterAdd(sums, r, lengths[r], out[r], skipped);
  }
}

// The six sums of a pass are kept in kAdapterCounterSlots slots of
// kAdapterCounterWords 64-bit words (a cache line each; words 0..5 used:
// cut_reads, cut_letters, adapter_found, pair_found, pair_skipped, emptied), a
// wave adding its sums to the slot of its number, as the quality and the mask
// pass do. The caller adds the slots up.
constexpr uint32_t kAdapterCounterSlots = 128, kAdapterCounterWords = 16;
// the launches: four waves to a block, at most this many blocks, the waves striding over the reads or the pairs
constexpr uint32_t kAdapterBlocksMax = 1024;

// Launches the stage's kernels (read_adapter.hip) on the caller's stream over n
// reads, read r = len[r] bytes at off[r] of d_letters: k_adapter_find when an
// adapter is set, then k_pair_overlap when the pair rule is on (n is then
// even). d_out = n records, d_counters = the counter slots, both zero on entry.
// The letters are only read. Returns the kernels launched. The caller has made
// ValidateAdapters' checks and p.On() holds.
uint32_t LaunchAdapterTrim(void *stream, const uint8_t *d_letters, const uint64_t *d_off, const uint32_t *d_len,
                           uint32_t n, const AdapterParams &p, GhostmAdapterOut *d_out, uint64_t *d_counters);

}  // namespace ghostm
