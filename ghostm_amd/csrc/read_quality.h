// read_quality.h — host arithmetic of the quality stage of a FASTQ read set
// (GhostmQualityTrimHost, QualityTrimGpu, DeviceModule::QualityTrim, the
// session's SetQuality): the parameters' ranges, the checks every call makes
// before anything is uploaded or launched, the rule for one read and the
// counters a read adds. Plain C++, so tests/native/test_read_quality.cpp runs it
// without a device; read_quality.hip restates the rule for one wave.
//
// The rule (include/ghostm_hip.h, above GhostmQualityTrimHost): q[i] =
// min(max(byte, 33), 126) - 33, d[i] = trim_q - q[i]. Each end is found on the
// untrimmed read by BWA's running sum: walk inwards adding d[i], stop at the
// first sum below 0, cut where the sum first reached its greatest value above 0.
// Then the floor (kept < min_len empties the read), then every kept letter
// with q[i] < mask_q becomes 'N'.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/ghostm_hip.h"

namespace ghostm {

constexpr uint32_t kQualScoreMax = 93;        // '~' - '!'
constexpr uint32_t kQualLengthMax = 1u << 24;  // of a read, and of min_len: the sums stay within 32 bits

struct QualParams {
  uint32_t trim_q = 0, mask_q = 0, min_len = 0;  // all 0: the stage is off
  bool On() const { return trim_q || mask_q || min_len; }
};

// "param" followed by the detail, or ""
inline std::string ValidateQualParams(uint32_t trim_q, uint32_t mask_q, uint32_t min_len) {
  if (trim_q > kQualScoreMax) return "param: trim_q " + std::to_string(trim_q) + " outside 0..93";
  if (mask_q > kQualScoreMax) return "param: mask_q " + std::to_string(mask_q) + " outside 0..93";
  if (min_len > kQualLengthMax) return "param: min_len " + std::to_string(min_len) + " outside 0..2^24";
  return std::string();
}

// Why a call is refused ("param", "null", "record", "length", each followed by
// the detail), or "".
inline std::string ValidateQuality(const uint8_t *letters, const uint8_t *qual, uint64_t total, const uint64_t *offsets,
                                   const uint32_t *lengths, uint32_t n, uint32_t trim_q, uint32_t mask_q,
                                   uint32_t min_len, const GhostmQualOut *out) {
  const std::string why = ValidateQualParams(trim_q, mask_q, min_len);
  if (!why.empty()) return why;
  if (n && (!offsets || !lengths || !out)) return "null: an array";
  if (total && n && (!letters || !qual)) return "null: the letters or the qualities";
  for (uint32_t r = 0; r < n; ++r) {
    if (offsets[r] > total || lengths[r] > total - offsets[r])
      return "record: read " + std::to_string(r) + " outside the " + std::to_string(total) + " bytes given";
    if (lengths[r] > kQualLengthMax) return "length: read " + std::to_string(r) + " has over 2^24 letters";
  }
  return std::string();
}

inline uint32_t QualScore(uint8_t byte) { return (byte < 33 ? 33u : byte > 126 ? 126u : byte) - 33u; }
inline bool QualByteBad(uint8_t byte) { return byte < 33 || byte > 126; }

// The counters of a pass besides launches, reads, letters and the time: what
// the reads add up to. A read left empty (crossing ends, or the floor) counts
// all its letters as trimmed3, so trimmed5 + trimmed3 + the kept letters =
// letters.
struct QualSums {
  uint64_t trimmed5 = 0, trimmed3 = 0, masked = 0, failed = 0, bad = 0;
};
inline void QualAdd(QualSums *s, uint32_t n, uint32_t min_len, const GhostmQualOut &o) {
  s->trimmed5 += o.kept ? o.begin : 0;
  s->trimmed3 += o.kept ? n - o.begin - o.kept : n;
  s->masked += o.masked;
  s->failed += o.kept < min_len;  // after the floor kept is 0 or at least min_len
  s->bad += o.bad;
}

// One read, letter by letter, straight from the definition; masks in place.
inline GhostmQualOut QualTrimRead(uint8_t *letters, const uint8_t *qual, uint32_t n, const QualParams &p) {
  GhostmQualOut o{0, 0, 0, 0};
  for (uint32_t i = 0; i < n; ++i) o.bad += QualByteBad(qual[i]);
  uint32_t end = n, begin = 0;
  {
    int64_t s = 0, best = 0;
    for (uint32_t i = n; i-- > 0;) {
      s += (int64_t)p.trim_q - (int64_t)QualScore(qual[i]);
      if (s < 0) break;
      if (s > best) best = s, end = i;
    }
  }
  {
    int64_t s = 0, best = 0;
    for (uint32_t i = 0; i < n; ++i) {
      s += (int64_t)p.trim_q - (int64_t)QualScore(qual[i]);
      if (s < 0) break;
      if (s > best) best = s, begin = i + 1;
    }
  }
  if (end > begin) o.begin = begin, o.kept = end - begin;
  if (o.kept < p.min_len) {
    o.begin = o.kept = 0;
    return o;
  }
  for (uint32_t i = o.begin; i < o.begin + o.kept; ++i) {
    if (QualScore(qual[i]) >= p.mask_q) continue;
    letters[i] = 'N';
    ++o.masked;
  }
  return o;
}

// The five sums of a pass are kept in kQualCounterSlots slots of
// kQualCounterWords 64-bit words (a cache line each; words 0..4 used: trimmed5,
// trimmed3, masked, failed, bad), a wave adding its sums to the slot of its
// number, as the mask pass does. The caller adds the slots up.
constexpr uint32_t kQualCounterSlots = 128, kQualCounterWords = 16;
// the launch: four waves to a block, at most this many blocks, the waves striding over the reads
constexpr uint32_t kQualBlocksMax = 1024;

// Launches k_qual_trim (read_quality.hip) on the caller's stream: n reads,
// read r = len[r] bytes at off[r] of d_letters and of d_qual; d_out = n records,
// d_counters = the counter slots, zero on entry. The caller has made
// ValidateQuality's checks.
void LaunchQualityTrim(void *stream, uint8_t *d_letters, const uint8_t *d_qual, const uint64_t *d_off,
                       const uint32_t *d_len, uint32_t n, const QualParams &p, GhostmQualOut *d_out,
                       uint64_t *d_counters);

}  // namespace ghostm
