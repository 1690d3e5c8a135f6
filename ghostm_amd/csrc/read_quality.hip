// read_quality.hip — the quality stage of a read set on the GPU
// (DeviceModule::QualityTrim; the rule: read_quality.h and include/ghostm_hip.h;
// the host model: read_quality_host.cpp).
//   k_qual_trim  one wave per read (grid-stride), 64 positions at a time. Each
//                end is walked inwards: lane t of group g holds the score of the
//                (64 g + t)-th position from that end, the running sum is a wave
//                prefix scan (six __shfl_up steps) on top of the sum carried from
//                the group before, the stop is the lowest bit of the ballot
//                "sum < 0", and the group's candidate is the first lane of the
//                greatest sum among the lanes before the stop (a butterfly max,
//                then a ballot). The carried best is replaced only by a greater
//                sum, so the first position walked wins a tie. The wave leaves
//                the walk at the stop. One more pass over the whole read counts
//                the bytes outside '!'..'~' and stores 'N' over the kept letters
//                below mask_q; it runs whatever the walks found, since a bad
//                byte refuses a set. Every load and store is a byte at
//                off + i with i < len: nothing beside the read is touched.
//                The five sums are kept per wave and added to one of 128 slots.
// No LDS is used (everything lives in registers and ballots), so there is
// nothing for the LDS-poison build to fill: the file is compiled into that
// library unchanged.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ghostm_hip.h"
#include "common.h"
#include "read_quality.h"

namespace ghostm {

namespace {

#define RQ_CHECK(expr)                                                                   \
  do {                                                                                   \
    hipError_t err_ = (expr);                                                            \
    if (err_ != hipSuccess)                                                              \
      throw Error(std::string("HIP error '") + hipGetErrorString(err_) + "' at " #expr); \
  } while (0)

constexpr uint32_t kQualBlock = 256, kQualWaves = kQualBlock / 64;

struct QualArgs {
  uint8_t *letters;
  const uint8_t *qual;
  const uint64_t *off;
  const uint32_t *len;
  GhostmQualOut *out;
  unsigned long long *counters;  // kQualCounterSlots slots: trimmed5, trimmed3, masked, failed, bad
  uint32_t n, trim_q, mask_q, min_len;
};

__device__ __forceinline__ int QualScoreDev(uint32_t byte) { return (int)min(max(byte, 33u), 126u) - 33; }

// The walk from one end of a read of n scores at q: from the 3' end (position
// n - 1 - k is the k-th walked) or the 5' end (position k). Returns the k of the
// position where the running sum first reached its greatest value above 0, or
// n when there is none.
__device__ __forceinline__ uint32_t QualWalk(const uint8_t *q, uint32_t n, int trim_q, bool from_end, uint32_t lane) {
  int carry = 0, best = 0;
  uint32_t best_k = n;
  for (uint32_t k0 = 0; k0 < n; k0 += 64) {
    const uint32_t k = k0 + lane;
    const bool valid = k < n;
    int s = valid ? trim_q - QualScoreDev(q[from_end ? n - 1 - k : k]) : 0;
    for (uint32_t d = 1; d < 64; d <<= 1) {  // inclusive prefix sum over the lanes
      const int up = __shfl_up(s, d);
      if (lane >= d) s += up;
    }
    s += carry;
    const unsigned long long stop = __ballot(valid && s < 0);
    const uint32_t stop_lane = stop ? (uint32_t)__ffsll((long long)stop) - 1 : 64u;
    const bool walked = valid && lane < stop_lane;
    int top = walked ? s : 0;  // every walked sum is at least 0
    for (uint32_t d = 32; d; d >>= 1) top = max(top, __shfl_xor(top, d));
    if (top > best) {  // uniform: top and best are the same in every lane
      const unsigned long long at = __ballot(walked && s == top);
      best = top;
      best_k = k0 + (uint32_t)__ffsll((long long)at) - 1;
    }
    if (stop) break;
    carry = __shfl(s, 63);
  }
  return best_k;
}

__global__ __launch_bounds__(kQualBlock) void k_qual_trim(QualArgs a) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  unsigned long long w5 = 0, w3 = 0, wmask = 0, wfail = 0, wbad = 0;
  for (uint32_t r = blockIdx.x * kQualWaves + wv; r < a.n; r += gridDim.x * kQualWaves) {
    const uint32_t n = a.len[r];
    const uint8_t *q = a.qual + a.off[r];
    uint8_t *letters = a.letters + a.off[r];
    uint32_t end = n, begin = 0;
    if (a.trim_q) {  // with trim_q 0 no sum rises above 0
      const uint32_t k3 = QualWalk(q, n, (int)a.trim_q, true, lane);
      const uint32_t k5 = QualWalk(q, n, (int)a.trim_q, false, lane);
      if (k3 < n) end = n - 1 - k3;
      if (k5 < n) begin = k5 + 1;
    }
    uint32_t kept = end > begin ? end - begin : 0u;
    if (kept == 0) begin = 0;
    const bool failed = kept < a.min_len;
    if (failed) kept = 0, begin = 0;
    uint32_t masked = 0, bad = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 64) {
      const uint32_t i = i0 + lane;
      const uint32_t byte = i < n ? q[i] : 33u;
      bad += (uint32_t)__popcll(__ballot(byte < 33u || byte > 126u));
      const bool hide = i >= begin && i - begin < kept && (uint32_t)QualScoreDev(byte) < a.mask_q;
      if (hide) letters[i] = (uint8_t)'N';
      masked += (uint32_t)__popcll(__ballot(hide));
    }
    if (lane == 0) a.out[r] = GhostmQualOut{begin, kept, masked, bad};
    w5 += kept ? begin : 0u;
    w3 += kept ? n - begin - kept : n;
    wmask += masked;
    wfail += failed;
    wbad += bad;
  }
  if (lane == 0 && (w5 | w3 | wmask | wfail | wbad)) {
    unsigned long long *slot = a.counters + (size_t)((blockIdx.x * kQualWaves + wv) % kQualCounterSlots) * kQualCounterWords;
    if (w5) atomicAdd(&slot[0], w5);
    if (w3) atomicAdd(&slot[1], w3);
    if (wmask) atomicAdd(&slot[2], wmask);
    if (wfail) atomicAdd(&slot[3], wfail);
    if (wbad) atomicAdd(&slot[4], wbad);
  }
}

}  // namespace

void LaunchQualityTrim(void *stream, uint8_t *d_letters, const uint8_t *d_qual, const uint64_t *d_off,
                       const uint32_t *d_len, uint32_t n, const QualParams &p, GhostmQualOut *d_out,
                       uint64_t *d_counters) {
  if (n == 0) return;
  QualArgs a{};
  a.letters = d_letters;
  a.qual = d_qual;
  a.off = d_off;
  a.len = d_len;
  a.out = d_out;
  a.counters = reinterpret_cast<unsigned long long *>(d_counters);
  a.n = n;
  a.trim_q = p.trim_q;
  a.mask_q = p.mask_q;
  a.min_len = p.min_len;
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n + kQualWaves - 1) / kQualWaves, kQualBlocksMax);
  hipLaunchKernelGGL(k_qual_trim, dim3(blocks), dim3(kQualBlock), 0, static_cast<hipStream_t>(stream), a);
  RQ_CHECK(hipGetLastError());
}

}  // namespace ghostm
