// query_mask.hip — the low-complexity mask of a resident query chunk on the GPU
// (DeviceModule::MaskQuery; the rule: query_mask.h and include/ghostm_hip.h; the
// host model: query_mask_host.cpp). Two kernels, so that every window sees the
// unmasked letters: the first only reads the records, the second only writes
// them.
//   k_mask_windows  one wave per source (grid-stride), 64 windows at a time: the
//                   group's 64 + w - 1 codes are staged once in LDS through the
//                   tile addressing; lane t walks window 64 g + t with its
//                   letter counts in LDS bytes of its own (four to a word, the
//                   words lane-interleaved), adding D[count so far] per letter
//                   (D[r] = T[r + 1] - T[r], so the sum is the sum of T[count]
//                   with no pass over a count table). The low and the trigger
//                   ballot go to the source's flag words.
//   k_mask_apply    one wave per source, lane k owning flag word 64 c + k of
//                   chunk c. A word's low bits reached from a seed are a carry
//                   chain: fill(L, s) = (((L + s) ^ L) & L) | s. A word hands
//                   the carry on when its last bit fills (generate) or when it
//                   is all low (propagate), and two ballots resolve 64 words'
//                   carries at once. Backward over the chunks from the
//                   triggers, then forward from what that reached: a trigger
//                   reaches both ends of its run however many words it spans.
//                   The segment windows widened by w - 1 letters are the
//                   masked letters; every word that has any is stored, 64
//                   letters at a time, into every tile record that covers them,
//                   and counted per record. The pass's two counters are summed
//                   per wave and added to one of 128 slots.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ghostm_hip.h"
#include "common.h"
#include "lds_poison.h"
#include "query_mask.h"

namespace ghostm {

namespace {

#define QM_CHECK(expr)                                                                   \
  do {                                                                                   \
    hipError_t err_ = (expr);                                                            \
    if (err_ != hipSuccess)                                                              \
      throw Error(std::string("HIP error '") + hipGetErrorString(err_) + "' at " #expr); \
  } while (0)

constexpr uint32_t kMaskBlock = 256, kMaskWaves = kMaskBlock / 64;
constexpr uint32_t kMaskStage = 64 + kMaskWindowMax;  // a group's codes: 64 + w - 1 of them
constexpr uint32_t kMaskCountWords = 6;               // codes 0..22 and "no letter" (23): 24 byte counts, four to a word

struct MaskArgs {
  uint8_t *seq;
  const GhostmBandSource *src;
  const uint32_t *word_off;
  unsigned long long *low, *trig;
  uint32_t *masked;
  unsigned long long *counters;  // kMaskCounterSlots slots: word 0 masked sources, word 1 masked source letters
  uint32_t nsrc, W, step, w;
  uint32_t low_at, trigger_at;  // extend * 1024 * w, trigger * 1024 * w
  uint32_t Tw;                  // T[w]
  uint32_t D[kMaskWindowMax];   // D[r] = T[r + 1] - T[r]
};

__device__ __forceinline__ void WaveSync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// BandLetterAt (band_align.h) for the device
__device__ __forceinline__ size_t MaskLetterAt(const GhostmBandSource &s, uint32_t p, uint32_t W, uint32_t step) {
  const uint32_t t = min(p / step, s.tiles - 1);
  const uint32_t start = t + 1 < s.tiles ? t * step : (s.letters > W ? s.letters - W : 0u);
  const uint32_t rec = s.first_record + (s.tiles > 1 ? s.stride * t : 0u);
  return (size_t)rec * W + (p - start);
}

__global__ __launch_bounds__(kMaskBlock) void k_mask_windows(MaskArgs a) {
  __shared__ uint32_t s_D[kMaskWindowMax];
  __shared__ uint8_t s_code[kMaskWaves][kMaskStage];
  __shared__ uint32_t s_count[kMaskWaves][kMaskCountWords * 64];
  GHOSTM_POISON_LDS();
  if (threadIdx.x < kMaskWindowMax) s_D[threadIdx.x] = a.D[threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, w = a.w;
  uint8_t *code = s_code[wv];
  uint32_t *count = s_count[wv];
  for (uint32_t h = blockIdx.x * kMaskWaves + wv; h < a.nsrc; h += gridDim.x * kMaskWaves) {
    const GhostmBandSource S = a.src[h];
    const uint32_t m = S.letters;
    if (m < w) continue;
    const uint32_t nw = m - w + 1, words = (nw + 63) / 64;
    const uint32_t off = a.word_off[h];
    for (uint32_t g = 0; g < words; ++g) {
      const uint32_t p0 = g * 64;
      WaveSync();  // the last group's windows have read their codes
      {
        const uint32_t p = p0 + lane;
        code[lane] = p < m ? a.seq[MaskLetterAt(S, p, a.W, a.step)] : (uint8_t)kBaseX;
      }
      if (lane + 1 < w) {
        const uint32_t p = p0 + 64 + lane;
        code[64 + lane] = p < m ? a.seq[MaskLetterAt(S, p, a.W, a.step)] : (uint8_t)kBaseX;
      }
      for (uint32_t k = 0; k < kMaskCountWords; ++k) count[k * 64 + lane] = 0;
      WaveSync();
      uint32_t sum = 0;
      bool letters = true;
      for (uint32_t j = 0; j < w; ++j) {
        const uint32_t c = code[lane + j];
        letters = letters && c < kBaseX;
        const uint32_t row = min(c, (uint32_t)kBaseX), sh = (row & 3) * 8;
        const uint32_t v = count[(row >> 2) * 64 + lane];
        sum += s_D[(v >> sh) & 0xFFu];  // at most w - 1 earlier equal letters
        count[(row >> 2) * 64 + lane] = v + (1u << sh);
      }
      // a window with an X or a '*' is not evaluated (its sum is then no sum of T's)
      const bool evaluated = letters && p0 + lane < nw;
      const uint32_t d = 100u * (a.Tw - sum);
      const unsigned long long lowm = __ballot(evaluated && d <= a.low_at);
      const unsigned long long trigm = __ballot(evaluated && d <= a.trigger_at);
      if (lane == 0) {
        a.low[off + g] = lowm;
        a.trig[off + g] = trigm;
      }
    }
  }
}

// the bits of L reached from the seeds (a subset of L) towards the higher bits through set bits of L
__device__ __forceinline__ unsigned long long MaskFill(unsigned long long L, unsigned long long seeds) {
  return (((L + seeds) ^ L) & L) | seeds;
}

// The carry into position pos (0..64) of 64 words in carry order: G = the words
// that hand a carry on whatever comes in, P = the words that hand on what comes
// in, cin0 = the carry into position 0.
__device__ __forceinline__ bool MaskCarryIn(unsigned long long G, unsigned long long P, uint32_t pos, bool cin0) {
  const unsigned long long below = pos >= 64 ? ~0ull : (1ull << pos) - 1;
  const unsigned long long stops = ~P & below;
  if (!stops) return cin0 || (G & below);
  const uint32_t j = 63u - (uint32_t)__clzll(stops);  // the last word below pos that stops a carry: it may make one
  return (G & below & ~((1ull << j) - 1)) != 0;
}

__device__ __forceinline__ unsigned long long MaskShfl(unsigned long long v, uint32_t from) {
  const uint32_t lo = __shfl((uint32_t)v, (int)from), hi = __shfl((uint32_t)(v >> 32), (int)from);
  return (unsigned long long)hi << 32 | lo;
}

// Letters 64 k .. 64 k + 63 of a source, those of bits: X into every tile record
// that covers them, the records' counts; returns the letters.
__device__ __forceinline__ uint32_t MaskStoreWord(const MaskArgs &a, const GhostmBandSource &S, uint32_t k,
                                                  unsigned long long bits, uint32_t lane) {
  const uint32_t W = a.W, step = a.step, m = S.letters, t0 = k * 64, p = t0 + lane;
  const bool mine = ((bits >> lane) & 1ull) && p < m;
  auto put_tile = [&](uint32_t t, uint32_t st) {
    const uint32_t rel = p - st;  // wraps below the tile's start
    const bool in = mine && p >= st && rel < W;
    const size_t rec = S.first_record + (S.tiles > 1 ? (size_t)S.stride * t : 0);
    if (in) a.seq[rec * W + rel] = (uint8_t)kBaseX;
    const unsigned long long inm = __ballot(in);
    if (lane == 0 && inm) atomicAdd(&a.masked[rec], (uint32_t)__popcll(inm));
  };
  // the regular tiles (start tt * step) with start + W > t0 and start < t0 + 64, then the flush-right one
  const uint32_t lo = t0 >= W ? (t0 - W) / step + 1 : 0u;
  const uint32_t hi = (uint32_t)min((unsigned long long)(S.tiles - 1), ((unsigned long long)t0 + 64 + step - 1) / step);
  for (uint32_t tt = lo; tt < hi; ++tt) put_tile(tt, tt * step);
  const uint32_t last_start = m > W ? m - W : 0u;
  if (last_start < (unsigned long long)t0 + 64 && (unsigned long long)last_start + W > t0) put_tile(S.tiles - 1, last_start);
  return (uint32_t)__popcll(__ballot(mine));
}

__global__ __launch_bounds__(kMaskBlock) void k_mask_apply(MaskArgs a) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6, w = a.w;
  uint32_t wave_sources = 0;
  unsigned long long wave_letters = 0;  // of this wave's masked sources
  for (uint32_t h = blockIdx.x * kMaskWaves + wv; h < a.nsrc; h += gridDim.x * kMaskWaves) {
    const GhostmBandSource S = a.src[h];
    const uint32_t m = S.letters;
    if (m < w) continue;
    const uint32_t nw = m - w + 1, words = (nw + 63) / 64;
    const unsigned long long *low = a.low + a.word_off[h];
    unsigned long long *reach = a.trig + a.word_off[h];  // the triggers, then what they reach backward
    // backward: the carry runs from the last word to the first, lane 63 of a chunk first (position 63 - lane)
    bool carry = false;
    for (uint32_t c = (words + 63) / 64; c-- > 0;) {
      const uint32_t k = c * 64 + lane;
      const unsigned long long L = k < words ? low[k] : 0ull, T = k < words ? reach[k] : 0ull;
      const unsigned long long Lr = __brevll(L), Tr = __brevll(T) & Lr;
      const unsigned long long G = __brevll(__ballot((MaskFill(Lr, Tr) >> 63) != 0)), P = __brevll(__ballot(L == ~0ull));
      const bool cin = MaskCarryIn(G, P, 63 - lane, carry);
      if (k < words) reach[k] = __brevll(MaskFill(Lr, Tr | ((unsigned long long)cin & Lr)));  // by the lane that reads it below
      carry = MaskCarryIn(G, P, 64, carry);
    }
    // forward from there, one word past the last: the last windows' letters spill into it
    carry = false;
    unsigned long long seg_before = 0;  // the segment windows of the word before this chunk
    uint32_t total = 0;
    for (uint32_t c = 0; c < (words + 1 + 63) / 64; ++c) {
      const uint32_t k = c * 64 + lane;
      const unsigned long long L = k < words ? low[k] : 0ull, R = k < words ? reach[k] : 0ull;
      const unsigned long long G = __ballot((MaskFill(L, R) >> 63) != 0), P = __ballot(L == ~0ull);
      const bool cin = MaskCarryIn(G, P, lane, carry);
      const unsigned long long seg = MaskFill(L, R | ((unsigned long long)cin & L));
      carry = MaskCarryIn(G, P, 64, carry);
      unsigned long long below = MaskShfl(seg, lane ? lane - 1 : 0);
      if (lane == 0) below = seg_before;
      seg_before = MaskShfl(seg, 63);
      // window i masks letters i .. i + w - 1
      unsigned long long letters = seg;
      for (uint32_t j = 1; j < w; ++j) letters |= seg << j | below >> (64 - j);
      for (unsigned long long todo = __ballot(letters != 0); todo; todo &= todo - 1) {
        const uint32_t l = (uint32_t)__ffsll((long long)todo) - 1;
        total += MaskStoreWord(a, S, c * 64 + l, MaskShfl(letters, l), lane);
      }
    }
    wave_sources += total != 0;
    wave_letters += total;
  }
  if (lane == 0 && wave_sources) {
    unsigned long long *slot = a.counters + (size_t)((blockIdx.x * kMaskWaves + wv) % kMaskCounterSlots) * kMaskCounterWords;
    atomicAdd(&slot[0], (unsigned long long)wave_sources);
    atomicAdd(&slot[1], wave_letters);
  }
}

}  // namespace

void LaunchQueryMask(void *stream, uint8_t *d_seq, uint32_t W, const GhostmBandSource *d_src,
                     const uint32_t *d_word_off, uint32_t nsrc, uint32_t step, const MaskParams &p,
                     uint64_t *d_low, uint64_t *d_trig, uint32_t *d_masked, uint64_t *d_counters) {
  if (nsrc == 0) return;
  const MaskTable tab = MakeMaskTable();
  MaskArgs a{};
  a.seq = d_seq;
  a.src = d_src;
  a.word_off = d_word_off;
  a.low = reinterpret_cast<unsigned long long *>(d_low);
  a.trig = reinterpret_cast<unsigned long long *>(d_trig);
  a.masked = d_masked;
  a.counters = reinterpret_cast<unsigned long long *>(d_counters);
  a.nsrc = nsrc;
  a.W = W;
  a.step = step;
  a.w = p.window;
  a.low_at = p.extend * 1024u * p.window;
  a.trigger_at = p.trigger * 1024u * p.window;
  a.Tw = tab.T[p.window];
  for (uint32_t r = 0; r < kMaskWindowMax; ++r) a.D[r] = tab.T[r + 1] - tab.T[r];
  // one wave per source, grid-stride over at most 64 K blocks
  const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)nsrc + kMaskWaves - 1) / kMaskWaves, 65536);
  hipStream_t st = static_cast<hipStream_t>(stream);
#ifdef GHOSTM_LDS_POISON
  const uint32_t v = kern::LdsPoisonPattern();
  QM_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(kern::g_lds_poison), &v, sizeof(v)));
#endif
  hipLaunchKernelGGL(k_mask_windows, dim3(blocks), dim3(kMaskBlock), 0, st, a);
  QM_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_mask_apply, dim3(blocks), dim3(kMaskBlock), 0, st, a);
  QM_CHECK(hipGetLastError());
}

}  // namespace ghostm
