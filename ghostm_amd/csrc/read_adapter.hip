// read_adapter.hip — the adapter stage of a read set on the GPU
// (DeviceModule::AdapterTrim; the rule: read_adapter.h and include/ghostm_hip.h;
// the host model: read_adapter_host.cpp). The letters are packed on the fly
// into three bit planes (the two bits of the code A C G T = 0..3, and "none of
// these"), 64 letters to a 64-bit word made by three ballots, and mismatches
// are counted 64 letters at a time: (lo ^ lo') | (hi ^ hi') | other, masked to
// the compared length, then one popcount.
//   k_adapter_find  one wave per read (grid-stride). The lanes own 64
//                   consecutive starts at a time, from the 5' end. The group's
//                   window of 64 + m - 1 letters is two plane words, this
//                   group's and the next one's (each letter is loaded once, one
//                   byte per lane); lane t's window is their funnel shift by t.
//                   The adapter's planes and its N mask come as arguments. A
//                   lane is accepted when L >= min_overlap and mm * 100 <=
//                   err_pct * L; the group's result is the lowest bit of the
//                   ballot, and the wave leaves at the first group with one.
//   k_pair_overlap  one wave per pair (grid-stride). Both mates are staged once
//                   as plane words, lane c holding word c of mate 1 and of the
//                   reverse complement Q of mate 2 (Q[k] = complement of
//                   R2[n2 - 1 - k]), so pm(f) = the i < f with R1[i] != Q[n2 -
//                   f + i]. The lanes own 64 fragment lengths at a time, lane t
//                   of group g top - 64 g - t, from top = min(n1, n2)
//                   downwards; per 64 letters a lane takes mate 1's word by a
//                   broadcast and its own shifted window of Q by two lane
//                   shuffles per plane. A group stops counting once every lane
//                   is over its budget err_pct * f / 100; the first group with
//                   an accepted lane ends the walk and its lowest lane holds the
//                   greatest f. It then sets kept in both mates' records.
// Every load is a byte at off + i with i < len: nothing beside the read is
// touched, and the letters are never written. The six sums are kept per wave
// and added to one of 128 slots, by the kernel that runs last.
// No LDS is used (the planes live in registers, ballots and lane shuffles), so
// there is nothing for the LDS-poison build to fill: the file is compiled into
// that library unchanged.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ghostm_hip.h"
#include "common.h"
#include "read_adapter.h"

namespace ghostm {

namespace {

#define RA_CHECK(expr)                                                                   \
  do {                                                                                   \
    hipError_t err_ = (expr);                                                            \
    if (err_ != hipSuccess)                                                              \
      throw Error(std::string("HIP error '") + hipGetErrorString(err_) + "' at " #expr); \
  } while (0)

constexpr uint32_t kAdapterBlock = 256, kAdapterWaves = kAdapterBlock / 64;
typedef unsigned long long Word;

struct AdapterArgs {
  const uint8_t *letters;
  const uint64_t *off;
  const uint32_t *len;
  GhostmAdapterOut *out;
  unsigned long long *counters;  // kAdapterCounterSlots slots: cut_reads, cut_letters, adapter_found, pair_found, pair_skipped, emptied
  uint32_t n, min_overlap, err_pct, pair_overlap;
  uint32_t m[2];                 // the adapters' letters; m[1] == 0: adapter 0 for every record
  Word lo[2], hi[2], any[2];     // their planes; any: the N's
};

__device__ __forceinline__ uint32_t AdapterCodeDev(uint32_t byte) {
  if (byte - (uint32_t)'a' < 26u) byte -= 32u;
  return byte == 'A' ? 0u : byte == 'C' ? 1u : byte == 'G' ? 2u : byte == 'T' ? 3u : (uint32_t)kAdapterOther;
}

struct Planes {
  Word lo, hi, other;
};

// the planes of 64 codes, one per lane
__device__ __forceinline__ Planes PlanesOf(uint32_t code) {
  Planes p;
  p.lo = __ballot(code & 1u);
  p.hi = __ballot(code & 2u);
  p.other = __ballot(code == (uint32_t)kAdapterOther);
  return p;
}

// bits s.. of the 128-bit word (b : a), s in 0..63
__device__ __forceinline__ Word Funnel(Word a, Word b, uint32_t s) { return s ? (a >> s) | (b << (64u - s)) : a; }

__device__ __forceinline__ Word LowBits(uint32_t count) { return count >= 64u ? ~0ull : (1ull << count) - 1ull; }

__device__ __forceinline__ Word Shfl64(Word v, uint32_t from) {
  const uint32_t lo = __shfl((uint32_t)v, (int)from), hi = __shfl((uint32_t)(v >> 32), (int)from);
  return (Word)hi << 32 | lo;
}

__device__ __forceinline__ GhostmAdapterOut AdapterResultDev(uint32_t n, uint32_t at, uint32_t mm, uint32_t pair_len,
                                                             uint32_t pair_mm) {
  const uint32_t by_pair = pair_len ? pair_len : n;
  GhostmAdapterOut o;
  o.kept = min(at, by_pair);
  o.adapter_at = at;
  o.pair_len = pair_len;
  o.adapter_mismatches = (uint16_t)mm;
  o.pair_mismatches = (uint16_t)pair_mm;
  return o;
}

struct WaveSums {
  unsigned long long cut_reads = 0, cut_letters = 0, adapter_found = 0, pair_found = 0, pair_skipped = 0, emptied = 0;
  __device__ __forceinline__ void Add(uint32_t n, const GhostmAdapterOut &o) {
    cut_reads += o.kept < n;
    cut_letters += n - o.kept;
    adapter_found += o.adapter_at < n;
    emptied += n && !o.kept;
  }
  __device__ __forceinline__ void Store(unsigned long long *counters, uint32_t wave) const {
    if (!(cut_reads | cut_letters | adapter_found | pair_found | pair_skipped | emptied)) return;
    unsigned long long *slot = counters + (size_t)(wave % kAdapterCounterSlots) * kAdapterCounterWords;
    if (cut_reads) atomicAdd(&slot[0], cut_reads);
    if (cut_letters) atomicAdd(&slot[1], cut_letters);
    if (adapter_found) atomicAdd(&slot[2], adapter_found);
    if (pair_found) atomicAdd(&slot[3], pair_found);
    if (pair_skipped) atomicAdd(&slot[4], pair_skipped);
    if (emptied) atomicAdd(&slot[5], emptied);
  }
};

__global__ __launch_bounds__(kAdapterBlock) void k_adapter_find(AdapterArgs a) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  WaveSums sums;
  for (uint32_t r = blockIdx.x * kAdapterWaves + wv; r < a.n; r += gridDim.x * kAdapterWaves) {
    const uint32_t n = a.len[r];
    const uint8_t *read = a.letters + a.off[r];
    const uint32_t sel = (r & 1u) && a.m[1] ? 1u : 0u;
    const uint32_t m = a.m[sel];
    const Word alo = a.lo[sel], ahi = a.hi[sel], care = ~a.any[sel];
    uint32_t at = n, mm_at = 0;
    if (m && n >= a.min_overlap) {
      Planes cur = PlanesOf(lane < n ? AdapterCodeDev(read[lane]) : (uint32_t)kAdapterOther);
      // a start p has L >= min_overlap only while p + min_overlap <= n
      for (uint32_t p0 = 0; p0 + a.min_overlap <= n; p0 += 64) {
        const uint32_t i = p0 + 64 + lane;  // below 2^24 + 128
        const Planes next = PlanesOf(i < n ? AdapterCodeDev(read[i]) : (uint32_t)kAdapterOther);
        const uint32_t p = p0 + lane;
        const uint32_t L = p < n ? min(m, n - p) : 0u;
        const Word diff = (Funnel(cur.lo, next.lo, lane) ^ alo) | (Funnel(cur.hi, next.hi, lane) ^ ahi) |
                          Funnel(cur.other, next.other, lane);
        const uint32_t mm = (uint32_t)__popcll(diff & care & LowBits(L));
        const Word ok = __ballot(L >= a.min_overlap && mm * 100u <= a.err_pct * L);
        if (ok) {
          const uint32_t first = (uint32_t)__ffsll((long long)ok) - 1;
          at = p0 + first;
          mm_at = (uint32_t)__shfl((int)mm, (int)first);
          break;
        }
        cur = next;
      }
    }
    const GhostmAdapterOut o = AdapterResultDev(n, at, mm_at, 0, 0);
    if (lane == 0) a.out[r] = o;
    if (!a.pair_overlap) sums.Add(n, o);  // else k_pair_overlap counts
  }
  if (lane == 0) sums.Store(a.counters, blockIdx.x * kAdapterWaves + wv);
}

__global__ __launch_bounds__(kAdapterBlock) void k_pair_overlap(AdapterArgs a) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t npairs = a.n / 2;
  const bool have_adapter = a.m[0] || a.m[1];
  WaveSums sums;
  for (uint32_t pr = blockIdx.x * kAdapterWaves + wv; pr < npairs; pr += gridDim.x * kAdapterWaves) {
    const uint32_t e = pr * 2;
    const uint32_t n1 = a.len[e], n2 = a.len[e + 1];
    const uint8_t *r1 = a.letters + a.off[e], *r2 = a.letters + a.off[e + 1];
    const uint32_t top = min(n1, n2);
    const bool skipped = n1 > kAdapterPairLettersMax || n2 > kAdapterPairLettersMax;
    uint32_t pair_len = 0, pair_mm = 0;
    if (!skipped && top >= a.pair_overlap) {
      // lane c: word c of mate 1 and of Q; the words behind a mate's end say "other"
      Planes x{0, 0, ~0ull}, q{0, 0, ~0ull};
      for (uint32_t c = 0; c * 64 < n1; ++c) {
        const uint32_t i = c * 64 + lane;
        const Planes w = PlanesOf(i < n1 ? AdapterCodeDev(r1[i]) : (uint32_t)kAdapterOther);
        if (lane == c) x = w;
      }
      for (uint32_t c = 0; c * 64 < n2; ++c) {
        const uint32_t k = c * 64 + lane;
        const uint32_t code = k < n2 ? AdapterCodeDev(r2[n2 - 1 - k]) : (uint32_t)kAdapterOther;
        const Planes w = PlanesOf(code < 4u ? 3u - code : code);
        if (lane == c) q = w;
      }
      for (uint32_t g0 = 0; g0 + a.pair_overlap <= top; g0 += 64) {
        const uint32_t fmax = top - g0;                           // lane 0's f
        const bool valid = g0 + lane + a.pair_overlap <= top;      // f >= pair_overlap
        const uint32_t f = valid ? fmax - lane : 0u;
        const uint32_t budget = a.err_pct * f / 100u;  // pm * 100 <= err_pct * f
        const uint32_t base = n2 - f;                  // Q's offset of R1[0]
        uint32_t pm = 0;
        for (uint32_t c = 0; c * 64 < fmax; ++c) {
          const Word xlo = Shfl64(x.lo, c), xhi = Shfl64(x.hi, c), xother = Shfl64(x.other, c);
          const uint32_t o = base + c * 64, w = (o >> 6) & 63u, s = o & 63u;  // letters at o < n2 <= 1024: w <= 15
          const Word qlo = Funnel(Shfl64(q.lo, w), Shfl64(q.lo, w + 1), s);
          const Word qhi = Funnel(Shfl64(q.hi, w), Shfl64(q.hi, w + 1), s);
          const Word qother = Funnel(Shfl64(q.other, w), Shfl64(q.other, w + 1), s);
          const uint32_t count = f > c * 64 ? f - c * 64 : 0u;
          pm += (uint32_t)__popcll(((xlo ^ qlo) | (xhi ^ qhi) | xother | qother) & LowBits(count));
          if (!__ballot(valid && pm <= budget)) break;  // every lane is over its budget
        }
        const Word ok = __ballot(valid && pm <= budget);
        if (ok) {
          const uint32_t first = (uint32_t)__ffsll((long long)ok) - 1;
          pair_len = fmax - first;
          pair_mm = (uint32_t)__shfl((int)pm, (int)first);
          break;
        }
      }
    }
    for (uint32_t k = 0; k < 2; ++k) {
      const uint32_t n = k ? n2 : n1;
      const uint32_t at = have_adapter ? a.out[e + k].adapter_at : n;
      const uint32_t mm = have_adapter ? a.out[e + k].adapter_mismatches : 0u;
      const GhostmAdapterOut o = AdapterResultDev(n, at, mm, pair_len, pair_mm);
      if (lane == 0) a.out[e + k] = o;
      sums.Add(n, o);
    }
    sums.pair_found += pair_len != 0;
    sums.pair_skipped += skipped;
  }
  if (lane == 0) sums.Store(a.counters, blockIdx.x * kAdapterWaves + wv);
}

void PlanesOfAdapter(const uint8_t *codes, uint32_t m, Word *lo, Word *hi, Word *any) {
  *lo = *hi = *any = 0;
  for (uint32_t i = 0; i < m; ++i) {
    if (codes[i] == kAdapterAny) *any |= 1ull << i;
    else *lo |= (Word)(codes[i] & 1u) << i, *hi |= (Word)(codes[i] >> 1 & 1u) << i;
  }
}

}  // namespace

uint32_t LaunchAdapterTrim(void *stream, const uint8_t *d_letters, const uint64_t *d_off, const uint32_t *d_len,
                           uint32_t n, const AdapterParams &p, GhostmAdapterOut *d_out, uint64_t *d_counters) {
  if (n == 0) return 0;
  AdapterArgs a{};
  a.letters = d_letters;
  a.off = d_off;
  a.len = d_len;
  a.out = d_out;
  a.counters = reinterpret_cast<unsigned long long *>(d_counters);
  a.n = n;
  a.min_overlap = p.min_overlap;
  a.err_pct = p.err_pct;
  a.pair_overlap = p.pair_overlap;
  a.m[0] = p.m1;
  a.m[1] = p.m2;
  PlanesOfAdapter(p.a1, p.m1, &a.lo[0], &a.hi[0], &a.any[0]);
  PlanesOfAdapter(p.a2, p.m2, &a.lo[1], &a.hi[1], &a.any[1]);
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint32_t launches = 0;
  if (p.m1 || p.m2) {
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n + kAdapterWaves - 1) / kAdapterWaves, kAdapterBlocksMax);
    hipLaunchKernelGGL(k_adapter_find, dim3(blocks), dim3(kAdapterBlock), 0, st, a);
    RA_CHECK(hipGetLastError());
    ++launches;
  }
  if (p.pair_overlap) {
    const uint32_t pairs = n / 2;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)pairs + kAdapterWaves - 1) / kAdapterWaves, kAdapterBlocksMax);
    hipLaunchKernelGGL(k_pair_overlap, dim3(blocks), dim3(kAdapterBlock), 0, st, a);
    RA_CHECK(hipGetLastError());
    ++launches;
  }
  return launches;
}

}  // namespace ghostm
