// qformat.hip — the `qry` formatter's per-residue work on the GPU.
//
// Reference: QueryCreator (query_creator.cpp:191-517).
//   protein  every record's letters -> residue codes (sequence.cpp:63-87), cut at
//            or X-padded to the record width (388-423)
//   DNA      every read of the chunk cut/padded to the chunk's first read length
//            (254-255), then six frames: forward offsets 0..2 and the reverse
//            complement's 0..2 (242-279); a stop codon switches the frame to '*'
//            until the next ATG (280-312); frames '*'-padded to dna_len/3 letters,
//            then coded and cut/padded to the width like protein records
//
// The host keeps what is sequential in the file format (FASTA parsing, chunk
// cuts, names) and hands the chunk's letters over as one concatenated buffer.
//   k_qry_protein  one wave per record: coalesced reads of the record's letters,
//                  one LDS table lookup, coalesced writes (HBM-bound)
//   k_qry_frames   one wave per read, 64 letters of a frame at a time; the
//                  stop/ATG state (a scan along the frame in the reference) is
//                  the last event at or before each letter, found by ballots
// Both are templates on QLEN: the resident form (DeviceModule::FormatQuery, a
// session's query set formatted straight into its DevQuery) also takes each
// record's QueryResidues from a ballot of the non-X lanes per 64 codes, so only
// the 4-byte lengths come back; GhostmFormatQueriesGpu (qry -D) runs the same
// bodies without it.
//   k_qry_protein_tiled, k_qry_frames_tiled  the tiled forms
//                  (DeviceModule::FormatQueryTiled, query_tiles.h): a record
//                  or frame longer than the width becomes overlapping tile
//                  records; the frame is still translated once, each group of
//                  64 letters stored into every tile that covers it
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "../../include/ghostm_hip.h"
#include "common.h"
#include "formats.h"
#include "lds_poison.h"
#include "qformat.h"

namespace ghostm {

void SetLastErrorMessage(const std::string &m);

namespace {

#define QF_CHECK(expr)                                                                   \
  do {                                                                                   \
    hipError_t err_ = (expr);                                                            \
    if (err_ != hipSuccess)                                                              \
      throw Error(std::string("HIP error '") + hipGetErrorString(err_) + "' at " #expr); \
  } while (0)

constexpr uint32_t kQfBlock = 256;

// Lookup tables (one small device buffer, staged into LDS per block).
struct QfTables {
  uint8_t protein[256];  // letter -> residue code (ProteinCode)
  uint8_t dna[256];      // letter -> base code (DnaCode: A0 C1 G2 T3, '-' 5, else 4)
  uint8_t codon[128];    // 2-bit codon (first base major) -> residue code; 64 = ambiguous
};

struct QfArgs {
  const uint8_t *raw;
  const unsigned long long *off;
  const uint32_t *len;
  uint32_t nrec, width, dna_len;
  uint8_t *out;
  const QfTables *tab;
  uint32_t *qlen;  // QLEN kernels: QueryResidues of every output record
};

constexpr uint32_t kQfWaves = kQfBlock / 64;

// QueryResidues (formats.h) of a record from the wave's own codes: `last` is
// one past the last non-X code seen so far, nonx the ballot of the non-X lanes
// of the 64 codes starting at k0.
__device__ __forceinline__ uint32_t LastResidue(uint32_t last, unsigned long long nonx, uint32_t k0) {
  return nonx ? k0 + 64u - (uint32_t)__clzll(nonx) : last;
}

// One wave per record (grid-stride): lanes walk the record's letters and its
// output bytes contiguously, the code table in LDS. QLEN: the record's
// QueryResidues too (the resident form, DeviceModule::FormatQuery).
template <bool QLEN> __global__ __launch_bounds__(kQfBlock) void k_qry_protein(QfArgs a) {
  __shared__ uint8_t s_code[256];
  s_code[threadIdx.x] = a.tab->protein[threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  for (uint32_t r = blockIdx.x * kQfWaves + (threadIdx.x >> 6); r < a.nrec; r += gridDim.x * kQfWaves) {
    const uint32_t n = min(a.len[r], a.width);
    const uint8_t *src = a.raw + a.off[r];
    uint8_t *dst = a.out + (uint64_t)r * a.width;
    uint32_t last = 0;
    for (uint32_t k0 = 0; k0 < a.width; k0 += 64) {
      const uint32_t k = k0 + lane;
      const uint8_t code = k < n ? s_code[src[k]] : (uint8_t)kBaseX;
      if (k < a.width) dst[k] = code;
      if (QLEN) last = LastResidue(last, __ballot(code != kBaseX), k0);
    }
    if (QLEN && lane == 0) a.qlen[r] = max(last, 1u);
  }
}

// One wave per read (grid-stride), its six frames in turn, 64 letters at a time:
// lane t codes letter t (the codon ending at strand position o + 2 + 3t). The
// stop/ATG state of a letter is the type of the last event (ATG clears, a stop
// codon sets) at or before it, else the state carried from the previous 64
// letters: two ballots and a leading-bit search, no sequential walk.
template <bool QLEN> __global__ __launch_bounds__(kQfBlock) void k_qry_frames(QfArgs a) {
  __shared__ uint8_t s_base[256];
  __shared__ uint8_t s_codon[128];
  s_base[threadIdx.x] = a.tab->dna[threadIdx.x];
  if (threadIdx.x < 128) s_codon[threadIdx.x] = a.tab->codon[threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t n = a.dna_len;
  const uint32_t letters = n / 3;  // every frame after '*' padding
  const uint32_t keep = min(letters, a.width);
  const unsigned long long upto = ~0ull >> (63 - lane);  // lanes 0..lane
  for (uint32_t r = blockIdx.x * kQfWaves + (threadIdx.x >> 6); r < a.nrec; r += gridDim.x * kQfWaves) {
    const uint32_t rl = a.len[r];
    const uint8_t *dna = a.raw + a.off[r];
    for (uint32_t f = 0; f < 6; ++f) {
      const uint32_t s = f / 3, o = f - s * 3;
      // base at strand position j (reads shorter than dna_len are padded with 4)
      auto base = [&](uint32_t j) -> uint32_t {
        const uint32_t p = s ? n - 1 - j : j;
        uint32_t b = p < rl ? s_base[dna[p]] : 4u;
        if (s && b <= 3) b = (~b) & 3u;
        return b;
      };
      uint8_t *rec = a.out + ((uint64_t)r * 6 + f) * a.width;
      uint32_t carry = 0;  // stop state entering this group of 64 letters
      uint32_t last = 0;
      for (uint32_t t0 = 0; t0 < keep; t0 += 64) {
        const uint32_t t = t0 + lane, k = o + 2 + 3 * t;
        uint32_t code = 24, ev = 0;  // '*' padding past the last codon
        if (t < keep && k < n) {
          const uint32_t b0 = base(k - 2), b1 = base(k - 1), b2 = base(k);
          const uint32_t codon = (b0 > 3 || b1 > 3 || b2 > 3) ? 64u : (b0 << 4 | b1 << 2 | b2);
          code = s_codon[codon];
          ev = codon == 14 ? 1u : (codon == 48 || codon == 50 || codon == 56) ? 2u : 0u;  // ATG / TAA TAG TGA
        }
        const unsigned long long evm = __ballot(ev != 0), setm = __ballot(ev == 2);
        const unsigned long long mine = evm & upto;
        const uint32_t stop = mine ? (uint32_t)(setm >> (63 - __clzll(mine))) & 1u : carry;
        const uint32_t put = stop ? 24u : code;
        if (t < keep) rec[t] = (uint8_t)put;
        if (QLEN) last = LastResidue(last, __ballot(t < keep && put != kBaseX), t0);
        carry = evm ? (uint32_t)(setm >> (63 - __clzll(evm))) & 1u : carry;
      }
      for (uint32_t t = keep + lane; t < a.width; t += 64) rec[t] = kBaseX;
      if (QLEN && lane == 0) a.qlen[(uint64_t)r * 6 + f] = max(last, 1u);
    }
  }
}

// ---------------------------------------------------------------- tiled forms
// A source longer than the width becomes overlapping tiles of `width` letters
// (query_tiles.h: the plan; TileCount / TileStart restated here). Output
// record first[r] is record r's first; always with the records' QueryResidues.
struct QfTileArgs {
  const uint8_t *raw;
  const unsigned long long *off;
  const uint32_t *len;    // kept letters (nt for DNA): cut at max_len by the host
  const uint32_t *first;  // first output record of every source record
  uint32_t nrec, width, step;
  uint8_t *out;
  const QfTables *tab;
  uint32_t *qlen;
};

__device__ __forceinline__ uint32_t QfTileCount(uint32_t m, uint32_t W, uint32_t step) {
  return m <= W ? 1u : 1u + (m - W + step - 1) / step;  // no wrap: the host refused a record over 1024 tiles
}

__device__ __forceinline__ uint32_t QfTileStart(uint32_t t, uint32_t tiles, uint32_t m, uint32_t W, uint32_t step) {
  return t + 1 < tiles ? t * step : (m > W ? m - W : 0u);
}

// One wave per record (grid-stride), its tiles in turn: tile t is what
// k_qry_protein makes of letters [start, start + width), X past the record's
// end. Overlapping tiles read their letters again (cache hits); the stores
// are the tile records' contiguous bytes.
__global__ __launch_bounds__(kQfBlock) void k_qry_protein_tiled(QfTileArgs a) {
  __shared__ uint8_t s_code[256];
  GHOSTM_POISON_LDS();
  s_code[threadIdx.x] = a.tab->protein[threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, W = a.width;
  for (uint32_t r = blockIdx.x * kQfWaves + (threadIdx.x >> 6); r < a.nrec; r += gridDim.x * kQfWaves) {
    const uint32_t m = a.len[r], tiles = QfTileCount(m, W, a.step);
    const uint8_t *src = a.raw + a.off[r];
    for (uint32_t t = 0; t < tiles; ++t) {
      const uint32_t start = QfTileStart(t, tiles, m, W, a.step);
      uint8_t *dst = a.out + (uint64_t)(a.first[r] + t) * W;
      uint32_t last = 0;
      for (uint32_t k0 = 0; k0 < W; k0 += 64) {
        const uint32_t k = k0 + lane;
        const uint8_t code = (k < W && start + k < m) ? s_code[src[start + k]] : (uint8_t)kBaseX;
        if (k < W) dst[k] = code;
        last = LastResidue(last, __ballot(code != kBaseX), k0);
      }
      if (lane == 0) a.qlen[a.first[r] + t] = max(last, 1u);
    }
  }
}

// One wave per (read, frame) (grid-stride): the frame is translated once over
// its whole length (n / 3 letters of the read's own kept length n), 64 letters
// at a time as k_qry_frames does, the stop/ATG state carried along the whole
// frame. Each group of 64 letters is then stored into every tile that covers
// it: output record first[r] + 6 t + f, byte (letter - start(t)). A tile's
// QueryResidues is the group ballot masked to the tile's range; groups come in
// increasing order, so lane 0 writes the length at the tile's first group (1
// when nothing is set yet) and again whenever a later group has a non-X letter
// in the tile.
__global__ __launch_bounds__(kQfBlock) void k_qry_frames_tiled(QfTileArgs a) {
  __shared__ uint8_t s_base[256];
  __shared__ uint8_t s_codon[128];
  GHOSTM_POISON_LDS();
  s_base[threadIdx.x] = a.tab->dna[threadIdx.x];
  if (threadIdx.x < 128) s_codon[threadIdx.x] = a.tab->codon[threadIdx.x];
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63, W = a.width, step = a.step;
  const unsigned long long upto = ~0ull >> (63 - lane);  // lanes 0..lane
  const uint64_t work = (uint64_t)a.nrec * 6;
  for (uint64_t w = blockIdx.x * kQfWaves + (threadIdx.x >> 6); w < work; w += (uint64_t)gridDim.x * kQfWaves) {
    const uint32_t r = (uint32_t)(w / 6), f = (uint32_t)(w - (uint64_t)r * 6);
    const uint32_t s = f / 3, o = f - s * 3;
    const uint32_t n = a.len[r], m = n / 3, tiles = QfTileCount(m, W, step);
    const uint32_t last_start = m > W ? m - W : 0u;
    const uint8_t *dna = a.raw + a.off[r];
    const uint64_t rec0 = (uint64_t)a.first[r] + f;  // tile t: record rec0 + 6 t
    auto base = [&](uint32_t j) -> uint32_t {  // base at strand position j < n
      uint32_t b = s_base[dna[s ? n - 1 - j : j]];
      if (s && b <= 3) b = (~b) & 3u;
      return b;
    };
    // the group's letters into tile t (start st): bytes and length
    auto put_tile = [&](uint32_t t, uint32_t st, uint32_t t0, uint32_t letter, uint32_t put) {
      const uint32_t rel = letter - st;  // wraps below the tile's start
      const bool in = letter < m && letter >= st && rel < W;
      if (in) a.out[(rec0 + 6ull * t) * W + rel] = (uint8_t)put;
      const unsigned long long nonx = __ballot(in && put != kBaseX);
      const bool opens = st >= t0;  // the first group that touches this tile
      if (lane == 0 && (opens || nonx))
        a.qlen[rec0 + 6ull * t] = nonx ? t0 - st + 64u - (uint32_t)__clzll(nonx) : 1u;
    };
    uint32_t carry = 0;  // stop state entering this group of 64 letters
    for (uint32_t t0 = 0; t0 < m; t0 += 64) {
      const uint32_t t = t0 + lane, k = o + 2 + 3 * t;
      uint32_t code = 24, ev = 0;  // '*' padding past the last whole codon
      if (t < m && k < n) {
        const uint32_t b0 = base(k - 2), b1 = base(k - 1), b2 = base(k);
        const uint32_t codon = (b0 > 3 || b1 > 3 || b2 > 3) ? 64u : (b0 << 4 | b1 << 2 | b2);
        code = s_codon[codon];
        ev = codon == 14 ? 1u : (codon == 48 || codon == 50 || codon == 56) ? 2u : 0u;  // ATG / TAA TAG TGA
      }
      const unsigned long long evm = __ballot(ev != 0), setm = __ballot(ev == 2);
      const unsigned long long mine = evm & upto;
      const uint32_t stop = mine ? (uint32_t)(setm >> (63 - __clzll(mine))) & 1u : carry;
      const uint32_t put = stop ? 24u : code;
      carry = evm ? (uint32_t)(setm >> (63 - __clzll(evm))) & 1u : carry;
      // the regular tiles (start tt * step) with start + W > t0 and start < t0 + 64, then the flush-right one
      const uint32_t lo = t0 >= W ? (t0 - W) / step + 1 : 0u;
      const uint32_t hi = min(tiles - 1, (t0 + 64 + step - 1) / step);
      for (uint32_t tt = lo; tt < hi; ++tt) put_tile(tt, tt * step, t0, t, put);
      if (last_start < t0 + 64 && last_start + W > t0) put_tile(tiles - 1, last_start, t0, t, put);
    }
    // a frame shorter than the width (its only tile): X past its letters; no letters at all: length 1
    if (m < W) {
      uint8_t *rec = a.out + rec0 * W;
      for (uint32_t t = m + lane; t < W; t += 64) rec[t] = kBaseX;
      if (m == 0 && lane == 0) a.qlen[rec0] = 1u;
    }
  }
}

struct Buf {
  void *p = nullptr;
  explicit Buf(size_t bytes) { QF_CHECK(hipMalloc(&p, bytes < 256 ? 256 : bytes)); }
  ~Buf() {
    if (p) (void)hipFree(p);
  }
  Buf(const Buf &) = delete;
  Buf &operator=(const Buf &) = delete;
  template <class T> T *as() const { return static_cast<T *>(p); }
};

QfTables MakeTables() {
  QfTables t;
  for (int i = 0; i < 256; ++i) {
    t.protein[i] = ProteinCode((unsigned char)i);
    t.dna[i] = DnaCode((unsigned char)i);
  }
  // the standard genetic code, first base major over A C G T (formatter.cpp
  // kCodons), as residue codes
  const char *letters = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF";
  for (int i = 0; i < 128; ++i) t.codon[i] = kBaseX;
  for (int i = 0; i < 64; ++i) t.codon[i] = ProteinCode((unsigned char)letters[i]);
  return t;
}

}  // namespace

size_t QueryFormatTableBytes() { return sizeof(QfTables); }

void QueryFormatTables(void *dst) {
  const QfTables t = MakeTables();
  std::memcpy(dst, &t, sizeof(t));
}

void LaunchQueryFormat(void *stream, const uint8_t *d_raw, const uint64_t *d_off, const uint32_t *d_len, uint32_t n,
                       uint32_t width, uint32_t dna_len, uint8_t *d_out, uint32_t *d_qlen, const void *d_tab) {
  QfArgs a{d_raw, reinterpret_cast<const unsigned long long *>(d_off), d_len, n, width, dna_len, d_out,
           static_cast<const QfTables *>(d_tab), d_qlen};
  // one wave per record / read, grid-stride over at most 64 K blocks
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((n + kQfWaves - 1) / kQfWaves, 65536);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dna_len && d_qlen) hipLaunchKernelGGL(k_qry_frames<true>, dim3(blocks), dim3(kQfBlock), 0, st, a);
  else if (dna_len) hipLaunchKernelGGL(k_qry_frames<false>, dim3(blocks), dim3(kQfBlock), 0, st, a);
  else if (d_qlen) hipLaunchKernelGGL(k_qry_protein<true>, dim3(blocks), dim3(kQfBlock), 0, st, a);
  else hipLaunchKernelGGL(k_qry_protein<false>, dim3(blocks), dim3(kQfBlock), 0, st, a);
  QF_CHECK(hipGetLastError());
}

void LaunchQueryFormatTiled(void *stream, const uint8_t *d_raw, const uint64_t *d_off, const uint32_t *d_len,
                            const uint32_t *d_first, uint32_t n, uint32_t width, bool dna, uint32_t step,
                            uint8_t *d_out, uint32_t *d_qlen, const void *d_tab) {
  QfTileArgs a{d_raw, reinterpret_cast<const unsigned long long *>(d_off), d_len, d_first, n, width, step, d_out,
               static_cast<const QfTables *>(d_tab), d_qlen};
  // one wave per record / per (read, frame), grid-stride over at most 64 K blocks
  const uint64_t waves = (uint64_t)n * (dna ? 6 : 1);
  const uint32_t blocks = (uint32_t)std::min<uint64_t>((waves + kQfWaves - 1) / kQfWaves, 65536);
  hipStream_t st = static_cast<hipStream_t>(stream);
#ifdef GHOSTM_LDS_POISON
  const uint32_t v = kern::LdsPoisonPattern();
  QF_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(kern::g_lds_poison), &v, sizeof(v)));
#endif
  if (dna) hipLaunchKernelGGL(k_qry_frames_tiled, dim3(blocks), dim3(kQfBlock), 0, st, a);
  else hipLaunchKernelGGL(k_qry_protein_tiled, dim3(blocks), dim3(kQfBlock), 0, st, a);
  QF_CHECK(hipGetLastError());
}

void FormatQueriesDevice(const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets, const uint32_t *lengths,
                         uint32_t n, uint32_t width, uint32_t dna_len, uint8_t *records, int device,
                         float *device_ms) {
  if (device_ms) *device_ms = 0.f;
  const uint64_t nout = (uint64_t)n * (dna_len ? 6 : 1);
  if (n == 0 || width == 0) return;
  for (uint32_t r = 0; r < n; ++r)
    if (offsets[r] + lengths[r] > raw_len) throw Error("qry: record outside the letter buffer");
  int ndev = 0;
  QF_CHECK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) throw Error("qry: no such device");
  QF_CHECK(hipSetDevice(device));
  hipStream_t st;
  QF_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  struct StreamGuard {
    hipStream_t s;
    ~StreamGuard() { (void)hipStreamDestroy(s); }
  } sg{st};
  Buf d_raw(raw_len), d_off(8ull * n), d_len(4ull * n), d_out(nout * width), d_tab(sizeof(QfTables));
  hipEvent_t e0, e1;
  QF_CHECK(hipEventCreate(&e0));
  QF_CHECK(hipEventCreate(&e1));
  struct EventGuard {
    hipEvent_t a, b;
    ~EventGuard() {
      (void)hipEventDestroy(a);
      (void)hipEventDestroy(b);
    }
  } eg{e0, e1};
  if (raw_len) QF_CHECK(hipMemcpyAsync(d_raw.p, raw, raw_len, hipMemcpyHostToDevice, st));
  QF_CHECK(hipMemcpyAsync(d_off.p, offsets, 8ull * n, hipMemcpyHostToDevice, st));
  QF_CHECK(hipMemcpyAsync(d_len.p, lengths, 4ull * n, hipMemcpyHostToDevice, st));
  const QfTables tables = MakeTables();
  QF_CHECK(hipMemcpyAsync(d_tab.p, &tables, sizeof(tables), hipMemcpyHostToDevice, st));
  QF_CHECK(hipEventRecord(e0, st));
  LaunchQueryFormat(st, d_raw.as<uint8_t>(), d_off.as<uint64_t>(), d_len.as<uint32_t>(), n, width, dna_len,
                    d_out.as<uint8_t>(), nullptr, d_tab.p);
  QF_CHECK(hipEventRecord(e1, st));
  QF_CHECK(hipMemcpyAsync(records, d_out.p, nout * width, hipMemcpyDeviceToHost, st));
  QF_CHECK(hipStreamSynchronize(st));
  if (device_ms) QF_CHECK(hipEventElapsedTime(device_ms, e0, e1));
}

}  // namespace ghostm

extern "C" int GhostmFormatQueriesGpu(const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets,
                                      const uint32_t *lengths, uint32_t n, uint32_t width, uint32_t dna_len,
                                      uint8_t *records, int device, float *device_ms) {
  try {
    if (n && (!offsets || !lengths || !records || (!raw && raw_len))) throw ghostm::Error("qry: null argument");
    ghostm::FormatQueriesDevice(raw, raw_len, offsets, lengths, n, width, dna_len, records, device, device_ms);
    return 0;
  } catch (std::exception &e) {
    ghostm::SetLastErrorMessage(e.what());
    return 1;
  }
}
