// capi.cpp — session part of the C ABI (include/ghostm_hip.h Part 2).
#include <getopt.h>

#include <algorithm>
#include <cstring>
#include <fstream>
#include <functional>
#include <iostream>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "aligner.h"
#include "common.h"
#include "db_set.h"
#include "query_set.h"
#include "query_tiles.h"

using namespace ghostm;

namespace ghostm {
void SetLastErrorMessage(const std::string &m);
}

namespace {

// The vector copy-outs: with dst null the size, else at most cap elements of
// the vector get(session) returns (by reference or by value) and their count;
// (size_t)-1 with the message set for a null session or a throw.
template <class T, class Get>
size_t CopyOut(void *s, T *dst, size_t cap, Get get) {
  try {
    if (!s) throw Error("null session");
    const std::vector<T> &v = get(*static_cast<Session *>(s));
    if (!dst) return v.size();
    const size_t n = std::min(cap, v.size());
    if (n) std::memcpy(dst, v.data(), n * sizeof(T));
    return n;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

// The sized stats structs: the first min(size, sizeof(T)) bytes of what
// get(session) returns, and sizeof(T); 0 for a null session or struct.
template <class T, class Get>
size_t CopyStats(void *s, T *stats, size_t size, Get get) {
  if (!s || !stats) return 0;
  const T st = get(*static_cast<Session *>(s));
  std::memcpy(stats, &st, std::min(size, sizeof(T)));
  return sizeof(T);
}

}  // namespace

extern "C" {

void *GhostmSessionCreate(int argc, char **argv) {
  try {
    AlignerOptions opt = ParseAlignerOptions(argc, argv);
    return new Session(opt);
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return nullptr;
  }
}

void *GhostmSessionCreateDb(int argc, char **argv) {
  try {
    AlignerOptions opt = ParseAlignerOptions(argc, argv);
    return new Session(opt, Session::DbOnly{});
  } catch (std::exception &e) {
    SetLastErrorMessage(*e.what() ? e.what() : "invalid option");
    return nullptr;
  }
}

int GhostmSessionSetQueries(void *s, const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets,
                            const uint32_t *lengths, const char *names, uint64_t names_len, uint32_t n,
                            uint32_t width, int dna, uint32_t chunk_mb) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetQueries(raw, raw_len, offsets, lengths, names, names_len, n, width, dna != 0,
                                          chunk_mb);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

int GhostmSessionSetQueriesFasta(void *s, const char *path, uint32_t width, int dna, uint32_t chunk_mb,
                                 uint64_t *cut_records) {
  try {
    if (!s) throw Error("null session");
    if (!path) throw Error("set queries: null path");
    static_cast<Session *>(s)->SetQueriesFasta(path, width, dna != 0, chunk_mb, cut_records);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

int GhostmSessionSetOutputFile(void *s, const char *path) {
  try {
    if (!s) throw Error("null session");
    if (!path) throw Error("set output file: null path");
    static_cast<Session *>(s)->SetOutputFile(path);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionQueryLengths(void *s, uint32_t *qlen, size_t cap) {
  if (!s) return 0;
  const std::vector<uint32_t> v = static_cast<Session *>(s)->AllQueryLengths();
  if (!qlen) return v.size();
  const size_t n = std::min(cap, v.size());
  std::memcpy(qlen, v.data(), n * sizeof(uint32_t));
  return n;
}

size_t GhostmSessionQueryRecords(void *s, uint32_t chunk, uint8_t *codes, size_t cap) {
  try {
    if (!s) throw Error("null session");
    return static_cast<Session *>(s)->QueryRecords(chunk, codes, cap);
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

int64_t GhostmQueryChunkCuts(const uint32_t lengths[], uint64_t n, uint32_t chunk_mb, int dna, uint64_t cuts[],
                             uint64_t cap) {
  try {
    if (n && !lengths) throw Error("chunk cuts: null argument");
    std::vector<uint64_t> c;
    const bool whole = QueryChunkCuts(lengths, n, QueryChunkLimit(chunk_mb != 0, chunk_mb, dna != 0), &c);
    if (cuts) std::copy(c.begin(), c.begin() + (long)std::min<uint64_t>(cap, c.size()), cuts);
    if (!whole) throw Error("chunk cuts: too small max length.");
    return (int64_t)c.size() - 1;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return -1;
  }
}

int GhostmSessionSetQueriesTiled(void *s, const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets,
                                 const uint32_t *lengths, const char *names, uint64_t names_len, uint32_t n,
                                 uint32_t width, int dna, uint32_t chunk_mb, uint32_t max_len, uint32_t step) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetQueriesTiled(raw, raw_len, offsets, lengths, names, names_len, n, width, dna != 0,
                                               chunk_mb, max_len, step);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

int GhostmSessionSetQueriesFastaTiled(void *s, const char *path, uint32_t width, int dna, uint32_t chunk_mb,
                                      uint32_t max_len, uint32_t step, uint64_t *cut_records) {
  try {
    if (!s) throw Error("null session");
    if (!path) throw Error("set queries: null path");
    static_cast<Session *>(s)->SetQueriesFastaTiled(path, width, dna != 0, chunk_mb, max_len, step, cut_records);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionQueryTiles(void *s, GhostmQueryTile *tiles, size_t cap) {
  if (!s) return 0;
  const std::vector<GhostmQueryTile> &v = static_cast<Session *>(s)->QueryTiles();
  if (!tiles) return v.size();
  const size_t n = std::min(cap, v.size());
  if (n) std::memcpy(tiles, v.data(), n * sizeof(GhostmQueryTile));
  return n;
}

int64_t GhostmQueryTilePlan(const uint32_t lengths[], uint64_t n, uint32_t width, int dna, uint32_t max_len,
                            uint32_t step, GhostmQueryTile tiles[], uint64_t cap, uint64_t *cut_records) {
  try {
    if (n && !lengths) throw Error("tile plan: null argument");
    if (n > UINT32_MAX) throw Error("tile plan: over 4 G records");
    bool capped = false;
    const uint32_t W = QueryRecordWidth(width, dna != 0, &capped);
    CheckTileStep(W, step);
    uint64_t rows = 0, cut = 0;
    std::vector<GhostmQueryTile> one;
    for (uint64_t r = 0; r < n; ++r) {
      const uint32_t kept = TileKept(lengths[r], max_len);
      cut += kept < lengths[r] ? (dna ? 6 : 1) : 0;
      one.clear();
      AppendTiles((uint32_t)r, kept, W, dna != 0, step, &one);
      for (const GhostmQueryTile &t : one) {
        if (tiles && rows < cap) tiles[rows] = t;
        ++rows;
      }
    }
    if (cut_records) *cut_records = cut;
    return (int64_t)rows;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return -1;
  }
}

void *GhostmSessionCreateQueries(int argc, char **argv) {
  try {
    AlignerOptions opt = ParseAlignerOptions(argc, argv);
    return new Session(opt, Session::NoDb{});
  } catch (std::exception &e) {
    SetLastErrorMessage(*e.what() ? e.what() : "invalid option");
    return nullptr;
  }
}

int GhostmSessionSetDb(void *s, const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets,
                       const uint32_t *lengths, const char *names, uint64_t names_len, uint32_t n, uint32_t k,
                       uint32_t chunk_mb) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetDb(raw, raw_len, offsets, lengths, names, names_len, n, k, chunk_mb);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

int GhostmSessionSetDbFasta(void *s, const char *path, uint32_t k, uint32_t chunk_mb) {
  try {
    if (!s) throw Error("null session");
    if (!path) throw Error("set db: null path");
    static_cast<Session *>(s)->SetDbFasta(path, k, chunk_mb);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionDbChunks(void *s, GhostmDbChunkInfo *info, size_t cap) {
  if (!s) return 0;
  const Session *p = static_cast<Session *>(s);
  const size_t all = p->DbChunkCount();
  if (!info) return all;
  const size_t n = std::min(cap, all);
  for (size_t c = 0; c < n; ++c) p->DbChunkInfo((uint32_t)c, &info[c]);
  return n;
}

size_t GhostmSessionDbRecords(void *s, uint32_t chunk, uint8_t *codes, size_t cap) {
  try {
    if (!s) throw Error("null session");
    return static_cast<Session *>(s)->DbRecords(chunk, codes, cap);
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

int GhostmSessionDbIndex(void *s, uint32_t chunk, uint32_t *keys_count, size_t kc_cap, uint32_t *positions,
                         size_t pos_cap) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->DbIndex(chunk, keys_count, kc_cap, positions, pos_cap);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionDbStats(void *s, GhostmDbSetStats *stats, size_t size) {
  return CopyStats(s, stats, size, std::mem_fn(&Session::DbSetStats));
}

int64_t GhostmDbChunkCuts(const uint32_t lengths[], uint64_t n, uint32_t chunk_mb, uint64_t cuts[], uint64_t cap) {
  try {
    if (n && !lengths) throw Error("chunk cuts: null argument");
    if (chunk_mb > kDbChunkMbMax) throw Error("chunk cuts: chunk size above " + std::to_string(kDbChunkMbMax) + " MiB");
    std::vector<uint64_t> c;
    const bool whole = DbChunkCuts(lengths, n, DbChunkLimit(chunk_mb), &c);
    if (cuts) std::copy(c.begin(), c.begin() + (long)std::min<uint64_t>(cap, c.size()), cuts);
    if (!whole) throw Error("chunk cuts: too small max length.");
    return (int64_t)c.size() - 1;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return -1;
  }
}

void *GhostmSessionCreateShardEx(int argc, char **argv, int rank, int world, GhostmAllGatherFn allgather,
                                 void *ctx) {
  try {
    if (world < 1 || rank < 0 || rank >= world) throw Error("shard rank outside 0..world-1");
    AlignerOptions opt = ParseAlignerOptions(argc, argv);
    ShardExchange ex;
    ex.fn = allgather;
    ex.ctx = ctx;
    return new Session(opt, (uint32_t)rank, (uint32_t)world, &ex);
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return nullptr;
  }
}

void *GhostmSessionCreateShard(int argc, char **argv, int rank, int world) {
  return GhostmSessionCreateShardEx(argc, argv, rank, world, nullptr, nullptr);
}

int GhostmSessionShardRange(void *s, uint64_t *begin, uint64_t *end) {
  if (!s) return 1;
  const Session *p = static_cast<Session *>(s);
  if (begin) *begin = p->ShardBegin();
  if (end) *end = p->ShardEnd();
  return 0;
}

uint64_t GhostmSessionHitCapacity(void *s) {
  if (!s) return UINT64_MAX;
  return static_cast<Session *>(s)->HitCapacity();
}

int GhostmShardCuts(uint64_t n, const uint32_t weights[], const uint8_t group_start[], int world,
                    uint64_t cuts[]) {
  try {
    if (world < 1) throw Error("world must be >= 1");
    ShardCuts(n, weights, group_start, (uint32_t)world, cuts);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

int GhostmSessionRun(void *s) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->Run();
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

int GhostmSessionRunToFile(void *s) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->Run(true);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionOutput(void *s, char *buf, size_t cap) {
  if (!s) return 0;
  const std::string &o = static_cast<Session *>(s)->Output();
  if (!buf) return o.size();
  const size_t n = std::min(cap, o.size());
  std::memcpy(buf, o.data(), n);
  return n;
}

int GhostmSessionWrite(void *s) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->WriteOutputFile();
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionHits(void *s, GhostmHit *hits, size_t cap) {
  if (!s) return 0;
  const std::vector<GhostmHit> &h = static_cast<Session *>(s)->Hits();
  if (!hits) return h.size();
  const size_t n = std::min(cap, h.size());
  std::memcpy(hits, h.data(), n * sizeof(GhostmHit));
  return n;
}

size_t GhostmSessionHitsExt(void *s, GhostmHitExt *ext, size_t cap) {
  return CopyOut(s, ext, cap, std::mem_fn(&Session::HitsExt));
}

size_t GhostmSessionHitsPath(void *s, GhostmHitPath *rec, size_t cap) {
  return CopyOut(s, rec, cap, std::mem_fn(&Session::HitsPath));
}

size_t GhostmSessionPathOps(void *s, uint32_t *ops, size_t cap) {
  return CopyOut(s, ops, cap, std::mem_fn(&Session::PathOps));
}

size_t GhostmSessionHitsBand(void *s, GhostmHitPath *rec, size_t cap) {
  return CopyOut(s, rec, cap, std::mem_fn(&Session::HitsBand));
}

size_t GhostmSessionBandOps(void *s, uint32_t *ops, size_t cap) {
  return CopyOut(s, ops, cap, std::mem_fn(&Session::BandOps));
}

int GhostmSessionSetBand(void *s, uint32_t band) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetBand(band);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

int GhostmSessionSetMask(void *s, uint32_t window, uint32_t trigger, uint32_t extend) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetMask(window, trigger, extend);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionQueryMasked(void *s, uint32_t *masked, size_t cap) {
  if (!s) return 0;
  const std::vector<uint32_t> v = static_cast<Session *>(s)->AllQueryMasked();
  if (!masked) return v.size();
  const size_t n = std::min(cap, v.size());
  if (n) std::memcpy(masked, v.data(), n * sizeof(uint32_t));
  return n;
}

size_t GhostmSessionMaskStats(void *s, GhostmMaskStats *stats, size_t size) {
  return CopyStats(s, stats, size, std::mem_fn(&Session::MaskStats));
}

int GhostmSessionSetQuality(void *s, uint32_t trim_q, uint32_t mask_q, uint32_t min_len) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetQuality(trim_q, mask_q, min_len);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

int GhostmSessionSetQueriesFastqTiled(void *s, const char *path, uint32_t width, int dna, uint32_t chunk_mb,
                                      uint32_t max_len, uint32_t step, uint64_t *cut_records) {
  try {
    if (!s) throw Error("null session");
    if (!path) throw Error("set queries: null path");
    static_cast<Session *>(s)->SetQueriesFastqTiled(path, width, dna != 0, chunk_mb, max_len, step, cut_records);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

int GhostmSessionSetQueriesFastqMatesTiled(void *s, const char *path1, const char *path2, uint32_t width, int dna,
                                           uint32_t chunk_mb, uint32_t max_len, uint32_t step, uint64_t *cut_records) {
  try {
    if (!s) throw Error("null session");
    if (!path1 || !path2) throw Error("set queries: null path");
    static_cast<Session *>(s)->SetQueriesFastqMatesTiled(path1, path2, width, dna != 0, chunk_mb, max_len, step,
                                                         cut_records);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

int GhostmSessionSetQueriesQualTiled(void *s, const uint8_t *raw, const uint8_t *qual, uint64_t raw_len,
                                     const uint64_t *offsets, const uint32_t *lengths, const char *names,
                                     uint64_t names_len, uint32_t n, uint32_t width, int dna, uint32_t chunk_mb,
                                     uint32_t max_len, uint32_t step) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetQueriesQualTiled(raw, qual, raw_len, offsets, lengths, names, names_len, n, width,
                                                   dna != 0, chunk_mb, max_len, step);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionQueryQuality(void *s, GhostmQualOut *out, size_t cap) {
  if (!s) return 0;
  const std::vector<GhostmQualOut> &v = static_cast<Session *>(s)->QueryQuality();
  if (!out) return v.size();
  const size_t n = std::min(cap, v.size());
  if (n) std::memcpy(out, v.data(), n * sizeof(GhostmQualOut));
  return n;
}

size_t GhostmSessionQualityStats(void *s, GhostmQualStats *stats, size_t size) {
  return CopyStats(s, stats, size, std::mem_fn(&Session::QualityStats));
}

int GhostmSessionSetAdapters(void *s, const char *adapter1, const char *adapter2, uint32_t min_overlap, uint32_t err_pct,
                             uint32_t pair_overlap) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetAdapters(adapter1 ? adapter1 : "", adapter2 ? adapter2 : "", min_overlap, err_pct,
                                           pair_overlap);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionQueryAdapters(void *s, GhostmAdapterOut *out, size_t cap) {
  if (!s) return 0;
  const std::vector<GhostmAdapterOut> &v = static_cast<Session *>(s)->QueryAdapters();
  if (!out) return v.size();
  const size_t n = std::min(cap, v.size());
  if (n) std::memcpy(out, v.data(), n * sizeof(GhostmAdapterOut));
  return n;
}

size_t GhostmSessionAdapterStats(void *s, GhostmAdapterStats *stats, size_t size) {
  return CopyStats(s, stats, size, std::mem_fn(&Session::AdapterStats));
}

size_t GhostmSessionBandStats(void *s, GhostmBandStats *stats, size_t size) {
  return CopyStats(s, stats, size, std::mem_fn(&Session::BandStats));
}

size_t GhostmSessionHitsFrame(void *s, GhostmHitPath *rec, size_t cap) {
  return CopyOut(s, rec, cap, std::mem_fn(&Session::HitsFrame));
}

size_t GhostmSessionFrameOps(void *s, uint32_t *ops, size_t cap) {
  return CopyOut(s, ops, cap, std::mem_fn(&Session::FrameOps));
}

size_t GhostmSessionFrameInfo(void *s, GhostmHitFrameInfo *info, size_t cap) {
  return CopyOut(s, info, cap, std::mem_fn(&Session::FrameInfo));
}

int GhostmSessionSetFrameShift(void *s, int shift_cost) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetFrameShift(shift_cost);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionFrameStats(void *s, GhostmFrameStats *stats, size_t size) {
  return CopyStats(s, stats, size, std::mem_fn(&Session::FrameStats));
}

size_t GhostmSessionHitsBandRows(void *s, GhostmHitReadRows *rec, size_t cap) {
  return CopyOut(s, rec, cap, [](Session &x) -> auto & { return x.HitsReadRows(false); });
}
size_t GhostmSessionBandRowBytes(void *s, uint8_t *rows, size_t cap) {
  return CopyOut(s, rows, cap, [](Session &x) -> auto & { return x.ReadRowBytes(false); });
}
size_t GhostmSessionHitsFrameRows(void *s, GhostmHitReadRows *rec, size_t cap) {
  return CopyOut(s, rec, cap, [](Session &x) -> auto & { return x.HitsReadRows(true); });
}
size_t GhostmSessionFrameRowBytes(void *s, uint8_t *rows, size_t cap) {
  return CopyOut(s, rows, cap, [](Session &x) -> auto & { return x.ReadRowBytes(true); });
}

size_t GhostmSessionReadRowsStats(void *s, GhostmReadRowsStats *stats, size_t size) {
  return CopyStats(s, stats, size, std::mem_fn(&Session::ReadRowsStats));
}

size_t GhostmSessionHitsRows(void *s, GhostmHitRows *rec, size_t cap) {
  return CopyOut(s, rec, cap, std::mem_fn(&Session::HitsRows));
}

size_t GhostmSessionRowBytes(void *s, uint8_t *rows, size_t cap) {
  return CopyOut(s, rows, cap, std::mem_fn(&Session::RowBytes));
}

size_t GhostmSessionPileup(void *s, GhostmSubjectPileup *subj, size_t cap) {
  return CopyOut(s, subj, cap, std::mem_fn(&Session::Pileup));
}

size_t GhostmSessionPileupArrays(void *s, uint32_t *depth, uint32_t *identities, uint8_t *consensus, size_t cap) {
  try {
    if (!s) throw Error("null session");
    Session *ses = static_cast<Session *>(s);
    const std::vector<uint32_t> &d = ses->PileupDepth();
    if (!depth && !identities && !consensus) return d.size();
    const size_t n = std::min(cap, d.size());
    if (depth && n) std::memcpy(depth, d.data(), n * 4);
    if (identities && n) std::memcpy(identities, ses->PileupIdentities().data(), n * 4);
    if (consensus && n) std::memcpy(consensus, ses->PileupConsensus().data(), n);
    return n;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

size_t GhostmSessionSubjectProfile(void *s, uint32_t db_id, uint32_t *profile, size_t cap) {
  return CopyOut(s, profile, cap, [&](Session &x) { return x.SubjectProfile(db_id, !profile); });
}

size_t GhostmSessionReadPileup(void *s, int frame, GhostmSubjectReadPileup *subj, size_t cap) {
  return CopyOut(s, subj, cap, [&](Session &x) -> auto & { return x.ReadPileup(frame != 0).subj; });
}

size_t GhostmSessionReadPileupArrays(void *s, int frame, uint32_t *depth, uint32_t *identities, uint8_t *consensus,
                                     uint32_t *shifts, size_t cap) {
  try {
    if (!s) throw Error("null session");
    const Session::ReadPileupResult &r = static_cast<Session *>(s)->ReadPileup(frame != 0);
    if (!depth && !identities && !consensus && !shifts) return r.depth.size();
    const size_t n = std::min(cap, r.depth.size());
    if (depth && n) std::memcpy(depth, r.depth.data(), n * 4);
    if (identities && n) std::memcpy(identities, r.ident.data(), n * 4);
    if (consensus && n) std::memcpy(consensus, r.cons.data(), n);
    if (shifts && n) std::memcpy(shifts, r.shifts.data(), n * 4);
    return n;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

size_t GhostmSessionReadSubjectProfile(void *s, int frame, uint32_t db_id, uint32_t *profile, size_t cap) {
  return CopyOut(s, profile, cap, [&](Session &x) { return x.ReadSubjectProfile(frame != 0, db_id, !profile); });
}

size_t GhostmSessionReadPileupStats(void *s, GhostmReadPileupStats *stats, size_t size) {
  return CopyStats(s, stats, size, std::mem_fn(&Session::ReadPileupStats));
}

size_t GhostmSessionReadCull(void *s, int frame, GhostmCullOut *out, size_t cap) {
  try {
    if (!s) throw Error("null session");
    const std::vector<GhostmCullOut> &r = static_cast<Session *>(s)->ReadCull(frame != 0).out;
    if (!out) return r.size();
    const size_t n = std::min(cap, r.size());
    if (n) std::memcpy(out, r.data(), n * sizeof(GhostmCullOut));
    return n;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

int GhostmSessionSetCull(void *s, uint32_t top_k, uint32_t cover_pct) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetCull(top_k, cover_pct);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

int GhostmSessionSetTileGroups(void *s, int on) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetTileGroups(on != 0);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionReadCullStats(void *s, GhostmReadCullStats *stats, size_t size) {
  if (!s || !stats) return 0;
  const GhostmReadCullStats st = static_cast<Session *>(s)->ReadCullStats();
  std::memcpy(stats, &st, std::min(size, sizeof(GhostmReadCullStats)));
  return sizeof(GhostmReadCullStats);
}

int GhostmSessionSetTaxonomy(void *s, uint32_t nnodes, const uint32_t taxid[], const uint32_t parent[],
                             size_t nsubjects, const uint32_t subject_node[]) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetTaxonomy(nnodes, taxid, parent, nsubjects, subject_node);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

int GhostmSessionSetTaxonomyFiles(void *s, const char *nodes_path, const char *map_path) {
  try {
    if (!s) throw Error("null session");
    if (!nodes_path || !map_path) throw Error("set taxonomy: null: a path");
    static_cast<Session *>(s)->SetTaxonomyFiles(nodes_path, map_path);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionTaxonomyInfo(void *s, GhostmTaxonomyInfo *info, size_t size) {
  if (!s || !info) return 0;
  const GhostmTaxonomyInfo t = static_cast<Session *>(s)->TaxonomyInfo();
  std::memcpy(info, &t, std::min(size, sizeof(GhostmTaxonomyInfo)));
  return sizeof(GhostmTaxonomyInfo);
}

int GhostmSessionSetLca(void *s, uint32_t top_pct, uint32_t support_pct) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetLca(top_pct, support_pct);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionReadLca(void *s, int frame, GhostmLcaOut *out, size_t cap) {
  try {
    if (!s) throw Error("null session");
    const std::vector<GhostmLcaOut> &r = static_cast<Session *>(s)->ReadLca(frame != 0).out;
    if (!out) return r.size();
    const size_t n = std::min(cap, r.size());
    if (n) std::memcpy(out, r.data(), n * sizeof(GhostmLcaOut));
    return n;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

size_t GhostmSessionReadLcaBegin(void *s, int frame, uint32_t *read_begin, size_t cap) {
  try {
    if (!s) throw Error("null session");
    const std::vector<uint32_t> &r = static_cast<Session *>(s)->ReadLca(frame != 0).read_begin;
    if (!read_begin) return r.size();
    const size_t n = std::min(cap, r.size());
    if (n) std::memcpy(read_begin, r.data(), n * sizeof(uint32_t));
    return n;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

size_t GhostmSessionReadLcaStats(void *s, GhostmReadLcaStats *stats, size_t size) {
  if (!s || !stats) return 0;
  const GhostmReadLcaStats st = static_cast<Session *>(s)->ReadLcaStats();
  std::memcpy(stats, &st, std::min(size, sizeof(GhostmReadLcaStats)));
  return sizeof(GhostmReadLcaStats);
}

int GhostmSessionSetProfile(void *s, uint32_t min_reads) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetProfile(min_reads);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionTaxonProfile(void *s, int frame, GhostmTaxonCount *out, size_t cap) {
  try {
    if (!s) throw Error("null session");
    const std::vector<GhostmTaxonCount> &r = static_cast<Session *>(s)->TaxonProfile(frame != 0).rec;
    if (!out) return r.size();
    const size_t n = std::min(cap, r.size());
    if (n) std::memcpy(out, r.data(), n * sizeof(GhostmTaxonCount));
    return n;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

size_t GhostmSessionTaxonProfileFinal(void *s, int frame, uint32_t *final_node, size_t cap) {
  try {
    if (!s) throw Error("null session");
    const std::vector<uint32_t> &r = static_cast<Session *>(s)->TaxonProfile(frame != 0).final_node;
    if (!final_node) return r.size();
    const size_t n = std::min(cap, r.size());
    if (n) std::memcpy(final_node, r.data(), n * sizeof(uint32_t));
    return n;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

size_t GhostmSessionTaxonProfileSummary(void *s, int frame, GhostmTaxonSummary *summary, size_t size) {
  if (!s || !summary) return 0;
  try {
    const GhostmTaxonSummary t = static_cast<Session *>(s)->TaxonProfile(frame != 0).summary;
    std::memcpy(summary, &t, std::min(size, sizeof(GhostmTaxonSummary)));
    return sizeof(GhostmTaxonSummary);
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

size_t GhostmSessionTaxonProfileStats(void *s, GhostmTaxonProfileStats *stats, size_t size) {
  if (!s || !stats) return 0;
  const GhostmTaxonProfileStats st = static_cast<Session *>(s)->TaxonProfileStats();
  std::memcpy(stats, &st, std::min(size, sizeof(GhostmTaxonProfileStats)));
  return sizeof(GhostmTaxonProfileStats);
}

int GhostmSessionSetMates(void *s, int on, uint32_t max_insert) {
  try {
    if (!s) throw Error("null session");
    static_cast<Session *>(s)->SetMates(on != 0, max_insert);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

int GhostmSessionSetQueriesFastaMatesTiled(void *s, const char *path1, const char *path2, uint32_t width, int dna,
                                           uint32_t chunk_mb, uint32_t max_len, uint32_t step, uint64_t *cut_records) {
  try {
    if (!s) throw Error("null session");
    if (!path1 || !path2) throw Error("set queries: null: a path");
    static_cast<Session *>(s)->SetQueriesFastaMatesTiled(path1, path2, width, dna != 0, chunk_mb, max_len, step,
                                                         cut_records);
    return 0;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return 1;
  }
}

size_t GhostmSessionPairJoin(void *s, int frame, GhostmLcaHit *cand, uint32_t *partner, size_t cap) {
  try {
    if (!s) throw Error("null session");
    const Session::PairJoinResult &r = static_cast<Session *>(s)->PairJoin(frame != 0);
    if (!cand && !partner) return r.cand.size();
    const size_t n = std::min(cap, r.cand.size());
    if (n && cand) std::memcpy(cand, r.cand.data(), n * sizeof(GhostmLcaHit));
    if (n && partner) std::memcpy(partner, r.partner.data(), n * sizeof(uint32_t));
    return n;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

size_t GhostmSessionPairJoinPairs(void *s, int frame, GhostmPairOut *out, uint32_t *pair_begin, uint32_t *pair_record,
                                  size_t cap) {
  try {
    if (!s) throw Error("null session");
    const Session::PairJoinResult &r = static_cast<Session *>(s)->PairJoin(frame != 0);
    if (!out && !pair_begin && !pair_record) return r.out.size();
    const size_t n = std::min(cap, r.out.size());
    if (n && out) std::memcpy(out, r.out.data(), n * sizeof(GhostmPairOut));
    if (pair_begin) std::memcpy(pair_begin, r.pair_begin.data(), (2 * n + 1) * sizeof(uint32_t));
    if (n && pair_record) std::memcpy(pair_record, r.pair_record.data(), n * sizeof(uint32_t));
    return n;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

size_t GhostmSessionPairLca(void *s, int frame, GhostmLcaOut *out, size_t cap) {
  try {
    if (!s) throw Error("null session");
    const std::vector<GhostmLcaOut> &r = static_cast<Session *>(s)->PairLca(frame != 0).out;
    if (!out) return r.size();
    const size_t n = std::min(cap, r.size());
    if (n) std::memcpy(out, r.data(), n * sizeof(GhostmLcaOut));
    return n;
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

size_t GhostmSessionPairJoinStats(void *s, GhostmPairJoinStats *stats, size_t size) {
  if (!s || !stats) return 0;
  const GhostmPairJoinStats st = static_cast<Session *>(s)->PairJoinStats();
  std::memcpy(stats, &st, std::min(size, sizeof(GhostmPairJoinStats)));
  return sizeof(GhostmPairJoinStats);
}

size_t GhostmSessionDeviceHits(void *s, void *dst_device, size_t cap) {
  try {
    if (!s) throw Error("null session");
    return static_cast<Session *>(s)->DeviceHits(dst_device, cap);
  } catch (std::exception &e) {
    SetLastErrorMessage(e.what());
    return (size_t)-1;
  }
}

int GhostmSessionStats(void *s, GhostmStats *stats) {
  if (!s || !stats) return 1;
  *stats = static_cast<Session *>(s)->Stats();
  return 0;
}

size_t GhostmSessionStatsSized(void *s, GhostmStats *stats, size_t size) {
  return CopyStats(s, stats, size, std::mem_fn(&Session::Stats));
}

void GhostmSessionDestroy(void *s) { delete static_cast<Session *>(s); }

// `ghostm aln` (reference Aligner::Execute via main.cpp:107-121): the output file
// is opened right after option parsing; every error is printed and 0 returned.
int GhostmAlignMain(int argc, char **argv) {
  try {
    AlignerOptions opt = ParseAlignerOptions(argc, argv);
    if (opt.output_style == 22 || opt.output_style == 23)
      throw Error("-y 22 and -y 23 need a taxonomy: use `ghostm search` with -n nodes.tsv -a map.tsv");
    if (opt.output_style == 24 || opt.output_style == 25)
      throw Error("-y 24 and -y 25 need a taxonomy: use `ghostm search` with -n nodes.tsv -a map.tsv");
    if (opt.output_style == 26 || opt.output_style == 27)
      throw Error("-y 26 and -y 27 need mates: use `ghostm search` with -T, -j or -J, -n nodes.tsv -a map.tsv");
    { std::ofstream touch(opt.output_file.c_str()); }
    Session session(opt);
    session.Run(true);       // the output file is written while the search runs
    session.WriteOutputFile();  // no-op after a streamed run
    if (opt.verbose) {
      const GhostmStats &st = session.Stats();
      std::cout << "# queries " << st.queries << " candidates " << st.candidates << " hits "
                << st.hits << "\n# seconds total " << st.seconds_total << " seed " << st.seconds_seed
                << " score " << st.seconds_score << " traceback " << st.seconds_traceback
                << " merge " << st.seconds_merge << " output " << st.seconds_output << std::endl;
    }
  } catch (std::exception &e) {
    std::cerr << e.what() << std::endl;
  }
  return 0;
}

// `ghostm search`: one session with the database resident (-d: from its files;
// -f: formatted on the device from FASTA), then qry + aln per (FASTA, output)
// pair without the formatted files. Usage errors return 1 before any device call.
int GhostmSearchMain(int argc, char **argv) {
  std::vector<char *> aln_argv{argv[0]};
  uint32_t width = 75, chunk_mb = 0, tile_step = 0, max_len = 0;
  bool dna = false, have_d = false, tiled = false, have_x = false;
  std::string db_fasta;
  uint32_t db_k = 4, db_mb = 0, band = 0;  // band 0: the session's default
  long shift_cost = -1;                    // -F; below 0: the session's default
  long cull_k = -1, cull_pct = -1;         // -K, -C; below 0: the session's defaults
  bool tile_groups = false;                // -g
  std::string tax_nodes, tax_map;          // -n, -a
  long lca_top = -1, lca_support = -1;     // -p, -P; below 0: the session's defaults
  long profile_min = -1;                   // -R; below 0: the session's default
  MaskParams mask;                         // -Z w,k1,k2; window 0: no masking
  QualParams quality;                      // -Q trim,mask,minlen; all 0: no quality stage
  std::string adapter1, adapter2;          // -A SEQ1[,SEQ2]; both empty: no adapter rule
  bool have_O = false;                     // -O min_overlap,err_pct[,pair_overlap]
  uint32_t ad_overlap = 5, ad_err = 10, ad_pair = 0;
  bool mates_one = false, mates_two = false;  // -j: every file is interleaved mates; -J: r1.fasta r2.fasta out triples
  long max_insert = -1;                    // -I; below 0: the session's default
  int style = 0;                           // -y, as aln reads it
  optind = 1;
  opterr = 1;
  int c;
  // aln's options (aligner.cpp ParseAlignerOptions) plus -q, -w, -c, -f, -k, -m and -T, -X, -B, -F, -g, -K, -C, -n, -a,
  // -p, -P, -R, -Z, -j, -J, -I, -Q, -A, -O
  while ((c = getopt(argc, argv, "b:d:D:e:E:G:i:l:M:o:r:s:t:S:L:y:vq:w:c:f:k:m:T:X:B:F:gK:C:n:a:p:P:R:Z:jJI:Q:A:O:")) >= 0) {
    switch (c) {
      case 'A': {  // FASTQ reads: the 3' adapter, and mate 2's after a comma
        const char *comma = strchr(optarg, ',');
        adapter1 = comma ? std::string(optarg, (size_t)(comma - optarg)) : std::string(optarg);
        adapter2 = comma ? std::string(comma + 1) : std::string();
        if (adapter1.empty() || (comma && adapter2.empty())) return 1;
        AdapterParams checked;
        if (!MakeAdapterParams(adapter1.c_str(), adapter2.c_str(), 5, 10, 0, &checked).empty()) return 1;
        break;
      }
      case 'O': {  // the adapter stage's min_overlap,err_pct[,pair_overlap]
        unsigned long v[3] = {0, 0, 0};
        const char *at = optarg;
        for (int k = 0; k < 3; ++k) {
          char *end = nullptr;
          if (*at < '0' || *at > '9') return 1;
          v[k] = strtoul(at, &end, 10);
          if (end == at || v[k] > 1024) return 1;
          if (*end == '\0' && k >= 1) break;  // the pair value may be left out
          if (*end != ',' || k == 2) return 1;
          at = end + 1;
        }
        if (!ValidateAdapterParams((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]).empty()) return 1;
        have_O = true;
        ad_overlap = (uint32_t)v[0];
        ad_err = (uint32_t)v[1];
        ad_pair = (uint32_t)v[2];
        break;
      }
      case 'j': mates_one = true; break;  // with -T: records 2i and 2i + 1 of every file are mates
      case 'J': mates_two = true; break;  // with -T: the mates come in two files
      case 'I': {  // the mates' insert limit in read units, 1..2^24
        char *end = nullptr;
        const long v = strtol(optarg, &end, 10);
        if (end == optarg || *end || v < 1 || v > (1 << 24)) return 1;
        max_insert = v;
        break;
      }
      case 'Q': {  // FASTQ reads: trim_q,mask_q,min_len
        unsigned long v[3];
        const char *at = optarg;
        for (int k = 0; k < 3; ++k) {
          char *end = nullptr;
          if (*at < '0' || *at > '9') return 1;
          v[k] = strtoul(at, &end, 10);
          if (end == at || v[k] > (1ul << 24) || *end != (k < 2 ? ',' : '\0')) return 1;
          at = end + 1;
        }
        if (!ValidateQualParams((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]).empty()) return 1;
        quality.trim_q = (uint32_t)v[0];
        quality.mask_q = (uint32_t)v[1];
        quality.min_len = (uint32_t)v[2];
        break;
      }
      case 'Z': {  // low-complexity masking: window,trigger,extend
        unsigned long v[3];
        const char *at = optarg;
        for (int k = 0; k < 3; ++k) {
          char *end = nullptr;
          if (*at < '0' || *at > '9') return 1;
          v[k] = strtoul(at, &end, 10);
          if (end == at || v[k] > 1000 || *end != (k < 2 ? ',' : '\0')) return 1;
          at = end + 1;
        }
        if (!ValidateMaskParams((uint32_t)v[0], (uint32_t)v[1], (uint32_t)v[2]).empty()) return 1;
        mask.window = (uint32_t)v[0];
        mask.trigger = (uint32_t)v[1];
        mask.extend = (uint32_t)v[2];
        break;
      }
      case 'R': {  // the profile's floor, 1 or more
        char *end = nullptr;
        const long long v = strtoll(optarg, &end, 10);
        if (end == optarg || *end || v < 1 || v > 0xFFFFFFFFll) return 1;
        profile_min = (long)v;
        break;
      }
      case 'n': tax_nodes = optarg; break;  // the taxonomy's nodes file
      case 'a': tax_map = optarg; break;    // and the subjects' taxids
      case 'p':    // the assignment's top_pct, 0..100
      case 'P': {  // and support_pct, 51..100
        char *end = nullptr;
        const long v = strtol(optarg, &end, 10);
        if (end == optarg || *end || v < (c == 'p' ? 0 : 51) || v > 100) return 1;
        (c == 'p' ? lca_top : lca_support) = v;
        break;
      }
      case 'g': tile_groups = true; break;  // with -T: -b per tile, not per read
      case 'K':    // the cull's top_k, 1..255
      case 'C': {  // the cull's cover_pct, 1..100
        char *end = nullptr;
        const long v = strtol(optarg, &end, 10);
        if (end == optarg || *end || v < 1 || v > (c == 'K' ? 255 : 100)) return 1;
        (c == 'K' ? cull_k : cull_pct) = v;
        break;
      }
      case 'T':  // reads longer than the width as overlapping tiles, this many letters apart
        tiled = true;
        tile_step = (uint32_t)atoi(optarg);
        break;
      case 'X':  // with -T: every read cut at this many letters (nt for DNA) first
        have_x = true;
        max_len = (uint32_t)atoi(optarg);
        break;
      case 'B': {  // the half-width of -y 12's band, 1..31
        char *end = nullptr;
        const long v = strtol(optarg, &end, 10);
        if (end == optarg || *end || v < 1 || v > 31) return 1;
        band = (uint32_t)v;
        break;
      }
      case 'F': {  // the frameshift cost of -y 13, 0..1 << 20
        char *end = nullptr;
        const long v = strtol(optarg, &end, 10);
        if (end == optarg || *end || v < 0 || v > (1 << 20)) return 1;
        shift_cost = v;
        break;
      }
      case 'f': db_fasta = optarg; break;
      case 'k': db_k = (uint32_t)atoi(optarg); break;
      case 'm': db_mb = (uint32_t)atoi(optarg); break;
      case 'q':
        if (strcmp(optarg, "d") == 0) dna = true;
        else if (strcmp(optarg, "p") == 0) dna = false;
        else return 1;
        break;
      case 'w': width = (uint32_t)atoi(optarg); break;
      case 'c': chunk_mb = (uint32_t)atoi(optarg); break;
      case 'i':
      case 'o':
      case 'S':
      case 'L':
      case '?': return 1;
      case 'v': aln_argv.push_back(const_cast<char *>("-v")); break;
      default: {
        if (c == 'd') have_d = true;
        if (c == 'y') style = atoi(optarg);
        static const char *const kFlags[] = {"-b", "-d", "-D", "-e", "-E", "-G", "-l", "-M", "-r", "-s", "-t", "-y"};
        for (const char *f : kFlags)
          if (f[1] == c) aln_argv.push_back(const_cast<char *>(f));
        aln_argv.push_back(optarg);
      }
    }
  }
  std::vector<std::string> pos(argv + optind, argv + argc);
  const size_t per = mates_two ? 3 : 2;  // positionals per search
  if (pos.empty() || pos.size() % per) return 1;
  const bool mates = mates_one || mates_two;
  if (mates_one && mates_two) return 1;                     // one layout or the other
  if ((mates || max_insert >= 0) && !tiled) return 1;       // mates are source records of a tiled set
  if (max_insert >= 0 && !mates) return 1;                  // -I limits mates only
  if ((style == 26 || style == 27) && !mates) return 1;     // the pair lines need them
  if ((!adapter2.empty() || ad_pair) && !mates) return 1;   // mate 2's adapter and the pair rule need mates
  if (have_O && adapter1.empty() && !ad_pair) return 1;     // -O alone sets nothing
  const bool adapters_on = !adapter1.empty() || ad_pair;
  if (have_d == !db_fasta.empty()) return 1;  // -d or -f, not both
  if (have_x && !tiled) return 1;             // -X cuts a tiled set only
  if (tile_groups && !tiled) return 1;        // -g groups a tiled set only
  if (tax_nodes.empty() != tax_map.empty()) return 1;                // -n and -a come together
  if (style >= 22 && style <= 27 && tax_nodes.empty()) return 1;  // the taxon lines, the profile and the pair lines need them
  try {
    aln_argv.push_back(nullptr);
    AlignerOptions opt = ParseAlignerOptions((int)aln_argv.size() - 1, aln_argv.data());
    std::unique_ptr<Session> made(have_d ? new Session(opt, Session::DbOnly{}) : new Session(opt, Session::NoDb{}));
    Session &session = *made;
    if (!have_d) session.SetDbFasta(db_fasta, db_k, db_mb);
    if (band) session.SetBand(band);
    if (shift_cost >= 0) session.SetFrameShift(-(int)shift_cost);
    if (cull_k >= 0 || cull_pct >= 0) session.SetCull(cull_k >= 0 ? (uint32_t)cull_k : 1u, cull_pct >= 0 ? (uint32_t)cull_pct : 50u);
    if (tile_groups) session.SetTileGroups(true);
    if (!tax_nodes.empty()) session.SetTaxonomyFiles(tax_nodes, tax_map);  // after the database
    if (lca_top >= 0 || lca_support >= 0)
      session.SetLca(lca_top >= 0 ? (uint32_t)lca_top : 10u, lca_support >= 0 ? (uint32_t)lca_support : 100u);
    if (profile_min >= 0) session.SetProfile((uint32_t)profile_min);
    if (mask.window) session.SetMask(mask.window, mask.trigger, mask.extend);
    if (quality.On()) session.SetQuality(quality.trim_q, quality.mask_q, quality.min_len);
    if (adapters_on) session.SetAdapters(adapter1, adapter2, ad_overlap, ad_err, ad_pair);
    if (mates) session.SetMates(true, max_insert >= 0 ? (uint32_t)max_insert : 1000u);
    for (size_t k = 0; k < pos.size(); k += per) {
      try {
        { std::ofstream touch(pos[k + per - 1].c_str()); }
        session.SetOutputFile(pos[k + per - 1]);
        std::vector<std::string> cut;
        bool capped = false;
        // a file whose first byte is '@' is FASTQ (the mates' two files go by the first)
        const bool fastq = LooksLikeFastq(pos[k]);
        if (fastq && !tiled) throw Error("fastq: needs -T");
        if (quality.On() && !fastq) throw Error("quality: " + pos[k] + " has no qualities");
        if (adapters_on && !fastq) throw Error("adapters: " + pos[k] + " is not FASTQ");
        if (fastq && mates_two)
          session.SetQueriesFastqMatesTiled(pos[k], pos[k + 1], width, dna, chunk_mb, max_len, tile_step, nullptr, &capped);
        else if (fastq) session.SetQueriesFastqTiled(pos[k], width, dna, chunk_mb, max_len, tile_step, nullptr, &capped);
        else if (mates_two)
          session.SetQueriesFastaMatesTiled(pos[k], pos[k + 1], width, dna, chunk_mb, max_len, tile_step, nullptr, &capped);
        else if (tiled) session.SetQueriesFastaTiled(pos[k], width, dna, chunk_mb, max_len, tile_step, nullptr, &capped);
        else session.SetQueriesFasta(pos[k], width, dna, chunk_mb, nullptr, &cut, &capped);
        if (capped)
          std::cerr << "Warring: over upper limit of query length. Max is " << kMaxQueryLength * (dna ? 3 : 1) << "."
                    << std::endl;
        for (const std::string &name : cut) std::cerr << "warning : the length of sequence is over. " << name << std::endl;
        session.Run(true);
        session.WriteOutputFile();
        if (opt.verbose) {
          const GhostmStats &st = session.Stats();
          std::cout << "# " << pos[k] << " queries " << st.queries << " candidates " << st.candidates << " hits "
                    << st.hits << " seconds " << st.seconds_total << " query format " << st.seconds_query_format
                    << std::endl;
          if (mask.window) {
            const GhostmMaskStats &ms = session.MaskStats();
            std::cout << "# " << pos[k] << " masked letters " << ms.masked_letters << " sources " << ms.masked_sources
                      << " of " << ms.mask_sources << " seconds " << ms.seconds_mask << std::endl;
          }
          if (quality.On()) {
            const GhostmQualStats &qs = session.QualityStats();
            std::cout << "# " << pos[k] << " quality trimmed 5' " << qs.trimmed5 << " 3' " << qs.trimmed3 << " masked "
                      << qs.masked << " failed reads " << qs.failed << " of " << qs.reads << " seconds "
                      << qs.seconds_quality << std::endl;
          }
          if (adapters_on) {
            const GhostmAdapterStats &as = session.AdapterStats();
            std::cout << "# " << pos[k] << " adapters cut reads " << as.cut_reads << " letters " << as.cut_letters
                      << " adapter found " << as.adapter_found << " pairs found " << as.pair_found << " skipped "
                      << as.pair_skipped << " emptied " << as.emptied << " of " << as.reads << " seconds "
                      << as.seconds_adapter << std::endl;
          }
        }
      } catch (std::exception &e) {
        std::cerr << e.what() << std::endl;
      }
    }
  } catch (std::exception &e) {
    std::cerr << e.what() << std::endl;
  }
  return 0;
}

}  // extern "C"
