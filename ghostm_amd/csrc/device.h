// device.h — host-side interface of the gfx950 device module (device.hip).
//
// The module owns one HIP device per process, one stream, the score tables and
// the resident query/DB chunks, and runs the three kernel families of the `aln`
// hot path:
//   K1 seed      k-mer lists -> diagonal-bin candidates   (SearchNextCpu, aligner.cpp:383-521)
//   K2 score     Gotoh local score + end per candidate    (CalculateScoreCpu, aligner.cpp:545-685)
//   K3 traceback reverse DP -> start, length, matches    (TraceBack, aligner.cpp:771-949)
// Everything on the device is exact integer work; the host keeps the merge
// (libstdc++ std::sort order) and the float E-value formatting.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../../include/ghostm_hip.h"

namespace ghostm {

namespace kern {
struct TbArgs;
}

struct SeedConfig {
  uint32_t seed_mask = 15;   // index seed bits (db -k 4 -> 0b1111)
  uint32_t threshold = 2;    // aln -t
  uint32_t shift = 2;        // aln -s
  uint32_t log_region = 4;   // log2(aln -r)
};

struct GapConfig {
  uint32_t extend = 2;       // aln -e
  uint32_t log_region = 4;
  int open = -11;            // negated -G
  int ext = -1;              // negated -E
};

// Device-resident chunk handles (opaque to callers).
struct DevQuery;
struct DevDb;
struct MaskParams;  // query_mask.h
struct QualParams;  // read_quality.h
struct AdapterParams;  // read_adapter.h

// One hit chosen by the device merge (K4), after its traceback (K3):
// subject-relative coordinates, ml = (aln_len << 8) | matches.
struct SelectedHit {
  uint32_t sid, score, start, end, ml, chunk;  // chunk: the hit's DB chunk
};

// Selected hits landed on the host: an uninitialised block, freed when the last
// copy of `block` goes (the formatter releases it).
struct HostHits {
  std::shared_ptr<void> block;
  SelectedHit *data = nullptr;
  size_t n = 0;
  const SelectedHit &operator[](size_t i) const { return data[i]; }
};

// One K4 pass: the batch's candidate range (absolute; a batch may cut a name
// group) and the carried result lists (reference result_list, aligner.cpp:114):
// carry_in merges them with the batch's candidates, carry_out keeps the new
// lists for the next batch or DB chunk.
struct MergePass {
  uint64_t cand_lo = 0, cand_hi = UINT64_MAX;
  bool carry_in = false, carry_out = false;
  uint32_t chunk = 0;  // DB chunk id of the new hits
};

struct DeviceTimes {
  double seed = 0, score = 0, traceback = 0, merge = 0;  // seconds of device time (HIP events)
  double traceback_scan = 0;  // ... of which K3's scan phase (prep, pairs, sorts, k_tb_scan)
  uint64_t seed_bytes = 0, seed_list_entries = 0;
  uint64_t score_launches = 0, score_launches_packed = 0, score_launches_half = 0;
  uint64_t score_cells = 0, traceback_cells = 0;
  uint64_t traceback_launches = 0, traceback_launches_key = 0;
  uint64_t seed_launches_hash = 0;  // Seed() calls whose slot pass used k_seed_hash
  uint64_t score_rechecks = 0;      // guarded f16 candidates re-scored in int16
  uint64_t traceback_launches_scan = 0, traceback_scan_cells = 0;  // K3a scores-only pass
  uint64_t score_launches_framed = 0;  // f16 K2 launches of the column-framed kernel (k_score16f)
  uint64_t merge_launches = 0, merge_launches_wave = 0;            // K4 (k_merge_wave: one wave per group)
  uint64_t seed_queries_class[4] = {0, 0, 0, 0};  // K1 queries per size class (3 = global merge)
  uint64_t seed_queries_wide = 0;                 // ... redone by the offset pass (more than a slot)
  uint64_t seed_launches_filter = 0;              // Seed() calls whose classes 0/1 ran k_seed_filter
  uint64_t traceback_launches_scan_swar = 0;  // K3a scans over 16-bit integer patterns
  uint64_t traceback_launches_strips = 0;  // key DPs run by strip class (lanes of strips 0..i* only)
  uint64_t score_launches_swar = 0;  // ... of the framed kernel over 16-bit integer patterns (k_score16f<S, true>)
  uint64_t score_launches_unit = 0;  // ... of its unit-pair profile variant (k_score16f<S, true, true>)
  uint64_t score_launches_pair = 0;  // sparse segments: the pair-table kernel (k_score_pair)
  uint64_t seed_compact_redo = 0;    // K1 compactions re-run by the host (overflow, buffer growth)
  uint64_t seed_filter_overflows = 0;             // ... queries redone by k_seed_hash (queue overflow)
  uint64_t score_launches_levels = 0;             // K2 launches with restart levels (k_score16f<S, true, false, true>)
  uint64_t traceback_launches_keyframe = 0;       // K3 key DPs with the column-framed E chain (k_traceback_key FRAME)
  uint64_t score_launches_sparse = 0;             // K2 launches of sparse segments run by k_score16f<16, true> (kScoreRowsSparse)
  uint64_t seed_table_full = 0;                   // ... queries redone by k_seed (bin table probe bound reached)
  uint64_t traced_hits = 0;                       // device merge: hits selected from new candidates (K3 run)
  double traceback_ext = 0;                       // the extended traceback (k_traceback_ext): seconds,
  uint64_t traceback_ext_launches = 0, traceback_ext_cells = 0;  // launches, L x processed columns
  double traceback_path = 0;                      // the alignment paths (k_tb_path_fill + k_tb_path_walk): seconds,
  uint64_t traceback_path_launches = 0, traceback_path_cells = 0;  // batches, L x processed columns,
  uint64_t traceback_path_dir_bytes = 0;          // direction-buffer bytes of the batches
  double path_rows = 0;                           // the aligned rows (k_path_rows): seconds,
  uint64_t path_rows_launches = 0, path_rows_columns = 0, path_rows_bytes = 0;  // batches, columns, row bytes
  double pileup = 0;                              // the subject pile-up (k_pileup + k_pileup_finish): seconds,
  uint64_t pileup_launches = 0, pileup_windows = 0, pileup_parts = 0, pileup_columns = 0;  // k_pileup launches,
                                                  // profile windows, (tile, part) workgroups, columns added
  // the read-level passes' counters as the public structs hand them out (include/ghostm_hip.h)
  GhostmBandStats band{};                // k_band_fill<false> + k_band_walk<false> + k_ops_compact
  GhostmFrameStats frame{};              // the <true> instantiations + k_ops_compact, counted as the band pass
  GhostmReadRowsStats read_rows{};       // k_read_rows
  GhostmReadPileupStats read_pileup{};   // k_read_pileup + k_pileup_finish<true>, counted as the pile-up
  GhostmReadCullStats cull{};            // k_read_cull
  GhostmReadLcaStats lca{};              // k_read_lca*
  GhostmPairJoinStats pair{};            // k_pair_join
  GhostmTaxonProfileStats profile{};     // k_taxon_*
  GhostmMaskStats mask{};                // k_mask_windows + k_mask_apply
  GhostmQualStats qual{};                // k_qual_trim
  GhostmAdapterStats adapter{};          // k_adapter_find + k_pair_overlap
};

class DeviceModule {
 public:
  struct Impl;  // device.hip
  static DeviceModule &Get();

  void Bind(int device);                 // hipSetDevice + stream; idempotent; one device per process
  void Use() const;                      // make the bound device current on this thread
  int device() const { return device_; }
  void SetMatrix(const int *m32x32);     // M[db*32 + q]
  std::string DeviceName() const;
  size_t TotalMemory() const;

  // Copies n bytes host to host (the session sets a parallel one; default memcpy).
  using HostCopyFn = std::function<void(void *dst, const void *src, size_t n)>;
  void SetHostCopy(HostCopyFn fn);
  // Runs fn(k), k < parts, on host worker threads (the session sets its pool;
  // used by the K2 pair-list build and K1's count pass).
  using HostParallelFn = std::function<void(size_t parts, const std::function<void(size_t)> &fn)>;
  void SetHostParallel(HostParallelFn fn);
  // Host to device through page-locked staging on the main stream (see device.hip).
  void StagedUpload(void *dst, const void *src, size_t bytes);
  DevQuery *UploadQuery(const uint8_t *seq, uint32_t nseq, uint32_t L);
  // UploadQuery from letters (the resident form of the `qry` formatter,
  // qformat.hip): record r's letters are raw[off[r] .. off[r] + len[r]). They
  // go up through StagedUpload and are coded (dna_len = 0) or six-frame
  // translated (dna_len = the chunk's read length, at least 1) on the main
  // stream straight into the chunk's records: n (x 6) records of `width` codes.
  // Only qlen[n (x 6)], every record's QueryResidues, comes back. *seconds:
  // the kernel's device time.
  DevQuery *FormatQuery(const uint8_t *raw, uint64_t raw_len, const uint64_t *off, const uint32_t *len, uint32_t n,
                        uint32_t width, uint32_t dna_len, uint32_t *qlen, double *seconds);
  // FormatQuery for a tiled set (query_tiles.h): record r becomes the output
  // records first[r] .. first[r + 1] (first holds n + 1 entries, first[n] =
  // nout) by the tiled kernels of qformat.hip; len[r] is the record's kept
  // letters (nt for DNA, each read translated at its own length).
  DevQuery *FormatQueryTiled(const uint8_t *raw, uint64_t raw_len, const uint64_t *off, const uint32_t *len,
                             const uint32_t *first, uint32_t n, uint32_t width, bool dna, uint32_t step,
                             uint32_t *qlen, double *seconds);
  // The low-complexity mask of a resident chunk (query_mask.h; kernels:
  // query_mask.hip), in place on the main stream, straight after FormatQuery or
  // FormatQueryTiled: the masked letters of the nsrc sources become X in every
  // tile record that covers them. Everything is checked before any upload or
  // launch (throws ValidateMask's reason). Only masked[nseq], the letters
  // stored into every record, comes back. *call (may be null): this call's
  // counters, seconds_mask the two kernels' device time.
  void MaskQuery(DevQuery *q, uint32_t nsrc, const GhostmBandSource *src, uint32_t step, const MaskParams &params,
                 uint32_t *masked, GhostmMaskStats *call);
  // The quality stage of n reads (read_quality.h; kernel: read_quality.hip) on
  // the main stream: read r is len[r] bytes at off[r] of letters and of qual.
  // The reads go up in pieces of at most a fixed number of bytes (whole reads,
  // packed one after the other), each piece is trimmed and masked by one
  // launch, and its records and, with mask_q on, its masked letters come back
  // before the next piece goes up: the device never holds more than one piece.
  // The caller has made ValidateQuality's checks and params.On() holds. *call
  // (may be null): this call's counters, seconds_quality the kernel's device time.
  void QualityTrim(uint8_t *letters, const uint8_t *qual, const uint64_t *off, const uint32_t *len, uint32_t n,
                   const QualParams &params, GhostmQualOut *out, GhostmQualStats *call);
  // The adapter stage of n reads (read_adapter.h; kernels: read_adapter.hip) on
  // the main stream: read r is len[r] bytes at reads[r], which need not share a
  // buffer (the mates of two files are interleaved this way). The reads go up
  // in pieces as QualityTrim's do, of whole pairs with the pair rule on (n is
  // then even), each piece is searched by k_adapter_find (when an adapter is
  // set) and k_pair_overlap (when the pair rule is on), and its records come
  // back before the next piece goes up. The letters are only read. The caller
  // has made ValidateAdapters' checks and params.On() holds. *call (may be
  // null): this call's counters, seconds_adapter the kernels' device time.
  void AdapterTrim(const uint8_t *const *reads, const uint32_t *len, uint32_t n, const AdapterParams &params,
                   GhostmAdapterOut *out, GhostmAdapterStats *call);
  // A resident chunk's coded records (nseq * L bytes) back on the host.
  size_t QueryBytes(const DevQuery *q) const;
  void DownloadQuery(const DevQuery *q, uint8_t *dst);
  DevDb *UploadDb(const uint8_t *seq, uint32_t len, const uint32_t *keys_count, uint32_t kcl,
                  const uint32_t *positions, uint32_t npos);
  // UploadDb from letters (the resident form of the `db` formatter): the
  // chunk's n >= 1 records packed one after the other, each record's letters
  // followed by one '\n' (len bytes together, lengths[r] letters in record r;
  // no letter may be '\n'). The bytes go up through StagedUpload, are coded on
  // the main stream straight into the chunk's residues (kern::k_db_code:
  // ProteinCode per letter, END per separator), and the k-mer index of `seed`
  // is built from those device residues by the index.hip kernels into the
  // chunk's keys_count and positions; k_low_keys as UploadDb. The result is
  // what UploadDb makes of the files `ghostm db` writes for these records
  // (end_gap and the code flags from the lengths). Only *npos, the number of
  // positions, comes back. The temporaries (the packed letters and 16 bytes
  // per position) are module buffers, kept for the next call. *code_seconds,
  // *index_seconds: the device time of the coding kernel and of the index
  // build. Throws what CheckIndexSeed says and on lengths that do not add up.
  DevDb *FormatDb(const uint8_t *packed, uint32_t len, const uint32_t *lengths, uint32_t n, uint32_t seed,
                  uint32_t *npos, double *code_seconds, double *index_seconds);
  // A resident DB chunk back on the host: its residues (len bytes, the .seq
  // file), keys_count (kcl words) and positions (npos words); null: not copied.
  void DownloadDb(const DevDb *d, uint8_t *seq, uint32_t *keys_count, uint32_t *positions);
  // Name groups of a query chunk (consecutive equal names), for the device merge.
  void SetQueryGroups(DevQuery *q, const uint32_t *first, const uint32_t *last, uint32_t ng);
  // Subject start offsets (.pos) of a DB chunk, for the device merge.
  void SetDbSubjects(DevDb *d, const uint32_t *starts, uint32_t nsubj);
  void Free(DevQuery *q);
  void Free(DevDb *d);

  // K1 over every query of q against d. On return: counts[nseq] (host) and the
  // compact device candidate arrays (start, qid) ordered by (query, start).
  // offsets[q] = first candidate of query q. Returns total candidates.
  uint64_t Seed(DevQuery *q, DevDb *d, const SeedConfig &cfg, std::vector<uint32_t> *counts,
                std::vector<uint64_t> *offsets);
  // Copy candidate starts [begin, begin+n) to host.
  void CopyStarts(uint64_t begin, uint64_t n, uint32_t *out);

  // K2 over candidates [cand_begin, cand_begin + n) whose queries are
  // [q_first, q_end) with per-query counts/offsets as returned by Seed.
  // Scores/ends land in host arrays score[n], end[n] (when not null). With
  // `next`, the host builds and uploads the next segment's tasks while this
  // launch runs, and the Score() call for that segment launches at once.
  struct ScoreSegment {
    uint64_t cand_begin, n;
    uint32_t q_first, q_end;
  };
  void Score(DevQuery *q, DevDb *d, uint64_t cand_begin, uint64_t n, uint32_t q_first,
             uint32_t q_end, const std::vector<uint32_t> &counts,
             const std::vector<uint64_t> &offsets, uint32_t base_search_length,
             const GapConfig &gap, uint32_t *score, uint32_t *end, const ScoreSegment *next = nullptr);
  // Score() in two steps for the device-merge pipeline: ScoreLaunch enqueues K2
  // and uploads `next`'s tasks (copy stream) with no host wait; ScoreFinish
  // waits for K2 and re-scores its guard list. A guarded launch (ScoreGuarded)
  // must be finished before anything reads its scores.
  void ScoreLaunch(DevQuery *q, DevDb *d, uint64_t cand_begin, uint64_t n, uint32_t q_first, uint32_t q_end,
                   const std::vector<uint32_t> &counts, const std::vector<uint64_t> &offsets,
                   uint32_t base_search_length, const GapConfig &gap, const ScoreSegment *next);
  bool ScoreGuarded() const;
  void ScoreFinish();
  // With ScoreDeferNext(true), ScoreLaunch only records `next`; ScorePrepareNext
  // builds and uploads its tasks (call it after enqueueing the segment's K4/K3).
  void ScoreDeferNext(bool on) { defer_next_ = on; }
  void ScorePrepareNext(const std::vector<uint32_t> &counts, const std::vector<uint64_t> &offsets);

  uint32_t ScorePerBlock(DevQuery *q, const DevDb *d, uint32_t base_search_length, const GapConfig &gap) const;

  // K4 + K3 for a batch that covers every group of the chunk and starts from
  // empty result lists (first batch, first DB chunk): the reference Merge
  // selection on the device, then the traceback of every selected hit. Uses the
  // scores/ends left on the device by the preceding Score() over the same range.
  // counts[g] hits per group; hits[g*cap + k], cap = max(best, 1) (hits may be
  // null: nothing but the counts is copied back).
  void MergeSelect(DevQuery *q, DevDb *d, uint32_t g0, uint32_t g1, uint64_t cand_begin, uint64_t n, uint32_t best,
                   uint32_t tb_base, int open, int ext, std::vector<uint32_t> *counts,
                   HostHits *hits, const MergePass &pass = MergePass());
  // MergeSelect in two steps: MergeLaunch enqueues K4/K3 behind the segment's
  // K2 with no host wait; MergeCollect copies the selection back on the copy
  // stream (the main stream meanwhile runs the next segment's K2). One launch
  // may be outstanding; AppendRecords for it must precede the next MergeLaunch.
  void MergeLaunch(DevQuery *q, DevDb *d, uint32_t g0, uint32_t g1, uint64_t cand_begin, uint64_t n, uint32_t best,
                   uint32_t tb_base, int open, int ext, const MergePass &pass);
  void MergeCollect(std::vector<uint32_t> *counts, HostHits *hits);
  // Carried result lists of a query chunk (all groups empty), and their copy to
  // the host (counts[g], hits[g * cap + k]).
  void ResetCarry(DevQuery *q, uint32_t cap);
  void CarryToHost(DevQuery *q, uint32_t g0, uint32_t g1, uint32_t cap, std::vector<uint32_t> *counts,
                   HostHits *hits);
  // a block of n SelectedHit slots (contents undefined)
  void AcquireHostHits(size_t n, HostHits *out);
  // Global index of each DB chunk's first subject (hit records' db_id).
  void SetChunkBases(const uint32_t *bases, uint32_t n);

  // Device-resident hit records of the current run (GhostmHit layout, 32 B),
  // for the multi-GPU gather. AppendRecords turns the last MergeSelect's hits
  // (groups [g0, g0 + counts.size())) into records at the end of the array.
  // expect: the run's record bound (its groups x -b), reserved up front so
  // the array does not grow (reallocate and free) while the run's kernels are
  // queued; at most kRecordReserveMax bytes, beyond that it grows on demand
  void ResetRecords(uint64_t expect = 0);
  void AppendRecords(DevQuery *q, uint32_t g0, const std::vector<uint32_t> &counts, uint32_t cap,
                     uint32_t q_base, bool from_carry = false);  // from_carry: groups' carried lists
  void UploadRecords(const void *records, uint64_t n);  // host records (other paths)
  uint64_t RecordCount() const { return records_; }
  void CopyRecords(void *dst_device, uint64_t n);         // device-to-device, synchronous

  // K3 on n hits (query id, absolute db end).
  void TraceBack(DevQuery *q, DevDb *d, uint32_t n, const uint32_t *qid, const uint32_t *db_end,
                 uint32_t base_search_length, int open, int ext, uint32_t *db_start,
                 uint32_t *aln_len, uint32_t *aln_match, float *seq_id);

  // The extended traceback (kern::k_traceback_ext) on n hits: K3's outputs plus
  // one GhostmHitExt per hit. db_start_in (may be null): the hits' known
  // starts; each DP then stops after end - start + 1 columns, and the hits run
  // in the order of that count (ColumnOrder, hit_batches.h). Throws what
  // RefuseHits (hit_batches.h) says: L or the window exceeds the packed
  // fields, or a hit lies outside the chunks. Adds its device time, launches
  // and cells to times().
  void TraceBackExt(DevQuery *q, DevDb *d, uint32_t n, const uint32_t *qid, const uint32_t *db_end,
                    const uint32_t *db_start_in, uint32_t base_search_length, int open, int ext,
                    uint32_t *db_start, uint32_t *aln_len, uint32_t *aln_match, GhostmHitExt *out);

  // The alignment path of n hits (kern::k_tb_path_fill + kern::k_tb_path_walk):
  // rec[n] (may be null) and the hits' run-length words in hit order (*ops is
  // replaced; rec[i].ops_offset indexes it). db_start_in as for TraceBackExt.
  // The hits run in the order of their column counts, in batches cut by
  // CutBatch (hit_batches.h) with the direction buffer's bytes as the cost,
  // GHOSTM_PATH_SCRATCH_MB (default 1024) as the budget and
  // GHOSTM_PATH_BATCH_HITS as the hit cap; a batch's slots are packed on the
  // device (kern::k_ops_compact, the offsets from the host's prefix sum
  // over the records) and the batches' words joined in hit order on the host.
  // Throws what RefuseHits says (L > 127, L + window >= 32768, an empty
  // window, a hit outside the chunks). Adds its device time, batches, cells
  // and direction bytes to times().
  void TraceBackPath(DevQuery *q, DevDb *d, uint32_t n, const uint32_t *qid, const uint32_t *db_end,
                     const uint32_t *db_start_in, uint32_t base_search_length, int open, int ext,
                     GhostmHitPath *rec, std::vector<uint32_t> *ops);

  // The aligned residue rows of n hits (kern::k_path_rows): hit i lies in query
  // record qid[i]; rec[i] gives q_start, s_start (absolute in the chunk) and its
  // words in ops[ops_len]. Everything is checked first (ValidatePathRows,
  // path_rows.h; throws with the reason before any upload or launch, the
  // outputs untouched). out[n] (may be null) receives the records, with
  // query_record = qid[i] + record_base. rows (may be null: counts only)
  // receives hit i's 3 * columns bytes at dst_off[i], or, with dst_off null, the
  // hits' bytes one after the other from 0; out[i].rows_offset is that offset.
  // Throws ("rows_cap") when a hit's bytes would end past rows_cap. Returns the
  // hits' bytes together. The hits run in hit order in CutBatch's batches
  // (hit_batches.h): the cost a hit's row bytes, the budget
  // GHOSTM_ROWS_SCRATCH_MB (default 1024), the cap GHOSTM_ROWS_BATCH_HITS.
  // Adds its device time, batches, columns and bytes to times().
  size_t PathRows(DevQuery *q, DevDb *d, uint32_t n, const uint32_t *qid, const GhostmHitPath *rec,
                  const uint32_t *ops, size_t ops_len, int open, int ext, uint32_t record_base,
                  GhostmHitRows *out, uint8_t *rows, size_t rows_cap, const uint64_t *dst_off);

  // The pile-up of hits on positions [p0, p1) of the resident DB chunk d
  // (kern::k_pileup, kern::k_pileup_finish; include/ghostm_hip.h has the
  // definitions). The hits come in groups, one per query chunk: group g's hit i
  // lies in record qid[i] of chunk q, rec[i] as for PathRows, the words in
  // ops[ops_len]. Every group is checked first (ValidatePathRows; throws with
  // the reason before any upload or launch, the outputs untouched). depth,
  // identities, consensus (p1 - p0 elements) and profile ((p1 - p0) x 32) may
  // each be null. The tiles meeting [p0, p1) are cut into windows whose profile
  // fits GHOSTM_PILEUP_SCRATCH_MB (pileup_plan.h); per window: a memset, one
  // k_pileup launch per group and upload batch with hits there (at most
  // GHOSTM_PILEUP_BATCH_HITS hits), k_pileup_finish, and the read-back. Adds its
  // device time, launches, windows, parts and columns to times().
  struct PileupGroup {
    DevQuery *q;
    uint32_t n;
    const uint32_t *qid;
    const GhostmHitPath *rec;
  };
  void PathPileup(DevDb *d, const PileupGroup *groups, size_t ngroups, const uint32_t *ops, size_t ops_len,
                  uint32_t p0, uint32_t p1, uint32_t *depth, uint32_t *identities, uint8_t *consensus,
                  uint32_t *profile);

  // The pile-up of read-level hits on positions [p0, p1) of chunk d
  // (kern::k_read_pileup<frame>, kern::k_pileup_finish<true>; the contract is
  // above ReadPileupGpu in include/ghostm_hip.h). PathPileup's shape: group g's
  // hit i has source src[i] of chunk q (W = q's record width, tile step
  // `step`) and rec[i] as for ReadRows. Every group is checked first
  // (ValidateReadRows, ReadPileupSpans; throws with the reason before any
  // upload or launch). The plan gives a hit to every tile its charged span
  // meets, a position only a shift charges included. shifts (p1 - p0
  // elements) may be null like the other outputs. Adds to times().read_pileup*.
  struct ReadPileupGroup {
    DevQuery *q;
    uint32_t n;
    const GhostmBandSource *src;
    const GhostmHitPath *rec;
  };
  void ReadPileup(DevDb *d, const ReadPileupGroup *groups, size_t ngroups, const uint32_t *ops, size_t ops_len,
                  uint32_t step, bool frame, uint32_t p0, uint32_t p1, uint32_t *depth, uint32_t *identities,
                  uint8_t *consensus, uint32_t *shifts, uint32_t *profile);

  // The cull of nreads reads' hits (kern::k_read_cull; the contract is above
  // ReadCullGpu in include/ghostm_hip.h): read r's hits are hit[read_begin[r],
  // read_begin[r + 1]), out[i] hit i's record. Everything is checked first
  // (ValidateReadCull, read_cull.h; throws with the reason before any upload or
  // launch, out untouched). Needs no resident chunk. Adds to times().cull*.
  void ReadCull(uint32_t nreads, const uint32_t *read_begin, uint32_t nhits, const GhostmCullHit *hit, uint32_t top_k,
                uint32_t cover_pct, GhostmCullOut *out);

  // The join of npairs mate pairs (kern::k_pair_join; the contract is above
  // PairJoinGpu in include/ghostm_hip.h): pair p's hits are hit[pair_begin[2p],
  // pair_begin[2p + 2]), mate 2's from pair_begin[2p + 1]; cand[i] and
  // partner[i] are hit i's, out[p] pair p's record. Everything is checked first
  // (ValidatePairJoin, pair_join.h; throws with the reason before any upload or
  // launch, the outputs untouched). Needs no resident chunk. Adds to
  // times().pair*.
  void PairJoin(uint32_t npairs, const uint32_t *pair_begin, const uint32_t *offset, uint32_t nhits,
                const GhostmPairHit *hit, uint32_t max_span, uint32_t orient, GhostmLcaHit *cand, uint32_t *partner,
                GhostmPairOut *out);

  // The taxonomy of ReadLca (the contract is above ReadLcaGpu in
  // include/ghostm_hip.h): checked (TaxonomyDepths, read_lca.h; throws with the
  // reason, the resident one stays), packed and uploaded. Resident until the
  // next SetTaxonomy or DropTaxonomy. taxonomy_serial() changes with both, so
  // a session can tell whether the resident words are still its own.
  void SetTaxonomy(uint32_t nnodes, const uint32_t *parent);
  void DropTaxonomy();
  uint32_t taxonomy_nodes() const { return tax_nodes_; }
  uint64_t taxonomy_serial() const { return tax_serial_; }
  // The taxon of nreads reads (kern::k_read_lca_wave, kern::k_read_lca): read
  // r's hits are hit[read_begin[r], read_begin[r + 1]), out[r] its record.
  // Everything is checked first (ValidateReadLca, read_lca.h; throws with the
  // reason before any upload or launch, out untouched). Needs no resident
  // chunk. Adds to times().lca*.
  void ReadLca(uint32_t nreads, const uint32_t *read_begin, uint32_t nhits, const GhostmLcaHit *hit, uint32_t top_pct,
               uint32_t support_pct, GhostmLcaOut *out);
  // The taxon profile of nreads reads over the resident taxonomy (kern::k_taxon_count,
  // k_taxon_climb, k_taxon_floor, k_taxon_final, k_taxon_sort_*, k_taxon_emit; the contract is
  // above TaxonProfileGpu in include/ghostm_hip.h). The checks that need no
  // count come first (ValidateTaxonProfile, taxon_profile.h; throws before any
  // upload or launch); "cap" is known after the climb and throws once the count
  // arrays are clean again. Nothing is written on a throw. Needs no resident
  // chunk. Adds to times().profile*. With grow given, out and cap are not
  // used: *grow becomes the records, however many.
  void TaxonProfile(uint32_t nreads, const uint32_t *node, uint32_t min_reads, size_t cap, GhostmTaxonCount *out,
                    size_t *nout, uint32_t *final_node, GhostmTaxonSummary *summary,
                    std::vector<GhostmTaxonCount> *grow = nullptr);

  // The read-level banded alignment of n hits (kern::k_band_fill<false>,
  // k_band_walk<false>, k_ops_compact; the contract is in include/ghostm_hip.h): hit i aligns
  // source src[i] of chunk q (W = q's record width, tile step `step`) to
  // subject range [s_lo[i], s_hi[i]] of chunk d around diagonal D[i] with
  // half-width B. Everything is checked first (ValidateBand, band_align.h;
  // throws with the reason before any upload or launch). rec[n] (may be null)
  // and the words in hit order (*ops replaced; may be null) as TraceBackPath.
  // The hits run in the order of their row counts, in CutBatch's batches: the
  // cost a hit's direction bytes and word slot, the budget
  // GHOSTM_BAND_SCRATCH_MB (default 1024), the cap GHOSTM_BAND_BATCH_HITS.
  // Adds its device time, batches, hits, cells and direction bytes to times().
  void BandAlign(DevQuery *q, DevDb *d, uint32_t n, const GhostmBandSource *src, const int32_t *D,
                 const uint32_t *s_lo, const uint32_t *s_hi, uint32_t step, uint32_t B, int open, int ext,
                 GhostmHitPath *rec, std::vector<uint32_t> *ops);

  // The frameshift-aware read-level alignment (kern::k_band_fill<true>,
  // k_band_walk<true>, k_ops_compact): BandAlign with strand sources (src[i] names
  // frame 0 of a strand; ValidateFrame, frame_align.h) and the frameshift cost
  // `shift`. Buffers of its own, the budget GHOSTM_FRAME_SCRATCH_MB, the cap
  // GHOSTM_FRAME_BATCH_HITS, and the frame_* fields of times().
  void FrameAlign(DevQuery *q, DevDb *d, uint32_t n, const GhostmBandSource *src, const int32_t *D,
                  const uint32_t *s_lo, const uint32_t *s_hi, uint32_t step, uint32_t B, int open, int ext, int shift,
                  GhostmHitPath *rec, std::vector<uint32_t> *ops);

  // The aligned rows of n read-level hits (kern::k_read_rows<frame>; the
  // contract is above GhostmHitReadRows in include/ghostm_hip.h): hit i has
  // source src[i] of chunk q (W = q's record width, tile step `step`), rec[i]
  // gives q_start, s_start (absolute in chunk d) and its words in ops[ops_len].
  // Everything is checked first (ValidateReadRows, read_rows.h; throws with the
  // reason before any upload or launch, the outputs untouched). out, rows,
  // rows_cap, dst_off, record_base and the return value as PathRows. The hits
  // run in hit order in CutBatch's batches (hit_batches.h): the cost a hit's row
  // bytes, the budget GHOSTM_READ_ROWS_SCRATCH_MB (default 1024), the cap
  // GHOSTM_READ_ROWS_BATCH_HITS. Adds its device time, batches, hits and
  // columns to times().
  size_t ReadRows(DevQuery *q, DevDb *d, uint32_t n, const GhostmBandSource *src, const GhostmHitPath *rec,
                  const uint32_t *ops, size_t ops_len, uint32_t step, bool frame, int open, int ext, int shift,
                  uint32_t record_base, GhostmHitReadRows *out, uint8_t *rows, size_t rows_cap,
                  const uint64_t *dst_off);

  DeviceTimes &times() {
    SettleSeedTime();
    return times_;
  }
  void SettleSeedTime();
  void ResetTimes() { times_ = DeviceTimes(); }
  void Synchronize();

 private:
  DeviceModule() = default;
  // span: runs of slots whose hits may pair (a name group's slots)
  void LaunchTraceback(kern::TbArgs a, DevQuery *q, uint32_t n, const DevDb *d, uint32_t span);
  // BandAlign (frame false, shift unused) and FrameAlign
  void BandPass(bool frame, int shift, DevQuery *q, DevDb *d, uint32_t n, const GhostmBandSource *src, const int32_t *D,
                const uint32_t *s_lo, const uint32_t *s_hi, uint32_t step, uint32_t B, int open, int ext,
                GhostmHitPath *rec, std::vector<uint32_t> *ops);
  int device_ = -1;
  uint32_t tax_nodes_ = 0;   // the resident taxonomy's nodes; 0: none
  uint64_t tax_serial_ = 0;  // counts SetTaxonomy and DropTaxonomy
  bool profile_dirty_ = false;  // a TaxonProfile call ended before its count arrays were clean again
  void *stream_ = nullptr;
  HostCopyFn host_copy_;
  HostParallelFn host_par_;
  bool defer_next_ = false;
  void *copy_stream_ = nullptr;  // D2H of selections and K2 task uploads, beside the kernels
  DeviceTimes times_;
  uint64_t records_ = 0;
  Impl *impl_ = nullptr;
  friend struct DeviceModuleAccess;
};

// dt's timings and counters in the GhostmStats fields of the same meaning.
void StageCounters(const DeviceTimes &dt, GhostmStats *st);

const char *DeviceBuildInfo();

}  // namespace ghostm
