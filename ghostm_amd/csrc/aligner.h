// aligner.h — the `aln` driver: the reference Aligner (aligner.h:42-92,
// aligner.cpp:65-1012) re-built around the gfx950 device module.
//
// Same options, same chunk loops, same batch cuts, same Merge order (libstdc++
// std::sort), same tie rules and the same text output as the reference CPU path.
// Seed search, score DP, merge selection and traceback run on the GPU when a query
// chunk is one batch against one DB chunk (the common case, and the benchmark);
// otherwise the merge runs on host threads with the reference's exact semantics.
// Output text is produced by a background formatter while the GPU works on the
// next segment.
#pragma once
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <thread>
#include <vector>

#include "../../include/ghostm_hip.h"
#include "device.h"
#include "fastq_reader.h"
#include "formats.h"
#include "query_mask.h"
#include "read_adapter.h"
#include "read_quality.h"
#include "scoring.h"

namespace ghostm {

struct LineFormat;  // output line writer with per-session caches (aligner.cpp)

// reference AlignerOption (aligner.h:42-61), defaults of SetOption (aligner.cpp:226-243)
struct AlignerOptions {
  std::string output_file;
  std::string query_prefix;
  std::string db_prefix;
  uint32_t start_query_chunk = UINT32_MAX;
  uint32_t end_query_chunk = UINT32_MAX;
  uint32_t log_region = 4;
  uint32_t shift = 2;
  uint32_t threshold = 2;
  uint32_t max_list_length = 1u << 27;
  int open_gap = -11;
  int extend_gap = -1;
  uint32_t extend = 2;
  uint32_t best = 10;
  int device = 0;            // -D; the GPU path is the only path here
  int output_style = 0;      // -y
  bool verbose = false;
  ScoreMatrix matrix;
  KarlinParams karlin;
};

// getopt "b:d:D:e:E:G:i:l:M:o:r:s:t:S:L:y:v" (aligner.cpp:248); throws
// std::invalid_argument like the reference.
AlignerOptions ParseAlignerOptions(int argc, char **argv);

// A resolved hit: what the reference keeps in an Alignment (alignment.h:136-145).
struct HitRecord {
  uint32_t query = 0;        // index within its query chunk
  uint32_t db_chunk = 0;
  uint32_t subject = 0;      // index within its DB chunk
  uint32_t score = 0;
  uint32_t start = 0;        // absolute until traceback + rebase, then subject-relative
  uint32_t end = 0;
  uint32_t aln_len = 0;
  uint32_t aln_match = 0;
  float seq_id = 0.f;
};

// Number of host worker threads: GHOSTM_THREADS, else this process's share of
// the CPUs it may run on (affinity mask, cgroup quota) divided among the ranks
// of this node (LOCAL_WORLD_SIZE), between 1 and 16.
unsigned HostThreads();

// One batch of the reference's batch loop (aligner.cpp:131-171 with
// SearchNextCpu's cut, :511-514): queries [q0, q1) of a query chunk.
struct Batch {
  uint32_t q0, q1;
};

// The CPU path's batch cuts of one query chunk against one DB chunk, from every
// query's candidate count.
std::vector<Batch> CpuBatches(const std::vector<uint32_t> &counts, uint64_t max_list);

// The collective a rank-local shard session uses at creation
// (GhostmSessionCreateShardEx): an all-gather of byte buffers in rank order.
struct ShardExchange {
  GhostmAllGatherFn fn = nullptr;
  void *ctx = nullptr;
};

// Parallel for over [0, n) in contiguous blocks.
void ParallelFor(size_t n, unsigned threads, const std::function<void(size_t, size_t, unsigned)> &fn);
// ... in PieceCount(n, pieces) contiguous blocks, claimed in order by at most
// `threads` threads (fn's third argument is the block's index)
size_t PieceCount(size_t n, size_t pieces);
void ParallelForPieces(size_t n, size_t pieces, unsigned threads,
                       const std::function<void(size_t, size_t, unsigned)> &fn);

// One background thread running submitted tasks in order.
class TaskQueue {
 public:
  TaskQueue();
  ~TaskQueue();
  void Submit(std::function<void()> fn);
  void Drain();  // waits for every submitted task; rethrows the first error
 private:
  void Loop();
  std::mutex mu_;
  std::condition_variable cv_, idle_;
  std::deque<std::function<void()>> tasks_;
  bool stop_ = false, busy_ = false;
  std::exception_ptr error_;
  std::thread worker_;
};

// Multi-GPU shards: cuts[0..world] splitting n queries into
// contiguous ranges of about equal total weight, cut only where group_start[i]
// is set (a name group's first query); ghostm_amd/shard.py balanced_cuts is the
// same rule.
void ShardCuts(uint64_t n, const uint32_t *weight, const uint8_t *group_start, uint32_t world, uint64_t *cuts);

class Session {
 public:
  // shard_rank/shard_world: search only that shard of the query set (one
  // process per GPU); the shards' outputs concatenated in rank order are the
  // unsharded output, and hit records keep global query indices. Every shard
  // replays the unsharded run's batch cuts (the batch plan, fixed here): with
  // `exchange`, the rank reads and counts only its own queries and the ranks
  // all-gather their candidate counts; without, the rank counts every query
  // of the set itself once.
  explicit Session(const AlignerOptions &opt, uint32_t shard_rank = 0, uint32_t shard_world = 1,
                   const ShardExchange *exchange = nullptr);
  // A database session (GhostmSessionCreateDb): every DB chunk resident, no
  // queries until SetQueries; -i, -S or -L in the options is an error.
  struct DbOnly {};
  Session(const AlignerOptions &opt, DbOnly);
  // A session without a database (GhostmSessionCreateQueries): `aln`'s options
  // without -d (giving it is an error); with -i the query chunks are loaded as
  // usual, without it the session starts with neither input. The database
  // comes from SetDb / SetDbFasta; Run before that gives empty output.
  struct NoDb {};
  Session(const AlignerOptions &opt, NoDb);
  // Replaces the database by what `ghostm db -k k -l chunk_mb` would format
  // from these records (chunk_mb 0: db's default), made resident chunk by chunk
  // by DeviceModule::FormatDb: neither the codes nor the index visit the host
  // and no file is written. The record layout is SetQueries'. The last run's
  // results are dropped, the old chunks' device blocks go back to the pool;
  // the query chunks stay. Throws on a shard session (its batch plan was
  // agreed on the old database) and on bad arguments (a null argument, a
  // record outside the buffer, a seed the index refuses, chunk_mb over
  // kDbChunkMbMax, a record that alone is over the chunk limit): the session
  // is then as it was. A failure while the chunks load leaves the session
  // with no database.
  void SetDb(const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets, const uint32_t *lengths,
             const char *names, uint64_t names_len, uint32_t n, uint32_t k, uint32_t chunk_mb);
  // ... read from a FASTA file with the formatter's reader. A file that cannot
  // be opened leaves the session as it was; a record over the chunk limit is
  // found only while the chunks load.
  void SetDbFasta(const std::string &path, uint32_t k, uint32_t chunk_mb);
  // the resident DB chunks: their number; one chunk's header values, its
  // residues (the .seq bytes; NULL: their size) and its index copied back
  size_t DbChunkCount() const { return dbs_.size(); }
  void DbChunkInfo(uint32_t chunk, GhostmDbChunkInfo *info) const;
  size_t DbRecords(uint32_t chunk, uint8_t *codes, size_t cap);
  void DbIndex(uint32_t chunk, uint32_t *keys_count, size_t kc_cap, uint32_t *positions, size_t pos_cap);
  // Replaces the query set by what `ghostm qry -l width [-t d] -L chunk_mb`
  // would format from these records (chunk_mb 0: qry's default), formatted on
  // the device straight into the resident chunks (DeviceModule::FormatQuery);
  // the last run's results are dropped, the old chunks' device blocks go back
  // to the pool. Throws on a shard session and on bad arguments (the session
  // is then as it was); a set that fails while loading leaves the session
  // with no queries. names: n names, each ended by '\n'.
  void SetQueries(const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets, const uint32_t *lengths,
                  const char *names, uint64_t names_len, uint32_t n, uint32_t width, bool dna, uint32_t chunk_mb);
  // ... read from a FASTA file with the formatter's reader. cut_records (may be
  // null): the output records over the width, cut_names (may be null): their
  // names in qry's warning order, *capped (may be null): the width was over
  // the limit (qry's other warning).
  void SetQueriesFasta(const std::string &path, uint32_t width, bool dna, uint32_t chunk_mb, uint64_t *cut_records,
                       std::vector<std::string> *cut_names = nullptr, bool *capped = nullptr);
  // SetQueries with tiles (query_tiles.h): every record is cut at max_len
  // (letters, nt for DNA; 0: no cut) and then enters as overlapping tile
  // records of the width under its name, made on the device by
  // DeviceModule::FormatQueryTiled. The chunk cuts are over the kept letters.
  // Everything is planned before the old set is dropped: besides SetQueries'
  // refusals, step 0, step over the width, a record over kMaxTileRecords and a
  // chunk that would wrap a 32-bit field leave the session as it was.
  // cut_records (may be null): the records max_len cut (x 6 for DNA reads).
  void SetQueriesTiled(const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets, const uint32_t *lengths,
                       const char *names, uint64_t names_len, uint32_t n, uint32_t width, bool dna,
                       uint32_t chunk_mb, uint32_t max_len, uint32_t step, uint64_t *cut_records = nullptr);
  // ... read from a FASTA file, the whole file before the first chunk is made.
  void SetQueriesFastaTiled(const std::string &path, uint32_t width, bool dna, uint32_t chunk_mb, uint32_t max_len,
                            uint32_t step, uint64_t *cut_records, bool *capped = nullptr);
  // The tile table of a tiled set, one entry per query record over the chunks
  // in order; empty for any other set. Forgotten with the set (DropQueries).
  const std::vector<GhostmQueryTile> &QueryTiles() const { return tile_table_; }
  // the -o path of later Run(true) and WriteOutputFile calls
  void SetOutputFile(const std::string &path);
  // every record's WriteOutput length over the chunks in order, and one
  // chunk's coded records copied back from the device (NULL: their size)
  std::vector<uint32_t> AllQueryLengths() const;
  size_t QueryRecords(uint32_t chunk, uint8_t *codes, size_t cap);
  uint64_t ShardBegin() const { return shard_begin_; }
  uint64_t ShardEnd() const { return shard_end_; }
  // the most hit records one run can return: name groups x max(-b, 1)
  uint64_t HitCapacity() const;
  ~Session();

  // whole search; replaces previous results. stream_to_file: also write the
  // output file (-o) while the search runs, each segment's text as soon as it
  // is formatted, in order (WriteOutputFile is then a no-op for this run)
  void Run(bool stream_to_file = false);
  const std::string &Output();         // text of the last run (joined on first use)
  void WriteOutputFile();
  const std::vector<GhostmHit> &Hits();
  // One GhostmHitExt per hit of Hits(): a post-pass of the extended traceback
  // over the final hits of the last run, grouped by (query chunk, DB chunk),
  // with the known starts; computed on first use, kept until the next run.
  // The search pipeline is not involved, so the records do not depend on the
  // merge mode or the batch cuts. With -y 6 Run makes them and the text.
  const std::vector<GhostmHitExt> &HitsExt();
  // One GhostmHitPath per hit of Hits() and the run-length words they index:
  // a post-pass of the path traceback (DeviceModule::TraceBackPath), one call
  // per (query chunk, DB chunk) that has hits, with the known starts and the
  // query HitsExt() resolved for each hit; subject coordinates relative to the
  // subject. Computed on first use, kept until the next run. With -y 7 Run
  // makes them and the text.
  const std::vector<GhostmHitPath> &HitsPath();
  const std::vector<uint32_t> &PathOps();
  // One GhostmHitRows per hit of Hits() and the row bytes they index, in hit
  // order: a post-pass of DeviceModule::PathRows over HitsPath(), one call per
  // (query chunk, DB chunk) that has hits, every hit's bytes landing at its
  // place in hit order. query_record is the global index of the record
  // HitsExt() resolved. Computed on first use, kept until the next run or the
  // next query set. With -y 8 and -y 9 Run makes them and the text.
  const std::vector<GhostmHitRows> &HitsRows();
  const std::vector<uint8_t> &RowBytes();
  // One read-level GhostmHitPath per hit of Hits() and the run-length words
  // they index (include/ghostm_hip.h, BandAlignGpu): a post-pass of
  // DeviceModule::BandAlign, one call per (query chunk, DB chunk) that has hits.
  // A hit's source is the whole read or frame its resolved record is a tile of
  // (on an untiled set the record itself, with its QueryLengths entry as m), its
  // subject range the whole subject, its anchor the first cell of its tile path
  // (HitsPath) in source coordinates; q_* are source coordinates, s_* relative
  // to the subject. Computed on first use, kept until the next run, query set,
  // database or SetBand.
  const std::vector<GhostmHitPath> &HitsBand() { return ReadLevel(false).rec; }
  const std::vector<uint32_t> &BandOps() { return ReadLevel(false).ops; }
  // the band's half-width, 1..31 (default 31); a change drops the band results
  void SetBand(uint32_t band);
  uint32_t Band() const { return band_; }
  const GhostmBandStats &BandStats() const { return band_stats_; }
  // One frameshift-aware read-level GhostmHitPath per hit of Hits(), the words
  // they index and a GhostmHitFrameInfo each (include/ghostm_hip.h,
  // FrameAlignGpu): a post-pass of DeviceModule::FrameAlign, one call per (query
  // chunk, DB chunk) that has hits. A hit's source is the strand of the frame
  // its resolved record is a tile of, its subject range the whole subject, its
  // anchor HitsBand's D; q_* are strand positions, s_* relative to the subject.
  // Throws on a set that is not a DNA set of a tiled setter. Computed on first
  // use, kept until the next run, query set, database, SetBand or SetFrameShift.
  const std::vector<GhostmHitPath> &HitsFrame() { return ReadLevel(true).rec; }
  const std::vector<uint32_t> &FrameOps() { return ReadLevel(true).ops; }
  const std::vector<GhostmHitFrameInfo> &FrameInfo();
  // the frameshift cost, -(1 << 20)..0 (default -15); a change drops the frame results
  void SetFrameShift(int shift);
  const GhostmFrameStats &FrameStats() const { return frame_stats_; }
  // One level's read-level paths, band [0] or frame [1]: per hit its record,
  // the words the records index, and the chunk-local source the pass aligned
  // (src[h].letters is the m a read-level line is priced with). HitsBand(),
  // HitsFrame() and every pass built on them read it through ReadLevel.
  struct ReadLevelResult {
    bool valid = false;
    std::vector<GhostmHitPath> rec;
    std::vector<uint32_t> ops;
    std::vector<GhostmBandSource> src;
    void Drop() {
      rec.clear();
      ops.clear();
      src.clear();
      valid = false;
    }
  };
  const ReadLevelResult &ReadLevel(bool frame);
  // One GhostmHitReadRows per hit of Hits() and the row bytes they index, in
  // hit order, for the read-level paths of HitsBand() (frame false) or
  // HitsFrame() (frame true, with the session's frameshift cost): a post-pass
  // of DeviceModule::ReadRows, one call per (query chunk, DB chunk) that has
  // hits, with the sources the path pass used. query_record is a global record
  // index. Computed on first use and kept as long as the paths they were made
  // from. With -y 14 / -y 15 Run makes them and the text.
  const std::vector<GhostmHitReadRows> &HitsReadRows(bool frame);
  const std::vector<uint8_t> &ReadRowBytes(bool frame);
  const GhostmReadRowsStats &ReadRowsStats() const { return read_rows_stats_; }
  // The subject pile-up of the last run's hits (include/ghostm_hip.h): one
  // GhostmSubjectPileup per subject over all DB chunks in db_id order, and the
  // subjects' depth, identities and consensus concatenated without the END
  // separators. A post-pass of DeviceModule::PathPileup over HitsPath() with
  // the records HitsExt() resolved: per DB chunk one call, which goes window by
  // window and, inside a window, query chunk by query chunk; the summary is
  // made here from the arrays that came back. Computed on first use, kept until
  // the next run or the next query set. With -y 10 and -y 11 Run makes them and
  // the text.
  const std::vector<GhostmSubjectPileup> &Pileup();
  const std::vector<uint32_t> &PileupDepth();
  const std::vector<uint32_t> &PileupIdentities();
  const std::vector<uint8_t> &PileupConsensus();
  // The 32-slot rows of one subject (length x 32), made on demand by the same
  // kernels on that subject's hits only; nothing is kept.
  // count_only: zeros of that size, no device work.
  std::vector<uint32_t> SubjectProfile(uint32_t db_id, bool count_only = false);
  // The same from the read-level paths (the contract is above ReadPileupGpu in
  // include/ghostm_hip.h): HitsBand()'s (frame false) or HitsFrame()'s (frame
  // true), with the sources those passes aligned; a post-pass of
  // DeviceModule::ReadPileup, per DB chunk one call. Kept as long as the paths
  // they were made from. With -y 16 to -y 19 Run makes them and the text.
  struct ReadPileupResult {
    std::vector<GhostmSubjectReadPileup> subj;
    std::vector<uint32_t> depth, ident, shifts;
    std::vector<uint8_t> cons;
    bool valid = false;
    void Drop() { *this = ReadPileupResult(); }
  };
  const ReadPileupResult &ReadPileup(bool frame);
  std::vector<uint32_t> ReadSubjectProfile(bool frame, uint32_t db_id, bool count_only = false);
  const GhostmReadPileupStats &ReadPileupStats() const { return read_pileup_stats_; }
  // The cull of the last run's hits by their read-level alignments (the
  // contract is above ReadCullGpu in include/ghostm_hip.h): one GhostmCullOut
  // per hit of Hits(), from HitsBand()'s records (frame false) or HitsFrame()'s
  // (frame true). A read is a maximal run of consecutive hits whose resolved
  // records have one source record in the tile table (on an untiled set: one
  // name group); dup_of is an index of Hits(). subject is the hit's db_id, the
  // s range the path's, the q range the path's interval in forward-strand read
  // units: letters on a protein set, nucleotides on a DNA set of a tiled setter
  // at both levels (CullInterval), so that the two strands' hits meet. One
  // DeviceModule::ReadCull call. Computed on first use and kept as long as the
  // paths it was made from and the parameters. With -y 20 / -y 21 Run makes it
  // and the text.
  struct ReadCullResult {
    std::vector<GhostmCullOut> out;
    std::vector<uint32_t> read_begin;
    bool valid = false;
    void Drop() { *this = ReadCullResult(); }
  };
  const ReadCullResult &ReadCull(bool frame);
  // top_k 1..255 (default 1), cover_pct 1..100 (default 50); a change drops the kept results
  void SetCull(uint32_t top_k, uint32_t cover_pct);
  const GhostmReadCullStats &ReadCullStats() const { return cull_stats_; }
  // Tile groups: from the next tiled setter on, a name group also ends where
  // the tile table begins a new tile (every record of a protein set, every six
  // of a DNA set), so -b is kept per tile and not per read. Off by default;
  // refused on a shard session.
  void SetTileGroups(bool on);
  bool TileGroups() const { return tile_groups_; }
  // Low-complexity masking (query_mask.h; the contract is above
  // GhostmMaskRecordsHost in include/ghostm_hip.h): from the next SetQueries*
  // call on, every chunk is masked on the device straight after it is
  // formatted (DeviceModule::MaskQuery). window 0: off, the default; otherwise
  // throws "window" / "levels" and keeps the old setting. The current set and
  // its results stay as they are; refused on a shard session.
  void SetMask(uint32_t window, uint32_t trigger, uint32_t extend);
  // the letters masked in every query record over the chunks in order; empty
  // for a set made with masking off
  std::vector<uint32_t> AllQueryMasked() const;
  // the mask counters of the current set (all 0 for a set made with masking off)
  const GhostmMaskStats &MaskStats() const { return mask_stats_; }
  // A taxonomy for the resident database and the taxon of every read (the
  // contract is above ReadLcaGpu in include/ghostm_hip.h; the session calls
  // are described at GhostmSessionSetTaxonomy). SetTaxonomy checks everything,
  // makes the words resident (DeviceModule::SetTaxonomy) and only then takes
  // the arrays; DropDb forgets them.
  void SetTaxonomy(uint32_t nnodes, const uint32_t *taxid, const uint32_t *parent, size_t nsubjects,
                   const uint32_t *subject_node, uint64_t map_unmatched = 0);
  void SetTaxonomyFiles(const std::string &nodes_path, const std::string &map_path);
  GhostmTaxonomyInfo TaxonomyInfo() const;
  // top_pct 0..100 (default 10), support_pct 51..100 (default 100); a change drops the kept results
  void SetLca(uint32_t top_pct, uint32_t support_pct);
  // One record per read of ReadCull(frame), from its records: a KEPT hit votes
  // with its read-level score and the cull's stretch, node =
  // subject_node[db_id]. One DeviceModule::ReadLca call over the KEPT hits
  // alone (a hit of score 0 is no candidate and changes nothing). Computed on first use;
  // kept as long as the cull's result, the parameters and the taxonomy.
  struct ReadLcaResult {
    std::vector<GhostmLcaOut> out;
    std::vector<uint32_t> read_begin;
    bool valid = false;
    void Drop() { *this = ReadLcaResult(); }
  };
  const ReadLcaResult &ReadLca(bool frame);
  const GhostmReadLcaStats &ReadLcaStats() const { return lca_stats_; }
  // The sample's taxon profile (the contract is above TaxonProfileGpu in
  // include/ghostm_hip.h; the session calls are described at
  // GhostmSessionSetProfile): one DeviceModule::TaxonProfile call over the
  // node field of ReadLca(frame)'s records. Computed on first use; kept as
  // long as the assignment under it and the floor. min_reads >= 1 (default 1);
  // a change drops only the profile.
  void SetProfile(uint32_t min_reads);
  struct TaxonProfileResult {
    std::vector<GhostmTaxonCount> rec;
    std::vector<uint32_t> final_node;
    GhostmTaxonSummary summary{};
    bool valid = false;
    void Drop() { *this = TaxonProfileResult(); }
  };
  const TaxonProfileResult &TaxonProfile(bool frame);
  const GhostmTaxonProfileStats &TaxonProfileStats() const { return profile_stats_; }
  // Mate pairs (the contract is above PairJoinGpu in include/ghostm_hip.h; the
  // session calls are described at GhostmSessionSetMates): with mates on,
  // source records 2i and 2i + 1 of a tiled set are the mates of pair i.
  // max_insert 1..2^24 in read units (default 1000). A change drops only the
  // pair results and the profile counted from them; refused on a shard
  // session. A pair pass throws "mates" while mates are off, on an untiled set
  // and on an odd number of source records.
  void SetMates(bool on, uint32_t max_insert);
  bool Mates() const { return mates_; }
  // PairJoin: one DeviceModule::PairJoin call over all hits of Hits(), from
  // ReadCull(frame): a KEPT hit is a candidate with the cull's record, its
  // subject's node (0xFFFFFFFF without a taxonomy) and its tile's strand, every
  // other hit has score 0. pair_begin has two entries per pair and one more
  // (indices of Hits()); pair_record is mate 1's source record. A pair is there
  // when either mate has a hit. PairLca: one DeviceModule::ReadLca call over
  // cand with the pairs as reads. Both computed on first use and kept as long
  // as the cull's and the assignment's results and SetMates' parameters.
  struct PairJoinResult {
    std::vector<GhostmLcaHit> cand;
    std::vector<uint32_t> partner;
    std::vector<GhostmPairOut> out;
    std::vector<uint32_t> pair_begin, pair_record;
    bool valid = false;
    void Drop() { *this = PairJoinResult(); }
  };
  const PairJoinResult &PairJoin(bool frame);
  struct PairLcaResult {
    std::vector<GhostmLcaOut> out;
    bool valid = false;
    void Drop() { *this = PairLcaResult(); }
  };
  const PairLcaResult &PairLca(bool frame);
  const GhostmPairJoinStats &PairJoinStats() const { return pair_stats_; }
  // The tiled FASTA setter over two files of mates: record i of path1 and
  // record i of path2 become source records 2i and 2i + 1. Files of different
  // record counts are refused before the old set is dropped.
  void SetQueriesFastaMatesTiled(const std::string &path1, const std::string &path2, uint32_t width, bool dna,
                                 uint32_t chunk_mb, uint32_t max_len, uint32_t step, uint64_t *cut_records,
                                 bool *capped = nullptr);
  // Quality trimming and masking of FASTQ and quality-carrying sets
  // (read_quality.h; the contract is above GhostmQualityTrimHost and
  // GhostmSessionSetQuality in include/ghostm_hip.h). 0, 0, 0: off, the
  // default; otherwise throws "param" and keeps the old setting. It takes
  // effect at the next SetQueriesFastq*Tiled / SetQueriesQualTiled; refused on
  // a shard session.
  void SetQuality(uint32_t trim_q, uint32_t mask_q, uint32_t min_len);
  // The tiled setters over reads with qualities: the file (or the two mates'
  // files, interleaved record by record) is parsed, the quality stage runs on
  // all reads (DeviceModule::QualityTrim, when it is on), read r enters as
  // letters[begin, begin + kept), max_len cuts what was kept, and
  // SetTiledRecords makes the set. A malformed file, a quality byte outside
  // '!'..'~' and every SetQueriesTiled refusal leave the session as it was.
  void SetQueriesFastqTiled(const std::string &path, uint32_t width, bool dna, uint32_t chunk_mb, uint32_t max_len,
                            uint32_t step, uint64_t *cut_records, bool *capped = nullptr);
  void SetQueriesFastqMatesTiled(const std::string &path1, const std::string &path2, uint32_t width, bool dna,
                                 uint32_t chunk_mb, uint32_t max_len, uint32_t step, uint64_t *cut_records,
                                 bool *capped = nullptr);
  void SetQueriesQualTiled(const uint8_t *raw, const uint8_t *qual, uint64_t raw_len, const uint64_t *offsets,
                           const uint32_t *lengths, const char *names, uint64_t names_len, uint32_t n, uint32_t width,
                           bool dna, uint32_t chunk_mb, uint32_t max_len, uint32_t step, uint64_t *cut_records = nullptr);
  // one record per source read of the current set; empty when the stage did not run for it
  const std::vector<GhostmQualOut> &QueryQuality() const { return qual_out_; }
  // the quality counters of the current set (all 0 when the stage did not run)
  const GhostmQualStats &QualityStats() const { return qual_stats_; }
  const QualParams &Quality() const { return qual_; }
  // Adapter removal on FASTQ and quality-carrying sets (read_adapter.h; the
  // contract is above GhostmAdapterTrimHost and GhostmSessionSetAdapters in
  // include/ghostm_hip.h). Both adapters empty and pair_overlap 0: off, the
  // default; throws "param" or "adapter" and keeps the old setting. It takes
  // effect at the next SetQueriesFastq*Tiled / SetQueriesQualTiled, where the
  // stage runs ahead of the quality stage; refused on a shard session.
  void SetAdapters(const std::string &adapter1, const std::string &adapter2, uint32_t min_overlap, uint32_t err_pct,
                   uint32_t pair_overlap);
  // one record per source read of the current set; empty when the stage did not run for it
  const std::vector<GhostmAdapterOut> &QueryAdapters() const { return adapter_out_; }
  // the adapter counters of the current set (all 0 when the stage did not run)
  const GhostmAdapterStats &AdapterStats() const { return adapter_stats_; }
  const AdapterParams &Adapters() const { return adapter_; }
  // Hit records of the last run in device memory (this session's GPU): copies
  // min(n, cap) records to dst_device; returns n.
  size_t DeviceHits(void *dst_device, size_t cap);
  const GhostmStats &Stats() const { return stats_; }
  // the counters of the database sets (GhostmSessionDbStats): all 0 for a database read from files
  GhostmDbSetStats DbSetStats() const;

 private:
  struct QueryData {
    QueryChunk chunk;
    DevQuery *dev = nullptr;
    std::vector<uint32_t> group_end;   // per query: one past the last query of its name group
    std::vector<uint32_t> group_first, group_last;  // name groups in order
    std::vector<uint32_t> qlen;        // WriteOutput's query length (last non-X + 1)
    std::vector<uint32_t> masked;      // letters masked per record (SetMask); empty: the chunk was not masked
    uint32_t global_base = 0;          // index of the chunk's first query over all chunks
    // shard sessions: this slice is queries [slice_lo, slice_lo + nseq) of a
    // chunk of chunk_nseq queries, and plan[d] holds the whole chunk's batch
    // cuts against DB chunk d (chunk indices); plan_sum[d] / plan_hash[d] are
    // the slice's candidate total and count hash, checked on every run
    bool planned = false;
    uint32_t slice_lo = 0, chunk_nseq = 0;
    std::vector<std::vector<Batch>> plan;
    std::vector<uint64_t> plan_sum, plan_hash;
  };
  struct DbData {
    DbChunk chunk;
    DevDb *dev = nullptr;
    uint32_t global_base = 0;
  };
  // Output of one segment: one piece per formatting worker, in output order.
  // Parts are reused across runs, so their buffers keep their capacity (no
  // release and re-fault of ~100 bytes per hit on every run).
  struct Part {
    std::vector<std::string> text;
    std::vector<std::vector<GhostmHit>> hits;
    // a streamed run (FormatSelected) writes each piece as soon as it is
    // formatted, in order: the formatting workers mark pieces done, the writer
    // waits for the next one; Abandon (formatting failed) releases the writer
    std::mutex mu;
    std::condition_variable cv;
    std::vector<uint8_t> done;
    bool abandoned = false, streaming = false;
    void Reset(size_t pieces);
    void MarkDone(size_t k);
    void Abandon();
    bool Wait(size_t k);  // false: abandoned before piece k was formatted
  };
  using Results = std::vector<std::vector<HitRecord>>;

  static void PrepareQueryChunk(QueryData *q, bool qlen = true);
  // one record of a set being loaded: its letters and its name
  struct QueryRecordView {
    const char *seq;
    uint32_t len;
    std::string_view name;
  };
  void CreateOrFree(uint32_t shard_rank, uint32_t shard_world, const ShardExchange *ex);
  void DropQueries();  // the last run's results and the resident query chunks
  // The one place a database is forgotten: the last run's results, the resident
  // DB chunks and everything priced or planned with them (the E-value text
  // cache of format_, the seed counts, the device's chunk bases).
  void DropDb();
  // the next chunk of a database being set (db's files for these records, resident)
  void AddDbChunk(const QueryRecordView *recs, uint32_t n, uint32_t seed);
  void RefuseDbSet(uint32_t k, uint32_t chunk_mb) const;  // throws on a shard session, a bad k or chunk_mb
  void FinishDbSet();
  // the next chunk of a set (qry's files for these records, resident)
  void AddQueryChunk(const QueryRecordView *recs, uint32_t n, uint32_t width, bool dna, uint64_t *cut_records,
                     std::vector<std::string> *cut_names);
  // the tiled set of these records (len: already cut at max_len), planned
  // whole before the old set is dropped
  struct TiledRule {
    uint32_t width, max_concat, step;
    bool dna;
  };
  void SetTiledRecords(const QueryRecordView *recs, uint32_t n, const TiledRule &rule);
  // its next chunk; record_base: recs[0]'s index in the set
  void AddQueryChunkTiled(const QueryRecordView *recs, uint32_t n, uint32_t record_base, const TiledRule &rule);
  // the offset a detail line adds to hit's query coordinates: its tile's, 0 on an untiled set
  uint32_t TileOffset(size_t hit) const {
    return tile_table_.empty() ? 0u
                               : tile_table_[queries_[hit_source_[hit].qi].global_base + hit_source_[hit].query].offset;
  }
  void FinishQuerySet();
  void QueryStats();  // the query-set fields of stats_
  void QueryLengths(std::vector<QueryData *> chunks);
  void ApplyShard(uint32_t rank, uint32_t world);
  // shard sessions: the batch plan of every (query chunk, DB chunk)
  void PlanFromCounts(QueryData &q, size_t di, const std::vector<uint32_t> &chunk_counts, uint32_t n);
  void Create(uint32_t shard_rank, uint32_t shard_world, const ShardExchange *ex);
  void Load(uint32_t shard_rank, uint32_t shard_world, bool local, std::vector<uint32_t> *chunk_nseq,
            std::vector<std::vector<uint64_t>> *rank_lo);
  void AgreeOnCreate(uint32_t rank, uint32_t world, const ShardExchange &ex, const std::string &err,
                     const std::vector<uint32_t> &chunk_nseq, const std::vector<std::vector<uint64_t>> &rank_lo);
  void PlanExchange(uint32_t rank, uint32_t world, const ShardExchange &ex,
                    const std::vector<uint32_t> &chunk_nseq, const std::vector<std::vector<uint64_t>> &rank_lo);
  // the passes of one Seed() result: the plan's batches restricted to the
  // slice (local indices, possibly empty), or the slice's own cuts unsharded
  // (total: the counts' sum when known, else UINT64_MAX)
  std::vector<Batch> Passes(QueryData &q, size_t di, const std::vector<uint32_t> &counts,
                            uint64_t total = UINT64_MAX) const;
  void RunQueryChunk(QueryData &q);
  void RunQueryChunkHostMerge(QueryData &q);
  void DevicePass(QueryData &q, DbData &d, const std::vector<uint32_t> &counts,
                  const std::vector<uint64_t> &offsets, uint32_t bq0, uint32_t bq1, uint64_t c_lo, uint64_t c_hi,
                  bool carry_in, bool final_pass);
  void HostMergeBatch(QueryData &q, DbData &d, uint32_t bq0, uint32_t bq1, uint64_t cand_begin,
                      const uint32_t *score, const uint32_t *end, const std::vector<uint32_t> &counts,
                      const std::vector<uint64_t> &offsets, Results *results);
  void FormatResults(const QueryData &q, const Results &results, Part *out);
  void FormatSelected(const QueryData &q, uint32_t g0, const std::vector<uint32_t> &counts,
                      const HostHits &hits, uint32_t cap, Part *out);
  Part *NewPart();
  // a part's text is complete: hands it to the output writer when streaming
  void PartDone(const Part *part);
  void StreamPart(Part *part);
  const LineFormat &Format();
  void DropResults();  // forgets the last run's results and everything derived from them
  uint32_t TbBase(const QueryData &q) const;  // the traceback's DP window of a query chunk
  // The detail passes (HitsExt, HitsPath, HitsRows) make one device call per
  // (query chunk, DB chunk): the hit indices of pair [qi * dbs_.size() + di] as
  // HitsExt() resolved them (hit_source_), and fn(qi, di, items) for every pair
  // that has any.
  std::vector<std::vector<size_t>> HitsByChunkPair() const;
  template <class Item, class F> void ForChunkPairs(const std::vector<std::vector<Item>> &groups, F fn);
  // Rewrites the parts' text, one line per hit in hit order, pieces in
  // parallel: line(hit, in, pos, nl, tab, out) appends hit's new text to out
  // from its line in[pos, nl), with tab[0 .. tabs) the line's last tabs found
  // from its end (tab[0] the trailing one); extra(first, n) is what to reserve
  // beyond the input's size for hits [first, first + n). Throws "<what>: ..."
  // on fewer lines than hits or fewer tabs than asked for.
  template <class Extra, class Line> void RewriteLines(const char *what, int tabs, Extra extra, Line line);
  // -y 6: rewrites the parts' style-0 lines as the twelve BLAST-tabular columns
  void FormatTabular();
  // -y 7: the same with columns 3 to 10 taken from the hit's path, and its CIGAR
  // -y 12 (read_level): ... from the hit's read-level path where its score is above 0
  void FormatPathTabular(bool read_level = false);
  // -y 13: the -y 7 columns from the hit's frame path in read nucleotide
  // coordinates, then qframe and frameshifts
  void FormatFrameTabular();
  // -y 8: the -y 7 line plus positives, the query row and the subject row;
  // -y 9: the pairwise view (a '#' line of the first fourteen columns, the
  // three rows, an empty line). Both rewrite the -y 7 text of FormatPathTabular.
  void FormatRows();
  // -y 14 (frame false) and -y 15 (frame true): positives, qseq and sseq from
  // the hit's read-level rows appended to the -y 12 / -y 13 line; a hit of
  // read-level score 0 takes the three fields from its tile rows (HitsRows).
  void FormatReadRows(bool frame);
  // The chunk pairs' words of a path pass joined in hit order (HitsPath, ReadLevel)
  void JoinWords(const std::vector<std::vector<uint32_t>> &words, std::vector<GhostmHitPath> *path,
                 std::vector<uint32_t> *ops) const;
  // The plan HitsRows and HitsReadRows share: places in hit order, *bytes sized,
  // call(qi, di, items, rec, dst) per chunk pair with absolute subject coordinates
  template <class Call>
  void RowsPlan(const std::vector<GhostmHitPath> &path, const std::vector<uint32_t> &words, std::vector<uint8_t> *bytes,
                Call call);
  // The paths a pile-up is made from: the tile paths (HitsPath), the band paths
  // (ReadLevel(false)) or the frame paths (ReadLevel(true)); LevelPaths makes them.
  enum PathLevel { kTileLevel = 0, kBandLevel = 1, kFrameLevel = 2 };
  const std::vector<GhostmHitPath> &LevelPaths(PathLevel lv);
  // The pile-up of a level, kept in pileup_[lv]; Pileup() and ReadPileup() return it
  const ReadPileupResult &PileupAt(PathLevel lv);
  // One PathPileup (tile level) or ReadPileup call on DB chunk di for the hits
  // `items` (indices of Hits()), grouped by query chunk, over the chunk's
  // positions [p0, p1); adds the device's counters to stats_ (tile level) or
  // read_pileup_stats_.
  void PileupChunk(PathLevel lv, size_t di, const std::vector<size_t> &items, uint32_t p0, uint32_t p1,
                   uint32_t *depth, uint32_t *identities, uint8_t *consensus, uint32_t *shifts, uint32_t *profile);
  std::vector<uint32_t> SubjectProfileAt(PathLevel lv, const char *what, uint32_t db_id, bool count_only);
  // -y 10 / -y 11 (tile level), -y 16 / -y 17 (band level) and -y 18 / -y 19
  // (frame level, with shifts_sum): replaces the parts' text by one line per
  // subject with hits
  void FormatPileup(PathLevel lv, bool consensus);
  // -y 20 (frame false) and -y 21 (frame true): from the -y 12 / -y 13 text
  // already in the parts, per read the lines of its KEPT hits in kept_rank
  // order with two more columns, rank and covered; a read may span several
  // parts, so the text is assembled over the joined lines and replaces the
  // parts' text as FormatPileup's does
  void FormatCull(bool frame);
  // the cull's input record of final hit h from its read-level path x, and (key not null) the key of its read:
  // consecutive hits with one key are one read (ReadCull; ReadLca for the kept hits)
  GhostmCullHit CullRecord(bool frame, size_t h, const GhostmHit &hit, const GhostmHitPath &x, uint64_t *key) const;
  // -y 22 (frame false) and -y 23 (frame true): one line per read with hits, in
  // read order: qname, taxid, depth, votes, support, lca_taxid, candidates,
  // unmapped, best_score; replaces the parts' text as FormatPileup's does
  void FormatLca(bool frame);
  // -y 24 (frame false) and -y 25 (frame true): the sample's report (TaxonReport, taxon_profile.h); replaces the
  // parts' text as FormatLca does
  void FormatProfile(bool frame);
  // the common end of FormatPileup, FormatCull, FormatLca and FormatProfile: *out (taken) becomes the parts' whole text
  void ReplaceText(std::string *out);
  uint32_t SubjectLength(const DbData &d, uint32_t subject) const;

  AlignerOptions opt_;
  uint64_t shard_begin_ = 0, shard_end_ = UINT64_MAX;  // query range over the loaded chunks
  uint32_t shard_world_ = 1;
  bool db_only_ = false, no_db_ = false;
  double db_format_seconds_ = 0, db_code_seconds_ = 0;  // FormatDb's device time: the current database
  uint64_t db_format_launches_ = 0, db_sets_ = 0;
  double db_read_seconds_ = 0, db_load_seconds_ = 0;    // host: FASTA reading; packing, upload, subjects
  double format_seconds_ = 0;          // FormatQuery's device time, launches: the current set
  uint64_t format_launches_ = 0, query_sets_ = 0;
  double read_seconds_ = 0, load_seconds_ = 0;  // host: FASTA reading; packing, upload and read-back
  std::vector<QueryData> queries_;
  std::vector<GhostmQueryTile> tile_table_;  // a tiled set's table, by global query record; else empty
  std::vector<DbData> dbs_;
  uint32_t db_sum_u32_ = 0;           // DBReader::GetSumDbLength() truncates to u32
  uint64_t merge_epoch_ = 0;
  std::deque<Part> parts_;             // parts_[0, used_parts_) hold the last run
  size_t used_parts_ = 0;
  std::string joined_;
  bool joined_valid_ = false;
  std::vector<GhostmHit> hits_;
  bool hits_valid_ = false;
  std::vector<GhostmHitExt> hits_ext_;
  bool hits_ext_valid_ = false;
  // per hit, from HitsExt(): query chunk, DB chunk, the chunk-local query that
  // reproduced the hit, its absolute end and start
  struct HitSource {
    uint32_t qi, di, query, end, start;
  };
  std::vector<HitSource> hit_source_;
  std::vector<GhostmHitPath> hits_path_;
  std::vector<uint32_t> path_ops_;
  bool hits_path_valid_ = false;
  std::vector<GhostmHitRows> hits_rows_;
  std::vector<uint8_t> row_bytes_;
  bool hits_rows_valid_ = false;
  ReadLevelResult level_[2];  // the band paths [0] and the frame paths [1]
  std::vector<GhostmHitFrameInfo> frame_info_;  // beside level_[1]
  // Drops a level's results from a stage on: its paths with the rows, the
  // pile-up, the cull, the LCA and the profile made from them; or the cull,
  // its LCA and the profile; or the LCA and the profile. A new per-level result
  // joins this one list.
  enum LevelStage { kFromPaths, kFromCull, kFromLca };
  void DropLevel(int lv, LevelStage from = kFromPaths);
  // the read-level rows of the band paths [0] and of the frame paths [1]
  struct ReadRowsResult {
    std::vector<GhostmHitReadRows> rec;
    std::vector<uint8_t> bytes;
    bool valid = false;
    void Drop() {
      rec.clear();
      bytes.clear();
      bytes.shrink_to_fit();
      valid = false;
    }
  };
  ReadRowsResult read_rows_[2];
  GhostmReadRowsStats read_rows_stats_{};
  uint32_t band_ = 31;
  uint32_t tile_step_ = 0;  // a tiled set's step; 0 on an untiled set
  bool tile_dna_ = false;   // ... whether its sources are DNA frames (tiles six records apart)
  GhostmBandStats band_stats_{};
  std::vector<uint32_t> tile_read_nt_;  // a tiled set's kept letters (nt for DNA) by source record
  int frame_shift_ = -15;
  GhostmFrameStats frame_stats_{};
  ReadPileupResult pileup_[3];                  // by PathLevel; the tile pile-up's shifts stay empty
  std::vector<GhostmSubjectPileup> pileup_subj_;  // pileup_[kTileLevel].subj as 40-byte records
  GhostmReadPileupStats read_pileup_stats_{};
  ReadCullResult cull_[2];  // of the band paths [0] and of the frame paths [1]
  uint32_t cull_top_k_ = 1, cull_cover_pct_ = 50;
  GhostmReadCullStats cull_stats_{};
  bool tile_groups_ = false;
  MaskParams mask_;                 // SetMask: the next set's masking (window 0: off)
  GhostmMaskStats mask_stats_{};    // the current set's
  // masks chunk q (just formatted) by mask_: its sources, DeviceModule::MaskQuery; returns the device time
  double MaskChunk(QueryData *q, const std::vector<GhostmBandSource> &src, uint32_t step);
  struct Taxonomy {
    std::vector<uint32_t> taxid, parent, subject_node;
    std::vector<uint32_t> depth;  // per node (the report's column)
    uint64_t mapped = 0, map_unmatched = 0;
    uint64_t serial = 0;  // DeviceModule::taxonomy_serial() after this taxonomy's upload
    bool set = false;
  };
  Taxonomy tax_;
  ReadLcaResult lca_[2];  // of the band paths [0] and of the frame paths [1]
  uint32_t lca_top_pct_ = 10, lca_support_pct_ = 100;
  GhostmReadLcaStats lca_stats_{};
  bool mates_ = false;  // SetMates
  uint32_t mates_max_insert_ = 1000;
  PairJoinResult pair_[2];     // of cull_[0] and of cull_[1]
  PairLcaResult pair_lca_[2];  // of pair_[0] and of pair_[1]
  GhostmPairJoinStats pair_stats_{};
  std::string MatesRefusal() const;              // why a pair pass cannot run, or ""
  std::string SourceName(uint32_t record) const;  // a tiled set's source record's name
  // -y 26 (frame false) and -y 27 (frame true): one line per pair with a hit, named by mate 1's record: the -y 22
  // columns of the pair's record, then mates, joined, best_span; replaces the parts' text as FormatLca does
  void FormatPairLca(bool frame);
  // the tiled FASTA setters' common body; path2 (may be null): the mates' file, interleaved record by record
  void SetFastaTiled(const std::string &path1, const std::string *path2, uint32_t width, bool dna, uint32_t chunk_mb,
                     uint32_t max_len, uint32_t step, uint64_t *cut_records, bool *capped);
  QualParams qual_;                     // SetQuality: the next quality-carrying set's stage (all 0: off)
  std::vector<GhostmQualOut> qual_out_;  // the current set's, per source read
  GhostmQualStats qual_stats_{};
  AdapterParams adapter_;                       // SetAdapters: the next quality-carrying set's stage (off by default)
  std::vector<GhostmAdapterOut> adapter_out_;  // the current set's, per source read
  GhostmAdapterStats adapter_stats_{};
  // the quality setters' common body: one read set, or two of mates interleaved; their letters are masked in place
  void SetQualTiled(FastqSet *a, FastqSet *b, uint32_t width, bool dna, uint32_t chunk_mb, uint32_t max_len,
                    uint32_t step, uint64_t *cut_records, bool *capped, double read_seconds);
  TaxonProfileResult profile_[2];  // of lca_[0] and of lca_[1]; with mates on, of pair_lca_
  uint32_t profile_min_reads_ = 1;
  GhostmTaxonProfileStats profile_stats_{};
  bool records_on_device_ = false;
  GhostmStats stats_{};
  unsigned threads_ = 1;
  std::unique_ptr<TaskQueue> formatter_;
  std::unique_ptr<TaskQueue> writer_;  // streamed output (Run(true)), in part order
  int stream_fd_ = -1;
  bool run_sync_ = true;  // drain the streams at run and chunk starts (Run)
  std::vector<uint32_t> seed_counts_;  // K1 counts/offsets of the current chunk (RunQueryChunk)
  std::vector<uint64_t> seed_offsets_;
  uint64_t stream_off_ = 0;
  bool stream_failed_ = false, streamed_ = false;
  std::unique_ptr<LineFormat> format_;
};

}  // namespace ghostm
