/*
 * ghostm_hip.h — C ABI of the MI355X (gfx950) search/align plugin.
 *
 * Part 1 is the reference GPU plugin surface, symbol for symbol: GHOSTM 2.0's
 * aligner.cpp binds exactly these ten functions (reference aligner_gpu.h:33-114,
 * called from aligner.cpp:77-93, 110, 123-124, 356-361, 529-531, 211). A build of
 * the reference host that links libghostm_hip.so instead of aligner_gpu.o runs
 * its `-D <device>` path on this implementation unchanged.
 *
 * Part 2 extends the surface where the reference ABI cannot express the whole
 * hot path: a whole-query-set candidate count (needed to
 * reproduce the CPU path's batching exactly), a device traceback, error strings
 * instead of exit(), and a session API that runs the complete `aln` pipeline
 * (seed -> score -> merge -> traceback -> E-value) with inputs resident in HBM.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types. Host arrays are
 * owned by the caller; copies are synchronous unless stated. Int returns: 0 = OK,
 * non-zero = error (message via GhostmGetLastError). One device per process.
 */
#ifndef GHOSTM_HIP_H_
#define GHOSTM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- Part 1: reference plugin surface ------------------------ */

/* replaces aligner_gpu.h:37 InitGpu (aligner_gpu.cu:588) — reset module state */
int InitGpu(void);

/* replaces aligner_gpu.h:39-47 (aligner_gpu.cu:506) — device bytes the search
 * needs for the given maxima (counts this build's buffers, not the reference's) */
size_t GetNeededGPUMemorySize(uint32_t seed, uint32_t shift_size,
                              uint32_t max_list_length, uint32_t max_query_length,
                              uint32_t max_number_queries, uint32_t max_db_length);

/* replaces aligner_gpu.h:49-57 (aligner_gpu.cu:560) — 1 if it does not fit */
int CheckGpuMemory(uint32_t seed, uint32_t shift_size, uint32_t max_list_length,
                   uint32_t max_query_length, uint32_t max_number_queries,
                   uint32_t max_db_length);

/* replaces aligner_gpu.h:59-64 (aligner_gpu.cu:620) — bind device, upload the
 * 32x32 score matrix M[db_code*32 + query_code], size candidate buffers */
int SetOptionGpu(uint32_t max_list_length, int score_matrix[], int device);

/* replaces aligner_gpu.h:66 (aligner_gpu.cu:646) */
void printGpuInfo(int device);

/* replaces aligner_gpu.h:68-73 (aligner_gpu.cu:654) — upload a query chunk of
 * number_sequences fixed-width records of sequence_length codes */
int SetQueryGpu(uint8_t sequences[], uint32_t number_sequences, uint32_t sequence_length);

/* replaces aligner_gpu.h:75-83 (aligner_gpu.cu:691) — upload a DB chunk and its
 * k-mer index (keys_count = CSR offsets, positions = ascending per key) */
int SetDbGpu(uint8_t sequences[], uint32_t sequences_legnth, uint32_t keys_count[],
             uint32_t keys_count_length, uint32_t positions[], uint32_t positions_length);

/* replaces aligner_gpu.h:85-97 (aligner_gpu.cu:759) — seed search for the queries
 * from start_query_id on. Batches queries with the reference GPU rule (stop before
 * the running candidate total reaches max_number_alignments). Fills
 * alignment_count_list[0..q] (prefix counts) and starts[] (candidate DB starts,
 * ascending per query); returns q = number of queries in the batch. The starts
 * stay resident on the device for the next CalculateScoreGpu. */
uint32_t SearchNextGpu(uint32_t query_sequence_length, uint32_t number_query_sequences,
                       uint32_t seed, uint32_t threshold, uint32_t shift_size,
                       uint32_t log_region_size, uint32_t max_number_alignments,
                       uint32_t start_query_id, uint32_t *alignment_count_list,
                       uint32_t *starts);

/* replaces aligner_gpu.h:99-110 (aligner_gpu.cu:971) — Gotoh local score + end of
 * every candidate of the last SearchNextGpu batch */
void CalculateScoreGpu(uint32_t db_length, uint32_t query_sequence_length,
                       uint32_t number_alignment_list, uint32_t scores[], uint32_t ends[],
                       uint32_t base_search_length, uint32_t offset, int open_gap,
                       int extend_gap);

/* replaces aligner_gpu.h:112 (aligner_gpu.cu:1029) */
int FreeGpu(void);

/* ---------------- Part 2: extensions -------------------------------------- */

/* Last error message of this thread's most recent failing call ("" if none). */
const char *GhostmGetLastError(void);

/* Build identity (kernel variant names, arch), for logs. */
const char *GhostmBuildInfo(void);

/* Device blocks a destroyed session released stay cached for the next session
 * (at most GHOSTM_DEV_POOL_MB, default 8192 MB). An allocation that runs out of
 * memory empties the cache and retries once. GhostmDevicePoolTrim frees every
 * cached block now (for a caller that shares the device with other allocators)
 * and returns the bytes freed; GhostmDevicePoolInfo reports the cached bytes and
 * how many allocations were retried after emptying the cache. No reference
 * counterpart (the reference allocates per Aligner, aligner_gpu.cu). */
uint64_t GhostmDevicePoolTrim(void);
int GhostmDevicePoolInfo(uint64_t *cached_bytes, uint64_t *oom_retries);

/* Candidate count of EVERY query of the resident chunk (no batching), K1 count
 * pass; counts[number_query_sequences]. Lets a host reproduce the CPU path's
 * batch cuts exactly (reference aligner.cpp:511-514). */
int CountCandidatesGpu(uint32_t query_sequence_length, uint32_t number_query_sequences,
                       uint32_t seed, uint32_t threshold, uint32_t shift_size,
                       uint32_t log_region_size, uint32_t counts[]);

/* Reverse-DP traceback (reference aligner.cpp:771-949) of nhits hits on the
 * resident query/DB chunk: per hit (query_id, db_end) -> db_start (absolute),
 * aln_len, aln_match, seq_id = match/len (float). base_search_length is the
 * reference's L + 2*e*2*R window. */
int TraceBackGpu(uint32_t nhits, const uint32_t query_ids[], const uint32_t db_ends[],
                 uint32_t query_sequence_length, uint32_t base_search_length,
                 int open_gap, int extend_gap, uint32_t db_starts[], uint32_t aln_lens[],
                 uint32_t aln_matches[], float seq_ids[]);

/* What the BLAST-tabular columns need beyond a GhostmHit (16 bytes): where the
 * alignment lies in the query, its mismatches and its gap opens. Zero-based,
 * "as printed minus one" like the GhostmHit coordinates. For a DNA query the
 * query coordinates count residues of the translated frame record. */
typedef struct GhostmHitExt {
  uint32_t q_start;     /* query row of the first maximal cell of the reverse DP */
  uint32_t q_end;       /* query row the path to that cell began in */
  uint32_t mismatches;
  uint32_t gap_opens;
} GhostmHitExt;

/* TraceBackGpu plus one GhostmHitExt per hit (kernel k_traceback_ext). The
 * reference's traceback keeps, per H cell, the alignment length and matches of
 * the H cell it steps from (also for its E and F chains); the extension carries
 * mismatches, gap opens (a gap step opens a gap unless that H cell was reached
 * by the same kind of gap step) and the path's first query row by the same
 * rule, so aln_len = aln_match + mismatches + gap residues. db_starts,
 * aln_lens and aln_matches are TraceBackGpu's. db_starts_in may be NULL; with
 * the hits' known starts each DP stops at its first maximal column (same
 * results, fewer columns). Fails (no wrapped field) when query_sequence_length
 * > 127 or query_sequence_length + base_search_length >= 32768. */
int TraceBackExtGpu(uint32_t nhits, const uint32_t query_ids[], const uint32_t db_ends[],
                    const uint32_t db_starts_in[], uint32_t query_sequence_length,
                    uint32_t base_search_length, int open_gap, int extend_gap, uint32_t db_starts[],
                    uint32_t aln_lens[], uint32_t aln_matches[], GhostmHitExt ext[]);

/* The same on the host, with no device call (the model the kernel is checked
 * against): query_seqs = nq records of L codes, db = db_len END-separated
 * codes, score_matrix = 32x32 M[db_code*32 + query_code]. Output arrays may be
 * NULL. */
int GhostmTraceBackExtHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                           uint32_t db_len, const int score_matrix[], uint32_t nhits,
                           const uint32_t query_ids[], const uint32_t db_ends[],
                           uint32_t base_search_length, int open_gap, int extend_gap,
                           uint32_t db_starts[], uint32_t aln_lens[], uint32_t aln_matches[],
                           GhostmHitExt ext[]);

/* The alignment path of one hit: which query residue lies against which
 * subject residue. Coordinates are zero-based and inclusive; the path's
 * operations are the n_runs run-length words at ops[ops_offset]: length << 4 |
 * op, op 0 '=' (equal codes), 1 'X' (different codes), 2 'I' (a query residue
 * against a gap), 3 'D' (a subject residue against a gap), in reading order of
 * both sequences. s_end is the path's last subject residue; it may lie before
 * the hit's db_end, which is where the forward search stopped. A hit of score
 * 0 has an empty path (n_runs 0, the end coordinates equal the start's). */
typedef struct GhostmHitPath {
  uint32_t q_start, q_end;   /* first and last query row of the path */
  uint32_t s_start, s_end;   /* first and last subject position of the path */
  uint32_t score;            /* H of the first maximal cell */
  uint32_t n_runs;
  uint64_t ops_offset;       /* index of the hit's first word in ops[] */
} GhostmHitPath;

/* The path of every hit (kernels k_tb_path_fill + k_tb_path_walk), stage level
 * like TraceBackExtGpu (after SetQueryGpu and SetDbGpu; subject coordinates
 * absolute in the chunk). The DP is TraceBackExtGpu's; every cell records the
 * term its H took (0, diagonal, E, F, each comparison strict in that order)
 * and whether its E and F extended or opened (a tie opens), and the path is
 * walked from the first strict maximum, in H state, towards column 0 and row
 * L - 1. Record i belongs to hit i; the hits' words follow each other in hit
 * order. ops == NULL: only *ops_used (the words needed) and rec (may be NULL)
 * are written. Fails when ops_cap is too small, when query_sequence_length >
 * 127 or query_sequence_length + base_search_length >= 32768. The direction
 * buffer (4 bits per cell) is cut into batches of hits that fit
 * GHOSTM_PATH_SCRATCH_MB (default 1024) and hold at most GHOSTM_PATH_BATCH_HITS
 * hits (default: no limit). */
int TraceBackPathGpu(uint32_t nhits, const uint32_t query_ids[], const uint32_t db_ends[],
                     const uint32_t db_starts_in[], uint32_t query_sequence_length,
                     uint32_t base_search_length, int open_gap, int extend_gap, GhostmHitPath rec[],
                     uint32_t ops[], size_t ops_cap, size_t *ops_used);

/* The same on the host, with no device call (the model the kernels are checked
 * against); arguments as GhostmTraceBackExtHost, db_starts_in may be NULL. */
int GhostmTraceBackPathHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                            uint32_t db_len, const int score_matrix[], uint32_t nhits,
                            const uint32_t query_ids[], const uint32_t db_ends[],
                            const uint32_t db_starts_in[], uint32_t base_search_length, int open_gap,
                            int extend_gap, GhostmHitPath rec[], uint32_t ops[], size_t ops_cap,
                            size_t *ops_used);

/* The alignment of one hit as text: its 3 * columns bytes at rows[rows_offset]
 * are the query row, the midline and the subject row, each columns bytes long
 * and without a terminator. The letter of residue code c is
 * "ARNDCQEGHILKMFPSTWYVBJZX*"[c]; codes of 25 and above give '?'. A '=' or 'X'
 * column holds both letters, an 'I' column the query letter and '-' in the
 * subject row, a 'D' column '-' in the query row and the subject letter. The
 * midline holds the query letter in a '=' column, '+' in an 'X' column whose
 * matrix entry M[db code * 32 + query code] is > 0, and a space elsewhere (the
 * matrix is indexed with the codes' low five bits). */
typedef struct GhostmHitRows {   /* 32 bytes */
  uint32_t query_record;  /* the query record the path lies in: stage level = query_ids[i]; session level =
                             its global index over the session's query chunks in order. For a DNA set,
                             query_record % 6 is the frame: 0..2 forward +0 +1 +2, 3..5 reverse complement
                             +0 +1 +2 */
  uint32_t columns;       /* the path's columns: the sum of its words' lengths */
  uint32_t identities;    /* '=' columns */
  uint32_t positives;     /* '=' and 'X' columns whose matrix entry is > 0 (an identical pair with a
                             non-positive score, such as X/X, is not one) */
  uint32_t gap_residues;  /* 'I' and 'D' columns */
  int32_t rescore;        /* the pair columns' matrix entries plus, per word of 'I' or 'D', open_gap for its
                             first column and extend_gap for every further one (both negative); equals
                             GhostmHitPath.score for a path TraceBackPathGpu made */
  uint64_t rows_offset;   /* first byte of the hit's 3 * columns bytes in rows[] */
} GhostmHitRows;

/* The rows of every hit (kernel k_path_rows), stage level like TraceBackPathGpu
 * (after SetQueryGpu and SetDbGpu): hit i lies in query record query_ids[i],
 * rec[i] gives its first query row, its first subject position (absolute in
 * the chunk) and its n_runs words at ops[ops_offset]; q_end, s_end and score
 * are not read. Any well-formed path is accepted, not only one a traceback
 * made. Record i belongs to hit i; the hits' bytes follow each other in hit
 * order. rows == NULL: only *rows_used (the bytes needed) and out (may be NULL)
 * are written. A path without words gives columns 0, counts 0 and no bytes.
 * Everything is checked on the host before any upload or launch; a refused
 * call leaves out, rows and *rows_used untouched and names its reason in
 * GhostmGetLastError:
 *   "ops"      ops_offset + n_runs > ops_len
 *   "word"     a word with bits 2-3 set or a zero length
 *   "bounds"   a path whose query residues run past query_sequence_length or
 *              whose subject residues run past the resident DB chunk
 *   "query"    a query_ids[i] outside the resident chunk
 *   "rows_cap" rows_cap smaller than the bytes needed
 * The row buffer is cut into batches of hits that fit GHOSTM_ROWS_SCRATCH_MB
 * (default 1024) and hold at most GHOSTM_ROWS_BATCH_HITS hits (default: no
 * limit); a batch holds at least one hit. */
int PathRowsGpu(uint32_t nhits, const uint32_t query_ids[], const GhostmHitPath rec[],
                const uint32_t ops[], size_t ops_len, uint32_t query_sequence_length,
                int open_gap, int extend_gap, GhostmHitRows out[], uint8_t rows[],
                size_t rows_cap, size_t *rows_used);

/* The same on the host, with no device call (the model the kernel is checked
 * against) and the same checks: query_seqs = nq records of L codes, db = the
 * chunk's db_len residues, score_matrix = M[db code * 32 + query code];
 * query_sequence_length must equal L. */
int GhostmPathRowsHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                       uint32_t db_len, const int score_matrix[], uint32_t nhits,
                       const uint32_t query_ids[], const GhostmHitPath rec[], const uint32_t ops[],
                       size_t ops_len, uint32_t query_sequence_length, int open_gap, int extend_gap,
                       GhostmHitRows out[], uint8_t rows[], size_t rows_cap, size_t *rows_used);

/* The subject pile-up: what a set of hits says about every position of a DB
 * chunk. All of it is integer sums, so a result does not depend on the order
 * of the hits or of the additions. With slot(c) = c for c < 25 and 25
 * otherwise, a profile row is 32 uint32_t per position p:
 *   a '=' or 'X' column at p adds 1 to profile[p][slot(query code)]
 *   a 'D' column at p adds 1 to profile[p][26]
 *   an 'I' column touches no subject position and adds nothing
 *   slots 27..31 stay 0
 *   depth[p]      = the sum of slots 0..26
 *   identities[p] = profile[p][slot(db[p])]
 *   consensus[p]  = the slot in 0..24 with the largest count, the lowest slot
 *                   winning a tie; 255 when slots 0..24 are all zero
 * A hit with an empty path adds nothing.
 *
 * PathPileupGpu (kernels k_pileup and k_pileup_finish) is stage level like
 * PathRowsGpu (after SetQueryGpu and SetDbGpu) and takes the same hits:
 * query_ids[i], rec[i] (q_start, s_start absolute in the chunk, n_runs words at
 * ops[ops_offset]). db_len must be the resident chunk's length; depth,
 * identities and consensus hold db_len elements, profile db_len * 32 or is
 * NULL. nhits == 0 gives zeros and 255s. Everything is checked on the host
 * before any upload or launch; a refused call leaves every output untouched
 * and names its reason in GhostmGetLastError: PathRowsGpu's "ops", "word",
 * "bounds" and "query", "db_len" when db_len is not the resident chunk's
 * length, and "null" for a null depth, identities or consensus, or null hit
 * arrays with nhits > 0.
 * The chunk's positions are cut into tiles of GHOSTM_PILEUP_TILE positions
 * (32..256, default 256) and every tile's hits into parts of
 * GHOSTM_PILEUP_PART_HITS hits (default 512), one workgroup per (tile, part);
 * the profile exists on the device one window of whole tiles at a time, a
 * window fitting GHOSTM_PILEUP_SCRATCH_MB (default 1024; a position costs
 * 128 bytes), so a chunk may be far larger than device memory / 128. Hits and
 * words are uploaded in batches of at most GHOSTM_PILEUP_BATCH_HITS hits. */
int PathPileupGpu(uint32_t nhits, const uint32_t query_ids[], const GhostmHitPath rec[],
                  const uint32_t ops[], size_t ops_len, uint32_t query_sequence_length,
                  uint32_t db_len, uint32_t depth[], uint32_t identities[], uint8_t consensus[],
                  uint32_t profile[]);

/* The same on the host, with no device call (the model the kernels are checked
 * against) and the same checks and reasons; the argument head is
 * GhostmPathRowsHost's (score_matrix is not read and may be NULL). */
int GhostmPathPileupHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                         uint32_t db_len, const int score_matrix[], uint32_t nhits,
                         const uint32_t query_ids[], const GhostmHitPath rec[], const uint32_t ops[],
                         size_t ops_len, uint32_t query_sequence_length, uint32_t depth[],
                         uint32_t identities[], uint8_t consensus[], uint32_t profile[]);

/* One subject's summary of the session-level pile-up (GhostmSessionPileup). */
typedef struct GhostmSubjectPileup {   /* 40 bytes */
  uint32_t length;          /* the subject's residues */
  uint32_t hits;            /* hits on it, those with an empty path included */
  uint32_t covered;         /* positions with depth > 0 */
  uint32_t max_depth;
  uint64_t depth_sum;
  uint64_t identities_sum;
  uint64_t offset;          /* the subject's first element in the session-level arrays */
} GhostmSubjectPileup;

/* The `db` formatter's k-mer index of one DB chunk, built on the GPU
 * (replaces DBCreator::ConstructIndex, db_creator.cpp:167-241).
 * seq[len] = the chunk's END-separated residues (.seq); seed = the index seed mask
 * (db -k k -> 2^k - 1); kcl = 32^weight(seed) + 1. Fills keys_count[kcl] (CSR
 * offsets) and positions[*npos] (ascending per key; the array must hold len
 * entries) byte-identical to the CPU formatter's .ind. device_ms (optional)
 * receives the device time of the build (HIP events, after the upload). */
int GhostmBuildIndexGpu(const uint8_t *seq, uint32_t len, uint32_t seed, uint32_t kcl,
                        uint32_t *keys_count, uint32_t *positions, uint32_t *npos, int device,
                        float *device_ms);

/* The `qry` formatter's per-residue work on the GPU (replaces QueryCreator's
 * coding, query_creator.cpp:388-423, and six-frame translation, :242-324;
 * SURVEY.md §8 f2). raw[raw_len] = the chunk's records' letters concatenated
 * (no newlines); record r is raw[offsets[r] .. + lengths[r]). dna_len = 0:
 * protein, records[n * width] = each record's residue codes, cut at or X-padded
 * to width. dna_len > 0: DNA reads cut/padded to dna_len letters (the reference
 * uses the chunk's first read length), records[6n * width] = per read the
 * frames +0 +1 +2 and the reverse complement's +0 +1 +2 with stop codons
 * masked to '*' until the next ATG, each cut/X-padded to width. Byte-identical
 * to the CPU formatter's .seq. device_ms (optional) = the kernel time. */
int GhostmFormatQueriesGpu(const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets,
                           const uint32_t *lengths, uint32_t n, uint32_t width, uint32_t dna_len,
                           uint8_t *records, int device, float *device_ms);

/* General Karlin-Altschul parameters. The reference `aln` knows
 * only two gapped parameter sets (statistics.cpp:134-146); its vendored routines
 * compute ungapped ones for any matrix. GhostmKarlinUngapped restates
 * Statistics::CalculateUngappedIdealKarlinParameters (statistics.cpp:100-112,
 * Robinson & Robinson background) with BlastKarlinBlkCalc (karlin.cpp:16-32) on
 * a 32x32 matrix M[db_code*32 + query_code]; the floats are bit-identical to the
 * reference's. `aln` uses them for E-values of matrix/gap combinations outside
 * the table when GHOSTM_KARLIN=ungapped is set (otherwise the reference's error). */
int GhostmKarlinUngapped(const int score_matrix[], float *lambda, float *K, float *H);

/* The 32x32 matrix `aln -M path` scores with (ScoreMatrixReader::Read,
 * score_matrix_reader.cpp:44-113: built-in BLOSUM62 when the path cannot be
 * opened), row-major M[db_code*32 + query_code]; the input GhostmKarlinUngapped takes. */
int GhostmReadScoreMatrix(const char *path, int score_matrix[]);

/* BlastComputeLengthAdjustment (karlin.cpp:393-476): the edge-effect length
 * adjustment; returns 0 when the iteration converged, 1 otherwise, as the
 * reference. */
int GhostmLengthAdjustment(float K, float logK, float alpha_d_lambda, float beta, int query_length,
                           uint32_t db_length, int db_num_seqs, int *length_adjustment);

/* One resolved hit, the record gathered across ranks (32 bytes). Coordinates are
 * subject-relative, as printed minus one. */
typedef struct GhostmHit {
  uint32_t query_id;   /* global query index over all chunks */
  uint32_t db_id;      /* global subject index over all DB chunks */
  uint32_t score;
  uint32_t db_start;
  uint32_t db_end;
  uint32_t aln_len;
  uint32_t aln_match;
  float seq_id;
} GhostmHit;

/* Stage timings / work counters of the last GhostmSessionRun. */
typedef struct GhostmStats {
  double seconds_total;      /* whole run, host wall clock */
  double seconds_seed;       /* K1 count + write passes (device time) */
  double seconds_score;      /* K2 (device time) */
  double seconds_traceback;  /* K3 (device time) */
  double seconds_merge;      /* host Merge (sort/dedup/select) */
  double seconds_output;     /* host E-value + text formatting */
  uint64_t queries;
  uint64_t query_residues;   /* sum over queries of non-X prefix length */
  uint64_t candidates;
  uint64_t score_cells;      /* sum over candidates of L x window columns W (END columns included: the
                                reference's CalculateScore loop visits them, aligner.cpp:576-660) */
  uint64_t tracebacks;       /* hits traced back (K3), new selections only */
  uint64_t traceback_cells;
  uint64_t hits;
  uint64_t batches;
  uint64_t score_launches;
  uint64_t seed_bytes;       /* algorithmic bytes of the K1 passes */
  uint64_t score_launches_packed; /* K2 launches that ran a packed 16-bit kernel */
  uint64_t score_launches_half;   /* ... of which the f16 encoding */
  uint64_t traceback_launches;
  uint64_t traceback_launches_key; /* K3 launches that ran the key formulation */
  uint64_t seed_runs_hash;        /* K1 runs whose slot pass used the hash-count kernel */
  uint64_t score_rechecks;        /* guarded f16 K2 candidates re-scored exactly in int16 */
  uint64_t traceback_launches_scan; /* K3 launches preceded by the scores-only scan (K3a) */
  uint64_t traceback_scan_cells;    /* K3a: sum over hits of L x reverse-window columns */
  uint64_t merge_launches;          /* K4 launches */
  uint64_t merge_launches_wave;     /* ... that ran one wave per name group (k_merge_wave) */
  uint64_t score_launches_framed;   /* f16 K2 launches of the column-framed kernel (k_score16f) */
  uint64_t seed_queries_class[4];   /* K1 queries per size class by list entries (3 = global merge) */
  uint64_t seed_queries_wide;       /* K1 queries with more candidates than a slot (offset pass) */
  uint64_t segments;                /* device-merge segments (K2 -> K4 -> K3 rounds) */
  uint64_t seed_runs_filter;        /* K1 runs whose classes 0/1 used the presence-filtered table */
  uint64_t seed_filter_overflows;   /* ... queries whose filter queue overflowed (redone unfiltered) */
  uint64_t score_launches_swar;     /* framed K2 launches over 16-bit integer patterns (k_score16f<S, true>) */
  uint64_t traceback_launches_scan_swar; /* K3a scans over 16-bit integer patterns (k_tb_scan<..., true>) */
  uint64_t seed_list_entries;       /* K1: sum over queries of the k-mer position-list lengths */
  uint64_t score_launches_unit;     /* framed integer-pattern K2 launches with unit-pair profile words (k_score16f<S, true, true>) */
  uint64_t traceback_launches_strips; /* K3 key DPs run by strip class (each hit on the strips up to its first maximal cell) */
  double seconds_traceback_scan;    /* of seconds_traceback: the scan phase (k_tb_prep, k_tb_pairs, the sorts,
                                       k_tb_scan); the rest is the key DP (k_traceback_key) */
  uint64_t score_launches_pair;     /* K2 launches of sparse segments run by the pair-table kernel (k_score_pair) */
  uint64_t seed_table_full;         /* K1 queries whose LDS bin table reached its probe bound (redone by the
                                       table-free merge kernel) */
  uint64_t seed_compact_redo;       /* K1 compactions re-run by the host (queue overflow, candidate buffers grown) */
  uint64_t score_launches_sparse;   /* K2 launches of sparse segments run by the 16-row profile kernel (k_score16f<16, true>,
                                       seven query profiles per block) */
  uint64_t traceback_launches_keyframe; /* K3 key DPs run with the column-framed E chain (k_traceback_key FRAME) */
  uint64_t score_launches_levels;   /* K2 launches of the 16-bit-row integer-pattern kernel with restart levels
                                       (k_score16f<S, true, false, true>) */
  double seconds_traceback_ext;     /* the extended traceback post-pass (k_traceback_ext, device time); 0 until
                                       -y 6 or GhostmSessionHitsExt asks for it */
  uint64_t traceback_ext_launches;
  uint64_t traceback_ext_cells;     /* sum over its DPs of L x processed columns */
  double seconds_traceback_path;    /* the alignment-path post-pass (k_tb_path_fill + k_tb_path_walk, device
                                       time); 0 until -y 7 or GhostmSessionHitsPath asks for it */
  uint64_t traceback_path_launches; /* batches of hits (one fill and one walk launch each) */
  uint64_t traceback_path_cells;    /* sum over its DPs of L x processed columns */
  uint64_t traceback_path_dir_bytes; /* direction-buffer bytes its batches addressed */
  double seconds_query_format;      /* the resident query formatting (k_qry_protein / k_qry_frames with the
                                       record lengths, device time) of the last GhostmSessionSetQueries*; 0 for
                                       a query set read from formatted files */
  uint64_t query_format_launches;   /* ... its launches (one per query chunk) */
  uint64_t query_sets;              /* GhostmSessionSetQueries* calls that replaced the set, since creation */
  double seconds_query_read;        /* ... of the last one, host wall clock: reading the FASTA file and cutting
                                       it into chunks (0 for GhostmSessionSetQueries) */
  double seconds_query_load;        /* ... packing the letters, the names and name groups, the staged upload and
                                       the lengths' read-back, without seconds_query_format */
  double seconds_path_rows;         /* the aligned-rows post-pass (k_path_rows, device time); 0 until -y 8, -y 9
                                       or GhostmSessionHitsRows / GhostmSessionRowBytes asks for it */
  uint64_t path_rows_launches;      /* batches of hits (one launch each) */
  uint64_t path_rows_columns;       /* sum of the hits' columns */
  uint64_t path_rows_bytes;         /* row bytes written: 3 x path_rows_columns */
  double seconds_pileup;            /* the pile-up post-pass (k_pileup and k_pileup_finish, device time); 0, like
                                       the four below, until -y 10, -y 11 or GhostmSessionPileup /
                                       GhostmSessionPileupArrays / GhostmSessionSubjectProfile asks for it */
  uint64_t pileup_launches;         /* k_pileup launches */
  uint64_t pileup_windows;          /* profile windows zeroed and finished */
  uint64_t pileup_parts;            /* (tile, part) workgroups */
  uint64_t pileup_columns;          /* '=', 'X' and 'D' columns charged; after one GhostmSessionPileup the sum
                                       of the subjects' depth_sum */
} GhostmStats;

/* Session: parse `aln` options exactly like the reference (getopt string
 * "b:d:D:e:E:G:i:l:M:o:r:s:t:S:L:y:v", aligner.cpp:225-345; argv[0] is ignored),
 * load every query and DB chunk and make them resident on the device given by
 * -D (default 0). Returns NULL on error. */
void *GhostmSessionCreate(int argc, char **argv);

/* A database session: `aln`'s options without -i, -S and -L (giving one is an
 * error); every DB chunk is loaded and made resident, with no queries.
 * GhostmSessionRun before any query set gives empty output and no hits. The
 * queries come from GhostmSessionSetQueries / GhostmSessionSetQueriesFasta, any
 * number of times: many read sets against one resident database. Returns NULL
 * on error. */
void *GhostmSessionCreateDb(int argc, char **argv);

/* Replaces the session's query set by n records given as letters: record r is
 * raw[offsets[r] .. offsets[r] + lengths[r]), names holds the n names, each
 * terminated by '\n'. width is given as `qry -l`, dna as `qry -t d`, chunk_mb
 * as `qry -L` (0: qry's default). Afterwards the session holds what a session
 * created with -i P would hold after `ghostm qry -i <that FASTA> -o P -l width
 * [-t d] -L chunk_mb`: the same chunk cuts (the halved limit for DNA), the same
 * width (a third for DNA, at most 127), DNA reads cut or padded to their
 * chunk's first read length and translated in six frames under the read's name,
 * records cut at the width. The letters are coded on the device straight into
 * the resident chunks; only the records' lengths come back. The results of the
 * previous run are dropped and the old chunks' device memory is kept for
 * re-use; the DB chunks, the matrix and the options are untouched. Works on
 * any unsharded session; fails on a shard session and on null arguments,
 * which leaves the session as it was (as does a record outside the letter
 * buffer or a file that cannot be opened); after a failure while the set is
 * being loaded the session holds no queries. Returns 0 on success. */
int GhostmSessionSetQueries(void *session, const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets,
                            const uint32_t *lengths, const char *names, uint64_t names_len, uint32_t n,
                            uint32_t width, int dna, uint32_t chunk_mb);

/* The same from a FASTA file, read as `ghostm qry` reads it. cut_records (may
 * be NULL) receives the number of output records over the width, for each of
 * which qry prints a warning; the library prints nothing. */
int GhostmSessionSetQueriesFasta(void *session, const char *path, uint32_t width, int dna, uint32_t chunk_mb,
                                 uint64_t *cut_records);

/* The -o path of later GhostmSessionRunToFile and GhostmSessionWrite calls. */
int GhostmSessionSetOutputFile(void *session, const char *path);

/* The length `aln` prints for every query record (index of the last non-X code
 * + 1, at least 1), over the session's chunks in order; the NULL/cap convention
 * of GhostmSessionHits. */
size_t GhostmSessionQueryLengths(void *session, uint32_t *qlen, size_t cap);

/* The coded records of query chunk `chunk` (the bytes of its .seq file) copied
 * back from the device; same convention, (size_t)-1 on error. */
size_t GhostmSessionQueryRecords(void *session, uint32_t chunk, uint8_t *codes, size_t cap);

/* qry's chunk cuts on their own (host only, no device): over n records of the
 * given letter counts, with `qry -L chunk_mb` (0: the default) and -t d when
 * dna. Chunk c is records [cuts[c], cuts[c + 1]). Returns the number of chunks
 * (cuts[0..chunks] written while they fit cap entries), or -1 when a record
 * alone is over the limit (qry's "too small max length"). */
int64_t GhostmQueryChunkCuts(const uint32_t lengths[], uint64_t n, uint32_t chunk_mb, int dna, uint64_t cuts[],
                             uint64_t cap);

/* Tiled query sets: reads longer than one record of W letters (the width rule
 * above: at most 127) enter the search as overlapping W-letter tile records
 * under the read's name, instead of losing every letter past W. A source is a
 * protein record's kept letters or one frame of a DNA read (n / 3 letters);
 * with m letters and 1 <= step <= W it becomes
 *   tiles = 1 when m <= W, else 1 + ceil((m - W) / step)
 * records, tile t starting at letter t x step, the last one flush right at
 * max(m - W, 0): every tile of a long source is full width, consecutive tiles
 * overlap by at least W - step letters, and every window of at most
 * W - step + 1 letters lies wholly inside some tile. A protein record's tiles
 * are consecutive records; a DNA read's are tile-major and frame-minor (read
 * base + 6 t + f), so a read of one tile gives the six records of the untiled
 * setter. Each DNA read is translated at its own kept length, every frame once
 * over its whole length with the stop/ATG state carried along it; a tile is a
 * window of that frame. A tile is searched, scored and priced as a query of its
 * own (its own length in the E-value), exactly as a frame record is; the name
 * group merges a read's tiles into one result list. An alignment longer than
 * W - step + 1 residues may be reported truncated to a tile by the hit records
 * and the per-tile detail passes (-y 6 to 11): tiles are not stitched there.
 * The read-level alignment of a hit, over the whole read or frame, comes from
 * GhostmSessionHitsBand / -y 12 (BandAlignGpu below).
 *
 * One entry per output record, in output order. */
typedef struct GhostmQueryTile {
  uint32_t record;  /* index of the source record in the set given */
  uint32_t offset;  /* the tile's first letter in the record (protein) or in the frame (DNA) */
  uint32_t letters; /* the source's letter count m: the record's kept letters, or n / 3 of the read's kept n */
  uint32_t frame;   /* 0 for protein; DNA: 0..2 forward, 3..5 reverse complement */
} GhostmQueryTile;

/* GhostmSessionSetQueries with tiles. max_len (letters, nt for DNA; 0: no cut)
 * cuts every record first; step is the tile step in letters of the record or
 * frame. The chunk cuts are GhostmQueryChunkCuts' over the kept letters, and a
 * record's tiles never straddle a chunk. One source record may become at most
 * 1024 output records (1024 protein tiles, 170 tiles x 6 frames). The contract
 * of GhostmSessionSetQueries otherwise; step 0, step over the width, a record
 * over that limit, and a chunk whose row count or bytes would wrap a 32-bit
 * field are refused too and leave the session as it was. On a tiled set the
 * query coordinates of the -y 6, 7, 8 and 9 text are in read coordinates (the
 * tile's plus its offset); the structs (GhostmHitExt, GhostmHitPath,
 * GhostmHitRows) stay relative to the tile, the record
 * GhostmHitRows.query_record names, whose offset GhostmSessionQueryTiles gives. */
int GhostmSessionSetQueriesTiled(void *session, const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets,
                                 const uint32_t *lengths, const char *names, uint64_t names_len, uint32_t n,
                                 uint32_t width, int dna, uint32_t chunk_mb, uint32_t max_len, uint32_t step);

/* The same from a FASTA file (the whole file is read before the first chunk is
 * made, so every refusal leaves the session as it was). cut_records (may be
 * NULL) receives what the untiled setter would count for a set cut at max_len:
 * one per record cut, six per DNA read cut; 0 when max_len is 0. */
int GhostmSessionSetQueriesFastaTiled(void *session, const char *path, uint32_t width, int dna, uint32_t chunk_mb,
                                      uint32_t max_len, uint32_t step, uint64_t *cut_records);

/* The tile table of the session's query set, one entry per query record over
 * the chunks in order (the indexing of GhostmSessionQueryLengths and of
 * GhostmHitRows.query_record); the NULL/cap convention of GhostmSessionHits.
 * 0 entries on a set that was not made by a tiled setter. */
size_t GhostmSessionQueryTiles(void *session, GhostmQueryTile *tiles, size_t cap);

/* The tile plan on its own (host only, no device): the table a tiled setter
 * would make of n records of the given letter counts, with width, dna, max_len
 * and step as given to it. Returns the number of output records (tiles[0..]
 * written while they fit cap entries; tiles may be NULL), or -1 on what the
 * setter refuses (step, a record over the per-record limit). cut_records (may be
 * NULL) as above. */
int64_t GhostmQueryTilePlan(const uint32_t lengths[], uint64_t n, uint32_t width, int dna, uint32_t max_len,
                            uint32_t step, GhostmQueryTile tiles[], uint64_t cap, uint64_t *cut_records);

/* Read-level alignments: a banded Gotoh DP with traceback over a whole source
 * (a protein record's kept letters, or one frame of a DNA read), however many
 * tile records it was cut into, against one subject range. This is the step
 * from "which tile hit which subject where" to "how does the read align to
 * that subject"; the per-tile paths of TraceBackPathGpu stay as they are.
 *
 * Per hit: the source's m letters q[0..m), read through its tile records
 * (letter p lies in tile t = min(p / step, tiles - 1), record first_record +
 * stride * t, byte p - start(t) with the tile starts above); the subject range
 * [s_lo, s_hi], absolute in the resident DB chunk and free of END codes (the
 * caller gives a subject's own residues); the anchor diagonal D (signed); the
 * band half-width B, 1..31. The band cells are (i, j) with 0 <= i < m, s_lo <=
 * j <= s_hi and |j - i - D| <= B. All arithmetic is int32. The DP runs in
 * reverse like GhostmTraceBackPathHost, rows i = m-1 .. 0 and j descending in a
 * row, so the walk is forward in both sequences:
 *   s      = H(i+1,j+1) + M[(db[j] & 31) * 32 + (q[i] & 31)]
 *   E(i,j) = max(E(i,j+1) + ext, H(i,j+1) + open)    'D': db[j] against a gap
 *   F(i,j) = max(F(i+1,j) + ext, H(i+1,j) + open)    'I': q[i] against a gap
 *   H(i,j) = s if s > 0 else 0; then E if E > H; then F if F > H (each strict,
 *            in that order: hsel 1 / 0, 2, 3)
 *   eext   = E(i,j+1) + ext > H(i,j+1) + open (a tie opens); fext likewise
 * A neighbour that is no band cell has H = 0 and E, F = minus infinity (no gap
 * extends from it). The start cell is the first strict maximum in processing
 * order: among the cells of maximal H the largest i, then the largest j. From
 * it the three-state walk of TraceBackPathGpu: H with hsel 1 emits '=' / 'X'
 * and goes to (i+1, j+1); hsel 2 / 3 enter E / F at the same cell; E emits 'D'
 * and goes to (i, j+1), F emits 'I' and goes to (i+1, j), staying in the gap
 * state if eext / fext; hsel 0 or leaving the band cells stops. The result is a
 * GhostmHitPath and run-length words in its encoding; q_start / q_end are in
 * source coordinates (they may exceed 127), s_* absolute in the chunk. Score 0
 * gives an empty path at q_start = 0, s_start = s_lo with the ends equal to the
 * starts. Limits: B <= 31 (one wave lane per diagonal); open_gap <= extend_gap
 * <= 0 (the kernel resolves a row's E chain with a max-plus scan, which equals
 * the sequential recurrence exactly under this condition; the reference's 11/1,
 * 9/1 and 14/2 meet it). */
typedef struct GhostmBandSource {          /* 16 bytes */
  uint32_t first_record;                   /* tile 0 of this source in the resident query chunk */
  uint32_t stride;                         /* records between consecutive tiles: 1, or 6 for a DNA frame; ignored
                                              when tiles == 1 */
  uint32_t tiles;                          /* must equal the tile count of letters, W and step */
  uint32_t letters;                        /* m, at least 1 */
} GhostmBandSource;

/* The read-level path of every hit (kernels k_band_fill<false> + k_band_walk<false>), stage
 * level like TraceBackPathGpu (after SetQueryGpu and SetDbGpu);
 * query_sequence_length is the records' width W, step the tile step. Record i
 * belongs to hit i; the hits' words follow each other in hit order. ops ==
 * NULL: only *ops_used (the words needed) and rec (may be NULL) are written.
 * Everything is checked on the host before any upload or launch; a refused call
 * leaves rec, ops and *ops_used untouched and names its reason in
 * GhostmGetLastError:
 *   "source"  a record outside the chunk; tiles == 0 or letters == 0; tiles
 *             disagrees with letters, W and step; step 0 or over W; W differs
 *             from the resident chunk's
 *   "band"    band outside 1..31
 *   "bounds"  s_lo > s_hi or s_hi >= the resident chunk's length
 *   "gaps"    not open_gap <= extend_gap <= 0
 *   "ops_cap" the words do not fit ops_cap
 *   "null"    a null ops_used, or a null input array with nhits > 0
 * One wave runs one hit, lane b = j - i - D + B owning a diagonal, over the
 * rows whose band meets [s_lo, s_hi] only: i from min(m-1, s_hi - D + B) down
 * to max(0, s_lo - D - B). A hit's direction buffer is one byte per lane and
 * row run: rows x ((2B + 1 + 3) & ~3) bytes. The hits are sorted by rows and
 * cut into batches that fit GHOSTM_BAND_SCRATCH_MB (default 1024) and hold at
 * most GHOSTM_BAND_BATCH_HITS hits (default: no limit); a batch holds at least
 * one hit. */
int BandAlignGpu(uint32_t nhits, const GhostmBandSource src[], const int32_t diagonal[],
                 const uint32_t s_lo[], const uint32_t s_hi[], uint32_t query_sequence_length,
                 uint32_t step, uint32_t band, int open_gap, int extend_gap,
                 GhostmHitPath rec[], uint32_t ops[], size_t ops_cap, size_t *ops_used);

/* The same on the host, with no device call (the model the kernels are checked
 * against, run cell by cell) and the same checks and reasons: query_seqs = nq
 * records of L codes, db = the chunk's db_len residues, score_matrix =
 * M[db code * 32 + query code]; query_sequence_length must equal L. */
int GhostmBandAlignHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db, uint32_t db_len,
                        const int score_matrix[], uint32_t nhits, const GhostmBandSource src[],
                        const int32_t diagonal[], const uint32_t s_lo[], const uint32_t s_hi[],
                        uint32_t query_sequence_length, uint32_t step, uint32_t band, int open_gap,
                        int extend_gap, GhostmHitPath rec[], uint32_t ops[], size_t ops_cap, size_t *ops_used);

/* The counters of the band pass. A struct of their own, like GhostmDbSetStats:
 * GhostmStats keeps its layout. */
typedef struct GhostmBandStats {
  double seconds_band;       /* k_band_fill<false> + k_band_walk<false> + k_ops_compact, device time */
  uint64_t band_launches;    /* batches of hits */
  uint64_t band_hits;
  uint64_t band_cells;       /* sum over the hits of rows run x (2B + 1) */
  uint64_t band_dir_bytes;   /* direction-buffer bytes the batches addressed */
} GhostmBandStats;

/* The band counters behind the stage-level calls, as GhostmStageStats gives the
 * others: they add up over the process's BandAlignGpu calls and start again at
 * 0 with every GhostmSessionRun. Copies min(size, sizeof(GhostmBandStats))
 * bytes and returns the library's sizeof; 0 on a null argument. */
size_t GhostmStageBandStats(GhostmBandStats *stats, size_t size);

/* Low-complexity masking of query records. Translated reads are full of
 * low-complexity stretches (poly-Q and poly-A runs, collagen-like repeats,
 * frames of AT-rich DNA); a read whose only similarity to a subject is such a
 * stretch would be seeded, aligned, kept by the cull and counted in a clade.
 * This pass hard-masks such stretches before seeding, as blastx -seg yes does:
 * a masked letter becomes X (code 23) in the resident query records, and every
 * pass downstream sees the same letters with no change of its own (K1 finds no
 * seed there, the DP passes and the rows score X, the pile-ups count X).
 *
 * The rule is the first stage of SEG (Wootton and Federhen), the raw segments,
 * in integer arithmetic, so that host and device agree byte for byte. SEG's
 * second stage, which trims each raw segment to its least probable sub-stretch,
 * is not done: a segment is masked whole.
 *
 * Parameters: window w, 6..32; trigger k1 and extend k2 in hundredths of a bit,
 * 0 <= k1 <= k2 <= 500. The customary values are 12, 220, 250.
 *
 * A source is BandAlignGpu's: a protein record's kept letters, or one frame of
 * a DNA read, m letters read through its tile records (letter p lies in tile
 * min(p / step, tiles - 1)). On an untiled set every record is its own source
 * with m = W, the record width.
 *   T[c] = lround(1024 * c * log2(c)) for c = 1..w, T[0] = 0 (w = 12: 0, 0,
 *          2048, 4869, 8192, 11888, 15882, 20123, 24576, 29214, 34017, 38967,
 *          44052)
 *   window i covers letters [i, i + w), 0 <= i <= m - w. It is evaluated only
 *          when all its codes are below 23; B, J and Z are letters of their own.
 *          A window with an X or a '*' in it is neither low nor a trigger, so
 *          the stop runs of a DNA frame and the padding of a record never mask
 *          a neighbour, and they break runs.
 *   S = the sum over the letters a of T[count of a in the window],
 *   d = 100 * (T[w] - S); the window is low when d <= k2 * 1024 * w and a
 *          trigger when d <= k1 * 1024 * w
 *   a maximal run of consecutive low windows i..j that holds at least one
 *          trigger is a segment: letters [i, j + w) are masked
 * A masked letter is stored as 23 into every tile record that covers it, so
 * overlapping tiles stay consistent. '*' is never inside an evaluated window and
 * is never rewritten. A source with m < w is left alone.
 *
 * The records' lengths are not recomputed: GhostmSessionQueryLengths, the
 * E-value's query length and the band pass's m stay those of the unmasked set,
 * as BLAST prices a filtered query.
 *
 * GhostmMaskRecordsHost: the rule on the host, letter by letter, with no device
 * call (the model the kernels are checked against). query_seqs = nq records of
 * L codes, changed in place; masked[nq] receives the letters stored as 23 into
 * every record (a letter under two tiles counts in both). Everything is checked
 * first; a refused call leaves the records and masked untouched and names its
 * reason in GhostmGetLastError:
 *   "window"   window outside 6..32
 *   "levels"   not 0 <= trigger <= extend <= 500
 *   "source"   BandAlignGpu's: a record outside the nq given; tiles == 0 or
 *              letters == 0; tiles disagrees with letters, L and step; step 0 or
 *              over L; L == 0 (MaskRecordsGpu: L over 127 too)
 *   "overlap"  two sources share a record
 *   "null"     a null array with nq or nsrc > 0 */
int GhostmMaskRecordsHost(uint8_t *query_seqs, uint32_t nq, uint32_t L, uint32_t nsrc,
                          const GhostmBandSource src[], uint32_t step, uint32_t window, uint32_t trigger,
                          uint32_t extend, uint32_t masked[]);

/* The same on the GPU (kernels k_mask_windows + k_mask_apply), stage level: the
 * records are uploaded as a chunk of their own (SetQueryGpu's chunk is not
 * touched), masked in place and brought back with masked[]; it exists to be
 * compared with the model byte for byte. The same checks and reasons, all made
 * before any upload or launch. k_mask_windows only reads the records (one wave
 * per source, one lane per window, 64 windows at a time from 64 + w - 1 codes
 * staged in LDS) and writes every window's low and trigger flag; k_mask_apply
 * only writes them (one wave per source resolves the runs over the flag words
 * with a carry in both directions, widens them by w - 1 letters and stores 23
 * into every covering tile). So every window sees the unmasked letters. */
int MaskRecordsGpu(uint8_t *query_seqs, uint32_t nq, uint32_t L, uint32_t nsrc, const GhostmBandSource src[],
                   uint32_t step, uint32_t window, uint32_t trigger, uint32_t extend, uint32_t masked[]);

/* The counters of the mask pass. A struct of their own, like GhostmBandStats:
 * GhostmStats keeps its layout. */
typedef struct GhostmMaskStats {
  double seconds_mask;       /* k_mask_windows + k_mask_apply, device time */
  uint64_t mask_launches;    /* passes launched (both kernels): one per chunk that has a window */
  uint64_t mask_sources;     /* sources with at least one window (m >= w) */
  uint64_t mask_windows;
  uint64_t masked_sources;   /* sources with a masked letter */
  uint64_t masked_letters;   /* letters of the sources masked (each once, under however many tiles) */
} GhostmMaskStats;

/* The mask counters behind the stage-level call; GhostmStageBandStats'
 * conventions. */
size_t GhostmStageMaskStats(GhostmMaskStats *stats, size_t size);

/* Quality trimming and masking of FASTQ reads. A miscalled 3' tail translates
 * into wrong residues in all six frames, which seed, vote and land in a clade;
 * the base qualities say where it begins. The stage runs on the GPU on the
 * reads' letters, before they are formatted and before the low-complexity mask.
 *
 * Integer arithmetic, so that host and device agree byte for byte. A read has n
 * letters and n quality bytes; q[i] = min(max(byte, 33), 126) - 33 (Phred+33);
 * a byte outside '!'..'~' is counted in `bad`.
 *
 * Parameters: trim_q 0..93, mask_q 0..93, min_len 0..2^24. All three 0: off.
 *
 * End trimming: the running-sum rule of BWA (-q) and cutadapt. Both ends are
 * found on the untrimmed read, d[i] = trim_q - q[i].
 *   3' end: i = n - 1, n - 2, ... with s += d[i], stopping at the first s < 0;
 *           end = the i where s first reached its greatest value > 0 (the
 *           largest such i), or n when there is none
 *   5' end: i = 0, 1, ... likewise; begin = i + 1 for the i where s first
 *           reached its greatest value > 0 (the smallest such i), or 0
 *   kept = end - begin when end > begin; else begin = 0, kept = 0
 * With trim_q 0 nothing is trimmed.
 * Floor: kept < min_len gives kept = 0, begin = 0, masked = 0 and leaves the
 * letters untouched (the read stays in the set as an empty record).
 * Masking: every kept letter with q[i] < mask_q is stored as 'N' (the query
 * formatter turns a codon with an N into X) and counted in `masked`. Letters
 * outside [begin, begin + kept) are never rewritten.
 *
 * GhostmQualityTrimHost: the rule on the host, letter by letter, with no device
 * call (the model the kernel is checked against). Read r is lengths[r] bytes at
 * offsets[r] of letters and of qual (both `total` bytes); letters are masked in
 * place, out[n] receives one record per read. With all three parameters 0 the
 * qualities are not read and out[r] = {0, lengths[r], 0, 0}. Everything is
 * checked first; a refused call leaves letters and out untouched and names its
 * reason in GhostmGetLastError:
 *   "param"   a parameter out of range
 *   "null"    a null array with n > 0
 *   "record"  an offset or a length outside `total`
 *   "length"  a read of over 2^24 letters (the running sums are 32 bits wide) */
typedef struct GhostmQualOut {
  uint32_t begin;   /* the first kept letter */
  uint32_t kept;    /* kept letters; 0: the read is empty (crossing ends, or the floor) */
  uint32_t masked;  /* kept letters stored as 'N' */
  uint32_t bad;     /* quality bytes outside '!'..'~', over the whole read */
} GhostmQualOut;
int GhostmQualityTrimHost(uint8_t *letters, const uint8_t *qual, uint64_t total, const uint64_t offsets[],
                          const uint32_t lengths[], uint32_t n, uint32_t trim_q, uint32_t mask_q,
                          uint32_t min_len, GhostmQualOut out[]);

/* The same on the GPU (kernel k_qual_trim: one wave per read, 64 positions at a
 * time from each end, the running sum a wave prefix scan on top of the carried
 * sum, the stop the lowest bit of a ballot), stage level: the reads go up in
 * bounded pieces of whole reads, so a large sample is never staged whole, and
 * the records and the masked letters come back piece by piece. The same checks
 * and reasons, all made before any upload or launch; with n == 0 or all three
 * parameters 0 nothing is launched. */
int QualityTrimGpu(uint8_t *letters, const uint8_t *qual, uint64_t total, const uint64_t offsets[],
                   const uint32_t lengths[], uint32_t n, uint32_t trim_q, uint32_t mask_q, uint32_t min_len,
                   GhostmQualOut out[]);

/* The counters of the quality stage. A read left empty counts all its letters
 * as trimmed3, so letters = trimmed5 + trimmed3 + the kept letters. */
typedef struct GhostmQualStats {
  uint64_t launches;   /* k_qual_trim launches: one per piece */
  uint64_t reads;
  uint64_t letters;
  uint64_t trimmed5;   /* letters cut at the 5' end of reads that keep any */
  uint64_t trimmed3;   /* letters cut at the 3' end, and all letters of the reads left empty */
  uint64_t masked;     /* letters stored as 'N' */
  uint64_t failed;     /* reads emptied by the floor (kept < min_len) */
  uint64_t bad;        /* quality bytes outside '!'..'~' */
  double seconds_quality;  /* k_qual_trim, device time */
} GhostmQualStats;

/* The quality counters behind the stage-level call; GhostmStageBandStats'
 * conventions. */
size_t GhostmStageQualStats(GhostmQualStats *stats, size_t size);

/* Adapter removal for FASTQ reads. A fragment shorter than the read is read
 * through into the sequencing adapter; the tail is translated in all six
 * frames, seeds, votes and piles up, the same wrong residues in every
 * contaminated read. The stage runs on the GPU on the reads' letters, before
 * the quality stage, and only ever shortens a read at its 3' end, so
 * GhostmQualOut.begin and every read coordinate keep their meaning.
 *
 * Integer arithmetic, so that host and device agree byte for byte.
 *
 * Letters: a read byte is upper-cased (ASCII letters only) and compared; a byte
 * that is then none of A, C, G, T mismatches everything but an adapter's N. An
 * adapter is 1..64 letters of ACGTN in either case; its N matches any read byte.
 *
 * Parameters: min_overlap 1..64, err_pct 0..50, pair_overlap 0 (the pair rule
 * is off) or 1..1024. Both adapters empty (or NULL) and pair_overlap 0: off.
 *
 * Adapter rule, a read of n letters and an adapter of m: for a start p in
 * 0..n-1, L = min(m, n - p) and mm(p) = the i < L where read[p + i] does not
 * match adapter[i]; p is accepted when L >= min_overlap and mm(p) * 100 <=
 * err_pct * L; adapter_at = the smallest accepted p, or n. No insertions or
 * deletions are considered: this is fastp's and Trimmomatic's rule, not
 * cutadapt's semiglobal alignment. adapter1 is used for every record, but a
 * non-empty adapter2 for the odd records (mate 2 of interleaved mates).
 *
 * Pair rule (pair_overlap > 0), records 2i and 2i + 1 being mates of n1 and n2
 * letters: for a fragment length f in pair_overlap..min(n1, n2), pm(f) = the
 * i < f where R1[i] is not the complement of R2[f - 1 - i], a byte that is none
 * of A, C, G, T on either mate counting as a mismatch; f is accepted when
 * pm(f) * 100 <= err_pct * f; pair_len = the greatest accepted f, or 0. The
 * greatest is the conservative one: poly-A against poly-T accepts every f and
 * loses nothing. A pair with a mate of over 1024 letters is not examined (the
 * check is quadratic, and read-through needs a fragment shorter than the read)
 * and counted in pair_skipped; neither is one with min(n1, n2) < pair_overlap.
 * Overlaps with f > min(n1, n2) are not looked for and mates are not merged.
 *
 * Per read: kept = min(adapter_at, pair_len ? pair_len : n). The read goes on
 * as its first kept letters; kept == 0 leaves an empty record, so record
 * indices and the pairing hold. The letters are never written.
 *
 * GhostmAdapterTrimHost: the rule on the host, letter by letter, with no device
 * call (the model the kernels are checked against). Read r is lengths[r] bytes
 * at offsets[r] of letters (`total` bytes); out[n] receives one record per read.
 * With the stage off out[r] = {lengths[r], lengths[r], 0, 0, 0}. Everything is
 * checked first; a refused call leaves out untouched and names its reason in
 * GhostmGetLastError:
 *   "param"    a parameter out of range
 *   "adapter"  an adapter letter outside ACGTN, or an adapter of over 64 letters
 *   "null"     a null array with n > 0
 *   "record"   an offset or a length outside `total`
 *   "length"   a read of over 2^24 letters
 *   "pairs"    pair_overlap > 0 with an odd n */
typedef struct GhostmAdapterOut {
  uint32_t kept;        /* the letters the read goes on with */
  uint32_t adapter_at;  /* the adapter rule's cut; the read's length: none */
  uint32_t pair_len;    /* the pair rule's fragment length, the same in both mates; 0: none */
  uint16_t adapter_mismatches;  /* mm(adapter_at); 0 when none */
  uint16_t pair_mismatches;     /* pm(pair_len); 0 when none */
} GhostmAdapterOut;
int GhostmAdapterTrimHost(const uint8_t *letters, uint64_t total, const uint64_t offsets[], const uint32_t lengths[],
                          uint32_t n, const char *adapter1, const char *adapter2, uint32_t min_overlap,
                          uint32_t err_pct, uint32_t pair_overlap, GhostmAdapterOut out[]);

/* The same on the GPU, stage level. k_adapter_find: one wave per read, the
 * lanes own 64 consecutive starts at a time from the 5' end, each counts its
 * mismatches over a window of the read staged in LDS, and the wave leaves at
 * the first group with an accepted lane (the ballot's lowest bit).
 * k_pair_overlap: one wave per pair, both mates staged in LDS once, mate 2
 * reverse-complemented, the lanes own 64 fragment lengths at a time from
 * min(n1, n2) downwards. The reads go up in bounded pieces of whole reads (of
 * whole pairs with the pair rule on). The same checks and reasons, all made
 * before any upload or launch; with n == 0 or the stage off nothing is
 * launched. */
int AdapterTrimGpu(const uint8_t *letters, uint64_t total, const uint64_t offsets[], const uint32_t lengths[],
                   uint32_t n, const char *adapter1, const char *adapter2, uint32_t min_overlap, uint32_t err_pct,
                   uint32_t pair_overlap, GhostmAdapterOut out[]);

/* The counters of the adapter stage. */
typedef struct GhostmAdapterStats {
  uint64_t launches;       /* kernel launches: per piece one k_adapter_find when an adapter is set and one
                              k_pair_overlap when the pair rule is on */
  uint64_t reads;
  uint64_t letters;
  uint64_t cut_reads;      /* reads with kept below their length */
  uint64_t cut_letters;    /* the letters they lost */
  uint64_t adapter_found;  /* reads with adapter_at below their length */
  uint64_t pair_found;     /* pairs with pair_len > 0 */
  uint64_t pair_skipped;   /* pairs not examined for a mate of over 1024 letters */
  uint64_t emptied;        /* reads with letters that keep none */
  double seconds_adapter;  /* both kernels, device time */
} GhostmAdapterStats;

/* The adapter counters behind the stage-level call; GhostmStageBandStats'
 * conventions. */
size_t GhostmStageAdapterStats(GhostmAdapterStats *stats, size_t size);

/* Frameshift-aware read-level alignments of DNA reads. BandAlignGpu aligns one
 * frame; after a single-nucleotide insertion or deletion the true alignment of
 * a read continues in another frame of the same strand, and this pass follows
 * it there for a cost.
 *
 * A strand source is one strand of a DNA read: its three frames g = 0, 1, 2
 * (tile-table frames 3 x strand + g), each of m letters (the tile table's
 * letters, n / 3). It is described by a GhostmBandSource with one added rule:
 * first_record is tile 0 of frame g = 0 of that strand, and letter c of frame g
 * lies in record first_record + g + stride * t, with t, the tile start and the
 * byte within the tile as in BandAlignGpu; stride is ignored when tiles == 1.
 * The read's strand position is p = 3c + g, 0 <= p < 3m, and its letter q(p) is
 * letter p / 3 of frame p % 3: letter t of the frame at offset o covers strand
 * positions o + 3t .. o + 3t + 2 (the reverse strand counted from the read's
 * last kept nucleotide), which is how the tiled setters lay the frames out.
 *
 * Per hit: the source, the subject range [s_lo, s_hi] (absolute in the chunk,
 * END-free), the anchor diagonal D in letters, the half-width B (1..31), open,
 * ext and the frameshift cost shift <= 0. The band cells are (p, j) with
 * 0 <= p < 3m, s_lo <= j <= s_hi and |j - floor(p / 3) - D| <= B. All
 * arithmetic is int32. The DP runs in reverse, rows p = 3m-1 .. 0 and j
 * descending within a row:
 *   d0 = H(p+3, j+1)            in frame
 *   d1 = H(p+2, j+1) + shift    the next codon starts one nucleotide early
 *   d2 = H(p+4, j+1) + shift    the next codon starts one nucleotide late
 *   diag = d0, fsel = 0; if d1 > diag: diag = d1, fsel = 1; if d2 > diag:
 *          diag = d2, fsel = 2 (each strict, in that order)
 *   s      = diag + M[(db[j] & 31) * 32 + (q(p) & 31)]
 *   E(p,j) = max(E(p,j+1) + ext, H(p,j+1) + open)    'D'
 *   F(p,j) = max(F(p+3,j) + ext, H(p+3,j) + open)    'I': one codon against a gap
 *   H(p,j) = s if s > 0 else 0; then E if E > H; then F if F > H (hsel 1 / 0,
 *            2, 3, as BandAlignGpu)
 *   eext   = E(p,j+1) + ext > H(p,j+1) + open (a tie opens); fext likewise
 *            with (p+3, j)
 * A neighbour that is no band cell has H = 0 and E = F = minus infinity. The
 * start cell is the first strict maximum in processing order (the largest p,
 * then the largest j). The walk: in H state with hsel 1 it emits '=' or 'X'
 * (the two codes masked with 31 are equal or not); if fsel is 1 it then emits
 * op 5 ('/') and goes to (p+2, j+1), if fsel is 2 op 4 ('\') and goes to
 * (p+4, j+1), otherwise it goes to (p+3, j+1). hsel 2 / 3 enter E / F at the
 * same cell; E emits 'D' and goes to (p, j+1), F emits 'I' and goes to
 * (p+3, j), both staying in the gap state while eext / fext. hsel 0 or leaving
 * the band cells stops. The run-length words keep the len << 4 | op encoding
 * with the two new op codes 4 and 5; the paths of every other call never
 * contain them. The result is a GhostmHitPath: q_start is the strand position
 * of the first codon's first nucleotide, q_end the last nucleotide consumed,
 * s_* absolute. Score 0 gives an empty path at q_start = 0, s_start = s_lo.
 *
 * Three consequences:
 *   A shift never ends a path: it is taken only if d1 or d2 beats d0 >= 0, so
 *   the cell stepped to is a band cell with H > 0 and the walk emits there.
 *   Two shift ops are never adjacent: a shift follows a pair column only.
 *   The row's E chain is still exact as a max-plus scan, under open <= ext <=
 *   0: E depends on the same row only, exactly as in BandAlignGpu.
 * With shift = -(1 << 20), and scores below 1 << 20, no shift is ever taken
 * and the score is the maximum over g of BandAlignGpu's on frame g with the
 * same D, B and range.
 *
 * FrameAlignGpu: stage level like BandAlignGpu, whose arguments it takes plus
 * shift_cost; the NULL / cap convention and the refusals are BandAlignGpu's
 * (a frame's record outside the chunk is "source"), plus
 *   "shift"   shift_cost > 0 or shift_cost < -(1 << 20)
 * A refused call leaves rec, ops and *ops_used untouched. One wave runs one
 * hit (kernels k_band_fill<true> + k_band_walk<true> + k_ops_compact), lane b = j -
 * floor(p / 3) - D + B, over the nucleotide rows of the codon rows BandAlignGpu
 * would run: p from 3 x c_top + 2 down to 3 x c_bot. A hit's direction buffer
 * is rows x ((2B + 1 + 3) & ~3) bytes, bits 5-6 of a byte holding fsel; its
 * words number at most rows + 4B + 4. The hits are sorted by rows and cut into
 * batches that fit GHOSTM_FRAME_SCRATCH_MB (default 1024) and hold at most
 * GHOSTM_FRAME_BATCH_HITS hits (default: no limit). */
int FrameAlignGpu(uint32_t nhits, const GhostmBandSource src[], const int32_t diagonal[],
                  const uint32_t s_lo[], const uint32_t s_hi[], uint32_t query_sequence_length,
                  uint32_t step, uint32_t band, int open_gap, int extend_gap, int shift_cost,
                  GhostmHitPath rec[], uint32_t ops[], size_t ops_cap, size_t *ops_used);

/* The same on the host, with no device call: the model the kernels equal byte
 * for byte in records and words, run cell by cell. Arguments as
 * GhostmBandAlignHost plus shift_cost. */
int GhostmFrameAlignHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db, uint32_t db_len,
                         const int score_matrix[], uint32_t nhits, const GhostmBandSource src[],
                         const int32_t diagonal[], const uint32_t s_lo[], const uint32_t s_hi[],
                         uint32_t query_sequence_length, uint32_t step, uint32_t band, int open_gap,
                         int extend_gap, int shift_cost, GhostmHitPath rec[], uint32_t ops[], size_t ops_cap,
                         size_t *ops_used);

/* The counters of the frame pass, a struct of their own like GhostmBandStats. */
typedef struct GhostmFrameStats {
  double seconds_frame;      /* k_band_fill<true> + k_band_walk<true> + k_ops_compact, device time */
  uint64_t frame_launches;   /* batches of hits */
  uint64_t frame_hits;
  uint64_t frame_cells;      /* sum over the hits of rows run x (2B + 1) */
  uint64_t frame_dir_bytes;  /* direction-buffer bytes the batches addressed */
} GhostmFrameStats;

/* The frame counters behind the stage-level calls; GhostmStageBandStats'
 * conventions. */
size_t GhostmStageFrameStats(GhostmFrameStats *stats, size_t size);

/* What GhostmSessionFrameInfo tells about a hit's frame path. */
typedef struct GhostmHitFrameInfo {
  uint32_t strand;   /* 0 forward, 1 reverse complement */
  uint32_t read_nt;  /* the read's kept nucleotides n */
  uint32_t letters;  /* m = n / 3, the letters of each frame */
  uint32_t shifts;   /* the summed length of the path's shift runs */
} GhostmHitFrameInfo;

/* The aligned rows of a read-level path: what GhostmHitRows and PathRowsGpu are
 * to a tile path, for the paths of BandAlignGpu (band mode) and FrameAlignGpu
 * (frame mode). The text layout is GhostmHitRows': 3 * columns bytes at
 * rows[rows_offset], the query row, the midline and the subject row, letters
 * "ARNDCQEGHILKMFPSTWYVBJZX*"[c] and '?' from code 25 up, the midline the query
 * letter in a '=' column, '+' in an 'X' column whose matrix entry
 * M[(db code & 31) * 32 + (query code & 31)] is > 0 and a space elsewhere.
 *
 * The query letters are read through the hit's GhostmBandSource, W and step,
 * by the rules above BandAlignGpu and FrameAlignGpu: letter c of frame offset
 * g (band mode: g = 0) lies in tile t = min(c / step, tiles - 1), whose start
 * is t * step, or max(letters - W, 0) for the last tile; its record is
 * first_record + g + stride * t (stride ignored when tiles == 1), its byte
 * c - start(t).
 *
 * Every word gives len display columns, and a position runs along the path
 * from rec.q_start (subject: rec.s_start, absolute in the chunk):
 *   band mode   the position is a source letter. A column of op 0, 1 or 2
 *               shows the letter at the position and advances it by 1; op 3
 *               advances the subject only.
 *   frame mode  the position p is a strand position in nucleotides. A column
 *               of op 0, 1 or 2 shows letter p / 3 of frame p % 3 and advances
 *               p by 3; op 3 leaves p; a column of op 4 ('\') advances p by 1
 *               and a column of op 5 ('/') takes 1 from it. A shift column
 *               holds '\' or '/' in the query row, a space in the midline and
 *               '-' in the subject row, and touches no subject residue.
 * Ops 0, 1 and 3 advance the subject position by 1 per column. The op of a
 * pair column is taken as given ('=' or 'X'): a '=' column counts as an
 * identity and puts the query letter on the midline whatever the codes are.
 *
 * query_record is the record of the first query letter, the letter at
 * rec.q_start (stage level: in the resident chunk; session level: the global
 * index as in GhostmHitRows); a path without words gives first_record, columns
 * 0, counts 0 and no bytes. shifts counts the columns of ops 4 and 5; they are
 * no gap_residues. rescore adds shift_cost per shift column to GhostmHitRows'
 * sum (band mode never reads shift_cost) and equals GhostmHitPath.score for a
 * path BandAlignGpu or FrameAlignGpu made with the same costs: a proof of the
 * DP that walks the sequences only. */
typedef struct GhostmHitReadRows {   /* 40 bytes; the first 32 are GhostmHitRows' */
  uint32_t query_record;
  uint32_t columns;
  uint32_t identities;
  uint32_t positives;
  uint32_t gap_residues;  /* 'I' and 'D' columns only */
  int32_t rescore;
  uint64_t rows_offset;
  uint32_t shifts;        /* columns of ops 4 and 5; 0 in band mode */
  uint32_t pad;           /* 0 */
} GhostmHitReadRows;

/* The rows of every read-level hit (kernel k_read_rows), stage level like
 * PathRowsGpu (after SetQueryGpu and SetDbGpu): hit i has source src[i], and
 * rec[i] gives q_start, s_start (absolute in the chunk) and its n_runs words
 * at ops[ops_offset]; q_end, s_end and score are not read.
 * query_sequence_length is the records' width W, step the tile step, frame 0
 * for band paths and 1 for frame paths (src[i] then names frame 0 of a strand).
 * Any well-formed path is accepted, not only one the passes made. Record i
 * belongs to hit i; the hits' bytes follow each other in hit order. rows ==
 * NULL: only *rows_used (the bytes needed) and out (may be NULL) are written.
 * nhits == 0 writes *rows_used = 0 and nothing else. Everything is checked on
 * the host before any upload or launch; a refused call leaves out, rows and
 * *rows_used untouched and names its reason in GhostmGetLastError:
 *   "source"   as BandAlignGpu: a record outside the chunk (frame mode: a
 *              frame's record); tiles == 0 or letters == 0; tiles disagrees
 *              with letters, W and step; stride 0 with several tiles; step 0 or
 *              over W; W differs from the resident chunk's
 *   "ops"      ops_offset + n_runs > ops_len
 *   "word"     a zero length or bit 3 set; band mode: an op above 3; frame
 *              mode: an op of 6 or 7
 *   "bounds"   a column of op 0, 1 or 2 whose position lies outside [0,
 *              letters) in band mode or [0, 3 * letters) in frame mode, or the
 *              q_start of a path with words outside it; subject residues past
 *              the resident chunk; more than 2^32 - 1 columns or strand
 *              positions
 *   "shift"    frame mode: shift_cost > 0 or shift_cost < -(1 << 20)
 *   "rows_cap" rows_cap smaller than the bytes needed
 *   "null"     null src or rec with nhits > 0
 * One wave runs one hit with k_path_rows' column machinery; the row buffer is
 * cut into batches of hits that fit GHOSTM_READ_ROWS_SCRATCH_MB (default 1024)
 * and hold at most GHOSTM_READ_ROWS_BATCH_HITS hits (default: no limit); a
 * batch holds at least one hit. */
int ReadRowsGpu(uint32_t nhits, const GhostmBandSource src[], const GhostmHitPath rec[],
                const uint32_t ops[], size_t ops_len, uint32_t query_sequence_length, uint32_t step,
                int frame, int open_gap, int extend_gap, int shift_cost, GhostmHitReadRows out[],
                uint8_t rows[], size_t rows_cap, size_t *rows_used);

/* The same on the host, with no device call (the model the kernel equals byte
 * for byte, written column by column) and the same checks and reasons:
 * query_seqs = nq records of L codes, db = the chunk's db_len residues,
 * score_matrix = M[db code * 32 + query code]; query_sequence_length must equal
 * L ("source"); null query_seqs, db or score_matrix with nhits > 0 is "null". */
int GhostmReadRowsHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                       uint32_t db_len, const int score_matrix[], uint32_t nhits,
                       const GhostmBandSource src[], const GhostmHitPath rec[], const uint32_t ops[],
                       size_t ops_len, uint32_t query_sequence_length, uint32_t step, int frame,
                       int open_gap, int extend_gap, int shift_cost, GhostmHitReadRows out[],
                       uint8_t rows[], size_t rows_cap, size_t *rows_used);

/* The counters of the read-level rows pass, a struct of their own like
 * GhostmBandStats. */
typedef struct GhostmReadRowsStats {
  double seconds_read_rows;    /* k_read_rows, device time */
  uint64_t read_rows_launches; /* batches of hits (one launch each) */
  uint64_t read_rows_hits;
  uint64_t read_rows_columns;  /* sum of the hits' columns */
} GhostmReadRowsStats;

/* The read-rows counters behind the stage-level calls; GhostmStageBandStats'
 * conventions. */
size_t GhostmStageReadRowsStats(GhostmReadRowsStats *stats, size_t size);

/* The read-level subject pile-up: PathPileupGpu's view (its definitions: 32
 * uint32_t per position, slot(c), depth, identities, consensus, integer sums
 * only) from read-level paths, so a read adds depth over its whole alignment
 * and not over one tile's 127 letters. These points differ.
 *   source letters   a hit is a GhostmBandSource and a GhostmHitPath (q_start,
 *                    s_start absolute in the chunk, n_runs words at
 *                    ops[ops_offset]) as for ReadRowsGpu, and its query letters
 *                    are read through the source by ReadRowsGpu's rules: band
 *                    mode (frame 0) the letter at the position, advancing by 1;
 *                    frame mode (frame 1) letter p / 3 of frame p % 3,
 *                    advancing by 3
 *   columns          a column of op 0 or 1 at subject position s adds 1 to
 *                    profile[s][slot(query code)], op 3 adds 1 to
 *                    profile[s][26], op 2 adds nothing
 *   shift columns    (frame mode) a column of op 4 moves the strand position
 *                    by +1, of op 5 by -1, and touches no subject residue. It
 *                    is charged to the position the path stands at, s =
 *                    rec.s_start + the subject residues of the columns before
 *                    it: 1 to profile[s][27] for op 4, to profile[s][28] for op
 *                    5. In a path FrameAlignGpu made that is the residue of the
 *                    column after the shift (a shift never ends a path); a
 *                    hand-made path that ends in a shift charges the position
 *                    one past its last residue. Slots 27 and 28 are not part of
 *                    depth. Band mode leaves slots 27..31 at 0, frame mode
 *                    29..31.
 *   shifts[s]        = profile[s][27] + profile[s][28]; shifts may be NULL
 * A hit with an empty path adds nothing.
 *
 * ReadPileupGpu (kernels k_read_pileup and k_pileup_finish) is stage level like
 * PathPileupGpu and ReadRowsGpu (after SetQueryGpu and SetDbGpu).
 * query_sequence_length is the records' width W, step the tile step. db_len
 * must be the resident chunk's length; depth, identities, consensus and shifts
 * hold db_len elements, profile db_len * 32 or is NULL. nhits == 0 gives zeros
 * and 255s. Everything is checked on the host before any upload or launch; a
 * refused call leaves every output untouched and names its reason in
 * GhostmGetLastError: ReadRowsGpu's "source", "ops", "word" and "bounds" by the
 * same validation ("bounds" also for a shift column whose position is >=
 * db_len), and PathPileupGpu's "db_len" and "null". The tiles, parts, windows
 * and upload batches are PathPileupGpu's, under the same GHOSTM_PILEUP_*
 * variables; a path is walked once by every tile it meets. 9 bytes per
 * position are read back, 13 with shifts. */
int ReadPileupGpu(uint32_t nhits, const GhostmBandSource src[], const GhostmHitPath rec[],
                  const uint32_t ops[], size_t ops_len, uint32_t query_sequence_length, uint32_t step,
                  int frame, uint32_t db_len, uint32_t depth[], uint32_t identities[],
                  uint8_t consensus[], uint32_t shifts[], uint32_t profile[]);

/* The same on the host, with no device call (the model the kernels equal
 * exactly, written column by column) and the same checks and reasons:
 * query_seqs = nq records of L codes, db = the chunk's db_len residues;
 * query_sequence_length must equal L ("source"). */
int GhostmReadPileupHost(const uint8_t *query_seqs, uint32_t nq, uint32_t L, const uint8_t *db,
                         uint32_t db_len, uint32_t nhits, const GhostmBandSource src[],
                         const GhostmHitPath rec[], const uint32_t ops[], size_t ops_len,
                         uint32_t query_sequence_length, uint32_t step, int frame, uint32_t depth[],
                         uint32_t identities[], uint8_t consensus[], uint32_t shifts[],
                         uint32_t profile[]);

/* The counters of the read-level pile-up, a struct of their own like
 * GhostmBandStats; GhostmStats' pileup_* fields count PathPileupGpu only. */
typedef struct GhostmReadPileupStats {
  double seconds_read_pileup;    /* k_read_pileup + k_pileup_finish, device time */
  uint64_t read_pileup_launches; /* k_read_pileup launches */
  uint64_t read_pileup_windows;  /* profile windows */
  uint64_t read_pileup_parts;    /* (tile, part) workgroups */
  uint64_t read_pileup_columns;  /* '=', 'X' and 'D' columns charged */
  uint64_t read_pileup_shifts;   /* shift columns charged */
} GhostmReadPileupStats;

/* The read-level pile-up counters behind the stage-level calls;
 * GhostmStageBandStats' conventions. */
size_t GhostmStageReadPileupStats(GhostmReadPileupStats *stats, size_t size);

/* One subject's summary of the session-level read pile-up
 * (GhostmSessionReadPileup). */
typedef struct GhostmSubjectReadPileup {  /* 48 bytes; the first 40 are GhostmSubjectPileup's */
  uint32_t length;
  uint32_t hits;
  uint32_t covered;
  uint32_t max_depth;
  uint64_t depth_sum;
  uint64_t identities_sum;
  uint64_t offset;
  uint64_t shifts_sum;      /* the sum of shifts over the subject; 0 in band mode */
} GhostmSubjectReadPileup;

/* The read-level cull: per read, its hits ranked by read-level score, the hits
 * that find one alignment twice marked, and the hits marked whose stretch of
 * the read better hits already cover. All arithmetic is on integers; the
 * kernel equals the host model exactly.
 *
 * Input: nreads reads; read r's hits are hit[read_begin[r] ..
 * read_begin[r + 1]) (read_begin has nreads + 1 entries, monotone, the last at
 * most nhits; hits outside every read get no output). A hit is its subject,
 * its score and two inclusive ranges, q on the read and s on the subject, lo
 * <= hi, every coordinate below 2^25 (so that d * 100 fits 32 bits).
 *
 * Per read:
 *   1. The hits are ordered by score descending, then input index ascending.
 *   2. In that order every hit gets its status:
 *        EMPTY   its score is 0. Such a hit covers nothing.
 *        DUP     an earlier KEPT hit has the same subject, a q range that
 *                meets this one's and an s range that meets this one's (ranges
 *                meet when they share a position; q_hi + 1 == the other's q_lo
 *                does not). detail names the first such hit in rank order, as
 *                its index in the call's hit array.
 *        CULLED  otherwise, with d = the positions p of [q_lo, q_hi] that at
 *                least top_k earlier KEPT hits contain in their q range, when
 *                d * 100 >= cover_pct * (q_hi - q_lo + 1). detail = d.
 *        KEPT    otherwise. kept_rank is the count of the read's hits kept
 *                before it; detail = d.
 *   3. out[i] is hit i's record: order (its place in the ranking, from 0),
 *      status, kept_rank (0xFFFFFFFF unless KEPT) and detail (0 for EMPTY).
 *
 * top_k is 1..255, cover_pct 1..100. */
typedef struct GhostmCullHit {  /* 24 bytes */
  uint32_t subject;
  uint32_t score;
  uint32_t q_lo, q_hi;  /* inclusive, on the read */
  uint32_t s_lo, s_hi;  /* inclusive, on the subject */
} GhostmCullHit;

enum { GHOSTM_CULL_KEPT = 0, GHOSTM_CULL_DUP = 1, GHOSTM_CULL_CULLED = 2, GHOSTM_CULL_EMPTY = 3 };

typedef struct GhostmCullOut {  /* 16 bytes */
  uint32_t order;      /* the hit's place in its read's ranking */
  uint32_t status;     /* GHOSTM_CULL_* */
  uint32_t kept_rank;  /* 0xFFFFFFFF unless KEPT */
  uint32_t detail;     /* d; DUP: the index of the kept hit it repeats; EMPTY: 0 */
} GhostmCullOut;

/* ReadCullGpu (kernel k_read_cull) is stage level, but needs neither
 * SetQueryGpu nor SetDbGpu: the records are all it reads. It runs on
 * SetOptionGpu's device, or on device 0 when that was not called. Everything is checked
 * on the host before any upload or launch; a refused call returns 1, leaves
 * out untouched and names its reason in GhostmGetLastError:
 *   "null"    a null pointer where one is needed (hit with nhits > 0,
 *             read_begin with nreads > 0, out when a read has a hit)
 *   "reads"   read_begin not monotone or ending past nhits; a read of more
 *             than 2^24 hits
 *   "range"   lo > hi
 *   "bounds"  a coordinate at or over 2^25
 *   "param"   top_k or cover_pct out of range
 * Reads of at most 64 hits take one wave each, reads of at most 256 and of at
 * most 1024 one workgroup with the tables in LDS, larger reads one workgroup
 * with the tables in device memory; no read is too large for the device path
 * and none is done on the host. The reads go in batches of at most
 * GHOSTM_CULL_BATCH_READS reads (default: no limit) and GHOSTM_CULL_SCRATCH_MB
 * megabytes of records and tables (default 1024); 16 bytes per hit are read
 * back. */
int ReadCullGpu(uint32_t nreads, const uint32_t read_begin[], uint32_t nhits, const GhostmCullHit hit[],
                uint32_t top_k, uint32_t cover_pct, GhostmCullOut out[]);

/* The same on the host, with no device call: the model the kernel equals
 * exactly, with the same checks and reasons. */
int GhostmReadCullHost(uint32_t nreads, const uint32_t read_begin[], uint32_t nhits,
                       const GhostmCullHit hit[], uint32_t top_k, uint32_t cover_pct,
                       GhostmCullOut out[]);

/* The counters of the read-level cull, a struct of their own like
 * GhostmBandStats; GhostmStats keeps its layout. */
typedef struct GhostmReadCullStats {
  double seconds_cull;     /* k_read_cull, device time */
  uint64_t cull_launches;  /* batches of reads */
  uint64_t cull_reads;
  uint64_t cull_hits;
  uint64_t cull_kept;
  uint64_t cull_dups;
  uint64_t cull_culled;
} GhostmReadCullStats;

/* The cull counters behind the stage-level calls; GhostmStageBandStats'
 * conventions. */
size_t GhostmStageReadCullStats(GhostmReadCullStats *stats, size_t size);

/* The taxon of a read: the lowest common ancestor (LCA) of the subjects its
 * best hits name, with a support threshold. All arithmetic is on integers; the
 * kernel equals the host model exactly.
 *
 * Taxonomy: nnodes nodes, indexed 0 .. nnodes - 1, parent[i] < nnodes. Exactly
 * one node is its own parent, the root; every node reaches the root;
 * depth[root] = 0 and depth[i] = depth[parent[i]] + 1. 1 <= nnodes <= 2^24 and
 * depth <= 255: one 32-bit word depth << 24 | parent holds a node, so a step up
 * the tree is one gather.
 *
 * Input: nreads reads; read r's hits are hit[read_begin[r] ..
 * read_begin[r + 1]) (read_begin has nreads + 1 entries, monotone, the last at
 * most nhits). A hit is the node of its subject (0xFFFFFFFF: the subject has no
 * taxon), its score (0: not a candidate; it was culled, a duplicate, or empty)
 * and its inclusive stretch q_lo <= q_hi of the read. Scores and coordinates
 * are below 2^25, so that score * 100 fits 32 bits.
 *
 * Per read:
 *   1. The candidates are the read's hits with score > 0; `candidates` is their
 *      number and best_score their largest score.
 *   2. Score test. For a candidate h, ref(h) is the largest score among the
 *      candidates g, h included, whose [q_lo, q_hi] shares a position with h's
 *      (q_hi + 1 == the other's q_lo does not). h passes when score(h) * 100 >=
 *      (100 - top_pct) * ref(h). The test is relative to the hits on the same
 *      stretch: a read that carries a strong and a weak gene lets both vote.
 *   3. The votes are the passing candidates with a node; `votes` is their
 *      number V, `unmapped` the number of passing candidates without a node.
 *   4. V == 0: node = lca = 0xFFFFFFFF, depth = support = 0.
 *   5. Otherwise count(n) is the number of votes whose node has n on its path
 *      to the root, ends included, and thr = (support_pct * V + 99) / 100.
 *      node is the deepest n with count(n) >= thr (unique: support_pct >= 51
 *      puts thr above V / 2, so two such nodes lie on one path), support =
 *      count(node), depth = depth[node]; lca is the deepest n with count(n) ==
 *      V. With support_pct == 100, node == lca.
 * A read without hits gets the record of 4 with all counts 0. The record does
 * not depend on the order of the hits. top_pct is 0..100, support_pct 51..100. */
typedef struct GhostmLcaHit {  /* 16 bytes */
  uint32_t node;        /* the subject's node, or 0xFFFFFFFF */
  uint32_t score;       /* 0: not a candidate */
  uint32_t q_lo, q_hi;  /* inclusive, on the read */
} GhostmLcaHit;

typedef struct GhostmLcaOut {  /* 32 bytes */
  uint32_t node;        /* the assignment, or 0xFFFFFFFF */
  uint32_t depth;       /* depth[node] */
  uint32_t votes;       /* V */
  uint32_t support;     /* count(node) */
  uint32_t lca;         /* the deepest node on every vote's path, or 0xFFFFFFFF */
  uint32_t candidates;
  uint32_t unmapped;
  uint32_t best_score;
} GhostmLcaOut;

/* The taxonomy of the stage-level calls: checked on the host, packed and made
 * resident on SetOptionGpu's device, or on device 0 when that was not called.
 * It stays until the next SetTaxonomyGpu or FreeGpu. Refusals (return 1, the
 * reason in GhostmGetLastError; the previous taxonomy stays):
 *   "taxonomy"  no root, a second root, a cycle, a parent out of range, nnodes
 *               outside 1..2^24, a node deeper than 255; the first offending
 *               node is named
 *   "null"      parent is null */
int SetTaxonomyGpu(uint32_t nnodes, const uint32_t parent[]);

/* The same checks and the depths on the host, without a device:
 * depth_out[nnodes]. */
int GhostmTaxonomyDepths(uint32_t nnodes, const uint32_t parent[], uint32_t depth_out[]);

/* ReadLcaGpu (kernels k_read_lca_wave, k_read_lca) needs neither SetQueryGpu
 * nor SetDbGpu: the records and the resident taxonomy are all it reads.
 * Everything is checked on the host before any upload or launch; a refused
 * call returns 1, leaves out untouched, launches nothing and names its reason:
 *   "param"     top_pct or support_pct out of range
 *   "null"      a null pointer where one is needed (hit with nhits > 0,
 *               read_begin with nreads > 0, out with nreads > 0)
 *   "taxonomy"  no taxonomy is resident
 *   "reads"     read_begin not monotone or ending past nhits; a read of more
 *               than 16384 candidates (the score test is quadratic in a read's
 *               candidates: 16384^2 pair tests over 1024 lanes is 262144
 *               iterations per lane, which stays in the milliseconds)
 *   "range"     q_lo > q_hi
 *   "bounds"    a score or coordinate at or over 2^25
 *   "node"      a node that is neither 0xFFFFFFFF nor below nnodes
 * A read of at most 64 candidates takes one wave, a read of at most 1024 one
 * workgroup with its tables in LDS, a larger read one workgroup with its
 * tables in device memory; none is done on the host (a read without a
 * candidate needs no kernel: its record is 4's). The reads go in batches of at
 * most GHOSTM_LCA_BATCH_READS reads (default: no limit) and
 * GHOSTM_LCA_SCRATCH_MB megabytes of hits, records and tables (default 1024);
 * 32 bytes per read are read back. out has nreads records. */
int ReadLcaGpu(uint32_t nreads, const uint32_t read_begin[], uint32_t nhits, const GhostmLcaHit hit[],
               uint32_t top_pct, uint32_t support_pct, GhostmLcaOut out[]);

/* The same on the host over the taxonomy given, with no device call: the model
 * the kernel equals exactly, with the same checks and reasons (and
 * SetTaxonomyGpu's for the taxonomy). */
int GhostmReadLcaHost(uint32_t nnodes, const uint32_t parent[], uint32_t nreads, const uint32_t read_begin[],
                      uint32_t nhits, const GhostmLcaHit hit[], uint32_t top_pct, uint32_t support_pct,
                      GhostmLcaOut out[]);

/* The counters of the assignment, a struct of their own like
 * GhostmReadCullStats; GhostmStats keeps its layout. */
typedef struct GhostmReadLcaStats {
  double seconds_lca;     /* k_read_lca*, device time */
  uint64_t lca_launches;  /* batches of reads with a candidate */
  uint64_t lca_reads;     /* reads with a hit */
  uint64_t lca_hits;
  uint64_t lca_votes;     /* V summed over the reads */
  uint64_t lca_assigned;  /* reads with a node */
} GhostmReadLcaStats;

/* The counters behind the stage-level calls; GhostmStageReadCullStats'
 * conventions. */
size_t GhostmStageReadLcaStats(GhostmReadLcaStats *stats, size_t size);

/* Mate pairs: the join of both mates' hits per fragment, the step between the
 * cull and the assignment. Two reads from the two ends of one DNA fragment hit
 * one subject close together; a hit of mate 1 and a hit of mate 2 that do are
 * joined into one candidate with the sum of their scores, so that the pair is
 * assigned (ReadLcaGpu, with the pairs as reads) and counted once. All
 * arithmetic is on integers; the kernel equals the host model exactly.
 *
 * Input: npairs pairs; pair p's hits are hit[pair_begin[2p] .. pair_begin[2p +
 * 1]) of mate 1 and hit[pair_begin[2p + 1] .. pair_begin[2p + 2]) of mate 2
 * (pair_begin has 2 * npairs + 1 entries, monotone, the last at most nhits;
 * either half may be empty). A hit is its subject, the subject's node
 * (0xFFFFFFFF: none), its score (0: not a candidate), two inclusive ranges, q on
 * its own mate and s on the subject, lo <= hi, and its strand (0 or 1). Scores
 * and coordinates are below 2^24, so that a pair's sum and an offset coordinate
 * stay below ReadLcaGpu's 2^25. offset[p], below 2^24, is mate 1's length in
 * read units: where mate 2's coordinates start in the pair's coordinate space.
 *
 * Candidates i of mate 1 and j of mate 2 are concordant when their subjects
 * are equal, orient == 0 or their strands differ, and max(s_hi) - min(s_lo) + 1
 * <= max_span (their span on the subject). max_span is 1..2^24, orient 0 or 1.
 *
 * Per pair:
 *   1. Every mate-1 candidate i takes as partner the concordant j of highest
 *      score, of lowest index among equal scores, or none.
 *   2. A mate-2 candidate is taken when some i chose it; its partner is the
 *      lowest such i.
 *   3. cand[h] and partner[h] are hit h's, in input order (no compaction;
 *      partner is an index of the call's hit array or 0xFFFFFFFF):
 *        mate 1, joined      node its own, score_i + score_j, [q_lo_i, offset +
 *                            q_hi_j]; partner j
 *        mate 1, not joined  itself; partner 0xFFFFFFFF
 *        mate 2, taken       all zero (score 0: no candidate of its own);
 *                            partner the lowest i that chose it
 *        mate 2, not taken   itself with q_lo + offset and q_hi + offset;
 *                            partner 0xFFFFFFFF
 *        not a candidate     all zero; partner 0xFFFFFFFF
 *   4. out[p]: joined = the mate-1 candidates with a partner; mates = bit 0 when
 *      mate 1 has a candidate, bit 1 when mate 2 has one; best_score = the
 *      largest cand score of the pair; best_span = the span of the joined
 *      candidate of highest score, lowest index among equals, 0 when none.
 * A pair without hits gets an all-zero record. Hits outside every pair are not
 * written. The result depends on the records alone. */
typedef struct GhostmPairHit {  /* 32 bytes */
  uint32_t subject;
  uint32_t node;        /* the subject's node, or 0xFFFFFFFF */
  uint32_t score;       /* 0: not a candidate */
  uint32_t q_lo, q_hi;  /* inclusive, on the hit's own mate */
  uint32_t s_lo, s_hi;  /* inclusive, on the subject */
  uint32_t strand;      /* 0 or 1 */
} GhostmPairHit;

typedef struct GhostmPairOut {  /* 16 bytes */
  uint32_t joined;
  uint32_t mates;       /* bit 0: mate 1 has a candidate; bit 1: mate 2 */
  uint32_t best_score;
  uint32_t best_span;
} GhostmPairOut;

/* PairJoinGpu (kernel k_pair_join) needs neither SetQueryGpu nor SetDbGpu: the
 * records are all it reads. Everything is checked on the host before any
 * upload or launch; a refused call returns 1, leaves cand, partner and out
 * untouched, launches nothing and names its reason:
 *   "null"    a null pointer where one is needed (hit with nhits > 0;
 *             pair_begin, offset and out with npairs > 0; cand and partner when
 *             a pair has a hit)
 *   "reads"   pair_begin not monotone or ending past nhits; a pair of more than
 *             16384 hits (the join is quadratic in a pair's hits and feeds
 *             ReadLcaGpu, whose reads end there)
 *   "range"   lo > hi
 *   "bounds"  a score, a coordinate or an offset at or over 2^24; a strand
 *             above 1
 *   "param"   max_span or orient out of range
 * A pair of at most 64 hits takes one wave, a pair of at most 1024 one
 * workgroup with its records in LDS, a larger pair one workgroup reading the
 * records from device memory; none is done on the host (a pair without hits
 * needs no kernel). The pairs go in batches of at most GHOSTM_PAIR_BATCH_PAIRS
 * pairs (default: no limit) and GHOSTM_PAIR_SCRATCH_MB megabytes of hits and
 * records (default 1024); 20 bytes per hit and 16 per pair are read back. */
int PairJoinGpu(uint32_t npairs, const uint32_t pair_begin[], const uint32_t offset[], uint32_t nhits,
                const GhostmPairHit hit[], uint32_t max_span, uint32_t orient, GhostmLcaHit cand[],
                uint32_t partner[], GhostmPairOut out[]);

/* The same on the host, with no device call: the model the kernel equals
 * exactly, with the same checks and reasons. */
int GhostmPairJoinHost(uint32_t npairs, const uint32_t pair_begin[], const uint32_t offset[], uint32_t nhits,
                       const GhostmPairHit hit[], uint32_t max_span, uint32_t orient, GhostmLcaHit cand[],
                       uint32_t partner[], GhostmPairOut out[]);

/* The counters of the join, a struct of their own like GhostmReadLcaStats;
 * GhostmStats keeps its layout. */
typedef struct GhostmPairJoinStats {
  double seconds_pair;     /* k_pair_join, device time */
  uint64_t pair_launches;  /* batches of pairs with a hit */
  uint64_t pair_pairs;     /* pairs with a hit */
  uint64_t pair_hits;
  uint64_t pair_joined;    /* mate-1 candidates with a partner */
  uint64_t pair_taken;     /* mate-2 candidates some mate-1 candidate chose */
} GhostmPairJoinStats;

/* The counters behind the stage-level calls; GhostmStageReadCullStats'
 * conventions. */
size_t GhostmStagePairJoinStats(GhostmPairJoinStats *stats, size_t size);

/* The taxon profile of a sample: how many reads fall on each clade of the
 * resident taxonomy, and what is left once clades with only a handful of reads
 * are discounted. A histogram and a sum up the tree: all arithmetic is on
 * integers; the kernels equal the host model exactly.
 *
 * Input: the resident taxonomy (SetTaxonomyGpu), nreads reads, node[nreads] and
 * min_reads >= 1. node[r] is a node index, or 0xFFFFFFFF for a read without a
 * taxon (GhostmLcaOut.node is such a value).
 *
 *   direct(n)  the number of reads with node[r] == n.
 *   clade(n)   the number of reads whose node has n on its path to the root,
 *              ends included. It never shrinks towards the root.
 *   final(r)   the floor: the first node a met climbing from node[r] to the
 *              root, node[r] included, with clade(a) >= min_reads; 0xFFFFFFFF
 *              when node[r] is, or when even the root's clade is below
 *              min_reads. With min_reads == 1, final == node.
 *   kept(n)    the number of reads with final(r) == n.
 *
 * Output: one record per node with clade(n) > 0, in ascending node index; the
 * nodes under the floor are included, with kept_reads == 0. From the
 * definitions: the direct_reads add up to `classified`, the kept_reads to
 * `kept`; kept == classified when classified >= min_reads, else 0; the root's
 * clade_reads == classified whenever classified > 0. */
typedef struct GhostmTaxonCount {  /* 16 bytes */
  uint32_t node, clade_reads, direct_reads, kept_reads;
} GhostmTaxonCount;

typedef struct GhostmTaxonSummary {
  uint64_t reads;
  uint64_t classified;  /* node != none */
  uint64_t kept;        /* final != none */
  uint64_t moved;       /* final != none && final != node */
  uint64_t nodes;       /* records */
  uint64_t nodes_kept;  /* records with clade_reads >= min_reads */
} GhostmTaxonSummary;

/* TaxonProfileGpu (kernels k_taxon_count, k_taxon_climb, k_taxon_floor,
 * k_taxon_final, k_taxon_sort_tile, k_taxon_sort_step, k_taxon_emit) needs neither SetQueryGpu nor SetDbGpu.
 * out[cap] receives the records and *nout their number; final_node[nreads]
 * (may be NULL) every read's final node; *summary (may be NULL) the totals.
 * A call with cap == 0 and out == NULL asks for the count: it sets *nout,
 * writes nothing else and returns 0.
 * Everything is checked on the host before any upload or launch; a refused
 * call returns 1, writes nothing, and names its reason:
 *   "param"     min_reads == 0
 *   "null"      node null with nreads > 0; nout null; out null with cap > 0
 *   "taxonomy"  no taxonomy is resident
 *   "node"      a node that is neither 0xFFFFFFFF nor below nnodes; the read is
 *               named
 *   "cap"       more records than cap; the number needed is named. This one is
 *               known only after the counts, so kernels have run; nothing is
 *               written.
 * The work and the bytes read back follow the nodes the sample touches, not
 * the taxonomy's size: three count arrays of one word per node are allocated
 * and zeroed when the taxonomy becomes resident (again with every
 * SetTaxonomyGpu, freed by FreeGpu), a call reaches them through lists of the
 * nodes it counts on and puts those entries back to zero before it returns, a
 * refused call included. No call clears, scans or copies a whole array. The
 * reads go up in batches of at most GHOSTM_PROFILE_BATCH_READS reads (default:
 * no limit); the counts add up over the batches and the records do not depend
 * on the cuts. The list of touched nodes is ordered by node index on the
 * device, and 16 bytes per record come back. */
int TaxonProfileGpu(uint32_t nreads, const uint32_t node[], uint32_t min_reads, size_t cap, GhostmTaxonCount out[],
                    size_t *nout, uint32_t final_node[], GhostmTaxonSummary *summary);

/* The same on the host over the taxonomy given, with no device call: the model
 * the kernels equal exactly, with the same checks and reasons (and
 * SetTaxonomyGpu's for the taxonomy). */
int GhostmTaxonProfileHost(uint32_t nnodes, const uint32_t parent[], uint32_t nreads, const uint32_t node[],
                           uint32_t min_reads, size_t cap, GhostmTaxonCount out[], size_t *nout,
                           uint32_t final_node[], GhostmTaxonSummary *summary);

/* The counters of the profile, a struct of their own like GhostmReadLcaStats;
 * GhostmStats keeps its layout. */
typedef struct GhostmTaxonProfileStats {
  double seconds_profile;     /* k_taxon_*, device time */
  uint64_t profile_launches;  /* batches of reads counted (k_taxon_count launches) */
  uint64_t profile_reads;     /* reads of the calls that were not refused */
  uint64_t profile_nodes;     /* records of those calls */
} GhostmTaxonProfileStats;

/* The counters behind the stage-level calls; GhostmStageReadCullStats'
 * conventions. */
size_t GhostmStageTaxonProfileStats(GhostmTaxonProfileStats *stats, size_t size);

/* A session without a database: `aln`'s options without -d (giving it is an
 * error). With -i the query chunks are loaded as GhostmSessionCreate loads
 * them; without -i the session starts with neither input and the queries come
 * from GhostmSessionSetQueries*. The database comes from GhostmSessionSetDb /
 * GhostmSessionSetDbFasta, any number of times: one read set against many
 * databases, and with both setters a search needs no formatted file at all.
 * GhostmSessionRun before any database gives empty output and no hits. Returns
 * NULL on error. */
void *GhostmSessionCreateQueries(int argc, char **argv);

/* Replaces the session's database by n records given as letters, in the layout
 * of GhostmSessionSetQueries. k is given as `db -k` (the seed mask is 2^k - 1),
 * chunk_mb as `db -l` (0: db's default of 128). Afterwards the session holds
 * what a session created with -d P would hold after `ghostm db -i <that FASTA>
 * -o P -k k -l chunk_mb`: the same chunk cuts, residues, subject starts, names
 * and k-mer index, and the search space of the E-values is the new database's.
 * The letters are coded on the device straight into the resident chunks and
 * the index is built there from the device residues; only one word per chunk
 * (the number of positions) comes back, and no file is written. The results of
 * the previous run are dropped and the old chunks' device memory is kept for
 * re-use; the query chunks, the matrix and the options are untouched. Works on
 * any unsharded session, one created with -d included. Fails on a shard
 * session (its batch plan was agreed on the old database), on null arguments,
 * a record outside the letter buffer, a file that cannot be opened, k = 0 or a
 * seed of weight above 6, chunk_mb above 2047, and a record that alone is over
 * the chunk limit: all of these leave the session as it was. A failure while
 * the chunks are being loaded (from a FASTA file, a record over the chunk
 * limit is found only then) leaves the session with no database. Returns 0 on
 * success. */
int GhostmSessionSetDb(void *session, const uint8_t *raw, uint64_t raw_len, const uint64_t *offsets,
                       const uint32_t *lengths, const char *names, uint64_t names_len, uint32_t n, uint32_t k,
                       uint32_t chunk_mb);

/* The same from a FASTA file, read as `ghostm db` reads it. */
int GhostmSessionSetDbFasta(void *session, const char *path, uint32_t k, uint32_t chunk_mb);

/* One resident DB chunk: the values of its <p>_<id>.inf and .ind headers. */
typedef struct GhostmDbChunkInfo {
  uint32_t id, nseq, len, seed, kcl, npos;
} GhostmDbChunkInfo;

/* The session's DB chunks in order, file-loaded or set; the NULL/cap convention
 * of GhostmSessionHits. */
size_t GhostmSessionDbChunks(void *session, GhostmDbChunkInfo *info, size_t cap);

/* The residues of DB chunk `chunk` (the bytes of its .seq file) copied back
 * from the device; the convention of GhostmSessionQueryRecords. */
size_t GhostmSessionDbRecords(void *session, uint32_t chunk, uint8_t *codes, size_t cap);

/* The index of DB chunk `chunk` copied back from the device: keys_count (kcl
 * words) and positions (npos words) of its .ind file, each may be NULL; a cap
 * below the array's length is an error. Returns 0 on success. */
int GhostmSessionDbIndex(void *session, uint32_t chunk, uint32_t *keys_count, size_t kc_cap, uint32_t *positions,
                         size_t pos_cap);

/* The counters of the session's database sets. They are a struct of their own
 * and not fields of GhostmStats, whose layout and end stay as they are for
 * existing callers. All are 0 for a database read from formatted files. */
typedef struct GhostmDbSetStats {
  double seconds_db_format;         /* the resident database formatting of the last GhostmSessionSetDb*: the coding
                                       kernel (k_db_code) and the index build (index.hip), device time over its
                                       chunks */
  double seconds_db_code;           /* ... of which the coding kernel alone */
  uint64_t db_format_launches;      /* ... its DeviceModule::FormatDb passes (one per DB chunk) */
  uint64_t db_sets;                 /* GhostmSessionSetDb* calls that replaced the database, since creation */
  double seconds_db_read;           /* ... of the last one, host wall clock: reading the FASTA file and cutting it
                                       into chunks (0 for GhostmSessionSetDb) */
  double seconds_db_load;           /* ... packing the letters, names and starts, the staged upload, the subject
                                       table, without seconds_db_format */
} GhostmDbSetStats;

/* Copies min(size, sizeof(GhostmDbSetStats)) bytes and returns the library's
 * sizeof (the convention of GhostmSessionStatsSized); 0 on a null argument. */
size_t GhostmSessionDbStats(void *session, GhostmDbSetStats *stats, size_t size);

/* The chunk cuts of `ghostm db` on their own (host only, no device): over n
 * records of the given letter counts with `db -l chunk_mb` (0: the default). A
 * record joins the chunk while the sum of length + 1 stays within chunk_mb
 * MiB. The conventions of GhostmQueryChunkCuts. Returns -1 when a record alone
 * is over the limit, as the file's first record too (where `ghostm db` itself
 * silently writes a database without chunks), and when chunk_mb is above 2047
 * (the chunk's 32-bit offsets). */
int64_t GhostmDbChunkCuts(const uint32_t lengths[], uint64_t n, uint32_t chunk_mb, uint64_t cuts[], uint64_t cap);

/* Multi-GPU (the reference has no multi-GPU path, common.h:37):
 * one process per GPU, each opening a shard session. The query set selected by
 * -i/-S/-L is cut into `world` contiguous ranges of about equal residues, only
 * at name-group starts (a DNA read's six frames stay together: the reference
 * merges a group into one result list, aligner.cpp:697-700), and this session
 * searches range `rank` on the device given by -D. Hit records keep global
 * query indices, and the shards' outputs concatenated in rank order are the
 * unsharded output byte for byte; the data-path collective is the caller's
 * gather of GhostmSessionDeviceHits records (RCCL over xGMI). Returns NULL on
 * error. world = 1 is GhostmSessionCreate.
 *
 * Batch cuts: the reference's output depends on where its batch loop cuts a
 * query chunk (aligner.cpp:131-171, 511-514: carried result lists are re-sorted
 * every batch, a batch may split a name group, a chunk whose first query alone
 * exceeds -l ends early). A shard therefore replays the UNSHARDED run's batches
 * on its own queries (a batch that misses them is a pass over its carried
 * lists only). This batch plan is made at creation from the whole chunk's
 * candidate counts: GhostmSessionCreateShard reads every query of the set and
 * counts them all itself (K1 once, no communication); see
 * GhostmSessionCreateShardEx for the rank-local form. Every run re-derives its
 * counts and fails if they differ from the plan's. */
void *GhostmSessionCreateShard(int argc, char **argv, int rank, int world);

/* The collective GhostmSessionCreateShardEx calls (on the creating thread, the
 * same calls in the same order on every rank): an all-gather. Each rank passes
 * send_bytes bytes; recv receives every rank's buffer concatenated in rank
 * order, recv_bytes[r] bytes from rank r (known to all ranks). 0 = success. */
typedef int (*GhostmAllGatherFn)(void *ctx, const void *send, uint64_t send_bytes, void *recv,
                                 const uint64_t *recv_bytes);

/* GhostmSessionCreateShard for one process per GPU with a communicator: the
 * rank reads only the .seq rows and .nam lines of its own range (every rank
 * still derives the cut from all queries' residue counts and name-group
 * starts), counts only its own queries, and the ranks agree on the batch plan
 * with one all-gather of their candidate totals per (query chunk, DB chunk),
 * plus one of the per-query counts when some chunk needs more than one batch.
 * allgather == NULL is GhostmSessionCreateShard. */
void *GhostmSessionCreateShardEx(int argc, char **argv, int rank, int world, GhostmAllGatherFn allgather,
                                 void *ctx);

/* The query range [begin, end) of a shard session, as indices over the
 * selected chunks' queries (0, UINT64_MAX for an unsharded session). */
int GhostmSessionShardRange(void *session, uint64_t *begin, uint64_t *end);

/* The most hit records one run of this session can return: its name groups x
 * max(-b, 1) (each group keeps at most -b hits, reference aligner.cpp:742-760;
 * -b is read with atoi as aligner.cpp:251 does). A caller sizes its
 * GhostmSessionDeviceHits destination, or a fixed-capacity gather buffer, from
 * it. Returns UINT64_MAX for a null session. */
uint64_t GhostmSessionHitCapacity(void *session);

/* The shard rule on its own (host only, no device): cuts[0..world] over n
 * queries of the given weights; a cut falls only where group_start[i] != 0 and
 * is the first such i at or after the previous cut with
 * sum(weights[0..i)) * world >= sum(weights) * r. */
int GhostmShardCuts(uint64_t n, const uint32_t weights[], const uint8_t group_start[], int world,
                    uint64_t cuts[]);

/* Run the whole search with the CPU path's semantics (batch cuts, merge order,
 * tie rules) on the device. Results replace those of any previous run. */
int GhostmSessionRun(void *session);

/* GhostmSessionRun that also writes the -o file while the search runs: each
 * segment's text is written, in output order, as soon as it is formatted (the
 * reference writes after each query chunk, aligner.cpp:211). The file equals
 * what GhostmSessionWrite writes; GhostmSessionWrite is then a no-op. With
 * -y 6 (BLAST-tabular: qseqid sseqid pident length mismatch gapopen qstart qend
 * sstart send evalue bitscore, one-based coordinates, pident/evalue/bitscore as
 * -y 0 prints them) the text exists only after the GhostmHitExt post-pass, so
 * the file is written at the end of the run. -y 7 is -y 6 with columns 3 to 10
 * (pident = 100 * matches / length, length, mismatch, gapopen = the I and D
 * runs, qstart, qend, sstart, send) taken from the hit's GhostmHitPath and a
 * thirteenth column, the extended CIGAR (for instance 31=1X2D40=); it too is
 * written at the end of the run. -y 8 is the -y 7 line followed by three more
 * columns from the hit's GhostmHitRows: positives, qseq (the query row) and
 * sseq (the subject row), sixteen in all. -y 9 is a pairwise view, one block
 * of five lines per hit:
 *   # <the first fourteen -y 8 columns, tab-separated>
 *   Query\t<qstart>\t<query row>\t<qend>
 *   \t\t<midline>\t
 *   Sbjct\t<sstart>\t<subject row>\t<send>
 *   <empty line>
 * Both price hits like -y 0 and are written at the end of the run.
 * -y 10 replaces the hit lines by the pile-up's summary (GhostmSessionPileup):
 * one line per subject with at least one hit, in db_id order, tab-separated
 * integers after the name: subject name, length, hits, covered, depth_sum,
 * identities_sum, max_depth. -y 11 is that line with an eighth column, the
 * subject's consensus as text: the residue letter, '-' where depth > 0 and
 * consensus is 255, '.' where depth is 0. Neither prints an E-value, so like
 * -y 1 and -y 2 they need no Karlin parameters.
 * -y 12 prints the thirteen -y 7 columns from the hit's read-level path
 * (GhostmSessionHitsBand): pident, length, mismatch, gapopen, qstart, qend,
 * sstart, send and the CIGAR describe the whole read or frame against the
 * subject, one-based and in read or frame coordinates; evalue and bitscore come
 * from the read-level score, priced like every line of the session for a query
 * of the source's m letters (search space m x the database's residues, the
 * reference's float / double steps). A hit whose read-level score is 0 prints
 * its -y 7 line unchanged. The lines keep the order of the hits (-y 20 ranks and
 * culls them by the new scores). Written at the end of the run, like -y 7.
 * -y 13 (DNA sets of a tiled setter only) prints the thirteen -y 7 columns
 * from the hit's frame path (GhostmSessionHitsFrame) and two more, qframe and
 * frameshifts: length counts the '=', 'X', 'I' and 'D' columns, mismatch the
 * 'X', gapopen the runs of 'I' or 'D'; qstart / qend are one-based read
 * nucleotide coordinates, q_start + 1 and q_end + 1 on the forward strand,
 * n - q_start and n - q_end on the reverse strand (so qstart > qend there);
 * the CIGAR writes '\' and '/' for ops 4 and 5; qframe is +-(q_start % 3 + 1);
 * frameshifts is the summed length of the shift runs; evalue and bitscore are
 * priced as -y 12 prices them, for a query of m letters. A hit whose frame
 * score is 0 prints its tile path in the same units (strand positions
 * 3 x (offset + q) + g, the end + 2, frameshifts 0). The lines keep the order
 * of the hits (-y 21 ranks and culls them).
 * -y 16 and -y 17 are the -y 10 and -y 11 lines from the read-level pile-up of
 * the band paths (GhostmSessionReadPileup with frame = 0). -y 18 (DNA sets of a
 * tiled setter only, as -y 13) is the -y 10 line from the pile-up of the frame
 * paths with an eighth column, shifts_sum; -y 19 is the -y 18 line and a ninth
 * column, the consensus text as -y 11 writes it. Like -y 10 they print no
 * E-value and are written at the end of the run. */
int GhostmSessionRunToFile(void *session);

/* Formatted output of the last run (reference WriteOutput/V1/V2 text). With
 * buf == NULL returns the byte count; otherwise copies min(cap, size) bytes. */
size_t GhostmSessionOutput(void *session, char *buf, size_t cap);

/* Write the formatted output of the last run to the -o file. */
int GhostmSessionWrite(void *session);

/* Hit records of the last run in output order; same NULL/cap convention. */
size_t GhostmSessionHits(void *session, GhostmHit *hits, size_t cap);

/* The GhostmHitExt of every hit of the last run (record i belongs to hit i of
 * GhostmSessionHits); same NULL/cap convention, (size_t)-1 on error. Works
 * after a run with any -y: a post-pass of k_traceback_ext over the final hits,
 * grouped by (query chunk, DB chunk), computed on first use and kept until the
 * next run. A hit of a name group of several queries (a DNA read's frames) is
 * traced with the group's first query that reproduces its db_start, aln_len
 * and aln_match. */
size_t GhostmSessionHitsExt(void *session, GhostmHitExt *ext, size_t cap);

/* The GhostmHitPath of every hit of the last run (record i belongs to hit i)
 * and the run-length words they index; both with the NULL/cap convention of
 * GhostmSessionHitsExt, (size_t)-1 on error. s_start and s_end are relative to
 * the subject, like GhostmHit.db_start. Works after a run with any -y: one
 * TraceBackPathGpu-style call per (query chunk, DB chunk) that has hits, with
 * the known starts, computed on first use and kept until the next run. A hit
 * of a name group of several queries is traced with the query
 * GhostmSessionHitsExt resolved. */
size_t GhostmSessionHitsPath(void *session, GhostmHitPath *rec, size_t cap);
size_t GhostmSessionPathOps(void *session, uint32_t *ops, size_t cap);

/* The GhostmHitRows of every hit of the last run (record i belongs to hit i)
 * and the row bytes they index, in hit order; both with the NULL/cap
 * convention of GhostmSessionHitsPath, (size_t)-1 on error. Works after a run
 * with any -y and on shard sessions: computed on first use from the paths of
 * GhostmSessionHitsPath, one PathRowsGpu-style call per (query chunk, DB chunk)
 * that has hits, and kept until the next run or GhostmSessionSetQueries*.
 * query_record is the global index, over the query chunks in order, of the
 * record the hit was traced with (GhostmHit.query_id names the last record of
 * its name group instead). */
size_t GhostmSessionHitsRows(void *session, GhostmHitRows *rec, size_t cap);
size_t GhostmSessionRowBytes(void *session, uint8_t *rows, size_t cap);

/* The read-level path of every hit of the last run (record i belongs to hit i)
 * and the run-length words they index, in hit order; both with the NULL/cap
 * convention of GhostmSessionHitsPath, (size_t)-1 on error. Where the hit's
 * GhostmHitPath describes at most one tile record, this one aligns the whole
 * read or frame to the whole subject (the contract above BandAlignGpu):
 *   source   the read or frame whose tile the hit's resolved record is
 *            (GhostmHitRows.query_record's tile-table entry: record, frame,
 *            letters); on an untiled set every record is its own single-tile
 *            source with m its entry of GhostmSessionQueryLengths
 *   subject  the whole subject, so no alignment crosses an END
 *   anchor   the first cell of the hit's tile path: D = s_start (absolute) -
 *            (tile offset + q_start); the read-level score is therefore at
 *            least the tile path's whenever every cell of the tile path lies
 *            within the band of D
 * q_start / q_end are in read or frame coordinates (they may exceed 127),
 * s_start / s_end relative to the subject. Works after a run with any -y and on
 * shard sessions (each rank its own hits): one BandAlignGpu-style call per
 * (query chunk, DB chunk) that has hits, computed on first use and kept until
 * the next run, GhostmSessionSetQueries*, GhostmSessionSetDb* or change of
 * band. The records come in the order of GhostmSessionHits; ranking and
 * culling a read's hits by these scores is GhostmSessionReadCull's (-y 20). */
size_t GhostmSessionHitsBand(void *session, GhostmHitPath *rec, size_t cap);
size_t GhostmSessionBandOps(void *session, uint32_t *ops, size_t cap);

/* The band's half-width for GhostmSessionHitsBand: 1..31, default 31. A
 * refusal (non-zero) leaves the old value; a change drops the kept results. */
int GhostmSessionSetBand(void *session, uint32_t band);

/* The band counters of the session since its last run (all 0 until the band
 * results are asked for); the size convention of GhostmSessionDbStats. */
size_t GhostmSessionBandStats(void *session, GhostmBandStats *stats, size_t size);

/* Low-complexity masking of the session's query sets (the rule above
 * GhostmMaskRecordsHost). window 0 turns masking off, which is the default;
 * otherwise window 6..32 and 0 <= trigger <= extend <= 500 (a refusal names
 * "window" or "levels" and leaves the old setting). The setting takes effect at
 * the next GhostmSessionSetQueries* call: each chunk is masked on the device
 * straight after it is formatted, and only 4 bytes a record come back. The
 * current set and its results stay as they are. Refused on a shard session, as
 * the setters are. A set loaded from `qry`'s files is never masked.
 * GhostmSessionQueryRecords shows the masked records as they are;
 * GhostmSessionQueryLengths stays that of the unmasked set. */
int GhostmSessionSetMask(void *session, uint32_t window, uint32_t trigger, uint32_t extend);

/* The letters masked in every query record, in the indexing of
 * GhostmSessionQueryLengths; the NULL/cap convention of GhostmSessionHits. 0
 * entries for a set made with masking off. */
size_t GhostmSessionQueryMasked(void *session, uint32_t *masked, size_t cap);

/* The mask counters of the session's current query set (all 0 for a set made
 * with masking off); the size convention of GhostmSessionDbStats. */
size_t GhostmSessionMaskStats(void *session, GhostmMaskStats *stats, size_t size);

/* Quality trimming and masking of the session's FASTQ and quality-carrying
 * query sets (the rule above GhostmQualityTrimHost). 0, 0, 0 is off, the
 * default; otherwise trim_q and mask_q 0..93 and min_len 0..2^24 (a refusal
 * names "param" and leaves the old setting). The setting takes effect at the
 * next GhostmSessionSetQueriesFastq*Tiled / GhostmSessionSetQueriesQualTiled
 * call; the current set and its results stay as they are. Refused on a shard
 * session, as the setters are. */
int GhostmSessionSetQuality(void *session, uint32_t trim_q, uint32_t mask_q, uint32_t min_len);

/* GhostmSessionSetQueriesFastaTiled from a FASTQ file: strict four-line records
 * ('@' name, letters, '+' line, qualities of the letters' length; CRLF is
 * tolerated; blank lines only between records and at the end; the name is the
 * header after '@' with leading blanks dropped, as for '>'). Multi-line FASTQ
 * and compressed files are not read. A malformed file is refused with
 * "fastq: record N: <reason>", N counted from 1.
 * The path: the file is parsed, the quality stage runs on all reads (when it is
 * on), read r enters as letters[begin, begin + kept) under its name, max_len
 * then cuts what was kept, and the set is tiled as ever. A read left empty stays
 * a source record with one all-X tile per frame, so record indices and mates do
 * not move. Every read coordinate the session reports is relative to the kept
 * stretch; GhostmSessionQueryQuality's begin converts it back.
 * A read with a quality byte outside '!'..'~' refuses the set ("fastq: record N:
 * quality byte outside '!'..'~'"). Any refusal leaves the session as it was.
 * With quality off the stage is not launched and the set is that of the FASTA
 * file of the same names and letters. */
int GhostmSessionSetQueriesFastqTiled(void *session, const char *path, uint32_t width, int dna, uint32_t chunk_mb,
                                      uint32_t max_len, uint32_t step, uint64_t *cut_records);
/* The same over two FASTQ files of mates (GhostmSessionSetQueriesFastaMatesTiled):
 * a mate left empty stays a record, so the pairing holds. */
int GhostmSessionSetQueriesFastqMatesTiled(void *session, const char *path1, const char *path2, uint32_t width,
                                           int dna, uint32_t chunk_mb, uint32_t max_len, uint32_t step,
                                           uint64_t *cut_records);
/* The letters form: GhostmSessionSetQueriesTiled's arguments with the reads'
 * quality bytes, qual[raw_len] laid out as raw. raw is not changed. */
int GhostmSessionSetQueriesQualTiled(void *session, const uint8_t *raw, const uint8_t *qual, uint64_t raw_len,
                                     const uint64_t *offsets, const uint32_t *lengths, const char *names,
                                     uint64_t names_len, uint32_t n, uint32_t width, int dna, uint32_t chunk_mb,
                                     uint32_t max_len, uint32_t step);

/* One record per source read of the current set, in the reads' order; the
 * NULL/cap convention of GhostmSessionHits. 0 entries when the quality stage did
 * not run for the set. */
size_t GhostmSessionQueryQuality(void *session, GhostmQualOut *out, size_t cap);

/* The quality counters of the session's current query set (all 0 when the stage
 * did not run); the size convention of GhostmSessionDbStats. */
size_t GhostmSessionQualityStats(void *session, GhostmQualStats *stats, size_t size);

/* Adapter removal on the session's FASTQ and quality-carrying query sets (the
 * rule above GhostmAdapterTrimHost). Both adapters empty or NULL and
 * pair_overlap 0 is off, the default; a refusal names "param" or "adapter" and
 * leaves the old setting. The setting takes effect at the next
 * GhostmSessionSetQueriesFastq*Tiled / GhostmSessionSetQueriesQualTiled call;
 * the current set and its results stay as they are. Refused on a shard
 * session, as the setters are.
 * In those setters the stage runs first, over the whole set in the records'
 * order (the mates of two files interleaved, so records 2i and 2i + 1 are
 * mates; GhostmSessionSetMates is independent of it). Each read then enters the
 * quality stage and the tiler as its first `kept` letters: the quality rule
 * sees the cut read, its `bad` counts the cut read's bytes, and with quality
 * off the set is that of the reads cut by hand. A protein set is refused
 * ("adapters: a protein set"), and so is an odd record count with
 * pair_overlap > 0 ("adapters: pairs: ..."); any refusal leaves the session as
 * it was. While the stage is off nothing is launched and nothing changes. */
int GhostmSessionSetAdapters(void *session, const char *adapter1, const char *adapter2, uint32_t min_overlap,
                             uint32_t err_pct, uint32_t pair_overlap);

/* One record per source read of the current set, in the reads' order; the
 * NULL/cap convention of GhostmSessionHits. 0 entries when the adapter stage
 * did not run for the set. */
size_t GhostmSessionQueryAdapters(void *session, GhostmAdapterOut *out, size_t cap);

/* The adapter counters of the session's current query set (all 0 when the
 * stage did not run); the size convention of GhostmSessionDbStats. */
size_t GhostmSessionAdapterStats(void *session, GhostmAdapterStats *stats, size_t size);

/* The frameshift-aware read-level path of every hit of the last run (record i
 * belongs to hit i) and the run-length words they index, in hit order (the
 * contract above FrameAlignGpu); the NULL/cap convention of
 * GhostmSessionHitsBand, (size_t)-1 on error. The query set must be a DNA set
 * made by a tiled setter (a read of one tile is fine); any other set is an
 * error. Per hit:
 *   source   the strand of the hit's resolved tile: frame f of the tile table
 *            gives strand f / 3, and first_record is the frame's own first
 *            record minus f % 3
 *   subject  the whole subject
 *   anchor   D as GhostmSessionHitsBand computes it, a codon diagonal
 * q_start / q_end are strand positions (nucleotides; the reverse strand counted
 * from the read's last kept nucleotide), s_start / s_end relative to the
 * subject. One FrameAlignGpu-style call per (query chunk, DB chunk) that has
 * hits, computed on first use and kept until the next run,
 * GhostmSessionSetQueries*, GhostmSessionSetDb*, a change of band or of the
 * frameshift cost. The records come in the order of GhostmSessionHits; ranking
 * and culling by these scores is GhostmSessionReadCull's with frame = 1 (-y 21). */
size_t GhostmSessionHitsFrame(void *session, GhostmHitPath *rec, size_t cap);
size_t GhostmSessionFrameOps(void *session, uint32_t *ops, size_t cap);

/* One GhostmHitFrameInfo per hit, beside GhostmSessionHitsFrame's records;
 * the same conventions. */
size_t GhostmSessionFrameInfo(void *session, GhostmHitFrameInfo *info, size_t cap);

/* The frameshift cost of GhostmSessionHitsFrame: -(1 << 20)..0, default -15.
 * A refusal (non-zero) leaves the old value; a change drops the kept results. */
int GhostmSessionSetFrameShift(void *session, int shift_cost);

/* The frame counters of the session since its last run (all 0 until the frame
 * results are asked for); the size convention of GhostmSessionBandStats. */
size_t GhostmSessionFrameStats(void *session, GhostmFrameStats *stats, size_t size);

/* The GhostmHitReadRows of every hit's read-level path (record i belongs to hit
 * i) and the row bytes they index, in hit order: the Band pair from the paths
 * of GhostmSessionHitsBand, the Frame pair from those of GhostmSessionHitsFrame
 * with the session's frameshift cost. The NULL/cap convention of
 * GhostmSessionHitsRows, (size_t)-1 on error; the Frame pair is refused where
 * GhostmSessionHitsFrame is. One ReadRowsGpu-style call per (query chunk, DB
 * chunk) that has hits, computed on first use and kept as long as the paths
 * they were made from (until the next run, GhostmSessionSetQueries*,
 * GhostmSessionSetDb*, a change of band, and for the Frame pair of the
 * frameshift cost). Works after a run with any -y and on shard sessions.
 * query_record is the global index of the record holding the path's first
 * query letter; a hit of read-level score 0 has columns 0. */
size_t GhostmSessionHitsBandRows(void *session, GhostmHitReadRows *rec, size_t cap);
size_t GhostmSessionBandRowBytes(void *session, uint8_t *rows, size_t cap);
size_t GhostmSessionHitsFrameRows(void *session, GhostmHitReadRows *rec, size_t cap);
size_t GhostmSessionFrameRowBytes(void *session, uint8_t *rows, size_t cap);

/* The read-rows counters of the session since its last run (all 0 until the
 * read-level rows are asked for); the size convention of
 * GhostmSessionBandStats. */
size_t GhostmSessionReadRowsStats(void *session, GhostmReadRowsStats *stats, size_t size);

/* The pile-up of the last run's hits on every subject (the definitions above
 * PathPileupGpu), built on the paths of GhostmSessionHitsPath with the record
 * each hit was traced with, so a DNA hit piles up the frame that reproduced
 * it. GhostmSessionPileup returns one GhostmSubjectPileup per subject over all
 * DB chunks, in db_id order; GhostmSessionPileupArrays the subjects' depth,
 * identities and consensus, concatenated in db_id order without the END
 * separators (subject i begins at subj[i].offset; a NULL array is skipped).
 * Both return the count with subj == NULL / all arrays NULL, else copy
 * min(cap, count) elements; (size_t)-1 on error. Works after a run with any
 * -y: per (DB chunk, profile window) one k_pileup launch per query chunk with
 * hits there, then k_pileup_finish and 9 bytes per position read back; the
 * summary is made on the host. Computed on first use and kept until the next
 * run or GhostmSessionSetQueries*. A shard session piles up its own hits:
 * depth, identities, the profile and the summary's hits, depth_sum and
 * identities_sum add up across the ranks; consensus, covered and max_depth do
 * not and have to be made again from the summed arrays. */
size_t GhostmSessionPileup(void *session, GhostmSubjectPileup *subj, size_t cap);
size_t GhostmSessionPileupArrays(void *session, uint32_t *depth, uint32_t *identities,
                                 uint8_t *consensus, size_t cap);

/* The full 32-slot rows of subject db_id: length x 32 values (NULL: the
 * count), made on demand by the same kernels on that subject's hits only;
 * nothing is kept. (size_t)-1 on error (a db_id outside the loaded chunks). */
size_t GhostmSessionSubjectProfile(void *session, uint32_t db_id, uint32_t *profile, size_t cap);

/* The read-level pile-up of the last run's hits (the definitions above
 * ReadPileupGpu): GhostmSessionPileup's three calls on the read-level paths,
 * frame = 0 those of GhostmSessionHitsBand, frame = 1 those of
 * GhostmSessionHitsFrame, with the sources those passes aligned and the subject
 * coordinates made absolute in the chunk again. The conventions are
 * GhostmSessionPileup*'s; shifts is a fourth array (NULL is skipped; all 0 with
 * frame = 0). frame = 1 is refused where GhostmSessionHitsFrame is. A hit of
 * read-level score 0 counts in hits and adds nothing. Computed on first use and
 * kept as long as the paths they were made from: until the next run,
 * GhostmSessionSetQueries*, GhostmSessionSetDb*, a change of band and, for
 * frame = 1, of the frameshift cost. A shard session piles up its own hits:
 * depth, identities, shifts, the profile and the sums add up across the ranks;
 * covered, max_depth and consensus do not. GhostmSessionReadSubjectProfile
 * keeps nothing, like GhostmSessionSubjectProfile. */
size_t GhostmSessionReadPileup(void *session, int frame, GhostmSubjectReadPileup *subj, size_t cap);
size_t GhostmSessionReadPileupArrays(void *session, int frame, uint32_t *depth, uint32_t *identities,
                                     uint8_t *consensus, uint32_t *shifts, size_t cap);
size_t GhostmSessionReadSubjectProfile(void *session, int frame, uint32_t db_id, uint32_t *profile,
                                       size_t cap);

/* The read-level pile-up counters of the session since its last run (all 0
 * until the read-level pile-up is asked for); the size convention of
 * GhostmSessionBandStats. */
size_t GhostmSessionReadPileupStats(void *session, GhostmReadPileupStats *stats, size_t size);

/* The cull of the last run's hits by their read-level alignments (the contract
 * is above ReadCullGpu): one GhostmCullOut per hit of GhostmSessionHits, from
 * the records of GhostmSessionHitsBand (frame = 0) or GhostmSessionHitsFrame
 * (frame = 1, a DNA set of a tiled setter). With out NULL returns the count,
 * else copies min(cap, count) records and returns that; (size_t)-1 on error.
 *   reads     a read is a maximal run of consecutive hits whose resolved
 *             records have the same source record in the tile table; on an
 *             untiled set a read is the name group. detail of a DUP is an index
 *             of GhostmSessionHits.
 *   subject   GhostmHit.db_id; s_lo, s_hi: the path's subject range
 *   score     the path's score; a hit whose read-level score is 0 is EMPTY
 *   q_lo, q_hi  the path's interval in forward-strand read units: letters on a
 *             protein set; on a DNA set of a tiled setter nucleotides from 0 at
 *             both levels: the frame path's interval as -y 13 prints it (less
 *             1, sorted), the band path's frame letters c of frame f as 3c + f
 *             % 3 to 3c + f % 3 + 2 on the strand, turned round on the reverse
 *             strand with the read's kept n. Hits of the two strands land on
 *             the same coordinates, so they cull each other.
 * One ReadCullGpu-style pass over all hits (its batches and variables).
 * Computed on first use; kept until the next run, query set, database, SetBand
 * (and SetFrameShift for frame = 1) or SetCull. -y 20 prints, per read, the
 * -y 12 line of every KEPT hit in kept_rank order with two more columns, rank
 * (kept_rank) and covered (d); -y 21 the same from the -y 13 line. */
size_t GhostmSessionReadCull(void *session, int frame, GhostmCullOut *out, size_t cap);
/* top_k 1..255 (default 1) and cover_pct 1..100 (default 50) of the session's
 * cull; a change drops the kept result. Returns 0, or 1 ("param"). */
int GhostmSessionSetCull(void *session, uint32_t top_k, uint32_t cover_pct);
/* The cull's counters since the last run began; GhostmSessionBandStats'
 * conventions. */
size_t GhostmSessionReadCullStats(void *session, GhostmReadCullStats *stats, size_t size);
/* Tile groups: with on != 0, from the next tiled setter on a name group also
 * ends where the tile table begins a new tile (every record of a protein set,
 * every six records of a DNA set), so the search keeps the best -b hits per
 * tile and not per read, and a read that carries two genes keeps hits of both.
 * The hit capacity grows with the group count. Off by default: then nothing
 * differs. A shard session refuses it as it refuses a tiled set. Returns 0, or
 * 1 on error. */
int GhostmSessionSetTileGroups(void *session, int on);

/* A taxonomy for the session's resident database (the contract is above
 * ReadLcaGpu). taxid[nnodes] are the printed labels, distinct and at least 1 (0
 * is printed for "unclassified"); parent[nnodes] as SetTaxonomyGpu takes it;
 * subject_node[nsubjects] is indexed by GhostmHit.db_id and holds a node or
 * 0xFFFFFFFF. nsubjects must equal the resident database's subject count over
 * all chunks, else the call is refused with "subjects"; "taxonomy" and "null" as
 * SetTaxonomyGpu, "taxonomy" also for a taxid of 0 or a repeated one, "node"
 * for a subject_node that is neither. The call also makes the stage-level
 * taxonomy resident. GhostmSessionSetDb* drop the taxonomy; a refused call
 * leaves the session as it was. Returns 0, or 1 on error. */
int GhostmSessionSetTaxonomy(void *session, uint32_t nnodes, const uint32_t taxid[], const uint32_t parent[],
                             size_t nsubjects, const uint32_t subject_node[]);
/* The same from two text files.
 * Nodes file: per line two unsigned integers, taxid and parent taxid, separated
 * by any run of tabs, spaces and '|'; further fields are ignored, so NCBI's
 * nodes.dmp reads as it is; blank lines are skipped. The root has itself as
 * parent. A parent that no line defines or a repeated taxid is refused with
 * "taxonomy" and the line number.
 * Map file: per line name, whitespace, taxid. name is compared with each
 * subject's name up to its first space or tab; a later line for the same name
 * wins; a taxid the nodes lack is refused with "map"; a name the database lacks
 * is counted, not refused; a subject without a line is unmapped. */
int GhostmSessionSetTaxonomyFiles(void *session, const char *nodes_path, const char *map_path);
typedef struct GhostmTaxonomyInfo {
  uint64_t nodes;             /* 0: no taxonomy */
  uint64_t subjects_mapped;
  uint64_t subjects_unmapped;
  uint64_t map_unmatched;     /* map lines whose name no subject has (file form) */
} GhostmTaxonomyInfo;
size_t GhostmSessionTaxonomyInfo(void *session, GhostmTaxonomyInfo *info, size_t size);
/* top_pct 0..100 (default 10) and support_pct 51..100 (default 100) of the
 * session's assignment; a change drops the kept result. Returns 0, or 1
 * ("param"). */
int GhostmSessionSetLca(void *session, uint32_t top_pct, uint32_t support_pct);
/* One GhostmLcaOut per read of GhostmSessionReadCull(session, frame, ...), with
 * the same definition of a read, built from that result: score is the
 * read-level score of a KEPT hit, else 0; q_lo, q_hi are the cull's; node =
 * subject_node[db_id]. node and lca are node indices (taxid[] labels them).
 * With out NULL returns the count of reads, else copies min(cap, count) records
 * and returns that; (size_t)-1 on error: "taxonomy" without one, and
 * GhostmSessionReadCull's errors. Computed on first use; dropped by everything
 * that drops the cull's result, by SetLca and by SetTaxonomy*. -y 22 (band
 * paths) and -y 23 (frame paths) print one line per read with hits, in read
 * order, tab separated:
 *   qname taxid depth votes support lca_taxid candidates unmapped best_score
 * taxid and lca_taxid are 0 when the read has no vote. */
size_t GhostmSessionReadLca(void *session, int frame, GhostmLcaOut *out, size_t cap);
/* Each read's first hit as an index of GhostmSessionHits, plus the end: one
 * more entry than GhostmSessionReadLca has records. */
size_t GhostmSessionReadLcaBegin(void *session, int frame, uint32_t *read_begin, size_t cap);
/* The assignment's counters since the last run began; GhostmSessionBandStats'
 * conventions. */
size_t GhostmSessionReadLcaStats(void *session, GhostmReadLcaStats *stats, size_t size);

/* The sample's taxon profile (the contract is above TaxonProfileGpu), built
 * from GhostmSessionReadLca(session, frame, ...)'s node field: one read per
 * ReadLca record. min_reads >= 1 (default 1) is the floor; a change drops only
 * the profile, not the assignment under it. Returns 0, or 1 ("param"). */
int GhostmSessionSetProfile(void *session, uint32_t min_reads);
/* The records, in ascending node index (taxid[] labels them). ReadLca's
 * conventions: with out NULL returns the count, else copies min(cap, count)
 * records and returns that; (size_t)-1 on error (GhostmSessionReadLca's).
 * Computed on first use by one TaxonProfileGpu call; dropped by everything
 * that drops the assignment and by SetProfile. -y 24 (band paths) and -y 25
 * (frame paths) print the sample's report, tab separated:
 *   percent clade_reads kept_reads direct_reads depth taxid parent_taxid
 * percent is clade_reads of the ReadLca record count `total` in hundredths of
 * a per cent, (clade_reads * 10000 + total / 2) / total in 64 bits, printed
 * I.FF. The first line is the unclassified reads (total - kept) when there
 * are any: taxid 0, depth 0, parent_taxid 0 and all three counts that number.
 * Then the nodes with clade_reads >= min_reads in depth-first pre-order from
 * the root, a node's children by clade_reads descending, then taxid ascending;
 * the root prints its own taxid as its parent's. A run without hits writes an
 * empty file. `search -R min_reads` sets the floor. */
size_t GhostmSessionTaxonProfile(void *session, int frame, GhostmTaxonCount *out, size_t cap);
/* Every read's final node: one entry per ReadLca record. */
size_t GhostmSessionTaxonProfileFinal(void *session, int frame, uint32_t *final_node, size_t cap);
/* The profile's totals, sized like GhostmSessionTaxonomyInfo: min(size, the
 * library's sizeof) bytes are written; returns the library's sizeof, 0 on a
 * null argument, (size_t)-1 on error. */
size_t GhostmSessionTaxonProfileSummary(void *session, int frame, GhostmTaxonSummary *summary, size_t size);
/* The profile's counters since the last run began; GhostmSessionBandStats'
 * conventions. */
size_t GhostmSessionTaxonProfileStats(void *session, GhostmTaxonProfileStats *stats, size_t size);

/* Mate pairs on a session (the contract is above PairJoinGpu). on != 0
 * declares source records 2i and 2i + 1 of a tiled query set to be the mates of
 * pair i; max_insert, 1..2^24 (default 1000), is the longest fragment in read
 * units (nucleotides on a DNA set). The join's max_span is max_insert on a
 * protein set and max_insert / 3 (at least 1) on a DNA set; orient is 1 on a
 * DNA set (the mates' hits lie on opposite strands) and 0 on a protein set.
 * Off by default: nothing of this runs and every other result is as without
 * it. A change drops only the pair results and the profile counted from them;
 * a shard session refuses the call. A pair pass fails with "mates" and the
 * reason while mates are off, on an untiled set and on an odd number of source
 * records. With mates on, GhostmSessionTaxonProfile* count fragments: one per
 * GhostmSessionPairLca record instead of one per GhostmSessionReadLca record. */
int GhostmSessionSetMates(void *session, int on, uint32_t max_insert);
/* GhostmSessionSetQueriesFastaTiled over two files of mates: record i of path1
 * and record i of path2 become source records 2i and 2i + 1. Files of
 * different record counts are refused, both counts named; a refusal leaves the
 * old set in place. */
int GhostmSessionSetQueriesFastaMatesTiled(void *session, const char *path1, const char *path2, uint32_t width,
                                           int dna, uint32_t chunk_mb, uint32_t max_len, uint32_t step,
                                           uint64_t *cut_records);
/* The join of every pair's hits, from GhostmSessionReadCull(session, frame,
 * ...): one PairJoinGpu-style pass over all hits of GhostmSessionHits, a KEPT
 * hit a candidate with the cull's record (GhostmCullHit's fields), its
 * subject's node (0xFFFFFFFF without a taxonomy) and its strand (frame / 3 of
 * the hit's tile on a DNA set, else 0), every other hit with score 0. The
 * hits are grouped by source record >> 1 and & 1, offset is mate 1's length. A
 * pair is there when either mate has a hit. cand and partner (either may be
 * NULL) get one entry per hit; partner indexes GhostmSessionHits. Made on first
 * use; kept as long as the cull's and the assignment's results and
 * GhostmSessionSetMates' parameters. With both NULL the call returns the
 * number of hits, else the number copied (at most cap); (size_t)-1 on error. */
size_t GhostmSessionPairJoin(void *session, int frame, GhostmLcaHit *cand, uint32_t *partner, size_t cap);
/* The pairs of that join (each array may be NULL): one GhostmPairOut per pair,
 * pair_begin with two entries per pair and one more (mate 1's and mate 2's
 * first hit, then the end), pair_record mate 1's source record, which names the
 * pair. With all NULL the number of pairs, else the number copied (at most cap
 * pairs; pair_begin gets 2 * that + 1 entries). */
size_t GhostmSessionPairJoinPairs(void *session, int frame, GhostmPairOut *out, uint32_t *pair_begin,
                                  uint32_t *pair_record, size_t cap);
/* One GhostmLcaOut per pair: one ReadLcaGpu-style pass over the joined
 * candidates with the pairs as reads, under GhostmSessionSetLca's top_pct and
 * support_pct. Needs a taxonomy. GhostmSessionReadLca's conventions. */
size_t GhostmSessionPairLca(void *session, int frame, GhostmLcaOut *out, size_t cap);
/* The join's counters since the last run began; GhostmSessionBandStats'
 * conventions. (The pairs' assignment counts into GhostmSessionReadLcaStats.) */
size_t GhostmSessionPairJoinStats(void *session, GhostmPairJoinStats *stats, size_t size);

/* The same records resident on the session's GPU, for a device-to-device
 * gather across ranks: copies min(n, cap) records to dst_device
 * (device memory on the session's GPU; NULL only counts) and returns n, or
 * (size_t)-1 on error. */
size_t GhostmSessionDeviceHits(void *session, void *dst_device, size_t cap);

int GhostmSessionStats(void *session, GhostmStats *stats);

/* The same with the caller's struct size: GhostmStats only ever grows by
 * fields appended at its end, so a caller built against an older header
 * passes its sizeof and gets exactly the fields it knows (min(size, the
 * library's sizeof) bytes are written). Returns the library's sizeof, or 0 on
 * a null argument. */
size_t GhostmSessionStatsSized(void *session, GhostmStats *stats, size_t size);

/* The stage-level calls (SearchNextGpu, CountCandidatesGpu, CalculateScoreGpu,
 * TraceBackGpu and the other calls on the chunks of SetQueryGpu / SetDbGpu)
 * belong to no session; this reads the device module's timings and counters
 * behind them, sized like GhostmSessionStatsSized. The device-side fields
 * (seconds_seed/score/traceback*, the *_launches*, *_cells, score_rechecks,
 * seed_*, and the post-pass counters) are filled, the others are 0. The
 * counters add up over the process's stage calls and start again at 0 with
 * every GhostmSessionRun, so a caller takes the difference around its calls:
 * which K2 encoding a CalculateScoreGpu chose, which K3 formulation a
 * TraceBackGpu. No device call. Returns the library's sizeof, or 0 on a null
 * argument. */
size_t GhostmStageStats(GhostmStats *stats, size_t size);

void GhostmSessionDestroy(void *session);

/* `ghostm aln ...` end to end (create + run + write + destroy). Exit status like
 * the reference CLI: errors are printed and 0 is still returned (main.cpp:116-121). */
int GhostmAlignMain(int argc, char **argv);

/* `ghostm search [aln options except -i -o -S -L] [-q d|p] [-w maxLength]
 * [-c chunkSizeMB] [-B band] [-F cost] (-d database | -f db.fasta [-k kSize] [-m chunkSizeMB])
 * q1.fasta out1 [q2.fasta out2 ...]`: one session with the database resident,
 * from its formatted files (-d) or formatted on the device from FASTA (-f, with
 * -k and -m as db's -k and -l: GhostmSessionCreateQueries and one
 * GhostmSessionSetDbFasta); for each pair the queries are set from the FASTA
 * file (-q, -w, -c as qry's -t, -l, -L; qry's warnings on stderr) and searched
 * into the output file, which equals [`ghostm db` +] `ghostm qry` + `ghostm
 * aln` on those files. -B sets the half-width of -y 12's band
 * (GhostmSessionSetBand; it applies to -y 13 too), -F the non-negative
 * frameshift cost of -y 13 (GhostmSessionSetFrameShift with its negative; a
 * cost that is negative or over 1 << 20 is wrong usage). Wrong usage (no pairs, an odd number of positionals,
 * -i, -o, -S or -L, both or neither of -d and -f, -B outside 1..31) returns 1 before any device
 * call; errors are printed and 0 returned, as GhostmAlignMain. */
int GhostmSearchMain(int argc, char **argv);

#ifdef __cplusplus
}
#endif

#endif /* GHOSTM_HIP_H_ */
