"""ctypes binding of the C ABI in include/ghostm_hip.h (libghostm_hip.so).

The library is built in-tree (ghostm_amd/lib) by `__graft_entry__.build()` /
`make -C ghostm_amd/csrc`. There is no fallback: if the library is missing or a
symbol is absent, loading raises, so nothing silently runs on the CPU.
"""
from __future__ import annotations

import ctypes
import os
import re
from ctypes import POINTER, c_char_p, c_float, c_int, c_size_t, c_uint32, c_uint64, c_void_p

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_DIR = os.path.dirname(PKG_DIR)
# GHOSTM_LIB_PATH selects another build of the same library (A/B timing runs)
LIB_PATH = os.environ.get("GHOSTM_LIB_PATH") or os.path.join(PKG_DIR, "lib", "libghostm_hip.so")
BIN_PATH = os.path.join(PKG_DIR, "bin", "ghostm")
HEADER_PATH = os.path.join(REPO_DIR, "include", "ghostm_hip.h")

u32p = POINTER(c_uint32)

# GhostmAllGatherFn (include/ghostm_hip.h): int (*)(void *ctx, const void *send,
# uint64_t send_bytes, void *recv, const uint64_t *recv_bytes)
ALLGATHER_FN = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_uint64, c_void_p, POINTER(c_uint64))


class GhostmHit(ctypes.Structure):
    """reference Alignment fields gathered per hit (alignment.h:136-145)."""

    _fields_ = [
        ("query_id", c_uint32),
        ("db_id", c_uint32),
        ("score", c_uint32),
        ("db_start", c_uint32),
        ("db_end", c_uint32),
        ("aln_len", c_uint32),
        ("aln_match", c_uint32),
        ("seq_id", c_float),
    ]


class GhostmHitExt(ctypes.Structure):
    """what the BLAST-tabular columns need beyond a GhostmHit (16 bytes, zero-based)."""

    _fields_ = [
        ("q_start", c_uint32),
        ("q_end", c_uint32),
        ("mismatches", c_uint32),
        ("gap_opens", c_uint32),
    ]


class GhostmQueryTile(ctypes.Structure):
    """one output record of a tiled query set (16 bytes): the source record, the
    tile's first letter in the record or frame, the source's letters, the frame."""

    _fields_ = [
        ("record", c_uint32),
        ("offset", c_uint32),
        ("letters", c_uint32),
        ("frame", c_uint32),
    ]


class GhostmHitPath(ctypes.Structure):
    """the alignment path of one hit (32 bytes): zero-based inclusive coordinates,
    its score and its run-length words ops[ops_offset : ops_offset + n_runs]."""

    _fields_ = [
        ("q_start", c_uint32),
        ("q_end", c_uint32),
        ("s_start", c_uint32),
        ("s_end", c_uint32),
        ("score", c_uint32),
        ("n_runs", c_uint32),
        ("ops_offset", c_uint64),
    ]


class GhostmBandSource(ctypes.Structure):
    """one source of the read-level band pass (16 bytes): its tile records in the
    resident query chunk and its letters."""

    _fields_ = [
        ("first_record", c_uint32),
        ("stride", c_uint32),
        ("tiles", c_uint32),
        ("letters", c_uint32),
    ]


class GhostmMaskStats(ctypes.Structure):
    """the counters of the mask pass (GhostmSessionMaskStats, GhostmStageMaskStats)."""

    _fields_ = [
        ("seconds_mask", ctypes.c_double),
        ("mask_launches", ctypes.c_uint64),
        ("mask_sources", ctypes.c_uint64),
        ("mask_windows", ctypes.c_uint64),
        ("masked_sources", ctypes.c_uint64),
        ("masked_letters", ctypes.c_uint64),
    ]


class GhostmQualOut(ctypes.Structure):
    """one read's record of the quality stage (GhostmQualityTrimHost, GhostmSessionQueryQuality)."""

    _fields_ = [
        ("begin", ctypes.c_uint32),
        ("kept", ctypes.c_uint32),
        ("masked", ctypes.c_uint32),
        ("bad", ctypes.c_uint32),
    ]


class GhostmQualStats(ctypes.Structure):
    """the counters of the quality stage (GhostmSessionQualityStats, GhostmStageQualStats)."""

    _fields_ = [
        ("launches", ctypes.c_uint64),
        ("reads", ctypes.c_uint64),
        ("letters", ctypes.c_uint64),
        ("trimmed5", ctypes.c_uint64),
        ("trimmed3", ctypes.c_uint64),
        ("masked", ctypes.c_uint64),
        ("failed", ctypes.c_uint64),
        ("bad", ctypes.c_uint64),
        ("seconds_quality", ctypes.c_double),
    ]


class GhostmAdapterOut(ctypes.Structure):
    """one read's record of the adapter stage (GhostmAdapterTrimHost, GhostmSessionQueryAdapters)."""

    _fields_ = [
        ("kept", ctypes.c_uint32),
        ("adapter_at", ctypes.c_uint32),
        ("pair_len", ctypes.c_uint32),
        ("adapter_mismatches", ctypes.c_uint16),
        ("pair_mismatches", ctypes.c_uint16),
    ]


class GhostmAdapterStats(ctypes.Structure):
    """the counters of the adapter stage (GhostmSessionAdapterStats, GhostmStageAdapterStats)."""

    _fields_ = [
        ("launches", ctypes.c_uint64),
        ("reads", ctypes.c_uint64),
        ("letters", ctypes.c_uint64),
        ("cut_reads", ctypes.c_uint64),
        ("cut_letters", ctypes.c_uint64),
        ("adapter_found", ctypes.c_uint64),
        ("pair_found", ctypes.c_uint64),
        ("pair_skipped", ctypes.c_uint64),
        ("emptied", ctypes.c_uint64),
        ("seconds_adapter", ctypes.c_double),
    ]


class GhostmBandStats(ctypes.Structure):
    """the counters of the band pass (GhostmSessionBandStats, GhostmStageBandStats)."""

    _fields_ = [
        ("seconds_band", ctypes.c_double),
        ("band_launches", c_uint64),
        ("band_hits", c_uint64),
        ("band_cells", c_uint64),
        ("band_dir_bytes", c_uint64),
    ]


class GhostmFrameStats(ctypes.Structure):
    """the counters of the frame pass (GhostmSessionFrameStats, GhostmStageFrameStats)."""

    _fields_ = [
        ("seconds_frame", ctypes.c_double),
        ("frame_launches", c_uint64),
        ("frame_hits", c_uint64),
        ("frame_cells", c_uint64),
        ("frame_dir_bytes", c_uint64),
    ]


class GhostmHitFrameInfo(ctypes.Structure):
    """what GhostmSessionFrameInfo tells about a hit's frame path (16 bytes)."""

    _fields_ = [
        ("strand", c_uint32),
        ("read_nt", c_uint32),
        ("letters", c_uint32),
        ("shifts", c_uint32),
    ]


class GhostmHitRows(ctypes.Structure):
    """the aligned rows of one hit (32 bytes): the record the path lies in, its
    counts and its 3 * columns bytes rows[rows_offset:] (query row, midline,
    subject row)."""

    _fields_ = [
        ("query_record", c_uint32),
        ("columns", c_uint32),
        ("identities", c_uint32),
        ("positives", c_uint32),
        ("gap_residues", c_uint32),
        ("rescore", ctypes.c_int32),
        ("rows_offset", c_uint64),
    ]


class GhostmHitReadRows(ctypes.Structure):
    """the aligned rows of one read-level hit (40 bytes): GhostmHitRows' fields
    (query_record: the record of the path's first query letter), then the shift
    columns."""

    _fields_ = GhostmHitRows._fields_ + [
        ("shifts", c_uint32),
        ("pad", c_uint32),
    ]


class GhostmReadRowsStats(ctypes.Structure):
    """the counters of the read-level rows pass (GhostmSessionReadRowsStats,
    GhostmStageReadRowsStats)."""

    _fields_ = [
        ("seconds_read_rows", ctypes.c_double),
        ("read_rows_launches", c_uint64),
        ("read_rows_hits", c_uint64),
        ("read_rows_columns", c_uint64),
    ]


class GhostmSubjectPileup(ctypes.Structure):
    """one subject's summary of the pile-up (40 bytes); offset is its first
    element in the session-level depth / identities / consensus arrays."""

    _fields_ = [
        ("length", c_uint32),
        ("hits", c_uint32),
        ("covered", c_uint32),
        ("max_depth", c_uint32),
        ("depth_sum", c_uint64),
        ("identities_sum", c_uint64),
        ("offset", c_uint64),
    ]


class GhostmSubjectReadPileup(ctypes.Structure):
    """one subject's summary of the read-level pile-up (48 bytes):
    GhostmSubjectPileup's fields, then the summed shift columns."""

    _fields_ = GhostmSubjectPileup._fields_ + [
        ("shifts_sum", c_uint64),
    ]


class GhostmReadPileupStats(ctypes.Structure):
    """the counters of the read-level pile-up (GhostmSessionReadPileupStats,
    GhostmStageReadPileupStats)."""

    _fields_ = [
        ("seconds_read_pileup", ctypes.c_double),
        ("read_pileup_launches", c_uint64),
        ("read_pileup_windows", c_uint64),
        ("read_pileup_parts", c_uint64),
        ("read_pileup_columns", c_uint64),
        ("read_pileup_shifts", c_uint64),
    ]


class GhostmCullHit(ctypes.Structure):
    """one hit of the read-level cull (24 bytes): subject, score, the inclusive
    ranges on the read and on the subject."""

    _fields_ = [
        ("subject", c_uint32),
        ("score", c_uint32),
        ("q_lo", c_uint32),
        ("q_hi", c_uint32),
        ("s_lo", c_uint32),
        ("s_hi", c_uint32),
    ]


class GhostmCullOut(ctypes.Structure):
    """one hit's record of the read-level cull (16 bytes)."""

    _fields_ = [
        ("order", c_uint32),
        ("status", c_uint32),
        ("kept_rank", c_uint32),
        ("detail", c_uint32),
    ]


class GhostmReadCullStats(ctypes.Structure):
    """the counters of the read-level cull (GhostmSessionReadCullStats,
    GhostmStageReadCullStats)."""

    _fields_ = [
        ("seconds_cull", ctypes.c_double),
        ("cull_launches", c_uint64),
        ("cull_reads", c_uint64),
        ("cull_hits", c_uint64),
        ("cull_kept", c_uint64),
        ("cull_dups", c_uint64),
        ("cull_culled", c_uint64),
    ]


class GhostmLcaHit(ctypes.Structure):
    """one hit of the per-read taxonomic assignment (16 bytes): the subject's
    node or 0xFFFFFFFF, the score (0: not a candidate), the inclusive stretch
    of the read."""

    _fields_ = [
        ("node", c_uint32),
        ("score", c_uint32),
        ("q_lo", c_uint32),
        ("q_hi", c_uint32),
    ]


class GhostmLcaOut(ctypes.Structure):
    """one read's record of the assignment (32 bytes)."""

    _fields_ = [
        ("node", c_uint32),
        ("depth", c_uint32),
        ("votes", c_uint32),
        ("support", c_uint32),
        ("lca", c_uint32),
        ("candidates", c_uint32),
        ("unmapped", c_uint32),
        ("best_score", c_uint32),
    ]


class GhostmReadLcaStats(ctypes.Structure):
    """the counters of the assignment (GhostmSessionReadLcaStats,
    GhostmStageReadLcaStats)."""

    _fields_ = [
        ("seconds_lca", ctypes.c_double),
        ("lca_launches", c_uint64),
        ("lca_reads", c_uint64),
        ("lca_hits", c_uint64),
        ("lca_votes", c_uint64),
        ("lca_assigned", c_uint64),
    ]


class GhostmPairHit(ctypes.Structure):
    """one hit of the mate-pair join (32 bytes): the subject and its node, the
    score (0: not a candidate), the inclusive ranges on the hit's own mate and
    on the subject, the strand."""

    _fields_ = [
        ("subject", c_uint32),
        ("node", c_uint32),
        ("score", c_uint32),
        ("q_lo", c_uint32),
        ("q_hi", c_uint32),
        ("s_lo", c_uint32),
        ("s_hi", c_uint32),
        ("strand", c_uint32),
    ]


class GhostmPairOut(ctypes.Structure):
    """one pair's record of the join (16 bytes)."""

    _fields_ = [
        ("joined", c_uint32),
        ("mates", c_uint32),
        ("best_score", c_uint32),
        ("best_span", c_uint32),
    ]


class GhostmPairJoinStats(ctypes.Structure):
    """the counters of the join (GhostmStagePairJoinStats)."""

    _fields_ = [
        ("seconds_pair", ctypes.c_double),
        ("pair_launches", c_uint64),
        ("pair_pairs", c_uint64),
        ("pair_hits", c_uint64),
        ("pair_joined", c_uint64),
        ("pair_taken", c_uint64),
    ]


class GhostmTaxonCount(ctypes.Structure):
    """one node's record of the taxon profile (16 bytes)."""

    _fields_ = [
        ("node", c_uint32),
        ("clade_reads", c_uint32),
        ("direct_reads", c_uint32),
        ("kept_reads", c_uint32),
    ]


class GhostmTaxonSummary(ctypes.Structure):
    """the totals of a taxon profile (TaxonProfileGpu, GhostmSessionTaxonProfileSummary)."""

    _fields_ = [(n, c_uint64) for n in ("reads", "classified", "kept", "moved", "nodes", "nodes_kept")]


class GhostmTaxonProfileStats(ctypes.Structure):
    """the counters of the profile (GhostmSessionTaxonProfileStats,
    GhostmStageTaxonProfileStats)."""

    _fields_ = [
        ("seconds_profile", ctypes.c_double),
        ("profile_launches", c_uint64),
        ("profile_reads", c_uint64),
        ("profile_nodes", c_uint64),
    ]


class GhostmTaxonomyInfo(ctypes.Structure):
    """a session's taxonomy (GhostmSessionTaxonomyInfo)."""

    _fields_ = [
        ("nodes", c_uint64),
        ("subjects_mapped", c_uint64),
        ("subjects_unmapped", c_uint64),
        ("map_unmatched", c_uint64),
    ]


class GhostmDbChunkInfo(ctypes.Structure):
    """one resident DB chunk: the values of its .inf and .ind headers."""

    _fields_ = [(n, c_uint32) for n in ("id", "nseq", "len", "seed", "kcl", "npos")]


class GhostmDbSetStats(ctypes.Structure):
    """the counters of a session's database sets (GhostmSessionDbStats)."""

    _fields_ = [
        ("seconds_db_format", ctypes.c_double),
        ("seconds_db_code", ctypes.c_double),
        ("db_format_launches", c_uint64),
        ("db_sets", c_uint64),
        ("seconds_db_read", ctypes.c_double),
        ("seconds_db_load", ctypes.c_double),
    ]


class GhostmStats(ctypes.Structure):
    _fields_ = [
        ("seconds_total", ctypes.c_double),
        ("seconds_seed", ctypes.c_double),
        ("seconds_score", ctypes.c_double),
        ("seconds_traceback", ctypes.c_double),
        ("seconds_merge", ctypes.c_double),
        ("seconds_output", ctypes.c_double),
        ("queries", c_uint64),
        ("query_residues", c_uint64),
        ("candidates", c_uint64),
        ("score_cells", c_uint64),
        ("tracebacks", c_uint64),
        ("traceback_cells", c_uint64),
        ("hits", c_uint64),
        ("batches", c_uint64),
        ("score_launches", c_uint64),
        ("seed_bytes", c_uint64),
        ("score_launches_packed", c_uint64),
        ("score_launches_half", c_uint64),
        ("traceback_launches", c_uint64),
        ("traceback_launches_key", c_uint64),
        ("seed_runs_hash", c_uint64),
        ("score_rechecks", c_uint64),
        ("traceback_launches_scan", c_uint64),
        ("traceback_scan_cells", c_uint64),
        ("merge_launches", c_uint64),
        ("merge_launches_wave", c_uint64),
        ("score_launches_framed", c_uint64),
        ("seed_queries_class", c_uint64 * 4),
        ("seed_queries_wide", c_uint64),
        ("segments", c_uint64),
        ("seed_runs_filter", c_uint64),
        ("seed_filter_overflows", c_uint64),
        ("score_launches_swar", c_uint64),
        ("traceback_launches_scan_swar", c_uint64),
        ("seed_list_entries", c_uint64),
        ("score_launches_unit", c_uint64),
        ("traceback_launches_strips", c_uint64),
        ("seconds_traceback_scan", ctypes.c_double),
        ("score_launches_pair", c_uint64),
        ("seed_table_full", c_uint64),
        ("seed_compact_redo", c_uint64),
        ("score_launches_sparse", c_uint64),
        ("traceback_launches_keyframe", c_uint64),
        ("score_launches_levels", c_uint64),
        ("seconds_traceback_ext", ctypes.c_double),
        ("traceback_ext_launches", c_uint64),
        ("traceback_ext_cells", c_uint64),
        ("seconds_traceback_path", ctypes.c_double),
        ("traceback_path_launches", c_uint64),
        ("traceback_path_cells", c_uint64),
        ("traceback_path_dir_bytes", c_uint64),
        ("seconds_query_format", ctypes.c_double),
        ("query_format_launches", c_uint64),
        ("query_sets", c_uint64),
        ("seconds_query_read", ctypes.c_double),
        ("seconds_query_load", ctypes.c_double),
        ("seconds_path_rows", ctypes.c_double),
        ("path_rows_launches", c_uint64),
        ("path_rows_columns", c_uint64),
        ("path_rows_bytes", c_uint64),
        ("seconds_pileup", ctypes.c_double),
        ("pileup_launches", c_uint64),
        ("pileup_windows", c_uint64),
        ("pileup_parts", c_uint64),
        ("pileup_columns", c_uint64),
    ]

    def as_dict(self) -> dict:
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            if name == "seed_queries_class":
                for k in range(4):
                    out[f"seed_queries_class{k}"] = v[k]
            else:
                out[name] = v
        return out


# name -> (restype, argtypes); covers every function declared in the header
SIGNATURES = {
    "InitGpu": (c_int, []),
    "GetNeededGPUMemorySize": (c_size_t, [c_uint32] * 6),
    "CheckGpuMemory": (c_int, [c_uint32] * 6),
    "SetOptionGpu": (c_int, [c_uint32, POINTER(c_int), c_int]),
    "printGpuInfo": (None, [c_int]),
    "SetQueryGpu": (c_int, [POINTER(ctypes.c_uint8), c_uint32, c_uint32]),
    "SetDbGpu": (c_int, [POINTER(ctypes.c_uint8), c_uint32, u32p, c_uint32, u32p, c_uint32]),
    "SearchNextGpu": (c_uint32, [c_uint32] * 8 + [u32p, u32p]),
    "CalculateScoreGpu": (None, [c_uint32, c_uint32, c_uint32, u32p, u32p, c_uint32, c_uint32, c_int, c_int]),
    "FreeGpu": (c_int, []),
    "GhostmGetLastError": (c_char_p, []),
    "GhostmBuildInfo": (c_char_p, []),
    "GhostmDevicePoolTrim": (c_uint64, []),
    "GhostmDevicePoolInfo": (c_int, [POINTER(c_uint64), POINTER(c_uint64)]),
    "CountCandidatesGpu": (c_int, [c_uint32] * 6 + [u32p]),
    "TraceBackGpu": (c_int, [c_uint32, u32p, u32p, c_uint32, c_uint32, c_int, c_int, u32p, u32p, u32p, POINTER(c_float)]),
    "TraceBackExtGpu": (c_int, [c_uint32, u32p, u32p, u32p, c_uint32, c_uint32, c_int, c_int, u32p, u32p, u32p,
                                POINTER(GhostmHitExt)]),
    "GhostmTraceBackExtHost": (c_int, [POINTER(ctypes.c_uint8), c_uint32, c_uint32, POINTER(ctypes.c_uint8), c_uint32,
                                       POINTER(c_int), c_uint32, u32p, u32p, c_uint32, c_int, c_int, u32p, u32p, u32p,
                                       POINTER(GhostmHitExt)]),
    "TraceBackPathGpu": (c_int, [c_uint32, u32p, u32p, u32p, c_uint32, c_uint32, c_int, c_int, POINTER(GhostmHitPath),
                                 u32p, c_size_t, POINTER(c_size_t)]),
    "GhostmTraceBackPathHost": (c_int, [POINTER(ctypes.c_uint8), c_uint32, c_uint32, POINTER(ctypes.c_uint8), c_uint32,
                                        POINTER(c_int), c_uint32, u32p, u32p, u32p, c_uint32, c_int, c_int,
                                        POINTER(GhostmHitPath), u32p, c_size_t, POINTER(c_size_t)]),
    "PathRowsGpu": (c_int, [c_uint32, u32p, POINTER(GhostmHitPath), u32p, c_size_t, c_uint32, c_int, c_int,
                            POINTER(GhostmHitRows), POINTER(ctypes.c_uint8), c_size_t, POINTER(c_size_t)]),
    "GhostmPathRowsHost": (c_int, [POINTER(ctypes.c_uint8), c_uint32, c_uint32, POINTER(ctypes.c_uint8), c_uint32,
                                   POINTER(c_int), c_uint32, u32p, POINTER(GhostmHitPath), u32p, c_size_t, c_uint32,
                                   c_int, c_int, POINTER(GhostmHitRows), POINTER(ctypes.c_uint8), c_size_t,
                                   POINTER(c_size_t)]),
    "PathPileupGpu": (c_int, [c_uint32, u32p, POINTER(GhostmHitPath), u32p, c_size_t, c_uint32, c_uint32, u32p, u32p,
                              POINTER(ctypes.c_uint8), u32p]),
    "GhostmPathPileupHost": (c_int, [POINTER(ctypes.c_uint8), c_uint32, c_uint32, POINTER(ctypes.c_uint8), c_uint32,
                                     POINTER(c_int), c_uint32, u32p, POINTER(GhostmHitPath), u32p, c_size_t, c_uint32,
                                     u32p, u32p, POINTER(ctypes.c_uint8), u32p]),
    "BandAlignGpu": (c_int, [c_uint32, POINTER(GhostmBandSource), POINTER(ctypes.c_int32), u32p, u32p, c_uint32,
                             c_uint32, c_uint32, c_int, c_int, POINTER(GhostmHitPath), u32p, c_size_t,
                             POINTER(c_size_t)]),
    "GhostmBandAlignHost": (c_int, [POINTER(ctypes.c_uint8), c_uint32, c_uint32, POINTER(ctypes.c_uint8), c_uint32,
                                    POINTER(c_int), c_uint32, POINTER(GhostmBandSource), POINTER(ctypes.c_int32), u32p,
                                    u32p, c_uint32, c_uint32, c_uint32, c_int, c_int, POINTER(GhostmHitPath), u32p,
                                    c_size_t, POINTER(c_size_t)]),
    "GhostmStageBandStats": (c_size_t, [POINTER(GhostmBandStats), c_size_t]),
    "GhostmMaskRecordsHost": (c_int, [POINTER(ctypes.c_uint8), c_uint32, c_uint32, c_uint32, POINTER(GhostmBandSource),
                                      c_uint32, c_uint32, c_uint32, c_uint32, u32p]),
    "MaskRecordsGpu": (c_int, [POINTER(ctypes.c_uint8), c_uint32, c_uint32, c_uint32, POINTER(GhostmBandSource),
                               c_uint32, c_uint32, c_uint32, c_uint32, u32p]),
    "GhostmStageMaskStats": (c_size_t, [POINTER(GhostmMaskStats), c_size_t]),
    "GhostmQualityTrimHost": (c_int, [POINTER(ctypes.c_uint8), POINTER(ctypes.c_uint8), c_uint64, POINTER(c_uint64),
                                      u32p, c_uint32, c_uint32, c_uint32, c_uint32, POINTER(GhostmQualOut)]),
    "QualityTrimGpu": (c_int, [POINTER(ctypes.c_uint8), POINTER(ctypes.c_uint8), c_uint64, POINTER(c_uint64), u32p,
                               c_uint32, c_uint32, c_uint32, c_uint32, POINTER(GhostmQualOut)]),
    "GhostmStageQualStats": (c_size_t, [POINTER(GhostmQualStats), c_size_t]),
    "GhostmAdapterTrimHost": (c_int, [POINTER(ctypes.c_uint8), c_uint64, POINTER(c_uint64), u32p, c_uint32, c_char_p,
                                      c_char_p, c_uint32, c_uint32, c_uint32, POINTER(GhostmAdapterOut)]),
    "AdapterTrimGpu": (c_int, [POINTER(ctypes.c_uint8), c_uint64, POINTER(c_uint64), u32p, c_uint32, c_char_p,
                               c_char_p, c_uint32, c_uint32, c_uint32, POINTER(GhostmAdapterOut)]),
    "GhostmStageAdapterStats": (c_size_t, [POINTER(GhostmAdapterStats), c_size_t]),
    "FrameAlignGpu": (c_int, [c_uint32, POINTER(GhostmBandSource), POINTER(ctypes.c_int32), u32p, u32p, c_uint32,
                              c_uint32, c_uint32, c_int, c_int, c_int, POINTER(GhostmHitPath), u32p, c_size_t,
                              POINTER(c_size_t)]),
    "GhostmFrameAlignHost": (c_int, [POINTER(ctypes.c_uint8), c_uint32, c_uint32, POINTER(ctypes.c_uint8), c_uint32,
                                     POINTER(c_int), c_uint32, POINTER(GhostmBandSource), POINTER(ctypes.c_int32),
                                     u32p, u32p, c_uint32, c_uint32, c_uint32, c_int, c_int, c_int,
                                     POINTER(GhostmHitPath), u32p, c_size_t, POINTER(c_size_t)]),
    "GhostmStageFrameStats": (c_size_t, [POINTER(GhostmFrameStats), c_size_t]),
    "ReadRowsGpu": (c_int, [c_uint32, POINTER(GhostmBandSource), POINTER(GhostmHitPath), u32p, c_size_t, c_uint32,
                            c_uint32, c_int, c_int, c_int, c_int, POINTER(GhostmHitReadRows), POINTER(ctypes.c_uint8),
                            c_size_t, POINTER(c_size_t)]),
    "GhostmReadRowsHost": (c_int, [POINTER(ctypes.c_uint8), c_uint32, c_uint32, POINTER(ctypes.c_uint8), c_uint32,
                                   POINTER(c_int), c_uint32, POINTER(GhostmBandSource), POINTER(GhostmHitPath), u32p,
                                   c_size_t, c_uint32, c_uint32, c_int, c_int, c_int, c_int,
                                   POINTER(GhostmHitReadRows), POINTER(ctypes.c_uint8), c_size_t, POINTER(c_size_t)]),
    "GhostmStageReadRowsStats": (c_size_t, [POINTER(GhostmReadRowsStats), c_size_t]),
    "ReadPileupGpu": (c_int, [c_uint32, POINTER(GhostmBandSource), POINTER(GhostmHitPath), u32p, c_size_t, c_uint32,
                              c_uint32, c_int, c_uint32, u32p, u32p, POINTER(ctypes.c_uint8), u32p, u32p]),
    "GhostmReadPileupHost": (c_int, [POINTER(ctypes.c_uint8), c_uint32, c_uint32, POINTER(ctypes.c_uint8), c_uint32,
                                     c_uint32, POINTER(GhostmBandSource), POINTER(GhostmHitPath), u32p, c_size_t,
                                     c_uint32, c_uint32, c_int, u32p, u32p, POINTER(ctypes.c_uint8), u32p, u32p]),
    "GhostmStageReadPileupStats": (c_size_t, [POINTER(GhostmReadPileupStats), c_size_t]),
    "ReadCullGpu": (c_int, [c_uint32, u32p, c_uint32, POINTER(GhostmCullHit), c_uint32, c_uint32,
                            POINTER(GhostmCullOut)]),
    "GhostmReadCullHost": (c_int, [c_uint32, u32p, c_uint32, POINTER(GhostmCullHit), c_uint32, c_uint32,
                                   POINTER(GhostmCullOut)]),
    "GhostmStageReadCullStats": (c_size_t, [POINTER(GhostmReadCullStats), c_size_t]),
    "SetTaxonomyGpu": (c_int, [c_uint32, u32p]),
    "GhostmTaxonomyDepths": (c_int, [c_uint32, u32p, u32p]),
    "ReadLcaGpu": (c_int, [c_uint32, u32p, c_uint32, POINTER(GhostmLcaHit), c_uint32, c_uint32, POINTER(GhostmLcaOut)]),
    "GhostmReadLcaHost": (c_int, [c_uint32, u32p, c_uint32, u32p, c_uint32, POINTER(GhostmLcaHit), c_uint32, c_uint32,
                                  POINTER(GhostmLcaOut)]),
    "GhostmStageReadLcaStats": (c_size_t, [POINTER(GhostmReadLcaStats), c_size_t]),
    "PairJoinGpu": (c_int, [c_uint32, u32p, u32p, c_uint32, POINTER(GhostmPairHit), c_uint32, c_uint32,
                            POINTER(GhostmLcaHit), u32p, POINTER(GhostmPairOut)]),
    "GhostmPairJoinHost": (c_int, [c_uint32, u32p, u32p, c_uint32, POINTER(GhostmPairHit), c_uint32, c_uint32,
                                   POINTER(GhostmLcaHit), u32p, POINTER(GhostmPairOut)]),
    "GhostmStagePairJoinStats": (c_size_t, [POINTER(GhostmPairJoinStats), c_size_t]),
    "TaxonProfileGpu": (c_int, [c_uint32, u32p, c_uint32, c_size_t, POINTER(GhostmTaxonCount), POINTER(c_size_t), u32p,
                                POINTER(GhostmTaxonSummary)]),
    "GhostmTaxonProfileHost": (c_int, [c_uint32, u32p, c_uint32, u32p, c_uint32, c_size_t, POINTER(GhostmTaxonCount),
                                       POINTER(c_size_t), u32p, POINTER(GhostmTaxonSummary)]),
    "GhostmStageTaxonProfileStats": (c_size_t, [POINTER(GhostmTaxonProfileStats), c_size_t]),
    "GhostmBuildIndexGpu": (c_int, [POINTER(ctypes.c_uint8), c_uint32, c_uint32, c_uint32, u32p, u32p, u32p, c_int,
                                    POINTER(c_float)]),
    "GhostmFormatQueriesGpu": (c_int, [POINTER(ctypes.c_uint8), c_uint64, POINTER(c_uint64), u32p, c_uint32, c_uint32,
                                       c_uint32, POINTER(ctypes.c_uint8), c_int, POINTER(c_float)]),
    "GhostmKarlinUngapped": (c_int, [POINTER(c_int), POINTER(c_float), POINTER(c_float), POINTER(c_float)]),
    "GhostmReadScoreMatrix": (c_int, [c_char_p, POINTER(c_int)]),
    "GhostmLengthAdjustment": (c_int, [c_float, c_float, c_float, c_float, c_int, c_uint32, c_int, POINTER(c_int)]),
    "GhostmSessionCreate": (c_void_p, [c_int, POINTER(c_char_p)]),
    "GhostmSessionCreateDb": (c_void_p, [c_int, POINTER(c_char_p)]),
    "GhostmSessionSetQueries": (c_int, [c_void_p, POINTER(ctypes.c_uint8), c_uint64, POINTER(c_uint64), u32p, c_char_p,
                                        c_uint64, c_uint32, c_uint32, c_int, c_uint32]),
    "GhostmSessionSetQueriesFasta": (c_int, [c_void_p, c_char_p, c_uint32, c_int, c_uint32, POINTER(c_uint64)]),
    "GhostmSessionSetOutputFile": (c_int, [c_void_p, c_char_p]),
    "GhostmSessionQueryLengths": (c_size_t, [c_void_p, u32p, c_size_t]),
    "GhostmSessionQueryRecords": (c_size_t, [c_void_p, c_uint32, POINTER(ctypes.c_uint8), c_size_t]),
    "GhostmQueryChunkCuts": (ctypes.c_int64, [u32p, c_uint64, c_uint32, c_int, POINTER(c_uint64), c_uint64]),
    "GhostmSessionSetQueriesTiled": (c_int, [c_void_p, POINTER(ctypes.c_uint8), c_uint64, POINTER(c_uint64), u32p,
                                             c_char_p, c_uint64, c_uint32, c_uint32, c_int, c_uint32, c_uint32,
                                             c_uint32]),
    "GhostmSessionSetQueriesFastaTiled": (c_int, [c_void_p, c_char_p, c_uint32, c_int, c_uint32, c_uint32, c_uint32,
                                                  POINTER(c_uint64)]),
    "GhostmSessionQueryTiles": (c_size_t, [c_void_p, POINTER(GhostmQueryTile), c_size_t]),
    "GhostmQueryTilePlan": (ctypes.c_int64, [u32p, c_uint64, c_uint32, c_int, c_uint32, c_uint32,
                                             POINTER(GhostmQueryTile), c_uint64, POINTER(c_uint64)]),
    "GhostmSessionCreateQueries": (c_void_p, [c_int, POINTER(c_char_p)]),
    "GhostmSessionSetDb": (c_int, [c_void_p, POINTER(ctypes.c_uint8), c_uint64, POINTER(c_uint64), u32p, c_char_p,
                                   c_uint64, c_uint32, c_uint32, c_uint32]),
    "GhostmSessionSetDbFasta": (c_int, [c_void_p, c_char_p, c_uint32, c_uint32]),
    "GhostmSessionDbChunks": (c_size_t, [c_void_p, POINTER(GhostmDbChunkInfo), c_size_t]),
    "GhostmSessionDbRecords": (c_size_t, [c_void_p, c_uint32, POINTER(ctypes.c_uint8), c_size_t]),
    "GhostmSessionDbIndex": (c_int, [c_void_p, c_uint32, u32p, c_size_t, u32p, c_size_t]),
    "GhostmSessionDbStats": (c_size_t, [c_void_p, POINTER(GhostmDbSetStats), c_size_t]),
    "GhostmDbChunkCuts": (ctypes.c_int64, [u32p, c_uint64, c_uint32, POINTER(c_uint64), c_uint64]),
    "GhostmSessionCreateShard": (c_void_p, [c_int, POINTER(c_char_p), c_int, c_int]),
    "GhostmSessionCreateShardEx": (c_void_p, [c_int, POINTER(c_char_p), c_int, c_int, c_void_p, c_void_p]),
    "GhostmSessionShardRange": (c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
    "GhostmSessionHitCapacity": (c_uint64, [c_void_p]),
    "GhostmShardCuts": (c_int, [c_uint64, u32p, POINTER(ctypes.c_uint8), c_int, POINTER(c_uint64)]),
    "GhostmSessionRun": (c_int, [c_void_p]),
    "GhostmSessionRunToFile": (c_int, [c_void_p]),
    "GhostmSessionOutput": (c_size_t, [c_void_p, c_char_p, c_size_t]),
    "GhostmSessionWrite": (c_int, [c_void_p]),
    "GhostmSessionHits": (c_size_t, [c_void_p, POINTER(GhostmHit), c_size_t]),
    "GhostmSessionHitsExt": (c_size_t, [c_void_p, POINTER(GhostmHitExt), c_size_t]),
    "GhostmSessionHitsPath": (c_size_t, [c_void_p, POINTER(GhostmHitPath), c_size_t]),
    "GhostmSessionPathOps": (c_size_t, [c_void_p, u32p, c_size_t]),
    "GhostmSessionHitsBand": (c_size_t, [c_void_p, POINTER(GhostmHitPath), c_size_t]),
    "GhostmSessionBandOps": (c_size_t, [c_void_p, u32p, c_size_t]),
    "GhostmSessionSetBand": (c_int, [c_void_p, c_uint32]),
    "GhostmSessionBandStats": (c_size_t, [c_void_p, POINTER(GhostmBandStats), c_size_t]),
    "GhostmSessionSetMask": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32]),
    "GhostmSessionQueryMasked": (c_size_t, [c_void_p, u32p, c_size_t]),
    "GhostmSessionMaskStats": (c_size_t, [c_void_p, POINTER(GhostmMaskStats), c_size_t]),
    "GhostmSessionSetQuality": (c_int, [c_void_p, c_uint32, c_uint32, c_uint32]),
    "GhostmSessionSetQueriesFastqTiled": (c_int, [c_void_p, c_char_p, c_uint32, c_int, c_uint32, c_uint32, c_uint32,
                                                  POINTER(c_uint64)]),
    "GhostmSessionSetQueriesFastqMatesTiled": (c_int, [c_void_p, c_char_p, c_char_p, c_uint32, c_int, c_uint32,
                                                       c_uint32, c_uint32, POINTER(c_uint64)]),
    "GhostmSessionSetQueriesQualTiled": (c_int, [c_void_p, POINTER(ctypes.c_uint8), POINTER(ctypes.c_uint8), c_uint64,
                                                 POINTER(c_uint64), u32p, c_char_p, c_uint64, c_uint32, c_uint32,
                                                 c_int, c_uint32, c_uint32, c_uint32]),
    "GhostmSessionQueryQuality": (c_size_t, [c_void_p, POINTER(GhostmQualOut), c_size_t]),
    "GhostmSessionQualityStats": (c_size_t, [c_void_p, POINTER(GhostmQualStats), c_size_t]),
    "GhostmSessionSetAdapters": (c_int, [c_void_p, c_char_p, c_char_p, c_uint32, c_uint32, c_uint32]),
    "GhostmSessionQueryAdapters": (c_size_t, [c_void_p, POINTER(GhostmAdapterOut), c_size_t]),
    "GhostmSessionAdapterStats": (c_size_t, [c_void_p, POINTER(GhostmAdapterStats), c_size_t]),
    "GhostmSessionHitsFrame": (c_size_t, [c_void_p, POINTER(GhostmHitPath), c_size_t]),
    "GhostmSessionFrameOps": (c_size_t, [c_void_p, u32p, c_size_t]),
    "GhostmSessionFrameInfo": (c_size_t, [c_void_p, POINTER(GhostmHitFrameInfo), c_size_t]),
    "GhostmSessionSetFrameShift": (c_int, [c_void_p, c_int]),
    "GhostmSessionFrameStats": (c_size_t, [c_void_p, POINTER(GhostmFrameStats), c_size_t]),
    "GhostmSessionHitsBandRows": (c_size_t, [c_void_p, POINTER(GhostmHitReadRows), c_size_t]),
    "GhostmSessionBandRowBytes": (c_size_t, [c_void_p, POINTER(ctypes.c_uint8), c_size_t]),
    "GhostmSessionHitsFrameRows": (c_size_t, [c_void_p, POINTER(GhostmHitReadRows), c_size_t]),
    "GhostmSessionFrameRowBytes": (c_size_t, [c_void_p, POINTER(ctypes.c_uint8), c_size_t]),
    "GhostmSessionReadRowsStats": (c_size_t, [c_void_p, POINTER(GhostmReadRowsStats), c_size_t]),
    "GhostmSessionHitsRows": (c_size_t, [c_void_p, POINTER(GhostmHitRows), c_size_t]),
    "GhostmSessionRowBytes": (c_size_t, [c_void_p, POINTER(ctypes.c_uint8), c_size_t]),
    "GhostmSessionPileup": (c_size_t, [c_void_p, POINTER(GhostmSubjectPileup), c_size_t]),
    "GhostmSessionPileupArrays": (c_size_t, [c_void_p, u32p, u32p, POINTER(ctypes.c_uint8), c_size_t]),
    "GhostmSessionSubjectProfile": (c_size_t, [c_void_p, c_uint32, u32p, c_size_t]),
    "GhostmSessionReadPileup": (c_size_t, [c_void_p, c_int, POINTER(GhostmSubjectReadPileup), c_size_t]),
    "GhostmSessionReadPileupArrays": (c_size_t, [c_void_p, c_int, u32p, u32p, POINTER(ctypes.c_uint8), u32p, c_size_t]),
    "GhostmSessionReadSubjectProfile": (c_size_t, [c_void_p, c_int, c_uint32, u32p, c_size_t]),
    "GhostmSessionReadPileupStats": (c_size_t, [c_void_p, POINTER(GhostmReadPileupStats), c_size_t]),
    "GhostmSessionReadCull": (c_size_t, [c_void_p, c_int, POINTER(GhostmCullOut), c_size_t]),
    "GhostmSessionSetCull": (c_int, [c_void_p, c_uint32, c_uint32]),
    "GhostmSessionSetTileGroups": (c_int, [c_void_p, c_int]),
    "GhostmSessionReadCullStats": (c_size_t, [c_void_p, POINTER(GhostmReadCullStats), c_size_t]),
    "GhostmSessionSetTaxonomy": (c_int, [c_void_p, c_uint32, u32p, u32p, c_size_t, u32p]),
    "GhostmSessionSetTaxonomyFiles": (c_int, [c_void_p, c_char_p, c_char_p]),
    "GhostmSessionTaxonomyInfo": (c_size_t, [c_void_p, POINTER(GhostmTaxonomyInfo), c_size_t]),
    "GhostmSessionSetLca": (c_int, [c_void_p, c_uint32, c_uint32]),
    "GhostmSessionReadLca": (c_size_t, [c_void_p, c_int, POINTER(GhostmLcaOut), c_size_t]),
    "GhostmSessionReadLcaBegin": (c_size_t, [c_void_p, c_int, u32p, c_size_t]),
    "GhostmSessionReadLcaStats": (c_size_t, [c_void_p, POINTER(GhostmReadLcaStats), c_size_t]),
    "GhostmSessionSetMates": (c_int, [c_void_p, c_int, c_uint32]),
    "GhostmSessionSetQueriesFastaMatesTiled": (c_int, [c_void_p, c_char_p, c_char_p, c_uint32, c_int, c_uint32,
                                                       c_uint32, c_uint32, POINTER(c_uint64)]),
    "GhostmSessionPairJoin": (c_size_t, [c_void_p, c_int, POINTER(GhostmLcaHit), u32p, c_size_t]),
    "GhostmSessionPairJoinPairs": (c_size_t, [c_void_p, c_int, POINTER(GhostmPairOut), u32p, u32p, c_size_t]),
    "GhostmSessionPairLca": (c_size_t, [c_void_p, c_int, POINTER(GhostmLcaOut), c_size_t]),
    "GhostmSessionPairJoinStats": (c_size_t, [c_void_p, POINTER(GhostmPairJoinStats), c_size_t]),
    "GhostmSessionSetProfile": (c_int, [c_void_p, c_uint32]),
    "GhostmSessionTaxonProfile": (c_size_t, [c_void_p, c_int, POINTER(GhostmTaxonCount), c_size_t]),
    "GhostmSessionTaxonProfileFinal": (c_size_t, [c_void_p, c_int, u32p, c_size_t]),
    "GhostmSessionTaxonProfileSummary": (c_size_t, [c_void_p, c_int, POINTER(GhostmTaxonSummary), c_size_t]),
    "GhostmSessionTaxonProfileStats": (c_size_t, [c_void_p, POINTER(GhostmTaxonProfileStats), c_size_t]),
    "GhostmSessionDeviceHits": (c_size_t, [c_void_p, c_void_p, c_size_t]),
    "GhostmSessionStats": (c_int, [c_void_p, POINTER(GhostmStats)]),
    "GhostmSessionStatsSized": (c_size_t, [c_void_p, POINTER(GhostmStats), c_size_t]),
    "GhostmStageStats": (c_size_t, [POINTER(GhostmStats), c_size_t]),
    "GhostmSessionDestroy": (None, [c_void_p]),
    "GhostmAlignMain": (c_int, [c_int, POINTER(c_char_p)]),
    "GhostmSearchMain": (c_int, [c_int, POINTER(c_char_p)]),
}

_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


def header_functions(path: str = HEADER_PATH) -> list[str]:
    """Function names declared in include/ghostm_hip.h."""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"\btypedef\b[^;]*;", "", text)  # function-pointer types are not exports
    names = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\(", text)
    skip = {"if", "defined", "sizeof"}
    out = []
    for n in names:
        if n in skip or n in out:
            continue
        out.append(n)
    return out


def load() -> ctypes.CDLL:
    """Load libghostm_hip.so (raises NativeLibraryMissing if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
        )
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def device_pool_info() -> tuple[int, int]:
    """(cached bytes, allocations retried after emptying the cache)."""
    cached, retries = c_uint64(0), c_uint64(0)
    load().GhostmDevicePoolInfo(ctypes.byref(cached), ctypes.byref(retries))
    return cached.value, retries.value


def last_error() -> str:
    return (load().GhostmGetLastError() or b"").decode(errors="replace")


def argv_array(args: list[str]):
    arr = (c_char_p * (len(args) + 1))()
    for i, a in enumerate(args):
        arr[i] = a.encode()
    arr[len(args)] = None
    return arr
