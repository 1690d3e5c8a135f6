"""ghostm_amd — MI355X (gfx950) build of the GHOSTM 2.0 `aln` hot path.

Seed lookup, Gotoh score DP and traceback are hand-written HIP kernels in
csrc/; the merge/E-value host logic and the C ABI live in libghostm_hip.so.
"""
from .aligner import (Aligner, GhostmError, HIT_DTYPE, HIT_EXT_DTYPE, HIT_PATH_DTYPE, HIT_ROWS_DTYPE,
                      SUBJECT_PILEUP_DTYPE, Session, cigar, consensus_text, db_chunk_cuts, format_db, format_queries, path_pileup_host,
                      path_rows_host, query_chunk_cuts, rows_of, run_cli, synth, traceback_ext_host,
                      traceback_path_host, QUERY_TILE_DTYPE, tile_plan, BAND_SOURCE_DTYPE, band_align_host,
                      band_align_gpu, stage_band_stats, HIT_FRAME_INFO_DTYPE, frame_align,
                      frame_align_host, frame_cigar, stage_frame_stats)
from .native import BIN_PATH, LIB_PATH, NativeLibraryMissing, load

__all__ = [
    "Aligner",
    "Session",
    "GhostmError",
    "HIT_DTYPE",
    "HIT_EXT_DTYPE",
    "HIT_PATH_DTYPE",
    "HIT_ROWS_DTYPE",
    "traceback_ext_host",
    "traceback_path_host",
    "cigar",
    "path_rows_host",
    "SUBJECT_PILEUP_DTYPE",
    "path_pileup_host",
    "consensus_text",
    "rows_of",
    "format_db",
    "format_queries",
    "query_chunk_cuts",
    "QUERY_TILE_DTYPE",
    "tile_plan",
    "BAND_SOURCE_DTYPE",
    "band_align_host",
    "band_align_gpu",
    "stage_band_stats",
    "HIT_FRAME_INFO_DTYPE",
    "frame_align",
    "frame_align_host",
    "frame_cigar",
    "stage_frame_stats",
    "db_chunk_cuts",
    "synth",
    "run_cli",
    "load",
    "LIB_PATH",
    "BIN_PATH",
    "NativeLibraryMissing",
]
