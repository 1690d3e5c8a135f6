// main.cpp — the `ghostm` command line (reference main.cpp:36-122): db | qry | aln,
// plus `synth` (synthetic benchmark inputs) and `search` (qry + aln for several
// FASTA files against one resident database, given as formatted files or, with
// -f, as FASTA formatted on the GPU). `aln` always runs on the GPU
// (-D selects the device, default 0). Errors are printed and the process exits 0
// like the reference; usage or an unknown command exits 1.
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>

#include "../../include/ghostm_hip.h"

namespace ghostm {
int DbFormatMain(int argc, char **argv);
int QueryFormatMain(int argc, char **argv);
int SynthMain(int argc, char **argv);
}  // namespace ghostm

static int Usage() {
  std::cerr << "ghostm (MI355X build of GHOSTM 2.0)\n"
            << "Command and Options\n"
            << "db:  ghostm db [-i dbFastaFile] [-o dbName] [-k kSize] [-l chunkSize]\n"
            << "qry: ghostm qry [-i qryFastaFile] [-o qryName] [-l maxLength] [-L chunkSize] [-t d|p]\n"
            << "aln: ghostm aln [-b best] [-D deviceId] [-l CandidatesSize] [-s skipSize]\n"
            << "       [-t threshold] [-r regionSize] [-e extendSize] [-G openGap] [-E extendGap]\n"
            << "       [-M scoreMatrix] [-y outputStyle] [-S startChunk] [-L endChunk] [-v]\n"
            << "       -i queries -d database -o output\n"
            << "       (-y 6: BLAST-tabular, the twelve -outfmt 6 columns; -y 12: the -y 7 columns from the\n"
            << "        read-level alignment of a read longer than one record; -y 14 and -y 15: the -y 12 and\n"
            << "        -y 13 lines with positives, qseq and sseq of the read-level alignment; -y 16 and -y 17: the\n"
            << "        -y 10 and -y 11 subject pile-up from the read-level alignments; -y 18 and -y 19: the same\n"
            << "        from the frameshift-aware alignments, with the subject's frameshift count)\n"
            << "search: ghostm search [aln options except -i -o -S -L] [-q d|p] [-w maxLength] [-c chunkSizeMB]\n"
            << "       (-d database | -f db.fasta [-k kSize] [-m chunkSizeMB]) q1.fasta out1 [q2.fasta out2 ...]\n"
            << "       (qry + aln per pair on one resident database; -q -w -c as qry's -t -l -L;\n"
            << "        -f: the database formatted on the GPU from FASTA, -k -m as db's -k -l)\n"
            << "       [-T tileStep [-X maxReadLength]]: reads longer than the record width searched as\n"
            << "        overlapping tiles tileStep letters apart, each read first cut at maxReadLength\n"
            << "       [-B band]: the half-width of -y 12 to 19's band around a hit's diagonal, 1..31 (default 31)\n"
            << "       [-F cost]: the frameshift cost of -y 13, 15, 18 and 19 (tiled DNA reads), 0 or more (default 15)\n"
            << "       [-g]: with -T, the best -b hits kept per tile and not per read (tile groups)\n"
            << "       [-K topK] [-C coverPct]: -y 20 and -y 21, the -y 12 and -y 13 lines of the hits the read-level\n"
            << "        cull keeps, per read by read-level score, with their rank and covered count; a hit is dropped\n"
            << "        when it repeats a kept alignment, or when topK (1..255, default 1) kept hits already cover\n"
            << "        coverPct (1..100, default 50) per cent of its stretch of the read\n"
            << "       [-n nodes.tsv -a map.tsv] [-p topPct] [-P supportPct]: -y 22 and -y 23, one line per read with\n"
            << "        hits: the taxon of the read from the hits the cull keeps (band paths, frame paths): qname taxid\n"
            << "        depth votes support lca_taxid candidates unmapped best_score. nodes.tsv: taxid, parent taxid per\n"
            << "        line (NCBI nodes.dmp reads as it is); map.tsv: subject name, taxid. A hit votes when its score is\n"
            << "        within topPct (0..100, default 10) per cent of the best on its stretch of the read; the taxon is\n"
            << "        the deepest node with supportPct (51..100, default 100) per cent of the votes\n"
            << "       [-R minReads]: -y 24 and -y 25 (with -n and -a), the sample's taxon profile from the -y 22 and\n"
            << "        -y 23 taxa: percent clade_reads kept_reads direct_reads depth taxid parent_taxid per line; first\n"
            << "        the unclassified reads (taxid 0), then the taxa with at least minReads (default 1) reads in their\n"
            << "        clade, depth first from the root, children by clade_reads; the reads of a smaller clade count\n"
            << "        for the first ancestor that has minReads\n"
            << "       [-Z window,trigger,extend]: low-complexity stretches of the reads masked with X before the search\n"
            << "        (SEG's raw segments; window 6..32, levels in hundredths of a bit, 0 <= trigger <= extend <= 500;\n"
            << "        e.g. -Z 12,220,250)\n"
            << "       [-Q trimQ,maskQ,minLen]: FASTQ reads (a file that begins with '@'; needs -T) trimmed at both ends by\n"
            << "        BWA's running sum at quality trimQ, kept letters below maskQ stored as N, reads left shorter than\n"
            << "        minLen emptied; 0..93, 0..93, 0..2^24 (e.g. -Q 20,0,30); read coordinates are of the kept stretch\n"
            << "       [-A SEQ1[,SEQ2]] [-O minOverlap,errPct[,pairOverlap]]: FASTQ reads cut at their 3' adapter before -Q:\n"
            << "        SEQ1 (SEQ2 for mate 2 of -j/-J; 1..64 letters of ACGTN) is looked for ungapped from each start,\n"
            << "        accepted with at least minOverlap letters (1..64, default 5) and at most errPct % mismatches\n"
            << "        (0..50, default 10); pairOverlap (with -j/-J; 0: off, 1..1024, 20 or more is sensible) also cuts\n"
            << "        both mates of a read-through pair at the end of their overlap, with or without -A\n"
            << "       [-j | -J] [-I maxInsert]: with -T, mate pairs. -j: records 2i and 2i + 1 of every input file are\n"
            << "        mates; -J: the positionals are triples r1.fasta r2.fasta out, interleaved record by record. A hit\n"
            << "        of each mate on one subject, at most maxInsert (default 1000; nt for DNA) apart and, for DNA, on\n"
            << "        opposite strands, joins into one candidate with the sum of the scores. -y 26 and -y 27 (with -n\n"
            << "        and -a): one line per pair with a hit, named by mate 1: the -y 22 columns of the pair, then mates\n"
            << "        (1: mate 1 has a hit, 2: mate 2, 3: both), joined, best_span; -y 24 and -y 25 count fragments\n"
            << "synth: ghostm synth -d db.fasta -q queries.fasta [-n nq] [-N dbResidues] [-s seed]\n";
  return 1;
}

int main(int argc, char **argv) {
  if (argc < 2) return Usage();
  const char *cmd = argv[1];
  try {
    const bool search = strcmp(cmd, "search") == 0;
    if (search || strcmp(cmd, "aln") == 0) {
      const int rc = search ? GhostmSearchMain(argc - 1, argv + 1) : GhostmAlignMain(argc - 1, argv + 1);
      if (search && rc != 0) return Usage();
      // the session is gone and its output file closed: leave without the HIP
      // runtime's teardown (tens of ms of a cold run; GHOSTM_FAST_EXIT=0 keeps it)
      std::cout.flush();
      std::cerr.flush();
      std::fflush(nullptr);
      const char *e = std::getenv("GHOSTM_FAST_EXIT");
      if (!(e && std::strcmp(e, "0") == 0)) _exit(rc);
      return rc;
    }
    if (strcmp(cmd, "db") == 0) { ghostm::DbFormatMain(argc - 1, argv + 1); return 0; }
    if (strcmp(cmd, "qry") == 0) { ghostm::QueryFormatMain(argc - 1, argv + 1); return 0; }
    if (strcmp(cmd, "synth") == 0) return ghostm::SynthMain(argc - 1, argv + 1);
  } catch (std::exception &e) {
    std::cerr << e.what() << std::endl;
    return 0;
  }
  std::cerr << "[main] unrecognized command " << cmd << std::endl;
  return 1;
}
