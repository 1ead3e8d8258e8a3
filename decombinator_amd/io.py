"""Arguments and writers of the `decombine` stage, with the names, defaults and file
formats of the reference's src/decombinator/io.py:

  create_args_dict        reference io.py:391-465 (same keys, same defaults)
  create_parser/cli_args  reference io.py:41-92, 95-383 (the common + decombine flags; the
                          collapse / translate flags as far as the front half of collapse and
                          the translate sub-command use them, the rest accepted so that existing
                          command lines parse)
  write_out_intermediate  reference io.py:480-513 (", "-joined rows, optional gzip, chmod 666)
"""
from __future__ import annotations

import argparse
import gzip
import os
import sys

from .decombine import __version__, sort_permissions


def create_args_dict(
    infile: str, chain: str, bc_read: str, suppresssummary: bool = False, dontgzip: bool = False,
    dontcheck: bool = False, dontcount: bool = False, extension: str = "n12", prefix: str = "dcr_",
    orientation: str = "reverse", tags: str = "extended", species: str = "human", allowNs: bool = False,
    lenthreshold: int = 130, tagfastadir: str = "Decombinator-Tags-FASTAs", nobarcoding: bool = False,
    bclength: int = 42, minbcQ: int = 20, bcQbelowmin: int = 1, avgQthreshold: int = 30,
    percentlevdist: int = 10, bcthreshold: int = 2, dontcheckinput: bool = False,
    barcodeduplication: bool = False, positionalbarcodes: bool = False, oligo: str = "M13",
    writeclusters: bool = False, UMIhistogram: bool = False, nonproductivefilter: bool = False,
    outpath: str = None, dontsave: bool = False, command: str = None, sampling_analysis: bool = False,
    cluster: bool = False, count_dcrs: bool = False, merge_errors: bool = False, merge_distance: int = 1,
    merge_ratio: int = 10, write_merges: bool = False, clonotypes: bool = False, cdr3_network: bool = False,
    cdr3_distance: int = 1, cdr3_class: str = "v", write_cdr3_edges: bool = False, cdr3_metric: str = None,
    cdr3_radius: int = None, cdr3_gap_cost: int = None, cdr3_trim: str = None, cdr3_cost_matrix: str = None,
) -> dict:
    """The function-argument dictionary threaded through the stages (the reference's 33 keys, `cluster`: run the
    grouping / clustering half of collapse, writing the `.freq`, and `count_dcrs`: with nobarcoding, count the DCRs on the
    GPU and write the `.nbc`; `merge_errors`: fold the counted DCRs within `merge_distance` substitutions of a DCR at least
    `merge_ratio` times as abundant into it before the `.nbc` is written, `write_merges`: list what was folded in a
    `.merges` file.  The defaults 1 and 10 are a design choice, not a measured optimum.  `clonotypes`: translate also groups the
    counted DCRs by (v_call, j_call, junction_aa) on the GPU and writes `<the .tsv's stem>.clonotypes.tsv`; `cdr3_network`:
    with clonotypes, link the clonotypes of one `cdr3_class` (none, v or vj) whose junction_aa have one length and differ in at
    most `cdr3_distance` (1 or 2) residues, on the GPU, and write `.cdr3_clusters.tsv`, with `write_cdr3_edges` also
    `.cdr3_edges.tsv`; `cdr3_metric` levenshtein (None: hamming) also links junction_aa of two lengths, at most
    `cdr3_distance` substitutions, insertions and deletions apart; `cdr3_metric` weighted links the junction_aa within
    `cdr3_radius` (None: 24) under match's weighted distance, with `cdr3_gap_cost` (12), `cdr3_trim` ("3,2") and
    `cdr3_cost_matrix` (a file; None: the default table) as `match` reads them, and `cdr3_distance` does not apply.  The defaults
    v and 1 are a design choice, not a measured optimum)."""
    return dict(
        infile=infile, chain=chain, bc_read=bc_read, suppresssummary=suppresssummary, dontgzip=dontgzip,
        dontcheck=dontcheck, dontcount=dontcount, extension=extension, prefix=prefix, orientation=orientation,
        tags=tags, species=species, allowNs=allowNs, lenthreshold=lenthreshold, tagfastadir=tagfastadir,
        nobarcoding=nobarcoding, bclength=bclength, minbcQ=minbcQ, bcQbelowmin=bcQbelowmin,
        avgQthreshold=avgQthreshold, percentlevdist=percentlevdist, bcthreshold=bcthreshold,
        dontcheckinput=dontcheckinput, barcodeduplication=barcodeduplication,
        positionalbarcodes=positionalbarcodes, oligo=oligo, writeclusters=writeclusters,
        UMIhistogram=UMIhistogram, nonproductivefilter=nonproductivefilter, outpath=outpath,
        dontsave=dontsave, command=command, sampling_analysis=sampling_analysis, cluster=cluster,
        count_dcrs=count_dcrs, merge_errors=merge_errors, merge_distance=merge_distance, merge_ratio=merge_ratio,
        write_merges=write_merges, clonotypes=clonotypes, cdr3_network=cdr3_network, cdr3_distance=cdr3_distance,
        cdr3_class=cdr3_class, write_cdr3_edges=write_cdr3_edges, cdr3_metric=cdr3_metric, cdr3_radius=cdr3_radius,
        cdr3_gap_cost=cdr3_gap_cost, cdr3_trim=cdr3_trim, cdr3_cost_matrix=cdr3_cost_matrix)


def _common(p: argparse.ArgumentParser):
    p.add_argument("-s", "--suppresssummary", action="store_true", help="Suppress the summary log")
    p.add_argument("-dz", "--dontgzip", action="store_true", help="Do not gzip the output files")
    p.add_argument("-dc", "--dontcount", action="store_true", help="Do not print the running count")
    p.add_argument("-op", "--outpath", type=str, default="", help="Output directory (default: cwd)")
    p.add_argument("-c", "--chain", type=str,
                   help="TCR chain (a/b/g/d); decombine and pipeline also take a comma-separated list (a,b or alpha,beta; g,d), "
                        "resolved in one pass over the FASTQ with the outputs each chain alone would give")
    p.add_argument("-pf", "--prefix", type=str, default="dcr_", help='Output file prefix. Default "dcr_"')
    p.add_argument("-ds", "--dontsave", action="store_true", help="Do not save output files")
    p.add_argument("-sa", "--sampling_analysis", action="store_true", help="Keep the R2 V-gene tail per row")


def _decombine(p: argparse.ArgumentParser):
    p.add_argument("-in", "--infile", type=str, required=True, help="FASTQ file with the TCR reads")
    p.add_argument("-br", "--bc_read", type=str, required=True, help="Which read holds the barcode (R1/R2)")
    p.add_argument("-dk", "--dontcheck", action="store_true", help="Skip the FASTQ check")
    p.add_argument("-ex", "--extension", type=str, default="n12", help='Output extension. Default "n12"')
    p.add_argument("-or", "--orientation", type=str, default="reverse", help="forward/reverse/both")
    p.add_argument("-tg", "--tags", type=str, default="extended", help="Tag set: extended or original")
    p.add_argument("-sp", "--species", type=str, default="human", help="human or mouse")
    p.add_argument("-N", "--allowNs", action="store_true", help="Allow rearrangements containing N")
    p.add_argument("-ln", "--lenthreshold", type=int, default=130, help="Inter-tag length threshold")
    p.add_argument("-tfdir", "--tagfastadir", type=str, default="Decombinator-Tags-FASTAs",
                   help="Folder with the tag and FASTA files")
    p.add_argument("-nbc", "--nobarcoding", action="store_true", help="Run without barcoding")
    p.add_argument("-bl", "--bclength", type=int, default=42, help="Barcode length. Default 42")


def _later_stage_flags(p: argparse.ArgumentParser):
    # collapse / translate flags of the reference (io.py:230-383): -ol, -mq, -bm, -aq steer the front half of collapse; the rest are parsed and carried
    p.add_argument("-mq", "--minbcQ", type=int, default=20)
    p.add_argument("-bm", "--bcQbelowmin", type=int, default=1)
    p.add_argument("-aq", "--avgQthreshold", type=int, default=30)
    p.add_argument("-lv", "--percentlevdist", type=int, default=10)
    p.add_argument("-bc", "--bcthreshold", type=int, default=2)
    p.add_argument("-di", "--dontcheckinput", action="store_true")
    p.add_argument("-bd", "--barcodeduplication", action="store_true")
    p.add_argument("-pb", "--positionalbarcodes", action="store_true")
    p.add_argument("-ol", "--oligo", type=str, default="M13")
    p.add_argument("-wc", "--writeclusters", action="store_true")
    p.add_argument("-uh", "--UMIhistogram", action="store_true")
    p.add_argument("-npf", "--nonproductivefilter", action="store_true")


def _cluster_flag(p: argparse.ArgumentParser):
    p.add_argument("--cluster", action="store_true",
                   help="Run the whole collapse stage: group reads by UMI, cluster UMIs (GPU neighbour search), count DCRs and "
                        "write the .freq (and the Collapsing_Summary.csv); without it only the per-row front half runs")


def _count_flag(p: argparse.ArgumentParser):
    p.add_argument("--count-dcrs", dest="count_dcrs", action="store_true",
                   help="With -nbc: count the distinct DCRs of a barcode-free run on the GPU and write them with their read "
                        "counts (.nbc: v, j, vdel, jdel, insert, count); translate reads such a file")


def _clonotypes_flag(p: argparse.ArgumentParser):
    p.add_argument("--clonotypes", action="store_true",
                   help="translate, pipeline --cluster / --count-dcrs: group the counted DCRs by V call, J call and CDR3 amino "
                        "acids on the GPU and write <the .tsv's stem>.clonotypes.tsv beside the .tsv (one row per clonotype: its "
                        "reads, its DCRs, its most abundant DCR)")
    p.add_argument("--cdr3-network", dest="cdr3_network", action="store_true",
                   help="With --clonotypes: link the clonotypes of one class (--cdr3-class) whose CDR3 amino acids have one length "
                        "and differ in at most --cdr3-distance residues, find the clusters they form (GPU) and write <the .tsv's "
                        "stem>.cdr3_clusters.tsv (one row per clonotype, in the order of the .clonotypes.tsv: its cluster, the "
                        "cluster's clonotypes and reads, its neighbours)")
    p.add_argument("--cdr3-distance", dest="cdr3_distance", type=int, default=None,
                   help="Residues in which two linked CDR3s may differ: 1 (default) or 2.  The default is a design choice, not a "
                        "measured optimum")
    # weighted (match's TCRdist-style distance with a radius; README) is taken with the four flags below it.  The help
    # texts of decombine, pipeline and translate are pinned word for word (tests/golden/overlap_help), so the metavar and the
    # help line stay what they were and the four flags are not listed; `match --help` describes them, the refusals name them,
    # and an unknown metric's error lists all three choices.
    p.add_argument("--cdr3-metric", dest="cdr3_metric", choices=["hamming", "levenshtein", "weighted"], default=None,
                   metavar="{hamming,levenshtein}",
                   help="How the residues between two linked CDR3s are counted: hamming (default; substitutions between CDR3s of "
                        "one length) or levenshtein (substitutions, insertions and deletions: the lengths may differ by up to "
                        "--cdr3-distance)")
    p.add_argument("--cdr3-radius", dest="cdr3_radius", type=int, default=None, help=argparse.SUPPRESS)           # 0 to 65535, default 24
    p.add_argument("--cdr3-gap-cost", dest="cdr3_gap_cost", type=int, default=None, help=argparse.SUPPRESS)       # 1 to 255, default 12
    p.add_argument("--cdr3-trim", dest="cdr3_trim", type=str, default=None, help=argparse.SUPPRESS)               # N,C, 0 to 16 each, default 3,2
    p.add_argument("--cdr3-cost-matrix", dest="cdr3_cost_matrix", type=str, default=None, help=argparse.SUPPRESS)  # a table as `match` reads it
    p.add_argument("--cdr3-class", dest="cdr3_class", choices=["none", "v", "vj"], default=None,
                   help="What two linked clonotypes must share beside the CDR3's length: nothing (none), the V call (v, the "
                        "default) or the V and the J call (vj).  The default is a design choice, not a measured optimum")
    p.add_argument("--write-cdr3-edges", dest="write_cdr3_edges", action="store_true",
                   help="With --cdr3-network: write <same stem>.cdr3_edges.tsv, one line per linked pair a < b (rows of the "
                        ".clonotypes.tsv, 0-based) with its distance")


def _merge_flags(p: argparse.ArgumentParser):
    p.add_argument("--merge-errors", dest="merge_errors", action="store_true",
                   help="With --count-dcrs: fold every DCR within --merge-distance substitutions (over the junction) of a DCR "
                        "with the same V, J and junction length and at least --merge-ratio times its reads into that DCR "
                        "before the .nbc is written (GPU)")
    p.add_argument("--merge-distance", dest="merge_distance", type=int, default=None,
                   help="Substitutions allowed between a DCR and its parent: 1 (default) or 2.  The default is a design choice, "
                        "not a measured optimum")
    p.add_argument("--merge-ratio", dest="merge_ratio", type=int, default=None,
                   help="A parent has at least this many times the reads of its child (integer >= 1; default 10, a design "
                        "choice, not a measured optimum)")
    p.add_argument("--write-merges", dest="write_merges", action="store_true",
                   help="With --merge-errors: write <same stem>.merges beside the .nbc, one line per folded DCR: its key, its "
                        "count, its root's key")


def _overlap(p: argparse.ArgumentParser):
    p.add_argument("-in", "--infile", type=str, nargs="+", required=True,
                   help="1 to 64 .clonotypes.tsv files (plain or .gz), one per sample; a sample is named by its file name "
                        "without .clonotypes.tsv[.gz]")
    p.add_argument("-op", "--outpath", type=str, default="", help="Output directory (default: cwd)")
    p.add_argument("-pf", "--prefix", type=str, default="dcr_", help='Output file prefix. Default "dcr_"')
    p.add_argument("-dz", "--dontgzip", action="store_true", help="Do not gzip the output files")
    p.add_argument("--overlap-key", dest="overlap_key", choices=["vj", "v", "none"], default="vj",
                   help="What two rows must share beside the CDR3 amino acids to be one clonotype: the V and the J call (vj, "
                        "the default), the V call (v) or nothing (none)")
    p.add_argument("--min-samples", dest="min_samples", type=int, default=2,
                   help="A clonotype is written to overlap_public.tsv when at least this many samples hold it (1 .. the number "
                        "of files; default 2)")
    p.add_argument("--downsample", dest="downsample", type=str, default=None, metavar="N|min",
                   help="Subsample every sample's reads without replacement to one depth before anything is compared (GPU): N "
                        "reads (1 or more), or min for the reads of the smallest sample that has any.  A sample with fewer reads "
                        "is kept whole")
    p.add_argument("--seed", dest="seed", type=int, default=None,
                   help="The seed of --downsample's subsample, 0 .. 2^64 - 1 (default 1); the same seed gives the same files")
    p.add_argument("--diversity", dest="diversity", action="store_true",
                   help="Also write overlap_diversity.tsv: per sample its reads, clonotypes, singletons, doubletons, largest "
                        "clonotype, D50, Chao1, Simpson, inverse Simpson, Gini, Shannon entropy and clonality")


def _match(p: argparse.ArgumentParser):
    p.add_argument("-in", "--infile", type=str, nargs="+", required=True,
                   help="1 to 64 .clonotypes.tsv files (plain or .gz), one per sample; a sample is named by its file name "
                        "without .clonotypes.tsv[.gz]")
    p.add_argument("-db", "--database", type=str, required=True,
                   help="The database: a tab-separated table (plain or .gz) with a header line, its columns found by name; a "
                        ".clonotypes.tsv is one as it stands")
    p.add_argument("-op", "--outpath", type=str, default="", help="Output directory (default: cwd)")
    p.add_argument("-pf", "--prefix", type=str, default="dcr_", help='Output file prefix. Default "dcr_"')
    p.add_argument("-dz", "--dontgzip", action="store_true", help="Do not gzip the output files")
    p.add_argument("--cdr3-distance", dest="cdr3_distance", type=int, default=1,
                   help="Residues in which a clonotype's CDR3 and a database entry's may differ: 0, 1 (default) or 2.  The default "
                        "is a design choice, not a measured optimum")
    p.add_argument("--cdr3-metric", dest="cdr3_metric", choices=["hamming", "levenshtein", "weighted"], default="hamming",
                   help="How those residues are counted: hamming (default; substitutions between CDR3s of one length), "
                        "levenshtein (substitutions, insertions and deletions) or weighted (a TCRdist-style distance with a "
                        "radius: a substitution costs what --cdr3-cost-matrix says, a length difference is one gap of "
                        "--cdr3-gap-cost per position, the ends given by --cdr3-trim do not count, and a hit lies within "
                        "--cdr3-radius; --cdr3-distance does not apply; CDR3s with a byte outside A..Z take no part)")
    p.add_argument("--cdr3-radius", dest="cdr3_radius", type=int, default=None,
                   help="With --cdr3-metric weighted: the largest weighted distance of a hit, 0 to 65535 (default 24: two radical "
                        "substitutions, or one gapped position and one radical substitution).  The defaults 24, 12 and 3,2 "
                        "follow TCRdist's CDR3 settings: a design choice, not a measured optimum")
    p.add_argument("--cdr3-gap-cost", dest="cdr3_gap_cost", type=int, default=None,
                   help="With --cdr3-metric weighted: the price of one gapped position, 1 to 255 (default 12)")
    p.add_argument("--cdr3-trim", dest="cdr3_trim", type=str, default=None,
                   help="With --cdr3-metric weighted: N,C - the first N and the last C residues of the shorter CDR3 do not count, "
                        "0 to 16 each (default 3,2)")
    p.add_argument("--cdr3-cost-matrix", dest="cdr3_cost_matrix", type=str, default=None,
                   help="With --cdr3-metric weighted: a tab-separated square table of substitution costs 0..255 (first row and "
                        "first column: single letters; symmetric, zero diagonal, covering the twenty amino acids).  Default: "
                        "3 * min(4, 4 - BLOSUM62), as TCRdist's")
    p.add_argument("--cdr3-class", dest="cdr3_class", choices=["none", "v", "vj"], default="v",
                   help="What a clonotype and a database entry must share beside the CDR3: nothing (none), the V call (v, the "
                        "default) or the V and the J call (vj).  The default is the network's: a design choice, not a measured "
                        "optimum")
    p.add_argument("--strip-alleles", dest="strip_alleles", action="store_true",
                   help="Compare a call up to its first * on both sides (TRBV7-9*01 and TRBV7-9*03 are then one V)")
    p.add_argument("--db-cdr3-column", dest="db_cdr3_column", type=str, default="junction_aa",
                   help="The database column that holds the CDR3 amino acids (default junction_aa; a VDJdb export: CDR3)")
    p.add_argument("--db-v-column", dest="db_v_column", type=str, default="v_call",
                   help="The database column that holds the V call (default v_call; a VDJdb export: V); read when the class needs it")
    p.add_argument("--db-j-column", dest="db_j_column", type=str, default="j_call",
                   help="The database column that holds the J call (default j_call; a VDJdb export: J); read when the class needs it")


def _motifs(p: argparse.ArgumentParser):
    p.add_argument("-in", "--infile", type=str, nargs="+", required=True,
                   help="1 to 64 .clonotypes.tsv files (plain or .gz), one per sample; a sample is named by its file name "
                        "without .clonotypes.tsv[.gz]")
    p.add_argument("-bg", "--background", type=str, required=True,
                   help="The background repertoire: a tab-separated table (plain or .gz) with a header line, its CDR3 column found "
                        "by name; another sample's .clonotypes.tsv is one as it stands")
    p.add_argument("-op", "--outpath", type=str, default="", help="Output directory (default: cwd)")
    p.add_argument("-pf", "--prefix", type=str, default="dcr_", help='Output file prefix. Default "dcr_"')
    p.add_argument("-dz", "--dontgzip", action="store_true", help="Do not gzip the output files")
    p.add_argument("--bg-cdr3-column", dest="bg_cdr3_column", type=str, default="junction_aa",
                   help="The background column that holds the CDR3 amino acids (default junction_aa)")
    p.add_argument("--motif-k", dest="motif_k", type=str, default=None,
                   help="The motif lengths, a comma-separated list out of 2, 3, 4 (default 2,3,4)")
    p.add_argument("--motif-trim", dest="motif_trim", type=str, default=None,
                   help="N,C - the first N and the last C residues of a CDR3 hold no motif, 0 to 16 each (default 3,3, after "
                        "GLIPH: a design choice, not a measured optimum)")
    p.add_argument("--motif-min-count", dest="motif_min_count", type=int, default=None,
                   help="A motif is reported when at least this many of the sample's distinct CDR3s hold it (1 or more; default 3, "
                        "a design choice)")
    p.add_argument("--resamples", dest="resamples", type=int, default=None,
                   help="How many times as many background CDR3s as the sample has are drawn without replacement (GPU), 0 to "
                        "65535 (default 1000); 0 gives the counts alone")
    p.add_argument("--seed", dest="seed", type=int, default=None,
                   help="The seed of the draws, 0 .. 2^64 - 1 (default 1); the same seed gives the same files")
    p.add_argument("--groups", dest="groups", action="store_true",
                   help="Also merge each sample's CDR3s into specificity groups (GPU): CDR3s that share a selected motif or lie "
                        "within --group-distance residues of each other are linked, and a group is a connected component; writes "
                        "<sample>.cdr3_groups.tsv (needs --resamples above 0)")
    p.add_argument("--group-p-value", dest="group_p_value", type=str, default=None,
                   help="--groups: a motif is selected when its p_value is at most this decimal, above 0 and at most 1 (default "
                        "0.001, after GLIPH: a design choice, not a measured optimum)")
    p.add_argument("--group-min-fold", dest="group_min_fold", type=str, default=None,
                   help="--groups: ... and its fold is at least this decimal, 0 or more (default 10, after GLIPH: a design choice)")
    p.add_argument("--group-distance", dest="group_distance", type=int, default=None,
                   help="--groups: CDR3s of one length that differ in at most this many residues are linked, 0, 1 or 2 (default 1, "
                        "after GLIPH: a design choice; 0: no such links)")
    p.add_argument("--write-motif-members", dest="write_motif_members", action="store_true",
                   help="--groups: also write <sample>.cdr3_motif_members.tsv, the CDR3s that hold each selected motif")


def _metaclonotypes(p: argparse.ArgumentParser):
    p.add_argument("-in", "--infile", type=str, nargs="+", required=True,
                   help="1 to 64 .clonotypes.tsv files (plain or .gz), one per sample; a sample is named by its file name "
                        "without .clonotypes.tsv[.gz]")
    p.add_argument("-bg", "--background", type=str, default=None,
                   help="The background repertoire (required): a tab-separated table (plain or .gz) with a header line, its "
                        "columns found by name; another sample's .clonotypes.tsv is one as it stands")
    p.add_argument("-op", "--outpath", type=str, default="", help="Output directory (default: cwd)")
    p.add_argument("-pf", "--prefix", type=str, default="dcr_", help='Output file prefix. Default "dcr_"')
    p.add_argument("-dz", "--dontgzip", action="store_true", help="Do not gzip the output files")
    p.add_argument("--cdr3-radius", dest="cdr3_radius", type=int, default=None,
                   help="The top of the ladder of radii, a multiple of --radius-step with at most 32 rungs (radius / step + 1), "
                        "0 to 65535 (default 48).  Radius 48, step 2, rate 1e-5 and class v follow tcrdist3's usage: design "
                        "choices, not measured optima")
    p.add_argument("--radius-step", dest="radius_step", type=int, default=None,
                   help="The distance between two radii of the ladder, 1 to 65535 (default 2)")
    p.add_argument("--max-background-rate", dest="max_background_rate", type=str, default=None,
                   help="A clonotype's radius is the largest of the ladder at which at most this share of the background's CDR3s "
                        "lies within it: a decimal or a fraction, 0 to 1, read exactly (1e-5 and 1/100000 are the same; default "
                        "1e-5)")
    p.add_argument("--cdr3-class", dest="cdr3_class", choices=["none", "v", "vj"], default="v",
                   help="What two CDR3s must share to be compared: nothing (none), the V call (v, the default) or the V and the "
                        "J call (vj)")
    p.add_argument("--strip-alleles", dest="strip_alleles", action="store_true",
                   help="Compare a call up to its first * on both sides (TRBV7-9*01 and TRBV7-9*03 are then one V)")
    p.add_argument("--cdr3-gap-cost", dest="cdr3_gap_cost", type=int, default=None,
                   help="The price of one gapped position, 1 to 255 (default 12)")
    p.add_argument("--cdr3-trim", dest="cdr3_trim", type=str, default=None,
                   help="N,C - the first N and the last C residues of the shorter CDR3 do not count, 0 to 16 each (default 3,2)")
    p.add_argument("--cdr3-cost-matrix", dest="cdr3_cost_matrix", type=str, default=None,
                   help="A tab-separated square table of substitution costs 0..255, as `match --cdr3-cost-matrix` takes it.  "
                        "Default: 3 * min(4, 4 - BLOSUM62), as TCRdist's")
    p.add_argument("--bg-cdr3-column", dest="bg_cdr3_column", type=str, default="junction_aa",
                   help="The background column that holds the CDR3 amino acids (default junction_aa)")
    p.add_argument("--bg-v-column", dest="bg_v_column", type=str, default="v_call",
                   help="The background column that holds the V call (default v_call); read when the class needs it")
    p.add_argument("--bg-j-column", dest="bg_j_column", type=str, default="j_call",
                   help="The background column that holds the J call (default j_call); read when the class needs it")
    p.add_argument("--write-radius-profile", dest="write_radius_profile", action="store_true",
                   help="Also write <sample>.cdr3_radius_profile.tsv: per clonotype the background's and the sample's CDR3s within "
                        "every radius of the ladder (cumulative)")
    p.add_argument("--write-metaclonotype-members", dest="write_metaclonotype_members", action="store_true",
                   help="Also write <sample>.cdr3_metaclonotype_members.tsv: per clonotype the sample's other clonotypes within "
                        "its radius, with their distances")


def _tabulate(p: argparse.ArgumentParser):
    p.add_argument("-in", "--infile", type=str, nargs="+", required=True,
                   help="1 to 64 .clonotypes.tsv files (plain or .gz), one per bulk sample; a sample is named by its file name "
                        "without .clonotypes.tsv[.gz]")
    p.add_argument("-mc", "--metaclonotypes", type=str, default=None,
                   help="The meta-clonotypes (required): a tab-separated table (plain or .gz) with a header line, its columns found "
                        "by name; a .cdr3_metaclonotypes.tsv of `metaclonotypes` is one as it stands.  A row whose radius is `.` is "
                        "left out")
    p.add_argument("-op", "--outpath", type=str, default="", help="Output directory (default: cwd)")
    p.add_argument("-pf", "--prefix", type=str, default="dcr_", help='Output file prefix. Default "dcr_"')
    p.add_argument("-dz", "--dontgzip", action="store_true", help="Do not gzip the output files")
    p.add_argument("--mc-cdr3-column", dest="mc_cdr3_column", type=str, default="junction_aa",
                   help="The -mc column that holds the centroid's CDR3 amino acids (default junction_aa)")
    p.add_argument("--mc-v-column", dest="mc_v_column", type=str, default="v_call",
                   help="The -mc column that holds the V call (default v_call); read when the class needs it")
    p.add_argument("--mc-j-column", dest="mc_j_column", type=str, default="j_call",
                   help="The -mc column that holds the J call (default j_call); read when the class needs it")
    p.add_argument("--mc-radius-column", dest="mc_radius_column", type=str, default="radius",
                   help="The -mc column that holds the radius, an integer 0 to 65535 or `.` (default radius)")
    p.add_argument("--cdr3-class", dest="cdr3_class", choices=["none", "v", "vj"], default="v",
                   help="What a clonotype and a centroid must share to be compared: nothing (none), the V call (v, the default) or "
                        "the V and the J call (vj).  The class, --strip-alleles and the three cost flags have to be the ones the "
                        "meta-clonotypes were made under")
    p.add_argument("--strip-alleles", dest="strip_alleles", action="store_true",
                   help="Compare a call up to its first * on both sides (TRBV7-9*01 and TRBV7-9*03 are then one V)")
    p.add_argument("--cdr3-gap-cost", dest="cdr3_gap_cost", type=int, default=None,
                   help="The price of one gapped position, 1 to 255 (default 12)")
    p.add_argument("--cdr3-trim", dest="cdr3_trim", type=str, default=None,
                   help="N,C - the first N and the last C residues of the shorter CDR3 do not count, 0 to 16 each (default 3,2)")
    p.add_argument("--cdr3-cost-matrix", dest="cdr3_cost_matrix", type=str, default=None,
                   help="A tab-separated square table of substitution costs 0..255, as `match --cdr3-cost-matrix` takes it.  "
                        "Default: 3 * min(4, 4 - BLOSUM62), as TCRdist's")


def _associate(p: argparse.ArgumentParser):
    p.add_argument("-in", "--infile", type=str, nargs="+", default=None,
                   help="The feature by sample table (required), plain or .gz, recognised by its header: a tabulate.tsv of "
                        "`tabulate` or an overlap_public.tsv of `overlap`.  Several tabulate.tsv — the runs of `tabulate` over one "
                        "-mc file, 64 samples each — are joined side by side: same meta-clonotypes in the same order, no sample "
                        "twice; 2 to 1024 samples with a group take part in all")
    p.add_argument("-ph", "--phenotype", type=str, default=None,
                   help="The cohort (required): a tab-separated table (plain or .gz) with a header line, its sample and group "
                        "columns found by name.  A group of `.` or nothing means unknown: the sample is left out")
    p.add_argument("--case", dest="case", type=str, default=None,
                   help="The label of the cases (required): one of the two labels of the group column")
    p.add_argument("-op", "--outpath", type=str, default="", help="Output directory (default: cwd)")
    p.add_argument("-pf", "--prefix", type=str, default="dcr_", help='Output file prefix. Default "dcr_"')
    p.add_argument("-dz", "--dontgzip", action="store_true", help="Do not gzip the output files")
    p.add_argument("--ph-sample-column", dest="ph_sample_column", type=str, default="sample",
                   help="The -ph column that holds the sample names, as -in's columns name them (default sample)")
    p.add_argument("--ph-group-column", dest="ph_group_column", type=str, default="group",
                   help="The -ph column that holds the group labels (default group)")
    p.add_argument("--value", dest="value", choices=["clonotypes", "reads"], default=None,
                   help="Which of a tabulate.tsv's two numbers per sample decides presence (default clonotypes); an "
                        "overlap_public.tsv holds reads only")
    p.add_argument("--min-count", dest="min_count", type=int, default=None,
                   help="A feature is present in a sample when its value is at least this, 1 or more (default 1).  The test is on "
                        "presence, not abundance")
    p.add_argument("--alternative", dest="alternative", choices=["greater", "less", "two-sided"], default=None,
                   help="The exact test's alternative: present in MORE cases than chance (greater, the default, as Emerson et al. "
                        "2017), in fewer (less), or either (two-sided: the tables no likelier than the observed one)")
    p.add_argument("--permutations", dest="permutations", type=int, default=None,
                   help="Relabelings of the samples the null is made of, 0 to 1048576 (default 10000; 0: p-values only, no GPU).  "
                        "greater, 10000 and 0.05 are design choices after Emerson et al., not measured optima")
    p.add_argument("--seed", dest="seed", type=int, default=None,
                   help="The seed of the relabelings, 0 to 2^64 - 1 (default 1): one seed, one set of files")
    p.add_argument("--max-p", dest="max_p", type=str, default=None,
                   help="The p-values up to this one form the tail the false discovery rate is estimated on: a decimal or a "
                        "fraction, 0 to 1, read exactly (0.05 and 1/20 are the same; default 0.05)")
    p.add_argument("--write-null", dest="write_null", action="store_true",
                   help="Also write associate_null.tsv: per p-value of the tail the features, the null's pairs and the false "
                        "discovery rate")
    p.add_argument("--test", dest="test", choices=["fisher", "rank-sum"], default=None,
                   help="The test per feature: fisher (the default), the exact test on presence above; or rank-sum, a Wilcoxon / "
                        "Mann-Whitney rank sum on the VALUES — ties share the mid-rank, values below --min-count count as 0 — with "
                        "Westfall and Young's max-T over the relabelings for the adjusted p-values; 2 to 64 samples; --max-p is "
                        "refused there")
    p.add_argument("--depths", dest="depths", type=str, default=None,
                   help="Only with --test rank-sum: a tab-separated table with a `sample` column and one named as --value "
                        "(tabulate_samples.tsv fits as it stands); samples are then ranked by value over depth, compared exactly "
                        "in integers.  Without it raw values are ranked, and a printed line says so")


def create_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        prog="decombinator",
        description="Decombinator `decombine` stage on MI355X (HIP), the per-row front half of `collapse` and `translate` (CDR3 per DCR).  "
                    "Sub-commands as in the reference; the grouping / clustering half of `collapse` (UMI clustering, the "
                    ".freq) runs with --cluster.")
    parser.add_argument("-v", "--version", action="version", version=__version__)
    parser.epilog = ("Further commands have parsers of their own: `match` (clonotypes near a database's CDR3s, GPU), `motifs` "
                     "(CDR3 k-mers enriched against a background, GPU), `metaclonotypes` (per clonotype the largest CDR3 radius "
                     "a background still stays out of, GPU) and `tabulate` (meta-clonotypes counted in bulk samples, GPU); see "
                     "`python -m decombinator_amd match --help`, `python -m decombinator_amd motifs --help`, "
                     "`python -m decombinator_amd metaclonotypes --help` and `python -m decombinator_amd tabulate --help`.  "
                     "`associate` (exact tests over a tabulate.tsv or an overlap_public.tsv with a permutation null, GPU) has one "
                     "too: `python -m decombinator_amd associate --help`.")
    sub = parser.add_subparsers(dest="command", help="Available commands")
    sub.required = False
    pipe = sub.add_parser("pipeline", help="decombine, then the front half of collapse; with --cluster the whole of collapse and "
                                           "translate (.n12, .freq, .tsv)")
    _common(pipe); _decombine(pipe); _later_stage_flags(pipe); _cluster_flag(pipe); _count_flag(pipe); _merge_flags(pipe); _clonotypes_flag(pipe)
    dec = sub.add_parser("decombine", help="Decombine TCR reads")
    _common(dec); _decombine(dec); _count_flag(dec); _merge_flags(dec); _clonotypes_flag(dec)
    col = sub.add_parser("collapse", help="front half of collapse over an .n12 file: barcode extraction and the row filters "
                                          "(writes .n12u); with --cluster the whole stage (writes .freq)")
    _common(col); _later_stage_flags(col); _cluster_flag(col); _count_flag(col); _clonotypes_flag(col)
    col.add_argument("-in", "--infile", type=str, required=True, help=".n12 file of the decombine stage (optionally gzipped)")
    col.add_argument("-N", "--allowNs", action="store_true", help="Allow barcodes containing N")
    col.add_argument("-ln", "--lenthreshold", type=int, default=130, help="Inter-tag length threshold")
    tr = sub.add_parser("translate", help="CDR3 extraction (translate.get_cdr3) for the DCRs of a .freq file; writes the AIRR .tsv")
    _common(tr); _later_stage_flags(tr)
    tr.add_argument("-in", "--infile", type=str, required=True, help=".freq file (v,j,vdel,jdel,insert,frequency,cluster size per line)")
    tr.add_argument("-tg", "--tags", type=str, default="extended")
    tr.add_argument("-sp", "--species", type=str, default="human")
    tr.add_argument("-tfdir", "--tagfastadir", type=str, default="Decombinator-Tags-FASTAs")
    tr.add_argument("-nbc", "--nobarcoding", action="store_true")
    _count_flag(tr); _clonotypes_flag(tr)
    ov = sub.add_parser("overlap", help="clonotype sharing between samples (GPU): per pair of .clonotypes.tsv files what they "
                                        "share (overlap_pairs.tsv), and the clonotypes several samples hold (overlap_public.tsv)")
    _overlap(ov)
    return parser


def create_match_parser() -> argparse.ArgumentParser:
    """The parser of `match`, a sub-command with a parser of its own: cli_args hands it what follows the word `match` (the
    list of create_parser()'s sub-commands stays what it was; its epilog names this one)."""
    parser = argparse.ArgumentParser(
        prog="python -m decombinator_amd match",
        description="Near matches between samples and a database (GPU): which clonotypes of .clonotypes.tsv files are the same "
                    "as, or one or two CDR3 residues from, an entry of a second table (a list of CDR3s of known specificity, or "
                    "another sample's .clonotypes.tsv); writes <sample>.cdr3_matches.tsv per sample and match_targets.tsv.")
    _match(parser)
    return parser


def create_motifs_parser() -> argparse.ArgumentParser:
    """The parser of `motifs`, a sub-command with a parser of its own, as `match` is."""
    parser = argparse.ArgumentParser(
        prog="python -m decombinator_amd motifs",
        description="CDR3 motif enrichment against a background (GPU): which 2-, 3- and 4-mers in the middle of the CDR3s of "
                    ".clonotypes.tsv files occur in more of a sample's distinct CDR3s than in as many CDR3s drawn from a "
                    "background repertoire; writes <sample>.cdr3_motifs.tsv per sample.  With --groups also the specificity groups "
                    "the enriched motifs and near-identical CDR3s join the sample's CDR3s into.")
    _motifs(parser)
    return parser


def create_metaclonotypes_parser() -> argparse.ArgumentParser:
    """The parser of `metaclonotypes`, a sub-command with a parser of its own, as `match` and `motifs` are."""
    parser = argparse.ArgumentParser(
        prog="python -m decombinator_amd metaclonotypes",
        description="Meta-clonotypes (GPU): per clonotype of .clonotypes.tsv files the largest radius of a TCRdist-style CDR3 "
                    "distance within which a background repertoire almost never falls, and how many of the sample's own "
                    "clonotypes fall inside it; writes <sample>.cdr3_metaclonotypes.tsv per sample.")
    _metaclonotypes(parser)
    return parser


def create_tabulate_parser() -> argparse.ArgumentParser:
    """The parser of `tabulate`, a sub-command with a parser of its own, as `match`, `motifs` and `metaclonotypes` are."""
    parser = argparse.ArgumentParser(
        prog="python -m decombinator_amd tabulate",
        description="Bulk tabulation of meta-clonotypes (GPU): per meta-clonotype (centroid CDR3, class, radius — as "
                    "`metaclonotypes` writes them) and per .clonotypes.tsv file, how many clonotypes and reads fall inside the "
                    "meta-clonotype's own radius of a TCRdist-style CDR3 distance; writes tabulate.tsv and tabulate_samples.tsv.")
    _tabulate(parser)
    return parser


def create_associate_parser() -> argparse.ArgumentParser:
    """The parser of `associate`, a sub-command with a parser of its own, as `match`, `motifs`, `metaclonotypes` and `tabulate`
    are."""
    parser = argparse.ArgumentParser(
        prog="python -m decombinator_amd associate",
        description="Association of features with a phenotype (GPU): per meta-clonotype of a tabulate.tsv, or public clonotype of "
                    "an overlap_public.tsv, an exact test of its presence in the cases against the controls of a cohort, and a "
                    "label-permutation null over all features for the adjusted p-values and the false discovery rate; writes "
                    "associate.tsv and, on demand, associate_null.tsv.  With --test rank-sum the question is abundance: a rank sum "
                    "of the feature's values in the cases against the controls, standardized in fixed point, with a max-T null over "
                    "the same relabelings; associate.tsv then holds mean ranks, z, the score, the feature's own permutation p-value, "
                    "the max-T adjusted p-value and a q-value over the largest observed scores.")
    _associate(parser)
    return parser


def cli_args(argv=None) -> dict:
    words = sys.argv[1:] if argv is None else list(argv)
    if words and words[0] == "associate":
        return dict(vars(create_associate_parser().parse_args(words[1:])), command="associate")
    if words and words[0] == "tabulate":
        return dict(vars(create_tabulate_parser().parse_args(words[1:])), command="tabulate")
    if words and words[0] == "metaclonotypes":
        return dict(vars(create_metaclonotypes_parser().parse_args(words[1:])), command="metaclonotypes")
    if words and words[0] == "match":
        return dict(vars(create_match_parser().parse_args(words[1:])), command="match")
    if words and words[0] == "motifs":
        return dict(vars(create_motifs_parser().parse_args(words[1:])), command="motifs")
    inp = vars(create_parser().parse_args(argv))
    if "merge_errors" in inp:
        # which of the merge options the command line named (they are refused without --merge-errors), then the defaults
        inp["merge_options_given"] = [f for f, k in (("--merge-distance", "merge_distance"), ("--merge-ratio", "merge_ratio"))
                                      if inp[k] is not None]
        inp["merge_distance"] = 1 if inp["merge_distance"] is None else inp["merge_distance"]
        inp["merge_ratio"] = 10 if inp["merge_ratio"] is None else inp["merge_ratio"]
    if "cdr3_network" in inp:
        # which of the network's options the command line named (they are refused without --cdr3-network), then the defaults
        inp["cdr3_options_given"] = [f for f, k in (("--cdr3-distance", "cdr3_distance"), ("--cdr3-class", "cdr3_class"),
                                                    ("--cdr3-metric", "cdr3_metric"), ("--cdr3-radius", "cdr3_radius"),
                                                    ("--cdr3-gap-cost", "cdr3_gap_cost"), ("--cdr3-trim", "cdr3_trim"),
                                                    ("--cdr3-cost-matrix", "cdr3_cost_matrix")) if inp[k] is not None]
        inp["cdr3_distance"] = 1 if inp["cdr3_distance"] is None else inp["cdr3_distance"]
        inp["cdr3_class"] = "v" if inp["cdr3_class"] is None else inp["cdr3_class"]
    return inp


class _GzText:
    """What write_text / write need of a text file object, in front of a GzipWriter: str is buffered and encoded as the
    reference's text-mode file does (UTF-8, "\n" kept), bytes go through `buffer` as they are."""

    def __init__(self, gz):
        self._gz, self._pending, self._n = gz, [], 0
        self.buffer = self

    def write(self, x):
        if isinstance(x, str):
            x = x.encode("utf-8")
            self._pending.append(x)
            self._n += len(x)
            if self._n >= (8 << 20):
                self.flush()
        else:
            self.flush()
            self._gz.write(x)

    def flush(self):
        if self._pending:
            self._gz.write(b"".join(self._pending))
            self._pending, self._n = [], 0


def write_out_intermediate(data: list, inputargs: dict, suffix: str):
    """`<outpath><prefix><file id>_<chain name><suffix>`: one row per line, fields joined by
    ", "; gzipped unless dontgzip; mode 666 (reference io.py:480-513)."""
    chainnams = {"a": "alpha", "b": "beta", "g": "gamma", "d": "delta"}
    filename_id = os.path.basename(inputargs["infile"]).split(".")[0]
    if inputargs["command"] in ["collapse", "translate"]:
        outfilename = inputargs["outpath"] + f"{filename_id}" + suffix
    else:
        outfilename = (inputargs["outpath"] + inputargs["prefix"] + f"{filename_id}"
                       + f"_{chainnams[inputargs['chain'].lower()]}" + suffix)
    if not inputargs["dontgzip"]:
        # the reference writes the text, re-reads it through gzip.open (one thread, level 9) and unlinks it; what is left
        # is the .gz, written here at once by libdcrx's threaded gzip writer (same decompressed bytes)
        from . import _native as nat
        print("Compressing intermediate output file to", outfilename + ".gz")
        with nat.GzipWriter(outfilename + ".gz", level=int(os.environ.get("DCRX_GZIP_LEVEL", "6"))) as gz:
            out = _GzText(gz)
            if hasattr(data, "write_text"):      # decombine.N12Rows: the rows are text already
                data.write_text(out, ", ")
            else:
                for line in data:
                    out.write(", ".join(map(str, line)) + "\n")
            out.flush()
        outfilename += ".gz"
    else:
        with open(outfilename, "w") as outfile:
            if hasattr(data, "write_text"):
                data.write_text(outfile, ", ")
            else:
                for line in data:
                    outfile.write(", ".join(map(str, line)) + "\n")
    sort_permissions(outfilename)
    return outfilename


class _RawText:
    """Text that is bytes already, for write_out_intermediate."""

    def __init__(self, text: bytes):
        self.text = text

    def write_text(self, fh, joiner: str = ", ") -> None:
        fh.flush()
        fh.buffer.write(self.text)


def write_out_counts(data, inputargs: dict):
    """The `.nbc` of the barcode-free count and, with write_merges, `<same stem>.merges` beside it (what --merge-errors
    folded: decombine.merges_text).  Returns the `.nbc`'s name."""
    name = write_out_intermediate(data, inputargs, nbc_suffix(inputargs))
    if inputargs.get("write_merges") and hasattr(data, "merges_text"):
        write_out_intermediate(_RawText(data.merges_text), inputargs, ".merges")
    return name


def nbc_suffix(inputargs: dict) -> str:
    """The suffix of the barcode-free count's file: `.nbc` while the extension is the default n12 (the reference's own
    message, decombine.py:1054-1057), `.<extension>` otherwise."""
    return ".nbc" if inputargs["extension"] == "n12" else "." + inputargs["extension"]


def _translated_stem(inputargs: dict) -> str:
    """The `.tsv`'s name without its suffix (write_out_translated's naming rules)."""
    chainnams = {"a": "alpha", "b": "beta", "g": "gamma", "d": "delta"}
    filename_id = os.path.basename(inputargs["infile"]).split(".")[0]
    if inputargs["command"] in ["collapse", "translate"]:
        return inputargs["outpath"] + f"{filename_id}"
    return inputargs["outpath"] + inputargs["prefix"] + f"{filename_id}" + f"_{chainnams[inputargs['chain'].lower()]}"


def write_out_clonotypes(clonotypes, inputargs: dict):
    """The clonotype table of --clonotypes beside the `.tsv`: `<the .tsv's stem>.clonotypes.tsv`, tab separated with a header
    line, gzipped unless dontgzip, mode 666 (the rules of write_out_translated).  `clonotypes`: translate.ClonotypeTable (or
    anything with text() -> bytes).  Returns the file's name."""
    outfilename = _translated_stem(inputargs) + ".clonotypes.tsv"
    text = clonotypes.text()
    if not inputargs["dontgzip"]:
        from . import _native as nat
        print("Compressing clonotype output file to", outfilename + ".gz")
        with nat.GzipWriter(outfilename + ".gz", level=int(os.environ.get("DCRX_GZIP_LEVEL", "6"))) as gz:
            gz.write(text)
        outfilename += ".gz"
    else:
        with open(outfilename, "wb") as fh:
            fh.write(text)
    sort_permissions(outfilename)
    return outfilename


def _write_beside_tsv(text: bytes, suffix: str, what: str, inputargs: dict):
    """`<the .tsv's stem><suffix>` with write_out_clonotypes' rules: gzipped unless dontgzip, mode 666.  Returns the name."""
    outfilename = _translated_stem(inputargs) + suffix
    if not inputargs["dontgzip"]:
        from . import _native as nat
        print(f"Compressing {what} output file to", outfilename + ".gz")
        with nat.GzipWriter(outfilename + ".gz", level=int(os.environ.get("DCRX_GZIP_LEVEL", "6"))) as gz:
            gz.write(text)
        outfilename += ".gz"
    else:
        with open(outfilename, "wb") as fh:
            fh.write(text)
    sort_permissions(outfilename)
    return outfilename


def write_out_overlap(text: bytes, name: str, inputargs: dict, what: str = "overlap"):
    """A file of the `overlap` sub-command: `<outpath><prefix><name>` (overlap_pairs.tsv, overlap_public.tsv,
    overlap_diversity.tsv), with
    write_out_clonotypes' rules: gzipped unless dontgzip, mode 666.  Returns the file's name."""
    outfilename = (inputargs.get("outpath") or "") + (inputargs.get("prefix") or "") + name
    if not inputargs.get("dontgzip"):
        from . import _native as nat
        print(f"Compressing {what} output file to", outfilename + ".gz")
        with nat.GzipWriter(outfilename + ".gz", level=int(os.environ.get("DCRX_GZIP_LEVEL", "6"))) as gz:
            gz.write(text)
        outfilename += ".gz"
    else:
        with open(outfilename, "wb") as fh:
            fh.write(text)
    sort_permissions(outfilename)
    return outfilename


def write_out_match(text: bytes, name: str, inputargs: dict):
    """A file of the `match` sub-command: `<outpath><prefix><name>` (<sample>.cdr3_matches.tsv, match_targets.tsv), with
    write_out_overlap's rules.  Returns the file's name."""
    return write_out_overlap(text, name, inputargs, what="match")


def write_out_motifs(text: bytes, name: str, inputargs: dict):
    """A file of the `motifs` sub-command: `<outpath><prefix><name>` (<sample>.cdr3_motifs.tsv, and with --groups
    <sample>.cdr3_groups.tsv and <sample>.cdr3_motif_members.tsv), with write_out_overlap's rules.
    Returns the file's name."""
    return write_out_overlap(text, name, inputargs, what="motif")


def write_out_metaclonotypes(text: bytes, name: str, inputargs: dict):
    """A file of the `metaclonotypes` sub-command: `<outpath><prefix><name>` (<sample>.cdr3_metaclonotypes.tsv, and on demand
    <sample>.cdr3_radius_profile.tsv and <sample>.cdr3_metaclonotype_members.tsv), with write_out_overlap's rules.  Returns the
    file's name."""
    return write_out_overlap(text, name, inputargs, what="meta-clonotype")


def write_out_tabulate(text: bytes, name: str, inputargs: dict):
    """A file of the `tabulate` sub-command: `<outpath><prefix><name>` (tabulate.tsv, tabulate_samples.tsv), with
    write_out_overlap's rules.  Returns the file's name."""
    return write_out_overlap(text, name, inputargs, what="tabulate")


def write_out_cdr3_clusters(network, inputargs: dict):
    """The cluster table of --cdr3-network beside the `.tsv`: `<the .tsv's stem>.cdr3_clusters.tsv`, tab separated with a
    header line, one row per clonotype in the clonotype table's order (clonotype = the 0-based row of the `.clonotypes.tsv`).
    `network`: translate.Cdr3Network (or anything with text() -> bytes).  Returns the file's name."""
    return _write_beside_tsv(network.text(), ".cdr3_clusters.tsv", "CDR3 cluster", inputargs)


def write_out_cdr3_edges(network, inputargs: dict):
    """The edges of --cdr3-network --write-cdr3-edges: `<the .tsv's stem>.cdr3_edges.tsv`, header `a b distance`, one line
    per linked pair a < b, ascending by (a, b).  `network`: anything with edges_text() -> bytes.  Returns the file's name."""
    return _write_beside_tsv(network.edges_text(), ".cdr3_edges.tsv", "CDR3 edge", inputargs)


def write_out_translated(rows, headers, inputargs: dict):
    """The AIRR table of the translate stage (reference io.py:516-548: `DataFrame.to_csv(sep="\t", index=False)`, then the
    gzip step unless dontgzip, then mode 666): `<outpath><file id>.tsv[.gz]` for the translate / collapse commands, the
    pipeline's `<prefix><file id>_<chain name>.tsv[.gz]` otherwise.  A missing value (None) is an empty field, as to_csv
    writes it."""
    outfilename = _translated_stem(inputargs) + ".tsv"

    def lines():
        yield "\t".join(headers) + "\n"
        for r in rows:
            yield "\t".join("" if x is None else str(x) for x in r) + "\n"

    if not inputargs["dontgzip"]:
        from . import _native as nat
        print("Compressing pipeline output file to", outfilename + ".gz")
        with nat.GzipWriter(outfilename + ".gz", level=int(os.environ.get("DCRX_GZIP_LEVEL", "6"))) as gz:
            out = _GzText(gz)
            for ln in lines():
                out.write(ln)
            out.flush()
        outfilename += ".gz"
    else:
        with open(outfilename, "w") as fh:
            fh.writelines(lines())
    sort_permissions(outfilename)
    return outfilename


def write_out_associate(text: bytes, name: str, inputargs: dict):
    """A file of the `associate` sub-command: `<outpath><prefix><name>` (associate.tsv, associate_null.tsv), with
    write_out_overlap's rules.  Returns the file's name."""
    return write_out_overlap(text, name, inputargs, what="associate")
