"""ctypes binding of libkaptive_amd.so (include/kaptive_amd.h).  There is no fallback: if the library or a GPU is
missing, every entry point raises."""

from __future__ import annotations

import atexit
import ctypes as C
import os
import threading
import weakref
from collections import namedtuple
from pathlib import Path

import numpy as np

LIB_PATH = Path(__file__).resolve().parent / "libkaptive_amd.so"
MAX_GENE_LEN = 65535  # KP_MAX_GENE_LEN of include/kp_spec.h (tests/test_native_abi.py compares the two)
FILL16_MAX_GENE_LEN = 15800  # KP_FILL16_MAX_GENE_LEN: longer genes are filled with 32-bit scores
WORK_SLOTS = 3  # KP_WORK_SLOTS of include/kaptive_amd.h: alignment results a context keeps resident
MAX_GENES = 131071  # KP_MAX_GENES of include/kp_spec.h: genes one context holds, all of its databases together
MAX_TYPING_GROUPS = 16  # KP_MAX_TYPING_GROUPS of include/kaptive_amd.h: databases one context types

HIT_DTYPE = np.dtype(
    [("gene", "<i4"), ("contig", "<i4"), ("q_start", "<i4"), ("q_end", "<i4"), ("t_start", "<i4"), ("t_end", "<i4"),
     ("score", "<i4"), ("matches", "<i4"), ("block_len", "<i4"), ("strand", "i1"), ("mapq", "u1"), ("n_seeds", "u1"), ("pad", "u1")]
)  # fmt: skip
TASK_DTYPE = np.dtype(
    [("gs", "<i4"), ("contig", "<i4"), ("lo", "<i4"), ("width", "<i4"), ("n_anchors", "<i4"), ("qmin", "<i4"),
     ("qmax", "<i4"), ("chain_score", "<i4")]
)  # fmt: skip

VARIANT_DTYPE = np.dtype(
    [("kept", "<i4"), ("q_pos", "<i4"), ("t_pos", "<i4"), ("len", "<i4"), ("kind", "u1"), ("ref", "u1"), ("alt", "u1"),
     ("ref_aa", "u1"), ("alt_aa", "u1"), ("pad", "u1", (3,))]
)  # fmt: skip (kp_variant of include/kp_spec.h, VARIANTS: 24 bytes; kind 0 = snv, 1 = ins, 2 = del)
VARIANTS_HEADER = (b"Assembly\tContig\tPosition\tStrand\tGene\tGene position\tType\tLength\tRef\tAlt\tCodon\tRef aa\tAlt aa\t"
                   b"Effect\n")  # the columns of kp_format_variants

BREAKPOINT_DTYPE = np.dtype(
    [("kept_a", "<i4"), ("kept_b", "<i4"), ("q_gap", "<i4"), ("t_gap", "<i4"), ("t_lo", "<i4"), ("edge_a", "<i4"), ("edge_b", "<i4"),
     ("kind", "u1"), ("ir_cols", "u1"), ("ir_matches", "u1"), ("pad", "u1")]
)  # fmt: skip (kp_breakpoint of include/kp_spec.h, BREAKPOINTS: 32 bytes; kind 0 = collinear, 1 = inverted, 2 = disordered, 3 = contigs)
BREAKPOINTS_HEADER = (b"Assembly\tGene\tEvent\tGene position\tGene gap\tContig A\tPosition A\tStrand A\tContig B\tPosition B\tStrand B\t"
                      b"Length\tDuplication\tEdge A\tEdge B\tInverted repeat\n")  # the columns of kp_format_breakpoints

ALLELE_DTYPE = np.dtype([("nt", "<u8"), ("aa", "<u8")])  # kp_allele of include/kp_spec.h, ALLELES: 16 bytes; aa is 0 where prot_len is 0
ALLELES_HEADER = (b"Assembly\tLocus\tLocus allele\tGene\tSet\tContig\tStart\tEnd\tStrand\tState\tLength\tAllele\tProtein length\t"
                  b"Protein allele\n")  # the columns of kp_format_alleles

ALIGNED_ROW_DTYPE = np.dtype([("off", "<i8"), ("gene_len", "<i4"), ("covered", "<i4"), ("inserted", "<i4"), ("n_ins", "<i4")])  # kp_aligned_row of include/kp_spec.h, ALIGNED ROWS: 24 bytes
ALIGNED_HEADER = (b"Assembly\tGene\tContig\tStart\tEnd\tStrand\tGene length\tGene start\tGene end\tCovered\tInserted\tInsertions\t"
                  b"Aligned\n")  # the columns of kp_format_aligned
ALIGNED_GAP = 5  # the code ``aligned_codes`` gives a GAP column (0..3 bases, 4 inside an N run)
BLOCK_N_SHIFT, BLOCK_GAP_SHIFT = 32, 48  # KP_DIST_N_SHIFT, KP_DIST_GAP_SHIFT of kaptive_amd/csrc/kp_dist.h: the N mask and the gap mask of a 16-column block

RESCUE_DTYPE = np.dtype(
    [("gene", "<i4"), ("piece", "<i4"), ("contig", "<i4"), ("t_start", "<i4"), ("t_end", "<i4"), ("score", "<i4"), ("matches", "<i4"),
     ("mismatches", "<i4"), ("gaps", "<i4"), ("p_start", "<i4"), ("p_end", "<i4"), ("stops", "<i4"), ("a_len", "<i4"), ("strand", "i1"),
     ("frame", "u1"), ("edge", "u1"), ("pad", "u1")]
)  # fmt: skip (kp_rescue of include/kp_spec.h, RESCUE: 56 bytes; piece -1 = nothing found)
RESCUE_HEADER = (b"Assembly\tLocus\tGene\tProtein length\tCall\tScore\tContig\tStart\tEnd\tStrand\tFrame\tProtein start\tProtein end\t"
                 b"Matches\tMismatches\tGaps\tIdentity\tCoverage\tStops\tEdge\n")  # the columns of kp_format_rescue
RESCUE_FLANK = 4096  # KP_RESCUE_FLANK of include/kp_spec.h (tests/test_native_abi.py's neighbours compare such pairs)
RESCUE_MIN_SCORE = 80  # KP_RESCUE_MIN_SCORE

# The reports derived from a reduction's kept list ("Reports derived from the kept list"), one row each: `name` (the command
# line's option, the keyword of Engine / Serotyper / BatchTyping, the key of a chunk's outputs), the `header` line of its table, the Batch
# method that fetches its records, the BatchTyping method that formats its lines (`tsv`), and the `noun` BatchTyping says a batch was
# typed without (its first word names the table).
Report = namedtuple("Report", "name header fetch tsv noun")
REPORTS = (
    Report("variants", VARIANTS_HEADER, "variants", "variants_tsv", "variant records"),
    Report("breakpoints", BREAKPOINTS_HEADER, "breakpoints", "breakpoints_tsv", "breakpoint records"),
    Report("alleles", ALLELES_HEADER, "alleles", "alleles_tsv", "allele digests"),
    Report("aligned", ALIGNED_HEADER, "aligned", "aligned_tsv", "aligned rows"),
    Report("rescue", RESCUE_HEADER, "rescue", "rescue_tsv", "rescue records"),
)

# Pairwise locus distances (include/kp_spec.h, DISTANCES): a layer beside the per-batch reports above, not one of them -- it spans the
# batches of a run (kaptive_amd/distances.py).
DIST_PAIR_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("compared", "<i4"), ("differences", "<i4"), ("unshared", "<i4"), ("pad", "<i4")])  # kp_dist_pair: 24 bytes
DISTANCES_HEADER = b"Locus\tAssembly A\tAssembly B\tColumns\tCompared\tDifferences\tUnshared\n"  # the columns of kp_format_distances
DIST_TILE = 64  # KP_DIST_TILE of kaptive_amd/csrc/kp_dist.h: pairs along either side of a workgroup's tile (tests/test_distances_cpu.py compares the mirrors)
DIST_CHUNK = 8  # KP_DIST_CHUNK: plane words (of 64 columns: four blocks) of a row strip that lie in LDS at a time
DIST_MAX_ROWS = 1 << 18  # KP_DIST_MAX_ROWS of kaptive_amd/csrc/kp_caps.h
DIST_MAX_DIFF = 10  # KP_DIST_MAX_DIFF of include/kp_spec.h: the command line's --max-distance
DIST_MIN_COMPARED = 1  # KP_DIST_MIN_COMPARED: its --min-compared
# Clusters and nearest neighbours of the same rows (include/kp_spec.h, CLUSTERS)
DIST_NEAREST_DTYPE = np.dtype([("row", "<i4"), ("compared", "<i4"), ("differences", "<i4"), ("unshared", "<i4")])  # kp_dist_nearest: 16 bytes
CLUST_MAX_LEVELS = 8  # KP_CLUST_MAX_LEVELS of include/kp_spec.h
CLUSTER_LEVELS = (0, 1, 2, 5, 10)  # the command line's --cluster-levels


def check_cluster_levels(levels) -> tuple:
    """``levels`` as a tuple of ints, or ValueError: at most CLUST_MAX_LEVELS, none negative, strictly ascending (kp_dist_clusters)."""
    lv = tuple(int(t) for t in levels)
    if len(lv) > CLUST_MAX_LEVELS or any(t < 0 or t > 2**31 - 1 for t in lv) or any(b <= a for a, b in zip(lv, lv[1:])):
        raise ValueError(f"cluster levels must be at most {CLUST_MAX_LEVELS} non-negative, strictly ascending numbers")
    return lv


def clusters_header(levels) -> bytes:
    """The header line of the cluster table for ``levels`` (the columns of kp_format_clusters)."""
    return ("\t".join(["Locus", "Assembly", *(f"HC{t}" for t in check_cluster_levels(levels)), "Nearest", "Differences", "Compared", "Unshared"]) + "\n").encode()


# Minimum spanning forest of the same rows (include/kp_spec.h, TREE): its edges are DIST_PAIR_DTYPE records, its edge table has the
# columns of DISTANCES_HEADER
TREE_MAX_COLUMNS = 1 << 28  # KP_TREE_MAX_COLUMNS of kaptive_amd/csrc/kp_caps.h: a locus of as many columns does not fit the packed edge key
NEWICK_HEADER = b"Locus\tTree\tAssemblies\tNewick\n"  # the columns of kp_format_newick


def newick_header() -> bytes:
    """The header line of the Newick table (the columns of kp_format_newick)."""
    return NEWICK_HEADER


# Neighbour-joining tree of the same rows (include/kp_spec.h, NJ)
NJ_NODE_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("c", "<i4"), ("pad", "<i4"), ("la", "<f8"), ("lb", "<f8"), ("lc", "<f8")])  # kp_nj_node: 40 bytes
NJ_MAX_TAXA = 16384  # KP_NJ_MAX_TAXA of kaptive_amd/csrc/kp_caps.h: the dense matrix of as many taxa is 2 GiB
NJ_HEADER = b"Locus\tAssemblies\tTaxa\tNewick\n"  # the columns of kp_format_nj


def nj_header() -> bytes:
    """The header line of the neighbour-joining table (the columns of kp_format_nj)."""
    return NJ_HEADER


# Bootstrap support of that tree (include/kp_spec.h, BOOTSTRAP)
BOOT_MAX_REPLICATES = 10000  # KP_BOOT_MAX_REPLICATES of kaptive_amd/csrc/kp_caps.h
BOOT_MATRIX_BYTES = 2 << 30  # KP_BOOT_MATRIX_BYTES: the matrices of one batch of replicates together
BOOT_MAX_BATCH = 65535  # KP_BOOT_MAX_BATCH: a replicate is a row of a grid
NJ_SUPPORT_HEADER = b"Locus\tAssemblies\tTaxa\tReplicates\tNewick\n"  # the columns of kp_format_nj_support


def nj_support_header() -> bytes:
    """The header line of the neighbour-joining table with support values (the columns of kp_format_nj_support)."""
    return NJ_SUPPORT_HEADER


# Variable sites of the same rows (include/kp_spec.h, SITES)
SITE_DTYPE = np.dtype([("column", "<i4"), ("n", "<i4", (4,)), ("n_n", "<i4")])  # kp_site: 24 bytes
SITES_HEADER = b"Locus\tGene\tPosition\tColumn\tAssemblies\tA\tC\tG\tT\tN\tGap\tAlleles\tMajor\tInformative\n"  # the columns of kp_format_sites
SNP_ALIGNMENT_HEADER = b"Locus\tAssembly\tSites\tAlignment\n"  # the columns of kp_format_site_rows
SITES_CORE = 1  # KP_SITES_CORE of include/kp_spec.h: a site must hold a base in every row
SITES_THREADS = 256  # KP_SITES_THREADS of kaptive_amd/csrc/kp_sites.h: lanes of a workgroup of the profile kernel (tests/test_sites_cpu.py compares the mirrors)
SITES_LANE_ROWS = 15  # KP_SITES_LANE_ROWS: rows a lane adds into its four-plane bit-sliced counters
SITES_SLAB = SITES_THREADS * SITES_LANE_ROWS  # KP_SITES_SLAB: rows of one workgroup

# Small parsimony of those columns on the neighbour-joining tree (include/kp_spec.h, PARSIMONY)
PARS_SITE_DTYPE = np.dtype([("column", "<i4"), ("steps", "<i4"), ("alleles", "<i4"), ("pad", "<i4")])  # kp_pars_site: 16 bytes
PARS_CHANGE_DTYPE = np.dtype([("column", "<i4"), ("node", "<i4"), ("parent", "<i4"), ("from", "u1"), ("to", "u1"), ("pad", "<u2")])  # kp_pars_change: 16 bytes
NJ_HOMOPLASY_HEADER = b"Locus\tGene\tPosition\tColumn\tAlleles\tSteps\tExcess\n"  # the columns of kp_format_nj_homoplasy
NJ_CHANGES_HEADER = b"Locus\tNode\tTip A\tTip B\tTips\tGene\tPosition\tColumn\tFrom\tTo\n"  # the columns of kp_format_nj_changes


def nj_homoplasy_header() -> bytes:
    """The header line of the homoplasy table (the columns of kp_format_nj_homoplasy)."""
    return NJ_HOMOPLASY_HEADER


def nj_changes_header() -> bytes:
    """The header line of the change table (the columns of kp_format_nj_changes)."""
    return NJ_CHANGES_HEADER


JOIN_MAX_PIECES = 8  # KP_JOIN_MAX_PIECES
JOIN_DTYPE = np.dtype(
    [("gs", "<i4"), ("contig", "<i4"), ("n_pieces", "<i4"), ("n_anchors", "<i4"), ("chain_score", "<i4"), ("width", "<i4"),
     ("lo", "<i4", (JOIN_MAX_PIECES,)), ("piece", "<i4", (JOIN_MAX_PIECES, 11))]
)  # fmt: skip (kp_batch_joins: per piece state, visited mask, cell score, q_start, q_end, t_start, t_end, matches, block_len, score, bonus)

EXPORTS = (
    "kp_ctx_create", "kp_ctx_destroy", "kp_last_error", "kp_ctx_stream", "kp_ctx_set_option", "kp_host_alloc",
    "kp_host_free", "kp_host_reserve", "kp_host_lock", "kp_host_pinned_bytes", "kp_device_allocations", "kp_db_load", "kp_db_n_postings", "kp_batch_create", "kp_batch_create_async",
    "kp_batch_upload_wait", "kp_batch_depends_on", "kp_batch_create_device", "kp_batch_device_words", "kp_batch_destroy", "kp_batch_align", "kp_batch_wait",
    "kp_batch_hit_offsets", "kp_batch_hits", "kp_batch_set_hits", "kp_batch_cigar_offsets", "kp_batch_cigars", "kp_batch_cs_offsets", "kp_batch_cs", "kp_batch_variant_offsets", "kp_batch_variants", "kp_format_variants", "kp_batch_breakpoint_offsets", "kp_batch_breakpoints", "kp_format_breakpoints", "kp_batch_alleles", "kp_format_alleles", "kp_allele_locus_digest", "kp_batch_aligned_size", "kp_batch_aligned_rows", "kp_batch_aligned_blocks", "kp_format_aligned", "kp_batch_rescue_offsets", "kp_batch_rescue", "kp_format_rescue", "kp_format_paf", "kp_format_paf_tags", "kp_batch_stats", "kp_batch_profile", "kp_batch_anchors",
    "kp_batch_tasks", "kp_batch_task_results", "kp_batch_joins", "kp_batch_occ", "kp_batch_candidates", "kp_db_load_typing", "kp_db_load_typing_group", "kp_batch_use_group", "kp_batch_score", "kp_batch_reduce", "kp_batch_typing_caps",
    "kp_device_count", "kp_device_numa_node", "kp_batch_typing", "kp_batch_proteins", "kp_protein_align", "kp_fasta_pack", "kp_fasta_ingest", "kp_fasta_ingest_many", "kp_fasta_ingest_file", "kp_fasta_ingest_shard", "kp_shard_words_into", "kp_shard_free", "kp_fasta_simd", "kp_pack_contigs",
    "kp_fasta_free", "kp_format_rows", "kp_format_json", "kp_format_fasta", "kp_protein_align_seeded", "kp_randstrobes", "kp_randstrobe_top_hits",
    "kp_dist_create", "kp_dist_count", "kp_dist_pairs", "kp_dist_destroy", "kp_format_distances", "kp_dist_clusters", "kp_format_clusters",
    "kp_dist_tree", "kp_dist_tree_rounds", "kp_format_newick", "kp_dist_nj", "kp_format_nj", "kp_dist_nj_bootstrap", "kp_dist_boot_weights", "kp_format_nj_support", "kp_dist_nj_transfer", "kp_format_nj_transfer",
    "kp_dist_profile", "kp_dist_sites_count", "kp_dist_sites", "kp_dist_site_rows", "kp_format_sites", "kp_format_site_rows",
    "kp_dist_nj_parsimony", "kp_dist_pars_sites", "kp_dist_pars_changes", "kp_format_nj_homoplasy", "kp_format_nj_changes",
)  # fmt: skip


class PackedFasta(C.Structure):  # kp_packed_fasta
    _fields_ = [("padded_len", C.c_int64), ("n_contigs", C.c_int32), ("n_runs", C.c_int32),
                ("words", C.POINTER(C.c_uint32)), ("ctg_start", C.POINTER(C.c_int32)), ("ctg_len", C.POINTER(C.c_int32)),
                ("n_run_pairs", C.POINTER(C.c_int32)), ("names", C.POINTER(C.c_char)), ("name_off", C.POINTER(C.c_int32)),
                ("seqs", C.POINTER(C.c_uint8)), ("n_seq_bytes", C.c_int64)]  # fmt: skip


class _FastaRecord:
    """Keeps a kp_packed_fasta alive for as long as an array that views its large buffers (packed words, sequence text)
    is: the arrays are handed out without a copy -- a copy is a few milliseconds with the GIL held per 5 Mbp assembly,
    which is what stopped a thread pool of readers from scaling -- and the buffers return to the library's block pool
    when the last view dies."""

    def __init__(self, out) -> None:
        self.out = out

    def __del__(self) -> None:
        try:
            h = lib()
            h.kp_fasta_free.restype = None
            h.kp_fasta_free(self.out)
        except Exception:  # interpreter shutdown
            pass

    def view(self, ptr, n: int, ctype, dtype) -> np.ndarray:
        if not n:
            return np.empty(0, dtype)
        buf = (ctype * n).from_address(C.addressof(ptr.contents))
        buf._record = self  # numpy keeps `buf` as the array's base, `buf` keeps the record
        return np.frombuffer(buf, dtype=dtype)


def _packed_from(out, want_names: bool, record: "_FastaRecord | None" = None):
    """kp_packed_fasta -> (PackedAssembly, names).  With ``record`` the packed words are a view of the library's buffer
    (the record frees it when the views are gone); without, everything is copied and the caller frees."""
    from kaptive_amd.pack import PackedAssembly

    p = out.contents
    nc, nr = p.n_contigs, p.n_runs
    arr = lambda ptr, n, dt: np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True) if n else np.empty(0, dt)  # noqa: E731
    if record is not None:
        words = record.view(p.words, p.padded_len // 16, C.c_uint32, np.uint32)
    else:
        words = arr(p.words, p.padded_len // 16, np.uint32)
    names = ()
    if want_names:
        off = arr(p.name_off, nc + 1, np.int32)
        blob = C.string_at(p.names, int(off[-1])) if nc else b""
        names = tuple(blob[off[i] : off[i + 1]].decode("utf-8", "replace") for i in range(nc))
    pa = PackedAssembly(words, int(p.padded_len), arr(p.ctg_start, nc, np.int32), arr(p.ctg_len, nc, np.int32),
                        arr(p.n_run_pairs, 2 * nr, np.int32).reshape(-1, 2))  # fmt: skip
    return pa, names


def pack_contigs(seqs: np.ndarray, offsets: np.ndarray, lengths: np.ndarray):
    """Contigs in memory (dense bytes + offsets + lengths) -> PackedAssembly, by the native packer (kp_pack_contigs;
    about ten times the numpy route)."""
    h = lib()
    h.kp_fasta_free.restype = None
    seqs, offsets, lengths = _c(seqs, np.uint8), _c(offsets, np.int64), _c(lengths, np.int32)
    out = C.POINTER(PackedFasta)()
    rc = h.kp_pack_contigs(_p(seqs), _p(offsets), _p(lengths), C.c_int32(len(lengths)), C.byref(out))
    if rc != 0:
        raise ValueError("assembly too long for the packed layout (KP_MAX_ASM_LEN)")
    try:
        return _packed_from(out, False)[0]
    finally:
        h.kp_fasta_free(out)


FASTA_FLAGS = {None: 0, "": 0, False: 0, True: 1, "gz": 1, "bz2": 4, "xz": 8}  # KP_FASTA_GZIP / _BZ2 / _XZ
ENOTSUP = -6
EIO = -7


def _host_inflate(data: bytes, compression) -> bytes:
    """bz2 / xz through Python's own modules: only for hosts whose libbz2 / liblzma the library could not load."""
    import bz2
    import lzma

    return (bz2.decompress if compression == "bz2" else lzma.decompress)(data)


def fasta_ingest(data: bytes, gzipped: "bool | str | None" = False, keep_text: bool = True):
    """A FASTA file's bytes -> (PackedAssembly, contig names, sequence text uint8, contig lengths int32) in one native
    pass (kp_fasta_ingest: inflate -- `gzipped` is True / "gz", "bz2" or "xz" --, split records, strip whitespace, pack;
    no GPU needed).  ``keep_text=False`` leaves the sequence text out (empty array): a run that only writes the TSV
    report never looks at it."""
    h = lib()
    h.kp_fasta_free.restype = None
    out = C.POINTER(PackedFasta)()
    text = 2 if keep_text else 0
    rc = h.kp_fasta_ingest(data, C.c_int64(len(data)), C.c_int32(FASTA_FLAGS[gzipped] | text), C.byref(out))
    if rc == ENOTSUP:
        data = _host_inflate(data, gzipped)
        rc = h.kp_fasta_ingest(data, C.c_int64(len(data)), C.c_int32(text), C.byref(out))
    if rc != 0:
        raise ValueError(f"kp_fasta_ingest failed ({rc}): not a readable FASTA / gzip stream, or longer than KP_MAX_ASM_LEN")
    record = _FastaRecord(out)  # frees the native record when the arrays below are gone
    pa, names = _packed_from(out, True, record)
    p = out.contents
    seqs = record.view(p.seqs, int(p.n_seq_bytes), C.c_uint8, np.uint8)
    return pa, names, seqs, pa.ctg_len.copy()


def fasta_ingest_file(path, gzipped: "bool | str | None" = False, keep_text: bool = True):
    """``fasta_ingest`` of a file by its path (kp_fasta_ingest_file): the library reads the file into a recycled buffer of its
    own, so its text never becomes a Python bytes object.  Falls back to reading the file here when the path is not a regular file or the
    host lacks the decompression library."""
    import os

    h = lib()
    h.kp_fasta_free.restype = None
    out = C.POINTER(PackedFasta)()
    text = 2 if keep_text else 0
    rc = h.kp_fasta_ingest_file(os.fsencode(path), C.c_int32(FASTA_FLAGS[gzipped] | text), C.byref(out))
    if rc in (ENOTSUP, EIO):
        with open(path, "rb") as f:
            return fasta_ingest(f.read(), gzipped, keep_text)
    if rc != 0:
        raise ValueError(f"kp_fasta_ingest_file failed ({rc}) for {path}: not a readable FASTA / compressed stream, or longer "
                         "than KP_MAX_ASM_LEN")
    record = _FastaRecord(out)
    pa, names = _packed_from(out, True, record)
    p = out.contents
    seqs = record.view(p.seqs, int(p.n_seq_bytes), C.c_uint8, np.uint8)
    return pa, names, seqs, pa.ctg_len.copy()


class _PackedShard(C.Structure):  # kp_packed_shard
    _fields_ = [("n_asm", C.c_int32), ("n_failed", C.c_int32), ("first_failed", C.c_int32), ("total_words", C.c_int64),
                ("asm_word_off", C.POINTER(C.c_int64)), ("ctg_start", C.POINTER(C.c_int32)), ("ctg_len", C.POINTER(C.c_int32)),
                ("asm_first_ctg", C.POINTER(C.c_int32)), ("n_runs", C.POINTER(C.c_int32)), ("asm_first_nrun", C.POINTER(C.c_int32)),
                ("rc", C.POINTER(C.c_int32))]  # fmt: skip


class FastaShard:
    """A chunk of FASTA files parsed and packed by the library's own threads (kp_fasta_ingest_shard), held as the tables
    of one batch: no per-file Python work at all -- with a Python call per file, names and arrays included, the interpreter
    lock capped a reader pool at ~6.5 k files/s whatever the parser did.  ``words_into`` copies the packed words into
    page-locked memory (kp_shard_words_into); ``Batch(ctx, tables=shard.tables(), pinned_words=...)`` uploads them."""

    def __init__(self, paths, compressions, threads: int = 0) -> None:
        import os

        h = lib()
        h.kp_shard_free.restype = None
        n = len(paths)
        self._paths = [os.fsencode(p) for p in paths]
        arr = (C.c_char_p * max(n, 1))(*self._paths)
        fl = (C.c_int32 * max(n, 1))(*[FASTA_FLAGS[c] for c in compressions])
        self._h = C.POINTER(_PackedShard)()
        rc = h.kp_fasta_ingest_shard(arr, fl, C.c_int32(n), C.c_int32(threads), C.byref(self._h))
        if rc != 0:
            raise MemoryError(f"kp_fasta_ingest_shard failed ({rc})")
        sh = self._h.contents
        self.n_asm, self.total_words = n, int(sh.total_words)
        self.failed = []
        if sh.n_failed:
            self.failed = [(i, int(sh.rc[i])) for i in range(n) if sh.rc[i] != 0]

    def tables(self) -> tuple:
        """(asm_word_off, ctg_start, ctg_len, asm_first_ctg, n_runs, asm_first_nrun): views of the library's arrays, valid
        while this object lives."""
        sh, n = self._h.contents, self.n_asm

        def view(ptr, k, dt):
            return np.ctypeslib.as_array(ptr, shape=(k,)) if k else np.empty(0, dt)

        first_ctg = view(sh.asm_first_ctg, n + 1, np.int32)
        first_run = view(sh.asm_first_nrun, n + 1, np.int32)
        nc, nr = (int(first_ctg[-1]), int(first_run[-1])) if n else (0, 0)
        return (view(sh.asm_word_off, n + 1, np.int64), view(sh.ctg_start, nc, np.int32), view(sh.ctg_len, nc, np.int32),
                first_ctg, view(sh.n_runs, 2 * nr, np.int32), first_run)

    def words_into(self, dst: np.ndarray, threads: int = 0) -> None:
        if dst.dtype != np.uint32 or not dst.flags.c_contiguous or len(dst) < self.total_words:
            raise ValueError("words_into needs a contiguous uint32 array of at least total_words")
        rc = lib().kp_shard_words_into(self._h, _p(dst), C.c_int64(len(dst)), C.c_int32(threads))
        if rc != 0:
            raise RuntimeError(f"kp_shard_words_into failed ({rc})")

    def close(self) -> None:
        if getattr(self, "_h", None):
            try:
                lib().kp_shard_free(self._h)
            except Exception:  # interpreter shutdown
                pass
            self._h = None

    __del__ = close


def device_count() -> int:
    """GPUs this process sees (kp_device_count)."""
    n = lib().kp_device_count()
    if n < 0:
        raise NativeError(f"kp_device_count failed ({n}): {lib().kp_last_error(None).decode()}")
    return int(n)


def compression_is_native() -> bool:
    """Whether the library found libbz2 and liblzma on this host (both tried with an empty stream)."""
    h = lib()
    out = C.POINTER(PackedFasta)()
    h.kp_fasta_free.restype = None
    ok = True
    for f in (4, 8):
        rc = h.kp_fasta_ingest(b"", C.c_int64(0), C.c_int32(f), C.byref(out))
        if rc == 0:
            h.kp_fasta_free(out)
        ok = ok and rc != ENOTSUP
    return ok


def fasta_ingest_many(datas: "list[bytes]", gzipped: "list[bool] | bool" = False, threads: int = 0) -> list:
    """``fasta_ingest`` of many files in one native call on the library's own threads (kp_fasta_ingest_many; 0 = one per
    core): a list of (PackedAssembly, names, sequence text, contig lengths), in input order.  Raises for the first file
    that could not be read."""
    h = lib()
    n = len(datas)
    if n == 0:
        return []
    flags = [gzipped] * n if isinstance(gzipped, (bool, str)) or gzipped is None else list(gzipped)
    if any(FASTA_FLAGS[g] & 12 for g in flags) and not compression_is_native():
        datas = [_host_inflate(d, g) if FASTA_FLAGS[g] & 12 else d for d, g in zip(datas, flags)]
        flags = [None if FASTA_FLAGS[g] & 12 else g for g in flags]
    ptrs = (C.c_char_p * n)(*datas)
    lens = (C.c_int64 * n)(*[len(d) for d in datas])
    fl = (C.c_int32 * n)(*[FASTA_FLAGS[g] | 2 for g in flags])
    outs = (C.POINTER(PackedFasta) * n)()
    rcs = (C.c_int32 * n)()
    rc = h.kp_fasta_ingest_many(ptrs, lens, fl, C.c_int32(n), C.c_int32(threads), outs, rcs)
    if rc != 0:
        raise ValueError(f"kp_fasta_ingest_many failed ({rc})")
    records = [_FastaRecord(C.cast(outs[i], C.POINTER(PackedFasta))) if rcs[i] == 0 else None for i in range(n)]
    result = []
    for i, rec in enumerate(records):
        if rec is None:
            raise ValueError(f"kp_fasta_ingest failed ({rcs[i]}) for file {i}: not a readable FASTA / gzip stream, or longer "
                             "than KP_MAX_ASM_LEN")
        pa, names = _packed_from(rec.out, True, rec)
        p = rec.out.contents
        result.append((pa, names, rec.view(p.seqs, int(p.n_seq_bytes), C.c_uint8, np.uint8), pa.ctg_len.copy()))
    return result


def fasta_pack(data: bytes):
    """FASTA text -> (PackedAssembly, contig names), parsed and packed by the native library (no GPU needed)."""
    h = lib()
    h.kp_fasta_free.restype = None
    out = C.POINTER(PackedFasta)()
    rc = h.kp_fasta_pack(data, C.c_int64(len(data)), C.byref(out))
    if rc != 0:
        raise ValueError(f"kp_fasta_pack failed ({rc}): sequence too long for the packed layout or bad arguments")
    try:
        return _packed_from(out, True)
    finally:
        h.kp_fasta_free(out)


class TypingTables(C.Structure):  # kp_typing_tables
    _fields_ = [("gene_locus", C.c_void_p), ("gene_extra", C.c_void_p), ("gene_pos", C.c_void_p),
                ("gene_strand", C.c_void_p), ("locus_gene_off", C.c_void_p), ("locus_gene_len", C.c_void_p),
                ("n_loci", C.c_int32), ("prot", C.c_void_p), ("prot_off", C.c_void_p), ("prot_len", C.c_void_p)]  # fmt: skip


class RowTables(C.Structure):  # kp_row_tables
    _fields_ = [("prefix", C.c_char_p), ("prefix_len", C.c_int32), ("gene_ids", C.c_void_p), ("gene_id_off", C.c_void_p),
                ("locus_names", C.c_void_p), ("locus_name_off", C.c_void_p), ("locus_gene_off", C.c_void_p),
                ("locus_gene_len", C.c_void_p)]  # fmt: skip


class RowColumns(C.Structure):  # kp_row_columns
    _fields_ = [("asm_ids", C.c_void_p), ("asm_id_off", C.c_void_p), ("phenotypes", C.c_void_p),
                ("phenotype_off", C.c_void_p), ("best_locus", C.c_void_p), ("typeable", C.c_void_p),
                ("problems", C.c_void_p), ("identity", C.c_void_p), ("coverage", C.c_void_p),
                ("length_discrepancy", C.c_void_p)]  # fmt: skip


def _blob(strings) -> tuple[np.ndarray, np.ndarray]:
    """utf-8 strings -> (bytes back to back, n + 1 offsets)."""
    enc = [s if isinstance(s, bytes) else str(s).encode("utf-8") for s in strings]
    off = np.zeros(len(enc) + 1, np.int32)
    if enc:
        np.cumsum([len(e) for e in enc], out=off[1:])
    return np.frombuffer(b"".join(enc) or b"\0", np.uint8), off


class RowFormatter:
    """KaptiveRow bytes for whole batches (kp_format_rows); the database's string tables are prepared once."""

    def __init__(self, db, kaptive_version: str) -> None:
        meta = db.metadata
        self._prefix = f"{kaptive_version}\t{meta.name}\t{meta.version}\t".encode("utf-8")
        self._keep = dict(
            gene_ids=_blob(db.genes.ids), locus_names=_blob(db.loci.ids),
            locus_gene_off=_c(db.locus_gene_offsets, np.int32), locus_gene_len=_c(db.locus_gene_lengths, np.int32),
        )  # fmt: skip
        k = self._keep
        self._tables = RowTables(
            prefix=self._prefix, prefix_len=len(self._prefix), gene_ids=_p(k["gene_ids"][0]).value,
            gene_id_off=_p(k["gene_ids"][1]).value, locus_names=_p(k["locus_names"][0]).value,
            locus_name_off=_p(k["locus_names"][1]).value, locus_gene_off=_p(k["locus_gene_off"]).value,
            locus_gene_len=_p(k["locus_gene_len"]).value,
        )  # fmt: skip

    def format(self, ids, phenotypes, sums, kept, best_locus, typeable, problems, identity, coverage, discrepancy) -> bytes:
        n = len(sums)
        if n == 0:
            return b""
        ids_b, ids_o = _blob(ids)
        ph_b, ph_o = _blob(phenotypes)
        cols = dict(best=_c(best_locus, np.int32), typeable=_c(typeable, np.uint8), problems=_c(problems, np.int32),
                    identity=_c(identity, np.float64), coverage=_c(coverage, np.float64),
                    discrepancy=_c(discrepancy, np.float64))  # fmt: skip
        c = RowColumns(asm_ids=_p(ids_b).value, asm_id_off=_p(ids_o).value, phenotypes=_p(ph_b).value,
                       phenotype_off=_p(ph_o).value, best_locus=_p(cols["best"]).value, typeable=_p(cols["typeable"]).value,
                       problems=_p(cols["problems"]).value, identity=_p(cols["identity"]).value,
                       coverage=_p(cols["coverage"]).value, length_discrepancy=_p(cols["discrepancy"]).value)  # fmt: skip
        sums, kept = np.ascontiguousarray(sums), np.ascontiguousarray(kept)
        stride = kept.shape[1] if kept.ndim == 2 else 0
        h = lib()
        h.kp_format_rows.restype = C.c_int64
        return _sized("kp_format_rows", 1200 * n, lambda out, cap: h.kp_format_rows(
            C.byref(self._tables), C.c_int32(n), _p(sums), _p(kept), C.c_int32(stride), C.byref(c), out, cap))


def _sized(name: str, room: int, call) -> bytes:
    """The bytes of one of the formatters: ``call(out, cap)`` formats into ``out`` and returns the room the table needs -- so a first
    buffer of ``room`` bytes is tried, and one of exactly the size asked for if that was too small."""
    out = np.empty(max(4096, room), np.uint8)
    for _ in range(2):
        need = call(_p(out), C.c_int64(len(out)))
        if need < 0:
            raise ValueError(f"{name} failed ({need})")
        if need <= len(out):
            return out[:need].tobytes()
        out = np.empty(int(need), np.uint8)
    raise NativeError(f"{name}: size kept changing")


class PafTables(C.Structure):  # kp_paf_tables
    _fields_ = [("gene_names", C.c_void_p), ("gene_name_off", C.c_void_p), ("gene_len", C.c_void_p), ("n_genes", C.c_int32),
                ("ctg_names", C.c_void_p), ("ctg_name_off", C.c_void_p), ("ctg_len", C.c_void_p), ("asm_first_ctg", C.c_void_p)]  # fmt: skip


PAF_CS, PAF_EQX = 1, 2  # KP_PAF_CS, KP_PAF_EQX


def _format_paf(gene_names, gene_lengths, contig_names, contig_lengths, asm_first_ctg, hits, hit_off, ops, cigar_off, cs=None, cs_off=None,
                flags: int = 0) -> bytes:
    """``format_paf`` (kp_format_paf), or with ``cs_off`` ``format_paf_tags`` (kp_format_paf_tags)."""
    tags = cs_off is not None
    gn_b, gn_o = _blob(gene_names)
    cn_b, cn_o = _blob64(contig_names)
    gene_len, ctg_len, first = _c(gene_lengths, np.int32), _c(contig_lengths, np.int32), _c(asm_first_ctg, np.int64)
    hits, hit_off = np.ascontiguousarray(hits, dtype=HIT_DTYPE), _c(hit_off, np.int64)
    ops, cigar_off = _c(ops, np.uint32), _c(cigar_off, np.int64)
    n_asm, n_hits = len(hit_off) - 1, len(hits)
    if tags:
        cs, cs_off = _c(np.frombuffer(cs, np.uint8) if isinstance(cs, (bytes, bytearray)) else cs, np.uint8), _c(cs_off, np.int64)
    if len(first) != n_asm + 1 or len(cigar_off) != n_hits + 1 or (tags and len(cs_off) != n_hits + 1) or int(hit_off[-1]) != n_hits:
        raise ValueError("offsets do not describe the hit table")
    if int(first[-1]) > len(ctg_len) or len(cn_o) != len(ctg_len) + 1 or len(gene_len) != len(gn_o) - 1:
        raise ValueError("name and length tables disagree")
    if tags and (int(cs_off[-1]) > len(cs) or int(cigar_off[-1]) > len(ops)):
        raise ValueError("offsets run past their arrays")
    t = PafTables(gene_names=_p(gn_b).value, gene_name_off=_p(gn_o).value, gene_len=_p(gene_len).value, n_genes=len(gn_o) - 1,
                  ctg_names=_p(cn_b).value, ctg_name_off=_p(cn_o).value, ctg_len=_p(ctg_len).value, asm_first_ctg=_p(first).value)  # fmt: skip
    h = lib()
    h.kp_format_paf.restype = h.kp_format_paf_tags.restype = C.c_int64
    if not tags:
        return _sized("kp_format_paf", 160 * n_hits + 8 * len(ops), lambda out, cap: h.kp_format_paf(
            C.byref(t), C.c_int32(n_asm), _p(hits), _p(hit_off), _p(ops), _p(cigar_off), out, cap))
    return _sized("kp_format_paf_tags", 176 * n_hits + 8 * len(ops) + 2 * len(cs), lambda out, cap: h.kp_format_paf_tags(
        C.byref(t), C.c_int32(n_asm), _p(hits), _p(hit_off), _p(ops), _p(cigar_off), _p(cs), _p(cs_off), C.c_int32(int(flags)), out, cap))


def format_paf(gene_names, gene_lengths, contig_names, contig_lengths, asm_first_ctg, hits, hit_off, ops, cigar_off) -> bytes:
    """PAF lines of a hit table (kp_format_paf; host only): one per hit, in the table's order.  ``contig_names`` /
    ``contig_lengths`` list the contigs of all assemblies back to back, assembly a's are ``asm_first_ctg[a]:asm_first_ctg[a + 1]``;
    ``hits`` are HIT_DTYPE rows, ``hit_off`` their per-assembly offsets, ``ops`` / ``cigar_off`` as ``Batch.cigars`` returns them."""
    return _format_paf(gene_names, gene_lengths, contig_names, contig_lengths, asm_first_ctg, hits, hit_off, ops, cigar_off)


def format_paf_tags(gene_names, gene_lengths, contig_names, contig_lengths, asm_first_ctg, hits, hit_off, ops, cigar_off, cs, cs_off,
                    flags: int) -> bytes:
    """``format_paf`` with what the cs strings add (kp_format_paf_tags): ``flags`` is ``PAF_CS`` (a ``cs:Z:`` tag behind ``cg:Z:``),
    ``PAF_EQX`` (``cg:Z:`` in =/X form) or both; ``cs`` / ``cs_off`` as ``Batch.cs`` returns them.  A cs string that does not fit
    its hit's ops raises ``ValueError``."""
    return _format_paf(gene_names, gene_lengths, contig_names, contig_lengths, asm_first_ctg, hits, hit_off, ops, cigar_off, cs, cs_off, flags)


class VariantTables(C.Structure):  # kp_variant_tables
    _fields_ = [("gene_names", C.c_void_p), ("gene_name_off", C.c_void_p), ("n_genes", C.c_int32), ("asm_names", C.c_void_p),
                ("asm_name_off", C.c_void_p), ("ctg_names", C.c_void_p), ("ctg_name_off", C.c_void_p), ("asm_first_ctg", C.c_void_p)]  # fmt: skip


class AlleleTables(C.Structure):  # kp_allele_tables
    _fields_ = [("names", VariantTables), ("locus_names", C.c_void_p), ("locus_name_off", C.c_void_p), ("n_loci", C.c_int32)]


def _batch_names(gene_names, asm_names, contig_names, asm_first_ctg, n_asm: int, locus_names=None, per_asm=(), per_gene=()):
    """The name tables of a batch of ``n_asm`` assemblies as kp_variant_tables -- with ``locus_names`` as kp_allele_tables --, and the
    arrays the struct points into, which the caller keeps for as long as it uses it.  ``per_asm`` / ``per_gene``: further columns that
    must have an entry per assembly / per gene."""
    gn_b, gn_o = _blob(gene_names)
    an_b, an_o = _blob64(asm_names)
    cn_b, cn_o = _blob64(contig_names)
    first = _c(asm_first_ctg, np.int64)
    if (len(first) != n_asm + 1 or len(an_o) != n_asm + 1 or any(len(c) != n_asm for c in per_asm) or any(len(c) != len(gn_o) - 1 for c in per_gene)
            or (n_asm and int(first[-1]) > len(cn_o) - 1)):
        raise ValueError("name tables do not describe the batch")
    t = VariantTables(gene_names=_p(gn_b).value, gene_name_off=_p(gn_o).value, n_genes=len(gn_o) - 1, asm_names=_p(an_b).value,
                      asm_name_off=_p(an_o).value, ctg_names=_p(cn_b).value, ctg_name_off=_p(cn_o).value, asm_first_ctg=_p(first).value)  # fmt: skip
    keep = [gn_b, gn_o, an_b, an_o, cn_b, cn_o, first]
    if locus_names is not None:
        ln_b, ln_o = _blob(locus_names)
        t = AlleleTables(names=t, locus_names=_p(ln_b).value, locus_name_off=_p(ln_o).value, n_loci=len(ln_o) - 1)
        keep += [ln_b, ln_o]
    return t, keep


def _kept_table(kept, n_asm: int, records=None, and_records: str = ""):
    """``kept`` as the contiguous [n_asm, stride] table of ``Batch.typing`` and its stride; ``records``, where given, has its shape."""
    from kaptive_amd.serotyping.batch import KEPT_DTYPE

    kept = np.ascontiguousarray(kept)
    if kept.itemsize != KEPT_DTYPE.itemsize or (n_asm and (kept.ndim != 2 or kept.shape[0] != n_asm)) or (records is not None and records.shape != kept.shape):
        raise ValueError("kept must be the [n_asm, stride] table of Batch.typing" + and_records)
    return kept, (kept.shape[1] if kept.ndim == 2 else 0)


def _record_runs(off, records) -> np.ndarray:
    """The per-assembly offsets of ``records`` as int64 [n_asm + 1]: they must lie inside the records."""
    off = _c(off, np.int64)
    if len(off) > 1 and (int(off[0]) < 0 or int(off[-1]) > len(records)):
        raise ValueError("offsets run past the records")
    return off


def format_variants(gene_names, asm_names, contig_names, asm_first_ctg, kept, variants, var_off) -> bytes:
    """The lines of the variant table (kp_format_variants; host only; no header: ``VARIANTS_HEADER``): one per record of
    ``variants`` (VARIANT_DTYPE), assembly a's being ``var_off[a]:var_off[a + 1]``.  ``kept`` is the [n_asm, stride] table of
    ``Batch.typing``; ``contig_names`` lists the contigs of all assemblies back to back, assembly a's are
    ``asm_first_ctg[a]:asm_first_ctg[a + 1]``."""
    variants = np.ascontiguousarray(variants, dtype=VARIANT_DTYPE)
    n_asm = len(var_off) - 1
    kept, stride = _kept_table(kept, n_asm)
    t, keep = _batch_names(gene_names, asm_names, contig_names, asm_first_ctg, n_asm)
    var_off = _record_runs(var_off, variants)
    h = lib()
    h.kp_format_variants.restype = C.c_int64
    return _sized("kp_format_variants", 160 * len(variants), lambda out, cap: h.kp_format_variants(
        C.byref(t), C.c_int32(n_asm), _p(kept), C.c_int32(stride), _p(variants), _p(var_off), out, cap))


def format_breakpoints(gene_names, asm_names, contig_names, asm_first_ctg, kept, breakpoints, bp_off, edge_tolerance: int) -> bytes:
    """The lines of the breakpoint table (kp_format_breakpoints; host only; no header: ``BREAKPOINTS_HEADER``): one per record of
    ``breakpoints`` (BREAKPOINT_DTYPE), assembly a's being ``bp_off[a]:bp_off[a + 1]``.  The name tables and ``kept`` are those of
    ``format_variants``; ``edge_tolerance`` (the typer's ``partial_edge_tolerance``) decides between contig_break and translocation."""
    breakpoints = np.ascontiguousarray(breakpoints, dtype=BREAKPOINT_DTYPE)
    n_asm = len(bp_off) - 1
    kept, stride = _kept_table(kept, n_asm)
    t, keep = _batch_names(gene_names, asm_names, contig_names, asm_first_ctg, n_asm)
    bp_off = _record_runs(bp_off, breakpoints)
    h = lib()
    h.kp_format_breakpoints.restype = C.c_int64
    return _sized("kp_format_breakpoints", 256 * len(breakpoints), lambda out, cap: h.kp_format_breakpoints(
        C.byref(t), C.c_int32(n_asm), _p(kept), C.c_int32(stride), _p(breakpoints), _p(bp_off), C.c_int32(int(edge_tolerance)), out, cap))


def format_rescue(gene_names, locus_names, asm_names, contig_names, asm_first_ctg, prot_len, best_locus, records, rescue_off,
                  min_score: int = RESCUE_MIN_SCORE) -> bytes:
    """The lines of the rescue table (kp_format_rescue; host only; no header: ``RESCUE_HEADER``): one per record of ``records``
    (RESCUE_DTYPE), assembly a's being ``rescue_off[a]:rescue_off[a + 1]``.  The name tables are those of ``format_alleles``;
    ``prot_len`` the database's protein lengths by gene (``Database.translations.lengths``); ``min_score`` decides between ``absent``
    and a call."""
    prot_len, best_locus = _c(prot_len, np.int32), _c(best_locus, np.int32)
    records = np.ascontiguousarray(records, dtype=RESCUE_DTYPE)
    n_asm = len(rescue_off) - 1
    t, keep = _batch_names(gene_names, asm_names, contig_names, asm_first_ctg, n_asm, locus_names, per_asm=(best_locus,), per_gene=(prot_len,))
    rescue_off = _record_runs(rescue_off, records)
    h = lib()
    h.kp_format_rescue.restype = C.c_int64
    return _sized("kp_format_rescue", 320 * len(records), lambda out, cap: h.kp_format_rescue(
        C.byref(t), C.c_int32(n_asm), _p(prot_len), _p(best_locus), _p(records), _p(rescue_off), C.c_int32(int(min_score)), out, cap))


def piece_order(pieces, n_pieces) -> np.ndarray:
    """int32 [n_asm, stride]: the order in which the product lists every assembly's locus pieces -- numpy's argsort of their mean
    positions (core.py:281), as ``kp_format_json`` is given it; entries beyond an assembly's pieces are their own index."""
    pieces = np.ascontiguousarray(pieces)
    n, stride = len(n_pieces), (pieces.shape[1] if pieces.ndim == 2 else 0)
    order = np.zeros((n, max(stride, 1)), np.int32)
    order[:] = np.arange(max(stride, 1), dtype=np.int32)[None, :]
    for a in np.flatnonzero(np.asarray(n_pieces) > 1):
        m = int(n_pieces[a])
        order[a, :m] = np.argsort(np.ascontiguousarray(pieces["mean_pos"][a, :m]))
    return order


def locus_alleles(piece_digests, order, n_pieces) -> np.ndarray:
    """uint64 [n_asm]: the locus digest of every assembly (kp_allele_locus_digest; include/kp_spec.h, ALLELES) from its pieces'
    digests ``piece_digests[a]`` taken in ``order[a]`` (``piece_order``); 0 for an assembly without a piece."""
    piece_digests, order = np.ascontiguousarray(piece_digests, np.uint64), np.ascontiguousarray(order, np.int32)
    h = lib()
    h.kp_allele_locus_digest.restype = C.c_uint64
    out = np.zeros(len(n_pieces), np.uint64)
    for a in np.flatnonzero(np.asarray(n_pieces) > 0):
        m = int(n_pieces[a])
        if m > piece_digests.shape[1] or m > order.shape[1]:
            raise ValueError("a summary counts more locus pieces than the digest table holds")
        out[a] = h.kp_allele_locus_digest(_p(piece_digests[a]), _p(order[a]), C.c_int32(m))
    return out


def format_alleles(gene_names, locus_names, asm_names, contig_names, asm_first_ctg, n_kept, n_pieces, best_locus, kept, alleles, piece_digests,
                   order) -> bytes:
    """The lines of the allele table (kp_format_alleles; host only; no header: ``ALLELES_HEADER``): one per kept record that is not
    spurious.  The name tables and ``kept`` are those of ``format_variants`` plus the loci's names; ``alleles`` (ALLELE_DTYPE, the
    shape of ``kept``) and ``piece_digests`` as ``Batch.alleles`` returns them, ``order`` as ``piece_order`` gives it."""
    n_kept, n_pieces, best_locus = _c(n_kept, np.int32), _c(n_pieces, np.int32), _c(best_locus, np.int32)
    alleles = np.ascontiguousarray(alleles, dtype=ALLELE_DTYPE)
    piece_digests, order = np.ascontiguousarray(piece_digests, np.uint64), np.ascontiguousarray(order, np.int32)
    n_asm = len(n_kept)
    kept, stride = _kept_table(kept, n_asm, alleles, " and alleles the records of Batch.alleles for it")
    t, keep = _batch_names(gene_names, asm_names, contig_names, asm_first_ctg, n_asm, locus_names, per_asm=(n_pieces, best_locus))
    pstride = piece_digests.shape[1] if piece_digests.ndim == 2 else 0
    if n_asm and (piece_digests.ndim != 2 or piece_digests.shape[0] != n_asm or order.ndim != 2 or order.shape[0] != n_asm or order.shape[1] < pstride):
        raise ValueError("piece digests and piece order must be [n_asm, stride] tables")
    if n_asm and order.shape[1] != pstride:
        order = np.ascontiguousarray(order[:, :pstride])
    h = lib()
    h.kp_format_alleles.restype = C.c_int64
    return _sized("kp_format_alleles", 256 * int(n_kept.sum()) if n_asm else 0, lambda out, cap: h.kp_format_alleles(
        C.byref(t), C.c_int32(n_asm), _p(n_kept), _p(n_pieces), _p(best_locus), _p(kept), _p(alleles), C.c_int32(stride), _p(piece_digests), _p(order),
        C.c_int32(pstride), out, cap))  # fmt: skip


def aligned_codes(row, blocks) -> np.ndarray:
    """uint8 [gene_len]: the columns of one aligned row (``row``: an ALIGNED_ROW_DTYPE record, ``blocks``: the batch's block array) as
    codes 0..3, 4 inside an N run and ``ALIGNED_GAP`` for GAP (include/kp_spec.h, ALIGNED ROWS)."""
    L, off = int(row["gene_len"]), int(row["off"])
    nb = (L + 15) // 16
    if L < 0 or off < 0 or off + nb > len(blocks):
        raise ValueError("the row runs outside the block array")
    v = np.ascontiguousarray(blocks[off:off + nb], np.uint64)[:, None]
    c = np.arange(16, dtype=np.uint64)[None, :]
    code = ((v >> (2 * c)) & np.uint64(3)).astype(np.uint8)
    code[((v >> (c + np.uint64(BLOCK_N_SHIFT))) & np.uint64(1)) != 0] = 4
    code[((v >> (c + np.uint64(BLOCK_GAP_SHIFT))) & np.uint64(1)) != 0] = ALIGNED_GAP
    return code.reshape(-1)[:L]


def format_aligned(gene_names, asm_names, contig_names, asm_first_ctg, n_kept, kept, rows, blocks) -> bytes:
    """The lines of the aligned table (kp_format_aligned; host only; no header: ``ALIGNED_HEADER``): one per kept record that is not
    spurious.  The name tables and ``kept`` are those of ``format_variants``; ``rows`` (ALIGNED_ROW_DTYPE, the shape of ``kept``) and
    ``blocks`` as ``Batch.aligned`` returns them."""
    n_kept = _c(n_kept, np.int32)
    rows = np.ascontiguousarray(rows, dtype=ALIGNED_ROW_DTYPE)
    blocks = np.ascontiguousarray(blocks, np.uint64)
    n_asm = len(n_kept)
    kept, stride = _kept_table(kept, n_asm, rows, " and rows the records of Batch.aligned for it")
    t, keep = _batch_names(gene_names, asm_names, contig_names, asm_first_ctg, n_asm)
    h = lib()
    h.kp_format_aligned.restype = C.c_int64
    return _sized("kp_format_aligned", 16 * len(blocks) + 256 * int(n_kept.sum()) if n_asm else 0, lambda out, cap: h.kp_format_aligned(
        C.byref(t), C.c_int32(n_asm), _p(n_kept), _p(kept), C.c_int32(stride), _p(rows), _p(blocks), C.c_int64(len(blocks)), out, cap))


def format_distances(locus_name: str, columns: int, names, pairs) -> bytes:
    """The lines of one locus's distance table (kp_format_distances; host only; no header: ``DISTANCES_HEADER``): one per record of
    ``pairs`` (DIST_PAIR_DTYPE), whose ``a`` and ``b`` index ``names``, the assemblies' names by row of the locus's matrix."""
    nm_b, nm_o = _blob64(names)
    pairs = np.ascontiguousarray(pairs, dtype=DIST_PAIR_DTYPE)
    locus = locus_name.encode("utf-8")
    h = lib()
    h.kp_format_distances.restype = C.c_int64
    return _sized("kp_format_distances", 96 * len(pairs), lambda out, cap: h.kp_format_distances(
        C.c_char_p(locus), C.c_int32(len(locus)), C.c_int64(int(columns)), _p(nm_b), _p(nm_o), C.c_int32(len(nm_o) - 1), _p(pairs), C.c_int64(len(pairs)), out, cap))  # fmt: skip


def format_clusters(locus_name: str, names, labels, nearest, rows=None) -> bytes:
    """The lines of one locus's cluster table (kp_format_clusters; host only; no header: ``clusters_header``): one per row of the
    locus's matrix.  ``labels`` int32 [K, R] and ``nearest`` (DIST_NEAREST_DTYPE [R]) as ``Distances.clusters`` returns them;
    ``names`` the R assemblies' names, by row -- or, with ``rows`` (int32 [R]), row i is ``names[rows[i]]``."""
    nm_b, nm_o = _blob64(names)
    nearest = np.ascontiguousarray(nearest, dtype=DIST_NEAREST_DTYPE)
    R = len(nearest)
    labels = np.ascontiguousarray(labels, np.int32).reshape(-1, R) if R else np.zeros((len(labels), 0), np.int32)
    if len(nm_o) - 1 != R or (rows is not None and len(rows) != R):
        raise ValueError("a name, a nearest record and a label per level for every row")
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    locus = locus_name.encode("utf-8")
    h = lib()
    h.kp_format_clusters.restype = C.c_int64
    return _sized("kp_format_clusters", 96 * R, lambda out, cap: h.kp_format_clusters(
        C.c_char_p(locus), C.c_int32(len(locus)), _p(nm_b), _p(nm_o), C.c_int32(R), None if rows is None else _p(rows), C.c_int32(labels.shape[0]), _p(labels),
        _p(nearest), out, cap))  # fmt: skip


def format_newick(locus_name: str, names, edges, component, rows=None) -> bytes:
    """The lines of one locus's Newick table (kp_format_newick; host only; no header: ``newick_header``): one per tree of the forest,
    ascending in the tree's smallest row.  ``edges`` (DIST_PAIR_DTYPE [E]) and ``component`` (int32 [R]) as ``Distances.tree``
    returns them; ``names`` the R assemblies' names, by row -- or, with ``rows`` (int32 [R]), row i is ``names[rows[i]]``."""
    nm_b, nm_o = _blob64(names)
    edges = np.ascontiguousarray(edges, dtype=DIST_PAIR_DTYPE)
    component = np.ascontiguousarray(component, np.int32)
    R = len(component)
    if len(nm_o) - 1 != R or (rows is not None and len(rows) != R):
        raise ValueError("a name and a component for every row")
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    locus = locus_name.encode("utf-8")
    h = lib()
    h.kp_format_newick.restype = C.c_int64
    return _sized("kp_format_newick", 64 * R + len(nm_b) + 64, lambda out, cap: h.kp_format_newick(
        C.c_char_p(locus), C.c_int32(len(locus)), _p(nm_b), _p(nm_o), C.c_int32(R), None if rows is None else _p(rows), _p(edges), C.c_int64(len(edges)),
        _p(component), out, cap))  # fmt: skip


def format_nj(locus_name: str, names, taxa, nodes, rows=None) -> bytes:
    """The line of one locus's neighbour-joining table (kp_format_nj; host only; no header: ``nj_header``), or nothing for fewer
    than two taxa.  ``taxa`` (int32 [n]) and ``nodes`` (NJ_NODE_DTYPE) as ``Distances.nj`` returns them; ``names`` the R assemblies'
    names, by row of the matrix -- or, with ``rows`` (int32 [R]), row i is ``names[rows[i]]``."""
    nm_b, nm_o = _blob64(names)
    taxa = np.ascontiguousarray(taxa, np.int32)
    nodes = np.ascontiguousarray(nodes, dtype=NJ_NODE_DTYPE)
    R = len(nm_o) - 1
    if rows is not None and len(rows) != R:
        raise ValueError("a name for every row")
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    locus = locus_name.encode("utf-8")
    h = lib()
    h.kp_format_nj.restype = C.c_int64
    return _sized("kp_format_nj", 48 * len(taxa) + len(nm_b) + len(locus) + 64, lambda out, cap: h.kp_format_nj(
        C.c_char_p(locus), C.c_int32(len(locus)), _p(nm_b), _p(nm_o), C.c_int32(R), None if rows is None else _p(rows), _p(taxa) if len(taxa) else None,
        C.c_int32(len(taxa)), _p(nodes) if len(nodes) else None, C.c_int64(len(nodes)), out, cap))  # fmt: skip


def format_nj_support(locus_name: str, names, taxa, nodes, support, replicates: int, rows=None) -> bytes:
    """``format_nj``'s line with support values (kp_format_nj_support; host only; no header: ``nj_support_header``): a Replicates
    column before the Newick text, in which the node of every record with an inner edge is labelled with its ``support`` (int32, one
    per record, as ``Distances.nj_support`` returns it), a count out of ``replicates``."""
    nm_b, nm_o = _blob64(names)
    taxa = np.ascontiguousarray(taxa, np.int32)
    nodes = np.ascontiguousarray(nodes, dtype=NJ_NODE_DTYPE)
    support = np.ascontiguousarray(support, np.int32)
    R = len(nm_o) - 1
    if (rows is not None and len(rows) != R) or len(support) != len(nodes):
        raise ValueError("a name for every row and a support value for every record")
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    locus = locus_name.encode("utf-8")
    h = lib()
    h.kp_format_nj_support.restype = C.c_int64
    return _sized("kp_format_nj_support", 60 * len(taxa) + len(nm_b) + len(locus) + 80, lambda out, cap: h.kp_format_nj_support(
        C.c_char_p(locus), C.c_int32(len(locus)), _p(nm_b), _p(nm_o), C.c_int32(R), None if rows is None else _p(rows), _p(taxa) if len(taxa) else None,
        C.c_int32(len(taxa)), _p(nodes) if len(nodes) else None, C.c_int64(len(nodes)), _p(support) if len(support) else None, C.c_int32(int(replicates)), out, cap))  # fmt: skip


def format_nj_transfer(locus_name: str, names, taxa, nodes, transfer, replicates: int, rows=None) -> bytes:
    """``format_nj_support``'s line, the same five columns, with transfer support (kp_format_nj_transfer; include/kp_spec.h,
    TRANSFER): the node of every record with an inner edge is labelled with ``1 - transfer / (replicates * (depth - 1))`` in
    thousandths, three decimals -- ``transfer`` (int64, one per record) as ``Distances.nj_transfer`` returns it."""
    nm_b, nm_o = _blob64(names)
    taxa = np.ascontiguousarray(taxa, np.int32)
    nodes = np.ascontiguousarray(nodes, dtype=NJ_NODE_DTYPE)
    transfer = np.ascontiguousarray(transfer, np.int64)
    R = len(nm_o) - 1
    if (rows is not None and len(rows) != R) or len(transfer) != len(nodes):
        raise ValueError("a name for every row and a transfer sum for every record")
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    locus = locus_name.encode("utf-8")
    h = lib()
    h.kp_format_nj_transfer.restype = C.c_int64
    return _sized("kp_format_nj_transfer", 60 * len(taxa) + len(nm_b) + len(locus) + 80, lambda out, cap: h.kp_format_nj_transfer(
        C.c_char_p(locus), C.c_int32(len(locus)), _p(nm_b), _p(nm_o), C.c_int32(R), None if rows is None else _p(rows), _p(taxa) if len(taxa) else None,
        C.c_int32(len(taxa)), _p(nodes) if len(nodes) else None, C.c_int64(len(nodes)), _p(transfer) if len(transfer) else None, C.c_int32(int(replicates)), out, cap))  # fmt: skip


def format_sites(locus_name: str, gene_names, gene_lengths, n_rows: int, sites, genes=None) -> bytes:
    """The lines of one locus's site table (kp_format_sites; host only; no header: ``SITES_HEADER``): one per record of ``sites``
    (SITE_DTYPE, as ``Distances.sites`` returns them).  ``gene_names`` and ``gene_lengths``: the locus's genes in database order --
    or, with ``genes`` (int32, one entry per gene), gene i is named ``gene_names[genes[i]]``; ``n_rows`` the rows of the matrix."""
    nm_b, nm_o = _blob64(gene_names)
    lens = np.ascontiguousarray(gene_lengths, np.int32)
    if len(nm_o) - 1 != len(lens) or (genes is not None and len(genes) != len(lens)):
        raise ValueError("a name and a length for every gene")
    genes = None if genes is None else np.ascontiguousarray(genes, np.int32)
    sites = np.ascontiguousarray(sites, dtype=SITE_DTYPE)
    locus = locus_name.encode("utf-8")
    h = lib()
    h.kp_format_sites.restype = C.c_int64
    return _sized("kp_format_sites", 128 * len(sites), lambda out, cap: h.kp_format_sites(
        C.c_char_p(locus), C.c_int32(len(locus)), _p(nm_b), _p(nm_o), C.c_int32(len(lens)), None if genes is None else _p(genes), _p(lens), C.c_int32(int(n_rows)),
        _p(sites), C.c_int64(len(sites)), out, cap))  # fmt: skip


def format_site_rows(locus_name: str, names, n_sites: int, blocks, rows=None) -> bytes:
    """The lines of one locus's SNP alignment (kp_format_site_rows; host only; no header: ``SNP_ALIGNMENT_HEADER``): one per row of
    the locus's matrix, none when ``n_sites`` is 0.  ``blocks`` uint64 [R, (n_sites + 15) // 16] as ``Distances.site_rows`` returns
    them; ``names`` the R assemblies' names, by row -- or, with ``rows`` (int32 [R]), row i is ``names[rows[i]]``."""
    nm_b, nm_o = _blob64(names)
    R, S = len(nm_o) - 1, int(n_sites)
    if S < 0 or (rows is not None and len(rows) != R):
        raise ValueError("a name for every row and no negative number of sites")
    blocks = np.ascontiguousarray(blocks, np.uint64).reshape(R, -1) if R else np.zeros((0, (S + 15) // 16), np.uint64)
    if blocks.shape[1] != (S + 15) // 16:
        raise ValueError("site rows of (n_sites + 15) // 16 blocks for every row")
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    locus = locus_name.encode("utf-8")
    h = lib()
    h.kp_format_site_rows.restype = C.c_int64
    return _sized("kp_format_site_rows", R * (S + 64) + len(nm_b), lambda out, cap: h.kp_format_site_rows(
        C.c_char_p(locus), C.c_int32(len(locus)), _p(nm_b), _p(nm_o), C.c_int32(R), None if rows is None else _p(rows), C.c_int64(S), _p(blocks), out, cap))  # fmt: skip


def _gene_table(gene_names, gene_lengths, genes):
    """(name blob, offsets, int32 lengths, int32 mapping or None) of a locus's genes, as the site formatters take them."""
    nm_b, nm_o = _blob64(gene_names)
    lens = np.ascontiguousarray(gene_lengths, np.int32)
    if len(nm_o) - 1 != len(lens) or (genes is not None and len(genes) != len(lens)):
        raise ValueError("a name and a length for every gene")
    return nm_b, nm_o, lens, None if genes is None else np.ascontiguousarray(genes, np.int32)


def format_nj_homoplasy(locus_name: str, gene_names, gene_lengths, sites, genes=None) -> bytes:
    """The lines of one locus's homoplasy table (kp_format_nj_homoplasy; host only; no header: ``nj_homoplasy_header``): one per
    record of ``sites`` (PARS_SITE_DTYPE, as ``Distances.nj_parsimony`` returns them) -- the column's gene and position as
    ``format_sites`` names them, the bases that occur, the changes the tree needs and how many of them are beyond one per further
    base.  ``gene_names``, ``gene_lengths`` and ``genes`` as ``format_sites`` takes them."""
    nm_b, nm_o, lens, genes = _gene_table(gene_names, gene_lengths, genes)
    sites = np.ascontiguousarray(sites, dtype=PARS_SITE_DTYPE)
    locus = locus_name.encode("utf-8")
    h = lib()
    h.kp_format_nj_homoplasy.restype = C.c_int64
    return _sized("kp_format_nj_homoplasy", 96 * len(sites), lambda out, cap: h.kp_format_nj_homoplasy(
        C.c_char_p(locus), C.c_int32(len(locus)), _p(nm_b), _p(nm_o), C.c_int32(len(lens)), None if genes is None else _p(genes), _p(lens),
        _p(sites) if len(sites) else None, C.c_int64(len(sites)), out, cap))  # fmt: skip


def format_nj_changes(locus_name: str, names, taxa, nodes, gene_names, gene_lengths, changes, rows=None, genes=None) -> bytes:
    """The lines of one locus's change table (kp_format_nj_changes; host only; no header: ``nj_changes_header``): one per record of
    ``changes`` (PARS_CHANGE_DTYPE, as ``Distances.nj_parsimony`` returns them) -- the branch by its child end, a leaf by its
    assembly's name, an inner node as ``#t`` with the two tips it is the last common ancestor of when the tree is read from its last
    record, the column's gene and position, and the base on either end.  ``names``, ``taxa``, ``nodes`` and ``rows`` as
    ``format_nj`` takes them; the genes as ``format_sites`` does."""
    nm_b, nm_o = _blob64(names)
    g_b, g_o, lens, genes = _gene_table(gene_names, gene_lengths, genes)
    taxa = np.ascontiguousarray(taxa, np.int32)
    nodes = np.ascontiguousarray(nodes, dtype=NJ_NODE_DTYPE)
    changes = np.ascontiguousarray(changes, dtype=PARS_CHANGE_DTYPE)
    R = len(nm_o) - 1
    if rows is not None and len(rows) != R:
        raise ValueError("a name for every row")
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    locus = locus_name.encode("utf-8")
    h = lib()
    h.kp_format_nj_changes.restype = C.c_int64
    return _sized("kp_format_nj_changes", 160 * len(changes), lambda out, cap: h.kp_format_nj_changes(
        C.c_char_p(locus), C.c_int32(len(locus)), _p(nm_b), _p(nm_o), C.c_int32(R), None if rows is None else _p(rows), _p(taxa) if len(taxa) else None,
        C.c_int32(len(taxa)), _p(nodes) if len(nodes) else None, C.c_int64(len(nodes)), _p(g_b), _p(g_o), C.c_int32(len(lens)), None if genes is None else _p(genes), _p(lens),
        _p(changes) if len(changes) else None, C.c_int64(len(changes)), out, cap))  # fmt: skip


class JsonTables(C.Structure):  # kp_json_tables
    _fields_ = [("head", C.c_char_p), ("head_len", C.c_int32), ("gene_names", C.c_void_p), ("gene_name_off", C.c_void_p),
                ("gene_ids", C.c_void_p), ("cluster_names", C.c_void_p), ("products", C.c_void_p), ("gene_id_off", C.c_void_p),
                ("cluster_name_off", C.c_void_p), ("product_off", C.c_void_p), ("locus_names", C.c_void_p),
                ("locus_name_off", C.c_void_p), ("locus_gene_off", C.c_void_p), ("locus_gene_len", C.c_void_p),
                ("gene_position", C.c_void_p), ("gene_strand", C.c_void_p), ("comp_map", C.c_void_p), ("char_map", C.c_void_p),
                ("codon_map", C.c_void_p), ("n_loci", C.c_int32), ("n_genes", C.c_int32)]  # fmt: skip


class JsonColumns(C.Structure):  # kp_json_columns
    _fields_ = [("asm_ids", C.c_void_p), ("asm_id_off", C.c_void_p), ("phenotypes", C.c_void_p), ("phenotype_off", C.c_void_p),
                ("best_locus", C.c_void_p), ("typeable", C.c_void_p), ("problems", C.c_void_p), ("best_score", C.c_void_p),
                ("completeness", C.c_void_p), ("identity", C.c_void_p), ("coverage", C.c_void_p), ("length_discrepancy", C.c_void_p),
                ("piece_order", C.c_void_p), ("piece_ctg_names", C.c_void_p), ("piece_ctg_name_off", C.c_void_p),
                ("ctg_seqs", C.c_void_p), ("ctg_off", C.c_void_p), ("n_ctg", C.c_void_p), ("ctg_text_len", C.c_void_p)]  # fmt: skip


def _blob64(strings) -> tuple[np.ndarray, np.ndarray]:
    """utf-8 strings -> (bytes back to back, n + 1 int64 offsets)."""
    enc = [s if isinstance(s, bytes) else str(s).encode("utf-8") for s in strings]
    off = np.zeros(len(enc) + 1, np.int64)
    if enc:
        np.cumsum([len(e) for e in enc], out=off[1:])
    return np.frombuffer(b"".join(enc) or b"\0", np.uint8), off


class JsonFormatter:
    """The JSON lines of whole batches (kp_format_json): what ``dumps_line(result.to_dict())`` writes per assembly
    (kaptive_amd/serotyping/jsonl.py), without an object per assembly.  The database's strings are escaped once."""

    def __init__(self, typer, kaptive_version: str) -> None:
        from kaptive_amd.core.seq import CHAR_MAP, CODON_MAP, COMP_MAP
        from kaptive_amd.serotyping.jsonl import _str

        db = typer._db
        self._typer_gene_ids = tuple(db.genes.ids)
        meta = db.metadata
        head = ("{" + f'"kaptive_version":{_str(kaptive_version)},"database_name":{_str(meta.name)},"database_version":{_str(meta.version)},'
                f'"database_organism":{_str(meta.organism)},"database_taxon":{int(meta.taxon)},"genome":').encode("utf-8")
        text = lambda col: [_str(v.decode("utf-8", "replace")) for v in col.tolist()]  # noqa: E731  (GeneHits.to_dict decodes the truncated bytes)
        self._keep = dict(
            head=head, gene_names=_blob64([_str(x) for x in db.genes.ids]), gene_ids=_blob64(text(typer._gene_ids_s32)),
            cluster=_blob64(text(typer._cluster_s10)), product=_blob64(text(typer._product_s64)),
            locus=_blob64([_str(x) for x in db.loci.ids]),
            locus_gene_off=_c(db.locus_gene_offsets, np.int32), locus_gene_len=_c(db.locus_gene_lengths, np.int32),
            gene_position=_c(db.gene_positions, np.int32), gene_strand=_c(db.gene_intervals.strands, np.int8),
            comp=_c(COMP_MAP, np.uint8), char=_c(CHAR_MAP, np.uint8), codon=_c(CODON_MAP, np.uint8),
        )  # fmt: skip
        k = self._keep
        self._tables = JsonTables(
            head=head, head_len=len(head), gene_names=_p(k["gene_names"][0]).value, gene_name_off=_p(k["gene_names"][1]).value,
            gene_ids=_p(k["gene_ids"][0]).value, cluster_names=_p(k["cluster"][0]).value, products=_p(k["product"][0]).value,
            gene_id_off=_p(k["gene_ids"][1]).value, cluster_name_off=_p(k["cluster"][1]).value, product_off=_p(k["product"][1]).value,
            locus_names=_p(k["locus"][0]).value, locus_name_off=_p(k["locus"][1]).value,
            locus_gene_off=_p(k["locus_gene_off"]).value, locus_gene_len=_p(k["locus_gene_len"]).value,
            gene_position=_p(k["gene_position"]).value, gene_strand=_p(k["gene_strand"]).value, comp_map=_p(k["comp"]).value,
            char_map=_p(k["char"]).value, codon_map=_p(k["codon"]).value, n_loci=len(db.loci.ids), n_genes=len(db.genes.ids),
        )  # fmt: skip

    def _prepare(self, ids, phenotypes, sums, kept, pieces, best_locus, best_score, completeness, typeable, problems, identity,
                 coverage, discrepancy, genomes) -> dict:
        """The batch's columns as kp_json_columns (and everything that must stay alive while the library reads them)."""
        from kaptive_amd.serotyping.jsonl import _str

        n = len(sums)
        sums, kept, pieces = np.ascontiguousarray(sums), np.ascontiguousarray(kept), np.ascontiguousarray(pieces)
        kstride = kept.shape[1] if kept.ndim == 2 else 0
        pstride = pieces.shape[1] if pieces.ndim == 2 else 0
        # order of the locus pieces: numpy's argsort of their mean positions (core.py:281), per assembly; names of their contigs
        order = np.zeros((n, max(pstride, 1)), np.int32)
        order[:] = np.arange(max(pstride, 1), dtype=np.int32)[None, :]
        names = [b""] * (n * pstride)
        raw_names = [b""] * (n * pstride)
        n_pieces = sums["n_pieces"]
        if n and (int(n_pieces.min()) < 0 or int(n_pieces.max()) > pstride):
            raise ValueError("kp_format_json: a summary counts more locus pieces than the piece table holds")
        for a in np.flatnonzero(n_pieces > 0):
            m = int(n_pieces[a])
            if m > 1:
                order[a, :m] = np.argsort(np.ascontiguousarray(pieces["mean_pos"][a, :m]))
            cids = genomes[a].contigs.ids
            for p_ in range(m):
                ci = int(pieces["contig"][a, p_])
                if not 0 <= ci < len(cids):
                    raise ValueError("kp_format_json: a locus piece names a contig the assembly does not have")
                cid = cids[ci]
                names[a * pstride + p_] = _str(cid)[1:-1].encode("utf-8")
                raw_names[a * pstride + p_] = cid.encode()
        ids_b, ids_o = _blob64([_str(x) for x in ids])
        ph_b, ph_o = _blob64([_str(x) for x in phenotypes])
        nm_b, nm_o = _blob64(names)
        seq_arrays = [np.ascontiguousarray(g.contigs.seqs, dtype=np.uint8) for g in genomes]
        off_arrays = [np.ascontiguousarray(g.contigs.offsets, dtype=np.int32) for g in genomes]
        seq_ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in seq_arrays])
        off_ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in off_arrays])
        n_ctg = np.array([len(o) for o in off_arrays], np.int32)
        text_len = np.array([len(a) for a in seq_arrays], np.int64)
        cols = dict(n_ctg=n_ctg, text_len=text_len, best=_c(best_locus, np.int32), typeable=_c(typeable, np.uint8), problems=_c(problems, np.int32),
                    score=_c(best_score, np.float64), compl=_c(completeness, np.float64), identity=_c(identity, np.float64),
                    coverage=_c(coverage, np.float64), discrepancy=_c(discrepancy, np.float64), order=order)  # fmt: skip
        c = JsonColumns(asm_ids=_p(ids_b).value, asm_id_off=_p(ids_o).value, phenotypes=_p(ph_b).value, phenotype_off=_p(ph_o).value,
                        best_locus=_p(cols["best"]).value, typeable=_p(cols["typeable"]).value, problems=_p(cols["problems"]).value,
                        best_score=_p(cols["score"]).value, completeness=_p(cols["compl"]).value, identity=_p(cols["identity"]).value,
                        coverage=_p(cols["coverage"]).value, length_discrepancy=_p(cols["discrepancy"]).value,
                        piece_order=_p(order).value, piece_ctg_names=_p(nm_b).value, piece_ctg_name_off=_p(nm_o).value,
                        ctg_seqs=C.cast(seq_ptrs, C.c_void_p).value, ctg_off=C.cast(off_ptrs, C.c_void_p).value,
                        n_ctg=_p(n_ctg).value, ctg_text_len=_p(text_len).value)  # fmt: skip
        return dict(n=n, sums=sums, kept=kept, pieces=pieces, kstride=kstride, pstride=pstride, c=c, raw_piece_names=raw_names,
                    keep=(ids_b, ids_o, ph_b, ph_o, nm_b, nm_o, seq_arrays, off_arrays, seq_ptrs, off_ptrs, cols))

    def format(self, *columns) -> bytes:
        """``columns``: ids, phenotypes, sums, kept, pieces, best_locus, best_score, completeness, typeable, problems, identity,
        coverage, length discrepancy, genomes (the attributes of a ``BatchTyping``)."""
        if len(columns[2]) == 0:
            return b""
        q = self._prepare(*columns)
        h = lib()
        h.kp_format_json.restype = C.c_int64
        return _sized("kp_format_json", max(1 << 16, 80_000 * q["n"]), lambda out, cap: h.kp_format_json(
            C.byref(self._tables), C.c_int32(q["n"]), _p(q["sums"]), _p(q["kept"]), C.c_int32(q["kstride"]), _p(q["pieces"]), C.c_int32(q["pstride"]),
            C.byref(q["c"]), out, cap))

    def fasta(self, kinds, *columns) -> dict:
        """Per-assembly FASTA bytes (kp_format_fasta) for every kind asked for -- "loci", "genes", "proteins": what
        ``result.locus_seqs / gene_seqs / translations .to_fasta()`` give per result -- as ``{kind: [bytes per assembly]}``."""
        n = len(columns[2])
        if n == 0:
            return {kind: [] for kind in kinds}
        q = self._prepare(*columns)
        if "gene_names_raw" not in self._keep:
            self._keep["gene_names_raw"] = _blob64([x.encode() for x in self._typer_gene_ids])
        piece_b, piece_o = _blob64(q["raw_piece_names"])
        h = lib()
        h.kp_format_fasta.restype = C.c_int64
        out = {}
        for kind in kinds:
            code = {"loci": 0, "genes": 1, "proteins": 2}[kind]
            nb, no = (piece_b, piece_o) if code == 0 else self._keep["gene_names_raw"]
            ends = np.zeros(n, np.int64)  # (filled by the call that fits)
            blob = _sized("kp_format_fasta", max(1 << 16, (40_000 if code < 2 else 12_000) * n), lambda out, cap: h.kp_format_fasta(
                C.byref(self._tables), C.c_int32(n), _p(q["sums"]), _p(q["kept"]), C.c_int32(q["kstride"]), _p(q["pieces"]), C.c_int32(q["pstride"]),
                C.byref(q["c"]), C.c_int32(code), _p(nb), _p(no), out, cap, _p(ends)))
            starts = np.concatenate([[0], ends[:-1]])
            out[kind] = [blob[int(a):int(b)] for a, b in zip(starts, ends)]
        return out


class TypingParams(C.Structure):  # kp_typing_params
    _fields_ = [("min_gene_coverage", C.c_double), ("id_threshold", C.c_float), ("max_locus_length", C.c_int32),
                ("edge_tolerance", C.c_int32)]  # fmt: skip

_lib = None
_lock = threading.Lock()
_live: "weakref.WeakSet" = weakref.WeakSet()  # contexts and batches still holding device memory


@atexit.register
def _close_all() -> None:
    """Release device objects before the HIP runtime's own exit handlers run (batches first, then contexts)."""
    objs = list(_live)
    for o in sorted(objs, key=lambda x: isinstance(x, Context)):
        try:
            o.close()
        except Exception:
            pass


class NativeError(RuntimeError):
    pass


def is_loaded() -> bool:
    """Whether the shared library (and with it the HIP runtime) has been loaded into this process."""
    return _lib is not None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not LIB_PATH.exists():
                    raise NativeError(
                        f"{LIB_PATH} is missing: build it with `python -m kaptive_amd.build` (hipcc, gfx950). "
                        "kaptive_amd has no CPU fallback."
                    )
                # The HIP runtime reads GPU_MAX_HW_QUEUES when it initialises, i.e. when the library below pulls it in: a
                # context drives a dozen streams and the default of 4 hardware queues costs a host-fed stream a fifth of
                # its throughput (kaptive_amd.tune_runtime).  Library users who never call an entry point get it here;
                # an explicit setting in the environment wins.
                os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
                h = C.CDLL(str(LIB_PATH))
                h.kp_last_error.restype = C.c_char_p
                h.kp_ctx_stream.restype = C.c_void_p
                for f in ("kp_db_n_postings", "kp_batch_anchors", "kp_batch_tasks", "kp_batch_task_results", "kp_batch_joins", "kp_batch_occ", "kp_batch_candidates"):
                    getattr(h, f).restype = C.c_int64
                h.kp_ctx_destroy.restype = None
                h.kp_batch_destroy.restype = None
                h.kp_dist_destroy.restype = None
                h.kp_dist_tree_rounds.restype = C.c_int32
                h.kp_batch_device_words.restype = C.c_void_p
                h.kp_host_free.restype = None
                h.kp_host_free.argtypes = [C.c_void_p]
                h.kp_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
                h.kp_host_reserve.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
                h.kp_host_lock.argtypes = [C.c_void_p]
                _lib = h
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _c(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


class Context:
    """One GPU + stream + resident database (kp_ctx)."""

    def __init__(self, device: int = 0) -> None:
        self._h = C.c_void_p()
        rc = lib().kp_ctx_create(C.c_int(device), C.byref(self._h))
        if rc != 0:
            raise NativeError(f"kp_ctx_create failed ({rc}): {lib().kp_last_error(None).decode()}")
        self.device = device
        self.group_loci: dict[int, int] = {}  # loci of every typing group's database (shapes of the score arrays)
        self._batches: "weakref.WeakSet" = weakref.WeakSet()
        _live.add(self)

    def close(self) -> None:
        if getattr(self, "_h", None):
            for b in list(self._batches):  # a batch must not outlive its context
                b.close()
            lib().kp_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc: int, what: str) -> None:
        if rc < 0:
            msg = lib().kp_last_error(self._h).decode()
            raise (ValueError if rc == -1 else NativeError)(f"{what} failed ({rc}): {msg}")

    @property
    def stream(self) -> int:
        return int(lib().kp_ctx_stream(self._h) or 0)

    def set_option(self, name: str, value: int) -> None:
        """Tuning knob of the context (kp_ctx_set_option; names in include/kaptive_amd.h)."""
        self._check(lib().kp_ctx_set_option(self._h, name.encode(), C.c_int64(int(value))), "kp_ctx_set_option")

    def load_genes(self, gene_codes: np.ndarray, gene_off: np.ndarray) -> None:
        codes, off = _c(gene_codes, np.uint8), _c(gene_off, np.int32)
        self._check(lib().kp_db_load(self._h, _p(codes), _p(off), C.c_int32(len(off) - 1)), "kp_db_load")

    def load_typing(self, db, group: int = 0, gene_lo: int = 0, gene_hi: int | None = None) -> None:
        """Upload the Database columns the batched reduction reads (kp_db_load_typing / kp_db_load_typing_group).  With
        several databases in one context, ``db``'s genes are ``[gene_lo, gene_hi)`` of the genes given to
        ``load_genes``."""
        prot = db.translations
        keep = dict(
            gene_locus=_c(db.gene_locus_indices, np.uint16), gene_extra=_c(db.extra_genes, np.uint8),
            gene_pos=_c(db.gene_positions, np.uint16), gene_strand=_c(db.gene_intervals.strands, np.int8),
            locus_gene_off=_c(db.locus_gene_offsets, np.int32), locus_gene_len=_c(db.locus_gene_lengths, np.int32),
            prot=_c(prot.seqs, np.uint8), prot_off=_c(prot.offsets, np.int32), prot_len=_c(prot.lengths, np.int32),
        )  # fmt: skip
        t = TypingTables(n_loci=len(db.loci), **{k: _p(v).value for k, v in keep.items()})
        gene_hi = gene_lo + len(db.genes) if gene_hi is None else gene_hi
        self._check(
            lib().kp_db_load_typing_group(self._h, C.c_int32(group), C.c_int32(gene_lo), C.c_int32(gene_hi), C.byref(t)),
            "kp_db_load_typing_group",
        )
        self.group_loci[group] = len(db.loci)
        if group == 0:
            self.n_loci = len(db.loci)

    @property
    def n_postings(self) -> int:
        return int(lib().kp_db_n_postings(self._h))

    def protein_align(self, q, q_off, q_len, t, t_off, t_len) -> np.ndarray:
        n = len(q_off)
        out = np.zeros((n, 8), np.int32)
        if n:
            q, t = _c(q, np.uint8), _c(t, np.uint8)
            self._check(
                lib().kp_protein_align(self._h, _p(q), _p(_c(q_off, np.int32)), _p(_c(q_len, np.int32)), _p(t),
                                       _p(_c(t_off, np.int32)), _p(_c(t_len, np.int32)), C.c_int32(n), _p(out)),
                "kp_protein_align",
            )  # fmt: skip
        return out

    def protein_align_seeded(self, q, q_off, q_len, t, t_off, t_len, offsets, k: int) -> np.ndarray:
        """Seeded mode (kp_protein_align_seeded): band ``k`` around the diagonal ``offsets[p]`` of every pair."""
        n = len(q_off)
        out = np.zeros((n, 8), np.int32)
        if n:
            q, t = _c(q, np.uint8), _c(t, np.uint8)
            self._check(
                lib().kp_protein_align_seeded(self._h, _p(q), _p(_c(q_off, np.int32)), _p(_c(q_len, np.int32)), _p(t),
                                              _p(_c(t_off, np.int32)), _p(_c(t_len, np.int32)), C.c_int32(n),
                                              _p(_c(offsets, np.int32)), C.c_int32(int(k)), _p(out)),
                "kp_protein_align_seeded",
            )  # fmt: skip
        return out

    def batch(self, packed: list, device_words: int | None = None, pinned_words: "np.ndarray | None" = None,
              after: "Batch | None" = None, tables: "tuple | None" = None) -> "Batch":
        return Batch(self, packed, device_words, pinned_words, after, tables)


class Batch:
    """Packed assemblies resident on the device (kp_batch). ``packed`` is a list of PackedAssembly; with
    ``device_words`` (a device pointer to the concatenated words) nothing but the small tables is copied."""

    def __init__(self, ctx: Context, packed: "list | None", device_words: int | None = None,
                 pinned_words: "np.ndarray | None" = None, after: "Batch | None" = None, tables: "tuple | None" = None) -> None:
        """``after``: the batch (of another context on the same GPU) whose device words this one adopts while their
        upload may still be in flight.  ``pinned_words``: the concatenated words of ``packed`` in page-locked memory (``pinned_array``); the upload
        is then enqueued asynchronously (kp_batch_create_async) and the array must stay alive until ``upload_wait`` or
        the first ``wait``/``score`` of the batch.  ``tables`` (instead of ``packed``): the batch's tables as they go to
        the library -- ``FastaShard.tables()`` -- next to ``pinned_words`` or ``device_words``."""
        self.ctx = ctx

        def cat(xs, dt):
            return np.ascontiguousarray(np.concatenate(xs), dtype=dt) if xs else np.empty(0, dt)

        if tables is not None:
            if packed is not None or (pinned_words is None and device_words is None):
                raise ValueError("tables come with pinned_words or device_words, not with packed assemblies")
            word_off, ctg_start, ctg_len, first_ctg, n_runs, first_run = tables
            self.n_asm = len(word_off) - 1
        else:
            self.n_asm = len(packed)
            word_off = np.zeros(self.n_asm + 1, np.int64)
            first_ctg = np.zeros(self.n_asm + 1, np.int32)
            first_run = np.zeros(self.n_asm + 1, np.int32)
            for i, pa in enumerate(packed):
                word_off[i + 1] = word_off[i] + pa.padded_len // 16
                first_ctg[i + 1] = first_ctg[i] + len(pa.ctg_start)
                first_run[i + 1] = first_run[i] + len(pa.n_runs)
            ctg_start = cat([pa.ctg_start for pa in packed], np.int32)
            ctg_len = cat([pa.ctg_len for pa in packed], np.int32)
            n_runs = cat([pa.n_runs.reshape(-1) for pa in packed], np.int32)
        self._h = C.c_void_p()
        self._pinned = pinned_words
        if pinned_words is not None:
            if pinned_words.dtype != np.uint32 or len(pinned_words) != int(word_off[-1]):
                raise ValueError("pinned_words must be the uint32 concatenation of the packed assemblies' words")
            rc = lib().kp_batch_create_async(ctx._h, C.c_int32(self.n_asm), _p(pinned_words), _p(word_off), _p(ctg_start),
                                             _p(ctg_len), _p(first_ctg), _p(n_runs), _p(first_run), C.byref(self._h))  # fmt: skip
        elif device_words is None:
            words = cat([pa.words for pa in packed], np.uint32)
            rc = lib().kp_batch_create(ctx._h, C.c_int32(self.n_asm), _p(words), _p(word_off), _p(ctg_start),
                                       _p(ctg_len), _p(first_ctg), _p(n_runs), _p(first_run), C.byref(self._h))  # fmt: skip
        else:
            rc = lib().kp_batch_create_device(ctx._h, C.c_int32(self.n_asm), C.c_void_p(device_words), _p(word_off),
                                              _p(ctg_start), _p(ctg_len), _p(first_ctg), _p(n_runs), _p(first_run),
                                              C.byref(self._h))  # fmt: skip
        ctx._check(rc, "kp_batch_create")
        self._after = after
        if after is not None:
            ctx._check(lib().kp_batch_depends_on(ctx._h, self._h, after._h), "kp_batch_depends_on")
        self.total_words = int(word_off[-1])
        ctx._batches.add(self)
        _live.add(self)

    def close(self) -> None:
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):  # the context owns the device; without it there is nothing to free
                lib().kp_batch_destroy(self._h)
            self._h = None

    __del__ = close

    @property
    def device_words(self) -> int:
        """Device address of the packed words (kp_batch_device_words); another context's batch can adopt them."""
        return int(lib().kp_batch_device_words(self._h) or 0)

    def upload_wait(self) -> None:
        self.ctx._check(lib().kp_batch_upload_wait(self.ctx._h, self._h), "kp_batch_upload_wait")

    def align_async(self) -> None:
        self.ctx._check(lib().kp_batch_align(self.ctx._h, self._h), "kp_batch_align")

    def wait(self) -> None:
        self.ctx._check(lib().kp_batch_wait(self.ctx._h, self._h), "kp_batch_wait")

    def align(self) -> tuple[np.ndarray, np.ndarray]:
        """Run the aligner; returns (hits [HIT_DTYPE], hit_off [n_asm + 1])."""
        self.align_async()
        self.wait()
        return self.hits()

    def hits(self) -> tuple[np.ndarray, np.ndarray]:
        off = np.zeros(self.n_asm + 1, np.int64)
        self.ctx._check(lib().kp_batch_hit_offsets(self.ctx._h, self._h, _p(off)), "kp_batch_hit_offsets")
        out = np.zeros(int(off[-1]), HIT_DTYPE)
        self.ctx._check(lib().kp_batch_hits(self.ctx._h, self._h, _p(out), C.c_int64(len(out))), "kp_batch_hits")
        return out, off

    def set_hits(self, hits: np.ndarray, off: np.ndarray) -> None:
        """Replace the finished hit table by the caller's (kp_batch_set_hits): rows ``off[a]:off[a + 1]`` are assembly a's."""
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        off = np.ascontiguousarray(off, dtype=np.int64)
        if len(off) != self.n_asm + 1 or int(off[-1]) != len(hits):
            raise ValueError("offsets do not describe the hit table")
        self.ctx._check(lib().kp_batch_set_hits(self.ctx._h, self._h, _p(hits), _p(off)), "kp_batch_set_hits")

    def cigars(self) -> tuple[np.ndarray, np.ndarray]:
        """(ops uint32, offsets int64 [total hits + 1]): the CIGAR of row i of ``hits()`` is ``ops[offsets[i]:offsets[i + 1]]``,
        BAM-encoded (kp_batch_cigars).  Only for a batch aligned with the context's ``cigar`` option set."""
        hit_off = np.zeros(self.n_asm + 1, np.int64)
        self.ctx._check(lib().kp_batch_hit_offsets(self.ctx._h, self._h, _p(hit_off)), "kp_batch_hit_offsets")
        off = np.zeros(int(hit_off[-1]) + 1, np.int64)
        self.ctx._check(lib().kp_batch_cigar_offsets(self.ctx._h, self._h, _p(off)), "kp_batch_cigar_offsets")
        ops = np.zeros(int(off[-1]), np.uint32)
        self.ctx._check(lib().kp_batch_cigars(self.ctx._h, self._h, _p(ops), C.c_int64(len(ops))), "kp_batch_cigars")
        return ops, off

    def cs(self) -> tuple[np.ndarray, np.ndarray]:
        """(bytes uint8, offsets int64 [total hits + 1]): the cs string of row i of ``hits()`` is ``bytes[offsets[i]:offsets[i + 1]]``
        (kp_batch_cs; include/kp_spec.h, CS).  Only for a batch aligned with the context's ``cs`` option set."""
        hit_off = np.zeros(self.n_asm + 1, np.int64)
        self.ctx._check(lib().kp_batch_hit_offsets(self.ctx._h, self._h, _p(hit_off)), "kp_batch_hit_offsets")
        off = np.zeros(int(hit_off[-1]) + 1, np.int64)
        self.ctx._check(lib().kp_batch_cs_offsets(self.ctx._h, self._h, _p(off)), "kp_batch_cs_offsets")
        data = np.zeros(int(off[-1]), np.uint8)
        self.ctx._check(lib().kp_batch_cs(self.ctx._h, self._h, _p(data), C.c_int64(len(data))), "kp_batch_cs")
        return data, off

    def stats(self) -> dict[str, int]:
        s = np.zeros(5, np.int64)
        self.ctx._check(lib().kp_batch_stats(self.ctx._h, self._h, _p(s)), "kp_batch_stats")
        return dict(zip(("anchors", "tasks", "dp_cells", "hits", "retries"), s.tolist()))

    # -- batched reduction ------------------------------------------------------------------------------------------
    def score(self, min_gene_coverage: float, group: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """(locus_scores f64, locus_counts i32), both [n_asm, n_loci]; finalises the hit tables on the device."""
        self.use_group(group)
        n_loci = self.ctx.group_loci[group]
        scores = np.zeros((self.n_asm, n_loci), np.float64)
        counts = np.zeros((self.n_asm, n_loci), np.int32)
        self.ctx._check(
            lib().kp_batch_score(self.ctx._h, self._h, C.c_double(min_gene_coverage), _p(scores), _p(counts)),
            "kp_batch_score",
        )
        return scores, counts

    def use_group(self, group: int) -> None:
        """The typing group (database) the score / reduce / typing / proteins calls address (kp_batch_use_group)."""
        self.ctx._check(lib().kp_batch_use_group(self.ctx._h, self._h, C.c_int32(group)), "kp_batch_use_group")

    def reduce_async(self, best_locus: np.ndarray, params: "TypingParams", group: int = 0) -> None:
        self.use_group(group)
        best = _c(best_locus, np.int32)
        self.ctx._check(lib().kp_batch_reduce(self.ctx._h, self._h, _p(best), C.byref(params)), "kp_batch_reduce")

    def typing(self, group: int = 0):
        """(summaries [n_asm], kept [n_asm, kept_cap], pieces [n_asm, piece_cap]) as structured arrays."""
        from kaptive_amd.serotyping.batch import KEPT_DTYPE, PIECE_DTYPE, SUMMARY_DTYPE

        self.use_group(group)
        for _ in range(2):  # capacities may grow inside kp_batch_typing when a buffer overflowed
            kc, pc = C.c_int32(0), C.c_int32(0)
            self.ctx._check(lib().kp_batch_typing_caps(self.ctx._h, self._h, C.byref(kc), C.byref(pc)), "typing_caps")
            sums = np.zeros(self.n_asm, SUMMARY_DTYPE)
            kept = np.zeros((self.n_asm, kc.value), KEPT_DTYPE)
            pieces = np.zeros((self.n_asm, pc.value), PIECE_DTYPE)
            rc = lib().kp_batch_typing(self.ctx._h, self._h, _p(sums), _p(kept), kc, _p(pieces), pc)
            if rc == -1 and b"strides too small" in lib().kp_last_error(self.ctx._h):
                continue
            self.ctx._check(rc, "kp_batch_typing")
            return sums, kept, pieces
        raise NativeError("kp_batch_typing: capacities kept changing")

    def variants(self, group: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """(records VARIANT_DTYPE, var_off int64 [n_asm + 1]): the variant records of the kept hits of ``typing(group)``, assembly
        a's being ``records[var_off[a]:var_off[a + 1]]`` (kp_batch_variants; include/kp_spec.h, VARIANTS).  Only after
        ``reduce_async`` of a batch aligned with the context's ``variants`` option set."""
        self.use_group(group)
        off = np.zeros(self.n_asm + 1, np.int64)
        self.ctx._check(lib().kp_batch_variant_offsets(self.ctx._h, self._h, _p(off)), "kp_batch_variant_offsets")
        out = np.zeros(int(off[-1]), VARIANT_DTYPE)
        self.ctx._check(lib().kp_batch_variants(self.ctx._h, self._h, _p(out), C.c_int64(len(out))), "kp_batch_variants")
        return out, off

    def breakpoints(self, group: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """(records BREAKPOINT_DTYPE, bp_off int64 [n_asm + 1]): the breakpoint records of the kept lists of ``typing(group)``,
        assembly a's being ``records[bp_off[a]:bp_off[a + 1]]`` (kp_batch_breakpoints; include/kp_spec.h, BREAKPOINTS).  After
        ``reduce_async``; no option is needed, and a hit table that ``set_hits`` put in place serves as well."""
        self.use_group(group)
        off = np.zeros(self.n_asm + 1, np.int64)
        self.ctx._check(lib().kp_batch_breakpoint_offsets(self.ctx._h, self._h, _p(off)), "kp_batch_breakpoint_offsets")
        out = np.zeros(int(off[-1]), BREAKPOINT_DTYPE)
        self.ctx._check(lib().kp_batch_breakpoints(self.ctx._h, self._h, _p(out), C.c_int64(len(out))), "kp_batch_breakpoints")
        return out, off

    def alleles(self, group: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """(records ALLELE_DTYPE [n_asm, kept_stride], piece digests uint64 [n_asm, piece_stride]): the allele digests of the kept
        records and the locus pieces of ``typing(group)``, laid out as its tables are (kp_batch_alleles; include/kp_spec.h, ALLELES);
        rows beyond the counts are zero.  After ``reduce_async``; no option is needed, and a hit table that ``set_hits`` put in
        place serves as well."""
        self.use_group(group)
        h = lib()
        # the first call makes the digests (or says why there are none); strides of zero serve a batch without a kept record only
        rc = h.kp_batch_alleles(self.ctx._h, self._h, None, C.c_int32(0), None, C.c_int32(0))
        if not (rc == -1 and b"strides too small" in h.kp_last_error(self.ctx._h)):
            self.ctx._check(rc, "kp_batch_alleles")
        kc, pc = C.c_int32(0), C.c_int32(0)
        self.ctx._check(h.kp_batch_typing_caps(self.ctx._h, self._h, C.byref(kc), C.byref(pc)), "typing_caps")
        out = np.zeros((self.n_asm, kc.value), ALLELE_DTYPE)
        pieces = np.zeros((self.n_asm, pc.value), np.uint64)
        self.ctx._check(h.kp_batch_alleles(self.ctx._h, self._h, _p(out), kc, _p(pieces), pc), "kp_batch_alleles")
        return out, pieces

    def aligned(self, group: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """(rows ALIGNED_ROW_DTYPE [n_asm, kept_stride], blocks uint64 [n_blocks]): the aligned rows of the kept hits of
        ``typing(group)`` (kp_batch_aligned_rows / _blocks; include/kp_spec.h, ALIGNED ROWS): ``rows[a, i]`` belongs to kept record i
        of assembly a, its ``(gene_len + 15) // 16`` blocks start at ``blocks[rows[a, i]["off"]]``; rows beyond the counts are zero.
        Only after ``reduce_async`` of a batch aligned with the context's ``aligned`` option set."""
        self.use_group(group)
        h = lib()
        n = C.c_int64(0)
        self.ctx._check(h.kp_batch_aligned_size(self.ctx._h, self._h, C.byref(n)), "kp_batch_aligned_size")
        kc, pc = C.c_int32(0), C.c_int32(0)
        self.ctx._check(h.kp_batch_typing_caps(self.ctx._h, self._h, C.byref(kc), C.byref(pc)), "typing_caps")
        rows = np.zeros((self.n_asm, kc.value), ALIGNED_ROW_DTYPE)
        blocks = np.zeros(n.value, np.uint64)
        self.ctx._check(h.kp_batch_aligned_rows(self.ctx._h, self._h, _p(rows), kc), "kp_batch_aligned_rows")
        self.ctx._check(h.kp_batch_aligned_blocks(self.ctx._h, self._h, _p(blocks), C.c_int64(len(blocks))), "kp_batch_aligned_blocks")
        return rows, blocks

    def rescue(self, group: int = 0) -> tuple[np.ndarray, np.ndarray]:
        """(records RESCUE_DTYPE, rescue_off int64 [n_asm + 1]): the rescue records of the genes ``typing(group)`` lists as missing,
        assembly a's being ``records[rescue_off[a]:rescue_off[a + 1]]`` (kp_batch_rescue; include/kp_spec.h, RESCUE).  After
        ``reduce_async``, on a context whose ``rescue`` option is set; a hit table that ``set_hits`` put in place serves as well."""
        self.use_group(group)
        off = np.zeros(self.n_asm + 1, np.int64)
        self.ctx._check(lib().kp_batch_rescue_offsets(self.ctx._h, self._h, _p(off)), "kp_batch_rescue_offsets")
        out = np.zeros(int(off[-1]), RESCUE_DTYPE)
        self.ctx._check(lib().kp_batch_rescue(self.ctx._h, self._h, _p(out), C.c_int64(len(out))), "kp_batch_rescue")
        return out, off

    def proteins(self, asm_index: int, nbytes: int, group: int = 0) -> np.ndarray:
        self.use_group(group)
        out = np.zeros(nbytes, np.uint8)
        self.ctx._check(lib().kp_batch_proteins(self.ctx._h, self._h, C.c_int32(asm_index), _p(out), C.c_int64(nbytes)),
                        "kp_batch_proteins")  # fmt: skip
        return out

    def profile(self) -> dict[str, float]:
        """Stage milliseconds of the most recent alignment pass (HIP events recorded on the context's stream)."""
        ms = np.zeros(7, np.float32)
        nbytes = C.c_int64(0)
        self.ctx._check(lib().kp_batch_profile(self.ctx._h, self._h, _p(ms), C.byref(nbytes)), "kp_batch_profile")
        d = dict(zip(("scan", "sort", "chain", "sw16", "sw32", "sw64", "sw128"), ms.tolist()))
        d["bytes_scanned"] = int(nbytes.value)
        return d

    def anchors(self, asm_index: int) -> np.ndarray:
        n = lib().kp_batch_anchors(self.ctx._h, self._h, C.c_int32(asm_index), None, C.c_int64(0))
        self.ctx._check(n, "kp_batch_anchors")
        out = np.zeros(n, np.uint64)
        lib().kp_batch_anchors(self.ctx._h, self._h, C.c_int32(asm_index), _p(out), C.c_int64(n))
        return out

    def tasks(self, asm_index: int) -> np.ndarray:
        n = lib().kp_batch_tasks(self.ctx._h, self._h, C.c_int32(asm_index), None, C.c_int64(0))
        self.ctx._check(n, "kp_batch_tasks")
        out = np.zeros(n, TASK_DTYPE)
        lib().kp_batch_tasks(self.ctx._h, self._h, C.c_int32(asm_index), _p(out), C.c_int64(n))
        return out


    def task_results(self, asm_index: int) -> np.ndarray:
        """[n_tasks, 7] int32 -- score, q_start, q_end, t_start, t_end, matches, block_len -- row for row with ``tasks``;
        tasks below the score cut-off carry their score and zeros (kp_batch_task_results)."""
        n = lib().kp_batch_task_results(self.ctx._h, self._h, C.c_int32(asm_index), None, C.c_int64(0))
        self.ctx._check(n, "kp_batch_task_results")
        out = np.zeros((n, 7), np.int32)
        lib().kp_batch_task_results(self.ctx._h, self._h, C.c_int32(asm_index), _p(out), C.c_int64(n))
        return out


    def joins(self, asm_index: int) -> np.ndarray:
        """The joins of one assembly (kp_spec.h, kp-align v5) as JOIN_DTYPE rows, in device order (kp_batch_joins)."""
        n = lib().kp_batch_joins(self.ctx._h, self._h, C.c_int32(asm_index), None, C.c_int64(0))
        self.ctx._check(n, "kp_batch_joins")
        out = np.zeros(n, JOIN_DTYPE)
        lib().kp_batch_joins(self.ctx._h, self._h, C.c_int32(asm_index), _p(out), C.c_int64(n))
        return out

    def occ(self, asm_index: int) -> tuple[int, int, np.ndarray]:
        """What the occurrence cut left for one assembly (kp_batch_occ): its state word (bit 0: a gene seed beyond the floor,
        bit 1: its own mid_occ decides), the mid_occ it was cut at, and -- where it claimed a counting table -- the table's
        non-empty entries as uint32 [n, 2] rows (seed value, count); [0, 2] otherwise."""
        n = lib().kp_batch_occ(self.ctx._h, self._h, C.c_int32(asm_index), None, C.c_int64(0))
        self.ctx._check(n, "kp_batch_occ")
        out = np.zeros(n, np.uint32)
        lib().kp_batch_occ(self.ctx._h, self._h, C.c_int32(asm_index), _p(out), C.c_int64(n))
        return int(out[0]), int(out[1]), out[2:].reshape(-1, 2)

    def candidates(self) -> tuple[np.ndarray, np.ndarray]:
        """The seed scan's candidate list of the batch's last pass (kp_batch_candidates) as two uint64 arrays: the streaming
        kernel's words (front) and the edge kernel's (back), each (batch-wide position << 31) | (strand bit << 30) | seed value.
        The order within either array is that of the device's appends: compare them sorted."""
        n = lib().kp_batch_candidates(self.ctx._h, self._h, None, C.c_int64(0))
        self.ctx._check(n, "kp_batch_candidates")
        out = np.zeros(n, np.uint64)
        self.ctx._check(lib().kp_batch_candidates(self.ctx._h, self._h, _p(out), C.c_int64(n)), "kp_batch_candidates")
        n_front, n_back = int(out[0]), int(out[1])
        return out[2 : 2 + n_front].copy(), out[2 + n_front : 2 + n_front + n_back].copy()


class Distances:
    """The locus rows of one locus on the device, ready to be compared all against all (kp_dist; include/kp_spec.h, DISTANCES).
    ``rows_matrix``: uint64 [n_rows, n_blocks], one locus row per assembly, padding flagged.  A context manager; closing the context
    closes it too."""

    def __init__(self, ctx: Context, rows_matrix) -> None:
        m = np.ascontiguousarray(rows_matrix, np.uint64)
        if m.ndim != 2:
            raise ValueError("the locus rows come as a [n_rows, n_blocks] matrix")
        self.ctx, self.n_rows, self.n_blocks = ctx, int(m.shape[0]), int(m.shape[1])
        self._h = C.c_void_p()
        ctx._check(lib().kp_dist_create(ctx._h, _p(m), C.c_int32(self.n_rows), C.c_int64(self.n_blocks), C.byref(self._h)), "kp_dist_create")
        ctx._batches.add(self)
        _live.add(self)

    def close(self) -> None:
        if getattr(self, "_h", None):
            if getattr(self.ctx, "_h", None):  # (as a batch: without its context there is nothing left to free)
                lib().kp_dist_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self) -> "Distances":
        return self

    def __exit__(self, *exc) -> None:
        self.close()

    def count(self, max_diff: "int | None" = None, min_compared: int = 0) -> int:
        """How many pairs ``pairs`` would list (kp_dist_count)."""
        n = C.c_int64(0)
        md = np.iinfo(np.int32).max if max_diff is None else int(max_diff)
        self.ctx._check(lib().kp_dist_count(self.ctx._h, self._h, C.c_int32(md), C.c_int32(int(min_compared)), C.byref(n)), "kp_dist_count")
        return n.value

    def pairs(self, max_diff: "int | None" = None, min_compared: int = 0) -> np.ndarray:
        """DIST_PAIR_DTYPE records of the pairs (a, b), a < b, with ``differences <= max_diff`` (None: no limit) and ``compared >=
        min_compared``, ascending in (a, b)."""
        out = np.zeros(self.count(max_diff, min_compared), DIST_PAIR_DTYPE)
        self.ctx._check(lib().kp_dist_pairs(self.ctx._h, self._h, _p(out), C.c_int64(len(out))), "kp_dist_pairs")
        return out

    def clusters(self, levels=CLUSTER_LEVELS, min_compared: int = DIST_MIN_COMPARED, nearest: bool = True):
        """(labels int32 [K, R], nearest DIST_NEAREST_DTYPE [R]) of the rows (kp_dist_clusters; include/kp_spec.h, CLUSTERS):
        ``labels[k, r]`` is the smallest row of r's single-linkage cluster at ``differences <= levels[k]``, ``nearest[r]`` the row
        with the fewest differences from r (then the smaller row) among those with ``compared >= min_compared``, with the pair's
        three counts; row -1 where there is none.  With ``nearest=False`` the second item is None.  No pair is listed for it, and
        the listing state of ``count`` / ``pairs`` is left alone."""
        lv = np.array(check_cluster_levels(levels), np.int32)
        labels = np.zeros((len(lv), self.n_rows), np.int32)
        near = np.zeros(self.n_rows, DIST_NEAREST_DTYPE) if nearest else None
        if nearest:
            near["row"] = -1
        self.ctx._check(lib().kp_dist_clusters(self.ctx._h, self._h, _p(lv) if len(lv) else None, C.c_int32(len(lv)), C.c_int32(int(min_compared)),
                                               _p(labels) if labels.size else None, _p(near) if nearest else None), "kp_dist_clusters")
        return labels, near

    def tree(self, min_compared: int = DIST_MIN_COMPARED):
        """(edges DIST_PAIR_DTYPE [E], component int32 [R]) of the rows' minimum spanning forest (kp_dist_tree; include/kp_spec.h,
        TREE): the graph's edges are the pairs with ``compared >= min_compared``, an edge's key is (differences, a, b); the forest's
        edges ascend by key, ``component[r]`` is the smallest row of r's tree and ``E == R - number of trees``.  No pair is listed
        for it; the listing state and the cluster tables are left alone."""
        edges = np.zeros(max(self.n_rows - 1, 0), DIST_PAIR_DTYPE)
        component = np.zeros(self.n_rows, np.int32)
        n = C.c_int64(0)
        self.ctx._check(lib().kp_dist_tree(self.ctx._h, self._h, C.c_int32(int(min_compared)), _p(edges) if len(edges) else None, C.c_int64(len(edges)),
                                           C.byref(n), _p(component) if self.n_rows else None), "kp_dist_tree")
        return edges[: n.value].copy(), component

    def tree_rounds(self) -> int:
        """The rounds the last ``tree`` ran on the device, the empty last one included (kp_dist_tree_rounds)."""
        return int(lib().kp_dist_tree_rounds(self._h))

    def nj_taxa(self, min_compared: int = DIST_MIN_COMPARED) -> int:
        """How many taxa ``nj`` would join (the counting form of kp_dist_nj): the rows that hold a base in at least half of the
        columns plus half of ``max(min_compared, 1)``."""
        n = C.c_int32(0)
        self.ctx._check(lib().kp_dist_nj(self.ctx._h, self._h, C.c_int32(int(min_compared)), None, C.c_int64(0), C.byref(n), None, C.c_int64(0), None), "kp_dist_nj")
        return n.value

    def nj(self, min_compared: int = DIST_MIN_COMPARED):
        """(taxa int32 [n], nodes NJ_NODE_DTYPE) of the rows' neighbour-joining tree (kp_dist_nj; include/kp_spec.h, NJ): ``taxa``
        the rows that are taxa, ascending; ``nodes`` the records of the joins in the order they were made -- node ids below n index
        ``taxa``, the id n + r is the inner node record r made -- and the last one holds the three nodes that were left.  More than
        ``NJ_MAX_TAXA`` taxa are refused.  The listing state and every other table of the handle are left alone."""
        n = self.nj_taxa(min_compared)
        taxa, nodes = np.zeros(n, np.int32), np.zeros(max(n - 2, 1 if n == 2 else 0), NJ_NODE_DTYPE)
        got, made = C.c_int32(0), C.c_int64(0)
        self.ctx._check(lib().kp_dist_nj(self.ctx._h, self._h, C.c_int32(int(min_compared)), _p(taxa) if n else None, C.c_int64(n), C.byref(got),
                                         _p(nodes) if len(nodes) else None, C.c_int64(len(nodes)), C.byref(made)), "kp_dist_nj")  # fmt: skip
        return taxa[: got.value].copy(), nodes[: made.value].copy()

    def nj_support(self, min_compared: int, nodes, replicates: int, seed: int = 1, max_batch: int = 0, trees: bool = False):
        """int32 [len(nodes)]: the bootstrap support of every record of ``nodes`` -- the tree ``nj(min_compared)`` gave -- out of
        ``replicates`` resamplings of the block columns under ``seed`` (kp_dist_nj_bootstrap; include/kp_spec.h, BOOTSTRAP): how
        many replicate trees hold the split of the node the record made, -1 for a record without an inner edge.  ``max_batch``: the
        most replicates joined at once (0: the library's choice; no result depends on it).  With ``trees`` the result is
        ``(support, NJ_NODE_DTYPE [replicates, len(nodes)])``: every replicate's records.  The state of every other report is left alone."""
        nodes = np.ascontiguousarray(nodes, dtype=NJ_NODE_DTYPE)
        support = np.zeros(len(nodes), np.int32)
        reps = np.zeros((int(replicates) if 0 < int(replicates) <= BOOT_MAX_REPLICATES else 0, len(nodes)), NJ_NODE_DTYPE) if trees else None
        self.ctx._check(lib().kp_dist_nj_bootstrap(self.ctx._h, self._h, C.c_int32(int(min_compared)), C.c_uint64(int(seed) & (2**64 - 1)), C.c_int32(int(replicates)),
                                                   C.c_int32(int(max_batch)), _p(nodes) if len(nodes) else None, C.c_int64(len(nodes)), _p(support) if len(nodes) else None,
                                                   C.c_int64(len(support)), _p(reps) if trees and reps.size else None, C.c_int64(reps.size if trees else 0)), "kp_dist_nj_bootstrap")  # fmt: skip
        return (support, reps) if trees else support

    def nj_transfer(self, min_compared: int, nodes, replicates: int, seed: int = 1, max_batch: int = 0, per_replicate: bool = False, trees: bool = False):
        """``(support int32, transfer int64)``, both ``[len(nodes)]``: the transfer bootstrap of every record of ``nodes`` -- any
        record list of the handle's taxa -- out of ``nj_support``'s replicates (kp_dist_nj_transfer; include/kp_spec.h, TRANSFER):
        ``transfer`` the sum over the replicates of the fewest taxa that must move for the replicate's tree to hold the record's
        split, ``support`` the replicates in which none must, counted on exact sets; -1 for a record without an inner edge.  With
        ``per_replicate`` the result also holds ``int32 [replicates, len(nodes)]``, every distance; with ``trees`` every replicate's
        records, last.  The state of every other report is left alone."""
        nodes = np.ascontiguousarray(nodes, dtype=NJ_NODE_DTYPE)
        support, transfer = np.zeros(len(nodes), np.int32), np.zeros(len(nodes), np.int64)
        N = int(replicates) if 0 < int(replicates) <= BOOT_MAX_REPLICATES else 0
        phi = np.zeros((N, len(nodes)), np.int32) if per_replicate else None
        reps = np.zeros((N, len(nodes)), NJ_NODE_DTYPE) if trees else None
        self.ctx._check(lib().kp_dist_nj_transfer(self.ctx._h, self._h, C.c_int32(int(min_compared)), C.c_uint64(int(seed) & (2**64 - 1)), C.c_int32(int(replicates)),
                                                  C.c_int32(int(max_batch)), _p(nodes) if len(nodes) else None, C.c_int64(len(nodes)), _p(support) if len(nodes) else None,
                                                  C.c_int64(len(support)), _p(transfer) if len(nodes) else None, C.c_int64(len(transfer)),
                                                  _p(phi) if per_replicate and phi.size else None, C.c_int64(phi.size if per_replicate else 0),
                                                  _p(reps) if trees and reps.size else None, C.c_int64(reps.size if trees else 0)), "kp_dist_nj_transfer")  # fmt: skip
        return (support, transfer, *((phi,) if per_replicate else ()), *((reps,) if trees else ()))

    def nj_parsimony(self, min_compared: int, nodes):
        """``(sites PARS_SITE_DTYPE, changes PARS_CHANGE_DTYPE)``: small parsimony of every column of the matrix on the tree
        ``nodes`` -- ``nj(min_compared)``'s records, or any record list of the handle's taxa in their form -- (kp_dist_nj_parsimony;
        include/kp_spec.h, PARSIMONY): ``sites`` the columns the tree needs a change for, ascending, with their steps and the bases
        that occur; ``changes`` every change, ascending by (node, column): the branch by its child end, its parent, the parent's
        state and the node's.  States are relative to the last record, which is no root.  A list that is no tree of the handle's
        taxa is refused.  The state of every other report is left alone."""
        nodes = np.ascontiguousarray(nodes, dtype=NJ_NODE_DTYPE)
        ns, nc = C.c_int64(0), C.c_int64(0)
        self.ctx._check(lib().kp_dist_nj_parsimony(self.ctx._h, self._h, C.c_int32(int(min_compared)), _p(nodes) if len(nodes) else None, C.c_int64(len(nodes)),
                                                   C.byref(ns), C.byref(nc)), "kp_dist_nj_parsimony")  # fmt: skip
        sites, changes = np.zeros(ns.value, PARS_SITE_DTYPE), np.zeros(nc.value, PARS_CHANGE_DTYPE)
        self.ctx._check(lib().kp_dist_pars_sites(self.ctx._h, self._h, _p(sites) if len(sites) else None, C.c_int64(len(sites))), "kp_dist_pars_sites")
        self.ctx._check(lib().kp_dist_pars_changes(self.ctx._h, self._h, _p(changes) if len(changes) else None, C.c_int64(len(changes))), "kp_dist_pars_changes")
        return sites, changes

    def boot_weights(self, seed: int, replicate: int) -> np.ndarray:
        """uint8 [16 * n_blocks]: how often every block column of the matrix, padding included, is drawn in replicate ``replicate`` of
        ``seed``, clamped at 255 (kp_dist_boot_weights): the weights the replicate's counts are made under."""
        out = np.zeros(16 * self.n_blocks, np.uint8)
        self.ctx._check(lib().kp_dist_boot_weights(self.ctx._h, self._h, C.c_uint64(int(seed) & (2**64 - 1)), C.c_int32(int(replicate)), _p(out) if len(out) else None,
                                                   C.c_int64(len(out))), "kp_dist_boot_weights")  # fmt: skip
        return out

    def profile(self) -> np.ndarray:
        """SITE_DTYPE records of all ``16 * n_blocks`` columns of the matrix, padding columns included, ascending (kp_dist_profile;
        include/kp_spec.h, SITES): how many rows hold a, c, g, t and N at the column.  Computed once per handle."""
        out = np.zeros(16 * self.n_blocks if self.n_rows else 0, SITE_DTYPE)
        self.ctx._check(lib().kp_dist_profile(self.ctx._h, self._h, _p(out) if len(out) else None, C.c_int64(len(out))), "kp_dist_profile")
        return out

    def sites_count(self, core: bool = False) -> int:
        """How many sites ``sites`` would list (kp_dist_sites_count)."""
        n = C.c_int64(0)
        self.ctx._check(lib().kp_dist_sites_count(self.ctx._h, self._h, C.c_int32(SITES_CORE if core else 0), C.byref(n)), "kp_dist_sites_count")
        self._n_sites = n.value  # (``site_rows`` sizes its table by it)
        return n.value

    def sites(self, core: bool = False) -> np.ndarray:
        """SITE_DTYPE records of the columns at which at least two bases occur among the rows, ascending in column (kp_dist_sites);
        with ``core`` only those at which every row holds a base.  No pair is looked at for it; the listing state, the cluster
        tables and the tree tables are left alone."""
        out = np.zeros(self.sites_count(core), SITE_DTYPE)
        self.ctx._check(lib().kp_dist_sites(self.ctx._h, self._h, _p(out) if len(out) else None, C.c_int64(len(out))), "kp_dist_sites")
        return out

    def site_rows(self) -> np.ndarray:
        """uint64 [n_rows, (S + 15) // 16]: every row's codes at the S sites of the last ``sites`` / ``sites_count``, in the packed
        form of the rows themselves, the columns at or beyond S GAP-flagged (kp_dist_site_rows) -- a matrix ``Distances`` takes.
        Without a count the library refuses the call."""
        S = getattr(self, "_n_sites", None)
        out = np.zeros((self.n_rows, ((S or 0) + 15) // 16), np.uint64)
        self.ctx._check(lib().kp_dist_site_rows(self.ctx._h, self._h, _p(out) if out.size else None, C.c_int64(out.size)), "kp_dist_site_rows")
        return out


RANDSTROBE_DTYPE = np.dtype([("hash", "<u8"), ("seq_idx", "<u4"), ("pos1", "<u4"), ("pos2", "<u4")])


def randstrobes(seqs, offsets, lengths, lut, k: int, s: int, w_min: int, w_max: int, sort_by_hash: bool) -> np.ndarray:
    """Randstrobe records of a batch of sequences (kp_randstrobes; host only)."""
    h = lib()
    h.kp_randstrobes.restype = C.c_int64
    seqs, offsets, lengths, lut = _c(seqs, np.uint8), _c(offsets, np.int32), _c(lengths, np.int32), _c(lut, np.uint8)
    args = (_p(seqs), _p(offsets), _p(lengths), C.c_int32(len(offsets)), _p(lut), C.c_int32(k), C.c_int32(s),
            C.c_int32(w_min), C.c_int32(w_max), C.c_int32(int(sort_by_hash)))  # fmt: skip
    n = h.kp_randstrobes(*args, None, C.c_int64(0))
    if n < 0:
        raise ValueError(f"kp_randstrobes failed ({n})")
    out = np.empty(int(n), RANDSTROBE_DTYPE)
    if n:
        h.kp_randstrobes(*args, _p(out), C.c_int64(n))
    return out


def randstrobe_top_hits(q_records: np.ndarray, n_queries: int, t_records: np.ndarray, n_targets: int):
    """(best target u32, score u32, diagonal offset i32) per query sequence (kp_randstrobe_top_hits; host only)."""
    q_records, t_records = np.ascontiguousarray(q_records), np.ascontiguousarray(t_records)
    best_t, score = np.zeros(n_queries, np.uint32), np.zeros(n_queries, np.uint32)
    off = np.zeros(n_queries, np.int32)
    rc = lib().kp_randstrobe_top_hits(_p(q_records), C.c_int64(len(q_records)), C.c_int32(n_queries), _p(t_records),
                                      C.c_int64(len(t_records)), C.c_int32(n_targets), _p(best_t), _p(score), _p(off))  # fmt: skip
    if rc != 0:
        raise ValueError(f"kp_randstrobe_top_hits failed ({rc})")
    return best_t, score, off


def pinned_bytes() -> int:
    """Page-locked host bytes this process holds through the library (kp_host_pinned_bytes)."""
    f = lib().kp_host_pinned_bytes
    f.restype = C.c_int64
    return int(f())


def device_allocations() -> int:
    """How many device buffers the library has re-allocated so far (kp_device_allocations): each one stalls every pass
    in flight, so a settled stream of batches must not add to it."""
    f = lib().kp_device_allocations
    f.restype = C.c_int64
    return int(f())


class PinnedBuffer:
    """Page-locked host memory (kp_host_alloc) exposed as a numpy array; freed by ``close`` / garbage collection.
    ``lazy``: plain huge-page memory for now (kp_host_reserve: no call into the device runtime), page-locked by ``lock()``
    once the caller's threads have filled it -- the first touch is then theirs, spread over as many threads as they are,
    and the lock itself takes 2 ms per GB."""

    def __init__(self, n_items: int, dtype=np.uint32, lazy: bool = False) -> None:
        self._p = C.c_void_p()
        dt = np.dtype(dtype)
        nbytes = max(1, int(n_items) * dt.itemsize)
        self.locked = not lazy
        rc = (lib().kp_host_reserve if lazy else lib().kp_host_alloc)(C.c_size_t(nbytes), C.byref(self._p))
        if rc != 0:
            raise NativeError(f"kp_host_alloc failed ({rc}): {lib().kp_last_error(None).decode()}")
        buf = (C.c_uint8 * nbytes).from_address(self._p.value)
        self.array = np.frombuffer(buf, dtype=dt, count=int(n_items))

    def lock(self) -> None:
        if not self.locked:
            rc = lib().kp_host_lock(self._p)
            if rc != 0:
                raise NativeError(f"kp_host_lock failed ({rc}): {lib().kp_last_error(None).decode()}")
            self.locked = True

    def close(self) -> None:
        if getattr(self, "_p", None) and self._p.value:
            self.array = None
            lib().kp_host_free(self._p)
            self._p = C.c_void_p()

    __del__ = close


_default_ctx: dict[int, Context] = {}


def default_context(device: int = 0) -> Context:
    with _lock:
        if device not in _default_ctx:
            _default_ctx[device] = Context(device)
        return _default_ctx[device]


def protein_align(device, q, q_off, q_len, t, t_off, t_len) -> np.ndarray:
    return default_context(device).protein_align(q, q_off, q_len, t, t_off, t_len)
