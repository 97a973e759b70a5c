/* kaptive_amd.h -- C ABI of libkaptive_amd.so: the MI355X (gfx950) implementation of Kaptive's typing hot path.
 *
 * The reference (klebgenomics/Kaptive) has no C ABI for this path: its native seam is the Python binding of the
 * third-party rammappy wheel plus numba-compiled kernels.  Each entry point below names the reference interface it
 * stands in for (paths relative to the reference checkout); INTEGRATION.md shows the ctypes binding a Kaptive
 * maintainer would add.  Conventions: every call returns 0 on success or a negative KP_E* code and records a message
 * retrievable with kp_last_error(); no exceptions cross the boundary; the caller owns every host buffer it passes and
 * may free it as soon as the call returns unless stated otherwise; the library owns all device memory.  A context is
 * bound to one GPU; calls on one context must be serialised by the caller, distinct contexts are independent (one
 * context per device / per host thread).
 *
 * Ownership of device memory.  Work buffers (anchors, band tasks, hit tables, reduction records) belong to the context,
 * not to a batch: a context owns KP_WORK_SLOTS work sets, kp_batch_align takes the next one round-robin, and the sizes
 * the library learns for them (overflow -> automatic rerun with more room) are kept for every later batch.  So a stream
 * of batches allocates nothing after its first few, and the context holds the alignment results of its KP_WORK_SLOTS
 * most recently aligned batches; calls that read results of a batch displaced since return KP_ESTATE.  The device
 * copies of batch inputs are recycled through the context in the same way.
 */
#ifndef KAPTIVE_AMD_H
#define KAPTIVE_AMD_H

#include <stddef.h>
#include <stdint.h>

#include "kp_spec.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KP_API __attribute__((visibility("default")))

#define KP_OK 0
#define KP_EINVAL (-1)    /* bad argument (null pointer, limits of kp_spec.h exceeded, inconsistent offsets) */
#define KP_EHIP (-2)      /* a HIP runtime call failed; message carries hipGetErrorString */
#define KP_ENOMEM (-3)    /* host or device allocation failed */
#define KP_ESTATE (-4)    /* call out of order (no database loaded, no batch aligned, ...) */
#define KP_EOVERFLOW (-5) /* an internal device buffer overflowed and the automatic retry also failed */
#define KP_ENOTSUP (-6)   /* the host lacks what the call needs (kp_fasta_ingest: no libbz2 / liblzma to load) */
#define KP_EIO (-7)       /* a file could not be opened or mapped (kp_fasta_ingest_file) */

typedef struct kp_ctx kp_ctx;     /* one GPU + stream + resident database */
typedef struct kp_batch kp_batch; /* a set of packed assemblies resident in HBM, plus its results */

/* ---- context -------------------------------------------------------------------------------------------------- */
/* GPUs the process sees (>= 0), or a negative KP_E* code: `kaptive assembly --devices all` shards over all of them, one
 * process each (the reference has no device notion; its unit of parallelism is the worker thread, cli.py:183-210). */
KP_API int kp_device_count(void);
/* NUMA node of a GPU (its PCI function's /sys/bus/pci/devices/<bus id>/numa_node), -1 when the host does not say: the
 * per-device processes pin themselves and their page-locked shards to it (kaptive_amd/affinity.py).  No context needed. */
KP_API int kp_device_numa_node(int device_id);
KP_API int kp_ctx_create(int device_id, kp_ctx **out);
KP_API void kp_ctx_destroy(kp_ctx *ctx);
/* Message of the last failed call on ctx (ctx may be NULL for a failed kp_ctx_create). Never NULL. */
KP_API const char *kp_last_error(const kp_ctx *ctx);
/* The context's own hipStream_t: database uploads and stand-alone protein alignments.  (Alignment passes run on the
 * stream of the work set they take, so that the passes of consecutive batches overlap; their stage times: kp_batch_profile.) */
KP_API void *kp_ctx_stream(kp_ctx *ctx);
/* Tuning knobs.  Defaults are read from the environment once, in kp_ctx_create (KAPTIVE_AMD_<NAME in upper case>);
 * names: anchor_cap, tasks_per_asm, hit_cap, trace_kb_per_asm, cand_cap, group_cap, join_cap, occ_slots, kept_cap,
 * piece_cap, prot_cap (initial sizes of the work buffers, at least 1; trace_kb_per_asm: direction bits of the banded
 * Smith-Waterman, KiB per assembly of a batch; cand_cap: seed candidates of the scan, entries per batch -- unset, both are
 * sized from the batch with a floor of 64 Ki entries and 64 KiB; group_cap, join_cap: groups of clusters and joins per
 * band class of a batch; occ_slots: counting tables of the occurrence cut, at most 65536 -- setting one also forgets
 * what the context has learnt for it), library_sort (anchors are sorted by the library's segmented radix sort instead of
 * the bucket sort of kp_bsort.hip; same result), scan_mode (ablation modes of the scan kernel, tools/scan_ablate.py),
 * cigar (0 | 1: CIGARs of the hits, kp_batch_cigars; from the next kp_batch_align) and cigar_ops_per_hit (first size of their
 * buffer; setting it forgets what the context has learnt for it), cs (0 | 1: cs difference strings of the hits, kp_batch_cs;
 * from the next kp_batch_align; such a pass computes the CIGARs as well) and cs_bytes_per_hit (first size of their buffer,
 * likewise), variants (0 | 1: variant records of the kept hits, kp_batch_variants; from the next kp_batch_align; such a pass
 * computes the CIGARs as well) and variants_per_kept (first size of their buffer, likewise), rescue (0 | 1) and rescue_flank (0 .. 65535:
 * the rescue records of the missing genes, kp_batch_rescue; read when the records are asked for). */
KP_API int kp_ctx_set_option(kp_ctx *ctx, const char *name, int64_t value);
#define KP_WORK_SLOTS 3

/* ---- pinned host memory ---------------------------------------------------------------------------------------------------
 * For callers that stream shards: kp_batch_create_async only overlaps with device work when `words` is page-locked. */
KP_API int kp_host_alloc(size_t bytes, void **out);
KP_API void kp_host_free(void *p);
/* The same in two steps, for a caller whose own threads fill the block: kp_host_reserve hands out plain anonymous
 * memory (2 MB-aligned, advised to use huge pages; no call into the device runtime, so it works -- and costs nothing --
 * before a context exists), kp_host_lock page-locks it once it has been written (2 ms per GB of touched huge pages;
 * untouched pages are faulted in by the lock itself, on the calling thread).  kp_host_free takes either state. */
KP_API int kp_host_reserve(size_t bytes, void **out);
KP_API int kp_host_lock(void *p);
/* Page-locked bytes this process currently holds through the library: kp_host_alloc blocks plus the table staging of
 * the contexts' input buffers.  (What a rank pins matters when eight of them share one host.) */
KP_API int64_t kp_host_pinned_bytes(void);
/* Device buffers the library has had to RE-allocate (free + allocate a larger one) since the process started.  Each of
 * those waits for the whole device, i.e. for every pass in flight: a stream of batches should settle at a constant
 * (work buffers are sized from what the context has learnt, with head-room) and a caller can check that it does. */
KP_API int64_t kp_device_allocations(void);

/* ---- database ---------------------------------------------------------------------------------------------------
 * Replaces what Serotyper.__init__ prepares for the aligner -- the list of (name, gene bytes) handed to
 * rammappy's map_batch (src/kaptive/serotyping/core.py:111-121,154) -- with a device-resident seed index over all
 * genes (both strands) and 4-bit copies of the gene sequences.
 *   gene_codes : one byte per base, 0..3 = ACGT, 4 = anything else; genes back to back
 *   gene_off   : n_genes + 1 offsets into gene_codes
 * Loading a database replaces any previous one. */
KP_API int kp_db_load(kp_ctx *ctx, const uint8_t *gene_codes, const int32_t *gene_off, int32_t n_genes);
/* Number of (k-mer, gene, strand, position) postings in the resident seed index. */
KP_API int64_t kp_db_n_postings(const kp_ctx *ctx);

/* ---- FASTA ingest (host only) --------------------------------------------------------------------------------------------
 * Replaces rammappy.fasta.parse_fasta_bytes + Sequences.from_records + the per-contig copies handed to Index.build
 * (src/kaptive/core/genome.py:35-46,188; src/kaptive/core/seq.py:281-325): one pass from (decompressed) FASTA text to
 * the packed layout of kp_spec.h.  The result is owned by the library until kp_fasta_free. */
typedef struct kp_packed_fasta {
    int64_t padded_len;   /* bases, multiple of KP_ASM_ALIGN */
    int32_t n_contigs, n_runs;
    uint32_t *words;      /* padded_len / 16 */
    int32_t *ctg_start, *ctg_len;
    int32_t *n_run_pairs; /* 2 * n_runs */
    char *names;          /* contig names back to back (first word of each header), not NUL-terminated */
    int32_t *name_off;    /* n_contigs + 1 */
    uint8_t *seqs;        /* KP_FASTA_KEEP_TEXT: the contigs' symbols as written, whitespace removed, back to back */
    int64_t n_seq_bytes;  /*   (contig c = seqs[sum of ctg_len[0..c) .. + ctg_len[c]]); NULL / 0 otherwise */
} kp_packed_fasta;
KP_API int kp_fasta_pack(const uint8_t *data, int64_t n, kp_packed_fasta **out);
/* The same from a file's bytes as they are on disk: KP_FASTA_GZIP inflates first (zlib; gzip or zlib framing, several
 * members), KP_FASTA_KEEP_TEXT also returns the sequence text, which is what GenomeAssembly.from_file needs next to the
 * packed form (src/kaptive/core/genome.py:194-214: open by suffix, read everything, parse). */
#define KP_FASTA_GZIP 1
#define KP_FASTA_KEEP_TEXT 2
#define KP_FASTA_BZ2 4 /* bzip2 stream(s): libbz2 of the host, looked up at first use; KP_ENOTSUP when the host has none */
#define KP_FASTA_XZ 8  /* .xz stream(s): liblzma of the host, likewise (the reference opens .gz / .bz2 / .xz by suffix) */
KP_API int kp_fasta_ingest(const uint8_t *data, int64_t n, int32_t flags, kp_packed_fasta **out);
/* The same from the file itself (GenomeAssembly.from_file, src/kaptive/core/genome.py:194-214, reads the whole file into a
 * bytes object first): the library reads it into a recycled buffer of its own and parses it there.
 * `flags` as above (the caller picks the compression from the suffix, as the reference does); KP_EIO when the path
 * cannot be opened or is not a regular file. */
KP_API int kp_fasta_ingest_file(const char *path, int32_t flags, kp_packed_fasta **out);
/* Many files in one call, on `threads` host threads of the library's own (0 = one per core, at most n_files): file i is
 * data[i][0 .. n[i]) with flags[i]; out[i] and rc[i] are what kp_fasta_ingest would have returned for it.  A reader that
 * feeds a GPU has to turn tens of GB/s of text into packed words; a Python thread per file spends too much of each call
 * holding the interpreter lock.  Returns KP_OK when the arguments were usable (look at rc[] for the files). */
KP_API int kp_fasta_ingest_many(const uint8_t *const *data, const int64_t *n, const int32_t *flags, int32_t n_files,
                                int32_t threads, kp_packed_fasta **out, int32_t *rc);
/* A chunk of files -> the tables of one batch, for a reader that feeds a GPU from FASTA files (the reference reads, parses
 * and indexes one file at a time on its worker threads, src/kaptive/serotyping/cli.py:183-210, core/genome.py:177-214).
 * kp_fasta_ingest_shard parses the files (kp_fasta_ingest_file, sequence text not kept) on `threads` threads of the library
 * (0 = one per core) and lays the tables out exactly as kp_batch_create* takes them; a file that failed is an empty
 * assembly here, rc[i] holds its code (n_failed / first_failed say whether to look).  kp_shard_words_into then copies the
 * packed words of all assemblies back to back into `dst` (total_words of them; page-locked memory the caller sized after
 * the first call) and releases the per-file buffers; the tables stay valid until kp_shard_free. */
typedef struct kp_packed_shard {
    int32_t n_asm, n_failed, first_failed;
    int64_t total_words;
    int64_t *asm_word_off;                /* n_asm + 1 */
    int32_t *ctg_start, *ctg_len;         /* asm_first_ctg[n_asm] each */
    int32_t *asm_first_ctg;               /* n_asm + 1 */
    int32_t *n_runs;                      /* 2 * asm_first_nrun[n_asm] */
    int32_t *asm_first_nrun;              /* n_asm + 1 */
    int32_t *rc;                          /* n_asm */
} kp_packed_shard;
KP_API int kp_fasta_ingest_shard(const char *const *paths, const int32_t *flags, int32_t n_files, int32_t threads,
                                 kp_packed_shard **out);
KP_API int kp_shard_words_into(kp_packed_shard *shard, uint32_t *dst, int64_t dst_words, int32_t threads);
KP_API void kp_shard_free(kp_packed_shard *shard);
/* Which text path the ingest runs on this host: 2 = 64 bytes at a time with AVX-512 (BW, VBMI2) + BMI2, 1 = AVX2 + BMI2,
 * 0 = table look-ups; settled from cpuid at first use (environment KAPTIVE_AMD_FASTA_SIMD caps it).  cap >= 0 lowers it
 * for the calls that follow (tests compare the paths), cap < 0 only asks.  All paths give the same bytes. */
KP_API int kp_fasta_simd(int32_t cap);
/* The same layout from contigs already in memory (Sequences.seqs / offsets / lengths of the reference's containers,
 * src/kaptive/core/seq.py:307-325): contig c is seqs[offsets[c] .. offsets[c] + lengths[c]).  names / name_off of the
 * result are empty. */
KP_API int kp_pack_contigs(const uint8_t *seqs, const int64_t *offsets, const int32_t *lengths, int32_t n_contigs,
                           kp_packed_fasta **out);
KP_API void kp_fasta_free(kp_packed_fasta *packed);

/* ---- batches of packed assemblies -------------------------------------------------------------------------------
 * Replaces GenomeAssembly.get_rammappy_index / rammappy.Index.build (src/kaptive/core/genome.py:177-191): instead of
 * a minimizer index per assembly, the 2-bit packed contigs themselves are made resident (layout: kp_spec.h).
 *   words          : packed bases of all assemblies back to back (assembly a = words[asm_word_off[a] .. asm_word_off[a+1]))
 *   asm_word_off   : n_asm + 1 offsets in uint32 words; each assembly's length is a multiple of KP_ASM_ALIGN bases
 *   ctg_start/len  : per contig, start (multiple of KP_CONTIG_ALIGN) and length in the assembly's own padded space
 *   asm_first_ctg  : n_asm + 1 offsets into ctg_start/ctg_len
 *   n_runs         : [start,end) pairs of N runs, sorted per assembly, in the assembly's padded space
 *   asm_first_nrun : n_asm + 1 offsets into n_runs (in runs, not ints)
 * kp_batch_create copies from host memory; kp_batch_create_device adopts `words` already in device memory (it must
 * stay valid until kp_batch_destroy) and copies only the small tables.  kp_batch_create_async enqueues the copies on
 * the context's copy stream and returns: `words` must stay valid and unchanged until kp_batch_upload_wait (or the
 * batch's first kp_batch_wait) has returned -- the tables may be freed at once; kp_batch_align of the batch waits for
 * the copies on the device, so the upload of batch i+1 overlaps the alignment pass of batch i. */
KP_API int kp_batch_create(kp_ctx *ctx, int32_t n_asm, const uint32_t *words, const int64_t *asm_word_off,
                    const int32_t *ctg_start, const int32_t *ctg_len, const int32_t *asm_first_ctg,
                    const int32_t *n_runs, const int32_t *asm_first_nrun, kp_batch **out);
KP_API int kp_batch_create_async(kp_ctx *ctx, int32_t n_asm, const uint32_t *words, const int64_t *asm_word_off,
                          const int32_t *ctg_start, const int32_t *ctg_len, const int32_t *asm_first_ctg,
                          const int32_t *n_runs, const int32_t *asm_first_nrun, kp_batch **out);
KP_API int kp_batch_upload_wait(kp_ctx *ctx, kp_batch *batch);
/* `batch` adopted (kp_batch_create_device) the device words of `other`, a batch of another context on the same GPU whose
 * upload may still be in flight: alignment passes of `batch` then wait for that upload on the device.  `other` must
 * outlive `batch`. */
KP_API int kp_batch_depends_on(kp_ctx *ctx, kp_batch *batch, kp_batch *other);
KP_API int kp_batch_create_device(kp_ctx *ctx, int32_t n_asm, const uint32_t *d_words, const int64_t *asm_word_off,
                           const int32_t *ctg_start, const int32_t *ctg_len, const int32_t *asm_first_ctg,
                           const int32_t *n_runs, const int32_t *asm_first_nrun, kp_batch **out);
/* Device address of the batch's packed words (valid until kp_batch_destroy): lets a second context on the same GPU
 * type the same resident assemblies against another database via kp_batch_create_device instead of a second copy. */
KP_API const void *kp_batch_device_words(const kp_batch *batch);
KP_API void kp_batch_destroy(kp_batch *batch);

/* ---- alignment --------------------------------------------------------------------------------------------------
 * Replaces Aligner(...).map_batch(gene_seqs) with best_n=50000, pri_ratio=0.0 (src/kaptive/serotyping/core.py:
 * 148-154): every database gene against every contig of every assembly of the batch, all hits reported.
 * kp_batch_align enqueues the kernels (seed scan -> anchor sort -> band tasks -> banded Smith-Waterman) and returns;
 * kp_batch_wait blocks until they finish, then finalises the hit table (emission order of kp_spec.h).  */
KP_API int kp_batch_align(kp_ctx *ctx, kp_batch *batch);
KP_API int kp_batch_wait(kp_ctx *ctx, kp_batch *batch);
/* hit_off[n_asm+1]: hits of assembly a are rows hit_off[a] .. hit_off[a+1] of the table returned by kp_batch_hits.
 * These are the columns the reference reads off rammappy hit objects (src/kaptive/core/alignment.py:415-446). */
KP_API int kp_batch_hit_offsets(kp_ctx *ctx, kp_batch *batch, int64_t *hit_off);
KP_API int kp_batch_hits(kp_ctx *ctx, kp_batch *batch, kp_hit *out, int64_t cap);
/* Replaces the batch's finished hit table (valid after kp_batch_wait) with the caller's: rows hit_off[a] .. hit_off[a+1] of
 * `hits` become assembly a's hits, taken as they are -- emission order, mapq and all.  What follows (kp_batch_score,
 * kp_batch_reduce, kp_batch_typing) then reduces THAT table.  The reference's reduction takes any rammappy hit table
 * (src/kaptive/core/alignment.py:392-474, src/kaptive/serotyping/core.py:157-396); this is how hit tables no aligner would
 * produce (equal scores, mapq 0 / 255 / 1 ties: src/kaptive/core/alignment.py:669-675) reach the device reduction in the
 * parity tests. */
KP_API int kp_batch_set_hits(kp_ctx *ctx, kp_batch *batch, const kp_hit *hits, const int64_t *hit_off);
/* CIGARs of the batch's hits (kp_spec.h, CIGAR): what the reference gets from Aligner(..., do_cigar=True)
 * (src/kaptive/serotyping/core.py:148) and keeps in Alignments.cigars (src/kaptive/core/alignment.py:872).  Only for a batch
 * whose kp_batch_align ran with the option `cigar` set (kp_ctx_set_option(ctx, "cigar", 1); default 0: nothing is computed,
 * allocated or launched for them) -- otherwise, and after kp_batch_set_hits, both calls return KP_ESTATE.
 *   kp_batch_cigar_offsets : cigar_off[total_hits + 1], rows as kp_batch_hits lists them: the ops of hit i are
 *                            ops[cigar_off[i] .. cigar_off[i + 1])
 *   kp_batch_cigars        : the ops, len << 4 | op with M = 0, I = 1, D = 2 (BAM), in the order of increasing target
 *                            position; KP_EINVAL when cap < cigar_off[total_hits]
 * The option `cigar_ops_per_hit` is the first guess for the size of the ops buffer (default 4); the context learns what its
 * batches need, and a buffer that was too small is grown and the ops written again without another alignment pass. */
KP_API int kp_batch_cigar_offsets(kp_ctx *ctx, kp_batch *batch, int64_t *cigar_off);
KP_API int kp_batch_cigars(kp_ctx *ctx, kp_batch *batch, uint32_t *ops, int64_t cap);
/* cs difference strings of the batch's hits (kp_spec.h, CS): minimap2's short form of the cs:Z: tag, which says which bases
 * differ where the CIGAR says only where the gaps are.  The reference's Alignments carries a cs column that it never fills
 * (do_cs=False).  Only for a batch whose kp_batch_align ran with the option `cs` set (default 0: nothing is computed, allocated
 * or launched for them; cs = 1 computes the CIGARs too, whatever `cigar` says) -- otherwise, and after kp_batch_set_hits, both
 * calls return KP_ESTATE.
 *   kp_batch_cs_offsets : cs_off[total_hits + 1], rows as kp_batch_hits lists them: the string of hit i is
 *                         bytes[cs_off[i] .. cs_off[i + 1]) (no terminator)
 *   kp_batch_cs         : the bytes; KP_EINVAL when cap < cs_off[total_hits]
 * The option `cs_bytes_per_hit` is the first guess for the size of the byte buffer (default 64); the context learns what its
 * batches need, and a buffer that was too small is grown and the bytes written again: no other kernel is rerun. */
KP_API int kp_batch_cs_offsets(kp_ctx *ctx, kp_batch *batch, int64_t *cs_off);
KP_API int kp_batch_cs(kp_ctx *ctx, kp_batch *batch, char *bytes, int64_t cap);
/* counters of the last kp_batch_align: [0] anchors, [1] band tasks, [2] DP cells, [3] hits, [4] overflow retries */
KP_API int kp_batch_stats(kp_ctx *ctx, kp_batch *batch, int64_t *stats5);

/* Stage durations of the most recent alignment pass of this batch (valid after kp_batch_wait), from HIP events the
 * library records on the context's stream around every pass: ms7 = seed scan (kp_scan_kernel), candidate expansion +
 * anchor compaction + sort, chaining + task ordering, banded SW fill (all band widths run in one launch: ms7[3]), its
 * traceback (ms7[4]); ms7[5..6] are 0 and kept for layout stability.  bytes_scanned receives the algorithmic bytes the scan kernel
 * streams (4 * total words). */
KP_API int kp_batch_profile(kp_ctx *ctx, kp_batch *batch, float *ms7, int64_t *bytes_scanned);

/* Stage outputs for stage-by-stage parity tests (valid after kp_batch_wait): sorted anchor keys of one assembly, and
 * the band tasks of one assembly as 8 x int32 rows (gs, contig, lo, width, n_anchors, qmin, qmax, chain_score) in device
 * order. */
KP_API int64_t kp_batch_anchors(kp_ctx *ctx, kp_batch *batch, int32_t asm_index, uint64_t *out, int64_t cap);
KP_API int64_t kp_batch_tasks(kp_ctx *ctx, kp_batch *batch, int32_t asm_index, int32_t *out8, int64_t cap);
/* ... and what the banded Smith-Waterman made of each of those tasks, row for row in the order of kp_batch_tasks: 7 x
 * int32 (score, q_start, q_end, t_start, t_end, matches, block_len).  Tasks whose best cell stays below the score
 * cut-off (KP_MIN_DP_SCORE) are not traced back: their row holds the score and zeros. */
KP_API int64_t kp_batch_task_results(kp_ctx *ctx, kp_batch *batch, int32_t asm_index, int32_t *out7, int64_t cap);
/* ... and the JOINS of one assembly (kp_spec.h, kp-align v5: chains of a group's anchors across diagonal jumps of up to KP_JOIN_BW, the
 * stand-in for minimap2's bw = 500 chaining inside rammappy's map_batch, src/kaptive/serotyping/core.py:147-155), in device
 * order, KP_JOIN_ROW_INTS x int32 each: gs, contig, n_pieces, n_anchors, chain_score, width, lo[KP_JOIN_MAX_PIECES], then per
 * piece 11 values -- state (0 nothing, 1 joined hit, 2 rejected by the drop test), mask of the pieces its path visits, cell
 * score, q_start, q_end, t_start, t_end (query as aligned, target in assembly coordinates), matches, block_len, reported
 * score, order-score bonus. */
#define KP_JOIN_ROW_INTS (6 + KP_JOIN_MAX_PIECES + 11 * KP_JOIN_MAX_PIECES)
KP_API int64_t kp_batch_joins(kp_ctx *ctx, kp_batch *batch, int32_t asm_index, int32_t *out, int64_t cap);
/* ... and what the OCCURRENCE CUT (kp_spec.h) left for one assembly, as uint32 words: [0] its state (bit 0: a gene seed with
 * more than KP_MID_OCC anchors, bit 1: the assembly's own mid_occ decides: it claimed a counting table), [1] the mid_occ
 * it was cut at (KP_MID_OCC without a table), then, with a table, the table's non-empty entries as (seed value, count)
 * pairs in table order: the assembly's distinct minimizers and how often each occurs.  Returns the number of words. */
KP_API int64_t kp_batch_occ(kp_ctx *ctx, kp_batch *batch, int32_t asm_index, uint32_t *out, int64_t cap);
/* ... and the seed scan's own output, the CANDIDATE LIST of the batch's last pass, as uint64 words: [0] how many the streaming
 * kernel listed (the front of the list), [1] how many the edge kernel listed (its back), then the front words in list order and
 * the back words in the order they were appended.  A word is (batch-wide base position << 31) | (strand bit << 30) | seed value.
 * The order of either part depends on the order in which waves and threads finished: compare them as sets.  A null `out` returns
 * the number of words; a buffer of fewer words is refused with nothing written; a pass whose list overflowed is never a batch's
 * last one, and is refused, not returned cut short. */
KP_API int64_t kp_batch_candidates(kp_ctx *ctx, kp_batch *batch, uint64_t *out, int64_t cap);

/* ---- batched typing: hit table -> per-assembly records -----------------------------------------------------------------
 * Replaces, for a whole batch, the reduction Serotyper.__call__ runs per genome after the aligner returns
 * (src/kaptive/serotyping/core.py:157-396): per-gene best coverage and locus scores, overlap cull, clustering, locus
 * pieces, inside/expected flags, missing genes, gene extraction + translation, protein identity, gene states.  Three
 * float steps stay with the caller in numpy because only numpy reproduces their bits (kaptive_amd/serotyping/batch.py):
 * the completeness**3 penalty and argmax between kp_batch_score and kp_batch_reduce, the argsort of piece positions
 * and the float32 mean identity afterwards.
 *
 * kp_db_load_typing: the Database columns the reduction reads (src/kaptive/db/core.py:82-98), host pointers; call it
 *   after kp_db_load (the gene count and gene lengths come from there). */
typedef struct kp_typing_tables {
    const uint16_t *gene_locus;    /* Database.gene_locus_indices */
    const uint8_t *gene_extra;     /* Database.extra_genes */
    const uint16_t *gene_pos;      /* Database.gene_positions */
    const int8_t *gene_strand;     /* Database.gene_intervals.strands */
    const int32_t *locus_gene_off; /* Database.locus_gene_offsets */
    const int32_t *locus_gene_len; /* Database.locus_gene_lengths */
    int32_t n_loci;
    const uint8_t *prot;           /* Database.translations.seqs (stop codons kept) */
    const int32_t *prot_off, *prot_len;
} kp_typing_tables;
KP_API int kp_db_load_typing(kp_ctx *ctx, const kp_typing_tables *tables);
/* Several databases in one context (typing groups).  The reference types an assembly against the K database and then
 * against the O database, aligning each database's genes in its own map_batch call (src/kaptive/serotyping/cli.py:183-210
 * runs one Serotyper per database).  Here the genes of all databases can be loaded into one context back to back
 * (kp_db_load over the concatenation) so that an assembly's bases are scanned, sorted, chained and aligned once; the
 * hit table is sorted by gene, so every database's reduction gets its own contiguous run of it.
 *   kp_db_load_typing_group: typing tables of the database whose genes are [gene_lo, gene_hi) of the context's genes
 *     (tables index genes relative to gene_lo); group is a small caller-chosen index < KP_MAX_TYPING_GROUPS.
 *     kp_db_load_typing(ctx, t) is kp_db_load_typing_group(ctx, 0, 0, n_genes, t).
 *   kp_batch_use_group: the group that kp_batch_score / kp_batch_reduce / kp_batch_typing_caps / kp_batch_typing /
 *     kp_batch_proteins address from now on (0 after kp_batch_create); every group keeps its own results. */
#define KP_MAX_TYPING_GROUPS 16
KP_API int kp_db_load_typing_group(kp_ctx *ctx, int32_t group, int32_t gene_lo, int32_t gene_hi,
                                   const kp_typing_tables *tables);
KP_API int kp_batch_use_group(kp_ctx *ctx, kp_batch *batch, int32_t group);
/* After kp_batch_align: finalises the hit tables on the device and returns locus_scores (float64, sum of best query
 * coverages per locus, core.py:188-193) and locus_counts (genes counted, core.py:196-198), both [n_asm][n_loci]. */
KP_API int kp_batch_score(kp_ctx *ctx, kp_batch *batch, double min_gene_coverage, double *locus_scores,
                          int32_t *locus_counts);
/* Enqueues the rest of the reduction for the caller's choice of best locus per assembly (core.py:206). */
KP_API int kp_batch_reduce(kp_ctx *ctx, kp_batch *batch, const int32_t *best_locus, const kp_typing_params *params);
/* kp_batch_typing_caps waits for the reduction and reports the largest number of kept hits / pieces any assembly of the
 * batch has (at least 1): the smallest strides kp_batch_typing accepts.  kp_batch_typing copies out one summary per
 * assembly and its kept hits / pieces at kept[a * kept_stride], pieces[a * piece_stride]. */
KP_API int kp_batch_typing_caps(kp_ctx *ctx, kp_batch *batch, int32_t *kept_cap, int32_t *piece_cap);
KP_API int kp_batch_typing(kp_ctx *ctx, kp_batch *batch, kp_asm_summary *summaries, kp_kept *kept, int32_t kept_stride,
                           kp_piece *pieces, int32_t piece_stride);
/* Translated proteins of one assembly (kp_kept.prot_off/prot_len index into it); returns bytes copied. */
KP_API int kp_batch_proteins(kp_ctx *ctx, kp_batch *batch, int32_t asm_index, uint8_t *out, int64_t cap);
/* Variant records of the kept hits (kp_spec.h, VARIANTS): for every record of the kept lists kp_batch_typing returns, which bases
 * of the contig differ from the database's gene -- in the gene's forward coordinates -- and what a substituted base does to its
 * codon.  The reference has no such output.  Only for a batch whose kp_batch_align ran with the option `variants` set (default 0:
 * nothing is computed, allocated or launched for them; variants = 1 computes the CIGARs too, whatever `cigar` says), after
 * kp_batch_reduce, for the group kp_batch_use_group chose.  Without ops for the current hit table -- the option was off, or
 * kp_batch_set_hits replaced the table -- both calls return KP_EINVAL and kp_last_error names the cause; the context types its
 * next batch as usual.  The records are made on the first of these calls after a reduction (three kernels on the reduction's
 * stream) and kept until the next kp_batch_reduce of the group, the batch's next kp_batch_align or kp_batch_set_hits.
 *   kp_batch_variant_offsets : var_off[n_asm + 1]: the records of assembly a are variants[var_off[a] .. var_off[a + 1])
 *   kp_batch_variants        : the records, hits in kept-list order, ascending in q_pos within a hit; KP_EINVAL when
 *                              cap < var_off[n_asm]
 * The option `variants_per_kept` is the first guess for the size of the record buffer (default 8 per kept record); the context
 * learns what its batches need, and a buffer that was too small is grown and the records stored again: no alignment pass and no
 * reduction is rerun, and the retries kp_batch_stats counts stay as they were.  A second overflow is KP_EOVERFLOW. */
KP_API int kp_batch_variant_offsets(kp_ctx *ctx, kp_batch *batch, int64_t *var_off);
KP_API int kp_batch_variants(kp_ctx *ctx, kp_batch *batch, kp_variant *out, int64_t cap);
/* Breakpoint records of the kept lists (kp_spec.h, BREAKPOINTS): which two records of a kept list are fragments of one gene -- cut by
 * an insertion longer than the aligner joins across, a deletion, an inversion or a contig end --, the gaps between them on the gene
 * and on the contig, the distances of the junction to the contig ends and the inverted repeat at the ends of an inserted stretch.
 * The reference has no such output.  For the group kp_batch_use_group chose, after kp_batch_reduce; they need no option and no ops,
 * so a hit table that kp_batch_set_hits put in place serves as well.  Without a reduction of the group's current hit table both calls
 * return KP_EINVAL and kp_last_error names the cause; the context types its next batch as usual.  The records are made on the first
 * of these calls after a reduction (three kernels on the reduction's stream; nothing is allocated or launched if nobody asks) and
 * kept until the next kp_batch_reduce of the group, the batch's next kp_batch_align or kp_batch_set_hits.  A record per kept record
 * is an upper bound, so there is no buffer option and nothing is retried.
 *   kp_batch_breakpoint_offsets : bp_off[n_asm + 1]: the records of assembly a are breakpoints[bp_off[a] .. bp_off[a + 1])
 *   kp_batch_breakpoints        : the records, ascending in kept_b within an assembly; KP_EINVAL when cap < bp_off[n_asm] */
KP_API int kp_batch_breakpoint_offsets(kp_ctx *ctx, kp_batch *batch, int64_t *bp_off);
KP_API int kp_batch_breakpoints(kp_ctx *ctx, kp_batch *batch, kp_breakpoint *out, int64_t cap);
/* Allele digests of the kept records and the locus pieces (kp_spec.h, ALLELES): a stable 64-bit digest of every kept record's
 * strand-corrected bases and of its protein bytes, and of every locus piece's bases -- what tells whether two isolates carry the
 * same allele of a gene, the same protein or the same locus.  The reference has no such output.  Laid out like kp_batch_typing:
 * out[a * kept_stride + i] belongs to kept record i of assembly a, piece_out[a * piece_stride + p] to its piece p; rows beyond the
 * counts are zero; strides smaller than the counts give KP_EINVAL (kp_batch_typing_caps).  Lifetime and refusals are those of
 * kp_batch_breakpoints: for the group kp_batch_use_group chose, after kp_batch_reduce, no option and no ops needed, a table that
 * kp_batch_set_hits put in place serves; made on the first call after a reduction (one kernel on the reduction's stream; nothing is
 * allocated or launched if nobody asks) and kept until the group's next kp_batch_reduce, the batch's next kp_batch_align or
 * kp_batch_set_hits; without a current reduction KP_EINVAL, and kp_last_error names the cause.  One record per kept row and per
 * piece row: nothing overflows, nothing is retried.  The locus digest of an assembly is kp_format_alleles' to combine. */
KP_API int kp_batch_alleles(kp_ctx *ctx, kp_batch *batch, kp_allele *out, int32_t kept_stride, uint64_t *piece_out, int32_t piece_stride);
/* Aligned rows of the kept hits (kp_spec.h, ALIGNED ROWS; option "aligned"): every kept record's contig bases projected through its
 * CIGAR onto the coordinates of the database's gene -- gene_len columns, sixteen to a 64-bit block --, so that the rows of one gene
 * from any number of batches stack into a multiple alignment.  The reference has no such output.  Option "aligned" (0 | 1) takes
 * effect from the next kp_batch_align; such a pass computes the CIGARs too, whatever "cigar" says, exactly as "variants" does.
 * Lifetime and refusals are those of kp_batch_variants: for the group kp_batch_use_group chose, after kp_batch_reduce; made on the
 * first call after a reduction (kernels on the reduction's stream; with the option off nothing is computed, allocated or launched)
 * and kept until the group's next kp_batch_reduce, the batch's next kp_batch_align or kp_batch_set_hits.  Without ops for the current
 * hit table -- the option was off, or kp_batch_set_hits replaced the table -- KP_EINVAL, and kp_last_error names the cause; the
 * context types its next batch as usual.  Sizes are exact: one record per kept row, (gene_len + 15) / 16 blocks per row.
 *   kp_batch_aligned_size   : the blocks of all rows
 *   kp_batch_aligned_rows   : the row of record i of assembly a at rows[a * kept_stride + i] (laid out like kp_batch_typing; rows
 *                             beyond the counts are zero; a stride smaller than a count gives KP_EINVAL)
 *   kp_batch_aligned_blocks : the blocks, rows back to back in kept-list order; KP_EINVAL when cap < n_blocks */
KP_API int kp_batch_aligned_size(kp_ctx *ctx, kp_batch *batch, int64_t *n_blocks);
KP_API int kp_batch_aligned_rows(kp_ctx *ctx, kp_batch *batch, kp_aligned_row *rows, int32_t kept_stride);
KP_API int kp_batch_aligned_blocks(kp_ctx *ctx, kp_batch *batch, uint64_t *out, int64_t cap);
/* Rescue records of the missing genes (kp_spec.h, RESCUE; options "rescue" (0 | 1) and "rescue_flank" (0 .. KP_RESCUE_FLANK_MAX, default
 * KP_RESCUE_FLANK)): every gene the reduction lists as missing is looked for by aligning its database protein against the six-frame
 * translation of the contig around every locus piece -- Kaptive 2 searched genes with tblastn; a nucleotide seed does not land in a
 * gene below 75-80 % identity.  One record per missing gene, in ascending gene order.  For the group kp_batch_use_group chose, after
 * kp_batch_reduce; made on the first call after a reduction (kernels on the reduction's stream) and kept until the group's next
 * kp_batch_reduce, the batch's next kp_batch_align or kp_batch_set_hits, or a call with another rescue_flank.  The options are read
 * when the records are asked for: no alignment pass and no reduction does anything for them, and with "rescue" off nothing is
 * computed, allocated or launched -- both calls then return KP_EINVAL, as they do without a current reduction, and kp_last_error
 * names the cause.  Sizes are exact: nothing overflows, nothing is retried.
 *   kp_batch_rescue_offsets : rescue_off[n_asm + 1]: the records of assembly a are out[rescue_off[a] .. rescue_off[a + 1])
 *   kp_batch_rescue         : the records; KP_EINVAL when cap < rescue_off[n_asm] */
KP_API int kp_batch_rescue_offsets(kp_ctx *ctx, kp_batch *batch, int64_t *rescue_off);
KP_API int kp_batch_rescue(kp_ctx *ctx, kp_batch *batch, kp_rescue *out, int64_t cap);

/* ---- report rows (host only) -----------------------------------------------------------------------------------------------
 * Replaces KaptiveRow.from_result + bytes(row) per genome (src/kaptive/serotyping/io.py:191-296, 37-43): the TSV lines
 * of a whole batch from the records kp_batch_typing returned and the per-assembly decisions the caller finished
 * (phenotype rules, typeability, problems: src/kaptive/serotyping/core.py:398-459, models.py:538-558).  Strings are
 * byte blobs with n + 1 offsets.  Returns the number of bytes the rows need (written to `out` while they fit `cap`), or
 * a negative error code.  No GPU involved. */
typedef struct kp_row_tables {   /* per database */
    const char *prefix;          /* "<Kaptive version>\t<database name>\t<database version>\t" */
    int32_t prefix_len;
    const char *gene_ids;        /* Database.genes.ids */
    const int32_t *gene_id_off;
    const char *locus_names;     /* Database.loci.ids */
    const int32_t *locus_name_off;
    const int32_t *locus_gene_off, *locus_gene_len;
} kp_row_tables;
typedef struct kp_row_columns {  /* per assembly of the batch */
    const char *asm_ids;
    const int32_t *asm_id_off;
    const char *phenotypes;      /* Best match type */
    const int32_t *phenotype_off;
    const int32_t *best_locus;
    const uint8_t *typeable;
    const int32_t *problems;     /* bit 0..4 = ? + - * ! */
    const double *identity, *coverage, *length_discrepancy; /* NaN discrepancy -> n/a */
} kp_row_columns;
KP_API int64_t kp_format_rows(const kp_row_tables *tables, int32_t n_asm, const kp_asm_summary *summaries,
                              const kp_kept *kept, int32_t kept_stride, const kp_row_columns *columns, char *out,
                              int64_t cap);

/* ---- PAF lines of a hit table (host only) -------------------------------------------------------------------------------------
 * One line per hit, in the table's order, as minimap2 -c writes a mapping: gene name, gene length, q_start, q_end, strand,
 * contig name, contig length, t_start, t_end, matches, block_len, mapq, AS:i:<score>, NM:i:<block_len - matches>,
 * cg:Z:<ops>; tab-separated, '\n' at the end.  Names are byte blobs with n + 1 offsets; the contigs of all assemblies lie
 * back to back, assembly a's are asm_first_ctg[a] .. asm_first_ctg[a + 1].  Returns the number of bytes the lines need
 * (written to `out` while they fit `cap`), or a negative error code (KP_EINVAL also for a hit that names a gene or contig
 * the tables do not have). */
typedef struct kp_paf_tables {
    const char *gene_names;
    const int32_t *gene_name_off;
    const int32_t *gene_len;
    int32_t n_genes;
    const char *ctg_names;
    const int64_t *ctg_name_off;
    const int32_t *ctg_len;
    const int64_t *asm_first_ctg; /* n_asm + 1 */
} kp_paf_tables;
KP_API int64_t kp_format_paf(const kp_paf_tables *tables, int32_t n_asm, const kp_hit *hits, const int64_t *hit_off,
                             const uint32_t *ops, const int64_t *cigar_off, char *out, int64_t cap);
/* The same lines with what the cs strings add (cs / cs_off as kp_batch_cs returns them; may be null when flags == 0):
 *   KP_PAF_CS  : "\tcs:Z:<string>" after cg:Z:
 *   KP_PAF_EQX : cg:Z: in =/X form (minimap2 --eqx), derived from the cs bytes (kp_spec.h, CS)
 * flags == 0 gives the bytes of kp_format_paf.  A cs string that breaks the grammar or the canonical form, or whose column
 * totals disagree with the hit's ops, is KP_EINVAL. */
#define KP_PAF_CS 1
#define KP_PAF_EQX 2
KP_API int64_t kp_format_paf_tags(const kp_paf_tables *tables, int32_t n_asm, const kp_hit *hits, const int64_t *hit_off,
                                  const uint32_t *ops, const int64_t *cigar_off, const char *cs, const int64_t *cs_off, int32_t flags,
                                  char *out, int64_t cap);

/* ---- variant table of a batch (host only) -------------------------------------------------------------------------------------
 * One tab-separated line per variant record, in the records' order: Assembly, Contig, Position (1-based, contig forward strand),
 * Strand (of the hit), Gene, Gene position (1-based, gene forward strand), Type (snv / ins / del), Length, Ref, Alt (gene-strand
 * letters of an SNV, n for an ambiguous base; "." for ins and del), Codon (1-based), Ref aa, Alt aa ("." for ins and del) and
 * Effect: for an SNV ambiguous (a side is n), synonymous (same amino acid), nonsense (alt is a stop, ref is not), stop_lost (ref is
 * a stop, alt is not) or missense; for ins and del frameshift when Length % 3 != 0, else inframe.  No header line.  kept /
 * kept_stride as kp_batch_typing filled them, variants / var_off as kp_batch_variants / kp_batch_variant_offsets did.  Names are
 * byte blobs with n + 1 offsets, the contigs of all assemblies back to back as in kp_paf_tables.  Returns the number of bytes the
 * lines need (written to `out` while they fit `cap`), or a negative error code (KP_EINVAL also for a record that names a kept
 * record, gene or contig the tables do not have, or whose kind is unknown). */
typedef struct kp_variant_tables {
    const char *gene_names;
    const int32_t *gene_name_off;
    int32_t n_genes;
    const char *asm_names;
    const int64_t *asm_name_off;  /* n_asm + 1 */
    const char *ctg_names;
    const int64_t *ctg_name_off;
    const int64_t *asm_first_ctg; /* n_asm + 1 */
} kp_variant_tables;
KP_API int64_t kp_format_variants(const kp_variant_tables *tables, int32_t n_asm, const kp_kept *kept, int32_t kept_stride,
                                  const kp_variant *variants, const int64_t *var_off, char *out, int64_t cap);

/* ---- breakpoint table of a batch (host only) -----------------------------------------------------------------------------------
 * One tab-separated line per breakpoint record, in the records' order: Assembly, Gene, Event, Gene position (q_end of fragment a:
 * its last gene base, 1-based), Gene gap (q_gap), Contig A, Position A (1-based), Strand A, Contig B, Position B, Strand B, Length
 * (t_gap; "." unless COLLINEAR), Duplication (max(0, -q_gap)), Edge A, Edge B and Inverted repeat (matches/cols; "." when ir_cols is
 * 0).  Event: for COLLINEAR insertion (q_gap <= 0 < t_gap), deletion (t_gap <= 0 < q_gap), replacement (both > 0) or overlap (both
 * <= 0); inversion for INVERTED; rearrangement for DISORDERED; for CONTIGS contig_break when both edges are <= edge_tolerance, else
 * translocation.  No header line.  Tables, kept / kept_stride and the return value as kp_format_variants has them (KP_EINVAL also
 * for a record that names a kept record, gene or contig the tables do not have, or whose kind is unknown). */
KP_API int64_t kp_format_breakpoints(const kp_variant_tables *tables, int32_t n_asm, const kp_kept *kept, int32_t kept_stride,
                                     const kp_breakpoint *breakpoints, const int64_t *bp_off, int32_t edge_tolerance, char *out, int64_t cap);

/* ---- allele table of a batch (host only) ----------------------------------------------------------------------------------------
 * One tab-separated line per kept record without KP_F_SPURIOUS, in kept-list order, assemblies in batch order: Assembly, Locus (the
 * best-match locus's name), Locus allele, Gene, Set (expected / other / extra from KP_F_EXPECTED / KP_F_EXTRA, then _in / _out from
 * KP_F_INSIDE), Contig, Start, End (1-based and closed, contig forward strand), Strand, State (normal / partial / truncated /
 * below_id_threshold), Length (t_end - t_start), Allele, Protein length, Protein allele.  Digests are 16 lower-case hex digits;
 * Locus allele is "." for an assembly without a piece, Protein allele "." for a record with prot_len == 0 (kp_spec.h, ALLELES).  No
 * header line.  Tables are kp_variant_tables plus the locus names; n_kept / n_pieces / best_locus per assembly as the summaries and
 * the host's choice have them; kept / alleles with kept_stride and piece_digests / piece_order with piece_stride as
 * kp_batch_typing and kp_batch_alleles filled them, piece_order as kp_format_json takes it (numpy's argsort of mean_pos per
 * assembly).  Return value as kp_format_variants has it; KP_EINVAL also for a count beyond its stride, a best locus, gene or contig
 * the tables do not have, an order entry outside the assembly's pieces or an unknown state.
 * kp_allele_locus_digest: the locus digest of n pieces listed in `order` (0 for n <= 0) -- the one the table prints. */
typedef struct kp_allele_tables {
    kp_variant_tables names;
    const char *locus_names;
    const int32_t *locus_name_off; /* n_loci + 1 */
    int32_t n_loci;
} kp_allele_tables;
KP_API int64_t kp_format_alleles(const kp_allele_tables *tables, int32_t n_asm, const int32_t *n_kept, const int32_t *n_pieces, const int32_t *best_locus,
                                 const kp_kept *kept, const kp_allele *alleles, int32_t kept_stride, const uint64_t *piece_digests,
                                 const int32_t *piece_order, int32_t piece_stride, char *out, int64_t cap);
KP_API uint64_t kp_allele_locus_digest(const uint64_t *piece_digests, const int32_t *order, int32_t n);

/* ---- aligned table of a batch (host only) ---------------------------------------------------------------------------------------
 * One tab-separated line per kept record without KP_F_SPURIOUS, in kept-list order, assemblies in batch order: Assembly, Gene, Contig,
 * Start, End (1-based and closed, contig forward strand), Strand, Gene length, Gene start, Gene end (1-based and closed, on the
 * gene), Covered, Inserted, Insertions, Aligned -- the row (kp_spec.h, ALIGNED ROWS) as acgt, n and -, exactly Gene length
 * characters.  No header line.  Tables as kp_format_variants takes them; n_kept per assembly as the summaries have it; kept and rows
 * with kept_stride and blocks / n_blocks as kp_batch_typing and kp_batch_aligned_rows / _blocks / _size filled them.  Return value as
 * kp_format_variants has it; KP_EINVAL also for a count beyond the stride, a row whose off or gene_len runs outside `blocks`, or a
 * gene or contig the tables do not have. */
KP_API int64_t kp_format_aligned(const kp_variant_tables *tables, int32_t n_asm, const int32_t *n_kept, const kp_kept *kept, int32_t kept_stride,
                                 const kp_aligned_row *rows, const uint64_t *blocks, int64_t n_blocks, char *out, int64_t cap);

/* ---- rescue table of a batch (host only) ----------------------------------------------------------------------------------------
 * One tab-separated line per rescue record, in the records' order: Assembly, Locus (the best-match locus's name), Gene, Protein length
 * (of the database's protein, its trailing * included), Call, Score, Contig, Start, End (1-based and closed, contig forward strand),
 * Strand, Frame (1..3), Protein start (1-based), Protein end, Matches, Mismatches, Gaps, Identity (matches * 100 / (matches +
 * mismatches + gaps), %.2f), Coverage ((p_end - p_start) * 100 / protein length, %.2f), Stops and Edge (start / end / both / .).  A
 * record with score 0 has "." in every column from Contig to Protein end.  Call is the first that applies of: absent (score <
 * min_score), interrupted (a stop inside the aligned stretch: stops > 0, not counting the gene's own stop where the alignment reaches the
 * protein's trailing *), partial (edge != 0 and coverage < 90), fragment (coverage < 90), diverged; the 90 is the
 * reference's TRUNCATED rule (prot_cov < 0.90).  No header line.  Tables are kp_allele_tables; prot_len the database's protein lengths
 * by gene; best_locus per assembly as the host chose it; records / rescue_off as kp_batch_rescue / kp_batch_rescue_offsets filled
 * them.  Return value as kp_format_variants has it; KP_EINVAL also for a best locus, gene or contig the tables do not have. */
KP_API int64_t kp_format_rescue(const kp_allele_tables *tables, int32_t n_asm, const int32_t *prot_len, const int32_t *best_locus, const kp_rescue *records,
                                const int64_t *rescue_off, int32_t min_score, char *out, int64_t cap);

/* ---- pairwise locus distances (kp_spec.h, DISTANCES) -----------------------------------------------------------------------------
 * The one result that spans batches: the caller collects the locus rows of every assembly of a run that carries one locus and hands
 * them over as a matrix.  The handle holds the matrix's bit planes on the device and nothing else of the context's; it needs no
 * database and no batch, and a run that never creates one allocates and launches nothing for it.
 *   kp_dist_create : blocks is the [n_rows, n_blocks] matrix of locus rows, row-major, padding flagged; it is uploaded and turned
 *                    into planes.  KP_EINVAL for null pointers, n_rows < 0, n_blocks <= 0 with n_rows > 0, 16 * n_blocks >= 2^31
 *                    and n_rows > KP_DIST_MAX_ROWS (kp_caps.h).  n_rows of 0 or 1 is valid and gives 0 pairs.
 *   kp_dist_count  : counts the listed pairs for (max_diff, min_compared) into *n_pairs.
 *   kp_dist_pairs  : the pairs of the last kp_dist_count, ascending (a, b); KP_ESTATE without one, KP_EINVAL if cap is short.
 *   kp_dist_destroy: frees the handle's device memory (while its context lives; a null handle is ignored).
 * kp_device_allocations does not count what a handle does: it shows whether a stream of batches has settled, and a handle works
 * outside that stream.  Its planes and tables are allocated once, in kp_dist_create; only the record buffer is replaced -- freed
 * and allocated anew, which waits for the device like any allocation -- when a listing is longer than every one before it. */
typedef struct kp_dist kp_dist;
KP_API int kp_dist_create(kp_ctx *ctx, const uint64_t *blocks, int32_t n_rows, int64_t n_blocks, kp_dist **out);
KP_API int kp_dist_count(kp_ctx *ctx, kp_dist *d, int32_t max_diff, int32_t min_compared, int64_t *n_pairs);
KP_API int kp_dist_pairs(kp_ctx *ctx, kp_dist *d, kp_dist_pair *out, int64_t cap);
KP_API void kp_dist_destroy(kp_dist *d);
/* The distance table of one locus (host only): one tab-separated line per pair, in the pairs' order: Locus, Assembly A, Assembly B,
 * Columns (the locus's total gene length), Compared, Differences, Unshared.  No header line.  names / name_off [n_names + 1]: the
 * assemblies' names by row of the matrix.  Return value as kp_format_variants has it; KP_EINVAL also for a pair that names a row
 * outside [0, n_names). */
KP_API int64_t kp_format_distances(const char *locus_name, int32_t locus_name_len, int64_t columns, const char *names, const int64_t *name_off,
                                   int32_t n_names, const kp_dist_pair *pairs, int64_t n_pairs, char *out, int64_t cap);
/* Clusters and nearest neighbours of a handle's rows (kp_spec.h, CLUSTERS): one pass over the same tiles, no pair stored.
 *   labels [n_levels][n_rows]: every row's label at every level; may be null when n_levels == 0.
 *   nearest [n_rows]: every row's nearest record; may be null, then the nearest pass stores nothing.
 * KP_EINVAL for a null context or handle, a handle of another device, n_levels outside [0, KP_CLUST_MAX_LEVELS], levels that are
 * negative or do not strictly ascend, null levels with n_levels > 0, and null labels with n_levels > 0 and n_rows > 0.  n_rows of 0
 * and 1 are valid; one row has label 0 and no neighbour.  The call leaves the handle's listing state alone: a kp_dist_pairs that
 * follows a kp_dist_count works with a kp_dist_clusters between them.  Its tables are the handle's own, allocated once, on the
 * first call; like everything a handle does, kp_device_allocations does not count them. */
KP_API int kp_dist_clusters(kp_ctx *ctx, kp_dist *d, const int32_t *levels, int32_t n_levels, int32_t min_compared,
                            int32_t *labels /* [n_levels][n_rows], may be null when n_levels == 0 */,
                            kp_dist_nearest *nearest /* [n_rows], may be null: then no nearest pass output */);
/* The cluster table of one locus (host only): one tab-separated line per row, in row order: Locus, Assembly, one cluster number
 * per level (the 1-based rank of the row's label among its level's labels), Nearest (the neighbour's name, "." for none),
 * Differences, Compared, Unshared ("." for none).  No header line.  names / name_off [n_names + 1]: the assemblies' names; row i of
 * the matrix is named names[rows[i]], or names[i] when rows is null; labels [n_levels][n_names] and nearest [n_names] as
 * kp_dist_clusters filled them.  Return value as kp_format_variants has it; KP_EINVAL also for a label, a neighbour or an entry of
 * rows outside [0, n_names), a label larger than its row or one that is not its own label, and n_levels outside [0,
 * KP_CLUST_MAX_LEVELS]. */
KP_API int64_t kp_format_clusters(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off,
                                  int32_t n_names, const int32_t *rows /* [n_names] or null */, int32_t n_levels,
                                  const int32_t *labels, const kp_dist_nearest *nearest, char *out, int64_t cap);
/* The minimum spanning forest of a handle's rows (kp_spec.h, TREE): Boruvka's rounds over the same tiles, no pair stored.
 *   edges [cap]: the forest's *n_edges = n_rows - (number of trees) records, ascending by (differences, a, b).
 *   component [n_rows]: the smallest row of every row's tree; may be null.
 * KP_EINVAL for a null context, handle or n_edges, a handle of another device, cap < n_rows - 1 with n_rows > 1, null edges with
 * cap > 0, and a matrix of 16 * n_blocks >= 2^28 columns, which does not fit the packed edge key (KP_TREE_MAX_COLUMNS, kp_caps.h;
 * the other calls of the handle keep their own limit).  min_compared as kp_dist_clusters takes it.  n_rows of 0 and 1 are valid:
 * no edge, and one row is its own component.  KP_ESTATE if the rounds reach their bound (ceil(log2 n_rows) + 1) with edges still
 * arriving; no matrix does that.  The call leaves the handle's listing state and its cluster tables alone.  Its tables are the
 * handle's own, allocated once, on the first call; like everything a handle does, kp_device_allocations does not count them.
 *   kp_dist_tree_rounds: the rounds the handle's last kp_dist_tree ran, the empty last one included (0: none ran). */
KP_API int kp_dist_tree(kp_ctx *ctx, kp_dist *d, int32_t min_compared, kp_dist_pair *edges, int64_t cap, int64_t *n_edges,
                        int32_t *component /* [n_rows], may be null */);
KP_API int32_t kp_dist_tree_rounds(const kp_dist *d);
/* The Newick table of one locus (host only): one tab-separated line per tree of the forest, ascending in the tree's smallest row:
 * Locus, Tree (the 1-based rank of the component's label), Assemblies (its rows), Newick (kp_spec.h, TREE, NEWICK).  No header
 * line.  names / name_off [n_names + 1]: the assemblies' names; row i of the matrix is named names[rows[i]], or names[i] when rows
 * is null; edges and component [n_names] as kp_dist_tree filled them.  Written without recursion.  Return value as
 * kp_format_variants has it; KP_EINVAL also for an edge or an entry of rows outside [0, n_names), an edge with a >= b, edges that
 * close a cycle or join rows of different components, and a component label that is not the smallest row of its tree.  The edge
 * table needs no formatter of its own: kp_format_distances writes kp_dist_pair records. */
KP_API int64_t kp_format_newick(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names,
                                const int32_t *rows /* [n_names] or null */, const kp_dist_pair *edges, int64_t n_edges, const int32_t *component,
                                char *out, int64_t cap);
/* The neighbour-joining tree of a handle's rows (kp_spec.h, NJ): the taxa -- the rows that hold a base in more than half of the
 * columns -- numbered, their dense matrix of p-distances filled by the same tiles, and every join run on the device.
 *   taxa  [cap_taxa] : the rows of the *n_taxa taxa, ascending; a record's node id below n_taxa is an index into it.
 *   nodes [cap_nodes]: the *n_nodes records, in the order the joins made them: n_taxa - 2, one for two taxa, none below that.
 * The counting form -- taxa and nodes null, both caps 0 -- only counts the taxa into *n_taxa (n_nodes may then be null); the
 * caller sizes its tables by it: cap_taxa >= n_taxa and cap_nodes >= max(n_taxa - 2, 1) always suffice.  KP_EINVAL for a null
 * context, handle or n_taxa, a null n_nodes outside the counting form, a handle of another device, a negative cap, a null table
 * with room asked for, caps short of the taxa or the records, and a matrix of more than KP_NJ_MAX_TAXA taxa (kp_caps.h), which this
 * call alone refuses, after the taxa are counted -- *n_taxa holds their number -- and before the matrix is allocated (the counting
 * form counts them without refusing).  min_compared as kp_dist_clusters takes it; here it moves the bar a row must clear to be a
 * taxon.  n_rows of 0 and 1 are valid.  KP_ENOMEM if the matrix, n_taxa^2 doubles, does not fit.  The call leaves the handle's
 * listing state, its cluster, tree and site tables alone.  Its O(n_rows) tables are the handle's own, allocated once, on the first
 * call; the matrix and the picks' partial results are allocated by every call and freed before it returns -- 2 GiB at the limit
 * must not stay with every handle a caller keeps open.  kp_device_allocations counts neither. */
KP_API int kp_dist_nj(kp_ctx *ctx, kp_dist *d, int32_t min_compared, int32_t *taxa /* [cap_taxa] rows of the taxa, ascending */, int64_t cap_taxa,
                      int32_t *n_taxa, kp_nj_node *nodes /* [cap_nodes] */, int64_t cap_nodes, int64_t *n_nodes);
/* The neighbour-joining table of one locus (host only): one tab-separated line -- Locus, Assemblies (n_names, the rows of the
 * matrix), Taxa (n_taxa), Newick (kp_spec.h, NJ, NEWICK) --, or no line for fewer than two taxa.  No header line.  names / name_off
 * [n_names + 1]: the assemblies' names; row i of the matrix is named names[rows[i]], or names[i] when rows is null; taxa [n_taxa]
 * and nodes [n_nodes] as kp_dist_nj filled them.  Written without recursion.  Return value as kp_format_variants has it; KP_EINVAL
 * also for taxa that do not ascend or lie outside [0, n_names), n_nodes other than the tree of n_taxa has, a node id outside the
 * nodes made before its record, a third child anywhere but in the last record, and a node that is a child twice. */
KP_API int64_t kp_format_nj(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names,
                            const int32_t *rows /* [n_names] or null */, const int32_t *taxa, int32_t n_taxa, const kp_nj_node *nodes, int64_t n_nodes,
                            char *out, int64_t cap);
/* Bootstrap support of that tree (kp_spec.h, BOOTSTRAP): `replicates` resamplings of the matrix's block columns, each one's
 * weighted matrix filled by the same tiles and joined by the same loop, a batch of them to every launch, and the splits of every
 * replicate tree counted against those of the tree the caller holds.
 *   ref_nodes [n_ref]      : the records of the supported tree, as kp_dist_nj made them for the same handle and min_compared.
 *   support [cap_support]  : support[t], t < n_ref: the replicates whose tree holds the split of the node record t made, 0 ..
 *                            replicates; -1 for a record without an inner edge: the last one, and every record of two or three taxa.
 *   trees [cap_trees]      : null, or the records of every replicate's tree, replicate r's at trees + r * n_ref.
 *   max_batch              : 0, or the most replicates joined at once; the library's own choice (kp_caps.h: the largest b with
 *                            b * n_taxa^2 * 8 <= KP_BOOT_MATRIX_BYTES) is never exceeded.  No result depends on it.
 * The same rows, min_compared, seed and replicates give the same bytes on every run.  KP_EINVAL for a null context or handle, a
 * handle of another device, replicates outside 1 .. KP_BOOT_MAX_REPLICATES (kp_caps.h), a negative max_batch or cap, a null
 * ref_nodes or support with n_ref > 0, a null trees with room asked for, n_ref other than the tree of the handle's taxa has
 * (n_taxa - 2; one for two taxa; none below), a node id of ref_nodes outside the nodes made before its record, cap_support < n_ref,
 * trees with cap_trees < replicates * n_ref, more than KP_NJ_MAX_TAXA taxa, and a matrix of KP_TREE_MAX_COLUMNS columns or more
 * (the weighted counts must fit 32 bits).  KP_ENOMEM if the tables of even one replicate -- its matrix above all -- do not fit.
 * Fewer than four taxa have no inner edge: every support is -1 and nothing is joined, unless trees asks for the replicates'
 * records.  The call leaves the handle's listing state, its cluster, tree and site tables alone; it numbers the taxa as kp_dist_nj
 * does and leaves kp_dist_nj's other tables alone.  Three O(n_rows) tables stay with the handle; the matrices, the weights and every
 * other table of a batch are allocated by the call and freed before it returns.  kp_device_allocations counts neither.
 *   kp_dist_boot_weights: weights [cap >= 16 * n_blocks]: the weight of every block column in replicate `replicate` (0 ..
 * KP_BOOT_MAX_REPLICATES - 1) of `seed`, as the device's weight planes hold them.  They depend on the column count alone. */
KP_API int kp_dist_nj_bootstrap(kp_ctx *ctx, kp_dist *d, int32_t min_compared, uint64_t seed, int32_t replicates, int32_t max_batch /* 0: the library's choice */,
                                const kp_nj_node *ref_nodes, int64_t n_ref, int32_t *support, int64_t cap_support,
                                kp_nj_node *trees /* null, or [replicates x n_ref] */, int64_t cap_trees);
KP_API int kp_dist_boot_weights(kp_ctx *ctx, kp_dist *d, uint64_t seed, int32_t replicate, uint8_t *weights, int64_t cap);
/* kp_format_nj with support values (host only): the line has a fifth column -- Locus, Assemblies, Taxa, Replicates, Newick -- and
 * the closing parenthesis of the node record t < n_taxa - 3 made is followed by support[t] as a decimal integer, a count out of
 * `replicates`: (A:0.1,B:0.2)87:0.05.  The outermost node has no label.  Otherwise byte for byte kp_format_nj's line, and its
 * refusals; KP_EINVAL also for a null support with records, replicates outside 1 .. KP_BOOT_MAX_REPLICATES, a support outside 0 ..
 * replicates at a record with an inner edge, and one other than -1 at a record without. */
KP_API int64_t kp_format_nj_support(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names,
                                    const int32_t *rows /* [n_names] or null */, const int32_t *taxa, int32_t n_taxa, const kp_nj_node *nodes, int64_t n_nodes,
                                    const int32_t *support /* [n_nodes] */, int32_t replicates, char *out, int64_t cap);
/* Transfer bootstrap of that tree (kp_spec.h, TRANSFER): kp_dist_nj_bootstrap's replicates -- the same weights, matrices, joins and
 * batches, so the same trees --, but every replicate's tree is compared with the supported tree by sets of taxa: phi_r(t) is the
 * fewest taxa that must move for replicate r's tree to hold the split of record t, at most depth - 1.
 *   support [cap_support]  : as kp_dist_nj_bootstrap's, but counted on exact sets: the replicates with phi_r(t) = 0.
 *   transfer [cap_transfer]: transfer[t], t < n_ref: the sum of phi_r(t) over the replicates; -1 for a record without an inner edge.
 *   per_replicate [cap_per]: null, or phi_r(t) at per_replicate[r * n_ref + t]; -1 likewise.
 *   trees, max_batch       : as kp_dist_nj_bootstrap's.
 * ref_nodes need not be the handle's own tree: any record list of the handle's taxa that passes the check of the node ids is
 * compared.  KP_EINVAL as kp_dist_nj_bootstrap, and for a negative cap_transfer or cap_per, a null transfer with n_ref > 0, a null
 * per_replicate with room asked for, cap_transfer < n_ref and per_replicate with cap_per < replicates * n_ref.  Fewer than four taxa:
 * every support, sum and distance is -1, and nothing is joined unless trees asks for the records.  The same rows, min_compared,
 * seed and replicates give the same bytes under any max_batch.  The call leaves the handle's listing state and its cluster, tree,
 * site and NJ tables alone.  Two more O(n_rows) tables stay with the handle; the bit-packed membership of the supported tree (n_taxa
 * * ceil((n_taxa - 3) / 32) words), O(n_taxa) tables and the distances of one batch are the call's own, and the rows of the counts
 * lie in the replicates' matrix blocks: nothing else of order n_taxa^2 is allocated beyond kp_dist_nj_bootstrap's tables. */
KP_API int kp_dist_nj_transfer(kp_ctx *ctx, kp_dist *d, int32_t min_compared, uint64_t seed, int32_t replicates, int32_t max_batch /* 0: the library's choice */,
                               const kp_nj_node *ref_nodes, int64_t n_ref, int32_t *support, int64_t cap_support, int64_t *transfer, int64_t cap_transfer,
                               int32_t *per_replicate /* null, or [replicates x n_ref] */, int64_t cap_per, kp_nj_node *trees /* null, or [replicates x n_ref] */,
                               int64_t cap_trees);
/* kp_format_nj_support's line byte for byte, the same five columns, but the label of the node record t < n_taxa - 3 made is its
 * transfer support: 1 - transfer[t] / (replicates * (depth - 1)), depth the light side of its split worked out from `nodes`, rounded
 * half up to thousandths and written with exactly three decimals, 0.000 .. 1.000: (A:0.1,B:0.2)0.934:0.05.  KP_EINVAL as
 * kp_format_nj, and for a null transfer with records, replicates outside 1 .. KP_BOOT_MAX_REPLICATES, a transfer outside 0 ..
 * replicates * (depth - 1) at a record with an inner edge, and one other than -1 at a record without.  Written without recursion. */
KP_API int64_t kp_format_nj_transfer(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names,
                                     const int32_t *rows /* [n_names] or null */, const int32_t *taxa, int32_t n_taxa, const kp_nj_node *nodes, int64_t n_nodes,
                                     const int64_t *transfer /* [n_nodes] */, int32_t replicates, char *out, int64_t cap);
/* Variable sites of a handle's rows (kp_spec.h, SITES): a reduction over the columns of the same planes, no pair looked at.
 *   kp_dist_profile    : out [cap >= 16 * n_blocks]: the profile of every column of the matrix, padding columns included, as
 *                        kp_site records with `column` filled, ascending.  Computed on the handle's first need of it and kept.
 *   kp_dist_sites_count: counts the sites for `flags` (0 or KP_SITES_CORE) into *n_sites.
 *   kp_dist_sites      : the sites of the last kp_dist_sites_count, ascending in column; KP_ESTATE without one, KP_EINVAL if cap
 *                        is short.
 *   kp_dist_site_rows  : blocks [n_rows][(n_sites + 15) / 16], row-major: the site rows of the last kp_dist_sites_count -- a matrix
 *                        kp_dist_create takes; KP_ESTATE without a count, KP_EINVAL if cap_blocks is short.
 * KP_EINVAL for a null context, handle or n_sites, a handle of another device, unknown flag bits, and a null table with room asked
 * for.  n_rows of 0 and 1 are valid and give no site (one row still has a profile).  The calls leave the handle's listing state,
 * its cluster tables and its tree tables alone, and those calls leave the profile and the last site count alone.  Their tables are
 * the handle's own, allocated once, on the first of these calls -- but for the site rows, whose buffer is replaced when a table is
 * larger than every one before it; like everything a handle does, kp_device_allocations does not count them. */
KP_API int kp_dist_profile(kp_ctx *ctx, kp_dist *d, kp_site *out, int64_t cap);
KP_API int kp_dist_sites_count(kp_ctx *ctx, kp_dist *d, int32_t flags, int64_t *n_sites);
KP_API int kp_dist_sites(kp_ctx *ctx, kp_dist *d, kp_site *out, int64_t cap);
KP_API int kp_dist_site_rows(kp_ctx *ctx, kp_dist *d, uint64_t *blocks, int64_t cap_blocks);
/* The site table of one locus (host only): one tab-separated line per site, in the sites' order: Locus, Gene, Position (1-based in
 * the gene: the coordinates of kp_format_variants' Gene position), Column (1-based in the locus's genes strung together, padding
 * not counted: 1 .. Columns of kp_format_distances), Assemblies (n_rows), A, C, G, T, N, Gap, Alleles, Major (one of acgt),
 * Informative (yes / no).  No header line.  gene_names / gene_name_off [n_genes + 1] and gene_len [n_genes]: the locus's genes in
 * database order; gene i is named gene_names[genes[i]], or gene_names[i] when genes is null.  Return value as kp_format_variants
 * has it; KP_EINVAL also for a site in a padding column or outside the matrix, counts that are negative or exceed n_rows, fewer
 * than two non-zero bases, sites that do not ascend, and an entry of genes outside [0, n_genes). */
KP_API int64_t kp_format_sites(const char *locus_name, int32_t locus_name_len, const char *gene_names, const int64_t *gene_name_off, int32_t n_genes,
                               const int32_t *genes /* [n_genes] or null */, const int32_t *gene_len, int32_t n_rows, const kp_site *sites, int64_t n_sites,
                               char *out, int64_t cap);
/* The SNP alignment of one locus (host only): one tab-separated line per row, in row order: Locus, Assembly, Sites, Alignment -- exactly
 * Sites characters of acgtn-.  No header line; no line at all when n_sites is 0.  names / name_off [n_names + 1]: the assemblies'
 * names; row i of the matrix is named names[rows[i]], or names[i] when rows is null; blocks [n_names][(n_sites + 15) / 16] as
 * kp_dist_site_rows filled them.  Return value as kp_format_variants has it; KP_EINVAL also for an entry of rows outside [0,
 * n_names), a column that is flagged both N and GAP, and a column at or beyond n_sites that is not GAP-flagged. */
KP_API int64_t kp_format_site_rows(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names,
                                   const int32_t *rows /* [n_names] or null */, int64_t n_sites, const uint64_t *blocks, char *out, int64_t cap);
/* Small parsimony of every column of a handle's rows on a neighbour-joining tree (kp_spec.h, PARSIMONY): on which branch a base
 * changes, and how many changes a column needs.  The taxa are numbered as kp_dist_nj numbers them for min_compared; ref_nodes
 * [n_ref] is a record list of those taxa -- kp_dist_nj's own, or any other tree in its form.
 *   kp_dist_nj_parsimony: runs the up- and the down-pass on the device, 64 columns to a lane, and lists the columns with a step and
 *                         the changes; *n_sites and *n_changes are their numbers.
 *   kp_dist_pars_sites  : the kp_pars_site records of the last call, ascending by column; KP_ESTATE without one, KP_EINVAL if cap
 *                         is short.
 *   kp_dist_pars_changes: its kp_pars_change records, ascending by (node, column); likewise.
 * The records are checked on the host before anything is launched for them: KP_EINVAL for a third child anywhere but in the last
 * record (and none there, for more than two taxa), a node id outside the nodes made before its record, a node that is a child twice
 * or -- but for the last -- never, and n_ref other than the tree of the handle's taxa has (n_taxa - 2; one for two taxa; none
 * below that).  KP_EINVAL also for a null context, handle or count pointer, a handle of another device, a negative n_ref, null
 * records with n_ref > 0, a null table with room asked for, and a matrix of more than KP_NJ_MAX_TAXA taxa, which this call alone
 * refuses.  Fewer than two taxa: no site, no change.  A refused call leaves the results of the call before it.  The call leaves the
 * handle's listing state, its cluster, tree and site tables and the bootstrap's alone; like kp_dist_nj it renumbers the taxa.  Only
 * the two record lists stay with the handle, each replaced when a list is longer than every one before it; the node tables -- of
 * the order of 7 * n_taxa * ceil(n_blocks / 4) words: 370 MB for 16384 taxa of 25 kb -- and the scans are allocated by every call
 * and freed before it returns: all of them or KP_ENOMEM.  kp_device_allocations counts none of it. */
KP_API int kp_dist_nj_parsimony(kp_ctx *ctx, kp_dist *d, int32_t min_compared, const kp_nj_node *ref_nodes, int64_t n_ref, int64_t *n_sites, int64_t *n_changes);
KP_API int kp_dist_pars_sites(kp_ctx *ctx, kp_dist *d, kp_pars_site *out, int64_t cap);
KP_API int kp_dist_pars_changes(kp_ctx *ctx, kp_dist *d, kp_pars_change *out, int64_t cap);
/* The homoplasy table of one locus (host only): one tab-separated line per kp_pars_site, in the records' order: Locus, Gene,
 * Position, Column (the three as kp_format_sites has them, from the same gene names and lengths), Alleles (the bases that occur),
 * Steps, Excess = Steps - (Alleles - 1).  No header line.  Return value as kp_format_variants has it; KP_EINVAL also for a site in
 * a padding column or outside the matrix, allele bits beyond the four bases, fewer than two alleles, fewer steps than Alleles - 1,
 * sites that do not ascend, and an entry of genes outside [0, n_genes). */
KP_API int64_t kp_format_nj_homoplasy(const char *locus_name, int32_t locus_name_len, const char *gene_names, const int64_t *gene_name_off, int32_t n_genes,
                                      const int32_t *genes /* [n_genes] or null */, const int32_t *gene_len, const kp_pars_site *sites, int64_t n_sites, char *out,
                                      int64_t cap);
/* The change table of one locus (host only): one tab-separated line per kp_pars_change, in the records' order: Locus, Node, Tip A,
 * Tip B, Tips, Gene, Position, Column, From, To.  A leaf: Node is the assembly's name under the quoting rule of kp_format_newick,
 * Tip A the same, Tip B `.`, Tips 1.  An inner node: Node is #t, t the 1-based number of its record; Tip A and Tip B the
 * lowest-numbered taxa below its first and its second child -- the node is their most recent common ancestor when the tree is read
 * from its last record, as kp_format_nj writes it --; Tips the taxa below it.  From and To are one of acgt, the parent's state and
 * the node's: relative to the last join, not to a root.  names, rows, taxa and nodes as kp_format_nj takes them, the genes as
 * kp_format_sites does.  No header line.  Written without recursion.  Return value as kp_format_variants has it; KP_EINVAL as
 * kp_format_nj, and for a change at the top node or outside the nodes, a parent other than the tree's, a state beyond 3, From
 * equal to To, a column in padding or outside the matrix, and changes that do not ascend by (node, column). */
KP_API int64_t kp_format_nj_changes(const char *locus_name, int32_t locus_name_len, const char *names, const int64_t *name_off, int32_t n_names,
                                    const int32_t *rows /* [n_names] or null */, const int32_t *taxa, int32_t n_taxa, const kp_nj_node *nodes, int64_t n_nodes,
                                    const char *gene_names, const int64_t *gene_name_off, int32_t n_genes, const int32_t *genes /* [n_genes] or null */,
                                    const int32_t *gene_len, const kp_pars_change *changes, int64_t n_changes, char *out, int64_t cap);

/* ---- JSON lines of a whole batch (host only) ----------------------------------------------------------------------------------
 * Replaces orjson.dumps(SerotypingResult.to_dict(), OPT_SERIALIZE_NUMPY | OPT_APPEND_NEWLINE) per genome
 * (src/kaptive/serotyping/cli.py:67-76, src/kaptive/serotyping/models.py:629-654) together with the construction of the
 * result object it serialises (GeneHits columns: src/kaptive/serotyping/core.py:303-329; locus / gene / protein sequences:
 * src/kaptive/core/seq.py:327-408): one line per assembly from the records of kp_batch_typing, the columns the host
 * finished and the contigs' text.  Strings that come from the database or the batch arrive as ready JSON literals (quotes
 * and escapes included; blobs with n + 1 offsets); contig names of the locus pieces arrive escaped but unquoted.  Returns the
 * number of bytes the lines need (written to `out` while they fit `cap`), or a negative error code. */
typedef struct kp_json_tables {  /* per database */
    const char *head;            /* {"kaptive_version":"..","database_name":"..",...,"database_taxon":N,"genome": */
    int32_t head_len;
    const char *gene_names;      /* Database.genes.ids (missing genes, ids of gene and protein sequences) */
    const int64_t *gene_name_off;
    const char *gene_ids, *cluster_names, *products;  /* GeneHits text columns: S32 / S10 / S64 truncations, per gene */
    const int64_t *gene_id_off, *cluster_name_off, *product_off;
    const char *locus_names;
    const int64_t *locus_name_off;
    const int32_t *locus_gene_off, *locus_gene_len;
    const int32_t *gene_position; /* Database.gene_positions */
    const int8_t *gene_strand;    /* Database.gene_intervals.strands */
    const uint8_t *comp_map;      /* [256] complement of a sequence byte (core/seq.py) */
    const uint8_t *char_map;      /* [256] byte -> 0..4 */
    const uint8_t *codon_map;     /* [125] codon -> amino acid, 42 = stop */
    int32_t n_loci, n_genes;      /* sizes of the tables above: every locus / gene index of the records is checked against them */
} kp_json_tables;
typedef struct kp_json_columns { /* per assembly of the batch */
    const char *asm_ids;
    const int64_t *asm_id_off;
    const char *phenotypes;
    const int64_t *phenotype_off;
    const int32_t *best_locus;
    const uint8_t *typeable;
    const int32_t *problems;
    const double *best_score, *completeness, *identity, *coverage, *length_discrepancy;
    const int32_t *piece_order;  /* [n_asm * piece_stride] numpy's argsort of the pieces' mean positions */
    const char *piece_ctg_names; /* escaped name of the contig of piece [a * piece_stride + p] */
    const int64_t *piece_ctg_name_off;
    const uint8_t *const *ctg_seqs;  /* per assembly: the contigs' text back to back ... */
    const int32_t *const *ctg_off;   /* ... and where each contig starts in it */
    const int32_t *n_ctg;            /* per assembly: how many contigs ctg_off[a] lists ... */
    const int64_t *ctg_text_len;     /* ... and how many bytes ctg_seqs[a] holds: records that point outside are KP_EINVAL */
} kp_json_columns;
KP_API int64_t kp_format_json(const kp_json_tables *tables, int32_t n_asm, const kp_asm_summary *summaries, const kp_kept *kept,
                              int32_t kept_stride, const kp_piece *pieces, int32_t piece_stride, const kp_json_columns *columns,
                              char *out, int64_t cap);
/* The per-assembly FASTA outputs (-l / -g / -p; src/kaptive/serotyping/cli.py:78-114: locus_seqs / gene_seqs /
 * translations .to_fasta() per result) from the same tables: kind 0 = locus pieces, 1 = gene sequences, 2 = translations;
 * `names` are RAW bytes -- for kind 0 the contig name of piece slot [a * piece_stride + p], for 1 and 2 the gene names by
 * gene index --; the records of all assemblies back to back, asm_end[a] = end of assembly a's.  Returns the size needed. */
KP_API int64_t kp_format_fasta(const kp_json_tables *tables, int32_t n_asm, const kp_asm_summary *summaries, const kp_kept *kept,
                               int32_t kept_stride, const kp_piece *pieces, int32_t piece_stride, const kp_json_columns *columns,
                               int32_t kind, const char *names, const int64_t *name_off, char *out, int64_t cap, int64_t *asm_end);

/* ---- protein alignment ------------------------------------------------------------------------------------------
 * Replaces PairwiseAligner.__call__ / _batched_banded_gotoh (src/kaptive/core/pairwise.py:255-325, 395-584) in its
 * unseeded mode with the defaults gap_open 11, gap_extend 1, k 20.  Sequences are raw bytes (amino-acid letters).
 *   out8 : n rows of score, matches, mismatches, gaps, q_start, q_end, t_start, t_end  */
KP_API int kp_protein_align(kp_ctx *ctx, const uint8_t *q, const int32_t *q_off, const int32_t *q_len, const uint8_t *t,
                     const int32_t *t_off, const int32_t *t_len, int32_t n, int32_t *out8);
/* The seeded mode of the same kernel (pairwise.py:449-451, PairwiseAligner.align_seeds; caller compare.LocusComparator,
 * src/kaptive/compare.py:360-366): the band is k diagonals either side of the seed diagonal of every pair,
 * |j - (i - diagonal_offsets[p])| <= k, and no longer widens with the length difference. */
KP_API int kp_protein_align_seeded(kp_ctx *ctx, const uint8_t *q, const int32_t *q_off, const int32_t *q_len,
                                   const uint8_t *t, const int32_t *t_off, const int32_t *t_len, int32_t n,
                                   const int32_t *diagonal_offsets, int32_t k, int32_t *out8);

/* ---- locus comparison seeds (host only) -------------------------------------------------------------------------------------
 * Replace the numba kernels of kaptive.core.kmers.RandstrobeIndex that compare.LocusComparator uses
 * (src/kaptive/core/kmers.py:997-1155, 779-819, 1158-1282; src/kaptive/compare.py:343-358).
 * kp_randstrobes: records {hash u64, seq_idx u32, pos1 u32, pos2 u32} (20 bytes, packed) of every sequence, in sequence
 *   and position order, or stably sorted by hash; returns how many there are (written when they fit `cap`).
 * kp_randstrobe_top_hits: per query sequence the target sequence sharing most record hashes (first maximum), that count
 *   and the diagonal offset pos1(query) - pos1(target) of the first shared record met; queries without records get 0. */
KP_API int64_t kp_randstrobes(const uint8_t *seqs, const int32_t *offsets, const int32_t *lengths, int32_t n_seqs,
                              const uint8_t *lut256, int32_t k, int32_t s, int32_t w_min, int32_t w_max,
                              int32_t sort_by_hash, void *out_records, int64_t cap);
KP_API int kp_randstrobe_top_hits(const void *query_records, int64_t n_query_records, int32_t n_queries,
                                  const void *target_records_sorted, int64_t n_target_records, int32_t n_targets,
                                  uint32_t *best_target, uint32_t *best_score, int32_t *diagonal_offset);

#ifdef __cplusplus
}
#endif
#endif /* KAPTIVE_AMD_H */
