// kp_host.h -- host-side state of the C ABI (include/kaptive_amd.h): context, batches, work sets, typing groups and runs,
// shared by the units that implement it (kp_ctx.hip, kp_db.hip, kp_batch.hip, kp_align.hip, kp_typing.hip).
#pragma once

#include <cstring>
#include <memory>
#include "kp_internal.h"
#include "kp_caps.h"
#include "kp_device.h"
#include "kp_reduce_core.h"
static_assert(KP_CAPS_ANCHOR_SUBS == KP_ANCHOR_SUBS, "the policy sizes the scan's sub-slices");

// Typing tables of one database.  Its genes are the contiguous range [gene_lo, gene_hi) of the context's genes; all
// tables use gene indices relative to gene_lo.
struct KpTypingGroup {
    int32_t gene_lo = 0, gene_hi = 0;
    DevBuf<uint16_t> d_gene_locus, d_gene_pos;
    DevBuf<uint8_t> d_gene_extra, d_prot_db;
    DevBuf<int8_t> d_gene_strand;
    DevBuf<int32_t> d_locus_off, d_locus_len, d_prot_db_off, d_prot_db_len;
    KpTypingDb typing{};
    int max_db_prot_len = 0;
};

// Reports derived from a finished reduction's kept list ("Reports derived from the kept list"): each is made on first
// request after the reduction and is the run's until the next kp_batch_reduce or until the hit table is rewritten
// (KpTypingRun::invalidate_derived); nothing of a report is allocated before somebody asks for it.
struct KpRowLayout {  // the kept rows and the piece rows of every assembly back to back: min(max(count, 0), cap) of each
    bool valid = false;
    size_t n_asm = 0;
    std::vector<int64_t> h_off;  // kept_off[n_asm + 1], then piece_off[n_asm + 1]: rows before every assembly
    DevBuf<int64_t> d_off;       // the same, uploaded once per reduction
    const int64_t *kept_off() const { return h_off.data(); }
    const int64_t *piece_off() const { return h_off.data() + n_asm + 1; }
    int64_t kept_total() const { return h_off.empty() ? 0 : h_off[n_asm]; }
    int64_t piece_total() const { return h_off.empty() ? 0 : h_off.back(); }
};
struct KpKeptSrcState {  // kp_launch_kept_locate: the variant records and the aligned rows both read it, whichever is asked for first makes it
    bool valid = false;
    DevBuf<int64_t> d_src;  // [kept rows] the row of the finished hit table behind every kept row
};
struct KpVariantsState {  // kp_variants.hip; only where the pass ran with the `variants` option
    bool valid = false;
    uint64_t cap = 0;            // records d_rec was sized for
    int64_t total = 0;           // records of all kept hits
    std::vector<int64_t> h_off;  // [kept rows + 1] first record of every kept hit
    DevBuf<int64_t> d_off;
    DevBuf<uint32_t> d_cnt;
    DevBuf<kp_variant> d_rec;
    KpPerHit<kp_variant> view() const { return {.cnt = d_cnt.p, .off = d_off.p, .data = d_rec.p, .cap = (int64_t)cap}; }
};
struct KpAlignedState {  // kp_aligned.hip; only where the pass ran with the `aligned` option
    bool valid = false;
    int64_t n_blocks = 0;                // blocks of all rows: what d_blocks holds, exactly
    std::vector<kp_aligned_row> h_rows;  // one per kept row, back to back
    DevBuf<uint32_t> d_cnt;
    DevBuf<int64_t> d_off;               // [kept rows + 1] first block of every row
    DevBuf<uint64_t> d_blocks;
    DevBuf<kp_aligned_row> d_rows;
};
struct KpBreakpointsState {  // kp_breakpoints.hip
    bool valid = false;
    std::vector<int64_t> h_off;          // [n_asm + 1] breakpoint records before every assembly
    DevBuf<int64_t> d_off;
    DevBuf<uint32_t> d_cnt;              // [n_asm]
    DevBuf<kp_breakpoint> d_tmp, d_rec;  // one record per kept row each: per assembly from its first row, then back to back
};
struct KpAllelesState {  // kp_alleles.hip
    bool valid = false;
    std::vector<kp_allele> h_rec;   // one per kept row, back to back
    std::vector<uint64_t> h_piece;  // one per piece row, back to back
    DevBuf<kp_allele> d_rec;
    DevBuf<uint64_t> d_piece;
};
struct KpRescueState {  // kp_rescue.hip; only where the context has the `rescue` option
    bool valid = false;
    int32_t flank = 0;           // the rescue_flank the records were made with (another one makes them again)
    std::vector<int64_t> h_off;  // rec_off[n_asm + 1], then unit_off[n_asm + 1]: records / (subject, piece) units before every assembly
    std::vector<kp_rescue> h_rec;
    DevBuf<int64_t> d_off;
    DevBuf<KpRescueUnit> d_units;
    DevBuf<int32_t> d_cell, d_sub, d_ctl, d_scratch;
    DevBuf<kp_rescue> d_rec;
};
struct KpDerived { KpRowLayout layout; KpKeptSrcState src; KpVariantsState var; KpAlignedState aln; KpBreakpointsState bp; KpAllelesState al; KpRescueState rs; };

// Reduction state of one (batch, typing group): the group's hits (copied out of the batch's hit table with gene indices
// rebased) and everything score / reduce / typing produce for it.
struct KpTypingRun {
    // every group works on streams of its own (highest priority), so the reductions of several databases over one
    // batch overlap: they are chains of short, low-occupancy kernels.  The streams belong to the context (one pair per
    // group, shared by the work sets: a context's streams should not outnumber the runtime's hardware queues): borrowed
    // from kp_ctx::group_streams, plain handles that the run does not destroy.  The two events are the run's own.
    hipStream_t stream = nullptr, aux = nullptr;
    Event ev_fork, ev_join;
    bool split = false;  // `hits` belongs to the work set's most recent alignment pass
    KpHitTable hits{};   // the group's hit rows: d_hits / d_hit_n, or the work set's table itself when the group spans every gene of the context (no copy)
    DevBuf<kp_hit> d_hits;
    DevBuf<uint32_t> d_hit_n;
    DevBuf<uint64_t> d_keys;   // cull keys
    DevBuf<uint32_t> d_order;
    DevBuf<uint8_t> d_flag;
    DevBuf<int32_t> d_dp_scratch;
    int kept_cap = 0, piece_cap = 0, prot_cap = 0;
    size_t n_asm = 0;  // assemblies of the most recent reduction: with kept_cap, the layout of d_pairs
    DevBuf<uint32_t> d_pack;  // kept / piece rows cut to the strides the caller asked for (kp_batch_typing)
    DevBuf<uint8_t> d_prot;
    DevBuf<double> d_scores;
    DevBuf<int32_t> d_lcounts, d_best, d_pairs, d_dp;
    DevBuf<KpKept> d_kept;
    DevBuf<KpPiece> d_pieces;
    DevBuf<KpAsmSummary> d_summary;
    KpTypingParams prm{};
    bool scored = false, reduced = false;
    bool sums_valid = false;  // h_sums / max_kept / max_pieces belong to the most recent reduction
    std::vector<KpAsmSummary> h_sums;
    int32_t max_kept = 1, max_pieces = 1;
    KpDerived derived;  // the reports made from the kept list, on request (above)
    void invalidate_derived() {  // the kept list they describe is about to be replaced: flags only, every buffer stays (a settled context allocates nothing)
        derived.layout.valid = derived.src.valid = derived.var.valid = derived.aln.valid = derived.bp.valid = derived.al.valid = derived.rs.valid = false;
    }
    // the only places the views of the kept and the piece rows are built (valid once derived.layout is)
    KpKeptRows kept_rows(int32_t gene_lo) const {
        return {.kept = d_kept.p, .kept_cap = kept_cap, .kept_off = derived.layout.d_off.p, .total = derived.layout.kept_total(), .gene_lo = gene_lo};
    }
    KpPieceRows piece_rows() const {
        return {.pieces = d_pieces.p, .piece_cap = piece_cap, .piece_off = derived.layout.d_off.p + derived.layout.n_asm + 1, .total = derived.layout.piece_total()};
    }
    // d_pairs: the pairs of the protein DP, one slot per kept row: q_off, q_len, t_off, t_len [slots each], then pair_base [n_asm], n_pairs [1]
    size_t slots() const { return n_asm * (size_t)kept_cap; }
    size_t pairs_len() const { return 4 * slots() + n_asm + 1; }
    KpReduceTables tables() const {
        int32_t *const q = d_pairs.p, *const base = q + 4 * slots();
        return {.best = d_best.p, .keys = d_keys.p, .order = d_order.p, .kept_flag = d_flag.p, .kept = d_kept.p, .kept_cap = kept_cap,
                .pieces = d_pieces.p, .piece_cap = piece_cap, .summary = d_summary.p, .prot = d_prot.p, .prot_cap = prot_cap,
                .q_off = q, .q_len = q + slots(), .t_off = q + 2 * slots(), .t_len = q + 3 * slots(), .pair_base = base, .n_pairs = base + n_asm, .dp8 = d_dp.p};
    }
};

struct kp_batch;

// Options of a context: defaults come from the environment once, at kp_ctx_create; kp_ctx_set_option changes them.
struct KpOptions : KpCapOptions {
    int scan_mode = 0;           // KAPTIVE_AMD_SCAN_ABLATE (tools/scan_ablate.py)
    int library_sort = 0;        // anchors through kp_anchor_compact + rocPRIM's segmented radix sort instead of kp_bsort.hip
    uint32_t upload_piece_mb = 4096;  // H2D copies of a batch's words are enqueued in pieces of this size (batch_make)
    int readback_copy_engine = 0;   // results read back with hipMemcpyAsync instead of the read-back kernel (see Fetch)
    int spin_wait = 0;              // host waits spin on the stream (the runtime's default) instead of blocking on an interrupt
    int cigar = 0;                  // CIGARs of the finished hits (kp_cigar.hip): off unless asked for; applies from the next kp_batch_align
    int variants = 0;               // variant records of the kept hits (kp_variants.hip); a pass with it computes the CIGARs too: the records are read off them
    int aligned = 0;                // aligned rows of the kept hits (kp_aligned.hip); a pass with it computes the CIGARs too: the rows are read off them
    int cs = 0;                     // cs difference strings of the finished hits (kp_cs.hip); a pass with it computes the CIGARs too: cs reads them
    int rescue = 0;                 // rescue records of the missing genes (kp_rescue.hip); read when the records are asked for: no pass does anything for them
    int rescue_flank = KP_RESCUE_FLANK;  // bases either side of a locus piece the translated search looks at (0 .. KP_RESCUE_FLANK_MAX)
    bool trace_summary = true;      // KAPTIVE_AMD_TRACE_SUMMARY=0: the band walks ignore the fills' piece summaries and fetch every piece on a path (kp_walk.h; A/B switch)
    bool join_stats = false;        // KAPTIVE_AMD_JOIN_STATS: kp_batch_wait reports the pass's group / join / mid_occ counts on stderr
    KpJoinLaunch join;              // KAPTIVE_AMD_JOIN_GRID / _JOIN_PRIO / _SKIP_JOINS: launch shape of the join kernels (kp_internal.h)
};

// Device copy of one batch's input (packed words + tables).  Recycled through the context (hipFree synchronises the
// device, so a stream of batches must not free anything).
struct KpInput {
    DevBuf<uint32_t> d_words;
    DevBuf<int64_t> d_asm_word_off;
    DevBuf<int32_t> d_ctg_start, d_ctg_len, d_asm_first_ctg, d_n_runs, d_asm_first_nrun;
    PinnedBlock h_stage;  // pinned staging of the tables (the caller's copies may be freed on return)
    Event ready;          // recorded on the copy stream after the last H2D copy of the batch
};

// Slots of KpWork::ev, each recorded after the stage named; kp_batch_profile returns the seven times between consecutive ones.
// JOINED: after the join back, i.e. what is left of the join kernels once the band tasks are through (its "sw64" value); END: end
// of the pass, recorded right behind it so that the layout stays (the last value reads 0).
enum KpPassEvent { KP_EV_START, KP_EV_SCAN, KP_EV_SORT, KP_EV_ORDER, KP_EV_FILL, KP_EV_TRACEBACK, KP_EV_JOINED, KP_EV_END, KP_N_EVENTS };
static_assert(KP_EV_END == 7, "kp_batch_profile returns seven stage times");
enum KpStat { KP_STAT_ANCHORS, KP_STAT_TASKS, KP_STAT_CELLS, KP_STAT_HITS, KP_STAT_RERUNS, KP_N_STATS };  // KpWork::stats, kp_batch_stats
enum KpTopWord { KP_TOP_TRACE = 0, KP_TOP_OCC = 3, KP_TOP_WORDS = 4 };  // d_trace_top: [0] trace units handed out, [1..2] the fill kernel's quad counters (four 32-bit words), [3] the occurrence cut's demand
enum KpJoinCount { KP_JOIN_GROUPS = 0, KP_JOIN_CLASSES = 1, KP_JOIN_COUNTS = 1 + KP_N_CLASSES };  // d_join_counts: [0] groups, [1 + c] joins of band class c
enum KpCandCount { KP_CAND_FRONT, KP_CAND_BACK, KP_CAND_COUNTS };  // d_cand_count: the streaming kernel's candidates (front of the list), the edge kernel's (back)

// Work set: every device buffer an alignment pass and the reductions after it write, and the results they leave.  A
// context owns KP_WORK_SLOTS of them and hands them to batches round-robin at kp_batch_align, so a stream of batches
// allocates nothing after the first few and keeps what it learnt about buffer sizes (the caps live in the context).
// Its base is what the buffers of the most recent pass were sized for.  The packed blocks (several tables behind one
// allocation, one memset and one read-back) are laid out here and nowhere else: each has its length, an accessor per
// region and, where the host keeps a mirror, the same for the mirror.
struct KpWork : KpPassCaps {
    kp_batch *owner = nullptr;
    size_t n_asm = 0;  // assemblies of `owner` (kp_batch_align): the blocks below are laid out by it
    KpKeyBits key_bits{16, 30};  // compact anchor keys of the most recent alignment pass
    DevBuf<uint64_t> d_anchors_a, d_anchors_b;
    DevBuf<uint32_t> d_counts;  // [n_asm] anchor counts, [KP_N_CLASSES] task counts, [n_asm] largest sub-slice demand; h_counts mirrors it
    size_t task_count_at() const { return n_asm; }
    size_t slice_need_at() const { return n_asm + KP_N_CLASSES; }
    size_t counts_len() const { return slice_need_at() + n_asm; }
    const uint32_t *h_anchor_count() const { return h_counts.data(); }
    const uint32_t *h_task_count() const { return h_counts.data() + task_count_at(); }
    const uint32_t *h_slice_need() const { return h_counts.data() + slice_need_at(); }
    DevBuf<uint32_t> d_sub_counts;  // [n_asm * KP_ANCHOR_SUBS]
    DevBuf<uint64_t> d_cand;        // candidates of the scan (kp_cand_pack); d_cand_count[0] = how many
    DevBuf<unsigned long long> d_cand_count;
    DevBuf<uint32_t> d_seg;     // the library sort's segments: [n_asm] begin, [n_asm] end
    size_t seg_len() const { return 2 * n_asm; }
    uint32_t *seg_begin() const { return d_seg.p; }
    uint32_t *seg_end() const { return d_seg.p + n_asm; }
    DevBuf<KpTask> d_tasks;
    DevBuf<KpSwResult> d_results;
    // d_task_drop, per task slot: a chain consumed the cluster, its band task reports no hit (kp_join.hip)
    DevBuf<uint8_t> d_task_drop, d_jscratch;
    // counting tables of the occurrence cut's quantile (kp_chain.hip: block_mid_occ): occ_slots tables of 2^occ_log2 entries
    DevBuf<uint32_t> d_occ_keys, d_occ_cnts, d_occ_state;
    uint32_t occ_log2 = 0;
    DevBuf<KpSwEnd> d_ends;
    DevBuf<unsigned long long> d_trace_top;  // [KP_TOP_WORDS]
    unsigned long long *occ_demand() const { return d_trace_top.p + KP_TOP_OCC; }
    // A work set's alignment pass runs on the set's own stream with its own trace buffer and sort scratch: the passes of
    // consecutive batches overlap on the device (the seed scan and the sort of one wait on the L2 and on HBM while the
    // fill kernel of the other keeps the vector ALUs busy)
    Stream astream;
    // ... and the joined fill of its joins on a second one, beside the band tasks' fill (kp_join.hip: a few waves, each a long
    // chain of dependent steps: 3 ms that the pass would otherwise wait for)
    Stream jstream;
    Event ev_jfork, ev_jdone;
    DevBuf<uint4> d_trace;  // direction bits of the banded Smith-Waterman: written by the fill kernel, read by the traceback
    DevBlock sort_temp;  // the library sort's scratch
    DevBuf<uint32_t> d_task_order;  // [KP_ORDER_HEAD] histogram + cursors (KP_ORDER_COUNTS inside), then [KP_N_CLASSES * task_cap] permutation
    size_t order_len() const { return KP_ORDER_HEAD + KP_N_CLASSES * (size_t)task_cap; }
    // kp-align v4 (kp_join.hip): groups of provisional clusters, joins per band class, their counts
    DevBuf<KpGroup> d_groups;
    DevBuf<KpJoin> d_joins;
    DevBuf<uint32_t> d_join_counts;
    uint32_t h_join_counts[KP_JOIN_COUNTS] = {};
    uint32_t h_group_count() const { return h_join_counts[KP_JOIN_GROUPS]; }
    const uint32_t *h_join_count() const { return h_join_counts + KP_JOIN_CLASSES; }
    std::vector<KpJoin> h_joins;  // fetched on first use (kp_batch_joins: stage tests only)
    // device-side hit tables (per-assembly regions of hit_cap rows)
    DevBuf<kp_hit> d_hits_raw, d_hits;
    DevBuf<uint32_t> d_hit_counts;  // [n_asm] raw, then [n_asm] final; h_hit_counts mirrors it
    size_t hit_counts_len() const { return 2 * n_asm; }
    uint32_t *h_raw_hit_count() { return h_hit_counts.data(); }
    uint32_t *h_hit_count() { return h_hit_counts.data() + n_asm; }
    DevBuf<uint64_t> d_keys;        // 3 per hit row
    DevBuf<unsigned long long> d_cells;
    // CIGARs of the finished hits (kp_cigar.hip), only where the pass was enqueued with the `cigar` option: nothing below is
    // allocated otherwise.  They are results like the hit tables: theirs until the work set's next pass or kp_batch_set_hits.
    bool cigar_on = false, cigar_valid = false;
    uint64_t cigar_cap = 0;          // ops d_cig_ops was sized for
    int64_t cigar_total = 0;         // ops of all hits
    DevBuf<unsigned long long> d_cig_src;  // per row of the hit tables: the source of the hit (kp_cigar.hip: src_key)
    DevBuf<uint32_t> d_cig_cnt, d_cig_ops;
    DevBuf<int64_t> d_cig_off, d_cig_hit_off;  // [total_hits + 1] first op of every hit; [n_asm + 1] the host's hit_off
    // cs strings of the finished hits (kp_cs.hip), only where the pass was enqueued with the `cs` option; results with the CIGARs' lifetime
    bool cs_on = false, cs_valid = false;
    uint64_t cs_cap = 0;             // bytes d_cs_bytes was sized for
    int64_t cs_total = 0;            // bytes of all hits
    DevBuf<uint32_t> d_cs_cnt;
    DevBuf<int64_t> d_cs_off;        // [total_hits + 1] first byte of every hit
    DevBuf<char> d_cs_bytes;
    bool var_on = false;             // the pass was enqueued with the `variants` option (kp_variants.hip; the records live in the typing runs)
    bool aln_on = false;             // the pass was enqueued with the `aligned` option (kp_aligned.hip; the rows live in the typing runs)
    // reduction: one run per typing group, created on first use
    std::vector<std::unique_ptr<KpTypingRun>> runs;
    // results
    bool aligned = false, finalised = false;
    std::vector<uint32_t> h_counts, h_hit_counts;
    std::vector<KpTask> h_tasks[KP_N_CLASSES];
    std::vector<int64_t> hit_off;
    int64_t stats[KP_N_STATS] = {};
    Event ev[KP_N_EVENTS];  // stage boundaries of the most recent alignment pass
    // the views the launchers take (kp_internal.h), built here and nowhere else
    KpAnchors anchors() const {
        return {.keys = d_anchors_a.p, .count = d_counts.p, .cap = anchor_cap, .kb = key_bits, .sub_count = d_sub_counts.p,
                .sub_cap = anchor_cap / KP_ANCHOR_SUBS, .second = d_anchors_b.p, .need = d_counts.p + slice_need_at()};
    }
    KpTasks tasks() const {
        return {.tasks = d_tasks.p, .count = d_counts.p + task_count_at(), .cap = task_cap, .results = d_results.p, .ends = d_ends.p, .drop = d_task_drop.p,
                .order_head = d_task_order.p, .order_count = d_task_order.p + KP_ORDER_COUNTS, .order = d_task_order.p + KP_ORDER_HEAD};
    }
    KpGroups groups() const { return {.list = d_groups.p, .count = d_join_counts.p + KP_JOIN_GROUPS, .cap = group_cap}; }
    KpJoins joins() const { return {.list = d_joins.p, .count = d_join_counts.p + KP_JOIN_CLASSES, .cap = join_cap}; }
    KpTrace trace() const { return {.units = d_trace.p, .top = d_trace_top.p + KP_TOP_TRACE, .cap = trace_cap}; }
    KpHitTable raw_hits() const { return {.rows = d_hits_raw.p, .count = d_hit_counts.p, .cap = hit_cap, .keys = d_keys.p}; }
    KpHitTable hits() const { return {.rows = d_hits.p, .count = d_hit_counts.p + n_asm, .cap = hit_cap, .keys = nullptr}; }
    KpHitRows hit_rows() const { return {.hit_off = d_cig_hit_off.p, .total = hit_off[n_asm]}; }
    KpPerHit<uint32_t> cigars() const { return {.cnt = d_cig_cnt.p, .off = d_cig_off.p, .data = d_cig_ops.p, .cap = (int64_t)cigar_cap}; }
    KpPerHit<char> cs() const { return {.cnt = d_cs_cnt.p, .off = d_cs_off.p, .data = d_cs_bytes.p, .cap = (int64_t)cs_cap}; }
    void reset_runs() { for (auto &r : runs) if (r) { r->split = r->scored = r->reduced = r->sums_valid = false; r->invalidate_derived(); } }  // their hit table is about to be rewritten
};

#define KP_INPUT_POOL 16  /* recycled device copies of batch inputs: uploads run several shards ahead of the passes that read them */

// Members are destroyed last to first; kp_ctx_destroy has made the device current and waited for it before that begins.
struct kp_ctx {
    int device = 0;
    PinnedBlock bounce;            // page-locked landing area of result read-backs (Fetch)
    int gs_bits = 18;              // bits of the gene/strand field of an anchor key this database can set
    int max_gene_len = 0;
    Stream stream;  // database uploads, stand-alone protein alignments (alignment passes: KpWork::astream)
    Stream post;    // everything after a batch's alignment pass (waits on that batch's event)
    Stream aux;     // forked off `post` for kernels that only fill a few CUs (wide-band proteins)
    Stream copy;    // H2D copies of batch inputs (overlap with the passes of earlier batches)
    std::string error;
    KpOptions opt;
    KpLearnt learnt;
    KpCsCaps cs_caps;  // byte buffer of the cs strings: option and learnt size (kp_caps.h)
    KpVarCaps var_caps;  // record buffer of the variant records, likewise
    // resident database
    bool has_db = false;
    int32_t n_genes = 0;
    int64_t n_postings = 0;
    std::vector<int32_t> gene_len;  // host copy (finalisation flips reverse-strand coordinates)
    DevBuf<uint2> d_slots;
    DevBuf<uint64_t> d_filter, d_filter2;
    DevBuf<uint64_t> d_postings;
    DevBuf<uint32_t> d_nib;
    DevBuf<int32_t> d_nib_off, d_gene_len;
    DevBuf<uint4> d_gene_prof;   // row profiles of the genes for the fill kernel (KpGenes::prof)
    DevBuf<uint8_t> d_gene_has_n;
    KpSeedIndex index{};
    KpGenes genes{};
    // protein stage
    DevBuf<int8_t> d_blosum;
    DevBuf<float> d_ln;  // logarithm tables of the mapping quality (kp_mapq.h): ln(i / 2), then ln(i), from kp_mapq_ln
    const float *ln_half() const { return d_ln.p; }
    const float *ln_int() const { return d_ln.p + KP_MAPQ_LN_HALF_SIZE; }
    DevBuf<uint8_t> d_pq, d_pt;
    DevBuf<int32_t> d_pmeta, d_pout, d_pscratch;
    // typing tables (kp_db_load_typing / kp_db_load_typing_group): one set per database whose genes are in the index
    std::vector<std::unique_ptr<KpTypingGroup>> groups;
    std::vector<KpRunCaps> run_caps;  // per typing group
    struct GroupStreams { Stream stream, aux; };
    std::vector<GroupStreams> group_streams;  // reduction streams, per typing group
    // work sets and recycled inputs
    KpWork work[KP_WORK_SLOTS];
    uint32_t next_slot = 0;
    std::vector<std::unique_ptr<KpInput>> free_inputs;
    std::vector<kp_batch *> batches;  // live batches (a context destroyed first detaches them)
};

struct kp_batch {
    kp_ctx *ctx = nullptr;
    int32_t n_asm = 0;
    // device copy of the input: returned to the context's pool by kp_batch_destroy; freed by kp_ctx_destroy where the
    // batch outlives its context, so that deleting such a batch touches no device
    std::unique_ptr<KpInput> in;
    const uint32_t *d_words = nullptr;  // in->d_words.p, or the caller's device pointer (kp_batch_create_device)
    KpBatchView view{};
    int64_t max_asm_bases = 0;  // longest assembly of the batch (padded)
    int32_t n_ctg_total = 0;    // contigs of all its assemblies (one thread each in the edge kernel)
    KpWork *w = nullptr;        // the work set holding this batch's alignment results, while it still does
    KpWork *last_w = nullptr;   // the work set of its most recent pass (for completion waits; may have a new owner)
    kp_batch *after = nullptr;  // its words are another batch's device copy: passes wait for that batch's upload
    int32_t group = 0;          // the typing group score / reduce / typing calls address
};

// Streams of the short, low-occupancy kernels that follow an alignment pass get the highest priority the device offers:
// when another batch's alignment pass fills the chip, their waves are scheduled as soon as any slot frees up.  (kp_ctx.hip)
hipError_t create_priority_stream(hipStream_t *stream);

// Results come back to the host through the shader, not through a copy engine: kernels of the stream write them into a
// page-locked landing area, the host waits for the stream and copies them out.  A read-back handed to the copy engines
// (hipMemcpyAsync) queued up behind the shard that was being uploaded -- 1.25 GB, 22 ms -- so that every kp_batch_score
// of a host-fed stream returned only when the upload in flight had landed (tools/experiments/h2d_interference.py: 20 ms
// per batch alone, 140 ms beside a continuous upload; profiles/r4_h2d_timeline.md).  KAPTIVE_AMD_READBACK=copy restores
// the copy-engine path for comparison.
struct Fetch {
    kp_ctx *ctx;
    hipStream_t stream;
    struct Item { void *dst; size_t off, bytes; };
    std::vector<Item> items;
    size_t used = 0;
    bool by_copy_engine;
    Fetch(kp_ctx *c, hipStream_t s) : ctx(c), stream(s), by_copy_engine(c->opt.readback_copy_engine != 0) {}
    // A Fetch that is dropped half-way (an error between add() and finish()) leaves kernels writing into the landing
    // area: wait for them, so that the next begin() never frees or reuses memory that is still being written.
    ~Fetch() { if (!items.empty()) (void)hipStreamSynchronize(stream); }
    // total bytes of everything that will be added before finish()
    int begin(size_t total) {
        if (by_copy_engine) return KP_OK;
        total += 64 * 8;
        // (calls on a context are serialised and every Fetch waits for its stream before it goes away, so nothing
        // is in flight towards the old area where this one grows)
        KP_HIP_CHECK(ctx, ctx->bounce.reserve(total, total + total / 4 + (1u << 20)));
        return KP_OK;
    }
    int add(void *dst, const void *src, size_t bytes) {
        if (!bytes) return KP_OK;
        if (by_copy_engine || (bytes & 3u)) { KP_HIP_CHECK(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream)); return KP_OK; }
        if (used + bytes > ctx->bounce.bytes) return kp_fail(ctx, KP_ESTATE, "read-back larger than announced");
        kp_launch_read_back(src, ctx->bounce.p + used, bytes, stream);
        items.push_back(Item{dst, used, bytes});
        used = (used + bytes + 63) & ~(size_t)63;
        return KP_OK;
    }
    int finish() {
        const hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { items.clear(); used = 0; }
        KP_HIP_CHECK(ctx, e);
        for (const Item &it : items) std::memcpy(it.dst, ctx->bounce.p + it.off, it.bytes);
        items.clear(); used = 0;
        return KP_OK;
    }
};

// one read-back of several pieces: begin, add each, finish
struct FetchItem { void *dst; const void *src; size_t bytes; };
inline int fetch_all(kp_ctx *ctx, hipStream_t stream, std::initializer_list<FetchItem> items) {
    size_t total = 0;
    for (const FetchItem &i : items) total += i.bytes;
    Fetch f(ctx, stream);
    int rc = f.begin(total);
    for (const FetchItem &i : items) if (!rc) rc = f.add(i.dst, i.src, i.bytes);
    return rc ? rc : f.finish();
}

template <class T>
int upload(kp_ctx *ctx, DevBuf<T> &buf, const T *src, size_t n, hipStream_t stream = nullptr) {
    KP_HIP_CHECK(ctx, buf.reserve(n));
    if (n) KP_HIP_CHECK(ctx, hipMemcpyAsync(buf.p, src, n * sizeof(T), hipMemcpyHostToDevice, stream ? stream : ctx->stream.h));
    return KP_OK;
}

inline KpWork *work_of(kp_batch *b) {  // null: never aligned, or its results have been displaced
    return (b->w && b->w->owner == b) ? b->w : nullptr;
}
// the batch's work set with finalised hit tables, or null after recording the error (kp_align.hip)
KpWork *finalised_work(kp_ctx *ctx, kp_batch *b);
