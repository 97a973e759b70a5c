// kp_align.hip -- the alignment pass of a batch on its work set's streams, the wait that grows what overflowed and runs the
// pass again (sizes: kp_caps.h), finalisation of the hit table and the accessors of every stage's results.
#include "kp_host.h"

#include <algorithm>

static const char *const NO_RESULTS = "this batch has no resident alignment results (not aligned yet, or displaced: a context keeps the results of its KP_WORK_SLOTS most recently aligned batches)";

// What a pass enqueues between its fork onto the join stream and the join back: chaining of the groups, joined fill and walk-back on `jstream`; the band
// tasks' order, fill and traceback on `stream`.  The caller joins the streams whatever this returns: the next pass never starts beside kernels of this one.
static int enqueue_forked(kp_ctx *ctx, kp_batch *b, KpWork *w, hipStream_t stream) {
    const KpAnchors an = w->anchors();
    const KpTasks tasks = w->tasks();
    const KpJoins joins = w->joins();
    const KpTrace trace = w->trace();
    kp_launch_join_chain(an, tasks, w->groups(), joins, w->d_jscratch.p, ctx->opt.join, w->jstream);
    kp_launch_join_fill(b->view, ctx->genes, joins, trace, ctx->opt.join, w->jstream);
    kp_launch_join_trace(b->view, ctx->genes, joins, tasks, trace, ctx->opt.join, w->jstream);
    kp_launch_task_order(b->view, ctx->genes, an, tasks, stream);
    KP_HIP_CHECK(ctx, hipEventRecord(w->ev[KP_EV_ORDER], stream));
    // all four band classes in one fill launch, then the traceback (kp_sw.hip)
    kp_launch_sw(b->view, ctx->genes, tasks, trace, ctx->max_gene_len > KP_FILL16_MAX_GENE_LEN, ctx->opt.trace_summary, stream, w->ev[KP_EV_FILL]);
    KP_HIP_CHECK(ctx, hipEventRecord(w->ev[KP_EV_TRACEBACK], stream));
    return KP_OK;
}

static int enqueue_align(kp_ctx *ctx, kp_batch *b, KpWork *w) {
    const size_t n_asm = w->n_asm;
    for (auto &e : w->ev)
        if (!e) KP_HIP_CHECK(ctx, hipEventCreate(&e.h));
    if (!w->astream) KP_HIP_CHECK(ctx, hipStreamCreateWithFlags(&w->astream.h, hipStreamNonBlocking));
    if (!w->jstream) {
        KP_HIP_CHECK(ctx, hipStreamCreateWithFlags(&w->jstream.h, hipStreamNonBlocking));
        KP_HIP_CHECK(ctx, hipEventCreateWithFlags(&w->ev_jfork.h, hipEventDisableTiming));
        KP_HIP_CHECK(ctx, hipEventCreateWithFlags(&w->ev_jdone.h, hipEventDisableTiming));
    }
    hipStream_t stream = w->astream;
    const Event *ev = w->ev;
    if ((uint64_t)n_asm * w->anchor_cap > 0xFFFFFFF0ull)
        return kp_fail(ctx, KP_EOVERFLOW, "anchor buffer would exceed 2^32 entries; use smaller batches");
    if (((uint64_t)b->view.total_words << 4) >> KP_CAND_POS_BITS)
        return kp_fail(ctx, KP_EOVERFLOW, "a batch holds at most 2^33 bases (candidate positions); use smaller batches");
    KP_HIP_CHECK(ctx, w->d_anchors_a.reserve(n_asm * w->anchor_cap));
    KP_HIP_CHECK(ctx, w->d_anchors_b.reserve(n_asm * w->anchor_cap));
    KP_HIP_CHECK(ctx, w->d_counts.reserve(w->counts_len()));
    KP_HIP_CHECK(ctx, w->d_sub_counts.reserve(n_asm * KP_ANCHOR_SUBS));
    KP_HIP_CHECK(ctx, w->d_seg.reserve(w->seg_len()));
    KP_HIP_CHECK(ctx, w->d_tasks.reserve(KP_N_CLASSES * (size_t)w->task_cap));
    KP_HIP_CHECK(ctx, w->d_results.reserve(KP_N_CLASSES * (size_t)w->task_cap));
    KP_HIP_CHECK(ctx, w->d_task_drop.reserve(KP_N_CLASSES * (size_t)w->task_cap));
    KP_HIP_CHECK(ctx, w->d_jscratch.reserve(kp_join_chain_scratch_bytes(ctx->opt.join)));
    {   // a table holds every distinct minimizer of the longest assembly (2 / 11 of its bases) at a load of at most a half
        uint32_t lg = 12;
        while (((uint64_t)1 << lg) < (uint64_t)b->max_asm_bases * 2 / 5 + 1 && lg < 31) ++lg;
        w->occ_log2 = lg;
        KP_HIP_CHECK(ctx, w->d_occ_keys.reserve((size_t)w->occ_slots << lg));
        KP_HIP_CHECK(ctx, w->d_occ_cnts.reserve((size_t)w->occ_slots << lg));
        KP_HIP_CHECK(ctx, w->d_occ_state.reserve(kp_occ_state_words(n_asm, w->occ_slots)));
    }
    KP_HIP_CHECK(ctx, w->d_task_order.reserve(w->order_len()));
    KP_HIP_CHECK(ctx, w->d_cand.reserve(w->cand_cap));
    KP_HIP_CHECK(ctx, w->d_cand_count.reserve(KP_CAND_COUNTS));  // the streaming kernel's candidates (front), the edge kernel's (back)
    KP_HIP_CHECK(ctx, w->d_ends.reserve(KP_N_CLASSES * (size_t)w->task_cap));
    KP_HIP_CHECK(ctx, w->d_trace_top.reserve(KP_TOP_WORDS));
    KP_HIP_CHECK(ctx, w->d_trace.reserve(w->trace_cap));
    KP_HIP_CHECK(ctx, w->d_groups.reserve(w->group_cap));
    KP_HIP_CHECK(ctx, w->d_joins.reserve(KP_N_CLASSES * (size_t)w->join_cap));
    KP_HIP_CHECK(ctx, w->d_join_counts.reserve(KP_JOIN_COUNTS));
    KP_HIP_CHECK(ctx, hipStreamWaitEvent(stream, b->in->ready, 0));  // the batch's H2D copies
    if (b->after && b->after->in) KP_HIP_CHECK(ctx, hipStreamWaitEvent(stream, b->after->in->ready, 0));
    KP_HIP_CHECK(ctx, hipMemsetAsync(w->d_counts.p, 0, w->counts_len() * sizeof(uint32_t), stream));
    KP_HIP_CHECK(ctx, hipMemsetAsync(w->d_sub_counts.p, 0, n_asm * KP_ANCHOR_SUBS * sizeof(uint32_t), stream));
    KP_HIP_CHECK(ctx, hipMemsetAsync(w->d_cand_count.p, 0, KP_CAND_COUNTS * sizeof(unsigned long long), stream));
    KP_HIP_CHECK(ctx, hipMemsetAsync(w->d_task_order.p, 0, KP_ORDER_HEAD * sizeof(uint32_t), stream));
    KP_HIP_CHECK(ctx, hipMemsetAsync(w->d_trace_top.p, 0, KP_TOP_WORDS * sizeof(unsigned long long), stream));
    KP_HIP_CHECK(ctx, hipMemsetAsync(w->d_join_counts.p, 0, KP_JOIN_COUNTS * sizeof(uint32_t), stream));
    // compact anchor keys: as many bits per field as this batch and database can set
    auto bits_for = [](uint64_t max_value) { uint32_t n = 1; while (n < 63 && (max_value >> n)) ++n; return n; };
    w->key_bits.qb = std::min<uint32_t>(16, bits_for((uint64_t)std::max(ctx->max_gene_len, 1)));
    w->key_bits.db = std::min<uint32_t>(30, bits_for((uint64_t)b->max_asm_bases + KP_DIAG_BIAS));
    const KpAnchors an = w->anchors();
    KP_HIP_CHECK(ctx, hipEventRecord(ev[KP_EV_START], stream));
    kp_launch_scan(b->view, ctx->index, w->d_cand.p, w->d_cand_count.p, w->cand_cap, an, ctx->opt.scan_mode, b->n_ctg_total, stream, ev[KP_EV_SCAN]);
    if (!ctx->opt.library_sort && kp_bsort_fits(2u * (uint32_t)ctx->n_genes)) {
        // buckets of the gene/strand field, each sorted on its own (kp_bsort.hip); sorted keys end up where the chaining reads them
        kp_launch_anchor_bsort(b->view, an, 2u * (uint32_t)ctx->n_genes, stream);
    } else {  // `library_sort`: compaction + the library's segmented radix sort (tests compare the two)
        kp_launch_anchor_compact(b->view, an, stream);
        int rc = kp_sort_anchors(ctx, an, b->n_asm, &w->sort_temp.p, &w->sort_temp.bytes, w->seg_begin(), w->seg_end(),
                                 (int)(w->key_bits.qb + w->key_bits.db) + ctx->gs_bits, stream);
        if (rc) return rc;
    }
    KP_HIP_CHECK(ctx, hipEventRecord(ev[KP_EV_SORT], stream));
    kp_launch_occ_cut(b->view, ctx->d_gene_len.p, an, w->d_occ_keys.p, w->d_occ_cnts.p, w->d_occ_state.p, w->occ_demand(), w->occ_slots, w->occ_log2, stream);
    kp_launch_chain(b->view, an, w->tasks(), w->groups(), stream);
    // kp-align v5: the chains of a group's anchors, their joined fill and walk-back need the groups and the sorted anchors only:
    // they fork off here and run on the work set's second stream beside the band tasks' order, fill and traceback
    KP_HIP_CHECK(ctx, hipMemsetAsync(w->d_task_drop.p, 0, KP_N_CLASSES * (size_t)w->task_cap, stream));
    KP_HIP_CHECK(ctx, hipEventRecord(w->ev_jfork, stream));
    KP_HIP_CHECK(ctx, hipStreamWaitEvent(w->jstream, w->ev_jfork, 0));
    const int rc = enqueue_forked(ctx, b, w, stream);
    const hipError_t e_done = hipEventRecord(w->ev_jdone, w->jstream), e_join = hipStreamWaitEvent(stream, w->ev_jdone, 0);
    if (rc) return rc;
    KP_HIP_CHECK(ctx, e_done);
    KP_HIP_CHECK(ctx, e_join);
    KP_HIP_CHECK(ctx, hipEventRecord(ev[KP_EV_JOINED], stream));
    KP_HIP_CHECK(ctx, hipEventRecord(ev[KP_EV_END], stream));
    KP_HIP_CHECK(ctx, hipGetLastError());
    return KP_OK;
}

// every stream the work set's reductions run on is idle (they read the hit tables that are about to be rewritten)
static int sync_runs(kp_ctx *ctx, KpWork *w) {
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->post));
    for (auto &r : w->runs)
        if (r && r->stream) { KP_HIP_CHECK(ctx, hipStreamSynchronize(r->stream)); if (r->aux) KP_HIP_CHECK(ctx, hipStreamSynchronize(r->aux)); }
    return KP_OK;
}

// the batch's work set with finalised hit tables, or null after recording the error
KpWork *finalised_work(kp_ctx *ctx, kp_batch *b) {
    KpWork *w = work_of(b);
    if (!w) { kp_fail(ctx, KP_ESTATE, NO_RESULTS); return nullptr; }
    if (!w->finalised) { kp_fail(ctx, KP_ESTATE, "kp_batch_wait has not completed"); return nullptr; }
    return w;
}

extern "C" {

int kp_batch_align(kp_ctx *ctx, kp_batch *b) {
    if (!ctx || !b || b->ctx != ctx) return kp_fail(ctx, KP_EINVAL, "bad context/batch");
    if (!ctx->has_db) return kp_fail(ctx, KP_ESTATE, "no database loaded");
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KpWork *w = work_of(b);
    if (!w) {  // next work set, round-robin; whoever held it loses its results
        w = &ctx->work[ctx->next_slot++ % KP_WORK_SLOTS];
        if (w->owner) {
            if (int rc = sync_runs(ctx, w)) return rc;  // its reductions may still be reading the hit tables
            w->owner->w = nullptr;
        }
        w->owner = b; w->n_asm = (size_t)b->n_asm;
        b->w = w; b->last_w = w;
    }
    kp_caps_size(ctx->opt, ctx->learnt, b->n_asm, b->view.total_words, *w);
    w->aligned = false; w->finalised = false;
    w->cs_on = ctx->opt.cs != 0; w->cs_valid = false;
    w->var_on = ctx->opt.variants != 0;
    w->aln_on = ctx->opt.aligned != 0;
    w->cigar_on = ctx->opt.cigar != 0 || w->cs_on || w->var_on || w->aln_on; w->cigar_valid = false;  // (cs, the variant records and the aligned rows read the ops)
    for (auto &v : w->h_tasks) v.clear();
    w->reset_runs();
    w->stats[KP_STAT_RERUNS] = 0;
    int rc = enqueue_align(ctx, b, w);
    if (rc) return rc;
    w->aligned = true;
    return KP_OK;
}

// hit-table finalisation on the device: compaction of the band-task results into per-assembly lists, emission order,
// duplicates, mapq.  Grows hit_cap and repeats if an assembly produced more hits than its region holds.
static int finalise_hits_on_device(kp_ctx *ctx, kp_batch *b, KpWork *w) {
    const size_t n_asm = w->n_asm;
    for (int attempt = 0;; ++attempt) {
        KP_HIP_CHECK(ctx, w->d_hits_raw.reserve(n_asm * w->hit_cap));
        KP_HIP_CHECK(ctx, w->d_hits.reserve(n_asm * w->hit_cap));
        KP_HIP_CHECK(ctx, w->d_keys.reserve(n_asm * w->hit_cap * 3));
        KP_HIP_CHECK(ctx, w->d_hit_counts.reserve(w->hit_counts_len()));
        KP_HIP_CHECK(ctx, w->d_cells.reserve(1));
        KP_HIP_CHECK(ctx, hipMemsetAsync(w->d_hit_counts.p, 0, w->hit_counts_len() * sizeof(uint32_t), ctx->post));
        KP_HIP_CHECK(ctx, hipMemsetAsync(w->d_cells.p, 0, sizeof(unsigned long long), ctx->post));
        kp_launch_hit_finalise(b->view, ctx->d_gene_len.p, w->tasks(), w->joins(), w->raw_hits(), w->hits(), w->d_cells.p, ctx->ln_half(), ctx->ln_int(), ctx->post);
        KP_HIP_CHECK(ctx, hipGetLastError());
        w->h_hit_counts.resize(w->hit_counts_len());
        unsigned long long cells = 0;
        if (int frc = fetch_all(ctx, ctx->post, {{w->h_hit_counts.data(), w->d_hit_counts.p, w->hit_counts_len() * sizeof(uint32_t)}, {&cells, w->d_cells.p, sizeof cells}}))
            return frc;
        const uint32_t max_raw = n_asm ? *std::max_element(w->h_raw_hit_count(), w->h_raw_hit_count() + n_asm) : 0;
        if (max_raw <= w->hit_cap) { w->stats[KP_STAT_CELLS] = (int64_t)cells; break; }
        if (attempt >= 2) return kp_fail(ctx, KP_EOVERFLOW, "hit buffers overflowed repeatedly");
        kp_caps_grow_hits(ctx->learnt, *w, max_raw, true);
        w->stats[KP_STAT_RERUNS] += 1;
    }
    w->hit_off.assign(n_asm + 1, 0);
    for (size_t a = 0; a < n_asm; ++a) w->hit_off[a + 1] = w->hit_off[a] + (int64_t)w->h_hit_count()[a];
    return KP_OK;
}

// CIGARs of the finished hits (kp_cigar.hip): sources located, ops counted, scanned and written on the post stream.  The ops
// buffer follows the policy of kp_caps.h; where it was too small only the writing kernel runs again -- the counts and offsets
// are exact whatever the buffer held, and the direction bits of the pass are still in the work set's trace buffer.
static int emit_cigars(kp_ctx *ctx, kp_batch *b, KpWork *w) {
    const size_t n_asm = w->n_asm;
    const int64_t total = w->hit_off[n_asm];
    w->cigar_cap = kp_caps_cigar_size(ctx->opt, ctx->learnt, (uint64_t)total);
    KP_HIP_CHECK(ctx, w->d_cig_src.reserve(n_asm * w->hit_cap));
    KP_HIP_CHECK(ctx, w->d_cig_cnt.reserve((size_t)total));
    KP_HIP_CHECK(ctx, w->d_cig_off.reserve((size_t)total + 1));
    KP_HIP_CHECK(ctx, w->d_cig_hit_off.reserve(n_asm + 1));
    KP_HIP_CHECK(ctx, w->d_cig_ops.reserve(w->cigar_cap));
    KP_HIP_CHECK(ctx, hipMemcpyAsync(w->d_cig_hit_off.p, w->hit_off.data(), (n_asm + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->post));
    kp_launch_cigar_locate(b->view, ctx->d_gene_len.p, w->tasks(), w->joins(), w->hits(), w->d_cig_src.p, ctx->post);
    kp_launch_cigar_walk(b->view, ctx->genes, w->tasks(), w->joins(), w->trace(), w->hits(), w->hit_rows(), w->d_cig_src.p, w->cigars(), false, ctx->opt.trace_summary, ctx->post);
    for (int attempt = 0;; ++attempt) {
        kp_launch_cigar_walk(b->view, ctx->genes, w->tasks(), w->joins(), w->trace(), w->hits(), w->hit_rows(), w->d_cig_src.p, w->cigars(), true, ctx->opt.trace_summary, ctx->post);
        KP_HIP_CHECK(ctx, hipGetLastError());
        int64_t need = 0;
        if (int frc = fetch_all(ctx, ctx->post, {{&need, w->d_cig_off.p + total, sizeof need}})) return frc;
        w->cigar_total = need;
        if (kp_caps_after_cigar(ctx->learnt, w->cigar_cap, (uint64_t)total, (uint64_t)need)) break;
        if (attempt >= 1) return kp_fail(ctx, KP_EOVERFLOW, "CIGAR buffer overflowed repeatedly");
        KP_HIP_CHECK(ctx, w->d_cig_ops.reserve(w->cigar_cap));
    }
    w->cigar_valid = true;
    return KP_OK;
}

// cs strings of the finished hits (kp_cs.hip), on the post stream behind emit_cigars -- whose ops are final by now, a grown and
// rewritten buffer included.  Bytes counted, scanned and written; the byte buffer follows the policy of kp_caps.h, and where it was
// too small only the writing kernel runs again: counts and offsets are exact whatever the buffer held.
static int emit_cs(kp_ctx *ctx, kp_batch *b, KpWork *w) {
    const int64_t total = w->hit_off[w->n_asm];
    w->cs_cap = kp_caps_cs_size(ctx->cs_caps, (uint64_t)total);
    KP_HIP_CHECK(ctx, w->d_cs_cnt.reserve((size_t)total));
    KP_HIP_CHECK(ctx, w->d_cs_off.reserve((size_t)total + 1));
    KP_HIP_CHECK(ctx, w->d_cs_bytes.reserve(w->cs_cap));
    kp_launch_cs_walk(b->view, ctx->genes, w->hits(), w->hit_rows(), w->cigars(), w->cs(), false, ctx->post);
    for (int attempt = 0;; ++attempt) {
        kp_launch_cs_walk(b->view, ctx->genes, w->hits(), w->hit_rows(), w->cigars(), w->cs(), true, ctx->post);
        KP_HIP_CHECK(ctx, hipGetLastError());
        int64_t need = 0;
        if (int frc = fetch_all(ctx, ctx->post, {{&need, w->d_cs_off.p + total, sizeof need}})) return frc;
        w->cs_total = need;
        if (kp_caps_after_cs(ctx->cs_caps, w->cs_cap, (uint64_t)total, (uint64_t)need)) break;
        if (attempt >= 1) return kp_fail(ctx, KP_EOVERFLOW, "cs buffer overflowed repeatedly");
        KP_HIP_CHECK(ctx, w->d_cs_bytes.reserve(w->cs_cap));
    }
    w->cs_valid = true;
    return KP_OK;
}

static const char *const NO_CS = "this batch has no cs strings (aligned without the cs option, or its hit table was replaced)";
static const char *const NO_CIGARS = "this batch has no CIGARs (aligned without the cigar option, or its hit table was replaced)";

int kp_batch_wait(kp_ctx *ctx, kp_batch *b) {
    if (!ctx || !b || b->ctx != ctx) return kp_fail(ctx, KP_EINVAL, "bad context/batch");
    KpWork *w = work_of(b);
    if (!w || !w->aligned) return kp_fail(ctx, KP_ESTATE, w ? "kp_batch_align has not been called" : NO_RESULTS);
    if (w->finalised) return KP_OK;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t n_asm = w->n_asm;
    const uint32_t *const n_join = w->h_join_count();
    for (;;) {
        // the post stream picks up where this batch's alignment pass ends; later passes on ctx->stream are not waited for
        KP_HIP_CHECK(ctx, hipStreamWaitEvent(ctx->post, w->ev[KP_EV_END], 0));
        w->h_counts.resize(w->counts_len());
        unsigned long long n_cand[KP_CAND_COUNTS] = {}, top[KP_TOP_WORDS] = {};
        if (int frc = fetch_all(ctx, ctx->post, {{w->h_counts.data(), w->d_counts.p, w->counts_len() * sizeof(uint32_t)},
                                                 {n_cand, w->d_cand_count.p, sizeof n_cand}, {top, w->d_trace_top.p, sizeof top},
                                                 {w->h_join_counts, w->d_join_counts.p, sizeof w->h_join_counts}}))
            return frc;
        KpPassSeen seen;
        seen.n_asm = n_asm; seen.total_words = b->view.total_words; seen.n_cand = n_cand[KP_CAND_FRONT] + n_cand[KP_CAND_BACK];
        seen.trace_need = top[KP_TOP_TRACE]; seen.occ_need = top[KP_TOP_OCC];
        seen.n_group = w->h_group_count();
        for (int c = 0; c < KP_N_CLASSES; ++c) seen.max_join = std::max(seen.max_join, n_join[c]);
        for (size_t a = 0; a < n_asm; ++a) seen.max_slice = std::max(seen.max_slice, w->h_slice_need()[a]);
        for (int c = 0; c < KP_N_CLASSES; ++c) seen.max_task = std::max(seen.max_task, w->h_task_count()[c]);
        if (ctx->opt.join_stats)
            std::fprintf(stderr, "[kp_batch_wait] %zu assemblies: %u groups, joins per band class %u %u %u %u, %llu assemblies needed their mid_occ (%u tables)\n", n_asm, seen.n_group,
                         n_join[0], n_join[1], n_join[2], n_join[3], (unsigned long long)seen.occ_need, w->occ_slots);
        std::string err;
        const KpCapsVerdict verdict = kp_caps_after_pass(ctx->learnt, *w, seen, err);
        if (verdict == KP_CAPS_FITTED) break;
        if (verdict == KP_CAPS_OVERFLOW) return kp_fail(ctx, KP_EOVERFLOW, err);
        w->stats[KP_STAT_RERUNS] += 1;
        int rc = enqueue_align(ctx, b, w);
        if (rc) return rc;
    }
    int64_t n_anchor = 0, n_task = 0;
    for (size_t a = 0; a < n_asm; ++a) n_anchor += w->h_anchor_count()[a];
    for (int c = 0; c < KP_N_CLASSES; ++c) n_task += w->h_task_count()[c];
    for (auto &v : w->h_tasks) v.clear();
    w->h_joins.clear();
    int rc = finalise_hits_on_device(ctx, b, w);
    if (rc) return rc;
    w->stats[KP_STAT_ANCHORS] = n_anchor; w->stats[KP_STAT_TASKS] = n_task; w->stats[KP_STAT_HITS] = w->hit_off[n_asm];
    if (w->cigar_on)
        if (int crc = emit_cigars(ctx, b, w)) return crc;
    if (w->cs_on)
        if (int crc = emit_cs(ctx, b, w)) return crc;
    w->finalised = true;
    return KP_OK;
}

int kp_batch_hit_offsets(kp_ctx *ctx, kp_batch *b, int64_t *hit_off) {
    if (!ctx || !b || b->ctx != ctx || !hit_off) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    std::memcpy(hit_off, w->hit_off.data(), w->hit_off.size() * sizeof(int64_t));
    return KP_OK;
}

int kp_batch_hits(kp_ctx *ctx, kp_batch *b, kp_hit *out, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || (!out && cap > 0)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    const size_t n_asm = w->n_asm;
    const KpHitTable hits = w->hits();
    if (cap < w->hit_off[n_asm]) return kp_fail(ctx, KP_EINVAL, "hit buffer too small");
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    for (size_t a = 0; a < n_asm; ++a) {  // regions are contiguous per assembly; copy each used prefix
        const int64_t n = w->hit_off[a + 1] - w->hit_off[a];
        if (n > 0)
            KP_HIP_CHECK(ctx, hipMemcpyAsync(out + w->hit_off[a], hits.of(a), (size_t)n * sizeof(kp_hit), hipMemcpyDeviceToHost, ctx->post));
    }
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->post));
    return KP_OK;
}

int kp_batch_set_hits(kp_ctx *ctx, kp_batch *b, const kp_hit *hits, const int64_t *hit_off) {
    if (!ctx || !b || b->ctx != ctx || !hit_off) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    const size_t n_asm = w->n_asm;
    int64_t max_n = 0;
    for (size_t a = 0; a < n_asm; ++a) {
        const int64_t n = hit_off[a + 1] - hit_off[a];
        if (n < 0 || (n > 0 && !hits)) return kp_fail(ctx, KP_EINVAL, "hit offsets must ascend");
        max_n = std::max(max_n, n);
    }
    if (max_n > (1 << 24)) return kp_fail(ctx, KP_EOVERFLOW, "too many hits for one assembly");
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = sync_runs(ctx, w)) return rc;  // nothing may still be reading the table that is about to be replaced
    if ((uint64_t)max_n > w->hit_cap) kp_caps_grow_hits(ctx->learnt, *w, (uint32_t)max_n, false);
    KP_HIP_CHECK(ctx, w->d_hits.reserve(n_asm * w->hit_cap));
    KP_HIP_CHECK(ctx, w->d_hit_counts.reserve(w->hit_counts_len()));
    w->h_hit_counts.resize(w->hit_counts_len());
    const KpHitTable table = w->hits();
    w->hit_off.assign(n_asm + 1, 0);
    for (size_t a = 0; a < n_asm; ++a) {
        const int64_t n = hit_off[a + 1] - hit_off[a];
        if (n > 0)
            KP_HIP_CHECK(ctx, hipMemcpy(table.of(a), hits + hit_off[a], (size_t)n * sizeof(kp_hit), hipMemcpyHostToDevice));
        w->h_hit_count()[a] = (uint32_t)n;
        w->hit_off[a + 1] = w->hit_off[a] + n;
    }
    if (n_asm)
        KP_HIP_CHECK(ctx, hipMemcpy(table.count, w->h_hit_count(), n_asm * sizeof(uint32_t), hipMemcpyHostToDevice));
    w->stats[KP_STAT_HITS] = w->hit_off[n_asm];
    w->cigar_valid = false; w->cs_valid = false;  // (they described the table that has just been replaced)
    w->reset_runs();
    return KP_OK;
}

int kp_batch_cigar_offsets(kp_ctx *ctx, kp_batch *b, int64_t *cigar_off) {
    if (!ctx || !b || b->ctx != ctx || !cigar_off) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    if (!w->cigar_valid) return kp_fail(ctx, KP_ESTATE, NO_CIGARS);
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KP_HIP_CHECK(ctx, hipMemcpyAsync(cigar_off, w->d_cig_off.p, ((size_t)w->hit_off[(size_t)b->n_asm] + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->post));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->post));
    return KP_OK;
}

int kp_batch_cigars(kp_ctx *ctx, kp_batch *b, uint32_t *ops, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || (!ops && cap > 0)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    if (!w->cigar_valid) return kp_fail(ctx, KP_ESTATE, NO_CIGARS);
    if (cap < w->cigar_total) return kp_fail(ctx, KP_EINVAL, "CIGAR buffer too small");
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (w->cigar_total > 0) {
        KP_HIP_CHECK(ctx, hipMemcpyAsync(ops, w->d_cig_ops.p, (size_t)w->cigar_total * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->post));
        KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->post));
    }
    return KP_OK;
}

int kp_batch_cs_offsets(kp_ctx *ctx, kp_batch *b, int64_t *cs_off) {
    if (!ctx || !b || b->ctx != ctx || !cs_off) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    if (!w->cs_valid) return kp_fail(ctx, KP_ESTATE, NO_CS);
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KP_HIP_CHECK(ctx, hipMemcpyAsync(cs_off, w->d_cs_off.p, ((size_t)w->hit_off[(size_t)b->n_asm] + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, ctx->post));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->post));
    return KP_OK;
}

int kp_batch_cs(kp_ctx *ctx, kp_batch *b, char *bytes, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || (!bytes && cap > 0)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    if (!w->cs_valid) return kp_fail(ctx, KP_ESTATE, NO_CS);
    if (cap < w->cs_total) return kp_fail(ctx, KP_EINVAL, "cs buffer too small");
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (w->cs_total > 0) {
        KP_HIP_CHECK(ctx, hipMemcpyAsync(bytes, w->d_cs_bytes.p, (size_t)w->cs_total, hipMemcpyDeviceToHost, ctx->post));
        KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->post));
    }
    return KP_OK;
}

int kp_batch_stats(kp_ctx *ctx, kp_batch *b, int64_t *stats5) {
    if (!ctx || !b || b->ctx != ctx || !stats5) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    std::memcpy(stats5, w->stats, sizeof w->stats);
    return KP_OK;
}

int kp_batch_profile(kp_ctx *ctx, kp_batch *b, float *ms7, int64_t *bytes_scanned) {
    if (!ctx || !b || b->ctx != ctx || !ms7) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    for (int i = KP_EV_START; i < KP_EV_END; ++i) {  // seven consecutive intervals
        const KpPassEvent next = KpPassEvent(i + 1);
        if (hipEventElapsedTime(&ms7[i], w->ev[i], w->ev[next]) != hipSuccess) return kp_fail(ctx, KP_EHIP, "event timing failed");
    }
    if (bytes_scanned) *bytes_scanned = 4 * b->view.total_words;
    return KP_OK;
}

int64_t kp_batch_anchors(kp_ctx *ctx, kp_batch *b, int32_t a, uint64_t *out, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || a < 0 || a >= b->n_asm) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    const int64_t n = w->h_anchor_count()[a];
    const int64_t m = std::min(n, cap);
    if (out && m > 0) {
        if (hipMemcpy(out, w->anchors().of((size_t)a), (size_t)m * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
            return kp_fail(ctx, KP_EHIP, "D2H anchors failed");
        for (int64_t i = 0; i < m; ++i) out[i] = kp_key_unpack(out[i], w->key_bits);  // callers see the spec's layout
    }
    return n;
}

int64_t kp_batch_tasks(kp_ctx *ctx, kp_batch *b, int32_t a, int32_t *out8, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || a < 0 || a >= b->n_asm) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    for (int c = 0; c < KP_N_CLASSES; ++c) {  // fetched on first use: only the stage tests look at tasks
        const size_t nt = w->h_task_count()[c];
        if (w->h_tasks[c].size() == nt) continue;
        w->h_tasks[c].resize(nt);
        if (nt && hipMemcpy(w->h_tasks[c].data(), w->tasks().cls(c), nt * sizeof(KpTask), hipMemcpyDeviceToHost) != hipSuccess)
            return kp_fail(ctx, KP_EHIP, "D2H tasks failed");
    }
    int64_t n = 0;
    for (int c = 0; c < KP_N_CLASSES; ++c)
        for (const KpTask &t : w->h_tasks[c]) {
            if (t.asm_id != a || t.n_anchors == 0) continue;  // (n_anchors == 0: a cluster the chaining rejected)
            if (out8 && n < cap) {
                int32_t *o = out8 + 8 * n;
                o[0] = t.gs; o[1] = t.contig; o[2] = t.lo; o[3] = t.width; o[4] = t.n_anchors; o[5] = (int32_t)(t.qspan & 0xFFFFu); o[6] = (int32_t)(t.qspan >> 16); o[7] = t.chain_score;
            }
            ++n;
        }
    return n;
}

int64_t kp_batch_task_results(kp_ctx *ctx, kp_batch *b, int32_t a, int32_t *out7, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || a < 0 || a >= b->n_asm) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    const int64_t n_tasks = kp_batch_tasks(ctx, b, a, nullptr, 0);  // (also fetches the task lists)
    if (n_tasks < 0) return n_tasks;
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    int64_t n = 0;
    std::vector<KpSwResult> res;
    for (int c = 0; c < KP_N_CLASSES; ++c) {
        const size_t nt = w->h_tasks[c].size();
        res.resize(nt);
        if (nt && hipMemcpy(res.data(), w->tasks().cls_results(c), nt * sizeof(KpSwResult), hipMemcpyDeviceToHost) != hipSuccess)
            return kp_fail(ctx, KP_EHIP, "D2H task results failed");
        for (size_t i = 0; i < nt; ++i) {
            if (w->h_tasks[c][i].asm_id != a || w->h_tasks[c][i].n_anchors == 0) continue;
            if (out7 && n < cap) {
                const KpSwResult &r = res[i];
                int32_t *o = out7 + 7 * n;
                o[0] = r.score; o[1] = r.q_start; o[2] = r.q_end; o[3] = r.t_start; o[4] = r.t_end; o[5] = r.matches; o[6] = r.block_len;
            }
            ++n;
        }
    }
    return n;
}

int64_t kp_batch_joins(kp_ctx *ctx, kp_batch *b, int32_t a, int32_t *out, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || a < 0 || a >= b->n_asm) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    size_t total = 0;
    for (int c = 0; c < KP_N_CLASSES; ++c) total += w->h_join_count()[c];
    if (w->h_joins.size() != total) {  // fetched on first use: only the stage tests look at joins
        w->h_joins.resize(total);
        size_t at = 0;
        for (int c = 0; c < KP_N_CLASSES; ++c) {
            const size_t nj = w->h_join_count()[c];
            if (nj && hipMemcpy(w->h_joins.data() + at, w->joins().cls(c), nj * sizeof(KpJoin), hipMemcpyDeviceToHost) != hipSuccess)
                return kp_fail(ctx, KP_EHIP, "D2H joins failed");
            at += nj;
        }
    }
    int64_t n = 0;
    for (const KpJoin &J : w->h_joins) {
        if (J.asm_id != a) continue;
        if (out && n < cap) {
            int32_t *o = out + KP_JOIN_ROW_INTS * n;
            std::memset(o, 0, KP_JOIN_ROW_INTS * sizeof(int32_t));
            o[0] = J.gs; o[1] = J.contig; o[2] = J.n_pieces; o[3] = J.n_anchors; o[4] = J.chain_score; o[5] = J.width;
            for (int k = 0; k < J.n_pieces; ++k) {
                o[6 + k] = J.lo[k];
                int32_t *pr = o + 6 + KP_JOIN_MAX_PIECES + 11 * k;
                pr[0] = J.state[k]; pr[1] = J.visited[k];
                if (J.state[k] == 1) std::memcpy(pr + 2, J.res[k], 9 * sizeof(int32_t));
            }
        }
        ++n;
    }
    return n;
}

int64_t kp_batch_occ(kp_ctx *ctx, kp_batch *b, int32_t a, uint32_t *out, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || a < 0 || a >= b->n_asm) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    // what the pass left (kp_chain.hip, OccScratch): [n_asm] state, [n_asm] mid_occ, [occ_slots] the tables' assemblies
    const size_t n_asm = w->n_asm;
    uint32_t head[2] = {0, (uint32_t)KP_MID_OCC};
    unsigned long long demand = 0;
    if (hipMemcpy(&head[0], w->d_occ_state.p + a, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&demand, w->occ_demand(), sizeof demand, hipMemcpyDeviceToHost) != hipSuccess)
        return kp_fail(ctx, KP_EHIP, "D2H occurrence-cut state failed");
    int64_t n = 2;
    if (head[0] & 2u) {  // the assembly claimed a table: its mid_occ, and the table among those the pass handed out
        if (hipMemcpy(&head[1], w->d_occ_state.p + n_asm + a, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
            return kp_fail(ctx, KP_EHIP, "D2H occurrence-cut state failed");
        const size_t n_slots = (size_t)std::min<unsigned long long>(demand, w->occ_slots), size = (size_t)1 << w->occ_log2;
        // (a stage test's accessor: the size query and the call that fills `out` each fetch the whole table, 2 x 4 x 2^occ_log2 bytes;
        // nothing is kept on the host between them, unlike h_tasks / h_joins, which every assembly of a batch shares)
        std::vector<uint32_t> owner(n_slots), keys(size), cnts(size);
        if (n_slots && hipMemcpy(owner.data(), w->d_occ_state.p + 2 * n_asm, n_slots * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
            return kp_fail(ctx, KP_EHIP, "D2H occurrence-cut state failed");
        size_t slot = 0;
        while (slot < n_slots && owner[slot] != (uint32_t)a) ++slot;
        if (slot == n_slots) return kp_fail(ctx, KP_ESTATE, "the occurrence cut's state names no counting table for this assembly");
        if (hipMemcpy(keys.data(), w->d_occ_keys.p + slot * size, size * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(cnts.data(), w->d_occ_cnts.p + slot * size, size * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
            return kp_fail(ctx, KP_EHIP, "D2H occurrence-cut table failed");
        for (size_t i = 0; i < size; ++i) {
            if (keys[i] == 0xFFFFFFFFu && cnts[i] == 0) continue;  // (an empty entry; a key without a count, or the reverse, is reported)
            if (out && n + 2 <= cap) { out[n] = keys[i]; out[n + 1] = cnts[i]; }
            n += 2;
        }
    }
    if (out && cap >= 2) { out[0] = head[0]; out[1] = head[1]; }
    return n;
}

int64_t kp_batch_candidates(kp_ctx *ctx, kp_batch *b, uint64_t *out, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || (out && cap < 0)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    // what the last pass's scan left (kp_scan.hip): the streaming kernel's words from the list's front, the edge kernel's from its back
    unsigned long long n_cand[KP_CAND_COUNTS] = {};
    if (hipMemcpy(n_cand, w->d_cand_count.p, sizeof n_cand, hipMemcpyDeviceToHost) != hipSuccess)
        return kp_fail(ctx, KP_EHIP, "D2H candidate counts failed");
    const uint64_t n_front = n_cand[KP_CAND_FRONT], n_back = n_cand[KP_CAND_BACK];
    if (n_front + n_back > w->cand_cap) return kp_fail(ctx, KP_ESTATE, "the last pass's candidate list overflowed: it holds no whole list");
    const int64_t n = KP_CAND_COUNTS + (int64_t)(n_front + n_back);
    if (!out) return n;
    if (cap < n) return kp_fail(ctx, KP_EINVAL, "candidate buffer too small");
    out[KP_CAND_FRONT] = n_front; out[KP_CAND_BACK] = n_back;
    uint64_t *front = out + KP_CAND_COUNTS, *back = front + n_front;
    if ((n_front && hipMemcpy(front, w->d_cand.p, n_front * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) ||
        (n_back && hipMemcpy(back, w->d_cand.p + (w->cand_cap - n_back), n_back * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess))
        return kp_fail(ctx, KP_EHIP, "D2H candidates failed");
    std::reverse(back, back + n_back);  // entry k of the back list lies at cand[cand_cap - 1 - k]
    return n;
}

}  // extern "C"
