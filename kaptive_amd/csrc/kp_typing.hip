// kp_typing.hip -- batched typing (locus scores, the reduction of a batch's hits, gene states, the variant and breakpoint records, the allele
// digests and the aligned rows of the kept hits; per typing group), stand-alone protein aligner.
#include "kp_host.h"

// the typing group a batch currently addresses and the run of the batch's work set for it (created on first use)
static KpTypingGroup *typing_group(kp_ctx *ctx, const kp_batch *b) {
    return (size_t)b->group < ctx->groups.size() ? ctx->groups[(size_t)b->group].get() : nullptr;
}
static KpTypingRun &typing_run(KpWork *w, int32_t group) {
    if (w->runs.size() <= (size_t)group) w->runs.resize((size_t)group + 1);
    if (!w->runs[(size_t)group]) w->runs[(size_t)group].reset(new KpTypingRun());
    return *w->runs[(size_t)group];
}
static KpRunCaps &run_caps(kp_ctx *ctx, int32_t group) {
    if (ctx->run_caps.size() <= (size_t)group) ctx->run_caps.resize((size_t)group + 1);
    KpRunCaps &c = ctx->run_caps[(size_t)group];
    if (c.kept_cap == 0) c.kept_cap = (int)ctx->opt.kept_cap;
    if (c.piece_cap == 0) c.piece_cap = (int)ctx->opt.piece_cap;
    if (c.prot_cap == 0) c.prot_cap = (int)ctx->opt.prot_cap;
    return c;
}
static int ensure_run_streams(kp_ctx *ctx, KpTypingRun &R, int32_t group) {
    if (R.stream) return KP_OK;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (ctx->group_streams.size() <= (size_t)group) ctx->group_streams.resize((size_t)group + 1);
    kp_ctx::GroupStreams &gs = ctx->group_streams[(size_t)group];
    if (!gs.stream) {
        KP_HIP_CHECK(ctx, create_priority_stream(&gs.stream.h));
        KP_HIP_CHECK(ctx, create_priority_stream(&gs.aux.h));
    }
    R.stream = gs.stream; R.aux = gs.aux;
    KP_HIP_CHECK(ctx, hipEventCreateWithFlags(&R.ev_fork.h, hipEventDisableTiming));
    KP_HIP_CHECK(ctx, hipEventCreateWithFlags(&R.ev_join.h, hipEventDisableTiming));
    return KP_OK;
}

// A buffer whose rows are read back beyond what the kernels wrote (the kept and piece rows behind an assembly's counts): zeroed
// whenever it is (re)allocated, so that those bytes never depend on what the device memory held before -- a settled context
// allocates nothing and pays nothing.
template <class T>
static hipError_t reserve_zeroed(DevBuf<T> &buf, size_t want, hipStream_t stream) {
    const size_t had = buf.n;
    hipError_t e = buf.reserve(want);
    if (e == hipSuccess && buf.n != had) e = hipMemsetAsync(buf.p, 0, buf.n * sizeof(T), stream);
    return e;
}

extern "C" {

int kp_batch_use_group(kp_ctx *ctx, kp_batch *b, int32_t group) {
    if (!ctx || !b || b->ctx != ctx) return kp_fail(ctx, KP_EINVAL, "bad context/batch");
    if (group < 0 || (size_t)group >= ctx->groups.size() || !ctx->groups[(size_t)group])
        return kp_fail(ctx, KP_EINVAL, "no typing tables loaded for this group");
    b->group = group;
    return KP_OK;
}

// the group's hits out of the batch's finalised hit table (sorted by gene, so they are one run per assembly), with gene
// indices made relative to the group's first gene.  A group that spans every gene of the context reads the table in place.
static int split_hits(kp_ctx *ctx, kp_batch *b, KpWork *w, const KpTypingGroup &T, KpTypingRun &R) {
    if (R.split) return KP_OK;
    if (T.gene_lo == 0 && T.gene_hi == ctx->n_genes) {
        R.hits = w->hits();
    } else {
        KP_HIP_CHECK(ctx, R.d_hits.reserve(w->n_asm * w->hit_cap));
        KP_HIP_CHECK(ctx, R.d_hit_n.reserve(w->n_asm));
        R.hits = KpHitTable{.rows = R.d_hits.p, .count = R.d_hit_n.p, .cap = w->hit_cap, .keys = nullptr};
        kp_launch_hit_split(w->hits(), T.gene_lo, T.gene_hi, R.hits, b->n_asm, R.stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
    }
    R.split = true;
    return KP_OK;
}

int kp_batch_score(kp_ctx *ctx, kp_batch *b, double min_gene_coverage, double *locus_scores, int32_t *locus_counts) {
    if (!ctx || !b || b->ctx != ctx || !locus_scores || !locus_counts) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingGroup *Tp = typing_group(ctx, b);
    if (!Tp) return kp_fail(ctx, KP_ESTATE, "kp_db_load_typing has not been called");
    KpTypingGroup &T = *Tp;
    int rc = kp_batch_wait(ctx, b);  // hit tables final (and the post stream idle) when this returns
    if (rc) return rc;
    KpWork *w = work_of(b);
    KpTypingRun &R = typing_run(w, b->group);
    if ((rc = ensure_run_streams(ctx, R, b->group))) return rc;
    if ((rc = split_hits(ctx, b, w, T, R))) return rc;
    const size_t n = (size_t)b->n_asm * (size_t)T.typing.n_loci;
    KP_HIP_CHECK(ctx, R.d_scores.reserve(n));
    KP_HIP_CHECK(ctx, R.d_lcounts.reserve(n));
    kp_launch_score(b->view, R.hits, T.typing, min_gene_coverage, R.d_scores.p, R.d_lcounts.p, R.stream);
    KP_HIP_CHECK(ctx, hipGetLastError());
    if (int frc = fetch_all(ctx, R.stream, {{locus_scores, R.d_scores.p, n * sizeof(double)}, {locus_counts, R.d_lcounts.p, n * sizeof(int32_t)}}))
        return frc;
    R.prm.min_gene_coverage = min_gene_coverage;
    R.scored = true;
    return KP_OK;
}

static int enqueue_reduce(kp_ctx *ctx, kp_batch *b, KpWork *w) {
    KpTypingGroup &T = *typing_group(ctx, b);
    KpTypingRun &R = typing_run(w, b->group);
    const KpRunCaps caps = run_caps(ctx, b->group);
    R.kept_cap = caps.kept_cap; R.piece_cap = caps.piece_cap; R.prot_cap = caps.prot_cap;
    const size_t n_asm = R.n_asm = w->n_asm;
    if ((uint64_t)n_asm * (uint64_t)R.prot_cap > 0x7FFFFFFFull)
        return kp_fail(ctx, KP_EOVERFLOW, "protein buffer would exceed 2^31 bytes; use smaller batches");
    const size_t slots = R.slots();
    KP_HIP_CHECK(ctx, R.d_keys.reserve(n_asm * w->hit_cap));
    KP_HIP_CHECK(ctx, R.d_order.reserve(n_asm * w->hit_cap));
    KP_HIP_CHECK(ctx, R.d_flag.reserve(n_asm * w->hit_cap));
    KP_HIP_CHECK(ctx, reserve_zeroed(R.d_kept, slots, R.stream));
    KP_HIP_CHECK(ctx, reserve_zeroed(R.d_pieces, n_asm * (size_t)R.piece_cap, R.stream));
    KP_HIP_CHECK(ctx, R.d_summary.reserve(n_asm));
    KP_HIP_CHECK(ctx, R.d_prot.reserve(n_asm * (size_t)R.prot_cap));
    KP_HIP_CHECK(ctx, R.d_pairs.reserve(R.pairs_len()));
    KP_HIP_CHECK(ctx, R.d_dp.reserve(8 * slots));
    const KpReduceTables t = R.tables();
    KP_HIP_CHECK(ctx, hipMemsetAsync(t.n_pairs, 0, sizeof(int32_t), R.stream));
    kp_launch_reduce(b->view, R.hits, T.typing, R.prm, t, R.stream);
    // protein DP of every kept hit against its database protein (pair list is compact; its length lives on the device)
    const int n_blocks = (int)std::min<size_t>(std::max<size_t>(slots, 1), 256 * 24);
    // row buffer of the strip kernel: KP_PROT_ROWBUF_FIELDS ints per column of the database protein, one region per
    // block, and 64 ints for its work counter (kp_prot.hip)
    const size_t scratch_per_block = (size_t)KP_PROT_ROWBUF_FIELDS * ((size_t)T.max_db_prot_len + 1);
    KP_HIP_CHECK(ctx, R.d_dp_scratch.reserve(scratch_per_block * (size_t)n_blocks + 64));
    kp_launch_protein(t.prot, t.q_off, t.q_len, T.d_prot_db.p, t.t_off, t.t_len, (int32_t)slots, t.n_pairs, ctx->d_blosum.p,
                      t.dp8, R.d_dp_scratch.p, scratch_per_block, n_blocks, R.stream, R.aux, R.ev_fork, R.ev_join);
    kp_launch_states(b->view, T.typing, R.prm, t, R.stream);
    KP_HIP_CHECK(ctx, hipGetLastError());
    return KP_OK;
}

int kp_batch_reduce(kp_ctx *ctx, kp_batch *b, const int32_t *best_locus, const kp_typing_params *prm) {
    if (!ctx || !b || b->ctx != ctx || !prm || (b->n_asm > 0 && !best_locus)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingGroup *Tp = typing_group(ctx, b);
    if (!Tp) return kp_fail(ctx, KP_ESTATE, "kp_db_load_typing has not been called");
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    KpTypingRun &R = typing_run(w, b->group);
    if (!R.scored) return kp_fail(ctx, KP_ESTATE, "kp_batch_score has not been called");
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    for (int a = 0; a < b->n_asm; ++a)
        if (best_locus[a] < 0 || best_locus[a] >= Tp->typing.n_loci) return kp_fail(ctx, KP_EINVAL, "best_locus out of range");
    R.prm = *prm;
    int rc;
    if (ctx->opt.readback_copy_engine) {
        rc = upload(ctx, R.d_best, best_locus, (size_t)b->n_asm, R.stream);
    } else {  // through the landing area and a kernel, like the read-backs: a copy-engine upload queues behind the shard in flight
        Fetch f(ctx, R.stream);
        const size_t bytes = (size_t)b->n_asm * sizeof(int32_t);
        if ((rc = f.begin(bytes))) return rc;
        KP_HIP_CHECK(ctx, R.d_best.reserve((size_t)b->n_asm));
        if (bytes) {
            std::memcpy(ctx->bounce.p, best_locus, bytes);
            kp_launch_read_back(ctx->bounce.p, R.d_best.p, bytes, R.stream);
        }
    }
    if (rc == KP_OK && hipStreamSynchronize(R.stream) != hipSuccess) rc = kp_fail(ctx, KP_EHIP, "H2D best loci failed");
    if (rc) return rc;
    rc = enqueue_reduce(ctx, b, w);
    if (rc) return rc;
    R.reduced = true;
    R.sums_valid = false;
    R.var_valid = false;  // (the variant records describe a kept list: the one that is about to be replaced)
    R.src_valid = false;  // (... and so do the hit rows behind its records
    R.aln_valid = false;  //  and the aligned rows)
    R.bp_valid = false;   // (the breakpoint records likewise)
    R.al_valid = false;   // (... and the allele digests)
    return KP_OK;
}

// waits for the reduction, re-runs it with larger buffers while any assembly overflowed one, and keeps the summaries
static int fetch_summaries(kp_ctx *ctx, kp_batch *b, KpWork *w) {
    KpTypingRun &R = typing_run(w, b->group);
    if (R.sums_valid) return KP_OK;
    const size_t n_asm = (size_t)b->n_asm;
    R.h_sums.resize(n_asm);
    for (int attempt = 0;; ++attempt) {
        if (int frc = fetch_all(ctx, R.stream, {{R.h_sums.data(), R.d_summary.p, n_asm * sizeof(KpAsmSummary)}})) return frc;
        int flags = 0;
        for (const auto &s : R.h_sums) flags |= s.overflow;
        if (flags & 4) return kp_fail(ctx, KP_EINVAL, "a locus has more genes than KP_MAX_LOCUS_GENES");
        if (!(flags & (1 | 2 | 8))) break;
        if (attempt >= 8) return kp_fail(ctx, KP_EOVERFLOW, "reduction buffers overflowed repeatedly");
        std::string err;
        if (!kp_caps_grow_run(run_caps(ctx, b->group), flags, err)) return kp_fail(ctx, KP_EOVERFLOW, err);
        w->stats[KP_STAT_RERUNS] += 1;
        int rc = enqueue_reduce(ctx, b, w);
        if (rc) return rc;
    }
    R.max_kept = 1; R.max_pieces = 1;
    for (const auto &s : R.h_sums) {
        R.max_kept = std::max(R.max_kept, s.n_kept);
        R.max_pieces = std::max(R.max_pieces, s.n_pieces);
    }
    R.sums_valid = true;
    return KP_OK;
}

// the run of the batch's current group after kp_batch_reduce, or null after recording the error
static KpTypingRun *reduced_run(kp_ctx *ctx, kp_batch *b, KpWork **w_out) {
    KpWork *w = finalised_work(ctx, b);
    if (!w) return nullptr;
    KpTypingRun &R = typing_run(w, b->group);
    if (!R.reduced) { kp_fail(ctx, KP_ESTATE, "kp_batch_reduce has not been called"); return nullptr; }
    *w_out = w;
    return &R;
}

int kp_batch_typing(kp_ctx *ctx, kp_batch *b, kp_asm_summary *summaries, kp_kept *kept, int32_t kept_stride, kp_piece *pieces, int32_t piece_stride) {
    if (!ctx || !b || b->ctx != ctx || (b->n_asm > 0 && (!summaries || !kept || !pieces)))
        return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = nullptr;
    KpTypingRun *Rp = reduced_run(ctx, b, &w);
    if (!Rp) return KP_ESTATE;
    KpTypingRun &R = *Rp;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t n_asm = (size_t)b->n_asm;
    int rc = fetch_summaries(ctx, b, w);
    if (rc) return rc;
    if (n_asm == 0) return KP_OK;
    if (kept_stride < R.max_kept || piece_stride < R.max_pieces)
        return kp_fail(ctx, KP_EINVAL, "output strides too small (see kp_batch_typing_caps)");
    std::memcpy(summaries, R.h_sums.data(), n_asm * sizeof(KpAsmSummary));
    // rows of the device buffers are kept_cap / piece_cap records long; only the first `stride` records of each are
    // wanted (a batch keeps a few dozen hits per assembly, the buffers leave room for hundreds): packed on the device,
    // then one linear copy each
    const size_t kw = (size_t)std::min(kept_stride, R.kept_cap) * sizeof(KpKept) / 4;
    const size_t pw = (size_t)std::min(piece_stride, R.piece_cap) * sizeof(KpPiece) / 4;
    {   // sized from the most any batch of this typing group has needed (plus a quarter), whichever work set it ran on: the
        // fullest assembly of a batch decides the strides, and three work sets learning that one by one re-allocate for steps
        size_t &hw = run_caps(ctx, b->group).pack_items;
        const size_t need = n_asm * ((size_t)kept_stride * sizeof(KpKept) + (size_t)piece_stride * sizeof(KpPiece)) / 4;
        if (need > hw) hw = need + need / 4;
        KP_HIP_CHECK(ctx, reserve_zeroed(R.d_pack, hw, R.stream));
    }
    uint32_t *pk = R.d_pack.p, *pp = pk + n_asm * (size_t)kept_stride * sizeof(KpKept) / 4;
    kp_launch_pack_rows(reinterpret_cast<const uint32_t *>(R.d_kept.p), (size_t)R.kept_cap * sizeof(KpKept) / 4, pk, (size_t)kept_stride * sizeof(KpKept) / 4, kw, (int)n_asm, R.stream);
    kp_launch_pack_rows(reinterpret_cast<const uint32_t *>(R.d_pieces.p), (size_t)R.piece_cap * sizeof(KpPiece) / 4, pp, (size_t)piece_stride * sizeof(KpPiece) / 4, pw, (int)n_asm, R.stream);
    const size_t kb = n_asm * (size_t)kept_stride * sizeof(KpKept), pb = n_asm * (size_t)piece_stride * sizeof(KpPiece);
    if (int frc = fetch_all(ctx, R.stream, {{kept, pk, kb}, {pieces, pp, pb}})) return frc;
    // identity sums use numpy's float32 association; a few dozen adds per assembly, done here on the copied rows
    std::vector<float> vals;
    for (size_t a = 0; a < n_asm; ++a) {
        vals.clear();
        const KpKept *k = kept + a * (size_t)kept_stride;
        for (int i = 0; i < summaries[a].n_kept; ++i)
            if (!(k[i].flags & KP_F_SPURIOUS) && k[i].state == KP_STATE_NORMAL) vals.push_back(k[i].pident);
        summaries[a].n_normal = (int32_t)vals.size();
        summaries[a].ident_sum = kp_np_sum_f32(vals.data(), (int)vals.size());
    }
    return KP_OK;
}

// ---- the hit behind every kept record (kp_variants.hip: kp_launch_kept_locate) ----------------------------------------------------
// What the variant records and the aligned rows both start from: the kept rows laid out back to back (h_kept_off / d_kept_off) and,
// in d_var_src, the row of the finished hit table behind each -- enqueued once per reduction, by whichever of the two is asked for
// first, on the reduction's stream behind the kernels that finalised the kept list.  The caller has fetched the summaries.
static int ensure_kept_src(kp_ctx *ctx, kp_batch *b, KpWork *w, KpTypingRun &R) {
    if (R.src_valid) return KP_OK;
    const size_t n_asm = (size_t)b->n_asm;
    R.h_kept_off.assign(n_asm + 1, 0);
    for (size_t a = 0; a < n_asm; ++a) R.h_kept_off[a + 1] = R.h_kept_off[a] + std::min(std::max(R.h_sums[a].n_kept, 0), R.kept_cap);
    const int64_t total = R.h_kept_off[n_asm];
    if (total > 0) {
        KP_HIP_CHECK(ctx, R.d_var_src.reserve((size_t)total));
        if (int rc = upload(ctx, R.d_kept_off, R.h_kept_off.data(), n_asm + 1, R.stream)) return rc;
        kp_launch_kept_locate(b->view, w->hits(), w->hit_rows(), R.kept_rows(typing_group(ctx, b)->gene_lo), R.d_var_src.p, R.stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
    }
    R.src_valid = true;
    return KP_OK;
}

// ---- variant records of the kept hits (kp_variants.hip; kp_spec.h, VARIANTS) ------------------------------------------------------
static const char *const NO_VARIANTS = "this batch has no variant records (aligned without the variants option, or its hit table was replaced)";

// The records of the batch's current group, made on first request after its reduction: the hit behind every kept record located and
// its records counted, the counts scanned, the records stored -- on the reduction's stream, behind the kernels that finalised the
// kept list.  The buffer follows the policy of kp_caps.h; where it was too small only the storing kernel runs again: counts and
// offsets are exact whatever the buffer held.  No alignment pass, no reduction and no kp_batch_stats counter is touched.
static int ensure_variants(kp_ctx *ctx, kp_batch *b, KpTypingRun **R_out) {
    KpWork *w = finalised_work(ctx, b);
    if (!w) return KP_ESTATE;
    if (!w->var_on || !w->cigar_valid) return kp_fail(ctx, KP_EINVAL, NO_VARIANTS);
    KpTypingRun *Rp = reduced_run(ctx, b, &w);
    if (!Rp) return KP_ESTATE;
    KpTypingRun &R = *Rp;
    *R_out = Rp;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = fetch_summaries(ctx, b, w)) return rc;
    if (R.var_valid) return KP_OK;
    if (int rc = ensure_kept_src(ctx, b, w, R)) return rc;
    const int64_t total = R.h_kept_off.back();
    R.h_var_off.assign((size_t)total + 1, 0);
    R.var_total = 0;
    if (total > 0) {
        R.var_cap = kp_caps_variants_size(ctx->var_caps, (uint64_t)total);
        KP_HIP_CHECK(ctx, R.d_var_cnt.reserve((size_t)total));
        KP_HIP_CHECK(ctx, R.d_var_off.reserve((size_t)total + 1));
        KP_HIP_CHECK(ctx, R.d_var.reserve(R.var_cap));
        const KpTypingGroup &T = *typing_group(ctx, b);
        kp_launch_variants_walk(b->view, ctx->genes, w->cigars(), R.kept_rows(T.gene_lo), R.d_var_src.p, R.variants(), false, R.stream);
        for (int attempt = 0;; ++attempt) {
            kp_launch_variants_walk(b->view, ctx->genes, w->cigars(), R.kept_rows(T.gene_lo), R.d_var_src.p, R.variants(), true, R.stream);
            KP_HIP_CHECK(ctx, hipGetLastError());
            if (int frc = fetch_all(ctx, R.stream, {{R.h_var_off.data(), R.d_var_off.p, ((size_t)total + 1) * sizeof(int64_t)}})) return frc;
            R.var_total = R.h_var_off[(size_t)total];
            if (kp_caps_after_variants(ctx->var_caps, R.var_cap, (uint64_t)total, (uint64_t)R.var_total)) break;
            if (attempt >= 1) return kp_fail(ctx, KP_EOVERFLOW, "variant buffer overflowed repeatedly");
            KP_HIP_CHECK(ctx, R.d_var.reserve(R.var_cap));
        }
    }
    R.var_valid = true;
    return KP_OK;
}

int kp_batch_variant_offsets(kp_ctx *ctx, kp_batch *b, int64_t *var_off) {
    if (!ctx || !b || b->ctx != ctx || !var_off) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_variants(ctx, b, &R)) return rc;
    for (size_t a = 0; a < R->h_kept_off.size(); ++a) var_off[a] = R->h_var_off[(size_t)R->h_kept_off[a]];
    return KP_OK;
}

int kp_batch_variants(kp_ctx *ctx, kp_batch *b, kp_variant *out, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || (!out && cap > 0)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_variants(ctx, b, &R)) return rc;
    if (cap < R->var_total) return kp_fail(ctx, KP_EINVAL, "variant buffer too small");
    if (R->var_total > 0)
        if (int frc = fetch_all(ctx, R->stream, {{out, R->d_var.p, (size_t)R->var_total * sizeof(kp_variant)}})) return frc;
    return KP_OK;
}

// ---- aligned rows of the kept hits (kp_aligned.hip; kp_spec.h, ALIGNED ROWS) -------------------------------------------------------
static const char *const NO_ALIGNED = "this batch has no aligned rows (aligned without the aligned option, or its hit table was replaced)";

// The rows of the batch's current group, made on first request after its reduction: the hit behind every kept record located (unless
// the variant records already did), the blocks of every row counted and scanned, the total fetched and exactly that reserved, the
// rows stored and their records fetched -- on the reduction's stream, behind the kernels that finalised the kept list.  Sizes are
// exact before anything is stored: no guessed capacity, no overflow, no retry.
static int ensure_aligned(kp_ctx *ctx, kp_batch *b, KpTypingRun **R_out) {
    KpWork *w = work_of(b);
    if (!w || !w->finalised || !w->aln_on || !w->cigar_valid || !typing_group(ctx, b)) return kp_fail(ctx, KP_EINVAL, NO_ALIGNED);
    KpTypingRun &R = typing_run(w, b->group);
    if (!R.reduced) return kp_fail(ctx, KP_EINVAL, "this batch has no aligned rows: kp_batch_reduce has not run for this group since its hit table was made");
    *R_out = &R;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = fetch_summaries(ctx, b, w)) return rc;
    if (R.aln_valid) return KP_OK;
    if (int rc = ensure_kept_src(ctx, b, w, R)) return rc;
    const int64_t total = R.h_kept_off.back();
    R.h_aln_rows.assign((size_t)total, kp_aligned_row{0, 0, 0, 0, 0});
    R.aln_blocks = 0;
    if (total > 0) {
        KP_HIP_CHECK(ctx, R.d_aln_cnt.reserve((size_t)total));
        KP_HIP_CHECK(ctx, R.d_aln_off.reserve((size_t)total + 1));
        KP_HIP_CHECK(ctx, R.d_aln_rows.reserve((size_t)total));
        const KpKeptRows rows = R.kept_rows(typing_group(ctx, b)->gene_lo);
        kp_launch_aligned_count(b->view, ctx->genes, rows, R.d_aln_cnt.p, R.d_aln_off.p, R.stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
        int64_t n_blocks = 0;
        if (int frc = fetch_all(ctx, R.stream, {{&n_blocks, R.d_aln_off.p + total, sizeof(int64_t)}})) return frc;
        if (n_blocks < 0) return kp_fail(ctx, KP_EHIP, "aligned rows: bad block count");
        KP_HIP_CHECK(ctx, R.d_aln_blocks.reserve((size_t)std::max<int64_t>(n_blocks, 1)));
        kp_launch_aligned_emit(b->view, ctx->genes, w->hit_rows(), w->cigars(), rows, R.d_var_src.p, R.d_aln_off.p, R.d_aln_blocks.p, R.d_aln_rows.p, R.stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
        if (int frc = fetch_all(ctx, R.stream, {{R.h_aln_rows.data(), R.d_aln_rows.p, (size_t)total * sizeof(kp_aligned_row)}})) return frc;
        R.aln_blocks = n_blocks;
    }
    R.aln_valid = true;
    return KP_OK;
}

int kp_batch_aligned_size(kp_ctx *ctx, kp_batch *b, int64_t *n_blocks) {
    if (!ctx || !b || b->ctx != ctx || !n_blocks) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_aligned(ctx, b, &R)) return rc;
    *n_blocks = R->aln_blocks;
    return KP_OK;
}

int kp_batch_aligned_rows(kp_ctx *ctx, kp_batch *b, kp_aligned_row *rows, int32_t kept_stride) {
    if (!ctx || !b || b->ctx != ctx || kept_stride < 0 || (b->n_asm > 0 && !rows && kept_stride > 0)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_aligned(ctx, b, &R)) return rc;
    const size_t n_asm = (size_t)b->n_asm;
    const std::vector<int64_t> &kept_off = R->h_kept_off;
    for (size_t a = 0; a < n_asm; ++a)
        if (kept_off[a + 1] - kept_off[a] > kept_stride) return kp_fail(ctx, KP_EINVAL, "output strides too small (see kp_batch_typing_caps)");
    if (kept_stride > 0) std::memset(rows, 0, n_asm * (size_t)kept_stride * sizeof(kp_aligned_row));
    for (size_t a = 0; a < n_asm; ++a) std::copy(R->h_aln_rows.begin() + kept_off[a], R->h_aln_rows.begin() + kept_off[a + 1], rows + a * (size_t)kept_stride);
    return KP_OK;
}

int kp_batch_aligned_blocks(kp_ctx *ctx, kp_batch *b, uint64_t *out, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || (!out && cap > 0)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_aligned(ctx, b, &R)) return rc;
    if (cap < R->aln_blocks) return kp_fail(ctx, KP_EINVAL, "aligned block buffer too small");
    if (R->aln_blocks > 0)
        if (int frc = fetch_all(ctx, R->stream, {{out, R->d_aln_blocks.p, (size_t)R->aln_blocks * sizeof(uint64_t)}})) return frc;
    return KP_OK;
}

// ---- breakpoint records of the kept lists (kp_breakpoints.hip; kp_spec.h, BREAKPOINTS) --------------------------------------------
static const char *const NO_BREAKPOINTS = "this batch has no breakpoint records: kp_batch_reduce has not run for this group since its hit table was made";

// The records of the batch's current group, made on first request after its reduction (three kernels on the reduction's stream,
// behind the ones that finalised the kept list) once the summaries show that no reduction buffer overflowed.  They need the kept
// list and the batch's contigs only: no option, no ops -- a table that kp_batch_set_hits put in place serves as well.  The buffers
// hold a record per kept record, which is an upper bound: nothing can overflow, nothing is retried.
static int ensure_breakpoints(kp_ctx *ctx, kp_batch *b, KpTypingRun **R_out) {
    KpWork *w = work_of(b);
    if (!w || !w->finalised || !typing_group(ctx, b)) return kp_fail(ctx, KP_EINVAL, NO_BREAKPOINTS);
    KpTypingRun &R = typing_run(w, b->group);
    if (!R.reduced) return kp_fail(ctx, KP_EINVAL, NO_BREAKPOINTS);
    *R_out = &R;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = fetch_summaries(ctx, b, w)) return rc;
    if (R.bp_valid) return KP_OK;
    const size_t n_asm = (size_t)b->n_asm;
    R.h_bp_kept_off.assign(n_asm + 1, 0);
    for (size_t a = 0; a < n_asm; ++a) R.h_bp_kept_off[a + 1] = R.h_bp_kept_off[a] + std::min(std::max(R.h_sums[a].n_kept, 0), R.kept_cap);
    const int64_t total = R.h_bp_kept_off[n_asm];
    R.h_bp_off.assign(n_asm + 1, 0);
    if (total > 0) {
        KP_HIP_CHECK(ctx, R.d_bp_cnt.reserve(n_asm));
        KP_HIP_CHECK(ctx, R.d_bp_off.reserve(n_asm + 1));
        KP_HIP_CHECK(ctx, R.d_bp_tmp.reserve((size_t)total));
        KP_HIP_CHECK(ctx, R.d_bp.reserve((size_t)total));
        if (int rc = upload(ctx, R.d_bp_kept_off, R.h_bp_kept_off.data(), n_asm + 1, R.stream)) return rc;
        const KpKeptRows rows{.kept = R.d_kept.p, .kept_cap = R.kept_cap, .kept_off = R.d_bp_kept_off.p, .total = total, .gene_lo = typing_group(ctx, b)->gene_lo};
        kp_launch_breakpoints(b->view, rows, R.max_kept, R.d_bp_tmp.p, R.d_bp_cnt.p, R.d_bp_off.p, R.d_bp.p, R.stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
        if (int frc = fetch_all(ctx, R.stream, {{R.h_bp_off.data(), R.d_bp_off.p, (n_asm + 1) * sizeof(int64_t)}})) return frc;
    }
    R.bp_valid = true;
    return KP_OK;
}

int kp_batch_breakpoint_offsets(kp_ctx *ctx, kp_batch *b, int64_t *bp_off) {
    if (!ctx || !b || b->ctx != ctx || !bp_off) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_breakpoints(ctx, b, &R)) return rc;
    std::copy(R->h_bp_off.begin(), R->h_bp_off.end(), bp_off);
    return KP_OK;
}

int kp_batch_breakpoints(kp_ctx *ctx, kp_batch *b, kp_breakpoint *out, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || (!out && cap > 0)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_breakpoints(ctx, b, &R)) return rc;
    const int64_t total = R->h_bp_off.back();
    if (cap < total) return kp_fail(ctx, KP_EINVAL, "breakpoint buffer too small");
    if (total > 0)
        if (int frc = fetch_all(ctx, R->stream, {{out, R->d_bp.p, (size_t)total * sizeof(kp_breakpoint)}})) return frc;
    return KP_OK;
}

// ---- allele digests of the kept records and the pieces (kp_alleles.hip; kp_spec.h, ALLELES) ---------------------------------------
static const char *const NO_ALLELES = "this batch has no allele digests: kp_batch_reduce has not run for this group since its hit table was made";

// The digests of the batch's current group, made on first request after its reduction (one kernel on the reduction's stream, behind
// the ones that finalised the kept list) once the summaries show that no reduction buffer overflowed, and fetched: a record per kept
// row and per piece row, back to back.  They need the kept list, the pieces, the proteins and the batch's contigs only: no option,
// no ops -- a table that kp_batch_set_hits put in place serves as well.
static int ensure_alleles(kp_ctx *ctx, kp_batch *b, KpTypingRun **R_out) {
    KpWork *w = work_of(b);
    if (!w || !w->finalised || !typing_group(ctx, b)) return kp_fail(ctx, KP_EINVAL, NO_ALLELES);
    KpTypingRun &R = typing_run(w, b->group);
    if (!R.reduced) return kp_fail(ctx, KP_EINVAL, NO_ALLELES);
    *R_out = &R;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (int rc = fetch_summaries(ctx, b, w)) return rc;
    if (R.al_valid) return KP_OK;
    const size_t n_asm = (size_t)b->n_asm;
    R.h_al_off.assign(2 * (n_asm + 1), 0);
    int64_t *const kept_off = R.h_al_off.data(), *const piece_off = kept_off + n_asm + 1;
    for (size_t a = 0; a < n_asm; ++a) {
        kept_off[a + 1] = kept_off[a] + std::min(std::max(R.h_sums[a].n_kept, 0), R.kept_cap);
        piece_off[a + 1] = piece_off[a] + std::min(std::max(R.h_sums[a].n_pieces, 0), R.piece_cap);
    }
    const int64_t total = kept_off[n_asm], total_pieces = piece_off[n_asm];
    R.h_al.assign((size_t)total, kp_allele{0, 0});
    R.h_al_piece.assign((size_t)total_pieces, 0);
    if (total + total_pieces > 0) {
        KP_HIP_CHECK(ctx, R.d_al.reserve((size_t)std::max<int64_t>(total, 1)));
        KP_HIP_CHECK(ctx, R.d_al_piece.reserve((size_t)std::max<int64_t>(total_pieces, 1)));
        if (int rc = upload(ctx, R.d_al_off, R.h_al_off.data(), 2 * (n_asm + 1), R.stream)) return rc;
        const KpKeptRows rows{.kept = R.d_kept.p, .kept_cap = R.kept_cap, .kept_off = R.d_al_off.p, .total = total, .gene_lo = typing_group(ctx, b)->gene_lo};
        kp_launch_alleles(b->view, rows, R.d_pieces.p, R.piece_cap, R.d_al_off.p + n_asm + 1, total_pieces, R.d_prot.p, R.prot_cap, R.d_al.p, R.d_al_piece.p,
                          R.stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
        if (int frc = fetch_all(ctx, R.stream, {{R.h_al.data(), R.d_al.p, (size_t)total * sizeof(kp_allele)},
                                                {R.h_al_piece.data(), R.d_al_piece.p, (size_t)total_pieces * sizeof(uint64_t)}})) return frc;
    }
    R.al_valid = true;
    return KP_OK;
}

int kp_batch_alleles(kp_ctx *ctx, kp_batch *b, kp_allele *out, int32_t kept_stride, uint64_t *piece_out, int32_t piece_stride) {
    if (!ctx || !b || b->ctx != ctx || kept_stride < 0 || piece_stride < 0 || (b->n_asm > 0 && ((!out && kept_stride > 0) || (!piece_out && piece_stride > 0))))
        return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_alleles(ctx, b, &R)) return rc;
    const size_t n_asm = (size_t)b->n_asm;
    const int64_t *const kept_off = R->h_al_off.data(), *const piece_off = kept_off + n_asm + 1;
    for (size_t a = 0; a < n_asm; ++a)
        if (kept_off[a + 1] - kept_off[a] > kept_stride || piece_off[a + 1] - piece_off[a] > piece_stride)
            return kp_fail(ctx, KP_EINVAL, "output strides too small (see kp_batch_typing_caps)");
    if (kept_stride > 0) std::memset(out, 0, n_asm * (size_t)kept_stride * sizeof(kp_allele));
    if (piece_stride > 0) std::memset(piece_out, 0, n_asm * (size_t)piece_stride * sizeof(uint64_t));
    for (size_t a = 0; a < n_asm; ++a) {
        std::copy(R->h_al.begin() + kept_off[a], R->h_al.begin() + kept_off[a + 1], out + a * (size_t)kept_stride);
        std::copy(R->h_al_piece.begin() + piece_off[a], R->h_al_piece.begin() + piece_off[a + 1], piece_out + a * (size_t)piece_stride);
    }
    return KP_OK;
}

int kp_batch_typing_caps(kp_ctx *ctx, kp_batch *b, int32_t *kept_cap, int32_t *piece_cap) {
    if (!ctx || !b || b->ctx != ctx || !kept_cap || !piece_cap) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = nullptr;
    KpTypingRun *Rp = reduced_run(ctx, b, &w);
    if (!Rp) return KP_ESTATE;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    int rc = fetch_summaries(ctx, b, w);
    if (rc) return rc;
    *kept_cap = Rp->max_kept;
    *piece_cap = Rp->max_pieces;
    return KP_OK;
}

int kp_batch_proteins(kp_ctx *ctx, kp_batch *b, int32_t asm_index, uint8_t *out, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || asm_index < 0 || asm_index >= b->n_asm || (!out && cap > 0))
        return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = nullptr;
    KpTypingRun *Rp = reduced_run(ctx, b, &w);
    if (!Rp) return KP_ESTATE;
    KpTypingRun &R = *Rp;
    const int64_t n = std::min<int64_t>(cap, R.prot_cap);
    if (n > 0 && hipMemcpy(out, R.d_prot.p + (size_t)asm_index * (size_t)R.prot_cap, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
        return kp_fail(ctx, KP_EHIP, "D2H proteins failed");
    return (int)n;
}

static int protein_align(kp_ctx *ctx, const uint8_t *q, const int32_t *q_off, const int32_t *q_len, const uint8_t *t,
                         const int32_t *t_off, const int32_t *t_len, int32_t n, const int32_t *seed_off, int32_t seed_k,
                         int32_t *out8) {
    if (!ctx) return kp_fail(nullptr, KP_EINVAL, "null context");
    if (n < 0 || (n > 0 && (!q_off || !q_len || !t_off || !t_len || !out8))) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    if (n == 0) return KP_OK;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    size_t q_bytes = 0, t_bytes = 0;
    int max_t_len = 0;
    for (int i = 0; i < n; ++i) {
        if (q_len[i] < 0 || t_len[i] < 0 || q_off[i] < 0 || t_off[i] < 0 || q_len[i] > 65535 || t_len[i] > 65535)
            return kp_fail(ctx, KP_EINVAL, "protein lengths must be within [0, 65535]");
        q_bytes = std::max(q_bytes, (size_t)q_off[i] + (size_t)q_len[i]);
        t_bytes = std::max(t_bytes, (size_t)t_off[i] + (size_t)t_len[i]);
        max_t_len = std::max(max_t_len, t_len[i]);
    }
    if ((q_bytes && !q) || (t_bytes && !t)) return kp_fail(ctx, KP_EINVAL, "null sequence data");
    const int n_blocks = std::max(1, std::min(n, 256 * 16));
    const size_t scratch_per_block = (size_t)KP_PROT_ROWBUF_FIELDS * ((size_t)max_t_len + 1);  // see kp_prot.hip
    std::vector<int32_t> meta(5 * (size_t)n, 0);
    std::memcpy(meta.data(), q_off, (size_t)n * 4);
    std::memcpy(meta.data() + n, q_len, (size_t)n * 4);
    std::memcpy(meta.data() + 2 * (size_t)n, t_off, (size_t)n * 4);
    std::memcpy(meta.data() + 3 * (size_t)n, t_len, (size_t)n * 4);
    if (seed_off) std::memcpy(meta.data() + 4 * (size_t)n, seed_off, (size_t)n * 4);
    int rc;
    if ((rc = upload(ctx, ctx->d_pq, q, q_bytes)) || (rc = upload(ctx, ctx->d_pt, t, t_bytes)) || (rc = upload(ctx, ctx->d_pmeta, meta.data(), meta.size()))) return rc;
    KP_HIP_CHECK(ctx, ctx->d_pout.reserve(8 * (size_t)n));
    KP_HIP_CHECK(ctx, ctx->d_pscratch.reserve(scratch_per_block * (size_t)n_blocks + 64));
    kp_launch_protein(ctx->d_pq.p, ctx->d_pmeta.p, ctx->d_pmeta.p + n, ctx->d_pt.p, ctx->d_pmeta.p + 2 * (size_t)n,
                      ctx->d_pmeta.p + 3 * (size_t)n, n, nullptr, ctx->d_blosum.p, ctx->d_pout.p, ctx->d_pscratch.p,
                      scratch_per_block, n_blocks, ctx->stream, nullptr, nullptr, nullptr,
                      seed_off ? ctx->d_pmeta.p + 4 * (size_t)n : nullptr, seed_k);
    KP_HIP_CHECK(ctx, hipGetLastError());
    KP_HIP_CHECK(ctx, hipMemcpyAsync(out8, ctx->d_pout.p, 8 * (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return KP_OK;
}

int kp_protein_align(kp_ctx *ctx, const uint8_t *q, const int32_t *q_off, const int32_t *q_len, const uint8_t *t, const int32_t *t_off, const int32_t *t_len, int32_t n, int32_t *out8) {
    return protein_align(ctx, q, q_off, q_len, t, t_off, t_len, n, nullptr, 0, out8);
}

int kp_protein_align_seeded(kp_ctx *ctx, const uint8_t *q, const int32_t *q_off, const int32_t *q_len, const uint8_t *t,
                            const int32_t *t_off, const int32_t *t_len, int32_t n, const int32_t *diagonal_offsets,
                            int32_t k, int32_t *out8) {
    if (ctx && n > 0 && (!diagonal_offsets || k < 0 || k > KP_MAX_GENE_LEN)) return kp_fail(ctx, KP_EINVAL, "bad seed arguments");
    return protein_align(ctx, q, q_off, q_len, t, t_off, t_len, n, diagonal_offsets, k, out8);
}

}  // extern "C"
