// kp_typing.hip -- batched typing (locus scores, the reduction of a batch's hits, gene states, the variant and breakpoint records, the allele
// digests and the aligned rows of the kept hits, the rescue records of the missing genes; per typing group), stand-alone protein aligner.
#include "kp_host.h"
#include "kp_rescue.h"

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
    R.invalidate_derived();  // (every report describes a kept list: the one that is about to be replaced)
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

// ---- reports derived from the kept list ("Reports derived from the kept list"; state: KpDerived, kp_host.h) ----------------
// What every entry point of a report answers once its own arguments have passed ("bad arguments", KP_EINVAL), checked in this order:
//                                        variants (_variant_offsets, _variants)  aligned (_size, _rows, _blocks)  breakpoints (_offsets, _breakpoints)  alleles
//   1 no work set (never aligned, or     KP_ESTATE, finalised_work's text        KP_EINVAL, NO_ALIGNED            KP_EINVAL, NO_BREAKPOINTS              KP_EINVAL, NO_ALLELES
//     displaced) / pass not waited for   (kp_align.hip), one per case
//   2 pass without the report's option   KP_EINVAL, NO_VARIANTS                  KP_EINVAL, NO_ALIGNED            (needs no option: a table that kp_batch_set_hits
//     (w->var_on / w->aln_on), or ops                                                                             put in place serves as well)
//     gone (!w->cigar_valid)
//   3 no typing group                    as 4 (such a run is never reduced)      KP_EINVAL, NO_ALIGNED            KP_EINVAL, NO_BREAKPOINTS              KP_EINVAL, NO_ALLELES
//   4 group's run not reduced since the  KP_ESTATE, "kp_batch_reduce has not     KP_EINVAL, ALIGNED_NOT_REDUCED   KP_EINVAL, NO_BREAKPOINTS              KP_EINVAL, NO_ALLELES
//     hit table was made                 been called"
// The variant records answer KP_ESTATE where a call is missing, as kp_batch_typing does; the later reports KP_EINVAL with their own text
// throughout.  kp_batch_set_hits clears cigar_valid and resets the runs: 2 for variants and aligned, 4 for the others.  The rescue
// records (further down) answer like the allele digests, with NO_RESCUE, and before anything else KP_EINVAL with the same text where the
// context's `rescue` option is off.  Then the device is
// made current and the summaries are fetched (the reduction run again where a buffer overflowed): their errors pass through.  `code`: that
// of 1 and 4; `no_records`: the text of 1-3 under KP_EINVAL; `not_reduced`: the text of 4; `option`: the flag of 2, or null.  The run: *R_out.
static const char *const NO_VARIANTS = "this batch has no variant records (aligned without the variants option, or its hit table was replaced)";
static const char *const NO_ALIGNED = "this batch has no aligned rows (aligned without the aligned option, or its hit table was replaced)";
static const char *const ALIGNED_NOT_REDUCED = "this batch has no aligned rows: kp_batch_reduce has not run for this group since its hit table was made";
static const char *const NO_BREAKPOINTS = "this batch has no breakpoint records: kp_batch_reduce has not run for this group since its hit table was made";
static const char *const NO_ALLELES = "this batch has no allele digests: kp_batch_reduce has not run for this group since its hit table was made";

static int report_run(kp_ctx *ctx, kp_batch *b, int code, const char *no_records, const char *not_reduced, bool KpWork::*option, KpWork **w_out, KpTypingRun **R_out) {
    if (!ctx || !b || b->ctx != ctx) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpWork *w = code == KP_ESTATE ? finalised_work(ctx, b) : work_of(b);
    if (!w) return code == KP_ESTATE ? KP_ESTATE : kp_fail(ctx, KP_EINVAL, no_records);
    if (!w->finalised || (option && (!(w->*option) || !w->cigar_valid))) return kp_fail(ctx, KP_EINVAL, no_records);
    if (code == KP_EINVAL && !typing_group(ctx, b)) return kp_fail(ctx, KP_EINVAL, no_records);
    KpTypingRun &R = typing_run(w, b->group);
    if (!R.reduced) return kp_fail(ctx, code, not_reduced);
    *w_out = w; *R_out = &R;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    return fetch_summaries(ctx, b, w);
}

// The rows of the reduction laid out back to back, from the summaries the caller has fetched and the caps of the reduction's last run: made
// and -- where there is a row -- uploaded once per reduction, for the report that asks first, on the reduction's stream.
static int ensure_layout(kp_ctx *ctx, KpTypingRun &R, size_t n_asm) {
    KpRowLayout &L = R.derived.layout;
    if (L.valid) return KP_OK;
    L.n_asm = n_asm;
    L.h_off.assign(2 * (n_asm + 1), 0);
    int64_t *const kept_off = L.h_off.data(), *const piece_off = kept_off + n_asm + 1;
    for (size_t a = 0; a < n_asm; ++a) {
        kept_off[a + 1] = kept_off[a] + std::min(std::max(R.h_sums[a].n_kept, 0), R.kept_cap);
        piece_off[a + 1] = piece_off[a] + std::min(std::max(R.h_sums[a].n_pieces, 0), R.piece_cap);
    }
    if (L.kept_total() + L.piece_total() > 0)
        if (int rc = upload(ctx, L.d_off, L.h_off.data(), L.h_off.size(), R.stream)) return rc;
    L.valid = true;
    return KP_OK;
}

// the hit behind every kept record (kp_variants.hip: kp_launch_kept_locate): what the variant records and the aligned rows both start
// from, enqueued once per reduction by whichever of the two is asked for first
static int ensure_kept_src(kp_ctx *ctx, kp_batch *b, KpWork *w, KpTypingRun &R) {
    if (int rc = ensure_layout(ctx, R, (size_t)b->n_asm)) return rc;
    KpKeptSrcState &S = R.derived.src;
    if (S.valid) return KP_OK;
    const int64_t total = R.derived.layout.kept_total();
    if (total > 0) {
        KP_HIP_CHECK(ctx, S.d_src.reserve((size_t)total));
        kp_launch_kept_locate(b->view, w->hits(), w->hit_rows(), R.kept_rows(typing_group(ctx, b)->gene_lo), S.d_src.p, R.stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
    }
    S.valid = true;
    return KP_OK;
}

// ---- variant records of the kept hits (kp_variants.hip; kp_spec.h, VARIANTS) ------------------------------------------------------
// The records of the batch's current group: the hit behind every kept record located and its records counted, the counts scanned, the
// records stored.  The buffer follows the policy of kp_caps.h; where it was too small only the storing kernel runs again: counts and
// offsets are exact whatever the buffer held.  No alignment pass, no reduction and no kp_batch_stats counter is touched.
static int ensure_variants(kp_ctx *ctx, kp_batch *b, KpTypingRun **R_out) {
    KpWork *w = nullptr;
    if (int rc = report_run(ctx, b, KP_ESTATE, NO_VARIANTS, "kp_batch_reduce has not been called", &KpWork::var_on, &w, R_out)) return rc;
    KpTypingRun &R = **R_out;
    KpVariantsState &V = R.derived.var;
    if (V.valid) return KP_OK;
    if (int rc = ensure_kept_src(ctx, b, w, R)) return rc;
    const int64_t total = R.derived.layout.kept_total();
    V.h_off.assign((size_t)total + 1, 0);
    V.total = 0;
    if (total > 0) {
        V.cap = kp_caps_variants_size(ctx->var_caps, (uint64_t)total);
        KP_HIP_CHECK(ctx, V.d_cnt.reserve((size_t)total));
        KP_HIP_CHECK(ctx, V.d_off.reserve((size_t)total + 1));
        KP_HIP_CHECK(ctx, V.d_rec.reserve(V.cap));
        const KpKeptRows rows = R.kept_rows(typing_group(ctx, b)->gene_lo);
        kp_launch_variants_walk(b->view, ctx->genes, w->cigars(), rows, R.derived.src.d_src.p, V.view(), false, R.stream);
        for (int attempt = 0;; ++attempt) {
            kp_launch_variants_walk(b->view, ctx->genes, w->cigars(), rows, R.derived.src.d_src.p, V.view(), true, R.stream);
            KP_HIP_CHECK(ctx, hipGetLastError());
            if (int frc = fetch_all(ctx, R.stream, {{V.h_off.data(), V.d_off.p, ((size_t)total + 1) * sizeof(int64_t)}})) return frc;
            V.total = V.h_off[(size_t)total];
            if (kp_caps_after_variants(ctx->var_caps, V.cap, (uint64_t)total, (uint64_t)V.total)) break;
            if (attempt >= 1) return kp_fail(ctx, KP_EOVERFLOW, "variant buffer overflowed repeatedly");
            KP_HIP_CHECK(ctx, V.d_rec.reserve(V.cap));
        }
    }
    V.valid = true;
    return KP_OK;
}

int kp_batch_variant_offsets(kp_ctx *ctx, kp_batch *b, int64_t *var_off) {
    if (!ctx || !b || b->ctx != ctx || !var_off) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_variants(ctx, b, &R)) return rc;
    const int64_t *const kept_off = R->derived.layout.kept_off();
    for (int a = 0; a <= b->n_asm; ++a) var_off[a] = R->derived.var.h_off[(size_t)kept_off[a]];
    return KP_OK;
}

int kp_batch_variants(kp_ctx *ctx, kp_batch *b, kp_variant *out, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || (!out && cap > 0)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_variants(ctx, b, &R)) return rc;
    const KpVariantsState &V = R->derived.var;
    if (cap < V.total) return kp_fail(ctx, KP_EINVAL, "variant buffer too small");
    if (V.total > 0)
        if (int frc = fetch_all(ctx, R->stream, {{out, V.d_rec.p, (size_t)V.total * sizeof(kp_variant)}})) return frc;
    return KP_OK;
}

// ---- aligned rows of the kept hits (kp_aligned.hip; kp_spec.h, ALIGNED ROWS) -------------------------------------------------------
// The rows of the batch's current group: the hit behind every kept record located (unless the variant records already did), the
// blocks of every row counted and scanned, the total fetched and exactly that reserved, the rows stored and their records fetched.
// Sizes are exact before anything is stored: no guessed capacity, no overflow, no retry.
static int ensure_aligned(kp_ctx *ctx, kp_batch *b, KpTypingRun **R_out) {
    KpWork *w = nullptr;
    if (int rc = report_run(ctx, b, KP_EINVAL, NO_ALIGNED, ALIGNED_NOT_REDUCED, &KpWork::aln_on, &w, R_out)) return rc;
    KpTypingRun &R = **R_out;
    KpAlignedState &A = R.derived.aln;
    if (A.valid) return KP_OK;
    if (int rc = ensure_kept_src(ctx, b, w, R)) return rc;
    const int64_t total = R.derived.layout.kept_total();
    A.h_rows.assign((size_t)total, kp_aligned_row{0, 0, 0, 0, 0});
    A.n_blocks = 0;
    if (total > 0) {
        KP_HIP_CHECK(ctx, A.d_cnt.reserve((size_t)total));
        KP_HIP_CHECK(ctx, A.d_off.reserve((size_t)total + 1));
        KP_HIP_CHECK(ctx, A.d_rows.reserve((size_t)total));
        const KpKeptRows rows = R.kept_rows(typing_group(ctx, b)->gene_lo);
        kp_launch_aligned_count(b->view, ctx->genes, rows, A.d_cnt.p, A.d_off.p, R.stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
        int64_t n_blocks = 0;
        if (int frc = fetch_all(ctx, R.stream, {{&n_blocks, A.d_off.p + total, sizeof(int64_t)}})) return frc;
        if (n_blocks < 0) return kp_fail(ctx, KP_EHIP, "aligned rows: bad block count");
        KP_HIP_CHECK(ctx, A.d_blocks.reserve((size_t)std::max<int64_t>(n_blocks, 1)));
        kp_launch_aligned_emit(b->view, ctx->genes, w->hit_rows(), w->cigars(), rows, R.derived.src.d_src.p, A.d_off.p, A.d_blocks.p, A.d_rows.p, R.stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
        if (int frc = fetch_all(ctx, R.stream, {{A.h_rows.data(), A.d_rows.p, (size_t)total * sizeof(kp_aligned_row)}})) return frc;
        A.n_blocks = n_blocks;
    }
    A.valid = true;
    return KP_OK;
}

int kp_batch_aligned_size(kp_ctx *ctx, kp_batch *b, int64_t *n_blocks) {
    if (!ctx || !b || b->ctx != ctx || !n_blocks) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_aligned(ctx, b, &R)) return rc;
    *n_blocks = R->derived.aln.n_blocks;
    return KP_OK;
}

int kp_batch_aligned_rows(kp_ctx *ctx, kp_batch *b, kp_aligned_row *rows, int32_t kept_stride) {
    if (!ctx || !b || b->ctx != ctx || kept_stride < 0 || (b->n_asm > 0 && !rows && kept_stride > 0)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_aligned(ctx, b, &R)) return rc;
    const size_t n_asm = (size_t)b->n_asm;
    const int64_t *const kept_off = R->derived.layout.kept_off();
    const std::vector<kp_aligned_row> &h_rows = R->derived.aln.h_rows;
    for (size_t a = 0; a < n_asm; ++a)
        if (kept_off[a + 1] - kept_off[a] > kept_stride) return kp_fail(ctx, KP_EINVAL, "output strides too small (see kp_batch_typing_caps)");
    if (kept_stride > 0) std::memset(rows, 0, n_asm * (size_t)kept_stride * sizeof(kp_aligned_row));
    for (size_t a = 0; a < n_asm; ++a) std::copy(h_rows.begin() + kept_off[a], h_rows.begin() + kept_off[a + 1], rows + a * (size_t)kept_stride);
    return KP_OK;
}

int kp_batch_aligned_blocks(kp_ctx *ctx, kp_batch *b, uint64_t *out, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || (!out && cap > 0)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_aligned(ctx, b, &R)) return rc;
    const KpAlignedState &A = R->derived.aln;
    if (cap < A.n_blocks) return kp_fail(ctx, KP_EINVAL, "aligned block buffer too small");
    if (A.n_blocks > 0)
        if (int frc = fetch_all(ctx, R->stream, {{out, A.d_blocks.p, (size_t)A.n_blocks * sizeof(uint64_t)}})) return frc;
    return KP_OK;
}

// ---- breakpoint records of the kept lists (kp_breakpoints.hip; kp_spec.h, BREAKPOINTS) --------------------------------------------
// The records of the batch's current group: three kernels.  They need the kept list and the batch's contigs only.  The buffers hold a
// record per kept record, which is an upper bound: nothing can overflow, nothing is retried.
static int ensure_breakpoints(kp_ctx *ctx, kp_batch *b, KpTypingRun **R_out) {
    KpWork *w = nullptr;
    if (int rc = report_run(ctx, b, KP_EINVAL, NO_BREAKPOINTS, NO_BREAKPOINTS, nullptr, &w, R_out)) return rc;
    KpTypingRun &R = **R_out;
    KpBreakpointsState &B = R.derived.bp;
    if (B.valid) return KP_OK;
    const size_t n_asm = (size_t)b->n_asm;
    if (int rc = ensure_layout(ctx, R, n_asm)) return rc;
    const int64_t total = R.derived.layout.kept_total();
    B.h_off.assign(n_asm + 1, 0);
    if (total > 0) {
        KP_HIP_CHECK(ctx, B.d_cnt.reserve(n_asm));
        KP_HIP_CHECK(ctx, B.d_off.reserve(n_asm + 1));
        KP_HIP_CHECK(ctx, B.d_tmp.reserve((size_t)total));
        KP_HIP_CHECK(ctx, B.d_rec.reserve((size_t)total));
        kp_launch_breakpoints(b->view, R.kept_rows(typing_group(ctx, b)->gene_lo), R.max_kept, B.d_tmp.p, B.d_cnt.p, B.d_off.p, B.d_rec.p, R.stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
        if (int frc = fetch_all(ctx, R.stream, {{B.h_off.data(), B.d_off.p, (n_asm + 1) * sizeof(int64_t)}})) return frc;
    }
    B.valid = true;
    return KP_OK;
}

int kp_batch_breakpoint_offsets(kp_ctx *ctx, kp_batch *b, int64_t *bp_off) {
    if (!ctx || !b || b->ctx != ctx || !bp_off) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_breakpoints(ctx, b, &R)) return rc;
    std::copy(R->derived.bp.h_off.begin(), R->derived.bp.h_off.end(), bp_off);
    return KP_OK;
}

int kp_batch_breakpoints(kp_ctx *ctx, kp_batch *b, kp_breakpoint *out, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || (!out && cap > 0)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_breakpoints(ctx, b, &R)) return rc;
    const int64_t total = R->derived.bp.h_off.back();
    if (cap < total) return kp_fail(ctx, KP_EINVAL, "breakpoint buffer too small");
    if (total > 0)
        if (int frc = fetch_all(ctx, R->stream, {{out, R->derived.bp.d_rec.p, (size_t)total * sizeof(kp_breakpoint)}})) return frc;
    return KP_OK;
}

// ---- allele digests of the kept records and the pieces (kp_alleles.hip; kp_spec.h, ALLELES) ---------------------------------------
// The digests of the batch's current group, one kernel, and fetched: a record per kept row and per piece row, back to back.  They need
// the kept list, the pieces, the proteins and the batch's contigs only.
static int ensure_alleles(kp_ctx *ctx, kp_batch *b, KpTypingRun **R_out) {
    KpWork *w = nullptr;
    if (int rc = report_run(ctx, b, KP_EINVAL, NO_ALLELES, NO_ALLELES, nullptr, &w, R_out)) return rc;
    KpTypingRun &R = **R_out;
    KpAllelesState &A = R.derived.al;
    if (A.valid) return KP_OK;
    if (int rc = ensure_layout(ctx, R, (size_t)b->n_asm)) return rc;
    const int64_t total = R.derived.layout.kept_total(), total_pieces = R.derived.layout.piece_total();
    A.h_rec.assign((size_t)total, kp_allele{0, 0});
    A.h_piece.assign((size_t)total_pieces, 0);
    if (total + total_pieces > 0) {
        KP_HIP_CHECK(ctx, A.d_rec.reserve((size_t)std::max<int64_t>(total, 1)));
        KP_HIP_CHECK(ctx, A.d_piece.reserve((size_t)std::max<int64_t>(total_pieces, 1)));
        kp_launch_alleles(b->view, R.kept_rows(typing_group(ctx, b)->gene_lo), R.piece_rows(), R.d_prot.p, R.prot_cap, A.d_rec.p, A.d_piece.p, R.stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
        if (int frc = fetch_all(ctx, R.stream, {{A.h_rec.data(), A.d_rec.p, (size_t)total * sizeof(kp_allele)},
                                                {A.h_piece.data(), A.d_piece.p, (size_t)total_pieces * sizeof(uint64_t)}})) return frc;
    }
    A.valid = true;
    return KP_OK;
}

int kp_batch_alleles(kp_ctx *ctx, kp_batch *b, kp_allele *out, int32_t kept_stride, uint64_t *piece_out, int32_t piece_stride) {
    if (!ctx || !b || b->ctx != ctx || kept_stride < 0 || piece_stride < 0 || (b->n_asm > 0 && ((!out && kept_stride > 0) || (!piece_out && piece_stride > 0))))
        return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_alleles(ctx, b, &R)) return rc;
    const size_t n_asm = (size_t)b->n_asm;
    const int64_t *const kept_off = R->derived.layout.kept_off(), *const piece_off = R->derived.layout.piece_off();
    const KpAllelesState &A = R->derived.al;
    for (size_t a = 0; a < n_asm; ++a)
        if (kept_off[a + 1] - kept_off[a] > kept_stride || piece_off[a + 1] - piece_off[a] > piece_stride)
            return kp_fail(ctx, KP_EINVAL, "output strides too small (see kp_batch_typing_caps)");
    if (kept_stride > 0) std::memset(out, 0, n_asm * (size_t)kept_stride * sizeof(kp_allele));
    if (piece_stride > 0) std::memset(piece_out, 0, n_asm * (size_t)piece_stride * sizeof(uint64_t));
    for (size_t a = 0; a < n_asm; ++a) {
        std::copy(A.h_rec.begin() + kept_off[a], A.h_rec.begin() + kept_off[a + 1], out + a * (size_t)kept_stride);
        std::copy(A.h_piece.begin() + piece_off[a], A.h_piece.begin() + piece_off[a + 1], piece_out + a * (size_t)piece_stride);
    }
    return KP_OK;
}

// ---- rescue records of the missing genes (kp_rescue.hip; kp_spec.h, RESCUE) ---------------------------------------------------------
// The records of the batch's current group: one per set bit of the summaries' missing masks, laid out here from the summaries the
// report has fetched; the plan, the score-only fill over every frame, the pick and the winners' fill with path statistics follow on
// the reduction's stream.  They need the summaries, the pieces, the batch's contigs and the database's proteins only.  The one
// buffer whose size the host cannot know -- the strips' boundary column, for proteins beyond 384 residues -- is sized from the
// longest such frame text, which the plan leaves and one read-back fetches (only where the database has such a protein).
static const char *const NO_RESCUE = "this batch has no rescue records: the rescue option is off, or kp_batch_reduce has not run for this group since its hit table was made";

static int ensure_rescue(kp_ctx *ctx, kp_batch *b, KpTypingRun **R_out) {
    if (!ctx || !b || b->ctx != ctx) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    if (!ctx->opt.rescue) return kp_fail(ctx, KP_EINVAL, NO_RESCUE);
    KpWork *w = nullptr;
    if (int rc = report_run(ctx, b, KP_EINVAL, NO_RESCUE, NO_RESCUE, nullptr, &w, R_out)) return rc;
    KpTypingRun &R = **R_out;
    KpRescueState &S = R.derived.rs;
    const int32_t flank = ctx->opt.rescue_flank;
    if (S.valid && S.flank == flank) return KP_OK;
    const size_t n_asm = (size_t)b->n_asm;
    if (int rc = ensure_layout(ctx, R, n_asm)) return rc;
    const KpTypingGroup &T = *typing_group(ctx, b);
    S.valid = false;
    S.h_off.assign(2 * (n_asm + 1), 0);
    int64_t *const rec_off = S.h_off.data(), *const unit_off = rec_off + n_asm + 1;
    const int64_t *const piece_off = R.derived.layout.piece_off();
    for (size_t a = 0; a < n_asm; ++a) {
        int n = 0;
        if (!(R.h_sums[a].overflow & 4))
            for (int x = 0; x < KP_MAX_LOCUS_GENES / 64; ++x) n += __builtin_popcountll(R.h_sums[a].missing_mask[x]);
        rec_off[a + 1] = rec_off[a] + n;
        unit_off[a + 1] = unit_off[a] + (int64_t)n * (piece_off[a + 1] - piece_off[a]);
    }
    const int64_t n_rec = rec_off[n_asm], n_units = unit_off[n_asm];
    if (n_units > 0x7FFFFFFFll / (4 * KP_RS_FRAMES)) return kp_fail(ctx, KP_EOVERFLOW, "too many missing genes and locus pieces for one rescue pass; use smaller batches");
    S.h_rec.assign((size_t)n_rec, kp_rescue{});
    if (n_rec > 0) {
        if (int rc = upload(ctx, S.d_off, S.h_off.data(), S.h_off.size(), R.stream)) return rc;
        KP_HIP_CHECK(ctx, S.d_rec.reserve((size_t)n_rec));
        KP_HIP_CHECK(ctx, S.d_sub.reserve(4 * (size_t)n_rec));
        KP_HIP_CHECK(ctx, S.d_units.reserve((size_t)std::max<int64_t>(n_units, 1)));
        KP_HIP_CHECK(ctx, S.d_cell.reserve(4 * (size_t)KP_RS_FRAMES * (size_t)std::max<int64_t>(n_units, 1)));
        KP_HIP_CHECK(ctx, S.d_ctl.reserve(KP_RS_CTL_WORDS));
        KP_HIP_CHECK(ctx, hipMemsetAsync(S.d_ctl.p, 0, KP_RS_CTL_WORDS * sizeof(int32_t), R.stream));
        KpRescueTables t{.rec_off = S.d_off.p, .unit_off = S.d_off.p + n_asm + 1, .n_rec = n_rec, .n_units = n_units, .units = S.d_units.p,
                         .cell = S.d_cell.p, .sub = S.d_sub.p, .ctl = S.d_ctl.p, .rec = S.d_rec.p, .scratch = nullptr, .scratch_per_block = 0};
        kp_launch_rescue_plan(b->view, T.typing, R.d_summary.p, R.d_pieces.p, R.piece_cap, flank, t, R.stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
        int n_blocks = 4096;  // one wave each; the waves take the tasks off a counter
        if (n_units > 0 && kp_rs_needs_strips(T.max_db_prot_len)) {
            int32_t rows = 0;
            if (int frc = fetch_all(ctx, R.stream, {{&rows, S.d_ctl.p + KP_RS_CTL_ROWS, sizeof(int32_t)}})) return frc;
            if (rows > 0) {
                n_blocks = 512;  // (a boundary column per block: 24 bytes a row)
                t.scratch_per_block = (size_t)KP_RS_SCRATCH_FIELDS * ((size_t)rows + 1);
                KP_HIP_CHECK(ctx, S.d_scratch.reserve(t.scratch_per_block * (size_t)n_blocks));
                t.scratch = S.d_scratch.p;
            }
        }
        kp_launch_rescue_fill(b->view, T.typing, ctx->d_blosum.p, R.prm.edge_tolerance, t, n_blocks, R.stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
        if (int frc = fetch_all(ctx, R.stream, {{S.h_rec.data(), S.d_rec.p, (size_t)n_rec * sizeof(kp_rescue)}})) return frc;
    }
    S.flank = flank;
    S.valid = true;
    return KP_OK;
}

int kp_batch_rescue_offsets(kp_ctx *ctx, kp_batch *b, int64_t *rescue_off) {
    if (!ctx || !b || b->ctx != ctx || !rescue_off) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_rescue(ctx, b, &R)) return rc;
    std::copy(R->derived.rs.h_off.begin(), R->derived.rs.h_off.begin() + b->n_asm + 1, rescue_off);
    return KP_OK;
}

int kp_batch_rescue(kp_ctx *ctx, kp_batch *b, kp_rescue *out, int64_t cap) {
    if (!ctx || !b || b->ctx != ctx || (!out && cap > 0)) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    KpTypingRun *R = nullptr;
    if (int rc = ensure_rescue(ctx, b, &R)) return rc;
    const std::vector<kp_rescue> &rec = R->derived.rs.h_rec;
    if (cap < (int64_t)rec.size()) return kp_fail(ctx, KP_EINVAL, "rescue buffer too small");
    std::copy(rec.begin(), rec.end(), out);
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
