// kp_batch.hip -- batch inputs: validation and staging of the tables, device copies recycled through the context, creation, destruction.
#include <new>

#include "kp_host.h"

static std::unique_ptr<KpInput> acquire_input(kp_ctx *ctx) {
    std::unique_ptr<KpInput> in;
    if (!ctx->free_inputs.empty()) {
        in = std::move(ctx->free_inputs.back());
        ctx->free_inputs.pop_back();
        return in;
    }
    in.reset(new (std::nothrow) KpInput());
    if (in && hipEventCreateWithFlags(&in->ready.h, hipEventDisableTiming) != hipSuccess) in.reset();
    return in;
}

// Validates the tables, stages them in the input's pinned buffer and enqueues their H2D copies on the copy stream (the
// caller's arrays may be freed as soon as this returns).
static int batch_tables(kp_ctx *ctx, kp_batch *b, int32_t n_asm, const int64_t *asm_word_off, const int32_t *ctg_start, const int32_t *ctg_len, const int32_t *asm_first_ctg, const int32_t *n_runs,
                 const int32_t *asm_first_nrun) {
    b->max_asm_bases = 0;
    for (int a = 0; a < n_asm; ++a) {
        const int64_t words = asm_word_off[a + 1] - asm_word_off[a];
        b->max_asm_bases = std::max<int64_t>(b->max_asm_bases, words * 16);
        if (words < 0 || (words * 16) % KP_ASM_ALIGN != 0 || (uint64_t)words * 16 > KP_MAX_ASM_LEN)
            return kp_fail(ctx, KP_EINVAL, "assembly length must be a multiple of KP_ASM_ALIGN and <= KP_MAX_ASM_LEN");
        if (asm_first_ctg[a + 1] < asm_first_ctg[a] || asm_first_nrun[a + 1] < asm_first_nrun[a])
            return kp_fail(ctx, KP_EINVAL, "offset tables must be non-decreasing");
        for (int c = asm_first_ctg[a]; c < asm_first_ctg[a + 1]; ++c) {
            if (ctg_start[c] % (int)KP_CONTIG_ALIGN != 0 || ctg_len[c] < 0 || (int64_t)ctg_start[c] + ctg_len[c] > words * 16 ||
                (c > asm_first_ctg[a] && ctg_start[c] < ctg_start[c - 1] + ctg_len[c - 1]))
                return kp_fail(ctx, KP_EINVAL, "contig table violates the packed layout (kp_spec.h)");
        }
    }
    KpInput &in = *b->in;
    const size_t n_ctg = (size_t)asm_first_ctg[n_asm], n_run = (size_t)asm_first_nrun[n_asm];
    const size_t na1 = (size_t)n_asm + 1;
    // staging layout: asm_word_off (8-byte entries first), then the int32 tables
    const size_t bytes = na1 * 8 + (2 * n_ctg + 2 * na1 + 2 * n_run) * 4;
    KP_HIP_CHECK(ctx, in.h_stage.reserve(bytes, bytes + bytes / 4 + 4096));
    uint8_t *p = in.h_stage.p;
    auto stage = [&](auto &buf, const auto *src, size_t n) -> int {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(src)>>;
        if (n) std::memcpy(p, src, n * sizeof(T));
        const int rc = upload(ctx, buf, reinterpret_cast<const T *>(p), n, ctx->copy);
        p += n * sizeof(T);
        return rc;
    };
    int rc;
    if ((rc = stage(in.d_asm_word_off, asm_word_off, na1)) || (rc = stage(in.d_ctg_start, ctg_start, n_ctg)) || (rc = stage(in.d_ctg_len, ctg_len, n_ctg)) ||
        (rc = stage(in.d_asm_first_ctg, asm_first_ctg, na1)) || (rc = stage(in.d_n_runs, n_runs, 2 * n_run)) || (rc = stage(in.d_asm_first_nrun, asm_first_nrun, na1)))
        return rc;
    b->view.words = b->d_words;
    b->view.asm_word_off = in.d_asm_word_off.p;
    b->view.ctg_start = in.d_ctg_start.p;
    b->view.ctg_len = in.d_ctg_len.p;
    b->view.asm_first_ctg = in.d_asm_first_ctg.p;
    b->view.n_runs = in.d_n_runs.p;
    b->view.asm_first_nrun = in.d_asm_first_nrun.p;
    b->view.n_asm = n_asm;
    b->view.total_words = asm_word_off[n_asm];
    b->n_ctg_total = (int32_t)n_ctg;
    KP_HIP_CHECK(ctx, hipEventRecord(in.ready, ctx->copy));
    return KP_OK;
}

// everything this batch enqueued has finished (its pass, its hit finalisation, its reductions)
static void quiesce_batch(kp_batch *b) {
    KpWork *w = b->last_w;
    if (!w) return;
    if (w->ev[KP_EV_END]) (void)hipEventSynchronize(w->ev[KP_EV_END]);  // end of the slot's most recent pass
    if (b->ctx) (void)hipStreamSynchronize(b->ctx->post);
    for (auto &r : w->runs)
        if (r && r->stream) { (void)hipStreamSynchronize(r->stream); if (r->aux) (void)hipStreamSynchronize(r->aux); }
}

static int batch_make(kp_ctx *ctx, int32_t n_asm, const uint32_t *words, bool words_on_device, const int64_t *asm_word_off,
               const int32_t *ctg_start, const int32_t *ctg_len, const int32_t *asm_first_ctg, const int32_t *n_runs,
               const int32_t *asm_first_nrun, kp_batch **out) {
    if (!ctx) return kp_fail(nullptr, KP_EINVAL, "null context");
    if (!out || n_asm < 0 || !asm_word_off) return kp_fail(ctx, KP_EINVAL, "bad batch arguments");
    *out = nullptr;
    if (asm_word_off[0] != 0) return kp_fail(ctx, KP_EINVAL, "asm_word_off[0] must be 0");
    if (!asm_first_ctg || !asm_first_nrun) return kp_fail(ctx, KP_EINVAL, "null offset table");
    if (asm_word_off[n_asm] > 0 && !words) return kp_fail(ctx, KP_EINVAL, "null words");
    if (words_on_device && ((uintptr_t)words & 15u) != 0) return kp_fail(ctx, KP_EINVAL, "device words must be 16-byte aligned");
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    kp_batch *b = new (std::nothrow) kp_batch();
    if (!b) return kp_fail(ctx, KP_ENOMEM, "out of host memory");
    b->ctx = ctx; b->n_asm = n_asm;
    b->in = acquire_input(ctx);
    if (!b->in) { delete b; return kp_fail(ctx, KP_ENOMEM, "out of memory (batch input)"); }
    ctx->batches.push_back(b);
    if (words_on_device) {
        b->d_words = words;
    } else {
        const size_t nw = (size_t)asm_word_off[n_asm];
        hipError_t e = b->in->d_words.reserve(std::max<size_t>(nw, 4));
        if (e != hipSuccess) { kp_batch_destroy(b); return kp_fail(ctx, KP_ENOMEM, std::string("hipMalloc(words): ") + hipGetErrorString(e)); }
        // (optionally in pieces -- `upload_piece_mb` --: tried so that result read-backs could slip in between them on the
        // copy engines; they did not, see Fetch)
        const size_t piece = (size_t)ctx->opt.upload_piece_mb << 18;  // words
        for (size_t at = 0; at < nw && e == hipSuccess; at += piece)
            e = hipMemcpyAsync(b->in->d_words.p + at, words + at, std::min(piece, nw - at) * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->copy);
        if (e != hipSuccess) { kp_batch_destroy(b); return kp_fail(ctx, KP_EHIP, std::string("H2D words: ") + hipGetErrorString(e)); }
        b->d_words = b->in->d_words.p;
    }
    const int rc = batch_tables(ctx, b, n_asm, asm_word_off, ctg_start, ctg_len, asm_first_ctg, n_runs, asm_first_nrun);
    if (rc) { const std::string msg = ctx->error; kp_batch_destroy(b); ctx->error = msg; return rc; }
    *out = b;
    return KP_OK;
}

extern "C" {

int kp_batch_create_async(kp_ctx *ctx, int32_t n_asm, const uint32_t *words, const int64_t *asm_word_off, const int32_t *ctg_start, const int32_t *ctg_len, const int32_t *asm_first_ctg,
                          const int32_t *n_runs, const int32_t *asm_first_nrun, kp_batch **out) {
    return batch_make(ctx, n_asm, words, false, asm_word_off, ctg_start, ctg_len, asm_first_ctg, n_runs, asm_first_nrun, out);
}

int kp_batch_create(kp_ctx *ctx, int32_t n_asm, const uint32_t *words, const int64_t *asm_word_off, const int32_t *ctg_start, const int32_t *ctg_len, const int32_t *asm_first_ctg,
                    const int32_t *n_runs, const int32_t *asm_first_nrun, kp_batch **out) {
    const int rc = batch_make(ctx, n_asm, words, false, asm_word_off, ctg_start, ctg_len, asm_first_ctg, n_runs, asm_first_nrun, out);
    if (rc) return rc;
    // the caller may free `words` on return
    if (hipStreamSynchronize(ctx->copy) != hipSuccess) {
        kp_batch_destroy(*out);
        *out = nullptr;
        return kp_fail(ctx, KP_EHIP, "H2D copy of the batch failed");
    }
    return KP_OK;
}

int kp_batch_create_device(kp_ctx *ctx, int32_t n_asm, const uint32_t *d_words, const int64_t *asm_word_off, const int32_t *ctg_start, const int32_t *ctg_len, const int32_t *asm_first_ctg,
                           const int32_t *n_runs, const int32_t *asm_first_nrun, kp_batch **out) {
    return batch_make(ctx, n_asm, d_words, true, asm_word_off, ctg_start, ctg_len, asm_first_ctg, n_runs, asm_first_nrun, out);
}

int kp_batch_depends_on(kp_ctx *ctx, kp_batch *b, kp_batch *other) {
    if (!ctx || !b || b->ctx != ctx || !other || !other->ctx) return kp_fail(ctx, KP_EINVAL, "bad arguments");
    if (other->ctx->device != ctx->device) return kp_fail(ctx, KP_EINVAL, "batches live on different devices");
    b->after = other;
    return KP_OK;
}

int kp_batch_upload_wait(kp_ctx *ctx, kp_batch *b) {
    if (!ctx || !b || b->ctx != ctx) return kp_fail(ctx, KP_EINVAL, "bad context/batch");
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KP_HIP_CHECK(ctx, hipEventSynchronize(b->in->ready));
    return KP_OK;
}

const void *kp_batch_device_words(const kp_batch *b) { return b ? (const void *)b->d_words : nullptr; }

void kp_batch_destroy(kp_batch *b) {
    if (!b) return;
    kp_ctx *ctx = b->ctx;
    if (ctx) {
        (void)hipSetDevice(ctx->device);
        if (b->in && b->in->ready.h) (void)hipEventSynchronize(b->in->ready);  // an upload still in flight
        quiesce_batch(b);
        if (b->w && b->w->owner == b) { b->w->owner = nullptr; b->w->aligned = false; b->w->finalised = false; }
        // the input goes back to the context's pool (past the pool's size it is freed with the batch)
        if (b->in && ctx->free_inputs.size() < KP_INPUT_POOL) ctx->free_inputs.push_back(std::move(b->in));
        ctx->batches.erase(std::remove(ctx->batches.begin(), ctx->batches.end(), b), ctx->batches.end());
    }
    delete b;
}

}  // extern "C"
