// kp_db.hip -- the resident database of a context: seed index and packed genes (kp_db_load), typing tables of its groups.
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <thread>

#include "kp_host.h"
#include "kp_sketch.h"

struct HostPosting { uint32_t key, gene, pos, z; };  // a gene seed: x, gene, first base on the forward strand, strand bit

extern "C" {

int kp_db_load(kp_ctx *ctx, const uint8_t *gene_codes, const int32_t *gene_off, int32_t n_genes) {
    if (!ctx) return kp_fail(nullptr, KP_EINVAL, "null context");
    if (!gene_off || n_genes < 0 || (n_genes > 0 && !gene_codes)) return kp_fail(ctx, KP_EINVAL, "bad database arguments");
    if (n_genes > KP_MAX_GENES) return kp_fail(ctx, KP_EINVAL, "too many genes (KP_MAX_GENES)");
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    ctx->has_db = false;
    ctx->groups.clear();  // typing tables index the genes that are being replaced
    ctx->run_caps.clear();
    ctx->gene_len.resize((size_t)n_genes);
    std::vector<int32_t> nib_off(2 * (size_t)n_genes);
    size_t n_words = 0;
    for (int g = 0; g < n_genes; ++g) {
        const int len = gene_off[g + 1] - gene_off[g];
        if (len < 0 || len > KP_MAX_GENE_LEN) return kp_fail(ctx, KP_EINVAL, "gene length outside [0, KP_MAX_GENE_LEN]");
        ctx->gene_len[(size_t)g] = len;
        nib_off[(size_t)g] = (int32_t)n_words;
        n_words += (size_t)(len + 7) / 8;
    }
    for (int g = 0; g < n_genes; ++g) {
        nib_off[(size_t)n_genes + g] = (int32_t)n_words;
        n_words += (size_t)(ctx->gene_len[(size_t)g] + 7) / 8;
    }
    const bool load_timing = std::getenv("KAPTIVE_AMD_LOAD_TIMING") != nullptr;  // (a measurement aid of this call, no option)
    const auto t_load0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) { if (load_timing) std::fprintf(stderr, "[kp_db_load] %s at %.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_load0).count()); };
    std::vector<uint32_t> nib(std::max<size_t>(n_words, 1), 0x44444444u);
    std::vector<uint16_t> prof(8 * nib.size(), 0);  // eight rows per word of `nib`
    std::vector<uint8_t> has_n(std::max<size_t>((size_t)n_genes, 1), 0);
    // Packing, profiles and sketches gene by gene on a few threads (45 ms of a 120 ms load on one: a command that types one
    // genome spends a fifth of its 0.6 s here); every thread keeps the postings of its own genes, joined in gene order
    std::vector<HostPosting> post;
    {
        const int n_thr = std::max(1, std::min({4, (int)std::thread::hardware_concurrency(), n_genes / 256}));
        std::vector<std::vector<HostPosting>> part((size_t)n_thr);
        std::atomic<bool> failed{false};
        auto work = [&](int t) {
            try {
            const int g_lo = (int)((int64_t)n_genes * t / n_thr), g_hi = (int)((int64_t)n_genes * (t + 1) / n_thr);
            std::vector<uint8_t> rc;
            std::vector<HostPosting> &post = part[(size_t)t];
            for (int g = g_lo; g < g_hi; ++g) {
            const int len = ctx->gene_len[(size_t)g];
            const uint8_t *fwd = gene_codes + gene_off[g];
            rc.resize((size_t)len);
            for (int i = 0; i < len; ++i) {
                const uint8_t c = fwd[len - 1 - i];
                rc[(size_t)i] = c > 3 ? 4 : (uint8_t)(3 - c);
            }
            for (int s = 0; s < 2; ++s) {
                const uint8_t *c = s ? rc.data() : fwd;
                uint32_t *dst = nib.data() + nib_off[(size_t)(s ? n_genes + g : g)];
                for (int i = 0; i < len; ++i) {
                    const uint32_t code = c[i] > 3 ? 4u : c[i];
                    dst[i >> 3] = (dst[i >> 3] & ~(15u << (4 * (i & 7)))) | (code << (4 * (i & 7)));
                    prof[8 * (size_t)(dst - nib.data()) + (size_t)i] = (uint16_t)kp_row_profile(code);
                    if (code > 3u) has_n[(size_t)g] = 1;
                }
            }
            // the gene's seeds: minimap2 sketches a query on its forward strand (kp_spec.h; kp_sketch.h is the state machine)
            KpSketchState st;
            kp_sketch_reset(st);
            auto emit = [&](int64_t start, uint32_t z, uint32_t x) { post.push_back(HostPosting{x, (uint32_t)g, (uint32_t)start, z}); };
            for (int i = 0; i < len; ++i) kp_sketch_step(st, i, fwd[i], emit);
            if (len > 0) kp_sketch_final(st, len - 1, emit);
            }
            } catch (...) { failed.store(true); }  // (out of memory in a worker must not end the process)
        };
        // A thread that cannot be started (std::system_error under a thread limit, bad_alloc) must not let the exception
        // leave this extern "C" function past joinable threads (std::terminate): the calling thread takes the ranges that
        // got no thread of their own
        std::vector<std::thread> pool;
        int n_started = 1;
        try {
            pool.reserve((size_t)n_thr);
            for (; n_started < n_thr; ++n_started) pool.emplace_back(work, n_started);
        } catch (...) {
        }
        work(0);
        for (int t = n_started; t < n_thr; ++t) work(t);
        for (auto &th : pool) th.join();
        if (failed.load()) return kp_fail(ctx, KP_ENOMEM, "out of host memory while sketching the genes");
        size_t total = 0;
        for (const auto &v : part) total += v.size();
        post.reserve(total);
        for (const auto &v : part) post.insert(post.end(), v.begin(), v.end());
    }
    lap("genes packed and sketched");
    {   // by (key, gene, pos): three stable counting passes over the 30-bit key, then the few postings that share a key --
        // they arrive in gene order, positions nearly so -- put right by insertion (a comparison sort took 45 ms of the load)
        static_assert(KP_KMER_MASK < (1u << 30), "three passes of ten bits cover the key");
        std::vector<HostPosting> tmp(post.size());
        for (int pass = 0; pass < 3; ++pass) {
            const int sh = 10 * pass;
            size_t cnt[1025] = {0};
            for (const HostPosting &q : post) ++cnt[((q.key >> sh) & 1023u) + 1];
            for (int b = 0; b < 1024; ++b) cnt[b + 1] += cnt[b];
            for (const HostPosting &q : post) tmp[cnt[(q.key >> sh) & 1023u]++] = q;
            post.swap(tmp);
        }
        auto less = [](const HostPosting &a, const HostPosting &b) { return a.gene != b.gene ? a.gene < b.gene : a.pos < b.pos; };
        for (size_t i = 1; i < post.size(); ++i) {
            if (post[i].key != post[i - 1].key || !less(post[i], post[i - 1])) continue;
            const HostPosting q = post[i];
            size_t j = i;
            for (; j > 0 && post[j - 1].key == q.key && less(q, post[j - 1]); --j) post[j] = post[j - 1];
            post[j] = q;
        }
    }
    lap("postings sorted");
    size_t n_unique = 0;
    for (size_t i = 0; i < post.size(); ++i) n_unique += (i == 0 || post[i].key != post[i - 1].key);
    uint32_t log_slots = 10;
    while (((size_t)1 << log_slots) < 2 * n_unique + 1) ++log_slots;
    if (log_slots > 30) return kp_fail(ctx, KP_EINVAL, "seed index too large");
    const uint32_t n_slots = 1u << log_slots, mask = n_slots - 1, shift = 32 - log_slots;
    std::vector<uint2> slots(n_slots, make_uint2(0xFFFFFFFFu, 0u));
    std::vector<uint64_t> filter((size_t)1 << (KP_FILTER_LOG2 - 6), 0ull), filter2((size_t)1 << (KP_FILTER2_LOG2 - 6), 0ull);
    std::vector<uint64_t> flat;
    flat.reserve(2 * post.size() + n_unique + 1);
    for (size_t i = 0; i < post.size();) {
        size_t j = i;
        while (j < post.size() && post[j].key == post[i].key) ++j;
        uint32_t slot = (post[i].key * 2654435769u) >> shift;
        while (slots[slot].x != 0xFFFFFFFFu) slot = (slot + 1) & mask;
        slots[slot] = make_uint2(post[i].key, (uint32_t)flat.size());
        filter[kp_filter_block(post[i].key)] |= kp_filter_mask(post[i].key);
        {
            const uint2 m2 = kp_filter2_mask2(post[i].key);
            filter2[kp_filter2_block(post[i].key)] |= ((uint64_t)m2.y << 32) | m2.x;
        }
        flat.push_back((uint64_t)(j - i));
        for (uint32_t zt = 0; zt < 2; ++zt)  // the anchors a contig seed with strand bit zt makes with these gene seeds
            for (size_t x = i; x < j; ++x) {
                const uint32_t rev = post[x].z != zt ? 1u : 0u;
                const uint32_t qpos = rev ? (uint32_t)(ctx->gene_len[post[x].gene] - KP_K) - post[x].pos : post[x].pos;
                flat.push_back(((uint64_t)(2u * post[x].gene + rev) << 46) | ((uint64_t)(KP_DIAG_BIAS - qpos) << 16) | qpos);
            }
        i = j;
    }
    if (flat.size() > 0xFFFFFFFFull) return kp_fail(ctx, KP_EINVAL, "seed index too large");
    if (flat.empty()) flat.push_back(0);
    lap("table, filters and anchor lists built");
    int rcode;
    if ((rcode = upload(ctx, ctx->d_slots, slots.data(), slots.size())) || (rcode = upload(ctx, ctx->d_filter, filter.data(), filter.size())) ||
        (rcode = upload(ctx, ctx->d_filter2, filter2.data(), filter2.size())) || (rcode = upload(ctx, ctx->d_postings, flat.data(), flat.size())) ||
        (rcode = upload(ctx, ctx->d_nib, nib.data(), nib.size())) || (rcode = upload(ctx, ctx->d_nib_off, nib_off.data(), nib_off.size())) ||
        (rcode = upload(ctx, ctx->d_gene_prof, reinterpret_cast<const uint4 *>(prof.data()), nib.size())) || (rcode = upload(ctx, ctx->d_gene_has_n, has_n.data(), has_n.size())) ||
        (rcode = upload(ctx, ctx->d_gene_len, ctx->gene_len.data(), ctx->gene_len.size())))
        return rcode;
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    lap("uploaded");
    ctx->index = KpSeedIndex{ctx->d_filter.p, ctx->d_filter2.p, ctx->d_slots.p, ctx->d_postings.p, mask, shift};
    ctx->genes = KpGenes{ctx->d_nib.p, ctx->d_nib_off.p, ctx->d_gene_len.p, n_genes, ctx->d_gene_prof.p, ctx->d_gene_has_n.p};
    ctx->n_genes = n_genes;
    ctx->gs_bits = 1;
    while (ctx->gs_bits < 18 && (2ull * (uint64_t)n_genes) >> ctx->gs_bits) ++ctx->gs_bits;
    ctx->max_gene_len = 0;
    for (int len : ctx->gene_len) ctx->max_gene_len = std::max(ctx->max_gene_len, len);
    ctx->n_postings = (int64_t)post.size();
    ctx->has_db = true;
    return KP_OK;
}

int64_t kp_db_n_postings(const kp_ctx *ctx) { return ctx && ctx->has_db ? ctx->n_postings : 0; }

int kp_db_load_typing(kp_ctx *ctx, const kp_typing_tables *t) {
    if (!ctx) return kp_fail(nullptr, KP_EINVAL, "null context");
    return kp_db_load_typing_group(ctx, 0, 0, ctx->n_genes, t);
}

int kp_db_load_typing_group(kp_ctx *ctx, int32_t group, int32_t gene_lo, int32_t gene_hi, const kp_typing_tables *t) {
    if (!ctx) return kp_fail(nullptr, KP_EINVAL, "null context");
    if (!ctx->has_db) return kp_fail(ctx, KP_ESTATE, "kp_db_load must come first");
    if (group < 0 || group >= KP_MAX_TYPING_GROUPS || gene_lo < 0 || gene_hi < gene_lo || gene_hi > ctx->n_genes)
        return kp_fail(ctx, KP_EINVAL, "bad typing group or gene range");
    if (!t || t->n_loci <= 0 || !t->gene_locus || !t->gene_extra || !t->gene_pos || !t->gene_strand || !t->locus_gene_off || !t->locus_gene_len || !t->prot_off || !t->prot_len)
        return kp_fail(ctx, KP_EINVAL, "bad typing tables");
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    const size_t G = (size_t)(gene_hi - gene_lo), L = (size_t)t->n_loci;
    size_t prot_bytes = 0;
    int max_len = 0;
    for (size_t g = 0; g < G; ++g) {
        if (t->gene_locus[g] >= L) return kp_fail(ctx, KP_EINVAL, "gene_locus out of range");
        if (t->prot_len[g] < 0 || t->prot_off[g] < 0 || t->prot_len[g] > 65535) return kp_fail(ctx, KP_EINVAL, "bad protein table");
        prot_bytes = std::max(prot_bytes, (size_t)t->prot_off[g] + (size_t)t->prot_len[g]);
        max_len = std::max(max_len, t->prot_len[g]);
    }
    for (size_t l = 0; l < L; ++l)
    {
        if (t->locus_gene_off[l] < 0 || t->locus_gene_len[l] < 0 || (size_t)t->locus_gene_off[l] + (size_t)t->locus_gene_len[l] > G)
            return kp_fail(ctx, KP_EINVAL, "locus gene range out of bounds");
        if (t->locus_gene_len[l] > KP_MAX_LOCUS_GENES)
            return kp_fail(ctx, KP_EINVAL, "a locus has more genes than KP_MAX_LOCUS_GENES (width of the missing-gene mask)");
    }
    if (prot_bytes && !t->prot) return kp_fail(ctx, KP_EINVAL, "null protein data");
    if (ctx->groups.size() <= (size_t)group) ctx->groups.resize((size_t)group + 1);
    if (!ctx->groups[(size_t)group]) ctx->groups[(size_t)group].reset(new KpTypingGroup());
    KpTypingGroup &T = *ctx->groups[(size_t)group];
    int rc;
    if ((rc = upload(ctx, T.d_gene_locus, t->gene_locus, G)) || (rc = upload(ctx, T.d_gene_extra, t->gene_extra, G)) ||
        (rc = upload(ctx, T.d_gene_pos, t->gene_pos, G)) || (rc = upload(ctx, T.d_gene_strand, t->gene_strand, G)) ||
        (rc = upload(ctx, T.d_locus_off, t->locus_gene_off, L)) || (rc = upload(ctx, T.d_locus_len, t->locus_gene_len, L)) ||
        (rc = upload(ctx, T.d_prot_db, t->prot, prot_bytes)) || (rc = upload(ctx, T.d_prot_db_off, t->prot_off, G)) ||
        (rc = upload(ctx, T.d_prot_db_len, t->prot_len, G)))
        return rc;
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    T.typing = KpTypingDb{T.d_gene_locus.p, T.d_gene_extra.p, T.d_gene_pos.p, T.d_gene_strand.p, ctx->d_gene_len.p + gene_lo, T.d_locus_off.p, T.d_locus_len.p, T.d_prot_db.p,
                          T.d_prot_db_off.p, T.d_prot_db_len.p, (int32_t)G, (int32_t)t->n_loci};
    T.max_db_prot_len = max_len;
    T.gene_lo = gene_lo; T.gene_hi = gene_hi;
    return KP_OK;
}

}  // extern "C"
