// kp_dist_pars.hip -- small parsimony of every column of a distance handle's matrix on a neighbour-joining tree (kp_spec.h, PARSIMONY;
// the arithmetic: kp_pars.h).  The handle and its planes: kp_dist_handle.h; the taxa are numbered as kp_dist_nj numbers them
// (dist_nj_taxa).  No pair is looked at here.
//
//   kp_pars_pass_kernel    a lane per plane word w (64 columns), one wave a workgroup.  UP: the lane walks the records in order; a
//                          child's set is the leaf set made of the three plane words of the taxon's row, or the four words the lane
//                          stored for an inner node; the node's set goes to the node table [node][plane][word], word fastest, so a
//                          wave's loads and stores are contiguous runs.  The step masks are added into bit-sliced counters in the
//                          lane (KpParsCounter), the bases the leaves hold are collected in four words.  DOWN: records descending;
//                          the top node's state is the smallest code of its set, a child's state follows kp_pars_child, and the
//                          child's state planes and change mask overwrite the first three planes of its set, which nobody needs
//                          again.  A LANE READS ONLY WORDS OF THE NODE TABLE IT STORED ITSELF, in its own column of words: program
//                          order is all the ordering there is -- no barrier, no atomic, no LDS, no grid-wide step.  The records
//                          are the same for every lane: scalar loads.
//   kp_pars_site_kernel    a lane per column of [0, 16 NB).  COUNT: steps >= 1 as 0 / 1 -> flag[c], whose exclusive scan
//                          (kp_launch_count_scan) is every site's place.  FILL: the records.
//   kp_pars_change_kernel  a lane per (branch, plane word), the branch named by its child end.  COUNT: the popcount of the change
//                          mask -> cnt[e]; the scan places them.  FILL: the set bits expanded into records, ascending (node, column).
//
// Bounds: taxa [k < n], its values rows < R (the numbering kernel stores rows only); planes at w < NW and those rows; rec [t <
// n_rec], its ids checked on the host (kp_pars_tree_ok) to be nodes made before their record; the node table holds
// kp_pars_node_planes(n + n_rec, n) * NW words, node v's at kp_pars_node_planes(v, n) * NW + plane * NW + w, plane < 3 for a leaf and
// < 4 for an inner node; steps [b < 14][w < NW], alleles [k < 4][w < NW]; flag, off [c < 16 NB (+ 1)], a site record only below
// n_out; cnt, off [e < (n + n_rec - 1) * NW (+ 1)], parent [v < n + n_rec], a change record only below n_out.
#include <vector>

#include "kp_dist_handle.h"
#include "kp_pars.h"

namespace {

constexpr int PARS_THREADS = 64;  // one wave a workgroup: a lane's walk is latency, and few lanes should spread over many units

// the words of one set of the node table
__device__ __forceinline__ KpParsSet pars_load(const uint64_t *at, int64_t NW) { return KpParsSet{{at[0], at[NW], at[2 * NW], at[3 * NW]}}; }

__global__ __launch_bounds__(PARS_THREADS) void kp_pars_pass_kernel(const uint64_t *__restrict__ planes, int32_t R, int64_t NW, const int32_t *__restrict__ taxa,
                                                                    const kp_nj_node *__restrict__ rec, int32_t n, int32_t n_rec, uint64_t *tab,
                                                                    uint64_t *__restrict__ steps_out, uint64_t *__restrict__ alleles_out) {
    const int64_t w = (int64_t)blockIdx.x * PARS_THREADS + threadIdx.x;
    if (w >= NW) return;
    const size_t plane = (size_t)NW * (size_t)R;
    const uint64_t *__restrict__ mine = planes + (size_t)w * (size_t)R;
    uint64_t *col = tab + w;  // the lane's own column of words
    uint64_t held[4] = {0, 0, 0, 0};
    // a child's set on the way up; a leaf's bases are collected once, here: every taxon is a child exactly once
    const auto child_set = [&](int32_t v, bool collect) {
        if (v < n) {
            const int32_t row = taxa[v];
            const uint64_t valid = mine[2 * plane + row];
            const KpParsSet bases = kp_pars_bases(mine[row], mine[plane + row], valid);
            if (collect)
#pragma unroll
                for (int k = 0; k < 4; ++k) held[k] |= bases.s[k];
            return kp_pars_leaf(bases, valid);
        }
        return pars_load(col + (size_t)kp_pars_node_planes(v, n) * (size_t)NW, NW);
    };
    // ---- up
    KpParsCounter steps;
#pragma unroll
    for (int b = 0; b < KP_PARS_STEP_PLANES; ++b) steps.p[b] = 0;
    for (int32_t t = 0; t < n_rec; ++t) {
        const kp_nj_node r = rec[t];
        const KpParsSet x = child_set(r.a, true), y = child_set(r.b, true);
        uint64_t s1 = 0, s2 = 0;
        const KpParsSet q = r.c >= 0 ? kp_pars_join3(x, y, child_set(r.c, true), &s1, &s2) : kp_pars_join2(x, y, &s1);
        uint64_t *at = col + (size_t)kp_pars_node_planes(n + t, n) * (size_t)NW;
#pragma unroll
        for (int k = 0; k < 4; ++k) at[(size_t)k * (size_t)NW] = q.s[k];
        kp_pars_counter_add(&steps, s1);
        if (r.c >= 0) kp_pars_counter_add(&steps, s2);  // (uniform: the record is every lane's)
    }
#pragma unroll
    for (int b = 0; b < KP_PARS_STEP_PLANES; ++b) steps_out[(size_t)b * (size_t)NW + (size_t)w] = steps.p[b];
#pragma unroll
    for (int k = 0; k < 4; ++k) alleles_out[(size_t)k * (size_t)NW + (size_t)w] = held[k];
    // ---- down
    {
        uint64_t *top = col + (size_t)kp_pars_node_planes(n + n_rec - 1, n) * (size_t)NW;
        const KpParsState s = kp_pars_pick(pars_load(top, NW));
        top[(size_t)KP_PARS_PLANE_LO * (size_t)NW] = s.lo;
        top[(size_t)KP_PARS_PLANE_HI * (size_t)NW] = s.hi;
        top[(size_t)KP_PARS_PLANE_CHANGE * (size_t)NW] = 0ull;
    }
    for (int32_t t = n_rec - 1; t >= 0; --t) {
        const kp_nj_node r = rec[t];
        const uint64_t *up = col + (size_t)kp_pars_node_planes(n + t, n) * (size_t)NW;
        const KpParsState parent{up[(size_t)KP_PARS_PLANE_LO * (size_t)NW], up[(size_t)KP_PARS_PLANE_HI * (size_t)NW]};
        for (int k = 0; k < kp_pars_children(r); ++k) {
            const int32_t v = kp_pars_child_id(r, k);
            const KpParsSet q = child_set(v, false);  // (all four words are read before the first store below)
            uint64_t change;
            const KpParsState s = kp_pars_child(q, parent, &change);
            uint64_t *at = col + (size_t)kp_pars_node_planes(v, n) * (size_t)NW;
            at[(size_t)KP_PARS_PLANE_LO * (size_t)NW] = s.lo;
            at[(size_t)KP_PARS_PLANE_HI * (size_t)NW] = s.hi;
            at[(size_t)KP_PARS_PLANE_CHANGE * (size_t)NW] = change;
        }
    }
}

// One lane per column of [0, n_cols = 16 NB).  COUNT: flag[c] = the column has a step.  FILL: its record at off[c].
template <bool FILL>
__global__ __launch_bounds__(DIST_THREADS) void kp_pars_site_kernel(const uint64_t *__restrict__ steps, const uint64_t *__restrict__ alleles, int64_t NW, int64_t n_cols,
                                                                    uint32_t *__restrict__ flag, const int64_t *__restrict__ off, kp_pars_site *__restrict__ out, int64_t n_out) {
    for (int64_t c = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; c < n_cols; c += (int64_t)gridDim.x * DIST_THREADS) {
        const int64_t w = c >> 6;
        const int j = (int)(c & 63);
        int32_t s = 0;
#pragma unroll
        for (int b = 0; b < KP_PARS_STEP_PLANES; ++b) s |= (int32_t)((steps[(size_t)b * (size_t)NW + (size_t)w] >> j) & 1ull) << b;
        if (!FILL) flag[c] = s >= 1 ? 1u : 0u;
        if (FILL && s >= 1) {
            int32_t a = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) a |= (int32_t)((alleles[(size_t)k * (size_t)NW + (size_t)w] >> j) & 1ull) << k;
            const int64_t at = off[c];
            if (at >= 0 && at < n_out) kp_pars_site_store(out + at, (int32_t)c, s, a);
        }
    }
}

// One lane per e = (node v, plane word w), v < n_nodes - 1: every node but the top is the child end of one branch.  COUNT: cnt[e] =
// the changes of the branch in the word.  FILL: their records from off[e] on, ascending in column.
template <bool FILL>
__global__ __launch_bounds__(DIST_THREADS) void kp_pars_change_kernel(const uint64_t *__restrict__ tab, const int32_t *__restrict__ parent, int32_t n, int64_t NW, int64_t n_entries,
                                                                      uint32_t *__restrict__ cnt, const int64_t *__restrict__ off, kp_pars_change *__restrict__ out,
                                                                      int64_t n_out) {
    for (int64_t e = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; e < n_entries; e += (int64_t)gridDim.x * DIST_THREADS) {
        const int64_t v = e / NW, w = e - v * NW;
        const uint64_t *mine = tab + (size_t)kp_pars_node_planes(v, n) * (size_t)NW + (size_t)w;
        uint64_t m = mine[(size_t)KP_PARS_PLANE_CHANGE * (size_t)NW];
        if (!FILL) { cnt[e] = (uint32_t)__popcll(m); continue; }
        if (!m) continue;
        const int32_t p = parent[v];
        const uint64_t *up = tab + (size_t)kp_pars_node_planes(p, n) * (size_t)NW + (size_t)w;
        const KpParsState to{mine[(size_t)KP_PARS_PLANE_LO * (size_t)NW], mine[(size_t)KP_PARS_PLANE_HI * (size_t)NW]};
        const KpParsState from{up[(size_t)KP_PARS_PLANE_LO * (size_t)NW], up[(size_t)KP_PARS_PLANE_HI * (size_t)NW]};
        for (int64_t at = off[e]; m; m &= m - 1, ++at) {
            const int j = __ffsll((unsigned long long)m) - 1;
            if (at >= 0 && at < n_out) kp_pars_change_store(out + at, (int32_t)(64 * w + j), (int32_t)v, p, kp_pars_state_at(from, j), kp_pars_state_at(to, j));
        }
    }
}

}  // namespace

extern "C" {

int kp_dist_nj_parsimony(kp_ctx *ctx, kp_dist *d, int32_t min_compared, const kp_nj_node *ref_nodes, int64_t n_ref, int64_t *n_sites, int64_t *n_changes) {
    int rc;
    if ((rc = dist_enter(ctx, d, n_sites && n_changes, "null distance handle or count pointer"))) return rc;
    if (n_ref < 0) return kp_fail(ctx, KP_EINVAL, "a negative record count");
    if (n_ref > 0 && !ref_nodes) return kp_fail(ctx, KP_EINVAL, "null record table of the tree");
    if (n_ref > (int64_t)KP_NJ_MAX_TAXA) return kp_fail(ctx, KP_EINVAL, "more records than a neighbour-joining tree may have (KP_NJ_MAX_TAXA)");
    // ---- the caller's records, on the host, before anything is launched: a tree of the taxa the list itself implies
    const int32_t implied = kp_pars_taxa_of(ref_nodes, n_ref);
    std::vector<int32_t> up((size_t)implied + (size_t)n_ref);
    if (n_ref > 0 && !kp_pars_tree_ok(ref_nodes, n_ref, implied, up.data()))
        return kp_fail(ctx, KP_EINVAL, "the records are no tree: a third child anywhere but in the last record, a node id outside the nodes made before its record, or a node that is a child twice or never");
    kp_dist::Pars &s = d->pars;
    const int32_t R = d->n_rows;
    int32_t n = 0;
    if (R > 0) {
        KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        if ((rc = dist_nj_taxa(ctx, d, min_compared, &n))) return rc;
    }
    if (n > KP_NJ_MAX_TAXA) return kp_fail(ctx, KP_EINVAL, "more taxa than a neighbour-joining tree may have (KP_NJ_MAX_TAXA)");
    const int64_t n_rec = kp_nj_records(n);
    if (n_ref != n_rec || (n_rec > 0 && implied != n))
        return kp_fail(ctx, KP_EINVAL, "the tree has other than the records of the tree of the handle's taxa (n_taxa - 2; one for two taxa)");
    s.done = false;
    s.n_sites = s.n_changes = 0;
    const int64_t NW = d->n_words, cols = 16 * d->n_blocks;
    if (n_rec > 0 && NW > 0) {
        const int64_t n_nodes = (int64_t)n + n_rec, entries = (n_nodes - 1) * NW;
        // ---- the call's own tables, freed when it returns
        DevBuf<uint64_t> tab, steps, alleles;
        DevBuf<kp_nj_node> rec;
        DevBuf<int32_t> parent;
        DevBuf<uint32_t> flag, cnt;
        DevBuf<int64_t> flag_off, cnt_off;
        if ((rc = DistReserve()(tab, (size_t)kp_pars_node_planes(n_nodes, n) * (size_t)NW)(steps, (size_t)KP_PARS_STEP_PLANES * (size_t)NW)(alleles, 4 * (size_t)NW)(rec, (size_t)n_rec)
                      (parent, (size_t)n_nodes)(flag, (size_t)cols)(flag_off, (size_t)cols + 1)(cnt, (size_t)entries)(cnt_off, (size_t)entries + 1).done(ctx, "parsimony tables")))
            return rc;
        KP_HIP_CHECK(ctx, hipMemcpyAsync(rec.p, ref_nodes, (size_t)n_rec * sizeof(kp_nj_node), hipMemcpyHostToDevice, ctx->stream));
        KP_HIP_CHECK(ctx, hipMemcpyAsync(parent.p, up.data(), (size_t)n_nodes * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(kp_pars_pass_kernel, dim3(dist_grid(NW, PARS_THREADS, 1ll << 30)), dim3(PARS_THREADS), 0, ctx->stream, d->d_planes.p, R, NW, d->nj.taxa.p, rec.p, n,
                           (int32_t)n_rec, tab.p, steps.p, alleles.p);
        hipLaunchKernelGGL(kp_pars_site_kernel<false>, dim3(dist_grid(cols)), dim3(DIST_THREADS), 0, ctx->stream, steps.p, alleles.p, NW, cols, flag.p, flag_off.p,
                           (kp_pars_site *)nullptr, (int64_t)0);
        kp_launch_count_scan(flag.p, cols, flag_off.p, ctx->stream);
        hipLaunchKernelGGL(kp_pars_change_kernel<false>, dim3(dist_grid(entries)), dim3(DIST_THREADS), 0, ctx->stream, tab.p, parent.p, n, NW, entries, cnt.p, cnt_off.p,
                           (kp_pars_change *)nullptr, (int64_t)0);
        kp_launch_count_scan(cnt.p, entries, cnt_off.p, ctx->stream);
        KP_HIP_CHECK(ctx, hipGetLastError());
        int64_t ns = 0, nc = 0;
        if ((rc = fetch_all(ctx, ctx->stream, {{&ns, flag_off.p + cols, sizeof(int64_t)}, {&nc, cnt_off.p + entries, sizeof(int64_t)}}))) return rc;
        if (ns < 0 || ns > cols || nc < ns || nc > cols * (n_nodes - 1)) return kp_fail(ctx, KP_ESTATE, "the sites and the changes of the columns do not add up");
        // ---- the records: tables larger than every one before take a buffer of their own size
        if ((rc = dist_grow(ctx, s.site, (size_t)ns, "parsimony sites")) || (rc = dist_grow(ctx, s.change, (size_t)nc, "parsimony changes"))) return rc;
        if (ns > 0)
            hipLaunchKernelGGL(kp_pars_site_kernel<true>, dim3(dist_grid(cols)), dim3(DIST_THREADS), 0, ctx->stream, steps.p, alleles.p, NW, cols, flag.p, flag_off.p, s.site.p, ns);
        if (nc > 0)
            hipLaunchKernelGGL(kp_pars_change_kernel<true>, dim3(dist_grid(entries)), dim3(DIST_THREADS), 0, ctx->stream, tab.p, parent.p, n, NW, entries, cnt.p, cnt_off.p,
                               s.change.p, nc);
        KP_HIP_CHECK(ctx, hipGetLastError());
        KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the node tables go away behind it)
        s.n_sites = ns; s.n_changes = nc;
    }
    s.done = true;
    *n_sites = s.n_sites;
    *n_changes = s.n_changes;
    return KP_OK;
}

int kp_dist_pars_sites(kp_ctx *ctx, kp_dist *d, kp_pars_site *out, int64_t cap) {
    int rc;
    if ((rc = dist_enter(ctx, d, true, "null distance handle"))) return rc;
    const kp_dist::Pars &s = d->pars;
    if (!s.done) return kp_fail(ctx, KP_ESTATE, "kp_dist_nj_parsimony must come first");
    if (cap < s.n_sites || (s.n_sites > 0 && !out)) return kp_fail(ctx, KP_EINVAL, "room for fewer sites than kp_dist_nj_parsimony counted");
    if (s.n_sites == 0) return KP_OK;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KP_HIP_CHECK(ctx, hipMemcpyAsync(out, s.site.p, (size_t)s.n_sites * sizeof(kp_pars_site), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return KP_OK;
}

int kp_dist_pars_changes(kp_ctx *ctx, kp_dist *d, kp_pars_change *out, int64_t cap) {
    int rc;
    if ((rc = dist_enter(ctx, d, true, "null distance handle"))) return rc;
    const kp_dist::Pars &s = d->pars;
    if (!s.done) return kp_fail(ctx, KP_ESTATE, "kp_dist_nj_parsimony must come first");
    if (cap < s.n_changes || (s.n_changes > 0 && !out)) return kp_fail(ctx, KP_EINVAL, "room for fewer changes than kp_dist_nj_parsimony counted");
    if (s.n_changes == 0) return KP_OK;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KP_HIP_CHECK(ctx, hipMemcpyAsync(out, s.change.p, (size_t)s.n_changes * sizeof(kp_pars_change), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return KP_OK;
}

}  // extern "C"
