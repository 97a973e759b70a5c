// kp_dist_boot.hip -- bootstrap support of the neighbour-joining tree of a distance handle (kp_spec.h, BOOTSTRAP; the arithmetic:
// kp_boot.h, kp_nj.h).  The handle, the tiles and the weighted chunk loop: kp_dist_handle.h; the join loop: kp_dist_nj.hip.
//
// A call's replicates are joined in batches (kp_caps.h: kp_boot_batch); a replicate of a batch is blockIdx.y of every kernel:
//   kp_boot_draw_kernel    the W draws of every replicate, histogrammed into count [batch][W]: integer atomic adds.
//   kp_boot_pack_kernel    a wave per (replicate, plane word): a lane clamps the count of its column, eight ballots are the word's
//                          weight planes wplane [batch][8][NW]; an atomic maximum keeps the replicate's highest plane with a bit.
//   kp_dist_boot_kernel    kp_dist_nj_kernel's tiles under the weight planes (dist_tile_counts_w): every pair of taxa stores the
//                          distance of its weighted counts into both triangles of the replicate's dense matrix.  A workgroup fills
//                          one tile of one replicate and loads the tile's strips itself: a strip chunk is 24 KiB that every
//                          replicate's workgroup of the same tile finds in L2, against 16 pairs x 8 words x two popcounts a plane
//                          of work per lane and chunk, and a loop over replicates inside the workgroup would serialise the matrix
//                          fills of a batch of small trees, which is where a batch is largest.
//   (the join loop)        dist_nj_joins (kp_dist_nj.hip): 4 (n - 3) launches a batch.
//   kp_boot_walk_kernel    a lane per replicate walks its records (kp_boot_walk) and leaves its n - 3 splits.
//   kp_boot_count_kernel   a lane per (replicate, split): a binary search of the supported tree's sorted splits, an atomic add into
//                          the counter of the record it matches.
// dist_boot_run is the body of kp_dist_nj_bootstrap and of kp_dist_nj_transfer (kp_dist_transfer.hip), which compares sets where the
// last two kernels compare keys.
// Bounds: count is indexed [rep < batch][column < W] -- a draw is below W by the high product --; wplane [rep][k < 8][word < NW]; top
// [rep]; D [rep][taxon < n][taxon < n] as in kp_dist_nj_kernel; splits [rep][t < n - 3]; ref, ref_rec [n - 3]; support at ref_rec's
// values, which the host checks to be below n - 3.
#include <algorithm>
#include <vector>

#include "kp_dist_handle.h"
#include "kp_boot.h"
#include "kp_nj.h"

namespace {

__global__ __launch_bounds__(DIST_THREADS) void kp_boot_draw_kernel(uint64_t seed, int64_t r0, int64_t W, uint32_t *__restrict__ count) {
    const uint64_t stream = kp_boot_stream(seed, (uint64_t)(r0 + blockIdx.y));
    uint32_t *mine = count + (size_t)blockIdx.y * (size_t)W;
    for (int64_t t = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; t < W; t += (int64_t)gridDim.x * DIST_THREADS) {
        const int64_t c = kp_boot_draw(stream, (uint64_t)t, W);
        if (c >= 0 && c < W) atomicAdd(mine + c, 1u);
    }
}

// (blockDim 256: four waves, a plane word each; the word is the same in every lane of a wave)
__global__ __launch_bounds__(DIST_THREADS) void kp_boot_pack_kernel(const uint32_t *__restrict__ count, int64_t W, int64_t NW, uint64_t *__restrict__ wplane,
                                                                    int32_t *__restrict__ top) {
    const int lane = threadIdx.x & 63;
    const uint32_t *mine = count + (size_t)blockIdx.y * (size_t)W;
    uint64_t *out = wplane + (size_t)blockIdx.y * KP_BOOT_PLANES * (size_t)NW;
    for (int64_t w = (int64_t)blockIdx.x * (DIST_THREADS / 64) + threadIdx.x / 64; w < NW; w += (int64_t)gridDim.x * (DIST_THREADS / 64)) {
        const int64_t c = 64 * w + lane;
        const uint32_t weight = c < W ? kp_boot_weight(mine[c]) : 0u;
        int high = 0;
#pragma unroll
        for (int k = 0; k < KP_BOOT_PLANES; ++k) {
            const uint64_t m = __ballot((weight >> k) & 1u);
            if (lane == 0) out[(size_t)k * (size_t)NW + (size_t)w] = m;
            if (m) high = k + 1;
        }
        if (lane == 0 && high) atomicMax(top + blockIdx.y, high);
    }
}

// kp_dist_nj_kernel under weights: blockIdx.x the tile, blockIdx.y the replicate.
// Bounds: taxon is read at rows < R; its values are -1 or numbers below n, and index the replicate's D [n][n].
__global__ __launch_bounds__(DIST_THREADS) void kp_dist_boot_kernel(const uint64_t *__restrict__ planes, int32_t R, int64_t NW, int32_t nt,
                                                                    const uint64_t *__restrict__ wplane, const int32_t *__restrict__ top,
                                                                    const int32_t *__restrict__ taxon, int32_t n, double *__restrict__ D_all) {
    __shared__ uint64_t s[2][BOOT_STRIP_PLANES][CH][T];
    int32_t ti, tj;
    kp_dist_tile_of((int64_t)blockIdx.x, nt, &ti, &tj);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int rep = blockIdx.y;
    double *__restrict__ D = D_all + (size_t)rep * (size_t)n * (size_t)n;
    int32_t cmp[RG][RG], dif[RG][RG];
    dist_tile_counts_w(planes, R, NW, ti, tj, wplane + (size_t)rep * KP_BOOT_PLANES * (size_t)NW, top[rep], s, cmp, dif);
    int32_t tb[RG];
#pragma unroll
    for (int j = 0; j < RG; ++j) {
        const int64_t b = (int64_t)tj * T + tx + 16 * j;
        tb[j] = b < R ? taxon[b] : -1;
    }
#pragma unroll
    for (int i = 0; i < RG; ++i) {
        const int64_t a = (int64_t)ti * T + ty + 16 * i;
        const int32_t ta = a < R ? taxon[a] : -1;
        if (ta < 0 || ta >= n) continue;
#pragma unroll
        for (int j = 0; j < RG; ++j) {
            const int64_t b = (int64_t)tj * T + tx + 16 * j;
            if (tb[j] < 0 || tb[j] >= n || a > b) continue;
            const double dist = a == b ? 0.0 : kp_nj_distance(dif[i][j], cmp[i][j]);
            D[(size_t)ta * (size_t)n + (size_t)tb[j]] = dist;
            D[(size_t)tb[j] * (size_t)n + (size_t)ta] = dist;
        }
    }
}

// a lane per replicate: its splits, [n - 3] behind the replicate's stride
__global__ __launch_bounds__(DIST_THREADS) void kp_boot_walk_kernel(const kp_nj_node *__restrict__ rec, int64_t n_rec, int32_t n, uint64_t total, int32_t batch,
                                                                    KpBootSplit *__restrict__ splits) {
    const int64_t rep = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x;
    if (rep >= batch) return;
    kp_boot_walk(rec + (size_t)rep * (size_t)n_rec, n, total, splits + (size_t)rep * (size_t)kp_boot_splits(n));
}

// a lane per split of the batch: the first entry of ref that is not less, and every entry equal to it, counts the split
__global__ __launch_bounds__(DIST_THREADS) void kp_boot_count_kernel(const KpBootSplit *__restrict__ splits, int64_t n_all, const KpBootSplit *__restrict__ ref,
                                                                     const int32_t *__restrict__ ref_rec, int32_t n_ref, uint32_t *__restrict__ support) {
    for (int64_t e = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; e < n_all; e += (int64_t)gridDim.x * DIST_THREADS) {
        const KpBootSplit x = splits[e];
        int32_t lo = 0, hi = n_ref;
        while (lo < hi) {
            const int32_t mid = lo + (hi - lo) / 2;
            if (kp_boot_split_less(ref[mid], x)) lo = mid + 1; else hi = mid;
        }
        for (; lo < n_ref && kp_boot_split_same(ref[lo], x); ++lo) {
            const int32_t r = ref_rec[lo];
            if (r >= 0 && r < n_ref) atomicAdd(support + r, 1u);
        }
    }
}

// count and wplane of `batch` replicates from replicate r0 on, top zeroed first
int boot_weigh(kp_ctx *ctx, const kp_dist *d, uint64_t seed, int64_t r0, int32_t batch, uint32_t *count, uint64_t *wplane, int32_t *top) {
    const int64_t W = 16 * d->n_blocks, NW = kp_dist_words(d->n_blocks);
    KP_HIP_CHECK(ctx, hipMemsetAsync(count, 0, (size_t)batch * (size_t)W * sizeof(uint32_t), ctx->stream));
    KP_HIP_CHECK(ctx, hipMemsetAsync(top, 0, (size_t)batch * sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(kp_boot_draw_kernel, dim3(dist_grid(W, DIST_THREADS, 1024), (unsigned)batch), dim3(DIST_THREADS), 0, ctx->stream, seed, r0, W, count);
    hipLaunchKernelGGL(kp_boot_pack_kernel, dim3(dist_grid(NW, DIST_THREADS / 64, 1024), (unsigned)batch), dim3(DIST_THREADS), 0, ctx->stream, count, W, NW, wplane, top);
    KP_HIP_CHECK(ctx, hipGetLastError());
    return KP_OK;
}

}  // namespace

// The body of kp_dist_nj_bootstrap and of kp_dist_nj_transfer (`pass`: kp_dist_transfer.hip): the checks, the tables, the batch loop.
// Without a pass the splits of every batch are counted by their keys; with one the pass compares the sets, and support is its count of
// the replicates at distance 0.
int dist_boot_run(kp_ctx *ctx, kp_dist *d, int32_t min_compared, uint64_t seed, int32_t replicates, int32_t max_batch, const kp_nj_node *ref_nodes, int64_t n_ref,
                  int32_t *support, int64_t cap_support, kp_nj_node *trees, int64_t cap_trees, TransferPass *pass) {
    int rc;
    if ((rc = dist_enter(ctx, d, true, "null distance handle"))) return rc;
    if (replicates < 1 || replicates > KP_BOOT_MAX_REPLICATES) return kp_fail(ctx, KP_EINVAL, "replicates outside 1 .. KP_BOOT_MAX_REPLICATES");
    if (max_batch < 0 || n_ref < 0 || cap_support < 0 || cap_trees < 0) return kp_fail(ctx, KP_EINVAL, "a negative batch limit, record count or room");
    if (n_ref > 0 && !ref_nodes) return kp_fail(ctx, KP_EINVAL, "null record table of the supported tree");
    if (n_ref > 0 && !support) return kp_fail(ctx, KP_EINVAL, "null support table");
    if (cap_trees > 0 && !trees) return kp_fail(ctx, KP_EINVAL, "null table of replicate trees with room asked for");
    if (pass) {
        if (pass->cap_transfer < 0 || pass->cap_per < 0) return kp_fail(ctx, KP_EINVAL, "a negative batch limit, record count or room");
        if (n_ref > 0 && !pass->transfer) return kp_fail(ctx, KP_EINVAL, "null transfer table");
        if (pass->cap_per > 0 && !pass->per_replicate) return kp_fail(ctx, KP_EINVAL, "null table of transfer distances with room asked for");
    }
    const int32_t R = d->n_rows;
    int32_t n = 0;
    if (R > 0) {
        if (16 * d->n_blocks >= KP_TREE_MAX_COLUMNS) return kp_fail(ctx, KP_EINVAL, "too many columns for weighted counts (KP_TREE_MAX_COLUMNS)");
        KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        if ((rc = dist_nj_taxa(ctx, d, min_compared, &n))) return rc;
    }
    if (n > KP_NJ_MAX_TAXA) return kp_fail(ctx, KP_EINVAL, "more taxa than a neighbour-joining tree may have (KP_NJ_MAX_TAXA)");
    const int64_t n_rec = kp_nj_records(n), S = kp_boot_splits(n);
    if (n_ref != n_rec) return kp_fail(ctx, KP_EINVAL, "the supported tree has other than the records of the tree of the handle's taxa (n_taxa - 2; one for two taxa)");
    if (cap_support < n_ref) return kp_fail(ctx, KP_EINVAL, "room for fewer support values than the tree has records");
    if (trees && cap_trees < (int64_t)replicates * n_rec) return kp_fail(ctx, KP_EINVAL, "room for fewer records than the replicate trees have (replicates x records)");
    if (pass && pass->cap_transfer < n_ref) return kp_fail(ctx, KP_EINVAL, "room for fewer transfer sums than the tree has records");
    if (pass && pass->per_replicate && pass->cap_per < (int64_t)replicates * n_ref)
        return kp_fail(ctx, KP_EINVAL, "room for fewer transfer distances than the replicates have (replicates x records)");
    for (int64_t t = 0; t < n_ref; ++t) {  // (the walk below reads children made before their record only; say so here)
        const kp_nj_node &p = ref_nodes[t];
        const int32_t child[3] = {p.a, p.b, p.c};
        for (int k = 0; k < (t == n_ref - 1 && n > 2 ? 3 : 2); ++k)
            if (child[k] < 0 || child[k] >= n + t) return kp_fail(ctx, KP_EINVAL, "a node id of the supported tree outside the nodes made before its record");
    }
    if (S == 0 && !trees) {  // two or three taxa, or none: no inner edge, nothing to join
        for (int64_t t = 0; t < n_ref; ++t) support[t] = -1;
        if (pass) pass->none(replicates, n_ref);
        return KP_OK;
    }
    if (n_rec == 0) return KP_OK;
    const int64_t W = 16 * d->n_blocks, NW = d->n_words;
    kp_dist::Boot &bt = d->boot;
    const size_t rows = (size_t)R;
    if ((rc = DistReserve()(bt.ref, rows)(bt.ref_rec, rows)(bt.support, rows).done(ctx, "bootstrap tables"))) return rc;
    const uint64_t total = kp_boot_total_key(n);
    // ---- the splits of the supported tree, sorted
    if (S > 0 && !pass) {
        std::vector<KpBootSplit> ref((size_t)S);
        kp_boot_walk(ref_nodes, n, total, ref.data());
        std::vector<int32_t> order((size_t)S);
        for (int64_t t = 0; t < S; ++t) order[(size_t)t] = (int32_t)t;
        std::sort(order.begin(), order.end(), [&ref](int32_t x, int32_t y) { return kp_boot_split_less(ref[(size_t)x], ref[(size_t)y]) || (!kp_boot_split_less(ref[(size_t)y], ref[(size_t)x]) && x < y); });
        std::vector<KpBootSplit> sorted((size_t)S);
        for (int64_t t = 0; t < S; ++t) sorted[(size_t)t] = ref[(size_t)order[(size_t)t]];
        KP_HIP_CHECK(ctx, hipMemcpyAsync(bt.ref.p, sorted.data(), (size_t)S * sizeof(KpBootSplit), hipMemcpyHostToDevice, ctx->stream));
        KP_HIP_CHECK(ctx, hipMemcpyAsync(bt.ref_rec.p, order.data(), (size_t)S * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
        KP_HIP_CHECK(ctx, hipMemsetAsync(bt.support.p, 0, (size_t)S * sizeof(uint32_t), ctx->stream));
        KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the host vectors go away)
    }
    // ---- a batch's tables: this call's own, freed when it returns
    const int32_t batch = kp_boot_batch(n, replicates, max_batch);
    const size_t B = (size_t)batch, N = (size_t)n;
    const int32_t parts = dist_nj_parts(n);
    DevBuf<uint32_t> count;
    DevBuf<uint64_t> wplane;
    DevBuf<int32_t> top, node, cell;
    DevBuf<double> D, sum;
    DevBuf<kp_nj_node> rec;
    DevBuf<NjBest> part;
    DevBuf<KpBootSplit> splits;
    if ((rc = DistReserve()(count, B * (size_t)W)(wplane, B * KP_BOOT_PLANES * (size_t)NW)(top, B)(D, B * N * N)(sum, B * N)(node, B * N)(cell, 2 * B)(rec, B * (size_t)n_rec)
                  (part, B * (size_t)parts)(splits, B * (size_t)std::max<int64_t>(S, 1)).done(ctx, "bootstrap matrices")))
        return rc;
    const NjBatch tables{D.p, sum.p, node.p, cell.p, rec.p, part.p, (int64_t)(N * N), n, (int32_t)n_rec, parts};
    const int64_t tiles = kp_dist_tiles(d->nt);
    if (tiles <= 0 || tiles * DIST_THREADS >= (1ll << 32)) return kp_fail(ctx, KP_EINVAL, "too many tiles for one grid (KP_DIST_MAX_ROWS)");
    if (pass && S > 0) {  // ---- the sets of the supported tree
        if ((rc = pass->reserve(ctx, d, n, batch))) return rc;
        if ((rc = pass->begin(ctx, d, ref_nodes))) return rc;
    }
    for (int32_t r0 = 0; r0 < replicates; r0 += batch) {
        const int32_t b = std::min<int32_t>(batch, replicates - r0);
        if ((rc = boot_weigh(ctx, d, seed, r0, b, count.p, wplane.p, top.p))) return rc;
        hipLaunchKernelGGL(kp_dist_boot_kernel, dim3((unsigned)tiles, (unsigned)b), dim3(DIST_THREADS), 0, ctx->stream, d->d_planes.p, R, NW, d->nt, wplane.p, top.p,
                           d->nj.taxon.p, n, D.p);
        KP_HIP_CHECK(ctx, hipGetLastError());
        int64_t made = 0;
        if ((rc = dist_nj_joins(ctx, tables, n, b, &made))) return rc;
        if (made != n_rec) return kp_fail(ctx, KP_ESTATE, "the joins do not add up to the tree's records");
        if (S > 0 && pass) {
            if ((rc = pass->batch(ctx, d, rec.p, D.p, (int64_t)(N * N), b))) return rc;
            if (pass->per_replicate)
                KP_HIP_CHECK(ctx, hipMemcpyAsync(pass->per_replicate + (size_t)r0 * (size_t)n_rec, pass->phi.p, (size_t)b * (size_t)n_rec * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
        } else if (S > 0) {
            hipLaunchKernelGGL(kp_boot_walk_kernel, dim3(dist_grid(b)), dim3(DIST_THREADS), 0, ctx->stream, rec.p, n_rec, n, total, b, splits.p);
            hipLaunchKernelGGL(kp_boot_count_kernel, dim3(dist_grid((int64_t)b * S)), dim3(DIST_THREADS), 0, ctx->stream, splits.p, (int64_t)b * S, bt.ref.p, bt.ref_rec.p,
                               (int32_t)S, bt.support.p);
            KP_HIP_CHECK(ctx, hipGetLastError());
        }
        if (trees) KP_HIP_CHECK(ctx, hipMemcpyAsync(trees + (size_t)r0 * (size_t)n_rec, rec.p, (size_t)b * (size_t)n_rec * sizeof(kp_nj_node), hipMemcpyDeviceToHost, ctx->stream));
    }
    std::vector<uint32_t> got((size_t)S);
    if (S > 0 && pass) {
        if ((rc = pass->fetch(ctx, d))) return rc;
    } else if (S > 0) KP_HIP_CHECK(ctx, hipMemcpyAsync(got.data(), bt.support.p, (size_t)S * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the matrices go away behind it)
    if (trees)
        for (int64_t r = 0; r < (int64_t)replicates * n_rec; ++r)
            if (trees[r].a < 0) return kp_fail(ctx, KP_ESTATE, "a join found no pair");
    if (pass && S == 0) pass->none(replicates, n_ref);
    if (pass && S > 0) {
        for (int64_t t = 0; t < n_ref; ++t) {
            support[t] = t < S ? (int32_t)pass->got_exact[(size_t)t] : -1;
            pass->transfer[t] = t < S ? (int64_t)pass->got_transfer[(size_t)t] : -1;
        }
        return KP_OK;
    }
    for (int64_t t = 0; t < n_ref; ++t) support[t] = t < S ? (int32_t)got[(size_t)t] : -1;
    return KP_OK;
}

extern "C" {

int kp_dist_boot_weights(kp_ctx *ctx, kp_dist *d, uint64_t seed, int32_t replicate, uint8_t *weights, int64_t cap) {
    int rc;
    if ((rc = dist_enter(ctx, d, weights || (d && d->n_blocks == 0), "null distance handle or weight table"))) return rc;
    if (replicate < 0 || replicate >= KP_BOOT_MAX_REPLICATES) return kp_fail(ctx, KP_EINVAL, "a replicate outside 0 .. KP_BOOT_MAX_REPLICATES - 1");
    const int64_t W = 16 * d->n_blocks, NW = kp_dist_words(d->n_blocks);  // (the draws need no row)
    if (cap < W) return kp_fail(ctx, KP_EINVAL, "room for fewer weights than the matrix has block columns (16 n_blocks)");
    if (W >= KP_TREE_MAX_COLUMNS) return kp_fail(ctx, KP_EINVAL, "too many columns for weighted counts (KP_TREE_MAX_COLUMNS)");
    if (W == 0) return KP_OK;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    DevBuf<uint32_t> count;
    DevBuf<uint64_t> wplane;
    DevBuf<int32_t> top;
    if ((rc = DistReserve()(count, (size_t)W)(wplane, KP_BOOT_PLANES * (size_t)NW)(top, 1).done(ctx, "bootstrap weights"))) return rc;
    if ((rc = boot_weigh(ctx, d, seed, replicate, 1, count.p, wplane.p, top.p))) return rc;
    std::vector<uint64_t> planes(KP_BOOT_PLANES * (size_t)NW);
    int32_t high = 0;
    KP_HIP_CHECK(ctx, hipMemcpyAsync(planes.data(), wplane.p, planes.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipMemcpyAsync(&high, top.p, sizeof high, hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (int64_t c = 0; c < W; ++c) {
        uint32_t w = 0;
        for (int k = 0; k < high && k < KP_BOOT_PLANES; ++k) w |= (uint32_t)((planes[(size_t)k * (size_t)NW + (size_t)(c / 64)] >> (c % 64)) & 1u) << k;  // (the planes the tile kernel reads)
        weights[c] = (uint8_t)w;
    }
    return KP_OK;
}

int kp_dist_nj_bootstrap(kp_ctx *ctx, kp_dist *d, int32_t min_compared, uint64_t seed, int32_t replicates, int32_t max_batch, const kp_nj_node *ref_nodes,
                         int64_t n_ref, int32_t *support, int64_t cap_support, kp_nj_node *trees, int64_t cap_trees) {
    return dist_boot_run(ctx, d, min_compared, seed, replicates, max_batch, ref_nodes, n_ref, support, cap_support, trees, cap_trees, nullptr);
}

}  // extern "C"
