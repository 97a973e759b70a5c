// kp_dist_graph.hip -- the two graph reports over the locus rows of a distance handle: single-linkage clusters with nearest neighbours
// (kp_spec.h, CLUSTERS; the arithmetic: kp_clust.h) and the minimum spanning forest (kp_spec.h, TREE; kp_tree.h).  The handle, the
// tiles and their chunk loop: kp_dist_handle.h.  One unit for both: they share a union-find (kp_clust_init_kernel,
// kp_clust_flatten_kernel) and the two key reductions of a tile, which no other report uses.
//
//   kp_dist_clust_kernel   the pair kernel's tiles and counts with another epilogue: every valid pair is united
//                          into the parent arrays of its levels by a lock-free union-find and offered to both of its rows as
//                          nearest partner -- reduced inside the tile, then one 64-bit atomic minimum per row and tile.  Around
//                          it kp_clust_init_kernel (identity parents, no partner), kp_clust_flatten_kernel (label = root) and
//                          kp_dist_nearest_kernel (the partner's three counts, recomputed).  No pair is stored.
//
//   kp_dist_tree_kernel    the same tiles and counts with a third epilogue: one round of Boruvka.  Every valid
//                          pair whose rows carry different labels offers its packed key to both components -- reduced inside the
//                          tile as the nearest keys are, then one 64-bit atomic minimum per row and tile.  Around it
//                          kp_tree_round_kernel (no edge yet), kp_tree_hook_kernel (one union per component and round; the root
//                          that moved keeps the edge), kp_clust_flatten_kernel (next round's labels) and, after the last round,
//                          kp_tree_edge_kernel (the edges' three counts, recomputed).  No pair is stored.
//
// Written once for both: dist_row_min / dist_col_min (a key's minimum per row and column of the tile).
#include <algorithm>
#include <climits>
#include <vector>

#include "kp_dist_handle.h"
#include "kp_clust.h"
#include "kp_tree.h"

#ifndef KP_TREE_SKIP
#define KP_TREE_SKIP 1 /* a tile whose rows all carry one label returns before the chunk loop: it holds no outgoing edge */
#endif

namespace {

// A 64-bit key's minimum over the tile, for the epilogues that send one atomic minimum per row and per column of it.
// Row a = ty + 16 i of the tile: its sixteen pairs of one j are the sixteen tx of ty's lanes in one wave, so the lane's minimum over j
// goes through four xor-shuffles and every tx holds the row's.
__device__ __forceinline__ uint64_t dist_row_min(uint64_t key) {
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) key = std::min(key, (uint64_t)__shfl_xor((unsigned long long)key, o));
    return key;
}
// Column b = tx + 16 j of the tile is spread over all ty: col_key[j] is the lane's minimum over i; two xor-shuffles take it over the
// four ty of its wave, then the four waves meet in LDS (the strips are free behind the last __syncthreads of the chunk loop), and
// lane tid < T returns the minimum of column tid.  The other lanes return KP_DIST_KEY_NONE.
// Bounds: LDS is written and read at [wave < 4][column < 64] of the strips' first 2 KiB.
__device__ __forceinline__ uint64_t dist_col_min(const uint64_t (&col_key)[RG], uint64_t (&s)[2][KP_DIST_PLANES][CH][T]) {
    const int tid = threadIdx.x, tx = tid & 15;
    uint64_t (*col_best)[T] = reinterpret_cast<uint64_t (*)[T]>(&s[0][0][0][0]);  // [wave][column of the tile]
    const int wave = tid >> 6;
#pragma unroll
    for (int j = 0; j < RG; ++j) {
        uint64_t k = col_key[j];
        k = std::min(k, (uint64_t)__shfl_xor((unsigned long long)k, 16));
        k = std::min(k, (uint64_t)__shfl_xor((unsigned long long)k, 32));
        if ((tid & 63) < 16) col_best[wave][tx + 16 * j] = k;
    }
    __syncthreads();
    if (tid >= T) return KP_DIST_KEY_NONE;
    return std::min(std::min(col_best[0][tid], col_best[1][tid]), std::min(col_best[2][tid], col_best[3][tid]));
}

// ---- clusters and nearest neighbours (kp_spec.h, CLUSTERS; the arithmetic: kp_clust.h) ----------------------------------------------
// parent[k][r] = r, best[r] = none
__global__ __launch_bounds__(DIST_THREADS) void kp_clust_init_kernel(int32_t R, int32_t K, int32_t *__restrict__ parent, unsigned long long *__restrict__ best) {
    const int64_t n = (int64_t)R * K;
    for (int64_t e = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; e < std::max<int64_t>(n, R); e += (int64_t)gridDim.x * DIST_THREADS) {
        if (e < n) parent[e] = (int32_t)(e % R);
        if (e < R) best[e] = KP_DIST_KEY_NONE;
    }
}

// The pair kernel's tiles and counts with another epilogue.  A valid pair (a < b < R, compared >= min_compared)
//   * is an edge from its first level on: it is united into parent[k][..] of those levels (kp_clust_edge; lock-free, no lane waits
//     for another), and
//   * offers b to a and a to b as nearest partner.  tx 0 sends row a's minimum of this tile (dist_row_min) to best[a], the first 64
//     lanes column b's (dist_col_min) to best[b] -- one 64-bit atomic minimum per row and tile and one per column and tile.  A
//     diagonal tile holds the same rows on both sides; a < b keeps each pair once, and it still offers both ways.
// Bounds: parent is read and written at rows a, b < R of levels < K and at values read from it, which are row indices (the init
// kernel stored r, a hook stores a root, halving a grandparent); best at a, b < R.
__global__ __launch_bounds__(DIST_THREADS) void kp_dist_clust_kernel(const uint64_t *__restrict__ planes, int32_t R, int64_t NW, int32_t nt,
                                                                     KpClustLevels levels, int32_t min_compared, int32_t *__restrict__ parent,
                                                                     unsigned long long *__restrict__ best) {
    __shared__ uint64_t s[2][KP_DIST_PLANES][CH][T];
    int32_t ti, tj;
    kp_dist_tile_of((int64_t)blockIdx.x, nt, &ti, &tj);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    int32_t cmp[RG][RG], dif[RG][RG], uns[RG][RG];
    dist_tile_counts(planes, R, NW, ti, tj, s, cmp, dif, uns);
    const int32_t K = levels.n;
    uint64_t col_key[RG];
#pragma unroll
    for (int j = 0; j < RG; ++j) col_key[j] = KP_DIST_KEY_NONE;
#pragma unroll
    for (int i = 0; i < RG; ++i) {
        const int64_t a = (int64_t)ti * T + ty + 16 * i;
        uint64_t row_key = KP_DIST_KEY_NONE;
#pragma unroll
        for (int j = 0; j < RG; ++j) {
            const int64_t b = (int64_t)tj * T + tx + 16 * j;
            if (a < b && b < R && cmp[i][j] >= min_compared) {
                row_key = std::min(row_key, kp_clust_key(dif[i][j], (int32_t)b));
                col_key[j] = std::min(col_key[j], kp_clust_key(dif[i][j], (int32_t)a));
                kp_clust_edge(parent, R, K, kp_clust_first_level(levels, dif[i][j]), (int32_t)a, (int32_t)b);
            }
        }
        row_key = dist_row_min(row_key);
        if (tx == 0 && a < R && row_key != KP_DIST_KEY_NONE) atomicMin(best + a, (unsigned long long)row_key);
    }
    const uint64_t k = dist_col_min(col_key, s);
    const int64_t b = (int64_t)tj * T + tid;
    if (tid < T && b < R && k != KP_DIST_KEY_NONE) atomicMin(best + b, (unsigned long long)k);
}

// label[k][r] = the root of r at level k.  A launch of its own: the kernel boundary is what orders it behind every hook.
__global__ __launch_bounds__(DIST_THREADS) void kp_clust_flatten_kernel(int32_t R, int32_t K, int32_t *__restrict__ parent, int32_t *__restrict__ label) {
    const int64_t n = (int64_t)R * K;
    for (int64_t e = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * DIST_THREADS) {
        const int64_t k = e / R;
        label[e] = kp_clust_find(parent + k * R, (int32_t)(e - k * R));
    }
}

// The nearest record of every row: the partner of best[r] and the pair's three counts, recomputed from the planes.
__global__ __launch_bounds__(DIST_THREADS) void kp_dist_nearest_kernel(const uint64_t *__restrict__ planes, int32_t R, int64_t NW,
                                                                       const unsigned long long *__restrict__ best, kp_dist_nearest *__restrict__ out) {
    for (int64_t r = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; r < R; r += (int64_t)gridDim.x * DIST_THREADS) {
        const int32_t partner = kp_clust_key_row(best[r]);
        KpDistCounts n{0, 0, 0};
        if (partner >= 0 && partner < R) n = kp_dist_plane_counts(planes, R, NW, r, partner);
        kp_dist_nearest_store(out + r, partner >= 0 && partner < R ? partner : -1, n.compared, n.differences, n.unshared);
    }
}

// ---- minimum spanning forest (kp_spec.h, TREE; the arithmetic: kp_tree.h) -------------------------------------------------------------
// a round begins: no component has an edge, the round has none
__global__ __launch_bounds__(DIST_THREADS) void kp_tree_round_kernel(int32_t R, unsigned long long *__restrict__ cbest, uint32_t *__restrict__ n_new) {
    for (int64_t r = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; r < R; r += (int64_t)gridDim.x * DIST_THREADS) cbest[r] = KP_DIST_KEY_NONE;
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_new = 0u;
}

// The pair kernel's tiles and counts with a third epilogue.  A valid pair (a < b < R, compared >= min_compared) whose rows carry
// different labels offers its packed key to label[a]'s and to label[b]'s component: the key is canonical, both sides send the same
// value.  The reductions are those of the cluster kernel's nearest keys (dist_row_min, dist_col_min), then one 64-bit atomic minimum
// per row and tile and one per column and tile.
// KP_TREE_SKIP: the labels of the tile's 128 rows are compared with the first one's before any plane word is read; where none
// differs the tile holds no outgoing edge and the whole block returns -- __syncthreads_or makes the branch uniform.
// Bounds: label is read at rows < R; its values are roots, rows < R (kp_clust_flatten_kernel stored them), and index cbest.
__global__ __launch_bounds__(DIST_THREADS) void kp_dist_tree_kernel(const uint64_t *__restrict__ planes, int32_t R, int64_t NW, int32_t nt, int32_t min_compared,
                                                                    const int32_t *__restrict__ label, unsigned long long *__restrict__ cbest) {
    __shared__ uint64_t s[2][KP_DIST_PLANES][CH][T];
    int32_t ti, tj;
    kp_dist_tile_of((int64_t)blockIdx.x, nt, &ti, &tj);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#if KP_TREE_SKIP
    {
        const int32_t first = label[(int64_t)ti * T];  // (a launched tile has a first row: ti * T < R)
        int differs = 0;
        if (tid < 2 * T) {
            const int64_t r = (int64_t)(tid < T ? ti : tj) * T + (tid & (T - 1));
            if (r < R) differs = label[r] != first;
        }
        if (!__syncthreads_or(differs)) return;
    }
#endif
    int32_t cmp[RG][RG], dif[RG][RG], uns[RG][RG];
    dist_tile_counts(planes, R, NW, ti, tj, s, cmp, dif, uns);
    int32_t lb[RG];
    uint64_t col_key[RG];
#pragma unroll
    for (int j = 0; j < RG; ++j) {
        const int64_t b = (int64_t)tj * T + tx + 16 * j;
        lb[j] = b < R ? label[b] : -1;
        col_key[j] = KP_DIST_KEY_NONE;
    }
#pragma unroll
    for (int i = 0; i < RG; ++i) {
        const int64_t a = (int64_t)ti * T + ty + 16 * i;
        const int32_t la = a < R ? label[a] : -1;
        uint64_t row_key = KP_DIST_KEY_NONE;
#pragma unroll
        for (int j = 0; j < RG; ++j) {
            const int64_t b = (int64_t)tj * T + tx + 16 * j;
            if (a < b && b < R && cmp[i][j] >= min_compared && la != lb[j]) {
                const uint64_t k = kp_tree_key(dif[i][j], (int32_t)a, (int32_t)b);
                row_key = std::min(row_key, k);
                col_key[j] = std::min(col_key[j], k);
            }
        }
        row_key = dist_row_min(row_key);
        if (tx == 0 && a < R && row_key != KP_DIST_KEY_NONE) atomicMin(cbest + la, (unsigned long long)row_key);
    }
    const uint64_t k = dist_col_min(col_key, s);
    const int64_t b = (int64_t)tj * T + tid;
    if (tid < T && b < R && k != KP_DIST_KEY_NONE) atomicMin(cbest + label[b], (unsigned long long)k);
}

// One lane per component that has an edge: the union of the edge's rows.  Under a strict total order the chosen edges close no
// cycle; an edge chosen from both sides is united once -- the second union finds one root -- and is kept iff the union moved a
// root, in that root's slot: a root moves at most once in its life, so no two lanes of any round share a slot.
// Bounds: a and b come out of a key the tree kernel packed from rows < R; the moved root is a row < R.
__global__ __launch_bounds__(DIST_THREADS) void kp_tree_hook_kernel(int32_t R, const int32_t *__restrict__ label, const unsigned long long *__restrict__ cbest,
                                                                    int32_t *__restrict__ parent, unsigned long long *__restrict__ slot, uint32_t *__restrict__ n_new) {
    for (int64_t r = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; r < R; r += (int64_t)gridDim.x * DIST_THREADS) {
        if (label[r] != (int32_t)r) continue;
        const uint64_t key = cbest[r];
        if (key == KP_DIST_KEY_NONE) continue;
        const int32_t a = kp_tree_key_a(key), b = kp_tree_key_b(key);
        if (a >= b || b >= R) continue;  // (no key the tree kernel packs)
        const int32_t moved = kp_clust_unite_root(parent, a, b);
        if (moved >= 0) {
            slot[moved] = key;
            atomicAdd(n_new, 1u);
        }
    }
}

// The slots as records: a row whose slot holds an edge gets the edge's rows and its three counts, recomputed from the planes; every
// other row a record with a = -1.
__global__ __launch_bounds__(DIST_THREADS) void kp_tree_edge_kernel(const uint64_t *__restrict__ planes, int32_t R, int64_t NW,
                                                                    const unsigned long long *__restrict__ slot, kp_dist_pair *__restrict__ out) {
    for (int64_t r = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; r < R; r += (int64_t)gridDim.x * DIST_THREADS) {
        const uint64_t key = slot[r];
        const int32_t a = kp_tree_key_a(key), b = kp_tree_key_b(key);
        if (key == KP_DIST_KEY_NONE || a >= b || b >= R) {
            kp_dist_pair_store(out + r, -1, -1, 0, 0, 0);
            continue;
        }
        const KpDistCounts n = kp_dist_plane_counts(planes, R, NW, a, b);
        kp_dist_pair_store(out + r, a, b, n.compared, n.differences, n.unshared);
    }
}

}  // namespace

extern "C" {

int kp_dist_clusters(kp_ctx *ctx, kp_dist *d, const int32_t *levels, int32_t n_levels, int32_t min_compared, int32_t *labels, kp_dist_nearest *nearest) {
    int rc;
    if ((rc = dist_enter(ctx, d, true, "null distance handle"))) return rc;
    if (n_levels < 0 || n_levels > KP_CLUST_MAX_LEVELS) return kp_fail(ctx, KP_EINVAL, "number of cluster levels outside 0 .. KP_CLUST_MAX_LEVELS");
    if (n_levels > 0 && !levels) return kp_fail(ctx, KP_EINVAL, "null cluster levels");
    if (!kp_clust_levels_valid(levels, n_levels)) return kp_fail(ctx, KP_EINVAL, "cluster levels must be non-negative and strictly ascending");
    if (n_levels > 0 && d->n_rows > 0 && !labels) return kp_fail(ctx, KP_EINVAL, "null label table");
    const int32_t R = d->n_rows, K = n_levels;
    if (R == 0 || (K == 0 && !nearest)) return KP_OK;
    KpClustLevels lv{};
    for (int32_t k = 0; k < KP_CLUST_MAX_LEVELS; ++k) lv.t[k] = k < K ? levels[k] : INT32_MAX;
    lv.n = K;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    kp_dist::Clusters &c = d->clust;
    const size_t all = (size_t)KP_CLUST_MAX_LEVELS * (size_t)R;
    if ((rc = DistReserve()(c.parent, all)(c.label, all)(c.best, (size_t)R)(c.nearest, (size_t)R).done(ctx, "cluster tables"))) return rc;
    hipLaunchKernelGGL(kp_clust_init_kernel, dim3(dist_grid((int64_t)R * std::max(K, 1))), dim3(DIST_THREADS), 0, ctx->stream, R, K, c.parent.p, c.best.p);
    // (one row: no tile kernel; label 0 and no neighbour come from the init kernel's tables)
    if (R > 1 && (rc = dist_launch_tiles(ctx, d, kp_dist_clust_kernel, lv, min_compared, c.parent.p, c.best.p))) return rc;
    if (K > 0) {
        hipLaunchKernelGGL(kp_clust_flatten_kernel, dim3(dist_grid((int64_t)R * K)), dim3(DIST_THREADS), 0, ctx->stream, R, K, c.parent.p, c.label.p);
        KP_HIP_CHECK(ctx, hipGetLastError());
        KP_HIP_CHECK(ctx, hipMemcpyAsync(labels, c.label.p, (size_t)K * (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (nearest) {
        hipLaunchKernelGGL(kp_dist_nearest_kernel, dim3(dist_grid(R)), dim3(DIST_THREADS), 0, ctx->stream, d->d_planes.p, R, d->n_words, c.best.p, c.nearest.p);
        KP_HIP_CHECK(ctx, hipGetLastError());
        KP_HIP_CHECK(ctx, hipMemcpyAsync(nearest, c.nearest.p, (size_t)R * sizeof(kp_dist_nearest), hipMemcpyDeviceToHost, ctx->stream));
    }
    KP_HIP_CHECK(ctx, hipGetLastError());
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return KP_OK;
}

int kp_dist_tree(kp_ctx *ctx, kp_dist *d, int32_t min_compared, kp_dist_pair *edges, int64_t cap, int64_t *n_edges, int32_t *component) {
    if (ctx && d && n_edges) *n_edges = 0;  // (whatever refuses the call from here on)
    int rc;
    if ((rc = dist_enter(ctx, d, n_edges, "null distance handle or edge count pointer"))) return rc;
    if (!kp_tree_fits(d->n_blocks)) return kp_fail(ctx, KP_EINVAL, "a locus of 2^28 columns or more does not fit the tree's edge key (KP_TREE_MAX_COLUMNS)");
    const int32_t R = d->n_rows;
    if (R > 1 && cap < (int64_t)R - 1) return kp_fail(ctx, KP_EINVAL, "room for fewer edges than a tree of the rows may have (n_rows - 1)");
    if (cap > 0 && !edges) return kp_fail(ctx, KP_EINVAL, "null edge table");
    kp_dist::Tree &t = d->tree;
    t.rounds = 0;
    if (R == 0) return KP_OK;
    if (R == 1) {  // one row: its own tree, no edge, no launch
        if (component) component[0] = 0;
        return KP_OK;
    }
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if ((rc = DistReserve()(t.parent, (size_t)R)(t.label, (size_t)R)(t.best, (size_t)R)(t.slot, (size_t)R)(t.rec, (size_t)R)(t.fresh, 1).done(ctx, "tree tables"))) return rc;
    const unsigned grid = dist_grid(R);
    // identity parents and empty slots; the first round's labels are the rows themselves
    hipLaunchKernelGGL(kp_clust_init_kernel, dim3(grid), dim3(DIST_THREADS), 0, ctx->stream, R, 1, t.parent.p, t.slot.p);
    hipLaunchKernelGGL(kp_clust_flatten_kernel, dim3(grid), dim3(DIST_THREADS), 0, ctx->stream, R, 1, t.parent.p, t.label.p);
    KP_HIP_CHECK(ctx, hipGetLastError());
    const int32_t bound = kp_tree_max_rounds(R);
    uint32_t fresh = 1;
    int64_t total = 0;
    for (int32_t round = 0; round < bound && fresh != 0; ++round) {
        hipLaunchKernelGGL(kp_tree_round_kernel, dim3(grid), dim3(DIST_THREADS), 0, ctx->stream, R, t.best.p, t.fresh.p);
        if ((rc = dist_launch_tiles(ctx, d, kp_dist_tree_kernel, min_compared, t.label.p, t.best.p))) return rc;
        hipLaunchKernelGGL(kp_tree_hook_kernel, dim3(grid), dim3(DIST_THREADS), 0, ctx->stream, R, t.label.p, t.best.p, t.parent.p, t.slot.p, t.fresh.p);
        hipLaunchKernelGGL(kp_clust_flatten_kernel, dim3(grid), dim3(DIST_THREADS), 0, ctx->stream, R, 1, t.parent.p, t.label.p);
        KP_HIP_CHECK(ctx, hipGetLastError());
        if ((rc = fetch_all(ctx, ctx->stream, {{&fresh, t.fresh.p, sizeof(uint32_t)}}))) return rc;
        t.rounds = round + 1;
        total += fresh;
    }
    // the bound holds for every matrix (kp_tree_max_rounds); past it the loop does not go round again
    if (fresh != 0) return kp_fail(ctx, KP_ESTATE, "the tree's rounds reached their bound with edges still arriving");
    if (total > (int64_t)R - 1) return kp_fail(ctx, KP_ESTATE, "more tree edges than rows");
    hipLaunchKernelGGL(kp_tree_edge_kernel, dim3(grid), dim3(DIST_THREADS), 0, ctx->stream, d->d_planes.p, R, d->n_words, t.slot.p, t.rec.p);
    KP_HIP_CHECK(ctx, hipGetLastError());
    std::vector<kp_dist_pair> rec((size_t)R);
    KP_HIP_CHECK(ctx, hipMemcpyAsync(rec.data(), t.rec.p, (size_t)R * sizeof(kp_dist_pair), hipMemcpyDeviceToHost, ctx->stream));
    if (component) KP_HIP_CHECK(ctx, hipMemcpyAsync(component, t.label.p, (size_t)R * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    // compact the slots and sort them by key (at most 2^18 records)
    int64_t n = 0;
    for (int32_t r = 0; r < R; ++r)
        if (rec[(size_t)r].a >= 0) rec[(size_t)n++] = rec[(size_t)r];
    if (n != total) return kp_fail(ctx, KP_ESTATE, "the tree's slots do not hold the edges its rounds counted");
    std::sort(rec.begin(), rec.begin() + n, [](const kp_dist_pair &x, const kp_dist_pair &y) {
        return kp_tree_key(x.differences, x.a, x.b) < kp_tree_key(y.differences, y.a, y.b);
    });
    std::copy(rec.begin(), rec.begin() + n, edges);
    *n_edges = n;
    return KP_OK;
}

int32_t kp_dist_tree_rounds(const kp_dist *d) { return d ? d->tree.rounds : 0; }

}  // extern "C"
