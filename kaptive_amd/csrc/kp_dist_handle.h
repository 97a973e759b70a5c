// kp_dist_handle.h -- what the units of the pair reports share: the handle, the tile geometry, the chunk loop of the tile kernels and
// the host helpers of their entry points.  The units: kp_dist.hip (kp_spec.h, DISTANCES), kp_dist_graph.hip (CLUSTERS, TREE),
// kp_dist_sites.hip (SITES), kp_dist_nj.hip (NJ), kp_dist_boot.hip (BOOTSTRAP), kp_dist_transfer.hip (TRANSFER), kp_dist_pars.hip
// (PARSIMONY).  Internal; includes HIP headers.
//
// A handle (kp_dist) holds the bit planes of one matrix of R locus rows of NB blocks -- kp_dist.hip makes them, once -- and the state
// of every report's most recent call, each in a struct of its own that only its unit touches.
//
// A report over pairs is an epilogue and a formatter; the rest is written once: dist_tile_counts (the chunk loop),
// kp_dist_plane_counts (kp_dist.h: one pair recounted), and on the host dist_enter (a call's first checks), dist_grid, DistReserve
// (all tables or the call's refusal), dist_grow (a table that outgrows every one before) and dist_launch_tiles (the tile grid).
//
// Bounds: a lane of the chunk loop reads planes only for r < R and w < NW.
#pragma once

#include <algorithm>
#include <string>
#include <utility>

#include "kp_host.h"
#include "kp_dist.h"
#include "kp_boot.h"

struct kp_dist {
    int device = 0;
    int32_t n_rows = 0;
    int64_t n_blocks = 0, n_words = 0;
    int32_t nt = 0;  // tile rows
    DevBuf<uint64_t> d_planes;  // [KP_DIST_PLANES][n_words][n_rows]
    struct Listing {  // kp_dist_count / kp_dist_pairs: allocated with the handle, but for the records
        DevBuf<uint32_t> cnt;      // [n_rows * nt]
        DevBuf<int64_t> off;       // [n_rows * nt] first record of every entry
        DevBuf<uint32_t> row_cnt;  // [n_rows] listed pairs of every row
        DevBuf<int64_t> row_off;   // [n_rows + 1] their scan
        DevBuf<kp_dist_pair> rec;
        bool counted = false;
        int32_t max_diff = 0, min_compared = 0;
        int64_t n_pairs = 0;
    } list;
    struct Clusters {  // kp_dist_clusters: allocated on its first call, at their largest size
        DevBuf<int32_t> parent;            // [KP_CLUST_MAX_LEVELS][n_rows]
        DevBuf<int32_t> label;             // [KP_CLUST_MAX_LEVELS][n_rows]
        DevBuf<unsigned long long> best;   // [n_rows] nearest keys
        DevBuf<kp_dist_nearest> nearest;   // [n_rows]
    } clust;
    struct Tree {  // kp_dist_tree: allocated on its first call
        DevBuf<int32_t> parent;            // [n_rows]
        DevBuf<int32_t> label;             // [n_rows] the smallest row of every row's component, as of the last round
        DevBuf<unsigned long long> best;   // [n_rows] by label: the component's lightest outgoing edge of this round
        DevBuf<unsigned long long> slot;   // [n_rows] by the root an edge's union moved: the edge's key
        DevBuf<kp_dist_pair> rec;          // [n_rows] the slots as records
        DevBuf<uint32_t> fresh;            // [1] edges of the round
        int32_t rounds = 0;                // rounds of the last kp_dist_tree, the empty one included
    } tree;
    struct Sites {  // kp_dist_profile / kp_dist_sites_count / kp_dist_sites / kp_dist_site_rows: allocated on the first of these calls, but for the site rows
        DevBuf<kp_site> prof;              // [64 * n_words] the profile of every column of the planes
        DevBuf<uint32_t> flag;             // [16 * n_blocks] 1: a site of the last count
        DevBuf<int64_t> off;               // [16 * n_blocks + 1] their scan
        DevBuf<kp_site> rec;               // [16 * n_blocks] the sites of the last count
        DevBuf<uint64_t> rows;             // the site rows of the last kp_dist_site_rows
        bool profiled = false, counted = false;
        int32_t flags = 0;
        int64_t n_sites = 0;
    } sites;
    struct Nj {  // kp_dist_nj: allocated on its first call.  Only these O(n_rows) tables stay: the dense matrix and the picks' partials live for one call
        DevBuf<uint32_t> bases;            // [n_rows] columns that hold a base
        DevBuf<uint32_t> flag;             // [n_rows] 1: a taxon of the last call
        DevBuf<int64_t> off;               // [n_rows + 1] their scan: a taxon's number
        DevBuf<int32_t> taxon;             // [n_rows] a row's taxon number, -1 for none
        DevBuf<int32_t> taxa;              // [n_rows] the rows of the taxa, ascending
        DevBuf<double> sum;                // [n_rows] R of every slot
        DevBuf<int32_t> node;              // [n_rows] the node id of every slot
        DevBuf<int32_t> cell;              // [2] the pair (i, j) of the join under way
        DevBuf<kp_nj_node> rec;            // [n_rows] the records
    } nj;
    struct Boot {  // kp_dist_nj_bootstrap, kp_dist_nj_transfer: allocated on their first call.  Only these O(n_rows) tables stay: the matrices, the weights and every table of a batch live for one call
        DevBuf<KpBootSplit> ref;           // [n_rows] the splits of the tree the call supports, ascending by (size, key)
        DevBuf<int32_t> ref_rec;           // [n_rows] the record of every one of them
        DevBuf<uint32_t> support;          // [n_rows] by record: the replicates that hold its split
        DevBuf<unsigned long long> transfer;  // [n_rows] kp_dist_nj_transfer, by record: the sum of its transfer distances
        DevBuf<uint32_t> exact;            // [n_rows] kp_dist_nj_transfer, by record: the replicates at distance 0
    } boot;
    struct Pars {  // kp_dist_nj_parsimony / kp_dist_pars_sites / kp_dist_pars_changes.  Only the two record lists stay: the node tables, the counters and the scans live for one call
        DevBuf<kp_pars_site> site;         // the sites of the last call
        DevBuf<kp_pars_change> change;     // the changes of the last call
        bool done = false;
        int64_t n_sites = 0, n_changes = 0;
    } pars;
};

// ---- the join loop of kp_dist_nj.hip, for one tree or a batch of them -------------------------------------------------------------------
struct NjBest { double q; int32_t a, b; };  // a pick: the smallest (Q, a, b) seen; nothing seen: (+inf, INT32_MAX, INT32_MAX)
// The tables of the trees one launch joins, tree y (blockIdx.y) a stride behind tree y - 1: its matrix D [n][n], R of its slots and
// their node ids, its records, the partials of its pick; its cell is two entries.  One tree: every stride may be 0.
struct NjBatch {
    double *D, *sum;
    int32_t *node, *cell;
    kp_nj_node *rec;
    NjBest *part;
    int64_t sD;
    int32_t sN, sRec, sPart;  // of sum and node; of rec; of part
};
int dist_nj_taxa(kp_ctx *ctx, kp_dist *d, int32_t min_compared, int32_t *n_taxa);
int32_t dist_nj_parts(int32_t n);  // partials of the picks of a tree of n taxa
int dist_nj_joins(kp_ctx *ctx, const NjBatch &t, int32_t n, int32_t batch, int64_t *n_rec);

// ---- the batch loop of kp_dist_boot.hip, for kp_dist_nj_bootstrap and kp_dist_nj_transfer ---------------------------------------------
// What kp_dist_nj_transfer adds to a bootstrap (kp_spec.h, TRANSFER; kp_dist_transfer.hip): the call's own tables -- the membership
// of the supported tree, O(n) tables of it and the transfer distances of one batch --, freed with the pass.  The batch loop calls
// reserve and begin once, before the first batch, batch after the joins of every batch, and fetch behind the last one.
struct TransferPass {
    int64_t *transfer = nullptr;        // [cap_transfer] the caller's
    int64_t cap_transfer = 0;
    int32_t *per_replicate = nullptr;   // null, or [cap_per]
    int64_t cap_per = 0;
    DevBuf<uint32_t> member;            // [n][MW] bit t % 32 of word t / 32 of row k: taxon k lies in A_t
    DevBuf<uint32_t> turn;              // [MW] bit t: the node of record t holds taxon 0 below it
    DevBuf<int32_t> parent;             // [n + records] the node a node is a child of, -1 for none
    DevBuf<int32_t> size;               // [n - 3] |A_t|
    DevBuf<int32_t> phi;                // [batch][records] the transfer distances of a batch, -1 at a record without an inner edge
    int32_t n = 0, n_rec = 0, S = 0, MW = 0;
    int reserve(kp_ctx *ctx, kp_dist *d, int32_t n_taxa, int32_t batch);
    int begin(kp_ctx *ctx, kp_dist *d, const kp_nj_node *ref_nodes);
    // rec [b][records]: the batch's trees; D: its matrices, sD doubles apart, which the joins are done with
    int batch(kp_ctx *ctx, kp_dist *d, const kp_nj_node *rec, double *D, int64_t sD, int32_t b);
    int fetch(kp_ctx *ctx, kp_dist *d);  // queues the copies of the sums into got_*, for the caller to read behind its synchronisation
    std::vector<unsigned long long> got_transfer;
    std::vector<uint32_t> got_exact;
    void none(int32_t replicates, int64_t n_ref) {  // a tree without an inner edge: -1 everywhere
        for (int64_t t = 0; t < n_ref; ++t) transfer[t] = -1;
        if (per_replicate)
            for (int64_t e = 0; e < (int64_t)replicates * n_ref; ++e) per_replicate[e] = -1;
    }
};
// kp_dist_nj_bootstrap's arguments; `pass` null for it
int dist_boot_run(kp_ctx *ctx, kp_dist *d, int32_t min_compared, uint64_t seed, int32_t replicates, int32_t max_batch, const kp_nj_node *ref_nodes, int64_t n_ref,
                  int32_t *support, int64_t cap_support, kp_nj_node *trees, int64_t cap_trees, TransferPass *pass);

constexpr int DIST_THREADS = 256;
constexpr int T = KP_DIST_TILE, CH = KP_DIST_CHUNK, RG = KP_DIST_REG;
static_assert(T == 64 && RG == 4 && DIST_THREADS == (T / RG) * (T / RG), "a lane per 4 x 4 pairs of a 64 x 64 tile");
static_assert((T / RG) == 16, "the pairs of one row and one j are sixteen neighbouring lanes");
// the largest grid of the pair kernel: HIP launches no grid of 2^32 work items or more in one dimension
constexpr int64_t DIST_MAX_NT = ((int64_t)KP_DIST_MAX_ROWS + T - 1) / T;
static_assert(DIST_MAX_NT * (DIST_MAX_NT + 1) / 2 * DIST_THREADS < (1ll << 32), "KP_DIST_MAX_ROWS: the tiles of the largest matrix must fit one grid dimension");

// The three counts of a lane's 4 x 4 pairs of tile (ti, tj), over all NW plane words: the chunk loop every pair kernel shares.  Ends
// behind a __syncthreads: the strips in `s` are free for the caller.
__device__ __forceinline__ void dist_tile_counts(const uint64_t *__restrict__ planes, int32_t R, int64_t NW, int32_t ti, int32_t tj,
                                                 uint64_t (&s)[2][KP_DIST_PLANES][CH][T], int32_t (&cmp)[RG][RG], int32_t (&dif)[RG][RG],
                                                 int32_t (&uns)[RG][RG]) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
    for (int i = 0; i < RG; ++i)
#pragma unroll
        for (int j = 0; j < RG; ++j) cmp[i][j] = dif[i][j] = uns[i][j] = 0;
    const size_t plane = (size_t)NW * (size_t)R;
    for (int64_t w0 = 0; w0 < NW; w0 += CH) {
        // ---- the chunk of both strips into LDS: entry e = ((strip * 4 + plane) * CH + word) * T + row
        uint64_t *const flat = &s[0][0][0][0];
        for (int e = tid; e < 2 * KP_DIST_PLANES * CH * T; e += DIST_THREADS) {
            const int row = e % T, w = (e / T) % CH, p = (e / (T * CH)) % KP_DIST_PLANES, strip = e / (T * CH * KP_DIST_PLANES);
            const int64_t r = (int64_t)(strip ? tj : ti) * T + row, ww = w0 + w;
            flat[e] = (r < R && ww < NW) ? planes[(size_t)p * plane + (size_t)ww * (size_t)R + (size_t)r] : 0ull;
        }
        __syncthreads();
#pragma unroll 1
        for (int w = 0; w < CH; ++w) {
            uint64_t la[RG], ha[RG], va[RG], pa[RG], lb[RG], hb[RG], vb[RG], pb[RG];
#pragma unroll
            for (int i = 0; i < RG; ++i) {
                la[i] = s[0][0][w][ty + 16 * i]; ha[i] = s[0][1][w][ty + 16 * i]; va[i] = s[0][2][w][ty + 16 * i]; pa[i] = s[0][3][w][ty + 16 * i];
                lb[i] = s[1][0][w][tx + 16 * i]; hb[i] = s[1][1][w][tx + 16 * i]; vb[i] = s[1][2][w][tx + 16 * i]; pb[i] = s[1][3][w][tx + 16 * i];
            }
#pragma unroll
            for (int i = 0; i < RG; ++i)
#pragma unroll
                for (int j = 0; j < RG; ++j)
                    kp_dist_word_counts(la[i], ha[i], va[i], pa[i], lb[j], hb[j], vb[j], pb[j], &cmp[i][j], &dif[i][j], &uns[i][j]);
        }
        __syncthreads();  // (the next chunk overwrites the strips)
    }
}

// The weighted chunk loop (kp_spec.h, BOOTSTRAP): the two weighted counts of a lane's 4 x 4 pairs of tile (ti, tj) under the weight
// planes wplane [KP_BOOT_PLANES][NW] of one replicate, of which the first `top` hold a bit.  The strips hold three planes -- no
// `present`: nothing counts unshared columns here --, 24 KiB.  A pair's v and d are made once per plane word and serve every weight
// plane: two popcounts a plane.  wplane and top are the same for every lane of the workgroup and indexed by nothing a lane owns, so
// the masks are scalar loads and live in scalar registers; `top` picks one of eight unrolled bodies once per chunk, a uniform branch.
// Ends behind a __syncthreads.
constexpr int BOOT_STRIP_PLANES = 3;  // lo, hi, valid
template <int TOP>
__device__ __forceinline__ void dist_chunk_counts_w(const uint64_t (&s)[2][BOOT_STRIP_PLANES][CH][T], const uint64_t *__restrict__ wplane, int64_t NW, int64_t w0,
                                                    int32_t (&cmp)[RG][RG], int32_t (&dif)[RG][RG]) {
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll 1
    for (int w = 0; w < CH; ++w) {
        if (w0 + w >= NW) break;  // (uniform)
        uint64_t M[KP_BOOT_PLANES];
#pragma unroll
        for (int k = 0; k < KP_BOOT_PLANES; ++k) M[k] = k < TOP ? wplane[(size_t)k * (size_t)NW + (size_t)(w0 + w)] : 0ull;
        uint64_t la[RG], ha[RG], va[RG], lb[RG], hb[RG], vb[RG];
#pragma unroll
        for (int i = 0; i < RG; ++i) {
            la[i] = s[0][0][w][ty + 16 * i]; ha[i] = s[0][1][w][ty + 16 * i]; va[i] = s[0][2][w][ty + 16 * i];
            lb[i] = s[1][0][w][tx + 16 * i]; hb[i] = s[1][1][w][tx + 16 * i]; vb[i] = s[1][2][w][tx + 16 * i];
        }
#pragma unroll
        for (int i = 0; i < RG; ++i)
#pragma unroll
            for (int j = 0; j < RG; ++j) kp_boot_word_counts<TOP>(la[i], ha[i], va[i], lb[j], hb[j], vb[j], M, &cmp[i][j], &dif[i][j]);
    }
}
__device__ __forceinline__ void dist_tile_counts_w(const uint64_t *__restrict__ planes, int32_t R, int64_t NW, int32_t ti, int32_t tj,
                                                   const uint64_t *__restrict__ wplane, int top, uint64_t (&s)[2][BOOT_STRIP_PLANES][CH][T],
                                                   int32_t (&cmp)[RG][RG], int32_t (&dif)[RG][RG]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < RG; ++i)
#pragma unroll
        for (int j = 0; j < RG; ++j) cmp[i][j] = dif[i][j] = 0;
    const size_t plane = (size_t)NW * (size_t)R;
    for (int64_t w0 = 0; w0 < NW; w0 += CH) {
        uint64_t *const flat = &s[0][0][0][0];
        for (int e = tid; e < 2 * BOOT_STRIP_PLANES * CH * T; e += DIST_THREADS) {
            const int row = e % T, w = (e / T) % CH, p = (e / (T * CH)) % BOOT_STRIP_PLANES, strip = e / (T * CH * BOOT_STRIP_PLANES);
            const int64_t r = (int64_t)(strip ? tj : ti) * T + row, ww = w0 + w;
            flat[e] = (r < R && ww < NW) ? planes[(size_t)p * plane + (size_t)ww * (size_t)R + (size_t)r] : 0ull;
        }
        __syncthreads();
        switch (top) {  // (uniform: a replicate's highest weight plane)
        case 0: break;
        case 1: dist_chunk_counts_w<1>(s, wplane, NW, w0, cmp, dif); break;
        case 2: dist_chunk_counts_w<2>(s, wplane, NW, w0, cmp, dif); break;
        case 3: dist_chunk_counts_w<3>(s, wplane, NW, w0, cmp, dif); break;
        case 4: dist_chunk_counts_w<4>(s, wplane, NW, w0, cmp, dif); break;
        case 5: dist_chunk_counts_w<5>(s, wplane, NW, w0, cmp, dif); break;
        case 6: dist_chunk_counts_w<6>(s, wplane, NW, w0, cmp, dif); break;
        case 7: dist_chunk_counts_w<7>(s, wplane, NW, w0, cmp, dif); break;
        default: dist_chunk_counts_w<8>(s, wplane, NW, w0, cmp, dif); break;
        }
        __syncthreads();  // (the next chunk overwrites the strips)
    }
}

// ---- what every entry point shares ------------------------------------------------------------------------------------------------
// A call's first checks: the context, the pointers it cannot do without (`args`: the handle and what `nulls` names), the device.
inline int dist_enter(kp_ctx *ctx, const kp_dist *d, bool args, const char *nulls) {
    if (!ctx) return kp_fail(nullptr, KP_EINVAL, "null context");
    if (!d || !args) return kp_fail(ctx, KP_EINVAL, nulls);
    if (d->device != ctx->device) return kp_fail(ctx, KP_EINVAL, "the distance handle belongs to another device");
    return KP_OK;
}

// blocks of a grid-stride kernel over n items, `per` of them to a block of the first round
inline unsigned dist_grid(int64_t n, int per = DIST_THREADS, int64_t most = 1 << 16) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, most)); }

// All of a call's tables or none: the first reserve that fails ends the chain; done() refuses under the call's label, KP_ENOMEM when out of memory.
struct DistReserve {
    hipError_t e = hipSuccess;
    template <class U> DistReserve &operator()(DevBuf<U> &buf, size_t n) { if (e == hipSuccess) e = buf.reserve(n); return *this; }
    int done(kp_ctx *ctx, const char *what) const {
        return e == hipSuccess ? KP_OK : kp_fail(ctx, e == hipErrorOutOfMemory ? KP_ENOMEM : KP_EHIP, std::string(what) + ": " + hipGetErrorString(e));
    }
};

// A table that is larger than every one before takes a buffer of its own size (the listing's records, the site rows): the old buffer
// goes first, then the new one is reserved under the call's label and moved in.  Handle-local growth is not counted by
// kp_device_allocations (kaptive_amd.h says so): that count shows whether a stream of batches has settled
template <class U>
int dist_grow(kp_ctx *ctx, DevBuf<U> &buf, size_t n, const char *what) {
    if (n <= buf.n) return KP_OK;
    DevBuf<U> fresh;
    buf = DevBuf<U>();
    int rc;
    if ((rc = DistReserve()(fresh, n).done(ctx, what))) return rc;
    buf = std::move(fresh);
    return KP_OK;
}

// A tile kernel -- its first parameters are planes, R, NW, nt -- over the tiles on or above the diagonal, one workgroup each.  The
// one place that looks at their number: kp_dist_create admits no matrix whose tiles overflow a grid (DIST_MAX_NT above).
template <class Kernel, class... Args>
int dist_launch_tiles(kp_ctx *ctx, const kp_dist *d, Kernel kernel, Args... args) {
    const int64_t tiles = kp_dist_tiles(d->nt);
    if (tiles <= 0) return KP_OK;
    if (tiles * DIST_THREADS >= (1ll << 32)) return kp_fail(ctx, KP_EINVAL, "too many tiles for one grid (KP_DIST_MAX_ROWS)");
    hipLaunchKernelGGL(kernel, dim3((unsigned)tiles), dim3(DIST_THREADS), 0, ctx->stream, d->d_planes.p, d->n_rows, d->n_words, d->nt, args...);
    KP_HIP_CHECK(ctx, hipGetLastError());
    return KP_OK;
}
