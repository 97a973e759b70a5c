// kp_dist.hip -- pairwise distances between the locus rows of a run (kp_spec.h, DISTANCES; the arithmetic: kp_dist.h).
//
// A handle (kp_dist) holds the bit planes of one matrix of R locus rows of NB blocks, and the listing of its most recent count.
//
//   kp_dist_plane_kernel   once per matrix, one lane per (row, plane word): four blocks -> the words lo, hi, valid, present of
//                          their 64 columns.  Stored plane-major, then word, then row -- planes[(p * NW + w) * R + r] -- so that a
//                          strip of consecutive rows of one word is one coalesced run for the pair kernel.
//   kp_dist_pair_kernel    a GEMM over bits.  One workgroup of 256 lanes owns one 64 x 64 tile of pairs on or above the diagonal
//                          (kp_dist_tile_of: only those are launched); lane (ty, tx) keeps the 4 x 4 pairs of rows ty + 16 i against
//                          rows tx + 16 j with their three int32 counters in registers.  The plane words of the two row strips pass
//                          through LDS KP_DIST_CHUNK words at a time (32 KiB: s[strip][plane][word][row], eight bytes an entry; the
//                          sixteen tx of a wave read sixteen consecutive entries, its four ty one entry each), so a plane word
//                          leaves global memory once per tile.  Rows beyond R and words beyond NW are staged as zeros: invalid and
//                          not present, they count nothing.  No atomics.
//       listing            the same kernel twice.  COUNT: for every row a of the tile and its tile column tj, how many pairs
//                          (a, b) qualify (a < b < R, kp_dist_listed) -> cnt[a * nt + tj]; one workgroup owns the entry.  The
//                          entries in index order ARE the listing's order (ascending a, then b), so their exclusive scan gives
//                          every entry's first record -- in two levels: a wave per row adds the row's entries, the one-block
//                          scan (kp_launch_count_scan) runs over the R row totals, a wave per row spreads its row's prefix.  FILL recomputes the counts and stores the
//                          records: for a fixed (i, j) the sixteen pairs of a row are sixteen neighbouring lanes of one wave -- a
//                          ballot, restricted to those sixteen bits, and mbcnt rank them in ascending b.
//
//   kp_dist_clust_kernel   the same tiles and counts with another epilogue (kp_spec.h, CLUSTERS; kp_clust.h): every valid pair is united
//                          into the parent arrays of its levels by a lock-free union-find and offered to both of its rows as
//                          nearest partner -- reduced inside the tile, then one 64-bit atomic minimum per row and tile.  Around
//                          it kp_clust_init_kernel (identity parents, no partner), kp_clust_flatten_kernel (label = root) and
//                          kp_dist_nearest_kernel (the partner's three counts, recomputed).  No pair is stored.
//
//   kp_dist_tree_kernel    the same tiles and counts with a third epilogue (kp_spec.h, TREE; kp_tree.h): one round of Boruvka.  Every valid
//                          pair whose rows carry different labels offers its packed key to both components -- reduced inside the
//                          tile as the nearest keys are, then one 64-bit atomic minimum per row and tile.  Around it
//                          kp_tree_round_kernel (no edge yet), kp_tree_hook_kernel (one union per component and round; the root
//                          that moved keeps the edge), kp_clust_flatten_kernel (next round's labels) and, after the last round,
//                          kp_tree_edge_kernel (the edges' three counts, recomputed).  No pair is stored.
//
//   kp_sites_profile_kernel  the transposed reduction (kp_spec.h, SITES; kp_sites.h): every column over all rows.  One workgroup of 256
//                          lanes per (plane word, slab of KP_SITES_SLAB rows).  A lane walks KP_SITES_LANE_ROWS rows of the slab, 256
//                          apart -- the rows of one plane word are contiguous, a wave's load is one run --, and adds the five class
//                          masks of each (a, c, g, t, N) into five bit-sliced counters of KP_SITES_PLANES words: no column is
//                          extracted per row.  Six shuffle exchanges per counter plane transpose the wave's 64 x 64 bits
//                          (kp_sites_transpose_step), a popcount gives lane j column j's count; the four waves meet in LDS
//                          (5 KiB), and 320 lanes send one integer atomic add each to the handle's zeroed table of kp_site
//                          records.  Integer adds: the profile is a pure function of the matrix.  Computed once per handle and kept.
//   kp_sites_list_kernel   one lane per column of [0, 16 NB).  COUNT: the site predicate as 0 / 1 -> flag[c], whose exclusive scan
//                          (kp_launch_count_scan) is every site's place: sites ascend in column.  FILL: the records.
//   kp_site_rows_kernel    one lane per (row, block of sixteen sites), rows fastest: it gathers the sixteen sites' bits from the four
//                          planes -- the lanes of a wave read neighbouring rows of one plane word -- and stores one block of the
//                          row's site row; the columns at or beyond S are GAP-flagged.
//
// A report over pairs is an epilogue and a formatter; the rest is written once: dist_tile_counts (the chunk loop), dist_row_min /
// dist_col_min (a key's minimum per row and column of the tile), kp_dist_plane_counts (kp_dist.h: one pair recounted), and on the host
// dist_enter (a call's first checks), dist_grid, DistReserve (all tables or the call's refusal) and dist_launch_tiles (the tile grid).
//
// Bounds: a lane reads planes only for r < R and w < NW, stores cnt only for a < R and tj < nt, and a record only below the total
// the count pass found (the fill recomputes the same flags, so it is the same total).
// Sites: the profile kernel reads planes for r < R and w < NW and adds at records 64 w + j < 64 NW of a table of 64 NW records; the
// list kernel reads records c < 16 NB <= 64 NW, stores flag[c] and a record only below min(off[c] + 1, 16 NB); the row kernel reads
// site records s < S, planes at the record's column -- a c < 16 NB the fill stored, checked again -- and r < R, and stores block
// r * SB + sb < R * SB.
#include <algorithm>
#include <climits>
#include <new>
#include <vector>

#include "kp_host.h"
#include "kp_dist.h"
#include "kp_clust.h"
#include "kp_tree.h"
#include "kp_sites.h"

#ifndef KP_TREE_SKIP
#define KP_TREE_SKIP 1 /* a tile whose rows all carry one label returns before the chunk loop: it holds no outgoing edge */
#endif

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
};

namespace {

constexpr int DIST_THREADS = 256;
constexpr int T = KP_DIST_TILE, CH = KP_DIST_CHUNK, RG = KP_DIST_REG;
static_assert(T == 64 && RG == 4 && DIST_THREADS == (T / RG) * (T / RG), "a lane per 4 x 4 pairs of a 64 x 64 tile");
static_assert((T / RG) == 16, "the pairs of one row and one j are sixteen neighbouring lanes");
// the largest grid of the pair kernel: HIP launches no grid of 2^32 work items or more in one dimension
constexpr int64_t DIST_MAX_NT = ((int64_t)KP_DIST_MAX_ROWS + T - 1) / T;
static_assert(DIST_MAX_NT * (DIST_MAX_NT + 1) / 2 * DIST_THREADS < (1ll << 32), "KP_DIST_MAX_ROWS: the tiles of the largest matrix must fit one grid dimension");

__global__ __launch_bounds__(DIST_THREADS) void kp_dist_plane_kernel(const uint64_t *__restrict__ blocks, int32_t R, int64_t NB, int64_t NW,
                                                                     uint64_t *__restrict__ planes) {
    const int64_t n = (int64_t)R * NW;
    for (int64_t e = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * DIST_THREADS) {
        const int64_t w = e / R, r = e - w * R;
        const KpDistWord q = kp_dist_word_planes(blocks + (size_t)r * (size_t)NB, NB, w);
        const size_t at = (size_t)w * (size_t)R + (size_t)r, plane = (size_t)NW * (size_t)R;
        planes[at] = q.lo; planes[plane + at] = q.hi; planes[2 * plane + at] = q.valid; planes[3 * plane + at] = q.present;
    }
}

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

template <bool FILL>
__global__ __launch_bounds__(DIST_THREADS) void kp_dist_pair_kernel(const uint64_t *__restrict__ planes, int32_t R, int64_t NW, int32_t nt,
                                                                    int32_t max_diff, int32_t min_compared, uint32_t *__restrict__ cnt,
                                                                    const int64_t *__restrict__ off, kp_dist_pair *__restrict__ out, int64_t n_out) {
    __shared__ uint64_t s[2][KP_DIST_PLANES][CH][T];
    int32_t ti, tj;
    kp_dist_tile_of((int64_t)blockIdx.x, nt, &ti, &tj);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    int32_t cmp[RG][RG], dif[RG][RG], uns[RG][RG];
    dist_tile_counts(planes, R, NW, ti, tj, s, cmp, dif, uns);
    // ---- listing: row a = ty + 16 i of the tile; its pairs with b = tx + 16 j ascend in (j, tx)
    const int lane = tid & 63, group = lane >> 4;  // the sixteen lanes of this lane's ty within its wave
    const unsigned long long group_bits = 0xffffull << (16 * group);
#pragma unroll
    for (int i = 0; i < RG; ++i) {
        const int64_t a = (int64_t)ti * T + ty + 16 * i;
        const int64_t entry = a * nt + tj;
        int before = 0;  // qualifying pairs of row a in this tile with a smaller j
        int64_t first = 0;
        if (FILL && a < R) first = off[entry];
#pragma unroll
        for (int j = 0; j < RG; ++j) {
            const int64_t b = (int64_t)tj * T + tx + 16 * j;
            const bool q = a < R && b < R && a < b && kp_dist_listed(cmp[i][j], dif[i][j], max_diff, min_compared);
            const unsigned long long mine = __ballot(q) & group_bits;
            if (FILL && q) {
                const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mine >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mine, 0u));
                const int64_t at = first + before + rank;
                if (at < n_out) kp_dist_pair_store(out + at, (int32_t)a, (int32_t)b, cmp[i][j], dif[i][j], uns[i][j]);
            }
            before += __popcll(mine);
        }
        if (!FILL && tx == 0 && a < R) cnt[entry] = (uint32_t)before;
    }
}

// ---- the scan of the count table, in two levels (one block over all R x nt entries would be the longest step after the pair kernel) ----
constexpr int DIST_WAVES = DIST_THREADS / 64;

// row_cnt[a] = the listed pairs of row a: a wave per row adds its nt entries (at most R - 1 < 2^18)
__global__ __launch_bounds__(DIST_THREADS) void kp_dist_row_sum_kernel(const uint32_t *__restrict__ cnt, int32_t R, int32_t nt, uint32_t *__restrict__ row_cnt) {
    const int lane = threadIdx.x & 63;
    for (int64_t a = (int64_t)blockIdx.x * DIST_WAVES + threadIdx.x / 64; a < R; a += (int64_t)gridDim.x * DIST_WAVES) {
        uint32_t sum = 0;
        for (int t = lane; t < nt; t += 64) sum += cnt[a * nt + t];
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) row_cnt[a] = sum;
    }
}

// off[a * nt + t] = row_off[a] + the entries of row a before t: a wave per row, 64 entries a round, the carry wave-uniform
__global__ __launch_bounds__(DIST_THREADS) void kp_dist_row_scan_kernel(const uint32_t *__restrict__ cnt, const int64_t *__restrict__ row_off, int32_t R,
                                                                        int32_t nt, int64_t *__restrict__ off) {
    const int lane = threadIdx.x & 63;
    for (int64_t a = (int64_t)blockIdx.x * DIST_WAVES + threadIdx.x / 64; a < R; a += (int64_t)gridDim.x * DIST_WAVES) {
        int64_t carry = row_off[a];
        for (int t0 = 0; t0 < nt; t0 += 64) {  // (t0 and nt are the same in every lane: the shuffles below see the whole wave)
            const int t = t0 + lane;
            const uint32_t c = t < nt ? cnt[a * nt + t] : 0u;
            uint32_t incl = c;
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t u = __shfl_up(incl, o);
                if (lane >= o) incl += u;
            }
            if (t < nt) off[a * nt + t] = carry + (int64_t)(incl - c);
            carry += (int64_t)__shfl(incl, 63);
        }
    }
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

// ---- variable sites (kp_spec.h, SITES; the arithmetic: kp_sites.h) ------------------------------------------------------------------
constexpr int SITES_THREADS = KP_SITES_THREADS, SITES_WAVES = SITES_THREADS / 64;
static_assert(SITES_THREADS % 64 == 0 && KP_SITES_SLAB == SITES_THREADS * KP_SITES_LANE_ROWS, "a slab is every lane's full share of rows");
static_assert(KP_SITES_CLASSES * 64 <= 2 * SITES_THREADS, "the slab's sums leave in two rounds of the workgroup at most");

// prof[c] = (c; 0, 0, 0, 0; 0) for every column of the planes
__global__ __launch_bounds__(DIST_THREADS) void kp_sites_zero_kernel(int64_t n_cols, kp_site *__restrict__ prof) {
    for (int64_t c = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; c < n_cols; c += (int64_t)gridDim.x * DIST_THREADS) kp_site_store(prof + c, (int32_t)c, 0, 0, 0, 0, 0);
}

// One workgroup per unit u = (plane word w, slab): prof[64 w + j].(n[0..3], n_n) += the rows of the slab that hold class k at column j.
// Bounds: w = u / n_slabs < NW; a row is read only for r < R; LDS at [wave < 4][k < 5][lane < 64]; the adds go to records
// 64 w + j, j < 64, of a table of 64 NW records, at the five int32 behind `column`.
__global__ __launch_bounds__(SITES_THREADS) void kp_sites_profile_kernel(const uint64_t *__restrict__ planes, int32_t R, int64_t NW, int64_t n_slabs,
                                                                         kp_site *__restrict__ prof) {
    __shared__ int32_t s_cnt[SITES_WAVES][KP_SITES_CLASSES][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t plane = (size_t)NW * (size_t)R;
    for (int64_t u = blockIdx.x; u < NW * n_slabs; u += gridDim.x) {  // (u and the bounds are the same in every lane: the shuffles below see whole waves)
        const int64_t w = u / n_slabs, slab = u - w * n_slabs;
        const uint64_t *at = planes + (size_t)w * (size_t)R;
        KpSiteCounter cnt[KP_SITES_CLASSES];
#pragma unroll
        for (int k = 0; k < KP_SITES_CLASSES; ++k)
#pragma unroll
            for (int b = 0; b < KP_SITES_PLANES; ++b) cnt[k].p[b] = 0;
#pragma unroll
        for (int i = 0; i < KP_SITES_LANE_ROWS; ++i) {  // at most 2^P - 1 adds: no counter carries out
            const int64_t r = slab * KP_SITES_SLAB + (int64_t)i * SITES_THREADS + tid;
            if (r < R) {
                const KpSiteMasks q = kp_sites_masks(at[r], at[plane + r], at[2 * plane + r], at[3 * plane + r]);
#pragma unroll
                for (int k = 0; k < KP_SITES_CLASSES; ++k) kp_sites_counter_add(&cnt[k], q.m[k]);
            }
        }
        // the wave's 64 counters of column j -> lane j
#pragma unroll
        for (int k = 0; k < KP_SITES_CLASSES; ++k) {
            int32_t sum = 0;
#pragma unroll
            for (int b = 0; b < KP_SITES_PLANES; ++b) {
                uint64_t x = cnt[k].p[b];
#pragma unroll
                for (int s = 32; s >= 1; s >>= 1) x = kp_sites_transpose_step(x, (uint64_t)__shfl_xor((unsigned long long)x, s), lane, s);
                sum += __popcll(x) << b;
            }
            s_cnt[wave][k][lane] = sum;
        }
        __syncthreads();
        for (int e = tid; e < KP_SITES_CLASSES * 64; e += SITES_THREADS) {
            const int j = e / KP_SITES_CLASSES, k = e - j * KP_SITES_CLASSES;
            int32_t sum = 0;
#pragma unroll
            for (int v = 0; v < SITES_WAVES; ++v) sum += s_cnt[v][k][j];
            if (sum) atomicAdd(reinterpret_cast<int32_t *>(prof + (w * 64 + j)) + 1 + k, sum);
        }
        __syncthreads();  // (the next unit overwrites s_cnt)
    }
}

// One lane per column of [0, n_cols = 16 NB).  COUNT: flag[c] = the column is a site.  FILL: a site's record at off[c], the place the
// scan of the flags gave it.
template <bool FILL>
__global__ __launch_bounds__(DIST_THREADS) void kp_sites_list_kernel(const kp_site *__restrict__ prof, int64_t n_cols, int32_t R, int32_t flags,
                                                                     uint32_t *__restrict__ flag, const int64_t *__restrict__ off, kp_site *__restrict__ out, int64_t n_out) {
    for (int64_t c = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; c < n_cols; c += (int64_t)gridDim.x * DIST_THREADS) {
        const kp_site p = prof[c];
        const bool is = kp_site_is(p.n, p.n_n, R, flags);
        if (!FILL) flag[c] = is ? 1u : 0u;
        if (FILL && is) {
            const int64_t at = off[c];
            if (at >= 0 && at < n_out) kp_site_store(out + at, (int32_t)c, p.n[0], p.n[1], p.n[2], p.n[3], p.n_n);
        }
    }
}

// One lane per (row r, block sb of the site row), rows fastest: the codes of sites 16 sb .. 16 sb + 15 of row r.
__global__ __launch_bounds__(DIST_THREADS) void kp_site_rows_kernel(const uint64_t *__restrict__ planes, int32_t R, int64_t NW, const kp_site *__restrict__ sites,
                                                                    int64_t S, int64_t SB, uint64_t *__restrict__ out) {
    const int64_t n = (int64_t)R * SB;
    const size_t plane = (size_t)NW * (size_t)R;
    for (int64_t e = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * DIST_THREADS) {
        const int64_t sb = e / R, r = e - sb * R;
        uint64_t v = 0;
#pragma unroll 4
        for (int k = 0; k < KP_SITES_BLOCK; ++k) {
            const int64_t s = sb * KP_SITES_BLOCK + k;
            const int64_t c = s < S ? (int64_t)sites[s].column : -1;
            if (c < 0 || c >= 64 * NW) {  // beyond S: padding (and no column the fill stores)
                v |= 1ull << (KP_DIST_GAP_SHIFT + k);
                continue;
            }
            const size_t at = (size_t)(c >> 6) * (size_t)R + (size_t)r;
            const int bit = (int)(c & 63);
            v |= kp_site_block_code(k, planes[at] >> bit, planes[plane + at] >> bit, planes[2 * plane + at] >> bit, planes[3 * plane + at] >> bit);
        }
        out[(size_t)r * (size_t)SB + (size_t)sb] = v;
    }
}

// ---- what every entry point shares ------------------------------------------------------------------------------------------------
// A call's first checks: the context, the pointers it cannot do without (`args`: the handle and what `nulls` names), the device.
int dist_enter(kp_ctx *ctx, const kp_dist *d, bool args, const char *nulls) {
    if (!ctx) return kp_fail(nullptr, KP_EINVAL, "null context");
    if (!d || !args) return kp_fail(ctx, KP_EINVAL, nulls);
    if (d->device != ctx->device) return kp_fail(ctx, KP_EINVAL, "the distance handle belongs to another device");
    return KP_OK;
}

// blocks of a grid-stride kernel over n items, `per` of them to a block of the first round
unsigned dist_grid(int64_t n, int per = DIST_THREADS, int64_t most = 1 << 16) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + per - 1) / per, most)); }

// All of a call's tables or none: the first reserve that fails ends the chain; done() refuses under the call's label, KP_ENOMEM when out of memory.
struct DistReserve {
    hipError_t e = hipSuccess;
    template <class U> DistReserve &operator()(DevBuf<U> &buf, size_t n) { if (e == hipSuccess) e = buf.reserve(n); return *this; }
    int done(kp_ctx *ctx, const char *what) const {
        return e == hipSuccess ? KP_OK : kp_fail(ctx, e == hipErrorOutOfMemory ? KP_ENOMEM : KP_EHIP, std::string(what) + ": " + hipGetErrorString(e));
    }
};

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

}  // namespace

extern "C" {

int kp_dist_create(kp_ctx *ctx, const uint64_t *blocks, int32_t n_rows, int64_t n_blocks, kp_dist **out) {
    if (!ctx) return kp_fail(nullptr, KP_EINVAL, "null context");
    if (!out) return kp_fail(ctx, KP_EINVAL, "null handle pointer");
    *out = nullptr;
    if (n_rows < 0) return kp_fail(ctx, KP_EINVAL, "negative number of locus rows");
    if (n_rows > KP_DIST_MAX_ROWS) return kp_fail(ctx, KP_EINVAL, "too many locus rows (KP_DIST_MAX_ROWS)");
    if (n_rows > 0 && n_blocks <= 0) return kp_fail(ctx, KP_EINVAL, "locus rows need at least one block");
    if (n_blocks < 0) n_blocks = 0;
    if (n_blocks >= (1ll << 31) / 16) return kp_fail(ctx, KP_EINVAL, "a locus of 2^31 columns or more: the counts are int32");
    if (n_rows > 0 && !blocks) return kp_fail(ctx, KP_EINVAL, "null block matrix");
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    kp_dist *d = new (std::nothrow) kp_dist();
    if (!d) return kp_fail(ctx, KP_ENOMEM, "out of host memory");
    std::unique_ptr<kp_dist> hold(d);
    d->device = ctx->device;
    d->n_rows = n_rows;
    d->n_blocks = n_rows > 0 ? n_blocks : 0;
    d->n_words = kp_dist_words(d->n_blocks);
    d->nt = (int32_t)(((int64_t)n_rows + T - 1) / T);
    if (n_rows > 0) {
        const size_t n = (size_t)n_rows * (size_t)d->n_words;
        DevBuf<uint64_t> d_blocks;  // only the planes stay
        int rc;
        if ((rc = upload(ctx, d_blocks, blocks, (size_t)n_rows * (size_t)n_blocks))) return rc;
        const size_t entries = (size_t)n_rows * (size_t)d->nt;
        if ((rc = DistReserve()(d->d_planes, KP_DIST_PLANES * n)(d->list.cnt, entries)(d->list.off, entries)(d->list.row_cnt, (size_t)n_rows)(
                      d->list.row_off, (size_t)n_rows + 1).done(ctx, "distance planes")))
            return rc;
        hipLaunchKernelGGL(kp_dist_plane_kernel, dim3(dist_grid((int64_t)n)), dim3(DIST_THREADS), 0, ctx->stream, d_blocks.p, n_rows, n_blocks, d->n_words, d->d_planes.p);
        KP_HIP_CHECK(ctx, hipGetLastError());
        KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (d_blocks goes away here)
    }
    *out = hold.release();
    return KP_OK;
}

int kp_dist_count(kp_ctx *ctx, kp_dist *d, int32_t max_diff, int32_t min_compared, int64_t *n_pairs) {
    int rc;
    if ((rc = dist_enter(ctx, d, n_pairs, "null distance handle or count pointer"))) return rc;
    kp_dist::Listing &l = d->list;
    l.counted = false;
    l.max_diff = max_diff; l.min_compared = min_compared; l.n_pairs = 0;
    if (d->n_rows > 1) {
        KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        const int64_t entries = (int64_t)d->n_rows * d->nt;
        // (the entries of tile columns left of the diagonal belong to no workgroup: they stay zero)
        KP_HIP_CHECK(ctx, hipMemsetAsync(l.cnt.p, 0, (size_t)entries * sizeof(uint32_t), ctx->stream));
        if ((rc = dist_launch_tiles(ctx, d, kp_dist_pair_kernel<false>, max_diff, min_compared, l.cnt.p, l.off.p, (kp_dist_pair *)nullptr, (int64_t)0))) return rc;
        const unsigned grid = dist_grid(d->n_rows, DIST_WAVES, 4096);
        hipLaunchKernelGGL(kp_dist_row_sum_kernel, dim3(grid), dim3(DIST_THREADS), 0, ctx->stream, l.cnt.p, d->n_rows, d->nt, l.row_cnt.p);
        kp_launch_count_scan(l.row_cnt.p, d->n_rows, l.row_off.p, ctx->stream);
        hipLaunchKernelGGL(kp_dist_row_scan_kernel, dim3(grid), dim3(DIST_THREADS), 0, ctx->stream, l.cnt.p, l.row_off.p, d->n_rows, d->nt, l.off.p);
        KP_HIP_CHECK(ctx, hipGetLastError());
        if ((rc = fetch_all(ctx, ctx->stream, {{&l.n_pairs, l.row_off.p + d->n_rows, sizeof(int64_t)}}))) return rc;
    }
    l.counted = true;
    *n_pairs = l.n_pairs;
    return KP_OK;
}

int kp_dist_pairs(kp_ctx *ctx, kp_dist *d, kp_dist_pair *out, int64_t cap) {
    int rc;
    if ((rc = dist_enter(ctx, d, true, "null distance handle"))) return rc;
    kp_dist::Listing &l = d->list;
    if (!l.counted) return kp_fail(ctx, KP_ESTATE, "kp_dist_count must come first");
    if (cap < l.n_pairs || (l.n_pairs > 0 && !out)) return kp_fail(ctx, KP_EINVAL, "room for fewer pairs than kp_dist_count counted");
    if (l.n_pairs == 0) return KP_OK;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if ((size_t)l.n_pairs > l.rec.n) {
        // a longer listing than every one before takes a buffer of its own size.  Handle-local growth is not counted by
        // kp_device_allocations (kaptive_amd.h says so): that count shows whether a stream of batches has settled
        DevBuf<kp_dist_pair> fresh;
        l.rec = DevBuf<kp_dist_pair>();
        if ((rc = DistReserve()(fresh, (size_t)l.n_pairs).done(ctx, "distance records"))) return rc;
        l.rec = std::move(fresh);
    }
    if ((rc = dist_launch_tiles(ctx, d, kp_dist_pair_kernel<true>, l.max_diff, l.min_compared, l.cnt.p, l.off.p, l.rec.p, l.n_pairs))) return rc;
    KP_HIP_CHECK(ctx, hipMemcpyAsync(out, l.rec.p, (size_t)l.n_pairs * sizeof(kp_dist_pair), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return KP_OK;
}

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

// The handle's profile: made by the first call that needs it and kept -- the planes never change.
static int sites_profile(kp_ctx *ctx, kp_dist *d) {
    kp_dist::Sites &s = d->sites;
    if (s.profiled) return KP_OK;
    const int64_t n_cols = 64 * d->n_words, cols = 16 * d->n_blocks;
    int rc;
    if ((rc = DistReserve()(s.prof, (size_t)n_cols)(s.flag, (size_t)cols)(s.off, (size_t)cols + 1)(s.rec, (size_t)cols).done(ctx, "site tables"))) return rc;
    if (n_cols > 0) {
        hipLaunchKernelGGL(kp_sites_zero_kernel, dim3(dist_grid(n_cols)), dim3(DIST_THREADS), 0, ctx->stream, n_cols, s.prof.p);
        const int64_t n_slabs = ((int64_t)d->n_rows + KP_SITES_SLAB - 1) / KP_SITES_SLAB;
        if (n_slabs > 0)
            hipLaunchKernelGGL(kp_sites_profile_kernel, dim3(dist_grid(d->n_words * n_slabs, 1, 1 << 20)), dim3(SITES_THREADS), 0, ctx->stream, d->d_planes.p, d->n_rows,
                               d->n_words, n_slabs, s.prof.p);
        KP_HIP_CHECK(ctx, hipGetLastError());
    }
    s.profiled = true;
    return KP_OK;
}

int kp_dist_profile(kp_ctx *ctx, kp_dist *d, kp_site *out, int64_t cap) {
    int rc;
    if ((rc = dist_enter(ctx, d, true, "null distance handle"))) return rc;
    const int64_t cols = 16 * d->n_blocks;
    if (cap < cols || (cols > 0 && !out)) return kp_fail(ctx, KP_EINVAL, "room for fewer records than the matrix has columns (16 * n_blocks)");
    if (cols == 0) return KP_OK;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if ((rc = sites_profile(ctx, d))) return rc;
    KP_HIP_CHECK(ctx, hipMemcpyAsync(out, d->sites.prof.p, (size_t)cols * sizeof(kp_site), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return KP_OK;
}

int kp_dist_sites_count(kp_ctx *ctx, kp_dist *d, int32_t flags, int64_t *n_sites) {
    int rc;
    if ((rc = dist_enter(ctx, d, n_sites, "null distance handle or count pointer"))) return rc;
    if (flags & ~KP_SITES_FLAGS) return kp_fail(ctx, KP_EINVAL, "unknown site flags");
    kp_dist::Sites &s = d->sites;
    s.counted = false;
    s.flags = flags; s.n_sites = 0;
    const int64_t cols = 16 * d->n_blocks;
    if (d->n_rows > 1 && cols > 0) {  // (one row differs from nobody)
        KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
        if ((rc = sites_profile(ctx, d))) return rc;
        const unsigned grid = dist_grid(cols);
        hipLaunchKernelGGL(kp_sites_list_kernel<false>, dim3(grid), dim3(DIST_THREADS), 0, ctx->stream, s.prof.p, cols, d->n_rows, flags, s.flag.p, s.off.p, s.rec.p, cols);
        kp_launch_count_scan(s.flag.p, cols, s.off.p, ctx->stream);
        // (the records at once: there are at most `cols` of them, and kp_dist_site_rows reads them on the device)
        hipLaunchKernelGGL(kp_sites_list_kernel<true>, dim3(grid), dim3(DIST_THREADS), 0, ctx->stream, s.prof.p, cols, d->n_rows, flags, s.flag.p, s.off.p, s.rec.p, cols);
        KP_HIP_CHECK(ctx, hipGetLastError());
        if ((rc = fetch_all(ctx, ctx->stream, {{&s.n_sites, s.off.p + cols, sizeof(int64_t)}}))) return rc;
        if (s.n_sites < 0 || s.n_sites > cols) return kp_fail(ctx, KP_ESTATE, "more sites than columns");
    }
    s.counted = true;
    *n_sites = s.n_sites;
    return KP_OK;
}

int kp_dist_sites(kp_ctx *ctx, kp_dist *d, kp_site *out, int64_t cap) {
    int rc;
    if ((rc = dist_enter(ctx, d, true, "null distance handle"))) return rc;
    const kp_dist::Sites &s = d->sites;
    if (!s.counted) return kp_fail(ctx, KP_ESTATE, "kp_dist_sites_count must come first");
    if (cap < s.n_sites || (s.n_sites > 0 && !out)) return kp_fail(ctx, KP_EINVAL, "room for fewer sites than kp_dist_sites_count counted");
    if (s.n_sites == 0) return KP_OK;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    KP_HIP_CHECK(ctx, hipMemcpyAsync(out, s.rec.p, (size_t)s.n_sites * sizeof(kp_site), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return KP_OK;
}

int kp_dist_site_rows(kp_ctx *ctx, kp_dist *d, uint64_t *blocks, int64_t cap_blocks) {
    int rc;
    if ((rc = dist_enter(ctx, d, true, "null distance handle"))) return rc;
    kp_dist::Sites &s = d->sites;
    if (!s.counted) return kp_fail(ctx, KP_ESTATE, "kp_dist_sites_count must come first");
    const int64_t SB = kp_site_row_blocks(s.n_sites), need = (int64_t)d->n_rows * SB;
    if (cap_blocks < need || (need > 0 && !blocks)) return kp_fail(ctx, KP_EINVAL, "room for fewer blocks than the site rows have (n_rows * ((n_sites + 15) / 16))");
    if (need == 0) return KP_OK;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if ((size_t)need > s.rows.n) {  // as the listing's records: a larger table than every one before takes a buffer of its own size
        DevBuf<uint64_t> fresh;
        s.rows = DevBuf<uint64_t>();
        if ((rc = DistReserve()(fresh, (size_t)need).done(ctx, "site rows"))) return rc;
        s.rows = std::move(fresh);
    }
    hipLaunchKernelGGL(kp_site_rows_kernel, dim3(dist_grid(need)), dim3(DIST_THREADS), 0, ctx->stream, d->d_planes.p, d->n_rows, d->n_words, s.rec.p, s.n_sites, SB, s.rows.p);
    KP_HIP_CHECK(ctx, hipGetLastError());
    KP_HIP_CHECK(ctx, hipMemcpyAsync(blocks, s.rows.p, (size_t)need * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return KP_OK;
}

void kp_dist_destroy(kp_dist *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    delete d;
}

}  // extern "C"
