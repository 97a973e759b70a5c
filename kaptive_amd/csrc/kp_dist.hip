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
//   kp_dist_nj_kernel      the same tiles and counts with a fourth epilogue (kp_spec.h, NJ; kp_nj.h): every pair of taxa stores its
//                          p-distance, one correctly rounded division, into both triangles of a dense n x n matrix of doubles.
//                          Before it kp_nj_bases_kernel (a row's bases: popcounts of its `valid` plane, integer adds),
//                          kp_nj_flag_kernel and kp_nj_number_kernel around the one-block scan (the taxa, numbered); behind it
//                          kp_nj_init_kernel (R of every slot: SUM64, a wave per row) and, per join, four launches the host
//                          enqueues without a look at the device: kp_nj_pick_kernel (the smallest (Q, a, b) of a workgroup's rows
//                          of the triangle), kp_nj_join_kernel (one workgroup: the smallest partial is the pair; the record; the
//                          pair into a device cell), kp_nj_update_kernel (u_k into row i and column i, R_k) and kp_nj_move_kernel
//                          (slot m - 1 into slot j, R_i by SUM64); kp_nj_end_kernel writes the last record.  The slots stay dense,
//                          so the pick is a plain triangular scan.  The matrix lives for one call.
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
#include "kp_nj.h"

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

// ---- neighbour joining (kp_spec.h, NJ; the arithmetic: kp_nj.h) ---------------------------------------------------------------------
// The state of the join loop: the dense matrix D of the taxa, n x n doubles, row-major with the row stride n throughout -- the m
// live slots are its first m rows and columns --, R of every slot (`sum`), the node id of every slot, and the pair of the join under
// way in a device cell: the host enqueues every join of a tree without looking at one.
// Bounds: D is read and written at [slot < m][slot < m], m <= n; sum and node at slots < m; part at blockIdx.x < its grid, which the
// host keeps at NJ_MAX_PARTS or less; rec at the record index the host passes, below kp_nj_records(n) <= n_rows.  A pair the cell
// holds is used only when 0 <= i < j < m.
constexpr int NJ_THREADS = 256, NJ_WAVES = NJ_THREADS / 64, NJ_MAX_PARTS = 1024;
static_assert(KP_NJ_LANES == 64, "SUM64 is one wavefront's reduction");

struct NjBest { double q; int32_t a, b; };  // a pick: the smallest (Q, a, b) seen; nothing seen: (+inf, INT32_MAX, INT32_MAX)

__device__ __forceinline__ NjBest nj_none() { return NjBest{__builtin_inf(), INT32_MAX, INT32_MAX}; }
__device__ __forceinline__ NjBest nj_better(const NjBest &x, const NjBest &y) { return kp_nj_less(y.q, y.a, y.b, x.q, x.a, x.b) ? y : x; }
// the wave's best in every lane
__device__ __forceinline__ NjBest nj_wave_best(NjBest x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = nj_better(x, NjBest{__shfl_xor(x.q, o), __shfl_xor(x.a, o), __shfl_xor(x.b, o)});
    return x;
}
// the workgroup's best, in thread 0 (s: a slot per wave)
__device__ __forceinline__ NjBest nj_block_best(NjBest x, NjBest (&s)[NJ_WAVES]) {
    x = nj_wave_best(x);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int v = 1; v < NJ_WAVES; ++v) x = nj_better(x, s[v]);
    return x;
}
// SUM64 by one whole wave: `mine` is the lane's strided left fold S_l; the xor shuffles are the halving adds (lanes l and l ^ o hold
// the same sum after the step of o, so lane l < o adds exactly S_{l+o})
__device__ __forceinline__ double nj_wave_sum64(double mine) {
    KP_NJ_EXACT
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mine = mine + __shfl_xor(mine, o);
    return mine;
}

// A lane's strided left fold S_lane of SUM64 over the entries c < m of a row, entry `swap` read from `from` instead (-1: none).  Eight
// loads are in flight before the first of their adds; the adds keep their order.
__device__ __forceinline__ double nj_lane_fold(const double *__restrict__ row, int32_t m, int lane, int32_t swap, int32_t from) {
    KP_NJ_EXACT
    constexpr int AHEAD = 8;
    double mine = 0.0;
    for (int32_t c0 = lane; c0 < m; c0 += 64 * AHEAD) {
        double v[AHEAD];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int32_t c = c0 + 64 * u;
            v[u] = c < m ? row[c == swap ? from : c] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < AHEAD; ++u)
            if (c0 + 64 * u < m) mine = mine + v[u];
    }
    return mine;
}

// bases[r] += the bases of plane word w of row r: one lane per (word, row), rows fastest.  Integer adds into a zeroed table.
__global__ __launch_bounds__(DIST_THREADS) void kp_nj_bases_kernel(const uint64_t *__restrict__ planes, int32_t R, int64_t NW, uint32_t *__restrict__ bases) {
    const int64_t n = (int64_t)R * NW;
    const uint64_t *valid = planes + 2 * (size_t)NW * (size_t)R;
    for (int64_t e = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; e < n; e += (int64_t)gridDim.x * DIST_THREADS) {
        const uint32_t c = (uint32_t)__popcll(valid[e]);  // (e = w * R + r)
        if (c) atomicAdd(bases + (e % R), c);
    }
}
// flag[r] = row r is a taxon
__global__ __launch_bounds__(DIST_THREADS) void kp_nj_flag_kernel(const uint32_t *__restrict__ bases, int32_t R, int64_t W, int32_t min_compared, uint32_t *__restrict__ flag) {
    for (int64_t r = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; r < R; r += (int64_t)gridDim.x * DIST_THREADS) flag[r] = kp_nj_taxon(bases[r], W, min_compared) ? 1u : 0u;
}
// the scan of the flags numbers the taxa: taxon[r] = row r's number or -1, taxa[number] = r
__global__ __launch_bounds__(DIST_THREADS) void kp_nj_number_kernel(const uint32_t *__restrict__ flag, const int64_t *__restrict__ off, int32_t R, int32_t *__restrict__ taxon,
                                                                    int32_t *__restrict__ taxa) {
    for (int64_t r = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x; r < R; r += (int64_t)gridDim.x * DIST_THREADS) {
        const int64_t at = off[r];
        const bool is = flag[r] != 0 && at >= 0 && at < R;
        taxon[r] = is ? (int32_t)at : -1;
        if (is) taxa[at] = (int32_t)r;
    }
}

// The pair kernel's tiles and counts with a fourth epilogue: every pair of taxa of the tile stores its distance into both triangles
// of the dense matrix, a diagonal tile the zeros of its taxa's diagonal entries -- together every entry of D.
// Bounds: taxon is read at rows < R; its values are -1 or numbers below n (kp_nj_number_kernel), and index D [n][n].
__global__ __launch_bounds__(DIST_THREADS) void kp_dist_nj_kernel(const uint64_t *__restrict__ planes, int32_t R, int64_t NW, int32_t nt,
                                                                  const int32_t *__restrict__ taxon, int32_t n, double *__restrict__ D) {
    __shared__ uint64_t s[2][KP_DIST_PLANES][CH][T];
    int32_t ti, tj;
    kp_dist_tile_of((int64_t)blockIdx.x, nt, &ti, &tj);
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    int32_t cmp[RG][RG], dif[RG][RG], uns[RG][RG];
    dist_tile_counts(planes, R, NW, ti, tj, s, cmp, dif, uns);
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

// The initial state: a wave per slot k < n: sum[k] = SUM64 of row k, node[k] = k.
__global__ __launch_bounds__(NJ_THREADS) void kp_nj_init_kernel(const double *__restrict__ D, int32_t n, double *__restrict__ sum, int32_t *__restrict__ node) {
    const int lane = threadIdx.x & 63;
    for (int64_t k = (int64_t)blockIdx.x * NJ_WAVES + threadIdx.x / 64; k < n; k += (int64_t)gridDim.x * NJ_WAVES) {  // (k is the same in every lane of a wave)
        const double mine = nj_wave_sum64(nj_lane_fold(D + (size_t)k * (size_t)n, n, lane, -1, -1));
        if (lane == 0) { sum[k] = mine; node[k] = (int32_t)k; }
    }
}

// A join's pick, first step: workgroup g scans the rows a = g, g + grid, .. of the triangle a < b < m -- a row is one coalesced run
// -- and leaves the smallest (Q, a, b) it met in part[g].
__global__ __launch_bounds__(NJ_THREADS) void kp_nj_pick_kernel(const double *__restrict__ D, int32_t n, int32_t m, const double *__restrict__ sum, NjBest *__restrict__ part) {
    __shared__ NjBest s_best[NJ_WAVES];
    const double f = (double)(m - 2);
    NjBest best = nj_none();
    for (int32_t a = (int32_t)blockIdx.x; a < m - 1; a += (int32_t)gridDim.x) {
        const double *row = D + (size_t)a * (size_t)n;
        const double ra = sum[a];
        for (int32_t b = a + 1 + (int32_t)threadIdx.x; b < m; b += NJ_THREADS) {
            const double q = kp_nj_q(f, row[b], ra, sum[b]);
            if (kp_nj_less(q, a, b, best.q, best.a, best.b)) best = NjBest{q, a, b};
        }
    }
    best = nj_block_best(best, s_best);
    if (threadIdx.x == 0) part[blockIdx.x] = best;
}

// Second step, one workgroup: the smallest of the partials is the pair (i, j).  It writes the join's record, makes slot i the new
// node and publishes the pair; a pair that is none (no matrix gives one) is published as (-1, -1) and recorded as (-1, -1, -1).
__global__ __launch_bounds__(NJ_THREADS) void kp_nj_join_kernel(const NjBest *__restrict__ part, int32_t n_parts, const double *__restrict__ D, int32_t n, int32_t m,
                                                                const double *__restrict__ sum, int32_t *__restrict__ node, int32_t *__restrict__ cell,
                                                                kp_nj_node *__restrict__ rec, int32_t at, int32_t new_id) {
    __shared__ NjBest s_best[NJ_WAVES];
    NjBest best = nj_none();
    for (int32_t p = (int32_t)threadIdx.x; p < n_parts; p += NJ_THREADS) best = nj_better(best, part[p]);
    best = nj_block_best(best, s_best);
    if (threadIdx.x != 0) return;
    const int32_t i = best.a, j = best.b;
    if (i < 0 || j <= i || j >= m) {
        cell[0] = cell[1] = -1;
        kp_nj_node_store(rec + at, -1, -1, -1, 0.0, 0.0, 0.0);
        return;
    }
    double li, lj;
    kp_nj_lengths(D[(size_t)i * (size_t)n + (size_t)j], sum[i], sum[j], (double)(m - 2), &li, &lj);
    kp_nj_node_store(rec + at, node[i], node[j], -1, li, lj, 0.0);
    node[i] = new_id;
    cell[0] = i; cell[1] = j;
}

// Third step, one lane per slot k other than i, j: u_k into row i and column i, R_k.  No lane reads what another writes: lane k
// reads d(i, k), d(j, k) and R_k and writes d(i, k), d(k, i) and R_k; d(i, j) is read by all and written by none.
__global__ __launch_bounds__(NJ_THREADS) void kp_nj_update_kernel(double *__restrict__ D, int32_t n, int32_t m, double *__restrict__ sum, const int32_t *__restrict__ cell) {
    const int32_t i = cell[0], j = cell[1];
    if (i < 0 || j <= i || j >= m) return;
    double *row_i = D + (size_t)i * (size_t)n;
    const double *row_j = D + (size_t)j * (size_t)n;
    const double dij = row_i[j];
    for (int64_t k = (int64_t)blockIdx.x * NJ_THREADS + threadIdx.x; k < m; k += (int64_t)gridDim.x * NJ_THREADS) {
        if (k == i || k == j) continue;
        const double dik = row_i[k], djk = row_j[k];
        const double u = kp_nj_u(dik, djk, dij);
        sum[k] = kp_nj_r(sum[k], dik, djk, u);
        row_i[k] = u;
        D[(size_t)k * (size_t)n + (size_t)i] = u;
    }
}

// Fourth step, a launch of its own because it overwrites the row the third reads: slot m - 1 moves into slot j -- one lane per
// slot k < m - 1 copies d(m - 1, k) into row j and column j --, and the first wave of workgroup 0 finishes R_i: SUM64 of row i over
// the m - 1 slots as they stand after the move, its entry at j read from where it stood before, d(i, m - 1).  The move reads row
// m - 1 and writes row j and column j; the sum reads row i, but for its entry in column j: no lane reads what another writes.
__global__ __launch_bounds__(NJ_THREADS) void kp_nj_move_kernel(double *__restrict__ D, int32_t n, int32_t m, double *__restrict__ sum, int32_t *__restrict__ node,
                                                                const int32_t *__restrict__ cell) {
    const int32_t i = cell[0], j = cell[1], last = m - 1;
    if (i < 0 || j <= i || j >= m) return;
    if (j != last) {
        const double *row_last = D + (size_t)last * (size_t)n;
        double *row_j = D + (size_t)j * (size_t)n;
        for (int64_t k = (int64_t)blockIdx.x * NJ_THREADS + threadIdx.x; k < last; k += (int64_t)gridDim.x * NJ_THREADS) {
            if (k == j) { row_j[j] = 0.0; continue; }
            const double v = row_last[k];
            row_j[k] = v;
            D[(size_t)k * (size_t)n + (size_t)j] = v;
        }
    }
    if (blockIdx.x != 0 || threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    const double mine = nj_wave_sum64(nj_lane_fold(D + (size_t)i * (size_t)n, last, lane, j, last));
    if (lane == 0) {
        sum[i] = mine;
        if (j != last) { sum[j] = sum[last]; node[j] = node[last]; }
    }
}

// END, one lane: the last record of three slots, or the one record of two taxa.
__global__ void kp_nj_end_kernel(const double *__restrict__ D, int32_t n, int32_t m, const int32_t *__restrict__ node, kp_nj_node *__restrict__ rec, int32_t at) {
    KP_NJ_EXACT
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    if (m == 2) {
        const double h = 0.5 * D[1];
        kp_nj_node_store(rec + at, node[0], node[1], -1, h, h, 0.0);
    } else if (m == 3) {
        double lx, ly, lz;
        kp_nj_end(D[1], D[2], D[(size_t)n + 2], &lx, &ly, &lz);
        kp_nj_node_store(rec + at, node[0], node[1], node[2], lx, ly, lz);
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

int kp_dist_nj(kp_ctx *ctx, kp_dist *d, int32_t min_compared, int32_t *taxa, int64_t cap_taxa, int32_t *n_taxa, kp_nj_node *nodes, int64_t cap_nodes,
               int64_t *n_nodes) {
    if (ctx && d) {  // (whatever refuses the call from here on)
        if (n_taxa) *n_taxa = 0;
        if (n_nodes) *n_nodes = 0;
    }
    int rc;
    if ((rc = dist_enter(ctx, d, n_taxa, "null distance handle or taxon count pointer"))) return rc;
    const bool counting = !taxa && !nodes && cap_taxa == 0 && cap_nodes == 0;  // the counting form: *n_taxa alone
    if (cap_taxa < 0 || cap_nodes < 0) return kp_fail(ctx, KP_EINVAL, "negative room for taxa or records");
    if (cap_taxa > 0 && !taxa) return kp_fail(ctx, KP_EINVAL, "null taxon table");
    if (cap_nodes > 0 && !nodes) return kp_fail(ctx, KP_EINVAL, "null record table");
    if (!counting && !n_nodes) return kp_fail(ctx, KP_EINVAL, "null record count pointer");
    const int32_t R = d->n_rows;
    if (R == 0) return KP_OK;
    KP_HIP_CHECK(ctx, hipSetDevice(ctx->device));
    kp_dist::Nj &t = d->nj;
    const size_t rows = (size_t)R;
    if ((rc = DistReserve()(t.bases, rows)(t.flag, rows)(t.off, rows + 1)(t.taxon, rows)(t.taxa, rows)(t.sum, rows)(t.node, rows)(t.cell, 2)(t.rec, rows).done(ctx, "neighbour-joining tables")))
        return rc;
    // ---- bases and taxa
    const unsigned grid = dist_grid(R);
    KP_HIP_CHECK(ctx, hipMemsetAsync(t.bases.p, 0, rows * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(kp_nj_bases_kernel, dim3(dist_grid((int64_t)R * d->n_words)), dim3(DIST_THREADS), 0, ctx->stream, d->d_planes.p, R, d->n_words, t.bases.p);
    hipLaunchKernelGGL(kp_nj_flag_kernel, dim3(grid), dim3(DIST_THREADS), 0, ctx->stream, t.bases.p, R, 16 * d->n_blocks, min_compared, t.flag.p);
    kp_launch_count_scan(t.flag.p, R, t.off.p, ctx->stream);
    hipLaunchKernelGGL(kp_nj_number_kernel, dim3(grid), dim3(DIST_THREADS), 0, ctx->stream, t.flag.p, t.off.p, R, t.taxon.p, t.taxa.p);
    KP_HIP_CHECK(ctx, hipGetLastError());
    int64_t counted = 0;
    if ((rc = fetch_all(ctx, ctx->stream, {{&counted, t.off.p + R, sizeof(int64_t)}}))) return rc;
    if (counted < 0 || counted > R) return kp_fail(ctx, KP_ESTATE, "more taxa than rows");
    const int32_t n = (int32_t)counted;
    *n_taxa = n;
    if (counting) return KP_OK;
    if (n > KP_NJ_MAX_TAXA) return kp_fail(ctx, KP_EINVAL, "more taxa than a neighbour-joining tree may have (KP_NJ_MAX_TAXA)");
    const int64_t n_rec = kp_nj_records(n);
    if (cap_taxa < n) return kp_fail(ctx, KP_EINVAL, "room for fewer taxa than the matrix has (the counting form gives n_taxa)");
    if (cap_nodes < n_rec) return kp_fail(ctx, KP_EINVAL, "room for fewer records than the tree has (n_taxa - 2; one for two taxa)");
    if (n_rec > 0) {
        // ---- the matrix and the partials: this call's own, freed when it returns
        DevBuf<double> D;
        DevBuf<NjBest> part;
        if ((rc = DistReserve()(D, (size_t)n * (size_t)n)(part, (size_t)std::min<int32_t>(n, NJ_MAX_PARTS)).done(ctx, "neighbour-joining matrix"))) return rc;
        if ((rc = dist_launch_tiles(ctx, d, kp_dist_nj_kernel, t.taxon.p, n, D.p))) return rc;
        hipLaunchKernelGGL(kp_nj_init_kernel, dim3(dist_grid(n, NJ_WAVES, 4096)), dim3(NJ_THREADS), 0, ctx->stream, D.p, n, t.sum.p, t.node.p);
        KP_HIP_CHECK(ctx, hipGetLastError());
        // ---- every join, enqueued without a look at one: m is known here, the pair lives in the cell
        int32_t at = 0;
        for (int32_t m = n; m > 3; --m, ++at) {
            const int32_t parts = std::min<int32_t>(m - 1, NJ_MAX_PARTS);
            const unsigned slots = dist_grid(m, NJ_THREADS);
            hipLaunchKernelGGL(kp_nj_pick_kernel, dim3((unsigned)parts), dim3(NJ_THREADS), 0, ctx->stream, D.p, n, m, t.sum.p, part.p);
            hipLaunchKernelGGL(kp_nj_join_kernel, dim3(1), dim3(NJ_THREADS), 0, ctx->stream, part.p, parts, D.p, n, m, t.sum.p, t.node.p, t.cell.p, t.rec.p, at, n + at);
            hipLaunchKernelGGL(kp_nj_update_kernel, dim3(slots), dim3(NJ_THREADS), 0, ctx->stream, D.p, n, m, t.sum.p, t.cell.p);
            hipLaunchKernelGGL(kp_nj_move_kernel, dim3(slots), dim3(NJ_THREADS), 0, ctx->stream, D.p, n, m, t.sum.p, t.node.p, t.cell.p);
            if ((at & 255) == 255) KP_HIP_CHECK(ctx, hipGetLastError());
        }
        hipLaunchKernelGGL(kp_nj_end_kernel, dim3(1), dim3(64), 0, ctx->stream, D.p, n, std::min<int32_t>(n, 3), t.node.p, t.rec.p, at);
        KP_HIP_CHECK(ctx, hipGetLastError());
        if (at + 1 != n_rec) return kp_fail(ctx, KP_ESTATE, "the joins do not add up to the tree's records");
        KP_HIP_CHECK(ctx, hipMemcpyAsync(nodes, t.rec.p, (size_t)n_rec * sizeof(kp_nj_node), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (n > 0) KP_HIP_CHECK(ctx, hipMemcpyAsync(taxa, t.taxa.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the matrix goes away behind it)
    for (int64_t r = 0; r < n_rec; ++r)
        if (nodes[r].a < 0) return kp_fail(ctx, KP_ESTATE, "a join found no pair");
    *n_nodes = n_rec;
    return KP_OK;
}

void kp_dist_destroy(kp_dist *d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    delete d;
}

}  // extern "C"
