// kp_dist_nj.hip -- the neighbour-joining tree of the locus rows of a distance handle (kp_spec.h, NJ; the arithmetic: kp_nj.h).  The
// handle, the tiles and their chunk loop: kp_dist_handle.h.
//
//   kp_dist_nj_kernel      the pair kernel's tiles and counts with a fourth epilogue: every pair of taxa stores its
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
// The state of the join loop: the dense matrix D of the taxa, n x n doubles, row-major with the row stride n throughout -- the m
// live slots are its first m rows and columns --, R of every slot (`sum`), the node id of every slot, and the pair of the join under
// way in a device cell: the host enqueues every join of a tree without looking at one.  The kernels of the loop take these tables as
// an NjBatch (kp_dist_handle.h) and join tree blockIdx.y of it: kp_dist_nj launches a batch of one, kp_dist_boot.hip (kp_spec.h,
// BOOTSTRAP) the replicates of a batch, which all have m slots at the same join -- dist_nj_joins below is the loop for both.
// Bounds: D is read and written at [slot < m][slot < m], m <= n; sum and node at slots < m; part at blockIdx.x < its grid, which the
// host keeps at NJ_MAX_PARTS or less; rec at the record index the host passes, below kp_nj_records(n) <= n_rows.  A pair the cell
// holds is used only when 0 <= i < j < m.
#include <algorithm>
#include <climits>

#include "kp_dist_handle.h"
#include "kp_nj.h"

namespace {

constexpr int NJ_THREADS = 256, NJ_WAVES = NJ_THREADS / 64, NJ_MAX_PARTS = 1024;
static_assert(KP_NJ_LANES == 64, "SUM64 is one wavefront's reduction");

// (NjBest, a pick -- the smallest (Q, a, b) seen; nothing seen: (+inf, INT32_MAX, INT32_MAX) --, and NjBatch, the tables of the trees a
// launch joins: kp_dist_handle.h)
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
__global__ __launch_bounds__(NJ_THREADS) void kp_nj_init_kernel(NjBatch t, int32_t n) {
    const double *__restrict__ D = t.D + (size_t)blockIdx.y * (size_t)t.sD;
    double *__restrict__ sum = t.sum + (size_t)blockIdx.y * (size_t)t.sN;
    int32_t *__restrict__ node = t.node + (size_t)blockIdx.y * (size_t)t.sN;
    const int lane = threadIdx.x & 63;
    for (int64_t k = (int64_t)blockIdx.x * NJ_WAVES + threadIdx.x / 64; k < n; k += (int64_t)gridDim.x * NJ_WAVES) {  // (k is the same in every lane of a wave)
        const double mine = nj_wave_sum64(nj_lane_fold(D + (size_t)k * (size_t)n, n, lane, -1, -1));
        if (lane == 0) { sum[k] = mine; node[k] = (int32_t)k; }
    }
}

// A join's pick, first step: workgroup g scans the rows a = g, g + grid, .. of the triangle a < b < m -- a row is one coalesced run
// -- and leaves the smallest (Q, a, b) it met in part[g].
__global__ __launch_bounds__(NJ_THREADS) void kp_nj_pick_kernel(NjBatch t, int32_t n, int32_t m) {
    __shared__ NjBest s_best[NJ_WAVES];
    const double *__restrict__ D = t.D + (size_t)blockIdx.y * (size_t)t.sD;
    const double *__restrict__ sum = t.sum + (size_t)blockIdx.y * (size_t)t.sN;
    NjBest *__restrict__ part = t.part + (size_t)blockIdx.y * (size_t)t.sPart;
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
__global__ __launch_bounds__(NJ_THREADS) void kp_nj_join_kernel(NjBatch t, int32_t n_parts, int32_t n, int32_t m, int32_t at, int32_t new_id) {
    __shared__ NjBest s_best[NJ_WAVES];
    const NjBest *__restrict__ part = t.part + (size_t)blockIdx.y * (size_t)t.sPart;
    const double *__restrict__ D = t.D + (size_t)blockIdx.y * (size_t)t.sD;
    const double *__restrict__ sum = t.sum + (size_t)blockIdx.y * (size_t)t.sN;
    int32_t *__restrict__ node = t.node + (size_t)blockIdx.y * (size_t)t.sN;
    int32_t *__restrict__ cell = t.cell + 2 * (size_t)blockIdx.y;
    kp_nj_node *__restrict__ rec = t.rec + (size_t)blockIdx.y * (size_t)t.sRec;
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
__global__ __launch_bounds__(NJ_THREADS) void kp_nj_update_kernel(NjBatch t, int32_t n, int32_t m) {
    double *__restrict__ D = t.D + (size_t)blockIdx.y * (size_t)t.sD;
    double *__restrict__ sum = t.sum + (size_t)blockIdx.y * (size_t)t.sN;
    const int32_t *__restrict__ cell = t.cell + 2 * (size_t)blockIdx.y;
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
__global__ __launch_bounds__(NJ_THREADS) void kp_nj_move_kernel(NjBatch t, int32_t n, int32_t m) {
    double *__restrict__ D = t.D + (size_t)blockIdx.y * (size_t)t.sD;
    double *__restrict__ sum = t.sum + (size_t)blockIdx.y * (size_t)t.sN;
    int32_t *__restrict__ node = t.node + (size_t)blockIdx.y * (size_t)t.sN;
    const int32_t *__restrict__ cell = t.cell + 2 * (size_t)blockIdx.y;
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
__global__ void kp_nj_end_kernel(NjBatch t, int32_t n, int32_t m, int32_t at) {
    KP_NJ_EXACT
    const double *__restrict__ D = t.D + (size_t)blockIdx.y * (size_t)t.sD;
    const int32_t *__restrict__ node = t.node + (size_t)blockIdx.y * (size_t)t.sN;
    kp_nj_node *__restrict__ rec = t.rec + (size_t)blockIdx.y * (size_t)t.sRec;
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

}  // namespace

// The taxa of the handle's rows for min_compared, numbered (the first tables of kp_dist::Nj, all of them reserved here), and their
// number: what kp_dist_nj and kp_dist_nj_bootstrap both begin with.
int dist_nj_taxa(kp_ctx *ctx, kp_dist *d, int32_t min_compared, int32_t *n_taxa) {
    const int32_t R = d->n_rows;
    int rc;
    kp_dist::Nj &t = d->nj;
    const size_t rows = (size_t)R;
    if ((rc = DistReserve()(t.bases, rows)(t.flag, rows)(t.off, rows + 1)(t.taxon, rows)(t.taxa, rows)(t.sum, rows)(t.node, rows)(t.cell, 2)(t.rec, rows).done(ctx, "neighbour-joining tables")))
        return rc;
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
    *n_taxa = (int32_t)counted;
    return KP_OK;
}

int32_t dist_nj_parts(int32_t n) { return std::min<int32_t>(std::max<int32_t>(n, 1), NJ_MAX_PARTS); }

// The trees of `batch` filled matrices of n >= 2 taxa each, enqueued without a look at the device: the row sums, every join -- four
// launches a join, whatever the batch: a tree is blockIdx.y of each, and every tree of a batch has m slots at the same join -- and
// the last record.  Returns the records a tree has through *n_rec.
int dist_nj_joins(kp_ctx *ctx, const NjBatch &t, int32_t n, int32_t batch, int64_t *n_rec) {
    const unsigned y = (unsigned)batch;
    hipLaunchKernelGGL(kp_nj_init_kernel, dim3(dist_grid(n, NJ_WAVES, 4096), y), dim3(NJ_THREADS), 0, ctx->stream, t, n);
    KP_HIP_CHECK(ctx, hipGetLastError());
    int32_t at = 0;
    for (int32_t m = n; m > 3; --m, ++at) {
        const int32_t parts = std::min<int32_t>(m - 1, NJ_MAX_PARTS);
        const unsigned slots = dist_grid(m, NJ_THREADS);
        hipLaunchKernelGGL(kp_nj_pick_kernel, dim3((unsigned)parts, y), dim3(NJ_THREADS), 0, ctx->stream, t, n, m);
        hipLaunchKernelGGL(kp_nj_join_kernel, dim3(1, y), dim3(NJ_THREADS), 0, ctx->stream, t, parts, n, m, at, n + at);
        hipLaunchKernelGGL(kp_nj_update_kernel, dim3(slots, y), dim3(NJ_THREADS), 0, ctx->stream, t, n, m);
        hipLaunchKernelGGL(kp_nj_move_kernel, dim3(slots, y), dim3(NJ_THREADS), 0, ctx->stream, t, n, m);
        if ((at & 255) == 255) KP_HIP_CHECK(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(kp_nj_end_kernel, dim3(1, y), dim3(64), 0, ctx->stream, t, n, std::min<int32_t>(n, 3), at);
    KP_HIP_CHECK(ctx, hipGetLastError());
    *n_rec = at + 1;
    return KP_OK;
}

extern "C" {

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
    // ---- bases and taxa
    int32_t n = 0;
    if ((rc = dist_nj_taxa(ctx, d, min_compared, &n))) return rc;
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
        if ((rc = DistReserve()(D, (size_t)n * (size_t)n)(part, (size_t)dist_nj_parts(n)).done(ctx, "neighbour-joining matrix"))) return rc;
        if ((rc = dist_launch_tiles(ctx, d, kp_dist_nj_kernel, t.taxon.p, n, D.p))) return rc;
        // ---- every join, enqueued without a look at one: m is known to the host, the pair lives in the cell.  One tree: a batch of one
        int64_t made = 0;
        const NjBatch one{D.p, t.sum.p, t.node.p, t.cell.p, t.rec.p, part.p, 0, 0, 0, 0};
        if ((rc = dist_nj_joins(ctx, one, n, 1, &made))) return rc;
        if (made != n_rec) return kp_fail(ctx, KP_ESTATE, "the joins do not add up to the tree's records");
        KP_HIP_CHECK(ctx, hipMemcpyAsync(nodes, t.rec.p, (size_t)n_rec * sizeof(kp_nj_node), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (n > 0) KP_HIP_CHECK(ctx, hipMemcpyAsync(taxa, t.taxa.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the matrix goes away behind it)
    for (int64_t r = 0; r < n_rec; ++r)
        if (nodes[r].a < 0) return kp_fail(ctx, KP_ESTATE, "a join found no pair");
    *n_nodes = n_rec;
    return KP_OK;
}

}  // extern "C"
