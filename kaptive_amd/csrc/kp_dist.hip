// kp_dist.hip -- pairwise distances between the locus rows of a run (kp_spec.h, DISTANCES; the arithmetic: kp_dist.h).
//
// A handle (kp_dist, kp_dist_handle.h) holds the bit planes of one matrix of R locus rows of NB blocks, and the listing of its most
// recent count.  This unit makes and destroys the handle; the other reports over it: kp_dist_graph.hip (clusters, tree),
// kp_dist_sites.hip (variable sites), kp_dist_nj.hip (neighbour joining).
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
//                          not present, they count nothing.  No atomics.  (The chunk loop: dist_tile_counts, kp_dist_handle.h.)
//       listing            the same kernel twice.  COUNT: for every row a of the tile and its tile column tj, how many pairs
//                          (a, b) qualify (a < b < R, kp_dist_listed) -> cnt[a * nt + tj]; one workgroup owns the entry.  The
//                          entries in index order ARE the listing's order (ascending a, then b), so their exclusive scan gives
//                          every entry's first record -- in two levels: a wave per row adds the row's entries, the one-block
//                          scan (kp_launch_count_scan) runs over the R row totals, a wave per row spreads its row's prefix.  FILL recomputes the counts and stores the
//                          records: for a fixed (i, j) the sixteen pairs of a row are sixteen neighbouring lanes of one wave -- a
//                          ballot, restricted to those sixteen bits, and mbcnt rank them in ascending b.
//
// Bounds: a lane reads planes only for r < R and w < NW, stores cnt only for a < R and tj < nt, and a record only below the total
// the count pass found (the fill recomputes the same flags, so it is the same total).
#include <new>

#include "kp_dist_handle.h"

namespace {

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
    if ((rc = dist_grow(ctx, l.rec, (size_t)l.n_pairs, "distance records"))) return rc;  // a longer listing than every one before
    if ((rc = dist_launch_tiles(ctx, d, kp_dist_pair_kernel<true>, l.max_diff, l.min_compared, l.cnt.p, l.off.p, l.rec.p, l.n_pairs))) return rc;
    KP_HIP_CHECK(ctx, hipMemcpyAsync(out, l.rec.p, (size_t)l.n_pairs * sizeof(kp_dist_pair), hipMemcpyDeviceToHost, ctx->stream));
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
