// kp_dist_sites.hip -- the variable sites of the locus rows of a distance handle (kp_spec.h, SITES; the arithmetic: kp_sites.h).  The
// handle and its planes: kp_dist_handle.h; no tile of pairs is looked at here.
//
//   kp_sites_profile_kernel  the transposed reduction: every column over all rows.  One workgroup of 256
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
// Bounds: the profile kernel reads planes for r < R and w < NW and adds at records 64 w + j < 64 NW of a table of 64 NW records; the
// list kernel reads records c < 16 NB <= 64 NW, stores flag[c] and a record only below min(off[c] + 1, 16 NB); the row kernel reads
// site records s < S, planes at the record's column -- a c < 16 NB the fill stored, checked again -- and r < R, and stores block
// r * SB + sb < R * SB.
#include "kp_dist_handle.h"
#include "kp_sites.h"

namespace {

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

}  // namespace

extern "C" {

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
    if ((rc = dist_grow(ctx, s.rows, (size_t)need, "site rows"))) return rc;  // a larger table than every one before
    hipLaunchKernelGGL(kp_site_rows_kernel, dim3(dist_grid(need)), dim3(DIST_THREADS), 0, ctx->stream, d->d_planes.p, d->n_rows, d->n_words, s.rec.p, s.n_sites, SB, s.rows.p);
    KP_HIP_CHECK(ctx, hipGetLastError());
    KP_HIP_CHECK(ctx, hipMemcpyAsync(blocks, s.rows.p, (size_t)need * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return KP_OK;
}

}  // extern "C"
