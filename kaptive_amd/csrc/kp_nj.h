// kp_nj.h -- neighbour-joining over locus rows (kp_spec.h, NJ), written once as plain functions: the taxon predicate, the distance of
// a pair, SUM64, the Q, length and update expressions, the order of the pick, a serial host NJ over a dense matrix, and the taxa and
// the matrix of a matrix of blocks.  The NJ kernels of kp_dist_nj.hip and their host share them.  No HIP header: tests/native_harness
// compiles it with g++.
//
// Every floating-point operation of the section is rounded to binary64 on its own.  hipcc contracts a * b + c into one fused
// operation by default, which rounds differently: KP_NJ_EXACT switches that off for the body it opens, and the setting stays with
// the operations where the function is inlined into a kernel.
#pragma once

#include <stdint.h>

#include <vector>

#include "kp_caps.h"
#include "kp_dist.h"

#if defined(__clang__)
#define KP_NJ_EXACT _Pragma("clang fp contract(off)")
#else
#define KP_NJ_EXACT /* g++ without -march emits no fused operation */
#endif

#define KP_NJ_LANES 64 /* partial sums of SUM64: the lanes of one wavefront */

// TAXA.  Row r is a taxon iff 2 bases(r) >= W + max(min_compared, 1): any two taxa then share at least that many compared columns.
KP_HD bool kp_nj_taxon(int64_t bases, int64_t W, int32_t min_compared) { return 2 * bases >= W + (int64_t)(min_compared > 1 ? min_compared : 1); }

// bases(r) of a row of nb blocks
inline int64_t kp_nj_row_bases(const uint64_t *row, int64_t nb) {
    int64_t n = 0;
    for (int64_t w = 0; w < kp_dist_words(nb); ++w) n += __builtin_popcountll(kp_dist_word_planes(row, nb, w).valid);
    return n;
}

// DISTANCE.  One correctly rounded division; a pair without a compared column -- no pair of taxa -- is 0 apart.
KP_HD double kp_nj_distance(int32_t differences, int32_t compared) {
    KP_NJ_EXACT
    return compared > 0 ? (double)differences / (double)compared : 0.0;
}

// JOIN.  Q of slots a < b; the pick's order (Q, a, b); the two lengths of the joined pair; the new node's distance to slot k and
// slot k's new R.
KP_HD double kp_nj_q(double f, double d, double ra, double rb) {
    KP_NJ_EXACT
    const double fd = f * d;
    const double q = fd - ra;
    return q - rb;
}
KP_HD bool kp_nj_less(double q, int32_t a, int32_t b, double q2, int32_t a2, int32_t b2) { return q < q2 || (q == q2 && (a < a2 || (a == a2 && b < b2))); }
KP_HD void kp_nj_lengths(double dij, double ri, double rj, double f, double *li, double *lj) {
    KP_NJ_EXACT
    const double diff = ri - rj;
    const double delta = diff / f;
    const double sum = dij + delta;
    *li = 0.5 * sum;
    *lj = dij - *li;
}
KP_HD double kp_nj_u(double dik, double djk, double dij) {
    KP_NJ_EXACT
    const double s = dik + djk;
    const double t = s - dij;
    return 0.5 * t;
}
KP_HD double kp_nj_r(double rk, double dik, double djk, double uk) {
    KP_NJ_EXACT
    const double a = rk - dik;
    const double b = a - djk;
    return b + uk;
}
// END.  The three lengths of the last record, slots x, y, z = 0, 1, 2.
KP_HD void kp_nj_end(double dxy, double dxz, double dyz, double *lx, double *ly, double *lz) {
    *lx = kp_nj_u(dxy, dxz, dyz);
    *ly = kp_nj_u(dxy, dyz, dxz);
    *lz = kp_nj_u(dxz, dyz, dxy);
}

// five 8-byte words, like every record the device stores
static_assert(sizeof(kp_nj_node) == 40, "an NJ record is five 8-byte words");
KP_HD void kp_nj_node_store(kp_nj_node *p, int32_t a, int32_t b, int32_t c, double la, double lb, double lc) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long *w = reinterpret_cast<unsigned long long *>(p);
    double *l = reinterpret_cast<double *>(p);
    w[0] = (uint64_t)(uint32_t)a | ((uint64_t)(uint32_t)b << 32);
    w[1] = (uint64_t)(uint32_t)c;
    l[2] = la; l[3] = lb; l[4] = lc;
#else
    p->a = a; p->b = b; p->c = c; p->pad_ = 0; p->la = la; p->lb = lb; p->lc = lc;
#endif
}

// SUM64 of v[0], v[stride], .. (m of them): 64 strided left folds from +0.0, then the halving adds S_l += S_{l + o}.
inline double kp_nj_sum64(const double *v, int64_t m, int64_t stride = 1) {
    KP_NJ_EXACT
    double s[KP_NJ_LANES];
    for (int l = 0; l < KP_NJ_LANES; ++l) s[l] = 0.0;
    for (int64_t k = 0; k < m; ++k) s[k % KP_NJ_LANES] = s[k % KP_NJ_LANES] + v[k * stride];
    for (int o = KP_NJ_LANES / 2; o >= 1; o >>= 1)
        for (int l = 0; l < o; ++l) s[l] = s[l] + s[l + o];
    return s[0];
}

// How many records the tree of n taxa has.
KP_HD int64_t kp_nj_records(int64_t n) { return n <= 1 ? 0 : (n == 2 ? 1 : n - 2); }

// The tree of a dense n x n matrix D (row-major, symmetric, zero diagonal), serially, by the section's rule.  out
// [kp_nj_records(n)].  Returns the number of records.
inline int64_t kp_nj_host(const double *D, int32_t n, kp_nj_node *out) {
    KP_NJ_EXACT
    if (n <= 1) return 0;
    if (n == 2) {
        const double h = 0.5 * D[1];
        kp_nj_node_store(out, 0, 1, -1, h, h, 0.0);
        return 1;
    }
    const size_t N = (size_t)n;
    std::vector<double> d(D, D + N * N), R(N);
    std::vector<int32_t> node(N);
    for (int32_t k = 0; k < n; ++k) {
        node[(size_t)k] = k;
        R[(size_t)k] = kp_nj_sum64(d.data() + (size_t)k * N, n);
    }
    int32_t m = n, next = n;
    int64_t rec = 0;
    while (m > 3) {
        const double f = (double)(m - 2);
        double bq = 0.0;
        int32_t bi = -1, bj = -1;
        for (int32_t a = 0; a < m; ++a)
            for (int32_t b = a + 1; b < m; ++b) {
                const double q = kp_nj_q(f, d[(size_t)a * N + (size_t)b], R[(size_t)a], R[(size_t)b]);
                if (bi < 0 || kp_nj_less(q, a, b, bq, bi, bj)) { bq = q; bi = a; bj = b; }
            }
        const size_t i = (size_t)bi, j = (size_t)bj;
        const double dij = d[i * N + j];
        double li, lj;
        kp_nj_lengths(dij, R[i], R[j], f, &li, &lj);
        kp_nj_node_store(out + rec++, node[i], node[j], -1, li, lj, 0.0);
        for (size_t k = 0; k < (size_t)m; ++k) {
            if (k == i || k == j) continue;
            const double dik = d[i * N + k], djk = d[j * N + k];
            const double u = kp_nj_u(dik, djk, dij);
            R[k] = kp_nj_r(R[k], dik, djk, u);
            d[i * N + k] = d[k * N + i] = u;
        }
        d[i * N + i] = 0.0;
        node[i] = next++;
        const size_t last = (size_t)m - 1;
        if (j != last) {
            for (size_t k = 0; k < last; ++k) {
                if (k == j) continue;
                d[j * N + k] = d[k * N + j] = d[last * N + k];
            }
            d[j * N + j] = 0.0;
            R[j] = R[last];
            node[j] = node[last];
        }
        --m;
        R[i] = kp_nj_sum64(d.data() + i * N, m);
    }
    double lx, ly, lz;
    kp_nj_end(d[1], d[2], d[N + 2], &lx, &ly, &lz);
    kp_nj_node_store(out + rec++, node[0], node[1], node[2], lx, ly, lz);
    return rec;
}

// The taxa of a matrix of R rows of nb blocks and their dense matrix.  taxa [R]: the rows of the taxa, ascending; D, if given,
// [n * n] for the n the call returns (call it with D null first to learn n).
inline int32_t kp_nj_matrix_host(const uint64_t *blocks, int32_t R, int64_t nb, int32_t min_compared, int32_t *taxa, double *D) {
    int32_t n = 0;
    for (int32_t r = 0; r < R; ++r)
        if (kp_nj_taxon(kp_nj_row_bases(blocks + (size_t)r * (size_t)nb, nb), 16 * nb, min_compared)) taxa[n++] = r;
    if (!D) return n;
    for (int32_t a = 0; a < n; ++a) {
        D[(size_t)a * (size_t)n + (size_t)a] = 0.0;
        for (int32_t b = a + 1; b < n; ++b) {
            const KpDistCounts c = kp_dist_row_counts(blocks + (size_t)taxa[a] * (size_t)nb, blocks + (size_t)taxa[b] * (size_t)nb, nb);
            D[(size_t)a * (size_t)n + (size_t)b] = D[(size_t)b * (size_t)n + (size_t)a] = kp_nj_distance(c.differences, c.compared);
        }
    }
    return n;
}
