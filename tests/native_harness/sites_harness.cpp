// sites_harness.cpp -- test infrastructure for tests/test_sites_cpu.py (g++, no GPU): the functions of kaptive_amd/csrc/kp_sites.h --
// the ones the device kernels call -- on host arrays.
//   * kpy_sites_layout: the record's size and the constants the Python side mirrors.
//   * kpy_sites_counter: n masks added into one bit-sliced counter, its 64 counts read back.
//   * kpy_sites_transpose: the six exchange steps over 64 words.
//   * kpy_site_derived: the predicate without and with the core flag, ALLELES, MAJOR, INFORMATIVE and gap of one profile.
//   * kpy_site_gene: the gene and position of a matrix column.
//   * kpy_sites_host: profile, sites and site rows of a matrix the way the kernels make them -- slabs of KP_SITES_SLAB rows, a
//     counter set per lane, the lanes of a wave combined by the transposition, integer adds into the table.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../kaptive_amd/csrc/kp_sites.h"

extern "C" {

void kpy_sites_layout(int32_t *out8) {
    out8[0] = (int32_t)sizeof(kp_site); out8[1] = KP_SITES_THREADS; out8[2] = KP_SITES_PLANES; out8[3] = KP_SITES_LANE_ROWS;
    out8[4] = KP_SITES_SLAB; out8[5] = KP_SITES_CLASSES; out8[6] = KP_SITES_CORE; out8[7] = KP_SITES_BLOCK;
}

void kpy_sites_counter(const uint64_t *masks, int32_t n, int32_t *out64) {
    KpSiteCounter c{};
    for (int32_t i = 0; i < n; ++i) kp_sites_counter_add(&c, masks[i]);
    for (int j = 0; j < 64; ++j) out64[j] = kp_sites_counter_get(&c, j);
}

void kpy_sites_transpose(uint64_t *x64) { kp_sites_transpose64(x64); }

void kpy_site_derived(const int32_t *n5, int32_t R, int32_t, int32_t *out6) {
    out6[0] = kp_site_is(n5, n5[4], R, 0); out6[1] = kp_site_is(n5, n5[4], R, KP_SITES_CORE); out6[2] = kp_site_alleles(n5);
    out6[3] = kp_site_major(n5); out6[4] = kp_site_informative(n5); out6[5] = kp_site_gap(n5, n5[4], R);
}

int32_t kpy_site_gene(const int64_t *gene_blocks, int32_t n_genes, int64_t column, int64_t *position) { return kp_site_gene(gene_blocks, n_genes, column, position); }

void kpy_site_store(kp_site *p, int32_t column, int32_t a, int32_t c, int32_t g, int32_t t, int32_t n_n) { kp_site_store(p, column, a, c, g, t, n_n); }

int64_t kpy_sites_host(const uint64_t *blocks, int32_t R, int64_t nb, int32_t flags, kp_site *prof, kp_site *rec, uint64_t *rows) {
    const int64_t NW = kp_dist_words(nb);
    std::vector<kp_site> table((size_t)(64 * NW));
    for (int64_t c = 0; c < 64 * NW; ++c) kp_site_store(&table[(size_t)c], (int32_t)c, 0, 0, 0, 0, 0);
    std::vector<KpDistWord> planes((size_t)NW * (size_t)R);
    for (int64_t w = 0; w < NW; ++w)
        for (int32_t r = 0; r < R; ++r) planes[(size_t)w * R + r] = kp_dist_word_planes(blocks + (size_t)r * nb, nb, w);
    const int64_t n_slabs = ((int64_t)R + KP_SITES_SLAB - 1) / KP_SITES_SLAB;
    for (int64_t w = 0; w < NW; ++w)
        for (int64_t slab = 0; slab < n_slabs; ++slab)
            for (int wave = 0; wave < KP_SITES_THREADS / 64; ++wave) {
                KpSiteCounter cnt[64][KP_SITES_CLASSES] = {};
                for (int lane = 0; lane < 64; ++lane)
                    for (int i = 0; i < KP_SITES_LANE_ROWS; ++i) {
                        const int64_t r = slab * KP_SITES_SLAB + (int64_t)i * KP_SITES_THREADS + wave * 64 + lane;
                        if (r >= R) continue;
                        const KpDistWord &q = planes[(size_t)w * R + r];
                        const KpSiteMasks m = kp_sites_masks(q.lo, q.hi, q.valid, q.present);
                        for (int k = 0; k < KP_SITES_CLASSES; ++k) kp_sites_counter_add(&cnt[lane][k], m.m[k]);
                    }
                for (int k = 0; k < KP_SITES_CLASSES; ++k)
                    for (int b = 0; b < KP_SITES_PLANES; ++b) {
                        uint64_t x[64];
                        for (int lane = 0; lane < 64; ++lane) x[lane] = cnt[lane][k].p[b];
                        kp_sites_transpose64(x);
                        for (int j = 0; j < 64; ++j) (&table[(size_t)(w * 64 + j)].n[0])[k] += __builtin_popcountll(x[j]) << b;
                    }
            }
    int64_t S = 0;
    for (int64_t c = 0; c < 16 * nb; ++c) {
        prof[c] = table[(size_t)c];
        if (R > 1 && kp_site_is(table[(size_t)c].n, table[(size_t)c].n_n, R, flags)) rec[S++] = table[(size_t)c];
    }
    const int64_t SB = kp_site_row_blocks(S);
    for (int32_t r = 0; r < R; ++r)
        for (int64_t sb = 0; sb < SB; ++sb) {
            uint64_t v = 0;
            for (int k = 0; k < KP_SITES_BLOCK; ++k) {
                const int64_t s = sb * KP_SITES_BLOCK + k;
                if (s >= S) { v |= 1ull << (KP_DIST_GAP_SHIFT + k); continue; }
                const int64_t c = rec[s].column;
                const KpDistWord &q = planes[(size_t)(c >> 6) * R + r];
                const int bit = (int)(c & 63);
                v |= kp_site_block_code(k, q.lo >> bit, q.hi >> bit, q.valid >> bit, q.present >> bit);
            }
            rows[(size_t)r * SB + sb] = v;
        }
    return S;
}

}  // extern "C"
