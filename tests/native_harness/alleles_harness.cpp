// alleles_harness.cpp -- test infrastructure for tests/test_alleles_cpu.py (g++, no GPU): the functions of
// kaptive_amd/csrc/kp_alleles.h -- the ones the device kernel gives a lane per block -- on host arrays.
//   * kpy_al_nt / kpy_al_aa / kpy_al_locus: the digests with the blocks taken one after the other.
//   * kpy_al_nt_lanes: the nucleotide digest with the blocks dealt out to `lanes` lanes as the kernel deals them (lane, lane + lanes,
//     ...), every lane keeping a partial sum, the sums added at the end.
//   * kpy_al_mix: the mixer.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../kaptive_amd/csrc/kp_alleles.h"

extern "C" {

uint64_t kpy_al_mix(uint64_t z) { return kp_al_mix(z); }

static KpTargetSeq target(const uint32_t *words, int n_words, const int32_t *runs, int n_runs, int cstart, int clen) {
    KpTargetSeq t;
    t.words = words; t.n_words = n_words; t.runs = runs; t.n_runs = n_runs; t.cstart = cstart; t.cend = cstart + clen;
    return t;
}

uint64_t kpy_al_nt(const uint32_t *words, int n_words, const int32_t *runs, int n_runs, int cstart, int clen, int start, int end, int strand) {
    return kp_al_nt_digest(target(words, n_words, runs, n_runs, cstart, clen), start, end, strand);
}

uint64_t kpy_al_nt_lanes(const uint32_t *words, int n_words, const int32_t *runs, int n_runs, int cstart, int clen, int start, int end, int strand,
                         int lanes) {
    const KpTargetSeq t = target(words, n_words, runs, n_runs, cstart, clen);
    int32_t s, e;
    if (!kp_al_interval(t, start, end, &s, &e)) return 0;
    const bool clear = kp_al_clear_of_runs(t, s, e);
    const int64_t nb = kp_al_nt_blocks((int64_t)e - s);
    std::vector<uint64_t> part((std::size_t)lanes, 0);
    for (int lane = 0; lane < lanes; ++lane)
        for (int64_t i = lane; i < nb; i += lanes) part[(std::size_t)lane] += kp_al_term(i, kp_al_nt_block(t, s, e, strand, i, clear));
    uint64_t S = 0;
    for (int lane = lanes - 1; lane >= 0; --lane) S += part[(std::size_t)lane];
    return kp_al_finish(S, KP_AL_TAG_NT, (uint64_t)((int64_t)e - s));
}

uint64_t kpy_al_aa(const uint8_t *p, int n) { return kp_al_aa_digest(p, n); }

uint64_t kpy_al_locus(const uint64_t *piece_digests, const int32_t *order, int n) { return kp_al_locus_digest(piece_digests, order, n); }

void kpy_al_layout(int32_t *out2) { out2[0] = (int32_t)sizeof(kp_allele); out2[1] = KP_AL_COLS; }

}  // extern "C"
