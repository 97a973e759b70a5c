// kp_alleles.hip -- allele digests of the kept records and the locus pieces (kp_spec.h, ALLELES; made when they are first asked for).
//
// On the reduction's stream, behind the kernels that finalise the kept list.  One kernel reads the kept records, the pieces, the
// translated proteins and the packed contigs with their N runs: no hit table, no op, no trace.
//
//   kp_alleles_kernel   one wave per interval row, grid-strided: the kept rows of every assembly (KpKeptRows), then the piece rows of
//                       every assembly.  Lanes take the blocks lane, lane + 64, ... of the interval (kp_alleles.h: sixteen columns
//                       from two neighbouring packed words; a sweep of the wave is 1024 bases), mix them and keep a partial sum; a
//                       64-bit butterfly adds the lanes' sums.  A wave-uniform look at the N runs lets an interval that no run
//                       touches -- nearly every one -- skip the mask.  For a kept row the same wave then digests the protein bytes,
//                       eight per lane.  Lane 0 stores the record: two 8-byte words for a kept row, one for a piece row.
//
// One record per row is exact, so no buffer can overflow and nothing is retried.  A row whose interval does not lie inside its contig
// (or whose protein does not lie inside the assembly's buffer) reads nothing and leaves digest 0.
#include <algorithm>

#include "kp_internal.h"
#include "kp_alleles.h"

namespace {

constexpr int AL_THREADS = 256;  // four waves, each with rows of its own
constexpr int AL_WAVE = 64;

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the last a with off[a] <= row, a < n_asm
__device__ __forceinline__ int asm_of_row(const int64_t *__restrict__ off, int n_asm, int64_t row) {
    int a = 0;
    for (int z = n_asm; a + 1 < z;) {
        const int mid = (a + z) >> 1;
        if (off[mid] <= row) a = mid; else z = mid;
    }
    return a;
}

__global__ __launch_bounds__(AL_THREADS) void kp_alleles_kernel(KpBatchView b, const kp_kept *__restrict__ kept, int kept_cap,
                                                                const int64_t *__restrict__ kept_off, int64_t total_kept,
                                                                const kp_piece *__restrict__ pieces, int piece_cap,
                                                                const int64_t *__restrict__ piece_off, int64_t total_pieces,
                                                                const uint8_t *__restrict__ prot, int prot_cap, kp_allele *__restrict__ out,
                                                                uint64_t *__restrict__ piece_out) {
    const int lane = threadIdx.x & (AL_WAVE - 1);
    const int64_t n_waves = (int64_t)gridDim.x * (AL_THREADS / AL_WAVE), total = total_kept + total_pieces;
    for (int64_t row = (int64_t)blockIdx.x * (AL_THREADS / AL_WAVE) + threadIdx.x / AL_WAVE; row < total; row += n_waves) {
        const bool is_kept = row < total_kept;
        int a, contig, start, end, strand;
        int64_t p_off = 0, p_len = 0;
        if (is_kept) {
            a = asm_of_row(kept_off, b.n_asm, row);
            const int i = (int)(row - kept_off[a]);
            if (i >= kept_cap) {  // (the host lays the rows out from counts that fitted the kept list)
                if (lane == 0) { out[row].nt = 0; out[row].aa = 0; }
                continue;
            }
            const kp_kept &k = kept[(size_t)a * kept_cap + i];
            contig = k.contig; start = k.t_start; end = k.t_end; strand = k.strand;
            p_off = k.prot_off; p_len = k.prot_len;
        } else {
            const int64_t prow = row - total_kept;
            a = asm_of_row(piece_off, b.n_asm, prow);
            const int i = (int)(prow - piece_off[a]);
            if (i >= piece_cap) {
                if (lane == 0) piece_out[prow] = 0;
                continue;
            }
            const kp_piece &p = pieces[(size_t)a * piece_cap + i];
            contig = p.contig; start = p.start; end = p.end; strand = p.strand;
        }
        const int c0 = b.asm_first_ctg[a], n_ctg = b.asm_first_ctg[a + 1] - c0;
        uint64_t nt = 0;
        if (contig >= 0 && contig < n_ctg) {
            KpTargetSeq t;
            const int r0 = b.asm_first_nrun[a];
            t.words = b.words + b.asm_word_off[a];
            t.n_words = (int)(b.asm_word_off[a + 1] - b.asm_word_off[a]);  // (every position below is checked against it: kp_al_interval)
            t.runs = b.n_runs + 2 * (size_t)r0;
            t.n_runs = b.asm_first_nrun[a + 1] - r0;
            t.cstart = b.ctg_start[c0 + contig];
            t.cend = t.cstart + b.ctg_len[c0 + contig];
            int32_t s, e;
            if (kp_al_interval(t, start, end, &s, &e)) {  // (uniform: the whole wave reads the same row)
                const bool clear = kp_al_clear_of_runs(t, s, e);
                const int64_t nb = kp_al_nt_blocks((int64_t)e - s);
                uint64_t S = 0;
                for (int64_t i = lane; i < nb; i += AL_WAVE) S += kp_al_term(i, kp_al_nt_block(t, s, e, strand, i, clear));
                nt = kp_al_finish(wave_sum(S), KP_AL_TAG_NT, (uint64_t)((int64_t)e - s));
            }
        }
        if (!is_kept) {
            if (lane == 0) piece_out[row - total_kept] = nt;
            continue;
        }
        uint64_t aa = 0;
        if (p_len > 0 && p_off >= 0 && p_off + p_len <= prot_cap) {
            const uint8_t *p = prot + (size_t)a * (size_t)prot_cap + p_off;
            const int64_t nb = kp_al_aa_blocks(p_len);
            uint64_t S = 0;
            for (int64_t i = lane; i < nb; i += AL_WAVE) S += kp_al_term(i, kp_al_aa_block(p, p_len, i));
            aa = kp_al_finish(wave_sum(S), KP_AL_TAG_AA, (uint64_t)p_len);
        }
        if (lane == 0) {
            unsigned long long *d = reinterpret_cast<unsigned long long *>(out + row);
            d[0] = nt; d[1] = aa;
        }
    }
}

}  // namespace

void kp_launch_alleles(const KpBatchView &b, const KpKeptRows &kept, const KpPieceRows &pieces, const uint8_t *prot, int prot_cap, kp_allele *out,
                       uint64_t *piece_out, hipStream_t stream) {
    const int64_t total = kept.total + pieces.total;
    if (b.n_asm <= 0 || total <= 0) return;
    constexpr int per_block = AL_THREADS / AL_WAVE;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + per_block - 1) / per_block, 2048);
    hipLaunchKernelGGL(kp_alleles_kernel, dim3(blocks), dim3(AL_THREADS), 0, stream, b, kept.kept, kept.kept_cap, kept.kept_off, kept.total, pieces.pieces,
                       pieces.piece_cap, pieces.piece_off, pieces.total, prot, prot_cap, out, piece_out);
}
