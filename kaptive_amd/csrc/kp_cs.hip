// kp_cs.hip -- cs difference strings of the finished hits (kp_spec.h, CS; only with the `cs` option).
//
// They follow the CIGARs kernel for kernel (kp_cigar.hip) and read what those left: the final ops of every hit, the hit tables
// and the two sequences -- never the trace buffer.
//
//   kp_cs_walk<false>   one lane per finished hit (grid and assembly loop of kp_cigar_walk_kernel): the bytes of its string, counted
//   kp_launch_count_scan  the exclusive scan of the counts (kp_cigar.hip's, as it is)
//   kp_cs_walk<true>    the same walk (kp_cs.h: one function, two sinks) writes the bytes forward from the hit's offset
//
// The byte buffer is sized by the policy of kp_caps.h; the writing pass checks every store against its end, so a buffer that is
// too small loses bytes but nothing else, and the counts say how much room the repeat needs.
#include <algorithm>

#include "kp_internal.h"
#include "kp_walk.h"
#include "kp_cs.h"

namespace {

constexpr int WALK_THREADS = 256;

template <bool EMIT>
__global__ __launch_bounds__(WALK_THREADS) void kp_cs_walk_kernel(KpBatchView b, KpGenes genes, const kp_hit *__restrict__ hits,
                                                                  const uint32_t *__restrict__ n_hits, uint32_t hit_cap,
                                                                  const int64_t *__restrict__ hit_off, const uint32_t *__restrict__ ops,
                                                                  const int64_t *__restrict__ cigar_off, int64_t ops_cap,
                                                                  uint32_t *__restrict__ cnt, const int64_t *__restrict__ off,
                                                                  char *__restrict__ bytes, int64_t bytes_cap) {
    for (int a = blockIdx.x; a < b.n_asm; a += gridDim.x) {
        const uint32_t n = min(n_hits[a], hit_cap);
        for (uint32_t i = threadIdx.x; i < n; i += WALK_THREADS) {
            const kp_hit h = hits[(size_t)a * hit_cap + i];
            const int64_t row = hit_off[a] + i;
            const int gs = h.gene * 2 + (h.strand < 0 ? 1 : 0);
            const KpTaskSeqs s = kp_task_seqs(b, genes, a, gs, h.contig);
            const int q0 = h.strand < 0 ? s.q.len - h.q_end : h.q_start, t0 = s.t.cstart + h.t_start;
            int64_t z0 = cigar_off[row], z1 = cigar_off[row + 1];
            if (z1 > ops_cap) z1 = ops_cap;  // (the ops are final when this runs: their buffer held them all)
            if (z0 > z1) z0 = z1;
            // the ops span the hit (kp_spec.h, CIGAR); a walk that would leave the gene or the contig reads nothing and writes ""
            int64_t rows = 0, cols = 0;
            for (int64_t z = z0; z < z1; ++z) {
                const uint32_t kind = ops[z] & 15u, len = ops[z] >> KP_CIGAR_SHIFT;
                if (kind != KP_CIGAR_D) rows += len;
                if (kind != KP_CIGAR_I) cols += len;
            }
            if (q0 < 0 || q0 + rows > s.q.len || h.t_start < 0 || t0 + cols > s.t.cend) z1 = z0;
            if (EMIT) {
                KpCsWrite out{bytes, off[row], bytes_cap};
                kp_cs_hit(ops + z0, z1 - z0, s, q0, t0, out);
            } else {
                KpCsCount out;
                kp_cs_hit(ops + z0, z1 - z0, s, q0, t0, out);
                cnt[row] = (uint32_t)out.n;
            }
        }
    }
}

dim3 walk_grid(const KpBatchView &b) { return dim3((unsigned)std::min(std::max(b.n_asm, 1), 4096)); }

}  // namespace

void kp_launch_cs_walk(const KpBatchView &b, const KpGenes &genes, const KpHitTable &hits, const KpHitRows &rows, const KpPerHit<uint32_t> &cig,
                       const KpPerHit<char> &cs, bool emit, hipStream_t stream) {
    if (!emit) {
        hipLaunchKernelGGL(kp_cs_walk_kernel<false>, walk_grid(b), dim3(WALK_THREADS), 0, stream, b, genes, hits.rows, hits.count, hits.cap, rows.hit_off,
                           cig.data, cig.off, cig.cap, cs.cnt, (const int64_t *)nullptr, (char *)nullptr, (int64_t)0);
        return kp_launch_count_scan(cs.cnt, rows.total, cs.off, stream);
    }
    hipLaunchKernelGGL(kp_cs_walk_kernel<true>, walk_grid(b), dim3(WALK_THREADS), 0, stream, b, genes, hits.rows, hits.count, hits.cap, rows.hit_off,
                       cig.data, cig.off, cig.cap, (uint32_t *)nullptr, cs.off, cs.data, cs.cap);
}
