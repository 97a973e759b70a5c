// kp_variants.hip -- variant records of the KEPT hits (kp_spec.h, VARIANTS; only with the `variants` option).
//
// They follow the cs strings kernel for kernel (kp_cs.hip), on the reduction's stream behind the kernels that finalise the kept
// list, and read what the pass and the reduction left: the kept records, the finished hit table with its final ops and the two
// sequences.
//
//   kp_kept_locate           one lane per kept record: the hit behind it is found in the assembly's finished hit list -- by gene
//                            (kp_lower_bound_gene), then by span (kp_same_span; same-span hits are emitted once, so the match is
//                            unique) --, its row kept in `src`.  Once per reduction, for whichever pass reads the ops of the kept
//                            hits first: this one or the aligned rows (kp_aligned.hip)
//   kp_variants_walk<false>  one lane per kept record: its records counted
//   kp_launch_count_scan     the exclusive scan of the counts (kp_cigar.hip's, as it is): tens of thousands of kept records per
//                            batch, not the 1.16 M hits its one block is slow for
//   kp_variants_walk<true>   the same walk (kp_variants.h: one function, two sinks) stores the records from the hit's offset
//
// The record buffer is sized by the policy of kp_caps.h; the storing pass checks every store against its end, so a buffer that is
// too small loses records but nothing else, and the counts say how much room the repeat needs.  A lane's walk is as long as its
// hit has ops and differing columns -- lanes of a wave diverge, which a pass over a fortieth of the hits can afford; a record
// leaves its lane as three 8-byte stores (kp_variant_store).
#include <algorithm>

#include "kp_internal.h"
#include "kp_walk.h"
#include "kp_reduce_core.h"
#include "kp_variants.h"

namespace {

constexpr int VAR_THREADS = 64;

// The hit behind every kept record: src[row] = its row among the batch's finished hits (hit_off[a] + index), -1 where there is none.
__global__ __launch_bounds__(VAR_THREADS) void kp_kept_locate_kernel(int32_t n_asm, const kp_hit *__restrict__ hits, const uint32_t *__restrict__ n_hits,
                                                                     uint32_t hit_cap, const int64_t *__restrict__ hit_off,
                                                                     const kp_kept *__restrict__ kept, int kept_cap,
                                                                     const int64_t *__restrict__ kept_off, int64_t total_kept, int32_t gene_lo,
                                                                     int64_t *__restrict__ src) {
    for (int64_t row = (int64_t)blockIdx.x * VAR_THREADS + threadIdx.x; row < total_kept; row += (int64_t)gridDim.x * VAR_THREADS) {
        int a = 0;  // the assembly whose kept records hold this row: the last one with kept_off[a] <= row
        for (int z = n_asm; a + 1 < z;) {
            const int mid = (a + z) >> 1;
            if (kept_off[mid] <= row) a = mid; else z = mid;
        }
        const int i = (int)(row - kept_off[a]);
        int64_t at = -1;
        if (i < kept_cap) {  // (the host lays the rows out from counts that fitted the kept list)
            const kp_kept k = kept[(size_t)a * kept_cap + i];
            kp_hit probe;
            probe.gene = k.gene + gene_lo; probe.contig = k.contig; probe.strand = k.strand;
            probe.q_start = k.q_start; probe.q_end = k.q_end; probe.t_start = k.t_start; probe.t_end = k.t_end;
            const kp_hit *h = hits + (size_t)a * hit_cap;
            const int n = (int)min(n_hits[a], hit_cap);
            for (int j = kp_lower_bound_gene(h, n, probe.gene); j < n && h[j].gene == probe.gene; ++j)
                if (kp_same_span(h[j], probe)) { at = hit_off[a] + j; break; }
        }
        src[row] = at;
    }
}

template <bool EMIT>
__global__ __launch_bounds__(VAR_THREADS) void kp_variants_walk_kernel(KpBatchView b, KpGenes genes, const uint32_t *__restrict__ ops,
                                                                       const int64_t *__restrict__ cigar_off, int64_t ops_cap,
                                                                       const kp_kept *__restrict__ kept, int kept_cap,
                                                                       const int64_t *__restrict__ kept_off, int64_t total_kept, int32_t gene_lo,
                                                                       const int64_t *__restrict__ src, uint32_t *__restrict__ cnt,
                                                                       const int64_t *__restrict__ off, kp_variant *__restrict__ out, int64_t out_cap) {
    __shared__ uint8_t s_codon[128];
    if (threadIdx.x == 0) kp_fill_codon_table(s_codon);
    __syncthreads();
    for (int64_t row = (int64_t)blockIdx.x * VAR_THREADS + threadIdx.x; row < total_kept; row += (int64_t)gridDim.x * VAR_THREADS) {
        int a = 0;  // the assembly whose kept records hold this row: the last one with kept_off[a] <= row
        for (int z = b.n_asm; a + 1 < z;) {
            const int mid = (a + z) >> 1;
            if (kept_off[mid] <= row) a = mid; else z = mid;
        }
        const int i = (int)(row - kept_off[a]);
        if (i >= kept_cap) {  // (the host lays the rows out from counts that fitted the kept list)
            if (!EMIT) cnt[row] = 0;
            continue;
        }
        const kp_kept k = kept[(size_t)a * kept_cap + i];
        kp_hit probe;
        probe.gene = k.gene + gene_lo; probe.contig = k.contig; probe.strand = k.strand;
        probe.q_start = k.q_start; probe.q_end = k.q_end; probe.t_start = k.t_start; probe.t_end = k.t_end;
        const int64_t at = src[row];  // (kp_kept_locate_kernel)
        int64_t z0 = 0, z1 = 0;
        if (at >= 0) {
            z0 = cigar_off[at]; z1 = cigar_off[at + 1];
            if (z1 > ops_cap) z1 = ops_cap;  // (the ops are final when this runs: their buffer held them all)
            if (z0 > z1) z0 = z1;
        }
        const bool rev = k.strand < 0;
        const KpTaskSeqs s = kp_task_seqs(b, genes, a, probe.gene * 2 + (rev ? 1 : 0), k.contig);
        const KpQuerySeq fwd{genes.nib + genes.word_off[probe.gene], s.q.len};
        const int q0 = rev ? s.q.len - k.q_end : k.q_start, t0 = s.t.cstart + k.t_start;
        // the ops span the hit (kp_spec.h, CIGAR); a walk that would leave the gene or the contig reads nothing and gives no record
        int64_t rows = 0, cols = 0;
        for (int64_t z = z0; z < z1; ++z) {
            const uint32_t kind = ops[z] & 15u, len = ops[z] >> KP_CIGAR_SHIFT;
            if (kind != KP_CIGAR_D) rows += len;
            if (kind != KP_CIGAR_I) cols += len;
        }
        if (q0 < 0 || q0 + rows > s.q.len || k.t_start < 0 || t0 + cols > s.t.cend) z1 = z0;
        if (EMIT) {
            KpVarStore sink{out, off[row], off[row + 1] - off[row], out_cap, rev};
            kp_variants_hit(ops + z0, z1 - z0, s, fwd, q0, t0, rev, i, s_codon, sink);
        } else {
            KpVarCount sink;
            kp_variants_hit(ops + z0, z1 - z0, s, fwd, q0, t0, rev, i, s_codon, sink);
            cnt[row] = (uint32_t)sink.n;
        }
    }
}

dim3 var_grid(int64_t total) { return dim3((unsigned)std::min<int64_t>(std::max<int64_t>((total + VAR_THREADS - 1) / VAR_THREADS, 1), 4096)); }

}  // namespace

void kp_launch_kept_locate(const KpBatchView &b, const KpHitTable &hits, const KpHitRows &rows, const KpKeptRows &kept, int64_t *src, hipStream_t stream) {
    if (kept.total <= 0) return;
    hipLaunchKernelGGL(kp_kept_locate_kernel, var_grid(kept.total), dim3(VAR_THREADS), 0, stream, b.n_asm, hits.rows, hits.count, hits.cap, rows.hit_off,
                       kept.kept, kept.kept_cap, kept.kept_off, kept.total, kept.gene_lo, src);
}

void kp_launch_variants_walk(const KpBatchView &b, const KpGenes &genes, const KpPerHit<uint32_t> &cig, const KpKeptRows &kept, const int64_t *src,
                             const KpPerHit<kp_variant> &var, bool emit, hipStream_t stream) {
    if (kept.total <= 0) return;
    if (!emit) {
        hipLaunchKernelGGL(kp_variants_walk_kernel<false>, var_grid(kept.total), dim3(VAR_THREADS), 0, stream, b, genes, cig.data, cig.off, cig.cap,
                           kept.kept, kept.kept_cap, kept.kept_off, kept.total, kept.gene_lo, src, var.cnt, (const int64_t *)nullptr,
                           (kp_variant *)nullptr, (int64_t)0);
        return kp_launch_count_scan(var.cnt, kept.total, var.off, stream);
    }
    hipLaunchKernelGGL(kp_variants_walk_kernel<true>, var_grid(kept.total), dim3(VAR_THREADS), 0, stream, b, genes, cig.data, cig.off, cig.cap, kept.kept,
                       kept.kept_cap, kept.kept_off, kept.total, kept.gene_lo, src, (uint32_t *)nullptr, var.off, var.data, var.cap);
}
