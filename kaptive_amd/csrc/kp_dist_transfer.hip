// kp_dist_transfer.hip -- transfer bootstrap of the neighbour-joining tree of a distance handle (kp_spec.h, TRANSFER; the arithmetic:
// kp_transfer.h).  The weights, the matrices, the joins and the batches are kp_dist_nj_bootstrap's (kp_dist_boot.hip: dist_boot_run);
// this unit is what runs once a batch's records are made, and the entry point.
//
//   kp_transfer_member_kernel  once a call, a lane per taxon k: row k of the membership table starts as `turn` -- bit t set where the
//                              node of record t holds taxon 0 below it, so that A_t is the other side -- and the lane walks from its
//                              leaf up the parents and flips the bit of every record it passes.  A row is the lane's own.
//   kp_transfer_count_kernel   a lane per (replicate, supported split t); a replicate is blockIdx.y.  The lane walks the replicate's
//                              records u = 0 .. n - 4 in order: the taxa below node n + u and those of them in A_t are the sums over
//                              its two children, a leaf's being 1 and its membership bit.  Both ride in one 32-bit word -- the size in
//                              the high half, the count in the low: each is at most KP_NJ_MAX_TAXA < 2^16, so one add sums both and no
//                              carry crosses -- and the word of node n + u is entry [u][t] of the replicate's rows.  The rows lie in
//                              the replicate's own matrix block, which the joins are done with: (n - 3)^2 words of 4 bytes in n^2
//                              doubles.  A LANE READS ONLY WORDS IT WROTE ITSELF, in its own column t: no lane waits for another, and
//                              there is no barrier, no atomic and no grid-wide step in the loop.  Neighbouring lanes hold neighbouring
//                              t, so a row is read and written in whole lines.  The records and the children are the same for every
//                              lane of a replicate: scalar loads.  The running minimum of delta starts at depth - 1 and is stored once.
//   kp_transfer_sum_kernel     a lane per supported split: the batch's distances added to its sum in 64 bits, its zeros counted.
// Bounds: member [k < n][w < MW]; parent [v < n + records], its values -1 or above their index -- the host checks the supported tree's
// ids to lie below their record's node --; rows [u < S][t < S] with S = n - 3 and S * S * 4 <= n * n * 8; a replicate's record ids are
// checked by kp_transfer_below before they index anything; phi [rep < batch][t < records]; transfer, exact [t < S <= n_rows].
#include <algorithm>
#include <vector>

#include "kp_dist_handle.h"
#include "kp_transfer.h"

namespace {

constexpr int TRANSFER_THREADS = 64;  // one wave a workgroup: the walks are latency, and few lanes should spread over many units
static_assert((int64_t)(KP_NJ_MAX_TAXA - 3) * (KP_NJ_MAX_TAXA - 3) * 4 <= (int64_t)KP_NJ_MAX_TAXA * KP_NJ_MAX_TAXA * 8, "the rows of a replicate fit its matrix block");
static_assert(((int64_t)KP_NJ_MAX_TAXA << 16) + KP_NJ_MAX_TAXA < (1ll << 31), "size and count of a node share a 32-bit word");

__global__ __launch_bounds__(DIST_THREADS) void kp_transfer_member_kernel(const int32_t *__restrict__ parent, const uint32_t *__restrict__ turn, int32_t n, int32_t n_nodes,
                                                                          int32_t S, int32_t MW, uint32_t *__restrict__ member) {
    const int64_t k = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x;
    if (k >= n) return;
    uint32_t *row = member + (size_t)k * (size_t)MW;
    for (int32_t w = 0; w < MW; ++w) row[w] = turn[w];
    int32_t v = parent[k];
    for (int32_t steps = 0; v >= n && v < n_nodes && steps < n_nodes; ++steps) {  // (parents ascend: at most one step a node)
        const int32_t t = v - n;
        if (t < S) row[t >> 5] ^= 1u << (t & 31);
        v = parent[v];
    }
}

__global__ __launch_bounds__(TRANSFER_THREADS) void kp_transfer_count_kernel(const kp_nj_node *__restrict__ rec_all, int32_t n_rec, int32_t n, int32_t S, int32_t MW,
                                                                             const uint32_t *__restrict__ member, const int32_t *__restrict__ size, double *D_all,
                                                                             int64_t sD, int32_t *__restrict__ phi_all) {
    const int32_t t = (int32_t)blockIdx.x * TRANSFER_THREADS + (int32_t)threadIdx.x;
    if (t >= n_rec) return;
    int32_t *phi = phi_all + (size_t)blockIdx.y * (size_t)n_rec;
    if (t >= S) { phi[t] = -1; return; }
    const kp_nj_node *__restrict__ rec = rec_all + (size_t)blockIdx.y * (size_t)n_rec;
    uint32_t *__restrict__ rows = reinterpret_cast<uint32_t *>(D_all + (size_t)blockIdx.y * (size_t)sD);
    const int32_t s = size[t], w = t >> 5, bit = t & 31;
    int32_t best = kp_transfer_depth(s, n) - 1;
    for (int32_t u = 0; u < S; ++u) {
        const int32_t both = kp_transfer_below(
            rec[u], n, u, [member, MW, w, bit](int32_t k) { return (int32_t)(65536u | ((member[(size_t)k * (size_t)MW + (size_t)w] >> bit) & 1u)); },
            [rows, S, t](int32_t v) { return (int32_t)rows[(size_t)v * (size_t)S + (size_t)t]; });
        rows[(size_t)u * (size_t)S + (size_t)t] = (uint32_t)both;
        const int32_t d = kp_transfer_delta(s, both >> 16, both & 65535, n);
        best = d < best ? d : best;
    }
    phi[t] = best;
}

__global__ __launch_bounds__(DIST_THREADS) void kp_transfer_sum_kernel(const int32_t *__restrict__ phi, int32_t n_rec, int32_t S, int32_t b, unsigned long long *__restrict__ transfer,
                                                                       uint32_t *__restrict__ exact) {
    const int64_t t = (int64_t)blockIdx.x * DIST_THREADS + threadIdx.x;
    if (t >= S) return;
    unsigned long long sum = 0;
    uint32_t zeros = 0;
    for (int32_t r = 0; r < b; ++r) {
        const int32_t v = phi[(size_t)r * (size_t)n_rec + (size_t)t];
        sum += (unsigned long long)(v > 0 ? v : 0);
        zeros += v == 0 ? 1u : 0u;
    }
    transfer[t] += sum;
    exact[t] += zeros;
}

}  // namespace

int TransferPass::reserve(kp_ctx *ctx, kp_dist *d, int32_t n_taxa, int32_t batch) {
    n = n_taxa; n_rec = (int32_t)kp_nj_records(n); S = (int32_t)kp_boot_splits(n); MW = (S + 31) / 32;
    const size_t rows = (size_t)d->n_rows;
    return DistReserve()(d->boot.transfer, rows)(d->boot.exact, rows)(member, (size_t)n * (size_t)MW)(turn, (size_t)MW)(parent, (size_t)n + (size_t)n_rec)(size, (size_t)S)
        (phi, (size_t)batch * (size_t)n_rec).done(ctx, "transfer tables");
}

int TransferPass::begin(kp_ctx *ctx, kp_dist *d, const kp_nj_node *ref) {
    const int32_t n_nodes = n + n_rec;
    std::vector<int32_t> up((size_t)n_nodes, -1), below((size_t)S), zero((size_t)S), sz((size_t)S);
    std::vector<uint32_t> tn((size_t)MW, 0u);
    for (int32_t t = 0; t < n_rec; ++t) {
        const int32_t child[3] = {ref[t].a, ref[t].b, ref[t].c};
        for (int k = 0; k < (t == n_rec - 1 ? 3 : 2); ++k)
            if (child[k] >= 0 && child[k] < n + t) up[(size_t)child[k]] = n + t;
    }
    for (int32_t t = 0; t < S; ++t) {  // (a list in which a node is a child twice is no tree: its sums are kept from running away)
        below[(size_t)t] = std::min(n, kp_transfer_below(ref[t], n, t, [](int32_t) { return 1; }, [&below](int32_t v) { return below[(size_t)v]; }));
        zero[(size_t)t] = std::min(1, kp_transfer_below(ref[t], n, t, [](int32_t k) { return k == 0 ? 1 : 0; }, [&zero](int32_t v) { return zero[(size_t)v]; }));
        sz[(size_t)t] = zero[(size_t)t] ? n - below[(size_t)t] : below[(size_t)t];
        if (zero[(size_t)t]) tn[(size_t)(t >> 5)] |= 1u << (t & 31);
    }
    KP_HIP_CHECK(ctx, hipMemcpyAsync(parent.p, up.data(), up.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    KP_HIP_CHECK(ctx, hipMemcpyAsync(turn.p, tn.data(), tn.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    KP_HIP_CHECK(ctx, hipMemcpyAsync(size.p, sz.data(), sz.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    KP_HIP_CHECK(ctx, hipMemsetAsync(d->boot.transfer.p, 0, (size_t)S * sizeof(unsigned long long), ctx->stream));
    KP_HIP_CHECK(ctx, hipMemsetAsync(d->boot.exact.p, 0, (size_t)S * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(kp_transfer_member_kernel, dim3(dist_grid(n)), dim3(DIST_THREADS), 0, ctx->stream, parent.p, turn.p, n, n_nodes, S, MW, member.p);
    KP_HIP_CHECK(ctx, hipGetLastError());
    KP_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the host vectors go away)
    return KP_OK;
}

int TransferPass::batch(kp_ctx *ctx, kp_dist *d, const kp_nj_node *rec, double *D, int64_t sD, int32_t b) {
    if ((int64_t)S * S * 4 > sD * 8) return kp_fail(ctx, KP_ESTATE, "the rows of a replicate do not fit its matrix block");
    hipLaunchKernelGGL(kp_transfer_count_kernel, dim3((unsigned)((n_rec + TRANSFER_THREADS - 1) / TRANSFER_THREADS), (unsigned)b), dim3(TRANSFER_THREADS), 0, ctx->stream, rec,
                       n_rec, n, S, MW, member.p, size.p, D, sD, phi.p);
    hipLaunchKernelGGL(kp_transfer_sum_kernel, dim3(dist_grid(S)), dim3(DIST_THREADS), 0, ctx->stream, phi.p, n_rec, S, b, d->boot.transfer.p, d->boot.exact.p);
    KP_HIP_CHECK(ctx, hipGetLastError());
    return KP_OK;
}

int TransferPass::fetch(kp_ctx *ctx, kp_dist *d) {
    got_transfer.assign((size_t)S, 0);
    got_exact.assign((size_t)S, 0);
    KP_HIP_CHECK(ctx, hipMemcpyAsync(got_transfer.data(), d->boot.transfer.p, (size_t)S * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    KP_HIP_CHECK(ctx, hipMemcpyAsync(got_exact.data(), d->boot.exact.p, (size_t)S * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    return KP_OK;
}

extern "C" int kp_dist_nj_transfer(kp_ctx *ctx, kp_dist *d, int32_t min_compared, uint64_t seed, int32_t replicates, int32_t max_batch, const kp_nj_node *ref_nodes,
                                   int64_t n_ref, int32_t *support, int64_t cap_support, int64_t *transfer, int64_t cap_transfer, int32_t *per_replicate, int64_t cap_per,
                                   kp_nj_node *trees, int64_t cap_trees) {
    TransferPass pass;
    pass.transfer = transfer; pass.cap_transfer = cap_transfer; pass.per_replicate = per_replicate; pass.cap_per = cap_per;
    return dist_boot_run(ctx, d, min_compared, seed, replicates, max_batch, ref_nodes, n_ref, support, cap_support, trees, cap_trees, &pass);
}
