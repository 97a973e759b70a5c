// kp_caps.h -- buffer-size policy of an alignment pass and the reductions after it: what the options seed, what a context
// learns from its passes, how a list grows that a pass overflowed.  No HIP header: tests/native_harness builds it with g++.
#pragma once

#include <stdint.h>
#include <algorithm>
#include <string>
#include <vector>

constexpr uint32_t KP_CAPS_ANCHOR_SUBS = 64;  // KP_ANCHOR_SUBS of the scan (kp_internal.h; kp_host.h checks that they agree)

// most counting tables of the occurrence cut a pass may hold (kp_chain.hip: block_mid_occ); a batch in which more assemblies
// need their own mid_occ fails with KP_EOVERFLOW
constexpr uint32_t KP_OCC_SLOTS_MAX = 1u << 16;

// Buffer-size options of a context (KpOptions, kp_host.h): first guesses, until a pass has shown what it needs.
struct KpCapOptions {
    uint32_t anchor_cap = 1u << 17, tasks_per_asm = 4096, hit_cap = 4096;
    uint32_t trace_kb_per_asm = 2048;  // first guess for the DP trace buffer (a 5 Mbp K-locus assembly needs ~12 MB)
    uint64_t cand_cap = 0;             // first candidate list of a pass (entries); 0: sized from the batch (kp_caps_size)
    uint32_t group_cap = 1024, join_cap = 1024, occ_slots = 2;
    bool trace_set = false;            // trace_kb_per_asm was given (environment or kp_ctx_set_option): no floor under it
    uint32_t kept_cap = 256, piece_cap = 32, prot_cap = 32768;
    // first guess for the CIGAR ops of a pass, per hit (kp_caps_cigar_size).  Not measured: most hits of a typing run are one
    // M op and a hit with one indel has three, so four leaves room; a batch that needs more grows the buffer once
    uint32_t cigar_ops_per_hit = 4;
};

// learnt buffer sizes of a context (0 = not yet sized: first use takes the option's value); they only grow
struct KpLearnt {
    uint32_t anchor_cap = 0, hit_cap = 0;
    uint32_t tasks_per_asm = 0;  // task_cap of a pass = n_asm * tasks_per_asm
    double cand_frac = 0.0;      // cand_cap of a pass = total selected positions * cand_frac
    int64_t words_hw = 0;        // most packed words any batch of this context held: candidate lists are sized for that, so a
                                 // work set that meets a slightly larger batch than before does not re-allocate (and stall)
    uint64_t trace_units_per_asm = 0;  // trace buffer of a pass = n_asm * this many 16-byte units
    uint32_t group_cap = 0, join_cap = 0;  // group / join lists of a pass (entries; joins per band class)
    uint32_t occ_slots = 0;                // counting tables of the occurrence cut's quantile a pass may use (learnt like the list sizes)
    uint32_t cigar_ops_per_hit = 0;        // CIGAR ops buffer of a pass = its hits * this many ops
};

// what the buffers of a work set's most recent pass were sized for
struct KpPassCaps {
    uint32_t anchor_cap = 0, task_cap = 0, hit_cap = 0;
    uint64_t cand_cap = 0, trace_cap = 0;  // (trace: 16-byte units)
    uint32_t group_cap = 0, join_cap = 0, occ_slots = 0;
};

// what a pass counted (counters keep counting past their list's end, so they say how much room a clean rerun needs)
struct KpPassSeen {
    uint64_t n_cand = 0, trace_need = 0, occ_need = 0;  // (occ_need: assemblies that needed their mid_occ)
    uint32_t max_slice = 0, max_task = 0;  // fullest anchor sub-slice of any assembly; fullest task list of any band class
    uint32_t n_group = 0, max_join = 0;
    uint64_t n_asm = 0;
    int64_t total_words = 0;
};

// learnt sizes of the reduction buffers, per typing group
struct KpRunCaps { int kept_cap = 0, piece_cap = 0, prot_cap = 0; size_t pack_items = 0; /* most words kp_batch_typing packed */ };

// sizes of the pass's buffers from what the context has learnt so far (first use: the options)
inline void kp_caps_size(const KpCapOptions &opt, KpLearnt &L, int32_t n_asm, int64_t total_words, KpPassCaps &w) {
    if (L.anchor_cap == 0) L.anchor_cap = opt.anchor_cap;
    L.anchor_cap = std::max<uint32_t>((L.anchor_cap + KP_CAPS_ANCHOR_SUBS - 1) / KP_CAPS_ANCHOR_SUBS, 16u) * KP_CAPS_ANCHOR_SUBS;
    if (L.tasks_per_asm == 0) L.tasks_per_asm = opt.tasks_per_asm;
    if (L.cand_frac <= 0.0 && !opt.cand_cap) L.cand_frac = 0.004;  // 2 / 11 of the positions are seeds; ~1 % of those pass both filters
    if (L.hit_cap == 0) L.hit_cap = opt.hit_cap;
    w.anchor_cap = L.anchor_cap;
    w.task_cap = (uint32_t)std::min<uint64_t>((uint64_t)std::max(n_asm, 1) * L.tasks_per_asm, 1u << 28);
    L.words_hw = std::max(L.words_hw, total_words + total_words / 64);  // (batches of one stream differ by a per cent or so)
    // (an explicit cand_cap / trace_kb_per_asm is taken as it is: the floors below are for sizes guessed from the batch)
    const uint64_t cand_learnt = (uint64_t)((double)L.words_hw * 4.0 * L.cand_frac);
    w.cand_cap = opt.cand_cap ? std::max<uint64_t>(opt.cand_cap, cand_learnt) : std::max<uint64_t>(1 << 16, cand_learnt);
    w.hit_cap = L.hit_cap;
    if (L.trace_units_per_asm == 0) L.trace_units_per_asm = (uint64_t)opt.trace_kb_per_asm * 64;
    const uint64_t trace_units = (uint64_t)std::max(n_asm, 1) * L.trace_units_per_asm;
    w.trace_cap = opt.trace_set ? std::min<uint64_t>(trace_units, 1ull << 32) : std::max<uint64_t>(4096, trace_units);
    if (L.group_cap == 0) L.group_cap = opt.group_cap;
    if (L.join_cap == 0) L.join_cap = opt.join_cap;
    if (L.occ_slots == 0) L.occ_slots = std::min(opt.occ_slots, KP_OCC_SLOTS_MAX);
    w.group_cap = L.group_cap; w.join_cap = L.join_cap;
    w.occ_slots = std::max<uint32_t>(L.occ_slots, 1u);
}

// FITTED: the results are whole; GREW: a list overflowed and `w` has grown, run the pass again; OVERFLOW: one that cannot grow (`err`)
enum KpCapsVerdict { KP_CAPS_FITTED, KP_CAPS_GREW, KP_CAPS_OVERFLOW };
inline KpCapsVerdict kp_caps_after_pass(KpLearnt &L, KpPassCaps &w, const KpPassSeen &s, std::string &err) {
    const uint32_t sub_cap = w.anchor_cap / KP_CAPS_ANCHOR_SUBS;
    if (s.max_slice <= sub_cap && s.max_task <= w.task_cap && s.n_cand <= w.cand_cap && s.trace_need <= w.trace_cap &&
        s.n_group <= w.group_cap && s.max_join <= w.join_cap && s.occ_need <= w.occ_slots) {
        // Everything fitted.  What came close makes room for the passes after this one: the sub-slice an anchor
        // lands in depends on the order in which the scan's waves flushed, so the fullest slice varies from pass to
        // pass on the same input, and a rerun costs a whole pass.
        if (s.max_slice + s.max_slice / 4 > sub_cap)
            L.anchor_cap = std::max(L.anchor_cap, ((s.max_slice + s.max_slice / 2 + 15u) & ~15u) * KP_CAPS_ANCHOR_SUBS);
        if (s.trace_need + s.trace_need / 16 > w.trace_cap && s.trace_need + s.trace_need / 4 <= (1ull << 32))
            L.trace_units_per_asm = std::max<uint64_t>(L.trace_units_per_asm, (s.trace_need + s.trace_need / 4 + s.n_asm - 1) / std::max<uint64_t>(s.n_asm, 1));
        if ((uint64_t)s.max_task + s.max_task / 16 > w.task_cap)
            L.tasks_per_asm = std::max<uint32_t>(L.tasks_per_asm, (uint32_t)(((uint64_t)s.max_task + s.max_task / 4 + s.n_asm - 1) / std::max<uint64_t>(s.n_asm, 1)));
        if (s.n_cand + s.n_cand / 16 > w.cand_cap)
            L.cand_frac = std::max(L.cand_frac, (double)(s.n_cand + s.n_cand / 4) / ((double)s.total_words * 4.0));
        if (s.n_group + s.n_group / 4 > w.group_cap) L.group_cap = std::max(L.group_cap, 2 * s.n_group);
        if (s.max_join + s.max_join / 4 > w.join_cap) L.join_cap = std::max(L.join_cap, 2 * s.max_join);
        return KP_CAPS_FITTED;
    }
    // a region overflowed: counts kept counting, so they say how much room a clean rerun needs.  The context
    // remembers it (with some headroom, later batches differ a little) for every later pass.  The lists feed one
    // another and a stage behind an overflow counts on truncated input, so a pass may uncover one overflow after
    // another: there is another pass as long as this one grew a list (caps only grow, so this ends).
    bool grew = false;
    if (s.n_cand > w.cand_cap) {
        w.cand_cap = s.n_cand + s.n_cand / 8;
        L.cand_frac = std::max(L.cand_frac, (double)w.cand_cap / ((double)s.total_words * 4.0) * 1.0001);
        grew = true;
    }
    if (s.max_slice > sub_cap) {
        w.anchor_cap = ((s.max_slice + s.max_slice / 2 + 15u) & ~15u) * KP_CAPS_ANCHOR_SUBS;
        L.anchor_cap = std::max(L.anchor_cap, w.anchor_cap);
        grew = true;
    }
    if (s.trace_need > w.trace_cap) {  // (a pass cut short by another overflow reports less than it will need)
        if (s.trace_need > (1ull << 32)) { err = "DP trace would exceed 64 GB; use smaller batches"; return KP_CAPS_OVERFLOW; }
        w.trace_cap = std::min<uint64_t>(s.trace_need + s.trace_need / 4, 1ull << 32);  // later batches differ by a few per cent
        L.trace_units_per_asm = std::max<uint64_t>(L.trace_units_per_asm, (w.trace_cap + s.n_asm - 1) / std::max<uint64_t>(s.n_asm, 1));
        grew = true;
    }
    if (s.n_group > w.group_cap) { w.group_cap = s.n_group + s.n_group / 4 + 64; L.group_cap = std::max(L.group_cap, w.group_cap); grew = true; }
    if (s.occ_need > w.occ_slots) {
        L.occ_slots = std::max<uint32_t>(L.occ_slots, (uint32_t)std::min<uint64_t>(s.occ_need + s.occ_need / 4 + 1, KP_OCC_SLOTS_MAX));
        if (L.occ_slots <= w.occ_slots) {
            err = "occurrence-cut tables overflowed: " + std::to_string(s.occ_need) + " assemblies of the batch need their own mid_occ, at most " +
                  std::to_string(KP_OCC_SLOTS_MAX) + " tables; use smaller batches";
            return KP_CAPS_OVERFLOW;
        }
        grew = true;
    }
    if (s.max_join > w.join_cap) { w.join_cap = s.max_join + s.max_join / 4 + 64; L.join_cap = std::max(L.join_cap, w.join_cap); grew = true; }
    if (s.max_task > w.task_cap) {
        w.task_cap = (s.max_task + s.max_task / 8 + 1023u) & ~1023u;
        L.tasks_per_asm = std::max<uint32_t>(L.tasks_per_asm, (uint32_t)((w.task_cap + s.n_asm - 1) / std::max<uint64_t>(s.n_asm, 1)));
        grew = true;
    }
    if (!grew) { err = "alignment pass overflowed a list that could not grow"; return KP_CAPS_OVERFLOW; }  // (unreachable: every overflow above grows or fails)
    w.occ_slots = std::max(w.occ_slots, L.occ_slots);  // (the rerun's tables are the context's, whichever pass grew them; an occ_slots option set since the pass began waits for the next one)
    return KP_CAPS_GREW;
}

// an assembly produced (or a caller set) more hits than its region of the hit tables holds
inline void kp_caps_grow_hits(KpLearnt &L, KpPassCaps &w, uint32_t max_hits, bool headroom) {
    w.hit_cap = ((headroom ? max_hits + max_hits / 4 : max_hits) + 255u) & ~255u;  // a quarter of headroom: later batches differ a little
    L.hit_cap = std::max(L.hit_cap, w.hit_cap);
}

// CIGAR ops (kp_cigar.hip; only with the `cigar` option): the buffer of a pass holds total_hits * ops-per-hit entries, from what
// the context has learnt (first use: the option).  The emission counts every hit's ops before it writes them, so `need`
// is exact however small the buffer was.
inline uint64_t kp_caps_cigar_size(const KpCapOptions &opt, KpLearnt &L, uint64_t total_hits) {
    if (L.cigar_ops_per_hit == 0) L.cigar_ops_per_hit = std::max<uint32_t>(opt.cigar_ops_per_hit, 1u);
    return std::max<uint64_t>(total_hits, 1) * L.cigar_ops_per_hit;
}
// true: the ops fitted (what came close makes room for later passes); false: `cap` has grown -- write the ops again, nothing
// else: the alignment pass and its direction bits stand
inline bool kp_caps_after_cigar(KpLearnt &L, uint64_t &cap, uint64_t total_hits, uint64_t need) {
    const uint64_t hits = std::max<uint64_t>(total_hits, 1);
    auto per_hit = [&](uint64_t ops) { return (uint32_t)std::min<uint64_t>((ops + hits - 1) / hits, 0xFFFFFFFFu); };
    if (need <= cap) {
        if (need + need / 8 > cap) L.cigar_ops_per_hit = std::max(L.cigar_ops_per_hit, per_hit(need + need / 4));
        return true;
    }
    cap = need + need / 4;  // later batches differ a little
    L.cigar_ops_per_hit = std::max(L.cigar_ops_per_hit, per_hit(cap));
    return false;
}

// cs strings (kp_cs.hip; only with the `cs` option): the same policy for their bytes, with its option and what the context has
// learnt in a pair of their own.  The walk counts every hit's bytes before it writes them, so `need` is exact however small the
// buffer was.
struct KpCsCaps {
    // first guess for the bytes of a pass's cs strings, per hit.  Not measured when it was chosen: a clean hit is 5 bytes (":1234")
    // and a hit of 1000 columns at 1 % divergence about 75, so 64 is a guess between them; a batch that needs more grows the buffer once
    uint32_t bytes_per_hit = 64;
    uint32_t learnt = 0;  // cs byte buffer of a pass = its hits * this many bytes (0: not yet sized); only grows
};
inline uint64_t kp_caps_cs_size(KpCsCaps &c, uint64_t total_hits) {
    if (c.learnt == 0) c.learnt = std::max<uint32_t>(c.bytes_per_hit, 1u);
    return std::max<uint64_t>(total_hits, 1) * c.learnt;
}
// true: the bytes fitted (what came close makes room for later passes); false: `cap` has grown -- write the bytes again, nothing else
inline bool kp_caps_after_cs(KpCsCaps &c, uint64_t &cap, uint64_t total_hits, uint64_t need) {
    const uint64_t hits = std::max<uint64_t>(total_hits, 1);
    auto per_hit = [&](uint64_t bytes) { return (uint32_t)std::min<uint64_t>((bytes + hits - 1) / hits, 0xFFFFFFFFu); };
    if (need <= cap) {
        if (need + need / 8 > cap) c.learnt = std::max(c.learnt, per_hit(need + need / 4));
        return true;
    }
    cap = need + need / 4;  // later batches differ a little
    c.learnt = std::max(c.learnt, per_hit(cap));
    return false;
}
// kp_ctx_set_option of `cs_bytes_per_hit` (false: `name` is something else): it also resets what the context has learnt
inline bool kp_caps_set_cs_option(KpCsCaps &c, const std::string &n, int64_t value) {
    if (n != "cs_bytes_per_hit") return false;
    c.bytes_per_hit = (uint32_t)std::max<int64_t>(std::min<int64_t>(value, 0xFFFFFFFFll), 1);
    c.learnt = 0;
    return true;
}

// variant records of the kept hits (kp_variants.hip; only with the `variants` option): the same policy once more, per kept record.
// The walk counts every kept hit's records before it writes them, so `need` is exact however small the buffer was.
struct KpVarCaps {
    // first guess for the records of a reduction, per kept record.  A guess, not a measurement: a kept gene of 1000 bases at 1 %
    // divergence has about ten, a clean copy none, so 8 lies between them; a batch that needs more grows the buffer once
    uint32_t per_kept = 8;
    uint32_t learnt = 0;  // record buffer of a reduction = its kept records * this many (0: not yet sized); only grows
};
inline uint64_t kp_caps_variants_size(KpVarCaps &c, uint64_t total_kept) {
    if (c.learnt == 0) c.learnt = std::max<uint32_t>(c.per_kept, 1u);
    return std::max<uint64_t>(total_kept, 1) * c.learnt;
}
// true: the records fitted (what came close makes room for later batches); false: `cap` has grown -- write the records again, nothing else
inline bool kp_caps_after_variants(KpVarCaps &c, uint64_t &cap, uint64_t total_kept, uint64_t need) {
    const uint64_t kept = std::max<uint64_t>(total_kept, 1);
    auto per_kept = [&](uint64_t records) { return (uint32_t)std::min<uint64_t>((records + kept - 1) / kept, 0xFFFFFFFFu); };
    if (need <= cap) {
        if (need + need / 8 > cap) c.learnt = std::max(c.learnt, per_kept(need + need / 4));
        return true;
    }
    cap = need + need / 4;  // later batches differ a little
    c.learnt = std::max(c.learnt, per_kept(cap));
    return false;
}
// kp_ctx_set_option of `variants_per_kept` (false: `name` is something else): it also resets what the context has learnt
inline bool kp_caps_set_variants_option(KpVarCaps &c, const std::string &n, int64_t value) {
    if (n != "variants_per_kept") return false;
    c.per_kept = (uint32_t)std::max<int64_t>(std::min<int64_t>(value, 0xFFFFFFFFll), 1);
    c.learnt = 0;
    return true;
}

// overflow flags of a reduction (KpAsmSummary::overflow: 1 kept hits, 2 pieces, 8 proteins); false: `err` says what cannot grow
inline bool kp_caps_grow_run(KpRunCaps &c, int flags, std::string &err) {
    if (flags & 1) {
        if (c.kept_cap >= 2048) { err = "more than 2048 non-overlapping hits in one assembly"; return false; }
        c.kept_cap = std::min(c.kept_cap * 4, 2048);
    }
    if (flags & 2) c.piece_cap *= 4;
    if (flags & 8) c.prot_cap *= 4;
    return true;
}

// kp_ctx_set_option of a buffer-size option (false: `name` is none): it also resets what the context has learnt, so the
// next pass starts from the new value
inline bool kp_caps_set_option(KpCapOptions &o, KpLearnt &L, std::vector<KpRunCaps> &runs, const std::string &n, int64_t value) {
    const uint32_t v = (uint32_t)std::max<int64_t>(value, 1);
    if (n == "anchor_cap") { o.anchor_cap = v; L.anchor_cap = 0; }
    else if (n == "tasks_per_asm") { o.tasks_per_asm = v; L.tasks_per_asm = 0; }
    else if (n == "hit_cap") { o.hit_cap = v; L.hit_cap = 0; }
    else if (n == "trace_kb_per_asm") { o.trace_kb_per_asm = v; o.trace_set = true; L.trace_units_per_asm = 0; }
    else if (n == "cand_cap") { o.cand_cap = (uint64_t)std::max<int64_t>(value, 1); L.cand_frac = 0.0; }
    else if (n == "group_cap") { o.group_cap = v; L.group_cap = 0; }
    else if (n == "join_cap") { o.join_cap = v; L.join_cap = 0; }
    else if (n == "occ_slots") { o.occ_slots = (uint32_t)std::max<int64_t>(std::min<int64_t>(value, KP_OCC_SLOTS_MAX), 1); L.occ_slots = 0; }
    else if (n == "cigar_ops_per_hit") { o.cigar_ops_per_hit = v; L.cigar_ops_per_hit = 0; }
    else if (n == "kept_cap") { o.kept_cap = v; for (auto &c : runs) c.kept_cap = 0; }
    else if (n == "piece_cap") { o.piece_cap = v; for (auto &c : runs) c.piece_cap = 0; }
    else if (n == "prot_cap") { o.prot_cap = v; for (auto &c : runs) c.prot_cap = 0; }
    else return false;
    return true;
}

// most rows of a distance matrix (kp_dist_create; kp_spec.h, DISTANCES).  The pair kernel's grid holds one block per tile on or
// above the diagonal in its x dimension, 256 lanes each: with nt = ceil(rows / 64) tile rows that is nt (nt + 1) / 2 blocks.  HIP
// launches no grid whose gridDim.x * blockDim.x reaches 2^32, so the blocks must stay below 2^24: nt <= 5792, some 370 000 rows.
// 2^18 rows are nt = 4096 and 8 390 656 blocks, 2 148 007 936 work items -- half the limit (kp_dist_handle.h asserts it) --; the
// listing's count table then has rows * nt = 2^30 entries, indexed in 64 bits, and every tile index fits an int32.
constexpr int32_t KP_DIST_MAX_ROWS = 1 << 18;

// the packed edge key of a tree (kp_tree.h; kp_spec.h, TREE): differences << 36 | a << 18 | b, one 64-bit word that a single
// atomic minimum orders as the tuple.  Rows take KP_TREE_ROW_BITS each -- all of KP_DIST_MAX_ROWS fit --, which leaves
// KP_TREE_DIFF_BITS for the differences: a matrix of 16 * n_blocks >= KP_TREE_MAX_COLUMNS columns is refused by kp_dist_tree, and by
// it alone (the other calls of a handle keep kp_dist_create's limit of 2^31 columns).
constexpr int KP_TREE_ROW_BITS = 18, KP_TREE_DIFF_BITS = 28;
constexpr int64_t KP_TREE_MAX_COLUMNS = 1ll << KP_TREE_DIFF_BITS;
static_assert(KP_TREE_DIFF_BITS + KP_TREE_ROW_BITS + KP_TREE_ROW_BITS == 64, "28 + 18 + 18: the key fills one 64-bit word");
static_assert(KP_DIST_MAX_ROWS <= (1 << KP_TREE_ROW_BITS), "every row of the largest matrix must fit the key's row fields");

// most taxa of a neighbour-joining tree (kp_dist_nj; kp_spec.h, NJ).  The join loop keeps the dense matrix of the taxa on the
// device: n * n doubles, 2 GiB at 16384 taxa, beside the planes of the rows -- and its picks read some n^3 / 3 of them.  A matrix
// with more taxa is refused by kp_dist_nj, and by it alone, once the taxa are counted and before the matrix is allocated.
constexpr int32_t KP_NJ_MAX_TAXA = 16384;
static_assert((int64_t)KP_NJ_MAX_TAXA * KP_NJ_MAX_TAXA * 8 == (2ll << 30), "the dense matrix of the most taxa is 2 GiB");
static_assert(KP_NJ_MAX_TAXA <= 65535, "the taxa below a node are counted in 16 bits (kp_dist_nj_transfer; kp_spec.h, TRANSFER)");

// bootstrap support of that tree (kp_dist_nj_bootstrap; kp_spec.h, BOOTSTRAP).  The replicates of a call are joined in batches: the
// dense matrices of one batch together take no more than the one matrix of the largest tree may take already, so a batch is the
// largest b with b * n * n * 8 <= KP_BOOT_MATRIX_BYTES -- at least 1, at most the replicates, and at most KP_BOOT_MAX_BATCH, the
// rows of a grid: a replicate is blockIdx.y of every kernel of the batch (kp_boot.h: kp_boot_batch).  No result depends on it.
constexpr int32_t KP_BOOT_MAX_REPLICATES = 10000;
constexpr int64_t KP_BOOT_MATRIX_BYTES = (int64_t)KP_NJ_MAX_TAXA * KP_NJ_MAX_TAXA * 8;
constexpr int32_t KP_BOOT_MAX_BATCH = 65535;
