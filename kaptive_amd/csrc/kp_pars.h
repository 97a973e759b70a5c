// kp_pars.h -- small parsimony of the columns of a matrix of locus rows on a neighbour-joining tree (kp_spec.h, PARSIMONY), written
// once as plain functions on plane words, 64 columns at a time: the set of a leaf, the set rule of a node of two and of three
// children with its step masks, the smallest code of a set, the state of a child under its parent's, the bit-sliced step counter,
// the check of a caller's record list, the place of a node's words in the node table, the record stores, and a serial restatement of
// the whole pass.  The kernels of kp_dist_pars.hip, the formatters (kp_rows.cpp) and the g++ harness share them.  No HIP header.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "kp_caps.h"
#include "kp_dist.h"
#include "kp_nj.h"

#define KP_PARS_STEP_PLANES 14 /* bit planes of a column's step counter: a tree of n taxa has at most n - 1 steps */
static_assert(KP_NJ_MAX_TAXA <= (1 << KP_PARS_STEP_PLANES), "the steps of a column of the largest tree fit the counter's planes");

// A SET of bases for each of the 64 columns of a plane word: bit j of s[k] says column j's set holds base k.
struct KpParsSet { uint64_t s[4]; };
// A STATE for each of the 64 columns: the two bits of its code.
struct KpParsState { uint64_t lo, hi; };

// The bases a row holds in one plane word (kp_dist.h, PLANES): bit j of s[k] says column j holds base k; N and GAP hold none.
KP_HD KpParsSet kp_pars_bases(uint64_t lo, uint64_t hi, uint64_t valid) {
    KpParsSet q;
    q.s[0] = valid & ~lo & ~hi;
    q.s[1] = valid & lo & ~hi;
    q.s[2] = valid & ~lo & hi;
    q.s[3] = valid & lo & hi;
    return q;
}
// LEAF SET: the base where the row holds one, every base where it holds none -- columns the matrix does not have among them.
KP_HD KpParsSet kp_pars_leaf(const KpParsSet &bases, uint64_t valid) {
    KpParsSet q;
    for (int k = 0; k < 4; ++k) q.s[k] = bases.s[k] | ~valid;
    return q;
}

// UP-PASS of a node of two children (Fitch): the intersection where it is not empty, otherwise the union and one step.
KP_HD KpParsSet kp_pars_join2(const KpParsSet &x, const KpParsSet &y, uint64_t *step) {
    uint64_t both[4], any = 0;
    for (int k = 0; k < 4; ++k) { both[k] = x.s[k] & y.s[k]; any |= both[k]; }
    KpParsSet q;
    for (int k = 0; k < 4; ++k) q.s[k] = (any & both[k]) | (~any & (x.s[k] | y.s[k]));
    *step = ~any;
    return q;
}
// UP-PASS of a node of three children (Hartigan): the bases most children hold; 3 - M steps, as *step1 + *step2 -- fewer than three
// agree, fewer than two agree.
KP_HD KpParsSet kp_pars_join3(const KpParsSet &x, const KpParsSet &y, const KpParsSet &z, uint64_t *step1, uint64_t *step2) {
    uint64_t all[4], two[4], a3 = 0, a2 = 0;
    for (int k = 0; k < 4; ++k) {
        all[k] = x.s[k] & y.s[k] & z.s[k];
        two[k] = (x.s[k] & y.s[k]) | (x.s[k] & z.s[k]) | (y.s[k] & z.s[k]);
        a3 |= all[k]; a2 |= two[k];
    }
    KpParsSet q;
    for (int k = 0; k < 4; ++k) q.s[k] = (a3 & all[k]) | (~a3 & a2 & two[k]) | (~a2 & (x.s[k] | y.s[k] | z.s[k]));
    *step1 = ~a3;
    *step2 = ~a2;
    return q;
}

// The SMALLEST CODE of a set that is not empty.
KP_HD KpParsState kp_pars_pick(const KpParsSet &q) {
    KpParsState t;
    t.lo = ~q.s[0] & (q.s[1] | ~q.s[2]);
    t.hi = ~q.s[0] & ~q.s[1];
    return t;
}
// DOWN-PASS: the columns in which the set holds the state.
KP_HD uint64_t kp_pars_holds(const KpParsSet &q, const KpParsState &t) {
    return (~t.hi & ~t.lo & q.s[0]) | (~t.hi & t.lo & q.s[1]) | (t.hi & ~t.lo & q.s[2]) | (t.hi & t.lo & q.s[3]);
}
// A child's state under its parent's: the parent's where the child's set holds it, the smallest code of the child's set elsewhere --
// and there, *change, the branch changes: the smallest code of a set that lacks the parent's state is another state.
KP_HD KpParsState kp_pars_child(const KpParsSet &q, const KpParsState &parent, uint64_t *change) {
    const uint64_t keep = kp_pars_holds(q, parent);
    const KpParsState own = kp_pars_pick(q);
    KpParsState t;
    t.lo = (keep & parent.lo) | (~keep & own.lo);
    t.hi = (keep & parent.hi) | (~keep & own.hi);
    *change = ~keep;
    return t;
}
KP_HD int32_t kp_pars_state_at(const KpParsState &t, int j) { return (int32_t)(((t.lo >> j) & 1ull) | (((t.hi >> j) & 1ull) << 1)); }

// STEPS.  64 counters of KP_PARS_STEP_PLANES bits, bit-sliced as KpSiteCounter is: bit j of p[b] is bit b of column j's steps.
// (A fixed trip count: the planes stay in registers where a loop that ends with the carry would index them.)
struct KpParsCounter { uint64_t p[KP_PARS_STEP_PLANES]; };
KP_HD void kp_pars_counter_add(KpParsCounter *c, uint64_t mask) {
    uint64_t carry = mask;
    for (int b = 0; b < KP_PARS_STEP_PLANES; ++b) {
        const uint64_t t = c->p[b] & carry;
        c->p[b] ^= carry;
        carry = t;
    }
}

// How many children the record has, and which.
KP_HD int kp_pars_children(const kp_nj_node &r) { return r.c >= 0 ? 3 : 2; }
KP_HD int32_t kp_pars_child_id(const kp_nj_node &r, int k) { return k == 0 ? r.a : (k == 1 ? r.b : r.c); }

// NODE TABLE.  The words of node v of a tree of n taxa lie [plane][word], behind those of the nodes before it: a leaf has three
// planes -- its state's two and its branch's change mask --, an inner node four: its set on the way up, and then the same three.
#define KP_PARS_LEAF_PLANES 3
#define KP_PARS_NODE_PLANES 4
#define KP_PARS_PLANE_LO 0
#define KP_PARS_PLANE_HI 1
#define KP_PARS_PLANE_CHANGE 2
KP_HD int64_t kp_pars_node_planes(int64_t v, int64_t n) { return v < n ? KP_PARS_LEAF_PLANES * v : KP_PARS_LEAF_PLANES * n + KP_PARS_NODE_PLANES * (v - n); }

// The taxa a record list of n_ref records is a tree of: n_ref + 2, but two for the one binary record, none for no record (-- one
// taxon has no record either: the caller's count decides).
inline int32_t kp_pars_taxa_of(const kp_nj_node *rec, int64_t n_ref) { return n_ref <= 0 ? 0 : (n_ref == 1 && rec[0].c < 0 ? 2 : (int32_t)(n_ref + 2)); }
// TREE.  The record list is a tree of n taxa in kp_dist_nj's form: kp_nj_records(n) records; a third child in the last record alone,
// and there unless n is 2; every child a node made before its record; every node but the last a child exactly once.  parent, if
// given, [n + n_ref]: every node's parent, -1 for the top.
inline bool kp_pars_tree_ok(const kp_nj_node *rec, int64_t n_ref, int32_t n, int32_t *parent) {
    if (n < 0 || n_ref != kp_nj_records(n) || (n_ref > 0 && !rec)) return false;
    std::vector<int32_t> up((size_t)(n + n_ref), -1);
    for (int64_t t = 0; t < n_ref; ++t) {
        const bool three = t == n_ref - 1 && n > 2;
        if (three != (rec[t].c >= 0) || (!three && rec[t].c != -1)) return false;
        for (int k = 0; k < (three ? 3 : 2); ++k) {
            const int32_t id = kp_pars_child_id(rec[t], k);
            if (id < 0 || id >= n + t || up[(size_t)id] >= 0) return false;
            up[(size_t)id] = (int32_t)(n + t);
        }
    }
    for (int64_t v = 0; v + 1 < n + n_ref; ++v)
        if (up[(size_t)v] < 0) return false;
    if (parent)
        for (int64_t v = 0; v < n + n_ref; ++v) parent[v] = up[(size_t)v];
    return true;
}

// two 8-byte words each, like every record the device stores
static_assert(sizeof(kp_pars_site) == 16 && sizeof(kp_pars_change) == 16 && offsetof(kp_pars_change, from) == 12 && offsetof(kp_pars_change, to) == 13, "a parsimony record is two 8-byte words");
KP_HD void kp_pars_site_store(kp_pars_site *p, int32_t column, int32_t steps, int32_t alleles) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long *d = reinterpret_cast<unsigned long long *>(p);
    d[0] = (uint64_t)(uint32_t)column | ((uint64_t)(uint32_t)steps << 32);
    d[1] = (uint64_t)(uint32_t)alleles;
#else
    p->column = column; p->steps = steps; p->alleles = alleles; p->pad_ = 0;
#endif
}
KP_HD void kp_pars_change_store(kp_pars_change *p, int32_t column, int32_t node, int32_t parent, int32_t from, int32_t to) {
#if defined(__HIP_DEVICE_COMPILE__)
    unsigned long long *d = reinterpret_cast<unsigned long long *>(p);
    d[0] = (uint64_t)(uint32_t)column | ((uint64_t)(uint32_t)node << 32);
    d[1] = (uint64_t)(uint32_t)parent | ((uint64_t)(uint32_t)(from & 255) << 32) | ((uint64_t)(uint32_t)(to & 255) << 40);
#else
    p->column = column; p->node = node; p->parent = parent; p->from = (uint8_t)from; p->to = (uint8_t)to; p->pad_ = 0;
#endif
}
KP_HD int32_t kp_pars_allele_count(int32_t alleles) { return (alleles & 1) + ((alleles >> 1) & 1) + ((alleles >> 2) & 1) + ((alleles >> 3) & 1); }

// The whole pass over a matrix of R rows of nb blocks, serially, one plane word at a time: the tree `rec` (n_ref records, checked by
// the caller) of the n taxa whose rows `taxa` names.  sites and changes are appended in the section's order.
inline void kp_pars_host(const uint64_t *blocks, int64_t nb, const int32_t *taxa, int32_t n, const kp_nj_node *rec, int64_t n_ref, std::vector<kp_pars_site> *sites,
                         std::vector<kp_pars_change> *changes) {
    if (n_ref <= 0) return;
    const int64_t NW = kp_dist_words(nb), nodes = n + n_ref;
    std::vector<int32_t> parent((size_t)nodes);
    if (!kp_pars_tree_ok(rec, n_ref, n, parent.data())) return;
    std::vector<KpParsSet> set((size_t)(nodes * NW));
    std::vector<KpParsState> state((size_t)(nodes * NW));
    std::vector<uint64_t> change((size_t)(nodes * NW), 0ull);
    for (int64_t w = 0; w < NW; ++w) {
        KpParsCounter steps;
        for (int b = 0; b < KP_PARS_STEP_PLANES; ++b) steps.p[b] = 0;
        uint64_t alleles[4] = {0, 0, 0, 0};
        for (int32_t k = 0; k < n; ++k) {
            const KpDistWord q = kp_dist_word_planes(blocks + (size_t)taxa[k] * (size_t)nb, nb, w);
            const KpParsSet bases = kp_pars_bases(q.lo, q.hi, q.valid);
            for (int c = 0; c < 4; ++c) alleles[c] |= bases.s[c];
            set[(size_t)(k * NW + w)] = kp_pars_leaf(bases, q.valid);
        }
        for (int64_t t = 0; t < n_ref; ++t) {
            const KpParsSet &x = set[(size_t)(rec[t].a * NW + w)], &y = set[(size_t)(rec[t].b * NW + w)];
            uint64_t s1 = 0, s2 = 0;
            if (rec[t].c >= 0) set[(size_t)((n + t) * NW + w)] = kp_pars_join3(x, y, set[(size_t)(rec[t].c * NW + w)], &s1, &s2);
            else set[(size_t)((n + t) * NW + w)] = kp_pars_join2(x, y, &s1);
            kp_pars_counter_add(&steps, s1);
            kp_pars_counter_add(&steps, s2);
        }
        state[(size_t)((nodes - 1) * NW + w)] = kp_pars_pick(set[(size_t)((nodes - 1) * NW + w)]);
        for (int64_t t = n_ref - 1; t >= 0; --t)
            for (int k = 0; k < kp_pars_children(rec[t]); ++k) {
                const int64_t v = kp_pars_child_id(rec[t], k);
                state[(size_t)(v * NW + w)] = kp_pars_child(set[(size_t)(v * NW + w)], state[(size_t)((n + t) * NW + w)], &change[(size_t)(v * NW + w)]);
            }
        for (int j = 0; j < 64; ++j) {
            int32_t s = 0, a = 0;
            for (int b = 0; b < KP_PARS_STEP_PLANES; ++b) s |= (int32_t)((steps.p[b] >> j) & 1ull) << b;
            for (int c = 0; c < 4; ++c) a |= (int32_t)((alleles[c] >> j) & 1ull) << c;
            if (s >= 1) {
                kp_pars_site r;
                kp_pars_site_store(&r, (int32_t)(64 * w + j), s, a);
                sites->push_back(r);
            }
        }
    }
    for (int64_t v = 0; v + 1 < nodes; ++v)
        for (int64_t w = 0; w < NW; ++w)
            for (int j = 0; j < 64; ++j)
                if ((change[(size_t)(v * NW + w)] >> j) & 1ull) {
                    kp_pars_change r;
                    kp_pars_change_store(&r, (int32_t)(64 * w + j), (int32_t)v, parent[(size_t)v], kp_pars_state_at(state[(size_t)(parent[(size_t)v] * NW + w)], j),
                                         kp_pars_state_at(state[(size_t)(v * NW + w)], j));
                    changes->push_back(r);
                }
}
