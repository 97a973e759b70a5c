// kp_prot_cell.h -- the cell update of the protein Smith-Waterman-Gotoh, stated once for the kernels that fill such a matrix: the
// banded pair aligner (kp_prot.hip) and the translated search of the missing genes (kp_rescue.hip).  It restates the reference's
// _batched_banded_gotoh (src/kaptive/core/pairwise.py:395-584): BLOSUM62 via the 32 x 32 corner of its 256 x 256 lookup, gap open 11 +
// extend 1, opening a gap beats extending it, diagonal beats D (vertical) beats I (horizontal), best <= 0 restarts, the reported cell
// is the first maximum in row-major order, and matches / mismatches / gaps / start are what the reference's traceback loop would count.
// Device code only; everything lives in an unnamed namespace: each unit that includes it gets its own copy.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/kp_spec.h"

namespace {

constexpr int NEGP = KP_PROT_NEG_INF;
constexpr int GO = KP_PROT_GAP_OPEN + KP_PROT_GAP_EXT;
constexpr int GE = KP_PROT_GAP_EXT;

// Path statistics a DP state carries: a = matches << 16 | mismatches, g = gaps that consumed a query row << 16 | gaps that
// consumed a target column.  The start of the path is not carried (round 2 did: a third register through every select):
// a path that ends in (bi, bj) has consumed matches + mismatches + row gaps rows and matches + mismatches + column gaps
// columns, so start_i = bi - (m + mm + g_row) and start_j = bj - (m + mm + g_col) -- exactly what the reference's traceback
// would reach (it stops at the first cell whose M is 0, which is where the counts were reset here).
struct Pay {
    unsigned a, g;
};
constexpr unsigned GAP_ROW = 0x10000u, GAP_COL = 1u;

// one-lane wave shifts; the edge lane reads 0 (bound_ctrl) and is overridden by the caller where that matters
__device__ __forceinline__ int from_lower(int v) {  // lane b <- lane b-1
    return __builtin_amdgcn_mov_dpp(v, 0x138 /*wave_shr:1*/, 0xf, 0xf, true);
}
__device__ __forceinline__ int from_upper(int v) {  // lane b <- lane b+1
    return __builtin_amdgcn_mov_dpp(v, 0x130 /*wave_shl:1*/, 0xf, 0xf, true);
}

struct Result {
    int best, bi, bj;
    Pay bp;
};

struct PCell {
    int m, dv, iv;
    Pay pm, pd, pi;
};

__device__ __forceinline__ Pay pick(bool c, const Pay &x, const Pay &y) {
    return Pay{c ? x.a : y.a, c ? x.g : y.g};
}

// one cell (i, j); `left` = (i, j-1): its M, I and their payloads; `up` = (i-1, j): its M, D and their payloads; the
// diagonal neighbour (i-1, j-1) comes in as c.m / c.pm.  Same statements as the reference's kernel (see top), written
// as selects: every lane executes the same instructions whatever its cell decides.
template <bool ROW_MAJOR = true>  // false: the lane does not visit its cells in row-major order and ties are settled by (i, j)
__device__ __forceinline__ void prot_cell(PCell &c, Result &r, bool in, int i, int j, unsigned c1, unsigned c2,
                                          const int8_t *s_mat, int lm, int li, Pay lpm, Pay lpi, int um, int ud, Pay upm,
                                          Pay upd) {
    // D: gap arriving from above.  (A path starts at a cell whose M is 0: such a cell keeps the payload of its M state at
    // zero -- the last statement below --, so none of its three readers has to ask.)
    const int d_open = um - GO, d_ext = ud - GE;
    int ndv = max(d_open, d_ext);
    Pay npd = pick(d_open >= d_ext, upm, upd);
    npd.g += GAP_ROW;
    // I: gap arriving from the left
    const int i_open = lm - GO, i_ext = li - GE;
    int niv = max(i_open, i_ext);
    Pay npi = pick(i_open >= i_ext, lpm, lpi);
    npi.g += GAP_COL;
    // M: diagonal first, then D, then I, each only if strictly better
    Pay npm = c.pm;
    const unsigned x1 = c1 & 255u, x2 = c2 & 255u;
    const int sc = (int)s_mat[x1 * 32 + x2];  // (index 31 = a byte outside the alphabet: its row and column hold KP_PROT_FILL)
    int bv = c.m + sc;
    npm.a += ((c1 >> 8) == (c2 >> 8)) ? 0x10000u : 1u;
    const bool take_d = ndv > bv;
    bv = max(bv, ndv);
    npm = pick(take_d, npd, npm);
    const bool take_i = niv > bv;
    bv = max(bv, niv);
    npm = pick(take_i, npi, npm);
    // cells outside the matrix or the band take boundary values, exactly as the reference's band array holds them
    const int nm = in ? max(bv, 0) : 0;
    // the first maximum in row-major order: a lane's cells come in that order (strict rise), or the tie is looked at
    if (nm > r.best || (!ROW_MAJOR && nm == r.best && nm > 0 && (i < r.bi || (i == r.bi && j < r.bj)))) {
        r.best = nm; r.bi = i; r.bj = j; r.bp = npm;
    }
    c.m = nm; c.dv = in ? ndv : NEGP; c.iv = in ? niv : NEGP;
    c.pm = pick(nm == 0, Pay{0, 0}, npm); c.pd = npd; c.pi = npi;
}

// The same cell without the path statistics: the three scores and the best cell, nothing else.  Every value it produces is the one
// prot_cell produces for the cell -- the payloads decide nothing --, so a fill with it finds the same first maximum.  m comes in
// holding the diagonal neighbour's M and goes out holding the cell's; dv and iv go out likewise.
struct LeanBest {
    int best, bi, bj;
};
template <bool ROW_MAJOR = true>
__device__ __forceinline__ void prot_cell_lean(int &m, int &dv, int &iv, LeanBest &r, bool in, int i, int j, unsigned c1, unsigned c2,
                                               const int8_t *s_mat, int lm, int li, int um, int ud) {
    const int ndv = max(um - GO, ud - GE), niv = max(lm - GO, li - GE);
    const int bv = max(max(m + (int)s_mat[(c1 & 255u) * 32 + (c2 & 255u)], ndv), niv);
    const int nm = in ? max(bv, 0) : 0;
    if (nm > r.best || (!ROW_MAJOR && nm == r.best && nm > 0 && (i < r.bi || (i == r.bi && j < r.bj)))) {
        r.best = nm; r.bi = i; r.bj = j;
    }
    m = nm; dv = in ? ndv : NEGP; iv = in ? niv : NEGP;
}

// compact substitution table in LDS: s_idx = index of each byte in ARNDCQEGHILKMFPSTWYVBJZX* (31 for everything else),
// s_mat = the 32 x 32 corner of the reference's 256 x 256 lookup those indices address
__device__ __forceinline__ void stage_blosum(const int8_t *__restrict__ blosum, int8_t *s_mat, uint8_t *s_idx, int lane) {
    for (int c = lane; c < 256; c += 64) s_idx[c] = 31;
    __syncthreads();
    if (lane < 25) s_idx[(uint8_t)"ARNDCQEGHILKMFPSTWYVBJZX*"[lane]] = (uint8_t)lane;
    __syncthreads();
    for (int x = lane; x < 32 * 32; x += 64) {
        const int a = x >> 5, c = x & 31;
        s_mat[x] = (a < 25 && c < 25) ? blosum[(int)(uint8_t)"ARNDCQEGHILKMFPSTWYVBJZX*"[a] * 256 +
                                               (int)(uint8_t)"ARNDCQEGHILKMFPSTWYVBJZX*"[c]]
                                      : (int8_t)KP_PROT_FILL;
    }
    __syncthreads();
}

}  // namespace
