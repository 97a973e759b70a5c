"""The yardstick of the variable sites (include/kp_spec.h, SITES): a numpy restatement over the codes of ``tests.distances_util.unpack``
-- 0..3 a base, 4 an N, 5 GAP -- that shares nothing with kaptive_amd/csrc/kp_sites.h or kaptive_amd/distances.py.  The profile is a
comparison per class summed over the rows, a site a column with two non-zero base counts, a site row a fancy index; both tables are
f-strings.  Kaptive has no such output, so there is no reference implementation: equality with this file is exact."""

from __future__ import annotations

import ctypes as C

import numpy as np

from tests import distances_util as D

SITE_DTYPE = np.dtype([("column", "<i4"), ("n", "<i4", (4,)), ("n_n", "<i4")])
SITES_HEADER = b"Locus\tGene\tPosition\tColumn\tAssemblies\tA\tC\tG\tT\tN\tGap\tAlleles\tMajor\tInformative\n"
SNP_ALIGNMENT_HEADER = b"Locus\tAssembly\tSites\tAlignment\n"
CORE, THREADS, PLANES, LANE_ROWS, SLAB = 1, 256, 4, 15, 3840  # the constants the headers must hold
TEXT = "acgtn-"


def profile(codes) -> np.ndarray:
    """SITE_DTYPE records of every column of ``codes`` [R, columns]."""
    codes = np.asarray(codes, np.uint8)
    out = np.zeros(codes.shape[1], SITE_DTYPE)
    out["column"] = np.arange(codes.shape[1])
    for k in range(4):
        out["n"][:, k] = (codes == k).sum(axis=0)
    out["n_n"] = (codes == D.N).sum(axis=0)
    return out


def sites(codes, core: bool = False) -> np.ndarray:
    """The records of the sites, ascending in column."""
    codes = np.asarray(codes, np.uint8)
    p = profile(codes)
    keep = (p["n"] > 0).sum(axis=1) >= 2
    if core:
        keep &= (codes < 4).all(axis=0) if codes.shape[0] else False
    return p[keep]


def site_codes(codes, columns) -> np.ndarray:
    """Codes [R, S] of the rows at the listed columns."""
    return np.asarray(codes, np.uint8)[:, np.asarray(columns, np.int64)]


def site_blocks(codes, columns) -> np.ndarray:
    """uint64 [R, (S + 15) // 16]: the site rows, packed, GAP beyond S."""
    sc = site_codes(codes, columns)
    R, S = sc.shape
    padded = np.concatenate([sc, np.full((R, -S % 16), D.GAP, np.uint8)], axis=1)
    return D.pack(padded).reshape(R, -1) if R and S else np.zeros((R, (S + 15) // 16), np.uint64)


def alleles(n) -> int:
    return sum(1 for x in n if x > 0)


def major(n) -> int:
    return [int(x) for x in n].index(max(int(x) for x in n))


def informative(n) -> bool:
    return sum(1 for x in n if x >= 2) >= 2


def gene_of(gene_lengths, column: int):
    """(gene, 0-based position, 0-based column without padding) of a matrix column; None in padding or outside."""
    first = real = 0
    for g, L in enumerate(int(x) for x in gene_lengths):
        width = 16 * ((L + 15) // 16)
        if first <= column < first + width:
            pos = column - first
            return (g, pos, real + pos) if pos < L else None
        first += width
        real += L
    return None


def site_lines(locus: str, gene_names, gene_lengths, R: int, recs) -> bytes:
    out = []
    for s in recs:
        g, pos, col = gene_of(gene_lengths, int(s["column"]))
        n = [int(x) for x in s["n"]]
        gap = R - sum(n) - int(s["n_n"])
        out.append(f"{locus}\t{gene_names[g]}\t{pos + 1}\t{col + 1}\t{R}\t{n[0]}\t{n[1]}\t{n[2]}\t{n[3]}\t{int(s['n_n'])}\t{gap}\t{alleles(n)}\t{TEXT[major(n)]}\t"
                   f"{'yes' if informative(n) else 'no'}\n".encode())  # fmt: skip
    return b"".join(out)


def alignment_lines(locus: str, names, sc) -> bytes:
    """``sc``: codes [R, S]; no line for S = 0."""
    sc = np.asarray(sc)
    if sc.shape[1] == 0:
        return b""
    return b"".join(f"{locus}\t{names[r]}\t{sc.shape[1]}\t{''.join(TEXT[c] for c in sc[r])}\n".encode() for r in range(sc.shape[0]))


# ---- a whole run: a ``LocusRows`` (or anything with its loci / locus_matrix / db / ids) --------------------------------------------------
def _locus_genes(rows, L):
    g0 = int(rows.db.locus_gene_offsets[L])
    return g0, g0 + int(rows.db.locus_gene_lengths[L])


def run_sites(rows, core: bool = False) -> list:
    """[(locus, gene, position, column, (n0, n1, n2, n3), n_n)] with the database's gene index and 0-based coordinates."""
    out = []
    for L in rows.loci():
        idx, mat = rows.locus_matrix(L)
        g0, g1 = _locus_genes(rows, L)
        if len(idx) < 2:
            continue
        for s in sites(D.unpack(mat), core):
            g, pos, col = gene_of(rows.db.genes.lengths[g0:g1], int(s["column"]))
            out.append((L, g0 + g, pos, col, tuple(int(x) for x in s["n"]), int(s["n_n"])))
    return out


def run_sites_tsv(rows, core: bool = False) -> bytes:
    out = []
    for L in rows.loci():
        idx, mat = rows.locus_matrix(L)
        g0, g1 = _locus_genes(rows, L)
        if len(idx) >= 2:
            out.append(site_lines(rows.db.loci.ids[L], list(rows.db.genes.ids[g0:g1]), rows.db.genes.lengths[g0:g1], len(idx), sites(D.unpack(mat), core)))
    return b"".join(out)


def run_alignment_tsv(rows, core: bool = False) -> bytes:
    out = []
    for L in rows.loci():
        idx, mat = rows.locus_matrix(L)
        if len(idx) >= 2:
            codes = D.unpack(mat)
            out.append(alignment_lines(rows.db.loci.ids[L], [rows.ids[i] for i in idx], site_codes(codes, sites(codes, core)["column"])))
    return b"".join(out)


# ---- kp_sites.h under g++ ----------------------------------------------------------------------------------------------------------------
def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    h = build_harness("sites_harness", "kp_sites.h")
    h.kpy_sites_counter.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    h.kpy_sites_host.restype = C.c_int64
    h.kpy_site_gene.restype = C.c_int32
    h.kpy_site_derived.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    return h


def harness_sites(blocks_matrix, flags: int):
    """(profile [16 NB], sites, site rows [R, SB]) of a [R, NB] matrix of blocks through the header alone: planes, class masks,
    bit-sliced counters per lane, the transposition, the predicate, the block codes -- as the kernels use them."""
    m = np.ascontiguousarray(blocks_matrix, np.uint64)
    R, nb = m.shape
    prof, rec = np.zeros(16 * nb, SITE_DTYPE), np.zeros(16 * nb, SITE_DTYPE)
    rows = np.zeros((R, nb), np.uint64)
    S = harness().kpy_sites_host(_p(m), C.c_int32(R), C.c_int64(nb), C.c_int32(flags), _p(prof), _p(rec), _p(rows))
    assert S >= 0
    sb = (S + 15) // 16
    return prof, rec[:S].copy(), np.ascontiguousarray(rows.reshape(-1)[: R * sb].reshape(R, sb))
