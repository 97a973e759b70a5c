"""Shared by tests/test_variants_cpu.py and tests/test_gpu_variants.py: the yardstick of the variant records (include/kp_spec.h,
VARIANTS) -- a Python restatement written straight from the spec, column by column, that shares nothing with
kaptive_amd/csrc/kp_variants.h --, a second, independent route that reads the same records off a cs string, a Python formatter of
the table, and the g++ build of kp_variants.h on host arrays.  The codon table is the one of the Python translation
(kaptive_amd/core/seq.py), not the C header's.  TEST INFRASTRUCTURE."""

from __future__ import annotations

import ctypes as C
from functools import lru_cache

import numpy as np

from kaptive_amd._native import VARIANT_DTYPE
from kaptive_amd.core.seq import CODON_MAP
from tests import cs_util as S

M, I, D = S.M, S.I, S.D
SNV, INS, DEL = 0, 1, 2
LETTERS = "acgtn"
HEADER = b"\t".join([b"Assembly", b"Contig", b"Position", b"Strand", b"Gene", b"Gene position", b"Type", b"Length", b"Ref", b"Alt", b"Codon",
                     b"Ref aa", b"Alt aa", b"Effect"]) + b"\n"  # fmt: skip


def comp(c: int) -> int:
    return 3 - c if c <= 3 else 4


def revcomp_codes(g) -> np.ndarray:
    g = np.asarray(g, np.uint8)
    return np.ascontiguousarray(np.where(g < 4, 3 - g, g)[::-1], np.uint8)


def _aa(codon) -> int:
    a, b, c = (min(int(x), 4) for x in codon)
    return int(CODON_MAP[a * 25 + b * 5 + c])


def _consequence(gene_fwd, q_pos: int, alt: int):
    """(ref_aa, alt_aa) of the one base replaced in the unmodified codon q_pos // 3 of the gene's forward sequence; a codon the
    gene's end cuts short is X on both sides."""
    c0 = q_pos // 3 * 3
    if c0 + 3 > len(gene_fwd):
        return ord("X"), ord("X")
    codon = [int(x) for x in gene_fwd[c0 : c0 + 3]]
    ref_aa = _aa(codon)
    codon[q_pos - c0] = alt
    return ref_aa, _aa(codon)


def _table(recs) -> np.ndarray:
    out = np.zeros(len(recs), VARIANT_DTYPE)
    for i, r in enumerate(recs):
        out[i] = (*r, (0, 0, 0))
    return out


def records_from_ops(ops, gene_fwd, asm_codes, strand: int, q_start: int, q_end: int, t_abs: int, cstart: int, kept: int = 0) -> np.ndarray:
    """The records of a hit, column by column from its ops: ``gene_fwd`` are the gene's forward codes (0..3, 4 = n), ``asm_codes`` the
    assembly's, ``[q_start, q_end)`` the hit's span on the gene's forward strand, ``t_abs`` its first column in the assembly's
    space and ``cstart`` the contig's."""
    gene_fwd = np.asarray(gene_fwd, np.uint8)
    n_gene = len(gene_fwd)
    aligned = gene_fwd if strand > 0 else revcomp_codes(gene_fwd)
    r, t = (int(q_start) if strand > 0 else n_gene - int(q_end)), int(t_abs)
    recs = []
    for op in np.asarray(ops).tolist():
        kind, n = op & 15, op >> 4
        if kind == M:
            for j in range(n):
                qc, tc = int(aligned[r + j]), int(asm_codes[t + j])
                if qc <= 3 and tc <= 3 and qc == tc:
                    continue
                q_pos = r + j if strand > 0 else n_gene - 1 - (r + j)
                ref, alt = min(int(gene_fwd[q_pos]), 4), (min(tc, 4) if strand > 0 else comp(tc))
                recs.append((kept, q_pos, t + j - cstart, 1, SNV, ref, alt, *_consequence(gene_fwd, q_pos, alt)))
            r += n
            t += n
        elif kind == I:  # the gene's rows r .. r + n have no column: a deletion in the contig
            recs.append((kept, r if strand > 0 else n_gene - (r + n), t - cstart, n, DEL, 0, 0, 0, 0))
            r += n
        else:  # the contig's columns t .. t + n lie between the rows r - 1 and r: an insertion
            assert kind == D, f"op kind {kind}"
            recs.append((kept, r if strand > 0 else n_gene - r, t - cstart, n, INS, 0, 0, 0, 0))
            t += n
    if strand < 0:
        recs.reverse()
    return _table(recs)


def records_from_cs(cs: bytes, gene_fwd, strand: int, q_start: int, q_end: int, t_abs: int, cstart: int, kept: int = 0) -> np.ndarray:
    """The same records read off the hit's cs string (kp_spec.h, CS): one per *, + and - token.  The bases come from the string's
    letters; the gene is read for the codon only."""
    gene_fwd = np.asarray(gene_fwd, np.uint8)
    n_gene = len(gene_fwd)
    r, t = (int(q_start) if strand > 0 else n_gene - int(q_end)), int(t_abs)
    recs = []
    for tok in S.TOKEN.findall(cs):
        head, body = tok[:1], tok[1:].decode()
        if head == b":":
            r += int(body)
            t += int(body)
        elif head == b"*":
            tc, qc = LETTERS.index(body[0]), LETTERS.index(body[1])
            q_pos = r if strand > 0 else n_gene - 1 - r
            ref, alt = (qc, tc) if strand > 0 else (comp(qc), comp(tc))
            recs.append((kept, q_pos, t - cstart, 1, SNV, ref, alt, *_consequence(gene_fwd, q_pos, alt)))
            r += 1
            t += 1
        elif head == b"+":
            n = len(body)
            recs.append((kept, r if strand > 0 else n_gene - (r + n), t - cstart, n, DEL, 0, 0, 0, 0))
            r += n
        else:
            n = len(body)
            recs.append((kept, r if strand > 0 else n_gene - r, t - cstart, n, INS, 0, 0, 0, 0))
            t += n
    if strand < 0:
        recs.reverse()
    return _table(recs)


def effect(v) -> bytes:
    if v["kind"] != SNV:
        return b"frameshift" if int(v["len"]) % 3 else b"inframe"
    if v["ref"] > 3 or v["alt"] > 3:
        return b"ambiguous"
    if v["ref_aa"] == v["alt_aa"]:
        return b"synonymous"
    if v["alt_aa"] == ord("*"):
        return b"nonsense"
    if v["ref_aa"] == ord("*"):
        return b"stop_lost"
    return b"missense"


def format_tsv(asm_names, contig_names, gene_names, kept, records, var_off) -> bytes:
    """The lines of the variant table (no header): ``contig_names[a]`` are assembly a's, ``kept[a]`` its kept records."""
    lines = []
    for a, name in enumerate(asm_names):
        for v in records[var_off[a] : var_off[a + 1]]:
            k = kept[a][int(v["kept"])]
            cols = [str(name).encode(), str(contig_names[a][int(k["contig"])]).encode(), b"%d" % (int(v["t_pos"]) + 1), b"-" if k["strand"] < 0 else b"+",
                    str(gene_names[int(k["gene"])]).encode(), b"%d" % (int(v["q_pos"]) + 1), (b"snv", b"ins", b"del")[int(v["kind"])], b"%d" % int(v["len"])]  # fmt: skip
            if v["kind"] == SNV:
                cols += [LETTERS[min(int(v["ref"]), 4)].encode(), LETTERS[min(int(v["alt"]), 4)].encode(), b"%d" % (int(v["q_pos"]) // 3 + 1),
                         bytes([int(v["ref_aa"])]), bytes([int(v["alt_aa"])])]  # fmt: skip
            else:
                cols += [b"."] * 5
            lines.append(b"\t".join(cols + [effect(v)]) + b"\n")
    return b"".join(lines)


def kept_yardstick(kept_row, hits, ops, coff, row0, gene_codes, gene_off, pa, asm_codes, gene_lo=0, cs=None, csoff=None, index=0):
    """The records of one kept record of an assembly: the hit behind it is the one row of the assembly's hits ``hits`` (rows of
    the batch's table from ``row0`` on) with its gene and span; its ops -- or, with ``cs``, its cs string -- give the records."""
    g = int(kept_row["gene"]) + gene_lo
    same = np.flatnonzero((hits["gene"] == g) & (hits["contig"] == kept_row["contig"]) & (hits["strand"] == kept_row["strand"])
                          & (hits["q_start"] == kept_row["q_start"]) & (hits["q_end"] == kept_row["q_end"])
                          & (hits["t_start"] == kept_row["t_start"]) & (hits["t_end"] == kept_row["t_end"]))  # fmt: skip
    assert len(same) == 1, f"kept record {kept_row}: {len(same)} hits with its span"
    i = row0 + int(same[0])
    gene = gene_codes[gene_off[g] : gene_off[g + 1]]
    cstart = int(pa.ctg_start[kept_row["contig"]])
    args = (int(kept_row["strand"]), int(kept_row["q_start"]), int(kept_row["q_end"]), cstart + int(kept_row["t_start"]), cstart, index)
    if cs is not None:
        return records_from_cs(cs[csoff[i] : csoff[i + 1]], gene, *args)
    return records_from_ops(ops[coff[i] : coff[i + 1]], gene, asm_codes, *args)


# ---- kp_variants.h on host arrays (tests/native_harness/variants_harness.cpp) ------------------------------------------------------
@lru_cache(maxsize=1)
def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    lib = build_harness("variants_harness", "kp_variants.h")
    lib.kpy_variants.restype = C.c_int64
    lib.kpy_var_size.restype = C.c_uint64
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


GUARD = 0x7E


def harness_variants(ops, gene_fwd, asm, strand: int, q_start: int, q_end: int, t_abs: int, cstart: int = 0, kept: int = 0, cap=None, base: int = 0):
    """(count, records stored, guard intact): kp_variants_hit with the counting sink, then with the storing sink on a buffer of
    ``cap`` records (default: base + the count) followed by guard records; the hit's records go to ``base`` on."""
    ops = np.ascontiguousarray(ops, np.uint32)
    gene_fwd = np.ascontiguousarray(gene_fwd, np.uint8)
    aligned = gene_fwd if strand > 0 else revcomp_codes(gene_fwd)
    nib, fwd_nib, (words, runs) = S.pack_gene(aligned), S.pack_gene(gene_fwd), S.pack_target(asm)
    runs = np.ascontiguousarray(runs.reshape(-1), np.int32)
    q0 = int(q_start) if strand > 0 else len(gene_fwd) - int(q_end)
    args = (_p(ops), C.c_int64(len(ops)), _p(nib), _p(fwd_nib), C.c_int(len(gene_fwd)), _p(words), C.c_int(len(words)), _p(runs), C.c_int(len(runs) // 2),
            C.c_int(int(cstart)), C.c_int(len(asm)), C.c_int(q0), C.c_int(int(t_abs)), C.c_int(1 if strand < 0 else 0), C.c_int32(int(kept)))  # fmt: skip
    count = harness().kpy_variants(*args, None, C.c_int64(0), C.c_int64(0), C.c_int64(0))
    cap = base + count if cap is None else cap
    buf = np.frombuffer(bytes([GUARD]) * ((max(cap, 0) + 4) * VARIANT_DTYPE.itemsize), VARIANT_DTYPE).copy()
    again = harness().kpy_variants(*args, _p(buf), C.c_int64(base), C.c_int64(count), C.c_int64(cap))
    assert again == count, f"the storing sink counted {again} records, the counting sink {count}"
    return count, buf[:cap].copy(), bool((buf[cap:].view(np.uint8) == GUARD).all())
