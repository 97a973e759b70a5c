"""Shared by tests/test_aligned_cpu.py and tests/test_gpu_aligned.py: the yardstick of the aligned rows (include/kp_spec.h, ALIGNED
ROWS) -- a Python restatement written straight from the spec, column by column, that shares nothing with
kaptive_amd/csrc/kp_aligned.h --, a second route that reads no op (the gene's own codes with the variant records applied), a Python
formatter of the table and the g++ build of kp_aligned.h on host arrays.  TEST INFRASTRUCTURE."""

from __future__ import annotations

import ctypes as C
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

ALIGNED_ROW_DTYPE = np.dtype([("off", "<i8"), ("gene_len", "<i4"), ("covered", "<i4"), ("inserted", "<i4"), ("n_ins", "<i4")])  # (restated: the tests compare it with _native.ALIGNED_ROW_DTYPE)
M, I, D = 0, 1, 2
GAP = 5
F_SPURIOUS = 16
SNV, INS, DEL = 0, 1, 2
LETTERS = b"acgtn-"
HEADER = b"\t".join([b"Assembly", b"Gene", b"Contig", b"Start", b"End", b"Strand", b"Gene length", b"Gene start", b"Gene end", b"Covered",
                     b"Inserted", b"Insertions", b"Aligned"]) + b"\n"  # fmt: skip


def op(kind: int, n: int) -> int:
    return (int(n) << 4) | kind


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def row_from_ops(ops, asm_codes, Lq: int, strand: int, q_start: int, q_end: int, t_start: int, cstart: int, cend: int, found: bool = True):
    """(codes uint8 [Lq] with GAP = 5, covered, inserted, n_ins) of one kept record: ``ops`` the ops of the hit behind it, ``asm_codes``
    the assembly's codes (0..3, 4 inside an N run) in its padded space, ``[cstart, cend)`` the contig there."""
    Lq = max(int(Lq), 0)
    row = np.full(Lq, GAP, np.uint8)
    ops = [(int(o) & 15, int(o) >> 4) for o in np.asarray(ops).tolist()]
    rows = sum(n for k, n in ops if k != D)
    cols = sum(n for k, n in ops if k != I)
    fwd = strand >= 0
    q0 = int(q_start) if fwd else Lq - int(q_end)
    if not found or Lq <= 0 or q0 < 0 or q0 + rows > Lq or t_start < 0 or cstart + t_start + cols > cend:
        return row, 0, 0, 0
    r, t, inserted, n_ins = q0, int(cstart) + int(t_start), 0, 0
    for kind, n in ops:
        if kind == M:
            for x in range(n):  # column by column
                c = int(asm_codes[t + x])
                j = r + x if fwd else Lq - 1 - (r + x)
                row[j] = min(c, 4) if fwd or c > 3 else 3 - c
            r += n
            t += n
        elif kind == I:
            r += n
        elif kind == D:
            t += n
            inserted += n
            n_ins += 1
    return row, int((row != GAP).sum()), inserted, n_ins


def pack_blocks(codes) -> np.ndarray:
    """The packed form of a row of codes (0..3, 4, GAP): v = w | m << 32 | g << 48 per sixteen columns."""
    x = np.asarray(codes, np.uint8)
    n = len(x)
    out = np.zeros((n + 15) // 16, np.uint64)
    for b in range(len(out)):
        v = 0
        for c, code in enumerate(x[16 * b : 16 * b + 16].tolist()):
            if code == GAP:
                v |= 1 << (48 + c)
            elif code == 4:
                v |= 1 << (32 + c)
            else:
                v |= code << (2 * c)
        out[b] = v
    return out


def unpack_blocks(blocks, Lq: int) -> np.ndarray:
    out = np.zeros(Lq, np.uint8)
    for j in range(Lq):
        v = int(blocks[j // 16])
        c = j % 16
        out[j] = GAP if (v >> (48 + c)) & 1 else (4 if (v >> (32 + c)) & 1 else (v >> (2 * c)) & 3)
    return out


def row_from_variants(gene_fwd, q_start: int, q_end: int, records):
    """The second route, which reads no op: inside [q_start, q_end) the gene's own forward code, an SNV record's alt in its place, GAP
    over a DEL record; GAP outside.  INS records give (inserted, n_ins).  ``records``: the variant records of this kept record."""
    g = np.minimum(np.asarray(gene_fwd, np.uint8), 4)
    row = np.full(len(g), GAP, np.uint8)
    row[q_start:q_end] = g[q_start:q_end]
    inserted = n_ins = 0
    for v in records:
        kind, q, n = int(v["kind"]), int(v["q_pos"]), int(v["len"])
        if kind == SNV:
            row[q] = int(v["alt"])
        elif kind == DEL:
            row[q : q + n] = GAP
        else:
            inserted += n
            n_ins += 1
    return row, int((row != GAP).sum()), inserted, n_ins


def text(codes) -> bytes:
    return bytes(LETTERS[int(c)] for c in codes)


def format_tsv(asm_names, contig_names, gene_names, n_kept, kept, rows, blocks) -> bytes:
    """The lines of the aligned table (no header): ``contig_names[a]`` are assembly a's, ``kept[a]`` / ``rows[a]`` its kept records
    and their row records."""
    lines = []
    for a, name in enumerate(asm_names):
        for i in range(int(n_kept[a])):
            k, r = kept[a][i], rows[a][i]
            if int(k["flags"]) & F_SPURIOUS:
                continue
            L, off = int(r["gene_len"]), int(r["off"])
            cols = [str(name).encode(), str(gene_names[int(k["gene"])]).encode(), str(contig_names[a][int(k["contig"])]).encode(),
                    b"%d" % (int(k["t_start"]) + 1), b"%d" % int(k["t_end"]), b"+" if k["strand"] >= 0 else b"-", b"%d" % L,
                    b"%d" % (int(k["q_start"]) + 1), b"%d" % int(k["q_end"]), b"%d" % int(r["covered"]), b"%d" % int(r["inserted"]),
                    b"%d" % int(r["n_ins"]), text(unpack_blocks(blocks[off : off + (L + 15) // 16], L))]  # fmt: skip
            lines.append(b"\t".join(cols) + b"\n")
    return b"".join(lines)


# ---- packed assemblies for the host tests ---------------------------------------------------------------------------------------------------
def pack(contigs, junk_rng=None):
    """One assembly from code arrays (0..3, 4 = N): contigs start on word edges, the words end with the last contig's last word, N
    runs are listed in the padded space.  ``junk_rng``: the two bits under an N are random (a row must not read them)."""
    starts, at = [], 0
    for c in contigs:
        starts.append(at)
        at += (len(c) + 15) // 16 * 16
    codes = np.zeros(at, np.uint8)
    for s, c in zip(starts, contigs):
        codes[s : s + len(c)] = c
    is_n = np.concatenate([[0], (codes == 4).astype(np.int8), [0]])
    edges = np.flatnonzero(np.diff(is_n))
    bits = np.where(codes == 4, junk_rng.integers(0, 4, size=at) if junk_rng is not None else 0, codes).astype(np.uint32)
    words = (bits.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1, dtype=np.uint32)
    return SimpleNamespace(words=words, n_runs=edges.astype(np.int32).reshape(-1, 2), ctg_start=np.array(starts, np.int32),
                           ctg_len=np.array([len(c) for c in contigs], np.int32), codes=codes)  # fmt: skip


# ---- kp_aligned.h on host arrays (tests/native_harness/aligned_harness.cpp) ------------------------------------------------------------
@lru_cache(maxsize=1)
def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    return build_harness("aligned_harness", "kp_aligned.h")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


GUARD = 0x7E7E7E7E7E7E7E7E


def harness_row(ops, pa, contig: int, Lq: int, strand: int, q_start: int, q_end: int, t_start: int, found: bool = True):
    """(valid, blocks, (covered, inserted, n_ins)): kp_aligned_row_blocks on the packed assembly ``pa``; the block buffer is followed
    by guard words that must survive."""
    ops = np.ascontiguousarray(ops, np.uint32)
    words, runs = np.ascontiguousarray(pa.words, np.uint32), np.ascontiguousarray(pa.n_runs, np.int32).reshape(-1)
    nb = (max(int(Lq), 0) + 15) // 16
    blocks = np.full(nb + 4, GUARD, np.uint64)
    rec = np.zeros(4, np.int32)
    ok = harness().kpy_aligned_row(_p(ops) if len(ops) else None, C.c_int64(len(ops)), C.c_int(1 if found else 0), _p(words), C.c_int(len(words)),
                                   _p(runs) if len(runs) else None, C.c_int(len(runs) // 2), C.c_int(int(pa.ctg_start[contig])), C.c_int(int(pa.ctg_len[contig])), C.c_int(int(Lq)),
            C.c_int(int(q_start)), C.c_int(int(q_end)), C.c_int(int(t_start)), C.c_int(int(strand)), _p(blocks), _p(rec))  # fmt: skip
    assert (blocks[nb:] == GUARD).all(), "a store beyond the row's blocks"
    assert int(rec[0]) == max(int(Lq), 0)
    return bool(ok), blocks[:nb].copy(), tuple(int(x) for x in rec[1:])
