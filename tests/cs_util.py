"""Shared by tests/test_cs_cpu.py and tests/test_gpu_cs.py: the yardstick of the cs strings (include/kp_spec.h, CS) -- a Python
restatement written straight from the spec, column by column, that shares nothing with kaptive_amd/csrc/kp_cs.h -- the
invariants of the spec as checks on a string, the g++ build of kp_cs.h on host arrays, and the hand-built batch of
tests/test_gpu_cs.py.  TEST INFRASTRUCTURE."""

from __future__ import annotations

import ctypes as C
import re
from functools import lru_cache

import numpy as np

from tests import cigar_util as U

M, I, D, EQ, X = 0, 1, 2, 7, 8
LETTERS = "acgtn"
GRAMMAR = re.compile(rb"(:[0-9]+|\*[acgtn]{2}|[+\-][acgtn]+)+")
TOKEN = re.compile(rb":[0-9]+|\*[acgtn]{2}|[+\-][acgtn]+")


def _letter(code) -> str:
    return LETTERS[min(int(code), 4)]


def cs_from_ops(ops, gene_as_aligned, asm_codes, q, t) -> bytes:
    """The cs string of a hit whose path starts at row ``q`` of the gene as aligned and column ``t`` of the assembly's codes
    (0..3, 4 = N on either side).  A column is identical iff both codes are <= 3 and equal."""
    out, same = [], 0
    q, t = int(q), int(t)
    for op in np.asarray(ops).tolist():
        kind, n = op & 15, op >> 4
        if kind == M:
            for j in range(n):
                qc, tc = int(gene_as_aligned[q + j]), int(asm_codes[t + j])
                if qc <= 3 and tc <= 3 and qc == tc:
                    same += 1
                    continue
                if same:
                    out.append(f":{same}")
                    same = 0
                out.append("*" + _letter(tc) + _letter(qc))
            q += n
            t += n
            continue
        if same:
            out.append(f":{same}")
            same = 0
        if kind == I:
            out.append("+" + "".join(_letter(c) for c in gene_as_aligned[q : q + n]))
            q += n
        else:
            assert kind == D, f"op kind {kind}"
            out.append("-" + "".join(_letter(c) for c in asm_codes[t : t + n]))
            t += n
    if same:
        out.append(f":{same}")
    return "".join(out).encode()


def eqx_from_cs(cs: bytes) -> list:
    """The =/X ops a cs string stands for: :n is n=, a run of k * tokens kX, + and - are I and D."""
    ops = []
    for tok in TOKEN.findall(cs):
        if tok[:1] == b":":
            ops.append((int(tok[1:]) << 4) | EQ)
        elif tok[:1] == b"*":
            if ops and ops[-1] & 15 == X:
                ops[-1] += 1 << 4
            else:
                ops.append((1 << 4) | X)
        else:
            ops.append(((len(tok) - 1) << 4) | (I if tok[:1] == b"+" else D))
    return ops


def check_cs(cs: bytes, ops, label: str, matches=None) -> None:
    """Grammar, canonical form and the column sums of kp_spec.h, CS."""
    assert GRAMMAR.fullmatch(cs), f"{label}: {cs[:80]!r} breaks the grammar"
    toks = TOKEN.findall(cs)
    assert b"".join(toks) == cs
    assert not any(t[:2] == b":0" for t in toks), f"{label}: a :0 token (or a leading zero)"
    assert not any(a[:1] == b":" and b[:1] == b":" for a, b in zip(toks, toks[1:])), f"{label}: two : tokens touch"
    ops = np.asarray(ops, np.int64)
    sm, si, sd = (int((ops >> 4)[(ops & 15) == k].sum()) for k in (M, I, D))
    same = sum(int(t[1:]) for t in toks if t[:1] == b":")
    n_sub = sum(1 for t in toks if t[:1] == b"*")
    assert same + n_sub == sm, f"{label}: {same} identical + {n_sub} substituted columns, M ops hold {sm}"
    assert sum(len(t) - 1 for t in toks if t[:1] == b"+") == si, f"{label}: letters behind + against the I ops"
    assert sum(len(t) - 1 for t in toks if t[:1] == b"-") == sd, f"{label}: letters behind - against the D ops"
    if matches is not None:
        assert same == int(matches), f"{label}: : lengths sum to {same}, matches = {int(matches)}"


def hit_cs_yardstick(hit, ops, gene_codes, gene_off, pa, asm_codes) -> bytes:
    """``cs_from_ops`` on a HIT_DTYPE row: the gene as aligned, the path's first row and column from the hit's fields."""
    gs = int(hit["gene"]) * 2 + (1 if hit["strand"] < 0 else 0)
    g = U.gene_as_aligned(gene_codes, gene_off, gs)
    q = len(g) - int(hit["q_end"]) if hit["strand"] < 0 else int(hit["q_start"])
    return cs_from_ops(ops, g, asm_codes, q, int(pa.ctg_start[hit["contig"]]) + int(hit["t_start"]))


# ---- kp_cs.h on host arrays (tests/native_harness/cs_harness.cpp) -----------------------------------------------------------------
@lru_cache(maxsize=1)
def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    lib = build_harness("cs_harness", "kp_cs.h")
    lib.kpy_cs.restype = C.c_int64
    lib.kpy_cs_size.restype = C.c_uint64
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def pack_gene(codes) -> np.ndarray:
    """4-bit codes, eight per word (KpGenes::nib)."""
    c = np.zeros((len(codes) + 7) // 8 * 8, np.uint32)
    c[: len(codes)] = codes
    return (c.reshape(-1, 8) << (4 * np.arange(8, dtype=np.uint32))).sum(axis=1).astype(np.uint32)


def pack_target(codes):
    """(2-bit words, sixteen bases each; N runs as (start, end) pairs): what a packed assembly holds of ``codes`` (0..4)."""
    codes = np.asarray(codes, np.uint8)
    c = np.zeros((len(codes) + 15) // 16 * 16, np.uint32)
    c[: len(codes)] = np.where(codes > 3, 0, codes)
    words = (c.reshape(-1, 16) << (2 * np.arange(16, dtype=np.uint32))).sum(axis=1).astype(np.uint32)
    isn = np.concatenate([[0], (codes > 3).astype(np.int8), [0]])
    edges = np.flatnonzero(np.diff(isn))
    return words, edges.astype(np.int32).reshape(-1, 2)


def harness_cs(ops, gene, asm, q, t, cap=None):
    """(count, bytes written, guard intact): kp_cs_hit with the counting sink, then with the writing sink on a buffer of ``cap``
    bytes (default: the count) followed by guard bytes."""
    ops = np.ascontiguousarray(ops, np.uint32)
    nib, (words, runs) = pack_gene(gene), pack_target(asm)
    runs = np.ascontiguousarray(runs.reshape(-1), np.int32)
    args = (_p(ops), C.c_int64(len(ops)), _p(nib), C.c_int(len(gene)), _p(words), C.c_int(len(words)), _p(runs), C.c_int(len(runs) // 2),
            C.c_int(0), C.c_int(len(asm)), C.c_int(int(q)), C.c_int(int(t)))  # fmt: skip
    count = harness().kpy_cs(*args, None, C.c_int64(0))
    cap = count if cap is None else cap
    buf = np.full(max(cap, 0) + 16, 0x7E, np.uint8)
    again = harness().kpy_cs(*args, _p(buf), C.c_int64(cap))
    assert again == count, f"the writing sink counted {again} bytes, the counting sink {count}"
    return count, buf[:cap].tobytes(), bool((buf[cap:] == 0x7E).all())


def build_pair(rng, ops, q0=0, t0=0, sub_rows=(), gene_n=(), n_runs=(), d_n=False, i_n=False):
    """(gene, asm) that the ops align from row q0 / column t0: the gene copies the target along M ops, then gets substitutions
    at the rows ``sub_rows`` and an n at the rows ``gene_n``; the target gets N runs ``(start, length)``; ``i_n`` / ``d_n`` put an n
    into the middle of every I / D op."""
    n_m, n_i, n_d = (sum(n for k, n in ops if k == kind) for kind in (M, I, D))
    asm = rng.integers(0, 4, size=t0 + n_m + n_d + 19).astype(np.uint8)
    gene = list(rng.integers(0, 4, size=q0).astype(np.uint8))
    t = t0
    n_at = []
    for k, n in ops:
        if k == M:
            gene.extend(asm[t : t + n])
            t += n
        elif k == I:
            ins = rng.integers(0, 4, size=n).astype(np.uint8)
            if i_n:
                ins[n // 2] = 4
            gene.extend(ins)
        else:
            if d_n:
                n_at.append(t + n // 2)
            t += n
    gene = np.array(gene + list(rng.integers(0, 4, size=5)), np.uint8)
    for r in sub_rows:
        gene[r] = (gene[r] + 1 + int(rng.integers(0, 3))) % 4
    for r in gene_n:
        gene[r] = 4
    for s, n in n_runs:
        asm[s : s + n] = 4
    for s in n_at:
        asm[s] = 4
    return gene, asm


def ops_of(*pairs):
    return np.array([(n << 4) | k for k, n in pairs], np.uint32)


# ---- the hand-built batch of tests/test_gpu_cs.py ---------------------------------------------------------------------------------------
SUB_COLUMNS = (7, 8, 63, 64, 65, 300, 301, 511, 512)  # columns of the 700-base gene that its copies change (300, 301: the adjacent pair)
BIG, SUB, RUN, WITH_N = 0, 1, 2, 3  # genes of hand_genes()
N_RUN_AT, GENE_N_AT = 430, 400


def _other_base(rng, b):
    return next(c for c in rng.permutation(np.frombuffer(b"ACGT", np.uint8)) if c != b)


def hand_genes():
    """A 12 000-base gene, the 700-base gene of the substituted copies, a 900-base gene (copied with an N run) and an 800-base
    gene that holds an N."""
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import random_orf

    rng = np.random.default_rng(4242)
    genes = [random_orf(rng, n, 0.5) for n in (12000, 702, 900, 801)]
    genes[SUB] = genes[SUB][:700]
    genes[WITH_N] = genes[WITH_N][:800].copy()
    genes[WITH_N][GENE_N_AT] = ord("N")
    recs = [SeqRecord(name, g.tobytes()) for name, g in zip(("big", "sub", "run", "with_n"), genes)]
    return Sequences.from_records(recs), genes


def hand_assembly(genes):
    """One assembly of 36 contigs: the N-run copy first (its contig starts the assembly's padded space, so the run's place in a
    packed word is known: it begins at base 15 of a word -- it straddles a word edge), a clean copy of the 12 000-base
    gene, a copy of the gene with an N (the contig has a base there), then the substituted copies of the 700-base gene at 16
    consecutive contig offsets, forward and reverse-complemented."""
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import random_dna, revcomp

    rng = np.random.default_rng(4243)
    flank = lambda n: random_dna(rng, n, 0.5)  # noqa: E731
    run_copy = genes[RUN].copy()
    run_copy[N_RUN_AT : N_RUN_AT + 3] = ord("N")
    contigs = [np.concatenate([flank(15 + 16 * 40 - N_RUN_AT), run_copy, flank(250)])]  # the run begins at contig base 655 = 16 * 40 + 15
    contigs.append(np.concatenate([flank(300), genes[BIG], flank(300)]))
    with_base = genes[WITH_N].copy()
    with_base[GENE_N_AT] = ord("C")
    contigs.append(np.concatenate([flank(222), with_base, flank(222)]))
    sub = genes[SUB].copy()
    for c in SUB_COLUMNS:
        sub[c] = _other_base(rng, sub[c])
    for k in range(16):
        contigs.append(np.concatenate([flank(200 + k), sub, flank(230)]))
    for k in range(16):
        contigs.append(revcomp(np.concatenate([flank(230), sub, flank(200 + k)])))
    recs = [SeqRecord(f"h{i}", c.tobytes()) for i, c in enumerate(contigs)]
    return GenomeAssembly("hand_built", Sequences.from_records(recs))
