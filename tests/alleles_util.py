"""Shared by tests/test_alleles_cpu.py and tests/test_gpu_alleles.py: the yardstick of the allele digests (include/kp_spec.h,
ALLELES) -- a numpy-uint64 restatement written straight from the spec that shares nothing with kaptive_amd/csrc/kp_alleles.h --, a
Python formatter of the table and the g++ build of kp_alleles.h on host arrays.  TEST INFRASTRUCTURE."""

from __future__ import annotations

import ctypes as C
from functools import lru_cache

import numpy as np

from kaptive_amd.serotyping.batch import KEPT_DTYPE

ALLELE_DTYPE = np.dtype([("nt", "<u8"), ("aa", "<u8")])  # (restated: the tests compare it with _native.ALLELE_DTYPE)
TAG_NT, TAG_AA, TAG_LOCUS = 1, 2, 3
F_EXPECTED, F_INSIDE, F_EXTRA, F_SPURIOUS = 1, 2, 4, 16
HEADER = b"\t".join([b"Assembly", b"Locus", b"Locus allele", b"Gene", b"Set", b"Contig", b"Start", b"End", b"Strand", b"State", b"Length",
                     b"Allele", b"Protein length", b"Protein allele"]) + b"\n"  # fmt: skip
STATES = (b"normal", b"partial", b"truncated", b"below_id_threshold")
M64 = (1 << 64) - 1


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def mix(z):
    """MIX of a uint64 array (wrap-around arithmetic)."""
    z = np.asarray(z, np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= np.uint64(0xBF58476D1CE4E5B9)
        z ^= z >> np.uint64(27)
        z *= np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
    return z


def mix1(z: int) -> int:
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def digest(blocks, length: int, tag: int) -> int:
    v = np.asarray(blocks, np.uint64)
    with np.errstate(over="ignore"):
        s = int(mix(mix(np.arange(1, len(v) + 1, dtype=np.uint64)) ^ v).sum(dtype=np.uint64)) if len(v) else 0
    return mix1(s ^ mix1((tag << 56) | int(length)))


def nt_digest(codes) -> int:
    """Nucleotide digest of a strand-corrected code sequence (0..3, 4 = N)."""
    x = np.asarray(codes, np.uint64)
    n = len(x)
    pad = np.zeros((-n) % 16, np.uint64)
    x = np.concatenate([x, pad]).reshape(-1, 16)
    live = np.concatenate([np.ones(n, bool), np.zeros(len(pad), bool)]).reshape(-1, 16)
    j = np.arange(16, dtype=np.uint64)
    w = (np.where((x < 4) & live, x, 0).astype(np.uint64) << (2 * j)).sum(axis=1, dtype=np.uint64)
    m = (((x == 4) & live).astype(np.uint64) << j).sum(axis=1, dtype=np.uint64)
    return digest(w | (m << np.uint64(32)), n, TAG_NT)


def text_codes(text) -> np.ndarray:
    """Codes of a text of acgtn letters in either case (anything else is N)."""
    lut = np.full(256, 4, np.uint8)
    for i, c in enumerate(b"ACGT"):
        lut[c] = lut[c + 32] = i
    return lut[np.frombuffer(text.encode() if isinstance(text, str) else bytes(text), np.uint8)]


def interval_codes(asm_codes, start: int, end: int, strand: int) -> np.ndarray:
    """The strand-corrected codes of positions [start, end) of the assembly's padded space."""
    x = np.asarray(asm_codes[start:end], np.uint8)
    if strand >= 0:
        return x
    x = x[::-1]
    return np.where(x <= 3, 3 - x, 4).astype(np.uint8)


def aa_digest(prot) -> int:
    b = np.frombuffer(bytes(prot), np.uint8)
    n = len(b)
    b = np.concatenate([b, np.zeros((-n) % 8, np.uint8)])
    return digest(b.view("<u8"), n, TAG_AA)


def locus_digest(piece_digests, order) -> int:
    """Locus digest of the pieces' nucleotide digests listed in ``order``; 0 without a piece."""
    if len(order) == 0:
        return 0
    return digest([int(piece_digests[int(p)]) for p in order], len(order), TAG_LOCUS)


def piece_order(pieces, n: int) -> np.ndarray:
    return np.argsort(np.ascontiguousarray(pieces["mean_pos"][:n]))


def restate(kept, pieces, prot, ctg_start, asm_codes):
    """(ALLELE_DTYPE per kept record, u64 per piece) of one assembly: ``kept`` / ``pieces`` its records, ``prot`` its protein buffer,
    ``ctg_start`` its contigs in the padded space whose codes are ``asm_codes``."""
    out = np.zeros(len(kept), ALLELE_DTYPE)
    for i, k in enumerate(kept):
        c0 = int(ctg_start[int(k["contig"])])
        out[i]["nt"] = nt_digest(interval_codes(asm_codes, c0 + int(k["t_start"]), c0 + int(k["t_end"]), int(k["strand"])))
        n = int(k["prot_len"])
        out[i]["aa"] = aa_digest(prot[int(k["prot_off"]) : int(k["prot_off"]) + n]) if n > 0 else 0
    pd = np.zeros(len(pieces), np.uint64)
    for p, r in enumerate(pieces):
        c0 = int(ctg_start[int(r["contig"])])
        pd[p] = nt_digest(interval_codes(asm_codes, c0 + int(r["start"]), c0 + int(r["end"]), int(r["strand"])))
    return out, pd


def _hex(v: int) -> bytes:
    return b"%016x" % int(v)


def set_name(flags: int) -> bytes:
    kind = b"expected" if flags & F_EXPECTED else (b"extra" if flags & F_EXTRA else b"other")
    return kind + (b"_in" if flags & F_INSIDE else b"_out")


def format_tsv(asm_names, contig_names, gene_names, locus_names, best_locus, n_kept, kept, alleles, n_pieces, pieces, piece_digests) -> bytes:
    """The lines of the allele table (no header): ``contig_names[a]`` are assembly a's, ``kept[a]`` / ``alleles[a]`` its kept records
    and their digests, ``pieces[a]`` / ``piece_digests[a]`` its pieces and theirs."""
    lines = []
    for a, name in enumerate(asm_names):
        m = int(n_pieces[a])
        la = locus_digest(piece_digests[a], piece_order(pieces[a], m))
        for i in range(int(n_kept[a])):
            k, d = kept[a][i], alleles[a][i]
            if int(k["flags"]) & F_SPURIOUS:
                continue
            cols = [str(name).encode(), str(locus_names[int(best_locus[a])]).encode(), _hex(la) if m else b".", str(gene_names[int(k["gene"])]).encode(),
                    set_name(int(k["flags"])), str(contig_names[a][int(k["contig"])]).encode(), b"%d" % (int(k["t_start"]) + 1), b"%d" % int(k["t_end"]),
                    b"+" if k["strand"] >= 0 else b"-", STATES[int(k["state"])], b"%d" % (int(k["t_end"]) - int(k["t_start"])), _hex(d["nt"]),
                    b"%d" % int(k["prot_len"]), _hex(d["aa"]) if int(k["prot_len"]) > 0 else b"."]  # fmt: skip
            lines.append(b"\t".join(cols) + b"\n")
    return b"".join(lines)


# ---- kp_alleles.h on host arrays (tests/native_harness/alleles_harness.cpp) ------------------------------------------------------------
@lru_cache(maxsize=1)
def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    lib = build_harness("alleles_harness", "kp_alleles.h")
    for f in ("kpy_al_mix", "kpy_al_nt", "kpy_al_nt_lanes", "kpy_al_aa", "kpy_al_locus"):
        getattr(lib, f).restype = C.c_uint64
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness_nt(pa, contig: int, start: int, end: int, strand: int, lanes: int = 0) -> int:
    """The header's nucleotide digest of an interval of the packed assembly ``pa``; ``lanes`` > 0: the blocks dealt out to that many
    lanes as the kernel deals them (lane, lane + lanes, ...), the partial sums added."""
    words, runs = np.ascontiguousarray(pa.words, np.uint32), np.ascontiguousarray(pa.n_runs, np.int32).reshape(-1)
    args = (_p(words), C.c_int(len(words)), _p(runs), C.c_int(len(runs) // 2), C.c_int(int(pa.ctg_start[contig])), C.c_int(int(pa.ctg_len[contig])),
            C.c_int(int(start)), C.c_int(int(end)), C.c_int(int(strand)))  # fmt: skip
    return int(harness().kpy_al_nt_lanes(*args, C.c_int(lanes)) if lanes else harness().kpy_al_nt(*args))


def harness_aa(prot) -> int:
    b = np.frombuffer(bytes(prot), np.uint8).copy() if len(prot) else np.zeros(1, np.uint8)
    return int(harness().kpy_al_aa(_p(b), C.c_int(len(prot))))


def harness_locus(piece_digests, order) -> int:
    d, o = np.ascontiguousarray(piece_digests, np.uint64), np.ascontiguousarray(order, np.int32)
    if len(d) == 0:
        d = np.zeros(1, np.uint64)
    return int(harness().kpy_al_locus(_p(d), _p(o) if len(o) else None, C.c_int(len(o))))


def kept_rows(rows, flags=None, states=None, prot=None) -> np.ndarray:
    """A kept list from (gene, contig, strand, t_start, t_end) rows; ``prot``: (prot_off, prot_len) per row."""
    k = np.zeros(len(rows), KEPT_DTYPE)
    for i, (g, c, st, t0, t1) in enumerate(rows):
        k[i]["gene"], k[i]["contig"], k[i]["strand"], k[i]["t_start"], k[i]["t_end"], k[i]["q_end"] = g, c, st, t0, t1, t1 - t0
    if flags is not None:
        k["flags"] = flags
    if states is not None:
        k["state"] = states
    if prot is not None:
        for i, (o, n) in enumerate(prot):
            k[i]["prot_off"], k[i]["prot_len"] = o, n
    return k
