"""Inputs that land on every path of the occurrence cut (csrc/kp_chain.hip: kp_occ_cut_kernel, kp_occ_sketch_kernel,
kp_occ_quantile_kernel) and on both sides of its thresholds.  Seeded and pure numpy; where a count has to be exact (the place
of a gene's stretch in the sorted anchor list, the number of distinct minimizers) the builder takes the oracle and trims a
copy base by base, as tests/sort_classes_util.py trims its buckets.  Shared by tests/test_occ_cut_oracle.py (the inputs are
what their labels say, by the oracle alone) and tests/test_gpu_occ_cut.py (the device equals the oracle on them).
TEST INFRASTRUCTURE.

How a case is made.  A CASSETTE is a piece of a gene between two fixed flanks of random bases, longer than a minimizer
window: every copy of a cassette yields the same seeds of the gene, on either strand, so a cassette in c copies gives every
one of its u seeds exactly c anchors on c (gene/strand, diagonal) pairs.  A filler gene planted as a contig of its own adds
a number of anchors that depends on nothing else in the assembly; fillers sort before the genes under test, tail genes
after them, so the stretch of gene R in the sorted list starts at the sum of the planted fillers' anchors."""

from __future__ import annotations

import functools
import re
from pathlib import Path
from typing import Callable, NamedTuple

import numpy as np

from kaptive_amd.core.genome import GenomeAssembly
from kaptive_amd.core.seq import SeqRecord, Sequences
from kaptive_amd.pack import words_to_codes
from kaptive_amd.synth import random_dna, revcomp

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kaptive_amd" / "csrc"
TOP_SHIFT = 46  # KP_ANCHOR_KEY: gene * 2 + strand above bit 46, the diagonal above bit 16, the query position below


# ---- the constants the paths hang on, read out of the sources ----------------------------------------------------------------------
def kernel_constants() -> dict[str, int]:
    chain, align = (CSRC / "kp_chain.hip").read_text(), (CSRC / "kp_align.hip").read_text()
    spec = (ROOT / "include" / "kp_spec.h").read_text()
    out = {}
    for name in ("KP_K", "KP_W", "KP_MID_OCC", "KP_MID_OCC_HIST", "KP_MIN_ANCHORS"):
        out[name] = int(re.search(rf"#define\s+{name}\s+(\d+)", spec).group(1))
    for name in ("KP_OCC_WAVES", "KP_OCC_BINS"):
        out[name[3:]] = int(re.search(rf"#ifndef {name}\b.*?#define {name} (\d+)", chain, flags=re.S).group(1))
    for name in ("OCC_CHUNK", "OCC_PARTS"):
        out[name] = int(re.search(rf"constexpr int {name} = (\d+);", chain).group(1))
    m = re.search(r"constexpr int OCC_WARM = (\d+) \+ (\d+) \* \(KP_K \+ KP_W\);", chain)
    out["OCC_WARM"] = int(m.group(1)) + int(m.group(2)) * (out["KP_K"] + out["KP_W"])
    m = re.search(r"max_asm_bases \* (\d+) / (\d+) \+ 1", align)  # the table rule of enqueue_align
    out["TABLE_NUM"], out["TABLE_DEN"] = int(m.group(1)), int(m.group(2))
    out["TABLE_LG_MIN"] = int(re.search(r"uint32_t lg = (\d+);", align).group(1))
    return out


EXPECTED_CONSTANTS = dict(KP_K=15, KP_W=10, KP_MID_OCC=10, KP_MID_OCC_HIST=2048, KP_MIN_ANCHORS=3, OCC_WAVES=8, OCC_BINS=1024,
                          OCC_CHUNK=256, OCC_PARTS=128, OCC_WARM=98, TABLE_NUM=2, TABLE_DEN=5, TABLE_LG_MIN=12)  # fmt: skip
C = EXPECTED_CONSTANTS  # every size below is derived from these; the CPU module asserts that the sources still hold them
K, MID, BINS, WAVES, CHUNK, WARM = C["KP_K"], C["KP_MID_OCC"], C["OCC_BINS"], C["OCC_WAVES"], C["OCC_CHUNK"], C["OCC_WARM"]
BLOCK = 64 * WAVES  # entries of a compaction chunk
SECOND_CHUNK = C["OCC_PARTS"] * 256 * CHUNK  # padded positions beyond which a thread of the sketch kernel takes a second chunk


def table_log2(max_asm_bases: int) -> int:
    """enqueue_align's rule: the batch's counting tables have 2^lg entries."""
    lg = C["TABLE_LG_MIN"]
    while (1 << lg) < max_asm_bases * C["TABLE_NUM"] // C["TABLE_DEN"] + 1 and lg < 31:
        lg += 1
    return lg


def kth_of(n: int) -> int:
    """kp_spec.h's index into the sorted counts of n distinct minimizers: (int)((1 - 2e-4f) n), in double."""
    return min(int((1.0 - float(np.float32(2e-4))) * float(n)), n - 1)


def slice_per(n: int) -> int:
    """Anchors per wave slice of kp_occ_cut_kernel (whole rounds of 64)."""
    return ((n + WAVES - 1) // WAVES + 63) & ~63


# ---- the database ------------------------------------------------------------------------------------------------------------------
N_FILL = 40
G_R, G_L, G_B1024, G_B1025, G_B1039 = N_FILL, N_FILL + 1, N_FILL + 2, N_FILL + 3, N_FILL + 4
N_TAIL = 40
G_TAIL = G_B1039 + 1
GENE_LEN = {G_R: 700, G_L: 2 * BINS + 252, G_B1024: BINS, G_B1025: BINS + 1, G_B1039: BINS + K}


# generator seeds of the genes under test: picked so that the database holds a seed (the gene's own minimizer) at the positions the
# window cases need -- B1024 / B1025 at their last position, B1039 at OCC_BINS - 1 and at OCC_BINS (its last), L at OCC_BINS - 1,
# OCC_BINS and its last position; tests/test_occ_cut_oracle.py asserts it
GENE_SEED = {G_R: 0, G_L: 90, G_B1024: 5, G_B1025: 2, G_B1039: 9}
EDGE_POSITIONS = {G_B1024: (BINS - K,), G_B1025: (BINS + 1 - K,), G_B1039: (BINS - 1, BINS), G_L: (BINS - 1, BINS, GENE_LEN[G_L] - K)}


@functools.lru_cache(maxsize=None)
def _genes() -> tuple:
    rng = np.random.default_rng(7301)
    fill = [random_dna(rng, int(rng.integers(150, 260)), 0.5) for _ in range(N_FILL)]
    test = [random_dna(np.random.default_rng([7301, GENE_LEN[g], GENE_SEED[g]]), GENE_LEN[g], 0.5) for g in range(G_R, G_TAIL)]
    tail = [random_dna(rng, int(rng.integers(150, 260)), 0.5) for _ in range(N_TAIL)]
    return tuple(fill + test + tail)


def genes() -> list[np.ndarray]:
    return list(_genes())


def gene_sequences() -> Sequences:
    return Sequences.from_records([SeqRecord(f"g{i}", g.tobytes()) for i, g in enumerate(genes())])


def asm_of(name: str, contigs) -> GenomeAssembly:
    return GenomeAssembly(name, Sequences.from_records([SeqRecord(f"c{i}", np.asarray(c, np.uint8).tobytes()) for i, c in enumerate(contigs)]))


# ---- reading an anchor list --------------------------------------------------------------------------------------------------------
def gene_of(anchors: np.ndarray) -> np.ndarray:
    return (anchors >> np.uint64(TOP_SHIFT + 1)).astype(np.int64)


def stretch(anchors: np.ndarray, gene: int) -> tuple[int, int]:
    """[s, e) of the gene's anchors in a sorted list."""
    g = gene_of(anchors)
    return int(np.searchsorted(g, gene, "left")), int(np.searchsorted(g, gene, "right"))


def forward_pos(anchors: np.ndarray, glen: int) -> np.ndarray:
    """Position of every anchor's seed on the gene's forward strand (anchors of ONE gene)."""
    q = (anchors & np.uint64(0xFFFF)).astype(np.int64)
    rev = ((anchors >> np.uint64(TOP_SHIFT)) & np.uint64(1)).astype(bool)
    return np.where(rev, glen - K - q, q)


def seed_counts(anchors: np.ndarray, gene: int) -> dict[int, int]:
    """Anchors per seed (forward position) of one gene."""
    s, e = stretch(anchors, gene)
    pos, cnt = np.unique(forward_pos(anchors[s:e], len(genes()[gene])), return_counts=True)
    return dict(zip(pos.tolist(), cnt.tolist()))


def n_pairs(anchors: np.ndarray, gene: int) -> int:
    """(gene/strand, diagonal) pairs the gene's anchors lie on."""
    s, e = stretch(anchors, gene)
    return len(np.unique(anchors[s:e] >> np.uint64(16)))


def n_over(anchors: np.ndarray, gene: int, thr: int = MID) -> list[int]:
    """Seeds of the gene with more than thr anchors, per counting window of OCC_BINS forward positions."""
    out = [0] * ((len(genes()[gene]) + BINS - 1) // BINS)
    for pos, c in seed_counts(anchors, gene).items():
        out[pos // BINS] += c > thr
    return out


def dropped_indices(before: np.ndarray, after: np.ndarray) -> np.ndarray:
    return np.flatnonzero(~np.isin(before, after))


def contig_codes(pa) -> list[np.ndarray]:
    """Codes (0..3, 4 = ambiguous) of every contig of a packed assembly."""
    codes = words_to_codes(np.asarray(pa.words, np.uint32), pa.padded_len).copy()
    for a, b in np.asarray(pa.n_runs).reshape(-1, 2):
        codes[a:b] = 4
    return [codes[s : s + n] for s, n in zip(pa.ctg_start.tolist(), pa.ctg_len.tolist())]


def minimizer_histogram(oracle, pa) -> tuple[np.ndarray, np.ndarray]:
    """(seed values, counts) of the assembly's minimizers, by the oracle's sketch of every contig."""
    xs = [oracle.seeds(c)[2] for c in contig_codes(pa)]
    return np.unique(np.concatenate(xs) if xs else np.empty(0, np.uint32), return_counts=True)


# ---- building blocks ---------------------------------------------------------------------------------------------------------------
FLANK = 2 * (K + C["KP_W"])  # longer than a minimizer window on either side: a cassette's gene seeds do not depend on what is around it


def cassette(gene: int, a: int, b: int, salt: int = 0) -> np.ndarray:
    """salt < 0: the BARE form, the piece between two N's -- no minimizer but the gene's own is repeated with it."""
    if salt < 0:
        return np.concatenate([[ord("N")], genes()[gene][a:b], [ord("N")]]).astype(np.uint8)
    rng = np.random.default_rng([7400, gene, a, b, salt])
    return np.concatenate([random_dna(rng, FLANK, 0.5), genes()[gene][a:b], random_dna(rng, FLANK, 0.5)])


def copies(rng, unit: np.ndarray, strands: str) -> np.ndarray:
    """One copy of the unit per letter of ``strands`` ('+' as it is, '-' reverse-complemented), random spacers between."""
    parts = [random_dna(rng, 40, 0.5)]
    for ch in strands:
        parts += [unit if ch == "+" else revcomp(unit), random_dna(rng, int(rng.integers(30, 60)), 0.5)]
    return np.concatenate(parts)


class Builder:
    """Oracle-guided pieces: cassettes with a given number of seeds, fillers trimmed to a given number of anchors."""

    def __init__(self, odb):
        self.odb = odb
        self.g = genes()
        self._count: dict[tuple[int, int], int] = {}
        self._unit: dict[tuple, tuple[int, int]] = {}

    def anchors(self, asm, cut=False) -> np.ndarray:
        return self.odb.anchors(asm.packed(), cut=cut)

    def planted_count(self, gene: int, p: int) -> int:
        """Anchors of the contig gene[:p] (all of them the gene's own)."""
        if (gene, p) not in self._count:
            a = self.anchors(asm_of("count", [self.g[gene][:p]]))
            assert (gene_of(a) == gene).all()
            self._count[gene, p] = len(a)
        return self._count[gene, p]

    def planted(self, pool: range, want: int) -> list[np.ndarray]:
        """Contigs -- whole genes of the pool, and one trimmed -- that add exactly ``want`` anchors."""
        out, left = [], want
        free = list(pool)
        for g in list(free):
            c = self.planted_count(g, len(self.g[g]))
            leaves_one = left - c == 1  # (a remainder of one anchor is the hardest to trim a gene to)
            if c <= left and not leaves_one:
                out.append(self.g[g])
                left -= c
                free.remove(g)
            if left == 0:
                return out
        for g in free:
            for p in range(len(self.g[g]), K - 1, -1):
                if self.planted_count(g, p) == left:
                    return out + [self.g[g][:p]]
        raise AssertionError(f"no trimmed gene of {pool} adds exactly {left} anchors (of {want})")

    def unit(self, gene: int, u: int, lo: int, hi: int, salt: int = 0) -> tuple[int, int, int]:
        """(a, b, salt): [a, b) within [lo, hi) of the gene whose cassette yields exactly u seeds of it, all starting in [lo, hi)."""
        key = (gene, u, lo, hi, salt)
        if key not in self._unit:
            glen = len(self.g[gene])
            for a in range(lo, hi):
                for b in range(a + K + C["KP_W"] - 1, min(hi + K, glen) + 1):
                    # (as it will be used: between spacers, on either strand; the bare form -- the sketch is lazy behind an N, and
                    # not the same on both strands there -- on the forward strand only)
                    got = self.anchors(asm_of("unit", [copies(np.random.default_rng(7450), cassette(gene, a, b, salt), "++" if salt < 0 else "+-")]))
                    if len(got) > 2 * u:
                        break
                    pos = forward_pos(got, glen)
                    if len(got) == 2 * u and (gene_of(got) == gene).all() and (pos >= lo).all() and (pos < hi).all() and (np.unique(pos, return_counts=True)[1] == 2).all():
                        self._unit[key] = (a, b, salt)
                        break
                if key in self._unit:
                    break
            assert key in self._unit, f"no cassette of gene {gene} in [{lo}, {hi}) with {u} seeds"
        return self._unit[key]

    def unit_at(self, gene: int, pos: int) -> tuple[int, int, int]:
        """A cassette of the gene's 15-mer at forward position ``pos`` alone, with flanks that leave it a minimizer."""
        key = (gene, "at", pos)
        if key not in self._unit:
            glen = len(self.g[gene])
            for salt in range(400):
                got = self.anchors(asm_of("unit", [copies(np.random.default_rng(7450), cassette(gene, pos, pos + K, salt), "+-")]))
                if len(got) == 2 and (gene_of(got) == gene).all() and (forward_pos(got, glen) == pos).all():
                    self._unit[key] = (pos, pos + K, salt)
                    break
            assert key in self._unit, f"no cassette of gene {gene} with one seed at {pos}"
        return self._unit[key]


class Case(NamedTuple):
    label: str  # which branch it pins
    asm: GenomeAssembly
    want: dict  # what the oracle must find: see tests/test_occ_cut_oracle.py (check_case)
    holds: Callable[[dict], bool] | None = None  # the label's claim about s, e, n (m: measured values)


def background(seed: int, n: int) -> np.ndarray:
    return random_dna(np.random.default_rng([7500, seed]), n, 0.5)


# ---- A. list positions -------------------------------------------------------------------------------------------------------------
def r_block(B: Builder, seed: int, full: int = 0, over: int = MID + 1, u: int = 2) -> np.ndarray:
    """Gene R's contig: ``full`` whole copies (kept: at most MID - 1) and a u-seed cassette until its seeds have ``over``
    anchors; alternating strands."""
    rng = np.random.default_rng([7600, seed])
    whole = np.concatenate([random_dna(rng, FLANK, 0.5), B.g[G_R], random_dna(rng, FLANK, 0.5)])
    strands = "+-" * 8
    return np.concatenate([copies(rng, whole, strands[:full]), copies(rng, cassette(G_R, *B.unit(G_R, u, 100, 400)), strands[: over - full])])


def list_cases(B: Builder) -> list[Case]:
    """R's stretch [s, e) of the pre-cut list at every place the round, slice and compaction logic tells apart.  The cut drops
    R's two repeated seeds (MID + 1 anchors each) at the floor: two seeds beyond it never ask for the quantile."""
    small = r_block(B, 1)  # 2 seeds x 11 copies
    m_small = len(B.anchors(asm_of("m", [small])))
    mid = r_block(B, 2, full=1)
    m_mid = len(B.anchors(asm_of("m", [mid])))
    big = r_block(B, 3, full=3)
    m_big = len(B.anchors(asm_of("m", [big])))
    assert m_small == 2 * (MID + 1) < 64 and 128 + 5 < m_mid < 192 and m_big >= 3 * 64 + 2, (m_small, m_mid, m_big)
    fill, tail = range(0, N_FILL), range(G_TAIL, G_TAIL + N_TAIL)

    def case(label, block, m, s, t, holds):
        contigs = [*B.planted(fill, s), block, *B.planted(tail, t)]
        return Case(label, asm_of(label.split(":")[0], contigs), dict(s=s, e=s + m, n=s + m + t, drops=True, state=1, mid_occ=MID), holds)

    out = []
    # n in (8 * 64, 8 * 128]: per = 128, two rounds a slice; slice 2 is [256, 384), its rounds begin at 256 and 320
    n_s = 2 * BLOCK - 30
    per = slice_per(n_s)
    assert per == 128
    sl = lambda label, block, m, s, holds: case(label, block, m, s, n_s - s - m, lambda v: slice_per(v["n"]) == per and holds(v))  # noqa: E731
    inside = lambda v: 2 * per < v["s"] and v["e"] <= 3 * per  # noqa: E731  (no slice edge is involved)
    out.append(sl("round_s0: s % 64 == 0, not a slice start", small, m_small, 2 * per + 64, lambda v: v["s"] % 64 == 0 and inside(v)))
    out.append(sl("round_s1: s % 64 == 1", small, m_small, 2 * per + 65, lambda v: v["s"] % 64 == 1 and inside(v)))
    out.append(sl("round_s63: the stretch starts on lane 63 and is carried", small, m_small, 2 * per + 63, lambda v: v["s"] % 64 == 63 and inside(v)))
    out.append(sl("round_e_inside: e inside the round of s", small, m_small, 2 * per + 10, lambda v: v["s"] // 64 == v["e"] // 64 and inside(v)))
    out.append(sl("round_e_on_end: e exactly on the round's end", small, m_small, 2 * per + 64 - m_small, lambda v: v["e"] % 64 == 0 and v["s"] // 64 == (v["e"] - 1) // 64 and inside(v)))
    out.append(sl("round_e_one_past: e one past the round's end (one carried anchor)", small, m_small, 2 * per + 65 - m_small, lambda v: v["e"] % 64 == 1 and inside(v)))
    out.append(sl("round_headless: the stretch spans three rounds and more, whole rounds without a head", big, m_big, 2 * per + 10, lambda v: (v["e"] - 1) // 64 - v["s"] // 64 >= 3))
    s = 2 * BLOCK - m_mid
    out.append(case("last_n64: the stretch ends the list, n % 64 == 0 (the loop after the rounds)", mid, m_mid, s, 0, lambda v: v["e"] == v["n"] and v["n"] % 64 == 0 and v["s"] // 64 < (v["e"] - 1) // 64))
    out.append(case("last_odd: the stretch ends the list, n % 64 != 0", mid, m_mid, s + 7, 0, lambda v: v["e"] == v["n"] and v["n"] % 64 != 0))
    out.append(case("first: the stretch starts the list (index 0 dropped)", small, m_small, 0, 2 * BLOCK, lambda v: v["s"] == 0))
    # slices
    out.append(sl("slice_s_at_start: s exactly at a slice start", small, m_small, 3 * per, lambda v: v["s"] % per == 0))
    out.append(sl("slice_start_1_in: s one before a slice start, the slice start one anchor in", small, m_small, 3 * per - 1, lambda v: v["s"] % per == per - 1))
    out.append(sl("slice_start_70_in: a slice start more than 64 anchors inside the stretch", mid, m_mid, 3 * per - 70, lambda v: v["s"] + 64 < 3 * per < v["e"]))
    out.append(sl("slice_covered: the stretch covers a whole slice and ends in the next", mid, m_mid, 2 * per - 5, lambda v: v["s"] < 2 * per and 3 * per < v["e"] < 4 * per))
    out.append(sl("slice_e_at_hi: e exactly at hi", small, m_small, 4 * per - m_small, lambda v: v["e"] % per == 0))
    out.append(sl("slice_past_hi: the stretch starts in a slice and goes on past hi (gene == g_hi)", small, m_small, 4 * per - 5, lambda v: v["s"] < 4 * per < v["e"]))
    out.append(case("one_wave: fewer than 64 anchors in all", small, m_small, 13, 9, lambda v: v["n"] < 64))
    # compaction
    out.append(case("chunk_drop_then_keep: drops in chunk 0, kept anchors in chunk 1", small, m_small, BLOCK - 100, 300, lambda v: v["e"] < BLOCK < v["n"]))
    out.append(case("chunk_511_512: drops at list index 511 and 512", small, m_small, BLOCK - 11, 300, lambda v: v["s"] < BLOCK - 1 and v["e"] > BLOCK))
    out.append(case("all_dropped: every anchor of the assembly is dropped", small, m_small, 0, 0, lambda v: v["s"] == 0 and v["e"] == v["n"]))
    return out


def two_gene_case(B: Builder) -> Case:
    """Drops in two genes owned by two waves: R (two seeds) in slice 0, L (two seeds, second window) from slice 1 on."""
    rng = np.random.default_rng([7600, 9])
    l_block = copies(rng, cassette(G_L, *B.unit(G_L, 2, BINS + 100, BINS + 500)), "+-" * 5 + "+")
    r = r_block(B, 4, full=1)
    m_r = len(B.anchors(asm_of("m", [r])))
    s = 64 - 10
    asm = asm_of("two_genes_two_waves", [*B.planted(range(N_FILL), s), r, l_block, *B.planted(range(G_TAIL, G_TAIL + N_TAIL), 200)])
    n = s + m_r + 2 * (MID + 1) + 200
    return Case("two_genes_two_waves: drops in two genes owned by two waves", asm, dict(s=s, e=s + m_r, n=n, drops=True, state=1, mid_occ=MID, over={G_R: [2], G_L: [0, 2, 0]}),
                lambda v: v["s"] // slice_per(v["n"]) == 0 and v["e"] // slice_per(v["n"]) >= 1)


# ---- B. counting -------------------------------------------------------------------------------------------------------------------
def counting_cases(B: Builder) -> list[Case]:
    out = []
    rng = np.random.default_rng([7700])
    ru = cassette(G_R, *B.unit(G_R, 2, 100, 400))
    pos_r = sorted(seed_counts(B.anchors(asm_of("u", [ru])), G_R))
    for strands, name in (("+" * MID, "kept_fwd"), ("+" * (MID + 1), "cut_fwd"), ("+-" * (MID // 2), "kept_both"), ("+-" * (MID // 2) + "-", "cut_both"),
                          ("-" * (MID + 1), "cut_rev")):  # fmt: skip
        cut = len(strands) > MID
        asm = asm_of(name, [copies(rng, ru, strands), *B.planted(range(N_FILL), 30)])
        out.append(Case(f"{name}: a seed with {len(strands)} anchors on strands {strands}", asm,
                        dict(counts={G_R: {p: len(strands) for p in pos_r}}, drops=cut, state=int(cut), mid_occ=MID, pairs={G_R: len(strands)})))
    # the certificate's edge: ten / eleven pairs and no seed beyond ten
    ru2 = cassette(G_R, *B.unit(G_R, 2, 450, 680))
    for extra, name in ((0, "pairs_10"), (1, "pairs_11")):
        contig = np.concatenate([copies(rng, ru, "+-" * (MID // 2)), copies(rng, ru2, "+" * extra)])
        out.append(Case(f"{name}: {MID + extra} pairs, no seed beyond {MID}: the certificate {'fails' if extra else 'passes'}, nothing is dropped",
                        asm_of(name, [contig, *B.planted(range(N_FILL), 70)]), dict(pairs={G_R: MID + extra}, drops=False, state=0, mid_occ=MID)))
    # the window's edge: a repeated seed at forward position OCC_BINS - 1 / OCC_BINS, on either strand; a gene's last position
    for gene in (G_B1024, G_B1025, G_B1039, G_L):
        glen = len(B.g[gene])
        for pos in EDGE_POSITIONS[gene]:
            edge_unit = cassette(gene, *B.unit_at(gene, pos))
            for strands, sname in (("+" * (MID + 1), "fwd"), ("-+" * (MID // 2) + "-", "both")):
                name = f"edge_g{gene}_p{pos}_{sname}"
                asm = asm_of(name, [*B.planted(range(N_FILL), 40), copies(rng, edge_unit, strands)])
                over = [0] * ((glen + BINS - 1) // BINS)
                over[pos // BINS] = 1
                out.append(Case(f"{name}: a seed at forward position {pos} of a gene of {glen} bases, {MID + 1} anchors ({sname})", asm,
                                dict(counts={gene: {pos: MID + 1}}, over={gene: over}, drops=True, state=1, mid_occ=MID)))
    # L with drops in window 0 and in window 2: window 2 walks over the tombstones of window 0 (a kept seed in window 1)
    u0, u1, u2 = B.unit(G_L, 1, 200, 600), B.unit(G_L, 1, BINS + 200, BINS + 600), B.unit(G_L, 1, 2 * BINS + 20, 2 * BINS + 230)
    contig = np.concatenate([copies(rng, cassette(G_L, *u0), "+-" * 5 + "+"), copies(rng, cassette(G_L, *u1), "+-" * 4), copies(rng, cassette(G_L, *u2), "-+" * 5 + "-")])
    out.append(Case("windows_0_and_2: drops in the first and third window of L, kept anchors in the second", asm_of("windows_0_and_2", [contig, *B.planted(range(N_FILL), 100)]),
                    dict(over={G_L: [1, 0, 1]}, drops=True, state=1, mid_occ=MID)))
    return out


# ---- C. floor or quantile ----------------------------------------------------------------------------------------------------------
def quantile_cases(B: Builder) -> list[Case]:
    """Small assemblies: the quantile is the largest count, above the floor.  Whether it is ASKED decides."""
    out = []
    rng = np.random.default_rng([7800])
    x11 = "+-" * 5 + "+"
    r2, r3 = cassette(G_R, *B.unit(G_R, 2, 100, 400)), cassette(G_R, *B.unit(G_R, 3, 100, 400))
    l2 = cassette(G_L, *B.unit(G_L, 2, 100, 600))
    l1b = cassette(G_L, *B.unit(G_L, 1, BINS + 100, BINS + 600))
    l1a = cassette(G_L, *B.unit(G_L, 1, 100, 600))
    fill = B.planted(range(N_FILL), 90)
    out.append(Case("two_over: two seeds beyond the floor, the floor cuts", asm_of("two_over", [*fill, copies(rng, r2, x11)]),
                    dict(over={G_R: [2]}, drops=True, state=1, mid_occ=MID, n_over_max=2)))
    out.append(Case("three_over: a third seed, the quantile decides and keeps them; 11 pairs <= mid_occ in phase 1", asm_of("three_over", [*fill, copies(rng, r3, x11)]),
                    dict(over={G_R: [3]}, drops=False, state=3, mid_occ=MID + 2, n_over_max=3, pairs={G_R: MID + 1})))
    out.append(Case("two_plus_one_windows: 2 + 1 seeds in two windows of L, the quantile decides", asm_of("two_plus_one_windows", [*fill, copies(rng, l2, x11), copies(rng, l1b, x11)]),
                    dict(over={G_L: [2, 1, 0]}, drops=False, state=3, mid_occ=MID + 2, n_over_max=3)))
    out.append(Case("two_plus_one_genes: 2 + 1 seeds in two genes, the floor", asm_of("two_plus_one_genes", [*fill, copies(rng, r2, x11), copies(rng, l1a, x11)]),
                    dict(over={G_R: [2], G_L: [1, 0, 0]}, drops=True, state=1, mid_occ=MID, n_over_max=2)))
    # exactly mid_occ copies and mid_occ + 1 in one assembly: 10 001 distinct minimizers and more put two counts above the
    # quantile's index -- B1024's seed in 13 copies and R's in 12 --, L's three seeds in 11 copies ask for the quantile and are
    # what it reads: mid_occ = 12
    b1 = cassette(G_B1024, *B.unit(G_B1024, 1, 100, 600, salt=-1))  # (bare: the gene's seed is the only value repeated with it)
    r1 = cassette(G_R, *B.unit(G_R, 1, 100, 400, salt=-1))
    l3 = cassette(G_L, *B.unit(G_L, 3, 100, 600))
    asm = asm_of("mid_occ_and_one_more", [copies(rng, l3, x11), copies(rng, r1, "+" * (MID + 2)), copies(rng, b1, "+" * (MID + 3)), background(1, 70_000)])
    out.append(Case("mid_occ_and_one_more: one gene's seed in exactly mid_occ = 12 copies (kept), another's in 13 (dropped)", asm,
                    dict(all_counts={G_R: MID + 2, G_B1024: MID + 3}, over={G_L: [3, 0, 0]}, drops=True, state=3, mid_occ=MID + 2, n_over_max=3, min_distinct=10_001)))
    # with a background: the quantile is worked out and FALLS BELOW the floor's successor -- mid_occ stays at the floor and cuts
    r3b = cassette(G_R, *B.unit(G_R, 3, 100, 400, salt=-1))  # (bare: three repeated values, 2e-4 of 15 000 distinct ones)
    asm = asm_of("quantile_at_floor", [copies(rng, r3b, "+" * (MID + 1)), background(2, 400_000)])
    out.append(Case("quantile_at_floor: three seeds ask for the quantile, which is below the floor: the floor cuts", asm,
                    dict(over={G_R: [3]}, drops=True, state=3, mid_occ=MID, n_over_max=3)))
    return out


# ---- D. sketch tables --------------------------------------------------------------------------------------------------------------
def trigger(B: Builder, seed: int) -> np.ndarray:
    """A contig that makes the assembly claim a counting table: three seeds of R in eleven copies."""
    return copies(np.random.default_rng([7900, seed]), cassette(G_R, *B.unit(G_R, 3, 100, 400)), "+-" * 5 + "+")


def _slot(n: int) -> int:
    return (n + 31) // 32 * 32  # contigs start on 32-base boundaries of the padded space


def sketch_cases(B: Builder) -> list[Case]:
    out = []
    rng = np.random.default_rng([8000])
    r = lambda n: random_dna(rng, n, 0.5)  # noqa: E731
    want = dict(state=3, table=True)
    lens = (K - 1, K, K + C["KP_W"] - 1, K + C["KP_W"], CHUNK - 1, CHUNK, CHUNK + 1)
    out.append(Case(f"contig_lengths: contigs of {lens} bases", asm_of("contig_lengths", [*[r(n) for n in lens], trigger(B, 1)]), dict(want, ctg_len=lens)))
    # layouts: (start, length) in the padded space, derived from the chunk size
    five = [r(n) for n in (15, 40, 22, 31, 17)]  # 5 slots of 32 or 64 bases: all inside chunk 0
    used = sum(_slot(len(c)) for c in five)
    assert used < CHUNK
    contigs, at, marks = list(five), used, {}
    for tail_in_next in (1, K + C["KP_W"], K + C["KP_W"] + 1):  # the last 1, 25 and 26 bases in the next chunk
        end = (at // CHUNK + 1) * CHUNK + tail_in_next
        if end - at < 60:
            end += CHUNK
        marks[f"end_{tail_in_next}"] = (at, end - at)
        contigs.append(r(end - at))
        at += _slot(end - at)
    start = (at // CHUNK + 1) * CHUNK - 64  # a contig that starts fewer than OCC_WARM bases before a chunk edge
    contigs.append(r(start - at - 31))  # (fills the slots up to `start`)
    marks["warm_start"] = (start, 300)
    contigs.append(r(300))
    assert 64 < WARM
    out.append(Case("contig_layouts: five contigs in one chunk; last 1 / 25 / 26 bases in the next chunk; a start inside the warm-up of a chunk edge",
                    asm_of("contig_layouts", [*contigs, trigger(B, 2)]), dict(want, marks=marks, n_in_chunk0=5)))
    # N runs, one contig from padded position 0
    c = r(7 * CHUNK + 100)
    runs = {"ends_at_edge": (CHUNK - 40, CHUNK), "starts_at_edge": (2 * CHUNK, 2 * CHUNK + 37), "whole_chunk": (3 * CHUNK, 4 * CHUNK),
            "in_warm_up": (6 * CHUNK - WARM + 20, 6 * CHUNK - WARM + 31), "first_base": (0, 1), "last_base": (len(c) - 1, len(c))}  # fmt: skip
    for a, b in runs.values():
        c[a:b] = ord("N")
    out.append(Case("n_runs: N runs at chunk edges, over a whole chunk, in the warm-up zone, on a contig's first and last base",
                    asm_of("n_runs", [c, trigger(B, 3)]), dict(want, runs=runs)))
    # low complexity across chunk edges: ties in every window
    units = (b"A", b"AC", b"ACG", b"ACGTTGA", b"ACGGTCATTGCA")
    c = r((len(units) + 1) * 2 * CHUNK)
    spans = {}
    for i, unit in enumerate(units):
        edge = (2 * i + 1) * CHUNK
        rep = np.frombuffer(unit * (160 // len(unit) + 1), np.uint8)[:160]
        c[edge - 80 : edge + 80] = rep
        spans[unit.decode()] = (edge - 80, edge + 80)
    out.append(Case("low_complexity: a homopolymer and unit repeats of period 2, 3, 7 and 12 across chunk edges", asm_of("low_complexity", [c, trigger(B, 4)]), dict(want, spans=spans)))
    return out


def second_chunk_case(B: Builder) -> Case:
    """More than OCC_PARTS * 256 * OCC_CHUNK padded positions: every thread of a table's blocks takes a second chunk; the repeats
    and the gene under test lie beyond that position."""
    big = background(3, SECOND_CHUNK + 300_000 - 8_000)
    rng = np.random.default_rng([8100])
    element = random_dna(rng, 300, 0.5)
    rest = np.concatenate([copies(rng, element, "+-" * 10), background(4, 4_000)])
    return Case("second_chunk: an assembly of more than 8 388 608 padded positions, its repeats beyond them", asm_of("second_chunk", [big, rest, trigger(B, 5)]),
                dict(state=3, table=True, min_padded=SECOND_CHUNK + 1, repeats_after=SECOND_CHUNK))


# ---- E. quantile -------------------------------------------------------------------------------------------------------------------
def distinct_cases(B: Builder, oracle) -> list[Case]:
    """Exactly n distinct minimizers on both sides of the steps of kth: poly-A (2000 times one value) and poly-C (1500 times
    another) are far above the rest, the trigger's values (eleven times each) follow, everything else occurs once or twice."""
    out = []
    fixed = [trigger(B, 6), np.full(2000 + K, ord("A"), np.uint8), np.full(1500 + K, ord("C"), np.uint8)]
    dup = background(5, 600)
    for n in (4999, 5000, 5001, 5002, 10_000, 10_001):
        bg = background(6, 6 * n + 2000)
        count = lambda length: len(minimizer_histogram(oracle, asm_of("d", [*fixed, dup, dup, bg[:length]]).packed())[0])  # noqa: E731
        lo, hi = K, len(bg)
        assert count(hi) >= n
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if count(mid) >= n else (mid + 1, hi)
        length = next((x for d in range(40) for x in (lo + d, lo - d) if count(x) == n), None)
        assert length, f"no background gives exactly {n} distinct minimizers"
        kth = kth_of(n)
        top = {1: 2000, 2: 1500}.get(n - kth, MID + 1)  # the count at kth: n - kth - 1 counts lie above it
        out.append(Case(f"distinct_{n}: {n} distinct minimizers, kth = n - {n - kth}", asm_of(f"distinct_{n}", [*fixed, dup, dup, bg[:length]]),
                        dict(state=3, table=True, distinct=n, kth=kth, count_at_kth=top, mid_occ=top + 1)))
    return out


def cap_cases(B: Builder) -> list[Case]:
    """A count of KP_MID_OCC_HIST - 2, - 1, KP_MID_OCC_HIST and 5000 at the quantile (fewer than 5000 distinct: kth = n - 1)."""
    out = []
    hist = C["KP_MID_OCC_HIST"]
    for count in (hist - 2, hist - 1, hist, 5000):
        asm = asm_of(f"poly_a_{count}", [trigger(B, 7), np.full(count + K, ord("A"), np.uint8), background(7, 3000)])
        out.append(Case(f"poly_a_{count}: one minimizer {count} times at the quantile", asm, dict(state=3, table=True, count_at_kth=count, mid_occ=min(count, hist - 1) + 1)))
    return out


# a database and an assembly of their own: ONE distinct minimizer in a claimed table.  A homopolymer run of the gene puts the
# same seed value on POLY_RUN - K + 1 forward positions, each of which gets every occurrence in the assembly as an anchor: one
# value, more than KP_MIN_ANCHORS seeds beyond the floor.
POLY_RUN = K + C["KP_W"] + 1


def single_value_gene_sequences() -> Sequences:
    rng = np.random.default_rng([8300])
    gene = np.concatenate([random_dna(rng, 120, 0.5), np.full(POLY_RUN, ord("A"), np.uint8), random_dna(rng, 120, 0.5)])
    return Sequences.from_records([SeqRecord("poly", gene.tobytes())])


def single_value_cases() -> list[Case]:
    """Pure poly-A assemblies of one contig: n = 1 distinct minimizer, kth = 0, mid_occ = its count + 1 (nothing is cut)."""
    return [Case(f"single_value_{n}: one contig of {n} A's, one distinct minimizer", asm_of(f"single_value_{n}", [np.full(n, ord("A"), np.uint8)]),
                 dict(state=3, table=True, distinct=1, kth=0)) for n in (POLY_RUN, 40, 60)]


def plain_neighbours() -> list[GenomeAssembly]:
    """Repeat-free neighbours of a batch: one with a few genes once, one without an anchor."""
    g = genes()
    rng = np.random.default_rng([8200])
    one = np.concatenate([random_dna(rng, 200, 0.5), g[3], random_dna(rng, 100, 0.5), revcomp(g[G_L]), random_dna(rng, 100, 0.5), g[G_TAIL + 2], random_dna(rng, 50, 0.5)])
    return [asm_of("plain_genes", [one, random_dna(rng, 4000, 0.5)]), asm_of("no_anchor", [random_dna(rng, 3000, 0.5)])]


def describe(cases, rows) -> str:
    """The table of cases a failing check prints: label and what the oracle measured."""
    return "\n".join(f"{c.label}\n    want {c.want}\n    got  {r}" for c, r in zip(cases, rows))


# ---- everything, built once a session ----------------------------------------------------------------------------------------------
_BUILT: dict = {}


def built(oracle) -> dict:
    """{"codes", "off", "odb", "groups": {name: [Case]}}: the database and every case, built once per process."""
    if not _BUILT:
        from kaptive_amd.pack import pack_sequences_flat

        codes, off = pack_sequences_flat(gene_sequences())
        odb = oracle.OracleDB(codes, off)
        B = Builder(odb)
        groups = {"A": [*list_cases(B), two_gene_case(B)], "B": counting_cases(B), "C": quantile_cases(B), "D": sketch_cases(B),
                  "D2": [second_chunk_case(B)], "E": [*distinct_cases(B, oracle), *cap_cases(B)]}  # fmt: skip
        _BUILT.update(codes=codes, off=off, odb=odb, groups=groups)
    return _BUILT


def measure(oracle, odb, case: Case) -> dict:
    """What the oracle finds in a case: the row that tests/test_occ_cut_oracle.py compares with ``case.want``."""
    pa = case.asm.packed()
    before, after = odb.anchors(pa, cut=False), odb.anchors(pa)
    n_over_max, mid_occ, asks = odb.occ(pa)
    s, e = stretch(before, G_R)
    x, cnt = minimizer_histogram(oracle, pa)
    cnt = np.sort(cnt)
    kth = kth_of(len(x))
    present = sorted(set(gene_of(before).tolist()) & set(range(G_R, G_TAIL)))
    return dict(s=s, e=e, n=len(before), kept=len(after), dropped=dropped_indices(before, after).tolist(), drops=len(after) < len(before),
                state=int(n_over_max > 0) | 2 * int(asks), mid_occ=mid_occ, n_over_max=n_over_max, table=asks,
                over={g: n_over(before, g) for g in present}, counts={g: seed_counts(before, g) for g in present},
                pairs={g: n_pairs(before, g) for g in present}, distinct=len(x), kth=kth, count_at_kth=int(cnt[kth]),
                table_entries=1 << table_log2(pa.n_bases), padded=pa.padded_len)  # fmt: skip
