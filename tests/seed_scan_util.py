"""Inputs that put a seed on every lane, unit, list and flank edge of the seed scan (csrc/kp_scan.hip: kp_scan_dense_kernel,
kp_edge_kernel, kp_expand_kernel), and a numpy restatement of the scan's bookkeeping that says where each of them lands.
Shared by tests/test_seed_scan_oracle.py (the inputs are what their labels say, by the model and the oracle alone) and
tests/test_gpu_seed_scan.py (the device's candidate list equals the model's, its anchors and hits the oracle's).
TEST INFRASTRUCTURE.

The MODEL (ScanModel) restates, from kp_spec.h and the comments of kp_scan.hip and with nothing shared with the product or with
oracle/kp_oracle.c: the seed value x(p) and strand bit of every position of a batch's padded stream taken as one clean
sequence (N runs and padding are code 0, the stream is zero beyond both ends, as the kernel's lanes without a unit read it),
the window rule, both presence filters (filled with the oracle's seeds of the genes), kp_seed_is_interior, and the order in
which a wave iteration lists, walks, stages and flushes: iteration `it` owns the units [62 it, 62 it + 62) on lanes 1..62, its
list is ordered by position within the unit first and by lane second, it is walked when more than DENSE_LIST - WALK_ROOM
entries are listed after eight positions and after the last eight, a round of the walk takes 64 * PROBES entries, stages those
that pass the FIRST filter and flushes when more than DENSE_STAGE - 64 * PROBES are staged.  What it expects of the device:
the FRONT candidates are the selected positions of the stream that pass both filters, the BACK candidates the oracle's seeds
of every contig that are not interior to their clean stretch and pass both filters.

The wave-stride loop of the dense kernel -- a wave that takes a second iteration with `staged` carried over -- is not
modelled: it needs a batch beyond 2048 x 4 x 62 units and stays with the full-size sweeps."""

from __future__ import annotations

import math
import re
from pathlib import Path
from typing import NamedTuple

import numpy as np

from kaptive_amd.core.genome import GenomeAssembly
from kaptive_amd.core.seq import SeqRecord, Sequences
from kaptive_amd.pack import pack_sequences_flat, words_to_codes
from kaptive_amd.synth import make_db, random_dna, revcomp

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kaptive_amd" / "csrc"


# ---- the constants the geometry hangs on, read out of the sources -------------------------------------------------------------------
def kernel_constants() -> dict[str, int]:
    scan, internal = (CSRC / "kp_scan.hip").read_text(), (CSRC / "kp_internal.h").read_text()
    spec = (ROOT / "include" / "kp_spec.h").read_text()
    out = {}
    for name in ("SCAN_OWN", "DENSE_STAGE"):
        out[name] = int(re.search(rf"constexpr int {name} = (\d+);", scan).group(1))
    for name in ("DENSE_LIST", "PROBES"):
        out[name] = int(re.search(rf"#ifndef KP_SCAN_{name}\n#define KP_SCAN_{name} (\d+)\n#endif\nconstexpr int {name} = KP_SCAN_{name};", scan).group(1))
    out["WALK_ROOM"] = int(re.search(r"if \(p0 == 56 \|\| listed > DENSE_LIST - (\d+)\) walk\(\);", scan).group(1))
    assert re.search(r"if \(staged > DENSE_STAGE - 64 \* PROBES\) flush\(\);", scan)
    m = re.search(r"const int64_t warm = E - \(KP_K \+ KP_W\) - (\d+);\s*if \(warm <= S\)", scan)
    out["EDGE_WARM"] = int(m.group(1))
    for name in ("KP_W", "KP_K", "KP_CONTIG_ALIGN", "KP_ASM_ALIGN"):
        out[name] = int(re.search(rf"#define\s+{name}\s+(\d+)u?\b", spec).group(1))
    for name in ("KP_FILTER_LOG2", "KP_FILTER2_LOG2", "KP_ANCHOR_SUBS"):
        out[name] = int(re.search(rf"#define\s+{name}\s+(\d+)\b", internal).group(1))
    return out


C = kernel_constants()
OWN, LIST, STAGE, PROBES, WALK_ROOM = C["SCAN_OWN"], C["DENSE_LIST"], C["DENSE_STAGE"], C["PROBES"], C["WALK_ROOM"]
K, W = C["KP_K"], C["KP_W"]
UNIT = 64  # bases a lane owns: one 16-byte load
ROUND = 64 * PROBES
SPLIT = K + W + C["EDGE_WARM"]  # longest clean stretch that one thread of the edge kernel takes whole
MASK30 = (1 << 30) - 1
CAND_POS_SHIFT, CAND_Z_SHIFT = 31, 30  # kp_cand_pack


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def hash30(key: np.ndarray) -> np.ndarray:
    """kp_spec.h's kp_hash30 on an array (64-bit arithmetic under the 30-bit mask gives the 32-bit function's low 30 bits)."""
    m = np.uint64(MASK30)
    key = np.asarray(key, np.uint64)
    key = (~key + (key << np.uint64(21))) & m
    key = key ^ (key >> np.uint64(24))
    key = ((key + (key << np.uint64(3))) + (key << np.uint64(8))) & m
    key = key ^ (key >> np.uint64(14))
    key = ((key + (key << np.uint64(2))) + (key << np.uint64(4))) & m
    key = key ^ (key >> np.uint64(28))
    return key.astype(np.uint32)


def kmer_values(codes: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """(fwd, rev, z, x) of the 15-mer that starts at every position of a clean code sequence (its last K - 1 positions have
    none and are left out): kp_spec.h's fwd, rev, strand bit and seed value."""
    c = np.asarray(codes, np.uint64)
    n = len(c) - K + 1
    fwd, rev = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(K):
        fwd |= c[j : j + n] << np.uint64(2 * (K - 1 - j))
        rev |= (np.uint64(3) - c[j : j + n]) << np.uint64(2 * j)
    z = (fwd >= rev).astype(np.uint8)  # (k is odd: never equal)
    return fwd, rev, z, hash30(np.where(z == 1, rev, fwd))


def window_rule(x: np.ndarray) -> np.ndarray:
    """sel[i] for i in [W - 1, len - W + 1): position i is selected iff the maximum, over the W windows of W consecutive
    positions that contain it, of the window's minimum equals x[i].  Positions closer than W - 1 to either end come out False."""
    from numpy.lib.stride_tricks import sliding_window_view as swv

    wm = swv(x, W).min(axis=1)  # wm[s] = min over [s, s + W)
    best = swv(wm, W).max(axis=1)  # best[j] = max over wm[j .. j + W - 1] = the windows that contain position j + W - 1
    sel = np.zeros(len(x), bool)
    sel[W - 1 : W - 1 + len(best)] = best == x[W - 1 : W - 1 + len(best)]
    return sel


def is_interior(t, S, E):
    """kp_seed_is_interior: the streaming kernel decides the 15-mer that starts at t of the clean stretch [S, E)."""
    return (t >= S + W) & (t + K + W <= E)


class Filters:
    """Both presence filters of kp_internal.h as bit sets over the oracle's seeds of the genes."""

    def __init__(self, xs: np.ndarray) -> None:
        self.lg1, self.lg2 = C["KP_FILTER_LOG2"], C["KP_FILTER2_LOG2"]
        self.f1 = np.zeros(1 << (self.lg1 - 6), np.uint64)
        self.f2 = np.zeros(1 << (self.lg2 - 6), np.uint64)
        xs = np.unique(np.asarray(xs, np.uint32))
        np.bitwise_or.at(self.f1, self._block1(xs), self._mask1(xs))
        np.bitwise_or.at(self.f2, self._block2(xs), self._mask2(xs))
        self.indexed = xs

    def _block1(self, x):
        return (x & np.uint32((1 << (self.lg1 - 6)) - 1)).astype(np.int64)

    @staticmethod
    def _mask1(x):
        x = x.astype(np.uint64)
        one = np.uint64(1)
        return (one << ((x >> np.uint64(18)) & np.uint64(31))) | (one << (np.uint64(32) + ((x >> np.uint64(23)) & np.uint64(31))))

    def _block2(self, x):
        return (((x.astype(np.uint64) * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - (self.lg2 - 6))).astype(np.int64)

    @staticmethod
    def _mask2(x):
        h = (x.astype(np.uint64) * np.uint64(0x27D4EB2F)) & np.uint64(0xFFFFFFFF)
        one, m = np.uint64(1), np.uint64(31)
        lo = (one << (h >> np.uint64(27))) | (one << ((h >> np.uint64(22)) & m))
        hi = (one << ((h >> np.uint64(17)) & m)) | (one << ((h >> np.uint64(12)) & m))
        return lo | (hi << np.uint64(32))

    def pass1(self, x: np.ndarray) -> np.ndarray:
        x = np.asarray(x, np.uint32)
        need = self._mask1(x)
        return (self.f1[self._block1(x)] & need) == need

    def pass2(self, x: np.ndarray) -> np.ndarray:
        x = np.asarray(x, np.uint32)
        need = self._mask2(x)
        return (self.f2[self._block2(x)] & need) == need

    def both(self, x: np.ndarray) -> np.ndarray:
        return self.pass1(x) & self.pass2(x)


def pack_cand(pos, z, x) -> np.ndarray:
    return (np.asarray(pos, np.uint64) << np.uint64(CAND_POS_SHIFT)) | (np.asarray(z, np.uint64) << np.uint64(CAND_Z_SHIFT)) | np.asarray(x, np.uint64)


def unpack_cand(words: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    w = np.asarray(words, np.uint64)
    return (w >> np.uint64(CAND_POS_SHIFT)).astype(np.int64), ((w >> np.uint64(CAND_Z_SHIFT)) & np.uint64(1)).astype(np.uint8), (w & np.uint64(MASK30)).astype(np.uint32)


class Stretch(NamedTuple):
    asm: int
    contig: int
    S: int  # batch-wide positions
    E: int
    left_n: bool  # the stretch starts behind an N run (else at its contig's start)
    right_n: bool


class Iteration(NamedTuple):
    walks: list  # list occupancy before every walk
    rounds: list  # (hits of the round, staged after it, flushed) for every round of every walk
    stage_peak: int
    n_listed: int
    n_hits: int  # selected positions that pass the first filter


def stream_scan(codes: np.ndarray, flt: Filters):
    """(x, z, sel, pass1, pass2) for every position of a stream of codes, zero beyond both ends."""
    pad = UNIT
    ext = np.concatenate([np.zeros(pad, np.uint8), np.asarray(codes, np.uint8), np.zeros(pad + K, np.uint8)])
    _, _, z, x = kmer_values(ext)
    sel = window_rule(x)
    sl = slice(pad, pad + len(codes))
    x, z, sel = x[sl], z[sl], sel[sl]
    return x, z, sel, flt.pass1(x), flt.pass2(x)


def bookkeeping(sel: np.ndarray, pass1: np.ndarray, walk_room: int = WALK_ROOM, flush_above: int = STAGE - ROUND) -> list[Iteration]:
    """The list and stage of every wave iteration over a stream of len(sel) / 64 units.  (walk_room, flush_above: the two
    thresholds, for asking what another value would do -- an OverflowError says that list or stage would overrun.)"""
    n_units = len(sel) // UNIT
    s2, h2 = sel.reshape(n_units, UNIT), (sel & pass1).reshape(n_units, UNIT)
    out = []
    for it in range((n_units + OWN - 1) // OWN):
        u0, u1 = it * OWN, min(it * OWN + OWN, n_units)  # lanes 1 .. u1 - u0
        entries: list = []
        walks, rounds, staged, peak = [], [], 0, 0
        for p0 in range(0, UNIT, 8):
            for p in range(p0, p0 + 8):
                entries.extend(h2[u0:u1, p][s2[u0:u1, p]].tolist())  # lane order within a position
            if len(entries) > LIST:
                raise OverflowError(f"iteration {it}: {len(entries)} entries listed")
            if p0 == UNIT - 8 or len(entries) > LIST - walk_room:
                walks.append(len(entries))
                for e0 in range(0, len(entries), ROUND):
                    hits = sum(entries[e0 : e0 + ROUND])
                    staged += hits
                    peak = max(peak, staged)
                    if staged > STAGE:
                        raise OverflowError(f"iteration {it}: {staged} candidates staged")
                    flushed = staged > flush_above
                    rounds.append((hits, staged, flushed))
                    if flushed:
                        staged = 0
                entries = []
        out.append(Iteration(walks, rounds, peak, int(s2[u0:u1].sum()), int(h2[u0:u1].sum())))
    return out


def contig_codes(pa) -> list[np.ndarray]:
    """Codes (0..3, 4 = ambiguous) of every contig of a packed assembly."""
    codes = words_to_codes(np.asarray(pa.words, np.uint32), pa.padded_len).copy()
    for a, b in np.asarray(pa.n_runs).reshape(-1, 2):
        codes[a:b] = 4
    return [codes[s : s + n] for s, n in zip(pa.ctg_start.tolist(), pa.ctg_len.tolist())]


def clean_stretches(codes: np.ndarray) -> list[tuple[int, int, bool, bool]]:
    """[S, E) of every maximal run without an ambiguous base, with whether an N run is on its left and on its right."""
    bad = np.r_[True, codes > 3, True]
    edges = np.flatnonzero(bad[1:] != bad[:-1])
    return [(int(s), int(e), s > 0, e < len(codes)) for s, e in edges.reshape(-1, 2)]


class ScanModel:
    """What the scan is expected to list for one batch of packed assemblies."""

    def __init__(self, world: "World", packed: list) -> None:
        oracle, flt = world.oracle, world.filters
        self.base = np.concatenate([[0], np.cumsum([pa.padded_len for pa in packed])]).astype(np.int64)
        stream = np.concatenate([words_to_codes(np.asarray(pa.words, np.uint32), pa.padded_len) for pa in packed] + [np.empty(0, np.uint8)])
        assert len(stream) % UNIT == 0
        self.n_units = len(stream) // UNIT
        self.x, self.z, self.sel, self.pass1, self.pass2 = stream_scan(stream, flt)
        both = self.sel & self.pass1 & self.pass2
        pos = np.flatnonzero(both)
        self.front = np.sort(pack_cand(pos, self.z[pos], self.x[pos]))
        self.iterations = bookkeeping(self.sel, self.pass1) if self.n_units else []
        # the oracle's seeds of every contig, by clean stretch
        self.stretches: list[Stretch] = []
        self.interior_oracle, self.edge_oracle = [], []  # per stretch: (pos, z, x) arrays, batch-wide positions
        back = []
        for a, pa in enumerate(packed):
            for c, (cs, cc) in enumerate(zip(pa.ctg_start.tolist(), contig_codes(pa))):
                start, z, x = oracle.seeds(cc)
                start = start.astype(np.int64)
                for S, E, ln, rn in clean_stretches(cc):
                    mine = (start >= S) & (start < E)
                    assert ((start[mine] + K) <= E).all()
                    inner = mine & is_interior(start, S, E)
                    edge = mine & ~inner
                    off = int(self.base[a]) + cs
                    self.stretches.append(Stretch(a, c, off + S, off + E, ln, rn))
                    self.interior_oracle.append((start[inner] + off, z[inner], x[inner]))
                    self.edge_oracle.append((start[edge] + off, z[edge], x[edge]))
                    keep = edge & flt.both(x)
                    back.append(pack_cand(start[keep] + off, z[keep], x[keep]))
        self.back = np.sort(np.concatenate(back + [np.empty(0, np.uint64)]))

    def interior_model(self, i: int):
        """The model's selected positions inside stretch i's interior: (pos, z, x)."""
        st = self.stretches[i]
        lo, hi = st.S + W, st.E - K - W + 1
        pos = np.arange(lo, hi)[self.sel[lo:hi]] if hi > lo else np.empty(0, np.int64)
        return pos, self.z[pos], self.x[pos]

    def stretch_of(self, pos: int):
        return next((s for s in self.stretches if s.S <= pos < s.E), None)

    def front_set(self) -> set:
        return set(zip(*[a.tolist() for a in unpack_cand(self.front)]))

    def rejected_front(self) -> np.ndarray:
        """Front candidates that the expansion has to reject: in no clean stretch's interior."""
        pos, _, _ = unpack_cand(self.front)
        ok = np.zeros(len(pos), bool)
        for s in self.stretches:
            ok |= (pos >= s.S) & (pos < s.E) & is_interior(pos, s.S, s.E)
        return self.front[~ok]


# ---- the database -------------------------------------------------------------------------------------------------------------------
ACGT = np.frombuffer(b"ACGT", np.uint8)
N = ord("N")


def dna(text: str) -> np.ndarray:
    return np.frombuffer(text.encode(), np.uint8).copy()


def codes_of(seq: np.ndarray) -> np.ndarray:
    lut = np.full(256, 4, np.uint8)
    lut[ACGT] = np.arange(4, dtype=np.uint8)
    return lut[seq]


def poly(base: str, n: int) -> np.ndarray:
    return np.full(n, ord(base), np.uint8)


def periodic(unit: str, n: int) -> np.ndarray:
    return np.tile(dna(unit), n // len(unit) + 1)[:n]


def near_palindromes() -> list[np.ndarray]:
    """15-mers whose reverse complement differs from them in the middle base only: 7 bases, a middle base, the reverse
    complement of the 7 -- with a seed value in the lowest thirtieth of the range, so that most contexts make them seeds.
    (A 15-mer equal to its reverse complement cannot exist: the middle base would be its own complement.)"""
    rng = np.random.default_rng(9107)
    out = []
    for mid in "ACGT":
        while True:
            left = random_dna(rng, 7, 0.5)
            pal = np.concatenate([left, dna(mid), revcomp(left)])
            if int(kmer_values(codes_of(pal))[3][0]) < (1 << 30) // 30:
                break
        out.append(pal)
    return out


def tie_block(d: int) -> tuple[np.ndarray, int]:
    """(block, i): random flanks around K + d bases of period d -- two equal 15-mers exactly d positions apart, at i and i + d --
    drawn until both are window minima of the block (the flanks are longer than a window: they stay minima wherever the block is planted)."""
    rng = np.random.default_rng([9108, d])
    flank = K + W + 5
    while True:
        block = np.concatenate([random_dna(rng, flank, 0.5), np.tile(random_dna(rng, d, 0.5), 4)[: K + d], random_dna(rng, flank, 0.5)])
        x = kmer_values(codes_of(block))[3]
        sel = window_rule(x)
        if sel[flank] and sel[flank + d] and x[flank] == x[flank + d] and (x == x[flank]).sum() == 2:
            return block, flank


FAR_KINDS = ("below_only_window", "below_false_positive", "above_only_window", "above_false_positive")


def far_blocks() -> dict[str, tuple[np.ndarray, int]]:
    """{kind: (block of 2 W - 1 + K - 1 bases, q)}: the decision at block position q hangs on the value NINE positions away, the
    farthest one a lane takes from a neighbour.  *_only_window: x(q) is the minimum of the one window that ends (below) or starts
    (above) at q and of no other -- selected; *_false_positive: the value nine away is smaller, the eight between are larger and
    the neighbour on the other side is smaller -- not selected, but selected by a scan that misses the ninth value."""
    rng = np.random.default_rng(9109)
    out: dict = {}
    q = W - 1
    while len(out) < len(FAR_KINDS):
        block = random_dna(rng, 2 * W - 1 + K - 1, 0.5)
        x = kmer_values(codes_of(block))[3].astype(np.int64)
        lo, hi = x[:q], x[q + 1 :]  # positions q - 9 .. q - 1 and q + 1 .. q + 9
        if len(set(x.tolist())) < len(x):
            continue
        if hi[0] < x[q] < lo.min():
            out.setdefault("below_only_window", (block, q))
        if hi[0] < x[q] < lo[1:].min() and lo[0] < x[q]:
            out.setdefault("below_false_positive", (block, q))
        if lo[-1] < x[q] < hi.min():
            out.setdefault("above_only_window", (block, q))
        if lo[-1] < x[q] < hi[:-1].min() and hi[-1] < x[q]:
            out.setdefault("above_false_positive", (block, q))
    return out


TIE_RUN = K + W - 1 + 6  # a run whose 15-mers fill a window of ties and more
PERIODS = ("AC", "ACG", "ACGG", "AACGT", "AACCGT", "AACCGTT", "AACCGTGT")  # (none equal to its own reverse complement)  # periods 2..8, indexed through the extra gene
FAMILY, FAMILY_BLOCK = 12, 300


def extra_gene() -> np.ndarray:
    """The tie-dense values and the near-palindromes that are in the index: a homopolymer run, a run of every period 2..8 and
    a 24-mer of period 9 (two equal 15-mers nine positions apart), and every near-palindrome preceded and followed by each of
    the four bases, between random spacers."""
    rng = np.random.default_rng(9101)
    sp = lambda: random_dna(rng, 40, 0.5)  # noqa: E731
    parts = [sp(), poly("A", TIE_RUN), sp()]
    for u in PERIODS:
        parts += [periodic(u, TIE_RUN + len(u)), sp()]
    parts += [tie_block(9)[0], sp(), tie_block(10)[0], sp()]
    for pal in near_palindromes():
        for b in "ACGT":
            parts += [dna(b), pal, dna(b), sp()]
    return np.concatenate(parts)


class World:
    """The database of the cases (make_db's genes, the extra gene, a gene family), its oracle index and its filters."""

    def __init__(self, oracle) -> None:
        self.oracle = oracle
        db = make_db("kpsc_k", seed=7, n_loci=4)
        g = db.genes
        self.genes = [g.seqs[int(o) : int(o) + int(n)].copy() for o, n in zip(g.offsets, g.lengths)]
        self.g_extra = len(self.genes)
        self.genes.append(extra_gene())
        rng = np.random.default_rng(9102)
        self.block = random_dna(rng, FAMILY_BLOCK, 0.5)
        self.g_family = len(self.genes)
        for _ in range(FAMILY):  # one 300-base block in every gene of the family
            self.genes.append(np.concatenate([random_dna(rng, 120, 0.5), self.block, random_dna(rng, 120, 0.5)]))
        self.g_far = len(self.genes)
        for block, q in far_blocks().values():  # genes of one 15-mer each: the far-neighbour blocks' deciding values are in the index
            self.genes.append(block[q : q + K].copy())
        seqs = Sequences.from_records([SeqRecord(f"g{i}", s.tobytes()) for i, s in enumerate(self.genes)])
        self.codes, self.off = pack_sequences_flat(seqs)
        self.odb = oracle.OracleDB(self.codes, self.off)
        self.gene_seeds = [oracle.seeds(self.codes[self.off[i] : self.off[i + 1]]) for i in range(len(self.genes))]
        self.filters = Filters(np.concatenate([s[2] for s in self.gene_seeds]))
        self._material = np.concatenate(self.genes[: self.g_extra])

    def indexed(self, x) -> np.ndarray:
        return np.isin(np.asarray(x, np.uint32), self.filters.indexed)

    def material(self, n: int, at: int = 0) -> np.ndarray:
        """n bases cut from the genes laid end to end (every seed away from a junction is an anchor)."""
        at %= len(self._material) - n
        return self._material[at : at + n].copy()

    def gene_piece(self, gene: int, a: int, n: int) -> np.ndarray:
        return self.genes[gene][a : a + n].copy()

    def model(self, asms) -> ScanModel:
        return ScanModel(self, [a.packed() for a in asms])


def asm_of(name: str, contigs) -> GenomeAssembly:
    return GenomeAssembly(name, Sequences.from_records([SeqRecord(f"c{i}", np.asarray(c, np.uint8).tobytes()) for i, c in enumerate(contigs)]))


class Case(NamedTuple):
    name: str
    asms: list  # the batch
    marks: dict  # what the labels are about: positions, parts, expected occupancies (tests/test_seed_scan_oracle.py reads them)
    cut_removes: bool = False  # the occurrence cut removes the anchors the label is about: pinned through the candidates only


def _slot(n: int) -> int:
    return (n + C["KP_CONTIG_ALIGN"] - 1) // C["KP_CONTIG_ALIGN"] * C["KP_CONTIG_ALIGN"]


def seeded_kmer(world: World, gene: int, lo: int = 40, nth: int = 0) -> int:
    """Start of the nth seed of a gene at or behind `lo` whose value occurs once in the index (with 40 bases of the gene behind it)."""
    start, _, x = world.gene_seeds[gene]
    allx = np.concatenate([s[2] for s in world.gene_seeds])
    found = 0
    for s, v in zip(start.tolist(), x.tolist()):
        if s >= lo and s + K + 40 < len(world.genes[gene]) and (allx == v).sum() == 1:
            if found == nth:
                return s
            found += 1
    raise AssertionError("no such seed")


# ---- a. phase sweep -----------------------------------------------------------------------------------------------------------------
def probe_contigs(world: World) -> tuple[list[np.ndarray], dict]:
    """The probe assembly's contigs and the part (contig index) of every kind of contig it holds."""
    s0 = seeded_kmer(world, 0)
    s1 = seeded_kmer(world, 1)
    with_n = world.gene_piece(2, 100, 400)
    with_n[150] = N  # an N run of one base
    with_n[260:300] = N  # and one of forty
    parts = {
        "gene_piece_a": world.gene_piece(3, 50, 333),
        "len_1": world.gene_piece(0, s0, 1),
        "len_14": world.gene_piece(0, s0, 14),
        "len_15": world.gene_piece(0, s0, 15),  # one 15-mer: mm_sketch's last minimum
        "len_16": world.gene_piece(1, s1, 16),
        "n_runs": with_n,
        "periodic": np.concatenate([world.gene_piece(4, 30, 90), periodic(PERIODS[1], TIE_RUN + 3), world.gene_piece(4, 200, 90)]),
        "abutting": world.gene_piece(5, 64, 8 * C["KP_CONTIG_ALIGN"]),  # fills its slots: the next contig starts on its last base + 1
        "gene_piece_b": revcomp(world.gene_piece(6, 20, 421)),
    }
    names = list(parts)
    used = sum(_slot(len(c)) for c in parts.values())
    # the last contig ends on the assembly's last base, and the padded length is 64 P with gcd(P, 62) = 1
    last = C["KP_CONTIG_ALIGN"] * 5
    while (used + last) % UNIT or math.gcd((used + last) // UNIT, OWN) != 1:
        last += C["KP_CONTIG_ALIGN"]
    parts["last"] = world.gene_piece(7, 33, last)
    names.append("last")
    return [parts[n] for n in names], {n: i for i, n in enumerate(names)}


def phase_case(world: World) -> Case:
    contigs, part = probe_contigs(world)
    probe = asm_of("probe", contigs)
    P = probe.packed().padded_len // UNIT
    asms = [asm_of(f"probe{j}", contigs) for j in range(OWN)]
    return Case("a_phase_sweep", asms, dict(P=P, part=part, probe=probe))


# ---- b. word and unit offsets -------------------------------------------------------------------------------------------------------
def planted(world: World, at: int, piece: np.ndarray, total_units: int, salt: int = 0) -> np.ndarray:
    """One contig of total_units units of gene material with `piece` written over it from base `at`."""
    c = world.material(total_units * UNIT, 977 * salt + 13)
    c[at : at + len(piece)] = piece
    return c


def offset_cases(world: World) -> list[Case]:
    """A gene's seed, with the W + K bases on either side that make it one, so that its 15-mer starts at each of the 64 offsets
    of a unit; near-palindromes between every pair of flanking bases in contigs."""
    g = 8
    s = seeded_kmer(world, g, lo=60)
    piece = world.gene_piece(g, s - 30, 2 * 30 + K)
    contigs, marks = [], {}
    for o in range(UNIT):
        at = 3 * UNIT + o - 30  # the 15-mer starts at offset o of unit 3 of its contig
        contigs.append(planted(world, at, piece, 6, salt=o))
    asm = asm_of("offsets", contigs)
    pa = asm.packed()
    marks["kmer_pos"] = [int(pa.ctg_start[o]) + 3 * UNIT + o for o in range(UNIT)]
    marks["x"] = int(world.gene_seeds[g][2][world.gene_seeds[g][0].tolist().index(s)])
    pal_contigs = []
    rng = np.random.default_rng(9110)
    for pal in near_palindromes():
        for before in "ACGT":
            for after in "ACGT":
                pal_contigs.append(np.concatenate([random_dna(rng, 31, 0.5), dna(before), pal, dna(after), random_dna(rng, 32, 0.5)]))
    pal_contigs.append(world.genes[world.g_extra].copy())
    pal_contigs.append(revcomp(world.genes[world.g_extra]))
    return [Case("b_unit_offsets", [asm], marks), Case("b_near_palindromes", [asm_of("palindromes", pal_contigs)], dict(n_pal=len(near_palindromes())))]


# ---- c. neighbour reach -------------------------------------------------------------------------------------------------------------
REACH_OFFSETS = (0, 8, 9, 63, 55, 54)
BOUNDARIES = (5, OWN)  # a unit boundary inside an iteration; the boundary between lane 62 of iteration 0 and lane 1 of iteration 1


def reach_case(world: World) -> Case:
    """Strict window minima at positions 0, 8, 9 of the unit behind a boundary and 63, 55, 54 of the unit before it, and ties
    9 and 10 positions apart across it, and the four far-neighbour blocks at it: one assembly each, a single contig from padded position 0 (batch unit = contig unit
    needs every assembly's length to be a multiple of 62 units: two iterations each)."""
    asms, marks = [], {"minima": [], "ties": [], "far": []}
    total = 2 * OWN
    g = 9
    base = 0
    salt = 0
    for b in BOUNDARIES:
        for o in REACH_OFFSETS:
            s = seeded_kmer(world, g, lo=60, nth=len(asms) % 3)
            unit = b if o < 32 else b - 1
            at = unit * UNIT + o
            piece = world.gene_piece(g, s - 40, 80 + K)
            asms.append(asm_of(f"reach_b{b}_o{o}", [planted(world, at - 40, piece, total, salt := salt + 1)]))
            marks["minima"].append((base + at, b, o))
            base += total * UNIT
        for d in (9, 10):
            piece, i = tie_block(d)  # as in the extra gene: both copies are in the index
            for first in (UNIT - 1, UNIT - 5):  # the first copy in the unit before the boundary, the second behind it
                at = (b - 1) * UNIT + first
                asms.append(asm_of(f"ties_b{b}_d{d}_{first}", [planted(world, at - i, piece, total, salt := salt + 1)]))
                marks["ties"].append((base + at, base + at + d, b, d))
                base += total * UNIT
        for kind, (block, q) in far_blocks().items():
            at = b * UNIT if kind.startswith("below") else b * UNIT - 1  # position 0 behind the boundary / position 63 before it
            asms.append(asm_of(f"far_b{b}_{kind}", [planted(world, at - q, block, total, salt := salt + 1)]))
            marks["far"].append((base + at, b, kind))
            base += total * UNIT
    return Case("c_neighbour_reach", asms, marks)


# ---- d. list and stage --------------------------------------------------------------------------------------------------------------
def _units_case(name: str, world: World, middle: np.ndarray, marks: dict, cut_removes=True) -> Case:
    """One assembly, one contig from padded position 0: iteration 0 and iteration 2 of gene material, iteration 1 = `middle`
    (62 units).  The material next to it is the middle's own first and last unit repeated, so that no lane of iteration 1 reads a
    foreign neighbour."""
    assert len(middle) == OWN * UNIT
    before, after = world.material(OWN * UNIT, 101), world.material(OWN * UNIT, 5003)
    before[-UNIT:] = middle[:UNIT]
    after[:UNIT] = middle[-UNIT:]
    return Case(name, [asm_of(name, [np.concatenate([before, middle, after])])], marks, cut_removes)


def _middle_model(world: World, middle: np.ndarray):
    """Iteration 1's bookkeeping for a candidate middle, without building an assembly."""
    stream = np.concatenate([middle[:UNIT], middle, middle[-UNIT:]])
    x, z, sel, p1, p2 = stream_scan(codes_of(stream), world.filters)
    core = slice(UNIT, UNIT + OWN * UNIT)
    return bookkeeping(sel[core], p1[core])[0], sel[core].reshape(OWN, UNIT), (sel & p1)[core].reshape(OWN, UNIT)


def dense_prefixed(rng, prefix_len: np.ndarray, kinds: list) -> np.ndarray:
    """62 units of poly-A, each behind a prefix of prefix_len[l] bases: kinds[l] = a base (a run of it) or 'R' (random)."""
    out = np.full((OWN, UNIT), ord("A"), np.uint8)
    for l, (n, kind) in enumerate(zip(prefix_len.tolist(), kinds)):
        if n:
            out[l, :n] = random_dna(rng, n, 0.5) if kind == "R" else ord(kind)
            out[l, n - 1] = ord("C") if out[l, n - 1] == ord("A") else out[l, n - 1]  # the prefix ends where it says
    return out.reshape(-1)


def search_list_peak(world: World) -> tuple[np.ndarray, int]:
    """Which units are dense: n all-A units and 62 - n units whose first 16 15-mers hold a random base, for the n and the draw
    that bring the list closest to DENSE_LIST - WALK_ROOM entries before the next eight positions add 8 x 62."""
    best, best_peak = None, 0
    for n_dense in range(30, 18, -1):
        for seed in range(24):
            rng = np.random.default_rng([9120, n_dense, seed])
            plen = np.full(OWN, 16)
            plen[rng.choice(OWN, n_dense, replace=False)] = 0
            middle = dense_prefixed(rng, plen, ["R"] * OWN)
            it, _, _ = _middle_model(world, middle)
            if max(it.walks) > best_peak:
                best, best_peak = middle, max(it.walks)
    return best, best_peak


def search_stage(world: World, want_hits: int) -> np.ndarray:
    """A middle whose first sixteen positions list exactly 64 * PROBES entries with `want_hits` of them passing the first filter,
    and whose positions 16..23 are poly-A on every lane (8 x 62 hits): the first round of the walk stages want_hits, the
    second 64 * PROBES."""
    rng = np.random.default_rng([9130, want_hits])
    n_a, extra = divmod(want_hits, 16)  # an all-A lane has 16 hits in the first sixteen positions, a prefix of 15 bases one
    plen = np.full(OWN, 16)
    lanes = rng.permutation(OWN)
    plen[lanes[:n_a]] = 0
    assert extra <= 1
    plen[lanes[n_a : n_a + extra]] = 15
    free = lanes[n_a:]
    units = dense_prefixed(rng, plen, ["R"] * OWN).reshape(OWN, UNIT)

    def cost(u):
        _, s2, h2 = _middle_model(world, u.reshape(-1))
        n, h = int(s2[:, :16].sum()), int(h2[:, :16].sum())
        return 1000 * abs(h - want_hits) + abs(n - ROUND), n, h

    c, n, h = cost(units)
    for _ in range(4000):
        if c == 0:
            return units.reshape(-1)
        l = int(rng.choice(free))
        trial = units.copy()
        trial[l, : plen[l]] = random_dna(rng, int(plen[l]), 0.5)
        if trial[l, plen[l] - 1] == ord("A"):
            trial[l, plen[l] - 1] = ord("G")
        c2, n2, h2 = cost(trial)
        if c2 <= c:
            units, c, n, h = trial, c2, n2, h2
    raise AssertionError(f"no middle with {ROUND} entries and {want_hits} hits in the first sixteen positions ({n}, {h})")


def list_stage_cases(world: World) -> list[Case]:
    out = []
    every = poly("A", OWN * UNIT)
    out.append(_units_case("d_every_lane", world, every, dict(walks=[2 * 8 * OWN] * 4, round_hits=[ROUND, ROUND, ROUND, 2 * 8 * OWN - 3 * ROUND] * 4)))
    peak_middle, peak = search_list_peak(world)
    out.append(_units_case("d_list_peak", world, peak_middle, dict(peak=peak)))
    out.append(_units_case("d_stage_full", world, search_stage(world, STAGE - ROUND), dict(first_rounds=[(STAGE - ROUND, STAGE - ROUND, False), (ROUND, STAGE, True)])))
    out.append(_units_case("d_stage_flush", world, search_stage(world, STAGE - ROUND + 1), dict(first_rounds=[(STAGE - ROUND + 1, STAGE - ROUND + 1, True), (ROUND, ROUND, True)])))
    # a walk at an occupancy between DENSE_LIST - WALK_ROOM and DENSE_LIST - WALK_ROOM / 2: forty dense units
    rng = np.random.default_rng(9140)
    plen = np.full(OWN, 16)
    plen[rng.choice(OWN, 40, replace=False)] = 0
    out.append(_units_case("d_walk_window", world, dense_prefixed(rng, plen, ["R"] * OWN), dict(lo=LIST - WALK_ROOM, hi=LIST - WALK_ROOM // 2)))
    # an iteration of a tie-dense value that is NOT in the index: the list fills, nothing is staged
    out.append(_units_case("d_nothing_passes", world, poly("C", OWN * UNIT), dict(n_hits=0, walks=[2 * 8 * OWN] * 4), cut_removes=False))
    # an iteration that lists fewer than DENSE_LIST - WALK_ROOM entries in all: its only walk is the last one
    out.append(_units_case("d_final_walk_only", world, periodic(PERIODS[-1], OWN * UNIT), dict(n_walks=1), cut_removes=False))
    # tie-dense units of every period, indexed, next to each other
    mixed = np.concatenate([periodic(u, 6 * UNIT) for u in PERIODS] + [poly("A", 6 * UNIT), poly("C", 6 * UNIT), poly("T", 6 * UNIT)] + [periodic("AG", 2 * UNIT)])
    out.append(_units_case("d_periods", world, mixed, dict(), cut_removes=False))
    return out


# ---- e. expansion -------------------------------------------------------------------------------------------------------------------
def split_kmer(world: World) -> tuple[np.ndarray, np.ndarray, int]:
    """(head, tail, s): two contigs of gene material, the first of a length that fills its slots, that hold a gene's seed 15-mer
    split 7 + 8 across their boundary -- in the stream it is whole."""
    g = 10
    n = 2 * C["KP_ASM_ALIGN"]
    s = seeded_kmer(world, g, lo=n + 20)
    head = world.gene_piece(g, s + 7 - n, n)
    tail = world.gene_piece(g, s + 7, 100)
    return head, tail, s


def expansion_cases(world: World) -> list[Case]:
    out = []
    head, tail, _ = split_kmer(world)
    # padding behind a contig, tail padding, an N run: all code 0, and poly-A is in the index
    with_n = world.gene_piece(11, 40, 500)
    with_n[200 : 200 + K + W + 20] = N
    short = world.gene_piece(12, 30, 70)  # 70 bases in a slot of 96: 26 bases of padding, then the next contig
    a0 = asm_of("rejects", [short, with_n, head, tail, world.gene_piece(13, 10, 130)])  # (130 bases: the assembly ends in padding)
    pa = a0.packed()
    marks = dict(padding=(int(pa.ctg_start[0]) + 70, int(pa.ctg_start[1])), n_run=(int(pa.ctg_start[1]) + 200, int(pa.ctg_start[1]) + 200 + K + W + 20),
                 split_at=int(pa.ctg_start[3]) - 7, tail_padding=(int(pa.ctg_start[4]) + 130, pa.padded_len))
    # the same 15-mer split across two assemblies
    a1, a2 = asm_of("split_head", [world.gene_piece(14, 0, 64), head]), asm_of("split_tail", [tail])
    marks["split_asm_at"] = pa.padded_len + a1.packed().padded_len - 7
    out.append(Case("e_rejects", [a0, a1, a2], marks))
    # empty assemblies: one between two others, one as the batch's last entry
    out.append(Case("e_empty", [asm_of("first", [world.gene_piece(15, 0, 300)]), asm_of("empty_mid", []), asm_of("third", [revcomp(world.gene_piece(16, 0, 300))]), asm_of("empty_last", [])], {}))
    # every gene piece once as it is and once reverse-complemented
    pieces = [world.gene_piece(g, 20, 260) for g in range(17, 29)]
    out.append(Case("e_strands", [asm_of("strands", [x for p in pieces for x in (p, revcomp(p))])], dict(n_pieces=len(pieces))))
    # a seed shared by a whole gene family next to seeds with one posting
    fam = np.concatenate([world.material(200, 31), world.block, world.material(200, 977)])
    out.append(Case("e_family", [asm_of("family", [fam, revcomp(fam), world.gene_piece(29, 0, 400)])], {}))
    # waves of 64 candidates with one survivor (a gene seed between N-run candidates) and with 64 (gene material only);
    # n_front not a multiple of 64 is asserted of this batch by the model
    n_heavy = world.material(4000, 2222)
    for at in range(100, 3900, 240):  # clean stretches of 40 bases (six interior positions) between N runs of 200
        n_heavy[at : at + 200] = N
    out.append(Case("e_survivors", [asm_of("survivors", [n_heavy, world.material(6000, 4444)])], {}))
    return out


# ---- f. flanks, enumerated ----------------------------------------------------------------------------------------------------------
FLANK_LENGTHS = range(1, 91)


def flank_cases(world: World) -> list[Case]:
    """A clean stretch of every length 1..90 with a contig end or an N run on either side, starting at padded offsets 0 and 32
    mod 64; and the further flank shapes.  Stretches are cut from genes at one of their seeds, so that short ones hold anchors."""
    out = []
    g_pool = list(range(30, 60))
    contigs, marks = [], []
    k = 0
    for n in FLANK_LENGTHS:
        for left_n in (False, True):
            for right_n in (False, True):
                for odd_slot in (False, True):
                    g = g_pool[k % len(g_pool)]
                    s = seeded_kmer(world, g, lo=60, nth=k % 2)
                    body = world.gene_piece(g, s - min(n - 1, 20) if n > K else s, n)
                    run = 3 if k % 3 else 12
                    parts = ([poly("N", run)] if left_n else []) + [body] + ([poly("N", 2 if k % 2 else 11)] if right_n else [])
                    if left_n:  # (the stretch before the run: the one under test starts 64 bases into its contig)
                        parts = [world.gene_piece(g, 0, UNIT - run)] + parts
                    if right_n:
                        parts = parts + [world.gene_piece(g, 100, 40)]
                    contigs.append((np.concatenate(parts), odd_slot))
                    marks.append((n, left_n, right_n, odd_slot))
                    k += 1
    # lay them out so that a contig starts at 0 or 32 mod 64 as asked: a one-base contig shifts the next slot by 32
    per = 360
    asms = []
    for i in range(0, len(contigs), per):
        laid, at = [], 0
        for c, odd in contigs[i : i + per]:
            if (at % UNIT == C["KP_CONTIG_ALIGN"]) != odd:
                laid.append(dna("A"))
                at += C["KP_CONTIG_ALIGN"]
            laid.append(c)
            at += _slot(len(c))
        asms.append(asm_of(f"flanks{len(asms)}", laid))
    out.append(Case("f_flank_lengths", asms, dict(grid=marks)))
    # further shapes
    shapes = {}
    c = world.gene_piece(60, 10, 300); c[:5] = N; shapes["n_at_first_base"] = c  # noqa: E702
    c = world.gene_piece(61, 10, 300); c[-7:] = N; shapes["n_at_last_base"] = c  # noqa: E702
    c = world.gene_piece(62, 10, 300); c[120:125] = N; c[126:140] = N; shapes["n_runs_one_apart"] = c  # noqa: E702
    for i, run in enumerate(range(1, W)):  # N runs shorter than KP_W behind a stretch: the right flank steps through them
        c = world.gene_piece(63 + i, 10, 300)
        c[150 : 150 + run] = N
        shapes[f"short_run_{run}"] = c
        c = world.gene_piece(63 + i, 10, 150 + run)  # ... and through such a run into the contig's end
        c[150:] = N
        shapes[f"short_run_{run}_to_end"] = c
    for i, unit in enumerate(("A", "AC", "ACG", "AACGT")):  # ties in either flank and across the hand-over positions
        for where in ("left", "right"):
            c = world.gene_piece(75 + i, 10, 200)
            run = periodic(unit, 2 * (K + W))
            if where == "left":
                c[: len(run)] = run
            else:
                c[-len(run) :] = run
            shapes[f"ties_{where}_{unit}"] = c
            c = world.gene_piece(75 + i, 10, 200)
            n_tie = K + 2 * W - 3  # 18 equal or periodic 15-mers: whole windows of ties
            c[W - 4 : W - 4 + n_tie] = periodic(unit, n_tie)  # on both sides of S + KP_W
            r0 = len(c) - K - W - 9
            c[r0 : r0 + n_tie] = periodic(unit, n_tie)  # ... and of E - KP_K - KP_W
            shapes[f"ties_handover_{where}_{unit}"] = c if where == "left" else revcomp(c)
    out.append(Case("f_flank_shapes", [asm_of("shapes", list(shapes.values()))], dict(names=list(shapes))))
    return out


# ---- everything, built once a process -----------------------------------------------------------------------------------------------
_BUILT: dict = {}


def built(oracle) -> dict:
    """{"world", "cases": {name: Case}, "models": {name: ScanModel}}."""
    if not _BUILT:
        world = World(oracle)
        cases = [phase_case(world), *offset_cases(world), reach_case(world), *list_stage_cases(world), *expansion_cases(world), *flank_cases(world)]
        _BUILT.update(world=world, cases={c.name: c for c in cases}, models={})
    return _BUILT


def model_of(oracle, name: str) -> ScanModel:
    b = built(oracle)
    if name not in b["models"]:
        b["models"][name] = b["world"].model(b["cases"][name].asms)
    return b["models"][name]
