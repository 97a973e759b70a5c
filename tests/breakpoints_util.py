"""Shared by tests/test_breakpoints_cpu.py and tests/test_gpu_breakpoints.py: the yardstick of the breakpoint records
(include/kp_spec.h, BREAKPOINTS) -- a Python restatement written straight from the spec that shares nothing with
kaptive_amd/csrc/kp_breakpoints.h --, a Python formatter of the table, the g++ build of kp_breakpoints.h on host arrays, a
generator of fragment tables with a target layout the overlap cull leaves alone (so that the same tables serve as kept lists on
the CPU and as hit tables on the device), the eight planted events of the miniature database and the inverted-repeat batch.
TEST INFRASTRUCTURE."""

from __future__ import annotations

import ctypes as C
from functools import lru_cache

import numpy as np

from kaptive_amd._native import BREAKPOINT_DTYPE, HIT_DTYPE
from kaptive_amd.serotyping.batch import KEPT_DTYPE

MAX_OVERLAP, IR_COLS = 64, 32
COLLINEAR, INVERTED, DISORDERED, CONTIGS = 0, 1, 2, 3
F_SPURIOUS = 16
HEADER = b"\t".join([b"Assembly", b"Gene", b"Event", b"Gene position", b"Gene gap", b"Contig A", b"Position A", b"Strand A", b"Contig B",
                     b"Position B", b"Strand B", b"Length", b"Duplication", b"Edge A", b"Edge B", b"Inverted repeat"]) + b"\n"  # fmt: skip
EVENTS = (b"insertion", b"deletion", b"replacement", b"overlap", b"inversion", b"rearrangement", b"contig_break", b"translocation")


# ---- the restatement -------------------------------------------------------------------------------------------------------------------
def _pair(a, b, len_a: int, len_b: int):
    """(key without the index, record fields without the inverted repeat) of the fragment pair (a, b), or None."""
    if not (a["q_start"] < b["q_start"] and a["q_end"] < b["q_end"]):
        return None
    if int(a["q_end"]) - int(b["q_start"]) > MAX_OVERLAP:
        return None
    sa, sb = (1 if a["strand"] >= 0 else -1), (1 if b["strand"] >= 0 else -1)
    q_gap = int(b["q_start"]) - int(a["q_end"])
    pos_a = int(a["t_end"]) - 1 if sa > 0 else int(a["t_start"])
    pos_b = int(b["t_start"]) if sb > 0 else int(b["t_end"]) - 1
    edge_a = len_a - int(a["t_end"]) if sa > 0 else int(a["t_start"])
    edge_b = int(b["t_start"]) if sb > 0 else len_b - int(b["t_end"])
    if a["contig"] != b["contig"]:
        return (2, edge_a + edge_b), dict(kind=CONTIGS, q_gap=q_gap, t_gap=0, t_lo=0, edge_a=edge_a, edge_b=edge_b)
    if sa != sb:
        return (1, abs(pos_a - pos_b)), dict(kind=INVERTED, q_gap=q_gap, t_gap=0, t_lo=0, edge_a=edge_a, edge_b=edge_b)
    t_gap = int(b["t_start"]) - int(a["t_end"]) if sa > 0 else int(a["t_start"]) - int(b["t_end"])
    if t_gap >= -MAX_OVERLAP:
        t_lo = (int(a["t_end"]) if sa > 0 else int(b["t_end"])) if t_gap > 0 else 0
        return (0, t_gap + MAX_OVERLAP), dict(kind=COLLINEAR, q_gap=q_gap, t_gap=t_gap, t_lo=t_lo, edge_a=edge_a, edge_b=edge_b)
    return (1, abs(pos_a - pos_b)), dict(kind=DISORDERED, q_gap=q_gap, t_gap=0, t_lo=0, edge_a=edge_a, edge_b=edge_b)


def restate(kept, ctg_start, ctg_len, asm_codes) -> np.ndarray:
    """The records of one kept list: ``kept`` its records (KEPT_DTYPE, list order), ``ctg_start`` / ``ctg_len`` the assembly's
    contigs in its padded space and ``asm_codes`` the codes of that space (0..3, 4 inside an N run)."""
    alive = [i for i in range(len(kept)) if not int(kept["flags"][i]) & F_SPURIOUS]
    by_gene: dict = {}
    for i in alive:
        by_gene.setdefault(int(kept["gene"][i]), []).append(i)
    out = []
    for ib in alive:
        b = kept[ib]
        best = None
        for ia in by_gene[int(b["gene"])]:
            if ia == ib:
                continue
            a = kept[ia]
            p = _pair(a, b, int(ctg_len[a["contig"]]), int(ctg_len[b["contig"]]))
            if p is not None and (best is None or (*p[0], ia) < best[0]):
                best = ((*p[0], ia), p[1])
        if best is None:
            continue
        r = best[1]
        cols = matches = 0
        if r["kind"] == COLLINEAR and r["t_gap"] >= 2:
            lo = int(ctg_start[b["contig"]]) + r["t_lo"]
            s = asm_codes[lo : lo + r["t_gap"]]
            cols = min(IR_COLS, r["t_gap"] // 2)
            matches = sum(1 for i in range(cols) if s[i] <= 3 and s[len(s) - 1 - i] <= 3 and int(s[i]) == 3 - int(s[len(s) - 1 - i]))
        out.append((best[0][2], ib, r["q_gap"], r["t_gap"], r["t_lo"], r["edge_a"], r["edge_b"], r["kind"], cols, matches, 0))
    return np.array(out, BREAKPOINT_DTYPE) if out else np.zeros(0, BREAKPOINT_DTYPE)


def event(r, edge_tolerance: int) -> bytes:
    if r["kind"] == COLLINEAR:
        if r["t_gap"] > 0:
            return b"replacement" if r["q_gap"] > 0 else b"insertion"
        return b"deletion" if r["q_gap"] > 0 else b"overlap"
    if r["kind"] == INVERTED:
        return b"inversion"
    if r["kind"] == DISORDERED:
        return b"rearrangement"
    return b"contig_break" if r["edge_a"] <= edge_tolerance and r["edge_b"] <= edge_tolerance else b"translocation"


def format_tsv(asm_names, contig_names, gene_names, kept, records, bp_off, edge_tolerance: int) -> bytes:
    """The lines of the breakpoint table (no header): ``contig_names[a]`` are assembly a's, ``kept[a]`` its kept records."""
    lines = []
    for i, name in enumerate(asm_names):
        for r in records[bp_off[i] : bp_off[i + 1]]:
            a, b = kept[i][int(r["kept_a"])], kept[i][int(r["kept_b"])]
            fa, fb = a["strand"] >= 0, b["strand"] >= 0
            pos_a = int(a["t_end"]) - 1 if fa else int(a["t_start"])
            pos_b = int(b["t_start"]) if fb else int(b["t_end"]) - 1
            cols = [str(name).encode(), str(gene_names[int(a["gene"])]).encode(), event(r, edge_tolerance), b"%d" % int(a["q_end"]), b"%d" % int(r["q_gap"]),
                    str(contig_names[i][int(a["contig"])]).encode(), b"%d" % (pos_a + 1), b"+" if fa else b"-",
                    str(contig_names[i][int(b["contig"])]).encode(), b"%d" % (pos_b + 1), b"+" if fb else b"-",
                    b"%d" % int(r["t_gap"]) if r["kind"] == COLLINEAR else b".", b"%d" % max(0, -int(r["q_gap"])), b"%d" % int(r["edge_a"]),
                    b"%d" % int(r["edge_b"]), b"%d/%d" % (int(r["ir_matches"]), int(r["ir_cols"])) if r["ir_cols"] else b"."]  # fmt: skip
            lines.append(b"\t".join(cols) + b"\n")
    return b"".join(lines)


# ---- kp_breakpoints.h on host arrays (tests/native_harness/breakpoints_harness.cpp) ---------------------------------------------------
@lru_cache(maxsize=1)
def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    lib = build_harness("breakpoints_harness", "kp_breakpoints.h")
    lib.kpy_breakpoints.restype = C.c_int64
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


GUARD = 0x7E


def harness_records(kept, pa, tile: int = 1 << 20):
    """(records, guard intact): the header's records of one kept list on the packed assembly ``pa``, the candidates offered in tiles of
    ``tile``; the buffer holds one record per kept record, then guard records."""
    kept = np.ascontiguousarray(kept, KEPT_DTYPE)
    words, runs = np.ascontiguousarray(pa.words, np.uint32), np.ascontiguousarray(pa.n_runs, np.int32).reshape(-1)
    cs, cl = np.ascontiguousarray(pa.ctg_start, np.int32), np.ascontiguousarray(pa.ctg_len, np.int32)
    buf = np.frombuffer(bytes([GUARD]) * ((len(kept) + 4) * BREAKPOINT_DTYPE.itemsize), BREAKPOINT_DTYPE).copy()
    n = harness().kpy_breakpoints(_p(kept), C.c_int(len(kept)), C.c_int(len(cs)), _p(cs), _p(cl), _p(words), C.c_int(len(words)), _p(runs),
                                  C.c_int(len(runs) // 2), C.c_int(int(tile)), _p(buf))  # fmt: skip
    assert 0 <= n <= len(kept)
    return buf[:n].copy(), bool((buf[len(kept) :].view(np.uint8) == GUARD).all())


# ---- fragment tables ---------------------------------------------------------------------------------------------------------------------
class Layout:
    """Fragments of genes laid out on contigs so that no two target ranges overlap by more than a tenth of the shorter one -- the
    overlap cull keeps them all --, built scenario by scenario: collinear pairs at chosen target and gene gaps, full copies next to
    fragments, candidates of all three ranks for one b, equal keys, random fragments.  ``frag``: target length of an ordinary fragment
    (one whose target overlaps its partner is 700 long: 65 bases are less than a tenth of it); ``long_pairs``: how many of those the
    table may hold; ``duplicates``: exact copies of a record may be added (a kept list the cull would not leave: CPU only)."""

    T_GAPS_SHORT = (0, 0, 1, 2, 3, 3, 5, 63, 64, 65)
    T_GAPS_LONG = (-65, -64, -63, -1)
    Q_OVERLAPS = (0, 0, 9, 63, 64, 65, 66, -1, -600)

    def __init__(self, rng, gene_lens, frag=300, contig_len=3000, long_pairs=8, duplicates=False, far_gaps=True):
        self.rng, self.gene_lens, self.frag, self.contig_len = rng, [int(x) for x in gene_lens], int(frag), int(contig_len)
        self.long_pairs, self.duplicates, self.far_gaps = long_pairs, duplicates, far_gaps
        self.contigs: list = []  # lengths
        self.frags: list = []  # (gene, contig, strand, q_start, q_end, t_start, t_end)
        self.cur, self.pos, self.n_genes_used = None, 0, 0
        self.classes: dict = {}

    # -- room on the contigs
    def contig(self, length: int) -> int:
        self.contigs.append(int(length))
        return len(self.contigs) - 1

    def room(self, span: int):
        if self.cur is None or self.pos + span > self.contigs[self.cur]:
            self.cur, self.pos = self.contig(max(self.contig_len, span)), 0
        c, s = self.cur, self.pos
        self.pos += span + int(self.rng.integers(0, 3))
        return c, s

    def gene(self) -> int:
        g = self.n_genes_used % len(self.gene_lens)
        self.n_genes_used += 1
        return g

    def add(self, gene, contig, strand, q_start, q_end, t_start, length):
        n = self.gene_lens[gene]
        q_start, q_end = max(0, min(int(q_start), n - 2)), max(2, min(int(q_end), n))
        self.frags.append((gene, contig, strand, q_start, max(q_end, q_start + 1), int(t_start), int(t_start) + int(length)))

    def note(self, name):
        self.classes[name] = self.classes.get(name, 0) + 1

    # -- scenarios
    def collinear(self, g=None, t_gap=None, overlap=None, strand=None):
        rng = self.rng
        g = self.gene() if g is None else g
        strand = int(rng.choice([1, -1])) if strand is None else strand
        if t_gap is None:
            pick = rng.random()
            if pick < 0.12 and self.long_pairs > 0:
                t_gap = int(rng.choice(self.T_GAPS_LONG))
            elif pick < 0.2 and self.far_gaps:
                t_gap = int(rng.choice([700, 1200]))
            else:
                t_gap = int(rng.choice(self.T_GAPS_SHORT))
        length = self.frag
        if t_gap < 0:
            self.long_pairs -= 1
            length = max(length, 700)
        overlap = int(rng.choice(self.Q_OVERLAPS)) if overlap is None else overlap
        c, s = self.room(2 * length + t_gap)
        x = int(rng.integers(100, 300))
        first, second = (s, s + length + t_gap)
        ta, tb = (first, second) if strand > 0 else (second, first)
        self.add(g, c, strand, int(rng.choice([0, 5])), x, ta, length)
        self.add(g, c, strand, x - overlap, self.gene_lens[g] - int(rng.choice([0, 7])), tb, length)
        self.note(f"t_gap {t_gap}" if t_gap in (-65, -64) else "collinear")
        self.note(f"q overlap {overlap}" if overlap in (64, 65) else "pair")

    def full_copies(self):
        g = self.gene()
        for _ in range(2):
            c, s = self.room(self.frag)
            self.add(g, c, int(self.rng.choice([1, -1])), 0, self.gene_lens[g], s, self.frag)
        if self.rng.random() < 0.6:
            self.collinear(g)
        self.note("full copies")

    def three_ranks(self):
        """b with a collinear, an inverted (or disordered) and an other-contig candidate; the better ones are left out at random."""
        rng, g, L = self.rng, self.gene(), self.frag
        c, s = self.room(3 * L + 10)
        keep0, keep1 = rng.random() < 0.6, rng.random() < 0.7
        x = int(rng.integers(100, 300))
        if keep0:
            self.add(g, c, 1, 0, x, s, L)  # collinear: ends 4 bases before b
        self.add(g, c, 1, x, self.gene_lens[g], s + L + 4, L)  # b
        if keep1:
            if rng.random() < 0.5:
                self.add(g, c, -1, 3, x + 2, s + 2 * L + 8, L)  # inverted
            else:
                self.add(g, c, 1, 3, x + 2, s + 2 * L + 8, L)  # same strand behind b: disordered
        other = self.contig(L + 20)
        self.add(g, other, int(rng.choice([1, -1])), 1, x + 1, int(rng.integers(0, 20)), L)
        self.note("three ranks" if keep0 and keep1 else ("rank 1 wins" if keep1 else ("rank 0 wins" if keep0 else "rank 2 wins")))

    def equal_keys(self):
        rng, g, L = self.rng, self.gene(), self.frag
        x = int(rng.integers(100, 300))
        if rng.random() < 0.5:  # two candidates on contigs of their own, as far from the ends they face
            e = int(rng.integers(0, 9))
            for _ in range(2):
                self.add(g, self.contig(L + e + 3), -1, 0, x, e, L)
            c, s = self.room(L)
            self.add(g, c, 1, x, self.gene_lens[g], s, L)
        else:  # two inverted candidates as far from b, one on either side
            d = int(rng.integers(0, 5))
            c, s = self.room(3 * L + 2 * d)
            self.add(g, c, -1, 0, x, s, L)
            self.add(g, c, 1, x, self.gene_lens[g], s + L + d, L)
            self.add(g, c, -1, 0, x, s + 2 * L + 2 * d, L)
        self.note("equal keys")

    def scattered(self):
        rng, g = self.rng, self.gene()
        n = self.gene_lens[g]
        for _ in range(int(rng.integers(1, 7))):
            c, s = self.room(self.frag)
            q0 = int(rng.integers(0, n - 60))
            self.add(g, c, int(rng.choice([1, -1])), q0, int(rng.integers(q0 + 30, n + 1)), s, self.frag)
        self.note("scattered")

    def fill(self, n: int):
        """Scenarios until the table holds ``n`` fragments (the last one may be cut short)."""
        kinds = (self.collinear, self.collinear, self.collinear, self.full_copies, self.three_ranks, self.equal_keys, self.scattered)
        if n >= 16:  # the limits of the pair rule and of the collinear kind, on both sides: in every table that has room for them
            for t_gap, overlap in ((-64, 0), (-65, 0), (3, 64), (3, 65)):
                self.collinear(t_gap=t_gap, overlap=overlap)
        while len(self.frags) < n:
            kinds[int(self.rng.integers(0, len(kinds)))]()
            if self.duplicates and self.rng.random() < 0.1:
                self.frags.append(self.frags[int(self.rng.integers(0, len(self.frags)))])
                self.note("duplicate")
        del self.frags[n:]
        if not self.contigs:
            self.contig(self.contig_len)
        return self

    # -- what the tables are made into
    def sequences(self, n_rate=0.002) -> list:
        """Random contigs (ASCII) with a sprinkle of short N runs."""
        out = []
        for n in self.contigs:
            seq = np.frombuffer(b"ACGT", np.uint8)[self.rng.integers(0, 4, size=n)].copy()
            for at in np.flatnonzero(self.rng.random(n) < n_rate):
                seq[at : at + int(self.rng.integers(1, 4))] = ord("N")
            out.append(seq)
        return out

    def genome(self, name: str):
        from kaptive_amd.core.genome import GenomeAssembly
        from kaptive_amd.core.seq import SeqRecord, Sequences

        return GenomeAssembly(name, Sequences.from_records([SeqRecord(f"{name}_c{i}", s.tobytes()) for i, s in enumerate(self.sequences())]))

    def kept(self, spurious=0.15, shuffle=True) -> np.ndarray:
        """The fragments as a kept list in any order, a share of them spurious, the fields no pair reads filled with noise."""
        k = np.zeros(len(self.frags), KEPT_DTYPE)
        for i, (g, c, st, q0, q1, t0, t1) in enumerate(self.frags):
            k[i]["gene"], k[i]["contig"], k[i]["strand"], k[i]["q_start"], k[i]["q_end"], k[i]["t_start"], k[i]["t_end"] = g, c, st, q0, q1, t0, t1
        k["flags"] = self.rng.integers(0, 16, size=len(k)) | np.where(self.rng.random(len(k)) < spurious, F_SPURIOUS, 0) | 32 * self.rng.integers(0, 2, size=len(k))
        k["score"], k["state"] = self.rng.integers(1, 3000, size=len(k)), self.rng.integers(0, 4, size=len(k))
        return k[self.rng.permutation(len(k))] if shuffle else k

    def hits(self) -> np.ndarray:
        """The fragments as a hit table: sorted by gene (the reduction's scoring expects that), a gene's hits in random order."""
        h = np.zeros(len(self.frags), HIT_DTYPE)
        for i, (g, c, st, q0, q1, t0, t1) in enumerate(self.frags):
            h[i]["gene"], h[i]["contig"], h[i]["strand"], h[i]["q_start"], h[i]["q_end"], h[i]["t_start"], h[i]["t_end"] = g, c, st, q0, q1, t0, t1
        span = h["t_end"] - h["t_start"]
        h["score"], h["matches"], h["block_len"], h["mapq"] = 2 * span - self.rng.integers(0, 20, size=len(h)), span, span, 60
        return h[np.lexsort((self.rng.random(len(h)), h["gene"]))]


# ---- the planted events of the miniature database ----------------------------------------------------------------------------------------
PLANT_LOCUS, FLANK = 2, 20_000


def plant_db():
    from kaptive_amd.synth import make_db

    return make_db("kpsc_k", seed=7, n_loci=9)


def locus_with_insertion(db, li: int, gi: int, at: int, size: int, dup: int, rng) -> np.ndarray:
    """Locus ``li`` with ``size`` random bases behind base ``at`` of its gene ``gi`` (database index; on the locus's forward strand),
    the ``dup`` gene bases before them repeated behind them.  Their first and last eight bases are chosen so that neither fragment
    can run on into them, straight or across a one-base gap: each differs from the gene base it would face and from that base's
    two neighbours.  (An end may still extend by a chance base of the duplication's surroundings; t_gap - q_gap does not change
    with that.)"""
    from kaptive_amd.synth import random_dna

    o, n = int(db.loci.offsets[li]), int(db.loci.lengths[li])
    locus = np.asarray(db.loci.seqs[o : o + n], np.uint8)
    assert db.gene_intervals.strands[gi] > 0
    s = int(db.gene_intervals.starts[gi])
    ins = random_dna(rng, size, 0.5)
    for i in range(8):
        for at_ins, faces in ((i, s + at + i), (size - 1 - i, s + at - dup - 1 - i)):
            ins[at_ins] = next(c for c in b"ACGT" if c not in set(locus[faces - 1 : faces + 2].tolist()))
    return np.concatenate([locus[: s + at], ins, locus[s + at - dup : s + at], locus[s + at :]])


def plants(db, flank_len: int = FLANK):
    """[(name, genome, gene index in the database, expectation)]: one assembly per event, each the locus of ``PLANT_LOCUS`` between
    20 kb (``flank_len``) of random flank with ONE gene edited.  Expectation: kind, event and what the gaps must add up to."""
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import random_dna, revcomp

    o, n = int(db.loci.offsets[PLANT_LOCUS]), int(db.loci.lengths[PLANT_LOCUS])
    locus = np.asarray(db.loci.seqs[o : o + n], np.uint8)
    g0 = int(db.locus_gene_offsets[PLANT_LOCUS])
    rng = np.random.default_rng(20261018)

    def gene(k):
        gi = g0 + k
        assert db.gene_intervals.strands[gi] > 0, "the planted genes lie on the locus's forward strand"
        return gi, int(db.gene_intervals.starts[gi]), int(db.gene_intervals.ends[gi])

    def asm(name, *contigs):
        return GenomeAssembly(name, Sequences.from_records([SeqRecord(f"{name}_{i}", np.ascontiguousarray(c).tobytes()) for i, c in enumerate(contigs)]))

    def flank():
        return random_dna(rng, flank_len, 0.5)

    def insertion(k, at, size, dup):
        return gene(k)[0], locus_with_insertion(db, PLANT_LOCUS, g0 + k, at, size, dup, rng)

    out = []
    gi, copy = insertion(1, 400, 1200, 9)
    out.append(("ins1200_dup9", asm("ins1200_dup9", np.concatenate([flank(), copy, flank()])), gi, dict(kind=COLLINEAR, event=b"insertion", gaps=1209)))
    gi, copy = insertion(2, 300, 1500, 0)
    out.append(("ins1500", asm("ins1500", np.concatenate([flank(), copy, flank()])), gi, dict(kind=COLLINEAR, event=b"insertion", gaps=1500)))
    gi, copy = insertion(3, 500, 800, 5)
    out.append(("ins800_dup5_rc", asm("ins800_dup5_rc", np.concatenate([flank(), revcomp(copy), flank()])), gi, dict(kind=COLLINEAR, event=b"insertion", gaps=805)))
    gi, s, e = gene(1)
    copy = np.concatenate([locus[: s + 300], locus[s + 900 :]])
    out.append(("del600", asm("del600", np.concatenate([flank(), copy, flank()])), gi, dict(kind=COLLINEAR, event=b"deletion", q_gap=600, t_gap=0)))
    out.append(("contig_cut", asm("contig_cut", np.concatenate([flank(), locus[: s + 500]]), np.concatenate([locus[s + 500 :], flank()])), gi,
                dict(kind=CONTIGS, event=b"contig_break", edges=0)))  # fmt: skip
    out.append(("contig_cut_dup9_rc", asm("contig_cut_dup9_rc", np.concatenate([flank(), locus[: s + 509]]), revcomp(np.concatenate([locus[s + 500 :], flank()]))), gi,
                dict(kind=CONTIGS, event=b"contig_break", edges=0)))  # fmt: skip
    copy = np.concatenate([locus[: s + 700], revcomp(locus[s + 700 : e]), locus[e:]])
    out.append(("tail_inverted", asm("tail_inverted", np.concatenate([flank(), copy, flank()])), gi, dict(kind=INVERTED, event=b"inversion")))
    gi, copy = insertion(1, 70, 1200, 0)
    out.append(("ins1200_at70", asm("ins1200_at70", np.concatenate([flank(), copy, flank()])), gi, dict(kind=COLLINEAR, event=b"insertion", gaps=1200)))
    return out


def check_plant(name, gene_index, expect, kept, records, edge_tolerance):
    """The records of a planted assembly: exactly one, for the edited gene, of the kind and event the plant implies."""
    assert len(records) == 1, f"{name}: {len(records)} records {records}"
    r = records[0]
    a, b = kept[int(r["kept_a"])], kept[int(r["kept_b"])]
    assert a["gene"] == b["gene"] == gene_index, f"{name}: record of gene {a['gene']}, edited {gene_index}"
    assert r["kind"] == expect["kind"] and event(r, edge_tolerance) == expect["event"], f"{name}: {r} is {event(r, edge_tolerance)}"
    if "gaps" in expect:  # an end may extend by a chance base: the sum is exact, the parts are not
        assert int(r["t_gap"]) - int(r["q_gap"]) == expect["gaps"], f"{name}: t_gap {r['t_gap']} - q_gap {r['q_gap']}"
    if "q_gap" in expect:
        assert r["q_gap"] == expect["q_gap"] and r["t_gap"] == expect["t_gap"], f"{name}: {r}"
    if "edges" in expect:
        assert r["edge_a"] == r["edge_b"] == expect["edges"], f"{name}: {r}"


# ---- the inverted-repeat batch -----------------------------------------------------------------------------------------------------------
IR_T_GAPS = (1, 2, 3, 63, 64, 65)
TIR = 20


def inverted_repeat_assembly(db, name="ir"):
    """(genome, hits, cases): one gene per case, cut after base 300 into two hand-made hits of 250 bases with an element between them.
    Cases: an element of 600 bases with a perfect 20-base terminal inverted repeat placed so that S starts at each of the 16 offsets
    inside a packed word (a contig starts on a word edge), on both strands; the same with an N in one repeat column; random elements
    of 1, 2, 3, 63, 64 and 65 bases on both strands.  cases[gene] = (label, strand, element length)."""
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import random_dna, revcomp

    rng = np.random.default_rng(20261019)
    L = 250
    element = random_dna(rng, 600, 0.5)
    element[-TIR:] = revcomp(element[:TIR])
    with_n = element.copy()
    with_n[7] = ord("N")
    todo = [("tir", strand, element, k) for strand in (1, -1) for k in range(16)]
    todo += [("tir with N", strand, with_n, 5) for strand in (1, -1)]
    todo += [(f"gap {n}", strand, random_dna(rng, n, 0.5), int(rng.integers(0, 16))) for n in IR_T_GAPS for strand in (1, -1)]
    contigs, hits, cases = [], [], {}
    for g, (label, strand, el, k) in enumerate(todo):
        assert db.genes.lengths[g] >= 600
        # S starts at contig base lead + L on strand +1, at tail + L on strand -1 (the contig is read from its other end: b comes
        # first on it): k bases more on that side put it at every offset of a packed word once over k (a contig starts on a word edge)
        lead, tail = 208 + (k if strand > 0 else 0), 40 + (k if strand < 0 else 0)
        fwd = np.concatenate([random_dna(rng, lead, 0.5), random_dna(rng, L, 0.5), el, random_dna(rng, L, 0.5), random_dna(rng, tail, 0.5)])
        ta, tb = lead, lead + L + len(el)
        if strand < 0:
            n = len(fwd)
            fwd, ta, tb = revcomp(fwd), n - (ta + L), n - (tb + L)
        contigs.append(fwd)
        for q0, q1, t0 in ((0, 300, ta), (300, int(db.genes.lengths[g]), tb)):
            h = np.zeros(1, HIT_DTYPE)[0]
            h["gene"], h["contig"], h["strand"], h["q_start"], h["q_end"], h["t_start"], h["t_end"] = g, g, strand, q0, q1, t0, t0 + L
            h["score"], h["matches"], h["block_len"], h["mapq"] = 2 * L, L, L, 60
            hits.append(h)
        cases[g] = (label, strand, len(el))
    genome = GenomeAssembly(name, Sequences.from_records([SeqRecord(f"{name}_c{i}", np.ascontiguousarray(c).tobytes()) for i, c in enumerate(contigs)]))
    return genome, np.array(hits, HIT_DTYPE), cases
