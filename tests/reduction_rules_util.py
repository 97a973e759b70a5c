"""Hit tables that put a hit on every rule and round edge of the typing reduction (csrc/kp_reduce.hip: kp_score_kernel,
kp_reduce_kernel, kp_state_kernel, and the functions of kp_reduce_core.h they call), and the "rules assembly" they refer to.
Shared by oracle/make_golden.py::gen_typing_rules (every case through the reference's Serotyper ->
tests/golden/typing_rules_<key>.npz), tests/test_reduction_rules_cpu.py (the cases are what their labels say; the core
header equals the reference on them) and tests/test_gpu_reduction_rules.py (so does the device).  TEST INFRASTRUCTURE:
pure numpy, nothing of the reference is imported here.

THE RULES ASSEMBLY (one per golden database, `rules_assembly(key)`): contigs whose text is planted on purpose, because the
translation and the gene states read the contig text and nothing else --
  locus      every gene of locus 0, exact, forward, in order
  variants   copies of S (a gene of locus 0 with 40 n residues, so that the identity threshold 82.5 = 33 / 40 is reachable):
             exact, reverse complement, a stop at codon 0 / 1 / either side of 3 * prot_len / gene_len = 0.90, two stops, no stop,
             an N in each codon position, an N run across two codon edges, N in a stop codon, and substituted codons that put
             the identity on the threshold and one residue either side
  foreign    the same three substituted copies of F (a gene of another locus with 40 n residues) and copies of C (a gene whose
             length is a multiple of 30) with a stop exactly at 0.90 and a codon either side: outside every locus piece
  e<f>[r|s]  S (r: reverse complement, s: with the stop at codon 1) with f = edge_tolerance or edge_tolerance + 1 bases of flank
  short      the first 100 bases of S: a contig shorter than the gene
  many       129 copies of S with 0 to 34 substituted codons each (all above the identity threshold): the long identity lists
  pad        random text, max_locus_length + 6000 bases, for tables whose hits are spans and nothing more
A hit table need not be what an aligner would emit: it is rows of HIT_DTYPE, gene ascending (Batch.set_hits).

THE FRAME.  A hit that lies outside every locus piece on random text is spurious and leaves no trace in the reference's result.
So the span-only tables (cull, rounds, residency) carry two full-length hits L and R of two genes of locus 0 at either end of
the pad region, with the top scores: they make locus 0 the best locus, are its primary hits, share a cluster with everything
between them (the tolerance is the whole region) and so span one piece that every other hit of the table lies inside.  They
are visit positions 0 and 1 of the cull."""

from __future__ import annotations

import inspect
import re
from dataclasses import dataclass, field
from functools import lru_cache
from pathlib import Path

import numpy as np

from kaptive_amd import _native
from kaptive_amd.core.genome import GenomeAssembly
from kaptive_amd.core.seq import Sequences
from kaptive_amd.serotyping.core import Serotyper
from kaptive_amd.synth import random_dna, revcomp
from tests.golden_util import load_db

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kaptive_amd" / "csrc"
HIT_DTYPE = _native.HIT_DTYPE
GROUPS = ("scores", "cull", "rounds", "clusters", "resident", "translation", "states")


# ---- the constants the cases hang on, read out of the sources -------------------------------------------------------------------------
def kernel_constants() -> dict[str, int]:
    red, spec = (CSRC / "kp_reduce.hip").read_text(), (ROOT / "include" / "kp_spec.h").read_text()
    out = {}
    for name in ("KEPT_LDS", "SORT_LDS"):
        out[name] = int(re.search(rf"constexpr int {name} = (\d+);", red).group(1))
    out["LANES"] = int(re.search(r"__launch_bounds__\((\d+)\) void kp_reduce_kernel", red).group(1))
    out["TR"] = int(re.search(r"constexpr int TR = (\d+);", red).group(1))
    out["PIECE_TMP"] = int(re.search(r"piece_tmp = in_lds && piece_cap <= (\d+) \?", red).group(1))
    assert re.search(r"in_lds = \(size_t\)nk \* sizeof\(KpKept\) <= 3 \* \(size_t\)KEPT_LDS \* sizeof\(int32_t\);", red)
    out["KP_MAX_LOCUS_GENES"] = int(re.search(r"#define KP_MAX_LOCUS_GENES (\d+)", spec).group(1))
    body = re.search(r"typedef struct kp_kept \{(.*?)\} kp_kept;", spec, re.S).group(1)
    size = 0
    for typ, names in re.findall(r"^\s*(int32_t|float|int8_t|uint8_t) ([^;]+);", body, re.M):
        for nm in names.split(","):
            m = re.search(r"\[(\d+)\]", nm)
            size += {"int32_t": 4, "float": 4, "int8_t": 1, "uint8_t": 1}[typ] * (int(m.group(1)) if m else 1)
    out["SIZEOF_KEPT"] = size
    return out


C = kernel_constants()
LANES, TR, PIECE_TMP = C["LANES"], C["TR"], C["PIECE_TMP"]
KEPT_IN_LDS = 3 * C["KEPT_LDS"] * 4 // C["SIZEOF_KEPT"]  # the most kept records the clustering holds in LDS
CODON_ROUND = LANES * TR
_TYPER_DEFAULTS = inspect.signature(Serotyper.__init__).parameters
EDGE_TOL = int(_TYPER_DEFAULTS["partial_edge_tolerance"].default)  # what a Serotyper made without keywords uses
MIN_COV = float(_TYPER_DEFAULTS["min_gene_coverage"].default)
STOP, SENSE = b"TAA", b"GCT"
MANY = 129  # copies of S for the identity lists: one past numpy's pairwise block of 128


# ---- the rules assembly ---------------------------------------------------------------------------------------------------------------
@dataclass
class Rules:
    key: str
    genome: GenomeAssembly
    contig: dict[str, int]  # contig name -> index
    at: dict[str, tuple[int, int, int, int]]  # planted copy -> (contig, start, end, gene)
    S: int
    F: int
    Cg: int
    g0: int
    n0: int  # locus 0: first gene, number of genes
    cstop: dict[str, int] = field(default_factory=dict)  # variant -> codon of its first stop


def _gene(db, g) -> np.ndarray:
    o, n = int(db.genes.offsets[g]), int(db.genes.lengths[g])
    return np.array(db.genes.seqs[o : o + n], np.uint8)


def _with_codon(seq, c, codon: bytes) -> np.ndarray:
    s = seq.copy()
    s[3 * c : 3 * c + 3] = np.frombuffer(codon, np.uint8)
    return s


def _substituted(seq, n_sub) -> np.ndarray:
    """`n_sub` codons, spread evenly and never neighbours or near an end, replaced by a codon of another amino acid (GCT, Ala; GGT,
    Gly, where the codon was one of Ala's, GC?)."""
    s = seq.copy()
    n_res = len(seq) // 3 - 1
    for c in np.linspace(8, n_res - 8, n_sub).astype(int):
        old = bytes(s[3 * c : 3 * c + 3])
        s[3 * c : 3 * c + 3] = np.frombuffer(b"GGT" if old[:2] == b"GC" else b"GCT", np.uint8)
    return s


@lru_cache(maxsize=None)
def rules_assembly(key: str) -> Rules:
    db = load_db(key)
    rng = np.random.default_rng({"k": 7101, "o": 7102}[key])
    L, loc = db.genes.lengths, db.gene_locus_indices
    g0, n0 = int(db.locus_gene_offsets[0]), int(db.locus_gene_lengths[0])
    res40 = np.flatnonzero((L // 3 - 1) % 40 == 0)
    S = int(next(g for g in res40 if loc[g] == 0))
    F = int(next(g for g in res40 if loc[g] != 0 and not db.extra_genes[g]))
    Cg = int(next(g for g in np.flatnonzero(L % 30 == 0) if loc[g] != 0 and not db.extra_genes[g]))
    contigs: list[tuple[str, np.ndarray]] = []
    at: dict[str, tuple[int, int, int, int]] = {}
    cstop: dict[str, int] = {}

    def fill(n):
        return random_dna(rng, n, 0.5)

    def contig(name, parts):  # parts: filler arrays and (label, gene, array) copies
        pos, chunks = 0, []
        for p in parts:
            if isinstance(p, tuple):
                at[p[0]] = (len(contigs), pos, pos + len(p[2]), p[1])
                p = p[2]
            chunks.append(p)
            pos += len(p)
        contigs.append((name, np.concatenate(chunks)))

    parts = [fill(200)]
    for g in range(g0, g0 + n0):
        parts += [(f"g{g - g0}", g, _gene(db, g)), fill(50)]
    contig("locus", parts)

    s, ls = _gene(db, S), int(L[S])
    n_cod = ls // 3  # codons of S, the stop included
    lo = (9 * ls - 1) // 30  # the last prot_len with 3 * prot_len / len < 0.90 (len is no multiple of 10 * 3)
    var = {"exact": s, "rc": revcomp(s)}
    for name, c in (("stop0", 0), ("stop1", 1), ("stop_lo", lo), ("stop_hi", lo + 1)):
        var[name], cstop[name] = _with_codon(s, c, STOP), c
    var["rc_stop_lo"], cstop["rc_stop_lo"] = revcomp(var["stop_lo"]), lo
    var["two_stops"], cstop["two_stops"] = _with_codon(_with_codon(s, 50, STOP), 120, b"TGA"), 50
    var["no_stop"] = _with_codon(s, n_cod - 1, SENSE)
    for x in range(3):
        v = s.copy()
        v[3 * 5 + x] = ord("N")
        var[f"n{x}"] = v
    v = s.copy()
    v[3 * 20 + 2 : 3 * 22 + 1] = ord("N")  # last base of codon 20, all of 21, first base of 22
    var["nrun"] = v
    v = _with_codon(s, 30, b"TAN")
    var["stop_n"] = v
    for tag, d in (("below", 1), ("at", 0), ("above", -1)):  # 33 matches in 40 residues are the threshold, 82.5 %
        var[f"id_{tag}"] = _substituted(s, 7 * (n_cod - 1) // 40 + d)
    parts = [fill(60)]
    for name, v in var.items():
        parts += [(name, S, v), fill(40)]
    contig("variants", parts)

    f, c, lc = _gene(db, F), _gene(db, Cg), int(L[Cg])
    parts = [fill(60)]
    for tag, d in (("below", 1), ("at", 0), ("above", -1)):
        parts += [(f"f_id_{tag}", F, _substituted(f, 7 * (len(f) // 3 - 1) // 40 + d)), fill(40)]
    for name, cod in (("c_lo", 3 * lc // 10 - 1), ("c_eq", 3 * lc // 10), ("c_hi", 3 * lc // 10 + 1)):
        parts += [(name, Cg, _with_codon(c, cod, STOP)), fill(40)]
        cstop[name] = cod
    contig("foreign", parts)

    for fl in (EDGE_TOL, EDGE_TOL + 1):
        contig(f"e{fl}", [fill(fl), (f"e{fl}", S, s), fill(fl)])
        contig(f"e{fl}r", [fill(fl), (f"e{fl}r", S, revcomp(s)), fill(fl)])
    contig(f"e{EDGE_TOL}s", [fill(EDGE_TOL), (f"e{EDGE_TOL}s", S, var["stop1"]), fill(EDGE_TOL)])
    contig("short", [("short", S, s[:100])])
    parts = [fill(40)]
    for i in range(MANY):
        parts += [(f"many{i}", S, _substituted(s, (11 * i) % 35)), fill(40)]
    contig("many", parts)
    contig("pad", [fill(int(db.max_locus_length) + 6000)])

    lengths = np.array([len(x[1]) for x in contigs], np.int32)
    offsets = np.zeros(len(contigs), np.int32)
    np.cumsum(lengths[:-1], out=offsets[1:])
    seqs = Sequences(tuple(x[0] for x in contigs), np.concatenate([x[1] for x in contigs]), offsets, lengths)
    return Rules(key, GenomeAssembly(f"rules_{key}", seqs), {x[0]: i for i, x in enumerate(contigs)}, at, S, F, Cg, g0, n0, cstop)


# ---- hits and cases -------------------------------------------------------------------------------------------------------------------
@dataclass
class Case:
    group: str
    name: str
    hits: np.ndarray
    kwargs: dict = field(default_factory=dict)
    pair: tuple[str, int] | None = None  # (boundary, side): the reference must answer the two sides differently
    info: dict = field(default_factory=dict)  # what the label test proves, by kind


def make_hit(gene, contig, t_start, t_end, *, strand=1, q_start=0, q_end=None, score=None, matches=None, mapq=60):
    n = t_end - t_start
    return (gene, contig, q_start, q_start + n if q_end is None else q_end, t_start, t_end, n if score is None else score,
            n if matches is None else matches, max(n, 0), strand, mapq, 0, 0)  # fmt: skip


def table(rows, manual=False) -> np.ndarray:
    """Rows -> HIT_DTYPE in emission order (kp_spec.h; kp_hit_keys).  `manual`: a gene's hits stay in the order given."""
    h = np.array(rows, HIT_DTYPE) if rows else np.zeros(0, HIT_DTYPE)
    if manual:
        return h[np.argsort(h["gene"], kind="stable")]
    return h[np.lexsort((h["block_len"], -h["matches"], h["t_end"], h["q_end"], h["q_start"], h["strand"] < 0, h["t_start"],
                         h["contig"], -h["score"], h["gene"]))]  # fmt: skip


def visit_order(hits, priority) -> np.ndarray:
    """alignment.py:669-675: lexsort of (score + 1e9 * priority) descending, matches descending, uint8(-mapq) ascending, stable."""
    s = hits["score"].astype(np.float64) + 1e9 * np.asarray(priority, np.float64)
    negq = (-hits["mapq"].astype(np.int64)).astype(np.uint8)
    return np.lexsort((negq, -hits["matches"].astype(np.int64), -s))


def cull_model(hits, order) -> np.ndarray:
    """interval.py:698-751 in exact integers and float64 side by side: kept flags in table order."""
    kept: list[int] = []
    flag = np.zeros(len(hits), bool)
    if len(hits) < 2:
        flag[:] = True
        return flag
    for i in order:
        s, e, c = int(hits["t_start"][i]), int(hits["t_end"][i]), int(hits["contig"][i])
        if e - s <= 0:
            continue
        clash = False
        for j in kept:
            if int(hits["contig"][j]) != c:
                continue
            ov = min(e, int(hits["t_end"][j])) - max(s, int(hits["t_start"][j]))
            mn = min(e - s, int(hits["t_end"][j]) - int(hits["t_start"][j]))
            if ov > 0:
                assert (ov / mn > 0.1) == (10 * ov > mn)
                clash = clash or 10 * ov > mn
        if not clash:
            kept.append(int(i))
            flag[i] = True
    return flag


def piece_model(db, hits, best, tol) -> dict:
    """core.py:219-301 and interval.py:596-637 on a hit table, in plain Python: the kept rows, their clusters, the primary hits, the
    pieces (contig, start, end, strand, mean position) and who lies inside one."""
    locus, extra = db.gene_locus_indices, db.extra_genes.astype(bool)
    flag = cull_model(hits, visit_order(hits, locus[hits["gene"]] == best))
    k = hits[flag]
    by_pos = sorted(range(len(k)), key=lambda i: (int(k["contig"][i]), int(k["t_start"][i]), int(k["t_end"][i])))
    cluster, cur, cur_e, cur_c = np.zeros(len(k), int), -1, 0, None
    for i in by_pos:
        if cur_c == int(k["contig"][i]) and int(k["t_start"][i]) <= cur_e + tol:
            cur_e = max(cur_e, int(k["t_end"][i]))
        else:
            cur, cur_e, cur_c = cur + 1, int(k["t_end"][i]), int(k["contig"][i])
        cluster[i] = cur
    expected = (locus[k["gene"]] == best) & ~extra[k["gene"]]
    primary = np.zeros(len(k), bool)
    for gene in np.unique(k["gene"]):
        rows = np.flatnonzero(k["gene"] == gene)
        top = rows[np.argmax(k["score"][rows])]  # argmax: the first of equal scores
        primary[top] = expected[top]
    pieces = []
    for c in range(cur + 1):
        rows = np.flatnonzero((cluster == c) & primary)
        if len(rows):
            vote = int((k["strand"][rows].astype(int) * db.gene_intervals.strands[k["gene"][rows]].astype(int)).sum())
            pieces.append((int(k["contig"][rows[0]]), int(k["t_start"][rows].min()), int(k["t_end"][rows].max()), -1 if vote < 0 else 1,
                           float(db.gene_positions[k["gene"][rows]].astype(np.int64).sum()) / len(rows), vote))
    inside = np.array([any(int(k["contig"][i]) == p[0] and int(k["t_start"][i]) <= p[2] and int(k["t_end"][i]) >= p[1] for p in pieces)
                       for i in range(len(k))], bool)
    return dict(kept=k, cluster=cluster, expected=expected, primary=primary, pieces=pieces, inside=inside)


def _frame(R: Rules, db, right=14000):
    """L and R (module docstring): rows, and the first free base behind L."""
    pad = R.contig["pad"]
    l0, l1 = int(db.genes.lengths[R.g0]), int(db.genes.lengths[R.g0 + 1])
    return [make_hit(R.g0, pad, 100, 100 + l0, score=5000), make_hit(R.g0 + 1, pad, right, right + l1, score=4999)], 100 + l0 + 100


def _planted(R: Rules, label, **kw):
    c, s, e, g = R.at[label]
    return make_hit(g, c, s, e, **kw)


@lru_cache(maxsize=None)
def cases(key: str) -> tuple[Case, ...]:
    db, R = load_db(key), rules_assembly(key)
    pad, tol, L = R.contig["pad"], int(db.max_locus_length), db.genes.lengths
    out: list[Case] = []
    g = [R.g0 + i for i in range(R.n0)]  # the genes of locus 0
    # first gene of the first other locus with as many expected genes as locus 0: equal coverage sums are then equal final scores
    n_exp = [int((~db.extra_genes[o : o + n].astype(bool)).sum()) for o, n in zip(db.locus_gene_offsets, db.locus_gene_lengths)]
    # ... and with a second gene whose length is a multiple of 5, so that a coverage of exactly min_gene_coverage = 1 / 5 exists
    other, floor_gene = next((int(db.locus_gene_offsets[l]), int(db.locus_gene_offsets[l]) + j) for l in range(1, len(n_exp)) if n_exp[l] == n_exp[0]
                             for j in range(1, int(db.locus_gene_lengths[l])) if L[int(db.locus_gene_offsets[l]) + j] % 5 == 0)

    F_other = next(x for x in range(len(L)) if db.gene_locus_indices[x] not in (0, db.gene_locus_indices[other]) and not db.extra_genes[x])

    def add(group, name, rows, manual=False, **kw):
        out.append(Case(group, name, table(rows, manual), **kw))

    # ---- scores ------------------------------------------------------------------------------------------------------------------------
    # locus 0 holds one full-length gene (score 1.0); locus 1 one full-length gene and a second whose coverage is on the floor
    lg = int(L[floor_gene])
    floor = lg // 5
    base = [_planted(R, "g0"), make_hit(other, pad, 100, 100 + int(L[other]))]
    for side, n in ((0, floor - 1), (1, floor)):
        add("scores", f"cov_floor_{side}", base + [make_hit(floor_gene, pad, 5000, 5000 + n)], pair=("cov_floor", side),
            info=dict(kind="cov", gene=floor_gene, at_floor=bool(side)))
    # two hits of one gene with equal coverage and different scores: the coverage enters once
    add("scores", "equal_cov_two_scores", [_planted(R, "g0"), _planted(R, "g1", score=900), make_hit(g[1], pad, 100, 100 + int(L[g[1]]), score=700)],
        info=dict(kind="equal_cov", gene=g[1]))
    # two loci with bit-equal final scores (one full-length gene each): argmax takes the first
    add("scores", "tie_first_locus", [make_hit(other, pad, 100, 100 + int(L[other])), _planted(R, "g0", q_end=int(L[g[0]]))],
        info=dict(kind="tie"))
    # only hits below the floor: every score is zero
    add("scores", "all_below_floor", [make_hit(floor_gene, pad, 5000, 5000 + floor - 1)], info=dict(kind="zero"))
    # ... and the one kept hit is of no expected gene, outside every piece (there is none) and on random text: spurious, n_final is 0
    add("states", "all_spurious", [make_hit(floor_gene, pad, 5000, 5000 + floor - 1), make_hit(F_other, pad, 7000, 7090)], info=dict(kind="all_spurious"))
    if db.extra_genes.any():  # an extra gene would tip the tie if it were counted
        xg = int(np.flatnonzero(db.extra_genes)[0])
        add("scores", "extra_not_counted", [make_hit(other, pad, 100, 100 + int(L[other])), _planted(R, "g0"),
                                             make_hit(xg, pad, 6000, 6000 + int(L[xg]))], info=dict(kind="tie"))
        # an extra-gene locus cannot be the best locus by its own genes alone; extra genes beside a typed locus are reported
        add("clusters", "extra_gene_beside_locus", [_planted(R, f"g{i}") for i in range(R.n0)] + [make_hit(xg, R.contig["locus"], 20, 120, q_end=100)],
            info=dict(kind="extra_beside", gene=xg))

    # ---- cull --------------------------------------------------------------------------------------------------------------------------
    fr, free = _frame(R, db)
    # X (kept first: higher score) and Y overlap by exactly 10 % of the shorter and by one base more
    for tag, lx, ly in (("cand_shorter", 1000, 500), ("kept_shorter", 500, 1000), ("odd_min", 1000, 507), ("odd_min_kept", 503, 1000)):
        mn = min(lx, ly)
        for side, ov in ((0, mn // 10), (1, mn // 10 + 1)):
            x0 = free
            y0 = x0 + lx - ov
            add("cull", f"ov_{tag}_{side}", fr + [make_hit(g[2], pad, x0, x0 + lx, score=3000, q_end=30), make_hit(g[3], pad, y0, y0 + ly, score=2000, q_end=30)],
                pair=(f"ov_{tag}", side), info=dict(kind="overlap", ov=ov, mn=mn, exact=mn % 10 == 0 and side == 0, x=g[2], y=g[3]))
    x0 = free
    add("cull", "same_span_other_contig", fr + [make_hit(g[2], pad, x0, x0 + 1000, score=3000, q_end=30),
                                                make_hit(g[3], R.contig["locus"], x0, x0 + 1000, score=2000, q_end=30)],
        info=dict(kind="two_contigs", a=g[2], b=g[3]))
    add("cull", "empty_span_among", fr + [make_hit(g[2], pad, x0, x0, score=3000, q_end=30)], info=dict(kind="empty", n=3))
    add("cull", "empty_span_alone", [make_hit(g[2], pad, x0, x0, score=3000, q_end=30)], info=dict(kind="empty", n=1))
    # visit-order ties: X and Y clash; who is visited first survives
    for tag, kx, ky, first in (("matches", dict(matches=40), dict(matches=41), "y"), ("mapq_0_1", dict(mapq=0), dict(mapq=1), "x"),
                               ("mapq_1_255", dict(mapq=1), dict(mapq=255), "y"), ("mapq_0_255", dict(mapq=0), dict(mapq=255), "x"),
                               ("index", {}, {}, "x")):  # uint8(-mapq): 0 -> 0, 255 -> 1, 1 -> 255, ascending
        add("cull", f"tie_{tag}", fr + [make_hit(g[2], pad, x0, x0 + 300, score=2000, q_end=30, **kx), make_hit(g[3], pad, x0 + 100, x0 + 400, score=2000, q_end=30, **ky)],
            info=dict(kind="tie_order", first=g[2] if first == "x" else g[3]))
    # the priority bit: a hit of the best locus with the lower score beats a foreign one
    add("cull", "priority", fr + [make_hit(g[2], pad, x0, x0 + 300, score=200, q_end=30), make_hit(other + 2, pad, x0 + 100, x0 + 400, score=2000, q_end=30)],
        info=dict(kind="tie_order", first=g[2]))

    # ---- rounds ------------------------------------------------------------------------------------------------------------------------
    def span(p):
        return free + 80 * p

    def round_table(n, shape):
        """n hits in all; the hit at visit position p (L and R are 0 and 1) has score 4000 - p, 30 bases, its own slot -- unless
        `shape` moves it: {p: offset} puts it on the slot of position `offset[0]` shifted by `offset[1]` bases."""
        rows = list(fr)
        for p in range(2, n):
            slot, shift = shape.get(p, (p, 0))
            rows.append(make_hit(g[2 + p % (R.n0 - 2)], pad, span(slot) + shift, span(slot) + shift + 30, score=4000 - p))
        return rows

    for n in (LANES, LANES + 1, 2 * LANES, 2 * LANES + 1):
        shapes = {"all_survive": {}, "chain_head": {3: (2, 15), 4: (2, 40)}, "chain_tail": {LANES - 2: (LANES - 3, 15), LANES - 1: (LANES - 3, 40)}}
        if n > LANES:  # A is lane 63; B (and C) open the next round
            shapes["chain_across"] = {LANES: (LANES - 1, 15), **({LANES + 1: (LANES - 1, 40)} if n > LANES + 1 else {})}
            shapes["chain_b_last"] = {LANES - 1: (LANES - 2, 15), LANES: (LANES - 2, 40)}
        if n >= 2 * LANES:
            shapes["round1_none"] = {p: (2 + (p - LANES) % (LANES - 2), 15) for p in range(LANES, 2 * LANES)}
            shapes["round1_lane63"] = {p: (2 + (p - LANES) % (LANES - 2), 15) for p in range(LANES, 2 * LANES - 1)}
        for tag, shape in shapes.items():
            add("rounds", f"n{n}_{tag}", round_table(n, shape), info=dict(kind="round", n=n, shape=tag, moved=sorted(shape)))

    # ---- clusters and pieces --------------------------------------------------------------------------------------------------------------
    l0 = int(L[g[0]])
    for side in (0, 1):  # next start exactly cur_e + tolerance, and one base past it
        add("clusters", f"linkage_{side}", [make_hit(g[0], pad, 100, 100 + l0), make_hit(g[1], pad, 100 + l0 + tol + side, 100 + l0 + tol + side + 300)],
            pair=("linkage", side), info=dict(kind="linkage", gap=tol + side))
        # a long hit extends cur_e: the third hit joins only through it (it starts before the long one ends + tol, after the first's)
        e2 = 100 + l0 - 50 + 2500  # (the long hit overlaps the first by 50 bases, under a tenth of either)
        add("clusters", f"linkage_through_{side}", [make_hit(g[0], pad, 100, 100 + l0), make_hit(g[2], pad, e2 - 2500, e2, q_end=30),
                                                    make_hit(g[1], pad, e2 + tol + side, e2 + tol + side + 300)], pair=("linkage_through", side), info=dict(kind="linkage_through", first=g[0], long=g[2], third=g[1]))
    # (equal (contig, t_start) ordered by t_end cannot reach the cluster sort: two non-empty hits with one start on one contig overlap by
    # the whole shorter one, and the cull keeps one of them)
    add("clusters", "same_coords_two_contigs", [make_hit(g[0], pad, 100, 100 + l0), make_hit(g[1], R.contig["locus"], 100, 100 + l0, q_end=min(l0, int(L[g[1]])))],
        info=dict(kind="two_contigs", a=g[0], b=g[1]))
    # a cluster of expected genes without a primary hit gives no piece: g1's top hit is in the first cluster
    far = 100 + l0 + 550 + tol + 500  # past the tolerance of the near hit's end as well
    add("clusters", "cluster_without_primary", [make_hit(g[0], pad, 100, 100 + l0), make_hit(g[1], pad, 100 + l0 + 50, 100 + l0 + 550, score=900),
                                                make_hit(g[1], pad, far, far + 400, score=400)], info=dict(kind="no_primary", gene=g[1]))
    # primary among equal scores: the earliest in emission order; and with the higher score later in emission order
    for side, (s1, s2) in enumerate(((700, 700), (700, 701))):
        add("clusters", f"primary_{side}", [make_hit(g[0], pad, 100, 100 + l0), make_hit(g[1], pad, 100 + l0 + 50, 100 + l0 + 450, score=s1),
                                            make_hit(g[1], pad, far, far + 400, score=s2)], manual=True, pair=("primary", side),
            info=dict(kind="primary", gene=g[1], equal=s1 == s2))
    # strand votes: the primaries of one piece, hit strand times gene strand summing to -1, 0 and +1; three hits each -- at 0 the
    # third is of a gene of another locus and has no vote
    gs = db.gene_intervals.strands
    for vote, strands in ((-1, (-1, -1, 1)), (0, (1, -1, 0)), (1, (1, 1, -1))):
        rows, pos = [], 100
        for i, st in enumerate(strands):
            gene = g[i] if st else other + 2
            n = int(L[gene])
            rows.append(make_hit(gene, pad, pos, pos + n, strand=int(st * gs[gene]) if st else 1))
            pos += n + 50
        add("clusters", f"vote_{vote}", rows, pair=("vote_sign", 0 if vote < 0 else 1) if vote != 1 else None, info=dict(kind="vote", vote=vote))
    add("clusters", "mean_pos_one", [make_hit(g[4], pad, 100, 100 + int(L[g[4]]))], info=dict(kind="mean_pos", n=1))
    # touching a piece: an unexpected gene's hit at t_start == piece.end / t_end == piece.start, and one base outside
    for side in (0, 1):
        add("clusters", f"touch_end_{side}", [make_hit(g[0], pad, 1000, 1000 + l0), make_hit(other + 2, pad, 1000 + l0 + side, 1000 + l0 + side + 90)],
            pair=("touch_end", side), info=dict(kind="touch", end="end", gene=other + 2))
        add("clusters", f"touch_start_{side}", [make_hit(g[0], pad, 1000, 1000 + l0), make_hit(other + 2, pad, 910 - side, 1000 - side)],
            pair=("touch_start", side), info=dict(kind="touch", end="start", gene=other + 2))
    # every gene of the locus found, and one of them not hit at all (missing).  An expected gene found ONLY outside every piece
    # cannot be built: its top-scoring kept hit is primary and makes a piece (cluster_without_primary is the nearest case)
    add("clusters", "all_genes_found", [_planted(R, f"g{i}") for i in range(R.n0)], info=dict(kind="found", absent=[]))
    add("clusters", "one_gene_absent", [_planted(R, f"g{i}") for i in range(R.n0) if i != 2], info=dict(kind="found", absent=[g[2]]))

    # ---- kept-list residency ----------------------------------------------------------------------------------------------------------------
    for side, nk in enumerate((KEPT_IN_LDS, KEPT_IN_LDS + 1)):
        rows = list(fr)
        for p in range(2, nk):
            rows.append(make_hit(g[2 + p % (R.n0 - 2)], pad, free + 40 * p, free + 40 * p + 30, score=4000 - p))
        add("resident", f"kept_{nk}", rows, info=dict(kind="resident", nk=nk))

    # ---- translation --------------------------------------------------------------------------------------------------------------------------
    ls = int(L[R.S])
    for strand, label in ((1, "exact"), (-1, "rc")):
        c, s, e, _ = R.at[label]
        for qs in (0, 1, 2):
            for cut in (0, 1, 2):  # q = [qs, ls - cut): the extracted text starts at gene base qs and ends `cut` short
                ts, te = (s + qs, e - cut) if strand > 0 else (s + cut, e - qs)
                add("translation", f"frame_q{qs}_cut{cut}_{'fwd' if strand > 0 else 'rev'}", [_planted(R, "g0"), make_hit(R.S, c, ts, te, strand=strand, q_start=qs)],
                    info=dict(kind="frame", q_mod=qs % 3, rem=(te - ts - (3 - qs % 3) % 3) % 3))
    for label in ("stop0", "stop1", "two_stops", "no_stop", "n0", "n1", "n2", "nrun", "stop_n", "exact"):
        add("translation", f"text_{label}", [_planted(R, "g0"), _planted(R, label)], info=dict(kind="text", label=label))
    # empty slots: a span no longer than its frame (2 bases, q_start % 3 == 1) -- first, last, two in a row in the middle of the kept list
    def tiny(gene, at):
        return make_hit(gene, pad, at, at + 2, q_start=1, score=50)

    fr2, free2 = _frame(R, db)
    mid = [make_hit(gx, pad, free2 + 100 * i, free2 + 100 * i + 60, score=3000 - i) for i, gx in enumerate(g[2:7])]
    add("translation", "empty_first", [make_hit(g[1], pad, 14000, 14000 + int(L[g[1]]), score=4999), tiny(g[0], free2 + 950)] + mid +
        [make_hit(g[0], pad, 100, 100 + l0, score=5000)], manual=True, info=dict(kind="empty_slot", where=[0]))
    add("translation", "empty_last", fr2 + mid + [tiny(g[6], free2 + 900)], info=dict(kind="empty_slot", where=[-1]))
    add("translation", "empty_two_mid", fr2 + mid + [tiny(g[3], free2 + 900), tiny(g[3], free2 + 950)], info=dict(kind="empty_slot", where="mid"))
    # the 256-codon rounds: S whole (its codons first in the list) and a piece of g<next> that brings the total to 255 / 256 / 257
    nS = ls // 3
    nxt = next(i for i in range(R.n0) if g[i] > R.S)
    for tot in (CODON_ROUND - 1, CODON_ROUND, CODON_ROUND + 1):
        c2, s2, _, g2 = R.at[f"g{nxt}"]
        add("translation", f"codons_{tot}", [_planted(R, "exact"), make_hit(g2, c2, s2, s2 + 3 * (tot - nS))], info=dict(kind="codons", total=tot))
    # a slot across the round edge whose stop lies in the later round: S whole, then S with the stop at codon stop_hi
    add("translation", "stop_in_later_round", [_planted(R, "exact", score=ls + 1), _planted(R, "stop_hi")], manual=True,
        info=dict(kind="codons", total=2 * nS, stop_at=nS + R.cstop["stop_hi"]))

    # ---- states ---------------------------------------------------------------------------------------------------------------------------------
    for fl in (EDGE_TOL, EDGE_TOL + 1):
        for rev in (False, True):
            c, s, e, _ = R.at[f"e{fl}{'r' if rev else ''}"]
            for edge in ("left", "right"):
                for clipped in (False, True):
                    # the hit touches one contig edge at distance fl and stays 3 bases further from the other; the query is clipped
                    # at the end that faces the edge, or at the other
                    ts, te = (s, e - 3) if edge == "left" else (s + 3, e)
                    q_low = (edge == "left") != rev  # the gene's start faces the tested edge
                    qs, qe = ((3, ls) if q_low else (0, ls - 3)) if clipped else ((0, ls - 3) if q_low else (3, ls))
                    add("states", f"edge_{edge}_{'rev' if rev else 'fwd'}_{'clipped' if clipped else 'whole'}_{fl}",
                        [_planted(R, "g0"), make_hit(R.S, c, ts, te, strand=-1 if rev else 1, q_start=qs, q_end=qe)],
                        pair=(f"edge_{edge}_{'rev' if rev else 'fwd'}", fl - EDGE_TOL) if clipped else None,
                        info=dict(kind="edge", edge=edge, dist=fl, clipped=clipped))
    c, s, e, _ = R.at[f"e{EDGE_TOL}s"]
    for side, (qs, qe) in enumerate(((3, ls), (0, ls - 3))):  # partial wins over truncated; unclipped, the same text is truncated
        add("states", f"partial_over_truncated_{side}", [_planted(R, "g0"), make_hit(R.S, c, s, e - 3, q_start=qs, q_end=qe)], pair=("partial_truncated", side),
            info=dict(kind="partial_truncated", clipped=side == 0))
    for side, label in enumerate(("stop_lo", "stop_hi")):
        add("states", f"prot_cov_{label}", [_planted(R, "g0"), _planted(R, label)], pair=("prot_cov", side), info=dict(kind="prot_cov", label=label, gene=R.S))
    for label in ("c_lo", "c_eq", "c_hi"):  # exactly 0.90 on a gene whose length allows it: not truncated
        add("states", f"prot_cov_{label}", [_planted(R, "g0"), _planted(R, label)], pair=("prot_cov_exact", 0 if label == "c_lo" else 1) if label != "c_hi" else None,
            info=dict(kind="prot_cov", label=label, gene=R.Cg))
    for d, tag in enumerate(("below", "at", "above")):  # identity around the threshold: inside the locus (novel / normal) and outside (spurious / kept)
        add("states", f"identity_inside_{tag}", [_planted(R, "g0"), _planted(R, f"id_{tag}")], pair=("id_inside", d) if d < 2 else None,
            info=dict(kind="identity", tag=tag, gene=R.S))
        add("states", f"identity_outside_{tag}", [_planted(R, "g0"), _planted(R, f"f_id_{tag}")], pair=("id_outside", d) if d < 2 else None,
            info=dict(kind="identity", tag=tag, gene=R.F))
    add("states", "short_contig", [_planted(R, "g0"), _planted(R, "short")], info=dict(kind="short_contig"))
    for n in (7, 8, 9):  # the mean identity over 7, 8 and 9 normal genes (kp_np_sum_f32: sequential below 8, eight running sums from 8)
        if n - 1 <= R.n0 - 1:
            rows = [_planted(R, f"g{i}") for i in range(R.n0) if g[i] != R.S][: n - 1] + [_planted(R, "id_above")]
            add("states", f"mean_of_{n}", rows, info=dict(kind="mean", n=n))
    for n in (MANY - 1, MANY):  # ... and over 128 and 129: the whole pairwise block, and the split in two halves behind it
    # (copy i is hit without its last i % 7 codons: identities over different totals, so that their float32 sum depends on its association)
        rows = [make_hit(R.S, R.at[f"many{i}"][0], R.at[f"many{i}"][1], R.at[f"many{i}"][2] - 3 * (i % 7), score=ls - i) for i in range(n)]
        add("states", f"mean_of_{n}", rows, info=dict(kind="mean", n=n))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def cases_of(key: str, group: str) -> list[Case]:
    return [c for c in cases(key) if c.group == group]


# ---- the fixture's layout ---------------------------------------------------------------------------------------------------------------
# One file per database.  A recorded field of all cases is one flat array and the cases' lengths (an entry per case and
# field would cost more in archive headers than in data); strings are joined by newlines; the two large sequence blobs, which are
# substrings of the assembly, are recorded by their SHA-1.
DIGESTED = ("locus_seqs.seqs", "gene_seqs.seqs")


def digest(a) -> np.ndarray:
    import hashlib

    return np.frombuffer(hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest().encode(), np.uint8)


def pack_records(records: list[dict]) -> dict:
    out = {}
    for f in records[0]:
        arrs = [np.asarray(r[f]) for r in records]
        assert all(a.ndim <= 1 for a in arrs) and len({a.ndim for a in arrs}) == 1, f
        if arrs[0].dtype.kind == "U":
            out[f"{f}|count"] = np.array([a.size for a in arrs], np.int64)
            arrs = [np.frombuffer("\n".join(str(x) for x in a.ravel()).encode(), np.uint8) for a in arrs]
        else:
            assert len({a.dtype for a in arrs}) == 1, f
        out[f"{f}|ndim"] = np.int64(np.asarray(records[0][f]).ndim)
        out[f"{f}|len"] = np.array([a.size for a in arrs], np.int64)
        out[f"{f}|data"] = np.concatenate([a.ravel() for a in arrs])
    return out


def unpack_records(z, prefix: str, n: int) -> list[dict]:
    fields = sorted({k[len(prefix) : -5] for k in z.files if k.startswith(prefix) and k.endswith("|data")})
    recs: list[dict] = [{} for _ in range(n)]
    for f in fields:
        data, lens, ndim = z[f"{prefix}{f}|data"], z[f"{prefix}{f}|len"], int(z[f"{prefix}{f}|ndim"])
        off = np.concatenate([[0], np.cumsum(lens)])
        counts = z[f"{prefix}{f}|count"] if f"{prefix}{f}|count" in z.files else None
        for i in range(n):
            a = data[off[i] : off[i + 1]]
            if counts is not None:
                a = np.array(bytes(a).decode().split("\n") if counts[i] else [], dtype="U")
            recs[i][f] = a.reshape(()) if ndim == 0 else a
    return recs


def fixture_path(key: str) -> Path:
    return ROOT / "tests" / "golden" / f"typing_rules_{key}.npz"


@lru_cache(maxsize=None)
def load_rules(key: str):
    """(genome, [(group, name, hits, exp, scalars, kwargs)]) as recorded: `exp` / `scalars` as tests.golden_util.load_case gives them,
    but for the DIGESTED fields, which hold the SHA-1 of the reference's bytes."""
    import json

    z = np.load(fixture_path(key), allow_pickle=False)
    lengths = z["contig_lengths"]
    offsets = np.zeros(len(lengths), np.int32)
    np.cumsum(lengths[:-1], out=offsets[1:])
    genome = GenomeAssembly(str(z["genome_id"]), Sequences(tuple(str(s) for s in z["contig_ids"]), z["contig_seqs"], offsets, lengths))
    names, groups = [str(s) for s in z["names"]], [str(s) for s in z["groups"]]
    hit_off = z["hit_off"]
    out = []
    for i, exp in enumerate(unpack_records(z, "exp.", len(names))):
        scalars = json.loads(bytes(exp.pop("scalars_json")).decode())
        kwargs = json.loads(bytes(exp.pop("typer_kwargs_json")).decode())
        out.append((groups[i], names[i], z["hits"][hit_off[i] : hit_off[i + 1]], exp, scalars, kwargs))
    return genome, out


def check_against_fixture(res, exp, scalars) -> None:
    """tests.test_host_golden.check_result_against_golden with the DIGESTED fields compared by digest."""
    from tests.test_host_golden import check_result_against_golden

    d = res.to_dict()
    full = dict(exp)
    for f in DIGESTED:
        group = f.split(".")[0]
        got = np.frombuffer(d[group]["seqs"].encode(), np.uint8)
        assert bytes(digest(got)) == bytes(exp[f]), f
        full[f] = got
    check_result_against_golden(res, full, scalars)


# ---- the core header's records of a case (the g++ harness; the oracle's protein DP in between) ----------------------------------------
def core_records(db, typer, genome, hits, oracle, **caps):
    """What test_core_reduction_matches_reference runs, kept whole: (scores, counts, best, kept, pieces, summary, prot)."""
    from kaptive_amd.serotyping import batch as B
    from tests import harness_util as H

    hdb, prm = H.HarnessDb(db), H.params(db, typer)
    scores, counts = H.locus_scores(hits, hdb, typer.min_gene_coverage)
    best, final, completeness = B.choose_best_loci(scores[None, :], counts[None, :], typer._expected_genes_per_locus)
    kept, pieces, summary, prot = H.reduce(hits, hdb, prm, best[0], genome.packed(), **caps)
    dp = oracle.protein_align(prot, kept["prot_off"], kept["prot_len"], db.translations.seqs, db.translations.offsets[kept["gene"]],
                              db.translations.lengths[kept["gene"]])  # fmt: skip
    kept = H.states(kept, hdb, prm, genome.contigs.lengths, dp, summary)
    return dict(scores=scores, counts=counts, best=int(best[0]), final=final[0], completeness=completeness[0], kept=kept, pieces=pieces,
                summary=summary, prot=prot)  # fmt: skip
