"""Inputs that walk the stretch between a sorted anchor list and the filled bands (csrc/kp_chain.hip: kp_chain_kernel,
kp_chain_score_kernel, kp_task_hist_kernel, kp_task_scatter_kernel; csrc/kp_sw.hip: kp_sw_kernel): every rule that decides
whether a cluster becomes a task, where a run is cut and how wide its band is, where the rounds of 64 anchors, the per-block
task stage, the chain-score tile and the length buckets of the task order end, and the shapes the packed fill can take.
Seeded and pure numpy.  Where a case needs an exact anchor count, span, chain score or row count, its parameters were searched
with the oracle (profiles/band_tasks.md) and are kept as literals; tests/test_band_tasks_oracle.py re-checks every label on every run
with the oracle alone, tests/test_gpu_band_tasks.py shows that the device equals the oracle on every case.
TEST INFRASTRUCTURE: no GPU, and the oracle only where a function takes it as an argument.

Restated here in Python, because the labels are claims about them: the clustering and band rule of kp_spec.h (clusters),
the chain of a small cluster with what it did on the way (chain_small), kp_task_rows of csrc/kp_internal.h (task_rows -- the
two point at each other), and the slice rule of kp_chain_kernel (owner_waves): per = the list's share of a wave in whole
rounds of 64, a wave skips ahead to the first anchor of another gene/strand than the one before its slice, and owns the
gene/strand groups that start in its slice."""

from __future__ import annotations

import functools
import re
from pathlib import Path
from typing import Callable, NamedTuple

import numpy as np

from kaptive_amd.core.genome import GenomeAssembly
from kaptive_amd.core.seq import SeqRecord, Sequences
from kaptive_amd.synth import random_dna, revcomp
from tests import occ_cut_util as OU

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "kaptive_amd" / "csrc"


# ---- the constants the paths hang on, read out of the sources ----------------------------------------------------------------------
def kernel_constants() -> dict[str, int]:
    spec = (ROOT / "include" / "kp_spec.h").read_text()
    chain, internal, sw = (CSRC / "kp_chain.hip").read_text(), (CSRC / "kp_internal.h").read_text(), (CSRC / "kp_sw.hip").read_text()
    out = {}
    for name in ("KP_K", "KP_W", "KP_DIAG_GAP", "KP_MAX_BAND", "KP_BAND_MARGIN", "KP_BAND_MARGIN_NARROW", "KP_MIN_ANCHORS", "KP_MIN_SEED_SPAN",
                 "KP_CHAIN_DP_MAX", "KP_MIN_CHAIN_SCORE", "KP_MIN_DP_SCORE", "KP_JOIN_BW", "KP_FILL16_MAX_GENE_LEN", "KP_CHAIN_MAX_DIST"):  # fmt: skip
        out[name] = int(re.search(rf"#define\s+{name}\s+(\d+)", spec).group(1))
    assert re.search(r"#define KP_MAX_SPREAD \(KP_MAX_BAND - 2 \* KP_BAND_MARGIN - 1\)", spec)
    out["KP_MAX_SPREAD"] = out["KP_MAX_BAND"] - 2 * out["KP_BAND_MARGIN"] - 1
    for name in ("KP_CHAIN_SLICES", "KP_CHAIN_WAVES", "KP_CHAIN_STAGE", "KP_CS_TILE"):
        out[name] = int(re.search(rf"#ifndef {name}\n#define {name} (\d+)", chain).group(1))
    m = re.search(r"int length_bucket\(int rows\) \{\s*const int b = rows >> (\d+);\s*return (\d+) - \(b > (\d+) \? (\d+) : b\);", chain)
    assert m and len({m.group(2), m.group(3), m.group(4)}) == 1
    out["BUCKET_SHIFT"], out["BUCKET_CLAMP"] = int(m.group(1)), int(m.group(2))
    out["KP_ORDER_BUCKETS"] = int(re.search(r"#define KP_ORDER_BUCKETS (\d+)", internal).group(1))
    out["CH"] = int(re.search(r"constexpr int CH = (\d+);", sw).group(1))
    lanes = [int(x) for x in re.findall(r"sw_class<(\d+)>\(b, genes, tasks \+ off", sw)]
    assert lanes == [32, 16, 8, 4], lanes  # classes 3, 2, 1, 0: a band of W diagonals is held by W / 4 lanes
    out["P16"], out["P64"], out["P128"] = lanes[3], lanes[1], lanes[0]
    return out


EXPECTED_CONSTANTS = dict(KP_K=15, KP_W=10, KP_DIAG_GAP=32, KP_MAX_BAND=128, KP_BAND_MARGIN=15, KP_BAND_MARGIN_NARROW=7, KP_MIN_ANCHORS=3,
                          KP_MIN_SEED_SPAN=40, KP_CHAIN_DP_MAX=24, KP_MIN_CHAIN_SCORE=40, KP_MIN_DP_SCORE=80, KP_JOIN_BW=500,
                          KP_FILL16_MAX_GENE_LEN=15800, KP_CHAIN_MAX_DIST=5000, KP_MAX_SPREAD=97, KP_CHAIN_SLICES=16, KP_CHAIN_WAVES=4,
                          KP_CHAIN_STAGE=640, KP_CS_TILE=512, BUCKET_SHIFT=5, BUCKET_CLAMP=63, KP_ORDER_BUCKETS=65, CH=64, P16=4, P64=16, P128=32)  # fmt: skip
C = EXPECTED_CONSTANTS  # every size below is derived from these; the CPU module asserts that the sources still hold them
K, GAP, SPREAD, JOIN_BW = C["KP_K"], C["KP_DIAG_GAP"], C["KP_MAX_SPREAD"], C["KP_JOIN_BW"]
MIN_ANCHORS, MIN_SPAN, DP_MAX, MIN_CHAIN, MIN_DP = C["KP_MIN_ANCHORS"], C["KP_MIN_SEED_SPAN"], C["KP_CHAIN_DP_MAX"], C["KP_MIN_CHAIN_SCORE"], C["KP_MIN_DP_SCORE"]
SLICES, WAVES, STAGE, TILE = C["KP_CHAIN_SLICES"], C["KP_CHAIN_WAVES"], C["KP_CHAIN_STAGE"], C["KP_CS_TILE"]
LANES = {16: C["P16"], 64: C["P64"], 128: C["P128"]}  # lanes per pair of tasks, by band width (32 diagonals: never reached)
DIAG_BIAS = 65536
CHAIN_PEN = [int(x) for x in re.search(r"#define KP_CHAIN_PEN_TABLE\s*\\\s*\{(.*?)\}", (ROOT / "include" / "kp_spec.h").read_text(), flags=re.S).group(1).replace("\\", " ").split(",")]


# ---- the rules, restated -----------------------------------------------------------------------------------------------------------
def band_of(spread: int) -> tuple[int, int, int]:
    """(margin, need, width) of a cluster whose diagonals range over ``spread`` (kp_spec.h: anchors -> DP tasks)."""
    margin, need = C["KP_BAND_MARGIN_NARROW"], spread + 1 + 2 * C["KP_BAND_MARGIN_NARROW"]
    if need <= 16:
        return margin, need, 16
    margin, need = C["KP_BAND_MARGIN"], spread + 1 + 2 * C["KP_BAND_MARGIN"]
    return margin, need, 32 if need <= 32 else (64 if need <= 64 else 128)


def task_rows(lo: int, width: int, cstart: int, cend: int, qlen: int) -> tuple[int, int]:
    """kp_task_rows of csrc/kp_internal.h: the rows [r_lo, r_hi) of the gene whose band cells can lie inside the contig."""
    a = max(cstart - lo - (width - 1), 0) & ~7
    z = max(min(cend - lo, qlen), a)
    return a, z


def length_bucket(rows: int) -> int:
    """length_bucket of csrc/kp_chain.hip: 32 rows a bucket, everything from 2016 rows on in the first."""
    return C["BUCKET_CLAMP"] - min(rows >> C["BUCKET_SHIFT"], C["BUCKET_CLAMP"])


class Cluster(NamedTuple):
    gs: int
    contig: int
    first: int  # index of its first anchor in the sorted list
    cnt: int
    d0: int  # lowest / highest diagonal, assembly coordinates
    dmax: int
    qmin: int
    qmax: int

    @property
    def span(self) -> int:
        return self.qmax - self.qmin + K

    @property
    def spread(self) -> int:
        return self.dmax - self.d0

    @property
    def provisional(self) -> bool:
        return self.cnt >= MIN_ANCHORS and self.span >= MIN_SPAN

    @property
    def width(self) -> int:
        return band_of(self.spread)[2]

    @property
    def lo(self) -> int:
        margin, need, w = band_of(self.spread)
        return self.d0 - margin - (w - need) // 2


def decode(keys: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(gs, diagonal, query position) of sorted anchor keys (KP_ANCHOR_KEY)."""
    return (keys >> np.uint64(46)).astype(np.int64), ((keys >> np.uint64(16)) & np.uint64(0x3FFFFFFF)).astype(np.int64) - DIAG_BIAS, (keys & np.uint64(0xFFFF)).astype(np.int64)


def clusters(keys: np.ndarray, pa) -> list[Cluster]:
    """kp_spec.h's clusters of a sorted anchor list: a new one where gs or the contig changes, the diagonal jumps by more than
    KP_DIAG_GAP, or the cluster would span more than KP_MAX_SPREAD diagonals.  Weak ones included."""
    gs, d, q = decode(keys)
    ctg = np.searchsorted(np.asarray(pa.ctg_start, np.int64), d + q, "right") - 1
    gs, d, q, ctg = gs.tolist(), d.tolist(), q.tolist(), ctg.tolist()
    out, i, n = [], 0, len(gs)
    while i < n:
        j, qmin, qmax = i + 1, q[i], q[i]
        while j < n and gs[j] == gs[i] and ctg[j] == ctg[i] and d[j] - d[j - 1] <= GAP and d[j] - d[i] <= SPREAD:
            qmin, qmax = min(qmin, q[j]), max(qmax, q[j])
            j += 1
        out.append(Cluster(gs[i], ctg[i], i, j - i, d[i], d[j - 1], qmin, qmax))
        i = j
    return out


class Chain(NamedTuple):
    score: int
    n_anchors: int
    moved: int  # entries the insertion sort by (target, query) moved
    t_ties: int  # neighbours of the sorted order with the same target position
    max_ties: int  # anchors with two predecessors of the same best f + sc: the FIRST met going backwards wins
    dropped: int  # anchors of the cluster that are not on the chain
    cut_early: bool  # the walk back peaked before the chain's first anchor
    dd: tuple  # dd of every link of the chain


def chain_small(keys: np.ndarray) -> Chain:
    """kp_spec.h's chain of a cluster of at most KP_CHAIN_DP_MAX anchors, as chain_small of csrc/kp_chain.hip works it out."""
    _, d, q = decode(keys)
    t, q = (d + q).tolist(), q.tolist()
    n, moved = len(t), 0
    for i in range(1, n):
        ti, qi, j = t[i], q[i], i
        while j > 0 and (t[j - 1] > ti or (t[j - 1] == ti and q[j - 1] > qi)):
            t[j], q[j] = t[j - 1], q[j - 1]
            j -= 1
            moved += 1
        t[j], q[j] = ti, qi
    f, p, ddl, best, max_ties = [0] * n, [-1] * n, [0] * n, 0, 0
    for i in range(n):
        max_f, max_j, tie = K, -1, False
        for j in range(i - 1, -1, -1):
            dq, dr = q[i] - q[j], t[i] - t[j]
            if dq <= 0 or dq > C["KP_CHAIN_MAX_DIST"] or dr == 0:
                continue
            dd, dg = abs(dr - dq), min(dr, dq)
            sc = min(dg, K) - (CHAIN_PEN[min(dd, len(CHAIN_PEN) - 1)] if dd or dg > K else 0) + f[j]
            if sc > max_f:
                max_f, max_j, tie, ddl[i] = sc, j, False, dd
            elif sc == max_f and max_j >= 0:
                tie = True
        f[i], p[i] = max_f, max_j
        max_ties += tie
        if f[i] >= f[best]:
            best = i
    i, max_s, steps, cut, dds = best, 0, 0, 0, []
    while True:
        dds.append(ddl[i])
        i = p[i]
        steps += 1
        sc = f[best] if i < 0 else f[best] - f[i]
        if sc > max_s:
            max_s, cut = sc, steps
        if i < 0:
            break
    return Chain(max_s, cut, moved, sum(a == b for a, b in zip(t, t[1:])), max_ties, n - cut, cut < steps, tuple(dds[: cut - 1]))


def end_anchor_walks(keys: np.ndarray) -> tuple[int, list[int]]:
    """(largest f, anchors on the walk back from every anchor that holds it, in (target, query) order): kp_spec.h takes the LATER
    anchor on ties, which shows where the walks differ in length."""
    _, d, q = decode(keys)
    order = sorted(range(len(q)), key=lambda i: (int(d[i] + q[i]), int(q[i])))
    t, q = [int(d[i] + q[i]) for i in order], [int(q[i]) for i in order]
    f, p = [0] * len(t), [-1] * len(t)
    for i in range(len(t)):
        f[i] = K
        for j in range(i - 1, -1, -1):
            dq, dr = q[i] - q[j], t[i] - t[j]
            if dq <= 0 or dq > C["KP_CHAIN_MAX_DIST"] or dr == 0:
                continue
            dd, dg = abs(dr - dq), min(dr, dq)
            sc = min(dg, K) - (CHAIN_PEN[min(dd, len(CHAIN_PEN) - 1)] if dd or dg > K else 0) + f[j]
            if sc > f[i]:
                f[i], p[i] = sc, j
    walks = []
    for i in (i for i in range(len(t)) if f[i] == max(f)):
        n = 0
        while i >= 0:
            n, i = n + 1, p[i]
        walks.append(n)
    return max(f), walks


def slice_per(n: int) -> int:
    """Anchors per wave slice of kp_chain_kernel (whole rounds of 64)."""
    return ((n + SLICES - 1) // SLICES + 63) & ~63


def owner_waves(keys: np.ndarray) -> tuple[np.ndarray, list[tuple[int, int]]]:
    """The slice rule of kp_chain_kernel.  Returns (owner, ranges): owner[i] = the wave that walks anchor i, ranges[w] =
    [start, end) of the anchors wave w walks (start == end: it walks none -- its slice lies past the list's end, or the
    gene/strand that covers its slice's start covers the rest of the slice as well)."""
    gs = decode(keys)[0]
    n, per = len(gs), slice_per(len(gs))
    owner, ranges = np.full(n, -1, np.int64), []
    for w in range(SLICES):
        lo, hi = w * per, min(n, (w + 1) * per)
        if lo >= n:
            ranges.append((n, n))
            continue
        start = lo
        if lo > 0:
            other = np.flatnonzero(gs[lo:] != gs[lo - 1])
            start = lo + int(other[0]) if len(other) else n
        if start >= hi:
            ranges.append((start, start))
            continue
        past = np.flatnonzero(gs[hi:] != gs[hi - 1])
        end = hi + int(past[0]) if len(past) else n
        owner[start:end] = w
        ranges.append((start, end))
    return owner, ranges


def lone(cl: list[Cluster]) -> list[bool]:
    """Which clusters are in no sequence of two or more (kp_spec.h, GROUPS): per gene/strand and contig a cluster continues
    the sequence whose last cluster ends at most KP_JOIN_BW diagonals below it.  (Valid where a gene/strand has clusters on at
    most KP_JOIN_OPEN contigs and no sequence reaches KP_JOIN_GROUP_MAX: the CPU module asserts both for the cases that use it.)"""
    out, last = [True] * len(cl), {}
    for i, c in enumerate(cl):
        j = last.get((c.gs, c.contig))
        if j is not None and c.d0 - cl[j].dmax <= JOIN_BW:
            out[i] = out[j] = False
        last[c.gs, c.contig] = i
    return out


def staged_per_block(keys: np.ndarray, pa) -> list[int]:
    """Tasks every block of kp_chain_kernel asks its stage for: the lone clusters that are not weak (rejected later or not) of
    the gene/strand groups its waves own."""
    cl = clusters(keys, pa)
    owner = owner_waves(keys)[0]
    out = [0] * (SLICES // WAVES)
    for c, alone in zip(cl, lone(cl)):
        if alone and c.provisional:
            out[int(owner[c.first]) // WAVES] += 1
    return out


# ---- the database ------------------------------------------------------------------------------------------------------------------
N_FILL, N_TAIL, N_STAGE = 40, 40, 400
G_T, G_S, G_REP = N_FILL, N_FILL + 1, N_FILL + 2  # the gene under test, a second one, one with a 25-base repeat 30 bases on
G_TAIL = G_REP + 1
G_STAGE = G_TAIL + N_TAIL  # N_STAGE genes of 1.2 kb: distinct pieces for the stage and tile cases
G_F16, G_F16P = G_STAGE + N_STAGE, G_STAGE + N_STAGE + 1  # a gene of KP_FILL16_MAX_GENE_LEN bases and one a base longer
GENE_LEN = {G_T: 4002, G_S: 1500, G_REP: 1000, G_F16: C["KP_FILL16_MAX_GENE_LEN"], G_F16P: C["KP_FILL16_MAX_GENE_LEN"] + 1}
REP_AT, REP_LEN, REP_SHIFT = 500, 25, 30


@functools.lru_cache(maxsize=None)
def _genes() -> tuple:
    rng = np.random.default_rng(9101)
    fill = [random_dna(rng, int(rng.integers(150, 260)), 0.5) for _ in range(N_FILL)]
    test = [random_dna(rng, GENE_LEN[g], 0.5) for g in (G_T, G_S, G_REP)]
    test[2][REP_AT + REP_SHIFT : REP_AT + REP_SHIFT + REP_LEN] = test[2][REP_AT : REP_AT + REP_LEN]
    tail = [random_dna(rng, int(rng.integers(150, 260)), 0.5) for _ in range(N_TAIL)]
    stage = [random_dna(rng, 1200, 0.5) for _ in range(N_STAGE)]
    long_ = [random_dna(rng, GENE_LEN[g], 0.5) for g in (G_F16, G_F16P)]
    return tuple(fill + test + tail + stage + long_)


def genes() -> list[np.ndarray]:
    return list(_genes())


def gene_sequences() -> Sequences:
    return Sequences.from_records([SeqRecord(f"g{i}", g.tobytes()) for i, g in enumerate(genes())])


asm_of = OU.asm_of
BASES = np.frombuffer(b"ACGT", np.uint8)


def _flat(seed) -> list[int]:
    return [x for s in seed for x in _flat(s)] if isinstance(seed, (list, tuple)) else [int(seed) if seed >= 0 else 1_000_000 - int(seed)]


def flank(seed, n: int) -> np.ndarray:
    return random_dna(np.random.default_rng([9200, *_flat(seed)]), n, 0.5)


def other_base(b: int, k: int = 1) -> int:
    """A base that differs from b (k = 1, 2, 3: which one)."""
    return int(BASES[(int(np.flatnonzero(BASES == b)[0]) + k) % 4])


def guarded(core: np.ndarray, before: int | None, after: int | None, seed, left: int = 100, right: int = 100) -> np.ndarray:
    """The core between random flanks whose bases next to it differ from the gene bases ``before`` / ``after`` that would
    continue the copy: the copy ends where the core ends."""
    a, b = flank([seed, 1], left), flank([seed, 2], right)
    if before is not None and left:
        a[-1] = other_base(before)
    if after is not None and right:
        b[0] = other_base(after)
    return np.concatenate([a, core, b])


def staircase(gene: int, at: int, lengths, steps, seed, rc: bool = False) -> np.ndarray:
    """Fragments of one gene in order, ``lengths[i]`` bases each from base ``at``, separated by ``steps[i]``: s > 0 an insertion
    of s random bases (the diagonal rises by s), s < 0 a deletion of -s gene bases (it falls by -s)."""
    g, parts, pos = genes()[gene], [], at  # (rc: of the gene's reverse complement -- the copy lies on strand -1, its rows are that strand's)
    if rc:
        g = revcomp(g)
    for i, n in enumerate(lengths):
        parts.append(g[pos : pos + n])
        pos += n
        if i < len(steps):
            if steps[i] > 0:
                ins = flank([seed, 10 + i], steps[i])
                ins[0], ins[-1] = other_base(g[pos]), other_base(g[pos - 1], 2)  # (neither end extends a fragment)
                parts.append(ins)
            else:
                pos -= steps[i]
    return np.concatenate(parts)


def in_flanks(core: np.ndarray, seed, left: int = 100, right: int = 100, reverse: bool = False) -> np.ndarray:
    c = np.concatenate([flank([seed, 1], left), core, flank([seed, 2], right)])
    return revcomp(c) if reverse else c


class Case(NamedTuple):
    label: str  # which rule or edge it pins
    asms: tuple  # one assembly, or several that have to follow each other in a batch
    gene: int | None = None  # the gene whose clusters the label speaks of
    holds: Callable[[dict], bool] | None = None  # the label's claim about what measure() finds
    hit: bool = False  # the label claims a task scoring at least KP_MIN_DP_SCORE: the oracle must report a hit


def case(label, contigs, gene=G_T, holds=None, hit=False) -> Case:
    return Case(label, (asm_of(label.split(":")[0], contigs),), gene, holds, hit)


# ---- what the oracle finds in an assembly --------------------------------------------------------------------------------------------
def measure(odb, asm, gene: int | None) -> dict:
    """The clusters (restated rule) of ``gene`` -- of every gene if None --, the oracle's tasks of it and their fill."""
    pa = asm.packed()
    keys = odb.anchors(pa)
    cl = clusters(keys, pa)
    tasks = odb.tasks(pa)
    mine = [c for c in cl if gene is None or c.gs >> 1 == gene]
    tk = tasks[tasks["gs"] >> 1 == gene] if gene is not None else tasks
    chains = [chain_small(keys[c.first : c.first + c.cnt]) if c.cnt <= DP_MAX else None for c in mine]
    glen = [len(g) for g in genes()]
    cs, cl_len = np.asarray(pa.ctg_start).tolist(), np.asarray(pa.ctg_len).tolist()
    rows = [task_rows(int(t["lo"]), int(t["width"]), cs[t["contig"]], cs[t["contig"]] + cl_len[t["contig"]], glen[t["gs"] >> 1]) for t in tk]
    sw = odb.sw(pa, tk)
    hits = odb.align(pa)
    return dict(n=len(keys), keys=keys, pa=pa, all=cl, cl=mine, chains=chains, tasks=tk, rows=rows, steps=[b - a + LANES.get(int(t["width"]), 8) - 1 for (a, b), t in zip(rows, tk)],
                sw=sw, hits=hits[hits["gene"] == gene] if gene is not None else hits, first=mine[0].first if mine else -1)  # fmt: skip


# ---- A. which cluster becomes a task -----------------------------------------------------------------------------------------------
# Literals found with the oracle (an exact fragment never has three seeds over 40 bases -- consecutive minimizers are at most
# KP_W apart, so three of them cover at most 2 KP_W + KP_K = 35 --: anchors_3 carries a substitution, the chain cases an
# indel, dp_24 a tandem duplication that puts one seed on two diagonals); tests/test_band_tasks_oracle.py re-checks each.
def _fragment(gene, a, n, seed, sub=None, reverse=False, left=100, right=100):
    g = genes()[gene]
    core = g[a : a + n].copy()
    if sub is not None:
        core[sub] = other_base(core[sub])
    c = guarded(core, g[a - 1] if a else None, g[a + n] if a + n < len(g) else None, seed, left, right)
    return revcomp(c) if reverse else c


def _two(a, l1, l2, s, tries):
    """Two fragments of G_T around one indel, as the search drew them."""
    g = genes()[G_T]
    return guarded(staircase(G_T, a, [l1, l2], [s], [3, tries]), g[a - 1], g[a + l1 + l2 + (-s if s < 0 else 0)], [3, tries])


def _dup(a, l1, dup, l2, tries):
    """l1 bases of G_T, then l2 bases from ``dup`` bases back: the seeds of the repeated bases lie on two diagonals."""
    g = genes()[G_T]
    return guarded(np.concatenate([g[a : a + l1], g[a + l1 - dup : a + l1 - dup + l2]]), g[a - 1], g[a + l1 - dup + l2], [4, tries])


COUNT_FRAGMENTS = {3: (3048, 44, 25), 4: (305, 46, None), 5: (300, 51), 6: (300, 52), 7: (300, 61), 8: (300, 66), 9: (300, 76), 10: (300, 82), 11: (300, 89),
                   12: (300, 88), 13: (300, 98), 14: (300, 102), 15: (300, 109), 16: (300, 118), 17: (300, 116), 18: (300, 123), 19: (300, 124),
                   20: (300, 127), 21: (300, 135), 22: (300, 138), 23: (300, 140), 24: (300, 146), 25: (300, 147), 26: (300, 154)}  # fmt: skip


def count_fragment(n: int, reverse: bool = False) -> np.ndarray:
    """A contig whose one cluster of G_T has exactly n anchors and becomes a task."""
    p = COUNT_FRAGMENTS[n]
    if len(p) == 3:
        return _fragment(G_T, p[0], p[1], [1, p[0], p[1]], sub=p[2], reverse=reverse)
    return _fragment(G_T, p[0], p[1], [2, p[0], p[1]], reverse=reverse)


def one_cluster(m) -> tuple:
    assert len(m["cl"]) == 1, [tuple(c) for c in m["cl"]]
    return m["cl"][0], m["chains"][0], m["tasks"]


def which_cases() -> list[Case]:
    out = []
    add = lambda label, contig, holds, hit=False, gene=G_T: out.append(case(label, [contig], gene, holds, hit))  # noqa: E731

    def h(pred, n_tasks):  # one cluster, n_tasks tasks, and the label's claim
        def holds(m):
            c, ch, tk = one_cluster(m)
            return len(tk) == n_tasks and pred(c, ch, tk)
        return holds

    add("anchors_2: two anchors, weak whatever they cover", _fragment(G_T, 100, 24, [1, 100, 24]), h(lambda c, ch, tk: c.cnt == MIN_ANCHORS - 1, 0))
    add("anchors_3: three anchors over at least 40 query bases", count_fragment(3), h(lambda c, ch, tk: c.cnt == MIN_ANCHORS and c.span >= MIN_SPAN and tk[0]["n_anchors"] == 3, 1))
    add("span_39: six anchors over 39 query bases, weak", _fragment(G_T, 121, 43, [1, 121, 43]), h(lambda c, ch, tk: c.cnt >= MIN_ANCHORS and c.span == MIN_SPAN - 1, 0))
    add("span_40: six anchors over 40 query bases", _fragment(G_T, 170, 47, [1, 170, 47]), h(lambda c, ch, tk: c.cnt >= MIN_ANCHORS and c.span == MIN_SPAN, 1))
    prov = lambda c: c.provisional and c.cnt <= DP_MAX  # noqa: E731
    add("chain_39_dd1: provisional, rejected at chain score 39; a link with dd = 1 (penalty 0)", _two(2213, 26, 20, 1, 3),
        h(lambda c, ch, tk: prov(c) and ch.score == MIN_CHAIN - 1 and max(ch.dd) == 1 and CHAIN_PEN[1] == 0, 0))
    add("chain_40_dd1: kept at chain score 40; a link with dd = 1 (penalty 0)", _two(3097, 18, 32, 1, 155),
        h(lambda c, ch, tk: prov(c) and ch.score == MIN_CHAIN == tk[0]["chain_score"] and max(ch.dd) == 1, 1))
    add("chain_39_dd20: provisional, rejected at chain score 39; a link with dd = 20", _two(1144, 27, 23, -20, 6),
        h(lambda c, ch, tk: prov(c) and ch.score == MIN_CHAIN - 1 and max(ch.dd) == 20 and CHAIN_PEN[20] > 0, 0))
    add("chain_40_dd12: kept at chain score 40; a link with dd = 12; two predecessors with the same f + sc (first_max)", _two(2581, 35, 18, 12, 0),
        h(lambda c, ch, tk: prov(c) and ch.score == MIN_CHAIN == tk[0]["chain_score"] and max(ch.dd) == 12 and ch.max_ties > 0, 1))
    add("dp_24: 24 anchors, chained exactly: the chain drops two of them", _dup(2691, 77, 24, 79, 24),
        h(lambda c, ch, tk: c.cnt == DP_MAX and ch.dropped == 2 and tk[0]["n_anchors"] == DP_MAX - 2 and tk[0]["chain_score"] == ch.score != min(K * c.cnt, c.span), 1), hit=True)
    add("dp_25: 25 anchors, the co-linear rule although a seed lies on two diagonals", _dup(2286, 57, 30, 106, 0),
        h(lambda c, ch, tk: c.cnt == DP_MAX + 1 and tk[0]["n_anchors"] == c.cnt and tk[0]["chain_score"] == min(K * c.cnt, c.span), 1), hit=True)
    g = genes()[G_T]
    add("end_tie: two anchors hold the largest f, the walk back from the earlier has 7 anchors, from the later 8: the later one ends the chain",
        guarded(np.concatenate([g[2496:2550], g[2522:2559]]), g[2495], g[2559], [70, 877]),
        h(lambda c, ch, tk: c.cnt <= DP_MAX and ch.score == 49 == tk[0]["chain_score"] and tk[0]["n_anchors"] == 8, 1))
    add("reorder_del: a 20-base deletion in the contig: the later anchors sort first by diagonal, the insertion sort moves them",
        guarded(staircase(G_T, 700, [80, 80], [-20], [5, -20]), g[699], g[880], [5, -20]), h(lambda c, ch, tk: c.cnt <= DP_MAX and ch.moved > 0 and c.spread == 20 and c.width == 64, 1), hit=True)
    r = genes()[G_REP]
    add("reorder_tie: a gene with a 25-base repeat 30 bases on: anchors with the same target position and different query positions",
        guarded(r[REP_TIE[0] : REP_TIE[1]], r[REP_TIE[0] - 1], r[REP_TIE[1]], [6]), h(lambda c, ch, tk: c.cnt <= DP_MAX and ch.t_ties > 0 and c.spread == 2 * REP_SHIFT, 1), gene=G_REP)
    return out


REP_TIE = (490, 565)


def count_cases() -> list[Case]:
    """One assembly per anchor count from 3 to 26 and strand: every bin of kp_chain_score_kernel's counting sort."""
    out = []
    for n in range(MIN_ANCHORS, DP_MAX + 3):
        for rev in (False, True):
            strand = "-" if rev else "+"
            out.append(case(f"count_{n}{strand}: one cluster of {n} anchors on strand {strand}", [count_fragment(n, rev)], G_T,
                            lambda m, n=n, rev=rev: one_cluster(m)[0].cnt == n and one_cluster(m)[0].gs == 2 * G_T + rev and len(m["tasks"]) == 1))  # fmt: skip
    return out


# ---- B. where a run is cut and how wide its band is ----------------------------------------------------------------------------------
STAIRS = {0: [], 1: [1], 2: [1, 1], 33: [32, 1], 34: [32, 2], 97: [32, 32, 32, 1]}  # diagonal range: steps of at most KP_DIAG_GAP
WIDTH_OF_RANGE = {0: 16, 1: 16, 2: 64, 33: 64, 34: 128, 97: 128}


def stairs(steps, seed, at=1000, n=120, reverse=False, left=100, right=100) -> np.ndarray:
    g = genes()[G_T]
    core = staircase(G_T, at, [n] * (len(steps) + 1), steps, seed)
    end = at + n * (len(steps) + 1) + sum(-s for s in steps if s < 0)
    c = guarded(core, g[at - 1], g[end], seed, left, right)
    return revcomp(c) if reverse else c


def cut_cases() -> list[Case]:
    out = []
    shape = lambda m: [(c.spread, c.width) for c in m["cl"] if c.provisional]  # noqa: E731
    widths = lambda m: sorted(int(w) for w in m["tasks"]["width"])  # noqa: E731
    out.append(case("jump_32: a jump of KP_DIAG_GAP between two provisional halves: one task of 64 diagonals", [stairs([GAP], [20, 32], n=200)], G_T,
                    lambda m: shape(m) == [(GAP, 64)] and widths(m) == [64], True))
    out.append(case("jump_33: a jump of KP_DIAG_GAP + 1: two tasks of 16 diagonals", [stairs([GAP + 1], [20, 33], n=200)], G_T,
                    lambda m: shape(m) == [(0, 16), (0, 16)] and widths(m) == [16, 16], True))
    for rng_, steps in STAIRS.items():
        for rev in (False, True):
            w = WIDTH_OF_RANGE[rng_]
            out.append(case(f"range_{rng_}{'-' if rev else '+'}: a diagonal range of {rng_}: {w} diagonals", [stairs(steps, [21, rng_], reverse=rev)], G_T,
                            lambda m, rng_=rng_, w=w: shape(m) == [(rng_, w)] and widths(m) == [w] and int(m["tasks"][0]["lo"]) == m["cl"][0].lo, True))
    out.append(case("spread_97: a run over KP_MAX_SPREAD diagonals stays one cluster", [stairs([32, 32, 32, 1], [22, 97])], G_T, lambda m: shape(m) == [(SPREAD, 128)], True))
    out.append(case("spread_98: one diagonal more: the greedy soft cut", [stairs([32, 32, 32, 2], [22, 98])], G_T, lambda m: shape(m) == [(96, 128), (0, 16)] and len(m["tasks"]) == 2, True))
    out.append(case("spread_twice: a run over 256 diagonals is cut twice", [stairs([32] * 8, [22, 256])], G_T, lambda m: shape(m) == [(96, 128), (96, 128), (0, 16)] and len(m["tasks"]) == 3, True))
    return out


def split_copy(x: int, seed) -> tuple[np.ndarray, np.ndarray]:
    """A whole copy of G_S cut after x bases: (flank + G_S[:x], G_S[x:] + flank), the first a multiple of 64 bases long, so the
    second follows it without a gap in the padded space of an assembly and of a batch: the diagonal is the same on both sides."""
    g = genes()[G_S]
    left = 256 + (-x) % 64
    return np.concatenate([flank([seed, 1], left), g[:x]]), np.concatenate([g[x:], flank([seed, 2], 200)])


SPLITS = (700, GENE_LEN[G_S] - 15, GENE_LEN[G_S] - 14)


def boundary_cases() -> list[Case]:
    out = []
    for x in SPLITS:
        a, b = split_copy(x, [23, x])

        def per_contig(m, x=x):
            """the hits are per contig and end at the boundary; the clusters share their diagonal"""
            first = [hh for hh in m["hits"] if hh["contig"] == 0]
            return len(first) == 1 and first[0]["q_end"] == x and first[0]["t_end"] == len(split_copy(x, [23, x])[0]) and len({c.d0 for c in m["cl"]} | {c.dmax for c in m["cl"]}) == 1

        def cut_between(ms, x=x):
            """no padding behind the first assembly's last contig; the copy's diagonal, taken from each assembly's own start, is
            the same on both sides once the second is laid behind the first; the hits end and begin at the boundary"""
            a, b = ms
            pa = a["pa"]
            flush = int(pa.ctg_start[1]) + int(pa.ctg_len[1]) == pa.padded_len
            diags = {c.d0 for c in a["cl"]} | {c.dmax for c in a["cl"]} | {c.d0 + pa.padded_len for c in b["cl"]} | {c.dmax + pa.padded_len for c in b["cl"]}
            return (flush and len(diags) == 1 and len(a["hits"]) == 1 and a["hits"][0]["q_end"] == x and a["hits"][0]["t_end"] == pa.ctg_len[1]
                    and all(h["q_start"] >= x and h["t_start"] == 0 and h["contig"] == 0 for h in b["hits"]) and len(b["hits"]) == (x == SPLITS[0]))

        out.append(case(f"contig_cut_{x}: a whole copy of a gene, a contig boundary after {x} of its {GENE_LEN[G_S]} bases", [a, b], G_S, per_contig, True))
        out.append(Case(f"assembly_cut_{x}: the same copy, cut between the last contig of an assembly and the first of the next",
                        (asm_of(f"assembly_cut_{x}_a", [flank([24, x], 500), a]), asm_of(f"assembly_cut_{x}_b", [b, flank([25, x], 500)])), G_S, cut_between, True))
    return out


# ---- E. shapes of the packed fill ----------------------------------------------------------------------------------------------------
HEAD = {16: ([], []), 64: ([30], [2]), 128: ([30, 30], [32, 2])}  # fragments and steps in front of the last fragment, by band width


def off_end(width: int, a: int, x: int, left: int, seed=30, reverse: bool = False, gene: int = G_T) -> np.ndarray:
    """A contig that ENDS with x bases of the gene's copy from base a on (in front of them the staircase that makes the band
    ``width`` diagonals wide, in front of that ``left`` random bases): the task's last row is set by the contig's end."""
    g = revcomp(genes()[gene]) if reverse else genes()[gene]
    lengths, steps = HEAD[width]
    c = np.concatenate([flank([seed, width, a, x, left], left), staircase(gene, a, [*lengths, x], steps, [seed, width, a, x], rc=reverse)])
    if left and a:
        c[left - 1] = other_base(g[a - 1])
    return c


def off_start(width: int, s: int, n: int, seed=31) -> np.ndarray:
    """A contig that STARTS with base s of the gene's copy: the task's first row is a multiple of 8 near s."""
    lengths, steps = HEAD[width]
    g = genes()[G_T]
    core = staircase(G_T, s, [*lengths, n], steps, [seed, width, s, n])
    right = flank([seed, width, s], 100)
    right[0] = other_base(g[s + sum(lengths) + n])
    return np.concatenate([core, right])


# (a, x, left) of off_end by (width, steps), steps = rows + lanes - 1: found with the oracle
STEP_SHAPES: dict[tuple[int, int], tuple[int, int, int]] = {}
STEP_SHAPES.update({(16, 64): (200, 46, 0), (16, 65): (200, 47, 0), (16, 72): (0, 62, 0), (16, 73): (0, 63, 0), (16, 120): (0, 110, 0), (16, 121): (0, 111, 0),
                    (64, 120): (0, 43, 0), (64, 121): (0, 44, 0), (64, 128): (0, 51, 0), (64, 129): (0, 52, 0), (64, 136): (0, 59, 0), (64, 137): (0, 60, 0),
                    (128, 200): (0, 29, 0), (128, 201): (0, 30, 0), (128, 248): (0, 77, 0), (128, 249): (0, 78, 0), (128, 256): (0, 85, 0), (128, 257): (0, 86, 0)})  # fmt: skip
STEP_SHAPES_REV = {(16, 64): (8, 46, 0), (16, 65): (8, 47, 0)}  # (where the reverse strand's seeds ask for another piece of the gene)
CHUNK_RESIDUES = (0, 1, 8, 9, 56, 57)  # steps mod CH: a full last chunk, one step, one piece of 8 steps, a step more, seven pieces, a step more
OFF_START = {16: (0, 20, 1000), 64: (0, 44, 1000), 128: (0, 92, 1000)}  # first gene base of off_start for r_lo = 0, 8 and a larger one


def _only_task(m, width):
    return len(m["tasks"]) == 1 and int(m["tasks"][0]["width"]) == width and len(m["cl"]) == 1


def shape_cases() -> list[Case]:
    out = []
    for (w, steps), (a, x, left) in STEP_SHAPES.items():
        for rev in (False, True):
            out.append(case(f"steps_{w}_{steps}{'-' if rev else '+'}: {w} diagonals, {steps} steps = {steps // C['CH']} chunks and {steps % C['CH']} steps", [off_end(w, *(STEP_SHAPES_REV.get((w, steps), (a, x, left)) if rev else (a, x, left)), reverse=rev)], G_T,
                            lambda m, w=w, steps=steps: _only_task(m, w) and m["steps"] == [steps], not (w == 16 and steps < 72)))  # fmt: skip
    for w, starts in OFF_START.items():
        for s, want in zip(starts, (lambda r: r == 0, lambda r: r == 8, lambda r: r > 8 and r % 8 == 0)):
            out.append(case(f"r_lo_{w}_{s}: {w} diagonals, the copy runs off the contig's start at gene base {s}", [off_start(w, s, 150)], G_T,
                            lambda m, w=w, want=want: _only_task(m, w) and want(m["rows"][0][0]), True))
    tiny = genes()[G_T][:K + 2]
    for w in (64, 128):
        a, x, left = (0, 29, 0)
        out.append(case(f"short_contig_{w}: a contig shorter than its band of {w} diagonals, beside one of KP_K + 2 bases", [tiny, off_end(w, a, x, left), tiny], G_T,
                        lambda m, w=w: _only_task(m, w) and int(m["pa"].ctg_len[1]) < w and int(m["pa"].ctg_len[0]) == K + 2, True))
    # contig starts are multiples of 32 in the padded space: the copy starts at every residue mod 16 behind them
    g = genes()[G_S]
    ctgs = [np.concatenate([flank([32, r], r), g[80 * r : 80 * r + 90], flank([33, r], 40 + r)]) for r in range(16)]
    out.append(case("residues: sixteen copies that start 0..15 bases behind a contig start", ctgs, G_S,
                    lambda m: [c.d0 + 80 * c.contig - int(m["pa"].ctg_start[c.contig]) for c in sorted(m["cl"], key=lambda c: c.contig) if c.provisional] == list(range(16)) and len(m["tasks"]) == 16, True))
    return out


def first_and_last_base() -> Case:
    """The gene's copy from base 0 of the batch's first assembly, and up to the last base of its last assembly (kept first and
    last by the GPU module): the fill's window words before the first and behind the last word of the batch."""
    g = genes()[G_T]
    first = asm_of("batch_first_base", [np.concatenate([g[:300], flank([34], 84)])])  # 384 bases: the padded space ends with the contig
    last = asm_of("batch_last_base", [np.concatenate([flank([35], 84), g[-300:]])])
    return Case("first_and_last_base: a copy from base 0 of the batch and one up to its last base", (first, last), G_T,
                lambda ms: ms[0]["hits"][0]["t_start"] == 0 and ms[1]["hits"][0]["t_end"] == ms[1]["pa"].ctg_len[-1] and ms[1]["pa"].padded_len == ms[1]["pa"].n_bases
                and [len(m["tasks"]) for m in ms] == [1, 1], True)


def stage_gene_piece(k: int, step: int, n: int) -> tuple[int, int]:
    return G_STAGE + k % N_STAGE, 20 + step * (k // N_STAGE)


def unit(width: int, k: int, n: int = 60, step: int = 80, reverse: bool = False) -> np.ndarray:
    """Piece k of the stage genes -- at most one copy of any base of them per k --: one provisional cluster of ``width``
    diagonals, with a spacer behind it."""
    gene, at = stage_gene_piece(k, step, n)
    if width == 16:
        core = genes()[gene][at : at + n]
    elif width == 64:
        core = staircase(gene, at, [n // 2, n - n // 2], [2], [40, k])
    else:
        core = staircase(gene, at, [26, 26, max(n - 52, 26)], [32, 2], [40, k])
    c = np.concatenate([core, flank([41, k], 20)])
    return revcomp(c) if reverse else c


def population_batches() -> list[Case]:
    """Batches whose classes hold 1, 2, 2G - 1, 2G and 2G + 1 tasks, G = 64 / lanes groups a wave: the absent partner of a pair,
    an absent pair, the second quad."""
    out, k = [], 0
    for which, name in ((lambda g: 1, "1"), (lambda g: 2, "2"), (lambda g: 2 * g - 1, "2G-1"), (lambda g: 2 * g, "2G"), (lambda g: 2 * g + 1, "2G+1")):
        want = {w: which(64 // p) for w, p in LANES.items()}
        asms = []
        for a in range(3):  # the tasks of a class come from three assemblies
            ctgs = []
            for w, n in want.items():
                for i in range(a, n, 3):
                    ctgs.append(np.concatenate([flank([42, k], 30), unit(w, k, 80, 100, reverse=k % 2 == 1)]))
                    k += 1
            asms.append(asm_of(f"population_{name}_{a}", ctgs or [flank([43, a], 200)]))
        out.append(Case(f"population_{name}: {want} tasks batch-wide", tuple(asms), None,
                        lambda ms, want=want: {w: sum(int((m["tasks"]["width"] == w).sum()) for m in ms) for w in want} == want, True))
    return out


def pair_cases() -> list[Case]:
    """A short and a 3 000-row task alone in their class: the pair runs for the longer one's steps."""
    out = []
    for w, short in ((16, (200, 46, 0)), (64, (0, 43, 0)), (128, (0, 29, 0))):
        asm = asm_of(f"pair_{w}", [off_end(w, *short), off_end(w, 0, 3010 - sum(HEAD[w][0]), 0, seed=36)])
        out.append(Case(f"pair_{w}: a task of a few dozen rows and one of 3 000 alone in the class of {w} diagonals", (asm,), G_T,
                        lambda m, w=w: sorted(b - a for a, b in m["rows"])[0] < 200 and sorted(b - a for a, b in m["rows"])[1] >= 3000 and [int(x) for x in m["tasks"]["width"]] == [w, w], True))
    return out


# ---- D. stage, tile and order ----------------------------------------------------------------------------------------------------------
def order_cases() -> list[Case]:
    """Rows on both sides of a bucket edge of the task order (32 rows a bucket), of its clamp (63 buckets: 2016 rows; 2047, 2048
    and 2100 rows share the first bucket), and a gene on either side of KP_FILL16_MAX_GENE_LEN in one class list."""
    out = []
    rows_of = lambda m: sorted(b - a for a, b in m["rows"])  # noqa: E731
    for rows, (a, x, left) in ((63, (200, 48, 0)), (64, (200, 49, 0)), (2015, (0, 2008, 0)), (2016, (0, 2009, 0)), (2047, (0, 2040, 0)), (2048, (0, 2041, 0)), (2100, (0, 2093, 0))):
        out.append(case(f"rows_{rows}: a task of {rows} rows (bucket {length_bucket(rows)})", [off_end(16, a, x, left, seed=37)], G_T, lambda m, rows=rows: rows_of(m) == [rows], True))
    both = asm_of("fill16_edge", [off_end(16, 0, 300, 50, seed=38, gene=G_F16), off_end(16, 0, 300, 50, seed=39, gene=G_F16P), off_end(16, 0, 300, 50, seed=44)])
    out.append(Case("fill16_edge: a gene of KP_FILL16_MAX_GENE_LEN bases (packed fill) and one a base longer (32-bit fill) in one class list", (both,), None,
                    lambda m: sorted(int(x) >> 1 for x in m["tasks"]["gs"]) == [G_T, G_F16, G_F16P] and set(m["tasks"]["width"].tolist()) == {16} and (m["sw"][:, 0] >= MIN_DP).all(), True))
    return out


def units_assembly(name: str, ks, widths=lambda k: 16, n=lambda k: 60, step: int = 80, more=()) -> GenomeAssembly:
    seed = [45, len(name), *name.encode()[-6:]]
    return asm_of(name, [np.concatenate([flank(seed, 50)] + [unit(widths(k), k, n(k), step, reverse=k % 3 == 1) for k in ks]), *more])


def tile_batches() -> list[Case]:
    """Class lists of KP_CS_TILE - 1, KP_CS_TILE, KP_CS_TILE + 1 and 2 KP_CS_TILE + 1 provisional tasks of 16 diagonals batch-wide,
    from three assemblies, every anchor count from KP_MIN_ANCHORS to beyond KP_CHAIN_DP_MAX mixed, one of them rejected by its chain."""
    out = []
    rejected = [_two(2213, 26, 20, 1, 3)]
    for total in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        few = [count_fragment(n, reverse=n % 2 == 0) for n in (3, 4, 5)]  # the low bins of the counting sort, inside the tile
        n_units = total - len(rejected) - len(few)
        cut = [0, n_units // 3, 2 * n_units // 3, n_units]
        asms = [units_assembly(f"tile_{total}_{a}", range(cut[a], cut[a + 1]), n=lambda k: 60 + 25 * (k % 7), step=300, more=rejected if a == 1 else (few if a == 0 else ())) for a in range(3)]
        out.append(Case(f"tile_{total}: {total} provisional tasks of 16 diagonals batch-wide", tuple(asms), None,
                        lambda ms, total=total: sum(sum(c.provisional and c.width == 16 for c in m["all"]) for m in ms) == total
                        and sum(int((m["tasks"]["width"] == 16).sum()) for m in ms) == total - 1 and set(range(MIN_ANCHORS, DP_MAX + 3)) <= {c.cnt for m in ms for c in m["all"] if c.provisional}))  # fmt: skip
    return out


STAGE_UNITS = {STAGE - 1: (2758, False), STAGE: (2537, False), STAGE + 1: (2760, False), 2 * (STAGE + 1): (5048, True)}  # staged count of one block -> (units of the assembly, classes mixed): found with the oracle


def stage_assembly(n_units: int, mixed: bool = False) -> GenomeAssembly:
    widths = (lambda k: 128 if k % 25 == 7 else (64 if k % 10 == 3 else 16)) if mixed else (lambda k: 16)
    return units_assembly(f"stage_{n_units}{'_mixed' if mixed else ''}", range(n_units), widths, n=lambda k: 78 if widths(k) == 128 else 60)


# ---- E, continued: scores at the cut-off and ties of the best cell -------------------------------------------------------------------------
def broken_copy(a: int, l1: int, kind: str, l2: int, rc: bool = False, seed=50, tail: int = 0) -> np.ndarray:
    """l1 bases of G_T from base a, one column that is a substitution ('X'), an N ('N') or a base the contig lacks ('D'), then
    l2 bases more -- and, with ``tail``, an N column and ``tail`` bases behind them; the flanks differ from the gene where they
    touch the copy.  ``rc``: the same of the gene's reverse complement, so that the copy lies on strand -1 and its rows run
    the same way."""
    g = revcomp(genes()[G_T]) if rc else genes()[G_T]
    mid = {"X": [other_base(g[a + l1])], "N": [ord("N")], "D": [], "I": [next(int(b) for b in BASES if b not in (g[a + l1 - 1], g[a + l1]))]}[kind]
    end = a + l1 + (kind != "I") + l2  # ('I': a base the gene lacks -- nothing of the gene is replaced)
    core = np.concatenate([g[a : a + l1], np.array(mid, np.uint8), g[a + l1 + (kind != "I") : end]])
    if tail:
        core = np.concatenate([core, [ord("N")], g[end + 1 : end + 1 + tail]]).astype(np.uint8)
        end += 1 + tail
    return guarded(core, g[a - 1], g[end], [seed, a, l1, l2])


def local_best_cells(q: np.ndarray, t: np.ndarray) -> tuple[int, list[tuple[int, int]]]:
    """Smith-Waterman-Gotoh of kp_spec.h (match 2, mismatch -4, N -1, gap 4 + 2 n) over the whole rectangle, in plain Python:
    the best score and every cell that holds it, in (row, column) order."""
    n, m = len(q), len(t)
    neg = -(1 << 29)
    H = [[0] * (m + 1) for _ in range(n + 1)]
    F = [neg] * (m + 1)
    best, cells = 0, []
    for i in range(1, n + 1):
        e = neg
        for j in range(1, m + 1):
            s = -1 if q[i - 1] == ord("N") or t[j - 1] == ord("N") else (2 if q[i - 1] == t[j - 1] else -4)
            e = max(H[i][j - 1] - 6, e - 2)
            F[j] = max(H[i - 1][j] - 6, F[j] - 2)
            h = max(0, H[i - 1][j - 1] + s, e, F[j])
            H[i][j] = h
            if h > best:
                best, cells = h, [(i - 1, j - 1)]
            elif h == best and h > 0:
                cells.append((i - 1, j - 1))
    return best, cells


# best score -> (a, l1, kind, l2, tail): found with the oracle.  An N column between 40 matching bases (79 = 2 * 40 - 1) leaves two clean
# stretches of 40 bases in all: an exhaustive search of G_T on both strands found no three seeds there that cover 40 bases and
# chain to 40.  79 is therefore 42 matches, a substitution and an N column: a copy like score_78's with an N and one more base.
SCORE_SHAPES = {78: (3851, 25, "X", 16, 0), 79: (1802, 25, "X", 16, 1), 80: (411, 27, "X", 15, 0)}
TIE_AT, TIE_LEN = 1500, 120


def tie_cases() -> list[Case]:
    """A copy of 120 bases whose best score is reached again (or beaten) k bases before its end: the reported cell is the
    FIRST maximum in (row, column) order."""
    out = []
    for rc in (False, True):
        s = "-" if rc else "+"
        g = revcomp(genes()[G_T]) if rc else genes()[G_T]
        for name, kind, k, tie in (("tie_mismatch_2", "X", 2, True), ("tie_mismatch_3", "X", 3, False), ("tie_gap_3", "D", 3, True), ("tie_lanes_3", "I", 3, True)):
            l1 = TIE_LEN - 1 - k
            at = next(a for a in range(TIE_AT, TIE_AT + 50) if len({g[a + l1 - 1], g[a + l1], g[a + l1 + 1]}) == 3)  # (the gap cannot slide)
            contig = broken_copy(at, l1, kind, k, rc)

            def holds(m, l1=l1, tie=tie, at=at, contig=contig, g=g, kind=kind):
                """the oracle reports the first maximum; a plain fill of the copy's surroundings shows the second one"""
                best, cells = local_best_cells(g[at - 5 : at + TIE_LEN + 5], contig[90:-90])
                ok = (len(m["tasks"]) == 1 and m["sw"][0][0] == best == 2 * l1 + (0 if tie else 2) and m["sw"][0][2] == at + (l1 if tie else TIE_LEN)
                      and len(cells) >= (2 if tie else 1) and cells[0][0] + at - 5 + 1 == m["sw"][0][2])
                if ok and kind == "I":  # the two cells lie on neighbouring diagonals that two LANES of the packed fill hold (four diagonals a lane)
                    d1 = int(m["sw"][0][4] - m["sw"][0][2]) - int(m["tasks"][0]["lo"])
                    ok = cells[1][1] - cells[1][0] == cells[0][1] - cells[0][0] + 1 and d1 // 4 + 1 == (d1 + 1) // 4
                return ok

            out.append(case(f"{name}{s}: a {'substitution' if kind == 'X' else ('base the gene lacks' if kind == 'I' else 'one-base gap')} {k} bases before the copy's end on strand {s}: the earlier maximum is {'met again' if tie else 'beaten'}",
                            [contig], G_T, holds, True))
        # the earlier maximum in the HIGHER lane: tie_gap_3 behind a 2-base insertion 40 bases into the copy.  The anchors before the
        # insertion lie on diagonal d - 2, so the band has 64 diagonals from lo = d - 32: the earlier maximum's diagonal d is the
        # first of lane 8, the later one's, d - 1, the last of lane 7 -- a fill that took the lowest lane on ties would report the later.
        l1, k, pre = TIE_LEN - 4, 3, 40
        at = next(a for a in range(TIE_AT + 60, TIE_AT + 110) if len({g[a + l1 - 1], g[a + l1], g[a + l1 + 1]}) == 3)
        ins = np.array([other_base(g[at]), other_base(g[at - 1], 2)], np.uint8)
        contig = guarded(np.concatenate([g[at - pre : at], ins, g[at : at + l1], g[at + l1 + 1 : at + l1 + 1 + k]]), g[at - pre - 1], g[at + l1 + 1 + k], [52, rc])

        def holds_up(m, at=at, contig=contig, g=g, l1=l1, pre=pre):
            best, cells = local_best_cells(g[at - pre - 5 : at + TIE_LEN + 5], contig[90:-90])
            if not (len(m["tasks"]) == 1 and m["tasks"][0]["width"] == 64 and m["sw"][0][0] == best == 2 * (pre + l1) - 8 and m["sw"][0][2] == at + l1
                    and len(cells) >= 2 and cells[0][0] + at - pre - 5 + 1 == m["sw"][0][2]):
                return False
            d1 = int(m["sw"][0][4] - m["sw"][0][2]) - int(m["tasks"][0]["lo"])  # band offset of the earlier maximum's diagonal
            return cells[1][1] - cells[1][0] == cells[0][1] - cells[0][0] - 1 and cells[1][0] > cells[0][0] and d1 // 4 == (d1 - 1) // 4 + 1

        out.append(case(f"tie_lanes_up_3{s}: a one-base gap 3 bases before the end of a copy with a 2-base insertion, strand {s}: the earlier maximum lies in the higher lane",
                        [contig], G_T, holds_up, True))
    return out


def score_cases() -> list[Case]:
    out = []
    for score, (a, l1, kind, l2, tail) in sorted(SCORE_SHAPES.items()):
        out.append(case(f"score_{score}: a best cell of {score} ({l1} bases, a substitution, {l2} bases{', an N, a base' if tail else ''})", [broken_copy(a, l1, kind, l2, seed=51, tail=tail)], G_T,
                        lambda m, score=score: len(m["tasks"]) == 1 and m["sw"][0][0] == score and len(m["hits"]) == (score >= MIN_DP), score >= MIN_DP))
    return out


# ---- C. rounds of 64 anchors ---------------------------------------------------------------------------------------------------------------
class _Builder(OU.Builder):
    def planted_count(self, gene: int, p: int) -> int:
        """(a prefix that shares a 15-mer with another of this database's 486 genes is never chosen)"""
        if (gene, p) not in self._count:
            a = self.anchors(asm_of("count", [self.g[gene][:p]]))
            self._count[gene, p] = len(a) if (OU.gene_of(a) == gene).all() else 10**9
        return self._count[gene, p]


def builder(odb) -> OU.Builder:
    """tests/occ_cut_util.py's builder of planted filler genes (contigs of their own that add an exact number of anchors
    before or behind the genes under test), on this database."""
    B = _Builder(odb)
    B.g = genes()
    return B


FILL, TAIL = range(0, N_FILL), range(G_TAIL, G_TAIL + N_TAIL)


FAR = 2 * C["KP_JOIN_BW"]
STRAY_GAPS = ((JOIN_BW, JOIN_BW), (JOIN_BW + 1, JOIN_BW + 1), (JOIN_BW, JOIN_BW + 1), (JOIN_BW + 1, JOIN_BW), (JOIN_BW, FAR), (FAR, JOIN_BW), (JOIN_BW + 1, FAR), (FAR, JOIN_BW + 1))


STRAY_SALT = {(JOIN_BW + 1, JOIN_BW): 1}


def stray_between(before: int, after: int) -> np.ndarray:
    """21 bases of G_T (a stray run of two anchors) ``before`` diagonals above the run before it and ``after`` below the run
    after it: kp_chain_kernel visits a stray run that is within KP_JOIN_BW of EITHER neighbour, by two clauses of their own."""
    g = genes()[G_T]
    salt = STRAY_SALT.get((before, after), 0)  # (flanks that leave the 21 bases two anchors at most)
    f = lambda i, n: flank([60, before, after, i, salt], n)  # noqa: E731
    return np.concatenate([flank([61, before, after], 200), g[200:700], f(0, before), g[700:721], f(1, after), g[721:1200], flank([62, before, after], 200)])


def is_head(m) -> np.ndarray:
    """Which anchors of the sorted list kp_chain_kernel's lanes flag as heads: the first, and every one whose gene/strand or
    contig differs from its predecessor's or whose diagonal lies more than KP_DIAG_GAP above it."""
    gs, d, q = decode(m["keys"])
    ctg = np.searchsorted(np.asarray(m["pa"].ctg_start, np.int64), d + q, "right") - 1
    head = np.ones(len(gs), bool)
    head[1:] = (gs[1:] != gs[:-1]) | (ctg[1:] != ctg[:-1]) | (d[1:] - d[:-1] > GAP)
    return head


def heads_case(B: OU.Builder) -> Case:
    """A round of 64 heads: 20 bases of each of 300 stage genes between flanks of 30 random bases, kept where the oracle finds
    exactly one anchor in the piece: one run of one anchor per gene/strand, 128 and more of them in a row, so some round
    holds nothing else."""
    parts = [flank([67], 60)]
    kept = 0
    for k in range(G_STAGE, G_STAGE + 300):
        g = genes()[k]
        piece = np.concatenate([flank([69, k], 30), g[400:420], flank([68, k], 30)])
        got = B.anchors(asm_of("one", [piece]))
        if len(got) == 1 and int(got[0] >> np.uint64(47)) == k:
            parts.append(piece)
            kept += 1
    assert kept >= 150, kept
    return case("heads_64: a round of 64 anchors that are all heads, each a run of one anchor", [np.concatenate(parts)], None,
                lambda m: any(is_head(m)[a:b].all() for a, b in kernel_rounds(m)) and not m["tasks"].size)


def kernel_pos(m, i: int) -> tuple[int, int, int]:
    """(wave, round, lane) at which kp_chain_kernel meets anchor i: a wave's rounds of 64 count from where its walk starts (the
    skip-ahead position of its slice), not from the list's first anchor."""
    owner, ranges = owner_waves(m["keys"])
    w = int(owner[i])
    return w, (i - ranges[w][0]) // 64, (i - ranges[w][0]) % 64


def kernel_rounds(m) -> list[tuple[int, int]]:
    """[a, b) of every whole round of 64 anchors that some wave of kp_chain_kernel walks."""
    return [(a, a + 64) for s, e in owner_waves(m["keys"])[1] for a in range(s, e - 63, 64)]


def round_cases(B: OU.Builder) -> list[Case]:
    """List positions against the rounds of 64 anchors and the wave slices of kp_chain_kernel.  tests/occ_cut_util.py's group A
    (list_cases) already walks a stretch's start and end through a round and a slice for the identical round logic of
    kp_occ_cut_kernel and kp_chain_kernel; here: what only the CLUSTER logic tells apart."""
    out = []
    three, two = count_fragment(MIN_ANCHORS), _fragment(G_T, 100, 24, [1, 100, 24])
    for lane in (61, 62, 63):
        out.append(case(f"head_lane_{lane}: a run of exactly KP_MIN_ANCHORS anchors whose head sits on lane {lane}: {64 - lane} + {lane - 61} over two rounds",
                        [*B.planted(FILL, lane), three], G_T,  # (fewer than 64 anchors before it: wave 0 walks the run, also past its slice's end)
                        lambda m, lane=lane: [kernel_pos(m, m["first"] + k) for k in range(3)] == [(0, (lane + k) // 64, (lane + k) % 64) for k in range(3)]
                        and m["cl"][0].cnt == MIN_ANCHORS and len(m["tasks"]) == 1))
    s = _fragment(G_S, 300, 200, [63])
    out.append(case("stray_lane_63: a two-anchor stray that ends on lane 63, an unrelated head on lane 0", [*B.planted(FILL, 62), two, s], None,
                    lambda m: [(c.gs >> 1, kernel_pos(m, c.first), kernel_pos(m, c.first + c.cnt - 1)[1:]) for c in m["all"] if c.gs >> 1 in (G_T, G_S)][:2]
                    == [(G_T, (0, 0, 62), (0, 63)), (G_S, (1, 0, 0), kernel_pos(m, 64 + [c for c in m["all"] if c.gs >> 1 == G_S][0].cnt - 1)[1:])]
                    and [c for c in m["all"] if c.gs >> 1 == G_T][0].cnt == 2))
    for before, after in STRAY_GAPS:
        out.append(case(f"stray_bw_{before}_{after}: a stray run {before} diagonals from the run before it and {after} from the run after it", [stray_between(before, after)], G_T,
                        lambda m, before=before, after=after: [c.cnt for c in m["cl"]][1] in (1, 2) and len(m["cl"]) == 3 and m["cl"][1].d0 - m["cl"][0].dmax == before
                        and m["cl"][2].d0 - m["cl"][1].dmax == after, True))  # fmt: skip
    whole = in_flanks(genes()[G_S], [64])
    out.append(case("headless_round: a round of 64 anchors that is all one run", [*B.planted(FILL, 10), whole], G_S,
                    lambda m: any(c.first < a and b <= c.first + c.cnt for c in m["cl"] for a, b in kernel_rounds(m)), True))
    for n, pools in ((64, (FILL,)), (65, (FILL,)), (SLICES * 64 + 1, (FILL, TAIL))):
        first = min(n, 700)
        contigs = [*B.planted(pools[0], first), *(B.planted(pools[1], n - first) if n > first else [])]
        out.append(case(f"list_{n}: a list of exactly {n} anchors", contigs, None, lambda m, n=n: m["n"] == n and slice_per(n) == (64 if n <= SLICES * 64 else 128)))
    for gap in (JOIN_BW, JOIN_BW + 1):
        out.append(case(f"stray_after_only_{gap}: a stray run with no run before it, {gap} diagonals below the first of fifteen small runs and a pair", [stray_opens_sequence(gap, 15)], G_T,
                        lambda m, gap=gap: m["cl"][0].cnt in (1, 2) and m["cl"][1].d0 - m["cl"][0].dmax == gap and len(m["cl"]) == 18
                        and all(b.d0 - a.dmax <= JOIN_BW for a, b in zip(m["cl"][1:], m["cl"][2:])) and len(m["hits"]) == (1 if gap == JOIN_BW else 2), True))  # fmt: skip
    # the soft cut on a round's FIRST anchor: the cluster carried over from the round before is flushed by merge(0, first, ...) at u == 0
    cut = stairs([32, 32, 32, 2], [22, 98])
    rel = clusters(B.anchors(asm_of("rel", [cut])), asm_of("rel", [cut]).packed())
    assert len(rel) == 2, rel
    out.append(case("spread_98_lane_0: the soft cut falls on the first anchor of a round", [*B.planted(FILL, (-rel[1].first) % 64), cut], G_T,  # (the run starts in wave 0's slice: that wave walks all of it)
                    lambda m: [(c.spread, c.width) for c in m["cl"]] == [(96, 128), (0, 16)] and kernel_pos(m, m["cl"][1].first)[0::2] == (0, 0)
                    and kernel_pos(m, m["cl"][0].first)[:2] < kernel_pos(m, m["cl"][1].first)[:2] and kernel_pos(m, m["cl"][0].first)[0] == 0 and len(m["tasks"]) == 2, True))
    out.append(heads_case(B))
    big = in_flanks(genes()[G_T], [65])
    out.append(case("three_slices: one gene/strand covers three whole slices: two waves skip ahead and find nothing", [*B.planted(FILL, 300), big, *B.planted(TAIL, 500)], G_T,
                    lambda m: sum(a == b and w * slice_per(m["n"]) < m["n"] for w, (a, b) in enumerate(owner_waves(m["keys"])[1])) >= 2, True))
    return out


def stage_cases() -> list[Case]:
    """One block's staged count at KP_CHAIN_STAGE - 1, KP_CHAIN_STAGE, KP_CHAIN_STAGE + 1 and, three classes mixed, twice that:
    every piece a lone provisional cluster, every piece distinct, at most ten pieces of any gene/strand in an assembly (the
    CPU module asserts it, and that the occurrence cut drops nothing)."""
    out = []
    for staged, (n_units, mixed) in STAGE_UNITS.items():
        out.append(Case(f"stage_{staged}: one block of kp_chain_kernel stages {staged} tasks{' of three classes' if mixed else ''}", (stage_assembly(n_units, mixed),), None,
                        lambda m, staged=staged, mixed=mixed: staged in staged_per_block(m["keys"], m["pa"]) and len({c.width for c in m["all"] if c.provisional}) == (3 if mixed else 1), True))
    return out


# ---- everything, built once a session ----------------------------------------------------------------------------------------------
_BUILT: dict = {}
GROUPS = ("A", "A_counts", "B", "B_cuts", "C", "D_order", "D_tile", "D_stage", "E_shapes", "E_batches", "E_scores")


def built(oracle) -> dict:
    """{"codes", "off", "odb", "groups": {name: [Case]}}: the database and every case, built once per process."""
    if not _BUILT:
        from kaptive_amd.pack import pack_sequences_flat

        codes, off = pack_sequences_flat(gene_sequences())
        odb = oracle.OracleDB(codes, off)
        groups = {"A": which_cases(), "A_counts": count_cases(), "B": cut_cases(), "B_cuts": boundary_cases(), "C": round_cases(builder(odb)),
                  "D_order": order_cases(), "D_tile": tile_batches(), "D_stage": stage_cases(), "E_shapes": [*shape_cases(), *pair_cases()],
                  "E_batches": [first_and_last_base(), *population_batches()], "E_scores": [*score_cases(), *tie_cases()]}  # fmt: skip
        assert tuple(groups) == GROUPS
        _BUILT.update(codes=codes, off=off, odb=odb, groups=groups)
    return _BUILT


_MEASURED: dict = {}


def measured(odb, c: Case):
    """measure() of every assembly of a case, once per process: one dict for a case of one assembly, a list otherwise."""
    if c.label not in _MEASURED:
        ms = [measure(odb, a, c.gene) for a in c.asms]
        _MEASURED[c.label] = ms[0] if len(ms) == 1 else ms
    return _MEASURED[c.label]


def stray_opens_sequence(gap: int, n_decoys: int) -> np.ndarray:
    """A stray run with NO run before it, ``gap`` diagonals below the first of ``n_decoys`` 30-base fragments of G_T (36 diagonals
    apart, the last 36 below a pair of clusters around a 100-base insertion): linked to the run AFTER it alone.  With fifteen
    fragments (the cases): at KP_JOIN_BW the stray run opens the sequence and the fragments fill it to KP_JOIN_GROUP_MAX, so the
    pair is a sequence of its own and is joined; a diagonal further the stray run is no member, the pair's first cluster is
    member 16 of the fragments' sequence, its second is not, and the pair stays two hits."""
    g = genes()[G_T]
    f = lambda i, n: flank([66, gap, i], n)  # noqa: E731
    parts, pos = [f(0, 200), g[0:600], f(1, 100), g[600:1200]], 1500
    pieces = [(2000 + 60 * i, 30, 200 - 36 * (n_decoys - i)) for i in range(n_decoys)] + [(3900, 21, 200 - 36 * n_decoys - gap)]
    for k, (q, n, diag) in enumerate(pieces):
        t = q + diag
        parts += [f(10 + k, t - pos), g[q : q + n]]
        pos = t + n
    parts.append(f(2, 200))
    return np.concatenate(parts)
