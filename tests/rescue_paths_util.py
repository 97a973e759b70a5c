"""Shared by tests/test_rescue_paths_cpu.py and tests/test_gpu_rescue_paths.py: inputs that walk the row, strip, tie and queue paths
of the rescue fill (kaptive_amd/csrc/kp_rescue.hip) which the shapes of tests/rescue_util.py leave alone.  Every fixture is a `Case`: a
``Database.from_parts`` database, genomes, hand-made hit tables (so the pieces, and with `flank` the windows, are exact) and a list of
expectations -- scenario checks that must hold for the YARDSTICK's records (tests/rescue_util.restate), with the summaries and pieces
of the CPU harness in the one test file and with the device's own in the other.  Nothing here compares a device value.
TEST INFRASTRUCTURE."""

from __future__ import annotations

from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

from kaptive_amd.synth import CODONS, random_dna, random_orf, revcomp
from tests import rescue_util as R

# rows of the frame text a wave takes per turn (KP_RS_LANES: the refill of the LDS ring, the publication of the previous strip's last
# column and lane 63's flush happen every ROW_CHUNK steps) and residues of the ring (two chunks).  kp_rescue.hip: RS_WAVE, RS_RING.
ROW_CHUNK, RING = 64, 128
STRIP = R.STRIP_LIMITS[-1]  # columns of a strip

_BY_AA: dict = {}
for _codon, _aa in sorted(CODONS.items()):
    _BY_AA.setdefault(_aa, []).append(_codon)
RESIDUES = sorted(a for a in _BY_AA if a != "*")


# ---- building blocks -------------------------------------------------------------------------------------------------------------------
def back(protein: str, rng=None) -> np.ndarray:
    """DNA of a residue string: the alphabetically first codon of every residue, or a drawn one."""
    cods = [_BY_AA[a][int(rng.integers(len(_BY_AA[a]))) if rng is not None else 0] for a in protein]
    return np.frombuffer("".join(cods).encode(), np.uint8).copy()


def rand_protein(rng, n: int, exclude: str = "") -> str:
    pool = [a for a in RESIDUES if a not in exclude]
    return "".join(pool[int(i)] for i in rng.integers(len(pool), size=n))


def keep(rng, dna: np.ndarray) -> np.ndarray:
    """Whole codons recoded without a substitution: the same residues."""
    return R.recode(rng, dna, substituted=0.0)


def sharp_tail(rng, gene: np.ndarray, m: int, recoded: np.ndarray | None = None) -> np.ndarray:
    """The last m codons of the gene, recoded, the last five of them (the stop included) with their residues kept: an alignment of it
    ends on the protein's last column."""
    rec = R.recode(rng, gene) if recoded is None else recoded
    return np.concatenate([rec[len(rec) - 3 * m : len(rec) - 15], keep(rng, gene[-15:])])


def genome(name, contigs):
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences

    return GenomeAssembly(name, Sequences.from_records([SeqRecord(f"{name}_{i}", np.ascontiguousarray(c).tobytes()) for i, c in enumerate(contigs)]))


def hit(db, gene: int, contig: int, t_start: int, t_len: int):
    from kaptive_amd import _native

    h = np.zeros(1, _native.HIT_DTYPE)
    L = int(db.genes.lengths[gene])
    h["gene"], h["contig"], h["strand"], h["q_start"], h["q_end"], h["t_start"], h["t_end"] = gene, contig, 1, 0, L, t_start, t_start + t_len
    h["score"], h["matches"], h["block_len"], h["mapq"] = 2 * L, L, L, 60
    return h


def build_db(name: str, loci, seed: int):
    """loci: [(locus name, [gene DNA, ...])]; 60 bases in front, 40 between the genes, all on the forward strand."""
    from kaptive_amd.db import Database

    rng = np.random.default_rng(seed)
    out = []
    for lname, genes in loci:
        parts, feats, pos = [random_dna(rng, 60, 0.5)], [], 60
        for i, g in enumerate(genes):
            parts += [g, random_dna(rng, 40, 0.5)]
            feats.append(dict(start=pos, end=pos + len(g), strand=1, gene=f"{lname.lower()}g{i}", product=f"{lname} {i}"))
            pos += len(g) + 40
        out.append(dict(name=lname, type=lname, extra=False, seq=np.concatenate(parts).tobytes(), genes=feats))
    meta = dict(name=name, keyword=name, genbank=f"{name}.gbk", organism="none", taxon=1, antigen="S", pathway="Wzx/Wzy", version="1",
                id_threshold=82.5, doi=[], owner="kaptive_amd", repo="synthetic", branch="main", contact={}, phenotype_logic={})  # fmt: skip
    return Database.from_parts(meta, out)


def gene_dna(db, g: int) -> np.ndarray:
    """Bases of database gene g (forward-strand genes only)."""
    loc = int(db.gene_locus_indices[g])
    o = int(db.loci.offsets[loc])
    return np.asarray(db.loci.seqs[o + int(db.gene_intervals.starts[g]) : o + int(db.gene_intervals.ends[g])], np.uint8)


@dataclass
class Case:
    """One batch: `tables[a]` is assembly a's hit table (genes ascending), `flank` the rescue_flank it is run with.  `expect`: dicts with
    `asm`, `gene` (database index) and the values the yardstick's record of that gene must show (check_expect)."""

    name: str
    db: object
    flank: int
    genomes: list = field(default_factory=list)
    tables: list = field(default_factory=list)
    expect: list = field(default_factory=list)
    notes: dict = field(default_factory=dict)

    def add(self, name, contigs, hits):
        self.genomes.append(genome(name, contigs))
        self.tables.append(np.concatenate(sorted(hits, key=lambda h: int(h["gene"][0]))))
        return len(self.genomes) - 1

    @property
    def ids(self):
        return [g.id for g in self.genomes]


def framed(rng, window: np.ndarray, flank: int, left: int = 31, right: int = 29):
    """(contig, hit start, hit length): the window between `left` and `right` random bases, and the hit whose piece gives exactly that
    window with `flank`."""
    assert len(window) > 2 * flank
    return np.concatenate([random_dna(rng, left, 0.5), window, random_dna(rng, right, 0.5)]), left + flank, len(window) - 2 * flank


# ---- the scenario checks ----------------------------------------------------------------------------------------------------------------
def end_rows(r, ws: int, we: int) -> tuple[int, int]:
    """(a0, a1): the rows of the frame text the record's stretch covers."""
    f = int(r["frame"])
    if int(r["strand"]) > 0:
        return (int(r["t_start"]) - ws - f) // 3, (int(r["t_end"]) - ws - f) // 3
    return (we - f - int(r["t_end"])) // 3, (we - f - int(r["t_start"])) // 3


def record_of(case, sums, records, off, a: int, gene: int):
    recs = records[int(off[a]) : int(off[a + 1])]
    r = recs[recs["gene"] == gene]
    assert len(r) == 1, f"{case.name}: {case.ids[a]} has {len(r)} records of gene {gene}"
    return r[0]


def window_of(case, packed, pieces, a: int, r) -> tuple[int, int]:
    pc = pieces[a][int(r["piece"])]
    return R.window(int(pc["start"]), int(pc["end"]), int(packed[a].ctg_len[int(pc["contig"])]), case.flank)


def check_expect(case, packed, sums, pieces, records, off):
    """Every expectation of the case on the yardstick's records.  Keys: found, strand, frame, contig, a_len, a1 (last row of the
    stretch), last_row (a1 == a_len), p_end, p_end_gt, crosses (p_start < it < p_end), score, score_min, t_start_rel (t_start - ws)."""
    for e in case.expect:
        a, label = e["asm"], f"{case.name}: {case.ids[e['asm']]} gene {e['gene']}"
        r = record_of(case, sums, records, off, a, e["gene"])
        if e.get("found") is False:
            assert int(r["piece"]) == -1 and int(r["score"]) == 0, (label, r)
            continue
        assert int(r["piece"]) >= 0 and int(r["score"]) > 0, (label, r)
        ws, we = window_of(case, packed, pieces, a, r)
        a0, a1 = end_rows(r, ws, we)
        have = dict(strand=int(r["strand"]), frame=int(r["frame"]), contig=int(r["contig"]), a_len=int(r["a_len"]), a1=a1, p_end=int(r["p_end"]),
                    score=int(r["score"]), t_start_rel=int(r["t_start"]) - ws)  # fmt: skip
        for key, want in e.items():
            if key in have:
                assert have[key] == want, (label, key, have[key], want, r)
        if e.get("last_row"):
            assert a1 == int(r["a_len"]), (label, "the stretch ends on the window's last row", a1, r)
        if "p_end_gt" in e:
            assert int(r["p_end"]) > e["p_end_gt"], (label, r)
        if "crosses" in e:
            assert int(r["p_start"]) < e["crosses"] < int(r["p_end"]), (label, "the stretch crosses the strip boundary", r)
        if "score_min" in e:
            assert int(r["score"]) >= e["score_min"], (label, r)


# ---- 1. rows: the rows DB ---------------------------------------------------------------------------------------------------------------
ROWS_ANCHORS = 3
# residues, the trailing * included: one protein per columns-per-lane class, one of two strips, one of three, and E -- designed: two strips,
# W C W on columns 384 .. 386 and no other W or C -- for frame texts of one to three residues.  D and T end 16 and 32 columns beyond a
# strip boundary: every planted tail is longer, so its stretch passes through the boundary column the strips hand over.
ROWS_PROTEINS = dict(S=100, M=200, W=300, D=400, T=800, E=500)
ROWS_T_TAIL = 50  # residues of T's tail (alone in its window of some 64 residues)
ROWS_GENE = {n: ROWS_ANCHORS + i for i, n in enumerate(ROWS_PROTEINS)}
ROW_KS = (64, 128, 192)
ROW_DELTAS = (-1, 0, 1, 2, 3)  # W = 3k + d.  (3k - 1 .. 3k + 2 give A = k - 1 and k in the planted frame; k + 1 needs 3k + 3)


@lru_cache(maxsize=1)
def rows_db():
    rng = np.random.default_rng(6400)
    genes = [random_orf(rng, 60, 0.5) for _ in range(ROWS_ANCHORS)]
    for name, n in ROWS_PROTEINS.items():
        if name == "E":
            p = list(rand_protein(rng, n - 1, exclude="WC"))
            p[STRIP - 1 : STRIP + 2] = "WCW"
            genes.append(back("".join(p) + "*", rng))
        else:
            genes.append(random_orf(rng, 3 * n, 0.5))
    db = build_db("rows", [("R1", genes)], seed=6401)
    assert [int(x) for x in db.translations.lengths[ROWS_ANCHORS:]] == list(ROWS_PROTEINS.values())
    return db


def plant_len(k: int) -> int:
    return 15 * k // 32  # residues of a planted tail: two of them fit a window of k residues


@lru_cache(maxsize=1)
def rows_case() -> Case:
    """One assembly per (k, d): contigs whose windows are 3k + d bases, each with the recoded tail of one gene at its end (forward) and
    of another at its start (reverse-complemented): both alignments end on the last row of their frame text."""
    db, flank = rows_db(), 40
    case = Case("rows", db, flank)
    rng = np.random.default_rng(6402)
    G = ROWS_GENE
    for k in ROW_KS:
        m = plant_len(k)
        for d in ROW_DELTAS:
            W = 3 * k + d
            pairs = [("S", "M"), ("W", "D")] + ([("T", None)] if k == ROW_KS[0] else [])
            contigs, hits, a = [], [], len(case.genomes)
            for c, (fw, rv) in enumerate(pairs):
                tail_f = sharp_tail(rng, gene_dna(db, G[fw]), m if rv else ROWS_T_TAIL)
                tail_r = revcomp(sharp_tail(rng, gene_dna(db, G[rv]), m)) if rv else np.zeros(0, np.uint8)
                window = np.concatenate([tail_r, random_dna(rng, W - len(tail_f) - len(tail_r), 0.5), tail_f])
                assert len(window) == W
                contig, hs, hl = framed(rng, window, flank, left=17 + c, right=23)
                contigs.append(contig)
                hits.append(hit(db, c, c, hs, hl))
                for name, strand in ((fw, 1), (rv, -1)):
                    if name is None:
                        continue
                    P = ROWS_PROTEINS[name]
                    e = dict(asm=a, gene=G[name], strand=strand, frame=W % 3, contig=c, a_len=(W - W % 3) // 3, last_row=True, p_end=P, score_min=R.MIN_SCORE)
                    if P > STRIP:
                        e["p_end_gt"] = STRIP
                        e["crosses"] = (P - 1) // STRIP * STRIP  # the last column of the last strip but one
                        assert P - (m if rv or name != fw else ROWS_T_TAIL) + 10 < e["crosses"]
                    case.expect.append(e)
            case.add(f"k{k}d{d}", contigs, hits)
    return case


@lru_cache(maxsize=1)
def few_rows_case() -> Case:
    """Frame texts of one, two and three residues against the strip protein E: windows of 3 .. 11 bases with rescue_flank 0."""
    db = rows_db()
    case = Case("few rows", db, 0)
    rng = np.random.default_rng(6403)
    for A, text in ((1, "C"), (2, "WC"), (3, "WCW")):
        for extra in range(3):
            window = np.concatenate([back(text), random_dna(rng, extra, 0.5)])
            contig, hs, hl = framed(rng, window, 0, left=100, right=50)
            a = case.add(f"few{A}x{extra}", [contig], [hit(db, 0, 0, hs, hl)])
            case.expect.append(dict(asm=a, gene=ROWS_GENE["E"], strand=1, frame=0, a_len=A, a1=A, p_end=STRIP + max(A, 2) - 1, p_end_gt=STRIP,
                                    score={1: 9, 2: 20, 3: 31}[A]))  # fmt: skip
    return case


# ---- 3. the second pass's rectangle -------------------------------------------------------------------------------------------------------
RECT_COLUMNS = tuple(c for lim in (128, 256, 384, 768) for c in (lim - 1, lim + 1))
RECT_ROWS = (ROW_CHUNK - 1, ROW_CHUNK + 1)


@lru_cache(maxsize=1)
def rect_case() -> Case:
    """Fifty recoded residues of the 800-residue protein T (a whole prefix of 127 residues or more cannot end on row 63) that end on column c, at the end of a window of A residues: the best cell is
    (A, c), and the second pass fills rows 1 .. A and columns 1 .. c only."""
    db, flank, L = rows_db(), 25, 50
    case = Case("rectangle", db, flank)
    rng = np.random.default_rng(6404)
    gene = gene_dna(db, ROWS_GENE["T"])
    rec = R.recode(rng, gene)
    for c in RECT_COLUMNS:
        for A in RECT_ROWS:
            frag = np.concatenate([rec[3 * (c - L) : 3 * (c - 4)], keep(rng, gene[3 * (c - 4) : 3 * c])])
            window = np.concatenate([random_dna(rng, 3 * (A - L), 0.5), frag])
            contig, hs, hl = framed(rng, window, flank)
            a = case.add(f"c{c}r{A}", [contig], [hit(db, 0, 0, hs, hl)])
            case.expect.append(dict(asm=a, gene=ROWS_GENE["T"], strand=1, frame=0, a_len=A, a1=A, p_end=c, score_min=R.MIN_SCORE))
    return case


# ---- 4. ties between tasks of one window ----------------------------------------------------------------------------------------------------
@lru_cache(maxsize=1)
def task_ties_case() -> Case:
    """The recoded gene S twice in one window: forward and reverse-complemented (strand + wins), and forward twice 319 bases apart (the
    lower frame wins: the second copy in one assembly, the first in the other).  notes[asm] = the two task indices that tie."""
    db, flank = rows_db(), 60
    case = Case("task ties", db, flank)
    rng = np.random.default_rng(6405)
    g = ROWS_GENE["S"]
    rec = R.recode(rng, gene_dna(db, g))
    pad = lambda n: random_dna(rng, n, 0.5)  # noqa: E731
    layouts = {
        "plus_minus": ([pad(12), rec, pad(20), revcomp(rec), pad(10)], dict(strand=1, frame=0, t_start_rel=12), (0, 3 + (10 % 3))),
        "second_copy": ([pad(11), rec, pad(19), rec, pad(10)], dict(strand=1, frame=0, t_start_rel=330), (0, 2)),
        "first_copy": ([pad(12), rec, pad(19), rec, pad(10)], dict(strand=1, frame=0, t_start_rel=12), (0, 1)),
    }
    for name, (parts, want, tasks) in layouts.items():
        contig, hs, hl = framed(rng, np.concatenate(parts), flank)
        a = case.add(name, [contig], [hit(db, 0, 0, hs, hl)])
        case.expect.append(dict(asm=a, gene=g, contig=0, score_min=R.MIN_SCORE, **want))
        case.notes[a] = tasks
    return case


# ---- 7. N runs --------------------------------------------------------------------------------------------------------------------------------
N_LEFT, N_FLANK = 40, 20
N_PLACEMENTS = {  # runs [start, end) relative to the window's first base; W: the window's length
    "ends_at_ws": lambda W: [(-7, 0)],          # clear of runs
    "starts_at_we": lambda W: [(W, W + 7)],      # clear of runs
    "first_base": lambda W: [(-3, 1)],
    "last_base": lambda W: [(W - 1, W + 4)],
    "in_codon": lambda W: [(3 * 30 + 1, 3 * 30 + 2), (3 * 60 + 2, 3 * 61 + 1)],
    "all_n": lambda W: [(-10, W + 10)],
}
N_CLEAR = ("ends_at_ws", "starts_at_we")


@lru_cache(maxsize=1)
def n_runs_case() -> Case:
    """The window is the recoded gene S, forward or reverse-complemented, with N runs at and across its edges and inside its codons.
    notes[asm] = (placement, runs in contig coordinates)."""
    db = rows_db()
    case = Case("N runs", db, N_FLANK)
    rng = np.random.default_rng(6406)
    g = ROWS_GENE["S"]
    rec = R.recode(rng, gene_dna(db, g))
    for place, runs in N_PLACEMENTS.items():
        for strand in (1, -1):
            if place == "all_n" and strand < 0:
                continue
            window = rec if strand > 0 else revcomp(rec)
            contig, hs, hl = framed(rng, window, N_FLANK, left=N_LEFT, right=40)
            at = [(N_LEFT + s, N_LEFT + e) for s, e in runs(len(window))]
            for s, e in at:
                contig[s:e] = ord("N")
            a = case.add(f"{place}{'+' if strand > 0 else '-'}", [contig], [hit(db, 0, 0, hs, hl)])
            case.notes[a] = (place, at)
            if place == "all_n":
                case.expect += [dict(asm=a, gene=j, found=False) for j in range(1, len(db.genes))]
            else:
                case.expect.append(dict(asm=a, gene=g, strand=strand, contig=0, score_min=R.MIN_SCORE))
    return case


# ---- 2. ties inside one task ------------------------------------------------------------------------------------------------------------------
# Two peptides of the same residues -- each scores 100 against itself and less against the other --, a spacer residue P and a filler K in
# the text: BLOSUM62 of P or K against W, C and each other is negative, so an alignment is one peptide against one peptide.
XA, XB = "WCWWCWCCWC", "CWCCWCWWCW"
TIE_SCORE = 5 * 11 + 5 * 9
TIE_PROTEINS = {  # name: the residues before the *
    "a": "PPP" + XA + "PPP",
    "b20": XA + "P" * 20 + XA,                 # two columns per lane
    "b150": XA + "P" * 150 + XA,               # four
    "b300": XA + "P" * 300 + XA,               # six
    "c": XA + "P" * 390 + XB,                  # XB ends on column 410: strip 1, lane 4 (XA's column 10 is lane 1 of strip 0)
    "d": XA + "P" * (STRIP - len(XA)) + XB,    # XB ends on column 394 = 10 + 384: the same lane of the next strip
}
TIE_GENE = {n: 2 + i for i, n in enumerate(TIE_PROTEINS)}
TIE_TEXTS = {  # name: frame text 0 of the forward strand
    "twice": "K" * 5 + XA + "K" * 70 + XA + "K" * 5,   # rows 15 and 95
    "once": "K" * 20 + XA + "K" * 20,                    # row 30
    "b_then_a": "K" * 20 + XB + "K" * 80 + XA + "K" * 10,  # XB ends on row 30, XA on row 120
    "a_then_b": "K" * 20 + XA + "K" * 80 + XB + "K" * 10,
}
# (text, protein): the cell (row, column) the two tying cells are, first the one that must be reported
TIE_CELLS = {
    ("twice", "a"): ((15, 13), (95, 13)),                    # one column, one lane: the smaller row
    ("once", "b20"): ((30, 10), (30, 40)),                   # one row, two lanes: the smaller column
    ("once", "b150"): ((30, 10), (30, 170)),
    ("once", "b300"): ((30, 10), (30, 320)),
    ("b_then_a", "c"): ((30, 410), (120, 10)),               # the strip-1 cell has the smaller row
    ("a_then_b", "c"): ((30, 10), (120, 410)),               # mirrored: the strip-0 cell stays
    ("b_then_a", "d"): ((30, 394), (120, 10)),               # ... and both in one lane
    ("a_then_b", "d"): ((30, 10), (120, 394)),
}


@lru_cache(maxsize=1)
def ties_db():
    rng = np.random.default_rng(6410)
    genes = [random_orf(rng, 60, 0.5) for _ in range(2)] + [back(p + "*") for p in TIE_PROTEINS.values()]
    return build_db("ties", [("T1", genes)], seed=6411)


@lru_cache(maxsize=1)
def ties_case() -> Case:
    db, flank = ties_db(), 9
    case = Case("cell ties", db, flank)
    rng = np.random.default_rng(6412)
    for name, text in TIE_TEXTS.items():
        contig, hs, hl = framed(rng, back(text), flank, left=51, right=50)
        a = case.add(name, [contig], [hit(db, 0, 0, hs, hl)])
        for (t, p), ((row, col), _) in TIE_CELLS.items():
            if t == name:
                case.expect.append(dict(asm=a, gene=TIE_GENE[p], strand=1, frame=0, a_len=len(text), a1=row, p_end=col, score=TIE_SCORE))
    return case


# ---- 5 / 6. many subjects, several tasks per wave ---------------------------------------------------------------------------------------------
MANY_GENES = R.MAX_LOCUS_GENES  # exactly the limit
MANY_STRIP_GENE, MANY_STRIP_LEN = 130, 400
MANY_BITS = (63, 64, 127, 128, 191, 192, 255)
MANY_RANKS = (63, 64, 65)  # with genes 0 and 1 found and all others missing, rank s is gene s + 2
MANY_PLANTS = tuple(sorted({*MANY_BITS, *(s + 2 for s in MANY_RANKS)}))
MANY_FOUND = (3, 62, 65, 126, 129, 190, 193, 254)
MANY_SECOND, MANY_WIDE = 4, R.MAX_LOCUS_GENES + 1  # genes of the second locus: a small one, and one beyond the mask (refused at load on the device)
MANY_BARE = "WFYPCA"  # every third small protein has none of these: nothing in a window that reads TGG (W, reverse P) scores above 0
FILL_BLOCKS = (4096, 512)  # blocks of the fill launch without and with a strip protein among the subjects (kp_typing.hip)


def _small_len(j: int) -> int:
    return 20 + (7 * j) % 41  # 20 .. 60 residues


@lru_cache(maxsize=2)
def many_db(n_second: int):
    """Locus M1 of exactly KP_MAX_LOCUS_GENES genes and locus M2 of n_second.  (The first locus does not depend on n_second.)"""
    rng = np.random.default_rng(6420)
    first = [random_orf(rng, 60, 0.5) for _ in range(2)]
    for j in range(2, MANY_GENES):
        n = MANY_STRIP_LEN if j == MANY_STRIP_GENE else _small_len(j)
        first.append(back(rand_protein(rng, n - 1, exclude=MANY_BARE if j % 3 == 0 and j != MANY_STRIP_GENE else "") + "*", rng))
    second = [random_orf(rng, 60, 0.5) for _ in range(2)] + [back(rand_protein(rng, 29) + "*", rng) for _ in range(n_second - 2)]
    db = build_db("many" if n_second <= MANY_GENES else "wide", [("M1", first), ("M2", second)], seed=6421)
    assert [int(x) for x in db.locus_gene_lengths] == [MANY_GENES, n_second]
    return db


@lru_cache(maxsize=2)
def many_case(n_second: int) -> Case:
    """rescue_flank 0: a piece is its window.  `all1`, `all2`: both anchors found, 254 subjects, two windows with recoded copies of the
    genes at the mask's word edges (reverse-complemented in all2) and the tail of the strip protein; `found`: eight more genes found by
    hand-made hits that tile the windows; `second`: typed to the second locus; `bare`: two windows of three bases."""
    db = many_db(n_second)
    case = Case("many subjects", db, 0)
    case.notes["n_second"] = n_second
    rng = np.random.default_rng(6422)
    g2 = int(db.locus_gene_offsets[1])
    plants = {j: R.recode(rng, gene_dna(db, j)) for j in MANY_PLANTS}
    strip_tail = sharp_tail(rng, gene_dna(db, MANY_STRIP_GENE), 60)
    half = len(MANY_PLANTS) // 2

    def windows(reverse: bool):
        out = []
        for js, extra in ((MANY_PLANTS[:half], []), (MANY_PLANTS[half:], [strip_tail])):
            parts = [random_dna(rng, 5, 0.5)]
            for x in [plants[j] for j in js] + extra:
                parts += [revcomp(x) if reverse else x, random_dna(rng, 7, 0.5)]
            out.append(np.concatenate(parts))
        return out[::-1] if reverse else out

    def where(reverse: bool, j: int) -> int:
        return int((j in MANY_PLANTS[:half]) == reverse)

    for name, reverse in (("all1", False), ("all2", True)):
        contigs, hits = [], []
        for c, w in enumerate(windows(reverse)):
            contig, hs, hl = framed(rng, w, 0, left=20, right=20)
            contigs.append(contig)
            hits.append(hit(db, c, c, hs, hl))
        a = case.add(name, contigs, hits)
        for j in MANY_PLANTS:
            case.expect.append(dict(asm=a, gene=j, strand=-1 if reverse else 1, contig=where(reverse, j), score_min=40))
        case.expect.append(dict(asm=a, gene=MANY_STRIP_GENE, strand=-1 if reverse else 1, contig=where(reverse, MANY_STRIP_GENE),
                                p_end=MANY_STRIP_LEN, p_end_gt=STRIP, score_min=R.MIN_SCORE))  # fmt: skip
        if name == "all1":
            # ... and the same windows with eight more genes found: the hits of each contig tile its window
            hits = []
            for c in range(2):
                genes = [c, *MANY_FOUND[4 * c : 4 * c + 4]]
                cuts = [20 + i * (len(contigs[c]) - 40) // len(genes) for i in range(len(genes) + 1)]
                hits += [hit(db, g, c, s, e - s) for g, s, e in zip(genes, cuts[:-1], cuts[1:])]
            b = case.add("found", contigs, hits)
            for j in MANY_PLANTS:
                if j not in MANY_FOUND:
                    case.expect.append(dict(asm=b, gene=j, strand=1, contig=where(False, j), score_min=40))
    case.notes["second"] = case.add("second", [random_dna(rng, 200, 0.5), random_dna(rng, 200, 0.5)], [hit(db, g2, 0, 20, 60), hit(db, g2 + 1, 1, 30, 60)])
    tgg = lambda: np.concatenate([random_dna(rng, 10, 0.5), back("W"), random_dna(rng, 10, 0.5)])  # noqa: E731
    case.notes["bare"] = case.add("bare", [tgg(), tgg()], [hit(db, 0, 0, 10, 3), hit(db, 1, 1, 10, 3)])
    return case


@lru_cache(maxsize=1)
def long_scratch_case() -> Case:
    """One window of 2001 bases against the many-subjects database: a strip task whose boundary column is longer than any of many_case's."""
    db = many_db(MANY_SECOND)
    case = Case("long scratch", db, 0)
    rng = np.random.default_rng(6423)
    window = np.concatenate([random_dna(rng, 2001 - 180, 0.5), sharp_tail(rng, gene_dna(db, MANY_STRIP_GENE), 60)])
    contig, hs, hl = framed(rng, window, 0, left=20, right=20)
    a = case.add("long", [contig], [hit(db, 0, 0, hs, hl)])
    case.expect.append(dict(asm=a, gene=MANY_STRIP_GENE, strand=1, a_len=667, last_row=True, p_end=MANY_STRIP_LEN))
    return case


def check_many(case, sums, records, off):
    """The counts the many-subjects batch is there for, from the summaries and the yardstick's records."""
    n_pieces = [int(x) for x in sums["n_pieces"]]
    n_rec = [int(off[a + 1] - off[a]) for a in range(len(case.genomes))]
    tasks = sum(6 * p * n for p, n in zip(n_pieces, n_rec))
    assert sum(n_rec) > FILL_BLOCKS[1] and tasks > 4 * FILL_BLOCKS[1], "both passes queue: more subjects and far more tasks than blocks"
    ids = case.ids
    for name in ("all1", "all2", "found", "bare"):
        a = ids.index(name)
        assert n_pieces[a] == 2 and n_rec[a] > 3 * ROW_CHUNK and int(sums["best_locus"][a]) == 0 and not int(sums["overflow"][a]), name
    everything = list(range(2, MANY_GENES))
    assert R.subjects(sums[ids.index("all1")]) == everything == R.subjects(sums[ids.index("bare")])
    assert R.subjects(sums[ids.index("found")]) == [j for j in everything if j not in MANY_FOUND], "the missing set is not a prefix"
    a = case.notes["second"]
    assert int(sums["best_locus"][a]) == 1 and n_pieces[a] == 2
    if case.notes["n_second"] > MANY_GENES:  # a locus beyond the mask: overflow bit 2, no record, the offset does not advance
        assert int(sums["overflow"][a]) & 4 and n_rec[a] == 0 and int(off[a]) == int(off[a + 1]) and 0 < a < len(ids) - 1
    else:
        assert not int(sums["overflow"][a]) and n_rec[a] == case.notes["n_second"] - 2
    a = case.notes["bare"]
    absent = records["piece"][int(off[a]) : int(off[a + 1])] == -1
    assert 40 < int(absent.sum()) < len(absent) - 40 and int(np.abs(np.diff(absent.astype(np.int8))).sum()) > 40, "found and absent records interleave"
    rec = records[int(off[ids.index("all1")]) : int(off[ids.index("all1") + 1])]
    for s in MANY_RANKS:
        assert int(rec["gene"][s]) == s + 2
