"""Assemblies on both sides of every limit of the join path (kp-align v5, include/kp_spec.h): KP_JOIN_BW, KP_DIAG_GAP,
KP_MAX_SPREAD, KP_JOIN_MAX_PIECES, KP_JOIN_OPEN, KP_JOIN_GROUP_MAX, the LDS / scratch instances of the chaining kernel
(JA_SMALL = 1024 anchors) and KP_JOIN_ANCHOR_MAX.  Every case keeps the limit's effect in one gene/strand, with random
flanks; each function returns its sides in order: just inside the limit, just outside it, and where useful the next value.
Shared by tests/test_join_limits_oracle.py (the oracle lands on the intended side of every limit) and
tests/test_gpu_join_limits.py (the device equals the oracle there).  TEST INFRASTRUCTURE: no GPU, no oracle."""

from __future__ import annotations

from typing import NamedTuple

import numpy as np

from kaptive_amd.core.genome import GenomeAssembly
from kaptive_amd.core.seq import SeqRecord, Sequences
from kaptive_amd.synth import random_dna, random_orf, revcomp

# genes of database(), in order: G (cases a-d), E (longer than KP_CHAIN_MAX_DIST: case e), F (case f), U (unrelated)
GENE_LENGTHS = (("G", 4002), ("E", 12600), ("F", 24000), ("U", 1200))
G, E, F = 0, 1, 2
# case f: the copy of F ends here (flanks as drawn by anchor_counts) when the gene/strand holds exactly this many anchors
ANCHOR_TRIMS = {1024: 5567, 1025: 5571, 4096: 22009, 4097: 22014}


class Side(NamedTuple):
    limit: str  # the constant of kp_spec.h (or of the device) the case straddles
    what: str  # the quantity at that limit
    value: int
    side: str  # "inside" the limit, just "outside" it, or "next": the value after that
    gene: int  # index into database().genes
    asm: GenomeAssembly

    @property
    def label(self) -> str:
        return self.asm.id


def _genes(seed: int = 2024) -> list[np.ndarray]:
    rng = np.random.default_rng(seed)
    return [random_orf(rng, n, 0.5) for _, n in GENE_LENGTHS]


_GENES = _genes()


def database():
    """One locus per gene (a gene, 100 random bases either side): what the typed rows of the GPU test are reduced against."""
    from kaptive_amd.db import Database

    rng = np.random.default_rng(2025)
    loci = []
    for i, ((name, _), g) in enumerate(zip(GENE_LENGTHS, _GENES)):
        seq = np.concatenate([random_dna(rng, 100, 0.5), g, random_dna(rng, 100, 0.5)]).tobytes()
        loci.append(dict(name=f"JL{i + 1}", type=f"JT{i + 1}", extra=False, seq=seq,
                         genes=[dict(start=100, end=100 + len(g), strand=1, gene=f"jl{name.lower()}", product=f"join limit gene {name}")]))  # fmt: skip
    meta = dict(name="join limits", keyword="join_limits", genbank="join_limits.gbk", organism="Klebsiella pneumoniae species complex", taxon=573,
                antigen="K", pathway="Wzx/Wzy", version="synth-2024", id_threshold=82.5, doi=[], owner="kaptive_amd",
                repo="synthetic", branch="main", contact={}, phenotype_logic={})  # fmt: skip
    return Database.from_parts(meta, loci)


def _side(limit, what, value, side, gene, contigs) -> Side:
    name = f"{limit}: {what} = {value}, {side if side == 'next' else side + ' the limit'}"
    recs = [SeqRecord(f"c{i}", c.tobytes()) for i, c in enumerate(contigs)]
    return Side(limit, what, value, side, gene, GenomeAssembly(name, Sequences.from_records(recs)))


def _where(value, last_inside):
    return "inside" if value <= last_inside else ("outside" if value == last_inside + 1 else "next")


def _flank(seed):
    rng = np.random.default_rng(seed)
    return lambda n: random_dna(rng, n, 0.5)


def _indel(g, at, kind, size, flank):
    return np.concatenate([g[:at], flank(size), g[at:]]) if kind == "ins" else np.concatenate([g[:at], g[at + size :]])


# ---- a. KP_JOIN_BW ----------------------------------------------------------------------------------------------------------------
def join_bw_indel(kind: str, reverse: bool) -> list[Side]:
    """An insertion or deletion of 499, 500, 501 and 502 bases 1200 bases into G: one cluster each side of it, 500 diagonals
    apart at most for the group (d0 - dmax <= KP_JOIN_BW) and for the chain's link (dd <= KP_JOIN_BW)."""
    g = _GENES[G]
    out = []
    for size in (499, 500, 501, 502):
        flank = _flank(100 + size + (kind == "del") * 10 + reverse * 20)
        c = np.concatenate([flank(300), _indel(g, 1200, kind, size, flank), flank(300)])
        what = f"{'insertion' if kind == 'ins' else 'deletion'} ({'reverse' if reverse else 'forward'} strand)"
        out.append(_side("KP_JOIN_BW", what, size, _where(size, 500), G, [revcomp(c) if reverse else c]))
    return out


def join_bw_weak_cluster() -> list[Side]:
    """A 25-base fragment of G (a weak cluster: fewer than KP_MIN_SEED_SPAN query bases) 500 / 501 diagonals above the
    cluster before it and below the one after it: kp_chain_kernel visits that stray run only when it is linked to a
    neighbour, and the group of three chains across it only at 500."""
    g = _GENES[G]
    out = []
    for gap in (500, 501):
        flank = _flank(200 + gap)
        c = np.concatenate([flank(300), g[:1500], flank(gap), g[1500:1525], flank(gap), g[1525:], flank(300)])
        out.append(_side("KP_JOIN_BW", "weak cluster's distance from both neighbours", gap, _where(gap, 500), G, [c]))
    return out


# ---- b. KP_DIAG_GAP, KP_MAX_SPREAD ------------------------------------------------------------------------------------------------
def diag_gap_indel(kind: str) -> list[Side]:
    """An indel of 32 bases stays inside one cluster (a wider band); one of 33 cuts it into two, which the chain joins."""
    g = _GENES[G]
    out = []
    for size in (32, 33):
        flank = _flank(300 + size + (kind == "del") * 10)
        c = np.concatenate([flank(300), _indel(g, 1500, kind, size, flank), flank(300)])
        out.append(_side("KP_DIAG_GAP", "insertion" if kind == "ins" else "deletion", size, _where(size, 32), G, [c]))
    return out


def max_spread() -> list[Side]:
    """Nine insertions 150 bases apart, eight of 10 bases and a last one that brings the stretch's diagonals to a spread of
    97 (one cluster, a 128-diagonal band) or 98 (the cluster and the chain's piece are cut at the spread bound)."""
    out = []
    for total in (97, 98):
        flank = _flank(400 + total)
        g = _GENES[G]
        sizes = [10] * 8 + [total - 80]
        for k in reversed(range(len(sizes))):
            g = _indel(g, 1000 + 150 * k, "ins", sizes[k], flank)
        out.append(_side("KP_MAX_SPREAD", "spread of one stretch's diagonals", total, _where(total, 97), G, [np.concatenate([flank(300), g, flank(300)])]))
    return out


# ---- c. KP_JOIN_MAX_PIECES ----------------------------------------------------------------------------------------------------------
def max_pieces(wide: bool = False) -> list[Side]:
    """A chain of 7, 8 and 9 pieces: 40-base insertions and deletions in turn, every 250 bases of G.  ``wide``: a 3-base
    insertion inside the first piece as well, so that every piece gets the band of a piece whose diagonals spread (a piece
    of spread 2 or more needs more than 32 diagonals: kp_piece_width gives 64), chains of 8 and 9 pieces."""
    out = []
    for n in (8, 9) if wide else (7, 8, 9):
        flank = _flank(500 + n + 50 * wide)
        g = _GENES[G]
        for k in reversed(range(n - 1)):
            g = _indel(g, 250 * (k + 1), "ins" if k % 2 == 0 else "del", 40, flank)
        if wide:
            g = _indel(g, 120, "ins", 3, flank)
        what = "pieces of a chain" + (" (64-diagonal band)" if wide else "")
        out.append(_side("KP_JOIN_MAX_PIECES", what, n, _where(n, 8), G, [np.concatenate([flank(300), g, flank(300)])]))
    return out


# ---- d. KP_JOIN_OPEN ----------------------------------------------------------------------------------------------------------------
def join_open(extra=(3, 4, 5)) -> list[Side]:
    """Contig 0 = G[0:300] + G[500:800]: its second cluster sorts 200 diagonals below its first.  Further contigs of 300 bases
    of G (G[800:1100], G[1100:1400], ...), packed 32-aligned, put their clusters between those two in the sorted list, so
    contig 0's sequence waits in an LDS slot while theirs come and go, and comes back to the registers to be continued (the
    `found` branch of flush_cluster).  With 3 further contigs four sequences are open and contig 0 is joined; from 4 on a
    fifth one evicts the sequence that ends lowest -- contig 0's -- and its two clusters stay two hits."""
    g = _GENES[G]
    out = []
    for n in extra:
        flank = _flank(600 + n)
        cs = [np.concatenate([flank(100), g[0:300], g[500:800], flank(100)])]
        cs += [g[800 + 300 * k : 1100 + 300 * k].copy() for k in range(n)]
        out.append(_side("KP_JOIN_OPEN", "further contigs", n, _where(n, 3), G, cs))
    return out


# ---- e. KP_JOIN_GROUP_MAX -----------------------------------------------------------------------------------------------------------
def group_max() -> list[Side]:
    """E[0:600] and E[600:1200] with a 100-base insertion between them, and about 7 kb to the right on the same contig 14, 15
    or 16 "decoys": 30-base fragments of E[8000:], each 36 diagonals below the next and the highest 36 below E[0:600]'s.  They
    sort before the two clusters but lie more than KP_CHAIN_MAX_DIST away in the query, so nothing links them to those.  With
    14 decoys the two clusters are members 15 and 16 of one sequence and are joined; with 15 they would be members 16 and
    17, and the sequence closes before the second (KP_JOIN_GROUP_MAX); with 16 the decoys fill a sequence of their own."""
    e = _GENES[E]
    out = []
    for n in (14, 15, 16):
        flank = _flank(700 + n)
        parts, pos = [flank(200), e[0:600], flank(100), e[600:1200]], 1500
        for i in range(n):
            q = 8000 + 250 * i
            t = q + 200 - 36 * (n - i)
            parts += [flank(t - pos), e[q : q + 30]]
            pos = t + 30
        parts.append(flank(200))
        out.append(_side("KP_JOIN_GROUP_MAX", "decoy clusters before the pair", n, _where(n, 14), E, [np.concatenate(parts)]))
    return out


# ---- f. JA_SMALL / KP_JOIN_ANCHOR_MAX -----------------------------------------------------------------------------------------------
def anchor_counts(trims: dict[int, int] | None = None) -> list[Side]:
    """One copy of F with a 100-base insertion 2000 bases in: a group of two clusters.  The copy ends at ANCHOR_TRIMS[n], where
    the gene/strand holds exactly n anchors on that contig: 1024 (the LDS instance of kp_join_chain_kernel), 1025 (the
    scratch instance), 4096 (KP_JOIN_ANCHOR_MAX: chained) and 4097 (not chained: two band-task hits)."""
    f = _GENES[F]
    flank = _flank(800)
    fl = [flank(300), flank(100), flank(300)]
    out = []
    for n, end in (trims or ANCHOR_TRIMS).items():
        c = np.concatenate([fl[0], f[:2000], fl[1], f[2000:end], fl[2]])
        limit = "JA_SMALL" if n <= 1025 else "KP_JOIN_ANCHOR_MAX"
        out.append(_side(limit, "anchors of the group", n, _where(n, 1024 if limit == "JA_SMALL" else 4096), F, [c]))
    return out


def join_limit_cases() -> list[Side]:
    """Every side of every case, in a fixed order."""
    return [*join_bw_indel("ins", False), *join_bw_indel("ins", True), *join_bw_indel("del", False), *join_bw_indel("del", True),
            *join_bw_weak_cluster(), *diag_gap_indel("ins"), *diag_gap_indel("del"), *max_spread(), *max_pieces(),
            *max_pieces(wide=True), *join_open(), *join_open(extra=(1,)), *group_max(), *anchor_counts()]  # fmt: skip
