"""Inputs that land on every size class and list overflow of the three device sorts: kp_anchor_bsort_kernel
(csrc/kp_bsort.hip), kp_hit_sort_kernel and the cull order / kept list of kp_reduce_kernel (csrc/kp_reduce.hip).  Seeded and
pure numpy; where a count has to be exact (anchors of one gene/strand bucket) the builder takes the oracle and trims a copy
base by base.  Shared by tests/test_sort_classes_oracle.py (the inputs are what they are meant to be, by the oracle alone)
and tests/test_gpu_sort_classes.py (the device equals the oracle and the host reduction on them).  TEST INFRASTRUCTURE."""

from __future__ import annotations

import re
from pathlib import Path

import numpy as np

from kaptive_amd.core.genome import GenomeAssembly
from kaptive_amd.core.seq import SeqRecord, Sequences
from kaptive_amd.synth import random_dna, random_orf, revcomp

CSRC = Path(__file__).resolve().parent.parent / "kaptive_amd" / "csrc"
TOP_SHIFT = 46  # the anchor key's top field, gene * 2 + strand, starts here (databases of ordinary gene lengths)


# ---- the constants the size classes hang on, read out of the sources ---------------------------------------------------------------
def kernel_constants() -> dict[str, int]:
    bsort, reduce_ = (CSRC / "kp_bsort.hip").read_text(), (CSRC / "kp_reduce.hip").read_text()
    out = {}
    for name in ("BS_THREADS", "BS_STAGE", "BS_RANK_MAX", "BS_TILE"):
        out[name] = int(re.search(rf"constexpr int (?:\w+ = [^,;]+, )*?{name} = (\d+)\s*[,;]", bsort).group(1))
    for name in ("KP_BS_BIG_LIST", "KP_BS_HUGE_LIST"):
        out[name] = int(re.search(rf"#ifndef {name}\b.*?#define {name} (\d+)", bsort, flags=re.S).group(1))
    for name in ("KEPT_LDS", "SORT_LDS"):
        out[name] = int(re.search(rf"constexpr int {name} = (\d+);", reduce_).group(1))
    return out


def bucket_edges(c: dict[str, int]) -> tuple[int, ...]:
    """Both sides of every decision on a bucket's size: copy / network in one lane (8 registers) / wave ranking / bitonic
    network of 1, 2, 4, 8 registers per lane / block-wide ranking, there a whole tile (which is also two rounds of
    BS_THREADS keys) and one key more, and three whole rounds (a tile and a half) and one key more."""
    widths = [w for w in (64, 128, 256) if w < c["BS_STAGE"]]
    last = [1, 8, c["BS_RANK_MAX"], *widths, c["BS_STAGE"], c["BS_TILE"], c["BS_TILE"] + c["BS_THREADS"]]  # the last size of each
    return tuple(sorted({v for x in last for v in (x, x + 1)}))


def padding_edges(lo: int, hi: int) -> list[int]:
    """n - 1, n, n + 1 for every power of two from lo to hi: both sides of every padded size of a bitonic network."""
    out, n = [], lo
    while n <= hi:
        out += [n - 1, n, n + 1]
        n <<= 1
    return out


def kept_lds_edge(c: dict[str, int]) -> int:
    """Kept records kp_reduce_kernel clusters in LDS (more: in global memory)."""
    from kaptive_amd.serotyping.batch import KEPT_DTYPE

    return 3 * c["KEPT_LDS"] * 4 // KEPT_DTYPE.itemsize


EDGE_SIZES = (1, 2, 8, 9, 24, 25, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 1536, 1537)
RAW_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 4300)
TIE_SIZES = (64, 65, 4096, 4097, 4304)
CULL_SIZES = (63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6000)


def _asm(name: str, contigs) -> GenomeAssembly:
    return GenomeAssembly(name, Sequences.from_records([SeqRecord(f"c{i}", np.asarray(c, np.uint8).tobytes()) for i, c in enumerate(contigs)]))


def bucket_sizes(anchors: np.ndarray, n_values: int, shift: int = TOP_SHIFT) -> np.ndarray:
    """Anchors per value of the top key field (gene * 2 + strand) of one assembly's sorted list."""
    return np.bincount((anchors >> np.uint64(shift)).astype(np.int64), minlength=n_values)


# ---- A. anchor bucket sort: one database of random genes ---------------------------------------------------------------------------
# genes 0..17: one per edge size, long enough for it (a copy adds about one anchor per 5.6 bases); then the genes of the
# overflow assembly, shuffled so that every 64-bin piece a wave walks holds every size: (length, genes); each gene is
# planted on both strands, two buckets
OVERFLOW_GENES = {"small": (185, 512), "w2": (540, 21), "w4": (1050, 21), "w8": (2100, 21), "huge": (3020, 38)}
N_EDGE_GENES = len(EDGE_SIZES)


def bucket_genes() -> list[np.ndarray]:
    rng = np.random.default_rng(4101)
    edge = [random_dna(rng, max(80, int(6.2 * n) + 80), 0.5) for n in EDGE_SIZES]
    rest = [random_dna(rng, length, 0.5) for length, n in OVERFLOW_GENES.values() for _ in range(n)]
    return edge + [rest[i] for i in rng.permutation(len(rest))]


def bucket_gene_sequences() -> Sequences:
    return Sequences.from_records([SeqRecord(f"g{i}", g.tobytes()) for i, g in enumerate(bucket_genes())])


def _edge_block(genes, i: int, trim) -> np.ndarray:
    rng = np.random.default_rng(4200 + i)  # a gene's flanks are its own: the count found alone holds beside the others
    return np.concatenate([random_dna(rng, 100, 0.5), genes[i][trim[0] : trim[1]], random_dna(rng, 100, 0.5)])


def edge_trims(odb) -> list[tuple[int, int]]:
    """Per edge gene the piece [start, end) of it whose copy puts exactly EDGE_SIZES[i] anchors into its forward bucket: a
    bisection on the end, then base by base around it (a base more can move a minimizer at the copy's end, and the count
    can step by two); where no end gives the count, the same from the next start."""
    genes = bucket_genes()

    def count(i, start, end):
        a = odb.anchors(_asm("trim", [_edge_block(genes, i, (start, end))]).packed())
        return int(((a >> np.uint64(TOP_SHIFT)) == np.uint64(2 * i)).sum())

    trims = []
    for i, want in enumerate(EDGE_SIZES):
        found = None
        for start in range(0, 30):
            lo, hi = start + 15, len(genes[i])
            assert count(i, start, hi) >= want, f"gene {i} is too short for {want} anchors"
            while lo < hi:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if count(i, start, mid) >= want else (mid + 1, hi)
            ends = (e for d in range(30) for e in (lo + d, lo - d) if start + 15 <= e <= len(genes[i]))
            found = next(((start, e) for e in ends if count(i, start, e) == want), None)
            if found:
                break
        assert found, f"no piece of gene {i} gives exactly {want} anchors"
        trims.append(found)
    return trims


def edge_assemblies(trims) -> list[GenomeAssembly]:
    """Every edge gene's trimmed copy on one contig, and that contig's reverse complement (the other strand's buckets)."""
    genes = bucket_genes()
    fwd = np.concatenate([_edge_block(genes, i, t) for i, t in enumerate(trims)])
    return [_asm("edges_forward", [fwd]), _asm("edges_reverse", [revcomp(fwd)])]


def overflow_assembly() -> GenomeAssembly:
    """Every overflow gene once forward and once as reverse complement, in a random order, 25 random bases between them:
    more buckets of 25..512 keys than BS_BIG_LIST and more above 512 than BS_HUGE_LIST, at the default constants."""
    genes = bucket_genes()[N_EDGE_GENES:]
    rng = np.random.default_rng(4300)
    parts = [random_dna(rng, 60, 0.5)]
    for j in rng.permutation(2 * len(genes)):
        g = genes[j // 2]
        parts += [g if j % 2 == 0 else revcomp(g), random_dna(rng, 25, 0.5)]
    seq = np.concatenate(parts)
    cuts = np.linspace(0, len(seq), 7).astype(int)  # six contigs; a cut through a copy only makes two smaller buckets' worth
    return _asm("both_lists_full", [seq[a:b] for a, b in zip(cuts[:-1], cuts[1:])])


def empty_assembly() -> GenomeAssembly:
    return _asm("no_anchor", [random_dna(np.random.default_rng(4400), 3000, 0.5)])


def ordinary_assembly() -> GenomeAssembly:
    from kaptive_amd.synth import mutate

    genes = bucket_genes()
    rng = np.random.default_rng(4500)
    parts = [random_dna(rng, 500, 0.5)]
    for i in rng.choice(np.arange(N_EDGE_GENES, len(genes)), size=30, replace=False):
        parts += [mutate(rng, genes[int(i)], 0.03), random_dna(rng, 200, 0.5)]
    return _asm("ordinary", [np.concatenate(parts), random_dna(rng, 20_000, 0.5)])


def bucket_batch(trims) -> list[GenomeAssembly]:
    over = overflow_assembly()
    return [over, empty_assembly(), ordinary_assembly(), *edge_assemblies(trims), over]


# buckets that span two values (more than 16384 genes: a bucket is a gene's two strands)
def span_db():
    from kaptive_amd.synth import make_db

    return make_db("ab_k", seed=105, n_loci=800)


def span_assembly(db) -> tuple[GenomeAssembly, int, int]:
    """(assembly, gene A, gene B): about 300 anchors of A on either strand -- each value below BS_STAGE, the bucket above --
    and about 15 of B on either strand -- each value a wave ranking's, the bucket a bitonic network's."""
    lengths = np.asarray(db.genes.lengths)
    a = next(i for i in range(9000, len(lengths)) if lengths[i] >= 1750)
    b = a + 46
    ga, gb = (np.frombuffer(db.genes[i].seq, np.uint8) for i in (a, b))
    rng = np.random.default_rng(4600)
    r = lambda n: random_dna(rng, n, 0.39)
    c = np.concatenate([r(400), ga[:1700], r(300), revcomp(ga[:1700]), r(300), gb[:96], r(200), revcomp(gb[:96]), r(400)])
    return _asm("spanning_buckets", [c, r(30_000)]), a, b


# ---- B / C. hit sort, cull order and kept hits: a database of short genes with typing tables -------------------------------------
HIT_LOCI, HIT_GENES_PER_LOCUS = 216, 20


def hit_db():
    """216 loci of 20 genes of 150-207 bases: 4320 genes; an exact copy scores 2 per base, 300 and more."""
    from kaptive_amd.db import Database

    rng = np.random.default_rng(5100)
    loci = []
    for li in range(HIT_LOCI):
        parts, genes = [random_dna(rng, 60, 0.5)], []
        pos = 60
        for gi in range(HIT_GENES_PER_LOCUS):
            orf = random_orf(rng, int(rng.integers(150, 210)), 0.5)
            parts += [orf, random_dna(rng, 40, 0.5)]
            genes.append(dict(start=pos, end=pos + len(orf), strand=1, gene=f"sc{li}_{gi}", product=f"sort class gene {li}-{gi}"))
            pos += len(orf) + 40
        loci.append(dict(name=f"SC{li + 1}", type=f"ST{li + 1}", extra=False, seq=np.concatenate(parts).tobytes(), genes=genes))
    meta = dict(name="sort classes", keyword="sort_classes", genbank="sort_classes.gbk", organism="Klebsiella pneumoniae species complex",
                taxon=573, antigen="K", pathway="Wzx/Wzy", version="synth-5100", id_threshold=82.5, doi=[], owner="kaptive_amd",
                repo="synthetic", branch="main", contact={}, phenotype_logic={})  # fmt: skip
    return Database.from_parts(meta, loci)


def _gene_order(db) -> np.ndarray:
    return np.random.default_rng(5200).permutation(len(db.genes))


def _planted(db, gene_ids, rng, per_contig=128, flip=True):
    """One exact copy per entry of gene_ids, 60-100 random bases between copies, every third one reverse-complemented."""
    contigs, parts = [], [random_dna(rng, 80, 0.5)]
    for k, g in enumerate(gene_ids):
        seq = np.frombuffer(db.genes[int(g)].seq, np.uint8)
        parts += [revcomp(seq) if flip and k % 3 == 2 else seq, random_dna(rng, int(rng.integers(60, 101)), 0.5)]
        if (k + 1) % per_contig == 0:
            contigs.append(np.concatenate(parts))
            parts = [random_dna(rng, 80, 0.5)]
    if len(parts) > 1:
        contigs.append(np.concatenate(parts))
    return contigs


def raw_hit_assembly(db, n: int, in_gene_order: bool = False) -> GenomeAssembly:
    """A_n: the first n genes of a seeded permutation, one exact copy each; nothing overlaps, nothing is joined: n raw hits,
    n hits, n kept hits.  ``in_gene_order``: planted in the order of the database."""
    ids = _gene_order(db)[:n]
    if in_gene_order:
        ids = np.sort(ids)
    return _asm(f"A_{n}{'_sorted' if in_gene_order else ''}", _planted(db, ids, np.random.default_rng(5300 + n)))


def tie_assembly(db, n: int) -> GenomeAssembly:
    """T_n: n // 8 genes in 8 identical copies each, 6 on contig 0 and 2 on contig 1 (hits equal in gene, score and contig in
    runs of 6 and of 2; eight occurrences of a seed stay below the occurrence cut), and n % 8 further genes once on contig 2."""
    order = _gene_order(db)
    ids, single = order[: n // 8], order[n // 8 : n // 8 + n % 8]
    rng = np.random.default_rng(5400 + n)
    big = lambda ids_: np.concatenate(_planted(db, ids_, rng, per_contig=1 << 30, flip=False))
    contigs = [big(np.tile(ids, 6)), big(np.tile(ids, 2))] + ([big(single)] if len(single) else [])
    return _asm(f"T_{n}", contigs)


def leading_runs(hits: np.ndarray) -> np.ndarray:
    """Lengths of the runs of equal leading keys (kp_hit_keys: gene, order score, contig) in a sorted hit table; the
    records of finished hits hold the plain score, and these inputs hold no joined hit, whose order score would differ."""
    key = np.stack([hits["gene"], hits["score"], hits["contig"]], axis=1).astype(np.int64)
    new = np.ones(len(key), bool)
    new[1:] = (key[1:] != key[:-1]).any(axis=1)
    return np.diff(np.append(np.flatnonzero(new), len(key)))


def raw_hit_count(odb, pa, min_dp_score: int) -> int:
    """Raw hits of the device's hit compaction, from the oracle's task results: band tasks at or above the score cut, none
    consumed by a join (the caller asserts there is no join)."""
    tasks = odb.tasks(pa)
    return int((odb.sw(pa, tasks)[:, 0] >= min_dp_score).sum())
