"""Batches of a thousand and more full-size assemblies from a few dozen distinct ones: the oracle runs once per distinct
assembly, and a batch is a list of keys into that set, each taken many times.  Shared by tests/test_large_batch_oracle.py
(the compositions land where they are meant to: totals on the intended side of 2^31, 2^32 and 2^33 bases, a hit across
each boundary) and tests/test_gpu_large_batches.py (the device equals the oracle there).  TEST INFRASTRUCTURE: no GPU;
the oracle runs in spawned workers (the GPU test's own process holds a HIP context, which does not survive a fork).

A key names one assembly:
  ("src", config, i)              tests.sweep_util.make(config, i): the sweep's variety at full size
  ("free", config, seed, genes)   make_assembly(main database, seed, locus=-1, + the configuration's shape): no locus, so no
                                  hits; with genes > 0 one more contig that holds that many genes of the main database
                                  between random bases: a few hits, a few band tasks
  ("rand", config, length, seed)  one contig of `length` random bases (a multiple of 64: it fills its padded slot)
and an Item holds what the tests need of it: the packed assembly, its id, the oracle's hit table and the host
reduction's row per database of the configuration, and which hits of the main database are joined ones."""

from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np

from kaptive_amd.pack import PackedAssembly

N_SOURCES = {"kpsc": 24, "ab_k": 8}
FREE = ((41_000, 0), (41_001, 2), (41_002, 0), (41_003, 3))  # the locus-free fillers of the batch just inside 2^33 bases
MAX_BASES = 1 << 33  # KP_CAND_POS_BITS = 33 (kp_scan.hip): a batch holds fewer bases than this
_ITEMS: dict = {}


class Item(NamedTuple):
    packed: PackedAssembly
    id: str
    hits: list  # per database of the configuration: the oracle's hit table
    rows: list  # per database: KaptiveRow bytes of the host reduction on those hits
    joined: np.ndarray  # per hit of the main database: reported by a join of two or more pieces (kp-align v5)


def sources(config: str) -> list[tuple]:
    return [("src", config, i) for i in range(N_SOURCES[config])]


def free_fillers(config: str = "kpsc") -> list[tuple]:
    return [("free", config, s, n) for s, n in FREE]


def databases(config: str) -> tuple:
    """(main database, further database or None) of a configuration of tests.sweep_util, kept where its make() keeps them."""
    from kaptive_amd.synth import make_db
    from tests import sweep_util as S

    if ("dbs", config) not in S._STATE:
        c = S.CONFIGS[config]
        S._STATE["dbs", config] = (make_db(c["main"][0], seed=c["main"][1]), make_db(c["also"][0], seed=c["also"][1]) if c["also"] else None)
    return S._STATE["dbs", config]


def _genome(key):
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import make_assembly, random_dna
    from tests import sweep_util as S

    kind, config = key[:2]
    if kind == "src":
        return S.make(config, key[2])
    main, also = databases(config)
    if kind == "free":
        g = make_assembly(main, seed=key[2], locus=-1, **S.CONFIGS[config]["asm"])
        if key[3]:
            rng = np.random.default_rng(key[2])
            parts = [random_dna(rng, 300, 0.5)]
            for gi in rng.choice(len(main.genes), size=key[3], replace=False):
                parts += [np.frombuffer(main.genes[int(gi)].seq, np.uint8), random_dna(rng, 300, 0.5)]
            recs = [SeqRecord(g.contigs.ids[i], g.contigs[i].seq) for i in range(len(g.contigs))]
            g = GenomeAssembly(g.id, Sequences.from_records(recs + [SeqRecord("genes", np.concatenate(parts).tobytes())]))
        return g, main, also
    length, seed = key[2:]
    assert kind == "rand" and length > 0 and length % 64 == 0, key
    dna = random_dna(np.random.default_rng(seed), length, 0.5)
    return GenomeAssembly(f"random_{length}_{seed}", Sequences.from_records([SeqRecord("c0", dna.tobytes())])), main, also


def packed_of(key) -> PackedAssembly:
    """The packed assembly of a key alone, without the oracle."""
    return _genome(key)[0].packed()


def _oracle_item(key):
    """Worker: one key -> the fields of its Item (in the style of tests.sweep_util.oracle_hits, whose tables it returns
    for the sources)."""
    from kaptive_amd.core.pairwise import PairwiseAlignments
    from kaptive_amd.pack import pack_sequences_flat
    from kaptive_amd.serotyping.core import Serotyper
    from kaptive_amd.serotyping.io import KaptiveRow
    from oracle import oracle as O
    from tests import sweep_util as S
    from tests.golden_util import hits_to_alignments

    g, main, also = _genome(key)
    config = key[1]
    pa = g.packed()
    for k, db in enumerate((main, also)):
        if db is not None and ("odb", config, k) not in S._STATE:
            S._STATE["odb", config, k] = O.OracleDB(*pack_sequences_flat(db.genes))
    if key[0] == "src":
        hits, rows = S.oracle_hits(key[1:])
    else:
        hits, rows = [], []
        for k, db in enumerate((main, also)):
            if db is None:
                continue
            h = np.array(S._STATE["odb", config, k].align(pa))
            hits.append(h)
            typer = Serotyper(
                db, aligner=lambda genome, db=db, h=h: hits_to_alignments(db, genome, h),
                protein_aligner=lambda q, t: PairwiseAlignments.from_table(
                    O.protein_align(q.seqs, q.offsets, q.lengths, t.seqs, t.offsets, t.lengths)),
            )  # fmt: skip
            rows.append(bytes(KaptiveRow.from_result(typer(g))))
    # hits of the main database that a join reports: a piece in state 1 whose path visited two pieces or more
    joins = S._STATE["odb", config, 0].joins(pa)
    spans = set()
    for j in joins:
        for p in j["piece"][: int(j["n_pieces"])]:
            if p[0] == 1 and bin(int(p[1]) & 0xFFFFFFFF).count("1") >= 2:
                spans.add((int(j["gs"]) // 2, int(j["contig"]), int(p[3]), int(p[4])))  # (its t_start, t_end: the assembly's coordinates)
    h = hits[0]
    joined = np.array([(int(x["gene"]), int(x["contig"]), int(x["q_start"]), int(x["q_end"])) in spans for x in h], bool)
    return (np.asarray(pa.words), pa.padded_len, pa.ctg_start, pa.ctg_len, pa.n_runs), g.id, hits, rows, joined


def workers() -> int:
    return min(16, max(2, (os.cpu_count() or 2) // 2))


def items(keys) -> dict:
    """{key: Item} for every key, each distinct assembly generated, packed and aligned by the oracle once per process."""
    import multiprocessing as mp

    todo = [k for k in dict.fromkeys(keys) if k not in _ITEMS]
    if todo:
        with mp.get_context("spawn").Pool(min(workers(), len(todo))) as pool:
            for k, (fields, id_, hits, rows, joined) in zip(todo, pool.map(_oracle_item, todo, chunksize=1)):
                _ITEMS[k] = Item(PackedAssembly(*fields), id_, hits, rows, joined)
    return {k: _ITEMS[k] for k in keys}


# ---- composition --------------------------------------------------------------------------------------------------------------
def compose(config: str, n_entries: int, seed: int) -> list[tuple]:
    """`n_entries` keys of the configuration's sources: one seeded permutation of all sources after another, counted from
    the END of the list (the part above 2^32 bases is the short one, and whole permutations lie in it), so every source
    occurs n_entries / n_sources times, next to ever different neighbours, on both sides of every boundary."""
    rng = np.random.default_rng(seed)
    src = sources(config)
    out: list[tuple] = []
    while len(out) < n_entries:
        out = [src[i] for i in rng.permutation(len(src))] + out
    return out[len(out) - n_entries :]


def word_offsets(keys, its) -> np.ndarray:
    """asm_word_off of the batch, as _native.Batch computes it: n + 1 offsets in 16-base words."""
    off = np.zeros(len(keys) + 1, np.int64)
    np.cumsum([its[k].packed.padded_len // 16 for k in keys], out=off[1:])
    return off


def total_bases(keys, its) -> int:
    return int(word_offsets(keys, its)[-1]) * 16


def hit_spans(keys, its, off, e: int) -> np.ndarray:
    """[n, 2] batch-wide first and one-past-last base of every hit of entry e on the main database: t_start and t_end are
    contig coordinates, the contig starts at ctg_start in the assembly's padded space, the assembly at 16 * off[e]."""
    it = its[keys[e]]
    h = it.hits[0]
    base = 16 * int(off[e]) + it.packed.ctg_start[h["contig"]].astype(np.int64)
    return np.stack([base + h["t_start"], base + h["t_end"]], axis=1)


def entry_of(off: np.ndarray, base: int) -> int:
    return int(np.searchsorted(off * 16, base, side="right")) - 1


def hit_across(keys, its, boundary: int):
    """(the entry that holds base `boundary`, indices of its main-database hits with t_start < boundary - 1 and
    boundary < t_end - 1: the boundary strictly inside them, two bases or more on either side)."""
    off = word_offsets(keys, its)
    e = entry_of(off, boundary)
    assert 0 <= e < len(keys), f"no entry of the batch holds base {boundary}"
    sp = hit_spans(keys, its, off, e)
    return e, np.flatnonzero((sp[:, 0] < boundary - 1) & (boundary < sp[:, 1] - 1))


def plant(keys: list, its: dict, boundary: int, joined: bool, seed: int) -> tuple[list, tuple]:
    """A copy of `keys` with one ("rand", ...) filler inserted so that base `boundary` of the batch falls in the middle of a
    hit of the main database, and that filler's key.  The hit is one of the entry that holds the boundary or of its
    predecessor, with its midpoint at least 64 bases below the boundary -- of all those the one in the middle --; the filler
    goes in front of that entry and pushes the midpoint up to the boundary, to within the 64 bases its length is a multiple
    of (hits shorter than 256 bases are not taken).  `joined`: the hit is a joined one; the predecessor then changes places with the nearest earlier entry of
    a source that has joined hits (i % 4 == 3), if it is not one itself."""
    keys = list(keys)
    e = entry_of(word_offsets(keys, its), boundary)
    assert 1 <= e < len(keys), f"no entry of the batch holds base {boundary}"
    if joined and not its[keys[e - 1]].joined.any():
        j = next(j for j in range(e - 2, -1, -1) if its[keys[j]].joined.any())
        keys[j], keys[e - 1] = keys[e - 1], keys[j]
    off = word_offsets(keys, its)
    cands = []  # (filler length, entry)
    for c in (e - 1, e):
        sp = hit_spans(keys, its, off, c)
        ok = (sp[:, 1] - sp[:, 0] >= 256) & (its[keys[c]].joined if joined else True)
        need = boundary - (sp[:, 0] + sp[:, 1]) // 2
        cands += [(int(n + 32) // 64 * 64, c) for n in need[ok & (need >= 64)]]
    assert cands, f"no hit to put across base {boundary}"
    best = sorted(cands)[len(cands) // 2]  # the median: hits of that entry remain on either side of the boundary
    filler = ("rand", keys[0][1], best[0], seed)
    return keys[: best[1]] + [filler] + keys[best[1] :], filler


# ---- the batches of the tests ---------------------------------------------------------------------------------------------------
def benchmark_shape_batch() -> tuple[list, dict, list]:
    """Case a: 1024 entries of the kpsc sources and two planted fillers, bases 2^31 and 2^32 inside a hit each (the second a
    joined one): (keys, items, the two fillers' keys).  2^31 first: each filler moves what follows it."""
    keys = compose("kpsc", 1024, seed=1)
    its = items(keys)
    fillers = []
    for boundary, joined, seed in ((1 << 31, False, 51_031), (1 << 32, True, 51_032)):
        keys, f = plant(keys, its, boundary, joined, seed)
        its = {**its, **items([f])}
        fillers.append(f)
    return keys, its, fillers


def many_contigs_batch() -> tuple[list, dict]:
    """Case b: 1100 entries of the ab_k sources (4 Mbp in about 1500 contigs each)."""
    keys = compose("ab_k", 1100, seed=2)
    return keys, items(keys)


def inside_limit_batch(n_real: int = 48) -> tuple[list, dict, tuple]:
    """Case c (and d, with a last entry 64 bases longer): a batch of exactly 2^33 - 64 bases -- locus-free fillers (four
    distinct ones, about 1600 entries), then `n_real` entries of the kpsc sources, then one contig of random bases whose
    length makes up the total: (keys, items, that last filler's key).  How many fillers there are and how often each is
    taken is chosen so that the last contig is as short as it can be (but 4096 bases or longer): the real sources sit at
    the highest positions a batch may hold."""
    free = free_fillers()
    real = compose("kpsc", n_real, seed=3)
    its = items(free + real)
    fl = [its[k].packed.padded_len for k in free]
    room = MAX_BASES - 64 - sum(its[k].packed.padded_len for k in real)  # what the fillers and the last contig share
    best = None  # (length of the last contig, how often each of the four fillers is taken)
    for n in range(room // max(fl) - 1, room // min(fl) + 1):
        n0, n1 = np.arange(8, n, 7)[:, None], np.arange(8, n, 11)[None, :]
        rest = n - n0 - n1  # the third and the fourth share these
        left = room - (n0 * fl[0] + n1 * fl[1] + (rest + 1) // 2 * fl[2] + rest // 2 * fl[3])
        left = np.where((rest >= 16) & (left >= 4096), left, room)
        i, j = np.unravel_index(int(left.argmin()), left.shape)
        if best is None or int(left[i, j]) < best[0]:
            r = int(rest[i, j])
            best = (int(left[i, j]), [int(n0[i, 0]), int(n1[0, j]), (r + 1) // 2, r // 2])
    order = np.random.default_rng(4).permutation(np.repeat(np.arange(4), best[1]))
    last = ("rand", "kpsc", best[0], 51_033)
    keys = [free[i] for i in order] + real + [last]
    its = {**its, **items([last])}
    assert total_bases(keys, its) == MAX_BASES - 64
    return keys, its, last
