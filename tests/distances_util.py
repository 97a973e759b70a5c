"""The yardstick of the pairwise locus distances (include/kp_spec.h, DISTANCES): a numpy restatement that shares nothing with
kaptive_amd/csrc/kp_dist.h or kaptive_amd/distances.py.  Blocks are unpacked to one code per column -- 0..3 a base, 4 an N, 5 GAP --,
padding is flagged by position, the counts come from comparing code arrays and the listing from a plain loop over a with one
broadcast over b.  Kaptive has no such output, so there is no reference implementation: equality with this file is exact."""

from __future__ import annotations

import ctypes as C

import numpy as np

N, GAP = 4, 5
PAIR_DTYPE = np.dtype([("a", "<i4"), ("b", "<i4"), ("compared", "<i4"), ("differences", "<i4"), ("unshared", "<i4"), ("pad", "<i4")])
HEADER = b"Locus\tAssembly A\tAssembly B\tColumns\tCompared\tDifferences\tUnshared\n"
TILE, CHUNK, WORD_BLOCKS, MAX_DIFF, MIN_COMPARED, MAX_ROWS = 64, 8, 4, 10, 1, 1 << 18  # the constants the headers must hold
LETTERS = {c: i for i, c in enumerate("acgt")} | {"n": N, "-": GAP}


def codes_of(text: str) -> np.ndarray:
    return np.array([LETTERS[c] for c in text], np.uint8)


def pack(codes) -> np.ndarray:
    """uint64 blocks of a code array whose length is a multiple of 16 (ALIGNED ROWS packed form; a GAP column sets its gap bit)."""
    c = np.asarray(codes, np.uint8).reshape(-1, 16).astype(np.uint64)
    j = np.arange(16, dtype=np.uint64)[None, :]
    w = (np.where(c < 4, c, 0) << (2 * j)).sum(axis=1, dtype=np.uint64)
    m = ((c == N).astype(np.uint64) << (j + np.uint64(32))).sum(axis=1, dtype=np.uint64)
    g = ((c == GAP).astype(np.uint64) << (j + np.uint64(48))).sum(axis=1, dtype=np.uint64)
    return w | m | g


def unpack(blocks) -> np.ndarray:
    """uint8 codes, sixteen per block, of an array of blocks of any shape [..., nb] -> [..., 16 nb]."""
    v = np.asarray(blocks, np.uint64)[..., None]
    j = np.arange(16, dtype=np.uint64)
    code = ((v >> (2 * j)) & np.uint64(3)).astype(np.uint8)
    code[((v >> (j + np.uint64(32))) & np.uint64(1)) != 0] = N
    code[((v >> (j + np.uint64(48))) & np.uint64(1)) != 0] = GAP
    return code.reshape(*np.asarray(blocks).shape[:-1], -1)


def gene_blocks(codes) -> np.ndarray:
    """The blocks a gene of len(codes) columns contributes to a locus row: its codes, then GAP up to the end of the last block."""
    codes = np.asarray(codes, np.uint8)
    return pack(np.concatenate([codes, np.full(-len(codes) % 16, GAP, np.uint8)]))


def counts(ca, cb) -> tuple[int, int, int]:
    """(compared, differences, unshared) of two code arrays."""
    ca, cb = np.asarray(ca), np.asarray(cb)
    both = (ca < 4) & (cb < 4)
    return int(both.sum()), int((both & (ca != cb)).sum()), int(((ca == GAP) != (cb == GAP)).sum())


def all_pairs(codes, max_diff=None, min_compared=0) -> np.ndarray:
    """PAIR_DTYPE records of the listed pairs of the rows of ``codes`` [R, columns], ascending (a, b)."""
    codes = np.asarray(codes, np.uint8)
    R = codes.shape[0]
    md = np.iinfo(np.int32).max if max_diff is None else max_diff
    out = []
    for a in range(R - 1):
        x, y = codes[a][None, :], codes[a + 1 :]
        both = (x < 4) & (y < 4)
        comp, diff, uns = both.sum(axis=1), (both & (x != y)).sum(axis=1), ((x == GAP) != (y == GAP)).sum(axis=1)
        for k in np.flatnonzero((diff <= md) & (comp >= min_compared)):
            out.append((a, a + 1 + int(k), int(comp[k]), int(diff[k]), int(uns[k]), 0))
    return np.array(out, PAIR_DTYPE) if out else np.zeros(0, PAIR_DTYPE)


def format_lines(locus: str, columns: int, names, pairs) -> bytes:
    return b"".join(f"{locus}\t{names[p['a']]}\t{names[p['b']]}\t{columns}\t{p['compared']}\t{p['differences']}\t{p['unshared']}\n".encode() for p in pairs)


# ---- locus rows, gene by gene ---------------------------------------------------------------------------------------------------------
F_SPURIOUS, F_PRIMARY = 16, 32


def locus_row(db, locus: int, n_kept: int, kept, rows, blocks) -> np.ndarray:
    """The locus row of one assembly as codes [16 NB]: for every gene of ``locus`` in database order the row of its kept record with
    KP_F_PRIMARY, unpacked to the gene's length, or GAP; padding GAP."""
    g0 = int(db.locus_gene_offsets[locus])
    out = []
    for g in range(g0, g0 + int(db.locus_gene_lengths[locus])):
        L = int(db.genes.lengths[g])
        codes = np.full(L, GAP, np.uint8)
        for i in range(int(n_kept)):
            if int(kept[i]["gene"]) == g and int(kept[i]["flags"]) & F_PRIMARY:
                off = int(rows[i]["off"])
                assert int(rows[i]["gene_len"]) == L
                codes = unpack(np.asarray(blocks[off : off + (L + 15) // 16], np.uint64))[:L]
        out.append(np.concatenate([codes, np.full(-L % 16, GAP, np.uint8)]))
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def run_pairs(db, best, n_kept, kept, rows, blocks, max_diff=MAX_DIFF, min_compared=MIN_COMPARED):
    """[(locus, a, b, compared, differences, unshared)] of a whole run, loci in database order, a and b numbering the assemblies."""
    out = []
    for L in sorted(set(int(b) for b in best)):
        members = [a for a in range(len(best)) if int(best[a]) == L]
        codes = np.stack([locus_row(db, L, n_kept[a], kept[a], rows[a], blocks) for a in members])
        for p in all_pairs(codes, max_diff, min_compared):
            out.append((L, members[p["a"]], members[p["b"]], int(p["compared"]), int(p["differences"]), int(p["unshared"])))
    return out


def run_tsv(db, ids, best, n_kept, kept, rows, blocks, max_diff=MAX_DIFF, min_compared=MIN_COMPARED) -> bytes:
    lines = []
    for L, a, b, c, d, u in run_pairs(db, best, n_kept, kept, rows, blocks, max_diff, min_compared):
        g0, g1 = int(db.locus_gene_offsets[L]), int(db.locus_gene_offsets[L] + db.locus_gene_lengths[L])
        lines.append(f"{db.loci.ids[L]}\t{ids[a]}\t{ids[b]}\t{int(np.asarray(db.genes.lengths[g0:g1]).sum())}\t{c}\t{d}\t{u}\n".encode())
    return b"".join(lines)


# ---- populations for the device tests ---------------------------------------------------------------------------------------------------
def population(rng, R: int, nb: int) -> np.ndarray:
    """Codes [R, 16 nb]: mutated copies of three founders (so that a max_diff splits the pairs) with planted N and GAP runs, and --
    where R allows -- the planted rows of the device tests: two identical rows, an all-GAP row, an all-N row, rows one column away
    from row 10 (at column 0, either side of a plane-word edge and of a chunk edge, the last column) and a pair of complements."""
    cols = 16 * nb
    founders = rng.integers(0, 4, (3, cols)).astype(np.uint8)
    codes = founders[rng.integers(0, 3, R)].copy() if R else np.zeros((0, cols), np.uint8)
    for r in range(R):
        k = int(rng.integers(0, 13))
        at = rng.integers(0, cols, k)
        codes[r, at] = (codes[r, at] + rng.integers(1, 4, k)) % 4
        if rng.random() < 0.5:
            s = int(rng.integers(0, cols))
            codes[r, s : s + int(rng.integers(1, 40))] = N
        if rng.random() < 0.5:
            s = int(rng.integers(0, cols))
            codes[r, s : s + int(rng.integers(1, 80))] = GAP
    if R >= 16:
        codes[1] = codes[0]
        codes[2] = GAP
        codes[3] = N
        codes[10] = founders[0]
        edges = [0, 63, 64, 64 * CHUNK - 1, 64 * CHUNK, cols - 1]
        for r, c in zip(range(4, 10), edges):
            codes[r] = codes[10]
            c = min(c, cols - 1)
            codes[r, c] = (codes[10, c] + 1) % 4
        codes[11] = founders[1]
        codes[12] = 3 - founders[1]
    return codes


# ---- kp_dist.h under g++ -----------------------------------------------------------------------------------------------------------------
def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    h = build_harness("dist_harness", "kp_dist.h")
    h.kpy_dist_pad_mask.restype = C.c_uint64
    h.kpy_dist_pad_mask.argtypes = [C.c_int64]
    h.kpy_dist_tiles.restype = C.c_int64
    h.kpy_dist_tiles.argtypes = [C.c_int64]
    return h


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness_counts(a_blocks, b_blocks) -> tuple[int, int, int]:
    a, b = np.ascontiguousarray(a_blocks, np.uint64), np.ascontiguousarray(b_blocks, np.uint64)
    out = np.zeros(3, np.int32)
    harness().kpy_dist_pair_counts(_p(a), _p(b), C.c_int64(len(a)), _p(out))
    return tuple(int(x) for x in out)


# ---- what the GPU modules of the pair reports (tests/test_gpu_distances.py, test_gpu_clusters.py, test_gpu_tree.py) share: their shapes
# and the run on the miniature database.  Not part of the yardstick above: this part drives the package.
from kaptive_amd import _native  # noqa: E402

T, CH = _native.DIST_TILE, _native.DIST_CHUNK
ROWS = (0, 1, 2, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5)
SPLIT = 6  # a max_diff between the relatives of a founder (at most 24 apart, most far fewer) and strangers (three quarters of the columns)


def _device_count() -> int:
    import torch

    return torch.cuda.device_count()


def _genome(name, rng, locus_seq):
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import random_dna

    contigs = [random_dna(rng, 30_000, 0.5), np.concatenate([random_dna(rng, 12_000, 0.5), locus_seq, random_dna(rng, 12_000, 0.5)]), random_dna(rng, 8_000, 0.5)]
    return GenomeAssembly(name, Sequences.from_records([SeqRecord(f"{name}_{i}", c.tobytes()) for i, c in enumerate(contigs)]))


def _flip(seq, at):
    out = seq.copy()
    out[at] = {65: 67, 67: 71, 71: 84, 84: 65}[int(seq[at])]
    return out


class Run:
    """A dozen 90 kb assemblies over three loci, typed in two batches by ``Serotyper(db, distances=True)``."""

    def __init__(self):
        from types import SimpleNamespace

        from kaptive_amd.distances import LocusRows
        from kaptive_amd.pack import pack_sequences_flat
        from kaptive_amd.serotyping.core import Serotyper
        from kaptive_amd.synth import make_db, mutate
        from tests.test_gpu_aligned import restate_batch

        self.db = db = make_db("kpsc_k", seed=7, n_loci=9)
        rng = np.random.default_rng(2024)
        genomes, self.plan = [], {}
        for L, kinds in ((0, ("exact", "exact", "snp", "lacking", "far")), (3, ("exact", "snp", "snp", "exact")), (6, ("exact", "lacking", "snp"))):
            o, n = int(db.loci.offsets[L]), int(db.loci.lengths[L])
            ref = np.asarray(db.loci.seqs[o : o + n], np.uint8).copy()
            g0 = int(db.locus_gene_offsets[L])
            for k, kind in enumerate(kinds):
                g = g0 + 2 + k  # the gene this assembly's edit lies in
                s, e = int(db.gene_intervals.starts[g]), int(db.gene_intervals.ends[g])
                seq = {"exact": lambda: ref, "snp": lambda: _flip(ref, (s + e) // 2 + 1), "lacking": lambda: np.concatenate([ref[:s], ref[e:]]),
                       "far": lambda: mutate(rng, ref, 0.01)}[kind]()  # fmt: skip
                name = f"L{L}_{kind}_{k}"
                self.plan[name] = (L, kind, g)
                genomes.append(_genome(name, rng, seq))
        order = rng.permutation(len(genomes))  # the loci interleaved: a locus's rows come from both batches
        self.genomes = [genomes[i] for i in order]
        self.ids = [g.id for g in self.genomes]
        self.typer = Serotyper(db, distances=True)
        eng = self.typer.engine
        codes, off = pack_sequences_flat(db.genes)
        self.want_rows, self.bts = LocusRows(db), []
        for part in (self.genomes[:7], self.genomes[7:]):
            packed = [g.packed() for g in part]
            batch = eng.ctx.batch(packed)
            bt = eng.type_batch(self.typer, batch, [g.id for g in part], part)
            restated = restate_batch(bt, *batch.hits(), *batch.cigars(), codes, off, packed)
            self.want_rows.add(SimpleNamespace(ids=bt.ids, sums=bt.sums, kept=bt.kept, best_locus=bt.best_locus, aligned=lambda r=restated: r))
            self.bts.append((bt, restated))
            batch.close()
        self.tsv = b"".join(bt.tsv() for bt, _ in self.bts)

    def close(self):
        self.typer.engine.close()


def _write_inputs(db, genomes, tmp_path):
    paths = []
    for g in genomes:
        p = tmp_path / f"{g.id}.fasta"
        p.write_bytes(g.contigs.to_fasta())
        paths.append(str(p))
    return str(db.save(tmp_path / "k.npz")), paths


def _count_handles(monkeypatch):
    made = []
    init = _native.Distances.__init__

    def counting(self, ctx, rows_matrix):
        made.append(np.asarray(rows_matrix).shape)
        init(self, ctx, rows_matrix)

    monkeypatch.setattr(_native.Distances, "__init__", counting)
    return made
