"""Shared by tests/test_rescue_cpu.py and tests/test_gpu_rescue.py: the yardstick of the rescue records (include/kp_spec.h, RESCUE) --
every frame text built with the reference-pinned ``oracle.extract`` + ``oracle.translate``, every alignment made by the
reference-pinned ``oracle.protein_align_seeded`` with a band that covers the whole rectangle, the tie rule and the derived fields
applied in plain Python --, the restatement of the table's formatter, and the helpers that plant a gene no nucleotide seed can find.
TEST INFRASTRUCTURE."""

from __future__ import annotations

import ctypes as C
from functools import lru_cache

import numpy as np

from oracle import oracle

RESCUE_DTYPE = np.dtype(
    [("gene", "<i4"), ("piece", "<i4"), ("contig", "<i4"), ("t_start", "<i4"), ("t_end", "<i4"), ("score", "<i4"), ("matches", "<i4"),
     ("mismatches", "<i4"), ("gaps", "<i4"), ("p_start", "<i4"), ("p_end", "<i4"), ("stops", "<i4"), ("a_len", "<i4"), ("strand", "i1"),
     ("frame", "u1"), ("edge", "u1"), ("pad", "u1")]
)  # fmt: skip
HEADER = b"\t".join([b"Assembly", b"Locus", b"Gene", b"Protein length", b"Call", b"Score", b"Contig", b"Start", b"End", b"Strand", b"Frame",
                     b"Protein start", b"Protein end", b"Matches", b"Mismatches", b"Gaps", b"Identity", b"Coverage", b"Stops", b"Edge"]) + b"\n"  # fmt: skip
FLANK, FLANK_MAX, MIN_SCORE = 4096, 65535, 80
MAX_LOCUS_GENES = 256
# columns of the protein a wave of the fill kernel holds with 2, 4 and 6 columns per lane (kp_rescue.h: KP_RS_LANES x KP_RS_NC_*): a
# protein beyond the last is cut into strips of that width.  Change them together.  (The rows a wave takes per turn, 64 = KP_RS_LANES,
# and the residues of its LDS ring, 128, are restated in tests/rescue_paths_util.py as ROW_CHUNK and RING;
# tests/test_rescue_paths_cpu.py ties them to the header.)
STRIP_LIMITS = (128, 256, 384)


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------------
def contig_texts(pa) -> list:
    """The contigs of a packed assembly as upper-case text, N inside the N runs."""
    from tests.cigar_util import assembly_codes

    codes = assembly_codes(pa)
    letters = np.frombuffer(b"ACGTN", np.uint8)
    return [np.ascontiguousarray(letters[codes[int(s) : int(s) + int(n)]]) for s, n in zip(pa.ctg_start, pa.ctg_len)]


def window(start: int, end: int, ctg_len: int, flank: int) -> tuple[int, int]:
    return max(0, start - flank), min(ctg_len, end + flank)


def frame_text(contig: np.ndarray, ws: int, we: int, strand: int, f: int) -> np.ndarray:
    """oracle.translate(oracle.extract(window, strand), frame f, to_stop=False)."""
    if we <= ws:
        return np.zeros(0, np.uint8)
    seq, _, _ = oracle.extract(contig, [0], [0], [ws], [we], [strand])
    out, _, n = oracle.translate(seq, [0], [len(seq)], [f], False)
    return np.ascontiguousarray(out[: int(n[0])])


def align(text: np.ndarray, prot: np.ndarray) -> np.ndarray:
    """The eight values of the reference's kernel with a band over the whole rectangle; zeros where a side is empty."""
    if len(text) == 0 or len(prot) == 0:
        return np.zeros(8, np.int32)
    return oracle.protein_align_seeded(text, [0], [len(text)], prot, [0], [len(prot)], [0], k=len(text) + len(prot))[0]


def subjects(summary) -> list:
    if int(summary["overflow"]) & 4:
        return []
    mask = summary["missing_mask"]
    return [j for j in range(MAX_LOCUS_GENES) if (int(mask[j >> 6]) >> (j & 63)) & 1]


def protein(db, gene: int) -> np.ndarray:
    t = db.translations
    return np.ascontiguousarray(t.seqs[int(t.offsets[gene]) : int(t.offsets[gene]) + int(t.lengths[gene])], np.uint8)


def restate(summary, pieces, pa, db, flank: int, tol: int) -> np.ndarray:
    """The records of one assembly from its summary and its pieces (the first n_pieces rows of the device's table)."""
    texts = contig_texts(pa)
    g0 = int(db.locus_gene_offsets[int(summary["best_locus"])])
    frames = []  # task index within a subject -> (piece, contig, ws, we, strand, f, text)
    for p, pc in enumerate(pieces):
        c = int(pc["contig"])
        ws, we = window(int(pc["start"]), int(pc["end"]), len(texts[c]), flank)
        for strand in (1, -1):
            for f in range(3):
                frames.append((p, c, ws, we, strand, f, frame_text(texts[c], ws, we, strand, f)))
    out = np.zeros(len(subjects(summary)), RESCUE_DTYPE)
    for r, j in zip(out, subjects(summary)):
        r["gene"], r["piece"] = g0 + j, -1
        prot = protein(db, g0 + j)
        best, at = None, None
        for task, fr in enumerate(frames):
            assert task == (fr[0] * 2 + (fr[4] < 0)) * 3 + fr[5]
            res = align(fr[6], prot)
            assert max(0, (fr[3] - fr[2] - fr[5]) // 3) == len(fr[6])
            if int(res[0]) > (int(best[0]) if best is not None else 0):
                best, at = res, fr
        if best is None:
            continue
        p, c, ws, we, strand, f, text = at
        score, m, mm, gaps, a0, a1, p0, p1 = (int(x) for x in best)
        t0, t1 = (ws + f + 3 * a0, ws + f + 3 * a1) if strand > 0 else (we - f - 3 * a1, we - f - 3 * a0)
        r["piece"], r["contig"], r["t_start"], r["t_end"] = p, c, t0, t1
        r["score"], r["matches"], r["mismatches"], r["gaps"], r["p_start"], r["p_end"] = score, m, mm, gaps, p0, p1
        r["stops"], r["a_len"], r["strand"], r["frame"] = int((text[a0:a1] == ord("*")).sum()), len(text), strand, f
        r["edge"] = (1 if t0 <= tol else 0) | (2 if t1 >= len(texts[c]) - tol else 0)
    return out


def restate_batch(sums, pieces, packed, db, flank: int, tol: int):
    """(records, rescue_off) of a batch from the device's own summaries and pieces."""
    recs = [restate(sums[a], pieces[a, : int(sums["n_pieces"][a])], pa, db, flank, tol) for a, pa in enumerate(packed)]
    off = np.concatenate([[0], np.cumsum([len(r) for r in recs])]).astype(np.int64)
    return (np.concatenate(recs) if recs else np.zeros(0, RESCUE_DTYPE)), off


def call(r, plen: int, min_score: int) -> bytes:
    short = (int(r["p_end"]) - int(r["p_start"])) * 100 < 90 * plen
    if int(r["score"]) < min_score:
        return b"absent"
    if int(r["stops"]) - (1 if int(r["score"]) > 0 and plen > 0 and int(r["p_end"]) == plen else 0) > 0:  # (the gene's own stop, aligned to the protein's *, interrupts nothing)
        return b"interrupted"
    if short:
        return b"partial" if int(r["edge"]) else b"fragment"
    return b"diverged"


def tsv(records, rescue_off, asm_names, contig_names, gene_names, locus_names, best_locus, prot_len, min_score: int = MIN_SCORE) -> bytes:
    """The table's lines; ``contig_names[a]`` lists assembly a's contigs."""
    lines = []
    for a in range(len(rescue_off) - 1):
        for r in records[int(rescue_off[a]) : int(rescue_off[a + 1])]:
            plen, found = int(prot_len[int(r["gene"])]), int(r["score"]) > 0
            cols = int(r["matches"]) + int(r["mismatches"]) + int(r["gaps"])
            where = ([contig_names[a][int(r["contig"])], int(r["t_start"]) + 1, int(r["t_end"]), "+" if int(r["strand"]) > 0 else "-", int(r["frame"]) + 1,
                      int(r["p_start"]) + 1, int(r["p_end"])] if found else ["."] * 7)  # fmt: skip
            ident = "%.2f" % (int(r["matches"]) * 100 / cols if cols else 0.0)
            cov = "%.2f" % ((int(r["p_end"]) - int(r["p_start"])) * 100 / plen if plen else 0.0)
            edge = {0: ".", 1: "start", 2: "end", 3: "both"}[int(r["edge"])] if found else "."
            fields = [asm_names[a], locus_names[int(best_locus[a])], gene_names[int(r["gene"])], plen, call(r, plen, min_score).decode(), int(r["score"]), *where,
                      int(r["matches"]), int(r["mismatches"]), int(r["gaps"]), ident, cov, int(r["stops"]), edge]  # fmt: skip
            lines.append("\t".join(str(x) for x in fields).encode() + b"\n")
    return b"".join(lines)


# ---- kp_rescue.h on host arrays (tests/native_harness/rescue_harness.cpp) ---------------------------------------------------------------
@lru_cache(maxsize=1)
def harness() -> C.CDLL:
    from tests.harness_util import build_harness

    return build_harness("rescue_harness", "kp_rescue.h")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def harness_text(pa, contig: int, ws: int, we: int, strand: int, f: int) -> np.ndarray:
    words, runs = np.ascontiguousarray(pa.words, np.uint32), np.ascontiguousarray(pa.n_runs, np.int32).reshape(-1)
    out = np.full(max(1, (we - ws) // 3 + 2), 0x7E, np.uint8)
    n = harness().kpy_rs_text(_p(words), C.c_int(len(words)), _p(runs), C.c_int(len(runs) // 2), C.c_int(int(pa.ctg_start[contig])),
                              C.c_int(int(pa.ctg_len[contig])), C.c_int(ws), C.c_int(we), C.c_int((3 if strand < 0 else 0) + f), _p(out))  # fmt: skip
    assert n >= 0, "the shortcut for windows clear of N runs disagrees with the searched run list"
    assert (out[n:] == 0x7E).all()
    return out[:n].copy()


# ---- planting ---------------------------------------------------------------------------------------------------------------------------
from kaptive_amd.synth import CODONS  # noqa: E402
from kaptive_amd.synth import recode_orf as recode  # noqa: E402  (the gene no nucleotide seed can find: codon by codon, a quarter of the residues substituted)


def shares_kmer(a: np.ndarray, b: np.ndarray, k: int = 15) -> bool:
    from kaptive_amd.synth import revcomp

    grams = {bytes(a[i : i + k]) for i in range(len(a) - k + 1)}
    return any(bytes(x[i : i + k]) in grams for x in (b, revcomp(b)) for i in range(len(x) - k + 1))


PLANT_LOCUS, PLANT_GENE, PLANT_LONG = 0, 2, 3  # the locus, the edited gene (241 residues) and one whose protein needs strips (498)


def plant_db():
    from kaptive_amd.synth import make_db

    return make_db("kpsc_o", seed=8)


def plants(db):
    """{name: (genome, database index of the edited gene, expectation)}: locus PLANT_LOCUS cut into contigs of two genes each -- every
    window is then clipped by its contig and the yardstick's band arrays stay small --, with ONE gene edited.  Expectation: `found`
    (the record reaches MIN_SCORE) and, where it does, the table's call."""
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import random_dna, revcomp

    o, n = int(db.loci.offsets[PLANT_LOCUS]), int(db.loci.lengths[PLANT_LOCUS])
    locus = np.asarray(db.loci.seqs[o : o + n], np.uint8)
    g0, ng = int(db.locus_gene_offsets[PLANT_LOCUS]), int(db.locus_gene_lengths[PLANT_LOCUS])
    span = [(int(db.gene_intervals.starts[g0 + k]), int(db.gene_intervals.ends[g0 + k])) for k in range(ng)]
    assert all(db.gene_intervals.strands[g0 + k] > 0 for k in (PLANT_GENE, PLANT_LONG)), "the edited genes lie on the locus's forward strand"
    cuts = [0] + [(span[k][1] + span[k + 1][0]) // 2 for k in range(1, ng - 1, 2)] + [n]  # between genes 1|2, 3|4, ...
    rng = np.random.default_rng(20261020)

    def contigs(seq):
        """The locus text `seq` (same length as the locus) cut at `cuts`."""
        return [seq[a:b] for a, b in zip(cuts[:-1], cuts[1:])]

    def asm(name, parts):
        return GenomeAssembly(name, Sequences.from_records([SeqRecord(f"{name}_{i}", np.ascontiguousarray(c).tobytes()) for i, c in enumerate(parts)]))

    def edited(k, new):
        s, e = span[k]
        assert len(new) == e - s
        return np.concatenate([locus[:s], new, locus[e:]])

    s, e = span[PLANT_GENE]
    orf = locus[s:e]
    div = recode(rng, orf)
    assert not shares_kmer(orf, div)
    out = {}
    out["diverged"] = (asm("diverged", contigs(edited(PLANT_GENE, div))), g0 + PLANT_GENE, dict(found=True, call=b"diverged"))
    stop = div.copy()
    stop[300:303] = np.frombuffer(b"TAA", np.uint8)
    out["stop"] = (asm("stop", contigs(edited(PLANT_GENE, stop))), g0 + PLANT_GENE, dict(found=True, call=b"interrupted"))
    parts = contigs(edited(PLANT_GENE, div))
    same = [CODONS[bytes(div[i : i + 3]).decode()] == CODONS[bytes(orf[i : i + 3]).decode()] for i in range(0, len(orf), 3)]
    at = next(c for c in range(100, len(same) - 3) if all(same[c : c + 3]))  # (three residues the recoding kept: the alignment starts on the contig's first base)
    parts[1] = parts[1][s - cuts[1] + 3 * at :]  # the contig begins some hundred codons into the gene
    out["cut"] = (asm("cut", parts), g0 + PLANT_GENE, dict(found=True, call=b"partial"))
    out["reversed"] = (asm("reversed", [revcomp(c) for c in contigs(edited(PLANT_GENE, div))]), g0 + PLANT_GENE, dict(found=True, call=b"diverged"))
    out["deleted"] = (asm("deleted", contigs(edited(PLANT_GENE, random_dna(rng, e - s, 0.5)))), g0 + PLANT_GENE, dict(found=False))
    parts = contigs(edited(PLANT_GENE, random_dna(rng, e - s, 0.5)))
    parts[1] = np.concatenate([parts[1], div, random_dna(rng, 40, 0.5)])  # behind the contig's other gene
    out["relocated"] = (asm("relocated", parts), g0 + PLANT_GENE, dict(found=True, call=b"diverged"))
    parts = contigs(edited(PLANT_GENE, div))
    parts[2] = np.concatenate([random_dna(rng, 31, 0.5), div, parts[2]])  # the same copy in a later window: the earlier task wins
    out["two_copies"] = (asm("two_copies", parts), g0 + PLANT_GENE, dict(found=True, call=b"diverged", piece_contig=1))
    for k in range(16):
        parts = contigs(edited(PLANT_GENE, div))
        parts[1] = np.concatenate([random_dna(rng, k, 0.5), parts[1]])
        out[f"shift{k}"] = (asm(f"shift{k}", parts), g0 + PLANT_GENE, dict(found=True, call=b"diverged"))
    with_n = div.copy()
    with_n[200:223] = ord("N")
    out["n_run"] = (asm("n_run", contigs(edited(PLANT_GENE, with_n))), g0 + PLANT_GENE, dict(found=True))
    s3, e3 = span[PLANT_LONG]
    long_div = recode(rng, locus[s3:e3])
    assert not shares_kmer(locus[s3:e3], long_div)
    out["long"] = (asm("long", contigs(edited(PLANT_LONG, long_div))), g0 + PLANT_LONG, dict(found=True, call=b"diverged"))
    parts = contigs(edited(PLANT_GENE, div))
    parts[1] = np.concatenate([random_dna(rng, 5000, 0.5), parts[1], random_dna(rng, 5000, 0.5)])  # the default flank fits: nothing clips the window
    out["wide"] = (asm("wide", parts), g0 + PLANT_GENE, dict(found=True, call=b"diverged", unclipped=True))
    out["no_hit"] = (asm("no_hit", [random_dna(np.random.default_rng(99), 3000, 0.5)]), -1, dict(found=False))
    return out


# ---- shapes: a database whose proteins sit on both sides of every limit of the fill kernel ------------------------------------------------
SHAPE_PROTEINS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 1100)  # residues, the trailing * included
SHAPE_ANCHORS = (600, 450)  # bases of the two genes whose hand-made hits give the locus its pieces
SHAPE_FLANK = 3000


def shape_db():
    """One locus of two anchor genes and one gene per entry of SHAPE_PROTEINS, and a second locus of two genes."""
    from kaptive_amd.db import Database
    from kaptive_amd.synth import random_dna, random_orf

    rng = np.random.default_rng(384)
    loci = []
    for name, sizes in (("S1", [*SHAPE_ANCHORS, *(3 * n for n in SHAPE_PROTEINS)]), ("S2", [900, 750])):
        parts, genes, pos = [random_dna(rng, 60, 0.5)], [], 60
        for i, n in enumerate(sizes):
            orf = random_orf(rng, n, 0.5)
            parts += [orf, random_dna(rng, 40, 0.5)]
            genes.append(dict(start=pos, end=pos + n, strand=1, gene=f"{name.lower()}g{i}", product=f"shape {n}"))
            pos += n + 40
        loci.append(dict(name=name, type=name, extra=False, seq=np.concatenate(parts).tobytes(), genes=genes))
    meta = dict(name="shapes", keyword="shapes", genbank="shapes.gbk", organism="none", taxon=1, antigen="S", pathway="Wzx/Wzy", version="1",
                id_threshold=82.5, doi=[], owner="kaptive_amd", repo="synthetic", branch="main", contact={}, phenotype_logic={})  # fmt: skip
    return Database.from_parts(meta, loci)


def shape_gene(db, i: int) -> np.ndarray:
    """Bases of gene i of the shapes locus."""
    o = int(db.loci.offsets[0])
    return np.asarray(db.loci.seqs[o + int(db.gene_intervals.starts[i]) : o + int(db.gene_intervals.ends[i])], np.uint8)


def shape_assemblies(db):
    """([genome], [hit table]): `shapes` -- two contigs, an anchor gene with its hand-made hit on each, recoded copies of the 129-, the
    385- and (in two parts) the 1100-residue gene around them --, and `tiny1` .. `tiny5`, whose one hit spans 1 .. 5 bases of the
    contig: with rescue_flank 0 that is the window."""
    from kaptive_amd import _native
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.core.seq import SeqRecord, Sequences
    from kaptive_amd.synth import random_dna

    rng = np.random.default_rng(1100)
    idx = {n: 2 + i for i, n in enumerate(SHAPE_PROTEINS)}
    big = recode(rng, shape_gene(db, idx[1100]))
    c0 = np.concatenate([random_dna(rng, 100, 0.5), shape_gene(db, 0), random_dna(rng, 50, 0.5), recode(rng, shape_gene(db, idx[129])),
                         random_dna(rng, 7, 0.5), big[1500:2400], random_dna(rng, 30, 0.5)])  # fmt: skip
    c1 = np.concatenate([random_dna(rng, 60, 0.5), shape_gene(db, 1), random_dna(rng, 41, 0.5), recode(rng, shape_gene(db, idx[385])),
                         random_dna(rng, 11, 0.5), big[:1500]])  # fmt: skip (the contig ends with the fragment)

    def genome(name, contigs):
        return GenomeAssembly(name, Sequences.from_records([SeqRecord(f"{name}_{i}", np.ascontiguousarray(c).tobytes()) for i, c in enumerate(contigs)]))

    def hit(gene, contig, t_start, t_len):
        h = np.zeros(1, _native.HIT_DTYPE)
        L = int(db.genes.lengths[gene])
        h["gene"], h["contig"], h["strand"], h["q_start"], h["q_end"], h["t_start"], h["t_end"] = gene, contig, 1, 0, L, t_start, t_start + t_len
        h["score"], h["matches"], h["block_len"], h["mapq"] = 2 * L, L, L, 60
        return h

    genomes, tables = [genome("shapes", [c0, c1])], [np.concatenate([hit(0, 0, 100, SHAPE_ANCHORS[0]), hit(1, 1, 60, SHAPE_ANCHORS[1])])]
    for n in range(1, 6):
        genomes.append(genome(f"tiny{n}", [np.concatenate([random_dna(rng, 100, 0.5), shape_gene(db, 0), random_dna(rng, 50, 0.5)])]))
        tables.append(hit(0, 0, 100 + n, n))
    return genomes, tables
