"""K and O in one pass (``kaptive_amd assembly ... --db``, ``MultiSerotyper``, ``Engine.type_stream_groups``): every report
of a run with two databases holds exactly the bytes of two runs with one database each."""

import gzip
import subprocess
import sys
from pathlib import Path

import pytest

from kaptive_amd.synth import make_assembly, make_db

ROOT = Path(__file__).resolve().parent.parent
N_ASM = 11
FLAGS = ("-l", "-g", "-p")


def _inputs(root: Path):
    """A K and an O database (saved), and N_ASM assemblies with a locus of each: one with neither, three gzip-compressed,
    N runs in every third.  Returns (db_k, db_o, k_path, o_path, fasta paths)."""
    db_k, db_o = make_db("kpsc_k", seed=7, n_loci=9), make_db("kpsc_o", seed=8)
    k_path, o_path = db_k.save(root / "k.npz"), db_o.save(root / "o.npz")
    paths = []
    for i in range(N_ASM):
        neither = i == 4
        g = make_assembly(db_k, seed=3100 + i, name=f"asm{i:02d}", length=300_000 + 10_000 * i, median_contigs=3 + i % 4,
                          n_run=10 * (i % 3), locus=-1 if neither else None, sub_rate=0.002 * (i % 4),
                          also=() if neither else (db_o,))  # fmt: skip
        data = g.contigs.to_fasta()
        p = root / f"asm{i:02d}.fasta{'.gz' if i % 4 == 1 else ''}"
        p.write_bytes(gzip.compress(data) if i % 4 == 1 else data)
        paths.append(str(p))
    return db_k, db_o, str(k_path), str(o_path), paths


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    return _inputs(tmp_path_factory.mktemp("multi_db"))


def _tree(d: Path) -> dict:
    return {p.relative_to(d).as_posix(): p.read_bytes() for p in sorted(d.rglob("*")) if p.is_file()}


def _run(args, cwd=ROOT):
    """The command line as a user runs it (a process of its own: --devices spawns workers that re-import __main__)."""
    r = subprocess.run([sys.executable, "-m", "kaptive_amd", "assembly", *args], capture_output=True, timeout=600, cwd=str(cwd))
    assert r.returncode == 0, r.stderr[-2000:].decode(errors="replace")
    return r.stdout


@pytest.mark.gpu
def test_one_pass_writes_what_two_single_database_runs_write(inputs, tmp_path):
    from kaptive_amd.cli import main

    db_k, db_o, k_path, o_path, paths = inputs
    common = ["--batch-size", "3", "-t", "3"]

    def outputs(d: Path) -> list:
        d.mkdir()
        return ["-o", str(d / "r.tsv"), "--pha4ge", str(d / "r.pha4ge"), "-j", str(d / "r.jsonl"),
                *[x for flag, sub in zip(FLAGS, ("loci", "genes", "prot")) for x in (flag, str(d / sub))]]  # fmt: skip

    alone = {}
    for kw, db_path in (("kpsc_k", k_path), ("kpsc_o", o_path)):
        d = tmp_path / f"alone_{kw}"
        assert main(["assembly", db_path, *paths, *outputs(d), *common]) == 0
        alone[kw] = d
    both = tmp_path / "both"
    assert main(["assembly", k_path, *paths, "--db", o_path, *outputs(both), *common]) == 0
    for kw, d in alone.items():
        for name, ext in (("r", "tsv"), ("r", "pha4ge"), ("r", "jsonl")):
            got = (both / f"{name}.{kw}.{ext}").read_bytes()
            assert got == (d / f"{name}.{ext}").read_bytes(), f"{kw} .{ext}"
        for sub in ("loci", "genes", "prot"):
            want = _tree(d / sub)
            assert len(want) == N_ASM and _tree(both / sub / kw) == want, f"{kw} {sub}"
    assert sorted(p.name for p in both.iterdir()) == sorted(
        [f"r.{kw}.{ext}" for kw in alone for ext in ("tsv", "pha4ge", "jsonl")] + ["loci", "genes", "prot"])
    tsv = {kw: (d / "r.tsv").read_bytes().splitlines(keepends=True) for kw, d in alone.items()}
    for kw, rows in tsv.items():
        assert len(rows) == 1 + N_ASM and [r.split(b"\t")[3] for r in rows[1:]] == [f"asm{i:02d}".encode() for i in range(N_ASM)]
        assert sum(b"\tTypeable\t" in r for r in rows[1:]) >= 3, f"{kw}: too few typeable assemblies to compare"

    # the TSV-only path (no object, no text kept: kp_fasta_ingest_shard, kp_format_rows) writes the same bytes
    fast = tmp_path / "fast"
    fast.mkdir()
    assert main(["assembly", k_path, *paths, "--db", o_path, "-o", str(fast / "r.tsv"), "--batch-size", "3"]) == 0
    for kw in alone:
        assert (fast / f"r.{kw}.tsv").read_bytes() == b"".join(tsv[kw])

    # stdout: one header, then every genome's K row and O row, in input order
    out = _run([k_path, *paths, "--db", o_path, "--batch-size", "3"])
    want = [tsv["kpsc_k"][0]] + [row for pair in zip(tsv["kpsc_k"][1:], tsv["kpsc_o"][1:]) for row in pair]
    assert out.splitlines(keepends=True) == want

    # two device processes on the one GPU: chunks dealt round-robin, every database's rows written in input order
    two = tmp_path / "two"
    two.mkdir()
    _run([k_path, *paths, "--db", o_path, "-o", str(two / "r.tsv"), "-j", str(two / "r.jsonl"), "--batch-size", "3",
          "--devices", "0,0", "-t", "2"])  # fmt: skip
    for kw, d in alone.items():
        assert (two / f"r.{kw}.tsv").read_bytes() == b"".join(tsv[kw])
        assert (two / f"r.{kw}.jsonl").read_bytes() == (d / "r.jsonl").read_bytes()


@pytest.mark.gpu
def test_multi_serotyper_equals_one_serotyper_per_database(inputs):
    from kaptive_amd.cli import result_to_json
    from kaptive_amd.serotyping import MultiSerotyper, Serotyper
    from kaptive_amd.serotyping.io import KaptiveRow

    db_k, db_o, _, _, paths = inputs
    multi = MultiSerotyper([db_k, db_o])
    assert all(s._db is d for s, d in zip(multi.serotypers, (db_k, db_o)))
    together = multi.type_many(paths)
    assert len(together) == N_ASM and all(len(t) == 2 for t in together)
    chunks = list(multi.tsv_from_files(paths, batch_size=3, threads=2))
    one = multi(paths[0])
    ctx = multi.engine.ctx
    assert all(s.engine.ctx is ctx for s in multi.serotypers)  # one context for both databases
    multi.close()
    assert multi._engine is None and ctx._h is None
    for i, db in enumerate((db_k, db_o)):
        typer = Serotyper(db)
        alone = typer.type_many(paths)
        for a, (want, got) in enumerate(zip(alone, (t[i] for t in together))):
            assert result_to_json(got) == result_to_json(want), (db.metadata.keyword, paths[a])
            assert bytes(KaptiveRow.from_result(got)) == bytes(KaptiveRow.from_result(want))
        assert result_to_json(one[i]) == result_to_json(alone[0])
        assert sum(r.typeable for r in alone) >= 3, f"{db.metadata.keyword}: too few typeable assemblies to compare"
        single_chunks = list(typer.tsv_from_files(paths, batch_size=3, threads=2))
        assert len(chunks) == len(single_chunks) == 4  # the last one ragged
        assert [c[i] for c in chunks] == single_chunks, db.metadata.keyword
        typer.engine.close()


@pytest.mark.gpu
def test_type_stream_groups_equals_type_stream_per_group(inputs):
    """The engine's window over every group: more batches than WORK_SLOTS, each group's records those of type_stream
    over that group's view of the same engine."""
    from kaptive_amd import _native
    from kaptive_amd.core.genome import GenomeAssembly
    from kaptive_amd.engine import Engine
    from kaptive_amd.serotyping.core import Serotyper

    db_k, db_o, _, _, paths = inputs
    genomes = [GenomeAssembly.from_file(p) for p in paths]
    typers = [Serotyper(db_k), Serotyper(db_o)]
    engine = Engine([db_k, db_o])
    groups_of = [genomes[i : i + 2] for i in range(0, N_ASM, 2)]
    assert len(groups_of) > _native.WORK_SLOTS

    def source():
        for gs in groups_of:
            yield engine.ctx.batch([g.packed() for g in gs]), [g.id for g in gs], gs

    got = []
    for bts, batch in engine.type_stream_groups(typers, source()):
        got.append([(bt.tsv(), bt.jsonl()) for bt in bts])
        batch.close()
    for g, typer in enumerate(typers):
        want = []
        for bt, batch in engine.view(g).type_stream(typer, source()):
            want.append((bt.tsv(), bt.jsonl()))
            batch.close()
        assert [row[g] for row in got] == want, f"group {g}"
    with pytest.raises(ValueError):
        next(engine.type_stream_groups(typers[:1], source()))
    engine.close()
