"""The typing pipeline (``kaptive_amd/pipeline.py``) on the device, through its two callers: three chunks of 2, 2 and 1 assemblies
go through the typing window (a buffer given back early, buffers reused), and the bytes are those of ``type_many``."""

import gzip

import pytest

from kaptive_amd import _native
from kaptive_amd.serotyping import MultiSerotyper, Serotyper
from kaptive_amd.serotyping.io import KaptiveRow
from kaptive_amd.synth import make_assembly, make_db

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    """The 3-locus K database, an O database, and five assemblies of 90-110 kb as files (the second gzip-compressed)."""
    root = tmp_path_factory.mktemp("gpu_pipeline")
    db, db_o = make_db("kpsc_k", seed=7, n_loci=3), make_db("kpsc_o", seed=8)
    paths = []
    for i in range(5):
        data = make_assembly(db, seed=500 + i, name=f"asm{i}", length=90_000 + 5_000 * i, median_contigs=3 + i, n_run=6 * (i % 2), also=(db_o,)).contigs.to_fasta()
        p = root / f"asm{i}.fasta{'.gz' if i == 1 else ''}"
        p.write_bytes(gzip.compress(data) if i == 1 else data)
        paths.append(str(p))
    return db, db_o, str(db.save(root / "k.npz")), paths


def test_tsv_from_files_equals_type_many(inputs):
    db, _, _, paths = inputs
    typer = Serotyper(db)
    try:
        chunks = list(typer.tsv_from_files(paths, batch_size=2))
        want = [bytes(KaptiveRow.from_result(r)) for r in typer.type_many(paths)]
    finally:
        typer.engine.close()
    assert [c.count(b"\n") for c in chunks] == [2, 2, 1] and b"".join(chunks) == b"".join(want)
    assert [row.split(b"\t")[3] for row in want] == [f"asm{i}".encode() for i in range(5)]


def test_multi_tsv_from_files_equals_type_many_per_database(inputs):
    db, db_o, _, paths = inputs
    multi = MultiSerotyper([db, db_o])
    try:
        chunks = list(multi.tsv_from_files(paths, batch_size=2))
        want = multi.type_many(paths)
    finally:
        multi.close()
    assert [tuple(block.count(b"\n") for block in c) for c in chunks] == [(2, 2), (2, 2), (1, 1)]
    for d in range(2):
        assert b"".join(c[d] for c in chunks) == b"".join(bytes(KaptiveRow.from_result(per_db[d])) for per_db in want), d


def test_cli_object_path_and_shard_path_write_the_same_tsv(inputs, tmp_path):
    from kaptive_amd.cli import main

    _, _, db_path, paths = inputs
    objects, shard = tmp_path / "objects.tsv", tmp_path / "shard.tsv"
    assert main(["assembly", db_path, *paths, "--batch-size", "2", "-o", str(objects), "-j", str(tmp_path / "r.jsonl")]) == 0
    assert main(["assembly", db_path, *paths, "--batch-size", "2", "-o", str(shard)]) == 0
    assert objects.read_bytes() == shard.read_bytes() and shard.read_bytes().count(b"\n") == 1 + len(paths)
    assert (tmp_path / "r.jsonl").read_bytes().count(b"\n") == len(paths)


@pytest.mark.parametrize("outputs", [{"tsv": True}, {"tsv": True, "json": True}], ids=["shard", "objects"])
def test_a_closed_pipeline_holds_no_page_locked_memory(inputs, outputs):
    from kaptive_amd.pipeline import PipelineOptions, TypingPipeline

    _, _, db_path, paths = inputs
    chunks = [(k, paths[i : i + 2]) for k, i in enumerate(range(0, len(paths), 2))]
    before = _native.pinned_bytes()
    pipe = TypingPipeline(PipelineOptions(**outputs), 0, databases=[db_path], chunks=chunks)
    try:
        during = [_native.pinned_bytes() for _ in pipe.run(chunks)]
        assert pipe.pins.held == {} and len(pipe.pins.kept) <= TypingPipeline.PREFETCH + 1  # every batch's buffer came back
    finally:
        pipe.close()
    assert len(during) == 3 and max(during) > before
    assert _native.pinned_bytes() == before
