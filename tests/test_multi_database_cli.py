"""Several databases in one ``kaptive_amd assembly`` run (``--db``), the parts that need no GPU: parsing, how the reports
are named and laid out per database, and the refusals that come before any typing."""

import re
from pathlib import Path

import pytest

from kaptive_amd import _native
from kaptive_amd.cli import _PerDatabaseOutputs, build_parser, interleave_lines, main, per_database_path
from kaptive_amd.serotyping.io import KaptiveRow, Pha4geRow
from kaptive_amd.synth import make_assembly

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"


def test_db_option_repeats_in_the_order_given():
    ap = build_parser()
    a = ap.parse_args(["assembly", "k.gbk", "a.fasta", "b.fasta.gz", "--db", "o.gbk", "-o", "r.tsv", "--db", "x.npz"])
    assert a.database == "k.gbk" and a.db == ["o.gbk", "x.npz"] and a.genomes == ["a.fasta", "b.fasta.gz"] and a.out == "r.tsv"
    b = ap.parse_args(["type", "k.gbk", "--db", "o.gbk", "a.fasta"])
    assert b.database == "k.gbk" and b.db == ["o.gbk"] and b.genomes == ["a.fasta"]
    with pytest.raises(SystemExit):
        ap.parse_args(["convert", "r.jsonl", "--db", "o.gbk"])  # convert reads results, not databases


def test_without_db_the_namespace_is_unchanged():
    ap = build_parser()
    a = ap.parse_args(["assembly", "db.npz", "a.fasta", "-o", "out.tsv", "-j", "-l", "loci", "--batch-size", "3"])
    got = vars(a)
    assert got.pop("db") is None
    assert got.pop("func").__name__ == "run_type"
    assert got == {"command": "assembly", "database": "db.npz", "genomes": ["a.fasta"], "out": "out.tsv", "loci": Path("loci"),
                   "genes": None, "proteins": None, "json": "kaptive_results.jsonl", "pha4ge": None, "max_other_genes": 1,
                   "min_completeness": 0.5, "below_threshold": False, "threads": 0, "partial_edge_tolerance": 5, "devices": "0",
                   "batch_size": 3, "verbose": False}  # fmt: skip


def test_per_database_file_names():
    assert per_database_path("results.tsv", "kpsc_k") == "results.kpsc_k.tsv"
    assert per_database_path("out.d/results", "kpsc_o") == "out.d/results.kpsc_o"  # no suffix: the keyword is appended
    assert per_database_path("runs/r.tar.gz", "ab_k") == "runs/r.tar.ab_k.gz"  # before the last suffix
    ns = build_parser().parse_args(["assembly", "db.npz", "a.fasta", "-j", "--pha4ge"])  # the defaults of -j and --pha4ge
    assert per_database_path(ns.json, "kpsc_k") == "kaptive_results.kpsc_k.jsonl"
    assert per_database_path(ns.pha4ge, "kpsc_o") == "kaptive_results.kpsc_o.pha4ge"


def _chunk(n, keywords):
    """What the pipeline hands ``run_type`` for one chunk of ``n`` assemblies: ((keyword, {report: bytes}), ...)."""
    return tuple(
        (kw, {"tsv": b"".join(b"%s\tasm%d\ttsv\n" % (kw.encode(), i) for i in range(n)),
              "pha4ge": b"".join(b"%s\tasm%d\tpha4ge\n" % (kw.encode(), i) for i in range(n)),
              "json": b"".join(b'{"db":"%s","genome":"asm%d"}\n' % (kw.encode(), i) for i in range(n))})
        for kw in keywords
    )  # fmt: skip


def test_reports_go_to_one_file_per_database(tmp_path):
    ns = build_parser().parse_args(["assembly", "db.npz", "a.fasta", "--db", "o.npz", "-o", str(tmp_path / "results.tsv"),
                                    "--pha4ge", str(tmp_path / "rep"), "-j", str(tmp_path / "r.jsonl")])  # fmt: skip
    out = _PerDatabaseOutputs(ns)
    for n in (3, 2):
        out.write(_chunk(n, ("kpsc_k", "kpsc_o")))
    out.close()
    for kw in ("kpsc_k", "kpsc_o"):
        one = [_chunk(n, (kw,))[0][1] for n in (3, 2)]
        assert (tmp_path / f"results.{kw}.tsv").read_bytes() == KaptiveRow.header() + b"".join(o["tsv"] for o in one)
        assert (tmp_path / f"rep.{kw}").read_bytes() == Pha4geRow.header() + b"".join(o["pha4ge"] for o in one)
        assert (tmp_path / f"r.{kw}.jsonl").read_bytes() == b"".join(o["json"] for o in one)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(
        ["results.kpsc_k.tsv", "results.kpsc_o.tsv", "rep.kpsc_k", "rep.kpsc_o", "r.kpsc_k.jsonl", "r.kpsc_o.jsonl"])


def test_stdout_gets_one_header_then_every_database_per_genome(capsysbinary):
    ns = build_parser().parse_args(["assembly", "db.npz", "a.fasta", "--db", "o.npz"])  # -o defaults to stdout
    out = _PerDatabaseOutputs(ns)
    out.write(_chunk(3, ("kpsc_k", "kpsc_o")))
    out.write(_chunk(1, ("kpsc_k", "kpsc_o")))
    out.close()
    lines = capsysbinary.readouterr().out.splitlines(keepends=True)
    assert lines[0] == KaptiveRow.header()
    want = [b"%s\tasm%d\ttsv\n" % (kw, i) for i in range(3) for kw in (b"kpsc_k", b"kpsc_o")]
    want += [b"kpsc_k\tasm0\ttsv\n", b"kpsc_o\tasm0\ttsv\n"]
    assert lines[1:] == want


def test_interleave_is_a_zip_of_the_lines():
    assert interleave_lines([b"k1\nk2\n", b"o1\no2\n", b"x1\nx2\n"]) == b"k1\no1\nx1\nk2\no2\nx2\n"
    assert interleave_lines([b"", b""]) == b""
    assert interleave_lines([b"only\n"]) == b"only\n"
    with pytest.raises(RuntimeError):
        interleave_lines([b"k1\nk2\n", b"o1\n"])  # every database has a line for every assembly


def _genome(tmp_path) -> str:
    from kaptive_amd.db import Database

    g = make_assembly(Database.load(GOLDEN / "db_k.npz"), seed=5, length=40_000, median_contigs=3, name="g1")
    p = tmp_path / "g1.fasta"
    p.write_bytes(g.contigs.to_fasta())
    return str(p)


def test_the_same_keyword_twice_is_refused_before_any_typing(tmp_path, capsys):
    db_k = str(GOLDEN / "db_k.npz")
    out = tmp_path / "results.tsv"
    assert main(["assembly", db_k, _genome(tmp_path), "--db", db_k, "-o", str(out)]) == 1
    err = capsys.readouterr().err
    assert "kpsc_k" in err and "twice" in err
    assert list(tmp_path.glob("results*")) == []  # nothing was written


def test_more_genes_than_one_pass_holds_is_refused(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(_native, "MAX_GENES", 300)  # db_k 228 + db_o 125 genes
    assert main(["assembly", str(GOLDEN / "db_k.npz"), _genome(tmp_path), "--db", str(GOLDEN / "db_o.npz"),
                 "-o", str(tmp_path / "r.tsv")]) == 1  # fmt: skip
    err = capsys.readouterr().err
    assert "353 genes" in err and "KP_MAX_GENES" in err


def test_pass_limits_match_the_headers():
    spec = (ROOT / "include" / "kp_spec.h").read_text()
    api = (ROOT / "include" / "kaptive_amd.h").read_text()
    assert int(re.search(r"#define\s+KP_MAX_GENES\s+(\d+)", spec).group(1)) == _native.MAX_GENES
    assert int(re.search(r"#define\s+KP_MAX_TYPING_GROUPS\s+(\d+)", api).group(1)) == _native.MAX_TYPING_GROUPS
