"""Command line: ``python -m kaptive_amd type|assembly DATABASE GENOMES... -o out.tsv`` and ``convert``.

Same positionals and flags as the reference's ``kaptive type`` (alias ``assembly``) and ``kaptive convert``
(src/kaptive/serotyping/cli.py:118-267, shared output flags src/kaptive/cli.py:424-504), minus the plot output.  What
differs underneath: genomes are read and packed by a thread pool (``--threads`` is honoured; the reference parses and
ignores it) while earlier ones are being typed, in batches, on the GPU(s) (``--devices``: one process per
device; ``--batch-size``), and written in input order (``kaptive_amd/pipeline.py``: ``TypingPipeline``, which this
module gives its ``PipelineOptions``: ``pipeline_options``).
DATABASE is a ``.npz`` blob written by ``Database.save`` or a GenBank file with its ``.toml`` next to it.

``--db DATABASE`` (repeatable) adds databases to the same run: ``kaptive_amd assembly kpsc_k.gbk genomes/*.fasta --db
kpsc_o.gbk -o results.tsv`` reads every file once and types it against the positional database and then every ``--db``, in
the order given (one alignment pass over the genes of all of them, ``MultiSerotyper``).  Each database's reports hold
exactly the bytes a run with that database alone writes: files get the database's keyword before their last suffix
(``results.kpsc_k.tsv``, ``results.kpsc_o.tsv``; ``.<keyword>`` appended to a name without one), ``-l/-g/-p`` write into
``DIR/<keyword>/``, and a report on stdout has one header and then, genome by genome in input order, one line per database.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

import numpy as np

from kaptive_amd._native import REPORTS  # the tables derived from the kept lists: one row per report, every loop below goes over it
from kaptive_amd.pipeline import FILE_SUFFIX, LOCUS_ROWS_KEY, PipelineOptions, TypingPipeline, load_database

_KEEP: list = []  # FAST_EXIT: what must not be finalised one object at a time on the way out
FAST_EXIT = False  # set by __main__: the process ends right after main() returns, so nothing needs to be torn down in order
FAST_EXIT_ARMED = False  # set by run_type once its output handles are closed: only then may __main__ skip the interpreter's teardown


def result_to_json(result) -> bytes:
    """One JSON line per result, laid out as the reference's ``orjson.dumps(result.to_dict(), OPT_SERIALIZE_NUMPY |
    OPT_APPEND_NEWLINE)`` lays it out (src/kaptive/serotyping/cli.py:67-76): ``serotyping/jsonl.py``."""
    from kaptive_amd.serotyping.jsonl import dumps_line

    return dumps_line(result.to_dict())


class ResultExporter:
    """Fan-out of one result to every requested output (reference: src/kaptive/serotyping/cli.py:20-114)."""

    def __init__(self, args: argparse.Namespace) -> None:
        from kaptive_amd.serotyping.io import KaptiveRow, Pha4geRow

        self.handles, self.writers = [], []

        def stream(path):
            h = sys.stdout.buffer if _is_stdout(path) else open(path, "wb")
            self.handles.append(h)
            return h

        if tsv := (getattr(args, "out", None) or getattr(args, "tsv", None)):
            h = stream(tsv)
            h.write(KaptiveRow.header())
            self.writers.append(lambda r, h=h: h.write(bytes(KaptiveRow.from_result(r))))
        if p := getattr(args, "pha4ge", None):
            h = stream(p)
            h.write(Pha4geRow.header())
            self.writers.append(lambda r, h=h: h.write(bytes(Pha4geRow.from_result(r))))
        if j := getattr(args, "json", None):
            h = stream(j)
            self.writers.append(lambda r, h=h: h.write(result_to_json(r)))
        for flag, attr, ext in (("loci", "locus_seqs", "fna"), ("genes", "gene_seqs", "ffn"), ("proteins", "translations", "faa")):
            if d := getattr(args, flag, None):
                d = Path(d)
                d.mkdir(parents=True, exist_ok=True)
                self.writers.append(
                    lambda r, d=d, attr=attr, ext=ext: (d / f"{r.genome}_{FILE_SUFFIX}.{ext}").write_bytes(
                        getattr(r, attr).to_fasta()
                    )
                )

    def __call__(self, result) -> None:
        for w in self.writers:
            w(result)

    def close(self) -> None:
        for h in self.handles:
            if h is not sys.stdout.buffer:
                h.close()
            else:
                h.flush()


def _add_outputs(p: argparse.ArgumentParser, tsv_flags, include_json: bool) -> None:
    """Defaults, ``nargs`` and ``const`` follow the reference (src/kaptive/cli.py:424-504): ``-o`` defaults to stdout,
    ``convert -t`` without a value means stdout, ``-l/-g/-p`` without a value mean the current directory."""
    g = p.add_argument_group("Outputs")
    if tsv_flags[0] == "-o":
        g.add_argument(*tsv_flags, metavar="FILE", default="stdout",
                       help="Write serotyping results as a TSV report to a file (default: %(default)s)")
    else:
        g.add_argument(*tsv_flags, metavar="FILE", nargs="?", const="stdout",
                       help="Write serotyping results as a TSV report to a file (default: %(const)s)")
    g.add_argument("-l", "--loci", metavar="DIR", nargs="?", const="./", type=Path,
                   help="Write locus nucleotide fasta files to a directory (default: %(const)s)")
    g.add_argument("-g", "--genes", metavar="DIR", nargs="?", const="./", type=Path,
                   help="Write gene nucleotide fasta files to a directory (default: %(const)s)")
    g.add_argument("-p", "--proteins", metavar="DIR", nargs="?", const="./", type=Path,
                   help="Write translation amino-acid fasta files to a directory (default: %(const)s)")
    if include_json:
        g.add_argument("-j", "--json", metavar="FILE", nargs="?", const="kaptive_results.jsonl",
                       help="Write serialised results to a newline-delimited JSON (default: %(const)s)")
        g.add_argument("--paf", metavar="FILE", default=argparse.SUPPRESS,  # (absent from the namespace unless given)
                       help="Write every gene hit (before the overlap cull, in the aligner's order) with its CIGAR as PAF lines to a file")
        g.add_argument("--cs", action="store_true", default=argparse.SUPPRESS,
                       help="With --paf: add a cs:Z: tag (minimap2's short form) that lists the differing bases of every hit")
        g.add_argument("--eqx", action="store_true", default=argparse.SUPPRESS,
                       help="With --paf: write the CIGARs with = and X ops in place of M")
    if include_json:
        g.add_argument("--variants", metavar="FILE", default=argparse.SUPPRESS,
                       help="Write the variants of the reported gene hits -- substitutions with their codon consequence, insertions and "
                            "deletions, in gene coordinates -- as a TSV table to a file")
        g.add_argument("--breakpoints", metavar="FILE", default=argparse.SUPPRESS,
                       help="Write the genes that are split across two reported hits -- by an insertion sequence, a long deletion, an "
                            "inversion or a contig end -- with what lies between the fragments, as a TSV table to a file")
        g.add_argument("--alleles", metavar="FILE", default=argparse.SUPPRESS,
                       help="Write a stable 64-bit digest of every reported gene's bases and protein and of the whole locus -- equal "
                            "digests, equal alleles, across runs -- as a TSV table to a file")
        g.add_argument("--aligned", metavar="FILE", default=argparse.SUPPRESS,
                       help="Write every reported gene's contig bases in the coordinates of the database's gene -- one row of exactly "
                            "gene-length columns per hit, ready to stack into an alignment -- as a TSV table to a file")
        g.add_argument("--rescue", metavar="FILE", default=argparse.SUPPRESS,
                       help="Look for every gene reported as missing by aligning its protein against the six-frame translation of the "
                            "contig around the locus -- absent, or present but too diverged for a nucleotide seed -- and write one line "
                            "per missing gene as a TSV table to a file")
        g.add_argument("--rescue-flank", type=int, metavar="N", default=argparse.SUPPRESS,
                       help="With --rescue: bases either side of every locus piece that are searched (0 .. 65535; default: 4096)")
        g.add_argument("--rescue-min-score", type=int, metavar="N", default=argparse.SUPPRESS,
                       help="With --rescue: alignment score below which a gene is called absent (default: 80)")
    if include_json:
        g.add_argument("--distances", metavar="FILE", default=argparse.SUPPRESS,
                       help="Compare the loci of all assemblies that carry the same locus, all against all, and write the pairs that lie "
                            "within --max-distance differing bases of each other as a TSV table to a file")
        g.add_argument("--max-distance", type=int, metavar="N", default=argparse.SUPPRESS,
                       help="With --distances: most differing bases a listed pair may have (default: 10)")
        g.add_argument("--min-compared", type=int, metavar="N", default=argparse.SUPPRESS,
                       help="With --distances, --clusters, --mst, --newick or --nj: fewest columns both assemblies must hold a base in (default: 1)")
        g.add_argument("--clusters", metavar="FILE", default=argparse.SUPPRESS,
                       help="Group the assemblies that carry the same locus by single linkage at every one of --cluster-levels "
                            "differing bases, name every assembly's nearest neighbour, and write one line per assembly as a TSV "
                            "table to a file; no pair is listed for it")
        g.add_argument("--cluster-levels", metavar="T0,T1,...", default=argparse.SUPPRESS,
                       help="With --clusters: the thresholds, comma-separated, strictly ascending, at most 8 (default: 0,1,2,5,10)")
        g.add_argument("--mst", metavar="FILE", default=argparse.SUPPRESS,
                       help="Build the minimum spanning tree of the assemblies that carry the same locus, by differing bases, and "
                            "write its edges as a TSV table with the columns of --distances to a file; no pair is listed for it")
        g.add_argument("--newick", metavar="FILE", default=argparse.SUPPRESS,
                       help="The same trees as Newick text, one line per tree, as a TSV table to a file")
        g.add_argument("--nj", metavar="FILE", default=argparse.SUPPRESS,
                       help="Build the neighbour-joining tree, with inferred inner nodes, of the assemblies that carry the same locus "
                            "and hold a base in more than half of it, from the share of differing bases, and write it as Newick "
                            "text, one line per locus, as a TSV table to a file")
        g.add_argument("--nj-bootstrap", type=int, metavar="N", default=argparse.SUPPRESS,
                       help="With --nj: resample the columns of every locus N times (1 .. 10000), build every replicate's tree, and "
                            "label every inner branch with the number of replicate trees that hold it; the table gets a Replicates column")
        g.add_argument("--nj-seed", type=int, metavar="S", default=argparse.SUPPRESS,
                       help="With --nj-bootstrap: the seed of the resampling (default: 1); the same seed gives the same table")
        g.add_argument("--nj-transfer", action="store_true", default=argparse.SUPPRESS,
                       help="With --nj-bootstrap: label every inner branch with its transfer support instead, 0.000 .. 1.000: one "
                            "minus the share of its lighter side that must move, on average, for a replicate tree to hold it")
        g.add_argument("--nj-changes", metavar="FILE", default=argparse.SUPPRESS,
                       help="With --nj: put every base change on the branch of the tree where parsimony places it -- the branch by the "
                            "node below it, the gene position, the base on either end, read from the tree's last join, which is no "
                            "root -- as a TSV table to a file")
        g.add_argument("--nj-homoplasy", metavar="FILE", default=argparse.SUPPRESS,
                       help="With --nj: list the gene positions the tree needs a change for, with the changes it needs and how many of "
                            "them are beyond one per further base (Excess > 0: homoplasy, the signal of recombination), as a TSV "
                            "table to a file")
        g.add_argument("--sites", metavar="FILE", default=argparse.SUPPRESS,
                       help="List the gene positions at which the assemblies that carry the same locus hold different bases, with the "
                            "number of assemblies that carry each base there, as a TSV table to a file; no pair is looked at for it")
        g.add_argument("--snp-alignment", metavar="FILE", default=argparse.SUPPRESS,
                       help="Write every assembly's bases at those positions, one row of exactly as many columns as its locus has "
                            "sites, as a TSV table to a file")
        g.add_argument("--core-sites", action="store_true", default=argparse.SUPPRESS,
                       help="With --sites or --snp-alignment: only positions at which every assembly of the locus holds a base")
    g.add_argument("--pha4ge", metavar="FILE", nargs="?", const="kaptive_results.pha4ge", type=Path,
                   help="Write PHA4GE-compliant serotyping report to a TSV file (default: %(const)s)")


class _Parser(argparse.ArgumentParser):
    """Reports options that only make sense beside another one as argparse reports any other error."""

    def parse_known_args(self, args=None, namespace=None):
        ns, rest = super().parse_known_args(args, namespace)
        for flag in ("cs", "eqx"):
            if getattr(ns, flag, False) and not getattr(ns, "paf", None):
                self.error(f"--{flag} requires --paf FILE")
        for flag in ("rescue_flank", "rescue_min_score"):
            if getattr(ns, flag, None) is not None:
                if not getattr(ns, "rescue", None):
                    self.error(f"--{flag.replace('_', '-')} requires --rescue FILE")
                if getattr(ns, flag) < 0 or (flag == "rescue_flank" and ns.rescue_flank > 65535):
                    self.error(f"--{flag.replace('_', '-')} is out of range")
        for flag, beside in (("max_distance", ("distances",)), ("min_compared", ("distances", "clusters", "mst", "newick", "nj"))):
            if getattr(ns, flag, None) is not None:
                if not any(getattr(ns, b, None) for b in beside):
                    self.error(f"--{flag.replace('_', '-')} requires " + " or ".join(f"--{b} FILE" for b in beside))
                if not 0 <= getattr(ns, flag) <= 2**31 - 1:
                    self.error(f"--{flag.replace('_', '-')} is out of range")
        if getattr(ns, "nj_bootstrap", None) is not None:
            if not getattr(ns, "nj", None):
                self.error("--nj-bootstrap requires --nj FILE")
            if not 1 <= ns.nj_bootstrap <= 10000:
                self.error("--nj-bootstrap is out of range (1 .. 10000)")
        if getattr(ns, "nj_seed", None) is not None:
            if getattr(ns, "nj_bootstrap", None) is None:
                self.error("--nj-seed requires --nj-bootstrap N")
            if not 0 <= ns.nj_seed <= 2**64 - 1:
                self.error("--nj-seed is out of range")
        if getattr(ns, "nj_transfer", False) and getattr(ns, "nj_bootstrap", None) is None:
            self.error("--nj-transfer requires --nj-bootstrap N")
        for flag in NJ_TABLES:
            if getattr(ns, flag, None) and not getattr(ns, "nj", None):
                self.error(f"--{flag.replace('_', '-')} requires --nj FILE")
        if getattr(ns, "core_sites", False) and not (getattr(ns, "sites", None) or getattr(ns, "snp_alignment", None)):
            self.error("--core-sites requires --sites FILE or --snp-alignment FILE")
        if getattr(ns, "cluster_levels", None) is not None:
            if not getattr(ns, "clusters", None):
                self.error("--cluster-levels requires --clusters FILE")
            try:
                from kaptive_amd._native import check_cluster_levels

                v = ns.cluster_levels  # (the sub-command's parser has been here before its parent: then it is a tuple already)
                ns.cluster_levels = check_cluster_levels(v if isinstance(v, tuple) else [int(t) for t in str(v).split(",")])
            except ValueError:
                self.error("--cluster-levels takes at most 8 comma-separated numbers, none negative, strictly ascending")
        return ns, rest


def build_parser() -> argparse.ArgumentParser:
    ap = _Parser(prog="kaptive_amd", description="MI355X-native locus typing (Kaptive-compatible)")
    sub = ap.add_subparsers(dest="command", required=True)
    t = sub.add_parser("type", aliases=["assembly"], help="In silico serotyping of assemblies")
    t.add_argument("database", help="Database blob (.npz) or GenBank file with its .toml")
    t.add_argument("genomes", nargs="+", help="Genome assemblies in fasta format; can be compressed")
    t.add_argument("--db", action="append", metavar="DATABASE",
                   help="A further database to type every assembly against in the same pass (repeatable; same formats as the "
                        "positional); reports are then written per database")
    _add_outputs(t, ("-o", "--out"), include_json=True)
    c = t.add_argument_group("Confidence options")
    c.add_argument("--max-other-genes", type=int, default=1, metavar="", help="Typeable if <= other genes (default: 1)")
    c.add_argument("--min-completeness", type=float, default=0.5, metavar="", help="Typeable if >= completeness (default: 0.5)")
    c.add_argument("--below-threshold", action="store_true", help="Typeable if any genes in locus are below threshold")
    o = t.add_argument_group("Other options")
    o.add_argument("-t", "--threads", type=int, default=0, metavar="", help="Threads for reading/packing genomes (0 = the CPUs this process is granted)")
    o.add_argument("--partial-edge-tolerance", type=int, default=5, metavar="", help="Bases from contig edge to call a partial gene")
    o.add_argument("--devices", default="0", metavar="", help="Comma-separated GPU indices, or 'all' (default: 0)")
    o.add_argument("--batch-size", type=int, default=0, metavar="",
                   help="Assemblies per device submission (default: 64, 128, 256, then 512 -- first rows early, large batches later)")
    o.add_argument("-V", "--verbose", action="store_true")
    t.set_defaults(func=run_type)
    v = sub.add_parser("convert", help="Convert JSON-lines results to other formats")
    v.add_argument("jsonl", help="Serialised results in JSON-lines format (- for stdin)")
    _add_outputs(v, ("-t", "--tsv"), include_json=False)
    v.set_defaults(func=run_convert)
    return ap


PAIR_TABLES = ("distances", "clusters", "mst", "newick", "nj", "sites", "snp_alignment")  # the flags whose tables are made of the run's locus rows
NJ_TABLES = ("nj_changes", "nj_homoplasy")  # further tables of the same rows, each beside --nj only: they never ask for the rows on their own


def pipeline_options(args: argparse.Namespace, threads: "int | None" = None, read_ahead_share: int = 1) -> PipelineOptions:
    """What a pipeline of this command line reads (an option declared with ``default=SUPPRESS`` is absent from the namespace unless
    given).  ``threads``, ``read_ahead_share``: this pipeline's part of the host, where several device processes share it."""
    def on(name) -> bool:
        return bool(getattr(args, name, None))

    return PipelineOptions(
        threads=args.threads if threads is None else threads, read_ahead_share=read_ahead_share, tsv=bool(args.out), pha4ge=bool(args.pha4ge),
        json=bool(args.json), loci=args.loci or None, genes=args.genes or None, proteins=args.proteins or None, paf=on("paf"), cs=on("cs"), eqx=on("eqx"),
        reports=frozenset(r.name for r in REPORTS if on(r.name)), locus_rows=any(on(f) for f in PAIR_TABLES),
        max_other_genes=args.max_other_genes, min_completeness=args.min_completeness, below_threshold=args.below_threshold,
        partial_edge_tolerance=args.partial_edge_tolerance, rescue_flank=getattr(args, "rescue_flank", None), rescue_min_score=getattr(args, "rescue_min_score", None))  # fmt: skip


class _RunDistances:
    """``--distances``, ``--clusters``, ``--mst``, ``--newick``, ``--nj`` (with ``--nj-changes`` and ``--nj-homoplasy``), ``--sites`` and ``--snp-alignment``: the locus rows of the whole run, collected once for all of them,
    merged chunk by chunk in input order -- one ``LocusRows`` per database -- and, after the last chunk, compared on a device and
    written: one table each, or with ``--db`` one per database (``per_database_path``).  All tables of a locus come from one device
    handle."""

    def __init__(self, args: argparse.Namespace) -> None:
        self.core_sites = bool(getattr(args, "core_sites", False))
        self.levels = getattr(args, "cluster_levels", None)
        self.max_diff = getattr(args, "max_distance", None)
        self.min_compared = getattr(args, "min_compared", None)
        self.bootstrap = getattr(args, "nj_bootstrap", None) or 0
        self.seed = getattr(args, "nj_seed", None)
        self.transfer = bool(getattr(args, "nj_transfer", False))
        self.rows: "list | None" = None  # [(keyword or None, LocusRows)]
        self.args = args

    def _start(self, dbs) -> None:
        from kaptive_amd.distances import LocusRows

        several = bool(getattr(self.args, "db", None))
        self.rows = [(db.metadata.keyword if several else None, LocusRows(db)) for db in dbs]

    def take(self, outs, dbs=None) -> None:
        """Removes every database's payload from one chunk's outputs and merges it.  ``dbs``: the run's databases, where somebody has
        them loaded already (the single-device pipeline); otherwise they are read from the command line's paths on first use."""
        if self.rows is None:
            self._start(dbs if dbs is not None else [load_database(p) for p in (self.args.database, *(getattr(self.args, "db", None) or []))])
        for (_, rows), (_, out) in zip(self.rows, outs):
            rows.merge(out.pop(LOCUS_ROWS_KEY))

    @staticmethod
    def _lines(rows, made) -> bytes:
        """A table's lines; a method that may skip loci returns them beside its lines (``nj_tsv``): one line to stderr for each."""
        if isinstance(made, tuple):
            made, skipped = made
            for L in skipped:
                print(f"--nj: locus {rows.db.loci.ids[L]} has more than the most taxa a neighbour-joining tree may have; it gets no line", file=sys.stderr)
        return made

    def write(self, ctx) -> None:
        from kaptive_amd import _native

        md = _native.DIST_MAX_DIFF if self.max_diff is None else self.max_diff
        mc = _native.DIST_MIN_COMPARED if self.min_compared is None else self.min_compared
        levels = _native.CLUSTER_LEVELS if self.levels is None else self.levels
        # one row per table, in PAIR_TABLES' order: the option that asks for it, its header, the LocusRows method that makes its lines, that method's arguments
        kinds = (
            ("distances", _native.DISTANCES_HEADER, "tsv", (md, mc)),
            ("clusters", _native.clusters_header(levels), "clusters_tsv", (levels, mc)),
            ("mst", _native.DISTANCES_HEADER, "tree_tsv", (mc,)),
            ("newick", _native.newick_header(), "newick_tsv", (mc,)),
            ("nj", _native.nj_support_header() if self.bootstrap else _native.nj_header(), "nj_tsv", (mc, self.bootstrap, 1 if self.seed is None else self.seed, self.transfer)),
            ("nj_changes", _native.nj_changes_header(), "nj_changes_tsv", (mc,)),
            ("nj_homoplasy", _native.nj_homoplasy_header(), "nj_homoplasy_tsv", (mc,)),
            ("sites", _native.SITES_HEADER, "sites_tsv", (self.core_sites,)),
            ("snp_alignment", _native.SNP_ALIGNMENT_HEADER, "snp_alignment_tsv", (self.core_sites,)),
        )
        for kw, rows in self.rows or []:
            # (the loci --nj skips are skipped by its two companions as well: --nj's line to stderr says so once)
            tables = [(path, header + (self._lines(rows, made) if flag not in NJ_TABLES else made[0]))
                      for flag, header, method, a in kinds if (path := getattr(self.args, flag, None)) for made in (getattr(rows, method)(ctx, *a),)]  # fmt: skip
            rows.close()  # (the handles of this database's loci: every table has been made of them)
            for path, text in tables:
                if kw is None and _is_stdout(path):
                    sys.stdout.buffer.write(text)
                    sys.stdout.buffer.flush()
                else:
                    with open(path if kw is None else per_database_path(path, kw), "wb") as h:
                        h.write(text)


def _device_worker(options: PipelineOptions, databases: list, device: int, chunks: list, conn, devices=None, nodes=None) -> None:
    """One process per device (``--devices a,b,...``): types its chunks and sends ``(k, outputs)`` up the pipe; an
    exception travels the same way and ends the worker.  Before it reads a file the process moves to its device's share of
    the granted CPUs on the device's NUMA node (kaptive_amd/affinity.py): reader threads and page-locked shards follow."""
    import kaptive_amd
    from kaptive_amd import affinity

    kaptive_amd.tune_runtime()
    placed = affinity.place(device, devices, nodes)
    if os.environ.get("KAPTIVE_AMD_CLI_TIMING"):
        print(f"[kaptive_amd] device {device}: NUMA node {placed['numa_node']}, {len(placed['cpus'] or [])} CPUs, pinned={placed['applied']}", file=sys.stderr)
    pipe = None
    try:
        pipe = TypingPipeline(options, device, databases=databases, chunks=chunks)
        for k, out in pipe.run(chunks):
            conn.send((k, out))
        conn.send(None)
    except BaseException as e:  # noqa: BLE001 - handed to the parent, which re-raises it
        try:
            conn.send(e)
        except Exception:  # noqa: BLE001 - an exception that does not pickle travels as its text
            conn.send(RuntimeError(f"{type(e).__name__}: {e}"))
    finally:
        if pipe is not None:
            pipe.close(fast=True)  # (a worker process: it ends here)
        conn.close()


def _since_process_start() -> float:
    """Seconds since the kernel created this process (Linux: /proc; elsewhere 0): interpreter start-up and imports included."""
    try:
        with open("/proc/self/stat") as f:
            start_ticks = float(f.read().rsplit(")", 1)[1].split()[19])
        with open("/proc/uptime") as f:
            return float(f.read().split()[0]) - start_ticks / os.sysconf("SC_CLK_TCK")
    except (OSError, ValueError, IndexError):
        return 0.0


def _is_stdout(path) -> bool:
    return str(path) in ("-", "stdout")


def per_database_path(path, keyword: str) -> str:
    """Where a database's copy of a report goes when several databases are typed: its keyword before the last suffix
    (``results.tsv`` -> ``results.kpsc_k.tsv``), or appended to a name without one (``results`` -> ``results.kpsc_k``)."""
    head, name = os.path.split(os.fspath(path))
    root, ext = os.path.splitext(name)
    return os.path.join(head, f"{root}.{keyword}{ext}")


def interleave_lines(blocks) -> bytes:
    """Line j of every block in turn, for j = 0, 1, ...: the blocks hold one line per assembly of the same chunk (one
    block per database), and a report on stdout lists every database's line of a genome before the next genome's.  A byte
    gather in numpy: no object per line."""
    if len(blocks) == 1:
        return bytes(blocks[0])
    arrs = [np.frombuffer(b, np.uint8) for b in blocks]
    ends = [np.flatnonzero(a == 0x0A) + 1 for a in arrs]
    n = len(ends[0])
    if any(len(e) != n or (e[-1] if n else 0) != len(a) for a, e in zip(arrs, ends)):
        raise RuntimeError("every database's report block must hold one whole line per assembly of the chunk")
    if n == 0:
        return b""
    base = np.cumsum([0] + [len(a) for a in arrs[:-1]])
    starts = np.stack([np.concatenate([[0], e[:-1]]) + b for e, b in zip(ends, base)], axis=1).ravel()  # line j of block d at j * D + d
    lens = np.stack([np.diff(np.concatenate([[0], e])) for e in ends], axis=1).ravel()
    out_start = np.cumsum(lens) - lens
    gather = np.arange(int(lens.sum())) - np.repeat(out_start - starts, lens)
    return np.concatenate(arrs)[gather].tobytes()


def _batch_outputs() -> tuple:
    """One row per output a chunk's bytes go to, in the order they are opened: the key of the chunk's outputs, the option that names the
    file, and the header line."""
    from kaptive_amd.serotyping.io import KaptiveRow, Pha4geRow

    return (("tsv", "out", KaptiveRow.header()), ("pha4ge", "pha4ge", Pha4geRow.header()), ("json", "json", b""), ("paf", "paf", b""),
            *((r.name, r.name, r.header) for r in REPORTS))


class _PerDatabaseOutputs:
    """Where the bytes of a run's chunks go (``_batch_outputs``): a file per database and report, each with its own header line;
    a report on stdout gets one header and the databases' lines genome by genome (``interleave_lines``: of one database, its
    block as it is).  A run without ``--db`` has one database, whose keyword is ``None``: its files are named as given, and they
    are opened -- headers written -- here, before anything is typed.  With ``--db`` the files are named by keyword
    (``per_database_path``) and opened with the first chunk's outputs, which carry the keywords."""

    def __init__(self, args: argparse.Namespace) -> None:
        self.wanted = [(key, path, header) for key, attr, header in _batch_outputs() if (path := getattr(args, attr, None))]
        self.streams: "dict | None" = None  # key -> one file per database, or None for stdout
        self.files: list = []
        if not getattr(args, "db", None):
            self._open((None,))

    def _open(self, keywords) -> None:
        self.streams = {}
        for key, path, header in self.wanted:
            if _is_stdout(path):
                sys.stdout.buffer.write(header)
                self.streams[key] = None
                continue
            self.streams[key] = []
            for kw in keywords:
                h = open(path if kw is None else per_database_path(path, kw), "wb")
                self.files.append(h)
                h.write(header)
                self.streams[key].append(h)

    def write(self, outs) -> None:
        """``outs``: ``((keyword, {key: bytes}), ...)`` of one chunk, one entry per database in order."""
        if self.streams is None:
            self._open([kw for kw, _ in outs])
        for key in outs[0][1]:  # (in the order the chunk was rendered)
            if key in self.streams:
                blocks = [out[key] for _, out in outs]
                if self.streams[key] is None:
                    sys.stdout.buffer.write(interleave_lines(blocks))
                else:
                    for h, block in zip(self.streams[key], blocks):
                        h.write(block)

    def close(self) -> None:
        for h in self.files:
            h.close()
        if self.streams and None in self.streams.values():
            sys.stdout.buffer.flush()


def run_type(args: argparse.Namespace) -> int:
    entered = _since_process_start()
    if str(args.devices).strip().lower() == "all":
        from kaptive_amd import _native

        devices = list(range(max(1, _native.device_count())))
    else:
        devices = [int(d) for d in str(args.devices).split(",") if d != ""] or [0]
    # Chunks: of --batch-size when given; otherwise small ones first (the first rows are out after 0.6 s instead of 1.5 s:
    # page-locking and device buffers of a 512-assembly chunk take a second to set up) and 512 from the fourth chunk of a
    # device on, where the steady rate is highest.
    sizes = iter(()) if args.batch_size else iter([64] * len(devices) + [128] * len(devices) + [256] * len(devices))
    chunks, i = [], 0
    while i < len(args.genomes):
        n = next(sizes, args.batch_size or 512)
        chunks.append((len(chunks), args.genomes[i : i + n]))
        i += n
    t_check = time.perf_counter()
    seen: set = set()
    for p in args.genomes:  # the reference fails before it types anything (src/kaptive/cli.py:287-289)
        if p not in seen:  # (a path listed twice is looked at once; os.stat directly: Path objects cost more than the call)
            seen.add(p)
            try:
                import stat as _stat

                if not _stat.S_ISREG(os.stat(p).st_mode):
                    raise FileNotFoundError(f"{p} does not exist")
            except OSError:
                raise FileNotFoundError(f"{p} does not exist") from None
    t_check = time.perf_counter() - t_check
    for flag in (*(r.name for r in REPORTS), *PAIR_TABLES, *NJ_TABLES):
        if getattr(args, "db", None) and (v := getattr(args, flag, None)) and _is_stdout(v):
            raise ValueError(f"--{flag.replace('_', '-')} with --db writes a table per database: it needs a file name, not stdout")
    databases = [args.database, *(args.db or [])]
    dist = _RunDistances(args) if any(getattr(args, f, None) for f in PAIR_TABLES) else None
    run_dbs = None  # the databases of the run, where this process has loaded them (one device)
    outputs = _PerDatabaseOutputs(args)  # (without --db its files are open, headers written, from here on)
    done = 0
    timing_path = os.environ.get("KAPTIVE_AMD_CLI_TIMING")  # bench.py: when each chunk's rows were written
    t_start, chunk_times, phases = time.perf_counter(), [], {}

    def write(outs, n):
        nonlocal done
        if dist is not None:
            dist.take(outs, run_dbs)
        outputs.write(outs)
        done += n
        chunk_times.append((done, time.perf_counter() - t_start))
        if args.verbose:
            print(f"\r{done}/{len(args.genomes)}", end="", file=sys.stderr, flush=True)

    try:
        if len(devices) == 1:
            pipe = TypingPipeline(pipeline_options(args), devices[0], databases=databases, chunks=chunks)
            try:
                run_dbs = [t._db for t in pipe.typers]
                for k, out in pipe.run(chunks):
                    write(out, len(chunks[k][1]))
                if dist is not None:  # after the last chunk, on the pipeline's own context
                    if dist.rows is None:
                        dist._start(run_dbs)
                    dist.write(pipe.engine.ctx)
            finally:
                phases = {name: round(t - t_start, 3) for name, t in pipe.marks.items()}
                pipe.close(fast=FAST_EXIT)
                if FAST_EXIT:
                    _KEEP.append(pipe)  # (its buffers and its context leave with the process, not through their destructors)
        else:
            # chunk k goes to device k mod n; rows come back through pipes and are written in input order
            import multiprocessing as mp

            ctx = mp.get_context("spawn")
            conns, procs = [], []
            from kaptive_amd import usable_cpus

            # the device processes share the host: each gets its part of the reader-thread budget and of the read-ahead memory
            options = pipeline_options(args, max(1, (args.threads or usable_cpus()) // len(devices)), len(devices))
            from kaptive_amd import affinity

            nodes = affinity.device_numa_nodes(list(devices))  # asked once, in a process of its own (0.3 s beside the first reads)
            for i, d in enumerate(devices):
                parent, child = ctx.Pipe(duplex=False)
                proc = ctx.Process(target=_device_worker, args=(options, databases, d, chunks[i :: len(devices)], child, list(devices), nodes), daemon=True)
                proc.start()
                child.close()
                conns.append(parent)
                procs.append(proc)
            ok = False
            try:
                for k in range(len(chunks)):
                    dev = devices[k % len(devices)]
                    try:
                        msg = conns[k % len(devices)].recv()
                    except (EOFError, OSError) as e:  # the worker died without a word (killed, crashed in native code)
                        raise RuntimeError(f"the worker of device {dev} ended unexpectedly (exit code {procs[k % len(devices)].exitcode})") from e
                    if isinstance(msg, BaseException):
                        raise msg
                    if msg is None or msg[0] != k:
                        raise RuntimeError(f"device worker {dev} ended early or out of order")
                    write(msg[1], len(chunks[k][1]))
                ok = True
            finally:
                if not ok:  # the others are blocked on full pipes: nothing to wait for
                    for proc in procs:
                        if proc.is_alive():
                            proc.terminate()
                for c in conns:
                    c.close()
                for proc in procs:
                    proc.join(timeout=30 if ok else 5)
                    if proc.is_alive():
                        proc.terminate()
            if dist is not None:
                # the workers have ended and this process has not touched a device yet: a context on the first listed one, for this step
                from kaptive_amd import _native

                if dist.rows is None:
                    dist.take(())
                dctx = _native.Context(devices[0])
                try:
                    dist.write(dctx)
                finally:
                    dctx.close()
    finally:
        outputs.close()
    if FAST_EXIT:
        # every stream this command writes is closed or flushed: what is left (reader threads, page-locked shards, the device
        # context) may leave with the process.  Other subcommands, and a run that raised, end through the interpreter.
        global FAST_EXIT_ARMED
        FAST_EXIT_ARMED = True
    if args.verbose:
        print(file=sys.stderr)
    if timing_path:
        # process_s: seconds since the process was created at three points -- run_type entered (interpreter start, imports,
        # argument parsing), typing started (t_start: the origin of rows_written_at / phases_s / seconds), and now
        Path(timing_path).write_text(json.dumps({"assemblies": len(args.genomes), "seconds": time.perf_counter() - t_start,
                                                 "batch_size": args.batch_size, "devices": devices,
                                                 "rows_written_at": chunk_times, "phases_s": phases,
                                                 "process_s": {"run_type_entered": round(entered, 3), "file_check": round(t_check, 3),
                                                               "end_of_run_type": round(_since_process_start(), 3)}}) + "\n")  # fmt: skip
    return 0


def run_convert(args: argparse.Namespace) -> int:
    from kaptive_amd.serotyping.models import SerotypingResult

    exporter = ResultExporter(args)
    handle = sys.stdin.buffer if args.jsonl in ("-", "stdin") else open(args.jsonl, "rb")
    try:
        for line in handle:
            line = line.strip()
            if line:
                exporter(SerotypingResult.from_dict(json.loads(line)))
    finally:
        exporter.close()
        if handle is not sys.stdin.buffer:
            handle.close()
    return 0


def main(argv=None) -> int:
    import kaptive_amd

    kaptive_amd.tune_runtime()  # before the first HIP call of the process
    from kaptive_amd.db.models import DatabaseError

    args = build_parser().parse_args(argv)
    try:
        return args.func(args)
    except (DatabaseError, FileNotFoundError, PermissionError, NotImplementedError, ValueError) as e:  # (ValueError: an unreadable FASTA / compressed stream)
        print(f"error: {e}", file=sys.stderr)
        return 1
    except KeyboardInterrupt:
        return 1
    except BrokenPipeError:
        return 130


if __name__ == "__main__":
    sys.exit(main())
