"""Small parsimony on the neighbour-joining tree without a GPU (include/kp_spec.h, PARSIMONY): kaptive_amd/csrc/kp_pars.h under g++
against the set restatement of tests/parsimony_util.py and against the exhaustive minimum; the spec's known answers; the section's
properties on ``D.population`` matrices; planted trees; the check of a record list; the two formatters (kp_format_nj_homoplasy,
kp_format_nj_changes) byte for byte against Python restatements, sized and filled exactly, with their refusals; the binding; and the
command line's refusals."""

from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from kaptive_amd import _native
from tests import distances_util as D
from tests import nj_transfer_util as TR
from tests import nj_util as NJ
from tests import parsimony_util as P

ROOT = Path(__file__).resolve().parent.parent


def _same(got, want, what):
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (what, got.tolist(), want.tolist())


# ---- the spec and the binding ------------------------------------------------------------------------------------------------------------
def test_spec_and_binding():
    spec = (ROOT / "include" / "kp_spec.h").read_text()
    assert "---- PARSIMONY (" in spec and spec.index("---- TRANSFER (") < spec.index("---- PARSIMONY (")
    section = spec[spec.index("---- PARSIMONY (") :]
    for word in ("NOT A ROOT", "UP-PASS", "DOWN-PASS", "PROPERTIES", "KNOWN ANSWERS", "OUT OF SCOPE", "ACCTRAN"):
        assert word in section, word
    for col in P.KNOWN:
        assert f'"{col}"' in section, col
    lib = _native.lib()
    for name in ("kp_dist_nj_parsimony", "kp_dist_pars_sites", "kp_dist_pars_changes", "kp_format_nj_homoplasy", "kp_format_nj_changes"):
        assert name in _native.EXPORTS and hasattr(lib, name), name
    assert hasattr(_native.Distances, "nj_parsimony") and callable(_native.format_nj_homoplasy) and callable(_native.format_nj_changes)
    assert _native.PARS_SITE_DTYPE == P.SITE_DTYPE and _native.PARS_CHANGE_DTYPE == P.CHANGE_DTYPE and P.SITE_DTYPE.itemsize == 16 == P.CHANGE_DTYPE.itemsize
    assert _native.nj_homoplasy_header() == P.HOMOPLASY_HEADER and _native.nj_changes_header() == P.CHANGES_HEADER
    h = P.harness()
    assert h.kpy_pars_step_planes() == 14 and 2**14 >= NJ.MAX_TAXA == _native.NJ_MAX_TAXA
    assert [h.kpy_pars_node_planes(v, 5) for v in (0, 1, 4, 5, 6, 8)] == [0, 3, 12, 15, 19, 27]
    assert "kp_dist_pars.hip" in (ROOT / "kaptive_amd" / "build.py").read_text()


# ---- the known answers ---------------------------------------------------------------------------------------------------------------------
def test_the_known_answers_of_the_spec():
    nodes = TR.records(P.KNOWN_TREE)
    cols = list(P.KNOWN)
    for text, (steps, alleles, changes) in P.KNOWN.items():
        got = P.column(5, nodes, D.codes_of(text))
        assert (got[0], got[1]) == (steps, alleles) and got[3] == [(v, p, "acgt".index(f), "acgt".index(t)) for v, p, f, t in changes], text
        assert P.exhaustive(5, nodes, D.codes_of(text)) == steps
    assert P.column(5, nodes, D.codes_of("ccctg"))[2][7] == 1  # the tie at the top: the smallest code, c
    assert P.column(5, nodes, D.codes_of("ccnaa"))[2][2] == 1  # the missing leaf takes its parent's state
    codes = np.full((5, 16), D.GAP, np.uint8)
    codes[:, : len(cols)] = np.array([D.codes_of(c) for c in cols]).T
    want = P.parsimony(codes, np.arange(5), nodes)
    assert want[0]["column"].tolist() == [1, 2, 3, 4] and want[0]["steps"].tolist() == [1, 2, 2, 1] and want[0]["alleles"].tolist() == [3, 5, 14, 3]
    assert [(int(c["node"]), int(c["column"])) for c in want[1]] == [(1, 2), (3, 3), (4, 3), (5, 1), (6, 2), (6, 4)]
    got = P.harness_parsimony(codes, np.arange(5), nodes)
    _same(got[0], want[0], "sites"), _same(got[1], want[1], "changes")


# ---- kp_pars.h against sets and against the exhaustive minimum ---------------------------------------------------------------------------------
def _random_codes(rng, n, W):
    """Few bases a column, missing data, one column nobody holds a base in."""
    pool = rng.integers(0, 4, (W, 2))
    codes = pool[np.arange(W)[None, :], rng.integers(0, 2, (n, W))].astype(np.uint8)
    wild = rng.random((n, W))
    codes[wild < 0.15] = rng.integers(0, 4, int((wild < 0.15).sum()))
    codes[(wild > 0.8) & (wild < 0.9)] = D.N
    codes[wild >= 0.9] = D.GAP
    codes[:, W - 1] = D.N
    return codes


@pytest.mark.parametrize("n", (2, 3, 4, 5, 6, 7))
def test_against_the_exhaustive_minimum(n):
    rng = np.random.default_rng([n, 3])
    for k in range(12):
        nodes = P.tree_of(n, rng if k % 3 else None, "caterpillar" if k % 3 == 2 and n > 3 else "grown")
        assert P.harness_tree_ok(n, nodes)
        codes = _random_codes(rng, n, 32)
        want = P.parsimony(codes, np.arange(n), nodes)
        steps = np.zeros(32, np.int64)
        steps[want[0]["column"]] = want[0]["steps"]
        for j in range(32):
            held = len({int(c) for c in codes[:, j] if c < 4})
            assert P.exhaustive(n, nodes, codes[:, j]) == steps[j] >= max(held - 1, 0) and (steps[j] == 0) == (held <= 1), (n, k, j)
        assert np.bincount(want[1]["column"], minlength=32).tolist() == steps.tolist()  # the changes number the steps
        got = P.harness_parsimony(codes, np.arange(n), nodes)
        _same(got[0], want[0], ("sites", n, k)), _same(got[1], want[1], ("changes", n, k))
        if n >= 4:  # steps do not depend on which record is last: another tree of the same splits
            other = P.tree_of(n, np.random.default_rng(k))
            if NJ.splits(n, other) == NJ.splits(n, nodes):
                assert P.parsimony(codes, np.arange(n), other)[0].tobytes() == want[0].tobytes()


@pytest.mark.parametrize("R,nb", ((16, 1), (40, 5), (70, 9)))
def test_properties_on_populations(R, nb):
    codes = D.population(np.random.default_rng([R, nb, 7]), R, nb)
    taxa, nodes, sites, changes = P.of_codes(codes, 1)
    n = len(taxa)
    assert 4 <= n < R and len(sites) > 0  # the all-GAP and the all-N row are no taxa
    got = P.harness_parsimony(codes, taxa, nodes)
    _same(got[0], sites, "sites"), _same(got[1], changes, "changes")
    c = codes[taxa]
    steps = np.zeros(codes.shape[1], np.int64)
    steps[sites["column"]] = sites["steps"]
    held = np.array([len({int(x) for x in c[:, j] if x < 4}) for j in range(c.shape[1])])
    assert (steps >= np.maximum(held - 1, 0)).all() and ((steps == 0) == (held <= 1)).all()
    assert np.bincount(changes["column"], minlength=len(steps)).tolist() == steps.tolist()
    assert [bin(int(a)).count("1") for a in sites["alleles"]] == held[sites["column"]].tolist()
    assert (np.diff(sites["column"]) > 0).all() and (changes["from"] != changes["to"]).all()
    key = changes["node"].astype(np.int64) * (1 << 32) + changes["column"]
    assert (np.diff(key) > 0).all() and changes["node"].max() < 2 * n - 3
    up = P.parents(n, nodes)
    assert all(up[int(v)] == int(p) for v, p in zip(changes["node"], changes["parent"]))
    for j in sites["column"][:20]:  # a leaf's state is its base wherever it holds one
        state = P.column(n, nodes, c[:, j])[2]
        assert all(state[k] == c[k, j] for k in range(n) if c[k, j] < 4)
    for shape in ("caterpillar", "grown"):  # hand-made trees of the same taxa
        other = P.tree_of(n, None, shape)
        want = P.parsimony(codes, taxa, other)
        got = P.harness_parsimony(codes, taxa, other)
        _same(got[0], want[0], shape), _same(got[1], want[1], shape)


@pytest.mark.parametrize("n", (6, 19))
def test_planted_trees(n):
    rng = np.random.default_rng([n, 5])
    codes, planted, at, (a, b) = P.planted_homoplasy(rng, n)
    taxa, nodes, sites, changes = P.of_codes(codes, 1)
    assert len(taxa) == n and NJ.splits(n, nodes) == planted
    under = P.below(n, nodes)
    everyone = frozenset(range(n))
    by_col = {int(s["column"]): s for s in sites}
    assert by_col[at]["steps"] == 2 and bin(int(by_col[at]["alleles"])).count("1") == 2  # excess 1
    assert sorted(int(c["node"]) for c in changes if c["column"] == at) == [a, b]
    some = 0
    for j in range(at):
        if len(set(codes[:, j].tolist())) < 2:
            continue
        s = by_col[j]
        assert s["steps"] == 1 and bin(int(s["alleles"])).count("1") == 2, j
        (c,) = [c for c in changes if c["column"] == j]
        assert frozenset([under[int(c["node"])], everyone - under[int(c["node"])]]) == P.bipartition(codes[:, j]), j
        some += 1
    assert some >= 3 * (2 * n - 3) and len(sites) == some + 1
    got = P.harness_parsimony(codes, taxa, nodes)
    _same(got[0], sites, "sites"), _same(got[1], changes, "changes")


def test_record_lists_that_are_no_tree():
    good = TR.records(P.KNOWN_TREE)
    assert P.harness_tree_ok(5, good) and not P.harness_tree_ok(4, good) and not P.harness_tree_ok(6, good) and not P.harness_tree_ok(5, good[:2])
    for bad in (((0, 1, -1), (5, 1, -1), (6, 4, 3)), ((0, 6, -1), (5, 2, -1), (1, 4, 3)), ((0, 1, 2), (5, 3, -1), (6, 4, -1)), ((0, 1, -1), (5, 2, -1), (6, 4, -1)),
                ((0, 1, -1), (5, 2, -1), (6, 4, 7)), ((-1, 1, -1), (5, 2, -1), (6, 4, 3)), ((0, 1, -2), (5, 2, -1), (6, 4, 3))):  # fmt: skip
        assert not P.harness_tree_ok(5, TR.records(bad)), bad
    assert P.harness_tree_ok(2, TR.records([(0, 1, -1)])) and P.harness_tree_ok(3, TR.records([(0, 1, 2)])) and not P.harness_tree_ok(2, TR.records([(0, 1, 2)]))
    assert P.harness_tree_ok(0, TR.records([])) and P.harness_tree_ok(1, TR.records([])) and not P.harness_tree_ok(2, TR.records([]))
    assert P.harness_tree_ok(65, P.tree_of(65, None, "caterpillar")) and P.harness_tree_ok(65, P.tree_of(65, np.random.default_rng(1)))


# ---- the formatters -----------------------------------------------------------------------------------------------------------------------------
GENES, LENGTHS = ["wzi", "wca J", "gnd"], [20, 5, 33]  # blocks 2, 1, 3: matrix columns 0, 32, 48


def _table():
    """A population of 24 rows over the three genes, padding GAP, with names that need quoting."""
    rng = np.random.default_rng(24)
    codes = D.population(rng, 24, 6)
    for first, L in ((0, 20), (32, 5), (48, 33)):
        codes[:, first + L : -(-(first + L) // 16) * 16] = D.GAP
    codes[:, 85:] = D.GAP
    names = [f"asm {k}" if k % 3 == 0 else f"it's_{k}" if k % 3 == 1 else f"asm_{k}" for k in range(24)]
    return (codes, names, *P.of_codes(codes, 1))


def test_formatters_against_the_restatement():
    codes, names, taxa, nodes, sites, changes = _table()
    assert len(sites) >= 10 and len(changes) >= len(sites) and (changes["node"] >= len(taxa)).any() and (changes["node"] < len(taxa)).any()
    got = _native.format_nj_homoplasy("KL1", GENES, LENGTHS, sites)
    assert got == P.homoplasy_lines("KL1", GENES, LENGTHS, sites) and got.count(b"\n") == len(sites)
    assert any(int(line.split(b"\t")[6]) > 0 for line in got.splitlines())  # a homoplasic column among them
    got = _native.format_nj_changes("KL1", names, taxa, nodes, GENES, LENGTHS, changes)
    assert got == P.changes_lines("KL1", names, taxa, nodes, GENES, LENGTHS, changes) and got.count(b"\n") == len(changes)
    assert b"\t'asm " in got and b"'it''s_" in got and b"\t#" in got and b"\t.\t1\t" in got
    rows = np.arange(24, dtype=np.int32)[::-1].copy()  # a mapping of rows and of genes
    assert _native.format_nj_changes("KL1", names[::-1], taxa, nodes, GENES, LENGTHS, changes, rows=rows) == got
    order = np.array([2, 0, 1], np.int32)
    assert _native.format_nj_homoplasy("KL1", [GENES[1], GENES[2], GENES[0]], LENGTHS, sites, genes=order) == P.homoplasy_lines("KL1", GENES, LENGTHS, sites)
    assert _native.format_nj_homoplasy("", GENES, LENGTHS, sites[:1]).startswith(b"\t")
    # empty lists
    assert _native.format_nj_homoplasy("KL1", GENES, LENGTHS, sites[:0]) == b"" == _native.format_nj_changes("KL1", names, taxa, nodes, GENES, LENGTHS, changes[:0])
    assert _native.format_nj_changes("KL1", ["x"], [0], np.zeros(0, NJ.NODE_DTYPE), GENES, LENGTHS, changes[:0]) == b""
    # the known answers as a table
    five = TR.records(P.KNOWN_TREE)
    kc = np.full((5, 16), D.GAP, np.uint8)
    kc[:, :5] = np.array([D.codes_of(c) for c in P.KNOWN]).T
    s, ch = P.parsimony(kc, np.arange(5), five)
    assert _native.format_nj_homoplasy("K", ["g"], [5], s) == b"K\tg\t2\t2\t2\t1\t0\nK\tg\t3\t3\t2\t2\t1\nK\tg\t4\t4\t3\t2\t0\nK\tg\t5\t5\t2\t1\t0\n"
    assert _native.format_nj_changes("K", list("vwxyz"), np.arange(5), five, ["g"], [5], ch) == (
        b"K\tw\tw\t.\t1\tg\t3\t3\tg\ta\nK\ty\ty\t.\t1\tg\t4\t4\tc\tt\nK\tz\tz\t.\t1\tg\t4\t4\tc\tg\nK\t#1\tv\tw\t2\tg\t2\t2\ta\tc\nK\t#2\tv\tx\t3\tg\t3\t3\ta\tg\nK\t#2\tv\tx\t3\tg\t5\t5\ta\tc\n")


def test_formatters_sized_then_filled_exactly():
    codes, names, taxa, nodes, sites, changes = _table()
    lib = _native.lib()
    lib.kp_format_nj_homoplasy.restype = lib.kp_format_nj_changes.restype = C.c_int64
    nb, no = _native._blob64(names)
    gb, go = _native._blob64(GENES)
    lens = np.array(LENGTHS, np.int32)
    p = P._p
    homoplasy = lambda out=None, cap=0, s=p(sites), n=len(sites), g=p(gb): lib.kp_format_nj_homoplasy(b"x", 1, g, p(go), 3, None, p(lens), s, C.c_int64(n), out, C.c_int64(cap))  # noqa: E731
    changed = lambda out=None, cap=0, c=p(changes), n=len(changes), nd=p(nodes), tx=p(taxa): lib.kp_format_nj_changes(  # noqa: E731
        b"x", 1, p(nb), p(no), 24, None, tx, len(taxa), nd, C.c_int64(len(nodes)), p(gb), p(go), 3, None, p(lens), c, C.c_int64(n), out, C.c_int64(cap))
    for call, want in ((homoplasy, _native.format_nj_homoplasy("x", GENES, LENGTHS, sites)), (changed, _native.format_nj_changes("x", names, taxa, nodes, GENES, LENGTHS, changes))):
        need = call()
        assert need == len(want) > 0
        buf = np.full(need + 8, 0x3F, np.uint8)
        assert call(out=p(buf), cap=need) == need and buf[:need].tobytes() == want and (buf[need:] == 0x3F).all()
        short = np.full(need, 0x3F, np.uint8)
        assert call(out=p(short), cap=need - 1) == need and short[need - 1] == 0x3F  # a short cap: the room it needs, nothing written past
        assert call(cap=5) == -1 and call(out=p(buf), cap=-1) == -1  # room without a buffer, negative room
    assert homoplasy(s=None) == -1 and homoplasy(n=-1) == -1 and homoplasy(g=None) == -1
    assert changed(c=None) == -1 and changed(n=-1) == -1 and changed(nd=None) == -1 and changed(tx=None) == -1


def test_formatter_refusals():
    codes, names, taxa, nodes, sites, changes = _table()
    n = len(taxa)

    def site(**kw):
        s = sites[:2].copy()
        for k, v in kw.items():
            s[k][1] = v
        return s

    for bad in (site(column=20), site(column=37), site(column=96), site(column=-1), site(column=int(sites["column"][0])), site(alleles=1), site(alleles=0), site(alleles=19),
                site(alleles=7, steps=1), site(steps=0)):  # fmt: skip
        with pytest.raises(ValueError):
            _native.format_nj_homoplasy("x", GENES, LENGTHS, bad)
    with pytest.raises(ValueError):
        _native.format_nj_homoplasy("x", GENES, LENGTHS[:2], sites)  # a length for every gene
    with pytest.raises(ValueError):
        _native.format_nj_homoplasy("x", GENES, [20, -5, 33], sites)

    def change(**kw):
        c = changes[:2].copy()
        for k, v in kw.items():
            c[k][1] = v
        return c

    top = 2 * n - 3
    for bad in (change(node=top, parent=-1), change(node=-1), change(node=top + 1), change(parent=int(changes["parent"][1]) + 1), change(to=int(changes["from"][1])), change(to=4),
                change(**{"from": 4}), change(column=20), change(column=96), changes[:2][::-1]):  # fmt: skip
        with pytest.raises(ValueError):
            _native.format_nj_changes("x", names, taxa, nodes, GENES, LENGTHS, bad)
    twice = nodes.copy()
    twice["b"][1] = twice["a"][1]
    for bad_taxa, bad_nodes in ((taxa[:-1], nodes), (taxa[::-1], nodes), (taxa, nodes[:-1]), (taxa, twice)):
        with pytest.raises(ValueError):
            _native.format_nj_changes("x", names, bad_taxa, bad_nodes, GENES, LENGTHS, changes[:0])
    with pytest.raises(ValueError):
        _native.format_nj_changes("x", names[:5], taxa, nodes, GENES, LENGTHS, changes)  # a taxon beyond the names
    assert _native.format_nj_changes("x", names, taxa, nodes, GENES, LENGTHS, changes[:2])


# ---- the command line ------------------------------------------------------------------------------------------------------------------------
def test_command_line_flags(capsys):
    from kaptive_amd.cli import NJ_TABLES, PAIR_TABLES, build_parser

    ap = build_parser()
    base = ["assembly", "db.npz", "a.fasta"]
    ns = ap.parse_args([*base, "--nj", "t.tsv"])
    assert not hasattr(ns, "nj_changes") and not hasattr(ns, "nj_homoplasy")  # the tree alone says nothing of them
    ns = ap.parse_args([*base, "--nj", "t.tsv", "--nj-changes", "c.tsv", "--nj-homoplasy", "h.tsv"])
    assert ns.nj_changes == "c.tsv" and ns.nj_homoplasy == "h.tsv"
    ns = ap.parse_args([*base, "--nj", "t.tsv", "--nj-homoplasy", "h.tsv", "--nj-bootstrap", "7", "--nj-transfer"])  # independent of the bootstrap
    assert ns.nj_homoplasy == "h.tsv" and not hasattr(ns, "nj_changes") and ns.nj_transfer is True
    for bad, why in ((["--nj-changes", "c.tsv"], "--nj-changes requires --nj FILE"), (["--nj-homoplasy", "h.tsv"], "--nj-homoplasy requires --nj FILE"),
                     (["--sites", "s.tsv", "--nj-changes", "c.tsv"], "--nj-changes requires --nj FILE")):  # fmt: skip
        with pytest.raises(SystemExit):
            ap.parse_args([*base, *bad])
        assert why in capsys.readouterr().err, bad
    assert NJ_TABLES == ("nj_changes", "nj_homoplasy") and not set(NJ_TABLES) & set(PAIR_TABLES)
