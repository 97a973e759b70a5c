"""The typing reduction's rules and round edges, case by case (tests/reduction_rules_util.py), without a GPU: every case is what
its label says, by its own numbers; every boundary moves the REFERENCE's recorded answer (tests/golden/typing_rules_<key>.npz,
oracle/make_golden.py::gen_typing_rules); the builder still builds what was recorded; and the core header
(kaptive_amd/csrc/kp_reduce_core.h through the g++ harness, the oracle's protein DP in between) gives the reference's record on
every case.  tests/test_gpu_reduction_rules.py repeats the last with the kernels of kp_reduce.hip."""

import numpy as np
import pytest

from kaptive_amd.serotyping import batch as B
from kaptive_amd.serotyping.core import Serotyper
from tests import reduction_rules_util as U
from tests.golden_util import load_db

KEYS = ("k", "o")
STOPS = (b"TAA", b"TAG", b"TGA")


def _typer(db, kwargs):
    t = Serotyper(db, aligner=lambda g: None, **kwargs)
    assert kwargs or (t.partial_edge_tolerance, t.min_gene_coverage) == (U.EDGE_TOL, U.MIN_COV)  # (read from its signature)
    return t


def _ids():
    return [(key, c.name) for key in KEYS for c in U.cases(key)]


@pytest.mark.parametrize("key", KEYS)
def test_builder_still_builds_the_recorded_cases(key):
    genome, recorded = U.load_rules(key)
    R, built = U.rules_assembly(key), U.cases(key)
    assert genome.contigs.ids == R.genome.contigs.ids
    assert np.array_equal(genome.contigs.lengths, R.genome.contigs.lengths)
    assert np.asarray(genome.contigs.seqs).tobytes() == np.asarray(R.genome.contigs.seqs).tobytes()
    assert [(r[0], r[1]) for r in recorded] == [(c.group, c.name) for c in built]
    for r, c in zip(recorded, built):
        assert r[2].dtype == U.HIT_DTYPE and r[2].tobytes() == c.hits.tobytes(), c.name
        assert r[5] == c.kwargs, c.name
        assert np.all(np.diff(c.hits["gene"]) >= 0), c.name  # Batch.set_hits: gene ascending
        clen = R.genome.contigs.lengths[c.hits["contig"]]
        assert np.all((c.hits["t_start"] >= 0) & (c.hits["t_end"] <= clen) & (c.hits["t_end"] >= c.hits["t_start"])), c.name
        glen = load_db(key).genes.lengths[c.hits["gene"]]
        assert np.all((c.hits["q_start"] >= 0) & (c.hits["q_end"] <= glen)), c.name
    assert {c.group for c in built} == set(U.GROUPS)


def test_constants_come_from_the_sources():
    assert U.C["SIZEOF_KEPT"] == B.KEPT_DTYPE.itemsize
    assert U.KEPT_IN_LDS * U.C["SIZEOF_KEPT"] <= 3 * U.C["KEPT_LDS"] * 4 < (U.KEPT_IN_LDS + 1) * U.C["SIZEOF_KEPT"]
    assert U.CODON_ROUND == U.LANES * U.TR and U.C["SORT_LDS"] * 8 == 4 * U.C["KEPT_LDS"] * 4


@pytest.mark.parametrize("key", KEYS)
def test_every_boundary_moves_the_references_answer(key):
    """Both sides of every two-sided pair are there, and the reference's record differs across it."""
    _, recorded = U.load_rules(key)
    by_name = {r[1]: r for r in recorded}
    pairs: dict[str, dict[int, str]] = {}
    for c in U.cases(key):
        if c.pair:
            assert c.pair[1] not in pairs.setdefault(c.pair[0], {}), c.name
            pairs[c.pair[0]][c.pair[1]] = c.name
    assert len(pairs) >= 20
    for what, sides in pairs.items():
        assert set(sides) == {0, 1}, what
        a, b = by_name[sides[0]], by_name[sides[1]]
        same = a[4] == b[4] and all(np.asarray(a[3][f]).tobytes() == np.asarray(b[3][f]).tobytes() for f in a[3] if f != "typer_kwargs_json")
        assert not same, f"{what}: the reference answers {sides[0]} and {sides[1]} alike"


def _priority(db, hits, best):
    return db.gene_locus_indices[hits["gene"]] == best


def _first_stop(text, strand, frame=0):
    from kaptive_amd.synth import revcomp

    s = bytes(text if strand > 0 else revcomp(np.asarray(text)))[frame:]
    return next((i for i in range(len(s) // 3) if s[3 * i : 3 * i + 3] in STOPS), None)


def _text(R, h):
    c = R.genome.contigs
    o = int(c.offsets[h["contig"]])
    return np.asarray(c.seqs[o + int(h["t_start"]) : o + int(h["t_end"])])


def _max_codons(h):
    frame, n = (3 - h["q_start"] % 3) % 3, h["t_end"] - h["t_start"]
    return np.where(n > frame, (n - frame) // 3, 0)


@pytest.mark.parametrize("key", KEYS)
def test_every_case_is_what_its_label_says(key):
    db, R = load_db(key), U.rules_assembly(key)
    _, recorded = U.load_rules(key)
    exp_of = {r[1]: (r[3], r[4]) for r in recorded}
    L, tol = db.genes.lengths, int(db.max_locus_length)
    seen = set()
    frames = set()
    for c in U.cases(key):
        h, info = c.hits, c.info
        kind = info.get("kind")
        seen.add(kind)
        exp, scalars = exp_of[c.name]
        order = U.visit_order(h, _priority(db, h, scalars["best_locus_idx"]))
        pos = np.empty(len(h), np.int64)
        pos[order] = np.arange(len(h))  # visit position of every row
        if kind == "cov":
            x = h[h["gene"] == info["gene"]][0]
            n, lg = int(x["q_end"] - x["q_start"]), int(L[info["gene"]])
            assert (5 * n == lg) == (n / lg == U.MIN_COV) == info["at_floor"] and 5 * (n + 1 - info["at_floor"]) == lg, c.name
        elif kind in ("tie", "zero"):
            from tests import harness_util as H

            t = _typer(db, {})
            sc, cn = H.locus_scores(h, H.HarnessDb(db), U.MIN_COV)
            best, final, _ = B.choose_best_loci(sc[None, :], cn[None, :], t._expected_genes_per_locus)
            top = np.flatnonzero(final[0] == final[0].max())
            assert len(top) >= 2 and int(best[0]) == top[0] == scalars["best_locus_idx"], c.name
            assert (final[0].max() == 0) == (kind == "zero"), c.name
        elif kind == "overlap":
            x, y = h[h["gene"] == info["x"]][0], h[h["gene"] == info["y"]][0]
            ov = min(x["t_end"], y["t_end"]) - max(x["t_start"], y["t_start"])
            mn = min(x["t_end"] - x["t_start"], y["t_end"] - y["t_start"])
            assert (ov, mn) == (info["ov"], info["mn"]) and pos[h["gene"] == info["x"]][0] < pos[h["gene"] == info["y"]][0], c.name
            if c.pair[1] == 0:
                assert 10 * ov <= mn < 10 * (ov + 1) and (10 * ov == mn) == info["exact"], c.name
            else:
                assert 10 * (ov - 1) <= mn < 10 * ov, c.name
            assert U.cull_model(h, order)[h["gene"] == info["y"]][0] == (c.pair[1] == 0), c.name
        elif kind == "empty":
            assert len(h) == info["n"] and int((h["t_end"] == h["t_start"]).sum()) == 1, c.name
            assert int(U.cull_model(h, order).sum()) == (1 if len(h) == 1 else len(h) - 1), c.name
        elif kind == "tie_order":
            rows = np.flatnonzero(pos >= 2)
            assert len(rows) == 2, c.name
            first = rows[np.argmin(pos[rows])]
            assert h["gene"][first] == info["first"], c.name
            flags = U.cull_model(h, order)
            assert flags[first] and not flags[rows[rows != first][0]], c.name
        elif kind == "round":
            n, moved = info["n"], info["moved"]
            assert len(h) == n and np.all(h["score"][order][2:] == 4000 - np.arange(2, n)), c.name
            kept_at = U.cull_model(h, order)[order]  # by visit position
            free = [p for p in range(n) if p not in moved]
            assert kept_at[free].all(), c.name
            shape = info["shape"]
            if shape.startswith("chain"):
                a = moved[0] - 1
                want = {"chain_head": 2, "chain_tail": U.LANES - 3, "chain_across": U.LANES - 1, "chain_b_last": U.LANES - 2}[shape]
                assert a == want and kept_at[a] and not kept_at[a + 1] and (a + 2 >= n or kept_at[a + 2]), c.name
                assert shape != "chain_across" or (a % U.LANES == U.LANES - 1 and (a + 1) % U.LANES == 0), c.name
            elif shape == "all_survive":
                assert kept_at.all(), c.name
            elif shape == "round1_none":
                assert not kept_at[U.LANES : 2 * U.LANES].any() and kept_at[: U.LANES].all(), c.name
            elif shape == "round1_lane63":
                assert np.flatnonzero(kept_at[U.LANES : 2 * U.LANES]).tolist() == [U.LANES - 1], c.name
        elif kind == "resident":
            assert int(U.cull_model(h, order).sum()) == info["nk"] == len(h) and info["nk"] in (U.KEPT_IN_LDS, U.KEPT_IN_LDS + 1), c.name
        elif kind == "linkage":
            by_start = h[np.argsort(h["t_start"])]
            assert int(by_start["t_start"][1] - by_start["t_end"][0]) == info["gap"] and info["gap"] - tol == c.pair[1], c.name
        elif kind == "vote":
            m = U.piece_model(db, h, scalars["best_locus_idx"], tol)
            assert len(h) == 3 and len(m["pieces"]) == 1 and m["pieces"][0][5] == info["vote"] and int(m["primary"].sum()) >= 2, c.name
            assert np.array_equal(exp["locus_pieces.strands"], [m["pieces"][0][3]]), c.name
        elif kind == "frame":
            x = h[h["gene"] == R.S][0]
            n, frame = int(x["t_end"] - x["t_start"]), (3 - int(x["q_start"]) % 3) % 3
            assert (int(x["q_start"]) % 3, (n - frame) % 3) == (info["q_mod"], info["rem"]), c.name
            frames.add((info["q_mod"], info["rem"], int(x["strand"])))
        elif kind == "text":
            x = h[-1] if R.S != R.g0 else h[0]
            text, label = _text(R, x), info["label"]
            stop = _first_stop(text, 1)
            want = {"stop0": 0, "stop1": 1, "two_stops": 50, "no_stop": None}.get(label, len(text) // 3 - 1)
            assert stop == want, (c.name, stop)
            if label in ("n0", "n1", "n2"):
                assert bytes(text[15:18]).index(b"N") == int(label[1]) and bytes(text).count(b"N") == 1, c.name
            if label == "nrun":
                assert bytes(text[60:69]) == bytes(text[60:62]) + b"NNNNN" + bytes(text[67:69]) and b"N" not in bytes(text[60:62]) + bytes(text[67:69]), c.name
            if label == "stop_n":
                assert bytes(text[90:93]) == b"TAN", c.name
            if label == "two_stops":
                assert bytes(text[360:363]) in STOPS, c.name
        elif kind == "empty_slot":
            assert U.cull_model(h, order).all(), c.name
            empty = np.flatnonzero(_max_codons(h) == 0)
            where = info["where"]
            if where == "mid":
                assert len(empty) == 2 and empty[1] == empty[0] + 1 and 0 < empty[0] and empty[1] < len(h) - 1, c.name
            else:
                assert empty.tolist() == [where[0] % len(h)], c.name
        elif kind == "codons":
            assert U.cull_model(h, order).all() and int(_max_codons(h).sum()) == info["total"], c.name
            if "stop_at" in info:
                assert int(_max_codons(h)[0]) < U.CODON_ROUND <= info["stop_at"] == int(_max_codons(h)[0]) + _first_stop(_text(R, h[1]), 1), c.name
        elif kind == "edge":
            x = h[h["gene"] == R.S][-1] if R.S != R.g0 else h[-1]
            clen = int(R.genome.contigs.lengths[x["contig"]])
            dist = int(x["t_start"]) if info["edge"] == "left" else clen - int(x["t_end"])
            other = clen - int(x["t_end"]) if info["edge"] == "left" else int(x["t_start"])
            assert dist == info["dist"] and other > U.EDGE_TOL and info["dist"] in (U.EDGE_TOL, U.EDGE_TOL + 1), c.name
            low = (info["edge"] == "left") == (x["strand"] > 0)  # the query end that faces the edge
            assert ((x["q_start"] > 0) if low else (x["q_end"] < L[R.S])) == info["clipped"], c.name
        elif kind == "prot_cov":
            n, lg = R.cstop[info["label"]], int(L[info["gene"]])
            want = {"stop_lo": -1, "c_lo": -1, "c_eq": 0, "stop_hi": 1, "c_hi": 1}[info["label"]]
            assert np.sign(30 * n - 9 * lg) == want and (3.0 * n / lg < 0.90) == (want < 0), c.name
            nxt = n + (1 if want < 0 else -1)
            assert want == 0 or np.sign(30 * nxt - 9 * lg) != want, c.name  # the nearest value on its side
        elif kind == "identity":
            thr = np.float32(db.metadata.id_threshold)
            ids = exp["protein_identities"][exp["gene_hits.gene_indices"] == info["gene"]]
            if info["tag"] == "below":
                assert all(v < thr for v in ids), c.name  # (outside the locus the hit is gone altogether)
            else:
                assert len(ids) == 1 and ((ids[0] == thr) if info["tag"] == "at" else (ids[0] > thr)), (c.name, ids)
        elif kind == "mean":
            assert int((exp["gene_states"] == 0).sum()) == info["n"] == len(h) == len(exp["protein_identities"]), c.name
            if info["n"] > 10:  # a sum whose association shows: adding one by one gives other bits than numpy's blocks
                ids, one_by_one = exp["protein_identities"], np.float32(0)
                for v in ids:
                    one_by_one = np.float32(one_by_one + v)
                assert one_by_one.tobytes() != np.float32(np.add.reduce(ids)).tobytes() and len(np.unique(ids)) >= 30, c.name
        elif kind == "equal_cov":
            x = h[h["gene"] == info["gene"]]
            assert len(x) == 2 and len(set((x["q_end"] - x["q_start"]).tolist())) == 1 and x["score"][0] != x["score"][1], c.name
            assert not (x["contig"][0] == x["contig"][1]), c.name  # (both survive the cull)
        elif kind == "all_spurious":
            m = U.piece_model(db, h, scalars["best_locus_idx"], tol)
            assert len(m["kept"]) == len(h) > 0 and not m["expected"].any() and not m["pieces"] and not m["inside"].any(), c.name
            assert len(exp["gene_states"]) == 0, c.name  # the reference reports no hit: every kept one was spurious
        elif kind == "extra_beside":
            assert db.extra_genes[info["gene"]] and int((h["gene"] == info["gene"]).sum()) == 1, c.name
            assert sorted(set(h["gene"].tolist()) - {info["gene"]}) == list(range(R.g0, R.g0 + R.n0)), c.name
        elif kind == "two_contigs":
            a, b = h[h["gene"] == info["a"]][0], h[h["gene"] == info["b"]][0]
            assert (a["t_start"], a["t_end"]) == (b["t_start"], b["t_end"]) and a["contig"] != b["contig"] and a["t_end"] > a["t_start"], c.name
            m = U.piece_model(db, h, scalars["best_locus_idx"], tol)
            ka, kb = (np.flatnonzero(m["kept"]["gene"] == x) for x in (info["a"], info["b"]))
            assert len(ka) == len(kb) == 1 and m["cluster"][ka[0]] != m["cluster"][kb[0]], c.name  # both kept, never one cluster
        elif kind == "linkage_through":
            first, long_, third = (h[h["gene"] == info[x]][0] for x in ("first", "long", "third"))
            assert int(third["t_start"]) - int(long_["t_end"]) == tol + c.pair[1] and int(third["t_start"]) - int(first["t_end"]) > tol, c.name
            assert first["t_start"] < long_["t_start"] <= first["t_end"] + tol and long_["t_end"] > first["t_end"], c.name
            m = U.piece_model(db, h, scalars["best_locus_idx"], tol)
            assert len(m["kept"]) == 3 and len(set(m["cluster"].tolist())) == 1 + c.pair[1], c.name
        elif kind == "no_primary":
            m = U.piece_model(db, h, scalars["best_locus_idx"], tol)
            rows = np.flatnonzero(m["kept"]["gene"] == info["gene"])
            weak = rows[np.argmin(m["kept"]["score"][rows])]
            assert len(rows) == 2 and m["expected"][weak] and not m["primary"][weak] and not m["inside"][weak], c.name
            assert int((m["cluster"] == m["cluster"][weak]).sum()) == 1 and len(m["pieces"]) == 1 and len(set(m["cluster"].tolist())) == 2, c.name
        elif kind == "primary":
            rows = np.flatnonzero(h["gene"] == info["gene"])
            assert len(rows) == 2 and rows[1] == rows[0] + 1, c.name
            sc = h["score"][rows]
            assert (sc[0] == sc[1]) if info["equal"] else (sc[1] > sc[0]), c.name  # the later row in emission order never scores less
            m = U.piece_model(db, h, scalars["best_locus_idx"], tol)
            kr = np.flatnonzero(m["kept"]["gene"] == info["gene"])
            assert len(kr) == 2 and m["primary"][kr].tolist() == ([True, False] if info["equal"] else [False, True]), c.name
            assert m["cluster"][kr[0]] != m["cluster"][kr[1]] and len(m["pieces"]) == (1 if info["equal"] else 2), c.name
        elif kind == "mean_pos":
            m = U.piece_model(db, h, scalars["best_locus_idx"], tol)
            assert len(m["pieces"]) == 1 and int(m["primary"].sum()) == info["n"], c.name
            assert m["pieces"][0][4] == float(db.gene_positions[h["gene"][0]]), c.name
        elif kind == "touch":
            m = U.piece_model(db, h, scalars["best_locus_idx"], tol)
            assert len(m["pieces"]) == 1 and len(m["kept"]) == 2, c.name
            x = np.flatnonzero(m["kept"]["gene"] == info["gene"])[0]
            gap = int(m["kept"]["t_start"][x]) - m["pieces"][0][2] if info["end"] == "end" else m["pieces"][0][1] - int(m["kept"]["t_end"][x])
            assert gap == c.pair[1] and not m["expected"][x] and m["inside"][x] == (gap == 0), c.name
            assert m["cluster"][0] == m["cluster"][1], c.name  # one cluster either way: only the closed interval decides
        elif kind == "found":
            want = [x for x in range(R.g0, R.g0 + R.n0) if x not in info["absent"]]
            assert h["gene"].tolist() == want and scalars["best_locus_idx"] == 0, c.name
            ids = [str(db.genes.ids[x]) for x in info["absent"]]
            assert all(any(i in str(miss) for miss in scalars["missing_expected_genes"]) for i in ids), c.name
            assert len(scalars["missing_expected_genes"]) == len(ids), c.name
        elif kind == "partial_truncated":
            x = h[h["gene"] == R.S][-1] if R.S != R.g0 else h[-1]
            assert int(x["t_start"]) == U.EDGE_TOL and x["strand"] == 1 and (x["q_start"] > 0) == info["clipped"], c.name
            clen = int(R.genome.contigs.lengths[x["contig"]])
            assert clen - int(x["t_end"]) > U.EDGE_TOL and _first_stop(_text(R, x), 1) == 1 and 3.0 * 1 / L[R.S] < 0.90, c.name
        elif kind == "short_contig":
            x = h[h["contig"] == R.contig["short"]][0]
            clen = int(R.genome.contigs.lengths[x["contig"]])
            assert clen < L[x["gene"]] and (int(x["t_start"]), int(x["t_end"])) == (0, clen), c.name
        else:
            raise AssertionError(f"{c.name}: no proof for a case of kind {kind!r}")
    assert {"cov", "tie", "zero", "overlap", "empty", "tie_order", "round", "resident", "linkage", "vote", "frame", "text", "empty_slot",
            "codons", "edge", "prot_cov", "identity", "mean", "equal_cov", "all_spurious", "two_contigs", "linkage_through", "no_primary",
            "primary", "mean_pos", "touch", "found", "partial_truncated", "short_contig"} <= seen  # fmt: skip
    assert frames == {(q, r, s) for q in range(3) for r in range(3) for s in (1, -1)}


@pytest.mark.parametrize("key,name", _ids())
def test_core_header_gives_the_references_record(key, name, oracle):
    genome, recorded = U.load_rules(key)
    _, _, hits, exp, scalars, kwargs = next(r for r in recorded if r[1] == name)
    db = load_db(key)
    typer = _typer(db, kwargs)
    r = U.core_records(db, typer, genome, hits, oracle)
    assert r["final"].tobytes() == exp["last_scores"].tobytes(), "penalised locus scores"
    assert r["completeness"].tobytes() == exp["last_completeness"].tobytes(), "locus completeness"
    assert r["best"] == scalars["best_locus_idx"]
    res = B.assemble(typer, genome.id, r["summary"], r["kept"], r["pieces"], r["scores"][r["best"]], genome=genome)
    U.check_against_fixture(res, exp, scalars)
    # the batched mean identity: float32(float64(ident_sum) / n_normal) with kp_np_sum_f32's sum is the reference's np.mean
    n_normal = int(r["summary"]["n_normal"])
    assert n_normal == int(((r["kept"]["state"] == 0) & ((r["kept"]["flags"] & B.F_SPURIOUS) == 0)).sum())
    if n_normal:
        mean = np.float32(np.float64(r["summary"]["ident_sum"]) / n_normal)
        assert np.float64(mean).tobytes() == np.float64(exp["percent_identity"]).tobytes(), (mean, exp["percent_identity"])
