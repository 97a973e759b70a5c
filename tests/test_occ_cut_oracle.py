"""What the inputs of tests/occ_cut_util.py are, by the CPU oracle alone: where gene R's stretch lies in the sorted anchor list
against the rounds of 64, the eight wave slices and the 512-entry compaction chunks of kp_occ_cut_kernel; how many
(gene/strand, diagonal) pairs and anchors per seed a gene has, per counting window; whether the assembly asks for its own
mid_occ and what it is; how many distinct minimizers it has and which count sits at the quantile's index; where contigs and N
runs lie against the chunks of kp_occ_sketch_kernel.  Every edge is derived from the constants that tests/occ_cut_util.py
was built for, and the first test reads them out of csrc/kp_chain.hip, csrc/kp_align.hip and include/kp_spec.h: whoever
changes one gets a failure here, not an edge that tests/test_gpu_occ_cut.py quietly no longer meets."""

import numpy as np
import pytest

from kaptive_amd.core.seq import CHAR_MAP
from tests import occ_cut_util as U


@pytest.fixture(scope="module")
def built(oracle):
    return U.built(oracle)


@pytest.fixture(scope="module")
def rows(oracle, built):
    return {g: [U.measure(oracle, built["odb"], c) for c in cases] for g, cases in built["groups"].items()}


# keys of a case's ``want`` that the group's own test checks, not _check
CHECKED_ELSEWHERE = {"marks", "runs", "spans", "ctg_len", "n_in_chunk0", "min_padded", "repeats_after", "all_counts", "min_distinct"}


def _check(cases, rows, extra=None):
    """Every key of a case's ``want`` equals what the oracle measured (dicts: every entry given), the label's claim about
    s, e and n holds, and the table the assembly would count into is at most half full."""
    bad = []
    for c, r in zip(cases, rows):
        for key, want in c.want.items():
            if key in CHECKED_ELSEWHERE:
                continue  # (by the group's own test)
            assert key in r, f"{c.label}: nothing measures '{key}'"
            got = r[key]
            if isinstance(want, dict):
                ok = all(got.get(g) == v if not isinstance(v, dict) else all(got.get(g, {}).get(p) == x for p, x in v.items()) for g, v in want.items())
            else:
                ok = got == want
            if not ok:
                bad.append(f"{c.label}: {key} is {got if not isinstance(got, dict) else {g: got.get(g) for g in want}}, not {want}")
        if c.holds is not None and not c.holds(r):
            bad.append(f"{c.label}: s = {r['s']}, e = {r['e']}, n = {r['n']} do not land where the label says")
        if 2 * r["distinct"] > r["table_entries"]:
            bad.append(f"{c.label}: {r['distinct']} distinct minimizers would fill more than half of {r['table_entries']} entries")
        if extra:
            bad += [f"{c.label}: {m}" for m in extra(c, r)]
    brief = [{k: v for k, v in r.items() if k not in ("dropped", "counts")} for r in rows]
    assert not bad, "\n".join(bad) + "\n\nthe cases:\n" + U.describe(cases, brief)


def test_sizes_follow_the_constants_in_the_sources(oracle):
    assert U.kernel_constants() == U.EXPECTED_CONSTANTS, "a constant moved: rebuild the inputs of tests/occ_cut_util.py around it"
    # kp_spec.h: kth = (int)((1 - 2e-4f) n) steps from n - 1 to n - 2 behind n = 5000 and to n - 3 at 10 001
    assert [n - U.kth_of(n) for n in (1, 4999, 5000, 5001, 5002, 10_000, 10_001)] == [1, 1, 1, 2, 2, 2, 3]
    assert U.SECOND_CHUNK == 8_388_608 and U.BLOCK == 512 and U.FLANK > U.K + U.C["KP_W"]
    for g, positions in U.EDGE_POSITIONS.items():  # the database has a seed there
        assert set(positions) <= set(oracle.seeds(CHAR_MAP[U.genes()[g]])[0].tolist()), f"gene {g} has no seed at {positions}: pick another GENE_SEED"
    assert U.GENE_LEN[U.G_L] > 2 * U.BINS and [U.GENE_LEN[g] - U.BINS for g in (U.G_B1024, U.G_B1025, U.G_B1039)] == [0, 1, U.K]


def test_list_cases_land_where_their_labels_say(built, rows):
    """Group A: s, e and n against rounds, slices and compaction chunks; every case drops R's two repeated seeds -- and only
    them -- at the floor, without asking for the quantile."""
    cases = built["groups"]["A"]

    def extra(c, r):
        over = r["over"].get(U.G_R)
        if over != [2]:
            yield f"R has {over} seeds beyond the floor, not two"
        d = np.asarray(r["dropped"])
        if len(d) == 0 or not ((d >= r["s"]) if "two_genes" in c.label else (d >= r["s"]) & (d < r["e"])).all():
            yield "the dropped anchors are not R's"
        if c.label.startswith("chunk_511_512") and not {U.BLOCK - 1, U.BLOCK} <= set(r["dropped"]):
            yield "indices 511 and 512 are not both dropped"
        if c.label.startswith("chunk_drop_then_keep") and not (d.max() < U.BLOCK < r["n"]):
            yield "drops and kept anchors do not sit in chunk 0 and chunk 1"
        if c.label.startswith("all_dropped") and r["kept"] != 0:
            yield f"{r['kept']} anchors are kept"
        if c.label.startswith("first") and 0 not in r["dropped"]:
            yield "index 0 is kept"
        if c.label.startswith("last") and r["n"] - 1 not in r["dropped"]:
            yield "the last index of the list is kept"

    _check(cases, rows["A"], extra)
    labels = " ".join(c.label for c in cases)
    for word in ("round_s0", "round_s1", "round_s63", "round_e_inside", "round_e_on_end", "round_e_one_past", "round_headless", "last_n64", "last_odd",
                 "first", "slice_s_at_start", "slice_start_1_in", "slice_start_70_in", "slice_covered", "slice_e_at_hi", "slice_past_hi", "one_wave",
                 "chunk_drop_then_keep", "chunk_511_512", "all_dropped", "two_genes_two_waves"):  # fmt: skip
        assert word in labels, f"the case {word} is gone"


def test_counting_cases_have_the_counts_their_labels_say(built, rows):
    """Group B: anchors per seed on both sides of KP_MID_OCC with one and with two gene/strand values, ten and eleven pairs
    without a seed beyond ten, a seed on either side of the counting window's edge and on a gene's last position, and L with
    drops in its first and third window."""
    cases = built["groups"]["B"]

    def extra(c, r):
        if r["n_over_max"] >= U.C["KP_MIN_ANCHORS"]:
            yield "the assembly asks for its quantile: the floor would not decide"
        if c.label.startswith("edge_"):
            (gene, by_pos), = c.want["counts"].items()
            (pos, _), = by_pos.items()
            strands = {int(x) & 1 for x in (built["odb"].anchors(c.asm.packed(), cut=False) >> np.uint64(U.TOP_SHIFT)).tolist()
                       if int(x) >> 1 == gene}
            if ("both" in c.label) != (strands == {0, 1}):
                yield f"the seed's anchors lie on strands {strands}"

    _check(cases, rows["B"], extra)
    edges = {(g, p) for c in cases if c.label.startswith("edge_") for g, d in c.want["counts"].items() for p in d}
    L = U.GENE_LEN
    assert edges == {(U.G_B1024, L[U.G_B1024] - U.K), (U.G_B1025, L[U.G_B1025] - U.K), (U.G_B1039, U.BINS - 1), (U.G_B1039, U.BINS),
                     (U.G_L, U.BINS - 1), (U.G_L, U.BINS), (U.G_L, L[U.G_L] - U.K)}, edges  # fmt: skip


def test_floor_or_quantile_cases_ask_what_their_labels_say(built, rows):
    """Group C: two seeds beyond the floor never ask, a third -- in the same window, in another window, NOT in another gene --
    does; the quantile of these assemblies is above the floor except where a background pulls it below."""
    cases = built["groups"]["C"]

    def extra(c, r):
        if "min_distinct" in c.want and r["distinct"] < c.want["min_distinct"]:
            yield f"{r['distinct']} distinct minimizers, fewer than {c.want['min_distinct']}"
        for g, count in c.want.get("all_counts", {}).items():
            if set(r["counts"].get(g, {}).values()) != {count}:
                yield f"gene {g} has seeds with {r['counts'].get(g)} anchors, not {count} each"
        if not c.label.startswith("quantile_at_floor") and r["count_at_kth"] + 1 <= U.MID:
            yield f"the quantile {r['count_at_kth']} + 1 is not above the floor"

    _check(cases, rows["C"], extra)


def test_sketch_cases_lie_where_their_labels_say(oracle, built, rows):
    """Group D: contig lengths, contig ends and starts, N runs and low-complexity runs against the chunk edges of the padded
    space; every assembly asks for its quantile, so the device fills a table."""
    cases = built["groups"]["D"]
    _check(cases, rows["D"])
    by = {c.asm.id: c for c in cases}
    chunk, warm = U.CHUNK, U.WARM
    pa = by["contig_lengths"].asm.packed()
    assert tuple(pa.ctg_len[: len(by["contig_lengths"].want["ctg_len"])].tolist()) == (14, 15, 24, 25, chunk - 1, chunk, chunk + 1)
    c = by["contig_layouts"]
    pa = c.asm.packed()
    start, length = pa.ctg_start.tolist(), pa.ctg_len.tolist()
    assert all(s + n <= chunk for s, n in zip(start[:5], length[:5])) and all(15 <= n <= 40 for n in length[:5])
    ends = [(s + n) % chunk for s, n in zip(start[5:8], length[5:8])]
    assert ends == [1, 25, 26] and all(s // chunk < (s + n - 1) // chunk for s, n in zip(start[5:8], length[5:8])), (start, length)
    s, n = start[9], length[9]
    assert (s, n) == c.want["marks"]["warm_start"] and 0 < chunk - s % chunk < warm and s + n > (s // chunk + 1) * chunk
    c = by["n_runs"]
    runs = {tuple(r) for r in np.asarray(c.asm.packed().n_runs).reshape(-1, 2).tolist()}
    want = c.want["runs"]
    n0 = int(c.asm.packed().ctg_len[0])
    assert {tuple(v) for v in want.values()} <= runs, (runs, want)
    assert want["ends_at_edge"][1] % chunk == 0 and want["starts_at_edge"][0] % chunk == 0
    assert want["whole_chunk"][0] % chunk == 0 and want["whole_chunk"][1] - want["whole_chunk"][0] == chunk
    edge = (want["in_warm_up"][1] // chunk + 1) * chunk
    assert edge - warm <= want["in_warm_up"][0] and want["in_warm_up"][1] <= edge
    assert want["first_base"] == (0, 1) and want["last_base"] == (n0 - 1, n0)
    c = by["low_complexity"]
    assert sorted(len(u) for u in c.want["spans"]) == [1, 2, 3, 7, 12]
    assert all(a // chunk + 1 == (b - 1) // chunk for a, b in c.want["spans"].values())
    x, cnt = U.minimizer_histogram(oracle, c.asm.packed())
    assert cnt.max() > 100, "the homopolymer does not repeat one value"


def test_second_chunk_case_is_past_the_first_round_of_chunks(built, rows):
    (c,), (r,) = built["groups"]["D2"], rows["D2"]
    _check([c], [r])
    pa = c.asm.packed()
    assert r["padded"] > U.SECOND_CHUNK + 250_000 and int(pa.ctg_start[1]) > U.SECOND_CHUNK and r["table"]
    assert r["count_at_kth"] < U.MID and r["mid_occ"] == U.MID  # millions of distinct values: the quantile is far below the floor, which holds
    assert r["drops"], "the gene under test loses nothing"


def test_quantile_cases_have_the_distinct_values_and_counts_their_labels_say(built, rows):
    """Group E: exactly 4999 ... 10 001 distinct minimizers with the counts 2000, 1500 and 11 on top, so that mid_occ follows
    kth; one value 2046, 2047, 2048 and 5000 times at the quantile (the histogram's last bin and its cap)."""
    cases = built["groups"]["E"]
    _check(cases, rows["E"])
    got = {c.asm.id: r["mid_occ"] for c, r in zip(cases, rows["E"])}
    assert got == {"distinct_4999": 2001, "distinct_5000": 2001, "distinct_5001": 1501, "distinct_5002": 1501, "distinct_10000": 1501,
                   "distinct_10001": 12, "poly_a_2046": 2047, "poly_a_2047": 2048, "poly_a_2048": 2048, "poly_a_5000": 2048}, got  # fmt: skip


def test_single_value_cases_hold_one_distinct_minimizer(oracle):
    """Group E, a database of its own: a gene with a homopolymer run, assemblies of poly-A alone.  One distinct minimizer asks
    for the quantile (its value sits on several forward positions of the gene): n = 1, kth = 0, mid_occ = its count + 1."""
    from kaptive_amd.pack import pack_sequences_flat

    odb = oracle.OracleDB(*pack_sequences_flat(U.single_value_gene_sequences()))
    assert U.POLY_RUN == U.K + U.C["KP_W"] + 1 and U.kth_of(1) == 0
    for c in U.single_value_cases():
        pa = c.asm.packed()
        x, cnt = U.minimizer_histogram(oracle, pa)
        n_over_max, mid_occ, asks = odb.occ(pa)
        assert len(x) == c.want["distinct"] == 1 and U.kth_of(len(x)) == c.want["kth"], (c.label, x, cnt)
        assert asks and n_over_max >= U.C["KP_MIN_ANCHORS"] and int(cnt[0]) > U.MID, (c.label, n_over_max, cnt)
        assert mid_occ == min(int(cnt[0]), U.C["KP_MID_OCC_HIST"] - 1) + 1, (c.label, mid_occ, cnt)
        before, after = odb.anchors(pa, cut=False), odb.anchors(pa)
        assert len(before) == len(after) > 0, c.label  # the quantile is the value's own count: nothing is cut
        assert 2 * len(x) <= 1 << U.table_log2(pa.n_bases)
