"""The protein DP's case tables (tests/protein_paths_util.py) without a GPU: the oracle equals the reference-recorded
seeded fixture, and the tables reach what they are for -- every path of kp_prot.hip in both modes with scoring, gapped
pairs, and every threshold of the dispatch on both sides.  The conditions are on the inputs and judged on the oracle's
rows alone; tests/test_gpu_protein_paths.py compares the device with the oracle on the same tables."""

from collections import Counter

import numpy as np
import pytest

from tests import protein_paths_util as U

MIN_PAIRS, MIN_SCORING, MIN_GAPPED = 6, 4, 2


@pytest.fixture(scope="module")
def unseeded(oracle):
    cases = U.unseeded_table()
    q, t = U.pack(cases)
    return cases, U.classify(cases), oracle.protein_align(q.seqs, q.offsets, q.lengths, t.seqs, t.offsets, t.lengths)


@pytest.fixture(scope="module")
def seeded(oracle):
    """Cases, paths and oracle rows of the seeded table in table order (one oracle call per k, as on the device)."""
    cases, paths, rows = [], [], []
    for k, group in U.by_k(U.seeded_table()).items():
        q, t = U.pack(group)
        cases += group
        paths += U.classify(group)
        rows.append(oracle.protein_align_seeded(q.seqs, q.offsets, q.lengths, t.seqs, t.offsets, t.lengths, [c[3] for c in group], k))
    return cases, paths, np.concatenate(rows)


def _coverage(paths, rows, reachable):
    bad, lines = [], []
    for path in reachable:
        sel = np.array([p == path for p in paths])
        n, scoring, gapped = int(sel.sum()), int((rows[sel, 0] > 0).sum()), int((rows[sel, 3] > 0).sum())
        lines.append(f"{path:7s} pairs {n:4d}  score>0 {scoring:4d}  gaps>0 {gapped:4d}")
        need_scoring = 0 if path == "empty" else MIN_SCORING
        need_gapped = 0 if path in ("empty", "exact") else MIN_GAPPED  # (an empty pair is all zeros, the shortcut's has no gap)
        if n < MIN_PAIRS or scoring < need_scoring or gapped < need_gapped:
            bad.append(path)
    return bad, "\n".join(lines)


def test_oracle_equals_the_reference_recorded_seeded_fixture(oracle, golden_dir):
    z = np.load(golden_dir / "protein_dp_seeded.npz")
    want = np.stack([z[c] for c in U.COLS], axis=1)
    assert len(want) >= 300 and set(z["k"].tolist()) == set(U.GOLDEN_KS)
    assert int(z["q_lengths"].max()) <= 60 and int(z["t_lengths"].max()) <= 60
    assert (want[:, 0] > 0).sum() >= 200 and (want[:, 3] > 0).sum() >= 20 and (want == 0).all(axis=1).sum() >= 50
    for k in U.GOLDEN_KS:
        sel = np.flatnonzero(z["k"] == k)
        got = oracle.protein_align_seeded(z["q_seqs"], z["q_offsets"][sel], z["q_lengths"][sel], z["t_seqs"], z["t_offsets"][sel],
                                          z["t_lengths"][sel], z["offsets"][sel], k)  # fmt: skip
        bad = np.flatnonzero((got != want[sel]).any(axis=1))
        assert len(bad) == 0, (k, z["names"][sel[bad[:3]]], want[sel[bad[:3]]], got[bad[:3]])


def test_classifier_constants_are_those_of_the_sources():
    import re
    from pathlib import Path

    root = Path(__file__).resolve().parent.parent
    hip = (root / "kaptive_amd" / "csrc" / "kp_prot.hip").read_text()
    spec = (root / "include" / "kp_spec.h").read_text()
    for name in ("REG_MAX_LEN", "S2_CAP", "WAVE_NC_MAX", "QP"):
        assert int(re.search(rf"constexpr int {name} = (\d+);", hip).group(1)) == getattr(U, name), name
    assert int(re.search(r"#define KP_PROT_K (\d+)", spec).group(1)) == U.KP_PROT_K
    assert "tests/protein_paths_util.py" in hip


def test_unseeded_table_reaches_every_path(unseeded):
    cases, paths, rows = unseeded
    assert len({c[0] for c in cases}) == len(cases)
    bad, table = _coverage(paths, rows, U.PATHS)
    assert not bad, f"unseeded cells below {MIN_PAIRS} pairs / {MIN_SCORING} scoring / {MIN_GAPPED} gapped: {bad}\n{table}"
    assert max(max(len(c[1]), len(c[2])) for c in cases) <= 2600
    assert sum(max(len(c[1]), len(c[2])) > 2200 for c in cases) == 1  # the one large strips case


def test_unseeded_table_holds_both_sides_of_every_threshold(unseeded):
    cases, paths, rows = unseeded
    by_name = {c[0]: (len(c[1]), len(c[2]), p) for c, p in zip(cases, paths)}
    # |len1 - len2| around 23 (three / four diagonals per lane), 31 (which kernel), 127 (four / eight per lane), 255 (registers or not)
    want = {22: "quad3", 23: "quad4", 30: "quad4", 31: "wave4", 126: "wave4", 127: "wave8", 254: "wave8"}
    for d in U.UNSEEDED_DS:
        for side in ("qshort", "qlong"):
            l1, l2, small = by_name[f"d{d}_{side}_small"]
            a1, a2, above = by_name[f"d{d}_{side}_above"]
            assert abs(l1 - l2) == d == abs(a1 - a2) and (l1 < l2) == (side == "qshort") == (a1 < a2)
            assert max(l1, l2) <= U.REG_MAX_LEN < max(a1, a2)
            if d < 255:
                assert small == want[d], (d, side, small)
                assert above == ("strips" if side == "qlong" else want[d].replace("quad3", "wave4").replace("quad4", "wave4")), (d, side, above)
            else:
                assert small == ("rows4" if side == "qshort" else "strips") and above == "strips", (d, side, small, above)
        # ... and a pair whose best path ends on the band's outermost diagonal j - i = k, which a band one diagonal short loses
        i = [c[0] for c in cases].index(f"d{d}_outer")
        assert paths[i] == by_name[f"d{d}_qshort_small"][2] and len(cases[i][2]) - len(cases[i][1]) == d
        assert rows[i, 7] - rows[i, 5] == d + 1 == U.band_k(len(cases[i][1]), len(cases[i][2]), False, None), (d, rows[i])
        assert rows[i, 3] >= 1 and rows[i, 1] > 100
    # staging limits, in both roles
    expect = {(763, 768): "quad3", (764, 769): "wave4", (768, 763): "quad3", (769, 764): "strips", (768, 768): "quad3",
              (769, 769): "strips", (768, 769): "wave4", (769, 768): "strips", (200, 2048): "rows4", (200, 2049): "strips",
              (700, 2048): "strips", (700, 2049): "strips", (128, 428): "rows2", (129, 429): "rows4", (256, 556): "rows4",
              (257, 557): "rows6", (384, 684): "rows6", (385, 685): "strips", (500, 900): "strips", (768, 1100): "strips",
              (64, 2100): "strips", (65, 2100): "strips", (128, 2100): "strips", (129, 2100): "strips", (384, 2048): "rows6"}  # fmt: skip
    for (l1, l2), path in expect.items():
        assert by_name[f"edge_{l1}x{l2}"] == (l1, l2, path), (l1, l2, by_name[f"edge_{l1}x{l2}"])
    # strips whose window is exactly one and two published chunks, the staged target residues, and one more
    for cols, l1, l2 in U.STRIP_WINDOWS:
        assert by_name[f"window{cols}_{l1}x{l2}"][2] == "strips"
        assert cols in U.strip_windows(l1, l2, U.band_k(l1, l2, False, None)), (cols, l1, l2)
    assert by_name["biggest_strips"][2] == "strips"
    assert by_name["exact_repeat_narrow"][2] == by_name["exact_repeat_wide"][2] == by_name["exact_800_of_800"][2] == "exact"
    # ties and bytes outside the alphabet on every DP path
    for path in U.PATHS[2:]:
        assert by_name[f"tie_{path}_w_first"][2] == by_name[f"tie_{path}_w_last"][2] == by_name[f"odd_{path}"][2] == path, path
        i = [c[0] for c in cases].index(f"odd_{path}")
        assert not set(cases[i][1]) <= set(U.AA.tolist()) and not set(cases[i][2]) <= set(U.AA.tolist()) | {ord("*")}
        assert rows[i, 0] > 0
    # the mixed quads: the DP pair in each of the wave's four groups, beside an empty, an exact and a wide-kernel pair
    names = [c[0] for c in cases]
    groups = set()
    for r in range(4):
        at = [names.index(f"mixed{r}_{role}") for role in ("dp", "empty", "exact", "wide")]
        assert len({i // 4 for i in at}) == 1 and [paths[i] for i in at] == ["quad3", "empty", "exact", "wave4"]
        groups.add(at[0] % 4)
    assert groups == {0, 1, 2, 3}


def test_same_pair_in_different_company_has_the_same_oracle_rows(unseeded):
    cases, paths, rows = unseeded
    pairs = U.company_pairs(cases)
    assert len(pairs) == 3
    for a, b in pairs:
        assert cases[a][1:3] == cases[b][1:3] and a // 4 != b // 4
        assert (paths[a], paths[b]) == ("quad3", "quad4")  # `narrow` true in one wave, false in the other
        assert np.array_equal(rows[a], rows[b]) and rows[a, 0] > 0


def test_seeded_table_reaches_every_path(seeded):
    cases, paths, rows = seeded
    assert len({c[0] for c in cases}) == len(cases)
    bad, table = _coverage(paths, rows, U.SEEDED_PATHS)
    assert not bad, f"seeded cells below {MIN_PAIRS} pairs / {MIN_SCORING} scoring / {MIN_GAPPED} gapped: {bad}\n{table}"
    assert "exact" not in paths and max(max(len(c[1]), len(c[2])) for c in cases) <= 2600
    # every k reaches every path open to it, each with a scoring pair at a non-zero offset
    for k in U.SEEDED_KS:
        got = Counter(p for c, p, r in zip(cases, paths, rows) if c[4] == k and r[0] > 0 and c[3] != 0)
        open_ = {"quad3" if k <= 23 else "quad4", "wave4", "strips"} if k <= 31 else {"wave4" if k <= 127 else "wave8", "strips"} \
            if k <= 255 else {"rows2", "rows4", "rows6", "strips"}  # fmt: skip
        assert open_ <= set(got), (k, open_, got)
        assert set(p for c, p in zip(cases, paths) if c[4] == k) == open_ | {"empty"}, k
    # the narrow-band wave form exists only by the target's length
    assert sum(p == "wave4" and c[4] <= 31 and 768 < len(c[2]) <= 2048 and r[0] > 0 for c, p, r in zip(cases, paths, rows)) >= 20
    by_name = {c[0]: p for c, p in zip(cases, paths)}
    expect = {31: ("quad4", "strips", "wave4", "wave4", "strips", "wave4", "strips", "wave4", "wave4", "quad4", "quad4", "quad4", "quad4"),
              32: ("wave4", "strips", "wave4", "wave4", "strips", "wave4", "strips", "wave4", "wave4", "wave4", "wave4", "wave4", "wave4"),
              255: ("wave8", "strips", "wave8", "wave8", "strips", "wave8", "strips", "wave8", "wave8", "wave8", "wave8", "wave8", "wave8"),
              256: ("strips", "strips", "rows6", "rows6", "strips", "strips", "strips", "rows6", "strips", "rows2", "rows4", "rows4", "rows6")}  # fmt: skip
    for k, want in expect.items():
        got = tuple(by_name[f"k{k}_edge_{l1}x{l2}"] for l1, l2 in U._SEEDED_EDGE_SHAPES)
        assert got == want, (k, got)


def test_seeded_offsets_do_what_their_names_say(seeded):
    cases, paths, rows = seeded
    n_out = n_corner = n_edge = 0
    by_name = {c[0]: (c, r) for c, r in zip(cases, rows)}
    for (name, q, t, off, k), row in zip(cases, rows):
        if not U.in_band_any(len(q), len(t), off, k):
            assert (row == 0).all(), (name, row)  # nothing in band (or nothing to align): all eight fields are 0
            n_out += "_out_" in name
        if name.endswith(("_corner_q", "_corner_t")):
            # exactly one cell of the matrix is in band: a one-residue alignment or nothing
            i, j = (len(q), 1) if name.endswith("_q") else (1, len(t))
            assert U.in_band_any(len(q), len(t), off, k)
            assert not U.in_band_any(len(q), len(t), off + (1 if name.endswith("_q") else -1), k)
            assert tuple(row) in ((0,) * 8, (row[0], int(q[i - 1] == t[j - 1]), int(q[i - 1] != t[j - 1]), 0, i - 1, i, j - 1, j)), (name, row)
            n_corner += 1
        if name.endswith(("_edge_hi", "_edge_lo")) and k >= 7:
            # the homology sits on the band's outermost diagonal and is found; one diagonal further it is not
            true_row = by_name[name.rsplit("_edge_", 1)[0] + "_true"][1]
            past_row = by_name[name.replace("_edge_", "_past_")][1]
            assert row[0] > past_row[0], (name, row, past_row)
            assert row[0] <= true_row[0] or k == 0
            n_edge += 1
    assert n_out >= 4 * len(U.SEEDED_KS) * 4 and n_corner >= 2 * len(U.SEEDED_KS) * 4 and n_edge >= 40
    # identical sequences, offset 0: the DP finds the whole diagonal
    for k in U.SEEDED_KS:
        for n, what in ((150, "reg"), (800, "strips")):
            c, row = by_name[f"k{k}_identical_{what}_{n}"]
            assert tuple(row[1:]) == (n, 0, 0, 0, n, 0, n) and row[0] > 4 * n
    # ties beyond the register forms, at offsets other than 0
    for k in (256, 300):
        for what in ("rows2", "rows4", "rows6", "strips"):
            for off in (-1, 7, -40):
                c, row = by_name[f"k{k}_tie_{what}_off{off}"]
                assert row[0] > 0 and U.path_of(len(c[1]), len(c[2]), True, k, False) == what


def test_big_batches_take_the_second_trip_of_the_pair_loop(oracle):
    for wide in (False, True):
        qs, ts, offs = U.big_batch(wide=wide)
        n = len(qs)
        assert n == U.BIG_N and n % 4 == 3 and len(offs) == n and offs.min() == -6 and offs.max() == 6
        quads = (n + 3) // 4
        assert quads > U.BIG_BLOCKS and 800 <= quads - U.BIG_BLOCKS <= 1000  # blocks that stage a second quad
        lq, lt = np.array([len(x) for x in qs]), np.array([len(x) for x in ts])
        small = np.ones(n, bool)
        if wide:
            small = ~((lq == 260) & (lt == 300))
            assert (~small).sum() == 24 and (np.flatnonzero(~small) // 4 >= U.BIG_BLOCKS).any() and (np.flatnonzero(~small) // 4 < U.BIG_BLOCKS).any()
        assert lq[small].min() == 8 and lq[small].max() == 40 and lt[small].min() == 8 and lt[small].max() == 40
        exact = np.array([U.is_exact_prefix(a, b) for a, b in zip(qs, ts)])
        assert 0.1 * n < exact.sum() < 0.4 * n
        paths = Counter(U.classify([("", a, b, None, None) for a, b in zip(qs, ts)]))
        assert paths["quad3"] > 5000 and paths["quad4"] > 100 and paths["exact"] > 2000, paths
        assert paths["wave4"] >= (24 if wide else 0), paths
    a, b = U.big_batch(wide=False), U.big_batch(wide=True)
    assert sum(x != y for x, y in zip(a[0], b[0])) == 24 and np.array_equal(a[2], b[2])
