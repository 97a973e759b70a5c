"""The inputs of tests/seed_scan_util.py are what their labels say -- by the numpy model of the scan and the oracle alone, no
device -- and the model agrees with the oracle wherever both speak: on every clean stretch of every case the model's selected
interior positions are the oracle's interior seeds (position, strand bit, value), and the anchors that the model's candidates
make are the oracle's anchors before the occurrence cut, target position by target position.  tests/test_gpu_seed_scan.py then
compares the device with both.  No label is skipped: a case whose claim cannot be shown fails here."""

import math

import numpy as np
import pytest

from tests import seed_scan_util as U

CASES = ("a_phase_sweep", "b_unit_offsets", "b_near_palindromes", "c_neighbour_reach", "d_every_lane", "d_list_peak", "d_stage_full",
         "d_stage_flush", "d_walk_window", "d_nothing_passes", "d_final_walk_only", "d_periods", "e_rejects", "e_empty", "e_strands", "e_family", "e_survivors",
         "f_flank_lengths", "f_flank_shapes")  # fmt: skip


@pytest.fixture(scope="module")
def built(oracle):
    b = U.built(oracle)
    assert tuple(b["cases"]) == CASES
    return b


def tpos(anchors: np.ndarray) -> np.ndarray:
    """Target position of every anchor key (kp_spec.h: diag = tpos - qpos + KP_DIAG_BIAS)."""
    a = np.asarray(anchors, np.uint64)
    return ((a >> np.uint64(16)) & np.uint64(0x3FFFFFFF)).astype(np.int64) - 65536 + (a & np.uint64(0xFFFF)).astype(np.int64)


def accepted(model) -> np.ndarray:
    """The candidates that become anchors: the front ones in a clean stretch's interior, and the back ones."""
    return np.concatenate([np.setdiff1d(model.front, model.rejected_front()), model.back])


def anchors_at(odb, asm, lo: int, hi: int, cut=True) -> int:
    t = tpos(odb.anchors(asm.packed(), cut=cut))
    return int(((t >= lo) & (t < hi)).sum())


def test_constants_are_those_the_cases_were_derived_for():
    """Every size in seed_scan_util.py is computed from the sources' constants; the geometry the cases rely on holds for them."""
    c = U.C
    assert (U.OWN, U.LIST, U.STAGE, U.PROBES, U.WALK_ROOM, U.K, U.W) == (62, 1024, 320, 4, 512, 15, 10), c
    assert U.SPLIT == U.K + U.W + 48 == 73
    assert (c["KP_CONTIG_ALIGN"], c["KP_ASM_ALIGN"], c["KP_FILTER_LOG2"], c["KP_FILTER2_LOG2"], c["KP_ANCHOR_SUBS"]) == (32, 64, 24, 23, 64)
    # a list beyond DENSE_LIST and a stage beyond DENSE_STAGE cannot exist: eight positions add at most 8 x 62 entries to at most
    # DENSE_LIST - WALK_ROOM, a round at most 64 x PROBES candidates to at most DENSE_STAGE - 64 x PROBES
    assert U.LIST - U.WALK_ROOM + 8 * U.OWN == U.LIST - 16
    assert U.STAGE - U.ROUND + U.ROUND == U.STAGE and U.STAGE - U.ROUND == 64


def test_hash_and_values_restate_the_spec(oracle):
    """kp_hash30 is a bijection of 30-bit values (checked on a sample through the oracle's seeds of a sequence whose every
    15-mer is its own window: K + W - 1 bases have one window, whose minimum the oracle reports with its value)."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        seq = rng.integers(0, 4, U.K).astype(np.uint8)  # one 15-mer: mm_sketch's last minimum
        start, z, x = oracle.seeds(seq)
        _, _, mz, mx = U.kmer_values(seq)
        assert (start.tolist(), z.tolist(), x.tolist()) == ([0], mz.tolist(), mx.tolist())
    # no 15-mer equals its reverse complement: the middle base would be its own complement
    fwd, rev, _, _ = U.kmer_values(rng.integers(0, 4, 200_000).astype(np.uint8))
    assert (fwd != rev).all()


@pytest.mark.parametrize("name", CASES)
def test_model_equals_oracle_on_every_clean_stretch(oracle, built, name):
    """Interior: the window rule on the stream taken as one clean sequence gives the oracle's seeds, strand bits and values.
    Edges: the model takes the oracle's.  Anchors: what the accepted candidates make is what the oracle lists before the cut."""
    m = U.model_of(oracle, name)
    case, world = built["cases"][name], built["world"]
    n_interior = 0
    for i, st in enumerate(m.stretches):
        pos, z, x = m.interior_model(i)
        opos, oz, ox = m.interior_oracle[i]
        assert np.array_equal(pos, opos) and np.array_equal(z, oz) and np.array_equal(x, ox), f"{name}: stretch {st}"
        n_interior += len(pos)
    assert n_interior > 0 and len(m.back) > 0
    assert len(np.unique(m.front)) == len(m.front) and len(np.unique(m.back)) == len(m.back)
    # anchors before the cut, per assembly: one per posting of every accepted candidate's value
    allx = np.concatenate([s[2] for s in world.gene_seeds])
    vals, counts = np.unique(allx, return_counts=True)
    pos, _, x = U.unpack_cand(accepted(m))
    at = np.searchsorted(vals, x)
    hit = (at < len(vals)) & (vals[np.minimum(at, len(vals) - 1)] == x)
    rep = np.where(hit, counts[np.minimum(at, len(vals) - 1)], 0)
    for a, asm in enumerate(case.asms):
        mine = (pos >= m.base[a]) & (pos < m.base[a + 1])
        want = np.sort(tpos(world.odb.anchors(asm.packed(), cut=False)))
        got = np.sort(np.repeat(pos[mine] - m.base[a], rep[mine]))
        assert np.array_equal(got, want), f"{name}, {asm.id}: the model's candidates make {len(got)} anchors, the oracle has {len(want)}"


# ---- a ------------------------------------------------------------------------------------------------------------------------------
def test_phase_sweep_labels(oracle, built):
    case, world = built["cases"]["a_phase_sweep"], built["world"]
    P, part, probe = case.marks["P"], case.marks["part"], case.marks["probe"]
    pa = probe.packed()
    assert pa.padded_len == U.UNIT * P and math.gcd(P, U.OWN) == 1 and len(case.asms) == U.OWN
    assert len({(j * P) % U.OWN for j in range(U.OWN)}) == U.OWN  # every unit of the probe is owned once by every lane 1..62
    assert (P * U.OWN) % U.OWN == 0 and max(a.packed().padded_len for a in case.asms) <= 65536
    lens = dict(zip(part, pa.ctg_len.tolist()))
    assert (lens["len_1"], lens["len_14"], lens["len_15"], lens["len_16"]) == (1, 14, 15, 16)
    i = part["abutting"]
    assert lens["abutting"] % U.C["KP_CONTIG_ALIGN"] == 0 and pa.ctg_start[i] + pa.ctg_len[i] == pa.ctg_start[i + 1]
    assert pa.ctg_start[part["last"]] + lens["last"] == pa.padded_len
    runs = (np.asarray(pa.n_runs).reshape(-1, 2)[:, 1] - np.asarray(pa.n_runs).reshape(-1, 2)[:, 0]).tolist()
    assert sorted(runs) == [1, 40]
    t = tpos(world.odb.anchors(pa))  # after the cut
    for name, c in part.items():
        n = int(((t >= pa.ctg_start[c]) & (t < pa.ctg_start[c] + pa.ctg_len[c])).sum())
        assert (n == 0) if lens[name] < U.K else n > 0, f"{name}: {n} anchors"  # (a contig shorter than k has no 15-mer)
    # the periodic stretch and each of the three clean stretches around the N runs hold anchors of their own
    s = pa.ctg_start[part["n_runs"]]
    for lo, hi in ((0, 150), (151, 260), (300, 400)):
        assert ((t >= s + lo) & (t < s + hi)).any()
    s = pa.ctg_start[part["periodic"]] + 90
    assert ((t >= s) & (t < s + U.TIE_RUN + 3 - U.K)).any()


# ---- b ------------------------------------------------------------------------------------------------------------------------------
def test_unit_offset_labels(oracle, built):
    case, world = built["cases"]["b_unit_offsets"], built["world"]
    m = U.model_of(oracle, "b_unit_offsets")
    front = m.front_set()
    t = set(tpos(world.odb.anchors(case.asms[0].packed())).tolist())
    assert [p % U.UNIT for p in case.marks["kmer_pos"]] == list(range(U.UNIT))  # all 16 word offsets of each of the four words
    for p in case.marks["kmer_pos"]:
        assert int(m.x[p]) == case.marks["x"] and (p, int(m.z[p]), case.marks["x"]) in front and p in t
        st = m.stretch_of(p)
        assert U.is_interior(p, st.S, st.E)


def test_near_palindrome_labels(oracle, built):
    """Every near-palindrome between every pair of flanking bases, in contigs and in a gene; each is a seed there, on both
    strands (the reverse-complemented gene), and its strand bit is decided by the middle base alone."""
    case, world = built["cases"]["b_near_palindromes"], built["world"]
    m = U.model_of(oracle, "b_near_palindromes")
    pa = case.asms[0].packed()
    stream = U.words_to_codes(np.asarray(pa.words, np.uint32), pa.padded_len)
    t = set(tpos(world.odb.anchors(pa)).tolist())
    accepted_pos = set(U.unpack_cand(accepted(m))[0].tolist())
    for pal in U.near_palindromes():
        pc = U.codes_of(pal)
        fwd, rev, z, _ = U.kmer_values(pc)
        assert int(fwd[0] ^ rev[0]) == 3 << (2 * 7)  # the reverse complement differs in the middle base only: bits 14-15
        seen = set()
        for i in range(len(stream) - U.K - 1):
            if i > 0 and np.array_equal(stream[i : i + U.K], pc):
                seen.add((int(stream[i - 1]), int(stream[i + U.K])))
                assert m.sel[i] and int(m.z[i]) == int(z[0]) and i in accepted_pos and i in t, i
        assert {(a, b) for a in range(4) for b in range(4) if a == b} <= seen and len(seen) == 16, seen
    assert len(world.genes[world.g_extra]) <= 65535


# ---- c ------------------------------------------------------------------------------------------------------------------------------
def test_neighbour_reach_labels(oracle, built):
    case, world = built["cases"]["c_neighbour_reach"], built["world"]
    m = U.model_of(oracle, "c_neighbour_reach")
    front = m.front_set()
    assert all(a.packed().padded_len == 2 * U.OWN * U.UNIT for a in case.asms)  # batch units and assembly units agree mod 62
    kept = [set((tpos(world.odb.anchors(a.packed())) + m.base[i]).tolist()) for i, a in enumerate(case.asms)]
    kept = set().union(*kept)
    seen = set()
    for p, b, o in case.marks["minima"]:
        unit = p // U.UNIT
        lane = unit % U.OWN + 1
        assert p % U.UNIT == o and unit % (2 * U.OWN) == (b if o < 32 else b - 1)
        if b == U.OWN:
            assert lane == (1 if o < 32 else U.OWN)  # behind / before the boundary between two iterations
        assert m.sel[p] and (m.x[p - U.W + 1 : p + U.W] == m.x[p]).sum() == 1  # a strict minimum
        assert (p, int(m.z[p]), int(m.x[p])) in front and p in kept
        seen.add((b, o))
    assert seen == {(b, o) for b in U.BOUNDARIES for o in U.REACH_OFFSETS}
    for p, q, b, d in case.marks["ties"]:
        assert q - p == d and p // U.UNIT % (2 * U.OWN) == b - 1 and q // U.UNIT % (2 * U.OWN) == b  # the pair straddles the boundary
        assert m.x[p] == m.x[q] and m.sel[p] and m.sel[q]
        assert {(p, int(m.z[p]), int(m.x[p])), (q, int(m.z[q]), int(m.x[q]))} <= front and {p, q} <= kept
    assert {(b, d) for _, _, b, d in case.marks["ties"]} == {(b, d) for b in U.BOUNDARIES for d in (9, 10)}
    # the ninth neighbour value: decisions that hang on the value nine positions away, both ways, in the index either way
    rejected = set(U.unpack_cand(m.rejected_front())[0].tolist())
    for p, b, kind in case.marks["far"]:
        x = m.x.astype(np.int64)
        assert p % U.UNIT == (0 if kind.startswith("below") else U.UNIT - 1) and (p // U.UNIT + (kind.startswith("above"))) % (2 * U.OWN) == b
        assert world.indexed([m.x[p]]).all() and m.pass1[p] and m.pass2[p]  # a wrong decision would show in the candidate list
        far, near, other = (x[p - 9], x[p - 8 : p], x[p + 1]) if kind.startswith("below") else (x[p + 9], x[p + 1 : p + 9], x[p - 1])
        assert other < x[p] < near.min()
        if kind.endswith("only_window"):
            assert far > x[p] and m.sel[p] and (p, int(m.z[p]), int(m.x[p])) in front and p not in rejected and p in kept
        else:
            assert far < x[p] and not m.sel[p] and p not in set(U.unpack_cand(m.front)[0].tolist())
    assert {(b, k) for _, b, k in case.marks["far"]} == {(b, k) for b in U.BOUNDARIES for k in U.FAR_KINDS}


# ---- d ------------------------------------------------------------------------------------------------------------------------------
def _poly_a_cut(world, case, m):
    """The poly-A anchors of a tie-dense case exist before the cut and are gone after it."""
    pa = case.asms[0].packed()
    xa = int(U.kmer_values(np.zeros(U.K, np.uint8))[3][0])
    pos = np.flatnonzero((m.x == xa) & m.sel)
    before, after = set(tpos(world.odb.anchors(pa, cut=False)).tolist()), set(tpos(world.odb.anchors(pa)).tolist())
    inner = [p for p in pos.tolist() if (s := m.stretch_of(p)) and s.S <= p and p + U.K <= s.E]
    assert len(inner) > U.OWN and set(inner) <= before and not (set(inner) & after)


def test_list_and_stage_labels(oracle, built):
    """The occupancies are the model's; the middle iteration (1) of every case is the one its label is about, between two
    iterations of gene material that list and stage candidates of their own."""
    world = built["world"]
    its = {n: U.model_of(oracle, n).iterations for n in CASES if n.startswith("d_")}
    for n, it in its.items():
        assert len(it) == 3 and it[0].n_hits > 0 and it[2].n_hits > 0, n
        assert built["cases"][n].asms[0].packed().padded_len == 3 * U.OWN * U.UNIT
    marks = {n: built["cases"][n].marks for n in its}
    # every lane at once: all 62 x 64 positions selected and passing, 992 entries before every walk, full rounds
    it = its["d_every_lane"][1]
    m = U.model_of(oracle, "d_every_lane")
    mid = slice(U.OWN * U.UNIT, 2 * U.OWN * U.UNIT)
    assert (m.sel[mid] & m.pass1[mid] & m.pass2[mid]).all()
    assert it.walks == marks["d_every_lane"]["walks"] == [992] * 4 and [r[0] for r in it.rounds] == marks["d_every_lane"]["round_hits"]
    assert all(r[2] for r in it.rounds) and it.stage_peak == U.ROUND
    # the highest list occupancy the model could construct (profiles/seed_scan.md records it)
    peak = max(its["d_list_peak"][1].walks)
    assert peak == marks["d_list_peak"]["peak"] and 992 <= peak <= U.LIST - 16
    assert peak == 1008
    # the stage filled to its last entry: a round leaves DENSE_STAGE - 64 PROBES without a flush, the next one stages 64 PROBES
    it = its["d_stage_full"][1]
    assert it.rounds[:2] == marks["d_stage_full"]["first_rounds"] == [(64, 64, False), (256, 320, True)] and it.stage_peak == U.STAGE
    # one more: the flush happens
    it = its["d_stage_flush"][1]
    assert it.rounds[:2] == marks["d_stage_flush"]["first_rounds"] == [(65, 65, True), (256, 256, True)] and it.stage_peak < U.STAGE
    # walk triggers
    it = its["d_nothing_passes"][1]
    assert it.n_hits == 0 and it.n_listed == U.OWN * U.UNIT and it.walks == [992] * 4 and not any(r[2] for r in it.rounds)
    m = U.model_of(oracle, "d_nothing_passes")
    assert not (m.sel[mid] & m.pass1[mid]).any()
    it = its["d_final_walk_only"][1]
    assert len(it.walks) == 1 and 0 < it.walks[0] <= U.LIST - U.WALK_ROOM and it.n_hits == it.n_listed
    # both tie-dense kinds side by side: an indexed and a foreign value
    it = its["d_periods"][1]
    assert 0 < it.n_hits < it.n_listed
    # which of these the cut leaves to the candidates alone
    for n in its:
        if built["cases"][n].cut_removes and n != "d_final_walk_only" and n != "d_periods":
            _poly_a_cut(world, built["cases"][n], U.model_of(oracle, n))
    # the periods: one value on every 8th position of 62 units asks for the assembly's own mid_occ, which keeps its anchors;
    # next to homopolymers the cut removes them
    for n in ("d_final_walk_only", "d_periods"):
        pa = built["cases"][n].asms[0].packed()
        t_before, t_after = tpos(world.odb.anchors(pa, cut=False)), tpos(world.odb.anchors(pa))
        inside = lambda t: int(((t >= U.OWN * U.UNIT + U.UNIT) & (t < 2 * U.OWN * U.UNIT - U.UNIT)).sum())  # noqa: E731
        assert inside(t_before) > 100 and inside(t_after) == (0 if built["cases"][n].cut_removes else inside(t_before)), (n, inside(t_before), inside(t_after))


def test_thresholds_moved_by_a_little_overrun_list_and_stage(oracle, built):
    """Two planted errors that must not run on a device, argued from the model's occupancies: a walk trigger at DENSE_LIST -
    WALK_ROOM / 2 lets `d_walk_window` (a walk at an occupancy the product reaches after sixteen positions) list eight more
    positions of all 62 lanes beyond DENSE_LIST; a flush threshold one higher lets `d_stage_flush` stage 64 * PROBES
    candidates on top of DENSE_STAGE - 64 * PROBES + 1."""
    m = U.model_of(oracle, "d_walk_window")
    first = m.iterations[1].walks[0]
    marks = built["cases"]["d_walk_window"].marks
    assert marks["lo"] < first <= marks["hi"] and first + 8 * U.OWN > U.LIST
    with pytest.raises(OverflowError, match="entries listed"):
        U.bookkeeping(m.sel, m.pass1, walk_room=U.WALK_ROOM // 2)
    m = U.model_of(oracle, "d_stage_flush")
    with pytest.raises(OverflowError, match=f"{U.STAGE + 1} candidates staged"):
        U.bookkeeping(m.sel, m.pass1, flush_above=U.STAGE - U.ROUND + 1)
    for n in CASES:  # ... and the product's own thresholds overrun nothing, anywhere
        m = U.model_of(oracle, n)
        U.bookkeeping(m.sel, m.pass1)


def test_no_iteration_of_any_case_overruns_list_or_stage(oracle, built):
    """bookkeeping() asserts the bounds while it runs; here: the largest occupancies over every iteration of every case."""
    walks = [w for n in CASES for it in U.model_of(oracle, n).iterations for w in it.walks]
    peaks = [it.stage_peak for n in CASES for it in U.model_of(oracle, n).iterations]
    assert max(walks) == U.LIST - 16 and max(peaks) == U.STAGE


# ---- e ------------------------------------------------------------------------------------------------------------------------------
def test_expansion_labels(oracle, built):
    world = built["world"]
    case = built["cases"]["e_rejects"]
    m = U.model_of(oracle, "e_rejects")
    rej_pos = set(U.unpack_cand(m.rejected_front())[0].tolist())
    front_pos = set(U.unpack_cand(m.front)[0].tolist())
    xa = int(U.kmer_values(np.zeros(U.K, np.uint8))[3][0])
    assert world.indexed([xa]).all()  # the index holds the poly-A value
    for key in ("padding", "tail_padding", "n_run"):
        lo, hi = case.marks[key]
        inside = [p for p in range(lo, hi - U.K + 1) if m.x[p] == xa]
        assert inside and set(inside) <= front_pos and set(inside) <= rej_pos, key  # poly-A 15-mers of code-0 bases: listed, to be rejected
    _, _, s = U.split_kmer(world)
    g_x = {int(v) for st, v in zip(world.gene_seeds[10][0].tolist(), world.gene_seeds[10][2].tolist()) if st == s}
    for key in ("split_at", "split_asm_at"):
        p = case.marks[key]
        assert {int(m.x[p])} == g_x and p in front_pos and p in rej_pos, key  # whole in the stream, in the index, in no contig
        st = m.stretch_of(p)
        assert st is not None and st.E == p + 7  # seven bases at the end of one contig ...
        nxt = m.stretch_of(p + 7)
        assert nxt is not None and nxt.S == p + 7 and (nxt.asm != st.asm) == (key == "split_asm_at")  # ... eight at the start of the next
    assert anchors_at(world.odb, case.asms[0], case.marks["split_at"], case.marks["split_at"] + 1, cut=False) == 0
    # empty assemblies pack to nothing
    case = built["cases"]["e_empty"]
    lens = [a.packed().padded_len for a in case.asms]
    assert lens[1] == lens[3] == 0 and lens[0] > 0 and lens[2] > 0 and [len(a.packed().ctg_len) for a in case.asms][1::2] == [0, 0]
    # strands: both strand bits in numbers, on the same values
    m = U.model_of(oracle, "e_strands")
    pos, z, x = U.unpack_cand(accepted(m))
    assert abs(int((z == 0).sum()) - int((z == 1).sum())) <= len(z) // 4 and set(x[z == 0].tolist()) & set(x[z == 1].tolist())
    assert len(tpos(world.odb.anchors(built["cases"]["e_strands"].asms[0].packed()))) >= len(z) // 2
    # a candidate with far more postings than its neighbours
    m = U.model_of(oracle, "e_family")
    allx = np.concatenate([s[2] for s in world.gene_seeds])
    _, _, x = U.unpack_cand(accepted(m))
    n_post = np.array([(allx == v).sum() for v in x.tolist()])
    assert (n_post >= U.FAMILY).sum() >= 20 and (n_post == 1).sum() >= 20
    _, per_pos = np.unique(tpos(world.odb.anchors(built["cases"]["e_family"].asms[0].packed())), return_counts=True)
    assert (per_pos >= U.FAMILY).sum() >= 20  # ... and the family's anchors stay after the cut
    # survivors: n_front is no multiple of 64 (a wave holds front and back candidates); one contig where most candidates are
    # rejected -- 64 consecutive ones hold a single survivor -- and one where none is
    case = built["cases"]["e_survivors"]
    m = U.model_of(oracle, "e_survivors")
    assert len(m.front) % 64 != 0 and len(m.back) > 0
    pa = case.asms[0].packed()
    rej = np.isin(m.front, m.rejected_front())  # (the front is sorted: by position)
    pos = U.unpack_cand(m.front)[0]
    second = pos >= pa.ctg_start[1] + U.W
    assert not rej[second & (pos + U.K + U.W <= pa.ctg_start[1] + pa.ctg_len[1])].any() and second.sum() > 640
    surv = np.convolve((~rej[~second]).astype(int), np.ones(64, int), "valid")
    assert (surv == 1).any() and (np.convolve((~rej).astype(int), np.ones(64, int), "valid") == 64).any()


# ---- f ------------------------------------------------------------------------------------------------------------------------------
def test_flank_grid_labels(oracle, built):
    world = built["world"]
    case = built["cases"]["f_flank_lengths"]
    m = U.model_of(oracle, "f_flank_lengths")
    got = {(s.E - s.S, s.left_n, s.right_n, s.S % U.UNIT) for s in m.stretches}
    need = {(n, left, right, o) for n in U.FLANK_LENGTHS for left in (False, True) for right in (False, True) for o in (0, 32)}
    assert need <= got and {15, 24, 25, 34, 35, 44, 45, U.SPLIT, U.SPLIT + 1} <= set(U.FLANK_LENGTHS)
    assert max(a.packed().padded_len for a in case.asms) <= 65536
    # every stretch of the grid that can hold a 15-mer has a seed, all of them on the edge kernel's side up to K + 2 W - 1 bases
    by_len: dict = {}
    kept = set().union(*[set((tpos(world.odb.anchors(a.packed())) + m.base[i]).tolist()) for i, a in enumerate(case.asms)])
    n_kept = 0
    for i, s in enumerate(m.stretches):
        n = s.E - s.S
        if (n, s.left_n, s.right_n, s.S % U.UNIT) not in need:
            continue
        edge, inner = m.edge_oracle[i][0], m.interior_oracle[i][0]
        by_len.setdefault(n, []).append((len(edge), len(inner), s.right_n))
        n_kept += len(set(edge.tolist()) & kept)
    for n, rows in by_len.items():
        if n < U.K:
            assert all(r[:2] == (0, 0) for r in rows), n
            continue
        # a stretch that ends with its contig reports its last minimum; before an N run that minimum is dropped
        assert all(e > 0 for e, _, right_n in rows if not right_n), (n, rows)
        assert all(i == 0 for _, i, _ in rows) or n >= U.K + 2 * U.W, (n, rows)
    # (mm_sketch reports nothing before its first full window: a stretch shorter than K + W - 1 that ends in an N run has no seed)
    assert all(e == 0 for n, rows in by_len.items() for e, _, right_n in rows if right_n and n < U.K + U.W - 1)
    assert any(e > 0 for n, rows in by_len.items() for e, _, right_n in rows if right_n and n < U.K + 2 * U.W)
    assert any(i > 0 for _, i, _ in by_len[U.K + 2 * U.W]) or any(i > 0 for _, i, _ in by_len[U.K + 2 * U.W + 1])
    assert n_kept > 2000  # the edge seeds are anchors, and stay after the cut


def test_flank_shape_labels(oracle, built):
    case = built["cases"]["f_flank_shapes"]
    m = U.model_of(oracle, "f_flank_shapes")
    pa = case.asms[0].packed()
    names = case.marks["names"]
    cc = U.contig_codes(pa)
    stretches = {n: U.clean_stretches(cc[i]) for i, n in enumerate(names)}
    assert stretches["n_at_first_base"][0][:3] == (5, 300, True) and stretches["n_at_last_base"][-1][:2] == (0, 293) and stretches["n_at_last_base"][-1][3]
    assert [s[:2] for s in stretches["n_runs_one_apart"]] == [(0, 120), (125, 126), (140, 300)]
    for run in range(1, U.W):
        # the sketch of the stretch alone ends by reporting its tracked minimum; in the contig it keeps stepping through the
        # short run and drops that minimum -- unless the contig ends inside the run, where it is a seed
        i, j = names.index(f"short_run_{run}"), names.index(f"short_run_{run}_to_end")
        alone = set(oracle.seeds(cc[i][:150])[0].tolist())
        inside = {s for s in oracle.seeds(cc[i])[0].tolist() if s < 150}
        assert len(alone - inside) == 1 and inside <= alone, run
        assert (cc[j][150:] == 4).all() and len(cc[j]) == 150 + run
        at_end = set(oracle.seeds(cc[j])[0].tolist())
        assert inside <= at_end and len(at_end - inside) == 1, run  # (the minimum tracked when the contig ends: not always the stretch's last)
    # ties inside either flank and across the hand-over positions: equal values on both sides of S + KP_W and of E - KP_K - KP_W
    n_ties = 0
    for i, n in enumerate(names):
        if not n.startswith("ties_"):
            continue
        S, E = pa.ctg_start[i], pa.ctg_start[i] + pa.ctg_len[i]
        start, _, x = oracle.seeds(cc[i])
        start = start + S
        inner = U.is_interior(start, S, E)
        shared = set(x[inner].tolist()) & set(x[~inner].tolist())
        if n.startswith("ties_handover"):
            assert shared, n  # one value decided by both kernels
        n_ties += len(shared)
        vals, cnt = np.unique(x[~inner], return_counts=True)
        assert (cnt > 1).any(), n  # equal seeds inside a flank
    assert n_ties >= 8
