"""cs strings, the parts that need no GPU (include/kp_spec.h, CS): kp_cs.h's per-hit function -- the one the device kernels give a
lane per hit -- built with g++ (tests/native_harness/cs_harness.cpp) and compared, count and bytes, with the Python yardstick
of tests/cs_util.py on hand-built cases that reach every edge of its word-wise comparison and on seeded random ones; the
spec's invariants on every yardstick string; the buffer policy of the bytes (kp_caps.h); kp_format_paf_tags against a Python
formatter; Cigars.from_cs; the command line's --cs and --eqx."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.core.alignment import Cigars
from tests import cigar_util as U
from tests import cs_util as S

M, I, D = S.M, S.I, S.D


def _same(ops, gene, asm, q, t, label):
    """The harness's count and bytes are the yardstick's; the yardstick's string keeps the spec's invariants.  Returns it."""
    ops = S.ops_of(*ops) if not isinstance(ops, np.ndarray) else ops
    want = S.cs_from_ops(ops, gene, asm, q, t)
    S.check_cs(want, ops, label)
    count, got, guard = S.harness_cs(ops, gene, asm, q, t)
    assert count == len(want), f"{label}: {count} bytes counted, the yardstick's string has {len(want)}"
    assert got == want, f"{label}: {got[:120]!r} vs the yardstick's {want[:120]!r}"
    assert guard, f"{label}: bytes written beyond the buffer"
    return want


@pytest.fixture()
def rng():
    return np.random.default_rng(20240)


@pytest.mark.parametrize("n", [9, 10, 99, 100, 999, 1000, 9999, 10000, 12000])
def test_identical_runs(rng, n):
    ops = [(M, n)]
    gene, asm = S.build_pair(rng, ops, q0=3, t0=5)
    assert _same(ops, gene, asm, 3, 5, f"run of {n}") == f":{n}".encode()
    # ... and the same run broken by one substitution next to its end: both numbers are written
    gene, asm = S.build_pair(rng, ops, q0=3, t0=5, sub_rows=(3 + n - 2,))
    assert _same(ops, gene, asm, 3, 5, f"run of {n - 2}").startswith(f":{n - 2}*".encode())


def test_substitution_in_the_first_and_last_column_of_a_chunk(rng):
    """Every start row modulo 8 against every target start modulo 16: the first column of the (partial) first chunk, the first and
    last column of whole chunks, the last column of the (partial) last one."""
    n = 45
    for q0 in range(8):
        for t0 in range(16):
            first_whole = (q0 // 8 + 1) * 8
            for rows in [(q0,), (first_whole,), (first_whole + 7,), (first_whole + 15,), (q0 + n - 1,), (q0, first_whole, first_whole + 7, first_whole + 8, q0 + n - 1)]:
                gene, asm = S.build_pair(rng, [(M, n)], q0=q0, t0=t0, sub_rows=rows)
                cs = _same([(M, n)], gene, asm, q0, t0, f"q0 {q0}, t0 {t0}, rows {rows}")
                assert cs.count(b"*") == len(rows)


def test_adjacent_substitutions_across_a_chunk_edge(rng):
    for q0 in (0, 3):
        for rows in [(15, 16), (15, 16, 17), (14, 15, 16), (7, 8), (22, 23, 24)]:
            for t0 in (0, 9, 15):
                gene, asm = S.build_pair(rng, [(M, 60)], q0=q0, t0=t0, sub_rows=rows)
                cs = _same([(M, 60)], gene, asm, q0, t0, f"rows {rows}")
                assert cs.count(b"*") == len(rows) and S.TOKEN.findall(cs)[1][:1] == b"*"
                assert [o & 15 for o in S.eqx_from_cs(cs)] == [S.EQ, S.X, S.EQ] and S.eqx_from_cs(cs)[1] >> 4 == len(rows)


@pytest.mark.parametrize("length", [1, 3, 20])
def test_n_runs_at_every_offset_of_a_target_word(rng, length):
    for off in range(16):
        for q0 in (0, 5):
            gene, asm = S.build_pair(rng, [(M, 90)], q0=q0, t0=7, n_runs=((32 + off, length),))
            cs = _same([(M, 90)], gene, asm, q0, 7, f"N run of {length} at word offset {off}")
            assert cs.count(b"*n") == length
    # two runs in one chunk, and a run that begins before the hit
    gene, asm = S.build_pair(rng, [(M, 90)], q0=2, t0=7, n_runs=((3, 6), (40, 1), (42, 2), (95, 8)))
    assert _same([(M, 90)], gene, asm, 2, 7, "several runs").count(b"*n") == 2 + 1 + 2 + 2


def test_gene_n_in_the_first_and_last_nibble_of_a_word(rng):
    gene, asm = S.build_pair(rng, [(M, 60)], q0=2, t0=11, gene_n=(16, 23, 31, 32))
    cs = _same([(M, 60)], gene, asm, 2, 11, "gene n")
    assert [t[2:3] for t in S.TOKEN.findall(cs) if t[:1] == b"*"] == [b"n"] * 4
    # n against n: a substituted column, not an identical one (the spec's one deviation from minimap2)
    gene, asm = S.build_pair(rng, [(M, 60)], q0=2, t0=11, gene_n=(20,), n_runs=((11 + 18, 1),))
    assert b"*nn" in _same([(M, 60)], gene, asm, 2, 11, "n against n")


@pytest.mark.parametrize("k", [1, 20, 500])
def test_gaps_with_an_n_inside(rng, k):
    ops = [(M, 30), (I, k), (M, 33), (D, k), (M, 30)]
    gene, asm = S.build_pair(rng, ops, q0=4, t0=13, i_n=True, d_n=True)
    toks = S.TOKEN.findall(_same(ops, gene, asm, 4, 13, f"gaps of {k}"))
    assert [t[:1] for t in toks] == [b":", b"+", b":", b"-", b":"] and len(toks[1]) == len(toks[3]) == k + 1
    assert toks[1].count(b"n") == 1 and toks[3].count(b"n") == 1


def test_reverse_strand(rng):
    """The gene as aligned is the reverse complement, starting at len - q_end (cigar_util.gene_as_aligned)."""
    codes = rng.integers(0, 4, size=300).astype(np.uint8)
    off = np.array([0, 300], np.int32)
    rc = U.gene_as_aligned(codes, off, 1)
    asm = np.concatenate([rng.integers(0, 4, size=21), rc[40:260], rng.integers(0, 4, size=30)]).astype(np.uint8)
    asm[21 + 100] = (asm[21 + 100] + 1) % 4
    hit = dict(gene=0, strand=-1, q_start=40, q_end=260, contig=0, t_start=21)  # (forward coordinates: 300 - 260 = 40 rows skipped)

    class Pa:
        ctg_start = [0]

    want = S.hit_cs_yardstick(hit, S.ops_of((M, 220)), codes, off, Pa, asm)
    assert want.startswith(b":100*") and want.endswith(b":119")
    assert _same([(M, 220)], rc, asm, 40, 21, "strand -1") == want


def test_m_ops_shorter_than_a_chunk(rng):
    ops = [(M, 3), (I, 1), (M, 2), (D, 1), (M, 5), (I, 2), (M, 1), (D, 3), (M, 7), (I, 1), (M, 4)]
    for q0 in range(8):
        gene, asm = S.build_pair(rng, ops, q0=q0, t0=14, sub_rows=(q0 + 4, q0 + 12))
        _same(ops, gene, asm, q0, 14, f"short ops from row {q0}")


def test_a_buffer_one_byte_too_small(rng):
    for ops, kw in [([(M, 1000)], {}), ([(M, 40), (I, 3), (M, 50)], dict(sub_rows=(10, 89))), ([(M, 30), (D, 20), (M, 9)], dict(sub_rows=(38,)))]:
        gene, asm = S.build_pair(rng, ops, q0=1, t0=3, **kw)
        o = S.ops_of(*ops)
        want = S.cs_from_ops(o, gene, asm, 1, 3)
        for cap in (len(want) - 1, 1, 0):
            count, got, guard = S.harness_cs(o, gene, asm, 1, 3, cap=cap)
            assert count == len(want) and got == want[:cap] and guard, f"cap {cap}: {count} bytes counted, {got!r} written"


def _random_case(rng):
    cols = int(rng.integers(40, 3001))
    ops, left, kind = [], cols, M
    while left > 0:
        if kind == M:
            n = min(left, int(rng.integers(1, 12)) if rng.random() < 0.2 else int(rng.integers(12, 900)))
        else:
            n = min(left, int(rng.integers(1, 4)) if rng.random() < 0.7 else int(rng.integers(4, 120)))
        ops.append((kind, n))
        left -= n
        kind = int(rng.choice([I, D])) if kind == M else M
    if ops[-1][0] != M:
        ops.append((M, int(rng.integers(1, 30))))
    q0, t0 = int(rng.integers(0, 40)), int(rng.integers(0, 70))
    gene, asm = S.build_pair(rng, ops, q0=q0, t0=t0, i_n=rng.random() < 0.1, d_n=rng.random() < 0.1)
    rate = rng.random() * 0.15
    rows = q0 + np.flatnonzero(rng.random(len(gene) - q0 - 5) < rate)
    gene[rows] = (gene[rows] + rng.integers(1, 4, size=len(rows))) % 4  # (rows of I ops change letters only)
    if rng.random() < 0.3:
        gene[q0 + rng.integers(0, len(gene) - q0 - 5, size=int(rng.integers(1, 4)))] = 4
    for _ in range(int(rng.integers(0, 3)) if rng.random() < 0.4 else 0):
        s = int(rng.integers(0, len(asm) - 1))
        asm[s : s + int(rng.integers(1, 40))] = 4
    return S.ops_of(*ops), gene, asm, q0, t0


def test_random_cases():
    rng = np.random.default_rng(777)
    n_sub = n_gap = 0
    for case in range(2000):
        ops, gene, asm, q0, t0 = _random_case(rng)
        cs = _same(ops, gene, asm, q0, t0, f"random case {case}")
        n_sub += cs.count(b"*")
        n_gap += cs.count(b"+") + cs.count(b"-")
    assert n_sub > 100000 and n_gap > 2000


# ---- buffer policy ------------------------------------------------------------------------------------------------------------------
def test_cs_buffer_policy():
    lib = S.harness()
    first = (C.c_int32 * 1)()
    lib.kpy_cs_layout(first)
    assert first[0] == 64  # the first guess (kp_caps.h says why)
    state = (C.c_uint32 * 2)(64, 0)
    assert lib.kpy_cs_size(state, C.c_uint64(1000)) == 64000 and state[1] == 64
    assert lib.kpy_cs_size(state, C.c_uint64(0)) == 64  # an empty table still gets a buffer
    # a pass whose bytes exceed the buffer grows it and asks for the bytes to be written again (0), nothing else
    cap = C.c_uint64(64000)
    assert lib.kpy_cs_after(state, C.byref(cap), C.c_uint64(1000), C.c_uint64(90000)) == 0
    assert cap.value == 90000 + 90000 // 4 and state[1] == 113  # ceil(112500 / 1000)
    assert lib.kpy_cs_after(state, C.byref(cap), C.c_uint64(1000), C.c_uint64(90000)) == 1 and cap.value == 112500
    assert lib.kpy_cs_size(state, C.c_uint64(500)) == 56500  # later passes start from what was learnt
    # the learnt size never shrinks
    cap = C.c_uint64(56500)
    assert lib.kpy_cs_after(state, C.byref(cap), C.c_uint64(500), C.c_uint64(600)) == 1 and state[1] == 113 and cap.value == 56500
    # a pass that came close makes room for the next one
    cap = C.c_uint64(56500)
    assert lib.kpy_cs_after(state, C.byref(cap), C.c_uint64(500), C.c_uint64(56000)) == 1 and state[1] == 140  # ceil(70000 / 500)
    # setting the option resets what was learnt, and only that
    other = C.c_uint32(777)
    assert lib.kpy_cs_set_option(state, C.byref(other), b"cs_bytes_per_hit", C.c_int64(1)) == 1
    assert (state[0], state[1], other.value) == (1, 0, 777)
    assert lib.kpy_cs_size(state, C.c_uint64(1000)) == 1000
    assert lib.kpy_cs_set_option(state, C.byref(other), b"cigar_ops_per_hit", C.c_int64(5)) == 1 and (state[0], state[1], other.value) == (1, 1, 0)
    assert lib.kpy_cs_set_option(state, C.byref(other), b"cs", C.c_int64(1)) == 0  # (not a buffer size: kp_ctx_set_option's own)


# ---- kp_format_paf_tags ---------------------------------------------------------------------------------------------------------------
def _tagged_table():
    """The table of tests/test_cigar_cpu.py with a cs string per hit whose column totals are its ops'."""
    from tests.test_cigar_cpu import _paf_table

    table = _paf_table()
    cs = [b":599*ag+c:300-gt:299", b":1234-" + b"acgtn" * 300 + b":64000", b":400*ca*tg*nn:492", b":300"]
    cs_off = np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)
    return table, cs, cs_off


def _paf_tags_python(table, cs, cs_tag, eqx) -> bytes:
    from tests.test_cigar_cpu import _paf_python

    lines = _paf_python(*table).split(b"\n")[:-1]
    out = []
    for line, c in zip(lines, cs):
        if eqx:
            head, _ = line.rsplit(b"\tcg:Z:", 1)
            line = head + b"\tcg:Z:" + "".join(f"{o >> 4}{'MIDNSHP=X'[o & 15]}" for o in S.eqx_from_cs(c)).encode()
        out.append(line + (b"\tcs:Z:" + c if cs_tag else b"") + b"\n")
    return b"".join(out)


def test_format_paf_tags_matches_python_formatter():
    table, cs, cs_off = _tagged_table()
    blob = b"".join(cs)
    for c, o in zip(cs, [table[7][table[8][i] : table[8][i + 1]] for i in range(4)]):
        S.check_cs(c, o, "table")
    assert _native.format_paf_tags(*table, blob, cs_off, 0) == _native.format_paf(*table)  # flags 0: kp_format_paf's bytes
    for cs_tag, eqx in [(True, False), (False, True), (True, True)]:
        got = _native.format_paf_tags(*table, blob, cs_off, (_native.PAF_CS if cs_tag else 0) | (_native.PAF_EQX if eqx else 0))
        assert got == _paf_tags_python(table, cs, cs_tag, eqx), f"cs {cs_tag}, eqx {eqx}"
    both = _native.format_paf_tags(*table, blob, cs_off, 3).decode().splitlines()
    assert both[0].endswith("cg:Z:599=1X1I300=2D299=\tcs:Z::599*ag+c:300-gt:299") and "cg:Z:400=3X492=" in both[2]


@pytest.mark.parametrize("bad", [b":0:300", b":100:200", b":0300", b":299", b":301", b":299*ax", b":299*a", b":300+", b":300-a", b":300+a", b"=300",
                                 b":150 :150", b"", b":300*", b":99999999999"])  # fmt: skip
def test_format_paf_tags_rejects_bad_cs(bad):
    table, cs, _ = _tagged_table()
    cs = [*cs[:3], bad]  # the last hit's ops are 300M
    cs_off = np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int64)
    for flags in (1, 2, 3):
        with pytest.raises(ValueError, match=r"\(-1\)"):  # KP_EINVAL
            _native.format_paf_tags(*table, b"".join(cs), cs_off, flags)
    assert _native.format_paf_tags(*table, b"".join(cs), cs_off, 0) == _native.format_paf(*table)  # flags 0 does not read them


# ---- Cigars.from_cs ---------------------------------------------------------------------------------------------------------------------
def test_cigars_from_cs_round_trip():
    rng = np.random.default_rng(31)
    cases = [_random_case(rng) for _ in range(60)]
    strings = [S.cs_from_ops(ops, gene, asm, q0, t0) for ops, gene, asm, q0, t0 in cases]
    strings.insert(7, b"")  # a row without a string
    all_ops = [c[0] for c in cases]
    all_ops.insert(7, np.zeros(0, np.uint32))
    off = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
    blob = np.frombuffer(b"".join(strings), np.uint8)
    eqx = Cigars.from_cs(blob, off)
    assert len(eqx) == len(strings)
    for i, (s, ops) in enumerate(zip(strings, all_ops)):
        assert eqx[i].tolist() == S.eqx_from_cs(s), f"row {i}"
        collapsed = []  # = and X back into M
        for o in eqx[i].tolist():
            k, n = (M if o & 15 in (S.EQ, S.X) else o & 15), o >> 4
            if collapsed and collapsed[-1][0] == k:
                collapsed[-1][1] += n
            else:
                collapsed.append([k, n])
        assert [(n << 4) | k for k, n in collapsed] == ops.tolist(), f"row {i}"
    part = Cigars.from_cs(blob, off[5:12])  # a slice of the offsets, as the rows of one assembly are
    assert [part[i].tolist() for i in range(6)] == [eqx[i].tolist() for i in range(5, 11)]
    assert Cigars.from_cs(b":5*ag*ca:10+acg:3-t:1", [0, 22]).strings() == ["5=2X10=3I3=1D1="]
    assert len(Cigars.from_cs(b"", [0])) == 0


# ---- command line -------------------------------------------------------------------------------------------------------------------------
def test_cs_and_eqx_require_paf(capsys):
    from kaptive_amd.cli import build_parser

    args = build_parser().parse_args(["assembly", "db.npz", "a.fasta", "--paf", "hits.paf", "--cs", "--eqx"])
    assert args.paf == "hits.paf" and args.cs is True and args.eqx is True
    plain = build_parser().parse_args(["assembly", "db.npz", "a.fasta", "--paf", "hits.paf"])
    assert not hasattr(plain, "cs") and not hasattr(plain, "eqx")  # off unless asked for
    for flag in ("--cs", "--eqx"):
        with pytest.raises(SystemExit):
            build_parser().parse_args(["assembly", "db.npz", "a.fasta", flag])
        assert "requires --paf" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        build_parser().parse_args(["convert", "x.jsonl", "--cs"])
