"""Case tables and path classifier for the protein DP (kaptive_amd/csrc/kp_prot.hip), shared by
tests/test_protein_paths_cpu.py (no GPU: the tables reach what they are for, judged on the oracle's rows) and
tests/test_gpu_protein_paths.py (the device equals the oracle on every case).

The kernel file sends one operation down five code paths; ``path_of`` restates its dispatch so that every case can be
named by the path it takes, and the CPU module fails when a table no longer reaches a path or a threshold.

A case is ``(name, query, target, offset-or-None, k-or-None)``; offset and k are None in the unseeded mode.  All
sequences come from generators with fixed seeds.  A query derives from its target by substitutions and one deletion
plus one insertion of the same size far apart, so that the sequence keeps its length, scores are positive and the best
path has gaps.
"""

from __future__ import annotations

import numpy as np

# ---- the dispatch -----------------------------------------------------------------------------------------------------
# The constants of kaptive_amd/csrc/kp_prot.hip and include/kp_spec.h (KP_PROT_K), restated: the comment at REG_MAX_LEN in
# kp_prot.hip points back here.  Whoever changes one there changes it here, and tests/test_protein_paths_cpu.py then says
# which threshold is no longer met on both sides.
KP_PROT_K = 20  # half band of the unseeded mode (widened to |len1 - len2| + 1)
REG_MAX_LEN = 768  # residues per sequence the register forms stage
S2_CAP = 2048  # residues of the target the wide kernel stages
WAVE_NC_MAX = 8  # diagonals per lane of the wave-register form: bands of up to 64 * 8 diagonals
QP = 16  # lanes per pair of kp_protein_kernel: bands of up to 3 * QP or 4 * QP diagonals
ROWS_MAX = 64 * 6  # query residues of the rows-per-lane form (two, four or six rows on 64 lanes)

PATHS = ("empty", "exact", "quad3", "quad4", "wave4", "wave8", "rows2", "rows4", "rows6", "strips")
SEEDED_PATHS = tuple(p for p in PATHS if p != "exact")  # the seeded mode takes no shortcut
COLS = ("scores", "matches", "mismatches", "gaps", "q_starts", "q_ends", "t_starts", "t_ends")
SEEDED_KS = (0, 1, 7, 8, 23, 24, 31, 32, 127, 128, 255, 256, 300)
GOLDEN_KS = (0, 1, 2, 3, 5, 8, 20)
UNSEEDED_DS = (22, 23, 30, 31, 126, 127, 254, 255)

_STANDARD = frozenset(b"ARNDCQEGHILKMFPSTWYV")


def band_k(len1: int, len2: int, seeded: bool, k) -> int:
    return int(k) if seeded else max(KP_PROT_K, abs(len1 - len2) + 1)


def is_exact_prefix(q: bytes, t: bytes) -> bool:
    """What the kernels' shortcut tests: standard residues only, equal to the first len(q) residues of the target."""
    return len(q) <= len(t) and t.startswith(q) and _STANDARD.issuperset(q)


def _fits_registers(len1: int, len2: int, nb: int) -> bool:
    return nb <= 4 * QP and len1 <= REG_MAX_LEN and len2 <= REG_MAX_LEN


def path_of(len1: int, len2: int, seeded: bool, k, is_exact_prefix: bool, neighbours=()) -> str:
    """The path kp_protein_kernel / kp_protein_wide_kernel send a pair down.  ``neighbours``: (len1, len2, k,
    is_exact_prefix) of the other pairs of the quad (positions 4 * (p / 4) .. + 3 of one call); only the choice between
    quad3 and quad4 reads them -- it is made once per wave."""
    if len1 == 0 or len2 == 0:
        return "empty"
    kk = band_k(len1, len2, seeded, k)
    nb = 2 * kk + 1
    exact = bool(is_exact_prefix) and not seeded
    if _fits_registers(len1, len2, nb):
        if exact:
            return "exact"
        narrow = nb <= 3 * QP
        for n1, n2, nk, nexact in neighbours:
            if n1 == 0 or n2 == 0:
                continue
            nnb = 2 * band_k(n1, n2, seeded, nk) + 1
            if _fits_registers(n1, n2, nnb) and not (nexact and not seeded):  # a neighbour that runs the DP here
                narrow = narrow and nnb <= 3 * QP
        return "quad3" if narrow else "quad4"
    if exact:
        return "exact"
    if nb <= 64 * WAVE_NC_MAX and len1 <= REG_MAX_LEN and len2 <= S2_CAP:
        return "wave4" if nb <= 64 * 4 else "wave8"
    if len1 <= ROWS_MAX and len2 <= S2_CAP:
        return "rows2" if len1 <= 64 * 2 else "rows4" if len1 <= 64 * 4 else "rows6"
    return "strips"


def classify(cases) -> list[str]:
    """Paths of the cases of ONE call, in call order (quads are formed by position)."""
    seeded = bool(cases) and cases[0][3] is not None
    info = [(len(q), len(t), k, (not seeded) and is_exact_prefix(q, t)) for _, q, t, _, k in cases]
    out = []
    for p, (l1, l2, k, ex) in enumerate(info):
        q0 = p - p % 4
        out.append(path_of(l1, l2, seeded, k, ex, [info[x] for x in range(q0, min(q0 + 4, len(info))) if x != p]))
    return out


def strip_windows(len1: int, len2: int, k: int, shift: int = 0) -> list[int]:
    """Columns j_hi - j_lo + 1 that protein_pair_strips visits in each strip of 64 rows."""
    return [min(len2, i0 + 63 - shift + k) - max(1, i0 - shift - k) + 1 for i0 in range(1, len1 + 1, 64)]


def in_band_any(len1: int, len2: int, off: int, k: int) -> bool:
    """Whether any cell 1 <= i <= len1, 1 <= j <= len2 has |j - (i - off)| <= k."""
    return len1 > 0 and len2 > 0 and 1 - len1 + off <= k and len2 - 1 + off >= -k


def by_k(cases) -> dict:
    """Seeded cases grouped by k, table order kept: one call per k."""
    out: dict = {}
    for c in cases:
        out.setdefault(c[4], []).append(c)
    return out


def pack(cases):
    """(queries, targets) of a case list as kaptive_amd Sequences."""
    from kaptive_amd.core.seq import Sequences

    return Sequences.from_bytes([c[1] for c in cases]), Sequences.from_bytes([c[2] for c in cases])


# ---- sequences --------------------------------------------------------------------------------------------------------
AA = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", np.uint8)
ODD = np.frombuffer(b"BZX*JUObzxj-\x00\xff", np.uint8)  # B / Z / X / * / J, and bytes outside the alphabet


def _prot(rng, n: int) -> np.ndarray:
    return AA[rng.integers(0, 20, size=n)]


def _diverge(rng, seg: np.ndarray, sub: float = 0.1) -> np.ndarray:
    """``seg`` with substitutions and, from 30 residues on, one deletion in its second sixth and one insertion of the
    same size in its fifth sixth: the length stays, and the third of the sequence between them lies one or two
    diagonals off, which is worth far more than the two gaps cost."""
    q = seg.copy()
    n = len(q)
    hit = rng.random(n) < sub
    q[hit] = AA[rng.integers(0, 20, size=int(hit.sum()))]
    g = 2 if n >= 60 else 1 if n >= 30 else 0
    if g:
        a, b = int(rng.integers(n // 6, n // 3)), int(rng.integers(2 * n // 3, 5 * n // 6))
        q = np.concatenate([q[:a], q[a + g : b], _prot(rng, g), q[b:]])
    assert len(q) == n
    return q


def _sprinkle(rng, a: np.ndarray, frac: float) -> np.ndarray:
    a = a.copy()
    hit = rng.random(len(a)) < frac
    a[hit] = ODD[rng.integers(0, len(ODD), size=int(hit.sum()))]
    low = np.flatnonzero(rng.random(len(a)) < frac / 2)
    a[low] = np.where((a[low] >= 65) & (a[low] <= 90), a[low] | 0x20, a[low])  # lower case
    return a


def _pair(rng, len_q: int, len_t: int, odd: bool = False) -> tuple[bytes, bytes]:
    """A target of len_t residues (stop included) and a query of len_q derived from a stretch of it (or, when the query
    is the longer one, from all of it, with random residues before and after)."""
    core = _prot(rng, len_t - 1)
    if len_q <= len_t - 1:
        s = int(rng.integers(0, len_t - len_q))
        q = _diverge(rng, core[s : s + len_q])
    else:
        ext = len_q - (len_t - 1)
        e1 = int(rng.integers(0, ext + 1))
        q = np.concatenate([_prot(rng, e1), _diverge(rng, core), _prot(rng, ext - e1)])
    t = np.concatenate([core, np.frombuffer(b"*", np.uint8)])
    if odd:
        q, t = _sprinkle(rng, q, 0.06), _sprinkle(rng, t, 0.03)
    assert len(q) == len_q and len(t) == len_t
    return q.tobytes(), t.tobytes()


def _outer(rng, len_q: int, d: int) -> tuple[bytes, bytes]:
    """A query d residues shorter than its target whose last three fifths lie on the band's outermost diagonal
    j - i = d + 1 = k: the target from residue d on, one residue skipped after two fifths, one random residue appended.
    A band that has lost its last diagonal cannot follow it."""
    t = np.concatenate([_prot(rng, len_q + d - 1), np.frombuffer(b"*", np.uint8)])
    a = 2 * len_q // 5
    q = np.concatenate([t[d : d + a], t[d + a + 1 :], _prot(rng, 1)])
    hit = rng.random(len_q) < 0.1
    q[hit] = AA[rng.integers(0, 20, size=int(hit.sum()))]
    assert len(q) == len_q
    return q.tobytes(), t.tobytes()


def _planted(rng, len1: int, len2: int, true_off: int, odd: bool = False) -> tuple[bytes, bytes]:
    """Query residue i is homologous to target residue i - true_off (offset = query position - target position)."""
    t = _prot(rng, len2)
    if true_off >= 0:
        n = max(0, min(len1 - true_off, len2))
        q = np.concatenate([_prot(rng, min(true_off, len1)), _diverge(rng, t[:n])])
    else:
        n = max(0, min(len1, len2 + true_off))
        q = _diverge(rng, t[-true_off : -true_off + n])
    q = np.concatenate([q, _prot(rng, len1 - len(q))])
    if odd:
        q, t = _sprinkle(rng, q, 0.06), _sprinkle(rng, t, 0.03)
    assert len(q) == len1 and len(t) == len2
    return q.tobytes(), t.tobytes()


# ---- unseeded table ---------------------------------------------------------------------------------------------------
# (name, unit, query repeats, target repeats): W + unit * n is no exact prefix, and every placement of the query scores the same
_TIES = (("quad3", b"GS", 50, 55), ("quad4", b"GS", 50, 62), ("wave4", b"MKL", 40, 70), ("wave8", b"PT", 60, 150),
         ("rows2", b"A", 100, 400), ("rows4", b"GS", 100, 300), ("rows6", b"Q", 300, 700), ("strips", b"GS", 250, 500))  # fmt: skip
_ODD_SHAPES = (("quad3", 150, 160), ("quad4", 150, 176), ("wave4", 150, 250), ("wave8", 150, 350), ("rows2", 100, 500),
               ("rows4", 200, 600), ("rows6", 300, 700), ("strips", 500, 900))  # fmt: skip
# query x target lengths at the edges of the staging limits and of the rows-per-lane classes
_EDGE_SHAPES = ((763, 768), (764, 769), (768, 763), (769, 764), (768, 768), (769, 769), (768, 769), (769, 768),
                (200, 2048), (200, 2049), (700, 2048), (700, 2049),
                (128, 428), (129, 429), (256, 556), (257, 557), (384, 684), (385, 685), (500, 900), (768, 1100),
                (64, 2100), (65, 2100), (128, 2100), (129, 2100),
                (100, 400), (60, 700), (127, 2048), (90, 1000), (250, 600), (350, 800), (384, 2048))  # fmt: skip
# strips whose window is exactly this many columns in some strip: (columns, query, target)
STRIP_WINDOWS = ((64, 800, 64), (128, 800, 128), (2048, 500, 2048), (2049, 500, 2049), (2048, 1100, 2091))
BIGGEST = (2500, 2600)  # the one large strips case


def unseeded_table(seed: int = 20240) -> list[tuple]:
    rng = np.random.default_rng(seed)
    cases: list[tuple] = []
    n_fill = [0]

    def add(name, q, t):
        cases.append((name, q, t, None, None))

    def quad(members):
        """Members at the start of a quad of their own, the rest of it narrow fillers."""
        assert len(cases) % 4 == 0 and len(members) <= 4
        for name, q, t in members:
            add(name, q, t)
        while len(cases) % 4:
            n_fill[0] += 1
            add(f"filler{n_fill[0]}", *_pair(rng, 30, 32))

    # the same pairs in different company: `narrow` is one choice per wave
    x, n1, n2, n3, w = _pair(rng, 90, 100), _pair(rng, 80, 85), _pair(rng, 100, 90), _pair(rng, 60, 82), _pair(rng, 100, 125)
    quad([("company_n1@A", *n1), ("company_x@A", *x), ("company_n2@A", *n2), ("company_n3@A", *n3)])
    quad([("company_n1@B", *n1), ("company_x@B", *x), ("company_d25", *w), ("company_n3@B", *n3)])
    # one empty, one exact-prefix, one DP pair and one pair of the wide kernel, the DP pair in every group of the wave
    tx = _prot(rng, 120).tobytes() + b"*"
    roles = [("dp", *_pair(rng, 90, 100)), ("empty", b"", tx), ("exact", tx[:50], tx), ("wide", *_pair(rng, 100, 160))]
    for r in range(4):
        order = roles[-r:] + roles[:-r] if r else roles
        quad([(f"mixed{r}_{role}", q, t) for role, q, t in order])
    # |len1 - len2| on both sides of every band threshold, in both directions
    for d in UNSEEDED_DS:
        quad([(f"d{d}_qshort_small", *_pair(rng, 150, 150 + d)), (f"d{d}_qlong_small", *_pair(rng, 150 + d, 150)),
              (f"d{d}_outer", *_outer(rng, 150, d))])  # fmt: skip
        add(f"d{d}_qshort_above", *_pair(rng, 790 - d, 790))
        add(f"d{d}_qlong_above", *_pair(rng, 790, 790 - d))
        while len(cases) % 4:
            n_fill[0] += 1
            add(f"filler{n_fill[0]}", *_pair(rng, 30, 32))
    for name, unit, nq, nt in _TIES:
        quad([(f"tie_{name}_w_first", unit * nq, b"W" + unit * nt + b"*"), (f"tie_{name}_w_last", unit * nq + b"W", unit * nt + b"*")])
    for name, lq, lt in _ODD_SHAPES:
        quad([(f"odd_{name}", *_pair(rng, lq, lt, odd=True))])
    for lq, lt in _EDGE_SHAPES:
        add(f"edge_{lq}x{lt}", *_pair(rng, lq, lt))
    for cols, lq, lt in STRIP_WINDOWS:
        add(f"window{cols}_{lq}x{lt}", *_pair(rng, lq, lt))
    add("biggest_strips", *_pair(rng, *BIGGEST))
    add("empty_query", b"", tx)
    add("empty_target", tx[:40], b"")
    add("empty_both", b"", b"")
    # the shortcut in both kernels' territory, and where the whole query also fits further right
    for n, cut in ((300, 300), (500, 100), (800, 800), (2100, 200)):
        t = _prot(rng, n).tobytes()
        add(f"exact_{cut}_of_{n}", t[:cut], t + b"*")
    add("exact_repeat_narrow", b"MK" * 15, b"MK" * 30 + b"*")
    add("exact_repeat_wide", b"GSG" * 100, b"GSG" * 200 + b"*")
    return cases


def company_pairs(cases) -> list[tuple[int, int]]:
    """Positions of the pairs that appear once in quad A and once in quad B."""
    pos = {c[0]: i for i, c in enumerate(cases)}
    return [(i, pos[name[:-2] + "@B"]) for name, i in pos.items() if name.endswith("@A") and name[:-2] + "@B" in pos]


# ---- seeded table -----------------------------------------------------------------------------------------------------
def _seeded_shapes(k: int):
    if k <= 31:  # register kernel; wave registers by the target's length; strips by either length
        return (("reg", 120, 150), ("wavelen", 200, 800), ("stripq", 800, 300), ("stript", 100, 2100))
    if k <= 255:
        return (("wave", 150, 180), ("wavelen", 200, 800), ("stripq", 800, 300), ("stript", 100, 2100))
    return (("rows2", 100, 400), ("rows4", 200, 400), ("rows6", 300, 500), ("stripq", 400, 500), ("stript", 100, 2100))


# lengths on both sides of every staging limit, run at the k of both sides of every band limit
_SEEDED_EDGE_KS = (31, 32, 255, 256)
_SEEDED_EDGE_SHAPES = ((768, 768), (769, 300), (300, 769), (300, 2048), (300, 2049), (768, 2048), (768, 2049), (384, 2048),
                       (385, 2048), (128, 400), (129, 400), (256, 400), (257, 400))  # fmt: skip


def offset_kinds(len1: int, len2: int, true_off: int, k: int) -> list[tuple[str, int]]:
    return [
        ("zero", 0), ("plus1", 1), ("minus1", -1), ("true", true_off),
        ("edge_hi", true_off + k), ("edge_lo", true_off - k),  # the homology on the band's first / last diagonal
        ("past_hi", true_off + k + 1), ("past_lo", true_off - k - 1),  # ... and just outside
        ("corner_q", len1 - 1 + k), ("corner_t", 1 - k - len2),  # only cell (len1, 1) / (1, len2) is in band
        ("out_q", len1 + k), ("out_q_far", len1 + k + 7), ("out_t", -(len2 + k)), ("out_t_far", -(len2 + k + 7)),
    ]  # fmt: skip


def _seeded_cases(rng, ks, shapes_of, edge_ks=(), edge_shapes=(), tie_ks=(), ident=((150, "reg"), (800, "strips"))) -> list[tuple]:
    cases: list[tuple] = []
    flip = 0
    for k in ks:
        for si, (sname, l1, l2) in enumerate(shapes_of(k)):
            flip += 1
            true_off = (5 if min(l1, l2) < 80 else 13) if flip % 2 else (-7 if min(l1, l2) < 80 else -19)
            q, t = _planted(rng, l1, l2, true_off)
            for oname, off in offset_kinds(l1, l2, true_off, k):
                cases.append((f"k{k}_{sname}_{l1}x{l2}_{oname}", q, t, off, k))
            if si == 0:
                cases.append((f"k{k}_{sname}_{l1}x{l2}_odd", *_planted(rng, l1, l2, true_off, odd=True), true_off, k))
        if k in edge_ks:
            for l1, l2 in edge_shapes:
                flip += 1
                true_off = 11 if flip % 2 else -17
                cases.append((f"k{k}_edge_{l1}x{l2}", *_planted(rng, l1, l2, true_off), true_off, k))
        for n, iname in ident:  # identical sequences: no shortcut in this mode, the DP finds the diagonal
            s = _prot(rng, n).tobytes()
            cases.append((f"k{k}_identical_{iname}_{n}", s, s, 0, k))
        some = _prot(rng, 40).tobytes()
        cases += [(f"k{k}_empty_query", b"", some, 3, k), (f"k{k}_empty_target", some, b"", -3, k), (f"k{k}_empty_both", b"", b"", 0, k)]
        if k in tie_ks:  # ties where the cells are not visited in row-major order (rows per lane), and in strips
            for tname, unit, nq, nt in (("rows2", b"GS", 60, 200), ("rows4", b"MKL", 80, 300), ("rows6", b"PT", 170, 400), ("strips", b"GS", 250, 400)):
                for off in (-1, 7, -40):
                    cases.append((f"k{k}_tie_{tname}_off{off}", unit * nq, b"W" + unit * nt + b"*", off, k))
    return cases


def seeded_table(seed: int = 20241) -> list[tuple]:
    return _seeded_cases(np.random.default_rng(seed), SEEDED_KS, _seeded_shapes, _SEEDED_EDGE_KS, _SEEDED_EDGE_SHAPES, tie_ks=(256, 300))


def golden_seeded_table(seed: int = 20242) -> list[tuple]:
    """The small end of the seeded table: what oracle/make_golden.py::gen_protein_dp_seeded runs through the reference
    (both sequences at most 60 residues).  The fixture stores these inputs; the tests read the fixture, not this."""
    shapes = (("a", 40, 55), ("b", 55, 40), ("c", 60, 60), ("d", 12, 30))
    return _seeded_cases(np.random.default_rng(seed), GOLDEN_KS, lambda k: shapes, ident=((40, "short"),))


# ---- big batches ------------------------------------------------------------------------------------------------------
BIG_N = 20003  # n % 4 == 3; 5001 quads on 4096 blocks: 905 blocks take a second trip through the pair loop
BIG_K = 20
BIG_BLOCKS = 4096  # kp_protein_align's grid


def big_batch(seed: int = 20243, wide: bool = False):
    """(queries, targets, offsets): 20 003 pairs of 8..40 residues, lengths drawn independently, about a third of the
    queries a prefix of their target, the rest diverged; with ``wide`` 24 of them replaced by pairs of 260 x 300
    residues (|len1 - len2| = 40: the wide kernel's in the unseeded mode).  Offsets in -6..6 for the seeded runs."""
    rng = np.random.default_rng(seed)
    lq, lt = rng.integers(8, 41, size=BIG_N), rng.integers(8, 41, size=BIG_N)
    pool = AA[rng.integers(0, 20, size=int(lt.sum()) + int(lq.sum()))]
    prefix = rng.random(BIG_N) < 1 / 3
    qs, ts = [], []
    at = 0
    for p in range(BIG_N):
        a, b = int(lq[p]), int(lt[p])
        t = pool[at : at + b]
        q = np.resize(t, a).copy() if a <= b else np.concatenate([t, pool[at + b : at + a]])
        at += max(a, b)
        if not prefix[p]:
            hit = rng.random(a) < 0.3
            q[hit] = AA[rng.integers(0, 20, size=int(hit.sum()))]
        qs.append(q.tobytes())
        ts.append(t.tobytes())
    if wide:
        wrng = np.random.default_rng(seed + 1)
        for p in sorted(wrng.choice(BIG_N, size=24, replace=False).tolist()):
            qs[p], ts[p] = _pair(wrng, 260, 300)
    return qs, ts, rng.integers(-6, 7, size=BIG_N).astype(np.int32)
