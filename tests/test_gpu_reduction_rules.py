"""The typing reduction on the device -- kp_score_kernel, kp_reduce_kernel, kp_state_kernel (csrc/kp_reduce.hip) -- on the cases of
tests/reduction_rules_util.py: per database ONE batch, the rules assembly once per case, the cases' hit tables put in place by
Batch.set_hits.  Every result is the REFERENCE's recorded one (tests/golden/typing_rules_<key>.npz); every raw record -- summary,
kept rows, pieces, protein bytes, locus scores -- is the core header's through the g++ harness (which
tests/test_reduction_rules_cpu.py pins to the same fixture); and typing the batch again, and a batch with the tables in
reverse order, gives every assembly the same bytes -- as do contexts made with KAPTIVE_AMD_PIECE_CAP on either side of the
`piece_tmp` limit and with KAPTIVE_AMD_PROT_CAP at the exact fit of the largest case and one codon short (overflow bit 3, rerun)."""

import ctypes as C
import os

import numpy as np
import pytest

from kaptive_amd import _native
from kaptive_amd.serotyping import batch as B
from kaptive_amd.serotyping.core import Serotyper
from tests import reduction_rules_util as U
from tests.golden_util import load_db

pytestmark = pytest.mark.gpu


def _type(eng, typer, batch, tables, genome):
    """set_hits + the steps of Engine.type_batch, keeping the raw records: (BatchTyping, scores, counts, sums, kept, pieces, prots)."""
    off = np.concatenate([[0], np.cumsum([len(t) for t in tables])]).astype(np.int64)
    batch.set_hits(np.concatenate(tables).astype(_native.HIT_DTYPE), off)
    scores, counts = batch.score(typer.min_gene_coverage)
    bt = eng.type_batch(typer, batch, [genome.id] * len(tables), [genome] * len(tables), aligned=True)
    sums, kept, pieces = batch.typing()
    prots = []
    for a in range(len(tables)):
        k = kept[a, : sums["n_kept"][a]]
        prots.append(batch.proteins(a, int((k["prot_off"] + k["prot_len"]).max()) if len(k) else 0))
    # kp_batch_proteins copies min(room, prot_cap) bytes and returns how many: with room to spare that is the capacity the run ended with
    room = np.zeros(1 << 22, np.uint8)
    cap = int(_native.lib().kp_batch_proteins(batch.ctx._h, batch._h, C.c_int32(0), room.ctypes.data_as(C.c_void_p), C.c_int64(len(room))))
    return bt, scores, counts, sums, kept, pieces, prots, cap


def _slot_codons(kept):
    frame, n = (3 - kept["q_start"] % 3) % 3, kept["t_end"] - kept["t_start"]
    return np.where(n > frame, (n - frame) // 3, 0)


def _bytes_of(run, a):
    """Everything the device reported for assembly a, limited to its counts."""
    _, scores, counts, sums, kept, pieces, prots, _ = run
    k = kept[a, : sums["n_kept"][a]]
    words = [prots[a][o : o + n].tobytes() for o, n in zip(k["prot_off"], k["prot_len"])]
    return (scores[a].tobytes(), counts[a].tobytes(), sums[a].tobytes(), k.tobytes(), pieces[a, : sums["n_pieces"][a]].tobytes(), b"|".join(words))


@pytest.fixture(scope="module", params=["k", "o"])
def runs(request, oracle):
    from kaptive_amd.engine import Engine

    key = request.param
    db = load_db(key)
    genome, recorded = U.load_rules(key)
    assert all(not r[5] for r in recorded)  # one set of Serotyper keywords: one batch
    eng, typer = Engine(db), Serotyper(db)
    typer._engine = eng
    tables = [np.asarray(r[2]) for r in recorded]
    packed = genome.packed()
    batch = eng.ctx.batch([packed] * len(tables))
    batch.align_async()
    batch.wait()
    first = _type(eng, typer, batch, tables, genome)
    again = _type(eng, typer, batch, tables, genome)
    batch.close()
    batch = eng.ctx.batch([packed] * len(tables))
    batch.align_async()
    batch.wait()
    turned = _type(eng, typer, batch, tables[::-1], genome)
    batch.close()
    core = [U.core_records(db, typer, genome, t, oracle) for t in tables]
    eng.close()
    # the capacities are read from the environment once per context
    codons = max(int(_slot_codons(c["kept"]).sum()) for c in core)
    capped = {}
    for name, value in (("KAPTIVE_AMD_PIECE_CAP", U.PIECE_TMP), ("KAPTIVE_AMD_PIECE_CAP", U.PIECE_TMP + 1), ("KAPTIVE_AMD_PROT_CAP", codons),
                        ("KAPTIVE_AMD_PROT_CAP", codons - 1)):  # fmt: skip
        old = os.environ.get(name)
        os.environ[name] = str(value)
        try:
            eng = Engine(db)
            typer._engine = eng
            batch = eng.ctx.batch([packed] * len(tables))
            batch.align_async()
            batch.wait()
            capped[f"{name}={value}"] = _type(eng, typer, batch, tables, genome)
            batch.close()
            eng.close()
        finally:
            if old is None:
                del os.environ[name]
            else:
                os.environ[name] = old
    yield key, recorded, first, again, turned, core, capped


def test_results_are_the_references(runs):
    key, recorded, first, *_ = runs
    for r, res in zip(recorded, first[0].results()):
        try:
            U.check_against_fixture(res, r[3], r[4])
        except AssertionError as e:
            raise AssertionError(f"{key} {r[0]} {r[1]}: {e}") from e


def test_locus_scores_are_the_core_headers(runs):
    key, recorded, first, _, _, core, _ = runs
    for a, (r, c) in enumerate(zip(recorded, core)):
        assert first[1][a].tobytes() == c["scores"].tobytes(), (key, r[1], "scores")
        assert first[2][a].tobytes() == c["counts"].tobytes(), (key, r[1], "counts")
        assert int(first[3]["best_locus"][a]) == c["best"], (key, r[1])


def test_raw_records_are_the_core_headers(runs):
    key, recorded, first, _, _, core, _ = runs
    _, _, _, sums, kept, pieces, prots, _ = first
    for a, (r, c) in enumerate(zip(recorded, core)):
        want = np.array([c["summary"]], B.SUMMARY_DTYPE)[0].copy()
        want["n_final"] = int(((c["kept"]["flags"] & B.F_SPURIOUS) == 0).sum())  # (the harness leaves kp_state_kernel's count out)
        for f in B.SUMMARY_DTYPE.names:
            assert np.asarray(sums[a][f]).tobytes() == np.asarray(want[f]).tobytes(), (key, r[1], f, sums[a][f], want[f])
        nk, npc = int(sums["n_kept"][a]), int(sums["n_pieces"][a])
        assert nk == len(c["kept"]) and npc == len(c["pieces"]), (key, r[1])
        for f in B.KEPT_DTYPE.names:
            assert kept[a, :nk][f].tobytes() == c["kept"][f].tobytes(), (key, r[1], f)
        assert kept[a, :nk].tobytes() == c["kept"].tobytes(), (key, r[1])
        assert pieces[a, :npc].tobytes() == c["pieces"].tobytes(), (key, r[1])
        for i in range(nk):
            o, n = int(c["kept"]["prot_off"][i]), int(c["kept"]["prot_len"][i])
            assert prots[a][o : o + n].tobytes() == c["prot"][o : o + n].tobytes(), (key, r[1], i)


def test_repeat_and_reverse_give_the_same_bytes(runs):
    key, recorded, first, again, turned, _, _ = runs
    n = len(recorded)
    for a, r in enumerate(recorded):
        assert _bytes_of(first, a) == _bytes_of(again, a), (key, r[1], "typed again")
        assert _bytes_of(first, a) == _bytes_of(turned, n - 1 - a), (key, r[1], "reverse order")


def test_capacities_on_either_side_of_their_limits_change_nothing(runs):
    key, recorded, first, _, _, core, capped = runs
    assert len(capped) == 4
    codons = [int(_slot_codons(c["kept"]).sum()) for c in core]
    assert sorted(codons)[-1] > sorted(set(codons))[-2]  # one codon short overflows the largest case alone
    # the capacity is counted in codons and taken as given: the exact fit runs once, one codon short raises overflow bit 3 and the
    # reduction runs again with four times the room (kp_caps_grow_run)
    top = max(codons)
    assert capped[f"KAPTIVE_AMD_PROT_CAP={top}"][7] == top and capped[f"KAPTIVE_AMD_PROT_CAP={top - 1}"][7] == 4 * (top - 1), (key, top)
    assert first[7] > top
    for what, run in capped.items():
        for a, r in enumerate(recorded):
            assert _bytes_of(first, a) == _bytes_of(run, a), (key, r[1], what)
