"""Multi-process / multi-device paths on real hardware (-m gpu).

A one-GPU box can still run the two-process form of bench.py: both ranks share device 0 (--share-gpu) and the barrier /
max-reduce run over gloo (RCCL refuses two ranks on one device).  That exercises what the 8-GPU scaling run does per
rank -- one process, one context, its own assemblies, no collective on the data path -- with two HIP contexts alive at
once.  The tests that need two devices are skipped below that."""

import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _device_count() -> int:
    import torch

    return torch.cuda.device_count()


def _run_bench(nproc: int, extra: list[str]) -> dict:
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), str(ROOT / "bench.py"), "--full", "--gpus", str(nproc), "--assemblies",
           "48", "--batch", "24", "--length", "400000", "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-e2e",
           "--workers", "1", *extra]  # fmt: skip
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)


def test_two_ranks_share_one_gpu_over_gloo():
    two = _run_bench(2, ["--dist-backend", "gloo", "--share-gpu"])
    assert two["n_gpus"] == 2 and two["scaling"] == "weak"
    # rank 0 of the two-process job types the same assemblies as a one-process job: same rows
    one = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--assemblies", "48", "--batch", "24", "--length", "400000",
                          "--steps", "1", "--warmup", "1", "--no-cpu-baseline", "--no-e2e", "--workers", "1"],
                         capture_output=True, text=True, timeout=900, cwd=ROOT)  # fmt: skip
    assert one.returncode == 0, one.stderr[-3000:]
    single = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][-1])
    digests = two["config"]["tsv_rows_sha1_per_rank"]
    assert len(digests) == 2 and digests[0] == single["config"]["tsv_rows_sha1"] and digests[1] != digests[0]
    assert two["config"]["typeable_in_last_step"] > 0


def test_eight_ranks_rehearse_config5_on_one_gpu():
    """BASELINE.json config 5 in miniature on whatever one box has: 8 ranks (8 processes, 8 HIP contexts, 8 driving
    threads) share device 0, `--assemblies-total` shards 256 assemblies over them with the product's partitioning rule,
    no collective on the data path.  Every rank's rows equal those of a single process typing the same seeds, no rank
    re-runs a pass for buffer growth after the warm-up, and the line says what each rank took of the host."""
    common = ["--batch", "16", "--length", "400000", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-e2e", "--workers", "1"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), str(ROOT / "bench.py"), "--full", "--gpus", "8", "--assemblies-total", "256",
           "--dist-backend", "gloo", "--share-gpu", *common]  # fmt: skip
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    eight = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    cfg = eight["config"]
    assert eight["n_gpus"] == 8 and cfg["assemblies_per_gpu"] == 32 and cfg["assemblies_total"] == 256
    assert "256 assemblies sharded over 8 ranks" in cfg["workload"]
    digests = cfg["tsv_rows_sha1_per_rank"]
    assert len(digests) == 8 and len(set(digests)) == 8
    per_rank = cfg["host_per_rank"]
    assert [h["rank"] for h in per_rank] == list(range(8))
    for h in per_rank:
        assert h["buffer_growth_reruns_in_timed_steps"] == [0], h
        # (a buffer may still grow ahead of need in these 16-assembly batches: a sub-slice's fill depends on the order in
        # which the scan's waves flushed, at this size by more than the 25 % of headroom that triggers growth; the default
        # run reports 0 -- profiles/r3_bench_line.json)
        assert 0 <= h["device_reallocations_in_timed_steps"] <= 4, h  # (a handful at most: growth ahead of need, never a rerun)
        assert h["process_cpu_s"] > 0 and h["driving_thread_cpu_s"] > 0 and h["max_rss_MB"] > 0 and h["pinned_host_MB"] >= 0
    for rank in (0, 3, 7):  # the same seeds in a process of their own
        one = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--assemblies", "32", "--as-rank", str(rank), *common],
                             capture_output=True, text=True, timeout=900, cwd=ROOT)  # fmt: skip
        assert one.returncode == 0, one.stderr[-3000:]
        single = json.loads([ln for ln in one.stdout.splitlines() if ln.startswith("{")][-1])
        assert single["config"]["tsv_rows_sha1"] == digests[rank], f"rank {rank}"


def test_schedule_does_not_change_the_rows():
    """One or two alignment passes ahead, resident batches or shards streamed from pinned host memory (with the TSV bytes
    formatted beside the main thread): the same rows, no buffer-growth rerun inside the timed steps, every leg reported."""
    def run(extra):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full", "--assemblies", "60", "--batch", "12", "--length", "400000",
                            "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--e2e-steps", "2", "--workers", "1", *extra],
                           capture_output=True, text=True, timeout=900, cwd=ROOT)  # fmt: skip
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])

    a, b = run(["--ahead", "1"]), run(["--ahead", "2"])
    assert a["config"]["tsv_rows_sha1"] == b["config"]["tsv_rows_sha1"]
    for line in (a, b):
        assert line["config"]["buffer_growth_reruns_in_timed_steps"] == [0]
        assert line["config"]["host_per_rank"][0]["device_reallocations_in_timed_steps"] >= 0  # (reported; see the 8-rank test)
        assert line["e2e"]["from_host_shards"] > 0 and line["e2e"]["with_tsv"] > 0 and line["e2e"]["tsv_bytes_per_step"] > 0
        assert line["roofline"]["alone"]["ms_per_launch"] > 0 and 0 < line["dp"]["fill_issue_model"]["frac"] < 1.5


def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    """A plain run times exactly --steps steps and prints the headline only; --dump-outputs writes the same arrays whether
    the run is plain or --full (same seeded inputs), and they agree with what the --full line reports."""
    import numpy as np

    def run(extra, out):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--assemblies", "40", "--batch", "16", "--length", "400000",
                            "--steps", "3", "--warmup", "1", "--workers", "1", "--dump-outputs", str(out), *extra],
                           capture_output=True, text=True, timeout=900, cwd=ROOT)  # fmt: skip
        assert r.returncode == 0, r.stderr[-3000:]
        return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])

    plain = run([], tmp_path / "plain")
    full = run(["--full", "--no-cpu-baseline", "--no-e2e"], tmp_path / "full")
    assert plain["steps"] == 3 and len(plain["ms_each_step"]) == 3 and plain["ms_per_step"] > 0 and plain["value"] > 0
    assert "roofline" not in plain and "e2e" not in plain and "roofline" in full
    names = sorted(p.name for p in (tmp_path / "plain").glob("*.npy"))
    assert names == sorted(p.name for p in (tmp_path / "full").glob("*.npy")) and "kpsc_k_best_locus.npy" in names
    for name in names:
        a, b = np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name)
        assert a.dtype == np.float64 and np.array_equal(a, b), name
    assert len(np.load(tmp_path / "plain" / "kpsc_o_typeable.npy")) == 40
    typeable = sum(int(np.load(tmp_path / "plain" / f"{db}_typeable.npy").sum()) for db in ("kpsc_k", "kpsc_o"))
    assert typeable == full["config"]["typeable_in_last_step"] > 0


@pytest.mark.skipif("_device_count() < 2")
def test_two_ranks_two_gpus_over_rccl():
    two = _run_bench(2, [])
    assert two["n_gpus"] == 2 and len(two["config"]["tsv_rows_sha1_per_rank"]) == 2


@pytest.mark.skipif("_device_count() < 2")
def test_cli_types_across_two_devices(tmp_path):
    """`--devices 0,1`: one worker thread bound to each device; rows come back in input order and equal the one-device
    run's."""
    from kaptive_amd.cli import main
    from kaptive_amd.synth import make_assembly, make_db

    db = make_db("kpsc_k", seed=7, n_loci=9)
    db_path = db.save(tmp_path / "db.npz")
    paths = []
    for i in range(10):
        g = make_assembly(db, seed=30 + i, length=80_000, median_contigs=5, min_contig=200)
        p = tmp_path / f"{g.id}.fasta"
        p.write_bytes(g.contigs.to_fasta())
        paths.append(str(p))
    out1, out2 = tmp_path / "one.tsv", tmp_path / "two.tsv"
    assert main(["assembly", str(db_path), *paths, "-o", str(out1), "--batch-size", "3"]) == 0
    assert main(["assembly", str(db_path), *paths, "-o", str(out2), "--batch-size", "3", "--devices", "0,1"]) == 0
    assert out1.read_bytes() == out2.read_bytes()
