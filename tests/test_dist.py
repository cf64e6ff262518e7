"""Multi-rank path of bench.py on CPU (gloo, world_size 2): stream sharding
covers every stream exactly once and the only collective (timing / sample
counters) reduces max / sum."""
import os
import socket

import pytest
import torch.multiprocessing as mp


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, q):
    import torch
    import torch.distributed as dist

    import bench
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    lo, hi = bench.shard_streams(1024, rank, world)
    elapsed, samples = bench.reduce_stats(0.5 + rank, (hi - lo) * 2 * 441000, device=torch.device("cpu"))
    q.put((rank, lo, hi, elapsed, samples))
    dist.destroy_process_group()


def test_gloo_two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (r0, lo0, hi0, e0, s0), (r1, lo1, hi1, e1, s1) = res
    assert (lo0, hi0, lo1, hi1) == (0, 512, 512, 1024)
    assert e0 == e1 == 1.5                     # max over ranks
    assert s0 == s1 == 1024 * 2 * 441000       # summed samples


@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
def test_shards_partition_streams(world):
    import bench
    seen = []
    for r in range(world):
        lo, hi = bench.shard_streams(1024, r, world)
        seen.extend(range(lo, hi))
    assert seen == list(range(1024))


def _worker_resample(rank, world, port, q):
    """Each rank resamples its contiguous shard of config 4's streams (dry-run handle: the host
    state machine, exact reference counts, no GPU) in 4096-frame ProcessMulti calls + FlushMulti,
    then the counters go through bench.reduce_stats (the only collective)."""
    import numpy as np
    import torch
    import torch.distributed as dist

    import bench
    import gar
    from helpers import chunk_sizes
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    streams, frames = 64, 44_100  # config 4's shape at 1/16 of the streams and 1/10 of the length
    lo, hi = bench.shard_streams(streams, rank, world)
    r = gar.NewBatch(gar.Config(44100, 48000, 2, gar.QualityHigh, DryRun=True), hi - lo)
    out = 0
    for n in chunk_sizes(frames, 4096):
        xs = [np.zeros(n)] * (2 * (hi - lo))
        out += sum(len(y) for y in r.ProcessMulti(xs))
    out += sum(len(y) for y in r.FlushMulti())
    _, total = bench.reduce_stats(1.0, out, device=torch.device("cpu"))
    q.put((rank, hi - lo, out, total))
    dist.destroy_process_group()


def test_gloo_two_ranks_resample_shards(O):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker_resample, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # the reference's own count for one stream, every stream identical
    ref = O.NewResampler(44100, 48000, 1, O.P_HIGH)
    per_channel = sum(len(ref.process(__import__("numpy").zeros(n), 0)) for n in [4096] * 10 + [44_100 - 40_960])
    per_channel += len(ref.flush(0))
    (_, n0, out0, t0), (_, n1, out1, t1) = res
    assert (n0, n1) == (32, 32)
    assert out0 == out1 == 32 * 2 * per_channel
    assert t0 == t1 == 64 * 2 * per_channel


def _run_bench(nproc, extra):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    args = ["--dry-run", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"] + extra
    if nproc == 1:
        cmd = [sys.executable, os.path.join(root, "bench.py")] + args
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
               "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(root, "bench.py")] + args
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 prints one JSON line
    return json.loads(lines[0])


def test_bench_main_two_ranks_dry_run():
    """bench.py main() end to end under torch.distributed.run with WORLD_SIZE=2 (gloo, dry-run
    handles = the exact host state machine): cfg4's 1024 streams sharded one NewBatch per
    rank, the counters reduced over ranks, equal the single-rank totals; the weak-scaled
    secondary (cfg5 per rank) doubles."""
    extra = ["--full", "--workload", "cfg4", "--seconds", "0.5", "--secondary", "cfg5"]
    one = _run_bench(1, extra)
    two = _run_bench(2, extra)
    assert two["n_gpus"] == 2 and one["n_gpus"] == 1
    assert two["dry_run"] is True
    assert two["input_samples_total"] == one["input_samples_total"] == 1024 * 2 * 22050
    assert two["output_samples_total"] == one["output_samples_total"]
    assert two["config"]["streams_per_gpu"] == 512 and one["config"]["streams_per_gpu"] == 1024
    s1, s2 = one["secondary"]["cfg5"], two["secondary"]["cfg5"]
    assert s2["input_samples_total"] == 2 * s1["input_samples_total"]
    assert s2["output_samples_total"] == 2 * s1["output_samples_total"]


def _bench_cmd(args, env_extra=None):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, capture_output=True, text=True,
                          timeout=600, env=env, cwd=root)


def test_bench_gpus_flag_starts_ranks_itself():
    """`bench.py --gpus 2` with no torchrun wrapper starts the two ranks itself (a child
    torch.distributed.run before any GPU call) and relays rank 0's line: n_gpus 2, cfg4 sharded
    512 streams per rank, both ranks listed (VERDICT r04 'make --gpus authoritative')."""
    import json
    p = _bench_cmd(["--dry-run", "--gpus", "2", "--workload", "cfg4", "--seconds", "0.5", "--secondary", "none",
                    "--steps", "2", "--warmup", "1", "--no-cpu-baseline"])
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2
    assert d["config"]["streams_per_gpu"] == 512
    assert sorted(r["rank"] for r in d["ranks"]) == [0, 1]
    assert d["input_samples_total"] == 1024 * 2 * 22050
    assert list(d)[:4] == ["metric", "value", "unit", "n_gpus"]


def test_bench_two_ranks_line_carries_cpu_baseline_and_per_rank():
    """A world-2 line is as complete as a world-1 line: rank 0 times the CPU
    baseline after the timed regions (here a bounded 0.3 s sample), and the line lists every rank's
    own step time and kernel figures (all_gather over the process group)."""
    import json
    p = _bench_cmd(["--full", "--dry-run", "--gpus", "2", "--workload", "cfg2", "--seconds", "0.5", "--secondary", "cfg4",
                    "--steps", "2", "--warmup", "1", "--cpu-baseline-seconds", "0.3"])
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][0])
    assert d["n_gpus"] == 2
    cb = d["cpu_baseline"]
    assert cb and cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] == "port"
    assert sorted(r["rank"] for r in d["per_rank"]) == [0, 1]
    assert all(r["local_ms_per_step"] is not None for r in d["per_rank"])
    assert sorted(r["rank"] for r in d["secondary"]["cfg4"]["per_rank"]) == [0, 1]
    # build provenance: the library the run loaded, and whether make would rebuild it
    nl = d["native_lib"]
    assert nl["path"].endswith("libgar.so") and nl["bytes"] > 0 and len(nl["sha256_16"]) == 16
    assert isinstance(nl["newer_than_sources"], bool)


def test_bench_gpus_flag_conflicts_with_world_size():
    """Under a torchrun environment whose WORLD_SIZE differs from --gpus, bench.py exits non-zero
    instead of reporting a world it was not asked for."""
    p = _bench_cmd(["--dry-run", "--gpus", "4", "--secondary", "none"], {"WORLD_SIZE": "2", "RANK": "0"})
    assert p.returncode == 2
    assert "WORLD_SIZE=2" in p.stderr
