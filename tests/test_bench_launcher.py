"""bench.py --gpus N without an outer launcher must start N ranks itself (the reference's pattern is
mp.spawn, train.py:289, 65).  Driven here on CPU tensors with gloo: same launcher, same rendezvous, same barrier + MAX
timing protocol, same single JSON line from rank 0 -- only the workload is a stand-in."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(*argv, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=300, env=e, cwd=ROOT)


def test_gpus_2_starts_two_ranks_and_prints_one_line():
    r = run("--gpus", "2", "--workload", "selftest", "--backend", "gloo", "--steps", "4", "--warmup", "1")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 4 and line["warmup"] == 1 and line["scaling"] == "weak"
    assert line["value"] > 0 and line["ms_per_step"] > 0


def test_dump_outputs_writes_the_last_step_and_repeats(tmp_path):
    """--dump-outputs DIR: what the timed step returned, as DIR/<name>.npy, the same from run to run (seeded inputs)."""
    import numpy as np
    dumps = []
    for i in range(2):
        d = tmp_path / str(i)
        r = run("--workload", "selftest", "--backend", "gloo", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d))
        assert r.returncode == 0, r.stderr[-2000:]
        dumps.append(np.load(d / "product.npy"))
    assert dumps[0].dtype == np.float32 and dumps[0].shape == (64, 64) and np.isfinite(dumps[0]).all()
    assert np.array_equal(dumps[0], dumps[1])


def test_dump_outputs_samples_above_64_mb(tmp_path):
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    big = {"flow": np.arange(10_000_000, dtype=np.float64).reshape(2, 5, 1_000_000), "metric": np.float64(1.5)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 10 ** 6
    a, b = np.load(tmp_path / "a" / "flow.npy"), np.load(tmp_path / "b" / "flow.npy")
    assert a.ndim == 1 and 0 < a.size < 10_000_000 and np.array_equal(a, b)  # a fixed sample: the same elements every run
    assert np.all(np.diff(a) > 0)                                            # distinct elements in ascending index order
    assert np.load(tmp_path / "a" / "metric.npy").dtype == np.float64


def test_steps_sets_the_timed_steps():
    r = run("--workload", "selftest", "--backend", "gloo", "--steps", "0")
    assert r.returncode != 0 and "--steps" in r.stderr


def test_launcher_world_size_must_match_gpus():
    """Under an outer launcher (WORLD_SIZE set) --gpus has to agree with it: a 1-rank run must not print n_gpus: 8."""
    r = run("--gpus", "2", "--workload", "selftest", "--backend", "gloo", env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "--gpus 2" in (r.stderr + r.stdout)


def test_failed_rank_fails_the_launch():
    r = run("--gpus", "2", "--workload", "selftest", "--backend", "nccl")  # selftest refuses nccl: both ranks exit non-zero
    assert r.returncode != 0


def test_hotpath_sequence_runs_with_the_cpu_port():
    """bench.py's cpu_baseline leg (--workload hotpath) drives rpeflow_amd.hotpath.HotPathWorkload with the PyTorch-CPU port of
    the reference path as ``ops``: the harness must not depend on the native operators' extra arguments."""
    from types import SimpleNamespace

    import torch

    from oracle import torch_ref
    from rpeflow_amd.hotpath import OP_NAMES, HotPathWorkload

    ops = SimpleNamespace(**{n: getattr(torch_ref, n) for n in OP_NAMES})
    wl = HotPathWorkload(batch=1, height=64, width=128, n_points=8192, device="cpu", ops=ops)
    flow_3d, corr_2d = wl()
    assert flow_3d.shape == (1, 3, 8192) and corr_2d.shape[:2] == (1, 81)
    assert torch.isfinite(flow_3d).all() and torch.isfinite(corr_2d).all()
