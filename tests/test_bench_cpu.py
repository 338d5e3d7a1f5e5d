"""bench.py without a device: the launcher logic (`--gpus N` starts N ranks itself when no launcher did, and never reports fewer devices as N), the argument
checks and the output dump of --dump-outputs."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "DMVIO_BENCH_SHARE_DEVICE")}


def test_more_gpus_than_devices_is_refused():
    import torch
    n = torch.cuda.device_count() + 2
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "1"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=200, env=_env())
    assert p.returncode == 2 and not p.stdout.strip()
    assert b"--gpus %d asked for" % n in p.stderr and b"refusing" in p.stderr


def test_launcher_world_size_must_match_gpus():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "1"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=200, env=dict(_env(), WORLD_SIZE="2", RANK="0", LOCAL_RANK="0"))
    assert p.returncode != 0 and not p.stdout.strip() and b"WORLD_SIZE=2" in p.stderr


def test_steps_must_be_at_least_one():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=200, env=_env())
    assert p.returncode != 0 and not p.stdout.strip() and b"--steps must be >= 1" in p.stderr


def test_dump_outputs_writes_finite_float64_within_the_size_limit(tmp_path):
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    B, levels = 300, 4
    rng = np.random.RandomState(1)
    lr = rng.rand(B, 5); lr[:, levels:] = np.nan                  # what the tracker returns: NaN in the slot of the level that does not exist
    res = dict(good=np.ones(B, np.int32), pose7=rng.rand(B, 7), aff=rng.rand(B, 2), lastResiduals=lr, flow=rng.rand(B, 3), H=rng.rand(B, 8, 8),
               b=rng.rand(B, 8), iterations=np.arange(B, dtype=np.int32))
    bench.dump_outputs(str(tmp_path / "all"), res, levels)
    got = {f.name[:-4]: np.load(f) for f in (tmp_path / "all").iterdir()}
    assert set(got) == set(res) | {"frame_index"} and all(a.dtype == np.float64 and np.isfinite(a).all() for a in got.values())
    assert np.array_equal(got["lastResiduals"], lr[:, :levels]) and np.array_equal(got["H"], res["H"]) and np.array_equal(got["iterations"], np.arange(B))
    # over the limit: a fixed, seeded sample of the frames, the same in every run, named in frame_index
    for run in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / run), res, levels, max_bytes=100000)
    k1, k2 = np.load(tmp_path / "s1" / "frame_index.npy"), np.load(tmp_path / "s2" / "frame_index.npy")
    assert 0 < len(k1) < B and np.array_equal(k1, k2) and sum(f.stat().st_size for f in (tmp_path / "s1").iterdir()) < 100000 + 2048
    assert np.array_equal(np.load(tmp_path / "s1" / "pose7.npy"), res["pose7"][k1.astype(int)])
    # a non-finite value among the results is an error, never written
    res["pose7"][3, 0] = np.inf
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "bad"), res, levels)
    assert not (tmp_path / "bad").exists()
