"""bench.py --dump-outputs / --full: the dumped arrays are what the timed path
computed (checked against the CPU parser), a large array is sampled at fixed
positions, and the result line carries ms_per_step for the steps asked for."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dmlc_core_amd import data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 20000  # ~0.8 M nnz: below bench.DUMP_MAX_ELEMS, so every array is dumped whole


def _bench(tmp_path, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rows", str(ROWS),
           "--data-dir", str(tmp_path / "bench"), *extra]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)


def _cpu_blocks(tmp_path):
    ddir = [d for d in os.listdir(tmp_path / "bench") if d.startswith("libsvm_")]
    assert len(ddir) == 1
    return list(data.iter_blocks(str(tmp_path / "bench" / ddir[0]), 0, 1, "libsvm"))


def test_dump_outputs_cpu_counts(tmp_path):
    out = tmp_path / "dump"
    p = _bench(tmp_path, "--device", "cpu", "--steps", "3", "--warmup", "0", "--full",
               "--dump-outputs", str(out))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    assert res["steps"] == 3 and res["warmup"] == 0 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(ROWS / (res["ms_per_step"] * 1e-3), rel=1e-3)
    cpu = _cpu_blocks(tmp_path)
    counts = np.load(out / "counts.npy")
    assert counts.dtype == np.float64
    assert counts[0] == ROWS == sum(len(b["label"]) for b in cpu)
    assert counts[1] == sum(len(b["index"]) for b in cpu)


def test_steps_must_be_positive(tmp_path):
    p = _bench(tmp_path, "--device", "cpu", "--steps", "0")
    assert p.returncode != 0 and "--steps must be >= 1" in p.stderr


def test_dump_sample_is_fixed(tmp_path, monkeypatch):
    import torch

    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 100)
    ids = np.arange(5000, dtype=np.uint32)
    ids[4999] = 2 ** 32 - 1  # negative when read as int32
    t = {"index": torch.from_numpy(ids),
         "offset": torch.from_numpy(np.arange(50, dtype=np.uint64) + (1 << 40)),
         "value": torch.arange(5000, dtype=torch.float32) * 0.5, "weight": None}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, t, (1, 2, 3, 4))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["counts.npy", "index.npy", "offset.npy", "value.npy"]
    for n in names:
        assert np.array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
    pos = np.sort(np.random.default_rng(0).integers(0, 5000, size=100))
    index, value = np.load(tmp_path / "a" / "index.npy"), np.load(tmp_path / "a" / "value.npy")
    assert index.dtype == np.float64 and value.dtype == np.float32
    expect = pos.astype(np.float64)
    expect[pos == 4999] = 2.0 ** 32 - 1
    assert np.array_equal(index, expect) and np.array_equal(value, pos * np.float32(0.5))
    assert np.array_equal(np.load(tmp_path / "a" / "offset.npy"), np.arange(50) + 2.0 ** 40)


@pytest.mark.gpu
def test_dump_outputs_match_cpu_parser(tmp_path):
    out = tmp_path / "dump"
    p = _bench(tmp_path, "--steps", "2", "--warmup", "1", "--dump-outputs", str(out))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads([x for x in p.stdout.splitlines() if x.startswith("{")][-1])
    assert res["steps"] == 2 and res["ms_per_step"] > 0 and res["allreduce_busbw_GBps"] is None
    cpu = _cpu_blocks(tmp_path)
    label = np.concatenate([b["label"] for b in cpu])
    index = np.concatenate([b["index"] for b in cpu])
    value = np.concatenate([b["value"] for b in cpu])
    lens = np.concatenate([np.diff(b["offset"].astype(np.int64)) for b in cpu])
    assert np.array_equal(np.load(out / "label.npy"), label)
    assert np.array_equal(np.load(out / "index.npy"), index.astype(np.float64))
    assert np.array_equal(np.load(out / "value.npy"), value)
    assert np.array_equal(np.diff(np.load(out / "offset.npy")), lens.astype(np.float64))
    assert list(np.load(out / "counts.npy")[:3]) == [len(label), len(index), index.max()]
