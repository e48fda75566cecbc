"""bench.py --dump-outputs DIR: the classes the last timed step computed, as DIR/classes.npy (float32), from inputs that
are the same in every run with the same arguments; a plain run prints the headline line and nothing that --full adds."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_outputs_under_test", BENCH)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_dump_writes_float32_classes(tmp_path):
    b = _bench_module()
    classes = np.arange(1000, dtype=np.int32) % 10
    b.dump_outputs(str(tmp_path / "out"), classes)
    got = np.load(tmp_path / "out" / "classes.npy")
    assert got.dtype == np.float32 and got.shape == (1000,)
    assert (got == classes).all()


def test_dump_of_a_large_output_is_a_fixed_sample_under_the_cap(tmp_path, monkeypatch):
    b = _bench_module()
    monkeypatch.setattr(b, "DUMP_MAX_VALUES", 100)
    classes = np.arange(1000, dtype=np.int32)
    b.dump_outputs(str(tmp_path / "a"), classes)
    b.dump_outputs(str(tmp_path / "b"), classes)
    a = np.load(tmp_path / "a" / "classes.npy")
    assert a.shape == (100,) and (np.diff(a) > 0).all()                    # image order, no repeats
    assert (a == np.load(tmp_path / "b" / "classes.npy")).all()            # the same sample every time


def test_the_cap_keeps_a_dump_under_64_mb():
    assert _bench_module().DUMP_MAX_VALUES * 4 + 128 <= 64e6


def test_full_is_off_by_default():
    b = _bench_module()
    assert b.parse_args([]).full is False and b.parse_args(["--full"]).full is True
    assert b.parse_args([]).dump_outputs is None


@pytest.mark.gpu
def test_plain_run_dumps_the_classes_of_its_timed_steps(tmp_path):
    """a plain single-GPU run: the line holds the headline keys and none of --full's figures; classes.npy holds the
    classes of the seeded batch, equal to the CPU restatement's on a sample"""
    import torch
    import oracle_lib as ol
    batch = 16384
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", str(batch),
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["value"] > 0 and d["ms_per_step"] > 0 and d["full"] is False
    assert d["unit"] == "images/s" and d["higher_is_better"] is True and d["dtype"] == "u1"
    for key in ("cpu_baseline", "other_configs", "pcie_inclusive", "file_abi_inclusive", "multi_gpu"):
        assert key not in d, key
    assert "calibration" not in d["valu"]
    got = np.load(tmp_path / "classes.npy")
    assert got.dtype == np.float32 and got.shape == (batch,)
    # the bench's rank-0 batch, regenerated from its seed on the same device
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    imgs = torch.randint(0, 256, (batch, 3072), dtype=torch.uint8, device="cuda:0", generator=g).cpu().numpy()
    k = 2048
    want = ol.Oracle("cnvW1A1", ol.param_dir("cifar10", "cnvW1A1")).classes_batched(imgs[:k], 10)
    assert (got[:k] == want).all()
