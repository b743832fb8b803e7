"""bench.py's command line: a plain run prints the headline figure only (the other legs need --full), and `--dump-outputs DIR`
writes what the last timed step returned as DIR/<name>.npy."""

import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]


def _bench():
    spec = importlib.util.spec_from_file_location("upa_bench", ROOT / "bench.py")
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_zeroes_rows_past_the_count_and_samples_large_arrays(tmp_path):
    bench = _bench()
    rows = torch.arange(2 * 300 * 6, dtype=torch.float32).reshape(2, 300, 6) + 1
    counts = torch.tensor([3, 0], dtype=torch.int32)
    keep = torch.arange(600, dtype=torch.int32).reshape(2, 300)
    big = torch.randn(bench.DUMP_SAMPLE + 1000)
    bench.dump_outputs(tmp_path, {"detections": bench._valid_rows(rows, counts), "counts": counts,
                                  "keep": bench._valid_rows(keep, counts, fill=-1), "parameters": big})
    det, cnt, kp, par = (np.load(tmp_path / f"{n}.npy") for n in ("detections", "counts", "keep", "parameters"))
    assert det.dtype == np.float32 and cnt.dtype == np.float64 and kp.dtype == np.float64
    assert np.array_equal(det[0, :3], rows[0, :3].numpy()) and not det[0, 3:].any() and not det[1].any()
    assert np.array_equal(cnt, [3, 0]) and np.array_equal(kp[0, :3], [0, 1, 2]) and (kp[0, 3:] == -1).all() and (kp[1] == -1).all()
    # a larger array: the same fixed sample every time, drawn from the array itself
    assert par.shape == (bench.DUMP_SAMPLE,) and np.isin(par, big.numpy()).all()
    bench.dump_outputs(tmp_path / "again", {"parameters": big})
    assert np.array_equal(np.load(tmp_path / "again" / "parameters.npy"), par)


def test_dump_outputs_is_refused_in_a_dry_run(tmp_path):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--dry-run", "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--dump-outputs" in r.stderr
    assert not (tmp_path / "d").exists()


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_the_last_step(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["unit"] == "images/s" and rec["higher_is_better"] is True and rec["dtype"] == "bf16"
    assert rec["metric"].startswith("images/sec (whole job = n_gpus x per-GPU bs=32) YOLOv8n 640x640")
    for leg in ("serial_ms_per_step", "latency_ms_per_batch", "roofline", "kernels", "cpu_baseline", "parity", "speed"):
        assert rec[leg] is None, leg
    det, cnt, keep = (np.load(tmp_path / f"{n}.npy") for n in ("detections", "counts", "keep"))
    assert det.dtype == np.float32 and det.shape == (32, 300, 6) and cnt.shape == (32,) and keep.shape == (32, 300)
    assert cnt.sum() > 0 and (cnt <= 300).all()
    for b, c in enumerate(cnt.astype(int)):
        assert not det[b, c:].any() and (keep[b, c:] == -1).all()
        assert (det[b, :c, 4] >= 0.25).all() and (keep[b, :c] >= 0).all() and (keep[b, :c] < 8400).all()
