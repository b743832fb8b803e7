"""Standalone step time of yolov5-BoT3 training: batch 16 at 640 x 640, bf16, the compiled step (one hipGraph), and - in a run of its
own, under the profiler - the time of the kernels this model's training path adds: the two MHSA backward launches, the MHSA train
forward and the 6x6 stem weight gradient.  Separate from bench.py, whose headline is the detection inference workload; nothing is gated
on it.  DESIGN.md section 8 quotes the attention backward's share: a matrix-core backward is an open item only above 5 %.

    python -m tools.bench_bot3_train                 # times; one JSON line, also written to profiles/bot3_train_bench.json
    python -m tools.bench_bot3_train --profile       # + per-kernel times: re-runs itself under `rocprofv3 --kernel-trace --stats`
    python -m tools.bench_bot3_train --steps-only    # what the profiled child runs: compiled steps, nothing printed

Timing: two eager steps (static buffers, code objects, the optimizer's first step), compile(), `--warmup` replays, then `--repeats`
windows of `--steps` steps each timed with device events; the median window is reported with the spread (min, max) next to it.  The
labels go up inside the timed window, as in real training."""

from __future__ import annotations

import argparse
import csv
import json
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from ultralytics_pro_amd.engine.trainer import DetectionTrainer  # noqa: E402
from ultralytics_pro_amd.nn.tasks import DetectionModel  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

KERNELS = ("mhsa_bwd_dq_kernel", "mhsa_bwd_dkv_kernel", "mhsa_mfma_bf16_d32_kernel", "mhsa_kernel", "wgrad_k6s2_kernel",
           "wgrad_k6_reduce_kernel")


def make(a, dev):
    m = DetectionModel("yolov5-BoT3.yaml")
    P.apply_procedural_weights(m)
    tr = DetectionTrainer(m, dtype=torch.bfloat16, device=dev)
    x = P.synthetic_images(a.batch, h=a.imgsz, w=a.imgsz).to(dev)
    lab = P.synthetic_labels(a.batch)
    tr.step(x, lab)
    tr.step(x, lab)
    tr.compile(x, lab, warm_steps=0)
    for _ in range(a.warmup):
        tr.step(x, lab)
    torch.cuda.synchronize()
    return tr, x, lab


def windows(tr, x, lab, a):
    ms = []
    for _ in range(a.repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            items = tr.step(x, lab)
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / a.steps)
    ms.sort()
    med = ms[len(ms) // 2]
    return dict(ms_per_step=round(med, 4), min=round(ms[0], 4), max=round(ms[-1], 4), images_per_s=round(a.batch / med * 1e3, 1),
                last_loss_items=[round(float(v), 4) for v in items])


def kernel_times(a, ms_per_step):
    """Run `--steps-only` under the profiler (a run of its own) and add up the kernel-stats rows of the new kernels."""
    out = ROOT / "profiles" / "bot3_train_trace"
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "--", sys.executable, "-m",
           "tools.bench_bot3_train", "--steps-only", "--batch", str(a.batch), "--imgsz", str(a.imgsz), "--steps", str(a.steps), "--warmup",
           str(a.warmup)]
    subprocess.run(cmd, check=True, cwd=str(ROOT), timeout=900)
    rows = []
    for f in out.rglob("*kernel_stats.csv"):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    if not rows:
        raise RuntimeError(f"no kernel_stats.csv under {out}")
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    ran = a.warmup + a.steps + 2  # the child's steps: two eager + warmup + steps
    per = {}
    for k in KERNELS:
        hit = [r for r in rows if k + "<" in r["Name"] or k + "(" in r["Name"] or r["Name"].endswith(k) or k + " " in r["Name"]]
        ns = sum(float(r["TotalDurationNs"]) for r in hit)
        per[k] = {"us_per_step": round(ns / ran / 1e3, 2), "share_of_kernel_time": round(ns / total, 5),
                  "launches": int(sum(float(r.get("Calls", 0) or 0) for r in hit))}
    bwd = per["mhsa_bwd_dq_kernel"]["us_per_step"] + per["mhsa_bwd_dkv_kernel"]["us_per_step"]
    return {"per_kernel": per, "kernels_in_trace": len(rows), "kernel_time_us_per_step": round(total / ran / 1e3, 1),
            "mhsa_bwd_us_per_step": round(bwd, 2),
            "mhsa_bwd_share_of_kernel_time": round((per["mhsa_bwd_dq_kernel"]["share_of_kernel_time"] +
                                                    per["mhsa_bwd_dkv_kernel"]["share_of_kernel_time"]), 5),
            "mhsa_bwd_share_of_step_time": round(bwd / (ms_per_step * 1e3), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile", action="store_true", help="also collect the new kernels' times (rocprofv3, a run of its own)")
    ap.add_argument("--steps-only", action="store_true", help="run compiled steps and exit (the profiled child)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bot3_train needs an MI355X: there is no CPU measurement path")
    dev = torch.device("cuda:0")
    tr, x, lab = make(a, dev)
    if a.steps_only:
        for _ in range(a.steps):
            tr.step(x, lab)
        torch.cuda.synchronize()
        return
    res = {"metric": f"compiled training step of yolov5-BoT3 (n scale) bs {a.batch} {a.imgsz}x{a.imgsz} bf16, ms per step (median of "
                     f"{a.repeats} windows of {a.steps} steps; forward + loss + backward + clip + SGD + EMA)", "batch": a.batch,
           "imgsz": a.imgsz, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    res["bf16_compiled"] = windows(tr, x, lab, a)
    del tr
    if a.profile:
        try:
            res.update(kernel_times(a, res["bf16_compiled"]["ms_per_step"]))
        except (subprocess.SubprocessError, OSError, RuntimeError, KeyError) as e:  # the times above stand; say what is missing
            res["kernel_times"] = f"not measured: {type(e).__name__}: {e}"
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "bot3_train_bench.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
