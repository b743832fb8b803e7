"""Standalone step time of yolov11n detection training (`DetectionTrainer(..., yolo11=True)`): batch 16 at 640 x 640, bf16, the compiled
step (one hipGraph), with `DWConvT.fused` on and off, and - in runs of their own, under the profiler - the share of the step's kernel
time spent in the depthwise kernels of the Detect class branch and in the C2PSA attention backward at 400 tokens.  Separate from
bench.py, whose headline is the detection inference workload; nothing is gated on it.  The default of `DWConvT.fused` follows this A/B
(DESIGN.md section 6), and section 8 quotes the attention backward's share: a matrix-core backward is an open item only above 5 %.

    python -m tools.bench_yolo11_train                 # the A/B; one JSON line, also written to profiles/yolo11_train_bench.json
    python -m tools.bench_yolo11_train --profile       # + per-kernel times: one `rocprofv3 --kernel-trace --stats` run per setting
    python -m tools.bench_yolo11_train --leg fused     # what each child runs: one setting, its windows as one JSON line
    python -m tools.bench_yolo11_train --leg composed --steps-only    # the profiled child: compiled steps, nothing printed

The A/B: every leg is a fresh process on the same box, in the order fused, composed, composed, fused (`--rounds` times), so a drift of
the box falls on both settings alike.  A leg: two eager steps (static buffers, code objects, the optimizer's first step), compile(),
`--warmup` replays, then `--repeats` windows of `--steps` steps each timed with device events.  A setting's figure is the median of all
its windows, with the spread (min, max) next to it.  The labels go up inside the timed window, as in real training.

The depthwise share counts the kernels of dwconv.hip by name.  The composed form's BatchNorm launches are the kernels every other
layer's BatchNorm uses and cannot be told apart in a trace: `kernel_time_us_per_step` of the two settings is the figure that holds them."""

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

from ultralytics_pro_amd.engine import trainer as TR  # noqa: E402
from ultralytics_pro_amd.nn.tasks import DetectionModel  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

DW_KERNELS = ("dwconv3_bn_fwd_kernel", "dwconv3_bn_bwd_kernel", "dwconv3_train_kernel", "dwconv3_wgrad_partial_kernel",
              "dwconv3_wgrad_combine_kernel")
ATTN_BWD = ("psa_bwd_dq_kernel", "psa_bwd_dkv_kernel")
LEGS = ("fused", "composed")


def make(a, dev):
    TR.DWConvT.fused = a.leg == "fused"
    m = DetectionModel("yolov11n.yaml")
    P.apply_procedural_weights(m, family="yolov11n")
    tr = TR.DetectionTrainer(m, dtype=torch.bfloat16, device=dev, yolo11=True)
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
    return dict(windows_ms=[round(v, 4) for v in ms], last_loss_items=[round(float(v), 4) for v in items])


def _child(a, leg, extra=(), prefix=()):
    return list(prefix) + [sys.executable, "-m", "tools.bench_yolo11_train", "--leg", leg, "--batch", str(a.batch), "--imgsz", str(a.imgsz),
                           "--steps", str(a.steps), "--warmup", str(a.warmup), "--repeats", str(a.repeats)] + list(extra)


def ab(a):
    """fused, composed, composed, fused - each a process of its own; the pooled windows of each setting."""
    pool = {k: [] for k in LEGS}
    order, items = [], {}
    for _ in range(a.rounds):
        for leg in ("fused", "composed", "composed", "fused"):
            r = subprocess.run(_child(a, leg), check=True, cwd=str(ROOT), timeout=600, capture_output=True, text=True)
            got = json.loads(r.stdout.strip().splitlines()[-1])
            pool[leg] += got["windows_ms"]
            items[leg] = got["last_loss_items"]
            order.append(leg)
    out = {"order": order}
    for leg, ms in pool.items():
        s = sorted(ms)
        med = s[len(s) // 2]
        out[leg] = dict(ms_per_step=round(med, 4), min=s[0], max=s[-1], windows=len(s), images_per_s=round(a.batch / med * 1e3, 1),
                        last_loss_items=items[leg])
    out["fused_over_composed"] = round(out["fused"]["ms_per_step"] / out["composed"]["ms_per_step"], 4)
    return out


def _hits(rows, k):
    return [r for r in rows if k + "<" in r["Name"] or k + "(" in r["Name"] or r["Name"].endswith(k) or k + " " in r["Name"]]


def kernel_times(a, leg, ms_per_step):
    """Run `--leg LEG --steps-only` under the profiler (a run of its own) and add up the kernel-stats rows of the depthwise kernels and
    of the attention backward."""
    out = ROOT / "profiles" / f"yolo11_train_trace_{leg}"
    prefix = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "--"]
    subprocess.run(_child(a, leg, ("--steps-only",), prefix), check=True, cwd=str(ROOT), timeout=900)
    rows = []
    for f in out.rglob("*kernel_stats.csv"):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    if not rows:
        raise RuntimeError(f"no kernel_stats.csv under {out}")
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    ran = a.warmup + a.steps + 2  # the child's steps: two eager + warmup + steps
    per = {}
    for k in DW_KERNELS + ATTN_BWD:
        hit = _hits(rows, k)
        ns = sum(float(r["TotalDurationNs"]) for r in hit)
        per[k] = {"us_per_step": round(ns / ran / 1e3, 2), "share_of_kernel_time": round(ns / total, 5),
                  "launches": int(sum(float(r.get("Calls", 0) or 0) for r in hit))}
    dw = sum(per[k]["us_per_step"] for k in DW_KERNELS)
    bwd = sum(per[k]["us_per_step"] for k in ATTN_BWD)
    return {"per_kernel": per, "kernels_in_trace": len(rows), "kernel_time_us_per_step": round(total / ran / 1e3, 1),
            "depthwise_us_per_step": round(dw, 2),
            "depthwise_share_of_kernel_time": round(sum(per[k]["share_of_kernel_time"] for k in DW_KERNELS), 5),
            "attention_bwd_us_per_step": round(bwd, 2),
            "attention_bwd_share_of_kernel_time": round(sum(per[k]["share_of_kernel_time"] for k in ATTN_BWD), 5),
            "attention_bwd_share_of_step_time": round(bwd / (ms_per_step * 1e3), 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1, help="how many times the order fused, composed, composed, fused runs")
    ap.add_argument("--profile", action="store_true", help="also collect the kernels' times (rocprofv3, one run per setting)")
    ap.add_argument("--leg", choices=LEGS, help="run one setting in this process (a child of the A/B)")
    ap.add_argument("--steps-only", action="store_true", help="with --leg: run compiled steps and exit (the profiled child)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_yolo11_train needs an MI355X: there is no CPU measurement path")
    if a.leg:
        tr, x, lab = make(a, torch.device("cuda:0"))
        if a.steps_only:
            for _ in range(a.steps):
                tr.step(x, lab)
            torch.cuda.synchronize()
            return
        print(json.dumps(windows(tr, x, lab, a)))
        return
    tokens = (a.imgsz // 32) ** 2
    res = {"metric": f"compiled training step of yolov11n bs {a.batch} {a.imgsz}x{a.imgsz} bf16 ({tokens} tokens in C2PSA), ms per step "
                     f"(median of {2 * a.rounds * a.repeats} windows of {a.steps} steps per setting; forward + loss + backward + clip + SGD + "
                     f"EMA), DWConvT.fused on and off, each leg a fresh process", "batch": a.batch, "imgsz": a.imgsz, "steps": a.steps,
           "warmup": a.warmup, "repeats": a.repeats, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    res.update(ab(a))
    if a.profile:
        for leg in LEGS:
            try:
                res[leg].update(kernel_times(a, leg, res[leg]["ms_per_step"]))
            except (subprocess.SubprocessError, OSError, RuntimeError, KeyError) as e:  # the times above stand; say what is missing
                res[leg]["kernel_times"] = f"not measured: {type(e).__name__}: {e}"
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "yolo11_train_bench.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
