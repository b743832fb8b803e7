"""Standalone step time of classification training: yolov8n-cls, batch 32 at 224 x 224, bf16 and f32, eager and compiled (one
hipGraph per step), and - in a run of its own, under the profiler - the share of the four kernels of csrc/classify_train.hip in the
step.  Separate from bench.py, whose headline is the detection workload; no earlier number exists for this one and nothing is gated
on it.

    python -m tools.bench_classify_train                       # times; one JSON line, also written to profiles/classify_train_bench.json
    python -m tools.bench_classify_train --profile             # + kernel shares: re-runs itself under `rocprofv3 --kernel-trace --stats`
    python -m tools.bench_classify_train --steps-only bf16     # what the profiled child runs: compiled bf16 steps, nothing printed

Timing: every mode is warmed (the first steps allocate the static buffers and load code objects; compile() needs one eager step),
then `--repeats` windows of `--steps` steps each are timed with device events on the trainer's stream; the median window is reported
with the spread (min, max) next to it.  The labels go up inside the timed window, as in real training.

    python -m tools.bench_classify_train --optimizer AdamW [--profile]   # -> profiles/classify_train_adamw_bench.json
`--optimizer Adam | AdamW` (default SGD: output unchanged) times the compiled step under that optimizer AND under SGD in the same
process, the windows of the two alternating (SGD, AdamW, SGD, ...), and with --profile adds the optimizer kernels' own time from a
kernel trace of each (runs of their own) with the bandwidth they reach: bytes per parameter (SGD 32: p, g, momentum, EMA read and
written; Adam 40: + exp_avg_sq) x parameters over the kernel time of one step's three group launches."""

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

from ultralytics_pro_amd.engine.trainer import ClassificationTrainer  # noqa: E402
from ultralytics_pro_amd.nn.tasks import ClassificationModel  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

NEW_KERNELS = ("avgpool_fwd_kernel", "avgpool_bwd_kernel", "cross_entropy_rows_kernel", "cross_entropy_mean_kernel", "linear_wgrad_kernel",
               "linear_dgrad_kernel")
# --model yolov11n-cls: the kernels only C2PSA's training path launches (csrc/psa.hip, csrc/dwconv.hip)
YOLO11_KERNELS = ("psa_attn_kernel", "psa_attn_mfma_kernel", "psa_bwd_dq_kernel", "psa_bwd_dkv_kernel", "dwconv3_train_kernel",
                  "dwconv3_wgrad_partial_kernel", "dwconv3_wgrad_combine_kernel")


OPT_KERNELS = {"SGD": ("sgd_nesterov_ema_kernel", 32), "Adam": ("adam_ema_kernel", 40), "AdamW": ("adam_ema_kernel", 40)}


def out_name(model, optimizer="SGD"):
    """profiles/classify_train_bench.json for the default model (unchanged), profiles/classify_train11_bench.json for yolov11n-cls;
    profiles/classify_train_adamw_bench.json (..._adam_...) for the optimizer comparison."""
    if optimizer != "SGD":
        return f"classify_train_{optimizer.lower()}_bench.json"
    return "classify_train_bench.json" if model == "yolov8n-cls" else f"classify_train{model.replace('yolov', '').replace('n-cls', '')}_bench.json"


def make(a, dtype, dev, optimizer="SGD"):
    m = ClassificationModel(a.model + ".yaml", nc=a.nc)
    P.apply_procedural_weights(m, family=a.model)
    kw = {} if optimizer == "SGD" else dict(optimizer=optimizer, hyp=dict(lr=round(0.002 * 5 / (4 + a.nc), 6)))  # auto's lr for nc
    tr = ClassificationTrainer(m, dtype=dtype, device=dev, yolo11="11" in a.model, **kw)
    x = P.synthetic_images(a.batch, h=a.imgsz, w=a.imgsz).to(dev)
    cls = (P.uniform("bench:cls", (a.batch,), 0.0, 1.0) * a.nc).long().clamp_(0, a.nc - 1)
    return tr, x, {"cls": cls}


def windows(tr, x, lab, a):
    for _ in range(a.warmup):
        tr.step(x, lab)
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            loss = tr.step(x, lab)
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1) / a.steps)
    ms.sort()
    return dict(ms_per_step=round(ms[len(ms) // 2], 4), min=round(ms[0], 4), max=round(ms[-1], 4), last_loss=round(float(loss[0]), 5))


def compare_optimizers(a, dev):
    """Compiled steps under SGD and under a.optimizer, both trainers alive, their timed windows alternating."""
    res = {}
    for name, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        trs = {}
        for opt in ("SGD", a.optimizer):
            tr, x, lab = make(a, dtype, dev, opt)
            tr.step(x, lab)
            tr.compile(x, lab, warm_steps=0)
            for _ in range(a.warmup):
                tr.step(x, lab)
            trs[opt] = tr
        torch.cuda.synchronize()
        ms = {opt: [] for opt in trs}
        for _ in range(a.repeats):
            for opt, tr in trs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.steps):
                    tr.step(x, lab)
                t1.record()
                torch.cuda.synchronize()
                ms[opt].append(t0.elapsed_time(t1) / a.steps)
        for opt, v in ms.items():
            v.sort()
            res[f"{name}_compiled_{opt}"] = dict(ms_per_step=round(v[len(v) // 2], 4), min=round(v[0], 4), max=round(v[-1], 4))
        res["parameters"] = int(trs["SGD"].groups[-1][0] + trs["SGD"].groups[-1][1])
        del trs
    return res


def optimizer_kernel_time(a, optimizer, nparams):
    """Kernel time of the optimizer's update kernel per step, from a kernel trace of compiled bf16 steps (a run of its own), and the
    bandwidth that is: bytes per parameter x parameters / time of one step's group launches."""
    out = ROOT / "profiles" / "classify_train_trace" / optimizer.lower()
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "--", sys.executable, "-m",
           "tools.bench_classify_train", "--model", a.model, "--steps-only", "bf16", "--optimizer", optimizer, "--batch", str(a.batch),
           "--imgsz", str(a.imgsz), "--nc", str(a.nc), "--steps", str(a.steps), "--warmup", str(a.warmup)]
    subprocess.run(cmd, check=True, cwd=str(ROOT), timeout=600)
    kname, nbytes = OPT_KERNELS[optimizer]
    ns = calls = 0.0
    for f in out.rglob("*kernel_stats.csv"):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                if kname in r["Name"]:
                    ns += float(r["TotalDurationNs"])
                    calls += float(r.get("Calls", 0) or 0)
    if not calls:
        raise RuntimeError(f"no {kname} row in the kernel trace under {out}")
    steps = calls / 3  # three group launches per optimizer step
    us = ns / steps / 1e3
    return {"kernel": kname, "launches": int(calls), "us_per_step": round(us, 2), "bytes_per_parameter": nbytes,
            "GB_per_s": round(nbytes * nparams / (us * 1e-6) / 1e9, 1)}


def kernel_shares(a):
    """Run `--steps-only bf16` under the profiler (a run of its own) and add up the kernel-stats rows."""
    out = ROOT / "profiles" / "classify_train_trace"
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "--", sys.executable, "-m",
           "tools.bench_classify_train", "--model", a.model, "--steps-only", "bf16", "--batch", str(a.batch), "--imgsz", str(a.imgsz), "--nc", str(a.nc),
           "--steps", str(a.steps), "--warmup", str(a.warmup)]
    subprocess.run(cmd, check=True, cwd=str(ROOT), timeout=600)
    rows = []
    for f in out.rglob("*kernel_stats.csv"):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    if not rows:
        raise RuntimeError(f"no kernel_stats.csv under {out}")
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    names = NEW_KERNELS + (YOLO11_KERNELS if "11" in a.model else ())
    new = {k: 0.0 for k in names}
    for r in rows:
        for k in names:
            if k + "<" in r["Name"] or k + "(" in r["Name"] or r["Name"].endswith(k) or k + " " in r["Name"]:
                new[k] += float(r["TotalDurationNs"])
    res = {"kernel_time_share_of_new_kernels": round(sum(new.values()) / total, 5),
           "per_kernel_share": {k: round(v / total, 5) for k, v in new.items()}, "kernels_in_trace": len(rows)}
    calls = sum(int(float(r.get("Calls", 0) or 0)) for r in rows)
    ran = a.warmup + a.steps + 3  # the child's steps: one eager + compile(warm_steps=2) + warmup + steps
    res["kernel_launches_per_step"] = round(calls / ran, 1)  # trace-wide calls / steps the child ran (the one-time packing included)
    if "11" in a.model:
        res["kernel_time_share_of_attention_bwd"] = round((new["psa_bwd_dq_kernel"] + new["psa_bwd_dkv_kernel"]) / total, 5)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="yolov8n-cls")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=224)
    ap.add_argument("--nc", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--profile", action="store_true", help="also collect the new kernels' share of the step (rocprofv3, a run of its own)")
    ap.add_argument("--optimizer", default="SGD", choices=["SGD", "Adam", "AdamW"], help="Adam / AdamW: compare the compiled step with SGD's")
    ap.add_argument("--steps-only", default=None, choices=["bf16", "f32"], help="run compiled steps and exit (the profiled child)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_classify_train needs an MI355X: there is no CPU measurement path")
    dev = torch.device("cuda:0")
    if a.steps_only:
        tr, x, lab = make(a, torch.bfloat16 if a.steps_only == "bf16" else torch.float32, dev, a.optimizer)
        tr.compile(x, lab, warm_steps=2)
        for _ in range(a.warmup + a.steps):
            tr.step(x, lab)
        torch.cuda.synchronize()
        return
    if a.optimizer != "SGD":
        res = {"metric": f"compiled training step of {a.model} nc {a.nc} bs {a.batch} {a.imgsz}x{a.imgsz} under SGD and {a.optimizer}, ms per "
                         f"step (median of {a.repeats} alternating windows of {a.steps} steps; forward + loss + backward + clip + optimizer "
                         "+ EMA)", "optimizer": a.optimizer, "batch": a.batch, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
        res.update(compare_optimizers(a, dev))
        if a.profile:
            for opt in ("SGD", a.optimizer):
                try:
                    res[f"optimizer_kernel_{opt}"] = optimizer_kernel_time(a, opt, res["parameters"])
                except (subprocess.SubprocessError, OSError, RuntimeError, KeyError) as e:
                    res[f"optimizer_kernel_{opt}"] = f"not measured: {type(e).__name__}: {e}"
        line = json.dumps(res)
        (ROOT / "profiles").mkdir(exist_ok=True)
        (ROOT / "profiles" / out_name(a.model, a.optimizer)).write_text(line + "\n")
        print(line)
        return
    res = {"metric": f"training step of {a.model} nc {a.nc} bs {a.batch} {a.imgsz}x{a.imgsz}, ms per step (median of {a.repeats} windows of "
                     f"{a.steps} steps; forward + loss + backward + clip + SGD + EMA)", "batch": a.batch, "steps": a.steps,
           "warmup": a.warmup, "repeats": a.repeats}
    for name, dtype in (("bf16", torch.bfloat16), ("f32", torch.float32)):
        tr, x, lab = make(a, dtype, dev)
        res[f"{name}_eager"] = windows(tr, x, lab, a)
        tr.compile(x, lab, warm_steps=0)
        res[f"{name}_compiled"] = windows(tr, x, lab, a)
        res[f"{name}_compiled"]["images_per_s"] = round(a.batch / res[f"{name}_compiled"]["ms_per_step"] * 1e3, 1)
        del tr
    if a.profile:
        try:
            res.update(kernel_shares(a))
        except (subprocess.SubprocessError, OSError, RuntimeError, KeyError) as e:  # the times above stand; say what is missing
            res["kernel_shares"] = f"not measured: {type(e).__name__}: {e}"
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / out_name(a.model)).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
