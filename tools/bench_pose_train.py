"""Standalone step time of yolov8n-pose training (`PoseTrainer`): batch 16 at 640 x 640, bf16, the compiled step (one hipGraph), beside
yolov8n DETECTION training (`DetectionTrainer`) at the same batch and size on the same box - the difference is the cost of the pose head
(the padded cv4 chains, the keypoint loss, the pad staging; less the narrower class branch of a one-class head) - and, in a run of its
own under the profiler, the share of the pose step spent in the keypoint loss (the kl_* kernels of csrc/pose_train.hip) and in the pad
gather / scatter launches.  Separate from bench.py, whose headline is the detection inference workload; nothing is gated on it.
DESIGN.md section 8 quotes the two shares: one above 5 % of the step opens a follow-up.

    python -m tools.bench_pose_train                 # pose against det; one JSON line, also written to profiles/pose_train_bench.json
    python -m tools.bench_pose_train --profile       # + per-kernel times of the pose step: one `rocprofv3 --kernel-trace --stats` run
    python -m tools.bench_pose_train --leg pose      # what each child runs: one model, its windows as one JSON line
    python -m tools.bench_pose_train --leg pose --steps-only    # the profiled child: compiled steps, nothing printed

Every leg is a fresh process on the same box, in the order pose, det, det, pose (`--rounds` times), so a drift of the box falls on both
alike.  A leg: two eager steps (static buffers, code objects, the optimizer's first step), compile(), `--warmup` replays, then
`--repeats` windows of `--steps` steps each timed with device events.  A figure is the median of all windows of its model, with the
spread (min, max) next to it.  The labels - for pose with their keypoints, built once on the host - go up inside the timed window, as in
real training."""

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
from ultralytics_pro_amd.nn.tasks import DetectionModel, PoseModel  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

KPT_LOSS = ("kl_compact_kernel", "kl_zero_bg_kernel", "kl_anchor_kernel", "kl_finish_kernel")
PAD_COPY = ("pad_gather_kernel", "pad_scatter_kernel")
LEGS = ("pose", "det")


def keypoints(labels, nkpt=17):
    """(n, nkpt, 3) normalised keypoints from the labels: around each box's centre, up to 0.65 box sizes away, visibility 0 / 1 / 2."""
    bb = labels["bboxes"].view(-1, 4).float()
    u = torch.from_numpy(P.hash_uniform("bench:keypoints", bb.shape[0] * nkpt * 3).reshape(bb.shape[0], nkpt, 3)).float()
    kp = torch.zeros(bb.shape[0], nkpt, 3)
    kp[..., 0] = bb[:, None, 0] + (u[..., 0] - 0.5) * 1.3 * bb[:, None, 2]
    kp[..., 1] = bb[:, None, 1] + (u[..., 1] - 0.5) * 1.3 * bb[:, None, 3]
    kp[..., 2] = (u[..., 2] * 3).floor().clamp(0, 2)
    return kp


def make(a, dev):
    x = P.synthetic_images(a.batch, h=a.imgsz, w=a.imgsz).to(dev)
    lab = P.synthetic_labels(a.batch)
    if a.leg == "pose":
        m = PoseModel("yolov8n-pose.yaml")
        P.apply_procedural_weights(m, family="yolov8n-pose")
        tr = TR.PoseTrainer(m, dtype=torch.bfloat16, device=dev)
        lab["cls"] = torch.zeros_like(lab["cls"])
        lab["keypoints"] = keypoints(lab)
    else:
        m = DetectionModel("yolov8n.yaml")
        P.apply_procedural_weights(m)
        tr = TR.DetectionTrainer(m, dtype=torch.bfloat16, device=dev)
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
    return list(prefix) + [sys.executable, "-m", "tools.bench_pose_train", "--leg", leg, "--batch", str(a.batch), "--imgsz", str(a.imgsz),
                           "--steps", str(a.steps), "--warmup", str(a.warmup), "--repeats", str(a.repeats)] + list(extra)


def ab(a):
    """pose, det, det, pose - each a process of its own; the pooled windows of each model."""
    pool = {k: [] for k in LEGS}
    order, items = [], {}
    for _ in range(a.rounds):
        for leg in ("pose", "det", "det", "pose"):
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
    out["pose_over_det"] = round(out["pose"]["ms_per_step"] / out["det"]["ms_per_step"], 4)
    out["pose_minus_det_ms_per_step"] = round(out["pose"]["ms_per_step"] - out["det"]["ms_per_step"], 4)
    return out


def _hits(rows, k):
    return [r for r in rows if k + "<" in r["Name"] or k + "(" in r["Name"] or r["Name"].endswith(k) or k + " " in r["Name"]]


def kernel_times(a, ms_per_step):
    """Run `--leg pose --steps-only` under the profiler (a run of its own) and add up the kernel-stats rows of the keypoint loss and of
    the pad gather / scatter."""
    out = ROOT / "profiles" / "pose_train_trace"
    prefix = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "--"]
    subprocess.run(_child(a, "pose", ("--steps-only",), prefix), check=True, cwd=str(ROOT), timeout=900)
    rows = []
    for f in out.rglob("*kernel_stats.csv"):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    if not rows:
        raise RuntimeError(f"no kernel_stats.csv under {out}")
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    ran = a.warmup + a.steps + 2  # the child's steps: two eager + warmup + steps
    per = {}
    for k in KPT_LOSS + PAD_COPY:
        hit = _hits(rows, k)
        ns = sum(float(r["TotalDurationNs"]) for r in hit)
        per[k] = {"us_per_step": round(ns / ran / 1e3, 2), "share_of_kernel_time": round(ns / total, 5),
                  "launches": int(sum(float(r.get("Calls", 0) or 0) for r in hit))}
    res = {"per_kernel": per, "kernels_in_trace": len(rows), "kernel_time_us_per_step": round(total / ran / 1e3, 1)}
    for tag, names in (("kpt_loss", KPT_LOSS), ("pad_copy", PAD_COPY)):
        us = sum(per[k]["us_per_step"] for k in names)
        res[f"{tag}_us_per_step"] = round(us, 2)
        res[f"{tag}_share_of_kernel_time"] = round(sum(per[k]["share_of_kernel_time"] for k in names), 5)
        res[f"{tag}_share_of_step_time"] = round(us / (ms_per_step * 1e3), 5)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1, help="how many times the order pose, det, det, pose runs")
    ap.add_argument("--profile", action="store_true", help="also collect the pose step's kernel times (rocprofv3, a run of its own)")
    ap.add_argument("--leg", choices=LEGS, help="run one model in this process (a child of the comparison)")
    ap.add_argument("--steps-only", action="store_true", help="with --leg: run compiled steps and exit (the profiled child)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose_train needs an MI355X: there is no CPU measurement path")
    if a.leg:
        tr, x, lab = make(a, torch.device("cuda:0"))
        if a.steps_only:
            for _ in range(a.steps):
                tr.step(x, lab)
            torch.cuda.synchronize()
            return
        print(json.dumps(windows(tr, x, lab, a)))
        return
    res = {"metric": f"compiled training step of yolov8n-pose (PoseTrainer) and of yolov8n (DetectionTrainer) bs {a.batch} "
                     f"{a.imgsz}x{a.imgsz} bf16, ms per step (median of {2 * a.rounds * a.repeats} windows of {a.steps} steps per model; forward + "
                     f"loss + backward + clip + SGD + EMA), each leg a fresh process", "batch": a.batch, "imgsz": a.imgsz, "steps": a.steps,
           "warmup": a.warmup, "repeats": a.repeats, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    res.update(ab(a))
    if a.profile:
        try:
            res["pose"].update(kernel_times(a, res["pose"]["ms_per_step"]))
        except (subprocess.SubprocessError, OSError, RuntimeError, KeyError) as e:  # the times above stand; say what is missing
            res["pose"]["kernel_times"] = f"not measured: {type(e).__name__}: {e}"
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "pose_train_bench.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
