"""Standalone step time of yolov8n-seg training (`SegmentationTrainer`): batch 16 at 640 x 640, bf16, the compiled step (one hipGraph),
beside yolov8n DETECTION training (`DetectionTrainer`) at the same batch and size on the same box - the difference is the cost of the seg
head (cv4 chains, Proto, the mask loss) - and, in a run of its own under the profiler, the share of the seg step spent in the mask loss
(the ml_* kernels of csrc/segment_train.hip) and in the ConvTranspose backward (convt2x2_dgrad / _wgrad / _wgrad_combine).  Separate from
bench.py, whose headline is the detection inference workload; nothing is gated on it.  DESIGN.md section 8 quotes the two shares: a
kernel above 5 % of the step opens a follow-up.

    python -m tools.bench_segment_train                 # seg against det; one JSON line, also written to profiles/segment_train_bench.json
    python -m tools.bench_segment_train --profile       # + per-kernel times of the seg step: one `rocprofv3 --kernel-trace --stats` run
    python -m tools.bench_segment_train --leg seg       # what each child runs: one model, its windows as one JSON line
    python -m tools.bench_segment_train --leg seg --steps-only    # the profiled child: compiled steps, nothing printed

Every leg is a fresh process on the same box, in the order seg, det, det, seg (`--rounds` times), so a drift of the box falls on both
alike.  A leg: two eager steps (static buffers, code objects, the optimizer's first step), compile(), `--warmup` replays, then
`--repeats` windows of `--steps` steps each timed with device events.  A figure is the median of all windows of its model, with the
spread (min, max) next to it.  The labels - and for seg the overlap masks, built once on the host - go up inside the timed window, as in
real training.  The bias gradient of the ConvTranspose runs in the channel-sum kernels every plain conv's bias gradient uses and cannot
be told apart in a trace; it is not in the ConvTranspose figure."""

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
from ultralytics_pro_amd.nn.tasks import DetectionModel, SegmentationModel  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

MASK_LOSS = ("ml_compact_kernel", "ml_zero_bg_kernel", "ml_anchor_kernel", "ml_proto_kernel", "ml_finish_kernel")
CONVT_BWD = ("convt2x2_dgrad_kernel", "convt2x2_wgrad_kernel", "convt2x2_wgrad_combine_kernel")
CONVT_FWD = ("convt2x2_kernel", "convt2x2_pack_kernel")
LEGS = ("seg", "det")


def overlap_masks(labels, batch_size, mh, mw):
    """(B, mh, mw) uint8 overlap mask from the labels: instance p of an image is an ellipse inscribed in its box, painted as p + 1, later
    instances over earlier ones."""
    bi = labels["batch_idx"].view(-1).long()
    bb = labels["bboxes"].view(-1, 4).float()
    ys = (torch.arange(mh, dtype=torch.float32) + 0.5).view(-1, 1) / mh
    xs = (torch.arange(mw, dtype=torch.float32) + 0.5).view(1, -1) / mw
    out = torch.zeros(batch_size, mh, mw, dtype=torch.uint8)
    for j in range(batch_size):
        for p, i in enumerate((bi == j).nonzero().view(-1).tolist()):
            cx, cy, w, h = (float(v) for v in bb[i])
            if w > 0 and h > 0:
                out[j][((xs - cx) / (w / 2)) ** 2 + ((ys - cy) / (h / 2)) ** 2 <= 1.0] = p + 1
    return out


def make(a, dev):
    x = P.synthetic_images(a.batch, h=a.imgsz, w=a.imgsz).to(dev)
    lab = P.synthetic_labels(a.batch)
    if a.leg == "seg":
        m = SegmentationModel("yolov8n-seg.yaml")
        P.apply_procedural_weights(m, family="yolov8n-seg")
        tr = TR.SegmentationTrainer(m, dtype=torch.bfloat16, device=dev)
        lab["masks"] = overlap_masks(lab, a.batch, a.imgsz // 4, a.imgsz // 4)
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
    return list(prefix) + [sys.executable, "-m", "tools.bench_segment_train", "--leg", leg, "--batch", str(a.batch), "--imgsz", str(a.imgsz),
                           "--steps", str(a.steps), "--warmup", str(a.warmup), "--repeats", str(a.repeats)] + list(extra)


def ab(a):
    """seg, det, det, seg - each a process of its own; the pooled windows of each model."""
    pool = {k: [] for k in LEGS}
    order, items = [], {}
    for _ in range(a.rounds):
        for leg in ("seg", "det", "det", "seg"):
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
    out["seg_over_det"] = round(out["seg"]["ms_per_step"] / out["det"]["ms_per_step"], 4)
    out["seg_head_ms_per_step"] = round(out["seg"]["ms_per_step"] - out["det"]["ms_per_step"], 4)
    return out


def _hits(rows, k):
    return [r for r in rows if k + "<" in r["Name"] or k + "(" in r["Name"] or r["Name"].endswith(k) or k + " " in r["Name"]]


def kernel_times(a, ms_per_step):
    """Run `--leg seg --steps-only` under the profiler (a run of its own) and add up the kernel-stats rows of the mask loss and of the
    ConvTranspose backward."""
    out = ROOT / "profiles" / "segment_train_trace"
    prefix = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", str(out), "--"]
    subprocess.run(_child(a, "seg", ("--steps-only",), prefix), check=True, cwd=str(ROOT), timeout=900)
    rows = []
    for f in out.rglob("*kernel_stats.csv"):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    if not rows:
        raise RuntimeError(f"no kernel_stats.csv under {out}")
    total = sum(float(r["TotalDurationNs"]) for r in rows)
    ran = a.warmup + a.steps + 2  # the child's steps: two eager + warmup + steps
    per = {}
    for k in MASK_LOSS + CONVT_BWD + CONVT_FWD:
        hit = _hits(rows, k)
        ns = sum(float(r["TotalDurationNs"]) for r in hit)
        per[k] = {"us_per_step": round(ns / ran / 1e3, 2), "share_of_kernel_time": round(ns / total, 5),
                  "launches": int(sum(float(r.get("Calls", 0) or 0) for r in hit))}
    res = {"per_kernel": per, "kernels_in_trace": len(rows), "kernel_time_us_per_step": round(total / ran / 1e3, 1)}
    for tag, names in (("mask_loss", MASK_LOSS), ("conv_transpose_bwd", CONVT_BWD)):
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
    ap.add_argument("--rounds", type=int, default=1, help="how many times the order seg, det, det, seg runs")
    ap.add_argument("--profile", action="store_true", help="also collect the seg step's kernel times (rocprofv3, a run of its own)")
    ap.add_argument("--leg", choices=LEGS, help="run one model in this process (a child of the comparison)")
    ap.add_argument("--steps-only", action="store_true", help="with --leg: run compiled steps and exit (the profiled child)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_segment_train needs an MI355X: there is no CPU measurement path")
    if a.leg:
        tr, x, lab = make(a, torch.device("cuda:0"))
        if a.steps_only:
            for _ in range(a.steps):
                tr.step(x, lab)
            torch.cuda.synchronize()
            return
        print(json.dumps(windows(tr, x, lab, a)))
        return
    res = {"metric": f"compiled training step of yolov8n-seg (SegmentationTrainer) and of yolov8n (DetectionTrainer) bs {a.batch} "
                     f"{a.imgsz}x{a.imgsz} bf16, ms per step (median of {2 * a.rounds * a.repeats} windows of {a.steps} steps per model; forward + "
                     f"loss + backward + clip + SGD + EMA), each leg a fresh process", "batch": a.batch, "imgsz": a.imgsz, "steps": a.steps,
           "warmup": a.warmup, "repeats": a.repeats, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    res.update(ab(a))
    if a.profile:
        try:
            res["seg"].update(kernel_times(a, res["seg"]["ms_per_step"]))
        except (subprocess.SubprocessError, OSError, RuntimeError, KeyError) as e:  # the times above stand; say what is missing
            res["seg"]["kernel_times"] = f"not measured: {type(e).__name__}: {e}"
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "segment_train_bench.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
