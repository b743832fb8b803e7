"""Standalone throughput of instance segmentation: yolov8n-seg (or --model), bf16, forward + NMS + coefficient gather + masks at the
input resolution, captured as ONE graph (`DetectionModel.compile(example, post=segment_postprocess_raw)`) and replayed.  Prints one
JSON line.  Separate from bench.py, which measures the detection workload.

    python -m tools.bench_segment --batch 32 --steps 50 --warmup 10
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from ultralytics_pro_amd.nn.tasks import SegmentationModel  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402
from ultralytics_pro_amd.utils.ops import segment_postprocess_raw  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="yolov8n-seg")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--max-det", type=int, default=300)
    ap.add_argument("--capacity", type=int, default=2048, help="rows of the ragged mask buffer (masks past it are reported, not written)")
    ap.add_argument("--family", default=None, help="procedural weight family (default: the model's; 'smooth:<model>' for the smooth one)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = SegmentationModel(a.model + ".yaml")
    P.apply_procedural_weights(m, family=a.family)
    m = m.to(dev).eval()
    m.set_compute_dtype(torch.bfloat16)
    m.model[-1].cat_out = False  # the postprocess reads y, mc and the protos directly
    x = P.synthetic_images(a.batch, h=a.imgsz, w=a.imgsz).to(dev).to(torch.bfloat16).contiguous()
    post = lambda o: segment_postprocess_raw(o, 0.25, 0.7, max_det=a.max_det, imgsz=(a.imgsz, a.imgsz), capacity=a.capacity,  # noqa: E731
                                             key="bench_seg")
    with torch.no_grad():
        run = m.compile(x, post=post)
        for _ in range(a.warmup):
            run()
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            res = run()
        t1.record()
        torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.steps
    total = int(res["total"].item())
    print(json.dumps({"metric": f"images/sec {a.model} {a.imgsz}x{a.imgsz} bf16 (forward + NMS + masks at {a.imgsz}x{a.imgsz}, one graph)",
                      "value": round(a.batch / ms * 1e3, 1), "unit": "images/s", "batch": a.batch, "steps": a.steps, "warmup": a.warmup,
                      "ms_per_step": round(ms, 4), "masks_per_step": total, "capacity": a.capacity, "overflow": total > a.capacity}))


if __name__ == "__main__":
    main()
