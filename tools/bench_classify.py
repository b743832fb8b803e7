"""Standalone throughput of image classification: yolov8n-cls and yolov11n-cls at batch 32, 224 x 224, f32 (parity mode) and bf16
(perf mode).  Per model and mode: the eager step one at a time, and several steps in flight through the graph executor
(`engine.pipeline.PipelinedRunner`: one hipGraph per copy, replayed round-robin on separate streams).  Plus the head's
`upa_classify_pool` launch alone (the model's own shape) against its HBM roofline, bytes = input + packed weights + pooled output.
Prints one JSON line.  Separate from bench.py, which measures the detection workload; there is no earlier number and no time gate.

    python -m tools.bench_classify --steps 50 --warmup 10
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from ultralytics_pro_amd import _lib as L  # noqa: E402
from ultralytics_pro_amd.engine import runtime as R  # noqa: E402
from ultralytics_pro_amd.engine.pipeline import PipelinedRunner  # noqa: E402
from ultralytics_pro_amd.nn.tasks import ClassificationModel  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM3E bandwidth


def pool_launch_us(head, n, hw, dtype, dev, steps, warmup):
    """Mean time (us) of `upa_classify_pool` alone on the head's shape, and its byte count."""
    cv = head.conv
    cin, cout = cv.conv.in_channels, cv.conv.out_channels
    pk = cv._packed(cv.conv, cv.bn, dev, dtype, False)
    x = torch.rand((n, hw[0], hw[1], cin), device=dev).to(dtype)
    out = torch.empty((n, cout), dtype=torch.float32, device=dev)
    st = L.current_stream(dev)
    call = lambda: L.check(L.lib().upa_classify_pool(x.data_ptr(), n, hw[0], hw[1], cin, cin, pk.w.data_ptr(), pk.bias.data_ptr(),  # noqa: E731
                                                     out.data_ptr(), cout, cout, L.ACT_SILU, L.dtype_code(dtype), None, st), "classify_pool")
    for _ in range(warmup):
        call()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        call()
    t1.record()
    torch.cuda.synchronize()
    nbytes = x.numel() * x.element_size() + pk.w.numel() + out.numel() * 4
    return t0.elapsed_time(t1) / steps * 1e3, nbytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="yolov8n-cls,yolov11n-cls")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=224)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--in-flight", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    for name in a.models.split(","):
        for dtype, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
            m = ClassificationModel(name + ".yaml")
            P.apply_procedural_weights(m)
            m = m.to(dev).eval()
            m.set_compute_dtype(dtype)
            x = P.synthetic_images(a.batch, h=a.imgsz, w=a.imgsz).to(dev).to(dtype).contiguous()
            with torch.no_grad():
                for _ in range(a.warmup):
                    m(x)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    m(x)
                torch.cuda.synchronize()
                eager = (time.perf_counter() - t0) / a.steps
                runner = PipelinedRunner(m, x, micro_batches=1, in_flight=a.in_flight, linear=True)
                flight = runner.measure(a.steps, a.warmup)
                hw = (a.imgsz // 32, a.imgsz // 32)
                us, nbytes = pool_launch_us(m.model[-1], a.batch, hw, dtype, dev, a.steps, a.warmup)
            roof = nbytes / HBM_BYTES_PER_S * 1e6
            res[f"{name}/{tag}"] = {"eager_ms_per_step": round(eager * 1e3, 4), "eager_images_per_s": round(a.batch / eager, 1),
                                    "in_flight_ms_per_step": round(flight * 1e3, 4), "in_flight_images_per_s": round(a.batch / flight, 1),
                                    "classify_pool_us": round(us, 2), "classify_pool_bytes": nbytes,
                                    "classify_pool_hbm_roofline_us": round(roof, 3), "classify_pool_roofline_share": round(roof / us, 4)}
            del runner, m
    print(json.dumps({"metric": f"image classification bs {a.batch} {a.imgsz}x{a.imgsz}: eager serial and {a.in_flight} graph copies in flight",
                      "unit": "images/s", "batch": a.batch, "imgsz": a.imgsz, "steps": a.steps, "warmup": a.warmup, "in_flight": a.in_flight,
                      "results": res}))


if __name__ == "__main__":
    main()
