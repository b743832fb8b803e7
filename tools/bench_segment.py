"""Standalone throughput of instance segmentation: yolov8n-seg (or --model), bf16, forward + NMS + coefficient gather + masks at the
input resolution, captured as ONE graph (`DetectionModel.compile(example, post=segment_postprocess_raw)`) and replayed.  Prints one
JSON line.  Separate from bench.py, which measures the detection workload.

    python -m tools.bench_segment --batch 32 --steps 50 --warmup 10
    python -m tools.bench_segment --val --batch 32 --steps 20 --warmup 3

--val times the validate post-processing of one forward's output two ways, in one process, alternating (A B A B ...):
  fused     val-mode NMS -> coefficient gather -> `upa_segment_match` (bit masks on the chip, TP matrices on the device)
  composed  what the library offered before that kernel: val-mode NMS -> coefficient gather -> `upa_process_mask` byte masks at proto
            resolution -> the reference's float-matmul mask_iou in torch, image by image -> matching on the host
Labels: every third detection's own mask and class (up to 30 per image).
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


def _host_match(iou, pcls, gcls, iouv):
    """match_predictions (engine/validator.py:267-308, non-scipy branch) on the host: iou (M, N) numpy."""
    import numpy as np
    correct = np.zeros((pcls.shape[0], len(iouv)), bool)
    iou = iou * (gcls[:, None] == pcls[None])
    for i, thr in enumerate(iouv.tolist()):
        mt = np.array(np.nonzero(iou >= thr)).T
        if mt.shape[0]:
            if mt.shape[0] > 1:
                mt = mt[iou[mt[:, 0], mt[:, 1]].argsort()[::-1]]
                mt = mt[np.unique(mt[:, 1], return_index=True)[1]]
                mt = mt[np.unique(mt[:, 0], return_index=True)[1]]
            correct[mt[:, 1].astype(int), i] = True
    return correct


def val_leg(a, m, x, dev):
    import time

    import numpy as np

    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.utils import metrics as M
    from ultralytics_pro_amd.utils import ops
    from ultralytics_pro_amd.utils.nms import nms_raw
    b, md = a.batch, a.max_det
    with torch.no_grad():
        preds = m(x)
        y, mc, p = ops._seg_parts(preds, 0)
        pv = ops._protos_nhwc(p)
        nm, mh, mw = int(mc.shape[1]), int(pv.shape[2]), int(pv.shape[3])
        words = M.mask_words(mh * mw)

        def rows_of():
            out, counts, keep = nms_raw(y, 0.001, 0.7, multi_label=True, max_det=md)
            rows = torch.empty((b, md, 6 + nm), dtype=torch.float32, device=dev)
            L.check(L.lib().upa_nms_gather_extra(mc.data_ptr(), b, nm, int(mc.shape[2]), keep.data_ptr(), counts.data_ptr(), md, out.data_ptr(),
                                                 rows.data_ptr(), 6 + nm, L.current_stream(dev)), "nms_gather_extra")
            return rows, counts

        def byte_masks(rows, counts):
            masks = torch.empty((b * md, mh, mw), dtype=torch.uint8, device=dev)
            nonempty = torch.empty((b * md,), dtype=torch.int32, device=dev)
            total = torch.empty((1,), dtype=torch.int32, device=dev)
            ops._launch_process_mask(pv, rows[..., 6:], 6 + nm, rows, 6 + nm, md, counts, (mh, mw), False, (mw / a.imgsz, mh / a.imgsz),
                                     (0, 0, mh, mw), masks, nonempty, b * md, total)
            return masks

        # labels: every third detection's own mask (up to 30 per image), packed once - label preparation is not part of either leg
        rows, counts = rows_of()
        masks = byte_masks(rows, counts)
        cnt = counts.tolist()
        base = np.concatenate([[0], np.cumsum(cnt)]).astype(int)
        sel = [list(range(0, min(cnt[i], 90), 3)) for i in range(b)]
        ngt = torch.tensor([len(s_) for s_ in sel], dtype=torch.int32, device=dev)
        planes = torch.cat([masks[base[i] + torch.tensor(sel[i], dtype=torch.long, device=dev)] for i in range(b) if sel[i]], 0)
        gt = torch.zeros((b, 64, 5), device=dev)
        for i in range(b):
            if sel[i]:
                gt[i, :len(sel[i]), 0] = rows[i, sel[i], 5]
        gt_bits, gt_area = M.pack_mask_bits(planes, b, 64, ngt)
        gt_planes = [planes[int(sum(len(s_) for s_ in sel[:i])):int(sum(len(s_) for s_ in sel[:i + 1]))].flatten(1).float() for i in range(b)]
        iouv = M.IOUV

        def fused():
            r, c = rows_of()
            return M.match_masks_batched(pv, r, c, (a.imgsz, a.imgsz), gt, gt_bits, gt_area, ngt)

        def composed():
            r, c = rows_of()
            bm = byte_masks(r, c)
            n = c.tolist()
            o = np.concatenate([[0], np.cumsum(n)]).astype(int)
            tp = []
            for i in range(b):
                pm = bm[o[i]:o[i + 1]].flatten(1).float()
                g = gt_planes[i]
                inter = torch.matmul(g, pm.T).clamp_(0)  # utils/metrics.py:159-161
                iou = inter / ((g.sum(1)[:, None] + pm.sum(1)[None]) - inter + 1e-7)
                tp.append(_host_match(iou.cpu().numpy(), r[i, :n[i], 5].cpu().numpy(), gt[i, :len(sel[i]), 0].cpu().numpy(), iouv))
            return tp

        t = {"fused": [], "composed": []}
        same = None
        for it in range(a.warmup + a.steps):
            for name, fn in (("fused", fused), ("composed", composed)) if it % 2 == 0 else (("composed", composed), ("fused", fused)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = fn()
                if name == "fused":
                    res = res.cpu()  # the TP matrices on the host, where the composed leg leaves them
                torch.cuda.synchronize()
                if it >= a.warmup:
                    t[name].append((time.perf_counter() - t0) * 1e3)
                if name == "fused":
                    tp_f = res.numpy().astype(bool)
                else:
                    tp_c = res
            same = sum(int((tp_f[i, :cnt[i]] != tp_c[i]).sum()) for i in range(b))
    med = {k: float(np.median(v)) for k, v in t.items()}
    dets = int(sum(cnt))
    print(json.dumps({"metric": f"validate post-processing of {a.model} bs {b} {a.imgsz}x{a.imgsz} bf16: NMS + gather + mask TP, ms per batch (median)",
                      "fused_ms": round(med["fused"], 3), "composed_ms": round(med["composed"], 3), "speedup": round(med["composed"] / med["fused"], 2),
                      "steps": a.steps, "warmup": a.warmup, "detections": dets, "labels": int(ngt.sum()), "tp_entries_that_differ": same,
                      "composed_mask_bytes_written_and_read": 2 * dets * mh * mw, "composed_float_mask_bytes": 4 * dets * mh * mw,
                      "fused_label_bit_bytes": int(ngt.sum()) * words * 4, "fused_mask_bytes": 0}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="yolov8n-seg")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--max-det", type=int, default=300)
    ap.add_argument("--capacity", type=int, default=2048, help="rows of the ragged mask buffer (masks past it are reported, not written)")
    ap.add_argument("--val", action="store_true", help="time the fused validate post-processing against the composed one")
    ap.add_argument("--family", default=None, help="procedural weight family (default: the model's; 'smooth:<model>' for the smooth one)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    m = SegmentationModel(a.model + ".yaml")
    P.apply_procedural_weights(m, family=a.family)
    m = m.to(dev).eval()
    m.set_compute_dtype(torch.bfloat16)
    m.model[-1].cat_out = False  # the postprocess reads y, mc and the protos directly
    x = P.synthetic_images(a.batch, h=a.imgsz, w=a.imgsz).to(dev).to(torch.bfloat16).contiguous()
    if a.val:
        return val_leg(a, m, x, dev)
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
