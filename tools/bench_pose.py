"""Standalone throughput of pose estimation: yolov8n-pose, bf16, bs 32 at 640 x 640, forward + NMS + keypoint gather
(`PoseModel.compile(example, post=pose_postprocess_raw)`, one graph, replayed), beside yolov8n DETECTION (forward + NMS, one graph) at
the same batch and size on the same box; a validation step (`--val`: forward + `PoseValidator.update`, one graph); and the time of the
three kernels of csrc/pose.hip at the step's shapes, as a share of the step they run in.  Separate from bench.py, whose headline is
the detection workload; nothing is gated on it.  DESIGN.md sections 6 and 8 quote the numbers: a first collection.

    python -m tools.bench_pose                  # pose against det + kernels; one JSON line, also written to profiles/pose_bench.json
    python -m tools.bench_pose --val            # + the validation step
    python -m tools.bench_pose --leg pose       # what each child runs: one workload, its windows as one JSON line

Every leg is a fresh process on the same box, in the order pose, det, det, pose (`--rounds` times), then val and kernels, so a drift
of the box falls on both models alike.  A leg: compile(), `--warmup` replays, then `--repeats` windows of `--steps` replays, each
timed with device events.  A figure is the median of all windows of its workload, with the spread (min, max) next to it.

The kernels leg times each new kernel ALONE, back to back on one stream (`--kernel-iters` launches between two events), at the shapes
of the step: `upa_kpt_decode_rows` on the three levels of a bs 32 bf16 forward (80 x 80, 40 x 40, 20 x 20; 56 channels), three
launches; `upa_scale_coords` on (32, 300, 57) rows and `upa_pose_match` on the same rows against 30 labels per image, both with every
row counted (counts = max_det: the most they can cost).  A share is that time over the step's; back-to-back launches of one kernel
hide no launch gap and keep its code hot, so the shares are estimates from below for the launch cost and from above for the rows.
The validation labels are every third detection of the model's own output (up to 30 per image), built once."""

from __future__ import annotations

import argparse
import json
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from ultralytics_pro_amd.nn.tasks import DetectionModel, PoseModel  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

LEGS = ("pose", "det", "val", "kernels")
NK, KSHAPE = 51, (17, 3)


def _events(fn, n):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(n):
        res = fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / n, res


def _windows(run, a):
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    ms, res = [], None
    for _ in range(a.repeats):
        t, res = _events(run, a.steps)
        ms.append(round(t, 4))
    return ms, res


def _pose_model(dev):
    m = PoseModel("yolov8n-pose.yaml")
    P.apply_procedural_weights(m, family="yolov8n-pose")
    m = m.to(dev).eval()
    m.set_compute_dtype(torch.bfloat16)
    return m


def _labels_from(rows, counts, dev, per_image=30, max_gt=64):
    """Every third detection (up to `per_image`) as a label: its class, box and keypoints, all keypoints visible."""
    b = rows.shape[0]
    cnt = counts.tolist()
    gt, gk = torch.zeros(b, max_gt, 5, device=dev), torch.zeros(b, max_gt, KSHAPE[0], 3, device=dev)
    ngt = []
    for i in range(b):
        sel = list(range(0, min(cnt[i], 3 * per_image), 3))
        ngt.append(len(sel))
        if sel:
            gt[i, :len(sel), 0], gt[i, :len(sel), 1:] = rows[i, sel, 5], rows[i, sel, :4]
            gk[i, :len(sel)] = rows[i, sel, 6:].reshape(len(sel), KSHAPE[0], 3)
            gk[i, :len(sel), :, 2] = 2.0
    return gt, torch.tensor(ngt, dtype=torch.int32, device=dev), gk


def leg_pose(a, dev):
    from ultralytics_pro_amd.utils.ops import pose_postprocess_raw
    m = _pose_model(dev)
    m.model[-1].cat_out = False  # the postprocess reads y and the decoded keypoints directly
    x = P.synthetic_images(a.batch, h=a.imgsz, w=a.imgsz).to(dev).to(torch.bfloat16).contiguous()
    with torch.no_grad():
        # procedural weights at nc = 1 put few scores above 0.25: then the threshold that leaves some 60 candidates per image, about
        # what the detection leg's NMS is given, so that NMS and the gather have work to do
        sc = m(x)[0][:, 4].float().flatten()
        conf = a.conf
        if int((sc > conf).sum()) < 20 * a.batch:
            top = sc.topk(60 * a.batch + 1).values
            conf = float((top[-1] + top[-2]) / 2)
        run = m.compile(x, post=lambda o: pose_postprocess_raw(o, conf, 0.7, max_det=a.max_det, key="bench_pose"))
        ms, res = _windows(run, a)
    return dict(windows_ms=ms, detections=int(res[1].sum().item()), conf_thres=round(conf, 6))


def leg_det(a, dev):
    from ultralytics_pro_amd.utils.nms import nms_raw
    m = DetectionModel("yolov8n.yaml")
    P.apply_procedural_weights(m)
    m = m.to(dev).eval()
    m.set_compute_dtype(torch.bfloat16)
    x = P.synthetic_images(a.batch, h=a.imgsz, w=a.imgsz).to(dev).to(torch.bfloat16).contiguous()
    with torch.no_grad():
        run = m.compile(x, post=lambda o: nms_raw(o[0], 0.25, 0.7, max_det=a.max_det, key="bench_det"))
        ms, res = _windows(run, a)
    return dict(windows_ms=ms, detections=int(res[1].sum().item()))


def leg_val(a, dev):
    from ultralytics_pro_amd.engine.validator import PoseValidator
    from ultralytics_pro_amd.utils.ops import pose_postprocess_raw
    m = _pose_model(dev)
    x = P.synthetic_images(a.batch, h=a.imgsz, w=a.imgsz).to(dev).to(torch.bfloat16).contiguous()
    v = PoseValidator(m, max_det=a.max_det)
    with torch.no_grad():
        rows, counts, _ = pose_postprocess_raw(m(x), v.conf, v.iou, max_det=a.max_det, multi_label=True)
        torch.cuda.synchronize()
        gt, ngt, gk = _labels_from(rows.float(), counts, dev)
        run = m.compile(x, post=lambda o: v.update(o, gt, ngt, gk, key="bench_poseval", record=False))
        ms, res = _windows(run, a)
    return dict(windows_ms=ms, detections=int(res[1].sum().item()), labels=int(ngt.sum().item()),
                pose_tp_at_50=int(res[3][..., 0].sum().item()))


def leg_kernels(a, dev):
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.utils import metrics as M
    lib, stream, b, md = L.lib(), L.current_stream(dev), a.batch, a.max_det
    levels = [(a.imgsz // s, a.imgsz // s, float(s)) for s in (8, 16, 32)]
    a_total = sum(h * w for h, w, _ in levels)
    xs = [P.uniform(f"bench:pose:kpt:{h}", (b, h, w, 56), -4.0, 4.0).to(dev).to(torch.bfloat16).contiguous() for h, w, _ in levels]
    out = torch.empty((b, NK, a_total), dtype=torch.float32, device=dev)
    code = L.dtype_code(torch.bfloat16)

    def decode():
        a0 = 0
        for x, (h, w, s) in zip(xs, levels):
            L.check(lib.upa_kpt_decode_rows(x.data_ptr(), b, h, w, 56, 56, code, KSHAPE[0], KSHAPE[1], s, out.data_ptr(), a_total, a0, None,
                                            stream), "kpt_decode_rows")
            a0 += h * w

    rows = torch.zeros((b, md, 6 + NK), device=dev)
    rows[..., :2] = P.uniform("bench:pose:xy", (b, md, 2), 0.0, 500.0).to(dev)
    rows[..., 2:4] = rows[..., :2] + P.uniform("bench:pose:wh", (b, md, 2), 20.0, 140.0).to(dev)
    rows[..., 4] = 0.5
    rows[..., 6:] = P.uniform("bench:pose:k", (b, md, NK), 0.0, 640.0).to(dev)
    counts = torch.full((b,), md, dtype=torch.int32, device=dev)
    gt, ngt, gk = _labels_from(rows, counts, dev)
    scaled = rows.clone()

    def scale():
        L.check(lib.upa_scale_coords(scaled.data_ptr(), b, md, 6 + NK, 6, KSHAPE[0], KSHAPE[1], counts.data_ptr(), 1.0, 0.0, 80.0, 1, 640.0,
                                     480.0, stream), "scale_coords")

    def match():
        return M.match_keypoints_batched(rows, counts, gt, ngt, gk, KSHAPE, M.OKS_SIGMA, key="bench_pose_match")

    res = {}
    for name, fn in (("kpt_decode_rows_x3", decode), ("scale_coords", scale), ("pose_match", match)):
        _events(fn, 20)
        res[name + "_us"] = round(sorted(_events(fn, a.kernel_iters)[0] for _ in range(5))[2] * 1e3, 2)
    return res


def _child(a, leg):
    return [sys.executable, "-m", "tools.bench_pose", "--leg", leg, "--batch", str(a.batch), "--imgsz", str(a.imgsz), "--steps", str(a.steps),
            "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--max-det", str(a.max_det), "--conf", str(a.conf),
            "--kernel-iters", str(a.kernel_iters)]


def _run_child(a, leg):
    r = subprocess.run(_child(a, leg), check=True, cwd=str(ROOT), timeout=600, capture_output=True, text=True)
    return json.loads(r.stdout.strip().splitlines()[-1])


def _pooled(ms, batch):
    s = sorted(ms)
    med = s[len(s) // 2]
    return dict(ms_per_step=round(med, 4), min=s[0], max=s[-1], windows=len(s), images_per_s=round(batch / med * 1e3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--imgsz", type=int, default=640)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1, help="how many times the order pose, det, det, pose runs")
    ap.add_argument("--max-det", type=int, default=300)
    ap.add_argument("--conf", type=float, default=0.25, help="confidence threshold of the pose inference leg")
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--val", action="store_true", help="also time the validation step (forward + PoseValidator.update, one graph)")
    ap.add_argument("--leg", choices=LEGS, help="run one workload in this process (a child of the comparison)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pose needs an MI355X: there is no CPU measurement path")
    if a.leg:
        print(json.dumps({"pose": leg_pose, "det": leg_det, "val": leg_val, "kernels": leg_kernels}[a.leg](a, torch.device("cuda:0"))))
        return
    res = {"metric": f"yolov8n-pose (forward + NMS + keypoint gather, one graph) beside yolov8n detection (forward + NMS, one graph), bs "
                     f"{a.batch} {a.imgsz}x{a.imgsz} bf16, ms per step (median of {2 * a.rounds * a.repeats} windows of {a.steps} steps per "
                     f"model), each leg a fresh process; a first collection", "batch": a.batch, "imgsz": a.imgsz, "steps": a.steps,
           "warmup": a.warmup, "repeats": a.repeats, "rounds": a.rounds, "device": torch.cuda.get_device_name(0)}
    pool, order, last = {"pose": [], "det": []}, [], {}
    for _ in range(a.rounds):
        for leg in ("pose", "det", "det", "pose"):
            got = _run_child(a, leg)
            pool[leg] += got["windows_ms"]
            last[leg] = {k: got[k] for k in ("detections", "conf_thres") if k in got}
            order.append(leg)
    res["order"] = order
    for leg in pool:
        res[leg] = dict(_pooled(pool[leg], a.batch), **last[leg])
    res["pose_over_det"] = round(res["pose"]["ms_per_step"] / res["det"]["ms_per_step"], 4)
    if a.val:
        got = _run_child(a, "val")
        res["val"] = dict(_pooled(got.pop("windows_ms"), a.batch), **got)
    k = _run_child(a, "kernels")
    step_us = res["pose"]["ms_per_step"] * 1e3
    k["kpt_decode_share_of_pose_step"] = round(k["kpt_decode_rows_x3_us"] / step_us, 5)
    k["scale_coords_share_of_pose_step_plus_itself"] = round(k["scale_coords_us"] / (step_us + k["scale_coords_us"]), 5)
    if a.val:
        k["pose_match_share_of_val_step"] = round(k["pose_match_us"] / (res["val"]["ms_per_step"] * 1e3), 5)
    res["kernels"] = k
    line = json.dumps(res)
    (ROOT / "profiles").mkdir(exist_ok=True)
    (ROOT / "profiles" / "pose_bench.json").write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
