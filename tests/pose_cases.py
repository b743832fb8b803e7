"""The case tables and input builders the pose tests and tools/gen_golden_pose.py share (data and numpy only: importable where the
reference is not), and the stored bf16 emulation distances the GPU keypoint gate is built from."""

from __future__ import annotations

import numpy as np

from ultralytics_pro_amd.utils import procedural as P

HEAD_CH, HEAD_MAPS = (16, 32, 64), ((6, 7), (3, 4), (2, 2))  # c4 = max(16 // 4, 51) = 51: the padded-channel chain
# name, legacy class branch, nc, kpt_shape
HEAD_CASES = [("pose", True, 1, (17, 3)), ("pose11", False, 1, (17, 3)), ("pose_k5", True, 3, (5, 2))]
# name, img1 (h, w), img0 (h, w), padding, ndim, ratio_pad
COORD_CASES = [("pad", (640, 640), (480, 600), True, 3, None), ("nopad", (640, 640), (480, 600), False, 3, None),
               ("up", (320, 416), (1080, 1920), True, 2, None), ("ratio", (640, 640), (500, 375), True, 3, ((1.28, 1.28), (80.0, 0.0)))]
# the ragged matching batch: name, detections, labels
MATCH_CASES = [("two_cls", 40, 6), ("no_labels", 25, 0), ("no_dets", 0, 3), ("one_label", 300, 1), ("k5", 30, 4)]

# bf16 keypoint gate on the smooth family: the largest distance of oracle/bf16_emul.py's emulation of the whole model from
# the reference's f32 golden over the sampled rows - (x / y in px, visibility) - as tests/pose_oracle.py:emulated_kpt_distance computes
# it on the CPU; tests/test_pose_oracle.py reproduces the pairs, and the GPU is held to TWICE them (the MFMA accumulation order
# differs from the emulation's).
BF16_KPT_EMUL = {"yolov8n-pose": (0.4619, 0.00138), "yolov11n-pose": (0.2346, 0.00078)}
# How far a CPU's own evaluation may sit from the stored pair: the figure is the maximum over some 20 000 values of a chain that rounds
# to bf16 after every layer, so a different f32 summation order (thread count, SIMD width) flips single roundings and moves the
# maximum itself.  Between 1 and 8 threads of one CPU it moved by 8 % (x / y) and 11 % (visibility); another CPU's SIMD width reorders
# the sums once more, independently, so a little over twice that, 25 %, is allowed here.  The GPU gate does not move with it: it is
# twice the stored pair.
BF16_KPT_EMUL_REL = 0.25


def match_case_inputs(name, n, m):
    """Labels: boxes of 20 - 200 px with keypoints inside, visibility in {0, 1, 2}; predictions: a label's keypoints moved by a
    hash-driven fraction of the box size (OKS spread over (0, 1]), or unrelated points.  Classes 0 / 1, plus class 7 on labels only."""
    from tests.pose_oracle import OKS_SIGMA
    kshape = (5, 2) if name == "k5" else (17, 3)
    nkpt, ndim = kshape
    ug = P.hash_uniform(f"poseval:{name}:gt", 8 * max(m, 1)).reshape(-1, 8)
    gk = P.hash_uniform(f"poseval:{name}:gtk", 3 * nkpt * max(m, 1)).reshape(-1, nkpt, 3)
    boxes, gcls, gkpt = np.zeros((m, 4), np.float32), np.zeros(m, np.float32), np.zeros((m, nkpt, 3), np.float32)
    for k in range(m):
        x1, y1 = 40 + 400 * ug[k, 0], 40 + 400 * ug[k, 1]
        w, h = 20 + 180 * ug[k, 2], 20 + 180 * ug[k, 3]
        boxes[k] = (x1, y1, x1 + w, y1 + h)
        gcls[k] = 7.0 if ug[k, 4] < 0.1 else float(int(ug[k, 4] * 2) % 2)
        gkpt[k, :, 0], gkpt[k, :, 1] = x1 + w * gk[k, :, 0], y1 + h * gk[k, :, 1]
        gkpt[k, :, 2] = np.floor(gk[k, :, 2] * 3)
    if name == "two_cls":
        gkpt[2, :, 2] = 0.0  # a label with every keypoint invisible: OKS 0 through the eps denominator
        boxes[3, 2] = boxes[3, 0]  # a zero-area label box
        gcls[:4] = (0.0, 1.0, 0.0, 1.0)
    up = P.hash_uniform(f"poseval:{name}:pred", 8 * max(n, 1)).reshape(-1, 8)
    pk = P.hash_uniform(f"poseval:{name}:predk", 3 * nkpt * max(n, 1)).reshape(-1, nkpt, 3)
    pred, pcls = np.zeros((n, nkpt, ndim), np.float32), np.zeros(n, np.float32)
    for i in range(n):
        if m and up[i, 0] < 0.85:
            k = int(up[i, 1] * m) % m
            w, h = boxes[k, 2] - boxes[k, 0], boxes[k, 3] - boxes[k, 1]
            s = 0.25 * up[i, 2] ** 2 * np.sqrt(max(w * h, 400.0))
            pred[i, :, 0] = gkpt[k, :, 0] + s * (pk[i, :, 0] - 0.5)
            pred[i, :, 1] = gkpt[k, :, 1] + s * (pk[i, :, 1] - 0.5)
            pcls[i] = gcls[k] if up[i, 3] > 0.2 else float((int(gcls[k]) + 1) % 2)
        else:
            pred[i, :, 0], pred[i, :, 1] = 640 * pk[i, :, 0], 640 * pk[i, :, 1]
            pcls[i] = float(int(up[i, 1] * 2) % 2)
        if ndim == 3:
            pred[i, :, 2] = pk[i, :, 2]
    if name == "two_cls" and n > 5:  # the zero-area label met exactly (OKS 1 despite area 0) and nearly
        pred[4, :, :2], pcls[4] = gkpt[3, :, :2], gcls[3]
        pred[5, :, :2], pcls[5] = gkpt[3, :, :2] + 1e-3, gcls[3]
    sigma = OKS_SIGMA if kshape == (17, 3) else np.ones(nkpt) / nkpt
    return pred, pcls, boxes, gcls, gkpt, sigma
