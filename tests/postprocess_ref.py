"""CPU reference (test infrastructure) of the detection post-processing, in plain numpy and Python loops: `non_max_suppression`
(ultralytics/utils/nms.py:13-166 with TorchNMS.nms, :239-296), `box_iou` (utils/metrics.py:54-74), `scale_boxes` + `clip_boxes`
(utils/ops.py:102-178) and the box half of DetectionValidator._process_batch (models/yolo/detect/val.py:274-288).

`nms_ref` writes the greedy pass as the textbook double loop - a candidate is kept unless a kept, higher-scored box suppresses it - and
takes every keep/suppress decision twice, in np.float32 in the reference's operation order and in float64.  The zero-area rule is
explicit: a pair whose intersection is 0 never suppresses.  (TorchNMS.nms gets there by leaving the suppression step early when the
kept box intersects nothing; for boxes with w, h >= 0 the two are the same: a kept box of positive area gives IoU 0 / area = 0, a
zero-area kept box intersects nothing at all.)

The `scenes()` / `match_scenes()` builders make inputs on which the outcome is DECIDABLE: every f32 decision agrees with its float64
twin, except the pairs a scene lists as deliberately on a threshold - those have integer coordinates below 2^24, so every f32 operation
before the one IEEE division is exact and the f32 quotient is the definition.  tests/test_postprocess_ref.py pins all of this against
oracle/nms.py and the reference goldens on the CPU; tests/test_hip_postprocess.py runs the kernels against it bit for bit.
"""

from __future__ import annotations

import numpy as np

from tests import segval_ref as V

F32 = np.float32
IOUV = V.IOUV
DEC = np.dtype([("kept", np.int64), ("cand", np.int64), ("f32", bool), ("f64", bool)])  # ids: anchor * nc + cls


# ---- non_max_suppression ----------------------------------------------------------------------------------------------------------


def _xyxy(p4: np.ndarray, dt) -> np.ndarray:
    """(4, n) xywh -> (n, 4) xyxy: xy -/+ wh / 2 (utils/ops.py:268-284)."""
    b = p4.astype(dt)
    hw, hh = b[2] / dt(2), b[3] / dt(2)
    return np.stack([b[0] - hw, b[1] - hh, b[0] + hw, b[1] + hh], 1)


def _suppress(K, ka, c, ca, thr):
    """Would each kept box K (k, 4) (areas ka) suppress candidate c?  inter == 0 never does; else `not (iou <= thr)`, no eps."""
    w = np.maximum(np.minimum(K[:, 2], c[2]) - np.maximum(K[:, 0], c[0]), 0)
    h = np.maximum(np.minimum(K[:, 3], c[3]) - np.maximum(K[:, 1], c[1]), 0)
    inter = w * h
    with np.errstate(invalid="ignore", divide="ignore"):
        iou = inter / (ka + ca - inter)
    return (inter != 0) & ~(iou <= thr)


def candidates(pred, conf_thres=0.25, iou_thres=0.45, classes=None, agnostic=False, multi_label=False, max_det=300, nc=0,
               max_nms=30000, max_wh=7680, tie_last=False):
    """Per image the candidate list in score order (stable: ties by candidate index anchor * nc + cls), cut at max_nms: a dict of
    anchor, cls, score, id, raw xyxy (f32), class-offset xyxy in f32 and in float64, and the count of `score > conf_thres` decisions on
    which f32 and float64 differ.  `tie_last` (for tests that break the rule on purpose) orders equal scores by DESCENDING index."""
    pred = np.asarray(pred, F32)
    assert pred.ndim == 3 and 0 <= conf_thres <= 1 and 0 <= iou_thres <= 1
    nc = nc or pred.shape[1] - 4
    multi_label = bool(multi_label) and nc > 1
    conf32 = F32(conf_thres)  # a Python scalar compared with an f32 tensor is taken in f32
    for p in pred:
        sc = p[4:4 + nc]  # (nc, A)
        undecided = int(((sc > conf32) != (sc.astype(np.float64) > float(conf_thres))).sum())
        if multi_label:
            a, c = np.nonzero(sc.T > conf32)  # anchor-major: candidate order anchor * nc + cls
        else:
            c = sc.argmax(0)  # first maximum
            a = np.nonzero(sc[c, np.arange(sc.shape[1])] > conf32)[0]
            c = c[a]
        if classes is not None:
            m = np.isin(c, np.asarray(list(classes), np.int64))
            a, c = a[m], c[m]
        if tie_last:
            a, c = a[::-1], c[::-1]
        o = np.argsort(-sc[c, a], kind="stable")[:max_nms]  # the reference sorts twice (the max_nms cut, then inside the NMS): one stable order
        a, c = a[o], c[o]
        raw = _xyxy(p[:4, a], F32)
        off = 0 if agnostic else max_wh
        yield dict(anchor=a.astype(np.int64), cls=c, score=sc[c, a], id=a.astype(np.int64) * nc + c, raw=raw, undecided=undecided,
                   ob32=raw + (c.astype(F32) * F32(off))[:, None],
                   ob64=_xyxy(p[:4, a], np.float64) + (c.astype(np.float64) * float(off))[:, None])


def nms_ref(pred, **kw):
    """(B, 4 + nc, A) f32 and the arguments of `non_max_suppression` -> per image (rows (n, 6) f32, kept anchor indices (n,) int64,
    decisions (DEC records: every (kept box, candidate) pair the greedy pass looked at, with the f32 and the float64 verdict
    "suppresses"), score_disagreements)."""
    thr32 = F32(kw.get("iou_thres", 0.45))
    thr64, max_det = np.float64(thr32), kw.get("max_det", 300)
    res = []
    for cd in candidates(pred, **kw):
        ob32, ob64, ids = cd["ob32"], cd["ob64"], cd["id"]
        a32 = (ob32[:, 2] - ob32[:, 0]) * (ob32[:, 3] - ob32[:, 1])
        a64 = (ob64[:, 2] - ob64[:, 0]) * (ob64[:, 3] - ob64[:, 1])
        kept = np.zeros(max(min(max_det, ids.shape[0]), 1), np.int64)
        nk, dec = 0, []
        for i in range(ids.shape[0]):  # the textbook double loop: candidate i against every kept box before it
            if nk >= max_det:
                break
            k = kept[:nk]
            s32 = _suppress(ob32[k], a32[k], ob32[i], a32[i], thr32)
            s64 = _suppress(ob64[k], a64[k], ob64[i], a64[i], thr64)
            d = np.empty(nk, DEC)
            d["kept"], d["cand"], d["f32"], d["f64"] = ids[k], ids[i], s32, s64
            dec.append(d)
            if not s32.any():
                kept[nk] = i
                nk += 1
        k = kept[:nk]
        rows = np.concatenate([cd["raw"][k], cd["score"][k, None], cd["cls"][k, None].astype(F32)], 1).astype(F32).reshape(nk, 6)
        res.append((rows, cd["anchor"][k], np.concatenate(dec) if dec else np.empty(0, DEC), cd["undecided"]))
    return res


def nms_fixed(res, max_det):
    """The fixed-shape outputs of the device NMS from `nms_ref`'s result: rows (B, max_det, 6) zero past counts, counts, keep (-1)."""
    b = len(res)
    out, counts, keep = np.zeros((b, max_det, 6), F32), np.zeros(b, np.int32), np.full((b, max_det), -1, np.int32)
    for i, (rows, k, _, _) in enumerate(res):
        n = rows.shape[0]
        out[i, :n], counts[i], keep[i, :n] = rows, n, k
    return out, counts, keep


def best_keys(pred, nc=0) -> np.ndarray:
    """(B, A) int64 bit patterns of the best-class NMS keys as the fused Detect class tails write them, one per anchor, candidate or
    not: (~bits(best score) << 32) | (anchor * nc + first argmax).  (The NMS applies conf_thres / the class filter to them itself; a
    word left at -1 decodes to score 0.)"""
    pred = np.asarray(pred, F32)
    nc = nc or pred.shape[1] - 4
    sc = pred[:, 4:4 + nc]
    c = sc.argmax(1)
    best = np.take_along_axis(sc, c[:, None], 1)[:, 0]
    bits = np.ascontiguousarray(best).view(np.uint32).astype(np.uint64)
    ids = np.arange(pred.shape[2], dtype=np.uint64)[None] * np.uint64(nc) + c.astype(np.uint64)
    return ((~bits & np.uint64(0xFFFFFFFF)) << np.uint64(32) | ids).view(np.int64)


# ---- box_iou, scale_boxes, match_predictions -----------------------------------------------------------------------------------------


def box_iou_ref(box1, box2, eps=1e-7, dtype=np.float64) -> np.ndarray:
    """(N, 4), (M, 4) xyxy -> (N, M): inter / (area1 + area2 - inter + eps) in `dtype`, in the order of utils/metrics.py:54-74."""
    a, b = np.asarray(box1, F32).astype(dtype)[:, None], np.asarray(box2, F32).astype(dtype)[None]
    w = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), 0)
    h = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), 0)
    inter = w * h
    return inter / ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]) - inter + dtype(eps))


def scale_boxes_ref(img1_shape, boxes, img0_shape, ratio_pad=None, padding=True, dtype=np.float64) -> np.ndarray:
    """utils/ops.py:102-152 + clip_boxes (:154-178) on rows (..., k >= 4): the first four columns rescaled and clipped in `dtype`."""
    if ratio_pad is None:
        gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
        pad_x = round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1)
        pad_y = round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1)
    else:
        gain, (pad_x, pad_y) = ratio_pad[0][0], ratio_pad[1]
    out = np.asarray(boxes, F32).astype(dtype).copy()
    if padding:
        out[..., 0] -= dtype(pad_x); out[..., 1] -= dtype(pad_y); out[..., 2] -= dtype(pad_x); out[..., 3] -= dtype(pad_y)
    out[..., :4] /= dtype(gain)
    out[..., 0] = np.clip(out[..., 0], 0, dtype(img0_shape[1])); out[..., 1] = np.clip(out[..., 1], 0, dtype(img0_shape[0]))
    out[..., 2] = np.clip(out[..., 2], 0, dtype(img0_shape[1])); out[..., 3] = np.clip(out[..., 3], 0, dtype(img0_shape[0]))
    return out


def match_ref(det, gt, iouv=IOUV):
    """det (N, 6) rows [x1, y1, x2, y2, conf, cls], gt (M, 5) rows [cls, x1, y1, x2, y2] -> (TP (N, len(iouv)) bool, IoU (M, N) in f32
    as the reference computes it - labels x detections, eps 1e-7 -, the same in float64)."""
    det, gt = np.asarray(det, F32).reshape(-1, 6), np.asarray(gt, F32).reshape(-1, 5)
    n, m = det.shape[0], gt.shape[0]
    if n == 0 or m == 0:
        return np.zeros((n, len(iouv)), bool), np.zeros((m, n), F32), np.zeros((m, n))
    i32, i64 = box_iou_ref(gt[:, 1:], det[:, :4], dtype=F32), box_iou_ref(gt[:, 1:], det[:, :4], dtype=np.float64)
    assert i32.dtype == F32
    return V.match_predictions(det[:, 5], gt[:, 0], i32, iouv), i32, i64


# ---- NMS scenes ---------------------------------------------------------------------------------------------------------------------


class Scene:
    """One NMS input with its arguments.  `on_thr`: the (kept id, candidate id) pairs that sit on the IoU threshold on purpose."""

    def __init__(self, name, pred, kw, on_thr=(), expect=None):
        self.name, self.pred, self.kw, self.on_thr, self.expect = name, np.ascontiguousarray(pred, F32), dict(kw), set(on_thr), expect
        self._ref = None

    @property
    def nc(self):
        return self.kw.get("nc", 0) or self.pred.shape[1] - 4

    @property
    def single_label(self):
        return not (self.kw.get("multi_label", False) and self.nc > 1)

    def ref(self):
        """`nms_ref` of the scene, computed once; asserts that the scene is decidable."""
        if self._ref is None:
            res = nms_ref(self.pred, **self.kw)
            max_wh = 0 if self.kw.get("agnostic", False) else self.kw.get("max_wh", 7680)
            for b, (rows, keep, dec, undecided) in enumerate(res):
                assert undecided == 0, f"{self.name}[{b}]: {undecided} score > conf_thres decisions differ between f32 and f64"
                for d in dec[dec["f32"] != dec["f64"]]:
                    assert (int(d["kept"]), int(d["cand"])) in self.on_thr, f"{self.name}[{b}]: undecidable pair {d}"
                for ids in self.on_thr:  # integer coordinates below 2^24: exact up to the one division
                    for i in ids:
                        box = _xyxy(self.pred[b, :4, i // self.nc][:, None], np.float64)[0] + (i % self.nc) * float(max_wh)
                        area = (box[2] - box[0]) * (box[3] - box[1])
                        assert (box == np.round(box)).all() and np.abs(box).max() < 2 ** 24 and area < 2 ** 23, (self.name, box)
                if self.expect is not None:
                    assert rows.shape[0] == self.expect[b], f"{self.name}[{b}]: {rows.shape[0]} kept, built for {self.expect[b]}"
            self._ref = res
        return self._ref

    def fixed(self):
        return nms_fixed(self.ref(), self.kw.get("max_det", 300))


def _desc(n: int, hi=0.95, lo=0.30) -> np.ndarray:
    """n strictly descending f32 scores."""
    s = (hi - (hi - lo) * np.arange(n) / max(n, 1)).astype(F32)
    assert (np.diff(s) < 0).all()
    return s


def build(name, units, nc, kw, *, shuffle=True, A=None, on_thr=(), expect=None, batch=None):
    """units: per image a list of (anchor key, (x1, y1, x2, y2), cls, score or None) in the order the scores should descend (None
    = the next of a strictly descending series).  One anchor per distinct key; `shuffle` scatters the anchors over the anchor axis, so
    the score order is not the memory order.  Anchors without a unit (padding up to A) have zero boxes and scores."""
    images = batch if batch is not None else [units]
    keysets = []
    for u in images:
        keys = []
        for k, *_ in u:
            if k not in keys:
                keys.append(k)
        keysets.append(keys)
    A = A or max(max(len(k) for k in keysets), 1)
    pred = np.zeros((len(images), 4 + nc, A), np.float64)
    rng = np.random.default_rng(len(name) * 7919 + A)
    for b, (u, keys) in enumerate(zip(images, keysets)):
        assert len(keys) <= A
        slot = rng.permutation(A)[:len(keys)] if shuffle else np.arange(len(keys))
        where = {k: int(s) for k, s in zip(keys, slot)}
        series = iter(_desc(sum(1 for x in u if x[3] is None)))
        for k, (x1, y1, x2, y2), c, s in u:
            a = where[k]
            pred[b, :4, a] = ((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1)
            assert pred[b, 4 + c, a] == 0, "one unit per (anchor, class)"
            pred[b, 4 + c, a] = next(series) if s is None else s
    p32 = pred.astype(F32)
    assert np.array_equal(p32[:, :4].astype(np.float64), pred[:, :4]), "box coordinates must be exact in f32"
    return Scene(name, p32, kw, on_thr, expect)


def _cell(i: int, y0=0.0, size=10.0):
    """Isolated boxes: cell i of a grid with 30 px pitch (boxes of 10 px never touch)."""
    x, y = 30.0 * (i % 60), y0 + 30.0 * (i // 60)
    return (x, y, x + size, y + size)


def _shift(box, dx=1.0):
    """The same box moved by dx in x: IoU (10 - dx) / (10 + dx) with the original = 9/11 for 1 px."""
    return (box[0] + dx, box[1], box[2] + dx, box[3])


def _iso(n, tag, first=0, cls=1, y0=0.0):
    return [((tag, i), _cell(first + i, y0), cls, None) for i in range(n)]


def _chain(n, step, tag, y0, cls=1, x0=0.0):
    """Boxes 10 wide stepped by `step`: IoU (10 - d step) / (10 + d step) at distance d.  step 3: 7/13 then 4/16 against thr 0.5 - keep,
    drop, keep, ...; step 1.5: 8.5/11.5, 7/13, 5.5/14.5 - keep, drop, drop, keep, ..."""
    return [((tag, i), (x0 + step * i, y0, x0 + step * i + 10.0, y0 + 10.0), cls, None) for i in range(n)]


def _two_classes(units, c2):
    """Every unit again in class c2 right behind it in score order (multi-label: two candidates per anchor)."""
    out = []
    for k, box, c, s in units:
        out += [(k, box, c, s), (k, box, c2, s)]
    return out


def _both(name, units, nc, kw, c2=2, **b):
    """A single-label scene, and the multi-label scene in which every anchor is a candidate in a second class too (twice the boxes:
    max_det and max_nms double with them)."""
    e, batch = b.pop("expect", None), b.pop("batch", None)
    ml = dict(kw, multi_label=True)
    for k in ("max_det", "max_nms"):
        if k in kw:
            ml[k] = 2 * kw[k]
    return [build(name + "-sl", units, nc, kw, expect=e, batch=batch, **b),
            build(name + "-ml", None if units is None else _two_classes(units, c2), nc, ml, expect=None if e is None else [2 * v for v in e],
                  batch=None if batch is None else [_two_classes(u, c2) for u in batch], **b)]


KW = dict(conf_thres=0.25, iou_thres=0.5)
BIG = (0.0, 3000.0, 1000.0, 3010.0)  # a long box: [0, 1000 - j] x the same rows has IoU (1000 - j) / 1000 with it


def _victims(n, tag):
    return [((tag, j), (0.0, 3000.0, 1000.0 - (j + 1), 3010.0), 1, None) for j in range(n)]


def _interleave(a, b):
    """b's units spread evenly between a's."""
    out = list(a)
    for j, u in enumerate(b):
        out.insert(min((j + 1) * (len(a) + len(b)) // (len(b) + 1), len(out)), u)
    return out


def _lead64():
    """The first chunk: 63 isolated boxes and BIG, all kept."""
    u = _iso(63, "lead")
    u.insert(30, (("big", 0), BIG, 1, None))
    return u


def scenes_structure():
    s = []
    # chains: suppression chains as long as the chunk, in one chunk and across chunk boundaries
    for n in (70, 200):
        s += _both(f"chain{n}_period2", _chain(n, 3.0, "c", 2000.0), 3, KW, expect=[(n + 1) // 2])
        s += _both(f"chain{n}_period3", _chain(n, 1.5, "c", 2000.0), 3, KW, expect=[(n + 2) // 3])
    s += _both("chain200_from60", _iso(60, "lead") + _chain(200, 3.0, "c", 2000.0), 3, dict(KW, max_det=400), expect=[160])
    s += _both("chain200_from60_staged", _iso(60, "lead") + _chain(200, 3.0, "c", 2000.0), 17, dict(KW, max_det=400), c2=16, A=1000, expect=[160])
    # serial walk / suppression columns: k alive candidates in the second chunk, the rest suppressed by a box kept in the first
    for k in (7, 8, 9):
        chunk = _interleave(_victims(64 - k, "v"), _chain(k, 3.0, "alive", 2500.0))
        s += _both(f"alive{k}", _lead64() + chunk + _iso(10, "tail", first=100), 3, KW, expect=[64 + (k + 1) // 2 + 10])
    # kept-list slices: every kept index 0..63 (each wave's slice four times) has exactly one candidate only it suppresses
    lead = _iso(64, "lead")
    s += _both("slices64", lead + [(("hit", i), _shift(u[1]), 1, None) for i, u in enumerate(lead)] + _iso(5, "tail", first=100), 3, KW,
               expect=[69])
    lead = _iso(40, "lead")
    s += _both("slices40", lead + [(("hit", i), _shift(u[1]), 1, None) for i, u in enumerate(lead)] + _iso(30, "tail", first=100), 3, KW,
               expect=[70])
    # max_det inside a chunk: serial walk (3 alive, room 2) and columns (20 alive in a chain = 10 kept, room 5), first and second chunk
    s += _both("cut_serial_first", _iso(3, "i"), 3, dict(KW, max_det=2), expect=[2])
    s += _both("cut_cols_first", _chain(20, 3.0, "c", 2000.0), 3, dict(KW, max_det=5), expect=[5])
    s += _both("cut_serial_second", _lead64() + _interleave(_victims(61, "v"), _iso(3, "alive", first=100)), 3, dict(KW, max_det=66),
               expect=[66])
    s += _both("cut_cols_second", _lead64() + _interleave(_victims(44, "v"), _chain(20, 3.0, "alive", 2500.0)), 3, dict(KW, max_det=69),
               expect=[69])
    iso = _iso(1100, "i")
    for md in (1, 64, 65, 1024):
        s.append(build(f"iso1100_maxdet{md}", iso, 2, dict(KW, max_det=md), expect=[md]))
    s.append(build("iso1100_maxdet1024-ml", _two_classes(iso, 0), 2, dict(KW, max_det=1024, multi_label=True), expect=[1024]))
    # stage boundary: one isolated box, then (suppressor, victim) pairs at sorted positions (1, 2), (3, 4), ... (1023, 1024), then
    # groups of four (one kept, three victims)
    def staged(n, ml):
        u = []
        for pos in range(n):
            if pos <= 1024:
                g, r = (pos + 1) // 2, (pos + 1) % 2  # group, 0 = suppressor
            else:
                g, r = 513 + (pos - 1025) // 4, (pos - 1025) % 4
            if ml:  # the victims are the same anchor in further classes, the NMS is class-agnostic
                u.append((("g", g), _cell(g), r, None))
            else:
                u.append((("g", g, r), _shift(_cell(g), float(r)), 1, None))
        return u
    for n in (1023, 1024, 1025, 2049):
        kept = sum(1 for pos in range(n) if pos == 0 or (pos <= 1024 and pos % 2 == 1) or (pos > 1024 and (pos - 1025) % 4 == 0))
        s.append(build(f"stage{n}-sl", staged(n, False), 2, dict(KW, max_det=1024), expect=[kept]))
        s.append(build(f"stage{n}-ml", staged(n, True), 4, dict(KW, max_det=1024, multi_label=True, agnostic=True), expect=[kept]))
    # max_nms: n = max_nms and max_nms + 1, a non-power of two with equal scores across the cut (the candidate index decides), max_nms 1
    def cut_units(n_in, n_out, tie):
        """n_in + n_out candidates; the `tie` candidates around the cut share one score; of the cut-away ones every fifth is isolated
        (would have been kept), the others are victims of kept boxes."""
        sc = _desc(n_in + n_out)
        if tie:
            sc[max(n_in - tie // 2, 0):n_in + tie - tie // 2] = sc[n_in]
        u = []
        for i in range(n_in + n_out):
            box = _cell(i) if (i < n_in or (i - n_in) % 5 == 0) else _shift(_cell(i % n_in))
            u.append((("c", i), box, 1, float(sc[i])))
        return u
    for n_in, n_out, tie, tag in ((100, 0, 0, "n_eq"), (100, 1, 0, "n_plus1"), (100, 50, 10, "ties"), (1, 30, 6, "one"), (256, 300, 40, "pow2")):
        s += _both(f"maxnms_{tag}", cut_units(n_in, n_out, tie), 3, dict(KW, max_nms=n_in, max_det=500), shuffle=True)
    return s


def scenes_edges():
    s = []
    A_, B_ = (0.0, 0.0, 10.0, 10.0), (5.0, 0.0, 15.0, 10.0)  # IoU 50 / 150
    C_, D_ = (0.0, 0.0, 10.0, 10.0), (5.0, 5.0, 15.0, 15.0)  # IoU 25 / 175
    third, q = float(F32(1) / F32(3)), float(F32(25) / F32(175))
    below = lambda v: float(np.nextafter(F32(v), F32(0)))  # noqa: E731
    for tag, boxes, thr in (("third", (A_, B_), third), ("25_175", (C_, D_), q)):
        for c in (0, 2):  # class 2: the offset 2 * 7680 is added first, the coordinates stay integers
            u = [(0, boxes[0], c, 0.9), (1, boxes[1], c, 0.8)]
            s.append(build(f"iou_eq_thr_{tag}_c{c}", u, 3, dict(KW, iou_thres=thr), shuffle=False, on_thr=[(c, 3 + c)], expect=[2]))
            s.append(build(f"iou_ulp_above_thr_{tag}_c{c}", u, 3, dict(KW, iou_thres=below(thr)), shuffle=False, on_thr=[(c, 3 + c)],
                           expect=[1]))
    touch = [(0, A_, 1, 0.9), (1, (10.0, 0.0, 20.0, 10.0), 1, 0.8), (2, (19.5, 0.0, 29.5, 10.0), 1, 0.7), (3, A_, 1, 0.6)]
    s += _both("iou_thres_0", touch, 3, dict(KW, iou_thres=0.0), shuffle=False, expect=[2])  # touching: inter 0, kept; any overlap: dropped
    s += _both("iou_thres_1", touch, 3, dict(KW, iou_thres=1.0), shuffle=False, expect=[4])  # identical boxes: IoU 1 <= 1, kept
    # score thresholds
    up = lambda v: float(np.nextafter(F32(v), F32(1)))  # noqa: E731
    u = [(0, _cell(0), 1, 0.25), (1, _cell(1), 1, up(0.25)), (2, _cell(2), 0, 0.5), (2, _cell(2), 2, 0.25), (3, _cell(3), 2, up(0.25))]
    s.append(build("score_eq_conf-sl", u, 3, KW, shuffle=False, expect=[3]))
    s.append(build("score_eq_conf-ml", u, 3, dict(KW, multi_label=True), shuffle=False, expect=[3]))
    u = [(0, _cell(0), 1, 0.0), (1, _cell(1), 1, float(np.finfo(F32).tiny)), (2, _cell(2), 0, 1.0), (3, _cell(3), 2, 0.0)]
    s.append(build("conf_0-sl", u, 3, dict(KW, conf_thres=0.0), shuffle=False, A=6, expect=[2]))
    s.append(build("conf_0-ml", u, 3, dict(KW, conf_thres=0.0, multi_label=True), shuffle=False, A=6, expect=[2]))
    # ties
    pairs = []
    for i in range(12):  # equal scores across anchors: the lower anchor index is first, whichever way the overlap goes
        pairs += [(2 * i, _cell(i), 1, 0.5), (2 * i + 1, _shift(_cell(i)), 1, 0.5 if i % 2 else 0.75)]
    s += _both("tie_anchors", pairs, 3, KW, shuffle=False)
    for nc in (9, 17):  # equal class maxima at classes 7 and 8: the unrolled-by-8 scan and its tail; first maximum wins
        u = []
        for i, (c1, c2) in enumerate(((7, 8), (1, 8) if nc == 9 else (8, 16), (0, 8), (6, 7), (0, 7))):
            u += [(i, _cell(i), c1, 0.5 + 0.0625 * i), (i, _cell(i), c2, 0.5 + 0.0625 * i)]
        u += [(9, _shift(_cell(0)), 8, 0.4), (10, _shift(_cell(1)), 8, 0.4)]  # survive iff the tied anchor went to the other class
        for ag in (False, True):
            s.append(build(f"tie_classes_nc{nc}{'_agn' if ag else ''}-sl", u, nc, dict(KW, agnostic=ag), shuffle=False, A=70))
            s.append(build(f"tie_classes_nc{nc}{'_agn' if ag else ''}-ml", u, nc, dict(KW, agnostic=ag, multi_label=True), shuffle=False, A=70))
    s.append(build("tie_classes_staged-ml", [(i, _cell(i // 2) if i % 2 == 0 else _shift(_cell(i // 2)), c, 0.5 + 0.01 * (i % 5))
                                             for i in range(100) for c in (0, 7, 8, 16)], 17,
                   dict(KW, multi_label=True), shuffle=True, A=1000))
    u = [(0, _cell(0), 0, 0.9), (1, _shift(_cell(0)), 0, 0.8), (2, _cell(1), 0, 0.8), (3, _cell(2), 0, 0.25)]
    s.append(build("nc1_multi_label", u, 1, dict(KW, multi_label=True), shuffle=False, expect=[2]))
    s.append(build("nc1", u, 1, KW, shuffle=False, expect=[2]))
    # class offset
    same = [(0, _cell(0), 0, 0.9), (1, _cell(0), 1, 0.8), (2, _cell(5), 2, 0.7), (2, _cell(5), 0, 0.6), (3, _cell(5), 2, 0.5)]
    s.append(build("offset_two_classes-sl", same, 3, KW, shuffle=False, expect=[3]))
    s.append(build("offset_two_classes-ml", same, 3, dict(KW, multi_label=True), shuffle=False, expect=[4]))
    s.append(build("offset_agnostic-sl", same, 3, dict(KW, agnostic=True), shuffle=False, expect=[2]))
    s.append(build("offset_agnostic-ml", same, 3, dict(KW, agnostic=True, multi_label=True), shuffle=False, expect=[2]))
    near = [(0, (64.0, 64.0, 74.0, 74.0), 0, 0.9), (1, (1.0, 1.0, 11.0, 11.0), 1, 0.8), (2, (130.0, 130.0, 140.0, 140.0), 0, 0.7),
            (3, (1.0, 1.0, 11.0, 11.0), 2, 0.6), (4, (300.0, 300.0, 310.0, 310.0), 1, 0.5)]
    s += _both("offset_max_wh64", near, 4, dict(KW, max_wh=64), c2=3, shuffle=False)  # class 1 at 1..11 lands on class 0 at 65..75
    s += _both("offset_max_wh64_default", near, 4, KW, c2=3, shuffle=False)
    filt = same + _iso(20, "i", first=10, cls=1) + _iso(20, "j", first=40, cls=0)
    s.append(build("classes_filter-sl", filt, 3, dict(KW, classes=[1, 2]), shuffle=False, expect=[22]))
    s.append(build("classes_filter-ml", filt, 3, dict(KW, classes=[0, 2], multi_label=True), shuffle=False, expect=[23]))
    s += _both("classes_filter_none", [(0, _cell(0), 0, 0.9), (1, _cell(1), 1, 0.8)], 4, dict(KW, classes=[3]), c2=2, shuffle=False, expect=[0])
    # degenerate boxes: w = 0, h = 0 or both, on top of each other, inside an ordinary box, far away
    P0, P1 = (50.0, 50.0, 50.0, 50.0), (500.0, 500.0, 500.0, 500.0)
    Vl, Hl, O, O2 = (50.0, 45.0, 50.0, 60.0), (45.0, 50.0, 55.0, 50.0), (40.0, 40.0, 60.0, 60.0), (41.0, 40.0, 61.0, 60.0)
    three = [(0, P0, 1, 0.9), (1, P0, 1, 0.8), (2, P1, 1, 0.7), (3, O, 1, 0.6)]
    s += _both("degenerate_three_points", three, 3, KW, shuffle=False, expect=[4])
    mix = [(0, P0, 1, None), (1, Vl, 1, None), (2, O, 1, None), (3, Hl, 1, None), (4, P0, 1, None), (5, O2, 1, None), (6, Vl, 1, None),
           (7, P1, 1, None), (8, Hl, 1, None), (9, P1, 1, None)]
    s += _both("degenerate_mix", mix, 3, KW, shuffle=False, expect=[9])
    s += _both("degenerate_mix_ordinary_first", mix[2:] + mix[:2], 3, KW, shuffle=False, expect=[9])
    agn = [(k, b, k % 3, sc) for k, b, _, sc in mix]
    s += _both("degenerate_agnostic", agn, 4, dict(KW, agnostic=True), c2=3, shuffle=False)
    s.append(build("degenerate_chunk", [((i,), P0 if i % 3 else _cell(i), 1, None) for i in range(150)], 3, dict(KW, max_det=300), expect=[150]))
    # shapes: A around the 64-lane and 256-thread edges; B = 3 with an image without candidates and one with a single candidate
    for A in (1, 63, 64, 65, 255, 256, 257):
        u = []
        for i in range(A):
            if i % 3 != 2:  # every third anchor is no candidate; odd ones are victims of their left neighbour
                u.append((i, _shift(_cell(i - 1)) if i % 2 else _cell(i), 1, None))
        s += _both(f"shape_A{A}", u, 3, KW, A=A)
        s += _both(f"shape_A{A}_B3", None, 3, KW, A=A, batch=[u, [], u[:1]])
    return s


_SCENES = None


def scenes():
    """Every NMS scene, built once."""
    global _SCENES
    if _SCENES is None:
        _SCENES = scenes_structure() + scenes_edges()
        names = [s.name for s in _SCENES]
        assert len(set(names)) == len(names)
    return _SCENES


def scene(name: str) -> Scene:
    return next(s for s in scenes() if s.name == name)


# ---- matching scenes ----------------------------------------------------------------------------------------------------------------


class MatchScene:
    """Fixed-shape inputs of `match_predictions_batched`: det (B, max_det, 6), counts (B,), gt (B, max_gt, 5), ngt (B,), iouv.  `on_thr`:
    the (image, label, detection) triples whose IoU sits on a threshold on purpose."""

    def __init__(self, name, det, counts, gt, ngt, iouv=IOUV, on_thr=()):
        self.name, self.det, self.gt = name, np.ascontiguousarray(det, F32), np.ascontiguousarray(gt, F32)
        self.counts, self.ngt = np.asarray(counts, np.int32), np.asarray(ngt, np.int32)
        self.iouv, self.on_thr = np.asarray(iouv, F32), set(on_thr)
        self._ref = None

    def ref(self):
        """(B, max_det, 10) uint8 true positives (zero rows at and past counts[b]), computed once; asserts decidability: every
        `IoU >= iouv[k]` agrees between f32 and f64 off the listed pairs, and no detection has two same-class labels at one IoU."""
        if self._ref is None:
            b, max_det, max_gt = self.det.shape[0], self.det.shape[1], self.gt.shape[1]
            tp = np.zeros((b, max_det, len(self.iouv)), np.uint8)
            for i in range(b):
                n, m = min(int(self.counts[i]), max_det), min(int(self.ngt[i]), max_gt)
                t, i32, i64 = match_ref(self.det[i, :n], self.gt[i, :m], self.iouv)
                tp[i, :n] = t
                same = self.gt[i, :m, 0][:, None] == self.det[i, :n, 5][None]
                for l, d in zip(*np.nonzero(same)):
                    if ((i32[l, d] >= self.iouv) != (i64[l, d] >= self.iouv.astype(np.float64))).any():
                        assert (i, int(l), int(d)) in self.on_thr, f"{self.name}: undecidable IoU, image {i} label {l} detection {d}"
                        box = np.concatenate([self.gt[i, l, 1:], self.det[i, d, :4]]).astype(np.float64)
                        assert (box == np.round(box)).all() and np.abs(box).max() < 2 ** 11  # areas and their sum below 2^24
                for d in range(n):
                    v = np.sort(i32[same[:, d] & (i32[:, d] > 0), d])
                    assert (np.diff(v) > 0).all(), f"{self.name}: image {i} detection {d} has two labels at one IoU"
            self._ref = tp
        return self._ref


def _lab(i):
    """Label i: 30 x 30 px at a cell of its own (detections [0, 30] x [0, h] on it have IoU h / 30: on no threshold for integer h)."""
    x, y = 100.0 * (i % 12), 100.0 * (i // 12)
    return np.array([x, y, x + 30.0, y + 30.0])


def _on(label, h, w=30.0):
    """A detection over the top-left w x h of a label box."""
    return np.array([label[0], label[1], label[0] + w, label[1] + h])


def match_scene(max_det: int, custom_iouv=False) -> MatchScene:
    """B = 3: image 0 holds the contests, image 1 has detections and no label, image 2 labels and no detection."""
    max_gt = 64
    det, gt = np.zeros((3, max_det, 6), F32), np.zeros((3, max_gt, 5), F32)
    on_thr = []
    # image 0.  Labels 0..39 of class l % 3; label 40..43 are 20 x 20 (IoU h / 20: on the thresholds)
    for l in range(40):
        gt[0, l] = (l % 3, *_lab(l))
    for l in range(40, 44):
        gt[0, l] = (1, *(_lab(l)[:2]), *(_lab(l)[:2] + 20.0))
    ngt0 = 44
    n0 = max_det - 10
    rows = {}  # detection index -> (box, cls)
    # several detections share their best label: the smallest index wins per threshold; the later one has the higher IoU
    rows[3], rows[7], rows[11] = (_on(_lab(0), 17), 0), (_on(_lab(0), 25), 0), (_on(_lab(0), 20), 0)
    for lo, hi, l in ((250, 260, 1), (255, 256, 2)) + (((510, 515, 4), (511, 512, 5)) if max_det > 515 else ()):
        rows[lo], rows[hi] = (_on(_lab(l), 17), l % 3), (_on(_lab(l), 28), l % 3)
    # a detection over two labels of its class takes the better one; the other label goes to a later detection
    # two overlapping labels of one class (3, and 36 moved 5 px below it): each detection takes the better one
    gt[0, 36, 1:] = _lab(3) + np.array([0.0, 5.0, 0.0, 5.0])
    rows[20], rows[21] = (_lab(3) + np.array([0.0, 1.0, 0.0, 1.0]), 0), (_lab(3) + np.array([0.0, 4.0, 0.0, 4.0]), 0)
    # class mismatch: full overlap with a label of another class
    rows[30], rows[31] = (_on(_lab(6), 30), 1), (_on(_lab(7), 30), 1)
    # IoU exactly on thresholds (20 x 20 labels, union 400: the eps is absorbed in f32; in f64 the quotient falls short)
    for j, (l, h) in enumerate(((40, 10), (41, 13), (42, 19), (43, 14))):
        rows[40 + j] = (_on(gt[0, l, 1:3], float(h), 20.0), 1)
        on_thr.append((0, l, 40 + j))
    # ordinary matches and misses over the rest
    for d in range(n0):
        if d not in rows:
            l = 8 + d % 30
            rows[d] = (_on(_lab(l), (16, 17, 19, 20, 22, 23, 25, 26, 28, 29)[(d * 7) % 10]) if d % 4 == 0 else np.array([2000.0 + d, 2000.0, 2010.0 + d, 2010.0]), l % 3 if d % 8 else (l + 1) % 3)
    for d, (box, c) in rows.items():
        det[0, d] = (*box, 0.9 - 0.001 * d, c)
    # rows at and past counts[0]: boxes that would match
    for d in range(n0, max_det):
        det[0, d] = (*_on(_lab(9), 30), 0.1, 0)
    # image 1: detections, no label (the label rows hold matching boxes that ngt = 0 hides); image 2: labels, no detection
    det[1, :50], gt[1, :44] = det[0, :50], gt[0, :44]
    det[2, :50], gt[2, :44] = det[0, :50], gt[0, :44]
    iouv = IOUV.copy()
    if custom_iouv:  # one ulp above the quotients 13/20 and 14/20: those detections now miss that threshold
        iouv[3], iouv[4] = np.nextafter(F32(260) / F32(400), F32(1)), np.nextafter(F32(280) / F32(400), F32(1))
    return MatchScene(f"match{max_det}{'_ulp' if custom_iouv else ''}", det, [n0, 50, 0], gt, [ngt0, 0, 44], iouv, on_thr)


def match_scene_clamped(max_det: int) -> MatchScene:
    """counts[b] > max_det and ngt[b] > max_gt: both clamped to the buffers; B = 2, ragged."""
    base = match_scene(max_det)
    det, gt = base.det[:2].copy(), base.gt[:2].copy()
    det[1], gt[1] = det[0], gt[0]
    for l in range(44, 64):  # fill every label row
        gt[:, l] = (l % 3, *_lab(l))
    return MatchScene(f"match{max_det}_clamped", det, [max_det + 50, max_det], gt, [100, 64], IOUV, base.on_thr | {(1, l, d) for _, l, d in base.on_thr})
