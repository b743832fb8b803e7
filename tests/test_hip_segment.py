"""-m gpu: instance segmentation on the HIP path against the CPU checker tests/segment_oracle.py and the reference goldens: the Proto
upsampling conv (`upa_conv_transpose2x2`), the coefficient gather behind NMS (`upa_nms_gather_extra`), the mask kernel
(`upa_process_mask`, every form, the ragged layout and its overflow report) and the whole yolov8n-seg / yolov11n-seg models (f32
parity, bf16 smooth family under three dispatches, graph replay, pipelined copies)."""

import contextlib

import numpy as np
import pytest
import torch

from oracle import nms as onms
from tests import segment_oracle as S
from ultralytics_pro_amd.utils import procedural as P

pytestmark = pytest.mark.gpu
TOL = 1e-3
THROUGHPUT = dict(c2f=4, conv_ws3=1, c2f_stream_rows=-1, detect_stream=2, conv_big=2)  # engine/pipeline.py PipelinedRunner.throughput_opts
# bf16 smooth family: the smallest per-instance mask IoU against the reference's f32 masks.  Measured on an MI355X under the three
# dispatches: yolov8n-seg 0.953 / 0.995 / 1.0 (session, serial), 0.984 / 1.0 / 1.0 (throughput); yolov11n-seg 0.930 - 0.990 (six
# instances of 313 - 475 px: one pixel is 0.2 - 0.3 % of IoU).  The floor sits a few percent under the measured minimum, 0.930.
BF16_MASK_IOU_FLOOR = 0.90


def _dispatch(which):
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    if which == "session":
        return contextlib.nullcontext()
    if which == "serial":
        return R.use_opts(L.Opts())
    return R.use_opts(**THROUGHPUT)


def _unpack(a, w):
    return np.unpackbits(a, axis=-1)[..., :w].astype(bool)


def _iou(a, b):
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    u = np.logical_or(a, b).sum()
    return 1.0 if u == 0 else float(np.logical_and(a, b).sum()) / float(u)


def _assert_masks(mine, ref_vals, what):
    """f32 mask rule: every pixel agrees where the checker's pre-threshold value has |v| > 1e-4 max|v|; per-instance IoU >= 0.999."""
    mine = np.asarray(mine, bool)
    v = ref_vals.numpy() if torch.is_tensor(ref_vals) else ref_vals
    ref = v > 0
    for k in range(v.shape[0]):
        sure = np.abs(v[k]) > 1e-4 * max(float(np.abs(v[k]).max()), 1e-30)
        bad = int((mine[k] != ref[k])[sure].sum())
        assert bad == 0, f"{what}: instance {k}: {bad} confident pixels differ"
        assert _iou(mine[k], ref[k]) >= 0.999, f"{what}: instance {k}: IoU {_iou(mine[k], ref[k]):.5f}"


# ---- ConvTranspose2d(2, 2) ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("cin,cout,hw", [(64, 64, (20, 20)), (32, 48, (7, 9)), (128, 16, (3, 5)), (8, 8, (1, 1)), (256, 64, (40, 40))])
def test_conv_transpose2x2_vs_oracle(cin, cout, hw):
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, rel_err, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd.nn.modules.block import hip_conv_transpose2x2
    ct = torch.nn.Sequential(torch.nn.ConvTranspose2d(cin, cout, 2, 2, 0, bias=True))
    P.apply_procedural_weights(ct, family="yolov8n-seg")
    owner = torch.nn.Module()
    x = P.uniform(f"unit:ct:{cin}:{cout}:{hw}", (2, cin, *hw), -1.0, 1.0)
    with torch.no_grad():
        ref = ct(x)
        y = to_cpu_nchw(hip_conv_transpose2x2(to_dev_nhwc(x), owner, ct[0].to(DEV)))
        assert rel_err(y, ref) <= 1e-5, rel_err(y, ref)
        ctb = torch.nn.ConvTranspose2d(cin, cout, 2, 2, 0, bias=True)
        ctb.weight.copy_(bf16_round(ct[0].weight.cpu()))
        ctb.bias.copy_(ct[0].bias.cpu())
        ref_b = ctb(bf16_round(x))
        yb = to_cpu_nchw(hip_conv_transpose2x2(to_dev_nhwc(x, torch.bfloat16), owner, ct[0]))
    assert_bf16_close(yb, ref_b, f"conv_transpose2x2 {cin}->{cout} {hw}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_conv_transpose2x2_channel_slice_views(dtype):
    """Input read from a channel slice of a wider NHWC buffer, output written into a channel slice; every other byte is untouched."""
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, rel_err
    from ultralytics_pro_amd.nn.modules.block import hip_conv_transpose2x2
    ct = torch.nn.Sequential(torch.nn.ConvTranspose2d(32, 16, 2, 2, 0, bias=True))
    P.apply_procedural_weights(ct, family="yolov8n-seg")
    x = P.uniform("unit:ct:slice", (2, 32, 5, 7), -1.0, 1.0)
    wide_in = torch.full((2, 5, 7, 96), 7.0, device=DEV, dtype=dtype)
    wide_in[..., 32:64] = x.permute(0, 2, 3, 1).to(DEV).to(dtype)
    xin = wide_in.permute(0, 3, 1, 2)[:, 32:64]
    out = torch.full((2, 10, 14, 64), -3.0, device=DEV, dtype=dtype)
    dst = out.permute(0, 3, 1, 2)[:, 16:32]
    with torch.no_grad():
        hip_conv_transpose2x2(xin, torch.nn.Module(), ct[0].to(DEV), out=dst)
        y = out[..., 16:32].permute(0, 3, 1, 2).float().cpu()
        wf = ct[0].weight.detach().cpu()
        ref = torch.nn.functional.conv_transpose2d(x if dtype == torch.float32 else bf16_round(x),
                                                   wf if dtype == torch.float32 else bf16_round(wf), ct[0].bias.detach().cpu(), stride=2)
    torch.cuda.synchronize()
    if dtype == torch.float32:
        assert rel_err(y, ref) <= 1e-5
    else:
        assert_bf16_close(y, ref, "conv_transpose2x2 slice")
    rest = torch.cat([out[..., :16], out[..., 32:]], -1)
    assert bool((rest == -3.0).all())


# ---- NMS with the coefficient columns --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("multi_label", [False, True], ids=["single", "multi"])
def test_nms_rows_carry_mask_coefficients(multi_label):
    """A Segment-shaped (B, 4+nc+nm, A) prediction: the (n, 6+nm) rows equal the checker's (n, 6) rows (boxes and scores exact, as
    NMS is) with the coefficients of the kept anchors (exact: a gather) - both from a plain concatenated tensor and from one that
    carries its parts."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.utils.nms import non_max_suppression
    b, nc, nm, a = 3, 80, 32, 2100
    xy = P.uniform("unit:segnms:xy", (b, 2, a), 0.0, 640.0)
    wh = P.uniform("unit:segnms:wh", (b, 2, a), 4.0, 120.0)
    sc = P.uniform("unit:segnms:sc", (b, nc, a), 0.0, 1.0) ** 6
    mc = P.uniform("unit:segnms:mc", (b, nm, a), -3.0, 3.0)
    y = torch.cat([xy, wh, sc], 1)
    cat = torch.cat([y, mc], 1)
    ref, idx = onms.non_max_suppression(y.clone(), 0.25, 0.7, multi_label=multi_label, return_idxs=True)
    for pred in ("plain", "parts"):
        t = cat.to(DEV)
        if pred == "parts":
            t._upa_parts = (y.to(DEV).contiguous(), mc.to(DEV).contiguous())
        out = non_max_suppression(t, 0.25, 0.7, multi_label=multi_label, nc=nc)
        assert [o.shape[0] for o in out] == [r.shape[0] for r in ref]
        for i, (o, r, k) in enumerate(zip(out, ref, idx)):
            o = o.cpu()
            assert o.shape[1] == 6 + nm
            assert torch.equal(o[:, :6], r), (pred, i)
            assert torch.equal(o[:, 6:], mc[i][:, k.long()].t()), (pred, i)


# ---- masks --------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case", S.mask_cases() + [("proto_n64", "mask:c", 64, 32, (40, 40), (160, 160), "proto")], ids=lambda c: c[0])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_process_mask_vs_oracle(case, dtype):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.utils import ops as O
    name, key, n, nm, mhw, shape, mode = case
    protos, coef, boxes = S.mask_inputs(key, n, nm, mhw, shape)
    pin = protos if dtype == torch.float32 else protos.to(torch.bfloat16).float()
    v, _ = S.mask_values((name, key, n, nm, mhw, shape, mode)) if dtype == torch.float32 else (None, None)
    if v is None:
        v = (S.process_mask_native_values(pin, coef, boxes, shape, "compare") if mode == "native"
             else S.process_mask_values(pin, coef, boxes, shape, mode == "up", "compare"))
    from ultralytics_pro_amd.engine import runtime as R
    p_dev = R.to_nhwc(pin[None].to(DEV).contiguous(), dtype)
    with torch.no_grad():
        if mode == "native":
            m = O.process_mask_native(p_dev, coef.to(DEV), boxes.to(DEV), shape)
        else:
            m = O.process_mask(p_dev, coef.to(DEV), boxes.to(DEV), shape, upsample=mode == "up")
    torch.cuda.synchronize()
    assert m.dtype == torch.uint8 and tuple(m.shape) == tuple(v.shape)
    _assert_masks(m.cpu().numpy() > 0, v, f"{name} {dtype}")


def test_process_mask_ragged_layout_overflow_and_flags():
    """Three images (counts n, 0, max_det), boxes touching and crossing the border: row base[i] + j holds (image i, detection j),
    rows past the capacity are not written, `total` reports the true count and `nonempty` flags exactly the masks with a pixel set."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.utils import ops as O
    nm, mh, mw, H, W, max_det = 32, 40, 48, 160, 192, 20
    counts = [7, 0, max_det]
    protos, dets, coefs = [], torch.zeros(3, max_det, 6 + nm), []
    for i, k in enumerate(counts):
        p, c, bx = S.mask_inputs(f"mask:rag{i}", max_det, nm, (mh, mw), (H, W))
        c[-1] = 0.0  # an all-zero coefficient row: empty mask
        protos.append(p)
        dets[i, :, :4], dets[i, :, 6:] = bx, c
    pdev = R.to_nhwc(torch.stack(protos).to(DEV).contiguous(), torch.float32)
    d = dets.to(DEV).contiguous()
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)
    total_rows = sum(counts)
    for cap in (total_rows, 10):
        spare = 3  # rows past the capacity: a sentinel that must survive
        masks_all = torch.full((cap + spare, H, W), 7, dtype=torch.uint8, device=DEV)
        flags_all = torch.full((cap + spare,), 5, dtype=torch.int32, device=DEV)
        masks, flags = masks_all[:cap], flags_all[:cap]
        total = torch.zeros(1, dtype=torch.int32, device=DEV)
        O._launch_process_mask(pdev, d[..., 6:], 6 + nm, d, 6 + nm, max_det, cnt, (H, W), False, (mw / W, mh / H), (0, 0, mh, mw),
                               masks, flags, cap, total)
        torch.cuda.synchronize()
        assert int(total.item()) == total_rows
        base = 0
        for i, k in enumerate(counts):
            for j in range(k):
                row = base + j
                if row >= cap:
                    continue
                v = S.process_mask_values(protos[i], dets[i, j:j + 1, 6:], dets[i, j:j + 1, :4], (H, W), True, "compare")
                mine = masks[row].cpu().numpy()[None] > 0
                _assert_masks(mine, v, f"ragged img {i} det {j} cap {cap}")
                assert int(flags[row].item()) == int(bool(mine.any())), (i, j)
            base += k
        assert bool((masks_all[cap:] == 7).all()) and bool((flags_all[cap:] == 5).all()), f"cap {cap}: rows past the capacity written"
        assert int(flags[total_rows - 1 if total_rows <= cap else cap - 1].item()) in (0, 1)
        if cap == total_rows:
            assert int(flags[total_rows - 1].item()) == 0  # the all-zero coefficient row of the last image
    with pytest.raises(L.UpaError):
        O._launch_process_mask(pdev, d[..., 6:], 6 + nm, d, 6 + nm, max_det, cnt, (H, W), False, (1.0, 1.0), (0, 0, mh + 1, mw),
                               masks, flags, 1, total)


# ---- whole model --------------------------------------------------------------------------------------------------------------------


def _build(name, dtype, family=None):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.nn.tasks import SegmentationModel
    m = SegmentationModel(name + ".yaml")
    P.apply_procedural_weights(m, family=family)
    m = m.to(DEV).eval()
    m.set_compute_dtype(dtype)
    return m


def _golden_masks(g):
    out, k0 = [], 0
    for k in g["mask_n"]:
        out.append(_unpack(g["masks_packed"][k0:k0 + int(k)], 640))
        k0 += int(k)
    return out


def _split(res):
    """segment_postprocess_raw output -> per image (rows (n, 6+nm), masks (n, H, W) bool) on the host."""
    n = res["counts"].cpu().tolist()
    masks = res["masks"].cpu().numpy() > 0
    out, base = [], 0
    for i, k in enumerate(n):
        out.append((res["rows"][i, :k].cpu().numpy(), masks[base:base + k]))
        base += k
    return out


@pytest.mark.parametrize("name", ["yolov8n-seg", "yolov11n-seg"])
def test_e2e_f32_matches_reference_golden(name, golden_dir):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.utils.ops import segment_postprocess_raw
    from ultralytics_pro_amd.utils.parity import rows_equivalent, split_rows
    g = np.load(golden_dir / f"e2e_{name}.npz")
    m = _build(name, torch.float32)
    with torch.no_grad():
        preds = m(P.synthetic_images(2).to(DEV))
        res = segment_postprocess_raw(preds, 0.25, 0.7, max_det=300)
    torch.cuda.synchronize()
    y = preds[0]
    d = np.abs(y.cpu()[:, :, g["anchor_sel"]].numpy() - g["y_sel"])
    print(f"{name} f32: max|box d|={d[:, :4].max():.3e} max|score d|={d[:, 4:84].max():.3e} max|coef d|={d[:, 84:].max():.3e}")
    assert d[:, :4].max() <= TOL and d[:, 4:].max() <= TOL
    per = _split(res)
    ref = split_rows(g["predict_rows"], g["predict_n"])
    assert rows_equivalent([r[:, :6] for r, _ in per], [r[:, :6] for r in ref])
    gm = _golden_masks(g)
    assert sum(int(m_.any()) for ms in gm for m_ in ms) * 2 > sum(len(ms) for ms in gm), "the stored masks are mostly empty"
    ious, k0 = [], 0
    for i, (rows, masks) in enumerate(per):
        k = len(gm[i])
        assert rows.shape[0] == ref[i].shape[0], f"image {i}: {rows.shape[0]} rows vs {ref[i].shape[0]}"
        assert np.abs(rows[:k, :6] - ref[i][:k, :6]).max(initial=0) <= TOL, f"image {i}: the mask-bearing rows differ"
        if k:
            # the reference's pre-threshold values at 640 x 640: its proto-resolution logits, cropped (comparison form), resampled
            logits = torch.from_numpy(g["mask_logits"][k0:k0 + k])
            v = S.crop_mask(logits, torch.from_numpy(ref[i][:k, :4]) * 0.25, "compare")
            v = torch.nn.functional.interpolate(v[None], (640, 640), mode="bilinear")[0]
            _assert_masks(masks[:k], v, f"{name} image {i}")
            ious += [_iou(masks[j], gm[i][j]) for j in range(k)]
            k0 += k
    print(f"{name} f32 mask IoU vs reference: {ious}")
    assert ious and min(ious) >= 0.999


@pytest.mark.parametrize("dispatch", ["session", "serial", "throughput"])
@pytest.mark.parametrize("name", ["yolov8n-seg", "yolov11n-seg"])
def test_e2e_bf16_smooth_family_matches_reference_golden(name, dispatch, golden_dir):
    """bf16 on the smooth family vs the reference's f32 outputs: sampled head rows within the AMP tolerance of the detection tests
    (0.5 px, 0.005 in score); matched instances' masks above BF16_MASK_IOU_FLOOR."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.utils.ops import segment_postprocess_raw
    from ultralytics_pro_amd.utils.parity import split_rows
    g = np.load(golden_dir / f"e2e_{name}_smooth.npz")
    m = _build(name, torch.bfloat16, family=f"smooth:{name}")
    x = P.synthetic_images(2).to(DEV).to(torch.bfloat16).contiguous()
    with torch.no_grad(), _dispatch(dispatch):
        preds = m(x)
        res = segment_postprocess_raw(preds, 0.25, 0.7, max_det=300)
    torch.cuda.synchronize()
    d = np.abs(preds[0].cpu()[:, :84][:, :, g["anchor_sel"]].numpy() - g["y_sel"][:, :84])
    per = _split(res)
    ref = split_rows(g["predict_rows"], g["predict_n"])
    gm = _golden_masks(g)
    ious = []
    for i, (rows, masks) in enumerate(per):
        for j in range(len(gm[i])):
            hit = [k for k in range(rows.shape[0]) if np.abs(rows[k, :4] - ref[i][j, :4]).max() <= 1.0 and rows[k, 5] == ref[i][j, 5]]
            if hit:
                ious.append(_iou(masks[hit[0]], gm[i][j]))
    print(f"{name} smooth bf16 [{dispatch}]: head box max|d| {d[:, :4].max():.3f} px score max|d| {d[:, 4:].max():.4f}; "
          f"detections {[r.shape[0] for r, _ in per]} vs {[r.shape[0] for r in ref]}; mask IoU {sorted(ious)}")
    assert d[:, :4].max() <= 0.5 and d[:, 4:].max() <= 0.005
    assert len(ious) >= sum(len(x) for x in gm) - 1
    assert min(ious) >= BF16_MASK_IOU_FLOOR


def test_e2e_graph_replay_equals_eager():
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.utils.ops import segment_postprocess_raw
    for name, dt in (("yolov8n-seg", torch.float32), ("yolov11n-seg", torch.bfloat16)):
        m = _build(name, dt, family=f"smooth:{name}")
        x = P.synthetic_images(2).to(DEV).to(dt).contiguous()
        post = lambda o: segment_postprocess_raw(o, 0.25, 0.7, max_det=100, capacity=256, key="seg_replay")  # noqa: E731
        with torch.no_grad():
            e = post(m(x))
            torch.cuda.synchronize()
            eager = {k: v.clone() for k, v in e.items()}
            run = m.compile(x, post=post)
            r1 = {k: v.clone() for k, v in run().items()}
            r2 = run()
        torch.cuda.synchronize()
        n = int(eager["total"].item())
        assert n > 0
        for k in ("rows", "counts", "total"):
            assert torch.equal(r1[k], eager[k]) and torch.equal(r2[k], eager[k]), (name, k)
        assert torch.equal(r1["masks"][:n], eager["masks"][:n]) and torch.equal(r2["masks"][:n], eager["masks"][:n])
        assert torch.equal(r1["nonempty"][:n], eager["nonempty"][:n])


def test_e2e_pipelined_runner_copies_equal_single_graph():
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.engine.pipeline import PipelinedRunner
    from ultralytics_pro_amd.utils.ops import segment_postprocess_raw
    m = _build("yolov8n-seg", torch.bfloat16, family="smooth:yolov8n-seg")
    x = P.synthetic_images(4).to(DEV).to(torch.bfloat16).contiguous()
    mk = lambda key: (lambda o: segment_postprocess_raw(o, 0.25, 0.7, max_det=100, capacity=256, key=key))  # noqa: E731
    with torch.no_grad():
        with R.use_opts(**THROUGHPUT):
            run1 = m.compile(x, post=mk("seg_ref"))
        ref = {k: v.clone() for k, v in run1().items()}
        torch.cuda.synchronize()
        runner = PipelinedRunner(m, x, post=mk("seg_pipe"), micro_batches=2, in_flight=3)
        for _ in range(4):
            runner.step()
        torch.cuda.synchronize()
    assert int(ref["total"].item()) > 0
    for parts in runner.results():
        rows = torch.cat([p_["rows"] for p_ in parts], 0)
        cnt = torch.cat([p_["counts"] for p_ in parts], 0)
        assert torch.equal(cnt, ref["counts"]) and torch.equal(rows, ref["rows"])
        masks = torch.cat([p_["masks"][:int(p_["total"].item())] for p_ in parts], 0)
        assert torch.equal(masks, ref["masks"][:int(ref["total"].item())])


def test_segment_cat_out_switch_and_trainer_refusal():
    """cat_out = False returns Detect's (B, 4+nc, A) output itself; the concatenated form equals cat([y, mc], 1)."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine.trainer import DetectionTrainer
    m = _build("yolov8n-seg", torch.float32)
    x = P.synthetic_images(1, h=320, w=320).to(DEV)
    with torch.no_grad():
        cat, (raw, mc, p) = m(x)
        cat = cat.clone()
        m.model[-1].cat_out = False
        try:
            y, (_, mc2, p2) = m(x)
        finally:
            m.model[-1].cat_out = True
    torch.cuda.synchronize()
    assert y.shape == (1, 84, 2100) and cat.shape == (1, 116, 2100) and tuple(p.shape) == (1, 32, 80, 80)
    assert torch.equal(cat[:, :84], y) and torch.equal(cat[:, 84:], mc2)
    with pytest.raises(L.UpaError):
        DetectionTrainer(m)


# ---- crop_mask / scale_masks, and the concatenated output at any anchor count ----------------------------------------------------------


@pytest.mark.parametrize("n", [0, 12, 64])
def test_crop_mask_vs_oracle(n):
    """crop_mask on float masks: bit-exact against the checker's comparison form (masks * bool), boxes crossing the border included."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.utils import ops as O
    protos, coef, boxes = S.mask_inputs("mask:crop", max(n, 2), 32, (40, 48), (160, 192))
    m = S.mask_logits(protos, coef)[:n]
    b = (boxes * 0.25)[:n]
    ref = S.crop_mask(m, b, "compare")
    out = O.crop_mask(m.to(DEV), b.to(DEV))
    torch.cuda.synchronize()
    assert out.shape == ref.shape and torch.equal(out.cpu(), ref)


@pytest.mark.parametrize("mhw,shape,padding", [((40, 40), (120, 200), True), ((32, 40), (90, 150), True), ((40, 48), (160, 192), False),
                                               ((40, 40), (20, 30), True)])
def test_scale_masks_vs_oracle(mhw, shape, padding):
    """scale_masks (letterbox window + bilinear): within f32 rounding of the checker's F.interpolate, up- and down-sampling."""
    from tests.hip_utils import DEV, rel_err
    from ultralytics_pro_amd.utils import ops as O
    protos, coef, _ = S.mask_inputs(f"mask:scale:{mhw}", 6, 32, mhw, shape)
    m = S.mask_logits(protos, coef)[None]
    ref = S.scale_masks(m, shape, padding)
    out = O.scale_masks(m.to(DEV), shape, padding)
    torch.cuda.synchronize()
    assert out.shape == ref.shape
    assert rel_err(out.cpu(), ref) <= 1e-5, rel_err(out.cpu(), ref)


def test_segment_cat_out_at_an_anchor_count_without_16_byte_rows():
    """nc = 1 on maps of 15 x 15, 8 x 8 and 4 x 4: (4 + nc) A = 1525 floats per image is no 16-byte multiple; the concatenated output
    still equals cat([y, mc], 1) of its parts, and y matches the checker."""
    from tests.hip_utils import DEV, bn_fix, rel_err
    from ultralytics_pro_amd.nn.modules.head import Segment
    from ultralytics_pro_amd.engine import runtime as R
    ch = (64, 128, 256)
    o = bn_fix(S.Segment(1, 32, 64, ch))
    p = bn_fix(Segment(1, 32, 64, ch))
    for mod in (o, p):
        mod.stride = torch.tensor([8.0, 16.0, 32.0])
        mod.bias_init()
        P.apply_procedural_weights(mod, family="yolov8n-seg")
    p = p.to(DEV).eval()
    xs = [P.uniform(f"unit:segcat:{i}", (2, c, s, s), -1.0, 1.0) for i, (c, s) in enumerate(zip(ch, (15, 8, 4)))]
    with torch.no_grad():
        ref = o([t.clone() for t in xs])[0]
        cat, (_, mc, _) = p([R.to_nhwc(t.to(DEV).contiguous(), torch.float32) for t in xs])
    torch.cuda.synchronize()
    y = cat._upa_parts[0]
    assert cat.shape == (2, 4 + 1 + 32, 305)
    assert torch.equal(cat[:, :5], y) and torch.equal(cat[:, 5:], mc)
    assert rel_err(cat.cpu(), ref) <= 1e-4, rel_err(cat.cpu(), ref)
