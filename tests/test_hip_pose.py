"""-m gpu: pose estimation on the HIP path against the CPU checker tests/pose_oracle.py and the reference goldens: the keypoint decode
(`upa_kpt_decode_rows`, every layout), the zero-padded 51-channel cv4 chain, the Pose head (legacy and depthwise class branch, nc = 1),
the keypoint columns behind NMS, `upa_scale_coords`, and the whole yolov8n-pose / yolov11n-pose models (f32 parity, bf16 smooth family
under three dispatches, graph replay, pipelined copies, refusals)."""

import contextlib

import numpy as np
import pytest
import torch

from oracle import nms as onms
from tests import kernel_check as KC
from tests import pose_oracle as PO
from tests import pose_cases as GP
from ultralytics_pro_amd.utils import procedural as P

pytestmark = pytest.mark.gpu
TOL = 1e-3
THROUGHPUT = dict(c2f=4, conv_ws3=1, c2f_stream_rows=-1, detect_stream=2, conv_big=2)  # engine/pipeline.py PipelinedRunner.throughput_opts
# The device sigmoid: the bound tests/test_hip_ops.py:978 (test_detect_decode_vs_oracle_random_logits) allows Detect's class scores, on
# the same logit range (-8, 8), for f32 and bf16 inputs alike.
SIGMOID_TOL = 2e-6
# bf16 keypoint gate on the smooth family: TWICE the CPU emulation's own distance, stored in tests/pose_cases.py and reproduced on the CPU
# by tests/test_pose_oracle.py::test_bf16_emulation_distance_reproduces_the_stored_gate.
BF16_KPT_EMUL = GP.BF16_KPT_EMUL


def _dispatch(which):
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    if which == "session":
        return contextlib.nullcontext()
    if which == "serial":
        return R.use_opts(L.Opts())
    return R.use_opts(**THROUGHPUT)


# ---- upa_kpt_decode_rows ----------------------------------------------------------------------------------------------------------------

# 9 x 11 = 99 pixels: a second 64-pixel tile (blockIdx.x = 1), a tail tile after a full one
MAPS = [(2, 5, 7, 8.0), (1, 1, 1, 32.0), (3, 4, 4, 16.0), (1, 9, 11, 8.0)]


def _decode_ref(v, w, stride, ndim):
    """v: (n, nk, h * w) f32 -> (x / y by the formula, bit-exact in f32; visibility by torch.sigmoid)."""
    hw = v.shape[2]
    gx = (torch.arange(hw) % w).float()
    gy = (torch.arange(hw) // w).float()
    y = v.clone()
    y[:, 0::ndim] = (v[:, 0::ndim] * 2.0 + gx) * stride
    y[:, 1::ndim] = (v[:, 1::ndim] * 2.0 + gy) * stride
    if ndim == 3:
        y[:, 2::ndim] = torch.sigmoid(v[:, 2::ndim])
    return y


@KC.stop_after_fault
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kshape", [(17, 3), (5, 2)], ids=["nk51", "nk10"])
@pytest.mark.parametrize("layout", ["c56_ld64", "slice", "odd_rows"])
def test_kpt_decode_rows(layout, kshape, dtype):
    """Four maps (odd sizes, one pixel, several images, two tiles) x two keypoint shapes x three layouts: c = 56 channels at ldx = 64; a channel
    slice of exactly nk channels at an offset of 3 elements (no 16-byte loads); a0 = 5 in rows of a_total = hw + 9 floats (no 16-byte
    stores).  Raw output on and off.  x / y bit-equal to the formula, visibility within SIGMOID_TOL, guard bands intact, two runs equal."""
    DEV, L, lib, stream = KC.env()
    nkpt, ndim = kshape
    nk = nkpt * ndim
    for (n, h, w, stride) in MAPS:
        hw = h * w
        v = KC.unit_input(f"kptdec:{n}:{h}:{w}:{nk}", (n, h, w, nk), -8.0, 8.0)
        if dtype == torch.bfloat16:
            v = v.to(torch.bfloat16).float()
        if layout == "c56_ld64":
            c, ldx, off = max(56, (nk + 7) // 8 * 8), 64, 0
        elif layout == "slice":
            c, ldx, off = nk, 64, 3
        else:
            c, ldx, off = (nk + 7) // 8 * 8, 64, 0
        a0, a_total = (5, hw + 9) if layout == "odd_rows" else (8, hw + 16 + (-hw) % 4)
        ref = _decode_ref(v.permute(0, 3, 1, 2).reshape(n, nk, hw).contiguous(), w, stride, ndim)
        for with_raw in (True, False):
            def run():
                x = torch.full((n + 1, h, w, ldx), 7.0, dtype=dtype, device=DEV)
                x[:n, ..., off:off + nk] = v.to(dtype).to(DEV)
                out = KC.out_buf((n, nk), a_total, torch.float32, spare=1)
                raw = KC.out_buf((n, nk), a_total, torch.float32, spare=1)
                rc = lib.upa_kpt_decode_rows(x.data_ptr() + off * x.element_size(), n, h, w, c, ldx, L.dtype_code(dtype), nkpt, ndim, stride,
                                             out.data_ptr(), a_total, a0, raw.data_ptr() if with_raw else None, stream)
                L.check(rc, "kpt_decode_rows")
                torch.cuda.synchronize()
                return out, raw
            out, raw = KC.twice(run, "kpt_decode_rows")
            what = f"{layout} {kshape} {dtype} map {(n, h, w)} raw={with_raw}"
            y = KC.payload(out, n, hw, what, offset=a0)
            for d in range(2):
                assert KC.same_bits(y[:, d::ndim], ref[:, d::ndim]), f"{what}: coordinate {d} is not the formula's bits"
            if ndim == 3:
                KC.check_bound(y[:, 2::3], ref[:, 2::3], SIGMOID_TOL, what + " visibility")
            if with_raw:
                r = KC.payload(raw, n, hw, what + " raw", offset=a0)
                assert KC.same_bits(r, v.permute(0, 3, 1, 2).reshape(n, nk, hw).contiguous())
            else:
                assert bool(torch.isnan(raw).all()), what + ": raw written without being asked for"


@KC.stop_after_fault
def test_kpt_decode_refusals_leave_the_outputs_untouched():
    DEV, L, lib, stream = KC.env()
    x = torch.zeros((1, 4, 4, 160), device=DEV)
    out = torch.full((1, 160, 16), float("nan"), device=DEV)
    raw = torch.full((1, 160, 16), float("nan"), device=DEV)

    def call(c=56, ldx=160, dtype=0, nkpt=17, ndim=3, a0=0, a_total=16, null=False):
        rc = lib.upa_kpt_decode_rows(None if null else x.data_ptr(), 1, 4, 4, c, ldx, dtype, nkpt, ndim, 8.0, out.data_ptr(), a_total, a0,
                                     raw.data_ptr(), stream)
        torch.cuda.synchronize()
        return rc, bool(torch.isnan(out).all()) and bool(torch.isnan(raw).all())

    assert call(dtype=2) == (L.UPA_EUNSUPPORTED, True)            # neither f32 nor bf16
    assert call(ndim=4, c=160) == (L.UPA_EUNSUPPORTED, True)      # a keypoint is 2 or 3 values
    assert call(nkpt=50, c=160) == (L.UPA_EUNSUPPORTED, True)     # nk = 150 > 128
    assert call(c=48) == (L.UPA_EINVAL, True)                     # fewer channels than keypoint values
    assert call(a0=1) == (L.UPA_EINVAL, True)                     # the level's anchors run past the row
    assert call(ldx=40) == (L.UPA_EINVAL, True)                   # pixel stride below the channel count
    assert call(null=True) == (L.UPA_EINVAL, True)
    assert call() == (0, False)                                   # the accepted form writes


# ---- the padded cv4 chain -----------------------------------------------------------------------------------------------------------------

def _heads(legacy, nc, kshape, dtype=torch.float32):
    from tests.hip_utils import DEV, bn_fix
    from tests.test_pose_oracle import oracle_head
    from ultralytics_pro_amd.nn.modules.head import Pose
    o, xs = oracle_head(legacy, nc, kshape)
    old = Pose.legacy
    Pose.legacy = legacy
    try:
        p = bn_fix(Pose(nc, kshape, GP.HEAD_CH))
    finally:
        Pose.legacy = old
    p.stride = torch.tensor([8.0, 16.0, 32.0])
    p.bias_init()
    P.apply_procedural_weights(p, family="yolov8n-pose")
    return o, p.to(DEV).eval(), xs


def _chain_f64(seq, x, round_bf16=False):
    """cv4[i] in float64 with the BatchNorm folded as the product folds it; with `round_bf16` the operands the bf16 kernels multiply
    (weights, input, intermediates rounded to bf16)."""
    from oracle import modules as om
    from tests.hip_utils import bf16_round
    import copy
    rnd = bf16_round if round_bf16 else (lambda t: t)
    t, outs = rnd(x), []
    for k, m in enumerate(seq):
        if k < 2:
            m = copy.deepcopy(m)
            conv = om.fuse_conv_and_bn(m.conv, m.bn)
            w, b = conv.weight.detach(), conv.bias.detach()
            z = torch.nn.functional.conv2d(t.double(), rnd(w).double(), b.double(), padding=1)
            t = rnd((z * torch.sigmoid(z)).float())
        else:
            t = rnd(torch.nn.functional.conv2d(t.double(), rnd(m.weight.detach()).double(), m.bias.detach().double()).float())
        outs.append(t)
    return outs


@KC.stop_after_fault
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_padded_cv4_chain_pad_channels_zero_real_channels_exact(dtype):
    """ch = (16, 32, 64) gives c4 = nk = 51: every intermediate is 56 channels wide, channels 51.. are exactly zero and the real ones
    match an unpadded float64 chain (f32: rel_err <= 1e-5; bf16: assert_bf16_close against the chain on bf16-rounded operands)."""
    from tests.hip_utils import DEV, assert_bf16_close, rel_err, to_cpu_nchw, to_dev_nhwc
    o, p, xs = _heads(True, 1, (17, 3))
    assert p.cv4[0][0].conv.out_channels == 51
    for i, x in enumerate(xs):
        with torch.no_grad():
            outs = [to_cpu_nchw(t) for t in p.kpt_chain(i, to_dev_nhwc(x, dtype))]
            refs = _chain_f64(o.cv4[i], x, round_bf16=dtype == torch.bfloat16)
        for k, (y, r) in enumerate(zip(outs, refs)):
            assert y.shape[1] == 56 and r.shape[1] == 51
            assert bool((y[:, 51:] == 0).all()), f"level {i} conv {k}: a pad channel is not zero"
            if dtype == torch.float32:
                assert rel_err(y[:, :51], r) <= 1e-5, (i, k, rel_err(y[:, :51], r))
            else:
                assert_bf16_close(y[:, :51], r, f"level {i} conv {k}")


# ---- the head against the reference goldens ---------------------------------------------------------------------------------------------

@KC.stop_after_fault
@pytest.mark.parametrize("case", GP.HEAD_CASES, ids=[c[0] for c in GP.HEAD_CASES])
def test_pose_head_matches_reference_golden(case, golden_dir):
    """f32: (cat([y, pred_kpt], 1), (raw, kpt)) against ops_pose.npz - the legacy and the depthwise class branch at nc = 1, and a
    (5, 2) keypoint shape at nc = 3; the parts travel with the concatenated tensor."""
    from tests.hip_utils import DEV, rel_err
    from ultralytics_pro_amd.engine import runtime as R
    g = np.load(golden_dir / "ops_pose.npz")
    tag, legacy, nc, kshape = case
    _, p, xs = _heads(legacy, nc, kshape)
    with torch.no_grad():
        cat, (raw, kpt) = p([R.to_nhwc(t.to(DEV).contiguous(), torch.float32) for t in xs])
    torch.cuda.synchronize()
    y, pk = cat._upa_parts
    nk = kshape[0] * kshape[1]
    assert cat.shape == (2, 4 + nc + nk, 58) and torch.equal(cat[:, :4 + nc], y) and torch.equal(cat[:, 4 + nc:], pk)
    ref = torch.from_numpy(g[tag])
    assert rel_err(cat.cpu(), ref) <= 1e-4, rel_err(cat.cpu(), ref)
    assert float((cat.cpu()[:, 4:4 + nc] - ref[:, 4:4 + nc]).abs().max()) <= 1e-5
    assert rel_err(kpt.cpu(), torch.from_numpy(g[tag + "_kpt"])) <= 1e-4


@KC.stop_after_fault
@pytest.mark.parametrize("legacy", [True, False], ids=["v8", "v11"])
def test_pose_head_bf16_nc1_forms_match_the_bf16_weight_oracle(legacy):
    """nc = 1 through Detect's bf16 inference forms (fused tails, grouped levels; the level-stream and stacked-first forms do not
    apply to a 64-channel class branch): scores and boxes against the oracle on bf16-rounded weights and inputs."""
    from tests.hip_utils import DEV, bf16_round, bf16_weight_oracle
    from ultralytics_pro_amd.engine import runtime as R
    o, p, xs = _heads(legacy, 1, (17, 3))
    ob = bf16_weight_oracle(o)
    xb = [bf16_round(t) for t in xs]
    with torch.no_grad():
        ref = ob([t.clone() for t in xb])[0]
        for opts in (dict(), THROUGHPUT):
            with R.use_opts(**opts):
                cat, _ = p([R.to_nhwc(t.to(DEV).contiguous(), torch.bfloat16) for t in xb])
            torch.cuda.synchronize()
            d = (cat.cpu() - ref).abs()
            print(f"bf16 nc=1 legacy={legacy} {opts}: box {float(d[:, :4].max()):.3f} px score {float(d[:, 4].max()):.5f} kpt xy "
                  f"{float(d[:, 5:][:, [k for k in range(51) if k % 3 != 2]].max()):.3f} px")
            assert float(d[:, :4].max()) <= 0.5 and float(d[:, 4].max()) <= 0.005


# ---- NMS rows -----------------------------------------------------------------------------------------------------------------------------

@KC.stop_after_fault
@pytest.mark.parametrize("multi_label", [False, True], ids=["single", "multi"])
def test_nms_rows_carry_keypoints(multi_label):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.utils.ops import pose_postprocess_raw
    b, nc, nk, a = 3, 2, 51, 2100
    xy = P.uniform("unit:posenms:xy", (b, 2, a), 0.0, 640.0)
    wh = P.uniform("unit:posenms:wh", (b, 2, a), 4.0, 120.0)
    sc = P.uniform("unit:posenms:sc", (b, nc, a), 0.0, 1.0) ** 6
    kp = P.uniform("unit:posenms:kp", (b, nk, a), -30.0, 670.0)
    y = torch.cat([xy, wh, sc], 1)
    ref, idx = onms.non_max_suppression(y.clone(), 0.25, 0.7, multi_label=multi_label, return_idxs=True)
    for pred in ("plain", "parts"):
        t = torch.cat([y, kp], 1).to(DEV)
        if pred == "parts":
            t._upa_parts = (y.to(DEV).contiguous(), kp.to(DEV).contiguous())
        rows, counts, _ = pose_postprocess_raw(t, 0.25, 0.7, nc=nc, multi_label=multi_label)
        torch.cuda.synchronize()
        assert counts.tolist() == [r.shape[0] for r in ref]
        for i, (r, k) in enumerate(zip(ref, idx)):
            o = rows[i, :r.shape[0]].cpu()
            assert torch.equal(o[:, :6], r) and torch.equal(o[:, 6:], kp[i][:, k.long()].t()), (pred, i)
            assert bool((rows[i, r.shape[0]:] == 0).all())


# ---- upa_scale_coords -----------------------------------------------------------------------------------------------------------------------

@KC.stop_after_fault
@pytest.mark.parametrize("case", GP.COORD_CASES, ids=[c[0] for c in GP.COORD_CASES])
def test_scale_coords(case, golden_dir):
    """Rows of stride 6 + nk (57 for 17 x 3), images with counts 0, 7 and max_det, padding on and off, ndim 2 and 3, a ratio_pad:
    the first counts rows equal the reference's scale_coords (one f32 rounding per operation: 1e-4 px), every other float - the box
    columns, the visibility, rows past counts, the guard row - keeps its bits.  The public scale_coords on the golden's own input."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.utils import ops as O
    g = np.load(golden_dir / "ops_pose.npz")
    name, img1, img0, padding, ndim, rp = case
    nkpt, max_det = 17, 23
    c = P.uniform(f"unit:coords:{name}", (max_det, nkpt, ndim), -40.0, max(img1) + 40.0)
    ref = torch.from_numpy(g[f"coords_{name}"])
    out = O.scale_coords(img1, c.clone().to(DEV), img0, ratio_pad=rp, padding=padding)
    torch.cuda.synchronize()
    assert float((out.cpu() - ref).abs().max()) <= 1e-4
    if ndim == 3:
        assert torch.equal(out.cpu()[..., 2], c[..., 2])
    ld = 6 + nkpt * ndim
    counts = [0, 7, max_det]
    rows = torch.full((len(counts) + 1, max_det, ld), 3.25)
    rows[:3, :, 6:] = c.reshape(max_det, -1)
    before = rows.clone()
    dev_rows = rows.to(DEV)
    gain, px, py = O._coords_geometry(img1, img0, rp)
    cnt = torch.tensor(counts, dtype=torch.int32, device=DEV)

    def run():
        t = dev_rows.clone()
        KC.env()[1].check(KC.env()[2].upa_scale_coords(t.data_ptr(), 3, max_det, ld, 6, nkpt, ndim, cnt.data_ptr(), float(gain), float(px),
                                                       float(py), int(padding), float(img0[1]), float(img0[0]), KC.env()[3]), "scale_coords")
        torch.cuda.synchronize()
        return t
    got = KC.twice(run, "scale_coords").cpu()
    for i, k in enumerate(counts):
        if k:
            assert float((got[i, :k, 6:].reshape(k, nkpt, ndim) - ref[:k]).abs().max()) <= 1e-4, (name, i)
        assert KC.same_bits(got[i, k:], before[i, k:]), f"{name}: image {i}: a row past counts changed"
        assert KC.same_bits(got[i, :, :6], before[i, :, :6])
    assert KC.same_bits(got[3], before[3])


# ---- whole model ----------------------------------------------------------------------------------------------------------------------

def _build(name, dtype, family=None):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.nn.tasks import PoseModel
    m = PoseModel(name + ".yaml")
    P.apply_procedural_weights(m, family=family or name)
    m = m.to(DEV).eval()
    m.set_compute_dtype(dtype)
    return m


_kpt_split = PO.kpt_split


@KC.stop_after_fault
@pytest.mark.parametrize("name", ["yolov8n-pose", "yolov11n-pose"])
def test_e2e_f32_matches_reference_golden(name, golden_dir):
    from tests.hip_utils import DEV
    from tests.postprocess_ref import scale_boxes_ref
    from ultralytics_pro_amd.utils.ops import pose_postprocess, pose_postprocess_raw
    from ultralytics_pro_amd.utils.parity import rows_equivalent, split_rows
    g = np.load(golden_dir / f"e2e_{name}.npz")
    nc, conf = int(g["nc"]), float(g["conf_thres"])
    m = _build(name, torch.float32)
    with torch.no_grad():
        preds = m(P.synthetic_images(2).to(DEV))
        rows, counts, _ = pose_postprocess_raw(preds, conf, 0.7, max_det=300)
        per = pose_postprocess(preds, conf, 0.7, max_det=300, orig_shapes=[(480, 600), (640, 640)])
    torch.cuda.synchronize()
    d = np.abs(preds[0].cpu()[:, :, g["anchor_sel"]].numpy() - g["y_sel"])
    box, score, kxy, kvis = _kpt_split(d, nc)
    print(f"{name} f32: max|box d|={box:.3e} max|score d|={score:.3e} max|kpt d|={kxy:.3e} max|vis d|={kvis:.3e}")
    assert box <= TOL and kxy <= TOL and score <= TOL and kvis <= TOL
    ref = split_rows(g["predict_rows"], g["predict_n"])
    n = counts.tolist()
    mine = [rows[i, :n[i]].cpu().numpy() for i in range(2)]
    assert rows_equivalent([r[:, :6] for r in mine], [r[:, :6] for r in ref])
    decided = len(np.unique(g["predict_rows"][:, 4])) == g["predict_rows"].shape[0]  # yolov11n-pose saturates: equal scores, a set of rows
    for i in range(2):
        assert mine[i].shape == ref[i].shape
        if decided:
            assert np.abs(mine[i] - ref[i]).max(initial=0) <= TOL, f"image {i}"
        else:  # a set of rows: every reference row has a row of mine with its box, score and class, and that row carries its keypoints
            for r in ref[i]:
                near = np.abs(mine[i][:, :6] - r[:6]).max(1) <= TOL
                assert near.any() and (np.abs(mine[i][near] - r).max(1) <= TOL).any(), f"image {i}: no row with this box carries its keypoints"
    # back to the original frame: the keypoints against the checker's scale_coords of the product's own network-frame rows
    for i, shape in enumerate([(480, 600), (640, 640)]):
        boxes, kpts = per[i]
        assert kpts.shape == (n[i], 17, 3) and boxes.shape == (n[i], 6)
        if n[i]:
            want = PO.scale_coords((640, 640), torch.from_numpy(mine[i][:, 6:]).reshape(-1, 17, 3), shape)
            assert float((kpts.cpu() - want).abs().max()) <= TOL
            want_b = scale_boxes_ref((640, 640), mine[i][:, :6], shape, dtype=np.float32)
            assert np.abs(boxes.cpu().numpy() - want_b).max() <= TOL and np.array_equal(boxes.cpu().numpy()[:, 4:], mine[i][:, 4:6])


@KC.stop_after_fault
@pytest.mark.parametrize("dispatch", ["session", "serial", "throughput"])
@pytest.mark.parametrize("name", ["yolov8n-pose", "yolov11n-pose"])
def test_e2e_bf16_smooth_family_matches_reference_golden(name, dispatch, golden_dir):
    """bf16 on the smooth family vs the reference's f32 outputs over the sampled head rows: boxes and scores within the AMP tolerance
    of the detection tests (0.5 px, 0.005); keypoints within twice the CPU bf16 emulation's own distance (BF16_KPT_EMUL)."""
    from tests.hip_utils import DEV
    g = np.load(golden_dir / f"e2e_{name}_smooth.npz")
    nc = int(g["nc"])
    m = _build(name, torch.bfloat16, family=f"smooth:{name}")
    x = P.synthetic_images(2).to(DEV).to(torch.bfloat16).contiguous()
    with torch.no_grad(), _dispatch(dispatch):
        preds = m(x)
    torch.cuda.synchronize()
    d = np.abs(preds[0].cpu()[:, :, g["anchor_sel"]].numpy() - g["y_sel"])
    box, score, kxy, kvis = _kpt_split(d, nc)
    exy, evis = BF16_KPT_EMUL[name]
    print(f"{name} smooth bf16 [{dispatch}]: box {box:.3f} px score {score:.4f} kpt {kxy:.3f} px (gate {2 * exy:.2f}) vis {kvis:.4f} "
          f"(gate {2 * evis:.4f})")
    assert box <= 0.5 and score <= 0.005
    assert kxy <= 2 * exy and kvis <= 2 * evis


@KC.stop_after_fault
def test_e2e_graph_replay_and_pipelined_copies_equal_eager():
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.engine.pipeline import PipelinedRunner
    from ultralytics_pro_amd.utils.ops import pose_postprocess_raw
    for name, dt in (("yolov8n-pose", torch.float32), ("yolov11n-pose", torch.bfloat16)):
        m = _build(name, dt, family=f"smooth:{name}")
        x = P.synthetic_images(2).to(DEV).to(dt).contiguous()
        post = lambda o: pose_postprocess_raw(o, 0.05, 0.7, max_det=100, key="pose_replay")  # noqa: E731
        with torch.no_grad():
            e = post(m(x))
            torch.cuda.synchronize()
            eager = [t.clone() for t in e]
            run = m.compile(x, post=post)
            r1 = [t.clone() for t in run()]
            r2 = run()
        torch.cuda.synchronize()
        assert int(eager[1].sum()) > 0, name
        for a, b, c in zip(eager[:2], r1[:2], r2[:2]):
            assert torch.equal(a, b) and torch.equal(a, c), name
    m = _build("yolov8n-pose", torch.bfloat16, family="smooth:yolov8n-pose")
    x = P.synthetic_images(4).to(DEV).to(torch.bfloat16).contiguous()
    mk = lambda key: (lambda o: pose_postprocess_raw(o, 0.05, 0.7, max_det=100, key=key))  # noqa: E731
    with torch.no_grad():
        with R.use_opts(**THROUGHPUT):
            run1 = m.compile(x, post=mk("pose_ref"))
        ref = [t.clone() for t in run1()]
        torch.cuda.synchronize()
        runner = PipelinedRunner(m, x, post=mk("pose_pipe"), micro_batches=2, in_flight=3)
        for _ in range(4):
            runner.step()
        torch.cuda.synchronize()
    assert int(ref[1].sum()) > 0
    for parts in runner.results():
        assert torch.equal(torch.cat([p_[1] for p_ in parts], 0), ref[1]) and torch.equal(torch.cat([p_[0] for p_ in parts], 0), ref[0])


@KC.stop_after_fault
def test_pose_cat_out_switch():
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.utils.ops import pose_postprocess_raw
    m = _build("yolov8n-pose", torch.float32)
    x = P.synthetic_images(1, h=320, w=320).to(DEV)
    with torch.no_grad():
        cat, (raw, kpt) = m(x)
        cat = cat.clone()
        r_cat = [t.clone() for t in pose_postprocess_raw((cat, None), 0.01, 0.7, nc=1)]
        m.model[-1].cat_out = False
        try:
            y, (_, kpt2) = m(x)
            r_y = [t.clone() for t in pose_postprocess_raw((y, None), 0.01, 0.7)]
        finally:
            m.model[-1].cat_out = True
    torch.cuda.synchronize()
    assert y.shape == (1, 5, 2100) and cat.shape == (1, 56, 2100) and kpt.shape == (1, 51, 2100)
    assert torch.equal(cat[:, :5], y) and torch.equal(cat[:, 5:], y._upa_parts[1]) and torch.equal(kpt, kpt2)
    assert int(r_cat[1].sum()) > 0 and torch.equal(r_cat[0], r_y[0]) and torch.equal(r_cat[1], r_y[1])
