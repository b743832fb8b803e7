"""-m gpu: YOLO11 on the HIP path against the CPU checker tests/yolo11_oracle.py and the reference goldens: the depthwise conv
(`upa_dwconv2d`), the PSA attention (`upa_psa_attention`), every yolov11n C3k2 shape under the three dispatches, C2PSA, a non-legacy
Detect level, and the whole model (f32 parity, bf16 smooth family, other input sizes, graph replay, pipelined copies)."""

import contextlib
import copy

import numpy as np
import pytest
import torch

from oracle import modules as om
from oracle import nms as onms
from tests import yolo11_oracle as Y
from ultralytics_pro_amd.utils import procedural as P

pytestmark = pytest.mark.gpu
TOL = 1e-3
SMOOTH_BAND = 0.005
THROUGHPUT = dict(c2f=4, conv_ws3=1, c2f_stream_rows=-1, detect_stream=2, conv_big=2)  # engine/pipeline.py PipelinedRunner.throughput_opts


def _dispatch(which):
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    if which == "session":
        return contextlib.nullcontext()
    if which == "serial":
        return R.use_opts(L.Opts())
    return R.use_opts(**THROUGHPUT)


def _fold(o):
    """Oracle copy with every Conv's BN folded (f32 weights: what the f32 kernels and the depthwise / PSA kernels multiply)."""
    o = copy.deepcopy(o).eval()
    for m in o.modules():
        if isinstance(m, om.Conv) and hasattr(m, "bn"):
            om.fuse_conv_and_bn(m.conv, m.bn)
            del m.bn
            m.forward = m.forward_fuse
    return o


def _pair(cls_name, args, family="yolov11n"):
    from tests.hip_utils import DEV, bn_fix
    from ultralytics_pro_amd.nn.modules import block as B
    from ultralytics_pro_amd.nn.modules import conv as CV
    pcls = {"DWConv": CV.DWConv, "C3k2": B.C3k2, "C2PSA": B.C2PSA}[cls_name]
    o = bn_fix(Y.ORACLE_CLASSES[cls_name](*args))
    p = bn_fix(pcls(*args))
    P.apply_procedural_weights(o, family=family)
    P.apply_procedural_weights(p, family=family)
    return o, p.to(DEV).eval()


# ---- depthwise conv ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (20, 20), (80, 80)], ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("c", [8, 24, 64, 80, 128, 256])
def test_dwconv_vs_oracle(c, stride, hw):
    from tests.hip_utils import assert_bf16_close, bf16_round, rel_err, to_cpu_nchw, to_dev_nhwc
    o, p = _pair("DWConv", (c, c, 3, stride))
    x = P.uniform(f"unit:dw:{c}:{hw}", (2, c, *hw), -1.0, 1.0)
    of = _fold(o)
    with torch.no_grad():
        ref = of(x)
        y = to_cpu_nchw(p(to_dev_nhwc(x)))
        assert rel_err(y, ref) <= 1e-5, rel_err(y, ref)
        ref_b = of(bf16_round(x))
        yb = to_cpu_nchw(p(to_dev_nhwc(x, torch.bfloat16)))
    assert_bf16_close(yb, ref_b, f"dwconv c{c} s{stride} {hw}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dwconv_channel_slice_views(dtype):
    """Input read from and output written into channel slices of wider NHWC buffers; the rest of the output buffer is untouched."""
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, rel_err, to_cpu_nchw
    from ultralytics_pro_amd.engine import runtime as R
    o, p = _pair("DWConv", (64, 64, 3, 1))
    x = P.uniform("unit:dw:slice", (2, 192, 20, 20), -1.0, 1.0)
    xb = R.to_nhwc(x.to(DEV), dtype)
    out = R.alloc_nhwc(2, 160, 20, 20, dtype, DEV)
    out.fill_(7.0)
    with torch.no_grad():
        p(xb[:, 64:128], out=out[:, 32:96])
        ref = _fold(o)(x[:, 64:128] if dtype == torch.float32 else bf16_round(x[:, 64:128]))
    y = to_cpu_nchw(out)
    assert torch.all(y[:, :32] == 7.0) and torch.all(y[:, 96:] == 7.0)
    if dtype == torch.float32:
        assert rel_err(y[:, 32:96], ref) <= 1e-5
    else:
        assert_bf16_close(y[:, 32:96], ref, "dwconv slice")


def test_dwconv_unsupported_forms_raise():
    from tests.hip_utils import DEV, to_dev_nhwc
    from ultralytics_pro_amd import _lib as L
    for args in [(16, 16, 5, 1), (16, 16, 3, 3)]:
        _, p = _pair("DWConv", args)
        with pytest.raises(L.UpaError):
            p(to_dev_nhwc(torch.zeros(1, 16, 8, 8)))
    torch.cuda.synchronize(DEV)


# ---- PSA attention ----------------------------------------------------------------------------------------------------------------------

PSA_MAPS = {1: (1, 1), 7: (1, 7), 100: (10, 10), 240: (12, 20), 400: (20, 20), 1600: (40, 40)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("heads", [1, 2, 4])
@pytest.mark.parametrize("n_tok", list(PSA_MAPS))
def test_psa_attention_vs_oracle(n_tok, heads, dtype):
    """`upa_psa_attention` on the qkv conv's output vs the checker's attention core (softmax(scale q^T k) v + pe(v))."""
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, rel_err, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn.modules.block import v10_Attention
    dim = 64 * heads
    h, w = PSA_MAPS[n_tok]
    o = Y.v10_Attention(dim, num_heads=heads).eval()
    p = v10_Attention(dim, num_heads=heads).eval()
    for m in (o, p):
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.eps = 1e-3
        P.apply_procedural_weights(m, family="yolov11n")
    of = _fold(o)
    x = P.uniform(f"unit:psa:{n_tok}:{heads}", (2, dim, h, w), -2.0, 2.0)
    with torch.no_grad():
        qkv = of.qkv(x)
        if dtype == torch.bfloat16:
            qkv = bf16_round(qkv)
        ref = of.core(qkv, h, w)
        if n_tok >= 100:  # the softmax must not be degenerate (one-hot or flat): otherwise q / k mix-ups pass
            mx = of.probs(x).max(-1).values
            print(f"psa N={n_tok} heads={heads}: max probability median {float(mx.median()):.3f}, p90 {float(mx.quantile(0.9)):.3f}")
            assert float(mx.median()) < 0.5 and float(mx.median()) > 5.0 / n_tok
        vq = to_dev_nhwc(qkv, dtype)
        y = R.alloc_nhwc(2, dim, h, w, dtype, DEV)
        pw, pb = p.pe._dw_packed(p.pe.conv, p.pe.bn, DEV)
        a, b = R.view_of(vq), R.view_of(y)
        L.check(L.lib().upa_psa_attention(a.ptr, a.ld, 2, h, w, heads, 32, 64, float(o.scale), pw.data_ptr(), pb.data_ptr(), b.ptr, b.ld,
                                          a.dtype, L.current_stream(DEV)), "psa")
        yc = to_cpu_nchw(y)
    if dtype == torch.float32:
        assert rel_err(yc, ref) <= 1e-5, rel_err(yc, ref)
    else:
        assert_bf16_close(yc, ref, f"psa N={n_tok} heads={heads}")


def test_psa_attention_unsupported_head_dim_raises():
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    q = torch.zeros(1, 4, 4, 3 * 32, device=DEV)
    y = torch.zeros(1, 4, 4, 32, device=DEV)
    pw, pb = torch.zeros(9, 32, device=DEV), torch.zeros(32, device=DEV)
    rc = L.lib().upa_psa_attention(q.data_ptr(), 96, 1, 4, 4, 1, 16, 32, 0.25, pw.data_ptr(), pb.data_ptr(), y.data_ptr(), 32, L.UPA_F32,
                                   L.current_stream(DEV))
    assert rc == L.UPA_EUNSUPPORTED


# ---- blocks -----------------------------------------------------------------------------------------------------------------------------

# yolov11n's C3k2 rows: (layer, c1, c2, c3k, e, map); layers 6, 13, 16, 19 pass the C2f whole-block predicates (C2f._form64 / _form32up)
C3K2_ROWS = [(2, 32, 64, False, 0.25, 160), (4, 64, 128, False, 0.25, 80), (6, 128, 128, True, 0.5, 40), (8, 256, 256, True, 0.5, 20),
             (13, 384, 128, False, 0.5, 40), (16, 256, 64, False, 0.5, 80), (19, 192, 128, False, 0.5, 40), (22, 384, 256, True, 0.5, 20)]


@pytest.mark.parametrize("dispatch", ["session", "serial", "throughput"])
@pytest.mark.parametrize("row", C3K2_ROWS, ids=lambda r: f"layer{r[0]}")
def test_c3k2_yolov11n_shapes_vs_oracle(row, dispatch):
    """Every yolov11n C3k2 shape, f32 and bf16, under the test-session options, the library defaults and the throughput dispatch: a C3k2
    routed into a C2f whole-block kernel computes another function (Bottleneck e = 1.0) and fails here by O(1)."""
    from tests.hip_utils import bf16_weight_oracle, bf16_round, rel_err, to_cpu_nchw, to_dev_nhwc
    _, c1, c2, c3k, e, s = row
    o, p = _pair("C3k2", (c1, c2, 1, c3k, e))
    x = P.uniform(f"unit:c3k2:{row[0]}", (2, c1, s, s), -1.0, 1.0)
    with torch.no_grad(), _dispatch(dispatch):
        ref = _fold(o)(x)
        y = to_cpu_nchw(p(to_dev_nhwc(x)))
        refb = bf16_weight_oracle(o)(bf16_round(x))
        yb = to_cpu_nchw(p(to_dev_nhwc(x, torch.bfloat16)))
    e32, e16 = rel_err(y, ref), rel_err(yb, refb)
    print(f"C3k2 layer {row[0]} [{dispatch}]: f32 rel {e32:.2e}, bf16 rel {e16:.2e}")
    assert e32 <= 1e-4
    assert e16 <= 2e-2  # bf16 activations between the five-to-seven convs; a mis-routed block is off by O(1)


@pytest.mark.parametrize("dispatch", ["session", "serial", "throughput"])
def test_c2psa_vs_oracle(dispatch):
    from tests.hip_utils import bf16_weight_oracle, bf16_round, rel_err, to_cpu_nchw, to_dev_nhwc
    o, p = _pair("C2PSA", (256, 256, 1))
    x = P.uniform("unit:c2psa:gpu", (2, 256, 20, 20), -1.0, 1.0)
    with torch.no_grad(), _dispatch(dispatch):
        ref = _fold(o)(x)
        y = to_cpu_nchw(p(to_dev_nhwc(x)))
        refb = bf16_weight_oracle(o)(bf16_round(x))
        yb = to_cpu_nchw(p(to_dev_nhwc(x, torch.bfloat16)))
    e32, e16 = rel_err(y, ref), rel_err(yb, refb)
    print(f"C2PSA [{dispatch}]: f32 rel {e32:.2e}, bf16 rel {e16:.2e}")
    assert e32 <= 1e-4
    assert e16 <= 6e-2  # bf16 q / k (rounded by the qkv conv) shift every attention logit; the oracle keeps them f32


@pytest.mark.parametrize("dispatch", ["session", "serial", "throughput"])
def test_nonlegacy_detect_level_vs_oracle(dispatch):
    """One 80 x 80 level of yolov11n's head (ch 64: c2 = 64, c3 = 80) through every Detect walk; the DWConv class branch ends in
    upa_detect_tail (bf16) or the conv + decode (f32)."""
    from tests.hip_utils import DEV, bn_fix, to_dev_nhwc
    from ultralytics_pro_amd.nn.modules import head as H
    ch = (64, 128, 256)
    o = bn_fix(Y.Detect(80, ch))
    legacy = H.Detect.legacy
    H.Detect.legacy = False
    try:
        p = bn_fix(H.Detect(80, ch))
    finally:
        H.Detect.legacy = legacy
    for m in (o, p):
        m.stride = torch.tensor([8.0, 16.0, 32.0])
        m.bias_init()
        P.apply_procedural_weights(m, family="yolov11n")
    p = p.to(DEV).eval()
    p.keep_raw = False
    xs = [P.uniform(f"unit:det11gpu:{i}", (2, c, s, s), -1.0, 1.0) for i, (c, s) in enumerate(zip(ch, (80, 40, 20)))]
    of = _fold(o)
    with torch.no_grad(), _dispatch(dispatch):
        ref = of([t.clone() for t in xs])[0]
        y = p([t.to(DEV) for t in xs])[0].cpu()
        yb = p([to_dev_nhwc(t, torch.bfloat16) for t in xs])[0].float().cpu()
        refb = of([t.to(torch.bfloat16).float() for t in xs])[0]
    d, db = (y - ref).abs(), (yb - refb).abs()
    print(f"Detect(legacy=False) [{dispatch}]: f32 box {d[:, :4].max():.2e} score {d[:, 4:].max():.2e}; bf16 box {db[:, :4].max():.3f} "
          f"score {db[:, 4:].max():.4f}")
    assert d[:, :4].max() <= TOL and d[:, 4:].max() <= TOL
    assert db[:, :4].max() <= 4.0 and db[:, 4:].max() <= 0.05  # smoke()'s bf16 bound


# ---- end to end -------------------------------------------------------------------------------------------------------------------------


def _build(dtype, family=None):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    m = DetectionModel("yolov11n.yaml")
    P.apply_procedural_weights(m, family=family)
    m = m.to(DEV).eval()
    m.set_compute_dtype(dtype)
    return m


def test_e2e_f32_matches_reference_golden(golden_dir):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.utils.nms import non_max_suppression
    g = np.load(golden_dir / "e2e_yolov11n.npz")
    m = _build(torch.float32)
    with torch.no_grad():
        y = m(P.synthetic_images(2).to(DEV))[0]
    torch.cuda.synchronize()
    d = np.abs(y.cpu()[:, :, g["anchor_sel"]].numpy() - g["y_sel"])
    print(f"yolov11n f32: max|box d|={d[:, :4].max():.3e} max|score d|={d[:, 4:].max():.3e}")
    assert d[:, :4].max() <= TOL and d[:, 4:].max() <= TOL
    out = non_max_suppression(y, conf_thres=0.25, iou_thres=0.7, max_det=300)
    assert [o.shape[0] for o in out] == list(g["predict_n"])
    rows = torch.cat(out, 0).cpu().numpy()
    assert np.abs(rows[:, :4] - g["predict_rows"][:, :4]).max() <= TOL
    assert np.abs(rows[:, 4] - g["predict_rows"][:, 4]).max() <= TOL
    assert np.array_equal(rows[:, 5], g["predict_rows"][:, 5])


@pytest.mark.parametrize("dispatch", ["session", "serial", "throughput"])
def test_e2e_bf16_smooth_family_matches_reference_golden(dispatch, golden_dir):
    """bf16 on the smooth family vs the reference's f32 detections, with the bounds of the v8 smooth-family test (tests/test_hip_e2e.py):
    bf16-exact weights, so only activation rounding remains; rows whose score sits within +-0.005 of the 0.25 threshold may flip, every
    other row must be found (IoU >= 0.9, both ways, >= 0.995), and matched rows and sampled head outputs stay within the reference's AMP
    tolerance (0.5 px, 0.005).  The yolov11n smooth recipe was chosen so that a CPU model rounding every conv output to bf16 stays at
    half of these (0.25 px, 0.0027)."""
    from tests.hip_utils import DEV, detection_agreement, split_rows
    from ultralytics_pro_amd.utils.nms import non_max_suppression
    g = np.load(golden_dir / "e2e_yolov11n_smooth.npz")
    m = _build(torch.bfloat16, family="smooth:yolov11n")
    x = P.synthetic_images(2).to(DEV).to(torch.bfloat16).contiguous()
    with torch.no_grad(), _dispatch(dispatch):
        y = m(x)[0]
    torch.cuda.synchronize()
    d = np.abs(y.cpu()[:, :, g["anchor_sel"]].numpy() - g["y_sel"])
    out = [o.cpu().numpy() for o in non_max_suppression(y, conf_thres=0.25, iou_thres=0.7, max_det=300)]
    ref = split_rows(g["predict_rows"], g["predict_n"])
    a = detection_agreement(out, ref, 0.9)
    ref_x = [r[np.abs(r[:, 4] - 0.25) > SMOOTH_BAND] for r in ref]
    out_x = [r[np.abs(r[:, 4] - 0.25) > SMOOTH_BAND] for r in out]
    rec_x = detection_agreement(out, ref_x, 0.9)["recall"]
    prec_x = detection_agreement(out_x, ref, 0.9)["precision"]
    print(f"yolov11n smooth bf16 [{dispatch}]: head box max|d| {d[:, :4].max():.3f} px score max|d| {d[:, 4:].max():.4f}; detections "
          f"{a['n_mine']} vs {a['n_ref']}: recall {a['recall']:.3f} precision {a['precision']:.3f}; outside the band {rec_x:.4f} / {prec_x:.4f}; "
          f"matched box max {a['box_max']:.3f} px score max {a['score_max']:.4f}")
    assert rec_x >= 0.995 and prec_x >= 0.995
    assert a["box_max"] <= 0.5 and a["score_max"] <= SMOOTH_BAND
    assert d[:, :4].max() <= 0.5 and d[:, 4:].max() <= SMOOTH_BAND


@pytest.mark.parametrize("shape", [(1, 384, 640), (1, 1280, 1280)], ids=["b1_384x640", "b1_1280"])
def test_e2e_other_sizes_vs_oracle(shape):
    """Rect letterbox (240 attention tokens) and 1280 x 1280 (1600 tokens: more keys than LDS holds) in f32 vs the checker."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.utils.nms import non_max_suppression
    b, h, w = shape
    x = P.synthetic_images(b, h=h, w=w)
    o = Y.DetectionModel("yolov11n.yaml")
    P.apply_procedural_weights(o)
    o.fuse()
    with torch.no_grad():
        y_ref = o.double()(x.double())[0].float()  # float64: the checker's own f32 rounding is not charged to the kernels
        y = _build(torch.float32)(x.to(DEV))[0]
    torch.cuda.synchronize()
    d = (y.cpu() - y_ref).abs()
    print(f"yolov11n f32 {shape}: box {d[:, :4].max():.2e} score {d[:, 4:].max():.2e}")
    assert d[:, :4].max().item() <= TOL and d[:, 4:].max().item() <= TOL
    out = non_max_suppression(y, 0.25, 0.7)
    ref = onms.non_max_suppression(y_ref, 0.25, 0.7)
    assert [a.shape[0] for a in out] == [r.shape[0] for r in ref]


def test_e2e_graph_replay_equals_eager():
    from tests.hip_utils import DEV
    for dt in (torch.float32, torch.bfloat16):
        m = _build(dt, family="smooth:yolov11n")
        x = P.synthetic_images(2).to(DEV).to(dt).contiguous()
        with torch.no_grad():
            y_eager = m(x)[0].clone()
            run = m.compile(x)
            y1 = run()[0].clone()
            y2 = run()[0].clone()
        torch.cuda.synchronize()
        assert torch.equal(y1, y2) and torch.equal(y1, y_eager), dt


def test_e2e_pipelined_runner_copies_equal_single_graph():
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.engine.pipeline import PipelinedRunner
    from ultralytics_pro_amd.utils.nms import nms_raw
    m = _build(torch.bfloat16, family="smooth:yolov11n")
    x = P.synthetic_images(4).to(DEV).to(torch.bfloat16).contiguous()
    with torch.no_grad():
        with R.use_opts(**THROUGHPUT):
            run1 = m.compile(x, post=lambda o: nms_raw(o[0], 0.25, 0.7, key="ref11"))
        out1, cnt1, _ = run1()
        torch.cuda.synchronize()
        out1, cnt1 = out1.clone(), cnt1.clone()
        runner = PipelinedRunner(m, x, post=lambda o: nms_raw(o[0], 0.25, 0.7, key="pipe11"), micro_batches=2, in_flight=3)
        for _ in range(4):
            runner.step()
        torch.cuda.synchronize()
    assert int(cnt1.sum()) > 0
    for parts in runner.results():
        out = torch.cat([p_[0] for p_ in parts], 0)
        cnt = torch.cat([p_[1] for p_ in parts], 0)
        assert torch.equal(cnt, cnt1) and torch.equal(out, out1)


def test_e2e_throughput_dispatch_matches_default_dispatch():
    from tests.hip_utils import DEV, detection_agreement
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.utils.nms import non_max_suppression
    m = _build(torch.bfloat16, family="smooth:yolov11n")
    m.model[-1].keep_raw = False
    x = P.synthetic_images(4).to(DEV).to(torch.bfloat16).contiguous()
    with torch.no_grad():
        with R.use_opts(c2f64_max_px=0):
            y_def = m(x)[0].float().clone()
        with R.use_opts(**THROUGHPUT):
            y_thr = m(x)[0].float().clone()
        d_def = [o.cpu().numpy() for o in non_max_suppression(y_def, 0.25, 0.7, max_det=300)]
        d_thr = [o.cpu().numpy() for o in non_max_suppression(y_thr, 0.25, 0.7, max_det=300)]
    d = (y_def - y_thr).abs()
    x_def = [r[np.abs(r[:, 4] - 0.25) > SMOOTH_BAND] for r in d_def]
    x_thr = [r[np.abs(r[:, 4] - 0.25) > SMOOTH_BAND] for r in d_thr]
    rec_x = detection_agreement(d_thr, x_def, 0.9)["recall"]
    prec_x = detection_agreement(x_thr, d_def, 0.9)["precision"]
    print(f"yolov11n throughput vs default dispatch: box max {d[:, :4].max():.3f} px score max {d[:, 4:].max():.4f}; {rec_x:.4f} / {prec_x:.4f}")
    assert d[:, :4].max().item() <= 0.5 and d[:, 4:].max().item() <= SMOOTH_BAND
    assert rec_x >= 0.995 and prec_x >= 0.995


def test_trainer_refuses_yolo11():
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine.trainer import DetectionTrainer
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    with pytest.raises(L.UpaError, match="no training path"):
        DetectionTrainer(DetectionModel("yolov11n.yaml"))
