"""-m gpu: every HIP operator, called through the C ABI via the reference-shaped Python modules, against the oracle
on the same procedural weights / inputs.  f32 = parity mode (tight tolerances); bf16 = perf mode (bf16 rounding)."""

import json

import numpy as np
import pytest
import torch

from oracle import modules as om
from oracle import nms as onms
from ultralytics_pro_amd.utils import procedural as P

pytestmark = pytest.mark.gpu

CONV_CASES = [
    # c1, c2, k, s, p, H, W, N
    (16, 32, 1, 1, None, 12, 12, 2),
    (16, 32, 3, 1, None, 12, 12, 2),
    (16, 32, 3, 2, None, 13, 13, 2),
    (32, 64, 3, 2, None, 40, 40, 2),
    (64, 64, 3, 1, None, 40, 40, 3),
    (64, 80, 3, 1, None, 20, 20, 2),
    (80, 80, 3, 1, None, 23, 17, 2),
    (48, 32, 1, 1, None, 24, 24, 2),
    (192, 128, 1, 1, None, 20, 20, 2),
    (384, 256, 1, 1, None, 10, 10, 2),
    (128, 128, 3, 1, None, 20, 20, 2),
    (256, 64, 3, 1, None, 20, 20, 1),
    (128, 256, 3, 2, None, 40, 40, 1),
    (16, 16, 3, 1, None, 64, 64, 1),
    (16, 32, 3, 1, None, 64, 48, 2),   # 16 -> 32 on whole 8 x 16 tiles: the two-n-tile form of conv3x3_c16_kernel (bf16, pipe_all)
    (32, 16, 1, 1, None, 33, 9, 1),
    (512, 1024, 3, 1, None, 10, 10, 1),
    (1024, 256, 1, 1, None, 10, 10, 1),
    (64, 32, 2, 1, 1, 9, 9, 2),     # even kernel, pad 1: the phase correlations of the stride-2 data gradient
    (128, 64, 2, 1, 1, 21, 21, 1),
]


def _mods():
    from ultralytics_pro_amd.nn import modules as pm
    from ultralytics_pro_amd.nn.modules import resample
    return pm, resample


def _pair(ocls, pcls, args, name, family="default"):
    from tests.hip_utils import DEV, bn_fix
    o = bn_fix(ocls(*args))
    p = bn_fix(pcls(*args))
    P.apply_procedural_weights(o, family=family)
    P.apply_procedural_weights(p, family=family)
    return o, p.to(DEV)


@pytest.mark.parametrize("case", CONV_CASES, ids=[f"c{c[0]}-{c[1]}k{c[2]}s{c[3]}_{c[5]}x{c[6]}" for c in CONV_CASES])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_conv(case, dtype):
    from tests.hip_utils import assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc, unit_input
    pm, _ = _mods()
    c1, c2, k, s, p, H, W, N = case
    o, m = _pair(om.Conv, pm.Conv, (c1, c2, k, s, p), "conv")
    x = unit_input(f"conv{case}", (N, c1, H, W))
    if dtype == torch.bfloat16:
        x = bf16_round(x)
        o = bf16_weight_oracle(o)
    with torch.no_grad():
        ref = o(x)
        y = to_cpu_nchw(m(to_dev_nhwc(x, dtype)))
    assert y.shape == ref.shape
    if dtype == torch.float32:
        assert (y - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    else:  # bf16-rounded inputs AND weights on the oracle side: what is left is summation order + the output rounding
        assert_bf16_close(y, ref, f"conv{case}")


PIPE_CASES = [
    # c1, c2, H, W, N  (3x3 s1 p1, H % 8 == 0, W % 16 == 0: the software-pipelined kernel, csrc/conv_pipe.hip)
    (64, 64, 16, 32, 2),     # KTT 2, NTW 4; interior + every edge
    (32, 32, 8, 16, 3),      # single tile per image (all four edges at once)
    (16, 16, 24, 16, 1),     # Cin 16: half a k-tile zero filled
    (80, 80, 16, 16, 2),     # KTT 3 (80 of 96 channels), 80 couts = launches of 64 + 16
    (128, 64, 8, 32, 1),     # KTT 4
    (16, 32, 40, 48, 5),     # many tiles per persistent wave (5*5*3 = 75 tiles ... several rounds with UPA_PIPE_WGS small)
    (64, 80, 8, 16, 2),
    (48, 48, 16, 16, 1),     # 48 couts = 32 + 16
    (24, 16, 8, 16, 1),      # Cin 24: partial k-tile
    (16, 16, 8, 16, 3),      # 16 -> 16: the two-taps-per-MFMA variant (conv3x3_c16_kernel), one tile per image
    (16, 16, 40, 48, 2),     # ... many tiles per persistent wave, interior tiles
]


@pytest.mark.parametrize("case", PIPE_CASES, ids=[f"c{c[0]}-{c[1]}_{c[2]}x{c[3]}n{c[4]}" for c in PIPE_CASES])
def test_conv_pipe_kernel(case):
    """bf16 3x3 s1 convs through the persistent pipelined kernel vs the oracle Conv (conv.py:188-197) on bf16-rounded
    inputs; includes image borders (zero padding by the DMA zero page), partial k-tiles and split output-channel launches."""
    from tests.hip_utils import assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd import _lib as L
    pm, _ = _mods()
    c1, c2, H, W, N = case
    from ultralytics_pro_amd.engine import runtime as R
    var = L.lib().upa_conv_variant(N, H, W, c1, c2, 3, 1, 1, 1, R.opts_ptr())
    assert (var >> 21) & 1, "case is not dispatched to the pipelined kernel"
    o, m = _pair(om.Conv, pm.Conv, (c1, c2, 3, 1), "conv_pipe")
    x = bf16_round(P.uniform(f"pipe{case}", (N, c1, H, W), -1, 1))
    with torch.no_grad():
        ref = bf16_weight_oracle(o)(x)
        y = to_cpu_nchw(m(to_dev_nhwc(x, torch.bfloat16)))
    assert_bf16_close(y, ref, f"conv_pipe{case}")


BIG_CASES = [
    # c1, c2, k, H, W, N, residual[, stride]  (the large-tile LDS-shared-operand kernel, csrc/conv_big.hip)
    (64, 80, 3, 24, 40, 2, False),     # 96-channel variant (Cout 80: 5 of 6 n-tiles, odd tail store), 128-pixel workgroups
    (80, 80, 3, 80, 80, 2, True),      # 96-channel variant with 256-pixel workgroups; Cin 80: 3 k-tiles, 2 chunks
    (32, 64, 3, 33, 47, 1, False),     # 64-channel variant (8 x 1 waves)
    (64, 128, 3, 40, 40, 2, False, 2),   # stride 2: 40 -> 20, halo (TH-1)*2+3
    (128, 256, 3, 31, 45, 1, False, 2),  # stride 2, odd input sizes, two output columns
    (32, 64, 3, 64, 64, 1, False, 2),    # stride 2, 64-channel variant
    (128, 128, 3, 20, 20, 2, False),   # 20-wide map: 20 x 12 tiles, second tile ragged (8 rows)
    (256, 128, 3, 40, 40, 1, False),   # 40 x 6 tiles, 7 per image, last one ragged; 4 chunks of 64 channels
    (128, 256, 3, 16, 32, 2, True),    # 16 x 16 tiles, two 128-channel workgroup columns, residual add
    (512, 1024, 3, 10, 10, 1, False),  # 10 x 10 map in one tile (100 of 256 pixels), K = 4608, 8 workgroup columns
    (96, 128, 3, 9, 13, 3, False),     # Cin 96: odd k-tile count (last chunk half zero), odd sizes
    (72, 64, 3, 8, 8, 1, False),       # Cin 72: partial k-tile; Cout 64: half a workgroup column masked
    (1024, 256, 1, 10, 10, 2, False),  # pointwise: 200 pixels flattened, 16 chunks
    (256, 128, 1, 33, 9, 1, True),     # pointwise, ragged pixel count, residual
    (128, 384, 1, 20, 20, 1, False),   # three workgroup columns
    (128, 64, 2, 80, 80, 2, False),    # 2 x 2 kernel, pad 1 (output 81 x 81): the phase kernels of a stride-2 data gradient (train.hip)
    (256, 128, 2, 40, 40, 1, False),   # 2 x 2, 128-channel column, 41 x 41 output
    (512, 256, 2, 21, 19, 2, False),   # 2 x 2, odd sizes, two columns
]


@pytest.mark.parametrize("case", BIG_CASES, ids=[f"c{c[0]}-{c[1]}k{c[2]}s{c[7] if len(c) > 7 else 1}_{c[3]}x{c[4]}n{c[5]}{'r' if c[6] else ''}" for c in BIG_CASES])
@pytest.mark.parametrize("bm", [0, 512], ids=["auto", "bm512"])
@pytest.mark.parametrize("act", [True, False], ids=["silu", "noact"])
def test_conv_big_kernel(case, act, bm):
    """bf16 convs forced through conv_big_kernel (upa_opts.conv_big = 2) vs the oracle Conv (conv.py:188-197) on
    bf16-rounded inputs: image borders (zero page), tiles that are not powers of two, ragged last tiles, partial k-tiles and
    odd chunk counts, masked output-channel columns, pointwise layers, the fused residual add (block.py:668)."""
    from tests.hip_utils import assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd import _lib as L
    pm, _ = _mods()
    c1, c2, k, H, W, N, res = case[:7]
    st = case[7] if len(case) > 7 else 1
    if bm == 512 and not (k == 3 and st == 1 and c2 in (64, 80)):
        pytest.skip("512-pixel workgroups exist for the 64- and 80-channel 3x3 stride-1 forms only")
    from ultralytics_pro_amd.engine import runtime as R
    with R.use_opts(conv_big=2, conv_big_bm=bm):
        var = L.lib().upa_conv_variant(N, H, W, c1, c2, k, st, k // 2, 1, R.opts_ptr())
        assert (var >> 23) & 1, "case is not dispatched to the large-tile kernel"
        o, m = _pair(om.Conv, pm.Conv, (c1, c2, k, st, None, 1, 1, act), "conv_big")
        x = bf16_round(P.uniform(f"big{case}", (N, c1, H, W), -1, 1))
        oh, ow = (H + 2 * (k // 2) - k) // st + 1, (W + 2 * (k // 2) - k) // st + 1
        rsd = bf16_round(P.uniform(f"bigres{case}", (N, c2, oh, ow), -1, 1)) if res else None
        with torch.no_grad():
            ref = bf16_weight_oracle(o)(x) + (rsd if res else 0)
            y = to_cpu_nchw(m(to_dev_nhwc(x, torch.bfloat16), residual=to_dev_nhwc(rsd, torch.bfloat16) if res else None))
    assert_bf16_close(y, ref, f"conv_big{case}")


WS3_CASES = [
    # c1, c2, H, W, N, act, residual  (persistent 3x3 with register-resident weights, csrc/conv_ws3.hip; 16 x 8 pixel tiles)
    (64, 64, 80, 80, 2, True, False),     # 50 tiles per image
    (64, 64, 40, 48, 3, True, True),      # Bottleneck shortcut
    (64, 64, 33, 47, 1, False, False),    # ragged right / bottom tiles, no activation
    (32, 64, 20, 20, 2, True, False),     # Cin 32: one k-tile, the second zero
    (48, 64, 9, 5, 1, True, True),        # a map smaller than a tile, partial channel group, shortcut
    (64, 64, 160, 160, 2, True, False),   # 400 tiles: every workgroup walks several (double-buffered halo, buffer reuse)
    (64, 64, 96, 96, 16, True, True),     # 1152 tiles on 512 workgroups with the shortcut
]


@pytest.mark.parametrize("case", WS3_CASES, ids=[f"c{c[0]}-{c[1]}_{c[2]}x{c[3]}n{c[4]}{'' if c[5] else '_lin'}{'_res' if c[6] else ''}" for c in WS3_CASES])
def test_conv_ws3_kernel(case):
    """bf16 3x3 convs forced through the persistent register-resident-weights kernel (upa_opts.conv_ws3 = 2) vs the oracle Conv
    (conv.py:188-197, + the Bottleneck add block.py:668) on BN-folded bf16 weights: image borders, ragged tiles, partial k-tiles,
    more tiles than workgroups (the halo double buffer is reused), the shortcut read."""
    from tests.hip_utils import assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    pm, _ = _mods()
    c1, c2, H, W, N, act, res = case
    with R.use_opts(conv_ws3=2):
        var = L.lib().upa_conv_variant(N, H, W, c1, c2, 3, 1, 1, 1, R.opts_ptr())
        assert (var >> 24) & 1, "case is not dispatched to the register-resident-weights kernel"
        o, m = _pair(om.Conv, pm.Conv, (c1, c2, 3, 1, None, 1, 1, act), "conv_ws3")
        x = bf16_round(P.uniform(f"ws3{case}", (N, c1, H, W), -1, 1))
        rsd = bf16_round(P.uniform(f"ws3res{case}", (N, c2, H, W), -1, 1)) if res else None
        with torch.no_grad():
            ref = bf16_weight_oracle(o)(x) + (rsd if res else 0)
            y = to_cpu_nchw(m(to_dev_nhwc(x, torch.bfloat16), residual=to_dev_nhwc(rsd, torch.bfloat16) if res else None))
    assert_bf16_close(y, ref, f"conv_ws3{case}")


PAIR_HALF_CASES = [
    # H, W, N, shortcut  (Bottleneck(64, 64, shortcut, k=(3,3), e=0.5): 64 -> 32 -> 64, the darknet block of yolov3-rtdetr rows 2 / 4)
    (40, 40, 2, True),
    (33, 47, 3, False),    # odd sizes, ragged tiles
    (9, 5, 1, True),       # smaller than one tile
    (14, 14, 1, True),     # exactly one tile
    (96, 96, 2, True),     # many tiles per image
]


@pytest.mark.parametrize("case", PAIR_HALF_CASES, ids=[f"{c[0]}x{c[1]}n{c[2]}{'r' if c[3] else ''}" for c in PAIR_HALF_CASES])
def test_bottleneck_pair_half_width_kernel(case):
    """`upa_bottleneck_pair_e` with cmid = c / 2 (bf16): x + cv2(cv1(x)) of an e = 0.5 Bottleneck (block.py:644-668) as one kernel with
    the 32-channel intermediate tile in LDS, vs the oracle Bottleneck on bf16-rounded inputs with the intermediate rounded to bf16 as
    the kernel stores it, and vs the product's own two-launch path."""
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    pm, _ = _mods()
    H, W, N, sc = case
    c = 64
    o, m = _pair(om.Bottleneck, pm.Bottleneck, (c, c, sc, 1, (3, 3), 0.5), "pairh")
    assert m.cv1.conv.out_channels == 32
    x = bf16_round(P.uniform(f"pairh{case}", (N, c, H, W), -1, 1))
    with torch.no_grad():
        ob = bf16_weight_oracle(o)
        t = bf16_round(ob.cv1(x))
        ref = ob.cv2(t) + (x if sc else 0)
    buf = R.alloc_nhwc(N, 3 * c, H, W, torch.bfloat16, DEV)
    buf.zero_()
    xin = buf[:, c:2 * c]
    xin.copy_(to_dev_nhwc(x, torch.bfloat16))
    with torch.no_grad():
        # the kernel itself (the module would fall back silently if the dispatch refused)
        p1 = m.cv1._packed(m.cv1.conv, m.cv1.bn, DEV, torch.bfloat16, False)
        p2 = m.cv2._packed(m.cv2.conv, m.cv2.bn, DEV, torch.bfloat16, False)
        vx, vy = R.view_of(xin), R.view_of(buf[:, 2 * c:])
        rc = L.lib().upa_bottleneck_pair_e(vx.ptr, vx.n, vx.h, vx.w, vx.c, 32, vx.ld, p1.w.data_ptr(), p1.bias.data_ptr(),
                                           p2.w.data_ptr(), p2.bias.data_ptr(), vy.ptr, vy.ld, int(sc), L.ACT_SILU, vx.dtype,
                                           R.opts_ptr(), L.current_stream(DEV))
        assert rc != L.UPA_EUNSUPPORTED, "64 -> 32 -> 64 must be inside the fused form"
        L.check(rc, "bottleneck_pair_e")
        y = to_cpu_nchw(buf[:, 2 * c:])
        m.fuse_pair = True
        y1 = to_cpu_nchw(m(xin))          # the module's own dispatch: the same kernel
        m.fuse_pair = False
        y2 = to_cpu_nchw(m(xin))          # two launches
    scale = max(1.0, ref.abs().max().item())
    assert_bf16_close(y, ref, f"pairh{case}", abs_=2.0 ** -7)
    assert torch.equal(y1, y)
    assert (y - y2).abs().max().item() <= 2e-2 * scale  # one bf16 ulp of the output
    assert float(to_cpu_nchw(buf[:, :c]).abs().max()) == 0.0  # nothing written outside the output slice


PAIR_CASES = [
    # c, H, W, N, shortcut  (Bottleneck(c, c, shortcut, k=(3,3), e=1.0) as one kernel, csrc/conv_pair.hip)
    (64, 40, 40, 2, True),     # 14 x 14 tiles, 3 x 3 per image, ragged right / bottom tiles, residual
    (64, 40, 40, 1, False),
    (32, 80, 80, 2, True),     # C = 32: 64-byte pixels (one k-tile)
    (32, 33, 47, 3, False),    # odd sizes, several images
    (64, 20, 20, 2, True),     # a map barely larger than one tile
    (32, 9, 5, 1, True),       # a map smaller than one tile: every mid pixel ring is image border (zero padding of conv 2)
    (64, 14, 14, 1, True),     # exactly one tile
]


@pytest.mark.parametrize("case", PAIR_CASES, ids=[f"c{c[0]}_{c[1]}x{c[2]}n{c[3]}{'r' if c[4] else ''}" for c in PAIR_CASES])
def test_bottleneck_pair_kernel(case):
    """`upa_bottleneck_pair` (bf16): x + cv2(cv1(x)) of a C2f inner Bottleneck (block.py:644-668, k = (3,3), e = 1.0) as one
    kernel with the intermediate tile in LDS, vs the oracle Bottleneck on bf16-rounded inputs with the intermediate rounded
    to bf16 as the kernel stores it; then vs the product's own two-launch path (same weights), which it must match to bf16
    resolution.  Zero padding of the SECOND conv at the image border (mid pixels outside the image must be zero, not
    act(bias)), ragged tiles, strided input / output views (channel slices of a wider buffer as inside C2f)."""
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd.engine import runtime as R
    pm, _ = _mods()
    c, H, W, N, sc = case
    o, m = _pair(om.Bottleneck, pm.Bottleneck, (c, c, sc, 1, (3, 3), 1.0), "pair")
    x = bf16_round(P.uniform(f"pair{case}", (N, c, H, W), -1, 1))
    with torch.no_grad():
        ob = bf16_weight_oracle(o)
        t = bf16_round(ob.cv1(x))
        ref = ob.cv2(t) + (x if sc else 0)
    # x and y are channel slices [c, 2c) and [2c, 3c) of one 3c-channel buffer, as C2f lays them out
    buf = R.alloc_nhwc(N, 3 * c, H, W, torch.bfloat16, DEV)
    buf.zero_()
    xin = buf[:, c:2 * c]
    xin.copy_(to_dev_nhwc(x, torch.bfloat16))
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R2
    with torch.no_grad():
        m.fuse_pair = True
        if c == 64:  # not dispatched in production (upa_opts.pair = 0): call the kernel directly so the 64-channel form stays covered
            p1 = m.cv1._packed(m.cv1.conv, m.cv1.bn, DEV, torch.bfloat16, False)
            p2 = m.cv2._packed(m.cv2.conv, m.cv2.bn, DEV, torch.bfloat16, False)
            vx, vy = R2.view_of(xin), R2.view_of(buf[:, 2 * c:])
            rc = L.lib().upa_bottleneck_pair(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, p1.w.data_ptr(), p1.bias.data_ptr(),
                                             p2.w.data_ptr(), p2.bias.data_ptr(), vy.ptr, vy.ld, int(sc), L.ACT_SILU, vx.dtype,
                                             R2.opts_ptr(), L.current_stream(DEV))
            assert rc != L.UPA_EUNSUPPORTED, "the 64-channel pair must be dispatched under the test options (pair = 2)"
            L.check(rc, "bottleneck_pair")
            y = to_cpu_nchw(buf[:, 2 * c:])
        else:
            y = to_cpu_nchw(m(xin, out=buf[:, 2 * c:]))
        m.fuse_pair = False
        y2 = to_cpu_nchw(m(xin))
    assert y.shape == ref.shape
    scale = max(1.0, ref.abs().max().item())
    # rounding points shared with the oracle (bf16 x, weights, mid tile); a mid value whose f32 sum lands within summation-order
    # noise of a bf16 tie may round the other way and moves its 9 x C consumers by one mid ulp x weight: allowed for in `abs_`
    assert_bf16_close(y, ref, f"pair{case}", abs_=2.0 ** -7)
    assert (y - y2).abs().max().item() <= 2e-2 * scale  # one bf16 ulp of the output
    assert float(to_cpu_nchw(buf[:, :c]).abs().max()) == 0.0  # nothing written outside the output slice


@pytest.mark.parametrize("case", [(2, 128, 64, 128, 20, 20), (1, 256, 128, 128, 10, 12), (3, 32, 16, 48, 7, 9), (2, 48, 16, 32, 6, 6)],
                         ids=["up128_skip64", "up256_skip128_cout128", "up32_ragged", "up48_fallback"])
def test_conv1x1_virtual_upsample_concat(case):
    """`upa_conv1x1_upcat`: the 1x1 conv after Concat([Upsample(2x nearest)(u), skip]) reading u at (y/2, x/2) instead of a
    materialised upsample (yolov8.yaml rows 10-12 / 13-15; nn.Upsample + conv.py Concat + C2f.cv1 block.py:479).  Same kernel,
    same values: bit-identical to the conv over the materialised concat buffer, and equal to the oracle's
    Conv(cat(upsample(u), skip)) to bf16 resolution.  The 48-channel case is outside the fused form (k-tiles of 32 channels):
    the call must fall back to writing the upsample."""
    from tests.hip_utils import DEV, bf16_round, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn.modules.conv import VirtualUpsample
    pm, rs = _mods()
    n, cu, cs, cout, h, w = case
    o, m = _pair(om.Conv, pm.Conv, (cu + cs, cout, 1, 1), "upcat")
    u = bf16_round(P.uniform(f"upcat_u{case}", (n, cu, h, w), -1, 1))
    sk = bf16_round(P.uniform(f"upcat_s{case}", (n, cs, 2 * h, 2 * w), -1, 1))
    from tests.hip_utils import assert_bf16_close, bf16_weight_oracle
    with torch.no_grad():
        ref = bf16_weight_oracle(o)(torch.cat([torch.nn.functional.interpolate(u, scale_factor=2, mode="nearest"), sk], 1))
        ud = to_dev_nhwc(u, torch.bfloat16)
        buf = R.alloc_nhwc(n, cu + cs, 2 * h, 2 * w, torch.bfloat16, DEV)
        buf.fill_(7.0)  # the leading channels must not be read on the fused path
        buf[:, cu:].copy_(to_dev_nhwc(sk, torch.bfloat16))
        up = rs.Upsample(None, 2, "nearest")
        done = []
        y = to_cpu_nchw(m(buf, up=VirtualUpsample(ud, cu, lambda: done.append(up(ud, out=buf[:, :cu])))))
        assert bool(done) == (cu % 32 != 0)  # fused unless the upsampled part is not whole k-tiles
        up(ud, out=buf[:, :cu])
        y2 = to_cpu_nchw(m(buf))
    assert torch.equal(y, y2)
    assert_bf16_close(y, ref, f"upcat{case}")


@pytest.mark.parametrize("case", [(192, True, (2, 37, 50)), (192, False, (2, 80, 80)), (64, False, (1, 14, 14)), (96, True, (3, 5, 9))],
                         ids=["c192s_37x50", "c192_80x80", "c64_14x14", "c96s_5x9"])
def test_c2f_pair_cv2_kernel(case):
    """`upa_bottleneck_pair_cv2` (bf16): C2f(c1, 64, n=1) with its 32-channel Bottleneck and cv2 as ONE launch after cv1
    (block.py:457-488, 644-668; yolov8n model.15 = C2f(192, 64, 1, shortcut=False)) vs the oracle C2f with the intermediates
    rounded to bf16 where the kernels round them, and vs the product's own path with the fusion switched off (cv1, pair kernel,
    cv2 as three launches).  Ragged tiles, maps smaller than a tile, with and without the shortcut, a strided output view."""
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd.engine import runtime as R
    pm, _ = _mods()
    c1, sc, (N, H, W) = case
    o, m = _pair(om.C2f, pm.C2f, (c1, 64, 1, sc), f"c2f_paircv2{c1}")
    o = bf16_weight_oracle(o)
    x = bf16_round(P.uniform(f"c2fpc{case}", (N, c1, H, W), -1.5, 1.5))
    with torch.no_grad():
        ys = list(bf16_round(o.cv1(x)).chunk(2, 1))
        t = bf16_round(o.m[0].cv1(ys[-1]))
        ys.append(bf16_round((ys[-1] if sc else 0) + o.m[0].cv2(t)))
        ref = o.cv2(torch.cat(ys, 1))
        buf = R.alloc_nhwc(N, 128, H, W, torch.bfloat16, DEV)
        buf.zero_()
        xd = to_dev_nhwc(x, torch.bfloat16)
        m.fuse_pair_cv2 = True
        y = to_cpu_nchw(m(xd, out=buf[:, 64:]))
        m.fuse_pair_cv2 = False
        y2 = to_cpu_nchw(m(xd))
        m.fuse_pair_cv2 = True
        cat = R.alloc_nhwc(N, 96, H, W, torch.bfloat16, DEV)
        m.cv1(xd, out=cat[:, :64])
        assert m._pair_cv2(cat, None) is not None, "the fused form was not dispatched"
    scale = max(1.0, ref.abs().max().item())
    assert_bf16_close(y, ref, f"c2f_pair_cv2{case}", abs_=2.0 ** -7)  # (flipped ties of three bf16 intermediates: see the pair test)
    d = (y - y2).abs()
    assert d.max().item() <= 3e-2 * scale and (d > 1e-6).float().mean().item() <= 0.03, (d.max().item(), (d > 1e-6).float().mean().item())
    assert float(to_cpu_nchw(buf[:, :64]).abs().max()) == 0.0  # nothing written outside the output slice


def test_c3_virtual_upsample_concat():
    """C3 after Concat([Upsample(u), skip]) (yolov5 neck rows 12-14 / 16-18): both 1x1 convs that read the Concat (cv1, cv2;
    block.py:509-532) take the half-resolution tensor through `upa_conv1x1_upcat` - bit-identical to the materialised path."""
    from tests.hip_utils import DEV, bf16_round, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn.modules.conv import VirtualUpsample
    pm, rs = _mods()
    n, cu, cs, h, w = 2, 128, 64, 10, 12
    o, m = _pair(om.C3, pm.C3, (cu + cs, 64, 1, False), "c3_upcat")
    u = bf16_round(P.uniform("c3up_u", (n, cu, h, w), -1, 1))
    sk = bf16_round(P.uniform("c3up_s", (n, cs, 2 * h, 2 * w), -1, 1))
    with torch.no_grad():
        ud = to_dev_nhwc(u, torch.bfloat16)
        buf = R.alloc_nhwc(n, cu + cs, 2 * h, 2 * w, torch.bfloat16, DEV)
        buf.fill_(7.0)
        buf[:, cu:].copy_(to_dev_nhwc(sk, torch.bfloat16))
        up = rs.Upsample(None, 2, "nearest")
        done = []
        v = VirtualUpsample(ud, cu, lambda: done.append(up(ud, out=buf[:, :cu])))
        y = to_cpu_nchw(m(buf, up=v))
        assert not done and not v.done  # neither conv needed the materialised copy
        up(ud, out=buf[:, :cu])
        y2 = to_cpu_nchw(m(buf))
        ref = o(torch.cat([torch.nn.functional.interpolate(u, scale_factor=2, mode="nearest"), sk], 1))
    assert torch.equal(y, y2)
    assert (y - ref).abs().max().item() <= 6e-2 * max(1.0, ref.abs().max().item())


C2F_CASES = [
    # c1, n, shortcut, (N, H, W)
    (32, 1, True, (2, 37, 50)), (32, 1, True, (1, 16, 16)), (32, 1, True, (3, 5, 9)), (32, 1, True, (2, 160, 160)),
    (32, 1, True, (1, 33, 16)),
    (64, 2, True, (2, 37, 50)), (64, 2, True, (1, 16, 16)), (64, 2, True, (3, 5, 9)), (64, 2, True, (2, 80, 80)),
    (64, 1, True, (2, 33, 47)), (64, 1, False, (1, 20, 35)), (64, 2, False, (2, 18, 16)),
]


@pytest.mark.parametrize("th", [0, 16, 10], ids=["auto", "th16", "th10"])
@pytest.mark.parametrize("case", C2F_CASES, ids=[f"c{c[0]}n{c[1]}{'s' if c[2] else ''}_{c[3][0]}x{c[3][1]}x{c[3][2]}" for c in C2F_CASES])
def test_c2f_fused_kernel(case, th):
    """`upa_c2f_fused` (bf16): a whole C2f block (block.py:457-488 with the Bottlenecks of :644-668 inside) as one kernel -
    C2f(32, 32, n=1) = model.2 of yolov8n, C2f(64, 64, n=2) = its model.4, C2f(64, 64, n=1) = model.2 of yolov8s - vs the
    oracle C2f with every intermediate (cv1 output, each Bottleneck's mid tensor and output) rounded to bf16 where the
    kernel rounds them, and vs the product's own multi-launch path on the same weights.  Ragged tiles, maps smaller than
    one 16 x 16 tile (every ring of the halo is image border: the 3x3 convs' zero padding must be zero, not SiLU(bias)),
    several images, with and without the shortcut, a strided output view."""
    from tests.hip_utils import DEV, bf16_round, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd.engine import runtime as R
    pm, _ = _mods()
    c1, nb, sc, (N, H, W) = case
    if th and not (c1 == 64 and nb == 2):
        pytest.skip("the output-tile height is a choice of the C2f(64, 64, n=2) form only")
    o, m = _pair(om.C2f, pm.C2f, (c1, c1, nb, sc), f"c2f_fused{c1}{nb}")
    from tests.hip_utils import assert_bf16_close, bf16_weight_oracle
    o = bf16_weight_oracle(o)
    x = bf16_round(P.uniform(f"c2f{case}", (N, c1, H, W), -1.5, 1.5))
    with torch.no_grad():
        y01 = bf16_round(o.cv1(x))
        ys = list(y01.chunk(2, 1))
        for bt in o.m:
            t = bf16_round(bt.cv1(ys[-1]))
            ys.append(bf16_round((ys[-1] if sc else 0) + bt.cv2(t)))
        ref = o.cv2(torch.cat(ys, 1))
        buf = R.alloc_nhwc(N, 2 * c1, H, W, torch.bfloat16, DEV)
        buf.zero_()
        xd = to_dev_nhwc(x, torch.bfloat16)
        m.fuse_block = True
        with R.use_opts(c2f32_th=th):  # 16 x 16 (0 / 16) or 10 x 16 output tiles
            assert m._fused(xd, None) is not None, "the fused form was not dispatched"
            y = to_cpu_nchw(m(xd, out=buf[:, c1:]))
        m.fuse_block = False
        y2 = to_cpu_nchw(m(xd))
    scale = max(1.0, ref.abs().max().item())
    assert_bf16_close(y, ref, f"c2f_fused{case}", abs_=2.0 ** -7)  # (flipped ties of up to six bf16 intermediates: see the pair test)
    # same rounding points as the separate launches; a bf16 tie that falls the other way in an intermediate moves few outputs
    # (measured: 0.02-0.03 % of the outputs differ with the shortcut, up to 1.4 % without it - nothing damps a flipped tie -; mean
    # |error| against the plain-f32 oracle equal to 5 digits, tools/experiments/c2f_err.py)
    d = (y - y2).abs()
    assert d.max().item() <= 3e-2 * scale and (d > 1e-6).float().mean().item() <= 0.03, (d.max().item(), (d > 1e-6).float().mean().item())
    assert float(to_cpu_nchw(buf[:, :c1]).abs().max()) == 0.0  # nothing written outside the output slice


C2F16_DOWN_CASES = [
    # (N, H, W), rows per workgroup (0 / -1 = auto, >= 4: that many input rows)
    ((2, 160, 160), 0), ((2, 160, 160), 160), ((1, 37, 50), 0), ((2, 37, 51), 8), ((1, 16, 16), 0), ((3, 5, 9), 0),
    ((1, 41, 23), 4), ((1, 64, 100), 22), ((1, 33, 20), -1), ((1, 2, 2), 0), ((1, 20, 21), 6), ((1, 160, 19), 0),
]


@pytest.mark.parametrize("case", C2F16_DOWN_CASES, ids=[f"{c[0][0]}x{c[0][1]}x{c[0][2]}_r{c[1]}" for c in C2F16_DOWN_CASES])
def test_c2f16_down_fused_kernel(case):
    """`upa_c2f16_down_fused` (csrc/c2f16_stream.hip): C2f(32, 32, n = 1, shortcut) AND the Conv(32, 64, 3, 2) row behind it (yolov8.yaml rows
    2-3; block.py:457-488 / 644-668, conv.py:188-197) as one line-buffer launch.  Against the oracle with bf16 rounding points (the block's
    output too: it is a bf16 tensor between the two rows) and against the two separate launches, which it must equal up to flipped rounding
    ties; odd heights and widths (the stride-2 conv's bottom / right padding), ragged strips, parts that end mid-image, maps smaller than a
    strip, a strided output view with nothing written outside it."""
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd.engine import runtime as R
    pm, _ = _mods()
    (N, H, W), rows = case
    o, m = _pair(om.C2f, pm.C2f, (32, 32, 1, True), "c2f16_down_block")
    od, md = _pair(om.Conv, pm.Conv, (32, 64, 3, 2), "c2f16_down_conv")
    o, od = bf16_weight_oracle(o), bf16_weight_oracle(od)
    x = bf16_round(P.uniform(f"c2f16d{case}", (N, 32, H, W), -1.5, 1.5))
    OH, OW = (H + 1) // 2, (W + 1) // 2
    with torch.no_grad():
        y01 = bf16_round(o.cv1(x))
        ys = list(y01.chunk(2, 1))
        t = bf16_round(o.m[0].cv1(ys[-1]))
        ys.append(bf16_round(ys[-1] + o.m[0].cv2(t)))
        ref = od(bf16_round(o.cv2(torch.cat(ys, 1))))
        assert tuple(ref.shape) == (N, 64, OH, OW)
        buf = R.alloc_nhwc(N, 128, OH, OW, torch.bfloat16, DEV)
        buf.zero_()
        xbuf = R.alloc_nhwc(N, 64, H, W, torch.bfloat16, DEV)   # x as a channel slice of a wider buffer (pixel pitch 64, as behind a Concat)
        xbuf.fill_(7.0)
        xbuf[:, 32:].copy_(to_dev_nhwc(x, torch.bfloat16))
        xd = xbuf[:, 32:]
        with R.use_opts(c2f_stream_rows=rows):
            yv = m.forward_down(xd, md, out=buf[:, 64:])
            assert yv is not None, "the fused form was not dispatched"
            y = to_cpu_nchw(yv)
        with R.use_opts(no_c2f16_down=1):
            assert m.forward_down(xd, md) is None
        y2 = to_cpu_nchw(md(m(xd)))
    scale = max(1.0, ref.abs().max().item())
    assert_bf16_close(y, ref, f"c2f16_down{case}", abs_=2.0 ** -7)
    d = (y - y2).abs()
    assert d.max().item() <= 3e-2 * scale and (d > 1e-6).float().mean().item() <= 0.03, (d.max().item(), (d > 1e-6).float().mean().item())
    assert float(to_cpu_nchw(buf[:, :64]).abs().max()) == 0.0  # nothing written outside the output slice


C2F_STREAM1_CASES = [
    # c1, shortcut, (N, H, W), up_c, rows per workgroup (0 = auto, -1 = whole height)
    (192, False, (2, 80, 80), 128, 0), (192, False, (2, 80, 80), 128, -1), (192, True, (1, 38, 50), 128, 8), (192, False, (2, 18, 24), 0, 0),
    (64, True, (2, 33, 47), 0, 0), (64, False, (1, 20, 35), 0, 6), (64, True, (2, 160, 160), 0, 0), (128, True, (1, 40, 44), 64, 0),
    (128, False, (3, 5, 9), 0, 0), (192, True, (1, 16, 16), 128, 0),
]


@pytest.mark.parametrize("case", C2F_STREAM1_CASES, ids=[f"c{c[0]}{'s' if c[1] else 'n'}_{c[2][0]}x{c[2][1]}x{c[2][2]}_u{c[3]}_r{c[4]}" for c in C2F_STREAM1_CASES])
def test_c2f_stream1_kernel(case):
    """The line-buffer kernel of the n = 1 block (csrc/c2f_stream.hip: C2f(64 k, 64, n = 1), block.py:457-488 / 644-668; k = 1, 2, 3),
    reached through `upa_c2f_fused` (c1 = 64) and `upa_c2f32_up_fused` (c1 = 128 | 192, with and without the virtual nn.Upsample + Concat
    in front): against the oracle with bf16 rounding points and against the 16 x 16 tile form (`c2f_stream=1`), which it must equal up
    to flipped rounding ties; ragged strips and parts, tiny maps, both shortcut settings, nothing written outside the output slice."""
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn.modules.conv import VirtualUpsample
    import ultralytics_pro_amd.nn.modules as rs
    pm, _ = _mods()
    c1, sc, (N, H, W), upc, rows = case
    o, m = _pair(om.C2f, pm.C2f, (c1, 64, 1, sc), f"c2f_stream1_{c1}")
    o = bf16_weight_oracle(o)
    if upc:
        u = bf16_round(P.uniform(f"c2fs1u{case}", (N, upc, H // 2, W // 2), -1.5, 1.5))
        sk = bf16_round(P.uniform(f"c2fs1s{case}", (N, c1 - upc, H, W), -1.5, 1.5))
        x = torch.cat([torch.nn.functional.interpolate(u, scale_factor=2, mode="nearest"), sk], 1)
    else:
        x = bf16_round(P.uniform(f"c2fs1{case}", (N, c1, H, W), -1.5, 1.5))
    with torch.no_grad():
        y01 = bf16_round(o.cv1(x))
        ys = list(y01.chunk(2, 1))
        t = bf16_round(o.m[0].cv1(ys[-1]))
        ys.append(bf16_round((ys[-1] if sc else 0) + o.m[0].cv2(t)))
        ref = o.cv2(torch.cat(ys, 1))
        out = R.alloc_nhwc(N, 128, H, W, torch.bfloat16, DEV)
        out.zero_()
        m.fuse_block = True

        def run(**opts):
            if upc:
                ud = to_dev_nhwc(u, torch.bfloat16)
                buf = R.alloc_nhwc(N, c1, H, W, torch.bfloat16, DEV)
                buf.fill_(7.0)  # the virtual channels must never be read from the concat buffer
                buf[:, upc:].copy_(to_dev_nhwc(sk, torch.bfloat16))
                v = VirtualUpsample(ud, upc, lambda: rs.Upsample(None, 2, "nearest")(ud, out=buf[:, :upc]))
                with R.use_opts(**opts):
                    yy = to_cpu_nchw(m(buf, out=out[:, 64:], up=v))
                assert not v.done, "the fused form must read the half-resolution tensor itself"
                return yy
            with R.use_opts(**opts):
                return to_cpu_nchw(m(to_dev_nhwc(x, torch.bfloat16), out=out[:, 64:]))
        y = run(c2f_stream_rows=rows)
        y_tile = run(c2f_stream=1)
    scale = max(1.0, ref.abs().max().item())
    assert_bf16_close(y, ref, f"c2f_stream1{case}", abs_=2.0 ** -7)
    d = (y - y_tile).abs()
    assert d.max().item() <= 3e-2 * scale and (d > 1e-6).float().mean().item() <= 0.03, (d.max().item(), (d > 1e-6).float().mean().item())
    assert float(to_cpu_nchw(out[:, :64]).abs().max()) == 0.0  # nothing written outside the output slice


C2F_STREAM_CASES = [
    # shortcut, (N, H, W), rows per workgroup (0 = auto)
    (True, (2, 80, 80), 0), (True, (2, 80, 80), 40), (True, (1, 37, 50), 0), (True, (2, 37, 50), 8), (True, (1, 16, 16), 0), (True, (3, 5, 9), 0),
    (True, (1, 41, 23), 4), (False, (2, 18, 16), 6), (True, (1, 64, 100), 22), (True, (2, 80, 80), -1), (True, (1, 33, 20), -1),
]


@pytest.mark.parametrize("case", C2F_STREAM_CASES, ids=[f"{'s' if c[0] else 'n'}_{c[1][0]}x{c[1][1]}x{c[1][2]}_r{c[2]}" for c in C2F_STREAM_CASES])
def test_c2f_stream_kernel(case):
    """`upa_c2f_fused` on its line-buffer kernel (csrc/c2f_stream.hip: C2f(64, 64, n = 2), block.py:457-488 / 644-668): strips of 20 columns
    streamed two rows per step through LDS ring buffers, fixed wave roles.  Against the oracle with bf16 rounding points, against the
    16 x 16 tile form (`c2f_stream=1`) and against the separate launches; whole and ragged strips, parts that end mid-image, maps smaller
    than one strip, every ring of the halo on the image border, with and without the shortcut, nothing written outside the output slice."""
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd.engine import runtime as R
    pm, _ = _mods()
    sc, (N, H, W), rows = case
    o, m = _pair(om.C2f, pm.C2f, (64, 64, 2, sc), "c2f_stream")
    o = bf16_weight_oracle(o)
    x = bf16_round(P.uniform(f"c2fs{case}", (N, 64, H, W), -1.5, 1.5))
    with torch.no_grad():
        y01 = bf16_round(o.cv1(x))
        ys = list(y01.chunk(2, 1))
        for bt in o.m:
            t = bf16_round(bt.cv1(ys[-1]))
            ys.append(bf16_round((ys[-1] if sc else 0) + bt.cv2(t)))
        ref = o.cv2(torch.cat(ys, 1))
        buf = R.alloc_nhwc(N, 128, H, W, torch.bfloat16, DEV)
        buf.zero_()
        xd = to_dev_nhwc(x, torch.bfloat16)
        m.fuse_block = True
        with R.use_opts(c2f_stream_rows=rows):
            y = to_cpu_nchw(m(xd, out=buf[:, 64:]))
        with R.use_opts(c2f_stream=1):
            y_tile = to_cpu_nchw(m(xd))
        with R.use_opts(c2f_stream=2, c2f_stream_rows=rows):  # the first wave-role set (cv2 recomputes y0)
            y_roles1 = to_cpu_nchw(m(xd))
        m.fuse_block = False
        y2 = to_cpu_nchw(m(xd))
    scale = max(1.0, ref.abs().max().item())
    assert_bf16_close(y, ref, f"c2f_stream{case}", abs_=2.0 ** -7)
    for other, name in ((y_tile, "tile form"), (y2, "separate launches"), (y_roles1, "first role set")):
        d = (y - other).abs()
        assert d.max().item() <= 3e-2 * scale and (d > 1e-6).float().mean().item() <= 0.03, (name, d.max().item(), (d > 1e-6).float().mean().item())
    assert float(to_cpu_nchw(buf[:, :64]).abs().max()) == 0.0  # nothing written outside the output slice


C2F32UP_CASES = [
    # c1, shortcut, (N, H, W), up_c  (C2f(c1, 64, n = 1) with 32-channel halves, cv1 streamed over 64-channel chunks: upa_c2f32_up_fused)
    (192, False, (2, 80, 80), 128),   # yolov8n model.15: virtual Upsample(128) + Concat(64) in front, three chunks
    (192, False, (1, 26, 38), 128),   # ragged 16 x 16 tiles
    (128, True, (2, 16, 16), 64),     # two chunks, shortcut, exactly one tile
    (256, False, (1, 10, 6), 0),      # four chunks from x alone, a map smaller than a tile
    (192, True, (3, 20, 20), 0),      # three chunks, no half-resolution source
]


@pytest.mark.parametrize("case", C2F32UP_CASES, ids=[f"c{c[0]}{'s' if c[1] else ''}_{c[2][0]}x{c[2][1]}x{c[2][2]}{'_up' + str(c[3]) if c[3] else ''}" for c in C2F32UP_CASES])
def test_c2f32_up_fused_kernel(case):
    """`upa_c2f32_up_fused` (bf16): C2f(64 k, 64, n = 1) (block.py:457-488) as one kernel with cv1's input streamed in 64-channel chunks,
    the leading channels optionally read from the half-resolution tensor of a virtual nn.Upsample + Concat (yolov8.yaml rows 13-15) - vs
    the oracle C2f on BN-folded bf16 weights with the intermediates rounded where the kernel rounds them, and vs the product's own
    multi-launch path.  The upsampled slice of the concat buffer holds a sentinel that must never be read."""
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn.modules.conv import VirtualUpsample
    pm, rs = _mods()
    c1, sc, (N, H, W), upc = case
    o, m = _pair(om.C2f, pm.C2f, (c1, 64, 1, sc), f"c2f32up_{c1}")
    o = bf16_weight_oracle(o)
    if upc:
        u = bf16_round(P.uniform(f"c2f32upu{case}", (N, upc, H // 2, W // 2), -1.5, 1.5))
        sk = bf16_round(P.uniform(f"c2f32ups{case}", (N, c1 - upc, H, W), -1.5, 1.5))
        x = torch.cat([torch.nn.functional.interpolate(u, scale_factor=2, mode="nearest"), sk], 1)
    else:
        x = bf16_round(P.uniform(f"c2f32up{case}", (N, c1, H, W), -1.5, 1.5))
    with torch.no_grad():
        ys = list(bf16_round(o.cv1(x)).chunk(2, 1))
        t = bf16_round(o.m[0].cv1(ys[-1]))
        ys.append(bf16_round((ys[-1] if sc else 0) + o.m[0].cv2(t)))
        ref = o.cv2(torch.cat(ys, 1))
        buf = R.alloc_nhwc(N, 128, H, W, torch.bfloat16, DEV)
        buf.zero_()
        xd = to_dev_nhwc(x, torch.bfloat16)
        up = None
        if upc:
            ud = to_dev_nhwc(u, torch.bfloat16)
            xd[:, :upc].fill_(77.0)  # never read on the fused path
            mat = []
            upm = rs.Upsample(None, 2, "nearest")
            up = VirtualUpsample(ud, upc, lambda: mat.append(upm(ud, out=xd[:, :upc])))
        m.fuse_block = True
        assert m._form32up()
        y = to_cpu_nchw(m(xd, out=buf[:, 64:], up=up))
        if upc:
            assert not mat and not up.done, "the fused block must read the half-resolution tensor itself"
            up.materialize()
        m.fuse_block = False
        y2 = to_cpu_nchw(m(xd))
    scale = max(1.0, ref.abs().max().item())
    assert_bf16_close(y, ref, f"c2f32up{case}", abs_=2.0 ** -7)
    d = (y - y2).abs()
    assert d.max().item() <= 3e-2 * scale and (d > 1e-6).float().mean().item() <= (0.05 if sc else 0.10), \
        (d.max().item(), (d > 1e-6).float().mean().item())
    assert float(to_cpu_nchw(buf[:, :64]).abs().max()) == 0.0  # nothing written outside the output slice


C2F64_CASES = [
    # c1, n, shortcut, (N, H, W), up_c  (C2f(c1, 128, n) with 64-channel halves as one kernel, csrc/c2f64.hip)
    (128, 2, True, (2, 40, 40), 0),     # yolov8n model.6: 10 x 10 tiles, no ragged edge
    (128, 2, False, (1, 23, 17), 0),    # ragged tiles, no shortcut
    (128, 2, True, (1, 10, 10), 0),     # exactly one tile: every ring is image border
    (128, 2, True, (3, 9, 5), 0),       # a map smaller than a tile
    (384, 1, False, (2, 40, 40), 256),  # yolov8n model.12: virtual Upsample + Concat in front, six 64-channel chunks, 10 x 20 tiles
    (192, 1, False, (2, 20, 36), 0),    # yolov8n model.18: three chunks, ragged 20-wide tiles
    (192, 1, True, (1, 14, 22), 128),   # up_c = 128 of 192, shortcut, odd tile counts
    (64, 1, True, (2, 12, 12), 0),      # a single chunk
]


@pytest.mark.parametrize("case", C2F64_CASES, ids=[f"c{c[0]}n{c[1]}{'s' if c[2] else ''}_{c[3][0]}x{c[3][1]}x{c[3][2]}{'_up' + str(c[4]) if c[4] else ''}" for c in C2F64_CASES])
def test_c2f64_fused_kernel(case):
    """`upa_c2f64_fused` (bf16): a whole C2f block with 64-channel halves (block.py:457-488, Bottlenecks :644-668) as one kernel -
    yolov8n model.6 / model.12 / model.18 - vs the oracle C2f on BN-folded bf16 weights with every intermediate (cv1 output, each
    Bottleneck's mid tensor and output) rounded to bf16 where the kernel rounds it, and vs the product's own multi-launch path.
    The input may be Concat([Upsample(2x)(u), skip]) with the upsample read on the fly (yolov8.yaml rows 10-12): the leading channels
    of the concat buffer are then filled with a sentinel that must never be read.  Ragged tiles, maps smaller than a tile (every
    ring is image border: the 3x3 convs' zero padding must be zero, not SiLU(bias)), 1 / 2 / 3 / 6 input chunks, strided output."""
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn.modules.conv import VirtualUpsample
    pm, rs = _mods()
    c1, nb, sc, (N, H, W), upc = case
    o, m = _pair(om.C2f, pm.C2f, (c1, 128, nb, sc), f"c2f64_{c1}{nb}")
    o = bf16_weight_oracle(o)
    if upc:
        u = bf16_round(P.uniform(f"c2f64u{case}", (N, upc, H // 2, W // 2), -1.5, 1.5))
        sk = bf16_round(P.uniform(f"c2f64s{case}", (N, c1 - upc, H, W), -1.5, 1.5))
        x = torch.cat([torch.nn.functional.interpolate(u, scale_factor=2, mode="nearest"), sk], 1)
    else:
        x = bf16_round(P.uniform(f"c2f64{case}", (N, c1, H, W), -1.5, 1.5))
    with torch.no_grad():
        ys = list(bf16_round(o.cv1(x)).chunk(2, 1))
        for bt in o.m:
            t = bf16_round(bt.cv1(ys[-1]))
            ys.append(bf16_round((ys[-1] if sc else 0) + bt.cv2(t)))
        ref = o.cv2(torch.cat(ys, 1))
        buf = R.alloc_nhwc(N, 256, H, W, torch.bfloat16, DEV)
        buf.zero_()
        xd = to_dev_nhwc(x, torch.bfloat16)
        up = None
        if upc:
            ud = to_dev_nhwc(u, torch.bfloat16)
            xd[:, :upc].fill_(77.0)  # never read on the fused path
            mat = []
            upm = rs.Upsample(None, 2, "nearest")
            up = VirtualUpsample(ud, upc, lambda: mat.append(upm(ud, out=xd[:, :upc])))
        m.fuse_block = True
        assert m._form64()
        y = to_cpu_nchw(m(xd, out=buf[:, 128:], up=up))
        if upc:
            assert not mat and not up.done, "the fused block must read the half-resolution tensor itself"
            up.materialize()
        m.fuse_block = False
        y2 = to_cpu_nchw(m(xd))
    scale = max(1.0, ref.abs().max().item())
    assert_bf16_close(y, ref, f"c2f64{case}", abs_=2.0 ** -7)  # (flipped ties of up to six bf16 intermediates: see the pair test)
    # vs the product's own launches: same rounding points, other f32 summation orders - a flipped bf16 tie of an intermediate moves
    # its consumers by an ulp; without the shortcut nothing damps it (measured: 3.6 % of the outputs one ulp apart with the shortcut, 5.5 % without, n = 2)
    d = (y - y2).abs()
    assert d.max().item() <= 3e-2 * scale and (d > 1e-6).float().mean().item() <= (0.05 if sc else 0.10), \
        (d.max().item(), (d > 1e-6).float().mean().item())
    assert float(to_cpu_nchw(buf[:, :128]).abs().max()) == 0.0  # nothing written outside the output slice


C1_CASES = [
    # c1, c2, H, W, N, act, env  (1x1 s1: the streaming pointwise kernel, csrc/conv1x1.hip)
    (64, 64, 16, 16, 2, True, {}),                                   # KTT 2, NTW 4
    (48, 32, 9, 7, 3, True, {}),                                     # 189 pixels: ragged last tile; Cin 48: half a k-tile
    (80, 80, 20, 20, 2, False, {}),                                  # NTW 5 (odd tail store), KTT 3 partial, no activation
    (384, 256, 10, 10, 2, True, {}),                                 # 16 n-tiles: two workgroup rows of 8; KTT 12
    (192, 128, 12, 20, 1, True, {"c1_mt": 2, "c1_waves": 8}),
    (32, 32, 40, 48, 2, True, {"c1_mt": 4, "c1_wgs": 3}),   # many rounds per persistent wave, ring wraps
    (32, 16, 33, 9, 1, True, {"c1_mt": 4, "c1_wgs": 2}),    # KTT 1: an epilogue every step (store counting)
    (128, 192, 8, 8, 1, False, {"c1_mt": 2, "c1_wgs": 1}),  # 12 n-tiles: second row half masked
    (256, 128, 5, 5, 1, True, {"c1_waves": 4}),                # KTT 8 = the whole ring of an MT 1 wave
    (96, 64, 30, 30, 1, True, {"c1_mt": 1, "c1_waves": 4, "c1_wgs": 2}),
]


@pytest.mark.parametrize("case", C1_CASES, ids=[f"c{c[0]}-{c[1]}_{c[2]}x{c[3]}n{c[4]}{'' if c[5] else '_lin'}{'_' + '_'.join(str(v) for v in c[6].values()) if c[6] else ''}" for c in C1_CASES])
def test_conv1x1_stream_kernel(case):
    """bf16 pointwise convs through the streaming kernel vs the oracle Conv (conv.py:188-197) on bf16-rounded inputs:
    ragged pixel counts, partial k-tiles, odd / split / masked output-channel tiles, every (MT, waves) shape of the
    kernel and few workgroups (many ring rounds per wave: the counted vmcnt waits)."""
    from tests.hip_utils import assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd import _lib as L
    pm, _ = _mods()
    from ultralytics_pro_amd.engine import runtime as R
    c1, c2, H, W, N, act, fields = case
    with R.use_opts(**fields) if fields else R.use_opts(R.current_opts()):
        var = L.lib().upa_conv_variant(N, H, W, c1, c2, 1, 1, 0, 1, R.opts_ptr())
        assert (var >> 22) & 1, "case is not dispatched to the streaming 1x1 kernel"
        o, m = _pair(om.Conv, pm.Conv, (c1, c2, 1, 1, None, 1, 1, act), "conv1x1")
        x = bf16_round(P.uniform(f"c1{case[:5]}", (N, c1, H, W), -1, 1))
        with torch.no_grad():
            ref = bf16_weight_oracle(o)(x)
            y = to_cpu_nchw(m(to_dev_nhwc(x, torch.bfloat16)))
    assert_bf16_close(y, ref, f"conv1x1{case[:5]}")


def test_conv_pipe_residual_and_concat_views():
    """Bottleneck (block.py:644-668) with shortcut inside a C2f: residual add fused in the pipelined kernel's epilogue,
    input / output / residual are channel slices of wider concat buffers (ld > C)."""
    from tests.hip_utils import bf16_round, to_cpu_nchw, to_dev_nhwc
    pm, _ = _mods()
    o, m = _pair(om.C2f, pm.C2f, (64, 64, 2, True), "c2f_pipe")
    x = bf16_round(P.uniform("c2f_pipe_x", (2, 64, 16, 32), -1, 1))
    with torch.no_grad():
        ref = o(x)
        y = to_cpu_nchw(m(to_dev_nhwc(x, torch.bfloat16)))
    err = (y - ref).abs().max().item()
    assert err <= 4e-2 * max(1.0, ref.abs().max().item()), err
    # 32-channel C2f: its Bottlenecks are 16 -> 16 convs with shortcut (conv3x3_c16_kernel, residual epilogue)
    o, m = _pair(om.C2f, pm.C2f, (32, 32, 2, True), "c2f_c16")
    x = bf16_round(P.uniform("c2f_c16_x", (2, 32, 24, 32), -1, 1))
    with torch.no_grad():
        ref = o(x)
        y = to_cpu_nchw(m(to_dev_nhwc(x, torch.bfloat16)))
    err = (y - ref).abs().max().item()
    assert err <= 4e-2 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("case", [(3, 16, 3, 2, None, 64, 64), (3, 16, 6, 2, 2, 64, 64), (3, 32, 3, 1, None, 40, 48)],
                         ids=["v8stem", "v5stem", "v3stem"])
def test_stem_reads_nchw(case, dtype):
    from tests.hip_utils import DEV, bf16_round, to_cpu_nchw, unit_input
    pm, _ = _mods()
    c1, c2, k, s, p, H, W = case
    o, m = _pair(om.Conv, pm.Conv, (c1, c2, k, s, p), "stem")
    x = unit_input(f"stem{case}", (2, c1, H, W), 0, 1)
    m.compute_dtype = dtype
    xin = x.to(DEV)
    if dtype == torch.bfloat16:
        xin = xin.to(torch.bfloat16)  # the reference's `im.half()` (predictor.py:151-173) - plumbing cast
        x = bf16_round(x)
    with torch.no_grad():
        ref = o(x)
        y = to_cpu_nchw(m(xin))
    tol = 2e-5 if dtype == torch.float32 else 2e-2
    assert (y - ref).abs().max().item() <= tol * max(1.0, ref.abs().max().item())


BLOCKS = [
    ("bottleneck", "Bottleneck", (16, 16, True, 1, (3, 3), 1.0), (2, 16, 10, 10)),
    ("bottleneck_noadd", "Bottleneck", (16, 32, False), (2, 16, 10, 10)),
    ("c2f_n2", "C2f", (32, 32, 2, True), (2, 32, 10, 10)),
    ("c2f_n1_noshortcut", "C2f", (48, 32, 1, False), (2, 48, 10, 10)),
    ("c3_n1", "C3", (32, 32, 1, True), (2, 32, 10, 10)),
    ("sppf", "SPPF", (32, 32, 5), (2, 32, 9, 11)),
    ("mhsa", "MHSA", (32, 6, 6, 4), (2, 32, 6, 6)),
    ("bot3", "BoT3", (32, 32, 1, 0.5, 1, 6, 6), (2, 32, 6, 6)),
]


@pytest.mark.parametrize("name,cls,args,xshape", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_blocks_match_golden_and_oracle(name, cls, args, xshape, golden_dir):
    """Same inputs as tests/golden/ops_unit.npz: HIP f32 vs the reference's recorded output."""
    from tests.hip_utils import to_cpu_nchw, to_dev_nhwc, unit_input
    pm, _ = _mods()
    G = np.load(golden_dir / "ops_unit.npz")
    o, m = _pair(getattr(om, cls), getattr(pm, cls), args, name)
    x = unit_input(name, xshape)
    with torch.no_grad():
        y = to_cpu_nchw(m(to_dev_nhwc(x)))
    assert np.abs(y.numpy() - G[name]).max() <= 2e-5
    with torch.no_grad():
        yb = to_cpu_nchw(m(to_dev_nhwc(x, torch.bfloat16)))
    assert np.abs(yb.numpy() - G[name]).max() <= 6e-2 * max(1.0, np.abs(G[name]).max())


SPPF_FRONT_CASES = [(256, 256, (2, 20, 20)), (256, 256, (3, 13, 11)), (128, 64, (1, 4, 4)), (512, 512, (2, 20, 20)), (256, 256, (1, 32, 32)), (256, 256, (32, 20, 20))]


@pytest.mark.parametrize("case", SPPF_FRONT_CASES, ids=[f"c{c[0]}_{c[2][0]}x{c[2][1]}x{c[2][2]}" for c in SPPF_FRONT_CASES])
def test_sppf_front_fused_kernel(case):
    """`upa_sppf_front` (csrc/elementwise.hip): SPPF's cv1 and its three chained 5 x 5 pools (block.py:382-406) as one launch, bf16.  Against the
    oracle SPPF with the bf16 rounding point after cv1 (where the separate launches round), against the two separate launches (equal up to flipped
    rounding ties of cv1; the pools themselves are exact: slice i + 1 must be EXACTLY the 5 x 5 max of slice i), odd map sizes, the largest map."""
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd.engine import runtime as R
    pm, _ = _mods()
    c1, c2, (N, H, W) = case
    o, m = _pair(om.SPPF, pm.SPPF, (c1, c2, 5), f"sppf_front{c1}")
    o = bf16_weight_oracle(o)
    x = bf16_round(P.uniform(f"sppff{case}", (N, c1, H, W), -1.5, 1.5))
    with torch.no_grad():
        y0 = bf16_round(o.cv1(x))
        y1 = o.m(y0); y2 = o.m(y1); y3 = o.m(y2)
        ref = o.cv2(torch.cat([y0, y1, y2, y3], 1))
        xd = to_dev_nhwc(x, torch.bfloat16)
        c_ = c1 // 2
        cat = R.alloc_nhwc(N, 4 * c_, H, W, torch.bfloat16, DEV)
        cat.fill_(7.0)
        assert m._front(xd, cat, c_), "the fused form was not dispatched"
        torch.cuda.synchronize()
        catc = to_cpu_nchw(cat)
        y = to_cpu_nchw(m(xd))
        with R.use_opts(no_sppf_front=1):
            assert not m._front(xd, cat, c_)
            y2l = to_cpu_nchw(m(xd))
    assert_bf16_close(catc[:, :c_], y0, f"sppf_front y0 {case}", abs_=2.0 ** -7)
    mp = torch.nn.MaxPool2d(5, 1, 2)
    for i in range(3):  # the pools are exact on whatever slice i holds
        assert torch.equal(catc[:, (i + 1) * c_:(i + 2) * c_], mp(catc[:, i * c_:(i + 1) * c_])), f"pool {i}"
    scale = max(1.0, ref.abs().max().item())
    assert_bf16_close(y, ref, f"sppf_front {case}", abs_=2.0 ** -6)
    d = (y - y2l).abs()
    assert d.max().item() <= 3e-2 * scale and (d > 1e-6).float().mean().item() <= 0.03, (d.max().item(), (d > 1e-6).float().mean().item())


@pytest.mark.parametrize("hw,batch", [((20, 20), 2), ((13, 11), 3), ((4, 4), 1), ((20, 20), 32)], ids=["20x20", "13x11", "4x4", "20x20_bs32"])
def test_mhsa_hot_path_shape_vs_oracle(hw, batch):
    """BoT3's real MHSA problem: 128 channels, 4 heads x 32 dims, 20x20 = 400 keys, plus the fused residual - f32 on the vector
    kernel, bf16 on the matrix-core kernel (csrc/attention.hip: mhsa_mfma_bf16_d32_kernel); key counts that are not multiples of
    the 32-key block or the 16-query tile (143, 16) and the config's batch."""
    from tests.hip_utils import bf16_round, to_cpu_nchw, to_dev_nhwc, unit_input
    pm, _ = _mods()
    o, m = _pair(om.BottleneckTransformer, pm.BottleneckTransformer, (128, 128, 1, 4, True, hw, 1), "bt")
    x = unit_input("bt_hot", (batch, 128, hw[0], hw[1]))
    with torch.no_grad():
        ref = o(x)
        y = to_cpu_nchw(m(to_dev_nhwc(x)))
        yb = to_cpu_nchw(m(to_dev_nhwc(x, torch.bfloat16)))
        refb = o(bf16_round(x))
    assert (y - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    print(f"mhsa bf16 {hw} bs {batch}: max|d| {(yb - refb).abs().max().item():.4f} of max|ref| {refb.abs().max().item():.3f}")
    assert (yb - ref).abs().max().item() <= 4e-2 * max(1.0, ref.abs().max().item())
    # bf16: against the f32 oracle on the bf16-rounded input the error is q / k / v / cv1 roundings + P in bf16: ~1 % of the range
    assert (yb - refb).abs().max().item() <= 2e-2 * max(1.0, refb.abs().max().item())


def test_upsample_concat_exact(golden_dir):
    from tests.hip_utils import to_cpu_nchw, to_dev_nhwc, unit_input
    pm, rs = _mods()
    G = np.load(golden_dir / "ops_unit.npz")
    a, b = unit_input("up_a", (2, 8, 5, 5)), unit_input("up_b", (2, 4, 10, 10))
    y = pm.Concat(1)([rs.Upsample(None, 2, "nearest")(to_dev_nhwc(a)), to_dev_nhwc(b)])
    assert np.array_equal(to_cpu_nchw(y).numpy(), G["upsample_concat"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_maxpool_variants_exact(dtype):
    from tests.hip_utils import bf16_round, to_cpu_nchw, to_dev_nhwc, unit_input
    _, rs = _mods()
    x = unit_input("pool", (2, 16, 13, 10))
    if dtype == torch.bfloat16:
        x = bf16_round(x)
    xd = to_dev_nhwc(x, dtype)
    y = to_cpu_nchw(rs.MaxPool2d(2, 2, 0)(xd))
    assert torch.equal(y, torch.nn.MaxPool2d(2, 2, 0)(x))
    y = to_cpu_nchw(rs.MaxPool2d(2, 1, 0)(rs.ZeroPad2d([0, 1, 0, 1])(xd)))
    assert torch.equal(y, torch.nn.MaxPool2d(2, 1, 0)(torch.nn.ZeroPad2d([0, 1, 0, 1])(x)))
    y = to_cpu_nchw(rs.MaxPool2d(5, 1, 2)(xd))
    assert torch.equal(y, torch.nn.MaxPool2d(5, 1, 2)(x))


def test_detect_head_matches_golden(golden_dir):
    from tests.hip_utils import DEV, bn_fix, to_cpu_nchw, to_dev_nhwc, unit_input
    pm, _ = _mods()
    G = np.load(golden_dir / "ops_unit.npz")
    pm.Detect.legacy = True
    d = bn_fix(pm.Detect(80, (16, 32, 64)))
    d.stride = torch.tensor([8.0, 16.0, 32.0])
    P.apply_procedural_weights(d, family="yolov8n")
    d = d.to(DEV)
    xs = [to_dev_nhwc(unit_input(f"det{i}", s)) for i, s in enumerate([(2, 16, 8, 8), (2, 32, 4, 4), (2, 64, 2, 2)])]
    with torch.no_grad():
        y, raw = d(xs)
    torch.cuda.synchronize()
    assert y.shape == (2, 84, 84)
    assert np.abs(to_cpu_nchw(raw[0]).numpy() - G["detect_raw0"]).max() <= 5e-5
    d_ = np.abs(y.cpu().numpy() - G["detect_y"])
    assert d_[:, :4].max() <= 1e-3 and d_[:, 4:].max() <= 1e-5


def test_detect_decode_vs_oracle_random_logits():
    """Decode kernel alone: DFL + dist2bbox + sigmoid on wide-range logits, f32 and bf16 inputs."""
    from tests.hip_utils import DEV, bf16_round, to_dev_nhwc, unit_input
    pm, _ = _mods()
    pm.Detect.legacy = True
    for dtype in (torch.float32, torch.bfloat16):
        det = pm.Detect(80, (64, 128)).eval()
        det.stride = torch.tensor([8.0, 16.0])
        raws = [unit_input(f"rawlvl{i}", (2, 144, s, s + 3), -8, 8) for i, s in enumerate((12, 6))]
        if dtype == torch.bfloat16:
            raws = [bf16_round(r) for r in raws]
        oref = om.Detect(80, (64, 128)).eval()
        oref.stride = det.stride
        ref = oref._inference([r.clone() for r in raws])
        y = det._inference([to_dev_nhwc(r, dtype) for r in raws])
        torch.cuda.synchronize()
        diff = (y.cpu() - ref).abs()
        assert diff[:, :4].max() <= 2e-4 and diff[:, 4:].max() <= 2e-6, (dtype, diff[:, :4].max(), diff[:, 4:].max())


@pytest.mark.parametrize("nc,shape", [(80, (2, 13, 21)), (80, (3, 40, 40)), (20, (1, 9, 16)), (3, (2, 7, 5))],
                         ids=["nc80_13x21", "nc80_40x40", "nc20", "nc3"])
def test_detect_tail_fused_decode_vs_oracle(nc, shape):
    """`upa_detect_tail` (bf16): the last 1x1 conv of a Detect branch with its half of the decode as epilogue - box (DFL +
    dist2bbox + stride, head.py:151-169 / block.py:250-253 / tal.py:367-376) and class (sigmoid) - vs the oracle's
    Detect._inference on f32 logits computed from the same bf16-rounded activations and weights; the optional raw rows
    equal the plain conv's output.  Ragged pixel counts (not multiples of 16), class counts that are not multiples of 16
    or 8, an anchor offset inside a larger output."""
    from tests.hip_utils import DEV, bf16_round, to_cpu_nchw, to_dev_nhwc, unit_input
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn.modules.conv import PackedConv
    n, h, w = shape
    c2, c3 = 64, max(16, (nc + 7) // 8 * 8)
    ncp = (nc + 7) // 8 * 8
    tb = bf16_round(unit_input(f"tail_b{nc}", (n, c2, h, w), -2, 2))
    tc = bf16_round(unit_input(f"tail_c{nc}", (n, c3, h, w), -2, 2))
    wb = bf16_round(unit_input(f"tail_wb{nc}", (64, c2, 1, 1), -0.6, 0.6))
    wc = bf16_round(unit_input(f"tail_wc{nc}", (nc, c3, 1, 1), -0.6, 0.6))
    bb, bc = unit_input(f"tail_bb{nc}", (64,), -1, 1), unit_input(f"tail_bc{nc}", (nc,), -3, 1)
    raw = torch.cat([torch.nn.functional.conv2d(tb, wb, bb), torch.nn.functional.conv2d(tc, wc, bc)], 1)
    oref = om.Detect(nc, (64,)).eval()
    oref.stride = torch.tensor([16.0])
    ref = oref._inference([raw.clone()])  # (n, 4 + nc, h*w)
    a0, extra = 37, 11
    a_total = a0 + h * w + extra
    y = torch.full((n, 4 + nc, a_total), -7.0, device=DEV)
    rawbuf = R.alloc_nhwc(n, 64 + ncp, h, w, torch.bfloat16, DEV)
    rawbuf.zero_()
    best_keys = torch.full((n, a_total), -1, dtype=torch.int64, device=DEV)  # NMS prefilter keys written by the class launch
    for keep_raw in (True, False):
        y.fill_(-7.0)
        best_keys.fill_(-1)
        for kind, t, wt, bias, cout, rv in ((1, tb, wb, bb, 64, rawbuf[:, :64]), (2, tc, wc, bc, ncp, rawbuf[:, 64:])):
            wpad = torch.cat([wt, torch.zeros(cout - wt.shape[0], *wt.shape[1:])], 0)
            bpad = torch.cat([bias, torch.zeros(cout - bias.shape[0])], 0)
            pk = PackedConv(wpad, bpad, 1, DEV, torch.bfloat16, False)
            vt = R.view_of(to_dev_nhwc(t, torch.bfloat16))
            vr = R.view_of(rv)
            L.check(L.lib().upa_detect_tail(vt.ptr, vt.n, vt.h, vt.w, vt.c, vt.ld, pk.w.data_ptr(), pk.bias.data_ptr(), cout, kind, nc,
                                            16.0, y.data_ptr(), a_total, a0, vr.ptr if keep_raw else None, vr.ld if keep_raw else 0,
                                            best_keys.data_ptr() if kind == 2 else None,
                                            L.UPA_BF16, R.opts_ptr(), L.current_stream(DEV)), "detect_tail")
        torch.cuda.synchronize()
        # every anchor of the level carries the NMS key of its best class, (~bits(best) << 32) | (anchor * nc + FIRST argmax)
        sc = y.cpu()[:, 4:, a0:a0 + h * w]
        best, arg = sc.max(1)
        bits = best.contiguous().numpy().view(np.uint32).astype(np.uint64)
        anchors = np.arange(a0, a0 + h * w, dtype=np.uint64)
        want = ((~bits & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | (anchors[None, :] * np.uint64(nc) + arg.numpy().astype(np.uint64))
        kc = best_keys.cpu()
        assert np.array_equal(kc[:, a0:a0 + h * w].numpy().view(np.uint64), want)
        assert bool((kc[:, :a0] == -1).all()) and bool((kc[:, a0 + h * w:] == -1).all())
        got = y[:, :, a0:a0 + h * w].cpu()
        d = (got - ref).abs()
        # f32 logits from f32 accumulation of bf16 products; v_exp_f32 / v_rcp_f32 (1 ulp) in the softmax / sigmoid
        assert d[:, :4].max().item() <= 2e-3 and d[:, 4:].max().item() <= 2e-6 + 1e-6, (keep_raw, d[:, :4].max().item(), d[:, 4:].max().item())
        assert float(y[:, :, :a0].min()) == -7.0 and float(y[:, :, a0 + h * w:].max()) == -7.0  # nothing outside the level
        if keep_raw:
            r = to_cpu_nchw(rawbuf)[:, :64 + nc]
            assert (r - raw).abs().max().item() <= 0.04 * raw.abs().max().item() / 4  # bf16-rounded logits


@pytest.mark.parametrize("nc,c3,shape", [(80, 80, (2, 13, 21)), (80, 80, (3, 40, 40)), (20, 64, (1, 9, 16)), (91, 96, (2, 7, 5)),
                                         (80, 80, (20, 80, 80))],
                         ids=["nc80_13x21", "nc80_40x40", "nc20_c64", "nc91_c96", "nc80_80x80_256px_tiles"])
def test_detect_branch_tail_vs_unfused_and_oracle(nc, c3, shape):
    """`upa_detect_branch_tail` (bf16): [conv3x3 + BN + SiLU -> 1x1 conv -> decode half] of a Detect branch in one launch
    (head.py:94-100, 116-126, 151-169).  Checked (a) against the two-launch HIP path (conv2d, then upa_detect_tail) that
    rounds the same intermediate to bf16 - only the k order of the 1x1 MFMA differs - and (b) against the oracle's
    conv -> SiLU -> conv -> Detect._inference in f32 on the same bf16-rounded inputs and weights."""
    from tests.hip_utils import DEV, bf16_round, to_dev_nhwc, unit_input
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn.modules.conv import PackedConv, hip_conv2d
    n, h, w = shape
    ncp = (nc + 7) // 8 * 8
    a0, extra = 19, 5
    a_total = a0 + h * w + extra
    y = torch.full((n, 4 + nc, a_total), -7.0, device=DEV)
    y2 = torch.full((n, 4 + nc, a_total), -7.0, device=DEV)
    best_keys = torch.full((n, a_total), -1, dtype=torch.int64, device=DEV)  # NMS prefilter: best-class sort keys (u64 bits)
    raws = []
    for kind, c, cout1 in ((1, 64, 64), (2, c3, nc)):
        cp = 64 if kind == 1 else (80 if c == 80 else 96)  # c = 80: the 5-tile form with a 16-wide last k-step
        x = bf16_round(unit_input(f"bt_x{kind}{nc}", (n, c, h, w), -1.5, 1.5))
        w3 = bf16_round(unit_input(f"bt_w3{kind}{nc}", (c, c, 3, 3), -0.12, 0.12))
        b3 = unit_input(f"bt_b3{kind}{nc}", (c,), -0.5, 0.5)
        w1 = bf16_round(unit_input(f"bt_w1{kind}{nc}", (cout1, c, 1, 1), -0.5, 0.5))
        b1 = unit_input(f"bt_b1{kind}{nc}", (cout1,), -2, 1)
        hmid = bf16_round(torch.nn.functional.silu(torch.nn.functional.conv2d(x, w3, b3, padding=1)))
        raws.append(torch.nn.functional.conv2d(hmid, w1, b1))
        xd = to_dev_nhwc(x, torch.bfloat16)
        vx = R.view_of(xd)
        # fused launch
        w3p = torch.cat([w3, torch.zeros(cp - c, c, 3, 3)], 0)
        b3p = torch.cat([b3, torch.zeros(cp - c)], 0)
        pk3 = PackedConv(w3p, b3p, 3, DEV, torch.bfloat16, False)
        wt = torch.zeros(cp, cp)
        wt[:cout1, :c] = w1.reshape(cout1, c)
        bt = torch.zeros(cp)
        bt[:cout1] = b1
        host = torch.empty(L.lib().upa_tail_packed_weight_bytes(cp, cp), dtype=torch.uint8)
        L.check(L.lib().upa_pack_tail_weight(wt.data_ptr(), cp, cp, host.data_ptr()), "pack_tail_weight")
        wtd, btd = host.to(DEV), bt.to(DEV)
        L.check(L.lib().upa_detect_branch_tail(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, pk3.w.data_ptr(), pk3.bias.data_ptr(),
                                               wtd.data_ptr(), btd.data_ptr(), kind, nc, 16.0, y.data_ptr(), a_total, a0,
                                               best_keys.data_ptr() if kind == 2 else None,
                                               L.UPA_BF16, R.opts_ptr(), L.current_stream(DEV)), "detect_branch_tail")
        # two launches
        pk3u = PackedConv(w3, b3, 3, DEV, torch.bfloat16, False)
        with R.use_opts(conv_ws3=1):  # the 3x3 conv in conv_big's summation order, as inside the fused launch (conv_ws3 has its own test)
            t = hip_conv2d(xd, pk3u, 1, 1, L.ACT_SILU)
        cout = 64 if kind == 1 else ncp
        w1p = torch.cat([w1, torch.zeros(cout - cout1, c, 1, 1)], 0)
        b1p = torch.cat([b1, torch.zeros(cout - cout1)], 0)
        pk1 = PackedConv(w1p, b1p, 1, DEV, torch.bfloat16, False)
        vt = R.view_of(t)
        L.check(L.lib().upa_detect_tail(vt.ptr, vt.n, vt.h, vt.w, vt.c, vt.ld, pk1.w.data_ptr(), pk1.bias.data_ptr(), cout, kind, nc,
                                        16.0, y2.data_ptr(), a_total, a0, None, 0, None, L.UPA_BF16, R.opts_ptr(), L.current_stream(DEV)),
                "detect_tail")
    torch.cuda.synchronize()
    got, two = y[:, :, a0:a0 + h * w].cpu(), y2[:, :, a0:a0 + h * w].cpu()
    d = (got - two).abs()
    # the two-launch path may run its 3x3 conv in another kernel (other f32 summation order): a few intermediate values
    # round to the neighbouring bf16, which moves a logit by <= 2^-8 |h| |w|; everything else agrees to f32 rounding
    flips = (d[:, 4:] > 1e-5).float().mean().item()
    assert d[:, :4].max().item() <= 2e-2 and d[:, 4:].max().item() <= 2e-3 and flips <= 0.02, \
        (d[:, :4].max().item(), d[:, 4:].max().item(), flips)
    assert float(y[:, :, :a0].min()) == -7.0 and float(y[:, :, a0 + h * w:].max()) == -7.0
    # every anchor of the level carries the NMS key of its best class: (~bits(best) << 32) | (anchor * nc + first argmax) in
    # utils/nms key order (torch.max = first maximum); anchors outside the level are untouched
    yc, keys = y.cpu(), best_keys.cpu()
    sc = yc[:, 4:, a0:a0 + h * w]
    best, arg = sc.max(1)  # (n, h*w), first maximum
    bits = best.contiguous().numpy().view(np.uint32).astype(np.uint64)
    anchors = np.arange(a0, a0 + h * w, dtype=np.uint64)
    want = ((~bits & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | (anchors[None, :] * np.uint64(nc) + arg.numpy().astype(np.uint64))
    assert np.array_equal(keys[:, a0:a0 + h * w].numpy().view(np.uint64), want)
    assert bool((keys[:, :a0] == -1).all()) and bool((keys[:, a0 + h * w:] == -1).all())
    oref = om.Detect(nc, (64,)).eval()
    oref.stride = torch.tensor([16.0])
    ref = oref._inference([torch.cat(raws, 1)])
    d = (got - ref).abs()
    # a bf16 rounding of the intermediate that falls the other way (f32 summation order) moves a logit by <= 2^-8 * |h| * |w|
    assert d[:, :4].max().item() <= 0.5 and d[:, :4].mean().item() <= 5e-3 and d[:, 4:].max().item() <= 1e-2, \
        (d[:, :4].max().item(), d[:, :4].mean().item(), d[:, 4:].max().item())


def test_rtdetr_decoder_small_matches_golden(golden_dir):
    """RTDETRDecoder(hd=32, nq=10, nh=4, ndl=2, d_ffn=64) on three tiny maps vs the reference's recorded output."""
    from tests.hip_utils import DEV, bn_fix, to_dev_nhwc, unit_input
    from ultralytics_pro_amd.nn.modules.rtdetr import RTDETRDecoder
    G = np.load(golden_dir / "ops_unit.npz")
    r = bn_fix(RTDETRDecoder(80, (16, 32, 64), 32, 10, 4, 4, 2, 64))
    P.apply_procedural_weights(r)
    r = r.to(DEV)
    xs = [to_dev_nhwc(unit_input(f"rtd{i}", s)) for i, s in enumerate([(2, 16, 8, 8), (2, 32, 4, 4), (2, 64, 2, 2)])]
    with torch.no_grad():
        y = r(xs)[0]
    torch.cuda.synchronize()
    assert y.shape == (2, 10, 84)
    assert np.abs(y.cpu().numpy() - G["rtdetr_decoder_small"]).max() <= 1e-4


def test_msdeform_attn_matches_golden(golden_dir):
    from tests.hip_utils import DEV, unit_input
    from ultralytics_pro_amd.nn.modules.rtdetr import MSDeformAttn
    G = np.load(golden_dir / "ops_unit.npz")
    m = MSDeformAttn(32, 3, 4, 4).eval()
    P.apply_procedural_weights(m)
    m = m.to(DEV)
    q = unit_input("msda_q", (2, 10, 32)).to(DEV)
    ref_b = unit_input("msda_ref", (2, 10, 1, 4), 0.1, 0.9).to(DEV)
    val = unit_input("msda_v", (2, 84, 32))
    # level-major token rows: [all images of level 0 | level 1 | level 2]
    shapes = [[8, 8], [4, 4], [2, 2]]
    parts, t0 = [], 0
    for h, w in shapes:
        parts.append(val[:, t0: t0 + h * w].reshape(-1, 32))
        t0 += h * w
    value_rows = torch.cat(parts, 0).contiguous().to(DEV)
    shp = torch.tensor([d for s_ in shapes for d in s_], dtype=torch.int32)
    with torch.no_grad():
        y = m(q.reshape(20, 32).contiguous(), ref_b.reshape(20, 4).contiguous(), value_rows, {"host_ptr": shp.data_ptr()}, 2)
    torch.cuda.synchronize()
    assert np.abs(y.cpu().numpy().reshape(2, 10, 32) - G["msdeform_attn"]).max() <= 1e-5


def _nms_names(g):
    return sorted(k[:-5] for k in g.files if k.endswith("_pred"))


def test_nms_golden_cases_bit_exact(golden_dir):
    """Every reference NMS fixture (hand cases + random dense cases): rows, counts and kept indices bit-exact."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.utils.nms import non_max_suppression
    g = np.load(golden_dir / "nms_cases.npz")
    for name in _nms_names(g):
        kw = json.loads(str(g[name + "_kw"]))
        pred = torch.from_numpy(g[name + "_pred"]).to(DEV)
        out, keep = non_max_suppression(pred, return_idxs=True, **kw)
        assert [o.shape[0] for o in out] == list(g[name + "_n"]), name
        rows = torch.cat(out, 0).cpu().numpy()
        assert np.array_equal(rows, g[name + "_out"]), name
        assert np.array_equal(torch.cat(keep).cpu().numpy(), g[name + "_keep"]), name


_NMS_BIG_REF = {}


@pytest.mark.parametrize("staging", [{}, {"nms_stages": 1}, {"nms_stages": 1, "nms_first_prefix": -1}, {"nms_stages": 2},
                                     {"nms_first_prefix": 256}, {"nms_first_prefix": 12000}],
                         ids=["default", "all_keys", "all_keys_16384", "radix_select", "prefix_256", "prefix_12000"])
def test_nms_large_multilabel_vs_oracle(staging):
    """> max_nms candidates (radix select + global bitonic path) and ragged per-image counts, vs the oracle - under every staging of
    long multi-label lists (upa_opts.nms_stages / nms_first_prefix: the forms differ in which kernels find the sorted prefixes, never
    in the result)."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.utils.nms import non_max_suppression as _nms

    def non_max_suppression(*a, **k):
        with R.use_opts(L.Opts(**staging)):
            return _nms(*a, **k)

    def oracle(name, t, **k):  # (the same scenes for every staging: the oracle's Python loop runs once per scene)
        key = (name, repr(sorted(k.items())))
        if key not in _NMS_BIG_REF:
            _NMS_BIG_REF[key] = onms.non_max_suppression(t.clone(), **k)
        return _NMS_BIG_REF[key]
    torch.set_num_threads(4)  # the oracle's Python NMS loop crawls when oversubscribed on the 256-core GPU host
    n = 1200
    p = torch.zeros(3, 84, n)
    u = P.uniform("nmsbig:box", (3, 4, n), 0, 1)
    p[:, 0] = u[:, 0] * 600 + 20
    p[:, 1] = u[:, 1] * 600 + 20
    p[:, 2] = u[:, 2] * 60 + 10
    p[:, 3] = u[:, 3] * 60 + 10
    p[:, 4:] = P.uniform("nmsbig:cls", (3, 80, n), 0, 1) ** 4
    p[2, 4:, 100:] = 0  # ragged: third image has few candidates
    for kw in (dict(conf_thres=0.001, iou_thres=0.7, multi_label=True, max_det=300, max_nms=30000),  # > LDS sort cap
               dict(conf_thres=0.05, iou_thres=0.5, multi_label=True, max_det=100, max_nms=2000),    # radix select
               dict(conf_thres=0.001, iou_thres=0.6, multi_label=True, max_det=300, max_nms=30000, classes=[0, 3, 17, 42, 78, 79],
                    agnostic=True),                                                                   # class filter inside the histogram / emit sweeps
               dict(conf_thres=0.25, iou_thres=0.45)):
        ref = oracle("p", p, **kw)
        out = non_max_suppression(p.to(DEV), **kw)
        for a, b in zip(out, ref):
            assert a.shape == b.shape
            assert torch.equal(a.cpu(), b), kw
    # the two-stage sort (round 4): with more than 16384 candidates only the top 16384 are sorted first (in LDS); an image whose
    # greedy pass exhausts them before max_det boxes are kept must come out of the second, full pass.  Image 0: 300 anchors share ONE
    # box and carry the highest scores in every class (24000 candidates - more than the 16384 of the first pass, fewer than max_nms -
    # that keep one box per class = 80 < max_det) in front of 900 distinct low-score boxes; image 1: the ordinary scene; image 2: few candidates.
    q = p.clone()
    q[0, 0, :300], q[0, 1, :300], q[0, 2, :300], q[0, 3, :300] = 300.0, 300.0, 50.0, 40.0
    q[0, 4:, :300] = 0.5 + 0.5 * P.uniform("nmsbig:dup", (80, 300), 0, 1)
    q[0, 4:, 300:] = 0.002 + 0.4 * P.uniform("nmsbig:low", (80, 900), 0, 1) ** 6
    kw = dict(conf_thres=0.001, iou_thres=0.7, multi_label=True, max_det=300, max_nms=30000)
    ref = oracle("q", q, **kw)
    out = non_max_suppression(q.to(DEV), **kw)
    assert ref[0].shape[0] > 80  # the distinct boxes behind the duplicates are needed: the first pass alone would stop at 80
    for a, b in zip(out, ref):
        assert a.shape == b.shape and torch.equal(a.cpu(), b)
    # the first stage picks its prefix from a coarse score histogram (round 5): scores that all fall in ONE coarse bin leave no usable
    # prefix (the exact radix select runs instead).  Image 0: 24000 candidates with the SAME score (order = candidate index), image 1:
    # scores inside one bin (0.75 .. 0.7529), image 2: the ordinary scene
    r = p.clone()
    r[2] = p[1]
    r[0, 4:, :300] = 0.6
    r[0, 4:, 300:] = 0.0
    r[1, 4:, :400] = 0.75 + 0.0029 * P.uniform("nmsbig:onebin", (80, 400), 0, 1)
    r[1, 4:, 400:] = 0.0005
    ref = oracle("r", r, **kw)
    out = non_max_suppression(r.to(DEV), **kw)
    for a, b in zip(out, ref):
        assert a.shape == b.shape and torch.equal(a.cpu(), b)


def test_nms_staging_options_are_validated():
    """upa_opts.nms_stages / nms_first_prefix outside their documented ranges are refused (UPA_EINVAL), not silently clamped."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.utils.nms import non_max_suppression
    p = torch.zeros(1, 84, 64, device=DEV)
    for bad in ({"nms_stages": 3}, {"nms_stages": -1}, {"nms_first_prefix": 100}, {"nms_first_prefix": 16384}, {"nms_first_prefix": -2}):
        with R.use_opts(L.Opts(**bad)), pytest.raises(L.UpaError):
            non_max_suppression(p, multi_label=True)
    with R.use_opts(L.Opts(nms_stages=2, nms_first_prefix=256)):
        assert non_max_suppression(p, multi_label=True)[0].shape == (0, 6)


def test_cpu_tensor_fails_loudly():
    from ultralytics_pro_amd._lib import UpaError
    pm, _ = _mods()
    with pytest.raises(UpaError):
        pm.Conv(16, 16, 3).eval()(torch.zeros(1, 16, 8, 8))


def test_stem_reads_uint8_bgr_frames():
    """uint8 HWC BGR frames go straight into the first conv (BGR->RGB, HWC->CHW, /255 fused),
    against the reference's preprocess semantics (engine/predictor.py:151-173) followed by the oracle Conv."""
    from tests.hip_utils import DEV, to_cpu_nchw
    pm, _ = _mods()
    o, m = _pair(om.Conv, pm.Conv, (3, 16, 3, 2), "stem_u8")
    frames = (P.hash_uniform("u8frames", 2 * 48 * 64 * 3) * 256).astype("uint8").reshape(2, 48, 64, 3)  # BGR
    ref_in = torch.from_numpy(frames[..., ::-1].transpose(0, 3, 1, 2).copy()).float() / 255  # predictor.preprocess
    m.compute_dtype = torch.float32
    with torch.no_grad():
        ref = o(ref_in)
        y = to_cpu_nchw(m(torch.from_numpy(frames).to(DEV)))
    assert (y - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("fmt", ["f32", "bf16", "u8"])
@pytest.mark.parametrize("case", [(16, 3, 2, None, 50, 67), (32, 3, 1, None, 21, 130), (16, 6, 2, 2, 70, 66), (64, 3, 2, None, 24, 40)],
                         ids=["v8n_odd", "v3_s1", "v5_k6", "cout64"])
def test_stem_mfma_formats_and_ragged_sizes(case, fmt):
    """bf16 compute mode of the first conv (MFMA form): f32 / bf16 NCHW and uint8 BGR HWC inputs, odd widths (unaligned
    column pairs), partial tiles. Reference = oracle Conv on the bf16-rounded input (conv.py:188-197)."""
    from tests.hip_utils import DEV, bf16_round, to_cpu_nchw
    pm, _ = _mods()
    c2, k, s, p, H, W = case
    o, m = _pair(om.Conv, pm.Conv, (3, c2, k, s, p), "stem_mfma")
    m.compute_dtype = torch.bfloat16
    if fmt == "u8":
        frames = (P.hash_uniform(f"u8m{case}", 2 * H * W * 3) * 256).astype("uint8").reshape(2, H, W, 3)
        x = torch.from_numpy(frames[..., ::-1].transpose(0, 3, 1, 2).copy()).float() / 255
        xin = torch.from_numpy(frames).to(DEV)
    else:
        x = P.uniform(f"stemm{case}", (2, 3, H, W), 0, 1)
        xin = x.to(DEV).to(torch.bfloat16) if fmt == "bf16" else x.to(DEV)
    with torch.no_grad():
        ref = o(bf16_round(x))
        y = to_cpu_nchw(m(xin))
    assert y.shape == ref.shape
    assert (y - ref).abs().max().item() <= 2e-2 * max(1.0, ref.abs().max().item())


def test_scale_boxes_matches_reference_formula():
    """scale_boxes + clip_boxes (utils/ops.py:102-178): letterboxed 640x640 -> 1080x810 original, and ratio_pad form."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.utils.ops import scale_boxes
    b = P.uniform("scale_boxes", (50, 6), -20, 660)
    for img1, img0, rp in (((640, 640), (1080, 810), None), ((384, 640), (720, 1280), None),
                           ((640, 640), (500, 375), ((1.28,), (80.0, 0.0)))):
        ref = b.clone()
        if rp is None:
            gain = min(img1[0] / img0[0], img1[1] / img0[1])
            px, py = round((img1[1] - img0[1] * gain) / 2 - 0.1), round((img1[0] - img0[0] * gain) / 2 - 0.1)
        else:
            gain, (px, py) = rp[0][0], rp[1]
        ref[:, [0, 2]] -= px
        ref[:, [1, 3]] -= py
        ref[:, :4] /= gain
        ref[:, 0].clamp_(0, img0[1]); ref[:, 1].clamp_(0, img0[0]); ref[:, 2].clamp_(0, img0[1]); ref[:, 3].clamp_(0, img0[0])
        got = scale_boxes(img1, b.clone().to(DEV), img0, ratio_pad=rp)
        assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("cfg", ["yolov8n", "yolov5-BoT3", "yolov8s", "yolov3-rtdetr"], ids=["k3", "k6", "c32", "c32s1"])
@pytest.mark.parametrize("shape", [(2, 3, 128, 128), (3, 3, 100, 136), (1, 3, 64, 256)], ids=["sq", "ragged", "wide"])
def test_fused_stem_and_second_conv_equals_the_two_layers(shape, cfg):
    """Rows 0-1 of yolov8n (Conv(3,16,3,2) -> Conv(16,32,3,2)), of the yolov5 family (Conv(3,16,6,2,2) -> Conv(16,32,3,2)) and of yolov8s
    (Conv(3,32,3,2) -> Conv(32,64,3,2)) and darknet53 (yolov3-rtdetr: Conv(3,32,3,1) -> Conv(32,64,3,2)) as one kernel (upa_stem_conv_fused_c: the stem output stays in LDS) vs the two separate HIP layers and vs the oracle (Conv,
    conv.py:188-197) on a bf16 NCHW input; image borders, partial tiles, odd tile counts."""
    from tests.hip_utils import DEV, bf16_round, to_cpu_nchw
    from ultralytics_pro_amd.nn.tasks import DetectionModel
    from oracle import tasks as ot
    m = DetectionModel(cfg + ".yaml")
    P.apply_procedural_weights(m)
    m = m.to(DEV).eval()
    m.set_compute_dtype(torch.bfloat16)
    x = bf16_round(P.uniform(f"fstem{shape}", shape, 0, 1))
    xd = x.to(DEV).to(torch.bfloat16).contiguous()
    with torch.no_grad():
        assert m._stem_fusable(xd, m._concat_placement()), cfg
        fused = to_cpu_nchw(m._fused_stem(xd))
        two = to_cpu_nchw(m.model[1](m.model[0](xd)))
        o = ot.DetectionModel(cfg + ".yaml")
        P.apply_procedural_weights(o)
        from tests.hip_utils import assert_bf16_close, bf16_weight_oracle
        l0, l1 = bf16_weight_oracle(o.model[0]), bf16_weight_oracle(o.model[1])
        ref = l1(bf16_round(l0(x)))  # the stem tile is rounded to bf16 in LDS, as the separate layers round it in HBM
    assert fused.shape == two.shape == ref.shape
    scale = max(1.0, float(ref.abs().max()))
    assert float((fused - two).abs().max()) <= 2e-2 * scale
    assert_bf16_close(fused, ref, f"fused_stem{shape}", abs_=2.0 ** -7)  # (flipped ties of the bf16 stem tile: see the pair test)


def test_results_to_host_kernel():
    """`upa_results_to_host`: counts + only the first counts[b] rows of every image reach pinned host memory, in one launch
    (capturable: no memcpy node); rows past the count are left untouched on the host."""
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    b, m = 5, 300
    rows = torch.arange(b * m * 6, dtype=torch.float32, device=DEV).reshape(b, m, 6)
    counts = torch.tensor([0, 1, 300, 57, 299], dtype=torch.int32, device=DEV)
    hrows = torch.full((b, m, 6), -1.0, pin_memory=True)
    hcounts = torch.full((b,), -1, dtype=torch.int32, pin_memory=True)
    L.check(L.lib().upa_results_to_host(rows.data_ptr(), counts.data_ptr(), b, m, 24, hrows.data_ptr(), hcounts.data_ptr(),
                                        L.current_stream(DEV)), "results_to_host")
    torch.cuda.synchronize()
    assert torch.equal(hcounts, counts.cpu())
    rc = rows.cpu()
    for i, c in enumerate(counts.tolist()):
        assert torch.equal(hrows[i, :c], rc[i, :c]) and bool((hrows[i, c:] == -1.0).all())


LINEAR_CASES = [
    # m, k, n, act, residual   (nn.Linear on token rows, `upa_linear`: the small-M kernel of csrc/transformer.hip and its fallbacks)
    (4800, 256, 256, 0, False),   # the RT-DETR decoder's shape: 150 row tiles x 4 column blocks
    (300, 256, 512, 2, False),    # ReLU (FFN linear1), n-tiles past one column block
    (77, 256, 80, 0, True),       # ragged rows (last tile holds 13), N = 5 tiles (a dead wave in the second block), residual
    (45, 1024, 256, 0, True),     # K = 1024: one m-tile per workgroup, weights in four register sets
    (33, 512, 4, 0, False),       # N = 4: one store group of one lane row
    (64, 96, 32, 1, False),       # K = 96 (three 32-channel units), SiLU in f32 (expf + IEEE divide)
    (50, 4, 512, 2, False),       # K = 4 (query_pos_head's first layer): outside the small-M form -> the conv kernel
    (20, 48, 40, 0, True),        # K = 48: not a multiple of 32 -> the conv kernel
    (20000, 256, 1024, 2, False), # many rows AND wide N (16 column blocks): gated off the small-M form -> the conv kernel
    (20000, 256, 256, 0, True),   # many rows, 4 column blocks: stays on the small-M form (the RT-DETR encoder's shape class)
]


TOPK_CASES = [
    # levels (h*w each), classes, batch, k, score pattern
    ([6400, 1600, 400], 80, 3, 300, "random"),      # yolov3-rtdetr at 640 x 640: radix select + sort of the survivors
    ([400, 100, 25], 80, 2, 300, "ties"),           # quantised scores: many equal keys around the k-th
    ([6400, 1600, 400], 80, 2, 300, "flat"),        # every token the same score: more candidates than the cap -> full sort
    ([100, 25], 6, 2, 50, "random"),                # class count not a multiple of four: scalar row reads
    ([64], 4, 1, 64, "random"),                     # k = all tokens
]


@pytest.mark.parametrize("case", TOPK_CASES, ids=[f"T{sum(c[0])}_nc{c[1]}_b{c[2]}_k{c[3]}_{c[4]}" for c in TOPK_CASES])
def test_topk_tokens_matches_stable_sort(case):
    """upa_topk_tokens (RTDETRDecoder._get_decoder_input, nn/modules/head.py: topk of the best-class score per token) against a
    stable descending sort of the same scores on the CPU: the same tokens in the same order (ties by token index), and the
    row of each token in the level-major token matrix."""
    import ctypes as C
    from tests.hip_utils import DEV
    from ultralytics_pro_amd import _lib as L
    hw, nc, B, K, pattern = case
    T = sum(hw)
    g = torch.Generator().manual_seed(T + nc)
    rows_total = B * T
    sc = torch.randn(rows_total, nc, generator=g) * 3
    if pattern == "ties":
        sc = (sc * 2).round() / 2
    elif pattern == "flat":
        sc = torch.zeros(rows_total, nc)
    scd = sc.to(DEV)
    out_rows = torch.zeros(B * K, dtype=torch.int32, device=DEV)
    out_tok = torch.zeros(B * K, dtype=torch.int32, device=DEV)
    hw_arr = (C.c_int32 * len(hw))(*hw)
    L.check(L.lib().upa_topk_tokens(scd.data_ptr(), nc, len(hw), hw_arr, B, K, out_rows.data_ptr(), out_tok.data_ptr(),
                                    L.current_stream(DEV)), "topk_tokens")
    torch.cuda.synchronize()
    # level-major token matrix: level l occupies rows row0[l] + b * hw[l] + p
    row0, tok0 = [], []
    r = t = 0
    for n in hw:
        row0.append(r); tok0.append(t); r += n * B; t += n
    for b in range(B):
        rows_of_tok = torch.cat([torch.arange(hw[l]) + row0[l] + b * hw[l] for l in range(len(hw))])
        best = sc[rows_of_tok].max(1).values
        order = torch.sort(best, descending=True, stable=True).indices[:K]
        assert torch.equal(out_tok[b * K:(b + 1) * K].cpu().long(), order)
        assert torch.equal(out_rows[b * K:(b + 1) * K].cpu().long(), rows_of_tok[order])


@pytest.mark.parametrize("case", LINEAR_CASES, ids=[f"m{c[0]}_k{c[1]}_n{c[2]}_a{c[3]}{'_res' if c[4] else ''}" for c in LINEAR_CASES])
def test_linear_f32_rows(case):
    """`upa_linear` (exact-f32 MFMA) vs float64 `x @ W^T + b` -> act -> + residual (nn.Linear / MLP of the RT-DETR head,
    transformer.py:348-399, head.py:1993-2003): strided inputs and outputs (columns of wider buffers), ragged row and column tiles."""
    from tests.hip_utils import DEV, unit_input
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.nn.modules.conv import PackedConv
    m, k, n, act, res = case
    ldx, ldy, ldr = k + 8, n + 12, n + 4
    x = unit_input(f"lin_x{case}", (m, ldx), -1.5, 1.5)
    w = unit_input(f"lin_w{case}", (n, k), -0.2, 0.2)
    b = unit_input(f"lin_b{case}", (n,), -1, 1)
    r = unit_input(f"lin_r{case}", (m, ldr), -1, 1)
    ref = x[:, :k].double() @ w.double().t() + b.double()
    if act == 2:
        ref = ref.clamp(min=0)
    elif act == 1:
        ref = ref * torch.sigmoid(ref)
    if res:
        ref = ref + r[:, :n].double()
    pk = PackedConv(w.reshape(n, k, 1, 1), b, 1, DEV, torch.float32, False)
    xd, rd = x.to(DEV), r.to(DEV)
    y = torch.full((m, ldy), -7.0, device=DEV)
    L.check(L.lib().upa_linear(xd.data_ptr(), m, k, ldx, pk.w.data_ptr(), pk.bias.data_ptr(), y.data_ptr(), n, ldy,
                               rd.data_ptr() if res else None, ldr if res else 0, act, L.current_stream(DEV)), "linear")
    torch.cuda.synchronize()
    got = y.cpu()
    assert float((got[:, :n].double() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))  # f32 accumulation over K <= 1024
    assert bool((got[:, n:] == -7.0).all())  # nothing outside the n output columns


def test_grouped_launches_equal_single_launches():
    """`upa_conv2d_bias_act_group` / `upa_detect_branch_tail_group`: several independent problems in one call - neighbours on the same
    128-pixel conv_big instantiation share ONE grid (conv_big_pair_kernel) - must give bit-identical results to one call per problem:
    the Detect head's first convs and branch tails of an 80 x 80, a 40 x 40 and a 20 x 20 level, box and class kinds: pairs (the default: the large level alone on its 256-pixel variant), all three in one grid (`no_group` = 2:
    the large level on the 128-pixel variant) and one launch per level (`no_group` = 1)."""
    import ctypes as C
    from tests.hip_utils import DEV, bf16_round, to_dev_nhwc, unit_input
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn.modules.conv import PackedConv
    lib, st = L.lib(), L.current_stream(DEV)
    n, nc = 16, 80
    # a 64- and an 80-channel conv on the SAME input and workgroup size (the two first convs of a Detect level): one grid on the five-tile
    # instantiation (the 64-channel problem's fifth n-tile multiplies zero weights and is not stored)
    for (h, w) in ((80, 80), (40, 40)):
        x = to_dev_nhwc(bf16_round(unit_input(f"grp2_x{h}", (n, 64, h, w), -1, 1)), torch.bfloat16)
        pks = [PackedConv(bf16_round(unit_input(f"grp2_w{h}{c}", (c, 64, 3, 3), -0.1, 0.1)), unit_input(f"grp2_b{h}{c}", (c,), -0.5, 0.5), 3, DEV,
                          torch.bfloat16, False) for c in (64, 80)]
        res = {}
        for tag, opts in (("g", L.Opts(conv_ws3=1)), ("s", L.Opts(conv_ws3=1, no_group=1))):
            outs = [R.alloc_nhwc(n, c, h, w, torch.bfloat16, DEV) for c in (64, 80)]
            probs = (L.ConvProblem * 2)()
            for j, c in enumerate((64, 80)):
                vx, vy = R.view_of(x), R.view_of(outs[j])
                probs[j] = L.ConvProblem(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, pks[j].w.data_ptr(), pks[j].bias.data_ptr(), vy.ptr, c, vy.ld, None, 0)
            L.check(lib.upa_conv2d_bias_act_group(C.cast(probs, C.c_void_p), 2, 3, 1, 1, L.ACT_SILU, L.UPA_BF16, C.pointer(opts), st), "conv2d_group")
            res[tag] = outs
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(res["g"], res["s"]))
    levels = [(80, 80, 64), (40, 40, 128), (20, 20, 256)]  # (h, w, cin) of the level's feature map
    for kind, cmid in ((1, 64), (2, 80)):
        xs, pks, outs_g, outs_s = [], [], [], []
        for li, (h, w, cin) in enumerate(levels):
            x = to_dev_nhwc(bf16_round(unit_input(f"grp_x{kind}{li}", (n, cin, h, w), -1, 1)), torch.bfloat16)
            wgt = bf16_round(unit_input(f"grp_w{kind}{li}", (cmid, cin, 3, 3), -0.1, 0.1))
            pk = PackedConv(wgt, unit_input(f"grp_b{kind}{li}", (cmid,), -0.5, 0.5), 3, DEV, torch.bfloat16, False)
            xs.append(x); pks.append(pk)
            outs_g.append(R.alloc_nhwc(n, cmid, h, w, torch.bfloat16, DEV)); outs_s.append(R.alloc_nhwc(n, cmid, h, w, torch.bfloat16, DEV))
        outs_p = [R.alloc_nhwc(n, cmid, h, w, torch.bfloat16, DEV) for (h, w, _) in levels]
        for outs, opts in ((outs_g, None), (outs_s, L.Opts(no_group=1)), (outs_p, L.Opts(no_group=2))):
            probs = (L.ConvProblem * 3)()
            for j in range(3):
                vx, vy = R.view_of(xs[j]), R.view_of(outs[j])
                probs[j] = L.ConvProblem(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, pks[j].w.data_ptr(), pks[j].bias.data_ptr(), vy.ptr, cmid, vy.ld, None, 0)
            L.check(lib.upa_conv2d_bias_act_group(C.cast(probs, C.c_void_p), 3, 3, 1, 1, L.ACT_SILU, L.UPA_BF16,
                                                  C.pointer(opts) if opts is not None else None, st), "conv2d_group")
        torch.cuda.synchronize()
        for a, b, c in zip(outs_g, outs_s, outs_p):
            assert torch.equal(a, b) and torch.equal(a, c)
        # the branch tails on those mid tensors
        cp = 64 if kind == 1 else 80
        a0s, tot = [0, 6400, 8000], 8400
        ys = [torch.full((n, 4 + nc, tot), -7.0, device=DEV) for _ in range(3)]
        keys = [torch.full((n, tot), -1, dtype=torch.int64, device=DEV) for _ in range(3)]
        packed = []
        for li, (h, w, _) in enumerate(levels):
            w3 = bf16_round(unit_input(f"grp_w3{kind}{li}", (cp, cmid, 3, 3), -0.1, 0.1))
            pk3 = PackedConv(w3, unit_input(f"grp_b3{kind}{li}", (cp,), -0.5, 0.5), 3, DEV, torch.bfloat16, False)
            wt = bf16_round(unit_input(f"grp_wt{kind}{li}", (cp, cp), -0.4, 0.4))
            bt = unit_input(f"grp_bt{kind}{li}", (cp,), -2, 1)
            host = torch.empty(lib.upa_tail_packed_weight_bytes(cp, cp), dtype=torch.uint8)
            L.check(lib.upa_pack_tail_weight(wt.data_ptr(), cp, cp, host.data_ptr()), "pack_tail_weight")
            packed.append((pk3, host.to(DEV), bt.to(DEV)))
        for which, opts in ((0, None), (1, L.Opts(no_group=1)), (2, L.Opts(no_group=2))):
            lv = (L.BranchLevel * 3)()
            for j, (h, w, _) in enumerate(levels):
                vt = R.view_of(outs_g[j])
                pk3, wt, bt = packed[j]
                lv[j] = L.BranchLevel(vt.ptr, vt.n, vt.h, vt.w, vt.c, vt.ld, pk3.w.data_ptr(), pk3.bias.data_ptr(), wt.data_ptr(), bt.data_ptr(),
                                      float(8 << j), a0s[j])
            L.check(lib.upa_detect_branch_tail_group(C.cast(lv, C.c_void_p), 3, kind, nc, ys[which].data_ptr(), tot,
                                                     keys[which].data_ptr() if kind == 2 else None, L.UPA_BF16,
                                                     C.pointer(opts) if opts is not None else None, st), "branch_tail_group")
        torch.cuda.synchronize()
        assert torch.equal(ys[0], ys[1]) and torch.equal(keys[0], keys[1]) and torch.equal(ys[0], ys[2]) and torch.equal(keys[0], keys[2])
        rows = slice(0, 4) if kind == 1 else slice(4, 4 + nc)
        assert int((ys[0][:, rows] == -7.0).sum()) == 0  # every anchor of the three levels was written


def test_detect_head_tails_equal_single_launches():
    """`upa_detect_head_tails`: the box and class branch tails of three levels in one call - problems of two kernel instantiations per
    grid (conv_big_mix_kernel: the 80 x 80 level's two tails as one launch, the 40 x 40 and 20 x 20 levels' four as another) - must equal
    one `upa_detect_branch_tail` per branch and level bit for bit, decoded rows and NMS keys."""
    import ctypes as C
    from tests.hip_utils import DEV, bf16_round, to_dev_nhwc, unit_input
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn.modules.conv import PackedConv
    lib, st = L.lib(), L.current_stream(DEV)
    n, nc, tot = 16, 80, 8400
    levels = [(80, 80, 0), (40, 40, 6400), (20, 20, 8000)]
    packed = {}
    for kind, c in ((1, 64), (2, 80)):
        for li, (h, w, a0) in enumerate(levels):
            t = to_dev_nhwc(bf16_round(unit_input(f"ht_t{kind}{li}", (n, c, h, w), -1.5, 1.5)), torch.bfloat16)
            pk3 = PackedConv(bf16_round(unit_input(f"ht_w3{kind}{li}", (c, c, 3, 3), -0.1, 0.1)), unit_input(f"ht_b3{kind}{li}", (c,), -0.5, 0.5),
                             3, DEV, torch.bfloat16, False)
            wt = bf16_round(unit_input(f"ht_wt{kind}{li}", (c, c), -0.4, 0.4))
            bt = unit_input(f"ht_bt{kind}{li}", (c,), -2, 1)
            host = torch.empty(lib.upa_tail_packed_weight_bytes(c, c), dtype=torch.uint8)
            L.check(lib.upa_pack_tail_weight(wt.data_ptr(), c, c, host.data_ptr()), "pack_tail_weight")
            packed[(kind, li)] = (t, pk3, host.to(DEV), bt.to(DEV))
    ys = [torch.full((n, 4 + nc, tot), -7.0, device=DEV) for _ in range(3)]
    keys = [torch.full((n, tot), -1, dtype=torch.int64, device=DEV) for _ in range(3)]
    for which, opts in ((0, None), (1, L.Opts(no_group=1))):
        lvs = {}
        for kind in (1, 2):
            lv = (L.BranchLevel * 3)()
            for j, (h, w, a0) in enumerate(levels):
                t, pk3, wt, bt = packed[(kind, j)]
                vt = R.view_of(t)
                lv[j] = L.BranchLevel(vt.ptr, vt.n, vt.h, vt.w, vt.c, vt.ld, pk3.w.data_ptr(), pk3.bias.data_ptr(), wt.data_ptr(), bt.data_ptr(),
                                      float(8 << j), a0)
            lvs[kind] = lv
        L.check(lib.upa_detect_head_tails(C.cast(lvs[1], C.c_void_p), C.cast(lvs[2], C.c_void_p), 3, nc, ys[which].data_ptr(), tot,
                                          keys[which].data_ptr(), L.UPA_BF16, C.pointer(opts) if opts is not None else None, st), "head_tails")
    for kind in (1, 2):  # one launch per branch and level
        for j, (h, w, a0) in enumerate(levels):
            t, pk3, wt, bt = packed[(kind, j)]
            vt = R.view_of(t)
            L.check(lib.upa_detect_branch_tail(vt.ptr, vt.n, vt.h, vt.w, vt.c, vt.ld, pk3.w.data_ptr(), pk3.bias.data_ptr(), wt.data_ptr(),
                                               bt.data_ptr(), kind, nc, float(8 << j), ys[2].data_ptr(), tot, a0,
                                               keys[2].data_ptr() if kind == 2 else None, L.UPA_BF16, None, st), "branch_tail")
    torch.cuda.synchronize()
    assert torch.equal(ys[0], ys[2]) and torch.equal(ys[1], ys[2]) and torch.equal(keys[0], keys[2]) and torch.equal(keys[1], keys[2])
    assert int((ys[0] == -7.0).sum()) == 0 and int((keys[0] == -1).sum()) == 0



POOL_CASES = [  # cin, cout, n, h, w  (cin 3 = the first layer on an NCHW image)
    (3, 16, 2, 64, 128), (3, 16, 1, 40, 72), (3, 32, 1, 16, 64),
    (16, 32, 2, 32, 48), (32, 64, 1, 24, 32), (64, 128, 2, 16, 16), (24, 96, 1, 8, 32), (16, 32, 3, 64, 64),
]


@pytest.mark.parametrize("case", POOL_CASES, ids=[f"c{c[0]}-{c[1]}_{c[2]}x{c[3]}x{c[4]}" for c in POOL_CASES])
def test_conv_maxpool_fused_equals_two_launches(case):
    """`Conv.forward_pool2` (`upa_conv2d_stem_nchw_pool2` / `upa_conv2d_pool2`): Conv(k 3, s 1) + SiLU + nn.MaxPool2d(2, 2, 0) as one
    launch must equal the conv launch followed by `upa_maxpool2d` BIT FOR BIT (the pool runs on the bf16-rounded activations), and
    both must match the oracle's conv -> pool at bf16 resolution.  Tiles with ragged right / bottom edges included."""
    from tests.hip_utils import DEV, assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc, unit_input
    pm, rs = _mods()
    cin, cout, n, h, w = case
    o, m = _pair(om.Conv, pm.Conv, (cin, cout, 3, 1), f"pool{case}")
    m.compute_dtype = torch.bfloat16
    x = bf16_round(unit_input(f"poolx{case}", (n, cin, h, w)))
    xd = x.to(DEV).to(torch.bfloat16).contiguous() if cin == 3 else to_dev_nhwc(x, torch.bfloat16)
    with torch.no_grad():
        two = to_cpu_nchw(rs.MaxPool2d(2, 2, 0)(m(xd)))
        one = m.forward_pool2(xd)
        assert one is not None, "the case is inside the fused form"
        one = to_cpu_nchw(one)
        ref = torch.nn.functional.max_pool2d(bf16_weight_oracle(o)(x), 2, 2, 0)
    assert one.shape == two.shape == ref.shape
    assert torch.equal(one, two)
    assert_bf16_close(one, ref, f"conv+pool {case}")


def test_conv_maxpool_fused_refuses_outside_the_form():
    from tests.hip_utils import DEV, to_dev_nhwc, unit_input
    pm, _ = _mods()
    _, m = _pair(om.Conv, pm.Conv, (16, 32, 3, 1), "poolrefuse")
    with torch.no_grad():
        assert m.forward_pool2(to_dev_nhwc(unit_input("pr1", (1, 16, 16, 16)), torch.float32)) is None  # f32 mode
        assert m.forward_pool2(to_dev_nhwc(unit_input("pr2", (1, 16, 12, 16)), torch.bfloat16)) is None  # h % 8 != 0
    _, m2 = _pair(om.Conv, pm.Conv, (16, 32, 3, 2), "poolrefuse2")
    with torch.no_grad():
        assert m2.forward_pool2(to_dev_nhwc(unit_input("pr3", (1, 16, 16, 16)), torch.bfloat16)) is None  # stride 2


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("cls,args,xshape", [("C3", (64, 64, 2, True), (2, 64, 12, 20)), ("C3", (48, 32, 1, False), (1, 48, 9, 9)),
                                             ("BoT3", (64, 64, 1, 0.5, 1, 6, 6), (2, 64, 6, 6))], ids=["c3_n2", "c3_48_32", "bot3"])
def test_c3_stacked_cv1_cv2_equals_separate_launches(cls, args, xshape, dtype):
    """C3 / BoT3 with cv1 and cv2 as ONE launch (their BN-folded filters stacked; `block._stacked_cv12`) and MHSA's query / key /
    value likewise, against the same module with the switches off and against the oracle."""
    from tests.hip_utils import assert_bf16_close, bf16_round, to_cpu_nchw, to_dev_nhwc, unit_input
    pm, _ = _mods()
    o, m = _pair(getattr(om, cls), getattr(pm, cls), args, f"stack_{cls}{args}")
    x = unit_input(f"stackx{cls}{xshape}", xshape)
    if dtype == torch.bfloat16:
        x = bf16_round(x)
    xd = to_dev_nhwc(x, dtype)
    saved = (pm.C3.stack_cv12, pm.BoT3.stack_cv12, pm.MHSA.stack_qkv)
    try:
        with torch.no_grad():
            y1 = to_cpu_nchw(m(xd))
            pm.C3.stack_cv12 = pm.BoT3.stack_cv12 = pm.MHSA.stack_qkv = False
            y0 = to_cpu_nchw(m(xd))
            ref = o(x)
    finally:
        pm.C3.stack_cv12, pm.BoT3.stack_cv12, pm.MHSA.stack_qkv = saved
    if dtype == torch.float32:
        assert (y1 - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
        assert (y1 - y0).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
    else:
        tol = 4e-2 * max(1.0, ref.abs().max().item())  # three to five bf16 layers deep (the blocks' own golden tests use 6e-2)
        assert (y1 - ref).abs().max().item() <= tol and (y1 - y0).abs().max().item() <= tol


P8_CASES = [
    # c1, c2, H, W, N, act, residual  (csrc/conv_p8.hip: Cin % 64 == 0, Cout % 128 == 0, 3x3 stride 1)
    (128, 128, 80, 80, 1, True, False),    # two chunks
    (256, 512, 40, 40, 2, True, False),    # four workgroup columns, four chunks
    (512, 256, 20, 20, 2, True, True),     # the Bottleneck shortcut
    (64, 128, 33, 47, 1, False, False),    # one chunk, ragged right / bottom tiles, no activation
    (128, 256, 9, 11, 3, True, True),      # a map smaller than a tile, shortcut
    (192, 128, 24, 56, 1, True, False),    # three chunks
    (1024, 128, 20, 20, 1, True, False),   # sixteen chunks: the halo double buffer and the weight ring wrap many times
    (64, 256, 16, 16, 2, True, True),      # ONE chunk: the prefetch of a chunk that does not exist (zero pieces), shortcut
]


@pytest.mark.parametrize("case", P8_CASES, ids=[f"c{c[0]}-{c[1]}_{c[2]}x{c[3]}n{c[4]}{'' if c[5] else '_lin'}{'_res' if c[6] else ''}" for c in P8_CASES])
def test_conv_p8_kernel(case):
    """bf16 3x3 convs forced through conv_p8_kernel (upa_opts.conv_p8 = 2: the 8-wave two-group phased kernel, csrc/conv_p8.hip) vs the
    oracle Conv (conv.py:188-197, + the Bottleneck add block.py:668) on BN-folded bf16 weights: every tile shape the host picks, 1 - 16
    chunks (halo double buffer, 4-slab weight ring, counted vmcnt), 1 - 4 workgroup columns, the shortcut read."""
    from tests.hip_utils import assert_bf16_close, bf16_round, bf16_weight_oracle, to_cpu_nchw, to_dev_nhwc
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    pm, _ = _mods()
    c1, c2, H, W, N, act, res = case
    with R.use_opts(conv_p8=2):
        var = L.lib().upa_conv_variant(N, H, W, c1, c2, 3, 1, 1, 1, R.opts_ptr())
        assert (var >> 26) & 1, "case is not dispatched to conv_p8"
        o, m = _pair(om.Conv, pm.Conv, (c1, c2, 3, 1, None, 1, 1, act), "conv_p8")
        x = bf16_round(P.uniform(f"p8{case}", (N, c1, H, W), -1, 1))
        rsd = bf16_round(P.uniform(f"p8res{case}", (N, c2, H, W), -1, 1)) if res else None
        with torch.no_grad():
            ref = bf16_weight_oracle(o)(x) + (rsd if res else 0)
            y = to_cpu_nchw(m(to_dev_nhwc(x, torch.bfloat16), residual=to_dev_nhwc(rsd, torch.bfloat16) if res else None))
    assert_bf16_close(y, ref, f"conv_p8{case}")


@pytest.mark.parametrize("shape", [(512, 256, 40, 40, 16), (128, 256, 80, 80, 16), (512, 1024, 20, 20, 16)],
                         ids=["512-256_40", "128-256_80", "512-1024_20"])
def test_conv_p8_equals_conv_big_full_size(shape):
    """At the yolov3-rtdetr batch-16 layer sizes conv_p8 must be BIT-IDENTICAL to conv_big (same fragments, same accumulation order:
    chunk, tap, k-tile) - and stay so over 30 back-to-back launches with other work in flight (a screen for the races a phased kernel
    can have: a fragment read before its DMA landed, a buffer re-staged under a reader)."""
    from tests.hip_utils import bf16_round, to_dev_nhwc
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    pm, _ = _mods()
    c1, c2, H, W, N = shape
    _, m = _pair(om.Conv, pm.Conv, (c1, c2, 3, 1, None, 1, 1, True), "conv_p8_full")
    x = to_dev_nhwc(bf16_round(P.uniform(f"p8full{shape}", (N, c1, H, W), -1, 1)), torch.bfloat16)
    with torch.no_grad():
        with R.use_opts(conv_p8=1):
            var = L.lib().upa_conv_variant(N, H, W, c1, c2, 3, 1, 1, 1, R.opts_ptr())
            assert (var >> 23) & 1 and not (var >> 26) & 1
            ref = m(x).clone()
        with R.use_opts(conv_p8=2):
            var = L.lib().upa_conv_variant(N, H, W, c1, c2, 3, 1, 1, 1, R.opts_ptr())
            assert (var >> 26) & 1
            outs = [m(x).clone() for _ in range(30)]
    torch.cuda.synchronize()
    bad = [i for i, y in enumerate(outs) if not torch.equal(y, ref)]
    assert not bad, f"conv_p8 differs from conv_big in launches {bad}: max|d| {max((outs[i].float() - ref.float()).abs().max().item() for i in bad)}"


LINEAR_BF16_CASES = [c for c in LINEAR_CASES if c[1] % 32 == 0 and c[1] <= 1024]


@pytest.mark.parametrize("case", LINEAR_BF16_CASES, ids=[f"m{c[0]}_k{c[1]}_n{c[2]}_a{c[3]}{'_res' if c[4] else ''}" for c in LINEAR_BF16_CASES])
def test_linear_bf16_product_rows(case):
    """`upa_linear_bf16` (the RT-DETR decoder's perf mode: float32 rows in and out, the product on the bf16 matrix cores) vs float64
    `bf16(x) @ bf16(W)^T + b` -> act -> + residual: with BOTH operands rounded as the kernel rounds them the only difference left is the
    order of the f32 accumulation, so the f32-GEMM bound holds; same strided / ragged shapes as the exact-f32 test."""
    from tests.hip_utils import DEV, bf16_round, unit_input
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.nn.modules.conv import PackedConv
    m, k, n, act, res = case
    ldx, ldy, ldr = k + 8, n + 12, n + 4
    x = unit_input(f"lin_x{case}", (m, ldx), -1.5, 1.5)
    w = unit_input(f"lin_w{case}", (n, k), -0.2, 0.2)
    b = unit_input(f"lin_b{case}", (n,), -1, 1)
    r = unit_input(f"lin_r{case}", (m, ldr), -1, 1)
    ref = bf16_round(x[:, :k]).double() @ bf16_round(w).double().t() + b.double()
    if act == 2:
        ref = ref.clamp(min=0)
    elif act == 1:
        ref = ref * torch.sigmoid(ref)
    if res:
        ref = ref + r[:, :n].double()
    pk = PackedConv(w.reshape(n, k, 1, 1), b, 1, DEV, torch.bfloat16, False)
    xd, rd = x.to(DEV), r.to(DEV)
    y = torch.full((m, ldy), -7.0, device=DEV)
    L.check(L.lib().upa_linear_bf16(xd.data_ptr(), m, k, ldx, pk.w.data_ptr(), pk.bias.data_ptr(), y.data_ptr(), n, ldy,
                                    rd.data_ptr() if res else None, ldr if res else 0, act, L.current_stream(DEV)), "linear_bf16")
    torch.cuda.synchronize()
    got = y.cpu()
    assert float((got[:, :n].double() - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max()))
    assert bool((got[:, n:] == -7.0).all())


@pytest.mark.parametrize("xb,yb", [(False, True), (True, False), (True, True)], ids=["f32_to_bf16", "bf16_to_f32", "bf16_to_bf16"])
@pytest.mark.parametrize("case", [(300, 256, 512, 0, False), (77, 256, 256, 0, True), (45, 1024, 256, 2, False), (4800, 256, 768, 0, False)],
                         ids=["m300", "m77_res", "k1024_relu", "m4800"])
def test_linear_mixed_row_types(case, xb, yb):
    """`upa_linear_mixed`: bf16 rows in (no conversion: the attention output feeding out_proj) and / or bf16 rows out (q, k, v for the
    matrix-core attention kernel) vs float64 on the bf16-rounded operands; a bf16 result must be the nearest bf16 of the float32 one
    up to the accumulation-order noise (half a bf16 ulp + the f32 bound)."""
    from tests.hip_utils import DEV, bf16_round, unit_input
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.nn.modules.conv import PackedConv
    m, k, n, act, res = case
    ldx, ldy, ldr = k + 8, n + 12, n + 4
    x = bf16_round(unit_input(f"linm_x{case}", (m, ldx), -1.5, 1.5))
    w = unit_input(f"linm_w{case}", (n, k), -0.2, 0.2)
    b = unit_input(f"linm_b{case}", (n,), -1, 1)
    r = unit_input(f"linm_r{case}", (m, ldr), -1, 1)
    ref = x[:, :k].double() @ bf16_round(w).double().t() + b.double()
    if act == 2:
        ref = ref.clamp(min=0)
    if res:
        ref = ref + r[:, :n].double()
    pk = PackedConv(w.reshape(n, k, 1, 1), b, 1, DEV, torch.bfloat16, False)
    xd = x.to(DEV).to(torch.bfloat16) if xb else x.to(DEV)
    rd = r.to(DEV)
    y = torch.full((m, ldy), -7.0, device=DEV, dtype=torch.bfloat16 if yb else torch.float32)
    code = lambda f: L.UPA_BF16 if f else L.UPA_F32
    L.check(L.lib().upa_linear_mixed(xd.data_ptr(), code(xb), m, k, ldx, pk.w.data_ptr(), pk.bias.data_ptr(), y.data_ptr(), code(yb), n, ldy,
                                     rd.data_ptr() if res else None, ldr if res else 0, act, L.current_stream(DEV)), "linear_mixed")
    torch.cuda.synchronize()
    got = y.float().cpu()
    scale = max(1.0, float(ref.abs().max()))
    tol = 2e-5 * scale + ((2.0 ** -8) * scale if yb else 0.0)
    assert float((got[:, :n].double() - ref).abs().max()) <= tol
    assert bool((got[:, n:] == -7.0).all())


def test_rtdetr_decoder_layer_perf_mode_close_to_exact():
    """One DeformableTransformerDecoderLayer at the model's width (d_model 256, 8 heads of 32, d_ffn 1024, 300 queries) with the perf-mode
    arithmetic of round 4 - nn.Linear products on the bf16 matrix cores (`upa_linear_mixed`), self-attention on the matrix-core kernel
    with bf16 q / k / v rows - against the same layer in exact float32 on the same inputs: the three post-LayerNorm outputs are O(1) and
    must agree to bf16-product accuracy (operands carry 8 bits; K = 256 / 1024 sums)."""
    from tests.hip_utils import DEV, unit_input
    from ultralytics_pro_amd.nn.modules import rtdetr as RT
    torch.manual_seed(0)
    layer = RT.DeformableTransformerDecoderLayer(256, 8, 1024, 0.0, torch.nn.ReLU(), 3, 4).eval()
    P.apply_procedural_weights(layer)
    layer = layer.to(DEV)
    bs, nq = 2, 300
    embed = unit_input("dl_embed", (bs * nq, 256), -1, 1).to(DEV)
    qpos = unit_input("dl_qpos", (bs * nq, 256), -1, 1).to(DEV)
    ref_b = unit_input("dl_ref", (bs * nq, 4), 0.1, 0.9).to(DEV)
    shapes = [[16, 16], [8, 8], [4, 4]]
    T = sum(h * w for h, w in shapes)
    feats = unit_input("dl_feats", (bs * T, 256), -1, 1).to(DEV)
    shp = torch.tensor([d for s_ in shapes for d in s_], dtype=torch.int32)
    outs = []
    for fast in (False, True):
        RT._LINEAR_BF16[0] = fast
        try:
            with torch.no_grad():
                outs.append(layer(embed, ref_b, feats, {"host_ptr": shp.data_ptr()}, bs, qpos, key=("t", fast)).clone())
        finally:
            RT._LINEAR_BF16[0] = False
    torch.cuda.synchronize()
    exact, perf = outs[0].cpu(), outs[1].cpu()
    assert torch.isfinite(perf).all() and float(exact.abs().max()) > 0.5
    d = (perf - exact).abs()
    print(f"decoder layer perf vs exact: max {float(d.max()):.4f} mean {float(d.mean()):.5f} (|exact| max {float(exact.abs().max()):.2f})")
    # measured on MI355X: max 0.0124, mean 0.0017 with |exact| up to 5.8
    assert float(d.max()) <= 0.03 and float(d.mean()) <= 0.004


def test_msdeform_attn_bf16_values_match_exact_path():
    """`upa_msdeform_attn_strided` on bf16 value rows (perf mode: the decoder's batched value projection; softmax on v_exp_f32 / v_rcp_f32,
    unconditional clamped corner fetches) vs the exact-f32 instantiation on the SAME bf16-rounded values (transformer.py:510-558): model
    shapes (3 levels 80/40/20, 8 heads of 32, 300 queries), offsets that throw a share of the sampling points outside the maps, a strided
    value matrix (one layer's columns of the six-layer projection)."""
    from tests.hip_utils import DEV, bf16_round, unit_input
    from ultralytics_pro_amd import _lib as L
    lib = L.lib()
    bs, nq, heads, d, npnt = 2, 300, 8, 32, 4
    shapes = [[80, 80], [40, 40], [20, 20]]
    T = sum(h * w for h, w in shapes)
    C = heads * d
    ldv = 3 * C
    vals = bf16_round(unit_input("msd16_v", (bs * T, ldv), -1, 1))
    off = unit_input("msd16_off", (bs * nq, heads * 3 * npnt * 2), -6, 6)
    lg = unit_input("msd16_lg", (bs * nq, heads * 3 * npnt), -3, 3)
    ref = torch.cat([unit_input("msd16_ref", (bs * nq, 2), 0.02, 0.98), unit_input("msd16_wh", (bs * nq, 2), 0.05, 0.6)], 1).contiguous()
    shp = torch.tensor([v for s_ in shapes for v in s_], dtype=torch.int32)
    st = L.current_stream(DEV)
    v32 = vals.to(DEV)
    v16 = vals.to(DEV).to(torch.bfloat16)
    offd, lgd, refd = off.to(DEV), lg.to(DEV), ref.to(DEV)
    y32 = torch.empty(bs * nq, C, device=DEV)
    y16 = torch.empty(bs * nq, C, device=DEV)
    col0 = C  # the middle layer's columns
    L.check(lib.upa_msdeform_attn_strided(v32.data_ptr() + col0 * 4, L.UPA_F32, ldv, shp.data_ptr(), 3, bs, heads, d, offd.data_ptr(),
                                          lgd.data_ptr(), refd.data_ptr(), nq, npnt, y32.data_ptr(), st), "msdeform f32")
    L.check(lib.upa_msdeform_attn_strided(v16.data_ptr() + col0 * 2, L.UPA_BF16, ldv, shp.data_ptr(), 3, bs, heads, d, offd.data_ptr(),
                                          lgd.data_ptr(), refd.data_ptr(), nq, npnt, y16.data_ptr(), st), "msdeform bf16")
    torch.cuda.synchronize()
    a, b = y32.cpu(), y16.cpu()
    assert float(a.abs().max()) > 0.05 and float((a == 0).float().mean()) < 0.5
    assert float((a - b).abs().max()) <= 2e-5  # same values, same weights up to v_exp_f32 / v_rcp_f32 (1 ulp) and the order of 48 f32 adds


@pytest.mark.parametrize("nc,shape,rows,keys_only", [(80, (2, 13, 21), 0, 0), (80, (3, 40, 40), 0, 0), (80, (2, 40, 40), 12, 0), (20, (1, 9, 16), 0, 0),
                                                      (80, (2, 23, 47), 8, 1), (80, (4, 80, 80), 0, 0), (80, (4, 80, 80), 40, 1),
                                                      (80, (1, 6, 61), 0, 1), (80, (2, 5, 30), 4, 0)],
                         ids=["13x21", "40x40", "40x40_parts12", "nc20_9x16", "23x47_parts8_keys", "80x80", "80x80_parts40_keys",
                              "6x61_one_column_strip_keys", "5x30_exact_strip_parts4"])
def test_detect_level_stream_vs_oracle(nc, shape, rows, keys_only):
    """`upa_detect_level_stream` (csrc/detect_stream.hip): one Detect level - conv3x3 -> conv3x3 -> 1x1 -> decode for BOTH branches - as one
    line-buffer launch (head.py:94-100, 116-126, 151-191), against the oracle's arithmetic on the same bf16-rounded input and weights with the
    kernel's rounding points (bf16 after each SiLU, f32 logits, f32 decode): boxes / scores of every anchor, the best-class NMS key of every
    anchor, nothing written outside the level.  Shapes: widths that are not a multiple of the 30-column strips, odd heights, parts of
    rows (`upa_opts.detect_stream_rows`), fewer classes than the class tail's 80 filters, the keys-only form (class rows not written)."""
    from tests.hip_utils import DEV, bf16_round, to_dev_nhwc, unit_input
    from ultralytics_pro_amd import _lib as L
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn.modules.conv import PackedConv
    import ctypes as C
    n, h, w = shape
    a0, extra = 19, 5
    a_total = a0 + h * w + extra
    y = torch.full((n, 4 + nc, a_total), -7.0, device=DEV)
    best_keys = torch.full((n, a_total), -1, dtype=torch.int64, device=DEV)
    x = bf16_round(unit_input(f"dls_x{nc}{h}", (n, 64, h, w), -1.5, 1.5))
    # the input as a channel slice of a wider buffer (ld = 96), as the neck hands it over
    wide = to_dev_nhwc(torch.cat([x, torch.zeros(n, 32, h, w)], 1), torch.bfloat16)
    xd = wide[:, :64]
    vx = R.view_of(xd)
    raws, branches, keep = [], [], []
    for kind, c, cout in ((1, 64, 64), (2, 80, nc)):
        w1 = bf16_round(unit_input(f"dls_w1{kind}{nc}", (c, 64, 3, 3), -0.1, 0.1))
        b1 = unit_input(f"dls_b1{kind}{nc}", (c,), -0.5, 0.5)
        w2 = bf16_round(unit_input(f"dls_w2{kind}{nc}", (c, c, 3, 3), -0.1, 0.1))
        b2 = unit_input(f"dls_b2{kind}{nc}", (c,), -0.5, 0.5)
        wt = bf16_round(unit_input(f"dls_wt{kind}{nc}", (cout, c, 1, 1), -0.4, 0.4))
        bt = unit_input(f"dls_bt{kind}{nc}", (cout,), -2, 1)
        t1 = bf16_round(torch.nn.functional.silu(torch.nn.functional.conv2d(x, w1, b1, padding=1)))
        t2 = bf16_round(torch.nn.functional.silu(torch.nn.functional.conv2d(t1, w2, b2, padding=1)))
        raws.append(torch.nn.functional.conv2d(t2, wt, bt))
        ct = 64 if kind == 1 else 80
        wtp = torch.cat([wt, torch.zeros(ct - cout, c, 1, 1)], 0)
        btp = torch.cat([bt, torch.zeros(ct - cout)], 0)
        pk1, pk2, pkt = (PackedConv(w1, b1, 3, DEV, torch.bfloat16, False), PackedConv(w2, b2, 3, DEV, torch.bfloat16, False),
                         PackedConv(wtp, btp, 1, DEV, torch.bfloat16, False))
        keep += [pk1, pk2, pkt]
        branches.append(L.DetectBranch(c, 0, pk1.w.data_ptr(), pk1.bias.data_ptr(), pk2.w.data_ptr(), pk2.bias.data_ptr(), pkt.w.data_ptr(),
                                       pkt.bias.data_ptr()))
    with R.use_opts(detect_stream=2, detect_stream_rows=rows, keys_only=keys_only):
        L.check(L.lib().upa_detect_level_stream(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, C.byref(branches[0]), C.byref(branches[1]), nc, 8.0,
                                                y.data_ptr(), a_total, a0, best_keys.data_ptr(), L.UPA_BF16, R.opts_ptr(),
                                                L.current_stream(DEV)), "detect_level_stream")
    torch.cuda.synchronize()
    oref = om.Detect(nc, (64,)).eval()
    oref.stride = torch.tensor([8.0])
    ref = oref._inference([torch.cat(raws, 1)])
    yc, keys = y.cpu(), best_keys.cpu()
    got = yc[:, :, a0:a0 + h * w]
    assert float(yc[:, :, :a0].min()) == -7.0 and float(yc[:, :, a0 + h * w:].max()) == -7.0  # nothing outside the level
    assert bool((keys[:, :a0] == -1).all()) and bool((keys[:, a0 + h * w:] == -1).all())
    db = (got[:, :4] - ref[:, :4]).abs()
    # f32 summation order differs from torch's: a bf16 rounding of an intermediate that falls the other way moves a logit by <= 2^-8 |h| |w|
    assert db.max().item() <= 0.5 and db.mean().item() <= 5e-3, (db.max().item(), db.mean().item())
    sc_ref = ref[:, 4:]
    kbits = keys[:, a0:a0 + h * w].numpy().view(np.uint64)
    kscore = torch.from_numpy((~(kbits >> np.uint64(32)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32))
    kidx = (kbits & np.uint64(0xFFFFFFFF)).astype(np.int64)
    anchors = np.arange(a0, a0 + h * w, dtype=np.int64)
    kcls = torch.from_numpy(kidx - anchors[None, :] * nc)
    assert bool(((kcls >= 0) & (kcls < nc)).all())
    if keys_only:
        assert float(got[:, 4:].min()) == -7.0 and float(got[:, 4:].max()) == -7.0   # class rows untouched
        best_ref = sc_ref.max(1).values
        assert (kscore - best_ref).abs().max().item() <= 1e-2
        # the key's class is the reference's best class wherever the reference's margin is beyond the intermediates' bf16 noise
        top2 = sc_ref.topk(2, dim=1).values
        clear = (top2[:, 0] - top2[:, 1]) > 2e-2
        assert bool((kcls == sc_ref.argmax(1))[clear].all()) and clear.float().mean().item() > 0.2
    else:
        ds_ = (got[:, 4:] - sc_ref).abs()
        assert ds_.max().item() <= 1e-2 and ds_.mean().item() <= 2e-4, (ds_.max().item(), ds_.mean().item())
        # the keys are exactly the first maxima of the scores the kernel itself wrote (utils/nms key order, nms.py:109)
        best, arg = got[:, 4:].max(1)
        assert torch.equal(kscore, best) and torch.equal(kcls, arg)
