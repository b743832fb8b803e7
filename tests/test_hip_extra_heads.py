"""-m gpu: the part Segment and Pose share (`ExtraDetect`: Detect plus one per-anchor cv4 branch) on the small heads of the head tests -
ch (16, 32, 64), batch 2, maps 6 x 7, 3 x 4, 2 x 2 (58 anchors).  The three ways a forward can be scheduled give the same bits and leave
no plan behind; the parts travel with the first output whether or not it is the concatenated tensor."""

import functools

import pytest
import torch

from tests import kernel_check as KC
from tests import pose_cases as GP
from ultralytics_pro_amd.utils import procedural as P

pytestmark = pytest.mark.gpu
KINDS = ["segment", "pose"]


@functools.lru_cache(maxsize=None)
def _head(kind):
    from tests.hip_utils import DEV, bn_fix
    from ultralytics_pro_amd.nn.modules.head import Pose, Segment
    cls = Segment if kind == "segment" else Pose
    old = cls.legacy
    cls.legacy = True  # the yolov8 class branch, as parse_model sets it for a yolov8 model
    try:
        h = bn_fix(Segment(3, 32, 64, GP.HEAD_CH) if kind == "segment" else Pose(1, (17, 3), GP.HEAD_CH))
    finally:
        cls.legacy = old
    h.stride = torch.tensor([8.0, 16.0, 32.0])
    h.bias_init()
    P.apply_procedural_weights(h, family="yolov8n-seg" if kind == "segment" else "yolov8n-pose")
    return h.to(DEV).eval()


def _inputs(dtype):
    from tests.hip_utils import DEV
    from ultralytics_pro_amd.engine import runtime as R
    return [R.to_nhwc(P.uniform(f"unit:extra:{i}", (2, c, *hw), -1.0, 1.0).to(DEV).contiguous(), dtype)
            for i, (c, hw) in enumerate(zip(GP.HEAD_CH, GP.HEAD_MAPS))]


def _outputs(kind, res):
    """Clones of (first output, extra tensor, kpt | protos, the parts) of one eval forward: the buffers are pooled."""
    out, rest = res
    y, extra = out._upa_parts
    third = rest[2] if kind == "segment" else rest[1]
    assert kind != "segment" or rest[1] is extra
    return [t.clone() for t in (out, extra, third, y)]


@KC.stop_after_fault
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", KINDS)
def test_three_schedules_give_the_same_bits(kind, dtype):
    """(a) a direct call; (b) begin with the true level sizes, every level started in order, forward; (c) begin with level sizes that
    do not match the inputs (each h doubled), forward.  Every output agrees in every bit and no per-tag plan survives a forward."""
    from tests.hip_utils import DEV
    h, xs = _head(kind), _inputs(dtype)
    hw = [tuple(int(v) for v in t.shape[2:]) for t in xs]

    def started(level_hw, start):
        h.begin(2, level_hw, dtype, DEV)
        for i in (range(h.nl) if start else ()):
            h.start_level(i, xs[i])
        return h(xs)

    runs = []
    with torch.no_grad():
        for run in (lambda: h(xs), lambda: started(hw, True), lambda: started([(2 * a, b) for a, b in hw], False)):
            runs.append(_outputs(kind, run()))
            assert h._plan() == {} and h._extra_plans() == {} and h._pend() == {}, "a plan outlived its forward"
    torch.cuda.synchronize()
    a = sum(p * q for p, q in hw)
    assert runs[0][0].shape == (2, runs[0][3].shape[1] + runs[0][1].shape[1], a) and runs[0][1].shape[2] == a
    for name, other in zip("bc", runs[1:]):
        for what, t0, t1 in zip(("first output", "extra", "kpt / protos", "y"), runs[0], other):
            assert KC.same_bits(t0, t1), f"{kind}: schedule ({name}) differs from the direct call in {what}"


@KC.stop_after_fault
@pytest.mark.parametrize("cat_out", [True, False], ids=["cat", "y"])
@pytest.mark.parametrize("kind", KINDS)
def test_parts_travel_with_the_first_output(kind, cat_out):
    """The first output carries `_upa_parts = (y, extra)` in both settings: with cat_out it equals cat([y, extra], 1), without it is y
    itself; the postprocess returns the same rows and counts from either."""
    from ultralytics_pro_amd.utils.ops import pose_postprocess_raw, segment_postprocess_raw
    h, xs = _head(kind), _inputs(torch.float32)

    def post(res):
        if kind == "segment":
            r = segment_postprocess_raw(res, 0.0, 0.7, max_det=20, capacity=64)
            return r["rows"].clone(), r["counts"].clone()
        rows, counts, _ = pose_postprocess_raw(res, 0.0, 0.7, max_det=20)
        return rows.clone(), counts.clone()

    got = {}
    try:
        with torch.no_grad():
            for setting in (cat_out, not cat_out):
                h.cat_out = setting
                res = h(xs)
                if setting == cat_out:
                    out = res[0]
                    y, extra = out._upa_parts
                    if cat_out:
                        assert out is not y and torch.equal(out, torch.cat([y, extra], 1))
                    else:
                        assert out is y
                    assert y.shape[1] == 4 + h.nc and extra.shape[1] == (h.nm if kind == "segment" else h.nk)
                got[setting] = post(res)
    finally:
        h.cat_out = True
    torch.cuda.synchronize()
    assert int(got[True][1].sum()) > 0
    assert torch.equal(got[True][0], got[False][0]) and torch.equal(got[True][1], got[False][1])
