"""CPU tests of tests/mask_ref.py, the float64 reference tests/test_hip_mask_kernels.py holds `upa_process_mask` and
`upa_resize_bilinear` to: it agrees with the f32 torch chain of tests/segment_oracle.py inside its own bound at every pixel, its case
table reaches every tile form, the row loop's second trip and both store paths, almost every pixel of every case is decided, and six
plausible mistakes each flip a decided pixel."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mask_ref as R
from tests import segment_oracle as S
from ultralytics_pro_amd.utils.ops import scale_masks_window

CASES = R.mask_kernel_cases()
RUN = [c for c in CASES if not getattr(c, "refused", False)]
UNDECIDED_CAP = 1e-3  # of the inside pixels of a case; none in a case with fewer than 1000


def _form(c):
    top, left, bottom, right = c.window
    return R.tile_form((bottom - top, right - left), c.out_hw)


def _torch_chain(case, inp):
    """(values (R, H, W) f32, crop factor bool) of the f32 torch chain, image by image: process_mask_values /
    process_mask_native_values where the case is one of theirs, else the same pieces (mask_logits, crop_mask 'compare',
    F.interpolate) on the sliced window."""
    mh, mw = case.mhw
    top, left, bottom, right = case.window
    vals, crops = [], []
    for i, n in enumerate(case.counts):
        if n == 0:
            continue
        p = inp.protos[i].permute(2, 0, 1).contiguous()
        coef, boxes = inp.coef[i, :n], inp.boxes[i, :n]
        if case.mode == 0:
            ratios = torch.tensor([[case.ratio[0], case.ratio[1], case.ratio[0], case.ratio[1]]])
            crops.append(S.crop_mask(torch.ones(n, mh, mw), boxes * ratios, "compare")[:, top:bottom, left:right] > 0)
            if case.window == (0, 0, mh, mw) and case.ratio == (mw / case.shape[1], mh / case.shape[0]):
                v = S.process_mask_values(p, coef, boxes, case.shape, upsample=case.out_hw != case.mhw, branch="compare")
            else:  # a window offset: the proto map cropped, sliced, resampled
                m = S.crop_mask(S.mask_logits(p, coef), boxes * ratios, "compare")[:, top:bottom, left:right]
                v = F.interpolate(m[None], case.out_hw, mode="bilinear")[0]
        else:
            crops.append(S.crop_mask(torch.ones(n, *case.out_hw), boxes, "compare") > 0)
            if case.window == scale_masks_window(mh, mw, case.out_hw):
                v = S.process_mask_native_values(p, coef, boxes, case.out_hw, branch="compare")
            else:
                m = F.interpolate(S.mask_logits(p, coef)[None, :, top:bottom, left:right], case.out_hw, mode="bilinear")[0]
                v = S.crop_mask(m, boxes, "compare")
        assert v.dtype == torch.float32
        vals.append(v)
    return torch.cat(vals).numpy(), torch.cat(crops).numpy()


@pytest.mark.parametrize("case", RUN, ids=lambda c: c.name)
def test_reference_holds_the_f32_torch_chain_inside_its_bound(case):
    inp, ref = R.case_reference(case, "f32")
    v32, crop = _torch_chain(case, inp)
    if case.mode == 0:
        assert np.array_equal(ref.inside_proto, crop), "the crop decision differs from crop_mask's"
        want = ref.v
    else:
        assert np.array_equal(ref.inside, crop), "the crop decision differs from crop_mask's"
        want = np.where(ref.inside, ref.v, 0.0)  # the chain multiplies by the crop factor last
    err = np.abs(v32.astype(np.float64) - want)
    bad = err > ref.bound
    assert not bad.any(), f"{int(bad.sum())} pixels of the torch chain outside the bound (worst {float((err / np.maximum(ref.bound, 1e-300))[bad].max()):.2f})"
    assert (ref.bound[(np.abs(ref.v) > 0)] > 0).all()


def test_case_table_reaches_every_path():
    forms = [_form(c) for c in CASES]
    for cand in R.CANDIDATES:
        assert cand in forms, f"no case launches the {cand} tile form"
    assert forms.count(None) == 1 and [getattr(c, "refused", False) for c in CASES].count(True) == 1
    assert all((f is None) == getattr(c, "refused", False) for c, f in zip(CASES, forms))
    assert any(sum(c.counts) > 1024 and min(c.capacities) > 1024 and min(c.capacities) < sum(c.counts) for c in RUN), "row loop: one trip only"
    assert any(c.b == R.PM_B and c.counts.count(0) > c.b // 2 for c in RUN)
    assert any(c.out_hw[1] % 2 == 1 and c.out_hw[1] > 16 and c.out_hw[0] > 1 for c in RUN), "no odd W with a 16-byte store"
    assert any(c.out_hw[1] < 16 for c in RUN) and any(c.out_hw[0] == 1 for c in RUN)
    assert {c.nm for c in RUN} >= {4, 8, 32, 36, 64, R.PM_NM}
    assert any(c.mode == 0 and c.window[0] > 0 and c.window[1] > 0 for c in RUN)
    assert any(c.mode == 1 and c.window[0] > 0 and c.window[2] < c.mhw[0] for c in RUN)


def test_tile_form_restates_the_examples_worked_by_hand():
    """{32, 128} wherever the output is no smaller than the window (34 x 130 taps at most).  160 x 160 -> 40 x 40 (s = 4 d + 1.5):
    t output rows read proto rows 4 y0 + 1 ... 4 (y0 + t - 1) + 2, 4 t - 2 of them, and the 40 columns read 158; 126 x 158 and 62 x 158
    exceed 8192, 30 x 158 fits.  One output row of a 512 x 512 -> 16 x 16 reads 2 rows x 482 columns."""
    assert R.tile_form((20, 28), (20, 28)) == (32, 128) and R.tile_form((160, 160), (640, 640)) == (32, 128)
    assert R.tile_form((160, 160), (40, 40)) == (8, 64)
    assert R.tile_form((512, 512), (16, 16)) == (1, 16)
    assert R.pm_max_window(R.scale32(160, 40), R.scale32(160, 40), 160, 160, 40, 40, 8, 64) == 30 * 158
    assert R.pm_max_window(R.scale32(160, 40), R.scale32(160, 40), 160, 160, 40, 40, 16, 64) == 62 * 158
    assert R.pm_max_window(R.scale32(512, 16), R.scale32(512, 16), 512, 512, 16, 16, 1, 16) == 2 * 482


@pytest.mark.parametrize("case", RUN, ids=lambda c: c.name)
def test_almost_every_pixel_is_decided(case):
    for dtype in case.dtypes:
        inp, ref = R.case_reference(case, dtype)
        inside = int(ref.inside.sum())
        undecided = int((ref.inside & ~ref.decided).sum())
        assert inside > 0 and ref.bit.any() and not ref.bit.all()
        assert undecided <= (UNDECIDED_CAP * inside if inside >= 1000 else 0), f"{case.name} {dtype}: {undecided} of {inside} inside pixels undecided"
        zero_rows = [r for r in range(len(inp.img)) if not inp.row_coef[r].any()]
        assert all((ref.bound[r] == 0).all() and not ref.bit[r].any() for r in zero_rows)


def _emulated(case, dtype, variant):
    inp, ref = R.case_reference(case, dtype)
    bits = R.emulate(inp.protos.numpy(), inp.row_coef, inp.row_boxes, case.out_hw, case.mode, case.ratio, case.window, inp.img,
                     vec=4 if dtype == "f32" else 8, variant=variant)
    return int(((bits != ref.bit) & ref.decided).sum())


def test_the_kernel_arithmetic_in_f32_flips_no_decided_pixel():
    for case in RUN:
        for dtype in case.dtypes:
            assert _emulated(case, dtype, None) == 0, (case.name, dtype)


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_negative_control_flips_a_decided_pixel(variant):
    flipped = {c.name: _emulated(c, c.dtypes[-1], variant) for c in RUN}
    print(variant, {k: v for k, v in flipped.items() if v})
    assert any(flipped.values()), f"no case notices `{variant}`"


@pytest.mark.parametrize("case", R.resize_cases(), ids=lambda c: c[0])
def test_resize_reference_holds_f_interpolate_inside_its_bound(case):
    name, planes, hw, window, out_hw = case
    x = R.resize_input(name, planes, hw)
    v, bound = R.resize_reference(x.numpy(), window, out_hw)
    top, left, bottom, right = window
    y = F.interpolate(x[None, :, top:bottom, left:right], out_hw, mode="bilinear")[0]
    err = (y.double() - v).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    # inputs in (-1, 1): slopes below 2 and 2 u (s + 1) an axis, s < max(hw), and gamma_7 for the blend
    assert float(bound.max()) <= 8 * R.U * (max(hw) + 1) + 8 * R.U
    if max(bottom - top, right - left) == 1:
        assert bool((bound <= R.gamma(R.BLEND_ROUNDINGS)).all()) and torch.equal(v, x[:, top:top + 1, left:left + 1].double().expand_as(v))
