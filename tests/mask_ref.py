"""CHECKER for the mask assembly kernels of csrc/segment.hip (`upa_process_mask`, `upa_resize_bilinear`): a float64 reference with a
per-pixel error bound derived from the operands, the kernel's tile selection restated, an f32 emulation with switchable mistakes
(the negative controls of tests/test_mask_ref.py) and the case table of tests/test_hip_mask_kernels.py.  Plain numpy / torch on the
CPU; line numbers are those of ultralytics_pro_amd/csrc/segment.hip unless another file is named.

What a mask pixel is (segment.hip:161-253, mask_dot.h):
  D(py, px)  = sum_k coef_k * proto_k(py, px), an nm-deep fma chain in f32 (mask_dot.h:9-30); mode 0 replaces it by exactly 0 where
               the proto pixel fails crop_mask's comparisons on the f32 products box * ratio (:204, :211, mask_dot.h:33-35);
  v(y, x)    = the bilinear blend of four D taps with torch's upsample_bilinear2d rule (bil_idx, :152-159; :237);
  bit        = in(y, x) & (v > 0), `in` being the mode-1 comparisons of (float(x), float(y)) with the raw box (:228, :239) and
               true in mode 0.
The reference takes D and v in float64 from the same f32 scale; `bound` says how far an f32 evaluation may be from that v."""

import functools
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24  # unit roundoff of f32
PM_LDS, PM_NM, PM_B = 8192, 128, 1024  # :125-127
CANDIDATES = ((32, 128), (16, 128), (16, 64), (8, 64), (8, 32), (4, 32), (4, 16), (2, 16), (1, 16))  # :443


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): n roundings compounded."""
    return n * U / (1.0 - n * U)


# Part 3 of the bound: the roundings of the blend itself.  With the kernel's own source coordinate, l1 = s - i0 is exact (the
# fraction of an f32 is an f32) and l0 = fl(1 - l1) carries one rounding (:224, :236).  In
#     v = ly0 * (lx0 * a + lx1 * b) + ly1 * (lx0 * c + lx1 * d)                                                        (:237)
# a tap is multiplied by a rounded lx0 (1), by a rounded ly0 (1), and passes two multiply-adds, each of which is either a rounded
# product and a rounded sum or one fma behind a rounded product: at most 2 roundings a level.  1 + 1 + 2 + 2 = 6 factors (1 + d)
# on any tap, so |fl(v) - v| <= gamma_6 * sum_taps w |D|.  One more is allowed for the second-order terms (the weights the kernel
# rounds are its own, not the reference's: they differ by the coordinate error of part 2, times gamma_6): BLEND_ROUNDINGS = 7.
BLEND_ROUNDINGS = 7


# ---- the source index ---------------------------------------------------------------------------------------------------------------
def bil_idx32(scale32, d, n):
    """bil_idx (:152-159) in f32, a rounded product and a rounded difference (what the host compiles to): (i0, i1, l1) arrays."""
    d = np.asarray(d)
    s = (np.float32(scale32) * (d.astype(np.float32) + np.float32(0.5))).astype(np.float32) - np.float32(0.5)
    s = np.maximum(s, np.float32(0.0)).astype(np.float32)
    i0 = np.minimum(s.astype(np.int64), n - 1)
    i1 = i0 + (i0 < n - 1)
    l1 = np.clip(s - i0.astype(np.float32), np.float32(0), np.float32(1)).astype(np.float32)
    return i0, i1, l1


def scale32(win_n, out_n):
    """torch's area_pixel_compute_scale for float and :440: the f32 quotient."""
    return np.float32(win_n) / np.float32(out_n)


def pm_max_window(sy, sx, wh, ww, H, W, th, tw):
    """pm_max_window (:256-271)."""
    def axis(scale, n, out, t):
        starts = np.arange(0, out, t)
        a = bil_idx32(scale, starts, n)[0]
        b = bil_idx32(scale, np.minimum(starts + t, out) - 1, n)[1]
        return int((b - a + 1).max())
    return axis(sy, wh, H, th) * axis(sx, ww, W, tw)


def tile_form(window_hw, out_hw):
    """The (th, tw) `upa_process_mask` launches with (:443-450), or None where it refuses (:451-454)."""
    wh, ww = window_hw
    H, W = out_hw
    for th, tw in CANDIDATES:
        if pm_max_window(scale32(wh, H), scale32(ww, W), wh, ww, H, W, th, tw) <= PM_LDS:
            return th, tw
    return None


def _axis(win_n, out_n):
    """The reference's source coordinates of one axis, in float64 from the f32 scale, with the reach of an f32 evaluation.
    e: |s_f32 - s| <= u |p| + u |s| <= 2 u (s + 1) for p = scale (d + 0.5) (a rounded product and a rounded difference, or one
    fma: a single rounding of s); 0 where p is an f32 (then p - 0.5 is too: a multiple of ulp(p) <= 0.5 no larger than p), as at
    every integer ratio.  (alt0, alt1): the other segment an evaluation within e of an integer s may pick, else (i0, i1)."""
    sc = float(scale32(win_n, out_n))
    p = sc * (np.arange(out_n, dtype=np.float64) + 0.5)
    s = np.maximum(p - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), win_n - 1)
    i1 = i0 + (i0 < win_n - 1)
    l1 = np.clip(s - i0, 0.0, 1.0)
    e = np.where(p.astype(np.float32).astype(np.float64) == p, 0.0, 2.0 * U * (s + 1.0))
    lo = np.floor(np.maximum(s - e, 0.0)).astype(np.int64)
    hi = np.minimum(np.floor(s + e).astype(np.int64), win_n - 1)
    alt0 = np.where(lo < i0, lo, np.where(hi > i0, hi, i0))
    alt1 = alt0 + (alt0 < win_n - 1)
    return SimpleNamespace(s=s, i0=i0, i1=i1, l1=l1, e=e, alt0=alt0, alt1=alt1)


def _blend(M, ay, ax):
    """(R, wh, ww) -> (R, H, W): the bilinear blend with the reference's weights."""
    wx = ax.l1[None, None, :]
    wy = ay.l1[None, :, None]
    r0, r1 = M[:, ay.i0], M[:, ay.i1]
    top = r0[:, :, ax.i0] * (1.0 - wx) + r0[:, :, ax.i1] * wx
    bot = r1[:, :, ax.i0] * (1.0 - wx) + r1[:, :, ax.i1] * wx
    return top * (1.0 - wy) + bot * wy


def _interp(D, ay, ax):
    """D (R, wh, ww) float64 tap values -> (v, parts 2 and 3 of the bound, the coordinate reaches)."""
    v = _blend(D, ay, ax)
    wabs = _blend(np.abs(D), ay, ax)
    wx = ax.l1[None, None, :]
    wy = ay.l1[None, :, None]

    def xrow(k):  # row k of the window, blended along x
        r = D[:, k]
        return r[:, :, ax.i0] * (1.0 - wx) + r[:, :, ax.i1] * wx

    def ycol(k):  # column k, blended along y
        return D[:, ay.i0][:, :, k] * (1.0 - wy) + D[:, ay.i1][:, :, k] * wy

    # part 2: v is piecewise linear and continuous in each source coordinate; its slope on a segment is the difference of the
    # two blended rows (columns), and an evaluation within e of an integer may sit on the neighbouring segment
    slope_y = np.maximum(np.abs(xrow(ay.i1) - xrow(ay.i0)), np.abs(xrow(ay.alt1) - xrow(ay.alt0)))
    slope_x = np.maximum(np.abs(ycol(ax.i1) - ycol(ax.i0)), np.abs(ycol(ax.alt1) - ycol(ax.alt0)))
    ey, ex = ay.e[None, :, None], ax.e[None, None, :]
    bound = ey * slope_y + ex * slope_x + gamma(BLEND_ROUNDINGS) * wabs
    return v, bound, (ey, ex)


def resize_reference(x, window, out_hw):
    """`upa_resize_bilinear` (:288-305): x (planes, h, w) -> (v, bound) float64 (planes, H, W); parts 2 and 3 of the bound only."""
    top, left, bottom, right = window
    D = np.asarray(x, dtype=np.float64)[:, top:bottom, left:right]
    v, bound, _ = _interp(D, _axis(bottom - top, out_hw[0]), _axis(right - left, out_hw[1]))
    return torch.from_numpy(v), torch.from_numpy(bound)


def crop_products(boxes, ratio):
    """:204: float32(box) * float32(ratio), one f32 product each; ratio = (cx, cy)."""
    b = np.asarray(boxes, dtype=np.float32)
    r = np.array([ratio[0], ratio[1], ratio[0], ratio[1]], dtype=np.float32)
    return (b * r[None]).astype(np.float32)


def in_box(fx, fy, c):
    """mask_in_crop (mask_dot.h:33-35) / :228, :239 on f32 operands: fx (n,), fy (m,), c (R, 4) -> (R, m, n)."""
    fx = np.asarray(fx, dtype=np.float32)[None, None, :]
    fy = np.asarray(fy, dtype=np.float32)[None, :, None]
    x1, y1, x2, y2 = (c[:, k].astype(np.float32)[:, None, None] for k in range(4))
    return (fx >= x1) & (fx < x2) & (fy >= y1) & (fy < y2)


def tap_sums(protos, coef, img, window):
    """(D, A) float64 (R, wh, ww): the dot products of the window's proto pixels and their absolute term sums.
    protos (b, mh, mw, nm), coef (R, nm), img (R,) the image of each row."""
    top, left, bottom, right = window
    P = np.asarray(protos, dtype=np.float64)[:, top:bottom, left:right]
    C = np.asarray(coef, dtype=np.float64)
    R = C.shape[0]
    D = np.zeros((R, bottom - top, right - left))
    A = np.zeros_like(D)
    for i in np.unique(img):
        sel = np.nonzero(img == i)[0]
        D[sel] = np.einsum("rk,yxk->ryx", C[sel], P[i])
        A[sel] = np.einsum("rk,yxk->ryx", np.abs(C[sel]), np.abs(P[i]))
    return D, A


def mask_reference(protos, coef, boxes, out_hw, mode, crop_ratio, window, img=None):
    """protos (b, mh, mw, nm) values the storage type holds, coef (R, nm), boxes (R, 4), img (R,) (default: image 0) ->
    inside (R, H, W) bool, inside_proto (R, wh, ww) bool (mode 0; the window's proto pixels), v, bound float64, decided, bit."""
    protos = np.asarray(protos)
    if protos.ndim == 3:
        protos = protos[None]
    coef = np.asarray(coef, dtype=np.float32)
    boxes = np.asarray(boxes, dtype=np.float32)
    R, nm = coef.shape
    img = np.zeros(R, np.int64) if img is None else np.asarray(img)
    top, left, bottom, right = window
    wh, ww = bottom - top, right - left
    H, W = out_hw
    D, A = tap_sums(protos, coef, img, window)
    ay, ax = _axis(wh, H), _axis(ww, W)
    inside_proto = None
    if mode == 0:
        inside_proto = in_box(np.arange(left, right), np.arange(top, bottom), crop_products(boxes, crop_ratio))
        D = np.where(inside_proto, D, 0.0)
        A = np.where(inside_proto, A, 0.0)
        # an output pixel is inside where any tap an f32 evaluation can reach is
        rows = inside_proto[:, ay.i0] | inside_proto[:, ay.i1] | inside_proto[:, ay.alt0] | inside_proto[:, ay.alt1]
        inside = rows[:, :, ax.i0] | rows[:, :, ax.i1] | rows[:, :, ax.alt0] | rows[:, :, ax.alt1]
    else:
        inside = in_box(np.arange(W), np.arange(H), boxes)
    v, bound, (ey, ex) = _interp(D, ay, ax)
    # part 1: each tap's chain is off by at most gamma_nm * sum_k |coef_k proto_k| in any order (fma: one rounding a term), and the
    # taps enter with their weights, times (1 + gamma_7) for the blend's roundings of that error.  The slopes of part 2 are those of
    # the ROUNDED taps: two taps a slope, each off by no more than the row's largest term sum
    amax = A.reshape(R, -1).max(1)[:, None, None]
    bound = bound + gamma(nm) * ((1.0 + gamma(BLEND_ROUNDINGS)) * _blend(A, ay, ax) + 2.0 * (ey + ex) * amax)
    decided = ~inside | (bound == 0) | (np.abs(v) > bound)
    return SimpleNamespace(inside=inside, inside_proto=inside_proto, v=v, bound=bound, decided=decided, bit=inside & (v > 0))


# ---- the kernel in f32, with switchable mistakes ------------------------------------------------------------------------------------
VARIANTS = ("le_x2", "align_corners", "drop_group", "no_left", "i1_unclamped", "mode1_at_proto")


def emulate(protos, coef, boxes, out_hw, mode, crop_ratio, window, img=None, vec=4, variant=None):
    """The bits an f32 evaluation of :161-253 gives (dot products rounded once from float64, which is inside part 1), or with one
    of VARIANTS: `< x2` as `<= x2`; align_corners = True coordinates; the last 16-byte channel group (`vec` channels) left out;
    the window's `left` ignored; i1 = i0 + 1 past the window's last row and column; the mode-1 crop applied to the proto pixels."""
    assert variant is None or variant in VARIANTS
    protos = np.asarray(protos)
    if protos.ndim == 3:
        protos = protos[None]
    coef = np.asarray(coef, dtype=np.float32)
    boxes = np.asarray(boxes, dtype=np.float32)
    b, mh, mw, nm = protos.shape
    R = coef.shape[0]
    img = np.zeros(R, np.int64) if img is None else np.asarray(img)
    top, left, bottom, right = window
    wh, ww = bottom - top, right - left
    H, W = out_hw
    k = nm - vec if variant == "drop_group" else nm
    D = tap_sums(protos[..., :k], coef[:, :k], img, (0, 0, mh, mw))[0].astype(np.float32)

    def box_test(fx, fy, c):
        if variant != "le_x2":
            return in_box(fx, fy, c)
        fx = np.asarray(fx, dtype=np.float32)[None, None, :]
        fy = np.asarray(fy, dtype=np.float32)[None, :, None]
        x1, y1, x2, y2 = (c[:, j][:, None, None] for j in range(4))
        return (fx >= x1) & (fx <= x2) & (fy >= y1) & (fy < y2)

    if mode == 0:
        D = np.where(box_test(np.arange(mw), np.arange(mh), crop_products(boxes, crop_ratio)), D, np.float32(0))
    elif variant == "mode1_at_proto":
        c = crop_products(boxes, (float(scale32(ww, W)), float(scale32(wh, H))))
        D = np.where(box_test(np.arange(mw) - left, np.arange(mh) - top, c), D, np.float32(0))

    def idx(n, out):
        d = np.arange(out)
        if variant == "align_corners":
            sc = np.float32(n - 1) / np.float32(out - 1) if out > 1 else np.float32(0)
            s = (sc * d.astype(np.float32)).astype(np.float32)
            i0 = np.minimum(s.astype(np.int64), n - 1)
            i1, l1 = i0 + (i0 < n - 1), (s - i0.astype(np.float32)).astype(np.float32)
        else:
            i0, i1, l1 = bil_idx32(scale32(n, out), d, n)
        if variant == "i1_unclamped":
            i1 = i0 + 1
        return i0, i1, l1

    (i0, i1, ly1), (j0, j1, lx1) = idx(wh, H), idx(ww, W)
    x_off = 0 if variant == "no_left" else left
    y0, y1 = np.minimum(top + i0, mh - 1), np.minimum(top + i1, mh - 1)
    x0, x1 = np.minimum(x_off + j0, mw - 1), np.minimum(x_off + j1, mw - 1)
    ly1, lx1 = ly1[None, :, None], lx1[None, None, :]
    ly0, lx0 = np.float32(1) - ly1, np.float32(1) - lx1
    r0, r1 = D[:, y0], D[:, y1]
    v = ly0 * (lx0 * r0[:, :, x0] + lx1 * r0[:, :, x1]) + ly1 * (lx0 * r1[:, :, x0] + lx1 * r1[:, :, x1])
    assert v.dtype == np.float32
    bits = v > 0
    if mode == 1 and variant != "mode1_at_proto":
        bits &= box_test(np.arange(W), np.arange(H), boxes)
    return bits


# ---- the case table -----------------------------------------------------------------------------------------------------------------
def _case(name, mhw, out_hw, mode, nm=8, b=1, max_det=12, counts=None, window=None, ratio=None, shape=None, capacities=None, key=None):
    """mode 0: `shape` is the image the boxes live in (default: the output), ratio = proto / shape as process_mask takes it
    (ops.py:527); mode 1: the boxes live in the output, the window is scale_masks' (default) or given."""
    from ultralytics_pro_amd.utils.ops import scale_masks_window
    mh, mw = mhw
    counts = list(counts) if counts is not None else [max_det] * b
    if mode == 0:
        shape = tuple(shape or out_hw)
        ratio = ratio or (mw / shape[1], mh / shape[0])
        window = window or (0, 0, mh, mw)
    else:
        shape, ratio = tuple(out_hw), (1.0, 1.0)
        window = window or scale_masks_window(mh, mw, out_hw)
    total = sum(counts)
    return SimpleNamespace(name=name, key=key or f"maskk:{name}", mhw=tuple(mhw), out_hw=tuple(out_hw), mode=mode, nm=nm, b=b,
                           max_det=max_det, counts=counts, window=tuple(window), ratio=ratio, shape=shape,
                           capacities=list(capacities or [total]), dtypes=("f32",) if nm % 8 else ("f32", "bf16"))


def mask_kernel_cases():
    """The cases of test_hip_mask_kernels.py::test_process_mask, the smallest shapes that reach each path (test_mask_ref.py asserts
    that they do).  `refused` (no tile form fits) belongs to the refusal test and carries no inputs."""
    c = [
        # the product's forms
        _case("proto_20x28", (20, 28), (20, 28), 0, nm=32, shape=(80, 112)),
        _case("up4_12x20", (12, 20), (48, 80), 0, nm=32),
        _case("native_32x40", (32, 40), (90, 150), 1, nm=32),  # scale_masks' window: top = 4, bottom = 28
        # the tile forms behind {32, 128}: outputs smaller than the window
        _case("form_16x128", (40, 208), (24, 72), 1, max_det=8, window=(0, 0, 40, 208)),
        _case("form_16x64", (40, 208), (16, 72), 0, max_det=8),
        _case("form_8x64", (24, 352), (16, 32), 1, max_det=8, window=(0, 0, 24, 352)),
        _case("form_8x32", (24, 368), (8, 40), 0, max_det=8),
        _case("form_4x32", (24, 368), (8, 32), 1, max_det=8, window=(0, 0, 24, 368)),
        _case("form_4x16", (56, 368), (8, 32), 0, max_det=8),
        _case("form_2x16", (48, 448), (8, 16), 1, max_det=8, window=(0, 0, 48, 448)),
        _case("form_1x16", (152, 416), (8, 16), 0, max_det=8),
        # depth
        _case("nm4", (8, 8), (16, 16), 0, nm=4),
        _case("nm36", (8, 8), (16, 16), 1, nm=36),
        _case("nm8", (8, 8), (16, 16), 0, nm=8),
        _case("nm64", (8, 8), (16, 16), 1, nm=64),
        _case("nm128", (8, 8), (16, 16), 0, nm=128),
        # stores: W < 16, H = 1, odd W (rows alternate between the 16-byte store and the byte loop)
        _case("out_5x7", (8, 8), (5, 7), 1, window=(0, 0, 8, 8)),
        _case("out_1x40", (4, 20), (1, 40), 0),
        _case("out_9x33", (6, 12), (9, 33), 1, window=(0, 0, 6, 12)),
        # the row loop's second trip, the capacity cut inside it
        _case("rows_1150", (8, 8), (8, 8), 0, b=5, max_det=300, counts=(300, 0, 300, 300, 250), shape=(32, 32), capacities=(1150, 1030)),
        # the image lookup at its limit
        _case("images_1024", (2, 2), (4, 4), 0, b=1024, max_det=2, counts=[2] + [2 if i % 97 == 5 else 1 if i % 41 == 7 else 0 for i in range(1, 1023)] + [1]),
        # mode 0 from a window that does not start at (0, 0)
        _case("mode0_window", (16, 20), (24, 28), 0, window=(2, 3, 14, 17), ratio=(0.25, 0.25), shape=(64, 80)),
    ]
    # no form fits: one output row reads two proto rows, and 16 output columns span more than PM_LDS / 2 proto columns
    c.append(SimpleNamespace(name="refused", mhw=(2, 4608), out_hw=(1, 16), window=(0, 0, 2, 4608), nm=8, refused=True))
    return c


def resize_cases():
    """(name, planes, (h, w), window, (oh, ow)) of `upa_resize_bilinear`: up, down, a window with offsets on all four sides, a
    1 x 1 window, a 1 x 1 output, and one past the 8192-workgroup cap (9 * 512 * 512 > 8192 * 256)."""
    return [("up", 3, (10, 12), (0, 0, 10, 12), (23, 31)), ("down", 3, (40, 48), (0, 0, 40, 48), (7, 9)),
            ("offsets", 2, (20, 24), (3, 5, 17, 20), (30, 28)), ("window_1x1", 2, (6, 6), (2, 3, 3, 4), (5, 4)),
            ("out_1x1", 2, (6, 7), (1, 1, 5, 6), (1, 1)), ("grid_cap", 9, (8, 8), (0, 0, 8, 8), (512, 512))]


def resize_input(name, planes, hw):
    from ultralytics_pro_amd.utils import procedural as P
    return P.uniform(f"maskk:resize:{name}", (planes, *hw), -1.0, 1.0)


def case_inputs(case, dtype="f32"):
    """protos (b, mh, mw, nm) float32 holding values of the storage type, coef (b, max_det, nm), boxes (b, max_det, 4), all
    procedural; the boxes are test_hip_segval._boxes' (its edge list first) in `case.shape` coordinates; the last counted row of
    an image with three or more has all-zero coefficients.  Also (rows' coef, boxes, img) of the counted rows in buffer order."""
    from tests.test_hip_segval import _boxes
    from ultralytics_pro_amd.utils import procedural as P
    b, md, nm = case.b, case.max_det, case.nm
    protos = P.uniform(f"{case.key}:p", (b, *case.mhw, nm), -1.0, 1.0)
    if dtype == "bf16":
        protos = protos.to(torch.bfloat16).float()
    coef = P.uniform(f"{case.key}:c", (b, md, nm), -1.0, 1.0)
    boxes = torch.from_numpy(_boxes(b * md, case.shape[0], case.shape[1], f"{case.key}:b")).reshape(b, md, 4)
    for i, n in enumerate(case.counts):
        if n >= 3:
            coef[i, n - 1] = 0.0
    sel = [(i, j) for i, n in enumerate(case.counts) for j in range(n)]
    ii = np.array([s[0] for s in sel], np.int64)
    jj = np.array([s[1] for s in sel], np.int64)
    return SimpleNamespace(protos=protos, coef=coef, boxes=boxes, row_coef=coef.numpy()[ii, jj], row_boxes=boxes.numpy()[ii, jj], img=ii)


@functools.lru_cache(maxsize=None)
def _reference(name, dtype):
    case = {c.name: c for c in mask_kernel_cases()}[name]
    inp = case_inputs(case, dtype)
    ref = mask_reference(inp.protos.numpy(), inp.row_coef, inp.row_boxes, case.out_hw, case.mode, case.ratio, case.window, inp.img)
    return inp, ref


def case_reference(case, dtype="f32"):
    """(inputs, reference) of a case, computed once a process and shared: leave them unchanged."""
    return _reference(case.name, dtype)
