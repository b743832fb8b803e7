"""Float64 CPU restatement of the first-layer kernels (csrc/stem.hip: stem_conv_kernel, stem_mfma_kernel with its POOL and G16 forms,
stem_conv_fused_kernel, stem_conv_fused32_kernel) and the per-element bound they are held to.

Where the kernels round (read off csrc/stem.hip, not off a run):
  scalar kernel    nothing before the output: f32 / bf16 / uint8 inputs and the f32 weights enter the fmaf chain as they are
                   (uint8: float(b) / 255.0f, one correctly rounded f32 division), one rounding into the output type;
  MFMA family      an f32 input, the uint8 table value and the f32 weights are rounded to bf16 ONCE, to nearest even (pack_bf16x2 /
                   f32_to_bf16 = v_cvt_pk_bf16_f32), on the way into LDS / the A fragments: a decided rounding of a given number - the
                   reference applies rn_bf16 to them and carries no interval for it;
  POOL             MaxPool2d(2, 2) of the bf16-rounded activations (G16 form: the max is taken on the f32 values before the rounding -
                   the same bits, rounding to nearest being monotone; only the sign of a zero may differ);
  fused pair       the stem tile is rounded to bf16 in LDS (pack_bf16x2) and is ZERO outside the stem map (the second conv's padding), the
                   second conv's weights are bf16 (upa_pack_conv_weight), one bf16 rounding of the output.

Plain torch on the CPU; nothing here imports the HIP package.  tests/test_stem_ref.py pins these functions; tests/test_hip_stem.py
compares every instantiation csrc/stem.hip can launch with them (SINGLE_CASES, POOL_CASES, FUSED_CASES below are the lists both walk)."""

import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests import block_ref as B
from tests import conv_ref as CR
from tests.block_ref import _bf, rn_bf16, stage, store_bf16
from tests.conv_ref import ACT_NONE, ACT_SILU, F64, conv_bound, conv_ref

BF16 = torch.bfloat16
# Below this a stored value counts as "zero, give or take": rn_bf16 does not restate the range under 2^-120, and SiLU's far tail is where the
# kernels' v_rcp_f32 may flush a denormal 1 / (1 + e^-v) (e^v < 2^-126 from v = -87.34 down, where |v| e^v <= 1.03e-36 < 2^-118 = 3.0e-36)
TINY = 2.0 ** -118

# upa_stem_variant's bit layout (include/upa.h)
SCALAR, MFMA, MFMA_G16, FUSED16, FUSED32 = 1, 2, 3, 4, 5
DMA, VGPR, U8 = 0, 1, 2


def decode_variant(v):
    assert v >= 0, v
    return dict(family=v & 7, nt=(v >> 3) & 7, ks=(v >> 6) & 7, s=(v >> 9) & 3, pool=(v >> 11) & 1, silu=(v >> 12) & 1, staging=(v >> 13) & 3,
                waves=(v >> 15) & 15, f32out=(v >> 19) & 1, wgs=v >> 32)


# ---------------------------------------------------------------------------------------------------------------------
# uint8 BGR HWC frames
# ---------------------------------------------------------------------------------------------------------------------
def u8_table():
    """The 256 values float32(b) / float32(255) (one correctly rounded f32 division: `im.float(); im /= 255`), as float64."""
    return torch.from_numpy((np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float64))


def u8_to_nchw(frames, mfma, reverse=True):
    """frames: uint8 (N, H, W, 3) BGR -> float64 NCHW RGB through the table; the MFMA family stages the table value as bf16."""
    tab = u8_table()
    if mfma:
        tab = rn_bf16(tab)
    x = tab[frames.long()]
    if reverse:
        x = x.flip(-1)
    return x.permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------------
# the three forms
# ---------------------------------------------------------------------------------------------------------------------
def stem_single(x, w, bias, k, stride, pad, act, out_dtype, mfma):
    """One first-layer conv -> (ref float64 NCHW, bound): conv_ref / conv_bound with K = cin k^2; the MFMA family's operands are rounded
    to bf16 first (rn_bf16: decided)."""
    x, w = x.to(F64), w.to(F64)
    if mfma:
        x, w = rn_bf16(x), rn_bf16(w)
    v, S, ref = conv_ref(x, w, bias, None, k, stride, pad, act)
    return ref, conv_bound(v, S, ref, x.shape[1] * k * k, act, out_dtype)


def stem_pool(x, w, bias, pad, stage_fn=stage):
    """Conv(k 3, s 1) + SiLU -> bf16 store -> MaxPool2d(2, 2): (pooled stored values, bound).  |max a_i' - max a_i| <= max |a_i' - a_i|: the
    pooled bound is the largest of the four stored-value bounds (0 where all four are decided)."""
    t, e = stage_fn(rn_bf16(x.to(F64)), None, rn_bf16(w.to(F64)), bias, 3, 1, ACT_SILU, pad=pad)
    return F.max_pool2d(t, 2, 2), F.max_pool2d(e, 2, 2)


def store_bf16_flush(a, e_pre):
    """store_bf16 for families whose outputs reach below TINY (SiLU's far negative tail): such an endpoint is taken as 0 and TINY - more than
    any value there can round to - is added to the element's bound, which is then never 0."""
    lo, hi = a - e_pre, a + e_pre
    small = (a.abs() < TINY) | (lo.abs() < TINY) | (hi.abs() < TINY)

    def fl(q):
        return torch.where(q.abs() < TINY, torch.zeros_like(q), q)
    t = rn_bf16(fl(a))
    e = torch.maximum((rn_bf16(fl(hi)) - t).abs(), (rn_bf16(fl(lo)) - t).abs())
    return t, e + small.to(F64) * TINY


def fused_pair(x, w0, b0, k0, s0, p0, w1, b1, stage_fn=stage, store=None, trace=None):
    """Conv(3, c0, k0, s0, p0) + SiLU -> bf16 tile -> Conv(c0, 2 c0, 3, 2, 1) + SiLU -> bf16 (upa_stem_conv_fused*).  The second stage's
    zero padding IS the zero stem pixels outside the stem map."""
    kw = {} if store is None else {"store": store}
    t, e = stage_fn(x.to(F64), None, rn_bf16(w0.to(F64)), b0, k0, s0, ACT_SILU, pad=p0, **kw)
    if trace is not None:
        trace.append((t, e))
    return stage_fn(t, e, w1, b1, 3, 2, ACT_SILU, **kw)


# ---------------------------------------------------------------------------------------------------------------------
# input families
# ---------------------------------------------------------------------------------------------------------------------
def single_data(case):
    """x (float32 NCHW holding what the input type stores, or uint8 NHWC BGR frames), w OIHW f32 (NOT bf16-exact: the MFMA family must
    round it), bias f32.  uniform: everything in [-1, 1]; saturated: conv_ref's (pre-activations to +-120); u8: random bytes."""
    g = torch.Generator().manual_seed(case["seed"])
    n, cin, h, w, cout, k = case["n"], case["cin"], case["h"], case["w"], case["cout"], case["k"]
    fam = "saturated" if case["family"] == "saturated" else "uniform"
    x, wt, bias, _ = CR.conv_family(fam, n, cin, h, w, cout, k, torch.float32, case["seed"])
    if case["fmt"] == "u8":
        x = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
        x[0, 0, 0], x[0, 0, 1], x[-1, -1, -1] = torch.tensor([0, 1, 255], dtype=torch.uint8), torch.tensor([254, 2, 3], dtype=torch.uint8), torch.tensor([1, 0, 255], dtype=torch.uint8)
    elif case["fmt"] == "bf16":
        x = _bf(x)
    return dict(x=x, w=wt, b=bias)


def single_reference(case, d):
    mfma = case["expect"]["family"] in (MFMA, MFMA_G16)
    x = u8_to_nchw(d["x"], mfma) if case["fmt"] == "u8" else d["x"]
    if case.get("pool"):
        return stem_pool(x, d["w"], d["b"], case["pad"])
    return stem_single(x, d["w"], d["b"], case["k"], case["s"], case["pad"], case["act"], BF16 if case["out"] == "bf16" else torch.float32, mfma)


def fused_data(case, family):
    """positive / impulse: block_ref's families (inputs in [0, 1.5] | lit pixels at the corners and on both sides of every tile seam; weights
    in [0, 3 / K], biases in [0, 0.5] - never zero, so that the stem map is SiLU(b0) > 0 where nothing is lit and a stem pixel outside the
    map that is not ZERO shows as whole taps of the second conv).  uniform: everything in [-1, 1], w0 not bf16-exact (the kernel rounds it).
    saturated: conv_ref's, on both convs.  w1 is bf16-exact throughout (its packing is host code with its own test)."""
    g = torch.Generator().manual_seed(case["seed"] + {"positive": 0, "impulse": 1, "uniform": 2, "saturated": 3}[family] * 100000)
    n, h, w, k0, c0 = case["n"], case["h"], case["w"], case["k0"], case["c0"]
    if family in ("positive", "impulse"):
        x = B.family_input(family, g, n, 3, h, w, case["seams_x"], case["seams_y"])
        w0, b0 = B.family_conv("positive", g, c0, 3, k0)
        w1, b1 = B.family_conv("positive", g, 2 * c0, c0, 3)
        return dict(x=x, w0=w0, b0=b0, w1=w1, b1=b1)
    x, w0, b0, _ = CR.conv_family(family, n, 3, h, w, c0, k0, torch.float32, case["seed"] + 7)
    _, w1, b1, _ = CR.conv_family(family, 1, c0, 3, 3, 2 * c0, 3, BF16, case["seed"] + 8)
    if family == "saturated":
        w1 = _bf(w1 / 8)  # the stem tile already spans +-120
    return dict(x=_bf(x), w0=w0, b0=b0, w1=w1, b1=b1)


def fused_reference(case, d, family, stage_fn=stage, trace=None):
    store = store_bf16_flush if family in ("uniform", "saturated") else None
    return fused_pair(d["x"], d["w0"], d["b0"], case["k0"], case["s0"], case["p0"], d["w1"], d["b1"], stage_fn, store, trace)


# ---------------------------------------------------------------------------------------------------------------------
# cases.  Every case states what upa_stem_variant / upa_stem_fused_variant must answer for it (`expect`) - the tile geometry is restated
# here from the kernels' constants (8 x 64 output tiles of stem_mfma_kernel, 256-pixel tiles of stem_conv_kernel, 8 x 16 of the fused pair).
# ---------------------------------------------------------------------------------------------------------------------
def _out_hw(h, w, k, s, pad):
    return (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1


def _cdiv(a, b):
    return -(-a // b)


def _single(fmt, n, cin, h, w, cout, k, s, pad, act, out, family="uniform", opts=None, pool=0, misalign=False, walk=False):
    opts = dict(opts or {})
    oh, ow = _out_hw(h, w, k, s, pad)
    mfma = out == "bf16" and not opts.get("stem_no_mfma") and cin == 3 and cout in (16, 32, 64) and (k, s) in ((3, 1), (3, 2), (6, 2))
    if mfma:
        tiles = _cdiv(ow, 64) * _cdiv(oh, 8) * n
        wgs = min(tiles, opts.get("stem_wgs") or 1024)
        fam = MFMA_G16 if (k, s, pad, act) == (3, 1, 1, ACT_SILU) else MFMA
        staging = U8 if fmt == "u8" else (DMA if (fmt == "bf16" and w % 8 == 0 and not misalign) else VGPR)
        exp = dict(family=fam, nt=cout // 16, ks=k, s=s, pool=pool, silu=int(act == ACT_SILU), staging=staging, waves=4, f32out=0, wgs=wgs)
    else:
        tw = 64 if ow >= 64 else (32 if ow >= 32 else 16)
        tiles = _cdiv(ow, tw) * _cdiv(oh, 256 // tw) * n
        exp = dict(family=SCALAR, nt=0, ks=k, s=s, pool=0, silu=int(act == ACT_SILU), staging=U8 if fmt == "u8" else VGPR, waves=4,
                   f32out=int(out == "f32"), wgs=tiles * _cdiv(cout, 16))
    return dict(fmt=fmt, n=n, cin=cin, h=h, w=w, cout=cout, k=k, s=s, pad=pad, act=act, out=out, family="u8" if fmt == "u8" else family, opts=opts,
                pool=pool, misalign=misalign, walk=walk, tiles=tiles, oh=oh, ow=ow, expect=exp)


def _finish(cs, seed0, name):
    for i, c in enumerate(cs):
        c["seed"] = seed0 + i
        c["id"] = name(c)
    return cs


def _single_id(c):
    e = c["expect"]
    fam = {SCALAR: "scalar", MFMA: "mfma", MFMA_G16: "g16"}[e["family"]] + ("pool" if c["pool"] else "")
    return "-".join([fam, f"nt{e['nt']}" if e["nt"] else f"c{c['cin']}x{c['cout']}", f"k{c['k']}s{c['s']}p{c['pad']}", "silu" if e["silu"] else "none",
                     c["fmt"] + ("mis" if c["misalign"] else ""), c["out"], c["family"][:3], f"{c['n']}x{c['h']}x{c['w']}"] + [f"{k}{v}" for k, v in c["opts"].items()])


def _mfma_cases():
    """Per kernel shape (k, s, pad, H, the DMA width, the odd width): the four input formats x stem_wgs {0, 2, 3}, with NT, the activation
    and the family dealt in turn so that every (NT, KS, S, SiLU | none | G16) instantiation is met by all of them over the list.  Two tiles
    in x and in y, the last ones partial, n = 2: stem_wgs 2 walks 4 tiles per workgroup, 3 walks 3 | 3 | 2 - across the image boundary."""
    cs = []
    shapes = [(3, 2, 1, 18, 136, 133), (3, 1, 1, 10, 72, 67), (6, 2, 2, 18, 136, 134), (3, 1, 0, 12, 72, 67)]
    for si, (k, s, pad, h, w8, wodd) in enumerate(shapes):
        i = 0
        for wgs in (0, 2, 3):
            for fmt, w in (("bf16", w8), ("bf16", wodd), ("f32", wodd), ("u8", wodd if wgs else w8)):
                nt = (1, 2, 4)[(i + si) % 3]
                act = (ACT_SILU, ACT_NONE)[(i // 3 + si) % 2]
                fam = "saturated" if (i % 5 == 4 and act == ACT_SILU) else "uniform"
                cs.append(_single(fmt, 2, 3, h, w, 16 * nt, k, s, pad, act, "bf16", fam, dict(stem_wgs=wgs) if wgs else {}, walk=bool(wgs)))
                i += 1
    # the XCD-aware walk over several rounds (grid a multiple of 8, fewer workgroups than tiles) and its switch; n = 5: 20 tiles
    for no_xcd in (0, 1):
        cs.append(_single("bf16", 5, 3, 18, 136, 32, 3, 2, 1, ACT_SILU, "bf16", "uniform", dict(stem_wgs=8, no_xcd=no_xcd), walk=True))
    cs.append(_single("bf16", 2, 3, 18, 136, 16, 3, 2, 1, ACT_SILU, "bf16", "uniform", dict(no_xcd=1)))
    # a bf16 input 2 bytes into its allocation, W % 8 == 0: VGPR staging (the 16-byte LDS-DMA needs an aligned source)
    cs.append(_single("bf16", 2, 3, 18, 136, 16, 3, 2, 1, ACT_SILU, "bf16", "uniform", dict(stem_wgs=3), misalign=True, walk=True))
    cs.append(_single("bf16", 2, 3, 10, 72, 32, 3, 1, 1, ACT_SILU, "bf16", "uniform", {}, misalign=True))
    return cs


def _pool_cases():
    cs = []
    i = 0
    for pad, shapes in ((1, ((10, 72), (12, 136))), (0, ((12, 72), (14, 136)))):   # pad 1: the G16 form, pad 0: the gather form
        for cout in (16, 32, 64):
            for (h, w) in shapes:
                for wgs in (0, 3):
                    j = (i + i // 4) % 4  # (moves on by one per channel count: each format meets both shapes and both walks)
                    fmt = ("bf16", "f32", "u8", "bf16")[j]
                    ww = w + 2 if j == 3 else w  # the fourth: a bf16 width that is no multiple of 8 (VGPR), still an even output
                    cs.append(_single(fmt, 2, 3, h, ww, cout, 3, 1, pad, ACT_SILU, "bf16", "uniform", dict(stem_wgs=wgs) if wgs else {}, pool=1, walk=bool(wgs)))
                    i += 1
    return cs


def _scalar_cases():
    S, N = ACT_SILU, ACT_NONE
    nm = dict(stem_no_mfma=1)
    return [
        # 64 x 4 tiles (OW >= 64), two in x, two in y, the last partial
        _single("f32", 2, 1, 6, 70, 8, 1, 1, 0, S, "f32"),
        _single("u8", 2, 3, 6, 70, 12, 5, 1, 2, S, "bf16"),
        _single("bf16", 2, 3, 18, 136, 16, 3, 2, 1, S, "bf16", opts=nm),            # the MFMA shape on the scalar kernel, even W: dword pairs
        _single("bf16", 2, 4, 6, 70, 48, 5, 1, 2, N, "f32", family="saturated"),
        _single("f32", 2, 3, 18, 133, 32, 6, 2, 2, N, "bf16", opts=nm),
        # 32 x 8 tiles
        _single("bf16", 2, 4, 22, 80, 12, 5, 2, 2, N, "bf16"),
        _single("bf16", 2, 1, 11, 41, 8, 7, 1, 3, S, "bf16", family="saturated"),   # odd W: the pair path's element loads
        _single("u8", 2, 3, 22, 81, 48, 3, 2, 1, N, "f32"),
        # 16 x 16 tiles
        _single("bf16", 2, 4, 37, 39, 48, 7, 2, 3, S, "f32"),
        _single("f32", 2, 4, 37, 39, 12, 1, 2, 0, N, "bf16"),
        _single("bf16", 3, 1, 19, 20, 8, 5, 1, 2, S, "f32"),
        # a bf16 input 2 bytes into its allocation, even W: no dword pair loads
        _single("bf16", 2, 4, 22, 80, 8, 5, 2, 2, S, "bf16", misalign=True),
    ]


SINGLE_CASES = _finish(_mfma_cases() + _scalar_cases(), 3000, _single_id)
POOL_CASES = _finish(_pool_cases(), 4000, _single_id)


def _fused(n, h, w, k0, s0, c0, opts=None, families=("positive", "impulse", "uniform", "saturated"), walk=False):
    opts = dict(opts or {})
    oh, ow = h // (2 * s0), w // (2 * s0)
    tiles = _cdiv(ow, 16) * _cdiv(oh, 8) * n
    waves = 8 if c0 == 32 else (4 if (k0 == 6 or opts.get("stemf_waves") == 4) else 8)
    exp = dict(family=FUSED32 if c0 == 32 else FUSED16, nt=c0 // 16, ks=k0, s=s0, pool=0, silu=1, staging=DMA, waves=waves, f32out=0,
               wgs=min(tiles, opts.get("stemf_wgs") or 512))
    px = 16 * 2 * s0  # input pixels per output tile column; rows: 8 * 2 * s0
    return dict(n=n, h=h, w=w, k0=k0, s0=s0, c0=c0, p0=1 if k0 == 3 else 2, opts=opts, families=families, walk=walk, tiles=tiles, oh=oh, ow=ow, expect=exp,
                seams_x=tuple(range(px, w, px)), seams_y=tuple(range(px // 2, h, px // 2)))


def _fused_id(c):
    return "-".join([f"k{c['k0']}s{c['s0']}c{c['c0']}w{c['expect']['waves']}", f"{c['n']}x{c['h']}x{c['w']}"] + [f"{k}{v}" for k, v in c["opts"].items()])


def _fused_cases():
    cs = []
    forms = [(3, 2, 16, {}), (3, 2, 16, dict(stemf_waves=4)), (6, 2, 16, {}), (3, 2, 32, {}), (3, 1, 32, {})]
    for k0, s0, c0, o in forms:
        h, w = (36, 72) if s0 == 2 else (18, 40)   # 9 x 18 | 9 x 20 outputs: 2 x 2 tiles, the last partial; n = 3: 12 tiles
        for wgs in (0, 2, 3):
            cs.append(_fused(3, h, w, k0, s0, c0, dict(o, **({"stemf_wgs": wgs} if wgs else {})), walk=bool(wgs)))
        # 3 x 3 tiles whose middle one is INTERIOR (the 17 x 33 stem tile inside the stem map and the whole staged patch inside the image: the
        # unmasked stage-2 loop and the unchecked DMA pass, what most tiles of a real image run; the shapes above have no such tile), walked by
        # 4 workgroups, and by 8 in the XCD-aware order over several rounds with its switch
        hb, wb = (72, 160) if s0 == 2 else (40, 72)
        cs.append(_fused(2, hb, wb, k0, s0, c0, dict(o, stemf_wgs=4), families=("positive", "impulse"), walk=True))
        cs.append(_fused(2, hb, wb, k0, s0, c0, dict(o, stemf_wgs=8), families=("positive",), walk=True))
    cs.append(_fused(2, 72, 160, 3, 2, 16, dict(stemf_wgs=8, no_xcd=1), families=("positive",), walk=True))
    return cs


FUSED_CASES = _finish(_fused_cases(), 5000, _fused_id)

# every kernel instantiation csrc/stem.hip can launch, as the key `instantiation` makes of a case's asserted variant
INSTANTIATIONS = ([("scalar", out, act) for out in ("f32", "bf16") for act in ("silu", "none")]
                  + [("mfma", nt, ks, s, form) for nt in (1, 2, 4) for (ks, s) in ((3, 2), (3, 1), (6, 2)) for form in ("silu", "none")]
                  + [("mfma", nt, 3, 1, form) for nt in (1, 2, 4) for form in ("g16", "pool", "g16pool")]
                  + [("fused16", 8, 3), ("fused16", 4, 3), ("fused16", 4, 6), ("fused32", 2), ("fused32", 1)])


def instantiation(e):
    """The kernel instantiation a decoded variant names."""
    if e["family"] == SCALAR:
        return ("scalar", "f32" if e["f32out"] else "bf16", "silu" if e["silu"] else "none")
    if e["family"] in (MFMA, MFMA_G16):
        g16 = e["family"] == MFMA_G16
        form = ("g16pool" if g16 else "pool") if e["pool"] else ("g16" if g16 else ("silu" if e["silu"] else "none"))
        return ("mfma", e["nt"], e["ks"], e["s"], form)
    if e["family"] == FUSED16:
        return ("fused16", e["waves"], e["ks"])
    return ("fused32", e["s"])


@functools.lru_cache(maxsize=None)
def single_case_reference(kind, index):
    """(data, (ref, bound)) of SINGLE_CASES / POOL_CASES[index], computed once per process and shared (treat as read-only)."""
    case = (SINGLE_CASES if kind == "single" else POOL_CASES)[index]
    d = single_data(case)
    with torch.no_grad():
        return d, single_reference(case, d)


@functools.lru_cache(maxsize=None)
def fused_case_reference(index, family):
    case = FUSED_CASES[index]
    d = fused_data(case, family)
    with torch.no_grad():
        return d, fused_reference(case, d, family)
