"""Float64 reference, input families and case lists for the Detect decode paths: `upa_detect_decode` (csrc/detect.hip), the decode epilogue
of the streaming 1x1 conv (`upa_detect_tail`, csrc/conv1x1.hip) and the tails of the 3x3 kernel (`upa_detect_branch_tail`, its `_group` form
and `upa_detect_head_tails`, csrc/conv_big.hip), all through csrc/detect_epi.h.  CPU only, on top of tests/block_ref.py: the 3x3 +
SiLU stage and the f32 logits are `B.stage` (stages 2 and 3 of `B.detect_branch`), boxes and scores with their bounds are `B.detect_decode`.
tests/test_detect_ref.py pins what is built here; tests/test_hip_detect_tails.py walks the case lists on the GPU.

Families
  random  logits through the `signed_tail` weights of `B.family_conv`: scores span (0, 1);
  built   the logits are WRITTEN: for `upa_detect_decode` they are the input, for the 1x1 tails the weight is an identity block over bf16
          inputs plus an f32 bias, so that the kernel's logit is fl32(x + bias) - computed here bit for bit in float32, bound 0.  `built_scene`
          lists what a scene holds (ITEMS_BOX, ITEMS_CLS);
  twins   behind a 3x3 stage nothing can be written exactly: `B.twins_tail` makes the ties by identical weight rows (the tails of
          csrc/conv_big.hip here, the level-stream cases in tests/block_ref.py)."""

import functools

import torch

from tests import block_ref as B
from tests.conv_ref import ACT_NONE, ACT_SILU, F64

F32 = torch.float32
NEXT4_UP, NEXT4_DOWN = 2.0 ** -21, -(2.0 ** -22)  # 4 + 2^-21 = nextafter(4, inf), 4 - 2^-22 = nextafter(4, 0) in float32

# the f32 biases of the built class rows: classes 2 / 3 sit one float32 step above / below a bf16 input, 5 / 6 a gap of 2^-14 / 2^-13 above one
CLS_BIAS = {2: NEXT4_UP, 3: NEXT4_DOWN, 5: 2.0 ** -14, 6: 2.0 ** -13}
BOX_BIAS = 0.25  # every bin alike: equal bins stay equal, 30.25 and -29.75 are float32 numbers

# name -> (smallest nc, needs the f32 biases, takes the keys_only fast path when alone in its tile, {class: bf16 input}, answer class or None)
# (answer None: the margin rule decides; nc - 1 is written as -1)
ITEMS_CLS = {
    "score_0_and_1":   (1, False, False, {0: 100.0, -1: -100.0}, 0),   # sigmoid exactly 1.0f and (nc >= 2) exactly 0.0f; largest logit > 4
    "neg_zero":        (1, False, True, {0: -0.0}, 0),
    "tie_one_lane":    (2, False, False, {0: 1.0, 1: 1.0}, 0),          # classes 4 kg + q and 4 kg + q'; also the gap of exactly 0
    "tie_lane_rows":   (5, False, False, {1: 1.5, 4: 1.5}, 1),          # kg 0 and 1
    "tie_n_tiles":     (17, False, False, {0: 0.5, 16: 0.5}, 0),        # c and c + 16
    "max_is_4":        (1, False, True, {0: 4.0}, 0),
    "max_above_4":     (3, True, False, {2: 4.0}, 2),
    "max_below_4":     (4, True, True, {3: 4.0}, 3),
    "gap_below_1e-4":  (6, True, False, {0: 1.0, 5: 1.0}, 5),
    "gap_above_1e-4":  (7, True, True, {0: 1.0, 6: 1.0}, 6),
    "saturated":       (3, False, False, None, None),                   # 17, 18 and 30, the largest logit last: filled in by _cls_row
    "pad_trap":        (1, False, True, {-1: -3.0}, -1),                # every real logit <= -3: with nc < cout a pad channel (logit 0) is the row's largest
    "clear":           (1, False, True, None, None),                    # one class at 2.0
}
ITEMS_BOX = ("hot0", "hot7", "hot15", "equal", "two_maxima", "underflow", "random")


def _cls_row(name, nc, p, base):
    """The bf16 inputs of one anchor's class row for item `name` -> (row, answer)."""
    row = base.clone()
    _, _, _, put, ans = ITEMS_CLS[name]
    if name == "saturated":
        cs = (7, 9, 12) if nc >= 13 else (0, 1, 2)
        for c, v in zip(cs, (17.0, 18.0, 30.0)):
            row[c] = v
        return row, cs[0]
    if name == "clear":
        row[p % nc] = 2.0
        return row, p % nc
    for c, v in put.items():
        if c >= 0 or nc >= 2 or name == "pad_trap":
            row[c] = v
    if name == "score_0_and_1" and nc == 1:
        row[0] = 100.0
    return row, ans % nc


def _box_side(kind, g):
    v = torch.full((16,), -30.0)
    if kind.startswith("hot"):
        v[int(kind[3:])] = 30.0
    elif kind == "equal":
        v[:] = 0.5
    elif kind == "two_maxima":  # bins 2 and 9: lane rows 0 and 2
        v[2] = v[9] = 3.0
    elif kind == "underflow":
        v[:] = -80.0
        v[5] = 80.0
    elif kind == "narrow":      # expectation 0.27: the box is half a pixel wide wherever it stands
        v[0], v[1] = 0.0, -1.0
    else:
        v = B._bf(torch.rand(16, generator=g) * 8 - 4)
    return v


def built_scene(seed, n, h, w, nc, cout=None, f32_bias=True, underflow=False):
    """One `built` scene.  Returns a dict:
      xb (n, 64, h, w), bb (64)        bf16-exact box inputs and the f32 box bias; xc (n, cout, h, w), bc (cout): the class side
                                       (channels nc .. cout - 1 are zero with zero bias: what the head's zero padding gives);
      bl (n, 64, h, w), cl (n, nc, h, w)   the logits fl32(x + bias), float32;
      items   name -> flat pixels that hold it;   want (n * h * w) the constructed best class, -1 where the margin rule is to decide;
      fast    (n * h * w) bool: the pixel is meant to pass the keys_only test of detect_epi.h on its own.
    Layout over the flat pixel index p (the 16-pixel tiles of the 1x1 kernel): tile 0 holds only pixels meant for the fast path, tile 1 the
    same but for ONE tie at p = 21, tile 2 the same but for ONE saturated pixel at p = 37 (17, 18 and 30 in different lane rows, a gap of
    12: only the `largest logit <= 4` clause keeps that tile off the fast path, which would name the class at 30 where the first of the
    three 1.0f scores is the answer), from p = 48 on the items take turns (13 items: every residue of 16 gets every item in the end, full and
    ragged tiles alike).  The box sides take turns from p = 0 (7 kinds, side s shifted by 2 s); the last column is `narrow` on sides 0 and 2
    (x2 - x1 cancels at the highest column index) and column 7 has side 0 `hot15` against side 2 `hot0` (x1 + x2 = -7.5 + 7.5)."""
    g = torch.Generator().manual_seed(seed)
    cout = nc if cout is None else cout
    P = n * h * w
    names = [k for k, v in ITEMS_CLS.items() if nc >= v[0] and (f32_bias or not v[1])]
    # (neg_zero stays out of the three leading tiles: its 0 would tie with an unmasked pad channel's 0 and send the tile through the full
    # path, hiding a keys_only scan that forgets to mask the pads behind the path that masks them)
    fast_names = [k for k in names if ITEMS_CLS[k][2] and k != "neg_zero"]
    xc = torch.zeros(P, cout)
    want = torch.full((P,), -1, dtype=torch.int64)
    fast = torch.zeros(P, dtype=torch.bool)
    items = {k: [] for k in names}
    for p in range(P):
        base = -(6.0 + torch.randint(0, 5, (nc,), generator=g).float())
        if p < 48 and P >= 48:
            name = "tie_one_lane" if (p == 21 and nc >= 2) else "saturated" if (p == 37 and nc >= 3) else fast_names[p % len(fast_names)]
        else:
            name = names[(p - 48) % len(names)] if P >= 48 else names[p % len(names)]
        row, ans = _cls_row(name, nc, p, base)
        xc[p, :nc] = row
        items[name].append(p)
        fast[p] = ITEMS_CLS[name][2]
        want[p] = -1 if ans is None else ans
    bc = torch.zeros(cout)
    if f32_bias:
        for c, v in CLS_BIAS.items():
            if c < nc:
                bc[c] = v
    kinds = [k for k in ITEMS_BOX if underflow or k != "underflow"]
    xb = torch.zeros(P, 64)
    box_items = {k: [] for k in kinds + ["narrow", "sum_cancels"]}
    for p in range(P):
        col = p % w
        for s in range(4):
            kind = kinds[(p + 2 * s) % len(kinds)]
            if w > 1 and col == w - 1 and s in (0, 2):
                kind = "narrow"
            elif col == 7 and col != w - 1 and s in (0, 2):
                kind = "hot15" if s == 0 else "hot0"
                if s == 0:
                    box_items["sum_cancels"].append(p)
            xb[p, 16 * s:16 * s + 16] = _box_side(kind, g)
            box_items[kind].append(p)
    bb = torch.full((64,), BOX_BIAS if f32_bias else 0.0)

    def nchw(t):
        return t.reshape(n, h, w, -1).permute(0, 3, 1, 2).contiguous()
    xb, xc = nchw(xb), nchw(xc)
    assert torch.equal(B._bf(xb), xb) and torch.equal(B._bf(xc), xc)
    bl = xb + bb.view(1, -1, 1, 1)          # float32 adds: the kernel's fl32(acc + bias) with acc = x exactly
    cl = (xc + bc.view(1, -1, 1, 1))[:, :nc]
    assert bl.dtype == F32 and cl.dtype == F32
    return dict(xb=xb, bb=bb, xc=xc, bc=bc, bl=bl, cl=cl, items=dict(items, **{"box_" + k: v for k, v in box_items.items()}), want=want, fast=fast,
                n=n, h=h, w=w, nc=nc, cout=cout)


def identity_weight(cout, cin):
    """A single 1.0 per row: output channel c reads input channel c."""
    wt = torch.zeros(cout, cin, 1, 1)
    wt[torch.arange(cout), torch.arange(cout)] = 1.0
    return wt


# ---------------------------------------------------------------------------------------------------------------------
# float32 emulations of detect_epi.h (what the CPU test shows about the scenes)
# ---------------------------------------------------------------------------------------------------------------------
def sigmoid_f32(l):
    """1 / (1 + exp(-l)) in float32 (the kernel's 1.0f + v_exp_f32 rounds the same way wherever exp(-l) is not within 2 ulp of a tie)."""
    l = l.to(F32)
    return 1.0 / (1.0 + torch.exp(-l))


def keys_only_sure(cl32, max_clause=True):
    """The `sure` test of upa_detect_cls_keys_only (detect_epi.h:105-120) in float32 on logits (n, nc, h, w) -> (n, h * w) bool.
    Lane row kg holds the classes with (c % 16) // 4 == kg; m1 / m2 are a row's largest and second largest logit (a tie inside the row makes
    m2 = m1), pm the pixel's largest, ps = max over rows of (m1 == pm ? m2 : m1); sure = pm <= 4 and pm - ps >= 1e-4f and one row holds pm.
    max_clause=False: the rule without `pm <= 4` (what the saturated tile of built_scene is there to tell apart)."""
    n, nc = cl32.shape[:2]
    lg = cl32.to(F32).reshape(n, nc, -1)
    kg = (torch.arange(nc) % 16) // 4
    m1 = torch.full((n, 4, lg.shape[2]), -float("inf"))
    m2 = m1.clone()
    for r in range(4):
        rows = lg[:, kg == r]
        if rows.shape[1] >= 1:
            top = rows.topk(min(2, rows.shape[1]), dim=1).values
            m1[:, r] = top[:, 0]
            if rows.shape[1] >= 2:
                m2[:, r] = top[:, 1]
    pm = m1.max(1).values
    ps = torch.where(m1 == pm.unsqueeze(1), m2, m1).max(1).values
    gap = pm - ps
    assert gap.dtype == F32
    return ((pm <= 4.0) | (not max_clause)) & (gap >= torch.tensor(1e-4, dtype=F32)) & ((m1 == pm.unsqueeze(1)).sum(1) == 1)


def tiles_fast(sure, tile=16):
    """(P) bool per flat pixel -> per 16-pixel tile: every pixel sure (the wave-uniform test; pixels past the end count as sure)."""
    P = sure.numel()
    pad = (-P) % tile
    return torch.cat([sure.flatten(), torch.ones(pad, dtype=torch.bool)]).view(-1, tile).all(1)


# ---------------------------------------------------------------------------------------------------------------------
# deciding the best class
# ---------------------------------------------------------------------------------------------------------------------
def margin_decided(sref, es):
    """The rule of tests/test_hip_blocks.py:223-226 -> (argmax (n, A), decided (n, A))."""
    if sref.shape[1] == 1:
        return torch.zeros_like(sref[:, 0], dtype=torch.int64), torch.ones_like(sref[:, 0], dtype=torch.bool)
    top, idx = sref.topk(2, dim=1)
    return idx[:, 0], (top[:, 0] - top[:, 1]) > es.gather(1, idx).sum(1)


def built_answer(scene, dec):
    """(want, decided) of a built scene: the constructed answer where the scene names one, else the margin rule."""
    n = scene["n"]
    arg, clear = margin_decided(dec["score"], dec["e_score"])
    want = scene["want"].view(n, -1)
    return torch.where(want >= 0, want, arg), clear | (want >= 0)


# ---------------------------------------------------------------------------------------------------------------------
# cases (walked by tests/test_detect_ref.py on the CPU and tests/test_hip_detect_tails.py on the GPU)
# ---------------------------------------------------------------------------------------------------------------------
DECODE_CASES = [dict(dtype=dt, family=fam, nc=nc, shape=shp, id=f"{dt}-{fam}-nc{nc}-{'x'.join(map(str, shp))}")
                for dt in ("f32", "bf16") for fam in ("random", "built") for nc in (1, 3, 80, 81, 128, 256) for shp in ((2, 5, 7), (1, 1, 1), (3, 9, 11))]
TAIL_CASES = [dict(nc=nc, cout=cout, family=fam, shape=shp, id=f"{fam}-nc{nc}-cout{cout}-{'x'.join(map(str, shp))}")
              for (nc, cout) in ((3, 8), (20, 24), (33, 48), (64, 64), (80, 80), (91, 96), (100, 112), (128, 128), (7, 8), (79, 80))
              for shp in ((2, 13, 21), (3, 5, 7)) for fam in ("random", "built")]
BRANCH_CASES = [dict(c=c, nc=nc, bm=bm, family=fam, shape=shp, id=f"{fam}-c{c}-nc{nc}-bm{bm}-{'x'.join(map(str, shp))}")
                for (c, nc) in ((80, 80), (80, 77), (64, 20), (96, 91), (96, 96), (80, 79)) for bm in (128, 256)
                for shp in ((2, 13, 21), (1, 9, 16)) for fam in ("random", "twins")]
# (7, 8), (79, 80) and c = 80 with nc = 79 are beyond the issue's list: exactly ONE zero-padded channel.  Two or more pads tie at 0 with each other, so a
# keys_only scan that forgot to mask them would call every such pixel unsure and fall back to the path that masks: only a single pad can win.
GROUP_LEVELS = ((1, 16, 16), (1, 8, 8), (1, 4, 4))
GROUP_CASES = [dict(entry="head_tails", no_group=0, id="head_tails"), dict(entry="group", no_group=0, id="group-pairs"),
               dict(entry="group", no_group=2, id="group-threes")]


def _seed(*key):
    s = 0
    for ch in repr(key):
        s = (s * 131 + ord(ch)) % 1000003
    return 5000 + s


@functools.lru_cache(maxsize=None)
def decode_reference(dtype, family, nc, shape):
    """-> (box input (n, 64, h, w) f32 tensor exact in `dtype`, class input (n, nc, h, w), B.detect_decode's dict, scene or None)."""
    n, h, w = shape
    g = torch.Generator().manual_seed(_seed("decode", dtype, family, nc, shape))
    if family == "built":
        sc = built_scene(_seed("decode-built", dtype, nc, shape), n, h, w, nc, f32_bias=dtype == "f32", underflow=dtype == "f32")
        bl, cl = sc["bl"], sc["cl"]
    else:
        sc = None
        bl, cl = torch.rand(n, 64, h, w, generator=g) * 16 - 8, torch.rand(n, nc, h, w, generator=g) * 16 - 8
        if dtype == "bf16":
            bl, cl = B._bf(bl), B._bf(cl)
    z = torch.zeros((), dtype=F64)
    dec = B.detect_decode(bl.to(F64), z.expand_as(bl), cl.to(F64), z.expand_as(cl), 8.0)
    return bl, cl, dec, sc


@functools.lru_cache(maxsize=None)
def tail_reference(nc, cout, family, shape):
    """`upa_detect_tail`: -> dict(xb, wb, bb, xc, wc, bc: inputs / OIHW weights (cout rows, zero-padded) / biases; dec; raw_b, raw_c:
    (bf16 value, bound) of the raw maps; scene or None)."""
    n, h, w = shape
    g = torch.Generator().manual_seed(_seed("tail", nc, cout, family, shape))
    if family == "built":
        sc = built_scene(_seed("tail-built", nc, cout, shape), n, h, w, nc, cout=cout)
        xb, wb, bb, xc, wc, bc = sc["xb"], identity_weight(64, 64), sc["bb"], sc["xc"], identity_weight(cout, cout), sc["bc"]
        bl, cl = sc["bl"].to(F64), sc["cl"].to(F64)
        be, ce = torch.zeros_like(bl), torch.zeros_like(cl)
        cl_all = (xc + bc.view(1, -1, 1, 1)).to(F64)
        raw_b, raw_c = (B.rn_bf16(bl), torch.zeros_like(bl)), (B.rn_bf16(cl_all), torch.zeros_like(cl_all))
    else:
        sc = None
        xb, xc = B.family_input("positive", g, n, 64, h, w), B.family_input("positive", g, n, cout, h, w)
        wb, bb = B.family_conv("positive", g, 64, 64, 1, signed_tail=True)
        wc, bc = B.family_conv("positive", g, nc, cout, 1, signed_tail=True)
        wc, bc = torch.cat([wc, torch.zeros(cout - nc, cout, 1, 1)]), torch.cat([bc, torch.zeros(cout - nc)])
        bl, be = B.stage(xb, None, wb, bb, 1, 1, ACT_NONE, out_dtype=F32)
        cl_all, ce_all = B.stage(xc, None, wc, bc, 1, 1, ACT_NONE, out_dtype=F32)
        cl, ce = cl_all[:, :nc], ce_all[:, :nc]
        raw_b, raw_c = B.stage(xb, None, wb, bb, 1, 1, ACT_NONE), B.stage(xc, None, wc, bc, 1, 1, ACT_NONE)
    dec = B.detect_decode(bl, be, cl, ce, 16.0)
    return dict(xb=xb, wb=wb, bb=bb, xc=xc, wc=wc, bc=bc, cl=cl, ce=ce, dec=dec, raw_b=raw_b, raw_c=raw_c, scene=sc)


def branch_cp(kind, c):
    """The padded channel count of a branch tail (conv_big.hip:737-740): 64 (box), 80 (class, c = 80), else 96."""
    return 64 if kind == 1 else (80 if c == 80 else 96)


@functools.lru_cache(maxsize=None)
def branch_reference(c, nc, family, shape, seed_extra=0):
    """`upa_detect_branch_tail`: box branch (c = 64) and class branch (c) of one level, each 3x3 + SiLU -> bf16 -> 1x1 -> f32 logits (stages
    2 and 3 of `B.detect_branch`).  -> dict(box=(x, (w3, b3), (wt, bt)), cls=(...), cl, ce, dec)."""
    n, h, w = shape
    g = torch.Generator().manual_seed(_seed("branch", c, nc, family, shape, seed_extra))
    out, lg = {}, {}
    for name, ch, co in (("box", 64, 64), ("cls", c, nc)):
        if family == "twins":
            x = B.twins_input(g, n, ch, h, w)
            c3 = B.family_conv("impulse", g, ch, ch, 3)
            tail = B.twins_tail(g, nc, ch) if name == "cls" else B.family_conv("positive", g, co, ch, 1, signed_tail=True)
        else:
            x = B.family_input("positive", g, n, ch, h, w)
            c3 = B.family_conv("positive", g, ch, ch, 3)
            tail = B.family_conv("positive", g, co, ch, 1, signed_tail=True)
        t, e = B.stage(x, None, *c3, 3, 1, ACT_SILU)
        lg[name] = B.stage(t, e, *tail, 1, 1, ACT_NONE, out_dtype=F32)
        out[name] = (x, c3, tail)
    out["cl"], out["ce"] = lg["cls"]
    out["dec"] = B.detect_decode(*lg["box"], *lg["cls"], 16.0)
    return out


def branch_answer(ref, family):
    """(want, decided) of a branch-tail case."""
    if family == "twins":
        return B.twins_answer(ref["cl"], ref["ce"])
    return margin_decided(ref["dec"]["score"], ref["dec"]["e_score"])
