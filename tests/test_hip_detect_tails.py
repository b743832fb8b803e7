"""-m gpu: `upa_detect_decode` (csrc/detect.hip, f32 and bf16) and `upa_detect_tail` (csrc/conv1x1.hip, EPI 1 / 2 through csrc/detect_epi.h)
against the float64 reference of tests/detect_ref.py, element by element inside the reference's bound, on random logits and on BUILT ones:
exact ties of the best class in one lane, across lane rows and across n-tiles, the keys_only thresholds (largest logit 4 and its two
float32 neighbours, gaps of 2^-14 / 2^-13 / 0), saturated pixels whose classes all score 1.0f, a zero-padded channel that holds the row's
largest logit, one unsure pixel in a tile of sure ones, one-hot / equal / two-maxima / underflowing DFL sides, boxes that cancel.

Buffers, sentinels, the two bit-identical runs, the bounds and the fault latch: the conventions of tests/kernel_check.py.  Inputs are channel
slices of NaN-filled buffers (E = 16 bytes on both sides), y is (n + 1, 4 + nc, a0 + hw + extra) NaN-filled with a0 and extra no multiples
of 4, the keys are filled with -1, the raw maps have ldraw > cout.  No bound was read off a GPU run.

BLOCK_STATS=1 prints, per case, the decided share and the worst |kernel - ref| / bound."""

import os

import numpy as np
import pytest
import torch

from tests import detect_ref as D
from tests import kernel_check as KC

pytestmark = pytest.mark.gpu
NAN = float("nan")
A0, EXTRA = 19, 5


def _stats(entry, cid, stats):
    if os.environ.get("BLOCK_STATS"):
        for what, z, s in stats:
            print(f"BLOCK_STATS {entry}|{cid}|{what}|decided={z:.4f}|worst_share={s:.4f}", flush=True)


def _slice(x_nchw, dtype):
    """CPU NCHW -> (whole NaN-filled NHWC device buffer, pointer / shape / pitch of its channel slice [E, E + c))."""
    from types import SimpleNamespace
    E = 16 // torch.tensor([], dtype=dtype).element_size()
    buf = KC.slice_buf(x_nchw.permute(0, 2, 3, 1), dtype, E, tail=E + (-x_nchw.shape[1]) % E)  # (the pitch stays a multiple of 16 bytes)
    n, c, h, w = x_nchw.shape  # (pointer and pitch stated here: the strides of a 1 x 1 map do not tell the pitch)
    return buf, SimpleNamespace(ptr=buf.data_ptr() + 16, n=n, h=h, w=w, c=c, ld=buf.shape[-1])


def _outputs(n, nc, hw):
    DEV = KC.env()[0]
    a_total = A0 + hw + EXTRA
    return (torch.full((n + 1, 4 + nc, a_total), NAN, device=DEV), torch.full((n + 1, a_total), -1, dtype=torch.int64, device=DEV), a_total)


def _level(y, n, hw, rows_written):
    """Asserts that y still holds NaN outside the level, the spare image and the rows a call must not write; returns the level (float64)."""
    lvl = slice(A0, A0 + hw)
    assert bool(torch.isnan(y[n]).all()) and bool(torch.isnan(y[:, :, :A0]).all()) and bool(torch.isnan(y[:, :, A0 + hw:]).all()), "wrote outside the level"
    keep = torch.ones(y.shape[1], dtype=torch.bool)
    keep[rows_written] = False
    assert bool(torch.isnan(y[:n, keep][:, :, lvl]).all()), "rows of the other branch (or, keys-only, the class rows) were written"
    return y[:n, rows_written, lvl].to(torch.float64)


def _keys(keys, n, hw, nc):
    """-> (score bits as float32 (n, hw), class (n, hw)); asserts the keys outside the level still hold -1 and the anchor part is right."""
    lvl = slice(A0, A0 + hw)
    assert bool((keys[n] == -1).all()) and bool((keys[:, :A0] == -1).all()) and bool((keys[:, A0 + hw:] == -1).all()), "keys outside the level"
    kb = keys[:n, lvl].contiguous().numpy().view(np.uint64)
    kscore = torch.from_numpy((~(kb >> np.uint64(32)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32))
    kidx = (kb & np.uint64(0xFFFFFFFF)).astype(np.int64)
    kcls = torch.from_numpy(kidx - np.arange(A0, A0 + hw, dtype=np.int64)[None, :] * nc)
    assert bool(((kcls >= 0) & (kcls < nc)).all()), "a key names a class outside [0, nc) or another anchor"
    return kscore, kcls


# ---------------------------------------------------------------------------------------------------------------------
# upa_detect_decode
# ---------------------------------------------------------------------------------------------------------------------
def _run_decode(bl, cl, dtype, nc, stride=8.0):
    DEV, L, lib, st = KC.env()
    n, _, h, w = bl.shape
    bbuf, vb = _slice(bl, dtype)
    cbuf, vc = _slice(cl, dtype)
    y, _, a_total = _outputs(n, nc, h * w)
    assert vb.ld > 64 and vc.ld > nc
    rc = lib.upa_detect_decode(vb.ptr, vb.ld, vc.ptr, vc.ld, n, h, w, 16, nc, stride, y.data_ptr(), a_total, A0, L.dtype_code(dtype), st)
    torch.cuda.synchronize()
    return rc, y.cpu()


@pytest.mark.parametrize("case", D.DECODE_CASES, ids=[c["id"] for c in D.DECODE_CASES])
@KC.stop_after_fault
def test_detect_decode_vs_f64(case):
    """Boxes and scores inside the bound of `block_ref.detect_decode` (derived for v_exp_f32 / v_rcp_f32; the f32 instantiation's ocml expf and IEEE
    divide are no less accurate and are held to the same bound); nothing outside the level is written and no NaN of the guard columns
    that the 16-byte class loads touch comes out.  nc 1 / 3 / 81: class counts that are no multiple of the 16-byte group; 80 -> gcp 32 of 20
    (bf16: 16 of 10) padded groups; 256: the largest f32 row that fits LDS.  Totals of 70, 1 and 297 anchors: the last wave clamps its reads."""
    L = KC.env()[1]
    dtype = torch.float32 if case["dtype"] == "f32" else torch.bfloat16
    bl, cl, dec, _ = D.decode_reference(case["dtype"], case["family"], case["nc"], case["shape"])
    n, h, w = case["shape"]

    def run():
        rc, y = _run_decode(bl, cl, dtype, case["nc"])
        L.check(rc, "detect_decode")
        return y
    y = KC.twice(run)
    got = _level(y, n, h * w, slice(0, 4 + case["nc"]))
    stats = [("box", 1.0, KC.check_bound(got[:, :4], dec["box"], dec["e_box"], "box")),
             ("score", 1.0, KC.check_bound(got[:, 4:], dec["score"], dec["e_score"], "score"))]
    _stats("detect_decode", case["id"], stats)


@pytest.mark.parametrize("dt,nc,ok", [("f32", 256, True), ("f32", 257, False), ("f32", 512, False), ("bf16", 512, True), ("bf16", 513, False)])
@KC.stop_after_fault
def test_detect_decode_refuses_rows_that_do_not_fit_lds(dt, nc, ok):
    """The kernel keeps 2 * 64 * (gb + gcp) * 16 bytes in LDS: 160 KB at f32 nc = 256 and 144 KB at bf16 nc = 512 fit, the next power of two
    of groups (288 KB / 272 KB) cannot be launched.  Such a call returns UPA_EINVAL before anything is launched and leaves y untouched
    (it used to pass an `nc <= 512` check and fail in the launch); the largest accepted rows are correct."""
    L = KC.env()[1]
    dtype = torch.float32 if dt == "f32" else torch.bfloat16
    bl, cl, dec, _ = D.decode_reference(dt, "random", nc, (1, 3, 5))
    rc, y = _run_decode(bl, cl, dtype, nc)
    if not ok:
        assert rc == L.UPA_EINVAL, rc
        assert b"LDS" in KC.env()[2].upa_last_error()
        assert bool(torch.isnan(y).all()), "a refused call wrote to y"
        return
    L.check(rc, "detect_decode")
    got = _level(y, 1, 15, slice(0, 4 + nc))
    KC.check_bound(got[:, :4], dec["box"], dec["e_box"], "box")
    KC.check_bound(got[:, 4:], dec["score"], dec["e_score"], "score")


# ---------------------------------------------------------------------------------------------------------------------
# upa_detect_tail
# ---------------------------------------------------------------------------------------------------------------------
def _run_tail(r, nc, cout, shape, keys_only, keep_raw):
    from ultralytics_pro_amd.engine import runtime as R
    from ultralytics_pro_amd.nn.modules.conv import PackedConv
    DEV, L, lib, st = KC.env()
    n, h, w = shape
    y, keys, a_total = _outputs(n, nc, h * w)
    raws = []
    with R.use_opts(keys_only=keys_only):
        for kind, x, wt, bias, co in ((1, r["xb"], r["wb"], r["bb"], 64), (2, r["xc"], r["wc"], r["bc"], cout)):
            pk = PackedConv(wt, bias, 1, DEV, torch.bfloat16, False)
            xbuf, vx = _slice(x, torch.bfloat16)
            raw = KC.out_buf((n, h, w), co + 16, torch.bfloat16, 1)  # the raw map: channels [8, 8 + co) of rows 24 elements wider
            rv = R.view_of(raw.permute(0, 3, 1, 2)[:n, 8:8 + co])
            assert vx.ld > vx.c and rv.ld > co
            rc = lib.upa_detect_tail(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, pk.w.data_ptr(), pk.bias.data_ptr(), co, kind, nc, 16.0, y.data_ptr(), a_total, A0,
                                     rv.ptr if keep_raw else None, rv.ld if keep_raw else 0, keys.data_ptr() if kind == 2 else None, L.UPA_BF16,
                                     R.opts_ptr(), st)
            assert rc != L.UPA_EUNSUPPORTED, f"upa_detect_tail refused kind {kind}, cout {co}"
            L.check(rc, "detect_tail")
            raws.append(raw)
    torch.cuda.synchronize()
    return y.cpu(), keys.cpu(), raws[0].cpu(), raws[1].cpu()


@pytest.mark.parametrize("case", D.TAIL_CASES, ids=[c["id"] for c in D.TAIL_CASES])
@KC.stop_after_fault
def test_detect_tail_vs_f64(case):
    """cout 8 .. 128: launch_c1_ntw<1..8, 2> (class) and <4, 1> (box).  Per (keys_only, raw maps) combination: (1) boxes and scores inside
    the reference's bound; (2) every key is the first maximum of the scores the kernel wrote, its class the reference's wherever that is
    decided - on `built` every anchor: the constructed ties, the saturated and the pad-trap pixels included; (3) with keys_only the keys are
    the same bits and the class rows untouched - unless raw maps are requested (conv1x1.hip:484), then the rows are written as before;
    (4) the raw maps are rn_bf16 of the reference logits inside the stage's bound, bit-equal where it is 0 (`built`: everywhere)."""
    nc, cout, shape, fam = case["nc"], case["cout"], case["shape"], case["family"]
    n, h, w = shape
    hw = h * w
    r = D.tail_reference(nc, cout, fam, shape)
    dec = r["dec"]
    if fam == "built":
        want, decided = D.built_answer(r["scene"], dec)
    else:
        want, decided = D.margin_decided(dec["score"], dec["e_score"])
    stats = []
    ref_keys = None
    for keep_raw in (False, True):
        for keys_only in (0, 1):
            tag = f"keys_only={keys_only} raw={int(keep_raw)}"
            y, keys, raw_b, raw_c = KC.twice(lambda: _run_tail(r, nc, cout, shape, keys_only, keep_raw), tag)
            rows_off = bool(keys_only and not keep_raw)
            got = _level(y, n, hw, slice(0, 4) if rows_off else slice(0, 4 + nc))
            stats.append((f"box {tag}", 1.0, KC.check_bound(got[:, :4], dec["box"], dec["e_box"], f"box {tag}")))
            kscore, kcls = _keys(keys, n, hw, nc)
            if not rows_off:
                stats.append((f"score {tag}", 1.0, KC.check_bound(got[:, 4:], dec["score"], dec["e_score"], f"score {tag}")))
                best, arg = y[:n, 4:, A0:A0 + hw].max(1)  # torch.max: the first maximum
                assert torch.equal(kscore, best) and torch.equal(kcls, arg), f"{tag}: a key is not the first maximum of the scores written"
            if ref_keys is None:
                ref_keys = keys
            assert torch.equal(keys, ref_keys), f"{tag}: the keys differ from those written next to the score rows"
            assert bool((kcls == want)[decided].all()), f"{tag}: best class differs where the reference decides it"
            for raw, (t, e), co, nm in ((raw_b, r["raw_b"], 64, "raw box"), (raw_c, r["raw_c"], cout, "raw class")):
                if keep_raw:
                    g = KC.payload(raw, n, co, nm, offset=8).permute(0, 3, 1, 2).to(torch.float64)
                    stats.append((f"{nm} {tag}", float((e == 0).float().mean()), KC.check_bound(g, t, e, nm, exact_where_zero=True)))
                else:
                    assert bool(torch.isnan(raw.float()).all()), f"{tag}: raw maps written though none were requested"
    stats.append(("key class decided", float(decided.float().mean()), 0.0))
    _stats("detect_tail", case["id"], stats)


# ---------------------------------------------------------------------------------------------------------------------
# upa_detect_branch_tail, upa_detect_branch_tail_group, upa_detect_head_tails (csrc/conv_big.hip, TAIL 1 / 2)
# ---------------------------------------------------------------------------------------------------------------------
def _pack_branch(kind, c, x, c3, tail):
    """Device operands of one branch tail -> (whole input buffer, its slice, packed 3x3 (c -> CP), packed tail weight, tail bias)."""
    from ultralytics_pro_amd.nn.modules.conv import PackedConv
    DEV, L, lib, _ = KC.env()
    cp = D.branch_cp(kind, c)
    (w3, b3), (wt, bt) = c3, tail
    pk3 = PackedConv(torch.cat([w3, torch.zeros(cp - c, c, 3, 3)]), torch.cat([b3, torch.zeros(cp - c)]), 3, DEV, torch.bfloat16, False)
    full = torch.zeros(cp, cp)
    full[:wt.shape[0], :c] = wt.reshape(wt.shape[0], c)
    bias = torch.zeros(cp)
    bias[:bt.shape[0]] = bt
    host = torch.empty(lib.upa_tail_packed_weight_bytes(cp, cp), dtype=torch.uint8)
    L.check(lib.upa_pack_tail_weight(full.data_ptr(), cp, cp, host.data_ptr()), "pack_tail_weight")
    xbuf, vx = _slice(x, torch.bfloat16)
    return xbuf, vx, pk3, host.to(DEV), bias.to(DEV)


def _check_level(y, keys, n, hw, nc, a0, dec, want, decided, keys_only, ref_keys, tag, stats):
    """Checks 1 - 3 on one level [a0, a0 + hw) of y / keys (already asserted untouched elsewhere by the caller)."""
    lvl = slice(a0, a0 + hw)
    stats.append((f"box {tag}", 1.0, KC.check_bound(y[:n, :4, lvl].to(torch.float64), dec["box"], dec["e_box"], f"box {tag}")))
    kb = keys[:n, lvl].contiguous().numpy().view(np.uint64)
    kscore = torch.from_numpy((~(kb >> np.uint64(32)) & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32))
    kcls = torch.from_numpy((kb & np.uint64(0xFFFFFFFF)).astype(np.int64) - np.arange(a0, a0 + hw, dtype=np.int64)[None, :] * nc)
    assert bool(((kcls >= 0) & (kcls < nc)).all()), f"{tag}: a key names a class outside [0, nc) or another anchor"
    if keys_only:
        assert bool(torch.isnan(y[:n, 4:, lvl]).all()), f"{tag}: keys-only: the class rows must stay untouched"
        assert torch.equal(keys[:n, lvl], ref_keys[:n, lvl]), f"{tag}: the keys differ from those written next to the score rows"
    else:
        stats.append((f"score {tag}", 1.0, KC.check_bound(y[:n, 4:, lvl].to(torch.float64), dec["score"], dec["e_score"], f"score {tag}")))
        best, arg = y[:n, 4:, lvl].max(1)
        assert torch.equal(kscore, best) and torch.equal(kcls, arg), f"{tag}: a key is not the first maximum of the scores written"
    assert bool((kcls == want)[decided].all()), f"{tag}: best class differs where the reference decides it"


def _run_branch(r, c, nc, shape, bm, keys_only):
    from ultralytics_pro_amd.engine import runtime as R
    DEV, L, lib, st = KC.env()
    n, h, w = shape
    y, keys, a_total = _outputs(n, nc, h * w)
    keep = []
    with R.use_opts(keys_only=keys_only, branch_tail_bm=bm):
        for kind, name, ch in ((1, "box", 64), (2, "cls", c)):
            ops = _pack_branch(kind, ch, *r[name])
            keep.append(ops)
            _, vx, pk3, wt, bt = ops
            assert vx.ld > vx.c
            rc = lib.upa_detect_branch_tail(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, pk3.w.data_ptr(), pk3.bias.data_ptr(), wt.data_ptr(), bt.data_ptr(), kind, nc,
                                            16.0, y.data_ptr(), a_total, A0, keys.data_ptr() if kind == 2 else None, L.UPA_BF16, R.opts_ptr(), st)
            assert rc != L.UPA_EUNSUPPORTED, f"upa_detect_branch_tail refused kind {kind}, c {ch}, bm {bm}"
            L.check(rc, "detect_branch_tail")
    torch.cuda.synchronize()
    return y.cpu(), keys.cpu()


@pytest.mark.parametrize("case", D.BRANCH_CASES, ids=[c["id"] for c in D.BRANCH_CASES])
@KC.stop_after_fault
def test_detect_branch_tail_vs_f64(case):
    """TAIL 1 (box, 4 tiles) and TAIL 2 (class: c = 80 the 5-tile form with its 16-wide last k-step, c = 64 / 96 the 6-tile form), each on the
    128- and the 256-pixel workgroup through `branch_tail_bm`, against 3x3 + SiLU -> bf16 -> 1x1 in float64 with the chain's bounds; checks
    1 - 3 as for the 1x1 tail.  `twins`: identical weight rows tie the best class in one lane, across lane rows and across n-tiles, pairs
    2^-14 / 2^-13 apart sit on either side of the keys_only gap, three +20 rows score 1.0f on the dark columns, and with nc < CP the pad
    channels' 0 is the largest logit of lit anchors."""
    c, nc, shape, bm, fam = case["c"], case["nc"], case["shape"], case["bm"], case["family"]
    n, h, w = shape
    r = D.branch_reference(c, nc, fam, shape)
    want, decided = D.branch_answer(r, fam)
    stats, ref_keys = [], None
    for keys_only in (0, 1):
        tag = f"keys_only={keys_only}"
        y, keys = KC.twice(lambda: _run_branch(r, c, nc, shape, bm, keys_only), tag)
        _level(y, n, h * w, slice(0, 4) if keys_only else slice(0, 4 + nc))
        _keys(keys, n, h * w, nc)
        ref_keys = keys if ref_keys is None else ref_keys
        _check_level(y, keys, n, h * w, nc, A0, r["dec"], want, decided, keys_only, ref_keys, tag, stats)
    stats.append(("key class decided", float(decided.float().mean()), 0.0))
    _stats("detect_branch_tail", case["id"], stats)


def _run_group(refs, entry, no_group, keys_only, nc=80):
    import ctypes as C
    from ultralytics_pro_amd.engine import runtime as R
    DEV, L, lib, st = KC.env()
    a0s, tot = [], A0
    for (n, h, w) in D.GROUP_LEVELS:
        a0s.append(tot)
        tot += h * w + 3  # (three untouched anchors between the levels)
    tot += EXTRA
    y = torch.full((2, 4 + nc, tot), NAN, device=DEV)
    keys = torch.full((2, tot), -1, dtype=torch.int64, device=DEV)
    keep, lvs = [], {}
    for kind, name, ch in ((1, "box", 64), (2, "cls", 80)):
        lv = (L.BranchLevel * 3)()
        for j, r in enumerate(refs):
            ops = _pack_branch(kind, ch, *r[name])
            keep.append(ops)
            _, vx, pk3, wt, bt = ops
            lv[j] = L.BranchLevel(vx.ptr, vx.n, vx.h, vx.w, vx.c, vx.ld, pk3.w.data_ptr(), pk3.bias.data_ptr(), wt.data_ptr(), bt.data_ptr(), 16.0, a0s[j])
        lvs[kind] = lv
    with R.use_opts(keys_only=keys_only, no_group=no_group):
        if entry == "head_tails":
            rc = lib.upa_detect_head_tails(C.cast(lvs[1], C.c_void_p), C.cast(lvs[2], C.c_void_p), 3, nc, y.data_ptr(), tot, keys.data_ptr(), L.UPA_BF16, R.opts_ptr(), st)
            assert rc != L.UPA_EUNSUPPORTED
            L.check(rc, "head_tails")
        else:
            for kind in (1, 2):
                rc = lib.upa_detect_branch_tail_group(C.cast(lvs[kind], C.c_void_p), 3, kind, nc, y.data_ptr(), tot, keys.data_ptr() if kind == 2 else None,
                                                      L.UPA_BF16, R.opts_ptr(), st)
                assert rc != L.UPA_EUNSUPPORTED
                L.check(rc, "branch_tail_group")
    torch.cuda.synchronize()
    return y.cpu(), keys.cpu(), torch.tensor(a0s)


@pytest.mark.parametrize("case", D.GROUP_CASES, ids=[c["id"] for c in D.GROUP_CASES])
@KC.stop_after_fault
def test_detect_grouped_tails_vs_f64(case):
    """Three levels (16 x 16, 8 x 8, 4 x 4; nc = 80, `twins`) in one call: `upa_detect_head_tails` (the mix grids) and
    `upa_detect_branch_tail_group` with no_group 0 (pairs) and 2 (threes), under checks 1 - 3 per level; the anchors between the levels, in
    front of the first, behind the last and the spare image keep their fill.  (The grids themselves are held bit-equal to single launches
    at full size by tests/test_hip_ops.py.)"""
    nc = 80
    refs = [D.branch_reference(80, nc, "twins", shape, li) for li, shape in enumerate(D.GROUP_LEVELS)]
    stats, ref_keys = [], None
    for keys_only in (0, 1):
        tag = f"keys_only={keys_only}"
        y, keys, a0s = KC.twice(lambda: _run_group(refs, case["entry"], case["no_group"], keys_only), tag)
        inside = torch.zeros(y.shape[2], dtype=torch.bool)
        for a0, (n, h, w) in zip(a0s.tolist(), D.GROUP_LEVELS):
            inside[a0:a0 + h * w] = True
        assert bool(torch.isnan(y[1]).all()) and bool(torch.isnan(y[:, :, ~inside]).all()), f"{tag}: wrote outside the levels"
        assert bool((keys[1] == -1).all()) and bool((keys[:, ~inside] == -1).all()), f"{tag}: keys outside the levels"
        ref_keys = keys if ref_keys is None else ref_keys
        for li, (r, a0, (n, h, w)) in enumerate(zip(refs, a0s.tolist(), D.GROUP_LEVELS)):
            want, decided = D.branch_answer(r, "twins")
            _check_level(y, keys, n, h * w, nc, a0, r["dec"], want, decided, keys_only, ref_keys, f"level {li} {tag}", stats)
    _stats(case["entry"], case["id"], stats)
