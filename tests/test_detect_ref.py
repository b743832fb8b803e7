"""Pins tests/detect_ref.py on the CPU: the decode reference against the oracle's Detect._inference in float64, what every `built` and
`twins` scene claims to hold, a float32 emulation of the keys_only rule of csrc/detect_epi.h on the anchors meant for either path, and the
share of anchors whose best class the reference decides.  No GPU; the whole file runs in seconds."""

import pytest
import torch

from tests import block_ref as B
from tests import detect_ref as D
from tests.conv_ref import ACT_NONE, F64

F32 = torch.float32


def test_decode_reference_agrees_with_the_oracle_in_float64():
    """A cross-check of the reference (1e-9 relative), not a tolerance for any kernel."""
    from oracle import modules as om
    for nc, shape in ((80, (2, 5, 7)), (3, (3, 9, 11))):
        bl, cl, dec, _ = D.decode_reference("f32", "random", nc, shape)
        det = om.Detect(nc, (64,)).eval().double()
        det.stride = torch.tensor([8.0], dtype=F64)
        ref = det._inference([torch.cat([bl, cl], 1).to(F64)])
        got = torch.cat([dec["box"], dec["score"]], 1)
        assert ref.dtype == F64 and ref.shape == got.shape
        assert bool(((got - ref).abs() <= 1e-9 * ref.abs().clamp_min(1e-30)).all()), float(((got - ref).abs() / ref.abs().clamp_min(1e-30)).max())


def _built_scenes():
    out = [(c["id"], D.decode_reference(c["dtype"], "built", c["nc"], c["shape"])[3]) for c in D.DECODE_CASES if c["family"] == "built"]
    out += [(c["id"], D.tail_reference(c["nc"], c["cout"], "built", c["shape"])["scene"]) for c in D.TAIL_CASES if c["family"] == "built"]
    return out


def _flat(t, n):
    return t.reshape(n, t.shape[1], -1).permute(0, 2, 1).reshape(-1, t.shape[1])  # (pixels, channels)


def test_built_scenes_hold_what_they_claim():
    """Every item of the list, found again by a predicate on the CPU logits; every scene with at least 64 pixels holds every item its class
    count and input type allow (the bf16 decode scenes have no f32 bias: max_above_4, max_below_4 and the two gap items exist only where the
    logit is float32), each in a full 16-pixel tile and, over the case list, in a ragged last one, and the saturated classes really score 1.0f in float32."""
    seen, ragged = set(), set()
    for cid, sc in _built_scenes():
        n, h, w, nc = sc["n"], sc["h"], sc["w"], sc["nc"]
        P = n * h * w
        cl, bl = _flat(sc["cl"], n), _flat(sc["bl"], n).view(P, 4, 16)
        xc = _flat(sc["xc"], n)
        top = cl.max(1).values
        ntop = (cl == top.unsqueeze(1)).sum(1)
        srt = cl.sort(1, descending=True).values
        gap = (srt[:, 0] - srt[:, 1]) if nc >= 2 else torch.full((P,), float("inf"))
        four = torch.tensor(4.0, dtype=F32)
        pred = {
            "score_0_and_1": lambda p: D.sigmoid_f32(cl[p]).max() == 1.0 and (nc == 1 or D.sigmoid_f32(cl[p]).min() == 0.0) and cl[p].abs().max() >= 100,
            "neg_zero": lambda p: bool(((xc[p, :nc] == 0) & torch.signbit(xc[p, :nc])).any()) and top[p] == 0,
            "tie_one_lane": lambda p: ntop[p] == 2 and cl[p, 0] == top[p] and cl[p, 1] == top[p] and gap[p] == 0,
            "tie_lane_rows": lambda p: ntop[p] == 2 and cl[p, 1] == top[p] and cl[p, 4] == top[p],
            "tie_n_tiles": lambda p: ntop[p] == 2 and cl[p, 0] == top[p] and cl[p, 16] == top[p],
            "max_is_4": lambda p: top[p] == four,
            "max_above_4": lambda p: top[p] == torch.nextafter(four, torch.tensor(float("inf"))),
            "max_below_4": lambda p: top[p] == torch.nextafter(four, torch.tensor(0.0)),
            "gap_below_1e-4": lambda p: gap[p] == 2.0 ** -14 and gap[p] < 1e-4,
            "gap_above_1e-4": lambda p: gap[p] == 2.0 ** -13 and gap[p] > 1e-4,
            "saturated": lambda p: int((D.sigmoid_f32(cl[p]) == 1.0).sum()) >= 3 and len(set(cl[p][cl[p] >= 17].tolist())) >= 3
                                   and int(cl[p].argmax()) != int((cl[p] >= 17).nonzero()[0]),
            "pad_trap": lambda p: top[p] <= -3 + 2.0 ** -13 and (sc["cout"] == nc or bool((xc[p, nc:] == 0).all())),  # (-3 + a CLS_BIAS step)
            "clear": lambda p: abs(float(top[p]) - 2.0) <= 2.0 ** -13 and gap[p] > 1,
        }
        for name, at in sc["items"].items():
            if name.startswith("box_"):
                continue
            if P >= 64:
                assert at, (cid, name)
            if P >= 96:
                assert any(p // 16 < P // 16 for p in at), (cid, name, "no full tile")
            if P % 16 and any(p // 16 == P // 16 for p in at):
                ragged.add(name)
            for p in at:
                assert pred[name](p), (cid, name, p)
            if at:
                seen.add(name)
        # the box sides
        E = (torch.softmax(bl.to(F64), 2) * torch.arange(16, dtype=F64)).sum(2)
        for kind, want in (("hot0", 0.0), ("hot7", 7.0), ("hot15", 15.0), ("equal", 7.5), ("two_maxima", 5.5), ("underflow", 5.0)):
            at = sc["items"].get("box_" + kind, [])
            if P >= 64:
                assert at or kind == "underflow", (cid, kind)
            for p in at:
                assert bool(((E[p] - want).abs() < 1e-9).any()), (cid, kind, p)
            if at:
                seen.add("box_" + kind)
        if sc["items"]["box_random"]:
            seen.add("box_random")
        for p in sc["items"]["box_two_maxima"]:
            s = [q for q in range(4) if abs(float(E[p, q]) - 5.5) < 1e-9][0]
            assert bl[p, s, 2] == bl[p, s].max() and bl[p, s, 9] == bl[p, s].max()  # bins 2 and 9: lane rows 0 and 2
        for p in sc["items"].get("box_underflow", []):
            assert float(bl[p].abs().max()) >= 80
        if w > 1:
            last = [p for p in range(P) if p % w == w - 1]
            assert last and all(0.4 < float(E[p, 0] + E[p, 2]) < 0.7 for p in last)  # x2 - x1: half a pixel at column w - 1
            seen.add("box_narrow")
        for p in sc["items"]["box_sum_cancels"]:
            assert p % w == 7 and abs(float(7.5 - E[p, 0]) + float(7.5 + E[p, 2])) < 1e-9
            seen.add("box_sum_cancels")
    assert ragged >= set(D.ITEMS_CLS), set(D.ITEMS_CLS) - ragged  # over the case list every item sits in a ragged last tile too
    assert seen >= set(D.ITEMS_CLS) | {"box_" + k for k in D.ITEMS_BOX} | {"box_narrow", "box_sum_cancels"}, set(D.ITEMS_CLS) - seen


def test_identity_tail_logits_are_the_float32_sum():
    """fl32(x + bias) of the built tails lies inside the bound `B.stage` gives the same conv: the written logits are the chain's."""
    r = D.tail_reference(33, 48, "built", (3, 5, 7))
    lg, e = B.stage(r["xc"], None, r["wc"], r["bc"], 1, 1, ACT_NONE, out_dtype=F32)
    assert bool(((lg[:, :33] - r["cl"]).abs() <= e[:, :33]).all())
    assert torch.equal(r["cl"], (r["xc"] + r["bc"].view(1, -1, 1, 1))[:, :33].to(F64))


def test_keys_only_rule_in_float32_takes_the_path_each_anchor_is_meant_for():
    for cid, sc in _built_scenes():
        sure = D.keys_only_sure(sc["cl"]).flatten()
        assert torch.equal(sure, sc["fast"]), (cid, (sure != sc["fast"]).nonzero().flatten().tolist()[:8])
        if sure.numel() >= 48 and sc["nc"] >= 3:
            tiles = D.tiles_fast(sure)
            assert bool(tiles[0]) and not bool(tiles[1]) and not bool(tiles[2])   # a whole tile on the fast path ...
            assert int((~sure[16:32]).sum()) == 1 and not bool(sure[21])         # ... one unsure pixel sends its wave through the full path
            # ... and in tile 2 that pixel is the saturated one: without the `largest logit <= 4` clause the tile would take the fast path
            # and name the class of the largest logit, which is not the first of the classes that score 1.0f
            assert int((~sure[32:48]).sum()) == 1 and 37 in sc["items"]["saturated"]
            loose = D.keys_only_sure(sc["cl"], max_clause=False).flatten()
            assert bool(D.tiles_fast(loose)[2]) and not bool(D.tiles_fast(loose)[1])
            row = _flat(sc["cl"], sc["n"])[37]
            assert int(row.argmax()) != int(sc["want"][37]) and float(D.sigmoid_f32(row)[int(sc["want"][37])]) == 1.0
    # the twins: a gap of 2^-14 is unsure, 2^-13 sure, identical rows unsure
    lg = torch.full((1, 20, 1, 4), -9.0)
    lg[0, 8, 0, 0], lg[0, 9, 0, 0] = -1.0, -1.0 - 2.0 ** -14
    lg[0, 10, 0, 1], lg[0, 13, 0, 1] = -1.0, -1.0 - 2.0 ** -13
    lg[0, 2, 0, 2], lg[0, 5, 0, 2] = -1.0, -1.0
    lg[0, 6, 0, 3], lg[0, 11, 0, 3], lg[0, 17, 0, 3] = 20.0, 20.0, 20.0
    assert D.keys_only_sure(lg).flatten().tolist() == [False, True, False, False]


def test_twins_tail_rows_are_what_the_family_claims():
    g = torch.Generator().manual_seed(3)
    wt, bias = B.twins_tail(g, 20, 64)
    for members, win in B.TWIN_GROUPS:
        assert all(torch.equal(wt[m], wt[members[0]]) for m in members) and win == members[0]
        assert float(bias[members[0]]) <= -3.0 and float(bias[members[0]] - bias[members[1]]) == B.TWIN_GAPS.get(members[1], 0.0)
    lanes = [[(m % 16) // 4 for m in ms] + [m // 16 for m in ms] for ms, _ in B.TWIN_GROUPS]
    assert lanes[0] == [0, 0, 0, 0] and lanes[1][:2] == [0, 1] and lanes[2] == [0, 0, 0, 1]  # one lane; two lane rows; two n-tiles
    assert len(B.TWIN_SAT) >= 3 and all(float(bias[s]) == 20.0 for s in B.TWIN_SAT)
    rest = [c for c in range(20) if c not in B.TWIN_SAT]
    assert float(bias[rest].max()) <= -3.0
    assert D.sigmoid_f32(torch.tensor([19.0, 20.0, 21.0])).tolist() == [1.0, 1.0, 1.0]


@pytest.mark.parametrize("case", D.TAIL_CASES, ids=[c["id"] for c in D.TAIL_CASES])
def test_decided_share_of_the_tail_cases(case):
    r = D.tail_reference(case["nc"], case["cout"], case["family"], case["shape"])
    if case["family"] == "built":
        want, decided = D.built_answer(r["scene"], r["dec"])
        arg, clear = D.margin_decided(r["dec"]["score"], r["dec"]["e_score"])
        assert bool(decided.all())                       # 100 %
        assert bool((arg == want)[clear].all())          # the constructed answers are the margin rule's wherever that rule decides
    else:
        _, decided = D.margin_decided(r["dec"]["score"], r["dec"]["e_score"])
        assert float(decided.float().mean()) >= 0.9, float(decided.float().mean())
        sc = r["dec"]["score"]
        assert float(sc.min()) < 0.5 < float(sc.max())


def test_decided_share_of_the_level_stream_twins():
    assert len(B.TWINS_CASES) == 2 and sorted(B.CASES[i]["opts"]["keys_only"] for i in B.TWINS_CASES) == [0, 1]
    for ci in B.TWINS_CASES:
        _, (bl, be, cl, ce, _) = B.reference(ci, "twins")
        want, decided = B.twins_answer(cl, ce)
        assert float(decided.float().mean()) >= 0.9, float(decided.float().mean())
        assert bool((want[:, :3] == B.TWIN_SAT[0]).all()) and bool(decided[:, :3].all())


BRANCH_REFS = sorted({(c["c"], c["nc"], c["family"], c["shape"]) for c in D.BRANCH_CASES}, key=repr)


@pytest.mark.parametrize("key", BRANCH_REFS, ids=[f"{k[2]}-c{k[0]}-nc{k[1]}-{'x'.join(map(str, k[3]))}" for k in BRANCH_REFS])
def test_decided_share_of_the_branch_tail_cases(key):
    """A cap with room, not a measurement: at least 90 % of the anchors behind a 3x3 stage have a decided best class.  On `twins` the dark
    columns are saturated (the first +20 row), the lit ones go to a twin group, and on a tenth of them at least every real logit is below the 0 of a pad channel."""
    c, nc, family, shape = key
    r = D.branch_reference(c, nc, family, shape)
    want, decided = D.branch_answer(r, family)
    assert float(decided.float().mean()) >= 0.9, float(decided.float().mean())
    if family == "twins":
        n, h, w = shape
        d = B.twins_dark_cols(w)
        wd, dd = want.view(n, h, w), decided.view(n, h, w)
        assert bool((wd[:, :, :d - 1] == B.TWIN_SAT[0]).all()) and bool(dd[:, :, :d - 1].all())
        winners = torch.tensor(sorted(win for _, win in B.TWIN_GROUPS))
        assert float(torch.isin(wd[:, :, d + 1:], winners).float().mean()) >= 0.9
        assert float((r["cl"][:, :, :, d + 1:].max(1).values < 0.0).float().mean()) >= 0.1  # where a pad channel's 0 is the largest logit


def test_twin_groups_take_turns_over_the_case_list():
    """Each case has its own weights: over the list at least three of the five groups are some lit anchor's decided answer."""
    seen = set()
    for c, nc, family, shape in BRANCH_REFS:
        if family == "twins":
            want, decided = D.branch_answer(D.branch_reference(c, nc, family, shape), family)
            seen |= set(want[decided].tolist())
    assert len(seen & {win for _, win in B.TWIN_GROUPS}) >= 3 and B.TWIN_SAT[0] in seen, seen


def test_decided_share_of_the_grouped_levels():
    for li, shape in enumerate(D.GROUP_LEVELS):
        _, decided = D.branch_answer(D.branch_reference(80, 80, "twins", shape, li), "twins")
        assert float(decided.float().mean()) >= 0.9, (shape, float(decided.float().mean()))
