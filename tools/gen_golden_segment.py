"""Generate the segmentation fixtures under tests/golden/ by running the IMPORTED REFERENCE (via oracle/ref_shim.py, as
tools/gen_golden_yolo11.py does) on procedural weights and inputs, and cross-check the CPU oracle tests/segment_oracle.py against it.

Run on a machine that has the reference checkout:   python -m tools.gen_golden_segment
Outputs (data only):
  tests/golden/builder_yolov{8,11}n-seg.json        layer table / save list / strides / parameter total / state_dict keys + shapes
  tests/golden/ops_segment.npz                      ConvTranspose2d, Proto, Segment (legacy and DWConv class branch) on three small
                                                    maps, the mask cases of segment_oracle.mask_cases() (+ the small-n CPU branch)
  tests/golden/e2e_yolov{8,11}n-seg[_smooth].npz    B = 2 at 640 x 640: sampled head rows, (n, 6 + nm) NMS rows, packed masks
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
GOLD = ROOT / "tests" / "golden"

from oracle.ref_shim import import_reference  # noqa: E402
from tests import segment_oracle as S  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

REF_YAML = {"yolov8n-seg": "/root/reference/ultralytics/cfg/models/v8/Segment/yolov8n-seg.yaml",
            "yolov11n-seg": "/root/reference/ultralytics/cfg/models/v11/Segment/yolov11n-seg.yaml"}
MASK_INSTANCES = 3  # full-resolution masks stored per image


def maxdiff(a, b):
    return float((a.float() - b.float()).abs().max()) if a.numel() else 0.0


def bn_fix(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eps, mod.momentum = 1e-3, 0.03
    return m.eval()


def layer_table(model):
    return [dict(i=m.i, f=m.f, type=m.type.split(".")[-1], np=int(sum(p.numel() for p in m.parameters()))) for m in model.model]


def _ref_model(rt, name):
    src = Path(REF_YAML[name])
    import yaml
    d = yaml.safe_load((src.parent / src.name.replace("n-seg", "-seg")).read_text())
    d["scale"] = "n"
    return rt.SegmentationModel(d, ch=3, nc=80, verbose=False)


def builder_tables(rt):
    for name in REF_YAML:
        ref = _ref_model(rt, name)
        mine = S.SegmentationModel(name + ".yaml")
        rsd, msd = ref.state_dict(), mine.state_dict()
        assert list(rsd) == list(msd) and all(tuple(rsd[k].shape) == tuple(msd[k].shape) for k in rsd), f"{name}: state_dict differs"
        assert layer_table(ref)[:-1] == layer_table(mine)[:-1], f"{name}: layer tables differ"
        assert list(ref.save) == list(mine.save) and torch.equal(ref.stride.float(), mine.stride.float())
        out = dict(config=name, layers=layer_table(ref), save=list(ref.save), stride=[float(x) for x in ref.stride],
                   n_params=int(sum(p.numel() for p in ref.parameters())), state_dict=[[k, list(v.shape)] for k, v in rsd.items()])
        (GOLD / f"builder_{name}.json").write_text(json.dumps(out, separators=(",", ":")))
        print(f"builder {name}: {out['n_params']} params, {len(out['layers'])} layers, save={out['save']}")


def segment_case(rt_head, legacy, ch=(64, 128, 256), fam="yolov8n-seg"):
    """A Segment head on three small maps (strides 8 / 16 / 32): (reference module, oracle module, inputs)."""
    old = rt_head.Segment.legacy
    rt_head.Segment.legacy = legacy
    try:
        r = bn_fix(rt_head.Segment(80, 32, 64, ch))
    finally:
        rt_head.Segment.legacy = old
    o = bn_fix((S.Segment if legacy else S.Segment11)(80, 32, 64, ch))
    for m in (r, o):
        m.stride = torch.tensor([8.0, 16.0, 32.0])
        m.bias_init()
        P.apply_procedural_weights(m, family=fam)
    xs = [P.uniform(f"unit:segment:{i}", (2, c, s, s), -1.0, 1.0) for i, (c, s) in enumerate(zip(ch, (16, 8, 4)))]
    return r, o, xs


def ops(rt):
    import ultralytics.nn.modules.block as rb
    import ultralytics.nn.modules.head as rh
    import ultralytics.utils.ops as rops

    G = {}
    # ConvTranspose2d(2, 2) and Proto
    ct = torch.nn.Sequential(torch.nn.ConvTranspose2d(64, 48, 2, 2, 0, bias=True))  # state_dict keys "0.weight", "0.bias"
    P.apply_procedural_weights(ct, family="yolov8n-seg")
    x = P.uniform("unit:convt", (2, 64, 7, 9), -1.0, 1.0)
    G["convt"] = ct(x).numpy()
    r, o = bn_fix(rb.Proto(64, 64, 32)), bn_fix(S.Proto(64, 64, 32))
    P.apply_procedural_weights(r, family="yolov8n-seg")
    P.apply_procedural_weights(o, family="yolov8n-seg")
    x = P.uniform("unit:proto", (2, 64, 10, 12), -1.0, 1.0)
    yr, yo = r(x), o(x)
    assert maxdiff(yr, yo) <= 1e-5, maxdiff(yr, yo)
    G["proto"] = yr.numpy()
    for legacy in (True, False):
        r, o, xs = segment_case(rh, legacy)
        assert list(r.state_dict()) == list(o.state_dict())
        yr, yo = r([t.clone() for t in xs]), o([t.clone() for t in xs])
        d = maxdiff(yr[0], yo[0])
        assert d <= 1e-4, d
        tag = "segment" if legacy else "segment11"
        G[tag] = yr[0].numpy()
        G[tag + "_proto"] = yr[1][2][0, :8].numpy()  # image 0, the first 8 protos (file size)
        print(f"op {tag}: out {tuple(yr[0].shape)} protos {tuple(yr[1][2].shape)} oracle-vs-ref {d:.2e}")
    # mask operations: the reference's functions (CPU: < 50 masks take the rounded loop) and the oracle's comparison form
    for case in S.mask_cases():
        name, key, n, nm, mhw, shape, mode = case
        protos, coef, boxes = S.mask_inputs(key, n, nm, mhw, shape)
        if mode == "native":
            ref = rops.process_mask_native(protos, coef, boxes.clone(), shape)
            auto = S.process_mask_native(protos, coef, boxes.clone(), shape)
        else:
            ref = rops.process_mask(protos, coef, boxes.clone(), shape, upsample=mode == "up")
            auto = S.process_mask(protos, coef, boxes.clone(), shape, upsample=mode == "up")
        assert torch.equal(ref, auto), f"{name}: oracle (reference branch choice) != reference"
        v, cmp = S.mask_values(case)
        G[f"mask_{name}_ref"] = np.packbits(ref.numpy().astype(bool), axis=-1)
        if n < 50:  # from 50 masks on the reference itself takes the comparison form: the two are equal (asserted)
            G[f"mask_{name}_cmp"] = np.packbits(cmp.numpy().astype(bool), axis=-1)
        else:
            assert torch.equal(ref, cmp), name
        print(f"mask {name}: {n} masks {tuple(ref.shape)}, reference branch vs comparison form differ in "
              f"{int((ref != cmp).sum())} px")
    np.savez_compressed(GOLD / "ops_segment.npz", **G)


def e2e(rt, name, smooth):
    from ultralytics.utils.nms import non_max_suppression as r_nms
    import ultralytics.utils.ops as rops

    fam = ("smooth:" if smooth else "") + name
    ref = _ref_model(rt, name)
    P.apply_procedural_weights(ref, family=fam)
    ref.eval().fuse(verbose=False)
    mine = S.SegmentationModel(name + ".yaml")
    P.apply_procedural_weights(mine, family=fam)
    mine.fuse()
    x = P.synthetic_images(2)
    with torch.no_grad():
        yr, (_, mcr, pr) = ref(x.clone())
        yo = mine(x.clone())[0]
    d = maxdiff(yr, yo)
    print(f"e2e {fam}: y {tuple(yr.shape)} protos {tuple(pr.shape)} oracle-vs-ref max|d| = {d:.3e}")
    assert d <= 2e-3, d
    A = yr.shape[-1]
    sel = np.unique(np.concatenate([np.arange(0, A, max(1, A // 256)), np.arange(64), np.arange(A - 64, A)]))
    G = {"oracle_vs_ref_maxdiff": np.array([d]), "anchor_sel": sel, "y_sel": yr[:, :, sel].numpy()}
    kw = dict(conf_thres=0.25, iou_thres=0.7, max_det=300)
    out_r = r_nms(yr.clone(), nc=80, max_time_img=1e9, **kw)
    G["predict_n"] = np.array([o.shape[0] for o in out_r])
    G["predict_rows"] = torch.cat(out_r, 0).numpy()
    masks, vals = [], []
    for i, det in enumerate(out_r):
        k = min(MASK_INSTANCES, det.shape[0])
        if k == 0:
            continue
        # the product runs on a GPU: the fixture pins crop_mask's comparison form (below 50 masks the reference's CPU call takes the
        # rounded loop, whose negative box corners wrap around); the reference's own call fixes the branch-independent part
        m_ref = rops.process_mask(pr[i], det[:k, 6:], det[:k, :4].clone(), (640, 640), upsample=True)
        assert torch.equal(m_ref, S.process_mask(pr[i], det[:k, 6:], det[:k, :4].clone(), (640, 640), upsample=True))
        m = S.process_mask(pr[i], det[:k, 6:], det[:k, :4].clone(), (640, 640), upsample=True, branch="compare")
        masks.append(np.packbits(m.numpy().astype(bool), axis=-1))
        vals.append(S.mask_logits(pr[i], det[:3, 6:]).numpy())
    filled = [int(np.unpackbits(m, axis=-1).sum()) for ms in masks for m in ms]
    # most stored masks must have pixels (an empty mask is legal - the predictor drops it - but a fixture of empty ones tests nothing)
    assert filled and 2 * sum(f > 0 for f in filled) > len(filled), f"{fam}: stored instance masks are mostly empty {filled}"
    G["mask_n"] = np.array([min(MASK_INSTANCES, o.shape[0]) for o in out_r])
    G["masks_packed"] = np.concatenate(masks, 0) if masks else np.zeros((0, 640, 80), np.uint8)
    G["mask_logits"] = np.concatenate(vals, 0) if vals else np.zeros((0, 160, 160), np.float32)
    print(f"   predict: n={[o.shape[0] for o in out_r]} rows {tuple(G['predict_rows'].shape)}; masks {G['masks_packed'].shape}")
    np.savez_compressed(GOLD / f"e2e_{name}{'_smooth' if smooth else ''}.npz", **G)


def main():
    torch.manual_seed(0)
    rt = import_reference()
    which = sys.argv[1:] or ["builder", "ops", "e2e"]
    with torch.no_grad():
        if "builder" in which:
            builder_tables(rt)
        if "ops" in which:
            ops(rt)
        if "e2e" in which:
            for name in REF_YAML:
                e2e(rt, name, smooth=False)
                e2e(rt, name, smooth=True)


if __name__ == "__main__":
    main()
