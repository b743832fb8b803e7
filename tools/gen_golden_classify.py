"""Generate the classification fixtures under tests/golden/ by running the IMPORTED REFERENCE (via oracle/ref_shim.py, as
tools/gen_golden_segment.py does) on procedural weights and inputs, and cross-check the CPU oracle tests/classify_oracle.py against it.

Run on a machine that has the reference checkout:   python -m tools.gen_golden_classify
Outputs (data only):
  tests/golden/builder_yolov{8,11}n-cls.json       layer table / save list / stride / parameter total / state_dict keys + shapes
  tests/golden/ops_classify.npz                    Classify (eval) on the small maps of classify_oracle.head_cases(): input, probs,
                                                   logits; a hand-made ClassifyMetrics case: top-5 lists, targets -> top1 / top5
  tests/golden/e2e_yolov{8,11}n-cls[_smooth].npz   B = 2 at 224 x 224, fused eval: probs, logits, argsort(1, descending)[:, :5]
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
from tests import classify_oracle as C  # noqa: E402
from ultralytics_pro_amd.utils import procedural as P  # noqa: E402

from oracle.ref_shim import REF_ROOT  # noqa: E402

REF_YAML = {"yolov8n-cls": REF_ROOT + "/ultralytics/cfg/models/v8/Classify/yolov8-cls.yaml",
            "yolov11n-cls": REF_ROOT + "/ultralytics/cfg/models/v11/Classify/yolov11-cls.yaml"}


def maxdiff(a, b):
    return float((a.float() - b.float()).abs().max()) if a.numel() else 0.0


def layer_table(model):
    return [dict(i=m.i, f=m.f, type=m.type.split(".")[-1], np=int(sum(p.numel() for p in m.parameters()))) for m in model.model]


def _ref_model(rt, name):
    import yaml
    d = yaml.safe_load(Path(REF_YAML[name]).read_text())
    d["scale"] = "n"
    d["yaml_file"] = name + ".yaml"
    # the reference's parse_model unpacks four values per scale (depth, width, max_channels, threshold); its v8 cls YAML lists three
    d["scales"] = {k: (list(v) + [0])[:4] for k, v in d["scales"].items()}
    return rt.ClassificationModel(d, ch=3, nc=None, verbose=False)


def builder_tables(rt):
    for name in REF_YAML:
        ref = _ref_model(rt, name)
        mine = C.ClassificationModel(name + ".yaml")
        rsd, msd = ref.state_dict(), mine.state_dict()
        assert list(rsd) == list(msd) and all(tuple(rsd[k].shape) == tuple(msd[k].shape) for k in rsd), f"{name}: state_dict differs"
        assert layer_table(ref) == layer_table(mine), f"{name}: layer tables differ"
        assert list(ref.save) == list(mine.save) and torch.equal(ref.stride.float(), mine.stride.float())
        assert ref.names == mine.names
        eps = sorted({m.eps for m in ref.modules() if isinstance(m, torch.nn.BatchNorm2d)})
        out = dict(config=name, layers=layer_table(ref), save=list(ref.save), stride=[float(x) for x in ref.stride], nc=len(ref.names),
                   bn_eps=eps, n_params=int(sum(p.numel() for p in ref.parameters())),
                   state_dict=[[k, list(v.shape)] for k, v in rsd.items()])
        (GOLD / f"builder_{name}.json").write_text(json.dumps(out, separators=(",", ":")))
        print(f"builder {name}: {out['n_params']} params, {len(out['layers'])} layers, nc={out['nc']}, bn eps {eps}")


def ops(rt):
    import ultralytics.nn.modules.head as rh
    import ultralytics.utils.metrics as rm

    G = {}
    for case in C.head_cases():
        r, x = C.head_case(case, rh.Classify)
        o, _ = C.head_case(case, C.Classify)
        assert list(r.state_dict()) == list(o.state_dict())
        (pr, zr), (po, zo) = r(x.clone()), o(x.clone())
        d = max(maxdiff(pr, po), maxdiff(zr, zo))
        assert d <= 1e-5, (case[0], d)
        G[f"{case[0]}_x"], G[f"{case[0]}_probs"], G[f"{case[0]}_logits"] = x.numpy(), pr.numpy(), zr.numpy()
        k6 = min(case[3], 6)
        s = zr.sort(1, descending=True).values[:, :k6]
        gap = float((s[:, :-1] - s[:, 1:]).min())
        assert gap >= 1e-3, (case[0], gap)  # the head tests compare top-5 index lists: they must be decidable in f32
        print(f"op classify {case[0]}: logits {tuple(zr.shape)} std {float(zr.std()):.2f} top-{k6} min gap {gap:.4f} oracle-vs-ref {d:.2e}")
    pred, targets = C.metrics_case()
    met = rm.ClassifyMetrics()
    met.process(targets, pred)
    mine = C.ClassifyMetrics()
    mine.process(targets, pred)
    assert (met.top1, met.top5) == (mine.top1, mine.top5) and met.results_dict == mine.results_dict
    G["metrics_pred"], G["metrics_targets"] = torch.cat(pred).numpy(), torch.cat(targets).numpy()
    G["metrics_split"] = np.array([p.shape[0] for p in pred])
    G["metrics_top1_top5_fitness"] = np.array([met.top1, met.top5, met.fitness], dtype=np.float64)
    G["metrics_keys"] = np.array(list(met.results_dict))
    cm = rm.ConfusionMatrix(names={i: str(i) for i in range(10)}, task="classify")
    cm.process_cls_preds(pred, targets)
    G["metrics_confusion"] = np.asarray(cm.matrix)
    print(f"metrics: top1 {met.top1:.6f} top5 {met.top5:.6f}; confusion {G['metrics_confusion'].shape}")
    np.savez_compressed(GOLD / "ops_classify.npz", **G)


def e2e(rt, name, smooth):
    fam = ("smooth:" if smooth else "") + name
    ref = _ref_model(rt, name)
    P.apply_procedural_weights(ref, family=fam)
    ref.eval().fuse(verbose=False)
    mine = C.ClassificationModel(name + ".yaml")
    P.apply_procedural_weights(mine, family=fam)
    mine.fuse()
    x = P.synthetic_images(2, h=224, w=224)
    with torch.no_grad():
        pr, zr = ref(x.clone())
        po, zo = mine(x.clone())
    d = max(maxdiff(pr, po), maxdiff(zr, zo))
    s = zr.sort(1, descending=True).values
    gap = float((s[:, :5] - s[:, 1:6]).min())
    print(f"e2e {fam}: logits {tuple(zr.shape)} std {float(zr.std(1).mean()):.2f} top-6 min gap {gap:.4f} max prob {float(pr.max()):.4f} "
          f"oracle-vs-ref max|d| = {d:.3e}")
    assert d <= 1e-3, d
    assert gap >= 1e-2 and float(pr.max()) < 0.999, "the recipe leaves an undecidable top-5 or a saturated row: retune CLS_LINEAR_GAIN"
    G = {"oracle_vs_ref_maxdiff": np.array([d]), "probs": pr.numpy(), "logits": zr.numpy(),
         "top5": pr.argsort(1, descending=True)[:, :5].numpy().astype(np.int32)}
    assert np.array_equal(G["top5"], zr.argsort(1, descending=True)[:, :5].numpy())
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
