"""CPU (-m "not gpu"): the integer checker tests/segval_ref.py against the reference goldens (tests/golden/ops_segval.npz,
map_yolov8n-seg.npz: outputs of the imported reference, tools/gen_golden_segval.py), its known answers, and SegmentationValidator's
statistics path (22-column rows, mask AP table) on one rank and across two gloo ranks."""

import socket

import numpy as np
import pytest
import torch

from tests import segval_ref as V


@pytest.fixture(scope="module")
def OPS(golden_dir):
    return np.load(golden_dir / "ops_segval.npz")


@pytest.fixture(scope="module")
def MAP(golden_dir):
    return np.load(golden_dir / "map_yolov8n-seg.npz")


def _case(G, name):
    hw = tuple(int(v) for v in G[f"{name}_hw"])
    n = hw[0] * hw[1]
    return (V.unpack_bits(G[f"{name}_pred_bits"], n), G[f"{name}_pred_cls"], V.unpack_bits(G[f"{name}_gt_bits"], n), G[f"{name}_gt_cls"])


def test_checker_equals_reference_on_the_small_cases(OPS):
    assert len(OPS["cases"]) >= 5
    hits = 0
    for name in OPS["cases"]:
        iou, tp = V.process_batch_masks(*_case(OPS, name))
        assert np.array_equal(iou, OPS[f"{name}_iou"]) and iou.dtype == np.float32, name
        assert np.array_equal(tp, OPS[f"{name}_tp"]), name
        hits += int(tp.sum())
    assert hits > 50  # the cases are not vacuous


def test_checker_and_host_ap_equal_reference_on_the_map_set(MAP):
    from ultralytics_pro_amd.utils import metrics as pmet
    tps, confs, pcls, tcls = [], [], [], []
    for i in range(4):
        det, gcls = MAP[f"det{i}"], MAP[f"gt_cls{i}"]
        gm = V.unpack_bits(MAP[f"gt_bits{i}"], 160 * 160)
        if i == 0:  # the image whose predicted masks are stored
            pm = V.unpack_bits(MAP["pred_bits0"], 160 * 160)
            k = pm.shape[0]
            iou, tp_m = V.process_batch_masks(pm, det[:k, 5], gm, gcls)
            assert np.array_equal(iou, MAP["mask_iou0"][:, :k])
            if k == det.shape[0]:
                assert np.array_equal(tp_m, MAP["tp_m0"])
        # from the stored IoU matrix: the matching alone
        assert np.array_equal(V.match_predictions(det[:, 5], gcls, MAP[f"mask_iou{i}"]), MAP[f"tp_m{i}"]), i
        tps.append(MAP[f"tp_m{i}"]); confs.append(det[:, 4]); pcls.append(det[:, 5]); tcls.append(gcls)
    tp, conf, pc, tc = (np.concatenate(v, 0) for v in (tps, confs, pcls, tcls))
    p, r, f1, ap, uc = pmet.ap_per_class(tp, conf, pc, tc)
    assert np.array_equal(ap, MAP["seg_ap"]) and np.array_equal(p, MAP["seg_p"]) and np.array_equal(r, MAP["seg_r"])
    assert np.array_equal(uc, MAP["seg_classes"])
    assert np.allclose(pmet.mean_results(p, r, ap), MAP["seg_mean"], rtol=0, atol=1e-12)
    # the fixture is not vacuous (the generator asserts the same)
    assert tp[:, 0].sum() > tp[:, 9].sum() > 0 and 0.05 < MAP["seg_mean"][3] < 0.95 and MAP["seg_mean"][3] != MAP["mean"][3]


def test_known_answers():
    a = np.zeros((1, 8, 8), bool)
    a[0, 2:5, 1:7] = True  # 18 pixels
    area = np.float32(18)
    assert V.mask_iou(a, a)[0, 0] == area / (area + np.float32(1e-7))
    b = np.zeros((1, 8, 8), bool)
    b[0, 6:, :] = True
    assert V.mask_iou(a, b)[0, 0] == 0.0
    e = np.zeros((1, 8, 8), bool)
    assert V.mask_iou(e, e)[0, 0] == 0.0 and not np.isnan(V.mask_iou(e, e)).any()  # empty vs empty: 0 / 1e-7, not NaN
    c = a.copy()
    c[0, 2, 1] = False  # 17 of 18
    assert V.mask_iou(a, c)[0, 0] == np.float32(17) / ((np.float32(18) + np.float32(17)) - np.float32(17) + np.float32(1e-7))
    # bit layout: pixel 32 w + k is bit k of word w; padding bits are zero
    m = np.zeros((1, 5, 8), bool)  # 40 pixels: 2 words, 24 padding bits
    m[0, 0, 0] = m[0, 3, 7] = m[0, 4, 7] = True  # pixels 0, 31, 39
    w = V.pack_bits(m)
    assert w.shape == (1, 2) and w.dtype == np.uint32 and w[0, 0] == (1 | (1 << 31)) and w[0, 1] == (1 << 7)
    assert np.array_equal(V.unpack_bits(w, 40).reshape(m.shape), m)
    # matching: two predictions on one label - the smaller index wins at the thresholds both reach; ties of a prediction go to the larger label
    iou = np.array([[0.91, 0.97]], np.float32)  # 1 label x 2 predictions
    tp = V.match_predictions(np.zeros(2), np.zeros(1), iou)
    assert tp[0, :9].all() and not tp[0, 9] and tp[1, 9] and not tp[1, :9].any()


def _fill(v, MAP, images):
    for i in images:
        det = torch.from_numpy(MAP[f"det{i}"])
        n = det.shape[0]
        out = torch.zeros(1, 300, 6)
        out[0, :n] = det[:, :6]
        tp, tp_m = torch.zeros(1, 300, 10, dtype=torch.uint8), torch.zeros(1, 300, 10, dtype=torch.uint8)
        tp[0, :n] = torch.from_numpy(MAP[f"tp{i}"].astype(np.uint8))
        tp_m[0, :n] = torch.from_numpy(MAP[f"tp_m{i}"].astype(np.uint8))
        gcls = torch.from_numpy(MAP[f"gt_cls{i}"])
        gt = torch.zeros(1, 64, 5)
        gt[0, : gcls.shape[0], 0] = gcls
        v.add_batch_stats(out, torch.tensor([n], dtype=torch.int32), tp, gt, torch.tensor([gcls.shape[0]], dtype=torch.int32), tp_m)


def _check_stats(st, MAP):
    assert st["tp"].shape == st["tp_m"].shape == (sum(MAP[f"det{i}"].shape[0] for i in range(4)), 10)
    assert np.array_equal(st["ap"], MAP["ap"]) and np.allclose(st["mean"], MAP["mean"], rtol=0, atol=1e-12)
    seg = st["seg"]
    assert np.array_equal(seg["ap"], MAP["seg_ap"]) and np.array_equal(seg["p"], MAP["seg_p"]) and np.array_equal(seg["r"], MAP["seg_r"])
    assert np.array_equal(seg["classes"], MAP["seg_classes"]) and np.allclose(seg["mean"], MAP["seg_mean"], rtol=0, atol=1e-12)


def test_validator_statistics_reproduce_the_reference_tables(MAP):
    """SegmentationValidator() without a model: the reference's TP matrices go in through add_batch_stats, get_stats returns the
    reference's box and mask tables (SegmentMetrics.process) - and DetectionValidator's own statistics stay 12 wide."""
    from ultralytics_pro_amd.engine.validator import DetectionValidator, SegmentationValidator
    v = SegmentationValidator()
    _fill(v, MAP, range(4))
    rows = v.local_stats()[0]
    assert rows.shape == (4, 300, 22)
    _check_stats(v.get_stats(), MAP)
    empty = SegmentationValidator()
    _fill(empty, MAP, [])
    assert DetectionValidator.stat_cols == 12 and SegmentationValidator.stat_cols == 22


def _rank(rank, world, port, golden, q):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group(backend="gloo", rank=rank, world_size=world)
    from ultralytics_pro_amd.engine.validator import SegmentationValidator
    G = np.load(golden)
    v = SegmentationValidator()
    _fill(v, G, [0] if rank == 0 else [1, 2, 3])  # uneven shards: 1 and 3 images
    st = v.get_stats()
    try:
        _check_stats(st, G)
        q.put((rank, "ok"))
    except AssertionError as e:  # report instead of hanging the other rank's barrier
        q.put((rank, f"mismatch: {e}"))
    dist.barrier()
    dist.destroy_process_group()


def test_validator_statistics_gather_two_ranks(golden_dir):
    """The 22-column statistics through `gather_stats` on two gloo ranks holding 1 and 3 images: both ranks get the reference's box
    and mask tables (`dp.gather_ragged` does not depend on the row width)."""
    import torch.multiprocessing as mp
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank, args=(r, 2, port, str(golden_dir / "map_yolov8n-seg.npz"), q)) for r in range(2)]
    for p_ in procs:
        p_.start()
    res = [q.get(timeout=240) for _ in procs]
    for p_ in procs:
        p_.join(timeout=60)
        assert p_.exitcode == 0
    assert sorted(res) == [(0, "ok"), (1, "ok")]
