"""The host-side pieces of the training package (ultralytics_pro_amd/engine/train): the Concat planner on hand-written node lists,
the pinned staging ring with injected allocation and events, and `engine.trainer` as a pure re-export of the submodules.  No device."""

import importlib
import subprocess
import sys
from pathlib import Path

import torch

from ultralytics_pro_amd.engine.train.ctx import PinnedRing
from ultralytics_pro_amd.engine.train.graph import plan_concats

ROOT = Path(__file__).resolve().parents[1]


# ---- 1. plan_concats: rows are (i, f, cout, can_write_in_place); a Concat is a row with a list f ----------------------------------------
def test_neck_concat_gives_both_producers_their_channel_offsets():
    """yolov8's first neck Concat: [upsample(-1), backbone layer 1] -> the upsample owns channels [0, 256), the backbone output
    [256, 384) of the 384-channel buffer."""
    rows = [(0, -1, 64, True), (1, -1, 128, True), (2, -1, 256, True),   # backbone ... SPPF
            (3, -1, 256, True),                                          # Upsample of 2
            (4, [-1, 1], 384, False),                                    # Concat
            (5, -1, 128, True), (6, [5], None, True)]                    # C2f, tail
    assert plan_concats(rows) == {3: (4, 0, 256, 384), 1: (4, 256, 128, 384)}


def test_producer_named_twice_in_one_concat_gets_no_slot():
    rows = [(0, -1, 16, True), (1, -1, 32, True), (2, [0, 1, 0], 64, False), (3, [2], None, True)]
    assert plan_concats(rows) == {1: (2, 16, 32, 64)}


def test_producer_of_two_concats_gets_its_slot_in_the_first():
    rows = [(0, -1, 16, True), (1, -1, 32, True), (2, [-1, 0], 48, False), (3, -1, 8, True), (4, [-1, 0], 24, False), (5, [4], None, True)]
    assert plan_concats(rows) == {1: (2, 0, 32, 48), 0: (2, 32, 16, 48), 3: (4, 0, 8, 24)}


def test_producer_that_cannot_write_in_place_gets_no_slot():
    """A Concat feeding a Concat (its own output is assembled, not written by a kernel with a pixel stride)."""
    rows = [(0, -1, 16, True), (1, -1, 16, True), (2, [0, 1], 32, False), (3, -1, 8, True), (4, [2, 3], 40, False), (5, [4], None, True)]
    assert plan_concats(rows) == {0: (2, 0, 16, 32), 1: (2, 16, 16, 32), 3: (4, 32, 8, 40)}


def test_producer_whose_index_is_not_its_position_gets_no_slot():
    rows = [(1, -1, 16, True), (0, -1, 16, True), (2, [0, 1], 32, False), (3, [2], None, True)]
    assert plan_concats(rows) == {}


def test_last_node_is_never_planned():
    """The tail has a list f as a Concat has: it is not planned as one, and no Concat hands it a slot."""
    rows = [(0, -1, 16, True), (1, -1, 16, True), (2, [0, 1], None, True)]
    assert plan_concats(rows) == {}
    rows = [(0, -1, 16, True), (1, [0, 2], 32, False), (2, -1, 16, True)]
    assert plan_concats(rows) == {0: (1, 0, 16, 32)}


# ---- 2. PinnedRing ---------------------------------------------------------------------------------------------------------------------
class _Event:
    log = []

    def record(self, stream):
        self.stream = stream

    def synchronize(self):
        _Event.log.append(self)


def _ring():
    made = []

    def alloc(shape, dtype):
        made.append(torch.zeros(shape, dtype=dtype))
        return made[-1]

    _Event.log = []
    return PinnedRing(slots=4, alloc=alloc, event=_Event), made


def test_ring_cycles_four_slots_and_waits_for_the_reused_one():
    ring, made = _ring()
    specs = [((2, 64, 5), torch.float32), ((2,), torch.int32)]
    got = []
    for step in range(5):
        bufs = ring.stage(specs)
        assert [tuple(b.shape) for b in bufs] == [(2, 64, 5), (2,)] and [b.dtype for b in bufs] == [torch.float32, torch.int32]
        assert len(_Event.log) == (1 if step == 4 else 0)  # only a slot that has carried a copy is waited for, before it is handed out
        got.append(bufs)
        ring.commit(f"stream{step}")
    assert len(made) == 8  # four slots of two tensors
    assert len({id(b[0]) for b in got[:4]}) == 4 and got[4][0] is got[0][0] and got[4][1] is got[0][1]
    assert _Event.log[0].stream == "stream0"


def test_ring_reallocates_only_the_slot_whose_shapes_changed():
    ring, made = _ring()
    small, big = [((2, 64, 5), torch.float32)], [((2, 128, 5), torch.float32)]
    first = [ring.stage(small)[0] for _ in range(4)]
    assert len(made) == 4
    grown = ring.stage(big)[0]                      # slot 0 again, other shape
    assert tuple(grown.shape) == (2, 128, 5) and len(made) == 5
    assert all(ring.stage(small)[0] is old for old in first[1:]) and len(made) == 5  # slots 1..3 untouched
    assert ring.stage(big)[0] is grown and len(made) == 5
    assert ring.stage(small)[0] is first[1]


# ---- 3. engine.trainer is a re-export --------------------------------------------------------------------------------------------------
HOMES = {"trainer": ["DetectionTrainer", "ClassificationTrainer", "SegmentationTrainer"],
         "layers": ["ConvT", "DWConvT", "ConvTransposeT", "UpsampleT", "BottleneckT", "C2fT", "SPPFT", "C3T", "C3k2T", "ProtoT"],
         "attention": ["MHSAT", "BottleneckTransformerT", "BoT3T", "AttentionT", "PSABlockT", "C2PSAT", "MHSA_HEAD_DIMS"],
         "heads": ["DetectT", "SegmentT", "ClassifyT"],
         "ctx": ["_Ctx", "_s", "_new", "add_into", "copy_into", "PinnedRing"],
         "targets": ["pack_targets", "pack_mask_ids", "pack_cls_targets", "_pixel_boxes", "MAX_GT", "MAX_GT_CAP", "MASK_ID_MAX"],
         "optim": ["GradScaler", "resolve_optimizer", "HYP", "OPTIMIZERS", "SCHED"],
         "graph": ["_Node", "plan_concats"]}


def test_engine_trainer_reexports_the_submodules_objects():
    import ctypes

    from ultralytics_pro_amd.engine import trainer as T
    assert T.C is ctypes
    for mod, names in HOMES.items():
        home = importlib.import_module(f"ultralytics_pro_amd.engine.train.{mod}")
        for name in names:
            assert getattr(T, name) is getattr(home, name), f"{name} is not engine.train.{mod}'s"
    # the class switches the tests flip through engine.trainer are the classes' own
    assert "fork_levels" in vars(T.DetectT) and "fused" in vars(T.DWConvT)


def test_targets_imports_without_the_library():
    code = ("import sys\n"
            "import ultralytics_pro_amd.engine.train.targets as t\n"
            "from ultralytics_pro_amd import _lib\n"
            "assert _lib._lib is None, 'the library was loaded'\n"
            "assert not [m for m in sys.modules if m.startswith('ultralytics_pro_amd.engine.') and m.split('.')[-1] in "
            "('runtime', 'layers', 'attention', 'heads', 'ctx', 'trainer')], sorted(sys.modules)\n"
            "assert t.MAX_GT == 64 and callable(t.pack_targets)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=str(ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
