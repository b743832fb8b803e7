"""Training step of the detection model on the HIP path (BASELINE config 3).

Mirrors the reference's step - forward in train mode, `v8DetectionLoss`, `loss.sum() * world_size`, backward, gradient
all-reduce, `optimizer_step` = clip_grad_norm_(10) + SGD(nesterov) + EMA (ultralytics/engine/trainer.py:416-432,
:674-682, :891-950; utils/torch_utils.py:606-650; utils/loss.py:415-528) - without torch autograd: every layer has an
explicit forward that keeps what its explicit backward needs, all of it upa_* kernels (include/upa.h, "training step").
torch is used for memory, streams, views and torch.distributed (the gradient all-reduce over RCCL).

This module is the public face of the package `engine/train/` and holds re-exports only:
  train/trainer.py  `DetectionTrainer`, `ClassificationTrainer` (tail `ClassifyT`, fused cross-entropy), `SegmentationTrainer` (tail
                    `SegmentT`, upa_mask_loss), `PoseTrainer` (tail `PoseT`, upa_kpt_loss): flat f32 parameter buffers, the graph walk, `optimizer=` SGD / Adam / AdamW / auto
  train/layers.py   the differentiable module set: yolov8's (Conv, C2f, Bottleneck, SPPF, nn.Upsample), yolov5's 6x6 stem and bare C3,
                    YOLO11's C3k2 and the depthwise `DWConvT` of its Detect head (trains with `yolo11=True` only), Proto
                    (`ConvTransposeT`), `PadConvT` (a conv whose channels are no 16-byte multiple, on padded staging); other modules raise
  train/attention.py  BoT3 = `MHSAT` (yolov5-BoT3) and C2PSA = `AttentionT` (YOLO11)
  train/heads.py    `DetectT`, `SegmentT`, `PoseT`, `ClassifyT`: the tails that own the loss
  train/targets.py  `pack_targets`, `pack_mask_ids`, `pack_keypoints`, `pack_cls_targets` (host only)
  train/optim.py    `GradScaler`, `resolve_optimizer`, `HYP`, `OPTIMIZERS`, `SCHED`
  train/graph.py    `_Node`, `plan_concats`
  train/ctx.py      `_Ctx`, the buffer helpers, `PinnedRing`
"""

import ctypes as C  # noqa: F401

from .train.ctx import PinnedRing, _Ctx, _new, _s, add_into, copy_into  # noqa: F401
from .train.graph import _Node, plan_concats  # noqa: F401
from .train.heads import ClassifyT, DetectT, PoseT, SegmentT  # noqa: F401
from .train.attention import MHSA_HEAD_DIMS, AttentionT, BoT3T, BottleneckTransformerT, C2PSAT, MHSAT, PSABlockT  # noqa: F401
from .train.layers import BottleneckT, C2fT, C3k2T, C3T, ConvT, ConvTransposeT, DWConvT, PadConvT, ProtoT, SPPFT, UpsampleT  # noqa: F401
from .train.optim import HYP, OPTIMIZERS, SCHED, GradScaler, _head_nc, resolve_optimizer  # noqa: F401
from .train.targets import (MASK_ID_MAX, MAX_GT, MAX_GT_CAP, _pixel_boxes, pack_cls_targets, pack_keypoints,  # noqa: F401
                            pack_mask_ids, pack_targets)
from .train.trainer import ClassificationTrainer, DetectionTrainer, PoseTrainer, SegmentationTrainer  # noqa: F401
