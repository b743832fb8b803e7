"""Operator library of the MI355X-native build: the class names a reference model YAML refers to
(ultralytics/nn/modules/__init__.py), each dispatching into libupa_hip.so."""

from .block import C2f, C2PSA, C3, C3k, C3k2, DFL, MHSA, SPPF, BoT3, Bottleneck, BottleneckTransformer, PSABlock, Proto, v10_Attention
from .conv import Concat, Conv, DWConv, autopad
from .head import Classify, Detect, Pose, Segment

__all__ = ("Conv", "DWConv", "Concat", "autopad", "C2f", "C3", "DFL", "SPPF", "Bottleneck", "MHSA", "BottleneckTransformer",
           "BoT3", "C3k", "C3k2", "v10_Attention", "PSABlock", "C2PSA", "Proto", "Detect", "Segment", "Pose", "Classify")
