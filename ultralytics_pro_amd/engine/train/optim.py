"""Hyper-parameter defaults, the optimizer resolver (`build_optimizer`'s choice) and the device-side AMP GradScaler."""

from __future__ import annotations

import torch

from ... import _lib as L
from ...nn.modules import head as H

HYP = dict(lr=0.01, momentum=0.9, weight_decay=5e-4, max_norm=10.0, ema_decay=0.9999, ema_tau=2000.0,
           box=7.5, cls=0.5, dfl=1.5, beta2=0.999, adam_eps=1e-8)  # (beta2, adam_eps: Adam / AdamW only; `momentum` is their beta1)
OPTIMIZERS = ("SGD", "Adam", "AdamW", "auto")  # of the reference's build_optimizer names (trainer.py:930); the others are refused
# warm-up / accumulation schedule of the reference's training loop (engine/trainer.py:337-338, 392-413, 245; cfg/default.yaml)
SCHED = dict(nbs=64, warmup_epochs=3.0, warmup_momentum=0.8, warmup_bias_lr=0.1, lrf=0.01, epochs=100)


class GradScaler:
    """`torch.amp.GradScaler("cuda", enabled=amp)` of the reference (engine/trainer.py:301-302; used at :429 scale(loss).backward(),
    :676 unscale_, :678 step, :679 update, :593 / :824-825 state_dict) with its state ON THE DEVICE: {scale, growth tracker, found_inf}.
    The loss kernels multiply their gradients by the scale (upa_detection_loss_scaled), the optimizer kernel divides it out again, clips
    on the unscaled norm and skips an overflowing step (upa_sgd_nesterov_ema_scaled), `upa_grad_scaler_update` adjusts the scale - the
    host never reads it, so a scaled step stays one hipGraph.  Defaults = torch's (init 2**16, growth 2, backoff 0.5, interval 2000).
    bf16 has f32's exponent range and needs no loss scaling; the scaler exists because the reference's AMP loop has one
    (`DetectionTrainer(..., amp_scaler=True)`)."""

    def __init__(self, device, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        self.enabled = bool(enabled)
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self.state = torch.tensor([float(init_scale), 0.0, 0.0, 0.0], dtype=torch.float32, device=device)

    def ptr(self):
        return self.state.data_ptr() if self.enabled else None

    def update(self, sumsq, stream):
        if self.enabled:
            L.check(L.lib().upa_grad_scaler_update(self.state.data_ptr(), sumsq.data_ptr(), self.growth_factor, self.backoff_factor,
                                                   self.growth_interval, stream), "grad_scaler_update")

    def get_scale(self) -> float:  # (host synchronisation: logging / tests only)
        return float(self.state[0].item()) if self.enabled else 1.0

    def carried_scale(self, after_update: bool) -> float:
        """The scale the gradients in the flat buffer were multiplied by: the current one before `update()` ran for them, the one
        `update()` saved (state[3]) after - on a step where the scale grew or backed off the two differ by that factor."""
        if not self.enabled:
            return 1.0
        return float(self.state[3 if after_update else 0].item())

    def found_inf(self) -> bool:
        return bool(self.state[2].item() != 0.0) if self.enabled else False

    def state_dict(self):
        if not self.enabled:
            return {}
        st = self.state.cpu()
        return {"scale": float(st[0]), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(st[1])}

    def load_state_dict(self, sd):
        if not self.enabled or not sd:
            return
        self.growth_factor, self.backoff_factor = float(sd["growth_factor"]), float(sd["backoff_factor"])
        self.growth_interval = int(sd["growth_interval"])
        self.state.copy_(torch.tensor([float(sd["scale"]), float(sd["_growth_tracker"]), 0.0, 0.0]))


def resolve_optimizer(name, iterations, nc):
    """`build_optimizer`'s choice (engine/trainer.py:891-950) as (name, hyp overrides, auto?): the name is case-insensitive; "auto" takes
    SGD(lr 0.01, momentum 0.9) for more than 10 000 iterations and AdamW(lr round(0.002 * 5 / (4 + nc), 6), beta1 0.9) otherwise,
    whatever `hyp` says, and forces warmup_bias_lr = 0 (the third element: `set_schedule` reads it)."""
    known = {x.lower(): x for x in OPTIMIZERS}
    got = known.get(str(name).lower())
    if got is None:
        raise L.UpaError(f"optimizer={name!r} has no fused step on HIP: supported are {', '.join(OPTIMIZERS)} (Adamax, NAdam, RAdam and "
                         "RMSProp of the reference's list are not built)")
    if got != "auto":
        return got, {}, False
    if iterations is None:
        raise L.UpaError("optimizer='auto' needs iterations= (the number of optimizer iterations of the run: auto picks SGD above 10000, "
                         "AdamW otherwise); or name one of SGD, Adam, AdamW")
    if iterations > 10000:
        return "SGD", dict(lr=0.01, momentum=0.9), True
    return "AdamW", dict(lr=round(0.002 * 5 / (4 + nc), 6), momentum=0.9), True


def _head_nc(model) -> int:
    """Number of classes of the model's head (the reference's `self.data["nc"]`)."""
    tail = model.model[-1] if hasattr(model, "model") and len(model.model) else None
    if isinstance(tail, H.Classify):
        return int(tail.linear.out_features)
    if tail is not None and hasattr(tail, "nc"):
        return int(tail.nc)
    raise L.UpaError(f"optimizer='auto' reads the number of classes from the model's head, got {type(tail).__name__}")
