"""NativeAdamW: the optimiser step as the library's own kernels (ops.adamw_step -> csrc/adamw.hip) -- torch.optim.AdamW's update with
global-norm gradient clipping, a learning-rate schedule, a non-finite guard and an EMA of the weights, all evaluated ON THE DEVICE from a
step counter that lives there: a captured training step (train.GraphedTrainStep) replays it with no host work in between.

Differences from torch, all deliberate:
  * clipping scales the gradient as it is read; ``p.grad`` keeps its unclipped values (torch.nn.utils.clip_grad_norm_ writes them back);
  * a step whose gradient norm is not finite is SKIPPED: parameters, moments, EMA and the step counter stay as they were, ``skipped`` counts;
  * one learning rate, one schedule and one step counter for all groups; a group may carry its own ``weight_decay`` and nothing else.
The state layout is torch's (``exp_avg``, ``exp_avg_sq``, ``step`` per parameter, created on the first step that sees a gradient), so a
checkpoint written by torch.optim.AdamW resumes here and the other way round; with ``ema_decay > 0`` there is an ``ema`` tensor as well."""
from __future__ import annotations

import math
from typing import Dict, List

import torch

from . import ops

_SHARED = ("lr", "betas", "eps", "max_norm", "schedule", "warmup_steps", "total_steps", "min_lr_ratio", "poly_power", "ema_decay")


def _dense(t: torch.Tensor) -> bool:
    """Every element of the storage span exactly once (contiguous in SOME dimension order)."""
    expect = 1
    for stride, size in sorted((st, s) for s, st in zip(t.shape, t.stride()) if s != 1):
        if stride != expect:
            return False
        expect *= size
    return True


def _strides(t: torch.Tensor):
    return tuple(st for s, st in zip(t.shape, t.stride()) if s != 1)


class NativeAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, max_norm: float = 0.0,
                 schedule: str = "constant", warmup_steps: int = 0, total_steps: int = 0, min_lr_ratio: float = 0.0, poly_power: float = 0.9,
                 ema_decay: float = 0.0):
        real = lambda x: isinstance(x, (int, float)) and not isinstance(x, bool) and math.isfinite(x) and x >= 0
        if not real(lr) or not real(eps) or not real(weight_decay) or not real(max_norm) or not real(poly_power):
            raise ValueError(f"NativeAdamW: lr = {lr}, eps = {eps}, weight_decay = {weight_decay}, max_norm = {max_norm}, poly_power = {poly_power} "
                             "must be finite and >= 0")
        if len(betas) != 2 or not all(real(b) and b < 1 for b in betas):
            raise ValueError(f"NativeAdamW: betas = {betas} outside [0, 1)")
        if schedule not in ops.ADAMW_SCHEDULES:
            raise ValueError(f"NativeAdamW: schedule = {schedule!r}, one of {sorted(ops.ADAMW_SCHEDULES)}")
        if not real(min_lr_ratio) or min_lr_ratio > 1 or not real(ema_decay) or ema_decay >= 1:
            raise ValueError(f"NativeAdamW: min_lr_ratio = {min_lr_ratio} outside [0, 1] or ema_decay = {ema_decay} outside [0, 1)")
        if any(isinstance(n, bool) or not isinstance(n, int) or n < 0 for n in (warmup_steps, total_steps)):
            raise ValueError(f"NativeAdamW: warmup_steps = {warmup_steps!r}, total_steps = {total_steps!r} must be integers >= 0")
        defaults = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=float(weight_decay),
                        max_norm=float(max_norm), schedule=schedule, warmup_steps=warmup_steps, total_steps=total_steps,
                        min_lr_ratio=float(min_lr_ratio), poly_power=float(poly_power), ema_decay=float(ema_decay))
        super().__init__(params, defaults)
        self._block = None                      # the device state block (ops.adamw_state): THE step counter
        self._pending_step = 0                  # a loaded counter waiting for the block
        self._ws = None
        self._shared()

    # ---- options -----------------------------------------------------------------------------------------------------------------------
    def _shared(self) -> dict:
        """The options all groups share; a group that differs in anything but weight_decay is refused."""
        first = self.param_groups[0]
        for gi, g in enumerate(self.param_groups):
            wd = g["weight_decay"]
            if isinstance(wd, bool) or not isinstance(wd, (int, float)) or not math.isfinite(wd) or wd < 0:
                raise ValueError(f"NativeAdamW: param group {gi}: weight_decay = {wd!r} must be finite and >= 0")
            for k in _SHARED:
                a, b = g[k], first[k]
                if (tuple(a) != tuple(b)) if k == "betas" else (a != b):
                    raise ValueError(f"NativeAdamW: param group {gi} sets {k} = {a!r} where group 0 has {b!r}: only weight_decay may differ between "
                                     "groups (one learning rate, schedule and step counter for all)")
        return {k: first[k] for k in _SHARED}

    def _name(self, gi: int, pi: int, p: torch.Tensor) -> str:
        names = self.param_groups[gi].get("param_names")
        return f"parameter {names[pi]!r}" if names else f"parameter {pi} of group {gi} {tuple(p.shape)}"

    # ---- the step ----------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _no_capture(what: str) -> None:
        """State is created by fills and copies; captured, they would run again on every replay and reset it."""
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"NativeAdamW: {what} would be created inside a stream capture: take one eager step first (GraphedTrainStep's "
                               "warm-up does), as with any capturable optimiser")

    def _state_block(self, device) -> torch.Tensor:
        if self._block is None or self._block.device != device:
            self._no_capture("the step counter")
            self._block = ops.adamw_state(device)
            self._block[0] = self._pending_step
        return self._block

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        opt = self._shared()
        ema_on = opt["ema_decay"] > 0
        rows: List[List[int]] = [[], [], [], [], []]
        counts: List[int] = []
        decays: List[float] = []
        dev = None
        for gi, group in enumerate(self.param_groups):
            for pi, p in enumerate(group["params"]):
                g = p.grad
                if g is None or p.numel() == 0:
                    continue
                if not p.is_cuda or not g.is_cuda or p.dtype != torch.float32 or g.dtype != torch.float32 or g.is_sparse:
                    raise RuntimeError(f"NativeAdamW: {self._name(gi, pi, p)} and its gradient must be dense fp32 tensors on the GPU "
                                       f"(parameter {p.dtype} on {p.device}, gradient {g.dtype} on {g.device}): there is no other path")
                if dev is None:
                    dev = p.device
                if p.device != dev or g.device != dev:
                    raise RuntimeError(f"NativeAdamW: {self._name(gi, pi, p)} is on {p.device}, its gradient on {g.device}, the others on {dev}")
                if not _dense(p):
                    raise RuntimeError(f"NativeAdamW: {self._name(gi, pi, p)} is not dense (strides {tuple(p.stride())})")
                st = self.state[p]
                if "exp_avg" not in st:         # (as torch: created on the first step that sees a gradient)
                    self._no_capture(f"the moments of {self._name(gi, pi, p)}")
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                if ema_on and "ema" not in st:
                    self._no_capture(f"the EMA copy of {self._name(gi, pi, p)}")
                    st["ema"] = p.detach().clone(memory_format=torch.preserve_format)
                others = [("gradient", g), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"])] + ([("ema", st["ema"])] if ema_on else [])
                for what, t in others:
                    if t.shape != p.shape or _strides(t) != _strides(p) or t.dtype != torch.float32 or t.device != dev:
                        raise RuntimeError(f"NativeAdamW: {self._name(gi, pi, p)}: its {what} ({t.dtype}, {tuple(t.shape)}, strides {tuple(t.stride())}, "
                                           f"{t.device}) does not share the parameter's layout (strides {tuple(p.stride())}): elements are paired "
                                           "by address")
                rows[0].append(p.data_ptr()); rows[1].append(g.data_ptr())
                rows[2].append(st["exp_avg"].data_ptr()); rows[3].append(st["exp_avg_sq"].data_ptr())
                rows[4].append(st["ema"].data_ptr() if ema_on else 0)
                counts.append(p.numel()); decays.append(float(group["weight_decay"]))
        if not counts:
            return loss
        total = sum(counts)
        block = self._state_block(dev)
        need = ops._bytes("gdkvm_adamw_workspace_bytes", dev, len(counts), total)
        if self._ws is None or self._ws.device != dev or self._ws.numel() < need:
            self._ws = ops.adamw_workspace(dev, len(counts), total)
        ops.adamw_step(torch.tensor(rows, dtype=torch.int64), torch.tensor(counts, dtype=torch.int64), torch.tensor(decays, dtype=torch.float32),
                       block, self._ws, **opt)
        return loss

    # ---- what the host may read --------------------------------------------------------------------------------------------------------
    def stats(self) -> Dict[str, float]:
        """{"step", "skipped", "grad_norm", "clip_coef", "lr"} of the last step, in one synchronising read of the state block."""
        if self._block is None:
            return {"step": self._pending_step, "skipped": 0, "grad_norm": 0.0, "clip_coef": 1.0, "lr": 0.0}
        host = self._block.cpu()
        f = host.view(torch.float64)
        return {"step": int(host[0]), "skipped": int(host[1]), "grad_norm": float(f[2]), "clip_coef": float(f[3]), "lr": float(f[4])}

    def ema_state_dict(self, model: torch.nn.Module) -> dict:
        """model.state_dict() with every trainable parameter that has an EMA copy replaced by it (buffers as they are)."""
        if not self._shared()["ema_decay"] > 0:
            raise RuntimeError("NativeAdamW.ema_state_dict: ema_decay is 0, there are no averaged weights")
        sd = model.state_dict()
        for name, p in model.named_parameters():
            st = self.state.get(p)
            if st is not None and "ema" in st and name in sd:
                sd[name] = st["ema"].detach().clone(memory_format=torch.preserve_format)
        return sd

    # ---- checkpoints -------------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        """torch's layout; the device counter is reported as every parameter's ``step``."""
        sd = super().state_dict()
        step = float(self.stats()["step"])
        for st in sd["state"].values():
            if "exp_avg" in st:
                st["step"] = torch.tensor(step)
        return sd

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        for g in self.param_groups:             # (a checkpoint of torch.optim.AdamW carries torch's group options and none of these)
            for k in [k for k in g if k not in self.defaults and k not in ("params", "param_names")]:
                del g[k]
            for k, v in self.defaults.items():
                g.setdefault(k, v)
        self._shared()
        steps = {int(float(st["step"])) for st in self.state.values() if "step" in st}
        if len(steps) > 1:
            raise ValueError(f"NativeAdamW.load_state_dict: the parameters' step counts differ ({sorted(steps)}): there is one counter for all")
        self._pending_step = steps.pop() if steps else 0
        if self._block is not None:
            self._block[0] = self._pending_step
            self._block[1] = 0
