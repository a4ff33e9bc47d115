"""The definition of the native optimiser step (include/gdkvm.h, gdkvm_adamw_step) restated in float64 torch on the CPU: AdamW with decoupled
weight decay, global-norm clipping, the learning-rate schedule, the non-finite guard and the EMA.  Test infrastructure only."""
import math

import torch


def schedule_lr(t: int, lr: float, schedule: str = "constant", warmup_steps: int = 0, total_steps: int = 0, min_lr_ratio: float = 0.0,
                poly_power: float = 0.9) -> float:
    """lr(t) for the step that brings the counter to t (t = 1 is the first step)."""
    W, N, r = warmup_steps, total_steps, min_lr_ratio
    if t <= W:
        return lr * t / W
    if schedule == "constant":
        return lr
    s = min(1.0, (t - W) / max(1, N - W))
    if schedule == "cosine":
        return lr * (r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * s)))
    if schedule == "poly":
        return lr * (r + (1.0 - r) * (1.0 - s) ** poly_power)
    raise ValueError(schedule)


def clip_coef(norm: float, max_norm: float) -> float:
    return min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0


def adamw_reference(params, grads_per_step, *, lr, betas=(0.9, 0.999), eps=1e-8, weight_decays=None, max_norm=0.0, schedule="constant",
                    warmup_steps=0, total_steps=0, min_lr_ratio=0.0, poly_power=0.9, ema_decay=0.0, step=0, exp_avg=None, exp_avg_sq=None,
                    ema=None):
    """params: list of tensors; grads_per_step: list (one per step) of lists of gradients (same shapes); weight_decays: one per tensor
    (default 0.01).  Everything is computed in float64.  Returns {"params", "exp_avg", "exp_avg_sq", "ema" (None when ema_decay == 0),
    "step", "skipped", "steps": [(norm, coef, lr, applied), ...]}; a step whose squared norm is not finite changes nothing."""
    f64 = lambda ts: [t.detach().to("cpu", torch.float64).clone() for t in ts]
    p = f64(params)
    m = f64(exp_avg) if exp_avg is not None else [torch.zeros_like(x) for x in p]
    v = f64(exp_avg_sq) if exp_avg_sq is not None else [torch.zeros_like(x) for x in p]
    e = None if not ema_decay > 0 else (f64(ema) if ema is not None else [x.clone() for x in p])
    wds = [0.01] * len(p) if weight_decays is None else list(weight_decays)
    b1, b2 = betas
    t, skipped, log = int(step), 0, []
    for grads in grads_per_step:
        g = f64(grads)
        total = sum(float((x * x).sum()) for x in g)
        norm = math.sqrt(total) if total >= 0 else float("nan")
        if not math.isfinite(total):
            skipped += 1
            log.append((norm, 0.0, None, False))
            continue
        t += 1
        coef = clip_coef(norm, max_norm)
        lr_t = schedule_lr(t, lr, schedule, warmup_steps, total_steps, min_lr_ratio, poly_power)
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
        for i in range(len(p)):
            gi = coef * g[i]
            p[i] = p[i] * (1.0 - lr_t * wds[i])
            m[i] = b1 * m[i] + (1.0 - b1) * gi
            v[i] = b2 * v[i] + (1.0 - b2) * gi * gi
            p[i] = p[i] - (lr_t / bc1) * m[i] / (v[i].sqrt() / math.sqrt(bc2) + eps)
            if e is not None:
                e[i] = ema_decay * e[i] + (1.0 - ema_decay) * p[i]
        log.append((norm, coef, lr_t, True))
    return {"params": p, "exp_avg": m, "exp_avg_sq": v, "ema": e, "step": t, "skipped": skipped, "steps": log}


def torch_adamw_run(params, grads_per_step, *, dtype, lr, betas=(0.9, 0.999), eps=1e-8, weight_decays=None, max_norm=0.0, lrs=None, ema_decay=0.0):
    """torch.optim.AdamW (one group per tensor, so that each has its own decay) preceded by clip_grad_norm_ when max_norm > 0, on CPU copies
    of the inputs in `dtype`; the learning rate is `lr`, or lrs[k] in step k (the schedule evaluated by the caller); with ema_decay > 0 an EMA of the parameters is kept in `dtype` beside them.
    Returns (parameters, optimiser, EMA copies or None)."""
    ps = [torch.nn.Parameter(t.detach().to("cpu", dtype).clone()) for t in params]
    wds = [0.01] * len(ps) if weight_decays is None else list(weight_decays)
    opt = torch.optim.AdamW([{"params": [q], "weight_decay": wd} for q, wd in zip(ps, wds)], lr=lr, betas=betas, eps=eps)
    ema = [q.detach().clone() for q in ps] if ema_decay > 0 else None
    for k, grads in enumerate(grads_per_step):
        if lrs is not None:
            for group in opt.param_groups:
                group["lr"] = lrs[k]
        for q, g in zip(ps, grads):
            q.grad = g.detach().to("cpu", dtype).clone()
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        if ema is not None:
            ema = [ema_decay * e + (1.0 - ema_decay) * q.detach() for e, q in zip(ema, ps)]
    return ps, opt, ema
