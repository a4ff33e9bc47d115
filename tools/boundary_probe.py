#!/usr/bin/env python3
"""What the boundary loss costs (profiles/r14_a_boundary_loss.txt).
python3 tools/boundary_probe.py [--quick] [--no-step]

(a) At the per-GPU shape of BASELINE configs[3] (16 clips x 32 frames = 512 frames of 112 x 112, 2 classes, stride-4 logits 28 x 28, bf16) and at
    64 frames of 256 x 256 with 4 classes (the CAMUS shape): gdkvm_signed_distance over the classes of the term, gdkvm_seg_loss_boundary_fwd +
    _bwd, and gdkvm_seg_loss_fwd + _bwd of the same build on the same logits and labels.  All are called through the C symbols on
    preallocated outputs, CALLS launches back to back between ONE pair of device events, time per call = window / CALLS, the forms alternated
    window by window over four rotating inputs, median and minimum over the windows (as tools/lv_probe.py does).  Labels: one rotated ellipse
    per frame (a ventricle), nested ellipses for 4 classes; uint8.
(b) The captured training step (GraphedTrainStep, default widths, bf16 autocast, fused capturable AdamW) at boundary_weight 0.05 against
    weight 0, two models from the same seed, replays timed in alternating windows of device events."""
import math
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gdkvm_amd import ops  # noqa: E402

CALLS = 20            # launches per timed window


def ellipse_labels(F, S, C, seed):
    """uint8 [F, S, S]: class c is the part of a rotated ellipse inside the ellipse of class c - 1 (class 1 the outermost)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    out = np.zeros((F, S, S), np.uint8)
    for f in range(F):
        th = rng.uniform(-0.5, 0.5)
        la, sa = S * rng.uniform(0.22, 0.30), S * rng.uniform(0.10, 0.14)
        dx, dy = xx - S * rng.uniform(0.45, 0.55), yy - S * rng.uniform(0.45, 0.55)
        al, ac = dx * math.sin(th) + dy * math.cos(th), dx * math.cos(th) - dy * math.sin(th)
        r2 = (al / la) ** 2 + (ac / sa) ** 2
        for c in range(1, C):
            out[f][r2 <= (1.0 - (c - 1) / C) ** 2] = c
    return out


def windows(forms, reps, n_in):
    times = {name: [] for name in forms}
    for r in range(reps + 3):
        for name, fn in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn(r % n_in)
            e1.record()
            e1.synchronize()
            if r >= 3:                           # (three warm-up rounds)
                times[name].append(e0.elapsed_time(e1) * 1e3 / CALLS)
    return times


def part_a(dev, F, S, C, reps, n_in=4):
    lib = ops.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator().manual_seed(S)
    h = S // 4
    tgt = [torch.from_numpy(ellipse_labels(F, S, C, s)).to(dev) for s in range(n_in)]
    z = [(2.0 * torch.randn((F, C, h, h), generator=g)).to(dev).bfloat16() for _ in range(n_in)]
    mask = (1 << C) - 2                          # every class but 0
    sd2 = torch.empty((F, C, S, S), dtype=torch.int32, device=dev)
    sd_ws = torch.empty(max(16, int(lib.gdkvm_signed_distance_workspace_bytes(F, C, S, S))), dtype=torch.uint8, device=dev)
    ws_b = torch.empty(int(lib.gdkvm_seg_loss_boundary_workspace_bytes(C)), dtype=torch.uint8, device=dev)
    ws_p = torch.empty(int(lib.gdkvm_seg_loss_workspace_bytes(C)), dtype=torch.uint8, device=dev)
    out = torch.empty(4, dtype=torch.float32, device=dev)
    dz = torch.empty_like(z[0])

    def ok(rc):
        assert rc == 0, lib.gdkvm_last_error()

    def sd(i):
        ok(lib.gdkvm_signed_distance(tgt[i].data_ptr(), sd2.data_ptr(), sd_ws.data_ptr(), sd_ws.numel(), F, C, S, S, mask, st))

    def loss_b(i):
        ok(lib.gdkvm_seg_loss_boundary_fwd(z[i].data_ptr(), tgt[i].data_ptr(), sd2.data_ptr(), out.data_ptr(), ws_b.data_ptr(), ws_b.numel(), F, C, h, h,
                                           S, S, 1.0, 1.0, 0.05, mask, ops.BF16, 1, st))
        ok(lib.gdkvm_seg_loss_boundary_bwd(z[i].data_ptr(), tgt[i].data_ptr(), sd2.data_ptr(), ws_b.data_ptr(), ws_b.numel(), None, dz.data_ptr(), F, C,
                                           h, h, S, S, mask, ops.BF16, 1, st))

    def loss_p(i):
        ok(lib.gdkvm_seg_loss_fwd(z[i].data_ptr(), tgt[i].data_ptr(), out.data_ptr(), ws_p.data_ptr(), ws_p.numel(), F, C, h, h, S, S, 1.0, 1.0,
                                  ops.BF16, 1, st))
        ok(lib.gdkvm_seg_loss_bwd(z[i].data_ptr(), tgt[i].data_ptr(), ws_p.data_ptr(), ws_p.numel(), None, dz.data_ptr(), F, C, h, h, S, S, ops.BF16, 1, st))

    def all_b(i):
        sd(i)
        loss_b(i)

    sd(0)                                        # (the loss forms below read the maps of input 0's labels: the timing does not depend on which)
    torch.cuda.synchronize()
    frac = float((tgt[0] > 0).float().mean())
    forms = {"signed_distance": sd, "seg_loss_boundary fwd + bwd": loss_b, "signed_distance + seg_loss_boundary fwd + bwd": all_b,
             "seg_loss fwd + bwd (no boundary term)": loss_p}
    times = windows(forms, reps, n_in)
    print(f"(a) {F} frames of {S}x{S}, {C} classes ({C - 1} in the term), logits {h}x{h} bf16, labels uint8 (foreground {100 * frac:.0f} % of the frame); "
          f"signed distance planes in {'LDS' if sd_ws.numel() == 16 else 'the workspace'}: us per call, {CALLS} calls back to back per window of "
          f"device events, median / minimum of {reps} windows per form (alternated, {n_in} inputs in rotation)")
    print(f"{'form':50s} {'median us':>10s} {'min us':>9s}")
    for name in forms:
        print(f"{name:50s} {statistics.median(times[name]):10.1f} {min(times[name]):9.1f}")
    print(flush=True)


def part_b(dev, B, T, S, reps, per_window):
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from gdkvm_amd.train import GraphedTrainStep
    cfg = GDKVMConfig()
    g = torch.Generator().manual_seed(5)
    frames = [torch.rand(B, T, 3, S, S, generator=g).to(dev) for _ in range(2)]
    target = [torch.from_numpy(ellipse_labels(B * T, S, cfg.num_classes, 9 + i)).to(dev).long().reshape(B, T, S, S) for i in range(2)]
    steps = {}
    for name, w in (("weight 0", 0.0), ("weight 0.05", 0.05)):
        torch.manual_seed(3)
        model = GDKVM(cfg).train().to(dev).to(memory_format=torch.channels_last)
        opt = torch.optim.AdamW(model.parameters(), lr=1.0e-4, fused=True, capturable=True)
        steps[name] = GraphedTrainStep(model, opt, frames[0], target[0], torch.bfloat16, warmup=3, boundary_weight=w)
    times = {name: [] for name in steps}
    losses = {}
    for r in range(reps + 2):
        for name, step in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for k in range(per_window):
                losses[name] = step(frames[k % 2], target[k % 2])
            e1.record()
            e1.synchronize()
            if r >= 2:                           # (two warm-up rounds)
                times[name].append(e0.elapsed_time(e1) / per_window)
    print(f"(b) the captured training step (GraphedTrainStep, default widths, {cfg.num_classes} classes, bf16 autocast, fused capturable AdamW), "
          f"{B} clips x {T} frames of {S}x{S}: ms per replay, {per_window} replays per window of device events (two batches in rotation through the "
          f"graph's input buffers), median / minimum of {reps} windows per form (alternated)")
    print(f"{'form':50s} {'median ms':>10s} {'min ms':>9s} {'last loss':>10s}")
    for name in steps:
        print(f"{name:50s} {statistics.median(times[name]):10.3f} {min(times[name]):9.3f} {float(losses[name]):10.4f}")
    d = statistics.median(times["weight 0.05"]) - statistics.median(times["weight 0"])
    print(f"difference of the medians: {1e3 * d:.1f} us per step", flush=True)


def main():
    quick = "--quick" in sys.argv
    ops.require_native()
    dev = torch.device("cuda", torch.cuda.current_device())
    part_a(dev, 8 if quick else 512, 112, 2, 5 if quick else 40)
    part_a(dev, 4 if quick else 64, 256, 4, 5 if quick else 40)
    if "--no-step" not in sys.argv:
        if quick:
            part_b(dev, 2, 2, 64, 3, 3)
        else:
            part_b(dev, 16, 32, 112, 15, 10)


if __name__ == "__main__":
    main()
