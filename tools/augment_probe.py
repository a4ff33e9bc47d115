#!/usr/bin/env python3
"""What the GPU clip augmentation costs (profiles/r08_a_augment_probe.txt).  python3 tools/augment_probe.py [--quick]

(a) ONE gdkvm_augment_clips launch (ops.augment_clips: warp + intensity table + cast, labels warped alike) against the pass it replaces in
    DevicePrefetcher._convert -- torch.mul(bytes, 1/255, out=buf); uint8 labels are handed on as they are, no pass -- at
    16 x 32 x 3 x 112^2 uint8 -> fp32 and -> bf16, with the identity row and with a 17 degree warp.  Device events around every single call,
    the forms alternated call by call over eight rotating input batches; bytes from the shapes over the median time, as a rate and as a share
    of the 6.3 TB/s achievable HBM rate (the bound of an element-wise pass is bandwidth: 1 byte in, 2 or 4 out per element).
(b) The host-fed graphed training step in train.py's form (pinned uint8 batches -> DevicePrefetcher -> make_train_step) with augmentation
    off and on, three runs each, alternated.  The rule of DESIGN.md section 6: the median of the runs with augmentation must lie inside the
    min - max spread of the runs without."""
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdkvm_amd import ops  # noqa: E402
from gdkvm_amd.data import IDENTITY_ROW, ClipAugment  # noqa: E402
from gdkvm_amd.model import GDKVM, GDKVMConfig  # noqa: E402
from gdkvm_amd.pipeline import DevicePrefetcher, make_train_step  # noqa: E402

HBM = 6.3e12          # bytes / s: the achievable rate the kernel tables of this project are quoted against


def warp_row(H, W, angle_deg=17.0, scale=1.13, tx=2.3, ty=-1.7, gain=1.2, bias=-0.05, gamma=0.7):
    a = math.radians(angle_deg)
    Ai = np.linalg.inv(scale * np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]))
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    off = c - Ai @ (c + np.array([tx, ty]))
    return [Ai[0, 0], Ai[0, 1], off[0], Ai[1, 0], Ai[1, 1], off[1], gain, bias, gamma, 0, 0, 0]


def part_a(dev, shape, n_batches, reps):
    B, T, C, H, W = shape
    g = torch.Generator().manual_seed(0)
    frames = [torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).to(dev) for _ in range(n_batches)]
    target = [torch.randint(0, 2, (B, T, H, W), dtype=torch.uint8, generator=g).to(dev) for _ in range(n_batches)]
    rows = {"identity": torch.tensor([IDENTITY_ROW] * B, dtype=torch.float32, device=dev),
            "17 deg warp": torch.tensor([warp_row(H, W)] * B, dtype=torch.float32, device=dev)}
    n_el, n_lab = B * T * C * H * W, B * T * H * W
    print(f"(a) one call, device events, median of {reps} calls per form (forms alternated, {n_batches} input batches in rotation); "
          f"{B} x {T} x {C} x {H}x{W} uint8 frames, uint8 labels")
    print(f"{'form':44s} {'median us':>10s} {'min us':>9s} {'MB moved':>9s} {'TB/s':>7s} {'% of 6.3 TB/s':>14s}")
    for fdt, esz in ((torch.float32, 4), (torch.bfloat16, 2)):
        out_f = [torch.empty(shape, dtype=fdt, device=dev) for _ in range(3)]
        out_t = [torch.empty((B, T, H, W), dtype=torch.uint8, device=dev) for _ in range(3)]
        forms = {f"torch.mul -> {fdt} (the parent's pass)": (lambda i, k: torch.mul(frames[i], 1.0 / 255.0, out=out_f[k]), n_el * (1 + esz))}
        for name, par in rows.items():
            forms[f"gdkvm_augment_clips -> {fdt}, {name}"] = (
                lambda i, k, par=par: ops.augment_clips(frames[i], target[i], par, fdt, fill_label=255, out=out_f[k], target_out=out_t[k]),
                n_el * (1 + esz) + 2 * n_lab)
        times = {name: [] for name in forms}
        for r in range(reps + 3):
            for name, (fn, _) in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(r % n_batches, r % 3)
                e1.record()
                e1.synchronize()
                if r >= 3:                       # (three warm-up rounds)
                    times[name].append(e0.elapsed_time(e1) * 1e3)
        for name, (_, nbytes) in forms.items():
            med = statistics.median(times[name])
            print(f"{name:44s} {med:10.1f} {min(times[name]):9.1f} {nbytes / 1e6:9.1f} {nbytes / med / 1e6:7.2f} {100 * nbytes / (med * 1e-6) / HBM:13.1f}%")
    print("bound: bandwidth (no arithmetic reuse; bytes = frames in + frames out [+ labels in + labels out]); the augmenting launch does strictly "
          "more than the pass it replaces (the label pass, 4 gathered taps per element), so no bar was fixed in advance", flush=True)


def part_b(dev, shape, n_batches, steps, warm, runs):
    B, T, C, H, W = shape
    g = torch.Generator().manual_seed(1)
    host = [(torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).pin_memory(),
             torch.randint(0, 2, (B, T, H, W), dtype=torch.uint8, generator=g).pin_memory()) for _ in range(n_batches)]
    torch.manual_seed(3)
    model = GDKVM(GDKVMConfig()).train().to(dev).to(memory_format=torch.channels_last)
    adamw = lambda params, fused, capturable: torch.optim.AdamW(params, lr=1e-4, **({"fused": True, "capturable": capturable} if fused else {}))
    f0 = torch.mul(host[0][0].to(dev), 1.0 / 255.0, out=torch.empty(shape, dtype=torch.float32, device=dev))
    step, _, how = make_train_step(model, adamw, f0, host[0][1].to(dev), torch.bfloat16, 1, dev, graph=True)
    print(f"\n(b) host-fed training step, train.py's form: pinned uint8 batches -> DevicePrefetcher(3 slots, fp32 frames) -> {how['launch']}; "
          f"{steps} timed steps after {warm}, ms per step")
    aug = ClipAugment(rotate_deg=10, scale=(0.9, 1.1), translate=0.05, hflip=0.5, gain=(0.9, 1.1), bias=0.05, gamma=(0.8, 1.25), seed=0)
    res = {"off": [], "on": []}
    for run in range(runs):
        for name, a in (("off", None), ("on", aug)):
            n = 0
            for f, t in DevicePrefetcher((host[i % n_batches] for i in range(warm + steps)), dev, slots=3, frames_dtype=torch.float32,
                                         augment=a, epoch=run):
                if n == warm:
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                loss = step(f, t)
                n += 1
            torch.cuda.synchronize()
            ms = 1e3 * (time.perf_counter() - t0) / steps
            res[name].append(ms)
            print(f"  run {run + 1} augmentation {name:3s}: {ms:.3f} ms per step (last loss {float(loss):.4f})", flush=True)
    lo, hi, med_off, med_on = min(res["off"]), max(res["off"]), statistics.median(res["off"]), statistics.median(res["on"])
    if lo <= med_on <= hi:
        verdict = "inside the spread of the runs without augmentation"
    elif med_on < lo:
        verdict = "below the spread of the runs without augmentation"
    else:
        verdict = (f"OUTSIDE the spread of the runs without augmentation by {med_on - hi:+.3f} ms per step "
                   f"({100 * (med_on - med_off) / med_off:+.2f} % of the median)")
    print(f"  off: min {lo:.3f} median {med_off:.3f} max {hi:.3f};  on: median {med_on:.3f}  ->  {verdict}", flush=True)


def main():
    quick = "--quick" in sys.argv
    ops.require_native()
    dev = torch.device("cuda", torch.cuda.current_device())
    shape = (2, 4, 3, 112, 112) if quick else (16, 32, 3, 112, 112)
    part_a(dev, shape, 8, 5 if quick else 40)
    part_b(dev, shape, 8, 4 if quick else 60, 2 if quick else 6, 1 if quick else 3)


if __name__ == "__main__":
    main()
