"""One graphed training step (GraphedTrainStep, bf16, fused AdamW) in the per-frame step mode (GDKVMConfig(mask_feedback=True): feedback
pass + training pass) at configs[3]'s per-GPU shape -- 16 clips x 32 frames x 112^2 -- beside the ordinary step of the same weights: replay
times (median of the timed replays, device events).  For the per-kernel split run it once per mode under
`rocprofv3 --kernel-trace --stats -- python3 tools/feedback_train_step.py --only feedback` (and `--only plain`): the feedback pass is the
difference of the two tables.

    python3 tools/feedback_train_step.py [--only feedback|plain] [--steps 10] [--warmup 2]"""
import argparse
import dataclasses
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("feedback", "plain"), default=None)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from gdkvm_amd import ops
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from gdkvm_amd.train import GraphedTrainStep
    ops.require_native()
    g = torch.Generator(device="cpu").manual_seed(1)
    frames = torch.rand(a.clips, a.frames, 3, a.size, a.size, generator=g).cuda()
    target = (torch.rand(a.clips, a.frames, a.size, a.size, generator=g) > 0.5).long().cuda()
    modes = [a.only] if a.only else ["plain", "feedback"]
    for mode in modes:
        cfg = GDKVMConfig(mask_feedback=mode == "feedback")
        torch.manual_seed(0)
        model = GDKVM(cfg).cuda().train().to(memory_format=torch.channels_last)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4, fused=True, capturable=True)
        step = GraphedTrainStep(model, opt, frames, target, torch.bfloat16, warmup=a.warmup)
        times = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = step(frames, target)
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        print(f"{mode}: B={a.clips} T={a.frames} {a.size}x{a.size}: graphed step {times[len(times) // 2]:.3f} ms median of {len(times)} "
              f"(min {times[0]:.3f}, max {times[-1]:.3f}); loss {loss.item():.4f}", flush=True)
        del step, opt, model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
