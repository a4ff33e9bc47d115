"""One graphed training step (GraphedTrainStep, bf16, fused AdamW) at configs[3]'s per-GPU shape -- 16 clips x 32 frames x 112^2 -- with a
chosen per-head key width: the replay time (median of the timed replays, device events) and the scan's training workspace.  Run under
`rocprofv3 --kernel-trace --stats -- python3 tools/wide_key_train_step.py` for the per-kernel split.

    python3 tools/wide_key_train_step.py [--key-dim 128] [--value-dim 128] [--steps 5] [--warmup 2]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--key-dim", type=int, default=128)
    ap.add_argument("--value-dim", type=int, default=128)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    from gdkvm_amd import ops
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from gdkvm_amd.train import GraphedTrainStep
    ops.require_native()
    cfg = GDKVMConfig(key_dim=a.key_dim, value_dim=a.value_dim)
    torch.manual_seed(0)
    model = GDKVM(cfg).cuda().train().to(memory_format=torch.channels_last)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, fused=True, capturable=True)
    g = torch.Generator(device="cpu").manual_seed(1)
    frames = torch.rand(a.clips, a.frames, 3, a.size, a.size, generator=g).cuda()
    target = (torch.rand(a.clips, a.frames, a.size, a.size, generator=g) > 0.5).long().cuda()
    step = GraphedTrainStep(model, opt, frames, target, torch.bfloat16, warmup=a.warmup)
    times = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        loss = step(frames, target)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    N = (a.size // cfg.stride) ** 2
    ws = int(ops.load().gdkvm_scan_train_workspace_bytes(a.clips, a.frames, cfg.heads, N, a.key_dim, a.value_dim, 1))
    times.sort()
    print(f"key_dim={a.key_dim} value_dim={a.value_dim} B={a.clips} T={a.frames} {a.size}x{a.size} N={N}: graphed step "
          f"{times[len(times) // 2]:.3f} ms median of {len(times)} (min {times[0]:.3f}); loss {loss.item():.4f}; "
          f"scan training workspace {ws} bytes ({ws / 2**20:.1f} MiB)")


if __name__ == "__main__":
    main()
