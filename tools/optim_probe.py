#!/usr/bin/env python3
"""What the optimiser part of the training step costs, alone (profiles/r15_a_optim_probe.txt).
python3 tools/optim_probe.py [--quick]

Over the parameters of the BASELINE configs[3] model (GDKVMConfig(): 74 tensors with their real shapes and strides, channels-last weights) and
of the 256 x 256 / 4-class model: torch.optim.AdamW(fused=True, capturable=True) against optim.NativeAdamW plain, with clipping, and with
clipping + EMA.  Gradients are seeded noise; no forward or backward runs.  Each form is captured ONCE as a graph that steps SETS independent
copies of (parameters, gradients, optimiser state) one after the other -- 6 x 64 MB, more than the 256 MB the Infinity Cache could keep between
two visits of a set -- so a replay is SETS steps with no host work in between; REPLAYS replays sit between one pair of device events, the forms
alternate window by window, and the figure is the median (and minimum) over the windows of window / (REPLAYS x SETS).  One JSON line per
form; `bytes` is what the step must move (fp32: torch reads p, g, m, v and writes p, m, v = 28 B per element; the native step reads g once
more for the norm = 32 B, + 8 B with the EMA), `gbytes_per_s` that over the median."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gdkvm_amd import ops  # noqa: E402
from gdkvm_amd.model import GDKVM, GDKVMConfig  # noqa: E402
from gdkvm_amd.optim import NativeAdamW  # noqa: E402

FORMS = {
    "torch AdamW(fused, capturable)": (None, 28),
    "NativeAdamW": (dict(), 32),
    "NativeAdamW + clip": (dict(max_norm=1.0), 32),
    "NativeAdamW + clip + EMA": (dict(max_norm=1.0, ema_decay=0.999), 40),
}


def build(form, model, sets, dev, seed):
    """`sets` copies of the model's parameters with gradients and an optimiser each; returns the graph that steps them all."""
    gen = torch.Generator().manual_seed(seed)
    opts = []
    for _ in range(sets):
        named = [(n, torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format))) for n, p in model.named_parameters()]
        for _, p in named:
            g = (1e-3 * torch.randn(p.numel(), generator=gen)).to(dev)
            p.grad = g.as_strided(p.shape, p.stride())
        kw = FORMS[form][0]
        opt = torch.optim.AdamW([p for _, p in named], lr=1e-4, fused=True, capturable=True) if kw is None else \
            NativeAdamW(named, lr=1e-4, schedule="cosine", warmup_steps=10, total_steps=100000, **kw)
        opts.append(opt)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        for _ in range(2):                       # (the state is created outside the capture)
            for opt in opts:
                opt.step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize(dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for opt in opts:
            opt.step()
    return graph, opts


def probe(label, cfg, dev, sets, replays, windows):
    torch.manual_seed(3)
    model = GDKVM(cfg).train().to(dev).to(memory_format=torch.channels_last)
    tensors = sum(1 for _ in model.parameters())
    elems = sum(p.numel() for p in model.parameters())
    built = {form: build(form, model, sets, dev, 7) for form in FORMS}
    times = {form: [] for form in FORMS}
    for r in range(windows + 3):
        for form, (graph, _) in built.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                graph.replay()
            e1.record()
            e1.synchronize()
            if r >= 3:                           # (three warm-up rounds)
                times[form].append(e0.elapsed_time(e1) * 1e3 / (replays * sets))
    for form, (_, per_elem) in FORMS.items():
        med = statistics.median(times[form])
        print(json.dumps({"probe": "optim", "model": label, "form": form, "tensors": tensors, "elements": elems, "bytes": per_elem * elems,
                          "median_us": round(med, 2), "min_us": round(min(times[form]), 2), "gbytes_per_s": round(per_elem * elems / med / 1e3, 1),
                          "windows": windows, "steps_per_window": replays * sets, "sets": sets}), flush=True)


def main():
    quick = "--quick" in sys.argv
    ops.require_native()
    dev = torch.device("cuda", torch.cuda.current_device())
    sets, replays, windows = (2, 2, 3) if quick else (6, 10, 30)
    probe("configs[3]: default widths, 2 classes (112 x 112 clips)", GDKVMConfig(), dev, sets, replays, windows)
    probe("4 classes (256 x 256 clips)", GDKVMConfig(num_classes=4), dev, sets, replays, windows)


if __name__ == "__main__":
    main()
