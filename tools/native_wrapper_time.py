"""Host time of the five native-size wrappers of gdkvm_amd.ops: `python tools/native_wrapper_time.py [REPS]`.

Each wrapper is called on CPU tensors with a batch of 64 clips of one 1 x 1 frame, where the host rule behind the checks has next to nothing
to compute, so a call's time is the wrapper's own work: the size (and spacing) tables, the offsets and the buffer checks.  Per wrapper: the
microseconds per call of REPS (default 9) repetitions of 200 calls each, sorted, then their median and max - min.  Needs no GPU."""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdkvm_amd import ops  # noqa: E402

CLIPS, CALLS = 64, 200


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 9
    sizes, sp = [(1, 1)] * CLIPS, [(300, 200)] * CLIPS
    flat = torch.zeros(CLIPS, dtype=torch.uint8)
    grid = torch.zeros((CLIPS, 1, 1, 1), dtype=torch.uint8)
    calls = {"mask_to_native": lambda: ops.mask_to_native(grid, sizes, 2, target=flat),
             "frames_from_native": lambda: ops.frames_from_native(flat, sizes, 1, grid=(1, 1), channels=1, dtype=torch.uint8),
             "overlay_native": lambda: ops.overlay_native(flat, flat, sizes, 1, 2, reference=flat),
             "surface_distance_native": lambda: ops.surface_distance_native(flat, flat, sizes, 1, sp),
             "lv_measure_native": lambda: ops.lv_measure_native(flat, sizes, 1, sp)}
    for name, f in calls.items():
        f()
        us = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for _ in range(CALLS):
                f()
            us.append((time.perf_counter() - t0) / CALLS * 1e6)
        us.sort()
        print(f"{name:24s} " + " ".join(f"{u:8.1f}" for u in us) + f"   median {us[len(us) // 2]:8.1f}  max-min {us[-1] - us[0]:6.1f}  us / call")


if __name__ == "__main__":
    main()
