#!/usr/bin/env python3
"""What the LV measurement, the temporal vote, the largest-component filter and the hole filling in front of it and the surface distances
cost (profiles/r10_a_lv_probe.txt, profiles/r12_a_cc_probe.txt, profiles/r13_a_surface_probe.txt, profiles/r16_a_fill_holes_probe.txt; the
vote's figures are in DESIGN.md).
python3 tools/lv_probe.py [--quick] [--no-eval] [--vote-only] [--mm-only] [--beats] [--native] [--native-input] [--overlay] [--native-surface] [--native-lv] [--contour]

(a) gdkvm_lv_measure (class 1, 20 disks) on 512 frames of 112^2 (the cfg2 mask) and of 256^2, beside the kernel that writes those very masks,
    gdkvm_upsample_argmax_dice (bf16 stride-4 logits of 2 classes + uint8 target -> mask + counts), in the same run.  Both are called through the
    C symbols on preallocated outputs, CALLS launches back to back between ONE pair of device events (a single launch between two events on an
    empty queue would time the host's way to the launch, not a kernel of a few microseconds); time per launch = window / CALLS, the forms
    alternated window by window over four rotating inputs, median and minimum over the windows.  Masks: one rotated ellipse per frame covering
    about a tenth of it (a ventricle); every pixel of the class (the worst case for the per-pixel passes); no pixel of the class.  The floor is
    the bytes read (and, for the mask kernel, written) once over the 6.3 TB/s achievable HBM rate.  gdkvm_largest_component (class 1,
    4-connected, fill 0, out of place, with a target) runs in the same windows on the same three fills, the ellipses with three islands each
    (discs of radius 1 to 5 % of the side; the kernel removes them), and at 8-connectivity on the first.  gdkvm_fill_holes (class 1, complement
    4-connected, any size, out of place, with a target) runs in the same windows: the ellipses with three holes punched into each (discs of
    class 0 of radius 1 to 3 % of the side; the kernel fills them), the same at connectivity 8, the ellipse alone (nothing to fill: a copy),
    every pixel of the class (no complement), no pixel of the class (the whole frame is one outside component, which the kernel knows after
    its counting pass: nothing can enclose a hole) and ONE pixel of the class in the middle (the labelling's worst case: every other pixel is
    one outside component, the same amount of labelling as largest_component's "every pixel of the class").  gdkvm_surface_distance (class 1)
    runs in the same windows: ellipse against the next input's ellipse (a prediction close to its target), the ellipse with islands against
    it, a checkerboard against a one-pixel-shifted checkerboard (every pixel of the class is surface) and against the ellipse (every row
    walk of the ellipse's surface ends at once, every walk of the checkerboard's is as long as the ellipse is far), and an empty class.
    gdkvm_lv_measure_mm and gdkvm_surface_distance_mm (a spacing of 330 x 468 um for every frame) run in the same windows on the same inputs
    as the pixel kernels' rows, so that each mm row reads against its pixel row of the same run (--mm-only: part (a) with the lv_measure and
    surface_distance rows alone, pixel and mm, and nothing else).  gdkvm_lv_biplane runs beside lv_measure_mm on the ellipse's records: the
    frames as clips of one frame, each paired with the next.
(v) gdkvm_temporal_vote at the cfg2 mask shape, 16 clips of 32 frames of 112^2 with 4 classes (--vote-only: this part alone), radius 1, 2
    and 7 with a target and radius 1 without, through the C symbol on preallocated outputs, beside two yardsticks in the same alternated
    windows: the plain torch expression of the same filter (torch_vote: a one-hot, a window sum along T, an argmax with the tie rules; the
    probe first checks that it computes what the kernel computes) and the byte floor, 2 clips T H W bytes over the copy bandwidth measured
    here on 512 MiB that no cache holds.  Inputs: clips of an ellipse in a ring that drifts over the frames with 15 % of the pixels
    re-drawn, four in rotation.  Then 320 clips (two inputs of 128 MB in rotation), where the launcher takes the form with 16 pixels
    per lane instead of 4, without the torch rows.
(e) --beats (this part alone): gdkvm_lv_beats (distance 20, prominence 500 per mille, 16 beats listed) on 16 clips of 512 frames and on 2 clips
    of 4096, on curves of the synthetic kind (the area and the volume of a pulsating ellipse with one beat per 40 frames and a few per cent of
    noise, samples made pairwise distinct, the last eighth of every second clip padding), through the C symbol on preallocated outputs in windows of device events; beside
    it what a user does without it: the same curves, already on the device as lv_measure left them, through .cpu() into
    scipy.signal.find_peaks and a host loop over the beats, timed on the host's clock around the whole round trip.  A device call against a
    host round trip, not kernel against kernel.
(n) --native (this part alone): gdkvm_mask_to_native on 16 clips of 10 frames of 256^2 with 4 classes taken to 549 x 778 each and to mixed
    CAMUS-like sizes, with a native target (out and counts, counts only, out only), beside the torch expression of the same thing (one-hot,
    F.interpolate, argmax, counts) and the byte floor: source + native out + native target bytes over the HBM rate above
    (profiles/native_probe.txt).
(i) --native-input (this part alone): gdkvm_frames_from_native on 16 clips of 10 frames of 549 x 778 (and of mixed CAMUS-like sizes) taken to
    256^2, three planes, bf16 (and uint8), beside F.adaptive_avg_pool2d + cast on the same data -- the nearest torch expression, NOT the
    same rule at ratios that are no whole number (it averages the pixels a window touches with equal weights; the rule weighs them by
    their overlap) -- and the byte floor: native bytes read plus output bytes written over the HBM rate above
    (profiles/native_input_probe.txt).
(o) --overlay (this part alone): gdkvm_overlay_native on 16 clips of 10 frames of 549 x 778 (and of mixed CAMUS-like sizes), ventricle-like
    masks of 4 classes, with and without a reference mask, at contour widths 1 and 3, beside the torch expression of the same rule on the
    same device tensors (padded shifts compared, palettes gathered, torch.where; the probe first checks that it draws the kernel's bytes)
    and the byte floor: 2 or 3 bytes read and 3 written per pixel over the HBM rate above (profiles/overlay_probe.txt).
(s) --native-surface (this part alone): gdkvm_surface_distance_native (class 1, 308 x 154 um per native pixel) on 16 clips of 10 frames of
    549 x 778 and of the mixed CAMUS-like sizes of (n): ventricle-like ellipses against a shifted copy (a prediction close to its tracing),
    the ellipses with islands against the ellipses, and an empty class (class 3); through the C symbol on a preallocated workspace, beside
    two yardsticks in the same alternated windows: gdkvm_surface_distance_mm's workspace form on the uniform 549 x 778 batch (one workgroup
    per frame; the only other way to these records, and the probe first checks that they are bit-equal there) and the byte floor, mask +
    target bytes over the HBM rate above.  Then ONE moderate pathological frame, a 512^2 checkerboard against a single pixel, run once and
    timed with a pair of events (profiles/native_surface_probe.txt).  --once: every form once, no windows (for a kernel trace).
(l) --native-lv (this part alone): gdkvm_lv_measure_native (class 1, 20 disks, 308 x 154 um per native pixel) on a CAMUS-like ragged batch,
    16 clips of 10 frames with sizes drawn between 584 x 323 and 1945 x 1181: ventricle-like ellipses, every pixel of the class, and an
    empty class, beside the byte floor -- every mask byte read once per pass (three passes) over the HBM rate above.  Then the largest shape
    gdkvm_lv_measure_mm runs too, 160 frames of 1024 x 1024, beside that entry (one workgroup per frame; the probe first checks that the
    records are bit-equal) in the same alternated windows, with the ratio (profiles/native_lv_probe.txt).  --once as for (s).
(c) --contour (this part alone): gdkvm_lv_contour (class 1 against the wall {2} and the base {3}) on 512 frames of 112^2 and of 256^2, the
    ellipses of (a) inside a ring of class 2 with class 3 over their lower quarter: without and with a spacing, without a base set, on every
    pixel of the class and on none, beside gdkvm_lv_measure on the same masks, the torch expression of the same eight counts (the padded
    mask compared, eight shifted ANDs and sums per set; the probe first checks that it counts what the kernel counts) and the byte floor.
(b) eval.py's wall time (a fresh process each: start-up, captures and the split) on the synthetic split with data.lv_class=1, with
    data.lv_keep_largest=4 on top of it, with data.lv_fill_holes=4 instead, with data.temporal_vote=1 instead, with data.surface_class=1
    instead, and with data.lv_class=-1, alternated, twice each."""
import math
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gdkvm_amd import ops  # noqa: E402

HBM = 6.3e12          # bytes / s: the achievable rate the kernel tables of this project are quoted against


def ellipse_masks(F, S, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    out = np.zeros((F, S, S), np.uint8)
    for f in range(F):
        th = rng.uniform(-0.5, 0.5)
        la, sa = S * rng.uniform(0.22, 0.30), S * rng.uniform(0.10, 0.14)
        dx, dy = xx - S * rng.uniform(0.45, 0.55), yy - S * rng.uniform(0.45, 0.55)
        al, ac = dx * math.sin(th) + dy * math.cos(th), dx * math.cos(th) - dy * math.sin(th)
        out[f][(al / la) ** 2 + (ac / sa) ** 2 <= 1.0] = 1
    return out


def add_islands(masks, seed):
    """Three discs of class 1 per frame, away from the centre where the ellipse lies (they may touch it: then they are no islands)."""
    rng = np.random.default_rng(seed)
    F, S, _ = masks.shape
    yy, xx = np.mgrid[0:S, 0:S]
    out = masks.copy()
    for f in range(F):
        for _ in range(3):
            cy, cx = (rng.uniform(0.04, 0.16) * S if rng.random() < 0.5 else rng.uniform(0.84, 0.96) * S for _ in range(2))
            out[f][(yy - cy) ** 2 + (xx - cx) ** 2 <= (rng.uniform(0.01, 0.05) * S) ** 2] = 1
    return out


def punch_holes(masks, seed):
    """Three discs of class 0 per frame, inside the ellipse (centres drawn from its own pixels; one that reaches its rim is a notch, no hole)."""
    rng = np.random.default_rng(seed)
    F, S, _ = masks.shape
    yy, xx = np.mgrid[0:S, 0:S]
    out = masks.copy()
    for f in range(F):
        ys, xs = np.nonzero(masks[f])
        for k in rng.integers(0, len(ys), 3):
            out[f][(yy - ys[k]) ** 2 + (xx - xs[k]) ** 2 <= (rng.uniform(0.01, 0.03) * S) ** 2] = 0
    return out


CALLS = 20            # launches per timed window


def part_a(dev, F, S, reps, n_in=4, only=()):
    lib = ops.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    g = torch.Generator().manual_seed(S)
    masks_np = [ellipse_masks(F, S, s) for s in range(n_in)]
    masks = [torch.from_numpy(m).to(dev) for m in masks_np]
    isl = [torch.from_numpy(add_islands(m, s)).to(dev) for s, m in enumerate(masks_np)]
    holed = [torch.from_numpy(punch_holes(m, s)).to(dev) for s, m in enumerate(masks_np)]
    fh_ws = torch.empty(max(16, int(lib.gdkvm_fill_holes_workspace_bytes(F, S, S))), dtype=torch.uint8, device=dev)
    cc_out = torch.empty((F, S, S), dtype=torch.uint8, device=dev)
    cc_info = torch.empty((F, 8), dtype=torch.int32, device=dev)
    cc_ws = torch.empty(max(16, int(lib.gdkvm_largest_component_workspace_bytes(F, S, S))), dtype=torch.uint8, device=dev)
    full = torch.ones((F, S, S), dtype=torch.uint8, device=dev)
    lone = full.clone()
    lone[:, S // 2, S // 2] = 2
    board = ((torch.arange(S, device=dev)[:, None] + torch.arange(S, device=dev)[None, :]) % 2 == 0).to(torch.uint8).expand(F, S, S).contiguous()
    board_shifted = (1 - board).contiguous()
    sd_out = torch.empty((F, 8), dtype=torch.int64, device=dev)
    sd_ws = torch.empty(max(16, int(lib.gdkvm_surface_distance_workspace_bytes(F, S, S))), dtype=torch.uint8, device=dev)
    logits = [torch.randn((F, 2, S // 4, S // 4), generator=g).to(dev).bfloat16() for _ in range(n_in)]
    m_out = torch.empty((F, S, S), dtype=torch.uint8, device=dev)
    c_out = torch.empty((F, 2, 3), dtype=torch.int32, device=dev)
    stats = torch.empty((F, 12), dtype=torch.int64, device=dev)
    disks = torch.empty((F, 20), dtype=torch.int64, device=dev)
    geom = torch.empty((F, 4), dtype=torch.float64, device=dev)
    geom_mm = torch.empty((F, 6), dtype=torch.float64, device=dev)
    spacing = torch.tensor([330, 468], dtype=torch.int32, device=dev).expand(F, 2).contiguous()
    sdm_ws = torch.empty(max(16, int(lib.gdkvm_surface_distance_mm_workspace_bytes(F, S, S))), dtype=torch.uint8, device=dev)

    def lv(mask, cls):
        rc = lib.gdkvm_lv_measure(mask.data_ptr(), stats.data_ptr(), disks.data_ptr(), geom.data_ptr(), F, S, S, cls, 20, st)
        assert rc == 0, lib.gdkvm_last_error()

    def lv_mm(mask, cls):
        rc = lib.gdkvm_lv_measure_mm(mask.data_ptr(), spacing.data_ptr(), stats.data_ptr(), disks.data_ptr(), geom_mm.data_ptr(), F, S, S, cls, 20, st)
        assert rc == 0, lib.gdkvm_last_error()

    def sd_mm(mask, target, cls):
        rc = lib.gdkvm_surface_distance_mm(mask.data_ptr(), target.data_ptr(), spacing.data_ptr(), sd_out.data_ptr(), sdm_ws.data_ptr(), sdm_ws.numel(),
                                           F, S, S, cls, st)
        assert rc == 0, lib.gdkvm_last_error()

    def cc(mask, target, cls, conn=4):
        rc = lib.gdkvm_largest_component(mask.data_ptr(), target.data_ptr(), cc_out.data_ptr(), cc_info.data_ptr(), cc_ws.data_ptr(), cc_ws.numel(),
                                         F, S, S, cls, conn, 0, st)
        assert rc == 0, lib.gdkvm_last_error()

    def fh(mask, target, cls, conn=4):
        rc = lib.gdkvm_fill_holes(mask.data_ptr(), target.data_ptr(), cc_out.data_ptr(), cc_info.data_ptr(), fh_ws.data_ptr(), fh_ws.numel(),
                                  F, S, S, cls, conn, 0, st)
        assert rc == 0, lib.gdkvm_last_error()

    def sd(mask, target, cls):
        rc = lib.gdkvm_surface_distance(mask.data_ptr(), target.data_ptr(), sd_out.data_ptr(), sd_ws.data_ptr(), sd_ws.numel(), F, S, S, cls, st)
        assert rc == 0, lib.gdkvm_last_error()

    def up(i):
        rc = lib.gdkvm_upsample_argmax_dice(logits[i].data_ptr(), masks[i].data_ptr(), m_out.data_ptr(), c_out.data_ptr(), F, 2, S // 4, S // 4, S, S,
                                            ops.BF16, st)
        assert rc == 0, lib.gdkvm_last_error()

    # gdkvm_lv_biplane on records of their own (the ellipse's, written once): the F frames as F clips of one frame, each paired with the next
    lv_mm(masks[0], 1)
    bp_rec = [t.clone() for t in (stats, disks, geom_mm)]
    bp_pairs = torch.stack([torch.arange(F), (torch.arange(F) + 1) % F], 1).to(torch.int32).to(dev)
    bp_out = torch.empty((F, 1, 3), dtype=torch.float64, device=dev)
    bp_npix = torch.empty((F, 1), dtype=torch.int64, device=dev)

    def bp():
        rc = lib.gdkvm_lv_biplane(bp_rec[0].data_ptr(), bp_rec[1].data_ptr(), bp_rec[2].data_ptr(), spacing.data_ptr(), bp_pairs.data_ptr(),
                                  bp_out.data_ptr(), bp_npix.data_ptr(), F, 1, 20, F, st)
        assert rc == 0, lib.gdkvm_last_error()

    frac = float(masks[0].float().mean())
    forms = {
        f"lv_measure, ellipse ({100 * frac:.0f} % of the frame)": (lambda i: lv(masks[i], 1), F * S * S),
        "lv_measure, every pixel of the class": (lambda i: lv(full, 1), F * S * S),
        "lv_measure, no pixel of the class": (lambda i: lv(full, 2), F * S * S),
        "upsample_argmax_dice (writes the mask)": (up, F * (2 * 2 * (S // 4) ** 2 + 2 * S * S)),
        "largest_component, ellipse + 3 islands": (lambda i: cc(isl[i], masks[i], 1), 2 * F * S * S),
        "largest_component, the same, 8-connected": (lambda i: cc(isl[i], masks[i], 1, 8), 2 * F * S * S),
        "largest_component, ellipse alone (a copy)": (lambda i: cc(masks[i], masks[i], 1), 2 * F * S * S),
        "largest_component, every pixel of the class": (lambda i: cc(full, masks[i], 1), 2 * F * S * S),
        "largest_component, no pixel of the class": (lambda i: cc(full, masks[i], 2), 2 * F * S * S),
        "fill_holes, ellipse with 3 holes": (lambda i: fh(holed[i], masks[i], 1), 2 * F * S * S),
        "fill_holes, the same, connectivity 8": (lambda i: fh(holed[i], masks[i], 1, 8), 2 * F * S * S),
        "fill_holes, ellipse alone (a copy)": (lambda i: fh(masks[i], masks[i], 1), 2 * F * S * S),
        "fill_holes, every pixel of the class": (lambda i: fh(full, masks[i], 1), 2 * F * S * S),
        "fill_holes, no pixel of the class": (lambda i: fh(full, masks[i], 2), 2 * F * S * S),
        "fill_holes, one pixel of the class": (lambda i: fh(lone, masks[i], 2), 2 * F * S * S),
        "surface_distance, ellipse against ellipse": (lambda i: sd(masks[i], masks[(i + 1) % n_in], 1), 2 * F * S * S),
        "surface_distance, ellipse + 3 islands against it": (lambda i: sd(isl[i], masks[i], 1), 2 * F * S * S),
        "surface_distance, checkerboard against shifted": (lambda i: sd(board, board_shifted, 1), 2 * F * S * S),
        "surface_distance, checkerboard against ellipse": (lambda i: sd(board, masks[i], 1), 2 * F * S * S),
        "surface_distance, no pixel of the class": (lambda i: sd(full, masks[i], 2), 2 * F * S * S),
        "lv_measure_mm, ellipse": (lambda i: lv_mm(masks[i], 1), F * S * S),
        "lv_measure_mm, every pixel of the class": (lambda i: lv_mm(full, 1), F * S * S),
        "lv_measure_mm, no pixel of the class": (lambda i: lv_mm(full, 2), F * S * S),
        "lv_measure_mm records -> lv_biplane, F pairs": (lambda i: bp(), F * (2 * 8 * (20 + 4) + 32)),
        "surface_distance_mm, ellipse against ellipse": (lambda i: sd_mm(masks[i], masks[(i + 1) % n_in], 1), 2 * F * S * S),
        "surface_distance_mm, ellipse + 3 islands against it": (lambda i: sd_mm(isl[i], masks[i], 1), 2 * F * S * S),
        "surface_distance_mm, checkerboard against shifted": (lambda i: sd_mm(board, board_shifted, 1), 2 * F * S * S),
        "surface_distance_mm, checkerboard against ellipse": (lambda i: sd_mm(board, masks[i], 1), 2 * F * S * S),
        "surface_distance_mm, no pixel of the class": (lambda i: sd_mm(full, masks[i], 2), 2 * F * S * S),
    }
    if only:
        forms = {name: f for name, f in forms.items() if name.startswith(only)}
    cc(isl[0], masks[0], 1)
    torch.cuda.synchronize()
    removed = (cc_info[:, 1] - cc_info[:, 2]).float()
    print(f"    (islands: {float(cc_info[:, 0].float().mean()):.2f} components per frame, {float(removed.mean()):.0f} of {float(cc_info[:, 1].float().mean()):.0f} "
          f"pixels removed; label words in {'LDS' if cc_ws.numel() == 16 else 'the workspace, ' + str(cc_ws.numel() >> 20) + ' MiB'})")
    fh(holed[0], masks[0], 1)
    torch.cuda.synchronize()
    print(f"    (holes: {float(cc_info[:, 0].float().mean()):.2f} per frame, {float(cc_info[:, 3].float().mean()):.0f} pixels filled beside "
          f"{float(cc_info[:, 2].float().mean()):.0f} of the class, {int((cc_out != masks[0]).any((1, 2)).sum())} of {F} frames differ from the ellipse; "
          f"label words in {'LDS' if fh_ws.numel() == 16 else 'the workspace, ' + str(fh_ws.numel() >> 20) + ' MiB'})")
    sd(masks[0], masks[1], 1)
    torch.cuda.synchronize()
    met, ok = ops.surface_metrics(sd_out)
    print(f"    (ellipse against ellipse: {float(sd_out[:, :2].float().mean()):.0f} surface pixels per set, mean HD {float(met[:, 0].mean()):.2f}, HD95 "
          f"{float(met[:, 1].mean()):.2f}, ASSD {float(met[:, 2].mean()):.2f} pixels over {int(ok.sum())} frames; the frame's words in "
          f"{'LDS' if sd_ws.numel() == 16 else 'the workspace, ' + str(sd_ws.numel() >> 20) + ' MiB'})")
    sd_mm(masks[0], masks[1], 1)
    torch.cuda.synchronize()
    met, ok = ops.surface_metrics_mm(sd_out)
    print(f"    (the same at 330 x 468 um: mean HD {float(met[:, 0].mean()):.2f}, HD95 {float(met[:, 1].mean()):.2f}, ASSD {float(met[:, 2].mean()):.2f} mm "
          f"over {int(ok.sum())} frames; the frame's words in {'LDS' if sdm_ws.numel() == 16 else 'the workspace, ' + str(sdm_ws.numel() >> 20) + ' MiB'})")
    times = {name: [] for name in forms}
    for r in range(reps + 3):
        for name, (fn, _) in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                fn(r % n_in)
            e1.record()
            e1.synchronize()
            if r >= 3:                           # (three warm-up rounds)
                times[name].append(e0.elapsed_time(e1) * 1e3 / CALLS)
    print(f"(a) {F} frames of {S}x{S}: us per launch, {CALLS} launches back to back per window of device events, median / minimum of {reps} windows "
          f"per form (alternated, {n_in} inputs in rotation)")
    print(f"{'form':48s} {'median us':>10s} {'min us':>9s} {'MB':>8s} {'floor us':>9s}")
    for name, (_, nbytes) in forms.items():
        print(f"{name:48s} {statistics.median(times[name]):10.1f} {min(times[name]):9.1f} {nbytes / 1e6:8.1f} {nbytes / HBM * 1e6:9.2f}")
    print(flush=True)


def drifting_masks(clips, T, S, ncls, seed, dev):
    """Label clips for the temporal vote: per clip an ellipse of class 1 inside a ring of class 2 that drifts and breathes over the frames,
    15 % of the pixels re-drawn uniformly over the classes (the flicker the vote removes)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    out = np.zeros((clips, T, S, S), np.uint8)
    for b in range(clips):
        cy, cx, dy, dx = S * rng.uniform(0.45, 0.55), S * rng.uniform(0.45, 0.55), S * rng.uniform(-0.003, 0.003), S * rng.uniform(-0.003, 0.003)
        for t in range(T):
            s = 1.0 + 0.15 * math.sin(2 * math.pi * t / T)
            d = ((yy - cy - dy * t) / (0.27 * S * s)) ** 2 + ((xx - cx - dx * t) / (0.13 * S * s)) ** 2
            out[b, t][d < 1.5] = 2 % ncls
            out[b, t][d < 1.0] = 1
    noise = rng.random(out.shape) < 0.15
    out[noise] = rng.integers(0, ncls, int(noise.sum()), dtype=np.uint8)
    return torch.from_numpy(out).to(dev)


def torch_vote(mask, ncls, r):
    """The same filter as a plain torch expression (the yardstick): a one-hot, a window sum along T from a running sum, and an argmax over
    keys 2 votes + (class == own label) -- the first maximum is the smallest class, the own label wins the ties it is part of."""
    T = mask.shape[1]
    oh = (mask.unsqueeze(-1) == torch.arange(ncls, dtype=torch.uint8, device=mask.device)).to(torch.int16)       # [clips, T, H, W, ncls]
    cs = torch.nn.functional.pad(oh.cumsum(1, dtype=torch.int16), (0, 0, 0, 0, 0, 0, 1, 0))
    t = torch.arange(T, device=mask.device)
    votes = cs[:, (t + r + 1).clamp(max=T)] - cs[:, (t - r).clamp(min=0)]
    return torch.where(mask < ncls, (votes * 2 + oh).argmax(-1).to(torch.uint8), mask)


def part_v(dev, clips, T, S, ncls, reps, n_in=4, torch_rows=True):
    """gdkvm_temporal_vote at the cfg2 mask shape beside its two yardsticks, in the same windows: the torch expression of the filter
    (torch_rows; left out at the large batch, where its one-hots take gigabytes), and the byte floor -- every mask byte read once, every
    out byte written once -- over the copy bandwidth measured here."""
    lib = ops.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    masks = [drifting_masks(clips, T, S, ncls, s, dev) for s in range(n_in)]
    out = torch.empty_like(masks[0])
    info = torch.empty((clips, T, 4), dtype=torch.int32, device=dev)
    counts = torch.empty((clips, T, ncls, 3), dtype=torch.int32, device=dev)
    big = [torch.empty(512 << 20, dtype=torch.uint8, device=dev) for _ in range(2)]      # a copy that no cache holds
    nbytes = 2 * masks[0].numel()

    def tv(i, r, target=True):
        rc = lib.gdkvm_temporal_vote(masks[i].data_ptr(), masks[(i + 1) % n_in].data_ptr() if target else None, out.data_ptr(), info.data_ptr(),
                                     counts.data_ptr() if target else None, None, 0, clips, T, S, S, ncls, r, st)
        assert rc == 0, lib.gdkvm_last_error()

    for r in (1, 2) if torch_rows else ():                         # the yardstick computes the same filter
        tv(0, r)
        assert torch.equal(out, torch_vote(masks[0], ncls, r)), r
    tv(0, 1)
    torch.cuda.synchronize()
    print(f"    (vote, r = 1: {float(info[..., 0].float().mean()):.0f} of {S * S} pixels changed per frame, {float(info[..., 1].float().mean()):.0f} "
          f"differ from the previous frame before and {float(info[..., 2].float().mean()):.0f} after)")
    forms = {
        "temporal_vote, r = 1, with a target": (lambda i: tv(i, 1), CALLS),
        "temporal_vote, r = 2, with a target": (lambda i: tv(i, 2), CALLS),
        "temporal_vote, r = 1, without a target": (lambda i: tv(i, 1, False), CALLS),
        "temporal_vote, r = 7, with a target": (lambda i: tv(i, 7), CALLS),
        "torch expression, r = 1": (lambda i: torch_vote(masks[i], ncls, 1), 2),
        "torch expression, r = 2": (lambda i: torch_vote(masks[i], ncls, 2), 2),
        "copy of the mask (out.copy_)": (lambda i: out.copy_(masks[i]), CALLS),
        "copy of 512 MiB": (lambda i: big[1].copy_(big[0]), 2),
    }
    if not torch_rows:
        forms = {name: f for name, f in forms.items() if not name.startswith("torch")}
    times = {name: [] for name in forms}
    for rep in range(reps + 3):
        for name, (fn, calls) in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn(rep % n_in)
            e1.record()
            e1.synchronize()
            if rep >= 3:
                times[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    bw = 2 * big[0].numel() / (statistics.median(times["copy of 512 MiB"]) * 1e-6)
    floor = nbytes / bw * 1e6
    print(f"(v) temporal vote, {clips} clips of {T} frames of {S}x{S}, {ncls} classes: us per call, windows of device events, median / minimum of "
          f"{reps} windows per form (alternated, {n_in} inputs in rotation)")
    print(f"    copy bandwidth {bw / 1e12:.2f} TB/s (read + write of 512 MiB); byte floor of the vote = {nbytes / 1e6:.1f} MB over it = {floor:.2f} us")
    print(f"{'form':48s} {'median us':>10s} {'min us':>9s} {'x floor':>9s} {'x torch':>9s}")
    for name in forms:
        med = statistics.median(times[name])
        ref = statistics.median(times["torch expression, r = 2" if "r = 2" in name else "torch expression, r = 1"]) if torch_rows else math.nan
        print(f"{name:48s} {med:10.1f} {min(times[name]):9.1f} {med / floor:9.1f} {med / ref:9.3f}")
    print(flush=True)


def beat_curves(clips, T, seed, dev):
    """area int64 [clips, T], vol float64 [clips, T], length int32 [clips]: a pulsating ellipse's pixel count and its volume, one beat per
    40 frames, a random phase and noise; every second clip ends in padding (zeros) behind 7/8 of its frames.  The areas are made pairwise
    distinct (times 8192, plus a permutation of the frame numbers): among equal minima scipy's choice is that of an unstable sort, and the
    yardstick has to find the beats the kernel finds."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    k = 1.0 + 0.18 * np.sin(rng.uniform(0, 2 * np.pi, (clips, 1)) + 2 * np.pi * t / 40.0) + rng.normal(0, 0.006, (clips, T))
    area = np.round(1200.0 * k * k).astype(np.int64) * 8192 + np.stack([rng.permutation(T) for _ in range(clips)])
    vol = 30000.0 * k ** 3
    length = np.full(clips, T, np.int32)
    length[1::2] = T - T // 8
    for b in range(clips):
        area[b, length[b]:], vol[b, length[b]:] = 0, 0.0
    return torch.from_numpy(area).to(dev), torch.from_numpy(vol).to(dev), torch.from_numpy(length).to(dev)


def part_e(dev, clips, T, reps, n_in=4):
    from scipy.signal import find_peaks
    lib = ops.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    ins = [beat_curves(clips, T, s, dev) for s in range(n_in)]
    beats = torch.empty((clips, 16, 2), dtype=torch.int32, device=dev)
    val = torch.empty((clips, 16, 3), dtype=torch.float64, device=dev)
    info = torch.empty((clips, 4), dtype=torch.int32, device=dev)
    summ = torch.empty((clips, 4), dtype=torch.float64, device=dev)

    def kernel(i):
        a, v, ln = ins[i]
        rc = lib.gdkvm_lv_beats(a.data_ptr(), v.data_ptr(), ln.data_ptr(), beats.data_ptr(), val.data_ptr(), info.data_ptr(), summ.data_ptr(),
                                clips, T, 16, 20, 500, 1, st)
        assert rc == 0, lib.gdkvm_last_error()

    def host(i):
        a, v, ln = (x.cpu().numpy() for x in ins[i])
        out = []
        for b in range(clips):
            ab, vb = a[b, :ln[b]], v[b, :ln[b]]
            es, _ = find_peaks(-ab.astype(np.float64), distance=20, prominence=0.5 * float(ab.max() - ab.min()))
            efs, prev = [], -1
            for j, e in enumerate(es):
                ed = prev + 1 + int(np.argmax(ab[prev + 1:e]))
                if not (j == 0 and ed == 0):
                    efs.append((vb[ed] - vb[e]) / vb[ed] if vb[ed] else 0.0)
                prev = int(e)
            out.append((len(es), float(np.mean(efs)) if efs else 0.0))
        return out

    kernel(0)
    torch.cuda.synchronize()
    want = host(0)                                                 # the yardstick computes the same beats (no ties on these curves)
    assert [w[0] for w in want] == info[:, 1].tolist(), (want, info[:, 1].tolist())
    assert np.allclose([w[1] for w in want], summ[:, 0].cpu().numpy(), rtol=1e-12, atol=0.0)
    t_k, t_h = [], []
    for r in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            kernel(r % n_in)
        e1.record()
        e1.synchronize()
        t0 = time.perf_counter()
        host(r % n_in)
        dt = time.perf_counter() - t0
        if r >= 3:
            t_k.append(e0.elapsed_time(e1) * 1e3 / CALLS)
            t_h.append(dt * 1e6)
    print(f"(e) lv_beats, {clips} clips of {T} frames ({float(info[:, 1].float().mean()):.1f} end-systoles, {float(info[:, 0].float().mean()):.1f} counted beats "
          f"per clip): us per call, median / minimum of {reps} windows ({n_in} inputs in rotation)")
    print(f"{'form':64s} {'median us':>10s} {'min us':>9s}")
    print(f"{'gdkvm_lv_beats (' + str(CALLS) + ' launches per window of device events)':64s} {statistics.median(t_k):10.1f} {min(t_k):9.1f}")
    print(f"{'.cpu() + scipy.signal.find_peaks + host loop (host clock)':64s} {statistics.median(t_h):10.1f} {min(t_h):9.1f}")
    print(flush=True)


def torch_native(mask, sizes, ncls, target, offsets):
    """ops.mask_to_native as a plain torch expression (the yardstick): per clip a one-hot, F.interpolate (bilinear, half-pixel centres), an
    argmax and the three counts per class and frame.  fp32 planes: it answers differently where the votes tie or nearly do."""
    T = mask.shape[1]
    cls = torch.arange(ncls, dtype=torch.uint8, device=mask.device)
    outs, counts = [], []
    for b, (h0, w0) in enumerate(sizes):
        oh = (mask[b].unsqueeze(1) == cls[None, :, None, None]).to(torch.float32)                    # [T, ncls, H, W]
        o = torch.nn.functional.interpolate(oh, size=(h0, w0), mode="bilinear", align_corners=False).argmax(1).to(torch.uint8)
        g = target[offsets[b]:offsets[b] + T * h0 * w0].view(T, 1, h0, w0)
        eo, et = o.unsqueeze(1) == cls[None, :, None, None], g == cls[None, :, None, None]
        counts.append(torch.stack([(eo & et).sum((2, 3)), eo.sum((2, 3)), et.sum((2, 3))], -1))
        outs.append(o.reshape(-1))
    return torch.cat(outs), torch.stack(counts)


def part_n(dev, clips, T, S, ncls, reps, n_in=2):
    """(n) gdkvm_mask_to_native: `clips` clips of T frames of S x S with ncls classes taken to 549 x 778 each, and to mixed CAMUS-like
    sizes, with a native target, through the C symbol on preallocated outputs, beside two yardsticks in the same alternated windows: the
    torch expression of the same resize and counts, and the byte floor -- the source read, the native masks written and the native target
    read once each -- over the HBM rate this probe quotes everywhere."""
    lib = ops.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    mixed = [(549, 778), (1181, 972), (843, 512), (300, 400), (487, 823), (708, 1050), (584, 439), (967, 601)]
    for label, sizes in (("549 x 778", [(549, 778)] * clips), ("mixed sizes", [mixed[b % len(mixed)] for b in range(clips)])):
        masks = [drifting_masks(clips, T, S, ncls, s, dev) for s in range(n_in)]
        for m in masks:                                            # (the vote's flicker is no prediction: keep the drawing, drop the noise)
            m.copy_(ops.temporal_vote(m, ncls, 2)[0])
        host = torch.tensor(sizes, dtype=torch.int32)
        offsets, total = [], 0
        for h0, w0 in sizes:
            offsets.append(total)
            total += T * h0 * w0
        # the target: the next input's masks at the native size, so that prediction and tracing are close to each other
        targets = [ops.mask_to_native(masks[(i + 1) % n_in], sizes, ncls)[0] for i in range(n_in)]
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        counts = torch.empty((clips, T, ncls, 3), dtype=torch.int32, device=dev)

        def mn(i, want_out=True, target=True):
            rc = lib.gdkvm_mask_to_native(masks[i].data_ptr(), host.data_ptr(), targets[i].data_ptr() if target else None,
                                          out.data_ptr() if want_out else None, counts.data_ptr() if target else None, total, None, 0,
                                          clips, T, S, S, ncls, st)
            assert rc == 0, lib.gdkvm_last_error()

        mn(0)
        t_out, t_counts = torch_native(masks[0], sizes, ncls, targets[0], offsets)
        torch.cuda.synchronize()
        differ = int((t_out != out).sum())
        print(f"    ({label}: the torch expression differs from the kernel in {differ} of {total} pixels (fp32 planes against exact votes); "
              f"counts {'equal' if torch.equal(t_counts.to(torch.int32), counts) else 'differ accordingly'})")
        src = masks[0].numel()
        forms = {
            "mask_to_native, out and counts": (lambda i: mn(i), CALLS, src + 2 * total),
            "mask_to_native, counts only": (lambda i: mn(i, want_out=False), CALLS, src + total),
            "mask_to_native, out only": (lambda i: mn(i, target=False), CALLS, src + total),
            "torch expression (one-hot, interpolate, argmax)": (lambda i: torch_native(masks[i], sizes, ncls, targets[i], offsets), 1, src + 2 * total),
        }
        times = {name: [] for name in forms}
        for rep in range(reps + 3):
            for name, (fn, calls, _) in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn(rep % n_in)
                e1.record()
                e1.synchronize()
                if rep >= 3:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / calls)
        print(f"(n) mask_to_native, {clips} clips of {T} frames of {S}x{S} to {label}, {ncls} classes, {total / 1e6:.1f} MB of native labels: us per call, "
              f"windows of device events, median / minimum of {reps} windows per form (alternated, {n_in} inputs in rotation)")
        print(f"{'form':52s} {'median us':>10s} {'min us':>9s} {'MB':>8s} {'floor us':>9s} {'x floor':>8s}")
        for name, (_, _, nbytes) in forms.items():
            med, floor = statistics.median(times[name]), nbytes / HBM * 1e6
            print(f"{name:52s} {med:10.1f} {min(times[name]):9.1f} {nbytes / 1e6:8.1f} {floor:9.2f} {med / floor:8.1f}")
        print(flush=True)


def torch_area(flat, sizes, offsets, T, S, dtype):
    """The nearest torch expression of ops.frames_from_native: per clip F.adaptive_avg_pool2d of the float frames to S x S, rounded to bytes,
    scaled by 1 / 255 into three planes of `dtype`.  Not the same rule at ratios that are no whole number: a window's pixels count equally."""
    out = torch.empty((len(sizes), T, 3, S, S), dtype=dtype, device=flat.device)
    for b, (h0, w0) in enumerate(sizes):
        v = flat[offsets[b]:offsets[b] + T * h0 * w0].view(T, 1, h0, w0).to(torch.float32)
        q = torch.floor(torch.nn.functional.adaptive_avg_pool2d(v, (S, S)) + 0.5)
        out[b] = (q * (1.0 / 255.0)).expand(T, 3, S, S)
    return out


def part_i(dev, clips, T, S, reps, n_in=2):
    """(i) gdkvm_frames_from_native: `clips` clips of T frames of 549 x 778 each, and of mixed CAMUS-like sizes, taken to S x S in three planes,
    through the C symbol on preallocated outputs, beside the torch expression above in the same alternated windows and the byte floor -- the
    native bytes read and the output written once each -- over the HBM rate this probe quotes everywhere."""
    lib = ops.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    mixed = [(549, 778), (1181, 972), (843, 512), (300, 400), (487, 823), (708, 1050), (584, 439), (967, 601)]
    for label, sizes in (("549 x 778", [(549, 778)] * clips), ("mixed sizes", [mixed[b % len(mixed)] for b in range(clips)])):
        host = torch.tensor(sizes, dtype=torch.int32)
        offsets, total = [], 0
        for h0, w0 in sizes:
            offsets.append(total)
            total += T * h0 * w0
        gen = torch.Generator(device=dev).manual_seed(7)
        flats = [torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n_in)]
        outs = {dt: torch.empty((clips, T, 3, S, S), dtype=dt, device=dev) for dt in (torch.bfloat16, torch.uint8)}
        code = {torch.uint8: 0, torch.bfloat16: 2}

        def fn(i, dt):
            rc = lib.gdkvm_frames_from_native(flats[i].data_ptr(), host.data_ptr(), outs[dt].data_ptr(), total, None, 0, clips, T, 3, S, S, code[dt], st)
            assert rc == 0, lib.gdkvm_last_error()

        fn(0, torch.uint8)
        t_out = torch_area(flats[0], sizes, offsets, T, S, torch.float32)
        torch.cuda.synchronize()
        differ = int(((t_out * 255.0).round().to(torch.uint8) != outs[torch.uint8]).sum())
        print(f"    ({label}: the torch expression differs from the kernel in {differ} of {outs[torch.uint8].numel()} bytes: adaptive_avg_pool2d is "
              f"not the area rule at ratios that are no whole number)")
        n_out = clips * T * 3 * S * S
        forms = {
            "frames_from_native, 3 planes bf16": (lambda i: fn(i, torch.bfloat16), CALLS, total + 2 * n_out),
            "frames_from_native, 3 planes uint8": (lambda i: fn(i, torch.uint8), CALLS, total + n_out),
            "torch expression (adaptive_avg_pool2d, cast), bf16": (lambda i: torch_area(flats[i], sizes, offsets, T, S, torch.bfloat16), 1, total + 2 * n_out),
        }
        times = {name: [] for name in forms}
        for rep in range(reps + 3):
            for name, (f, calls, _) in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    f(rep % n_in)
                e1.record()
                e1.synchronize()
                if rep >= 3:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / calls)
        print(f"(i) frames_from_native, {clips} clips of {T} frames of {label} to {S}x{S}, {total / 1e6:.1f} MB of native bytes: us per call, "
              f"windows of device events, median / minimum of {reps} windows per form (alternated, {n_in} inputs in rotation)")
        print(f"{'form':52s} {'median us':>10s} {'min us':>9s} {'MB':>8s} {'floor us':>9s} {'x floor':>8s}")
        for name, (_, _, nbytes) in forms.items():
            med, floor = statistics.median(times[name]), nbytes / HBM * 1e6
            print(f"{name:52s} {med:10.1f} {min(times[name]):9.1f} {nbytes / 1e6:8.1f} {floor:9.2f} {med / floor:8.1f}")
        print(flush=True)


def torch_overlay(grey, mask, ref, sizes, offsets, T, ncls, width, alpha, pal, rpal):
    """ops.overlay_native as a plain torch expression on the device (the yardstick): per clip the 2 w (w + 1) shifted compares of the
    zero-padded masks, the palettes gathered by class, the integer blend and three torch.where in the rule's order."""
    out = torch.empty(3 * grey.numel(), dtype=torch.uint8, device=grey.device)

    def contour(m):
        h0, w0 = m.shape[1:]
        p = torch.nn.functional.pad(m, (width, width, width, width))
        same = torch.ones_like(m, dtype=torch.bool)
        for dy in range(-width, width + 1):
            r = width - abs(dy)
            for dx in range(-r, r + 1):
                if dy or dx:
                    same &= p[:, width + dy:width + dy + h0, width + dx:width + dx + w0] == m
        return (m >= 1) & (m < ncls) & ~same

    for b, (h0, w0) in enumerate(sizes):
        sl = slice(offsets[b], offsets[b] + T * h0 * w0)
        g, m = grey[sl].view(T, h0, w0), mask[sl].view(T, h0, w0)
        g3 = g.to(torch.int32)[..., None].expand(T, h0, w0, 3)
        cls = (m >= 1) & (m < ncls)
        colour = pal[torch.where(cls, m, torch.zeros_like(m)).long()]
        o = torch.where(cls[..., None], (g3 * (256 - alpha) + colour * alpha + 128) >> 8, g3)
        if ref is not None:
            r = ref[sl].view(T, h0, w0)
            on_r = contour(r)
            o = torch.where(on_r[..., None], rpal[torch.where(on_r, r, torch.zeros_like(r)).long()], o)
        o = torch.where(contour(m)[..., None], colour, o)
        out[3 * sl.start:3 * sl.stop] = o.to(torch.uint8).reshape(-1)
    return out


def part_o(dev, clips, T, S, ncls, reps, n_in=2):
    """(o) gdkvm_overlay_native: `clips` clips of T frames of 549 x 778 each, and of mixed CAMUS-like sizes -- random grey bytes under
    ventricle-like masks (drifting ellipses drawn at S x S, voted and taken to the native size by ops.mask_to_native; the reference is the
    next input's mask, so the two contours lie close) -- through the C symbol on a preallocated out, with and without the reference, at
    contour widths 1 and 3, beside the torch expression of the same rule in the same alternated windows and the byte floor: grey, mask and
    reference read and three bytes per pixel written once each over the HBM rate this probe quotes everywhere.  The kernel writes a
    preallocated out; the torch expression allocates its result and its intermediates inside its timed window, as a plain torch expression
    does, and `x torch` is the ratio to that."""
    lib = ops.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    alpha = 96
    pal_h = torch.tensor(ops.OVERLAY_PALETTE[:ncls], dtype=torch.uint8)
    rpal_h = torch.tensor(ops.OVERLAY_REFERENCE_PALETTE[:ncls], dtype=torch.uint8)
    pal_d, rpal_d = pal_h.to(dev).to(torch.int32), rpal_h.to(dev).to(torch.int32)
    mixed = [(549, 778), (1181, 972), (843, 512), (300, 400), (487, 823), (708, 1050), (584, 439), (967, 601)]
    for label, sizes in (("549 x 778", [(549, 778)] * clips), ("mixed sizes", [mixed[b % len(mixed)] for b in range(clips)])):
        host = torch.tensor(sizes, dtype=torch.int32)
        offsets, total = [], 0
        for h0, w0 in sizes:
            offsets.append(total)
            total += T * h0 * w0
        grid = [drifting_masks(clips, T, S, ncls, s, dev) for s in range(n_in)]
        masks = [ops.mask_to_native(ops.temporal_vote(m, ncls, 2)[0], sizes, ncls)[0] for m in grid]
        gen = torch.Generator(device=dev).manual_seed(11)
        greys = [torch.randint(0, 256, (total,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n_in)]
        out = torch.empty(3 * total, dtype=torch.uint8, device=dev)
        drawn = sum(int(((m >= 1) & (m < ncls)).sum()) for m in masks) / (n_in * total)

        def ov(i, width, ref):
            rc = lib.gdkvm_overlay_native(greys[i].data_ptr(), masks[i].data_ptr(), masks[(i + 1) % n_in].data_ptr() if ref else None,
                                          host.data_ptr(), pal_h.data_ptr(), rpal_h.data_ptr(), out.data_ptr(), total, None, 0, clips, T, ncls,
                                          width, alpha, st)
            assert rc == 0, lib.gdkvm_last_error()

        def tov(i, width, ref):
            return torch_overlay(greys[i], masks[i], masks[(i + 1) % n_in] if ref else None, sizes, offsets, T, ncls, width, alpha, pal_d, rpal_d)

        for width, ref in ((1, False), (3, True)):
            ov(0, width, ref)
            differ = int((tov(0, width, ref) != out).sum())
            torch.cuda.synchronize()
            if differ:                                             # no table from a yardstick that draws something else
                raise SystemExit(f"lv_probe --overlay: the torch expression differs from the kernel in {differ} of {3 * total} bytes "
                                 f"({label}, width {width}, {'with' if ref else 'no'} reference)")
            print(f"    ({label}, width {width}, {'with' if ref else 'no'} reference: the torch expression differs from the kernel in {differ} of "
                  f"{3 * total} bytes)")
        forms = {}
        for ref in (False, True):
            for width in (1, 3):
                tag = f"width {width}, {'reference' if ref else 'no reference'}"
                nbytes = (3 if ref else 2) * total + 3 * total
                forms["overlay_native, " + tag] = (lambda i, w=width, r=ref: ov(i, w, r), CALLS, nbytes)
                forms["torch expression, " + tag] = (lambda i, w=width, r=ref: tov(i, w, r), 1, nbytes)
        times = {name: [] for name in forms}
        for rep in range(reps + 3):
            for name, (fn, calls, _) in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn(rep % n_in)
                e1.record()
                e1.synchronize()
                if rep >= 3:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / calls)
        print(f"(o) overlay_native, {clips} clips of {T} frames of {label}, {ncls} classes, {total / 1e6:.1f} MB of native pixels, {100 * drawn:.1f} % "
              f"of them of a drawn class: us per call, windows of device events, median / minimum of {reps} windows per form (alternated, "
              f"{n_in} inputs in rotation)")
        print(f"{'form':52s} {'median us':>10s} {'min us':>9s} {'MB':>8s} {'floor us':>9s} {'x floor':>8s} {'x torch':>8s}")
        for name, (_, _, nbytes) in forms.items():
            med, floor = statistics.median(times[name]), nbytes / HBM * 1e6
            ref_t = statistics.median(times[name.replace("overlay_native", "torch expression")])
            print(f"{name:52s} {med:10.1f} {min(times[name]):9.1f} {nbytes / 1e6:8.1f} {floor:9.2f} {med / floor:8.1f} {med / ref_t:8.3f}")
        print(flush=True)


def native_ellipses(sizes, T, seed):
    """Per clip uint8 [T, h0, w0]: one rotated ellipse of class 1 per frame covering about a tenth of it, with a ring of class 2 around it"""
    rng = np.random.default_rng(seed)
    out = []
    for h0, w0 in sizes:
        yy, xx = np.mgrid[0:h0, 0:w0].astype(np.float32)
        m = np.zeros((T, h0, w0), np.uint8)
        for t in range(T):
            th = rng.uniform(-0.5, 0.5)
            la, sa = rng.uniform(0.22, 0.30), rng.uniform(0.10, 0.14)
            dx, dy = xx / w0 - rng.uniform(0.45, 0.55), yy / h0 - rng.uniform(0.45, 0.55)
            al, ac = dx * math.sin(th) + dy * math.cos(th), dx * math.cos(th) - dy * math.sin(th)
            d = (al / la) ** 2 + (ac / sa) ** 2
            m[t][d <= 1.5] = 2
            m[t][d <= 1.0] = 1
        out.append(m)
    return out


def native_islands(clips, seed):
    """Three discs of class 1 per frame near the corners of every clip's frames (add_islands at native sizes)"""
    rng = np.random.default_rng(seed)
    out = []
    for m in clips:
        T, h0, w0 = m.shape
        yy, xx = np.mgrid[0:h0, 0:w0]
        m = m.copy()
        for t in range(T):
            for _ in range(3):
                cy, cx = ((rng.uniform(0.04, 0.16) if rng.random() < 0.5 else rng.uniform(0.84, 0.96)) * n for n in (h0, w0))
                m[t][(yy - cy) ** 2 + (xx - cx) ** 2 <= (rng.uniform(0.01, 0.05) * min(h0, w0)) ** 2] = 1
        out.append(m)
    return out


def part_s(dev, clips, T, reps, once=False):
    """(s) gdkvm_surface_distance_native: `clips` clips of T native frames, through the C symbol on a preallocated workspace, beside
    gdkvm_surface_distance_mm on the uniform batch and the byte floor (mask + target read once) in the same alternated windows."""
    lib = ops.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    ry, rx = 308, 154
    mixed = [(549, 778), (1181, 972), (843, 512), (300, 400), (487, 823), (708, 1050), (584, 439), (967, 601)]
    flat = lambda cl: torch.from_numpy(np.concatenate([c.reshape(-1) for c in cl])).to(dev)
    for label, sizes in (("549 x 778", [(549, 778)] * clips), ("mixed sizes", [mixed[b % len(mixed)] for b in range(clips)])):
        uniform = len(set(sizes)) == 1
        base = native_ellipses(sizes, T, 1)
        shifted = [np.roll(c, (7, -5), (1, 2)) for c in base]
        pred, tgt, isl = flat(base), flat(shifted), flat(native_islands(base, 2))
        total, rows = pred.numel(), T * sum(h0 for h0, _ in sizes)
        host_sz = torch.tensor(sizes, dtype=torch.int32)
        host_sp = torch.tensor([(ry, rx)] * clips, dtype=torch.int32)
        need = lib.gdkvm_surface_distance_native_workspace_bytes(clips, T, total, rows)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        surf = torch.empty((clips, T, 8), dtype=torch.int64, device=dev)

        def sn(m, g, cls=1):
            rc = lib.gdkvm_surface_distance_native(m.data_ptr(), g.data_ptr(), host_sz.data_ptr(), host_sp.data_ptr(), surf.data_ptr(), total,
                                                   ws.data_ptr(), need, clips, T, cls, st)
            assert rc == 0, lib.gdkvm_last_error()

        forms = {
            "surface_distance_native, ellipse against a shifted copy": (lambda: sn(pred, tgt), 5),
            "surface_distance_native, with islands against the ellipse": (lambda: sn(isl, pred), 5),
            "surface_distance_native, empty class": (lambda: sn(pred, tgt, 3), 5),
        }
        if uniform:
            h0, w0 = sizes[0]
            need_mm = lib.gdkvm_surface_distance_mm_workspace_bytes(clips * T, h0, w0)
            ws_mm = torch.empty(max(need_mm, 16), dtype=torch.uint8, device=dev)
            sp_dev = torch.tensor([(ry, rx)] * (clips * T), dtype=torch.int32, device=dev)
            surf_mm = torch.empty((clips, T, 8), dtype=torch.int64, device=dev)

            def mm(m, g, cls=1):
                rc = lib.gdkvm_surface_distance_mm(m.data_ptr(), g.data_ptr(), sp_dev.data_ptr(), surf_mm.data_ptr(), ws_mm.data_ptr(), need_mm,
                                                   clips * T, h0, w0, cls, st)
                assert rc == 0, lib.gdkvm_last_error()

            sn(isl, pred); mm(isl, pred)
            torch.cuda.synchronize()
            print(f"    ({label}: the records of surface_distance_mm's workspace form are "
                  f"{'bit-equal' if torch.equal(surf, surf_mm) else 'NOT EQUAL'} to surface_distance_native's)")
            forms["surface_distance_mm (one workgroup per frame), shifted copy"] = (lambda: mm(pred, tgt), 2)
            forms["surface_distance_mm (one workgroup per frame), islands"] = (lambda: mm(isl, pred), 2)
        times = {name: [] for name in forms}
        for rep_ in range(1 if once else reps + 3):
            for name, (fn, calls) in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(1 if once else calls):
                    fn()
                e1.record()
                e1.synchronize()
                if once or rep_ >= 3:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / (1 if once else calls))
        nbytes = 2 * total
        floor = nbytes / HBM * 1e6
        print(f"(s) surface_distance_native, {clips} clips of {T} native frames of {label}, class 1, {ry} x {rx} um, {total / 1e6:.1f} MB of labels "
              f"each side, workspace {need / 1e6:.1f} MB: us per call, windows of device events, median / minimum of {len(next(iter(times.values())))} "
              f"windows per form (alternated)")
        print(f"{'form':62s} {'median us':>10s} {'min us':>9s} {'MB':>8s} {'floor us':>9s} {'x floor':>8s}")
        for name in forms:
            med = statistics.median(times[name])
            print(f"{name:62s} {med:10.1f} {min(times[name]):9.1f} {nbytes / 1e6:8.1f} {floor:9.2f} {med / floor:8.1f}")
        print(flush=True)
    # one moderate pathological frame, once: every pixel of the checkerboard's class is surface, and every walk is as long as the pixel is far
    S = 512
    board = np.zeros((1, S, S), np.uint8)
    board[0, (np.add.outer(np.arange(S), np.arange(S)) % 2) == 0] = 1
    one = np.zeros((1, S, S), np.uint8)
    one[0, S - 1, 0] = 1
    bm, og = flat([board]), flat([one])
    hs, hp = torch.tensor([(S, S)], dtype=torch.int32), torch.tensor([(ry, rx)], dtype=torch.int32)
    need = lib.gdkvm_surface_distance_native_workspace_bytes(1, 1, S * S, S)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    surf = torch.empty((1, 1, 8), dtype=torch.int64, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = lib.gdkvm_surface_distance_native(bm.data_ptr(), og.data_ptr(), hs.data_ptr(), hp.data_ptr(), surf.data_ptr(), S * S, ws.data_ptr(), need,
                                           1, 1, 1, st)
    e1.record()
    e1.synchronize()
    assert rc == 0, lib.gdkvm_last_error()
    print(f"(s) one frame of {S} x {S}, a checkerboard ({int(surf[0, 0, 0])} surface pixels) against a single pixel, ONE call (its first: code "
          f"already loaded by the calls above): {e0.elapsed_time(e1) * 1e3:.1f} us; record {surf[0, 0].tolist()}", flush=True)


def part_l(dev, clips, T, reps, frames_1024, once=False):
    """(l) gdkvm_lv_measure_native (class 1, 20 disks): a CAMUS-like ragged batch beside the byte floor, then the largest shape that
    gdkvm_lv_measure_mm runs too, frames of 1024 x 1024, beside that entry (one workgroup per frame) in the same alternated windows."""
    lib = ops.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    ry, rx, D = 308, 154, 20
    rng = np.random.default_rng(3)
    camus = [(int(rng.integers(584, 1946)), int(rng.integers(323, 1182))) for _ in range(clips)]
    flat = lambda cl: torch.from_numpy(np.concatenate([c.reshape(-1) for c in cl])).to(dev)

    def windows(forms):
        times = {name: [] for name in forms}
        for rep_ in range(1 if once else reps + 3):
            for name, (fn, calls) in forms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(1 if once else calls):
                    fn()
                e1.record()
                e1.synchronize()
                if once or rep_ >= 3:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / (1 if once else calls))
        return times

    for label, sizes, frames in ((f"{clips} clips of {T} frames, sizes drawn between 584 x 323 and 1945 x 1181", camus, T),
                                 (f"{frames_1024} frames of 1024 x 1024", [(1024, 1024)], frames_1024)):
        uniform = len(sizes) == 1
        nclips = len(sizes)
        masks = [flat(native_ellipses(sizes, frames, s)) for s in (1, 2)]
        total = masks[0].numel()
        nbands = frames * sum((h0 + ops.LV_NATIVE_BAND_ROWS - 1) // ops.LV_NATIVE_BAND_ROWS for h0, _ in sizes)
        full = torch.ones(total, dtype=torch.uint8, device=dev)
        host_sz = torch.tensor(sizes, dtype=torch.int32)
        host_sp = torch.tensor([(ry, rx)] * nclips, dtype=torch.int32)
        stats = torch.empty((nclips, frames, 12), dtype=torch.int64, device=dev)
        disks = torch.empty((nclips, frames, D), dtype=torch.int64, device=dev)
        geom = torch.empty((nclips, frames, 6), dtype=torch.float64, device=dev)
        bands = torch.empty((nbands, 8 + D), dtype=torch.int64, device=dev)
        turn = [0]

        def ln(m, cls=1):
            rc = lib.gdkvm_lv_measure_native(m.data_ptr(), host_sz.data_ptr(), host_sp.data_ptr(), stats.data_ptr(), disks.data_ptr(),
                                             geom.data_ptr(), bands.data_ptr(), total, nbands, nclips, frames, cls, D, st)
            assert rc == 0, lib.gdkvm_last_error()

        def rotate(fn):
            def go():
                turn[0] += 1
                fn(masks[turn[0] % 2])
            return go

        forms = {
            "lv_measure_native, ellipse (a tenth of the frame)": (rotate(ln), 5),
            "lv_measure_native, every pixel of the class": (lambda: ln(full), 2),
            "lv_measure_native, no pixel of the class": (lambda: ln(masks[0], 3), 5),
        }
        if uniform:
            sp_dev = torch.tensor([(ry, rx)] * frames, dtype=torch.int32, device=dev)
            s_mm, d_mm, g_mm = torch.empty_like(stats), torch.empty_like(disks), torch.empty_like(geom)

            def mm(m, cls=1):
                rc = lib.gdkvm_lv_measure_mm(m.data_ptr(), sp_dev.data_ptr(), s_mm.data_ptr(), d_mm.data_ptr(), g_mm.data_ptr(), frames, 1024, 1024,
                                             cls, D, st)
                assert rc == 0, lib.gdkvm_last_error()

            ln(masks[0]); mm(masks[0])
            torch.cuda.synchronize()
            same = all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in ((stats, s_mm), (disks, d_mm), (geom, g_mm)))
            print(f"    ({label}: the records of lv_measure_mm are {'bit-equal' if same else 'NOT EQUAL'} to lv_measure_native's)")
            forms["lv_measure_mm (one workgroup per frame), ellipse"] = (rotate(mm), 2)
            forms["lv_measure_mm (one workgroup per frame), every pixel"] = (lambda: mm(full), 1)
        times = windows(forms)
        floor = total / HBM * 1e6
        print(f"(l) lv_measure_native, {label}, class 1, {D} disks, {ry} x {rx} um, {total / 1e6:.1f} MB of labels, {nbands} bands of "
              f"{ops.LV_NATIVE_BAND_ROWS} rows: us per call, windows of device events, median / minimum of {len(next(iter(times.values())))} windows "
              f"per form (alternated); floor = the mask read once per pass over the HBM rate: {floor:.2f} us a pass, three passes {3 * floor:.2f} us")
        print(f"{'form':62s} {'median us':>10s} {'min us':>9s} {'MB':>8s} {'x 3 passes':>11s}")
        for name in forms:
            med = statistics.median(times[name])
            print(f"{name:62s} {med:10.1f} {min(times[name]):9.1f} {total / 1e6:8.1f} {med / (3 * floor):11.1f}")
        if uniform:
            for tag in ("ellipse", "every pixel"):
                a = statistics.median(times[[n for n in forms if n.startswith("lv_measure_native") and tag in n][0]])
                b = statistics.median(times[[n for n in forms if n.startswith("lv_measure_mm") and tag in n][0]])
                print(f"    ({tag}: lv_measure_mm / lv_measure_native = {b / a:.2f})")
        print(flush=True)


def contour_masks(F, S, seed):
    """ellipse_masks with what the contour needs around the cavity: a ring of class 2 (the wall), and class 3 (the atrium) over the lower
    quarter of ellipse and ring, so that the cavity ends in a straight mitral plane"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float32)
    out = np.zeros((F, S, S), np.uint8)
    for f in range(F):
        th = rng.uniform(-0.5, 0.5)
        la, sa = S * rng.uniform(0.22, 0.30), S * rng.uniform(0.10, 0.14)
        dx, dy = xx - S * rng.uniform(0.45, 0.55), yy - S * rng.uniform(0.45, 0.55)
        al, ac = dx * math.sin(th) + dy * math.cos(th), dx * math.cos(th) - dy * math.sin(th)
        d = (al / la) ** 2 + (ac / sa) ** 2
        out[f][d <= 1.5] = 2
        out[f][d <= 1.0] = 1
        out[f][(d <= 1.5) & (al > 0.6 * la)] = 3
    return out


def torch_contour_counts(mask, cls, wall, base):
    """Words 1 .. 8 of ops.lv_contour's record as a plain torch expression (the yardstick): the zero-padded mask compared with the class and
    with the one class of each set, and per set eight shifted ANDs and sums, two per direction"""
    H, W = mask.shape[-2:]
    p = torch.nn.functional.pad(mask, (1, 1, 1, 1))
    c = mask == cls
    out = []
    for other in (wall, base):
        x = p == other
        for (dy, dx) in ((0, 1), (1, 0), (1, 1), (1, -1)):
            a = (c & x[:, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]).sum((1, 2))
            b = (c & x[:, 1 - dy:1 - dy + H, 1 - dx:1 - dx + W]).sum((1, 2))
            out.append(a + b)
    return torch.stack(out, 1)


def part_c(dev, F, S, reps, n_in=4):
    """(c) gdkvm_lv_contour (class 1 against the wall {2} and the base {3}) beside gdkvm_lv_measure on the same masks, the torch expression
    of its eight counts, and the byte floor (every mask byte once over the HBM rate above), in the same alternated windows."""
    lib = ops.load()
    st = torch.cuda.current_stream(dev).cuda_stream
    masks = [torch.from_numpy(contour_masks(F, S, s)).to(dev) for s in range(n_in)]
    full = torch.ones((F, S, S), dtype=torch.uint8, device=dev)
    rec = torch.empty((F, 16), dtype=torch.int64, device=dev)
    stats = torch.empty((F, 12), dtype=torch.int64, device=dev)
    disks = torch.empty((F, 20), dtype=torch.int64, device=dev)
    geom = torch.empty((F, 4), dtype=torch.float64, device=dev)
    spacing = torch.tensor([330, 468], dtype=torch.int32, device=dev).expand(F, 2).contiguous()

    def contour(mask, cls, sp=None, wall=1 << 2, base=1 << 3):
        rc = lib.gdkvm_lv_contour(mask.data_ptr(), None if sp is None else sp.data_ptr(), rec.data_ptr(), F, S, S, cls, wall, base, st)
        assert rc == 0, lib.gdkvm_last_error()

    def lv(mask, cls):
        rc = lib.gdkvm_lv_measure(mask.data_ptr(), stats.data_ptr(), disks.data_ptr(), geom.data_ptr(), F, S, S, cls, 20, st)
        assert rc == 0, lib.gdkvm_last_error()

    contour(masks[0], 1)
    want = torch_contour_counts(masks[0], 1, 2, 3)
    torch.cuda.synchronize()
    if not torch.equal(rec[:, 1:9], want):                         # no table from a yardstick that counts something else
        raise SystemExit("lv_probe --contour: the torch expression differs from the kernel's counts")
    lens = ops.contour_lengths(rec)
    print(f"    (contour: {float(rec[:, 0].float().mean()):.0f} pixels of the class, wall {float(lens[:, 0].mean()):.1f}, base {float(lens[:, 1].mean()):.1f}, "
          f"axis {float(lens[:, 2].mean()):.1f} pixels long on average; the torch expression counts the same)")
    forms = {
        "lv_contour, ventricle": (lambda i: contour(masks[i], 1), CALLS),
        "lv_contour, the same with a spacing": (lambda i: contour(masks[i], 1, spacing), CALLS),
        "lv_contour, no base set": (lambda i: contour(masks[i], 1, None, 1 << 2, 0), CALLS),
        "lv_contour, every pixel of the class": (lambda i: contour(full, 1, None, 1 << 2, 1), CALLS),
        "lv_contour, no pixel of the class": (lambda i: contour(full, 2, None, 1 << 3, 1), CALLS),
        "lv_measure, the same ventricle": (lambda i: lv(masks[i], 1), CALLS),
        "torch expression of the 8 counts": (lambda i: torch_contour_counts(masks[i], 1, 2, 3), 2),
    }
    times = {name: [] for name in forms}
    for r in range(reps + 3):
        for name, (fn, calls) in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn(r % n_in)
            e1.record()
            e1.synchronize()
            if r >= 3:
                times[name].append(e0.elapsed_time(e1) * 1e3 / calls)
    nbytes = F * S * S
    print(f"(c) {F} frames of {S}x{S}: us per launch, windows of device events, median / minimum of {reps} windows per form (alternated, {n_in} "
          f"inputs in rotation); floor = {nbytes / 1e6:.1f} MB over the HBM rate = {nbytes / HBM * 1e6:.2f} us")
    print(f"{'form':48s} {'median us':>10s} {'min us':>9s} {'x floor':>9s} {'x torch':>9s}")
    ref = statistics.median(times["torch expression of the 8 counts"])
    for name in forms:
        med = statistics.median(times[name])
        print(f"{name:48s} {med:10.1f} {min(times[name]):9.1f} {med / (nbytes / HBM * 1e6):9.1f} {med / ref:9.3f}")
    print(flush=True)


def part_b(runs, overrides):
    print(f"(b) eval.py wall time, synthetic split, a fresh process per run ({' '.join(overrides) or 'the shipped configuration'})")
    for run in range(runs):
        for keys in (["data.lv_class=1", "data.lv_keep_largest=0"], ["data.lv_class=1", "data.lv_keep_largest=4"],
                     ["data.lv_class=1", "data.lv_keep_largest=0", "data.lv_fill_holes=4"],
                     ["data.lv_class=1", "data.lv_keep_largest=0", "data.temporal_vote=1"],
                     ["data.lv_class=1", "data.lv_keep_largest=0", "data.surface_class=1"], ["data.lv_class=-1"]):
            t0 = time.perf_counter()
            out = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py")] + keys + overrides, capture_output=True, text=True, timeout=600)
            dt = time.perf_counter() - t0
            if out.returncode != 0:
                print(out.stderr[-2000:])
                raise SystemExit(f"eval.py failed with {' '.join(keys)}")
            print(f"  run {run + 1} {' '.join(keys):66s}: {dt:6.2f} s   {out.stdout.strip().splitlines()[-1]}", flush=True)


def main():
    quick = "--quick" in sys.argv
    ops.require_native()
    dev = torch.device("cuda", torch.cuda.current_device())
    if "--beats" in sys.argv:
        part_e(dev, 16, 512, 5 if quick else 40)
        part_e(dev, 2, 4096, 5 if quick else 40)
        return
    if "--native" in sys.argv:
        part_n(dev, 2 if quick else 16, 3 if quick else 10, 256, 4, 5 if quick else 40)
        return
    if "--native-input" in sys.argv:
        part_i(dev, 2 if quick else 16, 3 if quick else 10, 256, 5 if quick else 40)
        return
    if "--native-surface" in sys.argv:
        part_s(dev, 2 if quick else 16, 3 if quick else 10, 3 if quick else 20, once="--once" in sys.argv)
        return
    if "--native-lv" in sys.argv:
        part_l(dev, 2 if quick else 16, 3 if quick else 10, 3 if quick else 20, 4 if quick else 160, once="--once" in sys.argv)
        return
    if "--overlay" in sys.argv:
        part_o(dev, 2 if quick else 16, 3 if quick else 10, 256, 4, 5 if quick else 30)
        return
    if "--contour" in sys.argv:
        for S in (112, 256):
            part_c(dev, 8 if quick else 512, S, 5 if quick else 40)
        return
    if "--mm-only" in sys.argv:
        for S in (112, 256):
            part_a(dev, 8 if quick else 512, S, 5 if quick else 40, only=("lv_measure", "surface_distance"))
        return
    if "--vote-only" not in sys.argv:
        for S in (112, 256):
            part_a(dev, 8 if quick else 512, S, 5 if quick else 40)
    part_v(dev, 2 if quick else 16, 8 if quick else 32, 112, 4, 5 if quick else 40)
    if not quick:                                                  # 20 times the clips: the launcher's other form (16 pixels per lane)
        part_v(dev, 320, 32, 112, 4, 20, n_in=2, torch_rows=False)
    if "--no-eval" not in sys.argv and "--vote-only" not in sys.argv:
        part_b(1 if quick else 2, ["data.size=64", "data.frames=4", "batch_size=4", "model.value_dim=64"] if quick else [])


if __name__ == "__main__":
    main()
