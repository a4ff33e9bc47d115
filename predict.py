#!/usr/bin/env python3
"""Prediction entry point: native-size clips in, masks at every clip's own frame size and one JSON report out (gdkvm_amd.predict).

An input is a .npy file (uint8 [T, h0, w0]), a .npz file (`frames`, optional `spacing_um` = the native micrometres per pixel, rows then
columns) or a directory of native_frame_*.png / frame_*.png (tools/convert_camus.py --native-frames; its spacing.json is rescaled back to the
native pixel).  The frames are area-averaged onto the network's grid on the GPU (ops.frames_from_native), segmented as eval.py segments,
post-processed as the configuration says (data.temporal_vote, data.lv_keep_largest, data.lv_fill_holes), taken back to the native size
(ops.mask_to_native) and, with data.lv_class >= 0, measured: ED / ES frames, volumes and EF per clip, beat by beat with data.lv_beats, in mL
with a spacing; with data.native_lv (which the configuration accepts with data.native_eval and data.lv_class >= 0) also at the native size,
on the native masks themselves with the native spacing (`lv_native` per clip, ops.lv_measure_native).  Written: <out>/<name>/mask_XXX.png (class indices, native size) and <out>/report.json, which is also printed; with --overlay also
<out>/<name>/overlay_XXX.png, the picture to look at: the native frame in grey, the predicted classes tinted and their contours opaque
(ops.overlay_native on the GPU; colours, tint and contour width: the configuration's overlay: section).  The fourth member of the native
family, ops.surface_distance_native (HD, HD95 and ASSD in mm at native size), measures a mask against a tracing: a prediction has none, so
it adds nothing here and is eval.py's (data.native_surface_class).

    python predict.py --config config/config_gdkvm_01.yaml --weights outputs/gdkvm_step3000.pth [--ema] [--overlay] --out DIR INPUT... [key=value ...]"""
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

if __name__ == "__main__":
    from gdkvm_amd.predict import main
    main()
