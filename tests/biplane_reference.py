"""Reference of the bi-plane Simpson volume (include/gdkvm.h, gdkvm_lv_biplane) in Python ints and floats, working from the records of
gdkvm_lv_measure_mm (the device's own, or tests/spacing_reference.lv_measure_mm_ref's): the definition's operations in the definition's order
(IEEE fp64, no fused multiply-add).  Below it the `biplane` block of eval.py restated on top of tests/eval_reference.py: clip by clip and pair
by pair over the whole split, with no tables, no batches and no running sums.  Test infrastructure: imports nothing from the product and calls
none of ops.lv_biplane / lv_ef / ef_summary / ef_stats."""
import math

import numpy as np

from tests import eval_reference as E
from tests import lv_reference as LV
from tests import spacing_reference as SP

PI = 3.14159265358979323846


def ellipse_view(H, W, ry, rx, c, s, theta, cy_mm=0.0, cx_mm=0.0):
    """uint8 [H, W]: pixel (y, x) is 1 when its centre, in mm from the frame's centre (moved by cy_mm, cx_mm), lies inside the ellipse of
    semi-axes c (along the direction theta radians from the image's vertical) and s."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    py, px = (yy - (H / 2 - 0.5)) * ry / 1000 - cy_mm, (xx - (W / 2 - 0.5)) * rx / 1000 - cx_mm
    u = py * math.cos(theta) + px * math.sin(theta)
    v = -py * math.sin(theta) + px * math.cos(theta)
    return ((u / c) ** 2 + (v / s) ** 2 <= 1.0).astype(np.uint8)


def biplane_frame_ref(rec_a, rec_b, sp_a, sp_b):
    """One frame of one pair: rec_v = (stats [12], disks [D], geom [6]) of view v, sp_v = (ry, rx) of that frame.  Returns ([V mL, L mm,
    mismatch], npix)."""
    D = len(rec_a[1])
    assert len(rec_b[1]) == D and 1 <= D <= 64
    n = [int(rec_a[0][0]), int(rec_b[0][0])]
    if n[0] <= 0 or n[1] <= 0:
        return [0.0, 0.0, 0.0], 0
    widths, lengths = [], []
    for (stats, disks, geom), (ry, rx), nv in ((rec_a, sp_a, n[0]), (rec_b, sp_b, n[1])):
        Ev, Lv = int(stats[11]), float(geom[0])
        pix = float(int(ry) * int(rx)) / 1e6
        den = float(D * nv * Ev)
        widths.append([(((float(int(w)) / den) * pix) * float(D)) / Lv for w in disks])
        lengths.append(Lv)
    L = max(lengths)
    s = 0.0
    for wa, wb in zip(*widths):
        s = s + wa * wb
    V = (((PI / 4.0) * s) * (L / float(D))) / 1000.0
    return [V, L, (L - min(lengths)) / L], min(n)


def lv_biplane_ref(stats, disks, geom, spacing, pairs):
    """stats [C][T][12], disks [C][T][D], geom [C][T][6], spacing [C][T][2] or [C][2], pairs [P][2].  Returns (out [P][T][3], npix [P][T]);
    a pair that names a clip outside 0 .. C - 1 gives zeros."""
    C = len(stats)
    T = len(stats[0]) if C else 0
    sp = np.broadcast_to(np.asarray(spacing, np.int64).reshape(C, -1, 2), (C, T, 2)) if C else None
    out, npix = [], []
    for a, b in pairs:
        a, b = int(a), int(b)
        rows, ns = [], []
        for t in range(T):
            if not (0 <= a < C and 0 <= b < C):
                o, n = [0.0, 0.0, 0.0], 0
            else:
                o, n = biplane_frame_ref((stats[a][t], disks[a][t], geom[a][t]), (stats[b][t], disks[b][t], geom[b][t]), sp[a, t], sp[b, t])
            rows.append(o)
            ns.append(n)
        out.append(rows)
        npix.append(ns)
    return out, npix


def records_ref(clips, spacing, cls=1, D=20):
    """clips uint8 [C, T, H, W], spacing [C][2] -> (stats [C][T][12], disks [C][T][D], geom [C][T][6]) of spacing_reference.lv_measure_mm_ref."""
    recs = [[SP.lv_measure_mm_ref(f, int(spacing[c][0]), int(spacing[c][1]), cls, D) for f in clips[c]] for c in range(len(clips))]
    return tuple([[r[k] for r in row] for row in recs] for k in ("stats", "disks", "geom"))


def view_pairs_ref(patients, views):
    """([(2CH clip, 4CH clip)] of the patients with both views, in the order the patients first appear; the patients with one view only)."""
    seen = {}
    for i, (p, v) in enumerate(zip(patients, views)):
        seen.setdefault(p, {}).setdefault(v, i)
    pairs = [(v["2CH"], v["4CH"]) for v in seen.values() if "2CH" in v and "4CH" in v]
    return pairs, sum(1 for v in seen.values() if ("2CH" in v) != ("4CH" in v))


def _stated(info, a, b, key):
    for c in (a, b):
        v = (info[c] or {}).get(key)
        if isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v):
            return float(v)
    return None


def _mae_bias(pairs):
    n = max(len(pairs), 1)
    return math.fsum(abs(p - g) for p, g in pairs) / n, math.fsum(p - g for p, g in pairs) / n


def biplane_block_ref(pred, target, *, num_classes, lv_class, keep, fill, fill_max_area, vote, spacing, patients, views, info, clip_range=None):
    """eval.py's `biplane` block: pred, target uint8 [clips, T, H, W]; spacing [clips][2]; patients, views [clips] names; info = None or
    [clips] of dicts / None (CamusPng.info); clip_range = (lo, hi): only those clips were measured (one rank of a larger job before the ranks'
    tables are added: every other clip is an empty record), the pair table is still the whole split's."""
    pred, target = np.asarray(pred), np.asarray(target)
    B, T = pred.shape[:2]
    measured = E.post_process(pred, num_classes=num_classes, lv_class=lv_class, vote=vote, keep=keep, fill=fill, fill_max_area=fill_max_area)["measured"]
    if clip_range is not None:                               # the chain works clip by clip: blanking afterwards is what an unmeasured clip is
        out_of = [c for c in range(B) if not clip_range[0] <= c < clip_range[1]]
        measured, target = measured.copy(), target.copy()
        measured[out_of], target[out_of] = 255, 255
    pairs, single = view_pairs_ref(patients, views)
    p_out, p_np = lv_biplane_ref(*records_ref(measured, spacing, lv_class), spacing, pairs)
    g_out, g_np = lv_biplane_ref(*records_ref(target, spacing, lv_class), spacing, pairs)
    rows = []                                                # per pair with a target: (pair, predicted [EDV, ESV, EF], target's, mismatch at ED)
    for k in range(len(pairs)):
        g_vol, p_vol = [o[0] for o in g_out[k]], [o[0] for o in p_out[k]]
        idx, ref = LV.lv_ef_ref([g_vol], [g_np[k]])
        if idx[0][0] < 0 or not ref[0][0] > 0:
            continue
        _, got = LV.lv_ef_ref([p_vol], [p_np[k]], pick_vol=[g_vol], pick_npix=[g_np[k]])
        rows.append((k, got[0], ref[0], p_out[k][idx[0][0]][2]))
    blk = {"pairs": len(pairs), "patients_single_view": single, "pairs_with_target": len(rows)}
    blk.update(E.compare([(p[2], g[2]) for _, p, g, _ in rows]))
    for name, j in (("edv", 0), ("esv", 1)):
        blk[f"{name}_mae_ml"], blk[f"{name}_bias_ml"] = _mae_bias([(p[j], g[j]) for _, p, g, _ in rows])
    blk["length_mismatch_mean"] = math.fsum(m for *_, m in rows) / max(len(rows), 1)
    blk["pairs_length_mismatch_over_10pct"] = sum(1 for *_, m in rows if m > 0.1)
    blk = {k: E.r5(v) for k, v in blk.items()}
    if info is not None:
        ef = [(p, g, _stated(info, *pairs[k], "ef_percent")) for k, p, g, _ in rows]
        ef = [(p, g, f / 100.0) for p, g, f in ef if f is not None]
        st = E.compare([(p[2], f) for p, _, f in ef])
        vs = {"pairs_with_ef": len(ef), "ef_mae": st["ef_mae"], "ef_bias": st["ef_bias"], "ef_pearson_r": st["ef_pearson_r"],
              "target_ef_mae": _mae_bias([(g[2], f) for _, g, f in ef])[0]}
        for name, j in (("edv", 0), ("esv", 1)):
            vv = [(p, g, _stated(info, *pairs[k], f"{name}_ml")) for k, p, g, _ in rows]
            vv = [(p, g, f) for p, g, f in vv if f is not None]
            vs[f"pairs_with_{name}"] = len(vv)
            vs[f"{name}_mae_ml"], vs[f"{name}_bias_ml"] = _mae_bias([(p[j], f) for p, _, f in vv])
            vs[f"target_{name}_mae_ml"] = _mae_bias([(g[j], f) for _, g, f in vv])[0]
        blk["vs_file"] = {k: E.r5(v) for k, v in vs.items()}
    return blk
