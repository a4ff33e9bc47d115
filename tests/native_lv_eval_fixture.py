"""The split of tests/native_surface_eval_fixture.py (native_eval_fixture's prescribed predictions and native targets of five sizes, with a
spacing of the NATIVE pixel per clip) for the comparison of eval.py's native.lv block with a CPU restatement built from
tests/native_lv_reference.py: the prediction -- post-processed by the references of the clean-up kernels when a clean-up is on -- taken to
every clip's native size by native_reference's rule, measured there clip by clip against the native target, ED / ES picked on the target's
curve.  Test infrastructure: imports nothing from the product."""
import math

from tests import eval_reference as ER
from tests import lv_reference as LV
from tests import native_eval_fixture as F
from tests import native_lv_reference as NL
from tests import native_reference as R
from tests.native_surface_eval_fixture import SPACING, write_split  # noqa: F401  (the tree is that fixture's)

CLS = F.PARAMS["lv_class"]


def _curves(clip, sp):
    ms = [NL.measure(f, int(sp[0]), int(sp[1]), CLS) for f in clip]
    return [m["stats"][0] for m in ms], [m["geom"][1] for m in ms]


def block(clip_range=None, unit="mL", **over):
    """The native.lv block of the clips lo .. hi - 1; unit "px3" measures at 1000 x 1000 um and reports the EF alone."""
    fx, p = F.build(), {**F.PARAMS, **over}
    lo, hi = clip_range or (0, F.CLIPS)
    pred = fx["pred"][lo:hi]
    if p["vote"] or p["keep"] or p["fill"]:
        pred = ER.post_process(pred, **p)["measured"]
    flat, sizes = R.pack(fx["native"][lo:hi])
    out, _ = R.mask_to_native(pred, sizes, F.NCLS, flat)
    offs, _ = R.offsets(sizes, F.T)
    sp = SPACING[lo:hi] if unit == "mL" else [(1000, 1000)] * (hi - lo)
    rows = []
    for b, (o, (h0, w0)) in enumerate(zip(offs, sizes)):
        t_n, t_v = _curves(fx["native"][lo + b], sp[b])
        p_n, p_v = _curves(out[o:o + F.T * h0 * w0].reshape(F.T, h0, w0), sp[b])
        idx, ref = LV.lv_ef_ref([t_v], [t_n])
        if idx[0][0] < 0 or not ref[0][0] > 0:
            continue                                          # fewer than two frames with the class, or no volume: the clip has no EF
        _, got = LV.lv_ef_ref([p_v], [p_n], pick_vol=[t_v], pick_npix=[t_n])
        rows.append((got[0], ref[0]))
    blk = ER.compare([(g[2], r[2]) for g, r in rows])
    if unit == "mL":
        for name, k in (("edv", 0), ("esv", 1)):
            err = [g[k] - r[k] for g, r in rows]
            blk[f"{name}_mae_ml"] = math.fsum(abs(e) for e in err) / max(len(err), 1)
            blk[f"{name}_bias_ml"] = math.fsum(err) / max(len(err), 1)
    return {**{k: ER.r5(v) for k, v in blk.items()}, "unit": unit, "frames": (hi - lo) * F.T}
