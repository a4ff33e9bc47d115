"""The contour record without a GPU: tests/contour_reference.py against things it shares no code with (a pure-Python loop over pixel x 8
neighbours, np.diff transition counts, closed-form perimeters of discs and ellipses), the CPU path of ops.lv_contour bit for bit against the
reference, ops.contour_lengths and ops.lv_strain against their restatements, the configuration keys, and the synthetic 4-class clips, whose
atrium touches the cavity in diastole only."""
import math

import numpy as np
import pytest
import torch

from gdkvm_amd import ops
from tests import contour_reference as R

BYTES = np.array([0, 1, 2, 3, 4, 40, 255], np.uint8)
NB8 = {(0, 1): 0, (0, -1): 0, (1, 0): 1, (-1, 0): 1, (1, 1): 2, (-1, -1): 2, (1, -1): 3, (-1, 1): 3}       # neighbour offset -> direction


def _loop_counts(mask, cls, wall, base):
    """[n, 4 wall counts, 4 base counts, SX2, SY2] by the definition's second wording: over every cls pixel and each of its 8 neighbours"""
    H, W = mask.shape
    out = [0] * 11
    for y in range(H):
        for x in range(W):
            if mask[y, x] != cls:
                continue
            out[0] += 1
            for (dy, dx), d in NB8.items():
                yy, xx = y + dy, x + dx
                b = int(mask[yy, xx]) if 0 <= yy < H and 0 <= xx < W else 0
                if b in wall:
                    out[1 + d] += 1
                if b in base:
                    out[5 + d] += 1
                    if d < 2:
                        out[9] += x + xx
                        out[10] += y + yy
    return out


def _random_labels(rng, H, W):
    m = rng.choice(BYTES, size=(H, W), p=[0.25, 0.3, 0.15, 0.15, 0.05, 0.05, 0.05])
    m[0, rng.integers(W)] = m[H - 1, rng.integers(W)] = m[rng.integers(H), 0] = m[rng.integers(H), W - 1] = 1     # the class on all four edges
    return m


@pytest.mark.parametrize("wall,base", [((2,), (3,)), ((0, 2), (3, 4)), ((2,), (0,)), ((0,), ())])
def test_the_reference_counts_what_a_loop_over_pixels_and_neighbours_counts(wall, base):
    rng = np.random.default_rng(len(wall) * 7 + len(base))
    for H, W in [(1, 1), (1, 6), (5, 1), (6, 7), (9, 12), (13, 5)]:
        for _ in range(3):
            m = _random_labels(rng, H, W)
            rec = R.contour_ref(m, 1, wall, base)
            loop = _loop_counts(m, 1, wall, base)
            assert rec[:9] == loop[:9], (H, W, m.tolist())
            nb = loop[5] + loop[6]
            if nb:
                assert rec[9:11] == loop[9:11]
                assert rec[11] == math.floor(loop[9] / nb + 0.5) and rec[12] == math.floor(loop[10] / nb + 0.5)      # half up, in half pixels
                cand = [(y, x) for y in range(H) for x in range(W) if m[y, x] == 1]
                d2 = [(2 * y - rec[12]) ** 2 + (2 * x - rec[11]) ** 2 for y, x in cand]
                assert rec[14] == max(d2) and rec[13] == min(y * W + x for (y, x), v in zip(cand, d2) if v == max(d2)) and rec[15] == 0
            else:
                assert rec[9:] == [0, 0, -1, -1, -1, 0, 0]


def test_binary_transition_counts():
    """N_E and N_S of a binary mask against the outside and the background are the class changes along the rows and down the columns"""
    rng = np.random.default_rng(3)
    for H, W in [(1, 9), (8, 1), (11, 14), (32, 32)]:
        m = (rng.random((H, W)) < 0.45).astype(np.uint8)
        rec = R.contour_ref(m, 1, (0,), ())
        p = np.pad(m.astype(np.int64), 1)
        assert rec[1] == int(np.abs(np.diff(p, axis=1)).sum()) and rec[2] == int(np.abs(np.diff(p, axis=0)).sum())
        assert rec[0] == int(m.sum()) and rec[5:] == [0, 0, 0, 0, 0, 0, -1, -1, -1, 0, 0]


# --------------------------------------------------------------------------------------------------------------------- closed forms
# What the reference ALONE measures against the closed forms on the cases below (the worst of each family), and what is asserted: 1.5 x that.
# An estimator that drops a direction or swaps ry and rx is off by 10 % and more.
# Measured: 0.01997 over the discs (R = 6 .. 80), 0.04226 over the ellipses (the worst at 100 x 400 um; 0.0128, 0.0210 and 0.0075 at the other
# three spacings), 0.01807 for the strain of an ellipse against its 0.8-scaled copy (absolute, against -0.2).  Asserted: 0.02996, 0.06339, 0.02711.
MEASURED_DISC, MEASURED_ELLIPSE, MEASURED_STRAIN = 0.01997, 0.04226, 0.01807
SPACINGS = [(330, 468), (468, 330), (100, 400), (1000, 1000)]


def _physical_ellipse(H, W, cy_um, cx_um, a_um, b_um, deg, ry, rx):
    """Binary mask of the pixels whose centre (x rx, y ry) micrometres lies inside the rotated ellipse"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    Y, X = yy * ry - cy_um, xx * rx - cx_um
    t = math.radians(deg)
    u, v = X * math.cos(t) + Y * math.sin(t), -X * math.sin(t) + Y * math.cos(t)
    return ((u / a_um) ** 2 + (v / b_um) ** 2 <= 1.0).astype(np.uint8)


def _outline_um(mask, ry, rx):
    return R.crofton_length(*R.contour_ref(mask, 1, (0,), ())[1:5], ry, rx)


def disc_errors():
    rng = np.random.default_rng(11)
    errs = []
    for Rr in (6, 7, 9, 12, 16, 23, 32, 45, 64, 80):
        for _ in range(3):
            S = 2 * Rr + 6
            c = Rr + 2.5 + rng.random(2)
            m = _physical_ellipse(S, S, c[0], c[1], Rr, Rr, 0.0, 1, 1)
            errs.append(abs(_outline_um(m, 1, 1) / (2 * math.pi * Rr) - 1.0))
    return errs


def ellipse_cases():
    rng = np.random.default_rng(12)
    for ry, rx in SPACINGS:
        for deg in (0, 25, 45, 70, 90, 130):
            a, b = 14000.0 + 4000.0 * rng.random(), 7000.0 + 3000.0 * rng.random()     # semi-axes in micrometres: a ventricle's size
            H, W = int(2 * a / ry) + 8, int(2 * a / rx) + 8
            cy, cx = (H / 2 + rng.random()) * ry, (W / 2 + rng.random()) * rx
            yield ry, rx, H, W, cy, cx, a, b, deg


def ellipse_errors():
    errs, strain = [], []
    for ry, rx, H, W, cy, cx, a, b, deg in ellipse_cases():
        big = _outline_um(_physical_ellipse(H, W, cy, cx, a, b, deg, ry, rx), ry, rx)
        small = _outline_um(_physical_ellipse(H, W, cy, cx, 0.8 * a, 0.8 * b, deg, ry, rx), ry, rx)
        errs.append(abs(big / R.ellipse_perimeter(a, b) - 1.0))
        strain.append(abs((small - big) / big - (-0.2)))
    return errs, strain


def test_lengths_of_discs_and_ellipses_against_their_perimeters():
    d = max(disc_errors())
    e, s = (max(v) for v in ellipse_errors())
    print(f"worst relative error: discs {d:.5f}, ellipses {e:.5f}; worst absolute strain error {s:.5f}")
    assert d <= 1.5 * MEASURED_DISC and e <= 1.5 * MEASURED_ELLIPSE and s <= 1.5 * MEASURED_STRAIN
    # what the bounds tell apart: the same counts with ry and rx swapped, and with the diagonal directions dropped
    ry, rx, H, W, cy, cx, a, b, deg = next(c for c in ellipse_cases() if (c[0], c[1]) == (100, 400))
    n = R.contour_ref(_physical_ellipse(H, W, cy, cx, a, b, deg, ry, rx), 1, (0,), ())[1:5]
    per = R.ellipse_perimeter(a, b)
    assert abs(R.crofton_length(*n, rx, ry) / per - 1.0) > 0.2 and abs(R.crofton_length(n[0], n[1], 0, 0, ry, rx) / per - 1.0) > 0.2
    assert abs(R.crofton_length(4, 4, 4, 4) - (math.pi / 8) * (8 + 8 / math.sqrt(2))) < 1e-12               # the isotropic form


# ------------------------------------------------------------------------------------------------------------- the product's CPU path
def test_ops_lv_contour_on_cpu_tensors_is_the_reference_bit_for_bit():
    rng = np.random.default_rng(5)
    for H, W in [(1, 1), (1, 70), (66, 1), (7, 9), (13, 17), (65, 63), (64, 130)]:
        frames = np.stack([_random_labels(rng, H, W) for _ in range(3)])
        frames[2][frames[2] == 3] = 4                            # no base interface
        for cls, wall, base, sp in [(1, (2,), (3,), None), (1, (0, 2), (3, 4), (468, 330)), (2, (1,), (0,), (100, 4095)), (1, (0,), (), None)]:
            spt = None if sp is None else torch.tensor(sp, dtype=torch.int32)
            got = ops.lv_contour(torch.from_numpy(frames), cls=cls, wall=wall, base=base, spacing_um=spt)
            want = R.contour_ref_frames(frames, cls, wall, base, sp)
            assert got.dtype == torch.int64 and got.shape == (3, 16) and got.numpy().tolist() == want.tolist(), (H, W, cls, wall, base, sp)
            lens = ops.contour_lengths(got, spt).numpy()
            for f in range(3):
                ref = R.lengths_ref(want[f], sp)
                assert np.allclose(lens[f], ref, rtol=1e-12, atol=0.0), (lens[f], ref)
    lead = ops.lv_contour(torch.from_numpy(frames).reshape(1, 3, 64, 130), spacing_um=torch.tensor([[[300, 200]]], dtype=torch.int32))
    assert lead.shape == (1, 3, 16)
    assert ops.lv_contour(torch.zeros((0, 4, 4), dtype=torch.uint8)).shape == (0, 16)
    minus = torch.full((2, 16), -1, dtype=torch.int64)
    assert ops.contour_lengths(minus).tolist() == [[-1.0] * 3] * 2


def test_ops_lv_contour_refuses_bad_arguments():
    m = torch.zeros((2, 4, 4), dtype=torch.uint8)
    for kw, msg in [(dict(cls=32), "cls"), (dict(wall=()), "wall is empty"), (dict(wall=(2, 3)), "overlap"), (dict(wall=(1,)), "holds cls"),
                    (dict(base=(1,)), "holds cls"), (dict(wall=(32,)), "distinct integers"), (dict(wall=(2, 2)), "distinct integers"),
                    (dict(spacing_um=torch.tensor([0, 5], dtype=torch.int32)), "spacing_um outside"),
                    (dict(spacing_um=torch.tensor([5.0, 5.0])), "int32")]:
        with pytest.raises(ops.GdkvmError, match=msg):
            ops.lv_contour(m, **kw)
    with pytest.raises(ops.GdkvmError, match="uint8"):
        ops.lv_contour(m.to(torch.int64))
    with pytest.raises(ops.GdkvmError, match=r"\[\.\.\., 16\]"):
        ops.contour_lengths(torch.zeros((2, 12), dtype=torch.int64))
    assert ops.SIGNATURES["gdkvm_lv_contour"][1][-3:-1] == [__import__("ctypes").c_uint] * 2
    assert (ops.LV_CONTOUR_BAND_ROWS, ops.LV_CONTOUR_WORD_BITS) == (R.BAND_ROWS, R.WORD_BITS)


# --------------------------------------------------------------------------------------------------------------------------- lv_strain
def _strain(length, npix, ed_es, **kw):
    return ops.lv_strain(torch.tensor(length, dtype=torch.float64), torch.tensor(npix, dtype=torch.int64), torch.tensor(ed_es, dtype=torch.int32), **kw)


def test_lv_strain_on_hand_made_curves():
    length = [[10.0, 9.0, 8.0, 8.0, 9.5],       # a plain beat; the peak ties at frames 2 and 3: the lowest wins
              [10.0, 0.0, 7.0, 8.0, 12.0],      # frame 1 has no contour: invalid, and it is not the peak
              [10.0, 9.0, 8.0, 9.0, 10.0],      # ed = -1: no pick
              [10.0, 9.0, 8.0, 9.0, 10.0],      # the picked ES frame is below min_pixels
              [0.0, 9.0, 8.0, 9.0, 10.0]]       # the picked ED frame has no contour
    npix = [[50] * 5, [50, 0, 50, 50, 50], [50] * 5, [50, 50, 3, 50, 50], [50] * 5]
    ed_es = [[0, 2, 5], [0, 3, 4], [-1, -1, 1], [0, 2, 5], [0, 2, 5]]
    curve, gp, frame, ok = _strain(length, npix, ed_es, min_pixels=5)
    assert ok.tolist() == [True, True, False, False, False] and frame.tolist() == [2, 2, -1, -1, -1]
    assert gp[0].tolist() == [-0.2, -0.2, 10.0] and gp[1].tolist() == [(8.0 - 10.0) / 10.0, (7.0 - 10.0) / 10.0, 10.0]
    assert curve[0].tolist() == [0.0, (9.0 - 10.0) / 10.0, -0.2, -0.2, (9.5 - 10.0) / 10.0]
    assert curve[1].tolist() == [0.0, 0.0, (7.0 - 10.0) / 10.0, -0.2, (12.0 - 10.0) / 10.0]
    assert not curve[2:].any() and not gp[2:].any()
    for b in range(5):                                           # and the restatement agrees
        c, gls, peak, led, fr, k = R.strain_ref(length[b], npix[b], ed_es[b][0], ed_es[b][1], min_pixels=5)
        assert (c, [gls, peak, led], fr, k) == (curve[b].tolist(), gp[b].tolist(), int(frame[b]), bool(ok[b]))
    _, gp1, _, ok1 = _strain(length, npix, ed_es)                # min_pixels = 1: clip 3 counts
    assert ok1.tolist() == [True, True, False, True, False] and gp1[3, 0] == -0.2
    with pytest.raises(ops.GdkvmError, match="float64"):
        ops.lv_strain(torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int32))
    with pytest.raises(ops.GdkvmError, match="npix"):
        ops.lv_strain(torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------------ configuration
def test_config_keys_and_their_validation():
    from gdkvm_amd.config import load_config
    cfg = load_config(None, [])
    assert cfg.data.lv_strain is False and cfg.data.lv_wall_classes == [2] and cfg.data.lv_base_classes == [3]
    load_config(None, ["data.num_classes=2"])                    # off: a binary dataset keeps the defaults
    on = load_config(None, ["data.lv_strain=true"])
    assert on.data.lv_strain is True
    load_config(None, ["data.lv_strain=true", "data.num_classes=2", "data.lv_wall_classes=[0]", "data.lv_base_classes=[]"])
    for bad, msg in [(["data.lv_strain=1"], "true or false"), (["data.lv_strain=true", "data.lv_class=-1"], "lv_class >= 0"),
                     (["data.lv_strain=true", "data.num_classes=2"], "classes in 0..1"),
                     (["data.lv_strain=true", "data.lv_wall_classes=[1]"], "other than data.lv_class"),
                     (["data.lv_strain=true", "data.lv_base_classes=[1, 3]"], "other than data.lv_class"),
                     (["data.lv_strain=true", "data.lv_wall_classes=[]"], "lv_wall_classes is empty"),
                     (["data.lv_strain=true", "data.lv_wall_classes=[2, 3]"], "overlap"),
                     (["data.lv_wall_classes=[2, 2]"], "distinct"), (["data.lv_wall_classes=2"], "a list"),
                     (["data.lv_strain=true", "data.lv_base_classes=[4]"], "classes in 0..3")]:
        with pytest.raises(ValueError, match=msg):
            load_config(None, bad)
    import yaml, os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "config_gdkvm_01.yaml")) as f:
        raw = yaml.safe_load(f)["data"]
    assert raw["lv_strain"] is False and raw["lv_wall_classes"] == [2] and raw["lv_base_classes"] == [3]


def test_the_switch_is_off_by_default_in_eval_and_predict():
    """Off by default: eval.py and predict.py touch the new ops only behind data.lv_strain, and the report's keys are added there alone"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for fn, switch in (("eval.py", "st_on"), (os.path.join("gdkvm_amd", "predict.py"), "d.lv_strain")):
        src = open(os.path.join(root, fn)).read()
        body = src[src.index('"""', src.index('"""') + 3) + 3:]  # behind the module's docstring
        for m in re.finditer(r"ops\.(lv_contour|contour_lengths|lv_strain)\(|\[\"strain\"\]", body):
            head = body[:m.start()]
            opened = [ln for ln in head.splitlines() if re.match(rf"\s*if {re.escape(switch)}:", ln)]
            assert opened, (fn, body[m.start() - 80:m.end()])
            indent = len(opened[-1]) - len(opened[-1].lstrip())
            line = body[body.rfind("\n", 0, m.start()) + 1:m.start()]
            assert len(line) - len(line.lstrip()) > indent, (fn, line)
    assert re.search(r"st_on = cfg\.data\.lv_strain\b", open(os.path.join(root, "eval.py")).read())


# ------------------------------------------------------------------------------------------------------------ the synthetic 4-class clips
def test_synthetic_clips_have_a_wall_everywhere_and_a_base_in_diastole_only():
    from gdkvm_amd.data import SyntheticEchoClips
    ds = SyntheticEchoClips(3, 10, 32, num_classes=4, seed=7, as_uint8=True)
    with_base = without = 0
    for i in range(3):
        _, masks = ds[i]
        rec = ops.lv_contour(masks)                              # [T, 16] on the host
        assert rec.numpy().tolist() == R.contour_ref_frames(masks.numpy()).tolist()
        lens = ops.contour_lengths(rec)
        nb = rec[:, 5] + rec[:, 6]
        assert bool((rec[:, 0] > 0).all()) and bool((rec[:, 1:5].sum(1) > 0).all()) and bool((lens[:, 0] > 0).all())
        assert bool(((nb == 0) == (rec[:, 13] == -1)).all()) and bool(((nb == 0) == (lens[:, 2] == 0)).all())
        with_base += int((nb > 0).sum())
        without += int((nb == 0).sum())
        # a clip level pass: the frames without landmarks are invalid for the long axis, and a pick on one of them is not ok
        area = rec[:, 0][None].contiguous()
        ed, es = int(area.argmax()), int(area.argmin())
        picks = torch.tensor([[ed, es, 10]], dtype=torch.int32)
        _, gp, _, ok = ops.lv_strain(lens[:, 0][None].contiguous(), area, picks)
        assert bool(ok[0]) and -0.5 < float(gp[0, 0]) < 0.0       # the contour shortens from the largest to the smallest cavity
        _, ga, _, oka = ops.lv_strain(lens[:, 2][None].contiguous(), area, picks)
        assert bool(oka[0]) == bool(nb[ed] > 0 and nb[es] > 0) and (bool(oka[0]) or float(ga[0, 0]) == 0.0)
    assert with_base > 0 and without > 0
