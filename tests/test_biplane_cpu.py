"""The bi-plane Simpson volume without a device: tests/biplane_reference.py (the definition of gdkvm_lv_biplane in include/gdkvm.h) against the
closed forms of an ellipsoid and of one elliptic cylinder, its identities (a view paired with itself, the views swapped, an empty view), and the
plumbing around the kernel: the converter's info.json, CamusPng.patient / info, view_pair_table, the configuration key and the refusals of
ops.lv_biplane that need no device."""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import biplane_reference as R
from tests import spacing_reference as SP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pair_records(H, W, sp_a, sp_b, c, a, b, D):
    """The two views of the ellipsoid of semi-axes (c, a, b) mm, as one-frame clips: (stats, disks, geom) [2][1][.], spacing [2][2]."""
    views = [R.ellipse_view(H, W, *sp_a, c, a, +0.15), R.ellipse_view(H, W, *sp_b, c, b, -0.10)]
    recs = [SP.lv_measure_mm_ref(m, int(sp[0]), int(sp[1]), 1, D) for m, sp in zip(views, (sp_a, sp_b))]
    return tuple([[r[k]] for r in recs] for k in ("stats", "disks", "geom")), [list(sp_a), list(sp_b)]


# frame, spacing of view a, of view b, (c, a, b) mm, D
ELLIPSOIDS = [((64, 48), (330, 470), (410, 290), (9.0, 4.0, 3.0), 20),
              ((48, 40), (500, 500), (500, 500), (10.0, 5.0, 3.5), 20),
              ((96, 80), (300, 300), (250, 350), (12.0, 6.0, 4.0), 64)]


@pytest.mark.parametrize("case", range(len(ELLIPSOIDS)))
def test_ellipsoid_volume(case):
    """Two ellipses with semi-axes (c, a) and (c, b), tilted by +0.15 and -0.10 rad, are the two orthogonal long-axis sections of an ellipsoid:
    V = 4 pi a b c / 3 within 2 % (discretisation at these sizes; measured +0.98 %, -0.78 %, +0.90 %)."""
    (H, W), sp_a, sp_b, (c, a, b), D = ELLIPSOIDS[case]
    recs, sp = pair_records(H, W, sp_a, sp_b, c, a, b, D)
    out, npix = R.lv_biplane_ref(*recs, sp, [(0, 1)])
    want = 4.0 * math.pi * a * b * c / 3.0 / 1000.0          # mm^3 -> mL
    print(f"ellipsoid {case}: V = {out[0][0][0]:.6f} mL against {want:.6f}: {100 * (out[0][0][0] / want - 1):+.2f} %")
    assert abs(out[0][0][0] / want - 1.0) <= 0.02
    assert npix[0][0] == min(recs[0][0][0][0], recs[0][1][0][0]) > 0
    La, Lb = recs[2][0][0][0], recs[2][1][0][0]
    assert out[0][0][1] == max(La, Lb) and out[0][0][2] == (max(La, Lb) - min(La, Lb)) / max(La, Lb) and 0.0 <= out[0][0][2] < 0.1


def test_one_disk_is_one_elliptic_cylinder():
    """D = 1: the one disk has the ellipses' mean widths pi a / 2 and pi b / 2 and the height 2 c: V = pi^3 a b c / 8 within 2 % (+0.35 %)."""
    (H, W), sp_a, sp_b, (c, a, b), _ = ELLIPSOIDS[0]
    recs, sp = pair_records(H, W, sp_a, sp_b, c, a, b, 1)
    out, _ = R.lv_biplane_ref(*recs, sp, [(0, 1)])
    want = math.pi ** 3 * a * b * c / 8.0 / 1000.0
    print(f"one disk: V = {out[0][0][0]:.6f} mL against {want:.6f}: {100 * (out[0][0][0] / want - 1):+.2f} %")
    assert abs(out[0][0][0] / want - 1.0) <= 0.02


@pytest.mark.parametrize("case", range(len(ELLIPSOIDS)))
def test_self_pair_swap_and_empty_view(case):
    (H, W), sp_a, sp_b, (c, a, b), D = ELLIPSOIDS[case]
    (stats, disks, geom), sp = pair_records(H, W, sp_a, sp_b, c, a, b, D)
    # a third clip: an empty frame
    empty = SP.lv_measure_mm_ref(np.zeros((H, W), np.uint8), 300, 300, 1, D)
    stats, disks, geom, sp = stats + [[empty["stats"]]], disks + [[empty["disks"]]], geom + [[empty["geom"]]], sp + [[300, 300]]
    out, npix = R.lv_biplane_ref(stats, disks, geom, sp, [(0, 0), (1, 1), (0, 1), (1, 0), (0, 2), (2, 1), (2, 2), (0, 3), (-1, 0)])
    # a view paired with itself is the single-plane volume: the same terms in another order of operations, at most 3 * 64 + 8 roundings on
    # positive terms (below 3e-14)
    for k, clip in ((0, 0), (1, 1)):
        single = geom[clip][0][1]
        print(f"self pair of view {clip}: {out[k][0][0]!r} against {single!r}: {abs(out[k][0][0] / single - 1):.2e}")
        assert abs(out[k][0][0] - single) <= 1e-12 * single
        assert out[k][0][1] == geom[clip][0][0] and out[k][0][2] == 0.0 and npix[k][0] == stats[clip][0][0]
    assert out[2] == out[3] and npix[2] == npix[3]           # the product and max / min commute: bit-equal
    for k in (4, 5, 6, 7, 8):                                # an empty view, and clips outside the tables
        assert out[k] == [[0.0, 0.0, 0.0]] and npix[k] == [0]
    # the -1 record of a spacing out of range
    bad = SP.lv_measure_mm_ref(np.ones((H, W), np.uint8), 0, 300, 1, D)
    out, npix = R.lv_biplane_ref([stats[0], [bad["stats"]]], [disks[0], [bad["disks"]]], [geom[0], [bad["geom"]]], [sp[0], [0, 300]], [(0, 1), (1, 0)])
    assert out == [[[0.0, 0.0, 0.0]]] * 2 and npix == [[0], [0]]


def test_the_eval_fixture_holds_what_the_device_test_needs():
    """tests/biplane_eval_fixture.py, with the references only: pairs that straddle the batches, a patient with one view, a pair without a
    target curve, islands that move the block, file values for some pairs, and a range of clips that splits a pair."""
    from tests import biplane_eval_fixture as F
    pairs, single = R.view_pairs_ref(F.PATIENTS, F.VIEWS)
    assert pairs == F.PAIRS and single == 1 and all(a // F.BATCH != b // F.BATCH for a, b in pairs)
    off, on = F.block(keep=0), F.block(keep=4)
    assert list(off) == ["pairs", "patients_single_view", "pairs_with_target", "clips_with_ef", "ef_mae", "ef_bias", "ef_pearson_r", "mean_ref_ef",
                         "mean_pred_ef", "edv_mae_ml", "edv_bias_ml", "esv_mae_ml", "esv_bias_ml", "length_mismatch_mean",
                         "pairs_length_mismatch_over_10pct", "vs_file"]
    assert list(off["vs_file"]) == ["pairs_with_ef", "ef_mae", "ef_bias", "ef_pearson_r", "target_ef_mae", "pairs_with_edv", "edv_mae_ml", "edv_bias_ml",
                                    "target_edv_mae_ml", "pairs_with_esv", "esv_mae_ml", "esv_bias_ml", "target_esv_mae_ml"]
    assert off["pairs"] == 3 and off["pairs_with_target"] == off["clips_with_ef"] == 2 and 0.05 < off["mean_ref_ef"] < 0.8
    assert off["vs_file"]["pairs_with_ef"] == 2 and off["vs_file"]["pairs_with_edv"] == 1 and off["vs_file"]["pairs_with_esv"] == 1
    assert off["edv_mae_ml"] != on["edv_mae_ml"] and off["length_mismatch_mean"] != on["length_mismatch_mean"]     # the islands matter
    part = F.block(clip_range=(0, 4))
    assert part["pairs"] == 3 and part["pairs_with_target"] == 1 and part["vs_file"]["pairs_with_ef"] == 1
    assert F.block(info=None).keys() == off.keys() - {"vs_file"}


# ---- the plumbing ------------------------------------------------------------------------------------------------------------------------------
CFG_OLD = "ED: 1\nES: 17\nNbFrame: 17\nSex: F\nAge: 56\nImageQuality: Good\nLVedv: 94.0\nLVesv: 34.7\nLVef: 63.1\n"
CFG_NEW = "ed: 3\nes: 12\nNBFRAME: 20\nSex: M\nEF: 48.5\nFrameRate: 52.1\nsomething without a colon\n: 5\nLVedv: not a number\n"


def test_parse_info_cfg():
    from tools.convert_camus import parse_info_cfg
    assert parse_info_cfg(CFG_OLD) == {"ef_percent": 63.1, "edv_ml": 94.0, "esv_ml": 34.7, "ed_frame": 1, "es_frame": 17, "nb_frame": 17,
                                       "frame_rate": None}
    assert parse_info_cfg(CFG_NEW) == {"ef_percent": 48.5, "edv_ml": None, "esv_ml": None, "ed_frame": 3, "es_frame": 12, "nb_frame": 20,
                                       "frame_rate": 52.1}
    assert parse_info_cfg("LVef: 60\nEF: 55\n")["ef_percent"] == 60.0        # LVef first
    assert parse_info_cfg("LVef: nan\nEF: 55\nED: 1.5\n") == {**dict.fromkeys(("edv_ml", "esv_ml", "ed_frame", "es_frame", "nb_frame", "frame_rate")),
                                                             "ef_percent": 55.0}
    assert all(v is None for v in parse_info_cfg("").values())


def _camus_tree(src):
    """patient0001 with both views (2CH: the older spelling, 4CH: the newer), patient0002 with both views and no cfg, patient0003 with 4CH only."""
    from tools.convert_camus import write_nifti
    rng = np.random.default_rng(3)
    for pid, views in (("patient0001", ("2CH", "4CH")), ("patient0002", ("2CH", "4CH")), ("patient0003", ("4CH",))):
        (src / pid).mkdir(parents=True)
        for view in views:
            img = rng.integers(0, 255, (24, 30, 2), dtype=np.uint8)
            lab = np.zeros((24, 30, 2), np.uint8)
            lab[8:16, 6:24] = 1
            for name, arr in ((f"{pid}_{view}_half_sequence.nii.gz", img), (f"{pid}_{view}_half_sequence_gt.nii.gz", lab)):
                write_nifti(str(src / pid / name), arr, pixdim=(0.3, 0.3))
    (src / "patient0001" / "Info_2CH.cfg").write_text(CFG_OLD)
    (src / "patient0001" / "Info_4CH.cfg").write_text(CFG_NEW)
    (src / "patient0003" / "Info_4CH.cfg").write_text("EF: 51\n")


def test_info_from_the_cfg_to_the_dataset_and_the_pair_table(tmp_path):
    from gdkvm_amd.data import CamusPng, SyntheticEchoClips, view_pair_table
    from tools.convert_camus import convert
    src, dst = tmp_path / "camus", tmp_path / "png"
    _camus_tree(src)
    logs = []
    assert convert(str(src), str(dst), size=16, frames=2, split="val", log=logs.append) == {"sequences": 5}
    assert len(logs) == 1 and "3 with an info.json" in logs[0]
    with open(dst / "val" / "patient0001" / "2CH" / "info.json") as f:
        assert json.load(f) == {"ef_percent": 63.1, "edv_ml": 94.0, "esv_ml": 34.7, "ed_frame": 1, "es_frame": 17, "nb_frame": 17, "frame_rate": None}
    assert not os.path.exists(dst / "val" / "patient0002" / "2CH" / "info.json")
    ds = CamusPng(str(dst), "val", 2)
    assert [ds.patient(i) for i in range(5)] == ["patient0001"] * 2 + ["patient0002"] * 2 + ["patient0003"]
    assert [ds.view(i) for i in range(5)] == ["2CH", "4CH", "2CH", "4CH", "4CH"]
    assert ds.info(0)["ef_percent"] == 63.1 and ds.info(1)["ef_percent"] == 48.5 and ds.info(1)["edv_ml"] is None
    assert ds.info(2) is None and ds.info(3) is None and ds.info(4)["ef_percent"] == 51.0
    assert not hasattr(ds, "file_ef")                        # eval.py's beats block picks that name up
    (dst / "val" / "patient0002" / "2CH" / "info.json").write_text("[1, 2")
    (dst / "val" / "patient0002" / "4CH" / "info.json").write_text("[1, 2]")
    assert ds.info(2) is None and ds.info(3) is None
    pairs, single = view_pair_table(ds)
    assert pairs.dtype == torch.int32 and pairs.tolist() == [[0, 1], [2, 3]] and single == 1 and not pairs.is_cuda
    assert (pairs.tolist(), single) == (list(map(list, R.view_pairs_ref([ds.patient(i) for i in range(5)], [ds.view(i) for i in range(5)])[0])), 1)
    only4 = CamusPng(str(dst), "val", 2, views=("4CH",))
    pairs, single = view_pair_table(only4)
    assert tuple(pairs.shape) == (0, 2) and pairs.dtype == torch.int32 and single == 3
    assert view_pair_table(SyntheticEchoClips(4, 2, 16)) is None


def test_lv_biplane_config_key():
    from gdkvm_amd.config import load_config
    path = os.path.join(ROOT, "config", "config_gdkvm_01.yaml")
    assert load_config(path).data.lv_biplane is False and load_config(None, []).data.lv_biplane is False
    assert load_config(path, ["data.lv_biplane=true"]).data.lv_biplane is True
    for bad in ("1", "0", "yes please", "[true]", "null"):
        with pytest.raises(ValueError, match="lv_biplane"):
            load_config(path, [f"data.lv_biplane={bad}"])


def test_the_c_entry_checks_its_arguments_before_any_device_call():
    """Return codes that speak about the arguments alone, so they are the same without a device: shapes first (GDKVM_ERR_SHAPE = -1), P == 0
    or T == 0 is GDKVM_OK without a launch (with null pointers), then null and misaligned pointers (GDKVM_ERR_ARG = -6).  The addresses are
    never read: every call returns in front of the device check."""
    from gdkvm_amd import build, ops
    build.build()
    f = ops.load().gdkvm_lv_biplane
    a = 4096                                                 # an address aligned for everything
    for C, T, D, P in ((5, 3, 0, 2), (5, 3, 65, 2), (5, 3, 20, -1), (-1, 3, 20, 2), (5, -3, 20, 2), (5, 1 << 16, 20, 1 << 15), (1 << 16, 1 << 15, 20, 2)):
        assert f(a, a, a, a, a, a, a, C, T, D, P, None) == -1, (C, T, D, P)
        assert b"lv_biplane" in ops.load().gdkvm_last_error()
    for C, T, P in ((5, 3, 0), (5, 0, 2), (0, 0, 0), (0, 3, 0)):
        assert f(None, None, None, None, None, None, None, C, T, 20, P, None) == 0, (C, T, P)
    for args in ((None, a, a, a, a, a, a), (a, None, a, a, a, a, a), (a, a, None, a, a, a, a), (a, a, a, None, a, a, a), (a, a, a, a, None, a, a),
                 (a, a, a, a, a, None, a), (a, a, a, a, a, a, None),
                 (a, a, a, a, a, a + 8, a), (a, a, a, a, a, a, a + 8), (a + 4, a, a, a, a, a, a), (a, a + 4, a, a, a, a, a), (a, a, a + 4, a, a, a, a),
                 (a, a, a, a + 2, a, a, a), (a, a, a, a, a + 2, a, a)):
        assert f(*args, 5, 3, 20, 2, None) == -6, args


def test_ops_lv_biplane_refusals_without_a_device():
    from gdkvm_amd import ops
    C, T, D = 3, 2, 20
    stats, disks, geom = torch.zeros(C, T, 12, dtype=torch.int64), torch.zeros(C, T, D, dtype=torch.int64), torch.zeros(C, T, 6, dtype=torch.float64)
    sp = torch.full((C, 1, 2), 300, dtype=torch.int32)
    good = torch.tensor([[0, 1], [2, 2]], dtype=torch.int32)
    for bad in (torch.tensor([[0, 3]], dtype=torch.int32), torch.tensor([[-1, 0]], dtype=torch.int32)):
        with pytest.raises(ops.GdkvmError, match="outside 0..2"):
            ops.lv_biplane(stats, disks, geom, sp, bad)
    with pytest.raises(ops.GdkvmError, match="host tensor"):
        ops.lv_biplane(stats, disks, geom, sp, torch.empty((2, 2), dtype=torch.int32, device="meta"))
    for bad in (good.long(), good.reshape(4), good.reshape(1, 4), [[0, 1]]):
        with pytest.raises(ops.GdkvmError, match="pairs must be an int32 tensor"):
            ops.lv_biplane(stats, disks, geom, sp, bad)
    for args, what in (((stats.int(), disks, geom), "stats"), ((stats, disks.double(), geom), "disks"), ((stats, disks, geom.float()), "geom"),
                       ((stats[..., :11], disks, geom), "stats"), ((stats, disks, geom[..., :4]), "geom"), ((stats[0], disks, geom), "stats")):
        with pytest.raises(ops.GdkvmError, match=f"lv_biplane: {what} must be"):
            ops.lv_biplane(*args, sp, good)
    with pytest.raises(ops.GdkvmError, match="same"):
        ops.lv_biplane(stats, disks[:2], geom, sp, good)
    with pytest.raises(ops.GdkvmError, match="outside 1..64"):
        ops.lv_biplane(stats, torch.zeros(C, T, 65, dtype=torch.int64), geom, sp, good)
    with pytest.raises(ops.GdkvmError, match="device"):       # everything in order, and no device: no CPU path
        ops.lv_biplane(stats, disks, geom, sp, good)
    assert "gdkvm_lv_biplane" in ops.SIGNATURES
