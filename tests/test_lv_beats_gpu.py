"""gdkvm_lv_beats on the device against tests/beats_reference.py: every integer output with ==, every fp64 output to rtol = 1e-15 (the bound
tests/test_lv_measure_gpu.py uses for lv_ef: the EF is two correctly rounded operations on the same operands, the mean a sum in the same
order).  Shapes are the smallest that reach each path of the kernel: clips below, at and above one wave, beyond one pass of the 256 lanes,
both forms of the end-diastole search (a wave per beat up to 32 end-systoles, a lane per beat beyond), the LDS limit T = 4096."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import beats_reference as R
from tests.test_lv_beats_cpu import HAND_CASES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(ops, area, vol, length=None, max_beats=16, distance=20, permille=500, min_pixels=1):
    """Runs the kernel and the reference on area, vol [B][T] (and length [B]) and compares all four outputs; returns the reference's."""
    a = torch.tensor(np.asarray(area), dtype=torch.int64).cuda()
    v = torch.tensor(np.asarray(vol), dtype=torch.float64).cuda()
    ln = None if length is None else torch.tensor(length, dtype=torch.int32).cuda()
    beats, val, info, summ = ops.lv_beats(a, v, ln, max_beats=max_beats, distance=distance, prominence_permille=permille, min_pixels=min_pixels)
    B = len(area)
    assert beats.dtype == torch.int32 and beats.shape == (B, max_beats, 2) and val.dtype == torch.float64 and val.shape == (B, max_beats, 3)
    assert info.dtype == torch.int32 and info.shape == (B, 4) and summ.dtype == torch.float64 and summ.shape == (B, 4)
    want = R.lv_beats_ref(area, vol, length, max_beats=max_beats, distance=distance, permille=permille, min_pixels=min_pixels)
    what = (len(area[0]), max_beats, distance, permille)
    got_info, got_beats = info.cpu().tolist(), beats.cpu().tolist()
    assert got_info == want[2], (what, [(b, got_info[b], want[2][b]) for b in range(B) if got_info[b] != want[2][b]][:4])
    assert got_beats == want[0], (what, [(b, got_beats[b], want[0][b]) for b in range(B) if got_beats[b] != want[0][b]][:2])
    assert np.allclose(val.cpu().numpy(), np.asarray(want[1]), rtol=1e-15, atol=0.0), what
    assert np.allclose(summ.cpu().numpy(), np.asarray(want[3]), rtol=1e-15, atol=0.0), (what, summ.cpu().tolist(), want[3])
    return want


def _tied_curves(B, T, seed):
    """The curves scipy cannot judge: integer noise of range 0..5 (ties and plateaus everywhere) and a coarse sine (every extremum a plateau,
    equal minima beat after beat), alternating; volumes with a few zeros."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    area = np.empty((B, T), np.int64)
    for b in range(B):
        if b % 2 == 0:
            area[b] = rng.integers(0, 6, T)
        else:
            area[b] = np.round(3.0 * np.sin(2 * np.pi * t / rng.uniform(5, 40) + rng.uniform(0, 6.3))).astype(np.int64) + 3 + (rng.random(T) < 0.05)
    vol = rng.uniform(10.0, 900.0, (B, T))
    vol[rng.random((B, T)) < 0.03] = 0.0
    return area.tolist(), vol.tolist()


@pytest.mark.parametrize("T", [1, 2, 3, 63, 64, 65, 257, 700])
def test_lv_beats_matches_the_reference_on_ties_and_plateaus(hip, T):
    B = 12
    area, vol = _tied_curves(B, T, seed=T)
    rng = np.random.default_rng(1000 + T)
    length = [0, 1, T] + [int(x) for x in rng.integers(0, T + 1, B - 5)] + [T + 5, -2]       # (clamped to 0 .. T)
    many = 0
    for distance in (1, 7, 64):
        for pm in (0, 500, 1000):
            for mb in (1, 16, 64):
                for ln in (None, length):
                    want = _check(hip, area, vol, ln, max_beats=mb, distance=distance, permille=pm, min_pixels=2)
                    many += sum(1 for i in want[2] if i[1] > 32)
    if T == 700:
        assert many > 0                                          # more than 32 end-systoles: a lane per beat searched the end-diastoles


def test_lv_beats_hand_cases(hip):
    for name, area, kw, es, beats in HAND_CASES:
        vol = [float(3 * v + 1) for v in area]
        want = _check(hip, [area], [vol], max_beats=4, **kw)
        assert want[2][0][:2] == [len(beats), len(es)] and [tuple(b) for b in want[0][0] if b[0] >= 0] == beats, name
    # padding with a deep minimum, short clips, EDV == 0, n_below, more beats than max_beats: one batch, a clip each
    area = [[5, 9, 4, 8, 6, 9, 0, 9, 9, 9, 9, 9, 9]] * 5 + [[9, 1] * 6 + [9]]
    vol = [[float(10 + t) for t in range(13)]] * 6
    vol[1] = [0.0] * 13
    for mp in (1, 6):
        want = _check(hip, area, vol, [6, 13, 0, 1, 2, 13], max_beats=2, distance=1, permille=0, min_pixels=mp)
        assert want[2][0][:2] == [2, 2] and want[2][1][1] == 3 and want[1][1][0] == [0.0, 0.0, 0.0]
        assert [i[:2] for i in want[2][2:5]] == [[0, 0]] * 3 and want[2][5][:2] == [5, 6] and want[0][5] == [[2, 3], [4, 5]]
        assert [i[2] for i in want[2]] == ([0, 1, 0, 0, 0, 0] if mp == 1 else [2, 3, 0, 1, 1, 6])


def test_lv_beats_at_the_lds_limit(hip):
    """T = 4096: a systole every 9 frames (455 end-systoles at distance 1, far more beats than max_beats) and one long staircase whose
    minima are all the global minimum, so every prominence walk runs to both borders; then the largest distance."""
    T = 4096
    rng = np.random.default_rng(4096)
    saw = [[50, 40, 30, 20, 10, 20, 30, 40, 50][t % 9] for t in range(T)]
    stairs = [[3, 3, 2, 2, 1, 1, 0, 0, 0, 1, 1, 2, 2][t % 13] for t in range(T)]
    vol = rng.uniform(10.0, 900.0, (2, T)).tolist()
    want = _check(hip, [saw, stairs], vol, max_beats=64, distance=1, permille=500)
    assert want[2][0] == [454, 455, 0, 9 * 454] and want[2][1][:2] == [314, 315] and want[3][0][3] == 9.0 and want[3][1][3] == 13.0
    _check(hip, [saw, stairs], vol, [4095, 2049], max_beats=16, distance=9, permille=1000)
    want = _check(hip, [saw, stairs], vol, max_beats=1, distance=4096, permille=0)
    assert [i[1] for i in want[2]] == [1, 1]


def test_lv_beats_refuses_bad_arguments(hip):
    a, v = torch.zeros(2, 8, dtype=torch.int64).cuda(), torch.zeros(2, 8, dtype=torch.float64).cuda()
    with pytest.raises(hip.GdkvmError, match="T in 1..4096"):
        hip.lv_beats(torch.zeros(1, 4097, dtype=torch.int64).cuda(), torch.zeros(1, 4097, dtype=torch.float64).cuda())
    with pytest.raises(hip.GdkvmError, match="max_beats"):
        hip.lv_beats(a, v, max_beats=65)
    with pytest.raises(hip.GdkvmError, match="distance"):
        hip.lv_beats(a, v, distance=0)
    with pytest.raises(hip.GdkvmError, match="prominence_permille"):
        hip.lv_beats(a, v, prominence_permille=1001)
    with pytest.raises(hip.GdkvmError, match="length must be"):
        hip.lv_beats(a, v, torch.zeros(2, dtype=torch.int64).cuda())
    with pytest.raises(hip.GdkvmError, match="length must be"):
        hip.lv_beats(a, v, torch.zeros(3, dtype=torch.int32).cuda())
    with pytest.raises(hip.GdkvmError, match="vol must be"):
        hip.lv_beats(a, v.float())
    with pytest.raises(hip.GdkvmError, match="area must be"):
        hip.lv_beats(a.int(), v)
    with pytest.raises(hip.GdkvmError):                            # the library's own check, behind the wrapper's
        hip._call("gdkvm_lv_beats", a.device, a, v, None, a, v, a, v, 2, 8, 65, 20, 500, 1)
    out = hip.lv_beats(a[:0], v[:0])                              # no clip: no launch
    assert out[0].shape == (0, 16, 2) and out[3].shape == (0, 4)
    # non-contiguous views are copied
    wide_a, wide_v = torch.arange(32, dtype=torch.int64).view(2, 16).cuda() % 5, torch.rand(2, 16, dtype=torch.float64).cuda()
    got = hip.lv_beats(wide_a[:, ::2], wide_v[:, ::2], distance=1, prominence_permille=0)
    want = hip.lv_beats(wide_a[:, ::2].contiguous(), wide_v[:, ::2].contiguous(), distance=1, prominence_permille=0)
    assert all(torch.equal(x, y) for x, y in zip(got, want))


def test_lv_beats_is_reproducible_and_capturable(hip):
    from gdkvm_amd.data import SyntheticEchoClips
    da, db = (torch.stack([SyntheticEchoClips(2, 48, 48, num_classes=2, seed=s, beats=3.0, as_uint8=True)[i][1] for i in range(2)]).cuda() for s in (3, 4))

    def chain(mask):
        stats, _, geom = hip.lv_measure(mask, cls=1, disks=20)
        return hip.lv_beats(stats[..., 0], geom[..., 1], distance=5)

    first, second = chain(da), chain(da)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    static = da.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = chain(static)
    static.copy_(db)
    g.replay()
    torch.cuda.synchronize()
    want = chain(db)
    assert all(torch.equal(x, y) for x, y in zip(out, want))
    assert not all(torch.equal(x, y) for x, y in zip(first, want)) and int(want[2][:, 1].min()) >= 2


def _synthetic_beats(hip):
    from gdkvm_amd.data import SyntheticEchoClips
    ds = SyntheticEchoClips(8, 96, 64, num_classes=2, beats=3.0, as_uint8=True)
    target = torch.stack([ds[i][1] for i in range(8)]).cuda()
    stats, _, geom = hip.lv_measure(target)
    area, vol = stats[..., 0].contiguous(), geom[..., 1].contiguous()
    return area, vol, hip.lv_beats(area, vol, distance=10)


def test_beats_of_synthetic_labels(hip):
    """Clips of three periods of 32 frames, measured and read beat by beat: 2 or 3 counted beats, a mean cycle of 32 frames, no beat's EF above
    the clip's lv_ef EF (whose ED and ES are the global extremes), and a comparison of the result with itself without error."""
    area, vol, (beats, val, info, summ) = _synthetic_beats(hip)
    _check(hip, area.cpu().tolist(), vol.cpu().tolist(), distance=10)
    assert ((info[:, 0] == 2) | (info[:, 0] == 3)).all() and (info[:, 2] == 0).all()
    assert ((summ[:, 3] - 32.0).abs() <= 1.0).all()
    _, ef = hip.lv_ef(vol, area)
    counted = beats[..., 0] >= 0
    assert (val[..., 2][counted] > 0.2).all() and (val[..., 2] <= ef[:, 2:3]).all() and (summ[:, 2] <= ef[:, 2]).all()
    st = hip.beats_stats(hip.beats_summary(summ, info, summ, info).cpu())
    assert st["clips"] == 8 and st["clips_with_ef"] == 8 and st["ef_mae"] == 0.0 and st["ef_bias"] == 0.0
    assert st["systole_count_agreement"] == 1.0 and st["systole_count_mae"] == 0.0


def test_beats_of_synthetic_labels_three_systoles_each(hip):
    """Three end-systoles in every one of the eight clips: with a whole number of beats the generator keeps every period's minimum 0.3
    periods from the clip's ends, where it has the prominence (a minimum nearer than a quarter period to an end would have none, for the
    kernel as for scipy)."""
    _, _, (_, _, info, _) = _synthetic_beats(hip)
    assert info[:, 1].tolist() == [3] * 8


def test_eval_reports_the_beats_block_and_changes_nothing_else(hip, tmp_path):
    """eval.py's loop over 4 synthetic clips of 96 frames of 64 x 64 holding three beats each (the split's size is no configuration key: the
    driver below hands eval.py a 4-clip dataset), seeded random weights, with data.lv_beats on and off: the block is there with its keys
    in order, and every other key is unchanged."""
    driver = ("import sys; sys.path.insert(0, sys.argv[1]); import gdkvm_amd.data as D\n"
              "def four(cfg, split='train', n_synthetic=256, as_uint8=False):\n"
              "    d = cfg.data\n"
              "    return D.SyntheticEchoClips(4, d.frames, d.size, d.num_classes, seed=cfg.seed + 7919, as_uint8=as_uint8, beats=d.synthetic_beats)\n"
              "D.build_dataset = four\n"
              "import eval as E; E.main(sys.argv[2:])\n")
    common = ["data.size=64", "data.frames=96", "batch_size=4", "model.value_dim=64", "data.num_classes=2", "data.synthetic_beats=3",
              "data.beat_distance=10", f"run_dir={tmp_path}"]

    def run(extra):
        ev = subprocess.run([sys.executable, "-c", driver, ROOT] + common + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert ev.returncode == 0, ev.stderr[-2000:]
        return json.loads(ev.stdout.strip().splitlines()[-1])

    on, off = run(["data.lv_beats=true"]), run([])
    assert "beats" not in off and on["clips"] == 4
    bt = on["beats"]
    assert list(bt) == ["clips", "beats_per_clip", "mean_cycle_frames", "clips_dropped_below_min", "clips_with_target", "ef_mae", "ef_bias",
                        "ef_pearson_r", "systole_count_agreement"]
    assert bt["clips"] == 4 and bt["clips_with_target"] == 4 and 0 <= bt["clips_dropped_below_min"] <= 4
    assert bt["beats_per_clip"] >= 0 and bt["mean_cycle_frames"] >= 0 and 0 <= bt["systole_count_agreement"] <= 1 and bt["ef_mae"] >= abs(bt["ef_bias"])
    assert {k: v for k, v in on.items() if k != "beats"} == off


def test_eval_reads_whole_echonet_videos_beat_by_beat(hip, tmp_path):
    """eval.py on two converted EchoNet videos read from their first frame (data.whole_video): one of 40 frames with an EF in its file, one
    of 20 (shorter than the clip: 12 padding frames, which lv_beats must not read) without.  The target labels two frames at most, so no
    clip is compared with it, and the file's EF is the reference of the one clip that has one."""
    rng = np.random.default_rng(2)
    (tmp_path / "data" / "val").mkdir(parents=True)
    masks = np.zeros((2, 64, 64), np.uint8)
    masks[0, 12:52, 20:44], masks[1, 18:46, 24:40] = 1, 1
    video = rng.integers(0, 255, (40, 64, 64), dtype=np.uint8)
    np.savez_compressed(tmp_path / "data" / "val" / "a.npz", video=video, traced=np.asarray([5, 20]), masks=masks, ef=np.float64(58.0), fps=np.float64(50.0))
    np.savez_compressed(tmp_path / "data" / "val" / "b.npz", video=video[:20], traced=np.asarray([3, 12]), masks=masks)
    common = [f"data_path={tmp_path / 'data'}", "data.kind=echonet_npz", "data.size=64", "data.frames=32", "data.num_classes=2", "batch_size=2",
              "model.value_dim=64", "data.whole_video=true", "data.beat_distance=4", f"run_dir={tmp_path}"]

    def run(extra):
        ev = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py")] + common + extra, capture_output=True, text=True, timeout=600)
        assert ev.returncode == 0, ev.stderr[-2000:]
        return json.loads(ev.stdout.strip().splitlines()[-1])

    on, off = run(["data.lv_beats=true"]), run([])
    assert {k: v for k, v in on.items() if k != "beats"} == off and on["clips"] == 2
    bt = on["beats"]
    assert bt["clips"] == 2 and bt["clips_with_target"] == 0 and bt["ef_mae"] == 0.0 and bt["systole_count_agreement"] == 0.0
    assert list(bt["vs_file_ef"]) == ["clips_with_ef", "ef_mae", "ef_bias", "ef_pearson_r"] and bt["vs_file_ef"]["clips_with_ef"] in (0, 1)
    assert bt["vs_file_ef"]["ef_mae"] >= abs(bt["vs_file_ef"]["ef_bias"])
