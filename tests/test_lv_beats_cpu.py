"""The beat detection's definition on the CPU (tests/beats_reference.py restates include/gdkvm.h, gdkvm_lv_beats): against
scipy.signal.find_peaks where scipy is a definition (curves of pairwise distinct samples), by hand where it is not (plateaus, ties, borders,
padding, the beats' own rules), a closed form, and the data / configuration pieces around it: the new keys, the synthetic clips' beats, the
whole-video clips of EchoNetNpz."""
import math

import numpy as np
import pytest
import torch

from tests import beats_reference as R

PMS = (0, 100, 250, 500, 900, 1000)


def _distinct_curve(rng, n):
    """A sine plus noise, times 256, plus a distinct low byte: no two samples are equal (n <= 256)."""
    t = np.arange(n)
    wave = 400.0 + 300.0 * np.sin(2 * np.pi * t / rng.uniform(6, 60) + rng.uniform(0, 6.3)) + rng.normal(0, rng.uniform(0, 80), n)
    return (np.round(wave).astype(np.int64) * 256 + rng.permutation(256)[:n]).tolist()


def test_reference_end_systoles_are_scipys_on_distinct_curves():
    from scipy.signal import find_peaks
    rng = np.random.default_rng(0)
    for k in range(400):
        n = int(rng.integers(1, 201))
        a = _distinct_curve(rng, n)
        d, pm = int(rng.integers(1, 30)), PMS[k % len(PMS)]
        span = max(a) - min(a)
        want, _ = find_peaks(-np.asarray(a, np.float64), distance=d, prominence=None if pm == 0 else pm * span / 1000)
        assert R.end_systoles(a, d, pm) == want.tolist(), (k, n, d, pm)


def _one(area, vol=None, length=None, **kw):
    vol = [float(v) for v in area] if vol is None else vol
    beats, val, info, summ = R.lv_beats_ref([area], [vol], None if length is None else [length], **kw)
    return beats[0], val[0], info[0], summ[0]


# (name, area, keyword arguments, end-systoles, counted beats (ed, es)): the cases scipy leaves open or decides differently; the GPU file
# runs them through the kernel
HAND_CASES = [
    ("plateau minimum", [9, 5, 3, 3, 3, 3, 7, 9, 4, 8], dict(distance=1, permille=0), [3, 8], [(7, 8)]),
    ("even plateau", [9, 3, 3, 7], dict(distance=1, permille=0), [1], []),
    ("equal minima closer than distance", [9, 2, 8, 2, 9, 9], dict(distance=3, permille=0), [1], []),
    ("equal minima at the distance", [9, 2, 8, 2, 9, 9], dict(distance=2, permille=0), [1, 3], [(2, 3)]),
    ("borders are no systoles", [1, 5, 9, 5, 1], dict(distance=1, permille=0), [], []),
    ("plateau to the border", [9, 4, 4, 4], dict(distance=1, permille=0), [], []),
    ("beat 0 kept", [5, 9, 2, 8, 3, 9], dict(distance=1, permille=0), [2, 4], [(1, 2), (3, 4)]),
    ("beat 0 dropped", [9, 5, 2, 8, 3, 9], dict(distance=1, permille=0), [2, 4], [(3, 4)]),
    ("tie of the end-diastole", [1, 7, 7, 2, 9], dict(distance=1, permille=0), [3], [(1, 3)]),
    ("prominence drops the shallow one", [0, 100, 10, 100, 95, 100, 0], dict(distance=1, permille=500), [2], [(1, 2)]),
    ("prominence at the bound", [0, 100, 50, 100, 0], dict(distance=1, permille=500), [2], [(1, 2)]),
    ("prominence walk over equal minima", [0, 9, 4, 9, 4, 6, 0], dict(distance=1, permille=500), [2], [(1, 2)]),
]


@pytest.mark.parametrize("name,area,kw,es,beats", HAND_CASES, ids=[c[0] for c in HAND_CASES])
def test_reference_hand_cases(name, area, kw, es, beats):
    assert R.end_systoles(area, kw["distance"], kw["permille"]) == es
    bt, val, info, summ = _one(area, max_beats=4, **kw)
    assert [tuple(b) for b in bt if b[0] >= 0] == beats and info[:2] == [len(beats), len(es)]
    assert info[3] == (es[-1] - es[0] if es else 0)
    for (ed, e), v in zip(beats, val):
        assert v == [float(area[ed]), float(area[e]), (area[ed] - area[e]) / area[ed]]


def test_reference_padding_short_clips_and_limits():
    # a deep minimum in the padding is ignored, and so is everything else behind len
    area = [5, 9, 4, 8, 6, 9, 0, 9]
    assert R.end_systoles(area[:6], 1, 0) == [2, 4] and R.end_systoles(area, 1, 0) == [2, 4, 6]
    bt, val, info, summ = _one(area, length=6, max_beats=4, distance=1, permille=0)
    assert [b for b in bt if b[0] >= 0] == [[1, 2], [3, 4]] and info == [2, 2, 0, 2] and summ[3] == 2.0
    assert _one(area, length=6, max_beats=4, distance=1, permille=500)[2][:2] == [1, 1]     # the range is that of the valid frames: 5, not 9
    assert _one(area, length=99, max_beats=4, distance=1, permille=0)[2][1] == 3           # clamped to T
    for n in (0, 1, 2, -3):
        bt, val, info, summ = _one(area, length=n, max_beats=3, distance=1, permille=0, min_pixels=6)
        assert bt == [[-1, -1]] * 3 and val == [[0.0] * 3] * 3 and summ == [0.0] * 4
        assert info == [0, 0, sum(1 for v in area[:max(n, 0)] if v < 6), 0]
    # more beats than max_beats: all are counted and averaged, the first max_beats are listed
    saw = [9, 1] * 6 + [9]
    vol = [float(10 + t) for t in range(len(saw))]
    bt, val, info, summ = _one(saw, vol=vol, max_beats=2, distance=1, permille=0)
    assert bt == [[2, 3], [4, 5]] and info == [5, 6, 0, 10] and summ[3] == 2.0             # beat 0's ED is frame 0: not counted
    efs = [(vol[e - 1] - vol[e]) / vol[e - 1] for e in (3, 5, 7, 9, 11)]
    s = 0.0
    for e in efs:
        s = s + e
    assert summ[:3] == [s / 5.0, min(efs), max(efs)] and val[1] == [vol[4], vol[5], efs[1]]
    # EDV == 0: EF is 0
    bt, val, info, summ = _one([5, 9, 2, 8], vol=[1.0, 0.0, 3.0, 1.0], max_beats=1, distance=1, permille=0)
    assert bt == [[1, 2]] and val == [[0.0, 3.0, 0.0]] and summ[:3] == [0.0, 0.0, 0.0]
    # n_below is counted and changes nothing else
    base = _one([5, 9, 2, 8, 3, 9], max_beats=4, distance=1, permille=0, min_pixels=1)
    high = _one([5, 9, 2, 8, 3, 9], max_beats=4, distance=1, permille=0, min_pixels=4)
    assert base[2][2] == 0 and high[2][2] == 2 and base[:2] == high[:2] and base[3] == high[3] and base[2][:2] == high[2][:2]


def test_reference_closed_form_cosine():
    P, T = 25, 128
    area = [int(round(1000 + 300 * math.cos(2 * math.pi * t / P))) for t in range(T)]
    vol = [(v / 10.0) ** 1.5 for v in area]
    es = R.end_systoles(area, 10, 500)
    want = [k * P + P // 2 for k in range(5)]                    # the frames nearest P / 2 + k P: 12 and 13 tie in area, the plateau's middle is 12
    assert es == want
    bt, val, info, summ = _one(area, vol=vol, max_beats=8, distance=10, permille=500)
    assert info == [4, 5, 0, 4 * P] and summ[3] == float(P)      # the clip starts on a maximum: beat 0's ED is frame 0 and it does not count
    assert bt[:4] == [[k * P, k * P + P // 2] for k in range(1, 5)] and bt[4:] == [[-1, -1]] * 4
    efs = []
    for (ed, e), v in zip(bt[:4], val):
        assert v[2] == (vol[ed] - vol[e]) / vol[ed] and v[:2] == [vol[ed], vol[e]]
        efs.append(v[2])
    assert summ[1] == min(efs) and summ[2] == max(efs) and abs(summ[0] - sum(efs) / 4) < 1e-15


def test_config_keys_and_synthetic_beats():
    from gdkvm_amd.config import beat_prominence_permille, load_config
    from gdkvm_amd.data import SyntheticEchoClips, build_dataset, clip_length_table
    cfg = load_config(None, [])
    d = cfg.data
    assert (d.lv_beats, d.beat_distance, d.beat_prominence, d.synthetic_beats, d.whole_video) == (False, 20, 0.5, 1.0, False)
    assert beat_prominence_permille(cfg) == 500
    assert beat_prominence_permille(load_config(None, ["data.beat_prominence=0.0625"])) == 62       # round, half to even
    assert beat_prominence_permille(load_config(None, ["data.beat_prominence=1"])) == 1000
    for bad in ("data.beat_distance=0", "data.beat_distance=4097", "data.beat_distance=2.5", "data.beat_distance=true",
                "data.beat_prominence=-0.1", "data.beat_prominence=1.5", "data.beat_prominence=half", "data.synthetic_beats=0",
                "data.synthetic_beats=-1", "data.synthetic_beats=.inf", "data.lv_beats=1", "data.whole_video=2", "data.whole_video=true"):
        with pytest.raises(ValueError):
            load_config(None, [bad])
    assert load_config(None, ["data.whole_video=true", "data.kind=echonet_npz"]).data.whole_video is True
    with pytest.raises(ValueError):
        SyntheticEchoClips(2, 8, 16, beats=0.0)

    default, one = SyntheticEchoClips(4, 12, 32, num_classes=3, seed=5), SyntheticEchoClips(4, 12, 32, num_classes=3, seed=5, beats=1.0)
    for i in range(3):                                           # beats = 1.0: the clips of before, byte for byte
        (x0, y0), (x1, y1) = default[i], one[i]
        assert x0.numpy().tobytes() == x1.numpy().tobytes() and y0.numpy().tobytes() == y1.numpy().tobytes()
    ds = build_dataset(load_config(None, ["data.synthetic_beats=3", "data.frames=96", "data.size=64", "data.num_classes=2"]), "val", as_uint8=True)
    assert ds.beats == 3.0 and clip_length_table(ds).tolist() == [96] * len(ds) and clip_length_table(ds).dtype == torch.int32
    # A whole number of beats >= 2: every period's minimum keeps 0.3 periods from the clip's ends (SyntheticEchoClips), so all three of the
    # minima at t0, t0 + 32, t0 + 64, t0 = 9.6 + 11.8 u with u the generator's fifth draw, have the prominence: three end-systoles
    for i in range(3):
        rng = np.random.default_rng(ds.seed * 1_000_003 + i)
        rng.random(4)
        t0 = 0.3 * 32 + rng.random() * (0.4 * 32 - 1.0)
        area = (ds[i][1] == 1).sum((1, 2)).tolist()
        es = R.end_systoles(area, 10, 500)
        assert len(es) == 3 and all(abs(e - (t0 + 32 * k)) <= 2 for k, e in enumerate(es)), (i, t0, es)
    # any other value keeps the free phase: the generator's draws and every other parameter are those of beats = 1.0
    # (frame 0 depends on the phase alone, not on the rate)
    free, whole = (SyntheticEchoClips(4, 12, 32, num_classes=3, seed=5, beats=b)[0][1] for b in (2.5, 3.0))
    assert torch.equal(free[0], default[0][1][0]) and not torch.equal(whole[0], default[0][1][0])


def test_echonet_whole_video(tmp_path):
    from gdkvm_amd.data import IGNORE_LABEL, EchoNetNpz, clip_length_table
    rng = np.random.default_rng(1)
    (tmp_path / "val").mkdir()
    video = rng.integers(0, 255, (40, 24, 24), dtype=np.uint8)
    masks = np.zeros((2, 24, 24), np.uint8)
    masks[0, 4:20, 6:18], masks[1, 6:18, 8:16] = 1, 1
    np.savez_compressed(tmp_path / "val" / "a_long.npz", video=video, traced=np.asarray([5, 36]), masks=masks, ef=np.float64(61.5), fps=np.float64(50.0))
    np.savez_compressed(tmp_path / "val" / "b_short.npz", video=video[:20], traced=np.asarray([5, 12]), masks=masks)      # an old file: no ef
    ds = EchoNetNpz(str(tmp_path), "val", 32, as_uint8=True, whole=True)
    assert [ds.length(i) for i in range(2)] == [32, 20] and clip_length_table(ds).tolist() == [32, 20]
    assert ds.file_ef(0) == 61.5 and ds.file_fps(0) == 50.0 and ds.file_ef(1) is None and ds.file_fps(1) is None
    x, y = ds[0]
    assert x.shape == (32, 3, 24, 24) and np.array_equal(x[:, 0].numpy(), video[:32])
    labelled = [t for t in range(32) if (y[t] != IGNORE_LABEL).any()]
    assert labelled == [5] and np.array_equal(y[5].numpy(), masks[0])          # the frame traced at 36 lies behind the cut
    x, y = ds[1]
    assert np.array_equal(x[:20, 0].numpy(), video[:20]) and all(np.array_equal(x[t, 0].numpy(), video[19]) for t in range(20, 32))
    assert [t for t in range(32) if (y[t] != IGNORE_LABEL).any()] == [5, 12] and np.array_equal(y[12].numpy(), masks[1])
    window = EchoNetNpz(str(tmp_path), "val", 32, as_uint8=True)              # the window around the tracings is what it was
    assert window.length(0) == 32 and sum(bool((window[0][1][t] != IGNORE_LABEL).any()) for t in range(32)) == 2
    assert window.file_ef(0) == 61.5


def test_fixed_point_form_of_the_distance_rule_is_the_greedy_one():
    """What the kernel iterates -- a candidate keeps itself once every rival in range is dropped or of lower priority and drops itself once one
    rival in range is kept -- ends in the greedy result, ties and plateaus included (distance rule alone: permille = 0)."""
    rng = np.random.default_rng(7)
    for k in range(300):
        n = int(rng.integers(3, 120))
        a = rng.integers(0, int(rng.integers(2, 12)), n).tolist()
        d = int(rng.integers(1, 20))
        cand = R.end_systoles(a, 1, 0)                          # distance 1 and no prominence: every candidate
        state = {c: "open" for c in cand}
        for _ in range(len(cand) + 1):
            nxt = dict(state)
            for c in cand:
                if state[c] != "open":
                    continue
                rivals = [q for q in cand if q != c and abs(q - c) < d]
                if any(state[q] == "kept" for q in rivals):
                    nxt[c] = "dropped"
                elif all(state[q] == "dropped" or (a[q], q) > (a[c], c) for q in rivals):
                    nxt[c] = "kept"
            state = nxt
        assert "open" not in state.values()
        assert sorted(c for c in cand if state[c] == "kept") == R.end_systoles(a, d, 0), (k, a, d)


def test_lv_beats_has_no_cpu_path_and_refuses_bad_arguments():
    import ctypes
    from gdkvm_amd import build, ops
    build.build()
    a, v = torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, 8, dtype=torch.float64)
    with pytest.raises(ops.GdkvmError, match="device"):
        ops.lv_beats(a, v)
    for kw, what in ((dict(max_beats=0), "max_beats"), (dict(max_beats=65), "max_beats"), (dict(distance=0), "distance"),
                     (dict(distance=4097), "distance"), (dict(prominence_permille=-1), "permille"), (dict(prominence_permille=1001), "permille"),
                     (dict(length=torch.zeros(2, dtype=torch.int64)), "length must be"), (dict(length=torch.zeros(3, dtype=torch.int32)), "length must be")):
        with pytest.raises(ops.GdkvmError, match=what):
            ops.lv_beats(a, v, **kw)
    with pytest.raises(ops.GdkvmError, match="T in 1..4096"):
        ops.lv_beats(torch.zeros(1, 4097, dtype=torch.int64), torch.zeros(1, 4097, dtype=torch.float64))
    with pytest.raises(ops.GdkvmError, match="vol must be"):
        ops.lv_beats(a, v[:, :7])
    # the C entry's own checks sit in front of anything that needs a device
    lib = ops.load()
    buf = (ctypes.c_uint8 * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(area=p, vol=p, length=None, beats=p, val=p, info=p, summ=p, B=1, T=8, mb=16, d=20, pm=500)

    def call(**kw):
        k = dict(ok, **kw)
        return lib.gdkvm_lv_beats(k["area"], k["vol"], k["length"], k["beats"], k["val"], k["info"], k["summ"], k["B"], k["T"], k["mb"], k["d"],
                                  k["pm"], 1, None)

    assert call(B=0) == 0 and call(B=0, area=None) == 0
    for bad in (dict(T=0), dict(T=4097), dict(B=-1), dict(mb=0), dict(mb=65), dict(d=0), dict(d=4097), dict(pm=-1), dict(pm=1001)):
        assert call(**bad) == -1, bad
    for bad in (dict(area=None), dict(vol=None), dict(beats=None), dict(val=None), dict(info=None), dict(summ=None), dict(beats=p + 8),
                dict(info=p + 4), dict(summ=p + 8), dict(area=p + 4), dict(vol=p + 4), dict(length=p + 2)):
        assert call(**bad) == -6, bad


def test_beats_summary_adds_over_batches():
    from gdkvm_amd import ops
    summ = torch.tensor([[0.5, 0.4, 0.6, 30.0], [0.4, 0.4, 0.4, 0.0], [0.0, 0.0, 0.0, 0.0], [0.6, 0.5, 0.7, 28.0]], dtype=torch.float64)
    info = torch.tensor([[2, 3, 0, 60], [1, 1, 0, 0], [0, 0, 0, 0], [3, 3, 2, 56]], dtype=torch.int32)
    ref_summ = summ + torch.tensor([0.1, 0, 0, 0], dtype=torch.float64)
    ref_info = info.clone()
    ref_info[1, 1], ref_info[3, 2] = 3, 0
    s = ops.beats_summary(summ, info, ref_summ, ref_info)
    assert s.dtype == torch.float64 and s.shape == (11,)
    assert torch.equal(s, ops.beats_summary(summ[:2], info[:2], ref_summ[:2], ref_info[:2]) + ops.beats_summary(summ[2:], info[2:], ref_summ[2:], ref_info[2:]))
    st = ops.beats_stats(s)
    assert st["clips"] == 4 and st["clips_with_ef"] == 2                   # clip 2 has no beat, clip 3 a frame below min_pixels
    assert abs(st["ef_bias"] + 0.1) < 1e-12 and abs(st["ef_mae"] - 0.1) < 1e-12
    assert st["systole_count_agreement"] == 0.75 and st["systole_count_mae"] == 0.5
    st = ops.beats_stats(ops.beats_summary(summ, info, ref_summ, ref_info, ok=torch.tensor([True, False, True, True])))
    assert st["clips"] == 3 and st["clips_with_ef"] == 1 and st["systole_count_agreement"] == 1.0
    assert ops.beats_stats(torch.zeros(11))["clips"] == 0 and ops.beats_stats(torch.zeros(11))["systole_count_agreement"] == 0.0
