"""CPU checks of the temporal vote: the reference (tests/temporal_reference.py restates include/gdkvm.h) against scipy's median filter where the
two definitions coincide, against a plain per-pixel loop, and against known answers on hand-built label sequences; vote_summary against its
own definition; the configuration key; the refusals of the wrapper and of the C entry point."""
import os

import numpy as np
import pytest
import torch

from tests import temporal_reference as Tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pixel(labels, ncls, radius):
    """The reference's out of one pixel with these labels over the frames (a clip of 1 x 1 frames)."""
    m = np.asarray(labels, np.uint8).reshape(1, -1, 1, 1)
    out, info, _ = Tr.temporal_vote_ref(m, ncls, radius)
    assert [int(x) for x in info[0, :, 0]] == [int(a != b) for a, b in zip(out[0, :, 0, 0], labels)]
    return [int(x) for x in out[0, :, 0, 0]]


@pytest.mark.parametrize("shape,r", [((3, 5, 9, 7), 2), ((2, 9, 15, 13), 1), ((2, 8, 6, 5), 3)])
def test_interior_frames_of_binary_masks_are_the_temporal_median(shape, r):
    """On binary masks without 255 the majority of an odd window is its median: the frames r .. T-1-r, whose windows are not truncated, equal
    scipy.ndimage.median_filter along T."""
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(sum(shape) + r)
    m = (rng.random(shape) < 0.45).astype(np.uint8)
    out, info, counts = Tr.temporal_vote_ref(m, 2, r)
    T = shape[1]
    assert T > 2 * r and counts is None
    med = ndimage.median_filter(m, size=(1, 2 * r + 1, 1, 1))
    assert np.array_equal(out[:, r:T - r], med[:, r:T - r]) and (out != m).sum() > 0


@pytest.mark.parametrize("shape,ncls,r", [((2, 7, 5, 4), 4, 1), ((2, 6, 4, 5), 3, 2), ((3, 3, 3, 3), 3, 3), ((1, 1, 4, 4), 2, 1), ((2, 9, 3, 4), 8, 7),
                                          ((2, 5, 4, 4), 4, 0)])
def test_window_sums_agree_with_the_per_pixel_loop(shape, ncls, r):
    m = Tr.drifting_clips(*shape, ncls, seed=sum(shape))
    m[0, 0, 0, 0] = ncls                                               # the smallest byte that is no class
    tgt = np.roll(m, 1, 3)
    out, info, counts = Tr.temporal_vote_ref(m, ncls, r, tgt)
    B, T, H, W = shape
    for b in range(B):
        for y in range(H):
            for x in range(W):
                assert [Tr.vote_pixel(m[b, :, y, x], t, ncls, r) for t in range(T)] == out[b, :, y, x].tolist(), (b, y, x)
    assert info.dtype == np.int32 and counts.dtype == np.int32 and not info[..., 3].any() and not info[:, 0, 1:3].any()
    assert info[..., 0].sum() == (out != m).sum() and info[..., 1].sum() == (m[:, 1:] != m[:, :-1]).sum()
    assert info[..., 2].sum() == (out[:, 1:] != out[:, :-1]).sum()
    assert counts[..., 1].sum() == (out < ncls).sum() and counts[..., 2].sum() == (tgt < ncls).sum()
    assert counts[..., 0].sum() == ((out == tgt) & (out < ncls)).sum()
    if r == 0:
        assert np.array_equal(out, m)


def test_hand_built_pixels():
    # a tie the own label wins: the truncated windows of the first and last frame hold two frames that disagree
    assert _pixel([1, 0], 2, 1) == [1, 0]
    assert _pixel([2, 0, 0, 1], 3, 1) == [2, 0, 0, 1]                   # frame 0: {2, 0} stays 2; frame 3: {0, 1} stays 1
    assert _pixel([1, 0, 2], 3, 1)[1] == 0                              # a three-way tie of one vote each: the own label
    # a tie the own label is no part of: a a b b own with a < b gives a -- wherever own stands, and not b
    assert _pixel([1, 1, 3, 2, 2], 4, 2)[2] == 1
    assert _pixel([2, 2, 0, 1, 1], 4, 2)[2] == 1
    # T <= r: every window is the whole clip.  3 and 0 (3 and 2) tie two to two: own where own is one of them, else the smaller
    assert _pixel([3, 3, 0, 0, 1], 4, 4) == [3, 3, 0, 0, 0]
    assert _pixel([3, 3, 2, 2, 1], 4, 4) == [3, 3, 2, 2, 2]
    # a plain majority, and the flicker the filter exists for
    assert _pixel([1, 1, 0, 1, 1], 2, 1) == [1, 1, 1, 1, 1]
    assert _pixel([0, 0, 1, 1, 1, 0, 1], 2, 1) == [0, 0, 1, 1, 1, 1, 1]
    # a 255 in the window does not vote: {1, 255, 0} around frame 1 would otherwise be no tie of 1 and 0
    assert _pixel([1, 0, 255], 2, 1) == [1, 0, 255]                     # frame 1: 1 and 0 tie one to one, the own 0 stays
    assert _pixel([1, 255, 0, 0], 2, 1) == [1, 255, 0, 0]               # frame 0 keeps 1 on its own vote alone
    assert _pixel([1, 1, 255, 0, 0, 0, 255], 2, 2) == [1, 1, 255, 0, 0, 0, 255]
    assert _pixel([0, 255, 255, 1, 255], 2, 1) == [0, 255, 255, 1, 255]
    # a 255 at the centre passes through whatever its neighbours say; so does every byte >= ncls, which votes for nothing either
    assert _pixel([1, 255, 1], 2, 1) == [1, 255, 1]
    assert _pixel([1, 2, 1, 2, 2], 2, 1) == [1, 2, 1, 2, 2]
    assert _pixel([1, 2, 1, 2, 2], 3, 1) == [1, 1, 2, 2, 2]             # the same bytes with 2 a class
    # radius 0 and T = 1 change nothing
    assert _pixel([1, 0, 2, 255, 1], 3, 0) == [1, 0, 2, 255, 1] and _pixel([1], 2, 7) == [1]


def test_clips_do_not_influence_each_other():
    """Two clips whose border frames differ: the last frame of clip 0 and the first of clip 1 are neighbours in memory and no neighbours in
    time.  Voting them together equals voting each alone, and differs from voting the concatenation as one clip."""
    a = np.zeros((1, 4, 1, 2), np.uint8)
    b = np.ones((1, 4, 1, 2), np.uint8)
    a[0, 2] = 1                                                        # clip 0: 0 0 1 0 -- alone its last window {1, 0} is a tie the own 0 wins
    b[0, 1] = 0                                                        # clip 1: 1 0 1 1 -- alone its first window {1, 0} is a tie the own 1 wins
    both = np.concatenate([a, b])
    out = Tr.temporal_vote_ref(both, 2, 1)[0]
    assert (out[0] == 0).all() and (out[1] == 1).all()
    assert np.array_equal(out[:1], Tr.temporal_vote_ref(a, 2, 1)[0]) and np.array_equal(out[1:], Tr.temporal_vote_ref(b, 2, 1)[0])
    # as ONE clip of eight frames the two border frames would see each other: {1, 0, 1} -> 1 and {0, 1, 0} -> 0
    joined = Tr.temporal_vote_ref(both.reshape(1, 8, 1, 2), 2, 1)[0].reshape(2, 4, 1, 2)
    assert (joined[0, 3] == 1).all() and (joined[1, 0] == 0).all()


def test_the_planted_pixels_and_the_recipe_are_not_vacuous():
    for shape, ncls, r in (((3, 5, 15, 13), 4, 2), ((2, 6, 30, 58), 3, 2), ((1, 20, 12, 16), 8, 7), ((2, 8, 9, 9), 4, 1)):
        m = Tr.drifting_clips(*shape, ncls, seed=1)
        planted = Tr.plant_hand_pixels(m, ncls, r)
        assert list(planted) == ["own tie"] + ["other tie"] * (r >= 2) + ["255 in the window", "255 at the centre"]
        out = Tr.temporal_vote_ref(m, ncls, r)[0].reshape(shape[0], shape[1], -1)
        for name, (p, t, want) in planted.items():
            assert out[0, t, p] == want, (name, shape, r)
        assert m[0, 0, 0, 0] == 1                                      # the own label that won its tie
        if r >= 2:
            assert m[0, r, 0, 1] == 2                                  # 0 and 1 tied without the own label 2
        own, other, passed = Tr.tie_kinds(m, ncls, r)
        assert own > 0 and (other > 0 or r < 2) and passed > 0 and (out.reshape(shape) != m).sum() > 0
    m = Tr.drifting_clips(2, 1, 9, 7, 2, seed=2)
    assert Tr.plant_hand_pixels(m, 2, 1) == {} and Tr.tie_kinds(m, 2, 1)[:2] == (0, 0)       # T = 1: nothing to plant, nothing ties


def test_vote_summary_on_cpu_tensors():
    from gdkvm_amd import ops
    B, T, H, W, ncls, r = 3, 5, 9, 8, 4, 1
    m = Tr.drifting_clips(B, T, H, W, ncls, seed=7)
    tgt = np.roll(m, 1, 2)
    tgt[:, [0, 2, 4]] = 255                                            # two labelled frames per clip
    out, info, counts = Tr.temporal_vote_ref(m, ncls, r, tgt)
    labelled = torch.zeros(B, T, dtype=torch.bool)
    labelled[:, [1, 3]] = True
    got = ops.vote_summary(torch.from_numpy(info), torch.from_numpy(counts), labelled)
    o, g = torch.from_numpy(out)[:, [1, 3]], torch.from_numpy(tgt)[:, [1, 3]]
    want = [x for c in range(ncls) for x in (int(((o == c) & (g == c)).sum()), int((o == c).sum()), int((g == c).sum()))]
    want += [int((out != m).sum()), int((out != m).any((2, 3)).sum()), int((m[:, 1:] != m[:, :-1]).sum()), int((out[:, 1:] != out[:, :-1]).sum()), B * T]
    assert got.dtype == torch.int64 and got.tolist() == want and want[-5] > 0
    assert torch.equal(ops.vote_summary(torch.from_numpy(info), torch.from_numpy(counts), labelled.view(B, T)), got)
    assert ops.vote_summary(torch.from_numpy(info), None, labelled).tolist() == want[-5:]
    two = ops.vote_summary(torch.from_numpy(info[:2]), torch.from_numpy(counts[:2]), labelled[:2]) + \
        ops.vote_summary(torch.from_numpy(info[2:]), torch.from_numpy(counts[2:]), labelled[2:])
    assert torch.equal(two, got)                                       # sums of batches add
    with pytest.raises(ops.GdkvmError, match="info"):
        ops.vote_summary(torch.zeros(3, 5, 8, dtype=torch.int32), None, labelled)
    with pytest.raises(ops.GdkvmError, match="counts"):
        ops.vote_summary(torch.from_numpy(info), torch.from_numpy(counts[:2]), labelled)


def test_temporal_vote_config_key():
    from gdkvm_amd.config import load_config
    path = os.path.join(ROOT, "config", "config_gdkvm_01.yaml")
    for cfg in (load_config(path), load_config(None, [])):
        assert cfg.data.temporal_vote == 0
    assert load_config(path, ["data.temporal_vote=1"]).data.temporal_vote == 1
    assert load_config(path, ["data.temporal_vote=7", "data.lv_class=-1"]).data.temporal_vote == 7
    for bad in ("8", "true", "-1", "1.5", "one"):
        with pytest.raises(ValueError, match="temporal_vote"):
            load_config(path, [f"data.temporal_vote={bad}"])
    with pytest.raises(ValueError, match="temporal_vote"):
        load_config(path, ["data.temporal_vote=1", "data.num_classes=9"])


def test_no_cpu_fallback_and_wrapper_refusals():
    from gdkvm_amd import build, ops
    build.build()
    m = torch.zeros(2, 3, 8, 8, dtype=torch.uint8)
    with pytest.raises(ops.GdkvmError, match="device"):
        ops.temporal_vote(m, 4)
    with pytest.raises(ops.GdkvmError, match="device"):
        ops.temporal_vote(m[0], 2, radius=0, target=m[0])
    with pytest.raises(ops.GdkvmError, match="uint8"):
        ops.temporal_vote(m.float(), 4)
    with pytest.raises(ops.GdkvmError, match=r"T, H, W"):
        ops.temporal_vote(m[0, 0], 4)
    with pytest.raises(ops.GdkvmError, match="1..1024"):
        ops.temporal_vote(torch.zeros(1, 2, 2, 1025, dtype=torch.uint8), 4)
    for bad in (1, 9, True, 2.0):
        with pytest.raises(ops.GdkvmError, match="num_classes"):
            ops.temporal_vote(m, bad)
    for bad in (-1, 8, True, 1.0):
        with pytest.raises(ops.GdkvmError, match="radius"):
            ops.temporal_vote(m, 4, radius=bad)
    with pytest.raises(ops.GdkvmError, match="target must be"):
        ops.temporal_vote(m, 4, target=m[:1])
    with pytest.raises(ops.GdkvmError, match="out must be"):
        ops.temporal_vote(m, 4, out=m.int())


def test_c_entry_point_refuses_bad_arguments():
    """Every bad argument is GDKVM_ERR_SHAPE, in front of anything that needs a device; the workspace query is 0 for every shape."""
    import ctypes
    from gdkvm_amd import build, ops
    build.build()
    lib = ops.load()
    need = lib.gdkvm_temporal_vote_workspace_bytes
    assert need(16, 32, 112, 112, 4) == 0 and need(1, 20, 1024, 1024, 8) == 0 and need(0, 1, 8, 8, 2) == 0 and need(-1, 0, 0, 0, 0) == 0
    buf = (ctypes.c_uint8 * 8192)()
    p = (ctypes.addressof(buf) + 15) & ~15
    q = p + 4096                                                       # a second region: out never overlaps mask in the good call
    ok = lambda **kw: dict(dict(mask=p, target=None, out=q, info=p + 2048, counts=None, ws=None, wsb=0, clips=2, T=3, H=8, W=8, ncls=4, r=1), **kw)
    call = lambda a: lib.gdkvm_temporal_vote(a["mask"], a["target"], a["out"], a["info"], a["counts"], a["ws"], a["wsb"], a["clips"], a["T"],
                                             a["H"], a["W"], a["ncls"], a["r"], None)
    assert call(ok(clips=0)) == 0 and call(ok(clips=0, mask=None, out=None, info=None)) == 0
    total = 2 * 3 * 64
    bads = (dict(r=8), dict(r=-1), dict(ncls=1), dict(ncls=9), dict(ncls=0), dict(H=0), dict(W=0), dict(H=1025), dict(W=1025), dict(T=0),
            dict(T=-1), dict(clips=-1), dict(mask=None), dict(out=None), dict(info=None), dict(info=p + 2048 + 8),
            dict(target=p + 1024), dict(target=p + 1024, counts=p + 3072 + 4),                    # a target without counts; misaligned counts
            dict(out=p), dict(out=p + 1), dict(out=p + total - 1), dict(mask=q + total - 1))      # out == mask and partial overlaps
    for bad in bads:
        assert call(ok(**bad)) == -1, bad
        assert lib.gdkvm_last_error().startswith(b"temporal_vote:"), bad
    assert call(ok(clips=0, r=8)) == -1 and call(ok(clips=0, ncls=1)) == -1 and call(ok(clips=0, H=0)) == -1     # checks precede the shortcut
    # what remains of a good call is the device: without a gfx950 it is refused there, not before (GDKVM_ERR_ARCH or _LAUNCH), with one it runs
    if not torch.cuda.is_available():
        for good in (ok(), ok(out=p + total), ok(mask=q + total), ok(r=0, ncls=2), ok(r=7, ncls=8)):
            assert call(good) not in (0, -1), good
