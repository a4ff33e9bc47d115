"""gdkvm_temporal_vote on the device against tests/temporal_reference.py, bit for bit: out, info and counts.  The shapes sit where the kernel
can go wrong rather than at the workload's size: windows truncated at both ends, clips shorter than the radius, frames whose H*W is no
multiple of 16 (every frame then starts at another alignment), fewer than 16 pixels, both sides of a workgroup's run of pixel positions, of
the launch's workgroup cap and of the vector / byte split, and every class count the launcher has a kernel for."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lv_reference as R
from tests import temporal_reference as Tr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "include", "gdkvm.h")).read()
_define = lambda name: int(re.search(r"#define GDKVM_TEMPORAL_VOTE_" + name + r" (\d+)", _HDR).group(1))
RUN, NARROW_RUN = _define("RUN"), _define("NARROW_RUN")           # pixel positions per workgroup with 16 and with 4 per lane
NARROW_BELOW = _define("NARROW_BELOW")                            # 4 per lane while 16 per lane give fewer (clip, run) pairs than this
MAX_WG = _define("MAX_WG")                                        # workgroups per launch

# (clips, T, H, W, ncls, r).  The issue's list ...
SHAPES = [(2, 8, 112, 112, 4, 1),      # the aligned vector path (the cfg2 mask)
          (3, 5, 15, 13, 4, 2),        # T = 2r + 1, H*W = 195: every frame unaligned
          (2, 6, 30, 58, 3, 2),        # T = 2r + 2
          (2, 3, 5, 3, 3, 3),          # T <= r: every window is the whole clip; fewer than 16 pixels
          (2, 1, 9, 7, 2, 1),          # T = 1: out = mask
          (1, 2, 1, 1, 2, 1),          # a single pixel
          (2, 4, 8, 1024, 2, 1),       # long rows
          (1, 20, 144, 160, 8, 7),     # largest ncls and radius, more pixels than one workgroup's run
          (40, 3, 16, 16, 4, 1)]       # many clips
# ... and one shape on each side of every split of the launcher
# 4 pixels per lane: 256 (one run), 272 (two, words) and 257 (two, bytes) pixels; more (clip, run) pairs than a launch has workgroups
N_ONE_RUN, N_TWO_RUNS, N_TWO_RUNS_BYTES, N_PAST_CAP = (2, 4, 16, 16, 4, 1), (2, 3, 17, 16, 4, 1), (2, 3, 257, 1, 4, 1), (1100, 3, 32, 32, 2, 1)
# the last shape with 4 per lane and the first with 16, in bytes (15 pixels) and in words / vectors (16 pixels)
LAST_NARROW, FIRST_WIDE, LAST_NARROW_VEC, FIRST_WIDE_VEC = (3071, 3, 5, 3, 3, 1), (3072, 3, 5, 3, 3, 1), (3071, 3, 4, 4, 3, 1), (3072, 3, 4, 4, 3, 1)
# 16 pixels per lane: 1024 (one run), 1040 (two, vectors) and 1025 (two, bytes) pixels
ONE_RUN, TWO_RUNS, TWO_RUNS_BYTES = (3072, 3, 32, 32, 2, 1), (1536, 3, 26, 40, 2, 1), (1536, 3, 25, 41, 2, 1)
AT_CAP, PAST_CAP, PAST_CAP_RUNS = (4096, 3, 4, 4, 2, 1), (4100, 3, 4, 4, 2, 1), (2100, 3, 33, 32, 2, 1)   # 4096, 4100 and 4200 work items
SHAPES += [N_ONE_RUN, N_TWO_RUNS, N_TWO_RUNS_BYTES, N_PAST_CAP, LAST_NARROW, FIRST_WIDE, LAST_NARROW_VEC, FIRST_WIDE_VEC, ONE_RUN, TWO_RUNS,
           TWO_RUNS_BYTES, AT_CAP, PAST_CAP, PAST_CAP_RUNS,
           (2, 4, 9, 7, 5, 1), (2, 5, 9, 7, 6, 2), (2, 5, 8, 8, 7, 2),                                   # the kernels for 5, 6 and 7 classes ...
           (3080, 3, 2, 2, 5, 1), (3080, 3, 2, 2, 6, 1), (3080, 3, 2, 2, 7, 1), (3080, 5, 2, 2, 8, 2),   # ... with 16 pixels per lane
           (3080, 5, 2, 2, 4, 2)]


def _wide(shape):
    return shape[0] * -(-shape[2] * shape[3] // RUN) >= NARROW_BELOW


def _items(shape):
    return shape[0] * -(-shape[2] * shape[3] // (RUN if _wide(shape) else NARROW_RUN))


def test_the_shapes_lie_on_both_sides_of_every_split(hip):
    need = hip.load().gdkvm_temporal_vote_workspace_bytes
    assert all(need(*s[:5]) == 0 for s in SHAPES)                  # no workspace form to cover
    px = lambda s: s[2] * s[3]
    assert (RUN, NARROW_RUN, NARROW_BELOW, MAX_WG) == (1024, 256, 3072, 4096)
    assert not any(map(_wide, (N_ONE_RUN, N_TWO_RUNS, N_TWO_RUNS_BYTES))) and (px(N_ONE_RUN), px(N_TWO_RUNS), px(N_TWO_RUNS_BYTES)) == (256, 272, 257)
    assert all(map(_wide, (ONE_RUN, TWO_RUNS, TWO_RUNS_BYTES))) and (px(ONE_RUN), px(TWO_RUNS), px(TWO_RUNS_BYTES)) == (1024, 1040, 1025)
    assert not _wide(LAST_NARROW) and _wide(FIRST_WIDE) and not _wide(LAST_NARROW_VEC) and _wide(FIRST_WIDE_VEC)
    assert _items(AT_CAP) == MAX_WG and _items(PAST_CAP) == MAX_WG + 4 and _items(PAST_CAP_RUNS) == 4200 > MAX_WG
    assert not _wide(N_PAST_CAP) and _items(N_PAST_CAP) == 4400 > MAX_WG and max(_items(s) for s in SHAPES[:9]) <= MAX_WG
    for wide in (False, True):                                     # one kernel per class count, lane width and access width
        assert {s[4] for s in SHAPES if _wide(s) == wide} == set(range(2, 9))
        assert any(px(s) % 16 == 0 for s in SHAPES if _wide(s) == wide) and any(px(s) % 16 for s in SHAPES if _wide(s) == wide)


_CACHE = {}


def _case(shape):
    """(mask, target, reference out, info, counts, planted) -- computed once per shape and shared, never modified."""
    if shape not in _CACHE:
        B, T, H, W, ncls, r = shape
        mask = Tr.drifting_clips(B, T, H, W, ncls, seed=sum(shape))
        planted = Tr.plant_hand_pixels(mask, ncls, r)
        tr = np.random.default_rng(H * 7 + W)
        target = np.roll(mask, 1, 3)                               # overlaps the mask in most pixels, 255s included
        target[tr.random(target.shape) < 0.2] = ncls - 1
        target[:, (T + 1) // 2:] = 255                             # unlabelled frames
        _CACHE[shape] = (mask, target) + Tr.temporal_vote_ref(mask, ncls, r, target) + (planted,)
    return _CACHE[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_temporal_vote_matches_the_reference(hip, shape):
    B, T, H, W, ncls, r = shape
    mask, target, want_out, want_info, want_counts, planted = _case(shape)
    # no case is vacuous where the shape allows otherwise
    own_ties, other_ties, passed = Tr.tie_kinds(mask, ncls, r)
    flat_want = want_out.reshape(B, T, -1)
    for name, (p, t, lab) in planted.items():
        assert flat_want[0, t, p] == lab, name
    if T > 1:
        assert "own tie" in planted and own_ties > 0
        assert want_info[..., 0].sum() > 0 or H * W == 1            # (two frames of one pixel that disagree: both keep their own label)
    if T >= 2 * r + 1 and r >= 2 and ncls >= 3 and H * W >= 2:
        assert other_ties > 0 and "other tie" in planted
    if B * T * H * W >= 1000:
        assert passed > 0 and (want_out[mask >= ncls] == mask[mask >= ncls]).all()
    dm, dt = torch.from_numpy(mask).cuda(), torch.from_numpy(target).cuda()
    out, info, counts = hip.temporal_vote(dm, ncls, r, target=dt)
    assert out.shape == dm.shape and out.dtype == torch.uint8 and info.shape == (B, T, 4) and info.dtype == torch.int32
    assert counts.shape == (B, T, ncls, 3) and counts.dtype == torch.int32
    got_out, got_info, got_counts = out.cpu().numpy(), info.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(got_out, want_out), np.argwhere(got_out != want_out)[:5]
    assert np.array_equal(got_info, want_info), np.argwhere(got_info != want_info)[:5]
    assert np.array_equal(got_counts, want_counts), np.argwhere(got_counts != want_counts)[:5]
    assert torch.equal(dm.cpu(), torch.from_numpy(mask))           # the input is left alone
    # info and counts are those of out itself, recomputed in torch
    lo = out.long()
    assert torch.equal(info[..., 0].long(), (out != dm).sum((2, 3))) and not info[..., 3].any() and not info[:, 0, 1:3].any()
    assert torch.equal(info[:, 1:, 1].long(), (dm[:, 1:] != dm[:, :-1]).sum((2, 3))) and torch.equal(info[:, 1:, 2].long(), (lo[:, 1:] != lo[:, :-1]).sum((2, 3)))
    for c in range(ncls):
        o, g = out == c, dt == c
        assert torch.equal(counts[:, :, c].long(), torch.stack([(o & g).sum((2, 3)), o.sum((2, 3)), g.sum((2, 3))], -1))
    # without a target: the same mask and info, no counts
    out2, info2, none = hip.temporal_vote(dm, ncls, r)
    assert none is None and torch.equal(out2, out) and torch.equal(info2, info)
    # into a given tensor
    given = torch.full_like(dm, 0xEE)
    out3, info3, counts3 = hip.temporal_vote(dm, ncls, r, target=dt, out=given)
    assert out3 is given and torch.equal(given, out) and torch.equal(info3, info) and torch.equal(counts3, counts)


@pytest.mark.parametrize("shape", [(3, 5, 15, 13, 4, 2), (2, 8, 112, 112, 4, 1), (40, 3, 16, 16, 4, 1)], ids=lambda s: "x".join(map(str, s)))
def test_clips_are_voted_independently(hip, shape):
    """vote(cat(a, b)) == cat(vote(a), vote(b)) over the clip axis."""
    B, T, H, W, ncls, r = shape
    mask, target, want_out, want_info, want_counts, _ = _case(shape)
    k = max(1, B // 2)
    parts = [hip.temporal_vote(torch.from_numpy(mask[s]).cuda(), ncls, r, target=torch.from_numpy(target[s]).cuda()) for s in (slice(0, k), slice(k, B))]
    for i, want in enumerate((want_out, want_info, want_counts)):
        assert np.array_equal(torch.cat([p[i] for p in parts]).cpu().numpy(), want)
    # no clip at all: nothing is launched, empty results
    none = hip.temporal_vote(torch.empty((0, T, H, W), dtype=torch.uint8, device="cuda"), ncls, r)
    assert none[0].shape == (0, T, H, W) and none[1].shape == (0, T, 4) and none[2] is None


@pytest.mark.parametrize("shape,offs", [((3, 5, 15, 13, 4, 2), ((1, 15, 1), (7, 9, 12), (15, 1, 4), (1, 15, 6))),
                                        ((2, 4, 16, 16, 4, 1), ((0, 0, 0), (0, 3, 0), (0, 0, 5), (7, 9, 7), (15, 0, 0))),
                                        ((2, 3, 26, 40, 4, 1), ((0, 0, 0), (1, 1, 1))),
                                        (FIRST_WIDE_VEC, ((0, 0, 0), (3, 0, 0), (0, 0, 9)))], ids=("195px", "256px", "1040px", "16-per-lane"))
def test_temporal_vote_at_any_byte_address(hip, shape, offs):
    """mask, target and out as views at byte offsets into sentinel buffers (mask, target, out): the bytes around the mask are class 1 and may
    not vote, the bytes around out keep their sentinel.  out is tried at the mask's alignment (16-byte stores when everything is aligned)
    and at another."""
    B, T, H, W, ncls, r = shape
    mask, target, want_out, want_info, want_counts, _ = _case(shape)
    n = mask.size
    for off, t_off, o_off in offs:
        buf = torch.full((n + 48,), 1, dtype=torch.uint8, device="cuda")
        tbuf = torch.full((n + 48,), 1, dtype=torch.uint8, device="cuda")
        obuf = torch.full((n + 48,), 0xEE, dtype=torch.uint8, device="cuda")
        view, tview, oview = buf[off:off + n].view(mask.shape), tbuf[t_off:t_off + n].view(mask.shape), obuf[o_off:o_off + n].view(mask.shape)
        view.copy_(torch.from_numpy(mask)); tview.copy_(torch.from_numpy(target))
        assert view.data_ptr() % 16 == off and tview.data_ptr() % 16 == t_off and oview.data_ptr() % 16 == o_off
        out, info, counts = hip.temporal_vote(view, ncls, r, target=tview, out=oview)
        assert out is oview
        assert np.array_equal(oview.cpu().numpy(), want_out), (off, t_off, o_off)
        assert np.array_equal(info.cpu().numpy(), want_info) and np.array_equal(counts.cpu().numpy(), want_counts), (off, t_off, o_off)
        assert (obuf[:o_off] == 0xEE).all() and (obuf[o_off + n:] == 0xEE).all()
        assert (buf[:off] == 1).all() and (buf[off + n:] == 1).all() and torch.equal(view.cpu(), torch.from_numpy(mask))
    with pytest.raises(hip.GdkvmError, match="overlap"):
        hip.temporal_vote(view, ncls, r, out=view)
    with pytest.raises(hip.GdkvmError, match="overlap"):
        hip.temporal_vote(buf[:n].view(mask.shape), ncls, r, out=buf[16:16 + n].view(mask.shape))


@pytest.mark.parametrize("shape", [(2, 6, 30, 58, 3), (2, 4, 16, 16, 8), (2, 5, 112, 112, 4)], ids=lambda s: "x".join(map(str, s)))
def test_radius_zero_is_the_identity_with_argmax_dice_counts(hip, shape):
    B, T, H, W, ncls = shape
    rng = np.random.default_rng(B + T + H)
    mask = rng.integers(0, ncls, (B, T, H, W), dtype=np.uint8)        # no byte is >= ncls here
    target = rng.integers(0, ncls, (B, T, H, W), dtype=np.uint8)
    target[:, 1] = 255
    dm, dt = torch.from_numpy(mask).cuda(), torch.from_numpy(target).cuda()
    out, info, counts = hip.temporal_vote(dm, ncls, 0, target=dt)
    assert torch.equal(out, dm) and not info[..., 0].any() and torch.equal(info[..., 1], info[..., 2]) and info[:, 1:, 1].all()
    logits = torch.nn.functional.one_hot(dm.long().view(B * T, H, W), ncls).permute(0, 3, 1, 2).float().contiguous()
    mask2, counts2 = hip.argmax_dice(logits, dt.view(B * T, H, W))
    assert torch.equal(mask2.view(B, T, H, W), dm) and torch.equal(counts2.view(B, T, ncls, 3), counts)


@pytest.mark.parametrize("shape", [(2, 8, 112, 112, 4, 1), (3, 5, 15, 13, 4, 2), FIRST_WIDE_VEC], ids=lambda s: "x".join(map(str, s)))
def test_temporal_vote_is_reproducible_and_capturable(hip, shape):
    """Vector form and byte form: two calls agree; a captured call replays on new input (info and counts are zeroed inside the graph)."""
    B, T, H, W, ncls, r = shape
    mask, target, want_out, want_info, want_counts, _ = _case(shape)
    da, dt = torch.from_numpy(mask).cuda(), torch.from_numpy(target).cuda()
    db, du = da.flip(1).contiguous(), dt.flip(0, 1).contiguous()                   # other input: the clips played backwards
    first, second = hip.temporal_vote(db, ncls, r, target=du), hip.temporal_vote(db, ncls, r, target=du)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    static, static_t = db.clone(), du.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hip.temporal_vote(static, ncls, r, target=static_t)
    static.copy_(da); static_t.copy_(dt)
    g.replay()
    g.replay()                                                     # a second replay starts from zeroed sums again
    torch.cuda.synchronize()
    for got, want in zip(out, (want_out, want_info, want_counts)):
        assert np.array_equal(got.cpu().numpy(), want)


def test_leading_dimensions_are_kept(hip):
    shape = (6, 5, 15, 13, 4, 2)
    B, T, H, W, ncls, r = shape
    mask, target = _case(shape)[:2]
    dm, dt = torch.from_numpy(mask).cuda(), torch.from_numpy(target).cuda()
    flat = hip.temporal_vote(dm, ncls, r, target=dt)
    out, info, counts = hip.temporal_vote(dm.view(2, 3, T, H, W), ncls, r, target=dt.view(2, 3, T, H, W))
    assert out.shape == (2, 3, T, H, W) and info.shape == (2, 3, T, 4) and counts.shape == (2, 3, T, ncls, 3)
    assert torch.equal(out.view(B, T, H, W), flat[0]) and torch.equal(info.view(B, T, 4), flat[1]) and torch.equal(counts.view(B, T, ncls, 3), flat[2])
    one = hip.temporal_vote(dm[1], ncls, r, target=dt[1])          # a 3-D mask is one clip
    assert one[0].shape == (T, H, W) and one[1].shape == (T, 4) and one[2].shape == (T, ncls, 3)
    assert all(torch.equal(x, y[1]) for x, y in zip(one, flat))
    labelled = torch.zeros(2, 3, T, dtype=torch.bool, device="cuda")
    labelled[..., :T // 2] = True
    s = hip.vote_summary(info, counts, labelled)
    assert s.shape == (ncls * 3 + 5,) and int(s[-1]) == B * T and int(s[-5]) == int(flat[1][..., 0].sum())
    assert torch.equal(s[:ncls * 3].view(ncls, 3), flat[2][:, :T // 2].long().sum((0, 1)))


def flicker_clips(seed=3):
    """(clean, flickered) [2, 9, 112, 112]: per clip the ellipse A for three frames, the smaller B for three, A again (ED - ES - ED), and in
    the flickered copy one frame in three -- 1, 4 and 7, each between two clean frames that equal it -- re-drawn at random inside the ring of
    +-3 pixels around its border."""
    rng = np.random.default_rng(seed)
    clean = np.zeros((2, 9, 112, 112), np.uint8)
    flick = None
    for b, (deg, cx) in enumerate(((20, 56), (150, 60))):
        big, small = R.ellipse_mask(112, 112, 56, cx, 40, 18, deg), R.ellipse_mask(112, 112, 56, cx, 32, 13, deg)
        for t in range(9):
            clean[b, t] = small if 3 <= t < 6 else big
    flick = clean.copy()
    for b, (deg, cx) in enumerate(((20, 56), (150, 60))):
        for t in (1, 4, 7):
            la, sa = (32, 13) if t == 4 else (40, 18)
            ring = (R.ellipse_mask(112, 112, 56, cx, la + 3, sa + 3, deg) == 1) & (R.ellipse_mask(112, 112, 56, cx, la - 3, sa - 3, deg) == 0)
            flick[b, t][ring] = rng.integers(0, 2, int(ring.sum()), dtype=np.uint8)
    return clean, flick


def test_the_vote_removes_border_flicker_and_restores_the_ejection_fraction(hip):
    """The feature's purpose, on the device: frames whose border ring was drawn wrong come back wherever their two neighbours agree, the clip
    flips less from frame to frame, and lv_ef of the voted clip is that of the clean clip (the flickered clip's is not)."""
    clean, flick = flicker_clips()
    assert 200 < (clean != flick).sum((2, 3))[:, [1, 4, 7]].min() and not (clean != flick)[:, [0, 2, 3, 5, 6, 8]].any()
    dc, df = torch.from_numpy(clean).cuda(), torch.from_numpy(flick).cuda()
    out, info, counts = hip.temporal_vote(df, 2, 1, target=dc)
    for t in (1, 4, 7):
        agree = dc[:, t - 1] == dc[:, t + 1]
        assert agree.all()                                         # here: everywhere
        assert torch.equal(out[:, t][agree], dc[:, t][agree])
    assert torch.equal(out[:, [0, 1, 4, 7, 8]], dc[:, [0, 1, 4, 7, 8]])
    assert int(info[..., 2].sum()) < int(info[..., 1].sum()) and int(info[..., 0].sum()) > 0
    left = out != dc
    assert 0 < int(left.sum()) < int((df != dc).sum()) and not left[:, [0, 1, 4, 7, 8]].any()     # what is left sits in the frames where A meets B
    # Dice against the clean clip went up, from the counts alone
    before = hip.temporal_vote(df, 2, 0, target=dc)[2]
    assert float(hip.dice_from_counts(counts.sum((0, 1)))[1]) > float(hip.dice_from_counts(before.sum((0, 1)))[1])

    def ef(m):
        stats, _, geom = hip.lv_measure(m)
        return hip.lv_ef(geom[..., 1].contiguous(), stats[..., 0].contiguous())[1]

    want, dirty, got = ef(dc), ef(df), ef(out)
    assert torch.equal(got, want) and not torch.equal(dirty[:, 2], want[:, 2])
    assert (want[:, 2] > 0.3).all()


def test_eval_reports_the_temporal_vote_block_and_changes_nothing_else(hip, tmp_path):
    """eval.py on the tiny synthetic split (clips of 4 frames, seeded random weights) with the key on and with it off: the block is there with
    its keys in order, and every key other than `temporal_vote` and `lv` is unchanged."""
    common = ["data.size=64", "data.frames=4", "batch_size=4", f"run_dir={tmp_path}"]

    def run(extra):
        ev = subprocess.run([sys.executable, os.path.join(ROOT, "eval.py")] + common + extra, capture_output=True, text=True, timeout=600)
        assert ev.returncode == 0, ev.stderr[-2000:]
        return json.loads(ev.stdout.strip().splitlines()[-1])

    on, off = run(["data.temporal_vote=1"]), run([])
    assert "temporal_vote" not in off
    tv = on["temporal_vote"]
    assert list(tv) == ["radius", "frames_changed", "pixels_changed", "flips_per_frame_before", "flips_per_frame_after", "dice_per_class",
                        "mean_foreground_dice"]
    assert tv["radius"] == 1 and 0 <= tv["frames_changed"] <= min(tv["pixels_changed"], on["clips"] * 4)
    assert 0 <= tv["flips_per_frame_after"] <= tv["flips_per_frame_before"] <= 64 * 64
    assert len(tv["dice_per_class"]) == len(on["dice_per_class"]) and all(0 <= d <= 1 for d in tv["dice_per_class"])
    if tv["pixels_changed"] == 0:
        assert tv["dice_per_class"] == on["dice_per_class"] and tv["mean_foreground_dice"] == on["mean_foreground_dice"] and on["lv"] == off["lv"]
    assert {k: v for k, v in on.items() if k not in ("temporal_vote", "lv")} == {k: v for k, v in off.items() if k != "lv"}
