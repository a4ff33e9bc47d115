"""What tests/test_scan_backward_forms_gpu.py rests on, proved without a GPU: the constants of tests/scan_bwd_forms.py equal the .hip
source; every clip length and every large shape crosses or avoids what it claims; the frame-by-frame and the chained fp64 references
are the one-call reference (so what the GPU tests assert bit for bit across calls is a property of the function); and every fp64-checked
case can see the slips of scan_bwd_forms.SLIPS through its own bound."""
import os

import numpy as np
import pytest
import torch

from oracle import torch_ref as TR
from tests import grid_caps as gc
from tests import scan_bwd_forms as F


@pytest.mark.parametrize("name", sorted(F.CONSTANTS))
def test_constants_equal_the_source(name):
    assert F.source_constant(name) == F.CONSTANTS[name][0] == getattr(F, name)


def test_restated_expressions_are_the_source_text():
    texts = {}
    for fname, line in F.SOURCE_LINES:
        if fname not in texts:
            with open(os.path.join(gc.CSRC, fname)) as f:
                texts[fname] = f.read()
        assert line in texts[fname], (fname, line)
    assert F.ufd() == 6 and F.pseudo_frames(64) == 1 and F.pseudo_frames(65) == 2 and F.pseudo_frames(130) == 3 and F.pseudo_frames(256) == 4


def test_clip_lengths_take_every_tail_behind_zero_to_three_bodies():
    """Group 2: T = 1..14, 18, 19 at N = 5 and Tc = 2T, T = 1..7, at N = 65."""
    plans = {T: F.clip_plan(T, 5) for T in F.CLIP_LENGTHS}
    assert all(p.steps == T for T, p in plans.items())
    seen = {(p.bodies, p.tail) for p in plans.values()}
    assert {(0, t) for t in range(1, 6)} <= seen                            # the peeled tail alone
    assert {(1, t) for t in range(6)} <= seen                               # one body, every tail
    assert {(2, 0), (2, 1), (2, 2), (3, 0), (3, 1)} <= seen                 # the body run twice and three times, with and without a tail
    assert max(T for T in F.CLIP_LENGTHS if T <= 9) == 9 and all(F.clip_plan(T).bodies <= 1 for T in range(1, 10))   # (T <= 9: what the suite had)
    pseudo = {T: F.clip_plan(T, 65) for T in F.PSEUDO_CLIP_LENGTHS}
    assert [p.steps for p in pseudo.values()] == [2 * T for T in F.PSEUDO_CLIP_LENGTHS]
    assert {(p.bodies, p.tail) for p in pseudo.values()} == {(0, 2), (0, 4), (1, 0), (1, 2), (1, 4), (2, 0), (2, 2)}
    for case in F.GROUP2:
        assert F.rows_to_img(*case[:5]) is None or not F.rows_to_img(*case[:5]).capped


def test_group1_shapes_cover_what_they_name():
    assert {(c[5], c[6]) for c in F.GRID_CASES} == {(r, f) for r in (0, 1, 2) for f in (0, 3)}
    assert all(c[7] == "bf16" for c in F.GRID_CASES + F.SHAPE_CASES + F.TOKEN_CASES)
    assert any(c[3] == 2 for c in F.SHAPE_CASES) and any(c[2] % 16 for c in F.SHAPE_CASES)          # two heads; a ragged N
    lasts = {F.value_chunks(c[4]).last for c in F.GROUP1}
    assert {16, 32, 48, 64} <= lasts                                                                 # every width of the last value chunk
    assert all(F.value_chunks(c[4]).chunks > 4 for c in F.WIDE_CASES)                                # beyond Dv = 256
    assert all(F.pseudo_frames(c[2]) > 1 for c in F.TOKEN_CASES) and {F.pseudo_frames(c[2]) for c in F.TOKEN_CASES} == {2, 3, 4}
    assert any(c[2] % 64 == 0 for c in F.TOKEN_CASES) and any(c[2] % 64 == 1 for c in F.TOKEN_CASES)
    assert all(c[8] == 32 for c in F.NARROW_CASES)


def test_large_shapes_cross_exactly_the_cap_they_claim():
    """Group 6: the two-clip call is past the cap, each clip alone is under it."""
    B, T, N, Hh, Dv = F.ROWS_TO_IMG_SHAPE
    both, one = F.rows_to_img(B, T, N, Hh, Dv), F.rows_to_img(1, T, N, Hh, Dv)
    assert both.capped and both.blocks == F.ROWS_TO_IMG_CAP and both.trips == 2 and not one.capped and one.blocks == 4160
    assert -(-both.total // 256) == 8320
    assert not any(g.capped for g in F.train_copies(B, T, N, Hh, Dv, 2).values())
    B, T, N, Hh, Dv = F.COPY_GRID_SHAPE
    both, one = F.train_copies(B, T, N, Hh, Dv, 2), F.train_copies(1, T, N, Hh, Dv, 2)
    assert both["pad_v"].capped and both["pad_v"].total == 1100 * 4096 > F.COPY_GRID_CAP * 256 and both["pad_v"].trips == 2
    assert [k for k, g in both.items() if g.capped] == ["pad_v"] and not any(g.capped for g in one.values())
    assert F.rows_to_img(B, T, N, Hh, Dv).capped                            # (and gdr_rows_to_img_kernel strides further here: 5 trips)
    # the pad-gates launch has B T C 65 Hh items: its cap needs B T C Hh > 64527 frame-heads, which no clip reaches
    assert F.COPY_GRID_CAP * 256 // 65 == 64527
    B, T, N, Hh, Dv = F.REAL_SHAPE
    assert F.pseudo_frames(N) == 1 and F.clip_plan(T, N).bodies == 5 and F.clip_plan(T, N).tail == 2 and F.value_chunks(Dv).chunks == 4


def test_chain_pieces():
    shape, cuts, _, _ = F.LONG_CHAIN
    ps = F.pieces(shape[1], cuts)
    assert ps[0][0] == 0 and ps[-1][1] == shape[1] == 300 and all(a[1] == b[0] for a, b in zip(ps, ps[1:]))
    assert max(hi - lo for lo, hi in ps) == F.LONG_CHAIN_MAX_PIECE and len({(hi - lo) % F.ufd() for lo, hi in ps}) == 6   # every tail
    assert F.pieces(12, (1, 5)) == [(0, 1), (1, 5), (5, 12)] and F.pieces(6, (2, 3)) == [(0, 2), (2, 3), (3, 6)]


@pytest.mark.parametrize("shape", F.STATE_BWD_SHAPES)
def test_frame_by_frame_reference_is_the_scan(shape):
    """Group 4's reference: TR.scan one frame at a time with the state carried reproduces TR.scan's R and S_T, and its history starts
    at s0."""
    inp = F.make_inputs(F._c(shape, dtype="fp32"))
    ts = [torch.from_numpy(getattr(inp, n)).double() for n in F.NAMES]
    hist, R, S = F.ref_history(ts, 2, 3)
    R1, S1 = TR.scan(*ts, 2, 3)
    assert (R - R1).abs().max() <= 1e-12 and (S - S1).abs().max() <= 1e-12
    assert torch.equal(hist[:, 0], ts[5]) and hist.shape == (shape[0], shape[1], shape[3], 64, shape[4])
    _, _, S2 = F.ref_history([t[:, :3] for t in ts[:5]] + [ts[5]], 2, 3)
    assert (hist[:, 3] - S2).abs().max() <= 1e-12                           # entry t is the state after t frames


@pytest.mark.parametrize("case", F.CHAIN_CASES + [F.LONG_CHAIN], ids=str)
def test_chained_reference_is_the_one_call_reference(case):
    """Group 5's property: a clip cut into calls with the state handed on as a tensor has the values and gradients of one call."""
    shape, cuts, rule, flags = case
    inp = F.make_inputs(F._c(shape, rule, flags, "fp32"))
    R, S, g = F.ref_chain(inp, cuts)
    R1, S1, g1 = F.ref_one_call(inp)
    assert np.abs(R - R1).max() <= 1e-12 and np.abs(S - S1).max() <= 1e-12
    for n in F.NAMES:
        assert np.abs(g[n] - g1[n]).max() <= 1e-12 * max(1.0, np.abs(g1[n]).max()), n


@pytest.mark.parametrize("case", F.GROUP1 + F.GROUP2, ids=str)
def test_every_fp64_checked_case_sees_every_slip(case):
    inp = F.make_inputs(case)
    ref = F.ref_grads(inp)
    assert all(v == 0.0 for v in F.worst(ref, ref, inp.bf16).values())
    for slip in F.SLIPS:
        slipped = slip(inp, ref)
        if slipped is None:
            assert slip is F.slip_value_columns and case[4] <= F.FRAME_CHUNK
            continue
        assert F.sees(inp, ref, slipped), (slip.__name__, F.worst(slipped, ref, inp.bf16))


def test_bound_is_the_one_of_the_existing_backward_tests():
    r = np.array([[-300.0, 2.0], [0.5, 0.0]])
    assert F.allowed("alpha", r, False) == F.allowed("q", r, False) == F.allowed("s0", r, True) == pytest.approx(3e-2)
    assert np.allclose(F.allowed("k", r, True), 3e-2 + np.abs(r) / 128)
    assert F.allowed("v", np.array([0.1]), False) == pytest.approx(1e-4)
