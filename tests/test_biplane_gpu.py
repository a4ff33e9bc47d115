"""gdkvm_lv_biplane on the device against tests/biplane_reference.py evaluated on the device's OWN records (ops.lv_measure_mm's, read back):
the fp64 outputs to 1e-12 relative -- the definition fixes every operation, the allowance is the project's for fp64 outputs, as in
test_spacing_gpu.py -- and npix exactly; the identities (a view paired with itself, the views swapped), empty frames and -1 records, the edge
sizes D = 1 and 64, T = 1, P = 0, more pairs than one workgroup's four waves serve many times over, and two calls bit for bit."""
import numpy as np
import pytest
import torch

from tests import biplane_reference as R

pytestmark = pytest.mark.gpu

C, T, H, W = 5, 3, 64, 48
SPACINGS = [(330, 470), (410, 290), (365, 365), (297, 512), (455, 318)]        # (row_um, col_um) per clip
PAIRS = [[0, 1], [3, 2], [4, 4]]
RTOL = 1e-12

_CACHE = {}


def clips():
    """uint8 [C, T, H, W]: per clip an ellipse of its own size, tilt and place, shrinking over the frames -- built once, never modified."""
    if "clips" not in _CACHE:
        m = np.zeros((C, T, H, W), np.uint8)
        for c in range(C):
            for t in range(T):
                k = 1.0 - 0.12 * t
                m[c, t] = R.ellipse_view(H, W, *SPACINGS[c], (7.0 + 0.4 * c) * k, (3.0 + 0.5 * ((c * 2) % 3)) * k, 0.15 - 0.07 * c,
                                         cy_mm=0.3 * c - 0.5, cx_mm=0.4 - 0.2 * c)
        m.setflags(write=False)
        _CACHE["clips"] = m
    return _CACHE["clips"]


def records(hip, D, masks=None, spacing=None):
    """ops.lv_measure_mm's (stats, disks, geom) on the device, and the spacing tensor [C, 1, 2] (host) they were measured with."""
    masks = clips() if masks is None else masks
    sp = torch.tensor(SPACINGS, dtype=torch.int32).view(C, 1, 2) if spacing is None else spacing
    return hip.lv_measure_mm(torch.from_numpy(np.array(masks)).cuda(), sp, cls=1, disks=D), sp


def check(hip, recs, sp, pairs, what):
    """ops.lv_biplane against the reference on the records read back.  Returns (out, npix) as numpy arrays."""
    out, npix = hip.lv_biplane(*recs, sp, torch.tensor(pairs, dtype=torch.int32).reshape(-1, 2))
    P, Tn = len(pairs), recs[0].shape[1]
    assert out.shape == (P, Tn, 3) and out.dtype == torch.float64 and npix.shape == (P, Tn) and npix.dtype == torch.int64
    host_sp = sp.cpu().expand(recs[0].shape[0], Tn, 2).numpy()
    want, want_n = R.lv_biplane_ref(*(r.cpu().numpy().tolist() for r in recs), host_sp, pairs)
    got, got_n = out.cpu().numpy(), npix.cpu().numpy()
    want, want_n = np.asarray(want, np.float64).reshape(P, Tn, 3), np.asarray(want_n, np.int64).reshape(P, Tn)
    err = np.abs(got - want) / np.where(want != 0, np.abs(want), 1.0)
    print(f"{what}: largest relative difference {err.max() if err.size else 0.0:.2e}")
    assert np.array_equal(got_n, want_n), (what, got_n.tolist(), want_n.tolist())
    assert (np.abs(got - want) <= RTOL * np.abs(want)).all(), (what, got.tolist(), want.tolist())
    return got, got_n


def test_main_case_self_pair_and_swap(hip):
    recs, sp = records(hip, 20)
    assert int(recs[0][..., 0].min()) > 0
    got, got_n = check(hip, recs, sp, PAIRS, "main")
    assert (got[..., 0] > 0).all() and (got_n > 0).all()
    # the pair (4, 4) is clip 4's single-plane volume: the same terms in another order of operations
    single, L = recs[2][4, :, 1].cpu().numpy(), recs[2][4, :, 0].cpu().numpy()
    print("self pair:", (np.abs(got[2, :, 0] - single) / single).max())
    assert (np.abs(got[2, :, 0] - single) <= RTOL * single).all()
    assert np.array_equal(got[2, :, 1], L) and not got[2, :, 2].any() and np.array_equal(got_n[2], recs[0][4, :, 0].cpu().numpy())
    # the views swapped: bit for bit
    swapped, swapped_n = check(hip, recs, sp, [[1, 0], [2, 3], [4, 4]], "swapped")
    assert swapped.tobytes() == got.tobytes() and np.array_equal(swapped_n, got_n)
    # two calls: bit for bit
    again, again_n = check(hip, recs, sp, PAIRS, "again")
    assert again.tobytes() == got.tobytes() and np.array_equal(again_n, got_n)
    # the device spacing table as lv_measure_mm expanded it
    dev_sp = sp.cuda().expand(C, T, 2).contiguous()
    dev, dev_n = check(hip, recs, dev_sp, PAIRS, "device spacing")
    assert dev.tobytes() == got.tobytes()


def test_empty_frames_and_bad_spacings_give_zeros(hip):
    """Frame 1 of clip 1 holds no pixel of the class; clip 3 has a device spacing of 0 in every frame: its records are -1."""
    masks = clips().copy()
    masks[1, 1] = 0
    sp = torch.tensor(SPACINGS, dtype=torch.int32).view(C, 1, 2).expand(C, T, 2).clone()
    sp[3, :, 0] = 0
    dev_sp = sp.cuda()
    recs, _ = records(hip, 20, masks, dev_sp)
    assert int(recs[0][1, 1, 0]) == 0 and (recs[0][3] == -1).all() and (recs[2][3] == -1.0).all()
    got, got_n = check(hip, recs, dev_sp, PAIRS + [[1, 1], [3, 3], [2, 3]], "invalid")
    assert not got[0, 1].any() and got_n[0, 1] == 0 and got[0, 0, 0] > 0 and got[0, 2, 0] > 0          # pair (0, 1): frame 1 only
    for p in (1, 4, 5):                                      # every pair with clip 3
        assert not got[p].any() and not got_n[p].any()
    assert not got[3, 1].any() and got_n[3, 1] == 0 and got[3, 0, 0] > 0


@pytest.mark.parametrize("D", [1, 64])
def test_one_disk_and_sixty_four(hip, D):
    recs, sp = records(hip, D)
    got, _ = check(hip, recs, sp, PAIRS, f"D = {D}")
    assert (got[..., 0] > 0).all()


def test_one_frame_and_no_pair(hip):
    recs, sp = records(hip, 20, clips()[:, :1])
    assert recs[0].shape == (C, 1, 12)
    check(hip, recs, sp, PAIRS, "T = 1")
    out, npix = hip.lv_biplane(*recs, sp, torch.empty((0, 2), dtype=torch.int32))
    assert out.shape == (0, 1, 3) and npix.shape == (0, 1) and out.dtype == torch.float64 and npix.dtype == torch.int64


def test_seventy_pairs(hip):
    """70 pairs x 3 frames = 210 waves in 53 workgroups, the last of them half used: every pair of two of the clips, repeated."""
    recs, sp = records(hip, 20)
    pairs = [[k % C, (k // C + 2 * k) % C] for k in range(70)]
    assert len({tuple(p) for p in pairs}) == C * C
    out, _ = hip.lv_biplane(*recs, sp, torch.tensor(pairs, dtype=torch.int32))
    got, _ = check(hip, recs, sp, pairs, "70 pairs")
    assert out.cpu().numpy().tobytes() == got.tobytes()
    for k, p in enumerate(pairs):                            # a row depends on its pair alone
        first = pairs.index(p)
        assert got[k].tobytes() == got[first].tobytes()


def test_refusals_on_the_device(hip):
    recs, sp = records(hip, 20)
    with pytest.raises(hip.GdkvmError, match="outside 0..4"):
        hip.lv_biplane(*recs, sp, torch.tensor([[0, 5]], dtype=torch.int32))
    with pytest.raises(hip.GdkvmError, match="host tensor"):
        hip.lv_biplane(*recs, sp, torch.tensor(PAIRS, dtype=torch.int32).cuda())
    with pytest.raises(hip.GdkvmError, match="spacing_um"):
        hip.lv_biplane(*recs, torch.tensor([[0, 300]], dtype=torch.int32), torch.tensor(PAIRS, dtype=torch.int32))
