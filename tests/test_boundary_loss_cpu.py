"""CPU checks of the boundary loss: the restated definition (tests/boundary_reference.py) against brute force and scipy, the host loss
(gdkvm_amd.train.segmentation_loss with boundary_weight) against the fp64 restatement, the `loss:` section of the configuration, and
train_step on CPU tensors."""
import numpy as np
import pytest
import torch

from tests import boundary_reference as B

C = 4


def _frames():
    """[5, 37, 53] uint8: two blob-with-hole frames with scattered pixels and 255s, a frame without class 2 (and 3), a frame class 0 fills, and
    a frame of 255s with one pixel of class 3."""
    a, b = B.label_frame(37, 53, C, 1), B.label_frame(37, 53, C, 2)
    absent = a.copy()
    absent[absent >= 2] = 0
    full = np.zeros((37, 53), np.uint8)
    lone = np.full((37, 53), 255, np.uint8)
    lone[36, 0] = 3
    return np.stack([a, b, absent, full, lone])


@pytest.fixture(scope="module")
def frames():
    t = _frames()
    return t, B.sd2_reference(t, C)


def test_restated_sd2_is_brute_force_and_scipy(frames):
    from scipy import ndimage
    t, sd2 = frames
    assert sd2.dtype == np.int64 and sd2.shape == (5, C, 37, 53)
    assert (t == 255).any() and (t[0] == 1).sum() > 100
    for f in range(t.shape[0]):
        assert np.array_equal(sd2[f], B.sd2_bruteforce(t[f], C)), f
        for c in range(C):
            pos = t[f] == c
            neg = ~pos
            if not pos.any() or not neg.any():
                assert not sd2[f, c].any()                              # absent, or filling the frame: zero everywhere
                continue
            e_neg, e_pos = ndimage.distance_transform_edt(neg), ndimage.distance_transform_edt(pos)
            want = np.rint(e_neg ** 2).astype(np.int64) * neg - np.rint(e_pos ** 2).astype(np.int64) * pos
            assert np.array_equal(sd2[f, c], want), (f, c)
            assert (sd2[f, c] != 0).all()
            ref_phi = e_neg * neg - (e_pos - 1.0) * pos
            assert np.abs(B.phi(sd2[f, c]).numpy() - ref_phi).max() <= 1e-12
    assert not sd2[2, 2].any() and not sd2[2, 3].any() and not sd2[3].any()      # the absent classes, the frame class 0 fills
    assert sd2[4, 3, 36, 0] == -1 and sd2[4, 3, 0, 52] == 36 ** 2 + 52 ** 2      # 255 is the complement of every class


def test_corner_pixel_at_256():
    t = np.zeros((256, 256), np.uint8)
    t[0, 0] = 1
    sd2 = B.sd2_reference(t, 2)
    assert sd2.max() == 130050 == sd2[1, 255, 255] and sd2[1, 0, 0] == -1 and sd2[0, 0, 0] == 1 and sd2[0].min() == -130050


def test_host_signed_distance_maps_are_the_definition(frames):
    from gdkvm_amd.train import signed_distance_maps
    t, sd2 = frames
    got = signed_distance_maps(torch.from_numpy(t), C)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), sd2)
    got = signed_distance_maps(torch.from_numpy(t).long().reshape(1, 5, 37, 53), C)
    assert np.array_equal(got.numpy()[0], sd2)
    thin = torch.from_numpy(np.array([[0, 1, 1, 255, 2, 0, 0]], np.uint8))
    assert np.array_equal(signed_distance_maps(thin, 3).numpy(), B.sd2_reference(thin, 3))
    assert np.array_equal(signed_distance_maps(thin.t().contiguous(), 3).numpy(), B.sd2_reference(thin.t(), 3))


@pytest.mark.parametrize("classes", [None, [2, 1]])
def test_host_loss_matches_the_fp64_restatement(frames, classes):
    from gdkvm_amd.train import segmentation_loss
    t, sd2 = frames
    tg = torch.from_numpy(t).long()
    torch.manual_seed(3)
    z = 2.0 * torch.randn(5, C, 37, 53)
    za = z.clone().requires_grad_(True)
    loss = segmentation_loss(za.reshape(1, 5, C, 37, 53), tg.reshape(1, 5, 37, 53), 0.7, 1.0, boundary_weight=0.05, boundary_classes=classes)
    loss.backward()
    zb = z.double().requires_grad_(True)
    ref, _, _, lb = B.objective(zb, tg, 0.7, 1.0, 0.05, classes, sd2)
    ref.backward()
    assert abs(lb.item()) > 0.1                                          # the term is there
    assert abs(loss.item() - ref.item()) <= 1e-4
    assert (za.grad.double() - zb.grad).abs().max() <= 1e-4 * zb.grad.abs().max()
    plain = segmentation_loss(z.reshape(1, 5, C, 37, 53), tg.reshape(1, 5, 37, 53), 0.7, 1.0)
    zero = segmentation_loss(z.reshape(1, 5, C, 37, 53), tg.reshape(1, 5, 37, 53), 0.7, 1.0, boundary_weight=0.0, boundary_classes=classes)
    assert torch.equal(plain, zero) and abs(plain.item() - loss.item()) > 1e-3
    ref0 = B.objective(z.double(), tg, 0.7, 1.0, 0.0, classes, sd2)[0]
    assert abs(plain.item() - ref0.item()) <= 1e-4


def test_host_loss_without_a_labelled_pixel():
    from gdkvm_amd.train import segmentation_loss
    z = torch.randn(1, 2, 3, 9, 11, requires_grad=True)
    loss = segmentation_loss(z, torch.full((1, 2, 9, 11), 255), 0.7, 1.0, boundary_weight=0.05)
    loss.backward()
    assert torch.isfinite(loss) and torch.isfinite(z.grad).all()


def test_loss_section_of_the_configuration(tmp_path):
    import os
    from gdkvm_amd.config import load_config
    cfg = load_config()
    assert cfg.loss.boundary_weight == 0.0 and cfg.loss.boundary_classes is None and cfg.to_dict()["loss"] == {"boundary_weight": 0.0, "boundary_classes": None}
    shipped = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "config", "config_gdkvm_01.yaml")
    assert load_config(shipped).loss.boundary_weight == 0.0                # the shipped file keeps the keys commented out
    cfg = load_config(shipped, ["loss.boundary_weight=0.01"])
    assert cfg.loss.boundary_weight == 0.01 and isinstance(cfg.loss.boundary_weight, float) and cfg.loss.boundary_classes is None
    cfg = load_config(None, ["loss.boundary_weight=1", "loss.boundary_classes=[1, 3]"])
    assert cfg.loss.boundary_weight == 1.0 and cfg.loss.boundary_classes == [1, 3]
    y = tmp_path / "c.yaml"
    y.write_text("loss:\n  boundary_weight: 0.02\n  boundary_classes: [2]\n")
    cfg = load_config(str(y))
    assert cfg.loss.boundary_weight == 0.02 and cfg.loss.boundary_classes == [2]
    with pytest.raises(KeyError):
        load_config(None, ["loss.boundary_wieght=0.01"])
    for bad in ("loss.boundary_weight=-0.1", "loss.boundary_weight=.inf", "loss.boundary_weight=.nan", "loss.boundary_weight=true",
                "loss.boundary_weight=much", "loss.boundary_classes=[4]", "loss.boundary_classes=[-1]", "loss.boundary_classes=[1, 1]",
                "loss.boundary_classes=[1.5]", "loss.boundary_classes=2"):
        with pytest.raises(ValueError):
            load_config(None, [bad])
    with pytest.raises(ValueError):
        load_config(None, ["data.num_classes=2", "loss.boundary_classes=[2]"])


def test_train_step_on_the_cpu():
    from gdkvm_amd.model import GDKVMConfig
    from gdkvm_amd.train import train_step
    from oracle.model_ref import GDKVMRef                                 # (the CPU module: plain torch)
    frames = torch.rand(1, 2, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    target = torch.from_numpy(np.stack([B.label_frame(32, 32, 2, 5), B.label_frame(32, 32, 2, 6)])).long().reshape(1, 2, 32, 32)

    def run(**kw):
        torch.manual_seed(7)
        model = GDKVMRef(GDKVMConfig(widths=(16, 32, 64), pixel_dim=64, value_dim=32)).train()
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
        loss = train_step(model, opt, frames, target, **kw)
        return loss, [p.detach().clone() for p in model.parameters()]

    plain, wp = run()
    zero, wz = run(boundary_weight=0.0, boundary_classes=[1])
    assert torch.equal(plain, zero) and all(torch.equal(a, b) for a, b in zip(wp, wz))
    with_b, wb = run(boundary_weight=0.05)
    assert torch.isfinite(with_b) and all(torch.isfinite(w).all() for w in wb)
    assert with_b.item() != plain.item() and any(not torch.equal(a, b) for a, b in zip(wp, wb))
    with pytest.raises(ValueError):
        run(boundary_weight=0.05, boundary_classes=[2])
