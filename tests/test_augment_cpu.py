"""Host side of the clip augmentation: the parameter sampler (data.ClipAugment) and its configuration block.  No device needed."""
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = np.array([1, 0, 0, 0, 1, 0, 1, 0, 1, 0, 0, 0], np.float32)
REAL = dict(rotate_deg=20, scale=(0.8, 1.25), translate=0.1, hflip=0.5, gain=(0.8, 1.2), bias=0.1, gamma=(0.6, 1.6))


def test_degenerate_ranges_give_the_exact_identity_row():
    from gdkvm_amd.data import IDENTITY_ROW, ClipAugment
    for H, W in ((112, 112), (30, 58), (37, 41), (256, 256)):
        rows = ClipAugment(seed=7, rank=3).params(epoch=2, index=5, B=4, H=H, W=W)
        assert rows.dtype == torch.float32 and tuple(rows.shape) == (4, 12)
        assert np.array_equal(rows.numpy(), np.tile(IDENTITY, (4, 1)))
        assert not np.signbit(rows.numpy()).any()
    assert np.array_equal(np.array(IDENTITY_ROW, np.float32), IDENTITY)


def test_rows_repeat_for_the_same_arguments_and_differ_across_ranks_and_batches():
    from gdkvm_amd.data import ClipAugment
    a = ClipAugment(seed=1, rank=0, **REAL)
    base = a.params(3, 4, 8, 112, 112)
    assert torch.equal(base, ClipAugment(seed=1, rank=0, **REAL).params(3, 4, 8, 112, 112))     # a resumed run repeats its epoch
    assert not torch.equal(base, ClipAugment(seed=1, rank=1, **REAL).params(3, 4, 8, 112, 112))
    assert not torch.equal(base, ClipAugment(seed=2, rank=0, **REAL).params(3, 4, 8, 112, 112))
    assert not torch.equal(base, a.params(3, 5, 8, 112, 112))
    assert not torch.equal(base, a.params(4, 4, 8, 112, 112))
    assert len({tuple(r) for r in base.numpy().tolist()}) == 8                                 # clips of a batch differ
    assert (base[:, 9:] == 0).all()
    g, b, gm = base[:, 6].numpy(), base[:, 7].numpy(), base[:, 8].numpy()
    assert (g >= 0.8).all() and (g <= 1.2).all() and (np.abs(b) <= 0.1 + 1e-7).all() and (gm >= 0.6 - 1e-6).all() and (gm <= 1.6 + 1e-6).all()


def test_the_row_inverts_the_stated_forward_transform():
    """p' = A (p - c) + c + (tx W, ty H), A = scale R(angle) diag(+-1, 1): the four frame corners mapped forward in float64 and back through
    the fp32 row return to themselves within 1e-3 pixels at 256^2."""
    from gdkvm_amd.data import ClipAugment
    H = W = 256
    aug = ClipAugment(seed=11, rank=2, **REAL)
    d, rows = aug.draw(1, 9, 16), aug.params(1, 9, 16, H, W).numpy().astype(np.float64)
    assert d["flip"].any() and not d["flip"].all()
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    corners = np.array([[0, 0], [W - 1, 0], [0, H - 1], [W - 1, H - 1]], np.float64)
    worst = 0.0
    for b in range(16):
        a = math.radians(d["angle_deg"][b])
        assert abs(d["angle_deg"][b]) <= 20 and 0.8 <= d["scale"][b] <= 1.25 and abs(d["tx"][b]) <= 0.1 and abs(d["ty"][b]) <= 0.1
        A = d["scale"][b] * np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]) @ np.diag([-1.0 if d["flip"][b] else 1.0, 1.0])
        for p in corners:
            q = A @ (p - c) + c + np.array([d["tx"][b] * W, d["ty"][b] * H])
            back = np.array([rows[b, 0] * q[0] + rows[b, 1] * q[1] + rows[b, 2], rows[b, 3] * q[0] + rows[b, 4] * q[1] + rows[b, 5]])
            worst = max(worst, np.abs(back - p).max())
        assert np.allclose(rows[b, 6:9], [d["gain"][b], d["bias"][b], d["gamma"][b]], rtol=1e-6, atol=1e-7)
    assert worst <= 1e-3, worst


def test_bad_ranges_are_refused():
    from gdkvm_amd.data import ClipAugment
    for kw in (dict(scale=(1.2, 0.9)), dict(gamma=(0.0, 1.0)), dict(hflip=1.5), dict(rotate_deg=-5), dict(seed=-1)):
        with pytest.raises(ValueError):
            ClipAugment(**kw)


def test_config_block():
    from gdkvm_amd.config import load_config
    from gdkvm_amd.data import ClipAugment, build_augment
    cfg = load_config(os.path.join(ROOT, "config", "config_gdkvm_01.yaml"))
    assert cfg.augment.enabled is False and build_augment(cfg, 0) is None
    assert cfg.to_dict()["augment"]["scale"] == [1.0, 1.0]
    cfg = load_config(None, ["augment.enabled=true", "augment.rotate_deg=10", "augment.scale=[0.9, 1.1]", "seed=4"])
    assert cfg.augment.enabled is True and cfg.augment.rotate_deg == 10 and cfg.augment.hflip == 0.0
    aug = build_augment(cfg, 3)
    assert isinstance(aug, ClipAugment) and (aug.rotate_deg, aug.scale, aug.seed, aug.rank) == (10.0, (0.9, 1.1), 4, 3)
    with pytest.raises(KeyError, match="shear"):
        load_config(None, ["augment.shear=1"])


def test_prefetcher_takes_the_arguments_without_a_device_call():
    """augment / epoch are plain constructor arguments (train.py passes them every epoch); staging is what touches the device."""
    import inspect
    from gdkvm_amd.pipeline import DevicePrefetcher
    sig = inspect.signature(DevicePrefetcher.__init__).parameters
    assert sig["augment"].default is None and sig["epoch"].default == 0
