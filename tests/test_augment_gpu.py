"""gdkvm_augment_clips (csrc/augment.hip) behind ops.augment_clips, and the prefetcher that calls it: the uint8 -> [0, 1] cast of a batch of
clips with one affine warp and one intensity table per clip, labels warped alike.  The reference is the float64 numpy restatement of
include/gdkvm.h's semantics below (it imports nothing from the product).

Bounds.  fp32 frames 1e-4 absolute, bf16 frames 2^-8 absolute (half an ulp of bf16 below 1 is 2^-9; bilinear sampling with zero padding is
continuous in the coordinates, so no pixel is excluded).  Labels: equal at every pixel whose sx + 0.5 and sy + 0.5 both lie at least 2^-10
from an integer -- the only place where fp32 and float64 rounding may pick different neighbours -- and the excluded share is asserted to be
at most 1 % per case, so the band cannot hide a failure."""
import math
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0)
FILL = 255


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def _row(angle_deg, scale, tx, ty, flip, H, W, gain=1.0, bias=0.0, gamma=1.0):
    """fp32 row of the INVERSE of  p' = A (p - c) + c + (tx, ty),  A = scale R(angle) diag(-1 if flip else 1, 1),  c the frame centre
    (tx, ty in pixels)."""
    a = math.radians(angle_deg)
    A = scale * np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]) @ np.diag([-1.0 if flip else 1.0, 1.0])
    Ai = np.linalg.inv(A)
    c = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
    off = c - Ai @ (c + np.array([tx, ty]))
    return np.array([Ai[0, 0], Ai[0, 1], off[0], Ai[1, 0], Ai[1, 1], off[1], gain, bias, gamma, 0, 0, 0], np.float32)


def _reference(frames, target, params, fill=FILL):
    """float64 frames [B,T,C,H,W], labels [B,T,H,W] (or None) and, per clip, the pixels OUTSIDE the rounding band [B,H,W]; coordinates in
    float64 from the fp32 matrix entries."""
    B, T, C, H, W = frames.shape
    out = np.zeros(frames.shape, np.float64)
    tout = None if target is None else np.empty_like(target)
    safe = np.zeros((B, H, W), bool)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    for b in range(B):
        m = params[b].astype(np.float64)
        sx, sy = m[0] * xs + m[1] * ys + m[2], m[3] * xs + m[4] * ys + m[5]
        u = np.arange(256, dtype=np.float64) / 255.0
        lut = np.clip(m[6] * (u if m[8] == 1.0 else u ** m[8]) + m[7], 0.0, 1.0)
        x0, y0 = np.floor(sx), np.floor(sy)
        fx, fy = sx - x0, sy - y0
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

        def tap(img, yy, xx):
            ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            return np.where(ok, lut[img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]], 0.0)

        for t in range(T):
            for c in range(C):
                img = frames[b, t, c]
                top = (1 - fx) * tap(img, y0, x0) + fx * tap(img, y0, x0 + 1)
                bot = (1 - fx) * tap(img, y0 + 1, x0) + fx * tap(img, y0 + 1, x0 + 1)
                out[b, t, c] = (1 - fy) * top + fy * bot
        hx, hy = sx + 0.5, sy + 0.5
        ix, iy = np.floor(hx).astype(np.int64), np.floor(hy).astype(np.int64)
        safe[b] = (np.abs(hx - np.round(hx)) >= 2.0 ** -10) & (np.abs(hy - np.round(hy)) >= 2.0 ** -10)
        if target is not None:
            ok = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
            for t in range(T):
                tout[b, t] = np.where(ok, target[b, t][np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)], fill)
    return out, tout, safe


def _clips(shape, seed, classes=4):
    """Random bytes (every value 0..255 occurs) and labels in 4 x 4 blocks."""
    rng = np.random.default_rng(seed)
    B, T, C, H, W = shape
    frames = rng.integers(0, 256, shape, dtype=np.uint8)
    target = rng.integers(0, classes, (B, T, (H + 3) // 4, (W + 3) // 4), dtype=np.uint8).repeat(4, -2).repeat(4, -1)[..., :H, :W]
    return frames, np.ascontiguousarray(target)


def _plain_cast(frames_u8, dtype):
    return torch.mul(frames_u8, 1.0 / 255.0, out=torch.empty(frames_u8.shape, dtype=dtype, device=frames_u8.device))


DTYPES = [torch.float32, torch.bfloat16]
TDTYPES = [torch.uint8, torch.int64]


# ---- identity and exact maps ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt", TDTYPES, ids=["u8", "i64"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_identity_row_is_the_plain_cast_bit_for_bit(hip, dtype, tdt):
    f, t = _clips((2, 3, 3, 30, 58), 1)
    f, t = torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda().to(tdt)
    par = torch.tensor([IDENTITY] * 2, dtype=torch.float32, device="cuda")
    of, ot = hip.augment_clips(f, t, par, dtype, fill_label=FILL)
    assert of.dtype == dtype and ot.dtype == tdt
    assert torch.equal(of, _plain_cast(f, dtype))
    assert torch.equal(ot, t)
    of2, none = hip.augment_clips(f, None, par, dtype)                  # no labels: frames alone
    assert none is None and torch.equal(of2, of)


@pytest.mark.parametrize("tdt", TDTYPES, ids=["u8", "i64"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_flip_shift_and_quarter_turn_are_exact(hip, dtype, tdt):
    """Source coordinates land on pixel centres: bit-equal to the moved plain cast, zero / fill_label where the source falls outside."""
    S = 41
    f, t = _clips((1, 2, 1, S, S), 2)
    f, t = torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda().to(tdt)
    base = _plain_cast(f, dtype)
    row = lambda six: torch.tensor([list(six) + [1, 0, 1, 0, 0, 0]], dtype=torch.float32, device="cuda")

    of, ot = hip.augment_clips(f, t, row([-1, 0, S - 1, 0, 1, 0]), dtype, fill_label=FILL)          # left-right mirror
    assert torch.equal(of, base.flip(-1)) and torch.equal(ot, t.flip(-1))

    of, ot = hip.augment_clips(f, t, row([1, 0, -3, 0, 1, 2]), dtype, fill_label=7)                # content moves by (+3, -2) pixels
    ef, et = torch.zeros_like(base), torch.full_like(t, 7)
    ef[..., 0:S - 2, 3:S] = base[..., 2:S, 0:S - 3]
    et[..., 0:S - 2, 3:S] = t[..., 2:S, 0:S - 3]
    assert torch.equal(of, ef) and torch.equal(ot, et)

    of, ot = hip.augment_clips(f, t, row([0, 1, 0, -1, 0, S - 1]), dtype, fill_label=FILL)          # 90 degrees: (x, y) reads (y, S-1-x)
    yy, xx = torch.meshgrid(torch.arange(S, device="cuda"), torch.arange(S, device="cuda"), indexing="ij")
    assert torch.equal(of, base[..., S - 1 - xx, yy]) and torch.equal(ot, t[..., S - 1 - xx, yy])


# ---- general warps against the float64 reference ----------------------------------------------------------------------------------------
GEO = [(17.0, 1.13, 2.3, -1.7, False), (-9.0, 0.9, -3.25, 1.5, True), (33.0, 1.0, 0.4, 0.2, False)]
TONE = [(1.2, -0.05, 0.7), (0.85, 0.1, 1.6), (1.0, 0.0, 1.0)]
CASES = {  # shape -> (geometry, tone) per clip
    "scalar_30x58": ((2, 3, 3, 30, 58), [(0, 0), (1, 1)]),         # H W = 1740 = 4 * 435: element stores with bf16 output, 16-byte stores with fp32
    "odd_37x41": ((1, 1, 1, 37, 41), [(2, 2)]),                    # odd everything, C = 1, T = 1: element stores in both dtypes
    "vector_32x64": ((2, 2, 3, 32, 64), [(2, 1), (0, 0)]),         # 16-byte stores, two (fp32) tiles per frame
}
_REF = {}


def _case(name):
    if name not in _REF:
        shape, picks = CASES[name]
        f, t = _clips(shape, 10 + len(_REF))
        par = np.stack([_row(*GEO[g], shape[3], shape[4], *TONE[i]) for g, i in picks])
        _REF[name] = (f, t, par) + _reference(f, t, par)
    return _REF[name]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_general_warp_matches_the_float64_reference(hip, name, dtype):
    f, t, par, rf, rt, safe = _case(name)
    for tdt in TDTYPES:
        of, ot = hip.augment_clips(torch.from_numpy(f).cuda(), torch.from_numpy(t).cuda().to(tdt), torch.from_numpy(par).cuda(), dtype,
                                   fill_label=FILL)
        of, ot = of.float().cpu().numpy().astype(np.float64), ot.cpu().numpy()
        err = np.abs(of - rf).max()
        excluded = 1.0 - safe.mean(axis=(1, 2)).min()
        keep = np.broadcast_to(safe[:, None], rt.shape)
        wrong = int((ot[keep] != rt[keep]).sum())
        print(f"{name} {dtype} target {tdt}: max|frames - ref| = {err:.3e}; labels wrong outside the band: {wrong}; excluded share {excluded:.4f}")
        assert of.min() >= 0.0 and of.max() <= 1.0
        assert err <= (1e-4 if dtype == torch.float32 else 2.0 ** -8)
        assert excluded <= 0.01
        assert wrong == 0
        assert set(np.unique(ot)) <= set(np.unique(t)) | {FILL}
        assert (rt == FILL).any()                                          # the case does leave the frame somewhere


def test_one_warp_per_clip_and_one_row_per_clip(hip):
    """The same source frame T times gives T identical outputs; swapping the two clips' rows swaps their outputs."""
    f, t = _clips((1, 1, 3, 30, 58), 5)
    f = torch.from_numpy(f).cuda().expand(2, 4, 3, 30, 58).contiguous()
    t = torch.from_numpy(t).cuda().expand(2, 4, 30, 58).contiguous()
    par = torch.from_numpy(np.stack([_row(*GEO[0], 30, 58, *TONE[0]), _row(*GEO[1], 30, 58, *TONE[1])])).cuda()
    of, ot = hip.augment_clips(f, t, par, torch.float32)
    for k in range(1, 4):
        assert torch.equal(of[:, k], of[:, 0]) and torch.equal(ot[:, k], ot[:, 0])
    assert not torch.equal(of[0], of[1]) and not torch.equal(ot[0], ot[1])
    sf, st = hip.augment_clips(f, t, par.flip(0).contiguous(), torch.float32)
    assert torch.equal(sf, of.flip(0)) and torch.equal(st, ot.flip(0))


def test_argument_errors(hip):
    f = torch.zeros(2, 2, 3, 8, 8, dtype=torch.uint8, device="cuda")
    t = torch.zeros(2, 2, 8, 8, dtype=torch.uint8, device="cuda")
    par = torch.tensor([IDENTITY] * 2, dtype=torch.float32, device="cuda")
    E = hip.GdkvmError
    with pytest.raises(E, match="uint8"):
        hip.augment_clips(f.float(), t, par, torch.float32)                # float frames are not augmented
    with pytest.raises(E, match="device"):
        hip.augment_clips(f.cpu(), t.cpu(), par.cpu(), torch.float32)      # no CPU path
    with pytest.raises(E, match="params"):
        hip.augment_clips(f, t, par[:, :11].contiguous(), torch.float32)
    with pytest.raises(E, match="fill_label"):
        hip.augment_clips(f, t, par, torch.float32, fill_label=300)
    with pytest.raises(E, match="target"):
        hip.augment_clips(f, t[:, :, :7].contiguous(), par, torch.float32)
    with pytest.raises(E, match="frames_dtype"):
        hip.augment_clips(f, t, par, torch.float16)
    lib = hip.load()                                                       # the C entry point checks for itself
    args = lambda **kw: [kw.get(k, v) for k, v in dict(frames=f.data_ptr(), target=t.data_ptr(), params=par.data_ptr(),
                                                       out=torch.empty(f.shape, device="cuda").data_ptr(), tout=torch.empty_like(t).data_ptr(),
                                                       B=2, T=2, C=3, H=8, W=8, io=0, tb=1, fill=255, stream=None).items()]
    assert lib.gdkvm_augment_clips(*args(fill=300)) == -6
    assert lib.gdkvm_augment_clips(*args(tb=4)) == -2
    assert lib.gdkvm_augment_clips(*args(io=2)) == -2
    assert lib.gdkvm_augment_clips(*args(C=0)) == -1
    assert lib.gdkvm_augment_clips(*args(tout=None)) == -6
    assert lib.gdkvm_augment_clips(*args(frames=None)) == -6
    assert lib.gdkvm_augment_clips(*args(B=0, frames=None, out=None)) == 0  # nothing to do: no launch


# ---- the prefetcher -----------------------------------------------------------------------------------------------------------------------
def _host_batches(n, shape, seed, classes=4):
    out = []
    for i in range(n):
        f, t = _clips(shape, seed + i, classes)
        out.append((torch.from_numpy(f), torch.from_numpy(t)))
    return out


def _drain(pre):
    return [(f.clone(), t.clone()) for f, t in pre]


def test_prefetcher_augments_in_its_cast_pass(hip):
    from gdkvm_amd.data import ClipAugment
    from gdkvm_amd.pipeline import DevicePrefetcher
    dev = torch.device("cuda", torch.cuda.current_device())
    shape = (2, 2, 3, 30, 58)
    src = _host_batches(3, shape, 40)
    plain = _drain(DevicePrefetcher(src, dev, slots=3, frames_dtype=torch.float32))
    for kw in ({"augment": None}, {"augment": ClipAugment(seed=5), "epoch": 3}):      # off, and on with every range degenerate
        got = _drain(DevicePrefetcher(src, dev, slots=3, frames_dtype=torch.float32, **kw))
        assert len(got) == 3
        for (gf, gt), (pf, pt) in zip(got, plain):
            assert gf.dtype == pf.dtype and gt.dtype == pt.dtype and torch.equal(gf, pf) and torch.equal(gt, pt)

    aug = ClipAugment(rotate_deg=15, scale=(0.9, 1.15), translate=0.06, hflip=0.5, gain=(0.8, 1.2), bias=0.05, gamma=(0.7, 1.4), seed=3, rank=1)
    for fdt in DTYPES:
        a = _drain(DevicePrefetcher(src, dev, slots=3, frames_dtype=fdt, augment=aug, epoch=2))
        b = _drain(DevicePrefetcher(src, dev, slots=2, frames_dtype=fdt, augment=aug, epoch=2, threaded=True))
        assert len(a) == len(b) == 3
        for i, ((af, at), (bf, bt)) in enumerate(zip(a, b)):
            ef, et = hip.augment_clips(src[i][0].cuda(), src[i][1].cuda(), aug.params(2, i, 2, 30, 58).cuda(), fdt, fill_label=255)
            assert af.dtype == fdt and at.dtype == torch.uint8
            assert torch.equal(af, ef) and torch.equal(at, et) and torch.equal(bf, ef) and torch.equal(bt, et)
            assert set(at.unique().tolist()) <= set(src[i][1].unique().tolist()) | {255}
            assert not torch.equal(af, plain[i][0].to(fdt))                                   # it did warp
        assert not torch.equal(a[0][0], _drain(DevicePrefetcher(src, dev, frames_dtype=fdt, augment=aug, epoch=3))[0][0])   # epochs differ
    with pytest.raises(ValueError, match="uint8"):
        next(iter(DevicePrefetcher([(src[0][0].float(), src[0][1])], dev, augment=aug)))


def test_train_steps_on_augmented_clips(hip, monkeypatch):
    """Two eager train_step calls at default widths, bf16, on 2 x 2 x 3 x 64^2 synthetic byte clips through an augmenting prefetcher:
    finite losses, and no layer leaves the hand-written path (library fallbacks are fatal here)."""
    import gdkvm_amd.model
    from gdkvm_amd.data import ClipAugment, SyntheticEchoClips
    from gdkvm_amd.model import GDKVM, GDKVMConfig
    from gdkvm_amd.pipeline import DevicePrefetcher
    from gdkvm_amd.train import train_step
    monkeypatch.setattr(gdkvm_amd.model, "_STRICT", True)
    dev = torch.device("cuda", torch.cuda.current_device())
    ds = SyntheticEchoClips(4, 2, 64, num_classes=2, seed=1, as_uint8=True)
    batches = [tuple(torch.stack(x) for x in zip(ds[2 * i], ds[2 * i + 1])) for i in range(2)]
    assert batches[0][0].shape == (2, 2, 3, 64, 64) and batches[0][0].dtype == torch.uint8
    torch.manual_seed(0)
    model = GDKVM(GDKVMConfig()).train().to(dev).to(memory_format=torch.channels_last)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    aug = ClipAugment(rotate_deg=10, scale=(0.9, 1.1), translate=0.05, hflip=0.5, gain=(0.9, 1.1), bias=0.05, gamma=(0.8, 1.25), seed=0)
    losses = []
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        for frames, target in DevicePrefetcher(batches, dev, slots=3, frames_dtype=torch.float32, augment=aug, epoch=0):
            losses.append(float(train_step(model, opt, frames, target, torch.bfloat16)))
    assert len(losses) == 2 and all(np.isfinite(losses)), losses
    assert not [w for w in rec if "gdkvm" in str(w.message).lower()], [str(w.message) for w in rec]
