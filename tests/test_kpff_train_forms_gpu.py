"""gdkvm_kpff_fwd_train's four saves (gates, lp, gp, gms) and the KPFF backward in the forms that training batches select: two sub-tiles
per workgroup (`pair`), two 56-row sub-tiles (`packed56`), column-tiled grids (w > 16) and grids cut into row bands -- the small batches of
tests/test_backward_gpu.py and the training tests all run the one-tile form, and tests/test_configs_gpu.py sees only the output F of the
large ones.  (The epilogue's row index `grow` serves F and the saves alike, so a slip in it shows in the forward tests at w > 16; the saves'
own indexing -- the gms loop's `sb * SB + tok`, a row computed apart for the saves -- was unguarded.)  tests/test_kpff_forms_cpu.py proves, from the host arithmetic restated in tests/kpff_forms.py, which form, tile shapes and trip
counts each case here selects; batch sizes follow the device's compute-unit count.

References are float64 (oracle/torch_ref.py and numpy) from the kernels' own inputs.  The mixes and gates are compared with the reference
evaluated on the kernel's own saved pooled feature, which is itself compared with the float64 pooling first: its rounding is paid once.
Bounds (those of test_kpff_bf16_io_exact_arm, test_kpff_fp32_on_bf16_splits and test_kpff_fp32 in tests/test_kpff_argmax_gpu.py):
    bf16 I/O   gms  2^-8 |ref| + 1e-6 (one rounding)        lp / gp / gates / F  1e-4 max(1, max|ref|) + 2^-8 |ref|
    fp32 I/O   gms  1e-5                                    lp / gp / gates / F  3e-5 (arm on bf16 splits), 2e-5 (exact arm)
Every test prints the maxima it measured (pytest -s)."""
import functools

import pytest
import torch

from oracle import torch_ref as TR
from tests import kpff_forms as kf
from tests.util import make_kpff_inputs

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp32": torch.float32}
SAVES = ("F", "gates", "lp", "gp", "gms")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def _inputs(bt, h, w, ck, cv, cp):
    """(L, G, P, Wa, ba, Wl, Wg) as float32 CPU tensors, made once per shape and never written."""
    return tuple(torch.from_numpy(x) for x in make_kpff_inputs(bt, h, w, ck, cv, cp, seed=bt + 3 * h + 5 * w + ck + cv + cp))


def _on_device(arrs, io, frames=slice(None)):
    return [x[frames].cuda().to(DT[io]).contiguous() for x in arrs[:3]], [x.cuda() for x in arrs[3:]]


def _fwd_train(hip, feats, weights, h, w, workspace=True):
    """gdkvm_kpff_fwd_train as ops._KpffFunction calls it; the outputs start as NaN, so an element no workgroup wrote fails every check."""
    L, G, P = feats
    BT, N, Ck = L.shape
    Cv, Cp = G.shape[-1], P.shape[-1]
    dev = L.device
    new = lambda c: torch.full((BT, N, c), float("nan"), dtype=L.dtype, device=dev)
    out = dict(F=new(Cp), gates=new(2 * Cp), lp=new(Cp), gp=new(Cp), gms=new(Cv))
    ws = hip.kpff_workspace(L, G, P) if workspace else None
    hip._call("gdkvm_kpff_fwd_train", dev, L, G, P, *weights, out["F"], out["gates"], out["lp"], out["gp"], out["gms"], hip._Ws(ws),
              BT, Ck, Cv, Cp, h, w, hip._io_dtype(L))
    return out


def _reference(feats, weights, h, w, gms=None):
    """float64: the pooled feature, and gates / mixes / output from it (or from `gms` where given)."""
    L, G, P = feats
    Wa, ba, Wl, Wg = weights
    Cp = P.shape[-1]
    pooled = TR.multiscale_pool(G, h, w)
    gm = pooled if gms is None else gms
    gates = torch.sigmoid(torch.cat([P, L, gm], -1) @ Wa.T + ba)
    lp, gp = L @ Wl.T, gm @ Wg.T
    return dict(gms=pooled, gates=gates, lp=lp, gp=gp, F=P + gates[..., :Cp] * lp + gates[..., Cp:] * gp)


def _check_saves(got, feats, weights, h, w, io, arm, label):
    """`got` (device, I/O type) against float64 from the features as the kernel read them and the weights as its arm reads them."""
    f64 = [x.double().cpu() for x in feats]
    rw = (lambda x: x.bfloat16()) if arm == "bf16" else (lambda x: x)             # the bf16 arm packs Wa / Wl / Wg as bf16; ba stays fp32
    w64 = [(x if i == 1 else rw(x)).double().cpu() for i, x in enumerate(weights)]
    mine = {k: v.double().cpu() for k, v in got.items()}
    pooled = TR.multiscale_pool(f64[1], h, w)
    e = (mine["gms"] - pooled).abs()
    lim = 2.0 ** -8 * pooled.abs() + 1e-6 if io == "bf16" else torch.full_like(pooled, 1e-5)
    print("%s gms: max err %.3e, max err / allowed %.3f" % (label, e.max().item(), (e / lim).max().item()))
    assert bool((e <= lim).all()), (label, "gms", e.max().item(), (e / lim).max().item())
    # (the exact arm keeps the pooled feature in fp32 in its tile and rounds only the copy it saves: in bf16 I/O its mixes are those of the
    # unrounded feature)
    ref = _reference(f64, w64, h, w, gms=None if (arm, io) == ("exact", "bf16") else mine["gms"])
    for name in ("lp", "gp", "gates", "F"):
        r = ref[name]
        e = (mine[name] - r).abs()
        if io == "bf16":
            lim = 1e-4 * max(1.0, r.abs().max().item()) + 2.0 ** -8 * r.abs()
        else:
            lim = torch.full_like(r, 3e-5 if arm == "split" else 2e-5)
        print("%s %s: max err %.3e, max err / allowed %.3f" % (label, name, e.max().item(), (e / lim).max().item()))
        assert bool((e <= lim).all()), (label, name, e.max().item(), (e / lim).max().item())


# ------------------------------------------------------------------------------------------------------------------ (a)
_SAVE_CASES = [("bf16", "bf16", kf.CASES[c][0] + kf.CASES[c][1]) for c in kf.SAVES_BF16] \
    + [("fp32", "split", kf.CASES[c][0] + kf.CASES[c][1]) for c in kf.SAVES_SPLIT] \
    + [(io, "exact", c) for c in kf.SAVES_EXACT for io in ("bf16", "fp32")]


@pytest.mark.parametrize("io,arm,case", _SAVE_CASES, ids=["%s-%s-%s" % (io, arm, "x".join(map(str, c))) for io, arm, c in _SAVE_CASES])
def test_saves_against_float64_in_every_arm(hip, io, arm, case):
    """Three frames (the one-tile form of the bf16 arm, the arm on bf16 splits, the exact arm in both I/O types): each save against float64.
    Measured on an MI355X, the largest error over the cases (and the largest error / bound of any element):
        bf16 arm            gms 6.4e-3 (0.996: half an ulp next to a power of two)  lp 1.56e-2 (0.95)  gp 7.4e-3 (0.95)  gates 1.95e-3 (0.95)  F 1.55e-2 (0.93)
        exact arm, bf16 I/O gms 5.3e-3 (0.98)  lp 7.8e-3 (0.94)  gp 6.4e-3 (0.92)  gates 1.95e-3 (0.95)  F 1.46e-2 (0.89)
        arm on bf16 splits  gms 2.6e-7  lp 2.76e-5 (0.92 of 3e-5, at 6 x 19)  gp 1.43e-5  gates 4.6e-6  F 2.18e-5
        exact arm, fp32     gms 1.9e-7  lp 7.1e-7  gp 4.3e-7  gates 2.2e-7  F 6.0e-7 (0.035 of 2e-5 at most)
    The same checks on three frames of the threshold batches (the next test): within 0.996 / 0.95 / 0.95 / 0.95 / 0.94 of the bf16 bounds."""
    h, w, ck, cv, cp = case
    assert kf.arm(io, ck, cv, cp, workspace=arm != "exact" or io == "bf16") == arm
    arrs = _inputs(kf.SMALL_BT, h, w, ck, cv, cp)
    feats, weights = _on_device(arrs, io)
    got = _fwd_train(hip, feats, weights, h, w, workspace=not (arm == "exact" and io == "fp32"))
    _check_saves(got, feats, weights, h, w, io, arm, "%s/%s %s" % (io, arm, case))


# ------------------------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("case", sorted(kf.CASES))
def test_large_batch_forms_equal_the_one_tile_form_bit_for_bit(hip, case):
    """The fewest frames that select `pair` / `packed56` on this device in ONE call, against calls over slices that each stay on the one-tile
    form (the first cut at an odd frame: with one tile per frame that slice starts on the second sub-tile of a workgroup): the output and the
    four saves are the same bits.  First, middle and last frame of the one call are also checked against float64 as above."""
    (h, w), (ck, cv, cp), form, odd = kf.CASES[case]
    cus, t = _cus(), kf.tiling(h, w)
    bt = kf.threshold_bt(h, w, cus, odd)
    assert kf.bf16_form(bt * t.tiles, cus, t.rows * t.cols, cp + ck + cv).form == form and (not odd or (bt * t.tiles) % 2 == 1)
    arrs = _inputs(bt, h, w, ck, cv, cp)
    feats, weights = _on_device(arrs, "bf16")
    full = _fwd_train(hip, feats, weights, h, w)
    for f0, f1 in kf.slices(bt, h, w, cus):
        assert kf.bf16_form((f1 - f0) * t.tiles, cus, t.rows * t.cols, cp + ck + cv).form == "single"
        part = _fwd_train(hip, [x[f0:f1].clone() for x in feats], weights, h, w)
        for name in SAVES:
            a, b = full[name][f0:f1], part[name]
            assert torch.equal(a, b), (case, name, (f0, f1), int((a != b).sum()), int(torch.isnan(a.float()).sum()))
    frames = [0, bt // 2, bt - 1]
    _check_saves({k: v[frames] for k, v in full.items()}, [x[frames] for x in feats], weights, h, w, "bf16", "bf16", "%s/%s %d frames" % (case, form, bt))


# ------------------------------------------------------------------------------------------------------------------ (c)
def _bounded(got, ref, io, label):
    """fp32: 1e-6 max(1, max|ref|); bf16: one rounding of the fp32 value, 2^-8 |ref| + 1e-6."""
    e = (got.double() - ref).abs()
    lim = 2.0 ** -8 * ref.abs() + 1e-6 if io == "bf16" else torch.full_like(ref, 1e-6 * max(1.0, ref.abs().max().item()))
    print("%s: max err %.3e, max err / allowed %.3f, max|ref| %.3f" % (label, e.max().item(), (e / lim).max().item(), ref.abs().max().item()))
    assert bool((e <= lim).all()), (label, e.max().item(), (e / lim).max().item())


@pytest.mark.parametrize("io", ["fp32", "bf16"])
@pytest.mark.parametrize("case", kf.PRE_CASES, ids=["x".join(map(str, c)) for c in kf.PRE_CASES])
def test_bwd_pre_on_its_own(hip, case, io):
    """gdkvm_kpff_bwd_pre against float64 from its own inputs, on one trip of its grid-stride loop, on two (the second partial) and on seven.
    Measured on an MI355X: fp32 dz 3.6e-7 (0.11 of the bound), dlp / dgp 1.2e-7 (0.035); bf16: every output within 0.995 of one rounding."""
    bt, n, cp = case
    m = bt * n
    g = torch.Generator(device="cuda").manual_seed(m + cp)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
    dF, lp, gp = (rnd(m, cp).to(DT[io]) for _ in range(3))
    gates = torch.sigmoid(rnd(m, 2 * cp)).to(DT[io])
    new = lambda c: torch.full((m, c), float("nan"), dtype=DT[io], device="cuda")
    dz, dlp, dgp = new(2 * cp), new(cp), new(cp)
    hip._call("gdkvm_kpff_bwd_pre", dF.device, dF, gates, lp, gp, dz, dlp, dgp, bt, n, cp, hip._io_dtype(dF))
    d, gl, gg = dF.double(), gates.double()[:, :cp], gates.double()[:, cp:]
    label = "bwd_pre %s %s (%d trips)" % (io, case, kf.bwd_pre_trips(m, cp).trips)
    _bounded(dz, torch.cat([d * lp.double() * gl * (1 - gl), d * gp.double() * gg * (1 - gg)], 1), io, label + " dz")
    _bounded(dlp, d * gl, io, label + " dlp")
    _bounded(dgp, d * gg, io, label + " dgp")


def _pool_adjoint(v, h, w):
    """The adjoint of the multi-scale pooling on float64 [BT, h * w, C]: an output token's gradient goes back to its own input token, and in
    equal shares to every token of its 2 x 2 and of its 4 x 4 cell (cells clipped at the grid's edge), a third each."""
    bt, n, c = v.shape
    g = v.reshape(bt, h, w, c)
    out = g / 3.0
    for s in (2, 4):
        for y0 in range(0, h, s):
            for x0 in range(0, w, s):
                cell = g[:, y0:y0 + s, x0:x0 + s]
                out[:, y0:y0 + s, x0:x0 + s] += cell.sum((1, 2), keepdims=True) / (3.0 * cell.shape[1] * cell.shape[2])
    return out.reshape(bt, n, c)


@pytest.mark.parametrize("io", ["fp32", "bf16"])
@pytest.mark.parametrize("name,hw,chan", kf.POST_CASES, ids=[c[0] for c in kf.POST_CASES])
def test_bwd_post_on_its_own(hip, name, hw, chan, io):
    """gdkvm_kpff_bwd_post against float64 from its own inputs: dP and dL are sums of two terms, dG the pooling's adjoint of a sum.
    Measured on an MI355X: fp32 dP / dL 2.4e-7 (0.046 of the bound), dG 4.2e-7 (0.14); bf16: every output within 0.996 of one rounding."""
    (h, w), (ck, cv, cp) = hw, chan
    bt, n, cin = kf.SMALL_BT, h * w, cp + ck + cv
    g = torch.Generator(device="cuda").manual_seed(7 * h + w + cin)
    rnd = lambda *s: torch.randn(*s, device="cuda", generator=g).to(DT[io])
    dF, dX, dL_add, dG_add = rnd(bt, n, cp), rnd(bt, n, cin), rnd(bt, n, ck), rnd(bt, n, cv)
    new = lambda c: torch.full((bt, n, c), float("nan"), dtype=DT[io], device="cuda")
    dP, dL, dG = new(cp), new(ck), new(cv)
    hip._call("gdkvm_kpff_bwd_post", dF.device, dF, dX, dL_add, dG_add, dP, dL, dG, bt, ck, cv, cp, h, w, hip._io_dtype(dF))
    x = dX.double().cpu()
    label = "bwd_post %s %s %dx%d" % (io, name, h, w)
    _bounded(dP.cpu(), dF.double().cpu() + x[..., :cp], io, label + " dP")
    _bounded(dL.cpu(), x[..., cp:cp + ck] + dL_add.double().cpu(), io, label + " dL")
    want = _pool_adjoint((x[..., cp + ck:] + dG_add.double().cpu()).numpy(), h, w)
    _bounded(dG.cpu(), torch.from_numpy(want), io, label + " dG")


# ------------------------------------------------------------------------------------------------------------------ (d)
_BACKWARD = [("bf16", c) for c in kf.BACKWARD_BF16] + [("fp32", c) for c in kf.BACKWARD_FP32]


@pytest.mark.parametrize("io,case", _BACKWARD, ids=["%s-%s" % x for x in _BACKWARD])
def test_whole_backward_in_the_large_forms(hip, io, case):
    """hip.kpff(...).backward(dF) at the threshold batch against float64 autograd, with the bounds of test_kpff_backward_bf16 and
    test_kpff_backward_fp32 (tests/test_backward_gpu.py); and the gradients of the three features equal, bit for bit, those of calls over
    slices that stay on the one-tile form -- a token's row of every product of the backward (gdkvm_gemm_nt: a fixed order over K, edge
    tiles zero-filled) does not depend on the rows beside it.  The weight gradients are sums over all frames: no slice has them."""
    (h, w), (ck, cv, cp), form, odd = kf.CASES[case]
    cus = _cus()
    bt = kf.threshold_bt(h, w, cus, odd)
    arrs = _inputs(bt, h, w, ck, cv, cp)
    dF = torch.randn(bt, h * w, cp, generator=torch.Generator().manual_seed(50 + bt)).to(DT[io])

    def run(frames):
        gs = [(x[frames].to(DT[io]) if i < 3 else x).cuda().requires_grad_() for i, x in enumerate(arrs)]
        hip.kpff(*gs, h, w).backward(dF[frames].cuda())
        return [t.grad for t in gs]

    got = run(slice(None))
    rnd = (lambda i, x: x.bfloat16() if i != 4 else x) if io == "bf16" else (lambda i, x: x)          # as the bf16 arm sees them
    ts = [rnd(i, x).double().requires_grad_() for i, x in enumerate(arrs)]
    (TR.kpff(*ts, h, w) * dF.double()).sum().backward()
    for name, g, t in zip("L G P Wa ba Wl Wg".split(), got, ts):
        r = t.grad
        err, scale = (g.double().cpu() - r).abs(), r.abs().max().item()
        print("backward %s %s/%s %d frames d%s: max err %.3e mean %.3e, max|ref| %.3e" % (io, case, form, bt, name, err.max().item(), err.mean().item(), scale))
        if io == "bf16":
            assert err.max().item() <= 0.03 * scale + 1e-2 and err.mean().item() <= 4e-3 * scale + 1e-3, (name, err.max().item(), err.mean().item(), scale)
        else:
            assert err.max().item() <= 2e-4 * max(1.0, scale), (name, err.max().item(), scale)
    for f0, f1 in kf.slices(bt, h, w, cus):
        part = run(slice(f0, f1))
        for name, a, b in zip("L G P".split(), got, part):
            assert torch.equal(a[f0:f1], b), (case, io, name, (f0, f1), int((a[f0:f1] != b).sum()))
