"""The boundary loss of include/gdkvm.h restated (gdkvm_signed_distance, gdkvm_seg_loss_boundary_fwd / _bwd), independent of the product's
code: the signed squared distance maps in exact integers (brute force over pixel pairs, and a separable numpy transform for larger frames),
phi, and the whole objective in fp64 torch, so that autograd gives the gradient."""
import numpy as np
import torch
import torch.nn.functional as F


def sd2_bruteforce(t: np.ndarray, num_classes: int) -> np.ndarray:
    """int64 [C, H, W] from one frame of labels [H, W]: every pixel against every pixel of the other kind."""
    H, W = t.shape
    yy, xx = np.mgrid[0:H, 0:W]
    py, px = yy.reshape(-1).astype(np.int64), xx.reshape(-1).astype(np.int64)
    out = np.zeros((num_classes, H, W), np.int64)
    for c in range(num_classes):
        a = (t == c).reshape(-1)
        if not a.any() or a.all():
            continue
        d2 = (py[:, None] - py[None, :]) ** 2 + (px[:, None] - px[None, :]) ** 2           # [HW, HW]
        to_in = np.where(a[None, :], d2, np.iinfo(np.int64).max).min(1)
        to_out = np.where(~a[None, :], d2, np.iinfo(np.int64).max).min(1)
        out[c] = np.where(a, -to_out, to_in).reshape(H, W)
    return out


def _dist2_to(s: np.ndarray) -> np.ndarray:
    """int64 [H, W]: squared distance of every pixel to the nearest True pixel of s (s has one).  Columns first, then one minimum per row."""
    H, W = s.shape
    none = 1 << 20
    g = np.full((H, W), none, np.int64)
    d = np.full(W, none, np.int64)
    for y in range(H):
        d = np.where(s[y], 0, np.minimum(d + 1, none))
        g[y] = d
    d = np.full(W, none, np.int64)
    for y in range(H - 1, -1, -1):
        d = np.where(s[y], 0, np.minimum(d + 1, none))
        g[y] = np.minimum(g[y], d)
    dx2 = (np.arange(W)[:, None] - np.arange(W)[None, :]).astype(np.int64) ** 2       # [x, x']
    out = np.empty((H, W), np.int64)
    for y in range(H):
        out[y] = (dx2 + (g[y] ** 2)[None, :]).min(1)
    return out


def sd2_reference(target, num_classes: int) -> np.ndarray:
    """int64 [..., C, H, W] from labels [..., H, W] (numpy or torch; any integer type): the definition, by the separable transform."""
    t = np.asarray(target.cpu() if isinstance(target, torch.Tensor) else target).astype(np.int64)
    H, W = t.shape[-2:]
    flat = t.reshape(-1, H, W)
    out = np.zeros((flat.shape[0], num_classes, H, W), np.int64)
    for f in range(flat.shape[0]):
        for c in range(num_classes):
            a = flat[f] == c
            if a.any() and not a.all():
                out[f, c] = np.where(a, -_dist2_to(~a), _dist2_to(a))
    return out.reshape(*t.shape[:-2], num_classes, H, W)


def phi(sd2) -> torch.Tensor:
    """fp64 signed distance from the signed squared distance: sqrt(s) outside, -(sqrt(-s) - 1) inside, 0 at 0."""
    s = torch.as_tensor(np.asarray(sd2)).double() if not isinstance(sd2, torch.Tensor) else sd2.double()
    r = s.abs().sqrt()
    return torch.where(s > 0, r, torch.where(s < 0, 1.0 - r, torch.zeros_like(s)))


def objective(logits: torch.Tensor, target: torch.Tensor, dice_weight: float, eps: float, boundary_weight: float, classes=None, sd2=None):
    """(loss, ce, dice, L_B) in fp64 from FULL-resolution logits [N, C, H, W] (fp64, may require grad) and labels [N, H, W] on the CPU."""
    n, c, H, W = logits.shape
    tg = target.long()
    lab = (tg >= 0) & (tg < c)
    nlab = lab.sum().clamp_min(1).double()
    logp = logits.log_softmax(1)
    safe = torch.where(lab, tg, torch.zeros_like(tg))
    ce = -(logp.gather(1, safe.unsqueeze(1)).squeeze(1) * lab).sum() / nlab
    p = logp.exp() * lab.unsqueeze(1)
    oh = (F.one_hot(safe, c) * lab.unsqueeze(-1)).permute(0, 3, 1, 2).double()
    dice = 1.0 - ((2 * (p * oh).sum((0, 2, 3)) + eps) / (p.sum((0, 2, 3)) + oh.sum((0, 2, 3)) + eps)).mean()
    if sd2 is None:
        sd2 = sd2_reference(tg, c)
    take = torch.zeros(c, dtype=torch.float64)
    take[list(range(1, c)) if classes is None else list(classes)] = 1.0
    lb = (p * phi(sd2) * take.view(1, c, 1, 1)).sum() / nlab
    return ce + dice_weight * dice + boundary_weight * lb, ce, dice, lb


def objective_lowres(z: torch.Tensor, target: torch.Tensor, dice_weight: float, eps: float, boundary_weight: float, classes=None, sd2=None):
    """The same from stride-k logits z [N, C, h, w] (fp64): bilinear enlargement to the labels' size, align_corners = false."""
    up = F.interpolate(z, size=tuple(target.shape[-2:]), mode="bilinear", align_corners=False)
    return objective(up, target, dice_weight, eps, boundary_weight, classes, sd2)


def label_frame(H: int, W: int, num_classes: int, seed: int) -> np.ndarray:
    """uint8 [H, W]: class 1 a blob with a hole, scattered pixels of every class, and some 255s."""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    t = np.zeros((H, W), np.uint8)
    r2 = ((yy - 0.45 * H) / max(0.3 * H, 1.0)) ** 2 + ((xx - 0.55 * W) / max(0.25 * W, 1.0)) ** 2
    t[r2 < 1.0] = 1
    t[r2 < 0.08] = 0                                                  # the hole
    k = max(1, H * W // 40)
    t[rng.randint(0, H, k), rng.randint(0, W, k)] = rng.randint(0, num_classes, k)
    t[rng.randint(0, H, k), rng.randint(0, W, k)] = 255
    return t
