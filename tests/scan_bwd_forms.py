"""The cases of tests/test_scan_backward_forms_gpu.py and the host arithmetic they rest on (csrc/gdr_scan.hip, gdr_scan_bwd.hip,
gdr_train.hip), restated in plain Python: how many unrolled bodies and which peeled tail the state waves of gdr_affine_scan_kernel take
for a clip of T frames, how many 64-token pseudo-frames a frame of N tokens becomes, how many workgroups gdr_rows_to_img_kernel and the
pad / un-pad copies of gdkvm_scan_train_fwd / _bwd launch for a shape and whether that count hit its cap.  Beside them the references
the GPU tests compare with -- fp64 autograd through oracle/torch_ref.py, on the inputs as the kernels read them -- the bound per gradient
tensor, and the slips a case must be able to see.  tests/test_scan_backward_forms_cpu.py pins every constant below to the .hip source
and proves the claims, the references and the sensitivity of every case without a GPU."""
from types import SimpleNamespace as NS

import numpy as np
import torch

from oracle import gdkvm_oracle as O
from oracle import torch_ref as TR
from tests import grid_caps as gc
from tests.util import make_scan_inputs

# name -> (value, file, where, regex with ONE group holding the constant's expression): the format of tests/grid_caps.py CONSTANTS.
CONSTANTS = {
    "AFF_PD": (2, "gdr_scan.hip", None, r"constexpr int AFF_PD = (\d+);"),
    "ROWS_TO_IMG_CAP": (8192, "gdr_scan_bwd.hip", "scan_bwd_impl", r"/ 256 > (\d+) \? \1 :"),
    "COPY_GRID_CAP": (16384, "gdr_train.hip", "copy_grid", r"g > (\d+) \? \1 :"),
    "FRAME_CHUNK": (64, "gdr_scan_bwd.hip", "gdr_bwd_frame_kernel", r"const int nchunk = \(Dv \+ 63\) / (\d+);"),
    "PSEUDO_FRAME": (64, "gdr_train.hip", "train_carve", r"v\.C = N > 64 \? \(N \+ 63\) / (\d+) : 1;"),
    "PSEUDO_ABOVE": (64, "gdr_train.hip", "train_carve", r"v\.C = N > (\d+) \?"),
}
globals().update({k: v[0] for k, v in CONSTANTS.items()})
# Expressions the functions below restate (no single literal to read): test_scan_backward_forms_cpu.py pins their text.
SOURCE_LINES = (
    ("gdr_scan.hip", "constexpr int NR = AFF_PD + 1, UFD = NR % 2 == 0 ? NR : 2 * NR;"),
    ("gdr_scan.hip", "for (; t0 + UFD <= T; t0 += UFD)"),
    ("gdr_scan.hip", "static_for<0, UFD - 1>([&](auto fc) {"),
    ("gdr_scan.hip", "if (t0 + F < T) frame(t0 + F, od[F % NR], od[(F + AFF_PD) % NR], scaled_c);"),
    ("gdr_scan_bwd.hip", "const size_t n_img = (size_t)B * T * Hh * (Dv / 16) * 4 * 64;"),
    ("gdr_scan_bwd.hip", "const int nchunk = (Dv + 63) / 64;"),
    ("gdr_train.hip", "unsigned copy_grid(size_t n) { const size_t g = (n + 255) / 256; return (unsigned)(g > 16384 ? 16384 : (g ? g : 1)); }"),
    ("gdr_train.hip", "v.Tc = T * v.C;"),
    ("gdr_train.hip", "const size_t kq = (size_t)N * Hh * Dk * es / 16, kpq = (size_t)tv.C * 64 * Hh * Dk * es / 16;"),
    ("gdr_train.hip", "const size_t vq = (size_t)N * Hh * Dv * es / 16, vpq = (size_t)tv.C * 64 * Hh * Dv * es / 16;"),
    ("gdr_train.hip", "dim3(copy_grid(BT * kpq))"),
    ("gdr_train.hip", "dim3(copy_grid(BT * vpq))"),
    ("gdr_train.hip", "dim3(copy_grid(BT * tv.C * 65 * Hh))"),
    ("gdr_train.hip", "dim3(copy_grid(BT * kq))"),
    ("gdr_train.hip", "dim3(copy_grid(BT * vq))"),
    ("gdr_train.hip", "dim3(copy_grid(BT * (N + 1) * Hh))"),
)
NAMES = "q k v alpha beta s0".split()


def source_constant(name, csrc=gc.CSRC):
    return gc.source_constant(name, csrc, CONSTANTS)


# ---------------------------------------------------------------------------------------------------------------------------------------
# Host arithmetic
def ufd():
    """Frames per unrolled body of the state waves: NR = AFF_PD + 1 operand registers, UFD = NR if NR is even, else 2 NR."""
    nr = AFF_PD + 1
    return nr if nr % 2 == 0 else 2 * nr


def pseudo_frames(N):
    """C: 64-token pseudo-frames per frame (1 up to 64 tokens: the frame itself)."""
    return -(-N // PSEUDO_FRAME) if N > PSEUDO_ABOVE else 1


def clip_plan(T, N=1):
    """The serial kernel walks Tc = T * C steps: `bodies` trips through the unrolled body, then `tail` peeled frames."""
    tc = T * pseudo_frames(N)
    return NS(steps=tc, bodies=tc // ufd(), tail=tc % ufd())


def value_chunks(Dv):
    """Column chunks gdr_bwd_frame_kernel walks, and the width of the last one."""
    n = -(-Dv // FRAME_CHUNK)
    return NS(chunks=n, last=Dv - FRAME_CHUNK * (n - 1))


def rows_to_img(B, T, N, Hh, Dv):
    """gdr_rows_to_img_kernel's launch in gdkvm_scan_train_bwd (N > 64 only): one thread per 16-byte image entry of d_hist."""
    c = pseudo_frames(N)
    if c == 1:
        return None
    return gc.grid_stride(B * T * c * Hh * (Dv // 16) * 4 * 64, ROWS_TO_IMG_CAP)


def train_copies(B, T, N, Hh, Dv, es, Dk=64):
    """The six copy_grid launches of gdkvm_scan_train_fwd / _bwd for frames of more than 64 tokens (16-byte units; es bytes an element)."""
    c, bt = pseudo_frames(N), B * T
    kq, kpq = N * Hh * Dk * es // 16, c * 64 * Hh * Dk * es // 16
    vq, vpq = N * Hh * Dv * es // 16, c * 64 * Hh * Dv * es // 16
    totals = dict(pad_k=bt * kpq, pad_v=bt * vpq, pad_gates=bt * c * 65 * Hh, unpad_k=bt * kq, unpad_v=bt * vq, unpad_gates=bt * (N + 1) * Hh)
    return {k: gc.grid_stride(v, COPY_GRID_CAP) for k, v in totals.items()}


# ---------------------------------------------------------------------------------------------------------------------------------------
# The cases: (B, T, N, Hh, Dv, rule, flags, dtype name, Dk)
def _c(shape, rule=2, flags=3, dtype="bf16", Dk=64):
    return tuple(shape) + (rule, flags, dtype, Dk)


GRID_CASES = [_c((2, 4, 49, 1, 80), rule, flags) for flags in (0, 3) for rule in (0, 1, 2)]                      # group 1
SHAPE_CASES = [_c(s) for s in [(1, 2, 1, 1, 16), (2, 3, 17, 2, 32), (1, 2, 64, 1, 48), (2, 3, 63, 2, 80), (3, 5, 7, 1, 256)]]
WIDE_CASES = [_c(s, dtype=d) for s in [(1, 2, 16, 1, 272), (2, 2, 7, 2, 320)] for d in ("fp32", "bf16")]
TOKEN_CASES = [_c((2, 3, 100, 1, 32)), _c((1, 2, 130, 2, 48)), _c((1, 2, 256, 1, 64), 2, 0), _c((2, 2, 65, 1, 256), 0, 3)]
NARROW_CASES = [_c((2, 3, 20, 1, 32), dtype=d, Dk=32) for d in ("fp32", "bf16")]
GROUP1 = GRID_CASES + SHAPE_CASES + WIDE_CASES + TOKEN_CASES + NARROW_CASES

CLIP_LENGTHS = list(range(1, 15)) + [18, 19]                                                                     # group 2
PSEUDO_CLIP_LENGTHS = list(range(1, 8))


def clip_case(T, dtype, pseudo=False):
    return _c((1, T, 65 if pseudo else 5, 1, 16), dtype=dtype)


GROUP2 = [clip_case(T, d) for d in ("fp32", "bf16") for T in CLIP_LENGTHS] + [clip_case(T, d, True) for d in ("fp32", "bf16") for T in PSEUDO_CLIP_LENGTHS]

ASKED_SHAPE = (2, 4, 20, 1, 32)                                                                                  # group 3
ASKED_MODES = {"R_no_state": ("R", False), "R_with_state": ("R", True), "S_only": ("S", True), "R_and_S": ("R+S", True)}   # mode -> (loss on, s0 given)
STATE_BWD_SHAPES = [(2, 5, 17, 1, 32), (1, 7, 64, 2, 48)]                                                        # group 4
# group 5: (shape, cuts, rule, flags)
CHAIN_CASES = [((2, 12, 49, 1, 64), (1, 5), 0, 3), ((2, 12, 49, 1, 64), (1, 5), 2, 3), ((1, 6, 130, 1, 32), (2, 3), 2, 3)]
LONG_CHAIN = ((1, 300, 4, 1, 16), (38, 75, 111, 146, 180, 213, 245, 276), 2, 3)         # pieces of 38, 37, .. 31 and 24 frames
LONG_CHAIN_MAX_PIECE = 38
ROWS_TO_IMG_SHAPE = (2, 130, 65, 1, 256)                                                                         # group 6
COPY_GRID_SHAPE = (2, 550, 65, 1, 256)
REAL_SHAPE = (2, 32, 49, 1, 256)                                                                                 # group 7


def pieces(T, cuts):
    edges = (0,) + tuple(cuts) + (T,)
    return list(zip(edges[:-1], edges[1:]))


# ---------------------------------------------------------------------------------------------------------------------------------------
# Inputs, references, bounds
def make_inputs(case, seed=None):
    """Seeded inputs of a case as the kernel reads them (bf16 I/O: q, k, v and dR rounded to bf16), with a non-zero carried state and dS."""
    B, T, N, Hh, Dv, rule, flags, dtype, Dk = case
    seed = sum(case[:5]) + 7 * rule + flags + Dk if seed is None else seed
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, Dk, Dv, seed=seed, normalized=not flags, logits=bool(flags), corr=0.5)
    rng = np.random.default_rng(seed + 1)
    s0 = (0.3 * rng.standard_normal((B, Hh, Dk, Dv))).astype(np.float32)
    dR = rng.standard_normal((B, T, N, Hh, Dv)).astype(np.float32)
    dS = rng.standard_normal((B, Hh, Dk, Dv)).astype(np.float32)
    if dtype == "bf16":
        q, k, v, dR = (O.to_bf16_f32(x) for x in (q, k, v, dR))
    return NS(q=q, k=k, v=v, alpha=a, beta=b, s0=s0, dR=dR, dS=dS, rule=rule, flags=flags, bf16=dtype == "bf16", case=case)


def clip_of(inp, b):
    """Clip b of the inputs, alone."""
    out = NS(**vars(inp))
    for n in NAMES + ["dR", "dS"]:
        setattr(out, n, np.ascontiguousarray(getattr(inp, n)[b:b + 1]))
    return out


def to_device(inp):
    """The inputs as the tensors a call takes: q, k, v and dR in the I/O type, the gates, the state and dS in fp32."""
    io = torch.bfloat16 if inp.bf16 else torch.float32
    dev = lambda x, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(x)).cuda().to(dt)
    return NS(q=dev(inp.q, io), k=dev(inp.k, io), v=dev(inp.v, io), alpha=dev(inp.alpha), beta=dev(inp.beta), s0=dev(inp.s0),
              dR=dev(inp.dR, io), dS=dev(inp.dS))


def hip_grads(hip, inp, want="R+S", with_s0=True):
    """The kernels' side of ref_grads: ops.scan and autograd on the GPU; {name: fp32 numpy gradient}."""
    names = NAMES if with_s0 else NAMES[:5]
    t = to_device(inp)
    ts = [getattr(t, n).requires_grad_() for n in names]
    R, S = hip.scan(*ts, *(() if with_s0 else (None,)), inp.rule, inp.flags)
    outs = [(R, t.dR)] * ("R" in want) + [(S, t.dS)] * ("S" in want)
    torch.autograd.backward([o for o, _ in outs], [g for _, g in outs])
    return {n: x.grad.float().cpu().numpy() for n, x in zip(names, ts)}


def _f64(x):
    return torch.from_numpy(np.asarray(x, np.float64))


def ref_grads(inp, want="R+S", with_s0=True):
    """fp64 autograd through oracle.torch_ref.scan: {name: gradient} of <dR, R> (if "R" in want) + <dS, S_T> (if "S" in want)."""
    names = NAMES if with_s0 else NAMES[:5]
    ts = [_f64(getattr(inp, n)).requires_grad_() for n in names]
    R, S = TR.scan(*ts, *(() if with_s0 else (None,)), inp.rule, inp.flags)
    loss = 0
    if "R" in want:
        loss = loss + (R * _f64(inp.dR)).sum()
    if "S" in want:
        loss = loss + (S * _f64(inp.dS)).sum()
    loss.backward()
    return {n: np.zeros(t.shape) if t.grad is None else t.grad.numpy() for n, t in zip(names, ts)}      # (S_T alone does not depend on q)


def ref_chain(inp, cuts):
    """The same loss with the clip cut into calls of TR.scan, the state handed on as a tensor: (R, S_T, {name: gradient})."""
    ts = {n: _f64(getattr(inp, n)).requires_grad_() for n in NAMES}
    s, Rs = ts["s0"], []
    for lo, hi in pieces(inp.q.shape[1], cuts):
        r, s = TR.scan(*(ts[n][:, lo:hi] for n in NAMES[:5]), s, inp.rule, inp.flags)
        Rs.append(r)
    R = torch.cat(Rs, 1)
    ((R * _f64(inp.dR)).sum() + (s * _f64(inp.dS)).sum()).backward()
    return R.detach().numpy(), s.detach().numpy(), {n: t.grad.numpy() for n, t in ts.items()}


def ref_one_call(inp):
    ts = [_f64(getattr(inp, n)).requires_grad_() for n in NAMES]
    R, S = TR.scan(*ts, inp.rule, inp.flags)
    ((R * _f64(inp.dR)).sum() + (S * _f64(inp.dS)).sum()).backward()
    return R.detach().numpy(), S.detach().numpy(), {n: t.grad.numpy() for n, t in zip(NAMES, ts)}


def ref_history(ts, rule, flags):
    """The state before every frame, made differentiably: TR.scan one frame at a time with the state carried.  ts = (q, k, v, alpha,
    beta, s0) fp64 tensors; returns (hist [B,T,Hh,Dk,Dv], R, S_T)."""
    q, k, v, a, b, s = ts
    hist, Rs = [], []
    for t in range(q.shape[1]):
        hist.append(s)
        r, s = TR.scan(q[:, t:t + 1], k[:, t:t + 1], v[:, t:t + 1], a[:, t:t + 1], b[:, t:t + 1], s, rule, flags)
        Rs.append(r)
    return torch.stack(hist, 1), torch.cat(Rs, 1), s


def ref_state_grads(inp, d_hist, want_hist, want_state):
    """Gradients of <d_hist, hist> + <dS, S_T> with respect to k, v, alpha, beta and s0 (what gdkvm_scan_state_bwd returns)."""
    ts = [_f64(getattr(inp, n)).requires_grad_() for n in NAMES]
    hist, _, S = ref_history(ts, inp.rule, inp.flags)
    loss = (hist * _f64(d_hist)).sum() * (1.0 if want_hist else 0.0) + (S * _f64(inp.dS)).sum() * (1.0 if want_state else 0.0)
    loss.backward()
    return {n: t.grad.numpy() for n, t in zip(NAMES, ts) if n != "q"}


def allowed(name, ref, bf16):
    """The bound of test_scan_backward_fp32 / test_scan_backward_bf16_io: 1e-4 max(1, max|ref|), plus 2^-7 |ref| element-wise for the
    gradients a bf16 call stores as bf16 (d_q, d_k, d_v; d_alpha, d_beta and d_s0 are fp32 in both I/O types)."""
    lim = 1e-4 * max(1.0, float(np.abs(ref).max()))
    return lim + (np.abs(ref) * 2.0 ** -7 if bf16 and name in ("q", "k", "v") else 0.0)


def worst(got, ref, bf16):
    """{name: max over elements of |got - ref| / allowed}: the case passes where every figure is at most 1."""
    return {n: float((np.abs(np.asarray(got[n], np.float64) - ref[n]) / allowed(n, ref[n], bf16)).max()) for n in ref}


# ---------------------------------------------------------------------------------------------------------------------------------------
# The slips every fp64-checked case must be able to see: each returns the reference gradients as a kernel with that slip would leave them.
def _sub_inputs(inp, frames=None, cols=None):
    out = NS(**vars(inp))
    if frames is not None:
        for n in ("q", "k", "v", "alpha", "beta", "dR"):
            setattr(out, n, getattr(inp, n)[:, :frames])
    if cols is not None:
        for n in ("v", "s0", "dR", "dS"):
            setattr(out, n, np.ascontiguousarray(getattr(inp, n)[..., :cols]))
    return out


def slip_last_frame(inp, ref):
    """The reverse recurrence skips frame T - 1: dS reaches frame T - 2 as it came, and the last frame's own gradients are never written."""
    T = inp.q.shape[1]
    out = {n: np.zeros_like(r) for n, r in ref.items()}
    if T == 1:
        out["s0"] = inp.dS.astype(np.float64)
        return out
    part = ref_grads(_sub_inputs(inp, frames=T - 1))
    for n in NAMES[:5]:
        out[n][:, :T - 1] = part[n]
    out["s0"] = part["s0"]
    return out


def slip_token(inp, ref):
    """Token min(N, 64) - 1 -- the last row of the (first) 64-token tile -- gets no gradient."""
    tok = min(inp.q.shape[2], 64) - 1
    out = {n: r.copy() for n, r in ref.items()}
    for n in ("q", "k", "v", "beta"):
        out[n][:, :, tok] = 0
    return out


def slip_value_columns(inp, ref):
    """The frame kernel's chunk loop stops after its first 64 value columns (None where Dv <= 64: nothing to drop)."""
    Dv = inp.v.shape[-1]
    if Dv <= FRAME_CHUNK:
        return None
    part = ref_grads(_sub_inputs(inp, cols=FRAME_CHUNK))
    out = {n: part[n] for n in ("q", "k", "alpha", "beta")}
    for n in ("v", "s0"):
        out[n] = np.zeros_like(ref[n])
        out[n][..., :FRAME_CHUNK] = part[n]
    return out


def slip_first_decay(inp, ref):
    """d_s_in = a_0 P_0^T dS' + Qn_0^T dR_0 handed back without the a_0."""
    q0, a0 = inp.q[:, 0].astype(np.float64), inp.alpha[:, 0].astype(np.float64)            # [B,N,Hh,Dk], [B,Hh]
    if inp.flags & 1:
        q0 = q0 / np.sqrt((q0 * q0).sum(-1, keepdims=True) + TR.EPS_NORM)
    if inp.flags & 2:
        a0 = 1.0 / (1.0 + np.exp(-a0))
    gb = np.einsum("bnhd,bnhe->bhde", q0, inp.dR[:, 0].astype(np.float64))
    out = {n: r.copy() for n, r in ref.items()}
    out["s0"] = (ref["s0"] - gb) / a0[:, :, None, None] + gb
    return out


SLIPS = (slip_last_frame, slip_token, slip_value_columns, slip_first_decay)


def sees(inp, ref, slipped):
    """Whether the case's own bound is broken in at least one tensor."""
    return any(v > 1.0 for v in worst(slipped, ref, inp.bf16).values())
