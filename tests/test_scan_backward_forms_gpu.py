"""The Dk = 64 scan backward (gdkvm_scan_bwd, gdkvm_scan_state_bwd, gdkvm_scan_train_bwd: the reverse mode of gdr_affine_scan_kernel,
gdr_bwd_g_kernel, gdr_bwd_frame_kernel) in the forms training selects: bf16 I/O, every clip length, every subset of gradients asked
for, across calls and past its grid caps.  Cases, references and bounds are those of tests/scan_bwd_forms.py, proved on the CPU by
tests/test_scan_backward_forms_cpu.py.

Two kinds of comparison, and nothing else:
  * small cases against fp64 autograd through oracle/torch_ref.py on the inputs as the kernel reads them, at the bound of
    test_scan_backward_fp32 / test_scan_backward_bf16_io (scan_bwd_forms.allowed);
  * long and large cases bit for bit against a composition of smaller calls of the same kernels (torch.equal): a clip cut into calls
    with the state -- and, backwards, its gradient -- handed on as an fp32 tensor, and a batch of clips against each clip alone.

Every test prints `err / allowed` per gradient tensor (pytest -s).  Worst figure per group, measured on the MI355X -- for the gradients
a bf16 call stores as bf16 (whose figure is the final rounding: half an ulp, 2^-9 |ref|, against the bound's 2^-7 |ref|), and for the fp32
tensors (all six in an fp32 call; d_alpha, d_beta, d_s0 in a bf16 call):
                                                                       bf16-stored   fp32 tensors (fp32 call / bf16 call)
  group 1 (bf16 grid, shapes, wide values, > 64 tokens, narrow keys)   0.4827        0.0073 / 0.0148
  group 2 (every clip length)                                          0.4811        0.0189 / 0.0123
  group 3 (which gradients are asked for)                              0.4730        0.0074 / 0.0060
  group 4 (ops.scan_state_bwd called directly)                         0.4793        0.0088 / 0.0118
  group 7 (the real size, clip 0 against fp64)                         0.4851             -- / 0.0076
  groups 5 and 6 and the second half of group 7 are bit for bit and hold exactly: no figure.  No case exposed a kernel defect.

The pad-gates launch of gdkvm_scan_train_fwd has B T C 65 Hh items against a cap of 16384 x 256: it needs more than 64527 pseudo-frame
heads in one call, which no clip reaches; it is not crossed here."""
import numpy as np
import pytest
import torch

from tests import scan_bwd_forms as F

pytestmark = pytest.mark.gpu
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _report(group, tag, got, ref, bf16):
    """Prints err / allowed per tensor, then returns the tensors beyond their bound (the caller asserts there are none)."""
    w = F.worst(got, ref, bf16)
    print(f"[group {group}] {tag}: " + " ".join(f"d_{n} {v:.4f}" for n, v in w.items()) + f" | worst {max(w.values()):.4f}")
    return {n: v for n, v in w.items() if not v <= 1.0}


# ------------------------------------------------------------------------------------------------------------------ group 1
@pytest.mark.parametrize("case", F.GROUP1, ids=str)
def test_backward_against_fp64(hip, case):
    """The bf16 twin of test_scan_backward_fp32 (every rule x flags), the bf16 twin of test_scan_backward_shapes plus a ragged two-head
    shape, value widths beyond 256 in both I/O types, frames of more than 64 tokens in bf16 (_ScanTrainFunction) and keys of 32
    channels through ops.scan's padding -- all with a non-zero carried state and dS."""
    inp = F.make_inputs(case)
    bad = _report(1, case, F.hip_grads(hip, inp), F.ref_grads(inp), inp.bf16)
    assert not bad, (case, bad)


# ------------------------------------------------------------------------------------------------------------------ group 2
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_backward_every_clip_length(hip, dtype):
    """The reverse mode of gdr_affine_scan_kernel walks its running pointers backwards from frame T - 1 through an unrolled body of
    UFD = 6 frames and a peeled tail: T = 1..14, 18, 19 take every tail behind zero, one, two and three bodies; frames of 65 tokens
    do the same over Tc = 2T pseudo-frames."""
    for pseudo, lengths in ((False, F.CLIP_LENGTHS), (True, F.PSEUDO_CLIP_LENGTHS)):
        for T in lengths:
            inp = F.make_inputs(F.clip_case(T, dtype, pseudo))
            bad = _report(2, f"{dtype} N={inp.q.shape[2]} T={T}", F.hip_grads(hip, inp), F.ref_grads(inp), inp.bf16)
            assert not bad, (T, pseudo, bad)


# ------------------------------------------------------------------------------------------------------------------ group 3
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", list(F.ASKED_MODES))
def test_backward_of_the_gradients_asked_for(hip, mode, dtype):
    """Loss on R only (without and with a state input), on S_T only (the read-out's gradient arrives as zeros) and on both.  Autograd
    materialises the gradient nobody asked for as zeros; the entry's own NULL branches (no d_s_out; no d_s_in) are taken by calling
    ops.scan_bwd directly, against the same reference."""
    want, with_s0 = F.ASKED_MODES[mode]
    inp = F.make_inputs(F._c(F.ASKED_SHAPE, dtype=dtype))
    ref = F.ref_grads(inp, want, with_s0)
    bad = _report(3, f"{mode} {dtype}", F.hip_grads(hip, inp, want, with_s0), ref, inp.bf16)
    assert not bad, (mode, bad)
    if want == "R":
        B, T, N, Hh, Dv = F.ASKED_SHAPE
        t = F.to_device(inp)
        ws = hip.new_workspace(B, T, Hh, N, 64, Dv, t.q.device)
        hist = torch.empty((B, T, Hh, 64, Dv), dtype=torch.float32, device=t.q.device)
        hip.scan_fwd(t.q, t.k, t.v, t.alpha, t.beta, t.s0 if with_s0 else None, inp.rule, inp.flags, workspace=ws, state_hist=hist)
        out = hip.scan_bwd(t.q, t.k, t.v, t.alpha, t.beta, hist, ws, t.dR, None, inp.rule, inp.flags, need_d_state_in=with_s0)
        assert (out[5] is None) == (not with_s0)
        got = {n: g.float().cpu().numpy() for n, g in zip(F.NAMES, out) if g is not None}
        bad = _report(3, f"{mode} {dtype} scan_bwd(d_state_out=None)", got, ref, inp.bf16)
        assert not bad, (mode, bad)


# ------------------------------------------------------------------------------------------------------------------ group 4
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("shape", F.STATE_BWD_SHAPES)
def test_state_bwd_called_directly(hip, shape, dtype):
    """gdkvm_scan_state_bwd on its own: the gradient of <d_hist, hist> + <dS, S_T> (hist: the state before every frame) with d_hist
    and d_state_out both given, d_hist only, d_state_out only (the branch that zero-fills the additive term) and neither (every
    gradient exactly zero)."""
    B, T, N, Hh, Dv = shape
    inp = F.make_inputs(F._c(shape, dtype=dtype))
    d_hist = np.random.default_rng(sum(shape)).standard_normal((B, T, Hh, 64, Dv)).astype(np.float32)
    t = F.to_device(inp)
    ws = hip.new_workspace(B, T, Hh, N, 64, Dv, t.q.device)
    hist = torch.empty((B, T, Hh, 64, Dv), dtype=torch.float32, device=t.q.device)
    hip.scan_fwd(t.q, t.k, t.v, t.alpha, t.beta, t.s0, workspace=ws, state_hist=hist, flags=3)
    dh = torch.from_numpy(d_hist).cuda()
    for want_hist, want_state in ((True, True), (True, False), (False, True), (False, False)):
        out = hip.scan_state_bwd(t.k, t.v, t.alpha, t.beta, hist, ws, dh if want_hist else None, t.dS if want_state else None, 2, 3)
        got = {n: g.float().cpu().numpy() for n, g in zip(F.NAMES[1:], out)}
        if not (want_hist or want_state):
            assert all(not g.any() for g in got.values()), {n: np.abs(g).max() for n, g in got.items()}
            continue
        ref = F.ref_state_grads(inp, d_hist, want_hist, want_state)
        bad = _report(4, f"{shape} {dtype} d_hist={want_hist} d_state_out={want_state}", got, ref, inp.bf16)
        assert not bad, (want_hist, want_state, bad)


# ------------------------------------------------------------------------------------------------------------------ group 5
def _run(hip, inp, t, cuts=()):
    """[R, S_T, d_q, d_k, d_v, d_alpha, d_beta, d_s0] of one ops.scan call (cuts empty) or of a chain of calls over consecutive pieces
    of the clip, the state handed on as a tensor (autograd hands each piece's d_s_in to the piece before it)."""
    ts = [getattr(t, n).detach().clone().requires_grad_() for n in F.NAMES]
    s, Rs = ts[5], []
    for lo, hi in F.pieces(ts[0].shape[1], cuts):
        # (a copy of its own per piece: a slice of a one-clip tensor is contiguous where it lies, and no 16-byte-aligned operand)
        r, s = hip.scan(*(x[:, lo:hi].clone(memory_format=torch.contiguous_format) for x in ts[:5]), s, inp.rule, inp.flags)
        Rs.append(r)
    R = torch.cat(Rs, 1) if len(Rs) > 1 else Rs[0]
    torch.autograd.backward([R, s], [t.dR, t.dS])
    return [R.detach(), s.detach()] + [x.grad for x in ts]


def _assert_identical(a, b, what):
    names = ["R", "S"] + ["d_" + n for n in F.NAMES]
    print(f"[bit for bit] {what}: max|a - b| " + " ".join(f"{n} {(x.float() - y.float()).abs().max().item():.1e} (of {x.float().abs().max().item():.1e})"
                                                         for n, x, y in zip(names, a, b)))
    for name, x, y in zip(["R", "S"] + ["d_" + n for n in F.NAMES], a, b):
        assert torch.isfinite(x).all() and x.any(), (what, name, "nothing to compare")
        assert torch.equal(x, y), (what, name, (x.float() - y.float()).abs().max().item(), x.float().abs().max().item())


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", F.CHAIN_CASES, ids=str)
def test_backward_across_calls_bit_identity(hip, case, dtype):
    """A clip cut into calls with the state carried == one call, bit for bit, values and all six gradients: the reverse recurrence runs
    on the three-term operands whose state scale is 1, so a d_s_in written and read back as fp32 is the value the one call carried in
    registers, and the frame kernel is frame-local given the two histories."""
    shape, cuts, rule, flags = case
    inp = F.make_inputs(F._c(shape, rule, flags, dtype))
    t = F.to_device(inp)
    _assert_identical(_run(hip, inp, t), _run(hip, inp, t, cuts), (case, dtype))


def test_backward_of_a_300_frame_clip_in_calls_of_at_most_38(hip):
    """The long clip, with nothing running on the CPU: 300 frames in bf16 against a chain of nine calls of 38, 37, .. 31 and 24 frames."""
    shape, cuts, rule, flags = F.LONG_CHAIN
    inp = F.make_inputs(F._c(shape, rule, flags, "bf16"))
    t = F.to_device(inp)
    _assert_identical(_run(hip, inp, t), _run(hip, inp, t, cuts), shape)


# ------------------------------------------------------------------------------------------------------------------ groups 6 and 7
def _device_inputs(shape, seed):
    """bf16 inputs of ordinary magnitude made on the device (the large shapes: nothing runs on the CPU)."""
    B, T, N, Hh, Dv = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    return F.NS(q=rn(B, T, N, Hh, 64).bfloat16(), k=rn(B, T, N, Hh, 64).bfloat16(), v=rn(B, T, N, Hh, Dv).bfloat16(),
                alpha=2.0 + rn(B, T, Hh), beta=rn(B, T, N, Hh), s0=0.3 * rn(B, Hh, 64, Dv), dR=rn(B, T, N, Hh, Dv).bfloat16(), dS=rn(B, Hh, 64, Dv))


def _clips_alone(hip, t, what):
    """The call on all clips against the call on each clip alone, bit for bit on R, S_T and every gradient."""
    rule_flags = F.NS(rule=2, flags=3)
    both = _run(hip, rule_flags, t)
    for b in range(t.q.shape[0]):
        one = _run(hip, rule_flags, F.NS(**{n: x[b:b + 1].contiguous() for n, x in vars(t).items()}))
        _assert_identical([x[b:b + 1] for x in both], one, (what, "clip", b))
        del one


@pytest.mark.parametrize("shape", [F.ROWS_TO_IMG_SHAPE, F.COPY_GRID_SHAPE], ids=str)
def test_clips_are_independent_past_the_grid_caps(hip, shape):
    """Two clips of 65-token frames in one call: gdr_rows_to_img_kernel past its 8192 workgroups (T = 130), the padded-value copy of
    gdkvm_scan_train_fwd past copy_grid's 16384 (T = 550); each clip alone stays under both caps (test_scan_backward_forms_cpu.py)."""
    _clips_alone(hip, _device_inputs(shape, sum(shape)), shape)


def test_backward_at_the_real_size(hip):
    """cfg2's clip: 32 frames of 49 tokens, Dv = 256, bf16 -- clip 0 against fp64, and the two-clip call equal to the single-clip calls."""
    inp = F.make_inputs(F._c(F.REAL_SHAPE))
    one = F.clip_of(inp, 0)
    bad = _report(7, F.REAL_SHAPE, F.hip_grads(hip, one), F.ref_grads(one), True)
    assert not bad, bad
    _clips_alone(hip, F.to_device(inp), F.REAL_SHAPE)
