"""Every workspace-taking entry of gdkvm_amd.ops on poisoned, guarded outputs and workspaces (tests/poisoned_buffers.py).

Each row of ENTRIES runs four times -- unpatched, then with every torch.empty / empty_like / empty_strided of the wrappers and every
workspace filled with 0x00, 0xFF (NaN, -1, 255) and 0x5A (1.5e16, a large integer, 90) between guard bands -- and must give the same bits
each time, pass its existing reference check on the 0xFF run, leave no element of an allocation of its own unwritten, touch no guard byte,
and refuse a workspace 16 bytes short of what its size query asks.  Then a large-then-small order on the grown workspaces, the scan's range
status on workspaces nobody cleared, and a training step and a segmentation of the small model as a whole."""
import pytest
import torch

from tests import poisoned_buffers as pb

pytestmark = pytest.mark.gpu

_PARAMS = [pytest.param(r.name, i, id=f"{r.name}-{r.ids[i]}") for r in pb.ENTRIES for i in range(len(r.cases))]


def _detached(outs):
    return {k: v.detach() for k, v in outs.items() if v is not None}


def _same_bits(what, base, outs):
    assert base.keys() == outs.keys(), (what, sorted(base), sorted(outs))
    bad = [k for k in base if not pb.bit_equal(base[k], outs[k])]
    assert not bad, f"{what}: outputs {bad} differ from the unpatched run's"


def _both_unwritten(ff: pb.Poisoned, fa: pb.Poisoned):
    """Elements of the wrappers' own allocations that hold the pattern under 0xFF AND under 0x5A: no legitimate value is both."""
    a, b = ff.outputs(), fa.outputs()
    assert [(r.name.split(":")[0], r.name.split(" ")[-1], tuple(r.tensor.shape)) for r in a] == \
        [(r.name.split(":")[0], r.name.split(" ")[-1], tuple(r.tensor.shape)) for r in b], "the two runs allocated different outputs"
    left = []
    for x, y in zip(a, b):
        both = ff.unwritten(x.tensor) & fa.unwritten(y.tensor)
        if both.any():
            left.append((x.name, tuple(x.tensor.shape), int(both.sum()), both.nonzero()[0].tolist()))
    return left


@pytest.mark.parametrize("name,index", _PARAMS)
def test_entry_on_poisoned_guarded_buffers(hip, name, index):
    row = pb.row(name)
    case = row.cases[index]
    base = _detached(row.run(hip, case))
    torch.cuda.synchronize()
    runs = {}
    for byte in pb.PATTERNS:
        with pb.poisoned(byte) as p:
            outs = _detached(row.run(hip, case))
            torch.cuda.synchronize()
        p.check_guards()                                                       # 4. nothing before or after any output or workspace
        _same_bits(f"{name} {row.ids[index]} under 0x{byte:02X}", base, outs)  # 1. bit equality with the unpatched run
        runs[byte] = (p, outs)
    p_ff, outs_ff = runs[0xFF]
    asked = {r.name for r in p_ff.workspaces()}                                # no row runs without the workspaces it is there for
    assert asked and asked <= set(row.queries) and (len(row.queries) > 1 or asked == set(row.queries)), (asked, row.queries)
    for r in p_ff.workspaces():                                                # ... and each is what the query asks, at least the 16-byte floor
        assert r.tensor.numel() == r.need >= max(r.query, 16), (r.name, r.query, r.need, r.tensor.numel())
        assert r.query > 16 or r.name in pb.FLOOR_QUERIES.get(name, ()), f"{name} {row.ids[index]}: {r.name} returned {r.query}"
    row.check(hip, case, outs_ff)                                              # 2. the existing reference check, on the 0xFF run
    left = _both_unwritten(p_ff, runs[0x5A][0])                                # 3. no poison left in any allocation of the wrappers
    assert not left, f"{name} {row.ids[index]}: elements never written (site, shape, count, first index): {left}"
    # (a returned output that legitimately holds a pattern's value -- 255 in a mask, -1 in an info word -- is covered by 1: the unpatched run
    # has the same value there)
    for byte in (0xFF, 0x5A):
        p = runs[byte][0]
        for r in p.workspaces():       # a query of 0, or of the 16-byte floor (KPFF's exact arm packs nothing): those bytes are never touched
            if r.query <= 16:
                assert p.payload_intact(r), f"{name} {row.ids[index]}: {r.name} is {r.query} but the {r.need} floor bytes were written"
    # 5. 16 bytes short of a query above 16: refused, before anything was written
    for query in sorted({r.name for r in p_ff.workspaces() if r.query > 16}):
        with pb.poisoned(0xFF, short=query) as p:
            with pytest.raises(hip.GdkvmError, match="workspace"):
                row.run(hip, case)
            torch.cuda.synchronize()
        p.check_guards()
        entry, at, err = p.calls[-1]
        assert isinstance(err, hip.GdkvmError), (query, p.calls[-1])
        # (the outputs looked at are those allocated since the launch before the refused one: every wrapper allocates right before its own
        # launch.  An output allocated ahead of an EARLIER launch for the refused one to write would not be seen here.)
        since = p.calls[-2][1] if len(p.calls) > 1 else 0
        touched = [r.name for r in p.outputs(since) if r.seq < at and not p.payload_intact(r)]
        assert not touched, f"{name} {row.ids[index]}: {entry} refused a short {query} but outputs {touched} were written"
        short = [r for r in p.workspaces(query) if r.tensor.numel() < r.need]
        assert short and p.payload_intact(short[-1]), f"{name} {row.ids[index]}: {entry} wrote into the workspace it refused"


def test_zero_size_queries_are_zero_at_the_rows_shapes(hip):
    """The four entries whose query is 0 for every shape were run above with a 16-byte floor buffer that must stay untouched; here: the query
    really is 0 at those shapes, so the branch above was taken."""
    for q in pb.ZERO_SIZE:
        (row,) = [r for r in pb.ENTRIES if q in r.queries]
        with pb.poisoned(0x5A) as p:
            row.run(hip, row.cases[0])
            torch.cuda.synchronize()
        recs = p.workspaces(q)
        assert recs and all(r.query == 0 and r.need == 16 and p.payload_intact(r) for r in recs), q
        p.check_guards()


# ------------------------------------------------------------------------------------------------------------------ grown workspaces
@pytest.mark.parametrize("name", ["conv3x3_wgrad", "conv_wgrad_strided"])
def test_small_call_after_a_large_one_on_the_grown_workspace(hip, name):
    """ops._grown_workspace hands a small layer the largest layer's buffer, stale partial blocks included, and passes the C side the grown
    byte count: the small result must equal, bit for bit, the one on a workspace of exactly its own size, and nothing past its own share of
    the buffer may be written (the share's layout comes from the dims, not from workspace_bytes)."""
    row = pb.row(name)
    query = row.queries[0]
    exact, need = {}, {}
    for case in row.cases:
        with pb.poisoned(0xFF) as p:
            exact[case] = _detached(row.run(hip, case))
            torch.cuda.synchronize()
        p.check_guards()
        (need[case],) = [r.need for r in p.workspaces(query)]
    cases = sorted(row.cases, key=lambda c: -need[c])                          # the largest layer first, then ever smaller ones, both layouts
    assert need[cases[0]] > need[cases[-1]]
    for byte in (0xFF, 0x5A):
        hip._GROWN_WS.clear()
        try:
            with pb.poisoned(byte, grown="real") as p:
                got = {case: _detached(row.run(hip, case)) for case in cases}
                torch.cuda.synchronize()
            p.check_guards()
            sizes = [(r.flat.numel(), r.need) for r in p.workspaces(query)]
            assert max(n for n, _ in sizes) > min(need for _, need in sizes), sizes            # some call did run on a larger buffer
            assert any(n > need for n, need in sizes[1:]), sizes
            for case in cases:
                _same_bits(f"{name} {case} after a larger layer, 0x{byte:02X}", exact[case], got[case])
        finally:
            hip._GROWN_WS.clear()                                              # (views of the poisoned buffers: not for later tests)


# ------------------------------------------------------------------------------------------------------------------ the scan's range status
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_range_status_after_an_out_of_range_call_on_the_same_workspace(hip, dtype):
    """The construction of test_scan_large_values_in_frames_of_more_than_64_tokens: values 2^22 times the usual in frames of 130 tokens leave
    the fp16-pair range and check=True raises; an in-range call on the SAME workspace (poisoned before its first use) must then pass."""
    import numpy as np
    from oracle import gdkvm_oracle as O
    from tests.util import make_scan_inputs
    B, T, N, Hh, Dv = 1, 3, 130, 1, 64
    q, k, v, a, b = make_scan_inputs(B, T, N, Hh, 64, Dv, seed=77, normalized=False, logits=True, corr=0.5)
    if dtype == torch.bfloat16:
        q, k, v = (O.to_bf16_f32(x) for x in (q, k, v))
    v12, v22 = (v * 4096.0).astype(np.float32), (v * 2.0 ** 22).astype(np.float32)
    dev = lambda x, dt=None: pb._cuda(x, dt)
    for byte in pb.PATTERNS:
        with pb.poisoned(byte) as p:
            ws = hip.new_workspace(B, T, Hh, N, 64, Dv, torch.device("cuda", torch.cuda.current_device()))
            hip.scan_fwd(dev(q, dtype), dev(k, dtype), dev(v12, dtype), dev(a), dev(b), flags=3, workspace=ws, check=True)
            with pytest.raises(hip.GdkvmError, match="range"):
                hip.scan_fwd(dev(q, dtype), dev(k, dtype), dev(v22, dtype), dev(a), dev(b), flags=3, workspace=ws, check=True)
            r, s = hip.scan_fwd(dev(q, dtype), dev(k, dtype), dev(v12, dtype), dev(a), dev(b), flags=3, workspace=ws, check=True)
            torch.cuda.synchronize()
        p.check_guards()
        assert torch.isfinite(s).all() and torch.isfinite(r.float()).all()


# ------------------------------------------------------------------------------------------------------------------ the whole paths
def _small_cfg():
    from gdkvm_amd.model import GDKVMConfig
    return GDKVMConfig(widths=(16, 32, 64), pixel_dim=64, value_dim=64)


def test_training_steps_are_the_same_bits_on_poisoned_buffers(hip):
    """Two bf16 train_steps of the small model from one seed, unpatched and with every uninitialised allocation of ops, model, train and
    optim poisoned with NaN bytes: equal losses and parameters (what test_training_step_is_deterministic asserts for two unpatched runs).
    At these widths the 3x3 layers of 16, 32, 48 and 96 input channels are not served by the hand-written kernels (asserted below from
    ops.conv3x3_train_served) and run on the framework's convolution library, whose default weight-gradient kernels add atomically.  Measured
    on an MI355X, two UNPATCHED runs of this test's steps without the flag: equal losses, 8 of 74 gradients different after step 1 (the
    largest by 1.2e-7 of 9.1e-3, decoder.up4.conv.0.weight) and 6 after step 2 (1.5e-5 of 1.1e-2, encoder.stem.0.weight), all of them
    convolution weights of layers that the library runs (the 3 -> 16 stem is one); with the library's deterministic kernels asked for, two unpatched runs agree in every bit, and so must the poisoned one.
    (That the default kernels differ is not asserted: a run in which the atomic adds happen to land in the same order would fail it.)"""
    from gdkvm_amd import model as model_mod, optim, train
    g = torch.Generator().manual_seed(7)
    frames = [torch.rand(2, 3, 3, 64, 64, generator=g).cuda() for _ in range(2)]
    target = [(torch.rand(2, 3, 64, 64, generator=g) > 0.5).long().cuda() for _ in range(2)]

    def run(patched):
        torch.manual_seed(34)
        net = model_mod.GDKVM(_small_cfg()).cuda().train().to(memory_format=torch.channels_last)     # (built outside the block: parameters are
        opt = torch.optim.AdamW(net.parameters(), lr=1e-3)                                           # initialised memory either way)
        ctx = pb.poisoned(0xFF, modules=(model_mod, train, optim)) if patched else None
        if ctx is None:
            losses = [train.train_step(net, opt, frames[i], target[i], torch.bfloat16).item() for i in range(2)]
        else:
            with ctx:
                losses = [train.train_step(net, opt, frames[i], target[i], torch.bfloat16).item() for i in range(2)]
                torch.cuda.synchronize()
            ctx.check_guards()
            assert len(ctx.outputs()) > 50 and len(ctx.workspaces()) > 10
        return losses, {n: q.detach().clone() for n, q in net.named_parameters()}

    probe = model_mod.GDKVM(_small_cfg())
    convs = [m for m in probe.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (3, 3)]
    x = torch.zeros(1, 1, 8, 8, device="cuda", dtype=torch.bfloat16)
    library = [m for m in convs if not hip.conv3x3_train_served(x, m.weight, m.stride, m.padding, m.dilation, m.groups)]
    assert library and all(m.in_channels % 64 or m.out_channels % 64 or m.stride != (1, 1) for m in library), [tuple(m.weight.shape) for m in library]
    before = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        l0, w0 = run(False)
        l1, w1 = run(True)
    finally:
        torch.backends.cudnn.deterministic = before
    assert l0 == l1, (l0, l1)
    diff = {n: (float((w0[n].double() - w1[n].double()).abs().max()), int(torch.isnan(w1[n]).sum())) for n in w0 if not pb.bit_equal(w0[n], w1[n])}
    assert not diff, f"{len(diff)} of {len(w0)} parameters differ (name: largest difference, NaNs): {diff}"


def test_segmentation_is_the_same_bits_on_poisoned_buffers(hip):
    """model.segment on the fused inference build of the small model: masks, Dice counts and the memory state after the last frame (the
    float result every mask follows from: an untrained model may paint one class) bit-equal under every pattern, guards intact."""
    from gdkvm_amd import model as model_mod
    torch.manual_seed(5)
    net = model_mod.GDKVM(_small_cfg()).cuda().eval().to(torch.bfloat16).to(memory_format=torch.channels_last).fuse_for_inference()
    g = torch.Generator().manual_seed(8)
    frames = torch.rand(2, 3, 3, 64, 64, generator=g).cuda().bfloat16()
    target = (torch.rand(2, 3, 64, 64, generator=g) > 0.5).to(torch.uint8).cuda()
    with torch.no_grad():
        base = [t.clone() for t in net.segment(frames, target, return_state=True)]
        assert base[2].abs().max() > 0 and torch.isfinite(base[2]).all()
        for byte in pb.PATTERNS:
            with pb.poisoned(byte, modules=(model_mod,)) as p:
                got = net.segment(frames, target, return_state=True)
                torch.cuda.synchronize()
            p.check_guards()
            assert len(p.outputs()) > 10 and len(p.workspaces()) >= 1
            for what, a, b in zip(("masks", "counts", "state"), got, base):
                assert pb.bit_equal(a, b), f"{what} differ under 0x{byte:02X}: {int((pb.bits(a) != pb.bits(b)).sum())} elements"
