"""tests/poisoned_buffers.py without a GPU: the torch proxy on CPU tensors, every detector on a stand-in "kernel" made of plain tensor writes,
and the census -- every size query include/gdkvm.h declares, and every _workspace( / _grown_workspace( call site of the package, has a row
in ENTRIES."""
import pytest
import torch

from gdkvm_amd import ops
from tests import poisoned_buffers as pb

DTYPES = (torch.float32, torch.bfloat16, torch.uint8, torch.int32, torch.int64)
CL = torch.channels_last


# ------------------------------------------------------------------------------------------------------------------ the proxy
@pytest.mark.parametrize("byte", pb.PATTERNS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d)[6:])
def test_every_io_dtype_comes_back_filled_with_the_pattern(byte, dtype):
    with pb.poisoned(byte) as p:
        t = ops.torch.empty((3, 5), dtype=dtype)
        assert t.dtype == dtype and tuple(t.shape) == (3, 5) and t.is_contiguous() and t.data_ptr() % 16 == 0
        assert bool(p.unwritten(t).all())
        assert bool((t.contiguous().view(torch.uint8) == byte).all())
        p.check_guards()
    assert pb.pattern_value(0xFF, 4) == -1 and pb.pattern_value(0xFF, 1) == 255 and pb.pattern_value(0x5A, 1) == 90
    if byte == 0xFF and dtype.is_floating_point:
        assert bool(torch.isnan(t).all())
    if byte == 0x5A and dtype.is_floating_point:
        assert bool(torch.isfinite(t).all()) and 1e16 < float(t.float().max()) < 2e16


def test_shape_strides_and_memory_format_agree_with_the_real_call():
    src = torch.zeros(2, 8, 3, 5).contiguous(memory_format=CL)
    param = torch.zeros(6, 4, 3, 3).contiguous(memory_format=CL)
    sliced = torch.zeros(4, 6)[:, ::2]
    with pb.poisoned(0x5A) as p:
        T = ops.torch
        pairs = [
            (T.empty((2, 8, 3, 5)), torch.empty((2, 8, 3, 5))),
            (T.empty((2, 8, 3, 5), dtype=torch.bfloat16, memory_format=CL), torch.empty((2, 8, 3, 5), dtype=torch.bfloat16, memory_format=CL)),
            (T.empty_like(src), torch.empty_like(src)),                                                  # preserve_format: stays channels_last
            (T.empty_like(src, dtype=torch.float32, memory_format=torch.contiguous_format),
             torch.empty_like(src, dtype=torch.float32, memory_format=torch.contiguous_format)),
            (T.empty_like(sliced), torch.empty_like(sliced)),
            (T.empty_strided(tuple(param.shape), tuple(param.stride()), dtype=torch.float32),
             torch.empty_strided(tuple(param.shape), tuple(param.stride()), dtype=torch.float32)),
            (T.empty_strided((3, 4), (8, 2), dtype=torch.int32), torch.empty_strided((3, 4), (8, 2), dtype=torch.int32)),   # gaps
            (T.empty(7, dtype=torch.uint8), torch.empty(7, dtype=torch.uint8)),
        ]
        for got, real in pairs:
            assert got.shape == real.shape and got.stride() == real.stride() and got.dtype == real.dtype and got.device == real.device
            assert got.is_contiguous() == real.is_contiguous() and got.is_contiguous(memory_format=CL) == real.is_contiguous(memory_format=CL)
            assert got.data_ptr() % 16 == 0 and bool(p.unwritten(got).all())
            got.zero_()                                                    # the whole payload is the tensor's: no guard byte moves
        assert pairs[2][0].is_contiguous(memory_format=CL) and pairs[5][0].is_contiguous(memory_format=CL)
        p.check_guards()
        assert len(p.outputs()) == len(pairs) and all(r.name.startswith("test_poisoned_buffers_cpu.py:") for r in p.outputs())
        empty = T.empty((0, 4))                                            # zero elements: passed through, not recorded
        assert empty.numel() == 0 and len(p.outputs()) == len(pairs)
        assert T.zeros(3).sum() == 0 and T.Tensor is torch.Tensor and T.float32 is torch.float32       # everything else is torch's own


def test_the_real_names_are_back_after_the_block_also_when_it_raises():
    from gdkvm_amd import model, optim, train
    mods = (model, train, optim)
    real = (ops._workspace, ops._grown_workspace, ops._call)
    global_names = (torch.empty, torch.empty_like, torch.empty_strided)
    with pb.poisoned(0xFF, modules=mods):
        assert all(m.torch is not torch for m in (ops,) + mods) and ops._workspace is not real[0] and ops._call is not real[2]
        assert (torch.empty, torch.empty_like, torch.empty_strided) == global_names              # the global module is never patched
    assert all(m.torch is torch for m in (ops,) + mods) and (ops._workspace, ops._grown_workspace, ops._call) == real
    with pytest.raises(ZeroDivisionError):
        with pb.poisoned(0x00, modules=mods):
            1 / 0
    assert all(m.torch is torch for m in (ops,) + mods) and (ops._workspace, ops._grown_workspace, ops._call) == real
    with pytest.raises(RuntimeError, match="already patched"):
        with pb.poisoned(0xFF):
            with pb.poisoned(0x5A):
                pass
    assert ops.torch is torch


# ------------------------------------------------------------------------------------------------------------------ the detectors
QUERY = "gdkvm_bn_workspace_bytes"


@pytest.fixture
def cpu_sizes(monkeypatch):
    """The size query answered without the library: 64 bytes for the stand-in's entry."""
    monkeypatch.setattr(ops, "_bytes", lambda name, dev, *dims: {QUERY: 64, "zero": 0}[name])


def _stand_in(slip=None):
    """A "kernel" of plain tensor writes through the patched names: out [4, 6] fp32 = 2 x, with partial sums staged in a 64-byte workspace
    of which it uses the first 8 words.  `slip` plants one defect."""
    x = torch.arange(24, dtype=torch.float32).reshape(4, 6)
    out = ops.torch.empty((4, 6), dtype=torch.float32)
    ws = ops._workspace(QUERY, None, 4, floor=16)
    words = ws.view(torch.float32)
    words[:8] = 1.0
    rows = 3 if slip == "tail" else 4
    out[:rows] = 2 * x[:rows]
    if slip == "past_output":
        out.as_strided((1,), (1,), out.storage_offset() + out.numel())[0] = 7.0
    if slip == "past_workspace":
        ws.as_strided((1,), (1,), ws.storage_offset() + ws.numel())[0] = 1
    out[0, 0] += float(words[:9 if slip == "stale_read" else 8].sum()) - 8.0
    return out


def _patterns(slip):
    res = {}
    for byte in pb.PATTERNS:
        with pb.poisoned(byte) as p:
            out = _stand_in(slip)
            res[byte] = (p, out)
    return res


def test_a_correct_stand_in_passes_every_check(cpu_sizes):
    res = _patterns(None)
    for byte, (p, out) in res.items():
        p.check_guards()
        assert byte == 0x00 or not p.unwritten(out).any()
        assert pb.bit_equal(out, res[0x00][1])
        (ws,) = p.workspaces(QUERY)
        assert ws.need == 64 and ws.query == 64 and ws.tensor.numel() == 64 and ws.tensor.data_ptr() % 16 == 0


def test_an_unwritten_last_row_is_reported_by_unwritten(cpu_sizes):
    for byte in (0xFF, 0x5A):
        p, out = _patterns("tail")[byte]
        mask = p.unwritten(out)
        assert mask[3].all() and not mask[:3].any()
        p.check_guards()


def test_a_store_past_the_output_is_reported_by_the_guards(cpu_sizes):
    p, _ = _patterns("past_output")[0xFF]
    with pytest.raises(AssertionError, match=r"output test_poisoned_buffers_cpu.py:\d+ _stand_in .*after it.*offset 0 from the payload's end"):
        p.check_guards()


def test_a_byte_past_the_workspace_is_reported_by_the_guards(cpu_sizes):
    p, _ = _patterns("past_workspace")[0x5A]
    with pytest.raises(AssertionError, match=f"workspace {QUERY} .*1 guard byte.*after it"):
        p.check_guards()


def test_a_read_of_a_never_written_workspace_word_shows_between_the_patterns(cpu_sizes):
    res = _patterns("stale_read")
    outs = {b: o for b, (p, o) in res.items()}
    assert not pb.bit_equal(outs[0x00], outs[0x5A]) and not pb.bit_equal(outs[0x00], outs[0xFF])
    assert torch.isnan(outs[0xFF][0, 0]) and pb.bit_equal(outs[0xFF][1:], outs[0x00][1:])
    for p, _ in res.values():
        p.check_guards()


def test_short_and_zero_size_workspaces(cpu_sizes):
    with pb.poisoned(0xFF, short=QUERY) as p:
        ws = ops._workspace(QUERY, None, 4, floor=16)
        assert ws.numel() == 48 and p.workspaces(QUERY)[0].need == 64                # 16 bytes short, still inside the 64-byte payload
        ws[:] = 0
        p.check_guards()                                                             # the cut-off tail belongs to the payload, not the guard
        assert not p.payload_intact(p.workspaces(QUERY)[0])
        floor = ops._workspace("zero", None, floor=16)
        none = ops._workspace("zero", None)
        assert floor.numel() == 16 and none.numel() == 0 and none.data_ptr() == 0
        assert p.payload_intact(p.workspaces("zero")[0])
    with pb.poisoned(0x5A) as p:                                                     # grown="exact": exactly max(16, query), no growth
        assert ops._grown_workspace(QUERY, None, 4).numel() == 64 and ops._grown_workspace("zero", None).numel() == 16


# ------------------------------------------------------------------------------------------------------------------ the census
def test_every_declared_size_query_has_a_row():
    declared = pb.declared_queries()
    assert len(declared) >= 27 and len(set(declared)) == len(declared)
    assert set(declared) == {n for n in ops.SIGNATURES if n.endswith("_workspace_bytes")}          # (the bindings list the same ones)
    missing = sorted(set(declared) - pb.covered_queries())
    assert not missing, f"size queries without a row in tests/poisoned_buffers.py ENTRIES: {missing}"
    assert not sorted(pb.covered_queries() - set(declared))
    assert set(pb.ZERO_SIZE) <= set(declared)


def test_every_workspace_call_site_names_a_query_that_has_a_row():
    named = pb.named_queries()
    assert len(named) >= 27 and sum(map(len, named.values())) >= 30
    unknown = {n: sites for n, sites in named.items() if n not in pb.covered_queries()}
    assert not unknown, f"_workspace( / _grown_workspace( call sites whose query has no row in ENTRIES: {unknown}"
    assert set(named) == set(pb.declared_queries())                                   # no query is declared and never asked by a wrapper


def test_no_other_allocator_escapes_the_proxy():
    """The three patched names are the only uninitialised allocators the product modules use: a Tensor.new_empty would pass the proxy by."""
    import os
    import re
    pkg = os.path.join(pb.ROOT, "gdkvm_amd")
    for fn in ("ops.py", "model.py", "train.py", "optim.py"):
        src = open(os.path.join(pkg, fn)).read()
        assert not re.search(r"\.new_empty(_strided)?\(|from torch import|torch\.Tensor\.new_", src), fn
        assert re.search(r"^import torch$", src, re.M), fn


def test_rows_are_well_formed():
    from tests.test_train_side_gpu import STRIDED_WINDOW_CASES
    names = [r.name for r in pb.ENTRIES]
    assert len(set(names)) == len(names) and pb.STRIDED_CASES == STRIDED_WINDOW_CASES
    assert all(set(qs) <= set(pb.row(n).queries) for n, qs in pb.FLOOR_QUERIES.items())
    for r in pb.ENTRIES:
        assert r.cases and len(r.ids) == len(set(r.ids)) == len(r.cases), r.name
        assert callable(r.run) and callable(r.check) and r.reference and r.queries, r.name
