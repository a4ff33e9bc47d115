"""CPU-side checks of the drop-in boundary: the library loads and exports every symbol include/gdkvm.h
declares, and the host wrappers refuse to run without a device (no fallback path)."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "gdkvm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(gdkvm_[a-z_0-9]+)\s*\(", src)))


def test_header_symbols_all_exported_and_bound():
    from gdkvm_amd import build, ops
    build.build()
    lib = ops.load()
    declared = _declared_symbols()
    assert declared, "no symbols parsed from include/gdkvm.h"
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in gdkvm.h but not exported"
        assert name in ops.SIGNATURES, f"{name} has no ctypes signature in gdkvm_amd/ops.py"
    assert lib.gdkvm_abi_version() == 1
    assert lib.gdkvm_scan_workspace_bytes(16, 32, 1, 49, 64, 256) == (16 * 32 * (64 * (6 * 64 + 256 + 1 + 16) + 64 * 96 + 64 * (64 + 32 + 256) + 256 // 4) + 16 * 16) * 4 + 1024 + 1024      # (+ gmax per frame and slice, + 2^e per clip and slice)


def test_no_cpu_fallback():
    from gdkvm_amd import ops
    x = torch.zeros(1, 1, 4, 1, 64)
    with pytest.raises(ops.GdkvmError, match="device"):
        ops.scan_fwd(x, x, torch.zeros(1, 1, 4, 1, 16), torch.zeros(1, 1, 1), torch.zeros(1, 1, 4, 1))
    with pytest.raises(ops.GdkvmError, match="device"):
        ops.argmax_dice(torch.zeros(1, 2, 4, 4))


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under gdkvm_amd/ may reference it."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "gdkvm_amd")):
        for fn in files:
            if fn.endswith((".py", ".hip", ".hpp", ".h", ".cpp")):
                txt = open(os.path.join(dirpath, fn)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f"{fn} imports oracle"
                assert "gdkvm_oracle" not in txt, f"{fn} references the oracle"


def test_host_side_of_the_library_is_clean_under_sanitizers():
    """The HOST halves of the HIP library -- workspace carving (csrc/gdr_ws.hpp), the segmented scan's and the normalizer's own carves, argument
    checks and error reporting of gdr_segmented / gdr_normalizer / gdr_step / gdkvm_api -- built with -fsanitize=address,undefined on the CPU
    (tests/host_san/: device code compiled as usual and never run; the kernel-heavy entry points they call are stubbed) and driven with
    workspaces malloc'ed at EXACTLY the size the library asks for, every carved region written end to end: a carve that outgrows its own size
    request is a heap-buffer-overflow report, not a silent overwrite on the GPU box.  Also pins the error codes of ~25 bad-argument calls."""
    import subprocess
    here = os.path.join(ROOT, "tests", "host_san")
    subprocess.check_call(["bash", os.path.join(here, "build.sh")], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    out = subprocess.run([os.path.join(here, "_build", "host_san")], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1"))
    assert out.returncode == 0 and "host_san: ok" in out.stdout, out.stdout + out.stderr


_HELPERS = ("load", "_check", "_call", "_bytes")        # the only functions of ops.py that touch the library or the current device
# entry points that launch but have no torch wrapper (reached from C, or from callers of the C ABI only), with the reason
_C_ONLY = {"gdkvm_scan_prep_normed": "stage 1 of gdkvm_scan_fwd_normed; the split prep / apply pipeline of ops.py does not take norms"}


def test_one_call_path_for_every_entry_point():
    """ops.py reaches the library through ONE launch helper and ONE size-query helper: the marshalling of their arguments (pure, checked here on
    CPU tensors), the names the wrappers pass (each a bound symbol; every launching symbol passed somewhere) and the absence of hand-written
    launches outside the helpers."""
    import ast
    import ctypes
    from gdkvm_amd import ops
    t, w32, w8 = torch.zeros(5), torch.zeros(3, dtype=torch.float32), torch.zeros(7, dtype=torch.uint8)
    assert ops._c_args((t, None, torch.empty(0), 3, 2.5)) == [t.data_ptr(), None, None, 3, 2.5]
    assert ops._c_args((ops._Ws(w32), ops._Ws(w8), ops._Ws(None))) == [w32.data_ptr(), 12, w8.data_ptr(), 7, None, 0]
    passed = ops._c_args((7, 0.5))
    assert type(passed[0]) is int and type(passed[1]) is float

    path = os.path.join(ROOT, "gdkvm_amd", "ops.py")
    src = open(path).read()
    tree = ast.parse(src)
    skip = set()                                            # string nodes that are not names handed to a helper: SIGNATURES' keys and docstrings
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and any(isinstance(x, ast.Name) and x.id == "SIGNATURES" for x in node.targets):
            skip.update(id(k) for k in node.value.keys)
        if isinstance(node, (ast.Module, ast.FunctionDef, ast.ClassDef)) and ast.get_docstring(node, clean=False) is not None:
            skip.add(id(node.body[0].value))
    literals = {n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str) and id(n) not in skip
                and re.fullmatch(r"gdkvm_[a-z_0-9]+", n.value)}
    assert literals, "no entry-point names found in ops.py"
    for name in sorted(literals):
        assert name in ops.SIGNATURES, f"ops.py passes {name!r}, which has no signature"
    launching = {n for n, (res, args) in ops.SIGNATURES.items() if res is ctypes.c_int and args and args[-1] is ctypes.c_void_p}
    assert launching - literals == set(_C_ONLY), sorted((launching - literals) ^ set(_C_ONLY))

    outside = src
    for node in tree.body:                                  # blank the helpers out, then look at everything else
        if isinstance(node, ast.FunctionDef) and node.name in _HELPERS:
            outside = outside.replace(ast.get_source_segment(src, node), "")
    assert not re.search(r"\.gdkvm_[a-z_0-9]+\s*\(", outside), "a hand-written library call outside the helpers"
    assert "torch.cuda.device(" not in outside, "a hand-made device context outside the helpers"
