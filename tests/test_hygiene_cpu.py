"""CPU checks of round 6's host-side rules: pack / graph invalidation is per model and only on real changes, a convolution that leaves the
hand-written path says so (and raises under GDKVM_STRICT=1), the launcher honours the reference guide's CUDA_VISIBLE_DEVICES, the
flat-gradient exchange refuses a parameter without a gradient, stream groups of a captured segment must keep 16-byte output slabs.  And one rule of the kernel sources: the shared device idioms are
written once, in csrc/gdkvm_device.hpp, those of the per-frame mask kernels in csrc/mask_frame.hpp and csrc/mask_labels.hpp, and those of the
kernels over clips at their native size in csrc/native_clips.hpp."""
import glob
import os
import re
import subprocess
import types
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_on_an_eval_model_keeps_graphs_valid_and_epochs_are_per_model():
    from gdkvm_amd import model as M
    a = M.GDKVM(M.GDKVMConfig(widths=(16, 32, 64), pixel_dim=64, value_dim=32)).eval()
    b = M.GDKVM(M.GDKVMConfig(widths=(16, 32, 64), pixel_dim=64, value_dim=32)).eval()
    pa, pb = a._packs, b._packs
    ea, eb, sa = pa.drops, pb.drops, pa.stamp()
    a.eval()                                                     # a defensive eval(): no mode change, nothing invalidated
    assert pa.drops == ea and pa.stamp() == sa
    a.train()
    assert pa.drops == ea + 1 and pa.stamp() != sa               # a real mode change drops the packs ...
    assert pa.epoch == 0                                         # ... and is no weights epoch
    a.eval()
    ka, kb, wa, wb = pa.stamp(), pb.stamp(), pa.epoch, pb.epoch
    M.weights_changed(a)                                         # an optimiser step on `a` ...
    assert pa.stamp() != ka and pa.epoch == wa + 1               # ... moves its stamp, by its weights epoch ...
    assert pb.stamp() == kb and pb.epoch == wb                   # ... and leaves a frozen model `b` (teacher / EMA copy) alone
    assert pb.drops == eb
    M.weights_changed()                                          # the process-wide form tells everyone
    assert pb.stamp() != kb and pb.epoch == wb and pb.drops == eb
    # the sub-modules that cache packs share their model's cache, before and after folding
    assert a.decoder.__dict__["_packs"] is pa
    a.fuse_for_inference()
    convs = [m for m in a.modules() if isinstance(m, M.FusedConv)]
    assert convs and all(m.__dict__["_packs"] is pa for m in convs) and a._packs is pa
    wrapped = types.SimpleNamespace(module=a)                    # DistributedDataParallel-style wrapper
    k2 = pa.stamp()
    M.weights_changed(wrapped)
    assert pa.stamp() != k2


def test_pack_cache_key_rule_drops_and_deep_copy():
    """The pack cache alone (model._Packs) on CPU tensors with a counting builder: what rebuilds a pack, what does not, what a drop reaches,
    what is held for captured graphs, and that a deep copy of a module tree gets one new, empty cache of its own."""
    import copy
    from gdkvm_amd import model as M
    root = torch.nn.Module()
    root.decoder = M.Decoder(64, (16, 32, 64), 2)
    packs = M._Packs()
    packs.adopt(root)
    assert M._packs_of(root.decoder) is packs and "_packs" not in root.state_dict()
    w, w2 = torch.ones(4), torch.ones(3)
    builds = {"a": 0, root.decoder: 0}

    def get(slot, src, extras=("cpu",)):
        def build():
            builds[slot] += 1
            return src * 2.0
        return packs.get(slot, (src,), extras, build)

    v = get("a", w)
    assert get("a", w) is v and builds["a"] == 1                 # same sources: one build
    w.add_(1)                                                    # an in-place write bumps the version counter: rebuilt
    v = get("a", w)
    assert builds["a"] == 2 and torch.equal(v, w * 2.0)
    w.data.mul_(0)                                               # a write through .data is invisible to the key ...
    assert get("a", w) is v and builds["a"] == 2 and not torch.equal(v, w * 2.0)
    M.weights_changed(root)                                      # ... until the model says so
    v = get("a", w)
    assert builds["a"] == 3 and torch.equal(v, w * 2.0)
    assert get("a", w, ("cpu", True)) is not v and builds["a"] == 4      # the caller's extras are part of the key
    v = get("a", w)
    assert builds["a"] == 5
    d = get(root.decoder, w2)                                    # a sub-module's slot is the module itself
    assert builds[root.decoder] == 1 and get(root.decoder, w2) is d
    held = packs.held()
    assert len(held) == 2 and any(h is v for h in held) and any(h is d for h in held)     # exactly the live values
    packs.drop(root.decoder)                                     # a named drop rebuilds that slot only
    assert len(packs.held()) == 1 and packs.held()[0] is v
    get("a", w); d = get(root.decoder, w2)
    assert builds["a"] == 5 and builds[root.decoder] == 2
    stamp = packs.stamp()
    packs.graphs["shape"] = object()
    packs.drop_all()                                             # drop-all: every slot rebuilds, the graphs go, the stamp moves
    assert packs.held() == [] and not packs.graphs and packs.stamp() != stamp
    v = get("a", w); d = get(root.decoder, w2)
    assert builds["a"] == 6 and builds[root.decoder] == 3

    def failing():
        raise RuntimeError("no pack")
    w.add_(1)
    with pytest.raises(RuntimeError, match="no pack"):           # a builder that raises leaves the slot as it was
        packs.get("a", (w,), ("cpu",), failing)
    assert any(h is v for h in packs.held())
    get("a", w)
    assert builds["a"] == 7

    twin = copy.deepcopy(root)                                   # the copy: ONE new cache, shared by its sub-modules, empty
    assert twin._packs is not packs and twin.decoder.__dict__["_packs"] is twin._packs and twin._packs.held() == []
    stamp = packs.stamp()
    M.weights_changed(twin)
    assert packs.stamp() == stamp and twin._packs.epoch == 1
    lone = M.Decoder(64, (16, 32, 64), 2)                        # outside a model: a cache of its own on first use
    assert M._packs_of(lone) is M._packs_of(lone) is not packs


def test_library_fallbacks_are_loud(monkeypatch):
    from gdkvm_amd import model as M
    gpu_like = types.SimpleNamespace(is_cuda=True)
    cpu_like = types.SimpleNamespace(is_cuda=False)
    M._FALLBACKS_SEEN.clear()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        M._library_fallback(cpu_like, "layer", "why")            # the CPU reference module is plain torch by design: silent
        assert not rec
        M._library_fallback(gpu_like, "encoder.layer9.conv", "odd width")
        M._library_fallback(gpu_like, "encoder.layer9.conv", "odd width")    # once per layer and reason
        assert len(rec) == 1 and "encoder.layer9.conv" in str(rec[0].message) and issubclass(rec[0].category, RuntimeWarning)
    monkeypatch.setattr(M, "_STRICT", True)
    with pytest.raises(RuntimeError, match="GDKVM_STRICT"):
        M._library_fallback(gpu_like, "decoder.up4.conv", "fp32 inference")
    M._library_fallback(cpu_like, "decoder.up4.conv", "fp32 inference")      # still silent on the CPU


def test_train_sh_honours_cuda_visible_devices():
    """/root/reference/website/src/pages/[lang]/reprod/index.astro:238 sets CUDA_VISIBLE_DEVICES: 0,1 -- the launcher takes it (HIP_VISIBLE_DEVICES wins)."""
    env = {k: v for k, v in os.environ.items() if k not in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "MASTER_PORT")}
    run = lambda **kw: subprocess.run(["bash", os.path.join(ROOT, "train.sh")], env=dict(env, GDKVM_TRAIN_SH_DRY_RUN="1", **kw),
                                      capture_output=True, text=True, check=True).stdout.strip()
    assert run(CUDA_VISIBLE_DEVICES="0,1") == "HIP_VISIBLE_DEVICES=0,1 NGPU=2 MASTER_PORT=29500"
    assert run(CUDA_VISIBLE_DEVICES="0,1", HIP_VISIBLE_DEVICES="3", MASTER_PORT="29511") == "HIP_VISIBLE_DEVICES=3 NGPU=1 MASTER_PORT=29511"
    assert run() == "HIP_VISIBLE_DEVICES=0 NGPU=1 MASTER_PORT=29500"


def test_flat_grad_sync_refuses_a_parameter_without_gradient():
    import torch.distributed as dist
    from gdkvm_amd.train import FlatGradSync
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29617")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        net = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Linear(4, 2))
        unused = torch.nn.Linear(3, 3)
        net.add_module("unused", unused)
        sync = FlatGradSync(net)
        net[1](net[0](torch.randn(5, 4))).sum().backward()
        with pytest.raises(RuntimeError, match="unused"):
            sync()
        lenient = FlatGradSync(net, allow_unused=True)
        lenient()
        assert unused.weight.grad is not None and float(unused.weight.grad.abs().max()) == 0.0
        lenient.broadcast_buffers()
    finally:
        dist.destroy_process_group()


def test_segment_stream_groups_need_aligned_output_slabs():
    """GraphedSegment(streams=n) hands each group a slice of ONE mask / counts result and the mask kernel wants 16-byte aligned outputs:
    10 clips x 3 frames x 2 classes = 360-byte count slabs per group of 5 -- the automatic choice falls back to one stream, an explicit
    streams=2 says why it cannot be served.  (The check sits in front of anything that needs a device.)"""
    from gdkvm_amd import model as M
    m = M.GDKVM(M.GDKVMConfig(widths=(16, 32, 64), pixel_dim=64, value_dim=32)).eval()
    fake = types.SimpleNamespace(is_cuda=True, shape=(10, 3, 3, 20, 20), device="cuda")
    tgt = object()
    with pytest.raises(ValueError, match="16-byte"):
        M.GraphedSegment(m, fake, tgt, streams=2)


# The kernel sources that build.source_hash() pins (bench.py quotes the committed PMC summaries while they are unchanged) keep their own copies.
_FROZEN = {"gdr_prep.hip", "gdr_scan.hip", "gdr_device.hpp", "gdr_ws.hpp", "gdkvm_common.hpp"}
_RAW_IDIOMS = {
    "bf16 pair pack": r"\(unsigned\)\s*f32_to_bf16\([^;]*\|\s*\(\s*\(unsigned\)\s*f32_to_bf16\([^;]*<<\s*16",
    "bf16 pair unpack": r"__uint_as_float\([^;{}]*?(<<\s*16|&\s*0xffff0000u)\s*\)",
    "LDS-DMA destination cast": r"address_space\(3\)",
    "raw buffer descriptor": r"make_buffer_rsrc",
}
# Sites left as they were because the helper changed the file's gfx950 assembly (tools/isa_equal.py): (file, idiom) -> reason
_RAW_IDIOM_ALLOWED = {
    ("gdr_normalizer.hip", "bf16 pair pack"): "the packed values are quotients computed in the arguments: through pack_bf16x2 both divisions come "
                                              "before both conversions and the schedule changes (76 assembly lines)",
    ("gdr_step.hip", "bf16 pair pack"): "the packed values are products computed in the arguments: same reordering (6 assembly lines)",
    ("kpff.hip", "bf16 pair pack"): "the two bias-add epilogues pack sums computed in the arguments: same reordering (152 assembly lines)",
}


def test_device_idioms_live_in_one_header():
    csrc = os.path.join(ROOT, "gdkvm_amd", "csrc")
    found, local_defs = set(), []
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.hpp"))):
        name = os.path.basename(path)
        with open(path) as f:
            text = f.read()
        if name != "gdkvm_device.hpp" and name not in _FROZEN:
            found |= {(name, idiom) for idiom, rx in _RAW_IDIOMS.items() if re.search(rx, text)}
        if name.endswith(".hip"):
            # static_for_desc (gdr_scan_bwd.hip) counts DOWN: a different function, it stays
            local_defs += [(name, d) for d in re.findall(r"\bvoid\s+(\w*static_for\w*)\s*\(", text) if d != "static_for_desc"]
            local_defs += [(name, d) for d in re.findall(r"\b(\w+_div)\s*\(\s*int\s+n\s*,\s*float\s+inv\s*\)", text)]
    assert not local_defs, f"compile-time loop / reciprocal division defined outside gdkvm_device.hpp: {local_defs}"
    assert found == set(_RAW_IDIOM_ALLOWED), (f"raw idioms outside gdkvm_device.hpp that are not allowed: {sorted(found - set(_RAW_IDIOM_ALLOWED))}; "
                                              f"allowed but gone: {sorted(set(_RAW_IDIOM_ALLOWED) - found)}")
    with open(os.path.join(csrc, "gdkvm_device.hpp")) as f:
        header = f.read()
    assert all(re.search(rx, header) for rx in _RAW_IDIOMS.values())          # the patterns above do match the idioms they name
    assert re.search(r"\bvoid\s+static_for\s*\(", header) and re.search(r"\bidx_div\s*\(\s*int\s+n\s*,\s*float\s+inv\s*\)", header)


# The per-frame kernels over uint8 label masks share their frame plumbing through csrc/mask_frame.hpp, and the two that label connected
# components share the labelling through csrc/mask_labels.hpp, which builds on it.
_MASK_KERNELS = ("lv_measure.hip", "largest_component.hip", "surface_distance.hip", "fill_holes.hip", "signed_distance.hip")
_MASK_IDIOMS = {
    "match16 definition": r"\bmatch16\s*\([^()]*\)\s*\{",
    "wave reduction definition": r"\bwave_(sum|min|max)\w*\s*\([^()]*\)\s*\{",
    "bit walk definition": r"\bvisit\w*\s*\([^()]*\)\s*\{",
    "bit walk": r"&=\s*\w+\s*-\s*1\b",
    "head split": r"\(\s*16u?\s*-[^;]*&\s*15u?\s*\)\s*\)\s*&\s*15u?",
    "shuffle reduction": r"__shfl_xor",
    "atomic word access": r"__hip_atomic_(load|store)",
}
# what mask_labels.hpp holds: the union-find, and the frame rewritten vector by vector (a byte spliced into a 32-bit word of the vector)
_LABEL_IDIOMS = {
    "union-find definition": r"\b\w*(find|unite)\s*\([^()]*\)\s*\{",
    "vector rewrite": r"&\s*~\(\s*0xffu\s*<<\s*\(\s*8\s*\*",
}
# Sites left as they were: (file, idiom) -> reason; where the helper changed the file's gfx950 assembly, with the number of differing lines
_MASK_IDIOM_ALLOWED = {
    ("lv_measure.hip", "shuffle reduction"): "lv_ef_kernel's butterfly carries (volume, frame) pairs, a double compared with an index as the tie-break, "
                                             "beside a count: no integer reduction",
    ("surface_distance.hip", "bit walk"): "surface_bitmap's walk over a bitmap word: through visit_xy its registers are allocated differently "
                                          "(164 assembly lines)",
}


def test_mask_frame_idioms_live_in_one_header():
    csrc = os.path.join(ROOT, "gdkvm_amd", "csrc")
    with open(os.path.join(csrc, "mask_frame.hpp")) as f:
        header = f.read()
    with open(os.path.join(csrc, "mask_labels.hpp")) as f:
        labels = f.read()
    assert '#include "mask_frame.hpp"' in labels
    idioms = {**_MASK_IDIOMS, **_LABEL_IDIOMS}
    found = set()
    for name in _MASK_KERNELS:
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        assert '#include "mask_frame.hpp"' in text or '#include "mask_labels.hpp"' in text
        found |= {(name, idiom) for idiom, rx in idioms.items() if re.search(rx, text)}
    found |= {("mask_labels.hpp", idiom) for idiom, rx in _MASK_IDIOMS.items() if re.search(rx, labels)}     # it builds on the first header
    assert found == set(_MASK_IDIOM_ALLOWED), (f"mask-frame idioms outside mask_frame.hpp / mask_labels.hpp that are not allowed: "
                                               f"{sorted(found - set(_MASK_IDIOM_ALLOWED))}; allowed but gone: {sorted(set(_MASK_IDIOM_ALLOWED) - found)}")
    missing = [idiom for idiom, rx in _MASK_IDIOMS.items() if not re.search(rx, header)]
    missing += [idiom for idiom, rx in _LABEL_IDIOMS.items() if not re.search(rx, labels)]
    assert not missing, f"the patterns do not match the headers' own idioms: {missing}"
    assert all(re.search(r"\b" + d + r"\s*\(", header) for d in ("match16", "wave_sum", "wave_min", "wave_max", "visit_xy", "visit_p"))


# The kernels over ragged batches of clips at their own frame size share the clip table's check, the walk over a call's launches and the
# item decode through csrc/native_clips.hpp, which builds on mask_frame.hpp; that one holds the packed-byte compares temporal_vote.hip shares
# with them.
_NATIVE_KERNELS = ("mask_to_native.hip", "frames_from_native.hip", "overlay_native.hip", "surface_native.hip", "lv_native.hip")
_NATIVE_IDIOMS = {
    "item decode": r"\bitem\s*/\s*per_clip\b[^;]*;[^;]*;[^;]*\brem\s*/",
    "shared helper definition": r"\b\w*(eq80|_overlap|_aligned16)\s*\([^()]*\)\s*\{",
    "native bound": r"\b(h0|w0|ry|rx)\s*>\s*(\d+|[A-Z][A-Z0-9_]*)\b",
    "head split": _MASK_IDIOMS["head split"],
}
# Sites left as they were because the helper changed the file's gfx950 assembly, with the number of differing lines: (file, idiom) ->
# (the number of such sites in the file, reason), so that one more written-out copy in an allowed file fails too
_NATIVE_IDIOM_ALLOWED = {
    ("lv_native.hip", "item decode"): (1, "ln_item is a function that the compiler simplifies on its own before it inlines it: with native_item "
                                          "inside it the file's code moves (338 assembly lines)"),
    ("surface_native.hip", "item decode"): (2, "sn_columns_kernel and sn_rows_kernel decode a direction beside the strip or band: with their three "
                                               "lines replaced by native_item taking per_frame as a long long, tools/isa_equal.py counts 4 assembly "
                                               "lines, one sign extension that changes places in each; sn_surfaces_kernel uses the helper"),
}


def test_native_clip_idioms_live_in_one_header():
    csrc = os.path.join(ROOT, "gdkvm_amd", "csrc")
    with open(os.path.join(csrc, "native_clips.hpp")) as f:
        native = f.read()
    with open(os.path.join(csrc, "mask_frame.hpp")) as f:
        frame = f.read()
    assert '#include "mask_frame.hpp"' in native
    found = {}
    for name in _NATIVE_KERNELS + ("temporal_vote.hip",):
        with open(os.path.join(csrc, name)) as f:
            text = f.read()
        assert ('#include "native_clips.hpp"' if name in _NATIVE_KERNELS else '#include "mask_frame.hpp"') in text
        found.update({(name, idiom): len(re.findall(rx, text)) for idiom, rx in _NATIVE_IDIOMS.items() if re.search(rx, text)})
    allowed = {site: n for site, (n, _) in _NATIVE_IDIOM_ALLOWED.items()}
    assert found == allowed, (f"native-clip idioms outside native_clips.hpp / mask_frame.hpp, (file, idiom): sites -- found {sorted(found.items())}, "
                              f"allowed {sorted(allowed.items())}")
    missing = [idiom for idiom, rx in _NATIVE_IDIOMS.items() if not re.search(rx, native + frame)]
    assert not missing, f"the patterns do not match the headers' own idioms: {missing}"
    assert all(re.search(r"\b" + d + r"\s*\(", native) for d in ("native_check_clips", "native_launches", "native_grid", "native_overlap", "native_item"))
    assert all(re.search(r"\b" + d + r"\s*\(", frame) for d in ("eq80", "head16", "gdkvm_aligned16"))
