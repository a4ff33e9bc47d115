"""What the five native-size entries answer to bad arguments, in full: per C-level case the return code and the whole gdkvm_last_error()
text, per wrapper-level case the whole str(GdkvmError).  The cases are the ones the test_ops_refusals_without_a_device and
test_entry_refuses_bad_arguments_without_a_device tests of the five native test files enumerate (those check a code and a substring);
tests/golden/native_refusals.json holds collect()'s result as recorded before the entries' shared checks moved into
csrc/native_clips.hpp and ops.py's shared helpers, and tests/test_native_refusals_cpu.py compares.  No device is needed: every case is refused
before the first device call.

`python -m tests.native_refusals > tests/golden/native_refusals.json` records."""
import json
import sys

import numpy as np
import torch

SIZES, SPACING = [(5, 6), (7, 3)], [(300, 200), (100, 100)]
TOTAL = 2 * (30 + 21)


def _label(i, kw):
    return f"{i:02d} " + ",".join(sorted(kw))


def _wrapper(fn, base, cases):
    """{label: message} for fn(**{**base, **kw}) over the cases; a case that is not refused records None"""
    from gdkvm_amd import ops
    out = {}
    for i, kw in enumerate(cases):
        try:
            fn(**{**base, **kw})
            out[_label(i, kw)] = None
        except ops.GdkvmError as e:
            out[_label(i, kw)] = str(e)
    return out


def _entry(lib, call, cases):
    """{label: [code, message]} for call(**kw) over the cases"""
    out = {}
    for i, kw in enumerate(cases):
        rc = call(**kw)
        out[_label(i, kw)] = [rc, lib.gdkvm_last_error().decode() if rc else ""]
    return out


def _aligned(buf):
    return buf.ctypes.data + (-buf.ctypes.data) % 16


def _sz(rows):
    return np.array(rows, np.int32)


def _size_cases():
    meta = torch.ones((2, 2), dtype=torch.int32, device="meta")
    return [dict(sizes=[(5, 6), (0, 3)]), dict(sizes=[(5, 6), (7, 2049)]), dict(sizes=[(5, 6), (7.0, 3)]), dict(sizes=[(5, 6), (7, 3, 1)]),
            dict(sizes=5), dict(sizes=torch.zeros((2, 3), dtype=torch.int32)), dict(sizes=torch.ones((2, 2))), dict(sizes=meta), dict(sizes=None)]


def _spacing_cases():
    return [dict(spacing_um=[(0, 200), (100, 100)]), dict(spacing_um=[(300, 200), (100, 4096)]),
            dict(spacing_um=torch.tensor(SPACING, device="meta")), dict(spacing_um=SPACING[:1]), dict(spacing_um=[(300.0, 200), (100, 100)]),
            dict(spacing_um=7), dict(spacing_um=torch.ones((2, 2))), dict(spacing_um=[(300, 200), (100, 100, 1)]), dict(spacing_um=None)]


def mask_to_native(lib):
    from gdkvm_amd import ops
    m = torch.zeros((2, 2, 4, 4), dtype=torch.uint8)
    g = torch.zeros(TOTAL, dtype=torch.uint8)
    cases = [dict(mask=m.to(torch.int32)), dict(mask=m[0, 0]), dict(mask=torch.zeros((1, 1, 4, 1025), dtype=torch.uint8), sizes=[(4, 4)]),
             dict(num_classes=1), dict(num_classes=9), dict(num_classes=True), dict(mask=torch.zeros((2, 0, 4, 4), dtype=torch.uint8)),
             dict(sizes=[(5, 6)])] + _size_cases() + \
            [dict(want_out=False), dict(target=g[:-1]), dict(target=g.to(torch.int32)), dict(target=g.reshape(2, -1)), dict(out=g[:-1]),
             dict(out=g, target=g.clone(), want_out=False), dict(target=torch.zeros(2 * TOTAL, dtype=torch.uint8)[::2]),
             dict(out=torch.zeros(TOTAL, dtype=torch.uint8, device="meta"))]
    ops_ = _wrapper(ops.mask_to_native, dict(mask=m, sizes=SIZES, num_classes=4), cases)

    mn = np.zeros((2, 2, 4, 4), np.uint8)
    out, tgt = np.zeros(TOTAL + 16, np.uint8), np.zeros(TOTAL + 16, np.uint8)
    cb = np.zeros(2 * 2 * 4 * 3 + 8, np.int32)
    c_al = _aligned(cb)

    def call(mask=mn.ctypes.data, sz=_sz(SIZES), target=tgt.ctypes.data, o=out.ctypes.data, counts=c_al, nb=TOTAL, clips=2, T=2, H=4, W=4, ncls=4):
        return lib.gdkvm_mask_to_native(mask, sz.ctypes.data if sz is not None else None, target, o, counts, nb, None, 0, clips, T, H, W, ncls, None)

    c = _entry(lib, call, [dict(clips=-1), dict(T=0), dict(H=0), dict(W=1025), dict(ncls=1), dict(ncls=9), dict(sz=_sz([[5, 6], [0, 3]])),
                           dict(sz=_sz([[5, 6], [7, 2049]])), dict(mask=None), dict(sz=None), dict(counts=None), dict(counts=c_al + 4),
                           dict(o=None, target=None), dict(nb=TOTAL - 1), dict(o=mn.ctypes.data), dict(o=tgt.ctypes.data + 5), dict(clips=1 << 16, T=1 << 15),
                           dict(clips=0)])
    return {"ops": ops_, "c": c}


def frames_from_native(lib):
    from gdkvm_amd import ops
    flat = torch.zeros(TOTAL, dtype=torch.uint8)
    cases = [dict(flat=flat.to(torch.int32)), dict(flat=flat.reshape(2, -1)), dict(flat=flat[:-1]), dict(T=0), dict(T=True), dict(grid=(4, 1025)),
             dict(grid=(0, 4)), dict(grid=4), dict(grid=(4.0, 4)), dict(channels=0), dict(channels=5), dict(dtype=torch.float16)] + _size_cases() + \
            [dict(out=torch.zeros((2, 2, 3, 4, 4))), dict(out=torch.zeros((2, 2, 3, 4, 5), dtype=torch.uint8)),
             dict(flat=torch.zeros(2 * TOTAL, dtype=torch.uint8)[::2])]
    ops_ = _wrapper(ops.frames_from_native, dict(flat=flat, sizes=SIZES, T=2, grid=(4, 4), channels=3, dtype=torch.uint8), cases)

    nat = np.zeros(TOTAL + 64, np.uint8)
    ob = np.zeros(2 * 2 * 3 * 4 * 4 * 4 + 32, np.uint8)
    o_al = _aligned(ob)

    def call(native=nat.ctypes.data, sz=_sz(SIZES), o=o_al, nb=TOTAL, clips=2, T=2, C=3, H=4, W=4, dt=1):
        return lib.gdkvm_frames_from_native(native, sz.ctypes.data if sz is not None else None, o, nb, None, 0, clips, T, C, H, W, dt, None)

    c = _entry(lib, call, [dict(clips=-1), dict(T=0), dict(H=0), dict(W=1025), dict(C=0), dict(C=5), dict(dt=3), dict(dt=-1),
                           dict(sz=_sz([[5, 6], [0, 3]])), dict(sz=_sz([[5, 6], [7, 2049]])), dict(native=None), dict(sz=None), dict(o=None),
                           dict(o=o_al + 4), dict(nb=TOTAL - 1), dict(o=_aligned(nat)), dict(clips=1 << 16, T=1 << 15), dict(clips=0)])
    return {"ops": ops_, "c": c}


def overlay_native(lib):
    from gdkvm_amd import ops
    g, m = torch.zeros(TOTAL, dtype=torch.uint8), torch.zeros(TOTAL, dtype=torch.uint8)
    shared = torch.zeros(4 * TOTAL, dtype=torch.uint8)
    pal4 = [[1, 2, 3]] * 4
    meta_pal = torch.ones((4, 3), dtype=torch.uint8, device="meta")
    cases = _size_cases() + \
            [dict(palette=meta_pal), dict(reference_palette=meta_pal), dict(width=0), dict(width=4), dict(width=True), dict(alpha=257),
             dict(alpha=-1), dict(alpha=96.0), dict(grey=g[:-1]), dict(mask=m[:-1]), dict(reference=m[:-1]), dict(mask=m.to(torch.int32)),
             dict(out=torch.zeros(3 * TOTAL - 1, dtype=torch.uint8)), dict(palette=pal4[:3]), dict(reference_palette=pal4 + pal4),
             dict(palette=[[1, 2, 3]] * 3 + [[1, 2, 256]]), dict(palette=[[1, 2, 3]] * 3 + [[1, 2]]), dict(palette=torch.ones((4, 3))),
             dict(grey=shared[:TOTAL], out=shared[TOTAL - 1:]), dict(mask=shared[3 * TOTAL:], out=shared[2:3 * TOTAL + 2]),
             dict(reference=shared[3 * TOTAL:], out=shared[1:3 * TOTAL + 1]), dict(num_classes=1), dict(num_classes=9), dict(T=0), dict(T=True),
             dict(grey=None), dict(grey=[0]), dict(mask=shared[::2]), dict(reference=m.reshape(2, -1)),
             dict(mask=torch.zeros(TOTAL, dtype=torch.uint8, device="meta"))]
    ops_ = _wrapper(ops.overlay_native, dict(grey=g, mask=m, sizes=SIZES, T=2, num_classes=4), cases)

    gn, mk, r = np.zeros(TOTAL + 16, np.uint8), np.zeros(TOTAL + 16, np.uint8), np.zeros(TOTAL + 16, np.uint8)
    out = np.zeros(3 * TOTAL + 16, np.uint8)
    pal, rpal = np.zeros((4, 3), np.uint8), np.zeros((4, 3), np.uint8)

    def call(grey=gn.ctypes.data, mask=mk.ctypes.data, ref=r.ctypes.data, sz=_sz(SIZES), p=pal.ctypes.data, rp=rpal.ctypes.data, o=out.ctypes.data,
             nb=TOTAL, clips=2, T=2, ncls=4, width=2, alpha=96):
        return lib.gdkvm_overlay_native(grey, mask, ref, sz.ctypes.data if sz is not None else None, p, rp, o, nb, None, 0, clips, T, ncls,
                                        width, alpha, None)

    c = _entry(lib, call, [dict(clips=-1), dict(T=0), dict(ncls=1), dict(ncls=9), dict(width=0), dict(width=4), dict(alpha=-1), dict(alpha=257),
                           dict(sz=_sz([[5, 6], [0, 3]])), dict(sz=_sz([[5, 6], [7, 2049]])), dict(grey=None), dict(mask=None), dict(sz=None),
                           dict(p=None), dict(o=None), dict(rp=None), dict(nb=TOTAL - 1), dict(o=gn.ctypes.data), dict(o=mk.ctypes.data + 5),
                           dict(o=r.ctypes.data - 3 * TOTAL + 1), dict(grey=out.ctypes.data + 3 * TOTAL - 1), dict(clips=1 << 16, T=1 << 15),
                           dict(clips=0), dict(clips=0, grey=None, mask=None, sz=None, p=None, o=None)])
    return {"ops": ops_, "c": c}


def surface_distance_native(lib):
    from gdkvm_amd import ops
    m = torch.zeros(TOTAL, dtype=torch.uint8)
    cases = [dict(sizes=[(0, 6), (7, 3)])] + _size_cases() + _spacing_cases() + \
            [dict(target=m[:-1]), dict(mask=m.to(torch.int32)), dict(target=m.reshape(2, -1)), dict(cls=255), dict(cls=-1), dict(cls=True),
             dict(T=0), dict(T=2.0), dict(mask=None), dict(target=torch.zeros(2 * TOTAL, dtype=torch.uint8)[::2]),
             dict(target=torch.zeros(TOTAL, dtype=torch.uint8, device="meta")), dict(sizes=SIZES[:1]), dict(target=None)]
    ops_ = _wrapper(ops.surface_distance_native, dict(mask=m, target=m, sizes=SIZES, T=2, spacing_um=SPACING), cases)

    rows = 2 * (5 + 7)
    mk, t = np.zeros(TOTAL, np.uint8), np.zeros(TOTAL, np.uint8)
    need = lib.gdkvm_surface_distance_native_workspace_bytes(2, 2, TOTAL, rows)
    wb = np.zeros(need + 32, np.uint8)
    w_al = _aligned(wb)
    sb = np.zeros(4 * 8 + 4, np.int64)
    s_al = _aligned(sb)

    def call(mask=mk.ctypes.data, target=t.ctypes.data, sz=_sz(SIZES), spc=_sz(SPACING), surf=s_al, nb=TOTAL, ws=w_al, wsb=need, clips=2, T=2, cls=1):
        return lib.gdkvm_surface_distance_native(mask, target, sz.ctypes.data if sz is not None else None,
                                                 spc.ctypes.data if spc is not None else None, surf, nb, ws, wsb, clips, T, cls, None)

    c = _entry(lib, call, [dict(clips=-1), dict(T=0), dict(cls=255), dict(cls=-1), dict(sz=_sz([[5, 6], [0, 3]])), dict(sz=_sz([[2049, 6], [7, 3]])),
                           dict(spc=_sz([[0, 200], [100, 100]])), dict(spc=_sz([[300, 200], [100, 4096]])), dict(mask=None), dict(target=None),
                           dict(sz=None), dict(spc=None), dict(surf=None), dict(surf=s_al + 8), dict(nb=TOTAL - 1), dict(ws=None),
                           dict(wsb=need - 1), dict(ws=w_al + 4), dict(clips=1 << 16, T=1 << 15),
                           dict(sz=_sz([[5, 6], [0, 3]]), spc=_sz([[0, 200], [100, 100]])),      # clip 0's spacing is met before clip 1's size
                           dict(clips=0), dict(clips=0, mask=None, ws=None, wsb=0)])
    return {"ops": ops_, "c": c, "workspace_bytes": need}


def lv_measure_native(lib):
    from gdkvm_amd import ops
    m = torch.zeros(TOTAL, dtype=torch.uint8)
    cases = [dict(sizes=[(0, 6), (7, 3)])] + _size_cases() + _spacing_cases() + \
            [dict(mask=m[:-1]), dict(mask=m.to(torch.int32)), dict(mask=m.reshape(2, -1)), dict(cls=255), dict(cls=-1), dict(cls=True),
             dict(disks=0), dict(disks=65), dict(disks=True), dict(disks=2.0), dict(T=0), dict(mask=None),
             dict(mask=torch.zeros(2 * TOTAL, dtype=torch.uint8)[::2]), dict(sizes=SIZES[:1])]
    ops_ = _wrapper(ops.lv_measure_native, dict(mask=m, sizes=SIZES, T=2, spacing_um=SPACING), cases)

    sizes = _sz([[5, 6], [70, 3]])
    total, nbands, D = 2 * (30 + 210), 2 * (1 + 3), 20
    mk = np.zeros(total, np.uint8)
    bufs = [np.zeros(n + 2, np.int64) for n in (4 * 12, 4 * D, 4 * 6, nbands * (8 + D))]
    st, dk, ge, bd = (_aligned(b) for b in bufs)

    def call(mask=mk.ctypes.data, sz=sizes, spc=_sz(SPACING), stats=st, disks=dk, geom=ge, bands=bd, nb=total, nbd=nbands, clips=2, T=2, cls=1, D=D):
        return lib.gdkvm_lv_measure_native(mask, sz.ctypes.data if sz is not None else None, spc.ctypes.data if spc is not None else None,
                                           stats, disks, geom, bands, nb, nbd, clips, T, cls, D, None)

    c = _entry(lib, call, [dict(clips=-1), dict(T=0), dict(D=0), dict(D=65), dict(sz=_sz([[5, 6], [0, 3]])), dict(sz=_sz([[2049, 6], [70, 3]])),
                           dict(spc=_sz([[0, 200], [100, 100]])), dict(spc=_sz([[300, 200], [100, 4096]])), dict(nb=total - 1), dict(nbd=nbands - 1),
                           dict(nbd=nbands + 1), dict(nbd=-1), dict(clips=1 << 16, T=1 << 15), dict(cls=255), dict(cls=-1), dict(mask=None),
                           dict(sz=None), dict(spc=None), dict(stats=None), dict(disks=None), dict(geom=None), dict(bands=None), dict(stats=st + 8),
                           dict(disks=dk + 8), dict(geom=ge + 8), dict(bands=bd + 8),
                           dict(sz=_sz([[5, 6], [0, 3]]), spc=_sz([[0, 200], [100, 100]])),      # clip 0's spacing is met before clip 1's size
                           dict(nb=total - 1, nbd=nbands - 1), dict(clips=0), dict(clips=0, mask=None, bands=None, nbd=0)])
    return {"ops": ops_, "c": c}


def views():
    """native_frames, native_rgb_frames, pack_native and native_spacing_frames: the helpers beside the five entries"""
    from gdkvm_amd import ops
    g = torch.zeros(TOTAL, dtype=torch.uint8)
    rgb = torch.zeros(3 * TOTAL, dtype=torch.uint8)
    frames = [dict(b=2), dict(flat=g[:-1]), dict(T=0), dict(T=True), dict(b=-1), dict(b=True), dict(flat=None), dict(flat=g.reshape(2, -1)),
              dict(sizes=[(5, 6), (0, 3)]), dict(sizes=5)]
    rgbs = [dict(b=2), dict(flat=rgb[:-1]), dict(T=0), dict(T=2.0), dict(b=-1), dict(flat=None), dict(flat=rgb.reshape(2, -1)),
            dict(sizes=[(5, 6), (7, 2049)])]
    z = lambda *s: torch.zeros(s, dtype=torch.uint8)
    return {"native_frames": _wrapper(ops.native_frames, dict(flat=g, sizes=SIZES, T=2, b=0), frames),
            "native_rgb_frames": _wrapper(ops.native_rgb_frames, dict(flat=rgb, sizes=SIZES, T=2, b=0), rgbs),
            "pack_native": _wrapper(ops.pack_native, {}, [dict(clips=[z(2, 3, 3), z(3, 3, 3)]), dict(clips=[]), dict(clips=[z(2, 3, 3), z(2, 3, 2049)]),
                                                          dict(clips=[z(2, 3, 3).float()])]),
            "native_spacing_frames": _wrapper(ops.native_spacing_frames, dict(spacing_um=SPACING, T=2, device="cpu"),
                                              [dict(T=0), dict(T=True)] + _spacing_cases()[:3] + _spacing_cases()[4:])}


def collect() -> dict:
    from gdkvm_amd import ops
    lib = ops.load()
    out = {f.__name__: f(lib) for f in (mask_to_native, frames_from_native, overlay_native, surface_distance_native, lv_measure_native)}
    out["views"] = views()
    return out


if __name__ == "__main__":
    json.dump(collect(), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
