// native_clips.hpp -- what the kernels over RAGGED batches of clips at their own frame size (h0, w0) share (mask_to_native.hip,
// frames_from_native.hip, overlay_native.hip, surface_native.hip, lv_native.hip): clip b holds T frames of h0 w0 bytes and follows clip
// b - 1 in every native buffer.  The sizes (and the spacings) are HOST integers: the launcher validates them, computes every clip's offset and
// hands its clips to the kernels BY VALUE in the kernel arguments, at most X_CLIPS clips per launch and longer batches in several launches --
// as adamw.hip does with its addresses: no table in device memory whose contents a kernel would have to trust, nothing copied, nothing
// allocated.  Here: the bounds, the check of a call's clip table, the walk over a call's launches, and the decode of a work item into
// (clip, frame, band).  A new native-size kernel starts here.  It builds on mask_frame.hpp and, like it, holds no floating-point code, and
// every device helper is __forceinline__ and written with the exact expression the kernels used before they shared it (tools/isa_equal.py).
#pragma once
#include "mask_frame.hpp"

constexpr int NATIVE_MAX_SIDE = 2048;                      // h0, w0 in 1..2048
constexpr int NATIVE_UM_MAX = 4095;                        // ry, rx (micrometres per native pixel) in 1..4095

// ---- host side -------------------------------------------------------------------------------------
// The clip table of a call: clips * T <= 2^30, every (h0, w0), every (ry, rx) of spacing_um when the entry takes one (nullptr: none), and
// native_bytes against the bytes the clips take, which `total` returns.  `what` is the entry's word for its native buffers in the last
// message ("masks", "frames").  GDKVM_OK, or gdkvm_fail(GDKVM_ERR_SHAPE, ...) with the entry's name in front.
inline int native_check_clips(const char* name, const char* what, const int32_t* sizes, const int32_t* spacing_um, size_t native_bytes,
                              int clips, int T, size_t& total)
{
    const size_t frames = (size_t)clips * (size_t)T;
    if (frames > ((size_t)1 << 30)) return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: clips * T = %zu frames exceed 2^30", name, frames);
    total = 0;
    for (int b = 0; b < clips; ++b) {
        const int h0 = sizes[2 * b], w0 = sizes[2 * b + 1];
        if (h0 < 1 || h0 > NATIVE_MAX_SIDE || w0 < 1 || w0 > NATIVE_MAX_SIDE)
            return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: clip %d has the native size %d x %d (h0, w0 in 1..%d)", name, b, h0, w0, NATIVE_MAX_SIDE);
        if (spacing_um) {
            const int ry = spacing_um[2 * b], rx = spacing_um[2 * b + 1];
            if (ry < 1 || ry > NATIVE_UM_MAX || rx < 1 || rx > NATIVE_UM_MAX)
                return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: clip %d has the spacing %d x %d um (ry, rx in 1..%d)", name, b, ry, rx, NATIVE_UM_MAX);
        }
        total += (size_t)T * (size_t)h0 * (size_t)w0;      // (< 2^30 * 2^22)
    }
    if (native_bytes < total)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: the native %s of these sizes take %zu bytes, native_bytes = %zu", name, what, total, native_bytes);
    return GDKVM_OK;
}

// The launches of a call over validated sizes, CLIPS clips at a time.  Per launch: a zeroed Args a with a.maxbands = 1; for its clips
// k = 0 .. nb - 1 in turn, clip(a, k, b, h0, w0, off) -- b = b0 + k the clip of the call, off its first byte, carried from launch to launch --
// fills a.c[k] and the caller's own offsets and returns the clip's bands, which raise a.maxbands; then launch(a, b0, nb) fills the rest and
// launches, returning GDKVM_OK or the failure that ends the walk.
template <class Args, int CLIPS, class Clip, class Launch>
inline int native_launches(const int32_t* sizes, int clips, int T, Clip&& clip, Launch&& launch)
{
    size_t off = 0;
    for (int b0 = 0; b0 < clips; b0 += CLIPS) {
        const int nb = clips - b0 < CLIPS ? clips - b0 : CLIPS;
        Args a{};
        a.maxbands = 1;
        for (int k = 0; k < nb; ++k) {
            const int h0 = sizes[2 * (b0 + k)], w0 = sizes[2 * (b0 + k) + 1];
            const int nbands = clip(a, k, b0 + k, h0, w0, off);
            if (nbands > a.maxbands) a.maxbands = nbands;
            off += (size_t)T * (size_t)h0 * (size_t)w0;
        }
        if (int rc = launch(a, b0, nb)) return rc;
    }
    return GDKVM_OK;
}

// the workgroups of a launch: one per item up to max_wg, more items than that are walked grid-stride
inline dim3 native_grid(long long items, int max_wg) { return dim3((unsigned)(items < max_wg ? items : max_wg)); }

// do the byte ranges [a, a + na) and [b, b + nb) meet?
inline bool native_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    const uint8_t *pa = static_cast<const uint8_t*>(a), *pb = static_cast<const uint8_t*>(b);
    return pa < pb + nb && pb < pa + na;
}

// ---- device side -----------------------------------------------------------------------------------
// Work item -> (clip of the launch, frame, band): the items run over clips x T x maxbands, per_clip = T maxbands, and the grid follows the
// clip with the most bands of the launch, so a workgroup whose band lies past its clip's last leaves at once.  (A kernel whose items also
// carry a direction -- surface_native.hip's columns and rows -- keeps its own decode: through this one its instructions change places.)
struct NativeItem { int clip, t, band; };
__device__ __forceinline__ NativeItem native_item(long long item, long long per_clip, int maxbands)
{
    const int clip = (int)(item / per_clip);
    const long long rem = item - clip * per_clip;
    const int t = (int)(rem / maxbands), band = (int)(rem - (long long)t * maxbands);
    return {clip, t, band};
}
