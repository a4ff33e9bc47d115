// mask_to_native.hip -- take a clip's label masks from the network's grid [H, W] to the clip's own frame size (h0, w0) and count them against
// the native tracing in the same pass (what eval.py's `native` block is made of).  include/gdkvm.h holds the rule: the half-pixel-centre
// bilinear sampling of F.interpolate(align_corners = False) applied to the one-hot planes of the labels, in exact integers -- the four source
// pixels around a native pixel vote their weights wy wx for their classes, the class with the most votes wins, the smallest class among
// equals, 255 when nothing votes.  out and counts depend on neither the schedule nor the path taken.  No floating-point code in this file.
//
// The native sizes differ from clip to clip, so the native masks are ragged: native_clips.hpp holds the launcher's side of that; a clip's
// entry here is (offset, h0, w0, rows per band, bands), MN_CLIPS of them 1.6 KB of the 4 KB an argument block may have.
//
// A workgroup of 256 lanes owns a BAND of native rows of one (clip, frame): as many whole rows as come nearest above MN_BAND_PIXELS pixels,
// so that a band of a 549 x 778 frame (6 rows) and one of a 2048 x 3 frame (1366 rows) both keep the lanes busy.  The rows of a band follow each
// other in memory, so the band is ONE byte range [s, e) of the frame, and it is cut into runs on the 16-byte grid of the ADDRESSES of out
// (of target without an out): up to 15 head bytes, 16-byte runs, a ragged tail.  Lane l takes the runs l, l + 256, ...; a run is 16
// consecutive native pixels, which may cross from one row into the next.  A full run is stored with one 16-byte store and its target is
// loaded with one 16-byte load when the target's address is aligned too (out and target share every offset, so they are when both
// buffers are); the head, the tail and a misaligned target take byte accesses.  h0 w0 is odd as often as not, so every frame starts at
// another alignment -- the grid is found per band.
//
// Along a run nothing is divided: the run's first pixel costs three integer divisions (p / w0, and the floor divisions of the rule for its
// row and column, whose numerators reach 2^23 -- beyond the 2^16 up to which gdkvm_device.hpp's reciprocal idx_div is exact, which is why it
// is not used here), and from there (x0, fx) and (y0, fy) are CARRIED: a step to the right adds 2 W = qx dx + rx to nx, i.e. x0 += qx,
// fx += rx and one conditional carry, a row wrap does the same for y and restarts x from the constants of column 0.  The two source rows a
// native row needs are two pointers that change at a row wrap only.
//
// A pixel's four source bytes A B / C D are loaded with clamped indices (always inside the source frame, whatever the lane's position --
// a lane past its run's end computes on and its bytes are masked to 0xff), and the winner is found WITHOUT a vote array: a class can only
// win if one of the four bytes names it, so each byte is a candidate with the total t = its own weight + the weights of the bytes equal to
// it, and the key (t << 3) | (7 - class) of a byte < ncls (0 otherwise) orders candidates by votes, then by smaller class: the largest key
// is the answer, 255 when its t is 0.  t <= 4 h0 w0 <= 2^24, so a key fits 28 bits; the weights are below 2^13 and multiply in 24 bits.
// About 80 VALU instructions per pixel whatever ncls -- the kernel's cost, see DESIGN.md for how far that is from the bytes' floor.
//
// The counts are taken on the packed words (four pixels each) as temporal_vote.hip takes them: 0x80 per byte equal to the class, popcounts.
// A lane's 3 ncls counters cover its runs of the band (at most 16 pixels times a handful of runs), two 16-bit fields to a word for the wave
// sums (mask_frame.hpp's wave_sum), the four waves' partials meet in LDS (wg_sum) and lanes 0 .. 3 ncls - 1 add the non-zero ones to counts
// with integer atomics; the launcher zeroed counts with a kernel (gdkvm_zero_async), as temporal_vote's does.  Integer adds commute:
// bit-reproducible.
//
// The grid follows the clip with the most bands of the launch: item = (clip, frame, band) over clips x T x maxbands, and a workgroup whose
// band lies past its clip's last leaves at once.  More than MN_MAX_WG items are taken grid-stride.

#include "native_clips.hpp"

namespace {

constexpr int MN_NT = 256, MN_NW = MN_NT / 64;
constexpr int MN_RUN = GDKVM_MASK_TO_NATIVE_RUN;               // native pixels of a lane's run (gdkvm.h)
constexpr int MN_BAND_PIXELS = GDKVM_MASK_TO_NATIVE_BAND_PIXELS;       // a band is the fewest whole rows with at least this many pixels
constexpr int MN_MAX_WG = GDKVM_MASK_TO_NATIVE_MAX_WG;         // workgroups per launch; more items than that are walked grid-stride
constexpr int MN_CLIPS = GDKVM_MASK_TO_NATIVE_CLIPS;           // clips per launch
static_assert(MN_RUN == 16, "a run is one 16-byte vector");
static_assert(MN_BAND_PIXELS == MN_NT * MN_RUN, "a band gives every lane one run");

struct MnClip {
    unsigned long long off;                                // the clip's first byte in out / target
    int h0, w0, rpb, nbands;                               // native size, rows per band, bands per frame
};
struct MnArgs {
    const uint8_t* mask;                                   // (the launch's first clip)
    const uint8_t* target; uint8_t* out;                   // (the buffers' bases: off is absolute)
    int32_t* counts;                                       // (the launch's first clip)
    long long items;
    int T, H, W, maxbands;
    MnClip c[MN_CLIPS];
};
static_assert(sizeof(MnArgs) <= 2048, "the clip table travels in the kernel arguments");

__device__ __forceinline__ int mn_clamp(int i, int hi) { return i < 0 ? 0 : (i > hi ? hi : i); }

template <int NC>
__global__ __launch_bounds__(MN_NT) void mask_to_native_kernel(MnArgs a)
{
    constexpr int NV = 3 * NC, NP = (NV + 1) / 2;          // a lane's counters, and the words that hold them two by two for the wave sums
    __shared__ unsigned s_sum[MN_NW][NP];
    const int tid = threadIdx.x, H = a.H, W = a.W;
    const bool dice = a.target != nullptr;
    const long long per_clip = (long long)a.T * a.maxbands;
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const auto [clip, t, band] = native_item(item, per_clip, a.maxbands);      // (clip < MN_CLIPS)
        const MnClip c = a.c[clip];
        if (band >= c.nbands) continue;                    // (uniform: a smaller clip of the launch has fewer bands)
        const int h0 = c.h0, w0 = c.w0, row0 = band * c.rpb;
        const int rows = h0 - row0 < c.rpb ? h0 - row0 : c.rpb;
        const int s = row0 * w0, e = s + rows * w0;        // the band's bytes of the frame (e <= h0 w0 <= 2^22)
        const size_t fpos = (size_t)c.off + (size_t)t * (size_t)(h0 * w0);
        const uint8_t* src = a.mask + ((size_t)clip * (size_t)a.T + (size_t)t) * (size_t)(H * W);
        uint8_t* op = a.out ? a.out + fpos : nullptr;
        const uint8_t* tp = dice ? a.target + fpos : nullptr;
        // the 16-byte grid of out's addresses (target's without an out): run 0 is the head, run j >= 1 starts at s + head + 16 (j - 1)
        const uintptr_t ga = reinterpret_cast<uintptr_t>(op ? (const uint8_t*)op : tp) + (uintptr_t)s;
        int head = head16(ga);
        if (head > e - s) head = e - s;
        const int nrun = 1 + (e - s - head + MN_RUN - 1) / MN_RUN;
        // nx(x + 1) = nx(x) + 2 W = nx(x) + qx dx + rx with 0 <= rx < dx, and the same down the rows; column 0 starts from (ix00, fx00)
        const int dy = 2 * h0, dx = 2 * w0;
        const int qy = H / h0, ry = 2 * (H - qy * h0), qx = W / w0, rx = 2 * (W - qx * w0);
        const int nx00 = W - w0;                           // (> -dx: the floor is -1 when negative)
        const int ix00 = nx00 < 0 ? -1 : nx00 / dx, fx00 = nx00 - ix00 * dx;

        int cnt[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) cnt[i] = 0;
        for (int j = tid; j < nrun; j += MN_NT) {
            const int ps = j == 0 ? s : s + head + MN_RUN * (j - 1);
            const int n = j == 0 ? head : (e - ps < MN_RUN ? e - ps : MN_RUN);
            if (n <= 0) continue;                          // (an empty head)
            int y = ps / w0, x = ps - y * w0;
            const int ny = (2 * y + 1) * H - h0, nx = (2 * x + 1) * W - w0;   // (< 2^23, > -d)
            int iy = ny < 0 ? -1 : ny / dy, fy = ny - iy * dy;
            int ix = nx < 0 ? -1 : nx / dx, fx = nx - ix * dx;
            const uint8_t* r0 = src + mn_clamp(iy, H - 1) * W;
            const uint8_t* r1 = src + mn_clamp(iy + 1, H - 1) * W;
            unsigned wy0 = (unsigned)(dy - fy), wy1 = (unsigned)fy;
            // Four pixels to a word, and the words in a loop that is NOT unrolled: unrolled, the compiler issues all 64 byte loads of a run
            // first and keeps their bytes and weights in 185 registers, two waves per SIMD (the 549 x 778 batch measured 475 us that way).
            // The words rotate through ow[0..3], so that every index stays a compile-time one.
            unsigned ow[4] = {0u, 0u, 0u, 0u};
#pragma unroll 1
            for (int w = 0; w < 4; ++w) {
            unsigned word = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = 4 * w + q;
                const int c0 = mn_clamp(ix, W - 1), c1 = mn_clamp(ix + 1, W - 1);
                const unsigned A = r0[c0], B = r0[c1], C = r1[c0], D = r1[c1];
                const unsigned wx0 = (unsigned)(dx - fx), wx1 = (unsigned)fx;
                const unsigned wa = __umul24(wy0, wx0), wb = __umul24(wy0, wx1), wc = __umul24(wy1, wx0), wd = __umul24(wy1, wx1);
                const bool ab = A == B, ac = A == C, ad = A == D, bc = B == C, bd = B == D, cd = C == D;
                const unsigned ta = wa + (ab ? wb : 0u) + (ac ? wc : 0u) + (ad ? wd : 0u);
                const unsigned tb = wb + (ab ? wa : 0u) + (bc ? wc : 0u) + (bd ? wd : 0u);
                const unsigned tc = wc + (ac ? wa : 0u) + (bc ? wb : 0u) + (cd ? wd : 0u);
                const unsigned td = wd + (ad ? wa : 0u) + (bd ? wb : 0u) + (cd ? wc : 0u);
                const unsigned ka = A < (unsigned)NC ? (ta << 3) | (7u - A) : 0u, kb = B < (unsigned)NC ? (tb << 3) | (7u - B) : 0u;
                const unsigned kc = C < (unsigned)NC ? (tc << 3) | (7u - C) : 0u, kd = D < (unsigned)NC ? (td << 3) | (7u - D) : 0u;
                unsigned best = ka > kb ? ka : kb;
                const unsigned b2 = kc > kd ? kc : kd;
                best = best > b2 ? best : b2;
                unsigned res = (best >> 3) ? 7u - (best & 7u) : 0xffu;
                if (k >= n) res = 0xffu;                   // (past the run's end: matches no class, and is not stored)
                word |= res << (8 * q);
                ++x; ix += qx; fx += rx;
                if (fx >= dx) { fx -= dx; ++ix; }
                if (x == w0) {                             // into the next row
                    x = 0; ix = ix00; fx = fx00;
                    iy += qy; fy += ry;
                    if (fy >= dy) { fy -= dy; ++iy; }
                    r0 = src + mn_clamp(iy, H - 1) * W;
                    r1 = src + mn_clamp(iy + 1, H - 1) * W;
                    wy0 = (unsigned)(dy - fy); wy1 = (unsigned)fy;
                }
            }
            ow[0] = ow[1]; ow[1] = ow[2]; ow[2] = ow[3]; ow[3] = word;
            }
            if (op) {
                uint8_t* o = op + ps;
                if (n == MN_RUN && gdkvm_aligned16(o)) {
                    *reinterpret_cast<uint4*>(o) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
                } else {
#pragma unroll
                    for (int k = 0; k < MN_RUN; ++k)
                        if (k < n) o[k] = (uint8_t)(ow[k >> 2] >> (8 * (k & 3)));
                }
            }
            if (dice) {
                const uint8_t* g = tp + ps;
                unsigned tw[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
                if (n == MN_RUN && gdkvm_aligned16(g)) {
                    const uint4 v = *reinterpret_cast<const uint4*>(g);
                    tw[0] = v.x; tw[1] = v.y; tw[2] = v.z; tw[3] = v.w;
                } else {
#pragma unroll
                    for (int k = 0; k < MN_RUN; ++k)
                        if (k < n) tw[k >> 2] = (tw[k >> 2] & ~(0xffu << (8 * (k & 3)))) | ((unsigned)g[k] << (8 * (k & 3)));
                }
#pragma unroll
                for (int cl = 0; cl < NC; ++cl)
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        const unsigned eo = eq80(ow[w], (unsigned)cl), et = eq80(tw[w], (unsigned)cl);
                        cnt[3 * cl + 0] += __builtin_popcount(eo & et);
                        cnt[3 * cl + 1] += __builtin_popcount(eo);
                        cnt[3 * cl + 2] += __builtin_popcount(et);
                    }
            }
        }
        if (dice) {                                        // (uniform)
            // a field holds the wave's sum: a band has fewer than MN_BAND_PIXELS + 2048 pixels, i.e. at most 2 + 6144 / 16 < 2 MN_NT runs, two
            // per lane, so a lane counts at most 32 and a wave at most 2048 < 2^16
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const unsigned pk = (unsigned)cnt[2 * p] | (2 * p + 1 < NV ? (unsigned)cnt[2 * p + 1] << 16 : 0u);
                const unsigned sp = wave_sum(pk);
                if ((tid & 63) == 0) s_sum[tid >> 6][p] = sp;
            }
            __syncthreads();
            if (tid < NV) {
                const int v = (int)((wg_sum(s_sum, tid >> 1) >> (16 * (tid & 1))) & 0xffffu);
                if (v) atomicAdd(a.counts + ((size_t)clip * (size_t)a.T + (size_t)t) * (size_t)NV + tid, v);
            }
            __syncthreads();                               // (the next item parks its sums in the same words)
        }
    }
}

inline bool mn_shape_ok(int clips, int T, int H, int W, int ncls) { return mask_shape_ok(clips, H, W) && T >= 1 && ncls >= 2 && ncls <= 8; }

}  // namespace

// The kernel keeps its state in registers and adds its sums into the zeroed counts: no workspace for any shape.
extern "C" size_t gdkvm_mask_to_native_workspace_bytes(int clips, int T, int H, int W, int ncls)
{
    (void)clips; (void)T; (void)H; (void)W; (void)ncls;
    return 0;
}

extern "C" int gdkvm_mask_to_native(const uint8_t* mask, const int32_t* sizes, const uint8_t* target, uint8_t* out, int32_t* counts,
                                    size_t native_bytes, void* workspace, size_t workspace_bytes, int clips, int T, int H, int W, int ncls,
                                    void* stream)
{
    if (!mn_shape_ok(clips, T, H, W, ncls))
        return gdkvm_fail(GDKVM_ERR_SHAPE, "mask_to_native: bad shape clips=%d T=%d H=%d W=%d ncls=%d (T >= 1, H, W in 1..1024, ncls in 2..8)", clips,
                          T, H, W, ncls);
    if (clips == 0) return GDKVM_OK;
    if (!mask || !sizes) return gdkvm_fail(GDKVM_ERR_SHAPE, "mask_to_native: null pointer (mask and the host sizes are required)");
    if (!out && !target) return gdkvm_fail(GDKVM_ERR_SHAPE, "mask_to_native: neither out nor target: nothing to do");
    if (target && !counts) return gdkvm_fail(GDKVM_ERR_SHAPE, "mask_to_native: counts required with a target");
    if (int rc = mask_check_aligned16("mask_to_native", GDKVM_ERR_SHAPE, "counts", {target ? counts : nullptr})) return rc;
    size_t total;
    if (int rc = native_check_clips("mask_to_native", "masks", sizes, nullptr, native_bytes, clips, T, total)) return rc;
    const size_t frames = (size_t)clips * (size_t)T, src_bytes = frames * (size_t)H * (size_t)W;
    if (out && (native_overlap(out, total, mask, src_bytes) || (target && native_overlap(out, total, target, total))))
        return gdkvm_fail(GDKVM_ERR_SHAPE, "mask_to_native: out must overlap neither mask nor target");
    const size_t need = gdkvm_mask_to_native_workspace_bytes(clips, T, H, W, ncls);
    if (int rc = mask_check_workspace("mask_to_native", H, W, need, workspace, workspace_bytes)) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (target)
        if (int rc = gdkvm_zero_async(counts, frames * (size_t)ncls * 3 * sizeof(int32_t), st)) return rc;
    return native_launches<MnArgs, MN_CLIPS>(sizes, clips, T, [&](MnArgs& a, int k, int, int h0, int w0, size_t off) {
        int rpb = (MN_BAND_PIXELS + w0 - 1) / w0;          // the fewest whole rows with at least MN_BAND_PIXELS pixels
        if (rpb > h0) rpb = h0;
        const int nbands = (h0 + rpb - 1) / rpb;
        a.c[k] = MnClip{(unsigned long long)off, h0, w0, rpb, nbands};
        return nbands;
    }, [&](MnArgs& a, int b0, int nb) -> int {
        a.mask = mask + (size_t)b0 * (size_t)T * (size_t)H * (size_t)W;
        a.target = target; a.out = out;
        a.counts = target ? counts + (size_t)b0 * (size_t)T * (size_t)ncls * 3 : nullptr;
        a.T = T; a.H = H; a.W = W;
        a.items = (long long)nb * (long long)T * (long long)a.maxbands;
        const dim3 grid = native_grid(a.items, MN_MAX_WG);
        switch (ncls) {
            case 2: hipLaunchKernelGGL(mask_to_native_kernel<2>, grid, dim3(MN_NT), 0, st, a); break;
            case 3: hipLaunchKernelGGL(mask_to_native_kernel<3>, grid, dim3(MN_NT), 0, st, a); break;
            case 4: hipLaunchKernelGGL(mask_to_native_kernel<4>, grid, dim3(MN_NT), 0, st, a); break;
            case 5: hipLaunchKernelGGL(mask_to_native_kernel<5>, grid, dim3(MN_NT), 0, st, a); break;
            case 6: hipLaunchKernelGGL(mask_to_native_kernel<6>, grid, dim3(MN_NT), 0, st, a); break;
            case 7: hipLaunchKernelGGL(mask_to_native_kernel<7>, grid, dim3(MN_NT), 0, st, a); break;
            default: hipLaunchKernelGGL(mask_to_native_kernel<8>, grid, dim3(MN_NT), 0, st, a);
        }
        GDKVM_LAUNCH_CHECK("mask_to_native_kernel");
        return GDKVM_OK;
    });
}
