// fill_holes.hip -- fill the holes of one class of label masks on the device (the second clean-up in front of lv_measure, behind
// largest_component.hip: pixels inside the cavity that argmax gave to another class cost the method of disks about twice their pixel share).
// include/gdkvm.h holds the definition; the filled mask and the eight integers depend on neither the algorithm nor the schedule.
//
// ONE workgroup per frame (512 lanes in the LDS form -- 60 KiB of labels allow two workgroups per CU whatever their size, and on 512 frames
// of 112 x 112 the kernel measured 128 us with 256 lanes, 90 us with 512 and 123 us with 1024, of which 784 have a vector; 1024 in the
// workspace form, whose chains of dependent L2 loads want more waves in flight): no cross-workgroup synchronisation, no fences between workgroups, no flag anybody spins on.  The set that is labelled is the
// COMPLEMENT Q of the class (MaskFrame::sweep_not_*), typically 85-90 % of a frame.  A frame's labels are one 32-bit word per pixel, in LDS
// while the frame has at most FH_LDS_PIX pixels (60 KiB of the workgroup's 64 KiB; the 112 x 112 mask of cfg2 takes 49 KiB), otherwise in the
// frame's slice of the caller's workspace, where every access is an agent-scope relaxed atomic (served by L2).  Passes, a workgroup barrier
// between them:
//   1. n = |P|, hit_before and n_target.  P empty, P the whole frame, H <= 2 or W <= 2: no hole is possible, straight to the copy.
//   2. every word = NONE (the word of a pixel of the class).
//   3. L[p] = the first pixel of p's horizontal run of Q inside the lane's 16-byte vector (most of the complement's links cost nothing).
//   4. union-find as in largest_component.hip: unite(p, q) for the backward neighbours q of p that are not already joined through p's left
//      neighbour; the larger root is linked under the smaller with atomicMin.  A spiral corridor costs no sweeps: there is no sweep.
//   5. flatten: L[p] = root(p); a root's own word becomes ROOT | 0.
//   6. L[root] += 1 per pixel (run- and wave-combined) and L[root] |= OUT for a pixel on the frame's border.  Sums and ORs commute, and the
//      count (bits 0..20, at most 2^20) never reaches the flags: a root's word does not depend on the order in which lanes arrive.
//   7. the roots without OUT are the holes: their number, the largest, and FILL into the word of each that max_area lets through.
//   8. out: a pixel of Q becomes cls when its root's word has FILL; what the filled pixels were in the target.
// Loop bounds: as in largest_component.hip -- a chain p > L[p] > L[L[p]] ... strictly descends through pixel indices, so find() ends within H*W
// steps; in unite() the larger of the two roots strictly descends from one retry to the next, so it ends within H*W retries.  Both loops
// count to H*W and, should that ever be reached, raise the frame's failure flag: holes = -1 and out = mask, rather than spinning.  Every
// other loop walks the lane's share of the H*W pixels once, or the at most 16 bits of a match word.

#include "mask_frame.hpp"

namespace {

constexpr unsigned FH_NONE = 0xffffffffu;      // the word of a pixel of the class (not of Q)
constexpr unsigned FH_ROOT = 0x80000000u;      // from pass 5 on: this pixel is its component's smallest index; bits 0..20 count the component
constexpr unsigned FH_OUT = 0x40000000u;       // pass 6, in a root's word: the component holds a pixel of the frame's border
constexpr unsigned FH_FILL = 0x20000000u;      // pass 7, in a root's word: a hole that is filled
constexpr unsigned FH_SIZE = 0x001fffffu;
constexpr int FH_LDS_PIX = 15360;              // frames of up to this many pixels keep their labels in LDS (61440 bytes)

struct FhArgs {
    const uint8_t* mask; const uint8_t* target; uint8_t* out; int32_t* info; unsigned* ws;
    int HW, W, H, stride, cls, conn, max_area;
};

template <bool LDS>
struct Labels : FrameWords<LDS, unsigned> {
    using FrameWords<LDS, unsigned>::ld;
    __device__ __forceinline__ bool in(unsigned i) const { return ld(i) != FH_NONE; }
    // the word of the root of pixel p of Q, from pass 5 on
    __device__ __forceinline__ unsigned root_word(unsigned p) const { const unsigned v = ld(p); return (v & FH_ROOT) ? v : ld(v); }
};

template <bool LDS>
__device__ __forceinline__ unsigned fh_find(const Labels<LDS>& L, unsigned x, int bound, bool& fail)
{
    for (int it = 0; it < bound; ++it) {
        const unsigned v = L.ld(x);
        if (v == x || (v & FH_ROOT)) return x;
        x = v;
    }
    fail = true;
    return x;
}

template <bool LDS>
__device__ __forceinline__ void fh_unite(const Labels<LDS>& L, unsigned a, unsigned b, int bound, bool& fail)
{
    for (int it = 0; it < bound; ++it) {
        a = fh_find(L, a, bound, fail);
        b = fh_find(L, b, bound, fail);
        if (a == b || fail) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = L.amin(a, b);                 // a was a root when read: link it under b
        if (old == a) return;
        a = old;                                           // it no longer was (old < a): whatever a pointed to is united with b instead
    }
    fail = true;
}

template <bool LDS, int NT>
__global__ __launch_bounds__(NT) void fill_holes_kernel(FhArgs a)
{
    constexpr int NW = NT / 64;
    __shared__ uint4 s_lab[LDS ? FH_LDS_PIX / 4 : 1];
    __shared__ int s_cnt[NW][3], s_hole[NW][4], s_hit[NW][1], s_fail;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, HW = a.HW, W = a.W, H = a.H;
    const size_t f = blockIdx.x;
    const unsigned cls = (unsigned)a.cls;
    const uint8_t* base = a.mask + f * (size_t)HW;
    const uint8_t* tgt = a.target ? a.target + f * (size_t)HW : nullptr;
    uint8_t* outb = a.out + f * (size_t)HW;
    int32_t* info = a.info + f * 8;
    const MaskFrame<NT> fr(base, HW, W, cls);
    uint4* lab4;
    if constexpr (LDS) lab4 = s_lab;
    else lab4 = reinterpret_cast<uint4*>(a.ws + f * (size_t)a.stride);
    const Labels<LDS> L{{reinterpret_cast<unsigned*>(lab4)}};
    if (tid == 0) s_fail = 0;

    // pass 1: n, and against the target what P hits and how many pixels of the class it has
    int n, hit_before, n_target;
    {
        int c = 0, hb = 0, nt = 0;
        fr.sweep_bits([&](unsigned m, int p0) {
            c += __builtin_popcount(m);
            if (tgt) visit_p(m, p0, [&](int p) { hb += tgt[p] == cls ? 1 : 0; });
        });
        if (tgt) {
            const MaskFrame<NT> ft(tgt, HW, W, cls);
            ft.sweep_bits([&](unsigned m, int) { nt += __builtin_popcount(m); });
        }
        c = wave_sum(c);
        hb = wave_sum(hb);
        nt = wave_sum(nt);
        if (lane == 0) { s_cnt[wv][0] = c; s_cnt[wv][1] = hb; s_cnt[wv][2] = nt; }
        __syncthreads();
        n = wg_sum(s_cnt, 0);
        hit_before = wg_sum(s_cnt, 1);
        n_target = wg_sum(s_cnt, 2);
    }

    int holes = 0, holes_filled = 0, filled = 0, largest = 0;
    if (n > 0 && n < HW && H > 2 && W > 2) {               // (uniform; otherwise every pixel of Q touches the border)
        // pass 2: no pixel has a label
        for (int i = tid; i < a.stride / 4; i += NT) lab4[i] = make_uint4(FH_NONE, FH_NONE, FH_NONE, FH_NONE);
        __syncthreads();

        // pass 3: the lane's own horizontal runs of Q.  prev / run are carried from pixel to pixel: p continues a run when the lane saw p - 1
        // just before it and both lie in one row
        {
            int prev = -2;
            unsigned run = 0;
            fr.sweep_not_xy([&](int p, int x, int) {
                if (!(p == prev + 1 && x > 0)) run = (unsigned)p;
                L.st((unsigned)p, run);
                prev = p;
            });
        }
        __syncthreads();

        // pass 4: unite p with its backward neighbours in Q.  left: only where pass 3 started a new run at p.  up: not when left and up-left
        // are both in Q -- the left neighbour is then joined to up-left (by this very rule, by induction along the row) and up-left to up.
        // 8-connectivity, up not in Q: up-left unless left is in Q (left's own `up`), and up-right.  With up in Q the diagonal neighbours
        // are up's horizontal neighbours.
        bool fail = false;
        {
            int prev = -2;
            const bool c8 = a.conn == 8;
            fr.sweep_not_xy([&](int p, int x, int y) {
                const bool newrun = !(p == prev + 1 && x > 0);
                prev = p;
                const unsigned up_ = (unsigned)(p - W);
                const bool left = x > 0 && L.in((unsigned)p - 1u);
                if (left && newrun) fh_unite(L, (unsigned)p, (unsigned)p - 1u, HW, fail);
                if (y == 0) return;
                const bool up = L.in(up_);
                const bool upleft = x > 0 && L.in(up_ - 1u);
                if (up) {
                    if (!(left && upleft)) fh_unite(L, (unsigned)p, up_, HW, fail);
                } else if (c8) {
                    if (upleft && !left) fh_unite(L, (unsigned)p, up_ - 1u, HW, fail);
                    if (x < W - 1 && L.in(up_ + 1u)) fh_unite(L, (unsigned)p, up_ + 1u, HW, fail);
                }
            });
        }
        __syncthreads();

        // pass 5: every pixel points at its root; a root's own word becomes the (empty) record of its component
        fr.sweep_not_p([&](int p) {
            const unsigned r = fh_find(L, (unsigned)p, HW, fail);
            L.st((unsigned)p, r == (unsigned)p ? FH_ROOT : r);
        });
        if (fail) s_fail = 1;
        __syncthreads();

        // pass 6: sizes and the border flag.  A lane adds once per stretch of pixels with one root; what is left at the end goes wave-wide when
        // the whole wave holds one root (a 64-lane atomic on one address is served lane by lane) -- the outside component of an LV frame
        {
            unsigned cr = FH_NONE, cc = 0;
            bool cb = false;
            auto flush = [&]() {
                L.aadd(cr, cc);
                if (cb) L.aor(cr, FH_OUT);
            };
            fr.sweep_not_xy([&](int p, int x, int y) {
                const unsigned v = L.ld((unsigned)p);
                const unsigned r = (v & FH_ROOT) ? (unsigned)p : v;
                if (r != cr) {
                    if (cc) flush();
                    cr = r;
                    cc = 0;
                    cb = false;
                }
                ++cc;
                cb = cb || x == 0 || x == W - 1 || y == 0 || y == H - 1;
            });
            const bool has = cc > 0;
            const unsigned long long bal = __ballot(has);
            if (bal) {                                     // (wave-uniform)
                const int leader = __ffsll((long long)bal) - 1;
                const unsigned r0 = (unsigned)__shfl((int)cr, leader);
                if (__ballot(has && cr != r0) == 0) {
                    const int s = wave_sum(has ? (int)cc : 0);
                    const bool b = __ballot(has && cb) != 0;
                    if (lane == leader) {
                        L.aadd(r0, (unsigned)s);
                        if (b) L.aor(r0, FH_OUT);
                    }
                } else if (has) {
                    flush();
                }
            }
        }
        __syncthreads();

        // pass 7: the holes.  A root is met by the one lane that owns its pixel, which alone writes FILL into it
        {
            int c = 0, cf = 0, px = 0, big = 0;
            const bool bad = s_fail != 0;
            fr.sweep_not_p([&](int p) {
                const unsigned v = L.ld((unsigned)p);
                if ((v & FH_ROOT) && !(v & FH_OUT)) {
                    const int size = (int)(v & FH_SIZE);
                    ++c;
                    big = size > big ? size : big;
                    if (!bad && (a.max_area == 0 || size <= a.max_area)) {
                        ++cf;
                        px += size;
                        L.st((unsigned)p, v | FH_FILL);
                    }
                }
            });
            c = wave_sum(c);
            cf = wave_sum(cf);
            px = wave_sum(px);
            big = wave_max(big);
            if (lane == 0) { s_hole[wv][0] = c; s_hole[wv][1] = cf; s_hole[wv][2] = px; s_hole[wv][3] = big; }
            __syncthreads();
            holes = wg_sum(s_hole, 0);
            holes_filled = wg_sum(s_hole, 1);
            filled = wg_sum(s_hole, 2);
#pragma unroll
            for (int w = 0; w < NW; ++w) largest = s_hole[w][3] > largest ? s_hole[w][3] : largest;
        }
        if (s_fail) { holes = -1; holes_filled = filled = largest = 0; }
    }

    // pass 8: out, and what the filled pixels were in the target
    int hf = 0;
    const bool fill = holes_filled > 0;
    auto filled_at = [&](int p) -> bool {                  // p is of Q
        if (!(L.root_word((unsigned)p) & FH_FILL)) return false;
        if (tgt) hf += tgt[p] == cls ? 1 : 0;
        return true;
    };
    if (fill || outb != base) {                            // (uniform; in place with nothing to fill there is nothing to write)
        if (((reinterpret_cast<uintptr_t>(outb) - reinterpret_cast<uintptr_t>(base)) & 15u) == 0) {
            // out is aligned like mask: the same head / body / tail
            auto byte_at = [&](int p) {
                unsigned b = base[p];
                if (fill && b != cls && filled_at(p)) b = cls;
                outb[p] = (uint8_t)b;
            };
            if (tid < fr.head) byte_at(tid);
            uint4* obody = reinterpret_cast<uint4*>(outb + fr.head);
            for (int v = tid; v < fr.nvec; v += NT) {
                const uint4 r = fr.body[v];
                unsigned w[4] = {r.x, r.y, r.z, r.w};
                const unsigned m = fill ? match16(r, cls) ^ 0xffffu : 0u;
                if (m) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if ((m >> (4 * q + e)) & 1u)
                                if (filled_at(fr.head + 16 * v + 4 * q + e)) w[q] = (w[q] & ~(0xffu << (8 * e))) | (cls << (8 * e));
                }
                obody[v] = make_uint4(w[0], w[1], w[2], w[3]);
            }
            if (tid < fr.tail) byte_at(fr.head + fr.nbody + tid);
        } else {
            for (int p = tid; p < HW; p += NT) {
                unsigned b = base[p];
                if (fill && b != cls && filled_at(p)) b = cls;
                outb[p] = (uint8_t)b;
            }
        }
    }
    hf = wave_sum(hf);
    if (lane == 0) s_hit[wv][0] = hf;
    __syncthreads();
    if (tid < 8) {
        int v = 0;
        if (tid == 0) v = holes;
        else if (tid == 1) v = holes_filled;
        else if (tid == 2) v = n;
        else if (tid == 3) v = filled;
        else if (tid == 4) v = largest;
        else if (tid == 5) v = hit_before;
        else if (tid == 6) v = wg_sum(s_hit, 0);
        else v = n_target;
        info[tid] = v;
    }
}

// label words per frame in the workspace: H*W rounded up to whole 16-byte vectors
inline size_t fh_stride(int H, int W) { return ((size_t)H * (size_t)W + 3) & ~(size_t)3; }

}  // namespace

extern "C" size_t gdkvm_fill_holes_workspace_bytes(int frames, int H, int W)
{
    if (!mask_shape_ok(frames, H, W) || H * W <= FH_LDS_PIX) return 0;
    return (size_t)frames * fh_stride(H, W) * sizeof(unsigned);
}

extern "C" int gdkvm_fill_holes(const uint8_t* mask, const uint8_t* target, uint8_t* out, int32_t* info, void* workspace, size_t workspace_bytes,
                                int frames, int H, int W, int cls, int connectivity, int max_area, void* stream)
{
    if (int rc = mask_check_shape("fill_holes", frames, H, W)) return rc;
    if (int rc = mask_check_cls("fill_holes", GDKVM_ERR_SHAPE, cls)) return rc;
    if (connectivity != 4 && connectivity != 8) return gdkvm_fail(GDKVM_ERR_SHAPE, "fill_holes: connectivity=%d is neither 4 nor 8", connectivity);
    if (max_area < 0) return gdkvm_fail(GDKVM_ERR_SHAPE, "fill_holes: max_area=%d must be >= 0 (0 = holes of any size)", max_area);
    if (frames == 0) return GDKVM_OK;
    if (!mask || !out || !info) return gdkvm_fail(GDKVM_ERR_SHAPE, "fill_holes: null pointer (mask, out and info are required)");
    if (int rc = mask_check_aligned16("fill_holes", GDKVM_ERR_SHAPE, "info", {info})) return rc;
    const size_t total = (size_t)frames * (size_t)H * (size_t)W;
    if (out != mask && out < mask + total && mask < out + total)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "fill_holes: out must be mask itself (in place) or not overlap it");
    const size_t need = gdkvm_fill_holes_workspace_bytes(frames, H, W);
    if (int rc = mask_check_workspace("fill_holes", H, W, need, workspace, workspace_bytes)) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    FhArgs a{mask, target, out, info, static_cast<unsigned*>(workspace), H * W, W, H, (int)fh_stride(H, W), cls, connectivity, max_area};
    if (!need) hipLaunchKernelGGL((fill_holes_kernel<true, 512>), dim3((unsigned)frames), dim3(512), 0, st, a);
    else hipLaunchKernelGGL((fill_holes_kernel<false, 1024>), dim3((unsigned)frames), dim3(1024), 0, st, a);
    GDKVM_LAUNCH_CHECK("fill_holes_kernel");
    return GDKVM_OK;
}
