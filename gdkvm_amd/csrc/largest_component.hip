// largest_component.hip -- keep the largest connected component of one class of label masks on the device (the clean-up in front of
// lv_measure: a false-positive island far from the ventricle otherwise enters the long axis and the disks).  include/gdkvm.h holds the
// definition; labels, sizes and the filtered mask are integers that depend on neither the algorithm nor the schedule.
//
// ONE workgroup per frame (256 lanes in the LDS form; 1024 in the workspace form, whose chains of dependent L2 loads want more waves in
// flight): no cross-workgroup synchronisation, no fences between workgroups, no flag anybody spins on.  A frame's
// labels are one 32-bit word per pixel, in LDS while the frame has at most CC_LDS_PIX pixels (60 KiB of the workgroup's 64 KiB; the 112 x 112
// mask of cfg2 takes 49 KiB), otherwise in the frame's slice of the caller's workspace, where every access is an agent-scope relaxed atomic
// (served by L2, so no wave ever reads a stale line of the CU's L1 behind another wave's atomic).  Passes, a workgroup barrier between them:
//   1. n = |P|; an empty frame goes straight to the copy.                       2. every word = NONE.
//   3. L[p] = the first pixel of p's horizontal run inside the lane's 16-byte vector (so most of a blob's horizontal links cost nothing).
//   4. union-find: unite(p, q) for the backward neighbours q of p that are not already joined through p's left neighbour.  unite() links the
//      larger root under the smaller with atomicMin; labels only decrease and a word never exceeds its own index.
//   5. flatten: L[p] = root(p); a root's own word becomes ROOT | 0.                6. sizes: L[root] += 1 per pixel (run- and wave-combined).
//   7. components, and the kept one by a two-key maximum (size, then the smaller label).       8. the filtered mask and the hit counts.
// Loop bounds: a chain p > L[p] > L[L[p]] ... strictly descends through pixel indices, so find() ends within H*W steps; in unite() the larger
// of the two roots strictly descends from one retry to the next (the value atomicMin returns is below the index it was applied to, or the
// link succeeded), so it ends within H*W retries.  Both loops count to H*W and, should that ever be reached, raise the frame's failure flag:
// components = -1 and out = mask, rather than spinning.

#include "mask_frame.hpp"

namespace {

typedef unsigned long long u64;

constexpr unsigned CC_NONE = 0xffffffffu;      // the word of a pixel that is not of the class
constexpr unsigned CC_ROOT = 0x80000000u;      // from pass 5 on: this pixel is its component's label; the low bits count the component's pixels
constexpr int CC_LDS_PIX = 15360;              // frames of up to this many pixels keep their labels in LDS (61440 bytes)

struct CcArgs {
    const uint8_t* mask; const uint8_t* target; uint8_t* out; int32_t* info; unsigned* ws;
    int HW, W, stride, cls, fill, conn;
};

// The label words, and what passes 3 and 5 make of one
template <bool LDS>
struct Labels : FrameWords<LDS, unsigned> {
    using FrameWords<LDS, unsigned>::ld;
    __device__ __forceinline__ bool in(unsigned i) const { return ld(i) != CC_NONE; }
    // the label of pixel p of the class, from pass 5 on
    __device__ __forceinline__ unsigned root(unsigned p) const { const unsigned v = ld(p); return (v & CC_ROOT) ? p : v; }
};

template <bool LDS>
__device__ __forceinline__ unsigned cc_find(const Labels<LDS>& L, unsigned x, int bound, bool& fail)
{
    for (int it = 0; it < bound; ++it) {
        const unsigned v = L.ld(x);
        if (v == x || (v & CC_ROOT)) return x;
        x = v;
    }
    fail = true;
    return x;
}

template <bool LDS>
__device__ __forceinline__ void cc_unite(const Labels<LDS>& L, unsigned a, unsigned b, int bound, bool& fail)
{
    for (int it = 0; it < bound; ++it) {
        a = cc_find(L, a, bound, fail);
        b = cc_find(L, b, bound, fail);
        if (a == b || fail) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = L.amin(a, b);                 // a was a root when read: link it under b
        if (old == a) return;
        a = old;                                           // it no longer was (old < a): whatever a pointed to is united with b instead
    }
    fail = true;
}

template <bool LDS, int NT>
__global__ __launch_bounds__(NT) void largest_component_kernel(CcArgs a)
{
    constexpr int NW = NT / 64;
    __shared__ uint4 s_lab[LDS ? CC_LDS_PIX / 4 : 1];
    __shared__ int s_n[NW], s_comp[NW], s_hit[NW][2], s_fail;
    __shared__ u64 s_best[NW];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, HW = a.HW, W = a.W;
    const size_t f = blockIdx.x;
    const unsigned cls = (unsigned)a.cls, fill = (unsigned)a.fill;
    const uint8_t* base = a.mask + f * (size_t)HW;
    const uint8_t* tgt = a.target ? a.target + f * (size_t)HW : nullptr;
    uint8_t* outb = a.out + f * (size_t)HW;
    int32_t* info = a.info + f * 8;
    // (MaskFrame's constructor written out: the constructor's tail, (HW - head) & 15, is other code than this kernel was measured with)
    MaskFrame<NT> fr;
    fr.base = base; fr.W = W; fr.cls = cls;
    fr.head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(base) & 15u)) & 15u);
    if (fr.head > HW) fr.head = HW;
    fr.nvec = (HW - fr.head) >> 4;
    fr.nbody = 16 * fr.nvec;
    fr.tail = HW - fr.head - 16 * fr.nvec;
    fr.body = reinterpret_cast<const uint4*>(base + fr.head);
    uint4* lab4;
    if constexpr (LDS) lab4 = s_lab;
    else lab4 = reinterpret_cast<uint4*>(a.ws + f * (size_t)a.stride);
    const Labels<LDS> L{{reinterpret_cast<unsigned*>(lab4)}};
    if (tid == 0) s_fail = 0;

    // pass 1: n
    int n;
    {
        int c = 0;
        fr.sweep_bits([&](unsigned m, int) { c += __builtin_popcount(m); });
        c = wave_sum(c);
        if (lane == 0) s_n[wv] = c;
        __syncthreads();
        n = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) n += s_n[w];
    }

    int comps = 0, n_kept = 0, label_kept = -1;
    bool filter = false;
    if (n > 0) {                                           // (uniform)
        // pass 2: no pixel has a label
        for (int i = tid; i < a.stride / 4; i += NT) lab4[i] = make_uint4(CC_NONE, CC_NONE, CC_NONE, CC_NONE);
        __syncthreads();

        // pass 3: the lane's own horizontal runs.  prev / run are carried from pixel to pixel: p continues a run when the lane saw p - 1 just
        // before it and both lie in one row
        {
            int prev = -2;
            unsigned run = 0;
            fr.sweep_xy([&](int p, int x, int) {
                if (!(p == prev + 1 && x > 0)) run = (unsigned)p;
                L.st((unsigned)p, run);
                prev = p;
            });
        }
        __syncthreads();

        // pass 4: unite p with its backward neighbours.  left: only where pass 3 started a new run at p.  up: not when left and up-left are
        // both of the class -- the left neighbour is then joined to up-left (by this very rule, by induction along the row) and up-left to up.
        // 8-connectivity, up not of the class: up-left unless left is of the class (left's own `up`), and up-right.  With up of the class the
        // diagonal neighbours are up's horizontal neighbours.
        bool fail = false;
        {
            int prev = -2;
            const bool c8 = a.conn == 8;
            fr.sweep_xy([&](int p, int x, int y) {
                const bool newrun = !(p == prev + 1 && x > 0);
                prev = p;
                const unsigned up_ = (unsigned)(p - W);
                const bool left = x > 0 && L.in((unsigned)p - 1u);
                if (left && newrun) cc_unite(L, (unsigned)p, (unsigned)p - 1u, HW, fail);
                if (y == 0) return;
                const bool up = L.in(up_);
                const bool upleft = x > 0 && L.in(up_ - 1u);
                if (up) {
                    if (!(left && upleft)) cc_unite(L, (unsigned)p, up_, HW, fail);
                } else if (c8) {
                    if (upleft && !left) cc_unite(L, (unsigned)p, up_ - 1u, HW, fail);
                    if (x < W - 1 && L.in(up_ + 1u)) cc_unite(L, (unsigned)p, up_ + 1u, HW, fail);
                }
            });
        }
        __syncthreads();

        // pass 5: every pixel points at its label; a label's own word becomes the (empty) counter of its component
        fr.sweep_p([&](int p) {
            const unsigned r = cc_find(L, (unsigned)p, HW, fail);
            L.st((unsigned)p, r == (unsigned)p ? CC_ROOT : r);
        });
        if (fail) s_fail = 1;
        __syncthreads();

        // pass 6: sizes.  A lane adds once per stretch of pixels with one label; what is left at the end is summed wave-wide when the whole
        // wave holds one label (a 64-lane atomic on one address is served lane by lane)
        {
            unsigned cr = CC_NONE, cc = 0;
            fr.sweep_p([&](int p) {
                const unsigned r = L.root((unsigned)p);
                if (r != cr) {
                    if (cc) L.aadd(cr, cc);
                    cr = r;
                    cc = 0;
                }
                ++cc;
            });
            const bool has = cc > 0;
            const u64 bal = __ballot(has);
            if (bal) {                                     // (wave-uniform)
                const int leader = __ffsll((long long)bal) - 1;
                const unsigned r0 = (unsigned)__shfl((int)cr, leader);
                if (__ballot(has && cr != r0) == 0) {
                    const int s = wave_sum(has ? (int)cc : 0);
                    if (lane == leader) L.aadd(r0, (unsigned)s);
                } else if (has) {
                    L.aadd(cr, cc);
                }
            }
        }
        __syncthreads();

        // pass 7: the components, and the largest (ties: the smallest label) as the maximum of size * 2^32 + ~label
        {
            int c = 0;
            u64 best = 0;
            fr.sweep_p([&](int p) {
                const unsigned v = L.ld((unsigned)p);
                if (v & CC_ROOT) {
                    ++c;
                    const u64 key = ((u64)(v & ~CC_ROOT) << 32) | (u64)(~(unsigned)p);
                    best = key > best ? key : best;
                }
            });
            c = wave_sum(c);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {             // (not wave_max: through the helper this pass schedules differently)
                const u64 w = (u64)__shfl_xor((long long)best, o);
                best = w > best ? w : best;
            }
            if (lane == 0) { s_comp[wv] = c; s_best[wv] = best; }
            __syncthreads();
            comps = 0;
            best = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                comps += s_comp[w];
                best = s_best[w] > best ? s_best[w] : best;
            }
            n_kept = (int)(best >> 32);
            label_kept = (int)~(unsigned)best;
        }
        if (s_fail) { comps = -1; n_kept = n; label_kept = -1; }
        else filter = n_kept != n;
    }

    // pass 8: out, and what the removed pixels were in the target
    int hc = 0, hf = 0;
    const unsigned kl = (unsigned)label_kept;
    auto removed = [&](int p) -> bool {                    // p is of the class
        if (L.root((unsigned)p) == kl) return false;
        if (tgt) {
            const unsigned t = tgt[p];
            hc += t == cls ? 1 : 0;
            hf += t == fill ? 1 : 0;
        }
        return true;
    };
    if (filter || outb != base) {                          // (uniform; in place with nothing to remove there is nothing to write)
        if (((reinterpret_cast<uintptr_t>(outb) - reinterpret_cast<uintptr_t>(base)) & 15u) == 0) {
            // out is aligned like mask: the same head / body / tail
            auto byte_at = [&](int p) {
                unsigned b = base[p];
                if (filter && b == cls && removed(p)) b = fill;
                outb[p] = (uint8_t)b;
            };
            if (tid < fr.head) byte_at(tid);
            uint4* obody = reinterpret_cast<uint4*>(outb + fr.head);
            for (int v = tid; v < fr.nvec; v += NT) {
                const uint4 r = fr.body[v];
                unsigned w[4] = {r.x, r.y, r.z, r.w};
                const unsigned m = filter ? match16(r, cls) : 0u;
                if (m) {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if ((m >> (4 * q + e)) & 1u)
                                if (removed(fr.head + 16 * v + 4 * q + e)) w[q] = (w[q] & ~(0xffu << (8 * e))) | (fill << (8 * e));
                }
                obody[v] = make_uint4(w[0], w[1], w[2], w[3]);
            }
            if (tid < fr.tail) byte_at(fr.head + fr.nbody + tid);
        } else {
            for (int p = tid; p < HW; p += NT) {
                unsigned b = base[p];
                if (filter && b == cls && removed(p)) b = fill;
                outb[p] = (uint8_t)b;
            }
        }
    }
    hc = wave_sum(hc);
    hf = wave_sum(hf);
    if (lane == 0) { s_hit[wv][0] = hc; s_hit[wv][1] = hf; }
    __syncthreads();
    if (tid < 8) {
        int v = 0;
        if (tid == 0) v = comps;
        else if (tid == 1) v = n;
        else if (tid == 2) v = n_kept;
        else if (tid == 3) v = label_kept;
        else if (tid == 4 || tid == 5)
            for (int w = 0; w < NW; ++w) v += s_hit[w][tid - 4];
        info[tid] = v;
    }
}

// label words per frame in the workspace: H*W rounded up to whole 16-byte vectors
inline size_t cc_stride(int H, int W) { return ((size_t)H * (size_t)W + 3) & ~(size_t)3; }

}  // namespace

extern "C" size_t gdkvm_largest_component_workspace_bytes(int frames, int H, int W)
{
    if (!mask_shape_ok(frames, H, W) || H * W <= CC_LDS_PIX) return 0;
    return (size_t)frames * cc_stride(H, W) * sizeof(unsigned);
}

extern "C" int gdkvm_largest_component(const uint8_t* mask, const uint8_t* target, uint8_t* out, int32_t* info, void* workspace,
                                       size_t workspace_bytes, int frames, int H, int W, int cls, int connectivity, int fill, void* stream)
{
    if (int rc = mask_check_shape("largest_component", frames, H, W)) return rc;
    if (int rc = mask_check_cls("largest_component", GDKVM_ERR_SHAPE, cls)) return rc;
    if (connectivity != 4 && connectivity != 8) return gdkvm_fail(GDKVM_ERR_SHAPE, "largest_component: connectivity=%d is neither 4 nor 8", connectivity);
    if (fill < 0 || fill > 255 || fill == cls)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "largest_component: fill=%d must lie in 0..255 and differ from cls=%d", fill, cls);
    if (frames == 0) return GDKVM_OK;
    if (!mask || !out || !info) return gdkvm_fail(GDKVM_ERR_SHAPE, "largest_component: null pointer (mask, out and info are required)");
    if (int rc = mask_check_aligned16("largest_component", GDKVM_ERR_SHAPE, "info", {info})) return rc;
    const size_t total = (size_t)frames * (size_t)H * (size_t)W;
    if (out != mask && out < mask + total && mask < out + total)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "largest_component: out must be mask itself (in place) or not overlap it");
    const size_t need = gdkvm_largest_component_workspace_bytes(frames, H, W);
    if (int rc = mask_check_workspace("largest_component", H, W, need, workspace, workspace_bytes)) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    CcArgs a{mask, target, out, info, static_cast<unsigned*>(workspace), H * W, W, (int)cc_stride(H, W), cls, fill, connectivity};
    if (!need) hipLaunchKernelGGL((largest_component_kernel<true, 256>), dim3((unsigned)frames), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((largest_component_kernel<false, 1024>), dim3((unsigned)frames), dim3(1024), 0, st, a);
    GDKVM_LAUNCH_CHECK("largest_component_kernel");
    return GDKVM_OK;
}
