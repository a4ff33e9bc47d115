// mask_labels.hpp -- connected-component labelling of one frame by its workgroup, shared by largest_component.hip (labels the class) and
// fill_holes.hip (labels the complement).  On top of mask_frame.hpp: the label words, the union-find with its termination argument, passes
// 2-5 (clear, runs, unions, flatten), pass 6 (per-root counts and an optional flag), pass 8 (the rewritten frame), and the launchers' shared
// rules.  A kernel that labels starts here and adds what it counts, what it picks and its info layout.
//
// A frame's labels are one 32-bit word per pixel, in LDS while the frame has at most LABEL_LDS_PIX pixels, otherwise in the frame's slice of
// the caller's workspace (FrameWords: every access an agent-scope relaxed atomic served by L2).  NOT = false labels the pixels of the class
// (MaskFrame::sweep_*), NOT = true those of its complement (sweep_not_*); "the set" below is whichever is labelled.
#pragma once
#include "mask_frame.hpp"

constexpr unsigned LABEL_NONE = 0xffffffffu;   // the word of a pixel outside the set
constexpr unsigned LABEL_ROOT = 0x80000000u;   // from pass 5 on: this pixel is its component's smallest index, its label; the low bits count
                                               // the component's pixels (at most 2^20) and the bits between are the kernel's own flags
constexpr int LABEL_LDS_PIX = 15360;           // frames of up to this many pixels keep their labels in LDS (61440 of the workgroup's 64 KiB)

template <bool LDS>
struct Labels : FrameWords<LDS, unsigned> {
    using FrameWords<LDS, unsigned>::ld;
    __device__ __forceinline__ bool in(unsigned i) const { return ld(i) != LABEL_NONE; }
    // from pass 5 on, for a pixel p of the set: its label, and its label's word
    __device__ __forceinline__ unsigned root(unsigned p) const { const unsigned v = ld(p); return (v & LABEL_ROOT) ? p : v; }
    __device__ __forceinline__ unsigned root_word(unsigned p) const { const unsigned v = ld(p); return (v & LABEL_ROOT) ? v : ld(v); }
};

// The label words of frame f: the workgroup's LDS, or the frame's slice (stride words) of the workspace
template <bool LDS>
__device__ __forceinline__ Labels<LDS> frame_labels(unsigned* ws, size_t f, int stride)
{
    __shared__ uint4 s_lab[LDS ? LABEL_LDS_PIX / 4 : 1];
    if constexpr (LDS) return {{reinterpret_cast<unsigned*>(s_lab)}};
    else return {{ws + f * (size_t)stride}};
}

template <bool NOT, int NT, class F>
__device__ __forceinline__ void sweep_set_p(const MaskFrame<NT>& fr, F&& f)
{
    if constexpr (NOT) fr.sweep_not_p(f);
    else fr.sweep_p(f);
}
template <bool NOT, int NT, class F>
__device__ __forceinline__ void sweep_set_xy(const MaskFrame<NT>& fr, F&& f)
{
    if constexpr (NOT) fr.sweep_not_xy(f);
    else fr.sweep_xy(f);
}

// Union-find over the label words.  A word never exceeds its own index and labels only decrease: label_unite links the larger root under the
// smaller with atomicMin.  Loop bounds: a chain p > L[p] > L[L[p]] ... strictly descends through pixel indices, so label_find ends within
// bound = H*W steps; in label_unite the larger of the two roots strictly descends from one retry to the next (the value atomicMin returns is
// below the index it was applied to, or the link succeeded), so it ends within H*W retries.  Both loops count to H*W and, should that ever
// be reached, set `fail` rather than spinning: the kernel then reports -1 and writes out = mask.
template <bool LDS>
__device__ __forceinline__ unsigned label_find(const Labels<LDS>& L, unsigned x, int bound, bool& fail)
{
    for (int it = 0; it < bound; ++it) {
        const unsigned v = L.ld(x);
        if (v == x || (v & LABEL_ROOT)) return x;
        x = v;
    }
    fail = true;
    return x;
}

template <bool LDS>
__device__ __forceinline__ void label_unite(const Labels<LDS>& L, unsigned a, unsigned b, int bound, bool& fail)
{
    for (int it = 0; it < bound; ++it) {
        a = label_find(L, a, bound, fail);
        b = label_find(L, b, bound, fail);
        if (a == b || fail) return;
        if (a < b) { const unsigned t = a; a = b; b = t; }
        const unsigned old = L.amin(a, b);                 // a was a root when read: link it under b
        if (old == a) return;
        a = old;                                           // it no longer was (old < a): whatever a pointed to is united with b instead
    }
    fail = true;
}

// Passes 2-5, a workgroup barrier behind each: afterwards every pixel of the set holds its label and a label's own word is ROOT | 0.
// nwords = the frame's label words (label_stride); s_fail = the workgroup's failure flag in LDS, raised here when a union-find loop ran out.
template <bool NOT, bool LDS, int NT>
__device__ __forceinline__ void label_components(const MaskFrame<NT>& fr, const Labels<LDS>& L, int nwords, int HW, bool c8, int& s_fail)
{
    const int tid = threadIdx.x, W = fr.W;
    // pass 2: no pixel has a label
    uint4* lab4 = reinterpret_cast<uint4*>(L.w);
    for (int i = tid; i < nwords / 4; i += NT) lab4[i] = make_uint4(LABEL_NONE, LABEL_NONE, LABEL_NONE, LABEL_NONE);
    __syncthreads();

    // pass 3: L[p] = the first pixel of p's horizontal run inside the lane's 16-byte vector (most horizontal links then cost nothing).  prev /
    // run are carried from pixel to pixel: p continues a run when the lane saw p - 1 just before it and both lie in one row
    {
        int prev = -2;
        unsigned run = 0;
        sweep_set_xy<NOT>(fr, [&](int p, int x, int) {
            if (!(p == prev + 1 && x > 0)) run = (unsigned)p;
            L.st((unsigned)p, run);
            prev = p;
        });
    }
    __syncthreads();

    // pass 4: unite p with its backward neighbours in the set.  left: only where pass 3 started a new run at p.  up: not when left and
    // up-left are both in the set -- the left neighbour is then joined to up-left (by this very rule, by induction along the row) and up-left
    // to up.  8-connectivity, up not in the set: up-left unless left is in the set (left's own `up`), and up-right.  With up in the set the
    // diagonal neighbours are up's horizontal neighbours.
    bool fail = false;
    {
        int prev = -2;
        sweep_set_xy<NOT>(fr, [&](int p, int x, int y) {
            const bool newrun = !(p == prev + 1 && x > 0);
            prev = p;
            const unsigned up_ = (unsigned)(p - W);
            const bool left = x > 0 && L.in((unsigned)p - 1u);
            if (left && newrun) label_unite(L, (unsigned)p, (unsigned)p - 1u, HW, fail);
            if (y == 0) return;
            const bool up = L.in(up_);
            const bool upleft = x > 0 && L.in(up_ - 1u);
            if (up) {
                if (!(left && upleft)) label_unite(L, (unsigned)p, up_, HW, fail);
            } else if (c8) {
                if (upleft && !left) label_unite(L, (unsigned)p, up_ - 1u, HW, fail);
                if (x < W - 1 && L.in(up_ + 1u)) label_unite(L, (unsigned)p, up_ + 1u, HW, fail);
            }
        });
    }
    __syncthreads();

    // pass 5: every pixel points at its label; a label's own word becomes the (empty) record of its component
    sweep_set_p<NOT>(fr, [&](int p) {
        const unsigned r = label_find(L, (unsigned)p, HW, fail);
        L.st((unsigned)p, r == (unsigned)p ? LABEL_ROOT : r);
    });
    if (fail) s_fail = 1;
    __syncthreads();
}

// Pass 6 (the caller's barrier behind it): L[root] += 1 per pixel of the set, and with FLAG != 0, L[root] |= FLAG for a pixel with
// flagged(x, y).  A lane flushes once per stretch of pixels with one root; what is left at the end goes wave-wide when the whole wave holds
// one root (a 64-lane atomic on one address is served lane by lane).  Sums and ORs commute and the count never reaches the flags, so a
// root's word does not depend on the order in which lanes arrive.
struct NoLabelFlag {
    __device__ __forceinline__ bool operator()(int, int) const { return false; }
};
template <bool NOT, unsigned FLAG = 0u, bool LDS, int NT, class B = NoLabelFlag>
__device__ __forceinline__ void label_sizes(const MaskFrame<NT>& fr, const Labels<LDS>& L, B flagged = B())
{
    unsigned cr = LABEL_NONE, cc = 0;
    bool cb = false;
    auto flush = [&]() {
        L.aadd(cr, cc);
        if (FLAG != 0u && cb) L.aor(cr, FLAG);
    };
    auto pixel = [&](int p, bool b) {
        const unsigned r = L.root((unsigned)p);
        if (r != cr) {
            if (cc) flush();
            cr = r;
            cc = 0;
            cb = false;
        }
        ++cc;
        cb = cb || b;
    };
    if constexpr (FLAG != 0u) sweep_set_xy<NOT>(fr, [&](int p, int x, int y) { pixel(p, flagged(x, y)); });
    else sweep_set_p<NOT>(fr, [&](int p) { pixel(p, false); });
    const bool has = cc > 0;
    const unsigned long long bal = __ballot(has);
    if (bal) {                                             // (wave-uniform)
        const int leader = __ffsll((long long)bal) - 1;
        const unsigned r0 = (unsigned)__shfl((int)cr, leader);
        if (__ballot(has && cr != r0) == 0) {
            const int s = wave_sum(has ? (int)cc : 0);
            const bool b = FLAG != 0u && __ballot(has && cb) != 0;
            if ((int)(threadIdx.x & 63) == leader) {
                L.aadd(r0, (unsigned)s);
                if (b) L.aor(r0, FLAG);
            }
        } else if (has) {
            flush();
        }
    }
}

// Pass 8: out = the frame with byte `repl` at the pixels of the set (the CANDIDATES: of the class with NOT = false, of the complement with
// NOT = true) for which pick(p) holds.  pick is called once per candidate and only while `change` (uniform) says that anything changes; it
// may count as it goes.  Head bytes, 16-byte vectors and tail bytes when out is aligned like the frame, else byte by byte; in place with
// nothing to change there is nothing to write.
template <bool NOT, int NT, class P>
__device__ __forceinline__ void rewrite_frame(const MaskFrame<NT>& fr, uint8_t* out, int HW, bool change, unsigned repl, P&& pick)
{
    const int tid = threadIdx.x;
    const uint8_t* base = fr.base;
    const unsigned cls = fr.cls;
    if (!change && out == base) return;                    // (uniform)
    auto byte_at = [&](int p) {
        unsigned b = base[p];
        if (change && (b == cls) != NOT && pick(p)) b = repl;
        out[p] = (uint8_t)b;
    };
    if (((reinterpret_cast<uintptr_t>(out) - reinterpret_cast<uintptr_t>(base)) & 15u) == 0) {
        if (tid < fr.head) byte_at(tid);
        uint4* obody = reinterpret_cast<uint4*>(out + fr.head);
        for (int v = tid; v < fr.nvec; v += NT) {
            const uint4 r = fr.body[v];
            unsigned w[4] = {r.x, r.y, r.z, r.w};
            const unsigned m = change ? match16(r, cls) ^ (NOT ? 0xffffu : 0u) : 0u;
            if (m) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if ((m >> (4 * q + e)) & 1u)
                            if (pick(fr.head + 16 * v + 4 * q + e)) w[q] = (w[q] & ~(0xffu << (8 * e))) | (repl << (8 * e));
            }
            obody[v] = make_uint4(w[0], w[1], w[2], w[3]);
        }
        if (tid < fr.tail) byte_at(fr.head + fr.nbody + tid);
    } else {
        for (int p = tid; p < HW; p += NT) byte_at(p);
    }
}

// The launchers' shared rules, written like mask_frame.hpp's checks: GDKVM_OK or gdkvm_fail(...) with the kernel's name in front.
// label words per frame in the workspace: H*W rounded up to whole 16-byte vectors
inline size_t label_stride(int H, int W) { return ((size_t)H * (size_t)W + 3) & ~(size_t)3; }
// what a kernel's *_workspace_bytes returns: 0 for the LDS form (and for a shape the launcher refuses anyway)
inline size_t label_workspace_bytes(int frames, int H, int W)
{
    if (!mask_shape_ok(frames, H, W) || H * W <= LABEL_LDS_PIX) return 0;
    return (size_t)frames * label_stride(H, W) * sizeof(unsigned);
}
inline int mask_check_connectivity(const char* name, int connectivity)
{
    if (connectivity == 4 || connectivity == 8) return GDKVM_OK;
    return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: connectivity=%d is neither 4 nor 8", name, connectivity);
}
// mask, out and info are there, info is aligned, and out is mask itself or does not overlap its `total` bytes
inline int mask_check_in_out(const char* name, const uint8_t* mask, const uint8_t* out, const int32_t* info, size_t total)
{
    if (!mask || !out || !info) return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: null pointer (mask, out and info are required)", name);
    if (int rc = mask_check_aligned16(name, GDKVM_ERR_SHAPE, "info", {info})) return rc;
    if (out != mask && out < mask + total && mask < out + total)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: out must be mask itself (in place) or not overlap it", name);
    return GDKVM_OK;
}
