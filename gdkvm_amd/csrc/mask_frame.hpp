// mask_frame.hpp -- what the per-frame kernels over uint8 label masks share (lv_measure.hip, largest_component.hip, surface_distance.hip, fill_holes.hip):
// ONE workgroup walks one frame [H, W] of bytes at any byte address.  The frame split and its sweeps, the walk over the set bits of a match
// word, integer wave reductions and the workgroup fold of their per-wave partials, the accessors of a frame's 32-, 16- and 64-bit words, the
// byte-parallel compares of packed label bytes (temporal_vote.hip and mask_to_native.hip count with them) and the launchers' shared
// argument checks.  A new per-frame mask kernel starts here (one that labels connected components: from mask_labels.hpp, one over clips at
// their native size: from native_clips.hpp; both build on this).  No floating-point code: a file may include this ahead of an fp-contract
// pragma of its own.  Like gdkvm_device.hpp, every device helper is __forceinline__ and written with the exact expression the kernels used
// before they shared it (tools/isa_equal.py).
#pragma once
#include <initializer_list>

#include "gdkvm_device.hpp"

// gdkvm_common.hpp's gdkvm_aligned16 for device code (an overload: that header is one of the sources build.source_hash() pins)
__device__ __forceinline__ bool gdkvm_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// the bytes from address a up to the 16-byte grid: 0..15, the head of a run of bytes that is then read or written 16 bytes at a time
__device__ __forceinline__ int head16(uintptr_t a) { return (int)((16u - (unsigned)(a & 15u)) & 15u); }

// Four label bytes to a word, compared byte-parallel: each answer is 0x80 in every byte for which it is yes.
constexpr unsigned BYTES_HI = 0x80808080u, BYTES_LO = 0x7f7f7f7fu, BYTES_ONE = 0x01010101u;
// ... in every byte of x that equals c (exact for every byte value: the low seven bits are tested without a carry into the next byte)
__device__ __forceinline__ unsigned eq80(unsigned x, unsigned c)
{
    const unsigned y = x ^ (c * BYTES_ONE);
    return ~(((y & BYTES_LO) + BYTES_LO) | y) & BYTES_HI;
}
// ... where a and b differ
__device__ __forceinline__ unsigned ne80(unsigned a, unsigned b)
{
    const unsigned y = a ^ b;
    return (((y & BYTES_LO) + BYTES_LO) | y) & BYTES_HI;
}
// ... where a > b, for bytes below 128: (b + 128) - a borrows from no neighbour and keeps its top bit iff b >= a
__device__ __forceinline__ unsigned gt80(unsigned a, unsigned b) { return ~((b | BYTES_HI) - a) & BYTES_HI; }

// bit e = byte e of the vector equals cls
__device__ __forceinline__ unsigned match16(const uint4& v, unsigned cls)
{
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    unsigned m = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) m |= (((w[q] >> (8 * e)) & 0xffu) == cls ? 1u : 0u) << (4 * q + e);
    return m;
}

// f(p, x, y) for every set bit of m in ascending order; bit e is pixel p = p0 + e = y W + x of the frame (row-major, rows of W).  x and y are
// carried from bit to bit: one division per word, none per pixel.
template <class F>
__device__ __forceinline__ void visit_xy(unsigned m, int p0, int W, F&& f)
{
    if (!m) return;
    int y = p0 / W, x = p0 - y * W, prev = 0;
    while (m) {                                            // (at most 32 turns)
        const int e = __builtin_ctz(m);
        m &= m - 1;
        x += e - prev;
        prev = e;
        while (x >= W) { x -= W; ++y; }
        f(p0 + e, x, y);
    }
}
// f(p) for every set bit of m in ascending order
template <class F>
__device__ __forceinline__ void visit_p(unsigned m, int p0, F&& f)
{
    while (m) {
        const int e = __builtin_ctz(m);
        m &= m - 1;
        f(p0 + e);
    }
}

// A frame at any byte address (H W need not be a multiple of 16): up to 15 head bytes (lane t owns byte t), 16-byte vectors (lane t of NT
// owns vectors t, t + NT, ...), up to 15 tail bytes.  A lane meets its pixels in ascending order.
template <int NT>
struct MaskFrame {
    const uint8_t* base; const uint4* body;
    int head, nvec, nbody, tail, W;                        // nbody = 16 nvec, the bytes of the vectors: the tail starts at head + nbody
    unsigned cls;
    // The split is computed in locals: this function is simplified on its own before it is inlined, and from locals the tail comes out as
    // (HW - head) & 15 as in the kernels that had the split inline.
    __device__ __forceinline__ MaskFrame(const uint8_t* base_, int HW, int W_, unsigned cls_) : base(base_), W(W_), cls(cls_)
    {
        int h = head16(reinterpret_cast<uintptr_t>(base_));
        if (h > HW) h = HW;
        const int nv = (HW - h) >> 4;
        head = h; nvec = nv; nbody = 16 * nv; tail = HW - h - 16 * nv;
        body = reinterpret_cast<const uint4*>(base_ + h);
    }
    // f(m, p0): bit e of m = pixel p0 + e is of the class (m may be 0 for a vector; a head or tail byte comes as m = 1)
    template <class F>
    __device__ __forceinline__ void sweep_bits(F&& f) const
    {
        const int tid = threadIdx.x;
        if (tid < head && base[tid] == cls) f(1u, tid);
        for (int v = tid; v < nvec; v += NT) f(match16(body[v], cls), head + 16 * v);
        if (tid < tail && base[head + nbody + tid] == cls) f(1u, head + nbody + tid);
    }
    // f(p) for the lane's pixels of the class
    template <class F>
    __device__ __forceinline__ void sweep_p(F&& f) const
    {
        const int tid = threadIdx.x;
        if (tid < head && base[tid] == cls) f(tid);
        for (int v = tid; v < nvec; v += NT) visit_p(match16(body[v], cls), head + 16 * v, f);
        if (tid < tail && base[head + nbody + tid] == cls) f(head + nbody + tid);
    }
    // f(p, x, y) for the lane's pixels of the class
    template <class F>
    __device__ __forceinline__ void sweep_xy(F&& f) const
    {
        sweep_bits([&](unsigned m, int p0) { visit_xy(m, p0, W, f); });
    }
    // The same three sweeps over the COMPLEMENT, the lane's pixels that are NOT of the class (fill_holes.hip labels those)
    template <class F>
    __device__ __forceinline__ void sweep_not_bits(F&& f) const
    {
        const int tid = threadIdx.x;
        if (tid < head && base[tid] != cls) f(1u, tid);
        for (int v = tid; v < nvec; v += NT) f(match16(body[v], cls) ^ 0xffffu, head + 16 * v);
        if (tid < tail && base[head + nbody + tid] != cls) f(1u, head + nbody + tid);
    }
    template <class F>
    __device__ __forceinline__ void sweep_not_p(F&& f) const
    {
        sweep_not_bits([&](unsigned m, int p0) { visit_p(m, p0, f); });
    }
    template <class F>
    __device__ __forceinline__ void sweep_not_xy(F&& f) const
    {
        sweep_not_bits([&](unsigned m, int p0) { visit_xy(m, p0, W, f); });
    }
};

// Sum, minimum and maximum of an integer (32 or 64 bits, signed or not) over the 64 lanes of a wave, in every lane.  Integers only: the
// floating-point butterflies of the other kernels fix their own widths and orders, and a float sum's bits depend on them.
template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
    static_assert(std::is_integral<T>::value, "integer reductions only");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
template <class T>
__device__ __forceinline__ T wave_min(T v)
{
    static_assert(std::is_integral<T>::value, "integer reductions only");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const T w = __shfl_xor(v, o); v = w < v ? w : v; }
    return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v)
{
    static_assert(std::is_integral<T>::value, "integer reductions only");
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const T w = __shfl_xor(v, o); v = w > v ? w : v; }
    return v;
}

// The workgroup's sum of the NW per-wave partials that lane 0 of each wave stored in column k of s[w][..] in LDS (a barrier between the
// stores and this).
template <class T, int NW, int K>
__device__ __forceinline__ T wg_sum(const T (&s)[NW][K], int k)
{
    T v = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) v += s[w][k];
    return v;
}

// The 32-bit words a frame's workgroup keeps per pixel (labels, distances, bitmaps), indexed by I.  LDS: the frame is small enough for the
// workgroup's LDS, and workgroup-scope relaxed atomics are plain ds instructions.  Otherwise the words are the frame's slice of the caller's
// workspace and every access is an agent-scope relaxed atomic: loads and stores are served by L2, so no wave ever reads a stale line of
// the CU's L1 behind another wave's atomic.
template <bool LDS, class I>
struct FrameWords {
    unsigned* w;
    static constexpr int SCOPE = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
    __device__ __forceinline__ unsigned ld(I i) const { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void st(I i, unsigned v) const { __hip_atomic_store(w + i, v, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void aor(I i, unsigned v) const { __hip_atomic_fetch_or(w + i, v, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ unsigned amin(I i, unsigned v) const { return __hip_atomic_fetch_min(w + i, v, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void aadd(I i, unsigned v) const { __hip_atomic_fetch_add(w + i, v, __ATOMIC_RELAXED, SCOPE); }
};

// The same for 16-bit words (signed_distance.hip: a pixel's kind and an 11-bit distance), at half the bytes per pixel: a 256 x 256 plane is
// 128 KiB and fits one workgroup's LDS.  Loads and stores only.
template <bool LDS, class I>
struct FrameHalves {
    unsigned short* h;
    static constexpr int SCOPE = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
    __device__ __forceinline__ unsigned ld(I i) const { return __hip_atomic_load(h + i, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void st(I i, unsigned v) const { __hip_atomic_store(h + i, (unsigned short)v, __ATOMIC_RELAXED, SCOPE); }
};

// The same for 64-bit words (surface_distance.hip in micrometres: an 11-bit row count beside a 45-bit squared distance), 8-byte aligned.
// Loads and stores only.
template <bool LDS, class I>
struct FrameWords64 {
    unsigned long long* w;
    static constexpr int SCOPE = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
    __device__ __forceinline__ unsigned long long ld(I i) const { return __hip_atomic_load(w + i, __ATOMIC_RELAXED, SCOPE); }
    __device__ __forceinline__ void st(I i, unsigned long long v) const { __hip_atomic_store(w + i, v, __ATOMIC_RELAXED, SCOPE); }
};

// The launchers' shared argument checks.  Each returns GDKVM_OK or gdkvm_fail(...) with the kernel's name in front of the message; `code`
// is the kernel's own code for that failure (lv_measure reports a bad cls and misaligned outputs as GDKVM_ERR_ARG, the others as
// GDKVM_ERR_SHAPE).
inline bool mask_shape_ok(int frames, int H, int W) { return frames >= 0 && H >= 1 && H <= 1024 && W >= 1 && W <= 1024; }
inline int mask_check_shape(const char* name, int frames, int H, int W)
{
    if (mask_shape_ok(frames, H, W)) return GDKVM_OK;
    return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: bad shape frames=%d H=%d W=%d (H, W in 1..1024)", name, frames, H, W);
}
inline int mask_check_cls(const char* name, int code, int cls)
{
    if (cls >= 0 && cls <= 254) return GDKVM_OK;
    return gdkvm_fail(code, "%s: cls=%d outside 0..254", name, cls);
}
// `what` names the outputs in the message; every pointer of `outs` must be 16-byte aligned
inline int mask_check_aligned16(const char* name, int code, const char* what, std::initializer_list<const void*> outs)
{
    for (const void* p : outs)
        if (!gdkvm_aligned16(p)) return gdkvm_fail(code, "%s: %s must be 16-byte aligned", name, what);
    return GDKVM_OK;
}
// need = the kernel's *_workspace_bytes for this shape (0: the LDS form, no workspace)
inline int mask_check_workspace(const char* name, int H, int W, size_t need, const void* workspace, size_t workspace_bytes)
{
    if (!need || (workspace && workspace_bytes >= need && gdkvm_aligned16(workspace))) return GDKVM_OK;
    return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: frames of %d x %d need a 16-byte aligned workspace of %zu bytes, got %zu", name, H, W, need,
                      workspace ? workspace_bytes : (size_t)0);
}
