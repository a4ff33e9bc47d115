// gdkvm_device.hpp -- the small device idioms the hand-written kernels share: compile-time loops, the reciprocal index division, bf16
// pair packing and unpacking, buffer descriptors and LDS-DMA plumbing.  Device-only, not part of the C ABI.
//
// Why a header of its own and not more of gdkvm_common.hpp: build.source_hash() covers gdkvm_common.hpp, gdr_device.hpp, gdr_ws.hpp,
// gdr_prep.hip and gdr_scan.hip, and bench.py quotes the committed PMC summaries of the scan kernels only while that hash matches -- those
// five files stay byte for byte as they were measured.  For the same reason gdr_device.hpp keeps its own static_for: the scan sources
// include that header, everything else includes this one, and no translation unit includes both.
//
// Every helper is __forceinline__ and written with the exact expression the kernels used before they shared it, so that a kernel moved
// onto it compiles to the same instructions: tools/isa_equal.py compares the gfx950 assembly of every .hip against a git revision.
#pragma once
#include <type_traits>

#include "gdkvm_common.hpp"

typedef float f32x2 __attribute__((ext_vector_type(2)));       // packed fp32 pairs: v_pk_add_f32 / v_pk_max_f32
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));    // the 16 bytes of a buffer_load / buffer_store_dwordx4

// f(integral_constant<int, I>), ..., f(integral_constant<int, E - 1>): a loop whose index is a compile-time constant in the body (register
// arrays with static indices, immediates of asm operands).  Needs I <= E.
template <int I, int E, class F>
__device__ __forceinline__ void static_for(F&& f)
{
    if constexpr (I < E) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, E>(f);
    }
}

// floor(n / d) with inv = 1.0f / d, for the kernels' small non-negative indices: exact while 0 <= n < 2^16 and 0 < d < 2^16 (the launchers
// keep tile and band indices there), and 3 instructions where an integer division is ~40 -- the convolutions' prologues and epilogues do
// dozens per lane (17 % of a 128 -> 128 layer before it).
__device__ __forceinline__ int idx_div(int n, float inv) { return (int)(((float)n + 0.5f) * inv); }

// Two fp32 -> one 32-bit word of two bf16 (a in the low half), each rounded to nearest even like f32_to_bf16.  Any float, NaN included.
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) { return (unsigned)f32_to_bf16(a) | ((unsigned)f32_to_bf16(b) << 16); }
__device__ __forceinline__ uint2 pack_bf16x4(const f32x4& v) { return make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])); }
__device__ __forceinline__ uint4 pack_bf16x8(const float (&v)[8])
{
    uint4 o;
    o.x = pack_bf16x2(v[0], v[1]);
    o.y = pack_bf16x2(v[2], v[3]);
    o.z = pack_bf16x2(v[4], v[5]);
    o.w = pack_bf16x2(v[6], v[7]);
    return o;
}

// The two bf16 of a 32-bit word widened to fp32 (exact): the low half, the high half, both, and the four / eight of a uint2 / uint4 in
// memory order.  u is any bit pattern.
__device__ __forceinline__ float bf16_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __uint_as_float(u & 0xffff0000u); }
__device__ __forceinline__ f32x2 unpack_bf16x2(unsigned u) { return f32x2{bf16_lo(u), bf16_hi(u)}; }
__device__ __forceinline__ f32x4 unpack_bf16x4(uint2 u) { return f32x4{bf16_lo(u.x), bf16_hi(u.x), bf16_lo(u.y), bf16_hi(u.y)}; }
__device__ __forceinline__ void unpack_bf16x8(const uint4& u, float (&v)[8])
{
    const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) { v[2 * j] = bf16_lo(w[j]); v[2 * j + 1] = bf16_hi(w[j]); }
}

// An LDS pointer (or LDS byte address) as the destination operand of the LDS-DMA builtins (global_load_lds, raw_ptr_buffer_load_lds).
// p must point into __shared__ memory: only the low 32 bits of the generic address survive.
// In a kernel TEMPLATE, hand it a pointer whose type does not depend on a template parameter (cast a __shared__ array that is sized by
// one first): with a type-dependent argument the host pass fails, without a word, to emit the kernel's launch stub, and the library
// no longer loads (undefined __device_stub__ symbol).
typedef __attribute__((address_space(3))) void* lds_dst_t;
__device__ __forceinline__ lds_dst_t lds_dma_dst(const void* p) { return reinterpret_cast<lds_dst_t>(reinterpret_cast<uintptr_t>(p)); }
__device__ __forceinline__ lds_dst_t lds_dma_dst(unsigned addr) { return reinterpret_cast<lds_dst_t>(static_cast<uintptr_t>(addr)); }

// Raw buffer descriptor over `bytes` bytes at p (stride 0: offsets are bytes, and an offset >= bytes reads as zero / drops the store).
// RSRC_WORD3 is the descriptor's fourth dword: DATA_FORMAT = 32 (bits 12-18), the one setting gfx9 raw buffer accesses need; everything
// else -- swizzle, index stride, add-tid -- off.  p and bytes must be wave-uniform (the descriptor lives in SGPRs) and bytes < 2^31.
constexpr int RSRC_WORD3 = 0x00020000;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const void* p, int bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, bytes, RSRC_WORD3);
}
// A byte offset that is out of range of every descriptor the kernels make, whatever in-range scalar is added to it: the hardware answers
// it with zeros.  Holds because the launchers keep everything one descriptor addresses (frame or frame group, halo rows included) below
// 2^31 bytes, so offset + scalar stays in [2^31, 2^32).
constexpr unsigned RSRC_DEAD = 0x80000000u;

// A 2 x 2 block of output vectors (8 channels, 16 bytes each) of the exact-2x bilinear enlargement (align_corners = false): the output
// rows 2 ip + 1, 2 ip + 2 and columns 2 jp + 1, 2 jp + 2 share the four source taps a, b (row ip: columns jp, jp + 1) and c, d (row
// ip + 1), as in upsample_cat_bf16_2x_kernel (epilogue.hip).  o[ey][e] = hy[ey] (hx a + lx b) + ly[ey] (hx c + lx d) with (hx, lx) =
// (3/4, 1/4) for e = 0 and (1/4, 3/4) for e = 1, rounded by pack_bf16x2; hy + ly = 1 are the caller's row weights (1/4 and 3/4 inside,
// 1 / 0 on output row 0).  Each value goes through EXACTLY the multiply / fused-multiply-add sequence that kernel compiles to for gfx950,
// which is not the same for every channel: its pairs of packed fp32 instructions take channels 0, 1, 4, 5 of a vector with the products
// hx a, hx c and hy top rounded on their own and the other three terms inside the fused operations, and channels 2, 3, 6, 7 the other
// way round.  The horizontal products are exact either way (an 8-bit significand times 1/4 or 3/4); the vertical ones are not, so a
// consumer that must reproduce that kernel's bits (the convolution that builds the enlarged feature in its LDS band, conv3x3_tile.hip)
// has to round where it rounds.  Contraction is off in here: every rounding is the one written.
__device__ __forceinline__ void bilerp2x_bf16x8(const u32x4& a, const u32x4& b, const u32x4& c, const u32x4& d,
                                                const float (&hy)[2], const float (&ly)[2], u32x4 (&o)[2][2])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float v[2][2][2];                                  // [ey][e][half]
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float A = h ? bf16_hi(a[q]) : bf16_lo(a[q]), B = h ? bf16_hi(b[q]) : bf16_lo(b[q]);
            const float C = h ? bf16_hi(c[q]) : bf16_lo(c[q]), D = h ? bf16_hi(d[q]) : bf16_lo(d[q]);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const float lx = e ? 0.75f : 0.25f, hx = e ? 0.25f : 0.75f;
                if (q & 1) {
                    const float top = __fmaf_rn(hx, A, __fmul_rn(lx, B)), bot = __fmaf_rn(hx, C, __fmul_rn(lx, D));
#pragma unroll
                    for (int ey = 0; ey < 2; ++ey) v[ey][e][h] = __fmaf_rn(hy[ey], top, __fmul_rn(ly[ey], bot));
                } else {
                    const float top = __fmaf_rn(lx, B, __fmul_rn(hx, A)), bot = __fmaf_rn(lx, D, __fmul_rn(hx, C));
#pragma unroll
                    for (int ey = 0; ey < 2; ++ey) v[ey][e][h] = __fmaf_rn(ly[ey], bot, __fmul_rn(hy[ey], top));
                }
            }
        }
#pragma unroll
        for (int ey = 0; ey < 2; ++ey)
#pragma unroll
            for (int e = 0; e < 2; ++e) o[ey][e][q] = pack_bf16x2(v[ey][e][0], v[ey][e][1]);
    }
}
