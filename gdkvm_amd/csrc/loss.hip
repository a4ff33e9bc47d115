// loss.hip -- the training objective on the decoder's stride-4 logits without materialising full-resolution logits
// (the training twin of upsample_argmax_dice_kernel):
//     l = bilinear_upsample(z -> H x W, align_corners = false)          (fp32, PyTorch's source-index formula)
//     loss = mean_pixels CE(l, t) + dice_weight * (1 - mean_c (2 I_c + eps) / (P_c + O_c + eps))
//     with p = softmax(l),  I_c = sum p_c [t = c],  P_c = sum p_c,  O_c = sum [t = c]   (sums over the whole batch)
// In a cfg4 training step PyTorch spends ~0.75 ms on this chain (a 51 MB fp32 logit tensor written by an NCHW upsample kernel,
// log-softmax + softmax + one-hot + reductions and their backward).  Here: one pass over the pixels producing per-workgroup
// partial sums, a one-workgroup finalize (loss + the per-class coefficients of the backward), and a backward that is a
// GATHER per stride-4 pixel over its bilinear footprint, recomputing softmax on the fly -- deterministic, no atomics.
// The boundary form (gdkvm_seg_loss_boundary_fwd / _bwd) is the same three kernels with one more operand, the signed squared distance maps
// sd2 [images, C, H, W] of signed_distance.hip, and one more partial sum:  L_B = (1 / labelled) sum_x sum_{c in K} p_c(x) phi_c(x), linear in p
// like the Dice sums, so its gradient is one more summand of u_c in the backward.  Each kernel takes the extra operands as ONE trailing
// argument of a type that says whether they exist (NoBoundary: empty; Boundary / BoundaryWeight): with NoBoundary the kernels are, instruction
// for instruction, the ones gdkvm_seg_loss_fwd / _bwd ran before the boundary form existed (tools/isa_equal.py --kernels).
#include <type_traits>

#include "gdkvm_common.hpp"

namespace {

constexpr int LOSS_MAX_PART = 2048;
constexpr int LOSS_MAXC = 8;

struct Taps { int i0, i1; float l; };
__device__ __forceinline__ Taps taps_of(int o, float s, int n_in)
{
    const float f = fmaxf(s * ((float)o + 0.5f) - 0.5f, 0.f);
    Taps t;
    t.i0 = (int)f; t.i1 = min(t.i0 + 1, n_in - 1); t.l = f - (float)t.i0;
    return t;
}

// softmax of the upsampled logits of one pixel; returns log(sum exp) + max
template <int IO, int C>
__device__ __forceinline__ float pixel_softmax(const void* z, size_t img, int hw, int w, const Taps& ty, const Taps& tx, float (&p)[C],
                                               float (&lg)[C])
{
    const float hy = 1.f - ty.l, hx = 1.f - tx.l;
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const size_t pl = img + (size_t)c * hw;
        const float a = load1<IO>(z, pl + ty.i0 * w + tx.i0), b = load1<IO>(z, pl + ty.i0 * w + tx.i1);
        const float d = load1<IO>(z, pl + ty.i1 * w + tx.i0), e = load1<IO>(z, pl + ty.i1 * w + tx.i1);
        lg[c] = hy * (hx * a + tx.l * b) + ty.l * (hx * d + tx.l * e);
        m = fmaxf(m, lg[c]);
    }
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) { p[c] = expf(lg[c] - m); s += p[c]; }
    const float inv = 1.f / s;
#pragma unroll
    for (int c = 0; c < C; ++c) p[c] *= inv;
    return m + logf(s);
}

template <int TL>
__device__ __forceinline__ int target_at(const void* t, size_t i)
{
    if constexpr (TL == 8) return (int)static_cast<const long long*>(t)[i];
    else return (int)static_cast<const unsigned char*>(t)[i];
}

// the extra operands of the boundary form
struct NoBoundary { static constexpr bool ON = false; };
struct Boundary { static constexpr bool ON = true; const int* sd2; unsigned class_mask; };
struct BoundaryWeight { static constexpr bool ON = true; float weight; };

// the signed distance of the boundary loss from the signed squared distance: +sqrt(s) outside the class, -(sqrt(-s) - 1) inside, 0 at 0
__device__ __forceinline__ float phi_of(int s)
{
    return s > 0 ? sqrtf((float)s) : s < 0 ? 1.f - sqrtf((float)-s) : 0.f;
}

// part[block][1 + 3C (+ 1)]: ce sum, then I_c, P_c, O_c (boundary form: then the boundary sum)
template <int IO, int C, int TL, class BX>
__global__ __launch_bounds__(256) void seg_loss_fwd_kernel(const void* z, const void* target, float* part,
                                                           int NI, int h, int w, int H, int W, float sy, float sx, BX bx)
{
    constexpr int NV = 1 + 3 * C + (BX::ON ? 1 : 0);
    float acc[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] = 0.f;
    const size_t total = (size_t)NI * H * W;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int x = (int)(i % W);
        const size_t r = i / W;
        const int y = (int)(r % H), n = (int)(r / H);
        const Taps ty = taps_of(y, sy, h), tx = taps_of(x, sx, w);
        float p[C], lg[C];
        const float lse = pixel_softmax<IO, C>(z, (size_t)n * C * h * w, h * w, w, ty, tx, p, lg);
        const int t = target_at<TL>(target, i);
        const float lab = (unsigned)t < (unsigned)C ? 1.f : 0.f;        // an unlabelled pixel (EchoNet: every untraced frame) adds to NO sum
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float is = t == c ? 1.f : 0.f;
            acc[0] += is * (lse - lg[c]);
            acc[1 + c] += is * p[c];
            acc[1 + C + c] += lab * p[c];
            acc[1 + 2 * C + c] += is;
        }
        if constexpr (BX::ON) {
            if (lab != 0.f) {                                           // (the planes of classes outside class_mask are never read)
                const size_t px = (size_t)n * C * H * W + (size_t)y * W + x;
                float bs = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c)
                    if ((bx.class_mask >> c) & 1u) bs = fmaf(p[c], phi_of(bx.sd2[px + (size_t)c * H * W]), bs);
                acc[3 * C + 1] += bs;
            }
        }
    }
    __shared__ float s[4][NV];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        float v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == 0) s[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < NV) part[(size_t)blockIdx.x * NV + threadIdx.x] = s[0][threadIdx.x] + s[1][threadIdx.x] + s[2][threadIdx.x] + s[3][threadIdx.x];
}

// out[0] = loss, out[1] = CE, out[2] = Dice term;  coef[0..C) = dLoss/dI_c, coef[C..2C) = dLoss/dP_c, coef[2C] = 1 / pixels
// boundary form: out[3] = L_B, out[0] includes weight * L_B, coef[2C + 1] = weight / pixels
template <class BX>
__global__ __launch_bounds__(256) void seg_loss_finalize_kernel(const float* part, int nblk, int C, double npix, float dice_weight,
                                                                float eps, float* out, float* coef, BX bx)
{
    __shared__ double s[256];
    __shared__ double tot[1 + 3 * LOSS_MAXC + (BX::ON ? 1 : 0)];
    const int NV = 1 + 3 * C + (BX::ON ? 1 : 0);
    for (int k = 0; k < NV; ++k) {
        double a = 0.0;
        for (int b = threadIdx.x; b < nblk; b += 256) a += (double)part[(size_t)b * NV + k];
        s[threadIdx.x] = a;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0) tot[k] = s[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        // labels outside [0, C) carry no class: the cross-entropy averages over the labelled pixels only (ignore_index semantics)
        double labelled = 0.0;
        for (int c = 0; c < C; ++c) labelled += tot[1 + 2 * C + c];
        npix = labelled > 0.0 ? labelled : 1.0;
        const double ce = tot[0] / npix;
        double dsum = 0.0;
        for (int c = 0; c < C; ++c) {
            const double I = tot[1 + c], D = tot[1 + C + c] + tot[1 + 2 * C + c] + (double)eps;
            dsum += (2.0 * I + (double)eps) / D;
            coef[c] = (float)(-(double)dice_weight / C * 2.0 / D);
            coef[C + c] = (float)((double)dice_weight / C * (2.0 * I + (double)eps) / (D * D));
        }
        const double dice = 1.0 - dsum / C;
        coef[2 * C] = (float)(1.0 / npix);
        if constexpr (BX::ON) {
            const double lb = tot[1 + 3 * C] / npix;
            coef[2 * C + 1] = (float)((double)bx.weight / npix);
            out[0] = (float)(ce + (double)dice_weight * dice + (double)bx.weight * lb); out[1] = (float)ce; out[2] = (float)dice;
            out[3] = (float)lb;
        } else {
            out[0] = (float)(ce + (double)dice_weight * dice); out[1] = (float)ce; out[2] = (float)dice;
        }
    }
}

// dz[n, c, i, j] = gout * sum over the pixels (y, x) whose taps touch (i, j) of  wy wx dL/dl_c(y, x),
//   dL/dl_c = (p_c - [t = c]) / pixels + p_c (u_c - sum_k p_k u_k),   u_c = coefI_c [t = c] + coefP_c  (boundary form: + coefB phi_c for c in K).
template <int IO, int C, int TL, class BX>
__global__ __launch_bounds__(256) void seg_loss_bwd_kernel(const void* z, const void* target, const float* coef, const float* gout,
                                                           void* dz, int NI, int h, int w, int H, int W, float sy, float sx, BX bx)
{
    const size_t total = (size_t)NI * h * w;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int j = (int)(i % w);
    const size_t r = i / w;
    const int ii = (int)(r % h), n = (int)(r / h);
    float cI[C], cP[C], acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { cI[c] = coef[c]; cP[c] = coef[C + c]; acc[c] = 0.f; }
    const float inv_n = coef[2 * C];
    float cB = 0.f;
    if constexpr (BX::ON) cB = coef[2 * C + 1];
    const int y0 = max((int)(((float)ii - 0.5f) / sy - 0.5f) - 1, 0), y1 = min((int)(((float)ii + 1.5f) / sy - 0.5f) + 1, H - 1);
    const int x0 = max((int)(((float)j - 0.5f) / sx - 0.5f) - 1, 0), x1 = min((int)(((float)j + 1.5f) / sx - 0.5f) + 1, W - 1);
    const size_t img = (size_t)n * C * h * w;
    auto pixel = [&](int y, int x, const Taps& ty, const Taps& tx, float wgt) __attribute__((always_inline)) {
        float p[C], lg[C];
        pixel_softmax<IO, C>(z, img, h * w, w, ty, tx, p, lg);
        const int t = target_at<TL>(target, ((size_t)n * H + y) * W + x);
        float u[C], dot = 0.f;
        const bool lab = (unsigned)t < (unsigned)C;
        const float ce_w = lab ? inv_n : 0.f;                         // unlabelled pixel: no cross-entropy term, and no Dice term either
#pragma unroll
        for (int c = 0; c < C; ++c) {
            u[c] = lab ? (t == c ? cI[c] : 0.f) + cP[c] : 0.f;
            if constexpr (BX::ON) {
                if (lab && ((bx.class_mask >> c) & 1u)) u[c] = fmaf(cB, phi_of(bx.sd2[((size_t)n * C + c) * H * W + (size_t)y * W + x]), u[c]);
            }
            dot = fmaf(p[c], u[c], dot);
        }
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float dl = (p[c] - (t == c ? 1.f : 0.f)) * ce_w + p[c] * (u[c] - dot);
            acc[c] = fmaf(wgt, dl, acc[c]);
        }
    };
    if (H == 4 * h && W == 4 * w) {
        // exactly 4x (EchoNet 28 -> 112, CAMUS 64 -> 256): the footprint is rows 4i-2 .. 4i+5 and columns 4j-2 .. 4j+5; a fixed
        // 8-wide column loop puts the eight pixels' loads in flight together (the general loop below is one dependent chain
        // per pixel: 118 us per cfg4 step against 0.4 M threads x 64 pixels of arithmetic)
        for (int a = 0; a < 8; ++a) {
            const int y = 4 * ii - 2 + a;
            if (y < 0 || y >= H) continue;
            const Taps ty = taps_of(y, sy, h);
            const float wy = (ty.i0 == ii ? 1.f - ty.l : 0.f) + (ty.i1 == ii ? ty.l : 0.f);
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int xr = 4 * j - 2 + b, x = min(max(xr, 0), W - 1);
                const Taps tx = taps_of(x, sx, w);
                const float wx = (tx.i0 == j ? 1.f - tx.l : 0.f) + (tx.i1 == j ? tx.l : 0.f);
                pixel(y, x, ty, tx, xr == x ? wy * wx : 0.f);
            }
        }
    } else
    for (int y = y0; y <= y1; ++y) {
        const Taps ty = taps_of(y, sy, h);
        const float wy = (ty.i0 == ii ? 1.f - ty.l : 0.f) + (ty.i1 == ii ? ty.l : 0.f);
        if (wy == 0.f) continue;
        for (int x = x0; x <= x1; ++x) {
            const Taps tx = taps_of(x, sx, w);
            const float wgt = wy * ((tx.i0 == j ? 1.f - tx.l : 0.f) + (tx.i1 == j ? tx.l : 0.f));
            if (wgt == 0.f) continue;
            pixel(y, x, ty, tx, wgt);
        }
    }
    const float g = gout ? gout[0] : 1.f;
#pragma unroll
    for (int c = 0; c < C; ++c) store1<IO>(dz, img + (size_t)c * h * w + (size_t)ii * w + j, g * acc[c]);
}

int loss_check(const char* who, int NI, int C, int h, int w, int H, int W, int io, int tl)
{
    if (NI <= 0 || C < 2 || C > LOSS_MAXC || h <= 0 || w <= 0 || H <= 0 || W <= 0)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: images=%d classes=%d (2..%d) %dx%d -> %dx%d", who, NI, C, LOSS_MAXC, h, w, H, W);
    if (io != GDKVM_F32 && io != GDKVM_BF16) return gdkvm_fail(GDKVM_ERR_DTYPE, "%s: io_dtype=%d", who, io);
    if (tl != 1 && tl != 8) return gdkvm_fail(GDKVM_ERR_DTYPE, "%s: target_bytes=%d (1 = uint8, 8 = int64)", who, tl);
    return gdkvm_check_device();
}

template <class F>
int dispatch_c(int C, F&& f)
{
    switch (C) {
        case 2: f(std::integral_constant<int, 2>{}); return 1;
        case 3: f(std::integral_constant<int, 3>{}); return 1;
        case 4: f(std::integral_constant<int, 4>{}); return 1;
        case 5: f(std::integral_constant<int, 5>{}); return 1;
        case 6: f(std::integral_constant<int, 6>{}); return 1;
        case 7: f(std::integral_constant<int, 7>{}); return 1;
        case 8: f(std::integral_constant<int, 8>{}); return 1;
    }
    return 0;
}

size_t loss_ws_bytes(int C, bool bd)
{
    return C > 0 ? ((size_t)LOSS_MAX_PART * (1 + 3 * C + (bd ? 1 : 0)) + 2 * (size_t)C + 4) * sizeof(float) : 0;
}

bool loss_class_mask_ok(int C, unsigned class_mask) { return !(class_mask >> C); }         // (C <= LOSS_MAXC = 8: the shift is defined)

template <bool BD>
int loss_fwd(const char* who, const void* z, const void* target, const int* sd2, float* out, void* ws, size_t ws_bytes,
             int NI, int C, int h, int w, int H, int W, float dice_weight, float eps, float boundary_weight, unsigned class_mask,
             int io_dtype, int target_bytes, void* stream)
{
    if (int rc = loss_check(who, NI, C, h, w, H, W, io_dtype, target_bytes)) return rc;
    if (!z || !target || !out || !ws || (BD && !sd2)) return gdkvm_fail(GDKVM_ERR_ARG, "%s: null pointer", who);
    if (ws_bytes < loss_ws_bytes(C, BD)) return gdkvm_fail(GDKVM_ERR_ARG, "%s: workspace too small", who);
    if (BD && !loss_class_mask_ok(C, class_mask)) return gdkvm_fail(GDKVM_ERR_ARG, "%s: class_mask 0x%x names a class outside 0..%d", who, class_mask, C - 1);
    if (BD && !(boundary_weight >= 0.f && boundary_weight <= 3.0e38f)) return gdkvm_fail(GDKVM_ERR_ARG, "%s: boundary_weight must be finite and >= 0", who);
    using BX = std::conditional_t<BD, Boundary, NoBoundary>;
    using BW = std::conditional_t<BD, BoundaryWeight, NoBoundary>;
    BX bx{};
    BW bw{};
    if constexpr (BD) { bx.sd2 = sd2; bx.class_mask = class_mask; bw.weight = boundary_weight; }
    const size_t total = (size_t)NI * H * W;
    size_t blocks = (total + 255) / 256;
    if (blocks > LOSS_MAX_PART) blocks = LOSS_MAX_PART;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(ws);
    float* coef = part + (size_t)LOSS_MAX_PART * (1 + 3 * C + (BD ? 1 : 0));
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    dispatch_c(C, [&](auto Cc) {
        constexpr int CC = decltype(Cc)::value;
#define GDKVM_LF(IO, TL) hipLaunchKernelGGL((seg_loss_fwd_kernel<IO, CC, TL, BX>), dim3((unsigned)blocks), dim3(256), 0, st, z, target, part, NI, h, w, H, W, sy, sx, bx)
        if (io_dtype == GDKVM_F32) { if (target_bytes == 8) GDKVM_LF(GDKVM_F32, 8); else GDKVM_LF(GDKVM_F32, 1); }
        else { if (target_bytes == 8) GDKVM_LF(GDKVM_BF16, 8); else GDKVM_LF(GDKVM_BF16, 1); }
#undef GDKVM_LF
    });
    GDKVM_LAUNCH_CHECK("seg_loss_fwd_kernel");
    hipLaunchKernelGGL(seg_loss_finalize_kernel<BW>, dim3(1), dim3(256), 0, st, part, (int)blocks, C, (double)total, dice_weight, eps, out, coef, bw);
    GDKVM_LAUNCH_CHECK("seg_loss_finalize_kernel");
    return GDKVM_OK;
}

template <bool BD>
int loss_bwd(const char* who, const void* z, const void* target, const int* sd2, const void* ws, size_t ws_bytes, const float* grad_out, void* dz,
             int NI, int C, int h, int w, int H, int W, unsigned class_mask, int io_dtype, int target_bytes, void* stream)
{
    if (int rc = loss_check(who, NI, C, h, w, H, W, io_dtype, target_bytes)) return rc;
    if (!z || !target || !dz || !ws || (BD && !sd2)) return gdkvm_fail(GDKVM_ERR_ARG, "%s: null pointer", who);
    if (ws_bytes < loss_ws_bytes(C, BD)) return gdkvm_fail(GDKVM_ERR_ARG, "%s: workspace too small", who);
    if (BD && !loss_class_mask_ok(C, class_mask)) return gdkvm_fail(GDKVM_ERR_ARG, "%s: class_mask 0x%x names a class outside 0..%d", who, class_mask, C - 1);
    using BX = std::conditional_t<BD, Boundary, NoBoundary>;
    BX bx{};
    if constexpr (BD) { bx.sd2 = sd2; bx.class_mask = class_mask; }
    const size_t total = (size_t)NI * h * w;
    const size_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffu) return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: too many pixels", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const float* coef = static_cast<const float*>(ws) + (size_t)LOSS_MAX_PART * (1 + 3 * C + (BD ? 1 : 0));
    const float sy = (float)h / (float)H, sx = (float)w / (float)W;
    dispatch_c(C, [&](auto Cc) {
        constexpr int CC = decltype(Cc)::value;
#define GDKVM_LB(IO, TL) hipLaunchKernelGGL((seg_loss_bwd_kernel<IO, CC, TL, BX>), dim3((unsigned)blocks), dim3(256), 0, st, z, target, coef, grad_out, dz, NI, h, w, H, W, sy, sx, bx)
        if (io_dtype == GDKVM_F32) { if (target_bytes == 8) GDKVM_LB(GDKVM_F32, 8); else GDKVM_LB(GDKVM_F32, 1); }
        else { if (target_bytes == 8) GDKVM_LB(GDKVM_BF16, 8); else GDKVM_LB(GDKVM_BF16, 1); }
#undef GDKVM_LB
    });
    GDKVM_LAUNCH_CHECK("seg_loss_bwd_kernel");
    return GDKVM_OK;
}

}  // namespace

extern "C" size_t gdkvm_seg_loss_workspace_bytes(int C) { return loss_ws_bytes(C, false); }

extern "C" int gdkvm_seg_loss_fwd(const void* z, const void* target, float* out, void* ws, size_t ws_bytes,
                                  int NI, int C, int h, int w, int H, int W, float dice_weight, float eps,
                                  int io_dtype, int target_bytes, void* stream)
{
    return loss_fwd<false>("seg_loss_fwd", z, target, nullptr, out, ws, ws_bytes, NI, C, h, w, H, W, dice_weight, eps, 0.f, 0u, io_dtype,
                           target_bytes, stream);
}

extern "C" int gdkvm_seg_loss_bwd(const void* z, const void* target, const void* ws, size_t ws_bytes, const float* grad_out, void* dz,
                                  int NI, int C, int h, int w, int H, int W, int io_dtype, int target_bytes, void* stream)
{
    return loss_bwd<false>("seg_loss_bwd", z, target, nullptr, ws, ws_bytes, grad_out, dz, NI, C, h, w, H, W, 0u, io_dtype, target_bytes, stream);
}

extern "C" size_t gdkvm_seg_loss_boundary_workspace_bytes(int C) { return loss_ws_bytes(C, true); }

extern "C" int gdkvm_seg_loss_boundary_fwd(const void* z, const void* target, const int32_t* sd2, float* out, void* ws, size_t ws_bytes,
                                           int NI, int C, int h, int w, int H, int W, float dice_weight, float eps, float boundary_weight,
                                           unsigned class_mask, int io_dtype, int target_bytes, void* stream)
{
    return loss_fwd<true>("seg_loss_boundary_fwd", z, target, sd2, out, ws, ws_bytes, NI, C, h, w, H, W, dice_weight, eps, boundary_weight,
                          class_mask, io_dtype, target_bytes, stream);
}

extern "C" int gdkvm_seg_loss_boundary_bwd(const void* z, const void* target, const int32_t* sd2, const void* ws, size_t ws_bytes,
                                           const float* grad_out, void* dz, int NI, int C, int h, int w, int H, int W, unsigned class_mask,
                                           int io_dtype, int target_bytes, void* stream)
{
    return loss_bwd<true>("seg_loss_boundary_bwd", z, target, sd2, ws, ws_bytes, grad_out, dz, NI, C, h, w, H, W, class_mask, io_dtype,
                          target_bytes, stream);
}
