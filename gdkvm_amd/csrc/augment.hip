// augment.hip -- gdkvm_augment_clips: the uint8 -> [0, 1] cast of a batch of training clips with an affine warp, an intensity table and
// the matching nearest-neighbour warp of the labels folded into the same pass (include/gdkvm.h has the semantics).  Element-wise with a
// gather: one thread owns V consecutive destination pixels of ONE frame (V = 8 with bf16 output, 4 with fp32: 16 bytes of output per
// plane), computes their source coordinates, bilinear weights and tap validity once, writes the labels, then loops over the C planes --
// 4 byte gathers through L1/L2 per pixel and plane (no LDS tile of the source: a rotated footprint has no fixed shape, and the source of
// a frame is H W bytes that the neighbouring threads share in cache), 4 reads of the clip's 256-entry intensity table in LDS, one store.
// The table (256 powf per workgroup instead of one per pixel and plane) is built by the workgroup's 256 threads; blockIdx.y is the frame,
// so a workgroup never spans two clips.  16-byte stores need every plane to start aligned: H W a multiple of V and aligned bases,
// otherwise the same code stores element by element.  Bound: bandwidth (1 byte in, 2 or 4 out per element); the kernel has no reuse to find.
#include "gdkvm_device.hpp"

namespace {

constexpr int WG = 256;

struct AugArgs {
    const uint8_t* frames; const void* target; const float* params; void* fout; void* tout;
    int T, C, H, W, HW, fill;
};

template <int TB> struct label_t;
template <> struct label_t<1> { typedef uint8_t type; };
template <> struct label_t<8> { typedef long long type; };

template <int IO, int TB, bool VEC>
__global__ __launch_bounds__(WG) void augment_kernel(AugArgs a)
{
    constexpr int V = IO == GDKVM_F32 ? 4 : 8;
    typedef typename label_t<TB>::type lab_t;
    __shared__ float s_lut[256];
    const int tid = threadIdx.x, bt = blockIdx.y;
    const float* pr = a.params + (size_t)(bt / a.T) * 12;               // (uniform: the row of this frame's clip)
    const float m00 = pr[0], m01 = pr[1], m02 = pr[2], m10 = pr[3], m11 = pr[4], m12 = pr[5];
    {
        const float gain = pr[6], bias = pr[7], gamma = pr[8];
        const float u = (float)tid * (1.0f / 255.0f);
        s_lut[tid] = fminf(fmaxf(fmaf(gain, gamma == 1.0f ? u : powf(u, gamma), bias), 0.0f), 1.0f);
    }
    __syncthreads();
    const int p0 = (blockIdx.x * WG + tid) * V;
    if (p0 >= a.HW) return;
    const int W = a.W, H = a.H;
    const float wmax = (float)(W - 1), hmax = (float)(H - 1);

    // per pixel: the offset of tap (y0, x0) inside a plane (meaningful where the tap is valid), the weights, 4 validity bits (a b c d)
    int base[V], ok[V];
    float fx[V], fy[V];
    lab_t lab[V];
    int y = p0 / W, x = p0 - y * W;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float xf = (float)x, yf = (float)y;
        const float sx = fmaf(m00, xf, fmaf(m01, yf, m02)), sy = fmaf(m10, xf, fmaf(m11, yf, m12));
        const float x0f = floorf(sx), y0f = floorf(sy);
        fx[j] = sx - x0f;
        fy[j] = sy - y0f;
        // comparisons in float (a NaN coordinate fails them all), the integer made from a value clamped to [-1, W] / [-1, H]
        const bool vx0 = x0f >= 0.0f && x0f <= wmax, vx1 = x0f >= -1.0f && x0f <= wmax - 1.0f;
        const bool vy0 = y0f >= 0.0f && y0f <= hmax, vy1 = y0f >= -1.0f && y0f <= hmax - 1.0f;
        const int x0 = (int)fminf(fmaxf(x0f, -1.0f), wmax + 1.0f), y0 = (int)fminf(fmaxf(y0f, -1.0f), hmax + 1.0f);
        base[j] = y0 * W + x0;
        ok[j] = (vy0 && vx0 ? 1 : 0) | (vy0 && vx1 ? 2 : 0) | (vy1 && vx0 ? 4 : 0) | (vy1 && vx1 ? 8 : 0);
        if (a.target) {
            const float ixf = floorf(sx + 0.5f), iyf = floorf(sy + 0.5f);
            const bool in = ixf >= 0.0f && ixf <= wmax && iyf >= 0.0f && iyf <= hmax;
            lab_t l = (lab_t)a.fill;
            if (in && (VEC || p0 + j < a.HW))
                l = static_cast<const lab_t*>(a.target)[(size_t)bt * a.HW + (size_t)((int)iyf * W + (int)ixf)];
            lab[j] = l;
        }
        if (++x == W) { x = 0; ++y; }
    }
    if (a.target) {
        lab_t* to = static_cast<lab_t*>(a.tout) + (size_t)bt * a.HW + p0;
        if constexpr (VEC && TB == 1) {
            unsigned w[V / 4];
#pragma unroll
            for (int j = 0; j < V; j += 4)
                w[j / 4] = (unsigned)lab[j] | ((unsigned)lab[j + 1] << 8) | ((unsigned)lab[j + 2] << 16) | ((unsigned)lab[j + 3] << 24);
            if constexpr (V == 8) *reinterpret_cast<uint2*>(to) = uint2{w[0], w[1]};
            else *reinterpret_cast<unsigned*>(to) = w[0];
        } else if constexpr (VEC) {
#pragma unroll
            for (int j = 0; j < V; j += 2) *reinterpret_cast<longlong2*>(to + j) = longlong2{lab[j], lab[j + 1]};
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (p0 + j < a.HW) to[j] = lab[j];
        }
    }

    for (int c = 0; c < a.C; ++c) {
        const size_t plane = ((size_t)bt * a.C + c) * a.HW;
        const uint8_t* src = a.frames + plane;
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const uint8_t* s = src + base[j];
            const float ta = (ok[j] & 1) ? s_lut[s[0]] : 0.0f, tb = (ok[j] & 2) ? s_lut[s[1]] : 0.0f;
            const float tc = (ok[j] & 4) ? s_lut[s[W]] : 0.0f, td = (ok[j] & 8) ? s_lut[s[W + 1]] : 0.0f;
            const float top = (1.0f - fx[j]) * ta + fx[j] * tb, bot = (1.0f - fx[j]) * tc + fx[j] * td;
            o[j] = (1.0f - fy[j]) * top + fy[j] * bot;
        }
        if constexpr (VEC && IO == GDKVM_F32) {
            *reinterpret_cast<f32x4*>(static_cast<float*>(a.fout) + plane + p0) = f32x4{o[0], o[1], o[2], o[3]};
        } else if constexpr (VEC) {
            uint4 u;
            u = pack_bf16x8(o);
            *reinterpret_cast<uint4*>(static_cast<bf16_t*>(a.fout) + plane + p0) = u;
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (p0 + j < a.HW) store1<IO>(a.fout, plane + p0 + j, o[j]);
        }
    }
}

template <int IO, int TB>
void launch(const AugArgs& a, bool vec, dim3 grid, hipStream_t st)
{
    if (vec) hipLaunchKernelGGL((augment_kernel<IO, TB, true>), grid, dim3(WG), 0, st, a);
    else hipLaunchKernelGGL((augment_kernel<IO, TB, false>), grid, dim3(WG), 0, st, a);
}

}  // namespace

extern "C" int gdkvm_augment_clips(const uint8_t* frames, const void* target, const float* params, void* frames_out, void* target_out,
                                   int B, int T, int C, int H, int W, int io_dtype, int target_bytes, int fill_label, void* stream)
{
    if (B < 0 || T < 0 || C <= 0 || H <= 0 || W <= 0)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "augment_clips: B=%d T=%d C=%d frame %dx%d", B, T, C, H, W);
    if (io_dtype != GDKVM_F32 && io_dtype != GDKVM_BF16) return gdkvm_fail(GDKVM_ERR_DTYPE, "augment_clips: io_dtype=%d", io_dtype);
    if (target_bytes != 1 && target_bytes != 8) return gdkvm_fail(GDKVM_ERR_DTYPE, "augment_clips: target_bytes=%d (1: uint8, 8: int64)", target_bytes);
    if (fill_label < 0 || fill_label > 255) return gdkvm_fail(GDKVM_ERR_ARG, "augment_clips: fill_label=%d outside [0, 255]", fill_label);
    // offsets inside a frame are ints: the C planes, a tap offset clamped to one row and one pixel outside a plane, the last tile's overhang
    if ((long long)H * W * C + 2LL * W + 2 + WG * 8 > 0x7fffffffLL)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "augment_clips: a frame of %d x %dx%d overflows the offset arithmetic", C, H, W);
    const long long BT = (long long)B * T;
    if (BT > 65535) return gdkvm_fail(GDKVM_ERR_SHAPE, "augment_clips: B * T = %lld frames exceed the grid's 65535", BT);
    if (BT == 0) return GDKVM_OK;
    if (!frames || !params || !frames_out) return gdkvm_fail(GDKVM_ERR_ARG, "augment_clips: null pointer");     // (frames: bytes, any alignment)
    if ((target == nullptr) != (target_out == nullptr)) return gdkvm_fail(GDKVM_ERR_ARG, "augment_clips: target and target_out go together");
    const uintptr_t esz = io_dtype == GDKVM_F32 ? 4 : 2;
    if (reinterpret_cast<uintptr_t>(params) % 4 || reinterpret_cast<uintptr_t>(frames_out) % esz ||
        reinterpret_cast<uintptr_t>(target) % (uintptr_t)target_bytes || reinterpret_cast<uintptr_t>(target_out) % (uintptr_t)target_bytes)
        return gdkvm_fail(GDKVM_ERR_ARG, "augment_clips: a pointer is not aligned to its element");
    if (int rc = gdkvm_check_device()) return rc;
    const int V = io_dtype == GDKVM_F32 ? 4 : 8, HW = H * W;
    const bool vec = HW % V == 0 && gdkvm_aligned16(frames_out) && (!target_out || gdkvm_aligned16(target_out));
    const dim3 grid((unsigned)((HW + WG * V - 1) / (WG * V)), (unsigned)BT);
    const AugArgs a{frames, target, params, frames_out, target_out, T, C, H, W, HW, fill_label};
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (io_dtype == GDKVM_F32) {
        if (target_bytes == 1) launch<GDKVM_F32, 1>(a, vec, grid, st);
        else launch<GDKVM_F32, 8>(a, vec, grid, st);
    } else {
        if (target_bytes == 1) launch<GDKVM_BF16, 1>(a, vec, grid, st);
        else launch<GDKVM_BF16, 8>(a, vec, grid, st);
    }
    GDKVM_LAUNCH_CHECK("augment_clips");
    return GDKVM_OK;
}
