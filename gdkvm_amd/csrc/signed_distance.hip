// signed_distance.hip -- the signed squared Euclidean distance of every pixel to the contour of every class of a uint8 label frame, on the
// device (the operand of the boundary loss, loss.hip; include/gdkvm.h holds the definition).  Every output is an integer that depends on
// neither the algorithm nor the schedule.
//
// ONE workgroup of 1024 lanes per (frame, class): no cross-workgroup synchronisation, no fences between workgroups, no flag anybody spins
// on.  A (frame, class) keeps ONE 16-bit word per pixel: bit 15 = the pixel's kind (1: of the class), bits 0..10 = g, the vertical distance to
// the nearest pixel of the OTHER kind in its column (1..1023, or NONE when the column has none).  Both signs come out of the one plane: a
// pixel's distance is to the other kind whichever kind it is of.  The plane lives in dynamic LDS while the frame has at most SDM_LDS_PIX pixels
// (156 KiB of the workgroup's 160 KiB; a 256 x 256 frame takes 128 KiB), otherwise in the (frame, class) slice of the caller's workspace,
// where every access is an agent-scope relaxed atomic (served by L2, as in surface_distance.hip).
// Passes, a workgroup barrier between them:
//   1. the plane is cleared.       2. the kinds from the bytes (head / 16-byte vectors / tail) and their count n.  n == 0 or n == H W: the
//                                     class is absent or fills the frame, the output plane is zero and the workgroup ends here.
//   3. columns  one lane per column sweeps down, then up, carrying the distance to the last pixel of either kind: g.
//   4. rows     one lane per pixel: best = min over x' of (x - x')^2 where the pixel at x' is of the other kind, (x - x')^2 + g[y][x']^2
//               otherwise, walking outwards from x (four steps to either side at a time) and stopping once (x - x')^2 reaches the best so
//               far; the output is +best for a pixel outside the class and -best inside.
// Loop bounds: the sweeps count to H, the walks to W, the strided loops to H W / lanes.

#include "mask_frame.hpp"

#include <atomic>

namespace {

constexpr int SDM_NT = 1024;
constexpr int SDM_LDS_PIX = 79872;             // frames of up to this many pixels live in LDS: 2 * 79872 = 159744 bytes
constexpr unsigned SDM_NONE = 0x7ffu;          // g of a column without a pixel of the other kind (NONE^2 is above every real distance)
constexpr unsigned SDM_IN = 0x8000u;           // the pixel is of the class
constexpr int SDM_BATCH = 8;                   // words a column sweep loads before it needs the first (the sweep is a chain of LDS latencies)
constexpr int SDM_WALK = 4;                    // steps a row walk takes at a time, to either side: 8 loads in flight
constexpr int SDM_MAXC = 32;                   // class_mask is 32 bits

struct SdmArgs {
    const uint8_t* target; int* sd2; unsigned short* ws;
    int C, H, W, HW;
    unsigned stride, class_mask;
};

// 16-bit words of one (frame, class) in the workspace, rounded up to 128 bytes, so that no two planes share a cache line
inline size_t sdm_stride(int H, int W) { return ((size_t)H * W + 63) & ~(size_t)63; }

template <bool LDS>
__global__ __launch_bounds__(SDM_NT) void signed_distance_kernel(SdmArgs a)
{
    constexpr int NT = SDM_NT, NW = NT / 64;
    extern __shared__ uint4 sdm_plane[];
    __shared__ unsigned s_n[NW][1];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, H = a.H, W = a.W, HW = a.HW;
    const size_t b = blockIdx.x;
    const int f = (int)(b / (unsigned)a.C), c = (int)(b - (size_t)f * a.C);
    int* out = a.sd2 + b * (size_t)HW;
    if (!((a.class_mask >> c) & 1u)) {                     // (uniform) a class nobody asked for: its plane is zero
        for (int p = tid; p < HW; p += NT) out[p] = 0;
        return;
    }
    FrameHalves<LDS, int> M;
    if constexpr (LDS) M.h = reinterpret_cast<unsigned short*>(sdm_plane);
    else M.h = a.ws + b * (size_t)a.stride;

    // pass 1, 2: the kinds
    for (int p = tid; p < HW; p += NT) M.st(p, 0u);
    __syncthreads();
    unsigned n = 0;
    MaskFrame<NT>(a.target + (size_t)f * HW, HW, W, (unsigned)c).sweep_bits([&](unsigned m, int p0) {
        n += (unsigned)__builtin_popcount(m);
        visit_p(m, p0, [&](int p) { M.st(p, SDM_IN); });
    });
    n = wave_sum(n);
    if (lane == 0) s_n[wv][0] = n;
    __syncthreads();
    n = wg_sum(s_n, 0);
    if (n == 0 || n == (unsigned)HW) {                     // (uniform) no contour
        for (int p = tid; p < HW; p += NT) out[p] = 0;
        return;
    }

    // pass 3: columns.  dI / dO = the distance to the last pixel inside / outside the class met so far (NONE: none yet; d <= H - 1 < NONE)
    for (int x = tid; x < W; x += NT) {
        unsigned dI = SDM_NONE, dO = SDM_NONE;
        for (int y0 = 0; y0 < H; y0 += SDM_BATCH) {
            unsigned k[SDM_BATCH];
#pragma unroll
            for (int e = 0; e < SDM_BATCH; ++e) k[e] = M.ld(min(y0 + e, H - 1) * W + x);     // (clamped, not guarded: the loads leave together)
#pragma unroll
            for (int e = 0; e < SDM_BATCH; ++e) {
                if (y0 + e >= H) break;
                const bool in = k[e] & SDM_IN;
                if (in) { dI = 0; if (dO != SDM_NONE) ++dO; }
                else { dO = 0; if (dI != SDM_NONE) ++dI; }
                M.st((y0 + e) * W + x, in ? SDM_IN | dO : dI);
            }
        }
        dI = dO = SDM_NONE;
        for (int y0 = H - 1; y0 >= 0; y0 -= SDM_BATCH) {
            unsigned k[SDM_BATCH];
#pragma unroll
            for (int e = 0; e < SDM_BATCH; ++e) k[e] = M.ld(max(y0 - e, 0) * W + x);
#pragma unroll
            for (int e = 0; e < SDM_BATCH; ++e) {
                if (y0 - e < 0) break;
                const bool in = k[e] & SDM_IN;
                if (in) { dI = 0; if (dO != SDM_NONE) ++dO; }
                else { dO = 0; if (dI != SDM_NONE) ++dI; }
                const unsigned d = in ? dO : dI;
                if (d < (k[e] & SDM_NONE)) M.st((y0 - e) * W + x, (k[e] & SDM_IN) | d);
            }
        }
    }
    __syncthreads();

    // pass 4: rows.  The class has a pixel and the frame has one outside it: every row meets, in some column, either a pixel of the other
    // kind or one with a real g, so best ends below NONE^2 and below 2^21.
    for (int p = tid; p < HW; p += NT) {
        const int y = p / W, x = p - y * W, row = p - x;
        const unsigned w = M.ld(p), g0 = w & SDM_NONE;
        unsigned best = g0 * g0;
        const int kmax = x > W - 1 - x ? x : W - 1 - x;
        // SDM_WALK steps at a time, their loads in flight together.  A step past the stopping point costs a load and changes nothing: its
        // (x - x')^2 alone is at least the best so far.  A step past an end of the row is clamped to the row's end pixel and needs no guard
        // either: that pixel was met at its own, smaller k, and the larger k only raises the candidate.
        for (int k0 = 1; k0 <= kmax; k0 += SDM_WALK) {
            if ((unsigned)(k0 * k0) >= best) break;
            unsigned l[SDM_WALK], r[SDM_WALK];
#pragma unroll
            for (int e = 0; e < SDM_WALK; ++e) { l[e] = M.ld(row + max(x - k0 - e, 0)); r[e] = M.ld(row + min(x + k0 + e, W - 1)); }
#pragma unroll
            for (int e = 0; e < SDM_WALK; ++e) {
                const int k = k0 + e;
                const unsigned kk = (unsigned)(k * k), gl = l[e] & SDM_NONE, gr = r[e] & SDM_NONE;
                const unsigned dl = ((l[e] ^ w) & SDM_IN) ? kk : kk + gl * gl;
                const unsigned dr = ((r[e] ^ w) & SDM_IN) ? kk : kk + gr * gr;
                best = dl < best ? dl : best;
                best = dr < best ? dr : best;
            }
        }
        out[p] = (w & SDM_IN) ? -(int)best : (int)best;
    }
}

inline bool sdm_shape_ok(int frames, int C, int H, int W)
{
    return mask_shape_ok(frames, H, W) && C >= 1 && C <= SDM_MAXC && (size_t)frames * (size_t)C <= 0x7fffffffu;
}

}  // namespace

extern "C" size_t gdkvm_signed_distance_workspace_bytes(int frames, int C, int H, int W)
{
    if (!sdm_shape_ok(frames, C, H, W) || H * W <= SDM_LDS_PIX) return 0;
    return (size_t)frames * C * sdm_stride(H, W) * sizeof(unsigned short);
}

extern "C" int gdkvm_signed_distance(const uint8_t* target, int32_t* sd2, void* workspace, size_t workspace_bytes,
                                     int frames, int C, int H, int W, unsigned class_mask, void* stream)
{
    if (int rc = mask_check_shape("signed_distance", frames, H, W)) return rc;
    if (!sdm_shape_ok(frames, C, H, W))
        return gdkvm_fail(GDKVM_ERR_SHAPE, "signed_distance: classes=%d outside 1..%d, or frames * classes = %d * %d too many", C, SDM_MAXC, frames, C);
    if (frames == 0) return GDKVM_OK;
    if (!target || !sd2) return gdkvm_fail(GDKVM_ERR_SHAPE, "signed_distance: null pointer (target and sd2 are required)");
    if (reinterpret_cast<uintptr_t>(sd2) & 3u) return gdkvm_fail(GDKVM_ERR_SHAPE, "signed_distance: sd2 must be 4-byte aligned");
    const size_t need = gdkvm_signed_distance_workspace_bytes(frames, C, H, W);
    if (int rc = mask_check_workspace("signed_distance", H, W, need, workspace, workspace_bytes)) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    SdmArgs a{target, sd2, static_cast<unsigned short*>(workspace), C, H, W, H * W, (unsigned)sdm_stride(H, W), class_mask};
    const unsigned grid = (unsigned)((size_t)frames * C);
    if (!need) {
        const size_t lds = ((size_t)H * W * sizeof(unsigned short) + 15) & ~(size_t)15;
        if (lds > 32 * 1024) {                           // a large plane needs the opt-in once per device
            static std::atomic<unsigned long long> done_mask{0};
            int dev = 0;
            if (hipGetDevice(&dev) != hipSuccess) return gdkvm_fail(GDKVM_ERR_LAUNCH, "signed_distance: hipGetDevice");
            const unsigned long long bit = 1ull << (dev & 63);
            if (!(done_mask.load(std::memory_order_relaxed) & bit)) {
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(signed_distance_kernel<true>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, SDM_LDS_PIX * (int)sizeof(unsigned short));
                if (e != hipSuccess) return gdkvm_fail(GDKVM_ERR_LAUNCH, "signed_distance: LDS attribute: %s", hipGetErrorString(e));
                done_mask.fetch_or(bit, std::memory_order_relaxed);
            }
        }
        hipLaunchKernelGGL((signed_distance_kernel<true>), dim3(grid), dim3(SDM_NT), lds, st, a);
    } else {
        hipLaunchKernelGGL((signed_distance_kernel<false>), dim3(grid), dim3(SDM_NT), 0, st, a);
    }
    GDKVM_LAUNCH_CHECK("signed_distance_kernel");
    return GDKVM_OK;
}
