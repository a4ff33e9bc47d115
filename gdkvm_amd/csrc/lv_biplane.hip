// lv_biplane.hip -- bi-plane Simpson volume of the left ventricle from the records of two views (the link behind gdkvm_lv_measure_mm when a
// patient has an apical two-chamber and an apical four-chamber clip): per (pair, frame) the disks of both views become mean widths in mm, disk
// j of view a is multiplied with disk j of view b, and the products are added in ascending j.  include/gdkvm.h holds the definition.  ONE wave
// per (pair, frame), four of them in a workgroup that share nothing: no LDS, no atomics, no fences, no host read-back.  Every table index is
// checked before it is used: a pair that names a clip outside 0 .. C - 1 gets zeros.

#include "mask_frame.hpp"

// No fused multiply-add in this file's own arithmetic, as in lv_measure.hip: the fp64 steps are the definition's operations, one rounding each.
#pragma clang fp contract(off)

namespace {

typedef long long i64;

constexpr int BP_MAX_D = 64;         // disks: one lane of the wave each
constexpr int BP_WAVES = 4;          // (pair, frame)s of a workgroup

struct BiplaneArgs {
    const i64* stats; const i64* disks; const double* geom; const int32_t* spacing; const int32_t* pairs;
    double* out; i64* npix;
    i64 PT;
    int C, T, D;
};

// one view's disk j of frame f = clip * T + t as a mean width in mm (0 for a lane without a disk), n > 0 assured by the caller
__device__ __forceinline__ double disk_width_mm(const BiplaneArgs& a, size_t f, int lane, i64 n, double L)
{
    const i64 E = a.stats[f * 12 + 11];
    const int ry = a.spacing[2 * f], rx = a.spacing[2 * f + 1];
    const double pix = (double)(ry * rx) / 1e6;
    const i64 W = lane < a.D ? a.disks[f * (size_t)a.D + lane] : 0;
    const double aj = ((double)W / (double)((i64)a.D * n * E)) * pix;       // step 6' of gdkvm_lv_measure_mm, operation for operation
    return (aj * (double)a.D) / L;
}

__global__ __launch_bounds__(64 * BP_WAVES) void lv_biplane_kernel(BiplaneArgs a)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, T = a.T, D = a.D;
    const i64 w = (i64)blockIdx.x * BP_WAVES + wv;         // (wave-uniform, like everything up to the disks)
    if (w >= a.PT) return;
    const i64 p = w / T;
    const int t = (int)(w - p * T);
    double* o = a.out + (size_t)w * 3;
    const int ca = a.pairs[2 * p], cb = a.pairs[2 * p + 1];
    i64 na = 0, nb = 0;
    size_t fa = 0, fb = 0;
    if (ca >= 0 && ca < a.C && cb >= 0 && cb < a.C) {
        fa = (size_t)ca * T + t;
        fb = (size_t)cb * T + t;
        na = a.stats[fa * 12];
        nb = a.stats[fb * 12];
    }
    if (na <= 0 || nb <= 0) {                              // a clip outside the tables, an empty frame, or the -1 record of a bad spacing
        if (lane < 3) o[lane] = 0.0;
        if (lane == 3) a.npix[w] = 0;
        return;
    }
    const double La = a.geom[fa * 6], Lb = a.geom[fb * 6];
    const double prod = disk_width_mm(a, fa, lane, na, La) * disk_width_mm(a, fb, lane, nb, Lb);
    double s = 0.0;
    for (int j = 0; j < D; ++j) s = s + __shfl(prod, j);   // ascending j, from 0.0; every lane adds the same terms, lane 0 writes the result
    if (lane == 0) {
        const double L = La > Lb ? La : Lb, Ls = La > Lb ? Lb : La;
        o[0] = (((3.14159265358979323846 / 4.0) * s) * (L / (double)D)) / 1000.0;
        o[1] = L;
        o[2] = (L - Ls) / L;
        a.npix[w] = na < nb ? na : nb;
    }
}

}  // namespace

extern "C" int gdkvm_lv_biplane(const int64_t* stats, const int64_t* disks, const double* geom, const int32_t* spacing_um,
                                const int32_t* pairs, double* out, int64_t* npix, int C, int T, int D, int P, void* stream)
{
    if (C < 0 || T < 0 || P < 0) return gdkvm_fail(GDKVM_ERR_SHAPE, "lv_biplane: bad shape C=%d T=%d P=%d", C, T, P);
    if (D < 1 || D > BP_MAX_D) return gdkvm_fail(GDKVM_ERR_SHAPE, "lv_biplane: D=%d outside 1..%d", D, BP_MAX_D);
    const i64 PT = (i64)P * T;
    if (PT > 0x7fffffffLL || (i64)C * T > 0x7fffffffLL)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "lv_biplane: P*T and C*T must stay below 2^31 (P=%d C=%d T=%d)", P, C, T);
    if (PT == 0) return GDKVM_OK;
    if (!pairs || !out || !npix || (C > 0 && (!stats || !disks || !geom || !spacing_um)))
        return gdkvm_fail(GDKVM_ERR_ARG, "lv_biplane: null pointer");
    if (int rc = mask_check_aligned16("lv_biplane", GDKVM_ERR_ARG, "outputs", {out, npix})) return rc;
    if ((reinterpret_cast<uintptr_t>(stats) | reinterpret_cast<uintptr_t>(disks) | reinterpret_cast<uintptr_t>(geom)) & 7u)
        return gdkvm_fail(GDKVM_ERR_ARG, "lv_biplane: stats, disks and geom must be 8-byte aligned");
    if ((reinterpret_cast<uintptr_t>(spacing_um) | reinterpret_cast<uintptr_t>(pairs)) & 3u)
        return gdkvm_fail(GDKVM_ERR_ARG, "lv_biplane: spacing_um and pairs must be 4-byte aligned");
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    BiplaneArgs a{reinterpret_cast<const i64*>(stats), reinterpret_cast<const i64*>(disks), geom, spacing_um, pairs, out,
                  reinterpret_cast<i64*>(npix), PT, C, T, D};
    hipLaunchKernelGGL(lv_biplane_kernel, dim3((unsigned)((PT + BP_WAVES - 1) / BP_WAVES)), dim3(64 * BP_WAVES), 0, st, a);
    GDKVM_LAUNCH_CHECK("lv_biplane_kernel");
    return GDKVM_OK;
}
