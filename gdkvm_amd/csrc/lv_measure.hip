// lv_measure.hip -- left-ventricular geometry of label masks on the device (the evaluation's epilogue beside the Dice counts): per frame the
// pixel moments of one class, its long axis, the overlap-weighted disk areas along that axis and the single-plane method-of-disks volume
// (lv_measure_kernel); per clip the end-diastolic / end-systolic frames and the ejection fraction (lv_ef_kernel).  include/gdkvm.h holds the
// definition.  Everything up to the disk areas W_j is integer arithmetic: sums are reduced wave-wide by shuffles and per block through LDS, the
// disk areas are added with 64-bit integer LDS atomics -- integer adds commute, so the result is bit-reproducible.  The one floating-point step
// in front of integers (the axis, fp64) is evaluated by every lane from the same totals with explicitly un-fused multiplies and adds.
// ONE 256-lane workgroup per frame: no cross-workgroup reduction, no global atomics, no fences.

#include "mask_frame.hpp"

// No fused multiply-add in this file's own arithmetic: the fp64 steps are the definition's operations, one rounding each.  The pragma is what
// does it -- HIP's own _rn intrinsics are inline functions compiled with contraction allowed, and a product from one still fuses into a sum
// from the other (v_mul_f64 + v_fmac_f64 in the gfx950 code), so the steps are written with the operators below instead.
#pragma clang fp contract(off)

namespace {

typedef long long i64;
typedef unsigned long long u64;

__device__ __forceinline__ double mul_rn(double a, double b) { return a * b; }
__device__ __forceinline__ double add_rn(double a, double b) { return a + b; }
__device__ __forceinline__ double sub_rn(double a, double b) { return a - b; }

constexpr int LV_Q = 1 << 16;        // fixed-point scale of the axis
constexpr int LV_MAX_D = 64;         // disks
constexpr int LV_RES = 16;           // 16-byte vectors a lane keeps across the passes: 16 x 256 lanes x 16 bytes = a 256 x 256 frame

// The kernel's arguments in pixels and with a pixel spacing per frame (gdkvm_lv_measure_mm): each form keeps its own layout
struct LvArgs {
    const uint8_t* mask; i64* stats; i64* disks; double* geom;
    int HW, W, cls, D;
};
struct LvMmArgs {
    const uint8_t* mask; const int32_t* spacing; i64* stats; i64* disks; double* geom;
    int HW, W, cls, D;
};

// One pass over the frame's pixels of the class.  RES: the match bits of the lane's vectors are in registers (mk, filled by the first pass);
// otherwise the vectors are read again (the frame is L2-hot).  edge: bit 0 = the lane's head byte matches, bit 1 = its tail byte.
// f(p, x, y) per pixel; the callbacks of this file use the coordinates only.
template <bool RES, class F>
__device__ __forceinline__ void sweep(const unsigned (&mk)[LV_RES], const MaskFrame<256>& fr, unsigned edge, F&& f)
{
    const int tid = threadIdx.x, head = fr.head, W = fr.W;
    if (edge & 1u) visit_xy(1u, tid, W, f);
    if constexpr (RES) {
#pragma unroll
        for (int k = 0; k < LV_RES; ++k) visit_xy(mk[k], head + 16 * (tid + 256 * k), W, f);
    } else {
        for (int v = tid; v < fr.nvec; v += 256) visit_xy(match16(fr.body[v], fr.cls), head + 16 * v, W, f);
    }
    if (edge & 2u) visit_xy(1u, head + fr.nbody + tid, W, f);
}

// MM: with a pixel spacing per frame (gdkvm_lv_measure_mm).  The passes are the pixel form's, integer for integer, with the axis V of step 3'
// in place of U and one pixel's extent E along it in place of Q; step 6' turns the integers into mm and mL.  MM is a compile-time switch and
// each form keeps its own argument struct, so all four instantiations but one are the code they were as two kernels, instruction for
// instruction (tools/isa_equal.py --kernels: kept; the re-reading mm form differs in register names and the order of a few scalar
// instructions).  That rests on where statements stand, not on `if constexpr` alone:
//   - the pixel form computes its output pointers behind the moment totals, the mm form in front of its early exit;
//   - the eigenvector of pass 2 stands in a block of its own;
//   - the mm-only steps 3' and 6' are blocks under `if constexpr (MM)`, not functions: as functions they are simplified on their own
//     before they are inlined, and the mm forms' code moves (the fixed-point axis alone: 2 lines; the record: 72).
template <bool RES, bool MM>
__global__ __launch_bounds__(256) void lv_measure_kernel(std::conditional_t<MM, LvMmArgs, LvArgs> a)
{
    constexpr int NG = MM ? 6 : 4;                         // doubles of a frame's geom
    __shared__ i64 s_red[4][6];
    __shared__ i64 s_mm[4][2];
    __shared__ u64 s_w[LV_MAX_D];
    const int tid = threadIdx.x, wv = tid >> 6, HW = a.HW, W = a.W, D = a.D;
    const size_t f = blockIdx.x;
    const unsigned cls = (unsigned)a.cls;
    i64 *st, *dk;                                          // the frame's outputs: the mm form needs them for its early exit; in the pixel form
    double* ge;                                            // they stand behind the moment totals, where its code had them
    int ry = 1, rx = 1;
    if constexpr (MM) {
        st = a.stats + f * 12;
        dk = a.disks + f * (size_t)D;
        ge = a.geom + f * NG;
        ry = a.spacing[2 * f]; rx = a.spacing[2 * f + 1];
        if (ry < 1 || ry > 4095 || rx < 1 || rx > 4095) {  // (uniform) no error can be returned from here: the outputs say so
            if (tid < 12) st[tid] = -1;
            if (tid < D) dk[tid] = -1;
            if (tid < NG) ge[tid] = -1.0;
            return;
        }
    }
    const uint8_t* base = a.mask + f * (size_t)HW;
    const MaskFrame<256> fr(base, HW, W, cls);
    if (tid < LV_MAX_D) s_w[tid] = 0;

    unsigned edge = 0;
    if (tid < fr.head && base[tid] == cls) edge |= 1u;
    if (tid < fr.tail && base[fr.head + fr.nbody + tid] == cls) edge |= 2u;
    unsigned mk[LV_RES];
    if constexpr (RES) {
        uint4 r[LV_RES];
#pragma unroll
        for (int k = 0; k < LV_RES; ++k) {
            const int v = tid + 256 * k;
            r[k] = v < fr.nvec ? fr.body[v] : make_uint4(~0u, ~0u, ~0u, ~0u);      // 255 is no class (cls <= 254)
        }
#pragma unroll
        for (int k = 0; k < LV_RES; ++k) mk[k] = match16(r[k], cls);
    }

    // pass 1: moments.  A lane sees at most 4096 + 2 pixels of coordinates below 1024: n, sx, sy fit 32 bits, the second moments need 64
    unsigned n32 = 0, sx32 = 0, sy32 = 0;
    u64 sxx = 0, sxy = 0, syy = 0;
    sweep<RES>(mk, fr, edge, [&](int, int x, int y) {
        ++n32; sx32 += (unsigned)x; sy32 += (unsigned)y;
        sxx += (unsigned)(x * x); sxy += (unsigned)(x * y); syy += (unsigned)(y * y);
    });
    {
        const i64 part[6] = {(i64)n32, (i64)sx32, (i64)sy32, (i64)sxx, (i64)sxy, (i64)syy};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const i64 s = wave_sum(part[i]);
            if ((tid & 63) == 0) s_red[wv][i] = s;
        }
    }
    __syncthreads();
    i64 tot[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) tot[i] = wg_sum(s_red, i);
    const i64 n = tot[0], sx = tot[1], sy = tot[2];
    if constexpr (!MM) {
        st = a.stats + f * 12;
        dk = a.disks + f * (size_t)D;
        ge = a.geom + f * NG;
    }
    if (n == 0) {                                          // (uniform) empty frame: every output is 0
        if (tid < 12) st[tid] = 0;
        if (tid < D) dk[tid] = 0;
        if (tid < NG) ge[tid] = 0.0;
        return;
    }

    // pass 2: the long axis, the eigenvector of the larger eigenvalue of [[A, B], [B, C]] -- every lane, the same operations on the same
    // totals.  (Ux, Uy) is the axis in fixed point and E one pixel's extent along it: Q in pixels.  Step 3' with a spacing: the pixel's sides
    // py, px in units of gc = gcd(ry, rx) scale the moments in front of the eigenvector and the axis (V in the definition) behind it, and
    // eh is the pixel's extent along the axis in units of gc.
    int gc = 1, py = 1, px = 1, pm = 1;
    if constexpr (MM) {                                    // step 3', first part
        gc = ry;
        for (int b = rx; b != 0;) { const int t = gc % b; gc = b; b = t; }    // (uniform; at most 18 turns for 12-bit operands)
        py = ry / gc, px = rx / gc, pm = px > py ? px : py;
    }
    const i64 A = n * tot[3] - sx * sx, B = n * tot[4] - sx * sy, C = n * tot[5] - sy * sy;
    int Ux, Uy, E;
    double eh = 0.0;                                       // (mm only)
    {
        const double da = MM ? sub_rn(mul_rn((double)(px * px), (double)A), mul_rn((double)(py * py), (double)C)) : (double)(A - C);
        const double db = MM ? mul_rn(2.0, mul_rn((double)(px * py), (double)B)) : (double)(2 * B);
        const double r = sqrt(add_rn(mul_rn(da, da), mul_rn(db, db)));
        double vx, vy;
        if (r == 0.0) { vx = 0.0; vy = 1.0; }
        else if (da >= 0.0) { vx = add_rn(da, r); vy = db; }
        else { vx = db; vy = sub_rn(r, da); }
        const double nrm = sqrt(add_rn(mul_rn(vx, vx), mul_rn(vy, vy)));
        double ux = vx / nrm, uy = vy / nrm;
        if (uy < 0.0 || (uy == 0.0 && ux < 0.0)) { ux = -ux; uy = -uy; }
        if constexpr (MM) {                                // step 3', second part
            const double ex = mul_rn(ux, (double)px), ey = mul_rn(uy, (double)py);
            eh = sqrt(add_rn(mul_rn(ex, ex), mul_rn(ey, ey)));
            Ux = (int)rint(mul_rn(ux, (double)(px * LV_Q)) / (double)pm), Uy = (int)rint(mul_rn(uy, (double)(py * LV_Q)) / (double)pm);
            E = (int)rint(mul_rn(eh, (double)LV_Q) / (double)pm);
        } else {
            Ux = (int)rint(ux * (double)LV_Q); Uy = (int)rint(uy * (double)LV_Q); E = LV_Q;
        }
    }

    // pass 3: extent of the projections t_p = (n x - sx) Ux + (n y - sy) Uy; |n x - sx| < 2^30 and |Ux|, |Uy| <= Q, so two 32 x 32 -> 64
    // multiply-adds per pixel
    const int n_i = (int)n, sx_i = (int)sx, sy_i = (int)sy;
    auto proj = [&](int x, int y) -> i64 { return (i64)(n_i * x - sx_i) * Ux + (i64)(n_i * y - sy_i) * Uy; };
    i64 tmin = 0x7fffffffffffffffLL, tmax = -0x7fffffffffffffffLL - 1;
    sweep<RES>(mk, fr, edge, [&](int, int x, int y) {
        const i64 t = proj(x, y);
        tmin = t < tmin ? t : tmin;
        tmax = t > tmax ? t : tmax;
    });
    tmin = wave_min(tmin);
    tmax = wave_max(tmax);
    if ((tid & 63) == 0) { s_mm[wv][0] = tmin; s_mm[wv][1] = tmax; }
    __syncthreads();                                       // (also orders the zeroing of s_w in front of the atomics below)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        tmin = s_mm[w][0] < tmin ? s_mm[w][0] : tmin;
        tmax = s_mm[w][1] > tmax ? s_mm[w][1] : tmax;
    }

    // pass 4: pixel p covers [D (t_p - tmin), + D P1), P1 = n E, disk j covers [j Lt, (j + 1) Lt): W_j = sum of the overlaps
    const i64 P1 = n * E, Lt = tmax - tmin + P1, DP1 = (i64)D * P1;
    const double inv_lt = 1.0 / (double)Lt;
    sweep<RES>(mk, fr, edge, [&](int, int x, int y) {
        const i64 lo = (i64)D * (proj(x, y) - tmin), hi = lo + DP1;
        int j = (int)((double)lo * inv_lt);                // floor(lo / Lt) up to rounding, made exact below
        j = j < 0 ? 0 : (j > D - 1 ? D - 1 : j);
        while (j > 0 && (i64)j * Lt > lo) --j;
        while (j < D - 1 && (i64)(j + 1) * Lt <= lo) ++j;
        for (; j < D && (i64)j * Lt < hi; ++j) {
            const i64 d0 = (i64)j * Lt, d1 = d0 + Lt;
            const i64 ov = (hi < d1 ? hi : d1) - (lo > d0 ? lo : d0);
            atomicAdd(&s_w[j], (u64)ov);
        }
    });
    __syncthreads();

    // pass 5: the record (st[11]: E with a spacing, 0 in pixels), and step 6'
    if (tid < D) dk[tid] = (i64)s_w[tid];
    if (tid < 6) st[tid] = tot[tid];
    if (tid == 6) { st[6] = Ux; st[7] = Uy; st[8] = tmin; st[9] = tmax; st[10] = Lt; st[11] = MM ? E : 0; }
    if (tid == 64) {
        if constexpr (MM) {                                // step 6': mm and mL
            const double k = mul_rn(eh, (double)gc);
            const double L = mul_rn((double)Lt / (double)P1, k) / 1000.0;
            const double pix = (double)(ry * rx) / 1e6;
            double s = 0.0;
            for (int j = 0; j < D; ++j) {
                const double aj = mul_rn((double)(i64)s_w[j] / (double)DP1, pix);
                s = add_rn(s, mul_rn(aj, aj));
            }
            ge[0] = L;
            ge[1] = mul_rn(mul_rn(3.14159265358979323846, (double)D), s) / mul_rn(4.0, L) / 1000.0;
            ge[2] = mul_rn((double)sx / (double)n, (double)rx) / 1000.0;
            ge[3] = mul_rn((double)sy / (double)n, (double)ry) / 1000.0;
            ge[4] = k;
            ge[5] = (double)(n * (i64)(ry * rx)) / 1e6;
        } else {
            const double L = (double)Lt / (double)P1;
            double s = 0.0;
            for (int j = 0; j < D; ++j) {
                const double aj = (double)(i64)s_w[j] / (double)DP1;
                s = add_rn(s, mul_rn(aj, aj));
            }
            ge[0] = L;
            ge[1] = mul_rn(mul_rn(3.14159265358979323846, (double)D), s) / mul_rn(4.0, L);
            ge[2] = (double)sx / (double)n;
            ge[3] = (double)sy / (double)n;
        }
    }
}

struct EfArgs {
    const double* vol; const i64* npix; const double* pick_vol; const i64* pick_npix;
    int32_t* idx; double* val;
    int T; i64 min_pixels;
};

// one wave per clip; ED = the valid frame of the largest pick volume, ES = of the smallest, ties -> the lowest t
__global__ __launch_bounds__(64) void lv_ef_kernel(EfArgs a)
{
    const int lane = threadIdx.x, T = a.T;
    const size_t b = blockIdx.x;
    const double* pv = (a.pick_vol ? a.pick_vol : a.vol) + b * (size_t)T;
    const i64* pn = (a.pick_npix ? a.pick_npix : a.npix) + b * (size_t)T;
    int cnt = 0, edt = -1, est = -1;
    double edv = 0.0, esv = 0.0;
    for (int t = lane; t < T; t += 64) {
        if (pn[t] < a.min_pixels) continue;
        const double v = pv[t];
        ++cnt;
        if (edt < 0 || v > edv) { edv = v; edt = t; }       // (t ascends within a lane: strict comparisons keep the lowest t)
        if (est < 0 || v < esv) { esv = v; est = t; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cnt += __shfl_xor(cnt, o);
        const int t1 = __shfl_xor(edt, o), t2 = __shfl_xor(est, o);
        const double v1 = __shfl_xor(edv, o), v2 = __shfl_xor(esv, o);
        if (t1 >= 0 && (edt < 0 || v1 > edv || (v1 == edv && t1 < edt))) { edv = v1; edt = t1; }
        if (t2 >= 0 && (est < 0 || v2 < esv || (v2 == esv && t2 < est))) { esv = v2; est = t2; }
    }
    if (lane == 0) {
        int32_t* idx = a.idx + b * 3;
        double* val = a.val + b * 3;
        idx[2] = cnt;
        if (cnt < 2) {
            idx[0] = idx[1] = -1;
            val[0] = val[1] = val[2] = 0.0;
        } else {
            const double EDV = a.vol[b * (size_t)T + edt], ESV = a.vol[b * (size_t)T + est];
            idx[0] = edt; idx[1] = est;
            val[0] = EDV; val[1] = ESV;
            val[2] = EDV == 0.0 ? 0.0 : sub_rn(EDV, ESV) / EDV;
        }
    }
}

// What gdkvm_lv_measure (MM = false, spacing_um unused) and gdkvm_lv_measure_mm share: the checks in their order under the entry point's
// name, and the launch of the form the frame's size selects
template <bool MM>
int lv_measure_launch(const char* name, const char* kernel, const uint8_t* mask, const int32_t* spacing_um, int64_t* stats, int64_t* disks,
                      double* geom, int frames, int H, int W, int cls, int D, void* stream)
{
    if (int rc = mask_check_shape(name, frames, H, W)) return rc;
    if (D < 1 || D > LV_MAX_D) return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: D=%d outside 1..%d", name, D, LV_MAX_D);
    if (int rc = mask_check_cls(name, GDKVM_ERR_ARG, cls)) return rc;
    if (frames == 0) return GDKVM_OK;
    if (!mask || (MM && !spacing_um) || !stats || !disks || !geom) return gdkvm_fail(GDKVM_ERR_ARG, "%s: null pointer", name);
    if (MM && (reinterpret_cast<uintptr_t>(spacing_um) & 3u)) return gdkvm_fail(GDKVM_ERR_ARG, "%s: spacing_um must be 4-byte aligned", name);
    if (int rc = mask_check_aligned16(name, GDKVM_ERR_ARG, "outputs", {stats, disks, geom})) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    std::conditional_t<MM, LvMmArgs, LvArgs> a;
    if constexpr (MM) a = LvMmArgs{mask, spacing_um, reinterpret_cast<i64*>(stats), reinterpret_cast<i64*>(disks), geom, H * W, W, cls, D};
    else a = LvArgs{mask, reinterpret_cast<i64*>(stats), reinterpret_cast<i64*>(disks), geom, H * W, W, cls, D};
    // a frame of up to 15 head bytes + LV_RES * 256 vectors keeps its match bits in registers
    if (H * W <= LV_RES * 256 * 16) hipLaunchKernelGGL((lv_measure_kernel<true, MM>), dim3((unsigned)frames), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((lv_measure_kernel<false, MM>), dim3((unsigned)frames), dim3(256), 0, st, a);
    GDKVM_LAUNCH_CHECK(kernel);
    return GDKVM_OK;
}

}  // namespace

extern "C" int gdkvm_lv_measure(const uint8_t* mask, int64_t* stats, int64_t* disks, double* geom,
                                int frames, int H, int W, int cls, int D, void* stream)
{
    return lv_measure_launch<false>("lv_measure", "lv_measure_kernel", mask, nullptr, stats, disks, geom, frames, H, W, cls, D, stream);
}

extern "C" int gdkvm_lv_measure_mm(const uint8_t* mask, const int32_t* spacing_um, int64_t* stats, int64_t* disks, double* geom,
                                   int frames, int H, int W, int cls, int D, void* stream)
{
    return lv_measure_launch<true>("lv_measure_mm", "lv_measure_mm_kernel", mask, spacing_um, stats, disks, geom, frames, H, W, cls, D, stream);
}

extern "C" int gdkvm_lv_ef(const double* vol, const int64_t* npix, const double* pick_vol, const int64_t* pick_npix,
                           int32_t* ed_es_nvalid, double* edv_esv_ef, int B, int T, int64_t min_pixels, void* stream)
{
    if (B < 0 || T < 1) return gdkvm_fail(GDKVM_ERR_SHAPE, "lv_ef: bad shape B=%d T=%d", B, T);
    if ((pick_vol == nullptr) != (pick_npix == nullptr))
        return gdkvm_fail(GDKVM_ERR_ARG, "lv_ef: pick_vol and pick_npix go together (one of them is null)");
    if (B == 0) return GDKVM_OK;
    if (!vol || !npix || !ed_es_nvalid || !edv_esv_ef) return gdkvm_fail(GDKVM_ERR_ARG, "lv_ef: null pointer");
    if (!gdkvm_aligned16(ed_es_nvalid) || !gdkvm_aligned16(edv_esv_ef))
        return gdkvm_fail(GDKVM_ERR_ARG, "lv_ef: outputs must be 16-byte aligned");
    if ((reinterpret_cast<uintptr_t>(vol) | reinterpret_cast<uintptr_t>(npix) | reinterpret_cast<uintptr_t>(pick_vol) |
         reinterpret_cast<uintptr_t>(pick_npix)) & 7u)
        return gdkvm_fail(GDKVM_ERR_ARG, "lv_ef: inputs must be 8-byte aligned");
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    EfArgs a{vol, reinterpret_cast<const i64*>(npix), pick_vol, reinterpret_cast<const i64*>(pick_npix), ed_es_nvalid, edv_esv_ef, T,
             (i64)min_pixels};
    hipLaunchKernelGGL(lv_ef_kernel, dim3((unsigned)B), dim3(64), 0, st, a);
    GDKVM_LAUNCH_CHECK("lv_ef_kernel");
    return GDKVM_OK;
}
