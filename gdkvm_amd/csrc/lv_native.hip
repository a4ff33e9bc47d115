// lv_native.hip -- left-ventricular geometry of one class of label masks at every clip's own frame size (h0, w0) with the spacing of the
// native pixel (what EDV, ESV and EF in mL at native resolution are made of; eval.py's native.lv block).  include/gdkvm.h holds the
// definition (gdkvm_lv_measure_native): steps 1, 2, 3', 4, 5 and 6' of gdkvm_lv_measure_mm, integer for integer and fp64 operation for fp64
// operation, for sides up to 2048 -- so the index and product widths are this file's own (the header restates the bounds they rest on) and
// lv_measure.hip's kernel is neither instantiated nor touched.
//
// The mask is ragged: native_clips.hpp holds the launcher's side of that; a clip's entry here is (byte offset, band-row offset, h0, w0, ry,
// rx).  Nothing copied, nothing allocated, nothing synchronised.
//
// A frame's work is spread over many workgroups by FOUR kernels in stream order over BANDS of LN_BAND_ROWS native rows of one (clip,
// frame); a kernel reads what an earlier KERNEL wrote and nothing that another workgroup of its own launch writes: no flag, no spinning, no
// fence, no global atomic.  What they hand each other is the `bands` output, one row of 8 + D words per band:
//   (a) ln_moments   per band: n, sx, sy, sxx, sxy, syy of the band's rows (words 0..5).
//   (b) ln_extent    per band: every workgroup adds its frame's band moments (lane l of a wave holds band l; integer sums, so the order
//       gives no other word), evaluates step 3' itself -- every lane the same operations on the same totals, so every workgroup of a frame
//       gets the same axis -- and writes tmin, tmax of the band's pixels (words 6, 7).
//   (c) ln_disks     per band: the totals and the axis again, the frame's tmin / tmax from the bands' words, and the band's partial W_j,
//       added in LDS with 64-bit integer atomics as lv_measure.hip does (a lane adds a run of pixels that fall into one disk in a register
//       first), then stored (words 8 .. 8 + D - 1).
//   (d) ln_finish    per frame, one wave: adds the bands and writes stats, disks and geom.
// Integer adds commute, so every word is bit-reproducible.  Each of the passes (a) - (c) reads the band's bytes once, 16 bytes per load
// on the 16-byte grid of the addresses (mask_frame.hpp's sweep); (b) and (c) skip a band without a pixel of the class.
// Every kernel takes further items grid-stride past LN_MAX_WG workgroups.  Loop bounds: a band's vectors count to LN_BAND_ROWS w0 / 16 /
// 256 = 16 per lane, a pixel meets at most D disks, the gcd takes at most 18 turns, a frame has at most 64 bands.

#include "native_clips.hpp"

// No fused multiply-add in this file's own arithmetic (see lv_measure.hip): the fp64 steps are the definition's operations, one rounding each
#pragma clang fp contract(off)

namespace {

typedef long long i64;
typedef unsigned long long u64;

__device__ __forceinline__ double mul_rn(double a, double b) { return a * b; }
__device__ __forceinline__ double add_rn(double a, double b) { return a + b; }
__device__ __forceinline__ double sub_rn(double a, double b) { return a - b; }

constexpr int LN_NT = 256;
constexpr int LN_Q = 1 << 16;                                  // fixed-point scale of the axis
constexpr int LN_MAX_D = 64;                                   // disks
constexpr int LN_BAND_ROWS = GDKVM_LV_NATIVE_BAND_ROWS;        // rows of a band (gdkvm.h)
constexpr int LN_MAX_WG = GDKVM_LV_NATIVE_MAX_WG;              // workgroups per launch; more items than that are walked grid-stride
constexpr int LN_CLIPS = GDKVM_LV_NATIVE_CLIPS;                // clips per launch
constexpr int LN_MAX_BANDS = NATIVE_MAX_SIDE / LN_BAND_ROWS;   // 64: lane l of a wave holds band l of the frame
constexpr i64 LN_I64_MAX = 0x7fffffffffffffffLL, LN_I64_MIN = -0x7fffffffffffffffLL - 1;
static_assert(LN_MAX_BANDS <= 64, "one wave adds a frame's bands");
static_assert(LN_BAND_ROWS * NATIVE_MAX_SIDE <= (1 << 16), "a lane of 256 meets at most 256 + 2 pixels of a band: its n, sx, sy fit 32 bits");

struct LnClip {
    u64 off, brow;                                         // the clip's first byte in mask, its first row in bands
    unsigned short h0, w0, ry, rx;
};
struct LnArgs {
    const uint8_t* mask; i64* stats; i64* disks; double* geom; i64* bands;
    long long frame0;                                      // the launch's first frame of the call
    int nclips, T, cls, D, maxbands;
    LnClip c[LN_CLIPS];
};
static_assert(sizeof(LnArgs) <= 2048, "the clip table travels in the kernel arguments");

// One (clip, frame, band) of a launch, the same in every lane
struct LnItem {
    const uint8_t* base;                                   // the band's first byte
    i64* frame_rows;                                       // the frame's first row of bands
    int w0, ry, rx, nbands, band, row0, rows;
    bool live;                                             // false: this clip has fewer bands than the launch's largest
};
__device__ __forceinline__ LnItem ln_item(const LnArgs& a, long long item)
{
    const long long per_clip = (long long)a.T * a.maxbands;
    const int clip = (int)(item / per_clip);
    const long long rem = item - clip * per_clip;
    const int t = (int)(rem / a.maxbands), band = (int)(rem - (long long)t * a.maxbands);
    const LnClip c = a.c[clip];
    LnItem it;
    it.w0 = c.w0; it.ry = c.ry; it.rx = c.rx; it.band = band;
    const int h0 = c.h0;
    it.nbands = (h0 + LN_BAND_ROWS - 1) / LN_BAND_ROWS;
    it.live = band < it.nbands;
    it.row0 = band * LN_BAND_ROWS;
    it.rows = h0 - it.row0 < LN_BAND_ROWS ? h0 - it.row0 : LN_BAND_ROWS;
    it.base = a.mask + (size_t)c.off + (size_t)t * (size_t)(h0 * it.w0) + (size_t)it.row0 * (size_t)it.w0;
    it.frame_rows = a.bands + ((size_t)c.brow + (size_t)t * (size_t)it.nbands) * (size_t)(8 + a.D);
    return it;
}

// The frame's six moments from its bands' words 0..5, in every lane of the calling wave
__device__ __forceinline__ void ln_totals(const i64* frame_rows, int nbands, int stride, i64 (&tot)[6])
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int i = 0; i < 6; ++i) tot[i] = wave_sum(lane < nbands ? frame_rows[(size_t)lane * stride + i] : (i64)0);
}

// Steps 2 and 3' (n > 0).  A, B and C fit int64 (below 2^62.5 in magnitude) but the products n sxx and sx^2 reach 2^66: they are formed in
// unsigned 64-bit wrap-around arithmetic, whose difference is the exact value.  The fp64 part is lv_measure.hip's, operation for operation.
struct LnAxis { int Vx, Vy, E, gc; double eh; };
__device__ __forceinline__ LnAxis ln_axis(const i64 (&tot)[6], int ry, int rx)
{
    int gc = ry;
    for (int b = rx; b != 0;) { const int t = gc % b; gc = b; b = t; }        // (uniform; at most 18 turns for 12-bit operands)
    const int py = ry / gc, px = rx / gc, pm = px > py ? px : py;
    const u64 n = (u64)tot[0], sx = (u64)tot[1], sy = (u64)tot[2];
    const i64 A = (i64)(n * (u64)tot[3] - sx * sx), B = (i64)(n * (u64)tot[4] - sx * sy), C = (i64)(n * (u64)tot[5] - sy * sy);
    const double da = sub_rn(mul_rn((double)(px * px), (double)A), mul_rn((double)(py * py), (double)C));
    const double db = mul_rn(2.0, mul_rn((double)(px * py), (double)B));
    const double r = sqrt(add_rn(mul_rn(da, da), mul_rn(db, db)));
    double vx, vy;
    if (r == 0.0) { vx = 0.0; vy = 1.0; }
    else if (da >= 0.0) { vx = add_rn(da, r); vy = db; }
    else { vx = db; vy = sub_rn(r, da); }
    const double nrm = sqrt(add_rn(mul_rn(vx, vx), mul_rn(vy, vy)));
    double ux = vx / nrm, uy = vy / nrm;
    if (uy < 0.0 || (uy == 0.0 && ux < 0.0)) { ux = -ux; uy = -uy; }
    const double ex = mul_rn(ux, (double)px), ey = mul_rn(uy, (double)py);
    LnAxis ax;
    ax.gc = gc;
    ax.eh = sqrt(add_rn(mul_rn(ex, ex), mul_rn(ey, ey)));
    ax.Vx = (int)rint(mul_rn(ux, (double)(px * LN_Q)) / (double)pm);
    ax.Vy = (int)rint(mul_rn(uy, (double)(py * LN_Q)) / (double)pm);
    ax.E = (int)rint(mul_rn(ax.eh, (double)LN_Q) / (double)pm);
    return ax;
}

// Step 4 for the pixel (x, y) of the frame, t = (n x - sx) Vx + (n y - sy) Vy: |n x - sx| < 2^33 and |Vx|, |Vy| <= 2^16, so 64-bit
// products and |t| < 2^50.  Multiplied out, t = (n Vx) x + (n Vy) y - (sx Vx + sy Vy): the same integer (|n Vx x|, |sx Vx| < 2^49, no sum
// leaves 64 bits) from three per-frame constants and two 64 x 32-bit products per pixel
struct LnProj {
    i64 a, b, c;
    __device__ __forceinline__ LnProj(const i64 (&tot)[6], const LnAxis& ax)
        : a(tot[0] * ax.Vx), b(tot[0] * ax.Vy), c(-(tot[1] * ax.Vx + tot[2] * ax.Vy)) {}
    __device__ __forceinline__ i64 operator()(int x, int y) const { return a * x + b * y + c; }
};

// (a) the six moments of one band
__global__ __launch_bounds__(LN_NT) void ln_moments_kernel(LnArgs a)
{
    __shared__ i64 s_red[LN_NT / 64][6];
    const int tid = threadIdx.x, wv = tid >> 6;
    const long long items = (long long)a.T * a.maxbands * a.nclips;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const LnItem it = ln_item(a, item);
        if (!it.live) continue;                            // (uniform)
        unsigned n32 = 0, sx32 = 0, sy32 = 0;
        u64 sxx = 0, sxy = 0, syy = 0;
        MaskFrame<LN_NT>(it.base, it.rows * it.w0, it.w0, (unsigned)a.cls).sweep_xy([&](int, int x, int yb) {
            const int y = it.row0 + yb;                    // (x, y < 2048: the products fit 32 bits)
            ++n32; sx32 += (unsigned)x; sy32 += (unsigned)y;
            sxx += (unsigned)(x * x); sxy += (unsigned)(x * y); syy += (unsigned)(y * y);
        });
        const i64 part[6] = {(i64)n32, (i64)sx32, (i64)sy32, (i64)sxx, (i64)sxy, (i64)syy};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const i64 s = wave_sum(part[i]);
            if ((tid & 63) == 0) s_red[wv][i] = s;
        }
        __syncthreads();
        if (tid < 6) it.frame_rows[(size_t)it.band * (8 + a.D) + tid] = wg_sum(s_red, tid);
        __syncthreads();                                   // (the next item's partials)
    }
}

// (b) tmin, tmax of one band
__global__ __launch_bounds__(LN_NT) void ln_extent_kernel(LnArgs a)
{
    __shared__ i64 s_mm[LN_NT / 64][2];
    const int tid = threadIdx.x, wv = tid >> 6, stride = 8 + a.D;
    const long long items = (long long)a.T * a.maxbands * a.nclips;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const LnItem it = ln_item(a, item);
        if (!it.live) continue;                            // (uniform)
        i64* row = it.frame_rows + (size_t)it.band * stride;
        i64 tot[6];
        ln_totals(it.frame_rows, it.nbands, stride, tot);
        if (tot[0] == 0) {                                 // (uniform) empty frame: every word of its bands is 0
            if (tid < 2) row[6 + tid] = 0;
            continue;
        }
        i64 tmin = LN_I64_MAX, tmax = LN_I64_MIN;
        if (row[0] != 0) {                                 // (uniform) the band has pixels of the class
            const LnAxis ax = ln_axis(tot, it.ry, it.rx);
            const LnProj proj(tot, ax);
            MaskFrame<LN_NT>(it.base, it.rows * it.w0, it.w0, (unsigned)a.cls).sweep_xy([&](int, int x, int yb) {
                const i64 t = proj(x, it.row0 + yb);
                tmin = t < tmin ? t : tmin;
                tmax = t > tmax ? t : tmax;
            });
        }
        tmin = wave_min(tmin);
        tmax = wave_max(tmax);
        if ((tid & 63) == 0) { s_mm[wv][0] = tmin; s_mm[wv][1] = tmax; }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int w = 0; w < LN_NT / 64; ++w) {
                tmin = s_mm[w][0] < tmin ? s_mm[w][0] : tmin;
                tmax = s_mm[w][1] > tmax ? s_mm[w][1] : tmax;
            }
            row[6] = tmin; row[7] = tmax;
        }
        __syncthreads();                                   // (the next item's partials)
    }
}

// The frame's tmin and tmax from its bands' words 6 and 7 (a band without a pixel holds INT64_MAX, INT64_MIN), in every lane of the wave
__device__ __forceinline__ void ln_frame_extent(const i64* frame_rows, int nbands, int stride, i64& tmin, i64& tmax)
{
    const int lane = threadIdx.x & 63;
    tmin = wave_min(lane < nbands ? frame_rows[(size_t)lane * stride + 6] : LN_I64_MAX);
    tmax = wave_max(lane < nbands ? frame_rows[(size_t)lane * stride + 7] : LN_I64_MIN);
}

// (c) the partial disk areas of one band.  Pixel p covers [D (t_p - tmin), + D P1), P1 = n E, disk j covers [j Lt, (j + 1) Lt):
// D (t - tmin) + D P1 and (j + 1) Lt are below 2^58, a band's W_j below the frame's, which is below 2^61.6 (gdkvm.h)
__global__ __launch_bounds__(LN_NT) void ln_disks_kernel(LnArgs a)
{
    __shared__ u64 s_w[LN_MAX_D];
    const int tid = threadIdx.x, D = a.D, stride = 8 + D;
    const long long items = (long long)a.T * a.maxbands * a.nclips;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const LnItem it = ln_item(a, item);
        if (!it.live) continue;                            // (uniform)
        i64* row = it.frame_rows + (size_t)it.band * stride;
        if (row[0] == 0) {                                 // (uniform) no pixel of the class in the band (or in the frame)
            if (tid < D) row[8 + tid] = 0;
            continue;
        }
        i64 tot[6], tmin, tmax;
        ln_totals(it.frame_rows, it.nbands, stride, tot);
        ln_frame_extent(it.frame_rows, it.nbands, stride, tmin, tmax);
        const LnAxis ax = ln_axis(tot, it.ry, it.rx);
        const LnProj proj(tot, ax);
        if (tid < LN_MAX_D) s_w[tid] = 0;
        __syncthreads();
        const i64 P1 = tot[0] * ax.E, Lt = tmax - tmin + P1, DP1 = (i64)D * P1;
        const double inv_lt = 1.0 / (double)Lt;
        int cj = -1;                                       // the disk the lane's pending sum belongs to
        u64 acc = 0;
        MaskFrame<LN_NT>(it.base, it.rows * it.w0, it.w0, (unsigned)a.cls).sweep_xy([&](int, int x, int yb) {
            const i64 lo = (i64)D * (proj(x, it.row0 + yb) - tmin), hi = lo + DP1;
            int j = (int)((double)lo * inv_lt);            // floor(lo / Lt) up to rounding, made exact below
            j = j < 0 ? 0 : (j > D - 1 ? D - 1 : j);
            while (j > 0 && (i64)j * Lt > lo) --j;
            while (j < D - 1 && (i64)(j + 1) * Lt <= lo) ++j;
            for (; j < D && (i64)j * Lt < hi; ++j) {
                const i64 d0 = (i64)j * Lt, d1 = d0 + Lt;
                const i64 ov = (hi < d1 ? hi : d1) - (lo > d0 ? lo : d0);
                if (j != cj) {
                    if (cj >= 0) atomicAdd(&s_w[cj], acc);
                    cj = j; acc = 0;
                }
                acc += (u64)ov;
            }
        });
        if (cj >= 0) atomicAdd(&s_w[cj], acc);
        __syncthreads();
        if (tid < D) row[8 + tid] = (i64)s_w[tid];
        __syncthreads();                                   // (the next item zeroes the sums)
    }
}

// (d) one frame's record from its bands: one wave, lane l holds band l for the totals and disk l for the areas
__global__ __launch_bounds__(64) void ln_finish_kernel(LnArgs a)
{
    __shared__ i64 s_w[LN_MAX_D];
    const int lane = threadIdx.x, D = a.D, stride = 8 + D;
    const long long items = (long long)a.nclips * a.T;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int clip = (int)(item / a.T), t = (int)(item - (long long)clip * a.T);
        const LnClip c = a.c[clip];
        const int ry = c.ry, rx = c.rx, nbands = (c.h0 + LN_BAND_ROWS - 1) / LN_BAND_ROWS;
        const i64* frame_rows = a.bands + ((size_t)c.brow + (size_t)t * (size_t)nbands) * (size_t)stride;
        const size_t f = (size_t)a.frame0 + (size_t)item;
        i64 *st = a.stats + f * 12, *dk = a.disks + f * (size_t)D;
        double* ge = a.geom + f * 6;
        i64 tot[6];
        ln_totals(frame_rows, nbands, stride, tot);
        const i64 n = tot[0], sx = tot[1], sy = tot[2];
        if (n == 0) {                                      // (uniform) empty frame: every output is 0
            if (lane < 12) st[lane] = 0;
            if (lane < D) dk[lane] = 0;
            if (lane < 6) ge[lane] = 0.0;
            continue;
        }
        i64 tmin, tmax;
        ln_frame_extent(frame_rows, nbands, stride, tmin, tmax);
        const LnAxis ax = ln_axis(tot, ry, rx);
        const i64 P1 = n * ax.E, Lt = tmax - tmin + P1, DP1 = (i64)D * P1;
        if (lane < D) {
            i64 w = 0;
            for (int b = 0; b < nbands; ++b) w += frame_rows[(size_t)b * stride + 8 + lane];
            dk[lane] = w;
            s_w[lane] = w;
        }
        if (lane < 6) st[lane] = tot[lane];
        if (lane == 6) { st[6] = ax.Vx; st[7] = ax.Vy; st[8] = tmin; st[9] = tmax; st[10] = Lt; st[11] = ax.E; }
        __syncthreads();
        if (lane == 0) {                                   // step 6': mm and mL, lv_measure.hip's operations
            const double k = mul_rn(ax.eh, (double)ax.gc);
            const double L = mul_rn((double)Lt / (double)P1, k) / 1000.0;
            const double pix = (double)(ry * rx) / 1e6;
            double s = 0.0;
            for (int j = 0; j < D; ++j) {
                const double aj = mul_rn((double)s_w[j] / (double)DP1, pix);
                s = add_rn(s, mul_rn(aj, aj));
            }
            ge[0] = L;
            ge[1] = mul_rn(mul_rn(3.14159265358979323846, (double)D), s) / mul_rn(4.0, L) / 1000.0;
            ge[2] = mul_rn((double)sx / (double)n, (double)rx) / 1000.0;
            ge[3] = mul_rn((double)sy / (double)n, (double)ry) / 1000.0;
            ge[4] = k;
            ge[5] = (double)(n * (i64)(ry * rx)) / 1e6;
        }
        __syncthreads();                                   // (the next item's areas)
    }
}

}  // namespace

extern "C" int gdkvm_lv_measure_native(const uint8_t* mask, const int32_t* sizes, const int32_t* spacing_um, int64_t* stats, int64_t* disks,
                                       double* geom, int64_t* bands, size_t native_bytes, long long native_bands, int clips, int T, int cls,
                                       int D, void* stream)
{
    const char* name = "lv_measure_native";
    if (clips < 0 || T < 1) return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: bad arguments clips=%d T=%d (clips >= 0, T >= 1)", name, clips, T);
    if (D < 1 || D > LN_MAX_D) return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: D=%d outside 1..%d", name, D, LN_MAX_D);
    if (int rc = mask_check_cls(name, GDKVM_ERR_ARG, cls)) return rc;
    if (clips == 0) return GDKVM_OK;
    if (!mask || !sizes || !spacing_um || !stats || !disks || !geom || !bands)
        return gdkvm_fail(GDKVM_ERR_ARG, "%s: null pointer (mask, the host sizes, the host spacing_um, stats, disks, geom and bands are required)",
                          name);
    if (int rc = mask_check_aligned16(name, GDKVM_ERR_ARG, "outputs", {stats, disks, geom, bands})) return rc;
    size_t total, rows = 0;
    if (int rc = native_check_clips(name, "frames", sizes, spacing_um, native_bytes, clips, T, total)) return rc;
    for (int b = 0; b < clips; ++b) rows += (size_t)T * (size_t)((sizes[2 * b] + LN_BAND_ROWS - 1) / LN_BAND_ROWS);
    if (native_bands < 0 || (size_t)native_bands != rows)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: the native frames of these sizes have %zu bands of %d rows, native_bands = %lld", name, rows,
                          LN_BAND_ROWS, native_bands);
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    size_t brow = 0;                                       // carried from launch to launch, as the walk carries off
    return native_launches<LnArgs, LN_CLIPS>(sizes, clips, T, [&](LnArgs& a, int k, int b, int h0, int w0, size_t off) {
        a.c[k] = LnClip{(u64)off, (u64)brow, (unsigned short)h0, (unsigned short)w0, (unsigned short)spacing_um[2 * b],
                        (unsigned short)spacing_um[2 * b + 1]};
        const int nbands = (h0 + LN_BAND_ROWS - 1) / LN_BAND_ROWS;
        brow += (size_t)T * (size_t)nbands;
        return nbands;
    }, [&](LnArgs& a, int b0, int nb) -> int {
        a.mask = mask; a.stats = reinterpret_cast<i64*>(stats); a.disks = reinterpret_cast<i64*>(disks); a.geom = geom;
        a.bands = reinterpret_cast<i64*>(bands);
        a.frame0 = (long long)b0 * T;
        a.nclips = nb; a.T = T; a.cls = cls; a.D = D;
        const long long fr = (long long)nb * T;
        hipLaunchKernelGGL(ln_moments_kernel, native_grid(fr * a.maxbands, LN_MAX_WG), dim3(LN_NT), 0, st, a);
        GDKVM_LAUNCH_CHECK("ln_moments_kernel");
        hipLaunchKernelGGL(ln_extent_kernel, native_grid(fr * a.maxbands, LN_MAX_WG), dim3(LN_NT), 0, st, a);
        GDKVM_LAUNCH_CHECK("ln_extent_kernel");
        hipLaunchKernelGGL(ln_disks_kernel, native_grid(fr * a.maxbands, LN_MAX_WG), dim3(LN_NT), 0, st, a);
        GDKVM_LAUNCH_CHECK("ln_disks_kernel");
        hipLaunchKernelGGL(ln_finish_kernel, native_grid(fr, LN_MAX_WG), dim3(64), 0, st, a);
        GDKVM_LAUNCH_CHECK("ln_finish_kernel");
        return GDKVM_OK;
    });
}
