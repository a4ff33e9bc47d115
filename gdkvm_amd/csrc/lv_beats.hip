// lv_beats.hip -- the heart beats of a clip from its left-ventricular curve (the last link of the evaluation's chain vote -> largest -> fill ->
// measure -> beats): per clip the end-systoles of the area curve by scipy.signal.find_peaks' rules (strict local minima, distance, prominence),
// the end-diastole in front of each, one ejection fraction per beat and their mean.  include/gdkvm.h holds the definition.  Everything up to
// the per-beat EF is integer arithmetic on the curve in LDS.  ONE 256-lane workgroup per clip: no cross-workgroup traffic, no global atomics,
// no fences, no host read-back; every loop is bounded by T.

#include "mask_frame.hpp"

// No fused multiply-add in this file's own arithmetic, as in lv_measure.hip: the fp64 steps are the definition's operations, one rounding each.
#pragma clang fp contract(off)

namespace {

typedef long long i64;

constexpr int LB_MAX_T = 4096;       // frames of a clip: the curve (8 bytes a frame) and a state byte per frame live in LDS
constexpr int LB_MAX_M = LB_MAX_T / 2;   // strict local minima are never adjacent and never the first or last frame: fewer than T / 2
constexpr int LB_MAX_BEATS = 64;     // beats written out per clip (all of them are counted and averaged)
constexpr int LB_WAVE_BEATS = 32;    // up to this many end-systoles a wave searches one beat's end-diastole, beyond it a lane does

// a frame's state: no candidate / a candidate the distance rule has not decided / kept by it / dropped by it / an end-systole
enum : unsigned char { LB_NONE = 0, LB_OPEN = 1, LB_KEPT = 2, LB_DROPPED = 3, LB_SYSTOLE = 4 };

struct BeatsArgs {
    const i64* area; const double* vol; const int32_t* length;
    int32_t* beats; double* beat_val; int32_t* info; double* summ;
    int T, max_beats, distance, permille;
    i64 min_pixels;
};

__global__ __launch_bounds__(256) void lv_beats_kernel(BeatsArgs a)
{
    __shared__ i64 s_a[LB_MAX_T];
    __shared__ double s_ef[LB_MAX_M];
    __shared__ unsigned short s_es[LB_MAX_M], s_ed[LB_MAX_M];
    __shared__ unsigned char s_st[LB_MAX_T];
    __shared__ i64 s_red[4][3];
    __shared__ int s_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, T = a.T, mb = a.max_beats;
    const size_t b = blockIdx.x;
    const i64* ga = a.area + b * (size_t)T;
    const double* gv = a.vol + b * (size_t)T;
    int len = a.length ? a.length[b] : T;                  // (uniform) the frames behind len are padding and are never read
    len = len < 0 ? 0 : (len > T ? T : len);

    // the curve into LDS, with its extremes and the frames below min_pixels
    i64 lo = 0x7fffffffffffffffLL, hi = -0x7fffffffffffffffLL - 1, below = 0;
    for (int t = tid; t < len; t += 256) {
        const i64 v = ga[t];
        s_a[t] = v;
        s_st[t] = LB_NONE;
        lo = v < lo ? v : lo;
        hi = v > hi ? v : hi;
        below += v < a.min_pixels ? 1 : 0;
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    below = wave_sum(below);
    if (lane == 0) { s_red[wv][0] = lo; s_red[wv][1] = hi; s_red[wv][2] = below; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        lo = s_red[w][0] < lo ? s_red[w][0] : lo;
        hi = s_red[w][1] > hi ? s_red[w][1] : hi;
    }
    const int n_below = (int)wg_sum(s_red, 2);
    const i64 range = len > 0 ? hi - lo : 0;

    // 1. candidates: the lane of a plateau's first frame walks the plateau and marks its middle
    for (int t = tid; t < len; t += 256) {
        if (t == 0 || t >= len - 1) continue;
        const i64 v = s_a[t];
        if (!(s_a[t - 1] > v)) continue;
        int r = t;
        while (r + 1 < len && s_a[r + 1] == v) ++r;
        if (r + 1 < len && s_a[r + 1] > v) s_st[(t + r) >> 1] = LB_OPEN;
    }
    __syncthreads();

    // 2. distance: an open candidate drops itself once a rival in range is kept and keeps itself once every rival in range is dropped or of
    // lower priority (smaller area first, then the lower frame).  The states only ever move from open to decided, a decision is final and
    // is taken on what is already decided, so reading a rival's state while its lane writes it is harmless; the open candidate of the highest
    // priority decides in every turn, so the loop ends after at most as many turns as there are candidates.
    const int d = a.distance;
    for (int it = 0; it < LB_MAX_M; ++it) {
        int open = 0;
        for (int t = tid; t < len; t += 256) {
            if (s_st[t] != LB_OPEN) continue;
            const i64 v = s_a[t];
            const int q0 = t - d + 1 > 0 ? t - d + 1 : 0, q1 = t + d - 1 < len - 1 ? t + d - 1 : len - 1;
            bool drop = false, wait = false;
            for (int q = q0; q <= q1; ++q) {                       // (no early exit: the reads of a turn are independent of each other)
                const unsigned s = s_st[q];
                drop = drop || s == LB_KEPT;
                if (s == LB_OPEN && q != t) {
                    const i64 w = s_a[q];
                    wait = wait || w < v || (w == v && q < t);
                }
            }
            if (drop) s_st[t] = LB_DROPPED;
            else if (!wait) s_st[t] = LB_KEPT;
            else open = 1;
        }
        if (!__syncthreads_or(open)) break;
    }

    // 3. prominence of the kept candidates: two walks over the curve in LDS.  A deep minimum walks far (the deepest to both borders), so a
    // WAVE walks for one candidate, 64 frames a step: a wave takes every fourth run of 64 frames and serves its kept candidates in turn.
    for (int c0 = 64 * wv; c0 < len; c0 += 256) {
        unsigned long long todo = __ballot(c0 + lane < len && s_st[c0 + lane] == LB_KEPT);
        while (todo) {                                         // (wave-uniform)
            const int t = c0 + __builtin_ctzll(todo);
            todo &= todo - 1ull;
            const i64 v = s_a[t];
            i64 lmax = v, rmax = v;
            for (int j0 = t - 1; j0 >= 0; j0 -= 64) {          // the lanes look at frames j0, j0 - 1, ..: lane order is walking order
                const int j = j0 - lane;
                const i64 w = j >= 0 ? s_a[j] : v;
                const unsigned long long stop = __ballot(w < v);
                if (stop == 0 || lane < __builtin_ctzll(stop)) lmax = w > lmax ? w : lmax;
                if (stop) break;
            }
            for (int j0 = t + 1; j0 < len; j0 += 64) {
                const int j = j0 + lane;
                const i64 w = j < len ? s_a[j] : v;
                const unsigned long long stop = __ballot(w < v);
                if (stop == 0 || lane < __builtin_ctzll(stop)) rmax = w > rmax ? w : rmax;
                if (stop) break;
            }
            lmax = wave_max(lmax);
            rmax = wave_max(rmax);
            const i64 prom = (lmax < rmax ? lmax : rmax) - v;
            if (lane == 0 && prom * 1000 >= (i64)a.permille * range) s_st[t] = LB_SYSTOLE;
        }
    }
    __syncthreads();

    // the end-systoles in frame order: a ballot per wave, a prefix over the four waves, 256 frames a turn
    int m = 0;
    for (int t0 = 0; t0 < len; t0 += 256) {
        const int t = t0 + tid;
        const bool is = t < len && s_st[t] == LB_SYSTOLE;
        const unsigned long long bal = __ballot(is);
        if (lane == 0) s_cnt[wv] = __popcll(bal);
        __syncthreads();
        int off = m;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            off += w < wv ? s_cnt[w] : 0;
            m += s_cnt[w];
        }
        if (is) s_es[off + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)t;
        __syncthreads();
    }

    // 4. the end-diastole of beat j: the largest area in e_(j-1) + 1 .. e_j - 1 (never empty: two minima are never adjacent), the lowest frame
    // on a tie
    if (m <= LB_WAVE_BEATS) {
        for (int j = wv; j < m; j += 4) {
            const int f0 = j ? (int)s_es[j - 1] + 1 : 0, f1 = s_es[j];
            i64 best = -0x7fffffffffffffffLL - 1;
            int bt = 0x7fffffff;
            for (int t = f0 + lane; t < f1; t += 64) {
                const i64 v = s_a[t];
                if (bt == 0x7fffffff || v > best) { best = v; bt = t; }     // (t ascends within a lane: the strict comparison keeps the lowest t)
            }
            const i64 top = wave_max(best);
            const int ed = wave_min(bt != 0x7fffffff && best == top ? bt : 0x7fffffff);
            if (lane == 0) s_ed[j] = (unsigned short)ed;
        }
    } else {
        for (int j = tid; j < m; j += 256) {
            const int f0 = j ? (int)s_es[j - 1] + 1 : 0, f1 = s_es[j];
            i64 best = s_a[f0];
            int bt = f0;
            for (int t = f0 + 1; t < f1; ++t) {
                const i64 v = s_a[t];
                if (v > best) { best = v; bt = t; }
            }
            s_ed[j] = (unsigned short)bt;
        }
    }
    __syncthreads();

    // the counted beats: beat 0 only when its end-diastole is not frame 0 (the clip started inside that beat)
    const int drop0 = m > 0 && s_ed[0] == 0 ? 1 : 0, nb = m - drop0;
    int32_t* ob = a.beats + b * (size_t)mb * 2;
    double* ov = a.beat_val + b * (size_t)mb * 3;
    for (int k = tid; k < nb; k += 256) {
        const int ed = s_ed[k + drop0], es = s_es[k + drop0];
        const double EDV = gv[ed], ESV = gv[es];
        const double ef = EDV == 0.0 ? 0.0 : (EDV - ESV) / EDV;
        s_ef[k] = ef;
        if (k < mb) {
            ob[2 * k] = ed; ob[2 * k + 1] = es;
            ov[3 * k] = EDV; ov[3 * k + 1] = ESV; ov[3 * k + 2] = ef;
        }
    }
    for (int k = nb + tid; k < mb; k += 256) {
        ob[2 * k] = -1; ob[2 * k + 1] = -1;
        ov[3 * k] = 0.0; ov[3 * k + 1] = 0.0; ov[3 * k + 2] = 0.0;
    }
    __syncthreads();

    // 5. the clip's record: the EFs are added in ascending beat order by one lane
    if (tid == 0) {
        const int span = m > 0 ? (int)s_es[m - 1] - (int)s_es[0] : 0;
        int32_t* oi = a.info + b * 4;
        double* os = a.summ + b * 4;
        oi[0] = nb; oi[1] = m; oi[2] = n_below; oi[3] = span;
        if (nb == 0) {
            os[0] = os[1] = os[2] = os[3] = 0.0;
        } else {
            double sum = 0.0, emin = s_ef[0], emax = s_ef[0];
            for (int k = 0; k < nb; ++k) {
                const double e = s_ef[k];
                sum = sum + e;
                emin = e < emin ? e : emin;
                emax = e > emax ? e : emax;
            }
            os[0] = sum / (double)nb; os[1] = emin; os[2] = emax;
            os[3] = m < 2 ? 0.0 : (double)span / (double)(m - 1);
        }
    }
}

}  // namespace

extern "C" int gdkvm_lv_beats(const int64_t* area, const double* vol, const int32_t* length,
                              int32_t* beats, double* beat_val, int32_t* info, double* summ,
                              int B, int T, int max_beats, int distance, int prominence_permille, int64_t min_pixels, void* stream)
{
    if (B < 0 || T < 1 || T > LB_MAX_T) return gdkvm_fail(GDKVM_ERR_SHAPE, "lv_beats: bad shape B=%d T=%d (T in 1..%d)", B, T, LB_MAX_T);
    if (max_beats < 1 || max_beats > LB_MAX_BEATS)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "lv_beats: max_beats=%d outside 1..%d", max_beats, LB_MAX_BEATS);
    if (distance < 1 || distance > LB_MAX_T) return gdkvm_fail(GDKVM_ERR_SHAPE, "lv_beats: distance=%d outside 1..%d", distance, LB_MAX_T);
    if (prominence_permille < 0 || prominence_permille > 1000)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "lv_beats: prominence_permille=%d outside 0..1000", prominence_permille);
    if (B == 0) return GDKVM_OK;
    if (!area || !vol || !beats || !beat_val || !info || !summ) return gdkvm_fail(GDKVM_ERR_ARG, "lv_beats: null pointer");
    if (int rc = mask_check_aligned16("lv_beats", GDKVM_ERR_ARG, "outputs", {beats, beat_val, info, summ})) return rc;
    if ((reinterpret_cast<uintptr_t>(area) | reinterpret_cast<uintptr_t>(vol)) & 7u)
        return gdkvm_fail(GDKVM_ERR_ARG, "lv_beats: area and vol must be 8-byte aligned");
    if (reinterpret_cast<uintptr_t>(length) & 3u) return gdkvm_fail(GDKVM_ERR_ARG, "lv_beats: length must be 4-byte aligned");
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    BeatsArgs a{reinterpret_cast<const i64*>(area), vol, length, beats, beat_val, info, summ, T, max_beats, distance, prominence_permille,
                (i64)min_pixels};
    hipLaunchKernelGGL(lv_beats_kernel, dim3((unsigned)B), dim3(256), 0, st, a);
    GDKVM_LAUNCH_CHECK("lv_beats_kernel");
    return GDKVM_OK;
}
