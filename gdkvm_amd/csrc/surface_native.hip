// surface_native.hip -- surface distances in micrometres between one class of a predicted mask and of its target at every clip's own frame
// size (h0, w0) (what HD, HD95 and ASSD in mm at native resolution are made of; eval.py's native.surface block).  include/gdkvm.h holds the
// definition (gdkvm_surface_distance_native); every output is an integer that depends on neither the algorithm nor the schedule.
//
// The buffers are ragged: native_clips.hpp holds the launcher's side of that; a clip's entry here is (pixel offset, bitmap offset, h0, w0,
// ry, rx).  Nothing copied, nothing allocated, nothing synchronised.
//
// A frame's work is spread over many workgroups by FOUR kernels in stream order; a kernel reads what an earlier KERNEL wrote and nothing
// that another workgroup of its own launch writes: no flag, no spinning, no fence anybody polls.
//   (a) sn_surfaces   per (clip, frame, band of SN_BAND_ROWS rows): the class bits of the band's rows and of one halo row above and below
//       (read, not owned) go to LDS, 16 bytes per load on the 16-byte grid of the addresses (mask_frame.hpp's sweep; the bits are OR-ed
//       into the rows' words with workgroup atomics, whose order no bit depends on); the two SURFACE bitmaps S(A), S(B) of the band's
//       own rows go to the workspace.  A bitmap row is ceil(w0 / 32) whole words, so no two bands (and no two frames) write one word; bits past w0 are 0.
//       The band's nA, nB go to the frame's count slots.  One writer per global word and per slot.
//   (b) sn_columns    per (clip, frame, direction, strip of SN_STRIP columns), one lane per column: sweeps down, then up, and writes the row
//       count to the nearest pixel of the OTHER surface in its column as a 16-bit word (<= 2047; 0xffff: none) into the direction's plane.
//       The sweeps are latency, not bytes: SN_SWEEP rows' loads are issued together and the carried count runs through them in order.
//   (c) sn_rows       per (clip, frame, direction, band): the pixels of THIS surface's bitmap are queued in LDS, the words of SN_NT lanes
//       at a time, and then ONE LANE PER SURFACE PIXEL walks outwards along the row with the early stop of surface_distance.hip's
//       directed_distance, SN_WALK steps' loads in flight together.  It writes (dy, dx) of the nearest pixel, 11 bits each, to the frame's
//       COMPACTED list: d2 = (ry dy)^2 + (rx dx)^2 is recomputed from it.  A band's values start at the sum of the counts of the bands
//       above it; inside the band a lane takes its places in the queue from a workgroup counter in LDS (an integer atomic).  So the ORDER
//       of a band's values in the list depends on the schedule; every output is a function of the MULTISET (maxima, sums, ranks), and
//       nothing else rests on an atomic.
//   (d) sn_finish     per frame, one workgroup: maxima and isqrt sums per direction, the two ranks by bisection on the value over the list
//       (typically a few thousand values), and the record.  A frame with an empty surface skips (b) and (c) and gets its record here.
// No floating point except the isqrt estimate (sn_isqrt: operands below 2^63).  The workspace is scratch and is never assumed zeroed:
// every word that is read was written by an earlier kernel of the same call.
//
// Loop bounds.  (a): the vectors count to (SN_BAND_ROWS + 2) w0 / 16 / 256 per lane, a vector's bits are cut at most 16 times, the words
// count to SN_BAND_ROWS ceil(w0 / 32) / 256.
// (b): 2 h0 steps.  (c): the words of a band / 256 rounds, in each at most 32 pixels queued and 32 walked per lane, a walk at most
// max(x, w0 - 1 - x) + SN_WALK - 1 <= 2050 steps; the prefix over at most 64 bands is one wave reduction.  (d): the frame's surface
// count n / 256 per pass, at most 2 + SN_D2BITS passes.
// Every kernel takes further items grid-stride past SN_MAX_WG workgroups.
// Worst case, from the code: a 2048^2 checkerboard (every pixel of the class is surface, 2^21 of them) against one far pixel.  (a) and
// (b) do not depend on the content.  (c): every walk runs until k^2 rx^2 reaches the pixel's distance to that one pixel, up to 2047 steps
// of two 16-bit loads: 2^21 * 2047 * 2 = 8.6 G loads, over 64 bands x 256 lanes.  (d): n = 2^21 + 1 values, 49 passes of n / 256 = 8193
// trips per lane, in ONE workgroup per frame.  Slow, bounded, and only (d) is not spread.

#include "native_clips.hpp"

namespace {

typedef long long i64;
typedef unsigned long long u64;

constexpr int SN_NT = 256;
constexpr int SN_BAND_ROWS = GDKVM_SURFACE_NATIVE_BAND_ROWS;   // rows of a band (gdkvm.h)
constexpr int SN_STRIP = GDKVM_SURFACE_NATIVE_STRIP;           // columns of a strip: one wave
constexpr int SN_MAX_WG = GDKVM_SURFACE_NATIVE_MAX_WG;         // workgroups per launch; more items than that are walked grid-stride
constexpr int SN_CLIPS = GDKVM_SURFACE_NATIVE_CLIPS;           // clips per launch
constexpr int SN_MAX_BANDS = NATIVE_MAX_SIDE / SN_BAND_ROWS;   // 64: a frame's count slots, and one wave sums them
constexpr int SN_MAX_WPR = NATIVE_MAX_SIDE / 32;               // words of a bitmap row
constexpr unsigned SN_NONE = 0xffffu;                          // g of a column without a pixel of the other surface
constexpr int SN_SWEEP = 8;                                    // rows of a column sweep whose loads are in flight together
constexpr int SN_WALK = 4;                                     // steps of a row walk whose loads are in flight together
constexpr int SN_D2BITS = 47;                                  // d2 <= 2 (2047 * 4095)^2 < 2^47
static_assert(SN_STRIP == 64, "a strip is one wave's columns");
static_assert(SN_MAX_BANDS <= 64, "one wave sums a frame's band counts");
static_assert(SN_BAND_ROWS <= 32, "a queued pixel is its row of the band in 5 bits above its column in 11");

struct SnClip {
    u64 off, woff;                                         // the clip's first pixel in mask / target / a plane, its first word in a bitmap
    unsigned short h0, w0, ry, rx;
};
struct SnArgs {
    const uint8_t* mask; const uint8_t* target; i64* surf;
    unsigned* counts;                                      // [frames][SN_MAX_BANDS][2]
    unsigned* bm[2];                                       // S(A), S(B)
    unsigned short* g[2];                                  // [0]: rows to the nearest pixel of S(B), [1]: of S(A)
    unsigned* list;                                        // two entries per pixel: a frame's values start at twice its pixel offset
    long long frame0;                                      // the launch's first frame of the call
    int nclips, T, cls, maxbands, maxstrips;
    SnClip c[SN_CLIPS];
};
static_assert(sizeof(SnArgs) <= 2048, "the clip table travels in the kernel arguments");

// floor(sqrt(n)) for n < 2^63: the root is below 2^31.5, the fp64 estimate (operand rounded to 53 bits, root rounded once) is off by at
// most one either way, and (r + 1)^2 < 2^64
__device__ __forceinline__ u64 sn_isqrt(u64 n)
{
    u64 r = (u64)sqrt((double)n);
    if (r * r > n) --r;
    if ((r + 1) * (r + 1) <= n) ++r;
    return r;
}

__device__ __forceinline__ u64 sn_d2(unsigned e, u64 ry2, u64 rx2)
{
    const unsigned dy = e >> 11, dx = e & 0x7ffu;
    return (u64)(dy * dy) * ry2 + (u64)(dx * dx) * rx2;    // (< 2^22 * 2^24 each)
}

// (nA, nB) of a frame and the counts of the bands above `band`, in every lane of the calling wave: lane l holds band l's slots
__device__ __forceinline__ void sn_frame_counts(const unsigned* cnt, int nbands, int band, unsigned& nA, unsigned& nB, unsigned& pA, unsigned& pB)
{
    const int lane = threadIdx.x & 63;
    const unsigned a = lane < nbands ? cnt[2 * lane] : 0u, b = lane < nbands ? cnt[2 * lane + 1] : 0u;
    nA = wave_sum(a); nB = wave_sum(b);
    pA = wave_sum(lane < band ? a : 0u); pB = wave_sum(lane < band ? b : 0u);
}

// (a) the surface bitmaps and the counts of one band
__global__ __launch_bounds__(SN_NT) void sn_surfaces_kernel(SnArgs a)
{
    __shared__ unsigned s_c[2][(SN_BAND_ROWS + 2) * SN_MAX_WPR];
    __shared__ unsigned s_n[SN_NT / 64][2];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const unsigned cls = (unsigned)a.cls;
    const long long per_clip = (long long)a.T * a.maxbands, items = per_clip * a.nclips;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const auto [clip, t, band] = native_item(item, per_clip, a.maxbands);
        const SnClip c = a.c[clip];
        const int h0 = c.h0, w0 = c.w0, wpr = (w0 + 31) >> 5, nbands = (h0 + SN_BAND_ROWS - 1) / SN_BAND_ROWS;
        if (band >= nbands) continue;                      // (uniform: a smaller clip of the launch has fewer bands)
        const int row0 = band * SN_BAND_ROWS, rows = h0 - row0 < SN_BAND_ROWS ? h0 - row0 : SN_BAND_ROWS;
        const size_t fpix = (size_t)c.off + (size_t)t * (size_t)(h0 * w0), fword = (size_t)c.woff + (size_t)t * (size_t)(h0 * wpr);
        const uint8_t* src[2] = {a.mask + fpix, a.target + fpix};
        // LDS row r holds native row row0 - 1 + r; a row outside the frame is zeros.  The staged rows ra .. rb - 1 are one run of bytes
        // at any address: mask_frame.hpp's sweep (head bytes, 16-byte vectors, tail bytes), every 16 match bits OR-ed into the rows'
        // words, cut where a row ends
        const int ra = row0 > 0 ? row0 - 1 : 0, rb = row0 + rows + 1 < h0 ? row0 + rows + 1 : h0;
        for (int i = tid; i < (rows + 2) * wpr; i += SN_NT) { s_c[0][i] = 0u; s_c[1][i] = 0u; }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const FrameWords<true, int> M{&s_c[s][(ra - (row0 - 1)) * wpr]};
            MaskFrame<SN_NT>(src[s] + ra * w0, (rb - ra) * w0, w0, cls).sweep_bits([&](unsigned m, int p0) {
                if (!m) return;
                int y = p0 / w0, x = p0 - y * w0;          // (of the staged run)
                while (m) {                                // (at most 16 turns: every turn ends a row)
                    const int n = w0 - x;                  // the pixels left in this row
                    const unsigned part = n >= 16 ? m : m & ((1u << n) - 1u);
                    if (part) {
                        const int idx = y * wpr + (x >> 5), sh = x & 31;
                        M.aor(idx, part << sh);
                        if (sh > 16 && (part >> (32 - sh))) M.aor(idx + 1, part >> (32 - sh));      // (pixels below w0: a word of this row)
                    }
                    if (n >= 16) break;
                    m >>= n; x = 0; ++y;
                }
            });
        }
        __syncthreads();
        unsigned cnt[2] = {0u, 0u};
        for (int i = tid; i < rows * wpr; i += SN_NT) {
            const int r = i / wpr + 1, wi = i - (r - 1) * wpr;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const unsigned* row = &s_c[s][r * wpr];
                const unsigned m = row[wi];
                const unsigned lt = (m << 1) | (wi > 0 ? row[wi - 1] >> 31 : 0u), rt = (m >> 1) | (wi + 1 < wpr ? row[wi + 1] << 31 : 0u);
                const unsigned sf = m & ~(lt & rt & row[wi - wpr] & row[wi + wpr]);
                a.bm[s][fword + (size_t)(row0 + r - 1) * wpr + wi] = sf;
                cnt[s] += (unsigned)__builtin_popcount(sf);
            }
        }
        cnt[0] = wave_sum(cnt[0]); cnt[1] = wave_sum(cnt[1]);
        if (lane == 0) { s_n[wv][0] = cnt[0]; s_n[wv][1] = cnt[1]; }
        __syncthreads();                                   // (also: the next item writes the same LDS rows)
        if (tid < 2) a.counts[((size_t)a.frame0 + (size_t)clip * a.T + t) * (2 * SN_MAX_BANDS) + 2 * band + tid] = wg_sum(s_n, tid);
        __syncthreads();
    }
}

// (b) the vertical distances of one strip of columns in one direction
__global__ __launch_bounds__(64) void sn_columns_kernel(SnArgs a)
{
    const int lane = threadIdx.x;
    const long long per_frame = 2ll * a.maxstrips, per_clip = per_frame * a.T, items = per_clip * a.nclips;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int clip = (int)(item / per_clip);
        const long long rem = item - clip * per_clip;
        const int t = (int)(rem / per_frame), rest = (int)(rem - t * per_frame), dir = rest / a.maxstrips, strip = rest - dir * a.maxstrips;
        const SnClip c = a.c[clip];
        const int h0 = c.h0, w0 = c.w0, wpr = (w0 + 31) >> 5, nbands = (h0 + SN_BAND_ROWS - 1) / SN_BAND_ROWS;
        if (strip * SN_STRIP >= w0) continue;              // (uniform)
        unsigned nA, nB, pA, pB;
        sn_frame_counts(a.counts + ((size_t)a.frame0 + (size_t)clip * a.T + t) * (2 * SN_MAX_BANDS), nbands, 0, nA, nB, pA, pB);
        if (nA == 0 || nB == 0) continue;                  // (uniform) no surface distance: nobody reads the planes
        const int x = strip * SN_STRIP + lane;
        if (x >= w0) continue;                             // (nothing behind this in the loop's body crosses lanes)
        const size_t fpix = (size_t)c.off + (size_t)t * (size_t)(h0 * w0), fword = (size_t)c.woff + (size_t)t * (size_t)(h0 * wpr);
        const unsigned* __restrict__ O = a.bm[dir ^ 1] + fword + (x >> 5);        // the OTHER surface: column x's word of row 0
        unsigned short* G = a.g[dir] + fpix + x;
        const unsigned sh = (unsigned)x & 31u;
        // SN_SWEEP rows at a time: their loads are issued together, the carried count runs through them in order
        unsigned d = SN_NONE;
        for (int y0 = 0; y0 < h0; y0 += SN_SWEEP) {
            unsigned wv[SN_SWEEP];
#pragma unroll
            for (int j = 0; j < SN_SWEEP; ++j) wv[j] = y0 + j < h0 ? O[(size_t)(y0 + j) * wpr] : 0u;
#pragma unroll
            for (int j = 0; j < SN_SWEEP; ++j) {
                if (y0 + j >= h0) break;
                if ((wv[j] >> sh) & 1u) d = 0;
                else if (d != SN_NONE) ++d;                // (d <= h0 - 1 <= 2047 < NONE)
                G[(size_t)(y0 + j) * w0] = (unsigned short)d;
            }
        }
        d = SN_NONE;
        for (int y1 = h0 - 1; y1 >= 0; y1 -= SN_SWEEP) {
            unsigned wv[SN_SWEEP], gv[SN_SWEEP];
#pragma unroll
            for (int j = 0; j < SN_SWEEP; ++j) {
                wv[j] = y1 - j >= 0 ? O[(size_t)(y1 - j) * wpr] : 0u;
                gv[j] = y1 - j >= 0 ? (unsigned)G[(size_t)(y1 - j) * w0] : 0u;     // (the lane's own store of the sweep down)
            }
#pragma unroll
            for (int j = 0; j < SN_SWEEP; ++j) {
                if (y1 - j < 0) break;
                if ((wv[j] >> sh) & 1u) d = 0;
                else if (d != SN_NONE) ++d;
                if (d < gv[j]) G[(size_t)(y1 - j) * w0] = (unsigned short)d;
            }
        }
    }
}

// (c) the nearest pixel of the other surface for the pixels of this surface in one band
__global__ __launch_bounds__(SN_NT) void sn_rows_kernel(SnArgs a)
{
    __shared__ unsigned s_cnt;
    __shared__ unsigned short s_q[32 * SN_NT];             // the surface pixels of SN_NT bitmap words: row of the band << 11 | column
    const int tid = threadIdx.x;
    const long long per_frame = 2ll * a.maxbands, per_clip = per_frame * a.T, items = per_clip * a.nclips;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int clip = (int)(item / per_clip);
        const long long rem = item - clip * per_clip;
        const int t = (int)(rem / per_frame), rest = (int)(rem - t * per_frame), dir = rest / a.maxbands, band = rest - dir * a.maxbands;
        const SnClip c = a.c[clip];
        const int h0 = c.h0, w0 = c.w0, wpr = (w0 + 31) >> 5, nbands = (h0 + SN_BAND_ROWS - 1) / SN_BAND_ROWS;
        if (band >= nbands) continue;                      // (uniform)
        unsigned nA, nB, pA, pB;
        sn_frame_counts(a.counts + ((size_t)a.frame0 + (size_t)clip * a.T + t) * (2 * SN_MAX_BANDS), nbands, band, nA, nB, pA, pB);
        if (nA == 0 || nB == 0) continue;                  // (uniform)
        const int row0 = band * SN_BAND_ROWS, rows = h0 - row0 < SN_BAND_ROWS ? h0 - row0 : SN_BAND_ROWS;
        const size_t fpix = (size_t)c.off + (size_t)t * (size_t)(h0 * w0), fword = (size_t)c.woff + (size_t)t * (size_t)(h0 * wpr);
        const unsigned* S = a.bm[dir] + fword + (size_t)row0 * wpr;
        const unsigned short* G = a.g[dir] + fpix + (size_t)row0 * w0;
        unsigned* L = a.list + 2 * fpix + (dir ? nA + pB : pA);      // the band's places: behind those of the bands above it
        const u64 ry2 = (u64)((unsigned)c.ry * c.ry), rx2 = (u64)((unsigned)c.rx * c.rx);
        const int nwords = rows * wpr;
        // SN_NT words at a time: their pixels are queued in LDS (a lane takes its places from the counter), then every lane walks for
        // one queued pixel at a time, so that a word full of surface pixels is the work of 32 lanes and not of one
        for (int base = 0; base < nwords; base += SN_NT) { // (uniform)
            if (tid == 0) s_cnt = 0;
            __syncthreads();
            const int i = base + tid;
            if (i < nwords) {
                const unsigned m = S[i];                   // (the band's rows are one run of words)
                if (m) {
                    const int r = i / wpr, wi = i - r * wpr;
                    unsigned pos = atomicAdd(&s_cnt, (unsigned)__builtin_popcount(m));
                    visit_p(m, 32 * wi, [&](int x) { s_q[pos++] = (unsigned short)(r << 11 | x); });     // (x < w0: the bits past w0 are 0)
                }
            }
            __syncthreads();
            const unsigned total = s_cnt;                  // (<= 32 SN_NT)
            for (unsigned q = tid; q < total; q += SN_NT) {
                const int x = s_q[q] & 0x7ff;
                const unsigned short* row = G + (size_t)(s_q[q] >> 11) * w0;
                const unsigned g0 = row[x];
                u64 best = g0 == SN_NONE ? ~(u64)0 : (u64)(g0 * g0) * ry2;
                unsigned e = g0 == SN_NONE ? 0u : g0 << 11;
                const int kmax = x > w0 - 1 - x ? x : w0 - 1 - x;
                // SN_WALK steps at a time.  The stop is tested at the first of them: a later step of the group with k^2 rx^2 >= best
                // offers nothing below best, and a step past either end of the row offers NONE
                for (int k = 1; k <= kmax; k += SN_WALK) {
                    if ((u64)(unsigned)(k * k) * rx2 >= best) break;
                    unsigned gl[SN_WALK], gr[SN_WALK];
#pragma unroll
                    for (int j = 0; j < SN_WALK; ++j) {
                        gl[j] = x - k - j >= 0 ? (unsigned)row[x - k - j] : SN_NONE;
                        gr[j] = x + k + j < w0 ? (unsigned)row[x + k + j] : SN_NONE;
                    }
#pragma unroll
                    for (int j = 0; j < SN_WALK; ++j) {
                        const u64 kk = (u64)(unsigned)((k + j) * (k + j)) * rx2;
                        const u64 vl = kk + (u64)(gl[j] * gl[j]) * ry2, vr = kk + (u64)(gr[j] * gr[j]) * ry2;
                        if (gl[j] != SN_NONE && vl < best) { best = vl; e = gl[j] << 11 | (unsigned)(k + j); }
                        if (gr[j] != SN_NONE && vr < best) { best = vr; e = gr[j] << 11 | (unsigned)(k + j); }
                    }
                }
                L[q] = e;                                  // (the other surface is not empty: a pixel was found)
            }
            L += total;
            __syncthreads();                               // (the next words reset the counter and refill the queue)
        }
    }
}

// (d) one frame's record from its list
__global__ __launch_bounds__(SN_NT) void sn_finish_kernel(SnArgs a)
{
    constexpr int NW = SN_NT / 64;
    __shared__ u64 s_h[NW][2], s_s[NW][2], s_c[NW][2];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const long long items = (long long)a.nclips * a.T;
    for (long long item = blockIdx.x; item < items; item += gridDim.x) {
        const int clip = (int)(item / a.T), t = (int)(item - (long long)clip * a.T);
        const SnClip c = a.c[clip];
        const int h0 = c.h0, w0 = c.w0, nbands = (h0 + SN_BAND_ROWS - 1) / SN_BAND_ROWS;
        const size_t f = (size_t)a.frame0 + (size_t)item;
        i64* out = a.surf + f * 8;
        unsigned nA, nB, pA, pB;
        sn_frame_counts(a.counts + f * (2 * SN_MAX_BANDS), nbands, 0, nA, nB, pA, pB);
        if (nA == 0 || nB == 0) {                          // (uniform) no surface distance
            if (tid < 8) out[tid] = tid == 0 ? (i64)nA : tid == 1 ? (i64)nB : 0;
            continue;
        }
        const unsigned* L = a.list + 2 * ((size_t)c.off + (size_t)t * (size_t)(h0 * w0));
        const u64 ry2 = (u64)((unsigned)c.ry * c.ry), rx2 = (u64)((unsigned)c.rx * c.rx);
        const unsigned n = nA + nB;                        // (<= 2^23)
        u64 h[2] = {0, 0}, s[2] = {0, 0};
#pragma unroll 4
        for (unsigned i = tid; i < n; i += SN_NT) {
            const u64 d2 = sn_d2(L[i], ry2, rx2), r = sn_isqrt(d2 << 16);      // (d2 2^16 < 2^63; a term below 2^32, a sum below 2^54)
            const bool ba = i >= nA;                       // the values of S(A) come first
            h[0] = !ba && d2 > h[0] ? d2 : h[0]; s[0] += ba ? 0 : r;
            h[1] = ba && d2 > h[1] ? d2 : h[1]; s[1] += ba ? r : 0;
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) { h[k] = wave_max(h[k]); s[k] = wave_sum(s[k]); }
        if (lane == 0) { s_h[wv][0] = h[0]; s_h[wv][1] = h[1]; s_s[wv][0] = s[0]; s_s[wv][1] = s[1]; }
        __syncthreads();
        u64 hAB = 0, hBA = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) { hAB = s_h[w][0] > hAB ? s_h[w][0] : hAB; hBA = s_h[w][1] > hBA ? s_h[w][1] : hBA; }
        const u64 sAB = wg_sum(s_s, 0), sBA = wg_sum(s_s, 1);
        // count(m) = the pooled values <= m, and the smallest pooled value above m
        auto count = [&](u64 m, u64& above) -> unsigned {
            u64 cn = 0, mn = ~(u64)0;
#pragma unroll 4
            for (unsigned i = tid; i < n; i += SN_NT) {
                const u64 d2 = sn_d2(L[i], ry2, rx2);
                cn += d2 <= m ? 1u : 0u;
                mn = (d2 > m && d2 < mn) ? d2 : mn;
            }
            cn = wave_sum(cn); mn = wave_min(mn);
            __syncthreads();                               // (the reads of the count before)
            if (lane == 0) { s_c[wv][0] = cn; s_c[wv][1] = mn; }
            __syncthreads();
            mn = ~(u64)0;
#pragma unroll
            for (int w = 0; w < NW; ++w) mn = s_c[w][1] < mn ? s_c[w][1] : mn;
            above = mn;
            return (unsigned)wg_sum(s_c, 0);
        };
        const unsigned lo = (unsigned)((95ull * (n - 1)) / 100ull), hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
        u64 vlo = 0, vhi = hAB > hBA ? hAB : hBA, above;
        for (int it = 0; it < SN_D2BITS && vlo < vhi; ++it) {      // (uniform) the smallest v with count(v) > lo
            const u64 mid = (vlo + vhi) >> 1;
            if (count(mid, above) > lo) vhi = mid;
            else vlo = mid + 1;
        }
        const u64 q_lo = vlo;
        const unsigned c_lo = count(q_lo, above);
        const u64 q_hi = c_lo > hi ? q_lo : above;         // (c_lo <= hi <= n - 1: a pooled value above q_lo exists)
        if (tid == 0) {
            out[0] = (i64)nA; out[1] = (i64)nB; out[2] = (i64)hAB; out[3] = (i64)hBA;
            out[4] = (i64)sAB; out[5] = (i64)sBA; out[6] = (i64)q_lo; out[7] = (i64)q_hi;
        }
        __syncthreads();                                   // (the next item's partials)
    }
}

inline size_t sn_up16(size_t n) { return (n + 15) & ~(size_t)15; }
// The carve of the workspace for `frames` frames of `pixels` pixels and `rows` rows in all: the count slots, two bitmaps (a row is at most
// w0 / 32 + 1 words), two 16-bit planes, and the list of two 32-bit entries per pixel
struct SnCarve { size_t counts, bm, bm_bytes, g, g_bytes, list, total; };
inline SnCarve sn_carve(size_t frames, size_t pixels, size_t rows)
{
    SnCarve v;
    v.counts = 0;
    v.bm = sn_up16(frames * (2 * SN_MAX_BANDS) * sizeof(unsigned));
    v.bm_bytes = sn_up16((pixels / 32 + rows) * sizeof(unsigned));
    v.g = v.bm + 2 * v.bm_bytes;
    v.g_bytes = sn_up16(pixels * sizeof(unsigned short));
    v.list = v.g + 2 * v.g_bytes;
    v.total = v.list + sn_up16(2 * pixels * sizeof(unsigned));
    return v;
}

}  // namespace

extern "C" size_t gdkvm_surface_distance_native_workspace_bytes(int clips, int T, long long native_bytes, long long native_rows)
{
    if (clips < 1 || T < 1 || native_bytes < 1 || native_rows < 1 || (size_t)clips * (size_t)T > ((size_t)1 << 30) ||
        native_bytes > ((long long)1 << 52) || native_rows > ((long long)1 << 41))
        return 0;
    return sn_carve((size_t)clips * (size_t)T, (size_t)native_bytes, (size_t)native_rows).total;
}

extern "C" int gdkvm_surface_distance_native(const uint8_t* mask, const uint8_t* target, const int32_t* sizes, const int32_t* spacing_um,
                                             int64_t* surf, size_t native_bytes, void* workspace, size_t workspace_bytes, int clips, int T,
                                             int cls, void* stream)
{
    const char* name = "surface_distance_native";
    if (clips < 0 || T < 1) return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: bad arguments clips=%d T=%d (clips >= 0, T >= 1)", name, clips, T);
    if (int rc = mask_check_cls(name, GDKVM_ERR_SHAPE, cls)) return rc;
    if (clips == 0) return GDKVM_OK;
    if (!mask || !target || !sizes || !spacing_um || !surf)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: null pointer (mask, target, the host sizes, the host spacing_um and surf are required)", name);
    if (int rc = mask_check_aligned16(name, GDKVM_ERR_SHAPE, "surf", {surf})) return rc;
    size_t total, rows = 0;
    if (int rc = native_check_clips(name, "frames", sizes, spacing_um, native_bytes, clips, T, total)) return rc;
    for (int b = 0; b < clips; ++b) rows += (size_t)T * (size_t)sizes[2 * b];
    const size_t frames = (size_t)clips * (size_t)T;
    const SnCarve cv = sn_carve(frames, total, rows);
    if (!workspace || workspace_bytes < cv.total || !gdkvm_aligned16(workspace))
        return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: %zu frames of %zu pixels need a 16-byte aligned workspace of %zu bytes, got %zu", name, frames,
                          total, cv.total, workspace ? workspace_bytes : (size_t)0);
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* ws = static_cast<uint8_t*>(workspace);
    size_t woff = 0;                                       // carried from launch to launch, as the walk carries off
    return native_launches<SnArgs, SN_CLIPS>(sizes, clips, T, [&](SnArgs& a, int k, int b, int h0, int w0, size_t off) {
        a.c[k] = SnClip{(u64)off, (u64)woff, (unsigned short)h0, (unsigned short)w0, (unsigned short)spacing_um[2 * b],
                        (unsigned short)spacing_um[2 * b + 1]};
        const int nstrips = (w0 + SN_STRIP - 1) / SN_STRIP;
        if (nstrips > a.maxstrips) a.maxstrips = nstrips;  // (from 0: at least 1)
        woff += (size_t)T * (size_t)h0 * (size_t)((w0 + 31) >> 5);
        return (h0 + SN_BAND_ROWS - 1) / SN_BAND_ROWS;
    }, [&](SnArgs& a, int b0, int nb) -> int {
        a.mask = mask; a.target = target; a.surf = reinterpret_cast<i64*>(surf);
        a.counts = reinterpret_cast<unsigned*>(ws + cv.counts);
        a.bm[0] = reinterpret_cast<unsigned*>(ws + cv.bm); a.bm[1] = reinterpret_cast<unsigned*>(ws + cv.bm + cv.bm_bytes);
        a.g[0] = reinterpret_cast<unsigned short*>(ws + cv.g); a.g[1] = reinterpret_cast<unsigned short*>(ws + cv.g + cv.g_bytes);
        a.list = reinterpret_cast<unsigned*>(ws + cv.list);
        a.frame0 = (long long)b0 * T;
        a.nclips = nb; a.T = T; a.cls = cls;
        const long long fr = (long long)nb * T;
        hipLaunchKernelGGL(sn_surfaces_kernel, native_grid(fr * a.maxbands, SN_MAX_WG), dim3(SN_NT), 0, st, a);
        GDKVM_LAUNCH_CHECK("sn_surfaces_kernel");
        hipLaunchKernelGGL(sn_columns_kernel, native_grid(fr * 2 * a.maxstrips, SN_MAX_WG), dim3(64), 0, st, a);
        GDKVM_LAUNCH_CHECK("sn_columns_kernel");
        hipLaunchKernelGGL(sn_rows_kernel, native_grid(fr * 2 * a.maxbands, SN_MAX_WG), dim3(SN_NT), 0, st, a);
        GDKVM_LAUNCH_CHECK("sn_rows_kernel");
        hipLaunchKernelGGL(sn_finish_kernel, native_grid(fr, SN_MAX_WG), dim3(SN_NT), 0, st, a);
        GDKVM_LAUNCH_CHECK("sn_finish_kernel");
        return GDKVM_OK;
    });
}
