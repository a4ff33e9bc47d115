// surface_distance.hip -- surface distances between one class of a predicted mask and of its target, on the device (what HD, HD95 and ASSD
// are made of; the evaluation's epilogue beside the Dice counts and the LV volumes).  include/gdkvm.h holds the definition; every output is
// an integer that depends on neither the algorithm nor the schedule.
//
// ONE workgroup per frame: no cross-workgroup synchronisation, no fences between workgroups, no flag anybody spins on.  A frame keeps one
// word per pixel (the plane, whole 16-byte vectors) and four bitmaps (A, B, S(A), S(B), bit p = pixel p = y W + x, whole 16-byte vectors
// each).  They live in LDS while the frame is small enough, otherwise in the frame's slice of the caller's workspace, where every access is
// an agent-scope relaxed atomic (served by L2, as in largest_component.hip).  A pixel's word holds g in its low 11 bits and d2 above them.
// A pixel of both surfaces has d2 = 0 in both directions, so one word per pixel serves both sets.
// Passes, a workgroup barrier between them:
//   1. the bitmaps are cleared.                2. A and B from the bytes (head / 16-byte vectors / tail), OR-ed in 16 bits at a time.
//   3. S(A), S(B): one lane per bitmap word, four neighbour bits per pixel of the set; nA, nB.  An empty surface ends the frame here.
//   4. per direction (S(A) against S(B), then S(B) against S(A)) the exact Euclidean distance, separable, integers only:
//      columns  one lane per column sweeps down, then up: g[y][x] = the vertical distance in ROWS to the nearest pixel of the OTHER surface
//               in column x (NONE when the column has none).
//      rows     one lane per pixel of THIS surface: d2 = min over x' of the squared distance to (x', y -+ g[y][x']), walking outwards from x
//               and stopping once the horizontal part alone reaches the best so far.
//   5. maxima, the fixed-point sums, and every word becomes multiplicity (0, 1 or 2 surfaces) << D2BITS | d2.
//   6. the two ranks by bisection on the value: each step is one workgroup-wide count of d2 <= m over the words, 16 bytes per lane and read.
// Loop bounds: the sweeps count to H, the walks to W, the strided loops to H W / lanes, the bisection to D2BITS.
//
// Two forms of the pixel's word, one kernel body (SdPx and SdUm below): gdkvm_surface_distance counts in pixels, and
// gdkvm_surface_distance_mm brings a pixel spacing per frame (micrometres).  The form is a compile-time parameter, and all four
// instantiations are instruction for instruction what they were as two kernels (tools/isa_equal.py --kernels: kept).  That rests on each
// form's per-wave partials keeping their LDS layout and on the order in which each form folds them (the `if constexpr` in passes 3 and 6).

#include "mask_frame.hpp"

#include <atomic>

namespace {

typedef long long i64;
typedef unsigned long long u64;

constexpr unsigned SD_GBITS = 11;
constexpr unsigned SD_NONE = 0x7ffu;           // g of a column without a pixel of the other surface

struct SdArgs {
    const uint8_t* mask; const uint8_t* target; i64* surf; unsigned* ws;
    int H, W, HW, stride, cls;
};
struct SdUmArgs {
    const uint8_t* mask; const uint8_t* target; const int32_t* spacing; i64* surf; u64* ws;
    int H, W, HW, cls;
    size_t stride;                             // 64-bit words per frame of the workspace
};

// The frame's 32-bit words, and the bitmaps among them
template <bool LDS>
struct Words : FrameWords<LDS, int> {
    using FrameWords<LDS, int>::ld;
    // bit p of the bitmap that starts at word `bm`
    __device__ __forceinline__ bool bit(int bm, int p) const { return (ld(bm + (p >> 5)) >> (p & 31)) & 1u; }
};

// floor(sqrt(d2 << SH)): the operand is below 2^61 and its root below 2^31, so the fp64 estimate is off by at most one either way
template <int SH>
__device__ __forceinline__ u64 isqrt_q(u64 d2)
{
    const u64 n = d2 << SH;
    u64 r = (u64)sqrt((double)n);
    if (r * r > n) --r;
    if ((r + 1) * (r + 1) <= n) ++r;
    return r;
}

// The per-wave partials of a workgroup of NW waves in LDS, each form's in the layout its kernel had as separate 16-byte aligned arrays (in
// pixels the 32-bit partials share one).  n, h: the surface sizes and the maxima (column k of wave w); s: the sums; c: the count and the
// minimum of a bisection step in slot `turn`.
template <int NW>
struct SdPxPartials {
    alignas(16) unsigned u[2][NW][4];
    alignas(16) u64 s_[NW][2];
    __device__ __forceinline__ unsigned& n(int w, int k) { return u[0][w][k]; }
    __device__ __forceinline__ unsigned& h(int w, int k) { return u[1][w][k]; }
    __device__ __forceinline__ u64& s(int w, int k) { return s_[w][k]; }
    __device__ __forceinline__ unsigned& c(int turn, int w, int k) { return u[turn][w][2 + k]; }
};
template <int NW>
struct SdUmPartials {
    alignas(16) u64 c_[2][NW][2];
    alignas(16) u64 h_[NW][2];
    alignas(16) u64 s_[NW][2];
    alignas(16) unsigned n_[NW][2];
    __device__ __forceinline__ unsigned& n(int w, int k) { return n_[w][k]; }
    __device__ __forceinline__ u64& h(int w, int k) { return h_[w][k]; }
    __device__ __forceinline__ u64& s(int w, int k) { return s_[w][k]; }
    __device__ __forceinline__ u64& c(int turn, int w, int k) { return c_[turn][w][k]; }
};

// The pixel's word in pixels: 32 bits, g in the low 11 and d2 in the high 21 -- d2 < 2^21 and g <= 1023 or NONE fill it exactly.  4.5 bytes
// per pixel: frames of up to LDS_PIX pixels live in (static) LDS, 63 KiB of a workgroup's 64 KiB (the 112 x 112 mask of cfg2 takes 55 KiB),
// under 256 lanes.  The plane and the bitmaps are ONE array of 32-bit words, the bitmaps behind the plane.  NONE is squared like every
// other g: NONE^2 is above every real d2.  The weights are 1.
struct SdPx {
    typedef unsigned Word;
    typedef SdArgs Args;
    template <bool LDS> using Plane = Words<LDS>;
    template <int NW> using Partials = SdPxPartials<NW>;
    static constexpr bool SPACING = false, DYN_LDS = false;
    static constexpr unsigned D2BITS = 21;
    static constexpr int LDS_PIX = 14336, LDS_NT = 256;    // 4 * 14336 + 4 * 14336 / 8 = 64512 bytes
    static constexpr const char* REQUIRED = "mask, target and surf";
    __device__ static __forceinline__ bool none(unsigned) { return false; }
    __device__ static __forceinline__ unsigned vert(unsigned g, unsigned) { return g * g; }
    __device__ static __forceinline__ unsigned horiz(int k, unsigned) { return (unsigned)(k * k); }
    __device__ static __forceinline__ u64 root(unsigned d2) { return isqrt_q<32>(d2); }
    __device__ static __forceinline__ void unpack(const uint4& q, unsigned (&w)[4]) { w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w; }
    static Args args(const uint8_t* mask, const uint8_t* target, const int32_t*, i64* surf, void* ws, int H, int W, int cls, size_t stride)
    {
        return {mask, target, surf, static_cast<unsigned*>(ws), H, W, H * W, (int)stride, cls};
    }
};

// The pixel's word with a spacing: every frame brings its pixel's height ry and width rx in micrometres (1..4095), and a squared distance
// is (ry dy)^2 + (rx dx)^2 um^2, below 2^45.  64 bits: g in the low 11 as before (a count of ROWS), d2 in the 45 above them.  8.5 bytes
// per pixel: the 64-bit plane first, then the four bitmaps.  They live in dynamic LDS while the frame has at most
// GDKVM_SURFACE_MM_LDS_PIXELS pixels (153 KiB of the workgroup's 160 KiB; a 112 x 112 frame's 104 KiB leave room for ONE workgroup per CU,
// so it is a wide one: 1024 lanes).  NONE is tested for, not squared: with ry = 1 its square is below real distances.
struct SdUm {
    typedef u64 Word;
    typedef SdUmArgs Args;
    template <bool LDS> using Plane = FrameWords64<LDS, int>;
    template <int NW> using Partials = SdUmPartials<NW>;
    static constexpr bool SPACING = true, DYN_LDS = true;
    static constexpr unsigned D2BITS = 45;
    static constexpr int LDS_PIX = GDKVM_SURFACE_MM_LDS_PIXELS, LDS_NT = 1024;
    static constexpr const char* REQUIRED = "mask, target, spacing_um and surf";
    __device__ static __forceinline__ bool none(unsigned g) { return g == SD_NONE; }
    __device__ static __forceinline__ u64 vert(unsigned g, u64 ry2) { return (u64)(g * g) * ry2; }
    __device__ static __forceinline__ u64 horiz(int k, u64 rx2) { return (u64)(unsigned)(k * k) * rx2; }       // (< 2^20 * 2^24)
    __device__ static __forceinline__ u64 root(u64 d2) { return isqrt_q<16>(d2); }
    __device__ static __forceinline__ void unpack(const uint4& q, u64 (&w)[2]) { w[0] = ((u64)q.y << 32) | q.x; w[1] = ((u64)q.w << 32) | q.z; }
    static Args args(const uint8_t* mask, const uint8_t* target, const int32_t* spacing, i64* surf, void* ws, int H, int W, int cls, size_t stride)
    {
        return {mask, target, spacing, surf, static_cast<u64*>(ws), H, W, H * W, cls, stride};
    }
};

// words of one frame: the plane (whole 16-byte vectors of T::Word), then four bitmaps of 32-bit words (whole 16-byte vectors each)
template <class T>
__host__ __device__ inline int sd_plane_words(int HW) { return (HW + (int)(16 / sizeof(typename T::Word)) - 1) & ~((int)(16 / sizeof(typename T::Word)) - 1); }
__host__ __device__ inline int sd_bitmap_words(int HW) { return (((HW + 31) >> 5) + 3) & ~3; }
template <class T>
inline size_t sd_frame_bytes(int HW) { return sizeof(typename T::Word) * (size_t)sd_plane_words<T>(HW) + 16 * (size_t)sd_bitmap_words(HW); }
// words per frame in the workspace: the frame's bytes rounded up to 128, so that no two frames share a cache line
template <class T>
inline size_t sd_stride(int H, int W) { return ((sd_frame_bytes<T>(H * W) + 127) & ~(size_t)127) / sizeof(typename T::Word); }

// Pass 2 for one frame of bytes at any address: bits m of pixels p0 .. p0 + 15 are OR-ed into the bitmap at word bm.
template <bool LDS, int NT>
__device__ __forceinline__ void class_bitmap(const Words<LDS>& M, int bm, const uint8_t* base, int HW, int W, unsigned cls)
{
    MaskFrame<NT>(base, HW, W, cls).sweep_bits([&](unsigned m, int p0) {
        if (!m) return;
        const int s = p0 & 31;
        M.aor(bm + (p0 >> 5), m << s);
        if (s > 16 && (m >> (32 - s))) M.aor(bm + (p0 >> 5) + 1, m >> (32 - s));
    });
}

// Pass 3 for one set: surface word i from the set's bitmap at `bx` into the bitmap at `bs`; returns the lane's count of surface pixels
template <bool LDS, int NT>
__device__ __forceinline__ unsigned surface_bitmap(const Words<LDS>& M, int bx, int bs, int H, int W, int HW)
{
    unsigned cnt = 0;
    const int nw = (HW + 31) >> 5;
    for (int i = threadIdx.x; i < nw; i += NT) {
        unsigned m = M.ld(bx + i), s = 0;
        if (m) {
            const int p0 = 32 * i;
            int y = p0 / W, x = p0 - y * W, prev = 0;
            while (m) {                                    // (visit_xy written out: through the helper the registers are allocated differently)
                const int e = __builtin_ctz(m);
                m &= m - 1;
                x += e - prev;
                prev = e;
                while (x >= W) { x -= W; ++y; }
                const int p = p0 + e;
                const bool inner = x > 0 && x < W - 1 && y > 0 && y < H - 1 && M.bit(bx, p - 1) && M.bit(bx, p + 1) && M.bit(bx, p - W) &&
                                   M.bit(bx, p + W);
                if (!inner) s |= 1u << e;
            }
        }
        M.st(bs + i, s);
        cnt += (unsigned)__builtin_popcount(s);
    }
    return cnt;
}

// Pass 4 for one direction: g of the surface at `bo`, then d2 for the pixels of the surface at `bt`.  B holds the bitmaps, P the plane;
// ry2, rx2 = the squared spacings.  first: the words hold nothing yet.
template <class T, bool LDS, int NT>
__device__ __forceinline__ void directed_distance(const Words<LDS>& B, const typename T::template Plane<LDS>& P, int bt, int bo, int H, int W,
                                                  int HW, typename T::Word ry2, typename T::Word rx2, bool first)
{
    typedef typename T::Word Word;
    const int tid = threadIdx.x;
    for (int x = tid; x < W; x += NT) {
        unsigned d = SD_NONE;
        for (int y = 0, p = x; y < H; ++y, p += W) {
            if (B.bit(bo, p)) d = 0;
            else if (d != SD_NONE) ++d;                    // (d <= H - 1 <= 1023 < NONE)
            P.st(p, (first ? (Word)0 : (P.ld(p) & ~(Word)SD_NONE)) | d);
        }
        d = SD_NONE;
        for (int y = H - 1, p = (H - 1) * W + x; y >= 0; --y, p -= W) {
            if (B.bit(bo, p)) d = 0;
            else if (d != SD_NONE) ++d;
            const Word w = P.ld(p);
            if (d < ((unsigned)w & SD_NONE)) P.st(p, (w & ~(Word)SD_NONE) | d);
        }
    }
    __syncthreads();
    // while a lane replaces the d2 bits of its own word, other lanes read that word's g bits, which the (single) store leaves as they are
    for (int p = tid; p < HW; p += NT) {
        if (!B.bit(bt, p)) continue;
        const int y = p / W, x = p - y * W, row = p - x;
        const unsigned g0 = (unsigned)P.ld(p) & SD_NONE;
        Word best = T::none(g0) ? ~(Word)0 : T::vert(g0, ry2);
        const int kmax = x > W - 1 - x ? x : W - 1 - x;
        for (int k = 1; k <= kmax; ++k) {
            const Word kk = T::horiz(k, rx2);
            if (kk >= best) break;
            if (x - k >= 0) {
                const unsigned g = (unsigned)P.ld(row + x - k) & SD_NONE;
                const Word c = kk + T::vert(g, ry2);
                best = (!T::none(g) && c < best) ? c : best;
            }
            if (x + k < W) {
                const unsigned g = (unsigned)P.ld(row + x + k) & SD_NONE;
                const Word c = kk + T::vert(g, ry2);
                best = (!T::none(g) && c < best) ? c : best;
            }
        }
        P.st(p, (best << SD_GBITS) | g0);                  // (the other surface is not empty: best < 2^D2BITS)
    }
    __syncthreads();
}

template <class T, bool LDS, int NT>
__global__ __launch_bounds__(NT) void surface_distance_kernel(typename T::Args a)
{
    typedef typename T::Word Word;
    constexpr int NW = NT / 64, WPV = 16 / sizeof(Word);   // WPV words in a 16-byte vector
    constexpr Word D2MASK = ((Word)1 << T::D2BITS) - 1;    // pass 5 on: the low D2BITS bits are d2, the bits above the multiplicity
    uint4* mem = nullptr;                                  // the frame in LDS
    if constexpr (LDS && T::DYN_LDS) {
        extern __shared__ uint4 sd_dyn[];
        mem = sd_dyn;
    } else if constexpr (LDS) {
        __shared__ uint4 s_mem[(T::LDS_PIX + 4 * (T::LDS_PIX / 32)) / 4];
        mem = s_mem;
    }
    __shared__ typename T::template Partials<NW> s_u;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, H = a.H, W = a.W, HW = a.HW;
    const size_t f = blockIdx.x;
    const unsigned cls = (unsigned)a.cls;
    const int PW = sd_plane_words<T>(HW), BW = sd_bitmap_words(HW);
    const int b0 = T::SPACING ? 0 : PW;                    // the bitmaps: words of their own behind a 64-bit plane, or the plane's array
    const int bA = b0, bB = b0 + BW, bSA = b0 + 2 * BW, bSB = b0 + 3 * BW;
    i64* out;                                              // (in front of the spacing's early exit, or where the pixel form's code had it)
    int ry = 1, rx = 1;
    if constexpr (T::SPACING) {
        out = a.surf + f * 8;
        ry = a.spacing[2 * f]; rx = a.spacing[2 * f + 1];
        if (ry < 1 || ry > 4095 || rx < 1 || rx > 4095) {  // (uniform) no error can be returned from here: the record says so
            if (tid < 8) out[tid] = -1;
            return;
        }
    }
    const Word ry2 = (Word)(ry * ry), rx2 = (Word)(rx * rx);
    typename T::template Plane<LDS> P;
    if constexpr (LDS) P.w = reinterpret_cast<Word*>(mem);
    else P.w = a.ws + f * (size_t)a.stride;
    Words<LDS> M;
    if constexpr (T::SPACING) M.w = reinterpret_cast<unsigned*>(P.w + PW);
    else M.w = P.w;
    if constexpr (!T::SPACING) out = a.surf + f * 8;

    // pass 1, 2: the bitmaps
    for (int i = tid; i < 4 * BW; i += NT) M.st(b0 + i, 0u);
    __syncthreads();
    class_bitmap<LDS, NT>(M, bA, a.mask + f * (size_t)HW, HW, W, cls);
    class_bitmap<LDS, NT>(M, bB, a.target + f * (size_t)HW, HW, W, cls);
    __syncthreads();

    // pass 3: the surfaces and their sizes
    unsigned nA, nB;
    {
        const unsigned ca = wave_sum(surface_bitmap<LDS, NT>(M, bA, bSA, H, W, HW));
        const unsigned cb = wave_sum(surface_bitmap<LDS, NT>(M, bB, bSB, H, W, HW));
        if (lane == 0) { s_u.n(wv, 0) = ca; s_u.n(wv, 1) = cb; }
        __syncthreads();
        if constexpr (T::SPACING) {                        // (each form adds in the order its kernel had: the other order moves 52 lines
            nA = wg_sum(s_u.n_, 0); nB = wg_sum(s_u.n_, 1); // of the pixel LDS form's assembly, or 1064 of the mm LDS form's)
        } else {
            nA = nB = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) { nA += s_u.n(w, 0); nB += s_u.n(w, 1); }
        }
    }
    if (nA == 0 || nB == 0) {                              // (uniform) no surface distance
        if (tid < 8) out[tid] = tid == 0 ? (i64)nA : tid == 1 ? (i64)nB : 0;
        return;
    }

    // pass 4: both directions
    directed_distance<T, LDS, NT>(M, P, bSA, bSB, H, W, HW, ry2, rx2, true);
    directed_distance<T, LDS, NT>(M, P, bSB, bSA, H, W, HW, ry2, rx2, false);

    // pass 5: maxima, sums, and the words of the bisection (the words past H W up to the whole vector count nothing)
    Word hAB = 0, hBA = 0;
    {
        u64 sAB = 0, sBA = 0;
        for (int p = tid; p < PW; p += NT) {
            Word v = 0;
            if (p < HW) {
                const bool ina = M.bit(bSA, p), inb = M.bit(bSB, p);
                if (ina || inb) {
                    const Word d2 = P.ld(p) >> SD_GBITS;
                    const u64 r = T::root(d2);
                    if (ina) { hAB = d2 > hAB ? d2 : hAB; sAB += r; }
                    if (inb) { hBA = d2 > hBA ? d2 : hBA; sBA += r; }
                    v = ((Word)((ina ? 1u : 0u) + (inb ? 1u : 0u)) << T::D2BITS) | d2;
                }
            }
            P.st(p, v);
        }
        hAB = wave_max(hAB); hBA = wave_max(hBA);
        sAB = wave_sum(sAB); sBA = wave_sum(sBA);
        if (lane == 0) { s_u.h(wv, 0) = hAB; s_u.h(wv, 1) = hBA; s_u.s(wv, 0) = sAB; s_u.s(wv, 1) = sBA; }
        __syncthreads();
        hAB = hBA = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            hAB = s_u.h(w, 0) > hAB ? s_u.h(w, 0) : hAB;
            hBA = s_u.h(w, 1) > hBA ? s_u.h(w, 1) : hBA;
        }
    }

    // pass 6: the ranks.  count(m) = the pooled values <= m, and the smallest pooled value above m; the slots of the partials alternate, so
    // that one barrier per count is enough (a lane that is still reading slot k cannot meet a write before the barrier of the count in between)
    int turn = 0;
    auto count = [&](Word m, Word& above) -> unsigned {
        unsigned c = 0;
        Word mn = ~(Word)0;
        for (int i = tid; i < PW / WPV; i += NT) {
            Word w[WPV];
            if constexpr (LDS) {
                T::unpack(mem[i], w);
            } else {
#pragma unroll
                for (int e = 0; e < WPV; ++e) w[e] = P.ld(WPV * i + e);
            }
#pragma unroll
            for (int e = 0; e < WPV; ++e) {
                const Word d2 = w[e] & D2MASK;
                const unsigned mult = (unsigned)(w[e] >> T::D2BITS);
                c += d2 <= m ? mult : 0u;
                mn = (mult && d2 > m && d2 < mn) ? d2 : mn;
            }
        }
        c = wave_sum(c);
        mn = wave_min(mn);
        if (lane == 0) { s_u.c(turn, wv, 0) = c; s_u.c(turn, wv, 1) = mn; }
        __syncthreads();
        c = 0; mn = ~(Word)0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            c += (unsigned)s_u.c(turn, w, 0);
            mn = s_u.c(turn, w, 1) < mn ? s_u.c(turn, w, 1) : mn;
        }
        turn ^= 1;
        above = mn;
        return c;
    };
    const unsigned n = nA + nB, lo = (unsigned)((95ull * (n - 1)) / 100ull), hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
    Word vlo = 0, vhi = hAB > hBA ? hAB : hBA, above;
    for (int it = 0; it < (int)T::D2BITS && vlo < vhi; ++it) {     // (uniform) the smallest v with count(v) > lo
        const Word mid = (vlo + vhi) >> 1;
        if (count(mid, above) > lo) vhi = mid;
        else vlo = mid + 1;
    }
    const Word q_lo = vlo;
    const unsigned c_lo = count(q_lo, above);
    const Word q_hi = c_lo > hi ? q_lo : above;            // (c_lo <= hi <= n - 1: a pooled value above q_lo exists)

    if (tid == 0) {
        u64 sAB = 0, sBA = 0;
        if constexpr (!T::SPACING) {                       // (the pixel form adds its sums in front of the stores, the mm form between them)
            for (int w = 0; w < NW; ++w) { sAB += s_u.s(w, 0); sBA += s_u.s(w, 1); }
        }
        out[0] = (i64)nA; out[1] = (i64)nB; out[2] = (i64)hAB; out[3] = (i64)hBA;
        if constexpr (T::SPACING) { sAB = wg_sum(s_u.s_, 0); sBA = wg_sum(s_u.s_, 1); }
        out[4] = (i64)sAB; out[5] = (i64)sBA; out[6] = (i64)q_lo; out[7] = (i64)q_hi;
    }
}

// The workspace of `frames` frames: none while a frame lives in LDS
template <class T>
size_t sd_workspace_bytes(int frames, int H, int W)
{
    if (!mask_shape_ok(frames, H, W) || H * W <= T::LDS_PIX) return 0;
    return (size_t)frames * sd_stride<T>(H, W) * sizeof(typename T::Word);
}

// What gdkvm_surface_distance (T = SdPx, spacing_um unused) and gdkvm_surface_distance_mm (SdUm) share: the checks in their order under the
// entry point's name, and the launch of the form the frame's size selects
template <class T>
int sd_launch(const char* name, const char* kernel, const uint8_t* mask, const uint8_t* target, const int32_t* spacing_um, int64_t* surf,
              void* workspace, size_t workspace_bytes, int frames, int H, int W, int cls, void* stream)
{
    if (int rc = mask_check_shape(name, frames, H, W)) return rc;
    if (int rc = mask_check_cls(name, GDKVM_ERR_SHAPE, cls)) return rc;
    if (frames == 0) return GDKVM_OK;
    if (!mask || !target || (T::SPACING && !spacing_um) || !surf)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: null pointer (%s are required)", name, T::REQUIRED);
    if (T::SPACING && (reinterpret_cast<uintptr_t>(spacing_um) & 3u)) return gdkvm_fail(GDKVM_ERR_SHAPE, "%s: spacing_um must be 4-byte aligned", name);
    if (int rc = mask_check_aligned16(name, GDKVM_ERR_SHAPE, "surf", {surf})) return rc;
    const size_t need = sd_workspace_bytes<T>(frames, H, W);
    if (int rc = mask_check_workspace(name, H, W, need, workspace, workspace_bytes)) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const typename T::Args a = T::args(mask, target, spacing_um, reinterpret_cast<i64*>(surf), workspace, H, W, cls, sd_stride<T>(H, W));
    if (!need) {
        const size_t lds = T::DYN_LDS ? sd_frame_bytes<T>(H * W) : 0;
        if (lds > 32 * 1024) {                           // a large frame in dynamic LDS needs the opt-in once per device
            static std::atomic<unsigned long long> done_mask{0};
            int dev = 0;
            if (hipGetDevice(&dev) != hipSuccess) return gdkvm_fail(GDKVM_ERR_LAUNCH, "%s: hipGetDevice", name);
            const unsigned long long bit = 1ull << (dev & 63);
            if (!(done_mask.load(std::memory_order_relaxed) & bit)) {
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(surface_distance_kernel<T, true, T::LDS_NT>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)sd_frame_bytes<T>(T::LDS_PIX));
                if (e != hipSuccess) return gdkvm_fail(GDKVM_ERR_LAUNCH, "%s: LDS attribute: %s", name, hipGetErrorString(e));
                done_mask.fetch_or(bit, std::memory_order_relaxed);
            }
        }
        hipLaunchKernelGGL((surface_distance_kernel<T, true, T::LDS_NT>), dim3((unsigned)frames), dim3(T::LDS_NT), lds, st, a);
    } else {
        hipLaunchKernelGGL((surface_distance_kernel<T, false, 1024>), dim3((unsigned)frames), dim3(1024), 0, st, a);
    }
    GDKVM_LAUNCH_CHECK(kernel);
    return GDKVM_OK;
}

}  // namespace

extern "C" size_t gdkvm_surface_distance_workspace_bytes(int frames, int H, int W) { return sd_workspace_bytes<SdPx>(frames, H, W); }

extern "C" int gdkvm_surface_distance(const uint8_t* mask, const uint8_t* target, int64_t* surf, void* workspace, size_t workspace_bytes,
                                      int frames, int H, int W, int cls, void* stream)
{
    return sd_launch<SdPx>("surface_distance", "surface_distance_kernel", mask, target, nullptr, surf, workspace, workspace_bytes, frames, H, W,
                           cls, stream);
}

extern "C" size_t gdkvm_surface_distance_mm_workspace_bytes(int frames, int H, int W) { return sd_workspace_bytes<SdUm>(frames, H, W); }

extern "C" int gdkvm_surface_distance_mm(const uint8_t* mask, const uint8_t* target, const int32_t* spacing_um, int64_t* surf, void* workspace,
                                         size_t workspace_bytes, int frames, int H, int W, int cls, void* stream)
{
    return sd_launch<SdUm>("surface_distance_mm", "surface_distance_mm_kernel", mask, target, spacing_um, surf, workspace, workspace_bytes,
                           frames, H, W, cls, stream);
}
