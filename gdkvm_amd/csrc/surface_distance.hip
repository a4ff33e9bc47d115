// surface_distance.hip -- surface distances between one class of a predicted mask and of its target, on the device (what HD, HD95 and ASSD
// are made of; the evaluation's epilogue beside the Dice counts and the LV volumes).  include/gdkvm.h holds the definition; every output is
// an integer that depends on neither the algorithm nor the schedule.
//
// ONE workgroup per frame (256 lanes in the LDS form, 1024 in the workspace form): no cross-workgroup synchronisation, no fences between
// workgroups, no flag anybody spins on.  A frame keeps 4.5 bytes per pixel: one 32-bit word per pixel and four bitmaps (A, B, S(A), S(B), bit p
// = pixel p = y W + x).  They live in LDS while the frame has at most SD_LDS_PIX pixels (63 KiB of the workgroup's 64 KiB; the 112 x 112 mask
// of cfg2 takes 55 KiB), otherwise in the frame's slice of the caller's workspace, where every access is an agent-scope relaxed atomic (served
// by L2, as in largest_component.hip).  A pixel's word holds g in its low 11 bits and d2 in its high 21 -- d2 < 2^21 and g <= 1023 or NONE
// fill it exactly.  A pixel of both surfaces has d2 = 0 in both directions, so one word per pixel serves both sets.
// Passes, a workgroup barrier between them:
//   1. the bitmaps are cleared.                2. A and B from the bytes (head / 16-byte vectors / tail), OR-ed in 16 bits at a time.
//   3. S(A), S(B): one lane per bitmap word, four neighbour bits per pixel of the set; nA, nB.  An empty surface ends the frame here.
//   4. per direction (S(A) against S(B), then S(B) against S(A)) the exact Euclidean distance, separable, integers only:
//      columns  one lane per column sweeps down, then up: g[y][x] = the vertical distance to the nearest pixel of the OTHER surface in column
//               x (NONE when the column has none).
//      rows     one lane per pixel of THIS surface: d2 = min over x' of (x - x')^2 + g[y][x']^2, walking outwards from x and stopping once
//               (x - x')^2 reaches the best so far.
//   5. maxima, the fixed-point sums, and every word becomes multiplicity (0, 1 or 2 surfaces) << 21 | d2.
//   6. the two ranks by bisection on the value: each step is one workgroup-wide count of d2 <= m over the words, 16 bytes per lane and read.
// Loop bounds: the sweeps count to H, the walks to W, the strided loops to H W / lanes, the bisection to 21 (d2 < 2^21).
// gdkvm_surface_distance_mm, further down, is the same measurement with a pixel spacing per frame (micrometres; 64-bit words per pixel).

#include "mask_frame.hpp"

#include <atomic>

namespace {

typedef long long i64;
typedef unsigned long long u64;

constexpr int SD_LDS_PIX = 14336;              // frames of up to this many pixels live in LDS: 4 * 14336 + 4 * 14336 / 8 = 64512 bytes
constexpr unsigned SD_GBITS = 11;
constexpr unsigned SD_NONE = 0x7ffu;           // g of a column without a pixel of the other surface (NONE^2 is above every real d2)
constexpr unsigned SD_D2MASK = 0x1fffffu;      // pass 5 on: the low 21 bits are d2, the bits above the multiplicity

struct SdArgs {
    const uint8_t* mask; const uint8_t* target; i64* surf; unsigned* ws;
    int H, W, HW, stride, cls;
};

// words of one frame: the pixel words (whole 16-byte vectors), then four bitmaps (whole 16-byte vectors each)
__host__ __device__ inline int sd_plane_words(int HW) { return (HW + 3) & ~3; }
__host__ __device__ inline int sd_bitmap_words(int HW) { return (((HW + 31) >> 5) + 3) & ~3; }

// The frame's words, and the bitmaps among them
template <bool LDS>
struct Words : FrameWords<LDS, int> {
    using FrameWords<LDS, int>::ld;
    // bit p of the bitmap that starts at word `bm`
    __device__ __forceinline__ bool bit(int bm, int p) const { return (ld(bm + (p >> 5)) >> (p & 31)) & 1u; }
};

// floor(sqrt(d2 * 2^32)): the operand is below 2^53, so the fp64 estimate is off by at most one either way
__device__ __forceinline__ u64 isqrt_q32(unsigned d2)
{
    const u64 n = (u64)d2 << 32;
    u64 r = (u64)sqrt((double)n);
    if (r * r > n) --r;
    if ((r + 1) * (r + 1) <= n) ++r;
    return r;
}

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

// Pass 4 for one direction: g of the surface at `bo`, then d2 for the pixels of the surface at `bt`.  first: the words hold nothing yet.
template <bool LDS, int NT>
__device__ __forceinline__ void directed_distance(const Words<LDS>& M, int bt, int bo, int H, int W, int HW, bool first)
{
    const int tid = threadIdx.x;
    for (int x = tid; x < W; x += NT) {
        unsigned d = SD_NONE;
        for (int y = 0, p = x; y < H; ++y, p += W) {
            if (M.bit(bo, p)) d = 0;
            else if (d != SD_NONE) ++d;                    // (d <= H - 1 <= 1023 < NONE)
            M.st(p, (first ? 0u : (M.ld(p) & ~SD_NONE)) | d);
        }
        d = SD_NONE;
        for (int y = H - 1, p = (H - 1) * W + x; y >= 0; --y, p -= W) {
            if (M.bit(bo, p)) d = 0;
            else if (d != SD_NONE) ++d;
            const unsigned w = M.ld(p);
            if (d < (w & SD_NONE)) M.st(p, (w & ~SD_NONE) | d);
        }
    }
    __syncthreads();
    // while a lane replaces the d2 bits of its own word, other lanes read that word's g bits, which the store leaves as they are
    for (int p = tid; p < HW; p += NT) {
        if (!M.bit(bt, p)) continue;
        const int y = p / W, x = p - y * W, row = p - x;
        const unsigned w = M.ld(p), g0 = w & SD_NONE;
        unsigned best = g0 * g0;
        const int kmax = x > W - 1 - x ? x : W - 1 - x;
        for (int k = 1; k <= kmax; ++k) {
            const unsigned kk = (unsigned)(k * k);
            if (kk >= best) break;
            if (x - k >= 0) {
                const unsigned g = M.ld(row + x - k) & SD_NONE, c = kk + g * g;
                best = c < best ? c : best;
            }
            if (x + k < W) {
                const unsigned g = M.ld(row + x + k) & SD_NONE, c = kk + g * g;
                best = c < best ? c : best;
            }
        }
        M.st(p, (best << SD_GBITS) | g0);                  // (the other surface is not empty: best < 2^21)
    }
    __syncthreads();
}

template <bool LDS, int NT>
__global__ __launch_bounds__(NT) void surface_distance_kernel(SdArgs a)
{
    constexpr int NW = NT / 64;
    __shared__ uint4 s_mem[LDS ? (SD_LDS_PIX + 4 * (SD_LDS_PIX / 32)) / 4 : 1];
    __shared__ unsigned s_u[2][NW][4];
    __shared__ u64 s_s[NW][2];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, H = a.H, W = a.W, HW = a.HW;
    const size_t f = blockIdx.x;
    const unsigned cls = (unsigned)a.cls;
    const int PW = sd_plane_words(HW), BW = sd_bitmap_words(HW);
    const int bA = PW, bB = PW + BW, bSA = PW + 2 * BW, bSB = PW + 3 * BW;
    Words<LDS> M;
    if constexpr (LDS) M.w = reinterpret_cast<unsigned*>(s_mem);
    else M.w = a.ws + f * (size_t)a.stride;
    i64* out = a.surf + f * 8;

    // pass 1, 2: the bitmaps
    for (int i = tid; i < 4 * BW; i += NT) M.st(PW + i, 0u);
    __syncthreads();
    class_bitmap<LDS, NT>(M, bA, a.mask + f * (size_t)HW, HW, W, cls);
    class_bitmap<LDS, NT>(M, bB, a.target + f * (size_t)HW, HW, W, cls);
    __syncthreads();

    // pass 3: the surfaces and their sizes
    unsigned nA, nB;
    {
        const unsigned ca = wave_sum(surface_bitmap<LDS, NT>(M, bA, bSA, H, W, HW));
        const unsigned cb = wave_sum(surface_bitmap<LDS, NT>(M, bB, bSB, H, W, HW));
        if (lane == 0) { s_u[0][wv][0] = ca; s_u[0][wv][1] = cb; }
        __syncthreads();
        nA = nB = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) { nA += s_u[0][w][0]; nB += s_u[0][w][1]; }
    }
    if (nA == 0 || nB == 0) {                              // (uniform) no surface distance
        if (tid < 8) out[tid] = tid == 0 ? (i64)nA : tid == 1 ? (i64)nB : 0;
        return;
    }

    // pass 4: both directions
    directed_distance<LDS, NT>(M, bSA, bSB, H, W, HW, true);
    directed_distance<LDS, NT>(M, bSB, bSA, H, W, HW, false);

    // pass 5: maxima, sums, and the words of the bisection (the words past H W up to the whole vector count nothing)
    unsigned hAB = 0, hBA = 0;
    {
        u64 sAB = 0, sBA = 0;
        for (int p = tid; p < PW; p += NT) {
            unsigned v = 0;
            if (p < HW) {
                const bool ina = M.bit(bSA, p), inb = M.bit(bSB, p);
                if (ina || inb) {
                    const unsigned d2 = M.ld(p) >> SD_GBITS;
                    const u64 r = isqrt_q32(d2);
                    if (ina) { hAB = d2 > hAB ? d2 : hAB; sAB += r; }
                    if (inb) { hBA = d2 > hBA ? d2 : hBA; sBA += r; }
                    v = (((ina ? 1u : 0u) + (inb ? 1u : 0u)) << 21) | d2;
                }
            }
            M.st(p, v);
        }
        hAB = wave_max(hAB); hBA = wave_max(hBA);
        sAB = wave_sum(sAB); sBA = wave_sum(sBA);
        if (lane == 0) { s_u[1][wv][0] = hAB; s_u[1][wv][1] = hBA; s_s[wv][0] = sAB; s_s[wv][1] = sBA; }
        __syncthreads();
        hAB = hBA = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            hAB = s_u[1][w][0] > hAB ? s_u[1][w][0] : hAB;
            hBA = s_u[1][w][1] > hBA ? s_u[1][w][1] : hBA;
        }
    }

    // pass 6: the ranks.  count(m) = the pooled values <= m, and the smallest pooled value above m; the slots of s_u alternate, so that one
    // barrier per count is enough (a lane that is still reading slot k cannot meet a write before the barrier of the count in between)
    int turn = 0;
    auto count = [&](unsigned m, unsigned& above) -> unsigned {
        unsigned c = 0, mn = 0xffffffffu;
        for (int i = tid; i < PW / 4; i += NT) {
            unsigned w[4];
            if constexpr (LDS) {
                const uint4 q = s_mem[i];
                w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) w[e] = M.ld(4 * i + e);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned d2 = w[e] & SD_D2MASK, mult = w[e] >> 21;
                c += d2 <= m ? mult : 0u;
                mn = (mult && d2 > m && d2 < mn) ? d2 : mn;
            }
        }
        c = wave_sum(c);
        mn = wave_min(mn);
        if (lane == 0) { s_u[turn][wv][2] = c; s_u[turn][wv][3] = mn; }
        __syncthreads();
        c = 0; mn = 0xffffffffu;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            c += s_u[turn][w][2];
            mn = s_u[turn][w][3] < mn ? s_u[turn][w][3] : mn;
        }
        turn ^= 1;
        above = mn;
        return c;
    };
    const unsigned n = nA + nB, lo = (unsigned)((95ull * (n - 1)) / 100ull), hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
    unsigned vlo = 0, vhi = hAB > hBA ? hAB : hBA, above;
    for (int it = 0; it < 21 && vlo < vhi; ++it) {         // (uniform) the smallest v with count(v) > lo
        const unsigned mid = (vlo + vhi) >> 1;
        if (count(mid, above) > lo) vhi = mid;
        else vlo = mid + 1;
    }
    const unsigned q_lo = vlo;
    const unsigned c_lo = count(q_lo, above);
    const unsigned q_hi = c_lo > hi ? q_lo : above;        // (c_lo <= hi <= n - 1: a pooled value above q_lo exists)

    if (tid == 0) {
        u64 sAB = 0, sBA = 0;
        for (int w = 0; w < NW; ++w) { sAB += s_s[w][0]; sBA += s_s[w][1]; }
        out[0] = (i64)nA; out[1] = (i64)nB; out[2] = (i64)hAB; out[3] = (i64)hBA;
        out[4] = (i64)sAB; out[5] = (i64)sBA; out[6] = (i64)q_lo; out[7] = (i64)q_hi;
    }
}

// words per frame in the workspace: the frame's words rounded up to 128 bytes, so that no two frames share a cache line
inline size_t sd_stride(int H, int W) { return ((size_t)sd_plane_words(H * W) + 4 * (size_t)sd_bitmap_words(H * W) + 31) & ~(size_t)31; }

// ---- the same with a pixel spacing: gdkvm_surface_distance_mm ---------------------------------------------------------------------------------
// Every frame brings its pixel's height ry and width rx in micrometres (1..4095), and a squared distance is (ry dy)^2 + (rx dx)^2 um^2, below
// 2^45.  The bitmaps, the surfaces and the passes are those above; what changes is the pixel's word, now 64 bits: g in the low 11 bits as
// before (a count of ROWS: the column sweep is unchanged), d2 in the 45 bits above them, and from pass 5 on d2 in the low 45 bits with the
// multiplicity above.  A frame keeps 8.5 bytes per pixel: the 64-bit plane first (whole 16-byte vectors), then the four bitmaps.  They live in
// dynamic LDS while the frame has at most GDKVM_SURFACE_MM_LDS_PIXELS pixels (153 KiB of the workgroup's 160 KiB; a 112 x 112 frame takes
// 104 KiB; SDU_LDS_NT lanes), otherwise in the frame's slice of the workspace (1024 lanes).  NONE is tested for, not squared: with ry = 1
// its square is below real distances.  Loop bounds: as above, and the bisection counts to 45.
constexpr int SDU_LDS_PIX = GDKVM_SURFACE_MM_LDS_PIXELS;
constexpr int SDU_LDS_NT = 1024;               // lanes of the LDS form: a 112 x 112 frame's 104 KiB leave room for ONE workgroup per CU, so it is a wide one
constexpr unsigned SDU_D2BITS = 45;
constexpr u64 SDU_D2MASK = (1ull << SDU_D2BITS) - 1;
constexpr u64 SDU_INF = ~0ull;                 // no pixel of the other surface met yet

struct SdUmArgs {
    const uint8_t* mask; const uint8_t* target; const int32_t* spacing; i64* surf; u64* ws;
    int H, W, HW, cls;
    size_t stride;                             // 64-bit words per frame of the workspace
};

__host__ __device__ inline int sdu_plane_words(int HW) { return (HW + 1) & ~1; }          // 64-bit words: whole 16-byte vectors
inline size_t sdu_frame_bytes(int HW) { return 8 * (size_t)sdu_plane_words(HW) + 16 * (size_t)sd_bitmap_words(HW); }
inline size_t sdu_stride(int H, int W) { return ((sdu_frame_bytes(H * W) + 127) & ~(size_t)127) / 8; }

// floor(sqrt(d2 * 2^16)): the operand is below 2^61 and its root below 2^31, so the fp64 estimate is off by at most one either way
__device__ __forceinline__ u64 isqrt_q16(u64 d2)
{
    const u64 n = d2 << 16;
    u64 r = (u64)sqrt((double)n);
    if (r * r > n) --r;
    if ((r + 1) * (r + 1) <= n) ++r;
    return r;
}

// Pass 4 for one direction, as directed_distance: B holds the bitmaps, P the plane; ry2, rx2 = the squared spacings
template <bool LDS, int NT>
__device__ __forceinline__ void directed_distance_um(const Words<LDS>& B, const FrameWords64<LDS, int>& P, int bt, int bo, int H, int W, int HW,
                                                     u64 ry2, u64 rx2, bool first)
{
    const int tid = threadIdx.x;
    for (int x = tid; x < W; x += NT) {
        unsigned d = SD_NONE;
        for (int y = 0, p = x; y < H; ++y, p += W) {
            if (B.bit(bo, p)) d = 0;
            else if (d != SD_NONE) ++d;
            P.st(p, (first ? 0ull : (P.ld(p) & ~(u64)SD_NONE)) | d);
        }
        d = SD_NONE;
        for (int y = H - 1, p = (H - 1) * W + x; y >= 0; --y, p -= W) {
            if (B.bit(bo, p)) d = 0;
            else if (d != SD_NONE) ++d;
            const u64 w = P.ld(p);
            if (d < ((unsigned)w & SD_NONE)) P.st(p, (w & ~(u64)SD_NONE) | d);
        }
    }
    __syncthreads();
    // while a lane replaces the d2 bits of its own word, other lanes read that word's g bits, which the (single, 64-bit) store leaves as they are
    for (int p = tid; p < HW; p += NT) {
        if (!B.bit(bt, p)) continue;
        const int y = p / W, x = p - y * W, row = p - x;
        const unsigned g0 = (unsigned)P.ld(p) & SD_NONE;
        u64 best = g0 == SD_NONE ? SDU_INF : (u64)(g0 * g0) * ry2;
        const int kmax = x > W - 1 - x ? x : W - 1 - x;
        for (int k = 1; k <= kmax; ++k) {
            const u64 kk = (u64)(unsigned)(k * k) * rx2;     // (< 2^20 * 2^24)
            if (kk >= best) break;
            if (x - k >= 0) {
                const unsigned g = (unsigned)P.ld(row + x - k) & SD_NONE;
                const u64 c = kk + (u64)(g * g) * ry2;
                best = (g != SD_NONE && c < best) ? c : best;
            }
            if (x + k < W) {
                const unsigned g = (unsigned)P.ld(row + x + k) & SD_NONE;
                const u64 c = kk + (u64)(g * g) * ry2;
                best = (g != SD_NONE && c < best) ? c : best;
            }
        }
        P.st(p, (best << SD_GBITS) | g0);                   // (the other surface is not empty: best < 2^45)
    }
    __syncthreads();
}

template <bool LDS, int NT>
__global__ __launch_bounds__(NT) void surface_distance_mm_kernel(SdUmArgs a)
{
    constexpr int NW = NT / 64;
    extern __shared__ uint4 sdu_mem[];
    __shared__ unsigned s_n[NW][2];
    __shared__ u64 s_h[NW][2];
    __shared__ u64 s_s[NW][2];
    __shared__ u64 s_c[2][NW][2];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, H = a.H, W = a.W, HW = a.HW;
    const size_t f = blockIdx.x;
    const unsigned cls = (unsigned)a.cls;
    const int PW = sdu_plane_words(HW), BW = sd_bitmap_words(HW);
    const int bA = 0, bB = BW, bSA = 2 * BW, bSB = 3 * BW;
    i64* out = a.surf + f * 8;
    const int ry = a.spacing[2 * f], rx = a.spacing[2 * f + 1];
    if (ry < 1 || ry > 4095 || rx < 1 || rx > 4095) {      // (uniform) no error can be returned from here: the record says so
        if (tid < 8) out[tid] = -1;
        return;
    }
    const u64 ry2 = (u64)(ry * ry), rx2 = (u64)(rx * rx);
    FrameWords64<LDS, int> P;
    if constexpr (LDS) P.w = reinterpret_cast<u64*>(sdu_mem);
    else P.w = a.ws + f * a.stride;
    Words<LDS> M;
    M.w = reinterpret_cast<unsigned*>(P.w + PW);

    // pass 1, 2: the bitmaps
    for (int i = tid; i < 4 * BW; i += NT) M.st(i, 0u);
    __syncthreads();
    class_bitmap<LDS, NT>(M, bA, a.mask + f * (size_t)HW, HW, W, cls);
    class_bitmap<LDS, NT>(M, bB, a.target + f * (size_t)HW, HW, W, cls);
    __syncthreads();

    // pass 3: the surfaces and their sizes
    {
        const unsigned ca = wave_sum(surface_bitmap<LDS, NT>(M, bA, bSA, H, W, HW));
        const unsigned cb = wave_sum(surface_bitmap<LDS, NT>(M, bB, bSB, H, W, HW));
        if (lane == 0) { s_n[wv][0] = ca; s_n[wv][1] = cb; }
        __syncthreads();
    }
    const unsigned nA = wg_sum(s_n, 0), nB = wg_sum(s_n, 1);
    if (nA == 0 || nB == 0) {                              // (uniform) no surface distance
        if (tid < 8) out[tid] = tid == 0 ? (i64)nA : tid == 1 ? (i64)nB : 0;
        return;
    }

    // pass 4: both directions
    directed_distance_um<LDS, NT>(M, P, bSA, bSB, H, W, HW, ry2, rx2, true);
    directed_distance_um<LDS, NT>(M, P, bSB, bSA, H, W, HW, ry2, rx2, false);

    // pass 5: maxima, sums, and the words of the bisection (the word past an odd H W counts nothing)
    u64 hAB = 0, hBA = 0;
    {
        u64 sAB = 0, sBA = 0;
        for (int p = tid; p < PW; p += NT) {
            u64 v = 0;
            if (p < HW) {
                const bool ina = M.bit(bSA, p), inb = M.bit(bSB, p);
                if (ina || inb) {
                    const u64 d2 = P.ld(p) >> SD_GBITS;
                    const u64 r = isqrt_q16(d2);
                    if (ina) { hAB = d2 > hAB ? d2 : hAB; sAB += r; }
                    if (inb) { hBA = d2 > hBA ? d2 : hBA; sBA += r; }
                    v = ((u64)((ina ? 1u : 0u) + (inb ? 1u : 0u)) << SDU_D2BITS) | d2;
                }
            }
            P.st(p, v);
        }
        hAB = wave_max(hAB); hBA = wave_max(hBA);
        sAB = wave_sum(sAB); sBA = wave_sum(sBA);
        if (lane == 0) { s_h[wv][0] = hAB; s_h[wv][1] = hBA; s_s[wv][0] = sAB; s_s[wv][1] = sBA; }
        __syncthreads();
        hAB = hBA = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            hAB = s_h[w][0] > hAB ? s_h[w][0] : hAB;
            hBA = s_h[w][1] > hBA ? s_h[w][1] : hBA;
        }
    }

    // pass 6: the ranks, as above: the slots of s_c alternate, one barrier per count
    int turn = 0;
    auto count = [&](u64 m, u64& above) -> unsigned {
        unsigned c = 0;
        u64 mn = SDU_INF;
        for (int i = tid; i < PW / 2; i += NT) {
            u64 w[2];
            if constexpr (LDS) {
                const uint4 q = sdu_mem[i];
                w[0] = ((u64)q.y << 32) | q.x; w[1] = ((u64)q.w << 32) | q.z;
            } else {
                w[0] = P.ld(2 * i); w[1] = P.ld(2 * i + 1);
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const u64 d2 = w[e] & SDU_D2MASK;
                const unsigned mult = (unsigned)(w[e] >> SDU_D2BITS);
                c += d2 <= m ? mult : 0u;
                mn = (mult && d2 > m && d2 < mn) ? d2 : mn;
            }
        }
        c = wave_sum(c);
        mn = wave_min(mn);
        if (lane == 0) { s_c[turn][wv][0] = c; s_c[turn][wv][1] = mn; }
        __syncthreads();
        c = 0; mn = SDU_INF;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            c += (unsigned)s_c[turn][w][0];
            mn = s_c[turn][w][1] < mn ? s_c[turn][w][1] : mn;
        }
        turn ^= 1;
        above = mn;
        return c;
    };
    const unsigned n = nA + nB, lo = (unsigned)((95ull * (n - 1)) / 100ull), hi = lo + 1 < n - 1 ? lo + 1 : n - 1;
    u64 vlo = 0, vhi = hAB > hBA ? hAB : hBA, above;
    for (int it = 0; it < (int)SDU_D2BITS && vlo < vhi; ++it) {     // (uniform) the smallest v with count(v) > lo
        const u64 mid = (vlo + vhi) >> 1;
        if (count(mid, above) > lo) vhi = mid;
        else vlo = mid + 1;
    }
    const u64 q_lo = vlo;
    const unsigned c_lo = count(q_lo, above);
    const u64 q_hi = c_lo > hi ? q_lo : above;             // (c_lo <= hi <= n - 1: a pooled value above q_lo exists)

    if (tid == 0) {
        out[0] = (i64)nA; out[1] = (i64)nB; out[2] = (i64)hAB; out[3] = (i64)hBA;
        out[4] = (i64)wg_sum(s_s, 0); out[5] = (i64)wg_sum(s_s, 1); out[6] = (i64)q_lo; out[7] = (i64)q_hi;
    }
}

}  // namespace

extern "C" size_t gdkvm_surface_distance_workspace_bytes(int frames, int H, int W)
{
    if (!mask_shape_ok(frames, H, W) || H * W <= SD_LDS_PIX) return 0;
    return (size_t)frames * sd_stride(H, W) * sizeof(unsigned);
}

extern "C" int gdkvm_surface_distance(const uint8_t* mask, const uint8_t* target, int64_t* surf, void* workspace, size_t workspace_bytes,
                                      int frames, int H, int W, int cls, void* stream)
{
    if (int rc = mask_check_shape("surface_distance", frames, H, W)) return rc;
    if (int rc = mask_check_cls("surface_distance", GDKVM_ERR_SHAPE, cls)) return rc;
    if (frames == 0) return GDKVM_OK;
    if (!mask || !target || !surf) return gdkvm_fail(GDKVM_ERR_SHAPE, "surface_distance: null pointer (mask, target and surf are required)");
    if (int rc = mask_check_aligned16("surface_distance", GDKVM_ERR_SHAPE, "surf", {surf})) return rc;
    const size_t need = gdkvm_surface_distance_workspace_bytes(frames, H, W);
    if (int rc = mask_check_workspace("surface_distance", H, W, need, workspace, workspace_bytes)) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    SdArgs a{mask, target, reinterpret_cast<i64*>(surf), static_cast<unsigned*>(workspace), H, W, H * W, (int)sd_stride(H, W), cls};
    if (!need) hipLaunchKernelGGL((surface_distance_kernel<true, 256>), dim3((unsigned)frames), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((surface_distance_kernel<false, 1024>), dim3((unsigned)frames), dim3(1024), 0, st, a);
    GDKVM_LAUNCH_CHECK("surface_distance_kernel");
    return GDKVM_OK;
}

extern "C" size_t gdkvm_surface_distance_mm_workspace_bytes(int frames, int H, int W)
{
    if (!mask_shape_ok(frames, H, W) || H * W <= SDU_LDS_PIX) return 0;
    return (size_t)frames * sdu_stride(H, W) * sizeof(u64);
}

extern "C" int gdkvm_surface_distance_mm(const uint8_t* mask, const uint8_t* target, const int32_t* spacing_um, int64_t* surf, void* workspace,
                                         size_t workspace_bytes, int frames, int H, int W, int cls, void* stream)
{
    if (int rc = mask_check_shape("surface_distance_mm", frames, H, W)) return rc;
    if (int rc = mask_check_cls("surface_distance_mm", GDKVM_ERR_SHAPE, cls)) return rc;
    if (frames == 0) return GDKVM_OK;
    if (!mask || !target || !spacing_um || !surf)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "surface_distance_mm: null pointer (mask, target, spacing_um and surf are required)");
    if (reinterpret_cast<uintptr_t>(spacing_um) & 3u) return gdkvm_fail(GDKVM_ERR_SHAPE, "surface_distance_mm: spacing_um must be 4-byte aligned");
    if (int rc = mask_check_aligned16("surface_distance_mm", GDKVM_ERR_SHAPE, "surf", {surf})) return rc;
    const size_t need = gdkvm_surface_distance_mm_workspace_bytes(frames, H, W);
    if (int rc = mask_check_workspace("surface_distance_mm", H, W, need, workspace, workspace_bytes)) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    SdUmArgs a{mask, target, spacing_um, reinterpret_cast<i64*>(surf), static_cast<u64*>(workspace), H, W, H * W, cls, sdu_stride(H, W)};
    if (!need) {
        const size_t lds = sdu_frame_bytes(H * W);
        if (lds > 32 * 1024) {                           // a large frame needs the opt-in once per device
            static std::atomic<unsigned long long> done_mask{0};
            int dev = 0;
            if (hipGetDevice(&dev) != hipSuccess) return gdkvm_fail(GDKVM_ERR_LAUNCH, "surface_distance_mm: hipGetDevice");
            const unsigned long long bit = 1ull << (dev & 63);
            if (!(done_mask.load(std::memory_order_relaxed) & bit)) {
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(surface_distance_mm_kernel<true, SDU_LDS_NT>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)sdu_frame_bytes(SDU_LDS_PIX));
                if (e != hipSuccess) return gdkvm_fail(GDKVM_ERR_LAUNCH, "surface_distance_mm: LDS attribute: %s", hipGetErrorString(e));
                done_mask.fetch_or(bit, std::memory_order_relaxed);
            }
        }
        hipLaunchKernelGGL((surface_distance_mm_kernel<true, SDU_LDS_NT>), dim3((unsigned)frames), dim3(SDU_LDS_NT), lds, st, a);
    } else {
        hipLaunchKernelGGL((surface_distance_mm_kernel<false, 1024>), dim3((unsigned)frames), dim3(1024), 0, st, a);
    }
    GDKVM_LAUNCH_CHECK("surface_distance_mm_kernel");
    return GDKVM_OK;
}
