// lv_contour.hip -- contour length and landmarks of one class of label masks on the device (what global longitudinal strain needs beside
// lv_measure's volumes): per frame the pair counts of the class against a wall set and a base set of bytes in the four lattice directions, the
// base interface's centroid, and the class pixel farthest from it (the apex).  include/gdkvm.h holds the definition; every output is an exact
// integer.  ONE 256-lane workgroup per frame walks it in bands of rows: per band three bit planes in LDS (class, wall set, base set), each with
// one halo row above and below and one halo column on each side that hold the membership of byte 0 (what a position outside the frame reads
// as), so the frame's border needs no branches.  A count is then a popcount of the class plane ANDed with a shifted set plane, 64 pixels at a
// time, and only where a word holds a class pixel at all.  The apex pass reads the (L2-hot) frame again.  No workspace, no global atomics, no
// fences.

#include "mask_frame.hpp"

namespace {

typedef long long i64;
typedef unsigned long long u64;

constexpr int BAND = GDKVM_LV_CONTOUR_BAND_ROWS;           // rows of a band (its planes hold BAND + 2)
constexpr int WB = GDKVM_LV_CONTOUR_WORD_BITS;             // pixels of a plane word
static_assert(WB == 64, "the planes are 64-bit words");
constexpr int MAXW = (1024 + 2 + WB - 1) / WB;             // words of the widest row: pixel x is bit x + 1, bits 0 and W + 1 are the halo
constexpr int NRED = 11;                                   // n, 4 wall counts, 4 base counts, SX2, SY2

struct ContourArgs {
    const uint8_t* mask; const int32_t* spacing; i64* rec;
    int H, W, cls;
    unsigned wall, base;
};

// bit e = byte e of the vector is in the set s (a 32-bit mask over the bytes 0..31; a byte >= 32 is in no set), for three sets at once
__device__ __forceinline__ void member16(const uint4& v, const unsigned (&s)[3], unsigned (&m)[3])
{
    const unsigned w[4] = {v.x, v.y, v.z, v.w};
    m[0] = m[1] = m[2] = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const unsigned b = (w[q] >> (8 * e)) & 0xffu, in = b < 32u ? 1u : 0u, sh = b & 31u;
#pragma unroll
            for (int k = 0; k < 3; ++k) m[k] |= ((s[k] >> sh) & in) << (4 * q + e);
        }
}

// The sum of the positions of the set bits of h: position bit b is set in the bits of the constant K_b
__device__ __forceinline__ int bit_position_sum(u64 h)
{
    return __popcll(h & 0xaaaaaaaaaaaaaaaaull) + 2 * __popcll(h & 0xccccccccccccccccull) + 4 * __popcll(h & 0xf0f0f0f0f0f0f0f0ull) +
           8 * __popcll(h & 0xff00ff00ff00ff00ull) + 16 * __popcll(h & 0xffff0000ffff0000ull) + 32 * __popcll(h & 0xffffffff00000000ull);
}

// bit j of the result = bit j - 1 of the row (lo = the word in front, 0 at the row's start) / bit j + 1 (hi = the word behind)
__device__ __forceinline__ u64 from_left(u64 m, u64 lo) { return (m << 1) | (lo >> 63); }
__device__ __forceinline__ u64 from_right(u64 m, u64 hi) { return (m >> 1) | (hi << 63); }

__global__ __launch_bounds__(256) void lv_contour_kernel(ContourArgs a)
{
    __shared__ u64 s_pl[3][(BAND + 2) * MAXW];             // the band's planes: class, wall set, base set; row r, word k at [r NW + k]
    __shared__ i64 s_red[4][NRED];
    __shared__ i64 s_apex[4][2];
    const int tid = threadIdx.x, wv = tid >> 6, H = a.H, W = a.W;
    const size_t f = blockIdx.x;
    i64* rec = a.rec + f * 16;
    int ry = 1, rx = 1;
    if (a.spacing) {
        ry = a.spacing[2 * f]; rx = a.spacing[2 * f + 1];
        if (ry < 1 || ry > 4095 || rx < 1 || rx > 4095) {  // (uniform) no error can be returned from here: the record says so
            if (tid < 16) rec[tid] = -1;
            return;
        }
    }
    const uint8_t* base = a.mask + f * (size_t)H * W;
    const unsigned sets[3] = {1u << a.cls, a.wall, a.base};
    const int NW = (W + 2 + WB - 1) / WB;                  // words of a row of this frame
    const int wl = (W + 1) / WB, bl = (W + 1) % WB;        // word and bit of the right halo column

    unsigned n32 = 0, cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // per lane: at most 16 bands x 5 words x 64 pixels x 2 neighbours
    i64 sx2 = 0, sy2 = 0;
    for (int r0 = 0; r0 < H; r0 += BAND) {
        const int r1 = r0 + BAND < H ? r0 + BAND : H;      // the band's rows r0 .. r1 - 1; its planes hold the rows r0 - 1 .. r1
        const int rows = r1 - r0 + 2;
        // the planes before the frame's bytes: the halo holds byte 0's membership, everything else 0
        for (int i = tid; i < rows * NW; i += 256) {
            const int r = i / NW, k = i - r * NW, y = r0 - 1 + r;
            u64 halo;
            if (y < 0 || y >= H) {                         // a row outside the frame: bits 0 .. W + 1
                halo = k < wl ? ~0ull : (bl == 63 ? ~0ull : (1ull << (bl + 1)) - 1);
            } else {
                halo = (k == 0 ? 1ull : 0ull) | (k == wl ? 1ull << bl : 0ull);
            }
            s_pl[0][i] = 0;
            s_pl[1][i] = (sets[1] & 1u) ? halo : 0;
            s_pl[2][i] = (sets[2] & 1u) ? halo : 0;
        }
        __syncthreads();
        // the frame's rows lo .. hi - 1 of the band into the planes: 16 bytes at a time, each run of a row ORed in at its bit
        const int lo = r0 > 0 ? r0 - 1 : 0, hi = r1 < H ? r1 + 1 : H, rofs = lo - (r0 - 1);
        const MaskFrame<256> fr(base + (size_t)lo * W, (hi - lo) * W, W, (unsigned)a.cls);
        auto place = [&](const unsigned (&m)[3], int p0, int nbits) {
            if (!(m[0] | m[1] | m[2])) return;
            int y = p0 / W, x = p0 - y * W, sh = 0;
            while (sh < nbits) {
                const int len = nbits - sh < W - x ? nbits - sh : W - x;
                const unsigned seg = (1u << len) - 1u;     // (len <= 16)
                const int word = (x + 1) / WB, bit = (x + 1) % WB;
                u64* row = &s_pl[0][(y + rofs) * NW + word];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const u64 v = (m[k] >> sh) & seg;
                    if (v) {
                        atomicOr(row + k * (BAND + 2) * MAXW, v << bit);
                        if (bit + len > WB) atomicOr(row + k * (BAND + 2) * MAXW + 1, v >> (WB - bit));
                    }
                }
                sh += len; x = 0; ++y;
            }
        };
        auto place_byte = [&](int p) {
            const unsigned b = fr.base[p], in = b < 32u ? 1u : 0u, sh = b & 31u;
            const unsigned m[3] = {(sets[0] >> sh) & in, (sets[1] >> sh) & in, (sets[2] >> sh) & in};
            place(m, p, 1);
        };
        if (tid < fr.head) place_byte(tid);
        for (int v = tid; v < fr.nvec; v += 256) {
            unsigned m[3];
            member16(fr.body[v], sets, m);
            place(m, fr.head + 16 * v, 16);
        }
        if (tid < fr.tail) place_byte(fr.head + fr.nbody + tid);
        __syncthreads();
        // the counts of the band's own rows (plane rows 1 .. rows - 2)
        for (int i = tid; i < (rows - 2) * NW; i += 256) {
            const int r = i / NW + 1, k = i - (r - 1) * NW, j = r * NW + k;
            const u64 c = s_pl[0][j];
            if (!c) continue;
            n32 += __popcll(c);
            const bool first = k == 0, last = k + 1 == NW;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (s == 1 && !a.base) break;              // (uniform)
                const u64* X = s_pl[1 + s];
                const u64 mid = X[j], up = X[j - NW], dn = X[j + NW];
                const u64 midl = first ? 0 : X[j - 1], upl = first ? 0 : X[j - NW - 1], dnl = first ? 0 : X[j + NW - 1];
                const u64 midr = last ? 0 : X[j + 1], upr = last ? 0 : X[j - NW + 1], dnr = last ? 0 : X[j + NW + 1];
                const u64 hw = c & from_left(mid, midl), he = c & from_right(mid, midr), hn = c & up, hs = c & dn;
                cnt[4 * s + 0] += __popcll(hw) + __popcll(he);
                cnt[4 * s + 1] += __popcll(hn) + __popcll(hs);
                cnt[4 * s + 2] += __popcll(c & from_right(dn, dnr)) + __popcll(c & from_left(up, upl));
                cnt[4 * s + 3] += __popcll(c & from_left(dn, dnl)) + __popcll(c & from_right(up, upr));
                if (s == 1 && (hw | he | hn | hs)) {
                    // twice the crack midpoints: a hit at bit b is the pixel x = 64 k + b - 1 of row y, its partner one step away
                    const int y = r0 - 1 + r, x0 = WB * k - 1;
                    const int nw = __popcll(hw), ne = __popcll(he), nn = __popcll(hn), ns = __popcll(hs), all = nw + ne + nn + ns;
                    const int xs = bit_position_sum(hw) + bit_position_sum(he) + bit_position_sum(hn) + bit_position_sum(hs) + x0 * all;
                    sx2 += 2 * xs + ne - nw;
                    sy2 += 2 * y * all + ns - nn;
                }
            }
        }
        __syncthreads();                                   // (the next band's planes overwrite these)
    }
    {
        const i64 part[NRED] = {(i64)n32, (i64)cnt[0], (i64)cnt[1], (i64)cnt[2], (i64)cnt[3], (i64)cnt[4], (i64)cnt[5], (i64)cnt[6], (i64)cnt[7],
                                sx2, sy2};
#pragma unroll
        for (int i = 0; i < NRED; ++i) {
            const i64 s = wave_sum(part[i]);
            if ((tid & 63) == 0) s_red[wv][i] = s;
        }
    }
    __syncthreads();
    i64 tot[NRED];
#pragma unroll
    for (int i = 0; i < NRED; ++i) tot[i] = wg_sum(s_red, i);
    const i64 nb = tot[5] + tot[6];
    if (nb == 0) {                                         // (uniform) no base interface (an empty class included): no landmarks
        if (tid < 9) rec[tid] = tot[tid];
        else if (tid < 16) rec[tid] = (tid >= 11 && tid <= 13) ? -1 : 0;
        return;
    }
    // the base point in half pixels, rounded half up: floor towards -infinity of a numerator that may be negative
    auto floor_div = [](i64 num, i64 den) -> i64 { const i64 q = num / den; return (num % den != 0 && num < 0) ? q - 1 : q; };
    const i64 bx2 = floor_div(2 * tot[9] + nb, 2 * nb), by2 = floor_div(2 * tot[10] + nb, 2 * nb);
    // the apex: the class pixel farthest from the base point; a lane meets its pixels in ascending order, so `>` keeps its smallest p
    i64 best = -1;
    int bestp = 0x7fffffff;
    {
        const MaskFrame<256> fr(base, H * W, W, (unsigned)a.cls);
        fr.sweep_xy([&](int p, int x, int y) {
            const i64 dy = (i64)ry * (2 * y - by2), dx = (i64)rx * (2 * x - bx2), d2 = dy * dy + dx * dx;
            if (d2 > best) { best = d2; bestp = p; }
        });
    }
    {
        const i64 m = wave_max(best);
        const int p = wave_min(best == m ? bestp : 0x7fffffff);
        if ((tid & 63) == 0) { s_apex[wv][0] = m; s_apex[wv][1] = p; }
    }
    __syncthreads();
    if (tid == 0) {
        i64 m = s_apex[0][0], p = s_apex[0][1];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (s_apex[w][0] > m || (s_apex[w][0] == m && s_apex[w][1] < p)) { m = s_apex[w][0]; p = s_apex[w][1]; }
        rec[11] = bx2; rec[12] = by2; rec[13] = p; rec[14] = m; rec[15] = 0;
    }
    if (tid >= 64 && tid < 64 + 11) rec[tid - 64] = tot[tid - 64];
}

}  // namespace

extern "C" int gdkvm_lv_contour(const uint8_t* mask, const int32_t* spacing_um, int64_t* rec,
                                int frames, int H, int W, int cls, unsigned wall_set, unsigned base_set, void* stream)
{
    const char* name = "lv_contour";
    if (int rc = mask_check_shape(name, frames, H, W)) return rc;
    if (int rc = mask_check_cls(name, GDKVM_ERR_ARG, cls)) return rc;
    if (cls > 31) return gdkvm_fail(GDKVM_ERR_ARG, "%s: cls=%d outside 0..31 (the sets are masks over the bytes 0..31)", name, cls);
    if (wall_set == 0) return gdkvm_fail(GDKVM_ERR_ARG, "%s: wall_set is empty", name);
    if (wall_set & base_set) return gdkvm_fail(GDKVM_ERR_ARG, "%s: wall_set=0x%x and base_set=0x%x overlap", name, wall_set, base_set);
    if (((wall_set | base_set) >> cls) & 1u)
        return gdkvm_fail(GDKVM_ERR_ARG, "%s: wall_set=0x%x / base_set=0x%x holds cls=%d", name, wall_set, base_set, cls);
    if (frames == 0) return GDKVM_OK;
    if (!mask || !rec) return gdkvm_fail(GDKVM_ERR_ARG, "%s: null pointer", name);
    if (reinterpret_cast<uintptr_t>(spacing_um) & 3u) return gdkvm_fail(GDKVM_ERR_ARG, "%s: spacing_um must be 4-byte aligned", name);
    if (int rc = mask_check_aligned16(name, GDKVM_ERR_ARG, "rec", {rec})) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    ContourArgs a{mask, spacing_um, reinterpret_cast<i64*>(rec), H, W, cls, wall_set, base_set};
    hipLaunchKernelGGL(lv_contour_kernel, dim3((unsigned)frames), dim3(256), 0, st, a);
    GDKVM_LAUNCH_CHECK("lv_contour_kernel");
    return GDKVM_OK;
}
