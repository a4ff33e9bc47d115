// overlay_native.hip -- draw a mask, its contour and optionally a second mask's contour over grey frames at each clip's own frame size
// (h0, w0): the picture predict.py --overlay and eval.py's eval_stage.vis_overlay write.  include/gdkvm.h holds the rule: a pixel with the
// class byte k (1 <= k < ncls) is a contour pixel when some pixel within the 4-neighbour distance w holds another byte or lies outside the
// frame; contour of the mask > contour of the ref > tinted class > grey.  Exact integers, one writer per output byte, no atomics: out depends
// on neither the schedule nor the path taken.  No floating-point code in this file.
//
// The buffers are ragged: native_clips.hpp holds the launcher's side of that; a clip's entry here is (pixel offset, h0, w0, rows per band,
// bands), and the two palettes travel beside the clips, packed one colour to a word.
//
// A workgroup of 256 lanes owns a BAND of native rows of one (clip, frame): the most whole rows whose run slots (below: 1 + ceil(w0 / 16)
// per row) number at most OV_BAND_RUNS = 512, two to a lane -- 10 rows of a 549 x 778 frame -- at least one row and at most
// OV_BAND_ROWS.  A pixel's neighbourhood reaches w rows and columns beyond it, so the band's rows of mask (and of ref) with w
// rows above and below are STAGED IN LDS, one LDS row of P = (w0 + 71) & ~15 bytes per native row:
//   - the row's pixels start at byte 16 + (the row's global address mod 16) of its LDS row, so that every aligned 16-byte chunk of global
//     memory is one aligned 16-byte chunk of LDS: one 16-byte load and one 16-byte LDS store per chunk, whatever the frame's alignment
//     (h0 w0 and w0 are odd as often as not); the bytes of a chunk that belong to the neighbouring rows are masked away, and only a chunk
//     that sticks out of the FRAME (its first and last, at most) is gathered byte by byte, so that nothing outside the frame is read;
//   - every other byte of the LDS row, and every LDS row whose native row lies outside the frame, is ZERO.  Zero is class 0: it differs
//     from every class byte, which is all the rule asks of the outside of the frame, and a pixel that holds it is never drawn.  So the
//     contour needs no border case at all.
// The rows come from L2 (the band above staged most of them a moment ago); at the band of a 549 x 778 frame the halo is 2 w rows on 10.
// The rows go through LDS and not straight from L2 because a run reads 2 w + 1 rows at byte offsets that are aligned in none of them.
//
// Every row of the band is cut into RUNS of 16 pixels on the 16-byte grid of the ADDRESSES of out: pixel x of the row is at out byte
// 3 (row's pixel offset + x), and 3 is invertible mod 16, so one head length in 0..15 puts every later run's 48 output bytes on three
// aligned 16-byte stores.  With all buffers 16-byte aligned the inputs' grid is the same one (3 p = 0 mod 16 iff p = 0 mod 16) and the grey
// bytes of a run are one 16-byte load; a head, a tail and a misaligned grey take byte accesses.  Runs never cross a row: a crossing run would
// need the LDS rows' padding in its middle.  Lane l takes the slots l, l + 256, ... of the band's rows x slots-per-row grid (a head and ceil(w0 / 16) runs per row; the
// order of the slots is the run loop's business).
//
// The contour is found sixteen pixels at a time on packed words.  A run's window of a row -- the 22 bytes from x - 3 to x + 18 -- is seven
// aligned LDS words, shifted once by the window's byte offset (v_alignbyte_b32) into six words n[0..5]; the neighbour at dx of all sixteen
// pixels is then n shifted by the COMPILE-TIME 3 + dx bytes, XORed with the centre words and ORed into a difference word: a byte of it is
// non-zero iff one of the 2 w (w + 1) neighbours differs.  (2 w + 1 rows; 4, 12 or 24 shifted compares of four words.)  A run whose sixteen
// centre bytes hold no class byte skips all of it, which is most runs of an echo frame.  One kernel per width, with and without a ref.
//
// The colour of a pixel is ONE expression, (g ga + C ca + 128) >> 8 per channel, with (C, ca, ga) = (pal[k], 256, 0) on the mask's
// contour, (ref_pal[k'], 256, 0) on the ref's, (pal[k], alpha, 256 - alpha) inside a class and (-, 0, 256) elsewhere -- the rule's four
// cases exactly, since (256 C + 128) >> 8 = C.  ga + ca <= 256, so a channel's sum stays below 2^16 and red and blue are computed in the two
// halves of one word.  The (C ca + 128, ga) of the 24 cases -- grey, tint k, contour k, ref contour k' -- are a table of 8-byte LDS entries
// built once per workgroup; a pixel's entry number is found four pixels at a time on the packed words (k masked by its class flag, + 8 on
// the contour, replaced by 16 + k' where only the ref's contour lies), and a pixel costs one LDS read, one multiply and a few shifts.
// The two divisions of the loops (chunk -> row, run slot -> row) are multiplications by a reciprocal that the item computes once, exact
// for these ranges: integers, like everything else here.
//
// The grid follows the clip with the most bands of the launch: item = (clip, frame, band) over clips x T x maxbands, and a workgroup whose
// band lies past its clip's last leaves at once.  More than OV_MAX_WG items are taken grid-stride.  Dynamic LDS: the 192 bytes of the
// colour table and one or two tiles of the launch's largest (rows + 2 w) P, at most 192 + 2 * 9 * 2112 bytes (a 2048-wide frame).

#include "native_clips.hpp"

namespace {

constexpr int OV_NT = 256;
constexpr int OV_RUN = GDKVM_OVERLAY_NATIVE_RUN;               // native pixels of a lane's run (gdkvm.h)
constexpr int OV_BAND_RUNS = GDKVM_OVERLAY_NATIVE_BAND_RUNS;   // a band is the most whole rows with at most this many run slots ...
constexpr int OV_BAND_ROWS = GDKVM_OVERLAY_NATIVE_BAND_ROWS;   // ... and at most this many rows
constexpr int OV_MAX_WG = GDKVM_OVERLAY_NATIVE_MAX_WG;         // workgroups per launch; more items than that are walked grid-stride
constexpr int OV_CLIPS = GDKVM_OVERLAY_NATIVE_CLIPS;           // clips per launch
constexpr int OV_MAX_WIDTH = 3;
constexpr int OV_TAB = 24;                                     // entries of the colour table: [0] grey, [k] tint, [8 + k] contour, [16 + k] ref contour
constexpr int OV_PAL_BYTES = OV_TAB * 8;                       // the table in front of the tiles
static_assert(OV_RUN == 16, "a run is three 16-byte vectors of out");
static_assert(OV_BAND_RUNS == 2 * OV_NT, "a band gives every lane at most two runs");

// bytes of a native row's LDS row: 16 + 15 in front of the pixels, and a window's seven words may end 25 bytes behind the last pixel
__host__ __device__ constexpr int ov_pitch(int w0) { return (w0 + 71) & ~15; }

struct OvClip {
    unsigned long long off;                                // the clip's first pixel in grey / mask / ref (out: three times that)
    int h0, w0, rpb, nbands;                               // native size, rows per band, bands per frame
};
struct OvArgs {
    const uint8_t* grey; const uint8_t* mask; const uint8_t* ref; uint8_t* out;   // (the buffers' bases: off is absolute)
    long long items;
    int T, maxbands, ncls, alpha;
    unsigned pal[16];                                      // R | G << 8 | B << 16: [k] the mask's colours, [8 + k] the ref's
    OvClip c[OV_CLIPS];
};
static_assert(sizeof(OvArgs) <= 2048, "the clip table travels in the kernel arguments");

// 0x80 in every byte of d that is not zero
__device__ __forceinline__ unsigned ov_nz80(unsigned d) { return (((d & BYTES_LO) + BYTES_LO) | d) & BYTES_HI; }
// 0x80 in every byte of c that is a class byte: not zero and below ncls (<= 8)
__device__ __forceinline__ unsigned ov_cls80(unsigned c, unsigned ncls)
{
    const unsigned ge = (((c & BYTES_LO) + (0x80u - ncls) * BYTES_ONE) | c) & BYTES_HI;
    return ov_nz80(c) & ~ge;
}
// 0xff in every byte of x that holds 0x80 (x has no other bits)
__device__ __forceinline__ unsigned ov_expand(unsigned x80) { return (x80 >> 7) * 0xffu; }
// floor(i / d) as mulhi(i, m) with m = floor(2^32 / d) + 1: exact for 2 <= d and i d < 2^32 (here i < 2^14, d < 2^8).  Integers only.
__device__ __forceinline__ unsigned ov_recip(int d) { return (unsigned)(0x100000000ull / (unsigned)d) + 1u; }
__device__ __forceinline__ int ov_div(int i, unsigned m) { return (int)__umulhi((unsigned)i, m); }
__device__ __forceinline__ int ov_div(int i, int d, unsigned m) { return d == 1 ? i : ov_div(i, m); }   // (d uniform; d = 1 has no such m)
// the low n bytes of a word set (n <= 0: none, n >= 4: all)
__device__ __forceinline__ unsigned ov_below(int n) { return n <= 0 ? 0u : (n >= 4 ? 0xffffffffu : (1u << (8 * n)) - 1u); }

// The rows y0 .. y0 + trows - 1 of `frame` [h0, w0] into the tile (see the head of the file).  Every 16-byte chunk of the tile is written
// once, by one lane.
__device__ __forceinline__ void ov_stage(uint8_t* tile, const uint8_t* frame, int h0, int w0, int y0, int trows, int P)
{
    const int cpr = P >> 4, nchunk = trows * cpr, hw = h0 * w0;   // (cpr >= 4)
    const unsigned cinv = ov_recip(cpr);
    const unsigned fa = (unsigned)(reinterpret_cast<uintptr_t>(frame) & 15u);
    for (int ci = threadIdx.x; ci < nchunk; ci += OV_NT) {
        const int r = ov_div(ci, cinv), j = ci - r * cpr, y = y0 + r;
        unsigned w[4] = {0u, 0u, 0u, 0u};
        if (y >= 0 && y < h0) {
            const int q = y * w0;                          // the row's first byte of the frame
            const int lo = (int)((fa + (unsigned)q) & 15u) + 16 - 16 * j, hi = lo + w0;   // the row's pixels are the bytes [lo, hi) of chunk j
            if (hi > 0 && lo < 16) {
                const int p = q - lo;                      // the chunk's first byte of the frame; frame + p is 16-byte aligned
                if (p >= 0 && p + 16 <= hw) {
                    const uint4 v = *reinterpret_cast<const uint4*>(frame + p);
                    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
#pragma unroll
                    for (int k = 0; k < 4; ++k) w[k] &= ov_below(hi - 4 * k) & ~ov_below(lo - 4 * k);
                } else {                                   // the frame's first or last chunk: only the row's own bytes, which lie inside it
#pragma unroll
                    for (int b = 0; b < 16; ++b)
                        if (b >= lo && b < hi) w[b >> 2] |= (unsigned)frame[p + b] << (8 * (b & 3));
                }
            }
        }
        *reinterpret_cast<uint4*>(tile + 16 * ci) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// n[0..5] = the 24 bytes of the tile from byte L on (L >= 0 at any alignment; the seven words read lie inside L's LDS row)
__device__ __forceinline__ void ov_window(const uint8_t* tile, int L, unsigned (&n)[6])
{
    const unsigned* p = reinterpret_cast<const unsigned*>(tile + (L & ~3));
    const unsigned sh = (unsigned)L & 3u;
    unsigned v[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) v[i] = p[i];
#pragma unroll
    for (int i = 0; i < 6; ++i) n[i] = __builtin_amdgcn_alignbyte(v[i + 1], v[i], sh);
}

// The sixteen pixels x .. x + 15 of tile row tr (native row y, q = y w0): c = their bytes, cls = 0x80 per class byte, cont = 0x80 per
// contour pixel.  fa = the frame's address mod 16.  Pixels past the row's end come out as what the padding holds: not drawn.
template <int WD>
__device__ __forceinline__ void ov_contour(const uint8_t* tile, int P, int tr, unsigned fa, int q, int w0, int x, unsigned ncls,
                                           unsigned (&c)[4], unsigned (&cls)[4], unsigned (&cont)[4])
{
    unsigned n0[6];
    ov_window(tile, tr * P + 16 + (int)((fa + (unsigned)q) & 15u) + x - 3, n0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = __builtin_amdgcn_alignbyte(n0[j + 1], n0[j], 3);
        cls[j] = ov_cls80(c[j], ncls);
        cont[j] = 0u;
    }
    if (!(cls[0] | cls[1] | cls[2] | cls[3])) return;
    unsigned diff[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int dy = -WD; dy <= WD; ++dy) {
        const int r = WD - (dy < 0 ? -dy : dy);
        unsigned nd[6];
        if (dy == 0) {
#pragma unroll
            for (int i = 0; i < 6; ++i) nd[i] = n0[i];
        } else {
            // (a row outside the frame is a row of zeros at whatever alignment this comes to)
            ov_window(tile, (tr + dy) * P + 16 + (int)((fa + (unsigned)(q + dy * w0)) & 15u) + x - 3, nd);
        }
#pragma unroll
        for (int dx = -r; dx <= r; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const int o = 3 + dx;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned v = (o & 3) ? __builtin_amdgcn_alignbyte(nd[j + o / 4 + 1], nd[j + o / 4], (unsigned)(o & 3)) : nd[j + o / 4];
                diff[j] |= v ^ c[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) cont[j] = ov_nz80(diff[j]) & cls[j];
}

template <int WD, bool REF>
__global__ __launch_bounds__(OV_NT) void overlay_native_kernel(OvArgs a)
{
    extern __shared__ uint4 ov_lds[];                      // (16-byte aligned: the tiles take 16-byte stores)
    uint2* s_tab = reinterpret_cast<uint2*>(ov_lds);
    uint8_t* s_m = reinterpret_cast<uint8_t*>(ov_lds) + OV_PAL_BYTES;
    const int tid = threadIdx.x;
    const unsigned ncls = (unsigned)a.ncls, alpha = (unsigned)a.alpha;
    if (tid < OV_TAB) {                                    // (read behind the first item's barrier)
        // entry t = (C, ca, ga) as x = the red and blue of C times ca, plus the rounding halves, y = the green's | ga << 16: a pixel's
        // channels are (x or y + g ga) >> 8
        const unsigned C = tid == 0 ? 0u : a.pal[tid < 8 ? tid : tid - 8];
        const unsigned ca = tid == 0 ? 0u : (tid < 8 ? alpha : 256u), ga = 256u - ca;
        s_tab[tid] = make_uint2((C & 0x00ff00ffu) * ca + 0x00800080u, (((C >> 8) & 0xffu) * ca + 128u) | ga << 16);
    }
    const long long per_clip = (long long)a.T * a.maxbands;
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const auto [clip, t, band] = native_item(item, per_clip, a.maxbands);      // (clip < OV_CLIPS)
        const OvClip c = a.c[clip];
        if (band >= c.nbands) continue;                    // (uniform: a smaller clip of the launch has fewer bands)
        const int h0 = c.h0, w0 = c.w0, row0 = band * c.rpb;
        const int rows = h0 - row0 < c.rpb ? h0 - row0 : c.rpb;
        const int P = ov_pitch(w0), trows = rows + 2 * WD;
        const size_t fpos = (size_t)c.off + (size_t)t * (size_t)(h0 * w0);
        const uint8_t* gf = a.grey + fpos;
        const uint8_t* mf = a.mask + fpos;
        const uint8_t* rf = REF ? a.ref + fpos : nullptr;
        uint8_t* of = a.out + 3 * fpos;
        uint8_t* s_r = s_m + trows * P;                    // (at most the launch's largest tile in front of it)
        ov_stage(s_m, mf, h0, w0, row0 - WD, trows, P);
        if (REF) ov_stage(s_r, rf, h0, w0, row0 - WD, trows, P);
        __syncthreads();
        const unsigned fam = (unsigned)(reinterpret_cast<uintptr_t>(mf) & 15u), far = (unsigned)(reinterpret_cast<uintptr_t>(rf) & 15u);
        const int rpr = 1 + (w0 + OV_RUN - 1) / OV_RUN;    // runs of a row: the head and at most ceil(w0 / 16) more
        const int nrun = rows * rpr;                       // (<= OV_BAND_RUNS, or one row's)
        // The slots are numbered so that the runs that may be ragged meet in the band's last lanes: first the runs 1 .. nsure of every row,
        // which are full whatever the row's head (15 + 16 nsure <= w0), then every row's other slots -- its head and the one or two runs
        // behind the sure ones.  A wave of sure runs skips the byte accesses altogether.
        const int nsure = w0 >= 15 ? (w0 - 15) / OV_RUN : 0, nedge = rpr - nsure, sure = rows * nsure;   // (nedge is 2 or 3)
        const unsigned sinv = ov_recip(nsure > 1 ? nsure : 2), einv = ov_recip(nedge);
        for (int i = tid; i < nrun; i += OV_NT) {
            int rr, j;
            if (i < sure) {
                rr = ov_div(i, nsure, sinv);
                j = 1 + i - rr * nsure;
            } else {
                rr = ov_div(i - sure, einv);
                const int e = i - sure - rr * nedge;
                j = e == 0 ? 0 : nsure + e;
            }
            const int q = (row0 + rr) * w0;                // the row's first pixel of the frame
            // the head: the h in 0..15 with 3 h = -(the row's address in out) mod 16 (3 * 11 = 1 mod 16)
            int head = (int)(((0u - (unsigned)(reinterpret_cast<uintptr_t>(of) + (uintptr_t)(3 * q))) * 11u) & 15u);
            if (head > w0) head = w0;
            const int x = j == 0 ? 0 : head + OV_RUN * (j - 1);
            const int n = j == 0 ? head : (w0 - x < OV_RUN ? w0 - x : OV_RUN);
            if (n <= 0) continue;                          // (an empty head, or the spare run of a row with one)
            const bool full = n == OV_RUN;
            // the grey bytes, four pixels to a word; a byte past the run's end is neither loaded nor used
            unsigned gw[4] = {0u, 0u, 0u, 0u};
            const uint8_t* gp = gf + q + x;
            if (full && gdkvm_aligned16(gp)) {
                const uint4 v = *reinterpret_cast<const uint4*>(gp);
                gw[0] = v.x; gw[1] = v.y; gw[2] = v.z; gw[3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < OV_RUN; ++k)
                    if (k < n) gw[k >> 2] |= (unsigned)gp[k] << (8 * (k & 3));
            }
            unsigned mc[4], mcls[4], mcont[4], rc[4] = {0u, 0u, 0u, 0u}, rcont[4] = {0u, 0u, 0u, 0u};
            ov_contour<WD>(s_m, P, rr + WD, fam, q, w0, x, ncls, mc, mcls, mcont);
            if (REF) {
                unsigned rcls[4];
                ov_contour<WD>(s_r, P, rr + WD, far, q, w0, x, ncls, rc, rcls, rcont);
            }
            unsigned ow[12];
            if (!(mcls[0] | mcls[1] | mcls[2] | mcls[3] | rcont[0] | rcont[1] | rcont[2] | rcont[3])) {
                // nothing of either mask in this run: the grey value in three channels
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const unsigned g0 = gw[w] & 0xffu, g1 = (gw[w] >> 8) & 0xffu, g2 = (gw[w] >> 16) & 0xffu, g3 = gw[w] >> 24;
                    ow[3 * w + 0] = g0 * 0x010101u | g1 << 24;
                    ow[3 * w + 1] = g1 * 0x0101u | g2 * 0x01010000u;
                    ow[3 * w + 2] = g2 | g3 * 0x01010100u;
                }
            } else {
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    // the table entry of each of the word's four pixels, a byte each: k in a class, 8 + k on its contour, 16 + k' on the
                    // ref's contour where the mask's does not cover it, 0 elsewhere
                    unsigned tw = (mc[w] & ov_expand(mcls[w])) + ((mcont[w] >> 7) << 3);
                    if (REF) {
                        const unsigned sel = ov_expand(rcont[w] & ~mcont[w]);
                        tw = (tw & ~sel) | (((rc[w] & 0x07070707u) | 0x10101010u) & sel);
                    }
                    unsigned px[4];                        // R | G << 8 | B << 16 of the word's four pixels
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const unsigned g = (gw[w] >> (8 * e)) & 0xffu;
                        const uint2 t = s_tab[(tw >> (8 * e)) & 0xffu];                                   // (< OV_TAB)
                        // ga + ca <= 256: a channel's sum is at most 255 * 256 + 128 < 2^16, so red and blue share a word
                        const unsigned gga = g * (t.y >> 16);
                        const unsigned rb = ((t.x + (gga | gga << 16)) >> 8) & 0x00ff00ffu;
                        px[e] = rb | ((((t.y & 0xffffu) + gga) >> 8) << 8);
                    }
                    ow[3 * w + 0] = px[0] | px[1] << 24;
                    ow[3 * w + 1] = px[1] >> 8 | px[2] << 16;
                    ow[3 * w + 2] = px[2] >> 16 | px[3] << 8;
                }
            }
            uint8_t* o = of + 3 * (q + x);
            if (full && gdkvm_aligned16(o)) {                 // (every full run behind the head is)
                uint4* o4 = reinterpret_cast<uint4*>(o);
                o4[0] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
                o4[1] = make_uint4(ow[4], ow[5], ow[6], ow[7]);
                o4[2] = make_uint4(ow[8], ow[9], ow[10], ow[11]);
            } else {
#pragma unroll
                for (int k = 0; k < 3 * OV_RUN; ++k)
                    if (k < 3 * n) o[k] = (uint8_t)(ow[k >> 2] >> (8 * (k & 3)));
            }
        }
        __syncthreads();                                   // (the next item stages into the same tiles)
    }
}

inline int ov_rows_per_band(int h0, int w0)
{
    int rpb = OV_BAND_RUNS / (1 + (w0 + OV_RUN - 1) / OV_RUN);   // the most whole rows whose run slots are at most OV_BAND_RUNS
    if (rpb < 1) rpb = 1;
    if (rpb > OV_BAND_ROWS) rpb = OV_BAND_ROWS;
    return rpb > h0 ? h0 : rpb;
}

template <int WD>
void ov_launch(bool ref, dim3 grid, size_t lds, hipStream_t st, const OvArgs& a)
{
    if (ref) hipLaunchKernelGGL((overlay_native_kernel<WD, true>), grid, dim3(OV_NT), lds, st, a);
    else hipLaunchKernelGGL((overlay_native_kernel<WD, false>), grid, dim3(OV_NT), lds, st, a);
}

}  // namespace

// The kernel keeps a band in LDS and everything else in registers: no workspace for any shape.
extern "C" size_t gdkvm_overlay_native_workspace_bytes(int clips, int T, int ncls, int width)
{
    (void)clips; (void)T; (void)ncls; (void)width;
    return 0;
}

extern "C" int gdkvm_overlay_native(const uint8_t* grey, const uint8_t* mask, const uint8_t* ref, const int32_t* sizes, const uint8_t* pal,
                                    const uint8_t* ref_pal, uint8_t* out, size_t native_bytes, void* workspace, size_t workspace_bytes,
                                    int clips, int T, int ncls, int width, int alpha, void* stream)
{
    if (clips < 0 || T < 1 || ncls < 2 || ncls > 8 || width < 1 || width > OV_MAX_WIDTH || alpha < 0 || alpha > 256)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "overlay_native: bad arguments clips=%d T=%d ncls=%d width=%d alpha=%d (clips >= 0, T >= 1, ncls in "
                          "2..8, width in 1..%d, alpha in 0..256)", clips, T, ncls, width, alpha, OV_MAX_WIDTH);
    if (clips == 0) return GDKVM_OK;
    if (!grey || !mask || !sizes || !pal || !out)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "overlay_native: null pointer (grey, mask, the host sizes, the host palette and out are required)");
    if (ref && !ref_pal) return gdkvm_fail(GDKVM_ERR_SHAPE, "overlay_native: ref_pal required with a ref");
    size_t total;
    if (int rc = native_check_clips("overlay_native", "frames", sizes, nullptr, native_bytes, clips, T, total)) return rc;
    if (native_overlap(out, 3 * total, grey, total) || native_overlap(out, 3 * total, mask, total) ||
        (ref && native_overlap(out, 3 * total, ref, total)))
        return gdkvm_fail(GDKVM_ERR_SHAPE, "overlay_native: out must overlap none of grey, mask and ref");
    const size_t need = gdkvm_overlay_native_workspace_bytes(clips, T, ncls, width);
    if (int rc = mask_check_workspace("overlay_native", 0, 0, need, workspace, workspace_bytes)) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    size_t tile = 0;                                       // the current launch's largest tile: the launch callable clears it for the next
    return native_launches<OvArgs, OV_CLIPS>(sizes, clips, T, [&](OvArgs& a, int k, int, int h0, int w0, size_t off) {
        const int rpb = ov_rows_per_band(h0, w0), nbands = (h0 + rpb - 1) / rpb;
        a.c[k] = OvClip{(unsigned long long)off, h0, w0, rpb, nbands};
        const size_t tb = (size_t)(rpb + 2 * width) * (size_t)ov_pitch(w0);
        if (tb > tile) tile = tb;
        return nbands;
    }, [&](OvArgs& a, int, int nb) -> int {
        a.grey = grey; a.mask = mask; a.ref = ref; a.out = out;
        a.T = T; a.ncls = ncls; a.alpha = alpha;
        for (int k = 1; k < ncls; ++k) {                   // (class 0 is never drawn)
            a.pal[k] = (unsigned)pal[3 * k] | (unsigned)pal[3 * k + 1] << 8 | (unsigned)pal[3 * k + 2] << 16;
            if (ref) a.pal[8 + k] = (unsigned)ref_pal[3 * k] | (unsigned)ref_pal[3 * k + 1] << 8 | (unsigned)ref_pal[3 * k + 2] << 16;
        }
        a.items = (long long)nb * (long long)T * (long long)a.maxbands;
        const dim3 grid = native_grid(a.items, OV_MAX_WG);
        const size_t lds = OV_PAL_BYTES + (ref ? 2 : 1) * tile;   // (<= 192 + 2 * 9 * 2112: below the 64 KiB a launch may ask for)
        tile = 0;
        switch (width) {
            case 1: ov_launch<1>(ref != nullptr, grid, lds, st, a); break;
            case 2: ov_launch<2>(ref != nullptr, grid, lds, st, a); break;
            default: ov_launch<3>(ref != nullptr, grid, lds, st, a);
        }
        GDKVM_LAUNCH_CHECK("overlay_native_kernel");
        return GDKVM_OK;
    });
}
