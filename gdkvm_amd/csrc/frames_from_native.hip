// frames_from_native.hip -- take a ragged batch of native-size uint8 clips to the network's grid [H, W] by an exact-integer area (box)
// average and cast to the model's input dtype in the same pass (what predict.py's front end and tools/convert_camus.py --resample area are
// made of).  include/gdkvm.h holds the rule: N(i, j) = sum over k, l of wy(i, k) wx(j, l) v(k, l) with the integer overlap weights of the
// two pixel lattices, q = floor((2 N + h0 w0) / (2 h0 w0)), and every plane of the output holds q, float(q) * (1 / 255) or that rounded
// once to bf16.  out depends on neither the schedule nor the path taken.  No floating-point code in front of the final cast, no atomics.
//
// The native sizes differ from clip to clip, so the native frames are ragged: native_clips.hpp holds the launcher's side of that; a clip's
// entry here is its offset and its band geometry, FN_CLIPS of them 2.5 KB of the 4 KB an argument block may have.
//
// A workgroup of 256 lanes owns a BAND of grid rows of one (clip, frame): as many as one CHUNK of native rows covers, a chunk being the
// native rows whose bytes fit FN_CHUNK_BYTES of LDS and whose column sums fit FN_HS_WORDS (8 grid rows of a 549 x 778 frame on a 256 x 256
// grid: 19 or 20 native rows, 15 KB).  A band with more native rows than a chunk (2048 x 2048 to 16 x 16: 129 rows of 2048 bytes per grid
// row) walks them chunk after chunk.  The native rows of a chunk follow each other in memory, so a chunk is ONE byte range of the frame,
// read once with 16-byte loads on the grid of its own ADDRESSES (h0 w0 is odd as often as not, so every frame starts at another
// alignment): up to 15 head bytes and a ragged tail by byte loads, as mask_to_native.hip cuts its runs.  Only the native rows on a band's
// edge are read by two workgroups; a row that straddles two grid rows inside a band is read once.  All loads of a chunk are issued before
// the first is waited for, and the next chunk's before the current one is summed.
//
// Per chunk, three steps with a barrier between them:
//   1. FOLD: item (native row r, grid column j, part p) sums wx(j, l) v(r, l) over its share of the column's native range into a 32-bit
//      word of LDS (at most 255 w0 < 2^19).  The range floor(j w0 / W) .. ceil((j + 1) w0 / W) - 1 of every column is divided ONCE per
//      band into a table, not per row; a column with more than FN_PART native pixels is cut into P = 2^pl parts, so that 3 x 2048 to
//      2 x 5 (410 bytes per column) still spreads over the lanes.  A lane keeps its (row, column) and steps the row: nothing is divided.
//      Of a column's native pixels only the first and the last overlap it in part (their weights go into the table too); the ones
//      between them all weigh W, so a fold is two multiplications and a sum of bytes.
//   2. ACCUMULATE: item (grid row i, vertical part pv, column j, part p) adds wy(i, k) * fold(k, j, p) over every PV-th native row k of
//      the chunk that overlaps i into ITS OWN word of LDS -- no two lanes share a word, so there is nothing to make atomic.  PV = 2^pvl
//      parts per grid row when a grid row covers more than FN_PART native rows (2048 x 3 to 5 x 2: 411 rows per grid row).  The item
//      index is carried in (row, column) form with the constants 256 / WP and 256 % WP.
//   3. (after the last chunk) the P PV partial sums of a pixel are added -- in a fixed order, and integer sums commute anyway -- the byte
//      q is found WITHOUT a division: m = floor(2^32 / d) with d = 2 h0 w0 (the launcher's, per clip) gives q' = mulhi(x, m) in {q - 1, q} for every x < 2^32
//      (x / d - x m / 2^32 = x (2^32 - m d) / (d 2^32) < x / 2^32 < 1), and one compare of the remainder x - q' d against d decides: exact
//      over the whole range.  The C planes are written from the one value, 16 bytes per store where the band's first element and its
//      length allow (out is 16-byte aligned, so that is decided per band and is the same for every plane), element by element otherwise.
//
// The grid follows the clip with the most bands of the launch: item = (clip, frame, band) over clips x T x maxbands, and a workgroup whose
// band lies past its clip's last leaves at once.  More than FN_MAX_WG items are taken grid-stride.

#include "native_clips.hpp"

namespace {

constexpr int FN_NT = 256;
constexpr int FN_CHUNK_BYTES = GDKVM_FRAMES_FROM_NATIVE_CHUNK_BYTES;   // native bytes of a chunk in LDS (gdkvm.h)
constexpr int FN_HS_WORDS = GDKVM_FRAMES_FROM_NATIVE_HS_WORDS;         // folded column sums of a chunk: native rows x W P
constexpr int FN_ACC_WORDS = GDKVM_FRAMES_FROM_NATIVE_ACC_WORDS;       // a band's accumulators: grid rows x PV x W P
constexpr int FN_PART = GDKVM_FRAMES_FROM_NATIVE_PART;                 // native pixels of a column (rows of a grid row) beyond which it is cut
constexpr int FN_MAX_WG = GDKVM_FRAMES_FROM_NATIVE_MAX_WG;             // workgroups per launch; more items than that are walked grid-stride
constexpr int FN_CLIPS = GDKVM_FRAMES_FROM_NATIVE_CLIPS;               // clips per launch
constexpr int FN_BAND_ROWS = GDKVM_FRAMES_FROM_NATIVE_BAND_ROWS;       // grid rows of a band at most
constexpr int FN_MAX_GRID = 1024, FN_MAX_WP = 1024;
constexpr int FN_BATCH = 8, FN_ROWS = 4;                               // native bytes, and folds, a lane reads from LDS before it uses the first
constexpr int FN_U8 = 0, FN_F32 = 1, FN_BF16 = 2;                      // out_dtype (gdkvm.h)
static_assert(FN_CHUNK_BYTES >= NATIVE_MAX_SIDE && FN_CHUNK_BYTES % 16 == 0, "a chunk holds at least one native row");
static_assert(FN_CHUNK_BYTES / 16 + 1 <= 4 * FN_NT, "a lane carries a chunk's vectors in four registers of 16 bytes");
static_assert(FN_HS_WORDS >= FN_MAX_WP && FN_ACC_WORDS >= FN_MAX_WP && FN_ACC_WORDS <= FN_HS_WORDS, "one row of parts fits both; the sums fit the fold words");

struct FnClip {
    unsigned long long off;                                // the clip's first byte in native
    int h0, w0, rpb, nbands;                               // native size, grid rows per band, bands per frame
    int crow, parts;                                       // native rows per chunk; pl | pvl << 8
    unsigned recip, pad;                                   // floor(2^32 / (2 h0 w0)): the reciprocal the rounding division multiplies by
};
struct FnArgs {
    const uint8_t* native;                                 // (the buffer's base: off is absolute)
    void* out;                                             // (the buffers' bases: off is absolute, clip0 the launch's first clip)
    long long items;
    int T, C, H, W, maxbands, clip0;
    FnClip c[FN_CLIPS];
};
static_assert(sizeof(FnArgs) <= 2688, "the clip table travels in the kernel arguments");

// the overlap of cell a of a lattice with cells of size sb with cell b of one with cells of size sa, in units of 1 / (sa sb): wy and wx
__device__ __forceinline__ unsigned fn_weight(int a, int sb, int b, int sa)
{
    const int asb = __mul24(a, sb), bsa = __mul24(b, sa);  // (every factor <= 2048, every product < 2^22: full-rate 24-bit multiplies)
    const int lo = asb > bsa ? asb : bsa, hi = asb + sb < bsa + sa ? asb + sb : bsa + sa;
    return (unsigned)(hi - lo);                            // (callers stay inside the overlap range: positive)
}

// A chunk's bytes in memory, cut on the 16-byte grid of their addresses, and the registers a lane carries them in from the loads to the
// LDS writes: every load of a chunk is issued before anything waits for one, and the next chunk's are issued before the current one is
// folded, so a workgroup waits for memory once per band, not once per load.
constexpr int FN_VEC_PER_LANE = (FN_CHUNK_BYTES / 16 + FN_NT - 1) / FN_NT;
struct FnSpan {
    const uint8_t* g;                                      // the chunk's first byte
    int rows, mis, head, nvec, tail;                       // native rows; g's address mod 16; head bytes, 16-byte vectors, tail bytes
};
struct FnRegs {
    u32x4 v[FN_VEC_PER_LANE];
    unsigned hb, tb;
};
__device__ __forceinline__ FnSpan fn_span(const uint8_t* src, int ka, int k1, int crow, int w0)
{
    FnSpan s;
    s.rows = ka + crow < k1 ? crow : k1 - ka;
    s.g = src + (size_t)(ka * w0);
    const int len = s.rows * w0;                           // (<= FN_CHUNK_BYTES)
    s.mis = (int)(reinterpret_cast<uintptr_t>(s.g) & 15u);
    s.head = (16 - s.mis) & 15;
    if (s.head > len) s.head = len;
    s.nvec = (len - s.head) >> 4;
    s.tail = len - s.head - 16 * s.nvec;
    return s;
}
__device__ __forceinline__ void fn_fetch(const FnSpan& s, int tid, FnRegs& r)
{
    r.hb = tid < s.head ? (unsigned)s.g[tid] : 0u;
    r.tb = tid < s.tail ? (unsigned)s.g[s.head + 16 * s.nvec + tid] : 0u;
    const u32x4* gv = reinterpret_cast<const u32x4*>(s.g + s.head);
    static_for<0, FN_VEC_PER_LANE>([&](auto u) {
        if (tid + FN_NT * u.value < s.nvec) r.v[u.value] = gv[tid + FN_NT * u.value];
    });
}
// byte b of the chunk goes to raw[mis + b]: LDS and global addresses agree mod 16 (mis + head is 0 or 16 whenever there is a vector)
__device__ __forceinline__ void fn_commit(const FnSpan& s, int tid, const FnRegs& r, uint4* raw4)
{
    uint8_t* raw = reinterpret_cast<uint8_t*>(raw4);
    if (tid < s.head) raw[s.mis + tid] = (uint8_t)r.hb;
    if (tid < s.tail) raw[s.mis + s.head + 16 * s.nvec + tid] = (uint8_t)r.tb;
    u32x4* lv = reinterpret_cast<u32x4*>(raw4) + ((s.mis + s.head) >> 4);
    static_for<0, FN_VEC_PER_LANE>([&](auto u) {
        if (tid + FN_NT * u.value < s.nvec) lv[tid + FN_NT * u.value] = r.v[u.value];
    });
}

template <int DT>
__global__ __launch_bounds__(FN_NT) void frames_from_native_kernel(FnArgs a)
{
    using elem_t = std::conditional_t<DT == FN_U8, uint8_t, std::conditional_t<DT == FN_F32, float, unsigned short>>;
    constexpr int PER = 16 / (int)sizeof(elem_t);          // elements of a 16-byte store
    __shared__ uint4 s_raw4[FN_CHUNK_BYTES / 16 + 1];      // byte b of the chunk at s_raw[mis + b]: LDS and global addresses agree mod 16
    __shared__ unsigned s_hs[FN_HS_WORDS];
    __shared__ unsigned s_acc[FN_ACC_WORDS];
    __shared__ unsigned s_seg[FN_MAX_WP], s_wgt[FN_MAX_WP];            // part jp: first native column | columns << 16; wx of its first | of its last << 16
    __shared__ unsigned short s_klo[FN_BAND_ROWS], s_khi[FN_BAND_ROWS];   // grid row i0 + il: its first native row, one past its last
    uint8_t* s_raw = reinterpret_cast<uint8_t*>(s_raw4);
    const int tid = threadIdx.x, H = a.H, W = a.W, C = a.C;
    const long long per_clip = (long long)a.T * a.maxbands;
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        int clip, t, band;                                 // (clip < FN_CLIPS)
        if (a.items <= 0x7fffffffll) {                     // (uniform) the usual case: 32-bit divisions, a fifth of the 64-bit ones' cost
            const unsigned it = (unsigned)item, pc = (unsigned)per_clip, mb = (unsigned)a.maxbands;
            clip = (int)(it / pc);
            const unsigned rem = it - (unsigned)clip * pc;
            t = (int)(rem / mb); band = (int)(rem - (unsigned)t * mb);
        } else {
            const NativeItem it64 = native_item(item, per_clip, a.maxbands);
            clip = it64.clip; t = it64.t; band = it64.band;
        }
        const FnClip c = a.c[clip];
        if (band >= c.nbands) continue;                    // (uniform: a smaller clip of the launch has fewer bands)
        const int h0 = c.h0, w0 = c.w0, i0 = band * c.rpb;
        const int nR = H - i0 < c.rpb ? H - i0 : c.rpb;
        const int pl = c.parts & 0xff, pvl = c.parts >> 8, P = 1 << pl, WP = W << pl, nV = nR << pvl;   // nV: (grid row, vertical part) pairs
        const int nacc = nV * WP;                          // (<= FN_ACC_WORDS: the launcher chose rpb and pvl so)
        const uint8_t* src = a.native + (size_t)c.off + (size_t)t * (size_t)(h0 * w0);

        const int k0 = (i0 * h0) / H, k1 = ((i0 + nR) * h0 + H - 1) / H;   // the band's native rows [k0, k1)
        FnSpan sp = fn_span(src, k0, k1, c.crow, w0);
        FnRegs rg;
        fn_fetch(sp, tid, rg);                             // (in flight while the tables are made)
        __syncthreads();                                   // (the last item's readers of the tables and sums are done)
        for (int jp = tid; jp < WP; jp += FN_NT) {
            const int j = jp >> pl, p = jp & (P - 1);
            const int lo = (j * w0) / W, n = ((j + 1) * w0 + W - 1) / W - lo;
            const int b0 = lo + ((n * p) >> pl), b1 = lo + ((n * (p + 1)) >> pl);
            // (a part may be empty: its weights are then never used; b0 <= 2047, the count and the weights <= 2049 and 1024)
            s_seg[jp] = (unsigned)b0 | ((unsigned)(b1 - b0) << 16);
            s_wgt[jp] = b1 > b0 ? fn_weight(j, w0, b0, W) | (fn_weight(j, w0, b1 - 1, W) << 16) : 0u;
        }
        for (int il = tid; il < nR; il += FN_NT) {
            s_klo[il] = (unsigned short)(((i0 + il) * h0) / H);
            s_khi[il] = (unsigned short)(((i0 + il + 1) * h0 + H - 1) / H);
        }
        for (int x = tid; x < nacc; x += FN_NT) s_acc[x] = 0u;
        // a lane's first (row, part) of a 256-wide sweep over rows of WP parts, and the step of the sweep: nothing is divided after this
        const int sq = FN_NT / WP, sr = FN_NT - sq * WP;
        const int r_first = tid / WP, jp_first = tid - r_first * WP;

        for (int ka = k0; ka < k1; ka += c.crow) {
            const int rows = sp.rows, kb = ka + rows, mis = sp.mis;
            __syncthreads();                               // (the tables are written; the last chunk's bytes and sums are read)
            // the chunk's bytes [ka w0, kb w0) of the frame: head bytes up to the 16-byte grid of the addresses, vectors, tail bytes
            fn_commit(sp, tid, rg, s_raw4);
            __syncthreads();
            if (kb < k1) {                                 // (uniform) the next chunk's loads, in flight behind this chunk's sums
                sp = fn_span(src, kb, k1, c.crow, w0);
                fn_fetch(sp, tid, rg);
            }
            // 1. fold every native row of the chunk into its W P column sums.  Only the first and the last native pixel of a grid column
            // overlap it in part: every pixel between them has the weight W, so a part is wf first + wl last + W (the sum of the rest).
            {
                auto fold = [&](int r, int jp, unsigned seg, unsigned wgt) {
                    const int lo = (int)(seg & 0xffffu), n = (int)(seg >> 16);
                    const uint8_t* px = s_raw + mis + __mul24(r, w0) + lo;
                    // FN_BATCH bytes per turn, all read before one is used (index clamped into the part, weight 0 past its end): with two
                    // or three waves to a SIMD a read that waits for the one before it costs the LDS latency each time
                    unsigned sum = 0u;
                    for (int e0 = 0; e0 < n; e0 += FN_BATCH) {
                        unsigned b[FN_BATCH];
#pragma unroll
                        for (int e = 0; e < FN_BATCH; ++e) b[e] = px[e0 + e < n ? e0 + e : n - 1];
#pragma unroll
                        for (int e = 0; e < FN_BATCH; ++e) {
                            const int x = e0 + e;
                            const unsigned w = x == 0 ? (wgt & 0xffffu) : x < n - 1 ? (unsigned)W : x == n - 1 ? (wgt >> 16) : 0u;
                            sum += __umul24(w, b[e]);      // (weights <= 1024)
                        }
                    }
                    s_hs[__mul24(r, WP) + jp] = sum;
                };
                if (sr == 0) {                             // (uniform) 256 is a multiple of W P: a lane keeps its part, row after row
                    const unsigned seg = s_seg[jp_first], wgt = s_wgt[jp_first];
                    for (int r = r_first; r < rows; r += sq) fold(r, jp_first, seg, wgt);
                } else {
                    int r = r_first, jp = jp_first;
                    while (r < rows) {
                        fold(r, jp, s_seg[jp], s_wgt[jp]);
                        r += sq; jp += sr;
                        if (jp >= WP) { jp -= WP; ++r; }
                    }
                }
            }
            __syncthreads();
            // 2. every (grid row, vertical part, column part) adds its native rows of the chunk into its own word
            {
                int vr = r_first, jp = jp_first;
                while (vr < nV) {
                    const int il = vr >> pvl, pv = vr & ((1 << pvl) - 1), i = i0 + il;
                    const int ks = (int)s_klo[il] > ka ? (int)s_klo[il] : ka, ke = (int)s_khi[il] < kb ? (int)s_khi[il] : kb;
                    unsigned acc = s_acc[__mul24(vr, WP) + jp];
                    // FN_ROWS folds per turn, all read before one is used (a row past the end is read as the last one and weighs 0)
                    for (int k0b = ks + pv; k0b < ke; k0b += FN_ROWS << pvl) {
                        unsigned f[FN_ROWS];
#pragma unroll
                        for (int e = 0; e < FN_ROWS; ++e) {
                            const int k = k0b + (e << pvl);
                            f[e] = s_hs[__mul24((k < ke ? k : k0b) - ka, WP) + jp];
                        }
#pragma unroll
                        for (int e = 0; e < FN_ROWS; ++e) {
                            const int k = k0b + (e << pvl);
                            if (k < ke) acc += __umul24(fn_weight(i, h0, k, H), f[e]);   // (a weight <= 1024 times a fold < 2^19)
                        }
                    }
                    s_acc[__mul24(vr, WP) + jp] = acc;
                    vr += sq; jp += sr;
                    if (jp >= WP) { jp -= WP; ++vr; }
                }
            }
        }
        __syncthreads();
        // 3. a pixel's partial sums -> N, into the fold words (nR W <= FN_ACC_WORDS <= FN_HS_WORDS, and nobody reads a fold any more)
        const int npix = nR * W;
        {
            const int q1 = FN_NT / W, r1 = FN_NT - q1 * W;
            int il = tid / W, j = tid - il * W;
            while (il < nR) {
                unsigned n = 0u;
                for (int pv = 0; pv < (1 << pvl); ++pv)
                    for (int p = 0; p < P; ++p) n += s_acc[__mul24((il << pvl) + pv, WP) + (j << pl) + p];
                s_hs[__mul24(il, W) + j] = n;
                il += q1; j += r1;
                if (j >= W) { j -= W; ++il; }
            }
        }
        __syncthreads();
        // q = floor((2 N + A) / (2 A)) by the reciprocal m = floor(2^32 / d) and one correction (the file's head), then the C planes
        const unsigned A = (unsigned)(h0 * w0), d = 2u * A, m = c.recip;
        const size_t plane = (size_t)H * (size_t)W;
        const size_t first = ((size_t)(a.clip0 + clip) * (size_t)a.T + (size_t)t) * (size_t)C * plane + (size_t)i0 * (size_t)W;   // the band in plane 0
        elem_t* o0 = static_cast<elem_t*>(a.out) + first;
        const bool vec = (plane % PER) == 0 && (first % PER) == 0;     // (out is 16-byte aligned: every plane's band then starts on the grid)
        auto value = [&](int x) -> elem_t {
            const unsigned num = 2u * s_hs[x] + A;         // (< 2^32)
            unsigned q = __umulhi(num, m);
            if (num - __umul24(q, d) >= d) ++q;            // (q' <= 255, d <= 2^23)
            if constexpr (DT == FN_U8) return (uint8_t)q;
            else if constexpr (DT == FN_F32) return (float)q * (1.0f / 255.0f);
            else return f32_to_bf16((float)q * (1.0f / 255.0f));
        };
        const int ngroup = (npix + PER - 1) / PER;
        for (int gidx = tid; gidx < ngroup; gidx += FN_NT) {
            const int x0 = gidx * PER;
            if (vec && x0 + PER <= npix) {
                union { uint4 v; elem_t e[PER]; } u;
#pragma unroll
                for (int e = 0; e < PER; ++e) u.e[e] = value(x0 + e);
                for (int ch = 0; ch < C; ++ch) *reinterpret_cast<uint4*>(o0 + (size_t)ch * plane + x0) = u.v;
            } else {
                for (int e = 0; e < PER && x0 + e < npix; ++e) {
                    const elem_t v = value(x0 + e);
                    for (int ch = 0; ch < C; ++ch) o0[(size_t)ch * plane + x0 + e] = v;
                }
            }
        }
    }
}

inline bool fn_shape_ok(int clips, int T, int C, int H, int W)
{
    return clips >= 0 && T >= 1 && C >= 1 && C <= 4 && H >= 1 && H <= FN_MAX_GRID && W >= 1 && W <= FN_MAX_GRID;
}
inline size_t fn_elem(int out_dtype) { return out_dtype == FN_U8 ? 1 : out_dtype == FN_F32 ? 4 : 2; }

// The band geometry of one clip (the file's head): P = 2^pl parts per column and PV = 2^pvl per grid row while one has more than FN_PART
// native pixels and the words allow, the native rows per chunk, and as many grid rows per band as one chunk covers.
inline FnClip fn_geometry(size_t off, int h0, int w0, int H, int W)
{
    int pl = 0, pvl = 0;
    const int spanx = (w0 + W - 1) / W + 1, spany = (h0 + H - 1) / H + 1;
    while ((spanx >> pl) > FN_PART && (W << (pl + 1)) <= FN_MAX_WP) ++pl;
    const int WP = W << pl;
    while ((spany >> pvl) > FN_PART && (WP << (pvl + 1)) <= FN_ACC_WORDS) ++pvl;
    int crow = FN_CHUNK_BYTES / w0 < FN_HS_WORDS / WP ? FN_CHUNK_BYTES / w0 : FN_HS_WORDS / WP;   // (>= 1: the static_asserts)
    if (crow > h0) crow = h0;
    int rpb = crow > 2 ? (int)(((long long)(crow - 2) * H) / h0) : 1;   // R grid rows cover at most R h0 / H + 2 native rows
    if (rpb > FN_ACC_WORDS / (WP << pvl)) rpb = FN_ACC_WORDS / (WP << pvl);
    if (rpb > FN_BAND_ROWS) rpb = FN_BAND_ROWS;
    if (rpb > H) rpb = H;
    if (rpb < 1) rpb = 1;
    return FnClip{(unsigned long long)off, h0, w0, rpb, (H + rpb - 1) / rpb, crow, pl | (pvl << 8),
                  (unsigned)(0x100000000ull / (2ull * (unsigned long long)(h0 * w0))), 0u};
}

}  // namespace

// The kernel keeps a band's bytes and sums in LDS: no workspace for any shape.
extern "C" size_t gdkvm_frames_from_native_workspace_bytes(int clips, int T, int C, int H, int W, int out_dtype)
{
    (void)clips; (void)T; (void)C; (void)H; (void)W; (void)out_dtype;
    return 0;
}

extern "C" int gdkvm_frames_from_native(const uint8_t* native, const int32_t* sizes, void* out, size_t native_bytes, void* workspace,
                                        size_t workspace_bytes, int clips, int T, int C, int H, int W, int out_dtype, void* stream)
{
    if (!fn_shape_ok(clips, T, C, H, W))
        return gdkvm_fail(GDKVM_ERR_SHAPE, "frames_from_native: bad shape clips=%d T=%d C=%d H=%d W=%d (T >= 1, C in 1..4, H, W in 1..1024)", clips,
                          T, C, H, W);
    if (out_dtype != FN_U8 && out_dtype != FN_F32 && out_dtype != FN_BF16)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "frames_from_native: out_dtype=%d is none of GDKVM_FRAMES_U8, GDKVM_FRAMES_F32, GDKVM_FRAMES_BF16", out_dtype);
    if (clips == 0) return GDKVM_OK;
    if (!native || !sizes || !out) return gdkvm_fail(GDKVM_ERR_SHAPE, "frames_from_native: null pointer (native, the host sizes and out are required)");
    if (int rc = mask_check_aligned16("frames_from_native", GDKVM_ERR_SHAPE, "out", {out})) return rc;
    size_t total;
    if (int rc = native_check_clips("frames_from_native", "frames", sizes, nullptr, native_bytes, clips, T, total)) return rc;
    const size_t frames = (size_t)clips * (size_t)T;
    if (native_overlap(out, frames * (size_t)C * (size_t)H * (size_t)W * fn_elem(out_dtype), native, total))
        return gdkvm_fail(GDKVM_ERR_SHAPE, "frames_from_native: out must not overlap native");
    const size_t need = gdkvm_frames_from_native_workspace_bytes(clips, T, C, H, W, out_dtype);
    if (int rc = mask_check_workspace("frames_from_native", H, W, need, workspace, workspace_bytes)) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return native_launches<FnArgs, FN_CLIPS>(sizes, clips, T, [&](FnArgs& a, int k, int, int h0, int w0, size_t off) {
        a.c[k] = fn_geometry(off, h0, w0, H, W);
        return a.c[k].nbands;
    }, [&](FnArgs& a, int b0, int nb) -> int {
        a.native = native;
        a.out = out;
        a.T = T; a.C = C; a.H = H; a.W = W; a.clip0 = b0;
        a.items = (long long)nb * (long long)T * (long long)a.maxbands;
        const dim3 grid = native_grid(a.items, FN_MAX_WG);
        switch (out_dtype) {
            case FN_U8: hipLaunchKernelGGL(frames_from_native_kernel<FN_U8>, grid, dim3(FN_NT), 0, st, a); break;
            case FN_F32: hipLaunchKernelGGL(frames_from_native_kernel<FN_F32>, grid, dim3(FN_NT), 0, st, a); break;
            default: hipLaunchKernelGGL(frames_from_native_kernel<FN_BF16>, grid, dim3(FN_NT), 0, st, a);
        }
        GDKVM_LAUNCH_CHECK("frames_from_native_kernel");
        return GDKVM_OK;
    });
}
