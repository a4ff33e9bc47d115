// conv3x3_tile.hip -- hand-written 3x3 / stride 1 / pad 1 convolution for the encoder / decoder layers with 128 .. 384 input
// channels, NHWC bf16, bias (+ residual) (+ ReLU) in the epilogue.  It replaces the composable_kernel
// template instantiations of round 1: the layers it serves work on small maps (14x14, 7x7, 28x28 at the EchoNet shapes), where the
// implicit-GEMM library kernels re-fetch every input pixel nine times through L2 and sit near 20 % of the MFMA rate.
//
//   * a workgroup (8 waves) owns a tile of up to 208 output pixels -- a whole 14x14 frame, four 7x7 frames, or a 7-row band of a
//     28x28 frame -- and 64 or 128 output channels;
//   * the input is walked in chunks of 64 channels: the chunk's halo band ((rows + 2) x (W + 2) pixels per frame, 128 B of
//     channels + padding per pixel: a ds_read_b128 of 16 consecutive pixels is conflict-free and every operand
//     address is base + immediate -- 128 B + 32 B in fact: CT_PIX = 160) is staged in LDS by LDS-DMA, double-buffered: chunk c+1
//     streams in while chunk c computes; the input may be the channel concatenation of TWO tensors (x2 / C1), fetched in place;
//     the DMA goes through a buffer descriptor over the tile's frames, whose range check zero-fills the pixels above and below the
//     frame; the padding slots and the left / right halo columns carry an offset that is always out of range;
//   * the four-wave forms (112-pixel tiles, two workgroups per CU) cut the maps whose rows tile 112 pixels but whose frames do not -- 14 x 14
//     (196 pixels in two tiles of 8 and 6 rows) and 7 x 7 (two frames, 98 pixels, per tile) -- ACROSS frame boundaries: 4 (16) frames
//     are one stacked image of seven full tiles where whole rows of one frame group made eight, an eighth of them padded pixel slots that
//     cost their LDS reads and MFMAs in every k-step.  A tile's band holds its 8 (16) rows frame segment by segment, ONE zero row between
//     two consecutive frames (the lower halo of one, the upper of the next), and a row above and below that holds data where it lies in the
//     same frame: <= 11 rows x 16 pixels (28 pieces, 57 KB of LDS per workgroup) and <= 21 x 9 (30 pieces, 61 KB) where the row tiles
//     took 10 x 16 (25 pieces, 51 KB) and 18 x 9 (26 pieces, 53 KB).  The layout depends only on the tile's phase (tile % 7) and the grid is
//     a multiple of 7, so a workgroup computes it once like any other geometry; the UP form keeps the row tiles;
//   * the nine taps are nine SHIFTED READS of that image; the weights never touch LDS: a wave owns one or two 16-channel output
//     tiles and streams their weight fragments (one 16-byte load each per k-step, three k-steps ahead, straight from L2) -- each
//     is used for all the wave's pixel tiles (7 MFMAs per load);
//     with weights packed in fragment order (gdkvm_conv3x3_pack_weights) such a load is one contiguous KiB;
//   * weights are the A operand, so a lane ends with 4 consecutive output channels of one pixel -- 8 with the channel permutation
//     ct_channel (16-byte stores / residual loads);
//   * the same kernel computes the training-mode data gradient (weights packed flipped and transposed);
//   * the UP form (gdkvm_conv_upcat_bias_act: the decoder's first convolutions) takes the first C1 input channels as the exact-2x bilinear
//     enlargement of a low-resolution tensor and builds them in the band itself: the DMA brings the low-resolution rows into a staging
//     area of LDS, and the chunk iteration expands them into its band buffer before it computes -- the enlarged tensor never exists.
// Arithmetic: fp32 accumulation over the same 9 C products as a library convolution, one rounding after the epilogue.
#include <atomic>
#include "gdkvm_device.hpp"

namespace {

constexpr int CT_CK = 64;                // input channels per LDS chunk
constexpr int CT_PIX = 160;              // bytes between LDS pixels: 8 data chunks + 2 padding chunks of 16 B (144 B is NOT
                                         // conflict-free for ds_read_b128: its 16-lane groups mix two lane quarters)
constexpr int CT_SLOTS = CT_PIX / 16;    // 16-byte LDS slots per pixel
constexpr int CT_MAXMT = 13;             // 16-pixel tiles per workgroup tile (208 pixels)
// wave grids <NWN, NTW>: 1 = <4, 1>, 2 = <4, 2>, 3 = <2, 2> (eight waves, tiles of up to 208 pixels); 4 = <4, 2> on FOUR waves with tiles of up to 112
// pixels, two workgroups per CU (round 4: 1 - 4 % faster than 2 on every K % 128 == 0 layer, profiles/r04_w_conv_half_tiles.txt), 5 = <2, 2> likewise
// (64 channels per workgroup); the defaults are the measured picks (tools/conv_probe.py; K = 64: <2, 2> since the
// weights are packed -- 121 against 129 us on the 192 -> 64 layer: half the LDS operand reads per MFMA, and the fourfold weight fetch is cheap now)
constexpr int CT_VARIANT_128 = 4, CT_VARIANT_64 = 3;

struct ConvTileArgs {
    const bf16_t* x; const bf16_t* w; const float* bias; const bf16_t* res; bf16_t* y;
    const bf16_t* x2; int C1;            // x2 != NULL: the input is the channel concatenation [x (C1 channels) ; x2 (C - C1)], never
                                         // materialised: a 64-channel chunk is fetched from the tensor it lies in (C1 % 64 == 0)
    int N, H, W, C, K;                   // frames, map, input / output channels
    int fpt, th, tiles_y, ntiles;        // frames per tile, rows per tile, row tiles per frame, tiles in all
    int bw, bh, band_px, npieces;        // band geometry: (th + 2) x (W + 2) pixels per frame; 1 KiB DMA pieces per chunk
    int relu;
    float inv_band, inv_bw, inv_tw, inv_w;   // 1 / (bh bw), 1 / bw, 1 / (th W), 1 / W: index arithmetic without integer division
    int perm;                                // K % 32 == 0: output channels permuted within groups of 32 (ct_channel)
    // Frame-stacked tiling (four-wave forms, not UP; stk = 0: off).  A group of sg frames is ONE image of sg H rows, cut into stk tiles of
    // th = 112 / W rows that run across frame boundaries (fpt = 1, tiles_y = 1; bh = the tallest band of the stk phases): no padded pixel.
    int stk, sg;                             // tiles per frame group, frames per group: stk th W = sg H W
    float inv_hw, inv_h1;                    // 1 / (H W), 1 / (H + 1)
};
// The UP form (conv3x3_upcat_kernel): x is lo [N, hl, wl, C1] with H = 2 hl, W = 2 wl, and the first C1 input channels are its bilinear
// enlargement, built in the band from a staging area of LDS that holds the low-resolution rows a tile needs: per frame of the tile, nlr
// rows from the tile's first source row on, 128 B (one chunk's channels) per pixel, no padding.
struct ConvUpArgs : ConvTileArgs {
    int hl, wl, nlr;                         // low-resolution map; staged rows per frame
    int stage_px, nstage;                    // fpt nlr wl staged pixels, in nstage 1 KiB DMA pieces (8 pixels each)
    int stage_off;                           // LDS byte offset of the staging area (behind the two bands and the dump slot)
    int nrp;                                 // row pairs 2 ip + 1, 2 ip + 2 that cover a band's bh rows: bh / 2 + 1
    float inv_slr, inv_wl, inv_ncp, inv_nrp; // 1 / (nlr wl), 1 / wl, 1 / (wl + 1), 1 / nrp
};

// Row j of the 16-channel output tile kt is output channel ct_channel(kt, j).  With K a multiple of 32 the two tiles of a
// 32-channel group interleave in fours, so that the accumulator rows 4g .. 4g+3 of BOTH tiles of a wave are 8 consecutive
// channels 32G + 8g .. +7: one 16-byte store (and residual load) per pixel and lane instead of two 8-byte ones.  The weights
// are addressed (or packed) in the same order, so the result is that of the plain order.
__host__ __device__ __forceinline__ int ct_channel(int kt, int j, int perm)
{
    return perm ? 32 * (kt >> 1) + 8 * (j >> 2) + 4 * (kt & 1) + (j & 3) : 16 * kt + j;
}

// Waves form an MW (pixel-tile group) x NWN (output-channel group) grid, MW NWN = 8; a wave owns NTW 16-channel output tiles (the
// workgroup 16 NTW NWN output channels) and every MW-th pixel tile (MTW of 13).  Per 32-deep k-step a wave reads MTW pixel
// fragments from LDS and NTW weight fragments from L2 for MTW NTW MFMAs; per workgroup that is 8 MTW KB of LDS reads against
// 32 MTW NTW cycles of MFMA per SIMD.  <4, 2> (MTW 7): 56 KB / 448 cycles; <2, 2> (MTW 4, the 64-channel layers): 32 KB / 256
// cycles where <4, 1> had 56 KB / 224 -- the LDS read rate (128 B per cycle) is the co-bound, so the grid follows the channels.
// NWV = 4, MAXMT = 7 (round 4 experiment, variant 4): FOUR waves per workgroup, each with the SAME work as a wave of <4, 2> (seven pixel
// tiles x two channel tiles), on a tile of half the pixels (112) -- so that TWO workgroups share a CU and drift apart: one's barrier,
// first-band wait and epilogue overlap the other's MFMAs (what conv3x3_c64 gains from its two workgroups per CU, profiles/r04_v_...).
// UP (ARGS = ConvUpArgs): the chunks below C1 are enlarged in place from lo -- fetch() brings the low-resolution rows into the staging
// area with the same PP pieces per wave, and the chunk iteration expands them into its band buffer before it computes (below).
template <int NWN, int NTW, bool PK, int NWV = 8, int MAXMT = CT_MAXMT, bool UP = false>
__global__ __launch_bounds__(64 * NWV, (NWV == 4 ? 2 : 1)) void conv3x3_tile_kernel(std::conditional_t<UP, ConvUpArgs, ConvTileArgs> a)
{
    constexpr int MW = NWV / NWN, MTW = (MAXMT + MW - 1) / MW;         // pixel-tile groups, pixel tiles per wave
    extern __shared__ __attribute__((aligned(16))) unsigned char ct_band[];    // [2][npieces * 1024] | 1 KiB dump slot | UP: [nstage * 1024] staging
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), wn = w % NWN, wm = w / NWN;
    const int H = a.H, W = a.W, C = a.C, K = a.K, BW = a.bw;
    const int band_bytes = a.npieces * 1024, nchunk = C / CT_CK;
    const int tpix = a.fpt * a.th * W;                     // output pixels of a full tile
    const int co0 = blockIdx.y * (16 * NTW * NWN) + 16 * NTW * wn;     // this wave's output channels co0 .. co0 + 16 NTW - 1
    // Frame-stacked tiling: a workgroup's tiles are gridDim.x apart and the launcher keeps gridDim.x a multiple of stk (or gives every workgroup
    // one tile), so ALL its tiles share the phase ph = tile % stk -- and with it the band layout, which is computed once below like the
    // row-tile geometry.  The tile starts at stacked row s0 = row m0 of the group's frame f0.  Pixel p of the tile is pixel poff + p of the
    // group; its frame f and row py give band row f rmul + py - rsub for tap (0, 0): (H + 1) rows per frame, ONE zero row between two frames.
    const bool stk = NWV == 4 && !UP && a.stk != 0;
    const int ph = stk ? (int)(blockIdx.x % (unsigned)a.stk) : 0, s0 = ph * a.th, f0 = stk ? s0 / H : 0, m0 = s0 - f0 * H;
    const int poff = stk ? ph * tpix : 0, pper = stk ? H * W : a.th * W, rmul = stk ? H + 1 : a.bh, rsub = stk ? s0 + f0 : 0;
    const float inv_pper = stk ? a.inv_hw : a.inv_tw;
    const int tdiv = stk ? a.stk : a.tiles_y, fpg = stk ? a.sg : a.fpt;           // tiles per frame group, frames per group

    // bias of this lane's output channels: asm loads, first thing, waited for with the first band (they are older than its pieces).  A load
    // the compiler sees would be "pending" to it at the bias's first use in EVERY iteration of the tile loop -- it cannot count across the
    // LDS-DMA in between -- and it drains vmcnt to 0 there: at the top of each tile's epilogue, on the operands just requested for the next tile.
    f32x4 bias4[NTW];
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        const int kt = min(co0 / 16 + nt, K / 16 - 1);     // (a tile past K: the last tile's bias, results never stored)
        const float* bp = a.bias + ct_channel(kt, 4 * g, a.perm);
        asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(bias4[nt]) : "v"(bp) : "memory");
    }

    // DMA piece geometry (tile-invariant): piece j = w + NWV u, slot d = 64 j + lane = CT_SLOTS pix + c; c >= 8 is padding.
    // A piece is fetched through a raw buffer descriptor that spans exactly the tile's frame group (nfr H W pixels of the tensor the chunk
    // lies in): a lane's source is ONE 32-bit byte offset from the group's first byte, g_off + a per-chunk scalar (the tile's first row and
    // the chunk's channels), and a lane whose offset is out of the descriptor's range gets zeros from the hardware -- the row above the
    // frame (a negative offset: huge as unsigned), the rows below it and the frames a ragged last group lacks (>= num_records).  Slots that
    // hold zeros in EVERY tile carry RSRC_DEAD, out of range whatever the scalar: padding, the
    // left / right halo columns, slots past the band, surplus pieces -- and, with several whole frames per tile (tiles_y == 1), each frame's
    // halo rows, which in memory are the neighbouring frame's rows.  One offset set per pixel pitch (a concatenated input has two).
    constexpr int PP = NWV == 8 ? 7 : 8;                   // pieces per wave: npieces <= 56 (eight waves) / 32 (four)
    const int cs1 = a.C1, cs2 = a.x2 ? C - a.C1 : C;       // pixel pitch of x (the whole input when there is no x2) and of x2
    unsigned g_off1[PP], g_off2[PP];
#pragma unroll
    for (int u = 0; u < PP; ++u) {
        const int j = w + NWV * u, d = 64 * j + lane, pix = d / CT_SLOTS, c = d - CT_SLOTS * pix;
        const int f = idx_div(pix, a.inv_band), r = pix - f * (a.bh * BW), by = idx_div(r, a.inv_bw), bx = r - by * BW;
        // stacked: band row by is row rr of frame f0 + k in a layout of H + 1 rows per frame that starts at frame f0's row 1 - m0; rr = H is
        // the zero row two frames share; the band ends with the row below the tile where that lies in the same frame (rr != 0)
        const int uu = by - 1 + m0, k = idx_div(max(uu, 0), a.inv_h1), rr = uu - k * (H + 1), srow = s0 - m0 + k * H + rr;
        const bool srow_live = uu >= 0 && rr < H && (srow < s0 + a.th || (srow == s0 + a.th && rr != 0));
        // source pixel, from the group's first (unstacked: of a tile that starts at row 0)
        const int sp = ((stk ? srow : f * H + by - 1)) * W + bx - 1;
        const bool row_live = stk ? srow_live : a.tiles_y > 1 || (by >= 1 && by <= a.th);
        const bool live = j < a.npieces && c < 8 && pix < a.band_px && bx >= 1 && bx <= W && row_live;
        g_off1[u] = live ? (unsigned)(sp * cs1 * 2 + c * 16) : RSRC_DEAD;
        g_off2[u] = live ? (unsigned)(sp * cs2 * 2 + c * 16) : RSRC_DEAD;
        if constexpr (UP) {
            // x is never fetched into a band: g_off1 addresses the staging pieces instead.  Slot d = 8 spx + c of staged pixel
            // spx = (f nlr + lr) wl + lx <- lo pixel (f, lrow0 + lr, lx) of the frame group; lrow0 is the tile's scalar.  A row past the frame
            // reads the next frame's (never used: the taps clamp) or, past the group, zeros.
            const int spx = d >> 3, c8 = d & 7;
            const int sf = idx_div(spx, a.inv_slr), sr = spx - sf * (a.nlr * a.wl), lr = idx_div(sr, a.inv_wl), lx = sr - lr * a.wl;
            g_off1[u] = j < a.nstage && spx < a.stage_px ? (unsigned)((((sf * a.hl + lr) * a.wl + lx) * cs1 + c8 * 8) * 2) : RSRC_DEAD;
        }
    }
    const unsigned lds0 = (unsigned)reinterpret_cast<uintptr_t>(ct_band);
    const int nlive = max(0, (a.npieces - w + NWV - 1) / NWV);         // this wave's pieces u < nlive exist (j = w + NWV u < npieces)
    int nlive_up = 0, stage_off = 0;                                   // UP: likewise for the staging pieces
    if constexpr (UP) { nlive_up = max(0, (a.nstage - w + NWV - 1) / NWV); stage_off = a.stage_off; }
    // what a tile's band fetches need of the tile, computed ONCE per tile (scalar): the frame group's first pixel, its pixel count and the
    // tile's first row, in pixels -- the descriptor and the offset scalar of a chunk are a few scalar instructions from these
    struct Geo { int px0, npx, row0, r0, lr0, nfr; };     // (r0, lr0, nfr: UP only -- the tile's first row, its first staged source row, its frames)
    auto geo_of = [&](int tile) __attribute__((always_inline)) {
        const int ty = tile % tdiv, fg = tile / tdiv;                    // row tile (stacked: the phase), frame group
        Geo q;
        q.px0 = fg * fpg * H * W;
        q.npx = min(fpg, a.N - fg * fpg) * H * W;                       // (the frames that exist in the last group)
        q.row0 = stk ? 0 : ty * a.th * W;                               // (stacked: the phase's rows are in the lanes' offsets)
        q.r0 = q.lr0 = q.nfr = 0;
        if constexpr (UP) {
            // output row y >= 1 blends source rows (y - 1) >> 1 and the next one: the band's first row inside the frame is max(r0 - 1, 0)
            q.r0 = ty * a.th; q.lr0 = max((q.r0 - 2) >> 1, 0); q.nfr = min(a.fpt, a.N - fg * a.fpt);
        }
        return q;
    };
    auto fetch = [&](const Geo q, int chunk, int buf) __attribute__((always_inline)) {
        const bool second = a.x2 != nullptr && chunk * CT_CK >= a.C1;   // which tensor of a concatenated input holds this chunk
        const int cs = second ? cs2 : cs1;                              // its channel count = pixel pitch
        const bool up = UP && !second;                                  // a chunk of lo: a quarter of the pixels, into the staging area
        // wave-uniform values only (kernel arguments and scalars of the tile loop): the descriptor lives in SGPRs, no waterfall loop
        const bf16_t* base = (second ? a.x2 : a.x) + (long long)(up ? q.px0 >> 2 : q.px0) * cs;
        const __amdgpu_buffer_rsrc_t rsrc = make_rsrc(base, (up ? q.npx >> 2 : q.npx) * cs * 2);
        unsigned ts = (unsigned)((q.row0 * cs + chunk * CT_CK - (second ? a.C1 : 0)) * 2);
        unsigned dst0 = lds0 + buf * band_bytes + 1024 * w;             // LDS address of this wave's piece 0
        int nl = nlive;
        if constexpr (UP) {                                             // (selects, not a branch: a branch here put the offset sets in scratch)
            ts = up ? (unsigned)((q.lr0 * (W >> 1) * cs + chunk * CT_CK) * 2) : ts;
            dst0 = up ? lds0 + stage_off + 1024 * w : dst0;
            nl = up ? nlive_up : nlive;
        }
        // straight-line on purpose (always PP pieces: surplus ones land in a dump slot): the hand-written vmcnt counts of the chunk loop
        // assume exactly PP DMA operations per fetch
#pragma unroll
        for (int u = 0; u < PP; ++u) {
            const unsigned dst = u < nl ? dst0 + 1024 * NWV * u : lds0 + 2 * band_bytes;
            unsigned go;
            if constexpr (UP) go = g_off1[u] ^ ((g_off1[u] ^ g_off2[u]) & (second ? ~0u : 0u));    // (both sets read: a conditional read of one put them in scratch)
            else go = second ? g_off2[u] : g_off1[u];
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, lds_dma_dst(dst), 16, (int)(go + ts), 0, 0, 0);
        }
    };

    // the first band is requested before anything else is set up (it is the longest wait of the prologue: HBM); the bias loads above are
    // older than its pieces, so the first chunk's band wait covers them too
    int tile = blockIdx.x;
    Geo cur = geo_of(min(tile, a.ntiles - 1));
    if (tile < a.ntiles) fetch(cur, 0, 0);

    // this lane's pixel in each of the wave's pixel tiles: LDS byte offset of tap (0, 0), channel chunk g
    unsigned pbase[MTW];
#pragma unroll
    for (int m = 0; m < MTW; ++m) {
        const int p = poff + min(16 * (wm + MW * m) + li, tpix - 1);
        const int f = idx_div(p, inv_pper), r = p - f * pper, py = idx_div(r, a.inv_w), px = r - py * W;
        pbase[m] = (unsigned)(((f * rmul + py - rsub) * BW + px) * CT_PIX + g * 16);
    }
    const bf16_t* wrow[NTW];                               // weights [K][3][3][C]: A operand rows of output tile nt
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        const int kt = min(co0 / 16 + nt, K / 16 - 1);     // (a tile past K: the last tile's weights and bias, results never stored)
        // PK: the weights were re-laid out by gdkvm_conv3x3_pack_weights as [K / 16][k-step][lane][8], a fragment = 1 KiB contiguous
        // (8 full cache lines per load instruction instead of 16 half-used ones: the vector-memory path is this kernel's bound)
        if constexpr (PK) wrow[nt] = a.w + (size_t)kt * (9 * C * 16) + lane * 8;
        else wrow[nt] = a.w + (size_t)ct_channel(kt, li, a.perm) * 9 * C + 8 * g;
    }

    // k-steps of one tile: chunk-major, then tap, then channel half: ks = (chunk * 9 + tap) * 2 + kh
    const int nks = nchunk * 18;
    static_assert(NTW == 1 || NTW == 2, "wwait names the fragments of one or two output tiles");
    // Weight fragments are fetched and waited for by hand (asm loads the compiler does not count, s_waitcnt with counts written out
    // below): a wave that mixes LDS-DMA and register loads gets s_waitcnt vmcnt(0) from the compiler wherever it needs a loaded
    // register -- it cannot order the two kinds -- which put the whole L2 latency on every second k-step (3x the MFMA time).
    // The hardware returns them in issue order, so "at most N younger operations outstanding" is exact.
    struct WF { bf16x8 f[NTW]; };
    auto wload = [&](WF& o, int ks) __attribute__((always_inline)) {    // (wraps: a tile's last loads fetch the next tile's first k-steps)
        ks = ks >= nks ? ks - nks : ks;
        size_t off;
        if constexpr (PK) off = (size_t)ks * 512;
        else {
            const int chunk = ks / 18, r = ks - 18 * chunk, tap = r >> 1, kh = r & 1;
            off = (size_t)tap * C + chunk * CT_CK + 32 * kh;
        }
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(o.f[nt]) : "v"(wrow[nt] + off) : "memory");
    };
    // (the fragments are operands of the asm so that nothing that reads them can be scheduled above the wait)
    auto wwait = [&](WF& o, auto nc) __attribute__((always_inline)) {
        constexpr int N = decltype(nc)::value;
        if constexpr (NTW == 1) asm volatile("s_waitcnt vmcnt(%1)" : "+v"(o.f[0]) : "n"(N) : "memory");
        else asm volatile("s_waitcnt vmcnt(%2)" : "+v"(o.f[0]), "+v"(o.f[1]) : "n"(N) : "memory");
    };
    int gc = 0;                                             // gc: chunks processed so far; chunk gc lives in LDS buffer gc & 1
    // weight fragments, WD k-steps ahead, in a ring of WD register sets with STATIC indices: k-step r uses set r % WD and refills it
    // for k-step r + WD.  (Rotating named registers -- wf0 = wf1; ...; wf3 = load -- made the compiler copy the freshly loaded
    // fragment at the loop's back edge behind an s_waitcnt vmcnt(0): the whole L2 latency every second k-step, 3x the MFMA time.)
    constexpr int WD = 3, KU = 6;                           // 18 k-steps per chunk = 3 trips of KU; KU a multiple of WD and of 2
    WF wr[WD];
#pragma unroll
    for (int j = 0; j < WD; ++j) wload(wr[j], j);
    for (; tile < a.ntiles; tile += gridDim.x) {
        const Geo nxt = geo_of(min(tile + (int)gridDim.x, a.ntiles - 1));      // (past the last tile: one more band of the last tile, into the buffer nobody reads again)
        f32x4 acc[MTW][NTW];
#pragma unroll
        for (int m = 0; m < MTW; ++m)
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) acc[m][nt] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int chunk = 0; chunk < nchunk; ++chunk, ++gc) {
            const int buf = gc & 1;
            // this chunk's band (DMA issued a chunk ago) has landed once only the WD NTW weight loads of the last WD k-steps --
            // all younger than it -- are outstanding; past the barrier the other buffer is free.  (Not __syncthreads: its vmcnt(0)
            // would drain the weight fragments in flight.)
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(WD * NTW) : "memory");
            asm volatile("s_barrier" ::: "memory");
            if constexpr (UP) if (chunk * CT_CK < a.C1) {
                // An enlarged chunk: what has landed is the staging area.  All waves build band[buf] from it -- exactly what the DMA path would
                // have delivered from a materialised enlargement: zeros outside the frame (the halo ring, the rows above and below it, also
                // between the frames of a tile, and the frames a ragged last group lacks), the enlargement's clamped taps inside -- with LDS
                // reads, fp32 arithmetic and 16-byte LDS writes: no vector-memory operation, so the counts below stay exact.  band[buf] was
                // last read two chunks ago; the staging area is free for the next fetch behind the second barrier.
                // (The staging reads are asm, waited for by hand: the compiler answers an LDS read it knows of, behind LDS-DMA it cannot tell
                // apart, with s_waitcnt vmcnt(0) -- on the weight fragments in flight.)
                const unsigned stg = lds0 + stage_off;
                unsigned char* const bandw = ct_band + buf * band_bytes;
                // One item = the 2 x 2 output pixels that share four source taps (as in upsample_cat_bf16_2x_kernel), 8 channels: rows
                // 2 ip + 1, 2 ip + 2 and columns 2 jp + 1, 2 jp + 2, for jp = -1 .. wl - 1 (columns -1 .. W: the band's width) and the nrp row
                // pairs from ip0 on that cover the band's rows r0 - 1 .. r0 + th.  Four reads, 32 conversions and the horizontal blends serve
                // four output vectors.
                const int hl = H >> 1, wl = W >> 1, ncp = wl + 1, ip0 = (cur.r0 - 2) >> 1;
                const int nitems = a.fpt * a.nrp * ncp * 8;
#pragma unroll 1
                for (int i = tid; i < nitems; i += 64 * NWV) {
                    const int c8 = i & 7, t = i >> 3;
                    const int t2 = idx_div(t, a.inv_ncp), jp = t - t2 * ncp - 1, f = idx_div(t2, a.inv_nrp), ip = ip0 + t2 - f * a.nrp;
                    const int y0 = 2 * ip + 1, x0o = 2 * jp + 1;                            // the block's first output row / column
                    const int by0 = y0 - cur.r0 + 1;                                        // its first band row (the columns: bx = x + 1)
                    const bool vy[2] = {y0 >= 0 && y0 < H, y0 + 1 >= 0 && y0 + 1 < H}, vx[2] = {x0o >= 0, x0o + 1 < W};
                    u32x4 o[2][2] = {};
                    if ((vy[0] || vy[1]) && f < cur.nfr) {
                        const int ra = max(ip, 0) - cur.lr0, rb = min(ip + 1, hl - 1) - cur.lr0;
                        const int xa_ = max(jp, 0), xb_ = min(jp + 1, wl - 1);
                        const unsigned s0 = stg + (f * a.nlr + ra) * wl * 128 + c8 * 16, s1 = stg + (f * a.nlr + rb) * wl * 128 + c8 * 16;
                        u32x4 t00, t01, t10, t11;
                        asm volatile("ds_read_b128 %0, %1" : "=&v"(t00) : "v"(s0 + xa_ * 128) : "memory");
                        asm volatile("ds_read_b128 %0, %1" : "=&v"(t01) : "v"(s0 + xb_ * 128) : "memory");
                        asm volatile("ds_read_b128 %0, %1" : "=&v"(t10) : "v"(s1 + xa_ * 128) : "memory");
                        asm volatile("ds_read_b128 %0, %1" : "=&v"(t11) : "v"(s1 + xb_ * 128) : "memory");
                        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(t00), "+v"(t01), "+v"(t10), "+v"(t11) :: "memory");
                        // that kernel's row weights: fy = max(y / 2 - 1 / 4, 0): 1/4 on odd rows, 3/4 on even ones, 0 on row 0
                        const float ly[2] = {0.25f, y0 + 1 == 0 ? 0.f : 0.75f}, hy[2] = {0.75f, 1.f - ly[1]};
                        bilerp2x_bf16x8(t00, t01, t10, t11, hy, ly, o);
                    }
#pragma unroll
                    for (int ey = 0; ey < 2; ++ey) {
                        if (by0 + ey < 0 || by0 + ey >= a.bh) continue;                 // (a row pair may reach past the band)
                        const bool rowin = vy[ey] && f < cur.nfr;
#pragma unroll
                        for (int e = 0; e < 2; ++e) {
                            const u32x4 z = {0u, 0u, 0u, 0u};
                            *reinterpret_cast<u32x4*>(bandw + ((f * a.bh + by0 + ey) * BW + x0o + 1 + e) * CT_PIX + c8 * 16) = rowin && vx[e] ? o[ey][e] : z;
                        }
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                asm volatile("s_barrier" ::: "memory");
            }
            // the next band streams in behind this chunk's MFMAs: the tile's next chunk, or chunk 0 of the workgroup's next tile
            // (past the last tile: one more band of the last tile, into the buffer nobody reads again)
            {
                const bool more = chunk + 1 < nchunk;
                Geo q;                                     // (field by field: a select between the two structs would put them in scratch)
                q.px0 = more ? cur.px0 : nxt.px0; q.npx = more ? cur.npx : nxt.npx; q.row0 = more ? cur.row0 : nxt.row0;
                q.r0 = q.lr0 = q.nfr = 0;
                if constexpr (UP) q.lr0 = more ? cur.lr0 : nxt.lr0;
                fetch(q, more ? chunk + 1 : 0, buf ^ 1);
            }
            const unsigned char* band = ct_band + buf * band_bytes;
            auto load_x = [&](bf16x8 (&xb)[MTW], int r) __attribute__((always_inline)) {
                r = min(r, 17);                            // (past the chunk's last k-step: the same fragments again, branch-free)
                const int tap = r >> 1, kh = r & 1, dy = tap / 3, dx = tap - 3 * dy;
                const unsigned off = (unsigned)((dy * BW + dx) * CT_PIX + kh * 64);
#pragma unroll
                for (int m = 0; m < MTW; ++m) {
                    xb[m] = *reinterpret_cast<const bf16x8*>(band + pbase[m] + off);
                }
            };
            auto mfmas = [&](const bf16x8 (&xb)[MTW], const WF& wfr) __attribute__((always_inline)) {
#pragma unroll
                for (int m = 0; m < MTW; ++m)
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) {
                        acc[m][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wfr.f[nt], xb[m], acc[m][nt], 0, 0, 0);
                    }
            };
            const int ksb = chunk * 18;
            bf16x8 xa[MTW], xb[MTW];
            load_x(xa, 0);
            // KU k-steps per trip (not all 18: fully unrolled, the scheduler hoists the LDS reads of many k-steps and spills).
            // Younger than the fragments of k-step r at the time they are used: the loads of k-steps r+1, r+2 -- and, for the
            // first WD k-steps of a chunk, the PP band pieces issued above.
            auto trip = [&](int r0, auto firstc) __attribute__((always_inline)) {
                constexpr bool FIRST = decltype(firstc)::value;
                static_for<0, KU>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    wwait(wr[j % WD], std::integral_constant<int, (WD - 1) * NTW + (FIRST && j < WD ? PP : 0)>{});
                    if constexpr (j % 2 == 0) { load_x(xb, r0 + j + 1); mfmas(xa, wr[j % WD]); }
                    else { load_x(xa, r0 + j + 1); mfmas(xb, wr[j % WD]); }
                    wload(wr[j % WD], ksb + r0 + j + WD);
                    __builtin_amdgcn_sched_barrier(0);
                });
            };
            trip(0, std::true_type{});
#pragma unroll 1
            for (int r0 = KU; r0 < 18; r0 += KU) trip(r0, std::false_type{});
        }
        // epilogue: lane (li, g) holds rows 4g .. 4g+3 of each of the wave's output tiles for pixel 16 (wm + MW m) + li
        {
            const int fg = tile / tdiv, y0 = stk ? 0 : (tile - fg * tdiv) * a.th, n0 = fg * fpg;     // (stacked: frame and row come from the pixel)
            const float lo = a.relu ? 0.f : -INFINITY;
            if (NTW == 2 && a.perm) {                      // 8 consecutive channels 32G + 8g .. +7 (co0 and K are multiples of 32)
                if (co0 < K) {
                    // every pixel tile's output offset first, then ALL the residual loads, then the arithmetic: one wait for the seven
                    // loads (a load followed by its use per pixel tile was seven dependent round trips per epilogue)
                    unsigned o[MTW];                       // element offsets (the launcher keeps tensors below 2^31 elements); ~0u = no pixel
#pragma unroll
                    for (int m = 0; m < MTW; ++m) {
                        const int p = 16 * (wm + MW * m) + li;
                        const int pc = poff + min(p, tpix - 1);
                        const int f = idx_div(pc, inv_pper), r = pc - f * pper, py = idx_div(r, a.inv_w), px = r - py * W;
                        const int n = n0 + f, yy = y0 + py;
                        o[m] = p < tpix && n < a.N && yy < H ? (unsigned)(((n * H + yy) * W + px) * K + co0 + 8 * g) : ~0u;
                    }
                    // The epilogue's loads and stores are asm, invisible to the compiler's wait-count pass: while LDS-DMA (the next band) and the
                    // asm weight fragments are in flight it answers every use of a load it knows of -- and every rewrite of a register such a
                    // load or store touched -- with s_waitcnt vmcnt(0), i.e. with a wait for the operands just requested for the NEXT tile
                    // (round 4 stamps: 6 000 cycles per epilogue, a quarter of a tile's time, for ~1 500 cycles of work).  Without a residual
                    // nothing is waited for at all; with one, the loads go out in groups of four pixel tiles (all seven spill) and each group
                    // is waited for once (vmcnt(0): a count that relied on how many stores were issued would break when a pixel tile has no
                    // live lane and its store is branched over).
                    bf16_t* const yout = a.y;
                    const bf16_t* const resp = a.res;
                    const unsigned ofallback = (unsigned)(co0 + 8 * g);
                    auto finish = [&](auto resc) __attribute__((always_inline)) {
                        constexpr bool RES = decltype(resc)::value;
                        static_for<0, (MTW + 3) / 4>([&](auto bc) {
                            constexpr int M0 = 4 * decltype(bc)::value, M1 = M0 + 4 < MTW ? M0 + 4 : MTW;
                            u32x4 rr[4] = {};
                            if constexpr (RES) {
#pragma unroll
                                for (int m = M0; m < M1; ++m)
                                {
                                    const bf16_t* const rp = resp + (o[m] != ~0u ? o[m] : ofallback);
                                    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(rr[m - M0]) : "v"(rp) : "memory");
                                }
                                asm volatile("s_waitcnt vmcnt(0)" : "+v"(rr[0]), "+v"(rr[1]), "+v"(rr[2]), "+v"(rr[3]) :: "memory");
                            }
#pragma unroll
                            for (int m = M0; m < M1; ++m) {
                                f32x2 v[4];
#pragma unroll
                                for (int q = 0; q < 4; ++q)
                                    v[q] = f32x2{acc[m][q >> 1][2 * (q & 1)], acc[m][q >> 1][2 * (q & 1) + 1]} + f32x2{bias4[q >> 1][2 * (q & 1)], bias4[q >> 1][2 * (q & 1) + 1]};
                                if constexpr (RES) {
#pragma unroll
                                    for (int q = 0; q < 4; ++q) v[q] += unpack_bf16x2(rr[m - M0][q]);
                                }
                                u32x4 ow;
#pragma unroll
                                for (int q = 0; q < 4; ++q) {
                                    v[q] = __builtin_elementwise_max(v[q], f32x2{lo, lo});
                                    ow[q] = pack_bf16x2(v[q][0], v[q][1]);
                                }
                                // (s_nop: the hazard recogniser does not see an asm store's data registers being rewritten right behind it)
                                bf16_t* const yp = yout + o[m];
                                if (o[m] != ~0u) asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" :: "v"(yp), "v"(ow) : "memory");
                            }
                        });
                    };
                    if (a.res) finish(std::true_type{}); else finish(std::false_type{});
                }
            } else {
#pragma unroll
                for (int m = 0; m < MTW; ++m) {
                    const int p = 16 * (wm + MW * m) + li;
                    if (p >= tpix) continue;
                    const int pc = poff + p;
                    const int f = idx_div(pc, inv_pper), r = pc - f * pper, py = idx_div(r, a.inv_w), px = r - py * W;
                    const int n = n0 + f, yy = y0 + py;
                    if (n >= a.N || yy >= H) continue;
                    const size_t opix = (((size_t)n * H + yy) * W + px) * K;
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) {
                        if (co0 + 16 * nt >= K) continue;
                        const size_t o = opix + ct_channel(co0 / 16 + nt, 4 * g, a.perm);
                        f32x4 v = acc[m][nt] + bias4[nt];
                        if (a.res) v += unpack_bf16x4(*reinterpret_cast<const uint2*>(a.res + o));
                        v = __builtin_elementwise_max(v, f32x4{lo, lo, lo, lo});
                        *reinterpret_cast<uint2*>(a.y + o) = pack_bf16x4(v);
                    }
                }
            }
        }
        cur = nxt;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // nothing may land in LDS after the workgroup is gone
}

// Shapes this kernel serves: 3x3 / stride 1 / pad 1, C a multiple of 64, K a multiple of 16, and a map that tiles into <= 208
// pixels: whole frames of <= 208 pixels (several small frames per tile), or row bands of a wider frame.  Returns 0 when launched, 1
// when the shape is not covered (the caller falls back to the framework convolution + epilogue pass).
// weights [K][3][3][C] -> [K / 16][k-step = (chunk * 9 + tap) * 2 + kh][lane = 16 g + li][8]:  w[ct_channel(kt, li)][tap][64 chunk + 32 kh + 8 g ..]
__global__ __launch_bounds__(256) void conv3x3_pack_kernel(const uint4* w, uint4* packed, int K, int C)
{
    const int nks = C / CT_CK * 18;
    const size_t total = (size_t)(K / 16) * nks * 64;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int lane = (int)(i & 63), li = lane & 15, g = lane >> 4;
        const size_t f = i >> 6;
        const int ks = (int)(f % nks), kt = (int)(f / nks);
        const int chunk = ks / 18, r = ks - 18 * chunk, tap = r >> 1, kh = r & 1;
        packed[i] = w[(((size_t)ct_channel(kt, li, K % 32 == 0) * 9 + tap) * C + chunk * CT_CK + 32 * kh + 8 * g) / 8];
    }
}

// The pack of the DATA-GRADIENT convolution of the same layer, straight from the forward weights w [K][3][3][C]:
// dx = conv3x3(dy, w') with w'[c][ty][tx][k] = w[k][2 - ty][2 - tx][c]  (input channels K, output channels C), laid out as
// [C / 16][k-step = (chunk * 9 + tap) * 2 + kh][lane][8]:  w'[ct_channel(ct, li)][tap][64 chunk + 32 kh + 8 g + e]
__global__ __launch_bounds__(256) void conv3x3_pack_dgrad_kernel(const bf16_t* w, uint4* packed, int K, int C)
{
    const int nks = K / CT_CK * 18;
    const size_t total = (size_t)(C / 16) * nks * 64;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int lane = (int)(i & 63), li = lane & 15, g = lane >> 4;
        const size_t f = i >> 6;
        const int ks = (int)(f % nks), ct = (int)(f / nks);
        const int chunk = ks / 18, r = ks - 18 * chunk, tap = r >> 1, kh = r & 1;
        const int c = ct_channel(ct, li, C % 32 == 0), ftap = 8 - tap;                 // (2 - ty) * 3 + (2 - tx)
        const bf16_t* src = w + ((size_t)(chunk * CT_CK + 32 * kh + 8 * g) * 9 + ftap) * C + c;
        unsigned short e[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) e[j] = src[(size_t)j * 9 * C];
        packed[i] = make_uint4(e[0] | (unsigned)e[1] << 16, e[2] | (unsigned)e[3] << 16, e[4] | (unsigned)e[5] << 16, e[6] | (unsigned)e[7] << 16);
    }
}

}  // namespace

// ---- training: the forward pack AND the data-gradient pack of up to GDKVM_PACK_MAX_LAYERS layers in ONE launch, straight from the
// fp32 master weights.  Per layer and step the training step ran a cast to bf16 (a framework kernel), conv3x3_pack_kernel and, in the
// backward, conv3x3_pack_dgrad_kernel: 3 x 14 launches of ~5 us that move < 1 MB each (profiles/r04_n_train_cfg4_steady_state.csv:
// 0.19 ms of a 7.4 ms step).  Same bytes as those three: the fp32 -> bf16 conversion rounds to nearest even like the framework's cast.
struct PackTrainLayer { const float* w; uint4* fwd; uint4* dgrad; int K, C; long long sK, sC, sR, sS; };   // element strides of w[k][c][r][s]
struct PackTrainArgs { PackTrainLayer l[GDKVM_PACK_MAX_LAYERS]; };

namespace {
__global__ __launch_bounds__(256) void conv3x3_pack_train_kernel(PackTrainArgs a)
{
    const PackTrainLayer L = a.l[blockIdx.y];
    if (!L.w) return;
    const int K = L.K, C = L.C;
    const size_t nf = (size_t)(K / 16) * (C / CT_CK * 18) * 64, nd = (size_t)(C / 16) * (K / CT_CK * 18) * 64;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nf + nd; i += (size_t)gridDim.x * 256) {
        const bool fwd = i < nf;
        const size_t ii = fwd ? i : i - nf;
        const int lane = (int)(ii & 63), li = lane & 15, g = lane >> 4;
        const size_t f = ii >> 6;
        float e[8];
        if (fwd) {                                          // w[ct_channel(kt, li)][tap][64 chunk + 32 kh + 8 g ..]   (conv3x3_pack_kernel)
            const int nks = C / CT_CK * 18, ks = (int)(f % nks), kt = (int)(f / nks);
            const int chunk = ks / 18, r = ks - 18 * chunk, tap = r >> 1, kh = r & 1;
            const float* src = L.w + (long long)ct_channel(kt, li, K % 32 == 0) * L.sK + (long long)(tap / 3) * L.sR + (long long)(tap % 3) * L.sS
                               + (long long)(chunk * CT_CK + 32 * kh + 8 * g) * L.sC;
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = src[(long long)j * L.sC];
        } else {                                            // w'[c][tap][k] = w[k][8 - tap][c]   (conv3x3_pack_dgrad_kernel)
            const int nks = K / CT_CK * 18, ks = (int)(f % nks), ct = (int)(f / nks);
            const int chunk = ks / 18, r = ks - 18 * chunk, tap = r >> 1, kh = r & 1, ftap = 8 - tap;
            const float* src = L.w + (long long)ct_channel(ct, li, C % 32 == 0) * L.sC + (long long)(ftap / 3) * L.sR + (long long)(ftap % 3) * L.sS
                               + (long long)(chunk * CT_CK + 32 * kh + 8 * g) * L.sK;
#pragma unroll
            for (int j = 0; j < 8; ++j) e[j] = src[(long long)j * L.sK];
        }
        const uint4 o = pack_bf16x8(e);
        (fwd ? L.fwd : L.dgrad)[ii] = o;
    }
}
}  // namespace

extern "C" int gdkvm_conv3x3_pack_weights_train(int nlayers, const void* const* w, void* const* packed_fwd, void* const* packed_dgrad,
                                                const int* K, const int* C, const long long* strides, void* stream)
{
    if (nlayers < 0 || nlayers > GDKVM_PACK_MAX_LAYERS) return gdkvm_fail(GDKVM_ERR_SHAPE, "conv3x3_pack_weights_train: %d layers (at most %d per call)", nlayers, GDKVM_PACK_MAX_LAYERS);
    if (nlayers == 0) return GDKVM_OK;
    if (!w || !packed_fwd || !packed_dgrad || !K || !C || !strides) return gdkvm_fail(GDKVM_ERR_ARG, "conv3x3_pack_weights_train: null pointer");
    PackTrainArgs a{};
    for (int i = 0; i < nlayers; ++i) {
        if (K[i] <= 0 || C[i] <= 0 || K[i] % CT_CK || C[i] % CT_CK)
            return gdkvm_fail(GDKVM_ERR_SHAPE, "conv3x3_pack_weights_train: layer %d K=%d C=%d (multiples of 64)", i, K[i], C[i]);
        if (!w[i] || !packed_fwd[i] || !packed_dgrad[i] || !gdkvm_aligned16(packed_fwd[i]) || !gdkvm_aligned16(packed_dgrad[i]))
            return gdkvm_fail(GDKVM_ERR_ARG, "conv3x3_pack_weights_train: layer %d: null or unaligned pointer", i);
        a.l[i] = PackTrainLayer{static_cast<const float*>(w[i]), static_cast<uint4*>(packed_fwd[i]), static_cast<uint4*>(packed_dgrad[i]), K[i], C[i],
                                strides[4 * i], strides[4 * i + 1], strides[4 * i + 2], strides[4 * i + 3]};
    }
    if (int rc = gdkvm_check_device()) return rc;
    hipLaunchKernelGGL(conv3x3_pack_train_kernel, dim3(48, (unsigned)nlayers), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    GDKVM_LAUNCH_CHECK("conv3x3_pack_train_kernel");
    return GDKVM_OK;
}

extern "C" int gdkvm_conv3x3_pack_weights_dgrad(const void* w, void* packed, int K, int C, int io_dtype, void* stream)
{
    if (io_dtype != GDKVM_BF16) return gdkvm_fail(GDKVM_ERR_DTYPE, "conv3x3_pack_weights_dgrad: only bf16 is implemented");
    if (K <= 0 || C <= 0 || K % CT_CK || C % 16) return gdkvm_fail(GDKVM_ERR_SHAPE, "conv3x3_pack_weights_dgrad: K=%d C=%d (K a multiple of 64, C of 16)", K, C);
    if (!w || !packed || !gdkvm_aligned16(w) || !gdkvm_aligned16(packed)) return gdkvm_fail(GDKVM_ERR_ARG, "conv3x3_pack_weights_dgrad: null or unaligned pointer");
    if (int rc = gdkvm_check_device()) return rc;
    const size_t total = (size_t)(C / 16) * (K / CT_CK * 18) * 64;
    hipLaunchKernelGGL(conv3x3_pack_dgrad_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const bf16_t*>(w), static_cast<uint4*>(packed), K, C);
    GDKVM_LAUNCH_CHECK("conv3x3_pack_dgrad_kernel");
    return GDKVM_OK;
}

extern "C" int gdkvm_conv3x3_pack_weights(const void* w, void* packed, int K, int C, int io_dtype, void* stream)
{
    if (io_dtype != GDKVM_BF16) return gdkvm_fail(GDKVM_ERR_DTYPE, "conv3x3_pack_weights: only bf16 is implemented");
    if (K <= 0 || C <= 0 || K % 16 || C % CT_CK) return gdkvm_fail(GDKVM_ERR_SHAPE, "conv3x3_pack_weights: K=%d C=%d (K a multiple of 16, C of 64)", K, C);
    if (!w || !packed || !gdkvm_aligned16(w) || !gdkvm_aligned16(packed)) return gdkvm_fail(GDKVM_ERR_ARG, "conv3x3_pack_weights: null or unaligned pointer");
    if (int rc = gdkvm_check_device()) return rc;
    const size_t total = (size_t)(K / 16) * (C / CT_CK * 18) * 64;
    hipLaunchKernelGGL(conv3x3_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint4*>(w), static_cast<uint4*>(packed), K, C);
    GDKVM_LAUNCH_CHECK("conv3x3_pack_kernel");
    return GDKVM_OK;
}

namespace {
template <int NWN, int NTW, int NWV = 8, int MAXMT = CT_MAXMT>
void launch_tile(bool packed, dim3 grid, size_t lds, hipStream_t st, const ConvTileArgs& a)
{
    if (packed) hipLaunchKernelGGL((conv3x3_tile_kernel<NWN, NTW, true, NWV, MAXMT>), grid, dim3(64 * NWV), lds, st, a);
    else hipLaunchKernelGGL((conv3x3_tile_kernel<NWN, NTW, false, NWV, MAXMT>), grid, dim3(64 * NWV), lds, st, a);
}
template <int NWN, int NTW, int NWV = 8, int MAXMT = CT_MAXMT>
bool setattr_tile()
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_tile_kernel<NWN, NTW, true, NWV, MAXMT>), hipFuncAttributeMaxDynamicSharedMemorySize, 113 * 1024) == hipSuccess
        && hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_tile_kernel<NWN, NTW, false, NWV, MAXMT>), hipFuncAttributeMaxDynamicSharedMemorySize, 113 * 1024) == hipSuccess;
}
constexpr size_t CT_UP_LDS = 80 * 1024;                    // the UP forms keep two workgroups per CU (160 KB of LDS)
template <int NWN, int NTW>
bool setattr_up()
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_tile_kernel<NWN, NTW, true, 4, 7, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CT_UP_LDS) == hipSuccess;
}

// The tile and band geometry of a launch (a.N, a.H, a.W set): frames per tile, rows per tile, band size and DMA pieces, tile count.
// Returns false when the map does not tile into maxpix pixels under maxpieces pieces.
// Frame-stacked tiling of the four-wave forms (maxpix = 112 pixels, a multiple of the map's width): frames per group and tiles per group are
// the smallest with sg H W = stk maxpix, a tile is th = maxpix / W stacked rows (14 x 14: 4 frames, 7 tiles of 8 rows; 7 x 7: 16 frames, 7
// tiles of 16 rows).  The band holds th + 2 rows and one zero row per frame boundary inside the tile; bh is the tallest of the stk phases.
// A ragged last group ends with its last tile that has a row.  Returns false when a band does not fit the pieces.
bool stacked_geometry(ConvTileArgs& a, int maxpix, int maxpieces, int maxgrid)
{
    const int N = a.N, H = a.H, W = a.W, hw = H * W;
    int gcd = hw, b = maxpix;
    while (b) { const int t = gcd % b; gcd = b; b = t; }
    a.stk = hw / gcd; a.sg = maxpix / gcd;
    if (a.stk > maxgrid) return false;
    a.fpt = 1; a.tiles_y = 1; a.th = maxpix / W; a.bw = W + 2;
    int cross = 0;
    for (int ph = 0; ph < a.stk; ++ph) { const int s0 = ph * a.th, c = (s0 + a.th - 1) / H - s0 / H; if (c > cross) cross = c; }
    a.bh = a.th + 2 + cross;
    a.band_px = a.bh * a.bw;
    a.npieces = (a.band_px * CT_SLOTS + 63) / 64;
    if (a.npieces > maxpieces) return false;
    a.inv_band = 1.0f / (float)(a.bh * a.bw); a.inv_bw = 1.0f / (float)a.bw;
    a.inv_tw = 1.0f / (float)(a.th * W); a.inv_w = 1.0f / (float)W;
    a.inv_hw = 1.0f / (float)hw; a.inv_h1 = 1.0f / (float)(H + 1);
    const long long ntiles = (long long)(N / a.sg) * a.stk + ((long long)(N % a.sg) * H + a.th - 1) / a.th;
    if (ntiles <= 0 || ntiles > 0x7fffffffLL) return false;
    a.ntiles = (int)ntiles;
    return true;
}

bool tile_geometry(ConvTileArgs& a, int maxpix, int maxpieces)
{
    const int N = a.N, H = a.H, W = a.W;
    a.stk = 0; a.sg = 0; a.inv_hw = a.inv_h1 = 0.f;
    if (H * W <= maxpix) { a.th = H; a.fpt = maxpix / (H * W); a.tiles_y = 1; if (a.fpt > N) a.fpt = N; }
    else { a.fpt = 1; a.th = maxpix / W; if (a.th < 1) return false; a.tiles_y = (H + a.th - 1) / a.th; }
    a.bw = W + 2; a.bh = a.th + 2;
    // the halo band of a tile must fit the 56 DMA pieces (8 waves x 7) of a chunk: tiny maps take fewer frames, wide ones fewer rows
    auto pieces = [&]() { a.band_px = a.fpt * a.bh * a.bw; return (a.band_px * CT_SLOTS + 63) / 64; };
    while (pieces() > maxpieces && a.fpt > 1) --a.fpt;
    while (pieces() > maxpieces && a.th > 1) { --a.th; a.bh = a.th + 2; a.tiles_y = (H + a.th - 1) / a.th; }
    a.npieces = pieces();
    if (a.npieces > maxpieces) return false;
    a.inv_band = 1.0f / (float)(a.bh * a.bw); a.inv_bw = 1.0f / (float)a.bw;
    a.inv_tw = 1.0f / (float)(a.th * W); a.inv_w = 1.0f / (float)W;
    const long long groups = (N + a.fpt - 1) / a.fpt;
    const long long ntiles = groups * a.tiles_y;
    if (ntiles <= 0 || ntiles > 0x7fffffffLL) return false;
    a.ntiles = (int)ntiles;
    return true;
}
}  // namespace

// The UP form: the first C1 of the C input channels are the exact-2x enlargement of lo [N, H/2, W/2, C1], the rest x2 [N, H, W, C - C1];
// packed weights.  K % 128 == 0 runs <4, 2> on four waves, any other K (a multiple of 16) <2, 2> on four waves.  0 = launched.
int gdkvm_conv3x3_upcat_launch(const void* lo, const void* x2, int C1, const void* w, const float* bias, const void* residual, void* y,
                               int N, int C, int H, int W, int K, int relu, hipStream_t st)
{
    if (C % CT_CK || K % 16 || W > 64 || W < 2 || H < 2 || (H | W) & 1 || N < 1 || !x2 || C1 <= 0 || C1 >= C || C1 % CT_CK) return 1;
    ConvUpArgs a;
    a.x2 = static_cast<const bf16_t*>(x2); a.C1 = C1;
    a.x = static_cast<const bf16_t*>(lo); a.w = static_cast<const bf16_t*>(w); a.bias = bias;
    a.res = static_cast<const bf16_t*>(residual); a.y = static_cast<bf16_t*>(y);
    a.N = N; a.H = H; a.W = W; a.C = C; a.K = K; a.relu = relu;
    if (!tile_geometry(a, 16 * 7, 32)) return 1;
    if ((long long)(a.fpt * H + 2) * W * (C1 > C - C1 ? C1 : C - C1) * 2 >= 0x7fffffffLL) return 1;     // (as gdkvm_conv3x3_tile_launch)
    a.perm = K % 32 == 0;
    // staging: a band of bh rows blends at most bh / 2 + 2 source rows (rows (y - 1) >> 1 and the next, over bh consecutive y)
    a.hl = H / 2; a.wl = W / 2;
    a.nlr = a.bh / 2 + 2 < a.hl ? a.bh / 2 + 2 : a.hl;
    a.stage_px = a.fpt * a.nlr * a.wl;
    a.nstage = (a.stage_px + 7) / 8;
    if (a.nstage > 32) return 1;                           // (the pieces of one fetch: four waves x 8)
    a.inv_slr = 1.0f / (float)(a.nlr * a.wl); a.inv_wl = 1.0f / (float)a.wl;
    a.nrp = a.bh / 2 + 1; a.inv_ncp = 1.0f / (float)(a.wl + 1); a.inv_nrp = 1.0f / (float)a.nrp;
    a.stage_off = 2 * a.npieces * 1024 + 1024;
    const size_t lds = (size_t)a.stage_off + (size_t)a.nstage * 1024;
    if (lds > CT_UP_LDS) return 1;
    const int kwg = K % 128 == 0 ? 128 : 64;
    const int gy = (K + kwg - 1) / kwg;
    int per = 512 / gy; if (per < 1) per = 1;
    const int gx = a.ntiles < per ? a.ntiles : per;        // persistent: two workgroups per CU
    static std::atomic<unsigned long long> done_mask{0};   // per device; a lost race only repeats the idempotent call
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 1;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done_mask.load(std::memory_order_relaxed) & bit)) {
        if (!setattr_up<4, 2>() || !setattr_up<2, 2>()) return 1;
        done_mask.fetch_or(bit, std::memory_order_relaxed);
    }
    if (kwg == 128) hipLaunchKernelGGL((conv3x3_tile_kernel<4, 2, true, 4, 7, true>), dim3(gx, gy), dim3(256), lds, st, a);
    else hipLaunchKernelGGL((conv3x3_tile_kernel<2, 2, true, 4, 7, true>), dim3(gx, gy), dim3(256), lds, st, a);
    return 0;
}

int gdkvm_conv3x3_tile_launch(const void* x, const void* x2, int C1, const void* w, const float* bias, const void* residual, void* y,
                              int N, int C, int H, int W, int K, int relu, int variant, int packed, hipStream_t st)
{
    if (variant == 0 && K % 128 == 0 && CT_VARIANT_128 == 4) {
        // by shape: the two-workgroups-per-CU form where the tile's band fits its 32 DMA pieces, else the eight-wave form
        if (gdkvm_conv3x3_tile_launch(x, x2, C1, w, bias, residual, y, N, C, H, W, K, relu, 4, packed, st) == 0) return 0;
        variant = 2;
    }
    // (a half tile must still hold two rows of the map: on 64-pixel rows it would be ONE row under a three-row band -- at 256x256 inputs the
    //  192 -> 64 layer took 273 us that way and the forward 1.573 ms against 1.515 ms with the eight-wave form, same box, round 4)
    if (variant == 0 && K % 128 != 0 && (H * W <= 16 * 7 || 2 * W <= 16 * 7)) {
        if (gdkvm_conv3x3_tile_launch(x, x2, C1, w, bias, residual, y, N, C, H, W, K, relu, 5, packed, st) == 0) return 0;
        variant = 3;
    }
    if (C % CT_CK || K % 16 || W > 64 || W < 1 || H < 1 || N < 1 || variant < 0 || variant > 5) return 1;
    if (variant == 4 && K % 128) return 1;
    const bool half = variant == 4 || variant == 5;       // four waves, 112-pixel tiles, two workgroups per CU
    if (x2 && (C1 <= 0 || C1 >= C || C1 % CT_CK)) return 1;
    ConvTileArgs a;
    a.x2 = static_cast<const bf16_t*>(x2); a.C1 = x2 ? C1 : C;
    a.x = static_cast<const bf16_t*>(x); a.w = static_cast<const bf16_t*>(w); a.bias = bias;
    a.res = static_cast<const bf16_t*>(residual); a.y = static_cast<bf16_t*>(y);
    a.N = N; a.H = H; a.W = W; a.C = C; a.K = K; a.relu = relu;
    const int maxpix = half ? 16 * 7 : 16 * CT_MAXMT;
    const int maxpieces = half ? 32 : 56;
    // wave grid by output channels (variant 0; 1..4 pick one for tuning): 128 per workgroup where K allows, else 64
    if (variant == 0) variant = K % 128 == 0 ? 2 : CT_VARIANT_64;
    const int kwg = (variant == 2 || variant == 4) ? 128 : 64;   // output channels per workgroup
    const int gy = (K + kwg - 1) / kwg;
    int per = (half ? 512 : 256) / gy; if (per < 1) per = 1;     // workgroup slots per channel group
    // the four-wave forms stack frames where the map's rows tile 112 pixels but whole rows of ONE frame group leave padded pixel slots
    // (7 x 7: 98 of 112, 14 x 14: 196 of 224); a map that tiles exactly (28 x 28) or whose width does not divide 112 keeps the row tiles
    const bool padded = H * W <= maxpix ? maxpix % (H * W) != 0 : H % (maxpix / W) != 0;
    if (!(half && maxpix % W == 0 && padded && stacked_geometry(a, maxpix, maxpieces, per)) && !tile_geometry(a, maxpix, maxpieces)) return 1;
    // a band piece is addressed by a 32-bit byte offset from its frame group's first byte, and offsets from 2^31 on stand for "zeros":
    // a group, the band row below it included, stays below that
    if ((long long)((a.stk ? a.sg : a.fpt) * H + 2) * W * (x2 ? (C1 > C - C1 ? C1 : C - C1) : C) * 2 >= 0x7fffffffLL) return 1;
    a.perm = K % 32 == 0;
    const long long ntiles = a.ntiles;
    const size_t lds = (size_t)2 * a.npieces * 1024 + 1024;
    if (a.stk) per -= per % a.stk;                         // stacked: a workgroup's tiles, gridDim.x apart, share one phase
    const int gx = (int)(ntiles < per ? ntiles : per);     // persistent: one workgroup per CU
    static std::atomic<unsigned long long> done_mask{0};   // per device; a lost race only repeats the idempotent call
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 1;
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done_mask.load(std::memory_order_relaxed) & bit)) {
        if (!setattr_tile<4, 1>() || !setattr_tile<4, 2>() || !setattr_tile<2, 2>() || !setattr_tile<4, 2, 4, 7>() || !setattr_tile<2, 2, 4, 7>()) return 1;
        done_mask.fetch_or(bit, std::memory_order_relaxed);
    }
    switch (variant) {
        case 1: launch_tile<4, 1>(packed, dim3(gx, gy), lds, st, a); break;
        case 2: launch_tile<4, 2>(packed, dim3(gx, gy), lds, st, a); break;
        case 4: launch_tile<4, 2, 4, 7>(packed, dim3(gx, gy), lds, st, a); break;
        case 5: launch_tile<2, 2, 4, 7>(packed, dim3(gx, gy), lds, st, a); break;      // 64 channels per workgroup: 2 channel groups x 2 pixel-tile groups
        default: launch_tile<2, 2>(packed, dim3(gx, gy), lds, st, a); break;
    }
    return 0;
}
