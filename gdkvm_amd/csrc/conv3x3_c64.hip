// conv3x3_c64.hip -- hand-written 3x3 / stride 1 / pad 1 convolution for the 64 -> 64 channel layers at stride 4 (five of the
// twenty convolutions of a forward, 21 % of its time), NHWC bf16, with bias (+ residual) (+ ReLU) in the epilogue.
//
// Why not the implicit-GEMM library kernel: as a GEMM this layer is M = N*H*W pixels x K = 576 with only 64 output channels, so
// the "A matrix" (every input pixel repeated for its nine taps) is 9x the input -- 462 MB through L2 and the vector-memory path
// per call for a 51 MB tensor -- and the library kernels sit at ~62 us = 20 % of the MFMA rate whichever tile is chosen
// (round-1 sweep).  Here the nine taps are nine SHIFTED READS of one LDS image:
//   * a workgroup owns a 4 x TW pixel tile; its (4+2) x (TW+2) input halo band (64 channels = 128 B per pixel) is staged in LDS
//     once, pixels 160 B apart (128 B of channels + 32 B of padding: a ds_read_b128 of 16 consecutive pixels is then
//     conflict-free in every one of the instruction's four 16-lane groups, and every operand address is base + immediate);
//   * the weights never touch LDS: wave (wm, wn) keeps the 32 output channels 32wn.. as MFMA A-operand fragments for all 18
//     k-steps (tap x channel half) in 144 registers for the lifetime of the (persistent) workgroup;
//   * per k-step a wave reads one 16-pixel B fragment per m-tile (4 reads) and issues 8 v_mfma_f32_16x16x32_bf16; with the
//     weights as the A operand a lane ends with 4 consecutive output channels of one pixel -> 8-byte stores;
//   * the next tile's band streams into the other LDS buffer by LDS-DMA (global_load_lds, no registers: the 144 weight
//     registers leave none to stage through) while the current tile computes.  With one tile per row of the map (tiles_x == 1:
//     every map of the model) the DMA goes through a buffer descriptor over the tile's frame: its range check zero-fills the
//     rows above and below the frame, and the padding slots and the left / right halo columns (the DMA writes lane-linear, so
//     they are fetched too) carry an offset that is always out of range.  Wider maps keep per-lane pointers and fetch those
//     slots from a 16-byte zero constant.
// HBM traffic: input once (+ halo rows from L2), output once.  Arithmetic: fp32 accumulation over the same 576 products as the
// library kernel, one rounding after the epilogue.
#include "gdkvm_device.hpp"

namespace {

constexpr int CV_C = 64;                 // input = output channels
constexpr int CV_TH = 4;                 // tile rows
constexpr int CV_PIX = 160;              // bytes between LDS pixels: 8 data chunks + 2 padding chunks of 16 B

__device__ const uint4 g_conv_zero16 = {0, 0, 0, 0};          // source of the zero padding

struct Conv64Args {
    const bf16_t* x; const bf16_t* w; const float* bias; const bf16_t* res; bf16_t* y;
    int N, H, W, tiles_x, tiles_y, relu;
    int packed;                          // w is the gdkvm_conv3x3_pack_weights copy: fragment (kt, ks) = 1 KiB contiguous, rows in this kernel's channel order
};

// DESC: one tile per row (tiles_x == 1), band fetched through a buffer descriptor; else per-lane pointers, any tiles_x
template <int TW, bool DESC>
__global__ __launch_bounds__(256, 2) void conv3x3_c64_kernel(Conv64Args a)
{
    constexpr int BW = TW + 2, NPIX = CV_TH * TW, BAND_PIX = (CV_TH + 2) * BW;
    constexpr int SLOTS = BAND_PIX * 10, NPIECES = (SLOTS + 63) / 64, BAND_BYTES = NPIECES * 1024;
    __shared__ __attribute__((aligned(16))) unsigned char band2[2 * BAND_BYTES];
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6), wm = w >> 1, wn = w & 1;
    const int ntiles = a.N * a.tiles_y * a.tiles_x;

    // band fetch by LDS-DMA: piece j = w + 4u (64 consecutive 16-byte LDS slots) is issued by wave w; slot d = 10 pix + c holds
    // channel chunk c of band pixel pix (c = 8, 9: padding).  The slot geometry does not depend on the tile: kept in registers.
    // DESC: g_rel is the slot's BYTE offset from the frame's first byte for the tile at row 0 (band row 0 is row -1: negative, huge as
    // unsigned); a tile adds its first row as a scalar.  The descriptor spans exactly the frame, so the rows above and below it read as
    // zeros; the slots that are zero in every tile -- padding, the halo columns, past the band -- carry RSRC_DEAD, out of range with any
    // such scalar added.
    constexpr int PP = (NPIECES + 3) / 4;
    int g_rel[PP], g_yx[DESC ? 1 : PP];                    // !DESC: element offset from the band's (0, 0) pixel; (by << 8 | bx), -1 = no data
#pragma unroll
    for (int u = 0; u < PP; ++u) {
        const int j = w + 4 * u, d = 64 * j + lane, pix = d / 10, c = d - 10 * pix;
        const int by = pix / BW, bx = pix - by * BW;
        if constexpr (DESC) {
            const bool live = j < NPIECES && c < 8 && pix < BAND_PIX && bx >= 1 && bx <= a.W;
            g_rel[u] = live ? (((by - 1) * a.W + bx - 1) * CV_C + c * 8) * 2 : (int)RSRC_DEAD;
        } else {
            g_rel[u] = (by * a.W + bx) * CV_C + c * 8;
            bool live = j < NPIECES && c < 8 && pix < BAND_PIX;
            if (a.tiles_x == 1) live = live && bx >= 1 && bx <= a.W;     // one tile per row: the column test does not depend on the tile
            g_yx[u] = live ? (by << 8 | bx) : -1;
        }
    }
    // DESC: a tile is (frame n, row tile ty); the workgroup's tiles are gridDim.x apart, so the pair advances by a fixed step with one
    // carry (the split of the tile index by two run-time divisions was ~60 scalar instructions per tile, twice)
    struct TilePos { int n, ty; };
    const int step_n = DESC ? (int)gridDim.x / a.tiles_y : 0, step_ty = DESC ? (int)gridDim.x % a.tiles_y : 0;
    auto advance = [&](TilePos& p) __attribute__((always_inline)) {
        if constexpr (DESC) {
            p.n += step_n; p.ty += step_ty;
            if (p.ty >= a.tiles_y) { p.ty -= a.tiles_y; ++p.n; }
        }
    };
    auto fetch = [&](int tile, TilePos pos, int buf) __attribute__((always_inline)) {
        unsigned char* const bands = static_cast<unsigned char*>(band2);       // (a plain pointer type for lds_dma_dst: see its comment)
        if constexpr (DESC) {
            // wave-uniform values only: the descriptor lives in SGPRs, no waterfall loop
            const __amdgpu_buffer_rsrc_t rsrc = make_rsrc(a.x + (long long)pos.n * a.H * a.W * CV_C, a.H * a.W * CV_C * 2);
            const unsigned ts = (unsigned)(pos.ty * CV_TH * a.W * CV_C * 2);
#pragma unroll
            for (int u = 0; u < PP; ++u) {
                const int j = w + 4 * u;
                if (j >= NPIECES) break;                   // (wave-uniform)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, lds_dma_dst(bands + buf * BAND_BYTES + 1024 * j), 16, (int)((unsigned)g_rel[u] + ts), 0, 0, 0);
            }
        } else {
            const int tx = tile % a.tiles_x, t2 = tile / a.tiles_x, ty = t2 % a.tiles_y, n = t2 / a.tiles_y;
            const int y0 = ty * CV_TH - 1, x0 = tx * TW - 1;
            const bf16_t* origin = a.x + (((long long)n * a.H + y0) * a.W + x0) * CV_C;
            const bool one_col = a.tiles_x == 1;
#pragma unroll
            for (int u = 0; u < PP; ++u) {
                const int j = w + 4 * u;
                if (j >= NPIECES) break;                   // (wave-uniform)
                const int yy = y0 + (g_yx[u] >> 8), xx = x0 + (g_yx[u] & 255);
                const bool ok = g_yx[u] >= 0 && (unsigned)yy < (unsigned)a.H && (one_col || (unsigned)xx < (unsigned)a.W);
                const bf16_t* src = ok ? origin + g_rel[u] : reinterpret_cast<const bf16_t*>(&g_conv_zero16);
                __builtin_amdgcn_global_load_lds(src, lds_dma_dst(bands + buf * BAND_BYTES + 1024 * j), 16, 0, 0);
            }
        }
    };

    // this lane's pixel in each of the wave's m-tiles: LDS byte offset of tap (0, 0), channel chunk g
    unsigned pbase[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int p = min(16 * (4 * wm + m) + li, NPIX - 1);
        const int ty = p / TW, tx = p - ty * TW;
        pbase[m] = (unsigned)((ty * BW + tx) * CV_PIX + g * 16);
    }
    // DESC: the same pixel's BYTE offset in the output (and the residual) from the first byte of the frame for the tile at row 0, channels
    // 32wn + 8g ..; pixels the tile does not have carry RSRC_DEAD.  Output and residual go through descriptors over the tile's frame like the
    // band, so a row past the frame is out of range: its residual reads as zeros and its store is dropped -- every m-tile issues exactly one
    // load and one store whatever its pixels, which is what makes the epilogue's wait counts exact.
    unsigned o_rel[DESC ? 4 : 1];
    if constexpr (DESC) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int p = 16 * (4 * wm + m) + li, py = p / TW, px = p - py * TW;
            o_rel[m] = (p < NPIX && px < a.W) ? (unsigned)(((py * a.W + px) * CV_C + 32 * wn + 8 * g) * 2) : RSRC_DEAD;
        }
    }

    // Per tile: MFMAs from buffer `cur`, with no wait on memory (the weights were completed before the loop) | barrier + vmcnt(0):
    // outstanding then are the other buffer's band, requested a whole MFMA phase ago, and the previous epilogue's stores, older still
    // | this tile's epilogue: (descriptor form) the residual vectors requested together and consumed under counted waits that leave
    // the younger loads and the stores outstanding | DMA of the tile after next into `cur`.  Neither the stores nor the DMA are
    // waited for before the next barrier.  The per-lane pointer form keeps the compiler's epilogue (a vmcnt(0) behind each residual
    // load, which also covers the previous m-tile's store).
    int tile = blockIdx.x, cur = 0;
    TilePos tpos{DESC ? tile / a.tiles_y : 0, DESC ? tile % a.tiles_y : 0}, fpos = tpos;      // (DESC) this tile; the next tile to fetch
    if (tile < ntiles) fetch(tile, fpos, 0);               // (the first band is on its way while the weights load)
    advance(fpos);

    // weights of this wave's 32 output channels, all 18 k-steps, as A-operand fragments.  Which channel an MFMA row stands for is
    // free: row rho = 4 g' + r of n-tile nt is channel 32wn + 8g' + 4nt + r, so that a lane's two accumulator tiles hold EIGHT
    // consecutive channels of its pixel (one 16-byte store / residual load instead of two 8-byte ones).
    // (packed weights -- conv3x3_tile.hip's ct_channel order is this one -- make each of the 36 loads one contiguous KiB: the
    // prologue was a quarter of the kernel's time with 16 half-used cache lines per load)
    bf16x8 wf[2][18];
    if (a.packed) {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int ks = 0; ks < 18; ++ks)
                wf[nt][ks] = *reinterpret_cast<const bf16x8*>(a.w + ((size_t)((2 * wn + nt) * 18 + ks) * 64 + lane) * 8);
    } else {
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int ks = 0; ks < 18; ++ks) {
                const int tap = ks >> 1, kh = ks & 1, co = 32 * wn + 8 * (li >> 2) + 4 * nt + (li & 3);
                wf[nt][ks] = *reinterpret_cast<const bf16x8*>(a.w + ((size_t)co * 9 + tap) * CV_C + 32 * kh + 8 * g);
            }
    }
    float bia[2][4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(a.bias + 32 * wn + 8 * g + 4 * nt);
        bia[nt][0] = b4[0]; bia[nt][1] = b4[1]; bia[nt][2] = b4[2]; bia[nt][3] = b4[3];
    }
    // The weights and the bias are complete HERE, once: as operands of an (empty) asm statement they have to be in their registers in
    // front of it, so the compiler's one wait for them stands here and no pending load of theirs is carried into the tile loop.  Left
    // to its own placement it waited at their first uses, inside the loop's MFMA phase (vmcnt(29), then 11 down to 2): right on the
    // first tile, and on every later tile a wait for most of the band requested an epilogue earlier, which has until the barrier.
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
        asm volatile("" : "+v"(wf[nt][0]), "+v"(wf[nt][1]), "+v"(wf[nt][2]), "+v"(wf[nt][3]), "+v"(wf[nt][4]), "+v"(wf[nt][5]), "+v"(wf[nt][6]), "+v"(wf[nt][7]),
                          "+v"(wf[nt][8]), "+v"(wf[nt][9]), "+v"(wf[nt][10]), "+v"(wf[nt][11]), "+v"(wf[nt][12]), "+v"(wf[nt][13]), "+v"(wf[nt][14]),
                          "+v"(wf[nt][15]), "+v"(wf[nt][16]), "+v"(wf[nt][17]));
    asm volatile("" : "+v"(bia[0][0]), "+v"(bia[0][1]), "+v"(bia[0][2]), "+v"(bia[0][3]), "+v"(bia[1][0]), "+v"(bia[1][1]), "+v"(bia[1][2]), "+v"(bia[1][3]));

    __syncthreads();                                       // (vmcnt(0) + barrier: the first band has landed)
    if (tile + (int)gridDim.x < ntiles) fetch(tile + gridDim.x, fpos, 1);
    advance(fpos);
    for (; tile < ntiles; tile += gridDim.x, cur ^= 1) {
        const unsigned char* band = band2 + cur * BAND_BYTES;

        f32x4 acc[4][2];
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[m][0] = acc[m][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        // NM = m-tiles of this wave that hold pixels (wave wm = 1 of a 4 x 28 tile has three): no MFMA is spent on padding
        auto compute = [&](auto nm_c) __attribute__((always_inline)) {
            constexpr int NM = decltype(nm_c)::value;
            auto load_x = [&](bf16x8 (&xb)[4], int ks) __attribute__((always_inline)) {
                const int tap = ks >> 1, kh = ks & 1, dy = tap / 3, dx = tap - 3 * dy;
#pragma unroll
                for (int m = 0; m < NM; ++m)
                    xb[m] = *reinterpret_cast<const bf16x8*>(band + pbase[m] + (dy * BW + dx) * CV_PIX + kh * 64);
            };
            auto mfmas = [&](const bf16x8 (&xb)[4], int ks) __attribute__((always_inline)) {
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    acc[m][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[0][ks], xb[m], acc[m][0], 0, 0, 0);
                    acc[m][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[1][ks], xb[m], acc[m][1], 0, 0, 0);
                }
            };
            bf16x8 xa[4], xb[4];
            load_x(xa, 0);
#pragma unroll
            for (int ks = 0; ks < 18; ks += 2) {           // operands one k-step ahead of the MFMAs that use them
                load_x(xb, ks + 1);
                mfmas(xa, ks);
                __builtin_amdgcn_sched_barrier(0);
                if (ks + 2 < 18) load_x(xa, ks + 2);
                mfmas(xb, ks + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        constexpr int NMT = (NPIX + 15) / 16, NM1 = NMT - 4;            // m-tiles in all, and those of the wm = 1 waves
        if (wm == 0 || NM1 == 4) compute(std::integral_constant<int, (NMT < 4 ? NMT : 4)>{});
        else if constexpr (NM1 > 0 && NM1 < 4) compute(std::integral_constant<int, (NM1 > 0 ? NM1 : 1)>{});

        __syncthreads();                                   // everyone is done with this band; the next one has landed

        // epilogue: lane (li, g) holds channels 32wn + 8g .. +7 of pixel 16(4wm+m) + li (tile nt: the four channels 4nt ..)
        if constexpr (DESC) {
            // The residual vectors of ALL the wave's m-tiles are requested together, right behind the barrier, and consumed one by one
            // under a counted wait.  The loads are asm, so the compiler neither counts them nor answers their uses with vmcnt(0) (which
            // covered the previous m-tile's store: four serial chains of load round trip + store acknowledgement per tile); operations
            // retire from the counter in issue order, and behind residual m stand the NM - 1 - m younger loads and the m stores of the
            // m-tiles before it: NM - 1 younger operations for every m, none of which is waited for.
            const long long fo = (long long)tpos.n * a.H * a.W * CV_C;
            const unsigned fbytes = (unsigned)(a.H * a.W * CV_C * 2), ts = (unsigned)(tpos.ty * CV_TH * a.W * CV_C * 2);
            advance(tpos);
            const __amdgpu_buffer_rsrc_t yrs = make_rsrc(a.y + fo, (int)fbytes);
            const unsigned long long ra = reinterpret_cast<unsigned long long>(a.res + fo);
            const u32x4 rrs = {(unsigned)ra, (unsigned)(ra >> 32) & 0xffffu, fbytes, (unsigned)RSRC_WORD3};
            auto epilogue = [&](auto nm_c) __attribute__((always_inline)) {
                constexpr int NM = decltype(nm_c)::value;
                unsigned vo[NM];
                u32x4 rr[NM];
#pragma unroll
                for (int m = 0; m < NM; ++m) vo[m] = o_rel[m] + ts;
                if (a.res) {
#pragma unroll
                    for (int m = 0; m < NM; ++m) asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=&v"(rr[m]) : "v"(vo[m]), "s"(rrs) : "memory");
                }
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    f32x2 v[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        v[q] = f32x2{acc[m][q >> 1][2 * (q & 1)], acc[m][q >> 1][2 * (q & 1) + 1]} + f32x2{bia[q >> 1][2 * (q & 1)], bia[q >> 1][2 * (q & 1) + 1]};
                    if (a.res) {
                        asm volatile("s_waitcnt vmcnt(%1)" : "+v"(rr[m]) : "n"(NM - 1) : "memory");
                        const unsigned rw[4] = {rr[m][0], rr[m][1], rr[m][2], rr[m][3]};
#pragma unroll
                        for (int q = 0; q < 4; ++q) v[q] += unpack_bf16x2(rw[q]);
                    }
                    const float lo = a.relu ? 0.f : -INFINITY;
                    u32x4 ow;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        v[q] = __builtin_elementwise_max(v[q], f32x2{lo, lo});
                        ow[q] = pack_bf16x2(v[q][0], v[q][1]);
                    }
                    __builtin_amdgcn_raw_buffer_store_b128(ow, yrs, (int)vo[m], 0, 0);
                }
            };
            if (wm == 0 || NM1 == 4) epilogue(std::integral_constant<int, (NMT < 4 ? NMT : 4)>{});
            else if constexpr (NM1 > 0 && NM1 < 4) epilogue(std::integral_constant<int, (NM1 > 0 ? NM1 : 1)>{});
        } else {
        const int t2 = tile / a.tiles_x, tx = tile % a.tiles_x, ty = t2 % a.tiles_y, n = t2 / a.tiles_y;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int p = 16 * (4 * wm + m) + li;
            const int py = p / TW, px = p - py * TW, yy = ty * CV_TH + py, xx = tx * TW + px;
            if (p >= NPIX || yy >= a.H || xx >= a.W) continue;
            const size_t o = (((size_t)n * a.H + yy) * a.W + xx) * CV_C + 32 * wn + 8 * g;
            f32x2 v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                v[q] = f32x2{acc[m][q >> 1][2 * (q & 1)], acc[m][q >> 1][2 * (q & 1) + 1]} + f32x2{bia[q >> 1][2 * (q & 1)], bia[q >> 1][2 * (q & 1) + 1]};
            if (a.res) {
                const uint4 rr = *reinterpret_cast<const uint4*>(a.res + o);
                const unsigned rw[4] = {rr.x, rr.y, rr.z, rr.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] += unpack_bf16x2(rw[q]);
            }
            const float lo = a.relu ? 0.f : -INFINITY;
            unsigned ow[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                v[q] = __builtin_elementwise_max(v[q], f32x2{lo, lo});
                ow[q] = pack_bf16x2(v[q][0], v[q][1]);
            }
            *reinterpret_cast<uint4*>(a.y + o) = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        }
        }
        // the band of the tile after next, into the buffer just consumed.  Issued BEHIND the epilogue, where it has a whole tile of MFMAs
        // to land: in front of it the residual waits would cover it (the counter retires in issue order), in the pointer form as
        // vmcnt(0) (+9 us per residual layer, round 5), in the descriptor form unless the counts allowed for the wave's 7 or 8 pieces
        // (not built: DESIGN.md section 6, "After round 6: prefetch waits").
        if (tile + 2 * (int)gridDim.x < ntiles) fetch(tile + 2 * gridDim.x, fpos, cur);
        advance(fpos);
    }
}

}  // namespace

// internal entry used by gdkvm_conv_bias_act (conv_dispatch.hip): returns 0 on launch
int gdkvm_conv3x3_c64_launch(const void* x, const void* w, const float* bias, const void* residual, void* y, int N, int H, int W,
                             int relu, int packed, hipStream_t st)
{
    Conv64Args a;
    a.packed = packed;
    a.x = static_cast<const bf16_t*>(x); a.w = static_cast<const bf16_t*>(w); a.bias = bias;
    a.res = static_cast<const bf16_t*>(residual); a.y = static_cast<bf16_t*>(y);
    a.N = N; a.H = H; a.W = W; a.relu = relu;
    // tile width: 28 for rows that are a multiple of 28 pixels (EchoNet's stride-4 map), 16 for narrow maps, else 32 (ragged edge masked)
    const int TW = W % 28 == 0 ? 28 : (W <= 16 ? 16 : 32);
    a.tiles_x = (W + TW - 1) / TW;
    a.tiles_y = (H + CV_TH - 1) / CV_TH;
    const long long ntiles = (long long)N * a.tiles_x * a.tiles_y;
    if (ntiles <= 0 || ntiles > 0x7fffffffLL) return 1;
    const int grid = (int)(ntiles < 512 ? ntiles : 512);   // persistent: two workgroups per CU, weights loaded once each
    // one tile per row, and a frame (with the band rows below it) below 2^31 bytes -- offsets from there on stand for "zeros" --:
    // the band goes through a buffer descriptor; else the per-lane pointer form
    const bool desc = a.tiles_x == 1 && (long long)(H + CV_TH + 2) * W * CV_C * 2 < 0x7fffffffLL;
    if (desc) {
        if (TW == 28) hipLaunchKernelGGL((conv3x3_c64_kernel<28, true>), dim3(grid), dim3(256), 0, st, a);
        else if (TW == 16) hipLaunchKernelGGL((conv3x3_c64_kernel<16, true>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv3x3_c64_kernel<32, true>), dim3(grid), dim3(256), 0, st, a);
    } else {
        if (TW == 28) hipLaunchKernelGGL((conv3x3_c64_kernel<28, false>), dim3(grid), dim3(256), 0, st, a);
        else if (TW == 16) hipLaunchKernelGGL((conv3x3_c64_kernel<16, false>), dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((conv3x3_c64_kernel<32, false>), dim3(grid), dim3(256), 0, st, a);
    }
    return 0;
}
