// temporal_vote.hip -- smooth a clip's label masks over time: every pixel takes the class most frames of its window t - r .. t + r have (the
// first clean-up in front of lv_measure, ahead of largest_component.hip and fill_holes.hip, and the first kernel here that walks T).
// include/gdkvm.h holds the definition; out, info and counts are exact integers that depend on neither the schedule nor the path taken.
//
// A workgroup is ONE wave and owns a run of pixel positions of one clip, lane l the 4 VW positions from 4 VW (64 run + l), and walks the
// clip's frames in order.  VW = 4 (a lane holds 16 pixels as one uint4, a run is 1024 positions) when that alone gives the launch
// TV_NARROW_BELOW work items; below that VW = 1 (one 32-bit word per lane, a run is 256 positions): the walk along T is serial and the
// kernel's arithmetic -- some 200 instructions per word and frame -- is what it costs, so a cfg2 batch (16 clips of 112 x 112: 208 runs of
// 1024, on a chip with 1024 SIMDs) wants its words spread over four times as many waves.  Measured with either form forced, clips of 32
// frames of 112 x 112, 4 classes, with a target, us per call, VW = 1 / VW = 4: 16 clips 40 / 75, 40 clips 53 / 78, 79 clips 76 / 110,
// 160 clips (2080 items of 1024) 138 / 147, 320 clips (4160) 271 / 232, 640 clips 494 / 455 -- the wide form's fewer wave sums win once
// the SIMDs are full; the threshold sits between the two middle rows.  Work items (clip, run) beyond TV_MAX_WG workgroups are taken in a
// grid-stride loop, in either form.
//
// The lane's state is the per-class vote count of each of its pixels over the current window, one BYTE per pixel (a window has at most 15
// frames): NC classes x VW words, NC a template argument so that every index is a compile-time one.  A frame that enters the window adds
// its per-byte matches (0x01 where the byte equals the class), a frame that leaves subtracts them; bytes >= ncls match no class and invalid
// positions are read as 0xff.  The winner is computed byte-parallel on keys 2 votes + (class == own label), at most 31: the largest key, the
// smallest class among equal keys -- so the own label wins a tie it is part of and the smallest class one it is not.
//
// How every byte crosses HBM once: a position's byte of frame t is loaded three times, all by the SAME lane -- when the frame enters the
// window (step t - r - 1, the first touch: from HBM), as the centre (step t) and when it leaves (step t + r) -- and a lane's working set is
// the 2r + 2 <= 16 vectors in between, at most 256 bytes, 16 KiB per wave: the second and third load are hits in the cache the first one
// filled (re-loading instead of a register ring keeps one kernel for every radius and no runtime-indexed register array).  Nothing but that
// lane reads those bytes, a wave's 256 or 1024 bytes of a frame share a cache line with no other wave in the vector form, and every out byte
// is stored once.  The target is read once.  Steps go in blocks of K = 8 (VW = 4: 2): every load of block i + 1 is issued before block i is
// computed, so a wave waits for memory once per block.
//
// The vector form (16- or 4-byte loads and stores) needs H W % 16 == 0 and 16-byte aligned mask, out and target: the cfg2 mask of 112 x 112.
// Every other case assembles the same words from byte loads below the frame's end and stores bytes: correct at any address, not fast.
//
// changed, flips_in, flips_out and the 3 ncls Dice counts of a step are summed per wave, two 16-bit (VW = 1: three 10-bit) fields to a word
// -- a wave's 1024 (256) pixels fit --, and parked in LDS; every TV_FLUSH frames and at the clip's end the 64 lanes add the non-zero ones
// into info / counts, one (frame, sum) per lane and turn (lane 0's atomics in every step kept the step's loads waiting behind them: the cfg2
// batch measured 86 us that way with loads one step ahead, 40 us parked and in blocks).  The launcher zeroed info and counts with a kernel
// (gdkvm_zero_async: a memset node of a captured graph ran once, README round 6).  Integer adds commute: bit-reproducible.
// The wave's sum is tv_wave_total below, not mask_frame.hpp's wave_sum: with ONE wave per workgroup and a step that depends on the step
// before, the six dependent LDS-crossbar shuffles of each of wave_sum's butterflies are latency nothing hides (the cfg2 batch measured 146 us
// with a target and 73 us without, i.e. with two sums per step instead of eight); four DPP adds and four lane reads are plain ALU work.

#include "mask_frame.hpp"

namespace {

constexpr int TV_LANES = 64;                                   // one wave per workgroup
constexpr int TV_RUN = GDKVM_TEMPORAL_VOTE_RUN;                // pixel positions per work item with 16 per lane (gdkvm.h) ...
constexpr int TV_NARROW_RUN = GDKVM_TEMPORAL_VOTE_NARROW_RUN;  // ... and with 4 per lane, taken while the wide form has fewer than
constexpr int TV_NARROW_BELOW = GDKVM_TEMPORAL_VOTE_NARROW_BELOW;      // ... this many work items
constexpr int TV_MAX_WG = GDKVM_TEMPORAL_VOTE_MAX_WG;          // workgroups per launch; more items than that are walked grid-stride
static_assert(TV_RUN == TV_LANES * 16 && TV_NARROW_RUN == TV_LANES * 4, "a lane owns 16 or 4 positions");
constexpr int TV_FLUSH = 32;                                   // frames whose sums a wave parks in LDS before it adds them to info / counts

struct TvArgs {
    const uint8_t* mask; const uint8_t* target; uint8_t* out; int32_t* info; int32_t* counts;
    long long items;
    int nrun, T, HW, radius;
};

// 0x80 -> 0xff per byte
__device__ __forceinline__ unsigned tv_bytes(unsigned m80) { return m80 | (m80 - (m80 >> 7)); }

// The sum of v over the 64 lanes of a (full) wave, the same in every lane: quad, quad pair, half row, row by DPP, then one lane of each of
// the four rows of 16
__device__ __forceinline__ unsigned tv_wave_total(unsigned v)
{
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xb1, 0xf, 0xf, false);      // quad_perm [1,0,3,2]
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4e, 0xf, 0xf, false);      // quad_perm [2,3,0,1]
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xf, 0xf, false);     // row_half_mirror
    v += (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xf, 0xf, false);     // row_mirror
    return (unsigned)(__builtin_amdgcn_readlane((int)v, 0) + __builtin_amdgcn_readlane((int)v, 16) + __builtin_amdgcn_readlane((int)v, 32) +
                      __builtin_amdgcn_readlane((int)v, 48));
}

template <int VW>
struct TvVec { unsigned w[VW]; };

// The lane's 4 VW bytes at p; n of them lie inside the frame (0: the frame does not exist or the lane is past the frame's end), the others
// read 0xff
template <int VW, bool VEC>
__device__ __forceinline__ TvVec<VW> tv_load(const uint8_t* p, int n)
{
    TvVec<VW> v;
#pragma unroll
    for (int w = 0; w < VW; ++w) v.w[w] = 0xffffffffu;
    if (n > 0) {
        if constexpr (VEC && VW == 4) {
            const uint4 r = *reinterpret_cast<const uint4*>(p);
            v.w[0] = r.x; v.w[1] = r.y; v.w[2] = r.z; v.w[3] = r.w;
        } else if constexpr (VEC) {
            static_assert(VW == 1, "one word or four");
            v.w[0] = *reinterpret_cast<const unsigned*>(p);
        } else {
#pragma unroll
            for (int e = 0; e < 4 * VW; ++e)
                if (e < n) v.w[e >> 2] = (v.w[e >> 2] & ~(0xffu << (8 * (e & 3)))) | ((unsigned)p[e] << (8 * (e & 3)));
        }
    }
    return v;
}
template <int VW, bool VEC>
__device__ __forceinline__ void tv_store(uint8_t* p, int n, const TvVec<VW>& v)
{
    if (n <= 0) return;
    if constexpr (VEC && VW == 4) {
        *reinterpret_cast<uint4*>(p) = make_uint4(v.w[0], v.w[1], v.w[2], v.w[3]);
    } else if constexpr (VEC) {
        *reinterpret_cast<unsigned*>(p) = v.w[0];
    } else {
#pragma unroll
        for (int e = 0; e < 4 * VW; ++e)
            if (e < n) p[e] = (uint8_t)(v.w[e >> 2] >> (8 * (e & 3)));
    }
}

template <int NC, int VW, bool VEC>
__global__ __launch_bounds__(TV_LANES) void temporal_vote_kernel(TvArgs a)
{
    // a step's sums, PER of them to a word in fields of FB bits: a lane adds at most 4 VW to a field, the wave at most 256 VW
    constexpr int NV = 3 + 3 * NC, PER = VW == 1 ? 3 : 2, FB = VW == 1 ? 10 : 16, NP = (NV + PER - 1) / PER;
    static_assert(256 * VW < (1 << FB), "a field holds the wave's sum");
    constexpr int K = VW == 1 ? 8 : 2;                     // steps per block: 4 K VW registers hold the next block's loads
    static_assert(TV_FLUSH % K == 0, "a flush falls on a block's end");
    __shared__ unsigned s_sum[TV_FLUSH * NP];
    using Vec = TvVec<VW>;
    const int lane = threadIdx.x, T = a.T, HW = a.HW, r = a.radius;
    const bool dice = a.target != nullptr;
    for (long long item = blockIdx.x; item < a.items; item += gridDim.x) {
        const long long clip = item / a.nrun;
        const int run = (int)(item - clip * a.nrun);
        const int p0 = (run * TV_LANES + lane) * 4 * VW;   // (< 2^20 + 2^10)
        const int n = p0 >= HW ? 0 : (HW - p0 < 4 * VW ? HW - p0 : 4 * VW);
        const size_t f0 = (size_t)clip * (size_t)T;        // the clip's first frame
        const uint8_t* mp = a.mask + f0 * (size_t)HW + p0;
        const uint8_t* tp = dice ? a.target + f0 * (size_t)HW + p0 : nullptr;
        uint8_t* op = a.out + f0 * (size_t)HW + p0;
        // frame t of the clip as this lane sees it; a frame outside 0 .. T - 1 reads as 0xff, which votes for nothing
        auto frame = [&](int t) { return tv_load<VW, VEC>(mp + (size_t)(t < 0 ? 0 : t) * (size_t)HW, (t >= 0 && t < T) ? n : 0); };
        auto truth = [&](int t) { return tv_load<VW, VEC>(dice ? tp + (size_t)t * (size_t)HW : nullptr, (dice && t < T) ? n : 0); };

        unsigned cnt[NC][VW];
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int w = 0; w < VW; ++w) cnt[c][w] = 0;
        auto vote = [&](const Vec& v, bool enter) {
#pragma unroll
            for (int c = 0; c < NC; ++c)
#pragma unroll
                for (int w = 0; w < VW; ++w) {
                    const unsigned e1 = eq80(v.w[w], (unsigned)c) >> 7;
                    cnt[c][w] = enter ? cnt[c][w] + e1 : cnt[c][w] - e1;
                }
        };
        // the window of frame 0: frames 0 .. min(r, T - 1)
        for (int t = 0; t <= r && t < T; ++t) vote(frame(t), true);

        // Steps go in blocks of K: the 4 K loads of block i + 1 -- centres, targets, what enters and what leaves -- are issued before block i
        // is computed, so the wave waits for memory once per block, not once per step (its loads, stores and atomics share one counter here).
        struct Block { Vec own[K], tgt[K], ent[K], lev[K]; };
        auto fetch = [&](Block& b, int t0) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int t = t0 + k;                      // (t0 < T <= 2^30)
                const bool in = t < T;
                b.own[k] = frame(in ? t : -1);
                b.tgt[k] = truth(t);
                b.ent[k] = frame(in && t <= T - 2 - r ? t + 1 + r : -1);
                b.lev[k] = frame(in ? t - r : -1);
            }
        };
        Block cur;
        fetch(cur, 0);
        Vec prev_own = cur.own[0], prev_out = cur.own[0];
        int flushed = 0;                                   // the frames below this have their sums in info / counts
        for (int t0 = 0; t0 < T; t0 += K) {
            Block nxt;
            fetch(nxt, t0 + K);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int t = t0 + k;
                if (t >= T) break;                         // (uniform)
                const Vec& own = cur.own[k];
                Vec out;
                int v[NP * PER];
#pragma unroll
                for (int i = 0; i < NP * PER; ++i) v[i] = 0;
#pragma unroll
                for (int w = 0; w < VW; ++w) {
                    const unsigned o = own.w[w];
                    unsigned valid = 0, best = 0, arg = 0;
#pragma unroll
                    for (int c = 0; c < NC; ++c) {
                        const unsigned e80 = eq80(o, (unsigned)c);
                        valid |= e80;
                        const unsigned key = (cnt[c][w] << 1) + (e80 >> 7);
                        if (c == 0) {
                            best = key;
                        } else {
                            const unsigned m = tv_bytes(gt80(key, best));     // strictly more: the smallest class keeps an equal key
                            best = (key & m) | (best & ~m);
                            arg = (((unsigned)c * BYTES_ONE) & m) | (arg & ~m);
                        }
                    }
                    const unsigned vm = tv_bytes(valid);
                    const unsigned res = (arg & vm) | (o & ~vm);              // a byte >= ncls passes through
                    out.w[w] = res;
                    v[0] += __builtin_popcount(ne80(res, o));
                    v[1] += __builtin_popcount(ne80(o, prev_own.w[w]));
                    v[2] += __builtin_popcount(ne80(res, prev_out.w[w]));
                    if (dice) {
                        const unsigned g = cur.tgt[k].w[w];
#pragma unroll
                        for (int c = 0; c < NC; ++c) {
                            const unsigned eo = eq80(res, (unsigned)c), et = eq80(g, (unsigned)c);
                            v[3 + 3 * c + 0] += __builtin_popcount(eo & et);
                            v[3 + 3 * c + 1] += __builtin_popcount(eo);
                            v[3 + 3 * c + 2] += __builtin_popcount(et);
                        }
                    }
                }
                if (t == 0) v[1] = v[2] = 0;               // (prev_* are the frame itself there; spelled out all the same)
                tv_store<VW, VEC>(op + (size_t)t * (size_t)HW, n, out);

                // the wave's sums of this step (without a target only the word with the three info sums), parked in LDS
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    unsigned pk = 0;
#pragma unroll
                    for (int h = 0; h < PER; ++h) pk |= (unsigned)v[PER * j + h] << (FB * h);
                    const unsigned sj = (dice || PER * j < 3) ? tv_wave_total(pk) : 0u;      // (uniform)
                    if (lane == 0) s_sum[(t - flushed) * NP + j] = sj;
                }

                vote(cur.ent[k], true);
                vote(cur.lev[k], false);
                prev_own = own; prev_out = out;
            }
            // every TV_FLUSH frames and at the clip's end the 64 lanes add the parked sums that are not zero: one (frame, sum) each per turn
            const int done = t0 + K < T ? t0 + K : T;
            if (done - flushed >= TV_FLUSH || done == T) {
                __syncthreads();                           // (one wave: lane 0's LDS writes are ordered before every lane's reads)
                const int nk = dice ? NV : 3;
                for (int i = lane; i < (done - flushed) * nk; i += TV_LANES) {
                    const int st = i / nk, k = i - st * nk;
                    const int x = (int)((s_sum[st * NP + k / PER] >> (FB * (k % PER))) & ((1u << FB) - 1u));
                    const size_t f = f0 + (size_t)(flushed + st);
                    if (x) {
                        if (k < 3) atomicAdd(a.info + f * 4 + k, x);
                        else atomicAdd(a.counts + f * (size_t)(3 * NC) + (k - 3), x);
                    }
                }
                __syncthreads();                           // (... and those reads before lane 0 parks the next sums)
                flushed = done;
            }
            cur = nxt;
        }
    }
}

template <int NC>
void tv_launch(bool wide, bool vec, unsigned grid, hipStream_t st, const TvArgs& a)
{
    if (wide) {
        if (vec) hipLaunchKernelGGL((temporal_vote_kernel<NC, 4, true>), dim3(grid), dim3(TV_LANES), 0, st, a);
        else hipLaunchKernelGGL((temporal_vote_kernel<NC, 4, false>), dim3(grid), dim3(TV_LANES), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((temporal_vote_kernel<NC, 1, true>), dim3(grid), dim3(TV_LANES), 0, st, a);
        else hipLaunchKernelGGL((temporal_vote_kernel<NC, 1, false>), dim3(grid), dim3(TV_LANES), 0, st, a);
    }
}

inline bool tv_shape_ok(int clips, int T, int H, int W, int ncls)
{
    return mask_shape_ok(clips, H, W) && T >= 1 && ncls >= 2 && ncls <= 8;
}

}  // namespace

// The kernel keeps its state in registers and adds its sums into the zeroed outputs: no workspace for any shape.
extern "C" size_t gdkvm_temporal_vote_workspace_bytes(int clips, int T, int H, int W, int ncls)
{
    (void)clips; (void)T; (void)H; (void)W; (void)ncls;
    return 0;
}

extern "C" int gdkvm_temporal_vote(const uint8_t* mask, const uint8_t* target, uint8_t* out, int32_t* info, int32_t* counts,
                                   void* workspace, size_t workspace_bytes, int clips, int T, int H, int W, int ncls, int radius, void* stream)
{
    if (!tv_shape_ok(clips, T, H, W, ncls))
        return gdkvm_fail(GDKVM_ERR_SHAPE, "temporal_vote: bad shape clips=%d T=%d H=%d W=%d ncls=%d (T >= 1, H, W in 1..1024, ncls in 2..8)", clips,
                          T, H, W, ncls);
    if (radius < 0 || radius > 7) return gdkvm_fail(GDKVM_ERR_SHAPE, "temporal_vote: radius=%d outside 0..7", radius);
    if (clips == 0) return GDKVM_OK;
    if (!mask || !out || !info) return gdkvm_fail(GDKVM_ERR_SHAPE, "temporal_vote: null pointer (mask, out and info are required)");
    if (target && !counts) return gdkvm_fail(GDKVM_ERR_SHAPE, "temporal_vote: counts required with a target");
    if (int rc = mask_check_aligned16("temporal_vote", GDKVM_ERR_SHAPE, "info and counts", {info, target ? counts : nullptr})) return rc;
    const size_t frames = (size_t)clips * (size_t)T, HW = (size_t)H * (size_t)W, total = frames * HW;
    if (frames > ((size_t)1 << 30)) return gdkvm_fail(GDKVM_ERR_SHAPE, "temporal_vote: clips * T = %zu frames exceed 2^30", frames);
    if (out < mask + total && mask < out + total)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "temporal_vote: out must not overlap mask (later frames read earlier input)");
    const size_t need = gdkvm_temporal_vote_workspace_bytes(clips, T, H, W, ncls);
    if (int rc = mask_check_workspace("temporal_vote", H, W, need, workspace, workspace_bytes)) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = gdkvm_zero_async(info, frames * 4 * sizeof(int32_t), st)) return rc;
    if (target)
        if (int rc = gdkvm_zero_async(counts, frames * (size_t)ncls * 3 * sizeof(int32_t), st)) return rc;
    const bool wide = (long long)clips * (long long)((HW + TV_RUN - 1) / TV_RUN) >= TV_NARROW_BELOW;
    const int nrun = (int)((HW + (wide ? TV_RUN : TV_NARROW_RUN) - 1) / (wide ? TV_RUN : TV_NARROW_RUN));
    const long long items = (long long)clips * nrun;
    const unsigned grid = (unsigned)(items < TV_MAX_WG ? items : TV_MAX_WG);
    const bool vec = HW % 16 == 0 && gdkvm_aligned16(mask) && gdkvm_aligned16(out) && (!target || gdkvm_aligned16(target));
    TvArgs a{mask, target, out, info, counts, items, nrun, T, (int)HW, radius};
    switch (ncls) {
        case 2: tv_launch<2>(wide, vec, grid, st, a); break;
        case 3: tv_launch<3>(wide, vec, grid, st, a); break;
        case 4: tv_launch<4>(wide, vec, grid, st, a); break;
        case 5: tv_launch<5>(wide, vec, grid, st, a); break;
        case 6: tv_launch<6>(wide, vec, grid, st, a); break;
        case 7: tv_launch<7>(wide, vec, grid, st, a); break;
        default: tv_launch<8>(wide, vec, grid, st, a);
    }
    GDKVM_LAUNCH_CHECK("temporal_vote_kernel");
    return GDKVM_OK;
}
