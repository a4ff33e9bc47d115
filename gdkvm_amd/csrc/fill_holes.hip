// fill_holes.hip -- fill the holes of one class of label masks on the device (the second clean-up in front of lv_measure, behind
// largest_component.hip: pixels inside the cavity that argmax gave to another class cost the method of disks about twice their pixel share).
// include/gdkvm.h holds the definition; the filled mask and the eight integers depend on neither the algorithm nor the schedule.
//
// ONE workgroup per frame (512 lanes in the LDS form -- 60 KiB of labels allow two workgroups per CU whatever their size, and on 512 frames
// of 112 x 112 the kernel measured 128 us with 256 lanes, 90 us with 512 and 123 us with 1024, of which 784 have a vector; 1024 in the
// workspace form, whose chains of dependent L2 loads want more waves in flight): no cross-workgroup synchronisation, no fences between
// workgroups, no flag anybody spins on.  The set that is labelled is the COMPLEMENT Q of the class (MaskFrame::sweep_not_*), typically
// 85-90 % of a frame.  The labelling itself -- one 32-bit word per pixel, in LDS up to LABEL_LDS_PIX pixels (the 112 x 112 mask of cfg2 takes
// 49 KiB) and otherwise in the frame's slice of the caller's workspace -- is mask_labels.hpp's, shared with largest_component.hip.  Passes, a
// workgroup barrier between them:
//   1. n = |P|, hit_before and n_target.  P empty, P the whole frame, H <= 2 or W <= 2: no hole is possible, straight to the copy.
//   2-5. mask_labels.hpp, on Q: clear, horizontal runs, union-find over the backward neighbours, flatten.  A spiral corridor costs no
//      sweeps: there is no sweep.
//   6. mask_labels.hpp: L[root] += 1 per pixel and L[root] |= OUT for a pixel on the frame's border.  The count (bits 0..20, at most 2^20)
//      never reaches the flags.
//   7. the roots without OUT are the holes: their number, the largest, and FILL into the word of each that max_area lets through.
//   8. mask_labels.hpp's rewrite: a pixel of Q becomes cls when its root's word has FILL; what the filled pixels were in the target.
// Loop bounds: mask_labels.hpp gives the termination argument of the union-find (both loops count to H*W and raise the frame's failure flag
// rather than spin: holes = -1 and out = mask).  Every other loop walks the lane's share of the H*W pixels once, or the at most 16 bits of
// a match word.

#include "mask_labels.hpp"

namespace {

// what a root's word carries beside LABEL_ROOT and the count
constexpr unsigned FH_OUT = 0x40000000u;       // pass 6: the component holds a pixel of the frame's border
constexpr unsigned FH_FILL = 0x20000000u;      // pass 7: a hole that is filled
constexpr unsigned FH_SIZE = 0x001fffffu;

struct FhArgs {
    const uint8_t* mask; const uint8_t* target; uint8_t* out; int32_t* info; unsigned* ws;
    int HW, W, H, stride, cls, conn, max_area;
};

template <bool LDS, int NT>
__global__ __launch_bounds__(NT) void fill_holes_kernel(FhArgs a)
{
    constexpr int NW = NT / 64;
    __shared__ int s_cnt[NW][3], s_hole[NW][4], s_hit[NW][1], s_fail;
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, HW = a.HW, W = a.W, H = a.H;
    const size_t f = blockIdx.x;
    const unsigned cls = (unsigned)a.cls;
    const uint8_t* tgt = a.target ? a.target + f * (size_t)HW : nullptr;
    int32_t* info = a.info + f * 8;
    const MaskFrame<NT> fr(a.mask + f * (size_t)HW, HW, W, cls);
    const Labels<LDS> L = frame_labels<LDS>(a.ws, f, a.stride);
    if (tid == 0) s_fail = 0;

    // pass 1: n, and against the target what P hits and how many pixels of the class it has
    int n, hit_before, n_target;
    {
        int c = 0, hb = 0, nt = 0;
        fr.sweep_bits([&](unsigned m, int p0) {
            c += __builtin_popcount(m);
            if (tgt) visit_p(m, p0, [&](int p) { hb += tgt[p] == cls ? 1 : 0; });
        });
        if (tgt) {
            const MaskFrame<NT> ft(tgt, HW, W, cls);
            ft.sweep_bits([&](unsigned m, int) { nt += __builtin_popcount(m); });
        }
        c = wave_sum(c);
        hb = wave_sum(hb);
        nt = wave_sum(nt);
        if (lane == 0) { s_cnt[wv][0] = c; s_cnt[wv][1] = hb; s_cnt[wv][2] = nt; }
        __syncthreads();
        n = wg_sum(s_cnt, 0);
        hit_before = wg_sum(s_cnt, 1);
        n_target = wg_sum(s_cnt, 2);
    }

    int holes = 0, holes_filled = 0, filled = 0, largest = 0;
    if (n > 0 && n < HW && H > 2 && W > 2) {               // (uniform; otherwise every pixel of Q touches the border)
        label_components<true>(fr, L, a.stride, HW, a.conn == 8, s_fail);
        label_sizes<true, FH_OUT>(fr, L, [&](int x, int y) { return x == 0 || x == W - 1 || y == 0 || y == H - 1; });
        __syncthreads();

        // pass 7: the holes.  A root is met by the one lane that owns its pixel, which alone writes FILL into it
        {
            int c = 0, cf = 0, px = 0, big = 0;
            const bool bad = s_fail != 0;
            fr.sweep_not_p([&](int p) {
                const unsigned v = L.ld((unsigned)p);
                if ((v & LABEL_ROOT) && !(v & FH_OUT)) {
                    const int size = (int)(v & FH_SIZE);
                    ++c;
                    big = size > big ? size : big;
                    if (!bad && (a.max_area == 0 || size <= a.max_area)) {
                        ++cf;
                        px += size;
                        L.st((unsigned)p, v | FH_FILL);
                    }
                }
            });
            c = wave_sum(c);
            cf = wave_sum(cf);
            px = wave_sum(px);
            big = wave_max(big);
            if (lane == 0) { s_hole[wv][0] = c; s_hole[wv][1] = cf; s_hole[wv][2] = px; s_hole[wv][3] = big; }
            __syncthreads();
            holes = wg_sum(s_hole, 0);
            holes_filled = wg_sum(s_hole, 1);
            filled = wg_sum(s_hole, 2);
#pragma unroll
            for (int w = 0; w < NW; ++w) largest = s_hole[w][3] > largest ? s_hole[w][3] : largest;
        }
        if (s_fail) { holes = -1; holes_filled = filled = largest = 0; }
    }

    // pass 8: out, and what the filled pixels were in the target
    int hf = 0;
    rewrite_frame<true>(fr, a.out + f * (size_t)HW, HW, holes_filled > 0, cls, [&](int p) -> bool {       // p is of Q: is it filled?
        if (!(L.root_word((unsigned)p) & FH_FILL)) return false;
        if (tgt) hf += tgt[p] == cls ? 1 : 0;
        return true;
    });
    hf = wave_sum(hf);
    if (lane == 0) s_hit[wv][0] = hf;
    __syncthreads();
    if (tid < 8) {
        int v = 0;
        if (tid == 0) v = holes;
        else if (tid == 1) v = holes_filled;
        else if (tid == 2) v = n;
        else if (tid == 3) v = filled;
        else if (tid == 4) v = largest;
        else if (tid == 5) v = hit_before;
        else if (tid == 6) v = wg_sum(s_hit, 0);
        else v = n_target;
        info[tid] = v;
    }
}

}  // namespace

extern "C" size_t gdkvm_fill_holes_workspace_bytes(int frames, int H, int W) { return label_workspace_bytes(frames, H, W); }

extern "C" int gdkvm_fill_holes(const uint8_t* mask, const uint8_t* target, uint8_t* out, int32_t* info, void* workspace, size_t workspace_bytes,
                                int frames, int H, int W, int cls, int connectivity, int max_area, void* stream)
{
    if (int rc = mask_check_shape("fill_holes", frames, H, W)) return rc;
    if (int rc = mask_check_cls("fill_holes", GDKVM_ERR_SHAPE, cls)) return rc;
    if (int rc = mask_check_connectivity("fill_holes", connectivity)) return rc;
    if (max_area < 0) return gdkvm_fail(GDKVM_ERR_SHAPE, "fill_holes: max_area=%d must be >= 0 (0 = holes of any size)", max_area);
    if (frames == 0) return GDKVM_OK;
    if (int rc = mask_check_in_out("fill_holes", mask, out, info, (size_t)frames * (size_t)H * (size_t)W)) return rc;
    const size_t need = label_workspace_bytes(frames, H, W);
    if (int rc = mask_check_workspace("fill_holes", H, W, need, workspace, workspace_bytes)) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    FhArgs a{mask, target, out, info, static_cast<unsigned*>(workspace), H * W, W, H, (int)label_stride(H, W), cls, connectivity, max_area};
    if (!need) hipLaunchKernelGGL((fill_holes_kernel<true, 512>), dim3((unsigned)frames), dim3(512), 0, st, a);
    else hipLaunchKernelGGL((fill_holes_kernel<false, 1024>), dim3((unsigned)frames), dim3(1024), 0, st, a);
    GDKVM_LAUNCH_CHECK("fill_holes_kernel");
    return GDKVM_OK;
}
