// largest_component.hip -- keep the largest connected component of one class of label masks on the device (the clean-up in front of
// lv_measure: a false-positive island far from the ventricle otherwise enters the long axis and the disks).  include/gdkvm.h holds the
// definition; labels, sizes and the filtered mask are integers that depend on neither the algorithm nor the schedule.
//
// ONE workgroup per frame (256 lanes in the LDS form; 1024 in the workspace form, whose chains of dependent L2 loads want more waves in
// flight): no cross-workgroup synchronisation, no fences between workgroups, no flag anybody spins on.  The labelling itself -- one 32-bit
// word per pixel, in LDS up to LABEL_LDS_PIX pixels (the 112 x 112 mask of cfg2 takes 49 KiB) and otherwise in the frame's slice of the
// caller's workspace -- is mask_labels.hpp's, shared with fill_holes.hip.  Passes, a workgroup barrier between them:
//   1. n = |P|; an empty frame goes straight to the copy.
//   2-5. mask_labels.hpp, on the pixels of the class: clear, horizontal runs, union-find over the backward neighbours, flatten.
//   6. mask_labels.hpp: sizes, L[root] += 1 per pixel.
//   7. components, and the kept one by a two-key maximum (size, then the smaller label).
//   8. mask_labels.hpp's rewrite: a pixel of the class whose label is not the kept one becomes fill; the hit counts of the removed pixels.
// Loop bounds: mask_labels.hpp gives the termination argument of the union-find (both loops count to H*W and raise the frame's failure flag
// rather than spin: components = -1 and out = mask).  Every other loop walks the lane's share of the H*W pixels once.

#include "mask_labels.hpp"

namespace {

typedef unsigned long long u64;

struct CcArgs {
    const uint8_t* mask; const uint8_t* target; uint8_t* out; int32_t* info; unsigned* ws;
    int HW, W, stride, cls, fill, conn;
};

template <bool LDS, int NT>
__global__ __launch_bounds__(NT) void largest_component_kernel(CcArgs a)
{
    constexpr int NW = NT / 64;
    __shared__ int s_n[NW][1], s_comp[NW][1], s_hit[NW][2], s_fail;
    __shared__ u64 s_best[NW];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, HW = a.HW;
    const size_t f = blockIdx.x;
    const unsigned cls = (unsigned)a.cls, fill = (unsigned)a.fill;
    const uint8_t* tgt = a.target ? a.target + f * (size_t)HW : nullptr;
    int32_t* info = a.info + f * 8;
    const MaskFrame<NT> fr(a.mask + f * (size_t)HW, HW, a.W, cls);
    const Labels<LDS> L = frame_labels<LDS>(a.ws, f, a.stride);
    if (tid == 0) s_fail = 0;

    // pass 1: n
    int n;
    {
        int c = 0;
        fr.sweep_bits([&](unsigned m, int) { c += __builtin_popcount(m); });
        c = wave_sum(c);
        if (lane == 0) s_n[wv][0] = c;
        __syncthreads();
        n = wg_sum(s_n, 0);
    }

    int comps = 0, n_kept = 0, label_kept = -1;
    bool filter = false;
    if (n > 0) {                                           // (uniform)
        label_components<false>(fr, L, a.stride, HW, a.conn == 8, s_fail);
        label_sizes<false>(fr, L);
        __syncthreads();

        // pass 7: the components, and the largest (ties: the smallest label) as the maximum of size * 2^32 + ~label
        {
            int c = 0;
            u64 best = 0;
            fr.sweep_p([&](int p) {
                const unsigned v = L.ld((unsigned)p);
                if (v & LABEL_ROOT) {
                    ++c;
                    const u64 key = ((u64)(v & ~LABEL_ROOT) << 32) | (u64)(~(unsigned)p);
                    best = key > best ? key : best;
                }
            });
            c = wave_sum(c);
            best = wave_max(best);
            if (lane == 0) { s_comp[wv][0] = c; s_best[wv] = best; }
            __syncthreads();
            comps = wg_sum(s_comp, 0);
            best = 0;
#pragma unroll
            for (int w = 0; w < NW; ++w) best = s_best[w] > best ? s_best[w] : best;
            n_kept = (int)(best >> 32);
            label_kept = (int)~(unsigned)best;
        }
        if (s_fail) { comps = -1; n_kept = n; label_kept = -1; }
        else filter = n_kept != n;
    }

    // pass 8: out, and what the removed pixels were in the target
    int hc = 0, hf = 0;
    const unsigned kl = (unsigned)label_kept;
    rewrite_frame<false>(fr, a.out + f * (size_t)HW, HW, filter, fill, [&](int p) -> bool {        // p is of the class: is it removed?
        if (L.root((unsigned)p) == kl) return false;
        if (tgt) {
            const unsigned t = tgt[p];
            hc += t == cls ? 1 : 0;
            hf += t == fill ? 1 : 0;
        }
        return true;
    });
    hc = wave_sum(hc);
    hf = wave_sum(hf);
    if (lane == 0) { s_hit[wv][0] = hc; s_hit[wv][1] = hf; }
    __syncthreads();
    if (tid < 8) {
        int v = 0;
        if (tid == 0) v = comps;
        else if (tid == 1) v = n;
        else if (tid == 2) v = n_kept;
        else if (tid == 3) v = label_kept;
        else if (tid == 4 || tid == 5) v = wg_sum(s_hit, tid - 4);
        info[tid] = v;
    }
}

}  // namespace

extern "C" size_t gdkvm_largest_component_workspace_bytes(int frames, int H, int W) { return label_workspace_bytes(frames, H, W); }

extern "C" int gdkvm_largest_component(const uint8_t* mask, const uint8_t* target, uint8_t* out, int32_t* info, void* workspace,
                                       size_t workspace_bytes, int frames, int H, int W, int cls, int connectivity, int fill, void* stream)
{
    if (int rc = mask_check_shape("largest_component", frames, H, W)) return rc;
    if (int rc = mask_check_cls("largest_component", GDKVM_ERR_SHAPE, cls)) return rc;
    if (int rc = mask_check_connectivity("largest_component", connectivity)) return rc;
    if (fill < 0 || fill > 255 || fill == cls)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "largest_component: fill=%d must lie in 0..255 and differ from cls=%d", fill, cls);
    if (frames == 0) return GDKVM_OK;
    if (int rc = mask_check_in_out("largest_component", mask, out, info, (size_t)frames * (size_t)H * (size_t)W)) return rc;
    const size_t need = label_workspace_bytes(frames, H, W);
    if (int rc = mask_check_workspace("largest_component", H, W, need, workspace, workspace_bytes)) return rc;
    if (int rc = gdkvm_check_device()) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    CcArgs a{mask, target, out, info, static_cast<unsigned*>(workspace), H * W, W, (int)label_stride(H, W), cls, fill, connectivity};
    if (!need) hipLaunchKernelGGL((largest_component_kernel<true, 256>), dim3((unsigned)frames), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((largest_component_kernel<false, 1024>), dim3((unsigned)frames), dim3(1024), 0, st, a);
    GDKVM_LAUNCH_CHECK("largest_component_kernel");
    return GDKVM_OK;
}
