// adamw.hip -- the optimiser step of the training step: multi-tensor AdamW with global-norm clipping, the learning-rate schedule, a
// non-finite guard and an EMA of the weights, in three kernels on the caller's stream (include/gdkvm.h holds the definition).
//
// The tensors are addressed by a TABLE PASSED BY VALUE in the kernel arguments: per tensor the addresses of parameter, gradient, both moments
// and the optional EMA copy, the element count and the weight decay.  Autograd allocates gradients afresh every eager step, so a table kept
// on the device would go stale; under a capture the addresses are fixed and kernel arguments are captured with the launch, so a replay needs
// no host-to-device copy of anything.  A launch takes at most ADAMW_MAX_T entries (table + chunk prefix + scalars stay under the 4 KB of
// kernel arguments; the code object's .kernarg_segment_size is 3972 / 3996, without hidden arguments, and the kernels have no private segment: the table is read from the
// argument segment, not copied to scratch); gdkvm_adamw_step splits longer lists.  A workgroup serves ONE chunk of ADAMW_CHUNK elements of one
// tensor and finds its (tensor, chunk) by a binary search over the launch's prefix of chunk counts.
//   1. adamw_sumsq_kernel     one fp32 partial per chunk -- every lane sums its quads in element order, the lanes join in a fixed butterfly,
//                             the waves in wave order -- at the chunk's GLOBAL index in the workspace: the partials depend neither on the
//                             split into launches nor on the grid, and not on which access path (16-byte / element) a tensor takes.
//   2. adamw_finalize_kernel  one workgroup, double precision: every lane sums a contiguous run of partials in index order, the lane sums join
//                             in a fixed binary tree; norm, the non-finite verdict, step counter, clip coefficient, scheduled learning rate and
//                             bias corrections go to the persistent state block, rounded ONCE to fp32 where the update reads fp32.
//   3. adamw_update_kernel    returns at once when the verdict is "skip"; otherwise the update per element in fp32, every rounding the one
//                             written (contraction off, fused operations spelled out).
// No atomics, no workgroup waits for another, nothing allocates or synchronises; every loop is bounded by the element or partial count.

#include "gdkvm_device.hpp"

#include <cmath>

namespace {

constexpr int ADAMW_NT = 256;                  // lanes of a workgroup
constexpr int ADAMW_CHUNK = 4096;              // elements of a chunk: 4 quads per lane
constexpr int ADAMW_QUADS = ADAMW_CHUNK / (4 * ADAMW_NT);
constexpr int ADAMW_MAX_T = 76;                // table entries of one launch

struct AdamwEntry {
    float* p; const float* g; float* m; float* v; float* e;      // e: the EMA copy, or null
    unsigned n; float wd;
};
struct AdamwTable {
    AdamwEntry t[ADAMW_MAX_T];
    int first[ADAMW_MAX_T + 1];                // first[i]: chunks of this launch before entry i; first[count] = the grid
    int count;
};
static_assert(sizeof(AdamwEntry) == 48 && sizeof(AdamwTable) + 40 <= 4096, "table + scalars must fit the kernel argument segment");

// the persistent state block (gdkvm.h: GDKVM_ADAMW_STATE_BYTES); the host reads the first five slots
struct AdamwState {
    long long step, skipped;
    double grad_norm, clip_coef, lr;
    int apply; float coef, lr_t, step_size;    // what the update reads: the verdict, coef, lr(t), lr(t) / (1 - beta1^t)
    float sqrt_bc2; int pad;                   // sqrt(1 - beta2^t)
};
static_assert(sizeof(AdamwState) == GDKVM_ADAMW_STATE_BYTES, "state block layout");

struct AdamwHyper {
    double lr, beta1, beta2, max_norm, min_lr_ratio, poly_power;
    long long warmup, total;
    int schedule, partials;
};

__device__ __forceinline__ bool adamw_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// (wave-uniform) the entry whose chunks hold workgroup b: the largest i with first[i] <= b.  At most 7 halvings of ADAMW_MAX_T.
__device__ __forceinline__ int adamw_find(const AdamwTable& T, int b)
{
    int lo = 0, hi = T.count;                  // first[lo] <= b < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (T.first[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

// elements i .. i + 3 of x (zeros past n): one 16-byte load where the tensor allows it and the quad is whole
template <bool VEC>
__device__ __forceinline__ f32x4 adamw_ld4(const float* x, unsigned i, unsigned n)
{
    if (VEC && i + 4 <= n) return *reinterpret_cast<const f32x4*>(x + i);
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 4; ++k) if (i + k < n) r[k] = x[i + k];
    return r;
}
template <bool VEC>
__device__ __forceinline__ void adamw_st4(float* x, unsigned i, unsigned n, const f32x4& r)
{
    if (VEC && i + 4 <= n) { *reinterpret_cast<f32x4*>(x + i) = r; return; }
#pragma unroll
    for (int k = 0; k < 4; ++k) if (i + k < n) x[i + k] = r[k];
}

template <bool VEC>
__device__ __forceinline__ float adamw_chunk_sumsq(const float* g, unsigned base, unsigned n, int tid)
{
    f32x4 q[ADAMW_QUADS];
#pragma unroll
    for (int j = 0; j < ADAMW_QUADS; ++j) q[j] = adamw_ld4<VEC>(g, base + 4u * (unsigned)(j * ADAMW_NT + tid), n);
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < ADAMW_QUADS; ++j)
#pragma unroll
        for (int k = 0; k < 4; ++k) s = __fmaf_rn(q[j][k], q[j][k], s);
    return s;
}

__global__ __launch_bounds__(ADAMW_NT) void adamw_sumsq_kernel(AdamwTable T, float* partials, int chunk_base)
{
    __shared__ float s_w[ADAMW_NT / 64];
    const int tid = threadIdx.x, b = blockIdx.x, i = adamw_find(T, b);
    const float* g = T.t[i].g;
    const unsigned n = T.t[i].n, base = (unsigned)(b - T.first[i]) * (unsigned)ADAMW_CHUNK;
    float s = adamw_al16(g) ? adamw_chunk_sumsq<true>(g, base, n, tid) : adamw_chunk_sumsq<false>(g, base, n, tid);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
    if ((tid & 63) == 0) s_w[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        float r = s_w[0];
#pragma unroll
        for (int w = 1; w < ADAMW_NT / 64; ++w) r += s_w[w];
        partials[chunk_base + b] = r;
    }
}

__global__ __launch_bounds__(ADAMW_NT) void adamw_finalize_kernel(const float* partials, AdamwState* st, AdamwHyper h)
{
    __shared__ double s_a[ADAMW_NT];
    const int tid = threadIdx.x, per = (h.partials + ADAMW_NT - 1) / ADAMW_NT;
    const int lo = min(tid * per, h.partials), hi = min(lo + per, h.partials);
    double a = 0.0;
    for (int i = lo; i < hi; ++i) a += (double)partials[i];
    s_a[tid] = a;
    __syncthreads();
    for (int s = ADAMW_NT / 2; s >= 1; s >>= 1) {
        if (tid < s) s_a[tid] += s_a[tid + s];
        __syncthreads();
    }
    if (tid != 0) return;
    const double sum = s_a[0], norm = sqrt(sum);
    st->grad_norm = norm;
    if (!isfinite(sum)) {                      // a non-finite gradient: the step is skipped, the counter stays
        st->apply = 0;
        st->skipped += 1;
        st->clip_coef = 0.0;
        return;
    }
    const long long t = st->step + 1;
    st->step = t;
    const double coef = h.max_norm > 0.0 ? fmin(1.0, h.max_norm / (norm + 1e-6)) : 1.0;
    double lr = h.lr;
    if (t <= h.warmup) {
        lr = h.lr * (double)t / (double)h.warmup;
    } else if (h.schedule != GDKVM_SCHEDULE_CONSTANT) {
        const long long span = h.total - h.warmup > 1 ? h.total - h.warmup : 1;
        const double s = fmin(1.0, (double)(t - h.warmup) / (double)span), r = h.min_lr_ratio;
        const double shape = h.schedule == GDKVM_SCHEDULE_COSINE ? 0.5 * (1.0 + cos(3.14159265358979323846 * s)) : pow(1.0 - s, h.poly_power);
        lr = h.lr * (r + (1.0 - r) * shape);
    }
    const double bc1 = 1.0 - pow(h.beta1, (double)t), bc2 = 1.0 - pow(h.beta2, (double)t);
    st->clip_coef = coef;
    st->lr = lr;
    st->apply = 1;
    st->coef = (float)coef;
    st->lr_t = (float)lr;
    st->step_size = (float)(lr / bc1);
    st->sqrt_bc2 = (float)sqrt(bc2);
}

struct AdamwConst { float beta1, omb1, beta2, omb2, eps, ema, omema; };

template <bool VEC, bool EMA>
__device__ __forceinline__ void adamw_chunk_update(const AdamwEntry& t, unsigned base, int tid, const AdamwState* st, const AdamwConst& c)
{
#pragma clang fp contract(off)
    const unsigned n = t.n;
    const float coef = st->coef, step_size = st->step_size, sqrt_bc2 = st->sqrt_bc2;
    const float keep = 1.0f - st->lr_t * t.wd;
    f32x4 p[ADAMW_QUADS], g[ADAMW_QUADS], m[ADAMW_QUADS], v[ADAMW_QUADS], e[ADAMW_QUADS];
#pragma unroll
    for (int j = 0; j < ADAMW_QUADS; ++j) {
        const unsigned i = base + 4u * (unsigned)(j * ADAMW_NT + tid);
        p[j] = adamw_ld4<VEC>(t.p, i, n); g[j] = adamw_ld4<VEC>(t.g, i, n);
        m[j] = adamw_ld4<VEC>(t.m, i, n); v[j] = adamw_ld4<VEC>(t.v, i, n);
        if (EMA) e[j] = adamw_ld4<VEC>(t.e, i, n);
    }
#pragma unroll
    for (int j = 0; j < ADAMW_QUADS; ++j) {
        const unsigned i = base + 4u * (unsigned)(j * ADAMW_NT + tid);
        if (i >= n) break;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gs = coef * g[j][k];
            const float mk = __fmaf_rn(c.beta1, m[j][k], c.omb1 * gs);
            const float vk = __fmaf_rn(c.beta2, v[j][k], c.omb2 * gs * gs);
            const float denom = sqrtf(vk) / sqrt_bc2 + c.eps;
            const float pk = __fmaf_rn(-step_size, mk / denom, p[j][k] * keep);
            m[j][k] = mk; v[j][k] = vk; p[j][k] = pk;
            if (EMA) e[j][k] = __fmaf_rn(c.ema, e[j][k], c.omema * pk);
        }
        adamw_st4<VEC>(t.p, i, n, p[j]); adamw_st4<VEC>(t.m, i, n, m[j]); adamw_st4<VEC>(t.v, i, n, v[j]);
        if (EMA) adamw_st4<VEC>(t.e, i, n, e[j]);
    }
}

__global__ __launch_bounds__(ADAMW_NT) void adamw_update_kernel(AdamwTable T, const AdamwState* st, AdamwConst c)
{
    if (!st->apply) return;                    // (uniform) the step is skipped: nothing is written
    const int tid = threadIdx.x, b = blockIdx.x, i = adamw_find(T, b);
    const AdamwEntry& t = T.t[i];
    const unsigned base = (unsigned)(b - T.first[i]) * (unsigned)ADAMW_CHUNK;
    const bool vec = adamw_al16(t.p) && adamw_al16(t.g) && adamw_al16(t.m) && adamw_al16(t.v) && adamw_al16(t.e);
    if (t.e) {
        if (vec) adamw_chunk_update<true, true>(t, base, tid, st, c); else adamw_chunk_update<false, true>(t, base, tid, st, c);
    } else {
        if (vec) adamw_chunk_update<true, false>(t, base, tid, st, c); else adamw_chunk_update<false, false>(t, base, tid, st, c);
    }
}

inline bool adamw_real(double x) { return std::isfinite(x) && x >= 0.0; }
inline bool adamw_addr_ok(uint64_t a) { return a != 0 && (a & 3u) == 0; }
inline long long adamw_chunks(long long n) { return (n + ADAMW_CHUNK - 1) / ADAMW_CHUNK; }

}  // namespace

extern "C" size_t gdkvm_adamw_workspace_bytes(int tensors, long long total_elems)
{
    if (tensors <= 0 || total_elems <= 0) return 0;
    return (size_t)(total_elems / ADAMW_CHUNK + tensors) * sizeof(float);
}

extern "C" int gdkvm_adamw_step(const uint64_t* params, const uint64_t* grads, const uint64_t* exp_avg, const uint64_t* exp_avg_sq,
                                const uint64_t* ema, const int64_t* counts, const float* decays, int tensors, void* state,
                                void* workspace, size_t workspace_bytes, double lr, double beta1, double beta2, double eps,
                                double max_norm, double ema_decay, double min_lr_ratio, double poly_power, long long warmup_steps,
                                long long total_steps, int schedule, void* stream)
{
    if (tensors < 0) return gdkvm_fail(GDKVM_ERR_SHAPE, "adamw_step: tensors = %d", tensors);
    if (!adamw_real(lr) || !adamw_real(eps) || !adamw_real(max_norm) || !adamw_real(ema_decay) || ema_decay >= 1.0)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "adamw_step: lr = %g, eps = %g, max_norm = %g must be finite and >= 0, ema_decay = %g in [0, 1)",
                          lr, eps, max_norm, ema_decay);
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0))
        return gdkvm_fail(GDKVM_ERR_SHAPE, "adamw_step: betas = (%g, %g) outside [0, 1)", beta1, beta2);
    if (schedule != GDKVM_SCHEDULE_CONSTANT && schedule != GDKVM_SCHEDULE_COSINE && schedule != GDKVM_SCHEDULE_POLY)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "adamw_step: unknown schedule %d", schedule);
    if (!(min_lr_ratio >= 0.0 && min_lr_ratio <= 1.0) || !adamw_real(poly_power) || warmup_steps < 0 || total_steps < 0)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "adamw_step: min_lr_ratio = %g outside [0, 1], poly_power = %g, warmup_steps = %lld or total_steps = %lld "
                          "negative", min_lr_ratio, poly_power, warmup_steps, total_steps);
    if (tensors == 0) return GDKVM_OK;
    if (!params || !grads || !exp_avg || !exp_avg_sq || !counts || !decays)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "adamw_step: null host array (only ema may be null)");
    if (!state || (reinterpret_cast<uintptr_t>(state) & 7u))
        return gdkvm_fail(GDKVM_ERR_SHAPE, "adamw_step: the state block must be non-null and 8-byte aligned");
    long long chunks = 0, total = 0;
    for (int i = 0; i < tensors; ++i) {
        if (!adamw_addr_ok(params[i]) || !adamw_addr_ok(grads[i]) || !adamw_addr_ok(exp_avg[i]) || !adamw_addr_ok(exp_avg_sq[i]) ||
            (ema && ema[i] && !adamw_addr_ok(ema[i])))
            return gdkvm_fail(GDKVM_ERR_SHAPE, "adamw_step: tensor %d: a null or not 4-byte aligned address", i);
        if (counts[i] <= 0 || counts[i] > 0x7fffffffll - ADAMW_CHUNK)
            return gdkvm_fail(GDKVM_ERR_SHAPE, "adamw_step: tensor %d: count = %lld outside 1..2^31 - %d", i, (long long)counts[i], ADAMW_CHUNK + 1);
        if (!adamw_real((double)decays[i])) return gdkvm_fail(GDKVM_ERR_SHAPE, "adamw_step: tensor %d: weight decay = %g", i, (double)decays[i]);
        chunks += adamw_chunks(counts[i]);
        total += counts[i];
    }
    if (chunks > 0x7fffffffll) return gdkvm_fail(GDKVM_ERR_SHAPE, "adamw_step: %lld chunks are too many", chunks);
    const size_t need = gdkvm_adamw_workspace_bytes(tensors, total);
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 3u) || workspace_bytes < need)
        return gdkvm_fail(GDKVM_ERR_SHAPE, "adamw_step: workspace null, misaligned or short (%zu bytes, need %zu)", workspace_bytes, need);
    if (int rc = gdkvm_check_device()) return rc;

    hipStream_t st = static_cast<hipStream_t>(stream);
    AdamwState* S = static_cast<AdamwState*>(state);
    float* partials = static_cast<float*>(workspace);
    AdamwTable T;
    // fills T with the entries from `i0` on (at most ADAMW_MAX_T); returns the index after the last one taken
    auto fill = [&](int i0) {
        const int cnt = tensors - i0 < ADAMW_MAX_T ? tensors - i0 : ADAMW_MAX_T;
        int first = 0;
        for (int k = 0; k < cnt; ++k) {
            const int i = i0 + k;
            T.t[k] = AdamwEntry{reinterpret_cast<float*>(params[i]), reinterpret_cast<const float*>(grads[i]), reinterpret_cast<float*>(exp_avg[i]),
                                reinterpret_cast<float*>(exp_avg_sq[i]), ema_decay > 0.0 && ema ? reinterpret_cast<float*>(ema[i]) : nullptr,
                                (unsigned)counts[i], decays[i]};
            T.first[k] = first;
            first += (int)adamw_chunks(counts[i]);
        }
        for (int k = cnt; k < ADAMW_MAX_T; ++k) { T.t[k] = AdamwEntry{}; T.first[k] = first; }
        T.first[cnt] = first;
        T.first[ADAMW_MAX_T] = first;
        T.count = cnt;
        return i0 + cnt;
    };
    int chunk_base = 0;
    for (int i0 = 0; i0 < tensors;) {
        i0 = fill(i0);
        hipLaunchKernelGGL(adamw_sumsq_kernel, dim3((unsigned)T.first[T.count]), dim3(ADAMW_NT), 0, st, T, partials, chunk_base);
        GDKVM_LAUNCH_CHECK("adamw_sumsq_kernel");
        chunk_base += T.first[T.count];
    }
    const AdamwHyper h{lr, beta1, beta2, max_norm, min_lr_ratio, poly_power, warmup_steps, total_steps, schedule, (int)chunks};
    hipLaunchKernelGGL(adamw_finalize_kernel, dim3(1), dim3(ADAMW_NT), 0, st, partials, S, h);
    GDKVM_LAUNCH_CHECK("adamw_finalize_kernel");
    const AdamwConst c{(float)beta1, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps, (float)ema_decay, (float)(1.0 - ema_decay)};
    for (int i0 = 0; i0 < tensors;) {
        i0 = fill(i0);
        hipLaunchKernelGGL(adamw_update_kernel, dim3((unsigned)T.first[T.count]), dim3(ADAMW_NT), 0, st, T, S, c);
        GDKVM_LAUNCH_CHECK("adamw_update_kernel");
    }
    return GDKVM_OK;
}
