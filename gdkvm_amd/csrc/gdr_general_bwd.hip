// gdr_general_bwd.hip -- the backward of gdr_general.hip's recurrence: training at per-head key widths 72 .. 256 (gdr_wide_keys), behind
// gdkvm_scan_train_bwd.  The gradient of exactly the function the forward computes -- all three rules, any N, flags 0 .. 3, f32 / bf16 I/O.
//
// Two kernels, no float atomics (bit-reproducible):
//   gdr_general_bwd_kernel     one workgroup per (clip, head, 16-column slice of the state), like the forward: the columns of S never mix,
//                              so each slice walks the frames in reverse on its own with its [Dk][16] slice of S and of dS in LDS.  Per
//                              frame, from the saved state before it (s_hist):
//                                1. (delta rules) the forward's token loop once more, in the forward's exact arithmetic, to recover the
//                                   error rows e_n = v_n - S^T kn_n into the workspace;
//                                2. the tokens in reverse: dv = de = b (kn^T dS'), dS = dS' - kn de^T (rule 2; rule 1 sends -kn de^T to
//                                   the frame's decayed start state), and the rule-2 state before the token as S' - b kn e^T;
//                                3. the decay (d alpha) and the read-out, R = Qn S_{t-1}: dS += Qn^T dR.
//                              Every term that sums over the state's columns (d kn, d qn, d beta, d alpha) leaves as this slice's partial.
//   gdr_general_bwd_epilogue   one wave per token row: adds the slices' partials in slice order, then backpropagates through the q / k
//                              normalisation and the gate sigmoids.
// Serial over tokens like the forward (three workgroup barriers per token here, two there): a coverage path, not the measured one.
#include "gdkvm_common.hpp"
#include "gdr_ws.hpp"
#include "gdr_general.hpp"

namespace {

constexpr int GB_MAXDK = 256;
constexpr int GB_CHUNK = 64;             // tokens whose inverse norms / gates (and read-out gradients) are staged at a time

struct GeneralBwdArgs {
    const void* q; const void* k; const void* v; const float* alpha; const float* beta; const void* d_r; const float* d_s_out;
    const float* hist; void* d_v; float* d_s_in;
    float* e; float* pk; float* pq; float* pb; float* pa;
    int B, T, Hh, N, Dk, Dv, rule, flags;
};

template <int IO>
__device__ __forceinline__ float row_inv_norm(const void* x, size_t row, int Dk)
{   // the forward's rsqrt(sum x^2 + eps), summed in channel order
    float ss = 0.f;
    for (int d = 0; d < Dk; ++d) { const float y = load1<IO>(x, row + d); ss = fmaf(y, y, ss); }
    return rsqrtf(ss + 1e-12f);
}

template <int IO>
__global__ __launch_bounds__(256) void gdr_general_bwd_kernel(GeneralBwdArgs a)
{
    __shared__ float s_S[GB_MAXDK][17];                   // the state slice (rows padded: the row-wise phases read across columns)
    __shared__ float s_dS[GB_MAXDK][17];                  // its gradient
    __shared__ float s_dS0[GB_MAXDK][17];                 // rule 1: the gradient w.r.t. the frame's decayed start state, via the errors
    __shared__ float s_red[16][17];
    __shared__ float s_e[16], s_de[16];
    __shared__ float s_kinv[GB_CHUNK], s_be[GB_CHUNK];
    __shared__ float s_dr[GB_CHUNK][16];
    const int tid = threadIdx.x, c = tid & 15, dg = tid >> 4;
    const int sl = blockIdx.x, NS = gridDim.x, bh = blockIdx.y, b = bh / a.Hh, h = bh % a.Hh;
    const int N = a.N, Dk = a.Dk, Dv = a.Dv, Hh = a.Hh, T = a.T, rule = a.rule, c0 = 16 * sl;
    const bool norm = a.flags & GDKVM_FLAG_NORMALIZE_QK, logits = a.flags & GDKVM_FLAG_GATE_LOGITS;
    const int nj = (Dk + 15) / 16;
    const size_t FHN = (size_t)a.B * T * N * Hh, FH = (size_t)a.B * T * Hh;
    float* E = a.e + ((size_t)bh * NS + sl) * N * 16;

    for (int j = 0; j < nj; ++j) {
        const int d = dg + 16 * j;
        if (d < Dk) { s_dS[d][c] = a.d_s_out ? a.d_s_out[((size_t)bh * Dk + d) * Dv + c0 + c] : 0.f; s_dS0[d][c] = 0.f; }
    }

    for (int t = T - 1; t >= 0; --t) {
        const size_t bt = (size_t)b * T + t;
        const float* hs = a.hist + ((bt * Hh + h) * Dk) * Dv + c0;
        float al = a.alpha[bt * Hh + h];
        if (logits) al = 1.f / (1.f + __expf(-al));
        for (int j = 0; j < nj; ++j) {                     // the decayed start state, in the forward's bits
            const int d = dg + 16 * j;
            if (d < Dk) s_S[d][c] = al * hs[(size_t)d * Dv + c];
        }
        __syncthreads();

        // ---- 1. the errors of the delta rules, token by token in the forward's order and arithmetic (rule 2 also advances s_S to the frame's end)
        for (int nc = 0; rule != 0 && nc < N; nc += GB_CHUNK) {
            const int cnt = min(GB_CHUNK, N - nc);
            if (tid < cnt) s_kinv[tid] = norm ? row_inv_norm<IO>(a.k, ((bt * N + nc + tid) * Hh + h) * Dk, Dk) : 1.f;
            __syncthreads();
            for (int i = 0; i < cnt; ++i) {
                const int n = nc + i;
                const size_t krow = ((bt * N + n) * Hh + h) * Dk;
                const float kinv = s_kinv[i];
                float be = a.beta[(bt * N + n) * Hh + h];
                if (logits) be = 1.f / (1.f + __expf(-be));
                float kn[GB_MAXDK / 16];
                float part = 0.f;
                for (int j = 0; j < nj; ++j) {
                    const int d = dg + 16 * j;
                    kn[j] = d < Dk ? load1<IO>(a.k, krow + d) * kinv : 0.f;
                    if (d < Dk) part = fmaf(kn[j], s_S[d][c], part);
                }
                float e = load1<IO>(a.v, ((bt * N + n) * Hh + h) * Dv + c0 + c);
                s_red[dg][c] = part;
                __syncthreads();
                if (dg == 0) {
                    float dot = 0.f;
#pragma unroll
                    for (int g = 0; g < 16; ++g) dot += s_red[g][c];
                    s_e[c] = e - dot;
                    E[(size_t)n * 16 + c] = e - dot;
                }
                __syncthreads();
                e = s_e[c];
                if (rule == 2) {
                    const float bev = be * e;
                    for (int j = 0; j < nj; ++j) {
                        const int d = dg + 16 * j;
                        if (d < Dk) s_S[d][c] = fmaf(kn[j], bev, s_S[d][c]);
                    }
                }
            }
            __syncthreads();
        }

        // ---- 2. the tokens in reverse
        for (int nc = ((N - 1) / GB_CHUNK) * GB_CHUNK; nc >= 0; nc -= GB_CHUNK) {
            const int cnt = min(GB_CHUNK, N - nc);
            if (tid < cnt) {
                s_kinv[tid] = norm ? row_inv_norm<IO>(a.k, ((bt * N + nc + tid) * Hh + h) * Dk, Dk) : 1.f;
                const float be = a.beta[(bt * N + nc + tid) * Hh + h];
                s_be[tid] = logits ? 1.f / (1.f + __expf(-be)) : be;
            }
            __syncthreads();
            for (int i = cnt - 1; i >= 0; --i) {
                const int n = nc + i;
                const size_t krow = ((bt * N + n) * Hh + h) * Dk, vrow = ((bt * N + n) * Hh + h) * Dv + c0, rw = (bt * N + n) * Hh + h;
                const float kinv = s_kinv[i], be = s_be[i];
                const float e = rule == 0 ? load1<IO>(a.v, vrow + c) : E[(size_t)n * 16 + c];
                float kn[GB_MAXDK / 16];
                float part = 0.f;
                for (int j = 0; j < nj; ++j) {
                    const int d = dg + 16 * j;
                    kn[j] = d < Dk ? load1<IO>(a.k, krow + d) * kinv : 0.f;
                    if (d < Dk) {
                        if (rule == 2) s_S[d][c] = fmaf(-kn[j], be * e, s_S[d][c]);     // the state before this token
                        part = fmaf(kn[j], s_dS[d][c], part);
                    }
                }
                s_red[dg][c] = part;
                __syncthreads();
                if (dg == 0) {                             // g = kn^T dS' per column; de = b g is d v; d b = sum_c e g (this slice's part)
                    float g = 0.f;
#pragma unroll
                    for (int r = 0; r < 16; ++r) g += s_red[r][c];
                    const float de = be * g;
                    store1<IO>(a.d_v, vrow + c, de);
                    s_de[c] = de;
                    s_e[c] = e;
                    float x = e * g;
                    x += __shfl_xor(x, 8, 16);
                    x += __shfl_xor(x, 4, 16);
                    x += __shfl_xor(x, 2, 16);
                    x += __shfl_xor(x, 1, 16);
                    if (c == 0) a.pb[sl * FHN + rw] = x;
                }
                __syncthreads();
                if (tid < Dk) {                            // d kn = b dS' e - S_ref de, S_ref: the state the error was taken against
                    float a1 = 0.f, a2 = 0.f;
#pragma unroll
                    for (int cc = 0; cc < 16; ++cc) {
                        a1 = fmaf(s_dS[tid][cc], s_e[cc], a1);
                        if (rule != 0) a2 = fmaf(s_S[tid][cc], s_de[cc], a2);
                    }
                    a.pk[(sl * FHN + rw) * Dk + tid] = be * a1 - a2;
                }
                __syncthreads();
                if (rule != 0) {
                    const float de = s_de[c];
                    for (int j = 0; j < nj; ++j) {
                        const int d = dg + 16 * j;
                        if (d < Dk) {
                            if (rule == 2) s_dS[d][c] = fmaf(-kn[j], de, s_dS[d][c]);
                            else s_dS0[d][c] = fmaf(-kn[j], de, s_dS0[d][c]);
                        }
                    }
                }
            }
            __syncthreads();
        }

        // ---- 3. the decay: d alpha = <dS_decayed, S_{t-1}>, dS_{t-1} = alpha dS_decayed; s_S <- S_{t-1} for the read-out
        float part = 0.f;
        for (int j = 0; j < nj; ++j) {
            const int d = dg + 16 * j;
            if (d < Dk) {
                float g = s_dS[d][c];
                if (rule == 1) { g += s_dS0[d][c]; s_dS0[d][c] = 0.f; }
                const float sp = hs[(size_t)d * Dv + c];
                s_S[d][c] = sp;
                part = fmaf(g, sp, part);
                s_dS[d][c] = al * g;
            }
        }
        s_red[dg][c] = part;
        __syncthreads();
        if (tid == 0) {
            float x = 0.f;
            for (int r = 0; r < 16; ++r)
                for (int cc = 0; cc < 16; ++cc) x += s_red[r][cc];
            a.pa[sl * FH + bt * Hh + h] = x;
        }
        // ---- the read-out R = Qn S_{t-1}: d qn = dR S_{t-1}^T (this slice's columns), dS_{t-1} += Qn^T dR
        for (int nc = 0; nc < N; nc += GB_CHUNK) {
            const int cnt = min(GB_CHUNK, N - nc);
            if (tid < cnt) s_kinv[tid] = norm ? row_inv_norm<IO>(a.q, ((bt * N + nc + tid) * Hh + h) * Dk, Dk) : 1.f;
            for (int x = tid; x < cnt * 16; x += 256)
                s_dr[x >> 4][x & 15] = load1<IO>(a.d_r, ((bt * N + nc + (x >> 4)) * Hh + h) * Dv + c0 + (x & 15));
            __syncthreads();
            if (tid < Dk) {
                for (int i = 0; i < cnt; ++i) {
                    float acc = 0.f;
#pragma unroll
                    for (int cc = 0; cc < 16; ++cc) acc = fmaf(s_dr[i][cc], s_S[tid][cc], acc);
                    a.pq[(sl * FHN + (bt * N + nc + i) * Hh + h) * Dk + tid] = acc;
                }
            }
            for (int i = 0; i < cnt; ++i) {
                const size_t qrow = ((bt * N + nc + i) * Hh + h) * Dk;
                const float qinv = s_kinv[i], dr = s_dr[i][c];
                for (int j = 0; j < nj; ++j) {
                    const int d = dg + 16 * j;
                    if (d < Dk) s_dS[d][c] = fmaf(load1<IO>(a.q, qrow + d) * qinv, dr, s_dS[d][c]);
                }
            }
            __syncthreads();
        }
    }
    if (a.d_s_in) {
        for (int j = 0; j < nj; ++j) {
            const int d = dg + 16 * j;
            if (d < Dk) a.d_s_in[((size_t)bh * Dk + d) * Dv + c0 + c] = s_dS[d][c];
        }
    }
}

__device__ __forceinline__ float wave_sum(float x)
{   // butterfly: every lane ends with the same bits (each step adds the same two values in either lane)
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

struct EpilogueArgs {
    const void* q; const void* k; const float* alpha; const float* beta; const float* pk; const float* pq; const float* pb; const float* pa;
    void* d_q; void* d_k; float* d_alpha; float* d_beta;
    int B, T, Hh, N, Dk, NS, flags;
};

// d x = xinv (d xn - xn (xn . d xn)) for xn = x xinv, xinv = rsqrt(|x|^2 + eps); the identity without GDKVM_FLAG_NORMALIZE_QK
template <int IO>
__device__ __forceinline__ void epilogue_row(const void* x, const float* part, void* dx, size_t rw, size_t FHN, int Dk, int NS, bool norm, int lane)
{
    float g[4], xv[4], ss = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = lane + 64 * j;
        g[j] = 0.f; xv[j] = 0.f;
        if (d < Dk) {
            for (int s = 0; s < NS; ++s) g[j] += part[((size_t)s * FHN + rw) * Dk + d];
            xv[j] = load1<IO>(x, rw * Dk + d);
            ss = fmaf(xv[j], xv[j], ss);
        }
    }
    if (norm) {
        const float inv = rsqrtf(wave_sum(ss) + 1e-12f);
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) dot = fmaf(xv[j] * inv, g[j], dot);
        dot = wave_sum(dot);
#pragma unroll
        for (int j = 0; j < 4; ++j) g[j] = inv * (g[j] - xv[j] * inv * dot);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int d = lane + 64 * j;
        if (d < Dk) store1<IO>(dx, rw * Dk + d, g[j]);
    }
}

template <int IO>
__global__ __launch_bounds__(256) void gdr_general_bwd_epilogue_kernel(EpilogueArgs a)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool norm = a.flags & GDKVM_FLAG_NORMALIZE_QK, logits = a.flags & GDKVM_FLAG_GATE_LOGITS;
    const size_t FHN = (size_t)a.B * a.T * a.N * a.Hh, FH = (size_t)a.B * a.T * a.Hh;
    for (size_t rw = (size_t)blockIdx.x * 4 + w; rw < FHN; rw += (size_t)gridDim.x * 4) {
        epilogue_row<IO>(a.k, a.pk, a.d_k, rw, FHN, a.Dk, a.NS, norm, lane);
        epilogue_row<IO>(a.q, a.pq, a.d_q, rw, FHN, a.Dk, a.NS, norm, lane);
        if (lane == 0) {
            float db = 0.f;
            for (int s = 0; s < a.NS; ++s) db += a.pb[(size_t)s * FHN + rw];
            if (logits) { const float sg = 1.f / (1.f + __expf(-a.beta[rw])); db *= sg * (1.f - sg); }
            a.d_beta[rw] = db;
            const size_t h = rw % a.Hh, n = (rw / a.Hh) % a.N, bt = rw / ((size_t)a.Hh * a.N);
            if (n == 0) {                                  // one row per frame-head also finishes d alpha
                const size_t fh = bt * a.Hh + h;
                float da = 0.f;
                for (int s = 0; s < a.NS; ++s) da += a.pa[(size_t)s * FH + fh];
                if (logits) { const float sg = 1.f / (1.f + __expf(-a.alpha[fh])); da *= sg * (1.f - sg); }
                a.d_alpha[fh] = da;
            }
        }
    }
}

struct GenTrainView { float* hist; float* e; float* pk; float* pq; float* pb; float* pa; size_t total; };

GenTrainView gen_carve(void* base, int B, int T, int Hh, int N, int Dk, int Dv)
{
    GenTrainView v{};
    const size_t NS = (size_t)Dv / 16, FH = (size_t)B * T * Hh, FHN = FH * N;
    size_t off = 0;                                       // (base == NULL: sizes only)
    auto take = [&](size_t bytes) { float* r = base ? reinterpret_cast<float*>(static_cast<char*>(base) + off) : nullptr; off += gdr_up256(bytes); return r; };
    v.hist = take(FH * Dk * Dv * sizeof(float));
    v.e = take((size_t)B * Hh * Dv * N * sizeof(float));
    v.pk = take(NS * FHN * Dk * sizeof(float));
    v.pq = take(NS * FHN * Dk * sizeof(float));
    v.pb = take(NS * FHN * sizeof(float));
    v.pa = take(NS * FH * sizeof(float));
    v.total = off;
    return v;
}

}  // namespace

size_t gdr_general_train_workspace_bytes(int B, int T, int Hh, int N, int Dk, int Dv)
{
    return gen_carve(nullptr, B, T, Hh, N, Dk, Dv).total;
}

float* gdr_general_train_hist(void* ws) { return static_cast<float*>(ws); }   // (the first region)

int gdr_general_train_bwd(const void* q, const void* k, const void* v, const float* alpha, const float* beta, const void* d_r,
                          const float* d_s_out, void* d_q, void* d_k, void* d_v, float* d_alpha, float* d_beta, float* d_s_in, void* ws,
                          int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype, int rule, int flags, hipStream_t st)
{
    if (int rc = gdkvm_check_device()) return rc;
    const GenTrainView w = gen_carve(ws, B, T, Hh, N, Dk, Dv);
    const GeneralBwdArgs ba{q, k, v, alpha, beta, d_r, d_s_out, w.hist, d_v, d_s_in, w.e, w.pk, w.pq, w.pb, w.pa, B, T, Hh, N, Dk, Dv, rule, flags};
    const dim3 grid((unsigned)(Dv / 16), (unsigned)(B * Hh));
    if (io_dtype == GDKVM_F32) hipLaunchKernelGGL((gdr_general_bwd_kernel<GDKVM_F32>), grid, dim3(256), 0, st, ba);
    else hipLaunchKernelGGL((gdr_general_bwd_kernel<GDKVM_BF16>), grid, dim3(256), 0, st, ba);
    GDKVM_LAUNCH_CHECK("gdr_general_bwd_kernel");
    const EpilogueArgs ea{q, k, alpha, beta, w.pk, w.pq, w.pb, w.pa, d_q, d_k, d_alpha, d_beta, B, T, Hh, N, Dk, Dv / 16, flags};
    const size_t rows = (size_t)B * T * N * Hh, blocks = (rows + 3) / 4;
    const dim3 eg((unsigned)(blocks < 65536 ? blocks : 65536));
    if (io_dtype == GDKVM_F32) hipLaunchKernelGGL((gdr_general_bwd_epilogue_kernel<GDKVM_F32>), eg, dim3(256), 0, st, ea);
    else hipLaunchKernelGGL((gdr_general_bwd_epilogue_kernel<GDKVM_BF16>), eg, dim3(256), 0, st, ea);
    GDKVM_LAUNCH_CHECK("gdr_general_bwd_epilogue_kernel");
    return GDKVM_OK;
}
