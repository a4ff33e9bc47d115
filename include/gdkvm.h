/* gdkvm.h -- C ABI of the MI355X-native GDKVM memory path (libgdkvm_hip.so, gfx950 only).
 *
 * The reference snapshot exposes NO plugin / operator / FFI interface for this path: /root/reference is the
 * project website and holds no model code (the code lives in the repo named at
 * /root/reference/README.md:1 and is excluded at /root/reference/.gitignore:73-76).  There is therefore no
 * reference interface file:line for these entry points to replace; each one is instead tied to the
 * operation the reference *names* (/root/reference/README.md:20, .../website/src/content/homepage/en.json:20)
 * and to the row of SURVEY.md §8(a) that specifies it.  INTEGRATION.md shows the binding a maintainer of the
 * real model code would add (ctypes stub + nn.Module seam).
 *
 * Conventions (all entry points)
 *   - every pointer is a DEVICE pointer owned by the caller (hipMalloc / torch CUDA tensor); nothing is
 *     allocated, retained or freed by the callee; 16-byte alignment is required for every buffer;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); calls are asynchronous with
 *     respect to the host and stream-ordered; no host synchronisation happens inside (graph-capturable);
 *   - return value: 0 on success, <0 on error; never throws, never exits:
 *       GDKVM_ERR_SHAPE (-1) bad / unsupported shape    GDKVM_ERR_DTYPE (-2) unsupported io_dtype
 *       GDKVM_ERR_ARCH  (-3) device is not gfx950       GDKVM_ERR_LAUNCH(-4) HIP launch failure
 *       GDKVM_ERR_WORKSPACE (-5) workspace too small    GDKVM_ERR_ARG (-6) null / misaligned pointer
 *     (a return code speaks about the ARGUMENTS of an asynchronous call, never about its data: see gdkvm_scan_status, GDKVM_ERR_RANGE)
 *     gdkvm_last_error() returns a thread-local message for the most recent failure on this thread;
 *   - re-entrant; concurrent calls are safe iff their output / workspace buffers are distinct.
 *
 * Tensor layouts are token-major with the channel innermost (what an NHWC 1x1 convolution emits):
 *   q, k   [B, T, N, Hh, Dk]     v, r   [B, T, N, Hh, Dv]     (io_dtype: f32 or bf16)
 *   alpha  [B, T, Hh]  fp32      beta   [B, T, N, Hh]  fp32
 *   state  [B, Hh, Dk, Dv] fp32  (always fp32: the recurrent memory is never stored narrow)
 */
#ifndef GDKVM_H
#define GDKVM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDKVM_ABI_VERSION 1

enum { GDKVM_OK = 0, GDKVM_ERR_SHAPE = -1, GDKVM_ERR_DTYPE = -2, GDKVM_ERR_ARCH = -3,
       GDKVM_ERR_LAUNCH = -4, GDKVM_ERR_WORKSPACE = -5, GDKVM_ERR_ARG = -6,
       GDKVM_ERR_RANGE = -7 /* gdkvm_scan_status only: the data left the numeric range of the default operand format */ };

enum { GDKVM_F32 = 0, GDKVM_BF16 = 1 };                       /* io_dtype */

/* GDR write rule */
enum { GDKVM_RULE_GATED_LINEAR = 0,      /* S <- a S + sum_i b_i k_i v_i^T  (literal BASELINE.json formula) */
       GDKVM_RULE_DELTA_PARALLEL = 1,    /* all tokens of a frame erase against the decayed state          */
       GDKVM_RULE_DELTA_SEQUENTIAL = 2   /* token-sequential gated delta rule (default)                    */ };

/* prologue flags */
enum { GDKVM_FLAG_NORMALIZE_QK = 1,      /* q,k <- x * rsqrt(sum x^2 + 1e-12)   */
       GDKVM_FLAG_GATE_LOGITS = 2,       /* alpha, beta are logits -> sigmoid   */
       GDKVM_FLAG_TRAIN = 4,             /* prep also emits the operand layouts gdkvm_scan_bwd reads (set by
                                            gdkvm_scan_fwd itself whenever s_hist != NULL) */
       GDKVM_FLAG_WIDE_RANGE = 8         /* operands of the state recurrence as three bf16 terms (the whole fp32 range, twice
                                            the MFMAs) instead of the default fp16 pairs (22 bits).  The default serves
                                            values and carried states of any magnitude for rules GATED_LINEAR and
                                            DELTA_SEQUENTIAL PROVIDED every frame's map is a contraction -- keys of unit norm,
                                            alpha and beta in [0, 1]: guaranteed by the kernels themselves when both
                                            GDKVM_FLAG_NORMALIZE_QK and GDKVM_FLAG_GATE_LOGITS are set, and the caller's
                                            promise when it passes keys / gates it normalised itself (raw gates above 1 or
                                            un-normalised keys without the flags void the bound below: pass this flag then).
                                            The serial kernel carries the state at 2^-e and sizes e per call and 16-column
                                            slice from that bound, 8 (max|s_in| + sum_t max|G_t|) -- e = 4 (the
                                            format's default, hence bit-identical chunked calls) for every ordinary input,
                                            larger exactly when the state needs it.  One corner is refused loudly rather
                                            than served: frames of more than 64 tokens whose chunk composition leaves the
                                            pair's range (|values| around 1e5 times the usual) come back as NaNs -- pass
                                            this flag for such inputs.  gdkvm_scan_fwd sets it itself for rule
                                            DELTA_PARALLEL, the one rule without a bound (not contractive); a caller of the
                                            split prep / apply / transition entry points passes the same flags to each. */ };

int gdkvm_abi_version(void);
const char* gdkvm_last_error(void);

/* Bytes of scratch gdkvm_scan_fwd needs for this shape (per-frame WY factors). */
size_t gdkvm_scan_workspace_bytes(int B, int T, int Hh, int N, int Dk, int Dv);

/* Rows a1+a2+a3+a5: fused LKVA read + GDR write over T frames with state carry.
 *   for t in 0..T-1:  R_t = Q_t S_{t-1};   S_t = GDR(S_{t-1}, K_t, V_t, alpha_t, beta_t)
 * s_in may be NULL (zero state); s_out may be NULL.  T == 1 is the per-frame `step` entry point.  A clip
 * processed as consecutive calls with the state carried is bit-identical to one call.
 * Names: LKVA / GDR at /root/reference/README.md:20; "state transition matrix" at
 * /root/reference/website/src/content/homepage/en.json:20.
 * Supported: Dk == 64 (the measured kernels); 8 <= Dk < 64 in multiples of 8 (gdkvm_scan_fwd only, not with s_hist: the call zero-extends
 * q, k and the state to 64 channels inside the workspace, which is exact); 64 < Dk <= 256 in multiples of 8 (gdkvm_scan_fwd only,
 * inference: the definitional recurrence in fp32 on one workgroup per 16-column slice of the state, csrc/gdr_general.hip -- same
 * results, same chunk bit-identity, no workspace, far slower than the Dk = 64 path; gdkvm_scan_status has nothing to report for it;
 * training at these widths: gdkvm_scan_train_fwd / gdkvm_scan_train_bwd, not s_hist);
 * Dv % 16 == 0; 0 <= N <= 4096 (a 1024x1024 frame at stride 16).
 * s_hist (training): if non-NULL, [B,T,Hh,Dk,Dv] fp32 receives the state BEFORE every frame; gdkvm_scan_bwd needs
 * it together with the untouched workspace of this call. */
int gdkvm_scan_fwd(const void* q, const void* k, const void* v, const float* alpha, const float* beta,
                   const float* s_in, void* r_out, float* s_out, float* s_hist, void* workspace, size_t workspace_bytes,
                   int B, int T, int Hh, int N, int Dk, int Dv,
                   int io_dtype, int rule, int flags, void* stream);

/* Did the last gdkvm_scan_fwd / gdkvm_scan_fwd_normed / gdkvm_scan_apply on `workspace` (same shape arguments and flags) stay inside the
 * range of the default fp16-pair operands?  Those calls are asynchronous and return before a kernel has seen the data; where the bound
 * on the state is not finite -- or a chunk composition of a frame of more than 64 tokens overflowed on the way -- the results are NaNs
 * (never saturated numbers), and this call says so: it copies the per-slice exponents the serial kernel left in the workspace back on
 * `stream`, WAITS for the stream (the one synchronising entry point of the library), and returns GDKVM_ERR_RANGE or GDKVM_OK.
 * GDKVM_FLAG_WIDE_RANGE serves such inputs.  Optional: nothing else in the library depends on it being called. */
int gdkvm_scan_status(const void* workspace, size_t workspace_bytes, int B, int T, int Hh, int N, int Dk, int Dv, int flags, void* stream);

/* The two stages of gdkvm_scan_fwd as separate entry points (gdkvm_scan_fwd == prep then apply on one stream).
 * `prep` is state-independent and parallel over frames: the a5 prologue incl. the query norms, and every frame folded
 * into the affine map S' = alpha (P S) + G of SURVEY.md A.3 (P = I - Kn^T Wt, G = Kn^T Ut) in the workspace; with
 * GDKVM_FLAG_TRAIN also the WY factors the backward needs.  `apply` is the serial-in-time read/write recurrence.
 * Exposed so a caller can run the prep of chunk c+1 on a second stream while chunk c is being applied, and so each
 * kernel can be timed on its own. */
int gdkvm_scan_prep(const void* q, const void* k, const void* v, const float* beta, void* workspace, size_t workspace_bytes,
                    int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype, int rule, int flags, void* stream);
int gdkvm_scan_apply(const void* q, const float* alpha, const float* s_in, void* r_out, float* s_out,
                     float* s_hist, const void* workspace, size_t workspace_bytes,
                     int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype, int flags, void* stream);

/* the same two calls for a caller that already holds the inverse L2 norms of the key and query rows --
 * gdkvm_proj_gates, which produces q, k, v, the gate logits AND these norms in one launch.  norms [B*T*N, Hh, 2] fp32:
 * 1 / sqrt(sum k^2 + 1e-12) and the same for q, of the rows AS STORED (io_dtype).  The frame-parallel kernel then neither reads q
 * nor reduces anything in its first phase.  Requires GDKVM_FLAG_NORMALIZE_QK, Dk == 64, no s_hist (inference); everything else as
 * gdkvm_scan_prep / gdkvm_scan_fwd, and the results agree with them to the last few ulp of the norms' summation order. */
int gdkvm_scan_prep_normed(const void* q, const void* k, const void* v, const float* beta, const float* norms,
                           void* workspace, size_t workspace_bytes,
                           int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype, int rule, int flags, void* stream);
int gdkvm_scan_fwd_normed(const void* q, const void* k, const void* v, const float* alpha, const float* beta, const float* norms,
                          const float* s_in, void* r_out, float* s_out, void* workspace, size_t workspace_bytes,
                          int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype, int rule, int flags, void* stream);

/* SURVEY.md §8(f) row n3.  The effect of a block of frames on the state is affine, S_out = Phi S_in + S_loc, with the
 * state-transition matrix Phi = prod_t alpha_t (I - Kn_t^T Wt_t) ("Linear Key-Value Association defines frame-to-frame
 * causal relations as the state transition matrix", /root/reference/website/src/content/homepage/en.json:20).
 * gdkvm_scan_transition returns Phi [B,Hh,Dk,Dk] (fp32) of the T frames a preceding gdkvm_scan_prep call prepared in
 * `workspace` (the same recurrence kernel, started from S = I with a zero write term); S_loc is gdkvm_scan_apply with
 * s_in = NULL (r_out may be NULL when only states are wanted).  Segments of a long clip -- or of a clip sharded over GPUs
 * in time -- can then be scanned independently and stitched with one small exchange. */
int gdkvm_scan_transition(const void* q, const float* alpha, float* phi_out, const void* workspace, size_t workspace_bytes,
                          int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype, int flags, void* stream);
/* Row n3, the sequential stitch of a time-segmented scan: phi [B,S,Hh,Dk,Dk] and s_loc [B,S,Hh,Dk,Dv] are the transition matrix
 * and the zero-start end state of each of S consecutive segments (gdkvm_scan_transition / gdkvm_scan_apply on the clip viewed as
 * B*S clips of T/S frames); starts [B,S,Hh,Dk,Dv] receives the state every segment really starts from,
 *   starts[:,0] = s_in (zero if NULL),  starts[:,c+1] = phi[:,c] starts[:,c] + s_loc[:,c],
 * and s_end (optional) the state after the last segment.  All fp32; exact fp32 arithmetic. */
int gdkvm_scan_stitch(const float* phi, const float* s_loc, const float* s_in, float* starts, float* s_end,
                      int B, int S, int Hh, int Dk, int Dv, void* stream);

/* Row n3 as one call: gdkvm_scan_fwd with the time axis cut into `segments` equal pieces that run concurrently (prep of the clip
 * viewed as B*segments clips, gdkvm_scan_transition + a read-out-free gdkvm_scan_apply per segment, gdkvm_scan_stitch, then
 * gdkvm_scan_apply from the true start states).  For long clips on few clips / heads / columns, where the serial recurrence leaves
 * CUs idle: 2x512 frames, Dv = 256 (32 serial workgroups) 269 us with 16 segments against 346 us (round 3).  segments must divide T;
 * segments == 0 chooses by shape (gdkvm_scan_segments returns the choice: a power of two >= 4, or 1 = plain gdkvm_scan_fwd).
 * Equal to gdkvm_scan_fwd up to fp32 re-association through Phi -- NOT bit-identical, which is why gdkvm_scan_fwd, whose contract
 * is bit-identity under chunked calls, never takes this path by itself.  No s_hist (inference).  workspace:
 * gdkvm_scan_segmented_workspace_bytes with the same `segments` argument. */
int gdkvm_scan_segments(int B, int T, int Hh, int Dv, int segments);
size_t gdkvm_scan_segmented_workspace_bytes(int B, int T, int Hh, int N, int Dk, int Dv, int segments);
int gdkvm_scan_fwd_segmented(const void* q, const void* k, const void* v, const float* alpha, const float* beta,
                             const float* s_in, void* r_out, float* s_out, void* workspace, size_t workspace_bytes,
                             int B, int T, int Hh, int N, int Dk, int Dv, int segments,
                             int io_dtype, int rule, int flags, void* stream);

/* SURVEY.md A.1, the `normalizer` flag of the LKVA read: besides S the memory carries z [B, Hh, Dk] (fp32) -- "the same recurrence on
 * v == 1", i.e. the state column of a value channel that is 1 for every token -- and the read-out of token n of frame t is
 *     R_t[n, :] = (Qn_t[n] S_{t-1}) / (|Qn_t[n] . z_{t-1}| + eps).
 * Everything else as gdkvm_scan_fwd (Dk == 64, inference only: no s_hist): z_in / s_in may be NULL (zeros), z_out / s_out may be NULL;
 * a clip processed as consecutive calls with (S, z) carried is bit-identical to one call.  Implemented as the library's own scan on
 * Dv + 16 value channels (channel Dv holds the ones) with the division on the way out: csrc/gdr_normalizer.hip.  0 < eps < 1
 * (SPEC-v0 default 1e-6).  Names: "Linear Key-Value Association" at /root/reference/README.md:20. */
size_t gdkvm_scan_normalizer_workspace_bytes(int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype);
int gdkvm_scan_fwd_normalizer(const void* q, const void* k, const void* v, const float* alpha, const float* beta,
                              const float* s_in, const float* z_in, void* r_out, float* s_out, float* z_out,
                              void* workspace, size_t workspace_bytes,
                              int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype, int rule, int flags, float eps, void* stream);

/* The per-frame `step` mode with mask feedback: when the value written for frame t depends on the mask
 * predicted for frame t, the frame loop is read -> KPFF -> decoder -> mask -> write, one frame of every clip at a time.
 *   gdkvm_lkva_read       row a1 on its own: r_out [B, N, Hh, Dv] = Qn S for ONE frame per clip, q [B, N, Hh, Dk] (io_dtype), the state
 *                         s [B, Hh, Dk, Dv] fp32 given as a tensor.  flags: GDKVM_FLAG_NORMALIZE_QK as in gdkvm_scan_fwd; norms
 *                         (may be NULL) = gdkvm_proj_gates' [B*N, Hh, 2] inverse norms (entry 1 is the query's).  Plain fp32 fmaf
 *                         chains in key-channel order: deterministic.  Dk == 64.
 *   gdkvm_mask_embed_add  v [BT, h*w, C] (io_dtype) += w_embed[c] * m, m = the mean over the token's adaptive-average-pool cell
 *                         (PyTorch's adaptive_avg_pool2d cells) of the foreground indicator of mask [BT, H, W] (uint8: class != 0;
 *                         255 = unlabelled counts as background): the first-frame-mask embedding of the module applied to a predicted
 *                         mask.  The write itself is gdkvm_scan_fwd with T == 1.
 *   gdkvm_mask_embed_wgrad  the weight gradient of gdkvm_mask_embed_add (training in the step mode): d_w[c] (fp32 [C]) = the sum over
 *                         the F*h*w token rows of m(f, n) * d_v[f, n, c], m the pooled indicator of mask [F, H, W] exactly as
 *                         gdkvm_mask_embed_add computes it, d_v [F, h*w, C] (io_dtype; C a multiple of 8 for bf16, of 4 for f32, at most
 *                         256 16-byte pieces).  fp32 accumulation; per-block partials in `workspace`
 *                         (gdkvm_mask_embed_wgrad_workspace_bytes) added in a fixed order: deterministic, no float atomics.
 *                         F == 0 writes zeros. */
int gdkvm_lkva_read(const void* q, const float* norms, const float* s, void* r_out,
                    int B, int N, int Hh, int Dk, int Dv, int io_dtype, int flags, void* stream);
int gdkvm_mask_embed_add(const uint8_t* mask, const float* w_embed, void* v, int BT, int H, int W, int h, int w, int C,
                         int io_dtype, void* stream);
size_t gdkvm_mask_embed_wgrad_workspace_bytes(int F, int h, int w, int C);
int gdkvm_mask_embed_wgrad(const uint8_t* mask, const void* d_v, float* d_w, void* workspace, size_t workspace_bytes,
                           int F, int H, int W, int h, int w, int C, int io_dtype, void* stream);

/* Row a7: backward of gdkvm_scan_fwd.  Inputs: the forward's inputs, its s_hist, its workspace exactly as the
 * forward left it, the gradients d_r [B,T,N,Hh,Dv] (io_dtype) and d_s_out [B,Hh,Dk,Dv] (fp32, may be NULL = 0).
 * Outputs: d_q, d_k [B,T,N,Hh,Dk], d_v [B,T,N,Hh,Dv] (io_dtype), d_alpha [B,T,Hh], d_beta [B,T,N,Hh] (fp32; with
 * GDKVM_FLAG_GATE_LOGITS they are gradients w.r.t. the logits), d_s_in [B,Hh,Dk,Dv] (fp32, may be NULL).
 * bwd_workspace (gdkvm_scan_bwd_workspace_bytes) holds the per-frame state gradients.  Supported: N <= 64 (any N: gdkvm_scan_train_fwd /
 * gdkvm_scan_train_bwd below). */
size_t gdkvm_scan_bwd_workspace_bytes(int B, int T, int Hh, int N, int Dk, int Dv);
int gdkvm_scan_bwd(const void* q, const void* k, const void* v, const float* alpha, const float* beta,
                   const float* s_hist, const void* fwd_workspace, size_t fwd_workspace_bytes,
                   const void* d_r, const float* d_s_out,
                   void* d_q, void* d_k, void* d_v, float* d_alpha, float* d_beta, float* d_s_in,
                   void* bwd_workspace, size_t bwd_workspace_bytes,
                   int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype, int rule, int flags, void* stream);

/* Row a7 for frames of ANY token count in two calls.  gdkvm_scan_train_fwd is gdkvm_scan_fwd that keeps what the backward needs
 * in ONE opaque workspace (gdkvm_scan_train_workspace_bytes: state history, WY factors, and for N > 64 the frame re-cut into
 * ceil(N/64) pseudo-frames of 64 tokens -- the first with the frame's gate, the others with gate 1, padding tokens with beta = 0 --
 * on which the state recurrence runs; the read-out of all N tokens uses the state before the frame).  gdkvm_scan_train_bwd takes
 * the same inputs, that workspace untouched, d_r and d_s_out (may be NULL = 0), and returns the gradients of gdkvm_scan_bwd.
 * N <= 64 is exactly gdkvm_scan_fwd (s_hist inside the workspace) + gdkvm_scan_bwd; N > 64 composes gdkvm_scan_fwd without a
 * read-out, gdkvm_readout_fwd / _bwd and gdkvm_scan_state_bwd below.  GDKVM_RULE_DELTA_PARALLEL: N <= 64 only (its chunks
 * combine additively, not in sequence).  Supported: Dk == 64, or 72 <= Dk <= 256 in multiples of 8; Dv % 16 == 0, 1 <= N <= 4096.
 * Wide keys (Dk > 64; B * Hh <= 65535) train on their own pair at every N: the forward is gdkvm_scan_fwd's wide-key kernel (its R and
 * S_T bit for bit) writing the state before every frame beside, the backward the exact gradient of that fp32 recurrence
 * (csrc/gdr_general_bwd.hip: a reverse walk per 16-column state slice, per-slice partials summed in a fixed order -- deterministic).
 * Its workspace, every term rounded up to 256 bytes, with FH = B*T*Hh frame-heads and NS = Dv/16 slices:
 *     4 * (FH*Dk*Dv  +  B*Hh*Dv*N  +  2*NS*FH*N*Dk  +  NS*FH*N  +  NS*FH)  +  256 bytes. */
size_t gdkvm_scan_train_workspace_bytes(int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype);
int gdkvm_scan_train_fwd(const void* q, const void* k, const void* v, const float* alpha, const float* beta, const float* s_in,
                         void* r_out, float* s_out, void* train_workspace, size_t train_workspace_bytes,
                         int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype, int rule, int flags, void* stream);
int gdkvm_scan_train_bwd(const void* q, const void* k, const void* v, const float* alpha, const float* beta,
                         const void* d_r, const float* d_s_out,
                         void* d_q, void* d_k, void* d_v, float* d_alpha, float* d_beta, float* d_s_in,
                         void* train_workspace, size_t train_workspace_bytes,
                         int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype, int rule, int flags, void* stream);

/* Row a7 for frames of more than 64 tokens (and any caller that does its own read-out): the backward of the STATE recurrence
 * alone.  No q / d_r / d_q; instead d_hist [B,T,Hh,Dk,Dv] fp32 (may be NULL) is the gradient with respect to the state before
 * every frame (what a read-out R_t = f(S_{t-1}) done outside sends back), which enters the reverse recurrence as its additive
 * term.  gdkvm_amd/ops.py::scan uses it with every 64-token chunk of a frame as a pseudo-frame (gate 1 after the first, padding
 * tokens with beta = 0) and the read-out as a batched matmul on the saved states.  Same workspaces as gdkvm_scan_bwd. */
int gdkvm_scan_state_bwd(const void* k, const void* v, const float* alpha, const float* beta,
                         const float* s_hist, const void* fwd_workspace, size_t fwd_workspace_bytes,
                         const float* d_hist, const float* d_s_out,
                         void* d_k, void* d_v, float* d_alpha, float* d_beta, float* d_s_in,
                         void* bwd_workspace, size_t bwd_workspace_bytes,
                         int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype, int rule, int flags, void* stream);

/* Rows a1 / a7 for training on frames of more than 64 tokens: the LKVA read-out R_t = diag(qinv) Q_t S_{t-1} of all N tokens of
 * a frame from a saved state history, and its backward.  s_hist [B, T*hist_stride, Hh, Dk, Dv] fp32 is the history
 * gdkvm_scan_fwd saves over the 64-token pseudo-frames of gdkvm_amd/ops.py::_scan_chunked (hist_stride of them per frame): frame
 * t reads the state at index t*hist_stride.  q, r_out, d_r, d_q [B,T,N,Hh,*] in io_dtype.  gdkvm_readout_bwd writes
 * d_q and the state gradients dS = Qn^T dR into d_hist at the same indices t*hist_stride (the caller zero-fills the rest and
 * hands d_hist to gdkvm_scan_state_bwd).  GDKVM_FLAG_NORMALIZE_QK as in gdkvm_scan_fwd.  Any N >= 0; Dk == 64; exact fp32. */
int gdkvm_readout_fwd(const void* q, const float* s_hist, void* r_out, int B, int T, int Hh, int N, int Dk, int Dv,
                      int hist_stride, int io_dtype, int flags, void* stream);
int gdkvm_readout_bwd(const void* q, const float* s_hist, const void* d_r, void* d_q, float* d_hist,
                      int B, int T, int Hh, int N, int Dk, int Dv, int hist_stride, int io_dtype, int flags, void* stream);

/* Row a7: the plain products of the training backward (KPFF's dX / dW products, the 1x1 projections and their gradients),
 * hand-written like the rest of the path.  Row-major operands in io_dtype, fp32 accumulation.
 *   gdkvm_gemm_nt:  C[M,N] = A[M,K] B[N,K]^T (+ bias[N], fp32, may be NULL), C in io_dtype.  K % 32 == 0 (bf16) / % 16 (fp32).
 *   gdkvm_gemm_tn:  C[K1,N] (fp32) = A[M,K1]^T B[M,N]: the reduction over the M rows (the tokens of a batch) is split over
 *                   workgroups into fp32 partial tiles in `workspace` (gdkvm_gemm_tn_workspace_bytes) and summed in a fixed
 *                   order (deterministic).  K1, N multiples of 8 (bf16) / 4 (fp32); any M >= 0. */
int gdkvm_gemm_nt(const void* a, const void* b, const float* bias, void* c, int M, int N, int K, int io_dtype, void* stream);
size_t gdkvm_gemm_tn_workspace_bytes(int M, int K1, int N);
int gdkvm_gemm_tn(const void* a, const void* b, float* c, void* workspace, size_t workspace_bytes,
                  int M, int K1, int N, int io_dtype, void* stream);
/* The same product with the column sums of A as a second result: colsum[K1] (fp32) = sum over the M rows of A[m][k1] -- the bias
 * gradient of y = x W^T + b when A = dY -- from one more MFMA per step against a fragment of ones, summed over the row splits in the same
 * fixed order (workspace: gdkvm_gemm_tn_colsum_workspace_bytes). */
size_t gdkvm_gemm_tn_colsum_workspace_bytes(int M, int K1, int N);
int gdkvm_gemm_tn_colsum(const void* a, const void* b, float* c, float* colsum, void* workspace, size_t workspace_bytes,
                         int M, int K1, int N, int io_dtype, void* stream);

/* Row a4: Key-Pixel Feature Fusion ("fuses the local key feature, the global key feature with the pixel
 * feature", /root/reference/website/src/content/homepage/en.json:20; "multiple scales", README.md:20).
 *   local [BT,N,Ck]  global [BT,N,Cv]  pixel [BT,N,Cp]  out [BT,N,Cp]   (io_dtype), N = h*w
 *   wa [2Cp, Cp+Ck+Cv]  ba [2Cp]  wl [Cp,Ck]  wg [Cp,Cv]                 (fp32)
 *   Gms = mean_{s in 1,2,4} cellmean_s(global);  g = sigmoid([P;L;Gms] wa^T + ba) = (g_l | g_g)
 *   out = P + g_l * (L wl^T) + g_g * (Gms wg^T)
 * Arithmetic: io_dtype f32 with channel counts that are multiples of 32 and a workspace -> operands as two bf16 terms
 * (16 significant bits, the fp32 exponent range), three bf16 MFMAs per product, fp32 accumulation / pooling / residual /
 * epilogue: about 2^-16 relative per product (3e-5 absolute against the fp64 oracle at unit-variance features).  io_dtype f32
 * otherwise -- other channel counts, or workspace == NULL, which is how a caller asks for it -> exact fp32 MFMA (3x slower).
 * io_dtype bf16 with channel counts that are multiples of 32 -> bf16 MFMA with fp32 accumulation (weights and the pooled
 * feature are rounded to bf16, i.e. bf16-autocast accuracy); other bf16 shapes use the exact fp32 arm.  `workspace`
 * (gdkvm_kpff_workspace_bytes) holds the bf16 copies of the weights (high and low terms for f32), rebuilt on every call; the
 * exact arm packs nothing, and for its channel counts the size is the 16-byte floor in both I/O types.  A workspace of
 * fewer bytes than the size entry returns is refused (GDKVM_ERR_WORKSPACE) by every arm that uses it.
 * Supported: Ck, Cv, Cp multiples of 16; h*w <= 4096 (grids wider than 16 columns are processed as 4-row x 16-column tiles). */
size_t gdkvm_kpff_workspace_bytes(int Ck, int Cv, int Cp, int io_dtype);
int gdkvm_kpff_fwd(const void* local, const void* global, const void* pixel,
                   const float* wa, const float* ba, const float* wl, const float* wg, void* out,
                   void* workspace, size_t workspace_bytes,
                   int BT, int Ck, int Cv, int Cp, int h, int w, int io_dtype, void* stream);

/* gdkvm_kpff_fwd with the weight re-pack skipped: `packed_workspace` must be the workspace a previous gdkvm_kpff_fwd
 * call filled from the SAME (unchanged) wa / wl / wg -- the inference case. */
int gdkvm_kpff_fwd_packed(const void* local, const void* global, const void* pixel,
                          const float* wa, const float* ba, const float* wl, const float* wg, void* out,
                          void* packed_workspace, size_t workspace_bytes,
                          int BT, int Ck, int Cv, int Cp, int h, int w, int io_dtype, void* stream);

/* Row a7 for KPFF.  The training forward also stores what the backward needs (all [M = BT*N, .] in io_dtype): the
 * gates after the sigmoid [M,2Cp], L wl^T [M,Cp], Gms wg^T [M,Cp] and the pooled feature Gms [M,Cv].  The backward is
 *   gdkvm_kpff_bwd_pre   d_z = (d_out*Lp*g_l(1-g_l) | d_out*Gp*g_g(1-g_g)), d_lp = d_out*g_l, d_gp = d_out*g_g
 *   six plain GEMMs      d_x = d_z wa, d_l_add = d_lp wl, d_g_add = d_gp wg, d_wa = d_z^T [P;L;Gms], d_wl = d_lp^T L,
 *                        d_wg = d_gp^T Gms  (and d_ba = column sums of d_z) -- on the caller's side: gdkvm_gemm_nt for the
 *                        products against weights, gdkvm_gemm_tn (split over the token rows, deterministic) for the weight gradients
 *   gdkvm_kpff_bwd_post  d_pixel = d_out + d_x[:, :Cp], d_local = d_x[:, Cp:Cp+Ck] + d_l_add,
 *                        d_global = pool(d_x[:, Cp+Ck:] + d_g_add)   (the multi-scale pooling operator is symmetric) */
int gdkvm_kpff_fwd_train(const void* local, const void* global, const void* pixel,
                         const float* wa, const float* ba, const float* wl, const float* wg, void* out,
                         void* save_gates, void* save_lp, void* save_gp, void* save_gms,
                         void* workspace, size_t workspace_bytes,
                         int BT, int Ck, int Cv, int Cp, int h, int w, int io_dtype, void* stream);
int gdkvm_kpff_bwd_pre(const void* d_out, const void* gates, const void* lp, const void* gp,
                       void* d_z, void* d_lp, void* d_gp, int BT, int N, int Cp, int io_dtype, void* stream);
int gdkvm_kpff_bwd_post(const void* d_out, const void* d_x, const void* d_l_add, const void* d_g_add,
                        void* d_pixel, void* d_local, void* d_global,
                        int BT, int Ck, int Cv, int Cp, int h, int w, int io_dtype, void* stream);

/* Row a6: mask = argmax_c logits (ties -> lowest class index); optional integer Dice counts.
 *   logits [BT, ncls, H, W] (io_dtype)   target [BT,H,W] u8 or NULL   mask [BT,H,W] u8
 *   counts [BT, ncls, 3] int32 = { |mask==c & target==c|, |mask==c|, |target==c| }  (zeroed by the callee;
 *   required iff target != NULL). */
int gdkvm_argmax_dice(const void* logits, const uint8_t* target, uint8_t* mask, int32_t* counts,
                      int BT, int ncls, int H, int W, int io_dtype, void* stream);

/* Row a6, fused with the decoder's last step: logits [BT, ncls, hl, wl] at low resolution are upsampled bilinearly
 * (align_corners = false, PyTorch's formula, fp32 without fused multiply-add) to H x W inside the kernel and reduced to
 * the argmax mask / Dice counts directly; the full-resolution logits are never materialised. */
int gdkvm_upsample_argmax_dice(const void* logits, const uint8_t* target, uint8_t* mask, int32_t* counts,
                               int BT, int ncls, int hl, int wl, int H, int W, int io_dtype, void* stream);

/* ... and with the decoder's 1x1 head folded in as well: x [BT, hl, wl, C] is the stride-4 feature (NHWC, io_dtype), w [ncls, C] and
 * b [ncls] (fp32) the head; every block computes the class planes of the low-resolution rows it needs into LDS, with
 * gdkvm_head_logits' arithmetic and rounding -- masks and counts are bit-identical to gdkvm_head_logits followed by
 * gdkvm_upsample_argmax_dice, and the class planes never reach memory.  C/8 (bf16) or C/4 (f32) a power of two <= 64, ncls <= it. */
int gdkvm_head_upsample_argmax_dice(const void* x, const float* w, const float* b, const uint8_t* target, uint8_t* mask,
                                    int32_t* counts, int BT, int C, int ncls, int hl, int wl, int H, int W, int io_dtype, void* stream);

/* SURVEY.md §8(f) row n1 (inference build only): fused pointwise epilogue for the unchanged MIOpen convolutions,
 * y[r, c] = act(x[r, c] + bias[c] (+ residual[r, c])) over an NHWC tensor viewed as [rows, C]; relu != 0 applies ReLU.
 * x, residual, y in io_dtype (y may alias x), bias fp32.  C must be a multiple of 4 (f32) / 8 (bf16). */
int gdkvm_bias_act(const void* x, const float* bias, const void* residual, void* y,
                   size_t rows, int C, int relu, int io_dtype, void* stream);

/* Row n1, the decoder's head: 1x1 convolution + bias from an NHWC feature x [N, H, W, C] to NCHW class planes out [N, classes, H, W]
 * (io_dtype; weight fp32 [classes, C], bias fp32 [classes]; classes <= C/8 (bf16) / C/4 (f32)) -- the layout and dtype
 * gdkvm_upsample_argmax_dice reads; one pass instead of convolution + bias add + layout copy. */
int gdkvm_head_logits(const void* x, const float* w, const float* b, void* out, int N, int H, int W, int C, int classes,
                      int io_dtype, void* stream);
/* Training: the head's backward in one pass.  dz [N, classes, H, W] (io dtype, NCHW planes as gdkvm_seg_loss_bwd writes them), x the feature
 * gdkvm_head_logits read, w fp32 [classes, C] -> dx [N, H, W, C] (io dtype), dw fp32 [classes, C], db fp32 [classes]; per-workgroup partial
 * sums in `workspace` (gdkvm_head_bwd_workspace_bytes) added in index order: deterministic.  classes <= min(C/8 (C/4 for fp32), 8). */
size_t gdkvm_head_bwd_workspace_bytes(int C, int ncls);
int gdkvm_head_bwd(const void* x, const void* dz, const float* w, void* dx, float* dw, float* db, void* workspace, size_t workspace_bytes,
                   int N, int H, int W, int C, int ncls, int io_dtype, void* stream);

/* Row n4, the key / query / value projections in one pass over the token rows x [rows, K] (bf16):
 *   [out0 | out1 | out2][row, :] = x[row, :] W^T + bias,  W [w0 + w1 + w2, K] -- three contiguous outputs [rows, w0], [rows, w1],
 *   [rows, w2] (w1, w2 may be 0), widths multiples of 16, K a multiple of 32 up to 512, fp32 bias [w0 + w1 + w2].
 * wpack is W in MFMA fragment order, bf16: element ((ot * K/32 + ks) * 64 + lane) * 8 + j = W[16 ot + (lane & 15)][32 ks + 8 (lane >> 4) + j]
 * (gdkvm_amd/ops.py::pack_rows_weight builds it).  fp32 accumulation, one rounding. */
int gdkvm_proj_rows(const void* x, const void* wpack, const float* bias, void* out0, void* out1, void* out2,
                    long long rows, int K, int w0, int w1, int w2, int io_dtype, void* stream);

/* Row n4, the gates of the memory path in one pass over the stride-16 pixel feature p [frames, N, Cp] (io_dtype):
 *   beta_logit [frames, N, Hh]  = <p[f, n, :], w_gate[h, :]> + b_gate[h]           (per token; what the gate 1x1 projection computes)
 *   alpha_logit [frames, Hh]    = <mean_n p[f, n, :], w_decay[h, :]> + b_decay[h]  (per frame; token mean -> decay projection)
 * both fp32 (the dtype gdkvm_scan_prep / gdkvm_scan_apply read), weights fp32 [Hh, Cp], fp32 accumulation throughout. */
int gdkvm_gate_logits(const void* p, const float* w_gate, const float* b_gate, const float* w_decay, const float* b_decay,
                      float* beta, float* alpha, int frames, int N, int Cp, int Hh, int io_dtype, void* stream);

/* Row n4: gdkvm_proj_rows + gdkvm_gate_logits + the inverse norms of the key / query rows in ONE launch over the stride-16 pixel
 * feature x [frames * N, K] (bf16): out_k, out_q [rows, Hh*Dk], out_v [rows, Hh*Dv] (bf16; wpack / bias as for gdkvm_proj_rows with
 * the key, query and value weights stacked in that order), beta [rows, Hh] and alpha [frames, Hh] (fp32 logits, fp32 gate weights
 * [Hh, K]), norms [rows, Hh, 2] (fp32: what gdkvm_scan_fwd_normed takes).  The tokens are read from HBM once; deterministic (no
 * atomics).  K a power of two times 8 up to 512. */
int gdkvm_proj_gates(const void* x, const void* wpack, const float* bias, void* out_k, void* out_q, void* out_v,
                     const float* w_gate, const float* b_gate, const float* w_decay, const float* b_decay,
                     float* beta, float* alpha, float* norms,
                     int frames, int N, int K, int Hh, int Dk, int Dv, int io_dtype, void* stream);

/* Row n1 (inference build): 3x3 / stride 1 / pad 1 convolution with the folded-BatchNorm bias, the residual add and the ReLU
 * in its epilogue,  y = act(conv(x, w) + bias[k] (+ residual)),  x [N, H, W, C] (NHWC), w [K, 3, 3, C] (channels_last weights),
 * y / residual [N, H, W, K], bias fp32 [K]; bf16 only.  The fp32 accumulator is rounded ONCE (after the epilogue).  Both kernels
 * are hand-written: kernel 4 = 64 -> 64 channels (conv3x3_c64.hip: LDS halo band, weights resident in registers), kernel 5 = C a
 * multiple of 64, K of 16, rows of <= 64 pixels (conv3x3_tile.hip: 64-channel LDS chunks, weights streamed); kernel 0 picks by
 * shape; 6, 7, 8 pin kernel 5's wave grid (4 channel groups x 1 tile, 4 x 2, 2 x 2: tuning; 5 picks by K), 10 / 11 = the 4 x 2 / 2 x 2
 * grids on four waves with half-size pixel tiles, two workgroups per CU (what 0 / 5 pick: 10 for K a multiple of 128, else 11; same
 * sums, same bits).
 * kernel 9 | GDKVM_CONV_PACKED_WEIGHTS = the general implicit-GEMM kernel (conv_igemm.hip): any R x S, stride and padding, rows of
 * any width -- the strided 3x3 layers, the 1x1 downsamples, 3x3 / 1 / 1 on maps wider than 64 pixels; C a multiple of 32, K of 128,
 * w the gdkvm_conv_igemm_pack_weights copy of the [K, R, S, C] weights.  Shapes none of the three serves (odd channel counts)
 * return GDKVM_ERR_SHAPE: those stay on the framework convolution followed by gdkvm_bias_act.
 * kernel | GDKVM_CONV_PACKED_WEIGHTS: w is the fragment-ordered copy gdkvm_conv3x3_pack_weights made of the
 * [K, 3, 3, C] weights (same size) -- each 1 KiB weight fragment is then one contiguous read; same result bit for bit. */
enum { GDKVM_CONV_PACKED_WEIGHTS = 32 };
int gdkvm_conv3x3_pack_weights(const void* w, void* packed, int K, int C, int io_dtype, void* stream);
/* kernel 9's pack: w [K, R, S, C] bf16 -> the same bytes in MFMA-fragment order (K a multiple of 16, C of 32). */
int gdkvm_conv_igemm_pack_weights(const void* w, void* packed, int K, int C, int R, int S, int io_dtype, void* stream);
/* The pack of the same layer's DATA-GRADIENT convolution, from the forward weights w [K, 3, 3, C]:  dx = conv3x3(dy, w'),
 * w'[c][ty][tx][k] = w[k][2 - ty][2 - tx][c] -- K input channels (a multiple of 64), C output channels (of 16).  Use it as
 * gdkvm_conv_bias_act(dy, packed, zero bias, NULL, dx, N, K, H, W, C, 3, 3, 1, 1, 0, kernel | GDKVM_CONV_PACKED_WEIGHTS, ...). */
int gdkvm_conv3x3_pack_weights_dgrad(const void* w, void* packed, int K, int C, int io_dtype, void* stream);
/* Training: both packs of up to GDKVM_PACK_MAX_LAYERS 3x3 layers in ONE launch, straight from the fp32 master weights (the per-layer
 * sequence "cast to bf16, gdkvm_conv3x3_pack_weights, gdkvm_conv3x3_pack_weights_dgrad" is three launches of ~5 us per layer and step).
 * w[i]: fp32 [K_i, C_i, 3, 3] with element strides strides[4i .. 4i+3] = (k, c, r, s) -- any memory format; packed_fwd[i] /
 * packed_dgrad[i]: 18 K_i C_i bytes each, the copies the two calls above produce from the bf16-rounded weights, bit for bit.
 * K_i, C_i multiples of 64.  The five arrays are HOST arrays. */
#define GDKVM_PACK_MAX_LAYERS 24
int gdkvm_conv3x3_pack_weights_train(int nlayers, const void* const* w, void* const* packed_fwd, void* const* packed_dgrad,
                                     const int* K, const int* C, const long long* strides, void* stream);
/* Weight gradient of the same layers (training):  dw [K, C, 3, 3] fp32 = sum over pixels dy[n,y,x,k] * x[n,y+ty-1,x+tx-1,c]  for
 * NHWC bf16 x [N,H,W,C] and dy [N,H,W,K]; C and K multiples of 64, rows of <= 64 pixels.  Deterministic (per-workgroup partial
 * blocks in the workspace, added in a fixed order).  workspace: gdkvm_conv3x3_wgrad_workspace_bytes. */
size_t gdkvm_conv3x3_wgrad_workspace_bytes(int N, int C, int H, int W, int K);
int gdkvm_conv3x3_wgrad(const void* x, const void* dy, float* dw, void* workspace, size_t workspace_bytes,
                        int N, int C, int H, int W, int K, int io_dtype, void* stream);
/* The same gradient written as [K, 3, 3, C] -- the memory order of a channels_last [K, C, 3, 3] parameter (the framework re-lays a
 * contiguous gradient out with one copy per layer and step). */
int gdkvm_conv3x3_wgrad_krsc(const void* x, const void* dy, float* dw, void* workspace, size_t workspace_bytes,
                        int N, int C, int H, int W, int K, int io_dtype, void* stream);
int gdkvm_conv_bias_act(const void* x, const void* w, const float* bias, const void* residual, void* y,
                        int N, int C, int H, int W, int K, int R, int S, int stride, int pad, int relu, int kernel,
                        int io_dtype, void* stream);
/* A residual block's first convolution and its 1x1 downsample branch in ONE launch of kernel 9:  y = act(conv_RxS(x, w) + bias)  and
 * y_down = conv_1x1(x, w_down) (+ bias_down, may be NULL), both with the same stride and K output channels -- the 1x1's input pixel
 * is the centre of the R x S window (R = S odd, pad = R / 2).  w and w_down are gdkvm_conv_igemm_pack_weights copies of the
 * [K, R, S, C] and [K, 1, 1, C] weights; C a multiple of 32, K of 128; bf16. */
int gdkvm_conv_down_bias_act(const void* x, const void* w, const float* bias, void* y, int relu,
                             const void* w_down, const float* bias_down, void* y_down,
                             int N, int C, int H, int W, int K, int R, int S, int stride, int pad, int io_dtype, void* stream);
/* Training form of the same pair (a residual block's 3x3 / stride-2 / pad-1 convolution w [K, C, 3, 3] and its 1x1 / stride-2 branch
 * w_down [K, C, 1, 1], both without bias), forward and backward on hand-written kernels, deterministic:
 *   gdkvm_conv_s2_pack_train   ONE launch from the fp32 master weights (element strides (k, c, r, s) resp. (k, c): any memory format) to
 *                              packed_fwd / packed_fwd_down (what gdkvm_conv_igemm_pack_weights makes of the bf16-rounded weights: feed
 *                              them to gdkvm_conv_down_bias_act, stride 2, pad 1) and packed_dgrad (gdkvm_conv_s2_dgrad_pack_bytes).
 *                              w_down may be NULL (no branch).  K a multiple of 128, C of 64.
 *   gdkvm_conv_s2_dgrad        dx [N, H, W, C] = the gradient of x from dy [N, Ho, Wo, K] (and dy_down, same shape, or NULL), Ho = (H-1)/2+1:
 *                              every input pixel sums exactly the taps that reach it (four parity classes, no products with zeros), the
 *                              branch's gradient inside the same accumulation, one rounding to bf16.  with_down: was packed_dgrad made WITH the
 *                              1x1 branch (gdkvm_conv_s2_pack_train with w_down != NULL)?  The class offsets inside the pack follow
 *                              this, not dy_down: with_down = 1 and dy_down = NULL is a zero branch gradient; dy_down with
 *                              with_down = 0 is GDKVM_ERR_ARG.
 *   gdkvm_conv_wgrad_strided   dw[k sk + c sc + r sr + s ss] (fp32, element strides: the parameter's own memory format) =
 *                              sum_{n, yo, xo} dy[n, yo, xo, k] x[n, yo stride - pad + r, xo stride - pad + s, c]  for ANY R x S / stride /
 *                              pad; C a multiple of 64, K of 8; the rows of the batch are summed in fixed-order splits (no atomics).
 * (The reference's own recipe is a multi-process DDP launch, /root/reference/website/src/pages/[lang]/reprod/index.astro:238-249: with
 * every gradient of the step deterministic, the DDP-wrapped step at world size 1 is bit-equal to the bare one.) */
size_t gdkvm_conv_s2_dgrad_pack_bytes(int C, int K, int with_down);
int gdkvm_conv_s2_pack_train(const float* w, const long long* w_strides, const float* w_down, const long long* w_down_strides,
                             void* packed_fwd, void* packed_fwd_down, void* packed_dgrad, int K, int C, void* stream);
int gdkvm_conv_s2_dgrad(const void* dy, const void* dy_down, const void* packed_dgrad, void* dx,
                        int N, int C, int H, int W, int K, int with_down, int io_dtype, void* stream);
size_t gdkvm_conv_wgrad_strided_workspace_bytes(int N, int C, int H, int W, int K, int R, int S, int stride, int pad);
int gdkvm_conv_wgrad_strided(const void* x, const void* dy, float* dw, long long sk, long long sc, long long sr, long long ss,
                             void* workspace, size_t workspace_bytes,
                             int N, int C, int H, int W, int K, int R, int S, int stride, int pad, int io_dtype, void* stream);
/* The same 3x3 / 1 / 1 convolution over the channel concatenation [x1 (C1 channels) ; x2 (C2)] of two NHWC tensors, which is
 * never materialised -- the decoder's  conv(cat(upsample(feature), skip))  without the concatenated copy.  C1, C2 multiples of
 * 64, K of 16, rows of <= 64 pixels; w [K, 3, 3, C1 + C2] or its packed copy (kernel | GDKVM_CONV_PACKED_WEIGHTS); kernel 0 or
 * 5..8, 10, 11.  Bit-identical to gdkvm_conv_bias_act on the concatenated tensor. */
int gdkvm_conv_cat_bias_act(const void* x1, const void* x2, const void* w, const float* bias, const void* residual, void* y,
                            int N, int C1, int C2, int H, int W, int K, int relu, int kernel, int io_dtype, void* stream);
/* The same with x1 = the exact-2x bilinear enlargement (align_corners = false) of lo [N, H/2, W/2, C1], which is never materialised
 * either: the kernel builds it in its LDS band from the low-resolution rows.  H, W (both even, W <= 64) are the OUTPUT map; C1, C2
 * multiples of 64, K of 16; w = the gdkvm_conv3x3_pack_weights copy of [K, 3, 3, C1 + C2] and kernel = GDKVM_CONV_PACKED_WEIGHTS
 * (anything else: GDKVM_ERR_ARG).  Bit-identical to gdkvm_conv_cat_bias_act on gdkvm_upsample_cat(lo, NULL) and x2. */
int gdkvm_conv_upcat_bias_act(const void* lo, const void* x2, const void* w, const float* bias, const void* residual, void* y,
                              int N, int C1, int C2, int H, int W, int K, int relu, int kernel, int io_dtype, void* stream);

/* Row n1, the stem: bias + ReLU + 3x3 / stride 2 / pad 1 max-pool in one pass over the NHWC conv output
 * x [N, H, W, C] -> y [N, (H-1)/2+1, (W-1)/2+1, C]:  y = relu(max_window(x) + bias)  (== max_window(relu(x + bias)), the
 * rounding of x + b being monotonic).  The full-resolution activation is read once and never written back.  x may be the
 * top-left H x W corner of a larger stored image of x_rows x x_cols pixels (x_rows >= H, x_cols >= W). */
int gdkvm_bias_relu_maxpool(const void* x, const float* bias, void* y, int N, int H, int W, int C,
                            int x_rows, int x_cols, int io_dtype, void* stream);

/* Row n1, the inference stem in one kernel: y = maxpool3x3/2/pad1(relu(conv4x4/1/pad2(xs, w) + bias)) cropped to the Hs x Ws
 * convolution outputs -- xs [N, Hs, Ws, 16] is the space-to-depth image of gdkvm_stem_s2d, w [64, 4, 4, 16] the 4x4 kernel
 * model.FusedConvPool.enable_s2d builds from a 7x7 / stride 2 stem, y [N, (Hs-1)/2+1, (Ws-1)/2+1, 64]; bf16, 64 output
 * channels.  The full-resolution activation exists only as an LDS tile (csrc/stem_conv_pool.hip). */
int gdkvm_stem_conv_pool(const void* xs, const void* w, const float* bias, void* y, int N, int Hs, int Ws,
                         int io_dtype, void* stream);
/* The same kernel reading the NCHW frames x [N, C <= 4, H, W] themselves (H, W even; Hs = H/2, Ws = W/2): the workgroup builds its band of
 * the space-to-depth image on the way into LDS, so gdkvm_stem_s2d and its 16-channel copy of the input are not needed.  Bit-identical to
 * gdkvm_stem_s2d followed by gdkvm_stem_conv_pool. */
int gdkvm_stem_conv_pool_nchw(const void* x, const void* w, const float* bias, void* y, int N, int C, int H, int W,
                              int io_dtype, void* stream);
/* Training: the stem's raw convolution (7x7 / stride 2 / pad 3, no bias) on the same kernel, y [N, H/2, W/2, 64] bf16 written to memory
 * (BatchNorm follows), from NCHW frames and the kernel in the space-to-depth form w4 [64, 4, 4, 16] bf16 -- which gdkvm_stem_pack_s2d
 * builds from the fp32 [64, C, 7, 7] weight (element strides sk, sc, sr, ss) in one small launch per step. */
int gdkvm_stem_conv_nchw(const void* x, const void* w4, void* y, int N, int C, int H, int W, int io_dtype, void* stream);
int gdkvm_stem_pack_s2d(const float* w7, void* w4, int C, long long sk, long long sc, long long sr, long long ss, void* stream);
/* Training: the stem convolution's weight gradient dw7 [64, C, 7, 7] fp32 (element strides sk, sc, sr, ss; every element written) from
 * the NCHW frames x [N, C <= 4, H, W] bf16 and dy [N, H/2, W/2, 64] bf16 (NHWC), as a pixel-axis product in the space-to-depth form with a
 * fixed-order reduction over workgroup partials held in `workspace` (gdkvm_stem_wgrad_workspace_bytes): deterministic, unlike the framework
 * convolution's atomically accumulated gradient it replaces. */
size_t gdkvm_stem_wgrad_workspace_bytes(int N, int H, int W);
int gdkvm_stem_wgrad_nchw(const void* x, const void* dy, float* dw, long long sk, long long sc, long long sr, long long ss,
                          void* workspace, size_t workspace_bytes, int N, int C, int H, int W, int io_dtype, void* stream);

/* Row n1, the training stem: 3x3 / stride 2 / pad 1 max-pool of an NHWC tensor x [N, H, W, C] -> y [N, Ho, Wo, C]
 * (Ho = (H-1)/2+1) recording the winning tap of every output element in idx (one byte each, [N, Ho, Wo, C]: 3*dy + dx in
 * window coordinates; first maximum in scan order, NaN wins -- PyTorch's rule), and its backward: dx [N, H, W, C] gathers dy
 * from the at most four windows that contain a pixel (deterministic, dx written once). */
int gdkvm_maxpool_fwd(const void* x, void* y, void* idx, int N, int H, int W, int C, int io_dtype, void* stream);
int gdkvm_maxpool_bwd(const void* dy, const void* idx, void* dx, int N, int H, int W, int C, int io_dtype, void* stream);

/* Row n1, the stem input: NCHW frames x [N, C, H, W] (H, W even) -> the space-to-depth image out [N, H/2, W/2, Cp] (NHWC),
 * out[n, i, j, (c*2 + p)*2 + q] = x[n, c, 2i + p, 2j + q], channels 4C .. Cp-1 zero.  A k x k / stride 2 convolution on x is
 * a ceil(k/2)+... x stride 1 convolution on out (gdkvm_amd/model.py::FusedConvPool builds the 4x4 kernel of a 7x7 stem). */
int gdkvm_stem_s2d(const void* x, void* out, int N, int C, int H, int W, int Cp, int io_dtype, void* stream);

/* Row n1, the training side: BatchNorm in batch-statistics mode fused with the residual add and the ReLU that follow it
 * (what torch.nn.BatchNorm2d(train) -> (+ skip) -> ReLU computes on an NHWC conv output), forward and backward.
 * x, residual, y, dy, dx, dres: [rows, C] in io_dtype (rows = N*H*W of an NHWC tensor, C a multiple of 8 (bf16) / 4 (f32));
 * gamma, beta, running_*, dgamma, dbeta: fp32 [C];  save_stats: fp32 [4][C] = mean, 1/sqrt(var+eps), scale, shift.
 *   fwd:  mean, var (biased) over the rows;  y = act(x*scale + shift (+ residual)),  scale = gamma rstd, shift = beta - mean scale;
 *         running = (1 - momentum) running + momentum stat (variance unbiased; either pointer may be NULL).
 *   bwd:  g = dy masked by the ReLU;  dbeta = sum g,  dgamma = sum g xhat,  dx = gamma rstd (g - dbeta/n - xhat dgamma/n);
 *         dres (optional) receives g, the gradient of the residual branch.
 *         relu: 0 = none, 1 = mask from the saved output (y > 0), 2 = mask recomputed from x (x*scale + shift > 0, the forward's
 *         own expression: valid when the forward had NO residual; y is then not read and may be NULL).
 * Deterministic (no atomics).  ws: gdkvm_bn_workspace_bytes(C) bytes of scratch per call. */
size_t gdkvm_bn_workspace_bytes(int C);
int gdkvm_bn_fwd_train(const void* x, const void* residual, const float* gamma, const float* beta,
                       float* running_mean, float* running_var, void* y, float* save_stats,
                       void* ws, size_t ws_bytes, long long rows, int C, float eps, float momentum, int relu,
                       int io_dtype, void* stream);
int gdkvm_bn_bwd(const void* x, const void* y, const void* dy, const float* gamma, const float* save_stats,
                 void* dx, void* dres, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                 long long rows, int C, int relu, int io_dtype, void* stream);
/* The training stem's tail as ONE op: BatchNorm(batch statistics) -> ReLU -> 3x3 / stride 2 / pad 1 max-pool of the raw convolution
 * x [N, H, W, C] (bf16, NHWC): y_pool [N, Ho, Wo, C] (Ho = (H-1)/2+1) and the winning taps idx (one byte per element, gdkvm_maxpool_fwd's
 * format and tie rule) -- the normalised full-resolution activation is never written (every pooled element evaluates its window's
 * relu(x*scale + shift), rounded as gdkvm_bn_fwd_train would have stored it: the same bits as the two ops in sequence).  Backward:
 * dx, dgamma, dbeta from dy_pool, idx and x -- the pre-pool gradient is gathered inside the two BatchNorm backward passes
 * (gdkvm_maxpool_bwd's rule and rounding) and never written either.  Fewer than 2^22 pixels per call; bf16 only; deterministic. */
int gdkvm_bn_pool_fwd_train(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                            void* y_pool, void* idx, float* save_stats, void* ws, size_t ws_bytes,
                            int N, int H, int W, int C, float eps, float momentum, int io_dtype, void* stream);
int gdkvm_bn_pool_bwd(const void* x, const void* dy_pool, const void* idx, const float* gamma, const float* save_stats,
                      void* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                      int N, int H, int W, int C, int io_dtype, void* stream);

/* decoder glue, out = concat(bilinear_upsample(lo -> H x W), skip) over
 * NHWC tensors  lo [N,hl,wl,C1], skip [N,H,W,C2], out [N,H,W,C1+C2]; align_corners = false; bf16 only.  skip == NULL with
 * C2 == 0: the enlargement alone (its consumer, gdkvm_conv_cat_bias_act, reads the skip tensor where it lies). */
int gdkvm_upsample_cat(const void* lo, const void* skip, void* out,
                       int Nimg, int hl, int wl, int H, int W, int C1, int C2, int io_dtype, void* stream);
/* Backward of gdkvm_upsample_cat (training): dlo [Nimg, hl, wl, C1] = transpose of the bilinear enlargement applied to
 * dout[..., :C1] (a deterministic gather: no atomics), dskip [Nimg, H, W, C2] = dout[..., C1:].  bf16 only. */
int gdkvm_upsample_cat_bwd(const void* dout, void* dlo, void* dskip,
                           int Nimg, int hl, int wl, int H, int W, int C1, int C2, int io_dtype, void* stream);

/* Rows n1/n2, the training objective on the decoder's stride-4 logits z [images, C, h, w] (NCHW, io_dtype) and integer labels
 * target [images, H, W] (target_bytes = 1: uint8, 8: int64), 2 <= C <= 8:
 *   l = bilinear_upsample(z -> H x W, align_corners = false) in fp32;  p = softmax(l);
 *   loss = mean CE(l, target) + dice_weight * (1 - mean_c (2 I_c + eps) / (P_c + O_c + eps)),  sums over the whole batch.
 * A label outside [0, C) marks an unlabelled pixel (EchoNet-Dynamic: every frame but the two traced ones): it adds to no sum at all -- the CE
 * mean runs over the labelled pixels, and neither I_c, O_c nor P_c see it (round 5; before, its softmax still counted in P_c, which pushed
 * the predictions on unlabelled frames towards "nothing").
 * fwd: out[0] = loss, out[1] = CE, out[2] = Dice term; ws keeps the per-class coefficients the backward needs.
 * bwd: dz [images, C, h, w] = (*grad_out, or 1 if NULL) * dloss/dz -- a gather per stride-4 pixel, deterministic.
 * Full-resolution logits are never materialised.  ws: gdkvm_seg_loss_workspace_bytes(C), the SAME buffer for fwd and bwd. */
size_t gdkvm_seg_loss_workspace_bytes(int C);
int gdkvm_seg_loss_fwd(const void* z, const void* target, float* out, void* ws, size_t ws_bytes,
                       int images, int C, int h, int w, int H, int W, float dice_weight, float eps,
                       int io_dtype, int target_bytes, void* stream);
int gdkvm_seg_loss_bwd(const void* z, const void* target, const void* ws, size_t ws_bytes, const float* grad_out, void* dz,
                       int images, int C, int h, int w, int H, int W, int io_dtype, int target_bytes, void* stream);

/* The same objective with the boundary loss of Kervadec et al. (MIDL 2019) as a third term:  loss = CE + dice_weight * Dice + boundary_weight * L_B,
 *   L_B = (1 / n_lab) sum over the labelled pixels x, sum over c in K, of p_c(x) phi_c(x)
 * with p the softmax of the upsampled logits as above, n_lab the count of labelled pixels clamped to 1 (the cross-entropy's own denominator; an
 * unlabelled pixel adds nothing), K the classes whose bit is set in class_mask (bit c = class c; no bit at or above C), and phi_c the signed
 * distance to the contour of class c as the paper's reference implementation defines it (edt(neg) neg - (edt(pos) - 1) pos), evaluated in fp32
 * inside the kernels from sd2 [images, C, H, W] int32, the signed squared distances of gdkvm_signed_distance for the SAME target:
 *   s > 0: phi = sqrt(s);   s < 0: phi = -(sqrt(-s) - 1);   s = 0: phi = 0.
 * L_B is NOT divided by |K|: boundary_weight absorbs it (a weight tuned for three foreground classes is three times a per-class weight).
 * The planes of sd2 outside class_mask are never read.  boundary_weight is finite and >= 0.
 * fwd: out[0] = loss, out[1] = CE, out[2] = Dice term, out[3] = L_B.
 * bwd: with respect to an upsampled logit the term adds  boundary_weight / n_lab * p_c (psi_c - sum_k p_k psi_k),  psi_c = phi_c for c in K, else 0
 * -- one more summand of u_c in the gather of gdkvm_seg_loss_bwd; deterministic.  class_mask as in the forward.
 * ws: gdkvm_seg_loss_boundary_workspace_bytes(C), the SAME buffer for fwd and bwd (one partial sum more than gdkvm_seg_loss_workspace_bytes).
 * gdkvm_seg_loss_fwd / _bwd are unchanged by these entries. */
size_t gdkvm_seg_loss_boundary_workspace_bytes(int C);
int gdkvm_seg_loss_boundary_fwd(const void* z, const void* target, const int32_t* sd2, float* out, void* ws, size_t ws_bytes,
                                int images, int C, int h, int w, int H, int W, float dice_weight, float eps, float boundary_weight,
                                unsigned class_mask, int io_dtype, int target_bytes, void* stream);
int gdkvm_seg_loss_boundary_bwd(const void* z, const void* target, const int32_t* sd2, const void* ws, size_t ws_bytes,
                                const float* grad_out, void* dz, int images, int C, int h, int w, int H, int W, unsigned class_mask,
                                int io_dtype, int target_bytes, void* stream);

/* Training-clip augmentation folded into the uint8 -> [0, 1] cast of a batch (gdkvm_amd.pipeline.DevicePrefetcher): one pass, one launch.
 * frames uint8 [B,T,C,H,W]; target [B,T,H,W] (target_bytes = 1: uint8, 8: int64; target and target_out alike, both may be NULL together);
 * params fp32 [B,12] on the device, one row per clip -- every frame of a clip gets the same warp (the memory path needs temporally
 * consistent geometry):  m00 m01 m02 m10 m11 m12 gain bias gamma 0 0 0.  frames_out [B,T,C,H,W] in io_dtype.
 *   coordinates  destination pixel index (x, y) reads source index sx = m00 x + m01 y + m02, sy = m10 x + m11 y + m12; pixel centres sit
 *                at integers.  The matrix is the INVERSE (destination -> source) map, composed on the host: the kernel does no trigonometry.
 *   intensity    per clip a 256-entry table: u = float(b) * (1.0f/255.0f);  LUT[b] = clamp(fmaf(gain, gamma == 1 ? u : powf(u, gamma), bias), 0, 1)
 *                (built once per workgroup in LDS; a workgroup never spans two clips).
 *   frames       bilinear sampling of LUT[byte]: with x0 = floor(sx), fx = sx - x0 (likewise y) and the taps a = (x0, y0), b = (x0+1, y0),
 *                c = (x0, y0+1), d = (x0+1, y0+1):  out = (1-fy) ((1-fx) a + fx b) + fy ((1-fx) c + fx d).  A tap whose index lies outside the
 *                frame is 0 and is not loaded.  Rounded once to io_dtype.
 *   target       nearest neighbour: ix = floor(sx + 0.5), iy = floor(sy + 0.5); the label is copied unchanged when the index lies inside
 *                the frame, otherwise it is fill_label (in [0, 255]; gdkvm_amd.data.IGNORE_LABEL makes the loss and the Dice counts skip
 *                the invented corners).
 *   identity     with the row 1 0 0 0 1 0 1 0 1 the frames are fp32(byte) * fp32(1/255) rounded once to io_dtype -- bit for bit the plain
 *                cast -- and the target is copied unchanged.
 * 16-byte stores when H*W is a multiple of the 16-byte vector (8 pixels bf16, 4 fp32) and the output bases are 16-byte aligned, element
 * stores otherwise; B*T <= 65535 (one grid row per frame); B*T == 0 is GDKVM_OK without a launch. */
int gdkvm_augment_clips(const uint8_t* frames, const void* target, const float* params, void* frames_out, void* target_out,
                        int B, int T, int C, int H, int W, int io_dtype, int target_bytes, int fill_label, void* stream);

/* Left-ventricular geometry of label masks (the evaluation's epilogue beside the Dice counts; csrc/lv_measure.hip).  Integer-exact up to the
 * disk areas; volumes are in pixel^3 of the mask's grid (isotropic pixels assumed -- physical spacing is the caller's), EF is a ratio.
 * Per frame mask [H, W] uint8, class cls (0..254; every other byte, 255 included, is "not cls"), D disks (1..64), H, W in 1..1024, Q = 2^16;
 * P = the pixels (x, y) with mask[y][x] == cls:
 *   1. moments (int64)   n = |P|, sx = sum x, sy = sum y, sxx = sum x^2, sxy = sum x y, syy = sum y^2
 *   2. scaled central    A = n sxx - sx^2,  B = n sxy - sx sy,  C = n syy - sy^2
 *   3. long axis (fp64, un-fused multiplies and adds)   a = (double)(A - C), b = (double)(2 B), r = sqrt(a a + b b);
 *        r == 0: u = (0, 1);  a >= 0: u ~ (a + r, b);  else u ~ (b, r - a);  u / |u|, sign such that uy > 0 or (uy == 0 and ux > 0);
 *        Ux = rint(ux Q), Uy = rint(uy Q)   (the eigenvector of the larger eigenvalue of [[A, B], [B, C]]; the default is the image's vertical)
 *        (every operation rounded once, IEEE fp64, no fused multiply-add: the library is compiled with contraction off for this file.  A host
 *        restatement whose sqrt and division are correctly rounded reproduces Ux, Uy; one that fuses a a + b b may move a rint tie, so a
 *        cross-check should accept |dUx|, |dUy| <= 1 and compare steps 4 - 6 using the axis the device reported, as the tests do)
 *   4. projection (int64)   t_p = (n x - sx) Ux + (n y - sy) Uy;  tmin, tmax over P;  P1 = n Q (one pixel of extent);  Lt = tmax - tmin + P1
 *   5. disks by overlap (int64)   pixel p covers [D (t_p - tmin), D (t_p - tmin) + D P1), disk j covers [j Lt, (j + 1) Lt);
 *        W_j = sum_p overlap(p, j), hence sum_j W_j = n D P1 exactly
 *   6. geometry (fp64)   L = Lt / P1 (pixels);  a_j = W_j / (D P1) (pixels^2 in disk j);  V = pi D sum_j a_j^2 / (4 L) (single-plane method of
 *        disks: height L / D, mean width a_j D / L);  cx = sx / n, cy = sy / n.   n == 0: every output of the frame is 0.
 * mask [frames, H, W] contiguous, ANY byte alignment (frames of H W bytes follow each other).  Outputs (16-byte aligned):
 *   stats [frames, 12] = n, sx, sy, sxx, sxy, syy, Ux, Uy, tmin, tmax, Lt, 0;   disks [frames, D] = W_j;   geom [frames, 4] = L, V, cx, cy.
 * One workgroup per frame, integer sums only: bit-reproducible.  frames == 0 is GDKVM_OK without a launch. */
int gdkvm_lv_measure(const uint8_t* mask, int64_t* stats, int64_t* disks, double* geom,
                     int frames, int H, int W, int cls, int D, void* stream);
/* The same with a pixel spacing: lengths in mm, volumes in mL, the long axis found in the PHYSICAL plane (a CAMUS sequence squeezed to a square
 * grid has pixels of about 0.33 x 0.47 mm: in pixel units its ventricle is distorted).  spacing_um [frames, 2] int32 on the DEVICE (4-byte
 * aligned) holds, per frame, ry = the micrometres per pixel down the rows (y) and rx = along the columns (x), each in 1..4095.
 * Steps 1, 2, 4 and 5 are those above, integer for integer, with (Vx, Vy) in place of (Ux, Uy) and P1 = n E.  What is new:
 *   3'. axis (fp64, every operation rounded once, no fused multiply-add)   g = gcd(ry, rx), py = ry / g, px = rx / g, pm = max(px, py);
 *        a = (double)(px px) (double)A - (double)(py py) (double)C,  b = 2 ((double)(px py) (double)B)   (the central moments of the
 *        physical positions (x rx, y ry), over g^2);  r and the unit vector (ux, uy) with its sign rule exactly as in step 3: the long axis
 *        in the physical plane;
 *        ex = ux (double)px, ey = uy (double)py, e = sqrt(ex ex + ey ey);
 *        Vx = rint((ux (double)(px Q)) / (double)pm), Vy = rint((uy (double)(py Q)) / (double)pm), E = rint((e (double)Q) / (double)pm).
 *        (x, y) -> x Vx + y Vy is the projection of the physical position on the axis in units of g pm / Q um, and E one pixel's extent
 *        along the axis in the same units.  |Vx|, |Vy| <= Q and 16 <= E <= Q, so the integer ranges of steps 4 and 5 stand.  Isotropic
 *        spacing gives px = py = 1 and E = Q, and V is U up to the +-1 of a moved rint tie.
 *   6'. geometry (fp64)   k = e (double)g (um per pixel extent along the axis);  L = ((Lt / P1) k) / 1000 (mm);
 *        a_j = (W_j / (D P1)) ((double)(ry rx) / 1e6) (mm^2 in disk j);  V = ((pi D) sum_j a_j^2) / (4 L) / 1000 (mL), the sum in ascending j;
 *        cx = ((sx / n) (double)rx) / 1000, cy = ((sy / n) (double)ry) / 1000 (mm);  area = (double)(n ry rx) / 1e6 (mm^2).
 * Outputs (16-byte aligned):  stats [frames, 12] = n, sx, sy, sxx, sxy, syy, Vx, Vy, tmin, tmax, Lt, E;   disks [frames, D] = W_j;
 *   geom [frames, 6] = L, V, cx, cy, k, area.   n == 0: every output of the frame is 0.  A frame whose ry or rx is outside 1..4095: every
 * output of the frame is -1 (the kernel cannot return an error; gdkvm_amd.ops checks a host tensor before it is copied).  gdkvm_lv_ef takes
 * the mL curve (geom[..., 1]) as it is.  Everything else as for gdkvm_lv_measure. */
int gdkvm_lv_measure_mm(const uint8_t* mask, const int32_t* spacing_um, int64_t* stats, int64_t* disks, double* geom,
                        int frames, int H, int W, int cls, int D, void* stream);
/* Clip level: vol, npix [B, T] (geom[..., 1] and stats[..., 0] of gdkvm_lv_measure, made contiguous; 8-byte aligned), optional pick_vol /
 * pick_npix [B, T] (both or neither; e.g. the target's, so that the prediction's volumes are read at the annotated frames).  Frame t is valid
 * when pick_npix[b][t] >= min_pixels (npix without pick arrays); ED = the valid frame of the largest pick volume, ES = of the smallest, ties ->
 * the lowest t;  EDV = vol[b][ed], ESV = vol[b][es], EF = (EDV - ESV) / EDV (0 when EDV == 0).  Fewer than two valid frames: ed = es = -1 and
 * EDV = ESV = EF = 0.  ed_es_nvalid int32 [B, 3], edv_esv_ef fp64 [B, 3] (16-byte aligned).  B == 0 is GDKVM_OK without a launch. */
int gdkvm_lv_ef(const double* vol, const int64_t* npix, const double* pick_vol, const int64_t* pick_npix,
                int32_t* ed_es_nvalid, double* edv_esv_ef, int B, int T, int64_t min_pixels, void* stream);
/* Clip level, beat by beat (csrc/lv_beats.hip): gdkvm_lv_ef's global maximum and minimum belong to different beats as soon as a clip holds more
 * than one, and the EF they give is biased upwards.  area int64 [B, T] (stats[..., 0] of gdkvm_lv_measure; values in 0 .. 2^50), vol fp64
 * [B, T] (geom[..., 1], pixel^3 or mL: only read at the beats' frames), both 8-byte aligned; length int32 [B] on the device (4-byte aligned) or
 * NULL = T.  Per clip only the frames 0 .. len - 1 count, len = length[b] clamped to 0 .. T; the padding behind len is never read.  With a =
 * area[b], all integer arithmetic up to the per-beat EF:
 *   1. candidates   the strict local minima of a.  Frame p, 0 < p < len - 1, starts a plateau p .. r of equal values when a[p - 1] > a[p] and
 *        a[r + 1] > a[p] (r + 1 <= len - 1); the candidate is frame (p + r) / 2, integer division (scipy.signal.find_peaks' rule).  The
 *        first and the last valid frame are never candidates.
 *   2. distance     candidates are ordered by priority, smaller area first and the lower frame on a tie (a strict total order); a candidate
 *        is kept exactly when no kept candidate of higher priority lies closer than `distance` frames (|p - q| < distance): find_peaks'
 *        distance= rule, the greedy pass in priority order.  (Its result is the unique fixed point of "keep when every rival in range is
 *        dropped or of lower priority, drop when one rival in range is kept", which is what the kernel iterates.)
 *   3. prominence   for a kept candidate p: walk left from p while a[j] >= a[p], to a frame of strictly smaller area or to frame 0; lmax =
 *        the largest area met, a[p] included; rmax the same towards len - 1 (the walks are over ALL frames, as in scipy).  p is an
 *        END-SYSTOLE when (min(lmax, rmax) - a[p]) 1000 >= prominence_permille (max a - min a), both extremes over the valid frames.
 *   4. beats        end-systoles e_0 < .. < e_(m-1); beat j has ES = e_j and ED = the frame of the largest area in e_(j-1) + 1 .. e_j - 1
 *        (e_(-1) = -1), the lowest frame on a tie.  Beat 0 COUNTS only when its ED is not frame 0 (the clip started inside that beat: its true
 *        ED is unknown); every later beat counts.  Per counted beat, fp64, every operation rounded once, no fused multiply-add:
 *        EDV = vol[ed], ESV = vol[es], EF = (EDV - ESV) / EDV (0 when EDV == 0).
 * Outputs (16-byte aligned):
 *   beats int32 [B, max_beats, 2] = (ed, es) of the first max_beats counted beats, the rest -1;   beat_val fp64 [B, max_beats, 3] = EDV, ESV,
 *   EF, the rest 0;   info int32 [B, 4] = n_beats (ALL counted beats: it may exceed max_beats), m, n_below = the valid frames with area <
 *   min_pixels, e_(m-1) - e_0 (0 when m < 2);   summ fp64 [B, 4] = the mean EF over all counted beats (added in ascending beat order, then
 *   divided by n_beats), the smallest EF, the largest EF, the mean cycle in frames (double)(e_(m-1) - e_0) / (double)(m - 1) (0 when m < 2);
 *   all four 0 when no beat counts.
 * n_below > 0 drops nothing: a frame where the class vanished is a false systole, and what to do with such a clip is the caller's decision.
 * 1 <= T <= 4096, 1 <= max_beats <= 64, 1 <= distance <= 4096, 0 <= prominence_permille <= 1000, B >= 0: anything else is GDKVM_ERR_SHAPE, a
 * null or misaligned pointer GDKVM_ERR_ARG, both before any device call; B == 0 is GDKVM_OK without a launch.  One workgroup per clip, the curve
 * in LDS; no allocation, no synchronisation, no global atomics: capturable beside gdkvm_lv_measure; bit-reproducible. */
int gdkvm_lv_beats(const int64_t* area, const double* vol, const int32_t* length,
                   int32_t* beats, double* beat_val, int32_t* info, double* summ,
                   int B, int T, int max_beats, int distance, int prominence_permille, int64_t min_pixels, void* stream);
/* Bi-plane Simpson volume from two views of one ventricle (csrc/lv_biplane.hip): the apical two-chamber and four-chamber clips of a patient
 * combined into one volume per frame, the method of disks the echo guidelines prescribe and the quantity CAMUS states per patient.  Inputs are
 * the records exactly as gdkvm_lv_measure_mm wrote them for C clips of T frames, on the device: stats int64 [C, T, 12], disks int64 [C, T, D],
 * geom fp64 [C, T, 6] (8-byte aligned), spacing_um int32 [C, T, 2] (the table that call read), and pairs int32 [P, 2] (4-byte aligned): row p
 * holds the clip index of view a and of view b.  Per (pair, frame), for view v in {a, b}: n_v = stats[0], E_v = stats[11], L_v = geom[0], W_j^v =
 * disks[j], (ry, rx) = that frame's spacing.  fp64, every operation rounded once, no fused multiply-add:
 *   pix_v = (double)(ry rx) / 1e6
 *   a_j^v = ((double)W_j^v / (double)(D n_v E_v)) pix_v        (step 6' of gdkvm_lv_measure_mm, operation for operation: mm^2 in disk j)
 *   w_j^v = (a_j^v (double)D) / L_v                            (the mean width of disk j in mm)
 *   L     = max(L_a, L_b)
 *   s     = sum over j ascending, from 0.0, of w_j^a w_j^b
 *   V     = (((3.14159265358979323846 / 4.0) s) (L / (double)D)) / 1000.0      (mL: D elliptic disks of height L / D and axes w_j^a, w_j^b)
 *   mism  = (L - min(L_a, L_b)) / L                            (the guidelines ask for long axes within 10 % of each other)
 *   npix  = min(n_a, n_b)
 * With a = b this is the single-plane V of gdkvm_lv_measure_mm up to the order of its operations.  ASSUMPTION: disk j of both views counts from
 * the same end of the ventricle.  Disk 0 lies at tmin, and step 3's sign rule turns the axis towards growing y (down the image), so disk 0 is
 * the uppermost end of the ventricle in both views whenever both show the apex up, as CAMUS does; a view stored apex down must be flipped by
 * the caller.  The two views may differ in spacing, frame size and axis; they share D and T, and frame t of one is paired with frame t of the
 * other.
 * Outputs (16-byte aligned):  out fp64 [P, T, 3] = V, L, mism;   npix int64 [P, T].  If n_a <= 0 or n_b <= 0 (an empty frame, or the -1 record
 * of a spacing out of range): V = L = mism = 0 and npix = 0.  The kernel never reads outside the tables: a pair index outside 0 .. C - 1
 * gives the pair's rows as all 0 and npix 0 (gdkvm_amd.ops refuses such a table on the host before it is copied).
 * 1 <= D <= 64, C, T, P >= 0, P T and C T below 2^31: anything else is GDKVM_ERR_SHAPE, a null or misaligned pointer GDKVM_ERR_ARG, both before
 * any device call; P == 0 or T == 0 is GDKVM_OK without a launch.  One wave per (pair, frame): lanes j < D form the products, which are added
 * in ascending j; no allocation, no atomics, no synchronisation with the host: capturable; bit-reproducible. */
int gdkvm_lv_biplane(const int64_t* stats, const int64_t* disks, const double* geom, const int32_t* spacing_um, const int32_t* pairs,
                     double* out, int64_t* npix, int C, int T, int D, int P, void* stream);
/* Contour length and landmarks of one class of label masks (csrc/lv_contour.hip): what global longitudinal strain needs -- the length of the
 * endocardial contour, the width of the mitral annulus, the apex and the apex-to-annulus long axis.  CAMUS class 1 (cavity) borders class 2
 * (myocardium) along the endocardium and class 3 (atrium) along the mitral plane.  Per frame the inputs are:
 *   - mask [H, W] uint8, H, W in 1..1024.
 *   - class cls in 0..31.
 *   - two sets of bytes given as 32-bit masks over the bytes 0..31: wall_set and base_set.  The two sets are disjoint, and neither holds
 *     cls.  wall_set must be non-zero.  base_set may be 0.
 *   - Bytes >= 32 (255 included) belong to no set.
 *   - A position outside the frame reads as byte 0.  This is the background rule the surface kernels already use.
 *   - The spacing is (ry, rx) um per pixel down the rows and along the columns, each in 1..4095.  A NULL spacing pointer means ry = rx = 1.
 *   1. Pair counts.  The four directions are d in {E = (0,+1), S = (+1,0), SE = (+1,+1), SW = (+1,-1)}, written (dy, dx).  For a set X,
 *      N_d[X] is the number of unordered position pairs {p, p+d} where one member is an in-frame pixel holding cls and the other member's
 *      byte (outside the frame: 0) is in X.  Equivalently: over every cls pixel and each of its 8 neighbours, count the neighbours whose
 *      byte is in X, sorted by direction.  These are the intersection counts of the interface curve between the class and X with the four
 *      families of lattice lines.
 *   2. Base point.  Over the E and S pairs of base_set only:  n_b = N_E + N_S,  SX2 = sum (p.x + q.x),  SY2 = sum (p.y + q.y).  These are
 *      twice the crack midpoints, so they are integers.  An outside neighbour contributes -1 or W / H.
 *      bx2 = floor((2 SX2 + n_b) / (2 n_b)), with the floor taken towards -infinity, and by2 likewise.  This is the interface's centroid in
 *      half-pixel units, rounded half up.
 *   3. Apex.  The apex is the cls pixel p that maximises D2(p) = (ry (2 p.y - by2))^2 + (rx (2 p.x - bx2))^2.  This is below 2^48, so it
 *      is exact in int64.  Ties go to the smallest p.y W + p.x.
 *   4. Record rec [frames, 16] int64, 16-byte aligned:
 *        word 0: n, the pixels of cls.   words 1-4: N_E, N_S, N_SE, N_SW of wall_set.   words 5-8: the same four counts of base_set.
 *        words 9-10: SX2, SY2.   words 11-12: bx2, by2.   word 13: the apex's y W + x.   word 14: D2 at the apex.   word 15: 0.
 *      With n_b == 0 (which covers n == 0): words 9, 10 and 14 are 0 and words 11-13 are -1.
 *      For a frame whose spacing lies outside 1..4095, every word is -1, as in gdkvm_lv_measure_mm.
 *   5. Every word is an integer that depends on neither the algorithm nor the schedule.
 * From the record, three lengths in fp64 with one rounding per operation (gdkvm_amd.ops.contour_lengths, on the host or the device):
 *   phi = atan2(ry, rx),  delta = (ry rx) / sqrt(ry^2 + rx^2);
 *   for a set's four counts:  L = 0.5 (phi (N_E ry) + (pi/2 - phi) (N_S rx) + (pi/4) ((N_SE + N_SW) delta))
 *   (the Cauchy-Crofton length with the four lattice directions, weighted by their angular sectors; with ry = rx it reduces to
 *   (pi/8) (N_E + N_S + (N_SE + N_SW) / sqrt 2));  L_wall is the endocardial contour, L_base the annulus width, L_axis = sqrt(D2) / 2 the
 *   apex-to-base-point distance.  Units are um, then mm (/ 1000); without a spacing the units are pixels.
 * mask [frames, H, W] contiguous, ANY byte alignment; spacing_um [frames, 2] int32 on the device (4-byte aligned) or NULL.  A bad shape is
 * GDKVM_ERR_SHAPE; cls outside 0..31, sets that overlap or hold cls, wall_set == 0, a null mask, a null or misaligned rec and a misaligned
 * spacing_um are GDKVM_ERR_ARG; both before any device call.  frames == 0 is GDKVM_OK without a launch.  One 256-lane workgroup per frame
 * walks it in bands of GDKVM_LV_CONTOUR_BAND_ROWS rows held as bit planes of GDKVM_LV_CONTOUR_WORD_BITS-bit words in LDS; no workspace, no
 * allocation, no global atomics, no fences: capturable; bit-reproducible. */
#define GDKVM_LV_CONTOUR_BAND_ROWS 64
#define GDKVM_LV_CONTOUR_WORD_BITS 64
int gdkvm_lv_contour(const uint8_t* mask, const int32_t* spacing_um, int64_t* rec,
                     int frames, int H, int W, int cls, unsigned wall_set, unsigned base_set, void* stream);

/* Keep the largest connected component of one class of label masks (the clean-up in front of gdkvm_lv_measure: an argmax mask is no tracing,
 * and a false-positive island far from the ventricle enters tmin / tmax, the long axis and the disks; csrc/largest_component.hip).  Every
 * output is an integer that depends on neither the algorithm nor the schedule.
 * Per frame mask [H, W] uint8, class cls (0..254), connectivity 4 or 8, fill (0..255, != cls), H, W in 1..1024:
 *   1. P = the pixels with mask[y][x] == cls; every other byte, 255 and every other class included, is "not cls".
 *   2. Two pixels of P in the SAME frame are adjacent when |dx| + |dy| == 1 (connectivity 4) or max(|dx|, |dy|) == 1 (connectivity 8).
 *      Adjacency is geometric, not by linear index: (W - 1, y) and (0, y + 1) are no neighbours, nor are the last pixel of frame f and the
 *      first pixel of frame f + 1.
 *   3. A component is an equivalence class of the transitive closure of adjacency; its LABEL is its smallest linear index y W + x.
 *   4. The KEPT component is the one with the most pixels; on a tie the smallest label wins.
 *   5. out[p] = mask[p] when mask[p] != cls or p lies in the kept component, otherwise out[p] = fill.
 *   6. info [frames, 8] int32 = components (their number), n = |P|, n_kept, label_kept (-1 when P is empty),
 *        removed_hit_cls = |{p removed : target[p] == cls}|, removed_hit_fill = |{p removed : target[p] == fill}| (both 0 when target == NULL),
 *        0, 0.   P empty: out = mask and info = {0, 0, 0, -1, 0, 0, 0, 0}.
 * mask, target (optional) and out are [frames, H, W] contiguous at ANY byte address (frames of H W bytes follow each other); out is either
 * exactly mask (in place) or does not overlap it; info is 16-byte aligned.  The workspace (16-byte aligned, at least
 * gdkvm_largest_component_workspace_bytes(frames, H, W) bytes: 0 while H W <= 15360, where the labels live in LDS, else 4 bytes per pixel with
 * each frame's slice rounded up to 16 bytes) is scratch.  One workgroup per frame; neither entry allocates or synchronises; bit-reproducible.
 * Every loop of the kernel is bounded by H W; should a frame ever reach that bound (the derivation in the source says it cannot), it reports
 * components = -1, n_kept = n, label_kept = -1 and out = mask.  Bad arguments (shape, cls, connectivity, fill, null or misaligned pointers,
 * a short workspace, a partial overlap) are GDKVM_ERR_SHAPE before any device call; frames == 0 is GDKVM_OK without a launch. */
size_t gdkvm_largest_component_workspace_bytes(int frames, int H, int W);
int gdkvm_largest_component(const uint8_t* mask, const uint8_t* target, uint8_t* out, int32_t* info, void* workspace, size_t workspace_bytes,
                            int frames, int H, int W, int cls, int connectivity, int fill, void* stream);

/* Fill the holes of one class of label masks (the second clean-up in front of gdkvm_lv_measure, behind gdkvm_largest_component: pixels inside
 * the cavity that argmax gave to another class; the method of disks squares each disk's area, so a hole costs about twice its pixel share in
 * volume; csrc/fill_holes.hip).  Every output is an integer that depends on neither the algorithm nor the schedule.
 * Per frame mask [H, W] uint8, class cls (0..254), connectivity 4 or 8, max_area >= 0, H, W in 1..1024:
 *   1. P = the pixels with mask[y][x] == cls; every other byte, 255 and every other class included, belongs to the complement Q.
 *   2. Two pixels of Q in the SAME frame are adjacent when |dx| + |dy| == 1 (connectivity 4) or max(|dx|, |dy|) == 1 (connectivity 8).
 *      Adjacency is geometric, as for gdkvm_largest_component: (W - 1, y) and (0, y + 1) are no neighbours, nor are pixels of two frames.
 *      `connectivity` is that of the COMPLEMENT: 4 is scipy.ndimage.binary_fill_holes' default and the dual of an 8-connected class, 8 the
 *      dual of a 4-connected one.
 *   3. A component of Q is an equivalence class of the transitive closure of adjacency.  It is OUTSIDE when it holds a pixel with x == 0,
 *      x == W - 1, y == 0 or y == H - 1; every other component is a HOLE, and its size is its number of pixels.
 *   4. A hole is FILLED when max_area == 0 or its size is <= max_area (max_area lets the call serve a ring-shaped class: a myocardium whose
 *      cavity must stay open while speckle holes close).
 *   5. out[p] = cls for every pixel of a filled hole, out[p] = mask[p] everywhere else.
 *   6. info [frames, 8] int32 = holes (their number, filled or not), holes_filled, n = |P|, filled (pixels changed), largest_hole (the size of
 *        the largest hole, filled or not; 0 without holes), hit_before = |{p in P : target[p] == cls}|,
 *        hit_filled = |{p filled : target[p] == cls}|, n_target = |{p : target[p] == cls}| (the last three 0 when target == NULL).
 *        The class's three Dice counts of the filled mask are |A n B| = hit_before + hit_filled, |A| = n + filled, |B| = n_target: no second
 *        pass over the pixels.
 *   7. P empty, P the whole frame, H <= 2 or W <= 2: every pixel of Q touches the border, holes = 0 and out = mask.
 * mask, target (optional) and out are [frames, H, W] contiguous at ANY byte address (frames of H W bytes follow each other); out is either
 * exactly mask (in place) or does not overlap it; info is 16-byte aligned.  The workspace (16-byte aligned, at least
 * gdkvm_fill_holes_workspace_bytes(frames, H, W) bytes: 0 while H W <= 15360, where the labels live in LDS, else 4 bytes per pixel with each
 * frame's slice rounded up to 16 bytes) is scratch.  One workgroup per frame; neither entry allocates or synchronises; bit-reproducible.
 * Every loop of the kernel is bounded by H W or a constant; should a frame ever reach that bound (the derivation in the source says it
 * cannot), it reports holes = -1, holes_filled = filled = largest_hole = hit_filled = 0 and out = mask.  Bad arguments (shape, cls,
 * connectivity, max_area < 0, null or misaligned pointers, a short workspace, a partial overlap) are GDKVM_ERR_SHAPE before any device call;
 * frames == 0 is GDKVM_OK without a launch. */
size_t gdkvm_fill_holes_workspace_bytes(int frames, int H, int W);
int gdkvm_fill_holes(const uint8_t* mask, const uint8_t* target, uint8_t* out, int32_t* info, void* workspace, size_t workspace_bytes,
                     int frames, int H, int W, int cls, int connectivity, int max_area, void* stream);

/* Smooth a clip's label masks over time: a per-pixel majority vote over the frames t - r .. t + r (a temporal mode filter; the clean-up that
 * runs FIRST in front of gdkvm_lv_measure, ahead of gdkvm_largest_component and gdkvm_fill_holes: a border pixel that flips class from one
 * frame to the next makes the area curve jitter from which the ED / ES frames are read; csrc/temporal_vote.hip).  Every output is an integer
 * that depends on neither the algorithm nor the schedule.
 * mask [clips, T, H, W] uint8, ncls in 2..8, radius r in 0..7, T >= 1, H, W in 1..1024.  For clip b, frame t and pixel p:
 *   1. The window is the frames max(0, t - r) .. min(T - 1, t + r) of the same clip: truncated at the clip's ends, not padded, and never
 *      reaching into another clip.
 *   2. A frame of the window votes for class c at p when its byte at p equals c and c < ncls.  Bytes >= ncls (255 included) do not vote.
 *   3. If the pixel's own byte is >= ncls, out = mask there (pass-through).
 *   4. Otherwise out is the class with the most votes.  Among tied classes the pixel's own label wins if it is one of them, else the
 *      smallest class index.  (The own label always has its own vote: the maximum is at least 1.)
 *   5. info [clips, T, 4] int32 = changed = |{p : out != mask}|, flips_in = |{p : mask[t][p] != mask[t - 1][p]}| (0 at t = 0; the raw bytes
 *      are compared), flips_out = the same count on out, 0.
 *   6. counts [clips, T, ncls, 3] int32 = {|out == c & target == c|, |out == c|, |target == c|}, gdkvm_argmax_dice's definition; written only
 *      when target (mask's shape, uint8) is given -- without a target counts may be NULL.
 *   7. radius == 0: out = mask, info and counts still computed.
 * mask, target and out are contiguous at ANY byte address (frames of H W bytes follow each other, so with H W % 16 != 0 every frame is
 * aligned differently); out must not overlap mask at all (later frames read earlier input).  info and counts are 16-byte aligned and are
 * zeroed by the callee, with a kernel.  gdkvm_temporal_vote_workspace_bytes is 0 for every shape (the votes live in registers) and the
 * workspace may be NULL; the pair is there so that a caller treats every mask kernel alike.  Neither entry allocates or synchronises;
 * bit-reproducible (the sums are integer atomics).  Bad arguments (shape, ncls, radius, null or misaligned pointers, a target without
 * counts, a short workspace, any overlap of out with mask, clips * T > 2^30) are GDKVM_ERR_SHAPE before any device call; clips == 0 is
 * GDKVM_OK without a launch.
 * Launch geometry, for tests that want shapes on both sides of it: a workgroup (one wave) owns GDKVM_TEMPORAL_VOTE_RUN pixel positions of
 * one clip, 16 per lane, and walks its frames -- or, while that gives fewer than GDKVM_TEMPORAL_VOTE_NARROW_BELOW (clip, run) pairs,
 * GDKVM_TEMPORAL_VOTE_NARROW_RUN positions, 4 per lane; a launch has at most GDKVM_TEMPORAL_VOTE_MAX_WG workgroups, which take further
 * pairs in a grid-stride loop; 16- / 4-byte loads and stores when H W % 16 == 0 and mask, out and target are 16-byte aligned, byte accesses
 * otherwise; one kernel per ncls. */
#define GDKVM_TEMPORAL_VOTE_RUN 1024
#define GDKVM_TEMPORAL_VOTE_NARROW_RUN 256
#define GDKVM_TEMPORAL_VOTE_NARROW_BELOW 3072
#define GDKVM_TEMPORAL_VOTE_MAX_WG 4096
size_t gdkvm_temporal_vote_workspace_bytes(int clips, int T, int H, int W, int ncls);
int gdkvm_temporal_vote(const uint8_t* mask, const uint8_t* target, uint8_t* out, int32_t* info, int32_t* counts,
                        void* workspace, size_t workspace_bytes, int clips, int T, int H, int W, int ncls, int radius, void* stream);

/* Take a clip's label masks from the network's grid to the clip's NATIVE frame size and count them against the native tracing in the same
 * pass (what a Dice that can be set beside a published one is made of; csrc/mask_to_native.hip).  Every output is an integer that depends on
 * neither the algorithm nor the schedule.
 * mask [clips, T, H, W] uint8, H, W in 1..1024, T >= 1, ncls in 2..8; clip b has the native size (h0, w0) = sizes[b], each in 1..2048.  The
 * sampling is the half-pixel-centre bilinear one of F.interpolate(align_corners = False), applied to the one-hot planes of the labels, in
 * integers.  For frame m [H, W] of clip b and native row y:
 *   1. ny = (2 y + 1) H - h0, d = 2 h0, y0 = floor(ny / d) (floor division: -1 in the top half-pixel), fy = ny - y0 d in [0, d).  Row
 *      clamp(y0) has the weight d - fy and row clamp(y0 + 1) the weight fy; clamp clamps to 0 .. H - 1.  Columns likewise with W, w0.
 *   2. The four source pixels have the weights wy wx, which add up to 4 h0 w0 <= 2^24.  A source byte c < ncls votes its weight for class
 *      c; bytes >= ncls (255 included) do not vote.
 *   3. out = the class with the most votes; ties go to the smallest class index; 255 if no class has a vote.
 *   4. counts [clips, T, ncls, 3] int32 = {|out == c & target == c|, |out == c|, |target == c|}, gdkvm_argmax_dice's definition, over the
 *      frame's h0 w0 native pixels; written only when target is given (required then), and zeroed by the callee, with a kernel.
 * So with (h0, w0) == (H, W) out is mask with every byte >= ncls turned into 255, and the votes of a pixel add up to a constant per frame.
 * out and target are RAGGED: clip b's T frames of h0 w0 bytes follow each other, and clip b + 1 follows clip b; both optional, at least one
 * of them; 255 in target is unlabelled.  Frames start at ANY byte address.  native_bytes = the bytes out and target each hold; it must
 * cover the sum over the clips of T h0 w0.  out must overlap neither mask nor target.
 * sizes is a HOST int32 [clips, 2]: the entry validates every size, computes every clip's offset itself and hands them to the kernel by
 * value in the kernel arguments, GDKVM_MASK_TO_NATIVE_CLIPS clips per launch, longer batches in several launches; nothing is copied to the
 * device, nothing allocated, nothing synchronised (a capture holds the sizes).  counts is 16-byte aligned.
 * gdkvm_mask_to_native_workspace_bytes is 0 for every shape and the workspace may be NULL; the pair is there so that a caller treats every
 * mask kernel alike.  Bit-reproducible (the sums are integer atomics).  Bad arguments (shape, ncls, a size outside 1..2048, null mask or
 * sizes, null or misaligned counts with a target, neither out nor target, native_bytes short of the sum, out overlapping mask or target,
 * clips * T > 2^30) are GDKVM_ERR_SHAPE before any device call; clips == 0 is GDKVM_OK without a launch.
 * Launch geometry, for tests that want shapes on both sides of it: a workgroup owns a band of whole native rows of one (clip, frame), the
 * fewest with at least GDKVM_MASK_TO_NATIVE_BAND_PIXELS pixels, and cuts its bytes into runs of GDKVM_MASK_TO_NATIVE_RUN on the 16-byte
 * grid of out's addresses (a head of up to 15 bytes, 16-byte stores and loads, a ragged tail); a launch has at most
 * GDKVM_MASK_TO_NATIVE_MAX_WG workgroups, which take further (clip, frame, band) items in a grid-stride loop; one kernel per ncls. */
#define GDKVM_MASK_TO_NATIVE_RUN 16
#define GDKVM_MASK_TO_NATIVE_BAND_PIXELS 4096
#define GDKVM_MASK_TO_NATIVE_MAX_WG 4096
#define GDKVM_MASK_TO_NATIVE_CLIPS 64
size_t gdkvm_mask_to_native_workspace_bytes(int clips, int T, int H, int W, int ncls);
int gdkvm_mask_to_native(const uint8_t* mask, const int32_t* sizes, const uint8_t* target, uint8_t* out, int32_t* counts,
                         size_t native_bytes, void* workspace, size_t workspace_bytes, int clips, int T, int H, int W, int ncls,
                         void* stream);

/* Take a ragged batch of NATIVE-size uint8 clips to the network's grid by an area (box) average and cast them to the model's input dtype in
 * the same pass (the front end of predict.py, and what tools/convert_camus.py --resample area writes; csrc/frames_from_native.hip).  Every
 * output is a function of integers that depends on neither the algorithm nor the schedule.
 * A native frame v [h0, w0] is uint8 with one plane; clip b has the native size (h0, w0) = sizes[b], each in 1..2048.  The grid is (H, W),
 * each in 1..1024; any ratio on either axis, enlarging included.  The rule is the box integral of the piecewise-constant image, in integers.
 * For grid row i and native row k, grid column j and native column l:
 *   1. wy(i, k) = max(0, min((i + 1) h0, (k + 1) H) - max(i h0, k H)), and wx(j, l) the same with w0 and W: the overlap of the two pixels
 *      in units of 1 / (h0 H).  Sum over k of wy(i, k) = h0 for every i; sum over i of wy(i, k) = H for every k; the non-zero k of a row i
 *      are the contiguous range floor(i h0 / H) .. ceil((i + 1) h0 / H) - 1.
 *   2. N(i, j) = sum over k, l of wy(i, k) wx(j, l) v(k, l) <= 255 h0 w0 <= 255 * 2^22 < 2^30.
 *   3. q(i, j) = floor((2 N + h0 w0) / (2 h0 w0)): the mean rounded half up.  2 N + h0 w0 < 2^32, so unsigned 32-bit words suffice
 *      everywhere; the kernel has no floating point in front of the final cast, and what it puts in the division's place is exact for
 *      every numerator below 2^32.
 *   4. out [clips, T, C, H, W], C in 1..4; every plane of a frame holds the same value (the datasets' frames are grey and the model is
 *      handed the grey value in every plane).  out_dtype GDKVM_FRAMES_U8: q itself; GDKVM_FRAMES_F32: float(q) * (1.0f / 255.0f);
 *      GDKVM_FRAMES_BF16: that fp32 value rounded once, to nearest even.  The float forms are torch.mul(bytes, 1 / 255, out = ...) of the
 *      bytes q, bit for bit.
 * So (h0, w0) == (H, W) is the identity, a constant frame stays constant, the sum over i, j of N(i, j) is H W times the sum of v, and with
 * h0 % H == 0 and w0 % W == 0 q is the rounded mean of each h0 / H x w0 / W block.
 * native is RAGGED, the layout of gdkvm_mask_to_native's target: clip b's T frames of h0 w0 bytes follow each other, and clip b + 1 follows
 * clip b.  Frames start at ANY byte address.  native_bytes = the bytes native holds; it must cover the sum over the clips of T h0 w0.  out is
 * contiguous and 16-byte aligned (a misaligned out is refused, not served) and must not overlap native.
 * sizes is a HOST int32 [clips, 2]: the entry validates every size, computes every clip's offset and band geometry itself and hands them to
 * the kernel by value in the kernel arguments, GDKVM_FRAMES_FROM_NATIVE_CLIPS clips per launch, longer batches in several launches;
 * nothing is copied to the device, nothing allocated, nothing synchronised (a capture holds the sizes).
 * gdkvm_frames_from_native_workspace_bytes is 0 for every shape and the workspace may be NULL; the pair is there so that a caller treats
 * every kernel of this family alike.  Bit-reproducible: there are no atomics at all, every sum is an integer sum in a lane's own words.  Bad
 * arguments (shape, C outside 1..4, an unknown out_dtype, a size outside 1..2048, null native, sizes or out, a misaligned out,
 * native_bytes short of the sum, out overlapping native, clips * T > 2^30) are GDKVM_ERR_SHAPE before any device call; clips == 0 is
 * GDKVM_OK without a launch.
 * Launch geometry, for tests that want shapes on both sides of it: a workgroup owns a band of grid rows of one (clip, frame) and streams
 * the native rows the band covers through LDS in chunks of at most GDKVM_FRAMES_FROM_NATIVE_CHUNK_BYTES bytes (whole native rows, 16-byte
 * loads on the grid of their addresses, a head of up to 15 bytes and a ragged tail) whose per-column sums take at most
 * GDKVM_FRAMES_FROM_NATIVE_HS_WORDS words; a band is as many grid rows as one chunk covers, at most
 * GDKVM_FRAMES_FROM_NATIVE_BAND_ROWS of them and GDKVM_FRAMES_FROM_NATIVE_ACC_WORDS accumulators.  A grid column with more than GDKVM_FRAMES_FROM_NATIVE_PART native columns is cut into
 * 2, 4, ... parts that different lanes sum, and so is a grid row with more than that many native rows.  A launch has at most
 * GDKVM_FRAMES_FROM_NATIVE_MAX_WG workgroups, which take further (clip, frame, band) items in a grid-stride loop; one kernel per
 * out_dtype. */
#define GDKVM_FRAMES_U8 0
#define GDKVM_FRAMES_F32 1
#define GDKVM_FRAMES_BF16 2
#define GDKVM_FRAMES_FROM_NATIVE_CHUNK_BYTES 16368
#define GDKVM_FRAMES_FROM_NATIVE_HS_WORDS 5120
#define GDKVM_FRAMES_FROM_NATIVE_ACC_WORDS 2048
#define GDKVM_FRAMES_FROM_NATIVE_PART 16
#define GDKVM_FRAMES_FROM_NATIVE_BAND_ROWS 256
#define GDKVM_FRAMES_FROM_NATIVE_MAX_WG 4096
#define GDKVM_FRAMES_FROM_NATIVE_CLIPS 64
size_t gdkvm_frames_from_native_workspace_bytes(int clips, int T, int C, int H, int W, int out_dtype);
int gdkvm_frames_from_native(const uint8_t* native, const int32_t* sizes, void* out, size_t native_bytes, void* workspace,
                             size_t workspace_bytes, int clips, int T, int C, int H, int W, int out_dtype, void* stream);

/* Draw a mask, its contour and optionally a second mask's contour over grey frames at each clip's NATIVE size: the picture a person looks at
 * (predict.py --overlay, eval.py's eval_stage.vis_overlay; csrc/overlay_native.hip).  Every output byte is a function of integers that
 * depends on neither the algorithm nor the schedule.
 * Per native frame of clip b, (h0, w0) = sizes[b], each in 1..2048: grey [h0, w0] uint8, mask [h0, w0] uint8, optionally ref [h0, w0]
 * uint8; ncls in 2..8, a contour width w in 1..3, alpha in 0..256, and two palettes pal [ncls][3], ref_pal [ncls][3] of bytes (R, G, B).
 *   1. A byte k is a CLASS BYTE when 1 <= k < ncls.  Class 0, the bytes >= ncls and 255 are never drawn.
 *   2. Pixel (y, x) with the class byte k is a CONTOUR PIXEL of a mask when some (dy, dx) with |dy| + |dx| <= w has (y + dy, x + dx)
 *      outside the frame, or holding a byte != k (any other byte counts as different, 255 included).  That is the class minus its
 *      4-neighbour erosion iterated w times with the outside of the frame as background; with w = 1 it is gdkvm_surface_distance's surface.
 *   3. out [h0, w0, 3] uint8, interleaved RGB; the FIRST case that applies decides the pixel, with g = grey[y][x]:
 *        a. a contour pixel of mask with the byte k:              pal[k]
 *        b. with a ref, a contour pixel of ref with the byte k':  ref_pal[k']
 *        c. mask holds a class byte k:                            channel c = (g (256 - alpha) + pal[k][c] alpha + 128) >> 8
 *        d. otherwise:                                            (g, g, g)
 * So alpha = 0 draws contours only, alpha = 256 paints the class solid, and a mask without class bytes returns the grey frame in three
 * channels.
 * grey, mask and ref are RAGGED, the layout of gdkvm_mask_to_native's out / target: clip b's T frames of h0 w0 bytes follow each other, and
 * clip b + 1 follows clip b.  out is ragged the same way with three bytes per pixel: a frame's first byte is three times its pixel offset.
 * Frames start at ANY byte address.  native_bytes = the pixel bytes each input holds (out holds 3 native_bytes); it must cover the sum over
 * the clips of T h0 w0.  out overlaps no input.  ref is optional (NULL), ref_pal is required with it.
 * sizes (int32 [clips, 2]), pal and ref_pal are HOST arrays: the entry validates every value, computes every clip's offset and band geometry
 * itself and hands them and the packed palettes to the kernel by value in the kernel arguments, GDKVM_OVERLAY_NATIVE_CLIPS clips per
 * launch, longer batches in several launches; nothing is copied to the device, nothing allocated, nothing synchronised (a capture holds
 * the sizes and the colours).
 * gdkvm_overlay_native_workspace_bytes is 0 for every shape and the workspace may be NULL; the pair is there so that a caller treats every
 * kernel of this family alike.  Bit-reproducible: no atomics, no floating point, one writer per output byte.  Bad arguments (clips < 0,
 * T < 1, null grey, mask, sizes, pal or out, ref without ref_pal, a size outside 1..2048, ncls outside 2..8, width outside 1..3, alpha
 * outside 0..256, native_bytes short of the sum, out overlapping an input, clips * T > 2^30) are GDKVM_ERR_SHAPE before any device call;
 * clips == 0 is GDKVM_OK without a launch.
 * Launch geometry, for tests that want shapes on both sides of it: a workgroup owns a band of whole native rows of one (clip, frame):
 * floor(GDKVM_OVERLAY_NATIVE_BAND_RUNS / (1 + ceil(w0 / GDKVM_OVERLAY_NATIVE_RUN))) rows -- the most whose
 * run slots, a head and ceil(w0 / 16) runs per row, give a lane at most two -- at least 1, at most GDKVM_OVERLAY_NATIVE_BAND_ROWS, and keeps the band's rows of
 * mask and ref with w rows above and below in LDS (rows outside the frame and the columns beside it are zeros there: class 0).  Every row
 * is cut into runs of GDKVM_OVERLAY_NATIVE_RUN pixels on the 16-byte grid of the ADDRESSES of out (a head of up to 15 pixels, runs of three
 * 16-byte stores, a ragged tail; heads, tails and misaligned inputs take byte accesses); a launch has at most
 * GDKVM_OVERLAY_NATIVE_MAX_WG workgroups, which take further (clip, frame, band) items in a grid-stride loop; one kernel per width, with
 * and without a ref. */
#define GDKVM_OVERLAY_NATIVE_RUN 16
#define GDKVM_OVERLAY_NATIVE_BAND_RUNS 512
#define GDKVM_OVERLAY_NATIVE_BAND_ROWS 64
#define GDKVM_OVERLAY_NATIVE_MAX_WG 4096
#define GDKVM_OVERLAY_NATIVE_CLIPS 64
size_t gdkvm_overlay_native_workspace_bytes(int clips, int T, int ncls, int width);
int gdkvm_overlay_native(const uint8_t* grey, const uint8_t* mask, const uint8_t* ref, const int32_t* sizes, const uint8_t* pal,
                         const uint8_t* ref_pal, uint8_t* out, size_t native_bytes, void* workspace, size_t workspace_bytes, int clips,
                         int T, int ncls, int width, int alpha, void* stream);

/* Surface distances between one class of a predicted mask and of its target (what HD, HD95 and ASSD are made of; csrc/surface_distance.hip).
 * Every output is an integer that depends on neither the algorithm nor the schedule; the three floating-point metrics are a few lines on top
 * (gdkvm_amd.ops.surface_metrics) and not part of this ABI.  Distances are in pixels of the masks' grid (isotropic pixels assumed).
 * Per frame mask [H, W], target [H, W] uint8, class cls (0..254), H, W in 1..1024:
 *   1. A = the pixels with mask[y][x] == cls, B = those with target[y][x] == cls; every other byte, 255 and every other class included, is
 *      "not cls".
 *   2. The SURFACE S(X) of a set X is its pixels with at least one of the four neighbours (x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)
 *      outside X.  A neighbour outside the frame is outside X.  Adjacency is geometric, as for gdkvm_largest_component: (W - 1, y) and
 *      (0, y + 1) are no neighbours, nor are pixels of two frames.  (X minus its erosion by the 4-neighbour cross with a zero border.)
 *   3. Directed squared distances, integers below 2^21:  for p in S(A)  d2_AB(p) = min over q in S(B) of (px - qx)^2 + (py - qy)^2;
 *      for q in S(B)  d2_BA(q) likewise against S(A).
 *   4. surf [frames, 8] int64 = nA = |S(A)|, nB = |S(B)|, hAB = max d2_AB, hBA = max d2_BA, sAB = sum over S(A) of isqrt(d2_AB(p) 2^32),
 *      sBA likewise, q_lo, q_hi.  isqrt(n) = floor(sqrt(n)): every term is a distance in units of 2^-16 pixel, rounded down.
 *   5. With n = nA + nB, lo = floor(95 (n - 1) / 100) and hi = min(lo + 1, n - 1):  q_lo and q_hi are the values at the 0-based ranks lo and hi
 *      of the ascending pooled multiset of all d2_AB and d2_BA (the two neighbours of the pooled 95th percentile with linear interpolation).
 *   6. nA == 0 or nB == 0: the six other fields are 0 -- the frame has no surface distance.
 * mask and target are [frames, H, W] contiguous at ANY byte address (frames of H W bytes follow each other); surf is 16-byte aligned.  The
 * workspace (16-byte aligned, at least gdkvm_surface_distance_workspace_bytes(frames, H, W) bytes) is scratch: 0 while H W <= 14336 -- a
 * frame's 4.5 bytes per pixel (one 32-bit word per pixel and four bitmaps) then live in 63 KiB of LDS, which covers the 112 x 112 mask of
 * cfg2 -- else those 4.5 bytes per pixel with each frame's slice rounded up to 128 bytes.  One workgroup per frame; neither entry allocates
 * or synchronises; bit-reproducible; every loop of the kernel is bounded by H, W, H W or a constant.  Bad arguments (shape, cls, null or
 * misaligned pointers, a short workspace) are GDKVM_ERR_SHAPE before any device call; frames == 0 is GDKVM_OK without a launch. */
size_t gdkvm_surface_distance_workspace_bytes(int frames, int H, int W);
int gdkvm_surface_distance(const uint8_t* mask, const uint8_t* target, int64_t* surf, void* workspace, size_t workspace_bytes,
                           int frames, int H, int W, int cls, void* stream);
/* The same with a pixel spacing: distances in micrometres, so that HD, HD95 and ASSD come out in mm whatever the pixels' aspect (a CAMUS
 * sequence squeezed to a square grid has pixels of about 0.33 x 0.47 mm).  spacing_um [frames, 2] int32 on the DEVICE (4-byte aligned) holds,
 * per frame, ry = the micrometres per pixel down the rows (y) and rx = along the columns (x), each in 1..4095.
 *   1, 2. A, B and the surfaces are those of gdkvm_surface_distance: the erosion is topological and knows no spacing (what medpy does with
 *      `voxelspacing`).
 *   3. d2(p, q) = (ry (py - qy))^2 + (rx (px - qx))^2 in um^2, an exact integer below 2 (1023 * 4095)^2 < 2^45.
 *   4. surf [frames, 8] int64 = nA, nB, hAB, hBA (the largest d2 per direction), sAB = sum over S(A) of isqrt(d2_AB(p) 2^16), sBA likewise
 *      (every term a distance in units of 2^-8 um, rounded down; the operand is below 2^61, a sum below 2^51), q_lo, q_hi by rule 5 above.
 *   5. nA == 0 or nB == 0: the six other fields are 0.   A frame whose ry or rx is outside 1..4095: all eight fields are -1 (the kernel
 *      cannot return an error; gdkvm_amd.ops checks a host tensor before it is copied).
 * The workspace is 0 bytes while H W <= GDKVM_SURFACE_MM_LDS_PIXELS -- a frame's 8.5 bytes per pixel (one 64-bit word per pixel: 11 bits of
 * row count, 45 of d2, 2 of multiplicity; and the four bitmaps) then live in up to 153 KiB of dynamic LDS, 104 KiB for a 112 x 112 frame --
 * else those 8.5 bytes per pixel with each frame's slice rounded up to 128 bytes.  Everything else (alignment, one workgroup per frame, no
 * allocation, bit-reproducible, bounded loops -- the bisection takes at most 45 steps --, GDKVM_ERR_SHAPE for bad arguments, a null
 * spacing_um included) is as for gdkvm_surface_distance. */
#define GDKVM_SURFACE_MM_LDS_PIXELS 18432
size_t gdkvm_surface_distance_mm_workspace_bytes(int frames, int H, int W);
int gdkvm_surface_distance_mm(const uint8_t* mask, const uint8_t* target, const int32_t* spacing_um, int64_t* surf, void* workspace,
                              size_t workspace_bytes, int frames, int H, int W, int cls, void* stream);
/* The same at every clip's NATIVE frame size: HD, HD95 and ASSD in mm against the tracing as the dataset stores it, with the spacing of the
 * native pixel (eval.py's native.surface block; csrc/surface_native.hip).  Every output is an integer that depends on neither the algorithm
 * nor the schedule.
 * Per native frame of clip b: (h0, w0) = sizes[b], each side in 1..2048; (ry, rx) = spacing_um[b], micrometres per NATIVE pixel down the
 * rows and along the columns, each in 1..4095; class cls in 0..254.  Rules 1, 2, 5 and 6 of gdkvm_surface_distance and rules 3 and 4 of
 * gdkvm_surface_distance_mm apply unchanged: A and B are the pixels of mask and target equal to cls; the surface is the 4-neighbour erosion
 * with the outside of the frame as background; adjacency is geometric, no wrap between rows and none between the frames of the ragged
 * buffer; d2(p, q) = (ry dy)^2 + (rx dx)^2 in um^2.  surf [clips T, 8] int64 = nA, nB, hAB, hBA, sAB = sum over S(A) of
 * isqrt(d2_AB(p) 2^16), sBA, q_lo, q_hi with the ranks lo = floor(95 (n - 1) / 100) and hi = min(lo + 1, n - 1) of the pooled multiset;
 * nA == 0 or nB == 0: the six other fields are 0.  So gdkvm_amd.ops.surface_metrics_mm, surface_summary and surface_stats apply to the
 * records unchanged, and on uniform clips the records are those of gdkvm_surface_distance_mm bit for bit.
 * Bounds: d2 <= 2 (2047 * 4095)^2 < 2^47, so the isqrt's operand d2 2^16 is below 2^63 (the kernel's isqrt is exact for every operand
 * below 2^63: its root is below 2^31.5, the fp64 estimate is off by at most one, and (r + 1)^2 < 2^64); a term of a sum is below 2^32 and
 * a sum below 2^54.
 * mask and target are RAGGED, exactly the layout of gdkvm_mask_to_native's out / target: clip b's T frames of h0 w0 bytes follow each other
 * and clip b + 1 follows clip b.  Frames start at ANY byte address.  native_bytes = the bytes mask and target each hold; it must cover the
 * sum over the clips of T h0 w0.  surf is 16-byte aligned.
 * sizes and spacing_um are HOST int32 [clips, 2]: the entry validates every value (so this form has no -1 record), computes every clip's
 * offsets itself and hands them with the sizes and the spacings to the kernels by value in the kernel arguments,
 * GDKVM_SURFACE_NATIVE_CLIPS clips per launch, longer batches in several launches; nothing is copied to the device, nothing allocated,
 * nothing synchronised (a capture holds the sizes and the spacings).
 * The workspace (16-byte aligned, at least gdkvm_surface_distance_native_workspace_bytes(clips, T, native_bytes, native_rows) bytes with
 * native_bytes = the sum of T h0 w0 and native_rows = the sum of T h0 over the clips) is scratch and need not be zeroed: per frame 512
 * bytes of counts, per pixel 2 bits of surface bitmaps (rows padded to whole 32-bit words, hence native_rows), two 16-bit planes and two
 * 32-bit list entries: about 12.1 bytes per pixel, an upper bound that depends on the four integers of the query only (0 for a bad query).
 * Bad arguments (clips < 0, T < 1, cls, a size outside 1..2048, a spacing outside 1..4095, null mask, target, sizes, spacing_um or surf, a
 * misaligned surf, native_bytes short of the sum, clips * T > 2^30, a null, short or misaligned workspace) are GDKVM_ERR_SHAPE before any
 * device call; clips == 0 is GDKVM_OK without a launch.  Bit-reproducible.
 * Launch geometry, for tests that want shapes on both sides of it: four kernels in stream order per launch, no workgroup waits for
 * another.  The surfaces and the walks along the rows go by BANDS of GDKVM_SURFACE_NATIVE_BAND_ROWS native rows of one (clip, frame) (the
 * surface kernel reads one halo row above and below its band); the sweeps down the columns by STRIPS of GDKVM_SURFACE_NATIVE_STRIP columns,
 * one lane per column; a frame's maxima, sums and ranks by one workgroup.  A launch has at most GDKVM_SURFACE_NATIVE_MAX_WG workgroups per
 * kernel, which take further items in a grid-stride loop. */
#define GDKVM_SURFACE_NATIVE_BAND_ROWS 32
#define GDKVM_SURFACE_NATIVE_STRIP 64
#define GDKVM_SURFACE_NATIVE_MAX_WG 4096
#define GDKVM_SURFACE_NATIVE_CLIPS 64
size_t gdkvm_surface_distance_native_workspace_bytes(int clips, int T, long long native_bytes, long long native_rows);
int gdkvm_surface_distance_native(const uint8_t* mask, const uint8_t* target, const int32_t* sizes, const int32_t* spacing_um,
                                  int64_t* surf, size_t native_bytes, void* workspace, size_t workspace_bytes, int clips, int T, int cls,
                                  void* stream);
/* gdkvm_lv_measure_mm at every clip's NATIVE frame size: EDV, ESV and EF in mL from the tracing as the dataset stores it, with the spacing
 * of the native pixel (eval.py's native.lv block; csrc/lv_native.hip).
 * Per native frame of clip b: (h0, w0) = sizes[b], each side in 1..2048; (ry, rx) = spacing_um[b], micrometres per NATIVE pixel down the
 * rows and along the columns, each in 1..4095; class cls in 0..254; D disks in 1..64; Q = 2^16.  Steps 1, 2, 3', 4, 5 and 6' of
 * gdkvm_lv_measure_mm apply to every native frame, integer for integer and fp64 operation for fp64 operation (contraction off, each
 * operation rounded once).  The records are stats [clips, T, 12] = n, sx, sy, sxx, sxy, syy, Vx, Vy, tmin, tmax, Lt, E, disks [clips, T, D]
 * = W_j and geom [clips, T, 6] = L mm, V mL, cx mm, cy mm, k um, area mm^2, that entry's layout: gdkvm_lv_ef, gdkvm_lv_beats and
 * gdkvm_lv_biplane apply to them unchanged, and on uniform clips with sides <= 1024 the three records equal gdkvm_lv_measure_mm's bit for
 * bit, doubles included.  An empty frame (n = 0) gives all 0; the entry validates every size and spacing, so this form has no -1 record.
 * The bounds the integer widths rest on, for sides up to 2048 (x, y <= 2047):
 *   - n <= 2^22;  sx, sy < 2^33;  sxx, sxy, syy < 2^44.
 *   - A = n sxx - sx^2 equals the sum over pixel pairs of (x_i - x_j)^2, which only grows with the set: its largest value is the full
 *     2048^2 frame's, 2^44 (2048^2 - 1) / 12 < 2^62.5; the same holds for C, and |B| <= sqrt(A C).  So A, B and C fit int64, but the two
 *     products n sxx and sx^2 reach 2^66: A, B and C are formed in unsigned 64-bit wrap-around arithmetic, whose difference is the exact
 *     value, never in a double.
 *   - |n x - sx| < 2^33 and |Vx|, |Vy| <= 2^16, so the projection takes 64-bit products and |t_p| < 2^50.
 *   - P1 = n E <= 2^38;  Lt = tmax - tmin + P1 < 2^51 + 2^38;  D (t_p - tmin) + D P1 and (j + 1) Lt are both below 2^58.
 *   - W_j: a pixel meets disk j only inside a slab of (L / D + 1) pixel extents along the axis, which is at most sqrt(2) (L / D + 1) + 1
 *     pixels per row or column along the frame's dominant direction, over at most 2048 of them, with L <= 4095 pixel extents; an overlap
 *     is at most D P1.  So W_j <= 2048 (sqrt(2) (4095 / D + 1) + 1) D 2^38 < 2^61.6, and sum_j W_j = n D P1 <= 2^44 D exactly.
 * mask is RAGGED, exactly the layout of gdkvm_mask_to_native's out / target: clip b's T frames of h0 w0 bytes follow each other and clip
 * b + 1 follows clip b.  Frames start at ANY byte address.  native_bytes = the bytes mask holds; it must cover the sum over the clips of
 * T h0 w0.  stats, disks, geom and bands are 16-byte aligned.
 * sizes and spacing_um are HOST int32 [clips, 2], handled as gdkvm_surface_distance_native handles them: the entry validates every value,
 * computes every clip's offsets itself and hands them with the sizes and the spacings to the kernels by value in the kernel arguments,
 * GDKVM_LV_NATIVE_CLIPS clips per launch, longer batches in several launches; nothing is copied to the device, nothing allocated, nothing
 * synchronised (a capture holds the sizes and the spacings).
 * A frame's work is spread over many workgroups: four kernels in stream order per launch over BANDS of GDKVM_LV_NATIVE_BAND_ROWS native
 * rows of one (clip, frame) -- per band the six moments; per band tmin / tmax (every workgroup adds its frame's band moments and evaluates
 * step 3' itself: the same operations on the same totals give every workgroup of a frame the same axis); per band the partial W_j (64-bit
 * integer atomics in LDS, then stored); per frame one workgroup that adds the bands and writes the records.  No workgroup waits for
 * another, no global atomics, no fences.  A launch has at most GDKVM_LV_NATIVE_MAX_WG workgroups per kernel, which take further items in a
 * grid-stride loop.
 * The per-band partials are an OUTPUT, not scratch: bands int64 [native_bands, 8 + D] with native_bands = the sum over the clips of
 * T ceil(h0 / GDKVM_LV_NATIVE_BAND_ROWS), in clip, frame, band order.  One row holds n, sx, sy, sxx, sxy, syy, tmin, tmax and W_0 ..
 * W_(D-1) restricted to the band's rows (tmin, tmax over the band's pixels with the FRAME's n, sx, sy and axis; W_j against the frame's
 * tmin and Lt).  A band without a pixel of the class in a frame that has some holds 0 moments, tmin = INT64_MAX, tmax = INT64_MIN and
 * W = 0; every band of an empty frame holds all 0.  Every word is an exact integer that depends on no schedule.  (No workspace, hence no
 * size query.)
 * clips < 0, T < 1, D outside 1..64, a size outside 1..2048, a spacing outside 1..4095, native_bytes short of the sum, native_bands not
 * equal to the sum and clips * T > 2^30 are GDKVM_ERR_SHAPE; cls outside 0..254, a null mask, sizes, spacing_um, stats, disks, geom or
 * bands and a misaligned output are GDKVM_ERR_ARG (the codes of gdkvm_lv_measure_mm); all of them before any device call.  clips == 0 is
 * GDKVM_OK without a launch.  Bit-reproducible. */
#define GDKVM_LV_NATIVE_BAND_ROWS 32
#define GDKVM_LV_NATIVE_MAX_WG 4096
#define GDKVM_LV_NATIVE_CLIPS 64
int gdkvm_lv_measure_native(const uint8_t* mask, const int32_t* sizes, const int32_t* spacing_um, int64_t* stats, int64_t* disks,
                            double* geom, int64_t* bands, size_t native_bytes, long long native_bands, int clips, int T, int cls, int D,
                            void* stream);

/* Signed squared distance maps of label frames (the operand of gdkvm_seg_loss_boundary_fwd / _bwd; csrc/signed_distance.hip).  Every output is
 * an integer that depends on neither the algorithm nor the schedule.  Distances are in pixels of the frame's grid (isotropic pixels assumed).
 * Per frame t [H, W] uint8 of target [frames, H, W] and class c in [0, C), 1 <= C <= 32, H, W in 1..1024:  A = {x : t(x) == c}; every other
 * byte, a label outside [0, C) such as 255 included, is not c and belongs to the complement.  sd2 [frames, C, H, W] int32:
 *   A empty or A = the whole frame:  s_c = 0 everywhere;
 *   x outside A:  s_c(x) = + min over y in A of |x - y|^2;        x in A:  s_c(x) = - min over y outside A of |x - y|^2.
 * So s_c(x) = 0 only where the class is absent from the frame or fills it, and |s_c| <= 2 * 1023^2.
 * The plane of a class whose bit is clear in class_mask (bit c = class c) is zero-filled.
 * target is contiguous at ANY byte address (frames of H W bytes follow each other); sd2 is 4-byte aligned.  The workspace (16-byte aligned, at
 * least gdkvm_signed_distance_workspace_bytes(frames, C, H, W) bytes) is scratch: 0 while H W <= 79872 -- a (frame, class) keeps one 16-bit word
 * per pixel (its kind and the vertical distance to the other kind in its column), which then live in up to 156 KiB of dynamic LDS (a 256 x 256
 * frame: 128 KiB) -- else those 2 bytes per pixel with each plane rounded up to 128 bytes.  One workgroup per (frame, class); neither entry
 * allocates or synchronises; no workgroup waits for another; bit-reproducible; every loop of the kernel is bounded by H, W or H W / lanes.  Bad
 * arguments (shape, C, null or misaligned pointers, a short workspace) are GDKVM_ERR_SHAPE before any device call; frames == 0 is GDKVM_OK
 * without a launch. */
size_t gdkvm_signed_distance_workspace_bytes(int frames, int C, int H, int W);
int gdkvm_signed_distance(const uint8_t* target, int32_t* sd2, void* workspace, size_t workspace_bytes,
                          int frames, int C, int H, int W, unsigned class_mask, void* stream);

/* The optimiser step (csrc/adamw.hip): multi-tensor AdamW (decoupled weight decay, torch.optim.AdamW's update) over `tensors` fp32 tensors with
 * global-norm gradient clipping, a learning-rate schedule, a non-finite guard and an optional EMA of the weights, as three kernels on `stream`.
 * params, grads, exp_avg, exp_avg_sq, ema are HOST arrays of device addresses (4-byte aligned; 16-byte aligned tensors take 16-byte accesses),
 * counts / decays HOST arrays of element counts (1 .. 2^31 - 4097) and per-tensor weight decays; element i of a tensor's gradient and moments
 * belongs to element i of its parameter BY ADDRESS.  ema may be null, and so may single entries of it; it is read only when ema_decay > 0.
 * The addresses travel to the kernels by value in the kernel arguments (a capture holds them; nothing is copied to the device), at most 76
 * tensors per launch, longer lists in several launches.
 *   1. sum of squares: one fp32 partial per 4096-element chunk of a gradient, summed in a fixed order, at the chunk's index over the whole
 *      list in the workspace (gdkvm_adamw_workspace_bytes(tensors, total elements) bytes, an upper bound; 4-byte aligned).
 *   2. finalise, in double: S = the partials summed in a fixed order, norm = sqrt(S).  S not finite (a gradient holds inf or NaN, or a square
 *      overflows fp32): apply = 0, skipped += 1, step stays.  Otherwise t = step + 1 is stored,
 *        coef  = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1                         (torch.nn.utils.clip_grad_norm_)
 *        lr(t) = lr t / W  while t <= W = warmup_steps;  past it, with s = min(1, (t - W) / max(1, total_steps - W)), r = min_lr_ratio:
 *                GDKVM_SCHEDULE_CONSTANT  lr        GDKVM_SCHEDULE_COSINE  lr (r + (1 - r) (1 + cos(pi s)) / 2)
 *                GDKVM_SCHEDULE_POLY      lr (r + (1 - r) (1 - s)^poly_power)
 *        bc1 = 1 - beta1^t, bc2 = 1 - beta2^t;  coef, lr(t), lr(t) / bc1 and sqrt(bc2) are rounded once to fp32 for the update.
 *   3. update (nothing is written when apply = 0), per element in fp32 with g' = coef g:
 *        m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g'^2;  p = p (1 - lr(t) wd) - (lr(t) / bc1) m / (sqrt(v) / sqrt(bc2) + eps);
 *        ema entry present: e = ema_decay e + (1 - ema_decay) p.     The gradient is read, never written: it keeps its unclipped values.
 * state: GDKVM_ADAMW_STATE_BYTES bytes on the device (8-byte aligned), zeroed by the caller before the first step and kept between steps:
 *   int64 step, int64 skipped, double grad_norm, double clip_coef, double lr (of the last step; a skipped step stores its norm and coef 0),
 *   then 24 bytes private to the kernels.  The caller may read it, and may write `step` between calls (a resumed run).
 * No atomics; no workgroup waits for another; nothing allocates or synchronises; bit-reproducible, and independent of the split into launches
 * and of the alignment of the tensors.  Bad arguments (null or misaligned addresses, a count outside its range, a short workspace, betas
 * outside [0, 1), negative or non-finite lr / eps / decay / max_norm / poly_power, ema_decay outside [0, 1), an unknown schedule, min_lr_ratio
 * outside [0, 1], negative step counts) are GDKVM_ERR_SHAPE before any device call; tensors == 0 is GDKVM_OK without a launch. */
enum { GDKVM_SCHEDULE_CONSTANT = 0, GDKVM_SCHEDULE_COSINE = 1, GDKVM_SCHEDULE_POLY = 2 };
#define GDKVM_ADAMW_STATE_BYTES 64
size_t gdkvm_adamw_workspace_bytes(int tensors, long long total_elems);
int gdkvm_adamw_step(const uint64_t* params, const uint64_t* grads, const uint64_t* exp_avg, const uint64_t* exp_avg_sq, const uint64_t* ema,
                     const int64_t* counts, const float* decays, int tensors, void* state, void* workspace, size_t workspace_bytes,
                     double lr, double beta1, double beta2, double eps, double max_norm, double ema_decay, double min_lr_ratio,
                     double poly_power, long long warmup_steps, long long total_steps, int schedule, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GDKVM_H */
