// gdr_general.hpp -- training at key widths above 64 (gdr_wide_keys): the history-writing forward of gdr_general.hip and the backward of
// gdr_general_bwd.hip, behind gdkvm_scan_train_workspace_bytes / _fwd / _bwd (gdr_train.hip).  Not part of the C ABI.
#pragma once
#include "gdkvm_common.hpp"

// gdr_general_scan_kernel with the state before every frame written to s_hist [B,T,Hh,Dk,Dv] fp32 (shapes checked by the caller)
int gdr_general_scan_fwd_hist(const void* q, const void* k, const void* v, const float* alpha, const float* beta, const float* s_in,
                              void* r_out, float* s_out, float* s_hist, int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype, int rule,
                              int flags, hipStream_t st);

// The one training workspace at wide keys, NS = Dv / 16 state slices, FH = B*T*Hh frame-heads, every region rounded up to 256 bytes:
//   hist [B,T,Hh,Dk,Dv] fp32       the state before every frame (the forward writes it, the backward reads it)
//   e    [B*Hh][NS][N][16] fp32    the backward's per-frame scratch: the delta rules' error rows of the frame being walked
//   pk, pq [NS][FH*N][Dk] fp32     per-slice partial gradients w.r.t. the normalised keys / queries
//   pb   [NS][FH*N] fp32, pa [NS][FH] fp32   per-slice partial gradients w.r.t. beta and alpha (after the sigmoid)
size_t gdr_general_train_workspace_bytes(int B, int T, int Hh, int N, int Dk, int Dv);
float* gdr_general_train_hist(void* ws);

// gradients of gdr_general_scan_fwd_hist (shapes and workspace size checked by the caller; the workspace as the forward left it)
int gdr_general_train_bwd(const void* q, const void* k, const void* v, const float* alpha, const float* beta, const void* d_r,
                          const float* d_s_out, void* d_q, void* d_k, void* d_v, float* d_alpha, float* d_beta, float* d_s_in, void* ws,
                          int B, int T, int Hh, int N, int Dk, int Dv, int io_dtype, int rule, int flags, hipStream_t st);
