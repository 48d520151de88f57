/*
 * fgnn_hip_ldpc_nms.h — companion of fgnn_hip.h: the learned ("neural") min-sum LDPC decoder, forward and backward
 * (fgnn_amd/ldpc_nms.py: LearnedMinSum; csrc/ldpc_nms.hip).  Same conventions as the main header: plain pointers, sizes and a
 * hipStream_t; 0 on success, a negative FGNN_E* code otherwise, the message in the thread-local last-error string.  The main header,
 * its list of prototypes and FGNN_ABI_VERSION are unchanged by this file: a library that predates it lacks these symbols only, and
 * the binding (fgnn_amd/_hip.py: bind_header) reports that as "rebuild" when one of them is called.
 *
 * No counterpart in the reference: its one classical decoder is MacKay's sum-product with nothing to train.  These entry points exist
 * because min-sum with trained normalisation weights and offsets (Nachmani et al.; Lugosch & Gross) is the learned decoder every
 * neural-decoder paper compares against, and because it trains on every code fgnn_ldpc_decode_llr takes.
 *
 * THE DECODER.  Flooding schedule, a fixed number of iterations n_iter (1..64).  The tables are fgnn_ldpc_decode_llr's: col_ptr
 * [N + 1] (edge e = col_ptr[n] + u is variable n's u-th check), row_ptr [M + 1], row_edge / row_var [E] (each check's edges and
 * variables in increasing variable order).  Parameters alpha [n_iter][W] and beta [n_iter][W], f32, shared by `share`: 0 (per
 * iteration) W = 1; 1 (per check) W = M, index = the check; 2 (per edge) W = E, index = the edge id e.  Any finite value is allowed,
 * negative ones included.
 *
 * Forward, all f32, each expression in the order written (no fused multiply-adds):
 *   load         prior[n] = llr[n]; NaN -> 0; clamped to +-4096.  T_0 = prior, R_0 = 0.
 *   iteration t  = 1..n_iter, check m with edges l = 0..L-1 in row order:
 *                q_l = T_{t-1}[var_l] - R_{t-1}[edge_l];  a = |q_l|
 *                one sweep keeps the two smallest |q| and their places, m1 = m2 = +inf and i1 = i2 = none at first:
 *                    if (a < m1) { m2 = m1; i2 = i1; m1 = a; i1 = l; } else if (a < m2) { m2 = a; i2 = l; }
 *                mag_l = (l == i1) ? m2 : m1;  u_l = alpha_t[w] * mag_l - beta_t[w];  o_l = fmaxf(u_l, 0)
 *                R_t[edge_l] = s_l * o_l, s_l negative exactly when an odd number of the OTHER q are < 0;  L = 1 sends 0.
 *                then T_t[n] = prior[n] + R_t[col_ptr[n]] + R_t[col_ptr[n] + 1] + ... in that order
 *                viol = the number of checks with an odd number of T_t[var] < 0.
 * With beta = 0 and one alpha >= 0 this is fgnn_ldpc_decode_llr's normalized min-sum with a flooding schedule, operation for
 * operation; with alpha = 1 its offset min-sum.
 *
 * Backward.  Given g_totals [n_iter][B][N], the loss's gradient with respect to every iteration's totals.  Per word, t = n_iter..1,
 * with gT_t = g_totals[t] plus what iteration t + 1 sent back, and gR_t[e] = minus iteration t + 1's g_q_e (zero at t = n_iter):
 *   g_prior[n] += gT_t[n];  g_e = gT_t[var(e)] + gR_t[e];  g_o = s_e * g_e where u_e > 0, else 0 (u_e recomputed from the record with
 *   the forward's own expression);  g_alpha_t[w] += g_o * mag_e;  g_beta_t[w] -= g_o;  g_mag = g_o * alpha_t[w];
 *   per check g_m1 = the sum of g_mag over l != i1 and g_m2 = g_mag at i1; g_m1 goes to place i1, g_m2 to place i2;
 *   g_q_l = (q_l < 0 ? -1 : +1) * that;  gT_{t-1}[var_l] += g_q_l;  at t = 0 the rest of gT_0 goes to g_prior.  L = 1 contributes
 *   nothing.  g_llr = g_prior, zero where the load clamped or replaced a NaN.
 * The batch sums of g_alpha / g_beta use no floating-point atomics: each workgroup takes the words b = g, g + G, ... of its own,
 * accumulates into a partial of its own, and a second launch adds the G partials in a fixed order (eight interleaved runs g = k, k + 8,
 * ..., then the eight sums in the order of k).  Two calls on the same inputs return the same bits.  Gradients are unspecified where totals left the finite range.
 */
#ifndef FGNN_HIP_LDPC_NMS_H
#define FGNN_HIP_LDPC_NMS_H

#include "fgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The forward of B words from llr [B][N] f32 (row stride llr_sb elements), in one launch, one workgroup per word.
 *   decode  stop_early = 1: a word stops after the first iteration with viol = 0.  Outputs x [B][N] uint8 (T < 0), post [B][N] f32
 *           (the final T; or NULL), viol [B] int32, iters [B] int32 (iterations run, >= 1).  totals and record must be NULL.
 *   train   stop_early = 0: every word runs all n_iter iterations.  Writes totals [n_iter][B][N] f32 (T_t for every t) and the record
 *           the backward reads (record_bytes >= fgnn_ldpc_nms_record_bytes(...); its layout is private to csrc/ldpc_nms.hip).  x, post,
 *           viol and iters are written where not NULL (iters = n_iter).
 * No counterpart in the reference (see the head of this file).
 *
 * N or M outside 1..1024, E outside 1..16 min(N, M): FGNN_EUNSUPPORTED.  n_iter outside 1..64, share outside 0..2, stop_early outside
 * 0..1, a negative stride, B < 0 or >= 2^31, a null required pointer with B > 0, totals or record given in decode mode, a record
 * smaller than the query says: FGNN_EINVAL.  Weights are not inspected on the host.  B = 0 is a no-op.  All checks run before the launch.
 */
int fgnn_ldpc_nms_forward(const float* llr, int64_t llr_sb, const int32_t* col_ptr, const int32_t* row_ptr, const int32_t* row_edge,
                          const int32_t* row_var, const float* alpha, const float* beta, int64_t B, int N, int M, int E, int n_iter,
                          int share, int stop_early, uint8_t* x, float* post, int32_t* viol, int32_t* iters, float* totals,
                          void* record, int64_t record_bytes, fgnn_stream_t stream);

/*
 * The backward of a train-mode forward (same llr, tables, weights, sizes and record): g_alpha, g_beta [n_iter][W] f32, summed over the
 * batch, and, where g_llr is not NULL, g_llr [B][N] f32 (llr may be NULL when g_llr is).  workspace: at least
 * fgnn_ldpc_nms_backward_workspace_bytes(...) bytes of device memory, 16-byte aligned, contents irrelevant before and after.  Two
 * launches: fgnn_ldpc_nms_backward_workgroups(B) workgroups over the words, then the sum of their partials.
 * No counterpart in the reference (see the head of this file).
 *
 * Refusals as fgnn_ldpc_nms_forward's; a workspace smaller than the query says: FGNN_EINVAL.  B = 0 writes zeros to g_alpha and g_beta
 * (null pointers: a no-op).
 */
int fgnn_ldpc_nms_backward(const float* g_totals, const float* llr, int64_t llr_sb, const int32_t* col_ptr, const int32_t* row_ptr,
                           const int32_t* row_edge, const int32_t* row_var, const float* alpha, const float* beta, const void* record,
                           int64_t record_bytes, int64_t B, int N, int M, int E, int n_iter, int share, float* g_alpha, float* g_beta,
                           float* g_llr, void* workspace, int64_t workspace_bytes, fgnn_stream_t stream);

/*
 * The bytes of the record a train-mode forward of these sizes writes (three 32-bit values per word, iteration and check), or a
 * negative value, with the last-error string set, where a size is refused.  No counterpart in the reference.
 */
int64_t fgnn_ldpc_nms_record_bytes(int64_t B, int N, int M, int E, int n_iter);

/*
 * The bytes of workspace fgnn_ldpc_nms_backward needs (one partial of g_alpha and g_beta per workgroup), or a negative value, with the
 * last-error string set, where a size is refused.  No counterpart in the reference.
 */
int64_t fgnn_ldpc_nms_backward_workspace_bytes(int64_t B, int N, int M, int E, int n_iter, int share);

/*
 * The LDS bytes one word's state occupies in the forward (backward = 0) or the backward (1; the partial of g_alpha / g_beta comes on
 * top where it fits), sized from the code, or a negative value, with the last-error string set, where the shape is not taken.
 * No counterpart in the reference.
 */
int64_t fgnn_ldpc_nms_lds_bytes(int N, int M, int E, int backward);

/*
 * The number of workgroups fgnn_ldpc_nms_backward launches over B words: workgroup g takes the words g, g + G, ...
 * No counterpart in the reference.
 */
int64_t fgnn_ldpc_nms_backward_workgroups(int64_t B);

#ifdef __cplusplus
}
#endif
#endif
