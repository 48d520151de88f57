/*
 * fgnn_hip_ldpc_nms_layered.h — companion of fgnn_hip.h and fgnn_hip_ldpc_nms.h: the learned min-sum LDPC decoder with a layered
 * schedule, forward and backward (fgnn_amd/ldpc_nms.py: LearnedMinSum(schedule='layered'); csrc/ldpc_nms_layered.hip).  Same
 * conventions as the main header.  The main header, fgnn_hip_ldpc_nms.h, their lists of prototypes and FGNN_ABI_VERSION are unchanged
 * by this file: a library that predates it lacks these symbols only, and the binding (fgnn_amd/_hip.py: bind_header) reports that as
 * "rebuild" when one of them is called.
 *
 * No counterpart in the reference: its one classical decoder is MacKay's sum-product with a flooding schedule and nothing to train.
 * These entry points exist because layered neural min-sum is the variant neural-decoder papers and hardware use when iterations are
 * scarce, and because fgnn_ldpc_decode_llr's layered min-sum, the fixed decoder the trained one is held against, decodes more words
 * in fewer iterations than its flooding one.
 *
 * THE DECODER.  Tables as fgnn_ldpc_decode_llr's: col_ptr [N + 1], row_ptr [M + 1], row_edge / row_var [E]; layer_ptr
 * [n_layers + 1], layer_chk [M]: the checks of layer k are layer_chk[layer_ptr[k] .. layer_ptr[k + 1] - 1], every check in exactly
 * one layer, no two checks of a layer sharing a variable (the caller's duty, LdpcCode.layers() gives such tables; not inspected).
 * Weights alpha, beta [n_iter][W] f32 indexed by `share` exactly as in fgnn_hip_ldpc_nms.h (0: W = 1; 1: W = M, by check; 2: W = E,
 * by edge id).
 *
 * Forward, all f32, each expression in the order written (no fused multiply-adds):
 *   load         prior[n] = llr[n]; NaN -> 0; clamped to +-4096.  T = prior, R = 0.
 *   iteration t  = 1..n_iter runs the layers k = 0..n_layers-1 in order; within a layer every check m of it, over its edges
 *                l = 0..L-1 in row order:
 *                q_l = T[var_l] - R[edge_l]   (the current values: they hold the updates of this iteration's earlier layers)
 *                one sweep keeps the two smallest |q| and their places, as in fgnn_hip_ldpc_nms.h: m1, i1, m2, i2
 *                mag_l = (l == i1) ? m2 : m1;  u_l = alpha_t[w] * mag_l - beta_t[w];  o_l = fmaxf(u_l, 0)
 *                R'_l = s_l * o_l, s_l negative exactly when an odd number of the OTHER q are < 0;  L = 1 sends R'_l = 0
 *                R[edge_l] = R'_l;  T[var_l] = q_l + R'_l
 *                after the last layer: T_t = T (written to totals[t] in train mode); viol = the number of checks with an odd number
 *                of T[var] < 0.
 * With beta = 0 and one alpha >= 0 this is fgnn_ldpc_decode_llr's layered normalized min-sum, operation for operation; with
 * alpha = 1 its layered offset min-sum.
 *
 * Backward.  Given g_totals [n_iter][B][N].  Per word, gT [N] and gR [E] start at zero.  For t = n_iter..1:
 *   1. gT[n] += g_totals[t][n].
 *   2. the layers k = n_layers-1..0, every check of the layer.  For L > 1:
 *        g_e = gT[var_l] + gR[edge_l];  g_o = s_l * g_e where u_l > 0, else 0 (u recomputed from the record with the forward's own
 *        expression);  g_alpha_t[w] += g_o * mag_l;  g_beta_t[w] -= g_o;  g_mag = g_o * alpha_t[w];
 *        g_m1 = the sum of g_mag over l != i1 and goes to place i1, g_m2 = g_mag at i1 and goes to place i2, every other place gets 0;
 *        g_q_l = gT[var_l] + (q_l < 0 ? -1 : +1) * (that)            (the first term because T' = q + R')
 *      For L = 1: g_q_l = gT[var_l], and nothing goes to the weights.
 *      Then gT[var_l] = g_q_l and gR[edge_l] = -g_q_l: overwrites, the check being the only reader of both inside its layer.
 *   3. after t = 1, g_llr[n] = gT[n], zero where the load clamped or replaced a NaN.
 * There is no g_prior accumulator and no variable pass.  The batch sums of g_alpha / g_beta are formed as fgnn_ldpc_nms_backward's:
 * no floating-point atomics, one partial per workgroup, the same second launch; two calls on the same inputs return the same bits.
 * Gradients are unspecified where totals left the finite range.
 *
 * The record has fgnn_ldpc_nms_forward's size and the workspace fgnn_ldpc_nms_backward's: fgnn_ldpc_nms_record_bytes,
 * fgnn_ldpc_nms_backward_workspace_bytes and fgnn_ldpc_nms_backward_workgroups answer for these calls too.  A record is read by the
 * backward of the schedule that wrote it.
 */
#ifndef FGNN_HIP_LDPC_NMS_LAYERED_H
#define FGNN_HIP_LDPC_NMS_LAYERED_H

#include "fgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * fgnn_ldpc_nms_forward with the layered schedule: its parameters, decode (stop_early = 1) and train (0) modes and outputs, with the
 * layer tables behind row_var.  One launch, one workgroup per word, one barrier per layer and one for viol per iteration.
 * No counterpart in the reference (see the head of this file: its decoder has one schedule and no weights).
 *
 * Refusals: fgnn_ldpc_nms_forward's; in addition n_layers outside 1..M, or a null layer table with B > 0: FGNN_EINVAL.  B = 0 is a
 * no-op.  All checks run before the launch.
 */
int fgnn_ldpc_nms_layered_forward(const float* llr, int64_t llr_sb, const int32_t* col_ptr, const int32_t* row_ptr,
                                  const int32_t* row_edge, const int32_t* row_var, const int32_t* layer_ptr, const int32_t* layer_chk,
                                  int n_layers, const float* alpha, const float* beta, int64_t B, int N, int M, int E, int n_iter,
                                  int share, int stop_early, uint8_t* x, float* post, int32_t* viol, int32_t* iters, float* totals,
                                  void* record, int64_t record_bytes, fgnn_stream_t stream);

/*
 * The backward of a train-mode fgnn_ldpc_nms_layered_forward (same llr, tables, weights, sizes and record): fgnn_ldpc_nms_backward's
 * parameters and outputs, with the layer tables behind row_var.  Two launches: fgnn_ldpc_nms_backward_workgroups(B) workgroups over
 * the words, then fgnn_ldpc_nms_backward's sum of their partials.
 * No counterpart in the reference (see the head of this file: nothing there is trained by a decoder's backward).
 *
 * Refusals: fgnn_ldpc_nms_backward's and the two of the layered forward.  B = 0 writes zeros to g_alpha and g_beta (null pointers:
 * a no-op).
 */
int fgnn_ldpc_nms_layered_backward(const float* g_totals, const float* llr, int64_t llr_sb, const int32_t* col_ptr,
                                   const int32_t* row_ptr, const int32_t* row_edge, const int32_t* row_var, const int32_t* layer_ptr,
                                   const int32_t* layer_chk, int n_layers, const float* alpha, const float* beta, const void* record,
                                   int64_t record_bytes, int64_t B, int N, int M, int E, int n_iter, int share, float* g_alpha,
                                   float* g_beta, float* g_llr, void* workspace, int64_t workspace_bytes, fgnn_stream_t stream);

/*
 * The LDS bytes of one word's state, or a negative value, with the last-error string set, where the shape is not taken.  With
 * r16(v) = v rounded up to a multiple of 16:
 *   forward  (backward = 0)  r16(4 (2 E + 2 N) + 16) + r16(2 ((M + 1) + (N + 1) + M + (M + 1)))
 *            f32 R [E], T [N], prior [N], the packed row table [E], 4 wave counts; 16-bit row_ptr, col_ptr, layer_chk, layer_ptr
 *   backward (backward = 1)  r16(4 (2 E + N) + 32) + r16(2 ((M + 1) + M + (M + 1)))
 *            f32 gR [E], gT [N], the packed row table [E], 8 wave sums; 16-bit row_ptr, layer_chk, layer_ptr (no prior, no col_ptr:
 *            there is no variable pass).  The partial of g_alpha / g_beta, 8 n_iter W bytes, comes on top while the sum stays
 *            within 64 KiB; else it lies in the workspace.
 * No counterpart in the reference (a size query of kernels it does not have).
 */
int64_t fgnn_ldpc_nms_layered_lds_bytes(int N, int M, int E, int backward);

#ifdef __cplusplus
}
#endif
#endif
