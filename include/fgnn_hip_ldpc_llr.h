/*
 * fgnn_hip_ldpc_llr.h — companion of fgnn_hip.h: the LLR-domain LDPC decoders (fgnn_amd/datapath.py: LdpcDataPath.decode_llr;
 * csrc/ldpc_llr.hip).  Same conventions as the main header: plain pointers, sizes and a hipStream_t; 0 on success, a negative FGNN_E*
 * code otherwise, the message in the thread-local last-error string.  The main header, its list of prototypes and FGNN_ABI_VERSION
 * are unchanged by this file: a library that predates it lacks these two symbols only, and the binding (fgnn_amd/_hip.py:
 * bind_header) reports that as "rebuild" when one of them is called.
 */
#ifndef FGNN_HIP_LDPC_LLR_H
#define FGNN_HIP_LDPC_LLR_H

#include "fgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Decodes B received words of an (N variables, M checks, E edges) LDPC code from their log-likelihood ratios llr [B][N] f32 =
 * log P(bit = 0) / P(bit = 1) (row stride llr_sb elements), by normalized min-sum (algorithm 0: alpha), offset min-sum (1: beta)
 * or LLR-domain sum-product (2), with a flooding schedule (n_layers = 0; layer_ptr / layer_chk may be NULL) or a layered one
 * (layer_ptr [n_layers + 1], layer_chk [M]: the checks of layer k are layer_chk[layer_ptr[k] .. layer_ptr[k + 1] - 1], and no two
 * checks of a layer share a variable).  The incidence tables are fgnn_ldpc_decode's: col_ptr [N + 1] (edge e = col_ptr[n] + u is
 * variable n's u-th check), row_ptr [M + 1], row_edge / row_var [E] (each check's edges and variables in increasing variable order).
 *
 * No counterpart in the reference: its one classical decoder is MacKay's probability-domain sum-product in float64 with a flooding
 * schedule (fgnn_ldpc_decode restates it bit for bit).  This entry point exists because normalized / offset min-sum and layered
 * schedules are what LDPC papers and hardware use as the baseline, and because the f64 decoder's edge limit (1024) refuses most
 * codes the data path takes.
 *
 * All state is f32.  prior[n] = llr[n] (NaN -> 0, then clamped to +-4096); totals T[n] = prior[n]; messages R[e] = 0.  One check
 * update forms q_l = T[var] - R[edge] over the check's edges and sends R'_l = s_l * alpha * min_{k != l} |q_k| (0), s_l * max(min_{k
 * != l} |q_k| - beta, 0) (1), s_l the product of the other signs (negative exactly when q < 0), or 2 atanhf(clamp(prod_{k != l}
 * tanhf(q_k / 2), +-(1 - 2^-24))) (2: prefix times suffix products, no division); a check of degree 1 sends 0.  A flooding iteration
 * updates every check from the old totals, then T[n] = prior[n] + R[col_ptr[n]] + R[col_ptr[n] + 1] + ...; a layered iteration takes
 * the layers in order and each check stores R[e] = R'_l and T[var] = q_l + R'_l at once.  After each iteration x[n] = T[n] < 0 and
 * viol = the number of checks of odd parity; a word stops when viol = 0 or after max_iter iterations.  The steps in full, in the
 * order of their operations, and what an overflow of min-sum totals past the f32 range does (a NaN is skipped by the minimum):
 * csrc/ldpc_llr.hip.  Outputs: x [B][N] uint8, post [B][N] f32 (the final T; or NULL), viol [B] int32,
 * iters [B] int32 (iterations run, >= 1).
 *
 * N or M outside 1..1024, E outside 1..16384 (degrees are at most 16), algorithm outside 0..2: FGNN_EUNSUPPORTED, as
 * fgnn_ldpc_decode_llr_lds_bytes says beforehand.  max_iter < 1, alpha or beta not finite or negative, a negative stride, n_layers
 * outside 0..M, B < 0 or >= 2^31, a null required pointer with B > 0 (the layer tables are required when n_layers > 0):
 * FGNN_EINVAL.  B = 0 is a no-op.  All checks run before the launch.
 */
int fgnn_ldpc_decode_llr(const float* llr, int64_t llr_sb, const int32_t* col_ptr, const int32_t* row_ptr, const int32_t* row_edge,
                         const int32_t* row_var, const int32_t* layer_ptr, const int32_t* layer_chk, int n_layers, int64_t B, int N,
                         int M, int E, int algorithm, int max_iter, float alpha, float beta, uint8_t* x, float* post, int32_t* viol,
                         int32_t* iters, fgnn_stream_t stream);

/*
 * The LDS bytes one word of fgnn_ldpc_decode_llr occupies (messages, totals, priors and the staged tables stay there for the whole
 * run; sized from the code, not from the limits), or a negative value, with the last-error string set, where the decoder does not
 * take the shape: N or M outside 1..1024, E outside 1..16384.  No counterpart in the reference (it has no such decoder); it exists
 * so that the host side can refuse a code before anything reaches the device.
 */
int64_t fgnn_ldpc_decode_llr_lds_bytes(int N, int M, int E);

#ifdef __cplusplus
}
#endif
#endif
