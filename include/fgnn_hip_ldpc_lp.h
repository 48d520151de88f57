/*
 * fgnn_hip_ldpc_lp.h — companion of fgnn_hip.h: the ADMM linear-programming LDPC decoder (fgnn_amd/ldpc_decoders.py:
 * LdpcDecoders.decode_lp; csrc/ldpc_lp.hip).  Same conventions as the main header: plain pointers, sizes and a hipStream_t; 0 on
 * success, a negative FGNN_E* code otherwise, the message in the thread-local last-error string.  The main header, its list of
 * prototypes and FGNN_ABI_VERSION are unchanged by this file: a library that predates it lacks these two symbols only, and the binding
 * (fgnn_amd/_hip.py: bind_header) reports that as "rebuild" when one of them is called.
 */
#ifndef FGNN_HIP_LDPC_LP_H
#define FGNN_HIP_LDPC_LP_H

#include "fgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Decodes B received words of an (N variables, M checks, E edges) LDPC code from their log-likelihood ratios llr [B][N] f32 =
 * log P(bit = 0) / P(bit = 1) (row stride llr_sb elements) by ADMM on Feldman's linear-programming relaxation (Barman, Liu, Draper &
 * Recht 2013), with the penalty term of Liu & Draper's penalised decoder (penalty = 0: the plain LP) and over-relaxation.  The
 * incidence tables are fgnn_ldpc_decode_llr's: col_ptr [N + 1] (edge e = col_ptr[n] + u is variable n's u-th check), row_ptr [M + 1],
 * row_edge / row_var [E] (each check's edges and variables in increasing variable order).
 *
 * No counterpart in the reference: it has no LP decoder.  This entry point exists because the LP relaxation is the baseline the
 * paper's own argument (MAP inference and its relaxations) points at, and the one decoder whose answer can prove itself
 * maximum-likelihood: an integral LP optimum is the ML codeword (Feldman's ML certificate).
 *
 * All state is f32.  g[n] = llr[n] (NaN -> 0, then clamped to +-4096); per edge z[e] = 0.5 and u[e] = 0 (u: the scaled dual lambda /
 * mu).  Parameters: mu > 0, penalty a >= 0, relax rho in [1, 2), eps (any finite value; eps < 0 switches the residual rule off, since res and dz are never negative), max_iter >=
 * 1, stop_on_codeword 0 or 1.  Iteration k = 1 ..
 * max_iter:
 *   variable pass  for every variable n of degree d_n >= 1: t = sum of (z[e] - u[e]) over e = col_ptr[n] .. in that order, then
 *                  x[n] = clip((t - g[n] / mu - a / mu) / (d_n - 2 a / mu), 0, 1); a variable of degree 0 takes x = (g < 0).
 *                  THE CALLER guarantees that 2 a / mu is smaller than the smallest positive variable degree (the quadratic in x[n] is
 *                  convex only then); this function cannot see the degrees without reading device memory and does not check it
 *                  (fgnn_amd.ldpc_decoders.check_decode_lp_args does, from the code).  Violating it gives meaningless x, nothing worse.
 *   check pass     for every check, over its edges l in row-table order: w_l = rho x[var_l] + (1 - rho) z_l + u_l, z' = P(w),
 *                  u_l = w_l - z'_l.  The word's res = max |x[var_l] - z'_l| and dz = max |z'_l - z_l| over all edges.  Then z = z'.
 *   decision       xh[n] = x[n] > 0.5; viol = the number of checks of odd parity in xh.
 * A word stops when res <= eps and dz <= eps (the residual rule: flag bit 0), or stop_on_codeword is set and viol = 0, or k reaches
 * max_iter.  Flag bit 1 = bit 0 and min(x[n], 1 - x[n]) <= 1e-3 for every n; with penalty = 0 that bit is the ML certificate.
 *
 * P is the Euclidean projection onto the parity polytope (the convex hull of the even-weight 0/1 vectors of length d), by cut search
 * (Zhang & Siegel 2013): c = clip(w, 0, 1); f_l = w_l > 0.5; if |f| is even, f is flipped at the first l with the smallest
 * |w_l - 0.5|; theta_l = +1 where f_l, else -1; p = |f| - 1.  If theta . c <= p the result is c; otherwise it is clip(w - beta theta,
 * 0, 1) for the beta > 0 with theta . clip(w - beta theta, 0, 1) = p.  That function of beta is non-increasing and piecewise linear
 * with the 2 d breakpoints {w_l - 1, w_l} (theta_l = +1) and {-w_l, 1 - w_l} (theta_l = -1): it is evaluated at every positive
 * breakpoint, the largest breakpoint where it is still above p and the smallest where it is not are kept, and beta is interpolated
 * linearly between them (the upper one if the two values are equal).  A check of degree 1 gives z = 0 by the same steps.  The steps in
 * the order of their operations: csrc/ldpc_lp.hip.
 *
 * Outputs: x [B][N] uint8 (xh), soft [B][N] f32 (the final x; or NULL), viol [B] int32, iters [B] int32 (iterations run, >= 1),
 * flags [B] int32.
 *
 * N or M outside 1..1024, E outside 1..16 min(N, M) (degrees are at most 16), or a word state above 160 KiB of LDS (z, u and the row
 * table are three E-word arrays, so the largest E do not fit): FGNN_EUNSUPPORTED, as fgnn_ldpc_decode_lp_lds_bytes says beforehand.
 * max_iter < 1, mu not finite or <= 0, penalty not finite or negative, eps not finite, relax outside [1, 2), stop_on_codeword outside 0..1, a
 * negative stride, B < 0 or >= 2^31, a null required pointer with B > 0: FGNN_EINVAL.  B = 0 is a no-op.  All checks run before the
 * launch.
 */
int fgnn_ldpc_decode_lp(const float* llr, int64_t llr_sb, const int32_t* col_ptr, const int32_t* row_ptr, const int32_t* row_edge,
                        const int32_t* row_var, int64_t B, int N, int M, int E, int max_iter, float mu, float penalty, float relax,
                        float eps, int stop_on_codeword, uint8_t* x, float* soft, int32_t* viol, int32_t* iters, int32_t* flags,
                        fgnn_stream_t stream);

/*
 * The LDS bytes one word of fgnn_ldpc_decode_lp occupies (z, u, x, g and the staged tables stay there for the whole run; sized from
 * the code, not from the limits), or a negative value, with the last-error string set, where the decoder does not take the shape: N
 * or M outside 1..1024, E outside 1..16 min(N, M), or more than 160 KiB.  No counterpart in the reference (it has no such decoder); it
 * exists so that the host side can refuse a code before anything reaches the device.
 */
int64_t fgnn_ldpc_decode_lp_lds_bytes(int N, int M, int E);

#ifdef __cplusplus
}
#endif
#endif
