/*
 * fgnn_hip_ldpc_osd.h — companion of fgnn_hip.h: ordered-statistics reprocessing behind a message-passing LDPC decoder ("BP-OSD";
 * fgnn_amd/datapath.py: LdpcDataPath.decode_osd; csrc/ldpc_osd.hip).  Same conventions as the main header: plain pointers, sizes
 * and a hipStream_t; 0 on success, a negative FGNN_E* code otherwise, the message in the thread-local last-error string.  The main
 * header, its list of prototypes and FGNN_ABI_VERSION are unchanged by this file: a library that predates it lacks these two symbols
 * only, and the binding (fgnn_amd/_hip.py: bind_header) reports that as "rebuild" when one of them is called.
 */
#ifndef FGNN_HIP_LDPC_OSD_H
#define FGNN_HIP_LDPC_OSD_H

#include "fgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Fossorier-Lin ordered-statistics decoding of order 0, 1 or 2 for B words of a binary linear code given by its parity-check matrix
 * H in CSR form: row_ptr [M + 1], row_var [E] (fgnn_ldpc_decode_llr's tables; the variables of a row are distinct; any H, irregular
 * and M > N included).  rel [B][N] f32 (row stride rel_sb elements) orders the positions and gives the hard decisions, typically a
 * decoder's posteriors; metric [B][N] f32 (row stride metric_sb; NULL: rel) is what candidates are scored against, typically the
 * channel LLRs; viol [B] (or NULL: every word is reprocessed) is the decoder's violated-check count.
 *
 * No counterpart in the reference: it has message-passing decoders only.  This entry point exists because BP followed by OSD is the
 * standard near-maximum-likelihood baseline on short codes, the yardstick for how much of the gap a learned decoder can still win.
 *
 * Every deciding operation is an integer one, so the result is defined bit for bit.  Per word:
 *   q(v) = 0 for a NaN, else (uint32)(fminf(fabsf(v), 4096.0f) * 256.0f) (truncated; at most 2^20).
 *   w[n] = q(rel[n]), h[n] = rel[n] < 0, wm[n] = q(metric[n]), hc[n] = metric[n] < 0; d = h ^ hc, sw[n] = d[n] ? -wm[n] : wm[n],
 *   C0 = sum wm[n] d[n].  The cost of a candidate x is sum wm[n] (x[n] ^ hc[n]) <= 2^30.
 *   viol given and viol[b] == 0: x = h, cost = C0, pattern = -1, nothing else.
 *   The positions are sorted by (w[n], n) ascending.  [H | s], s = H h, is brought to reduced form by Gauss-Jordan elimination over
 *   GF(2), the columns taken in that order: a column is a pivot exactly when a row not yet used has a one in it, and is then cleared
 *   from every other row.  piv_i: the pivot columns in the order found, s'_i the reduced syndrome bit and a_i(c) the reduced entry of
 *   pivot row i; f_0, f_1, ...: the other columns in the same order; L = min(span, N - rank).
 *   Candidate 0 flips piv_i where s'_i = 1; for order >= 1 candidate 1 + j (j < L) flips f_j and piv_i where s'_i ^ a_i(f_j) = 1; for
 *   order 2 the pairs j < k follow in lexicographic order from 1 + L and flip f_j, f_k and piv_i where s'_i ^ a_i(f_j) ^ a_i(f_k) = 1.
 *   A candidate costs C0 + sum sw over what it flips; the one with the smallest (cost, index) gives x = h ^ flips, cost and
 *   pattern = its index.  Every reprocessed x satisfies every check.
 * Outputs: x [B][N] uint8, cost [B] int32, pattern [B] int32.
 *
 * N or M outside 1..1024, E outside 1..16 min(N, M), order outside 0..2, order 2 with span > 256: FGNN_EUNSUPPORTED.  span < 1, a
 * negative stride, B < 0 or >= 2^31, a null required pointer with B > 0: FGNN_EINVAL.  B = 0 is a no-op.  All checks run before the
 * launch, which allocates nothing and does not synchronise.
 */
int fgnn_ldpc_osd(const float* rel, int64_t rel_sb, const float* metric, int64_t metric_sb, const int32_t* viol,
                  const int32_t* row_ptr, const int32_t* row_var, int64_t B, int N, int M, int E, int order, int span,
                  uint8_t* x, int32_t* cost, int32_t* pattern, fgnn_stream_t stream);

/*
 * The LDS bytes one word of fgnn_ldpc_osd occupies (the bit-packed augmented matrix, the weights, the order and the pivot tables), or
 * a negative value, with the last-error string set, where N or M is outside 1..1024.  No counterpart in the reference (it has no such
 * decoder); it exists so that the host side can refuse a code before anything reaches the device.
 */
int64_t fgnn_ldpc_osd_lds_bytes(int N, int M);

#ifdef __cplusplus
}
#endif
#endif
