/*
 * fgnn_hip_pgm_bp.h — companion of fgnn_hip.h: the max-product belief-propagation baseline for the synthetic-PGM chains
 * (fgnn_amd/pgm_datapath.py: PgmDataPath.solve_bp; csrc/pgm_bp.hip).  Same conventions as the main header: plain pointers, sizes and a
 * hipStream_t; 0 on success, a negative FGNN_E* code otherwise, the message in the thread-local last-error string.  The main header,
 * its list of prototypes and FGNN_ABI_VERSION are unchanged by this file: a library that predates it lacks these two symbols only,
 * and the binding (fgnn_amd/_hip.py: bind_header) reports that as "rebuild" when one of them is called.
 */
#ifndef FGNN_HIP_PGM_BP_H
#define FGNN_HIP_PGM_BP_H

#include "fgnn_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Damped, parallel (flooding) max-product belief propagation on B chains of the model the chain-budget MAP and LP entry points of
 * the main header take: unary [B][N][2] f32 log-potentials (row stride unary_sb elements), link table pair [*][N-1][4] (row-major
 * [x_i][x_{i+1}]), caps [*][N-h+1] int32 (window w = x_w .. x_{w+h-1} holds at most caps[w] ones; cap > h-1: no constraint); pair_sb
 * / caps_sb = 0 share the input across the batch.
 *
 * No counterpart in the reference: it labels its random models with AD3 only (exactly, and by the LP relaxation) and ships no
 * max-product solver for these graphs.  The entry point exists because the network this project accelerates is presented as one that
 * emulates max-product belief propagation, so that algorithm is the baseline its decisions are to be compared with, next to the
 * LP label and the exact MAP.
 *
 * Messages are log-ratios m(1) - m(0) in f64, all 0 at the start; per iteration every message is recomputed from the previous ones
 * (link: the max over the other end; window: minus the positive part of the cap-th largest incoming value of the other members, or
 * -2^20 for a cap of 0), damped as new = damping * old + (1 - damping) * computed, and the sample stops after the iteration in which
 * the largest |new - old| is below tol (strict), or after max_iter iterations.  The steps in full, in the order of their
 * operations: csrc/pgm_bp.hip.  Outputs: labels [B][N] int64 (1 exactly where the final belief is > 0), and each where not NULL
 * beliefs [B][N] f64, status [B] int32 (0 converged, 3 iteration cap reached, 2 a negative cap: no iteration, labels and beliefs 0)
 * and iters [B] int32 (iterations performed).
 *
 * (N, h) outside what fgnn_chain_budget_bp_lds_bytes takes: FGNN_EUNSUPPORTED.  B < 0 or >= 2^31, max_iter < 0, tol not a finite
 * value >= 0, damping outside [0, 1), a negative stride, a null input or labels pointer with B > 0: FGNN_EINVAL.  B = 0 is a no-op.
 * All checks run before the launch.
 */
int fgnn_chain_budget_bp(const float* unary, int64_t unary_sb, const float* pair, int64_t pair_sb, const int32_t* caps,
                         int64_t caps_sb, int64_t B, int N, int h, int max_iter, double tol, double damping, int64_t* labels,
                         double* beliefs, int32_t* status, int32_t* iters, fgnn_stream_t stream);

/*
 * The LDS bytes one sample of fgnn_chain_budget_bp occupies (its messages, deltas, beliefs and potentials stay there for the whole
 * run), or a negative value, with the last-error string set, where the solver does not take the shape: h outside 2..13, N < h, or a
 * footprint above the workgroup's LDS.  Every 2 <= h <= 13, h <= N <= 128 is taken.  No counterpart in the reference (it has no such
 * solver); it exists so that the host side can refuse a shape before anything reaches the device, as it does for the MAP and LP
 * solvers.
 */
int64_t fgnn_chain_budget_bp_lds_bytes(int N, int h);

#ifdef __cplusplus
}
#endif
#endif
