// pgm_bp.hip — max-product belief propagation on the synthetic-PGM chains: the algorithm the factor-graph network is said to emulate,
// as a baseline beside the exact MAP (pgm_datapath.hip) and the LP relaxation (pgm_lp.hip).  The reference ships no max-product
// solver for these graphs (it labels with AD3 only), so this one is derived here and restated in tests/pgm_bp_oracle.py.
//
//   fgnn_chain_budget_bp    damped flooding max-product per sample: labels, beliefs, status, iterations
//
// The model is fgnn_chain_budget_map's: unary [B][N][2], link table pair [B][N-1][4] (row-major [x_i][x_{i+1}]), caps [B][N-h+1]
// int32 (window w = x_w .. x_{w+h-1} holds at most caps[w] ones); a batch stride of 0 shares an input across the batch.
//
// Messages are log-ratios m(1) - m(0), all 0 at the start, all updated in parallel from the previous iteration's.  One iteration:
//   1. beliefs  bel_i = u_i (= unary[i][1] - unary[i][0]) + the message from link i-1 (i > 0) + the message from link i (i < N-1)
//      + the messages from windows w = max(0, i-h+1) .. min(i, N-h) in ascending w; added in that order.
//   2. variable-to-factor  delta = bel_i - (that factor's message to i).
//   3. link i, table t = pair[i]:  to x_{i+1}: f = max(t[1], t[3] + d) - max(t[0], t[2] + d), d the delta from x_i;
//                                  to x_i:     f = max(t[2], t[3] + d) - max(t[0], t[1] + d), d the delta from x_{i+1}.
//   4. window w with cap c to its member j, over the deltas of the OTHER h-1 members:  c > h-1: f = 0;  c == 0: f = -BP_FORCE;
//      otherwise f = -max(0, the c-th largest of the others) — the exact max-marginal ratio of an at-most-c factor (with x_j = 1
//      the others may hold c-1 ones, with x_j = 0 c of them: the difference of the two best sums is minus the c-th largest, if
//      that one is positive).  The c-th largest is found by rank counts against the other members: no sort, no scratch.
//   5. damping  new = damping * old + (1 - damping) * f, with 1 - damping formed once.
//   6. change = the largest |new - old| over the sample's messages; the sample stops after this iteration when change < tol
//      (strict: tol = 0 always runs max_iter iterations).
// After the last iteration the beliefs are formed once more (step 1); x_i = 1 exactly when bel_i > 0.
//
// status 0 converged, 3 the iteration cap reached, 2 a negative cap (no iteration, labels 0, beliefs 0: as fgnn_chain_budget_lp).
//
// Arithmetic: inputs read as f32, everything in f64, this file built with -ffp-contract=off; each expression in the order written.
// `change` is a maximum (lane partials, then a butterfly), so nothing here depends on the lane mapping.
//
// Layout: one wave64 per sample and per workgroup (each wave stops on its own; its loop condition is wave-uniform).  Per sample
// in LDS, for the whole run: f64 bel [N], u [N], the links' messages to x_{i+1} and to x_i [N-1] each, the windows' messages
// [(N-h+1)][h] and the deltas into the windows [(N-h+1)][h]; f32 pair [4(N-1)]; int caps [N-h+1].  Global memory is read once for
// the potentials and written once for the results.  Lane mapping: step 1 and 2, variable i = lane, lane + 64, ... (the variable
// also writes its deltas into its windows' rows); step 3, link i = lane, lane + 64, ...; step 4, window edge e = w h + j = lane,
// lane + 64, ...: the lanes of one window read the same row of deltas (same addresses broadcast).  The link deltas are formed by
// the link's lane from bel and its own two messages.  Two barriers per iteration.
#include "fgnn_common.h"
#include "fgnn_hip_pgm_bp.h"
#include <stdint.h>

#define BP_MAX_H 13
#define BP_LDS_MAX (160 * 1024)
#define BP_FORCE 1048576.0          // 2^20: the message of a window that allows no ones

extern __shared__ __attribute__((aligned(16))) unsigned char bp_lds[];

struct BpParams {
    const float* unary; int64_t u_sb;
    const float* pair; int64_t p_sb;
    const int32_t* caps; int64_t c_sb;
    int64_t* labels;
    double* beliefs;
    int32_t *status, *iters;
    double tol, damping;
    int N, h, max_iter;
};

// per-sample LDS (see Layout); -1 outside the family
static int64_t bp_sample_bytes(int N, int h) {
    if (h < 2 || h > BP_MAX_H || N < h) return -1;
    const int64_t n = N, W = n - h + 1;
    const int64_t bytes = 8 * (2 * n + 2 * (n - 1) + 2 * W * h) + 4 * (4 * (n - 1)) + 4 * W;
    const int64_t r = (bytes + 15) / 16 * 16;
    return r <= BP_LDS_MAX ? r : -1;
}

__global__ __launch_bounds__(64) void chain_budget_bp_kernel(const BpParams p) {
    const int lane = threadIdx.x;
    const int N = p.N, h = p.h, W = N - h + 1, L = N - 1, E = W * h;
    const int64_t b = blockIdx.x;
    double* bel = (double*)bp_lds;      // [N]
    double* un = bel + N;               // [N]
    double* mR = un + N;                // [L] link i -> x_{i+1}
    double* mL = mR + L;                // [L] link i -> x_i
    double* mW = mL + L;                // [W][h] window w -> x_{w+j}
    double* dW = mW + E;                // [W][h] x_{w+j} -> window w
    float* pr = (float*)(dW + E);       // [L][4]
    int* cp = (int*)(pr + 4 * L);       // [W]

    {
        const float* u = p.unary + b * p.u_sb;
        const float* q = p.pair + b * p.p_sb;
        const int32_t* c = p.caps + b * p.c_sb;
        for (int i = lane; i < N; i += 64) un[i] = (double)u[2 * i + 1] - (double)u[2 * i];
        for (int k = lane; k < 4 * L; k += 64) pr[k] = q[k];
        for (int k = lane; k < W; k += 64) cp[k] = c[k];
        for (int k = lane; k < L; k += 64) { mR[k] = 0.0; mL[k] = 0.0; }
        for (int k = lane; k < E; k += 64) mW[k] = 0.0;
    }
    __syncthreads();
    bool neg = false;
    for (int k = lane; k < W; k += 64) neg |= cp[k] < 0;
    const bool infeasible = __ballot(neg) != 0ull;

    const double damping = p.damping, omd = 1.0 - damping;
    int it = 0;
    bool conv = false;
    while (!infeasible && it < p.max_iter) {
        // ---- 1, 2. beliefs, and the deltas into the windows ----
        for (int i = lane; i < N; i += 64) {
            double s = un[i];
            if (i > 0) s = s + mR[i - 1];
            if (i < L) s = s + mL[i];
            const int w0 = i - h + 1 > 0 ? i - h + 1 : 0, w1 = i < W - 1 ? i : W - 1;
            for (int w = w0; w <= w1; ++w) s = s + mW[w * h + (i - w)];
            bel[i] = s;
            for (int w = w0; w <= w1; ++w) dW[w * h + (i - w)] = s - mW[w * h + (i - w)];
        }
        __syncthreads();
        double change = 0.0;
        // ---- 3. links ----
        for (int i = lane; i < L; i += 64) {
            const float* pt = pr + 4 * i;
            const double t0 = pt[0], t1 = pt[1], t2 = pt[2], t3 = pt[3];
            const double oR = mR[i], oL = mL[i];
            const double dl = bel[i] - oL, dr = bel[i + 1] - oR;
            const double fR = fmax(t1, t3 + dl) - fmax(t0, t2 + dl);
            const double fL = fmax(t2, t3 + dr) - fmax(t0, t1 + dr);
            const double nR = damping * oR + omd * fR, nL = damping * oL + omd * fL;
            mR[i] = nR;
            mL[i] = nL;
            change = fmax(change, fmax(fabs(nR - oR), fabs(nL - oL)));
        }
        // ---- 4. windows: one edge per lane ----
        for (int e = lane; e < E; e += 64) {
            const int w = e / h, j = e - w * h, c = cp[w];
            double f = 0.0;
            if (c == 0) {
                f = -BP_FORCE;
            } else if (c <= h - 1) {
                const double* d = dW + w * h;
                double kth = 0.0;
                for (int k = 0; k < h; ++k) {
                    if (k == j) continue;
                    const double v = d[k];
                    int gt = 0, ge = 0;                 // among the others: strictly above v; at or above v (v itself included)
                    for (int m = 0; m < h; ++m) {
                        if (m == j) continue;
                        const double x = d[m];
                        gt += x > v;
                        ge += x >= v;
                    }
                    if (gt < c && ge >= c) kth = v;     // every k that passes holds the same value
                }
                f = -fmax(0.0, kth);
            }
            const double o = mW[e], nw = damping * o + omd * f;
            mW[e] = nw;
            change = fmax(change, fabs(nw - o));
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) change = fmax(change, __shfl_xor(change, m));
        change = __shfl(change, 0);
        ++it;
        __syncthreads();
        if (change < p.tol) { conv = true; break; }
    }

    // ---- the final beliefs and the decision ----
    for (int i = lane; i < N; i += 64) {
        double s = 0.0;
        if (!infeasible) {
            s = un[i];
            if (i > 0) s = s + mR[i - 1];
            if (i < L) s = s + mL[i];
            const int w0 = i - h + 1 > 0 ? i - h + 1 : 0, w1 = i < W - 1 ? i : W - 1;
            for (int w = w0; w <= w1; ++w) s = s + mW[w * h + (i - w)];
        }
        p.labels[b * N + i] = s > 0.0 ? 1 : 0;
        if (p.beliefs) p.beliefs[b * N + i] = s;
    }
    if (lane == 0) {
        if (p.status) p.status[b] = infeasible ? 2 : conv ? 0 : 3;
        if (p.iters) p.iters[b] = it;
    }
}

extern "C" int64_t fgnn_chain_budget_bp_lds_bytes(int N, int h) {
    const int64_t r = bp_sample_bytes(N, h);
    if (r < 0) {
        if (h < 2 || h > BP_MAX_H) fgnn_set_error("chain_budget_bp: window h=%d outside 2..%d", h, BP_MAX_H);
        else if (N < h) fgnn_set_error("chain_budget_bp: chain length N=%d shorter than the window h=%d", N, h);
        else fgnn_set_error("chain_budget_bp: N=%d h=%d needs more than %d bytes of LDS per sample", N, h, BP_LDS_MAX);
    }
    return r;
}

extern "C" int fgnn_chain_budget_bp(const float* unary, int64_t unary_sb, const float* pair, int64_t pair_sb, const int32_t* caps,
                                    int64_t caps_sb, int64_t B, int N, int h, int max_iter, double tol, double damping,
                                    int64_t* labels, double* beliefs, int32_t* status, int32_t* iters, fgnn_stream_t stream) {
    const int64_t per = fgnn_chain_budget_bp_lds_bytes(N, h);
    if (per < 0) return FGNN_EUNSUPPORTED;
    if (B < 0 || B > 0x7fffffffll) FGNN_FAIL(FGNN_EINVAL, "chain_budget_bp: batch %lld outside 0 .. 2^31-1", (long long)B);
    if (max_iter < 0) FGNN_FAIL(FGNN_EINVAL, "chain_budget_bp: max_iter=%d is negative", max_iter);
    if (!(tol >= 0.0 && tol <= 1e150)) FGNN_FAIL(FGNN_EINVAL, "chain_budget_bp: tol=%g is not a finite value >= 0", tol);
    if (!(damping >= 0.0 && damping < 1.0)) FGNN_FAIL(FGNN_EINVAL, "chain_budget_bp: damping=%g is not in [0, 1)", damping);
    if (unary_sb < 0 || pair_sb < 0 || caps_sb < 0) FGNN_FAIL(FGNN_EINVAL, "chain_budget_bp: negative batch stride");
    if (B == 0) return FGNN_OK;
    if (!unary || !pair || !caps) FGNN_FAIL(FGNN_EINVAL, "chain_budget_bp: null input pointer");
    if (!labels) FGNN_FAIL(FGNN_EINVAL, "chain_budget_bp: null labels");
    BpParams p = {};
    p.unary = unary; p.u_sb = unary_sb;
    p.pair = pair; p.p_sb = pair_sb;
    p.caps = caps; p.c_sb = caps_sb;
    p.labels = labels; p.beliefs = beliefs; p.status = status; p.iters = iters;
    p.tol = tol; p.damping = damping;
    p.N = N; p.h = h; p.max_iter = max_iter;
    const int lds = (int)per;
    fgnn_note_kernel("chain_budget_bp_kernel");
    return fgnn_launch("chain_budget_bp", chain_budget_bp_kernel, dim3((unsigned)B), dim3(64), lds, fgnn_stream(stream), p);
}
