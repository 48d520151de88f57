// pgm_lp.hip — the LP relaxation of the synthetic-PGM chains: what `PFactorGraph.solve(branch_and_bound=False)` (AD3) labels the
// reference's random models with (`assign1`, the reference's lib/data/random_pgm_hop.py:119-125 and the other random_pgm*.py).
//
//   fgnn_chain_budget_lp    the LP's ADMM iterate per sample: labels, marginals, objective, status, iterations
//
// The model is fgnn_chain_budget_map's (pgm_datapath.hip): unary [B][N][2], link table pair [B][N-1][4] (row-major [x_i][x_{i+1}]),
// caps [B][N-h+1] int32 (cap >= h: the window has no factor); a batch stride of 0 shares an input across the batch.
//
// The LP, in binary form.  z_i = mu_i(1) in [0,1]; y_i = mu_{i,i+1}(1,1) with max(0, z_i + z_{i+1} - 1) <= y_i <= min(z_i, z_{i+1})
// (the 2x2 marginal simplex of AD3's dense pair factor); sum_{j=w}^{w+h-1} z_j <= cap[w] for every window with a factor (AD3's
// budget factor over the state-1 binaries; that polytope is integral).  Maximise the expected log-potential sum
//   sum_i (u_i(0) + (u_i(1) - u_i(0)) z_i) + sum_i (p00 + (p10 - p00) z_i + (p01 - p00) z_{i+1} + (p00 - p01 - p10 + p11) y_i).
//
// The solver: AD3-style ADMM (alternating directions dual decomposition, Martins et al., JMLR 2015).  Factors: one link factor per
// link and one budget factor per constrained window; variable i has deg_i of them and each takes the share (u_i(1) - u_i(0)) / deg_i
// of its unary.  Every variable-factor slot carries a copy q and a multiplier lambda.  Start: z = 1/2, lambda = 0, eta = `eta`.
// One iteration:
//   1. each factor solves its QP  argmin 1/2 |q - c|^2 - (pair term) over its polytope, c = z + ((share + own linear term) + lambda)
//      / eta per slot:
//      link (k = c12 / eta): k >= 0: c1 >= c2 + k -> (clip c1, clip(c2 + k)); c2 >= c1 + k -> (clip(c1 + k), clip c2); otherwise
//        both clip(((c1 + c2) + k) / 2); y = min(z1, z2).  k < 0: the same on (c1 + k, 1 - c2, -k), then z2 -> 1 - z2, y -> z1 - y.
//      budget (b = cap): clip c to [0,1]; if the clipped sum (over j in order) exceeds b, tau solves sum clip(c - tau, 0, 1) = b:
//        t_lo = the largest of 0 and the breakpoints c_j, c_j - 1 where that sum is still > b; on (t_lo, next breakpoint) the sum is
//        linear with ones = {c_j - 1 > t_lo}, free = {c_j - 1 <= t_lo < c_j}: tau = ((|ones| + sum_free c_j) - b) / |free|
//        (t_lo when free is empty); q = clip(c - tau).  Serial in the lane, O(h^2), h <= 13, the c's staged in the slot's LDS.
//   2. consensus z'_i = (left link + right link + the budget windows in increasing w) / deg_i;
//   3. dual update lambda -= eta (q - z');
//   4. residuals over the S = 2(N-1) + h nb slots: P = sum (q - z')^2, D = sum_i deg_i (z'_i - z_i)^2.  Stop when P / S < tol^2 and
//      D / S < tol^2 (both RMS residuals below `tol`).  Else, with `adapt`, after every 50th iteration: eta *= 2 when P > 100 D,
//      eta /= 2 when D > 100 P (residual balancing at an RMS ratio of 10).  At most `max_iter` iterations.
// The values follow AD3's Python `solve()` defaults as the reference calls it (eta 0.1, adapt on, 1000 iterations, tol 1e-6).  The
// balancing runs every 50th iteration and not every one: on the reference's models, balancing at every iteration (with or without
// eta in the dual residual) converged on fewer samples within 1000 iterations than a fixed eta and left gaps to the LP optimum up to
// 0.7; every 50th it is within a few samples of the fixed step (tests/pgm_lp_oracle.py restates all of this).
//
// Outputs: labels z_i > 0.5 (ties to 0, np.argmax of [1 - z, z]); marginals z; value = the objective at z with each y_i the link
// factor's last copy clipped into its bounds at z; status 0 integral (every z_i within 1e-6 of 0 or 1), 1 fractional, 2 infeasible
// (a cap < 0: labels 0, marginals 0, value -inf, no iteration), 3 the iteration cap reached; iters = iterations run.
//
// Arithmetic: f64 throughout, this file built with -ffp-contract=off; each expression above in the order written.  The residual
// sums are lane partials then a butterfly, so only they may round differently from the restatement.
//
// Layout: one wave64 per sample and per workgroup (each wave stops on its own; its loop condition is wave-uniform).  Lanes take the
// factors (budgets first, then links) and the variables in strided passes.  Everything lives in LDS: no scratch.
#include "fgnn_common.h"
#include <stdint.h>

#define LP_MAX_H 13
#define LP_LDS_MAX (160 * 1024)
#define LP_ADAPT_EVERY 50
#define LP_INTEGRAL_EPS 1e-6

extern __shared__ __attribute__((aligned(16))) unsigned char lp_lds[];

struct LpParams {
    const float* unary; int64_t u_sb;
    const float* pair; int64_t p_sb;
    const int32_t* caps; int64_t c_sb;
    int64_t* labels;
    double *marginals, *value;
    int32_t *status, *iters;
    double tol2, eta;
    int N, h, max_iter, adapt;
};

// per-sample LDS: f64 z, z', share, deg [N], lambda and q of the link slots [2(N-1)], y [N-1], lambda and q of the budget slots
// [(N-h+1) h]; f32 unary [2N], pair [4(N-1)]; int caps and the list of windows with a factor [N-h+1].  -1 outside the family.
static int64_t lp_sample_bytes(int N, int h) {
    if (h < 2 || h > LP_MAX_H || N < h) return -1;
    const int64_t n = N, W = n - h + 1;
    const int64_t bytes = 8 * (4 * n + 5 * (n - 1) + 2 * W * h) + 4 * (2 * n + 4 * (n - 1)) + 4 * (2 * W + 1);
    const int64_t r = (bytes + 15) / 16 * 16;
    return r <= LP_LDS_MAX ? r : -1;
}

__device__ __forceinline__ double lp_clip(double v) { return fmin(fmax(v, 0.0), 1.0); }

__global__ __launch_bounds__(64) void chain_budget_lp_kernel(const LpParams p) {
    const int lane = threadIdx.x;
    const int N = p.N, h = p.h, W = N - h + 1, L = N - 1;
    const int64_t b = blockIdx.x;
    double* z = (double*)lp_lds;
    double* zn = z + N;
    double* share = zn + N;
    double* dg = share + N;
    double* lamL = dg + N;                 // [L][2]
    double* qL = lamL + 2 * L;             // [L][2]
    double* yL = qL + 2 * L;               // [L]
    double* lamB = yL + L;                 // [W][h]
    double* qB = lamB + (int64_t)W * h;    // [W][h]
    float* un = (float*)(qB + (int64_t)W * h);
    float* pr = un + 2 * N;
    int* cp = (int*)(pr + 4 * L);
    int* bw = cp + W;                      // windows with a factor, then their count at bw[W]

    {
        const float* u = p.unary + b * p.u_sb;
        const float* q = p.pair + b * p.p_sb;
        const int32_t* c = p.caps + b * p.c_sb;
        for (int k = lane; k < 2 * N; k += 64) un[k] = u[k];
        for (int k = lane; k < 4 * L; k += 64) pr[k] = q[k];
        for (int k = lane; k < W; k += 64) cp[k] = c[k];
    }
    __syncthreads();
    bool neg = false;
    for (int k = lane; k < W; k += 64) neg |= cp[k] < 0;
    const bool infeasible = __ballot(neg) != 0ull;
    if (lane == 0) {
        int nb = 0;
        for (int w = 0; w < W; ++w)
            if (cp[w] < h) bw[nb++] = w;
        bw[W] = nb;
    }
    for (int i = lane; i < N; i += 64) {
        int d = (i > 0) + (i < L);
        const int w0 = i - h + 1 > 0 ? i - h + 1 : 0, w1 = i < W - 1 ? i : W - 1;
        for (int w = w0; w <= w1; ++w) d += cp[w] < h;
        dg[i] = (double)d;
        share[i] = ((double)un[2 * i + 1] - (double)un[2 * i]) / (double)d;
        z[i] = 0.5;
    }
    for (int k = lane; k < 2 * L; k += 64) lamL[k] = 0.0;
    for (int k = lane; k < W * h; k += 64) lamB[k] = 0.0;
    __syncthreads();
    const int nb = bw[W], nf = nb + L;
    const double S = 2.0 * L + (double)h * nb;

    double eta = p.eta;
    int it = 0;
    bool conv = false;
    while (!infeasible && it < p.max_iter) {
        // ---- 1. the factors' QPs ----
        for (int f = lane; f < nf; f += 64) {
            if (f < nb) {
                const int w = bw[f];
                double* c = qB + w * h;
                const double* lam = lamB + w * h;
                const double bcap = (double)cp[w];
                double s = 0.0;
                for (int j = 0; j < h; ++j) {
                    c[j] = z[w + j] + (share[w + j] + lam[j]) / eta;
                    s = s + lp_clip(c[j]);
                }
                if (s > bcap) {
                    double tlo = 0.0;
                    for (int m = 0; m < 2 * h; ++m) {
                        const double t = m < h ? c[m] : c[m - h] - 1.0;
                        double g = 0.0;
                        for (int j = 0; j < h; ++j) g = g + lp_clip(c[j] - t);
                        if (g > bcap && t > tlo) tlo = t;
                    }
                    double acc = 0.0;
                    int nfree = 0;
                    for (int j = 0; j < h; ++j) {
                        if (c[j] - 1.0 > tlo) acc = acc + 1.0;
                        else if (c[j] > tlo) { acc = acc + c[j]; ++nfree; }
                    }
                    const double tau = nfree > 0 ? (acc - bcap) / (double)nfree : tlo;
                    for (int j = 0; j < h; ++j) c[j] = lp_clip(c[j] - tau);
                } else {
                    for (int j = 0; j < h; ++j) c[j] = lp_clip(c[j]);
                }
            } else {
                const int i = f - nb;
                const float* pt = pr + 4 * i;
                const double p0 = pt[0], p1 = pt[1], p2 = pt[2], p3 = pt[3];
                const double a1 = p2 - p0, a2 = p1 - p0, c12 = ((p0 - p1) - p2) + p3;
                const double c1 = z[i] + ((share[i] + a1) + lamL[2 * i]) / eta;
                const double c2 = z[i + 1] + ((share[i + 1] + a2) + lamL[2 * i + 1]) / eta;
                const double k = c12 / eta;
                const bool ng = k < 0;
                const double a = ng ? c1 + k : c1, bb = ng ? 1.0 - c2 : c2, kk = ng ? -k : k;
                const double mid = lp_clip(((a + bb) + kk) * 0.5);
                double z1, z2;
                if (a >= bb + kk) { z1 = lp_clip(a); z2 = lp_clip(bb + kk); }
                else if (bb >= a + kk) { z1 = lp_clip(a + kk); z2 = lp_clip(bb); }
                else { z1 = mid; z2 = mid; }
                const double y = fmin(z1, z2);
                qL[2 * i] = z1;
                qL[2 * i + 1] = ng ? 1.0 - z2 : z2;
                yL[i] = ng ? z1 - y : y;
            }
        }
        __syncthreads();
        // ---- 2. consensus ----
        double D = 0.0;
        for (int i = lane; i < N; i += 64) {
            double s = 0.0;
            if (i > 0) s = s + qL[2 * (i - 1) + 1];
            if (i < L) s = s + qL[2 * i];
            const int w0 = i - h + 1 > 0 ? i - h + 1 : 0, w1 = i < W - 1 ? i : W - 1;
            for (int w = w0; w <= w1; ++w)
                if (cp[w] < h) s = s + qB[w * h + (i - w)];
            const double v = s / dg[i], d = v - z[i];
            zn[i] = v;
            D = D + dg[i] * d * d;
        }
        __syncthreads();
        // ---- 3. dual update ----
        double P = 0.0;
        for (int f = lane; f < nf; f += 64) {
            if (f < nb) {
                const int w = bw[f];
                for (int j = 0; j < h; ++j) {
                    const double d = qB[w * h + j] - zn[w + j];
                    lamB[w * h + j] = lamB[w * h + j] - eta * d;
                    P = P + d * d;
                }
            } else {
                const int i = f - nb;
                const double d1 = qL[2 * i] - zn[i], d2 = qL[2 * i + 1] - zn[i + 1];
                lamL[2 * i] = lamL[2 * i] - eta * d1;
                lamL[2 * i + 1] = lamL[2 * i + 1] - eta * d2;
                P = P + d1 * d1;
                P = P + d2 * d2;
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            P = P + __shfl_xor(P, m);
            D = D + __shfl_xor(D, m);
        }
        P = __shfl(P, 0);
        D = __shfl(D, 0);
        double* t = z; z = zn; zn = t;
        ++it;
        __syncthreads();
        if (P / S < p.tol2 && D / S < p.tol2) { conv = true; break; }
        if (p.adapt && it % LP_ADAPT_EVERY == 0) {
            if (P > 100.0 * D) eta = eta * 2.0;
            else if (D > 100.0 * P) eta = eta * 0.5;
        }
    }

    // ---- outputs ----
    bool frac = false;
    for (int i = lane; i < N; i += 64) {
        const double v = infeasible ? 0.0 : z[i];
        frac |= fmin(v, 1.0 - v) > LP_INTEGRAL_EPS;
        p.labels[b * N + i] = v > 0.5 ? 1 : 0;
        if (p.marginals) p.marginals[b * N + i] = v;
    }
    const bool fractional = __ballot(frac) != 0ull;
    if (lane == 0) {
        double v = 0.0;
        for (int i = 0; i < N; ++i) {
            const double u0 = un[2 * i], u1 = un[2 * i + 1];
            v = v + (u0 + (u1 - u0) * z[i]);
        }
        for (int i = 0; i < L; ++i) {
            const float* pt = pr + 4 * i;
            const double p0 = pt[0], p1 = pt[1], p2 = pt[2], p3 = pt[3];
            const double a1 = p2 - p0, a2 = p1 - p0, c12 = ((p0 - p1) - p2) + p3;
            const double zl = z[i], zr = z[i + 1];
            const double y = fmin(fmax(yL[i], fmax(0.0, (zl + zr) - 1.0)), fmin(zl, zr));
            v = v + (((p0 + a1 * zl) + a2 * zr) + c12 * y);
        }
        if (p.value) p.value[b] = infeasible ? -__builtin_inf() : v;
        if (p.status) p.status[b] = infeasible ? 2 : !conv ? 3 : fractional ? 1 : 0;
        if (p.iters) p.iters[b] = it;
    }
}

extern "C" int64_t fgnn_chain_budget_lp_lds_bytes(int N, int h) {
    const int64_t r = lp_sample_bytes(N, h);
    if (r < 0) {
        if (h < 2 || h > LP_MAX_H) fgnn_set_error("chain_budget_lp: window h=%d outside 2..%d", h, LP_MAX_H);
        else if (N < h) fgnn_set_error("chain_budget_lp: chain length N=%d shorter than the window h=%d", N, h);
        else fgnn_set_error("chain_budget_lp: N=%d h=%d needs more than %d bytes of LDS per sample", N, h, LP_LDS_MAX);
    }
    return r;
}

extern "C" int fgnn_chain_budget_lp(const float* unary, int64_t unary_sb, const float* pair, int64_t pair_sb, const int32_t* caps,
                                    int64_t caps_sb, int64_t B, int N, int h, int max_iter, double tol, double eta, int adapt,
                                    int64_t* labels, double* marginals, double* value, int32_t* status, int32_t* iters,
                                    fgnn_stream_t stream) {
    const int64_t per = fgnn_chain_budget_lp_lds_bytes(N, h);
    if (per < 0) return FGNN_EUNSUPPORTED;
    if (B < 0 || B > 0x7fffffffll) FGNN_FAIL(FGNN_EINVAL, "chain_budget_lp: batch %lld outside 0 .. 2^31-1", (long long)B);
    if (max_iter < 0) FGNN_FAIL(FGNN_EINVAL, "chain_budget_lp: max_iter=%d is negative", max_iter);
    if (!(tol >= 0.0 && tol <= 1e150)) FGNN_FAIL(FGNN_EINVAL, "chain_budget_lp: tol=%g is not a finite value >= 0", tol);
    if (!(eta > 0.0 && eta <= 1e150)) FGNN_FAIL(FGNN_EINVAL, "chain_budget_lp: eta=%g is not a finite value > 0", eta);
    if (unary_sb < 0 || pair_sb < 0 || caps_sb < 0) FGNN_FAIL(FGNN_EINVAL, "chain_budget_lp: negative batch stride");
    if (B == 0) return FGNN_OK;
    if (!unary || !pair || !caps) FGNN_FAIL(FGNN_EINVAL, "chain_budget_lp: null input pointer");
    if (!labels) FGNN_FAIL(FGNN_EINVAL, "chain_budget_lp: null labels");
    LpParams p = {};
    p.unary = unary; p.u_sb = unary_sb;
    p.pair = pair; p.p_sb = pair_sb;
    p.caps = caps; p.c_sb = caps_sb;
    p.labels = labels; p.marginals = marginals; p.value = value; p.status = status; p.iters = iters;
    p.tol2 = tol * tol; p.eta = eta;
    p.N = N; p.h = h; p.max_iter = max_iter; p.adapt = adapt ? 1 : 0;
    const int lds = (int)per;
    fgnn_note_kernel("chain_budget_lp_kernel");
    return fgnn_launch("chain_budget_lp", chain_budget_lp_kernel, dim3((unsigned)B), dim3(64), lds, fgnn_stream(stream), p);
}
