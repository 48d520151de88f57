// ldpc_lp.hip — the ADMM linear-programming LDPC decoder for a batch of received words: Feldman's LP relaxation solved by ADMM
// (Barman, Liu, Draper & Recht 2013) with over-relaxation and the penalty term of Liu & Draper's penalised decoder; the projection
// onto the parity polytope is a sort-free cut search (Zhang & Siegel 2013).  The reference has no counterpart; the steps are
// derived here and restated in tests/ldpc_lp_oracle.py.
//
//   fgnn_ldpc_decode_lp              one launch decodes the batch: hard decisions, the final x, violated checks, iterations, flags
//   fgnn_ldpc_decode_lp_lds_bytes    the LDS one word occupies, or < 0 where the shape is not taken
//
// The tables, the per-word LDS layout, the thread rule and the steps shared with the other word kernels (staging, load, the
// violated-check count) are ldpc_word.h's: R holds z, T holds x, prior holds g; u [E] is appended behind col_ptr.
//
// Steps, all f32, each expression in the order written (this file is built with -ffp-contract=off):
//   load       g[n] = llr[n]; NaN -> 0; clamped to +-4096.  z[e] = 0.5, u[e] = 0.
//   constants  amu = penalty / mu, omr = 1 - relax.
//   variable n of degree d >= 1:  t = 0; t = t + (z[e] - u[e]) for e = col_ptr[n] ..;  x[n] = clip(((t - g[n] / mu) - amu) / (d - 2 amu), 0, 1).
//              degree 0:  x[n] = (g[n] < 0).
//   check m    over its edges l = 0 .. L-1 in row order:  w_l = (relax x[var_l] + omr z_l) + u_l;  z' = project(w);  u_l = w_l - z'_l;
//              res = max |x[var_l] - z'_l|, dz = max |z'_l - z_l| over all edges; then z = z'.
//   decision   xh[n] = x[n] > 0.5, viol = the checks of odd parity in xh.
//   stop       conv = res <= eps and dz <= eps (never with eps < 0); a word stops when conv, or stop_on_codeword and viol = 0, or at max_iter.
//   flags      bit 0 = conv (at the word's last iteration); bit 1 = bit 0 and min(x[n], 1 - x[n]) <= 1e-3 for every n.
//   project    c = clip(w, 0, 1); f_l = w_l > 0.5; if |f| is even, f is flipped at the first l with the smallest |w_l - 0.5|;
//              theta_l = +1 where f_l, else -1; p = |f| - 1;  phi(beta) = 0 + theta_0 clip(w_0 - beta theta_0, 0, 1) + theta_1 ...
//              if phi(0) <= p: c.  Otherwise over the breakpoints b in the order (l = 0: first, second; l = 1: ...), first = w_l - 1
//              and second = w_l where f_l, first = -w_l and second = 1 - w_l elsewhere, and only those with b > 0:  v = phi(b); if v > p
//              and b > lo: (lo, vlo) = (b, v); if v <= p and b < hi: (hi, vhi) = (b, v); from (lo, vlo) = (0, phi(0)), hi = +inf.
//              beta = hi if vlo = vhi, else lo + ((vlo - p) (hi - lo)) / (vlo - vhi);  the result is clip(w - beta theta, 0, 1).
//              (phi(+inf) = |f| - L <= p, so hi is always found; with no cut beta = 0 gives c by the same expression.)
//
// Layout: one workgroup per word, one launch per batch; the state stays in LDS for the whole run, global memory is read once
// (tables, llr) and written once.  A lane owns a variable in the variable pass and a whole check in the check pass; the check's
// w, x[var], old z and row-table words (at most 16 each) stay in registers (fully unrolled, predicated on L), so the row table is
// read once per edge and pass.  res and dz reduce per wave by lane exchange, then over the waves through the scratch words.  The
// violated checks are counted only when the answer is used: every iteration with stop_on_codeword, else at the last one.
#include "fgnn_hip_ldpc_lp.h"
#include "ldpc_word.h"

#define LP_LDS_MAX (160 * 1024)
#define LP_SCRATCH 16               // words: [0..3] violated checks, [4..7] res, [8..11] dz, [12..15] fractional variables, per wave
#define LP_INTEGRAL 1.0e-3f

struct LpParams {
    const float* llr; int64_t llr_sb;
    const int32_t *col_ptr, *row_ptr, *row_edge, *row_var;
    uint8_t* x;
    float* soft;
    int32_t *viol, *iters, *flags;
    int N, M, E, max_iter, stop_on_codeword;
    float mu, penalty, relax, eps;
};

struct LpLds : LdpcWord { float* u; };          // u [E], behind cp (padded to a whole word)

__device__ __forceinline__ LpLds lp_carve(int N, int M, int E) {
    LpLds s;
    (LdpcWord&)s = ldpc_word_carve(N, M, E, LP_SCRATCH);
    s.u = (float*)(s.rp + (((M + 1) + (N + 1) + 1) & ~1));
    return s;
}

__device__ __forceinline__ float lp_clip(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// phi(beta) of a check with L edges: bit l of fm = f_l
__device__ __forceinline__ float lp_phi(const float (&w)[LDPC_MAXD], uint32_t fm, int L, float beta) {
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < LDPC_MAXD; ++k)
        if (k < L) {
            const float th = (fm >> k & 1u) ? 1.0f : -1.0f;
            s = s + th * lp_clip(w[k] - beta * th);
        }
    return s;
}

__device__ __forceinline__ float lp_wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

// one check's update (see Steps); res and dz take the check's share of the two maxima
__device__ __forceinline__ void lp_check(const LpLds& s, int m, float rho, float omr, float& res, float& dz) {
    const int r0 = s.rp[m], L = s.rp[m + 1] - r0;
    float w[LDPC_MAXD], xv[LDPC_MAXD], zo[LDPC_MAXD];
    uint32_t ev[LDPC_MAXD];
    uint32_t fm = 0;
    int nf = 0, first = 0;
    float nearest = INFINITY;
#pragma unroll
    for (int l = 0; l < LDPC_MAXD; ++l)
        if (l < L) {
            ev[l] = s.rtab[r0 + l];
            const int e = ev[l] & 0xffffu;
            xv[l] = s.T[ev[l] >> 16];
            zo[l] = s.R[e];
            w[l] = (rho * xv[l] + omr * zo[l]) + s.u[e];
            const bool f = w[l] > 0.5f;
            fm |= (uint32_t)f << l;
            nf += f;
            const float d = fabsf(w[l] - 0.5f);
            if (d < nearest) { nearest = d; first = l; }
        }
    if (!(nf & 1)) {
        fm ^= 1u << first;
        nf += (fm >> first & 1u) ? 1 : -1;
    }
    const float p = (float)(nf - 1);
    const float v0 = lp_phi(w, fm, L, 0.0f);
    float beta = 0.0f;
    if (v0 > p) {
        float lo = 0.0f, vlo = v0, hi = INFINITY, vhi = 0.0f;
#pragma unroll
        for (int l = 0; l < LDPC_MAXD; ++l)
            if (l < L) {
                const bool f = fm >> l & 1u;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const float b = h == 0 ? (f ? w[l] - 1.0f : -w[l]) : (f ? w[l] : 1.0f - w[l]);
                    if (b > 0.0f) {
                        const float v = lp_phi(w, fm, L, b);
                        if (v > p) {
                            if (b > lo) { lo = b; vlo = v; }
                        } else if (b < hi) { hi = b; vhi = v; }
                    }
                }
            }
        beta = vlo == vhi ? hi : lo + ((vlo - p) * (hi - lo)) / (vlo - vhi);
    }
#pragma unroll
    for (int l = 0; l < LDPC_MAXD; ++l)
        if (l < L) {
            const int e = ev[l] & 0xffffu;
            const float th = (fm >> l & 1u) ? 1.0f : -1.0f;
            const float zn = lp_clip(w[l] - beta * th);
            s.u[e] = w[l] - zn;
            s.R[e] = zn;
            res = fmaxf(res, fabsf(xv[l] - zn));
            dz = fmaxf(dz, fabsf(zn - zo[l]));
        }
}

__global__ __launch_bounds__(256) void ldpc_lp_kernel(const LpParams p) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const int N = p.N, M = p.M, E = p.E;
    const int64_t b = blockIdx.x;
    const LpLds s = lp_carve(N, M, E);
    float* const fsum = (float*)s.wsum;

    ldpc_stage_tables(s, p, false);
    for (int e = tid; e < E; e += nt) { s.R[e] = 0.5f; s.u[e] = 0.0f; }
    ldpc_load_word(s, p.llr + b * p.llr_sb, N);
    __syncthreads();

    const float mu = p.mu, rho = p.relax, eps = p.eps;
    const float amu = p.penalty / mu, omr = 1.0f - rho;
    const auto bit = [](float x) { return x > 0.5f; };
    int it = 0, viol = 0;
    bool conv = false;
    for (;;) {
        ++it;
        for (int n = tid; n < N; n += nt) {
            const int e0 = s.cp[n], e1 = s.cp[n + 1];
            float t = 0.0f;
            for (int e = e0; e < e1; ++e) t = t + (s.R[e] - s.u[e]);
            const float g = s.prior[n];
            const float x = lp_clip(((t - g / mu) - amu) / ((float)(e1 - e0) - 2.0f * amu));
            s.T[n] = e1 > e0 ? x : (g < 0.0f ? 1.0f : 0.0f);
        }
        __syncthreads();
        float res = 0.0f, dz = 0.0f;
        for (int m = tid; m < M; m += nt) lp_check(s, m, rho, omr, res, dz);
        res = lp_wave_max(res);
        dz = lp_wave_max(dz);
        if (lane == 0) { fsum[4 + wave] = res; fsum[8 + wave] = dz; }
        __syncthreads();            // (the next write of these words comes after the next variable pass's barrier)
        res = dz = 0.0f;
        for (int w = 0; w < nw; ++w) { res = fmaxf(res, fsum[4 + w]); dz = fmaxf(dz, fsum[8 + w]); }
        conv = res <= eps && dz <= eps;
        const bool last = conv || it >= p.max_iter;
        if (p.stop_on_codeword || last) viol = ldpc_count_violated_by(s, M, bit);
        if (last || (p.stop_on_codeword && viol == 0)) break;
    }

    int flags = conv ? 1 : 0;
    if (conv) {         // (uniform over the workgroup) the certificate: no variable further than 1e-3 from 0 and 1
        bool frac = false;
        for (int n = tid; n < N; n += nt) {
            const float x = s.T[n];
            frac |= !(fminf(x, 1.0f - x) <= LP_INTEGRAL);
        }
        const bool any = __ballot(frac) != 0;
        if (lane == 0) s.wsum[12 + wave] = any;
        __syncthreads();
        int n_frac = 0;
        for (int w = 0; w < nw; ++w) n_frac += s.wsum[12 + w];
        if (n_frac == 0) flags |= 2;
    }
    for (int n = tid; n < N; n += nt) {
        const float x = s.T[n];
        p.x[b * N + n] = x > 0.5f ? 1 : 0;
        if (p.soft) p.soft[b * N + n] = x;
    }
    if (tid == 0) { p.viol[b] = viol; p.iters[b] = it; p.flags[b] = flags; }
}

extern "C" int64_t fgnn_ldpc_decode_lp_lds_bytes(int N, int M, int E) {
    if (ldpc_word_check_sizes("ldpc_decode_lp", N, M, E) != FGNN_OK) return -1;
    const int64_t bytes = ldpc_word_bytes_lp(N, M, E);
    if (bytes > LP_LDS_MAX) {
        fgnn_set_error("ldpc_decode_lp: a word of N=%d, M=%d, E=%d needs %lld B of LDS (z, u and the row table are three E-word arrays), "
                       "above %d", N, M, E, (long long)bytes, LP_LDS_MAX);
        return -1;
    }
    return bytes;
}

extern "C" int fgnn_ldpc_decode_lp(const float* llr, int64_t llr_sb, const int32_t* col_ptr, const int32_t* row_ptr,
                                   const int32_t* row_edge, const int32_t* row_var, int64_t B, int N, int M, int E, int max_iter,
                                   float mu, float penalty, float relax, float eps, int stop_on_codeword, uint8_t* x, float* soft,
                                   int32_t* viol, int32_t* iters, int32_t* flags, fgnn_stream_t stream) {
    const int64_t per = fgnn_ldpc_decode_lp_lds_bytes(N, M, E);
    if (per < 0) return FGNN_EUNSUPPORTED;
    if (B < 0 || B > 0x7fffffffll) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_lp: batch %lld outside 0 .. 2^31-1", (long long)B);
    if (max_iter < 1) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_lp: max_iter=%d is below 1", max_iter);
    if (!(mu > 0.0f && mu <= 3.0e38f)) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_lp: mu=%g is not a finite value > 0", mu);
    if (!(penalty >= 0.0f && penalty <= 3.0e38f)) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_lp: penalty=%g is not a finite value >= 0", penalty);
    if (!(relax >= 1.0f && relax < 2.0f)) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_lp: relax=%g outside [1, 2)", relax);
    if (!(eps >= -3.0e38f && eps <= 3.0e38f)) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_lp: eps=%g is not a finite value", eps);
    if (stop_on_codeword < 0 || stop_on_codeword > 1)
        FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_lp: stop_on_codeword=%d outside 0..1", stop_on_codeword);
    if (llr_sb < 0) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_lp: negative row stride");
    if (B == 0) return FGNN_OK;
    if (!llr || !col_ptr || !row_ptr || !row_edge || !row_var) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_lp: null input pointer");
    if (!x || !viol || !iters || !flags) FGNN_FAIL(FGNN_EINVAL, "ldpc_decode_lp: null output pointer");
    LpParams p = {};
    p.llr = llr; p.llr_sb = llr_sb;
    p.col_ptr = col_ptr; p.row_ptr = row_ptr; p.row_edge = row_edge; p.row_var = row_var;
    p.x = x; p.soft = soft; p.viol = viol; p.iters = iters; p.flags = flags;
    p.N = N; p.M = M; p.E = E; p.max_iter = max_iter; p.stop_on_codeword = stop_on_codeword;
    p.mu = mu; p.penalty = penalty; p.relax = relax; p.eps = eps;
    const int threads = ldpc_word_threads(N, M);
    fgnn_note_kernel("ldpc_lp_kernel x%d", threads);
    return fgnn_launch("ldpc_decode_lp", ldpc_lp_kernel, dim3((unsigned)B), dim3(threads), (size_t)per, fgnn_stream(stream), p);
}
